// lgcn_fusion_bwd.hip — the backward of the LightGCN_Fusion item pre-layer (lgcn_fusion.hip) for
// gfx950: from the saved output and dL/d out,
//     g    = out > 0 ? g_out : g_out * slope            (masked in registers, never stored)
//     d_id = g · W[:, :d]        d_w = gᵀ · [id | content]        d_b = Σ_i g[i, :]
// in ONE pass over the rows, both products on exact-f32 MFMA (v_mfma_f32_32x32x2_f32: bitwise an
// fmaf chain), and a two-step combine of the per-chunk weight-gradient partials. No float atomics:
// every sum has one documented order (include/lgcn.h).
//
//  * block = 4 waves (one per SIMD), persistent over chunks of LGCN_FUSION_BWD_CHUNK rows (block b
//    takes chunks b, b + grid, ...), a chunk walked in 32-row tiles. All 256 threads stage a tile
//    into LDS with 16-B loads: the masked g [32 x d] (row stride d + 1 floats: both the row reads
//    of d_w and the column reads of d_id are bank-conflict-free) and x = [id | content]
//    [32 x (d + c)]. Two LDS buffers: the next tile's global loads are in flight during the
//    current tile's MFMAs, one barrier per tile.
//  * d_w: A = gᵀ (lane (o, h) reads g[row s + 16 h][o], a row read), B = x (lane (k, h) reads
//    x[row s + 16 h][k]); step s = 0..15 of a tile consumes rows (s, s + 16). The 32 x 32 tiles of
//    d_w are split over the waves: at d = 128 wave w owns output rows [32 w, 32 w + 32) and all
//    (d + c) / 32 column tiles (96 accumulator registers at c = 64); at d = 64 wave w owns output
//    rows 32 (w & 1) and the column tiles of parity w >> 1. The accumulators live across the
//    chunk's tiles and go to the chunk's scratch slot at its end.
//  * d_b: the lane that holds g[row][o] as an A operand adds it up (VALU, idle otherwise): two
//    chains per column (rows s and rows s + 16 of every tile), added lo + hi at the chunk's end.
//  * d_id: A = g (lane (i, h) reads g[i][2 s + h], a column read), B = W[2 s + h][32 nt + lane],
//    held in d / 2 registers for the whole kernel; one 32 x 32 tile per wave (d = 128: wave w
//    column tile w; d = 64: the waves with the fewer d_w tiles), stored as in the forward.
//  * k_fusion_bwd_combine: groups of 32 consecutive chunk slots, then the group sums.
// Work: 2·I·d·d + 2·I·d·(d+C) flop (C5: 360 GFLOP, MFMA-bound); bytes: I·(3d + C)·4 read +
// I·d·4 written + the chunk partials (C5: 212 MB written and read once).
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "lgcn.h"

namespace lgcn_detail {
extern int g_fusion_bwd_blocks;  // LGCN_TUNE_FUSION_BWD_BLOCKS (lgcn_engine.hip)
}  // namespace lgcn_detail

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kWaves = 4;  // one wave per SIMD: the whole 512-register file per lane
constexpr int kThreads = kWaves * 64;
constexpr int kChunk = LGCN_FUSION_BWD_CHUNK;
constexpr int kTilesPerChunk = kChunk / 32;
constexpr int kGroup = 32;  // chunk slots per first-level group of the combine
static_assert(kChunk % 32 == 0 && (kChunk & (kChunk - 1)) == 0 && kChunk <= 8192, "chunk");

enum { kWantId = 1, kWantW = 2, kWantB = 4 };

constexpr int64_t slot_floats(int d, int c) { return (int64_t)d * (d + c) + d; }

template <int D, int K>
struct Stage {  // one tile on its way from global memory to LDS, per thread
    float4 g[D / 32], o[D / 32], x[K / 32];
};

// Addresses are a wave-uniform 64-bit base (the tile's first row, the chunk's slot) plus a 32-bit
// byte offset per lane: leading dims are at most kMaxLd floats (checked on the host), so 32 rows
// span less than 2^32 bytes. Kept this way, the compiler does not carry a 64-bit address per
// load and store across the loops.
constexpr int64_t kMaxLd = (int64_t)1 << 24;

__device__ __forceinline__ float4 ld4(const float* base, uint32_t byte_off) {
    return *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(base) + byte_off);
}
__device__ __forceinline__ void st1(float* base, uint32_t byte_off, float v) {
    *reinterpret_cast<float*>(reinterpret_cast<char*>(base) + byte_off) = v;
}

// The value, opaque to the optimiser from here on: the store offsets computed from it are formed
// where they are used (a few VALU instructions per tile or chunk), not hoisted out of both loops
// and kept in 64 registers for the whole kernel.
__device__ __forceinline__ uint32_t pin(uint32_t v) {
    asm volatile("" : "+v"(v));
    return v;
}

template <int D, int K>
__device__ __forceinline__ void load_tile(
    Stage<D, K>& st, const float* __restrict__ out, int64_t ld_out,
    const float* __restrict__ gout, int64_t ld_g, const float* __restrict__ idw, int64_t ld_id,
    const float* __restrict__ content, int64_t ld_c, int64_t row0, int32_t n, bool want_x) {
    // a row >= n reads row n - 1 instead (row0 < n) and is zeroed by store_tile: no branch per load
    const int64_t rest = (int64_t)n - 1 - row0;
    const uint32_t rmax = rest < 31 ? (uint32_t)rest : 31u;
    const float* gb = gout + row0 * ld_g;
    const float* ob = out + row0 * ld_out;
#pragma unroll
    for (int q = 0; q < D / 32; ++q) {
        const uint32_t f = threadIdx.x + kThreads * q;
        uint32_t r = f / (D / 4);
        r = r < rmax ? r : rmax;
        const uint32_t c = (f % (D / 4)) * 4;
        st.g[q] = ld4(gb, (r * (uint32_t)ld_g + c) * 4u);
        st.o[q] = ld4(ob, (r * (uint32_t)ld_out + c) * 4u);
    }
    if (want_x) {
        const float* ib = idw + row0 * ld_id;
        const float* cb = content + row0 * ld_c;
#pragma unroll
        for (int q = 0; q < K / 32; ++q) {
            const uint32_t f = threadIdx.x + kThreads * q;
            uint32_t r = f / (K / 4);
            r = r < rmax ? r : rmax;
            const uint32_t k = (f % (K / 4)) * 4;
            // [id | content]: a lane's float4 lies in one of the two tables
            if (k < D)
                st.x[q] = ld4(ib, (r * (uint32_t)ld_id + k) * 4u);
            else
                st.x[q] = ld4(cb, (r * (uint32_t)ld_c + (k - D)) * 4u);
        }
    }
}

// g = out > 0 ? g_out : g_out * slope (a zero of either sign and a NaN in out: the slope branch);
// a row >= n is +0 whatever the slope
__device__ __forceinline__ float mask_g(float o, float g, float slope, bool ok) {
    return ok ? (o > 0.f ? g : g * slope) : 0.f;
}

template <int D, int K>
__device__ __forceinline__ void store_tile(const Stage<D, K>& st, float* __restrict__ gl,
                                           float* __restrict__ xl, int64_t row0, int32_t n,
                                           float slope, bool want_x) {
    constexpr int SG = D + 1;
#pragma unroll
    for (int q = 0; q < D / 32; ++q) {
        const int f = threadIdx.x + kThreads * q;
        const int r = f / (D / 4), c = (f % (D / 4)) * 4;
        const bool ok = row0 + r < n;
        float* dst = gl + r * SG + c;
        dst[0] = mask_g(st.o[q].x, st.g[q].x, slope, ok);
        dst[1] = mask_g(st.o[q].y, st.g[q].y, slope, ok);
        dst[2] = mask_g(st.o[q].z, st.g[q].z, slope, ok);
        dst[3] = mask_g(st.o[q].w, st.g[q].w, slope, ok);
    }
    if (want_x) {
#pragma unroll
        for (int q = 0; q < K / 32; ++q) {
            const int f = threadIdx.x + kThreads * q;
            const int r = f / (K / 4);
            *reinterpret_cast<float4*>(xl + r * K + (f % (K / 4)) * 4) =
                row0 + r < n ? st.x[q] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
}

// WW: d_w is wanted (a template parameter: the accumulators then never meet a path without
// their MFMAs, and stay in their registers across the tile loop)
template <int D, int K, bool WW>
__global__ __launch_bounds__(kThreads) void k_fusion_bwd(
    const float* __restrict__ out, int64_t ld_out, const float* __restrict__ gout, int64_t ld_g,
    const float* __restrict__ idw, int64_t ld_id, const float* __restrict__ content, int64_t ld_c,
    int32_t n, const float* __restrict__ w, float slope, float* __restrict__ d_id, int64_t ld_did,
    float* __restrict__ scratch, int want) {
    constexpr int NTO = D / 32, NTK = K / 32;
    constexpr int KSPLIT = 4 / NTO;                    // waves that share one 32-row slice of d_w
    constexpr int MAXKT = (NTK + KSPLIT - 1) / KSPLIT;  // column tiles of d_w per wave, at most
    constexpr int JFULL = NTK / KSPLIT;                 // ... and those that every wave has
    constexpr int SG = D + 1, SX = K;
    constexpr int BUF = 32 * SG + 32 * SX;  // floats per LDS buffer: g tile, then x tile
    static_assert(NTO == 2 || NTO == 4, "d");
    static_assert((32 * SG) % 4 == 0 && BUF % 4 == 0, "x tile 16-B aligned");
    extern __shared__ __attribute__((aligned(16))) float lds[];

    // wave-uniform roles as scalars: the branches on them are scalar branches
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int h = lane >> 5;
    const int col = lane & 31;
    const int osl = wave % NTO;                        // this wave's 32-row slice of d_w / d_b
    const int kpart = KSPLIT == 1 ? 0 : wave / NTO;    // its share of the column tiles
    constexpr bool want_w = WW, want_x = WW;
    const bool want_b = want & kWantB;
    const bool does_b = want_b && kpart == 0;
    const bool does_id = (want & kWantId) && kpart == KSPLIT - 1;  // column tile osl of d_id

    float wreg[D / 2];  // W[2 s + h][32 osl + col]: the B operand of d_id's step s
    const float* wp = w + (h * K + osl * 32 + col);
#pragma unroll
    for (int s = 0; s < D / 2; ++s) wreg[s] = wp[2 * s * K];

    const int64_t n_chunks = ((int64_t)n + kChunk - 1) / kChunk;
    int buf = 0;
    Stage<D, K> st;
    // the launcher keeps the grid <= n_chunks: every block has a first chunk
    load_tile<D, K>(st, out, ld_out, gout, ld_g, idw, ld_id, content, ld_c,
                    (int64_t)blockIdx.x * kChunk, n, want_x);
    store_tile<D, K>(st, lds, lds + 32 * SG, (int64_t)blockIdx.x * kChunk, n, slope, want_x);
    __syncthreads();

    for (int64_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        const int64_t left = ((int64_t)n - chunk * kChunk + 31) / 32;
        const int tiles_here = left < kTilesPerChunk ? (int)left : kTilesPerChunk;
        f32x16 acc[MAXKT];
#pragma unroll
        for (int j = 0; j < MAXKT; ++j) acc[j] = f32x16{};
        float db = 0.f;
        for (int tile = 0; tile < tiles_here; ++tile) {
            const int64_t row0 = chunk * kChunk + (int64_t)tile * 32;
            // the tile after this one: the next of the chunk, or the first of the block's next
            // chunk; its rows are in flight while this tile's MFMA chains run
            const bool chunk_ends = tile + 1 == tiles_here;
            const int64_t next_row0 = chunk_ends ? (chunk + gridDim.x) * kChunk : row0 + 32;
            const bool has_next = !chunk_ends || chunk + gridDim.x < n_chunks;
            if (has_next)
                load_tile<D, K>(st, out, ld_out, gout, ld_g, idw, ld_id, content, ld_c, next_row0,
                                n, want_x);
            const float* gl = lds + buf * BUF;
            const float* xl = gl + 32 * SG;

            // d_w / d_b: step s sums rows s (h = 0) and s + 16 (h = 1) of the tile
            const float* ga = gl + (16 * h) * SG + osl * 32 + col;
            if constexpr (want_w) {
                const float* xb = xl + (16 * h) * SX + col;
#pragma unroll
                for (int s = 0; s < 16; ++s) {
                    const float a = ga[s * SG];
                    db += a;
#pragma unroll
                    for (int j = 0; j < JFULL; ++j)
                        acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(
                            a, xb[s * SX + (kpart + j * KSPLIT) * 32], acc[j], 0, 0, 0);
                    // bound the scheduler's LDS read-ahead (it would hoist every operand read)
                    if (s & 1) __builtin_amdgcn_sched_barrier(0);
                }
                if constexpr (MAXKT > JFULL) {
                    // the odd column tile (d = 64, c = 32): a chain of its own on the waves
                    // that own it, so that no branch sits between the MFMAs above
                    if (kpart < NTK % KSPLIT) {
#pragma unroll
                        for (int s = 0; s < 16; ++s)
                            acc[JFULL] = __builtin_amdgcn_mfma_f32_32x32x2f32(
                                ga[s * SG], xb[s * SX + (kpart + JFULL * KSPLIT) * 32], acc[JFULL],
                                0, 0, 0);
                    }
                }
            } else if (does_b) {
#pragma unroll
                for (int s = 0; s < 16; ++s) db += ga[s * SG];
            }
            if (does_id) {
                // d_id: step s consumes o = 2 s (h = 0) and 2 s + 1 (h = 1): o ascending from +0
                f32x16 ai = f32x16{};
                const float* gc = gl + col * SG + h;
#pragma unroll
                for (int s = 0; s < D / 2; ++s) {
                    ai = __builtin_amdgcn_mfma_f32_32x32x2f32(gc[2 * s], wreg[s], ai, 0, 0, 0);
                    if ((s & 7) == 7) __builtin_amdgcn_sched_barrier(0);
                }
                // lane holds rows (r&3) + 8(r>>2) + 4h of the tile, column osl*32 + col
                float* db0 = d_id + row0 * ld_did + osl * 32;
                const int64_t rows = (int64_t)n - row0;  // of this tile: >= 1
                const uint32_t hs = pin(h);
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const uint32_t i = (r & 3) + 8 * (r >> 2) + 4 * hs;
                    if (i < rows) st1(db0, (i * (uint32_t)ld_did + col) * 4u, ai[r]);
                }
            }
            if (has_next) {
                store_tile<D, K>(st, lds + (buf ^ 1) * BUF, lds + (buf ^ 1) * BUF + 32 * SG,
                                 next_row0, n, slope, want_x);
                __syncthreads();
                buf ^= 1;
            }
        }
        // the chunk's partials: d_w tile rows as the MFMA leaves them, d_b = lo + hi
        float* slot = scratch + chunk * slot_floats(D, K - D);
        if constexpr (want_w) {
            float* sw = slot + (osl * 32) * K + kpart * 32;
            const uint32_t hs = pin(h);
#pragma unroll
            for (int j = 0; j < MAXKT; ++j) {
                if (j < JFULL || kpart < NTK % KSPLIT) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const uint32_t o = (r & 3) + 8 * (r >> 2) + 4 * hs;
                        st1(sw, (o * K + j * KSPLIT * 32 + col) * 4u, acc[j][r]);
                    }
                }
            }
        }
        if (does_b) {
            const float hi = __shfl_xor(db, 32);
            if (h == 0) slot[D * K + osl * 32 + col] = db + hi;
        }
    }
}

// One level of the combine: thread e of group j = blockIdx.y adds element e of the slots
// (j * per_group + i) * step, i = 0, 1, ... < per_group (below n_slots), in that order from +0.
// FINAL: the sum goes to d_w / d_b; otherwise back into the group's first slot (element-wise in
// place: a thread reads and writes its own element only).
template <bool FINAL>
__global__ __launch_bounds__(256) void k_fusion_bwd_combine(
    float* __restrict__ scratch, int64_t slot, int64_t w_floats, int64_t n_slots, int64_t step,
    int64_t per_group, float* __restrict__ d_w, float* __restrict__ d_b, int want) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= slot) return;
    const bool is_w = e < w_floats;
    if (!(want & (is_w ? kWantW : kWantB))) return;  // that part of a slot was never written
    const int64_t first = (int64_t)blockIdx.y * per_group;
    int64_t last = first + per_group;
    if (last > n_slots) last = n_slots;
    const float* src = scratch + e;
    float s = 0.f;
#pragma unroll 8
    for (int64_t i = first; i < last; ++i) s += src[i * step * slot];
    if (FINAL) {
        if (is_w) d_w[e] = s; else d_b[e - w_floats] = s;
    } else {
        scratch[first * step * slot + e] = s;
    }
}

template <int D, int K>
int launch_bwd(const float* out, int64_t ld_out, const float* gout, int64_t ld_g,
               const float* idw, int64_t ld_id, const float* content, int64_t ld_c, int32_t n,
               const float* w, float slope, float* d_id, int64_t ld_did, float* d_w, float* d_b,
               float* scratch, hipStream_t s) {
    constexpr size_t lds = sizeof(float) * 2 * (32 * (D + 1) + 32 * K);
    auto kern = d_w ? k_fusion_bwd<D, K, true> : k_fusion_bwd<D, K, false>;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
    const int64_t n_chunks = ((int64_t)n + kChunk - 1) / kChunk;
    int64_t cap = lgcn_detail::g_fusion_bwd_blocks;
    if (cap <= 0) {
        int dev = 0, n_cu = 256;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
            n_cu = 256;
        cap = n_cu;  // persistent: one block (up to 96 KB of LDS, 4 waves) per CU
    }
    const int64_t grid = n_chunks < cap ? n_chunks : cap;
    const int want = (d_id ? kWantId : 0) | (d_w ? kWantW : 0) | (d_b ? kWantB : 0);
    hipLaunchKernelGGL(kern, dim3((uint32_t)grid), dim3(kThreads), lds, s, out, ld_out, gout, ld_g,
                       idw, ld_id, content, ld_c, n, w, slope, d_id, ld_did, scratch, want);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    if (!(want & (kWantW | kWantB))) return 0;
    const int64_t slot = slot_floats(D, K - D), w_floats = (int64_t)D * K;
    const uint32_t bx = (uint32_t)((slot + 255) / 256);
    const int64_t n_groups = (n_chunks + kGroup - 1) / kGroup;
    if (n_groups > 1) {
        hipLaunchKernelGGL(k_fusion_bwd_combine<false>, dim3(bx, (uint32_t)n_groups), dim3(256), 0,
                           s, scratch, slot, w_floats, n_chunks, (int64_t)1, (int64_t)kGroup, d_w,
                           d_b, want);
        if ((e = hipGetLastError()) != hipSuccess) return (int)e;
        hipLaunchKernelGGL(k_fusion_bwd_combine<true>, dim3(bx, 1), dim3(256), 0, s, scratch, slot,
                           w_floats, n_groups, (int64_t)kGroup, n_groups, d_w, d_b, want);
    } else {
        // one group: its sum is the result (the second level would add it to +0)
        hipLaunchKernelGGL(k_fusion_bwd_combine<true>, dim3(bx, 1), dim3(256), 0, s, scratch, slot,
                           w_floats, n_chunks, (int64_t)1, (int64_t)kGroup, d_w, d_b, want);
    }
    e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
inline bool shape_ok(int32_t d, int32_t c_dim) {
    return (d == 64 || d == 128) && (c_dim == 32 || c_dim == 64 || c_dim == 128);
}

}  // namespace

extern "C" {

size_t lgcn_fusion_prelayer_backward_scratch_bytes(int32_t n_items, int32_t d, int32_t c_dim) {
    if (n_items < 0 || !shape_ok(d, c_dim)) return 0;
    const int64_t n_chunks = ((int64_t)n_items + kChunk - 1) / kChunk;
    return (size_t)(n_chunks * slot_floats(d, c_dim)) * sizeof(float);
}

int lgcn_fusion_prelayer_backward(const float* out, int64_t ld_out, const float* g_out,
                                  int64_t ld_g, const float* id_emb, int64_t ld_id,
                                  const float* content, int64_t ld_c, int32_t n_items, int32_t d,
                                  int32_t c_dim, const float* weight, float slope, float* d_id,
                                  int64_t ld_did, float* d_w, float* d_b, void* scratch,
                                  size_t scratch_bytes, void* stream) {
    if (n_items < 0 || !shape_ok(d, c_dim)) return LGCN_EINVAL;
    if (ld_out < d || ld_g < d || ld_id < d || ld_c < c_dim || (d_id && ld_did < d))
        return LGCN_EINVAL;
    if (ld_out > kMaxLd || ld_g > kMaxLd || ld_id > kMaxLd || ld_c > kMaxLd ||
        (d_id && ld_did > kMaxLd))
        return LGCN_EINVAL;
    if (n_items == 0) return 0;
    if (!d_id && !d_w && !d_b) return 0;
    if (!out || !g_out || !id_emb || !content || !weight) return LGCN_EINVAL;
    if ((d_w || d_b) &&
        (!scratch ||
         scratch_bytes < lgcn_fusion_prelayer_backward_scratch_bytes(n_items, d, c_dim)))
        return LGCN_EINVAL;
    if (!al16(out) || !al16(g_out) || !al16(id_emb) || !al16(content) || !al16(d_id) ||
        ld_out % 4 || ld_g % 4 || ld_id % 4 || ld_c % 4 || (d_id && ld_did % 4))
        return LGCN_EALIGN;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
#define LGCN_F(D_, C_)                                                                         \
    if (d == D_ && c_dim == C_)                                                                \
        return launch_bwd<D_, D_ + C_>(out, ld_out, g_out, ld_g, id_emb, ld_id, content, ld_c,  \
                                       n_items, weight, slope, d_id, ld_did, d_w, d_b,         \
                                       static_cast<float*>(scratch), s);
    LGCN_F(64, 32) LGCN_F(64, 64) LGCN_F(64, 128) LGCN_F(128, 32) LGCN_F(128, 64) LGCN_F(128, 128)
#undef LGCN_F
    return LGCN_EINVAL;
}

}  // extern "C"

// lgcn_eval.hip — fused evaluation for gfx950: scores = user rows · item tableᵀ, training items
// masked to -1e10, top-K per user (the semantics of the reference's evaluate, main.py:404-439:
// matmul :420, mask loop :422-424, topk :426), without materialising the [users x items] score
// matrix (1024 x 4.4M fp32 = 18 GB per batch at Books scale).
//
//  * scores: exact-f32 MFMA v_mfma_f32_32x32x2_f32 (A = 32 users, B = 32 items, K = d): each
//    score is an ordered fmaf chain over the d features (feature order 0,32,1,33,… at d = 64);
//  * a block = 4 waves x 32 users; every wave streams the SAME item split (L1/L2 reuse), so the
//    item table is read once per 128 users; grid = user tiles x item splits;
//  * top-K: a lane keeps the current K-th best score of its 16 users in registers; only scores
//    above it are candidates (after the first few tiles, ~K·ln(items/K) per user in total): the
//    train-item mask is a binary search in the user's sorted list, done for candidates only
//    (every item is a candidate while the K-th best is below -1e10: masking raises such a score);
//    candidates go to a per-user LDS buffer (capacity 64); users whose buffer passes 32 are
//    compacted to their K best by rank counting under the total order (score desc, index asc):
//    deterministic regardless of LDS arrival order;
//  * k_topk_merge: per user, the splits' K-th scores bound the global K-th from below, so only
//    candidates >= max_s kth_s are ranked.
//
// lgcn_score_rank (further down) ranks one held-out item per user under the same total order, and
// lgcn_score_rank_lists (after it) every item of a held-out list per user from one pass over the
// user's score row: a histogram over p(x), the number of the list's targets an item does not beat.
// The entry points stand on the same pieces, each written once: load_row_half (guarded row load),
// score_tile (the one MFMA chain: every score either entry point compares comes from it), c_row
// (which user row a C register holds), and on the host eval_args, eval_split_len, user_tiles and
// with_width. The double-buffered loop over an item split stays written out in k_score_topk and
// in k_rank_count: as one template over a consumer callable, the consumer is optimised on its own
// before it is inlined, and k_rank_count's comparisons then compile to other code.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <type_traits>

#include "lgcn.h"

namespace {

#ifndef LGCN_EVAL_WAVES
#define LGCN_EVAL_WAVES 4
#endif
constexpr int kWaves = LGCN_EVAL_WAVES;  // waves (x 32 users) per block: they share item tiles
constexpr int kUsersPerWave = 32;
constexpr int kCap = 64;     // candidate buffer per user
constexpr int kCompact = 32; // compact when a buffer holds more than this (one tile adds <= 32)
constexpr float kMasked = -1e10f;
constexpr int kLgkm0 = 0xC07F;  // s_waitcnt lgkmcnt(0) only (vmcnt/expcnt left alone)

typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ bool better(float s1, int i1, float s2, int i2) {
    return s1 > s2 || (s1 == s2 && i1 < i2);
}

__device__ __forceinline__ bool in_sorted(const int32_t* __restrict__ a, int32_t lo, int32_t hi,
                                          int32_t x) {
    while (lo < hi) {
        const int32_t mid = (lo + hi) >> 1;
        const int32_t v = a[mid];
        if (v == x) return true;
        if (v < x) lo = mid + 1; else hi = mid;
    }
    return false;
}

struct WaveState {
    float score[kUsersPerWave][kCap];
    int32_t idx[kUsersPerWave][kCap];
    int32_t cnt[kUsersPerWave];
    float thr[kUsersPerWave];
    int32_t mlo[kUsersPerWave];  // the user's train items: mask_items[mlo, mhi); mhi < mlo: no user
    int32_t mhi[kUsersPerWave];
};

// Keep the K best of user u's buffer (entries at ranks >= K dropped), set its threshold.
__device__ void compact_user(WaveState& st, int u, int K, int lane) {
    const int n = st.cnt[u];
    float s0 = 0.f;
    int i0 = 0, r0 = kCap;
    static_assert(kCap <= 64, "one buffer entry per lane");
    if (lane < n) { s0 = st.score[u][lane]; i0 = st.idx[u][lane]; r0 = 0; }
    for (int m = 0; m < n; ++m) {
        const float sm = st.score[u][m];
        const int im = st.idx[u][m];
        if (lane < n && better(sm, im, s0, i0)) ++r0;
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_s_waitcnt(kLgkm0);  // every lane has read the old buffer
    __builtin_amdgcn_wave_barrier();
    if (lane < n && r0 < K) { st.score[u][r0] = s0; st.idx[u][r0] = i0; }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_s_waitcnt(kLgkm0);
    __builtin_amdgcn_wave_barrier();
    if (lane == 0) {
        const int keep = n < K ? n : K;
        st.cnt[u] = keep;
        // the candidate filter compares raw scores, and masking raises a raw score below -1e10:
        // no threshold while the K-th best is below -1e10 (every item stays a candidate)
        const float kth = keep == K ? st.score[u][K - 1] : -INFINITY;
        st.thr[u] = kth < kMasked ? -INFINITY : kth;
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_s_waitcnt(kLgkm0);
    __builtin_amdgcn_wave_barrier();
}

// Half a row (this lane half's D/2 features, starting at p) as float4s; zeros when !ok (p is then
// any valid address: nothing is read).
template <int D>
__device__ __forceinline__ void load_row_half(const float* __restrict__ p, bool ok,
                                              float4 (&v)[D / 8]) {
#pragma unroll
    for (int q = 0; q < D / 8; ++q)
        v[q] = ok ? *reinterpret_cast<const float4*>(p + 4 * q) : make_float4(0.f, 0.f, 0.f, 0.f);
}

// C[user row][item col] = the ordered fmaf chain over the features (feature order 0,32,1,33,… at
// d = 64). A score is a function of its (user row, item row) pair alone, wherever the pair sits
// in a tile.
template <int D>
__device__ __forceinline__ f32x16 score_tile(const float4 (&a)[D / 8], const float4 (&b)[D / 8]) {
    f32x16 acc = {};
#pragma unroll
    for (int q = 0; q < D / 8; ++q) {
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q].x, b[q].x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q].y, b[q].y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q].z, b[q].z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q].w, b[q].w, acc, 0, 0, 0);
    }
    return acc;
}

// Register r of the C tile in lane half h holds user row c_row(r, h) (of column lane & 31);
// row = c_row(c_reg(row), c_half(row)).
__device__ __forceinline__ int c_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }
__device__ __forceinline__ int c_reg(int row) { return (row & 3) + 4 * (row >> 3); }
__device__ __forceinline__ int c_half(int row) { return (row >> 2) & 1; }

template <int D>
__global__ __launch_bounds__(kWaves * 64) void k_score_topk(
    const float* __restrict__ uemb, int64_t ld_u, const int32_t* __restrict__ users,
    int32_t n_users, const float* __restrict__ iemb, int64_t ld_i, int32_t n_items,
    int32_t split_len, const int32_t* __restrict__ mrow, const int32_t* __restrict__ mitems, int K,
    float* __restrict__ part_s, int32_t* __restrict__ part_i) {
    constexpr int DH = D / 2;  // features per lane half
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int wave = threadIdx.x >> 6;
    const int lane = threadIdx.x & 63;
    const int h = lane >> 5;
    const int col = lane & 31;
    WaveState& st = reinterpret_cast<WaveState*>(smem)[wave];
    const int32_t ub = (blockIdx.x * kWaves + wave) * kUsersPerWave;  // first user slot
    const int32_t split = blockIdx.y;
    const int32_t it0 = split * split_len;
    const int32_t it1 = min(n_items, it0 + split_len);

    if (lane < kUsersPerWave) {
        st.cnt[lane] = 0;
        st.thr[lane] = -INFINITY;
    }
    // A operand: user (ub + col), features [h*DH, h*DH + DH)
    float4 a[D / 8];
    {
        const bool ok = ub + col < n_users;
        load_row_half<D>(uemb + (ok ? (int64_t)users[ub + col] * ld_u : 0) + h * DH, ok, a);
    }
    if (lane < kUsersPerWave) {
        const bool ok = ub + lane < n_users;
        const int32_t u = ok ? users[ub + lane] : 0;
        st.mlo[lane] = ok ? mrow[u] : 0;
        st.mhi[lane] = ok ? mrow[u + 1] : -1;
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_s_waitcnt(kLgkm0);
    __builtin_amdgcn_wave_barrier();
    // The B operand (32 items x this lane's feature half) is double-buffered: the next tile's
    // loads are in flight during the current tile's MFMA chain.
    float4 bcur[D / 8], bnxt[D / 8];
    auto load_tile = [&](int32_t t0, float4 (&b)[D / 8]) {
        const int32_t item = t0 + col;
        const bool iok = item < it1;
        load_row_half<D>(iemb + (iok ? (int64_t)item * ld_i : 0) + h * DH, iok, b);
    };
    if (it0 < it1) load_tile(it0, bcur);
    for (int32_t t0 = it0; t0 < it1; t0 += 32) {
        if (t0 + 32 < it1) load_tile(t0 + 32, bnxt);
        const int32_t item = t0 + col;
        const bool iok = item < it1;
        const f32x16 acc = score_tile<D>(a, bcur);
        bool any = false;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = c_row(r, h);
            float sc = acc[r];
            const float thr = st.thr[row];
            if (iok && sc > thr) {
                const int32_t lo = st.mlo[row], hi = st.mhi[row];
                if (hi >= lo) {
                    if (in_sorted(mitems, lo, hi, item)) sc = kMasked;  // main.py:422-424
                    if (sc > thr) {
                        const int pos = atomicAdd(&st.cnt[row], 1);
                        st.score[row][pos] = sc;
                        st.idx[row][pos] = item;
                        any = true;
                    }
                }
            }
        }
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_s_waitcnt(kLgkm0);
        __builtin_amdgcn_wave_barrier();
        if (__any(any)) {
            // compact every user whose buffer could overflow on the next tile
            uint64_t need = __ballot(lane < kUsersPerWave && st.cnt[lane] > kCompact);
            while (need) {
                const int u = __builtin_ctzll(need);
                need &= need - 1;
                compact_user(st, u, K, lane);
            }
        }
#pragma unroll
        for (int q = 0; q < D / 8; ++q) bcur[q] = bnxt[q];
    }
    // final: every buffer to its K best in rank order, written to this split's partial list
    for (int u = 0; u < kUsersPerWave; ++u) {
        if (ub + u >= n_users) break;
        compact_user(st, u, K, lane);
        const int n = st.cnt[u];
        if (lane < K) {
            const int64_t o = ((int64_t)split * n_users + ub + u) * K + lane;
            part_s[o] = lane < n ? st.score[u][lane] : -INFINITY;
            part_i[o] = lane < n ? st.idx[u][lane] : -1;
        }
    }
}

// One wave per user: merge the splits' K-best lists. The global K-th score is >= every split's
// K-th score, so only candidates >= max_s kth_s are ranked (always >= K of them exist).
__global__ __launch_bounds__(64) void k_topk_merge(const float* __restrict__ part_s,
                                                   const int32_t* __restrict__ part_i,
                                                   int32_t n_users, int32_t n_splits, int K,
                                                   float* __restrict__ top_s,
                                                   int32_t* __restrict__ top_i) {
    extern __shared__ __attribute__((aligned(16))) char msm[];  // n_splits*K (score, idx) pairs
    float* cs = reinterpret_cast<float*>(msm);
    int32_t* ci = reinterpret_cast<int32_t*>(msm) + n_splits * K;
    __shared__ int ncand;
    const int u = blockIdx.x;
    const int lane = threadIdx.x;
    float t = -INFINITY;
    for (int s = lane; s < n_splits; s += 64) {
        const float v = part_s[((int64_t)s * n_users + u) * K + K - 1];
        t = fmaxf(t, v);
    }
    for (int off = 32; off > 0; off >>= 1) t = fmaxf(t, __shfl_xor(t, off));
    if (lane == 0) ncand = 0;
    __syncthreads();
    const int total = n_splits * K;
    for (int e = lane; e < total; e += 64) {
        const int s = e / K, j = e - s * K;
        const int64_t o = ((int64_t)s * n_users + u) * K + j;
        const float v = part_s[o];
        const int32_t id = part_i[o];
        if (id >= 0 && v >= t) {
            const int p = atomicAdd(&ncand, 1);
            cs[p] = v;
            ci[p] = id;
        }
    }
    __syncthreads();
    const int n = ncand;
    for (int e = lane; e < n; e += 64) {
        int rank = 0;
        for (int m = 0; m < n; ++m) rank += better(cs[m], ci[m], cs[e], ci[e]) ? 1 : 0;
        if (rank < K) {
            top_s[(int64_t)u * K + rank] = cs[e];
            top_i[(int64_t)u * K + rank] = ci[e];
        }
    }
    for (int r = n + lane; r < K; r += 64) {  // fewer than K items in total
        top_s[(int64_t)u * K + r] = -INFINITY;
        top_i[(int64_t)u * K + r] = -1;
    }
}

// ---------------------------------------------------------------------------------------------
// lgcn_score_rank: the rank of one held-out item per user under the same total order, with no
// top-K selection. Every score that enters a comparison comes from score_tile, as k_score_topk's
// do, so one score table explains every rank and every list.
//  1. k_rank_target: per 32 slots a gathered tile (column c = the target of slot c); its diagonal
//     is score(slot, target). A train item as target scores -1e10. -> target_score
//  2. k_rank_count: k_score_topk's tile loop without WaveState: per (lane, C-row) an integer
//     count of raw scores that beat the target's, summed over the 32 columns -> part[split][slot]
//  3. k_rank_finish: one wave per slot sums the parts and corrects them for the user's train
//     items (32 per gathered tile): minus what the raw score counted, plus what -1e10 counts.
// ---------------------------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(kWaves * 64) void k_rank_target(
    const float* __restrict__ uemb, int64_t ld_u, const int32_t* __restrict__ users,
    int32_t n_users, const float* __restrict__ iemb, int64_t ld_i, int32_t n_items,
    const int32_t* __restrict__ mrow, const int32_t* __restrict__ mitems,
    const int32_t* __restrict__ targets, float* __restrict__ target_score) {
    constexpr int DH = D / 2;
    const int wave = threadIdx.x >> 6;
    const int lane = threadIdx.x & 63;
    const int h = lane >> 5;
    const int col = lane & 31;
    const int32_t slot = (blockIdx.x * kWaves + wave) * kUsersPerWave + col;
    const bool ok = slot < n_users;
    const int32_t u = ok ? users[slot] : 0;
    const int32_t t = ok ? targets[slot] : -1;
    const bool tok = t >= 0 && t < n_items;
    float4 a[D / 8], b[D / 8];
    load_row_half<D>(uemb + (int64_t)u * ld_u + h * DH, ok, a);
    load_row_half<D>(iemb + (tok ? (int64_t)t * ld_i : 0) + h * DH, tok, b);
    const f32x16 acc = score_tile<D>(a, b);
    // the diagonal: row col of column col
    const int rd = c_reg(col);
    float sc = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) sc = r == rd ? acc[r] : sc;
    if (ok && h == c_half(col)) {
        if (!tok) sc = __builtin_nanf("");
        else if (in_sorted(mitems, mrow[u], mrow[u + 1], t)) sc = kMasked;
        target_score[slot] = sc;
    }
}

template <int D>
__global__ __launch_bounds__(kWaves * 64, D <= 64 ? 3 : 1) void k_rank_count(
    const float* __restrict__ uemb, int64_t ld_u, const int32_t* __restrict__ users,
    int32_t n_users, const float* __restrict__ iemb, int64_t ld_i, int32_t n_items,
    int32_t split_len, const int32_t* __restrict__ targets,
    const float* __restrict__ target_score, int32_t* __restrict__ part) {
    constexpr int DH = D / 2;
    __shared__ __attribute__((aligned(16))) float s_ts[kWaves][kUsersPerWave];
    __shared__ __attribute__((aligned(16))) int32_t s_tg[kWaves][kUsersPerWave];
    const int wave = threadIdx.x >> 6;
    const int lane = threadIdx.x & 63;
    const int h = lane >> 5;
    const int col = lane & 31;
    const int32_t ub = (blockIdx.x * kWaves + wave) * kUsersPerWave;
    const int32_t split = blockIdx.y;
    const int32_t it0 = split * split_len;
    const int32_t it1 = min(n_items, it0 + split_len);
    const bool ok = ub + col < n_users;
    if (h == 0) {  // a slot past the batch compares against NaN: it counts nothing
        s_ts[wave][col] = ok ? target_score[ub + col] : __builtin_nanf("");
        s_tg[wave][col] = ok ? targets[ub + col] : -1;
    }
    float4 a[D / 8];
    load_row_half<D>(uemb + (ok ? (int64_t)users[ub + col] * ld_u : 0) + h * DH, ok, a);
    __syncthreads();
    // (the targets' scores and indices sit in LDS, as k_score_topk's thresholds do: under the
    // launch bounds the compiler keeps them there or in registers, whichever fits 3 waves per
    // SIMD at d <= 64)
    int32_t cnt[16] = {};
    float4 bcur[D / 8], bnxt[D / 8];
    auto load_tile = [&](int32_t t0, float4 (&b)[D / 8]) {
        const int32_t item = t0 + col;
        const bool iok = item < it1;
        load_row_half<D>(iemb + (iok ? (int64_t)item * ld_i : 0) + h * DH, iok, b);
    };
    if (it0 < it1) load_tile(it0, bcur);
    for (int32_t t0 = it0; t0 < it1; t0 += 32) {
        if (t0 + 32 < it1) load_tile(t0 + 32, bnxt);
        const int32_t item = t0 + col;
        const bool iok = item < it1;
        const f32x16 acc = score_tile<D>(a, bcur);
#pragma unroll
        for (int g = 0; g < 4; ++g) {  // rows c_row(4g .. 4g+3, h) are four neighbours in LDS
            const float4 ts = *reinterpret_cast<const float4*>(&s_ts[wave][c_row(4 * g, h)]);
            const int4 tg = *reinterpret_cast<const int4*>(&s_tg[wave][c_row(4 * g, h)]);
            cnt[4 * g] += (iok && item != tg.x && better(acc[4 * g], item, ts.x, tg.x)) ? 1 : 0;
            cnt[4 * g + 1] +=
                (iok && item != tg.y && better(acc[4 * g + 1], item, ts.y, tg.y)) ? 1 : 0;
            cnt[4 * g + 2] +=
                (iok && item != tg.z && better(acc[4 * g + 2], item, ts.z, tg.z)) ? 1 : 0;
            cnt[4 * g + 3] +=
                (iok && item != tg.w && better(acc[4 * g + 3], item, ts.w, tg.w)) ? 1 : 0;
        }
#pragma unroll
        for (int q = 0; q < D / 8; ++q) bcur[q] = bnxt[q];
    }
    // the 32 columns of a row live in the 32 lanes of this half
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        int c = cnt[r];
#pragma unroll
        for (int off = 16; off > 0; off >>= 1) c += __shfl_xor(c, off);
        const int row = c_row(r, h);
        if (col == 0 && ub + row < n_users) part[(int64_t)split * n_users + ub + row] = c;
    }
}

template <int D>
__global__ __launch_bounds__(64) void k_rank_finish(
    const float* __restrict__ uemb, int64_t ld_u, const int32_t* __restrict__ users,
    int32_t n_users, const float* __restrict__ iemb, int64_t ld_i, int32_t n_items,
    const int32_t* __restrict__ mrow, const int32_t* __restrict__ mitems,
    const int32_t* __restrict__ targets, const float* __restrict__ target_score,
    const int32_t* __restrict__ part, int32_t n_splits, int32_t* __restrict__ rank) {
    constexpr int DH = D / 2;
    const int32_t slot = blockIdx.x;
    const int lane = threadIdx.x;
    const int h = lane >> 5;
    const int col = lane & 31;
    const int32_t t = targets[slot];
    if (t < 0 || t >= n_items) {  // (uniform over the wave)
        if (lane == 0) rank[slot] = -1;
        return;
    }
    const int32_t u = users[slot];
    const float ts = target_score[slot];
    int32_t c = 0;
    for (int32_t s = lane; s < n_splits; s += 64) c += part[(int64_t)s * n_users + slot];
    const int32_t lo = mrow[u], hi = mrow[u + 1];
    if (lo < hi) {
        float4 a[D / 8], b[D / 8];
        load_row_half<D>(uemb + (int64_t)u * ld_u + h * DH, true, a);  // every row: this user
        for (int32_t e0 = lo; e0 < hi; e0 += 32) {
            const int32_t e = e0 + col;
            const int32_t m = e < hi ? mitems[e] : -1;
            // (an entry outside the table masks nothing; a repeated entry masks once)
            const bool mok = m >= 0 && m < n_items && !(e > lo && mitems[e - 1] == m);
            load_row_half<D>(iemb + (mok ? (int64_t)m * ld_i : 0) + h * DH, mok, b);
            const f32x16 acc = score_tile<D>(a, b);
            if (h == 0 && mok && m != t)
                c += (better(kMasked, m, ts, t) ? 1 : 0) - (better(acc[0], m, ts, t) ? 1 : 0);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off);
    if (lane == 0) rank[slot] = c;
}

// ---------------------------------------------------------------------------------------------
// lgcn_score_rank_lists: the ranks of all the held-out items of a slot's list from ONE pass over
// the slot's score row. Sort the list's targets under the total order, t_0 > t_1 > ... > t_{T-1}
// (ties of (score, item), a target listed twice, by entry index). An item x beats exactly the
// suffix {t_j : j >= p(x)}, p(x) = #{j : x does not beat t_j} (x itself among them), so a
// histogram hist[p] over the items gives every rank: rank(t_j) = sum_{p <= j} hist[p]. The counts
// are integers: no order of the atomics changes them.
//  1. k_lists_target: one wave per slot, the gathered tile of k_rank_finish (every row the slot's
//     user, column c the c-th target of the list) -> target_score; rank -1 for a target outside.
//  2. k_lists_sort: one wave per slot places the list's entries by rank counting -> sorted
//     (score, item, entry) and the number of ranked entries in scratch.
//  3. k_lists_count: k_rank_count's tile loop. Per C-row the worst target of the list sits where
//     k_rank_count keeps its one target: a score that does not beat it costs that one compare.
//     One that does is placed by binary search in the sorted list (LDS) and counted in hist[p]
//     (LDS, integer atomic) -> part[split][sorted place]. kListCap sorted places per slot fit
//     one pass; a wave whose longest list is longer streams its split once per kListCap places
//     (a chunk of the sorted list is ranked on its own: a rank depends on its own target only).
//  4. k_lists_finish: one wave per slot sums the splits, a prefix sum per chunk gives the raw
//     ranks, the train items' correction is k_rank_finish's with the same p(.): for each train
//     item, out where its raw score was counted, in where -1e10 is.
// kListCap = 32: per block 128 slots x 32 places x (score, item, count) = 48 KB of LDS, the most
// that still lets three blocks share a CU's 160 KB, which is k_rank_count's occupancy at d <= 64
// (64 places would leave one block per CU).
// ---------------------------------------------------------------------------------------------
constexpr int kListCap = 32;
static_assert(kListCap == kUsersPerWave, "a chunk is one lane half: loads, write-out and the scan");

// The first j in [0, n) whose target (ts[j], tg[j]) the item (s, x) beats; n when it beats none.
// The lists are sorted best first, so the answer is p(x).
__device__ __forceinline__ int list_place(const float* ts, const int32_t* tg, int n, float s,
                                          int32_t x) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (better(s, x, ts[mid], tg[mid])) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// The slot's entries [lo, hi) of the window that starts at trow[0]; false when they do not lie
// inside the cap_n entries the scratch was sized for (such a slot is left alone).
__device__ __forceinline__ bool list_range(const int32_t* __restrict__ trow, int32_t slot,
                                           int64_t cap_n, int32_t& lo, int32_t& hi,
                                           int32_t& base) {
    base = trow[0];
    lo = trow[slot];
    hi = trow[slot + 1];
    return lo >= base && hi >= lo && (int64_t)hi - base <= cap_n;
}

template <int D>
__global__ __launch_bounds__(64) void k_lists_target(
    const float* __restrict__ uemb, int64_t ld_u, const int32_t* __restrict__ users,
    const float* __restrict__ iemb, int64_t ld_i, int32_t n_items,
    const int32_t* __restrict__ mrow, const int32_t* __restrict__ mitems,
    const int32_t* __restrict__ trow, const int32_t* __restrict__ titems, int64_t cap_n,
    float* __restrict__ target_score, int32_t* __restrict__ rank) {
    constexpr int DH = D / 2;
    const int32_t slot = blockIdx.x;
    const int lane = threadIdx.x;
    const int h = lane >> 5;
    const int col = lane & 31;
    int32_t lo, hi, base;
    if (!list_range(trow, slot, cap_n, lo, hi, base) || lo == hi) return;  // (uniform)
    const int32_t u = users[slot];
    const int32_t mlo = mrow[u], mhi = mrow[u + 1];
    float4 a[D / 8], b[D / 8];
    load_row_half<D>(uemb + (int64_t)u * ld_u + h * DH, true, a);  // every row: this user
    for (int32_t e0 = lo; e0 < hi; e0 += 32) {
        const int32_t e = e0 + col;
        const int32_t t = e < hi ? titems[e] : -1;
        const bool tok = t >= 0 && t < n_items;
        load_row_half<D>(iemb + (tok ? (int64_t)t * ld_i : 0) + h * DH, tok, b);
        const f32x16 acc = score_tile<D>(a, b);
        if (h == 0 && e < hi) {
            float sc = acc[0];
            if (!tok) {
                sc = __builtin_nanf("");
                rank[e] = -1;
            } else if (in_sorted(mitems, mlo, mhi, t)) {
                sc = kMasked;
            }
            target_score[e] = sc;
        }
    }
}

__global__ __launch_bounds__(64) void k_lists_sort(
    const int32_t* __restrict__ trow, const int32_t* __restrict__ titems, int32_t n_items,
    const float* __restrict__ target_score, int64_t cap_n, int32_t* __restrict__ cnt,
    float* __restrict__ sorted_s, int32_t* __restrict__ sorted_t, int32_t* __restrict__ sorted_e,
    int32_t* __restrict__ rank) {
    const int32_t slot = blockIdx.x;
    const int lane = threadIdx.x;
    int32_t lo, hi, base;
    if (!list_range(trow, slot, cap_n, lo, hi, base)) {  // (uniform)
        if (lane == 0) cnt[slot] = 0;
        return;
    }
    const int32_t T = hi - lo, rb = lo - base;
    int32_t nv = 0;
    for (int32_t i = lane; i < T; i += 64) {
        const float s = target_score[lo + i];
        const int32_t t = titems[lo + i];
        const bool tok = t >= 0 && t < n_items;
        // a score that is a NaN beats nothing and nothing beats it: rank 0, as lgcn_score_rank's
        if (tok && s != s) rank[lo + i] = 0;
        if (!tok || s != s) continue;
        int32_t pos = 0;
        for (int32_t k = 0; k < T; ++k) {
            const float sk = target_score[lo + k];
            const int32_t tk = titems[lo + k];
            const bool ahead = better(sk, tk, s, t) || (sk == s && tk == t && k < i);
            pos += (tk >= 0 && tk < n_items && ahead) ? 1 : 0;  // (a NaN sk is never ahead)
        }
        sorted_s[rb + pos] = s;
        sorted_t[rb + pos] = t;
        sorted_e[rb + pos] = lo + i;
        ++nv;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) nv += __shfl_xor(nv, off);
    if (lane == 0) cnt[slot] = nv;
}

template <int D>
__global__ __launch_bounds__(kWaves * 64, D <= 64 ? 3 : 1) void k_lists_count(
    const float* __restrict__ uemb, int64_t ld_u, const int32_t* __restrict__ users,
    int32_t n_users, const float* __restrict__ iemb, int64_t ld_i, int32_t n_items,
    int32_t split_len, const int32_t* __restrict__ trow, const int32_t* __restrict__ cnt,
    const float* __restrict__ sorted_s, const int32_t* __restrict__ sorted_t, int64_t cap_n,
    int32_t* __restrict__ part) {
    constexpr int DH = D / 2;
    __shared__ float s_ts[kWaves][kUsersPerWave][kListCap];      // this chunk of the sorted lists
    __shared__ int32_t s_tg[kWaves][kUsersPerWave][kListCap];
    __shared__ int32_t s_hist[kWaves][kUsersPerWave][kListCap];
    __shared__ __attribute__((aligned(16))) float s_ws[kWaves][kUsersPerWave];  // its worst target
    __shared__ __attribute__((aligned(16))) int32_t s_wg[kWaves][kUsersPerWave];
    __shared__ int32_t s_len[kWaves][kUsersPerWave];
    const int wave = threadIdx.x >> 6;
    const int lane = threadIdx.x & 63;
    const int h = lane >> 5;
    const int col = lane & 31;
    const int32_t ub = (blockIdx.x * kWaves + wave) * kUsersPerWave;
    const int32_t split = blockIdx.y;
    const int32_t it0 = split * split_len;
    const int32_t it1 = min(n_items, it0 + split_len);
    const bool ok = ub + col < n_users;
    // slot ub + col (both lane halves hold it): its ranked entries and where its sorted list starts
    const int32_t my_T = ok ? cnt[ub + col] : 0;
    const int32_t my_rb = ok ? trow[ub + col] - trow[0] : 0;
    int32_t max_T = my_T;
#pragma unroll
    for (int off = 16; off > 0; off >>= 1) max_T = max(max_T, __shfl_xor(max_T, off));
    float4 a[D / 8];
    load_row_half<D>(uemb + (ok ? (int64_t)users[ub + col] * ld_u : 0) + h * DH, ok, a);
    float4 bcur[D / 8], bnxt[D / 8];
    auto load_tile = [&](int32_t t0, float4 (&b)[D / 8]) {
        const int32_t item = t0 + col;
        const bool iok = item < it1;
        load_row_half<D>(iemb + (iok ? (int64_t)item * ld_i : 0) + h * DH, iok, b);
    };
    for (int32_t c0 = 0; c0 < max_T; c0 += kListCap) {  // (uniform over the wave)
        // places [c0, c0 + kListCap) of every slot's sorted list; a slot with none left compares
        // against NaN: it counts nothing
#pragma unroll 1
        for (int i = 0; i < kUsersPerWave / 2; ++i) {
            const int row = 2 * i + h;
            const int32_t len = min(max(__shfl(my_T, row) - c0, 0), kListCap);
            const int32_t src = __shfl(my_rb, row) + c0 + col;
            s_hist[wave][row][col] = 0;
            if (col < len) {
                s_ts[wave][row][col] = sorted_s[src];
                s_tg[wave][row][col] = sorted_t[src];
            }
        }
        if (h == 0) {
            const int32_t len = min(max(my_T - c0, 0), kListCap);
            s_len[wave][col] = len;
            s_ws[wave][col] = len > 0 ? sorted_s[my_rb + c0 + len - 1] : __builtin_nanf("");
            s_wg[wave][col] = len > 0 ? sorted_t[my_rb + c0 + len - 1] : -1;
        }
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_s_waitcnt(kLgkm0);
        __builtin_amdgcn_wave_barrier();
        if (it0 < it1) load_tile(it0, bcur);
        for (int32_t t0 = it0; t0 < it1; t0 += 32) {
            if (t0 + 32 < it1) load_tile(t0 + 32, bnxt);
            const int32_t item = t0 + col;
            const bool iok = item < it1;
            const f32x16 acc = score_tile<D>(a, bcur);
#pragma unroll
            for (int g = 0; g < 4; ++g) {  // rows c_row(4g .. 4g+3, h) are four neighbours in LDS
                const float4 ws = *reinterpret_cast<const float4*>(&s_ws[wave][c_row(4 * g, h)]);
                const int4 wg = *reinterpret_cast<const int4*>(&s_wg[wave][c_row(4 * g, h)]);
                const float wsq[4] = {ws.x, ws.y, ws.z, ws.w};
                const int32_t wgq[4] = {wg.x, wg.y, wg.z, wg.w};
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int r = 4 * g + q;
                    if (iok && better(acc[r], item, wsq[q], wgq[q])) {
                        const int row = c_row(r, h);
                        // (it beats the last place: the search is over the places before it)
                        const int p = list_place(s_ts[wave][row], s_tg[wave][row],
                                                 s_len[wave][row] - 1, acc[r], item);
                        atomicAdd(&s_hist[wave][row][p], 1);
                    }
                }
            }
#pragma unroll
            for (int q = 0; q < D / 8; ++q) bcur[q] = bnxt[q];
        }
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_s_waitcnt(kLgkm0);
        __builtin_amdgcn_wave_barrier();
#pragma unroll 1
        for (int i = 0; i < kUsersPerWave / 2; ++i) {
            const int row = 2 * i + h;
            const int32_t dst = __shfl(my_rb, row) + c0 + col;
            if (col < s_len[wave][row]) part[(int64_t)split * cap_n + dst] = s_hist[wave][row][col];
        }
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_s_waitcnt(kLgkm0);  // every lane has read the chunk before the next
        __builtin_amdgcn_wave_barrier();
    }
}

template <int D>
__global__ __launch_bounds__(64) void k_lists_finish(
    const float* __restrict__ uemb, int64_t ld_u, const int32_t* __restrict__ users,
    const float* __restrict__ iemb, int64_t ld_i, int32_t n_items,
    const int32_t* __restrict__ mrow, const int32_t* __restrict__ mitems,
    const int32_t* __restrict__ trow, const int32_t* __restrict__ cnt,
    const float* __restrict__ sorted_s, const int32_t* __restrict__ sorted_t,
    const int32_t* __restrict__ sorted_e, int64_t cap_n, const int32_t* __restrict__ part,
    int32_t n_splits, int32_t* __restrict__ rank) {
    constexpr int DH = D / 2;
    const int32_t slot = blockIdx.x;
    const int lane = threadIdx.x;
    const int h = lane >> 5;
    const int col = lane & 31;
    const int32_t T = cnt[slot];
    if (T == 0) return;  // (uniform; a slot outside the scratch has no ranked entry either)
    const int32_t rb = trow[slot] - trow[0];
    const int32_t u = users[slot];
    const int32_t lo = mrow[u], hi = mrow[u + 1];
    const float* ss = sorted_s + rb;
    const int32_t* st = sorted_t + rb;
    float4 a[D / 8], b[D / 8];
    if (lo < hi) load_row_half<D>(uemb + (int64_t)u * ld_u + h * DH, true, a);
    for (int32_t j0 = 0; j0 < T; j0 += 64) {  // two chunks of the sorted list, one per lane half
        const int32_t j = j0 + lane;
        int32_t c = 0;
        if (j < T)
            for (int32_t s = 0; s < n_splits; ++s) c += part[(int64_t)s * cap_n + rb + j];
        // hist -> rank within the chunk: an inclusive prefix sum over the lane half
#pragma unroll
        for (int off = 1; off < kListCap; off <<= 1) {
            const int32_t v = __shfl_up(c, off, kListCap);
            if (col >= off) c += v;
        }
        for (int32_t e0 = lo; e0 < hi; e0 += 32) {
            const int32_t e = e0 + col;
            const int32_t m = e < hi ? mitems[e] : -1;
            // (an entry outside the table masks nothing; a repeated entry masks once)
            const bool mok = m >= 0 && m < n_items && !(e > lo && mitems[e - 1] == m);
            load_row_half<D>(iemb + (mok ? (int64_t)m * ld_i : 0) + h * DH, mok, b);
            const f32x16 acc = score_tile<D>(a, b);
            int32_t p_raw = INT32_MAX, p_msk = INT32_MAX;
            if (h == 0 && mok) {
                p_raw = list_place(ss, st, T, acc[0], m);
                p_msk = list_place(ss, st, T, kMasked, m);
            }
            for (int k = 0; k < 32; ++k)  // train item k of this tile: out at p_raw, in at p_msk
                c += (__shfl(p_msk, k) <= j ? 1 : 0) - (__shfl(p_raw, k) <= j ? 1 : 0);
        }
        if (j < T) rank[sorted_e[rb + j]] = c;
    }
}

// ---- host side ----
constexpr int64_t user_tiles(int64_t n_users) {  // blocks of kWaves x 32 user slots
    return (n_users + kWaves * kUsersPerWave - 1) / (kWaves * kUsersPerWave);
}

// Items per split: ceil(n_items / n_splits) rounded up to whole 32-item tiles, never zero.
int32_t eval_split_len(int32_t n_items, int32_t n_splits) {
    const int32_t len = (int32_t)(((int64_t)n_items + n_splits - 1) / n_splits);
    return len == 0 ? 32 : ((len + 31) / 32) * 32;
}

// What both entry points ask of their common arguments.
int eval_args(const float* user_emb, int64_t ld_u, int32_t n_users, const float* item_emb,
              int64_t ld_i, int32_t n_items, int32_t d, int32_t n_splits) {
    if (n_users < 0 || n_items < 0 || n_splits < 1 || n_splits > 256) return LGCN_EINVAL;
    if (d != 32 && d != 64 && d != 128 && d != 256) return LGCN_EINVAL;
    if (ld_u % 4 || ld_i % 4 || (reinterpret_cast<uintptr_t>(user_emb) & 15) ||
        (reinterpret_cast<uintptr_t>(item_emb) & 15))
        return LGCN_EALIGN;
    return 0;
}

// f(std::integral_constant<int, D>{}) for the width d (one eval_args accepted).
template <class F>
hipError_t with_width(int32_t d, F&& f) {
    switch (d) {
        case 32: return f(std::integral_constant<int, 32>{});
        case 64: return f(std::integral_constant<int, 64>{});
        case 128: return f(std::integral_constant<int, 128>{});
        default: return f(std::integral_constant<int, 256>{});
    }
}

// Scratch of lgcn_score_rank_lists for n entries: cnt [n_users] | sorted score, item, entry [n]
// each | part [n_splits x n].
constexpr size_t lists_bytes(int64_t n_users, int64_t n, int64_t n_splits) {
    return ((size_t)4 * n_users + (size_t)(12 + 4 * n_splits) * n + 15) / 16 * 16;
}

}  // namespace

extern "C" {

int lgcn_eval_splits(int32_t n_users, int32_t n_items, int32_t n_cu) {
    // enough (user tile x split) blocks for ~2 per CU, splits of >= 2048 items, <= 256 splits
    // (no users count as one tile: the answer never grows with n_users)
    int64_t tiles = user_tiles(n_users);
    if (tiles < 1) tiles = 1;
    int64_t s = (2LL * (n_cu > 0 ? n_cu : 256) + tiles - 1) / tiles;
    const int64_t max_by_len = ((int64_t)n_items + 2047) / 2048;
    if (s > max_by_len) s = max_by_len;
    if (s > 256) s = 256;
    if (s < 1) s = 1;
    return (int)s;
}

int lgcn_score_topk(const float* user_emb, int64_t ld_u, const int32_t* users, int32_t n_users,
                    const float* item_emb, int64_t ld_i, int32_t n_items, int32_t d,
                    const int32_t* mask_rowptr, const int32_t* mask_items, int32_t k,
                    int32_t n_splits, float* part_scores, int32_t* part_idx, float* top_scores,
                    int32_t* top_idx, void* stream) {
    if (k < 1 || k > kCompact) return LGCN_EINVAL;
    if (const int rc = eval_args(user_emb, ld_u, n_users, item_emb, ld_i, n_items, d, n_splits))
        return rc;
    if (n_users == 0) return 0;
    if (!user_emb || !users || !item_emb || !mask_rowptr || !part_scores || !part_idx ||
        !top_scores || !top_idx)
        return LGCN_EINVAL;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int32_t split_len = eval_split_len(n_items, n_splits);
    const dim3 grid(user_tiles(n_users), n_splits);
    const size_t lds = sizeof(WaveState) * kWaves;
    hipError_t e = with_width(d, [&](auto width) {
        constexpr int D = decltype(width)::value;
        const hipError_t ea =
            hipFuncSetAttribute(reinterpret_cast<const void*>(k_score_topk<D>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (ea != hipSuccess) return ea;
        hipLaunchKernelGGL(k_score_topk<D>, grid, dim3(kWaves * 64), lds, s, user_emb, ld_u, users,
                           n_users, item_emb, ld_i, n_items, split_len, mask_rowptr, mask_items, k,
                           part_scores, part_idx);
        return hipGetLastError();
    });
    if (e != hipSuccess) return (int)e;
    const size_t mlds = (size_t)n_splits * k * 8;
    hipLaunchKernelGGL(k_topk_merge, dim3(n_users), dim3(64), mlds, s, part_scores, part_idx,
                       n_users, n_splits, k, top_scores, top_idx);
    e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}

int lgcn_score_rank(const float* user_emb, int64_t ld_u, const int32_t* users, int32_t n_users,
                    const float* item_emb, int64_t ld_i, int32_t n_items, int32_t d,
                    const int32_t* mask_rowptr, const int32_t* mask_items,
                    const int32_t* targets, int32_t n_splits, int32_t* part, float* target_score,
                    int32_t* rank, void* stream) {
    if (const int rc = eval_args(user_emb, ld_u, n_users, item_emb, ld_i, n_items, d, n_splits))
        return rc;
    if (n_users == 0) return 0;
    if (!user_emb || !users || !item_emb || !mask_rowptr || !targets || !part || !target_score ||
        !rank)
        return LGCN_EINVAL;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int32_t split_len = eval_split_len(n_items, n_splits);
    const int32_t tiles = user_tiles(n_users);
    const hipError_t e = with_width(d, [&](auto width) {
        constexpr int D = decltype(width)::value;
        hipLaunchKernelGGL(k_rank_target<D>, dim3(tiles), dim3(kWaves * 64), 0, s, user_emb, ld_u,
                           users, n_users, item_emb, ld_i, n_items, mask_rowptr, mask_items,
                           targets, target_score);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_rank_count<D>, dim3(tiles, n_splits), dim3(kWaves * 64), 0, s,
                           user_emb, ld_u, users, n_users, item_emb, ld_i, n_items, split_len,
                           targets, target_score, part);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        hipLaunchKernelGGL(k_rank_finish<D>, dim3(n_users), dim3(64), 0, s, user_emb, ld_u, users,
                           n_users, item_emb, ld_i, n_items, mask_rowptr, mask_items, targets,
                           target_score, part, n_splits, rank);
        return hipGetLastError();
    });
    return e == hipSuccess ? 0 : (int)e;
}

size_t lgcn_score_rank_lists_scratch_bytes(int32_t n_users, int64_t n_targets, int32_t n_splits) {
    if (n_users < 0 || n_targets < 0 || n_splits < 1 || n_splits > 256) return 0;
    return lists_bytes(n_users, n_targets, n_splits);
}

int lgcn_score_rank_lists(const float* user_emb, int64_t ld_u, const int32_t* users,
                          int32_t n_users, const float* item_emb, int64_t ld_i,
                          int32_t n_items, int32_t d,
                          const int32_t* mask_rowptr, const int32_t* mask_items,
                          const int32_t* target_rowptr, const int32_t* target_items,
                          int32_t n_splits, void* scratch, size_t scratch_bytes,
                          float* target_score, int32_t* rank, void* stream) {
    if (const int rc = eval_args(user_emb, ld_u, n_users, item_emb, ld_i, n_items, d, n_splits))
        return rc;
    if (n_users == 0) return 0;
    if (!user_emb || !users || !item_emb || !mask_rowptr || !target_rowptr || !target_items ||
        !scratch || !target_score || !rank)
        return LGCN_EINVAL;
    if (scratch_bytes < lists_bytes(n_users, 0, n_splits)) return LGCN_EINVAL;
    if (reinterpret_cast<uintptr_t>(scratch) & 3) return LGCN_EALIGN;
    // the entries the scratch holds (the host never reads target_rowptr: the kernels leave a slot
    // whose entries lie past them alone)
    const int64_t cap_n =
        (int64_t)((scratch_bytes - (size_t)4 * n_users) / (size_t)(12 + 4 * n_splits));
    int32_t* cnt = static_cast<int32_t*>(scratch);
    float* sorted_s = reinterpret_cast<float*>(cnt + n_users);
    int32_t* sorted_t = reinterpret_cast<int32_t*>(sorted_s + cap_n);
    int32_t* sorted_e = sorted_t + cap_n;
    int32_t* part = sorted_e + cap_n;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int32_t split_len = eval_split_len(n_items, n_splits);
    const int32_t tiles = user_tiles(n_users);
    const hipError_t e = with_width(d, [&](auto width) {
        constexpr int D = decltype(width)::value;
        hipLaunchKernelGGL(k_lists_target<D>, dim3(n_users), dim3(64), 0, s, user_emb, ld_u, users,
                           item_emb, ld_i, n_items, mask_rowptr, mask_items, target_rowptr,
                           target_items, cap_n, target_score, rank);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_lists_sort, dim3(n_users), dim3(64), 0, s, target_rowptr, target_items,
                           n_items, target_score, cap_n, cnt, sorted_s, sorted_t, sorted_e, rank);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        hipLaunchKernelGGL(k_lists_count<D>, dim3(tiles, n_splits), dim3(kWaves * 64), 0, s,
                           user_emb, ld_u, users, n_users, item_emb, ld_i, n_items, split_len,
                           target_rowptr, cnt, sorted_s, sorted_t, cap_n, part);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        hipLaunchKernelGGL(k_lists_finish<D>, dim3(n_users), dim3(64), 0, s, user_emb, ld_u, users,
                           item_emb, ld_i, n_items, mask_rowptr, mask_items, target_rowptr, cnt,
                           sorted_s, sorted_t, sorted_e, cap_n, part, n_splits, rank);
        return hipGetLastError();
    });
    return e == hipSuccess ? 0 : (int)e;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// lgcn_score_topk_wide: lgcn_score_topk's lists for k up to LGCN_TOPK_WIDE_MAX_K. The tile loop
// and the candidate filter are k_score_topk's; what differs is where a user's candidates live:
//  * LDS holds a user's count and threshold only. The candidates go to a per-(split, slot) buffer
//    in scratch of capacity cap = 2 kp, kp the power of two >= max(k, 32). One tile adds at most
//    32 entries per user, and a user whose count passes cap - 32 is selected right after the
//    tile: a buffer cannot overflow (and every position is still checked against cap).
//  * wide_select (out of line: the tile loop keeps k_score_topk's registers): the user's wave
//    reads the buffer into its LDS area (cap pairs, at most 2048 = 16 KB), sorts it with a bitonic
//    network under better(), writes the first k back and sets the threshold. All (score, index)
//    pairs are distinct, so the sorted order does not depend on the order they arrived in.
//  * at the end of a split the buffer's first cnt entries are the split's sorted list.
//  * k_topk_wide_merge: one block per slot. The splits' lists are sorted and disjoint, so the
//    global rank of an entry is its place in its own list plus its binary-search place in every
//    other list; an entry with rank < k is stored at [rank]. Only entries >= the largest k-th
//    score of a full list can have such a rank. No sort, no atomics on the outputs.
// ---------------------------------------------------------------------------------------------
namespace {

constexpr int kWideMaxK = LGCN_TOPK_WIDE_MAX_K;
constexpr int kWideMergeThreads = 256;
constexpr int64_t kWideMergeEntries = 16384;  // lgcn_topk_wide_splits keeps n_splits * k below it

constexpr int wide_kp(int k) {  // the power of two >= max(k, 32)
    int p = 32;
    while (p < k) p <<= 1;
    return p;
}
static_assert(wide_kp(kWideMaxK) == 1024, "a wave's sort area is 2 kp <= 2048 pairs");

struct WideState {
    int32_t cnt[kUsersPerWave];
    float thr[kUsersPerWave];
    int32_t mlo[kUsersPerWave];  // as WaveState's
    int32_t mhi[kUsersPerWave];
};

__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_s_waitcnt(kLgkm0);
    __builtin_amdgcn_wave_barrier();
}

// Sort user u's buffer (cs, ci)[0, cnt) under better(), keep the first K there, set the count and
// the threshold. ss / si: this wave's LDS area of cap pairs.
__device__ __noinline__ void wide_select(WideState& st, float* ss, int32_t* si, float* cs,
                                         int32_t* ci, int u, int K, int cap, int lane) {
    const int n = min(st.cnt[u], cap);
    int m = 32;
    while (m < n) m <<= 1;  // <= cap: cap is a power of two >= 64
    // the candidates' stores (other lanes' too) have landed before they are read back
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    for (int e = lane; e < m; e += 64) {  // padding sorts after every candidate
        ss[e] = e < n ? cs[e] : -INFINITY;
        si[e] = e < n ? ci[e] : INT32_MAX;
    }
    wave_sync();
    for (int size = 2; size <= m; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = lane; t < (m >> 1); t += 64) {
                const int i = 2 * t - (t & (stride - 1));
                const int j = i + stride;
                const float s1 = ss[i], s2 = ss[j];
                const int32_t i1 = si[i], i2 = si[j];
                const bool first = (i & size) == 0;  // this run is sorted best first
                if (first ? better(s2, i2, s1, i1) : better(s1, i1, s2, i2)) {
                    ss[i] = s2; si[i] = i2;
                    ss[j] = s1; si[j] = i1;
                }
            }
            wave_sync();
        }
    }
    const int keep = n < K ? n : K;
    for (int e = lane; e < keep; e += 64) {
        cs[e] = ss[e];
        ci[e] = si[e];
    }
    if (lane == 0) {
        st.cnt[u] = keep;
        // (no threshold while the K-th best is below -1e10: see compact_user)
        const float kth = keep == K ? ss[K - 1] : -INFINITY;
        st.thr[u] = kth < kMasked ? -INFINITY : kth;
    }
    wave_sync();
}

template <int D>
__global__ __launch_bounds__(kWaves * 64) void k_score_topk_wide(
    const float* __restrict__ uemb, int64_t ld_u, const int32_t* __restrict__ users,
    int32_t n_users, const float* __restrict__ iemb, int64_t ld_i, int32_t n_items,
    int32_t split_len, const int32_t* __restrict__ mrow, const int32_t* __restrict__ mitems, int K,
    int cap, float* cand_s, int32_t* cand_i, int32_t* __restrict__ part_cnt) {
    constexpr int DH = D / 2;
    // per wave: WideState | cap scores | cap indices
    extern __shared__ __attribute__((aligned(16))) char wsm[];
    const int wave = threadIdx.x >> 6;
    const int lane = threadIdx.x & 63;
    const int h = lane >> 5;
    const int col = lane & 31;
    char* mine = wsm + (size_t)wave * (sizeof(WideState) + (size_t)cap * 8);
    WideState& st = *reinterpret_cast<WideState*>(mine);
    float* ss = reinterpret_cast<float*>(mine + sizeof(WideState));
    int32_t* si = reinterpret_cast<int32_t*>(ss + cap);
    const int32_t ub = (blockIdx.x * kWaves + wave) * kUsersPerWave;
    const int32_t split = blockIdx.y;
    const int32_t it0 = split * split_len;
    const int32_t it1 = min(n_items, it0 + split_len);
    // row r of this wave: buffer (split, ub + r), cap entries (only slots < n_users are touched)
    const int64_t buf0 = ((int64_t)split * n_users + ub) * cap;

    if (lane < kUsersPerWave) {
        st.cnt[lane] = 0;
        st.thr[lane] = -INFINITY;
    }
    float4 a[D / 8];
    {
        const bool ok = ub + col < n_users;
        load_row_half<D>(uemb + (ok ? (int64_t)users[ub + col] * ld_u : 0) + h * DH, ok, a);
    }
    if (lane < kUsersPerWave) {
        const bool ok = ub + lane < n_users;
        const int32_t u = ok ? users[ub + lane] : 0;
        st.mlo[lane] = ok ? mrow[u] : 0;
        st.mhi[lane] = ok ? mrow[u + 1] : -1;
    }
    wave_sync();
    float4 bcur[D / 8], bnxt[D / 8];
    auto load_tile = [&](int32_t t0, float4 (&b)[D / 8]) {
        const int32_t item = t0 + col;
        const bool iok = item < it1;
        load_row_half<D>(iemb + (iok ? (int64_t)item * ld_i : 0) + h * DH, iok, b);
    };
    if (it0 < it1) load_tile(it0, bcur);
    for (int32_t t0 = it0; t0 < it1; t0 += 32) {
        if (t0 + 32 < it1) load_tile(t0 + 32, bnxt);
        const int32_t item = t0 + col;
        const bool iok = item < it1;
        const f32x16 acc = score_tile<D>(a, bcur);
        bool any = false;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = c_row(r, h);
            float sc = acc[r];
            const float thr = st.thr[row];
            if (iok && sc > thr) {
                const int32_t lo = st.mlo[row], hi = st.mhi[row];
                if (hi >= lo) {
                    if (in_sorted(mitems, lo, hi, item)) sc = kMasked;  // main.py:422-424
                    if (sc > thr) {
                        const int pos = atomicAdd(&st.cnt[row], 1);
                        if (pos < cap) {  // (always: at most cap - 32 before a tile, 32 a tile)
                            cand_s[buf0 + (int64_t)row * cap + pos] = sc;
                            cand_i[buf0 + (int64_t)row * cap + pos] = item;
                        }
                        any = true;
                    }
                }
            }
        }
        wave_sync();
        if (__any(any)) {
            // select every user whose buffer could overflow on the next tile
            uint64_t need = __ballot(lane < kUsersPerWave && st.cnt[lane] > cap - 32);
            while (need) {
                const int u = __builtin_ctzll(need);
                need &= need - 1;
                wide_select(st, ss, si, cand_s + buf0 + (int64_t)u * cap,
                            cand_i + buf0 + (int64_t)u * cap, u, K, cap, lane);
            }
        }
#pragma unroll
        for (int q = 0; q < D / 8; ++q) bcur[q] = bnxt[q];
    }
    // final: every buffer's first cnt entries become the split's sorted list
    for (int u = 0; u < kUsersPerWave; ++u) {
        if (ub + u >= n_users) break;
        wide_select(st, ss, si, cand_s + buf0 + (int64_t)u * cap, cand_i + buf0 + (int64_t)u * cap,
                    u, K, cap, lane);
        if (lane == 0) part_cnt[(int64_t)split * n_users + ub + u] = st.cnt[u];
    }
}

// The number of entries of the sorted list (ls, li)[0, n) that beat (s, x).
__device__ __forceinline__ int wide_place(const float* __restrict__ ls,
                                          const int32_t* __restrict__ li, int n, float s,
                                          int32_t x) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (better(ls[mid], li[mid], s, x)) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(kWideMergeThreads) void k_topk_wide_merge(
    const float* __restrict__ cand_s, const int32_t* __restrict__ cand_i,
    const int32_t* __restrict__ part_cnt, int32_t n_users, int32_t n_splits, int K, int cap,
    float* __restrict__ top_s, int32_t* __restrict__ top_i) {
    __shared__ int32_t s_cnt[256];  // n_splits <= 256
    __shared__ float s_t[kWideMergeThreads / 64];
    __shared__ int32_t s_tot[kWideMergeThreads / 64];
    const int32_t slot = blockIdx.x;
    const int tid = threadIdx.x;
    float t = -INFINITY;
    int32_t tot = 0;
    for (int s = tid; s < n_splits; s += kWideMergeThreads) {
        const int64_t b = ((int64_t)s * n_users + slot) * cap;
        const int32_t c = min(max(part_cnt[(int64_t)s * n_users + slot], 0), K);
        s_cnt[s] = c;
        tot += c;
        if (c == K) t = fmaxf(t, cand_s[b + K - 1]);  // a full list bounds the global K-th score
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        t = fmaxf(t, __shfl_xor(t, off));
        tot += __shfl_xor(tot, off);
    }
    if ((tid & 63) == 0) {
        s_t[tid >> 6] = t;
        s_tot[tid >> 6] = tot;
    }
    __syncthreads();
    t = s_t[0];
    tot = s_tot[0];
#pragma unroll
    for (int w = 1; w < kWideMergeThreads / 64; ++w) {
        t = fmaxf(t, s_t[w]);
        tot += s_tot[w];
    }
    const int total = n_splits * K;  // <= 256 * 1024
    for (int e = tid; e < total; e += kWideMergeThreads) {
        const int s = e / K, j = e - s * K;
        if (j >= s_cnt[s]) continue;
        const int64_t b = ((int64_t)s * n_users + slot) * cap;
        const float v = cand_s[b + j];
        if (!(v >= t)) continue;
        const int32_t id = cand_i[b + j];
        int rank = j;
        for (int s2 = 0; s2 < n_splits && rank < K; ++s2) {
            if (s2 == s) continue;
            const int64_t b2 = ((int64_t)s2 * n_users + slot) * cap;
            rank += wide_place(cand_s + b2, cand_i + b2, s_cnt[s2], v, id);
        }
        if (rank < K) {
            top_s[(int64_t)slot * K + rank] = v;
            top_i[(int64_t)slot * K + rank] = id;
        }
    }
    for (int r = min(tot, K) + tid; r < K; r += kWideMergeThreads) {  // fewer than K listable items
        top_s[(int64_t)slot * K + r] = -INFINITY;
        top_i[(int64_t)slot * K + r] = -1;
    }
}

// Scratch: cand score [n_splits x n_users x cap] | cand index, the same | count [n_splits x n_users]
constexpr size_t wide_bytes(int64_t n_users, int64_t cap, int64_t n_splits) {
    return ((size_t)n_splits * (size_t)n_users * (size_t)(8 * cap + 4) + 15) / 16 * 16;
}

}  // namespace

extern "C" {

int lgcn_topk_wide_splits(int32_t n_users, int32_t n_items, int32_t k, int32_t n_cu) {
    int64_t s = lgcn_eval_splits(n_users, n_items, n_cu);
    if (k < 1) k = 1;
    if (k > kWideMaxK) k = kWideMaxK;
    const int64_t floor_len = 8LL * k > 2048 ? 8LL * k : 2048;
    const int64_t max_by_len = (int64_t)(n_items > 0 ? n_items : 0) / floor_len;
    if (s > max_by_len) s = max_by_len;
    if (s > kWideMergeEntries / k) s = kWideMergeEntries / k;
    if (s < 1) s = 1;
    return (int)s;
}

size_t lgcn_score_topk_wide_scratch_bytes(int32_t n_users, int32_t k, int32_t n_splits) {
    if (n_users < 0 || k < 1 || k > kWideMaxK || n_splits < 1 || n_splits > 256) return 0;
    return wide_bytes(n_users, 2 * wide_kp(k), n_splits);
}

int lgcn_score_topk_wide(const float* user_emb, int64_t ld_u, const int32_t* users,
                         int32_t n_users, const float* item_emb, int64_t ld_i, int32_t n_items,
                         int32_t d, const int32_t* mask_rowptr, const int32_t* mask_items,
                         int32_t k, int32_t n_splits, void* scratch, size_t scratch_bytes,
                         float* top_scores, int32_t* top_idx, void* stream) {
    if (k < 1 || k > kWideMaxK) return LGCN_EINVAL;
    if (const int rc = eval_args(user_emb, ld_u, n_users, item_emb, ld_i, n_items, d, n_splits))
        return rc;
    if (n_users == 0) return 0;
    if (!user_emb || !users || !item_emb || !mask_rowptr || !scratch || !top_scores || !top_idx)
        return LGCN_EINVAL;
    const int cap = 2 * wide_kp(k);
    if (scratch_bytes < wide_bytes(n_users, cap, n_splits)) return LGCN_EINVAL;
    if (reinterpret_cast<uintptr_t>(scratch) & 3) return LGCN_EALIGN;
    const size_t n_buf = (size_t)n_splits * (size_t)n_users * (size_t)cap;
    float* cand_s = static_cast<float*>(scratch);
    int32_t* cand_i = reinterpret_cast<int32_t*>(cand_s + n_buf);
    int32_t* part_cnt = cand_i + n_buf;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int32_t split_len = eval_split_len(n_items, n_splits);
    const dim3 grid(user_tiles(n_users), n_splits);
    const size_t lds = (sizeof(WideState) + (size_t)cap * 8) * kWaves;
    hipError_t e = with_width(d, [&](auto width) {
        constexpr int D = decltype(width)::value;
        const hipError_t ea =
            hipFuncSetAttribute(reinterpret_cast<const void*>(k_score_topk_wide<D>),
                                hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)((sizeof(WideState) + (size_t)2 * kWideMaxK * 8) * kWaves));
        if (ea != hipSuccess) return ea;
        hipLaunchKernelGGL(k_score_topk_wide<D>, grid, dim3(kWaves * 64), lds, s, user_emb, ld_u,
                           users, n_users, item_emb, ld_i, n_items, split_len, mask_rowptr,
                           mask_items, k, cap, cand_s, cand_i, part_cnt);
        return hipGetLastError();
    });
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_topk_wide_merge, dim3(n_users), dim3(kWideMergeThreads), 0, s, cand_s,
                       cand_i, part_cnt, n_users, n_splits, k, cap, top_scores, top_idx);
    e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}

}  // extern "C"

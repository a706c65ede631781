// lgcn_inbatch_rows.h — the in-batch softmax kernels of lgcn_inbatch.hip, templated on how sample
// b's rows, its validity, the off(b, c) predicate and the column correction are obtained (gathered
// blocks with masks, or the tables by index with the sampler's CSR: one body, so the two are
// bitwise equal by construction).
//
//   z_bc = <FU[users[b]], FI[pos[c]]> / tau - q[pos[c]]
//   L_b  = log(sum_{c on} exp(z_bc - zmax_b)) + (zmax_b - z_bb)
//   loss = mean_b L_b + lambda * (|U0|^2 + |P0|^2) / B
//
// The B x B logits are never stored: every sweep recomputes its 32 x 32 score tiles on the exact
// f32 MFMA. What is stored between the launches: the on(b, c) bits (k_inb_mask, one search per
// pair instead of one per pair and sweep) and per sample L_b, the squared norms, zmax_b, Z_b and
// the column's correction (work = [5 x B]). include/lgcn.h (lgcn_inbatch_loss) states every order
// of summation.
#ifndef LGCN_INBATCH_ROWS_H_
#define LGCN_INBATCH_ROWS_H_

#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "lgcn_ssm_rows.h"  // kWave, kRowsPerBlock, wave_sum, k_ssm_reduce

namespace lgcn_inb {

using lgcn_bpr::kRowsPerBlock;
using lgcn_bpr::kWave;
using lgcn_bpr::wave_sum;

constexpr int kTile = 32;      // samples per side of a score tile
constexpr int kSweepWaves = 4; // waves of a sweep block: they share the block's own tile
constexpr int kMaskBlock = 256;

typedef float f32x16 __attribute__((ext_vector_type(16)));

// gathered blocks: sample b is row b of u, p, u0, p0; off (NULL = none) uint8 [B x B], valid
// (NULL = every sample) uint8 [B], q (NULL = 0) float [B]
struct GatheredRows {
    const float* p[4];  // u, p, u0, p0
    int64_t ld[4];
    const uint8_t* offm;
    const uint8_t* valid;
    const float* q;
    __device__ __forceinline__ bool live(int64_t b) const {
        return valid == nullptr || valid[b] != 0;
    }
    // element offset of sample b's row in block / table i (i & 1: 0 the user side, 1 the positive)
    __device__ __forceinline__ int64_t at(int i, int64_t b) const { return b * ld[i]; }
    __device__ __forceinline__ bool off(int64_t b, int64_t c, int32_t B) const {
        return offm != nullptr && offm[b * B + c] != 0;
    }
    __device__ __forceinline__ float qcol(int64_t c) const { return q != nullptr ? q[c] : 0.f; }
};

// the tables themselves: p = final user, final item, layer-0 user, layer-0 item. A sample whose
// user or positive lies outside its table is not live and nothing of it is dereferenced. off(b, c)
// for two live samples: the same item, the same user, or (rowptr given) pos[c] in the sorted list
// of users[b] (lgcn_bpr_sample's CSR).
struct IndexedRows {
    const float* p[4];
    int64_t ld[4];
    const int64_t* users;
    const int64_t* pos;
    int64_t n_users, n_items;
    const int32_t* rowptr;
    const int32_t* items;
    const float* qtab;
    __device__ __forceinline__ bool live(int64_t b) const {
        const int64_t iu = users[b], ip = pos[b];
        return iu >= 0 && iu < n_users && ip >= 0 && ip < n_items;
    }
    __device__ __forceinline__ int64_t at(int i, int64_t b) const {
        return ((i & 1) ? pos[b] : users[b]) * ld[i];
    }
    __device__ __forceinline__ bool off(int64_t b, int64_t c, int32_t) const {
        const int64_t ub = users[b], pc = pos[c];
        if (pc == pos[b] || users[c] == ub) return true;
        if (rowptr == nullptr) return false;
        int32_t lo = rowptr[ub], hi = rowptr[ub + 1];
        while (lo < hi) {
            const int32_t mid = lo + ((hi - lo) >> 1);
            const int64_t v = items[mid];
            if (v == pc) return true;
            if (v < pc) lo = mid + 1; else hi = mid;
        }
        return false;
    }
    __device__ __forceinline__ float qcol(int64_t c) const {
        return qtab != nullptr ? qtab[pos[c]] : 0.f;
    }
};

// mask = [B x W] words, W = ceil(B / 32): bit (c & 31) of word [b][c >> 5] = on(b, c) = both
// samples live and (c == b or not off(b, c)); the bits past column B - 1 are zero.
template <typename Rows>
__global__ __launch_bounds__(kMaskBlock) void k_inb_mask(Rows rows, int32_t B, int32_t W,
                                                         uint32_t* __restrict__ mask) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t b = blockIdx.y;
    const int64_t c = (int64_t)blockIdx.x * kMaskBlock + threadIdx.x;
    bool on = false;
    if (c < B && rows.live(b) && rows.live(c)) on = c == b || !rows.off(b, c, B);
    const uint64_t bal = __ballot(on);
    const int64_t w0 = (c - lane) >> 5;  // the wave's 64 columns are words w0 and w0 + 1
    if (lane == 0 && w0 < W) mask[b * W + w0] = (uint32_t)bal;
    if (lane == 32 && w0 + 1 < W) mask[b * W + w0 + 1] = (uint32_t)(bal >> 32);
}

// work = [5 x B]: L_b, squared norms, zmax_b, Z_b, q of column b. One wave per sample: the squared
// norms of its two layer-0 rows, their gradient rows (half 0 of grads) and the column correction.
template <typename Rows>
__global__ __launch_bounds__(kWave * kRowsPerBlock) void k_inb_prep(
    Rows rows, int32_t B, int32_t d, float lambda, float* __restrict__ work,
    float* __restrict__ grads) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t b = (int64_t)blockIdx.x * kRowsPerBlock + threadIdx.x / kWave;
    if (b >= B) return;
    float* gu0 = grads + b * (int64_t)d;
    float* gp0 = grads + ((int64_t)B + b) * d;
    if (!rows.live(b)) {  // skipped: +0 rows, a zero term
        for (int k = lane; k < d; k += kWave) gu0[k] = gp0[k] = 0.f;
        if (lane == 0) work[(int64_t)B + b] = work[4 * (int64_t)B + b] = 0.f;
        return;
    }
    const float* ub0 = rows.p[2] + rows.at(2, b);
    const float* pb0 = rows.p[3] + rows.at(3, b);
    const float r = 2.f * lambda / (float)B;
    float sq = 0.f;
    for (int k = lane; k < d; k += kWave) {
        sq = __builtin_fmaf(ub0[k], ub0[k], sq);
        sq = __builtin_fmaf(pb0[k], pb0[k], sq);
        gu0[k] = r * ub0[k];
        gp0[k] = r * pb0[k];
    }
    sq = wave_sum(sq);
    if (lane == 0) {
        work[(int64_t)B + b] = sq;
        work[4 * (int64_t)B + b] = rows.qcol(b);
    }
}

// Which row of a 32 x 32 MFMA result register r holds in lane half h (its column is lane & 31).
__device__ __forceinline__ int c_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// One operand of a score tile: this lane's features of one row (row = nullptr: zeros, nothing is
// read). Lane half h holds features 8q + 4h + {0, 1, 2, 3} in v[q]; features >= d are +0. vec: the
// row is 16-byte aligned (pointer and leading dimension), so a whole group is one load.
template <int NQ>
__device__ __forceinline__ void load_operand(const float* __restrict__ row, int h, int32_t d,
                                             bool vec, float4 (&v)[NQ]) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const int k = 8 * q + 4 * h;
        float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row != nullptr && k < d) {
            if (vec && k + 4 <= d) {
                x = *reinterpret_cast<const float4*>(row + k);
            } else {
                x.x = row[k];
                if (k + 1 < d) x.y = row[k + 1];
                if (k + 2 < d) x.z = row[k + 2];
                if (k + 3 < d) x.w = row[k + 3];
            }
        }
        v[q] = x;
    }
}

// acc[r] in lane (j = lane & 31, h) = the score of A-side row c_row(r, h) and B-side row j: one
// fmaf chain from +0 over MFMA steps 4q + x, step 4q + x adding feature 8q + x, then 8q + 4 + x.
// A score is a function of its two rows and of d's width class alone.
template <int NQ>
__device__ __forceinline__ f32x16 score_tile(const float4 (&a)[NQ], const float4 (&b)[NQ]) {
    f32x16 acc = {};
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q].x, b[q].x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q].y, b[q].y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q].z, b[q].z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q].w, b[q].w, acc, 0, 0, 0);
    }
    return acc;
}

// the logit of a score and the coefficient of a logit: each one expression, used by every sweep
__device__ __forceinline__ float logit_of(float s, float inv_tau, float q) {
    return s * inv_tau - q;
}
__device__ __forceinline__ float coef_of(float z, bool on, bool diag, float zmax, float Z,
                                         float cf) {
    if (!on) return 0.f;
    return (expf(z - zmax) / Z - (diag ? 1.f : 0.f)) * cf;
}

// What a sweep block knows of the samples of one tile, per lane j = lane & 31: sample t0 + j.
struct TileSide {
    int64_t at;     // element offset of its final row, -1: not live or past B
    const float* row;
};

template <typename Rows>
__device__ __forceinline__ TileSide tile_side(const Rows& rows, int side, int64_t s, int32_t B) {
    TileSide t;
    t.at = -1;
    t.row = nullptr;
    if (s < B && rows.live(s)) {
        t.at = rows.at(side, s);
        t.row = rows.p[side] + t.at;
    }
    return t;
}

// The row sweep for zmax_b, then Z_b, then L_b. A block owns 32 users; wave w of its four takes
// the column tiles t = w, w + 4, ... in ascending t. Tile: A = the 32 positives, B = the 32 users,
// so lane (j, h) holds user b0 + j against columns c0 + c_row(r, h).
template <typename Rows, int NT>
__global__ __launch_bounds__(kWave * kSweepWaves) void k_inb_stats(
    Rows rows, int32_t B, int32_t W, int32_t d, float inv_tau, bool vec_u, bool vec_p,
    const uint32_t* __restrict__ mask, float* __restrict__ work) {
    constexpr int NQ = 4 * NT;
    __shared__ float s_part[kSweepWaves][kTile];
    __shared__ float s_diag[kTile];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int h = lane >> 5, j = lane & 31;
    const int64_t b0 = (int64_t)blockIdx.x * kTile, b = b0 + j;
    const float* qc = work + 4 * (int64_t)B;
    const TileSide own = tile_side(rows, 0, b, B);
    float4 fb[NQ];
    load_operand<NQ>(own.row, h, d, vec_u, fb);
    if (threadIdx.x < kTile) s_diag[threadIdx.x] = 0.f;
    const int32_t n_tiles = W;

    float part = 0.f, zmax = 0.f;
    for (int pass = 0; pass < 2; ++pass) {  // 0: the maximum, 1: the sum
        part = pass == 0 ? -INFINITY : 0.f;
        for (int32_t t = wave; t < n_tiles; t += kSweepWaves) {
            const int64_t c0 = (int64_t)t * kTile;
            const TileSide oth = tile_side(rows, 1, c0 + j, B);
            float4 fa[NQ];
            load_operand<NQ>(oth.row, h, d, vec_p, fa);
            const uint32_t bits = b < B ? mask[b * W + t] : 0u;
            const float qv = c0 + j < B ? qc[c0 + j] : 0.f;
            const f32x16 acc = score_tile<NQ>(fa, fb);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int cr = c_row(r, h);
                const float q = __shfl(qv, cr, kWave);
                if ((bits >> cr) & 1) {
                    const float z = logit_of(acc[r], inv_tau, q);
                    if (pass == 0) {
                        part = fmaxf(part, z);
                    } else {
                        part += expf(z - zmax);
                        if (c0 + cr == b) s_diag[j] = z;
                    }
                }
            }
        }
        // the two lane halves of a user, then the four waves in order
        const float other = __shfl_xor(part, 32, kWave);
        part = pass == 0 ? fmaxf(part, other) : part + other;
        __syncthreads();  // pass 1: every wave has read s_part of pass 0
        if (h == 0) s_part[wave][j] = part;
        __syncthreads();
        if (pass == 0) {
            zmax = fmaxf(fmaxf(s_part[0][j], s_part[1][j]), fmaxf(s_part[2][j], s_part[3][j]));
            if (!(zmax > -INFINITY)) zmax = 0.f;  // no column on: a skipped sample
        }
    }
    if (wave == 0 && h == 0 && b < B) {
        float Z = ((s_part[0][j] + s_part[1][j]) + s_part[2][j]) + s_part[3][j];
        const bool alive = own.row != nullptr;
        if (!alive) Z = 1.f;
        work[b] = alive ? logf(Z) + (zmax - s_diag[j]) : 0.f;
        work[2 * (int64_t)B + b] = zmax;
        work[3 * (int64_t)B + b] = Z;
    }
}

// The two gradient sweeps, blockIdx.y = the side that owns the block's 32 output rows: 0 the users
// (dFU = G P, the other side = the positives, its tiles column tiles), 1 the positives (dFI = G^T
// U, the other side = the users, its tiles row tiles). Wave w of the four takes the other side's
// tiles t = w, w + 4, ... in ascending t. Tile: A = the other side's 32 rows, B = the own 32 rows:
// lane (j, h) holds own sample o0 + j against the other side's samples t0 + c_row(r, h), and the
// 16 coefficients it forms are, register by register, the A operand of the gradient product — step
// r multiplies them with rows t0 + c_row(r, 0) and t0 + c_row(r, 1) of the other side.
template <typename Rows, int NT>
__global__ __launch_bounds__(kWave * kSweepWaves) void k_inb_grad(
    Rows rows, int32_t B, int32_t W, int32_t d, float inv_tau, float cf, bool vec_u, bool vec_p,
    const uint32_t* __restrict__ mask, const float* __restrict__ work, float* __restrict__ grads,
    float* __restrict__ coef) {
    constexpr int NQ = 4 * NT;
    __shared__ float s_out[kTile * kTile * NT];  // [NT][16 regs][64 lanes]
    const int side = blockIdx.y;                 // uniform over the block
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int h = lane >> 5, j = lane & 31;
    const int64_t o0 = (int64_t)blockIdx.x * kTile, o = o0 + j;
    const float* zm = work + 2 * (int64_t)B;
    const float* zs = work + 3 * (int64_t)B;
    const float* qc = work + 4 * (int64_t)B;
    const TileSide own = tile_side(rows, side, o, B);
    float4 fb[NQ];
    load_operand<NQ>(own.row, h, d, side == 0 ? vec_u : vec_p, fb);
    // per lane: the own sample's statistics (side 0) or its correction (side 1)
    const float own_m = o < B ? (side == 0 ? zm[o] : qc[o]) : 0.f;
    const float own_Z = side == 0 && o < B ? zs[o] : 1.f;
    const float* otab = rows.p[1 - side];

    f32x16 out[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i) out[i] = f32x16{};
    for (int32_t t = wave; t < W; t += kSweepWaves) {
        const int64_t t0 = (int64_t)t * kTile;
        const TileSide oth = tile_side(rows, 1 - side, t0 + j, B);
        float4 fa[NQ];
        load_operand<NQ>(oth.row, h, d, side == 0 ? vec_p : vec_u, fa);
        // side 0: this user's word of on bits, the columns' corrections; side 1: the words and the
        // statistics of the tile's 32 users, one per lane
        uint32_t bits = 0u;
        float tv_m = 0.f, tv_Z = 1.f;
        if (side == 0) {
            if (o < B) bits = mask[o * W + t];
            if (t0 + j < B) tv_m = qc[t0 + j];
        } else if (t0 + j < B) {
            bits = mask[(t0 + j) * W + blockIdx.x];
            tv_m = zm[t0 + j];
            tv_Z = zs[t0 + j];
        }
        const f32x16 acc = score_tile<NQ>(fa, fb);
        float g[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int cr = c_row(r, h);
            const float om = __shfl(tv_m, cr, kWave);
            const float oZ = __shfl(tv_Z, cr, kWave);
            const uint32_t ow = (uint32_t)__shfl((int)bits, cr, kWave);
            const bool on = side == 0 ? (bits >> cr) & 1 : (ow >> j) & 1;
            const float z = logit_of(acc[r], inv_tau, side == 0 ? om : own_m);
            g[r] = coef_of(z, on, t0 + cr == o, side == 0 ? own_m : om, side == 0 ? own_Z : oZ,
                           cf);
            if (coef != nullptr && side == 0 && o < B && t0 + cr < B)
                coef[o * B + t0 + cr] = g[r];
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int64_t at = __shfl(oth.at, c_row(r, h), kWave);
#pragma unroll
            for (int i = 0; i < NT; ++i) {
                const int k = kTile * i + j;
                const float v = at >= 0 && k < d ? otab[at + k] : 0.f;
                out[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(g[r], v, out[i], 0, 0, 0);
            }
        }
    }
    // the four waves' partial tiles, added in wave order: ((w0 + w1) + w2) + w3
    for (int w = 0; w < kSweepWaves; ++w) {
        if (wave == w) {
#pragma unroll
            for (int i = 0; i < NT; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    float* s = &s_out[(i * 16 + r) * kWave + lane];
                    *s = w == 0 ? out[i][r] : *s + out[i][r];
                }
        }
        __syncthreads();
    }
    // s_out[i][r][lane (k, hh)] = own row c_row(r, hh), feature 32 i + k
    float* dst = grads + ((int64_t)2 * B + (int64_t)side * B) * d;  // half 1, users or positives
    for (int e = threadIdx.x; e < kTile * kTile * NT; e += kWave * kSweepWaves) {
        const int k = e & 31, row = (e >> 5) & 31, i = e >> 10;
        const int feat = kTile * i + k;
        if (o0 + row < B && feat < d) {
            const int r = (row & 3) + 4 * (row >> 3), hh = (row >> 2) & 1;
            dst[(o0 + row) * d + feat] = s_out[(i * 16 + r) * kWave + 32 * hh + k];
        }
    }
}

template <typename Rows, int NT>
inline int launch_sweeps(const Rows& rows, int32_t B, int32_t W, int32_t d, float inv_tau,
                         float cf, bool vec_u, bool vec_p, const uint32_t* mask, float* work,
                         float* grads, float* coef, hipStream_t s) {
    const uint32_t tiles = (uint32_t)W;
    hipLaunchKernelGGL((k_inb_stats<Rows, NT>), dim3(tiles), dim3(kWave * kSweepWaves), 0, s, rows,
                       B, W, d, inv_tau, vec_u, vec_p, mask, work);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL((k_inb_grad<Rows, NT>), dim3(tiles, 2), dim3(kWave * kSweepWaves), 0, s,
                       rows, B, W, d, inv_tau, cf, vec_u, vec_p, mask, (const float*)work, grads,
                       coef);
    e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}

inline bool aligned16(const float* p, int64_t ld) {
    return (reinterpret_cast<uintptr_t>(p) & 15) == 0 && (ld & 3) == 0;
}

// every launch of one batch: the on bits, the per-sample part, the three sweeps, the reduction
template <typename Rows>
inline int launch(const Rows& rows, int32_t B, int32_t d, float lambda, float tau, float* work,
                  uint32_t* mask, float* loss, float* grads, float* coef, hipStream_t s) {
    const int32_t W = (B + kTile - 1) / kTile;
    hipLaunchKernelGGL(k_inb_mask<Rows>, dim3((uint32_t)((B + kMaskBlock - 1) / kMaskBlock),
                                              (uint32_t)B),
                       dim3(kMaskBlock), 0, s, rows, B, W, mask);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    const int64_t grid = ((int64_t)B + kRowsPerBlock - 1) / kRowsPerBlock;
    hipLaunchKernelGGL(k_inb_prep<Rows>, dim3((uint32_t)grid), dim3(kWave * kRowsPerBlock), 0, s,
                       rows, B, d, lambda, work, grads);
    e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    const float inv_tau = 1.f / tau;
    const float cf = inv_tau / (float)B;
    const bool vu = aligned16(rows.p[0], rows.ld[0]), vp = aligned16(rows.p[1], rows.ld[1]);
    int rc;
    if (d <= 32)
        rc = launch_sweeps<Rows, 1>(rows, B, W, d, inv_tau, cf, vu, vp, mask, work, grads, coef, s);
    else if (d <= 64)
        rc = launch_sweeps<Rows, 2>(rows, B, W, d, inv_tau, cf, vu, vp, mask, work, grads, coef, s);
    else if (d <= 128)
        rc = launch_sweeps<Rows, 4>(rows, B, W, d, inv_tau, cf, vu, vp, mask, work, grads, coef, s);
    else
        rc = launch_sweeps<Rows, 8>(rows, B, W, d, inv_tau, cf, vu, vp, mask, work, grads, coef, s);
    if (rc != 0) return rc;
    hipLaunchKernelGGL(lgcn_ssm::k_ssm_reduce, dim3(1), dim3(256), 0, s, (const float*)work, B,
                       lambda, loss);
    e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}

}  // namespace lgcn_inb
#endif  // LGCN_INBATCH_ROWS_H_

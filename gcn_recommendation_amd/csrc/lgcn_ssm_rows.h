// lgcn_ssm_rows.h — the sampled-softmax batch kernels of lgcn_ssm.hip: one row kernel, templated
// on how sample b's rows are obtained (gathered blocks, or the tables by index: one body, so the
// two are bitwise equal by construction), and the fixed-order batch reduction. A sample has
// 2 + M rows in each of the two tables' views: user, positive, M candidate negatives.
//
//   z_0 = <u,p> / tau - q_0, z_m = <u,n_m> / tau - q_m   (scores: lgcn_bpr::row_scores; q: the
//                                                         optional logQ correction, else no term)
//   L_b = log(sum_j exp(z_j - z_max)) + (z_max - z_0)
//   loss = mean_b L_b + lambda * (|U0|^2 + |P0|^2 + |N0|^2) / B
//
// include/lgcn.h (lgcn_ssm_loss) states every order of summation.
#ifndef LGCN_SSM_ROWS_H_
#define LGCN_SSM_ROWS_H_

#include <hip/hip_runtime.h>

#include <stdint.h>

#include "lgcn_bpr_rows.h"  // kWave, kRowsPerBlock, wave_sum, row_scores

namespace lgcn_ssm {

using lgcn_bpr::kRowsPerBlock;
using lgcn_bpr::kWave;
using lgcn_bpr::row_scores;
using lgcn_bpr::wave_sum;

constexpr int kInFlight = 4;  // candidate rows whose loads are in flight together

// the four fixed rows of one sample: u, p (final) and u0, p0 (layer 0)
struct SampleRows {
    const float* r[4];
};

// rows of gathered blocks: sample b is row b of u, p, u0, p0 and rows b * M + m of the two
// [B*M x d] candidate blocks; valid (NULL = every entry) masks candidates; q likewise by ordinal
struct GatheredRows {
    const float* p[4];  // u, p, u0, p0
    int64_t ld[4];
    const float* n;
    int64_t ldn;
    const float* n0;
    int64_t ldn0;
    const uint8_t* valid;
    const float* q_pos;  // [B], nullptr = none
    const float* q_neg;  // [B x M], nullptr = none
    __device__ __forceinline__ bool get(int64_t b, SampleRows& o) const {
#pragma unroll
        for (int i = 0; i < 4; ++i) o.r[i] = p[i] + b * ld[i];
        return true;
    }
    // the logQ correction: whether there is one, the positive's, the candidate's at ordinal `at`
    __device__ __forceinline__ bool has_q() const { return q_pos != nullptr || q_neg != nullptr; }
    __device__ __forceinline__ float qpos(int64_t b) const {
        return q_pos != nullptr ? q_pos[b] : 0.f;
    }
    __device__ __forceinline__ float qcand(int64_t at) const {
        return q_neg != nullptr ? q_neg[at] : 0.f;
    }
    // candidate m of sample b: its row ordinal, and whether it takes part
    __device__ __forceinline__ bool cand(int64_t b, int m, int32_t M, int64_t& at) const {
        at = b * M + m;
        return valid == nullptr || valid[at] != 0;
    }
    __device__ __forceinline__ const float* nrow(int64_t at) const { return n + at * ldn; }
    __device__ __forceinline__ const float* n0row(int64_t at) const { return n0 + at * ldn0; }
};

// rows of the tables themselves: tab = final user, final item, layer-0 user, layer-0 item. A
// sample whose user or positive lies outside its table has no rows (false); a candidate outside
// [0, n_items) takes no part; nothing of either is dereferenced. q is item_q at the item's index.
struct IndexedRows {
    const float* tab[4];
    int64_t ld[4];
    const int64_t* users;
    const int64_t* pos;
    const int64_t* neg;  // [B x M]
    int64_t n_users, n_items;
    const float* item_q;  // [n_items], nullptr = none
    __device__ __forceinline__ bool get(int64_t b, SampleRows& o) const {
        const int64_t iu = users[b], ip = pos[b];
        if (iu < 0 || iu >= n_users || ip < 0 || ip >= n_items) return false;
        o.r[0] = tab[0] + iu * ld[0];
        o.r[1] = tab[1] + ip * ld[1];
        o.r[2] = tab[2] + iu * ld[2];
        o.r[3] = tab[3] + ip * ld[3];
        return true;
    }
    // asked only of a sample that has rows and of a candidate that takes part: both in range
    __device__ __forceinline__ bool has_q() const { return item_q != nullptr; }
    __device__ __forceinline__ float qpos(int64_t b) const { return item_q[pos[b]]; }
    __device__ __forceinline__ float qcand(int64_t at) const { return item_q[at]; }
    __device__ __forceinline__ bool cand(int64_t b, int m, int32_t M, int64_t& at) const {
        at = neg[b * M + m];
        return at >= 0 && at < n_items;
    }
    __device__ __forceinline__ const float* nrow(int64_t at) const { return tab[1] + at * ld[1]; }
    __device__ __forceinline__ const float* n0row(int64_t at) const { return tab[3] + at * ld[3]; }
};

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, kWave));
    return v;
}

// grads = [2 x (2+M)B x d]: half 0 the layer-0 rows, half 1 the final rows; inside a half rows
// [0, B) users, [B, 2B) positives, 2B + b * M + m candidate m of sample b. terms = [2 x B] (L_b,
// squared norms); coef (nullptr = not wanted) = [B x (1+M)] (g_0, g_1..g_M). One wave per sample;
// lane m owns candidate m: its row ordinal, its validity, then its logit and its coefficient.
template <typename Rows>
__global__ __launch_bounds__(kWave * kRowsPerBlock) void k_ssm_rows(
    Rows rows, int32_t B, int32_t M, int32_t d, float lambda, float inv_tau,
    float* __restrict__ terms, float* __restrict__ grads, float* __restrict__ coef) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t b = (int64_t)blockIdx.x * kRowsPerBlock + threadIdx.x / kWave;
    if (b >= B) return;
    const int64_t half = (int64_t)(2 + M) * B * d;
    float* gu0 = grads + b * (int64_t)d;
    float* gp0 = grads + ((int64_t)B + b) * d;
    float* gn0 = grads + (2 * (int64_t)B + b * M) * d;
    float* gu = gu0 + half;
    float* gp = gp0 + half;
    float* gn = gn0 + half;
    SampleRows sr;
    const bool have = rows.get(b, sr);
    int64_t at = -1;
    const bool ok = have && lane < M && rows.cand(b, lane, M, at);
    const uint64_t live = __ballot(ok);
    const bool has_q = rows.has_q();                            // uniform over the grid
    const float qm = has_q && ok ? rows.qcand(at) : 0.f;        // lane m: q of candidate m
    if (live == 0) {  // skipped: +0 rows, zero terms and coefficients
        for (int k = lane; k < d; k += kWave) gu[k] = gp[k] = gu0[k] = gp0[k] = 0.f;
        for (int64_t o = lane; o < (int64_t)M * d; o += kWave) gn[o] = gn0[o] = 0.f;
        if (lane == 0) {
            terms[b] = terms[B + b] = 0.f;
            if (coef != nullptr) coef[b * (1 + M)] = 0.f;
        }
        if (coef != nullptr && lane < M) coef[b * (1 + M) + 1 + lane] = 0.f;
        return;
    }
    const float* ub = sr.r[0];
    const float* pb = sr.r[1];
    const float* ub0 = sr.r[2];
    const float* pb0 = sr.r[3];

    // pass 1: the logits; the squared norms ride along
    float sq = 0.f;
    for (int k = lane; k < d; k += kWave) {
        sq = __builtin_fmaf(ub0[k], ub0[k], sq);
        sq = __builtin_fmaf(pb0[k], pb0[k], sq);
    }
    const float* const pr[1] = {pb};
    float s0[1];
    row_scores(ub, pr, d, lane, s0);
    float z0 = s0[0] * inv_tau;
    if (has_q) z0 = z0 - rows.qpos(b);
    float z = 0.f;  // lane m: z_m
    uint64_t todo = live;
    while (todo != 0) {
        int src[kInFlight];
        const float* nr[kInFlight];
        const float* nr0[kInFlight];
        int n = 0;
#pragma unroll
        for (int i = 0; i < kInFlight; ++i) {
            if (todo != 0) {  // uniform over the wave; true for i = 0
                src[i] = __builtin_ctzll(todo);  // ascending ordinal
                todo &= todo - 1;
                n = i + 1;
            } else {
                src[i] = src[0];  // a short last group repeats its first row
            }
            const int64_t a = __shfl(at, src[i], kWave);
            nr[i] = rows.nrow(a);
            nr0[i] = rows.n0row(a);
        }
        float sc[kInFlight];
        row_scores(ub, nr, d, lane, sc);
#pragma unroll
        for (int i = 0; i < kInFlight; ++i) {
            if (i < n) {
                if (lane == src[i]) z = sc[i] * inv_tau;
                for (int k = lane; k < d; k += kWave)
                    sq = __builtin_fmaf(nr0[i][k], nr0[i][k], sq);
            }
        }
    }
    if (has_q) z = z - qm;
    sq = wave_sum(sq);
    const float zmax = fmaxf(z0, wave_max(ok ? z : z0));
    const float e0 = expf(z0 - zmax);
    const float e = ok ? expf(z - zmax) : 0.f;
    const float Z = e0 + wave_sum(e);
    const float c = inv_tau / (float)B;
    const float g0 = (e0 / Z - 1.f) * c;
    const float g = (e / Z) * c;  // lane m: g_m, +0 for a candidate that takes no part
    const float r = 2.f * lambda / (float)B;

    // pass 2: the same rows again (L2 hits), a column chunk of 64 at a time
    for (int k0 = 0; k0 < d; k0 += kWave) {
        const int k = k0 + lane;
        const bool in = k < d;
        const float uk = in ? ub[k] : 0.f;
        float du = in ? g0 * pb[k] : 0.f;
        for (int m0 = 0; m0 < M; m0 += kInFlight) {
            float gm[kInFlight], v[kInFlight], v0[kInFlight];
#pragma unroll
            for (int i = 0; i < kInFlight; ++i) {
                const int m = m0 + i;
                gm[i] = v[i] = v0[i] = 0.f;
                if (m < M && ((live >> m) & 1)) {  // uniform over the wave
                    gm[i] = __shfl(g, m, kWave);
                    const int64_t a = __shfl(at, m, kWave);
                    if (in) {
                        v[i] = rows.nrow(a)[k];
                        v0[i] = rows.n0row(a)[k];
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < kInFlight; ++i) {
                const int m = m0 + i;
                if (m < M) {
                    const bool on = (live >> m) & 1;
                    if (on) du = __builtin_fmaf(gm[i], v[i], du);
                    if (in) {
                        gn[(int64_t)m * d + k] = on ? gm[i] * uk : 0.f;
                        gn0[(int64_t)m * d + k] = on ? r * v0[i] : 0.f;
                    }
                }
            }
        }
        if (in) {
            gu[k] = du;
            gp[k] = g0 * uk;
            gu0[k] = r * ub0[k];
            gp0[k] = r * pb0[k];
        }
    }
    if (lane == 0) {
        terms[b] = logf(Z) + (zmax - z0);
        terms[B + b] = sq;
        if (coef != nullptr) coef[b * (1 + M)] = g0;
    }
    if (coef != nullptr && lane < M) coef[b * (1 + M) + 1 + lane] = g;
}

// loss = (sum L_b) / B + lambda * (sum squares) / B, summed in lgcn_bpr::k_bpr_reduce's order
static __global__ __launch_bounds__(256) void k_ssm_reduce(const float* __restrict__ terms,
                                                           int32_t B, float lambda,
                                                           float* __restrict__ loss) {
    __shared__ float sl[256], sr[256];
    float a = 0.f, q = 0.f;
    for (int i = threadIdx.x; i < B; i += 256) {
        a += terms[i];
        q += terms[B + i];
    }
    sl[threadIdx.x] = a;
    sr[threadIdx.x] = q;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            sl[threadIdx.x] += sl[threadIdx.x + w];
            sr[threadIdx.x] += sr[threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[0] = sl[0] / (float)B + lambda * sr[0] / (float)B;
}

// both launches of one batch: rows kernel, then the reduction
template <typename Rows>
inline int launch(const Rows& rows, int32_t B, int32_t M, int32_t d, float lambda, float tau,
                  float* terms, float* loss, float* grads, float* coef, hipStream_t s) {
    const int64_t grid = ((int64_t)B + kRowsPerBlock - 1) / kRowsPerBlock;
    hipLaunchKernelGGL(k_ssm_rows<Rows>, dim3((uint32_t)grid), dim3(kWave * kRowsPerBlock), 0, s,
                       rows, B, M, d, lambda, 1.f / tau, terms, grads, coef);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_ssm_reduce, dim3(1), dim3(256), 0, s, terms, B, lambda, loss);
    e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}

}  // namespace lgcn_ssm
#endif  // LGCN_SSM_ROWS_H_

// lgcn_ssm.hip — the sampled-softmax (InfoNCE) loss of one training batch over every drawn
// negative: per sample one softmax over the positive and its M candidate negatives, with a
// temperature, plus the L2 term of the layer-0 rows, and every input gradient.
//   lgcn_ssm_loss          the rows given as gathered blocks
//   lgcn_ssm_loss_indexed  the rows read from the tables by index (the fused step)
//   lgcn_ssm_loss_q, lgcn_ssm_loss_indexed_q  the two with a logQ correction of the logits; the
//                          two above are these with q = NULL
//   lgcn_ssm_keys          the (2+M)B destination keys of the batch's per-sample gradient rows
// Declared in include/lgcn.h; the kernels are in lgcn_ssm_rows.h. The sort, the scatter and the
// clear of the step are the BPR step's (lgcn_coo_sort_perm, lgcn_rows_scatter, lgcn_rows_clear).
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "lgcn.h"
#include "lgcn_ssm_rows.h"

namespace {

using lgcn_ssm::kRowsPerBlock;
using lgcn_ssm::kWave;

// One wave per sample, lane m its candidate m, in the row order of k_ssm_rows' grads: keys
// [0, B) users, [B, 2B) positives, 2B + b * M + m candidates (bit 0 set). A sample the loss
// kernel skips has every key "none"; a candidate that takes no part has its own key "none".
__global__ __launch_bounds__(kWave * kRowsPerBlock) void k_ssm_keys(
    const int64_t* __restrict__ users, const int64_t* __restrict__ pos,
    const int64_t* __restrict__ cand, int32_t B, int32_t M, int64_t n_users, int64_t n_items,
    int64_t* __restrict__ keys) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t b = (int64_t)blockIdx.x * kRowsPerBlock + threadIdx.x / kWave;
    if (b >= B) return;
    const int64_t iu = users[b], ip = pos[b];
    const bool have = iu >= 0 && iu < n_users && ip >= 0 && ip < n_items;
    const int64_t in = lane < M ? cand[b * M + lane] : -1;
    const bool ok = have && in >= 0 && in < n_items;
    const bool any = __ballot(ok) != 0;
    const int64_t none = 2 * (n_users + n_items);  // the key past every row
    if (lane == 0) {
        keys[b] = any ? 2 * iu : none;
        keys[(int64_t)B + b] = any ? 2 * (n_users + ip) : none;
    }
    if (lane < M) keys[2 * (int64_t)B + b * M + lane] = ok ? 2 * (n_users + in) + 1 : none;
}

inline bool sizes_ok(int32_t B, int32_t M, int32_t d) {
    return B >= 1 && d >= 1 && M >= 1 && M <= LGCN_BPR_MAX_NEG &&
           (int64_t)(2 + M) * B <= 0x7fffffffLL;
}

inline bool tau_ok(float tau) { return __builtin_isfinite(tau) && tau > 0.f; }

}  // namespace

extern "C" {

int lgcn_ssm_loss(const float* u, int64_t ldu, const float* p, int64_t ldp, const float* n,
                  int64_t ldn, const float* u0, int64_t ldu0, const float* p0, int64_t ldp0,
                  const float* n0, int64_t ldn0, const uint8_t* valid, int32_t B, int32_t M,
                  int32_t d, float lambda, float temperature, float* terms, float* loss,
                  float* grads, float* coef, void* stream) {
    return lgcn_ssm_loss_q(u, ldu, p, ldp, n, ldn, u0, ldu0, p0, ldp0, n0, ldn0, valid, nullptr,
                           nullptr, B, M, d, lambda, temperature, terms, loss, grads, coef, stream);
}

int lgcn_ssm_loss_q(const float* u, int64_t ldu, const float* p, int64_t ldp, const float* n,
                    int64_t ldn, const float* u0, int64_t ldu0, const float* p0, int64_t ldp0,
                    const float* n0, int64_t ldn0, const uint8_t* valid, const float* q_pos,
                    const float* q_neg, int32_t B, int32_t M, int32_t d, float lambda,
                    float temperature, float* terms, float* loss, float* grads, float* coef,
                    void* stream) {
    if (!sizes_ok(B, M, d) || !tau_ok(temperature) || !loss || !terms || !grads)
        return LGCN_EINVAL;
    if (!u || !p || !n || !u0 || !p0 || !n0) return LGCN_EINVAL;
    if (ldu < d || ldp < d || ldn < d || ldu0 < d || ldp0 < d || ldn0 < d) return LGCN_EINVAL;
    const lgcn_ssm::GatheredRows rows = {{u, p, u0, p0}, {ldu, ldp, ldu0, ldp0}, n, ldn,
                                         n0, ldn0, valid, q_pos, q_neg};
    return lgcn_ssm::launch(rows, B, M, d, lambda, temperature, terms, loss, grads, coef,
                            reinterpret_cast<hipStream_t>(stream));
}

int lgcn_ssm_loss_indexed(const float* fu, int64_t ld_fu, const float* fi, int64_t ld_fi,
                          const float* u0, int64_t ld_u0, const float* i0, int64_t ld_i0,
                          int64_t n_users, int64_t n_items, const int64_t* users,
                          const int64_t* pos, const int64_t* cand, int32_t B, int32_t M,
                          int32_t d, float lambda, float temperature, float* terms, float* loss,
                          float* grads, float* coef, void* stream) {
    return lgcn_ssm_loss_indexed_q(fu, ld_fu, fi, ld_fi, u0, ld_u0, i0, ld_i0, n_users, n_items,
                                   users, pos, cand, nullptr, B, M, d, lambda, temperature, terms,
                                   loss, grads, coef, stream);
}

int lgcn_ssm_loss_indexed_q(const float* fu, int64_t ld_fu, const float* fi, int64_t ld_fi,
                            const float* u0, int64_t ld_u0, const float* i0, int64_t ld_i0,
                            int64_t n_users, int64_t n_items, const int64_t* users,
                            const int64_t* pos, const int64_t* cand, const float* item_q,
                            int32_t B, int32_t M, int32_t d, float lambda, float temperature,
                            float* terms, float* loss, float* grads, float* coef, void* stream) {
    if (!sizes_ok(B, M, d) || !tau_ok(temperature) || !loss || !terms || !grads)
        return LGCN_EINVAL;
    if (!fu || !fi || !u0 || !i0 || !users || !pos || !cand) return LGCN_EINVAL;
    if (ld_fu < d || ld_fi < d || ld_u0 < d || ld_i0 < d) return LGCN_EINVAL;
    if (n_users < 0 || n_items < 0) return LGCN_EINVAL;
    const lgcn_ssm::IndexedRows rows = {{fu, fi, u0, i0}, {ld_fu, ld_fi, ld_u0, ld_i0},
                                        users, pos, cand, n_users, n_items, item_q};
    return lgcn_ssm::launch(rows, B, M, d, lambda, temperature, terms, loss, grads, coef,
                            reinterpret_cast<hipStream_t>(stream));
}

int lgcn_ssm_keys(const int64_t* users, const int64_t* pos, const int64_t* cand, int32_t B,
                  int32_t M, int64_t n_users, int64_t n_items, int64_t* keys, void* stream) {
    if (!sizes_ok(B, M, 1) || !users || !pos || !cand || !keys) return LGCN_EINVAL;
    // every key, the "none" one included, must fit the sort's int32 keys
    if (n_users < 0 || n_items < 0 || n_users + n_items > 0x3ffffffeLL) return LGCN_EINVAL;
    const int64_t grid = ((int64_t)B + kRowsPerBlock - 1) / kRowsPerBlock;
    hipLaunchKernelGGL(k_ssm_keys, dim3((uint32_t)grid), dim3(kWave * kRowsPerBlock), 0,
                       reinterpret_cast<hipStream_t>(stream), users, pos, cand, B, M, n_users,
                       n_items, keys);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}

}  // extern "C"

// lgcn_inbatch.hip — the in-batch softmax loss of one training batch: sample b's negatives are the
// positives of the other samples of its batch, less the ones that are no true negatives of its
// user; a temperature, an optional per-item logQ correction, the L2 term of the layer-0 rows, and
// every input gradient. 2B rows are read, differentiated and scattered, whatever B.
//   lgcn_inbatch_loss          the rows given as gathered blocks, the masks as arrays
//   lgcn_inbatch_loss_indexed  the rows read from the tables by index, the masks derived (the
//                              fused step)
//   lgcn_inbatch_keys          the 2B destination keys of the batch's per-sample gradient rows
// Declared in include/lgcn.h; the kernels are in lgcn_inbatch_rows.h. The sort, the scatter and
// the clear of the step are the BPR step's (lgcn_coo_sort_perm, lgcn_rows_scatter,
// lgcn_rows_clear).
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "lgcn.h"
#include "lgcn_inbatch_rows.h"

namespace {

using lgcn_inb::kRowsPerBlock;
using lgcn_inb::kWave;

// One thread per sample, in the row order of the grads halves: keys [0, B) users, [B, 2B)
// positives (both bit 0 clear). A sample the loss kernels skip has both keys "none".
__global__ __launch_bounds__(kWave * kRowsPerBlock) void k_inb_keys(
    const int64_t* __restrict__ users, const int64_t* __restrict__ pos, int32_t B,
    int64_t n_users, int64_t n_items, int64_t* __restrict__ keys) {
    const int64_t b = (int64_t)blockIdx.x * (kWave * kRowsPerBlock) + threadIdx.x;
    if (b >= B) return;
    const int64_t iu = users[b], ip = pos[b];
    const bool have = iu >= 0 && iu < n_users && ip >= 0 && ip < n_items;
    const int64_t none = 2 * (n_users + n_items);  // the key past every row
    keys[b] = have ? 2 * iu : none;
    keys[(int64_t)B + b] = have ? 2 * (n_users + ip) : none;
}

inline bool sizes_ok(int32_t B, int32_t d) {
    return B >= 1 && B <= LGCN_INBATCH_MAX_B && d >= 1 && d <= LGCN_INBATCH_MAX_D;
}

inline bool tau_ok(float tau) { return __builtin_isfinite(tau) && tau > 0.f; }

}  // namespace

extern "C" {

int lgcn_inbatch_loss(const float* u, int64_t ldu, const float* p, int64_t ldp, const float* u0,
                      int64_t ldu0, const float* p0, int64_t ldp0, const uint8_t* off,
                      const uint8_t* valid, const float* q, int32_t B, int32_t d, float lambda,
                      float temperature, float* work, uint32_t* mask, float* loss, float* grads,
                      float* coef, void* stream) {
    if (!sizes_ok(B, d) || !tau_ok(temperature) || !work || !mask || !loss || !grads)
        return LGCN_EINVAL;
    if (!u || !p || !u0 || !p0) return LGCN_EINVAL;
    if (ldu < d || ldp < d || ldu0 < d || ldp0 < d) return LGCN_EINVAL;
    if (coef != nullptr && B > LGCN_INBATCH_MAX_COEF_B) return LGCN_EINVAL;
    const lgcn_inb::GatheredRows rows = {{u, p, u0, p0}, {ldu, ldp, ldu0, ldp0}, off, valid, q};
    return lgcn_inb::launch(rows, B, d, lambda, temperature, work, mask, loss, grads, coef,
                            reinterpret_cast<hipStream_t>(stream));
}

int lgcn_inbatch_loss_indexed(const float* fu, int64_t ld_fu, const float* fi, int64_t ld_fi,
                              const float* u0, int64_t ld_u0, const float* i0, int64_t ld_i0,
                              int64_t n_users, int64_t n_items, const int64_t* users,
                              const int64_t* pos, const int32_t* pos_rowptr,
                              const int32_t* pos_items, const float* item_q, int32_t B, int32_t d,
                              float lambda, float temperature, float* work, uint32_t* mask,
                              float* loss, float* grads, float* coef, void* stream) {
    if (!sizes_ok(B, d) || !tau_ok(temperature) || !work || !mask || !loss || !grads)
        return LGCN_EINVAL;
    if (!fu || !fi || !u0 || !i0 || !users || !pos) return LGCN_EINVAL;
    if (ld_fu < d || ld_fi < d || ld_u0 < d || ld_i0 < d) return LGCN_EINVAL;
    if (n_users < 0 || n_items < 0) return LGCN_EINVAL;
    if ((pos_rowptr == nullptr) != (pos_items == nullptr)) return LGCN_EINVAL;
    if (coef != nullptr && B > LGCN_INBATCH_MAX_COEF_B) return LGCN_EINVAL;
    const lgcn_inb::IndexedRows rows = {{fu, fi, u0, i0}, {ld_fu, ld_fi, ld_u0, ld_i0}, users, pos,
                                        n_users, n_items, pos_rowptr, pos_items, item_q};
    return lgcn_inb::launch(rows, B, d, lambda, temperature, work, mask, loss, grads, coef,
                            reinterpret_cast<hipStream_t>(stream));
}

int lgcn_inbatch_keys(const int64_t* users, const int64_t* pos, int32_t B, int64_t n_users,
                      int64_t n_items, int64_t* keys, void* stream) {
    if (!sizes_ok(B, 1) || !users || !pos || !keys) return LGCN_EINVAL;
    // every key, the "none" one included, must fit the sort's int32 keys
    if (n_users < 0 || n_items < 0 || n_users + n_items > 0x3ffffffeLL) return LGCN_EINVAL;
    const int per = kWave * kRowsPerBlock;
    hipLaunchKernelGGL(k_inb_keys, dim3((uint32_t)((B + per - 1) / per)), dim3(per), 0,
                       reinterpret_cast<hipStream_t>(stream), users, pos, B, n_users, n_items,
                       keys);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}

}  // extern "C"

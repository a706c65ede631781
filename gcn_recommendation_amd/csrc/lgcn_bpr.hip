// lgcn_bpr.hip — fused BPR loss + regulariser of one training batch (main.py:366-402 on the
// device): the two dot products, log-sigmoid, the L2 term of the layer-0 rows, and every input
// gradient, in one pass over the 6 x B gathered rows; the batch mean is a fixed-order reduction
// (deterministic, run to run). Declared in include/lgcn.h (lgcn_bpr_loss).
//
//   loss = -mean_b log(sigmoid(<u_b,p_b> - <u_b,n_b>) + 1e-8)
//          + lambda * (|U0|^2 + |P0|^2 + |N0|^2) / B
//
// Gradients follow autograd's chain for that expression: c_b = ((-1/B) / (s_b + 1e-8)) *
// (1 - s_b) * s_b (NegBackward, MeanBackward, LogBackward, SigmoidBackward), du = c*p + (-c)*n,
// dp = c*u, dn = (-c)*u, d(row0) = (2*lambda/B) * row0.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "lgcn.h"
#include "lgcn_bpr_rows.h"  // k_bpr_rows / k_bpr_reduce, shared with lgcn_bpr_loss_indexed

extern "C" int lgcn_bpr_loss(const float* u, int64_t ldu, const float* p, int64_t ldp,
                             const float* n, int64_t ldn, const float* u0, int64_t ldu0,
                             const float* p0, int64_t ldp0, const float* n0, int64_t ldn0,
                             int32_t B, int32_t d, float lambda, float* terms, float* loss,
                             float* grads, void* stream) {
    if (B < 1 || d < 1 || !loss || !terms || !grads) return LGCN_EINVAL;
    if (!u || !p || !n || !u0 || !p0 || !n0) return LGCN_EINVAL;
    if (ldu < d || ldp < d || ldn < d || ldu0 < d || ldp0 < d || ldn0 < d) return LGCN_EINVAL;
    const lgcn_bpr::GatheredRows rows = {{u, p, n, u0, p0, n0}, {ldu, ldp, ldn, ldu0, ldp0, ldn0}};
    return lgcn_bpr::launch(rows, B, d, lambda, terms, loss, grads,
                            reinterpret_cast<hipStream_t>(stream));
}

// the same batch with the brand-preference term (main.py:382-391): eight gathered blocks
extern "C" int lgcn_bpr_brand_loss(const float* u, int64_t ldu, const float* p, int64_t ldp,
                                   const float* n, int64_t ldn, const float* u0, int64_t ldu0,
                                   const float* p0, int64_t ldp0, const float* n0, int64_t ldn0,
                                   const float* bp, int64_t ldbp, const float* bn, int64_t ldbn,
                                   const uint8_t* brand_ok, int32_t B, int32_t d, float lambda,
                                   float brand_weight, float* terms, float* loss, float* grads,
                                   float* coef, void* stream) {
    if (B < 1 || d < 1 || !loss || !terms || !grads) return LGCN_EINVAL;
    if (!u || !p || !n || !u0 || !p0 || !n0 || !bp || !bn) return LGCN_EINVAL;
    if (ldu < d || ldp < d || ldn < d || ldu0 < d || ldp0 < d || ldn0 < d || ldbp < d || ldbn < d)
        return LGCN_EINVAL;
    const lgcn_bpr::GatheredBrandRows rows = {{u, p, n, u0, p0, n0, bp, bn},
                                              {ldu, ldp, ldn, ldu0, ldp0, ldn0, ldbp, ldbn},
                                              brand_ok};
    return lgcn_bpr::launch_brand(rows, B, d, lambda, brand_weight, terms, loss, grads, coef,
                                  reinterpret_cast<hipStream_t>(stream));
}

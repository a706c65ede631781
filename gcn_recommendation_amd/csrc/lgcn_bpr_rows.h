// lgcn_bpr_rows.h — the BPR batch kernels shared by lgcn_bpr.hip (rows given as gathered
// [B x d] blocks) and lgcn_bpr_step.hip (rows read from the tables by index): one row kernel,
// templated on how sample b's six row pointers are obtained, and the fixed-order batch reduction;
// below them their siblings with the brand-preference term (eight rows per sample). row_scores,
// how all of them form a score, is also what lgcn_bpr_select_hardest ranks candidates by.
//
//   loss = -mean_b log(sigmoid(<u_b,p_b> - <u_b,n_b>) + 1e-8)
//          + lambda * (|U0|^2 + |P0|^2 + |N0|^2) / B
//
// Gradients follow autograd's chain for that expression: c_b = ((-1/B) / (s_b + 1e-8)) *
// (1 - s_b) * s_b (NegBackward, MeanBackward, LogBackward, SigmoidBackward), du = c*p + (-c)*n,
// dp = c*u, dn = (-c)*u, d(row0) = (2*lambda/B) * row0.
#ifndef LGCN_BPR_ROWS_H_
#define LGCN_BPR_ROWS_H_

#include <hip/hip_runtime.h>

#include <stdint.h>

namespace lgcn_bpr {

constexpr int kWave = 64;
constexpr int kRowsPerBlock = 4;  // one wave per batch row

// the six rows of one sample: u, p, n (final) and u0, p0, n0 (layer 0)
struct SampleRows {
    const float* r[6];
};

// rows of six gathered blocks: sample b is row b of each
struct GatheredRows {
    const float* p[6];
    int64_t ld[6];
    __device__ __forceinline__ bool get(int64_t b, SampleRows& o) const {
#pragma unroll
        for (int i = 0; i < 6; ++i) o.r[i] = p[i] + b * ld[i];
        return true;
    }
};

// rows of the tables themselves: sample b is (users[b], pos[b], neg[b]); tab = final user, final
// item, layer-0 user, layer-0 item. A sample with an index outside its table has no rows (false)
// and nothing of it is dereferenced.
struct IndexedRows {
    const float* tab[4];
    int64_t ld[4];
    const int64_t* users;
    const int64_t* pos;
    const int64_t* neg;
    int64_t n_users, n_items;
    __device__ __forceinline__ bool get(int64_t b, SampleRows& o) const {
        const int64_t iu = users[b], ip = pos[b], in = neg[b];
        if (iu < 0 || iu >= n_users || ip < 0 || ip >= n_items || in < 0 || in >= n_items)
            return false;
        o.r[0] = tab[0] + iu * ld[0];
        o.r[1] = tab[1] + ip * ld[1];
        o.r[2] = tab[1] + in * ld[1];
        o.r[3] = tab[2] + iu * ld[2];
        o.r[4] = tab[3] + ip * ld[3];
        o.r[5] = tab[3] + in * ld[3];
        return true;
    }
};

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
    return v;
}

// The scores s[i] = <u, v[i]> of one user row against N item (or brand) rows, the one statement of
// how a batch kernel forms a score: per lane an fmaf chain over k = lane, lane + 64, ... from +0,
// then wave_sum; every lane returns the sum. A score is a function of its two rows alone: N only
// sets how many rows' loads are in flight.
template <int N>
__device__ __forceinline__ void row_scores(const float* u, const float* const (&v)[N], int32_t d,
                                           int lane, float (&s)[N]) {
#pragma unroll
    for (int i = 0; i < N; ++i) s[i] = 0.f;
    for (int k = lane; k < d; k += kWave) {
        const float x = u[k];
#pragma unroll
        for (int i = 0; i < N; ++i) s[i] = __builtin_fmaf(x, v[i][k], s[i]);
    }
#pragma unroll
    for (int i = 0; i < N; ++i) s[i] = wave_sum(s[i]);
}

// grads = [6 x B x d] (u, p, n, u0, p0, n0); terms = [2 x B] (log term, squared norms). A sample
// without rows (Rows::get false) contributes zero terms and zero gradient rows.
template <typename Rows>
__global__ __launch_bounds__(kWave * kRowsPerBlock) void k_bpr_rows(
    Rows rows, int32_t B, int32_t d, float lambda, float* __restrict__ terms,
    float* __restrict__ grads) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t b = (int64_t)blockIdx.x * kRowsPerBlock + threadIdx.x / kWave;
    if (b >= B) return;
    const int64_t bd = (int64_t)B * d;
    float* gu = grads;
    float* gp = grads + bd;
    float* gn = grads + 2 * bd;
    float* gu0 = grads + 3 * bd;
    float* gp0 = grads + 4 * bd;
    float* gn0 = grads + 5 * bd;
    SampleRows sr;
    if (!rows.get(b, sr)) {
        for (int k = lane; k < d; k += kWave) {
            const int64_t o = b * (int64_t)d + k;
            gu[o] = gp[o] = gn[o] = gu0[o] = gp0[o] = gn0[o] = 0.f;
        }
        if (lane == 0) terms[b] = terms[B + b] = 0.f;
        return;
    }
    const float* ub = sr.r[0];
    const float* pb = sr.r[1];
    const float* nb = sr.r[2];
    const float* ub0 = sr.r[3];
    const float* pb0 = sr.r[4];
    const float* nb0 = sr.r[5];
    float sq = 0.f;
    for (int k = lane; k < d; k += kWave) {
        sq = __builtin_fmaf(ub0[k], ub0[k], sq);
        sq = __builtin_fmaf(pb0[k], pb0[k], sq);
        sq = __builtin_fmaf(nb0[k], nb0[k], sq);
    }
    const float* const pn[2] = {pb, nb};
    float sc[2];  // sp, sn
    row_scores(ub, pn, d, lane, sc);
    sq = wave_sum(sq);
    const float x = sc[0] - sc[1];
    const float s = 1.f / (1.f + expf(-x));
    const float c = ((-1.f / (float)B) / (s + 1e-8f)) * (1.f - s) * s;
    const float r = 2.f * lambda / (float)B;
    for (int k = lane; k < d; k += kWave) {
        const int64_t o = b * (int64_t)d + k;
        gu[o] = c * pb[k] + (-c) * nb[k];
        gp[o] = c * ub[k];
        gn[o] = (-c) * ub[k];
        gu0[o] = r * ub0[k];
        gp0[o] = r * pb0[k];
        gn0[o] = r * nb0[k];
    }
    if (lane == 0) {
        terms[b] = logf(s + 1e-8f);
        terms[B + b] = sq;
    }
}

// loss = -(sum log terms) / B + lambda * (sum squares) / B, summed in a fixed order
static __global__ __launch_bounds__(256) void k_bpr_reduce(const float* __restrict__ terms,
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
    if (threadIdx.x == 0) loss[0] = -(sl[0] / (float)B) + lambda * sr[0] / (float)B;
}

// both launches of one batch: rows kernel, then the reduction
template <typename Rows>
inline int launch(const Rows& rows, int32_t B, int32_t d, float lambda, float* terms, float* loss,
                  float* grads, hipStream_t s) {
    const int64_t grid = ((int64_t)B + kRowsPerBlock - 1) / kRowsPerBlock;
    hipLaunchKernelGGL(k_bpr_rows<Rows>, dim3((uint32_t)grid), dim3(kWave * kRowsPerBlock), 0, s,
                       rows, B, d, lambda, terms, grads);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_bpr_reduce, dim3(1), dim3(256), 0, s, terms, B, lambda, loss);
    e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}

// ---- the batch with the brand-preference term (main.py:382-391, 499-522) ------------------------
//   loss = (bpr + w * -mean_b log(sigmoid(<u_b,bp_b> - <u_b,bn_b>) + 1e-8)) + reg
// bp / bn = the final brand rows of the sample's positive / negative item. The brand term's chain
// is the base one with -w/B for -1/B: c'_b = ((-w/B) / (s'_b + 1e-8)) * (1 - s'_b) * s'_b,
// du += c'*bp + (-c')*bn, dbp = c'*u, dbn = (-c')*u. A sample without brand rows (kBase) has no
// brand term: c' = 0, a zero log term, +0 brand gradient rows, and the base kernel's du.

// the eight rows of one sample: SampleRows' six, then bp, bn (final brand rows)
struct BrandSampleRows {
    const float* r[8];
};

enum { kSkip = 0, kBase = 1, kBrand = 2 };  // what Rows::get found of a sample

// rows of eight gathered blocks; brand_ok (NULL = every sample) tells per sample whether rows b of
// the two brand blocks are its brand rows
struct GatheredBrandRows {
    const float* p[8];
    int64_t ld[8];
    const uint8_t* brand_ok;
    __device__ __forceinline__ int get(int64_t b, BrandSampleRows& o) const {
#pragma unroll
        for (int i = 0; i < 8; ++i) o.r[i] = p[i] + b * ld[i];
        return (brand_ok == nullptr || brand_ok[b]) ? kBrand : kBase;
    }
};

// IndexedRows plus the final brand table fb, looked up through item_brand (int32 [n_items]; a
// value outside [0, n_brands), -1 by convention, = the item has no brand)
struct IndexedBrandRows {
    IndexedRows base;
    const float* fb;
    int64_t ld_fb;
    const int32_t* item_brand;
    int64_t n_brands;
    __device__ __forceinline__ int get(int64_t b, BrandSampleRows& o) const {
        SampleRows s;
        if (!base.get(b, s)) return kSkip;
#pragma unroll
        for (int i = 0; i < 6; ++i) o.r[i] = s.r[i];
        const int64_t rp = item_brand[base.pos[b]], rn = item_brand[base.neg[b]];
        if (rp < 0 || rp >= n_brands || rn < 0 || rn >= n_brands) {
            o.r[6] = o.r[7] = nullptr;
            return kBase;
        }
        o.r[6] = fb + rp * ld_fb;
        o.r[7] = fb + rn * ld_fb;
        return kBrand;
    }
};

// grads = [8 x B x d] in the order u0, p0, n0, u, p, n, bp, bn: the three layer-0 blocks, then the
// five final-row blocks as one [5B x d] source of the scatter. terms = [3 x B] (log term, squared
// norms, brand log term); coef (nullptr = not wanted) = [2 x B] (c, c'). The base quantities are
// computed by k_bpr_rows' own expressions, in its order.
template <typename Rows>
__global__ __launch_bounds__(kWave * kRowsPerBlock) void k_bpr_brand_rows(
    Rows rows, int32_t B, int32_t d, float lambda, float w, float* __restrict__ terms,
    float* __restrict__ grads, float* __restrict__ coef) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t b = (int64_t)blockIdx.x * kRowsPerBlock + threadIdx.x / kWave;
    if (b >= B) return;
    const int64_t bd = (int64_t)B * d;
    float* gu0 = grads;
    float* gp0 = grads + bd;
    float* gn0 = grads + 2 * bd;
    float* gu = grads + 3 * bd;
    float* gp = grads + 4 * bd;
    float* gn = grads + 5 * bd;
    float* gbp = grads + 6 * bd;
    float* gbn = grads + 7 * bd;
    BrandSampleRows sr;
    const int kind = rows.get(b, sr);
    if (kind == kSkip) {
        for (int k = lane; k < d; k += kWave) {
            const int64_t o = b * (int64_t)d + k;
            gu[o] = gp[o] = gn[o] = gu0[o] = gp0[o] = gn0[o] = gbp[o] = gbn[o] = 0.f;
        }
        if (lane == 0) {
            terms[b] = terms[B + b] = terms[2 * (int64_t)B + b] = 0.f;
            if (coef != nullptr) coef[b] = coef[B + b] = 0.f;
        }
        return;
    }
    const bool brand = kind == kBrand;
    const float* ub = sr.r[0];
    const float* pb = sr.r[1];
    const float* nb = sr.r[2];
    const float* ub0 = sr.r[3];
    const float* pb0 = sr.r[4];
    const float* nb0 = sr.r[5];
    const float* bpb = sr.r[6];  // read only when brand
    const float* bnb = sr.r[7];
    float sq = 0.f;
    for (int k = lane; k < d; k += kWave) {
        sq = __builtin_fmaf(ub0[k], ub0[k], sq);
        sq = __builtin_fmaf(pb0[k], pb0[k], sq);
        sq = __builtin_fmaf(nb0[k], nb0[k], sq);
    }
    const float* const pn[2] = {pb, nb};
    float sc[2], tc[2] = {0.f, 0.f};  // sp, sn and tp, tn
    row_scores(ub, pn, d, lane, sc);
    if (brand) {  // uniform over the wave: one sample per wave
        const float* const bpn[2] = {bpb, bnb};
        row_scores(ub, bpn, d, lane, tc);
    }
    sq = wave_sum(sq);
    const float sp = sc[0], sn = sc[1], tp = tc[0], tn = tc[1];
    const float x = sp - sn;
    const float s = 1.f / (1.f + expf(-x));
    const float c = ((-1.f / (float)B) / (s + 1e-8f)) * (1.f - s) * s;
    const float r = 2.f * lambda / (float)B;
    float cb = 0.f, lb = 0.f;
    if (brand) {
        const float xb = tp - tn;
        const float sb = 1.f / (1.f + expf(-xb));
        cb = ((-w / (float)B) / (sb + 1e-8f)) * (1.f - sb) * sb;
        lb = logf(sb + 1e-8f);
    }
    for (int k = lane; k < d; k += kWave) {
        const int64_t o = b * (int64_t)d + k;
        const float base = c * pb[k] + (-c) * nb[k];
        if (brand) {
            gu[o] = base + (cb * bpb[k] + (-cb) * bnb[k]);
            gbp[o] = cb * ub[k];
            gbn[o] = (-cb) * ub[k];
        } else {
            gu[o] = base;
            gbp[o] = gbn[o] = 0.f;
        }
        gp[o] = c * ub[k];
        gn[o] = (-c) * ub[k];
        gu0[o] = r * ub0[k];
        gp0[o] = r * pb0[k];
        gn0[o] = r * nb0[k];
    }
    if (lane == 0) {
        terms[b] = logf(s + 1e-8f);
        terms[B + b] = sq;
        terms[2 * (int64_t)B + b] = lb;
        if (coef != nullptr) {
            coef[b] = c;
            coef[B + b] = cb;
        }
    }
}

// loss = (-(sl / B) + w * -(sb / B)) + lambda * sr / B: torch's (bpr + w * brand) + reg, the three
// sums in k_bpr_reduce's fixed order
static __global__ __launch_bounds__(256) void k_bpr_brand_reduce(const float* __restrict__ terms,
                                                                 int32_t B, float lambda, float w,
                                                                 float* __restrict__ loss) {
    __shared__ float sl[256], sr[256], sb[256];
    float a = 0.f, q = 0.f, t = 0.f;
    for (int i = threadIdx.x; i < B; i += 256) {
        a += terms[i];
        q += terms[B + i];
        t += terms[2 * (int64_t)B + i];
    }
    sl[threadIdx.x] = a;
    sr[threadIdx.x] = q;
    sb[threadIdx.x] = t;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) {
            sl[threadIdx.x] += sl[threadIdx.x + h];
            sr[threadIdx.x] += sr[threadIdx.x + h];
            sb[threadIdx.x] += sb[threadIdx.x + h];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0)
        loss[0] = (-(sl[0] / (float)B) + w * -(sb[0] / (float)B)) + lambda * sr[0] / (float)B;
}

template <typename Rows>
inline int launch_brand(const Rows& rows, int32_t B, int32_t d, float lambda, float w,
                        float* terms, float* loss, float* grads, float* coef, hipStream_t s) {
    const int64_t grid = ((int64_t)B + kRowsPerBlock - 1) / kRowsPerBlock;
    hipLaunchKernelGGL(k_bpr_brand_rows<Rows>, dim3((uint32_t)grid),
                       dim3(kWave * kRowsPerBlock), 0, s, rows, B, d, lambda, w, terms, grads,
                       coef);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_bpr_brand_reduce, dim3(1), dim3(256), 0, s, terms, B, lambda, w, loss);
    e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}

}  // namespace lgcn_bpr
#endif  // LGCN_BPR_ROWS_H_

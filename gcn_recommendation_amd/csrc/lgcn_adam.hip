// lgcn_adam.hip — one Adam step over up to LGCN_ADAM_MAX_TENSORS fp32 tensors in ONE launch for
// gfx950, bit for bit torch.optim.Adam's default on a HIP device (torch 2.10 _multi_tensor_adam,
// non-capturable branch: seven _foreach passes, each writing a rounded fp32 intermediate).
//
//  * the descriptor table travels by value in the kernel arguments (AdamArgs, < 1 KB): no copy,
//    no synchronisation, capture-safe;
//  * a block takes one chunk of LGCN_ADAM_CHUNK consecutive elements of one tensor; it finds its
//    tensor by a scan of the (wave-uniform) prefix of chunk counts in the arguments;
//  * a tensor whose p, g, m, v are all 16-B aligned moves as 16-B vectors: a full chunk issues all
//    of its 16 loads per lane before the first use; the last chunk is guarded, its n % 4 tail by
//    element. Any other tensor goes by element. Offsets are 64-bit (chunk index * CHUNK);
//  * 7 streams of 4 B per element (4 read, 3 written), ~20 flops: HBM-bound.
//
// Rounding. The engine is built with -ffp-contract=off; ATen's kernels with hipcc's default
// contraction, which fuses every a + s*x of the foreach functors. So each of those shapes is an
// explicit __fmaf_rn here, and nothing else is fused:
//     weight decay  g' = fma(wd, p, g)                    BinaryOpListAlphaFunctor: a + alpha*b
//     lerp          m  = fma(w, g'-m, m)                  |w| < 0.5
//                   m  = fma(-(1-w), g'-m, g')            otherwise: a - b*c contracts the same, and
//                                                         ATen's code negates 1-w, not g'-m: a NaN
//                                                         keeps its sign bit
//     addcmul       v  = fma(1-beta2, g'*g', v*beta2)     the inner product g'*g' is rounded
//     addcdiv       p  = fma(step_size, m/t, p)           the quotient is rounded
// t = sqrt(v) / bc2_sqrt + eps: IEEE square root, a true IEEE division (no reciprocal), one add;
// m / t IEEE as well — hipcc's defaults for HIP, which is how ATen is built too.
// tests/test_gpu_adam.py compares p, m and v as bit patterns with torch after every step
// (DESIGN.md §5 "Optimizer").
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "lgcn.h"

// non-temporal loads of g, m, v and stores of m, v: nothing reads them again before they leave
// the caches (p is the next forward's input and keeps plain accesses). Measured faster than plain
// accesses at C3's table sizes, both builds in one process (tools/adam_bench.py --ab-lib; the
// figures: profiles/adam_nt_ab_c3.log, DESIGN.md §5 "Optimizer"); -DLGCN_ADAM_NT=0 builds the other.
#ifndef LGCN_ADAM_NT
#define LGCN_ADAM_NT 1
#endif

namespace {

constexpr int kAdamThreads = 256;
constexpr int kAdamVecs = LGCN_ADAM_CHUNK / (4 * kAdamThreads);  // 16-B vectors per lane and stream
constexpr int64_t kAdamMaxChunks = (1 << 24) - 1;  // grid * block stays below 2^32 threads
static_assert(LGCN_ADAM_CHUNK % (4 * kAdamThreads) == 0 && kAdamVecs >= 1, "chunk");

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct AdamArgs {
    float* p[LGCN_ADAM_MAX_TENSORS];
    const float* g[LGCN_ADAM_MAX_TENSORS];
    float* m[LGCN_ADAM_MAX_TENSORS];
    float* v[LGCN_ADAM_MAX_TENSORS];
    int64_t n[LGCN_ADAM_MAX_TENSORS];
    int64_t chunk_end[LGCN_ADAM_MAX_TENSORS];  // chunks of tensors 0..t (unused slots: the total)
    float step_size[LGCN_ADAM_MAX_TENSORS];
    float bc2_sqrt[LGCN_ADAM_MAX_TENSORS];
    float lerp_w, beta2, one_minus_beta2, eps, wd;
    uint32_t vec_mask;  // bit t: p, g, m, v of tensor t are all 16-B aligned
    int32_t decay;      // weight_decay != 0 as a double, which is what adam.py tests
};

struct AdamCoef {
    float w, neg_one_minus_w, beta2, one_minus_beta2, eps, wd, step_size, bc2_sqrt;
    bool w_small, decay;
};

template <typename T>
__device__ __forceinline__ T ld_stream(const T* p) {
#if LGCN_ADAM_NT
    return __builtin_nontemporal_load(p);
#else
    return *p;
#endif
}

template <typename T>
__device__ __forceinline__ void st_stream(T* p, T x) {
#if LGCN_ADAM_NT
    __builtin_nontemporal_store(x, p);
#else
    *p = x;
#endif
}

__device__ __forceinline__ void adam_elem(float& p, float g, float& m, float& v,
                                          const AdamCoef& c) {
    if (c.decay) g = __fmaf_rn(c.wd, p, g);
    const float d = g - m;
    m = c.w_small ? __fmaf_rn(c.w, d, m) : __fmaf_rn(c.neg_one_minus_w, d, g);
    v = __fmaf_rn(c.one_minus_beta2, g * g, v * c.beta2);
    float t = sqrtf(v);
    t = t / c.bc2_sqrt;
    t = t + c.eps;
    p = __fmaf_rn(c.step_size, m / t, p);
}

__device__ __forceinline__ void adam_vec(f32x4& p, const f32x4& g, f32x4& m, f32x4& v,
                                         const AdamCoef& c) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float pj = p[j], mj = m[j], vj = v[j];
        adam_elem(pj, g[j], mj, vj, c);
        p[j] = pj;
        m[j] = mj;
        v[j] = vj;
    }
}

__global__ __launch_bounds__(kAdamThreads) void k_adam(const AdamArgs a) {
    const int64_t b = blockIdx.x;
    int t = 0;
    while (t < LGCN_ADAM_MAX_TENSORS - 1 && b >= a.chunk_end[t]) ++t;
    const int64_t beg = (b - (t ? a.chunk_end[t - 1] : 0)) * LGCN_ADAM_CHUNK;
    const int64_t left = a.n[t] - beg;
    if (left <= 0) return;
    const int len = left < LGCN_ADAM_CHUNK ? (int)left : LGCN_ADAM_CHUNK;
    float* __restrict__ p = a.p[t] + beg;
    const float* __restrict__ g = a.g[t] + beg;
    float* __restrict__ m = a.m[t] + beg;
    float* __restrict__ v = a.v[t] + beg;
    AdamCoef c;
    c.w = a.lerp_w;
    c.neg_one_minus_w = -(1.0f - a.lerp_w);
    c.w_small = fabsf(a.lerp_w) < 0.5f;
    c.beta2 = a.beta2;
    c.one_minus_beta2 = a.one_minus_beta2;
    c.eps = a.eps;
    c.wd = a.wd;
    c.decay = a.decay != 0;
    c.step_size = a.step_size[t];
    c.bc2_sqrt = a.bc2_sqrt[t];
    const int tid = threadIdx.x;

    if (!((a.vec_mask >> t) & 1u)) {  // a misaligned pointer: by element
        for (int i = tid; i < len; i += kAdamThreads) {
            float pp = p[i], mm = ld_stream(m + i), vv = ld_stream(v + i);
            adam_elem(pp, ld_stream(g + i), mm, vv, c);
            p[i] = pp;
            st_stream(m + i, mm);
            st_stream(v + i, vv);
        }
        return;
    }
    // beg is a multiple of the chunk, so the chunk's pointers keep the tensor's alignment
    f32x4* __restrict__ p4 = reinterpret_cast<f32x4*>(p);
    const f32x4* __restrict__ g4 = reinterpret_cast<const f32x4*>(g);
    f32x4* __restrict__ m4 = reinterpret_cast<f32x4*>(m);
    f32x4* __restrict__ v4 = reinterpret_cast<f32x4*>(v);
    if (len == LGCN_ADAM_CHUNK) {
        f32x4 pp[kAdamVecs], gg[kAdamVecs], mm[kAdamVecs], vv[kAdamVecs];
#pragma unroll
        for (int k = 0; k < kAdamVecs; ++k) {
            const int i = k * kAdamThreads + tid;
            pp[k] = p4[i];
            gg[k] = ld_stream(g4 + i);
            mm[k] = ld_stream(m4 + i);
            vv[k] = ld_stream(v4 + i);
        }
#pragma unroll
        for (int k = 0; k < kAdamVecs; ++k) {
            const int i = k * kAdamThreads + tid;
            adam_vec(pp[k], gg[k], mm[k], vv[k], c);
            p4[i] = pp[k];
            st_stream(m4 + i, mm[k]);
            st_stream(v4 + i, vv[k]);
        }
        return;
    }
    const int nv = len >> 2;
    for (int i = tid; i < nv; i += kAdamThreads) {
        f32x4 pp = p4[i], mm = ld_stream(m4 + i), vv = ld_stream(v4 + i);
        adam_vec(pp, ld_stream(g4 + i), mm, vv, c);
        p4[i] = pp;
        st_stream(m4 + i, mm);
        st_stream(v4 + i, vv);
    }
    const int i = 4 * nv + tid;  // the n % 4 tail
    if (i < len) {
        float pp = p[i], mm = m[i], vv = v[i];
        adam_elem(pp, g[i], mm, vv, c);
        p[i] = pp;
        m[i] = mm;
        v[i] = vv;
    }
}

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

extern "C" {

int64_t lgcn_adam_chunks(int64_t n) {
    if (n <= 0) return 0;
    return n / LGCN_ADAM_CHUNK + (n % LGCN_ADAM_CHUNK != 0);
}

int lgcn_adam_step(const lgcn_adam_tensor_t* tensors_host, int32_t n_tensors,
                   const lgcn_adam_hyper_t* hyper, void* stream) {
    if (n_tensors < 0 || n_tensors > LGCN_ADAM_MAX_TENSORS) return LGCN_EINVAL;
    if (n_tensors == 0) return 0;
    if (!tensors_host || !hyper) return LGCN_EINVAL;
    if (!isfinite(hyper->lerp_w) || !isfinite(hyper->beta2) || !isfinite(hyper->one_minus_beta2) ||
        !isfinite(hyper->eps) || !isfinite(hyper->weight_decay))
        return LGCN_EINVAL;
    AdamArgs a = {};
    int k = 0;  // tensors with n > 0, packed
    int64_t chunks = 0;
    for (int32_t t = 0; t < n_tensors; ++t) {
        const lgcn_adam_tensor_t& d = tensors_host[t];
        // step_size is not checked: torch accepts lr = inf and the kernel then forms what
        // _foreach_addcdiv_ forms; a bc2_sqrt that is 0, negative or NaN has no torch counterpart
        if (d.n < 0 || !(d.bc2_sqrt > 0.0)) return LGCN_EINVAL;
        if (d.n == 0) continue;
        if (!d.p || !d.g || !d.m || !d.v) return LGCN_EINVAL;
        chunks += lgcn_adam_chunks(d.n);
        if (chunks > kAdamMaxChunks) return LGCN_EINVAL;
        a.p[k] = d.p;
        a.g[k] = d.g;
        a.m[k] = d.m;
        a.v[k] = d.v;
        a.n[k] = d.n;
        a.chunk_end[k] = chunks;
        a.step_size[k] = (float)d.step_size;
        a.bc2_sqrt[k] = (float)d.bc2_sqrt;
        if (al16(d.p) && al16(d.g) && al16(d.m) && al16(d.v)) a.vec_mask |= 1u << k;
        ++k;
    }
    if (k == 0) return 0;
    for (int t = k; t < LGCN_ADAM_MAX_TENSORS; ++t) a.chunk_end[t] = chunks;
    a.lerp_w = (float)hyper->lerp_w;
    a.beta2 = (float)hyper->beta2;
    a.one_minus_beta2 = (float)hyper->one_minus_beta2;
    a.eps = (float)hyper->eps;
    a.wd = (float)hyper->weight_decay;
    a.decay = hyper->weight_decay != 0.0;
    hipLaunchKernelGGL(k_adam, dim3((uint32_t)chunks), dim3(kAdamThreads), 0,
                       reinterpret_cast<hipStream_t>(stream), a);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}

}  // extern "C"

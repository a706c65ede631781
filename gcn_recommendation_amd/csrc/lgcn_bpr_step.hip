// lgcn_bpr_step.hip — the pieces of a fused BPR training step that know the batch indices
// (main.py:495-525 without autograd's six gathers and six dense IndexBackward blocks):
//   lgcn_bpr_loss_indexed  the BPR + L2 loss of lgcn_bpr_loss, rows read from the tables by index
//   lgcn_bpr_select_hardest  per sample the highest-scoring of n_neg candidate negatives, scored
//                          by the loss kernel's own expression: the step then trains on it
//   lgcn_bpr_keys          the 3B destination keys of a batch's per-sample gradient rows
//   lgcn_bpr_brand_loss_indexed / lgcn_bpr_brand_keys   both with the brand-preference term: the
//                          brand rows found through a device-resident item -> brand map, 5B keys
//   lgcn_rows_scatter      deterministic scatter-accumulate of per-sample rows into table rows
//   lgcn_rows_clear        zero exactly the rows (and mask words) a scatter touched
// Declared in include/lgcn.h.
//
// Summation order of the scatter = autograd's (IndexBackward's index_put into zeros, then the sum
// of the positive and negative item blocks): per destination row and column, each run starts
// from +0 and adds its contributions in ascending batch position; a row with a positive
// (key bit 0 clear) and a negative (set) run is (+0 + sum pos) + (+0 + sum neg). A missing run is
// +0, and x + (+0) == x for every x a run from +0 can produce (never -0). Plain fp32 adds, no
// float atomics.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "lgcn.h"
#include "lgcn_bpr_rows.h"

namespace {

constexpr int kWave = 64;
constexpr int kWavesPerBlock = 4;

__global__ __launch_bounds__(256) void k_bpr_keys(const int64_t* __restrict__ users,
                                                  const int64_t* __restrict__ pos,
                                                  const int64_t* __restrict__ neg, int32_t B,
                                                  int64_t n_users, int64_t n_items,
                                                  int64_t* __restrict__ keys) {
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    const int64_t iu = users[b], ip = pos[b], in = neg[b];
    const bool ok = iu >= 0 && iu < n_users && ip >= 0 && ip < n_items && in >= 0 && in < n_items;
    const int64_t none = 2 * (n_users + n_items);  // a skipped sample: the key past every row
    keys[b] = ok ? 2 * iu : none;
    keys[(int64_t)B + b] = ok ? 2 * (n_users + ip) : none;
    keys[2 * (int64_t)B + b] = ok ? 2 * (n_users + in) + 1 : none;
}

// The 5B keys of a batch with the brand term: k_bpr_keys' three, then the positive and the
// negative item's brand row (U + I + brand). A sample without a brand keeps its first three.
__global__ __launch_bounds__(256) void k_bpr_brand_keys(
    const int64_t* __restrict__ users, const int64_t* __restrict__ pos,
    const int64_t* __restrict__ neg, const int32_t* __restrict__ item_brand, int32_t B,
    int64_t n_users, int64_t n_items, int64_t n_brands, int64_t* __restrict__ keys) {
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    const int64_t iu = users[b], ip = pos[b], in = neg[b];
    const bool ok = iu >= 0 && iu < n_users && ip >= 0 && ip < n_items && in >= 0 && in < n_items;
    const int64_t first = n_users + n_items;
    const int64_t none = 2 * (first + n_brands);  // the key past every row
    int64_t rp = -1, rn = -1;
    if (ok) {
        rp = item_brand[ip];
        rn = item_brand[in];
    }
    const bool brand = ok && rp >= 0 && rp < n_brands && rn >= 0 && rn < n_brands;
    keys[b] = ok ? 2 * iu : none;
    keys[(int64_t)B + b] = ok ? 2 * (n_users + ip) : none;
    keys[2 * (int64_t)B + b] = ok ? 2 * (n_users + in) + 1 : none;
    keys[3 * (int64_t)B + b] = brand ? 2 * (first + rp) : none;
    keys[4 * (int64_t)B + b] = brand ? 2 * (first + rn) + 1 : none;
}

constexpr int kSelectRows = 4;  // candidate rows whose loads are in flight together

// One wave per sample: the hardest of its n_neg candidates (include/lgcn.h states the rule). Lane
// m holds candidate m's index, so the indices are gathered before the first row load; the valid
// ones are then scored kSelectRows at a time, in ascending ordinal, by the loss kernel's own
// row_scores. A short last group repeats its first candidate and does not compare the repeats.
__global__ __launch_bounds__(kWave * lgcn_bpr::kRowsPerBlock) void k_bpr_select_hardest(
    const float* __restrict__ fu, int64_t ld_fu, const float* __restrict__ fi, int64_t ld_fi,
    int64_t n_users, int64_t n_items, const int64_t* __restrict__ users,
    const int64_t* __restrict__ cand, int32_t B, int32_t n_neg, int32_t d,
    int64_t* __restrict__ neg_out, float* __restrict__ score_out) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t b = (int64_t)blockIdx.x * lgcn_bpr::kRowsPerBlock + threadIdx.x / kWave;
    if (b >= B) return;
    const int64_t iu = users[b];
    const int64_t mine = lane < n_neg ? cand[b * n_neg + lane] : -1;
    const bool ok = iu >= 0 && iu < n_users && mine >= 0 && mine < n_items;
    uint64_t todo = __ballot(ok);
    int64_t best = -1;
    float best_s = __builtin_nanf("");
    if (todo != 0) {
        const float* ub = fu + iu * ld_fu;
        while (todo != 0) {
            int64_t item[kSelectRows];
            const float* rows[kSelectRows];
            int n = 0;
#pragma unroll
            for (int i = 0; i < kSelectRows; ++i) {
                if (todo != 0) {  // uniform over the wave; true for i = 0
                    item[i] = __shfl(mine, __builtin_ctzll(todo), kWave);  // ascending ordinal
                    todo &= todo - 1;
                    n = i + 1;
                } else {
                    item[i] = item[0];
                }
                rows[i] = fi + item[i] * ld_fi;
            }
            float sc[kSelectRows];
            lgcn_bpr::row_scores(ub, rows, d, lane, sc);
#pragma unroll
            for (int i = 0; i < kSelectRows; ++i)
                if (i < n && (best < 0 || sc[i] > best_s)) {
                    best = item[i];
                    best_s = sc[i];
                }
        }
    }
    if (lane == 0) {
        neg_out[b] = best;
        if (score_out != nullptr) score_out[b] = best_s;
    }
}

// One wave per sorted position; the wave at the head of a run of equal rows (key >> 1) walks the
// run sequentially, lanes across columns. Rows outside [row_lo, row_hi) are left alone.
template <int MODE>
__global__ __launch_bounds__(kWave * kWavesPerBlock) void k_rows_scatter(
    const int32_t* __restrict__ keys, const int32_t* __restrict__ perm, int32_t n,
    const float* __restrict__ src, int64_t ld_src, int32_t row_lo, int32_t row_hi,
    float* __restrict__ dst, int64_t ld_dst, int32_t d, uint32_t* __restrict__ mask,
    int32_t* __restrict__ count) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t i = (int64_t)blockIdx.x * kWavesPerBlock + threadIdx.x / kWave;
    if (i >= n) return;
    const int32_t row = keys[i] >> 1;
    if (row < row_lo || row >= row_hi) return;
    if (i > 0 && (keys[i - 1] >> 1) == row) return;  // not the head of its run
    float* out = dst + (int64_t)(row - row_lo) * ld_dst;
    bool nz = false;
    for (int c = lane; c < d; c += kWave) {
        float ap = 0.f, an = 0.f;
        for (int64_t j = i; j < n; ++j) {
            const int32_t k = keys[j];
            if ((k >> 1) != row) break;
            const int32_t r = perm[j];
            if (r < 0 || r >= n) continue;  // a permutation never holds one: memory safety only
            const float v = src[(int64_t)r * ld_src + c];
            if (k & 1) an = an + v;
            else ap = ap + v;
        }
        const float acc = ap + an;
        if (MODE == LGCN_SCATTER_ADD) {
            out[c] = out[c] + acc;
        } else {
            out[c] = acc;
            nz |= !(acc == 0.f);
        }
    }
    if (MODE == LGCN_SCATTER_STORE && mask != nullptr) {
        if (__any(nz) && lane == 0) {
            const int32_t bit = row - row_lo;
            atomicOr(&mask[bit >> 5], 1u << (bit & 31));
            if (count != nullptr) atomicAdd(count, 1);
        }
    }
}

__global__ __launch_bounds__(kWave * kWavesPerBlock) void k_rows_clear(
    const int32_t* __restrict__ keys, int32_t n, int32_t row_lo, int32_t row_hi,
    float* __restrict__ dst, int64_t ld_dst, int32_t d, uint32_t* __restrict__ mask,
    int32_t* __restrict__ count) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t i = (int64_t)blockIdx.x * kWavesPerBlock + threadIdx.x / kWave;
    if (i == 0 && lane == 0 && count != nullptr) count[0] = 0;
    if (i >= n) return;
    const int32_t row = keys[i] >> 1;
    if (row < row_lo || row >= row_hi) return;
    float* out = dst + (int64_t)(row - row_lo) * ld_dst;
    for (int c = lane; c < d; c += kWave) out[c] = 0.f;
    if (lane == 0 && mask != nullptr) mask[(row - row_lo) >> 5] = 0u;
}

inline int last_err() {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}

}  // namespace

extern "C" {

int lgcn_bpr_loss_indexed(const float* fu, int64_t ld_fu, const float* fi, int64_t ld_fi,
                          const float* u0, int64_t ld_u0, const float* i0, int64_t ld_i0,
                          int64_t n_users, int64_t n_items, const int64_t* users,
                          const int64_t* pos, const int64_t* neg, int32_t B, int32_t d,
                          float lambda, float* terms, float* loss, float* grads, void* stream) {
    if (B < 1 || d < 1 || !loss || !terms || !grads) return LGCN_EINVAL;
    if (!fu || !fi || !u0 || !i0 || !users || !pos || !neg) return LGCN_EINVAL;
    if (ld_fu < d || ld_fi < d || ld_u0 < d || ld_i0 < d) return LGCN_EINVAL;
    if (n_users < 0 || n_items < 0) return LGCN_EINVAL;
    const lgcn_bpr::IndexedRows rows = {{fu, fi, u0, i0}, {ld_fu, ld_fi, ld_u0, ld_i0},
                                        users, pos, neg, n_users, n_items};
    return lgcn_bpr::launch(rows, B, d, lambda, terms, loss, grads,
                            reinterpret_cast<hipStream_t>(stream));
}

int lgcn_bpr_keys(const int64_t* users, const int64_t* pos, const int64_t* neg, int32_t B,
                  int64_t n_users, int64_t n_items, int64_t* keys, void* stream) {
    if (B < 1 || !users || !pos || !neg || !keys) return LGCN_EINVAL;
    // every key, the skipped samples' included, must fit the sort's int32 keys
    if (n_users < 0 || n_items < 0 || n_users + n_items > 0x3ffffffeLL) return LGCN_EINVAL;
    hipLaunchKernelGGL(k_bpr_keys, dim3((uint32_t)(((int64_t)B + 255) / 256)), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), users, pos, neg, B, n_users, n_items,
                       keys);
    return last_err();
}

int lgcn_bpr_select_hardest(const float* fu, int64_t ld_fu, const float* fi, int64_t ld_fi,
                            int64_t n_users, int64_t n_items, const int64_t* users,
                            const int64_t* cand, int32_t B, int32_t n_neg, int32_t d,
                            int64_t* neg_out, float* score_out, void* stream) {
    if (B < 0 || d < 1 || n_neg < 1 || n_neg > LGCN_BPR_MAX_NEG) return LGCN_EINVAL;
    if (ld_fu < d || ld_fi < d || n_users < 0 || n_items < 0) return LGCN_EINVAL;
    if (B == 0) return 0;
    if (!fu || !fi || !users || !cand || !neg_out) return LGCN_EINVAL;
    const int64_t grid = ((int64_t)B + lgcn_bpr::kRowsPerBlock - 1) / lgcn_bpr::kRowsPerBlock;
    hipLaunchKernelGGL(k_bpr_select_hardest, dim3((uint32_t)grid),
                       dim3(kWave * lgcn_bpr::kRowsPerBlock), 0,
                       reinterpret_cast<hipStream_t>(stream), fu, ld_fu, fi, ld_fi, n_users,
                       n_items, users, cand, B, n_neg, d, neg_out, score_out);
    return last_err();
}

int lgcn_bpr_brand_loss_indexed(const float* fu, int64_t ld_fu, const float* fi, int64_t ld_fi,
                                const float* fb, int64_t ld_fb, const float* u0, int64_t ld_u0,
                                const float* i0, int64_t ld_i0, int64_t n_users, int64_t n_items,
                                int64_t n_brands, const int64_t* users, const int64_t* pos,
                                const int64_t* neg, const int32_t* item_brand, int32_t B,
                                int32_t d, float lambda, float brand_weight, float* terms,
                                float* loss, float* grads, float* coef, void* stream) {
    if (B < 1 || d < 1 || !loss || !terms || !grads) return LGCN_EINVAL;
    if (!fu || !fi || !fb || !u0 || !i0 || !users || !pos || !neg || !item_brand)
        return LGCN_EINVAL;
    if (ld_fu < d || ld_fi < d || ld_fb < d || ld_u0 < d || ld_i0 < d) return LGCN_EINVAL;
    if (n_users < 0 || n_items < 0 || n_brands < 0) return LGCN_EINVAL;
    const lgcn_bpr::IndexedBrandRows rows = {
        {{fu, fi, u0, i0}, {ld_fu, ld_fi, ld_u0, ld_i0}, users, pos, neg, n_users, n_items},
        fb, ld_fb, item_brand, n_brands};
    return lgcn_bpr::launch_brand(rows, B, d, lambda, brand_weight, terms, loss, grads, coef,
                                  reinterpret_cast<hipStream_t>(stream));
}

int lgcn_bpr_brand_keys(const int64_t* users, const int64_t* pos, const int64_t* neg,
                        const int32_t* item_brand, int32_t B, int64_t n_users, int64_t n_items,
                        int64_t n_brands, int64_t* keys, void* stream) {
    if (B < 1 || !users || !pos || !neg || !item_brand || !keys) return LGCN_EINVAL;
    if (n_users < 0 || n_items < 0 || n_brands < 0) return LGCN_EINVAL;
    // every key, the "none" one included, must fit the sort's int32 keys (each term is checked on
    // its own first: the sum of three int64 must not wrap)
    if (n_users > 0x3ffffffeLL || n_items > 0x3ffffffeLL || n_brands > 0x3ffffffeLL ||
        n_users + n_items + n_brands > 0x3ffffffeLL)
        return LGCN_EINVAL;
    hipLaunchKernelGGL(k_bpr_brand_keys, dim3((uint32_t)(((int64_t)B + 255) / 256)), dim3(256), 0,
                       reinterpret_cast<hipStream_t>(stream), users, pos, neg, item_brand, B,
                       n_users, n_items, n_brands, keys);
    return last_err();
}

int lgcn_rows_scatter(const int32_t* keys_sorted, const int32_t* perm, int32_t n, const float* src,
                      int64_t ld_src, int32_t row_lo, int32_t row_hi, float* dst, int64_t ld_dst,
                      int32_t d, int32_t mode, uint32_t* mask, int32_t* count, void* stream) {
    if (n < 0 || d < 1 || ld_src < d || ld_dst < d || row_lo < 0 || row_hi < row_lo)
        return LGCN_EINVAL;
    if (mode != LGCN_SCATTER_STORE && mode != LGCN_SCATTER_ADD) return LGCN_EINVAL;
    if (mode == LGCN_SCATTER_ADD && (mask || count)) return LGCN_EINVAL;
    if (count && !mask) return LGCN_EINVAL;
    if (n == 0 || row_hi == row_lo) return 0;
    if (!keys_sorted || !perm || !src || !dst) return LGCN_EINVAL;
    const dim3 grid((uint32_t)(((int64_t)n + kWavesPerBlock - 1) / kWavesPerBlock));
    const dim3 block(kWave * kWavesPerBlock);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (mode == LGCN_SCATTER_STORE)
        hipLaunchKernelGGL(k_rows_scatter<LGCN_SCATTER_STORE>, grid, block, 0, s, keys_sorted, perm,
                           n, src, ld_src, row_lo, row_hi, dst, ld_dst, d, mask, count);
    else
        hipLaunchKernelGGL(k_rows_scatter<LGCN_SCATTER_ADD>, grid, block, 0, s, keys_sorted, perm,
                           n, src, ld_src, row_lo, row_hi, dst, ld_dst, d, mask, count);
    return last_err();
}

int lgcn_rows_clear(const int32_t* keys_sorted, int32_t n, int32_t row_lo, int32_t row_hi,
                    float* dst, int64_t ld_dst, int32_t d, uint32_t* mask, int32_t* count,
                    void* stream) {
    if (n < 0 || d < 1 || ld_dst < d || row_lo < 0 || row_hi < row_lo) return LGCN_EINVAL;
    if (n > 0 && (!keys_sorted || !dst)) return LGCN_EINVAL;
    if (n == 0 && !count) return 0;
    const int64_t waves = n > 0 ? n : 1;
    hipLaunchKernelGGL(k_rows_clear, dim3((uint32_t)((waves + kWavesPerBlock - 1) / kWavesPerBlock)),
                       dim3(kWave * kWavesPerBlock), 0, reinterpret_cast<hipStream_t>(stream),
                       keys_sorted, n, row_lo, row_hi, dst, ld_dst, d, mask, count);
    return last_err();
}

}  // extern "C"

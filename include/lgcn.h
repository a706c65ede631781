/*
 * lgcn.h — C ABI of the MI355X-native LightGCN propagation engine (liblgcn_engine.so, gfx950).
 *
 * The hot path this library replaces is the K-layer propagation of the reference model
 *     ego = cat(user, item, brand)                         models/lightgcn.py:37-40
 *     for k < K: ego = torch.sparse.mm(adj_mat, ego)       models/lightgcn.py:44-46
 *     final = mean(stack([E0..EK]), 0)                     models/lightgcn.py:54
 *     (and the identical loop, models/lightgcn_fusion.py:52-59)
 * plus its autograd backward (torch SparseAddmmBackward0 + MeanBackward + CatBackward), and the
 * one-time conversion of the caller-owned `torch.sparse_coo_tensor` Â (main.py:331-336) into the
 * engine's CSR form. A ctypes binding of every entry point ships in
 * gcn_recommendation_amd/engine.py; INTEGRATION.md shows how a maintainer binds it.
 *
 * Conventions
 *  - Every pointer is a device pointer (hipMalloc / torch CUDA storage) unless named *_host.
 *  - No entry point allocates, frees or synchronises. Work is enqueued on `stream`
 *    (hipStream_t passed as void*; NULL = legacy default stream). Graph-capture safe.
 *  - Return value: 0 on success; a positive hipError_t value if a HIP launch failed; or a
 *    negative LGCN_E* code for invalid arguments (checked on the host before any launch).
 *    lgcn_error_string() names either kind.
 *  - Dense embedding blocks are row-major fp32 [rows x d] with leading dimension ld >= d
 *    (elements). Node ids follow main.py:283-287: users [0,U), items [U,U+I), brands [U+I,N).
 *  - CSR edge records are 8-byte {int32 col, fp32 val} pairs stored as int64 (lgcn_edge_t),
 *    rows keep the COO's stored order of their nonzeros (the order torch.sparse.mm sums them in).
 *  - Processing order: the propagation entry points take an optional `row_ids` [n_rows]. When
 *    it is non-NULL the CSR rows are stored in slots (lgcn_csr_order_by_degree): slot s holds
 *    the edges of row row_ids[s] and its result is written to row row_ids[s]. Column ids, X, Y
 *    and the epilogue operands are always in row-id space; only the work order changes.
 *  - Numerics: every row is the exact arithmetic of ATen's addmm_sparse_dense_cpu loop that
 *    torch.sparse.mm runs on CPU — one sequential fmaf chain per row in stored order — so
 *    results are bitwise identical, under an exact hub plan (lgcn_hub_plan_t without chunk
 *    items): short rows run that chain directly, rows of any length up to millions of edges are
 *    reproduced by block emulation (lgcn_emu_*). Hub CHUNK items are the optional fast mode: a
 *    long row cut into fixed chunks summed in a fixed order (deterministic, not bitwise).
 *  - Range of that guarantee: K = 0..16 (LGCN_MAX_LAYERS; K = 17 is refused with LGCN_ETOOMANY:
 *    over 18 stacked layers torch.mean no longer sums them one after the other), d = 1..2048.
 *    Every layer E1..EK and every gradient is bitwise for every K of the range. The final
 *    mean is bitwise the reference's everywhere for K <= 3; for K = 4..16 everywhere except the
 *    last n*d mod 32 elements of the flattened [n x d] table (32 measured with torch
 *    2.10.0+rocm7.0, AVX512; the width belongs to the ATen build). On that tail ATen itself
 *    leaves the sequential order (four interleaved partial sums); the engine keeps
 *    (((+0 + E0) + E1) + ... + EK) / (K+1) there too (DESIGN.md §3,
 *    tests/test_reference_mean.py). The sum starts from +0 as ATen's does, K = 0 included: an
 *    element that is -0 in every layer has the mean +0.
 */
#ifndef LGCN_H_
#define LGCN_H_

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 14 since the sided propagation; the training-step entry points (lgcn_bpr_loss_indexed,
 * lgcn_bpr_keys, lgcn_rows_scatter, lgcn_rows_clear) and the sampler (lgcn_bpr_sample,
 * LGCN_TUNE_SAMPLE_BLOCKS), the rank evaluation (lgcn_score_rank; lgcn_score_rank_lists and its
 * scratch query for lists of held-out items) and the brand-loss entry points
 * (lgcn_bpr_brand_loss, lgcn_bpr_brand_loss_indexed, lgcn_bpr_brand_keys) and the fusion pre-layer's
 * backward (lgcn_fusion_prelayer_backward, its scratch query, LGCN_FUSION_BWD_CHUNK,
 * LGCN_TUNE_FUSION_BWD_BLOCKS) and the Adam step (lgcn_adam_step, lgcn_adam_chunks, their two
 * structs, LGCN_ADAM_MAX_TENSORS, LGCN_ADAM_CHUNK) and the wide recommendation lists
 * (lgcn_score_topk_wide, lgcn_topk_wide_splits, its scratch query, LGCN_TOPK_WIDE_MAX_K) and
 * several negatives per sample (lgcn_bpr_sample_multi, lgcn_bpr_select_hardest,
 * LGCN_BPR_MAX_NEG) and the sampled-softmax loss over them (lgcn_ssm_loss,
 * lgcn_ssm_loss_indexed, lgcn_ssm_keys) and the in-batch softmax loss (lgcn_inbatch_loss,
 * lgcn_inbatch_loss_indexed, lgcn_inbatch_keys, LGCN_INBATCH_MAX_B / _D / _COEF_B) were added
 * without a bump: purely additive, no existing symbol, struct or constant changed. */
#define LGCN_ABI_VERSION 14

/* engine error codes (negative; positive values are hipError_t) */
#define LGCN_EINVAL      (-1)   /* bad size / null pointer / unsupported dimension */
#define LGCN_EALIGN      (-2)   /* a vectorised path needs 16-B aligned rows; see engine.py */
#define LGCN_ETOOMANY    (-3)   /* K > LGCN_MAX_LAYERS in a propagation entry point, more than
                                   LGCN_MAX_LAYERS prev_dense rows in a mean epilogue, or a
                                   schedule's event pool exhausted by one call */

#define LGCN_MAX_LAYERS 16      /* the deepest K: torch.mean over K+1 <= 17 stacked layers sums
                                   them sequentially (but for a short tail, see Numerics), over 18
                                   it does not; also the size of lgcn_epilogue_t.prev_dense */

/* status flags written by lgcn_coo_inspect */
#define LGCN_COO_ROWS_UNSORTED   1  /* some row index decreases in stored order */
#define LGCN_COO_OUT_OF_RANGE    2  /* an index is < 0 or >= its dimension */
#define LGCN_COO_COLS_UNSORTED   4  /* inside a row, columns are not strictly increasing */

/* epilogue modes of lgcn_spmm_layer / lgcn_hub_combine */
#define LGCN_EPI_STORE 0  /* Y = Â·X */
#define LGCN_EPI_MEAN  1  /* Y = (((P0 + P1) + ... + P_{n-1}) + Â·X) / div   (lightgcn.py:54) */
#define LGCN_EPI_ADD   2  /* Y = Z / div + Â·X          (backward Horner step) */
#define LGCN_EPI_ROWS  3  /* emulated-row entry points only (lgcn_emu_walk, lgcn_chain_rows): the
                             sum of row i of the row list to Y row i — an epilogue deferred to
                             lgcn_emu_epilogue, so a walk need not wait for the epilogue's operands */

typedef int64_t lgcn_edge_t;

/* Up to three row segments viewed as one [n x d] block: rows [0,end0) in p0, [end0,end1) in p1,
 * [end1,n) in p2. This is how E0 = cat(user, item, brand) (lightgcn.py:40) is read without the
 * copy. A single buffer is {p, p, p, n, n, ld}. */
typedef struct {
    const float* p0;
    const float* p1;
    const float* p2;
    int32_t end0;
    int32_t end1;
    int64_t ld;
} lgcn_rows_t;

/* hub work: one chunk of one long row -> one partial-sum slot of d floats (beg/end index the
 * edge array as stored, i.e. in slot order when the CSR is degree-ordered). slot < 0: the item
 * is a WHOLE row, summed as one sequential chain (bitwise = reference) with the epilogue applied
 * in place to output row `row` (exact plans: rows between the bundle and emulation sizes). */
typedef struct {
    int32_t row;
    int32_t beg;
    int32_t end;
    int32_t slot;
} lgcn_hub_item_t;

/* one long row: its partials occupy slots [first_slot, first_slot + n_slots); row = output row.
 * A row list may start with n_pre pre-reduction entries: `row` is then a partial slot that
 * receives the sum of slots [first_slot, first_slot + n_slots) (two-level combine of rows with
 * thousands of chunks); pad = 1 marks them (informational). */
typedef struct {
    int32_t row;
    int32_t first_slot;
    int32_t n_slots;
    int32_t pad;
} lgcn_hub_row_t;

/* ---- exact hub rows: parallel reproduction of one long sequential chain (lgcn_exact.hip) ---- */
#define LGCN_EMU_BLOCK 256       /* max edges per emulation block */
#define LGCN_EMU_CANDS 16        /* translation-table binades per (block, column) */
#define LGCN_EMU_META_BYTES 16   /* per (block, column) metadata record (opaque) */
#define LGCN_EMU_MAX_WALK_SLOTS 28 /* lgcn_emu_walk: LDS slots per chunk (CU LDS, vmcnt range) */

/* one block of an emulated row: edges [beg, end) as stored; first = 1 for the row's block 0;
 * row = index of its lgcn_emu_row_t (informational) */
typedef struct {
    int32_t row;
    int32_t beg;
    int32_t end;
    int32_t first;
} lgcn_emu_block_t;

/* one emulated row: output row id, its blocks [first_block, first_block + n_blocks) in edge
 * order in the block list */
typedef struct {
    int32_t row;
    int32_t first_block;
    int32_t n_blocks;
    int32_t pad;
} lgcn_emu_row_t;

/* Everything a layer needs beyond the CSR to treat rows above the bundle threshold:
 *  - items/n_items: hub chunks (slot >= 0, combined by `rows`) and whole long rows (slot < 0);
 *  - rows/n_rows/n_pre/partials: the chunk combine (lgcn_hub_combine); n_rows = 0 if none;
 *  - emu_*: rows summed exactly outside the layer kernel: block emulation (lgcn_emu_blocks +
 *    lgcn_emu_walk) or the sequential chain kernel (lgcn_chain_rows), see emu_part_*;
 *    emu_rel [n_emu_blocks x d x LGCN_EMU_CANDS] 4-byte words (the per-binade translation
 *    tables) and emu_meta [n_emu_blocks x d x LGCN_EMU_META_BYTES] are caller scratch, 16-B
 *    aligned; emu_stage (optional, NULL = off) [n_emu_blocks x
 *    (d + 1) x LGCN_EMU_BLOCK] fp32 scratch: the block pass writes each block's X elements per
 *    column there (and its edge values as column d), so a block the walk must re-run is read
 *    contiguously (LDS-DMA) instead of gathered.
 * threshold: rows of degree <= threshold run as bundles in the layer kernel; every row above it
 * must be covered by exactly one of: chunk items, a long-row item, an emulated row. */
typedef struct {
    const lgcn_hub_item_t* items;
    const lgcn_hub_row_t* rows;
    float* partials;
    const lgcn_emu_block_t* emu_blocks;
    const lgcn_emu_row_t* emu_rows;
    float* emu_rel;
    void* emu_meta;
    float* emu_stage;
    int32_t threshold;
    int32_t n_items;
    int32_t n_rows;
    int32_t n_pre;
    int32_t n_emu_blocks;
    int32_t n_emu_rows;
    /* The emulated rows (stored longest first) in three parts: rows [0, emu_part_rows[0]) and
     * [emu_part_rows[0], emu_part_rows[1]) are block-passed and walked (their blocks: [0,
     * emu_part_blocks[0]) and [emu_part_blocks[0], emu_part_blocks[1])); the rows after
     * emu_part_rows[1] run as sequential chains (lgcn_chain_rows) when lgcn_chain_supported(d)
     * and X is 16-B aligned, and are walked otherwise. The scratch (emu_rel / emu_meta /
     * emu_stage) must cover the walked blocks: [0, emu_part_blocks[1]) when chains run, all
     * n_emu_blocks otherwise; emu_scratch_blocks = the blocks it covers (a layer that would walk
     * past it returns LGCN_EINVAL). {0, 0} = every emulated row is a chain row. */
    int32_t emu_part_rows[2];
    int32_t emu_part_blocks[2];
    int32_t emu_scratch_blocks;
    /* optional (NULL = off) scratch of lgcn_live_scratch_bytes(n_emu_rows, n_emu_blocks) bytes,
     * 256-B aligned: with a row-sparse X (x_nz) every emulated row runs as a chain over its live
     * edges (lgcn_live_rows) instead of block pass + walk / chain over all of them */
    void* emu_live;
    /* the longest row's block count in part 0 / part 1 (lgcn_plan_exact writes them;
     * informational) */
    int32_t emu_part_max_blocks[2];
    /* optional (NULL = off) scratch [n_emu_rows x d] fp32, 16-B aligned: a MEAN layer under a
     * schedule with a late epilogue operand (lgcn_propagate_forward_sides' final half-layers)
     * writes the emulated rows' sums here (LGCN_EPI_ROWS) and applies their mean once the
     * operands are ready (lgcn_emu_epilogue), so its walks and chains need not wait for them */
    float* emu_out;
} lgcn_hub_plan_t;

/* Host planner of an exact hub plan (host memory only, no GPU call): from the host row pointers
 * of the CSR as stored (slot order when row_ids_host != NULL: slot s holds row row_ids_host[s]),
 * every row of degree > emu_min_degree becomes an emulated row — longest first, equal degrees in
 * slot order — cut into LGCN_EMU_BLOCK-edge blocks: rows_host[n_emu_rows], blocks_host
 * [n_emu_blocks] (copy both to the device for plan->emu_rows / emu_blocks). Part 0 = rows of
 * more than max(part0_blocks, ceil(chain_max / LGCN_EMU_BLOCK)) blocks, part 1 = rows of more
 * than ceil(chain_max / LGCN_EMU_BLOCK), the rest run as sequential chains (lgcn_chain_rows).
 * Writes plan->n_emu_rows, n_emu_blocks, emu_part_rows, emu_part_blocks, emu_part_max_blocks and
 * emu_scratch_blocks (= emu_part_blocks[1]); nothing else. Two-call protocol: rows_host = blocks_host = NULL writes
 * only the counts. chain_max <= 0: lgcn_chain_max_default(nnz); part0_blocks <= 0: 8192.
 * emu_min_degree = the bundle threshold (128) for the default exact plan. Replaces, for a C
 * host, the Python planner engine.plan_hubs (which calls it). */
int32_t lgcn_chain_max_default(int64_t nnz);
/* the chain cut for the plans of the backward's operator Âᵀ (lgcn_propagate_backward*): the
 * forward's default favours longer chains (fewer walks) than the backward's row-sparse layers do */
int32_t lgcn_chain_max_backward_default(int64_t nnz);
int lgcn_plan_exact(const int32_t* rowptr_host, const int32_t* row_ids_host, int32_t n_rows,
                    int32_t emu_min_degree, int32_t chain_max, int32_t part0_blocks,
                    lgcn_emu_row_t* rows_host, lgcn_emu_block_t* blocks_host,
                    lgcn_hub_plan_t* plan);
/* Whole-row items of an exact plan (host memory only): every row (slot) of threshold < degree <=
 * emu_min_degree becomes one lgcn_hub_item_t {row, beg, end, slot = -1}, in slot order — the
 * layer kernel runs each as one sequential chain with the epilogue in place, dispatched first in
 * its grid; lgcn_plan_exact(..., emu_min_degree, ...) then emulates / chains only the longer
 * rows. Two-call protocol: items_host = NULL writes only *n_items_host. Copy the items to the
 * device for plan->items / n_items. lgcn_emu_min_default(nnz) is the engine's default
 * emu_min_degree for a graph of nnz nonzeros (1024 from 2^23 nonzeros, else 0 = no items): the
 * headline C3 plan, as engine.plan_hubs builds it. */
int32_t lgcn_emu_min_default(int64_t nnz);
int lgcn_plan_items(const int32_t* rowptr_host, const int32_t* row_ids_host, int32_t n_rows,
                    int32_t threshold, int32_t emu_min_degree, lgcn_hub_item_t* items_host,
                    int32_t* n_items_host);
/* Scratch of a plan at width d: bytes_host[0..2] = emu_rel, emu_meta, emu_stage sizes covering
 * the walked blocks (walk_all = 0: parts 0 and 1; 1: every emulated block, when chains cannot
 * run — lgcn_chain_supported(d) false or X not 16-B aligned). */
int lgcn_plan_scratch_bytes(const lgcn_hub_plan_t* plan, int32_t d, int32_t walk_all,
                            size_t* bytes_host);

/* Epilogue operands. MEAN: prev0 is a segmented block (E0), prev_dense[i] (i < n_prev-1) are the
 * dense layer buffers E1..E_{n_prev-1} with leading dimension ld_prev, div = K+1. ADD: addend
 * is a segmented block Z, div its divisor (1 = plain add; the backward passes G and K+1);
 * addend_nz: NULL, or a row bitmask (lgcn_rows_nonzero) — rows whose bit is 0 are all zero and
 * are not read (results unchanged). */
typedef struct {
    int32_t mode;
    int32_t n_prev;
    float div;
    int32_t pad;          /* reserved: the engine overwrites it */
    lgcn_rows_t prev0;
    const float* prev_dense[LGCN_MAX_LAYERS];
    int64_t ld_prev;
    lgcn_rows_t addend;
    const uint32_t* addend_nz;
} lgcn_epilogue_t;

/* ---- identification ---------------------------------------------------------------------- */
int lgcn_abi_version(void);
const char* lgcn_error_string(int code);
/* Tuning knobs (process-global; results never depend on them). 0 = automatic (default).
 * Returns the previous value (value < 0 only queries), or LGCN_EINVAL for an unknown knob. */
#define LGCN_TUNE_ROWS_PER_GROUP 1  /* rows streamed by one lane group in k_layer (1 = one row) */
#define LGCN_TUNE_UNROLL         2  /* gathers in flight per lane group (d = 64 variants) */
#define LGCN_TUNE_MEAN_PREFETCH  3  /* MEAN layer on row bundles of <= 8 lanes per row: the
                                       bundle's E0..E_{K-1} rows loaded up front (0 = auto = on,
                                       2 = off) */
#define LGCN_TUNE_MIN_GROUPS     4  /* row bundles only when n_rows >= 2 x this many lane groups
                                       (0 = auto = 65536; 1 forces bundles on small graphs) */
/* (5: LGCN_TUNE_EMU_RESOLVE until ABI 12 — the walk's parallel exact-step runs, measured slower
   than the sequential chain and removed) */
#define LGCN_TUNE_EMU_MARGIN     6  /* emulation walk: the prediction's widened bounds, base << 4 |
                                       shift: (hi - lo) >> shift + base (default 128 << 4 | 4;
                                       A/B at C3: 3,256 / 2,256 / 3,1024 / 2,2048 within noise);
                                       results identical for every value (prediction only) */
#define LGCN_TUNE_SAMPLE_BLOCKS  7  /* lgcn_bpr_sample: the most blocks (of 256 slots per pass) its
                                       grid-stride launch uses (0 = auto = 8 per CU); a draw never
                                       depends on the launch geometry */
#define LGCN_TUNE_FUSION_BWD_BLOCKS 8 /* lgcn_fusion_prelayer_backward: the most blocks its main
                                       kernel's grid uses (0 = auto = one per CU); block b walks
                                       the row chunks b, b + grid, ...: no bit depends on it */
int lgcn_tune(int knob, int value);

/* device properties the host side needs (CU count); returns 0/hipError */
int lgcn_device_info(int device, int32_t* n_cu_host, int32_t* arch_major_host);

/* A stream of the schedule's own on the current device (non-blocking; high != 0: the greatest
 * priority, else the least): the schedule's streams must be distinct from every stream the host
 * hands out elsewhere — torch.cuda.Stream() returns streams from a round-robin pool of 32 per
 * priority, so two of them can be one HIP stream. */
int lgcn_stream_create(int32_t high, void** stream);
int lgcn_stream_destroy(void* stream);

/* ---- graph preparation (replaces the per-call COO handling inside torch.sparse.mm) ---------- */

/* Inspect a COO (rows/cols int64, as torch.sparse_coo_tensor._indices()) and OR LGCN_COO_*
 * flags into *flags (device int32, caller zeroes it). */
int lgcn_coo_inspect(const int64_t* rows, const int64_t* cols, int64_t nnz, int32_t n_rows,
                     int32_t n_cols, int32_t* flags, void* stream);

/* Row-sorted COO -> CSR. rowptr[n_rows+1] (int32), edges[nnz]. Order inside a row is kept.
 * If perm != NULL, input element i is taken from position perm[i] (a stable sort permutation
 * from lgcn_coo_sort_perm), and row indices are read as keys_sorted[i]. For the transpose of a
 * non-symmetric Â pass (rows, cols) swapped and the permutation of the stable sort by column. */
int lgcn_coo_to_csr(const int64_t* rows, const int64_t* cols, const float* vals, int64_t nnz,
                    int32_t n_rows, const int32_t* perm, const int32_t* keys_sorted,
                    int32_t* rowptr, lgcn_edge_t* edges, void* stream);

/* Stable sort permutation of nnz keys (int64 in [0, n_keys)) — used for unsorted COO input
 * (keys = rows) and for the transpose of a non-symmetric Â (keys = cols). Two-call protocol:
 * with temp == NULL only *temp_bytes_host is written. keys_tmp/keys_sorted/perm_tmp/perm are
 * caller buffers of nnz int32 each. */
int lgcn_coo_sort_perm(const int64_t* keys, int64_t nnz, int32_t n_keys, int32_t* keys_tmp,
                       int32_t* keys_sorted, int32_t* perm_tmp, int32_t* perm, void* temp,
                       size_t* temp_bytes_host, void* stream);

/* Bitwise symmetry test of a CSR with sorted unique columns: *asym (device int32, zeroed by the
 * caller) becomes nonzero if some (r,c,v) lacks a bit-identical (c,r,v). When Â is symmetric the
 * backward Âᵀ·G reuses the forward CSR (torch: SparseAddmmBackward0 computes Âᵀ·G). */
int lgcn_csr_check_symmetric(const int32_t* rowptr, const lgcn_edge_t* edges, int32_t n_rows,
                             int64_t nnz, int32_t* asym, void* stream);

/* Degree-ordered copy of a CSR for the propagation kernels: row_ids[s] = the row processed in
 * slot s (degree descending), rowptr_out[n_rows+1] / edges_out[nnz] = the rows in slot order,
 * each row's edges in their original order (so every result is bitwise unchanged). Ties: with
 * key_tmp / key_sorted NULL, row order (a stable radix sort); with them (n_rows uint64 each,
 * square operators only: columns index rows), rows of equal degree are grouped by their least
 * popular neighbour (highest degree rank) — rows gathered by the same row then sit in
 * consecutive slots, which a narrow (featsplit) shard turns into shared 128-B lines.
 * Sides: with side_lo < side_hi the rows in [side_lo, side_hi) (main.py:283-287: the items)
 * take the last n_rows - (side_hi - side_lo) .. n_rows - 1 slots, every other row the first
 * ones, each side degree-descending — the slot order the bipartite schedule
 * (lgcn_propagate_forward_sides) cuts into its two half-layers. side_lo == side_hi: one order.
 * Scratch deg_tmp / deg_sorted / iota_tmp: n_rows int32 each. Two-call protocol for temp
 * (temp == NULL: only *temp_bytes_host is written; pass the same key pointers both times). */
int lgcn_csr_order_by_degree(const int32_t* rowptr, const lgcn_edge_t* edges, int32_t n_rows,
                             int64_t nnz, int32_t side_lo, int32_t side_hi, int32_t* deg_tmp,
                             int32_t* deg_sorted, int32_t* iota_tmp,
                             int32_t* row_ids, int32_t* rowptr_out, lgcn_edge_t* edges_out,
                             uint64_t* key_tmp, uint64_t* key_sorted,
                             void* temp, size_t* temp_bytes_host, void* stream);

/* Bipartite test for the schedule of lgcn_propagate_*_sides: *bad (device int32, zeroed by the
 * caller) becomes nonzero if some edge joins two rows on the same side of [side_lo, side_hi)
 * (a row inside the range linked to another inside, or outside to outside). row_ids: the slot
 * order (NULL = rows stored in id order). The reference graph passes: users and brands link only
 * to items (main.py:295-311). */
int lgcn_csr_check_bipartite(const int32_t* rowptr, const lgcn_edge_t* edges,
                             const int32_t* row_ids, int32_t n_rows, int64_t nnz,
                             int32_t side_lo, int32_t side_hi, int32_t* bad, void* stream);

/* Column relabelling: edges_out[j] = edges[j] with column c replaced by new_id[c]. With the
 * slot order of lgcn_csr_order_by_degree (new_id = its inverse) this stores P·Â·Pᵀ: an operator
 * whose rows, columns and embedding rows all live in slot space (the featsplit shards keep
 * their parameters there), so writes and the layer buffers are sequential. */
int lgcn_csr_relabel_cols(const lgcn_edge_t* edges, int64_t nnz, const int32_t* new_id,
                          lgcn_edge_t* edges_out, void* stream);

/* Side-0 classes of a side-major slot order (lgcn_csr_order_by_degree with sides; split = the
 * first side-1 slot) for the sided propagation's dependency schedule: side-1 slots [split, split +
 * part_rows0) are the rows of the side-1 plans' walked part 0 (the longest item rows), [split +
 * part_rows0, split + part_rows1) part 1 — a degree-ordered plan lists its emulated rows in slot
 * order, so these are the first slots of side 1. A side-0 row is class 0 if it is linked to a
 * part-0 row, class 1 if linked to a part-1 row only, class 2 otherwise — linked in either
 * direction (the part row reads it, or it reads the part row), so the classes also hold for an
 * operator that is not structurally symmetric. Writes the same operator
 * with side 0's slots stably re-sorted by class (each class keeps its degree order; side 1 is
 * unchanged): row_ids_out / rowptr_out / edges_out as lgcn_csr_order_by_degree's, and
 * class_end[0..1] (device int32[2]) = the first slot of class 1 and of class 2. Bitwise-neutral
 * (every row keeps its edges). work: 5 n_rows int32 scratch. Two-call protocol for temp. Pass
 * the class ends and part_rows to the sided propagation in lgcn_sides_t. */
int lgcn_csr_side_classes(const int32_t* rowptr, const lgcn_edge_t* edges, const int32_t* row_ids,
                          int32_t n_rows, int64_t nnz, int32_t split, int32_t part_rows0,
                          int32_t part_rows1, int32_t* work, int32_t* row_ids_out,
                          int32_t* rowptr_out, lgcn_edge_t* edges_out, int32_t* class_end,
                          void* temp, size_t* temp_bytes_host, void* stream);

/* ---- adjacency builder (main.py:313-336 on the device) -------------------------------------- */
/* deg[r] = number of stored edges with row r (duplicates counted, main.py:326 rowsum of the
 * ones matrix), by binary search over the SORTED keys (keys_b of lgcn_adj_sort_unique). */
int lgcn_adj_degree(const uint64_t* keys_sorted, int64_t n_edges, int32_t n, int32_t* deg,
                    void* stream);

/* Sort keys row*n+col (64-bit radix) and run-length encode them: uniq[0..*n_unique) ascending
 * (= (row, col) order), counts = duplicate multiplicity m. Two-call protocol for temp (temp ==
 * NULL: only *temp_bytes_host). keys_a/keys_b/uniq: n_edges uint64; counts: n_edges int32;
 * n_unique: one device int32. */
int lgcn_adj_sort_unique(const int64_t* rows, const int64_t* cols, int64_t n_edges, int32_t n,
                         uint64_t* keys_a, uint64_t* keys_b, uint64_t* uniq, int32_t* counts,
                         int32_t* n_unique, void* temp, size_t* temp_bytes_host, void* stream);

/* Values fp32((dinv[r] * m) * dinv[c]) (main.py:330-331 scipy D·A·D, each product rounded), the
 * COO the reference hands to the model (int64 rows/cols, fp32 vals: main.py:334-336) and the
 * engine's CSR (rowptr[n+1], edges[nnz]) in one pass. dinv = rowsum^-1/2 with inf -> 0, computed
 * by the caller (numpy's float32 power, main.py:328, is reproduced bitwise only by numpy). */
int lgcn_adj_finish(const uint64_t* uniq, const int32_t* counts, int64_t nnz, int32_t n,
                    const float* dinv, int64_t* coo_rows, int64_t* coo_cols, float* vals,
                    int32_t* rowptr, lgcn_edge_t* edges, void* stream);

/* ---- the propagation (models/lightgcn.py:44-54) -------------------------------------------- */

/* One layer Y = epilogue(Â·(X / x_div)) over rows [0, n_rows):
 *  - rows with degree <= hub_threshold: one pass, sequential fmaf, epilogue applied in-kernel;
 *  - hub chunks (n_hub_items, from the host planner) write partials[slot*d ...];
 *    lgcn_hub_combine then finishes those rows. Both kinds run in ONE launch.
 * X is read through `x` (segments allowed); x_div = 1 reads it as is, otherwise every gathered
 * element is divided by x_div once (ADD epilogue only: the backward's G/(K+1)).
 * Y is [n_rows x ldy]. d in [1, 2048]. row_ids: NULL, or the slot -> row map of a
 * degree-ordered CSR (see Conventions). x_nz (ADD epilogue only): NULL, or the row bitmask of
 * X from lgcn_rows_nonzero — edges into all-zero rows of X are skipped, bitwise-neutrally (a
 * row-sparse upstream gradient makes the first backward layer read only its live rows). */
int lgcn_spmm_layer(const int32_t* rowptr, const lgcn_edge_t* edges, const int32_t* row_ids,
                    int32_t n_rows, int32_t hub_threshold, const lgcn_hub_item_t* hub_items,
                    int32_t n_hub_items, float* partials, lgcn_rows_t x, float x_div,
                    const uint32_t* x_nz, float* y, int64_t ldy, int32_t d,
                    const lgcn_epilogue_t* epi_host, void* stream);

/* Finish hub rows: entries [0, n_pre_rows) first sum runs of partial slots into other partial
 * slots (one launch), then every remaining entry sums its slots in a fixed order, applies the
 * epilogue and writes Y (a second launch). Deterministic. */
int lgcn_hub_combine(const lgcn_hub_row_t* hub_rows, int32_t n_hub_rows, int32_t n_pre_rows,
                     float* partials, float* y, int64_t ldy, int32_t d,
                     const lgcn_epilogue_t* epi_host, void* stream);

/* Row-sparsity of a block: mask[(n_rows+31)/32] gets bit r set iff row r holds a value != 0
 * (NaN included); *count (device int32) = number of such rows. No pre-zeroing needed. */
int lgcn_rows_nonzero(lgcn_rows_t x, int32_t n_rows, int32_t d, uint32_t* mask, int32_t* count,
                      void* stream);

/* Y[r,:] = X[r,:] / div for r < n_rows (the backward seed G/(K+1); a -0 keeps its sign. The
 * forward at K = 0 is lgcn_propagate_forward's (+0 + X) / 1, the mean of one stacked layer). */
/* dst[i] = dst[i] + src[i] wherever src[i] != 0 (n floats each): the gradient of layer-0 rows a
 * training step gathers (main.py:497, a row-sparse [rows x d] block) accumulated into the
 * propagation's dense gradient — the autograd accumulation of the two, reading dst only where src
 * holds a value (bitwise the dense add: dst is never -0). */
int lgcn_add_nonzero(const float* src, float* dst, int64_t n, void* stream);
int lgcn_scale_rows(lgcn_rows_t x, int32_t n_rows, int32_t d, float div, float* y, int64_t ldy,
                    void* stream);

/* Emulation block pass for one layer: for every block of every emulated row, candidate chains
 * + bounds over X (read as lgcn_spmm_layer reads it: x_div, x_nz) into rel / meta, and (stage
 * != NULL) the block's X elements per column into stage. live: NULL, or lgcn_live_flags() of a
 * preceding lgcn_live_rows over the plan's whole emulated-row list — blocks of the rows it ran
 * (flag n_blocks != 0, indexed by the block's `row`) are skipped. */
int lgcn_emu_blocks(const lgcn_edge_t* edges, const lgcn_emu_block_t* blocks, int32_t n_blocks,
                    lgcn_rows_t x, float x_div, const uint32_t* x_nz, int32_t d, float* rel,
                    void* meta, float* stage, const lgcn_emu_row_t* live, void* stream);

/* Emulation walk: each emulated row's final value per column (bitwise the sequential chain),
 * epilogue applied, written to Y. live: NULL, or the live-edge flags aligned with `rows` (rows
 * flagged n_blocks != 0 are skipped: lgcn_live_rows wrote them). Needs lgcn_emu_blocks' rel / meta (and stage, if it wrote
 * one; NULL = blocks to resolve gather X) of the same X. slots: LDS slots per 64-block chunk
 * for the blocks predicted to need an in-block resolve, 1..LGCN_EMU_MAX_WALK_SLOTS (0 = the
 * library default, 12; the Python binding and INTEGRATION.md's C recipe pass 20 for part 0 and
 * 8 for part 1): 4 KB of LDS per wave each (two chunks in flight), so a walk over short rows
 * runs more waves per CU with fewer slots, and the longest rows (few waves) take many. A chunk
 * with more predicted blocks than slots refills a slot as soon as the walk has passed the block
 * it held. */
int lgcn_emu_walk(const lgcn_edge_t* edges, const lgcn_emu_block_t* blocks,
                  const lgcn_emu_row_t* rows, int32_t n_rows, const float* rel, const void* meta,
                  const float* stage, lgcn_rows_t x, float x_div, const uint32_t* x_nz, float* y,
                  int64_t ldy, int32_t d, const lgcn_epilogue_t* epi_host, int32_t slots,
                  const lgcn_emu_row_t* live, void* stream);

/* The deferred epilogue of emulated rows written with LGCN_EPI_ROWS: row i of `rows` (output row
 * rows[i].row) = epilogue(tmp row i) with the STORE / MEAN / ADD epilogue epi_host — the
 * arithmetic, and order, of the kernels' own epilogue (bitwise the same rows). */
int lgcn_emu_epilogue(const lgcn_emu_row_t* rows, int32_t n_rows, const float* tmp, int64_t ld_tmp,
                      float* y, int64_t ldy, int32_t d, const lgcn_epilogue_t* epi_host,
                      void* stream);

/* Mid-size emulated rows run as the reference's sequential chain itself (no block pass): one
 * wave per (row, column slice) folds acc = fma(val_j, X[col_j, c], acc) in stored order from +0
 * while the next windows of gathered X rows are in flight by LDS-DMA. rows / blocks: as for
 * lgcn_emu_walk (a row's edges are [blocks[first].beg, blocks[first + n - 1].end)). X rows and
 * segments 16-B aligned; d: lgcn_chain_supported(d) (a multiple of 8: slices of 32, 16 or 8
 * columns — the last two for featsplit shards of d/P columns). x_nz is not
 * taken: dead rows of a row-sparse X are all zero, and folding them is exact. */
int lgcn_chain_supported(int32_t d);
int lgcn_chain_rows(const lgcn_edge_t* edges, const lgcn_emu_block_t* blocks,
                    const lgcn_emu_row_t* rows, int32_t n_rows, lgcn_rows_t x, float x_div,
                    float* y, int64_t ldy, int32_t d, const lgcn_epilogue_t* epi_host,
                    void* stream);

/* Row-sparse X (x_nz from lgcn_rows_nonzero: the backward's first layer on a BPR batch's
 * gradient): an edge into an all-zero row adds fma(v, +-0, acc) == acc to the reference's chain,
 * so each emulated row's chain equals the chain over its LIVE edges in stored order (edges with a
 * non-finite value are kept). lgcn_live_rows compacts them on the device (no host sync) into
 * scratch (lgcn_live_scratch_bytes, 256-B aligned) and runs them as lgcn_chain_rows; a 2.77M-edge
 * row keeps a few hundred. rows / blocks: the plan's emulated rows (lgcn_plan_exact). d and X as
 * for lgcn_chain_rows. */
#define LGCN_LIVE_MAX 65536  /* a walked row with more live edges than this stays walked */
size_t lgcn_live_scratch_bytes(int32_t n_rows, int32_t n_blocks);
/* Rows [live_min, n_rows) are always run as live-edge chains, rows below live_min only when
 * they hold at most max_live live edges (a dense X keeps the long rows on block pass + walk);
 * lgcn_live_flags(scratch, ...) then marks per row (n_blocks != 0) the rows it ran — pass it to
 * lgcn_emu_blocks / lgcn_emu_walk so they skip those. */
int lgcn_live_rows(const lgcn_edge_t* edges, const lgcn_emu_block_t* blocks, int32_t n_blocks,
                   const lgcn_emu_row_t* rows, int32_t n_rows, lgcn_rows_t x, float x_div,
                   const uint32_t* x_nz, float* y, int64_t ldy, int32_t d,
                   const lgcn_epilogue_t* epi_host, int32_t live_min, int32_t max_live,
                   void* scratch, void* stream);
const lgcn_emu_row_t* lgcn_live_flags(const void* scratch, int32_t n_rows, int32_t n_blocks);

/* Concurrent schedule of the exact layers (lgcn_layer, lgcn_propagate_forward/backward): the
 * emulated and chain rows run on auxiliary streams beside the layer kernel, forked from and
 * joined back into the caller's stream by events (graph-capture safe). Part 0 (the longest rows,
 * whose walk is a layer's critical path) goes to aux_streams[0] — create it with a high
 * priority — part 1 to [1], the chain rows to [2]; with fewer streams the later parts share the
 * last one (a budget for GPU_MAX_HW_QUEUES with RCCL running).
 * Bipartite lanes (lgcn_propagate_*_sides): with n_aux = 4 + m (m = 0..3), aux_streams[3] is
 * the main stream of the second lane of half-layers and [4..3+m] its part 0 / part 1 / chain
 * streams ([4] high priority), so the two chains of half-layers run side by side; with n_aux <= 3
 * both lanes share the caller's stream and [0..2]. HIP keeps a pool of hardware queues per
 * stream priority (GPU_MAX_HW_QUEUES each, default 4): with lane 1's four streams created at
 * high priority and the caller's + aux 0..2 at normal priority, every stream has a queue of its
 * own under the default (measured at C3: as fast as GPU_MAX_HW_QUEUES=8).
 * lgcn_sched_create allocates the events (the only allocating call; once per stream set); NULL
 * sched = everything in order on the caller's stream. */
typedef struct lgcn_sched lgcn_sched_t;
int lgcn_sched_create(void* const* aux_streams, int32_t n_aux, lgcn_sched_t** out);
int lgcn_sched_destroy(lgcn_sched_t* sched);
#define LGCN_SCHED_SLOTS0        1  /* walk LDS slots of part 0 (0..LGCN_EMU_MAX_WALK_SLOTS) */
#define LGCN_SCHED_SLOTS1        2  /* ... of part 1 (and of chain rows walked for lack of chains) */
#define LGCN_SCHED_CHAIN         3  /* 0: walk the chain rows too (A/B, tests) */
#define LGCN_SCHED_TIMING_START  4  /* hipEvent_t (or 0) recorded on the caller's stream right */
#define LGCN_SCHED_TIMING_END    5  /* before / after the layer kernel of every layer (timing) */
#define LGCN_SCHED_TRACE         6  /* hipEvent_t[8] (or 0): per-layer phase events — fork, part 0
                                       and part 1 block passes done, layer kernel done, chains
                                       done, part 0 and part 1 walks done, joined */
#define LGCN_SCHED_TRACE_SIDES   7  /* hipEvent_t[32 * K] (or 0): the same 8 phases of every
                                       segment of lgcn_propagate_*_sides — g = 0..2 the side-0
                                       classes, 3 side 1 — of layer k at [((k - 1) * 4 + g) * 8]
                                       (an empty segment records none) */
#define LGCN_SCHED_TIMING_SIDES  8  /* hipEvent_t[8 * K] (or 0): recorded on its lane's stream right
                                       before / after the layer kernel of segment g of layer k,
                                       at [((k - 1) * 4 + g) * 2] and [... + 1] (timing) */
/* (9 .. 15: BLOCKS_FIRST and MEAN_EARLY — now always on — and the measured-and-dropped PIECES,
   CHAINS_FIRST, LANE_FLIP, PRESUM, PRESUM_BUF of ABI 12) */
#define LGCN_SCHED_CLASSES      16  /* 1 (default): lgcn_propagate_*_sides runs side 0 class by class
                                       and lets side 1's walked parts wait only for the classes
                                       they read (lgcn_sides_t); 0: every part waits for the
                                       whole side-0 half-layer before it (same bits) */
#define LGCN_SCHED_LK_NORMAL    17  /* 1 (default): the final mean's side-1 layer kernel (lane
                                       1's last) runs on aux_streams[2] at normal priority, so the
                                       side-0 mean overlaps it instead of waiting for its grid;
                                       0: on lane 1's main stream (same bits) */
#define LGCN_SCHED_LANE1_SHARED 18  /* 1: lgcn_propagate_*_sides runs lane 1 on the caller's stream
                                       and aux_streams[2], [1], [0] (lane 0's, reversed): two lanes
                                       of half-layers that share lane 0's streams — the schedule of
                                       a row-sparse backward; the rest of aux_streams
                                       is not used (same bits) */
/* Captures: a HIP runtime before 7.2 segfaults in hipStreamEndCapture on the full two-lane
 * schedule (the same C host captures it on 7.2 and crashes on the 7.0 runtime the
 * torch 2.10.0+rocm7.0 wheel bundles). Under a capture on such a runtime lane 1 runs its
 * half-layers on its main stream alone and every part is joined at the end of its half-layer
 * (same bits); from 7.2 on the capture records the eager schedule. 1 = this process's runtime
 * captures the full schedule. */
int lgcn_capture_full_schedule(void);
int lgcn_sched_set(lgcn_sched_t* sched, int32_t knob, int64_t value);
/* What the latest lgcn_propagate_*_sides call on this schedule ran (diagnostics, tests). */
#define LGCN_SCHED_STATE_LANES     1  /* 2: two lanes, 1: one */
#define LGCN_SCHED_STATE_L1_AUX    2  /* aux streams lane 1 ran its parts on (0: its main stream) */
#define LGCN_SCHED_STATE_CAPTURING 3  /* 1: the caller's stream was being captured */
#define LGCN_SCHED_STATE_CLASSES   4  /* 1: the class dependencies were used */
#define LGCN_SCHED_STATE_CAPTURE_FULL 5  /* 1: captured with the eager schedule itself (below) */
int64_t lgcn_sched_state(const lgcn_sched_t* sched, int32_t what);

/* One whole layer under a hub plan: lgcn_spmm_layer (bundles, chunks and whole long rows) +
 * chunk combine, the emulation block pass + walk of the emulated parts, the chain rows — every
 * row of Y written once; concurrently under `sched` (above), else in order on `stream`. */
int lgcn_layer(const int32_t* rowptr, const lgcn_edge_t* edges, const int32_t* row_ids,
               int32_t n_rows, const lgcn_hub_plan_t* plan, lgcn_rows_t x, float x_div,
               const uint32_t* x_nz, float* y, int64_t ldy, int32_t d,
               const lgcn_epilogue_t* epi_host, const lgcn_sched_t* sched, void* stream);

/* Whole forward in one call: E1..E_{K-1} into layer_bufs_host[0..K-2] (each [n x d], ld = d),
 * final = mean(E0..EK) into out [n x d]. emb = E0 segments. plan: as in lgcn_layer (its
 * scratch sized for d). ev_host: NULL or 2*K hipEvent_t recorded around each layer (timing
 * only). sched: as in lgcn_layer. K = 0..LGCN_MAX_LAYERS: a larger K returns LGCN_ETOOMANY, here
 * and in every lgcn_propagate_* entry point below, before anything is looked at or launched. */
int lgcn_propagate_forward(const int32_t* rowptr, const lgcn_edge_t* edges,
                           const int32_t* row_ids, int32_t n, const lgcn_hub_plan_t* plan,
                           lgcn_rows_t emb, int32_t d,
                           int32_t K, float* const* layer_bufs_host, float* out,
                           void* const* ev_host, const lgcn_sched_t* sched, void* stream);

/* Whole backward: grad_e0 = sum_k (Âᵀ)^k G/(K+1) in the Horner order autograd uses
 * (c = G/(K+1); h = c; K times h = c + Âᵀ h). rowptr/edges must be Âᵀ (== Â when symmetric)
 * and plan its hub plan. G is read in place as segments (the user/item/brand output grads); c
 * is never stored. grad_nz: NULL, or G's row bitmask (lgcn_rows_nonzero): a BPR batch touches
 * a few thousand rows, so the first layer gathers only those and no epilogue reads G's zero
 * rows. work_h: [n x d] scratch (K > 1); grad_e0: [n x d], ld = d. sched: as in lgcn_layer. */
int lgcn_propagate_backward(const int32_t* rowptr, const lgcn_edge_t* edges,
                            const int32_t* row_ids, int32_t n, const lgcn_hub_plan_t* plan,
                            lgcn_rows_t grad_out,
                            const uint32_t* grad_nz, int32_t d, int32_t K, float* work_h,
                            float* grad_e0, const lgcn_sched_t* sched, void* stream);

/* Bipartite propagation: the rows of one side reference only rows of the other (users and
 * brands vs items, lgcn_csr_check_bipartite), so layer k of one side needs only layer k-1 of the
 * other. Every layer runs as half-layers over a side-major slot order (lgcn_csr_order_by_degree
 * with side_lo < side_hi, then lgcn_csr_side_classes): side 0 = slots [0, split) in its three
 * classes, side 1 = [split, n). Half-layer (k, side) runs on lane (k + side + K) % 2, each lane a
 * chain of half-layers that alternate sides (lane 1 = aux_streams[3..]), and:
 *  - layer 1 of side 0 runs class 0, 1, 2 in that order; the walked part 0 of layer 2's side 1
 *    (the longest item rows: the critical path) starts once class 0 — the rows it reads — is
 *    done, part 1 once classes 0 and 1 are;
 *  - side 1's parts 0 and 1 are not joined into their lane: layer k+1 of side 0 runs class 2 (it
 *    reads neither), then class 1 after part 1, then class 0 after part 0;
 *  - a final mean half-layer waits, per class / part, for the rows of layer K-1 it reads (made
 *    on the other lane), and its block passes not at all.
 * Same arguments and results (bitwise) as lgcn_propagate_forward / _backward, except:
 *  - sides: the slot layout (below); class_end = {split, split} and part_rows = {0, 0} when the
 *    slot order has no classes (side 0 is then one class);
 *  - plans: 8 hub plans, plans[2 * g + j] for segment g (0..2 = the side-0 classes, 3 = side 1;
 *    each built over its slot range, row ids absolute) with two scratch sets j = 0, 1 (the
 *    half-layers of one side on consecutive layers run on different lanes);
 *  - row_ids is required; no per-layer timing events (LGCN_SCHED_TRACE_SIDES traces phases);
 *  - the class dependencies are used only when side 1's plans walk no rows outside the ones the
 *    classes were built from (their emu_part_rows <= part_rows); otherwise every part waits for
 *    the whole side-0 half-layer (lgcn_sched_state reports which). */
typedef struct {
    int32_t n;             /* rows (= slots) */
    int32_t split;         /* first slot of side 1 */
    int32_t class_end[2];  /* side 0: class 0 = [0, class_end[0]), 1 = [.., class_end[1]), 2 = the
                              rest up to split (lgcn_csr_side_classes) */
    int32_t part_rows[2];  /* the part_rows0 / part_rows1 the classes were built from */
} lgcn_sides_t;
int lgcn_propagate_forward_sides(const int32_t* rowptr, const lgcn_edge_t* edges,
                                 const int32_t* row_ids, const lgcn_sides_t* sides,
                                 const lgcn_hub_plan_t* plans, lgcn_rows_t emb, int32_t d,
                                 int32_t K, float* const* layer_bufs_host, float* out,
                                 const lgcn_sched_t* sched, void* stream);
/* lgcn_propagate_forward_sides without the rows the result does not need. empty_tail[g]: the
 * last empty_tail[g] slots of segment g hold rows with no stored record that no stored record
 * names as its column (slots are degree-ordered, so such rows end their segment). Every layer of
 * such a row but E0 is +0 and nothing gathers it: the STORE layers' launches end before these
 * slots and leave their rows of layer_bufs_host UNWRITTEN, and the final mean writes
 * (E0 + 0) / (K+1) for them from E0 alone — the reference's bits. `out` is bitwise that of
 * lgcn_propagate_forward_sides; the layer buffers are private to the call (a caller that reads
 * them passes lean = NULL, which is lgcn_propagate_forward_sides itself). */
typedef struct {
    int32_t empty_tail[4];
} lgcn_lean_t;
int lgcn_propagate_forward_sides_lean(const int32_t* rowptr, const lgcn_edge_t* edges,
                                      const int32_t* row_ids, const lgcn_sides_t* sides,
                                      const lgcn_hub_plan_t* plans, const lgcn_lean_t* lean,
                                      lgcn_rows_t emb, int32_t d, int32_t K,
                                      float* const* layer_bufs_host, float* out,
                                      const lgcn_sched_t* sched, void* stream);
/* The lean forward with one layer row per group of single-record side-0 rows. Side-0
 * rows with exactly one stored record (p, w) and equal (p, value bits of w) hold bit-identical
 * rows fma(w, E_{k-1}[p], +0) in every layer k >= 1, so the member in the lowest slot (the
 * representative) stands for its group and the others ("shared" rows) are never materialised:
 *  - row_ids: the graph's row ids with side 0's single-record slots stably partitioned, the
 *    shared rows last — the shared_tail[g] slots directly before segment g's empty_tail[g] (all
 *    these slots hold one record, so rowptr and every hub plan stay as they are);
 *  - edges_l1: the graph's records with those slots' records moved the same way — what side 0
 *    reads in every layer and side 1 in layer 1 (E0 rows are parameters: all different);
 *  - edges_ln: edges_l1 with every column that names a shared row re-pointed to its
 *    representative (positions and value bits unchanged: every chain multiplies the same values
 *    with bit-identical rows in the same order) — what side 1 reads in layers k >= 2;
 *  - rep[t]: the representative's row id of shared slot t, in slot order over the segments.
 * Every half-layer launch of segment g ends before shared_tail[g] + empty_tail[g]; the STORE
 * layers leave the shared rows of layer_bufs_host UNWRITTEN, and after the segment's MEAN layer
 * one kernel writes out[u] = (((+0 + E0[u]) + L_1[r]) + ... + L_{K-1}[r] + fma(w, L_{K-1}[p], +0))
 * / (K+1) for every shared row u with representative r: epilogue_store's order, the reference's
 * bits. K <= 1 has no intermediate layer: it runs as the lean forward over row_ids / edges_l1.
 * LGCN_EINVAL before any launch: a negative tail or tails that do not fit their segment, a NULL
 * pointer beside a nonzero tail, shared rows on side 1 (shared_tail[3] != 0), shared rows in
 * more than one of side 0's segments (a class's mean waits for its own class's earlier layers
 * only, and a representative may lie in another class: sharing needs side 0 as one segment). */
typedef struct {
    int32_t empty_tail[4], shared_tail[4];
    const int32_t* row_ids;
    const lgcn_edge_t* edges_l1;
    const lgcn_edge_t* edges_ln;
    const int32_t* rep;
} lgcn_shared_t;
int lgcn_propagate_forward_sides_shared(const int32_t* rowptr, const lgcn_sides_t* sides,
                                        const lgcn_hub_plan_t* plans, const lgcn_shared_t* shared,
                                        lgcn_rows_t emb, int32_t d, int32_t K,
                                        float* const* layer_bufs_host, float* out,
                                        const lgcn_sched_t* sched, void* stream);
int lgcn_propagate_backward_sides(const int32_t* rowptr, const lgcn_edge_t* edges,
                                  const int32_t* row_ids, const lgcn_sides_t* sides,
                                  const lgcn_hub_plan_t* plans, lgcn_rows_t grad_out,
                                  const uint32_t* grad_nz, int32_t d, int32_t K, float* work_h,
                                  float* grad_e0, const lgcn_sched_t* sched, void* stream);

/* ---- training batch loss (main.py:366-402) -------------------------------------------------- */
/* Fused BPR + L2 loss of one batch of B gathered rows (u, p, n = final user / positive /
 * negative item rows; u0, p0, n0 = their layer-0 rows; row-major, leading dims ld*):
 *   *loss = -mean_b log(sigmoid(<u_b,p_b> - <u_b,n_b>) + 1e-8) + lambda*(|U0|^2+|P0|^2+|N0|^2)/B
 * and d(loss)/d(input) for all six inputs into grads = [6 x B x d] (order u, p, n, u0, p0, n0,
 * each dense [B x d]). terms: scratch [2 x B]. The batch reduction runs in a fixed order. */
int lgcn_bpr_loss(const float* u, int64_t ldu, const float* p, int64_t ldp, const float* n,
                  int64_t ldn, const float* u0, int64_t ldu0, const float* p0, int64_t ldp0,
                  const float* n0, int64_t ldn0, int32_t B, int32_t d, float lambda, float* terms,
                  float* loss, float* grads, void* stream);

/* ---- fused training step: the batch indices kept (main.py:495-525) --------------------------- */
/* lgcn_bpr_loss with the six row blocks read straight from the tables: sample b uses rows
 * users[b] of fu (final user table) and u0 (layer-0 user table), pos[b] / neg[b] of fi and i0
 * (final and layer-0 item tables); users / pos / neg are device int64 [B]. Same kernels, so loss
 * and grads ([6 x B x d], lgcn_bpr_loss's order) are bitwise those of lgcn_bpr_loss on gathered
 * copies. A sample with an index outside [0, n_users) / [0, n_items) is skipped: nothing of it is
 * dereferenced, its terms and gradient rows are zero. terms: scratch [2 x B]. */
int lgcn_bpr_loss_indexed(const float* fu, int64_t ld_fu, const float* fi, int64_t ld_fi,
                          const float* u0, int64_t ld_u0, const float* i0, int64_t ld_i0,
                          int64_t n_users, int64_t n_items, const int64_t* users,
                          const int64_t* pos, const int64_t* neg, int32_t B, int32_t d,
                          float lambda, float* terms, float* loss, float* grads, void* stream);

/* Destination keys of the batch's 3B per-sample gradient rows (rows [0,B) users, [B,2B) positive,
 * [2B,3B) negative items), keys [3 x B] int64 for lgcn_coo_sort_perm: 2 * row + is_neg, row in
 * the numbering of lgcn_propagate_backward's grad_out (user u -> u, item i -> n_users + i). All
 * three keys of a skipped sample (see above) are 2 * (n_users + n_items), past every row: sort
 * with n_keys = 2 * (n_users + n_items) + 1. */
int lgcn_bpr_keys(const int64_t* users, const int64_t* pos, const int64_t* neg, int32_t B,
                  int64_t n_users, int64_t n_items, int64_t* keys, void* stream);

/* Deterministic scatter-accumulate of n contributions into table rows. Contribution j (in sorted
 * order) has key keys_sorted[j] = 2 * row + sub and source row perm[j] of src [n x ld_src] —
 * keys_sorted / perm from lgcn_coo_sort_perm (stable: equal keys keep their batch order). Only
 * rows in [row_lo, row_hi) are written; row r lands in dst row r - row_lo (bit r - row_lo of
 * mask). Per destination row and column: (+0 + the sub = 0 contributions in sorted order) +
 * (+0 + the sub = 1 ones) — what IndexBackward's sequential index_put into zeros and autograd's
 * sum of the positive and negative item blocks give; plain fp32 adds, one wave per row, no float
 * atomics.
 *  STORE: dst row = that sum (dst all zero on entry: untouched rows stay zero); mask (NULL = none;
 *    zero on entry) gets the row's bit iff the sum holds a value != 0 (NaN included) and *count
 *    (NULL = none; zero on entry) the number of such rows — lgcn_rows_nonzero's of the dense dst.
 *  ADD: dst row = dst row + that sum, one add per element, touched rows only (an untouched row
 *    would receive +0: no change unless it held -0). mask and count must be NULL. */
#define LGCN_SCATTER_STORE 0
#define LGCN_SCATTER_ADD   1
int lgcn_rows_scatter(const int32_t* keys_sorted, const int32_t* perm, int32_t n, const float* src,
                      int64_t ld_src, int32_t row_lo, int32_t row_hi, float* dst, int64_t ld_dst,
                      int32_t d, int32_t mode, uint32_t* mask, int32_t* count, void* stream);

/* Undo a STORE scatter without touching the whole block: zero the dst rows the keys name (those
 * in [row_lo, row_hi)), the mask words they fall in (mask NULL = none) and *count (NULL = none). */
int lgcn_rows_clear(const int32_t* keys_sorted, int32_t n, int32_t row_lo, int32_t row_hi,
                    float* dst, int64_t ld_dst, int32_t d, uint32_t* mask, int32_t* count,
                    void* stream);

/* ---- the brand-preference term of the training batch (main.py:382-391, 499-522) -------------- */
/* lgcn_bpr_loss plus the reference's optional second BPR term over the final brand rows bp / bn of
 * a sample's positive / negative item, w = brand_weight:
 *   *loss = (bpr + w * -mean_b log(sigmoid(<u_b,bp_b> - <u_b,bn_b>) + 1e-8)) + reg
 * with bpr and reg lgcn_bpr_loss's two terms, each sum in its fixed order and
 *   *loss = fp32(fp32(-(sl/B)) + fp32(w * fp32(-(sb/B)))) + fp32(fp32(lambda * sr) / B).
 * Per sample x' = <u,bp> - <u,bn> (the fma and wave-sum order of the base scores),
 * s' = 1 / (1 + expf(-x')), c' = ((-w/B) / (s' + 1e-8f)) * (1 - s') * s', and
 *   du  = fp32(fp32(c*p) + fp32(-c*n)) + fp32(fp32(c'*bp) + fp32(-c'*bn)),
 *   dbp = c'*u, dbn = (-c')*u; dp, dn and the layer-0 rows as lgcn_bpr_loss writes them.
 * grads = [8 x B x d] in the order u0, p0, n0, u, p, n, bp, bn: blocks [3, 8) are one [5B x d]
 * source for lgcn_rows_scatter under lgcn_bpr_brand_keys' 5B keys, blocks [0, 3) the layer-0
 * source under the same keys (a permutation entry of a brand key, >= 3B, stays inside grads).
 * terms: scratch [3 x B] (log term, squared norms, brand log term logf(s' + 1e-8f)).
 * coef (NULL = not wanted): [2 x B], (c_b, c'_b).
 * brand_ok (NULL = every sample): uint8 [B]; a sample with brand_ok[b] == 0 has no brand term —
 * c' = 0, a zero brand log term, +0 dbp / dbn rows, and du exactly lgcn_bpr_loss's; rows b of bp
 * and bn are not read. The means still divide by B. */
int lgcn_bpr_brand_loss(const float* u, int64_t ldu, const float* p, int64_t ldp, const float* n,
                        int64_t ldn, const float* u0, int64_t ldu0, const float* p0, int64_t ldp0,
                        const float* n0, int64_t ldn0, const float* bp, int64_t ldbp,
                        const float* bn, int64_t ldbn, const uint8_t* brand_ok, int32_t B,
                        int32_t d, float lambda, float brand_weight, float* terms, float* loss,
                        float* grads, float* coef, void* stream);

/* lgcn_bpr_brand_loss with the rows read from the tables (lgcn_bpr_loss_indexed's, plus fb, the
 * final brand table [n_brands x ld_fb]): bp = fb + item_brand[pos[b]] * ld_fb, bn likewise from
 * neg[b]; item_brand: device int32 [n_items]. A sample whose positive or negative item maps
 * outside [0, n_brands) (-1 = the item has no brand) has no brand term, as under brand_ok == 0. A
 * sample with a user or item index outside its table is skipped whole: zero terms, coefficients
 * and gradient rows, item_brand not read. Same kernels as lgcn_bpr_brand_loss: bitwise its
 * outputs on gathered copies. */
int lgcn_bpr_brand_loss_indexed(const float* fu, int64_t ld_fu, const float* fi, int64_t ld_fi,
                                const float* fb, int64_t ld_fb, const float* u0, int64_t ld_u0,
                                const float* i0, int64_t ld_i0, int64_t n_users, int64_t n_items,
                                int64_t n_brands, const int64_t* users, const int64_t* pos,
                                const int64_t* neg, const int32_t* item_brand, int32_t B,
                                int32_t d, float lambda, float brand_weight, float* terms,
                                float* loss, float* grads, float* coef, void* stream);

/* The 5B destination keys of that batch's final-row gradient blocks, keys [5 x B] int64:
 * lgcn_bpr_keys' 3B, then [3B,4B) the positive item's brand row (bit 0 clear) and [4B,5B) the
 * negative item's (bit 0 set), brand r -> row n_users + n_items + r. "None" =
 * 2 * (n_users + n_items + n_brands), past every row: all five keys of a skipped sample, the two
 * brand keys of a sample without a brand term. Sort with n_keys = none + 1. LGCN_EINVAL when that
 * would not fit the sort's int32 keys (n_users + n_items + n_brands > 0x3ffffffe). A brand row is
 * then summed like an item row: (+0 + its positive run) + (+0 + its negative run). */
int lgcn_bpr_brand_keys(const int64_t* users, const int64_t* pos, const int64_t* neg,
                        const int32_t* item_brand, int32_t B, int64_t n_users, int64_t n_items,
                        int64_t n_brands, int64_t* keys, void* stream);

/* ---- BPR negative sampler (main.py:349-363, BPRDataset.__getitem__) -------------------------- */
/* The triples of `count` training samples in one launch (count may be a whole epoch). Output slot
 * s in [0, count) takes interaction idx = order ? order[first + s] : first + s (order: device
 * int64 with at least first + count entries, e.g. a permutation; NULL = identity) and writes
 *   users[s] = inter_user[idx], pos[s] = inter_item[idx], neg[s] = the draw below
 * (inter_user / inter_item: the int32 [n_inter] train interactions, duplicates kept as samples;
 * users / pos / neg: int64 [count], what lgcn_bpr_loss_indexed and lgcn_bpr_keys take).
 *
 * The draw. The negative of an interaction is a pure function of (seed, epoch, idx, the user's
 * positive list, n_items): it does not depend on batch size, order, first / count, the launch
 * geometry (LGCN_TUNE_SAMPLE_BLOCKS) or the device.
 *  - Positives: pos_rowptr [n_users + 1] / pos_items, int32: per user the sorted, de-duplicated
 *    items of its interactions (the CSR lgcn_score_topk masks with: mask_rowptr / mask_items).
 *    L = the user's list, deg its length.
 *  - Random bits: Philox4x32-10 (multipliers 0xD2511F53 / 0xCD9E8D57, Weyl constants 0x9E3779B9 /
 *    0xBB67AE85) of counter (idx_lo32, idx_hi32, epoch, 0) under key (seed_lo32, seed_hi32);
 *    r64 = (out[1] << 32) | out[0].
 *  - Range: n_free = n_items - deg, j = the high 64 bits of r64 * n_free (no modulo, no
 *    rejection loop).
 *  - Selection: the j-th (0-based) item not in L: m = the number of positions t with
 *    L[t] - t <= j (L[t] - t is non-decreasing: an upper-bound binary search), neg = j + m.
 *    Uniform over the complement of L up to the 2^-33 bias of the range reduction.
 *  - n_free <= 0 (a user with every item as a positive — the reference's rejection loop never
 *    returns): neg = -1 and *n_unsampled (device int32, NULL = not counted; the caller zeroes it)
 *    is incremented by an integer atomic. lgcn_bpr_loss_indexed and lgcn_bpr_keys skip a sample
 *    whose index lies outside its table, so such a triple goes through a training step as a
 *    sample with zero loss terms and zero gradient rows (the batch mean still divides by B).
 * Memory safety: idx outside [0, n_inter) or inter_user[idx] outside [0, n_users) writes -1 to
 * all three outputs of the slot and dereferences nothing further (not counted in *n_unsampled);
 * pos_rowptr must be a CSR over pos_items. Refused on the host (LGCN_EINVAL): a NULL pointer
 * other than order / n_unsampled / stream, n_inter / n_users / n_items < 0 or >= 2^31, first < 0,
 * count < 0. count == 0 returns 0 and launches nothing. */
int lgcn_bpr_sample(const int32_t* inter_user, const int32_t* inter_item, int64_t n_inter,
                    const int64_t* order, int64_t first, int64_t count,
                    const int32_t* pos_rowptr, const int32_t* pos_items, int64_t n_users,
                    int64_t n_items, uint64_t seed, uint32_t epoch, int64_t* users, int64_t* pos,
                    int64_t* neg, int32_t* n_unsampled, void* stream);

/* lgcn_bpr_sample with n_neg negatives per sample, neg = int64 [count x n_neg] row-major (a
 * slot's n_neg entries side by side). Entry m ("ordinal m") of interaction idx is the draw above
 * with the counter's fourth word set to m: Philox counter (idx_lo32, idx_hi32, epoch, m); key,
 * r64, range reduction and selection unchanged. So column 0 is lgcn_bpr_sample's negative bit for
 * bit, and column m depends neither on n_neg nor on anything the draw above does not depend on.
 * The ordinals of a slot are independent draws over the complement of the user's list: the same
 * item may come up more than once (no sequential exclusion, which would tie column m to the
 * columns before it). A slot whose interaction or user is out of range has -1 in users, pos and
 * all n_neg entries; a user without a free item -1 in all n_neg entries, and *n_unsampled rises
 * once for the slot. Refused on the host (LGCN_EINVAL), in this order: the sizes lgcn_bpr_sample
 * refuses; n_neg outside [1, LGCN_BPR_MAX_NEG]; count * n_neg past int64. Then count == 0 returns
 * 0, launches nothing and looks at no pointer; then a NULL pointer other than order /
 * n_unsampled / stream (LGCN_EINVAL). */
#define LGCN_BPR_MAX_NEG 64
int lgcn_bpr_sample_multi(const int32_t* inter_user, const int32_t* inter_item, int64_t n_inter,
                          const int64_t* order, int64_t first, int64_t count,
                          const int32_t* pos_rowptr, const int32_t* pos_items, int64_t n_users,
                          int64_t n_items, uint64_t seed, uint32_t epoch, int32_t n_neg,
                          int64_t* users, int64_t* pos, int64_t* neg, int32_t* n_unsampled,
                          void* stream);

/* lgcn_bpr_sample_multi with negatives drawn in proportion to integer item weights w[i] in
 * [0, 2^24] (popularity^alpha, quantised), given as two device int64 tables:
 *  - item_cumw [n_items + 1]: the exclusive prefix sum of w; W = item_cumw[n_items].
 *  - pos_cumw [n_pos + 1]: the exclusive prefix sum of w[pos_items[.]] over the whole positive
 *    CSR, aligned with pos_rowptr: with beg = pos_rowptr[u], end = pos_rowptr[u + 1], a user's
 *    prefix is pw[t] = pos_cumw[beg + t] - pos_cumw[beg], t in [0, deg], and pos_cumw[end] -
 *    pos_cumw[beg] the weight of all its positives. The totals stay below 2^55.
 * The draw of interaction idx, ordinal m: r64 is lgcn_bpr_sample_multi's (Philox4x32-10, counter
 * (idx_lo32, idx_hi32, epoch, m), key = seed), then
 *   W_free = W - (pos_cumw[end] - pos_cumw[beg])   <= 0: neg = -1 in all n_neg entries, and
 *                                                  *n_unsampled rises once for the slot
 *   r   = the high 64 bits of r64 * W_free
 *   t*  = #{t in [0, deg) : item_cumw[L[t]] - pw[t] <= r}   (an upper-bound binary search: the
 *         free weight below L[t] is non-decreasing in t)
 *   r'  = r + pw[t*]
 *   neg = (the first k in [0, n_items] with item_cumw[k] > r') - 1   (upper-bound binary search)
 * r is a position in the concatenated weights of the user's free items, r' the same position in
 * the weights of all items: a free item i is drawn with probability w[i] / W_free up to the 2^-64
 * granularity of the range reduction, a positive or a zero-weight item never. A pure function of
 * (seed, epoch, idx, m, the user's list, the weights): no alias table, no rejection loop. With
 * every w[i] = 1 it is lgcn_bpr_sample_multi's draw bit for bit (item_cumw[k] = k, pw[t] = t).
 * Memory safety, for any table contents: an L[t] outside [0, n_items) is not used as an index (it
 * counts as "greater than r"); a result outside [0, n_items) is written as -1; pos_rowptr must be
 * a CSR over pos_items and pos_cumw. Slots out of range are lgcn_bpr_sample_multi's. Refused on
 * the host as lgcn_bpr_sample_multi refuses, in its order, NULL tables with the NULL pointers. */
int lgcn_bpr_sample_weighted(const int32_t* inter_user, const int32_t* inter_item,
                             int64_t n_inter, const int64_t* order, int64_t first, int64_t count,
                             const int32_t* pos_rowptr, const int32_t* pos_items,
                             const int64_t* pos_cumw, const int64_t* item_cumw, int64_t n_users,
                             int64_t n_items, uint64_t seed, uint32_t epoch, int32_t n_neg,
                             int64_t* users, int64_t* pos, int64_t* neg, int32_t* n_unsampled,
                             void* stream);

/* Dynamic negative sampling: per sample the hardest of n_neg candidate negatives, neg_out[b] =
 * the candidate the current tables score highest for users[b] (cand: device int64 [B x n_neg]
 * row-major, e.g. lgcn_bpr_sample_multi's neg; fu / fi: the final user / item tables).
 *  - Score of candidate m: <fu[users[b]], fi[cand[b][m]]> by the expression lgcn_bpr_loss_indexed
 *    forms its negative score with (one device function, called by both): per lane an fmaf chain
 *    over k = lane, lane + 64, ... from +0, then the 32, 16, ..., 1 xor butterfly. score_out[b]
 *    (NULL = not wanted) is therefore bitwise the negative score the loss kernel forms for
 *    neg_out[b]; it does not depend on how many candidate rows the kernel loads at a time.
 *  - Rule (NaN scores included): the choice starts as the first candidate, in ascending m, whose
 *    index lies in [0, n_items); a later candidate in range replaces it only if its score compares
 *    greater (>). A tie between different items goes to the lower ordinal; a NaN score is kept if
 *    it comes first and never chosen later.
 *  - Memory safety: a candidate outside [0, n_items) (the sampler's -1) is passed over and nothing
 *    of it is dereferenced. A sample whose user lies outside [0, n_users) or which has no
 *    candidate in range gets neg_out = -1 and score_out = NaN, and a training step skips it.
 * Any d >= 1 and ld >= d. Allocates nothing, never synchronises, everything runs on `stream`.
 * LGCN_EINVAL before any launch: B < 0, d < 1, n_neg outside [1, LGCN_BPR_MAX_NEG], ld < d,
 * n_users or n_items < 0; then B == 0 returns 0 and looks at no pointer; then a NULL pointer
 * other than score_out / stream (LGCN_EINVAL). */
int lgcn_bpr_select_hardest(const float* fu, int64_t ld_fu, const float* fi, int64_t ld_fi,
                            int64_t n_users, int64_t n_items, const int64_t* users,
                            const int64_t* cand, int32_t B, int32_t n_neg, int32_t d,
                            int64_t* neg_out, float* score_out, void* stream);

/* ---- sampled-softmax loss over all M candidate negatives of a sample ------------------------- */
/* One softmax per sample over its positive and its M candidates (1 <= M <= LGCN_BPR_MAX_NEG),
 * temperature tau > 0, plus lgcn_bpr_loss's L2 term over the 2 + M layer-0 rows of the sample:
 *   z_0 = <u,p> / tau, z_m = <u,n_m> / tau
 *   L_b = log(sum_j exp(z_j - z_max)) + (z_max - z_0),  j over 0 and the valid m
 *   *loss = mean_b L_b + lambda * (|U0|^2 + |P0|^2 + |N0|^2) / B
 * Rows: u, p, u0, p0 [B x d]; n, n0 [B*M x d], row b * M + m = candidate m of sample b (a
 * contiguous [B, M, d] block). valid (NULL = every entry): uint8 [B x M]; a candidate with
 * valid == 0 is no term of the softmax or of the regulariser, its rows are not read and its two
 * gradient rows are +0. A sample without a valid candidate is skipped: zero terms, +0 gradient
 * rows, zero coefficients, nothing of it read. Both means divide by B whatever was skipped.
 * Orders, all fp32, one wave per sample:
 *  - a score <u,v> is lgcn_bpr_select_hardest's (per lane an fmaf chain over k = lane, lane + 64,
 *    ... from +0, then the 32, 16, ..., 1 xor butterfly); z = fp32(score * it), it = fp32(1 / tau);
 *  - z_max = the maximum over z_0 and the valid z_m; e_j = expf(z_j - z_max);
 *    Z = fp32(e_0 + S), S = the xor butterfly sum over the 64 lanes, lane m holding e_m (+0 for
 *    m >= M or an invalid candidate); L_b = fp32(logf(Z) + fp32(z_max - z_0));
 *  - c = fp32(it / B); g_0 = fp32(fp32(fp32(e_0 / Z) - 1) * c), g_m = fp32(fp32(e_m / Z) * c);
 *  - du[k] = one chain from fp32(g_0 * p[k]), then fmaf(g_m, n_m[k], .) over the valid m in
 *    ascending m; dp = g_0 * u, dn_m = g_m * u; d(row0) = fp32(fp32(2 * lambda) / B) * row0;
 *  - squared norms: per lane one fmaf chain from +0 — over k = lane, lane + 64, ... u0[k]^2 then
 *    p0[k]^2, then each valid candidate's row in ascending m, each over k — then the butterfly;
 *  - *loss = fp32(sl / B) + fp32(fp32(lambda * sr) / B), sl / sr the sums of L_b / of the squared
 *    norms in lgcn_bpr_loss's fixed batch order (256 strided partial sums, then a halving tree).
 * No float atomics: run-to-run identical.
 * grads = [2 x (2+M)B x d]: half 0 the layer-0 gradient rows, half 1 the final ones; inside a
 * half rows [0, B) users, [B, 2B) positives, 2B + b * M + m candidate m of sample b. One
 * permutation of lgcn_ssm_keys' (2+M)B keys therefore indexes either half as lgcn_rows_scatter's
 * source. terms: scratch [2 x B]. coef (NULL = not wanted): [B x (1+M)], g_0, g_1..g_M per
 * sample, 0 for invalid entries.
 * LGCN_EINVAL before any launch: a NULL pointer other than valid / coef / stream, B < 1, d < 1,
 * ld < d, M outside [1, LGCN_BPR_MAX_NEG], (2+M) * B past int32, tau not finite or <= 0. */
int lgcn_ssm_loss(const float* u, int64_t ldu, const float* p, int64_t ldp, const float* n,
                  int64_t ldn, const float* u0, int64_t ldu0, const float* p0, int64_t ldp0,
                  const float* n0, int64_t ldn0, const uint8_t* valid, int32_t B, int32_t M,
                  int32_t d, float lambda, float temperature, float* terms, float* loss,
                  float* grads, float* coef, void* stream);

/* lgcn_ssm_loss with the rows read from the tables (lgcn_bpr_loss_indexed's four): users / pos
 * int64 [B], cand int64 [B x M] row-major (lgcn_bpr_sample_multi's neg). A candidate outside
 * [0, n_items) (the sampler's -1) is invalid; a sample whose user or positive lies outside its
 * table, or without a valid candidate, is skipped; nothing of either is dereferenced. The same
 * kernel body: bitwise lgcn_ssm_loss's outputs on gathered copies with the matching valid mask.
 * Also LGCN_EINVAL: n_users or n_items < 0. */
int lgcn_ssm_loss_indexed(const float* fu, int64_t ld_fu, const float* fi, int64_t ld_fi,
                          const float* u0, int64_t ld_u0, const float* i0, int64_t ld_i0,
                          int64_t n_users, int64_t n_items, const int64_t* users,
                          const int64_t* pos, const int64_t* cand, int32_t B, int32_t M,
                          int32_t d, float lambda, float temperature, float* terms, float* loss,
                          float* grads, float* coef, void* stream);

/* The two above with a logQ correction of the logits (negatives drawn with probability Q, e.g.
 * lgcn_bpr_sample_weighted's w[i] / W): z_0 = fp32(fp32(<u,p> * it) - q_0) and z_m =
 * fp32(fp32(<u,n_m> * it) - q_m), lgcn_inbatch_loss's form; q enters the logits only, every other
 * formula, order and layout is lgcn_ssm_loss's. Gathered: q_pos float32 [B], q_neg [B x M] (the
 * candidate's by ordinal b * M + m); indexed: item_q [n_items], q_0 = item_q[pos[b]], q_m =
 * item_q[cand[b][m]] — bitwise the gathered form on those values (one body). A q pointer may be
 * NULL: no correction of that term; with every q NULL the subtraction is skipped and these are
 * lgcn_ssm_loss / lgcn_ssm_loss_indexed, which call them so. q of a skipped sample or of an
 * invalid candidate is not read. */
int lgcn_ssm_loss_q(const float* u, int64_t ldu, const float* p, int64_t ldp, const float* n,
                    int64_t ldn, const float* u0, int64_t ldu0, const float* p0, int64_t ldp0,
                    const float* n0, int64_t ldn0, const uint8_t* valid, const float* q_pos,
                    const float* q_neg, int32_t B, int32_t M, int32_t d, float lambda,
                    float temperature, float* terms, float* loss, float* grads, float* coef,
                    void* stream);
int lgcn_ssm_loss_indexed_q(const float* fu, int64_t ld_fu, const float* fi, int64_t ld_fi,
                            const float* u0, int64_t ld_u0, const float* i0, int64_t ld_i0,
                            int64_t n_users, int64_t n_items, const int64_t* users,
                            const int64_t* pos, const int64_t* cand, const float* item_q,
                            int32_t B, int32_t M, int32_t d, float lambda, float temperature,
                            float* terms, float* loss, float* grads, float* coef, void* stream);

/* The (2+M)B destination keys of that batch's gradient rows, keys int64 in grads' row order:
 * lgcn_bpr_keys' numbering (2 * row, bit 0 set for a candidate's row). "None" =
 * 2 * (n_users + n_items): every key of a skipped sample, the key of an invalid candidate. Sort
 * with n_keys = none + 1; the stable sort then sums a destination row's negative run in
 * ascending (b, m) and its positive run in ascending b, autograd's index_put order for the 1-D
 * gather indices users, pos and cand.reshape(-1). LGCN_EINVAL: lgcn_bpr_keys' limits, M outside
 * [1, LGCN_BPR_MAX_NEG], (2+M) * B past int32. */
int lgcn_ssm_keys(const int64_t* users, const int64_t* pos, const int64_t* cand, int32_t B,
                  int32_t M, int64_t n_users, int64_t n_items, int64_t* keys, void* stream);

/* ---- in-batch softmax loss: a sample's negatives are the other samples' positives ------------ */
/* One softmax per sample b over the positives of all B samples of the batch, temperature tau > 0,
 * an optional per-column correction q (logQ: the log of an item's share of the interactions), plus
 * lgcn_bpr_loss's L2 term over the sample's two layer-0 rows:
 *   z_bc = <u_b, p_c> / tau - q_c                                   (q = 0 when NULL)
 *   on(b,c) = b and c both valid, and (c == b or not off(b,c))
 *   L_b = log(sum_{c on} exp(z_bc - zmax_b)) + (zmax_b - z_bb)
 *   *loss = mean_b L_b + lambda * (|U0|^2 + |P0|^2) / B
 *   g_bc = (softmax_bc - [c == b]) * fp32(fp32(1/tau) / B),  +0 where not on
 *   du_b = sum_c g_bc p_c,  dp_c = sum_b g_bc u_b,  d(row0) = fp32(fp32(2 * lambda) / B) * row0
 * Rows: u, p, u0, p0 [B x d] (leading dims ld*). off (NULL = none): uint8 [B x B], off[b * B + c]
 * != 0 drops column c from row b (c != b; the diagonal is not looked at). valid (NULL = every
 * sample): uint8 [B]; a sample with valid == 0 is skipped: no row of it is read, it is off as a
 * column of every row, its L_b, squared norms, gradient rows and coefficients are +0. Both means
 * divide by B whatever was skipped. A row with no column on besides its own has L_b = 0 and zero
 * coefficients and keeps its regulariser term. q: float [B], q[c] the correction of column c; it
 * enters the logits only.
 * The B x B logits are never stored: 32 x 32 score tiles are recomputed by each sweep on
 * v_mfma_f32_32x32x2_f32 (exact f32, bitwise an fmaf chain). Orders, all fp32:
 *  - a score <u_b, p_c>: one fmaf chain from +0 over the features in the order 0, 4, 1, 5, 2, 6,
 *    3, 7, then 8, 12, 9, 13, ... (MFMA step 4q + x adds feature 8q + x, then 8q + 4 + x), over
 *    ceil(d / 32) * 32 features, those past d - 1 being +0 products (exact). It depends on the two
 *    rows and d alone, not on B or on where the pair sits; z = fp32(fp32(score * it) - q_c),
 *    it = fp32(1 / tau);
 *  - zmax_b: the maximum over the columns on (exact in any order);
 *  - Z_b: a block of four waves owns users [32 i, 32 i + 32); wave w takes column tiles t = w,
 *    w + 4, ... (columns [32 t, 32 t + 32)) in ascending t. Per wave, lane half h of a user sums
 *    expf(z - zmax) over the columns on of its tiles in ascending t and, inside a tile, over the
 *    local columns (r & 3) + 8 * (r >> 2) + 4 * h in ascending r = 0..15, one add each from +0;
 *    then half 0 + half 1; then the waves ((w0 + w1) + w2) + w3;
 *    L_b = fp32(logf(Z_b) + fp32(zmax_b - z_bb));
 *  - g_bc = fp32(fp32(fp32(expf(z_bc - zmax_b) / Z_b) - [c == b]) * cf), cf = fp32(it / B): one
 *    device function, evaluated by both gradient sweeps on the same score bits;
 *  - du_b[k] (column-tile order) and dp_c[k] (row-tile order): a block of four waves owns 32
 *    output rows; wave w takes the other side's tiles t = w, w + 4, ... in ascending t and keeps
 *    one fmaf chain per output element from +0: per tile 16 MFMA steps r = 0..15, step r adding
 *    the other side's local sample (r & 3) + 8 * (r >> 2), then that + 4 (g * row[k], +0 where not
 *    on or past B); then the waves ((w0 + w1) + w2) + w3;
 *  - squared norms: per lane one fmaf chain from +0 over k = lane, lane + 64, ... of u0[k]^2 then
 *    p0[k]^2, then the 32, 16, ..., 1 xor butterfly;
 *  - *loss = fp32(sl / B) + fp32(fp32(lambda * sr) / B), sl / sr the sums of L_b / of the squared
 *    norms in lgcn_bpr_loss's fixed batch order (256 strided partial sums, then a halving tree).
 * No float atomics: run-to-run identical.
 * grads = [2 x 2B x d]: half 0 the layer-0 gradient rows, half 1 the final ones; inside a half
 * rows [0, B) users, [B, 2B) positives: one permutation of lgcn_inbatch_keys' 2B keys indexes
 * either half as lgcn_rows_scatter's source. work: scratch, float [5 x B] (L_b, squared norms,
 * zmax_b, Z_b, q per column). mask: scratch, uint32 [B x ceil(B / 32)] (the on bits, formed once
 * per batch). coef (NULL = not wanted): [B x B], g_bc; for tests, refused for B >
 * LGCN_INBATCH_MAX_COEF_B. Allocates nothing, never synchronises, everything runs on `stream`.
 * LGCN_EINVAL before any launch: a NULL pointer other than off / valid / q / coef / stream, B
 * outside [1, LGCN_INBATCH_MAX_B], d outside [1, LGCN_INBATCH_MAX_D], ld < d, tau not finite or
 * <= 0. */
#define LGCN_INBATCH_MAX_B      32768
#define LGCN_INBATCH_MAX_D      256
#define LGCN_INBATCH_MAX_COEF_B 4096
int lgcn_inbatch_loss(const float* u, int64_t ldu, const float* p, int64_t ldp, const float* u0,
                      int64_t ldu0, const float* p0, int64_t ldp0, const uint8_t* off,
                      const uint8_t* valid, const float* q, int32_t B, int32_t d, float lambda,
                      float temperature, float* work, uint32_t* mask, float* loss, float* grads,
                      float* coef, void* stream);

/* lgcn_inbatch_loss with the rows read from the tables (lgcn_bpr_loss_indexed's four) by users /
 * pos, int64 [B], and the masks derived on the device. A sample whose user or positive lies
 * outside its table is skipped (valid == 0) and nothing of it is dereferenced. For two valid
 * samples off(b,c) holds when pos[c] == pos[b] (the same item again), or users[c] == users[b]
 * (pos[c] is a known positive of that user), or — pos_rowptr / pos_items given: lgcn_bpr_sample's
 * CSR, int32, [n_users + 1] and the sorted, de-duplicated lists; both NULL = no lists — pos[c] is
 * in the list of users[b] (a binary search). item_q (NULL = none): float [n_items], q_c =
 * item_q[pos[c]]. The same kernel bodies: bitwise lgcn_inbatch_loss's outputs on gathered copies
 * with the matching off / valid / q. Also LGCN_EINVAL: n_users or n_items < 0, one of pos_rowptr /
 * pos_items NULL and the other not. */
int lgcn_inbatch_loss_indexed(const float* fu, int64_t ld_fu, const float* fi, int64_t ld_fi,
                              const float* u0, int64_t ld_u0, const float* i0, int64_t ld_i0,
                              int64_t n_users, int64_t n_items, const int64_t* users,
                              const int64_t* pos, const int32_t* pos_rowptr,
                              const int32_t* pos_items, const float* item_q, int32_t B, int32_t d,
                              float lambda, float temperature, float* work, uint32_t* mask,
                              float* loss, float* grads, float* coef, void* stream);

/* The 2B destination keys of that batch's gradient rows, keys int64 [2 x B] in grads' row order,
 * lgcn_bpr_keys' numbering: 2 * users[b], then 2 * (n_users + pos[b]) (bit 0 clear: an item row is
 * summed as one run in ascending b, autograd's index_put order for the gather index pos). Both
 * keys of a skipped sample are "none" = 2 * (n_users + n_items); sort with n_keys = none + 1.
 * LGCN_EINVAL: a NULL pointer other than stream, B outside [1, LGCN_INBATCH_MAX_B], n_users or
 * n_items < 0, n_users + n_items > 0x3ffffffe (the sort's int32 keys). */
int lgcn_inbatch_keys(const int64_t* users, const int64_t* pos, int32_t B, int64_t n_users,
                      int64_t n_items, int64_t* keys, void* stream);

/* ---- LightGCN_Fusion item pre-layer (models/lightgcn_fusion.py:45-49) ------------------------ */
/* out[i,:] = leaky_relu(weight · [id_emb[i,:] | content[i,:]] + bias, slope) for i < n_items,
 * i.e. F.leaky_relu(nn.Linear(d + c_dim, d)(torch.cat([id, content], 1))) without the
 * concatenation: exact-f32 MFMA GEMM with the bias and activation fused into its epilogue.
 * weight: [d x (d + c_dim)] row-major (nn.Linear.weight), dense; bias: [d] or NULL (NULL = no
 * bias: the bits of an all-zero bias). d in {64, 128}, c_dim in {32, 64, 128}; id_emb, content
 * and out: 16-B aligned rows (pointer and leading dim; weight and bias are read by element).
 * z is an fp32 sum of the d + c_dim products from +0 in a fixed order that does not depend on
 * where the row sits or on n_items, plus the bias; out = z > 0 ? z : z * slope, for any slope
 * (the sign of the output equals the sign of z only for slope >= 0: fusion.py's backward reads
 * it, so its wrapper sends slope < 0 to the torch expression). NaN and infinities follow IEEE
 * arithmetic (0 * inf is a NaN) and stay within their row.
 * Writes exactly out[i, 0..d) for i < n_items: never the columns [d, ld_out) of a row, never a
 * row >= n_items; reads only rows < n_items of id_emb and content.
 * Checks, in this order: n_items < 0, d or c_dim unsupported, a leading dim below its width
 * (LGCN_EINVAL); then n_items == 0 returns 0, launches nothing and looks at no pointer (all may
 * be NULL or misaligned); then id_emb, content, weight or out NULL (LGCN_EINVAL); then id_emb,
 * content or out not 16-B aligned, or a leading dim not a multiple of 4 (LGCN_EALIGN). */
int lgcn_fusion_prelayer(const float* id_emb, int64_t ld_id, const float* content, int64_t ld_c,
                         int32_t n_items, int32_t d, int32_t c_dim, const float* weight,
                         const float* bias, float slope, float* out, int64_t ld_out,
                         void* stream);

/* The pre-layer's backward: from the forward's saved output `out` and g_out = dL/d out
 * ([n_items x d] each), with x = [id_emb | content] and weight W [d x (d + c_dim)] dense:
 *   g[i,o]    = out[i,o] > 0 ? g_out[i,o] : fp32(g_out[i,o] * slope)
 *   d_id[i,k] = sum_o g[i,o] * W[o,k], k < d      d_w[o,k] = sum_i g[i,o] * x[i,k]
 *   d_b[o]    = sum_i g[i,o]
 * Each of d_id / d_w / d_b may be NULL (= not wanted). g is formed in registers and never stored.
 * A zero of either sign or a NaN in `out` takes the slope branch (torch.where(out > 0, ...)). The
 * branch is read from `out`, which has the sign of the pre-activation only for slope >= 0: a
 * caller with slope < 0 must not use this entry (fusion.py refuses it).
 * Both products run on exact-f32 MFMA: every sum below is an fp32 fmaf chain (one rounding per
 * term). No float atomics.
 *  - d_id[i,k]: one chain from +0 over o = 0, 1, ..., d-1. It does not depend on where row i
 *    sits, on n_items or on the launch; a NaN or an infinity stays inside its row.
 *  - d_w / d_b: the rows are cut into chunks of LGCN_FUSION_BWD_CHUNK consecutive rows, chunk c =
 *    rows [c*CHUNK, min((c+1)*CHUNK, n_items)), a chunk into tiles of 32 consecutive rows (the
 *    last one of the last chunk padded with +0 terms, which change no bit).
 *      d_w partial of a chunk: ONE chain from +0 over its tiles in ascending order, the rows of a
 *        tile in the order 0, 16, 1, 17, ..., 15, 31 (at most CHUNK roundings).
 *      d_b partial of a chunk: two plain fp32 sums from +0, `lo` over the rows 0..15 of every
 *        tile and `hi` over the rows 16..31 of every tile, each in ascending row order; the
 *        partial is lo + hi (at most CHUNK/2 + 1 roundings).
 *      Combine, a fixed two-level tree: the partials of every 32 consecutive chunks (chunks
 *        [32j, 32j+32)) are added in ascending order from +0; then the group sums in ascending j
 *        from +0 (at most min(32, n_chunks) + ceil(n_chunks/32) roundings, no more than
 *        n_chunks + 1).
 *    The longest path of a d_w element, the rounding of g_out * slope included, is therefore
 *    R <= CHUNK + n_chunks + 2 roundings, n_chunks = ceil(n_items / CHUNK). The bits depend on
 *    the inputs and n_items only: not on the grid (LGCN_TUNE_FUSION_BWD_BLOCKS), the CU count,
 *    the stream, the run, or which of d_id / d_w / d_b were requested.
 * Shapes as the forward's: d in {64, 128}, c_dim in {32, 64, 128}. out, g_out, id_emb, content
 * and d_id: 16-B aligned rows (pointer and leading dim); weight, d_w [d x (d + c_dim)] dense and
 * d_b [d] are accessed by element. Reads only rows < n_items; writes exactly d_id[i, 0..d) for
 * i < n_items, d_w[0 .. d*(d+c_dim)) and d_b[0..d). ld_did is looked at only when d_id is wanted.
 * scratch (needed only when d_w or d_b is wanted; 4-B aligned, contents opaque):
 * lgcn_fusion_prelayer_backward_scratch_bytes(n_items, d, c_dim) bytes — one slot per chunk, so
 * constant inside a chunk and non-decreasing in n_items; 0 for arguments out of range.
 * Checks, in this order, all on the host before any launch: n_items < 0, d or c_dim unsupported,
 * a leading dim below its width or above 2^24 floats (the kernel addresses the 32 rows of a tile
 * with 32-bit byte offsets) (LGCN_EINVAL); then n_items == 0 returns 0, launches nothing and
 * looks at no pointer (the caller owns zeroing d_w and d_b); then all three outputs NULL returns
 * 0 and launches nothing; then out, g_out, id_emb, content or weight NULL, or, while d_w or d_b
 * is wanted, scratch NULL or scratch_bytes too small (LGCN_EINVAL); then out, g_out, id_emb,
 * content or d_id not 16-B aligned, or a leading dim not a multiple of 4 (LGCN_EALIGN).
 * Allocates nothing, never synchronises, everything on `stream` (capture-safe). */
#define LGCN_FUSION_BWD_CHUNK 2048   /* fixed at build time; a power of two, <= 8192 */
size_t lgcn_fusion_prelayer_backward_scratch_bytes(int32_t n_items, int32_t d, int32_t c_dim);
int lgcn_fusion_prelayer_backward(const float* out, int64_t ld_out, const float* g_out,
                                  int64_t ld_g, const float* id_emb, int64_t ld_id,
                                  const float* content, int64_t ld_c, int32_t n_items, int32_t d,
                                  int32_t c_dim, const float* weight, float slope, float* d_id,
                                  int64_t ld_did, float* d_w, float* d_b, void* scratch,
                                  size_t scratch_bytes, void* stream);

/* ---- evaluation (main.py:404-439) ----------------------------------------------------------- */
/* Item splits for lgcn_score_topk and lgcn_score_rank: ~2 blocks per CU, >= 2048 items per split,
 * <= 256. */
int lgcn_eval_splits(int32_t n_users, int32_t n_items, int32_t n_cu);

/* Fused score + train-item mask + top-k for a batch of users (main.py:420-426) without the
 * [n_users x n_items] score matrix: scores = user_emb[users[b]] · item_emb[i] (exact-f32 MFMA,
 * an ordered fmaf chain), items of user u listed in mask_items[mask_rowptr[u]:mask_rowptr[u+1]]
 * (sorted ascending) score -1e10, ties broken by lower item index. Outputs top_scores/top_idx
 * [n_users x k] in rank order (-inf / -1 past n_items). d in {32, 64, 128, 256}, k in [1, 32], 16-B
 * aligned rows. part_scores/part_idx: scratch [n_splits x n_users x k]. -1e10 is a value, not a
 * sentinel: an unmasked item scoring below it ranks after the masked ones. The sizes and the
 * alignment are checked first; then n_users == 0 returns 0 and touches no pointer (all may be
 * NULL); otherwise every pointer must be non-NULL, except mask_items when every list is empty. */
int lgcn_score_topk(const float* user_emb, int64_t ld_u, const int32_t* users, int32_t n_users,
                    const float* item_emb, int64_t ld_i, int32_t n_items, int32_t d,
                    const int32_t* mask_rowptr, const int32_t* mask_items, int32_t k,
                    int32_t n_splits, float* part_scores, int32_t* part_idx, float* top_scores,
                    int32_t* top_idx, void* stream);

/* Leave-one-out evaluation without a top-k: the rank of one held-out item per batch slot among
 * all items, under lgcn_score_topk's total order (score descending, item index ascending, the
 * user's train items at -1e10, a value and not a sentinel). For slot b with u = users[b] and
 * t = targets[b]:
 *   score(i)        = the ordered fmaf chain lgcn_score_topk computes for (u, i), replaced by
 *                     fp32(-1e10) iff i is in mask_items[mask_rowptr[u]:mask_rowptr[u+1]];
 *   rank[b]         = #{ i in [0, n_items), i != t : score(i) > score(t), or score(i) == score(t)
 *                     and i < t }: the 0-based place t has in lgcn_score_topk's list whenever it
 *                     appears there, for any k; Recall@k = (rank < k), NDCG@k = 1/log2(rank + 2);
 *   target_score[b] = score(t) (-1e10 when t is one of u's train items).
 * A slot whose t lies outside [0, n_items) gets rank -1 and target_score NaN; nothing of it is
 * dereferenced. Every score that enters a comparison is bitwise the MFMA tile's value for its
 * (user, item) pair, and the counts are integers: the result does not depend on n_splits, the
 * launch geometry, the slot's place in the batch or the run. d in {32, 64, 128, 256}, 16-B
 * aligned rows, n_splits in [1, 256] (lgcn_eval_splits). part: scratch [n_splits x n_users];
 * target_score is read back by the later kernels of the call. Allocates nothing, never
 * synchronises, everything on `stream` (capture-safe). The sizes and the alignment are checked
 * first; then n_users == 0 returns 0 and touches no pointer; otherwise every pointer must be
 * non-NULL, except mask_items when every list is empty. */
int lgcn_score_rank(const float* user_emb, int64_t ld_u, const int32_t* users, int32_t n_users,
                    const float* item_emb, int64_t ld_i, int32_t n_items, int32_t d,
                    const int32_t* mask_rowptr, const int32_t* mask_items,
                    const int32_t* targets, int32_t n_splits, int32_t* part, float* target_score,
                    int32_t* rank, void* stream);

/* Several held-out items per user, ranked from one pass over the user's score row. Slot b is user
 * users[b]; its list is the entries e in [target_rowptr[b], target_rowptr[b+1]) of target_items.
 * The offsets are absolute indices into target_items, target_score and rank, and target_rowptr[0]
 * need not be 0: a batch of a larger set is target_rowptr + s with the same three base pointers.
 * Entries outside [target_rowptr[0], target_rowptr[n_users]) are neither read nor written.
 * For every entry e of slot b, rank[e] and target_score[e] equal, bit for bit, what lgcn_score_rank
 * returns for the single slot (users[b], target_items[e]): -1e10 for a target that is a train
 * item, rank -1 and a NaN score for a target outside [0, n_items); the other targets of the list
 * count as ordinary items, a target listed twice gets its rank twice, a list may be in any order
 * and may be empty (nothing is written), a user may appear in several slots. The result does not
 * depend on n_splits, the slot, the order inside a list or the run.
 * The item split is streamed once per 128 slots as long as no list of them has more than 32
 * ranked entries, and once per 32 places of the longest list beyond that; any length works.
 * scratch: lgcn_score_rank_lists_scratch_bytes(n_users, n_targets, n_splits) bytes, 4-B aligned,
 * n_targets = target_rowptr[n_users] - target_rowptr[0] (0 bytes for arguments out of range). The
 * call never reads target_rowptr on the host: a scratch below the size for n_targets = 0 is
 * LGCN_EINVAL, and a slot whose entries lie past the entries the scratch holds is left unwritten.
 * Widths, alignment, strides, n_splits and the order of the checks as lgcn_score_rank's;
 * n_users == 0 returns 0 and touches no pointer. Allocates nothing, never synchronises, reads
 * nothing back, everything on `stream` (capture-safe). */
size_t lgcn_score_rank_lists_scratch_bytes(int32_t n_users, int64_t n_targets, int32_t n_splits);
int lgcn_score_rank_lists(const float* user_emb, int64_t ld_u, const int32_t* users,
                          int32_t n_users, const float* item_emb, int64_t ld_i,
                          int32_t n_items, int32_t d,
                          const int32_t* mask_rowptr, const int32_t* mask_items,
                          const int32_t* target_rowptr, const int32_t* target_items,
                          int32_t n_splits, void* scratch, size_t scratch_bytes,
                          float* target_score, int32_t* rank, void* stream);

/* Recommendation lists: lgcn_score_topk's lists for k in [1, LGCN_TOPK_WIDE_MAX_K], still without
 * the [n_users x n_items] score matrix. For slot b with u = users[b], top_idx[b][j] is the item t
 * for which lgcn_score_rank gives rank j for the slot (u, t), for every j < k, and top_scores[b][j]
 * is that call's target_score, bit for bit: every score that enters a comparison is the MFMA
 * tile's value for its (user row, item row) pair, u's mask items count at fp32(-1e10) (a value,
 * not a sentinel: an unmasked item scoring below it ranks after the masked ones), and the order
 * is score descending, item index ascending. Positions past the number of listable items hold
 * -inf / -1. An item whose score is a NaN (or -inf) is never listed, as in lgcn_score_topk. For
 * k <= 32 both outputs equal lgcn_score_topk's as raw bits. The result does not depend on
 * n_splits, the slot's place in the batch, the launch geometry or the run. users[b] must be a
 * valid row, as for lgcn_score_topk; a user may appear in several slots, and user_emb may be
 * item_emb.
 * A user's candidates (scores above its current k-th best) are kept per (split, slot) in scratch,
 * 2 kp entries with kp the power of two >= max(k, 32); a buffer that could overflow on the next
 * 32-item tile is sorted in LDS (bitonic, at most 2048 pairs per wave) and cut to its k best. The
 * splits' sorted lists are merged by rank: an entry's place is the sum of its binary-search
 * places in the splits' lists.
 * scratch: lgcn_score_topk_wide_scratch_bytes(n_users, k, n_splits) bytes, 4-B aligned, contents
 * opaque: n_splits * n_users * (16 kp + 4) rounded up to 16 (0 for arguments out of range).
 * lgcn_topk_wide_splits: lgcn_eval_splits(n_users, n_items, n_cu), capped so that (a) with more
 * than one split n_items / n_splits >= max(2048, 8 k): a split is several times k long and its
 * list is not most of the split, and (b) n_splits * k <= 16384: the merge stays small. Always in
 * [1, 256]; never grows with n_users. Any n_splits in [1, 256] gives the same lists.
 * Checks, in this order, on the host before any launch: k outside [1, LGCN_TOPK_WIDE_MAX_K]
 * (LGCN_EINVAL); then d, alignment, strides and n_splits in [1, 256] as lgcn_score_rank's; then
 * n_users == 0 returns 0 and touches no pointer (all may be NULL); then a NULL pointer (mask_items
 * may be NULL when every list is empty) or scratch_bytes below the stated size (LGCN_EINVAL); then
 * a scratch that is not 4-B aligned (LGCN_EALIGN). Allocates nothing, never synchronises, reads
 * nothing back, everything on `stream` (capture-safe). */
#define LGCN_TOPK_WIDE_MAX_K 1024
int lgcn_topk_wide_splits(int32_t n_users, int32_t n_items, int32_t k, int32_t n_cu);
size_t lgcn_score_topk_wide_scratch_bytes(int32_t n_users, int32_t k, int32_t n_splits);
int lgcn_score_topk_wide(const float* user_emb, int64_t ld_u, const int32_t* users,
                         int32_t n_users, const float* item_emb, int64_t ld_i, int32_t n_items,
                         int32_t d, const int32_t* mask_rowptr, const int32_t* mask_items,
                         int32_t k, int32_t n_splits, void* scratch, size_t scratch_bytes,
                         float* top_scores, int32_t* top_idx, void* stream);

/* ---- optimizer (main.py's torch.optim.Adam(model.parameters(), lr)) ------------------------- */
/* One Adam step over up to LGCN_ADAM_MAX_TENSORS fp32 tensors in ONE launch, bit for bit what
 * torch.optim.Adam with default arguments leaves on a HIP device (torch 2.10's
 * _multi_tensor_adam, non-capturable branch: seven _foreach passes, every intermediate rounded
 * to fp32). Per element, in fp32, fma = one rounding:
 *     g' = fma(weight_decay, p, g)                       only if weight_decay != 0
 *     m  = |w| < 0.5 ? fma(w, g' - m, m) : fma(-(1 - w), g' - m, g')        w = lerp_w (ATen lerp)
 *     v  = fma(one_minus_beta2, g' * g', v * beta2)
 *     t  = sqrt(v) / bc2_sqrt + eps                      IEEE sqrt and division, three roundings
 *     p  = fma(step_size, m / t, p)                      IEEE division
 * (DESIGN.md §5 "Optimizer" records how each rounding was settled against torch on the GPU.)
 * The caller computes the scalars in double exactly as torch/optim/adam.py does:
 *     lerp_w = 1 - beta1, one_minus_beta2 = 1 - beta2,
 *     step_size = (lr / (1 - beta1 ** step)) * -1,  bc2_sqrt = (1 - beta2 ** step) ** 0.5
 * (per tensor: step counts may differ); the library narrows each to float once, as ATen's opmath
 * cast does.
 * The table is read on the host during the call and travels to the kernel by value in its
 * arguments: no copy, no synchronisation, nothing read back, capture-safe, on `stream`. A block
 * takes one chunk of LGCN_ADAM_CHUNK consecutive elements of one tensor; a tensor whose four
 * pointers are all 16-B aligned is accessed with 16-B loads and stores (scalar for the last
 * n % 4 elements), any other tensor by element. Element counts and offsets are 64-bit.
 * p, g, m and v of all tensors must not overlap (not checked).
 * LGCN_EINVAL, before any HIP call: n_tensors outside [0, LGCN_ADAM_MAX_TENSORS]; with
 * n_tensors > 0 a NULL table or NULL hyper, a non-finite hyper value, n < 0, bc2_sqrt not above
 * 0, a NULL pointer in a tensor with n > 0, or more than 2^24 - 1 chunks in all (the grid).
 * n_tensors == 0 or every n == 0 returns 0 without a launch; a tensor with n == 0 is skipped. */
#define LGCN_ADAM_MAX_TENSORS 16
#define LGCN_ADAM_CHUNK 4096       /* elements per block; a multiple of 1024 */
typedef struct {
    float* p;            /* parameter, updated in place */
    const float* g;      /* gradient, read only */
    float* m;            /* exp_avg, updated in place */
    float* v;            /* exp_avg_sq, updated in place */
    int64_t n;           /* elements */
    double step_size;    /* (lr / bias_correction1) * -1 */
    double bc2_sqrt;     /* bias_correction2 ** 0.5 */
} lgcn_adam_tensor_t;
typedef struct {
    double lerp_w, beta2, one_minus_beta2, eps, weight_decay;
} lgcn_adam_hyper_t;
int     lgcn_adam_step(const lgcn_adam_tensor_t* tensors_host, int32_t n_tensors,
                       const lgcn_adam_hyper_t* hyper, void* stream);
/* host only: the blocks a tensor of n elements takes, ceil(n / LGCN_ADAM_CHUNK) (0 for n <= 0) */
int64_t lgcn_adam_chunks(int64_t n);

#ifdef __cplusplus
}
#endif
#endif /* LGCN_H_ */

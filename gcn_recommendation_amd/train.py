"""One call for a BPR training step (main.py:495-525) that keeps the batch indices.

main.py's route — `model(adj)`, six advanced-index gathers, `bpr_loss_reg`, `loss.backward()` —
makes autograd zero-fill and index_put six dense [rows x d] gradients, after which the engine's
backward searches the dense G for its few thousand live rows again (lgcn_rows_nonzero) and reads
the two dense ego gradients in full (lgcn_add_nonzero). `bpr_step` runs the same arithmetic with
the indices in hand:

    forward   propagate_forward, then lgcn_bpr_loss_indexed on views of its output buffer and of
              the layer-0 tables (no gathered copies); the six per-sample gradient blocks are kept
    backward  the 3B destination keys sorted once (lgcn_bpr_keys, lgcn_coo_sort_perm); the three
              final-row blocks STORE-scattered into a zero workspace together with G's row mask
              and live-row count (lgcn_rows_scatter); propagate_backward on the workspace with
              that mask; the three layer-0 blocks ADD-scattered into dE0's touched rows; the
              workspace rows cleared again (lgcn_rows_clear)

Loss and every parameter gradient are bitwise those of main.py's route: the scatter sums each
destination row in autograd's order (per row from +0 in ascending batch position, an item row's
positive run plus its negative run). Nothing is read back to the host and everything is issued on
the caller's current stream.

With `item_brand` (data.item_brand_map) the reference's optional brand loss (main.py --brand_loss)
joins the same step: a sample has eight rows, the brand rows read from the output buffer's brand
block through the device-resident map (lgcn_bpr_brand_loss_indexed), the batch 5B keys
(lgcn_bpr_brand_keys) and the STORE scatter covers the brand rows of the workspace. Bitwise the
gathered route through loss.bpr_brand_loss_reg.

With a [B, M] `neg` (several candidate negatives per sample, sampler.BprSampler.epoch(n_neg=M))
the step trains on the hardest candidate — dynamic negative sampling — at the cost of one small
kernel: lgcn_bpr_select_hardest runs between the propagation and the loss, on the tables the loss
is about to read, and scores a candidate by the loss kernel's own expression. The route composed
of public calls (model(adj) under no_grad, gather, argmax, bpr_step) propagates twice.

With negatives="softmax" the [B, M] candidates are all used: the sampled-softmax (InfoNCE) loss,
one softmax per sample over its positive and its M candidates with a temperature
(lgcn_ssm_loss_indexed, SsmStepFunction). A sample has 2 + M rows: the batch has (2+M)B
destination keys (lgcn_ssm_keys) and 2(2+M)B gradient rows, where negatives="all" — pairwise BPR on
the B*M expanded triples — has 3BM and 6BM. Bitwise the gathered route through loss.ssm_loss_reg.

`inbatch_step` draws no negative at all: sample b's negatives are the positives of the other
samples of its batch, less the ones that are no true negatives of its user (the in-batch softmax,
lgcn_inbatch_loss_indexed, InBatchStepFunction). The [B, B] logits are recomputed tile by tile on
the exact-f32 MFMA in each sweep and never stored; the batch has 2B rows and 2B destination keys
(lgcn_inbatch_keys). Bitwise the gathered route through loss.inbatch_loss_reg.

`bpr_epoch` is the loop around it (main.py:488-531): the batches are views of one device-side draw
of sampler.BprSampler, the per-batch losses come back as one device tensor.
"""
import ctypes
import weakref

import torch

from . import engine
from .loss import (_check_temperature, bpr_loss_reg, inbatch_loss_torch, inbatch_off_mask,
                   ssm_loss_torch)


class _Workspace:
    """Per (graph, d): the dense [n x d] zero block the final-row gradients are scattered into
    (the autograd route allocates and zero-fills as much every step), its row mask and live-row
    count, and sort scratch for the largest batch seen. Invariant: G, mask and count are all zero
    on entry to and on exit from a step; a step that raises in between leaves `dirty` set and the
    next one re-zeroes them whole. One backward at a time per graph: steps issued on different
    streams at once would share it."""

    def __init__(self, n, d, device):
        self.n, self.d, self.device = n, d, device
        self.G = torch.zeros((n, d), dtype=torch.float32, device=device)
        self.mask = torch.zeros(max((n + 31) // 32, 1), dtype=torch.int32, device=device)
        self.count = torch.zeros(1, dtype=torch.int32, device=device)
        self.dirty = False
        self.cap = 0
        self.temp = self.temp_for = None

    def sort_scratch(self, lib, m, n_keys, stream):
        """Buffers of lgcn_coo_sort_perm for m keys (grown, never shrunk)."""
        if m > self.cap:
            dev = self.device
            self.keys = torch.empty(m, dtype=torch.int64, device=dev)
            self.i32 = torch.empty((4, m), dtype=torch.int32, device=dev)
            self.cap = m
        if self.temp_for != (m, n_keys):
            nbytes = ctypes.c_size_t(0)
            b = self.i32
            engine._check(lib.lgcn_coo_sort_perm(None, m, n_keys, engine._ptr(b[0]),
                                                 engine._ptr(b[1]), engine._ptr(b[2]),
                                                 engine._ptr(b[3]), None, ctypes.byref(nbytes),
                                                 stream), "lgcn_coo_sort_perm(size)")
            if self.temp is None or self.temp.numel() < nbytes.value:
                self.temp = torch.empty(max(nbytes.value, 1), dtype=torch.uint8, device=self.device)
            self.temp_bytes, self.temp_for = nbytes.value, (m, n_keys)

    def rezero(self):
        self.G.zero_()
        self.mask.zero_()
        self.count.zero_()
        self.dirty = False


_graphs = weakref.WeakSet()  # graphs that own workspaces (graph._bpr_workspaces: d -> _Workspace)


def _workspace(graph, d):
    table = graph.__dict__.setdefault("_bpr_workspaces", {})
    ws = table.get(d)
    if ws is None:
        ws = table[d] = _Workspace(graph.n_rows, d, graph.device)
        _graphs.add(graph)
    return ws


def release_workspace(graph=None):
    """Free the step workspaces of `graph` (an engine.Graph), or of every graph."""
    for g in [graph] if graph is not None else list(_graphs):
        g.__dict__.pop("_bpr_workspaces", None)
        _graphs.discard(g)


def _scatter(lib, ws, m, src, lo, hi, dst, mode, mask, count, stream):
    engine._check(lib.lgcn_rows_scatter(engine._ptr(ws.i32[1]), engine._ptr(ws.i32[3]), m,
                                        engine._ptr(src), src.stride(0), lo, hi, engine._ptr(dst),
                                        dst.stride(0), ws.d, mode, engine._ptr(mask),
                                        engine._ptr(count), stream), "lgcn_rows_scatter")


def _check_candidates(cand, device, B=None):
    """A 2-D `neg`: int64 [B, M], contiguous, on `device`, 1 <= M <= engine.BPR_MAX_NEG."""
    if not torch.is_tensor(cand) or cand.dtype != torch.int64:
        raise engine.LgcnError("bpr_step: neg must be an int64 tensor "
                               f"(got {getattr(cand, 'dtype', type(cand))})")
    if cand.dim() != 2 or not cand.is_contiguous():
        raise engine.LgcnError("bpr_step: several negatives per sample are a contiguous "
                               f"[B, M] tensor, got shape {tuple(cand.shape)} strides "
                               f"{cand.stride()}")
    if cand.device != device:
        raise engine.LgcnError(f"bpr_step: neg on {cand.device}, adjacency on {device}")
    if not 1 <= int(cand.shape[1]) <= engine.BPR_MAX_NEG:
        raise engine.LgcnError(f"bpr_step: {int(cand.shape[1])} negatives per sample "
                               f"(1 to {engine.BPR_MAX_NEG})")
    if B is not None and int(cand.shape[0]) != B:
        raise engine.LgcnError("bpr_step: users, pos and neg must have one length")


def select_hardest(fu, fi, users, cand, return_scores=False):
    """lgcn_bpr_select_hardest on the HIP device of `fu`, on the caller's current stream: per
    sample the candidate of cand[b] (int64 [B, M], 1 <= M <= 64) that the final tables fu / fi
    ([rows x d] fp32, unit column stride; row slices of one buffer are fine) score highest for
    users[b], int64 [B]. The first candidate in range is the choice until a later one in range
    scores greater (>): ties go to the lower ordinal, a candidate outside [0, items) (the
    sampler's -1) is passed over, and a sample with no candidate in range or a user out of range
    gets -1. return_scores=True: (negatives, scores), scores[b] bitwise the negative score the
    loss kernel forms for negatives[b] (NaN where the negative is -1)."""
    dev = fu.device
    if dev.type != "cuda":
        raise engine.LgcnError("select_hardest: the tables must be on a HIP device")
    for name, t in (("fu", fu), ("fi", fi)):
        if t.dtype != torch.float32 or t.dim() != 2 or t.device != dev or \
                (t.numel() and t.stride(1) != 1):
            raise engine.LgcnError(f"select_hardest: {name} must be a [rows x d] fp32 table on "
                                   f"{dev} with unit column stride")
    d = int(fu.shape[1])
    if int(fi.shape[1]) != d or d < 1:
        raise engine.LgcnError("select_hardest: fu and fi must have one width d >= 1")
    if not torch.is_tensor(users) or users.dtype != torch.int64 or users.dim() != 1 or \
            users.device != dev or not users.is_contiguous():
        raise engine.LgcnError(f"select_hardest: users must be a contiguous 1-D int64 tensor on "
                               f"{dev}")
    B = int(users.shape[0])
    _check_candidates(cand, dev, B)
    lib = engine.load_library()
    neg = torch.empty(B, dtype=torch.int64, device=dev)
    scores = torch.empty(B, dtype=torch.float32, device=dev) if return_scores else None
    if B:
        with torch.cuda.device(dev):
            engine._check(lib.lgcn_bpr_select_hardest(
                engine._ptr(fu), fu.stride(0) if fu.shape[0] else d, engine._ptr(fi),
                fi.stride(0) if fi.shape[0] else d, int(fu.shape[0]), int(fi.shape[0]),
                engine._ptr(users), engine._ptr(cand), B, int(cand.shape[1]), d,
                engine._ptr(neg), engine._ptr(scores), engine._stream(dev)),
                "lgcn_bpr_select_hardest")
    return (neg, scores) if return_scores else neg


def select_hardest_torch(fu, fi, users, cand):
    """select_hardest's rule in torch ops (what a CPU adjacency runs): (negatives, found), found[b]
    False where no candidate of sample b lies in range or its user does not. Scores are torch's
    own sums, so against the HIP kernel two candidates whose scores differ in the last bits may
    swap: the rule is the same, the bits of a score are not claimed across devices."""
    U, I = int(fu.shape[0]), int(fi.shape[0])
    valid = ((cand >= 0) & (cand < I)) & ((users >= 0) & (users < U)).unsqueeze(1)
    with torch.no_grad():
        rows = fi[cand.clamp(0, max(I - 1, 0))]                       # [B, M, d]
        scores = (fu[users.clamp(0, max(U - 1, 0))].unsqueeze(1) * rows).sum(-1)
    best = torch.full_like(users, -1)
    best_s = torch.zeros(users.shape, dtype=scores.dtype, device=scores.device)
    for m in range(int(cand.shape[1])):  # ascending ordinal: replace only on a greater score
        take = valid[:, m] & ((best < 0) | (scores[:, m] > best_s))
        best = torch.where(take, cand[:, m], best)
        best_s = torch.where(take, scores[:, m], best_s)
    return best, valid.any(1)


class BprStepFunction(torch.autograd.Function):
    """(graph, K, hub_threshold, lambda_reg, users, pos, neg, n_e0, *segments) -> the loss.

    neg [B]: the step on those negatives. neg [B, M] (several candidates per sample): after the
    propagation, lgcn_bpr_select_hardest picks each sample's negative from this step's final
    tables, the ones the loss is about to read; loss, keys and scatter run on the picked [B]
    negatives, which are saved for backward in place of neg, and (loss, negatives) is returned.

    Mirrors engine.PropagateFunction: segments = the (user, item, brand) layer-0 blocks the
    propagation reads; the first n_e0 of them are also the tables the regulariser's rows come
    from. n_e0 = 2 (LightGCN): user and item. n_e0 = 1 (LightGCN_Fusion): the user block only —
    the item block is the pre-layer's output, and one more tensor follows the segments, the item
    id table the regulariser reads, whose gradient (row-sparse, a fresh zero tensor filled by the
    scatter) is returned for it."""

    @staticmethod
    def forward(ctx, graph, K, hub_threshold, lambda_reg, users, pos, neg, n_e0, *segments):
        if n_e0 not in (1, 2):
            raise engine.LgcnError(f"bpr_step: n_e0={n_e0} (1 or 2)")
        nseg = len(segments) - (2 - n_e0)
        if nseg < 2:
            raise engine.LgcnError("bpr_step: user and item segments expected")
        lib = engine.load_library()
        dev = graph.device
        segs = [t.detach() for t in segments[:nseg]]
        sizes = [int(t.shape[0]) for t in segs]
        U, I = sizes[0], sizes[1]
        out = engine.propagate_forward(graph, segs, K, hub_threshold)
        d = int(out.shape[1])
        i0 = segs[1] if n_e0 == 2 else segments[nseg].detach()
        if i0.shape != (I, d) or i0.dtype != torch.float32 or i0.device != dev or \
                (I > 0 and i0.stride(1) != 1):
            raise engine.LgcnError("bpr_step: the item regulariser table must be [items x d] fp32")
        B = int(users.shape[0])
        fu, fi, u0 = out[:U], out[U:U + I], segs[0]
        picked = neg.dim() == 2
        if picked:
            neg = select_hardest(fu, fi, users, neg)
        terms = torch.empty(2 * B, dtype=torch.float32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        grads = torch.empty((6, B, d), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            engine._check(lib.lgcn_bpr_loss_indexed(
                engine._ptr(fu), d, engine._ptr(fi), d, engine._ptr(u0), d, engine._ptr(i0),
                i0.stride(0) if I else d, U, I, engine._ptr(users), engine._ptr(pos),
                engine._ptr(neg), B, d, float(lambda_reg), engine._ptr(terms), engine._ptr(loss),
                engine._ptr(grads), engine._stream(dev)), "lgcn_bpr_loss_indexed")
        ctx.save_for_backward(grads, users, pos, neg)
        ctx.graph, ctx.K, ctx.hub_threshold = graph, K, hub_threshold
        ctx.sizes, ctx.n_e0, ctx.n_inputs = sizes, n_e0, len(segments)
        if picked:
            ctx.mark_non_differentiable(neg)
            return loss, neg
        return loss

    @staticmethod
    def backward(ctx, g, *_):
        grads, users, pos, neg = ctx.saved_tensors
        graph, sizes, n_e0 = ctx.graph, ctx.sizes, ctx.n_e0
        U, I = sizes[0], sizes[1]
        _, B, d = grads.shape
        m = 3 * B
        lib = engine.load_library()
        dev = graph.device
        sg = (grads * g).view(2, m, d)  # BPRLossFunction.backward's scaling, all six blocks
        ws = _workspace(graph, d)
        gi = None
        with torch.cuda.device(dev):
            stream = engine._stream(dev)
            if ws.dirty:
                ws.rezero()
            n_keys = 2 * (U + I) + 1
            ws.sort_scratch(lib, m, n_keys, stream)
            engine._check(lib.lgcn_bpr_keys(engine._ptr(users), engine._ptr(pos), engine._ptr(neg),
                                            B, U, I, engine._ptr(ws.keys), stream), "lgcn_bpr_keys")
            b = ws.i32
            nbytes = ctypes.c_size_t(ws.temp_bytes)
            engine._check(lib.lgcn_coo_sort_perm(engine._ptr(ws.keys), m, n_keys, engine._ptr(b[0]),
                                                 engine._ptr(b[1]), engine._ptr(b[2]),
                                                 engine._ptr(b[3]), engine._ptr(ws.temp),
                                                 ctypes.byref(nbytes), stream),
                          "lgcn_coo_sort_perm")
            ws.dirty = True
            _scatter(lib, ws, m, sg[0], 0, U + I, ws.G, engine.LGCN_SCATTER_STORE, ws.mask,
                     ws.count, stream)
            g0 = engine.propagate_backward(graph, ws.G, ctx.K, ctx.hub_threshold,
                                           nz=(ws.mask, ws.count))
            _scatter(lib, ws, m, sg[1], 0, U + I if n_e0 == 2 else U, g0,
                     engine.LGCN_SCATTER_ADD, None, None, stream)
            if n_e0 == 1:
                gi = torch.zeros((I, d), dtype=torch.float32, device=dev)
                _scatter(lib, ws, m, sg[1], U, U + I, gi, engine.LGCN_SCATTER_STORE, None, None,
                         stream)
            engine._check(lib.lgcn_rows_clear(engine._ptr(b[1]), m, 0, U + I, engine._ptr(ws.G), d,
                                              d, engine._ptr(ws.mask), engine._ptr(ws.count),
                                              stream), "lgcn_rows_clear")
            ws.dirty = False
        blocks = tuple(torch.split(g0, sizes, 0))
        return (None,) * 8 + blocks + ((gi,) if n_e0 == 1 else ())


class BprBrandStepFunction(torch.autograd.Function):
    """(graph, K, hub_threshold, lambda_reg, brand_loss_weight, users, pos, neg, item_brand, n_e0,
    *segments) -> the loss with the brand-preference term (main.py:382-391, 499-522).

    BprStepFunction with eight rows per sample: the brand rows are read from the output buffer's
    brand block through item_brand (lgcn_bpr_brand_loss_indexed), the batch has 5B destination
    keys (lgcn_bpr_brand_keys) and the STORE scatter of the five final-row blocks covers the
    brand rows of the workspace too. The brand segment is required."""

    @staticmethod
    def forward(ctx, graph, K, hub_threshold, lambda_reg, brand_loss_weight, users, pos, neg,
                item_brand, n_e0, *segments):
        if n_e0 not in (1, 2):
            raise engine.LgcnError(f"bpr_step: n_e0={n_e0} (1 or 2)")
        nseg = len(segments) - (2 - n_e0)
        if nseg != 3 or int(segments[2].shape[0]) < 1:
            raise engine.LgcnError("bpr_step: the brand loss needs user, item and brand segments")
        lib = engine.load_library()
        dev = graph.device
        segs = [t.detach() for t in segments[:nseg]]
        sizes = [int(t.shape[0]) for t in segs]
        U, I, NB = sizes
        out = engine.propagate_forward(graph, segs, K, hub_threshold)
        d = int(out.shape[1])
        i0 = segs[1] if n_e0 == 2 else segments[nseg].detach()
        if i0.shape != (I, d) or i0.dtype != torch.float32 or i0.device != dev or \
                (I > 0 and i0.stride(1) != 1):
            raise engine.LgcnError("bpr_step: the item regulariser table must be [items x d] fp32")
        B = int(users.shape[0])
        fu, fi, fb, u0 = out[:U], out[U:U + I], out[U + I:U + I + NB], segs[0]
        picked = neg.dim() == 2
        if picked:  # the brand rows then follow the picked item
            neg = select_hardest(fu, fi, users, neg)
        terms = torch.empty(3 * B, dtype=torch.float32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        grads = torch.empty((8, B, d), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            engine._check(lib.lgcn_bpr_brand_loss_indexed(
                engine._ptr(fu), d, engine._ptr(fi), d, engine._ptr(fb), d, engine._ptr(u0), d,
                engine._ptr(i0), i0.stride(0) if I else d, U, I, NB, engine._ptr(users),
                engine._ptr(pos), engine._ptr(neg), engine._ptr(item_brand), B, d,
                float(lambda_reg), float(brand_loss_weight), engine._ptr(terms),
                engine._ptr(loss), engine._ptr(grads), None, engine._stream(dev)),
                "lgcn_bpr_brand_loss_indexed")
        ctx.save_for_backward(grads, users, pos, neg, item_brand)
        ctx.graph, ctx.K, ctx.hub_threshold = graph, K, hub_threshold
        ctx.sizes, ctx.n_e0 = sizes, n_e0
        if picked:
            ctx.mark_non_differentiable(neg)
            return loss, neg
        return loss

    @staticmethod
    def backward(ctx, g, *_):
        grads, users, pos, neg, item_brand = ctx.saved_tensors
        graph, sizes, n_e0 = ctx.graph, ctx.sizes, ctx.n_e0
        U, I, NB = sizes
        n = U + I + NB
        _, B, d = grads.shape
        m = 5 * B
        lib = engine.load_library()
        dev = graph.device
        # the layer-0 blocks [3B x d], then the final-row blocks [5B x d] (include/lgcn.h): a
        # permutation entry of the 5B keys stays inside sg whichever source it indexes
        sg = (grads * g).view(8 * B, d)
        ws = _workspace(graph, d)
        gi = None
        with torch.cuda.device(dev):
            stream = engine._stream(dev)
            if ws.dirty:
                ws.rezero()
            n_keys = 2 * n + 1
            ws.sort_scratch(lib, m, n_keys, stream)
            engine._check(lib.lgcn_bpr_brand_keys(engine._ptr(users), engine._ptr(pos),
                                                  engine._ptr(neg), engine._ptr(item_brand), B, U,
                                                  I, NB, engine._ptr(ws.keys), stream),
                          "lgcn_bpr_brand_keys")
            b = ws.i32
            nbytes = ctypes.c_size_t(ws.temp_bytes)
            engine._check(lib.lgcn_coo_sort_perm(engine._ptr(ws.keys), m, n_keys, engine._ptr(b[0]),
                                                 engine._ptr(b[1]), engine._ptr(b[2]),
                                                 engine._ptr(b[3]), engine._ptr(ws.temp),
                                                 ctypes.byref(nbytes), stream),
                          "lgcn_coo_sort_perm")
            ws.dirty = True
            _scatter(lib, ws, m, sg[3 * B:], 0, n, ws.G, engine.LGCN_SCATTER_STORE, ws.mask,
                     ws.count, stream)
            g0 = engine.propagate_backward(graph, ws.G, ctx.K, ctx.hub_threshold,
                                           nz=(ws.mask, ws.count))
            _scatter(lib, ws, m, sg, 0, U + I if n_e0 == 2 else U, g0,
                     engine.LGCN_SCATTER_ADD, None, None, stream)
            if n_e0 == 1:
                gi = torch.zeros((I, d), dtype=torch.float32, device=dev)
                _scatter(lib, ws, m, sg, U, U + I, gi, engine.LGCN_SCATTER_STORE, None, None,
                         stream)
            engine._check(lib.lgcn_rows_clear(engine._ptr(b[1]), m, 0, n, engine._ptr(ws.G), d,
                                              d, engine._ptr(ws.mask), engine._ptr(ws.count),
                                              stream), "lgcn_rows_clear")
            ws.dirty = False
        blocks = tuple(torch.split(g0, sizes, 0))
        return (None,) * 10 + blocks + ((gi,) if n_e0 == 1 else ())


class SsmStepFunction(torch.autograd.Function):
    """(graph, K, hub_threshold, lambda_reg, temperature, users, pos, cand, item_q, n_e0,
    *segments) -> the sampled-softmax loss over all M candidates of cand [B, M]
    (loss.ssm_loss_reg's expression), segments as BprStepFunction's; item_q: the float32
    [items] logQ correction looked up by item index (lgcn_ssm_loss_indexed_q), or None.

    BprStepFunction with 2 + M rows per sample: lgcn_ssm_loss_indexed reads them from the output
    buffer and the layer-0 tables and keeps grads = [2 x (2+M)B x d] (layer-0 half, final half,
    one row layout); the batch has (2+M)B destination keys (lgcn_ssm_keys), sorted once. A user
    row and a positive row are read, differentiated and scattered once per sample, not M times."""

    @staticmethod
    def forward(ctx, graph, K, hub_threshold, lambda_reg, temperature, users, pos, cand, item_q,
                n_e0, *segments):
        if n_e0 not in (1, 2):
            raise engine.LgcnError(f"bpr_step: n_e0={n_e0} (1 or 2)")
        nseg = len(segments) - (2 - n_e0)
        if nseg < 2:
            raise engine.LgcnError("bpr_step: user and item segments expected")
        lib = engine.load_library()
        dev = graph.device
        segs = [t.detach() for t in segments[:nseg]]
        sizes = [int(t.shape[0]) for t in segs]
        U, I = sizes[0], sizes[1]
        out = engine.propagate_forward(graph, segs, K, hub_threshold)
        d = int(out.shape[1])
        i0 = segs[1] if n_e0 == 2 else segments[nseg].detach()
        if i0.shape != (I, d) or i0.dtype != torch.float32 or i0.device != dev or \
                (I > 0 and i0.stride(1) != 1):
            raise engine.LgcnError("bpr_step: the item regulariser table must be [items x d] fp32")
        if item_q is not None:
            _check_item_log_q(item_q, I, dev, "bpr_step: neg_log_q")
        B, M = int(cand.shape[0]), int(cand.shape[1])
        fu, fi, u0 = out[:U], out[U:U + I], segs[0]
        terms = torch.empty(2 * B, dtype=torch.float32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        grads = torch.empty((2, (2 + M) * B, d), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            engine._check(lib.lgcn_ssm_loss_indexed_q(
                engine._ptr(fu), d, engine._ptr(fi), d, engine._ptr(u0), d, engine._ptr(i0),
                i0.stride(0) if I else d, U, I, engine._ptr(users), engine._ptr(pos),
                engine._ptr(cand), engine._ptr(item_q), B, M, d, float(lambda_reg),
                float(temperature), engine._ptr(terms), engine._ptr(loss), engine._ptr(grads),
                None, engine._stream(dev)), "lgcn_ssm_loss_indexed_q")
        ctx.save_for_backward(grads, users, pos, cand)
        ctx.graph, ctx.K, ctx.hub_threshold = graph, K, hub_threshold
        ctx.sizes, ctx.n_e0 = sizes, n_e0
        return loss

    @staticmethod
    def backward(ctx, g):
        grads, users, pos, cand = ctx.saved_tensors
        graph, sizes, n_e0 = ctx.graph, ctx.sizes, ctx.n_e0
        U, I = sizes[0], sizes[1]
        _, m, d = grads.shape
        B, M = int(cand.shape[0]), int(cand.shape[1])
        lib = engine.load_library()
        dev = graph.device
        sg = grads * g  # SSMLossFunction.backward's scaling: [0] the layer-0 half, [1] the final
        ws = _workspace(graph, d)
        gi = None
        with torch.cuda.device(dev):
            stream = engine._stream(dev)
            if ws.dirty:
                ws.rezero()
            n_keys = 2 * (U + I) + 1
            ws.sort_scratch(lib, m, n_keys, stream)
            engine._check(lib.lgcn_ssm_keys(engine._ptr(users), engine._ptr(pos),
                                            engine._ptr(cand), B, M, U, I, engine._ptr(ws.keys),
                                            stream), "lgcn_ssm_keys")
            b = ws.i32
            nbytes = ctypes.c_size_t(ws.temp_bytes)
            engine._check(lib.lgcn_coo_sort_perm(engine._ptr(ws.keys), m, n_keys, engine._ptr(b[0]),
                                                 engine._ptr(b[1]), engine._ptr(b[2]),
                                                 engine._ptr(b[3]), engine._ptr(ws.temp),
                                                 ctypes.byref(nbytes), stream),
                          "lgcn_coo_sort_perm")
            ws.dirty = True
            _scatter(lib, ws, m, sg[1], 0, U + I, ws.G, engine.LGCN_SCATTER_STORE, ws.mask,
                     ws.count, stream)
            g0 = engine.propagate_backward(graph, ws.G, ctx.K, ctx.hub_threshold,
                                           nz=(ws.mask, ws.count))
            _scatter(lib, ws, m, sg[0], 0, U + I if n_e0 == 2 else U, g0,
                     engine.LGCN_SCATTER_ADD, None, None, stream)
            if n_e0 == 1:
                gi = torch.zeros((I, d), dtype=torch.float32, device=dev)
                _scatter(lib, ws, m, sg[0], U, U + I, gi, engine.LGCN_SCATTER_STORE, None, None,
                         stream)
            engine._check(lib.lgcn_rows_clear(engine._ptr(b[1]), m, 0, U + I, engine._ptr(ws.G), d,
                                              d, engine._ptr(ws.mask), engine._ptr(ws.count),
                                              stream), "lgcn_rows_clear")
            ws.dirty = False
        blocks = tuple(torch.split(g0, sizes, 0))
        return (None,) * 10 + blocks + ((gi,) if n_e0 == 1 else ())


class InBatchStepFunction(torch.autograd.Function):
    """(graph, K, hub_threshold, lambda_reg, temperature, users, pos, rowptr, items, item_q, n_e0,
    *segments) -> the in-batch softmax loss (loss.inbatch_loss_reg's expression with
    loss.inbatch_off_mask(users, pos, (rowptr, items)) and q = item_q[pos]); rowptr / items and
    item_q are device tensors or None, segments as BprStepFunction's.

    SsmStepFunction with 2B rows and nothing drawn: lgcn_inbatch_loss_indexed reads the batch's
    rows from the output buffer and the layer-0 tables and keeps grads = [2 x 2B x d] (layer-0
    half, final half, one row layout); the batch has 2B destination keys (lgcn_inbatch_keys),
    sorted once. The same workspace, STORE and ADD scatter and clear."""

    @staticmethod
    def forward(ctx, graph, K, hub_threshold, lambda_reg, temperature, users, pos, rowptr, items,
                item_q, n_e0, *segments):
        if n_e0 not in (1, 2):
            raise engine.LgcnError(f"inbatch_step: n_e0={n_e0} (1 or 2)")
        nseg = len(segments) - (2 - n_e0)
        if nseg < 2:
            raise engine.LgcnError("inbatch_step: user and item segments expected")
        lib = engine.load_library()
        dev = graph.device
        segs = [t.detach() for t in segments[:nseg]]
        sizes = [int(t.shape[0]) for t in segs]
        U, I = sizes[0], sizes[1]
        out = engine.propagate_forward(graph, segs, K, hub_threshold)
        d = int(out.shape[1])
        i0 = segs[1] if n_e0 == 2 else segments[nseg].detach()
        if i0.shape != (I, d) or i0.dtype != torch.float32 or i0.device != dev or \
                (I > 0 and i0.stride(1) != 1):
            raise engine.LgcnError("inbatch_step: the item regulariser table must be [items x d] "
                                   "fp32")
        B = int(users.shape[0])
        fu, fi, u0 = out[:U], out[U:U + I], segs[0]
        work = torch.empty(5 * B, dtype=torch.float32, device=dev)
        bits = torch.empty(B * ((B + 31) // 32), dtype=torch.int32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        grads = torch.empty((2, 2 * B, d), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            engine._check(lib.lgcn_inbatch_loss_indexed(
                engine._ptr(fu), d, engine._ptr(fi), d, engine._ptr(u0), d, engine._ptr(i0),
                i0.stride(0) if I else d, U, I, engine._ptr(users), engine._ptr(pos),
                engine._ptr(rowptr), engine._ptr(items), engine._ptr(item_q), B, d,
                float(lambda_reg), float(temperature), engine._ptr(work), engine._ptr(bits),
                engine._ptr(loss), engine._ptr(grads), None, engine._stream(dev)),
                "lgcn_inbatch_loss_indexed")
        ctx.save_for_backward(grads, users, pos)
        ctx.graph, ctx.K, ctx.hub_threshold = graph, K, hub_threshold
        ctx.sizes, ctx.n_e0 = sizes, n_e0
        return loss

    @staticmethod
    def backward(ctx, g):
        grads, users, pos = ctx.saved_tensors
        graph, sizes, n_e0 = ctx.graph, ctx.sizes, ctx.n_e0
        U, I = sizes[0], sizes[1]
        _, m, d = grads.shape
        B = m // 2
        lib = engine.load_library()
        dev = graph.device
        sg = grads * g  # InBatchLossFunction.backward's scaling: [0] the layer-0 half, [1] the final
        ws = _workspace(graph, d)
        gi = None
        with torch.cuda.device(dev):
            stream = engine._stream(dev)
            if ws.dirty:
                ws.rezero()
            n_keys = 2 * (U + I) + 1
            ws.sort_scratch(lib, m, n_keys, stream)
            engine._check(lib.lgcn_inbatch_keys(engine._ptr(users), engine._ptr(pos), B, U, I,
                                                engine._ptr(ws.keys), stream), "lgcn_inbatch_keys")
            b = ws.i32
            nbytes = ctypes.c_size_t(ws.temp_bytes)
            engine._check(lib.lgcn_coo_sort_perm(engine._ptr(ws.keys), m, n_keys, engine._ptr(b[0]),
                                                 engine._ptr(b[1]), engine._ptr(b[2]),
                                                 engine._ptr(b[3]), engine._ptr(ws.temp),
                                                 ctypes.byref(nbytes), stream),
                          "lgcn_coo_sort_perm")
            ws.dirty = True
            _scatter(lib, ws, m, sg[1], 0, U + I, ws.G, engine.LGCN_SCATTER_STORE, ws.mask,
                     ws.count, stream)
            g0 = engine.propagate_backward(graph, ws.G, ctx.K, ctx.hub_threshold,
                                           nz=(ws.mask, ws.count))
            _scatter(lib, ws, m, sg[0], 0, U + I if n_e0 == 2 else U, g0,
                     engine.LGCN_SCATTER_ADD, None, None, stream)
            if n_e0 == 1:
                gi = torch.zeros((I, d), dtype=torch.float32, device=dev)
                _scatter(lib, ws, m, sg[0], U, U + I, gi, engine.LGCN_SCATTER_STORE, None, None,
                         stream)
            engine._check(lib.lgcn_rows_clear(engine._ptr(b[1]), m, 0, U + I, engine._ptr(ws.G), d,
                                              d, engine._ptr(ws.mask), engine._ptr(ws.count),
                                              stream), "lgcn_rows_clear")
            ws.dirty = False
        blocks = tuple(torch.split(g0, sizes, 0))
        return (None,) * 11 + blocks + ((gi,) if n_e0 == 1 else ())


def _check_item_brand(item_brand, num_items, device):
    if not torch.is_tensor(item_brand) or item_brand.dtype != torch.int32:
        raise engine.LgcnError("bpr_step: item_brand must be an int32 tensor (data.item_brand_map),"
                               f" got {getattr(item_brand, 'dtype', type(item_brand))}")
    if item_brand.dim() != 1 or int(item_brand.shape[0]) != num_items or \
            not item_brand.is_contiguous():
        raise engine.LgcnError(f"bpr_step: item_brand must be a contiguous 1-D tensor of "
                               f"{num_items} entries, got {tuple(item_brand.shape)}")
    if item_brand.device != device:
        raise engine.LgcnError(f"bpr_step: item_brand on {item_brand.device}, adjacency on "
                               f"{device}")


def _check_index_tensors(users, pos, neg, device):
    B = None
    many = torch.is_tensor(neg) and neg.dim() != 1  # [B, M]: several negatives per sample
    for name, t in (("users", users), ("pos", pos)) + ((() if many else (("neg", neg),))):
        if not torch.is_tensor(t) or t.dtype != torch.int64:
            raise engine.LgcnError(f"bpr_step: {name} must be an int64 tensor "
                                   f"(got {getattr(t, 'dtype', type(t))})")
        if t.dim() != 1:
            raise engine.LgcnError(f"bpr_step: {name} must be 1-D, got {tuple(t.shape)}")
        if t.device != device:
            raise engine.LgcnError(f"bpr_step: {name} on {t.device}, adjacency on {device}")
        if B is None:
            B = int(t.shape[0])
        elif int(t.shape[0]) != B:
            raise engine.LgcnError("bpr_step: users, pos and neg must have one length")
    if many:
        _check_candidates(neg, device, B)
    if B < 1:
        raise engine.LgcnError("bpr_step: empty batch")


def _cpu_loss(tables, users, pos, neg, lambda_reg, item_brand, brand_loss_weight):
    """The reference's own expression on model(adj)'s five tables (the CPU route)."""
    fu, fi, fb, u0, i0 = tables
    if item_brand is None:
        return bpr_loss_reg(fu[users], fi[pos], fi[neg], u0[users], i0[pos], i0[neg],
                            lambda_reg, final_brand_emb=fb)
    pb, nb = item_brand[pos].long(), item_brand[neg].long()
    n_brands = int(fb.shape[0])
    if bool(((pb < 0) | (pb >= n_brands) | (nb < 0) | (nb >= n_brands)).any()):
        raise engine.LgcnError("bpr_step: an item of the batch has no brand; the CPU route "
                               "cannot leave the sample out of the brand term")
    return bpr_loss_reg(fu[users], fi[pos], fi[neg], u0[users], i0[pos], i0[neg], lambda_reg,
                        brand_loss=True, final_brand_emb=fb, pos_item_brand_idx=pb,
                        neg_item_brand_idx=nb, brand_loss_weight=brand_loss_weight)


def bpr_step(model, adj, users, pos, neg, lambda_reg, check_indices=False, *, item_brand=None,
             brand_loss_weight=0.1, negatives="hardest", return_negatives=False,
             temperature=1.0, neg_log_q=None):
    """The loss of one BPR batch (main.py:495-522) as a tensor whose
    `.backward()` leaves exactly the parameter `.grad`s main.py's route leaves:

        optimizer.zero_grad()
        loss = model.bpr_step(adj, users, pos, neg, weight_decay)
        loss.backward(); optimizer.step()

    users / pos / neg: 1-D int64 tensors on the adjacency's device (wrong dtype, device or rank
    raises LgcnError before any launch). check_indices=True also validates them against the table
    sizes with torch ops first (one sync) and raises LgcnError; by default nothing is checked or
    synchronised — the kernels are memory-safe either way (a sample with an index outside its
    table is skipped). On a CPU adjacency the reference's own expression runs (model(adj), the
    gathers, the torch formula): the device dispatch of the models and loss.py.

    item_brand (data.item_brand_map: a contiguous int32 [num_items] tensor on the adjacency's
    device, -1 = no brand; anything else raises LgcnError before any launch) switches the
    reference's brand loss on (main.py --brand_loss): the loss is `bpr + brand_loss_weight *
    brand + reg`, the brand rows of a sample are looked up on the device, and loss and `.grad`s
    are bitwise those of the gathered route through loss.bpr_brand_loss_reg. A sample whose
    positive or negative item has no brand contributes no brand term (the mean still divides by
    the batch size). item_brand=None or brand_loss_weight == 0 is the step without the term. On a
    CPU adjacency bpr_loss_reg(brand_loss=True, ...) runs; an unbranded item in the batch raises
    LgcnError there, where the reference's indexing would take -1 for the last brand.

    Several negatives per sample: neg of shape [B, M] (int64, contiguous, on the adjacency's
    device, 1 <= M <= 64, e.g. a batch of sampler.epoch(..., n_neg=M); anything else raises
    LgcnError before any launch). A 1-D neg is the step above and `negatives` is not looked at.
      negatives="hardest"  dynamic negative sampling: each sample trains on the candidate this
          step's model scores highest. The choice is made inside the step, between its one
          propagation and the loss (lgcn_bpr_select_hardest on the final tables the loss then
          reads; select_hardest states the rule: first maximum, lowest ordinal, candidates
          outside [0, items) passed over, a sample without one skipped). Loss and `.grad`s are
          bitwise those of bpr_step(adj, users, pos, chosen); with item_brand the brand rows
          follow the chosen item.
      negatives="all"  BPR over the B*M pairs: by definition the step on
          users.repeat_interleave(M), pos.repeat_interleave(M), neg.reshape(-1) — main.py's
          formula on the expanded triples (its means divide by B*M).
      negatives="softmax"  the sampled-softmax (InfoNCE) loss: one softmax per sample over its
          positive and all M candidates, logits divided by `temperature` (a finite number > 0,
          else ValueError), plus the L2 term over the sample's 2 + M layer-0 rows; both means
          divide by B (loss.ssm_loss_reg states the expression). One propagation, then
          lgcn_ssm_loss_indexed on views of its output: a user row and a positive row are read,
          differentiated and scattered once per sample, and the batch has (2+M)B scatter keys
          where "all" has 3BM. Loss and `.grad`s are bitwise those of the gathered route (model(adj),
          fu[users], fi[pos], fi[neg.reshape(-1)].view(B, M, d), the same of the layer-0 tables,
          loss.ssm_loss_reg, backward). A candidate outside [0, items) (the sampler's -1) is no
          term of the softmax or of the regulariser; a sample without one in range is skipped.
          With item_brand (and a weight != 0) it raises LgcnError before any launch: the brand
          term has no softmax form here. On a CPU adjacency the torch expression runs and a
          candidate out of range raises LgcnError.
          neg_log_q (sampler.neg_log_q(): a contiguous float32 [num_items] tensor on the
          adjacency's device, else LgcnError before any launch) is the logQ correction of
          negatives drawn with probability Q: the logits become <u, i> / temperature -
          neg_log_q[i] for the positive and every candidate (lgcn_ssm_loss_indexed_q), still
          bitwise the gathered route through loss.ssm_loss_reg(q_pos=neg_log_q[pos],
          q_neg=neg_log_q[neg]). It belongs to this mode alone: with another, or with a 1-D
          neg, it raises ValueError ("hardest" and "all" train on weighted candidates as given).
    Any other value raises ValueError. return_negatives=True returns (loss, neg_used), the int64
    negatives the loss ran on: [B] for "hardest" (and for a 1-D neg, neg itself), [B*M] for "all",
    neg as given for "softmax". With a 1-D neg neither negatives nor temperature is looked at.
    check_indices=True validates every entry of a 2-D neg. On a CPU adjacency model(adj) runs
    once, the candidates are scored and chosen with torch ops by the same rule
    (select_hardest_torch) and the reference expression runs on the choice; a sample without a
    candidate in range raises LgcnError (the reference's indexing would take -1 for the last
    item; bpr_epoch refuses a neg = -1 there for the same reason). The choice is not claimed
    bitwise across devices: torch sums a score in another order, so two candidates whose scores
    differ in the last bits can swap."""
    _check_index_tensors(users, pos, neg, adj.device)
    U, I = model.num_users, model.num_items
    brand = item_brand is not None and brand_loss_weight != 0
    if brand:
        _check_item_brand(item_brand, I, adj.device)
    many = neg.dim() == 2
    if many and negatives not in ("hardest", "all", "softmax"):
        raise ValueError(f"bpr_step: negatives={negatives!r} ('hardest', 'all' or 'softmax')")
    softmax = many and negatives == "softmax"
    if neg_log_q is not None:
        if not softmax:
            raise ValueError("bpr_step: neg_log_q belongs to a [B, M] neg with "
                             "negatives='softmax'")
        _check_item_log_q(neg_log_q, I, adj.device, "bpr_step: neg_log_q")
    if softmax:
        temperature = _check_temperature(temperature, "bpr_step")
        if brand:
            raise engine.LgcnError("bpr_step: negatives='softmax' has no brand term (item_brand "
                                   "must be None or brand_loss_weight 0)")
    if check_indices:
        for name, t, n in (("users", users, U), ("pos", pos, I), ("neg", neg, I)):
            if bool(((t < 0) | (t >= n)).any()):
                raise engine.LgcnError(f"bpr_step: {name} holds an index outside [0, {n})")
    if many and negatives == "all":
        M = int(neg.shape[1])
        return bpr_step(model, adj, users.repeat_interleave(M), pos.repeat_interleave(M),
                        neg.reshape(-1), lambda_reg, item_brand=item_brand,
                        brand_loss_weight=brand_loss_weight, return_negatives=return_negatives)
    if adj.device.type != "cuda":
        if softmax and bool(((neg < 0) | (neg >= I)).any()):
            raise engine.LgcnError("bpr_step: a candidate negative is out of range; the CPU "
                                   "route cannot leave it out of the softmax")
        tables = model(adj)
        if softmax:
            fu, fi, _, u0, i0 = tables
            B, M = neg.shape
            flat = neg.reshape(-1)
            q = {} if neg_log_q is None else {"q_pos": neg_log_q[pos],
                                              "q_neg": neg_log_q[flat].view(B, M)}
            loss = ssm_loss_torch(fu[users], fi[pos], fi[flat].view(B, M, -1), u0[users], i0[pos],
                                  i0[flat].view(B, M, -1), lambda_reg, temperature, **q)
            return (loss, neg) if return_negatives else loss
        if many:
            neg, found = select_hardest_torch(tables[0], tables[1], users, neg)
            if not bool(found.all()):
                raise engine.LgcnError("bpr_step: a sample has no candidate negative in range; "
                                       "the CPU route cannot skip the sample")
        loss = _cpu_loss(tables, users, pos, neg, lambda_reg, item_brand if brand else None,
                         brand_loss_weight)
        return (loss, neg) if return_negatives else loss
    n_e0 = model._bpr_n_e0
    if n_e0 == 2:
        tensors = [model.user_embedding.weight, model.item_embedding.weight,
                   model.brand_embedding.weight]
    else:
        tensors = [model.user_embedding.weight, model.fused_item_embedding(),
                   model.brand_embedding.weight, model.item_id_embedding.weight]
    graph = engine.graph_from_coo(adj, sides=engine.segment_sides(tensors[:3]))
    if softmax:
        loss = SsmStepFunction.apply(graph, model.n_layers, engine.hub_threshold_from_env(),
                                     float(lambda_reg), temperature, users, pos, neg, neg_log_q,
                                     n_e0, *tensors)
        return (loss, neg) if return_negatives else loss
    if brand:
        out = BprBrandStepFunction.apply(graph, model.n_layers, engine.hub_threshold_from_env(),
                                         float(lambda_reg), float(brand_loss_weight), users, pos,
                                         neg, item_brand, n_e0, *tensors)
    else:
        out = BprStepFunction.apply(graph, model.n_layers, engine.hub_threshold_from_env(),
                                    float(lambda_reg), users, pos, neg, n_e0, *tensors)
    loss, used = out if many else (out, neg)  # a 2-D neg: (loss, the chosen negatives)
    return (loss, used) if return_negatives else loss


def _check_inbatch_tensors(users, pos, device):
    for name, t in (("users", users), ("pos", pos)):
        if not torch.is_tensor(t) or t.dtype != torch.int64:
            raise engine.LgcnError(f"inbatch_step: {name} must be an int64 tensor "
                                   f"(got {getattr(t, 'dtype', type(t))})")
        if t.dim() != 1 or not t.is_contiguous():
            raise engine.LgcnError(f"inbatch_step: {name} must be 1-D and contiguous, got "
                                   f"{tuple(t.shape)}")
        if t.device != device:
            raise engine.LgcnError(f"inbatch_step: {name} on {t.device}, adjacency on {device}")
    B = int(users.shape[0])
    if int(pos.shape[0]) != B:
        raise engine.LgcnError("inbatch_step: users and pos must have one length")
    if not 1 <= B <= engine.INBATCH_MAX_B:
        raise engine.LgcnError(f"inbatch_step: a batch of {B} (1 to {engine.INBATCH_MAX_B})")


def _check_positives(positives, num_users, device):
    """`positives` of inbatch_step as the (rowptr, items) pair the kernel takes."""
    if hasattr(positives, "positives"):  # a sampler.BprSampler
        if positives.num_users != num_users:
            raise engine.LgcnError(f"inbatch_step: the sampler has {positives.num_users} users, "
                                   f"the model {num_users}")
        positives = positives.positives()
    if not isinstance(positives, (tuple, list)) or len(positives) != 2:
        raise engine.LgcnError("inbatch_step: positives must be a BprSampler or a (rowptr, items) "
                               "pair")
    rowptr, items = positives
    for name, t in (("rowptr", rowptr), ("items", items)):
        if not torch.is_tensor(t) or t.dtype != torch.int32 or t.dim() != 1 or \
                not t.is_contiguous():
            raise engine.LgcnError(f"inbatch_step: positives {name} must be a contiguous 1-D "
                                   f"int32 tensor, got {getattr(t, 'dtype', type(t))}")
        if t.device != device:
            raise engine.LgcnError(f"inbatch_step: positives {name} on {t.device}, adjacency on "
                                   f"{device}")
    if int(rowptr.numel()) != num_users + 1:
        raise engine.LgcnError(f"inbatch_step: positives rowptr must hold {num_users + 1} "
                               f"entries, got {int(rowptr.numel())}")
    if int(items.numel()) == 0:  # no list holds anything, and an empty tensor has no pointer
        return None
    return rowptr, items


def _check_item_log_q(q, num_items, device, what="inbatch_step: item_log_q"):
    if not torch.is_tensor(q) or q.dtype != torch.float32:
        raise engine.LgcnError(f"{what} must be a float32 tensor, got "
                               f"{getattr(q, 'dtype', type(q))}")
    if q.dim() != 1 or int(q.shape[0]) != num_items or not q.is_contiguous():
        raise engine.LgcnError(f"{what} must be a contiguous 1-D tensor of "
                               f"{num_items} entries, got {tuple(q.shape)}")
    if q.device != device:
        raise engine.LgcnError(f"{what} on {q.device}, adjacency on {device}")


def inbatch_step(model, adj, users, pos, lambda_reg, temperature=1.0, *, positives=None,
                 item_log_q=None, check_indices=False):
    """The in-batch softmax loss of one batch as a tensor whose `.backward()` leaves the
    parameter `.grad`s of the gathered route (model(adj), fu[users], fi[pos], the same of the
    layer-0 tables, loss.inbatch_loss_reg with loss.inbatch_off_mask, backward), bit for bit:

        optimizer.zero_grad()
        loss = model.inbatch_step(adj, users, pos, weight_decay, 0.2, positives=sampler)
        loss.backward(); optimizer.step()

    Sample b's negatives are the positives of the other samples of its batch: B - 1 negatives per
    sample and no drawn one, so the step reads, differentiates and scatters 2B rows where the
    plain step has 3B and negatives="softmax" (2 + M)B. loss.inbatch_loss_torch states the
    expression: logits <fu[users[b]], fi[pos[c]]> / temperature - item_log_q[pos[c]], one softmax
    per row, plus the L2 term over the 2B layer-0 rows; both means divide by B. One propagation,
    then lgcn_inbatch_loss_indexed on views of its output: the [B, B] logits are never stored.

    A column c is dropped from row b (c != b) when it is no true negative of users[b]: the same
    item again, the same user again, or — positives given: a sampler.BprSampler, or its
    `positives()` pair (rowptr, items) of int32 tensors on the adjacency's device — pos[c] in the
    known positives of users[b]. A row left with no column but its own contributes a zero
    softmax term and keeps its regulariser term. item_log_q (sampler.item_log_q(): float32
    [num_items] on the adjacency's device) is the logQ correction of the logits.

    users / pos: 1-D contiguous int64 tensors of one length in [1, 32768] on the adjacency's
    device; the embedding width at most 256. A wrong dtype, device, rank or length of any tensor
    raises LgcnError before any launch, a temperature that is no finite number > 0 ValueError.
    check_indices=True validates users and pos against the table sizes with torch ops first (one
    sync); by default a sample with an index outside its table is skipped: nothing of it is
    read, it is no column of any row, its terms and gradient rows are zero. On a CPU adjacency
    the torch expression runs and an index out of range raises LgcnError."""
    temperature = _check_temperature(temperature, "inbatch_step")
    dev = adj.device
    _check_inbatch_tensors(users, pos, dev)
    U, I = model.num_users, model.num_items
    pair = None if positives is None else _check_positives(positives, U, dev)
    if item_log_q is not None:
        _check_item_log_q(item_log_q, I, dev)
    d = getattr(model, "embedding_dim", None)
    if dev.type == "cuda" and d is not None and not 1 <= int(d) <= engine.INBATCH_MAX_D:
        raise engine.LgcnError(f"inbatch_step: embedding width {d} (1 to {engine.INBATCH_MAX_D})")
    if check_indices or dev.type != "cuda":
        for name, t, n in (("users", users, U), ("pos", pos, I)):
            if bool(((t < 0) | (t >= n)).any()):
                raise engine.LgcnError(f"inbatch_step: {name} holds an index outside [0, {n})")
    if dev.type != "cuda":
        fu, fi, _, u0, i0 = model(adj)
        return inbatch_loss_torch(fu[users], fi[pos], u0[users], i0[pos], lambda_reg, temperature,
                                  off=inbatch_off_mask(users, pos, pair),
                                  q=None if item_log_q is None else item_log_q[pos])
    n_e0 = model._bpr_n_e0
    if n_e0 == 2:
        tensors = [model.user_embedding.weight, model.item_embedding.weight,
                   model.brand_embedding.weight]
    else:
        tensors = [model.user_embedding.weight, model.fused_item_embedding(),
                   model.brand_embedding.weight, model.item_id_embedding.weight]
    graph = engine.graph_from_coo(adj, sides=engine.segment_sides(tensors[:3]))
    rowptr, items = pair if pair is not None else (None, None)
    return InBatchStepFunction.apply(graph, model.n_layers, engine.hub_threshold_from_env(),
                                     float(lambda_reg), temperature, users, pos, rowptr, items,
                                     item_log_q, n_e0, *tensors)


def bpr_epoch(model, adj, sampler, optimizer, lambda_reg, batch_size, epoch, shuffle=True,
              item_brand=None, brand_loss_weight=0.1, n_neg=None, negatives="hardest",
              temperature=1.0, *, mask_positives=False, log_q=False, neg_log_q=False):
    """One training epoch (main.py:488-531) that never leaves the device: the sampler draws the
    epoch's (user, positive, negative) triples in one launch (sampler.BprSampler.epoch), then per
    batch

        optimizer.zero_grad(); loss = model.bpr_step(adj, users, pos, neg, lambda_reg)
        loss.backward(); optimizer.step()

    on views of that draw. Returns the per-batch losses as one tensor on the adjacency's device
    (empty for a sampler without interactions); nothing is read back inside the loop. A sample
    whose user has no free item carries neg = -1: on a HIP device bpr_step skips it
    (sampler.unsampled counts them); on a CPU adjacency, where the reference's own indexing would
    take -1 for the last item, it raises before the first optimizer step. item_brand and
    brand_loss_weight are bpr_step's: the brand loss of every batch, looked up on the device.
    Any optimizer works; `optim.Adam(model.parameters(), lr)` keeps the whole step inside the
    engine (one launch, lgcn_adam_step) and leaves torch.optim.Adam's bits.

    n_neg (None = the epoch above; an integer in [1, 64]) is passed to sampler.epoch: the draw
    holds n_neg candidate negatives per sample and every batch's neg is [batch, n_neg]; negatives
    ("hardest", "all" or "softmax") is bpr_step's and says what the step does with them;
    temperature is the softmax step's. neg_log_q=True (with an integer n_neg and
    negatives="softmax", else ValueError) passes sampler.neg_log_q() to every step as its
    `neg_log_q`: the logQ correction that matches the sampler's draw, what a sampler built with
    weights needs for an unbiased softmax.

    negatives="in_batch" (with n_neg=None; an integer n_neg raises ValueError): every batch runs
    model.inbatch_step(adj, users, pos, lambda_reg, temperature) — the in-batch softmax, a
    sample's negatives being the other samples' positives; the draw's neg column is not used (a
    neg = -1 is therefore no obstacle on a CPU adjacency). mask_positives=True passes the
    sampler's own positive lists as `positives`, log_q=True sampler.item_log_q() as `item_log_q`;
    either with another `negatives` raises ValueError. item_brand with a non-zero weight raises
    LgcnError, as "softmax" does: the brand term has no softmax form here."""
    if sampler.device != adj.device:
        raise engine.LgcnError(f"bpr_epoch: sampler on {sampler.device}, adjacency on {adj.device}")
    in_batch = negatives == "in_batch"
    if (mask_positives or log_q) and not in_batch:
        raise ValueError("bpr_epoch: mask_positives and log_q belong to negatives='in_batch'")
    if neg_log_q and (n_neg is None or negatives != "softmax"):
        raise ValueError("bpr_epoch: neg_log_q belongs to an integer n_neg with "
                         "negatives='softmax'")
    if in_batch:
        if n_neg is not None:
            raise ValueError("bpr_epoch: negatives='in_batch' draws no negatives (n_neg must be "
                             f"None, got {n_neg!r})")
        temperature = _check_temperature(temperature, "bpr_epoch")
        if item_brand is not None and brand_loss_weight != 0:
            raise engine.LgcnError("bpr_epoch: negatives='in_batch' has no brand term")
        extra = {"positives": sampler if mask_positives else None,
                 "item_log_q": sampler.item_log_q() if log_q else None}
        losses = []
        for users, pos, _ in sampler.epoch(epoch, batch_size, shuffle=shuffle):
            optimizer.zero_grad()
            loss = model.inbatch_step(adj, users, pos, lambda_reg, temperature, **extra)
            loss.backward()
            optimizer.step()
            losses.append(loss.detach())
        if not losses:
            return torch.empty(0, dtype=torch.float32, device=adj.device)
        return torch.stack(losses)
    if n_neg is not None and negatives not in ("hardest", "all", "softmax"):
        raise ValueError(f"bpr_epoch: negatives={negatives!r} ('hardest', 'all' or 'softmax')")
    if n_neg is not None and negatives == "softmax":
        temperature = _check_temperature(temperature, "bpr_epoch")
        if item_brand is not None and brand_loss_weight != 0:
            raise engine.LgcnError("bpr_epoch: negatives='softmax' has no brand term")
    # the draw is made here
    batches = sampler.epoch(epoch, batch_size, shuffle=shuffle, n_neg=n_neg)
    if adj.device.type != "cuda" and int(sampler.unsampled.item()):
        raise engine.LgcnError("bpr_epoch: a user has every item as a positive (no negative to "
                               "draw); the CPU route cannot skip the sample")
    many = {} if n_neg is None else {"negatives": negatives, "temperature": temperature}
    if neg_log_q:
        many["neg_log_q"] = sampler.neg_log_q()
    losses = []
    for users, pos, neg in batches:
        optimizer.zero_grad()
        loss = model.bpr_step(adj, users, pos, neg, lambda_reg, item_brand=item_brand,
                              brand_loss_weight=brand_loss_weight, **many)
        loss.backward()
        optimizer.step()
        losses.append(loss.detach())
    if not losses:
        return torch.empty(0, dtype=torch.float32, device=adj.device)
    return torch.stack(losses)

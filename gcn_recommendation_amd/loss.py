"""BPR-loss API kept from the reference (main.py:366-402), callable exactly as main.py:515-522.

On a HIP device the base BPR term and the L2 term run as ONE fused kernel (lgcn_bpr_loss,
csrc/lgcn_bpr.hip): both dot products, log-sigmoid, the squared norms of the layer-0 rows and
all six input gradients in one pass, the batch mean in a fixed order. On CPU tensors the
reference's own torch expression runs (device dispatch, as the models do). The brand-loss branch
(dead in the reference snapshot: main.py:505/509 never define item_to_brand) stays the
reference's torch expression on either device in bpr_loss_reg; bpr_brand_loss_reg is the same
call with the brand term fused into the launch (lgcn_bpr_brand_loss). Arithmetic: BPR = -mean(log(sigmoid(pos - neg)
+ 1e-8)), L2 of the layer-0 rows / batch size; fp32 reductions, so GPU parity with the
reference is a tolerance (tests/test_gpu_parity.py::test_fused_bpr_loss_vs_torch).
"""
import numbers

import torch

from . import engine


class BPRLossFunction(torch.autograd.Function):
    """Fused forward; the gradients are produced by the same launch and scaled on backward."""

    @staticmethod
    def forward(ctx, u, p, n, u0, p0, n0, lambda_reg):
        lib = engine.load_library()
        B, d = u.shape
        xs = [t.detach() for t in (u, p, n, u0, p0, n0)]
        for t in xs:
            if t.shape != (B, d) or t.dtype != torch.float32 or t.stride(1) != 1:
                raise engine.LgcnError("bpr_loss: six [B x d] fp32 row-major blocks expected")
        dev = u.device
        terms = torch.empty(2 * B, dtype=torch.float32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        grads = torch.empty((6, B, d), dtype=torch.float32, device=dev)
        args = []
        for t in xs:
            args += [engine._ptr(t), t.stride(0)]
        with torch.cuda.device(dev):
            engine._check(lib.lgcn_bpr_loss(*args, B, d, float(lambda_reg), engine._ptr(terms),
                                            engine._ptr(loss), engine._ptr(grads),
                                            engine._stream(dev)), "lgcn_bpr_loss")
        ctx.save_for_backward(grads)
        return loss

    @staticmethod
    def backward(ctx, g):
        (grads,) = ctx.saved_tensors
        return tuple(grads[i] * g for i in range(6)) + (None,)


class BPRBrandLossFunction(torch.autograd.Function):
    """BPRLossFunction with the brand-preference term (lgcn_bpr_brand_loss): eight gathered
    blocks in, (u, p, n, u0, p0, n0, bp, bn), then brand_ok (uint8 [B] or None), lambda and the
    brand weight; the eight gradient blocks come from the same launch."""

    ORDER = (3, 4, 5, 0, 1, 2, 6, 7)  # input i's block in grads (u0, p0, n0, u, p, n, bp, bn)

    @staticmethod
    def forward(ctx, u, p, n, u0, p0, n0, bp, bn, brand_ok, lambda_reg, brand_loss_weight):
        lib = engine.load_library()
        B, d = u.shape
        xs = [t.detach() for t in (u, p, n, u0, p0, n0, bp, bn)]
        for t in xs:
            if t.shape != (B, d) or t.dtype != torch.float32 or t.stride(1) != 1:
                raise engine.LgcnError("bpr_brand_loss: eight [B x d] fp32 row-major blocks "
                                       "expected")
        dev = u.device
        if brand_ok is not None and (brand_ok.shape != (B,) or brand_ok.dtype != torch.uint8 or
                                     brand_ok.device != dev or not brand_ok.is_contiguous()):
            raise engine.LgcnError("bpr_brand_loss: brand_ok must be a contiguous uint8 [B] tensor")
        terms = torch.empty(3 * B, dtype=torch.float32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        grads = torch.empty((8, B, d), dtype=torch.float32, device=dev)
        args = []
        for t in xs:
            args += [engine._ptr(t), t.stride(0)]
        with torch.cuda.device(dev):
            engine._check(lib.lgcn_bpr_brand_loss(*args, engine._ptr(brand_ok), B, d,
                                                  float(lambda_reg), float(brand_loss_weight),
                                                  engine._ptr(terms), engine._ptr(loss),
                                                  engine._ptr(grads), None, engine._stream(dev)),
                          "lgcn_bpr_brand_loss")
        ctx.save_for_backward(grads)
        return loss

    @staticmethod
    def backward(ctx, g):
        (grads,) = ctx.saved_tensors
        return tuple(grads[i] * g for i in BPRBrandLossFunction.ORDER) + (None, None, None)


def _torch_bpr(u, p, n):
    pos_scores = torch.sum(u * p, dim=1)
    neg_scores = torch.sum(u * n, dim=1)
    return -torch.mean(torch.log(torch.sigmoid(pos_scores - neg_scores) + 1e-8))


def bpr_loss_reg(final_user_emb, final_pos_item_emb, final_neg_item_emb,
                 initial_user_emb, initial_pos_item_emb, initial_neg_item_emb,
                 lambda_reg,
                 brand_loss=False,
                 final_brand_emb=None,
                 pos_item_brand_idx=None,
                 neg_item_brand_idx=None,
                 brand_loss_weight=0.1):
    brand_loss_val = 0.0
    if brand_loss and final_brand_emb is not None:
        pos_brand_emb = final_brand_emb[pos_item_brand_idx]
        neg_brand_emb = final_brand_emb[neg_item_brand_idx]
        brand_loss_val = _torch_bpr(final_user_emb, pos_brand_emb, neg_brand_emb)

    if final_user_emb.device.type == "cuda":
        base = BPRLossFunction.apply(final_user_emb, final_pos_item_emb, final_neg_item_emb,
                                     initial_user_emb, initial_pos_item_emb,
                                     initial_neg_item_emb, float(lambda_reg))
        return base + brand_loss_weight * brand_loss_val if brand_loss_val != 0.0 else base

    bpr_loss = _torch_bpr(final_user_emb, final_pos_item_emb, final_neg_item_emb)
    reg_loss = lambda_reg * (
        initial_user_emb.norm(2).pow(2)
        + initial_pos_item_emb.norm(2).pow(2)
        + initial_neg_item_emb.norm(2).pow(2)
    ) / float(len(final_user_emb))
    return bpr_loss + brand_loss_weight * brand_loss_val + reg_loss


def bpr_brand_loss_reg(final_user_emb, final_pos_item_emb, final_neg_item_emb,
                       initial_user_emb, initial_pos_item_emb, initial_neg_item_emb,
                       lambda_reg,
                       brand_loss=False,
                       final_brand_emb=None,
                       pos_item_brand_idx=None,
                       neg_item_brand_idx=None,
                       brand_loss_weight=0.1):
    """bpr_loss_reg (same signature, same call as main.py:515-522) with the brand term fused: on
    a HIP device `bpr + brand_loss_weight * brand + reg` and all eight input gradients come from
    one launch (lgcn_bpr_brand_loss) — the two brand gathers are made here, the other six by the
    caller. A sample whose positive or negative brand index lies outside the brand table (-1 =
    the item has no brand, data.item_brand_map) has no brand term; the mean still divides by the
    batch size. On CPU tensors, or without brand_loss / final_brand_emb, this is bpr_loss_reg."""
    if final_user_emb.device.type != "cuda" or not brand_loss or final_brand_emb is None:
        return bpr_loss_reg(final_user_emb, final_pos_item_emb, final_neg_item_emb,
                            initial_user_emb, initial_pos_item_emb, initial_neg_item_emb,
                            lambda_reg, brand_loss, final_brand_emb, pos_item_brand_idx,
                            neg_item_brand_idx, brand_loss_weight)
    n_brands = int(final_brand_emb.shape[0])
    if n_brands < 1:
        raise engine.LgcnError("bpr_brand_loss_reg: an empty brand table")
    pi, ni = pos_item_brand_idx.long(), neg_item_brand_idx.long()
    ok = (pi >= 0) & (pi < n_brands) & (ni >= 0) & (ni < n_brands)
    # an unbranded sample gathers row 0 in place of its brand rows: the kernel does not read them
    # and returns +0 gradient rows for them, which leave row 0's sum as it is
    pi, ni = pi.clamp(0, n_brands - 1), ni.clamp(0, n_brands - 1)
    return BPRBrandLossFunction.apply(final_user_emb, final_pos_item_emb, final_neg_item_emb,
                                      initial_user_emb, initial_pos_item_emb,
                                      initial_neg_item_emb, final_brand_emb[pi],
                                      final_brand_emb[ni], ok.to(torch.uint8), float(lambda_reg),
                                      float(brand_loss_weight))


class SSMLossFunction(torch.autograd.Function):
    """BPRLossFunction's sibling for the sampled-softmax loss (lgcn_ssm_loss): (u, p, n, u0, p0,
    n0, valid, lambda, temperature) with n / n0 the [B, M, d] candidate blocks and valid a uint8
    [B, M] mask or None; the six gradient blocks come from the same launch. q_pos (float32 [B])
    and q_neg (float32 [B, M]), each or None: the logQ correction (lgcn_ssm_loss_q)."""

    @staticmethod
    def forward(ctx, u, p, n, u0, p0, n0, valid, lambda_reg, temperature, q_pos=None,
                q_neg=None):
        lib = engine.load_library()
        B, d = u.shape
        if n.dim() != 3 or int(n.shape[0]) != B or not 1 <= int(n.shape[1]) <= engine.BPR_MAX_NEG:
            raise engine.LgcnError("ssm_loss: the negatives must be a [B, M, d] block, 1 <= M <= "
                                   f"{engine.BPR_MAX_NEG}, got {tuple(n.shape)}")
        M = int(n.shape[1])
        dev = u.device
        rows = [t.detach() for t in (u, p, u0, p0)]
        for t in rows:
            if t.shape != (B, d) or t.dtype != torch.float32 or t.stride(1) != 1 or \
                    t.device != dev:
                raise engine.LgcnError("ssm_loss: four [B x d] fp32 row-major blocks expected")
        blocks = [t.detach() for t in (n, n0)]
        for t in blocks:
            if t.shape != (B, M, d) or t.dtype != torch.float32 or t.stride(2) != 1 or \
                    t.stride(0) != M * t.stride(1) or t.device != dev:
                raise engine.LgcnError("ssm_loss: two [B, M, d] fp32 blocks with evenly strided "
                                       "rows expected")
        if valid is not None and (valid.shape != (B, M) or valid.dtype != torch.uint8 or
                                  valid.device != dev or not valid.is_contiguous()):
            raise engine.LgcnError("ssm_loss: valid must be a contiguous uint8 [B, M] tensor")
        for name, t, shape in (("q_pos", q_pos, (B,)), ("q_neg", q_neg, (B, M))):
            if t is not None and (not torch.is_tensor(t) or t.shape != shape or
                                  t.dtype != torch.float32 or t.device != dev or
                                  not t.is_contiguous()):
                raise engine.LgcnError(f"ssm_loss: {name} must be a contiguous float32 tensor of "
                                       f"shape {shape} on {dev}")
        terms = torch.empty(2 * B, dtype=torch.float32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        grads = torch.empty((2, (2 + M) * B, d), dtype=torch.float32, device=dev)
        xu, xp, xu0, xp0 = rows
        args = []
        for t, ld in ((xu, xu.stride(0)), (xp, xp.stride(0)), (blocks[0], blocks[0].stride(1)),
                      (xu0, xu0.stride(0)), (xp0, xp0.stride(0)),
                      (blocks[1], blocks[1].stride(1))):
            args += [engine._ptr(t), ld]
        with torch.cuda.device(dev):
            engine._check(lib.lgcn_ssm_loss_q(*args, engine._ptr(valid), engine._ptr(q_pos),
                                              engine._ptr(q_neg), B, M, d, float(lambda_reg),
                                              float(temperature), engine._ptr(terms),
                                              engine._ptr(loss), engine._ptr(grads), None,
                                              engine._stream(dev)), "lgcn_ssm_loss_q")
        ctx.save_for_backward(grads)
        ctx.dims = (B, M, d)
        return loss

    @staticmethod
    def backward(ctx, g):
        (grads,) = ctx.saved_tensors
        B, M, d = ctx.dims
        sg = grads * g
        out = []
        for half in (1, 0):  # the final rows, then the layer-0 rows
            out += [sg[half, :B], sg[half, B:2 * B], sg[half, 2 * B:].view(B, M, d)]
        return tuple(out) + (None,) * 5


def _check_temperature(temperature, what):
    if isinstance(temperature, bool) or not isinstance(temperature, numbers.Real) or \
            not temperature > 0 or temperature == float("inf"):
        raise ValueError(f"{what}: temperature={temperature!r} (a finite number > 0)")
    return float(temperature)


def ssm_loss_torch(final_user_emb, final_pos_item_emb, final_neg_item_emb, initial_user_emb,
                   initial_pos_item_emb, initial_neg_item_emb, lambda_reg, temperature=1.0,
                   valid=None, q_pos=None, q_neg=None):
    """The sampled-softmax loss as a torch expression, in the dtype of its inputs: what a CPU
    adjacency runs, and the reference the HIP kernel is measured against. q_pos [B] / q_neg
    [B, M], each or None: the logQ correction, subtracted from the logits after the division."""
    u, p, n = final_user_emb, final_pos_item_emb, final_neg_item_emb
    u0, p0, n0 = initial_user_emb, initial_pos_item_emb, initial_neg_item_emb
    pos_scores = torch.sum(u * p, dim=1)
    neg_scores = torch.sum(u.unsqueeze(1) * n, dim=-1)
    if valid is not None:
        on = valid.bool()
        keep = on.any(1)  # a sample without a valid candidate is skipped whole
        neg_scores = neg_scores.masked_fill(~on, float("-inf"))
        n0 = n0 * on.unsqueeze(-1).to(n0.dtype)
        u0 = u0 * keep.unsqueeze(-1).to(u0.dtype)
        p0 = p0 * keep.unsqueeze(-1).to(p0.dtype)
    logits = torch.cat([pos_scores.unsqueeze(1), neg_scores], dim=1) / temperature
    if q_pos is not None or q_neg is not None:
        q = torch.zeros_like(logits)
        if q_pos is not None:
            q[:, 0] = q_pos.to(logits.dtype)
        if q_neg is not None:
            q[:, 1:] = q_neg.to(logits.dtype)
        if valid is not None:  # the q of a masked candidate or of a skipped sample is not read
            q[:, 1:] = q[:, 1:].masked_fill(~on, 0.0)
            q[:, 0] = q[:, 0].masked_fill(~keep, 0.0)
        logits = logits - q
    ssm = torch.mean(torch.logsumexp(logits, dim=1) - logits[:, 0])
    reg = lambda_reg * (u0.norm(2).pow(2) + p0.norm(2).pow(2) + n0.norm(2).pow(2)) / float(len(u))
    return ssm + reg


def ssm_loss_reg(final_user_emb, final_pos_item_emb, final_neg_item_emb,
                 initial_user_emb, initial_pos_item_emb, initial_neg_item_emb,
                 lambda_reg, temperature=1.0, valid=None, q_pos=None, q_neg=None):
    """Sampled-softmax (InfoNCE) loss over all M negatives of a sample, plus bpr_loss_reg's L2
    term: bpr_loss_reg's call with [B, M, d] negative blocks.

        z_0 = <u, p> / temperature - q_pos, z_m = <u, n_m> / temperature - q_neg[:, m]
        loss = mean_b (logsumexp_j z_j - z_0) + lambda_reg * (|U0|^2 + |P0|^2 + |N0|^2) / B

    valid (None = every entry): a uint8 or bool [B, M] mask; a candidate with valid == 0 is no
    term of the softmax or of the regulariser, a sample without a valid candidate contributes
    nothing; the means still divide by B. q_pos (float32 [B]) / q_neg (float32 [B, M]), each or
    None = no such term: the logQ correction of negatives drawn with probability Q — the log
    probabilities of the positive and of each candidate (sampler.neg_log_q()[pos] and [neg]); it
    enters the logits only. On a HIP device loss and all six input gradients come
    from one launch (lgcn_ssm_loss, include/lgcn.h states its orders of summation); on CPU
    tensors ssm_loss_torch runs."""
    temperature = _check_temperature(temperature, "ssm_loss_reg")
    if final_user_emb.device.type != "cuda":
        return ssm_loss_torch(final_user_emb, final_pos_item_emb, final_neg_item_emb,
                              initial_user_emb, initial_pos_item_emb, initial_neg_item_emb,
                              lambda_reg, temperature, valid, q_pos, q_neg)
    if valid is not None and valid.dtype == torch.bool:
        valid = valid.to(torch.uint8)
    return SSMLossFunction.apply(final_user_emb, final_pos_item_emb, final_neg_item_emb,
                                 initial_user_emb, initial_pos_item_emb, initial_neg_item_emb,
                                 valid, float(lambda_reg), temperature, q_pos, q_neg)


# ---- in-batch softmax: a sample's negatives are the other samples' positives --------------------
def inbatch_off_mask(users, pos, positives=None):
    """off[b, c] of the in-batch softmax as a bool [B, B] (torch tensors in, a tensor on their
    device out; numpy arrays in, an array out): column c is no true negative of row b when
    pos[c] == pos[b] (the same item again), users[c] == users[b] (pos[c] is a known positive of
    that user) or, with positives = (rowptr, items) — the sampler's sorted, de-duplicated per-user
    lists (BprSampler.positives()) — pos[c] lies in the list of users[b] (a user outside the CSR
    has no list). The diagonal is False: a sample's own positive is always a column of its row.
    What lgcn_inbatch_loss_indexed derives on the device, stated with torch ops: for tests, for
    the gathered route (inbatch_loss_reg) and for the CPU route."""
    as_numpy = not torch.is_tensor(users)
    users, pos = torch.as_tensor(users).long(), torch.as_tensor(pos).long()
    B = int(users.shape[0])
    off = (pos.unsqueeze(0) == pos.unsqueeze(1)) | (users.unsqueeze(0) == users.unsqueeze(1))
    if positives is not None:
        rowptr = torch.as_tensor(positives[0]).to(users.device).long()
        items = torch.as_tensor(positives[1]).to(users.device).long()
        n_users = int(rowptr.numel()) - 1
        if n_users > 0 and items.numel() > 0:
            ok = (users >= 0) & (users < n_users)
            uc = users.clamp(0, n_users - 1)
            lo = torch.where(ok, rowptr[uc], torch.zeros_like(uc))
            hi = torch.where(ok, rowptr[uc + 1], torch.zeros_like(uc))
            lo, hi = lo.unsqueeze(1).repeat(1, B), hi.unsqueeze(1).repeat(1, B)
            target = pos.unsqueeze(0).expand(B, B)
            found = torch.zeros((B, B), dtype=torch.bool, device=users.device)
            while True:  # the kernel's binary search, every pair advanced one step per round
                act = lo < hi
                if not bool(act.any()):
                    break
                mid = (lo + hi) >> 1
                v = items[mid.clamp(max=items.numel() - 1)]
                found |= act & (v == target)
                lo = torch.where(act & (v < target), mid + 1, lo)
                hi = torch.where(act & (v >= target), mid, hi)
            off |= found
    off.fill_diagonal_(False)
    return off.numpy() if as_numpy else off


def inbatch_loss_torch(final_user_emb, final_pos_item_emb, initial_user_emb,
                       initial_pos_item_emb, lambda_reg, temperature=1.0, off=None, valid=None,
                       q=None):
    """The in-batch softmax loss as a torch expression, in the dtype of its inputs: what a CPU
    adjacency runs, and the reference the HIP kernels are measured against.

        z_bc = <u_b, p_c> / temperature - q_c,   on(b, c) = (c == b) or not off[b, c]
        loss = mean_b (logsumexp_{c on} z_bc - z_bb) + lambda_reg * (|U0|^2 + |P0|^2) / B

    off: bool or uint8 [B, B] (inbatch_off_mask), its diagonal not looked at; valid: bool or
    uint8 [B], a sample with valid == 0 is skipped — off as a column of every row, no term of its
    own, no regulariser term; q: [B], the correction of column c. Both means divide by B."""
    u, p, u0, p0 = final_user_emb, final_pos_item_emb, initial_user_emb, initial_pos_item_emb
    B = int(u.shape[0])
    logits = (u @ p.t()) / temperature
    if q is not None:
        logits = logits - q.to(logits.dtype).unsqueeze(0)
    eye = torch.eye(B, dtype=torch.bool, device=u.device)
    on = torch.ones((B, B), dtype=torch.bool, device=u.device)
    if off is not None:
        on = ~off.bool() | eye
    keep = None
    if valid is not None:
        keep = valid.bool()
        on = on & keep.unsqueeze(0) & keep.unsqueeze(1)
        on = on | ~keep.unsqueeze(1)  # a skipped row: any finite logits, its term is dropped below
    masked = logits.masked_fill(~on, float("-inf"))
    terms = torch.logsumexp(masked, dim=1) - torch.diagonal(logits)
    if keep is not None:
        terms = torch.where(keep, terms, torch.zeros_like(terms))
        u0 = u0 * keep.unsqueeze(-1).to(u0.dtype)
        p0 = p0 * keep.unsqueeze(-1).to(p0.dtype)
    reg = lambda_reg * (u0.norm(2).pow(2) + p0.norm(2).pow(2)) / float(B)
    return torch.mean(terms) + reg


class InBatchLossFunction(torch.autograd.Function):
    """SSMLossFunction's sibling for the in-batch softmax loss (lgcn_inbatch_loss): (u, p, u0, p0,
    off, valid, q, lambda, temperature) with off a uint8 [B, B] mask, valid a uint8 [B] mask and q
    a float32 [B] correction, each or None; the four gradient blocks come from the same launches."""

    @staticmethod
    def forward(ctx, u, p, u0, p0, off, valid, q, lambda_reg, temperature):
        lib = engine.load_library()
        B, d = u.shape
        dev = u.device
        rows = [t.detach() for t in (u, p, u0, p0)]
        for t in rows:
            if t.shape != (B, d) or t.dtype != torch.float32 or t.stride(1) != 1 or \
                    t.device != dev:
                raise engine.LgcnError("inbatch_loss: four [B x d] fp32 row-major blocks expected")
        if not 1 <= B <= engine.INBATCH_MAX_B or not 1 <= d <= engine.INBATCH_MAX_D:
            raise engine.LgcnError(f"inbatch_loss: B={B}, d={d} (1 <= B <= "
                                   f"{engine.INBATCH_MAX_B}, 1 <= d <= {engine.INBATCH_MAX_D})")
        for name, t, shape, dt in (("off", off, (B, B), torch.uint8),
                                   ("valid", valid, (B,), torch.uint8),
                                   ("q", q, (B,), torch.float32)):
            if t is not None and (t.shape != shape or t.dtype != dt or t.device != dev or
                                  not t.is_contiguous()):
                raise engine.LgcnError(f"inbatch_loss: {name} must be a contiguous {dt} tensor of "
                                       f"shape {shape} on {dev}")
        work = torch.empty(5 * B, dtype=torch.float32, device=dev)
        mask = torch.empty(B * ((B + 31) // 32), dtype=torch.int32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        grads = torch.empty((2, 2 * B, d), dtype=torch.float32, device=dev)
        args = []
        for t in rows:
            args += [engine._ptr(t), t.stride(0)]
        with torch.cuda.device(dev):
            engine._check(lib.lgcn_inbatch_loss(*args, engine._ptr(off), engine._ptr(valid),
                                                engine._ptr(q), B, d, float(lambda_reg),
                                                float(temperature), engine._ptr(work),
                                                engine._ptr(mask), engine._ptr(loss),
                                                engine._ptr(grads), None, engine._stream(dev)),
                          "lgcn_inbatch_loss")
        ctx.save_for_backward(grads)
        return loss

    @staticmethod
    def backward(ctx, g):
        (grads,) = ctx.saved_tensors
        B = grads.shape[1] // 2
        sg = grads * g
        return (sg[1, :B], sg[1, B:], sg[0, :B], sg[0, B:]) + (None,) * 5


def inbatch_loss_reg(final_user_emb, final_pos_item_emb, initial_user_emb, initial_pos_item_emb,
                     lambda_reg, temperature=1.0, off=None, valid=None, q=None):
    """In-batch softmax loss plus bpr_loss_reg's L2 term over the batch's 2B layer-0 rows: sample
    b's negatives are the positives of the other samples, less the columns off[b] names
    (inbatch_off_mask); inbatch_loss_torch states the expression. On a HIP device loss and all
    four input gradients come from lgcn_inbatch_loss (32 x 32 score tiles recomputed on the exact
    f32 MFMA, no [B, B] logits in memory; include/lgcn.h states its orders of summation), for
    B <= 32768 and d <= 256; on CPU tensors inbatch_loss_torch runs."""
    temperature = _check_temperature(temperature, "inbatch_loss_reg")
    if final_user_emb.device.type != "cuda":
        return inbatch_loss_torch(final_user_emb, final_pos_item_emb, initial_user_emb,
                                  initial_pos_item_emb, lambda_reg, temperature, off, valid, q)
    if off is not None and off.dtype == torch.bool:
        off = off.to(torch.uint8)
    if valid is not None and valid.dtype == torch.bool:
        valid = valid.to(torch.uint8)
    return InBatchLossFunction.apply(final_user_emb, final_pos_item_emb, initial_user_emb,
                                     initial_pos_item_emb, off, valid, q, float(lambda_reg),
                                     temperature)

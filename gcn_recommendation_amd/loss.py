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

"""The LightGCN_Fusion item pre-layer (reference models/lightgcn_fusion.py:45-49)

    fused_item_emb_0 = F.leaky_relu(item_fusion_layer(torch.cat([item_id_emb_0, content], 1)))

on a HIP device as one kernel (lgcn_fusion_prelayer: no concatenation, exact-f32 MFMA GEMM,
bias + leaky_relu in its epilogue). The backward is the same arithmetic autograd would run for
the reference expression: g = dF where F > 0, else slope * dF; d_id = g · W[:, :d];
dW = gᵀ · [id | content]; db = Σ g. BACKWARD selects its route: "kernel" is
lgcn_fusion_prelayer_backward (one pass, g masked in registers, both products on exact-f32 MFMA,
dW and db summed in the fixed order include/lgcn.h documents: the same bits whatever the launch,
the run or the device); "torch" is the expression written out with torch ops (two [I x d]
temporaries and three library GEMMs, whose summation order the BLAS picks), kept for A/B timing
and as the documented fallback. The content table is a buffer (no gradient), as in the reference.

The backward reads the branch from the sign of the saved output, which equals the sign of z only
for slope >= 0 (a negative z times a negative slope is positive). fused_item_embedding therefore
sends slope < 0 to the torch expression, and FusionPreLayer refuses it. The C entry's forward is
valid for any slope.
"""

import torch

from . import engine

SUPPORTED_D = (64, 128)
SUPPORTED_C = (32, 64, 128)
# The route of FusionPreLayer.backward: "kernel" | "torch". DESIGN.md section 8 has the measurement
# the default rests on.
BACKWARD = "kernel"


def supported(d, c_dim):
    return d in SUPPORTED_D and c_dim in SUPPORTED_C


def uses_kernel(device_type, d, c_dim, weight_shape, slope):
    """Whether fused_item_embedding runs the engine kernel for these arguments: a HIP device, a
    supported (d, c_dim), the Linear's weight [d x (d + c_dim)] and slope >= 0 (the backward
    takes its branch from the sign of the output)."""
    return device_type == "cuda" and supported(d, c_dim) and \
        tuple(weight_shape) == (d, d + c_dim) and slope >= 0


class FusionPreLayer(torch.autograd.Function):
    @staticmethod
    def forward(ctx, id_w, content, weight, bias, slope):
        if not slope >= 0:
            raise engine.LgcnError(f"FusionPreLayer: slope {slope} < 0 (the backward reads the "
                                   "branch from the output's sign); use the torch expression")
        lib = engine.load_library()
        n, d = id_w.shape
        c_dim = content.shape[1]
        idc, cc = id_w.detach().contiguous(), content.detach().contiguous()
        wc = weight.detach().contiguous()
        bc = bias.detach().contiguous() if bias is not None else None
        out = torch.empty((n, d), dtype=torch.float32, device=id_w.device)
        with torch.cuda.device(id_w.device):
            engine._check(lib.lgcn_fusion_prelayer(
                engine._ptr(idc), idc.stride(0) if n else d, engine._ptr(cc),
                cc.stride(0) if n else c_dim, n, d, c_dim, engine._ptr(wc), engine._ptr(bc),
                float(slope), engine._ptr(out), d, engine._stream(id_w.device)),
                "lgcn_fusion_prelayer")
        ctx.save_for_backward(idc, cc, wc, out)
        ctx.slope = slope
        ctx.has_bias = bias is not None
        return out

    @staticmethod
    def backward(ctx, g_out):
        idc, cc, wc, out = ctx.saved_tensors
        d = idc.shape[1]
        if BACKWARD not in ("kernel", "torch"):
            raise engine.LgcnError(f"fusion.BACKWARD = {BACKWARD!r}: expected 'kernel' or 'torch'")
        if BACKWARD == "kernel" and out.is_cuda:
            return _backward_kernel(ctx, idc, cc, wc, out, g_out)
        g = torch.where(out > 0, g_out, g_out * ctx.slope)
        d_id = g @ wc[:, :d] if ctx.needs_input_grad[0] else None
        d_w = None
        if ctx.needs_input_grad[2]:
            d_w = torch.cat([g.t() @ idc, g.t() @ cc], 1)
        d_b = g.sum(0) if ctx.has_bias and ctx.needs_input_grad[3] else None
        return d_id, None, d_w, d_b, None


def _backward_kernel(ctx, idc, cc, wc, out, g_out):
    """lgcn_fusion_prelayer_backward; each output is requested only when autograd needs it."""
    lib = engine.load_library()
    n, d = idc.shape
    c_dim = cc.shape[1]
    dev = out.device
    want_id, want_w = ctx.needs_input_grad[0], ctx.needs_input_grad[2]
    want_b = ctx.has_bias and ctx.needs_input_grad[3]
    d_id = torch.empty((n, d), dtype=torch.float32, device=dev) if want_id else None
    if n == 0:  # nothing to sum: the call would leave d_w and d_b unwritten
        d_w = torch.zeros((d, d + c_dim), dtype=torch.float32, device=dev) if want_w else None
        d_b = torch.zeros(d, dtype=torch.float32, device=dev) if want_b else None
        return d_id, None, d_w, d_b, None
    d_w = torch.empty((d, d + c_dim), dtype=torch.float32, device=dev) if want_w else None
    d_b = torch.empty(d, dtype=torch.float32, device=dev) if want_b else None
    gc = g_out.contiguous()
    scratch, nbytes = None, 0
    if want_w or want_b:
        nbytes = lib.lgcn_fusion_prelayer_backward_scratch_bytes(n, d, c_dim)
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        engine._check(lib.lgcn_fusion_prelayer_backward(
            engine._ptr(out), d, engine._ptr(gc), d, engine._ptr(idc), d, engine._ptr(cc), c_dim,
            n, d, c_dim, engine._ptr(wc),
            float(ctx.slope), engine._ptr(d_id), d, engine._ptr(d_w), engine._ptr(d_b),
            engine._ptr(scratch), nbytes, engine._stream(dev)),
            "lgcn_fusion_prelayer_backward")
    return d_id, None, d_w, d_b, None


def fused_item_embedding(id_w, content, linear, slope=0.01):
    """leaky_relu(linear(cat([id_w, content], 1))) — the engine kernel on a HIP device for the
    supported shapes and slope >= 0, the reference's torch ops otherwise (CPU tensors, other
    dims, a negative slope)."""
    if uses_kernel(id_w.device.type, id_w.shape[1], content.shape[1], linear.weight.shape, slope):
        return FusionPreLayer.apply(id_w, content, linear.weight, linear.bias, slope)
    combined = torch.cat([id_w, content], dim=1)
    return torch.nn.functional.leaky_relu(linear(combined), slope)

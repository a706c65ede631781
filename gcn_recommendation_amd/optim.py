"""Adam inside the engine: main.py's `torch.optim.Adam(model.parameters(), lr)` as one HIP launch
per 16 tensors (lgcn_adam_step, csrc/lgcn_adam.hip) instead of torch's seven foreach passes.

    opt = optim.Adam(model.parameters(), lr=cfg.lr)      # a torch.optim.Adam: same arguments,
    model.bpr_epoch(adj, sampler, opt, cfg.l2_reg)       # same state, same state_dict

After any number of steps the parameters, `exp_avg`, `exp_avg_sq` and `step` are bit for bit what
`torch.optim.Adam` with default arguments leaves on the same HIP device (tests/test_gpu_adam.py),
so a checkpoint moves between the two classes in either direction. A parameter group that the
kernel does not cover (a CPU model, amsgrad, AdamW-style decay, a tensor lr, ...) runs torch's own
`adam()` unchanged: the usual device dispatch, never an error for a configuration torch accepts.
"""
import ctypes

import torch
from torch.optim.adam import adam as _torch_adam
from torch.optim.optimizer import _get_value, _use_grad_for_differentiable

from . import engine

__all__ = ["Adam"]


def _dense_f32(t, device):
    return (t.dtype == torch.float32 and t.layout == torch.strided and t.device == device
            and t.is_contiguous())


class Adam(torch.optim.Adam):
    """`torch.optim.Adam` whose step runs in the engine where it can. State is torch's own
    (`state[p] = {"step": CPU scalar, "exp_avg", "exp_avg_sq"}`, created by torch's `_init_group`);
    `state_dict` / `load_state_dict` are inherited. A group takes the engine path when every
    parameter with a gradient, its gradient and its state are fp32, dense, contiguous and on one
    HIP device, `lr` is a Python number, the betas are floats and `amsgrad`, `maximize`,
    `capturable`, `differentiable`, `decoupled_weight_decay` and `fused` are off and `foreach` is
    not False (a caller who asks for torch's single-tensor or fused arithmetic gets it); any
    other group runs torch's `adam()`."""

    def _engine_group(self, group, params, grads, exp_avgs, exp_avg_sqs, steps):
        """The group takes the engine path: fp32, contiguous, dense, one HIP device, plain Adam."""
        if (group["amsgrad"] or group["maximize"] or group["capturable"]
                or group["differentiable"] or group["decoupled_weight_decay"] or group["fused"]
                or group["foreach"] is False):
            return False
        if isinstance(group["lr"], torch.Tensor) or not isinstance(group["lr"], (int, float)):
            return False
        if not all(isinstance(b, float) for b in group["betas"]):
            return False
        dev = params[0].device
        if dev.type != "cuda" or torch.version.hip is None:
            return False
        return all(_dense_f32(t, dev) for ts in (params, grads, exp_avgs, exp_avg_sqs) for t in ts) \
            and all(s.is_cpu for s in steps)

    def _engine_step(self, group, params, grads, exp_avgs, exp_avg_sqs, steps):
        lib = engine.load_library()
        beta1, beta2 = group["betas"]
        lr = group["lr"]
        # the scalars exactly as _multi_tensor_adam forms them, in double
        torch._foreach_add_(steps, torch.tensor(1.0, device="cpu"), alpha=1.0)
        hyper = engine.AdamHyperT(1 - beta1, beta2, 1 - beta2, group["eps"], group["weight_decay"])
        dev = params[0].device
        with torch.cuda.device(dev):
            stream = engine._stream(dev)
            for lo in range(0, len(params), engine.ADAM_MAX_TENSORS):
                hi = min(lo + engine.ADAM_MAX_TENSORS, len(params))
                table = (engine.AdamTensorT * (hi - lo))()
                for d, i in zip(table, range(lo, hi)):
                    step = _get_value(steps[i])
                    bias_correction1 = 1 - beta1 ** step
                    bias_correction2 = 1 - beta2 ** step
                    d.p, d.g = params[i].data_ptr(), grads[i].data_ptr()
                    d.m, d.v = exp_avgs[i].data_ptr(), exp_avg_sqs[i].data_ptr()
                    d.n = params[i].numel()
                    d.step_size = (lr / bias_correction1) * -1
                    d.bc2_sqrt = bias_correction2 ** 0.5
                engine._check(lib.lgcn_adam_step(table, hi - lo, ctypes.byref(hyper), stream),
                              "lgcn_adam_step")

    @_use_grad_for_differentiable
    def step(self, closure=None):
        self._cuda_graph_capture_health_check()
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            params, grads, exp_avgs, exp_avg_sqs, max_exp_avg_sqs, steps = [], [], [], [], [], []
            beta1, beta2 = group["betas"]
            has_complex = self._init_group(group, params, grads, exp_avgs, exp_avg_sqs,
                                           max_exp_avg_sqs, steps)
            if not params:
                continue
            if self._engine_group(group, params, grads, exp_avgs, exp_avg_sqs, steps):
                self._engine_step(group, params, grads, exp_avgs, exp_avg_sqs, steps)
                continue
            # torch.optim.Adam.step's own call, unchanged
            _torch_adam(params, grads, exp_avgs, exp_avg_sqs, max_exp_avg_sqs, steps,
                        amsgrad=group["amsgrad"], has_complex=has_complex, beta1=beta1,
                        beta2=beta2, lr=group["lr"], weight_decay=group["weight_decay"],
                        eps=group["eps"], maximize=group["maximize"], foreach=group["foreach"],
                        capturable=group["capturable"], differentiable=group["differentiable"],
                        fused=group["fused"], grad_scale=getattr(self, "grad_scale", None),
                        found_inf=getattr(self, "found_inf", None),
                        decoupled_weight_decay=group["decoupled_weight_decay"])
        return loss

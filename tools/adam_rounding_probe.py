"""Which roundings do torch's _foreach kernels make on this device? Each op of _multi_tensor_adam
(torch/optim/adam.py) is run alone on 2^20 random fp32 values and compared, as bit patterns, with
the candidate forms lgcn_adam.hip could take: a fused multiply-add (emulated in fp64: the product
of two fp32 values is exact there, so only a double rounding in ~2^-29 of the elements can
differ), the separate multiply and add (torch's own fp32 ops), a true division or a multiply by
the reciprocal, IEEE sqrt and division (fp64 then one rounding: exact for both). Prints one JSON
line: mismatching elements per candidate (profiles/adam_rounding_probe.log). The bitwise proof is
tests/test_gpu_adam.py; this only says which form to write.

    python tools/adam_rounding_probe.py [device]
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

N = 1 << 20


def f32(x):
    return torch.tensor(x, dtype=torch.float32).double().item()   # ATen's opmath cast of a scalar


def miss(got, cand):
    return int((got.view(torch.int32) != cand.view(torch.int32)).sum().item())


def main():
    dev = torch.device(sys.argv[1] if len(sys.argv) > 1 else "cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1)
    p, g, m = (torch.randn(N, device=dev, generator=gen) for _ in range(3))
    v = torch.rand(N, device=dev, generator=gen) * 1e-2 + 1e-12
    out = {"torch": torch.__version__, "n": N,
           "device": torch.cuda.get_device_name(dev) if dev.type == "cuda" else "cpu"}

    wd = f32(1e-2)
    got = torch._foreach_add([g], [p], alpha=1e-2)[0]
    out["add_alpha"] = {"fma": miss(got, (g.double() + wd * p.double()).float()),
                        "mul_add": miss(got, g + p * 1e-2)}

    for name, w in (("lerp_small_w0.1", 0.1), ("lerp_large_w0.7", 0.7)):
        got = m.clone()
        torch._foreach_lerp_([got], [g], w)
        d, wf = g - m, f32(w)
        if w < 0.5:
            fma = (m.double() + wf * d.double()).float()
            plain = m + d * w
        else:
            omw = (torch.tensor(1.0) - torch.tensor(w)).double().item()
            fma = (g.double() - d.double() * omw).float()
            plain = g - d * torch.tensor(omw, dtype=torch.float32).item()
        out[name] = {"fma": miss(got, fma), "mul_add": miss(got, plain)}

    s = f32(1 - 0.999)
    v2 = v * 0.999
    got = v2.clone()
    torch._foreach_addcmul_([got], [g], [g], 1 - 0.999)
    gg = g * g
    out["addcmul"] = {"fma_of_rounded_product": miss(got, (v2.double() + s * gg.double()).float()),
                      "all_exact_then_round": miss(got, (v2.double() + s * g.double() * g.double())
                                                   .float()),
                      "mul_mul_add": miss(got, v2 + gg * (1 - 0.999)),
                      "fma_of_scaled_g_times_g": miss(got, (v2.double() + (g * (1 - 0.999))
                                                            .double() * g.double()).float()),
                      "scaled_g_mul_add": miss(got, v2 + (g * (1 - 0.999)) * g)}

    got = torch._foreach_sqrt([v])[0]
    out["sqrt"] = {"ieee": miss(got, v.double().sqrt().float())}
    t = got
    b = 0.0316069770620507
    got = t.clone()
    torch._foreach_div_([got], [b])
    bf = f32(b)
    out["div_scalarlist"] = {"ieee_true_division": miss(got, (t.double() / bf).float()),
                             "mul_by_fp32_reciprocal": miss(got, t * (1.0 / torch.tensor(
                                 b, dtype=torch.float32)).item())}
    t = got + 1e-8
    step = f32(-0.01)
    got = p.clone()
    torch._foreach_addcdiv_([got], [m], [t], [-0.01])
    q = (m.double() / t.double()).float()
    out["addcdiv"] = {"fma_of_ieee_quotient": miss(got, (p.double() + step * q.double()).float()),
                      "mul_add_of_ieee_quotient": miss(got, p + q * -0.01),
                      "quotient_differs_from_torch_div": miss(m / t, q)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()

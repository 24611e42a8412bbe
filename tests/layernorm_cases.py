"""fp64 references and derived bounds of the LayerNorm kernels, shared by tests/test_layernorm_forms_gpu.py (whose docstring
derives the bound) and tests/unet_plan_cases.py.  x [rows][C] fp64 holding fp16 values, gamma / beta fp64 holding fp32 values;
the backward takes mean / rstd [rows][1] as given."""
import torch

U, W = 2.0 ** -11, 2.0 ** -24
EPS = 1e-5


def fwd_ref(x, gamma, beta):
    C = x.shape[-1]
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    rstd = (var + EPS) ** -0.5
    y = (x - mean) * rstd * gamma + beta
    e_m = (C + 2) * W * x.abs().mean(-1, keepdim=True)
    e_r = 0.5 * ((C + 6) * W + e_m ** 2 / var) + 2.0 ** -22
    bound = U * y.abs() + 2.0 ** -25 + (x - mean).abs() * rstd * gamma.abs() * (e_r + 3 * W) + e_m * rstd * gamma.abs() + W * y.abs()
    return dict(y=y, bound=bound, mean=mean, rstd=rstd, bound_mean=e_m + W * mean.abs(), bound_rstd=rstd * (e_r + W))


def bwd_ref(x, gy, gamma, mean, rstd, base=None):
    C = x.shape[-1]
    d = gy * gamma
    xh = (x - mean) * rstd
    s1 = d.mean(-1, keepdim=True)
    s2 = (d * xh).mean(-1, keepdim=True)
    dx = rstd * (d - s1 - xh * s2)
    out = dx if base is None else dx + base
    bound = (U * out.abs() + 2.0 ** -25 + 2 * W * out.abs()
             + rstd * ((C + 2) * W * d.abs().mean(-1, keepdim=True) + xh.abs() * (C + 4) * W * (d * xh).abs().mean(-1, keepdim=True)
                       + 6 * W * (d.abs() + s1.abs() + (xh * s2).abs())))
    return out, bound

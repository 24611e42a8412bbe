"""The UNet reverse plan on the device, op by op (tests/unet_plan_cases.py): every case's grad plan runs eagerly on poisoned
buffers with a synchronize between ops; every forward output, saved statistic, gradient and scratch result is compared with
its fp64 statement at the device's own inputs, inside the bound the kernel family's conformance module derives.

Per case: the worst forward and the worst backward ratio (error / bound) are gated at 1.0 and name their op; integrity (an op
changes its declared outputs, gradient outputs and scratch only) and completeness hold; the whole reverse plan run twice gives
bit-identical latent gradients.

End to end: the device's latent gradient against the fp64 VJP chain evaluated at the device's own forward activations, as
rel-L2.  The yardstick is the reference alone: E_store, the rel-L2 between that chain and the same chain with every gradient
rounded to fp16 where the plan stores it.  The gate is 8 x E_store: the margin covers the fp16 roundings inside the attention
backward (P, dS) and the fp32 statistics of the norm backwards, which E_store does not contain.

Measured on an MI355X (ops; worst forward ratio and its op; worst backward ratio and its op; E_store; device rel-L2 / E_store):
  A  221  0.9970 GEGLU forward (op 76)        0.9994 residual add behind down_blocks.3.resnets.0.conv2   1.557e-3  1.007
  B  301  0.9970 GEGLU forward (op 200)       0.9994 residual add behind down_blocks.3.resnets.0.conv2   1.655e-3  1.008
  C  221  0.9951 GEGLU forward (op 204)       0.9994 residual add behind down_blocks.2.resnets.1.conv2   1.512e-3  1.043
  D  141  0.9946 GEGLU forward (op 57)        0.9971 GEGLU backward (op 97)                              1.114e-3  1.038
  E   14  0.9925 norm1 of the first resnet    0.9972 LayerNorm backward, norm1 of the first block        5.968e-4  1.101
The ratios sit just under 1 because the half-ulp fp16 rounding of the stored value is the leading term of every bound.  No op
was outside its bound, integrity and completeness held: the walker found no defect in the reverse plan."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import unet_plan_cases as U  # noqa: E402
from conftest import gate  # noqa: E402


@pytest.mark.parametrize("case", sorted(U.CASES))
def test_reverse_plan_op_by_op(dev, case):
    s = U.Setup(case, dev)
    w = U.Walker(s)
    gl = w.run().clone()
    f, fname = w.worst("fwd")
    b, bname = w.worst("bwd")
    print(f"[unet plan {case}] {len(s.plan.ops)} ops, {sum(op.bwd is not None for op in s.plan.ops)} with a backward")
    gate(f"case {case}: worst forward error / bound, at {fname}", f, 1.0)
    gate(f"case {case}: worst backward error / bound, at {bname}", b, 1.0)
    assert w.integrity == [], w.integrity[:8]
    assert s.graph.completeness() == []
    assert w.x0_grad_stable, "the reverse plan run whole left another gradient of conv_in's output than the stepped run"
    again = s.plan.backward(U.GRAD_SCALE)
    torch.cuda.synchronize()
    assert torch.equal(U._bits(again), U._bits(gl)), "the reverse plan run twice: the latent gradients differ in their bits"

    # ---- end to end, against the chain at the device's own forward activations
    ch = U.Chain(s, pure=False)
    ch.adopt(s.plan)
    cot = {k: v.to(dev) for k, v in s.cot.items()}
    ref, _ = ch.backward(cot, U.GRAD_SCALE)
    stored, _ = ch.backward(cot, U.GRAD_SCALE, round_store=True)
    e_store = U.rel_l2(stored, ref)
    e_dev = U.rel_l2(gl, ref)
    print(f"[unet plan {case}] E_store {e_store:.4e}, device rel-L2 {e_dev:.4e}")
    gate(f"case {case}: device latent gradient vs the fp64 chain, rel-L2 / E_store", e_dev / e_store, 8.0)


def test_residual_gradient_alias_changes_no_bit(dev, monkeypatch):
    """LGD_RES_GRAD_ALIAS=0 gives the first writer of a pass-through gradient a buffer of its own (a copy): case A on a fresh
    engine with it must give the latent gradient of the default, bit for bit."""
    outs = []
    for alias in ("1", "0"):
        monkeypatch.setenv("LGD_RES_GRAD_ALIAS", alias)
        s = U.Setup("A", dev)
        aliased = sum(op.passthrough is not None and op.passthrough[0].g.data_ptr() == op.passthrough[1].g.data_ptr()
                      for op in s.plan.ops if op.bwd is not None)
        assert (aliased > 0) == (alias == "1")
        s.eng.poison_arena()
        s.plan.forward(s.lat.to(dev))
        for k, t in s.plan.gmaps.items():
            t.copy_(s.cot[k])
        outs.append(s.plan.backward(U.GRAD_SCALE).clone())
        torch.cuda.synchronize()
    assert bool(torch.isfinite(outs[0]).all())
    assert torch.equal(U._bits(outs[0]), U._bits(outs[1]))

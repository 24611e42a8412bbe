"""The UNet inference plan on the device, op by op (tests/unet_fwd_plan_cases.py): every case's no-grad plan runs eagerly on
poisoned buffers with a synchronize between ops; every output, the statistics of every ln_linear and every captured map are
compared with their fp64 statement at the device's own inputs, inside the bound the kernel family's conformance module derives.

Per case: the worst error / bound is gated at 1.0 and names its op; integrity holds for every op (an op changes its declared
outputs, side outputs and scratch only); after a HALF op rows >= M/2 of its output (and of an ln_linear's statistics) still
hold the poison, after a DUP op the halves are bit-identical; the plan run whole twice gives the bits of the stepped run.

End to end: eps_out and every saved map against the fp64 chain at exact weights and constants, as rel-L2.  The yardstick is the
reference alone: E_store, the rel-L2 between that chain and the same chain with the weights rounded as the store rounds them
(the folded ones included), the constants rounded to their storage types and every activation rounded to fp16 where the plan
stores it.  The gate is 8 x E_store, the factor of test_unet_plan_gpu for the same reason: E_store contains neither the fp16 P
inside attention nor the fp32 statistics of the norms.

Hot rows (F and H): rows with |mean| / std >= 32 enter the three ln_linear ops of the first transformer block (asserted on the
device's own rows); the device stays inside the same bound; the amplification (bound of the fold / bound of the two-op form at
the same rows) is printed for every ln_linear: a recorded figure, not a gate.

Measured on an MI355X (ops; ops in pair mode; worst error / bound and its op; E_store of eps_out; device rel-L2 / E_store,
worst over eps_out and the maps, and where):
  F  287  9  0.9938 GroupNorm up_blocks.3.resnets.0.norm1 (op 237)   2.226e-3  1.039 map (up, 1, 0, 0)
  G  383  8  0.9951 GroupNorm up_blocks.3.resnets.0.norm1 (op 315)   2.222e-3  1.129 map (up, 1, 2, 0)
  H  287  0  0.9945 GroupNorm conv_norm_out (op 285)                 2.274e-3  1.027 eps_out
  I  320  0  0.9939 GroupNorm up_blocks.3.resnets.1.norm2 (op 310)   2.309e-3  1.031 eps_out
  J  335  0  0.9943 GroupNorm up_blocks.3.resnets.0.norm2 (op 278)   2.199e-3  1.019 eps_out
  K  383  8  0.9943 GroupNorm up_blocks.3.resnets.2.norm2 (op 361)   2.356e-3  1.020 eps_out
The ratios sit just under 1 because the half-ulp fp16 rounding of the stored value leads every bound.  Integrity, the HALF /
DUP properties and both repeatability checks held in every case.
One finding, in the statement and not in a kernel: case H's up_blocks.3.attentions.0 ff.net.0.proj (op 250) measured 1.4147
against the first GEGLU-epilogue bound, which took the gelu_f of the geglu_fwd kernel for the epilogue's gelu2_f (a polynomial
Phi, 1.2e-5 of gelu: above half an ulp of outputs below 0.02).  With the statement on gelu2_f (unet_fwd_plan_cases) that op
measures 0.89; the host emulation shows the same 1.414 -> 0.87 (test_unet_fwd_plan_cpu).
The three largest ln_linear amplifications (bound of the fold / bound of the two-op form at the same rows), hot rows, all of
down_blocks.0.attentions.0.transformer_blocks.0 (every other ln_linear: 1.01 .. 1.08):
  F  ff.net.0.proj 57.3 (|mean| / std >= 90.5, error / bound 0.056)   attn1.qkv 32.5 (94.5, 0.118)   attn2.to_q 28.3 (97.0, 0.120)
  H  ff.net.0.proj 57.6 (85.3, 0.070)                                  attn1.qkv 32.7 (90.0, 0.137)   attn2.to_q 28.4 (88.8, 0.123)
"""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import unet_fwd_plan_cases as Fw  # noqa: E402
import unet_plan_cases as U  # noqa: E402
from conftest import gate  # noqa: E402


@pytest.mark.parametrize("case", sorted(Fw.CASES))
def test_forward_plan_op_by_op(dev, case):
    s = Fw.FSetup(case, dev)
    w = Fw.FWalker(s)
    eps = w.run().clone()
    maps = {k: t.clone() for k, t in s.plan.maps.items()}
    worst, name = w.worst()
    print(f"[unet fwd plan {case}] {len(s.plan.ops)} ops, {s.plan.pair_ops} in pair mode")
    gate(f"case {case}: worst forward error / bound, at {name}", worst, 1.0)
    assert w.integrity == [], w.integrity[:8]
    assert set(maps) == set(s.keys)

    # ---- run whole, twice: the bits of the stepped run
    for _ in range(2):
        s.plan.forward()
        torch.cuda.synchronize()
        assert torch.equal(U._bits(s.plan.eps_out), U._bits(eps)), "the plan run whole: eps_out differs from the stepped run in its bits"
        for k, t in maps.items():
            assert torch.equal(U._bits(s.plan.maps[k]), U._bits(t)), f"the plan run whole: map {k} differs from the stepped run in its bits"

    # ---- end to end against the fp64 chain at exact weights and constants
    lat = s.lat.to(dev)
    ref_eps, ref_maps = Fw.FChain(s, pure=True, dev=dev).forward(lat)
    st_eps, st_maps = Fw.FChain(s, pure=False, consts="rounded", dev=dev).forward(lat, round_store=True)
    rows = [("eps_out", U.rel_l2(st_eps, ref_eps), U.rel_l2(eps, ref_eps))]
    rows += [(f"map {k}", U.rel_l2(st_maps[k], ref_maps[k]), U.rel_l2(maps[k], ref_maps[k])) for k in s.keys]
    for n, e_store, e_dev in rows:
        print(f"[unet fwd plan {case}] {n}: E_store {e_store:.4e}, device rel-L2 {e_dev:.4e}, ratio {e_dev / e_store:.3f}")
    n, e_store, e_dev = max(rows, key=lambda r: r[2] / r[1])
    gate(f"case {case}: device vs the fp64 chain, rel-L2 / E_store, worst at {n}", e_dev / e_store, 8.0)


@pytest.mark.parametrize("case", Fw.HOT_CASES)
def test_hot_rows_stay_inside_the_bound(dev, case):
    s = Fw.FSetup(case, dev, hot=True)
    w = Fw.FWalker(s)
    w.run(amplify=True)
    hot = Fw.hot_ops(s)
    assert len(hot) == 3
    for i in hot:
        assert w.hot[i] >= Fw.HOT_RATIO, (s.graph.label(i), w.hot[i])
    low = [a for i, a in w.amplification.items() if i not in hot]
    print(f"[unet fwd plan {case} hot] {len(low)} other ln_linear ops: amplification {min(low):.2f} .. {max(low):.2f}")
    for i in sorted(hot, key=w.amplification.get, reverse=True):
        print(f"[unet fwd plan {case} hot] {s.graph.label(i)}: min |mean| / std {w.hot[i]:.1f}, error / bound {w.fwd_ratio[i][0]:.4f}, "
              f"amplification {w.amplification[i]:.2f}")
    worst, name = w.worst()
    gate(f"case {case} hot rows: worst forward error / bound, at {name}", worst, 1.0)
    gate(f"case {case} hot rows: worst error / bound over the three hot ln_linear ops", max(w.fwd_ratio[i][0] for i in hot), 1.0)
    assert w.integrity == [], w.integrity[:8]

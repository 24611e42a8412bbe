"""The state-reuse suite's own tools, without a GPU: the poison walker on a stub object graph, and every call description
of tests/test_state_reuse_gpu.py against LMDSampler._refuse_undefined (a sequence must not contain a call the sampler
refuses: the GPU test would then compare two exceptions, not two runs)."""
import os
import sys
from collections import OrderedDict

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lgd_amd  # noqa: E402,F401
from lgd_amd.loop import LoopState, StateCache  # noqa: E402
from lgd_amd.sampler import LMDSampler  # noqa: E402
from lgd_amd.scheduler import DDIM, MULTISTEP  # noqa: E402
import state_reuse_cases as sr  # noqa: E402


class HipGraph:                                    # by name, as the walker knows captured graphs
    def __init__(self, t):
        self.held = t


class _Weights:
    def __init__(self):
        self.h = {"conv_in.w": torch.ones(4, dtype=torch.float16)}
        self.f = {"conv_in.b": torch.ones(4)}


class _Engine:
    def __init__(self):
        self.w = _Weights()
        self.dyn = torch.zeros(4, dtype=torch.int32)
        self.step_idx = self.dyn[:1]
        self.text_kv = {"mid": torch.ones((2, 3), dtype=torch.float16)}
        self._arena = [torch.zeros(16, dtype=torch.uint8)]
        self.plans = OrderedDict(p=_Plan(self))


class _Plan:
    def __init__(self, eng):
        self.eng = eng                                                 # a cycle, as unet.Plan has
        self.weight_view = eng.w.f["conv_in.b"][:2]                    # a view of a packed weight
        self.buffers = [torch.ones(3), (torch.ones(2), torch.ones(2, dtype=torch.float16))]


class _Sampler:
    def __init__(self):
        self.eng = _Engine()
        self._states = StateCache(2)
        st = self._states.get((1, 4, 8), lambda: LoopState(torch.ones((1, 4, 8, 8)), 5))
        st.hist = torch.ones((6, 1, 4, 8, 8))
        st.step_kernel(DDIM)
        st.step_kernel(MULTISTEP)
        st.graphs["main"] = HipGraph(torch.ones(7))
        st.picks = torch.ones(3, dtype=torch.int32)
        self.alias = st.hist                                           # the same tensor object by a second path
        self.nested = {"a": [torch.ones(1), {"b": torch.ones(1)}], "n": None, "s": "text", "f": lambda: None}


def test_walker_reaches_every_tensor_once_and_skips_the_excluded():
    sm = _Sampler()
    st = sm._states.states[(1, 4, 8)]
    found = sr.walk_tensors(sm, exclude=sr.excluded_of(sm))
    ids = [id(t) for _, t in found]
    assert len(ids) == len(set(ids))                                   # each tensor once, `alias` included
    want = [sm.eng.dyn, sm.eng.step_idx, sm.eng.text_kv["mid"], sm.eng._arena[0], st.lat, st.hist, st.picks,
            st.steps[DDIM].tab, st.steps[MULTISTEP].tab, st.steps[MULTISTEP].x0_prev,
            sm.nested["a"][0], sm.nested["a"][1]["b"], *sm.eng.plans["p"].buffers[:1], *sm.eng.plans["p"].buffers[1]]
    assert {id(t) for t in want} == set(ids)
    # not reached: the packed weights, a view of one, what only a captured graph holds
    for t in (sm.eng.w.h["conv_in.w"], sm.eng.w.f["conv_in.b"], sm.eng.plans["p"].weight_view, st.graphs["main"].held):
        assert id(t) not in ids
    # the paths name how a tensor was reached
    paths = dict((id(t), p) for p, t in found)
    assert paths[id(st.steps[MULTISTEP].x0_prev)].endswith(f".steps[{MULTISTEP!r}].x0_prev")


def test_poison_writes_nan_patterns_and_the_stale_frozen_count_only():
    sm = _Sampler()
    st = sm._states.states[(1, 4, 8)]
    done = sr.poison(sm, any_device=True)
    for t in (st.lat, st.hist, st.steps[DDIM].tab, st.steps[MULTISTEP].x0_prev, sm.eng.text_kv["mid"],
              sm.nested["a"][1]["b"], sm.eng.plans["p"].buffers[1][1]):
        assert bool(torch.isnan(t).all())
    assert bool((st.hist.view(torch.int32) == -1).all())               # the all-ones byte pattern
    assert sm.eng.dyn.tolist() == [0, sr.STALE_FROZEN_STEPS, 0, 0]
    assert st.picks.tolist() == [1, 1, 1] and int(sm.eng._arena[0].sum()) == 0      # integer tensors stay
    for t in (sm.eng.w.h["conv_in.w"], sm.eng.w.f["conv_in.b"], st.graphs["main"].held):
        assert bool((t == 1).all())
    assert "eng.dyn[1]" in done and len(done) == len(set(done))
    # without any_device only device tensors are written: nothing of this host-side stub
    sm2 = _Sampler()
    assert sr.poison(sm2) == ["eng.dyn[1]"]
    assert bool((sm2._states.states[(1, 4, 8)].hist == 1).all())


SAMPLER_CALLS = [(name, i, c) for name, seq in (("A", sr.SEQ_A), ("B", sr.SEQ_B), ("C", sr.SEQ_C), ("D", sr.SEQ_D))
                 for i, c in enumerate(seq)]


@pytest.mark.parametrize("name,i,call", SAMPLER_CALLS, ids=[f"{n}{i + 1}" for n, i, _ in SAMPLER_CALLS])
def test_every_sampler_call_of_the_sequences_is_accepted(name, i, call):
    kind, args = sr.refusal_arguments(call)
    LMDSampler._refuse_undefined(kind, **args)                         # raises if the sampler would refuse the call


def test_the_refusal_check_is_not_blind():
    """The same path refuses what the sampler refuses: LMS from a later step, PLMS with frozen steps, a guided inversion."""
    lms = dict(sr.SEQ_A[4], kw=dict(first_step=1))
    plms = dict(sr.SEQ_A[0], kw=dict(frozen_steps=2))
    inv = dict(sr.SEQ_A[8], kw=dict(fast_after_steps=2))
    for call in (lms, plms, inv):
        kind, args = sr.refusal_arguments(call)
        with pytest.raises(RuntimeError):
            LMDSampler._refuse_undefined(kind, **args)


def test_the_sequences_are_what_the_suite_says():
    assert [c["sched"] for c in sr.SEQ_A] == ["pndm", "ddim", "ddim", "dpm", "lms", "euler", "ddim", "ddim", "ddim", "ddim"]
    assert [c["steps"] for c in sr.SEQ_A] == [6, 4, 3, 5, 5, 5, 4, 4, 4, 7]
    assert sr.SEQ_A[sr.PARTIAL_A]["kw"] == dict(first_step=2, n_steps=1)
    assert all(c["jobs"] == 1 and c.get("L", 32) == 32 for c in sr.SEQ_A)                 # one (1, C, 32) state
    assert [c["steps"] for c in sr.SEQ_C] == [60, 4, 60] and LMDSampler.STATE_MIN_STEPS < 60
    assert sorted({(c["jobs"], c["L"], bool(c["guided"])) for c in sr.SEQ_D}) == [(1, 32, False), (1, 32, True),
                                                                                   (2, 16, False), (2, 32, True)]
    e0, e1 = (c["kw"] for c in sr.SEQ_E)
    assert e0["num_inference_steps"] - e0["first_index"] == e1["num_inference_steps"] - e1["first_index"] == 4
    for path, calls in sr.SEQ_F.items():
        assert len({c["width"] for c in calls}) == 1 and calls[1]["kw"]["first_step"] > 0
        assert calls[1]["picks_rows"] < calls[0]["picks_rows"]
        a, b = (sr.md_inputs(c) for c in calls)
        assert not torch.equal(a["masks"], b["masks"]) and b["noise"] is not None
        assert bool((a["masks"].sum(0) == 1).all())

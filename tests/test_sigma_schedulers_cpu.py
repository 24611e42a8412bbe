"""The sigma-space samplers (lgd_amd.scheduler.EulerDiscreteScheduler, LMSDiscreteScheduler) where there is no GPU: their
table forms against the stateful restatements of the diffusers 0.18.0 classes (tests/sigma_sched_restate.py) in fp64, the
closed-form LMS coefficients against the class's quad call, the sigmas of the reference's beta schedule, the fractional
timesteps on their way to the time embedding, the drop-in's scheduler resolver and the sampler's refusals."""
import os
import sys

import numpy as np
import pytest
import torch

import lgd_amd  # noqa: F401
from lgd_amd import _lib
from lgd_amd.sampler import LMDSampler
from lgd_amd.scheduler import (C_IN_GCOL, DDIM, LMS, MULTISTEP, DDIMScheduler, DPMSolverMultistepScheduler,
                               EulerDiscreteScheduler, LMSDiscreteScheduler)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from sigma_sched_restate import EulerRestate, LMSRestate, sd_config  # noqa: E402

F64 = torch.float64
STEPS = (1, 2, 5, 20, 50)
SPACINGS = ("linspace", "leading", "trailing")
PREDICTIONS = ("epsilon", "v_prediction")
REL = 1e-9                                                   # the issue's bound: fp64 on both sides, the same fp32 sigmas


def _pair(ours_cls, restate_cls, spacing, prediction, n):
    cfg = sd_config(prediction, timestep_spacing=spacing)
    ours = ours_cls.from_config(cfg)
    ref = restate_cls(dtype=F64, **cfg)
    ours.set_timesteps(n)
    ref.set_timesteps(n)
    return ours, ref


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def _run(ours, ref, step_ours):
    """Both samplers from the same start through the same random model outputs -> worst relative difference of any step."""
    g = torch.Generator().manual_seed(len(ref.timesteps))
    x = torch.randn(2, 4, 3, 3, generator=g, dtype=F64) * float(ref.init_noise_sigma)
    xr, worst = x.clone(), 0.0
    for i, t in enumerate(ref.timesteps):
        m = torch.randn(x.shape, generator=g, dtype=F64)
        assert _rel(ours.scale_model_input(x, t), ref.scale_model_input(xr, t)) <= REL
        x, xr = step_ours(m, i, x), ref.step(m, t, xr).prev_sample
        worst = max(worst, _rel(x, xr))
    return worst


@pytest.mark.parametrize("prediction", PREDICTIONS)
@pytest.mark.parametrize("spacing", SPACINGS)
def test_euler_rows_against_the_restatement(spacing, prediction):
    worst = 0.0
    for n in STEPS:
        ours, ref = _pair(EulerDiscreteScheduler, EulerRestate, spacing, prediction, n)
        assert torch.equal(ours.sigmas, ref.sigmas.float()) and ours.timesteps.tolist() == ref.timesteps.tolist()
        rows = ours.multistep_rows()

        def by_row(m, i, x):
            c0, c1, A, B, C, c_in = rows[i]
            assert C == 0.0
            return A * x + B * (c0 * x + c1 * m)
        worst = max(worst, _run(ours, ref, by_row), _run(ours, ref, lambda m, i, x: ours.step_host(m, i, x)))
        tab = ours.multistep_table(7.5, "cpu")
        assert tab.shape == (n, 8) and torch.equal(tab[:, 5], torch.full((n,), 7.5))
        assert torch.allclose(tab[:, EulerDiscreteScheduler.C_IN_COL].double(), 1 / (ours.sigmas[:-1].double() ** 2 + 1).sqrt(), rtol=1e-6)
    print(f"[euler {spacing} {prediction}] worst relative step difference {worst:.3e}")
    assert worst <= REL


@pytest.mark.parametrize("prediction", PREDICTIONS)
@pytest.mark.parametrize("spacing", SPACINGS)
def test_lms_rows_against_the_restatement(spacing, prediction):
    worst = worst_c = 0.0
    for n in STEPS:
        ours, ref = _pair(LMSDiscreteScheduler, LMSRestate, spacing, prediction, n)
        assert torch.equal(ours.sigmas, ref.sigmas.float())
        state = ours.host_state(torch.zeros(2, 4, 3, 3, dtype=F64))
        for r in state["ring"]:
            r.fill_(float("nan"))                            # nothing the run has not written is read
        worst = max(worst, _run(ours, ref, lambda m, i, x: ours.step_host(m, i, x, state)))
        for i in range(n):                                   # the closed form against the class's quad call
            order = min(i + 1, 4)
            for k, c in enumerate(ours.lms_coefficients(i)):
                q = ref.get_lms_coefficient(order, i, k)
                worst_c = max(worst_c, abs(c - q) / abs(q))
        tab = ours.lms_table(7.5, "cpu")
        assert tab.shape == (n, 16) and tab[:, 8].tolist() == [float(i % 4) for i in range(n)]
        assert not bool(tab[:, 9:].any()) and torch.equal(tab[:, 7], torch.full((n,), 7.5))
        for i in range(min(n, 3)):                           # a slot the order does not reach has weight 0
            assert tab[i, 3 + i + 1:7].tolist() == [0.0] * (3 - i)
    print(f"[lms {spacing} {prediction}] worst relative step difference {worst:.3e}, coefficient against quad {worst_c:.3e}")
    assert worst <= REL and worst_c <= REL


def test_lms_of_order_one_is_euler():
    for spacing in SPACINGS:
        cfg = sd_config(timestep_spacing=spacing)
        eu, lm = EulerDiscreteScheduler.from_config(cfg), LMSDiscreteScheduler.from_config(cfg)
        eu.set_timesteps(20)
        lm.set_timesteps(20)
        g = torch.Generator().manual_seed(3)
        x = torch.randn(1, 4, 4, 4, generator=g, dtype=F64) * eu.init_noise_sigma
        state = lm.host_state(x)
        for i in range(20):
            m = torch.randn(x.shape, generator=g, dtype=F64)
            a, b = eu.step_host(m, i, x), lm.step_host(m, i, x, state, order=1)
            assert _rel(b, a) <= 1e-12
            x = a
        assert lm.lms_coefficients(7, order=1) == [float(lm.sigmas[8]) - float(lm.sigmas[7])]


def test_last_euler_step_returns_x0():
    for prediction in PREDICTIONS:
        eu = EulerDiscreteScheduler.from_config(sd_config(prediction))
        eu.set_timesteps(6)
        c0, c1, A, B, C, _ = eu.multistep_rows()[-1]
        assert (A, B, C) == (0.0, 1.0, 0.0)
        g = torch.Generator().manual_seed(1)
        x, m = torch.randn(8, generator=g, dtype=F64), torch.randn(8, generator=g, dtype=F64)
        assert torch.equal(A * x + B * (c0 * x + c1 * m), c0 * x + c1 * m)
        assert _rel(eu.step_host(m, 5, x), c0 * x + c1 * m) <= 1e-12


@pytest.mark.parametrize("cls", [EulerDiscreteScheduler, LMSDiscreteScheduler])
def test_sigma_max_of_the_reference_beta_schedule(cls):
    """Computed from the reference's betas (scaled_linear 0.00085 .. 0.012, 1000 steps)."""
    for n in (5, 20, 50):
        for spacing in ("linspace", "trailing"):
            s = cls.from_config(sd_config(timestep_spacing=spacing))
            s.set_timesteps(n)
            assert round(float(s.sigmas.max()), 4) == 14.6146, (spacing, n)
    for n, want in ((5, 5.1344), (20, 11.0283), (50, 13.1204)):
        s = cls.from_config(sd_config(timestep_spacing="leading"))
        s.set_timesteps(n)
        assert round(float(s.sigmas.max()), 4) == want, n


@pytest.mark.parametrize("cls,restate", [(EulerDiscreteScheduler, EulerRestate), (LMSDiscreteScheduler, LMSRestate)])
def test_init_noise_sigma_before_and_after_set_timesteps(cls, restate):
    for spacing in SPACINGS:
        cfg = sd_config(timestep_spacing=spacing)
        s, r = cls.from_config(cfg), restate(**cfg)
        assert s.sigmas.shape == (1001,) and float(s.sigmas[-1]) == 0.0 and torch.equal(s.sigmas, r.sigmas)
        assert s.init_noise_sigma == float(r.init_noise_sigma)                   # the training sigmas
        top = float(s.sigmas.max())
        assert s.init_noise_sigma == (top if spacing != "leading" else float((s.sigmas.max() ** 2 + 1) ** 0.5))
        s.set_timesteps(20)
        r.set_timesteps(20)
        assert s.init_noise_sigma == float(r.init_noise_sigma) and len(s.sigmas) == 21
        if spacing == "leading":
            assert s.init_noise_sigma < (top * top + 1) ** 0.5                   # it follows the current sigmas


def test_the_bare_euler_constructor_is_the_refiner():
    s = EulerDiscreteScheduler()
    c = s.config
    assert (c.timestep_spacing, c.steps_offset, c.prediction_type, c.beta_schedule) == ("leading", 1, "epsilon", "scaled_linear")
    s.set_timesteps(50)
    assert s.timesteps.dtype == torch.float32 and s.timesteps[0] == 981 and s.step_kind == MULTISTEP
    d = EulerDiscreteScheduler.from_config({})                                   # the diffusers class defaults
    assert (d.config.timestep_spacing, d.config.steps_offset, d.config.beta_schedule, d.config.beta_start, d.config.beta_end) == \
        ("linspace", 0, "linear", 0.0001, 0.02)
    for bad in (dict(use_karras_sigmas=True), dict(interpolation_type="log_linear")):
        with pytest.raises(NotImplementedError, match="karras|interpolation"):
            EulerDiscreteScheduler.from_config(sd_config(**bad))
    assert LMSDiscreteScheduler().step_kind == LMS and LMSDiscreteScheduler().config.timestep_spacing == "linspace"
    assert EulerDiscreteScheduler.scales_model_input and LMSDiscreteScheduler.scales_model_input
    assert not getattr(DDIMScheduler, "scales_model_input", False)
    assert EulerDiscreteScheduler.stateless_rows and not LMSDiscreteScheduler.stateless_rows


@pytest.mark.parametrize("cls", [EulerDiscreteScheduler, LMSDiscreteScheduler])
def test_guidance_step_table(cls):
    s = cls.from_config(sd_config())
    s.set_timesteps(6)
    tab = s.guidance_step_table("cpu")
    sig = s.sigmas[:-1].double()
    c_in = 1 / (sig ** 2 + 1).sqrt()
    assert tab.shape == (6, 4) and C_IN_GCOL == 1 and not bool(tab[:, 2:].any())
    assert torch.allclose(tab[:, 0].double(), sig ** 2 * c_in, rtol=1e-6) and torch.allclose(tab[:, 1].double(), c_in, rtol=1e-6)
    assert torch.equal(s.guidance_step_table("cpu", timesteps=s.timesteps[2:4]), tab[2:4])


def test_fractional_timesteps_reach_prepare_timesteps():
    for n in (5, 20, 50):
        s = EulerDiscreteScheduler.from_config(sd_config())
        s.set_timesteps(n)
        ts = LMDSampler._timestep_list(s.timesteps)
        assert ts == np.linspace(0, 999, n)[::-1].tolist() and any(t != int(t) for t in ts)
        assert all(isinstance(t, float) for t in ts)
    for sch in (DDIMScheduler(), DPMSolverMultistepScheduler()):                  # integer schedules: the same fp32 values
        sch.set_timesteps(50)
        ints = torch.as_tensor([int(t) for t in sch.timesteps], dtype=torch.float32)
        assert torch.equal(torch.as_tensor(LMDSampler._timestep_list(sch.timesteps), dtype=torch.float32), ints)


# ---- the sampler's refusals
def test_fast_and_partial_schedules():
    off = dict(fast=False, partial=False, conditioned=False)
    for kind, stateless in ((MULTISTEP, True), (LMS, False)):
        LMDSampler._refuse_undefined(kind, sigma_space=True, stateless=stateless, **dict(off, conditioned=True))   # guided runs
        with pytest.raises(RuntimeError, match="fast schedule"):
            LMDSampler._refuse_undefined(kind, sigma_space=True, stateless=stateless, **dict(off, fast=True))
    LMDSampler._refuse_undefined(MULTISTEP, sigma_space=True, stateless=True, **dict(off, partial=True))   # Euler: no state
    with pytest.raises(RuntimeError, match="LMSDiscreteScheduler"):
        LMDSampler._refuse_undefined(LMS, sigma_space=True, **dict(off, partial=True))
    with pytest.raises(RuntimeError, match="multistep"):                          # DPM-Solver++ as before
        LMDSampler._refuse_undefined(MULTISTEP, **dict(off, partial=True))
    LMDSampler._refuse_undefined(DDIM, **dict(off, fast=True, partial=True, conditioned=True))
    s = LMSDiscreteScheduler()
    s.set_timesteps(6)
    with pytest.raises(RuntimeError, match="whole schedule"):
        s.lms_rows(s.timesteps[1:])
    with pytest.raises(RuntimeError, match="fast schedule"):
        s.fast_schedule(s.timesteps, 2)


# ---- the drop-in's resolver
@pytest.fixture
def models():
    sys.path.insert(0, os.path.join(ROOT, "llm-groundeddiffusion_amd", "dropin"))
    import models
    return models


def test_resolver_accepts(models):
    r = models.resolve_scheduler
    cfg = sd_config()
    assert type(r()) is DDIMScheduler and type(r(None, True)) is DPMSolverMultistepScheduler
    assert type(r("DDIMScheduler", scheduler_config=cfg)) is DDIMScheduler
    assert type(r("DPMSolverMultistepScheduler")) is DPMSolverMultistepScheduler
    for name, cls in (("EulerDiscreteScheduler", EulerDiscreteScheduler), ("LMSDiscreteScheduler", LMSDiscreteScheduler)):
        for handle in (name, type(name, (), {})):                                  # the name, or a class of that name
            s = r(handle, scheduler_config=cfg)
            assert type(s) is cls and s.config.timestep_spacing == "linspace" and s.config.beta_schedule == "scaled_linear"
            assert (s.config.beta_start, s.config.beta_end, s.config.prediction_type) == (0.00085, 0.012, "epsilon")
        assert r(name, scheduler_config=sd_config("v_prediction"), prediction_type="v_prediction").config.prediction_type == "v_prediction"
        assert r(name, scheduler_config=dict(cfg, timestep_spacing="trailing")).config.timestep_spacing == "trailing"
        assert r(name).config.timestep_spacing == "linspace"                       # no config: the SD 1.x fields
    assert set(models.SERVED_SCHEDULERS) == {"DDIMScheduler", "DPMSolverMultistepScheduler", "EulerDiscreteScheduler",
                                             "LMSDiscreteScheduler"}


def test_resolver_refuses_with_the_reason(models):
    r = models.resolve_scheduler
    for name in ("HeunDiscreteScheduler", "KDPM2DiscreteScheduler"):
        with pytest.raises(RuntimeError, match=f"{name}.*two UNet evaluations per step"):
            r(name)
    for name in ("EulerAncestralDiscreteScheduler", "KDPM2AncestralDiscreteScheduler", "DPMSolverSDEScheduler"):
        with pytest.raises(RuntimeError, match=f"{name}.*generator the reference does not seed"):
            r(name)
    for name in ("UniPCMultistepScheduler", "PNDMScheduler", "DEISMultistepScheduler"):
        with pytest.raises(RuntimeError, match=f"{name} is not implemented"):
            r(name)
    with pytest.raises(AssertionError, match="cannot be used with"):
        r("EulerDiscreteScheduler", True)
    with pytest.raises(RuntimeError, match="prediction_type disagrees"):
        r("EulerDiscreteScheduler", scheduler_config=sd_config("v_prediction"))
    with pytest.raises(RuntimeError, match="beta_schedule"):
        r("LMSDiscreteScheduler", scheduler_config=sd_config(beta_schedule="squaredcos_cap_v2"))
    with pytest.raises(NotImplementedError, match="karras"):
        r("LMSDiscreteScheduler", scheduler_config=sd_config(use_karras_sigmas=True))


def test_the_new_entry_is_bound():
    import __graft_entry__ as ge
    ge.build()
    assert hasattr(_lib.load(), "lgd_cfg_lms_step_f32") and len(_lib.SIGNATURES["lgd_cfg_lms_step_f32"]) == 13
    assert _lib.ABI_VERSION == 12

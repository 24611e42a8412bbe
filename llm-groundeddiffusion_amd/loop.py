"""What the denoising loops share on the host (sampler.LMDSampler, sdxl.SDXLRefiner, multidiffusion): captured graphs,
the cache of fixed-address device states, the capture-or-eager runner, the per-step skeleton and the fused CFG + scheduler
step that a scheduler's `step_kind` selects.  Sits below all three in the import graph.

Order every loop keeps: per-run constants and coefficient tables (text, timesteps, set_step), then the runners (a capture's
warm-up launch must see valid constants), then this call's latents."""
import torch

from . import ops
from .lanes import GATE
from .scheduler import DDIM, LMS, MULTISTEP, PLMS

F32 = torch.float32


class HipGraph:
    """A captured hipGraph of a launch sequence (torch.cuda.CUDAGraph drives hipStreamBeginCapture on
    torch's current stream — the stream every lgd_* call is enqueued on).  Replaces ~400 host-side
    launches per UNet call by one hipGraphLaunch; everything that varies between replays (timestep,
    frozen-step count, latents, maps) lives in device memory at fixed addresses."""

    def __init__(self, fn, warmup: int = 1):
        # exclusive among the host threads of a lanes.LanePool: other lanes park at their next step boundary
        with GATE.exclusive():
            cur = torch.cuda.current_stream()
            side = torch.cuda.Stream()
            side.wait_stream(cur)
            with torch.cuda.stream(side):
                for _ in range(warmup):
                    fn()                       # also triggers one-time hipFuncSetAttribute calls
            cur.wait_stream(side)
            cur.synchronize()
            side.synchronize()
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph, capture_error_mode="thread_local"):
                fn()

    def __call__(self):
        self.graph.replay()


class StepKernel:
    """The fused CFG + scheduler step of one kind on one state's latents: its coefficient table (`capacity` rows) and the
    extra buffers that kernel carries between steps, at fixed addresses because captured graphs bake them."""
    COLS = {DDIM: 4, MULTISTEP: 8, PLMS: 16, LMS: 16}

    def __init__(self, kind, lat, capacity):
        self.kind = kind
        self.tab = torch.zeros((capacity, self.COLS[kind]), device=lat.device, dtype=F32)
        if kind == MULTISTEP:
            self.x0_prev = torch.zeros_like(lat)
        elif kind == PLMS:                                  # ring of the last three outputs, saved sample
            self.ets = torch.zeros((3,) + tuple(lat.shape), device=lat.device, dtype=F32)
            self.cur_sample = torch.zeros_like(lat)
        elif kind == LMS:                                   # ring of the last four derivatives
            self.ring = torch.zeros((4,) + tuple(lat.shape), device=lat.device, dtype=F32)

    def load(self, scheduler, guidance_scale, timesteps):
        dev = self.tab.device
        if self.kind == PLMS:
            rows = scheduler.plms_table(guidance_scale, dev, timesteps=timesteps)
        elif self.kind == LMS:
            rows = scheduler.lms_table(guidance_scale, dev, timesteps=timesteps)
        elif self.kind == MULTISTEP:
            rows = scheduler.multistep_table(guidance_scale, dev, timesteps=timesteps)
        else:
            rows = scheduler.coef_table(guidance_scale, dev, timesteps=timesteps,
                                        step_ratios=scheduler.dynamic_step_sizes(timesteps))
        self.tab[:len(rows)].copy_(rows)

    def launch(self, eps, lat, dyn, frozen_ref=None, mask=None, hist=None):
        if self.kind == PLMS:
            ops.cfg_plms_step(eps, lat, lat, self.ets, self.cur_sample, self.tab, dyn, hist=hist)
        elif self.kind == LMS:
            ops.cfg_lms_step(eps, lat, lat, self.ring, self.tab, dyn, frozen_ref=frozen_ref, mask=mask, hist=hist)
        elif self.kind == MULTISTEP:
            ops.cfg_multistep_step(eps, lat, lat, self.x0_prev, self.tab, dyn, frozen_ref=frozen_ref, mask=mask, hist=hist)
        else:
            ops.cfg_ddim_step(eps, lat, lat, self.tab, dyn, frozen_ref=frozen_ref, mask=mask, hist=hist)


class LoopState:
    """Fixed-address device buffers of one loop shape with room for `capacity` steps.  The captured graphs and the step
    kernels bake these addresses, so they live and die with the state."""

    def __init__(self, lat, capacity):
        self.lat, self.capacity = lat, capacity
        self.graphs, self.steps = {}, {}

    def step_kernel(self, kind) -> StepKernel:
        """Created on first use: a state only carries the buffers of the kinds it ran."""
        if kind not in self.steps:
            self.steps[kind] = StepKernel(kind, self.lat, self.capacity)
        return self.steps[kind]

    def runner(self, name, fn, use_graphs):
        """fn enqueued eagerly or as a cached hipGraph."""
        if not use_graphs:
            return fn
        if name not in self.graphs:
            self.graphs[name] = HipGraph(fn)
        return self.graphs[name]


class StateCache:
    """Least-recently-used cache of states, so that a long run over many shapes keeps a bounded footprint."""

    def __init__(self, capacity):
        self.capacity, self.states = capacity, {}

    def get(self, key, make, fits=lambda st: True):
        st = self.states.pop(key, None)
        if st is None or not fits(st):
            st = make()
        self.states[key] = st                                    # (re)insert at the MRU end
        while len(self.states) > self.capacity:
            self.states.pop(next(iter(self.states)))
        return st


def clamp_steps(first_step, n_steps, total):
    """(first, last) of `first_step .. first_step + n_steps - 1` within a schedule of `total` steps."""
    first = max(0, min(int(first_step), total))
    return first, total if n_steps is None else min(total, first + int(n_steps))


def history_of(hist, rows, first, last):
    """The history a call returns: rows first .. last of the state's `hist` (the start it ran from and the steps it ran),
    every other row of hist[:rows] zero.  The state keeps whatever earlier calls wrote in those rows; a call never returns it."""
    if first == 0 and last == rows - 1:
        return hist[:rows].clone()
    out = torch.zeros_like(hist[:rows])
    out[first:last + 1].copy_(hist[first:last + 1])
    return out


def run_steps(eng, first, last, body):
    for index in range(first, last):
        GATE.checkpoint()                    # lanes.py: a safe point per step, another lane may be waiting to capture
        eng.set_step(index)
        body(index)

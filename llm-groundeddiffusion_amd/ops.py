"""Thin host wrappers over the C ABI: torch tensors in, raw device pointers across the boundary.

torch is used for device memory and the current HIP stream only.  Every function enqueues kernels on
`torch.cuda.current_stream()` and returns immediately (graph-capturable).  No fallbacks: a failing
call raises RuntimeError (the error convention of the reference's plugin boundary,
generate.py:391-396).
"""
import contextlib
import ctypes as C

import torch

from . import _lib
from ._lib import EPI_GEGLU, EPI_OUT_F32, EPI_RES_F32, EPI_ROWNORM, PAIR_DUP, PAIR_HALF, LgdGemmDesc

F16, F32 = torch.float16, torch.float32


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _call(name, *args):
    lib = _lib.load()
    rc = getattr(lib, name)(*args)
    _lib.check(rc, name)


def _operands(fn, *specs):
    """What the library cannot see from an address: every (name, tensor, dtype, element count) of `specs` is a contiguous
    tensor of that dtype with that many elements (count None: any; tensor None: an optional operand left out)."""
    for name, t, dtype, count in specs:
        if t is None:
            continue
        if t.dtype != dtype:
            raise RuntimeError(f"{fn}: {name} is {t.dtype}, the kernel reads {dtype}")
        if not t.is_contiguous():
            raise RuntimeError(f"{fn}: {name} is not contiguous (shape {tuple(t.shape)}, strides {t.stride()})")
        if count is not None and t.numel() != count:
            raise RuntimeError(f"{fn}: {name} holds {t.numel()} elements, the call addresses {count}")


def set_option(name: str, value: int):
    """Kernel-variant switch of the library (lgd_set_option): e.g. set_option("attn32", 0 | 1 | 2)."""
    _call("lgd_set_option", name.encode(), int(value))


def get_option(name: str) -> int:
    """Current value of an option (lgd_get_option answers every name lgd_set_option knows)."""
    v = _lib.load().lgd_get_option(name.encode())
    if v < 0:
        raise RuntimeError(f"lgd_get_option({name}) failed")
    return v


# ---------------------------------------------------------------------------------------------
# GEMM / conv
# ---------------------------------------------------------------------------------------------
import threading as _threading
_TLS = _threading.local()   # split-K workspace of ad-hoc calls: one per host thread (= one per HIP stream lane, lanes.py)
WS_FLOATS = 1 << 26


def workspace(device) -> torch.Tensor:
    """fp32 split-K scratch for calls that bring none.  Launches of ONE host thread run back to back on its current
    stream and may share it; two threads driving two streams (lanes.LanePool) must not, hence thread-local.  Engines
    own their own (UNetEngine.workspace): their descriptors are baked into plans and hipGraphs."""
    dev = torch.device(device)
    ws = getattr(_TLS, "ws", None)
    if ws is None or ws.device != dev:
        ws = _TLS.ws = torch.empty(WS_FLOATS, device=dev, dtype=F32)
    return ws


N_COUNTERS = 1 << 16
import os as _os
# In-launch split-K combine ("last arriver reduces", LgdGemmDesc.cnt): implemented, bit-identical, and MEASURED SLOWER on
# MI355X than the second launch it replaces — every workgroup's agent-scope release is a write-back of its XCD's L2
# (M = 256, K = 11520, 12 splits: 57 us vs 26 us; default bench 1.21 vs 1.28 images/s) — so it stays off.
SPLITK_IN_LAUNCH = _os.environ.get("LGD_SPLITK_IN_LAUNCH", "0") == "1"


def splitk_counters(device):
    # one buffer per host thread = per lane = per stream: the header allows one counter buffer to serve the GEMMs of ONE
    # stream only (concurrent launches of one shape on two streams would share ticket slots).  Thread-local, like the
    # split-K scratch: the buffer goes away with its lane thread instead of accumulating under dead thread ids
    dev = torch.device(device)
    cnt = getattr(_TLS, "cnt", None)
    if cnt is None or cnt.device != dev:
        cnt = _TLS.cnt = torch.zeros(N_COUNTERS, device=dev, dtype=torch.int32)
    return cnt


def choose_splits(M, N, K, batches=1):
    """Split-K heuristic (used when the tuning table has no entry): spread small-M problems
    (8x8 / 16x16 levels) over all 256 CUs."""
    wgs = ((M + 127) // 128) * ((N + 63) // 64) * batches
    if wgs >= 256:
        return 1
    ktiles = K // 64
    s = min((512 + wgs - 1) // wgs, max(1, ktiles // 4), 16)
    return max(1, s)


def gemm_desc(a0, w, c, M, N, K, *, a1=None, lda0=None, lda1=0, c0=None, c1=0, taps=1,
              hin=0, win=0, hout=0, wout=0, stride=1, ups=0, ldw=None, bias=None, bias2=None,
              res=None, ldr=0, alpha=1.0, epi=0, ldc=None, splits=None, ws=None, tile=0,
              nb_o=1, nb_i=1, a_bs=(0, 0), w_bs=(0, 0), c_bs=(0, 0), r_bs=(0, 0), rowstat=None, colsum=None):
    """Builds an LgdGemmDesc from raw pointers (ints) or tensors.  splits=None / tile=0: taken from
    the measured tuning table (tuning_gfx950.json) when the shape is listed, else from heuristics."""
    d = LgdGemmDesc()
    ptr = lambda t: (t.data_ptr() if torch.is_tensor(t) else (t or 0))
    d.a0, d.a1 = ptr(a0), ptr(a1)
    cin = K // taps
    d.c0 = cin - c1 if c0 is None else c0
    d.c1 = c1
    d.lda0 = d.c0 if lda0 is None else lda0
    d.lda1 = lda1 if lda1 else max(c1, 0)
    d.taps, d.hin, d.win, d.hout, d.wout, d.stride, d.ups = taps, hin, win, hout, wout, stride, ups
    d.w = ptr(w)
    d.ldw = K if ldw is None else ldw
    d.M, d.N, d.K = M, N, K
    d.nb_o, d.nb_i = nb_o, nb_i
    d.a_bs_o, d.a_bs_i = a_bs
    d.w_bs_o, d.w_bs_i = w_bs
    d.c_bs_o, d.c_bs_i = c_bs
    d.r_bs_o, d.r_bs_i = r_bs
    d.bias, d.bias2 = ptr(bias), ptr(bias2)
    d.res, d.ldr = ptr(res), ldr
    if rowstat is not None:                              # rows arrive raw, w / bias / colsum are the folded set (weightstore)
        epi |= EPI_ROWNORM
    d.rowstat, d.colsum = ptr(rowstat), ptr(colsum)
    d.alpha, d.epi = alpha, epi
    d.c = ptr(c)
    n_out = N // 2 if (epi & EPI_GEGLU) else N
    d.ldc = n_out if ldc is None else ldc
    ent = tuning_table().get(shape_key(d)) if (splits is None or not tile) else None
    if splits is None:
        splits = ent["splits"] if ent else choose_splits(M, N, K, nb_o * nb_i)
    if splits > 1 and ws is None:
        need = splits * M * N * nb_o * nb_i
        ws = workspace(c.device if torch.is_tensor(c) else "cuda")
        if need > ws.numel():
            raise RuntimeError(f"split-K workspace too small for {splits}x{M}x{N}")
    d.splits, d.ws = splits, ptr(ws)
    d.cnt = 0
    d.tile = tile
    if not tile:
        # the table is keyed by shape_key (M, N, K, gather, GEGLU flag), not by the whole descriptor: its tile serves
        # this one only where the library accepts it (epilogue form, strides, alignment), else the heuristic's
        if ent and ent["splits"] == splits:
            d.tile = ent["tile"]
        if not d.tile or not gemm_accepts(d):
            d.tile = choose_tile(M, N, nb_o * nb_i * max(splits, 1), bool(epi & EPI_GEGLU), K,
                                 pipe_ok=(K % 64 == 0 and d.c0 % 64 == 0 and d.c1 % 64 == 0))
    log = getattr(_TUNING_TLS, "log", None)
    if log is not None:                                  # tests: which table entries a plan was built from
        log.append((shape_key(d), d.tile, splits))
    if splits > 1 and SPLITK_IN_LAUNCH and torch.is_tensor(c) and c.is_cuda:
        # the smallest tile of the library is 32 rows x 64 columns: an upper bound of the launch's output tiles
        if nb_o * nb_i * ((M + 31) // 32) * ((N + 63) // 64) <= N_COUNTERS:
            d.cnt = splitk_counters(c.device).data_ptr()
            if not gemm_accepts(d):                      # a tile without the in-launch combine: reduce launch
                d.cnt = 0
    return d


def gemm_accepts(d) -> bool:
    """Whether lgd_gemm_f16 would launch descriptor `d` (lgd_gemm_check: host only, needs no GPU)."""
    return _lib.load().lgd_gemm_check(C.byref(d)) == 0


def gemm_set_pair(d, mode) -> bool:
    """CFG pair mode of a built descriptor (LgdGemmDesc.pair: rows m and m + M/2 are identical, rows < M/2 are computed;
    PAIR_HALF leaves the second half of C alone, PAIR_DUP stores every piece twice).  Tile, splits and shape key stay
    those of the full launch.  False — and the descriptor unchanged — where the library refuses (split-K, batched, odd M)."""
    prev, d.pair = d.pair, mode
    if mode and not gemm_accepts(d):
        d.pair = prev
        return False
    return True


def choose_tile(M, N, batches=1, geglu=False, K=64, pipe_ok=False):
    """Tile heuristic for shapes the tuning table does not list (same rule as the library's auto mode,
    done here so the choice is known to the profiler): the largest tile that still yields enough
    workgroups for 256 CUs; 160-wide tiles when they divide N (every UNet width is 320 k).  Codes
    17..23 select the LDS-DMA main loop (the library falls back to register staging if K % 64)."""
    wgs = lambda bm, bn: batches * ((M + bm - 1) // bm) * ((N + bn - 1) // bn)
    if M <= 32:
        return 21
    if pipe_ok:
        # shapes outside the measured table (VAE decoder, SAM, batch sizes the tuner did not visit): the 8-wave pipelined
        # tiles, largest first, as soon as they fill the chip once — what the table picks for 2/3 of the UNet's shapes
        if not geglu and N % 160 == 0 and wgs(256, 160) >= 256:
            return 33
        if N % 128 == 0 and wgs(256, 128) >= 256:
            return 34
        if not geglu and N % 160 == 0 and wgs(128, 160) >= 256:
            return 37
        if N % 128 == 0 and wgs(128, 128) >= 256:
            return 38
    if not geglu and N % 160 == 0:
        if wgs(128, 160) >= 384:
            return 22
        if wgs(64, 160) >= 256:
            return 23
    if wgs(128, 128) >= 384 and N % 128 == 0:
        return 17
    if wgs(64, 128) >= 256 and N % 128 == 0:
        return 19
    return 20


def shape_key(d) -> str:
    """Identity of a GEMM launch for the tuning table (everything that changes its cost)."""
    return (f"M{d.M}_N{d.N}_K{d.K}_t{d.taps}_c{d.c0}+{d.c1}_h{d.hin}x{d.hout}_s{d.stride}_u{d.ups}"
            f"_e{d.epi & 1}_b{d.nb_o * d.nb_i}")


_TUNING = {}
# "latency": tile / split-K per shape chosen for the shortest isolated launch (one launch sequence owns the GPU);
# "throughput": chosen for the lowest cost when several sequences share the GPU (lanes.LanePool; the same launch on
# 4 streams at once, tools/tune_gemm.py LGD_TUNE_STREAMS=4): fewer split-K slabs, larger tiles — a launch may leave CUs
# idle, another lane fills them.  Plans read the table when they are BUILT.
TUNING_MODE = _os.environ.get("LGD_TUNING_MODE", "latency")
# "heuristic": no table at all — choose_tile / choose_splits for every shape: a launch configuration that does not move
# when the tables are re-tuned (the pinned reference point of the full-width gradient gate, tests/test_bench_path_gpu.py)
_TUNING_FILES = {"latency": ("tuning_gfx950.json",), "throughput": ("tuning_gfx950.json", "tuning_gfx950_lanes.json"),
                 "heuristic": ()}
_TUNING_TLS = _threading.local()


def set_tuning_mode(mode: str):
    """Process-wide DEFAULT (tools / A-B runs).  Engines and lanes do not use it: a lane engine carries its own
    `tuning_mode` and a lane thread selects the table with `tuning(...)` for the launches it describes itself."""
    global TUNING_MODE
    if mode not in _TUNING_FILES:
        raise ValueError(f"tuning mode {mode!r}: expected one of {sorted(_TUNING_FILES)}")
    if _os.environ.get("LGD_TUNING_MODE"):       # an explicit environment choice wins (A/B measurements)
        return
    TUNING_MODE = mode


def current_tuning_mode() -> str:
    if _os.environ.get("LGD_TUNING_MODE"):
        return TUNING_MODE
    return getattr(_TUNING_TLS, "mode", None) or TUNING_MODE


@contextlib.contextmanager
def tuning(mode):
    """Table selection for the GEMM descriptors built by THIS thread inside the block (None = leave as is): plan
    construction of an engine, the body of a lane thread.  Nothing process-wide changes."""
    if mode is not None and mode not in _TUNING_FILES:
        raise ValueError(f"tuning mode {mode!r}: expected one of {sorted(_TUNING_FILES)}")
    prev = getattr(_TUNING_TLS, "mode", None)
    if mode is not None:
        _TUNING_TLS.mode = mode
    try:
        yield
    finally:
        _TUNING_TLS.mode = prev


@contextlib.contextmanager
def desc_log():
    """Collects (shape key, tile, splits) of every GEMM descriptor this thread builds inside the block."""
    prev, _TUNING_TLS.log = getattr(_TUNING_TLS, "log", None), []
    try:
        yield _TUNING_TLS.log
    finally:
        _TUNING_TLS.log = prev


def tuning_table():
    mode = current_tuning_mode()
    if mode not in _TUNING:
        import json
        tab = {}
        for fname in _TUNING_FILES[mode]:      # later files override earlier ones shape by shape
            path = _os.path.join(_os.path.dirname(_os.path.abspath(__file__)), fname)
            if _os.path.exists(path):
                tab.update(json.load(open(path)))
        _TUNING[mode] = tab
    return _TUNING[mode]


class LaunchProfiler:
    """Samples kernel durations with HIP events on the launch stream (torch.cuda.Event records on
    torch's current stream, which is the stream every lgd_* call is enqueued on)."""

    def __init__(self, max_records=20000):
        self.recs = []
        self.max = max_records
        self.enabled = True

    def wrap(self, name, flops, nbytes, fn, tag=None, shape=None):
        if not self.enabled or len(self.recs) >= self.max:
            return fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        self.recs.append((name, flops, nbytes, e0, e1, tag, shape))
        return r

    def summary(self, by_tag=False, by_shape=False):
        """Per kernel name (or per caller tag, e.g. "attn_path"; or per launch shape "kernel | shape key"): ms,
        algorithmic flops / bytes, launches."""
        torch.cuda.synchronize()
        agg = {}
        for name, fl, nb, e0, e1, tag, shape in self.recs:
            if by_tag and tag is None:
                continue
            key = tag if by_tag else (f"{name} | {shape}" if by_shape else name)
            a = agg.setdefault(key, dict(ms=0.0, flops=0.0, bytes=0.0, n=0))
            a["ms"] += e0.elapsed_time(e1)
            a["flops"] += fl
            a["bytes"] += nb
            a["n"] += 1
        return agg


PROFILER = None


def _prof(name, nbytes, fn, *, flops=0.0, tag=None, shape=None):
    """Runs `fn` (one kernel launch, or the few launches of one C-ABI entry point); under a LaunchProfiler the launch is
    bracketed by HIP events and booked under `name` with its ALGORITHMIC bytes / flops.  Every entry point a UNet plan
    or a sampler step enqueues goes through here or through gemm_launch / attn_fwd, so that the profiler's kernels sum
    to the launch sequence's time (bench.py `roofline.all_kernels`)."""
    if PROFILER is not None:
        return PROFILER.wrap(name, flops, nbytes, fn, tag, shape)
    return fn()


def copy_(dst, src):
    """dst.copy_(src) on the current stream, visible to the launch profiler (plan-internal copies: CFG duplication of the
    latents, first-writer gradient copies of residual branches, captured-map slices)."""
    return _prof("copy", 2.0 * dst.numel() * dst.element_size(), lambda: dst.copy_(src))


def zero_(t):
    return _prof("fill", float(t.numel() * t.element_size()), lambda: t.zero_())


def gemm_launch(desc, tag=None, flops=None):
    """`flops`: algorithmic work when it differs from 2*M*N*K of the launch (conv_in multiplies a zero / remainder-padded K)."""
    if PROFILER is not None:
        nb = desc.nb_o * desc.nb_i
        if flops is None:
            flops = 2.0 * desc.M * desc.N * desc.K * nb
        if desc.pair:                                    # half the rows are computed (the shape key keeps the full M)
            flops *= 0.5
        m_in, m_out = (desc.M // 2 if desc.pair else desc.M), (desc.M // 2 if desc.pair == PAIR_HALF else desc.M)
        nbytes = 2.0 * nb * (m_in * desc.K / max(desc.taps, 1) + desc.N * desc.K + m_out * desc.N)
        return PROFILER.wrap(_table("TILE_NAMES").get(desc.tile, "gemm"), flops, nbytes,
                             lambda: _call("lgd_gemm_f16", C.byref(desc), _stream()), tag,
                             shape=f"{shape_key(desc)} splits={desc.splits}")
    _call("lgd_gemm_f16", C.byref(desc), _stream())


def linear(x, w, bias=None, res=None, out=None, *, alpha=1.0, geglu=False, out_f32=False,
           splits=None, ws=None, tile=0, bias2=None, rowstat=None, colsum=None):
    """y = x @ w.T (+bias) ... ; x [M,K] fp16 contiguous, w [N,K] fp16."""
    M, K = x.shape
    N = w.shape[0]
    n_out = N // 2 if geglu else N
    if out is None:
        out = torch.empty((M, n_out), device=x.device, dtype=F32 if out_f32 else F16)
    epi = (EPI_GEGLU if geglu else 0) | (EPI_OUT_F32 if out_f32 else 0)
    if res is not None and res.dtype == F32:
        epi |= EPI_RES_F32
    d = gemm_desc(x, w, out, M, N, K, bias=bias, bias2=bias2, res=res,
                  ldr=(res.stride(0) if res is not None else 0), alpha=alpha, epi=epi,
                  splits=splits, ws=ws, tile=tile, lda0=x.stride(0), ldw=w.stride(0),
                  ldc=out.stride(0), rowstat=rowstat, colsum=colsum)
    gemm_launch(d)
    return out


def conv3x3(x, w, B, H, W, *, x1=None, bias=None, bias2=None, res=None, stride=1, ups=False,
            out=None, splits=None, ws=None, tile=0, alpha=1.0):
    """3x3 conv, pad 1, channels-last.  x [B*H*W, C0] (stored map; with ups the logical input is
    2H x 2W), optional x1 [B*H*W, C1] concatenated on channels; w [Cout, 9*(C0+C1)]."""
    c0 = x.shape[1]
    c1 = x1.shape[1] if x1 is not None else 0
    Cout = w.shape[0]
    K = 9 * (c0 + c1)
    assert w.shape[1] == K
    if ups:
        Hl, Wl = 2 * H, 2 * W
    else:
        Hl, Wl = H, W
    Ho, Wo = (Hl - 1) // stride + 1, (Wl - 1) // stride + 1
    M = B * Ho * Wo
    if out is None:
        out = torch.empty((M, Cout), device=x.device, dtype=F16)
    d = gemm_desc(x, w, out, M, Cout, K, a1=x1, c0=c0, c1=c1, lda0=x.stride(0),
                  lda1=(x1.stride(0) if x1 is not None else 0), taps=9, hin=H, win=W, hout=Ho,
                  wout=Wo, stride=stride, ups=int(ups), bias=bias, bias2=bias2, res=res,
                  ldr=(res.stride(0) if res is not None else 0), splits=splits, ws=ws, tile=tile,
                  alpha=alpha, ldc=out.stride(0))
    gemm_launch(d)
    return out


def conv_in(x_nchw, w, bias, out=None):
    B, Cin, L, _ = x_nchw.shape
    Cout = w.shape[0]
    if out is None:
        out = torch.empty((B * L * L, Cout), device=x_nchw.device, dtype=F16)
    _operands("conv_in", ("x", x_nchw, F32, B * Cin * L * L), ("w", w, F16, Cout * 9 * Cin), ("bias", bias, F32, Cout),
              ("out", out, F16, B * L * L * Cout))
    _call("lgd_conv_in_f16", _p(x_nchw), _p(w), _p(bias), _p(out), B, Cin, L, Cout, _stream())
    return out


def nchw_to_nhwc8(x_nchw, out=None):
    """(B, C<=8, H, W) fp32 -> [B*H*W, 8] fp16, zero channels behind C."""
    B, C_, H, W = x_nchw.shape
    if out is None:
        out = torch.empty((B * H * W, 8), device=x_nchw.device, dtype=F16)
    _operands("nchw_to_nhwc8", ("x", x_nchw, F32, None), ("out", out, F16, B * H * W * 8))
    _prof("nchw_to_nhwc8_kernel", 4.0 * x_nchw.numel() + 2.0 * out.numel(),
          lambda: _call("lgd_nchw_to_nhwc8_f16", _p(x_nchw), _p(out), B, C_, H * W, _stream()))
    return out


_U8_TABLES = {}


def u8_table(device) -> torch.Tensor:
    """fp32 [256] = 2 * (u / 255) - 1, computed by the host in fp32 with true division (pipelines.py:101-104: numpy's
    astype(float32) / 255.0, then 2.0 * x - 1.0) — the table lgd_image_u8_to_nhwc8_f16 reads."""
    key = str(device)
    if key not in _U8_TABLES:
        u = torch.arange(256, dtype=F32)
        _U8_TABLES[key] = (2.0 * (u / 255.0) - 1.0).to(device)
    return _U8_TABLES[key]


def image_u8_to_nhwc8(img_u8, out=None):
    """uint8 (B, H, W, 3) on the device -> [B*H*W, 8] fp16: value, rounding remainder, zeros (lgd_hip.h)."""
    if img_u8.dim() != 4 or img_u8.shape[3] != 3:
        raise RuntimeError(f"image_u8_to_nhwc8: img {tuple(img_u8.shape)} is not (B, H, W, 3)")
    B, H, W, _ = img_u8.shape
    if out is None:
        out = torch.empty((B * H * W, 8), device=img_u8.device, dtype=F16)
    _operands("image_u8_to_nhwc8", ("img", img_u8, torch.uint8, None), ("out", out, F16, B * H * W * 8))
    _call("lgd_image_u8_to_nhwc8_f16", _p(img_u8), _p(u8_table(img_u8.device)), _p(out), B, H * W, _stream())
    return out


def vae_sample(moments, noise, scale, out=None):
    """moments fp16 [B*HW, 2z] (channels-last), noise fp32 (B, z, H, W) -> scale * (mean + std * noise), NCHW fp32."""
    if noise.dim() != 4:
        raise RuntimeError(f"vae_sample: noise {tuple(noise.shape)} is not (B, z, H, W)")
    B, z, H, W = noise.shape
    if out is None:
        out = torch.empty_like(noise)
    _operands("vae_sample", ("moments", moments, F16, B * H * W * 2 * z), ("noise", noise, F32, None),
              ("out", out, F32, noise.numel()))
    _call("lgd_vae_sample_f32", _p(moments), _p(noise), _p(out), B, z, H * W, float(scale), _stream())
    return out


def range_f16(x2d, table, site):
    """Row `site` of `table` (int32 [n, 2], zeroed by the caller) takes the range of x2d (fp16 [rows, cols], rows
    `stride(0)` elements apart): word 0 = the fp32 bits of the largest finite |x| so far, word 1 = how many elements were
    not finite (lgd_hip.h: lgd_range_f16).  Calls accumulate; read word 0 through `table.view(torch.float32)`."""
    if x2d.dim() != 2 or x2d.dtype != F16 or (x2d.shape[1] > 1 and x2d.stride(1) != 1):
        raise RuntimeError(f"range_f16: x is {x2d.dtype} {tuple(x2d.shape)} with strides {x2d.stride()}, the kernel reads fp16 rows")
    _operands("range_f16", ("table", table, torch.int32, None))
    if table.dim() != 2 or table.shape[1] != 2 or not 0 <= int(site) < table.shape[0]:
        raise RuntimeError(f"range_f16: table {tuple(table.shape)} has no pair {site}")
    rows, cols = x2d.shape
    ld = x2d.stride(0) if rows > 1 else cols
    _call("lgd_range_f16", _p(x2d), rows, cols, ld, C.c_void_p(table.data_ptr() + 8 * int(site)), _stream())


def conv_out(x, w, bias, B, L, out=None, out_scale=1.0):
    Cin = x.shape[1]
    Cout = w.shape[0]
    if out is None:
        out = torch.empty((B, Cout, L, L), device=x.device, dtype=F32)
    _operands("conv_out", ("x", x, F16, B * L * L * Cin), ("w", w, F16, Cout * 9 * Cin), ("bias", bias, F32, Cout),
              ("out", out, F32, B * Cout * L * L))
    _prof("conv_out_kernel", 2.0 * x.numel() + 4.0 * out.numel(),
          lambda: _call("lgd_conv_out_f16", _p(x), _p(w), _p(bias), _p(out), B, Cin, L, Cout, float(out_scale), _stream()),
          flops=2.0 * B * L * L * Cout * 9 * Cin)
    return out


# ---------------------------------------------------------------------------------------------
# norms
# ---------------------------------------------------------------------------------------------
GN_STATS_WGS = int(_os.environ.get("LGD_GN_STATS_WGS", "1024"))      # workgroups per launch the statistics pass aims at


def gn_chunks(B, HW):
    """Pixel chunks per image of the GroupNorm statistics pass (>= 8 pixels each, at most 64 so that the
    partial table [B, nchunk, G, 2] every apply workgroup re-reduces stays at 16 KB per image)."""
    return max(1, min(HW // 8, GN_STATS_WGS // max(B, 1), 64))


def groupnorm(x, B, HW, G, eps, gamma, beta, silu, *, x1=None, out=None, part=None, stats=None, pair=0):
    """pair (PAIR_HALF / PAIR_DUP): images b and b + B/2 are identical, images < B/2 are normalised (lgd_groupnorm_pair_f16)."""
    c0 = x.shape[1]
    c1 = x1.shape[1] if x1 is not None else 0
    C_ = c0 + c1
    nchunk = gn_chunks(B, HW)
    if out is None:
        out = torch.empty((B * HW, C_), device=x.device, dtype=F16)
    if part is None:
        part = torch.empty((B, nchunk, G, 2), device=x.device, dtype=F32)
    if pair:
        assert stats is None, "pair mode is a no-grad forward: no statistics output"
        _prof("groupnorm (gn_stats + gn_apply | gn_fused)", (2.0 + (2.0 if pair == PAIR_DUP else 1.0)) * B * HW * C_,
              lambda: _call("lgd_groupnorm_pair_f16", _p(x), _p(x1), c0, c1, B, HW, G, float(eps), _p(gamma), _p(beta),
                            1 if silu else 0, _p(out), _p(part), nchunk, int(pair), _stream()), shape=f"B{B}_HW{HW}_C{C_}")
        return out
    # algorithmic bytes: the map read once for the statistics, once for the apply, written once
    _prof("groupnorm (gn_stats + gn_apply | gn_fused)", 6.0 * B * HW * C_,
          lambda: _call("lgd_groupnorm_f16", _p(x), _p(x1), c0, c1, B, HW, G, float(eps), _p(gamma), _p(beta),
                        1 if silu else 0, _p(out), _p(part), nchunk, _p(stats), _stream()), shape=f"B{B}_HW{HW}_C{C_}")
    return out


def groupnorm_bwd(gy, x, B, HW, G, gamma, beta, silu, stats, *, x1=None, gx0=None, gx1=None,
                  part=None, accumulate=False):
    c0 = x.shape[1]
    c1 = x1.shape[1] if x1 is not None else 0
    nchunk = gn_chunks(B, HW)
    if gx0 is None:
        gx0 = torch.empty_like(x)
    if x1 is not None and gx1 is None:
        gx1 = torch.empty_like(x1)
    if part is None:
        part = torch.empty((B, nchunk, G, 2), device=x.device, dtype=F32)
    _prof("groupnorm_bwd (gn_bwd_stats + gn_bwd_apply)", (10.0 + (2.0 if accumulate else 0.0)) * B * HW * (c0 + c1),
          lambda: _call("lgd_groupnorm_bwd_f16", _p(gy), _p(x), _p(x1), c0, c1, B, HW, G, _p(gamma), _p(beta),
                        1 if silu else 0, _p(stats), _p(gx0), _p(gx1), _p(part), nchunk, 1 if accumulate else 0, _stream()),
          shape=f"B{B}_HW{HW}_C{c0 + c1}")
    return gx0, gx1


# Codes of the norm dispatch (LGD_GN_* / LGD_LN_* of include/lgd_hip.h): the kernel instantiation a call runs; GN_VARIANTS /
# LN_VARIANTS (below) name them.
GN_OP_FWD, GN_OP_BWD = 0, 1
LN_OP_FWD, LN_OP_STATS, LN_OP_BWD = 0, 1, 2


def groupnorm_plan(op, c0, c1, B, HW, G, *, silu=False, pair=0) -> int:
    """The code (a key of GN_VARIANTS) of the kernel instantiation the GroupNorm call with these arguments runs under the
    current option state ("gn_fused", "gn_slab"); host only.  Raises for arguments the library refuses."""
    code = _lib.load().lgd_groupnorm_plan(int(op), c0, c1, B, HW, G, 1 if silu else 0, int(pair))
    _lib.check(min(code, 0), "lgd_groupnorm_plan")
    return code


def layernorm_plan(op, rows, C_, *, ln_stream=None) -> int:
    """The code (a key of LN_VARIANTS) of the kernel instantiation the LayerNorm call runs: op LN_OP_FWD (y written),
    LN_OP_STATS (statistics only) or LN_OP_BWD, `rows` of the full call (a pair launch runs the kernel chosen for them),
    under "ln_stream" = 0 / 1 or, by default, the current option state; host only.  Raises for arguments the library refuses."""
    code = _lib.load().lgd_layernorm_plan(int(op), rows, C_, -1 if ln_stream is None else int(ln_stream))
    _lib.check(min(code, 0), "lgd_layernorm_plan")
    return code


def layernorm_stats_served(rows, C_) -> bool:
    """Whether the statistics-only form serves rows of C_ channels whatever "ln_stream" says (the row kernels do)."""
    return _lib.load().lgd_layernorm_plan(LN_OP_STATS, rows, C_, 0) > 0


def layernorm(x, gamma, beta, eps=1e-5, *, out=None, ldy=None, stats=None, rows_per_batch=0,
              x_bs=0, y_bs=0, rows=None, ldx=None, pair=0):
    """pair = PAIR_HALF: rows r and r + rows/2 are identical, the first rows/2 are normalised (lgd_layernorm_pair_f16)."""
    C_ = gamma.shape[0]
    if rows is None:
        rows = x.numel() // C_
    if out is None:
        out = torch.empty((rows, C_), device=x.device, dtype=F16)
    if pair:
        _prof("layernorm_rows_kernel", 2.0 * rows * C_,
              lambda: _call("lgd_layernorm_pair_f16", _p(x), ldx or C_, _p(out), ldy or C_, rows, C_, float(eps), _p(gamma),
                            _p(beta), _p(stats), rows_per_batch, x_bs, y_bs, int(pair), _stream()), shape=f"R{rows}_C{C_}")
        return out
    _prof("layernorm_rows_kernel", 4.0 * rows * C_,
          lambda: _call("lgd_layernorm_f16", _p(x), ldx or C_, _p(out), ldy or C_, rows, C_, float(eps), _p(gamma),
                        _p(beta), _p(stats), rows_per_batch, x_bs, y_bs, _stream()), shape=f"R{rows}_C{C_}")
    return out


def layernorm_stats(x, C_, eps=1e-5, *, stats=None, rows=None, ldx=None, pair=0):
    """(mean, rstd) of every row, fp32 [rows][2]: the statistics half of LayerNorm, whose other half rides in the
    consuming GEMM's epilogue (EPI_ROWNORM).  pair = PAIR_HALF: the first rows/2 rows only (the halves are identical)."""
    if rows is None:
        rows = x.numel() // C_
    if stats is None:
        stats = torch.empty((rows, 2), device=x.device, dtype=torch.float32)
    if pair:
        _prof("ln_stats_kernel (LayerNorm statistics only)", 1.0 * rows * C_,
              lambda: _call("lgd_layernorm_pair_f16", _p(x), ldx or C_, _p(None), C_, rows, C_, float(eps), _p(None),
                            _p(None), _p(stats), 0, 0, 0, int(pair), _stream()), shape=f"R{rows}_C{C_}")
        return stats
    _prof("ln_stats_kernel (LayerNorm statistics only)", 2.0 * rows * C_,
          lambda: _call("lgd_layernorm_f16", _p(x), ldx or C_, _p(None), C_, rows, C_, float(eps), _p(None), _p(None),
                        _p(stats), 0, 0, 0, _stream()), shape=f"R{rows}_C{C_}")
    return stats


def layernorm_bwd(gy, x, gamma, stats, *, gx=None, rows=None, ldgy=None, ldx=None, ldgx=None,
                  rows_per_batch=0, gy_bs=0, x_bs=0, gx_bs=0, accumulate=False):
    C_ = gamma.shape[0]
    if rows is None:
        rows = x.numel() // C_
    if gx is None:
        gx = torch.empty((rows, C_), device=x.device, dtype=F16)
    _prof("layernorm_bwd_kernel", (6.0 + (2.0 if accumulate else 0.0)) * rows * C_,
          lambda: _call("lgd_layernorm_bwd_f16", _p(gy), ldgy or C_, _p(x), ldx or C_, _p(gx), ldgx or C_, rows, C_,
                        _p(gamma), _p(stats), rows_per_batch, gy_bs, x_bs, gx_bs, 1 if accumulate else 0, _stream()),
          shape=f"R{rows}_C{C_}")
    return gx


# ---------------------------------------------------------------------------------------------
# attention.  Views are (tensor, ld, batch_stride) with head h at column offset h*d.
# ---------------------------------------------------------------------------------------------
def _default_views(H, Sq, Sk, d):
    """The (ld, batch_stride) pairs of contiguous [B, S, H * d] operands: the query side and the key side."""
    return (H * d, Sq * H * d), (H * d, Sk * H * d)


def attn_fwd(q, k, v, o, B, H, Sq, Sk, d, scale, *, lse=None, q_view=None, k_view=None,
             v_view=None, o_view=None, pair=0):
    """pair (PAIR_HALF / PAIR_DUP): images b and b + B/2 hold identical q / k / v, images < B/2 are computed
    (lgd_attn_fwd_pair_f16: the kernel the full launch would run, over half the grid)."""
    dq_, dk_ = _default_views(H, Sq, Sk, d)
    qv, kv, vv, ov = q_view or dq_, k_view or dk_, v_view or dk_, o_view or dq_
    if pair:
        fn = lambda: _call("lgd_attn_fwd_pair_f16", _p(q), qv[0], qv[1], _p(k), kv[0], kv[1], _p(v), vv[0], vv[1],
                           _p(o), ov[0], ov[1], _p(lse), B, H, Sq, Sk, d, float(scale), int(pair), _stream())
    else:
        fn = lambda: _call("lgd_attn_fwd_f16", _p(q), qv[0], qv[1], _p(k), kv[0], kv[1], _p(v), vv[0], vv[1],
                           _p(o), ov[0], ov[1], _p(lse), B, H, Sq, Sk, d, float(scale), _stream())
    if PROFILER is not None:
        Bc = B // 2 if pair else B                        # images computed (the shape keeps the full B)
        PROFILER.wrap(f"attn_self_kernel d={d}", 4.0 * Bc * H * Sq * Sk * d, 2.0 * Bc * H * d * (2 * Sq + 2 * Sk), fn,
                      "attn_path", shape=f"B{B}_H{H}_Sq{Sq}_Sk{Sk}")
    else:
        fn()
    return o


def attn_wide(q, k, v, o, B, Sq, Sk, d, scale, *, q_view=None, k_view=None, v_view=None, o_view=None):
    """Single-head attention for heads up to 512 wide (lgd_attn_wide_f16): o = softmax(scale q k^T) v with fp32 logits
    and no score matrix.  Views (ld, batch_stride) as attn_fwd's, default contiguous [B, S, d]."""
    dq_, dk_ = _default_views(1, Sq, Sk, d)
    qv, kv, vv, ov = q_view or dq_, k_view or dk_, v_view or dk_, o_view or dq_
    fn = lambda: _call("lgd_attn_wide_f16", _p(q), _p(k), _p(v), _p(o), B, Sq, Sk, d, qv[0], kv[0], vv[0], ov[0],
                       qv[1], kv[1], vv[1], ov[1], float(scale), _stream())
    if PROFILER is not None:
        PROFILER.wrap(f"attn_wide_kernel d={d}", 4.0 * B * Sq * Sk * d, 2.0 * B * d * (2 * Sq + 2 * Sk), fn, "attn_path",
                      shape=f"B{B}_Sq{Sq}_Sk{Sk}")
    else:
        fn()
    return o


def attn_bwd(q, k, v, o, go, lse, delta, gq, gk, gv, B, H, Sq, Sk, d, scale, *, q_view=None,
             k_view=None, v_view=None, o_view=None, go_view=None, gq_view=None, gk_view=None,
             gv_view=None, sk_grad=None):
    """sk_grad: dK / dV are computed (and written) for the first sk_grad keys only (lgd_attn_bwd_keys_f16); default all."""
    skg = Sk if sk_grad is None else int(sk_grad)
    dq_, dk_ = _default_views(H, Sq, Sk, d)
    qv, kv, vv = q_view or dq_, k_view or dk_, v_view or dk_
    ov, gov = o_view or dq_, go_view or dq_
    gqv, gkv, gvv = gq_view or dq_, gk_view or dk_, gv_view or dk_
    # flash backward with recompute: QK^T twice (dQ and dK/dV passes), dP = dO V^T twice, dV, dK, dQ -> 14 B H Sq Sk d
    # executed; the ALGORITHMIC work of an attention backward is 5 contractions = 10 B H Sq Sk d (DESIGN.md kernel table)
    _prof(f"attn_bwd_dq + attn_bwd_dkv d={d}", 2.0 * B * H * d * (4 * Sq + 4 * Sk),
          lambda: _call("lgd_attn_bwd_keys_f16", _p(q), qv[0], qv[1], _p(k), kv[0], kv[1], _p(v), vv[0], vv[1], _p(o),
                        ov[0], ov[1], _p(go), gov[0], gov[1], _p(lse), _p(delta), _p(gq), gqv[0], gqv[1], _p(gk),
                        gkv[0], gkv[1], _p(gv), gvv[0], gvv[1], B, H, Sq, Sk, skg, d, float(scale), _stream()),
          # algorithmic: dQ over all keys (S, dP, dQ) + dK / dV for the keys whose gradient is wanted (2 of the 5 contractions)
          flops=6.0 * B * H * Sq * Sk * d + 4.0 * B * H * Sq * skg * d, tag="attn_path_bwd", shape=f"B{B}_H{H}_Sq{Sq}_Sk{Sk}")


def cross_attn_fwd(q, k, v, o, B, H, Sq, Sk, d, scale, *, probs=None, tok=-1, cond_only=False,
                   q_view=None, k_view=None, v_view=None, o_view=None):
    dq_, dk_ = _default_views(H, Sq, Sk, d)
    qv, kv, vv, ov = q_view or dq_, k_view or dk_, v_view or dk_, o_view or dq_
    fn = lambda: _call("lgd_cross_attn_fwd_f16", _p(q), qv[0], qv[1], _p(k), kv[0], kv[1], _p(v), vv[0], vv[1],
                       _p(o), ov[0], ov[1], _p(probs), int(tok), 1 if cond_only else 0, B, H, Sq, Sk, d,
                       float(scale), _stream())
    if PROFILER is not None:
        PROFILER.wrap(f"attn_fwd_kernel(cross) d={d}", 4.0 * B * H * Sq * Sk * d,
                      2.0 * B * H * d * (2 * Sq + 2 * Sk), fn, "attn_path")
    else:
        fn()
    return o


def attn_causal_fwd(q, k, v, o, B, H, S, d, scale, *, view=None):
    """Causal self-attention over a fused [B,S,3*H*d] projection (or separate q/k/v with the default view)."""
    vw = view or (H * d, S * H * d)
    _call("lgd_attn_causal_fwd_f16", _p(q), vw[0], vw[1], _p(k), vw[0], vw[1], _p(v), vw[0], vw[1], _p(o),
          H * d, S * H * d, B, H, S, d, float(scale), _stream())
    return o


# Variant codes of the attention dispatch (lgd_attn_plan): family * 100000 + DP * 100 + sub, DP = the padded head dim of the
# kernel instantiation.
ATTN_OP_FWD, ATTN_OP_BWD, ATTN_OP_CROSS_BWD = 0, 1, 2


# Tables the library owns, read from it on first access (so importing this module does not need it):
#   TILE_NAMES              GEMM tile code -> profiler kernel name (lgd_gemm_tile; tools/ and profiles/ key on the names;
#                           which descriptors a code serves is the library's to say: gemm_accepts)
#   GN_VARIANTS, LN_VARIANTS  LGD_GN_* (below 500) / LGD_LN_* code -> kernel instantiation (lgd_norm_variant)
#   ATTN_VARIANTS           attention variant code -> kernel instantiation (lgd_attn_variant); ATTN_VARIANTS_ENV_ONLY: the
#                           codes only the process-wide A/B switches of the environment (LGD_ATTN_NW, LGD_ATTN_BWD) select
_TABLES = ("TILE_NAMES", "GN_VARIANTS", "LN_VARIANTS", "ATTN_VARIANTS", "ATTN_VARIANTS_ENV_ONLY")


def _rows(export, n_ints):
    """The rows (int, .., name) of a table the library enumerates with export(index, &int, .., name, name_cap)."""
    fn = getattr(_lib.load(), export)
    ints, name, rows = [C.c_int() for _ in range(n_ints)], C.create_string_buffer(128), []
    while fn(len(rows), *map(C.byref, ints), name, len(name)) == 0:
        if len(name.value) >= len(name) - 1:
            raise RuntimeError(f"{export}: the name of row {len(rows)} does not fit {len(name)} bytes")
        rows.append(tuple(i.value for i in ints) + (name.value.decode(),))
    return rows


def _table(attr):
    g = globals()
    if attr not in g:
        attn, norm = _rows("lgd_attn_variant", 2), _rows("lgd_norm_variant", 1)
        g.update(TILE_NAMES=dict(sorted((c, nm) for c, _, _, nm in _rows("lgd_gemm_tile", 3))),
                 GN_VARIANTS={c: nm for c, nm in norm if c < 500}, LN_VARIANTS={c: nm for c, nm in norm if c >= 500},
                 ATTN_VARIANTS={c: nm for c, _, nm in attn},
                 ATTN_VARIANTS_ENV_ONLY=frozenset(c for c, env, _ in attn if env))
    return g[attr]


def __getattr__(attr):
    if attr in _TABLES:
        return _table(attr)
    raise AttributeError(f"module {__name__!r} has no attribute {attr!r}")


def attn_plan(op, B, H, Sq, Sk, d, *, sk_grad=None, probs=False, causal=False, pair=0, aligned=True) -> int:
    """The variant code (a key of ATTN_VARIANTS) the attention call with these arguments runs under the current option
    state; host only.  Raises for arguments the library refuses.  aligned: read for ATTN_OP_CROSS_BWD only (q / go / gq move as
    vectors: the MFMA kernel; else the one-wave-per-row kernel)."""
    code = _lib.load().lgd_attn_plan(int(op), B, H, Sq, Sk, Sk if sk_grad is None else int(sk_grad), d,
                                     1 if probs else 0, 1 if causal else 0, int(pair), 1 if aligned else 0)
    _lib.check(min(code, 0), "lgd_attn_plan")
    return code


def quick_gelu(x, out=None):
    if out is None:
        out = torch.empty_like(x)
    _operands("quick_gelu", ("x", x, F16, None), ("out", out, F16, x.numel()))
    _call("lgd_quick_gelu_f16", _p(x), _p(out), x.numel(), _stream())
    return out


ACT_GELU, ACT_RELU = 1, 2


def act(x, mode, out=None):
    """Exact GELU / ReLU on an fp16 tensor (SAM encoder and mask-decoder MLPs)."""
    if out is None:
        out = torch.empty_like(x)
    _operands("act", ("x", x, F16, None), ("out", out, F16, x.numel()))
    _call("lgd_act_f16", _p(x), _p(out), x.numel(), int(mode), _stream())
    return out


def _sam_rows(B, Hs, Ws, window):
    S = window or Hs
    return B * (-(-Hs // S)) * (-(-Ws // S)) * S * S, S


def sam_relpos_qkv(qkv, qkv_bias, rel_h, rel_w, B, Hs, Ws, window, NH, d, DA, scale, qa=None, ka=None, va=None):
    """Window partition + decomposed rel-pos bias folded into the attention operands (csrc/sam.hip).
    Returns qa, ka, va [B*nwin*S*S, NH*DA] fp16."""
    rows, S = _sam_rows(B, Hs, Ws, window)
    qa, ka, va = (torch.empty((rows, NH * DA), device=qkv.device, dtype=F16) if t is None else t for t in (qa, ka, va))
    _operands("sam_relpos_qkv", ("qkv", qkv, F16, B * Hs * Ws * 3 * NH * d), ("qkv_bias", qkv_bias, F32, 3 * NH * d),
              ("rel_h", rel_h, F32, (2 * S - 1) * d), ("rel_w", rel_w, F32, (2 * S - 1) * d), ("qa", qa, F16, rows * NH * DA),
              ("ka", ka, F16, rows * NH * DA), ("va", va, F16, rows * NH * DA))
    _call("lgd_sam_relpos_qkv_f16", _p(qkv), _p(qkv_bias), _p(rel_h), _p(rel_w), B, Hs, Ws, window, NH, d, DA,
          float(scale), _p(qa), _p(ka), _p(va), _stream())
    return qa, ka, va


def sam_window_merge(oa, B, Hs, Ws, window, NH, d, DA, out=None):
    rows, _ = _sam_rows(B, Hs, Ws, window)
    if out is None:
        out = torch.empty((B * Hs * Ws, NH * d), device=oa.device, dtype=F16)
    _operands("sam_window_merge", ("oa", oa, F16, rows * NH * DA), ("out", out, F16, B * Hs * Ws * NH * d))
    _call("lgd_sam_window_merge_f16", _p(oa), _p(out), B, Hs, Ws, window, NH, d, DA, _stream())
    return out


def cross_attn_bwd(q, k, v, go, gp, gq, B, H, Sq, Sk, d, scale, *, q_view=None, k_view=None,
                   v_view=None, go_view=None, gq_view=None):
    dq_, dk_ = _default_views(H, Sq, Sk, d)
    qv, kv, vv = q_view or dq_, k_view or dk_, v_view or dk_
    gov, gqv = go_view or dq_, gq_view or dq_
    # dQ only (text K / V are constants of the run): recomputed scores, dP = dO V^T (+ the map gradient), dQ = dS K
    _prof(f"cross_attn_bwd_mfma_kernel d={d}", 2.0 * B * H * d * (3 * Sq + 2 * Sk) + (4.0 * B * H * Sq * Sk if gp is not None else 0.0),
          lambda: _call("lgd_cross_attn_bwd_f16", _p(q), qv[0], qv[1], _p(k), kv[0], kv[1], _p(v), vv[0], vv[1],
                        _p(go), gov[0], gov[1], _p(gp), _p(gq), gqv[0], gqv[1], B, H, Sq, Sk, d, float(scale), _stream()),
          flops=(6.0 if go is not None else 4.0) * B * H * Sq * Sk * d, tag="attn_path_bwd")
    return gq


# ---------------------------------------------------------------------------------------------
# elementwise / step
# ---------------------------------------------------------------------------------------------
def geglu_bwd(h, gy, gh=None):
    rows, n2 = h.shape
    if gh is None:
        gh = torch.empty_like(h)
    _operands("geglu_bwd", ("h", h, F16, None), ("gy", gy, F16, rows * (n2 // 2)), ("gh", gh, F16, rows * n2))
    _prof("geglu_bwd_kernel", 2.0 * rows * (n2 + n2 // 2 + n2),
          lambda: _call("lgd_geglu_bwd_f16", _p(h), _p(gy), _p(gh), rows, n2 // 2, _stream()))
    return gh


def geglu_fwd(h, out=None):
    rows, n2 = h.shape
    if out is None:
        out = torch.empty((rows, n2 // 2), device=h.device, dtype=F16)
    _operands("geglu_fwd", ("h", h, F16, None), ("out", out, F16, rows * (n2 // 2)))
    _prof("geglu_fwd_kernel", 2.0 * rows * (n2 + n2 // 2),
          lambda: _call("lgd_geglu_fwd_f16", _p(h), _p(out), rows, n2 // 2, _stream()))
    return out


def softmax_rows(x, scale=1.0, out=None):
    rows, n = x.shape
    if out is None:
        out = torch.empty_like(x)
    _operands("softmax_rows", ("x", x, F16, None), ("out", out, F16, rows * n))
    _call("lgd_softmax_rows_f16", _p(x), _p(out), rows, n, float(scale), _stream())
    return out


def add(a, b, out=None):
    if out is None:
        out = torch.empty_like(a)
    _operands("add", ("a", a, F16, None), ("b", b, F16, a.numel()), ("out", out, F16, a.numel()))
    _prof("add_kernel", 6.0 * a.numel(), lambda: _call("lgd_add_f16", _p(a), _p(b), _p(out), a.numel(), _stream()))
    return out


def scale(x, alpha, out=None):
    if out is None:
        out = torch.empty_like(x)
    _operands("scale", ("x", x, F16, None), ("out", out, F16, x.numel()))
    _call("lgd_scale_f16", _p(x), _p(out), float(alpha), x.numel(), _stream())
    return out


def upsample2x_bwd(gy, B, H, W, C_, out=None):
    if out is None:
        out = torch.empty((B * H * W, C_), device=gy.device, dtype=F16)
    _operands("upsample2x_bwd", ("gy", gy, F16, 4 * B * H * W * C_), ("out", out, F16, B * H * W * C_))
    _prof("upsample2x_bwd_kernel", 2.0 * 5 * B * H * W * C_,
          lambda: _call("lgd_upsample2x_bwd_f16", _p(gy), _p(out), B, H, W, C_, _stream()))
    return out


def _step_operands(fn, eps, x, x_out, coef_table, cols, dyn, frozen_ref, mask, hist):
    """The operands the two fused sampler steps share: x (B, C, L, L), eps its CFG pair, the table [T][cols], the mask one
    plane per image, frozen_ref and hist whole (B, C, L, L) latents per step."""
    n = x.numel()
    if x.dim() != 4 or x.shape[2] != x.shape[3]:
        raise RuntimeError(f"{fn}: x {tuple(x.shape)} is not (B, C, L, L)")
    _operands(fn, ("eps", eps, F32, 2 * n), ("x", x, F32, None), ("x_out", x_out, F32, n), ("coef_table", coef_table, F32, None),
              ("dyn", dyn, torch.int32, None), ("frozen_ref", frozen_ref, F32, None), ("mask", mask, F32, x.shape[0] * x.shape[2] ** 2),
              ("hist", hist, F32, None))
    if coef_table.numel() % cols or dyn.numel() < 2:
        raise RuntimeError(f"{fn}: the table is not [T][{cols}] or dyn holds fewer than two entries")
    for name, t in (("frozen_ref", frozen_ref), ("hist", hist)):
        if t is not None and t.numel() % n:
            raise RuntimeError(f"{fn}: {name} holds {t.numel()} elements, no whole number of latents of {n}")


def cfg_ddim_step(eps, x, x_out, coef_table, dyn, *, frozen_ref=None, mask=None, hist=None):
    """dyn: device int32[2] = {step, frozen_steps}."""
    B, C_, L, _ = x.shape
    _step_operands("cfg_ddim_step", eps, x, x_out, coef_table, 4, dyn, frozen_ref, mask, hist)
    _prof("cfg_ddim_kernel", 4.0 * x.numel() * 6,
          lambda: _call("lgd_cfg_ddim_step_f32", _p(eps), _p(x), _p(x_out), _p(coef_table), _p(dyn),
                        _p(frozen_ref), _p(mask), _p(hist), B, C_, L * L, _stream()))
    return x_out


def cfg_multistep_step(eps, x, x_out, x0_prev, coef_table, dyn, *, frozen_ref=None, mask=None, hist=None):
    """CFG + one linear multistep update (DPM-Solver++ 2M); coef_table fp32 [T][8], see lgd_hip.h."""
    B, C_, L, _ = x.shape
    _step_operands("cfg_multistep_step", eps, x, x_out, coef_table, 8, dyn, frozen_ref, mask, hist)
    _operands("cfg_multistep_step", ("x0_prev", x0_prev, F32, x.numel()))
    _call("lgd_cfg_multistep_step_f32", _p(eps), _p(x), _p(x_out), _p(x0_prev), _p(coef_table), _p(dyn),
          _p(frozen_ref), _p(mask), _p(hist), B, C_, L * L, _stream())
    return x_out


def _at_least(fn, name, t, count):
    if t is not None and t.numel() < count:
        raise RuntimeError(f"{fn}: {name} holds {t.numel()} elements, the call addresses {count}")


def cfg_plms_step(eps, x, x_out, ets, cur_sample, coef_table, dyn, *, hist=None):
    """CFG + one PLMS evaluation (PNDMScheduler, skip_prk_steps); coef_table fp32 [E][16], ets fp32 [3, *x.shape],
    see lgd_hip.h."""
    if x.dim() != 4:
        raise RuntimeError(f"cfg_plms_step: x {tuple(x.shape)} is not (B, C, H, W)")
    B, C_, H, W = x.shape
    n = x.numel()
    _operands("cfg_plms_step", ("eps", eps, F32, 2 * n), ("x", x, F32, None), ("x_out", x_out, F32, n), ("ets", ets, F32, 3 * n),
              ("cur_sample", cur_sample, F32, n), ("coef_table", coef_table, F32, None), ("dyn", dyn, torch.int32, None),
              ("hist", hist, F32, None))
    if coef_table.numel() % 16 or dyn.numel() < 1:
        raise RuntimeError("cfg_plms_step: the table is not [E][16] or dyn is empty")
    if hist is not None and hist.numel() % n:
        raise RuntimeError(f"cfg_plms_step: hist holds {hist.numel()} elements, no whole number of latents of {n}")
    _prof("cfg_plms_kernel", 4.0 * x.numel() * 7,
          lambda: _call("lgd_cfg_plms_step_f32", _p(eps), _p(x), _p(x_out), _p(ets), _p(cur_sample), _p(coef_table),
                        _p(dyn), _p(hist), B, C_, H * W, _stream()))
    return x_out


def cfg_lms_step(eps, x, x_out, ring, coef_table, dyn, *, frozen_ref=None, mask=None, hist=None):
    """CFG + one step of the order-4 linear multistep sampler in sigma space (LMSDiscreteScheduler); coef_table fp32
    [T][16], ring fp32 [4, *x.shape], see lgd_hip.h."""
    _step_operands("cfg_lms_step", eps, x, x_out, coef_table, 16, dyn, frozen_ref, mask, hist)
    B, C_, L, _ = x.shape
    _operands("cfg_lms_step", ("ring", ring, F32, 4 * x.numel()))
    _prof("cfg_lms_kernel", 4.0 * x.numel() * 9,
          lambda: _call("lgd_cfg_lms_step_f32", _p(eps), _p(x), _p(x_out), _p(ring), _p(coef_table), _p(dyn),
                        _p(frozen_ref), _p(mask), _p(hist), B, C_, L * L, _stream()))
    return x_out


def _md_operands(fn, eps, x_in, latent, masks, coef_table, dyn, bg, noise, picks, hist, P, plane, bg_plane, n_picks,
                 n_steps, n_boot, prep):
    """The operands the two MultiDiffusion entry points share: eps the size of x_in (not read with prep), masks at least P
    planes, bg at least n_boot latents, picks at least n_picks indices, hist whole latents; plane = Hp * Wp elements."""
    n = latent.numel()
    _operands(fn, ("eps", None if prep else eps, F32, x_in.numel()), ("x_in", x_in, F32, None), ("latent", latent, F32, None),
              ("masks", masks, F32, None), ("coef_table", coef_table, F32, None), ("dyn", dyn, torch.int32, None),
              ("bg", bg, F32, None), ("noise", noise, F32, n), ("picks", picks, torch.int32, None), ("hist", hist, F32, None))
    if not prep and eps is None:
        raise RuntimeError(f"{fn}: eps is missing")
    _at_least(fn, "masks", masks, P * plane)
    _at_least(fn, "coef_table", coef_table, 4 * n_steps)
    _at_least(fn, "dyn", dyn, 1)
    if n_boot > 0 and P > 1:
        _at_least(fn, "bg", bg, n_boot * bg_plane)
        _at_least(fn, "picks", picks, n_picks)
    if hist is not None and hist.numel() % n:
        raise RuntimeError(f"{fn}: hist holds {hist.numel()} elements, no whole number of latents of {n}")


def multidiffusion_step(eps, x_in, latent, masks, coef_table, dyn, *, n_prompts, n_steps, bg=None, noise=None,
                        picks=None, n_boot=0, hist=None, prep=False):
    """One MultiDiffusion step (CFG + P DDIM steps + masked sum) and the next step's UNet input rows, or with prep=True
    only the input rows of step dyn[0] from `latent`; x_in / eps fp32 (2Pp, C, H, W), see lgd_hip.h."""
    if x_in.dim() != 4 or x_in.shape[0] % 2:
        raise RuntimeError(f"multidiffusion_step: x_in {tuple(x_in.shape)} is not (2 Pp, C, H, W)")
    Pp2, C_, H, W = x_in.shape
    P = int(n_prompts)
    if latent.numel() != C_ * H * W:
        raise RuntimeError(f"multidiffusion_step: latent {tuple(latent.shape)} is no row of x_in {tuple(x_in.shape)}")
    _md_operands("multidiffusion_step", eps, x_in, latent, masks, coef_table, dyn, bg, noise, picks, hist, P, H * W,
                 C_ * H * W, int(n_steps) * (P - 1), int(n_steps), int(n_boot), prep)
    _prof("multidiffusion_step_kernel", 4.0 * latent.numel() * (2 + (0 if prep else 3 * P) + Pp2),
          lambda: _call("lgd_multidiffusion_step_f32", _p(None if prep else eps), _p(x_in), _p(latent), _p(masks),
                        _p(bg), _p(noise), _p(picks), _p(coef_table), _p(dyn), _p(hist), P, Pp2 // 2, C_, H * W,
                        int(n_steps), int(n_boot), 1 if prep else 0, _stream()))
    return latent


def multidiffusion_views(eps, x_in, latent, value, count, masks, coef_table, dyn, *, n_prompts, rows_per_view, n_views,
                         v0, nv, n_steps, indep_uncond=True, normalization=False, bg=None, noise=None, picks=None,
                         n_boot=0, hist=None, prep=False):
    """MultiDiffusion over overlapping 64x64 views of the panorama `latent` (C, Hp, Wp) for the chunk of views
    [v0, v0 + nv): with prep=True the chunk's UNet input rows of step dyn[0], else the chunk's share of value / count
    and, behind the last view, the blended latent; x_in / eps fp32 (2 * nvc * rows_per_view, C, 64, 64), see lgd_hip.h."""
    if x_in.dim() != 4 or latent.dim() != 3:
        raise RuntimeError(f"multidiffusion_views: x_in {tuple(x_in.shape)}, latent {tuple(latent.shape)}: want 4 and 3 dimensions")
    rows, C_, L, _ = x_in.shape
    P, Pp = int(n_prompts), int(rows_per_view)
    _, Hp, Wp = latent.shape
    if L != 64 or rows % (2 * Pp) or tuple(x_in.shape[2:]) != (64, 64) or (eps is not None and eps.shape != x_in.shape):
        raise RuntimeError(f"multidiffusion_views: x_in {tuple(x_in.shape)} is not (2 * views * {Pp}, C, 64, 64)")
    if latent.shape[0] != C_:
        raise RuntimeError(f"multidiffusion_views: latent {tuple(latent.shape)} for x_in {tuple(x_in.shape)}")
    _md_operands("multidiffusion_views", eps, x_in, latent, masks, coef_table, dyn, bg, noise, picks, hist, P, Hp * Wp,
                 C_ * 4096, int(n_steps) * int(n_views) * (P - 1), int(n_steps), int(n_boot) if prep else 0, prep)
    _operands("multidiffusion_views", ("value", value, F32, latent.numel()), ("count", count, F32, latent.numel()))
    nvc = rows // (2 * Pp)
    nbytes = 4.0 * C_ * 4096 * nv * (1 + 2 * Pp) if prep else 4.0 * (C_ * 4096 * nv * 3 * P + latent.numel() * 6)
    _prof("multidiffusion_views_prep_kernel" if prep else "multidiffusion_views_accum_kernel", nbytes,
          lambda: _call("lgd_multidiffusion_views_f32", _p(None if prep else eps), _p(x_in), _p(latent), _p(value),
                        _p(count), _p(masks), _p(bg), _p(noise), _p(picks), _p(coef_table), _p(dyn), _p(hist), P, Pp,
                        C_, Hp, Wp, int(n_views), int(v0), int(nv), nvc, int(n_steps), int(n_boot),
                        1 if indep_uncond else 0, 1 if normalization else 0, 1 if prep else 0, _stream()))
    return latent


def axpy(g, x, coef_table, step_idx, col, active=None):
    per = x.numel() // x.shape[0] if active is not None else 0
    _operands("axpy", ("g", g, F32, x.numel()), ("x", x, F32, None), ("coef_table", coef_table, F32, None),
              ("step_idx", step_idx, torch.int32, None), ("active", active, F32, x.shape[0]))
    _prof("axpy_kernel", 12.0 * x.numel(),
          lambda: _call("lgd_axpy_f32", _p(g), _p(x), _p(coef_table), _p(step_idx), int(col), _p(active), per, x.numel(),
                        _stream()))


def scale_rows(x, out, table, dyn, col, reps=1):
    """out[r] = x * table[dyn[0]][col], r < reps (EulerDiscrete.scale_model_input for the CFG pair; lgd_hip.h)."""
    _operands("scale_rows", ("x", x, F32, None), ("out", out, F32, int(reps) * x.numel()), ("table", table, F32, None),
              ("dyn", dyn, torch.int32, None))
    _call("lgd_scale_rows_f32", _p(x), _p(out), _p(table), _p(dyn), int(table.shape[1]), int(col), x.numel(), int(reps),
          _stream())
    return out


def select_row(table, idx, out):
    _operands("select_row", ("table", table, F32, None), ("idx", idx, torch.int32, None), ("out", out, F32, None))
    if table.numel() % max(out.numel(), 1):
        raise RuntimeError(f"select_row: a table of {table.numel()} elements has no rows of {out.numel()}")
    _prof("select_row_kernel", 8.0 * out.numel(),
          lambda: _call("lgd_select_row_f32", _p(table), _p(idx), _p(out), out.numel(), _stream()))


def ca_energy(map_ptrs, gmap_ptrs, map_hw, items, coefs, masks, refs, refs_step_stride, dyn, groups, n_groups,
              n_items, H, T, max_hw, partial, loss, grad_scale=1.0, n_samples=1):
    """Cross-attention energy + map gradients (lgd_ca_energy_f32, include/lgd_hip.h).  With n_items = 0 the tables are
    placeholders of any size; otherwise their element counts follow from the integer arguments."""
    some = n_items > 0
    I32, I64 = torch.int32, torch.int64
    if refs is not None and dyn is None:
        raise RuntimeError("ca_energy: refs without dyn (the step slice of refs is chosen by dyn[0])")
    _operands("ca_energy", ("map_ptrs", map_ptrs, I64, None), ("gmap_ptrs", gmap_ptrs, I64, map_ptrs.numel()),
              ("map_hw", map_hw, I32, map_ptrs.numel()), ("items", items, I32, 8 * n_items if some else None),
              ("coefs", coefs, F32, 4 * n_items if some else None), ("masks", masks, F32, None), ("refs", refs, F32, None),
              ("dyn", dyn, I32, None), ("groups", groups, I32, 2 * n_groups if some else None),
              ("partial", partial, F32, n_items * H if some else None), ("loss", loss, F32, n_samples))
    if masks.numel() % max(int(max_hw), 1):
        raise RuntimeError(f"ca_energy: masks of {masks.numel()} elements are no rows of max_hw = {max_hw}")
    if dyn is not None and dyn.numel() < 1:
        raise RuntimeError("ca_energy: dyn holds no element, the kernel reads dyn[0]")
    if refs is not None and refs.numel() < int(H) * int(max_hw):
        raise RuntimeError(f"ca_energy: refs holds {refs.numel()} elements, one reference is [H = {H}][max_hw = {max_hw}]")
    tensors = [t for t in (map_ptrs, gmap_ptrs, map_hw, items, coefs, masks, refs, dyn, groups, partial, loss) if t is not None]
    if len({t.device for t in tensors}) != 1:
        raise RuntimeError(f"ca_energy: operands on different devices: {sorted({str(t.device) for t in tensors})}")
    _prof("ca_energy_kernel + energy_sum_kernel", 4.0 * n_groups * H * max_hw * 2,
          lambda: _call("lgd_ca_energy_f32", _p(map_ptrs), _p(gmap_ptrs), _p(map_hw), _p(items), _p(coefs),
                        _p(masks), _p(refs), int(refs_step_stride), _p(dyn), _p(groups), n_groups, n_items, n_samples, H, T,
                        max_hw, float(grad_scale), _p(partial), _p(loss), _stream()))


def boxdiff_energy(map_ptrs, gmap_ptrs, n_maps, side, items, masks, smooth, groups, n_samples, max_items, H, T,
                   loss_scale, grad_scale, loss):
    """BoxDiff energy + map gradients (lgd_boxdiff_energy_f32, include/lgd_hip.h; utils/boxdiff.py:20-196)."""
    I32, I64 = torch.int32, torch.int64
    _operands("boxdiff_energy", ("map_ptrs", map_ptrs, I64, int(n_maps)), ("gmap_ptrs", gmap_ptrs, I64, int(n_maps)),
              ("items", items, I32, None), ("masks", masks, F32, None), ("smooth", smooth, F32, 9),
              ("groups", groups, I32, 2 * int(n_samples)), ("loss", loss, F32, int(n_samples)))
    if items.numel() % 8 or masks.numel() % max(3 * int(side) * int(side), 1):
        raise RuntimeError(f"boxdiff_energy: items of {items.numel()} elements are no [n][8] table, or masks of {masks.numel()} "
                           f"no [n][3][{side}*{side}] table")
    tensors = [t for t in (map_ptrs, gmap_ptrs, items, masks, smooth, groups, loss) if t is not None]
    if len({t.device for t in tensors}) != 1:
        raise RuntimeError(f"boxdiff_energy: operands on different devices: {sorted({str(t.device) for t in tensors})}")
    _prof("boxdiff_energy_kernel", 4.0 * 2 * n_maps * n_samples * H * side * side * T * 2,
          lambda: _call("lgd_boxdiff_energy_f32", _p(map_ptrs), _p(gmap_ptrs), int(n_maps), int(side), _p(items), _p(masks),
                        _p(smooth), _p(groups), int(n_samples), int(max_items), int(H), int(T), float(loss_scale),
                        float(grad_scale), _p(loss), _stream()))


# ---------------------------------------------------------------------------------------------
# detection tail of the stage-2 evaluator (csrc/detect.hip)
# ---------------------------------------------------------------------------------------------
def owl_heads(class_embeds, query_embeds, query_mask, shift, scale_raw, box_raw, box_bias, B, P, *, logits=None,
              pred_boxes=None):
    """Tail of OWL-ViT's class and box heads (lgd_owl_heads_f32).  class_embeds fp16 [B*P, >=D] (row stride = its
    stride(0)), query_embeds fp32 [B, Q, D], query_mask int32 [B, Q] or None, shift / scale_raw fp32 views of B*P
    elements with a common stride, box_raw fp16 / fp32 [B*P, 4], box_bias fp32 [P, 4] ->
    (logits fp32 [B, P, Q], pred_boxes fp32 [B, P, 4])."""
    _, Q, D = query_embeds.shape
    dev = class_embeds.device
    if logits is None:
        logits = torch.empty((B, P, Q), device=dev, dtype=F32)
    if pred_boxes is None:
        pred_boxes = torch.empty((B, P, 4), device=dev, dtype=F32)
    if class_embeds.dtype != F16 or query_embeds.dtype != F32 or shift.dtype != F32 or scale_raw.dtype != F32:
        raise RuntimeError("owl_heads: class_embeds fp16; query_embeds, shift and scale_raw fp32")
    if shift.stride(0) != scale_raw.stride(0) or not query_embeds.is_contiguous() or not box_raw.is_contiguous():
        raise RuntimeError("owl_heads: shift / scale_raw share a stride; query_embeds and box_raw are contiguous")
    _call("lgd_owl_heads_f32", _p(class_embeds), class_embeds.stride(0), _p(query_embeds), _p(query_mask), _p(shift),
          _p(scale_raw), shift.stride(0), _p(box_raw), 1 if box_raw.dtype == F32 else 0, _p(box_bias), _p(logits),
          _p(pred_boxes), B, P, Q, D, _stream())
    return logits, pred_boxes


def detect_nms(scores_or_logits, boxes, *, labels=None, counts=None, score_threshold=0.1, nms_threshold=0.5,
               class_aware=False, out=None):
    """post_process + score filter + greedy NMS (lgd_detect_nms_f32).  3-D `scores_or_logits` [B, P, Q] with cxcywh
    `boxes` is mode 0 (from the model); 2-D scores [B, P] with int32 labels, xyxy boxes and per-image int32 counts is
    mode 1 (candidates).  Returns (boxes [B, P, 4], scores [B, P], labels, index int32 [B, P], count int32 [B]) in
    picking order; rows past an image's count are not written.  `out`: that tuple, preallocated."""
    mode = 0 if scores_or_logits.dim() == 3 else 1
    B, P = scores_or_logits.shape[:2]
    Q = scores_or_logits.shape[2] if mode == 0 else 0
    dev = scores_or_logits.device
    if scores_or_logits.dtype != F32 or boxes.dtype != F32 or not scores_or_logits.is_contiguous() or not boxes.is_contiguous():
        raise RuntimeError("detect_nms: contiguous fp32 scores / logits and boxes")
    for t in (labels, counts):
        if t is not None and (t.dtype != torch.int32 or not t.is_contiguous()):
            raise RuntimeError("detect_nms: labels and counts are contiguous int32")
    if out is None:
        out = (torch.zeros((B, P, 4), device=dev, dtype=F32), torch.zeros((B, P), device=dev, dtype=F32),
               torch.zeros((B, P), device=dev, dtype=torch.int32), torch.zeros((B, P), device=dev, dtype=torch.int32),
               torch.zeros((B,), device=dev, dtype=torch.int32))
    _call("lgd_detect_nms_f32", mode, _p(scores_or_logits), _p(boxes), _p(labels), _p(counts), B, P, Q,
          float(score_threshold), float(nms_threshold), 1 if class_aware else 0, *(_p(t) for t in out), _stream())
    return out


# ---------------------------------------------------------------------------------------------
# safety checker of the `sd` baseline (csrc/safety.hip)
# ---------------------------------------------------------------------------------------------
def safety_head(embeds, special, special_w, concepts, concept_w, *, scores=None, flags=None):
    """Tail of StableDiffusionSafetyChecker.forward (lgd_safety_head_f32).  embeds fp32 [B, >=D] (row stride = its
    stride(0), D columns read), special fp32 [n_special, D] with special_w [n_special] (None, None: no special rows),
    concepts fp32 [n_concepts, D] with concept_w [n_concepts] -> (scores fp32 [B, n_special + n_concepts], special rows
    first; flags int32 [B, 2] = (has_nsfw, a special row hit))."""
    if embeds.dim() != 2 or concepts.dim() != 2 or embeds.stride(1) != 1:
        raise RuntimeError("safety_head: embeds [B, D] with unit column stride and concepts [n_concepts, D]")
    if (special is None) != (special_w is None):
        raise RuntimeError("safety_head: special and special_w go together")
    B, D = embeds.shape[0], concepts.shape[1]
    ns, nc = (0 if special is None else special.shape[0]), concepts.shape[0]
    if embeds.dtype != F32 or embeds.shape[1] < D or (B > 1 and embeds.stride(0) < D):
        raise RuntimeError(f"safety_head: embeds is fp32 with at least D = {D} columns per row")
    dev = embeds.device
    if scores is None:
        scores = torch.empty((B, ns + nc), device=dev, dtype=F32)
    if flags is None:
        flags = torch.empty((B, 2), device=dev, dtype=torch.int32)
    _operands("safety_head", ("special", special, F32, ns * D), ("special_w", special_w, F32, ns),
              ("concepts", concepts, F32, nc * D), ("concept_w", concept_w, F32, nc),
              ("scores", scores, F32, B * (ns + nc)), ("flags", flags, torch.int32, B * 2))
    if len({t.device for t in (embeds, special, special_w, concepts, concept_w, scores, flags) if t is not None}) != 1:
        raise RuntimeError("safety_head: operands on different devices")
    _call("lgd_safety_head_f32", _p(embeds), embeds.stride(0) if B > 1 else max(embeds.stride(0), D), _p(special),
          _p(special_w), ns, _p(concepts), _p(concept_w), nc, _p(scores), _p(flags), B, D, _stream())
    return scores, flags


def blank_flagged(images, flags):
    """Zeroes image n of the contiguous uint8 batch `images` (N, ...) in place iff flags[n] != 0 (lgd_blank_flagged_u8).
    flags: int32, one element per image at a constant stride, e.g. column 0 of safety_head's flags.  Returns images."""
    if images.dtype != torch.uint8 or not images.is_contiguous() or images.dim() < 1 or images.numel() == 0:
        raise RuntimeError("blank_flagged: images is a contiguous, non-empty uint8 batch")
    N = images.shape[0]
    if flags.dtype != torch.int32 or flags.dim() != 1 or flags.shape[0] != N or (N > 1 and flags.stride(0) < 1):
        raise RuntimeError(f"blank_flagged: flags is an int32 vector of {N} elements (a strided view is fine)")
    if flags.device != images.device:
        raise RuntimeError("blank_flagged: operands on different devices")
    _call("lgd_blank_flagged_u8", _p(images), images.numel() // N, _p(flags), flags.stride(0) if N > 1 else 1, N, _stream())
    return images


# ---------------------------------------------------------------------------------------------
# mask refinement around the SAM network (csrc/sam_tail.hip)
# ---------------------------------------------------------------------------------------------
def sam_mask_tail(logits, iou, geom, target, grid, coarse, below_conf, below_iou, *, want_cand=True):
    """SAM's low-resolution logits -> the selected latent-grid mask of every item (lgd_sam_mask_tail_f32).  logits fp32
    [N, K, S, S], iou fp32 [N, K], geom int32 [N, 4] = (h, w, nh, nw), coarse uint8 / bool [N, hc, wc], grid = (H, W) ->
    (mask uint8 [N, H, W], conf fp32 [N], stats int32 [N, 1 + 3K], cand uint8 [N, K, H, W] or None)."""
    N, K, S = logits.shape[:3]
    H, W = int(grid[0]), int(grid[1])
    dev = logits.device
    if coarse.dtype == torch.bool:
        coarse = coarse.view(torch.uint8)
    if (logits.dtype != F32 or iou.dtype != F32 or geom.dtype != torch.int32 or coarse.dtype != torch.uint8
            or logits.dim() != 4 or logits.shape[3] != S or tuple(iou.shape) != (N, K) or tuple(geom.shape) != (N, 4)
            or coarse.dim() != 3 or coarse.shape[0] != N):
        raise RuntimeError("sam_mask_tail: logits fp32 [N,K,S,S], iou fp32 [N,K], geom int32 [N,4], coarse uint8 [N,hc,wc]")
    if not (logits.is_contiguous() and iou.is_contiguous() and geom.is_contiguous() and coarse.is_contiguous()):
        raise RuntimeError("sam_mask_tail: contiguous operands")
    mask = torch.empty((N, H, W), device=dev, dtype=torch.uint8)
    conf = torch.empty((N,), device=dev, dtype=F32)
    stats = torch.empty((N, 1 + 3 * K), device=dev, dtype=torch.int32)
    cand = torch.empty((N, K, H, W), device=dev, dtype=torch.uint8) if want_cand else None
    ws = torch.empty((3 * N * K * H + (0 if want_cand else (N * K * H * W + 3) // 4),), device=dev, dtype=torch.int32)
    _call("lgd_sam_mask_tail_f32", _p(logits), _p(iou), _p(geom), _p(coarse), N, K, S, int(target), H, W,
          coarse.shape[1], coarse.shape[2], float(below_conf), float(below_iou), _p(cand), _p(mask), _p(conf), _p(stats),
          _p(ws), _stream())
    return mask, conf, stats, cand


def sam_attn_prompt(attn, sigma, mask_th, up_w, up_h, *, want_smooth=False):
    """LMD's point prompt and coarse mask from the object token's attention maps (lgd_sam_attn_prompt_f32).  attn fp32
    [N, hm, wm] -> (coarse uint8 [N, hm, wm], points fp32 [N, 2] = (peak_x * up_h, peak_y * up_w), smoothed map or None)."""
    if attn.dtype != F32 or attn.dim() != 3 or not attn.is_contiguous():
        raise RuntimeError("sam_attn_prompt: attn is a contiguous fp32 [N, hm, wm] tensor")
    N, hm, wm = attn.shape
    coarse = torch.empty((N, hm, wm), device=attn.device, dtype=torch.uint8)
    points = torch.empty((N, 2), device=attn.device, dtype=F32)
    smooth = torch.empty_like(attn) if want_smooth else None
    _call("lgd_sam_attn_prompt_f32", _p(attn), N, hm, wm, float(sigma), float(mask_th), int(up_w), int(up_h), _p(coarse),
          _p(points), _p(smooth), _stream())
    return coarse, points, smooth


def sam_attn_box_prompt(attn, sigma, mask_th, n_open, up_w, up_h, *, want_smooth=False):
    """LMD's box prompt and opened coarse mask from the object token's attention maps (lgd_sam_attn_box_prompt_f32).  attn
    fp32 [N, hm, wm] -> (coarse uint8 [N, hm, wm] after n_open erosions and n_open dilations, boxes fp32 [N, 4] =
    (xmin * up_w, ymin * up_h, xmax * up_w, ymax * up_h) of the mask's bounding box grown by one, empty int32 [N] = 1
    where the opened mask has no pixel (its box is 0, 0, 0, 0)[, smoothed map]).  Nothing is read back."""
    if attn.dtype != F32 or attn.dim() != 3 or not attn.is_contiguous():
        raise RuntimeError("sam_attn_box_prompt: attn is a contiguous fp32 [N, hm, wm] tensor")
    N, hm, wm = attn.shape
    coarse = torch.empty((N, hm, wm), device=attn.device, dtype=torch.uint8)
    boxes = torch.empty((N, 4), device=attn.device, dtype=F32)
    empty = torch.empty((N,), device=attn.device, dtype=torch.int32)
    smooth = torch.empty_like(attn) if want_smooth else None
    _call("lgd_sam_attn_box_prompt_f32", _p(attn), N, hm, wm, float(sigma), float(mask_th), int(n_open), int(up_w),
          int(up_h), _p(coarse), _p(boxes), _p(empty), _p(smooth), _stream())
    return (coarse, boxes, empty, smooth) if want_smooth else (coarse, boxes, empty)


# ---------------------------------------------------------------------------------------------
# the hand-off between the two stages of LMD / LMD+ (csrc/handoff.hip; the tables are packed by lgd_amd.handoff)
# ---------------------------------------------------------------------------------------------
HANDOFF_PLAN = 8            # int32 per plan row: ox, oy, area, x0, y0, x1, y1, empty


def _i32(t, name, shape=None):
    if t.dtype != torch.int32 or not t.is_contiguous() or (shape is not None and tuple(t.shape) != tuple(shape)):
        raise RuntimeError(f"{name}: a contiguous int32 tensor" + (f" of shape {tuple(shape)}" if shape else ""))
    return t


def handoff_place(masks, targets, seg, max_boxes, *, align, horizontal_shift_only):
    """Per-box placement of a batch of layouts (lgd_handoff_place).  masks uint8 / bool [NB, L, L], targets fp64 [NB, 4],
    seg int32 [NL + 1], max_boxes = the largest box count of a layout (host int) -> (plan int32 [NB, 8], win int32
    [NL, 2, L, L] = the owner maps win_mask, win_box)."""
    if masks.dtype == torch.bool:
        masks = masks.view(torch.uint8)
    NB, NL = targets.shape[0], seg.shape[0] - 1
    if masks.dtype != torch.uint8 or masks.dim() != 3 or masks.shape[0] != NB or masks.shape[1] != masks.shape[2] \
            or not masks.is_contiguous():
        raise RuntimeError("handoff_place: masks is a contiguous uint8 [NB, L, L] tensor")
    if targets.dtype != torch.float64 or tuple(targets.shape) != (NB, 4) or not targets.is_contiguous():
        raise RuntimeError("handoff_place: targets is a contiguous fp64 [NB, 4] tensor")
    _i32(seg, "handoff_place: seg")
    L, dev = masks.shape[1], seg.device
    plan = torch.empty((NB, HANDOFF_PLAN), device=dev, dtype=torch.int32)
    win = torch.empty((NL, 2, L, L), device=dev, dtype=torch.int32)
    _call("lgd_handoff_place", _p(masks), _p(targets), _p(seg), NL, NB, int(max_boxes), L, 1 if align else 0,
          1 if horizontal_shift_only else 0, _p(plan), _p(win), _stream())
    return plan, win


def handoff_compose(plan, win, seg, hist, bg, steps, *, rows=None):
    """Composition of every layout from the placement (lgd_handoff_compose_f32).  hist int64 [NB, 2] = (address, step
    stride in elements) of each box's fp32 history, bg fp32 [NL, C, L, L] -> (composed fp32 [NL, steps + 1, C, L, L],
    fg_idx int64 [NL, L, L], aligned fp32 [NB, rows, C, L, L] or None).  rows: also write the aligned histories, that many
    steps of each."""
    NL, C, L = bg.shape[0], bg.shape[1], bg.shape[2]
    NB = plan.shape[0]
    if bg.dtype != F32 or bg.dim() != 4 or bg.shape[3] != L or not bg.is_contiguous():
        raise RuntimeError("handoff_compose: bg is a contiguous fp32 [NL, C, L, L] tensor")
    if hist.dtype != torch.int64 or hist.dim() != 2 or hist.shape[0] < NB or hist.shape[1] != 2 or not hist.is_contiguous():
        raise RuntimeError("handoff_compose: hist is a contiguous int64 [NB, 2] tensor")
    _i32(plan, "handoff_compose: plan"), _i32(win, "handoff_compose: win", (NL, 2, L, L)), _i32(seg, "handoff_compose: seg", (NL + 1,))
    dev = bg.device
    composed = torch.empty((NL, int(steps) + 1, C, L, L), device=dev, dtype=F32)
    fg_idx = torch.empty((NL, L, L), device=dev, dtype=torch.int64)
    aligned = torch.empty((NB, int(rows), C, L, L), device=dev, dtype=F32) if rows is not None and NB else None
    _call("lgd_handoff_compose_f32", _p(plan), _p(win), _p(seg), _p(hist), _p(bg), NL, NB, int(steps), C, L,
          int(rows) if aligned is not None else 0, _p(composed), _p(fg_idx), _p(aligned), _stream())
    return composed, fg_idx, aligned


def handoff_ref_maps(plan, seg, lay_of, maps, T, heads, max_hw, L):
    """The reference-map tensors of every layout (lgd_handoff_ref_maps_f32).  maps int64 [NB, NK, 3] = (address, rows,
    side) of each saved map, lay_of int32 [NB] -> one flat fp32 buffer; layout l's [T, n_boxes, NK, heads, max_hw] block
    starts at seg[l] * T * NK * heads * max_hw."""
    NB, NK = maps.shape[0], maps.shape[1]
    if maps.dtype != torch.int64 or maps.dim() != 3 or maps.shape[2] != 3 or not maps.is_contiguous():
        raise RuntimeError("handoff_ref_maps: maps is a contiguous int64 [NB, NK, 3] tensor")
    _i32(plan, "handoff_ref_maps: plan", (NB, HANDOFF_PLAN)), _i32(seg, "handoff_ref_maps: seg"), _i32(lay_of, "handoff_ref_maps: lay_of", (NB,))
    out = torch.empty((NB * int(T) * NK * int(heads) * int(max_hw),), device=plan.device, dtype=F32)
    if NB:
        _call("lgd_handoff_ref_maps_f32", _p(plan), _p(seg), _p(lay_of), _p(maps), NB, int(T), NK, int(heads), int(max_hw),
              int(L), _p(out), _stream())
    return out


# ---------------------------------------------------------------------------------------------
# Pillow's Image.resize on the device (csrc/resample.hip)
# ---------------------------------------------------------------------------------------------
FILTERS = {"lanczos": 1, "bilinear": 2, "bicubic": 3}       # Pillow's Image.Resampling codes = LGD_FILTER_*
RESAMPLE_FORMS = {"u8": 0, "affine": 1, "unit": 2}           # LGD_RESAMPLE_*
_RESAMPLE_TABLES = {}


def resample_filter(filter) -> int:
    """A filter name, a Pillow Image.Resampling member or its integer code -> the LGD_FILTER_* code."""
    code = FILTERS.get(filter.lower()) if isinstance(filter, str) else int(filter)
    if code not in FILTERS.values():
        raise RuntimeError(f"resample: filter {filter!r} is none of {sorted(FILTERS)} (Pillow codes 1, 2, 3)")
    return code


def resample_plan(n_in: int, n_out: int, filter):
    """The tables of one axis as the library's host function makes them (lgd_resample_plan; no GPU needed): (coef int32
    [n_out, width], bounds int32 [n_out, 2] = (first input index, taps), width) as host tensors."""
    lib = _lib.load()
    code = resample_filter(filter)
    width = C.c_int(0)
    _lib.check(lib.lgd_resample_plan(int(n_in), int(n_out), code, None, None, C.byref(width)), "lgd_resample_plan")
    coef = torch.empty((int(n_out), width.value), dtype=torch.int32)
    bounds = torch.empty((int(n_out), 2), dtype=torch.int32)
    _lib.check(lib.lgd_resample_plan(int(n_in), int(n_out), code, _p(coef), _p(bounds), None), "lgd_resample_plan")
    return coef, bounds, width.value


def resample_tables(n_in: int, n_out: int, filter, device):
    """resample_plan's tables on `device`, uploaded once per (n_in, n_out, filter): a launch that finds them makes no
    host -> device copy and can be captured."""
    key = (str(torch.device(device)), int(n_in), int(n_out), resample_filter(filter))
    if key not in _RESAMPLE_TABLES:
        coef, bounds, width = resample_plan(n_in, n_out, filter)
        _RESAMPLE_TABLES[key] = (coef.to(device), bounds.to(device), width)
    return _RESAMPLE_TABLES[key]


def resample_u8(images, size, filter, form="u8", *, dtype=None, rescale=1.0 / 255.0, mean=(0.0, 0.0, 0.0),
                std=(1.0, 1.0, 1.0), out=None, scratch=None, stream=None, canvas=None, pad=0.0):
    """PIL.Image.resize of a uint8 (N, h, w, 3) batch on the device, bit for bit (lgd_resample_u8).  size = (H, W);
    filter: "bilinear" / "bicubic" / "lanczos" or Pillow's code.  form "u8" -> uint8 (N, H, W, 3); "affine" ->
    (v * rescale - mean[c]) / std[c] and "unit" -> v / 255 * 2 - 1, both (N, 3, H, W) in `dtype` (fp32, the default, or
    fp16).  scratch: uint8, N * h * W * 3 elements, needed when both axes change size (allocated when left out).
    canvas = (CH, CW): the result has CH x CW in place of H x W, the resized image at its top left and `pad` (in output
    units; an integral byte for "u8") everywhere else, written by the last resize pass itself
    (lgd_resample_canvas_u8); None: the dense call, `pad` not read."""
    if images.dim() != 4 or images.shape[3] != 3:
        raise RuntimeError(f"resample_u8: images is a (N, h, w, 3) batch, got shape {tuple(images.shape)}")
    if form not in RESAMPLE_FORMS:
        raise RuntimeError(f"resample_u8: form {form!r} is none of {sorted(RESAMPLE_FORMS)}")
    N, h, w, _ = images.shape
    H, W = int(size[0]), int(size[1])
    code = resample_filter(filter)
    CH, CW = (H, W) if canvas is None else (int(canvas[0]), int(canvas[1]))
    if CH < H or CW < W:
        raise RuntimeError(f"resample_u8: canvas {CH} x {CW} does not hold the {H} x {W} image")
    if form == "u8":
        if dtype not in (None, torch.uint8):
            raise RuntimeError("resample_u8: form 'u8' writes uint8")
        dtype, shape = torch.uint8, (N, CH, CW, 3)
    else:
        dtype = F32 if dtype is None else dtype
        if dtype not in (F32, F16):
            raise RuntimeError(f"resample_u8: form {form!r} writes fp32 or fp16, not {dtype}")
        shape = (N, 3, CH, CW)
    if len(mean) != 3 or len(std) != 3:
        raise RuntimeError("resample_u8: mean and std hold one value per channel")
    if min(N, h, w, H, W) <= 0:
        raise RuntimeError(f"resample_u8: empty operand ({N} images of {h} x {w} -> {H} x {W})")
    dev = images.device
    if out is None:
        out = torch.empty(shape, device=dev, dtype=dtype)
    elif tuple(out.shape) != shape:
        raise RuntimeError(f"resample_u8: out has shape {tuple(out.shape)}, the call writes {shape}")
    both = h != H and w != W
    if both and scratch is None:
        scratch = torch.empty((N * h * W * 3,), device=dev, dtype=torch.uint8)
    _operands("resample_u8", ("images", images, torch.uint8, None), ("out", out, dtype, N * CH * CW * 3),
              ("scratch", scratch if both else None, torch.uint8, N * h * W * 3))
    cx, bx, wx = resample_tables(w, W, code, dev) if w != W else (None, None, 0)
    cy, by, wy = resample_tables(h, H, code, dev) if h != H else (None, None, 0)
    st = _stream() if stream is None else C.c_void_p(stream.cuda_stream)
    args = (_p(images), N, h, w, H, W, code, _p(cx), _p(bx), wx, W, _p(cy), _p(by), wy, H,
            _p(scratch if both else None), RESAMPLE_FORMS[form], 1 if dtype == F16 else 0, float(rescale),
            *(float(v) for v in mean), *(float(v) for v in std), _p(out))
    if canvas is None:
        _call("lgd_resample_u8", *args, st)
    else:
        _call("lgd_resample_canvas_u8", *args, CH, CW, float(pad), st)
    return out

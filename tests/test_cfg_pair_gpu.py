"""CFG pair modes (LgdGemmDesc.pair, lgd_attn_fwd_pair_f16, lgd_groupnorm_pair_f16, lgd_layernorm_pair_f16, Plan.pair_shared):
a classifier-free-guidance batch [uncond halves; cond halves] holds the same latents in both halves, so every op in front
of the first text / grounding-token read is computed for the first half only and — where a later op reads all rows —
stored twice.  Every comparison here is torch.equal against the SAME launch with pair = 0 on inputs whose two halves are
identical: the pair launch runs the kernel, tile and split the full launch runs, over half the grid."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lgd_amd  # noqa: E402,F401
from lgd_amd import _lib, ops, weights  # noqa: E402
from lgd_amd._lib import EPI_GEGLU, EPI_RES_F32, PAIR_DUP, PAIR_HALF  # noqa: E402
from lgd_amd.unet import UNetEngine  # noqa: E402

gpu = pytest.mark.gpu
F16, F32 = torch.float16, torch.float32
GOLD = os.path.join(ROOT, "tests", "golden")
SENTINEL = 123.0


def twice(t):
    """[t; t]: a batch whose two halves are identical."""
    return torch.cat([t, t]).contiguous()


def rnd(shape, dev, seed, scale=1.0, dtype=F16):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dev, dtype)


def check_pair(run, out, half_rows):
    """run(pair) launches into `out` (rows = first dim).  Full launch = reference; HALF leaves the second half of a
    pre-filled output untouched, DUP reproduces all of it."""
    out.fill_(SENTINEL)
    run(0)
    ref = out.clone()
    assert not torch.equal(ref, torch.full_like(ref, SENTINEL))
    assert torch.equal(ref[:half_rows], ref[half_rows:]), "identical halves in, identical halves out"
    out.fill_(SENTINEL)
    run(PAIR_DUP)
    assert torch.equal(out, ref), "dup mode differs from the full launch"
    out.fill_(SENTINEL)
    run(PAIR_HALF)
    assert torch.equal(out[:half_rows], ref[:half_rows]), "half mode differs from the full launch"
    assert torch.equal(out[half_rows:], torch.full_like(out[half_rows:], SENTINEL)), "half mode wrote the second half"


# ---- GEMM ------------------------------------------------------------------------------------------------------------
def gemm_case(dev, tile, M, N, K, *, res=None, geglu=False, rownorm=False, conv=None, seed=0):
    h = M // 2
    a = twice(rnd((h, K if conv is None else conv["C"]), dev, seed, 0.5))
    w = rnd((N, K), dev, seed + 1, K ** -0.5)
    bias = rnd((N,), dev, seed + 2, 0.1, F32)
    n_out = N // 2 if geglu else N
    out = torch.empty((M, n_out), device=dev, dtype=F16)
    kw = dict(bias=bias, splits=1, tile=tile, epi=EPI_GEGLU if geglu else 0)
    if res == "f16":
        r = twice(rnd((h, n_out), dev, seed + 3))
        kw.update(res=r, ldr=n_out)
    elif res == "f32":
        r = twice(rnd((h, n_out), dev, seed + 3, dtype=F32))
        kw.update(res=r, ldr=n_out)
        kw["epi"] |= EPI_RES_F32
    if rownorm:
        kw.update(rowstat=ops.layernorm_stats(a, K), colsum=w.float().sum(1).contiguous())
    if conv is not None:
        s, C = conv["side"], conv["C"]
        kw.update(c0=C, lda0=C, taps=9, hin=s, win=s, hout=s, wout=s)
    d = ops.gemm_desc(a, w, out, M, N, K, **kw)
    assert d.tile == tile and d.splits == 1
    key = ops.shape_key(d)

    def run(pair):
        assert ops.gemm_set_pair(d, pair), "the library refuses the pair descriptor"
        assert ops.shape_key(d) == key and d.tile == tile and d.splits == 1 and d.M == M    # the descriptor stays the full one
        ops.gemm_launch(d)
        torch.cuda.synchronize()
    check_pair(run, out, h)


@gpu
def test_gemm_tile47_fp16_residual(dev):
    gemm_case(dev, 47, 1024, 320, 320, res="f16")


@gpu
def test_gemm_tile47_rownorm(dev):
    gemm_case(dev, 47, 1024, 320, 320, rownorm=True, seed=10)


@gpu
def test_gemm_tile46_geglu(dev):
    gemm_case(dev, 46, 512, 512, 320, geglu=True, seed=20)


@gpu
@pytest.mark.parametrize("tile", [33, 37])
def test_gemm_pipe_tiles_half_not_a_tile_multiple(dev, tile):
    """M / 2 = 384 is not a multiple of the 256-row tile of code 33: the last row tile of the half is masked."""
    gemm_case(dev, tile, 768, 320, 640, res="f16", seed=30)


@gpu
def test_gemm_register_epilogue_fp32_residual(dev):
    """Tile 17 leaves through the register epilogue (8-byte stores); M / 2 = 192 is not a multiple of its 128 rows."""
    gemm_case(dev, 17, 384, 256, 192, res="f32", seed=40)


@gpu
def test_conv3x3_tile47(dev):
    """Rows are image-major: M / 2 = one whole 16x16 image; its bottom edge must not see the next image."""
    gemm_case(dev, 47, 2 * 256, 320, 9 * 320, conv=dict(side=16, C=320), res="f16", seed=50)


def _host_desc(splits, pair, M=1024):
    """A descriptor lgd_gemm_check can judge without a GPU: pointers count for NULL-ness and alignment only."""
    d = _lib.LgdGemmDesc()
    d.a0, d.w, d.c, d.ws = 0x10000, 0x20000, 0x30000, 0x40000
    d.M, d.N, d.K = M, 320, 640
    d.c0, d.c1, d.taps = 640, 0, 1
    d.lda0, d.ldw, d.ldc = 640, 640, 320
    d.nb_o = d.nb_i = 1
    d.alpha, d.splits, d.tile, d.pair = 1.0, splits, 37, pair
    return d


def test_gemm_check_refuses_pair_with_split_k():
    """Host only (lgd_gemm_check makes no HIP call): runs without a GPU too."""
    lib = _lib.load()
    chk = lambda d: lib.lgd_gemm_check(ctypes.byref(d))
    assert chk(_host_desc(1, 0)) == 0 and chk(_host_desc(2, 0)) == 0
    for pair in (PAIR_HALF, PAIR_DUP):
        assert chk(_host_desc(1, pair)) == 0
        assert chk(_host_desc(2, pair)) != 0                    # split-K
        assert chk(_host_desc(1, pair, M=1023)) != 0            # odd M
        d = _host_desc(1, pair)
        d.nb_i = 2
        assert chk(d) != 0                                      # batched
    assert chk(_host_desc(1, 3)) != 0                           # not a mode


# ---- attention -------------------------------------------------------------------------------------------------------
def attn_case(dev, d, Sq, Sk, *, lse=False, options=(), seed=0):
    B, H = 2, 2
    C = H * d
    q = twice(rnd((1, Sq, C), dev, seed))
    k = twice(rnd((1, Sk, C), dev, seed + 1))
    v = twice(rnd((1, Sk, C), dev, seed + 2))
    o = torch.empty((B, Sq, C), device=dev, dtype=F16)
    ls = torch.empty((B, H, Sq), device=dev, dtype=F32) if lse else None
    for name, val in options:
        ops.set_option(name, val)
    try:
        def run(pair):
            if ls is not None:
                ls.fill_(SENTINEL)
            ops.attn_fwd(q, k, v, o, B, H, Sq, Sk, d, d ** -0.5, lse=ls, pair=pair)
            torch.cuda.synchronize()
            run.lse[pair] = None if ls is None else ls.clone()
        run.lse = {}
        check_pair(run, o, 1)
        if lse:
            ref = run.lse[0]
            assert torch.equal(run.lse[PAIR_DUP], ref)
            assert torch.equal(run.lse[PAIR_HALF][:1], ref[:1])
            assert torch.equal(run.lse[PAIR_HALF][1:], torch.full_like(ref[1:], SENTINEL))
    finally:
        for name, _ in options:
            ops.set_option(name, 1)                  # the defaults of "attn_w4" and "attn32"


# w4 = 2: the one-wave-per-SIMD d = 40 kernel at every size (it takes the 64x64 level); w4 = 1: the size picks the
# four-waves-per-SIMD kernel here
@gpu
@pytest.mark.parametrize("w4", [1, 2])
@pytest.mark.parametrize("Sq,Sk,lse", [(300, 300, False), (300, 330, False), (300, 300, True)])
def test_attention_d40(dev, w4, Sq, Sk, lse):
    attn_case(dev, 40, Sq, Sk, lse=lse, options=[("attn_w4", w4)])


@gpu
@pytest.mark.parametrize("d,a32", [(80, 1), (80, 2), (160, 1)])
def test_attention_wide_heads(dev, d, a32):
    """d = 80 / 160 at S = 256 (the 32x32 and 16x16 levels); a32 = 2: the 32x32x16 kernel the large d = 80 launches take."""
    attn_case(dev, d, 256, 256, lse=True, options=[("attn32", a32)], seed=7)


# ---- norms -----------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("HW", [1024, 64], ids=["two_launches", "fused"])
@pytest.mark.parametrize("silu", [True, False])
def test_groupnorm(dev, HW, silu):
    B, C, G = 2, 320, 32
    x = twice(rnd((HW, C), dev, 3))
    gm, bt = rnd((C,), dev, 4, dtype=F32), rnd((C,), dev, 5, dtype=F32)
    y = torch.empty((B * HW, C), device=dev, dtype=F16)
    part = torch.empty((B, ops.gn_chunks(B, HW), G, 2), device=dev, dtype=F32)

    def run(pair):
        ops.groupnorm(x, B, HW, G, 1e-5, gm, bt, silu, out=y, part=part, pair=pair)
        torch.cuda.synchronize()
    check_pair(run, y, HW)


@gpu
@pytest.mark.parametrize("rows", [2 * 512, 2 * 16384], ids=["row_kernel", "streaming_kernel"])
def test_ln_stats(dev, rows):
    """2 x 512 rows of 320 run the one-wave-per-row kernel, 2 x 16384 the streaming one (the 64x64 level's)."""
    x = twice(rnd((rows // 2, 320), dev, 6))
    st = torch.empty((rows, 2), device=dev, dtype=F32)
    st.fill_(SENTINEL)
    ops.layernorm_stats(x, 320, stats=st)
    ref = st.clone()
    st.fill_(SENTINEL)
    ops.layernorm_stats(x, 320, stats=st, pair=PAIR_HALF)
    torch.cuda.synchronize()
    assert torch.equal(st[:rows // 2], ref[:rows // 2])
    assert torch.equal(st[rows // 2:], torch.full_like(st[rows // 2:], SENTINEL))


@gpu
def test_layernorm_with_output_half(dev):
    x = twice(rnd((512, 320), dev, 8))
    gm, bt = rnd((320,), dev, 9, dtype=F32), rnd((320,), dev, 10, dtype=F32)
    y = torch.empty((1024, 320), device=dev, dtype=F16)
    y.fill_(SENTINEL)
    ops.layernorm(x, gm, bt, out=y)
    ref = y.clone()
    y.fill_(SENTINEL)
    ops.layernorm(x, gm, bt, out=y, pair=PAIR_HALF)
    torch.cuda.synchronize()
    assert torch.equal(y[:512], ref[:512]) and torch.equal(y[512:], torch.full_like(y[512:], SENTINEL))


# ---- plans -----------------------------------------------------------------------------------------------------------
KEYS = [("down", 2, 1, 0), ("mid", 0, 0, 0), ("up", 1, 0, 0), ("up", 1, 1, 0), ("up", 1, 2, 0)]
_ENG = {}


def engine(name, dev):
    if name not in _ENG:
        cfg = weights.CONFIGS[name]
        _ENG[name] = UNetEngine(cfg, dev, weights.synth_state_dict(cfg, 0))
    return _ENG[name]


def plan_pair_vs_full(eng, x, fuser, save_keys, L):
    """eps_out and the captured maps of a pair_shared plan, option "cfg_pair" 1 vs 0 (two plans: the option is read when
    a plan is built).  The arena is poisoned in front of each run: nothing may rely on the rows a pair op skips."""
    outs, plans = [], []
    try:
        for on in (0, 1):
            ops.set_option("cfg_pair", on)
            plan = eng.plan(2, L, fuser=fuser, save_keys=save_keys, pair_shared=True)
            assert plan.pair_shared == bool(on)
            eng.poison_arena()
            plan.latents_in[:1].copy_(x)
            if not plan.latents_pair:
                plan.latents_in[1:].copy_(x)
            eps = plan.forward()
            torch.cuda.synchronize()
            outs.append((eps.clone(), {k: plan.maps[k].clone() for k in save_keys},
                         {n: a.t.clone() for n, a in plan.dbg.items()}))
            plans.append(plan)
    finally:
        ops.set_option("cfg_pair", 1)
    full, pair = plans
    assert full.pair_ops == 0 and not full.latents_pair
    assert pair.pair_ops > 0 and pair.latents_pair
    (e0, m0, d0), (e1, m1, d1) = outs
    assert torch.isfinite(e0).all()
    assert torch.equal(e0, e1), "eps_out differs between cfg_pair 1 and 0"
    for k in save_keys:
        assert torch.equal(m0[k], m1[k]), k
    for n in d0:                                     # dbg entries point at full buffers
        assert torch.equal(d0[n], d1[n]), n
    return pair


@gpu
@pytest.mark.parametrize("fuser", [True, False], ids=["fuser_on", "fuser_off"])
def test_tiny_gligen_main_plan(dev, fuser):
    g = np.load(os.path.join(GOLD, "unet_fwd_tiny_gligen.npz"))
    eng = engine("tiny_gligen", dev)
    eng.prepare_timesteps([int(g["t"])])
    eng.set_step(0)
    eng.prepare_text(torch.from_numpy(g["ehs"]))
    for on in (0, 1):                                # the concat buffers of both plans exist before the tokens are written
        ops.set_option("cfg_pair", on)
        eng.plan(2, 32, fuser=fuser, save_keys=KEYS, pair_shared=True)
    ops.set_option("cfg_pair", 1)
    eng.prepare_gligen(boxes=torch.from_numpy(g["gl_boxes"]), masks=torch.from_numpy(g["gl_masks"]),
                       positive_embeddings=torch.from_numpy(g["gl_emb"]))
    x = torch.from_numpy(g["x"])[:1].to(dev)
    plan_pair_vs_full(eng, x, fuser, KEYS, 32)


@gpu
def test_full_width_sd14_gligen_call(dev):
    """One B = 2 call of the full-width network at the 64x64 latent: the tuned tiles (phase tiles 46 / 47, the pipelined
    ones) and the d = 40 one-wave-per-SIMD attention kernel of the benchmark, fuser on."""
    cfg = weights.CONFIGS["sd14_gligen"]
    eng = UNetEngine(cfg, dev, weights.synth_state_dict(cfg, 0), max_text_batch=2)
    eng.prepare_timesteps([500])
    eng.set_step(0)
    eng.prepare_text(rnd((2, 77, cfg.cross_attention_dim), dev, 1, dtype=F32))
    for on in (0, 1):
        ops.set_option("cfg_pair", on)
        eng.plan(2, 64, fuser=True, pair_shared=True)
    ops.set_option("cfg_pair", 1)
    boxes = torch.zeros((2, 30, 4))
    boxes[:, 0] = torch.tensor([0.1, 0.2, 0.6, 0.7])
    masks = torch.zeros((2, 30))
    masks[1, 0] = 1
    eng.prepare_gligen(boxes=boxes, masks=masks, positive_embeddings=rnd((2, 30, 768), "cpu", 2, dtype=F32))
    pair = plan_pair_vs_full(eng, rnd((1, 4, 64, 64), dev, 3, dtype=F32), True, [], 64)
    # conv_in, 2 GroupNorms + 2 convs of the resnet, GroupNorm + proj_in, qkv, attention, to_out
    assert pair.pair_ops == 10


@gpu
def test_grad_and_multidiffusion_plans_have_no_pair_launch(dev):
    from fake_text import FakeTextEncoder, FakeTokenizer
    import json
    import md_golden_cases as cases
    from lgd_amd import multidiffusion as mdc
    from lgd_amd.sampler import LMDSampler
    eng = engine("tiny_gligen", dev)
    pg = eng.plan(2, 32, grad=True, fuser=False, stop_key=("up", 1, 2, 0), save_keys=KEYS[1:], pair_shared=True)
    assert not pg.pair_shared and pg.pair_ops == 0 and not pg.latents_pair
    # MultiDiffusion: the rows of its UNet batch differ (bootstrapped region latents): its plans never ask
    cfg = weights.CONFIGS[cases.UNET]
    e2 = UNetEngine(cfg, dev, weights.synth_state_dict(cfg, 0))
    case = next(c for c in cases.CASES if c[0] == "two")
    c = json.load(open(os.path.join(GOLD, "multidiffusion_surface.json")))["constants"]
    prep = mdc.prepare(case[1], case[2], c["bg_negative"], c["fg_negative_prompt"], extra_neg_prompt=case[6], first_top=case[5])
    texts = mdc.encode_texts(FakeTokenizer(), FakeTextEncoder(cfg.cross_attention_dim, device=dev), prep["prompts"],
                             prep["negative_prompts"], dev)
    d = mdc.draw_randomness(cases.StandInVAE(), "cpu", case[7], case[4], len(prep["prompts"]), case[3])
    mdc.multidiffusion_generate(LMDSampler(e2), texts, prep["masks"], d["start_latent"], d["bg_latents"], d["picks"],
                                steps=case[3], guidance_scale=cases.GUIDANCE, n_boot=case[4], decode=False, n_steps=1)
    assert e2._plans and all(p.pair_ops == 0 and not p.pair_shared for p in e2._plans.values())


@gpu
def test_sampler_main_plans_are_pair_plans_and_match_cfg_pair_off(dev):
    """The sampler asks for pair plans (and then fills the first half of latents_in only); a whole run is bit-identical
    to one with "cfg_pair" 0."""
    from lgd_amd.sampler import LMDSampler
    from lgd_amd.scheduler import DDIMScheduler
    cfg = weights.CONFIGS["tiny_gligen"]
    outs = []
    try:
        for on in (0, 1):
            ops.set_option("cfg_pair", on)
            eng = UNetEngine(cfg, dev, weights.synth_state_dict(cfg, 0))
            sm = LMDSampler(eng, DDIMScheduler())
            text = rnd((2, 77, cfg.cross_attention_dim), "cpu", 11, dtype=F32)
            r = sm.denoise(rnd((1, 4, 32, 32), "cpu", 12, dtype=F32), text, 3)
            outs.append(r["latents"].cpu())
            mains = [p for p in eng._plans.values() if not p.grad]
            assert mains and all(p.pair_shared == bool(on) and p.latents_pair == bool(on) for p in mains)
    finally:
        ops.set_option("cfg_pair", 1)
    assert torch.equal(outs[0], outs[1])

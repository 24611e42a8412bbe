"""The UNet inference (no-grad) plan as test data: tests/unet_plan_cases.py extended to the plan that produces every image.

What a no-grad plan has and the reverse-plan walker never reaches:
  * `ln_linear` (Plan.ln_linear with fold_ln): a statistics-only pass and a GEMM on the RAW rows with the gamma-folded
    weights, colsum and folded bias under LGD_EPI_ROWNORM;
  * GEGLU as a GEMM epilogue (EPI_GEGLU) instead of the geglu_fwd kernel;
  * everything behind the last guidance key: two-source GroupNorm / conv / shortcut on popped skips, the ups = True sampler
    convs, conv_norm_out and conv_out inside a plan;
  * the CFG pair modes (PAIR_HALF / PAIR_DUP) of the shared prefix, in place in a real plan's arena;
  * per-image time-embedding rows (text_time) and the "@d" K/V layers of deeper transformer blocks.

Statements.  Every kind keeps the statement and the bound of unet_plan_cases (which takes them from the kernel families'
conformance modules); new here:

  ln_linear    two things.  (1) The statistics side["stats"] [M][2] fp32 against the fp64 mean / rstd of the rows as given,
               inside layernorm_cases.fwd_ref's bound_mean / bound_rstd.  (2) The output against the LGD_EPI_ROWNORM statement
               of gemm_conformance_cases.Case WITH THE STATISTICS AS GIVEN:
                   v = rstd (x W'^T - mean cs) + b',   s = rstd (sum |x W'| + |mean cs|) + |b'|,
                   bound = 2^-11 |v| + 2^-25 + (K + 8) 2^-23 s + pack terms.
               The folded operands are rebuilt by name from the state dict, rounded where weightstore.fold rounds them:
                   W'  = fp16(fp32(fp16(W)) * fp32(gamma))      (one fp32 product, then the fp16 store)
                   cs  = fp32(sum_k W'[n][k])                    (of the STORED fp16 values)
                   b'  = fp32(b + fp16(W) beta)
               with the GEGLU row packing for .net.0.proj.  cs and b' are fp32 dot products of length K in the pack, whose
               order of summation the statement does not fix; the pack terms are their worst case
                   rstd |mean| K 2^-24 sum_k |W'[n][k]|   and   (K + 1) 2^-24 (sum_k |W[n][k] beta[k]| + |b[n]|).
               The .wln / .cs / .bln buffers are never read by the statement.
  GEGLU epilogue  read from csrc/gemm.hip (epilogue_value4 and the LDS epilogue, `normed` + gelu2_f): the accumulators, the
               row normalisation, the biases, the GELU and the product value * gelu(gate) are all fp32 — the pre-activation
               is NOT rounded to fp16 in front of the GELU; the only fp16 rounding is the final store.  The GELU of the
               epilogue is NOT the gelu_f of the geglu_fwd kernel (A&S erf, 1.5e-7) that small_kernel_cases.gelu_v renders:
               it is gelu2_f of csrc/common.h, x Phi2(x) with Phi2(x) = 0.5 + xc P(2 xc^2 / 20.25 - 1), xc = clamp(x, +-4.5),
               P a degree-10 polynomial — an approximation of Phi whose error the kernel's comment puts at 1.2e-5 of gelu.
               So the bound is small_kernel_cases' GEGLU bound (V arithmetic, r16) on a value and a gate that carry the
               GEMM's fp32 error e32 = (K + 8) 2^-23 s (+ pack terms), with gelu(g) carrying
                   1.13 e32 + (|g| + e32) (E_PHI + E_HORNER):   |gelu'| <= 1.13;
                   E_PHI = sup_x |Phi2(x) - Phi(x)|, measured here against math.erf on a grid (phi2_error, as
                   small_kernel_cases measures its erf polynomial);
                   E_HORNER = 4.5 2^-24 (11 sum |C_k| + 3 sum k |C_k|) + 2^-24: eleven fp32 fmas of the Horner form on
                   |s| <= 1, the three roundings of s through P', times |xc| <= 4.5, and the last fma.
               (The first version of this statement took gelu_v for the epilogue; the emulation used gelu_f as well and so
               could not show that bound too tight.  With the emulation on gelu2_f the old bound fails on the host too:
               tests/test_unet_fwd_plan_cpu.py::test_the_epilogue_gelu_is_not_the_kernel_gelu.)
  conv_out     small_kernel_cases.ConvOut (bias given, out_scale 1).
  per-image temb  the bias2 of a conv under text_time is row text_off + image of temb_cur; the statement adds that row to
               the rows of its image.

Pair mode.  Op.meta["pair"] is the op's PairMode (None outside the prefix).  A HALF / DUP op is checked on the first half of
its rows against the statement at the first half of its inputs (the launch keeps the full geometry: the variant codes are
asked with the full batch and the pair mode).  After a HALF op rows >= M/2 of the output still hold the poison; after a DUP op
the halves are bit-identical; the statistics pass of an ln_linear in pair mode is always HALF.  A LayerNorm whose PairMode
was turned to DUP runs in full (Plan.layernorm).

E_store (the end-to-end yardstick, reference alone): rel-L2 between the fp64 chain at exact weights and constants and the same
chain with the weights rounded as the store rounds them (folded ones included), the constants rounded to their storage types
and every activation rounded to fp16 where the plan stores it.

Hot rows (cases F and H): proj_in's bias of the first transformer is raised by a constant so that every row entering that
block's three ln_linear ops has |mean| / std >= 32 (a LayerNorm's beta cannot move the mean of its own INPUT; the betas of
norm1 / norm2 / norm3 are set as well, so that b' = b + W beta is not small).  The statement's bound already contains
rstd (K + 8) 2^-23 (sum |x W'| + |mean cs|); `amplification` is its ratio to the two-op form's bound at the same rows."""
import functools
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import unet_plan_cases as U  # noqa: E402
from unet_plan_cases import F32, F64, H16, L, T0, DEFAULT_KEYS, Act, N_OBJ_TOKENS, _bits, _f, _ns  # noqa: E402,F401
from lgd_amd import ops, weights  # noqa: E402
from lgd_amd._lib import PAIR_DUP, PAIR_HALF  # noqa: E402
from lgd_amd.unet import UNetEngine  # noqa: E402

R, attn, gn, lnc, sk = U.R, U.attn, U.gn, U.lnc, U.sk

CASES = {
    "F": dict(cfg="tiny", B=2, pair=True, keys=DEFAULT_KEYS),
    "G": dict(cfg="tiny_gligen", B=2, pair=True, keys=DEFAULT_KEYS, fuser=True),
    "H": dict(cfg="tiny_sd21", B=3, text_off=2),
    "I": dict(cfg="tiny_xl", B=2),
    "J": dict(cfg="tiny", B=1, fold=False),
    "K": dict(cfg="tiny_gligen", B=4, pair=True, fuser=True),
}
HOT_CASES = ("F", "H")
HOT_RATIO = 32.0
HOT_SHIFT = 96.0            # added to proj_in's bias of the first transformer (hot rows)
HOT_LAT_SCALE = 0.5
GLIGEN_BT = 4               # grounding rows of the fuser cases: B = 4 takes them all, B = 2 the first Bt // 2


def pair_of(m):
    """'half' / 'dup' / None: how the op's OUTPUT is written"""
    pm = m.get("pair")
    if pm is None:
        return None
    if pm.mode == PAIR_HALF:
        return "half"
    return None if m["kind"] == "layernorm" else "dup"       # a LayerNorm has no DUP form: it runs in full


def first_transformer(cfg):
    return next(a.prefix for b in weights.unet_blocks(cfg) for a in b.attns)


# =================================================================================================
# a case
# =================================================================================================
class FGraph(U.Graph):
    KINDS = U.KINDS + ("ln_linear",)

    def __init__(self, plan):
        assert not plan.grad and getattr(plan, "bwd_tail_meta", None) is None
        self.plan, self.metas = plan, []
        for i, op in enumerate(plan.ops):
            m = op.meta
            what = getattr(getattr(op.fwd, "__code__", None), "co_firstlineno", "?")
            assert isinstance(m, dict) and m.get("kind") in self.KINDS, \
                f"op {i} of the no-grad plan (built at unet.py:{what}) carries no meta of a known kind: {None if not isinstance(m, dict) else m.get('kind')}"
            assert not op.gouts and op.bwd is None
            self.metas.append(m)
        self.names = {id(a): n for n, a in plan.dbg.items()}


class FSetup(U.Setup):
    def __init__(self, case, device="cpu", hot=False):
        c = CASES[case]
        self.case, self.c, self.hot = case, c, hot
        self.cfg = weights.CONFIGS[c["cfg"]]
        self.sd = weights.synth_state_dict(self.cfg, 0)
        if hot:
            t = f"{first_transformer(self.cfg)}.transformer_blocks.0"
            self.sd = dict(self.sd)
            pb = f"{first_transformer(self.cfg)}.proj_in.bias"
            self.sd[pb] = self.sd[pb] + HOT_SHIFT
            for j, n in enumerate(("norm1", "norm2", "norm3")):
                self.sd[f"{t}.{n}.bias"] = self.sd[f"{t}.{n}.bias"] + (0.5 + 0.25 * j)
        self.sd64 = {k: v.to(F64) for k, v in self.sd.items()}
        self.device = torch.device(device)
        self.eng = UNetEngine(self.cfg, self.device, self.sd)
        if not c.get("fold", True):
            self.eng.fold_ln = False
        B = self.B = c["B"]
        self.keys = [tuple(k) for k in c.get("keys", ())]
        self.text_off, self.obj_off, self.fuser = c.get("text_off", 0), c.get("obj_off", 0), c.get("fuser", False)
        g = torch.Generator().manual_seed(4321 + sum(map(ord, case)))
        self.lat = torch.randn(B, self.cfg.in_channels, L, L, generator=g) * (HOT_LAT_SCALE if hot else 1.0)
        if c.get("pair"):
            self.lat[B // 2:] = self.lat[:B // 2]                        # a CFG batch over one set of latents
        self.ehs = torch.randn(self.text_off + B, self.eng.text_len, self.cfg.cross_attention_dim, generator=g)
        self.gligen = self.added = None
        if self.fuser:
            Bt = GLIGEN_BT
            boxes, masks = torch.zeros(Bt, N_OBJ_TOKENS, 4), torch.zeros(Bt, N_OBJ_TOKENS)
            xy = torch.rand(Bt, 3, 2, generator=g) * 0.5
            boxes[:, :3] = torch.cat([xy, xy + 0.1 + 0.4 * torch.rand(Bt, 3, 2, generator=g)], -1)
            masks[Bt // 2:, :3] = 1.0                                    # the first half is zero-masked (the unconditional one)
            emb = torch.zeros(Bt, N_OBJ_TOKENS, self.cfg.gligen_positive_len)
            emb[:, :3] = torch.randn(Bt, 3, self.cfg.gligen_positive_len, generator=g)
            self.gligen = dict(boxes=boxes, masks=masks, positive_embeddings=emb)
        if self.cfg.addition_embed_type == "text_time":
            Rn = self.text_off + B
            ids = torch.tensor([[32.0, 32.0, 0.0, 0.0, 6.0], [48.0, 24.0, 4.0, 8.0, 2.5]])[torch.arange(Rn) % 2]
            self.added = dict(text_embeds=torch.randn(Rn, self.cfg.pooled_dim, generator=g), time_ids=ids)
        self.stop = None
        self.plan = self.eng.plan(B, L, grad=False, fuser=self.fuser, save_keys=self.keys, text_batch_offset=self.text_off,
                                  obj_batch_offset=self.obj_off, pair_shared=bool(c.get("pair")))
        self.graph = FGraph(self.plan)
        self.cot = None
        self.install_constants()

    # ---- constants ---------------------------------------------------------------------------------
    def pure_temb_act(self, sd=None):
        """silu(time embedding (+ the text_time embedding of every image)) [rows][ted], fp64"""
        sd = self.sd64 if sd is None else sd
        Fn = torch.nn.functional
        emb = R.timestep_embedding(torch.tensor([T0]), self.cfg.block_out_channels[0], F64)
        emb = Fn.linear(emb, sd["time_embedding.linear_1.weight"], sd["time_embedding.linear_1.bias"])
        emb = Fn.linear(Fn.silu(emb), sd["time_embedding.linear_2.weight"], sd["time_embedding.linear_2.bias"])
        if self.added is not None:
            te, ids = self.added["text_embeds"].to(F64), self.added["time_ids"].to(F64)
            tid = R.timestep_embedding(ids.reshape(-1), self.cfg.addition_time_embed_dim, F64).reshape(ids.shape[0], -1)
            a = Fn.linear(torch.cat([te, tid], -1), sd["add_embedding.linear_1.weight"], sd["add_embedding.linear_1.bias"])
            a = Fn.linear(Fn.silu(a), sd["add_embedding.linear_2.weight"], sd["add_embedding.linear_2.bias"])
            emb = emb + a                                                # [R][ted]
        return Fn.silu(emb)

    def pure_constants(self, sd=None):
        out = super().pure_constants(sd)
        out["temb_act"] = self.pure_temb_act(sd)
        return out

    def temb_rows_of(self, m, pc):
        """fp64 [images][Cout] of a conv with a time embedding: the projection of each image's row"""
        p = m["name"][:-len(".conv1")]
        v = torch.nn.functional.linear(pc["temb_act"], self.sd64[f"{p}.time_emb_proj.weight"], self.sd64[f"{p}.time_emb_proj.bias"])
        return v if self.added is None else v[self.text_off:self.text_off + self.B]

    def install_constants(self):
        eng = self.eng
        if self.device.type == "cuda":
            eng.prepare_timesteps([T0], self.added)
            eng.set_step(0)
            eng.prepare_text(self.ehs)
            if self.gligen is not None:
                eng.prepare_gligen(self.gligen["boxes"], self.gligen["masks"], self.gligen["positive_embeddings"])
        else:
            pc = self.pure_constants()
            for m in self.graph.metas:
                if m["kind"] == "conv" and m["temb_off"] is not None:
                    v = self.temb_rows_of(m, pc).to(F32)
                    sl = slice(m["temb_off"], m["temb_off"] + v.shape[1])
                    if self.added is None:
                        eng.temb_cur[0, sl] = v[0]
                    else:
                        eng.temb_cur[self.text_off:self.text_off + self.B, sl] = v
                if m["kind"] == "cross_attn":
                    m["kv"][:self.B].copy_(pc["kv"][m["layer"]].to(H16))
                if m["kind"] == "layernorm" and m["S"]:
                    m["out"].t.view(self.B, m["S"] + N_OBJ_TOKENS, -1)[:, m["S"]:] = pc["tail"][id(m["out"])].to(H16)
        self.tails0 = {id(m["out"]): m["out"].t.view(self.B, m["S"] + N_OBJ_TOKENS, -1)[:, m["S"]:].clone()
                       for m in self.graph.metas if m["kind"] == "layernorm" and m["S"]}


class FCtx(U.Ctx):
    """consts: "given" (the engine's buffers), "rounded" (the fp64 constants rounded to their storage types); pure: exact"""

    def __init__(self, setup, pure, consts="given", dev=None):
        super().__init__(setup, pure)
        self.consts = "pure" if pure else consts
        if dev is not None:
            self.dev = torch.device(dev)
        if self.consts == "rounded":
            self.pc = setup.pure_constants()

    def temb(self, m):
        """[Cout], or under text_time [rows][Cout] (the row of each image repeated over its pixels)"""
        if m.get("temb_off") is None:
            return None
        s = self.s
        n = m["out"].C
        if self.consts == "given":
            rows = s.eng.temb_cur[:, m["temb_off"]:m["temb_off"] + n].to(F64)
            rows = rows[0:1] if s.added is None else rows[s.text_off:s.text_off + s.B]
        else:
            rows = s.temb_rows_of(m, self.pc)
            if self.consts == "rounded":
                rows = rows.to(F32).to(F64)
        rows = rows.to(self.dev)
        if s.added is None:
            return rows[0]
        return rows.repeat_interleave(m["H"] * m["H"], 0)

    def kv(self, m):
        if self.consts == "given":
            return m["kv"][:self.s.B].to(F64)
        kv = self.pc["kv"][m["layer"]]
        return kv if self.pure else kv.to(H16).to(F64)

    def tail(self, m):
        if self.consts == "given":
            return self.s.tails0[id(m["out"])].to(F64)
        t = self.pc["tail"][id(m["out"])]
        return t if self.pure else t.to(H16).to(F64)

    def folded(self, m):
        """(W', cs, b', pack error of cs per |mean| rstd, pack error of b') of an ln_linear, by name, in fp64"""
        key = ("fold", m["name"])
        if key not in self._c:
            p = m["params"]
            Wm = self.mat(p["weight"], p["geglu_rows"])                   # fp16 values (or exact)
            gamma, beta = self.vec(p["norm_weight"]), self.vec(p["norm_bias"])
            b = self.vec(p["bias"], p["geglu_rows"]) if p["bias"] else torch.zeros(Wm.shape[0], dtype=F64, device=self.dev)
            K = Wm.shape[1]
            if self.pure:
                wln = Wm * gamma
                self._c[key] = (wln, wln.sum(1), b + Wm @ beta, torch.zeros_like(b), torch.zeros_like(b))
            else:
                wln = (Wm.to(F32) * gamma.to(F32)).to(H16).to(F64)
                cs = wln.sum(1).to(F32).to(F64)
                bln = (b + Wm @ beta).to(F32).to(F64)
                e_cs = K * 2.0 ** -24 * wln.abs().sum(1)
                e_b = (K + 1) * 2.0 ** -24 * (Wm.abs() @ beta.abs() + b.abs())
                self._c[key] = (wln, cs, bln, e_cs, e_b)
        return self._c[key]


# =================================================================================================
# statements
# =================================================================================================
def gemm_pre(A, Wm, bias=None, bias2=None):
    """value and fp32 error of A W^T + biases in front of any rounding (gemm_stmt without its fp16 store)"""
    K = A.shape[1]
    v, s = A @ Wm.t(), A.abs() @ Wm.abs().t()
    for b in (bias, bias2):
        if b is not None:
            v, s = v + b, s + b.abs()
    return v, (K + 8) * 2.0 ** -23 * s


GELU2_C = (1.569049306e-01, -7.719386027e-02, 5.470118655e-02, -4.010922254e-02, 2.828396914e-02, -1.902089461e-02,
           1.143910392e-02, -5.251618182e-03, 2.716435037e-03, -2.339980905e-03, 9.806225403e-04)       # csrc/common.h: gelu2_f


def phi2(x):
    """Phi2 of gelu2_f in the arithmetic of x's dtype (fp32: the emulation; fp64 with the fp32 coefficients: the function)"""
    c = [torch.tensor(sk.f32(ck), dtype=x.dtype, device=x.device) for ck in GELU2_C]
    xc = x.clamp(-4.5, 4.5)
    s_ = xc * xc * torch.tensor(sk.f32(2.0 / 20.25), dtype=x.dtype, device=x.device) - 1.0
    p = c[10]
    for k in range(9, -1, -1):
        p = p * s_ + c[k]
    return xc * p + 0.5


def gelu2_32(g):
    return g * phi2(g.to(F32))


@functools.lru_cache(maxsize=None)
def phi2_error():
    """sup |Phi2(x) - Phi(x)|: a grid of 1e-3 over [-12, 12] (beyond it both sides are constant to 1e-30)"""
    x = torch.arange(-12000, 12001, dtype=F64) * 1e-3
    return float((phi2(x) - 0.5 * (1.0 + torch.erf(x * 2.0 ** -0.5))).abs().max())


E_HORNER = 4.5 * 2.0 ** -24 * (11 * sum(abs(c) for c in GELU2_C) + 3 * sum(k * abs(c) for k, c in enumerate(GELU2_C))) + 2.0 ** -24


def gelu2_v(g):
    """the epilogue's GELU of a V: the exact gelu as the value, gelu2_f's approximation and fp32 evaluation in the error"""
    v = 0.5 * g.v * (1.0 + torch.erf(g.v * 2.0 ** -0.5))
    return sk.V(v, 1.13 * g.e + (g.v.abs() + g.e) * (phi2_error() + E_HORNER))


def geglu_epilogue(v, e32, gelu=None):
    """value * gelu2_f(gate) of a packed fp32 pre-activation with error e32 (module docstring); gelu: another rendering of the
    GELU (sk.gelu_v: the statement this module had first, kept for the test that shows it too tight)"""
    n = v.shape[1] // 2
    pv, pg = (p.to(v.device) for p in sk.geglu_positions(n))
    y = sk.V(v[:, pv], e32[:, pv]) * (gelu or gelu2_v)(sk.V(v[:, pg], e32[:, pg]))
    return y.v, sk.r16(y)


def fwd_linear(m, ins, cx, saved=None):
    if not m["geglu_epilogue"]:
        return U.fwd_linear(m, ins, cx, saved)
    p, M = m["params"], m["rows"]
    assert m["res"] is None and float(m["alpha"]) == 1.0
    v, e = gemm_pre(ins[0][:M], cx.mat(p["weight"], p["geglu_rows"]), cx.vec(p["bias"], p["geglu_rows"]) if p["bias"] else None)
    return dict(out=geglu_epilogue(v, e))


def ln_linear_parts(m, x, stats, cx):
    """(v, e32) of the LGD_EPI_ROWNORM GEMM in front of GEGLU / the fp16 store, with the statistics as given"""
    wln, cs, bln, e_cs, e_b = cx.folded(m)
    K = x.shape[1]
    mean, rstd = stats[:, 0:1], stats[:, 1:2]
    acc, s = x @ wln.t(), x.abs() @ wln.abs().t()
    v = rstd * (acc - mean * cs) + bln
    s = rstd.abs() * (s + (mean * cs).abs()) + bln.abs()
    return v, (K + 8) * 2.0 ** -23 * s + rstd.abs() * mean.abs() * e_cs + e_b


def fwd_ln_linear(m, ins, cx, saved=None):
    p, M = m["params"], m["rows"]
    x = ins[0][:M]
    r = lnc.fwd_ref(x, torch.ones(x.shape[1], dtype=F64, device=x.device), torch.zeros(x.shape[1], dtype=F64, device=x.device))
    st_ref = torch.cat([r["mean"], r["rstd"]], 1)
    st_bound = torch.cat([r["bound_mean"], r["bound_rstd"]], 1)
    stats = saved["stats"][:M] if saved and "stats" in saved else st_ref
    v, e = ln_linear_parts(m, x, stats, cx)
    out = geglu_epilogue(v, e) if m["geglu_epilogue"] else (v, 2.0 ** -11 * v.abs() + 2.0 ** -25 + e)
    return dict(out=out, stats=(st_ref, st_bound))


def two_op_bound(m, x, cx):
    """the bound of the form the fold replaces, at the same rows: LayerNorm to fp16 (taken as given), then the plain GEMM"""
    p = m["params"]
    y = lnc.fwd_ref(x, cx.vec(p["norm_weight"]), cx.vec(p["norm_bias"]))["y"].to(H16).to(F64)
    v, e = gemm_pre(y, cx.mat(p["weight"], p["geglu_rows"]), cx.vec(p["bias"], p["geglu_rows"]) if p["bias"] else None)
    return geglu_epilogue(v, e)[1] if m["geglu_epilogue"] else 2.0 ** -11 * v.abs() + 2.0 ** -25 + e


def _pair_int(m):
    return {None: 0, "half": PAIR_HALF, "dup": PAIR_DUP}[m.get("_pair")]


def fwd_groupnorm(m, ins, cx, saved=None):
    p = m["params"]
    x = torch.cat(ins, 1)
    B = x.shape[0] // m["HW"]
    c0, c1 = ins[0].shape[1], ins[1].shape[1] if len(ins) > 1 else 0
    code = ops.groupnorm_plan(ops.GN_OP_FWD, c0, c1, m.get("_B", B), m["HW"], m["G"], silu=m["silu"], pair=_pair_int(m))
    row = gn.Row(code, "fwd", c0, c1, m["HW"], B, G=m["G"], silu=m["silu"])
    r = gn.fwd_reference(x.reshape(B, m["HW"], -1), cx.vec(p["weight"]), cx.vec(p["bias"]), m["G"], m["eps"], m["silu"],
                         depth=row.depth, two_launch=row.two_launch)
    return dict(out=(r["y"].reshape(x.shape), r["bound_y"].reshape(x.shape)))


def fwd_self_attn(m, ins, cx, saved=None):
    B, C, q, k, v = U._self_qkv(m, ins[0])
    code = ops.attn_plan(ops.ATTN_OP_FWD, m.get("_B", B), m["heads"], m["S"], m["Sk"], m["d"], pair=_pair_int(m))
    row = attn.Row(code, "self", B, m["heads"], m["d"], Sq=m["S"], Sk=m["Sk"])
    r = U._per_image(lambda b: attn.fwd_reference(q[b], k[b], v[b], m["scale"], DP=row.DP, ones=row.ones), B, ("o", "bound_o"))
    return dict(out=(U._rows(r["o"]), U._rows(r["bound_o"])))


def _conv_out_row(m, B):
    return _ns(B=B, L=m["H"], Cin=m["ins"][0].C, Cout=m["out"].shape[1], dgrad=False, out_scale=1.0, bias=True)


def fwd_conv_out(m, ins, cx, saved=None):
    x = ins[0]
    Ls = m["H"]
    B = x.shape[0] // (Ls * Ls)
    d = {"x": x.reshape(B, Ls * Ls, -1), "w": U.pack_fwd(cx.mat(m["params"]["weight"])), "bias": cx.vec(m["params"]["bias"])}
    return dict(out=sk.ConvOut().reference(_conv_out_row(m, B), d)["y"])


FWD = dict(U.FWD, linear=fwd_linear, ln_linear=fwd_ln_linear, groupnorm=fwd_groupnorm, self_attn=fwd_self_attn, conv_out=fwd_conv_out)
SIDES = ("stats", "maps")


# =================================================================================================
# the forward chain
# =================================================================================================
class FChain:
    def __init__(self, setup, pure, consts="rounded", dev=None):
        self.s, self.g, self.cx = setup, setup.graph, FCtx(setup, pure, consts, dev)
        self.vals = {}

    def forward(self, lat, round_store=False, until=None):
        """(eps, {key: map}).  round_store: every activation rounded where the plan stores it (fp16; eps and the maps fp32).
        until: the chain ends behind this op."""
        maps, eps = {}, None
        for i, m in enumerate(self.g.metas):
            if until is not None and i > until:
                break
            ins = [lat.to(self.cx.dev, F64)] if m["kind"] == "conv_in" else [self.vals[id(a)] for a in U.Graph.inputs(m)]
            r = FWD[m["kind"]](m, ins, self.cx)
            out = r["out"][0]
            if round_store:
                out = out.to(H16 if isinstance(m["out"], Act) else F32).to(F64)
            self.vals[id(m["out"])] = out
            if m["kind"] == "cross_attn" and m["key"] in self.s.plan.save_keys:
                maps[m["key"]] = r["maps"][0].to(F32).to(F64) if round_store else r["maps"][0]
            if m["kind"] == "conv_out":
                eps = out
        return eps, maps


def restate_forward(setup):
    """fp64 (eps, maps, taps) of oracle/restate.unet_forward on the case's inputs"""
    s = setup
    saved, taps = {}, {}
    gl = None
    if s.gligen is not None:
        gl = {k: v.to(F64)[s.obj_off:s.obj_off + s.B] for k, v in s.gligen.items()}
    with torch.no_grad():
        eps = R.unet_forward(s.sd64, s.restate_cfg(), s.lat.to(F64), T0, s.ehs.to(F64)[s.text_off:s.text_off + s.B], saved=saved,
                             save_keys=s.keys, gligen=gl, fuser_enabled=s.fuser, taps=taps)
    return eps, saved, taps


# =================================================================================================
# the emulator of a no-grad plan (fp32 arithmetic, fp16 storage, the PACKED weights), and wrong plans
# =================================================================================================
class FEmulator(U.Emulator):
    """Every op is computed over ALL rows (each op is independent per image, so the poison of a half that was never written
    stays in that half) and the pair mode is applied to what it stores: HALF puts the second half back, DUP copies the first.

    mutant: dict(kind=.., op=index, ...) — MUTANTS."""

    def fwd(self, i):
        m = self.metas[i]
        mode = pair_of(m)
        out = m["out"].t if isinstance(m["out"], Act) else m["out"]
        before = out.clone() if mode else None
        st = m["side"]["stats"] if m["kind"] == "ln_linear" else None
        st_before = st.clone() if (st is not None and m.get("pair") is not None) else None
        getattr(self, "f_" + m["kind"])(i, m)
        h = out.shape[0] // 2
        if mode == "half":
            out[h:] = before[h:]
            if self._is("half_writes_row", i):
                out[h] = out[0]
        elif mode == "dup":
            out[h:] = out[:h]
        if st_before is not None:
            st[st.shape[0] // 2:] = st_before[st.shape[0] // 2:]

    def _temb(self, i, m, rows):
        off = m["temb_off"]
        if self._is("neighbour_temb", i):
            off = self.mut["other_off"]
        n, s = m["out"].C, self.s
        if s.added is None:
            return s.eng.temb_cur[0, off:off + n]
        return s.eng.temb_cur[s.text_off:s.text_off + s.B, off:off + n].repeat_interleave(rows // s.B, 0)

    def f_conv_in(self, i, m):
        lat, lat8 = m["ins"][0], m["scratch"][0]                         # under the pair: the first half of the images
        B, Cl, Ls, _ = lat.shape
        lat8.copy_(sk.Nhwc8().reference(None, {"x": lat.reshape(B, Cl, Ls * Ls)})["y"][0].to(H16))
        A = self._gather(lat8, B, Ls, Ls, Ls, Ls, 1, 0)
        m["out"].t[:A.shape[0]] = (A @ _f(self.w.h["conv_in.w8"]).t() + self.w.f["conv_in.b"]).to(H16)

    def f_conv(self, i, m):
        n, B = m["name"], self.s.B
        H, Hl, Ho, stride = U._conv_geom(m, B)
        ups = 1 if m["ups"] else 0
        if self._is("ups_at_input_res", i):
            ups, Ho = 0, H
        A = torch.cat([self._gather(a.t, B, H, H, Ho, Ho, stride, ups).reshape(B * Ho * Ho, 9, -1) for a in m["ins"]], 2)
        y = A.reshape(B * Ho * Ho, -1) @ _f(self.w.h[f"{n}.w"]).t() + self.w.f[f"{n}.b"]
        if m["temb_off"] is not None:
            y = y + self._temb(i, m, y.shape[0])
        if m["res"] is not None:
            y = y + _f(m["res"].t)
        m["out"].t[:y.shape[0]] = y.to(H16)

    def f_groupnorm(self, i, m):
        n, B, HW, G = m["name"], self.s.B, m["HW"], m["G"]
        srcs = list(m["ins"])
        if self._is("gn_sources_swapped", i):
            srcs = srcs[::-1]
        if self._is("skip_swapped", i):
            srcs[1] = self.mut["other"]
        x = torch.cat([_f(a.t) for a in srcs], 1).reshape(B, HW, G, -1)
        mean = x.mean((1, 3), keepdim=True)
        rstd = torch.rsqrt(((x - mean) ** 2).mean((1, 3), keepdim=True) + torch.tensor(m["eps"], dtype=F32))
        cpg = x.shape[-1]
        z = (x - mean) * rstd * self.w.f[f"{n}.g"].view(G, cpg) + self.w.f[f"{n}.b"].view(G, cpg)
        if m["silu"]:
            z = z / (1.0 + torch.exp(-z))
        m["out"].t.copy_(z.reshape(B * HW, -1).to(H16))

    def f_layernorm(self, i, m):
        n = m["name"]
        x = _f(m["ins"][0].t[:m["rows"]])
        mean = x.mean(-1, keepdim=True)
        rstd = torch.rsqrt(((x - mean) ** 2).mean(-1, keepdim=True) + torch.tensor(m["eps"], dtype=F32))
        y = ((x - mean) * rstd * self.w.f[f"{n}.g"] + self.w.f[f"{n}.b"]).to(H16)
        if m["S"]:
            S = m["S"]
            m["out"].t.view(-1, S + N_OBJ_TOKENS, x.shape[1])[:, :S] = y.view(-1, S, x.shape[1])
        else:
            m["out"].t.copy_(y)

    def _geglu(self, y):
        n, v, g = U._geglu_parts(y)
        if self.mut.get("kind") == "geglu_swapped":
            v, g = g, v
        return v * gelu2_32(g)

    def f_linear(self, i, m):
        if not m["geglu_epilogue"]:
            return super().f_linear(i, m)
        M, n = m["rows"], m["name"]
        y = _f(m["ins"][0].t[:M]) @ _f(self.w.h[f"{n}.w"]).t() + self.w.f[f"{n}.b"]
        m["out"].t[:M] = self._geglu(y).to(H16)

    def f_ln_linear(self, i, m):
        M, n = m["rows"], m["name"]
        x = _f(m["ins"][0].t[:M])
        if self._is("half_stats_upper", i):
            assert m.get("pair") is not None
            x_st = torch.cat([x[M // 2:], x[M // 2:]])
        else:
            x_st = x
        mean = x_st.mean(-1, keepdim=True)
        rstd = torch.rsqrt(((x_st - mean) ** 2).mean(-1, keepdim=True) + torch.tensor(lnc.EPS, dtype=F32))
        st = m["side"]["stats"]
        st.copy_(torch.cat([rstd, mean], 1) if self._is("stats_swapped", i) else torch.cat([mean, rstd], 1))
        mean, rstd = st[:, 0:1], st[:, 1:2]                               # the GEMM reads what the pass stored
        cs, bln = self.w.f[f"{n}.cs"], self.w.f[f"{n}.bln"]
        if self._is("cs_unrounded", i):
            gamma = self.s.sd[m["params"]["norm_weight"]].to(F32)
            cs = (_f(self.w.h[f"{n}.w"]) * gamma).sum(1)
        if self._is("bln_no_beta", i):
            bln = self.w.f[f"{n}.b"] if f"{n}.b" in self.w.f else torch.zeros_like(bln)
        y = rstd * (x @ _f(self.w.h[f"{n}.wln"]).t() - mean * cs) + bln
        m["out"].t[:M] = (self._geglu(y) if m["geglu_epilogue"] else y).to(H16)

    def f_self_attn(self, i, m):
        B, C, q, k, v = U._self_qkv(m, _f(m["ins"][0].t))
        code = ops.attn_plan(ops.ATTN_OP_FWD, B, m["heads"], m["S"], m["Sk"], m["d"], pair=_pair_int(dict(_pair=pair_of(m))))
        row = attn.Row(code, "self", B, m["heads"], m["d"], Sq=m["S"], Sk=m["Sk"])
        for b in range(B):
            r = attn.fwd_emulation(q[b], k[b], v[b], m["scale"], ones=row.ones)
            m["out"].t.view(B, m["S"], C)[b] = r["o"].permute(1, 0, 2).reshape(m["S"], C).to(H16)

    def _cross(self, m):
        if self.mut.get("kind") == "text_off_minus_1" and self.metas[self.mut["op"]] is m:
            H, B, s = m["heads"], self.s.B, self.s
            qx = _f(m["ins"][0].t)
            C = qx.shape[1]
            kv = _f(s.eng.text_kv[m["layer"]][s.text_off - 1:s.text_off - 1 + B])
            return B, C, U._heads(qx, B, H), U._heads(kv[:, :, :C].reshape(-1, C), B, H), U._heads(kv[:, :, C:].reshape(-1, C), B, H)
        return super()._cross(m)

    def f_conv_out(self, i, m):
        B, Ls = self.s.B, m["H"]
        bias = None if self._is("conv_out_no_bias", i) else self.w.f["conv_out.b"]
        d = {"x": m["ins"][0].t.view(B, Ls * Ls, -1), "w": self.w.h["conv_out.w"], "bias": bias}
        m["out"].copy_(sk.ConvOut().emulate(_conv_out_row(m, B), d)["y"])


# =================================================================================================
# the walker of a no-grad plan
# =================================================================================================
class FWalker(U.Walker):
    def __init__(self, setup, executor=None):
        super().__init__(setup, executor or (U.Device(setup) if setup.device.type == "cuda" else FEmulator(setup)))
        self.cx = FCtx(setup, pure=False)
        self.amplification = {}                                          # op index -> bound of the fold / bound of the two ops
        self.hot = {}                                                    # op index -> smallest |mean| / std of its input rows
        self.final = None

    @staticmethod
    def _out(m):
        return m["out"].t if isinstance(m["out"], Act) else m["out"]

    def _declared(self, m):
        decl = [self._out(m)] + [t for t in m.get("side", {}).values() if t is not None]
        return decl + [t for t in m.get("scratch", []) if m["kind"] in ("conv_in", "groupnorm")]

    def _check_pair(self, i, m):
        label = self.g.label(i)
        mode, out = pair_of(m), self._out(m)
        h = out.shape[0] // 2
        if mode == "half" and not bool((_bits(out[h:]) == -1).all()):
            self.integrity.append(f"{label} runs HALF and changed rows >= M/2 of its output")
        if mode == "dup" and not torch.equal(_bits(out[:h]), _bits(out[h:])):
            self.integrity.append(f"{label} runs DUP and its halves differ")
        if m["kind"] == "ln_linear" and m.get("pair") is not None:
            st = m["side"]["stats"]
            if not bool((_bits(st[st.shape[0] // 2:]) == -1).all()):
                self.integrity.append(f"{label}: the HALF statistics pass changed rows >= M/2")

    def _check_fwd(self, i, m, amplify=False):
        mode = pair_of(m)
        in_pair = m.get("pair") is not None and not (m["kind"] == "layernorm" and mode is None)
        ins = self._given(m)
        mm = m
        if in_pair:
            if m["kind"] != "conv_in":
                ins = [t[:t.shape[0] // 2] for t in ins]
            mm = dict(m, _pair=mode, _B=self.s.B)
            if "rows" in m:
                mm["rows"] = m["rows"] // 2
        saved = {}
        if m["kind"] == "conv_in":
            saved["lat8"] = m["scratch"][0].to(F64)
        if m["kind"] == "ln_linear":
            saved["stats"] = m["side"]["stats"].to(F64)
        r = FWD[m["kind"]](mm, ins, self.cx, saved=saved)
        n = r["out"][0].shape[0]
        out = self._out(m)
        what = {"output": self._ratio(out[:n], r["out"], fp16=isinstance(m["out"], Act))}
        for sn in SIDES:
            if sn in r and m["side"][sn] is not None:
                what[sn] = self._ratio(m["side"][sn][:r[sn][0].shape[0]], r[sn], fp16=False)
        if "lat8" in r:
            what["lat8"] = self._ratio(m["scratch"][0], r["lat8"])
        worst = max(what, key=what.get)
        self.fwd_ratio[i] = (what[worst], worst)
        if amplify and m["kind"] == "ln_linear":
            x = ins[0][:mm["rows"]]
            self.amplification[i] = float(r["out"][1].mean() / two_op_bound(mm, x, self.cx).mean())
            self.hot[i] = row_heat(x)

    def run(self, check_fwd=None, integrity=True, amplify=False):
        s, plan, eng, metas = self.s, self.plan, self.s.eng, self.g.metas
        eng.poison_arena()
        plan.latents_in.copy_(s.lat)
        if plan.latents_pair:
            plan.latents_in[s.B // 2:].view(torch.int32).fill_(-1)      # the second half is never read
        if integrity:
            self._snapshot()
        for i, m in enumerate(metas):
            self.ex.fwd(i)
            if integrity:
                self._check_integrity(f"forward of {self.g.label(i)}", self._declared(m))
            self._check_pair(i, m)
            if check_fwd is None or i in check_fwd:
                self._check_fwd(i, m, amplify)
        self.final = (self.seg[:self.ext].clone(), [t.clone() for _, t in self.outside])
        return plan.eps_out

    def replay(self, i, executor):
        """op i alone, by another executor, on the operands a whole run recorded: (ratio, what, violations)"""
        assert self.final is not None
        m = self.g.metas[i]
        self.seg[:self.ext].copy_(self.final[0])
        for (_, t), t0 in zip(self.outside, self.final[1]):
            t.copy_(t0)
        for t in self._declared(m):
            if self._range(t) is not None:
                _bits(t).fill_(-1)
        self.integrity, self.fwd_ratio = [], {}
        self._snapshot()
        executor.fwd(i)
        self._check_integrity(f"forward of {self.g.label(i)}", self._declared(m))
        self._check_pair(i, m)
        self._check_fwd(i, m)
        return self.fwd_ratio[i] + (list(self.integrity),)

    def worst(self, which="fwd"):
        d = self.fwd_ratio
        i = max(d, key=lambda j: d[j][0])
        return d[i][0], f"{self.g.label(i)}: {d[i][1]}"


def hot_ops(setup):
    """the ln_linear ops of the first transformer block (hot rows)"""
    t = f"{first_transformer(setup.cfg)}.transformer_blocks.0."
    return [i for i, m in enumerate(setup.graph.metas) if m["kind"] == "ln_linear" and m["name"].startswith(t) and ".fuser." not in m["name"]]


def row_heat(x):
    """the smallest |mean| / std over the rows of x"""
    x = x.to(F64)
    mean = x.mean(-1)
    return float((mean.abs() / (x - mean[:, None]).pow(2).mean(-1).sqrt()).min())


def find_op(setup, pred, last=False):
    idx = [i for i, m in enumerate(setup.graph.metas) if pred(m)]
    return idx[-1] if last else idx[0]


# =================================================================================================
# wrong plans: name -> (case, hot, setup -> (op index, mutant)); each has to be caught at that op by FWalker.replay
# =================================================================================================
def _two_source_norms(s):
    return [i for i, m in enumerate(s.graph.metas) if m["kind"] == "groupnorm" and len(m["ins"]) == 2]


def _skip_swap(s):
    idx = _two_source_norms(s)
    for i in idx:
        for j in idx:
            a, b = s.graph.metas[i]["ins"][1], s.graph.metas[j]["ins"][1]
            if a is not b and a.t.shape == b.t.shape:
                return i, dict(kind="skip_swapped", op=i, other=b)
    raise AssertionError("no two skips of equal shape")


def _neighbour_temb(s):
    convs = [i for i, m in enumerate(s.graph.metas) if m["kind"] == "conv" and m["temb_off"] is not None]
    i = convs[0]
    j = next(j for j in convs[1:] if s.graph.metas[j]["out"].C == s.graph.metas[i]["out"].C)
    return i, dict(kind="neighbour_temb", op=i, other_off=s.graph.metas[j]["temb_off"])


def _at(kind, pred, last=False):
    def make(s):
        i = find_op(s, pred, last)
        return i, dict(kind=kind, op=i)
    return make


def _is_fold(m):
    return m["kind"] == "ln_linear"


MUTANTS = {
    "cs summed from the unrounded W gamma": ("F", True, _at("cs_unrounded", _is_fold)),
    "bln without W beta": ("F", True, _at("bln_no_beta", _is_fold)),
    "mean and rstd swapped in the statistics": ("F", True, _at("stats_swapped", _is_fold)),
    "a HALF statistics pass that reads rows M/2..M": ("F", True, _at("half_stats_upper", lambda m: _is_fold(m) and m.get("pair") is not None)),
    "value and gate swapped in the GEGLU epilogue": ("F", True, _at("geglu_swapped", lambda m: _is_fold(m) and m["geglu_epilogue"])),
    "the two sources of an up-block groupnorm in the wrong order": ("F", True, lambda s: (_two_source_norms(s)[-1], dict(kind="gn_sources_swapped", op=_two_source_norms(s)[-1]))),
    "two skips of equal shape exchanged": ("F", True, _skip_swap),
    "the ups conv applied at the input resolution": ("F", True, _at("ups_at_input_res", lambda m: m["kind"] == "conv" and m["ups"])),
    "a resnet reading its neighbour's temb_off": ("F", True, _neighbour_temb),
    "a cross-attention reading text rows at text_off - 1": ("H", True, _at("text_off_minus_1", lambda m: m["kind"] == "cross_attn")),
    "conv_out without its bias": ("F", True, _at("conv_out_no_bias", lambda m: m["kind"] == "conv_out")),
    "a HALF op writing row M/2": ("F", True, _at("half_writes_row", lambda m: m["kind"] == "linear" and pair_of(m) == "half")),
}


# =================================================================================================
# the constants of a run against fp64 (UNetEngine.prepare_timesteps / set_step / prepare_text / prepare_gligen)
# =================================================================================================
"""Every constant is a chain of stages: a GEMM (fp16 operands, fp32 accumulation) followed by a stated rounding — out_f32 keeps
fp32; SiLU runs in fp32; then .to(F16).  The reference carries, per element, a VALUE and a bound e on |device - value|.

The value is the fp64 result WITH THE ENGINE'S STORAGE ROUNDINGS APPLIED at exactly those points (weights to fp16, vectors to
fp32, activations to fp16 where the engine writes .to(F16) or an fp16 GEMM output): a storage rounding is deterministic, so it
belongs to the value, not to the error.  What remains is the fp32 arithmetic in between, and it is bounded stage by stage:

  input        fp32 inputs are exact.  A sinusoid cos / sin(arg) whose argument the device forms in fp32 has
               e = |arg| rel + 2^-23, rel = (|ln freq| + 1.5) 2^-23 for freq = exp(-ln(10000) i / half) (the product in the
               exponent, the exp, the product with t) and rel = 1.25 2^-22 for PositionNet's freq = 100^(i/8) (a pow).
  GEMM         the gemm_stmt bound on the operands as stored, plus the error of stage n entering through |W| err:
               e' = e |W|^T + (K + 8) 2^-23 ((|x| + e) |W|^T + |b|);  out_f32 keeps fp32: + 2^-24 (|v| + e').
  SiLU         in fp32: Lipschitz <= 1.1, evaluated to 4 ulp: e' = 1.1 e + 4 2^-24 |silu(v)|.
  a + b        fp32: e' = e_a + e_b + 2^-24 (|v| + e_a + e_b).
  .to(F16)     (and the fp16 store of a GEMM or LayerNorm)  value' = fp16(v).  Every real in (v - e, v + e) rounds to the same
               fp16 number unless that interval reaches a rounding tie: with r = fp16(v) and its neighbours r-, r+, if
               v - e > (r- + r) / 2 and v + e < (r + r+) / 2 the device stores r exactly, e' = 0; otherwise it may store a
               neighbour, e' = e + (r+ - r-).  (An exact input, e = 0, rounds as the value does.)
  LayerNorm    d y_i = gamma_i rstd (d x_i - mean(dx) - xhat_i mean(xhat dx)), so to first order
               e' = |gamma| rstd (e + mean(e) + |xhat| mean(|xhat| e)), times (1 + 4 rstd max e) for the remainder, plus
               layernorm_cases.fwd_ref's bound of the kernel without its fp16 store term; then the fp16 store as above.

Why the storage roundings are in the value: with them in the error (2^-11 |x| |W| per stage, propagated through |W| err) the
bound was measured vacuous — at the grounding tails (four GEMMs with K up to 832 and a LayerNorm) it came to 4e4 times the
values, and no wrong constant fell outside it.  The value at stored weights is tied to Setup.pure_constants (exact weights)
by rel-L2 on the CPU.  The same chain runs on an EMULATION backend: torch fp32 arithmetic, fp16 roundings at these points."""
import math  # noqa: E402


class E:
    """value (fp64 with the storage roundings applied) and bound of |device - value|"""

    def __init__(self, v, e=None):
        self.v = v.to(F64)
        self.e = torch.zeros_like(self.v) if e is None else e.to(F64)

    def reshape(self, *shape):
        return E(self.v.reshape(*shape), self.e.reshape(*shape))


def _fp16_neighbours(r):
    """the fp16 numbers below and above the fp16 values r (fp64 tensor), as fp64"""
    a = r.abs().to(H16)
    bits = a.view(torch.int16).to(torch.int32)
    up = (bits + 1).clamp_max(0x7BFF).to(torch.int16).view(H16).to(F64)
    dn = (bits - 1).clamp_min(0).to(torch.int16).view(H16).to(F64)
    dn = torch.where(bits == 0, torch.full_like(dn, -2.0 ** -24), dn)
    up = torch.where(bits >= 0x7BFF, a.to(F64) + 32.0, up)
    sgn = torch.where(r < 0, -1.0, 1.0)
    lo, hi = torch.minimum(sgn * dn, sgn * up), torch.maximum(sgn * dn, sgn * up)
    return lo, hi


def round16(x):
    r = x.v.to(H16).to(F64)
    lo, hi = _fp16_neighbours(r)
    safe = (x.e == 0) | ((x.v - x.e > 0.5 * (lo + r)) & (x.v + x.e < 0.5 * (r + hi)))
    return E(r, torch.where(safe, torch.zeros_like(x.e), x.e + (hi - lo)))


class RefB:
    ref = True

    def const(self, x):
        return E(x)

    def f32_param(self, x):
        return E(x.to(F32))

    def trig(self, arg, rel, fns):
        """fns of an fp32 argument with relative error rel [broadcast over arg]: list of E"""
        arg = arg.to(F64)
        e = arg.abs() * rel + 2.0 ** -23
        return [E(f(arg), e) for f in fns]

    def cat(self, xs, dim=-1):
        return E(torch.cat([x.v for x in xs], dim), torch.cat([x.e for x in xs], dim))

    def stack(self, xs, dim=-1):
        return E(torch.stack([x.v for x in xs], dim), torch.stack([x.e for x in xs], dim))

    def permute(self, x, *dims):
        return E(x.v.permute(*dims), x.e.permute(*dims))

    def mix(self, x, m, null):
        return E(x.v * m + (1 - m) * null.v, x.e * m + (1 - m) * null.e)

    def r16(self, x):
        return round16(x)

    def gemm(self, x, Wm, b, f32_out):
        Wm = Wm.to(H16).to(F64)
        K = Wm.shape[1]
        v = x.v @ Wm.t()
        s = (x.v.abs() + x.e) @ Wm.abs().t()
        e = x.e @ Wm.abs().t()
        if b is not None:
            b = b.to(F32).to(F64)
            v, s = v + b, s + b.abs()
        e = e + (K + 8) * 2.0 ** -23 * s
        return E(v, e + 2.0 ** -24 * (v.abs() + e)) if f32_out else round16(E(v, e))

    def silu(self, x):
        v = torch.nn.functional.silu(x.v)
        return E(v, 1.1 * x.e + 4 * 2.0 ** -24 * v.abs())

    def add_outer(self, h, a):
        """[T][1][C] + [1][R][C] -> [T * R][C]"""
        v = h.v[:, None] + a.v[None]
        e = h.e[:, None] + a.e[None]
        return E(v, e + 2.0 ** -24 * (v.abs() + e)).reshape(-1, v.shape[-1])

    def layernorm16(self, x, gamma, beta):
        g, bt = gamma.to(F32).to(F64), beta.to(F32).to(F64)
        r = lnc.fwd_ref(x.v, g, bt)
        own = r["bound"] - (2.0 ** -11 * r["y"].abs() + 2.0 ** -25)       # the kernel's fp32 part, without its fp16 store
        xh = (x.v - r["mean"]) * r["rstd"]
        prop = g.abs() * r["rstd"] * (x.e + x.e.mean(-1, keepdim=True) + xh.abs() * (xh.abs() * x.e).mean(-1, keepdim=True))
        rem = 1.0 + 4.0 * r["rstd"] * x.e.amax(-1, keepdim=True)
        return round16(E(r["y"], (own + prop) * rem))


class EmuB:
    """torch fp32 arithmetic, fp16 roundings where the engine rounds"""
    ref = False

    def const(self, x):
        return x.to(F32)

    f32_param = const

    def trig(self, arg, rel, fns):
        return [f(arg.to(F32)) for f in fns]

    def cat(self, xs, dim=-1):
        return torch.cat(xs, dim)

    def stack(self, xs, dim=-1):
        return torch.stack(xs, dim)

    def permute(self, x, *dims):
        return x.permute(*dims)

    def mix(self, x, m, null):
        m = m.to(F32)
        return x * m + (1 - m) * null

    def r16(self, x):
        return x.to(H16).to(F32)

    def gemm(self, x, Wm, b, f32_out):
        y = x.to(H16).to(F32) @ Wm.to(H16).to(F32).t()
        if b is not None:
            y = y + b.to(F32)
        return y if f32_out else y.to(H16).to(F32)

    def silu(self, x):
        return torch.nn.functional.silu(x)

    def add_outer(self, h, a):
        return (h[:, None] + a[None]).reshape(-1, h.shape[-1])

    def layernorm16(self, x, gamma, beta):
        mean = x.mean(-1, keepdim=True)
        rstd = torch.rsqrt(((x - mean) ** 2).mean(-1, keepdim=True) + torch.tensor(lnc.EPS, dtype=F32))
        return ((x - mean) * rstd * gamma.to(F32) + beta.to(F32)).to(H16).to(F32)


def _lin(sd, name):
    return sd[f"{name}.weight"], sd.get(f"{name}.bias")


def _sinusoid(be, t, dim, swapped=False):
    """Timesteps(dim, flip_sin_to_cos=True, shift 0) of the values t [n] as the engine forms it: [n][dim] = [cos | sin]"""
    half = dim // 2
    if be.ref:
        a = -math.log(10000.0) * torch.arange(half, dtype=F64) / half
        arg, rel = t.to(F64)[:, None] * torch.exp(a)[None], ((a.abs() + 1.5) * 2.0 ** -23)[None]
    else:
        freqs = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=F32) / half)
        arg, rel = t.to(F32)[:, None] * freqs[None], None
    c, s_ = be.trig(arg, rel, [torch.cos, torch.sin])
    return be.cat([s_, c] if swapped else [c, s_])


def temb_tables(be, cfg, sd, timesteps, added=None, wrong=None):
    """{resnet prefix: [T * R][Cout]} — the time-embedding projection of every resnet for every timestep (and image)"""
    t = torch.as_tensor(list(timesteps), dtype=F32)
    x = be.r16(_sinusoid(be, t, cfg.block_out_channels[0], swapped=wrong == "sincos"))
    h = be.gemm(x, *_lin(sd, "time_embedding.linear_1"), True)
    h = be.gemm(be.r16(be.silu(h)), *_lin(sd, "time_embedding.linear_2"), True)
    if added is not None:
        te, ids = added["text_embeds"].to(F32), added["time_ids"].to(F32)
        tid = _sinusoid(be, ids.reshape(-1), cfg.addition_time_embed_dim)
        tid = tid.reshape(ids.shape[0], -1)
        a = be.r16(be.cat([be.const(te), tid]))
        a = be.gemm(a, *_lin(sd, "add_embedding.linear_1"), True)
        a = be.gemm(be.r16(be.silu(a)), *_lin(sd, "add_embedding.linear_2"), True)
        h = be.add_outer(h, a)
    h = be.r16(be.silu(h))
    return {r.prefix: be.gemm(h, *_lin(sd, f"{r.prefix}.time_emb_proj"), True)
            for b in weights.unet_blocks(cfg) for r in b.resnets}


def text_kv(be, cfg, sd, ehs, wrong=None):
    """{kv_name: [Bt * T][2C]} — [K | V] of every cross-attention layer, the "@d" layers of deeper blocks included"""
    x = be.r16(be.const(ehs.reshape(-1, ehs.shape[-1])))
    out = {}
    for b in weights.unet_blocks(cfg):
        for a in b.attns:
            for dpt in range(a.depth):
                t = f"{a.prefix}.transformer_blocks.{dpt}.attn2"
                ws = [sd[f"{t}.to_k.weight"], sd[f"{t}.to_v.weight"]]
                out[UNetEngine.kv_name(a.prefix, dpt)] = be.gemm(x, torch.cat(ws[::-1] if wrong == "kv" else ws, 0), None, False)
    return out


def position_net_objs(be, cfg, sd, boxes, masks, emb, wrong=None):
    """[Bt * 30][Cx] — PositionNet (the engine keeps it as UNetEngine._objs, fp16)"""
    Bt = boxes.shape[0]
    m = masks.to(F64 if be.ref else F32).unsqueeze(-1)
    if wrong == "null":
        m = 1 - m
    base = 10000.0 if wrong == "freq" else 100.0
    if be.ref:
        freq = base ** (torch.arange(8, dtype=F64) / 8)
        arg, rel = freq[None, None, None] * boxes.to(F64).unsqueeze(-1), 1.25 * 2.0 ** -22
    else:
        freq = (base ** (torch.arange(8) / 8)).float()
        arg, rel = freq[None, None, None] * boxes.to(F32).unsqueeze(-1), None
    s_, c = be.trig(arg, rel, [torch.sin, torch.cos])                     # [Bt][30][4][8]
    xyxy = be.permute(be.stack([s_, c]), 0, 1, 3, 4, 2).reshape(Bt, N_OBJ_TOKENS, -1)
    pos = be.mix(be.const(emb), m, be.f32_param(sd["position_net.null_positive_feature"].reshape(1, 1, -1)))
    xyxy = be.mix(xyxy, m, be.f32_param(sd["position_net.null_position_feature"].reshape(1, 1, -1)))
    h = be.r16(be.cat([pos, xyxy]).reshape(Bt * N_OBJ_TOKENS, -1))
    h = be.r16(be.silu(be.gemm(h, *_lin(sd, "position_net.linears.0"), True)))
    h = be.r16(be.silu(be.gemm(h, *_lin(sd, "position_net.linears.2"), True)))
    return be.gemm(h, *_lin(sd, "position_net.linears.4"), False)


def grounding_tails(be, cfg, sd, objs, Bt):
    """{kv_name: [Bt][30][C]} — fuser.linear and fuser.norm1 of every fuser layer on the grounding tokens objs"""
    out = {}
    for b in weights.unet_blocks(cfg):
        for a in b.attns:
            for dpt in range(a.depth):
                f = f"{a.prefix}.transformer_blocks.{dpt}.fuser"
                o = be.gemm(objs, *_lin(sd, f"{f}.linear"), False)
                o = be.layernorm16(o, sd[f"{f}.norm1.weight"], sd[f"{f}.norm1.bias"])
                out[UNetEngine.kv_name(a.prefix, dpt)] = o.reshape(Bt, N_OBJ_TOKENS, -1)
    return out


def const_ratio(got, ref):
    """worst |got - value| / bound of one constant"""
    return sk.worst_ratio(got.reshape(ref.v.shape), ref.v.to(got.device), ref.e.to(got.device), fp16=False)


TIMESTEPS = [981, 601, 1]
EMB_SCALE = 0.0625


def constant_inputs(cfg, seed=77):
    """the inputs of the constants tests: text batch Bt = 3, R = 2 images of a text_time model, Bt = 4 grounding rows with
    the first half masked out (the null features) and 3 of the 30 tokens in use"""
    g = torch.Generator().manual_seed(seed)
    d = dict(ehs=torch.randn(3, 77, cfg.cross_attention_dim, generator=g))
    if cfg.addition_embed_type == "text_time":
        d["added"] = dict(text_embeds=torch.randn(2, cfg.pooled_dim, generator=g),
                          time_ids=torch.tensor([[32.0, 32.0, 0.0, 0.0, 6.0], [48.0, 24.0, 4.0, 8.0, 2.5]]))
    if cfg.use_gated_attention:
        Bt = GLIGEN_BT
        boxes, masks = torch.zeros(Bt, N_OBJ_TOKENS, 4), torch.zeros(Bt, N_OBJ_TOKENS)
        xy = torch.rand(Bt, 3, 2, generator=g) * 0.5
        boxes[:, :3] = torch.cat([xy, xy + 0.1 + 0.4 * torch.rand(Bt, 3, 2, generator=g)], -1)
        masks[Bt // 2:, :3] = 1.0
        masks[Bt - 1, 1] = 0.0                                           # a masked-out box between two live ones
        emb = torch.zeros(Bt, N_OBJ_TOKENS, cfg.gligen_positive_len)
        emb[:, :3] = torch.randn(Bt, 3, cfg.gligen_positive_len, generator=g) * EMB_SCALE
        d["gligen"] = dict(boxes=boxes, masks=masks, positive_embeddings=emb)
    return d

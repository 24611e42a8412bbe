"""The UNet reverse plan (lgd_amd/unet.py: Plan.linear .. Plan.ff, _finalize_backward, Plan.backward) as test data.

A grad plan describes itself (Op.meta).  From the metas this module builds
  * the GRAPH: which op reads and writes which activation, with its views and geometry;
  * per op kind an fp64 STATEMENT of the forward and of the vector-Jacobian product, each with the per-element bound the
    kernel family's own conformance module derives (nothing new is derived here, nothing is fitted):
        GEMM / conv / shortcut   gemm_conformance_cases: _gather3x3 and the bound of Case — restated (`gemm_stmt`), because Case
                                 builds its own operands and cannot be called with operands as given:
                                 2^-11 |v| + 2^-25 + (K + 8) 2^-23 (|alpha| s + |residual|), s = sum |products| + |biases|
        attention                attn_conformance_cases.fwd_reference / bwd_reference (sk_grad) / xbwd_reference (gp, go = None)
        GroupNorm                groupnorm_conformance_cases.fwd_reference / bwd_reference
        LayerNorm                layernorm_cases.fwd_ref / bwd_ref
        GEGLU, the 2x2 sum, the layout converter, conv_in's input gradient, add, copy
                                 small_kernel_cases (Geglu, Upsample, Nhwc8, ConvOut, Elementwise)
    The folded-upsample dgrad is two kernels: its fp16 `tmp` is checked with the GEMM bound and the 2x2 sum with the
    Upsample bound on tmp as given.  Weights come from the state dict BY NAME (rounded as the store rounds them: matrices
    to fp16, vectors to fp32), never from the packed .w / .wt / .wd buffers: the packing is part of what is checked;
  * the CHAIN: the statements composed over the graph in fp64 — `pure` (exact weights and constants: compared with
    oracle/restate.py and torch.autograd) or at activations as given (the yardstick of the device's latent gradient);
  * the WALKER: runs a plan op by op on poisoned buffers, checks every output against its statement with inputs as given,
    and proves integrity (an op changes the bits of its declared outputs, gradient outputs and scratch only) and
    completeness (every non-constant input on a path from the latents to a saved map receives a gradient);
  * the EMULATOR: every op in fp32 with fp16 storage, reading the PACKED weights like the kernels do and writing the plan's
    own buffers on a host engine, so that the walker — and wrong plans (MUTANTS) — run without a GPU.

Intentional cuts (constants of a run, no gradient): the text K/V, the time embedding, the 30 grounding rows of the fuser's
concat buffer (their gradient rows are cleared) and, at the last key, the attention output."""
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "oracle"), os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import lgd_amd  # noqa: E402,F401
import restate as R  # noqa: E402
from lgd_amd import ops, weights  # noqa: E402
from lgd_amd.unet import N_OBJ_TOKENS, Act, UNetEngine  # noqa: E402

import attn_conformance_cases as attn  # noqa: E402
import groupnorm_conformance_cases as gn  # noqa: E402
import layernorm_cases as lnc  # noqa: E402
import small_kernel_cases as sk  # noqa: E402
from gemm_conformance_cases import _gather3x3  # noqa: E402

H16, F32, F64 = torch.float16, torch.float32, torch.float64
U, W = 2.0 ** -11, 2.0 ** -24
L = 32
T0 = 601                        # the timestep of every case
DEFAULT_KEYS = [("mid", 0, 0, 0), ("up", 1, 0, 0), ("up", 1, 1, 0), ("up", 1, 2, 0)]
# text_off / obj_off as LMDSampler._guide_pass passes them: the conditional half of the text batch, the zero-masked GLIGEN half
CASES = {
    "A": dict(cfg="tiny", B=2, keys=DEFAULT_KEYS, text_off=1),
    "B": dict(cfg="tiny_gligen", B=3, keys=DEFAULT_KEYS, text_off=3, fuser=True),
    "C": dict(cfg="tiny_sd21", B=2, keys=DEFAULT_KEYS, text_off=2),
    "D": dict(cfg="tiny", B=2, keys=[("down", 1, 1, 0), ("mid", 0, 0, 0)], text_off=2),
    "E": dict(cfg="tiny", B=2, keys=[("down", 0, 0, 0)], text_off=2),
}
# power-of-two scale of the map cotangents per case (sensitivity condition, tests/test_unet_plan_cpu.py)
COT_SCALE = {"A": 2.0 ** 9, "B": 2.0 ** 9, "C": 2.0 ** 9, "D": 2.0 ** 9, "E": 2.0 ** 9}
GRAD_SCALE = 4.0                # Plan.backward(grad_scale): the latent gradient is divided by it


def _ns(**kw):
    return types.SimpleNamespace(**kw)


def rel_l2(a, b):
    a, b = a.to(F64).reshape(-1).cpu(), b.to(F64).reshape(-1).cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


# =================================================================================================
# a case: engine, plan, inputs, constants
# =================================================================================================
class Setup:
    def __init__(self, case, device="cpu", build_plan=True):
        c = CASES[case]
        self.case, self.c = case, c
        self.cfg = weights.CONFIGS[c["cfg"]]
        self.sd = weights.synth_state_dict(self.cfg, 0)
        self.sd64 = {k: v.to(F64) for k, v in self.sd.items()}
        self.device = torch.device(device)
        self.eng = UNetEngine(self.cfg, self.device, self.sd)
        self.B, self.keys, self.text_off, self.fuser = c["B"], [tuple(k) for k in c["keys"]], c["text_off"], c.get("fuser", False)
        self.obj_off = c.get("obj_off", 0)
        g = torch.Generator().manual_seed(1234 + sum(map(ord, case)))
        B = self.B
        self.lat = torch.randn(B, self.cfg.in_channels, L, L, generator=g)
        self.ehs = torch.randn(self.text_off + B, self.eng.text_len, self.cfg.cross_attention_dim, generator=g)
        self.gligen = None
        if self.fuser:
            boxes = torch.zeros(2 * B, N_OBJ_TOKENS, 4)
            masks = torch.zeros(2 * B, N_OBJ_TOKENS)
            xy = torch.rand(2 * B, 3, 2, generator=g) * 0.5
            boxes[:, :3] = torch.cat([xy, xy + 0.1 + 0.4 * torch.rand(2 * B, 3, 2, generator=g)], -1)
            masks[B:, :3] = 1.0                                          # pipelines.py:317: the first half is zero-masked
            emb = torch.zeros(2 * B, N_OBJ_TOKENS, self.cfg.gligen_positive_len)
            emb[:, :3] = torch.randn(2 * B, 3, self.cfg.gligen_positive_len, generator=g)
            self.gligen = dict(boxes=boxes, masks=masks, positive_embeddings=emb)
        self.stop = self.eng.last_key(self.keys)
        self.plan = self.graph = None
        if build_plan:
            self.plan = self.eng.plan(B, L, grad=True, fuser=self.fuser, stop_key=self.stop, save_keys=self.keys,
                                      text_batch_offset=self.text_off, obj_batch_offset=self.obj_off)
            self.graph = Graph(self.plan)
            self.install_constants()
        self.cot = {k: (torch.randn(B, self._heads(k), self._hw(k), self.eng.text_len, generator=g) * COT_SCALE[case]).to(F32)
                    for k in self.keys} if build_plan else None

    def _node(self, key):
        return next(m for m in self.graph.metas if m["kind"] == "cross_attn" and m["key"] == key)

    def _heads(self, key):
        return self._node(key)["heads"]

    def _hw(self, key):
        return self._node(key)["S"]

    # ---- the constants of a run -----------------------------------------------------------------
    def pure_constants(self, sd=None):
        """fp64, from the restatement's own functions: temb_act = silu(time embedding) [1][ted]; text K/V per layer;
        grounding rows per layer (position_net, fuser.linear, fuser.norm1)."""
        sd = self.sd64 if sd is None else sd
        Fn = torch.nn.functional
        emb = R.timestep_embedding(torch.tensor([T0]), self.cfg.block_out_channels[0], F64)
        emb = Fn.linear(emb, sd["time_embedding.linear_1.weight"], sd["time_embedding.linear_1.bias"])
        emb = Fn.linear(Fn.silu(emb), sd["time_embedding.linear_2.weight"], sd["time_embedding.linear_2.bias"])
        out = dict(temb_act=Fn.silu(emb), kv={}, tail={})
        ehs = self.ehs.to(F64)[self.text_off:self.text_off + self.B]
        objs = None
        if self.gligen is not None:
            gl = {k: v.to(F64)[self.obj_off:self.obj_off + self.B] for k, v in self.gligen.items()}
            objs = R.position_net(sd, gl["boxes"], gl["masks"], gl["positive_embeddings"])
        for m in self.graph.metas:
            if m["kind"] == "cross_attn":
                wk, wv = (sd[n] for n in m["params"]["kv"])
                out["kv"][m["layer"]] = torch.cat([Fn.linear(ehs, wk), Fn.linear(ehs, wv)], -1)
            if m["kind"] == "layernorm" and m["S"]:
                f = m["name"][:-len(".norm1")]
                o = Fn.linear(objs, sd[f"{f}.linear.weight"], sd[f"{f}.linear.bias"])
                out["tail"][id(m["out"])] = R.layer_norm(sd, f"{f}.norm1", o)
        return out

    def install_constants(self):
        eng = self.eng
        if self.device.type == "cuda":
            eng.prepare_timesteps([T0])
            eng.set_step(0)
            eng.prepare_text(self.ehs)
            if self.gligen is not None:
                eng.prepare_gligen(self.gligen["boxes"], self.gligen["masks"], self.gligen["positive_embeddings"])
        else:
            # a host engine has no kernels to prepare them with: the fp64 constants, rounded to their storage types
            pc = self.pure_constants()
            for m in self.graph.metas:
                if m["kind"] == "conv" and m["temb_off"] is not None:
                    p = m["name"][:-len(".conv1")]
                    v = torch.nn.functional.linear(pc["temb_act"], self.sd64[f"{p}.time_emb_proj.weight"], self.sd64[f"{p}.time_emb_proj.bias"])
                    eng.temb_cur[0, m["temb_off"]:m["temb_off"] + v.shape[1]] = v[0].to(F32)
                if m["kind"] == "cross_attn":
                    m["kv"][:self.B].copy_(pc["kv"][m["layer"]].to(H16))
                if m["kind"] == "layernorm" and m["S"]:
                    S = m["S"]
                    m["out"].t.view(self.B, S + N_OBJ_TOKENS, -1)[:, S:] = pc["tail"][id(m["out"])].to(H16)
        self.tails0 = {id(m["out"]): m["out"].t.view(self.B, m["S"] + N_OBJ_TOKENS, -1)[:, m["S"]:].clone()
                       for m in self.graph.metas if m["kind"] == "layernorm" and m["S"]}

    def restate_cfg(self):
        c = self.cfg
        return dict(block_out_channels=c.block_out_channels, layers_per_block=c.layers_per_block,
                    attention_head_dim=c.attention_head_dim if isinstance(c.attention_head_dim, (tuple, list)) else
                    [c.attention_head_dim] * len(c.block_out_channels), norm_num_groups=c.norm_num_groups, norm_eps=c.norm_eps)


# =================================================================================================
# (a) the graph
# =================================================================================================
KINDS = ("conv_in", "linear", "conv", "shortcut", "groupnorm", "layernorm", "self_attn", "cross_attn", "geglu", "conv_out")


class Graph:
    def __init__(self, plan):
        self.plan = plan
        self.metas = []
        for i, op in enumerate(plan.ops):
            m = op.meta
            assert isinstance(m, dict) and m.get("kind") in KINDS, f"op {i} carries no meta"
            self.metas.append(m)
            if op.bwd is not None:
                assert op.gouts, f"op {i} ({m['kind']}) has a backward and lists no gouts"
        assert getattr(plan, "bwd_tail_meta", None) is not None and plan.bwd_tail_meta["kind"] == "conv_in_dgrad"
        self.names = {id(a): n for n, a in plan.dbg.items()}

    def label(self, i):
        m = self.metas[i]
        return f"op {i} {m['kind']}" + (f" {m['name']}" if "name" in m else (f" {m['key']}" if "key" in m else ""))

    @staticmethod
    def inputs(m):
        """every Act the op reads: its sources and its residual"""
        return [a for a in m["ins"] if isinstance(a, Act)] + ([m["res"]] if m.get("res") is not None else [])

    def on_path(self):
        """indices of the ops whose output lies on a path from the latents to a saved map"""
        plan = self.plan
        needed, ops_on = set(), set()
        for i in reversed(range(len(self.metas))):
            m = self.metas[i]
            is_map = m["kind"] == "cross_attn" and m["key"] in plan.save_keys
            if is_map or id(m["out"]) in needed:
                ops_on.add(i)
                # what reaches a map through this op: all inputs if its output is needed; q alone for the map itself
                for a in self.inputs(m):
                    needed.add(id(a))
        return ops_on

    def completeness(self, gouts_of=None):
        """violations: (op label, what is missing)"""
        plan, bad = self.plan, []
        for i in sorted(self.on_path()):
            m, op = self.metas[i], plan.ops[i]
            if m["kind"] == "conv_in":
                continue                                   # its input gradient is the tail of Plan.backward
            gouts = (gouts_of or {}).get(i, op.gouts)
            if op.make_bwd is None:
                bad.append((self.label(i), "no backward"))
            have = {id(a) for a in gouts}
            for a in self.inputs(m):
                if id(a) not in have:
                    bad.append((self.label(i), f"input {self.names.get(id(a), 'activation')} [{a.rows} x {a.C}] is not in gouts"))
        return bad


# =================================================================================================
# weights by name
# =================================================================================================
class Ctx:
    """pure: exact fp64 parameters and constants.  Otherwise the parameters rounded as the store holds them (matrices fp16,
    vectors fp32) and the constants as given in the engine's buffers."""

    def __init__(self, setup, pure):
        self.s, self.pure, self.dev = setup, pure, (torch.device("cpu") if pure else setup.device)
        self._c = {}
        self.pc = setup.pure_constants() if pure else None

    def mat(self, names, geglu_rows=False):
        key = (tuple(names), geglu_rows)
        if key not in self._c:
            ws = []
            for n in names:
                w = self.s.sd64[n]
                ws.append(w if self.pure else w.to(H16).to(F64))
            w = torch.cat(ws, 0)
            if w.dim() == 4 and w.shape[2] == 1:
                w = w.reshape(w.shape[0], w.shape[1])
            if geglu_rows:
                w = self.geglu_pack(w)
            self._c[key] = w.to(self.dev)
        return self._c[key]

    def vec(self, name, geglu_rows=False):
        key = (name, geglu_rows, "v")
        if key not in self._c:
            v = self.s.sd64[name]
            v = v if self.pure else v.to(F32).to(F64)
            self._c[key] = (self.geglu_pack(v) if geglu_rows else v).to(self.dev)
        return self._c[key]

    @staticmethod
    def geglu_pack(w):
        """rows in the packed order of include/lgd_hip.h: [16 value | 16 gate] blocks (small_kernel_cases.geglu_positions)"""
        n = w.shape[0] // 2
        pv, pg = sk.geglu_positions(n)
        out = torch.empty_like(w)
        out[pv], out[pg] = w[:n], w[n:]
        return out

    def alpha(self, m):
        n = m["params"].get("alpha")
        if n is None or not self.pure:
            return float(m["alpha"])
        return float(self.s.sd64[n].tanh())

    def temb(self, m):
        if m.get("temb_off") is None:
            return None
        p = m["name"][:-len(".conv1")]
        if self.pure:
            sd = self.s.sd64
            return torch.nn.functional.linear(self.pc["temb_act"], sd[f"{p}.time_emb_proj.weight"], sd[f"{p}.time_emb_proj.bias"])[0]
        n = m["out"].C
        return self.s.eng.temb_cur[0, m["temb_off"]:m["temb_off"] + n].to(F64)

    def kv(self, m):
        return self.pc["kv"][m["layer"]] if self.pure else m["kv"][:self.s.B].to(F64)

    def tail(self, m):
        return self.pc["tail"][id(m["out"])] if self.pure else self.s.tails0[id(m["out"])].to(F64)


# =================================================================================================
# (b) the statements.  ins: fp64 tensors of the op's sources; saved: what the forward left, as given
# =================================================================================================
def gemm_stmt(A, Wm, bias=None, bias2=None, alpha=1.0, res=None):
    """gemm_conformance_cases.Case restated for operands as given: value and bound of C = alpha (A W^T + biases) + res"""
    K = A.shape[1]
    v, s = A @ Wm.t(), A.abs() @ Wm.abs().t()
    for b in (bias, bias2):
        if b is not None:
            v, s = v + b, s + b.abs()
    e = (K + 8) * 2.0 ** -23 * s * abs(alpha)
    v = v * alpha
    if res is not None:
        v, e = v + res, e + (K + 8) * 2.0 ** -23 * res.abs()
    return v, 2.0 ** -11 * v.abs() + 2.0 ** -25 + e


def _gather(x, *geom):
    return _gather3x3(x.cpu(), *geom).to(x.device)


def pack_fwd(w):
    """[Cout][Cin][3][3] -> [Cout][(ky, kx, ci)]   (weightstore docstring)"""
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1)


def pack_dgrad(w):
    """Wd[ci][(ky', kx', co)] = W[co][ci][2 - ky'][2 - kx']   (weightstore docstring)"""
    return w.flip(2, 3).permute(1, 2, 3, 0).reshape(w.shape[1], -1)


def _passthrough(gy, base):
    """d/d res of y = f(x) + res: a copy (bit-exact) or, accumulating, small_kernel_cases' add"""
    if base is None:
        return gy, torch.zeros_like(gy)
    y = sk.V(gy) + sk.V(base)
    return y.v, sk.r16(y)


def _with_base(v, base):
    return v if base is None else v + base


# ---- linear / shortcut / conv --------------------------------------------------------------------
def fwd_linear(m, ins, cx, saved=None):
    p = m["params"]
    M = m["rows"]
    Wm = cx.mat(p["weight"], p["geglu_rows"])
    b = cx.vec(p["bias"], p["geglu_rows"]) if p["bias"] else None
    res = ins[1][:M] if m["res"] is not None else None
    assert not m["geglu_epilogue"]
    return dict(out=gemm_stmt(ins[0][:M], Wm, b, alpha=cx.alpha(m), res=res))


def vjp_linear(m, ins, saved, gy, cx, bases):
    p = m["params"]
    M = m["rows"]
    Wm = cx.mat(p["weight"], p["geglu_rows"])
    out = [gemm_stmt(gy[:M], Wm.t(), alpha=cx.alpha(m), res=bases[0])]
    if m["res"] is not None:
        out.append(_passthrough(gy, bases[1]))
    return out, {}


def fwd_shortcut(m, ins, cx, saved=None):
    p = m["params"]
    return dict(out=gemm_stmt(torch.cat(ins, 1), cx.mat(p["weight"]), cx.vec(p["bias"])))


def vjp_shortcut(m, ins, saved, gy, cx, bases):
    Wm = cx.mat(m["params"]["weight"])
    out, lo = [], 0
    for x, base in zip(ins, bases):
        cn = x.shape[1]
        out.append(gemm_stmt(gy, Wm[:, lo:lo + cn].t(), res=base))
        lo += cn
    return out, {}


def _conv_geom(m, B):
    H, stride = m["H"], m["stride"]
    Hl = 2 * H if m["ups"] else H
    Ho = (Hl - 1) // stride + 1
    return H, Hl, Ho, stride


def fwd_conv(m, ins, cx, saved=None):
    p = m["params"]
    n_src = len(m["ins"])
    B = ins[0].shape[0] // (m["H"] ** 2)
    H, Hl, Ho, stride = _conv_geom(m, B)
    srcs = [_gather(x, B, H, H, Ho, Ho, stride, 1 if m["ups"] else 0).reshape(B * Ho * Ho, 9, -1) for x in ins[:n_src]]
    A = torch.cat(srcs, 2).reshape(B * Ho * Ho, -1)
    res = ins[n_src] if m["res"] is not None else None
    return dict(out=gemm_stmt(A, pack_fwd(cx.mat(p["weight"])), cx.vec(p["bias"]), cx.temb(m), res=res))


def vjp_conv(m, ins, saved, gy, cx, bases):
    n_src = len(m["ins"])
    B = ins[0].shape[0] // (m["H"] ** 2)
    H, Hl, Ho, stride = _conv_geom(m, B)
    Wd = pack_dgrad(cx.mat(m["params"]["weight"]))                       # [Cin][9 Cout]
    out, extra = [], {}
    if stride == 1 and not m["ups"]:
        A = _gather(gy, B, H, H, H, H, 1, 0)
        lo = 0
        for x, base in zip(ins[:n_src], bases):
            cn = x.shape[1]
            out.append(gemm_stmt(A, Wd[lo:lo + cn], res=base))
            lo += cn
    elif stride == 2:
        out.append(gemm_stmt(_gather(gy, B, Ho, Ho, H, H, 1, 2), Wd, res=bases[0]))
    else:
        assert bases[0] is None
        tmp = gemm_stmt(_gather(gy, B, Hl, Hl, Hl, Hl, 1, 0), Wd)
        extra["tmp"] = tmp
        c0 = Wd.shape[0]
        given = saved.get("tmp", tmp[0]).reshape(B, Hl * Hl, c0)     # the 2x2 sum takes the fp16 tmp as given
        out.append(sk.Upsample().reference(_ns(B=B, H=H, W=H, C=c0), {"gy": given})["gx"])
        out[-1] = (out[-1][0].reshape(-1, c0), out[-1][1].reshape(-1, c0))
    if m["res"] is not None:
        out.append(_passthrough(gy, bases[-1]))
    return out, extra


# ---- norms -----------------------------------------------------------------------------------------
def _gn_row(m, op, c0, c1, B):
    code = ops.groupnorm_plan(ops.GN_OP_FWD if op == "fwd" else ops.GN_OP_BWD, c0, c1, B, m["HW"], m["G"], silu=m["silu"])
    return gn.Row(code, op, c0, c1, m["HW"], B, G=m["G"], silu=m["silu"])


def fwd_groupnorm(m, ins, cx, saved=None):
    p = m["params"]
    x = torch.cat(ins, 1)
    B = x.shape[0] // m["HW"]
    row = _gn_row(m, "fwd", ins[0].shape[1], ins[1].shape[1] if len(ins) > 1 else 0, B)
    r = gn.fwd_reference(x.reshape(B, m["HW"], -1), cx.vec(p["weight"]), cx.vec(p["bias"]), m["G"], m["eps"], m["silu"],
                         depth=row.depth, two_launch=row.two_launch)
    return dict(out=(r["y"].reshape(x.shape), r["bound_y"].reshape(x.shape)),
                stats=(torch.stack([r["mean"], r["rstd"]], -1), torch.stack([r["bound_mean"], r["bound_rstd"]], -1)))


def vjp_groupnorm(m, ins, saved, gy, cx, bases):
    p = m["params"]
    x = torch.cat(ins, 1)
    B, HW = x.shape[0] // m["HW"], m["HW"]
    c0 = ins[0].shape[1]
    row = _gn_row(m, "bwd", c0, ins[1].shape[1] if len(ins) > 1 else 0, B)
    assert all((b is None) == (bases[0] is None) for b in bases)
    base = torch.cat(bases, 1).reshape(B, HW, -1) if bases[0] is not None else None
    st = saved["stats"]
    r = gn.bwd_reference(x.reshape(B, HW, -1), gy.reshape(B, HW, -1), cx.vec(p["weight"]), cx.vec(p["bias"]), st[..., 0], st[..., 1],
                         m["G"], m["silu"], depth=row.depth, slab=row.slab, base=base)
    dx, bd = r["dx"].reshape(x.shape), r["bound_dx"].reshape(x.shape)
    out = [(dx[:, :c0], bd[:, :c0])]
    if len(ins) > 1:
        out.append((dx[:, c0:], bd[:, c0:]))
    return out, {}


def fwd_layernorm(m, ins, cx, saved=None):
    p = m["params"]
    x = ins[0][:m["rows"]]
    r = lnc.fwd_ref(x, cx.vec(p["weight"]), cx.vec(p["bias"]))
    y, bd = r["y"], r["bound"]
    if m["S"]:                                            # the rows of each image at the head of its [S + 30] block
        S, C = m["S"], x.shape[1]
        B = x.shape[0] // S
        full = torch.zeros(B, S + N_OBJ_TOKENS, C, dtype=F64, device=x.device)
        fb = torch.zeros_like(full)
        full[:, :S], fb[:, :S] = y.reshape(B, S, C), bd.reshape(B, S, C)
        full[:, S:] = cx.tail(m).to(x.device)             # constants of the run: unchanged, bit for bit
        y, bd = full.reshape(-1, C), fb.reshape(-1, C)
    return dict(out=(y, bd), stats=(torch.cat([r["mean"], r["rstd"]], 1), torch.cat([r["bound_mean"], r["bound_rstd"]], 1)))


def vjp_layernorm(m, ins, saved, gy, cx, bases):
    x = ins[0][:m["rows"]]
    if m["S"]:
        S, C = m["S"], x.shape[1]
        gy = gy.reshape(-1, S + N_OBJ_TOKENS, C)[:, :S].reshape(-1, C)
    st = saved["stats"]
    return [lnc.bwd_ref(x, gy, cx.vec(m["params"]["weight"]), st[:, 0:1], st[:, 1:2], bases[0])], {}


# ---- attention ---------------------------------------------------------------------------------------
def _heads(t, B, H):
    """[B * S][H * d] -> [B][H][S][d]"""
    return t.reshape(B, -1, H, t.shape[-1] // H).permute(0, 2, 1, 3)


def _rows(t):
    """[B][H][S][d] -> [B * S][H * d]"""
    B, H, S, d = t.shape
    return t.permute(0, 2, 1, 3).reshape(B * S, H * d)


def _attn_row(op, m, B, probs=False):
    code = ops.attn_plan({"self": ops.ATTN_OP_FWD, "map": ops.ATTN_OP_FWD, "bwd": ops.ATTN_OP_BWD, "xbwd": ops.ATTN_OP_CROSS_BWD}[op],
                         B, m["heads"], m["S"], m["Sk"], m["d"], sk_grad=m["S"] if op == "bwd" else None, probs=probs)
    return attn.Row(code, op, B, m["heads"], m["d"], Sq=m["S"], Sk=m["Sk"], sk_grad=m["S"] if op == "bwd" else None)


def _self_qkv(m, qkv):
    S, Sk, H = m["S"], m["Sk"], m["heads"]
    C = qkv.shape[1] // 3
    B = qkv.shape[0] // Sk
    t = qkv.reshape(B, Sk, 3 * C)
    q = _heads(t[:, :S, :C].reshape(B * S, C), B, H)
    k = _heads(t[:, :, C:2 * C].reshape(B * Sk, C), B, H)
    v = _heads(t[:, :, 2 * C:].reshape(B * Sk, C), B, H)
    return B, C, q, k, v


def _per_image(fn, B, names):
    """the module references on one image at a time (the score matrices of 1024 x 1024 x heads in fp64 stay small)"""
    parts = [fn(b) for b in range(B)]
    return {n: torch.stack([p[n] for p in parts]) for n in names}


def fwd_self_attn(m, ins, cx, saved=None):
    B, C, q, k, v = _self_qkv(m, ins[0])
    row = _attn_row("self", m, B)
    r = _per_image(lambda b: attn.fwd_reference(q[b], k[b], v[b], m["scale"], DP=row.DP, ones=row.ones), B,
                   ("o", "lse", "bound_o", "bound_lse"))
    return dict(out=(_rows(r["o"]), _rows(r["bound_o"])), lse=(r["lse"], r["bound_lse"]))


def vjp_self_attn(m, ins, saved, gy, cx, bases):
    assert bases[0] is None
    S, Sk, H = m["S"], m["Sk"], m["heads"]
    B, C, q, k, v = _self_qkv(m, ins[0])
    row = _attn_row("bwd", m, B)
    go, o = _heads(gy, B, H), _heads(saved["out"], B, H)
    names = ("gq", "gk", "gv", "delta", "bound_gq", "bound_gk", "bound_gv", "bound_delta")
    r = _per_image(lambda b: attn.bwd_reference(q[b], k[b], v[b], go[b], o[b], saved["lse"][b], m["scale"], DP=row.DP, sk_grad=S),
                   B, names)
    g = torch.zeros(B, Sk, 3 * C, dtype=F64, device=gy.device)           # the rows of the grounding tokens: cleared whole
    bd = torch.zeros_like(g)
    for j, n in enumerate(("gq", "gk", "gv")):
        g[:, :S, j * C:(j + 1) * C] = _rows(r[n]).reshape(B, S, C)
        bd[:, :S, j * C:(j + 1) * C] = _rows(r["bound_" + n]).reshape(B, S, C)
    return [(g.reshape(B * Sk, 3 * C), bd.reshape(B * Sk, 3 * C))], {"delta": (r["delta"], r["bound_delta"])}


def _cross_qkv(m, qx, cx):
    H = m["heads"]
    B = qx.shape[0] // m["S"]
    C = qx.shape[1]
    kv = cx.kv(m).to(qx.device)
    return B, _heads(qx, B, H), _heads(kv[:, :, :C].reshape(-1, C), B, H), _heads(kv[:, :, C:].reshape(-1, C), B, H)


def fwd_cross_attn(m, ins, cx, saved=None):
    B, q, k, v = _cross_qkv(m, ins[0], cx)
    want = m["side"]["maps"] is not None
    row = _attn_row("map" if want else "self", m, B, probs=want)
    names = ("o", "bound_o") + (("p", "bound_p") if want else ())
    r = _per_image(lambda b: attn.fwd_reference(q[b], k[b], v[b], m["scale"], DP=row.DP, ones=row.ones, want_probs=want), B, names)
    out = dict(out=(_rows(r["o"]), _rows(r["bound_o"])))
    if want:
        out["maps"] = (r["p"], r["bound_p"])
    return out


def vjp_cross_attn(m, ins, saved, gy, cx, bases, gp=None):
    assert bases[0] is None
    B, q, k, v = _cross_qkv(m, ins[0], cx)
    row = _attn_row("xbwd", m, B)
    go = None if m["last"] else _heads(gy, B, m["heads"])
    r = _per_image(lambda b: attn.xbwd_reference(q[b], k[b], v[b], None if go is None else go[b], None if gp is None else gp[b],
                                                 m["scale"], DP=row.DP, ds16=row.ds16), B, ("gq", "bound_gq"))
    return [(_rows(r["gq"]), _rows(r["bound_gq"]))], {}


# ---- the small kernels ---------------------------------------------------------------------------------
def _geglu_parts(pre):
    n = pre.shape[1] // 2
    pv, pg = sk.geglu_positions(n)
    return n, pre[:, pv.to(pre.device)], pre[:, pg.to(pre.device)]


def fwd_geglu(m, ins, cx, saved=None):
    n, v, g = _geglu_parts(ins[0])
    return dict(out=sk.Geglu(False).reference(_ns(n=n), {"v": v, "g": g})["y"])


def vjp_geglu(m, ins, saved, gy, cx, bases):
    assert bases[0] is None
    n, v, g = _geglu_parts(ins[0])
    ref, bnd = sk.Geglu(True).reference(_ns(n=n), {"v": v.cpu(), "g": g.cpu(), "gy": gy.cpu(), "h": ins[0].cpu()})["gh"]
    return [(ref.to(gy.device), bnd.to(gy.device))], {}


def fwd_conv_in(m, ins, cx, saved=None):
    lat = ins[0]                                           # [B][C][L][L]: fp32 values (fp64 in the pure chain)
    B, Cl, Ls, _ = lat.shape
    wi = cx.mat(m["params"]["weight"])
    if saved is None:                                      # the chain: the plain convolution of the latents
        A = _gather(lat.permute(0, 2, 3, 1).reshape(B * Ls * Ls, Cl).to(F64), B, Ls, Ls, Ls, Ls, 1, 0)
        return dict(out=gemm_stmt(A, pack_fwd(wi), cx.vec(m["params"]["bias"])))
    # as launched: [fp16(x) | fp16(x - fp16(x)) | 0] in 8 channels, the filter over [W | W | 0]
    lat8 = sk.Nhwc8().reference(None, {"x": lat.to(F32).reshape(B, Cl, Ls * Ls)})["y"]
    w8 = pack_fwd(torch.cat([wi, wi, wi.new_zeros(wi.shape[0], 8 - 2 * Cl, 3, 3)], 1))
    A = _gather(saved["lat8"], B, Ls, Ls, Ls, Ls, 1, 0)
    return dict(out=gemm_stmt(A, w8, cx.vec(m["params"]["bias"])), lat8=lat8)


def vjp_conv_in(m, gx0, cx, grad_scale):
    """the latent gradient [B][C][L][L] (fp32 on the device) from the gradient of conv_in's output"""
    wi = cx.mat(m["params"]["weight"])
    c0, Cl = wi.shape[0], wi.shape[1]
    Ls = m["H"]
    B = gx0.shape[0] // (Ls * Ls)
    row = _ns(B=B, L=Ls, Cin=c0, Cout=Cl, dgrad=True, out_scale=1.0 / grad_scale, bias=False)
    d = {"x": gx0.reshape(B, Ls * Ls, c0), "w": pack_dgrad(wi), "w_in": wi, "bias": None}
    return sk.ConvOut().reference(row, d)["y"]


FWD = dict(linear=fwd_linear, conv=fwd_conv, shortcut=fwd_shortcut, groupnorm=fwd_groupnorm, layernorm=fwd_layernorm,
           self_attn=fwd_self_attn, cross_attn=fwd_cross_attn, geglu=fwd_geglu, conv_in=fwd_conv_in)
VJP = dict(linear=vjp_linear, conv=vjp_conv, shortcut=vjp_shortcut, groupnorm=vjp_groupnorm, layernorm=vjp_layernorm,
           self_attn=vjp_self_attn, cross_attn=vjp_cross_attn, geglu=vjp_geglu)
SIDES = ("stats", "lse", "maps")


# =================================================================================================
# the chain: the statements composed over the graph in fp64
# =================================================================================================
class Chain:
    def __init__(self, setup, pure):
        self.s, self.g, self.cx = setup, setup.graph, Ctx(setup, pure)
        self.vals, self.sides = {}, {}

    def forward(self, lat):
        """from the latents on (pure chain)"""
        plan = self.s.plan
        for i, m in enumerate(self.g.metas):
            ins = [lat.to(F64)] if m["kind"] == "conv_in" else [self.vals[id(a)] for a in Graph.inputs(m)]
            r = FWD[m["kind"]](m, ins, self.cx)
            self.vals[id(m["out"])] = r["out"][0]
            self.sides[i] = {n: r[n][0] for n in SIDES if n in r}
        return {m["key"]: self.sides[i]["maps"] for i, m in enumerate(self.g.metas) if m["kind"] == "cross_attn" and m["key"] in plan.save_keys}

    def adopt(self, plan):
        """the forward activations and saved statistics of a plan that ran, as given"""
        for i, m in enumerate(self.g.metas):
            for a in Graph.inputs(m) + [m["out"]]:
                self.vals[id(a)] = a.t.to(F64)
            self.sides[i] = {n: t.to(F64) for n, t in m.get("side", {}).items() if t is not None and n in SIDES}

    def backward(self, cot, grad_scale=1.0, round_store=False, drop=()):
        """the VJP chain.  round_store: every gradient rounded to fp16 where the plan stores it (each write of an Act.g,
        the upsample's tmp).  drop: (op index, position in its gouts) pairs whose gradient is not delivered (a wrong plan).
        Returns (g_latents, {id(Act): gradient})."""
        plan, grads = self.s.plan, {}
        r16 = (lambda t: t.to(H16).to(F64)) if round_store else (lambda t: t)
        for i in reversed(range(len(self.g.metas))):
            m, op = self.g.metas[i], plan.ops[i]
            if op.bwd is None:
                continue
            gy = grads.get(id(m["out"]))
            if gy is None:
                assert m["kind"] == "cross_attn" and m["last"], self.g.label(i)
            ins = [self.vals[id(a)] for a in Graph.inputs(m)]
            saved = dict(self.sides[i], out=self.vals[id(m["out"])])
            bases = [grads.get(id(a)) for a in op.gouts]
            kw = {}
            if m["kind"] == "cross_attn":
                kw["gp"] = cot[m["key"]].to(F64).to(gy.device if gy is not None else ins[0].device) if m["key"] in cot else None
            if round_store and m["kind"] == "conv" and m["ups"]:
                _, extra = VJP["conv"](m, ins, saved, gy, self.cx, bases)
                saved["tmp"] = r16(extra["tmp"][0])
            outs, _ = VJP[m["kind"]](m, ins, saved, gy, self.cx, bases, **kw)
            for j, (a, (v, _b)) in enumerate(zip(op.gouts, outs)):
                if (i, j) not in drop:
                    grads[id(a)] = r16(v)
                elif id(a) not in grads:
                    grads[id(a)] = torch.zeros_like(v)
        gl = vjp_conv_in(plan.bwd_tail_meta, grads[id(plan._x0)], self.cx, grad_scale)[0]
        return gl, grads


# =================================================================================================
# the restatement and autograd (the independent oracle of the graph and of the VJPs)
# =================================================================================================
def restate_run(setup, cot=None):
    """fp64: (maps, taps, latent gradient, {tap name: gradient}) of oracle/restate.unet_forward on the case's inputs"""
    s = setup
    lat = s.lat.to(F64).requires_grad_(True)
    saved, taps = {}, {}
    gl = None
    if s.gligen is not None:
        gl = {k: v.to(F64)[s.obj_off:s.obj_off + s.B] for k, v in s.gligen.items()}
    R.unet_forward(s.sd64, s.restate_cfg(), lat, T0, s.ehs.to(F64)[s.text_off:s.text_off + s.B], saved=saved, save_keys=s.keys,
                   gligen=gl, fuser_enabled=s.fuser, stop_after=s.stop, taps=taps, taps_live=True)
    if cot is None:
        return saved, taps, None, {}
    loss = sum((saved[k] * cot[k].to(F64)).sum() for k in s.keys)
    loss.backward()
    return saved, taps, lat.grad, {n: t.grad for n, t in taps.items() if t.grad is not None}


def tap_to_rows(t):
    """a tap of the restatement, [B][C][H][W] or [B][S][C], as the plan's [B * HW][C]"""
    if t.dim() == 4:
        return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])
    return t.reshape(-1, t.shape[-1])


# =================================================================================================
# (d) the emulator: every op in fp32 with fp16 storage, on the plan's own buffers, from the PACKED weights
# =================================================================================================
def _f(t):
    return t.to(F32)


class Emulator:
    """mutant: dict(kind=.., op=index[, pos=..]) — one wrong plan (MUTANTS)."""

    def __init__(self, setup, mutant=None):
        self.s, self.plan, self.w = setup, setup.plan, setup.eng.w
        self.metas = setup.graph.metas
        self.mut = mutant or {}

    def _is(self, kind, i):
        return self.mut.get("kind") == kind and self.mut.get("op") == i

    def _acc(self, i):
        acc = list(self.plan.ops[i].acc)
        if self._is("acc_inverted", i):
            acc[self.mut["pos"]] = not acc[self.mut["pos"]]
        return acc

    @staticmethod
    def _gather(t, *geom):
        return _gather3x3(_f(t), *geom)

    def _residual(self, m, racc):
        res, y = m["res"], m["out"]
        if racc:
            res.g.copy_((_f(res.g) + _f(y.g)).to(H16))
        elif res.g.data_ptr() != y.g.data_ptr():
            res.g.copy_(y.g)

    # ---- forward ---------------------------------------------------------------------------------
    def fwd(self, i):
        m = self.metas[i]
        getattr(self, "f_" + m["kind"])(i, m)

    def f_conv_in(self, i, m):
        lat = m["ins"][0]
        B, Cl, Ls, _ = lat.shape
        lat8 = m["scratch"][0]
        lat8.copy_(sk.Nhwc8().reference(None, {"x": lat.reshape(B, Cl, Ls * Ls)})["y"][0].to(H16))
        A = self._gather(lat8, B, Ls, Ls, Ls, Ls, 1, 0)
        m["out"].t.copy_((A @ _f(self.w.h["conv_in.w8"]).t() + self.w.f["conv_in.b"]).to(H16))

    def f_linear(self, i, m):
        M, n = m["rows"], m["name"]
        y = _f(m["ins"][0].t[:M]) @ _f(self.w.h[f"{n}.w"]).t()
        if m["params"]["bias"]:
            y = y + self.w.f[f"{n}.b"]
        y = y * torch.tensor(m["alpha"], dtype=F32)
        if m["res"] is not None:
            y = y + _f(m["res"].t[:M])
        m["out"].t[:M] = y.to(H16)

    def f_shortcut(self, i, m):
        n = m["name"]
        A = torch.cat([_f(a.t) for a in m["ins"]], 1)
        m["out"].t.copy_((A @ _f(self.w.h[f"{n}.w"]).t() + self.w.f[f"{n}.b"]).to(H16))

    def f_conv(self, i, m):
        n, B = m["name"], self.s.B
        H, Hl, Ho, stride = _conv_geom(m, B)
        A = torch.cat([self._gather(a.t, B, H, H, Ho, Ho, stride, 1 if m["ups"] else 0).reshape(B * Ho * Ho, 9, -1) for a in m["ins"]], 2)
        y = A.reshape(B * Ho * Ho, -1) @ _f(self.w.h[f"{n}.w"]).t() + self.w.f[f"{n}.b"]
        if m["temb_off"] is not None:
            y = y + self.s.eng.temb_cur[0, m["temb_off"]:m["temb_off"] + y.shape[1]]
        if m["res"] is not None:
            y = y + _f(m["res"].t)
        m["out"].t.copy_(y.to(H16))

    def f_groupnorm(self, i, m):
        n, B, HW, G = m["name"], self.s.B, m["HW"], m["G"]
        x = torch.cat([_f(a.t) for a in m["ins"]], 1).reshape(B, HW, G, -1)
        mean = x.mean((1, 3), keepdim=True)
        rstd = torch.rsqrt(((x - mean) ** 2).mean((1, 3), keepdim=True) + torch.tensor(m["eps"], dtype=F32))
        cpg = x.shape[-1]
        z = (x - mean) * rstd * self.w.f[f"{n}.g"].view(G, cpg) + self.w.f[f"{n}.b"].view(G, cpg)
        if m["silu"]:
            z = z / (1.0 + torch.exp(-z))
        m["out"].t.copy_(z.reshape(B * HW, -1).to(H16))
        m["side"]["stats"].copy_(torch.stack([mean.reshape(B, G), rstd.reshape(B, G)], -1))

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
        m["side"]["stats"].copy_(torch.cat([mean, rstd], 1))

    def f_self_attn(self, i, m):
        B, C, q, k, v = _self_qkv(m, _f(m["ins"][0].t))
        row = _attn_row("self", m, B)
        for b in range(B):
            r = attn.fwd_emulation(q[b], k[b], v[b], m["scale"], ones=row.ones)
            m["out"].t.view(B, m["S"], C)[b] = r["o"].permute(1, 0, 2).reshape(m["S"], C).to(H16)
            m["side"]["lse"][b] = r["lse"]

    def _cross(self, m):
        H, B = m["heads"], self.s.B
        qx = _f(m["ins"][0].t)
        C = qx.shape[1]
        kv = _f(m["kv"][:B])
        return B, C, _heads(qx, B, H), _heads(kv[:, :, :C].reshape(-1, C), B, H), _heads(kv[:, :, C:].reshape(-1, C), B, H)

    def f_cross_attn(self, i, m):
        B, C, q, k, v = self._cross(m)
        want = m["side"]["maps"] is not None
        row = _attn_row("map" if want else "self", m, B, probs=want)
        for b in range(B):
            r = attn.fwd_emulation(q[b], k[b], v[b], m["scale"], ones=row.ones)
            m["out"].t.view(B, m["S"], C)[b] = r["o"].permute(1, 0, 2).reshape(m["S"], C).to(H16)
            if want:
                m["side"]["maps"][b] = r["p"]

    def f_geglu(self, i, m):
        n, v, g = _geglu_parts(_f(m["ins"][0].t))
        m["out"].t.copy_((v * sk._gelu32(g)).to(H16))

    # ---- backward -----------------------------------------------------------------------------------
    def bwd(self, i):
        m = self.metas[i]
        getattr(self, "b_" + m["kind"])(i, m, self._acc(i))
        if self._is("clobber", i):                         # a gradient buffer this op does not own is overwritten
            self.mut["victim"].g.zero_()

    def b_linear(self, i, m, acc):
        M, n = m["rows"], m["name"]
        x, y = m["ins"][0], m["out"]
        alpha = 1.0 if self._is("alpha_dropped", i) else m["alpha"]
        gx = (_f(y.g[:M]) @ _f(self.w.h[f"{n}.wt"]).t()) * torch.tensor(alpha, dtype=F32)
        if acc[0]:
            gx = gx + _f(x.g[:M])
        x.g[:M] = gx.to(H16)
        if m["res"] is not None:
            self._residual(m, acc[1])

    def b_shortcut(self, i, m, acc):
        Wt = _f(self.w.h[f"{m['name']}.wt"])
        gy = _f(m["out"].g)
        los = [0, m["ins"][0].C]
        if self._is("wd_slices_swapped", i):
            los = [Wt.shape[0] - m["ins"][0].C, 0]
        for j, a in enumerate(m["ins"]):
            g = gy @ Wt[los[j]:los[j] + a.C].t()
            a.g.copy_((g + _f(a.g) if acc[j] else g).to(H16))

    def b_conv(self, i, m, acc):
        n, B = m["name"], self.s.B
        H, Hl, Ho, stride = _conv_geom(m, B)
        Wd = _f(self.w.h[f"{n}.wd"])
        y, srcs = m["out"], m["ins"]
        if self._is("wd_not_flipped", i):                  # the taps in the forward's order
            Cout = y.C
            Wd = _f(self.w.h[f"{n}.w"]).view(Cout, 3, 3, -1).permute(3, 1, 2, 0).reshape(-1, 9 * Cout)
        if stride == 1 and not m["ups"]:
            A = self._gather(y.g, B, H, H, H, H, 1, 0)
            los = [0, srcs[0].C]
            if self._is("wd_slices_swapped", i):
                los = [Wd.shape[0] - srcs[0].C, 0]
            for j, a in enumerate(srcs):
                g = A @ Wd[los[j]:los[j] + a.C].t()
                a.g.copy_((g + _f(a.g) if acc[j] else g).to(H16))
        elif stride == 2:
            a = srcs[0]
            g = self._gather(y.g, B, Ho, Ho, H, H, 1, 2) @ Wd.t()
            a.g.copy_((g + _f(a.g) if acc[0] else g).to(H16))
        else:
            tmp, a = m["scratch"][0], srcs[0]
            tmp.copy_((self._gather(y.g, B, Hl, Hl, Hl, Hl, 1, 0) @ Wd.t()).to(H16))
            c = [_f(t) for t in sk.Upsample().children(_ns(B=B, H=H, W=H, C=a.C), {"gy": tmp.view(B, Hl * Hl, a.C)})]
            a.g.copy_((((c[0] + c[1]) + c[2]) + c[3]).reshape(-1, a.C).to(H16))
        if m["res"] is not None:
            self._residual(m, acc[-1])

    def b_groupnorm(self, i, m, acc):
        n, B, HW, G = m["name"], self.s.B, m["HW"], m["G"]
        x = torch.cat([_f(a.t) for a in m["ins"]], 1).reshape(B, HW, G, -1)
        cpg = x.shape[-1]
        gy = _f(m["out"].g).reshape(B, HW, G, cpg)
        st = m["side"]["stats"]
        mean, rstd = st[..., 0].view(B, 1, G, 1), st[..., 1].view(B, 1, G, 1)
        gm, bt = self.w.f[f"{n}.g"].view(G, cpg), self.w.f[f"{n}.b"].view(G, cpg)
        xh = (x - mean) * rstd
        dz = gy
        if m["silu"]:
            z = gm * xh + bt
            sg = 1.0 / (1.0 + torch.exp(-z))
            dz = gy * (sg * (1.0 + z * (1.0 - sg)))
        d = dz * gm
        dx = rstd * (d - d.mean((1, 3), keepdim=True) - xh * (d * xh).mean((1, 3), keepdim=True))
        dx = dx.reshape(B * HW, -1)
        lo = 0
        for j, a in enumerate(m["ins"]):
            g = dx[:, lo:lo + a.C]
            a.g.copy_((g + _f(a.g) if acc[j] else g).to(H16))
            lo += a.C

    def b_layernorm(self, i, m, acc):
        n, a = m["name"], m["ins"][0]
        x = _f(a.t[:m["rows"]])
        gy = m["out"].g
        if m["S"]:
            gy = gy.view(-1, m["S"] + N_OBJ_TOKENS, x.shape[1])[:, :m["S"]].reshape(-1, x.shape[1])
        st = m["side"]["stats"]
        d = _f(gy) * self.w.f[f"{n}.g"]
        xh = (x - st[:, 0:1]) * st[:, 1:2]
        g = st[:, 1:2] * (d - d.mean(-1, keepdim=True) - xh * (d * xh).mean(-1, keepdim=True))
        a.g.copy_((g + _f(a.g) if acc[0] else g).to(H16))

    def b_self_attn(self, i, m, acc):
        S, Sk = m["S"], m["Sk"]
        qkv = m["ins"][0]
        B, C, q, k, v = _self_qkv(m, _f(qkv.t))
        go, o = _heads(_f(m["out"].g), B, m["heads"]), _heads(_f(m["out"].t), B, m["heads"])
        g = qkv.g.view(B, Sk, 3 * C)
        if Sk > S and not self._is("tail_not_cleared", i):
            g[:, S:] = 0
        for b in range(B):
            r = attn.bwd_emulation(q[b], k[b], v[b], go[b], o[b], m["side"]["lse"][b], m["scale"], sk_grad=S)
            m["scratch"][0][b] = r["delta"]
            for j, nme in enumerate(("gq", "gk", "gv")):
                g[b, :S, j * C:(j + 1) * C] = r[nme].permute(1, 0, 2).reshape(S, C).to(H16)

    def b_cross_attn(self, i, m, acc):
        B, C, q, k, v = self._cross(m)
        row = _attn_row("xbwd", m, B)
        go = None if m["last"] else _heads(_f(m["out"].g), B, m["heads"])
        gp = m["gmap"]
        for b in range(B):
            r = attn.xbwd_emulation(q[b], k[b], v[b], None if go is None else go[b], None if gp is None else gp[b], m["scale"], ds16=row.ds16)
            m["ins"][0].g.view(B, m["S"], C)[b] = r["gq"].permute(1, 0, 2).reshape(m["S"], C).to(H16)

    def b_geglu(self, i, m, acc):
        pre = m["ins"][0]
        n, v, g = _geglu_parts(_f(pre.t))
        gy = _f(m["out"].g)
        pv, pg = sk.geglu_positions(n)
        pre.g[:, pv], pre.g[:, pg] = (gy * sk._gelu32(g)).to(H16), (gy * v * sk._gelu_grad32(g)).to(H16)

    def tail(self, grad_scale):
        plan = self.plan
        B, Ls = self.s.B, plan.L
        g = self._gather(plan._x0.g, B, Ls, Ls, Ls, Ls, 1, 0) @ _f(self.w.h["conv_in.wd"]).t()
        plan.g_latents.copy_((g * torch.tensor(1.0 / grad_scale, dtype=F32)).reshape(B, Ls, Ls, -1).permute(0, 3, 1, 2))
        return plan.g_latents


class Device:
    """the plan's own launch closures, one op at a time with a synchronize behind each"""

    def __init__(self, setup):
        self.plan = setup.plan

    def fwd(self, i):
        self.plan.ops[i].fwd()
        torch.cuda.synchronize()

    def bwd(self, i):
        self.plan.ops[i].bwd()
        torch.cuda.synchronize()

    def tail(self, grad_scale):
        """Plan.backward has the conv_in input gradient inline behind the reverse ops: the whole reverse plan runs again (it
        overwrites what it wrote: the gradient of conv_in's output is bit for bit what the stepped run left)."""
        g = self.plan.backward(grad_scale)
        torch.cuda.synchronize()
        return g


# =================================================================================================
# (c) the walker
# =================================================================================================
def _bits(t):
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


class Walker:
    def __init__(self, setup, executor=None):
        self.s, self.plan, self.g = setup, setup.plan, setup.graph
        self.ex = executor or (Device(setup) if setup.device.type == "cuda" else Emulator(setup))
        self.cx = Ctx(setup, pure=False)
        self.fwd_ratio, self.bwd_ratio = {}, {}              # op index -> (worst ratio, what)
        self.integrity = []                                  # violations
        eng = setup.eng
        assert len(eng._arena) == 1 and self.plan._cursor[0] == 0, "the cases fit one arena segment"
        self.seg = eng._arena[0]
        self.ext = (self.plan._cursor[1] + 7) // 8 * 8
        self.outside = [("temb_cur", eng.temb_cur)] + [(f"text_kv {k}", t) for k, t in eng.text_kv.items()] + \
                       [(f"fuser_cat {k}", t) for k, t in eng._fuser_cat.items()]
        self.owner = {}
        for i, (m, op) in enumerate(zip(self.g.metas, self.plan.ops)):
            lab = self.g.label(i)
            for n, t in [("output", m["out"].t if isinstance(m["out"], Act) else m["out"])] + list(m.get("side", {}).items()):
                if t is not None:
                    self.owner.setdefault(t.data_ptr(), f"{n} of {lab}")
            for t in m.get("scratch", []):
                self.owner.setdefault(t.data_ptr(), f"scratch of {lab}")
            if isinstance(m["out"], Act) and m["out"].g is not None:
                self.owner.setdefault(m["out"].g.data_ptr(), f"gradient of the output of {lab}")
        for k, t in self.plan.gmaps.items():
            self.owner[t.data_ptr()] = f"gmap {k}"

    # ---- integrity ------------------------------------------------------------------------------
    def _snapshot(self):
        self.snap = self.seg[:self.ext].clone()
        self.snap_out = [t.clone() for _, t in self.outside]

    def _range(self, t):
        off = t.data_ptr() - self.seg.data_ptr()
        if off < 0 or off >= self.ext:
            return None
        return off // 8, (off + t.numel() * t.element_size() + 7) // 8

    def _check_integrity(self, label, declared):
        cur, snap = self.seg[:self.ext].view(torch.int64), self.snap.view(torch.int64)
        diff = cur != snap
        ptrs = set()
        for t in declared:
            r = self._range(t)
            ptrs.add(t.data_ptr())
            if r is not None:
                diff[r[0]:r[1]] = False
                snap[r[0]:r[1]] = cur[r[0]:r[1]]
        if bool(diff.any()):
            for b in self.plan._buffers:
                r = self._range(b)
                if r is not None and bool(diff[r[0]:r[1]].any()):
                    self.integrity.append(f"{label} changed {self.owner.get(b.data_ptr(), 'a plan buffer')}")
            snap.copy_(cur)
        for j, (n, t) in enumerate(self.outside):
            if t.data_ptr() in ptrs:
                self.snap_out[j] = t.clone()
            elif not torch.equal(_bits(t), _bits(self.snap_out[j])):
                self.integrity.append(f"{label} changed {n}")
                self.snap_out[j] = t.clone()

    # ---- per-op checks ----------------------------------------------------------------------------
    @staticmethod
    def _ratio(got, ref_bound, fp16=True):
        ref, bound = ref_bound
        return sk.worst_ratio(got.reshape(ref.shape), ref, bound, fp16=fp16)

    def _given(self, m):
        return [(a.t if isinstance(a, Act) else a).to(F64) for a in (m["ins"] if m["kind"] == "conv_in" else Graph.inputs(m))]

    def _check_fwd(self, i, m):
        saved = {"lat8": m["scratch"][0].to(F64)} if m["kind"] == "conv_in" else {}
        r = FWD[m["kind"]](m, self._given(m), self.cx, saved=saved)
        what = {"output": self._ratio(m["out"].t, r["out"])}
        for n in SIDES:
            if n in r and m["side"][n] is not None:
                what[n] = self._ratio(m["side"][n], r[n], fp16=False)
        if "lat8" in r:
            what["lat8"] = self._ratio(m["scratch"][0], r["lat8"])
        worst = max(what, key=what.get)
        self.fwd_ratio[i] = (what[worst], worst)

    def run(self, check_fwd=None, check_bwd=None, integrity=True, grad_scale=GRAD_SCALE, until=None):
        """check_fwd / check_bwd: the op indices whose outputs are compared with their statements (None: all).
        until: the reverse walk ends behind this op (wrong plans that are caught there)."""
        s, plan, eng, metas = self.s, self.plan, self.s.eng, self.g.metas
        dev = s.device
        eng.poison_arena()
        plan.latents_in.copy_(s.lat)
        if integrity:
            self._snapshot()
        for i, m in enumerate(metas):
            self.ex.fwd(i)
            if integrity:
                decl = [m["out"].t] + [t for t in m.get("side", {}).values() if t is not None]
                decl += [t for t in m.get("scratch", []) if m["kind"] in ("conv_in", "groupnorm")]
                self._check_integrity(f"forward of {self.g.label(i)}", decl)
            if check_fwd is None or i in check_fwd:
                self._check_fwd(i, m)
        for k, t in plan.gmaps.items():
            t.copy_(s.cot[k])
        seen_g = set()
        for m in metas:
            for a in Graph.inputs(m) + [m["out"]]:
                if a.g is not None and a.g.data_ptr() not in seen_g:
                    seen_g.add(a.g.data_ptr())
                    a.g.fill_(float("nan"))
        if integrity:
            self._snapshot()
        written = set()
        for i in reversed(range(len(metas))):
            m, op = metas[i], plan.ops[i]
            if op.bwd is None:
                continue
            assert len({id(a) for a in op.gouts}) == len(op.gouts)
            check = check_bwd is None or i in check_bwd
            if check:
                gy = None if (m["kind"] == "cross_attn" and m["last"]) else m["out"].g.to(F64)
                bases = [a.g.to(F64) if id(a) in written else None for a in op.gouts]
            self.ex.bwd(i)
            if integrity:
                self._check_integrity(f"backward of {self.g.label(i)}", [a.g for a in op.gouts] + list(m.get("scratch", [])))
            if check:
                saved = {n: t.to(F64) for n, t in m.get("side", {}).items() if t is not None and n in SIDES}
                saved["out"] = m["out"].t.to(F64)
                if m["kind"] == "conv" and m["ups"]:
                    saved["tmp"] = m["scratch"][0].to(F64)
                kw = {}
                if m["kind"] == "cross_attn":
                    kw["gp"] = m["gmap"].to(F64) if m["gmap"] is not None else None
                outs, extra = VJP[m["kind"]](m, self._given(m)[:len(Graph.inputs(m))], saved, gy, self.cx, bases, **kw)
                what = {f"gradient {j}": self._ratio(a.g, ob) for j, (a, ob) in enumerate(zip(op.gouts, outs))}
                if "tmp" in extra:
                    what["tmp"] = self._ratio(m["scratch"][0], extra["tmp"])
                if "delta" in extra:
                    what["delta"] = self._ratio(m["scratch"][0], extra["delta"], fp16=False)
                worst = max(what, key=what.get)
                self.bwd_ratio[i] = (what[worst], worst)
            written.update(id(a) for a in op.gouts)
            if i == until:
                return None
        gx0 = plan._x0.g.clone()
        gl = self.ex.tail(grad_scale)
        if integrity and isinstance(self.ex, Emulator):
            self._check_integrity("the conv_in input gradient", [plan.g_latents])
        self.x0_grad_stable = torch.equal(_bits(gx0), _bits(plan._x0.g))
        ref = vjp_conv_in(plan.bwd_tail_meta, plan._x0.g.to(F64), self.cx, grad_scale)
        self.bwd_ratio[-1] = (self._ratio(gl, ref, fp16=False), "g_latents")
        return gl

    def worst(self, which):
        d = self.fwd_ratio if which == "fwd" else self.bwd_ratio
        i = max(d, key=lambda j: d[j][0])
        return d[i][0], (self.g.label(i) if i >= 0 else "the conv_in input gradient") + f": {d[i][1]}"


# =================================================================================================
# wrong plans, and where each has to be caught (tests/test_unet_plan_cpu.py)
# =================================================================================================
def find_op(setup, pred):
    return next(i for i, m in enumerate(setup.graph.metas) if pred(m, setup.plan.ops[i]))

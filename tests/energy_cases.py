"""The launch contracts of the two guidance-energy kernels, lgd_ca_energy_f32 (csrc/energy.hip) and lgd_boxdiff_energy_f32
(csrc/boxdiff.hip), as test data — the layout of tests/small_kernel_cases.py, whose V, Carved, GUARD, sentinels and
worst_ratio are reused.

A ROW is (entry point, label, parameters).  `row.data()` builds the RAW tables of one launch on the host (items, groups, coefs,
masks, refs, dyn, the maps) without EnergyTables / BoxDiffTables, so forms those classes never produce are reachable.
`reference(row, d)` is the fp64 result computed from the fp32 inputs: index arithmetic on the logical operands after the
statements of include/lgd_hip.h and the formulas of utils/guidance.py / utils/boxdiff.py as the header cites them.  It returns
name -> (value, bound) for "loss", "partial" (ca_energy) and one "gmap<k>" per map: the WHOLE gradient buffer, in which every
element the header does not name holds the sentinel with bound 0, so that "only the documented elements are stored" is part
of the same comparison.  `emulate(row, d)` is an fp32 rendering of the kernel's arithmetic in its own order (CPU suite: the
bound is not too tight), MUTATIONS wrong answers of the reference that have to fall outside.  REFUSALS / UNSUPPORTED are one
changed argument per row of a call the library serves (BASE).

The bounds.  w = 2^-24.  V (small_kernel_cases) carries a value and the error bound of its fp32 rendering, one rounding per
operation (a contracted fma rounds once: the bound holds).  On top of V:
    vsum(x, D)   a sum in which every term passes through at most D additions: e = (1 + g) sum e_i + g sum |x_i|,
                 g = D w / (1 - D w).
    block sum    block_sum_256 of per-thread strided sums: a thread adds ceil(HW / 256) terms, the first of them to 0 (exact),
                 the wave butterfly has six levels, three adds join the four waves: D = ceil(HW / 256) - 1 + 9.
    constants    REF_EPS and 1 / (n_maps H) are carried as V(real value, |fp32 value - real value|).
ca_energy, per (column, head), A the map column, M the mask row, both fp32; every row's masks are in {0, 0.5, 1} (asserted), so
A M, R M and A (1 - M) are EXACT in fp32:
    kind 0  v = A M and w = A (1 - M) are exact, so the fp64 ranking is the fp32 ranking and
            the selection is the same set bit for bit; fg = block sum of the selected v, term = c_fg (1 - fg / k_fg) +
            c_bg (bg / k_bg) through V; gradient ((0 - (c_fg / k_fg) M) + (c_bg / k_bg)(1 - M)) grad_scale through V.
    kind 2  sa = block sum A, sm = block sum A M, r = sm / sa, term c (1 - r)^2, gradient
            (((-2 c)(1 - r)) / (sa sa) grad_scale)(M sa - sm), all through V.
    kind 1  am = A M, rm = R M, sa, sr block sums, ia = 1 / (sa + eps), ir likewise (correctly rounded divisions),
            df = am ia - rm ir, term c block sum |df|, dot = block sum sign(df) am, gradient
            ((grad_scale c) M)(sign(df) ia - (dot ia) ia) through V.  The sign is a bit condition: |df| exceeds its bound
            or df is zero by construction (M = 0, or R = A on the column: both products are then the same fp32 number).
    the column's gradient is the sum of its items in table order through V; loss[b] = block sum over n_items H partials.
BoxDiff, per image:
    x = ((sequential sum over n_maps H maps) inv_n) 100: vsum with D = n_maps H, two products; t = x - max (the maximum
    shifts numerator and denominator alike), e = __expf(t) at 2^-22 behind the rounded product (V.expf), z = vsum(e, 7) (one
    add of the lane's two tokens and six butterfly levels), p = e / z for the item tokens; the smoothed image is nine
    products and adds in tap order through V; v M and v (1 - M), the top-k block sums, 1 - fg / k, bg / k through V; the
    corner terms |max - gt| cmask / side through V, summed with D = 9 (one term per thread); the smoothing backward is the
    transpose of the forward operator: element i gathers n_i products, e = (1 + g) |K|^T e + g |K|^T |g_sm|, g from
    D = n_i; c = sequential sum of g_img p over the items; gs = ((100 loss_scale) grad_scale) inv_n; p again as e (1 / z);
    d = (gs p)(g_tok - c), g_tok the sequential sum of the items on that token.
    Ranking smoothed values is a bit condition: the k-th and (k+1)-th reference values differ by more than their two bounds,
    or they are equal by construction — both products exactly 0, or identical input rows with smooth = NULL, which the kernel
    takes through identical operations.  The same holds for the arg-max of every row and column and for the signs of
    1 - mean, mean and max - gt.
Nothing above is fitted to kernel output."""
import functools
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from small_kernel_cases import GUARD, SENT32, Carved, P, V, W, f32, worst_ratio, _butterfly  # noqa: E402,F401

F32, F64, I32 = torch.float32, torch.float64, torch.int32
NAN = float("nan")
SENT = f32(SENT32)                                       # the sentinel as the fp32 buffers hold it
REF_EPS = V(1e-5, abs(f32(1e-5) - 1e-5))                # guidance.py:150
BD_LDS_BYTES = 150 * 1024                                # the header's rule: (7 + 2 max_items) side^2 4 <= 150 KB
LDS_DEFAULT = 64 * 1024                                  # above it the launch raises the kernel's dynamic LDS limit


def bd_lds(side, max_items):
    return (7 + 2 * max_items) * side * side * 4


def bd_max_items(side):
    return (BD_LDS_BYTES // (side * side * 4) - 7) // 2


# ---------------------------------------------------------------------------------------------
# sums
# ---------------------------------------------------------------------------------------------
def vsum(x, dim, depth, keepdim=False):
    g = depth * W / (1.0 - depth * W)
    return V(x.v.sum(dim, keepdim=keepdim), (1.0 + g) * x.e.sum(dim, keepdim=keepdim) + g * x.v.abs().sum(dim, keepdim=keepdim))


def block_depth(n):
    return -(-n // 256) - 1 + 9                          # a thread's first add is to 0 and exact


def block_sum32(x):
    """block_sum_256 over the last dimension in fp32: thread t adds elements t, t + 256, ...; the butterfly; the four waves"""
    n = x.shape[-1]
    pad = (-n) % 256
    if pad:
        x = torch.cat([x, torch.zeros(*x.shape[:-1], pad, dtype=F32)], -1)
    x = x.reshape(*x.shape[:-1], -1, 256)
    acc = torch.zeros(*x.shape[:-2], 256, dtype=F32)
    for k in range(x.shape[-2]):
        acc = acc + x[..., k, :]
    wv = _butterfly(acc.reshape(*acc.shape[:-1], 4, 64))
    return ((wv[..., 0] + wv[..., 1]) + wv[..., 2]) + wv[..., 3]


def topk_lowest(v, k, highest=False):
    """the k largest of v, the lowest index first among equals (include/lgd_hip.h) -> selection mask"""
    n = v.numel()
    if highest:
        order = (n - 1) - torch.sort(v.flip(0), descending=True, stable=True).indices
    else:
        order = torch.sort(v, descending=True, stable=True).indices
    sel = torch.zeros(n, dtype=torch.bool)
    sel[order[:max(k, 0)]] = True
    return sel, order


def _sel(x, mask):
    m = mask.to(F64)
    return V(x.v * m, x.e * m)


def _at(x, idx):
    return V(x.v[idx], x.e[idx])


def _sign(v):
    return torch.sign(v)


# ---------------------------------------------------------------------------------------------
# rows
# ---------------------------------------------------------------------------------------------
class Row:
    def __init__(self, entry, label, **p):
        self.entry, self.label = entry, label
        self.p = dict(DEFAULTS[entry], **p)
        assert set(p) <= set(DEFAULTS[entry]), (label, set(p) - set(DEFAULTS[entry]))
        self.name = f"{entry}:{label}"

    def __getattr__(self, k):
        p = self.__dict__.get("p", {})
        if k in p:
            return p[k]
        raise AttributeError(k)

    def seed(self):
        return 9000 + sum(map(ord, self.name)) % 1000 + self.p["reseed"]

    def data(self):
        return _data(self.name)


@functools.lru_cache(maxsize=4)
def _data(name):
    row = ROWS_BY_NAME[name]
    g = torch.Generator().manual_seed(row.seed())
    return (ca_data if row.entry == "ca_energy" else bd_data)(row, g)


# ca_energy.  cols: the columns in table order, (map, image, token, ((kind, k mode), ...)); k mode of kind 0: "p" a fifth of
# the count, "one", "fgall" (k_fg = the in-mask count), "bgall" (k_bg = the out-of-mask count), "zeros" (k past the count of
# non-zero values of every head: tied zeros are selected).  mask "01" / "half" ({0, 0.5, 1}) / "allhalf" (0.5 everywhere).
# maps "rand" / "tied" (multiples of 2^-10 below 2^-8, half of them zero).  pad = max_hw - max(hw): the padding of the mask and
# reference rows holds NaN.  dyn0 the step, gap the floats between two step slices of refs.  ref_equal: R = A on kind 1.
_CA = dict(hw=(256,), H=1, T=77, S=1, pad=0, cols=((0, 0, 5, ((0, "p"),)),), mask="01", maps="rand", dyn0=0, gap=0, gscale=1.0,
           ref_equal=False, tie=False, reseed=0)
# BoxDiff.  images: per image its objects (tokens, box (x0, y0, x1, y1) in cells, options); options: k_fg / k_bg (else a fifth
# of the count, as utils/boxdiff.py:80,85), corner "zero", half (the box mask is 0.5).  smooth None / "gauss" / "asym".
# dup: 2 x 2 blocks of positions share their input rows.  max_items None = the largest count.
_BD = dict(side=16, T=77, n_maps=1, H=1, images=((((5,), (3, 4, 11, 12), {}),),), smooth="gauss", dup=False, ls=1.0, gs=1.0,
           max_items=None, tie=False, reseed=0)
DEFAULTS = {"ca_energy": _CA, "boxdiff": _BD}


def _ca_mask(kind, hw, g):
    if kind == "allhalf":
        return torch.full((hw,), 0.5)
    m = (torch.rand(hw, generator=g) < 0.4).to(F32)
    if kind == "half":
        m = torch.randint(0, 3, (hw,), generator=g).to(F32) * 0.5
    m[0], m[-1] = 1.0, 0.0
    return m


def ca_data(row, g):
    p = row.p
    H, T, S, hws = p["H"], p["T"], p["S"], p["hw"]
    max_hw = max(hws) + p["pad"]
    maps = []
    for hw in hws:
        if p["maps"] == "tied":
            a = (torch.randint(0, 6, (S, H, hw, T), generator=g).clamp_min(2) - 2).to(F32) / 1024.0
        else:
            a = torch.rand(S, H, hw, T, generator=g) * (2.0 / hw)
        maps.append(a.contiguous())
    items, coefs, masks, groups, ref_cols = [], [], [], [], []
    for mp, img, tok, kinds in p["cols"]:
        hw = hws[mp]
        groups.append([len(items), len(kinds)])
        col = maps[mp][img, :, :, tok]                                  # [H][hw]
        for kind, mode in kinds:
            m = _ca_mask(p["mask"], hw, g)
            row_m = torch.full((max_hw,), NAN)
            row_m[:hw] = m
            mid = len(masks)
            masks.append(row_m)
            k_fg = k_bg = 1
            if kind == 0:
                n_in, n_out = int((m > 0).sum()), int((m < 1).sum())
                k_fg, k_bg = max(1, n_in // 5), max(1, n_out // 5)
                if mode == "one":
                    k_fg = k_bg = 1
                elif mode == "fgall":
                    k_fg = n_in
                elif mode == "bgall":
                    k_bg = n_out
                elif mode == "zeros":
                    k_fg = min(hw, int(((col * m) != 0).sum(-1).max()) + 2)
                    k_bg = min(hw, int(((col * (1 - m)) != 0).sum(-1).max()) + 2)
                elif mode != "p":
                    raise ValueError(f"{row.name}: unknown k mode {mode!r}")
            elif mode not in ("", "p"):                           # kinds 1 and 2 have no k: only the default may be named
                raise ValueError(f"{row.name}: kind {kind} takes no k mode, got {mode!r}")
            c = torch.full((4,), NAN)                                  # the coefficients a kind does not use hold NaN
            if kind == 0:
                c[:2] = 0.5 + torch.rand(2, generator=g)
            else:
                c[2 if kind == 1 else 3] = 0.5 + float(torch.rand(1, generator=g))
            rid = 0
            if kind == 1:
                rid = len(ref_cols)
                ref_cols.append((mp, col.clone() if p["ref_equal"] else None))
            items.append([mp, kind, tok, mid, k_fg, k_bg, rid, img])
            coefs.append(c)
    n_items, n_refs = len(items), len(ref_cols)
    d = dict(maps=maps, map_hw=torch.tensor(list(hws), dtype=I32), n_items=n_items, n_groups=len(groups), max_hw=max_hw,
             items=torch.tensor(items or [[0] * 8], dtype=I32), coefs=torch.stack(coefs) if coefs else torch.full((1, 4), NAN),
             masks=torch.stack(masks) if masks else torch.full((1, max_hw), NAN),
             groups=torch.tensor(groups or [[0, 0]], dtype=I32), refs=None, dyn=None, stride=0)
    if n_refs:
        n_steps = p["dyn0"] + 1
        stride = n_refs * H * max_hw + p["gap"]
        refs = torch.full((n_steps * stride,), NAN)
        for s in range(n_steps):
            for rid, (mp, same) in enumerate(ref_cols):
                hw = hws[mp]
                r = torch.rand(H, hw, generator=g) * (2.0 / hw)
                if same is not None and s == p["dyn0"]:
                    r = same
                for h in range(H):
                    o = s * stride + (rid * H + h) * max_hw
                    refs[o:o + hw] = r[h]
        d.update(refs=refs, stride=stride, dyn=torch.tensor([p["dyn0"], 0, 0, 0], dtype=I32))
    return d


def _bd_object_rows(side, box, opt):
    x0, y0, x1, y1 = box
    m = torch.zeros(side, side)
    m[y0:y1, x0:x1] = 0.5 if opt.get("half") else 1.0
    cx, cy = torch.zeros(side), torch.zeros(side)
    if opt.get("corner") != "zero":                                     # utils/boxdiff.py:64-67 with L = 1
        for lo, line in ((x0, cx), (x1, cx), (y0, cy), (y1, cy)):
            line[max(lo - 1, 0):min(lo + 2, side)] = 1.0
    rows = torch.zeros(3, side * side)
    rows[0] = m.reshape(-1)
    rows[1, :side], rows[1, side:2 * side] = cx, cy
    rows[2, :side], rows[2, side:2 * side] = (m > 0).to(F32).max(0).values, (m > 0).to(F32).max(1).values
    k_fg = opt.get("k_fg", int((m > 0).sum() * 0.2))
    k_bg = opt.get("k_bg", int((m < 1).sum() * 0.2))
    return rows, k_fg, k_bg


SMOOTH_ASYM = [0.02, 0.11, 0.05, 0.17, 0.31, 0.07, 0.03, 0.13, 0.11]   # nine distinct weights, sum 1


def bd_data(row, g):
    from lgd_amd.energy import gaussian_kernel
    p = row.p
    side, T, n_maps, H, S = p["side"], p["T"], p["n_maps"], p["H"], len(p["images"])
    HW = side * side
    maps = []
    for _ in range(n_maps):
        if p["dup"]:
            base = torch.softmax(0.7 * torch.randn(S, H, side // 2, side // 2, T, generator=g), -1)
            a = base.repeat_interleave(2, 2).repeat_interleave(2, 3).reshape(S, H, HW, T)
        else:
            a = torch.softmax(0.7 * torch.randn(S, H, HW, T, generator=g), -1)
        maps.append(a.contiguous())
    items, masks, groups = [], [], []
    for objs in p["images"]:
        first = len(items)
        for toks, box, opt in objs:
            rows, k_fg, k_bg = _bd_object_rows(side, box, opt)
            mid = len(masks)
            masks.append(rows)
            for t in toks:
                items.append([t, mid, k_fg, k_bg, 0, 0, 0, 0])
        groups.append([first, len(items) - first])
    smooth = {None: None, "gauss": gaussian_kernel(3, 0.5).reshape(-1).to(F32), "asym": torch.tensor(SMOOTH_ASYM, dtype=F32)}[p["smooth"]]
    count = max(c for _, c in groups)
    max_items = count if p["max_items"] is None else p["max_items"]
    assert max_items >= count
    return dict(maps=maps, items=torch.tensor(items or [[0] * 8], dtype=I32), n_items=len(items),
                masks=torch.stack(masks) if masks else torch.zeros(1, 3, HW), groups=torch.tensor(groups, dtype=I32),
                smooth=smooth, max_items=max_items, S=S)


# ---------------------------------------------------------------------------------------------
# ca_energy: reference and emulation
# ---------------------------------------------------------------------------------------------
class Conditions:
    """the bit conditions of one reference run: (label, holds); `ties` the places where an exact tie decided"""

    def __init__(self):
        self.failed, self.ties, self.checked = [], set(), 0

    def need(self, ok, label):
        self.checked += 1
        if not bool(ok):
            self.failed.append(label)


def _ca_item_ref(kind, A, M, R, c, k_fg, k_bg, gs, cond, wrong, label):
    HW = A.numel()
    D = block_depth(HW)
    cond.need(bool(((M == 0) | (M == 0.5) | (M == 1)).all()), f"{label}: a mask outside 0, 0.5, 1")
    if kind == 0:
        v, w = A * M, A * ((M if wrong.get("bg_uses_m") else 1.0 - M))
        cond.need(bool((v.to(F32).to(F64) == v).all() and (w.to(F32).to(F64) == w).all()), f"{label}: A M is not exact in fp32")
        extra = 1 if wrong.get("k_plus_1") else 0
        sf, of = topk_lowest(v, k_fg + extra, wrong.get("tie_high"))
        sb, ob = topk_lowest(w, k_bg + extra, wrong.get("tie_high"))
        for o, k, x in ((of, k_fg, v), (ob, k_bg, w)):
            if k < HW and float(x[o[k - 1]]) == float(x[o[k]]):
                cond.ties.add("k")
        fg, bg = vsum(_sel(V(v), sf), -1, D), vsum(_sel(V(w), sb), -1, D)
        cf, cb = float(c[0]), float(c[1])
        term = cf * (1.0 - fg / float(k_fg)) + cb * (bg / float(k_bg))
        mf = V(torch.ones_like(M)) if wrong.get("no_m") else V(M)
        g = _sel(-((V(cf) / float(k_fg)) * mf), sf) + _sel((V(cb) / float(k_bg)) * V(1.0 - M), sb)
        return term, g * gs
    if kind == 2:
        cr = float(c[3])
        sa, sm = vsum(V(A), -1, D), vsum(V(A).times_exact(V(M)), -1, D)
        r = sm / sa
        gk = (V(-2.0 * cr) * (1.0 - r)) / (sa * sa) * gs
        inner = V(M) * sa if wrong.get("ratio_no_sm") else V(M) * sa - sm
        return V(cr) * (1.0 - r) * (1.0 - r), gk * inner
    cr = float(c[2])
    am, rm = V(A).times_exact(V(M)), V(R).times_exact(V(M))
    sa, sr = vsum(am, -1, D), vsum(rm, -1, D)
    eps = V(0.0) if wrong.get("no_eps") else REF_EPS
    ia, ir = V(1.0) / (sa + eps), V(1.0) / (sr + eps)
    df = am * ia - rm * ir
    by_construction = M == 0                            # both products are exactly 0
    if bool((A == R).all()):                            # R = A on the whole column: the two block sums are the same number too
        by_construction = torch.ones_like(M, dtype=torch.bool)
        cond.ties.add("df")
    cond.need(bool((by_construction | (df.v.abs() > df.e)).all()), f"{label}: the sign of a df is inside its bound")
    df = V(torch.where(by_construction, 0.0, df.v), torch.where(by_construction, 0.0, df.e))
    sg = _sign(df.v)
    l1 = vsum(df.abs(), -1, D)
    dot = vsum(V(sg * am.v, am.e), -1, D)
    g = ((V(gs) * cr) * V(M)) * (V(sg) * ia - (dot * ia) * ia)
    return V(cr) * l1, g


def _ca_operands(row, d, item, h, wrong):
    """the logical column, mask row and reference row of (item, head) in fp64"""
    p = row.p
    mp, kind, tok, mid, k_fg, k_bg, rid, img = [int(x) for x in d["items"][item]]
    hw, max_hw, H = p["hw"][mp], d["max_hw"], p["H"]
    A = d["maps"][mp][img, h, :, tok].to(F64)
    mstride = hw if wrong.get("mask_stride_hw") else max_hw
    M = d["masks"].reshape(-1)[mid * mstride:mid * mstride + hw].to(F64)
    R = None
    if kind == 1:
        step = 0 if wrong.get("step0") else int(d["dyn"][0])
        hstride = hw if wrong.get("ref_head_stride") else max_hw
        o = step * d["stride"] + (rid * H + h) * hstride
        R = d["refs"][o:o + hw].to(F64)
    return (mp, kind, tok, k_fg, k_bg, img), A, M, R


def ca_reference(row, d, **wrong):
    p = row.p
    H, T, S, gs = p["H"], p["T"], p["S"], f32(p["gscale"])
    cond = Conditions()
    gv = [torch.full((S, H, hw, T), SENT, dtype=F64) for hw in p["hw"]]
    ge = [torch.zeros(S, H, hw, T, dtype=F64) for hw in p["hw"]]
    n_items = d["n_items"]
    pv, pe = torch.zeros(max(n_items * H, 1), dtype=F64), torch.zeros(max(n_items * H, 1), dtype=F64)
    for first, count in d["groups"].tolist()[:d["n_groups"]]:
        for h in range(H):
            acc = None
            for item in range(first, first + count):
                (mp, kind, tok, k_fg, k_bg, img), A, M, R = _ca_operands(row, d, item, h, wrong)
                term, g = _ca_item_ref(kind, A, M, R, d["coefs"][item].to(F64), k_fg, k_bg, gs, cond, wrong,
                                       f"{row.name} item {item} head {h}")
                if wrong.get("gscale_on_loss"):
                    term = term * gs
                pv[item * H + h], pe[item * H + h] = term.v, term.e
                acc = (V(torch.zeros_like(g.v)) + g) if (acc is None or wrong.get("overwrite")) else acc + g
            gv[mp][img, h, :, tok], ge[mp][img, h, :, tok] = acc.v, acc.e
    image = d["items"][:, 7].to(torch.long).repeat_interleave(H)[:n_items * H] if n_items else torch.zeros(0, dtype=torch.long)
    lv, le = torch.zeros(S, dtype=F64), torch.zeros(S, dtype=F64)
    for b in range(S):
        own = torch.ones_like(image, dtype=torch.bool) if wrong.get("cross_image") else image == b
        s = vsum(_sel(V(pv[:n_items * H], pe[:n_items * H]), own), -1, block_depth(max(n_items * H, 1)))
        lv[b], le[b] = s.v, s.e
    out = {"loss": (lv, le), "_cond": cond}
    if n_items:
        out["partial"] = (pv, pe)
    for k in range(len(gv)):
        out[f"gmap{k}"] = (gv[k], ge[k])
    return out


def _sign32(x):
    return torch.sign(x)


def ca_emulate(row, d):
    p = row.p
    H, T, S = p["H"], p["T"], p["S"]
    gs = torch.tensor(p["gscale"], dtype=F32)
    one = torch.tensor(1.0, dtype=F32)
    eps = torch.tensor(1e-5, dtype=F32)
    gm = [torch.full((S, H, hw, T), SENT32, dtype=F32) for hw in p["hw"]]
    n_items = d["n_items"]
    partial = torch.zeros(max(n_items * H, 1), dtype=F32)
    for first, count in d["groups"].tolist()[:d["n_groups"]]:
        for h in range(H):
            s_g = None
            for item in range(first, first + count):
                (mp, kind, tok, k_fg, k_bg, img), A, M, R = _ca_operands(row, d, item, h, {})
                A, M = A.to(F32), M.to(F32)
                c = d["coefs"][item]
                if s_g is None:
                    s_g = torch.zeros_like(A)
                if kind == 0:
                    v, w = A * M, A * (one - M)
                    sf, _ = topk_lowest(v, k_fg)
                    sb, _ = topk_lowest(w, k_bg)
                    fg, bg = block_sum32(v * sf), block_sum32(w * sb)
                    kf, kb = torch.tensor(float(k_fg), dtype=F32), torch.tensor(float(k_bg), dtype=F32)
                    g = torch.zeros_like(A) - (c[0] / kf * M) * sf + (c[1] / kb * (one - M)) * sb
                    s_g = s_g + g * gs
                    partial[item * H + h] = c[0] * (one - fg / kf) + c[1] * (bg / kb)
                elif kind == 2:
                    sa, sm = block_sum32(A), block_sum32(A * M)
                    r = sm / sa
                    gk = -2.0 * c[3] * (one - r) / (sa * sa) * gs
                    s_g = s_g + gk * (M * sa - sm)
                    partial[item * H + h] = c[3] * (one - r) * (one - r)
                else:
                    R = R.to(F32)
                    am, rm = A * M, R * M
                    sa, sr = block_sum32(am), block_sum32(rm)
                    ia, ir = one / (sa + eps), one / (sr + eps)
                    df = am * ia - rm * ir
                    sg = _sign32(df)
                    l1, dot = block_sum32(df.abs()), block_sum32(sg * am)
                    s_g = s_g + torch.where(M != 0, gs * c[2] * M * (sg * ia - dot * ia * ia), torch.zeros_like(A))
                    partial[item * H + h] = c[2] * l1
            gm[mp][img, h, :, tok] = s_g
    loss = torch.zeros(S, dtype=F32)
    image = d["items"][:, 7].to(torch.long).repeat_interleave(H)[:n_items * H]
    for b in range(S):
        loss[b] = block_sum32(partial[:n_items * H] * (image == b)) if n_items else 0.0
    out = {"loss": loss}
    if n_items:
        out["partial"] = partial
    for k in range(len(gm)):
        out[f"gmap{k}"] = gm[k]
    return out


# ---------------------------------------------------------------------------------------------
# BoxDiff: reference and emulation
# ---------------------------------------------------------------------------------------------
def _refl(i, n):
    return torch.where(i < 0, -i, torch.where(i >= n, 2 * n - 2 - i, i))


def _taps(side, zero_pad=False):
    """per tap (dy, dx) in the kernel's order: the source index of every output position, and whether the tap counts"""
    i = torch.arange(side * side)
    y, x = i // side, i % side
    out = []
    for dy in range(3):
        for dx in range(3):
            yy, xx = y + dy - 1, x + dx - 1
            inside = (yy >= 0) & (yy < side) & (xx >= 0) & (xx < side)
            src = _refl(yy, side) * side + _refl(xx, side)
            out.append((src, inside if zero_pad else torch.ones_like(inside)))
    return out


def _first_max(t2, dim):
    """maximum along `dim` of a [side][side] image and the LOWEST index that holds it"""
    mx = t2.max(dim, keepdim=True).values
    ar = torch.arange(t2.shape[dim]).view(-1, 1) if dim == 0 else torch.arange(t2.shape[dim]).view(1, -1)
    return mx.squeeze(dim), torch.where(t2 == mx, ar, t2.shape[dim]).min(dim).values


def _last_max(t2, dim):
    mx = t2.max(dim, keepdim=True).values
    ar = torch.arange(t2.shape[dim]).view(-1, 1) if dim == 0 else torch.arange(t2.shape[dim]).view(1, -1)
    return mx.squeeze(dim), torch.where(t2 == mx, ar, -1).max(dim).values


def _same_rows(stack, i, j):
    return bool((stack[:, i, :] == stack[:, j, :]).all())


def _tie_or_gap(cond, x, i, j, stack, smooth, label):
    """positions i and j of V x are ordered beyond their bounds, or equal by construction: both exactly 0, identical input
    rows with smooth = NULL, or T = 3, where the single soft-max token has probability __expf(0) / 1 = 1 at every position"""
    vi, vj, ei, ej = float(x.v[i]), float(x.v[j]), float(x.e[i]), float(x.e[j])
    if vi == vj:
        ok = (ei == 0.0 and ej == 0.0) or (smooth is None and _same_rows(stack, i, j)) or stack.shape[-1] == 3
        cond.need(ok, f"{label}: equal values that are not equal by construction")
        return True
    cond.need(abs(vi - vj) > ei + ej, f"{label}: a gap {abs(vi - vj):.3e} inside the bounds {ei + ej:.3e}")
    return False


def bd_reference(row, d, **wrong):
    p = row.p
    side, T, n_maps, H, S = p["side"], p["T"], p["n_maps"], p["H"], d["S"]
    HW, n = side * side, n_maps * H
    ls, gsc = f32(p["ls"]), f32(p["gs"])
    cond = Conditions()
    smooth = d["smooth"].to(F64) if d["smooth"] is not None else None
    if smooth is not None and wrong.get("smooth_transposed"):
        smooth = smooth.reshape(3, 3).t().reshape(-1)
    taps = _taps(side)
    btaps = _taps(side, zero_pad=bool(wrong.get("zero_pad_backward")))
    inv_n = V(1.0 / n, abs(f32(1.0 / n) - 1.0 / n))
    lo, hi = (0, T) if wrong.get("softmax_all") else (1, T - 1)
    gv = [torch.full((S, H, HW, T), SENT, dtype=F64) for _ in range(n_maps)]
    ge = [torch.zeros(S, H, HW, T, dtype=F64) for _ in range(n_maps)]
    lv, le = torch.zeros(S, dtype=F64), torch.zeros(S, dtype=F64)
    if smooth is not None:                               # the forward operator and its element-wise magnitude
        K, Ka, Kn = (torch.zeros(HW, HW, dtype=F64) for _ in range(3))
        o = torch.arange(HW)
        for t, (src, live) in enumerate(btaps):
            K.index_put_((o[live], src[live]), smooth[t].expand(int(live.sum())), accumulate=True)
            Ka.index_put_((o[live], src[live]), smooth[t].abs().expand(int(live.sum())), accumulate=True)
            Kn.index_put_((o[live], src[live]), torch.ones(int(live.sum()), dtype=F64), accumulate=True)
    for b in range(S):
        first, count = d["groups"][b].tolist()
        stack = torch.stack([m[b] for m in d["maps"]]).to(F64).reshape(n, HW, T)
        x = (vsum(V(stack), 0, n) * inv_n)
        x = x if wrong.get("no_x100") else x * 100.0
        xs = V(x.v[:, lo:hi], x.e[:, lo:hi])
        t = xs.v - xs.v.max(-1, keepdim=True).values
        e = V(t, xs.e + W * t.abs()).expf()
        z = vsum(e, -1, 7, keepdim=True)
        prob = e / z                                    # [HW][tokens lo .. hi-1]
        total = V(torch.zeros((), dtype=F64))
        imgs, gimgs, toks = [], [], []
        for it in range(first, first + count):
            tok, mid, k_fg, k_bg = d["items"][it, :4].tolist()
            label = f"{row.name} image {b} item {it}"
            M = d["masks"][mid, 0].to(F64)
            cmask, gt = d["masks"][mid, 1, :2 * side].to(F64), d["masks"][mid, 2, :2 * side].to(F64)
            cond.need(1 <= tok <= T - 2, f"{label}: token {tok}")
            img = _at(prob, (slice(None), tok - lo))
            if smooth is not None:
                sm = V(torch.zeros(HW, dtype=F64))
                for tp, (src, _) in enumerate(taps):
                    sm = sm + V(smooth[tp]) * _at(img, src)
            else:
                sm = img
            ranked = img if wrong.get("rank_unsmoothed") else sm
            vm, wm = ranked * V(M), ranked * V(1.0 - M)
            sf, of = topk_lowest(vm.v, k_fg)
            sb, ob = topk_lowest(wm.v, k_bg)
            for order, k, xx, which in ((of, k_fg, vm, "fg"), (ob, k_bg, wm, "bg")):
                if 0 < k < HW and _tie_or_gap(cond, xx, int(order[k - 1]), int(order[k]), stack, smooth, f"{label} {which} top-k"):
                    cond.ties.add("k")
            D = block_depth(HW)
            vm, wm = sm * V(M), sm * V(1.0 - M)
            gsm = V(torch.zeros(HW, dtype=F64))
            part = V(torch.zeros((), dtype=F64))
            if wrong.get("k0_nan") and (k_fg == 0 or k_bg == 0):
                part = V(torch.tensor(NAN, dtype=F64))
            if k_fg > 0:
                l_fg = 1.0 - vsum(_sel(vm, sf), -1, D) / float(k_fg)
                # T = 3 without smoothing: every probability is exactly 1, the sum of k ones is k and 1 - k / k is exactly 0
                cond.need(abs(float(l_fg.v)) > float(l_fg.e) or (float(l_fg.v) == 0.0 and T == 3 and smooth is None),
                          f"{label}: the sign of 1 - mean is inside its bound")
                if float(l_fg.v) > 0:
                    part = part + l_fg
                    gsm = gsm - _sel(V(M) / float(k_fg), sf)
            if k_bg > 0:
                l_bg = vsum(_sel(wm, sb), -1, D) / float(k_bg)
                cond.need(float(l_bg.v) == 0.0 or float(l_bg.v) > float(l_bg.e), f"{label}: the sign of the bg mean is inside its bound")
                if float(l_bg.v) > 0:
                    part = part + l_bg
                    gsm = gsm + _sel(V(1.0 - M) / float(k_bg), sb)
            # corner terms (:89-99): the maxima of every column (over y) and of every row (over x), lowest index first
            s2 = sm.v.reshape(side, side)
            pick = _last_max if wrong.get("argmax_high") else _first_max
            _, ay = pick(s2, 0)                          # per column x: the row index y of its maximum
            _, ax = pick(s2, 1)                          # per row y: the column index x of its maximum
            pos = torch.cat([ay * side + torch.arange(side), torch.arange(side) * side + ax])
            for q in range(2 * side):
                line = (torch.arange(side) * side + q) if q < side else ((q - side) * side + torch.arange(side))
                win = int(pos[q])
                rest = line[line != win]
                if rest.numel():
                    ru = int(rest[torch.argmax(sm.v[rest])])
                    if _tie_or_gap(cond, sm, win, ru, stack, smooth, f"{label} arg-max of line {q}"):
                        cond.ties.add("argmax")
            line = _at(sm, pos)
            dl = line - V(gt)
            live = cmask != 0
            cond.need(bool((~live | (dl.v == 0) | (dl.v.abs() > dl.e)).all()), f"{label}: the sign of max - gt is inside its bound")
            mean_over = 2 * side if wrong.get("corner_mean_2side") else side
            dist = vsum(dl.abs() * V(cmask) / float(mean_over), -1, 9)
            step = V(_sign(dl.v) * cmask) / float(mean_over)
            for half in (slice(0, side), slice(side, 2 * side)):
                add = V(torch.zeros(HW, dtype=F64))
                add.v[pos[half]], add.e[pos[half]] = step.v[half], step.e[half]
                gsm = gsm + add
            total = total + (part + dist)
            if smooth is not None:
                g = (Kn.t() @ torch.ones(HW, dtype=F64)) * W
                g = g / (1.0 - g)
                gimg = V(K.t() @ gsm.v, (1.0 + g) * (Ka.t() @ gsm.e) + g * (Ka.t() @ gsm.v.abs()))
            else:
                gimg = gsm
            imgs.append(img), gimgs.append(gimg), toks.append(tok)
        lossb = V(ls) * total
        lv[b], le[b] = lossb.v, lossb.e
        # soft-max backward over the tokens, the 1 / (n_maps H) of the mean, fan-out to every (layer, head) map
        c = V(torch.zeros(HW, dtype=F64))
        for img, gimg in zip(imgs, gimgs):
            c = c + gimg * img
        gs = (V(100.0) * V(ls)) * V(gsc)
        if not wrong.get("no_fanout"):
            gs = gs * inv_n
        p3 = e * (V(1.0) / z)
        gtok = V(torch.zeros(HW, hi - lo, dtype=F64))
        for tok, gimg in zip(toks, gimgs):
            col = V(torch.zeros(HW, hi - lo, dtype=F64))
            col.v[:, tok - lo], col.e[:, tok - lo] = gimg.v, gimg.e
            if wrong.get("no_token_add"):
                gtok.v[:, tok - lo], gtok.e[:, tok - lo] = gimg.v, gimg.e
            else:
                gtok = gtok + col
        dmap = (gs * p3) * (gtok - V(c.v.unsqueeze(-1), c.e.unsqueeze(-1)))
        for k in range(n_maps):
            gv[k][b, :, :, 1:T - 1] = dmap.v[:, 1 - lo:T - 1 - lo]
            ge[k][b, :, :, 1:T - 1] = dmap.e[:, 1 - lo:T - 1 - lo]
    out = {"loss": (lv, le), "_cond": cond}
    for k in range(n_maps):
        out[f"gmap{k}"] = (gv[k], ge[k])
    return out


def bd_emulate(row, d):
    p = row.p
    side, T, n_maps, H, S = p["side"], p["T"], p["n_maps"], p["H"], d["S"]
    HW, n = side * side, n_maps * H
    t32 = lambda v: torch.tensor(v, dtype=F32)
    one, ls, gsc, fside = t32(1.0), t32(p["ls"]), t32(p["gs"]), t32(float(side))
    inv_n = one / t32(float(n))
    smooth = d["smooth"]
    taps = _taps(side)
    i = torch.arange(HW)
    y, x = i // side, i % side
    gm = [torch.full((S, H, HW, T), SENT32, dtype=F32) for _ in range(n_maps)]
    loss = torch.zeros(S, dtype=F32)
    ok = torch.zeros(128, dtype=torch.bool)
    ok[1:T - 1] = True
    for b in range(S):
        first, count = d["groups"][b].tolist()
        a = torch.zeros(HW, T, dtype=F32)
        for k in range(n_maps):
            for h in range(H):
                a = a + d["maps"][k][b, h]
        xx = torch.full((HW, 128), -float("inf"), dtype=F32)
        xx[:, :T] = a * inv_n * 100.0
        xx[:, ~ok] = -float("inf")
        m = xx.max(-1, keepdim=True).values
        e = torch.exp(xx - m)                            # exp(-inf) = 0 for the tokens outside 1 .. T-2
        z = _butterfly(e[:, :64] + e[:, 64:]).unsqueeze(-1)
        total = t32(0.0)
        imgs, gimgs, toks = [], [], []
        for it in range(first, first + count):
            tok, mid, k_fg, k_bg = d["items"][it, :4].tolist()
            M = d["masks"][mid, 0]
            cmask, gt = d["masks"][mid, 1, :2 * side], d["masks"][mid, 2, :2 * side]
            img = (e / z)[:, tok]
            if smooth is not None:
                sm = torch.zeros(HW, dtype=F32)
                for tp, (src, _) in enumerate(taps):
                    sm = sm + smooth[tp] * img[src]
            else:
                sm = img
            vm, wm = sm * M, sm * (one - M)
            sf, _ = topk_lowest(vm, k_fg)
            sb, _ = topk_lowest(wm, k_bg)
            fg, bg = block_sum32(vm * sf), block_sum32(wm * sb)
            l_fg = one - fg / t32(float(k_fg)) if k_fg > 0 else t32(0.0)
            l_bg = bg / t32(float(k_bg)) if k_bg > 0 else t32(0.0)
            on_fg, on_bg = k_fg > 0 and bool(l_fg > 0), k_bg > 0 and bool(l_bg > 0)
            gsm = torch.zeros(HW, dtype=F32)
            if on_fg:
                gsm = gsm - (M / t32(float(k_fg))) * sf
            if on_bg:
                gsm = gsm + ((one - M) / t32(float(k_bg))) * sb
            s2 = sm.reshape(side, side)
            my, ay = _first_max(s2, 0)
            mx, ax = _first_max(s2, 1)
            line = torch.cat([my, mx])
            dl = line - gt
            dist = block_sum32(dl.abs() * cmask / fside)
            step = _sign32(dl) * cmask / fside
            gsm[ay * side + torch.arange(side)] += step[:side]
            gsm[torch.arange(side) * side + ax] += step[side:]
            total = total + (((l_fg if on_fg else t32(0.0)) + (l_bg if on_bg else t32(0.0))) + dist)
            if smooth is not None:                       # the kernel's gather: yo, dy, xo, dx ascending
                g = torch.zeros(HW, dtype=F32)
                for oy in (-1, 0, 1):
                    yo = y + oy
                    for dy in range(3):
                        hit_y = (yo >= 0) & (yo < side) & (_refl(yo + dy - 1, side) == y)
                        for ox in (-1, 0, 1):
                            xo = x + ox
                            for dx in range(3):
                                hit = hit_y & (xo >= 0) & (xo < side) & (_refl(xo + dx - 1, side) == x)
                                src = (yo.clamp(0, side - 1) * side + xo.clamp(0, side - 1))
                                g = torch.where(hit, g + smooth[dy * 3 + dx] * gsm[src], g)
                gimg = g
            else:
                gimg = gsm
            imgs.append(img), gimgs.append(gimg), toks.append(tok)
        loss[b] = ls * total
        c = torch.zeros(HW, dtype=F32)
        for img, gimg in zip(imgs, gimgs):
            c = c + gimg * img
        gs = 100.0 * ls * gsc * inv_n
        p3 = e[:, :T] * (one / z)
        gtok = torch.zeros(HW, T, dtype=F32)
        for tok, gimg in zip(toks, gimgs):
            gtok[:, tok] = gtok[:, tok] + gimg
        dmap = gs * p3 * (gtok - c.unsqueeze(-1))
        for k in range(n_maps):
            gm[k][b, :, :, 1:T - 1] = dmap[:, 1:T - 1]
    out = {"loss": loss}
    for k in range(n_maps):
        out[f"gmap{k}"] = gm[k]
    return out


def reference(row, d, **wrong):
    return (ca_reference if row.entry == "ca_energy" else bd_reference)(row, d, **wrong)


def emulate(row, d):
    return (ca_emulate if row.entry == "ca_energy" else bd_emulate)(row, d)


def outputs(ref):
    return {k: v for k, v in ref.items() if not k.startswith("_")}


# ---------------------------------------------------------------------------------------------
# the rows: the smallest shapes at which these kernels can still go wrong
# ---------------------------------------------------------------------------------------------
def _ca(label, **p):
    return Row("ca_energy", label, **p)


def _one(kind, mode="p", tok=5, mp=0, img=0):
    return ((mp, img, tok, ((kind, mode),)),)


_ROW_LIST = []
for _k in (0, 1, 2):                                     # each kind alone over the sizes: below a wave, one pass of the block,
    for _hw in (7, 256, 257, 576):                       # one element past it, three ragged passes
        _ROW_LIST.append(_ca(f"kind{_k} hw{_hw} H3", hw=(_hw,), H=3, cols=_one(_k)))
    _ROW_LIST.append(_ca(f"kind{_k} hw4096 H1", hw=(4096,), H=1, cols=_one(_k)))         # the LDS arrays to their last element
    _ROW_LIST.append(_ca(f"kind{_k} T3 tokens 0 and 2", hw=(7,), T=3, H=1, cols=_one(_k, tok=0) + _one(_k, tok=2)))
    _ROW_LIST.append(_ca(f"kind{_k} T77 tokens 0 and 76", hw=(257,), H=1, cols=_one(_k, tok=0) + _one(_k, tok=76)))
    _ROW_LIST.append(_ca(f"kind{_k} padded rows", hw=(257,), H=3, pad=63, cols=_one(_k) + _one(_k, tok=9)))
    _ROW_LIST.append(_ca(f"kind{_k} half mask gscale 1024", hw=(256,), H=1, mask="half", gscale=1024.0, cols=_one(_k)))
    _ROW_LIST.append(_ca(f"kind{_k} mask 0.5 everywhere", hw=(64,), H=1, mask="allhalf", cols=_one(_k)))
_ROW_LIST += [
    _ca("kind0 k one", hw=(257,), cols=_one(0, "one")),
    _ca("kind0 k_fg the in-mask count", hw=(257,), H=3, cols=_one(0, "fgall")),
    _ca("kind0 k_bg the out-of-mask count", hw=(257,), H=3, cols=_one(0, "bgall")),
    _ca("kind0 tied maps", hw=(576,), H=3, maps="tied", tie=True, cols=_one(0)),
    _ca("kind0 tied maps half mask", hw=(257,), H=1, maps="tied", mask="half", tie=True, cols=_one(0)),
    _ca("kind0 tied zeros selected", hw=(257,), H=3, maps="tied", tie=True, cols=_one(0, "zeros")),
    _ca("kind1 R equals A", hw=(257,), H=3, ref_equal=True, tie=True, cols=_one(1)),
    _ca("kind1 step 2 strided", hw=(256,), H=3, pad=5, dyn0=2, gap=37, cols=_one(1) + _one(1, tok=9)),
    _ca("column 0 1", hw=(257,), H=3, cols=((0, 0, 5, ((0, "p"), (1, ""))),)),
    _ca("column 1 0", hw=(257,), H=3, cols=((0, 0, 5, ((1, ""), (0, "p"))),)),
    _ca("column 2 1", hw=(257,), H=3, cols=((0, 0, 5, ((2, ""), (1, ""))),)),
    _ca("column 1 2", hw=(257,), H=3, cols=((0, 0, 5, ((1, ""), (2, ""))),)),
    _ca("column 0 1 1", hw=(257,), H=3, gscale=1024.0, cols=((0, 0, 5, ((0, "p"), (1, ""), (1, ""))),)),
    _ca("column 2 1 1", hw=(257,), H=3, cols=((0, 0, 5, ((2, ""), (1, ""), (1, ""))),)),
    _ca("column 0 1 2", hw=(64,), H=1, cols=((0, 0, 5, ((0, "p"), (1, ""), (2, ""))),)),
    _ca("column 1 0 2", hw=(64,), H=1, cols=((0, 0, 5, ((1, ""), (0, "p"), (2, ""))),)),
    _ca("column 2 1 0", hw=(64,), H=1, cols=((0, 0, 5, ((2, ""), (1, ""), (0, "p"))),)),
    _ca("column 0 2 1", hw=(64,), H=1, cols=((0, 0, 5, ((0, "p"), (2, ""), (1, ""))),)),
    _ca("column 1 2 0", hw=(64,), H=1, cols=((0, 0, 5, ((1, ""), (2, ""), (0, "p"))),)),
    _ca("column 2 0 1", hw=(64,), H=1, cols=((0, 0, 5, ((2, ""), (0, "p"), (1, ""))),)),
    _ca("column 0 0 tied", hw=(257,), H=1, maps="tied", tie=True, gscale=1024.0, cols=((0, 0, 5, ((0, "p"), (0, "one"))),)),
    _ca("two columns of one map", hw=(257,), H=3, cols=_one(0, tok=3) + _one(2, tok=4)),
    _ca("two maps of different HW", hw=(64, 576), H=3, cols=_one(0, mp=0) + _one(1, mp=0, tok=6) + _one(2, mp=1) + _one(1, mp=1, tok=6)),
    _ca("three images the middle without items", hw=(257,), H=3, S=3,
        cols=((0, 0, 5, ((0, "p"), (1, ""))),) + _one(2, tok=7, img=0) + _one(0, img=2) + _one(1, tok=7, img=2)),
    _ca("no items", hw=(64,), H=3, S=2, cols=()),
]
_B = (3, 4, 11, 12)


def _bd(label, **p):
    return Row("boxdiff", label, **p)


def _img(*objs):
    return tuple((tuple(t), tuple(b), dict(o)) for t, b, o in objs)


def _many(n, T):
    """n items on tokens 1 .. T-2 (tokens repeat), spread over three objects"""
    toks = [1 + i % (T - 2) for i in range(n)]
    cut = (n + 2) // 3
    boxes = ((3, 4, 11, 12), (0, 0, 5, 6), (8, 2, 16, 9))
    return _img(*[(toks[i * cut:(i + 1) * cut], boxes[i], {}) for i in range(3) if toks[i * cut:(i + 1) * cut]])


_SMALL_K = {2: dict(k_fg=1, k_bg=1), 3: dict(k_fg=2, k_bg=2)}
_K3 = _SMALL_K[3]
_N64 = (LDS_DEFAULT // (16 * 16 * 4) - 7) // 2           # 28 items: the last count inside the default LDS limit
for _s, _box in ((2, (0, 0, 1, 1)), (3, (1, 0, 3, 2)), (16, _B), (24, (5, 3, 17, 20)), (32, (4, 6, 30, 19))):
    for _sm in (None, "gauss", "asym"):
        # a fifth of the count is 0 at sides 2 and 3: there the counts are given, so that the fg top-k gradient runs too
        _ROW_LIST.append(_bd(f"side{_s} smooth {_sm}", side=_s, smooth=_sm, n_maps=2, H=2,
                             images=(_img(((5, 9), _box, _SMALL_K.get(_s, {}))),)))
_ROW_LIST += [
    _bd("T3 the single token", T=3, side=3, smooth=None, images=(_img(((1,), (1, 0, 3, 2), _K3)),)),
    _bd("T64 tokens 1 62", T=64, side=3, smooth="asym", images=(_img(((1, 62), (1, 0, 3, 2), _K3)),)),
    _bd("T65 tokens 1 63", T=65, side=3, smooth="asym", images=(_img(((1, 63), (1, 0, 3, 2), _K3)),)),
    _bd("T77 tokens 1 63 64 75", T=77, side=3, smooth="asym", images=(_img(((1, 63, 64, 75), (1, 0, 3, 2), _K3)),)),
    _bd("T128 tokens 1 63 64 126", T=128, side=3, smooth="asym", images=(_img(((1, 63, 64, 126), (1, 0, 3, 2), _K3)),)),
    _bd("five maps of eight heads", n_maps=5, H=8, smooth="asym", ls=10.0, gs=1024.0, images=(_img(((5, 9), _B, {})),)),
    _bd("one map of one head scaled", n_maps=1, H=1, smooth="asym", ls=10.0, gs=0.25, images=(_img(((5,), _B, {})),)),
    _bd("two items on one token and two objects on one token", smooth="asym",
        images=(_img(((5, 5), _B, {}), ((9, 5), (0, 0, 6, 5), {})),)),
    _bd("k_fg 0", smooth="asym", images=(_img(((5,), _B, dict(k_fg=0))),)),
    _bd("k_bg 0", smooth="asym", images=(_img(((5,), _B, dict(k_bg=0))),)),
    _bd("both k 0", smooth=None, images=(_img(((5,), _B, dict(k_fg=0, k_bg=0))),)),
    _bd("box on the border", smooth="asym", images=(_img(((5,), (0, 0, 16, 7), {}), ((9,), (9, 0, 16, 16), {})),)),
    _bd("all-zero corner masks", smooth="asym", images=(_img(((5,), _B, dict(corner="zero"))),)),
    _bd("half box mask", smooth="asym", images=(_img(((5,), _B, dict(half=True))),)),
    _bd("duplicated rows tied top-k and arg-max", smooth=None, dup=True, tie=True, n_maps=2, H=2,
        images=(_img(((5, 9), _B, dict(k_fg=13, k_bg=37))),)),
    _bd("three images the middle without items", smooth="asym", n_maps=2, H=2,
        images=(_img(((5,), _B, {})), (), _img(((9, 70), (0, 2, 9, 16), {})))),
    _bd(f"lds {_N64} items below 64 KB", smooth="gauss", reseed=1, images=(_many(_N64, 77),)),
    _bd(f"lds {_N64 + 1} items above 64 KB", smooth="gauss", images=(_many(_N64 + 1, 77),)),
    _bd(f"lds {bd_max_items(16)} items the largest count", smooth="gauss", images=(_many(bd_max_items(16), 77), _img(((5,), _B, {})))),
    _bd("lds side 32 the largest count", side=32, smooth="gauss", images=(_many(bd_max_items(32), 77),)),
]
ROWS_BY_NAME = {r.name: r for r in _ROW_LIST}
assert len(ROWS_BY_NAME) == len(_ROW_LIST)


def rows_of(entry):
    return [r for r in _ROW_LIST if r.entry == entry]


def kinds_of(row, d=None):
    """the label under which a row's ratio is reported: the kinds it holds (ca_energy), the smoothing (BoxDiff)"""
    if row.entry == "boxdiff":
        return "boxdiff smooth " + str(row.smooth)
    ks = sorted({k for col in row.cols for k, _ in col[3]})
    return "ca_energy kind " + ("+".join(map(str, ks)) if ks else "none")


LABELS = sorted({kinds_of(r) for r in _ROW_LIST})


def _r(entry, label):
    name = f"{entry}:{label}"
    assert name in ROWS_BY_NAME, name
    return name


# wrong answers of the reference: name -> (row, the reference's `wrong` switch)
MUTATIONS = {
    "ca: the tie goes to the highest index": (_r("ca_energy", "kind0 tied maps"), "tie_high"),
    "ca: k + 1 elements are selected": (_r("ca_energy", "kind0 hw257 H3"), "k_plus_1"),
    "ca: the gradient loses its m": (_r("ca_energy", "kind0 mask 0.5 everywhere"), "no_m"),
    "ca: the bg term uses m for 1 - m": (_r("ca_energy", "kind0 hw257 H3"), "bg_uses_m"),
    "ca: the mask row strided by HW": (_r("ca_energy", "kind0 padded rows"), "mask_stride_hw"),
    "ca: the ref slice of step 0 at dyn[0] = 2": (_r("ca_energy", "kind1 step 2 strided"), "step0"),
    "ca: the ref head stride is HW": (_r("ca_energy", "kind1 step 2 strided"), "ref_head_stride"),
    "ca: the second item overwrites the first": (_r("ca_energy", "column 0 1"), "overwrite"),
    "ca: grad_scale applied to the loss": (_r("ca_energy", "kind2 half mask gscale 1024"), "gscale_on_loss"),
    "ca: the ratio gradient misses - sm": (_r("ca_energy", "kind2 hw257 H3"), "ratio_no_sm"),
    "ca: REF_EPS missing": (_r("ca_energy", "kind1 hw257 H3"), "no_eps"),
    "ca: a loss includes another image's items": (_r("ca_energy", "three images the middle without items"), "cross_image"),
    "boxdiff: the soft-max includes tokens 0 and T-1": (_r("boxdiff", "side16 smooth asym"), "softmax_all"),
    "boxdiff: the x100 missing": (_r("boxdiff", "side16 smooth asym"), "no_x100"),
    "boxdiff: smooth transposed": (_r("boxdiff", "side16 smooth asym"), "smooth_transposed"),
    "boxdiff: the smoothing backward pads with zeros": (_r("boxdiff", "side16 smooth gauss"), "zero_pad_backward"),
    "boxdiff: top-k ranked on the unsmoothed image": (_r("boxdiff", "side16 smooth asym"), "rank_unsmoothed"),
    "boxdiff: the corner arg-max goes to the highest index": (_r("boxdiff", "duplicated rows tied top-k and arg-max"), "argmax_high"),
    "boxdiff: the corner mean over 2 side": (_r("boxdiff", "side16 smooth asym"), "corner_mean_2side"),
    "boxdiff: the 1 / (n_maps H) fan-out missing": (_r("boxdiff", "side16 smooth asym"), "no_fanout"),
    "boxdiff: two items on one token do not add": (_r("boxdiff", "two items on one token and two objects on one token"), "no_token_add"),
    "boxdiff: a term with k = 0 gives NaN": (_r("boxdiff", "k_fg 0"), "k0_nan"),
}


# ---------------------------------------------------------------------------------------------
# host refusals: the layout of small_kernel_cases (operands 1 MiB apart, None = NULL, a byte offset, or (operand, offset))
# ---------------------------------------------------------------------------------------------
ARGS = {
    "lgd_ca_energy_f32": "p:maps p:gmaps p:map_hw p:items p:coefs p:masks p:refs refs_step_stride p:dyn p:groups n_groups n_items "
                         "n_samples H T max_hw grad_scale p:partial p:loss stream",
    "lgd_boxdiff_energy_f32": "p:maps p:gmaps n_maps side p:items p:masks p:smooth p:groups n_samples max_items H T loss_scale "
                              "grad_scale p:loss stream",
}
BASE = {
    "lgd_ca_energy_f32": dict(refs_step_stride=3 * 256, n_groups=2, n_items=3, n_samples=1, H=3, T=77, max_hw=256, grad_scale=1.0),
    "lgd_boxdiff_energy_f32": dict(n_maps=2, side=16, n_samples=1, max_items=4, H=2, T=77, loss_scale=1.0, grad_scale=1.0),
}
ALIGN = {fn: {n[2:]: (8 if n[2:] in ("maps", "gmaps") else 4) for n in a.split() if n.startswith("p:")} for fn, a in ARGS.items()}
OPTIONAL = {"lgd_ca_energy_f32": {"gmaps", "refs", "dyn"}, "lgd_boxdiff_energy_f32": {"gmaps", "smooth"}}
RULES = {
    "lgd_ca_energy_f32": [("refs without dyn", dict(dyn=None)), ("n_items = -1", dict(n_items=-1)), ("n_groups = -1", dict(n_groups=-1)),
                          ("n_groups = 0 with items", dict(n_groups=0)), ("n_samples = 0", dict(n_samples=0)), ("H = 0", dict(H=0)),
                          ("T = 0", dict(T=0)), ("max_hw = 0", dict(max_hw=0)), ("max_hw = 4097", dict(max_hw=4097)),
                          ("refs_step_stride = -1", dict(refs_step_stride=-1)),
                          ("loss NULL without items", dict(loss=None, n_items=0, n_groups=0))],
    "lgd_boxdiff_energy_f32": [("n_maps = 0", dict(n_maps=0)), ("n_samples = 0", dict(n_samples=0)), ("H = 0", dict(H=0)),
                               ("max_items = -1", dict(max_items=-1))],
}


def pointers(fn):
    return [n[2:] for n in ARGS[fn].split() if n.startswith("p:")]


def _generated(fn):
    rows = []
    for p in pointers(fn):
        if p not in OPTIONAL[fn]:
            rows.append((fn, f"{p} NULL", {p: None}))
        rows.append((fn, f"{p} off {ALIGN[fn][p]} bytes", {p: ALIGN[fn][p] // 2}))
    return rows


REFUSALS = [r for fn in ARGS for r in _generated(fn) + [(fn, label, change) for label, change in RULES[fn]]]
UNSUPPORTED = [("lgd_boxdiff_energy_f32", what, change) for what, change in (
    ("side 1", dict(side=1)), ("side 33", dict(side=33)), ("T 2", dict(T=2)), ("T 129", dict(T=129)),
    ("one item past the LDS at 16 x 16", dict(max_items=bd_max_items(16) + 1)),
    ("one item past the LDS at 32 x 32", dict(side=32, max_items=bd_max_items(32) + 1)))]
# calls the library serves: the optional operands left out, the limits themselves, no items
ACCEPTED = [("lgd_ca_energy_f32", {}), ("lgd_ca_energy_f32", dict(gmaps=None)), ("lgd_ca_energy_f32", dict(refs=None, dyn=None)),
            ("lgd_ca_energy_f32", dict(refs=None)), ("lgd_ca_energy_f32", dict(max_hw=4096)), ("lgd_ca_energy_f32", dict(refs_step_stride=0)),
            ("lgd_ca_energy_f32", dict(n_items=0, n_groups=0, maps=None, map_hw=None, items=None, coefs=None, masks=None,
                                       partial=None, groups=None, refs=None, dyn=None, gmaps=None)),
            ("lgd_boxdiff_energy_f32", {}), ("lgd_boxdiff_energy_f32", dict(gmaps=None)), ("lgd_boxdiff_energy_f32", dict(smooth=None)),
            ("lgd_boxdiff_energy_f32", dict(max_items=0)), ("lgd_boxdiff_energy_f32", dict(side=2, T=3)),
            ("lgd_boxdiff_energy_f32", dict(side=32, T=128, max_items=bd_max_items(32))),
            ("lgd_boxdiff_energy_f32", dict(max_items=bd_max_items(16)))]


def call_args(fn, change, base=P):
    """The argument list of BASE[fn] with `change` applied; operands 1 MiB apart from `base`, a NULL stream."""
    vals = dict(BASE[fn], stream=None)
    ptrs = pointers(fn)
    vals.update({p: 0 for p in ptrs})
    vals.update(change)
    out = []
    for n in ARGS[fn].split():
        if not n.startswith("p:"):
            out.append(vals[n])
            continue
        v = vals[n[2:]]
        if v is None:
            out.append(None)
        else:
            slot, off = (v[0], v[1]) if isinstance(v, tuple) else (n[2:], v)
            out.append(base + (ptrs.index(slot) << 20) + off)
    return out

"""Cases of the safety checker (csrc/safety.hip, lgd_amd/safety.py, lgd_amd/clip_processor.py), shared by
tests/test_safety_cpu.py and tests/test_safety_gpu.py.

The restatements are the contract include/lgd_hip.h states for lgd_safety_head_f32 ([ext] diffusers 0.18.0
StableDiffusionSafetyChecker.forward): `decide` in numpy fp32, operation by operation, for the known answers and the
mutations; `head_reference` in fp64 for the GPU comparison; `clip_pixel_values` for the processor (Pillow + numpy)."""
import numpy as np

F32 = np.float32
ADJ = F32(0.01)
UNIT = 2.0 ** -24                                   # fp32 unit roundoff


# ---------------------------------------------------------------------------------------------
# the decision rule
# ---------------------------------------------------------------------------------------------
def hit_reference(s):
    """The reference's test, `round(score, 3) > 0` of a numpy.float32 score."""
    return bool(round(F32(s), 3) > 0)


def hit(s):
    """The kernel's form of it: the fp32 product against 0.5."""
    return bool(F32(s) * F32(1000.0) > F32(0.5))


def decide(cos, w, n_special, mutation=None):
    """cos, w: one value per row, special rows first -> dict(scores fp32 [rows], hits [rows], has_nsfw, special).
    mutation: None, or one of the wrong readings of the rule that MUTATIONS names."""
    cos, w = np.asarray(cos, F32), np.asarray(w, F32)
    test = (lambda s: bool(s > 0)) if mutation == "no rounding" else hit
    rows = len(cos)
    scores, hits = np.zeros(rows, F32), [False] * rows
    adj = F32(0.0)
    if mutation == "parallel adjustment":               # any special hit (judged without adjustment) adjusts EVERY row
        if any(test((cos[j] - w[j]) + F32(0.0)) for j in range(n_special)):
            adj = ADJ
    for j in range(rows):
        scores[j] = (cos[j] - w[j]) + adj
        hits[j] = test(scores[j])
        if j < n_special and hits[j] and mutation != "parallel adjustment":
            adj = ADJ
    special = any(hits[:n_special])
    nsfw = any(hits) if mutation == "specials count as nsfw" else any(hits[n_special:])
    return dict(scores=scores, hits=hits, has_nsfw=nsfw, special=special)


MUTATIONS = ("parallel adjustment", "no rounding", "specials count as nsfw")

# (name, cos - w of the special rows, cos - w of the concept rows, hits of all rows, has_nsfw, special): w is 0 and cos the
# score itself, so that every value is the fp32 number written here
RULE_CASES = [
    ("0.0004 is no hit", [], [0.0004], [False], False, False),
    ("0.0006 is a hit", [], [0.0006], [True], True, False),
    ("exactly 0.0005 is no hit", [], [0.0005], [False], False, False),
    ("a concept at -0.005 without a special hit", [0.0004], [-0.005], [False, False], False, False),
    ("a concept at -0.005 behind a special hit", [0.0006], [-0.005], [True, True], True, True),
    ("a special row at -0.005 behind a special hit", [0.0006, -0.005], [-0.5], [True, True, False], False, True),
    ("a special row at -0.005 before a special hit", [-0.005, 0.0006], [-0.02], [False, True, False], False, True),
    ("a special row at -0.005 alone", [-0.005], [-0.02], [False, False], False, False),
    ("a special hit alone is not nsfw", [0.0006], [-0.5], [True, False], False, True),
]


# ---------------------------------------------------------------------------------------------
# the head in fp64, and the cases of the GPU comparison
# ---------------------------------------------------------------------------------------------
def cosines64(e, rows):
    n = lambda x: x / np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-12)
    return n(e.astype(np.float64)) @ n(rows.astype(np.float64)).T


def head_reference(cos, w, n_special):
    """cos fp64 [B, rows], w fp32 [rows] -> (scores fp64 [B, rows], flags int32 [B, 2], through_adjustment bool [B]): the
    rule in fp64 with the boundary at 0.0005 (the cases keep every score away from it)."""
    B, rows = cos.shape
    w64, adj64 = w.astype(np.float64), float(ADJ)
    scores, flags, through = np.zeros((B, rows)), np.zeros((B, 2), np.int32), np.zeros(B, bool)
    for b in range(B):
        adj = 0.0
        for j in range(rows):
            scores[b, j] = (cos[b, j] - w64[j]) + adj
            if scores[b, j] > 0.0005:
                if j < n_special:
                    adj, flags[b, 1] = adj64, 1
                else:
                    flags[b, 0] = 1
        through[b] = bool(flags[b, 0]) and not bool(((cos[b, n_special:] - w64[n_special:]) > 0.0005).any())
    return scores, flags, through


def cosine_bound(D):
    return (D + 8) * UNIT


HEAD_SHAPES = [(B, D, ns, nc, D) for B in (1, 3, 65) for D in (4, 36, 768, 1024) for ns, nc in ((3, 17), (0, 1), (32, 64))]
HEAD_SHAPES.append((3, 36, 3, 17, 44))                 # ld_embeds > D


def head_case(B, D, ns, nc, ld, seed=0):
    """Operands of one head call.  Every threshold starts above every image's cosine (nothing hits); then special row 0 is
    lowered under image 1's cosine, concept row 0 under image 2's and concept row 1 to 0.005 ABOVE image 1's (a hit only
    through the adjustment), each where the shape has that row and image.  Every threshold is then moved up in steps of
    1e-4 until every image's fp64 score is farther than the margin from 0.0005 — under the adjustment state the rows before
    it leave, which is why the rows are fixed in order."""
    g = np.random.default_rng(seed + 7919 * (B + 131 * D + 17 * ns + nc))
    e = g.standard_normal((B, ld)).astype(F32)
    rows = g.standard_normal((ns + nc, D)).astype(F32)
    cos = cosines64(e[:, :D], rows)
    margin = 2 * cosine_bound(D)
    w = (cos.max(axis=0) + 0.05).astype(F32)
    if ns and B > 1:
        w[0] = F32(cos[1, 0] - 0.003)
    w[ns] = F32(cos[2 % B, ns] - 0.003)
    if nc > 1 and ns and B > 1:
        w[ns + 1] = F32(cos[1, ns + 1] + 0.005)
    adj = np.zeros(B)
    for j in range(ns + nc):
        for _ in range(10000):
            s = cos[:, j] - float(w[j]) + adj
            if (np.abs(s - 0.0005) > 2 * margin).all():          # twice the margin the tests assert
                break
            w[j] = F32(float(w[j]) + 1e-4)
        else:
            raise AssertionError("no threshold with the margin found")
        if j < ns:
            adj = np.where(s > 0.0005, float(ADJ), adj)
    return dict(e=e, special=rows[:ns], special_w=w[:ns], concepts=rows[ns:], concept_w=w[ns:], cos=cos, w=w, margin=margin)


def outcome(flags_row, through):
    return ("concept through the adjustment" if through else "concept" if flags_row[0] else
            "special only" if flags_row[1] else "nothing")


# ---------------------------------------------------------------------------------------------
# refusals: both entry points through the library with placeholder pointers (the pattern of tests/small_kernel_cases.py)
# ---------------------------------------------------------------------------------------------
P = 1 << 32
ARGS = {
    "lgd_safety_head_f32": "p:embeds ld_embeds p:special p:special_w n_special p:concepts p:concept_w n_concepts p:scores "
                           "p:flags B D stream",
    "lgd_blank_flagged_u8": "p:images image_bytes p:flags flag_stride N stream",
}
BASE = {
    "lgd_safety_head_f32": dict(ld_embeds=8, n_special=3, n_concepts=17, B=4, D=8),
    "lgd_blank_flagged_u8": dict(image_bytes=4099, flag_stride=2, N=4),
}
ALIGN = {
    "lgd_safety_head_f32": dict(embeds=16, special=16, concepts=16, special_w=4, concept_w=4, scores=4, flags=4),
    "lgd_blank_flagged_u8": dict(flags=4),               # images needs no alignment
}


def pointers(fn):
    return [n[2:] for n in ARGS[fn].split() if n.startswith("p:")]


def call_args(fn, change, base=P):
    """The argument list of BASE[fn] with `change` applied; operands 1 MiB apart from `base`, a NULL stream.  A pointer's
    change is None (NULL), a byte offset, or (another operand's name, byte offset)."""
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


def _generated(fn, counts):
    rows = [(fn, f"{p} NULL", {p: None}) for p in pointers(fn)]
    rows += [(fn, f"{p} off {a // 2} bytes", {p: a // 2}) for p, a in ALIGN[fn].items()]
    for c in counts:
        rows += [(fn, f"{c} = 0", {c: 0}), (fn, f"{c} = -1", {c: -1})]
    return rows


_H, _B = "lgd_safety_head_f32", "lgd_blank_flagged_u8"
REFUSALS = _generated(_H, ("B", "D", "n_concepts")) + [
    (_H, "n_special = -1", dict(n_special=-1)),
    (_H, "D = 6", dict(D=6)),
    (_H, "ld_embeds < D", dict(ld_embeds=4)),
    (_H, "ld_embeds = 10", dict(ld_embeds=10)),
    (_H, "scores is embeds", dict(scores=("embeds", 0))),
    (_H, "scores inside concepts", dict(scores=("concepts", 64))),
    (_H, "scores over concept_w", dict(scores=("concept_w", 0))),
    (_H, "flags inside embeds", dict(flags=("embeds", 96))),
    (_H, "flags over special_w", dict(flags=("special_w", 8))),
    (_H, "flags inside special", dict(flags=("special", 32))),
    (_H, "flags inside scores", dict(flags=("scores", 16))),
] + _generated(_B, ("image_bytes", "flag_stride", "N")) + [
    (_B, "flags inside the images", dict(flags=("images", 4096))),
    (_B, "flags inside the last image", dict(flags=("images", 4 * 4099 - 4))),
]
UNSUPPORTED = [(_H, "D = 1028", dict(D=1028, ld_embeds=1028)), (_H, "n_concepts = 65", dict(n_concepts=65)),
               (_H, "n_special = 33", dict(n_special=33)), (_H, "B = 65536", dict(B=65536))]
# calls the library accepts: the base calls, no special rows with NULL operands, an unaligned image base, the limits
ACCEPTED = [(_H, {}), (_H, dict(n_special=0, special=None, special_w=None)), (_H, dict(D=1024, ld_embeds=1024, B=1)),
            (_H, dict(n_special=32, n_concepts=64)), (_B, {}), (_B, dict(images=1)), (_B, dict(images=15, image_bytes=1)),
            (_B, dict(flag_stride=1))]


# ---------------------------------------------------------------------------------------------
# the processor
# ---------------------------------------------------------------------------------------------
def clip_geometry(h, w, s):
    """((H, W) of the resize, (top, left) of the crop): shortest edge to s, the other side int(s * long / short)."""
    short, long_ = min(h, w), max(h, w)
    other = int(s * long_ / short)
    H, W = (s, other) if h <= w else (other, s)
    return (H, W), ((H - s) // 2, (W - s) // 2)


def clip_pixel_values(images, s, mean, std, rescale=1.0 / 255.0):
    """uint8 (N, h, w, 3) -> fp32 (N, 3, s, s): Pillow BICUBIC, centre crop, (v * rescale - mean) / std in fp32."""
    from PIL import Image
    (H, W), (top, left) = clip_geometry(images.shape[1], images.shape[2], s)
    out = []
    for im in images:
        r = np.asarray(Image.fromarray(im).resize((W, H), Image.BICUBIC))[top:top + s, left:left + s].astype(F32)
        out.append(((r * F32(rescale) - np.asarray(mean, F32)) / np.asarray(std, F32)).transpose(2, 0, 1))
    return np.stack(out)

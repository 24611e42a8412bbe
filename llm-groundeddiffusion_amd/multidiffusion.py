"""MultiDiffusion, the region-prompt baseline of the reference (generation/multidiffusion.py, `generate.py --run-model
multidiffusion`), on the HIP engine.

What the reference's `run()` reaches: one 512 x 512 view (get_views(512, 512) yields one window), indep_uncond=True,
normalization=False, DDIM (eta 0) from the checkpoint's scheduler config.  Per step i:
    x_k = latent for every prompt k; while i < bootstrapping, for k >= 1 outside the region of prompt k the latent is
          replaced by add_noise(bg[pick], start latent, t_i) (a randomly picked constant-colour background);
    the UNet runs on [x_0 .. x_{P-1}] * 2 with text [uncond_k; cond_k];
    latent <- sum_k mask_k * DDIM(x_k, CFG(eps_k)).
Host prep (boxes -> disjoint masks and prompts) is restated below from utils/parse.py and generation/multidiffusion.py,
which do not exist where this runs.  The device side is one launch of lgd_multidiffusion_step_f32 per step after the
UNet (plus one to write step 0's input rows), and the UNet plan and that launch are captured as one hipGraph.

What `MultiDiffusion.generate` itself offers beyond that, panoramas: V = len(get_views(H, W)) overlapping 64 x 64 latent
windows at stride 8, each denoised per prompt as above, then
    latent <- value / count where count > 0,  value = sum over views and prompts of mask_k * DDIM(x_k, cfg_k) placed at
              the view, count = the same sum of mask_k (normalization; without it count = 1 and overlapping views sum),
    cfg_k = eps_uncond_0 + gs * (eps_cond_k - eps_uncond_k) unless indep_uncond.
That path (_generate_views) is taken for any other latent size or flag value and leaves the single-view path as it was:
chunks of views per UNet call, lgd_multidiffusion_views_f32 before (input rows) and after (gather into value / count, and
behind the last chunk the latent) each call, one step one hipGraph.

Precision: UNet in fp16 with fp32 accumulation, CFG and the step in fp32, the HIP VAE in fp16 (the reference runs the
VAE in fp32 and the UNet and CFG in fp16 under autocast).
"""

import numpy as np
import torch

from . import ops
from .loop import LoopState, clamp_steps, history_of, run_steps
from .scheduler import DDIMScheduler

F32 = torch.float32
SIZE = (512, 512)                 # utils/parse.py:21-24: box_scale (h, w)
LATENT_SCALE = 0.18215            # generation/multidiffusion.py:157,163
WINDOW = 64                       # get_views: the latent window of a view (stride 8)


# ---- host prep --------------------------------------------------------------------------------------------------------
def filter_boxes(gen_boxes, scale_boxes=True, ignore_background=True, max_scale=3):
    """utils/parse.py:126-226: drop empty and background boxes, then (scale_boxes, the default, and forced when a box is
    out of bounds) shift and scale all boxes so that they span the width, shift vertically into the frame, strip a
    trailing '.' from the names and round to ints.  Boxes are dicts {name, bounding_box} or (name, box) pairs."""
    if gen_boxes is None or len(gen_boxes) == 0:
        return []
    size_h, size_w = SIZE
    box_dict_format = False
    kept = []
    for gen_box in gen_boxes:
        if isinstance(gen_box, dict):
            if not gen_box['bounding_box']:
                continue
            name, [bbox_x, bbox_y, bbox_w, bbox_h] = gen_box['name'], gen_box['bounding_box']
            box_dict_format = True
        else:
            if not gen_box[1]:
                continue
            name, [bbox_x, bbox_y, bbox_w, bbox_h] = gen_box
        if bbox_w <= 0 or bbox_h <= 0:
            continue
        if ignore_background:
            if (bbox_w >= size_w and bbox_h >= size_h) or bbox_x > size_w or bbox_y > size_h:
                continue
        if bbox_x < 0 or bbox_y < 0 or bbox_x + bbox_w > size_w or bbox_y + bbox_h > size_h:
            scale_boxes = True                                                    # utils/parse.py:154-157
        kept.append(gen_box)
    gen_boxes = kept
    if len(gen_boxes) == 0:
        return []
    box = (lambda b: b['bounding_box']) if box_dict_format else (lambda b: b[1])
    x_min = min(box(b)[0] for b in gen_boxes)
    x_max = max(box(b)[0] + box(b)[2] for b in gen_boxes)
    y_min = min(box(b)[1] for b in gen_boxes)
    y_max = max(box(b)[1] + box(b)[3] for b in gen_boxes)
    if (x_max - x_min) == 0:
        return []
    shift = -x_min
    scale = min(size_w / (x_max - x_min), size_h / (y_max - y_min), max_scale)
    out = []
    for gen_box in gen_boxes:
        if box_dict_format:
            name, [bbox_x, bbox_y, bbox_w, bbox_h] = gen_box['name'], gen_box['bounding_box']
        else:
            name, [bbox_x, bbox_y, bbox_w, bbox_h] = gen_box
        if scale_boxes:                                                           # utils/parse.py:196-212
            bbox_x = (bbox_x + shift) * scale
            bbox_y = bbox_y * scale
            bbox_w, bbox_h = bbox_w * scale, bbox_h * scale
            bbox_y_offset = 0
            if y_min * scale + bbox_y_offset < 0:
                bbox_y_offset -= y_min * scale
            if y_max * scale + bbox_y_offset >= size_h:
                bbox_y_offset -= y_max * scale - size_h
            bbox_y += bbox_y_offset
            if bbox_y < 0:
                bbox_y, bbox_h = 0, bbox_h - bbox_y
        name = name.rstrip(".")
        bounding_box = (int(np.round(bbox_x)), int(np.round(bbox_y)), int(np.round(bbox_w)), int(np.round(bbox_h)))
        out.append({'name': name, 'bounding_box': bounding_box} if box_dict_format else (name, bounding_box))
    return out


def boxes_to_masks_prompts(boxes, fg_negative_prompt, first_top=True):
    """generation/multidiffusion.py:303-336: disjoint 512 x 512 float32 masks (a pixel belongs to the box painted last;
    first_top paints in reverse so that the first box wins), prompt = box name, one negative prompt per box."""
    h, w = SIZE
    if first_top:
        boxes = boxes[::-1]
    inds_arr = np.full((h, w), fill_value=-1, dtype=np.int32)
    prompts = []
    for ind, box in enumerate(boxes):
        name, [bbox_x, bbox_y, bbox_w, bbox_h] = box["name"], box["bounding_box"]
        inds_arr[bbox_y:bbox_y + bbox_h, bbox_x:bbox_x + bbox_w] = ind
        prompts.append(f"{name}")
    masks = [(inds_arr == ind).astype(np.float32) for ind in range(len(boxes))]
    negs = [fg_negative_prompt] * len(masks)
    if first_top:
        masks, prompts, negs = masks[::-1], prompts[::-1], negs[::-1]
    return masks, prompts, negs


def preprocess_mask(mask, h, w):
    """generation/multidiffusion.py:288-300 for an array mask: threshold at 0.5, nearest resize -> (1, 1, h, w)."""
    m = np.asarray(mask).astype(np.float32)[None, None]
    m[m < 0.5] = 0
    m[m >= 0.5] = 1
    return torch.nn.functional.interpolate(torch.from_numpy(m), size=(h, w), mode="nearest")


def prepare(gen_boxes, bg_prompt, bg_negative, fg_negative_prompt, extra_neg_prompt="", first_top=False):
    """The host half of multidiffusion.run (generation/multidiffusion.py:366-451) -> dict(masks (P, 1, 64, 64) fp32
    [background; boxes], prompts, negative_prompts, boxes (the filtered boxes)).  P = 1 + number of boxes."""
    gen_boxes = [{"name": b[0], "bounding_box": b[1]} if not isinstance(b, dict) else b for b in gen_boxes]
    gen_boxes = filter_boxes(gen_boxes)
    if extra_neg_prompt:
        full_bg_negative = extra_neg_prompt + ", " + bg_negative
        full_fg_negative = extra_neg_prompt + ", " + fg_negative_prompt
    else:
        full_bg_negative, full_fg_negative = bg_negative, fg_negative_prompt
    masks, fg_prompts, fg_negs = boxes_to_masks_prompts(gen_boxes, full_fg_negative, first_top=first_top)
    lh, lw = SIZE[0] // 8, SIZE[1] // 8
    if masks:
        fg = torch.cat([preprocess_mask(m, lh, lw) for m in masks])
    else:
        fg = torch.zeros((0, 1, lh, lw), dtype=F32)
    bg = 1 - torch.sum(fg, dim=0, keepdim=True)                                  # bg_weight == 0.0
    bg[bg < 0] = 0
    return dict(masks=torch.cat([bg, fg]), prompts=[bg_prompt] + fg_prompts, negative_prompts=[full_bg_negative] + fg_negs,
                boxes=gen_boxes)


def get_views(panorama_height, panorama_width, window_size=64, stride=8):
    """generation/multidiffusion.py:30-43: the (h_start, h_end, w_start, w_end) latent windows of a panorama given in
    pixels, row-major; a size that is no window + whole strides leaves a right / bottom margin no view covers."""
    # true division and float floor division, as there: 516 pixels are 64.5 latent rows and still one window
    rows = int((panorama_height / 8 - window_size) // stride + 1)
    cols = int((panorama_width / 8 - window_size) // stride + 1)
    starts = [(r * stride, c * stride) for r in range(rows) for c in range(cols)] if rows > 0 and cols > 0 else []
    return [(hs, hs + window_size, ws, ws + window_size) for hs, ws in starts]


# ---- the random draws of one run --------------------------------------------------------------------------------------
def draw_randomness(encoder, device, seed, n_boot, n_prompts, steps, in_channels=4, size=SIZE, chunk=4, n_views=1,
                    bg_size=None):
    """The reference's draws, call for call (generation/multidiffusion.py:170-197,205-214,236 with run():443-447):
      seed_everything(seed); torch.rand(n_boot, 3, device) -> background colours;
      per background in order: constant image, 2*img-1, VAE posterior sample (one device randn) * 0.18215;
      torch.manual_seed(seed); start latent randn (1, C, H/8, W/8) on the CPU;
      per step i < n_boot and per view in order: torch.randint(0, n_boot, (P-1,)) on the CPU (nothing else draws inside
      the loop).
    Explicit generators seeded like the global ones give the same numbers without touching process state.
    encoder: .encode_moments(image [B,3,H,W] in [-1,1]) -> (mean, logvar clamped to [-30, 20]) (HipVAEEncoder); the
    moments may be computed in batches, the posterior draws follow the reference's order.
    size: pixels of the start latent (the panorama); bg_size: pixels of the background images, `size` when None (a
    panorama passes 512 x 512, what get_random_background always encodes, line 113-118); n_views: len(get_views(*size)).
    Returns dict(colours (n_boot,3), bg_latents (n_boot,C,bh/8,bw/8) on `device`, start_latent (1,C,h/8,w/8) CPU,
    picks int64 CPU: (min(n_boot, steps), P-1) for n_views == 1 (one view draws what it always drew), else
    (min(n_boot, steps), n_views, P-1))."""
    device = torch.device(device)
    h, w = size
    bh, bw = size if bg_size is None else bg_size
    n_views = int(n_views)
    colours = bg_lat = None
    if n_boot:
        gd = torch.Generator(device).manual_seed(int(seed))
        colours = torch.rand(n_boot, 3, generator=gd, device=device)
        moments = []
        for c0 in range(0, n_boot, chunk):
            img = colours[c0:c0 + chunk, :, None, None].repeat(1, 1, bh, bw)
            moments.append(encoder.encode_moments(2 * img - 1))
        mean = torch.cat([m for m, _ in moments]).to(device, F32)
        std = torch.exp(0.5 * torch.cat([lv for _, lv in moments]).to(device, F32))
        rows = []
        for b in range(n_boot):                                      # DiagonalGaussianDistribution.sample, in order
            e = torch.randn(mean[b:b + 1].shape, generator=gd, device=device, dtype=F32)
            rows.append((mean[b:b + 1] + std[b:b + 1] * e) * LATENT_SCALE)
        bg_lat = torch.cat(rows)
    g = torch.Generator().manual_seed(int(seed))
    start = torch.randn((1, in_channels, h // 8, w // 8), generator=g, dtype=F32)
    n_pick = min(n_boot, steps) if n_boot and steps else 0
    picks = torch.stack([torch.randint(0, n_boot, (n_prompts - 1,), generator=g) for _ in range(n_pick * n_views)]) \
        if n_pick and n_views else torch.zeros((0, n_prompts - 1), dtype=torch.int64)
    if n_views != 1:                                                      # step-major, view-minor: lines 210-223
        picks = picks.reshape(n_pick, n_views, n_prompts - 1)
    return dict(colours=colours, bg_latents=bg_lat, start_latent=start, picks=picks)


def to_uint8_truncating(images):
    """T.ToPILImage of a float image in [0, 1] (generation/multidiffusion.py:280): mul(255).byte() truncates, where
    the other plugins' sampler.decode rounds.  images [B,3,H,W] -> uint8 [B,H,W,3] (CPU numpy)."""
    return images.detach().float().mul(255).byte().permute(0, 2, 3, 1).cpu().numpy()


def decode_truncating(vae, latent):
    """decode_latents + ToPILImage (generation/multidiffusion.py:160-165,279-280) -> uint8 [B,H,W,3]."""
    imgs = vae.decode(latent / LATENT_SCALE)
    return to_uint8_truncating((imgs / 2 + 0.5).clamp(0, 1))


# ---- the loop ---------------------------------------------------------------------------------------------------------
class _MDState(LoopState):
    """Persistent buffers of one (prompts, padded rows, latent shape, steps, bootstrapping): fixed addresses for the
    captured graph, allocated with torch and not in the engine's activation arena (plans alias each other there)."""

    def __init__(self, dev, P, Pp, C, L, T, n_boot):
        super().__init__(torch.zeros((C, L, L), device=dev, dtype=F32), T)
        self.noise = torch.zeros((C, L, L), device=dev, dtype=F32)
        self.masks = torch.zeros((Pp, L * L), device=dev, dtype=F32)
        self.bg = torch.zeros((max(n_boot, 1), C, L, L), device=dev, dtype=F32)
        self.picks = torch.zeros((T, max(P - 1, 1)), device=dev, dtype=torch.int32)
        self.ctab = torch.zeros((T, 4), device=dev, dtype=F32)
        self.hist = torch.zeros((T + 1, C, L, L), device=dev, dtype=F32)


class _MDViewsState(LoopState):
    """_MDState for a panorama seen through V views: the panorama-sized latent, frozen noise, masks and the value / count
    accumulators of lgd_multidiffusion_views_f32, view-sized backgrounds, and one pick per step, view and foreground
    prompt."""

    def __init__(self, dev, P, C, Hp, Wp, V, T, n_boot):
        super().__init__(torch.zeros((C, Hp, Wp), device=dev, dtype=F32), T)
        self.noise = torch.zeros((C, Hp, Wp), device=dev, dtype=F32)
        self.value = torch.zeros((C, Hp, Wp), device=dev, dtype=F32)
        self.count = torch.zeros((C, Hp, Wp), device=dev, dtype=F32)
        self.masks = torch.zeros((P, Hp * Wp), device=dev, dtype=F32)
        self.bg = torch.zeros((max(n_boot, 1), C, WINDOW, WINDOW), device=dev, dtype=F32)
        self.picks = torch.zeros((T, V, max(P - 1, 1)), device=dev, dtype=torch.int32)
        self.ctab = torch.zeros((T, 4), device=dev, dtype=F32)
        self.hist = torch.zeros((T + 1, C, Hp, Wp), device=dev, dtype=F32)


def _ddim_of(sampler):
    """The DDIM scheduler of the checkpoint (models/models.py:49; generation/multidiffusion.py:86)."""
    s = sampler.scheduler
    if type(s) is DDIMScheduler:
        return s
    c = s.config
    return DDIMScheduler(c.num_train_timesteps, c.beta_start, c.beta_end, c.steps_offset, c.prediction_type)


def padded_rows(sampler, P):
    """UNet rows per CFG half: P padded up to the sampler's buckets (inert rows: mask 0, text row 0)."""
    cap = sampler.eng.max_text_batch // 2
    for b in sorted(sampler.BUCKETS):
        if P <= b <= cap:
            return b
    if P <= cap:
        return P
    raise RuntimeError(f"{P} prompts need a UNet batch of {2 * P}; the engine's text buffers hold {2 * cap}")


@torch.no_grad()
def multidiffusion_generate(sampler, texts, masks, start_latent, bg_latents, picks, steps=50, guidance_scale=10.0,
                            n_boot=20, decode=True, save_all_latents=False, first_step=0, n_steps=None, noise=None,
                            record_inputs=False, indep_uncond=True, normalization=False, views_per_call=None):
    """MultiDiffusion.generate (generation/multidiffusion.py:167-282); with the defaults, as run() calls it.

    texts: (2P, 77, Cx) = [uncond_0 .. uncond_{P-1}; cond_0 .. cond_{P-1}];  masks: (P, 1, L, L) or (P, L, L), row 0 the
    background;  start_latent: (1, C, L, L);  bg_latents: (n_boot, C, L, L) encoded backgrounds;  picks: int
    (>= min(n_boot, steps), P-1), the background of each step and foreground prompt.  Both are taken explicitly so that
    tests can teacher-force them (draw_randomness makes the reference's).
    first_step / n_steps: run only those steps, from `start_latent` as the state before step first_step; the frozen
    bootstrapping noise is then `noise` (by default the start latent, as in the reference).
    Returns dict(latent (1,C,L,L), image uint8 (H,W,3) truncated like ToPILImage or None, latents_all (T+1,1,C,L,L)
    with save_all_latents (rows first_step .. the last step run are this call's, every other row zero: loop.history_of),
    inputs: per step run the (P,C,L,L) UNet input rows with record_inputs).

    A start latent (1, C, Hp, Wp) other than 64 x 64 (with masks (P, 1, Hp, Wp)), indep_uncond=False (prompt 0's
    unconditional prediction for every prompt of a view) or normalization=True (value / count over the overlaps) take
    the path over the V = len(get_views(8 Hp, 8 Wp)) views: see _generate_views.  bg_latents stay (n_boot, C, 64, 64),
    picks become (>= min(n_boot, steps), V, P-1), `inputs` per step (V, P, C, 64, 64), and views_per_call caps the views
    per UNet call below what the engine's text buffers hold."""
    eng, dev = sampler.eng, sampler.dev
    P = int(masks.shape[0])
    n_boot = int(n_boot)
    if tuple(start_latent.shape[2:]) != (WINDOW, WINDOW) or not indep_uncond or normalization:
        return _generate_views(sampler, texts, masks, start_latent, bg_latents, picks, steps, guidance_scale, n_boot,
                               decode, save_all_latents, first_step, n_steps, noise, record_inputs, bool(indep_uncond),
                               bool(normalization), views_per_call)
    _, C, L, _ = start_latent.shape
    if tuple(texts.shape[:1]) != (2 * P,):
        raise ValueError(f"texts {tuple(texts.shape)} for {P} prompts: want (2P, 77, Cx) = [uncond; cond]")
    if n_boot < 0:
        raise ValueError("bootstrapping must be >= 0")
    sch = _ddim_of(sampler)
    sch.set_timesteps(int(steps))
    ts = sch.timesteps
    T = len(ts)
    n_pick = min(n_boot, T)
    boot = n_boot > 0 and P > 1
    if boot:
        picks = torch.as_tensor(picks).reshape(-1, P - 1)
        if picks.shape[0] < n_pick or bg_latents is None or bg_latents.shape[0] != n_boot:
            raise ValueError("bootstrapping needs bg_latents (n_boot, C, L, L) and picks (min(n_boot, steps), P-1)")
        if n_pick and (int(picks[:n_pick].min()) < 0 or int(picks[:n_pick].max()) >= n_boot):
            raise ValueError("picks index the n_boot backgrounds")
    Pp = padded_rows(sampler, P)

    st = sampler.md_states.get((P, Pp, C, L, T, n_boot), lambda: _MDState(dev, P, Pp, C, L, T, n_boot))

    # ---- per-run constants (before graph capture so that the capture's warm-up launch sees valid inputs)
    st.ctab.copy_(sch.coef_table(guidance_scale, dev, timesteps=ts))
    unc, cond = texts[:P].to(dev, F32), texts[P:].to(dev, F32)
    pad = lambda t: torch.cat([t, t[:1].expand(Pp - P, *t.shape[1:])]) if Pp > P else t
    eng.prepare_timesteps([int(t) for t in ts])
    eng.prepare_text(torch.cat([pad(unc), pad(cond)]))
    eng.set_step(0)
    plan = eng.plan(2 * Pp, L)
    st.picks.zero_()

    def step_fn():
        plan.forward()
        ops.multidiffusion_step(plan.eps_out, plan.latents_in, st.lat, st.masks, st.ctab, eng.dyn, n_prompts=P,
                                n_steps=T, bg=st.bg, noise=st.noise, picks=st.picks, n_boot=n_boot, hist=st.hist)
    runner = st.runner("step", step_fn, sampler.use_graphs)

    # ---- state of this call
    st.masks.zero_()
    st.masks[:P].copy_(masks.reshape(P, L * L).to(dev, F32))
    st.lat.copy_(start_latent.reshape(C, L, L).to(dev, F32))
    st.noise.copy_((start_latent if noise is None else noise).reshape(C, L, L).to(dev, F32))
    if boot:
        st.bg.copy_(bg_latents.to(dev, F32))
        if n_pick:
            st.picks[:n_pick].copy_(picks[:n_pick].to(dev, torch.int32))
    first_step, last_step = clamp_steps(first_step, n_steps, T)
    st.hist[first_step].copy_(st.lat)
    inputs = []
    if first_step < T:
        eng.set_step(first_step)
        ops.multidiffusion_step(None, plan.latents_in, st.lat, st.masks, st.ctab, eng.dyn, n_prompts=P, n_steps=T,
                                bg=st.bg, noise=st.noise, picks=st.picks, n_boot=n_boot, prep=True)

    def one_step(index):
        if record_inputs:
            inputs.append(plan.latents_in[:P].clone())
        runner()
    run_steps(eng, first_step, last_step, one_step)
    lat = st.lat.reshape(1, C, L, L).clone()
    image = decode_truncating(sampler.vae, lat)[0] if decode else None
    return dict(latent=lat, image=image, inputs=inputs,
                latents_all=history_of(st.hist, T + 1, first_step, last_step).unsqueeze(1) if save_all_latents else None)


@torch.no_grad()
def _generate_views(sampler, texts, masks, start_latent, bg_latents, picks, steps, guidance_scale, n_boot, decode,
                    save_all_latents, first_step, n_steps, noise, record_inputs, indep_uncond, normalization,
                    views_per_call):
    """The loop of generation/multidiffusion.py:210-280 over the V views of a panorama.  The engine's text buffers hold
    max_text_batch rows, so the views go through the UNet in chunks of max_text_batch // (2 Pp) whole views; the text
    rows are repeated per view of a chunk.  Per chunk: lgd_multidiffusion_views_f32 (prep) writes the chunk's input
    rows, the plan runs, lgd_multidiffusion_views_f32 adds the chunk's share to value / count, and behind the last
    chunk writes the blended latent.  All chunks use one plan: a last, shorter chunk leaves the rows behind its views
    as they are (finite: an earlier chunk's), the UNet computes them and nobody reads the result.  One step, all its
    chunks, is one captured hipGraph."""
    eng, dev = sampler.eng, sampler.dev
    P = int(masks.shape[0])
    _, C, Hp, Wp = start_latent.shape
    if Hp < WINDOW or Wp < WINDOW or Wp % 4:
        raise ValueError(f"panorama latent {Hp} x {Wp}: want at least {WINDOW} x {WINDOW} and a width divisible by 4")
    if tuple(texts.shape[:1]) != (2 * P,):
        raise ValueError(f"texts {tuple(texts.shape)} for {P} prompts: want (2P, 77, Cx) = [uncond; cond]")
    if int(masks.numel()) != P * Hp * Wp:
        raise ValueError(f"masks {tuple(masks.shape)} for a {Hp} x {Wp} latent: want (P, 1, Hp, Wp)")
    if n_boot < 0:
        raise ValueError("bootstrapping must be >= 0")
    views = get_views(8 * Hp, 8 * Wp)
    V = len(views)                                           # >= 1: the latent holds at least one window
    sch = _ddim_of(sampler)
    sch.set_timesteps(int(steps))
    ts = sch.timesteps
    T = len(ts)
    n_pick = min(n_boot, T)
    boot = n_boot > 0 and P > 1
    if boot:
        picks = torch.as_tensor(picks)
        if picks.numel() < n_pick * V * (P - 1) or bg_latents is None or \
                tuple(bg_latents.shape) != (n_boot, C, WINDOW, WINDOW):
            raise ValueError(f"bootstrapping needs bg_latents (n_boot, C, {WINDOW}, {WINDOW}) and picks "
                             "(min(n_boot, steps), V, P-1)")
        picks = picks.reshape(-1, V, P - 1)
        if n_pick and (int(picks[:n_pick].min()) < 0 or int(picks[:n_pick].max()) >= n_boot):
            raise ValueError("picks index the n_boot backgrounds")
    Pp = padded_rows(sampler, P)
    nvc = min(V, eng.max_text_batch // (2 * Pp))
    if views_per_call is not None:
        nvc = min(nvc, int(views_per_call))
    if nvc < 1:
        raise ValueError("views_per_call must be >= 1")

    st = sampler.md_states.get(("views", P, Pp, C, Hp, Wp, T, n_boot, indep_uncond, normalization, nvc),
                               lambda: _MDViewsState(dev, P, C, Hp, Wp, V, T, n_boot))

    # ---- per-run constants (before graph capture so that the capture's warm-up launch sees valid inputs)
    st.ctab.copy_(sch.coef_table(guidance_scale, dev, timesteps=ts))
    unc, cond = texts[:P].to(dev, F32), texts[P:].to(dev, F32)
    pad = lambda t: torch.cat([t, t[:1].expand(Pp - P, *t.shape[1:])]) if Pp > P else t
    eng.prepare_timesteps([int(t) for t in ts])
    eng.prepare_text(torch.cat([pad(unc).repeat(nvc, 1, 1), pad(cond).repeat(nvc, 1, 1)]))
    eng.set_step(0)
    plan = eng.plan(2 * Pp * nvc, WINDOW)
    st.picks.zero_()
    kw = dict(n_prompts=P, rows_per_view=Pp, n_views=V, n_steps=T, indep_uncond=indep_uncond,
              normalization=normalization, bg=st.bg, noise=st.noise, picks=st.picks, n_boot=n_boot)
    chunks = [(v0, min(nvc, V - v0)) for v0 in range(0, V, nvc)]

    def prep(v0, nv):
        ops.multidiffusion_views(None, plan.latents_in, st.lat, st.value, st.count, st.masks, st.ctab, eng.dyn, v0=v0,
                                 nv=nv, prep=True, **kw)

    def step_fn():
        for v0, nv in chunks:
            prep(v0, nv)
            plan.forward()
            ops.multidiffusion_views(plan.eps_out, plan.latents_in, st.lat, st.value, st.count, st.masks, st.ctab,
                                     eng.dyn, v0=v0, nv=nv, hist=st.hist, **kw)
    plan.latents_in.zero_()                                  # rows behind a short last chunk: finite from the start
    runner = st.runner("step", step_fn, sampler.use_graphs)

    # ---- state of this call
    st.masks.copy_(masks.reshape(P, Hp * Wp).to(dev, F32))
    st.lat.copy_(start_latent.reshape(C, Hp, Wp).to(dev, F32))
    st.noise.copy_((start_latent if noise is None else noise).reshape(C, Hp, Wp).to(dev, F32))
    if boot:
        st.bg.copy_(bg_latents.to(dev, F32))
        if n_pick:
            st.picks[:n_pick].copy_(picks[:n_pick].to(dev, torch.int32))
    first_step, last_step = clamp_steps(first_step, n_steps, T)
    st.hist[first_step].copy_(st.lat)
    inputs = []

    def one_step(index):
        if record_inputs:                                    # the rows the step's own prep launches write again
            rows = []
            for v0, nv in chunks:
                prep(v0, nv)
                rows.append(plan.latents_in[:nv * Pp].reshape(nv, Pp, C, WINDOW, WINDOW)[:, :P].clone())
            inputs.append(torch.cat(rows))
        runner()
    run_steps(eng, first_step, last_step, one_step)
    lat = st.lat.reshape(1, C, Hp, Wp).clone()
    image = decode_truncating(sampler.vae, lat)[0] if decode else None
    return dict(latent=lat, image=image, inputs=inputs, views=views,
                latents_all=history_of(st.hist, T + 1, first_step, last_step).unsqueeze(1) if save_all_latents else None)


@torch.no_grad()
def encode_texts(tokenizer, text_encoder, prompts, negative_prompts, device="cuda"):
    """MultiDiffusion.get_text_embeds (generation/multidiffusion.py:126-150): the prompts are truncated to the
    tokenizer's length, the negative prompts are padded to it but not truncated -> (2P, 77, Cx) [uncond; cond]."""
    text_input = tokenizer(list(prompts), padding="max_length", max_length=tokenizer.model_max_length, truncation=True,
                           return_tensors="pt")
    cond = text_encoder(text_input.input_ids.to(device))[0]
    uncond_input = tokenizer(list(negative_prompts), padding="max_length", max_length=tokenizer.model_max_length,
                             return_tensors="pt")
    uncond = text_encoder(uncond_input.input_ids.to(device))[0]
    return torch.cat([uncond, cond]).float()

"""Mask refinement with SAM: the host rules of the reference's models/sam.py around the network
of lgd_amd.sam.HipSamModel.

Same functions and argument meaning as the reference module (models/sam.py:13-213, re-exported under that name by
dropin/models/sam.py); the model object in `sam_model_dict["sam_model"]` is the HIP implementation, the processor object
stays the Hugging Face `SamProcessor` (host-side image resizing / normalisation and mask post-processing).

  sam()               :25-55   processor -> model -> post_process_masks -> bilinear resize to the latent grid
  select_mask()       :67-111  "largest_over_conf": the largest of the three masks, candidates with low predicted IoU
                               or low IoU with the coarse mask pushed behind every admissible one
  sam_refine_boxes()  :182-213 LMD+: the layout box is the prompt and the coarse mask
  sam_refine_attn()   :125-172 LMD: the smoothed, thresholded cross-attention map gives a box (or its arg-max a point)

Reference quirks kept on purpose: `sam()` returns the predicted IoUs of image 0 / prompt 0 only (:45), and
`sam_refine_boxes` scores every box of every image with them (the plugins call it with one image and one box);
`sam_refine_attn(use_box_input=True)` hands the processor a two-level box list (:141-144), which transformers refuses
("Input boxes must be a list of list of list of floating points") — the plugins' default is the point prompt.
`SamRefiner(use_box_input=True, attn_box="device").attns` builds that box on the device and hands the model a proper
(N, 1, 4) tensor.
"""
import numpy as np
import torch
import torch.nn.functional as F
from scipy import ndimage

from . import hostprep
from .sam import HipSamModel, SamConfig


class _Encoding(dict):
    """What the processor returns, as far as models/sam.py:39 uses it: a mapping with `.to(device)`."""

    def to(self, *_a, **_k):
        return self


class DeviceSamProcessor:
    """The Hugging Face `SamProcessor` + `SamImageProcessor` defaults on the model's device, for generation loops where
    the host-side PIL path (resize of every decoded single-object image on the CPU) would stall the GPU: longest edge ->
    1024 (bilinear), 1/255, ImageNet mean / std, zero padding bottom / right; prompts scaled by new/old size ([ext]
    processing_sam.py `_normalize_coordinates`); `post_process_masks` = interpolate to the padded size, crop,
    interpolate to the original size, threshold ([ext] image_processing_sam.py).

    resize="torch" (the default: existing results and goldens stay as they are) approximates Pillow's resize with
    `F.interpolate` (half-pixel centres, antialias when shrinking) rounded to the 8-bit grid, then divides, subtracts,
    divides and pads in separate torch launches.  That is NOT Pillow's arithmetic — Pillow resamples in two passes with
    22-bit integer weights and an 8-bit image between them — and the share of SAM input pixels that come out one full
    8-bit level away from `SamImageProcessor`'s (transformers 5.15, Pillow backend), measured on the CPU, is
        512 x 512 -> 1024 x 1024, random image                        26.5 %
        512 x 512 -> 1024 x 1024, first image of tests/sam_cases      27.3 %
        1200 x 900                                                    13.7 %
        512 x 2048                                                     4.1 %
    resize="pillow" is the exact path: one `ops.resample_u8` call per batch of equal-sized images (csrc/resample.hip:
    Pillow's BILINEAR bit for bit, (v * fp32(1/255) - mean) / std and the zero padding written by the last resize pass
    itself), within 1e-6 absolute of `SamImageProcessor`'s pixel_values.  It needs the HIP library and a GPU."""
    MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    RESIZES = ("torch", "pillow")

    def __init__(self, device="cuda", longest_edge=1024, resize="torch"):
        if resize not in self.RESIZES:
            raise ValueError(f"DeviceSamProcessor: resize {resize!r} is none of {self.RESIZES}")
        self.dev, self.target, self.resize = torch.device(device), int(longest_edge), resize
        if resize == "pillow" and self.dev.type != "cuda":
            raise RuntimeError(f"DeviceSamProcessor(resize='pillow') runs the HIP resampler (ops.resample_u8) and needs a "
                               f"GPU, not device {self.dev}: there is no torch fallback for it (resize='torch' is the "
                               "other processor, with other results)")
        self.image_processor = self
        self.on_device = True
        self._mean = torch.tensor(self.MEAN, device=self.dev).view(1, 3, 1, 1)
        self._std = torch.tensor(self.STD, device=self.dev).view(1, 3, 1, 1)

    def _shape(self, h, w):
        scale = self.target / max(h, w)
        return int(h * scale + 0.5), int(w * scale + 0.5)

    def _resize(self, t):
        """uint8 (n, h, w, 3) on the device -> normalised, padded fp32 (n, 3, target, target) and the resized size."""
        h, w = int(t.shape[1]), int(t.shape[2])
        nh, nw = self._shape(h, w)
        if self.resize == "pillow":
            from . import ops
            px = ops.resample_u8(t.contiguous(), (nh, nw), "bilinear", "affine", rescale=1.0 / 255.0, mean=self.MEAN,
                                 std=self.STD, canvas=(self.target, self.target), pad=0.0)
            return px, (nh, nw)
        r = F.interpolate(t.permute(0, 3, 1, 2).float(), (nh, nw), mode="bilinear", align_corners=False,
                          antialias=(nh < h or nw < w)).round().clamp(0, 255)
        r = (r / 255.0 - self._mean) / self._std
        return F.pad(r, (0, self.target - nw, 0, self.target - nh)), (nh, nw)

    def pixels(self, images):
        """One HxWx3 image, a list of them, a stacked (N, h, w, 3) array or a uint8 tensor (N, h, w, 3), on the host or
        already on the device -> (pixel_values (N, 3, target, target), [[h, w]] * N, [[nh, nw]] * N).  Images of one size
        are resized in one call; the result per image does not depend on what it shares the call with."""
        if torch.is_tensor(images):
            batch = images[None] if images.dim() == 3 else images
        elif isinstance(images, np.ndarray):
            batch = torch.as_tensor(np.ascontiguousarray(images[None] if images.ndim == 3 else images))
        else:
            imgs = [im if torch.is_tensor(im) else torch.as_tensor(np.ascontiguousarray(im)) for im in images]
            if len({tuple(im.shape) for im in imgs}) != 1:        # mixed sizes (or none): one call per image
                if not imgs:
                    raise ValueError("images must be HxWx3 arrays")
                parts = [self.pixels(im) for im in imgs]
                return torch.cat([p[0] for p in parts]), [p[1][0] for p in parts], [p[2][0] for p in parts]
            batch = torch.stack(imgs) if imgs[0].dim() == 3 else None
        if batch is None or batch.dim() != 4 or batch.shape[3] != 3:
            raise ValueError("images must be HxWx3 arrays")
        px, (nh, nw) = self._resize(batch.to(self.dev))
        n, h, w = int(batch.shape[0]), int(batch.shape[1]), int(batch.shape[2])
        return px, [[h, w]] * n, [[nh, nw]] * n

    def __call__(self, images, input_points=None, input_labels=None, input_boxes=None, return_tensors="pt", **_kw):
        pixel_values, orig, resh = self.pixels(images)
        enc = _Encoding(pixel_values=pixel_values, original_sizes=torch.tensor(orig), reshaped_input_sizes=torch.tensor(resh))

        def scaled(prompts, box):
            if len(prompts) != len(orig):
                sizes = [(orig[0], resh[0])] * len(prompts)
            else:
                sizes = list(zip(orig, resh))
            out = []
            for p, ((h, w), (nh, nw)) in zip(prompts, sizes):
                a = np.array(p, dtype=np.float64)
                a = a.reshape(-1, 2, 2) if box else a
                a[..., 0] *= nw / w
                a[..., 1] *= nh / h
                out.append(a.reshape(-1, 4) if box else a)
            return torch.from_numpy(np.array(out))
        if input_boxes is not None:
            if not (isinstance(input_boxes, list) and isinstance(input_boxes[0], list) and isinstance(input_boxes[0][0], list)):
                raise ValueError("Input boxes must be a list of list of list of floating points.")
            b = scaled(input_boxes, True)
            enc["input_boxes"] = b.unsqueeze(1) if b.dim() != 3 else b
        if input_points is not None:
            if not (isinstance(input_points, list) and isinstance(input_points[0], list)):
                raise ValueError("Input points must be a list of list of list of floating points.")
            pts = scaled(input_points, False)
            enc["input_points"] = pts.unsqueeze(1) if pts.dim() != 4 else pts
        if input_labels is not None:
            lab = torch.as_tensor(np.array(input_labels))
            enc["input_labels"] = lab.unsqueeze(1) if lab.dim() != 3 else lab
        return enc

    def post_process_masks(self, masks, original_sizes, reshaped_input_sizes, mask_threshold=0.0, binarize=True):
        out = []
        for i, (h, w) in enumerate(torch.as_tensor(original_sizes).tolist()):
            nh, nw = torch.as_tensor(reshaped_input_sizes).tolist()[i]
            m = F.interpolate(masks[i].float(), (self.target, self.target), mode="bilinear", align_corners=False)
            m = F.interpolate(m[..., :nh, :nw], (h, w), mode="bilinear", align_corners=False)
            out.append(m > mask_threshold if binarize else m)
        return out


def wrap_sam(hf_sam_model, sam_processor=None, device="cuda"):
    """A loaded Hugging Face `SamModel` (weights) -> the `sam_model_dict` of the reference with the HIP model in it."""
    if sam_processor is None:
        import transformers
        sam_processor = transformers.SamProcessor(transformers.SamImageProcessor())
    elif sam_processor == "device":
        sam_processor = DeviceSamProcessor(device)
    elif sam_processor == "device-pillow":                        # Pillow-exact resize (DeviceSamProcessor's docstring)
        sam_processor = DeviceSamProcessor(device, resize="pillow")
    model = HipSamModel(SamConfig.from_hf(hf_sam_model.config), hf_sam_model.state_dict(), device=device)
    return dict(sam_model=model, sam_processor=sam_processor)


def load_sam(checkpoint="facebook/sam-vit-base", device="cuda"):
    """models/sam.py:13-21."""
    from transformers import SamModel, SamProcessor
    return wrap_sam(SamModel.from_pretrained(checkpoint), SamProcessor.from_pretrained(checkpoint), device)


def _listify(boxes):
    """Tuples anywhere in the nested box list -> lists (the processor only takes lists; :29-35)."""
    if isinstance(boxes, (tuple, list)):
        return [_listify(b) for b in boxes]
    return boxes


def sam(sam_model_dict, image, input_points=None, input_boxes=None, target_mask_shape=None, return_numpy=True):
    """-> (per image: bool masks [n_prompts, 3, h, w] at `target_mask_shape`, predicted IoUs of image 0 / prompt 0 [3])."""
    model, processor = sam_model_dict["sam_model"], sam_model_dict["sam_processor"]
    if input_boxes:
        input_boxes = _listify(input_boxes)
    enc = processor(image, input_points=input_points, input_boxes=input_boxes, return_tensors="pt")
    out = model(**enc)
    logits = out.pred_masks.float()
    if not getattr(processor, "on_device", False):                 # the Hugging Face processor works on host tensors
        logits = logits.cpu()
    full = processor.image_processor.post_process_masks(logits, enc["original_sizes"].cpu(), enc["reshaped_input_sizes"].cpu())
    conf_scores = out.iou_scores.float().cpu().numpy()[0, 0]
    small = [F.interpolate(m.float(), target_mask_shape, mode="bilinear").bool().cpu() for m in full]
    return ([m.numpy() for m in small] if return_numpy else small), conf_scores


def sam_point_input(sam_model_dict, image, input_points, **kwargs):
    return sam(sam_model_dict, image, input_points=input_points, **kwargs)


def sam_box_input(sam_model_dict, image, input_boxes, **kwargs):
    return sam(sam_model_dict, image, input_boxes=input_boxes, **kwargs)


def get_iou_with_resize(mask, masks, masks_shape):
    """IoU of `mask` with each candidate after bringing the candidates to `masks_shape` (:63-65: cv2.resize of the 0/255
    image, INTER_LINEAR, non-zero = inside; the plugins pass candidates that already have that shape)."""
    h, w = masks_shape
    cand = np.asarray(masks).astype(bool)
    if cand.shape[1:] != (h, w):
        t = torch.from_numpy(cand.astype(np.float32))[:, None]
        cand = (F.interpolate(t, (h, w), mode="bilinear", align_corners=False)[:, 0] > 0).numpy()
    return hostprep.iou(np.asarray(mask), cand)


def select_mask(masks, conf_scores, coarse_ious=None, rule="largest_over_conf", discourage_mask_below_confidence=0.85,
                discourage_mask_below_coarse_iou=0.2, verbose=False):
    if rule != "largest_over_conf":
        raise ValueError(f"Unknown rule: {rule}")
    area = masks.sum(axis=(1, 2))
    penalty = area.max()
    score = area - penalty * (conf_scores < discourage_mask_below_confidence)
    if coarse_ious is not None:
        score = score - penalty * (coarse_ious < discourage_mask_below_coarse_iou)
    best = int(np.argmax(score))
    if verbose:
        print(f"mask_sizes: {area}, scores: {score}")
        print(f"Selected a mask with confidence: {conf_scores[best]}, "
              f"coarse_iou: {None if coarse_ious is None else coarse_ious[best]}")
    return masks[best], conf_scores[best]


def preprocess_mask(token_attn_np_smooth, mask_th, n_erode_dilate_mask=0):
    """Min-max normalise, threshold, optionally open (erode then dilate) the binary map (:113-122)."""
    a = token_attn_np_smooth - token_attn_np_smooth.min()
    binary = a / a.max() > mask_th
    if n_erode_dilate_mask:
        binary = ndimage.binary_dilation(ndimage.binary_erosion(binary, iterations=n_erode_dilate_mask),
                                         iterations=n_erode_dilate_mask)
    return binary


def _pick(three_masks, conf_scores, coarse, below_conf, below_iou):
    ious = get_iou_with_resize(coarse, three_masks, masks_shape=coarse.shape)
    return select_mask(three_masks, conf_scores, coarse_ious=ious, rule="largest_over_conf",
                       discourage_mask_below_confidence=below_conf, discourage_mask_below_coarse_iou=below_iou, verbose=True)


def sam_refine_attn(sam_input_image, token_attn_np, model_dict, height, width, H, W, use_box_input, gaussian_sigma,
                    mask_th_for_box, n_erode_dilate_mask_for_box, mask_th_for_point, discourage_mask_below_confidence,
                    discourage_mask_below_coarse_iou, verbose):
    smooth = ndimage.gaussian_filter(token_attn_np.astype(float), sigma=gaussian_sigma)
    up_w, up_h = height // smooth.shape[1], width // smooth.shape[0]       # (w, h) order of the reference (:135)
    if use_box_input:
        coarse = preprocess_mask(smooth, mask_th_for_box, n_erode_dilate_mask=n_erode_dilate_mask_for_box)
        box = hostprep.binary_mask_to_box(coarse, w_scale=up_w, h_scale=up_h)
        masks, conf = sam_box_input(model_dict, image=sam_input_image, input_boxes=[box], target_mask_shape=(H, W))
    else:
        coarse = preprocess_mask(smooth, mask_th_for_point, n_erode_dilate_mask=0)
        peak_y, peak_x = np.unravel_index(smooth.argmax(), smooth.shape)
        masks, conf = sam_point_input(model_dict, image=sam_input_image, input_points=[[[peak_x * up_h, peak_y * up_w]]],
                                      target_mask_shape=(H, W))
    return _pick(masks[0][0], conf, coarse, discourage_mask_below_confidence, discourage_mask_below_coarse_iou)


def sam_refine_boxes(sam_input_images, boxes, model_dict, height, width, H, W, discourage_mask_below_confidence,
                     discourage_mask_below_coarse_iou, verbose):
    pixel_boxes = [[hostprep.scale_proportion(b, H=height, W=width) for b in per_image] for per_image in boxes]
    masks, conf = sam_box_input(model_dict, image=sam_input_images, input_boxes=pixel_boxes, target_mask_shape=(H, W))
    picked = [[_pick(three, conf, hostprep.proportion_to_mask(b, H, W, return_np=True), discourage_mask_below_confidence,
                     discourage_mask_below_coarse_iou) for b, three in zip(per_image, per_image_masks)]
              for per_image, per_image_masks in zip(boxes, masks)]
    return [[m for m, _ in row] for row in picked], [[c for _, c in row] for row in picked]


def sam_refine_box(sam_input_image, box, *args, **kwargs):
    masks, confs = sam_refine_boxes([sam_input_image], [[box]], *args, **kwargs)
    return masks[0][0], confs[0][0]


def _upload(t, dev):
    """Host tensor -> device without stalling the stream (pinned staging, asynchronous copy); device tensors pass."""
    if t.device == dev or dev.type != "cuda" or t.is_cuda:
        return t.to(dev)
    return t.pin_memory().to(dev, non_blocking=True)


class SamRefiner:
    """What the generation pipelines (lgd_amd.pipeline) call per generated single-object image: the arguments the
    reference's plugins put into `sam_refine_kwargs` (generation/lmd_plus.py:320-327, generation/lmd.py:354-366), bound
    once.

    `box` / `attn` refine one image, with host work between the processor, the model and the selection.  `boxes` /
    `attns` refine a batch in one pass that stays on the device: processor -> HipSamModel in chunks of at most
    MODEL_CHUNK images -> ops.sam_mask_tail (for `attns`, ops.sam_attn_prompt first).  They need the device processor.
    `batched` tells the pipelines which pair to call: None = on exactly when the processor is `DeviceSamProcessor`
    (measured faster there), False = the per-image path only.  `attns` covers the point prompt; with
    `use_box_input` the attention maps go through `attn` whatever `batched` says, unless `attn_box="device"` opts in to
    the box prompt made on the device (ops.sam_attn_box_prompt: smoothing, threshold, opening and bounding box in one
    launch), which `attns` then serves for the whole batch.  `attn_box="host"` (the default) keeps `attn`'s scipy
    opening; "device" needs the device processor.  Each item is scored with its own predicted IoUs."""
    MODEL_CHUNK = 8
    ATTN_BOXES = ("host", "device")

    def __init__(self, sam_model_dict, height=512, width=512, discourage_mask_below_confidence=0.85,
                 discourage_mask_below_coarse_iou=0.25, use_box_input=False, gaussian_sigma=None, mask_th_for_box=0.05,
                 n_erode_dilate_mask_for_box=1, mask_th_for_point=0.25, verbose=False, batched=None,
                 attn_box="host"):
        self.md, self.verbose = sam_model_dict, verbose
        on_device = bool(getattr(sam_model_dict["sam_processor"], "on_device", False))
        if batched and not on_device:
            raise ValueError("batched refinement needs the device processor (wrap_sam(..., sam_processor='device'))")
        if attn_box not in self.ATTN_BOXES:
            raise ValueError(f"SamRefiner: attn_box {attn_box!r} is none of {self.ATTN_BOXES}")
        if attn_box == "device" and not on_device:
            raise ValueError("attn_box='device' needs the device processor (wrap_sam(..., sam_processor='device'))")
        self.attn_box = attn_box
        self.batched = on_device if batched is None else bool(batched)
        self.common = dict(height=height, width=width, H=height // 8, W=width // 8,
                           discourage_mask_below_confidence=discourage_mask_below_confidence,
                           discourage_mask_below_coarse_iou=discourage_mask_below_coarse_iou)
        if gaussian_sigma is None:                               # generation/lmd.py:39-40,336-338
            gaussian_sigma = 0.1 if use_box_input else 1.5
        self.attn_kw = dict(use_box_input=use_box_input, gaussian_sigma=gaussian_sigma, mask_th_for_box=mask_th_for_box,
                            n_erode_dilate_mask_for_box=n_erode_dilate_mask_for_box, mask_th_for_point=mask_th_for_point)

    def box(self, image, box):
        """LMD+ (generation/lmd_plus.py:122-128) -> (bool mask [H/8, W/8], confidence)."""
        return sam_refine_box(sam_input_image=image, box=box, model_dict=self.md, verbose=self.verbose, **self.common)

    def attn(self, image, token_attn_np):
        """LMD (generation/lmd.py:141-147) -> (bool mask [H/8, W/8], confidence)."""
        return sam_refine_attn(sam_input_image=image, token_attn_np=token_attn_np, model_dict=self.md,
                               verbose=self.verbose, **self.attn_kw, **self.common)

    # ---- a batch in one pass, on the device
    def _device_processor(self):
        processor = self.md["sam_processor"]
        if not getattr(processor, "on_device", False):
            raise RuntimeError("boxes() / attns() need the device processor; use box() / attn() with the Hugging Face one")
        return processor

    def _tail(self, images, coarse, **prompt):
        """processor -> model (chunks of MODEL_CHUNK) -> mask tail.  coarse: uint8 (N, hc, wc) on the device; prompt:
        `input_boxes=` (N, 1, 4) or `input_points=` (N, 1, 1, 2) in pixels of the ORIGINAL image, device or host."""
        from . import ops
        model, processor = self.md["sam_model"], self._device_processor()
        pixel_values, orig, resh = processor.pixels(images)
        N, dev = pixel_values.shape[0], pixel_values.device
        if coarse.shape[0] != N:
            raise ValueError(f"{N} images but {coarse.shape[0]} prompts")
        # one upload, in front of the model: the tail's geometry rows and the prompt scaling of processing_sam.py
        # `_normalize_coordinates` (x * new_w / old_w, y * new_h / old_h, in fp64)
        meta = _upload(torch.tensor([[h, w, nh, nw, nw / w, nh / h] for (h, w), (nh, nw) in zip(orig, resh)],
                                    dtype=torch.float64), dev)
        geom, ratio = meta[:, :4].to(torch.int32), meta[:, 4:]
        (name, p), = prompt.items()
        p = _upload(p, dev).to(torch.float64)
        p = (p.reshape(N, -1, 2) * ratio[:, None]).reshape(p.shape).float()
        logits, iou = [], []
        for c0 in range(0, N, self.MODEL_CHUNK):
            out = model(pixel_values=pixel_values[c0:c0 + self.MODEL_CHUNK], **{name: p[c0:c0 + self.MODEL_CHUNK]})
            logits.append(out.pred_masks[:, 0].float())
            iou.append(out.iou_scores[:, 0].float())
        logits = logits[0] if len(logits) == 1 else torch.cat(logits)
        iou = iou[0] if len(iou) == 1 else torch.cat(iou)
        mask, conf, _stats, _cand = ops.sam_mask_tail(
            logits.contiguous(), iou.contiguous(), geom, processor.target, (self.common["H"], self.common["W"]), coarse,
            self.common["discourage_mask_below_confidence"], self.common["discourage_mask_below_coarse_iou"])
        return mask.bool(), conf

    def boxes(self, images, boxes):
        """LMD+ for N (image, box) pairs: images uint8 (N, h, w, 3) (a device tensor, or anything the processor takes),
        boxes N (x0, y0, x1, y1) proportions -> (bool masks (N, H/8, W/8), confidences fp32 (N)), both on the device."""
        dev = self._device_processor().dev
        height, width, H, W = (self.common[k] for k in ("height", "width", "H", "W"))
        pixel = np.array([hostprep.scale_proportion(b, H=height, W=width) for b in boxes], dtype=np.float64)
        coarse = np.stack([hostprep.proportion_to_mask(b, H, W, return_np=True) for b in boxes]).astype(np.uint8)
        return self._tail(images, _upload(torch.from_numpy(coarse), dev), input_boxes=torch.from_numpy(pixel).reshape(-1, 1, 4))

    def attns(self, images, token_attns):
        """LMD for N (image, attention map) pairs: token_attns fp32 (N, hm, wm), a device tensor or a list of arrays ->
        (bool masks (N, H/8, W/8), confidences fp32 (N)), both on the device.  The point-prompt branch, and with
        `attn_box="device"` the box-prompt branch (`use_box_input`): the candidates are then scored against the OPENED
        mask, as `attn` scores them.

        The box branch reads the N `empty` flags of ops.sam_attn_box_prompt once, before the model runs: 4 N bytes, the
        only host read of the call.  The reference fails on an empty opened mask (`min()` of an empty sequence in
        utils.binary_mask_to_box, which generate.py logs before it skips the prompt); running SAM on the zero box and
        handing on its mask would silently differ from that, so `attns` raises ValueError naming the empty items."""
        from . import ops
        box = bool(self.attn_kw["use_box_input"])
        if box and self.attn_box != "device":
            raise NotImplementedError("attns() covers the point prompt; the box prompt of the attention map is attn()'s "
                                      "unless the refiner was built with attn_box='device'")
        dev = self._device_processor().dev
        if not torch.is_tensor(token_attns):
            token_attns = torch.from_numpy(np.stack([np.asarray(t, dtype=np.float32) for t in token_attns]))
        maps = _upload(token_attns, dev).to(torch.float32).contiguous()
        up_w, up_h = self.common["height"] // maps.shape[2], self.common["width"] // maps.shape[1]     # (w, h) as attn()
        if box:
            coarse, boxes, empty = ops.sam_attn_box_prompt(maps, self.attn_kw["gaussian_sigma"], self.attn_kw["mask_th_for_box"],
                                                           self.attn_kw["n_erode_dilate_mask_for_box"], up_w, up_h)
            gone = torch.nonzero(empty).flatten().tolist()         # the one host read: 4 N bytes
            if gone:
                raise ValueError(f"The mask is empty: the opened attention mask of item(s) {gone} of {maps.shape[0]} has no "
                                 "pixel, so there is no box to prompt SAM with")
            return self._tail(images, coarse, input_boxes=boxes.reshape(-1, 1, 4))
        coarse, points, _ = ops.sam_attn_prompt(maps, self.attn_kw["gaussian_sigma"], self.attn_kw["mask_th_for_point"],
                                                up_w, up_h)
        return self._tail(images, coarse, input_points=points.reshape(-1, 1, 1, 2))

"""[ext] transformers' CLIPImageProcessor on the device: what StableDiffusionPipeline's `feature_extractor` does to a
decoded image before the safety checker sees it.

With the checkpoints' configuration the processor is: Pillow BICUBIC resize of the SHORTEST edge to s (the long side to
int(s * long / short)), centre crop to s x s with top = (H - s) // 2 and left = (W - s) // 2, times rescale_factor, minus
mean, over std, channels first.  `DeviceClipProcessor` does that to a uint8 (N, h, w, 3) batch that is already on the GPU
through `ops.resample_u8` (csrc/resample.hip: Pillow's algorithm bit for bit, the affine step in fp32 folded into the last
pass):

  square input      ONE call: the resize lands on s x s and the crop is the whole image
  any other input   one "u8" resize to the processor's (H, W), a slice of the crop, then one same-size "affine" call (the
                    resampler applies the output form without resizing when neither axis changes)

It is built from the image processor or its configuration and refuses one it does not serve — it never approximates."""
import torch

from . import ops
from .owl_processor import _FILTER_NAMES, _get

_SIZE_KEYS = ("height", "width", "shortest_edge", "longest_edge", "max_height", "max_width")


def _size_fields(size):
    if size is None or isinstance(size, (int, tuple, list)):
        return size
    return {k: _get(size, k) for k in _SIZE_KEYS if _get(size, k) is not None}


class DeviceClipProcessor:
    def __init__(self, processor):
        """processor: a CLIPImageProcessor (a pipeline's `feature_extractor`) or its configuration as a dict."""
        self.processor = cfg = processor
        name = "DeviceClipProcessor"
        if not _get(cfg, "do_resize", True):
            raise ValueError(f"{name}: do_resize=False is not served (the checker takes one fixed input size)")
        if _get(cfg, "do_pad", False):
            raise ValueError(f"{name}: do_pad is not served")
        size = _size_fields(_get(cfg, "size"))
        if isinstance(size, int):
            size = {"shortest_edge": size}
        if not isinstance(size, dict) or set(size) != {"shortest_edge"}:
            raise ValueError(f"{name}: size {size!r} is not a shortest_edge (a fixed (height, width) is not served)")
        self.edge = s = int(size["shortest_edge"])
        if not _get(cfg, "do_center_crop", True):
            raise ValueError(f"{name}: do_center_crop=False is not served (only square inputs would fit the tower)")
        crop = _size_fields(_get(cfg, "crop_size"))
        if isinstance(crop, int):
            crop = {"height": crop, "width": crop}
        elif isinstance(crop, (tuple, list)) and len(crop) == 2:
            crop = {"height": crop[0], "width": crop[1]}
        if not isinstance(crop, dict) or set(crop) != {"height", "width"} or crop["height"] != crop["width"]:
            raise ValueError(f"{name}: crop_size {crop!r} is not a square (height, width)")
        if int(crop["height"]) != s:
            raise ValueError(f"{name}: crop_size {crop!r} differs from the shortest edge {s} (a crop that pads or cuts a "
                             "resized square is not served)")
        resample = _get(cfg, "resample")
        if resample is None or int(resample) not in _FILTER_NAMES:
            raise ValueError(f"{name}: resample {resample!r} is none of Pillow's BILINEAR (2), BICUBIC (3), LANCZOS (1)")
        self.filter = _FILTER_NAMES[int(resample)]
        self.rescale = float(_get(cfg, "rescale_factor", 1.0 / 255.0)) if _get(cfg, "do_rescale", True) else 1.0
        if _get(cfg, "do_normalize", True):
            mean, std = _get(cfg, "image_mean"), _get(cfg, "image_std")
            if mean is None or std is None or len(mean) != 3 or len(std) != 3:
                raise ValueError(f"{name}: image_mean and image_std hold one value per RGB channel")
            self.mean, self.std = tuple(float(v) for v in mean), tuple(float(v) for v in std)
        else:
            self.mean, self.std = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)

    def resized_size(self, h, w):
        """(H, W) of the resize: the shortest edge becomes s, the other one int(s * long / short)."""
        s = self.edge
        short, long_ = (h, w) if h <= w else (w, h)
        other = int(s * long_ / short)
        return (s, other) if h <= w else (other, s)

    def crop_box(self, H, W):
        """(top, left) of the s x s centre crop of a resized H x W image."""
        return (H - self.edge) // 2, (W - self.edge) // 2

    def pixel_values(self, images, dtype=torch.float32):
        """uint8 (N, h, w, 3) on the device -> `pixel_values` (N, 3, s, s)."""
        if images.dim() != 4 or images.shape[3] != 3:
            raise RuntimeError(f"DeviceClipProcessor: images is a (N, h, w, 3) batch, got shape {tuple(images.shape)}")
        s = self.edge
        kw = dict(dtype=dtype, rescale=self.rescale, mean=self.mean, std=self.std)
        H, W = self.resized_size(images.shape[1], images.shape[2])
        if (H, W) == (s, s):
            return ops.resample_u8(images, (s, s), self.filter, "affine", **kw)
        top, left = self.crop_box(H, W)
        resized = ops.resample_u8(images, (H, W), self.filter, "u8")
        return ops.resample_u8(resized[:, top:top + s, left:left + s].contiguous(), (s, s), self.filter, "affine", **kw)

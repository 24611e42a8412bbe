"""The image half of [ext] transformers' OwlViTProcessor on the device.

`OwlViTImageProcessor` with the checkpoints' configuration is: Pillow resize to size x size with the configured filter,
times rescale_factor, minus mean, over std, channels first.  `DeviceOwlProcessor` does that to a uint8 (N, h, w, 3) batch
that is already on the GPU in ONE call of `ops.resample_u8` (csrc/resample.hip: Pillow's algorithm bit for bit, the affine
step `(v * rescale_factor - mean) / std` in fp32 folded into the last pass), so a generated image reaches `detect()`
without a host copy.  It is built from the image processor's own configuration and refuses one it does not serve — it
never approximates.  Token ids still come from the processor's tokenizer (`input_ids`)."""
import torch

from . import ops

_FILTER_NAMES = {v: k for k, v in ops.FILTERS.items()}


def _get(cfg, name, default=None):
    return cfg.get(name, default) if isinstance(cfg, dict) else getattr(cfg, name, default)


class DeviceOwlProcessor:
    def __init__(self, processor):
        """processor: an OwlViTProcessor (its `image_processor` is read, and it is kept for the token ids), a bare
        OwlViTImageProcessor, or that one's configuration as a dict."""
        self.processor = processor
        cfg = _get(processor, "image_processor", None) or processor
        if not _get(cfg, "do_resize", True):
            raise ValueError("DeviceOwlProcessor: do_resize=False is not served (the detector takes one fixed input size)")
        if _get(cfg, "do_center_crop", False):
            raise ValueError("DeviceOwlProcessor: do_center_crop is not served")
        if _get(cfg, "do_pad", False):
            raise ValueError("DeviceOwlProcessor: do_pad is not served")
        size = _get(cfg, "size")
        if isinstance(size, int):
            size = {"height": size, "width": size}
        elif isinstance(size, (tuple, list)) and len(size) == 2:
            size = {"height": size[0], "width": size[1]}
        keys = ("height", "width", "shortest_edge", "longest_edge", "max_height", "max_width")
        given = {k: _get(size, k) for k in keys if size is not None and _get(size, k) is not None}
        if set(given) != {"height", "width"}:
            raise ValueError(f"DeviceOwlProcessor: size {size!r} is not a fixed (height, width)")
        self.size = (int(given["height"]), int(given["width"]))
        resample = _get(cfg, "resample")
        if resample is None or int(resample) not in _FILTER_NAMES:
            raise ValueError(f"DeviceOwlProcessor: resample {resample!r} is none of Pillow's BILINEAR (2), BICUBIC (3), "
                             "LANCZOS (1)")
        self.filter = _FILTER_NAMES[int(resample)]
        self.rescale = float(_get(cfg, "rescale_factor", 1.0 / 255.0)) if _get(cfg, "do_rescale", True) else 1.0
        if _get(cfg, "do_normalize", True):
            mean, std = _get(cfg, "image_mean"), _get(cfg, "image_std")
            if mean is None or std is None or len(mean) != 3 or len(std) != 3:
                raise ValueError("DeviceOwlProcessor: image_mean and image_std hold one value per RGB channel")
            self.mean, self.std = tuple(float(v) for v in mean), tuple(float(v) for v in std)
        else:
            self.mean, self.std = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)

    def resized(self, images):
        """uint8 (N, h, w, 3) on the device -> uint8 (N, H, W, 3): the processor's Pillow resize alone."""
        return ops.resample_u8(images, self.size, self.filter, "u8")

    def pixel_values(self, images, dtype=torch.float32):
        """uint8 (N, h, w, 3) on the device -> `pixel_values` (N, 3, H, W), one call."""
        return ops.resample_u8(images, self.size, self.filter, "affine", dtype=dtype, rescale=self.rescale, mean=self.mean,
                               std=self.std)

    def input_ids(self, texts):
        """Query strings of one image -> the tokenizer's id rows (Q, S), through the processor this one was built from."""
        if _get(self.processor, "image_processor", None) is None or not callable(self.processor):
            raise RuntimeError("DeviceOwlProcessor was built from an image processor alone: it has no tokenizer")
        return self.processor(text=[list(texts)], return_tensors="pt")["input_ids"]

"""utils/eval/eval.py of the reference on the HIP engine: same names and signatures.

`nms` / `class_aware_nms` (eval.py:11-105) run `lgd_detect_nms_f32` in mode 1 on the host lists they are given and
return the same numpy triples; `eval_prompt` (eval.py:120-174) with a `lgd_amd.owlvit.HipOwlViTDetector` as `model`
runs `model.detect()` (forward + post_process + score filter + NMS on the device, one host read) and builds the same
`det_boxes` dicts.  `eval_images` is the batched form the reference does not have, `eval_device_images` the same for
images that are still on the GPU (lgd_amd.owl_processor.DeviceOwlProcessor in place of the processor's image half).
Scores are ordered with the lower index first where they are equal (numpy's argsort at eval.py:45 leaves that open);
arithmetic is fp32 where the reference's numpy runs in the precision of its inputs."""
import numpy as np
import torch
from PIL import Image

from lgd_amd import ops
from lgd_amd.owl_processor import DeviceOwlProcessor
from lgd_amd.owlvit import HipOwlViTDetector

__all__ = ["get_eval_info_from_prompt", "nms", "class_aware_nms", "evaluate_with_boxes", "to_gen_box_format",
           "eval_prompt", "eval_images", "eval_device_images"]


def get_eval_info_from_prompt(prompt, prompt_type):
    if prompt_type.startswith("lmd"):
        from .lmd import get_eval_info_from_prompt_lmd      # the reference's own file (LGD_REFERENCE_ROOT)
        return get_eval_info_from_prompt_lmd(prompt)
    raise ValueError(f"Unknown prompt type: {prompt_type}")


def _device_nms(bounding_boxes, confidence_score, labels, threshold, class_aware, input_in_pixels, return_array=True):
    if input_in_pixels:
        raise NotImplementedError("input_in_pixels=True (areas with +1) is not used by eval_prompt")
    if len(bounding_boxes) == 0:
        return np.array([]), np.array([]), np.array([])
    n = len(bounding_boxes)
    dev = torch.device("cuda")
    boxes = torch.as_tensor(np.asarray(bounding_boxes, dtype=np.float32).reshape(1, n, 4), device=dev)
    scores = torch.as_tensor(np.asarray(confidence_score, dtype=np.float32).reshape(1, n), device=dev)
    # labels may be any sortable values: the kernel sees their ranks (np.unique order = class_aware_nms's label order)
    _, ranks = np.unique(np.asarray(labels).reshape(n), return_inverse=True)
    lab = torch.as_tensor(ranks.astype(np.int32).reshape(1, n), device=dev)
    counts = torch.full((1,), n, device=dev, dtype=torch.int32)
    # every given box is a candidate: the filter of eval.py:144-148 happened at the caller
    _, _, _, index, count = ops.detect_nms(scores, boxes, labels=lab, counts=counts, score_threshold=0.0,
                                           nms_threshold=threshold, class_aware=class_aware)
    keep = index[0, :int(count.item())].cpu().numpy()
    picked = ([bounding_boxes[i] for i in keep], [confidence_score[i] for i in keep], [labels[i] for i in keep])
    return tuple(np.array(p) for p in picked) if return_array else picked


def nms(bounding_boxes, confidence_score, labels, threshold, input_in_pixels=False, return_array=True):
    """Greedy NMS over all boxes, whatever their labels (a box suppresses boxes of other labels too)."""
    return _device_nms(bounding_boxes, confidence_score, labels, threshold, False, input_in_pixels, return_array)


def class_aware_nms(bounding_boxes, confidence_score, labels, threshold, input_in_pixels=False):
    """Greedy NMS within each label; labels come out in ascending order."""
    return _device_nms(bounding_boxes, confidence_score, labels, threshold, True, input_in_pixels)


def evaluate_with_boxes(boxes, eval_info, verbose=False):
    """Applies the prompt's predicate (built by the reference's lmd.py) to the detections."""
    print("boxes:", boxes)
    return eval_info["predicate"](boxes, verbose)


def to_gen_box_format(box, width, height):
    """Normalised (x0, y0, x1, y1) -> [x, y, w, h] in pixels, the layout boxes have in the generation specs."""
    x0, y0, x1, y1 = box
    return [x0 * width, y0 * height, (x1 - x0) * width, (y1 - y0) * height]


def _det_boxes(text, boxes, scores, labels, width, height):
    return [{"name": text[label], "bounding_box": to_gen_box_format(box, width, height), "score": score}
            for box, score, label in zip(boxes, scores, labels)]


def eval_images(model, processor, items, score_threshold=0.1, nms_threshold=0.5, use_class_aware_nms=False):
    """Several images, each with its own queries, through ONE `model.detect()` call.  items: [(PIL image, [query
    strings])]; query sets shorter than the longest are padded by all-zero id rows (masked queries).  Returns one
    `det_boxes` list per image (name, xywh in pixels, score), in the order eval_prompt produces."""
    if not isinstance(model, HipOwlViTDetector):
        raise TypeError("eval_images needs a lgd_amd.owlvit.HipOwlViTDetector")
    Q = max(len(texts) for _, texts in items)
    pixel_values, ids = [], []
    for image, texts in items:
        inputs = processor(text=[list(texts)], images=image, return_tensors="pt")
        pixel_values.append(inputs["pixel_values"])
        rows = inputs["input_ids"]
        ids.append(torch.cat([rows, rows.new_zeros((Q - rows.shape[0], rows.shape[1]))]))
    det = model.detect(torch.cat(pixel_values), torch.cat(ids), score_threshold=score_threshold,
                       nms_threshold=nms_threshold, class_aware=use_class_aware_nms)
    out = []
    for b, (image, texts) in enumerate(items):
        width, height = image.size
        boxes, scores, labels = (t.cpu().numpy() for t in det.image(b))
        out.append(_det_boxes(texts, boxes, scores, labels, width, height))
    return out


def eval_device_images(model, processor, images, texts, score_threshold=0.1, nms_threshold=0.5, use_class_aware_nms=False):
    """eval_images for images that are already on the GPU: images uint8 (N, h, w, 3) on the device (a generation made with
    decode="device", or the refiner's output="device"), texts one list of query strings per image.  processor: the
    OwlViTProcessor, or a DeviceOwlProcessor built from it — its image half (Pillow resize, rescale, normalise) runs as
    one ops.resample_u8 call on the device, bit for bit Pillow's resize; the token ids come from its tokenizer.  The
    pixels never visit the host.  Returns one `det_boxes` list per image, as eval_images."""
    if not isinstance(model, HipOwlViTDetector):
        raise TypeError("eval_device_images needs a lgd_amd.owlvit.HipOwlViTDetector")
    if not torch.is_tensor(images) or not images.is_cuda or images.dtype != torch.uint8 or images.dim() != 4:
        raise TypeError("eval_device_images takes a uint8 (N, h, w, 3) tensor on the GPU; eval_images takes PIL images")
    if len(texts) != images.shape[0]:
        raise ValueError(f"{len(texts)} query lists for {images.shape[0]} images")
    dproc = processor if isinstance(processor, DeviceOwlProcessor) else DeviceOwlProcessor(processor)
    Q = max(len(t) for t in texts)
    ids = []
    for t in texts:
        rows = dproc.input_ids(t)
        ids.append(torch.cat([rows, rows.new_zeros((Q - rows.shape[0], rows.shape[1]))]))
    det = model.detect(dproc.pixel_values(images.contiguous()), torch.cat(ids), score_threshold=score_threshold,
                       nms_threshold=nms_threshold, class_aware=use_class_aware_nms)
    height, width = images.shape[1], images.shape[2]
    out = []
    for b, t in enumerate(texts):
        boxes, scores, labels = (x.cpu().numpy() for x in det.image(b))
        out.append(_det_boxes(t, boxes, scores, labels, width, height))
    return out


def eval_prompt(p, prompt_type, path, processor, model, score_threshold=0.1, nms_threshold=0.5,
                use_class_aware_nms=False, verbose=False, use_cuda=True):
    texts, eval_info = get_eval_info_from_prompt(p, prompt_type)
    image = Image.open(path)
    width, height = image.size
    text = texts[0]       # one image per call: its query strings

    if not isinstance(model, HipOwlViTDetector):
        raise TypeError("eval_prompt runs on a lgd_amd.owlvit.HipOwlViTDetector (owlvit.from_hf(hf_model)); there is no "
                        "torch fallback")
    inputs = processor(text=texts, images=image, return_tensors="pt")
    det = model.detect(inputs["pixel_values"], inputs["input_ids"], score_threshold=score_threshold,
                       nms_threshold=nms_threshold, class_aware=use_class_aware_nms)
    boxes, scores, labels = (t.cpu().numpy() for t in det.image(0))

    print("Post-NMS:")
    for box, score, label in zip(boxes, scores, labels):
        box = [round(i, 2) for i in box.tolist()]
        print(f"Detected {text[label]} ({label}) with confidence {round(score.item(), 3)} at location {box}")
    if verbose:
        print(f"prompt: {p}, texts: {texts}, boxes: {boxes}, labels: {labels}, eval_info: {eval_info}")

    det_boxes = _det_boxes(text, boxes, scores, labels, width, height)
    eval_type = eval_info["type"]
    eval_success = evaluate_with_boxes(det_boxes, eval_info, verbose=verbose)
    return eval_type, eval_success

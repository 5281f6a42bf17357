"""Image chunking: the model-free 'simple' / 'overlap' patch methods and the attention-based 'dino-v1' / 'dino-v2' of the reference
(src/marqo/s2_inference/processing/image.py:46-151,154-373, image_utils.py:16-22,40-56,98-139,141-307, DINO_utils.py).

`chunk_image(image, device, method)` keeps the reference's signature and return value
`(patches: List[PIL.Image], bboxes_orig: List[[x1, y1, x2, y2] floats])` — the whole 240x240 working image first —
but the resampling runs on the GPU, bit-identical to Pillow, and so does the DINO ViT with everything up to the boxes of its attention
maps (engine/dino.py).  The detector-based chunkers (frcnn / yolox) are separate detector networks and out of scope.

`chunk_images_to_tensors` is the engine's fused form: for a CLIP model it returns the crops already resized /
centre-cropped / normalised on the device (K11), ready for `encode_image` without a host round trip.
"""
from __future__ import annotations

import datetime
import os
import threading
from typing import List, Optional, Tuple, Union
from urllib.parse import urlparse

import numpy as np
import PIL
from PIL import Image
from PIL.Image import Image as ImageType

from marqo_amd.s2_inference.errors import ChunkerError, ChunkerMethodProcessError, ModelLoadError
from marqo_amd.s2_inference.image_input import format_and_load_CLIP_image, pil_to_pixels, pil_to_rgb_u8

_local = threading.local()
_load_model_lock = threading.Lock()


def get_default_size() -> Tuple[int, int]:
    return (240, 240)


def str2bool(string: str) -> bool:
    return string.lower() in ("true", "1", "t")   # image_utils.py:204-213 (pinned by tests/test_ref_parity.py)


def rescale_box(box, from_size: Tuple, to_size: Tuple) -> List[float]:
    fy, fx = to_size[1] / from_size[1], to_size[0] / from_size[0]
    x1, y1, x2, y2 = box
    return [x1 * fx, y1 * fy, x2 * fx, y2 * fy]


def generate_boxes(image_size: Tuple[int, int], hn: int, wn: int, overlap: bool = False) -> List[Tuple]:
    """grid of (x1, y1, x2, y2) integer boxes; cells that would exceed the image are skipped; `overlap` adds a box shifted
    by half a cell after every grid cell (image_utils.py:165-202)."""
    img_width, img_height = image_size
    height, width = img_height // hn, img_width // wn
    bboxes = []
    for i in range(0, img_height, height):
        for j in range(0, img_width, width):
            p1, p2 = j + width, i + height
            if p1 > img_width or p2 > img_height:
                continue
            bboxes.append((j, i, p1, p2))
            if overlap:
                p3, p4 = p1 + width // 2, p2 + height // 2
                if p3 > img_width or p4 > img_height:
                    continue
                bboxes.append((j + width // 2, i + height // 2, p3, p4))
    return bboxes


def patchify_image(image: ImageType, bboxes) -> List[ImageType]:
    return [image.crop(bb) for bb in bboxes]


def _process_patch_method(method: str):
    """'simple', 'simple?hn=3', 'overlap?hn=3&wn=4' -> (method, params)"""
    req = urlparse(method)
    params = dict()
    if len(req.query) == 0:
        return req.path, params
    try:
        params = dict(x.split("=") for x in req.query.split("&"))
    except Exception:
        raise ChunkerMethodProcessError(message=f"could not pass parameters for string {req.query} from full path {method}")
    return req.path, params


def _preprocessor(device: str, size: int = 224):
    from marqo_amd.engine.preprocess import ImagePreprocessor
    key = (device, size)
    cache = getattr(_local, "pre", None)
    if cache is None:
        cache = _local.pre = {}
    if key not in cache:
        cache[key] = ImagePreprocessor(device, size)
    return cache[key]


class PatchifySimple:
    def __init__(self, size: Tuple = (512, 512), hn: int = 3, wn: int = 3, overlap: bool = False, device: str = "cuda", **kwargs):
        self.size, self.hn, self.wn, self.overlap, self.device = size, hn, wn, overlap, device

    def infer(self, image: Union[str, ImageType]):
        self.image = format_and_load_CLIP_image(image, {})
        self.original_size = self.image.size
        u8 = _preprocessor(self.device).resize_u8([pil_to_pixels(self.image)], self.size[1], self.size[0])
        self.image_resized = Image.fromarray(u8[0].cpu().numpy(), "RGB")
        self.bboxes_simple = generate_boxes(self.size, self.hn, self.wn, overlap=self.overlap)

    def process(self):
        self.bboxes = [(0, 0, self.size[0], self.size[1])] + self.bboxes_simple
        self.patches = patchify_image(self.image_resized, self.bboxes)
        self.bboxes_orig = [rescale_box(bb, self.size, self.original_size) for bb in self.bboxes]


# ---- the box pipeline of the model-based chunkers (image_utils.py:40-56,98-139,215-265; image.py:243-310) ---------------------------------------
def _keep_topk(boxes_xyxy, k: int = 10):
    if k == 0:
        return []
    if len(boxes_xyxy) <= k:
        return boxes_xyxy
    return boxes_xyxy[:k]


def calc_area(bboxes, size: Optional[Tuple[int, int]] = None) -> List[float]:
    """area of every (x1, y1, x2, y2) box as a fraction of `size` (w, h)"""
    A = 1.0 if size is None else size[0] * size[1] * 1.0
    return [(bb[2] - bb[0]) * (bb[3] - bb[1]) / A for bb in bboxes]


def filter_boxes(bboxes, max_aspect_ratio: int = 4, min_area: int = 40 * 40) -> List[int]:
    """indices of the boxes whose area exceeds min_area and whose aspect ratio is below max_aspect_ratio"""
    inds = []
    for ind, bb in enumerate(bboxes):
        w, h = (bb[2] - bb[0]), (bb[3] - bb[1])
        if w * h > min_area and max(w, h) / min(w, h) < max_aspect_ratio:
            inds.append(ind)
    return inds


def replace_small_boxes(boxes, min_area: float = 40 * 40, new_size: Tuple = (100, 100)) -> List[Tuple]:
    """a box below min_area gives way to one of new_size around the same centre"""
    new_boxes = []
    for box in boxes:
        if (box[2] - box[0]) * (box[3] - box[1]) < min_area:
            xc = (box[2] - box[0]) / 2 + box[0]
            yc = (box[3] - box[1]) / 2 + box[1]
            box = (xc - new_size[0] / 2, yc - new_size[1] / 2, xc + new_size[0] / 2, yc + new_size[1] / 2)
        new_boxes.append(box)
    return new_boxes


def clip_boxes(boxes, xmin: int, ymin: int, xmax: int, ymax: int) -> List[Tuple]:
    return [(np.clip(x1, xmin, xmax), np.clip(y1, ymin, ymax), np.clip(x2, xmin, xmax), np.clip(y2, ymin, ymax)) for x1, y1, x2, y2 in boxes]


def nms(boxes, scores, iou_threshold: float) -> List[int]:
    """class-agnostic non-maximum suppression with torchvision.ops.nms semantics, in float32: boxes taken by falling score (ties: input order), a
    box is dropped when its IoU with a kept one EXCEEDS the threshold; returns the kept indices by falling score"""
    b = np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
    sc = np.asarray(scores, dtype=np.float32).reshape(-1)
    order = np.argsort(-sc, kind="stable")
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    dead = np.zeros(len(b), dtype=bool)
    keep = []
    for pos, i in enumerate(order):
        if dead[i]:
            continue
        keep.append(int(i))
        rest = order[pos + 1:]
        w = np.maximum(np.float32(0), np.minimum(b[i, 2], b[rest, 2]) - np.maximum(b[i, 0], b[rest, 0]))
        h = np.maximum(np.float32(0), np.minimum(b[i, 3], b[rest, 3]) - np.maximum(b[i, 1], b[rest, 1]))
        inter = w * h
        dead[rest[inter / (area[i] + area[rest] - inter) > np.float32(iou_threshold)]] = True
    return keep


def box_pipeline(boxes_xyxy, scores, size, min_area=60 * 60, min_area_replace=60 * 60, new_size=(100, 100), iou_thresh=0.6, top_k=10,
                 filter_bb=True, replace_small=True, do_nms=True):
    """PatchifyModel.process() without the crops (image.py:243-302): filter -> replace small + clip -> NMS -> _keep_top_k -> (boxes, scores)"""
    boxes_xyxy, scores = list(boxes_xyxy), list(scores)
    if filter_bb:
        n = len(boxes_xyxy)
        inds = filter_boxes(boxes_xyxy, min_area=min_area)
        boxes_xyxy = [bb for i, bb in enumerate(boxes_xyxy) if i in inds]
        if len(scores) == n:
            scores = [sc for i, sc in enumerate(scores) if i in inds]
    if replace_small and len(boxes_xyxy):
        boxes_xyxy = clip_boxes(replace_small_boxes(boxes_xyxy, min_area=min_area_replace, new_size=new_size), 0, 0, size[0], size[1])
    if do_nms and len(boxes_xyxy) > 1:
        inds = nms(boxes_xyxy, scores, iou_thresh)
        boxes_xyxy, scores = [boxes_xyxy[i] for i in inds], [scores[i] for i in inds]
    if top_k is not None and top_k > len(boxes_xyxy):      # as written in the reference: acts only when there is nothing to cut
        boxes_xyxy = _keep_topk(boxes_xyxy, k=top_k)
    return boxes_xyxy, scores


DINO_CHECKPOINT_ENV = "MARQO_DINO_CHECKPOINT"
DINO_HUB_FILES = {("vit_small", 16): "dino_deitsmall16_pretrain.pth", ("vit_small", 8): "dino_deitsmall8_pretrain.pth",
                  ("vit_base", 16): "dino_vitbase16_pretrain.pth", ("vit_base", 8): "dino_vitbase8_pretrain.pth"}


def _find_dino_checkpoint(model_name: str, patch_size: int) -> str:
    """MARQO_DINO_CHECKPOINT, else the file torch.hub.load('facebookresearch/dino:main', ...) leaves in torch hub's checkpoint directory (local
    files only: nothing is downloaded) -> path, or ChunkerError naming both places"""
    import torch
    env = os.environ.get(DINO_CHECKPOINT_ENV)
    hub = os.path.join(torch.hub.get_dir(), "checkpoints", DINO_HUB_FILES[(model_name, patch_size)])
    for p in (env, hub):
        if p and os.path.isfile(p):
            return p
    raise ChunkerError(f"the dino patch methods need the DINO {model_name}/{patch_size} checkpoint: neither ${DINO_CHECKPOINT_ENV} "
                       f"({env or 'not set'}) nor {hub} is a file")


def _load_DINO_model(arch: str, device: str, patch_size: int = 16):
    from marqo_amd.engine.dino import load_dino
    return load_dino(_find_dino_checkpoint(arch, patch_size), device, arch, patch_size), None


class PatchifyViT:
    """'dino-v1' (attention_method 'abs': one map, the mean over the heads) / 'dino-v2' ('pos': one map per head): boxes around the bright regions
    of the class token's last-block attention in a DINO ViT-S/16, then the reference's box pipeline (image.py:154-373).  Kept as written there:
    the maps are 224 px wide while scores, clipping and crops use `size` (240 x 240), and `_keep_top_k` never truncates."""
    model_name, patch_size, model_size = "vit_small", 16, 224

    def __init__(self, device: str = None, size: Tuple = (224, 224), min_area: float = 60 * 60, do_nms: bool = True, replace_small: bool = True,
                 top_k: int = 10, filter_bb: bool = True, min_area_replace: float = 60 * 60, attention_method: str = "pos"):
        if not device:
            raise ValueError("`device` is required for loading the DINO model")
        self.scores: List[float] = []
        self.size, self.device = size, device
        self.min_area, self.min_area_replace = min_area, min_area_replace
        self.do_nms, self.replace_small, self.top_k, self.filter_bb = do_nms, replace_small, top_k, filter_bb
        self.new_size, self.iou_thresh, self.top_k_scores = (100, 100), 0.6, 100
        self.attention_method = attention_method
        if not (attention_method.startswith("abs") or attention_method.startswith("pos")):
            raise TypeError(f"unknown method of {attention_method}")
        self._load_and_cache_model()

    def _load_and_cache_model(self):
        """the available-models cache and the load lock of the reference (image.py:207-232); the entry keeps the reference's (model, preprocess)
        pair, whose second half is None here: the resizes run on the device in infer()"""
        from marqo_amd.s2_inference.enums import AvailableModelsKey
        from marqo_amd.s2_inference.s2_inference import _create_model_cache_key, get_available_models
        key = _create_model_cache_key(self.model_name, self.device)
        if _load_model_lock.locked():
            raise ModelLoadError("Request rejected, as this request attempted to load and cache the model, but the lock is already held by another "
                                 "operation. Please wait for a few seconds and send the request again.\n")
        with _load_model_lock:
            if key not in get_available_models():
                self.model, _ = _load_DINO_model(self.model_name, self.device, self.patch_size)
                get_available_models()[key] = {AvailableModelsKey.model: (self.model, None),
                                               AvailableModelsKey.most_recently_used_time: datetime.datetime.now()}
            else:
                self.model, _ = get_available_models()[key][AvailableModelsKey.model]

    def infer(self, image: Union[str, ImageType]):
        from marqo_amd.engine.dino import MODE_MEAN, MODE_PER_HEAD
        image = format_and_load_CLIP_image(image, {})
        self.original_size = image.size
        pre = _preprocessor(self.device)
        u8 = pre.resize_u8([pil_to_rgb_u8(image)], self.size[1], self.size[0])                   # convert('RGB').resize(size): BICUBIC
        self.image = Image.fromarray(u8[0].cpu().numpy(), "RGB")
        S = self.model_size
        model_in = pre.resize_u8([u8[0]], S, S, interpolation="bilinear")                       # the DINO transform's Resize((224, 224))
        mode = MODE_MEAN if self.attention_method.startswith("abs") else MODE_PER_HEAD
        boxes, counts = self.model.boxes(model_in, mode)
        boxes, counts = boxes[0].cpu().numpy(), counts[0].cpu().numpy()
        self.boxes_xyxy = [tuple(int(v) for v in boxes[m, k]) for m in range(boxes.shape[0]) for k in range(int(counts[m]))]
        self.scores = calc_area(self.boxes_xyxy, self.size) if self.boxes_xyxy else []
        self._keep_top_k_sorted()

    def _keep_top_k_sorted(self):
        if len(self.scores) > self.top_k_scores:
            inds = np.argsort(np.array(self.scores).squeeze())[::-1][:self.top_k_scores]
            self.boxes_xyxy = [self.boxes_xyxy[i] for i in inds]
            self.scores = [self.scores[i] for i in inds]

    def process(self):
        self.boxes_xyxy, self.scores = box_pipeline(self.boxes_xyxy, self.scores, self.size, min_area=self.min_area,
                                                    min_area_replace=self.min_area_replace, new_size=self.new_size, iou_thresh=self.iou_thresh,
                                                    top_k=self.top_k, filter_bb=self.filter_bb, replace_small=self.replace_small, do_nms=self.do_nms)
        self.bboxes = [(0, 0, self.size[0], self.size[1])] + self.boxes_xyxy
        self.patches = patchify_image(self.image, self.bboxes)
        self.bboxes_orig = [rescale_box(bb, self.size, self.original_size) for bb in self.bboxes]


def chunk_image(image: Union[str, ImageType], device: str, method: str, size=get_default_size()):
    HN = WN = 3
    if method in [None, "none", "", "None", " "]:
        if isinstance(image, str):
            return [image], [image]
        elif isinstance(image, ImageType):
            return [image], [(0, 0, image.size[0], image.size[1])]
        raise TypeError(f"only pointers to an image or a PIL image are allowed. received {type(image)}")
    method, params = _process_patch_method(method)
    hn, wn = int(params.get("hn", HN)), int(params.get("wn", WN))
    if method == "simple":
        patch = PatchifySimple(size=size, hn=hn, wn=wn, device=device)
    elif method == "overlap":
        patch = PatchifySimple(size=size, hn=hn, wn=wn, overlap=True, device=device)
    elif method in ["dino-v1", "dino-v2", "dino/v1", "dino/v2"]:
        patch = PatchifyViT(device=device, filter_bb=True, size=size, attention_method="abs" if "v1" in method else "pos", do_nms=True,
                            replace_small=True)
    elif method in ["fastercnn", "frcnn", "marqo-yolo", "yolox"]:
        raise ChunkerError(f"patch method {method!r} needs a detector model, which the marqo_amd engine does not provide")
    else:
        raise ValueError(f"unexpected image chunking type. found {method}")
    try:
        patch.infer(image)
        patch.process()
    except PIL.UnidentifiedImageError as e:
        raise ChunkerError from e
    return patch.patches, patch.bboxes_orig


def chunk_images_to_tensors(images: List[Union[str, ImageType, np.ndarray]], model, method: str = "simple"):
    """Fused K11 path for a loaded CLIP-family engine model: -> (Tensor [n, count, 3, S, S] fp32 on device, boxes [n, count, 4])."""
    method, params = _process_patch_method(method)
    if method not in ("simple", "overlap"):
        raise ValueError(f"unexpected image chunking type. found {method}")
    hn, wn = int(params.get("hn", 3)), int(params.get("wn", 3))
    raw = [pil_to_pixels(format_and_load_CLIP_image(i, {})) if not isinstance(i, np.ndarray) else i for i in images]
    pre = model._pre()
    u8, boxes = pre.chunk_grid_u8(raw, hn, wn, method == "overlap")
    t = pre.to_tensor_normalize(u8)
    return t.reshape(len(raw), -1, *t.shape[1:]), boxes

"""The LanguageBind video front end on the GPU: decoded uint8 frames -> the `pixel_values` [b, 3, T, S, S] its video tower takes (reference:
s2_inference/languagebind/video/processing_video.py:20-93 — `np.linspace` frame pick, x / 255, NormalizeVideo, pytorchvideo's ShortSideScale,
torchvision's CenterCropVideo, RandomHorizontalFlipVideo).

    mq_video_preprocess (per clip: pick T frames, normalise each tap, bilinear short-side scale, S x S centre window, optional mirror; one pass, the
    scaled frame is never stored)

It runs on the current stream of the calling thread; a call allocates the output, the frame picks and, for a clip that comes from the host, its
device copy (T_in x H x W x 3 bytes) through PyTorch's allocator.

The integers are where a port goes wrong silently, so each is a function of its own here:
  * `pick_frames`:      np.linspace(0, T_in - 1, num_frames, dtype=int), which TRUNCATES: 11 frames -> [0, 1, 2, 4, 5, 7, 8, 10];
  * `short_side_scale`: pytorchvideo's rule, the floor of the DOUBLE product float(h) / w * S: 320 x 240 at 224 -> 298 (not 299);
  * `center_crop`:      torchvision's video center_crop, int(round((new - S) / 2.0)) with Python's round, half to EVEN: 75 -> 38, 73 -> 36.

What is NOT here, and what differs from the reference:
  * decoding: a clip is the uint8 [T_in, H, W, 3] array a decoder (decord, opencv after its BGR -> RGB) returns.  Paths, URLs and bytes are refused:
    nothing in this engine decodes media;
  * the RANDOM flip.  The reference mirrors a clip with probability 0.5 (RandomHorizontalFlipVideo): the same file gives one of two pictures at
    every call.  This front end never flips unless told to (`flip`), the same decision as the audio front end's crop starts (engine/audio.py);
  * the side: the reference hard-codes 224 for both ShortSideScale and CenterCropVideo; here it is the checkpoint's `image_size` (224 for the
    released ones).
"""
from __future__ import annotations

import ctypes as C
import math
from typing import List, Sequence, Tuple

import numpy as np
import torch

from marqo_amd import _lib as L

Tensor = torch.Tensor
OPENAI_MEAN = (0.48145466, 0.4578275, 0.40821073)
OPENAI_STD = (0.26862954, 0.26130258, 0.27577711)
MAX_SIDE, MAX_SIZE, MAX_FRAMES_OUT = 16384, 4096, 4096     # mq_video_preprocess


def pick_frames(t_in: int, num_frames: int) -> List[int]:
    """np.linspace(0, t_in - 1, num_frames, dtype=int): evenly spaced positions, truncated towards zero (one frame: that frame num_frames times)"""
    if t_in < 1 or num_frames < 1:
        raise ValueError(f"a clip has at least one frame and at least one is picked (T_in = {t_in}, num_frames = {num_frames})")
    return [int(v) for v in np.linspace(0, t_in - 1, num_frames, dtype=int)]


def short_side_scale(h: int, w: int, size: int) -> Tuple[int, int]:
    """(new_h, new_w) of pytorchvideo.transforms.functional.short_side_scale: the short side becomes `size`, the long one the floor of the double
    product float(long) / short * size"""
    if w < h:
        return int(math.floor((float(h) / w) * size)), size
    return size, int(math.floor((float(w) / h) * size))


def center_crop(new_h: int, new_w: int, size: int) -> Tuple[int, int]:
    """(top, left) of torchvision's video center_crop: int(round((new - size) / 2.0)), Python's round (half to even)"""
    return int(round((new_h - size) / 2.0)), int(round((new_w - size) / 2.0))


class VideoPreprocessor:
    """`__call__(clips, flip=None)` -> {"pixel_values": fp32 [b, 3, num_frames, size, size] on the device}.  A clip is a uint8 tensor / ndarray
    [T_in, H, W, 3] (T_in >= 1, RGB last: what decord's get_batch returns), on the host or on the device, or a {"frames": such an array} dict;
    `clips` is one clip or a list of clips, whose sizes may differ.  `flip`: None (no clip is mirrored), one bool (for every clip), or one bool per
    clip.  The reference mirrors at RANDOM with p = 0.5; this front end never flips unless told to."""

    def __init__(self, device: str, size: int, num_frames: int, mean: Sequence[float] = OPENAI_MEAN, std: Sequence[float] = OPENAI_STD):
        if not 1 <= size <= MAX_SIZE or not 1 <= num_frames <= MAX_FRAMES_OUT:
            raise ValueError(f"the video front end takes a side of 1 to {MAX_SIZE} pixels and 1 to {MAX_FRAMES_OUT} frames per clip "
                             f"(size = {size}, num_frames = {num_frames})")
        if len(mean) != 3 or len(std) != 3 or not all(float(s) > 0 for s in std):
            raise ValueError(f"the video front end takes three means and three positive stds (mean = {mean}, std = {std})")
        self.device, self.size, self.num_frames = device, int(size), int(num_frames)
        self.mean, self.std = tuple(float(m) for m in mean), tuple(float(s) for s in std)

    # ---- host side: what is accepted ---------------------------------------------------------------------------------------------------------
    def _clip(self, item) -> Tensor:
        """one item -> a host or device uint8 tensor [T_in, H, W, 3], checked; nothing is moved yet"""
        if isinstance(item, dict) and set(item) == {"frames"}:
            item = item["frames"]
        if isinstance(item, (str, bytes, bytearray)):
            what = "bytes" if not isinstance(item, str) else repr(item if len(item) <= 80 else item[:77] + "...")
            raise ValueError(f"Unsupported video content type: {type(item)}: {what} — nothing in this engine decodes media; pass the decoded frames "
                             f"(uint8 [T_in, H, W, 3])")
        if isinstance(item, np.ndarray):
            if item.dtype != np.uint8:
                raise ValueError(f"Unsupported video content type: a clip is a uint8 tensor or ndarray [T_in, H, W, 3], got {item.dtype} {item.shape}")
            item = torch.from_numpy(np.ascontiguousarray(item))
        if not isinstance(item, torch.Tensor) or item.dtype != torch.uint8 or item.ndim != 4 or item.shape[3] != 3 or item.shape[0] < 1:
            got = f"{item.dtype} {tuple(item.shape)}" if isinstance(item, torch.Tensor) else type(item).__name__
            raise ValueError(f"Unsupported video content type: a clip is a uint8 tensor or ndarray [T_in, H, W, 3] of decoded frames (RGB last, "
                             f"T_in >= 1), got {got} — nothing in this engine decodes media, and no other layout is rearranged")
        t_in, h, w = item.shape[:3]
        new_h, new_w = short_side_scale(h, w, self.size) if h >= 1 and w >= 1 else (0, 0)
        if not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE and new_h <= MAX_SIDE and new_w <= MAX_SIDE and t_in < 2 ** 31):
            raise ValueError(f"frames of {h} x {w} ({t_in} of them) are outside what mq_video_preprocess indexes: both sides in [1, {MAX_SIDE}] before "
                             f"and after the short side is scaled to {self.size} (that would be {new_h} x {new_w}), fewer than 2^31 frames")
        return item

    def _flips(self, flip, count: int) -> List[bool]:
        is_bool = lambda v: isinstance(v, (bool, np.bool_))
        if flip is None:
            return [False] * count
        if is_bool(flip):
            return [bool(flip)] * count
        if isinstance(flip, (list, tuple)) and len(flip) == count and all(is_bool(v) for v in flip):
            return [bool(v) for v in flip]
        raise ValueError(f"`flip` is None, one bool, or a list with one bool per clip ({count} here), got {flip!r}")

    # ---- the call -------------------------------------------------------------------------------------------------------------------------------
    def __call__(self, clips, flip=None):
        items = list(clips) if isinstance(clips, (list, tuple)) else [clips]
        if not items:
            raise ValueError("Unsupported video content type: an empty list of clips")
        frames = [self._clip(it) for it in items]
        flips = self._flips(flip, len(frames))
        lib, dev, S, T = L.load(), self.device, self.size, self.num_frames
        mean, std = (C.c_float * 3)(*self.mean), (C.c_float * 3)(*self.std)
        picks = torch.tensor([pick_frames(f.shape[0], T) for f in frames], dtype=torch.int32)
        with torch.cuda.device(dev):
            s = torch.cuda.current_stream(dev).cuda_stream
            out = torch.empty(len(frames), 3, T, S, S, dtype=torch.float32, device=dev)
            d_picks = picks.to(dev)
            for i, (f, fl) in enumerate(zip(frames, flips)):
                f = f.detach().to(device=dev, non_blocking=True).contiguous()
                t_in, h, w = f.shape[:3]
                new_h, new_w = short_side_scale(h, w, S)
                top, left = center_crop(new_h, new_w, S)
                L.check(lib.mq_video_preprocess(f.data_ptr(), t_in, h, w, d_picks[i].data_ptr(), T, S, new_h, new_w, top, left, mean, std, int(fl),
                                                out[i].data_ptr(), s), "mq_video_preprocess")
        return {"pixel_values": out}

"""The LanguageBind video front end without a GPU: the three integer rules of engine/video.py (frame pick, short-side scale, centre-crop offsets)
against the reference's formulas evaluated here independently, what VideoPreprocessor and encode(..., VIDEO) accept and refuse, the routing of
decoded frames, and mq_video_preprocess's argument checks."""
import math
from decimal import ROUND_HALF_EVEN, Decimal

import numpy as np
import pytest
import torch

from marqo_amd import _lib as L
from marqo_amd.engine import video as V
from marqo_amd.s2_inference import multimodal_model_load as MM
from marqo_amd.s2_inference.enums import Modality

NAME = "LanguageBind/Video_V1.5_FT"
PROPS = {"name": NAME, "dimensions": 64, "type": "languagebind", "loader": "languagebind", "model_size": 1,
         "supported_modalities": ["video", "language"], "video_chunk_length": 20, "audio_chunk_length": 10}


# ---- the integers ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_frames", [1, 8, 16])
def test_frame_pick_is_linspace_truncated(num_frames):
    for t_in in (1, 7, 8, 9, 11, 30, 300):
        want = np.linspace(0, t_in - 1, num_frames, dtype=int)
        got = V.pick_frames(t_in, num_frames)
        assert got == [int(v) for v in want] and all(type(v) is int for v in got)
        assert got[0] == 0 and all(0 <= v < t_in for v in got) and (num_frames == 1 or got[-1] == t_in - 1)
    assert V.pick_frames(11, 8) == [0, 1, 2, 4, 5, 7, 8, 10]              # truncation, not rounding (rounded: 0, 1, 3, 4, 6, 7, 9, 10)
    assert V.pick_frames(1, 8) == [0] * 8
    for bad in ((0, 8), (8, 0)):
        with pytest.raises(ValueError, match="at least one"):
            V.pick_frames(*bad)


# (h, w, S): landscape and portrait at the released side, the two odd crop differences, a square, upscaling, strips, an awkward ratio
SIZES = [(240, 320, 224), (320, 240, 224), (224, 299, 224), (224, 297, 224), (299, 224, 224), (64, 64, 32), (224, 224, 224), (20, 27, 32),
         (27, 20, 32), (1, 50, 32), (50, 1, 32), (64, 107, 32), (45, 60, 32), (60, 45, 32), (33, 32, 32), (1080, 1920, 224), (719, 1279, 224)]


@pytest.mark.parametrize("h,w,S", SIZES)
def test_scale_and_crop_integers(h, w, S):
    # pytorchvideo.transforms.functional.short_side_scale, restated: the floor of the double product
    if w < h:
        want = (int(math.floor((float(h) / w) * S)), S)
    else:
        want = (S, int(math.floor((float(w) / h) * S)))
    assert V.short_side_scale(h, w, S) == want
    new_h, new_w = want
    assert min(new_h, new_w) == S
    # torchvision's video center_crop, restated with an explicit half-to-even rounding (not Python's round)
    half_even = lambda d: int((Decimal(d) / 2).quantize(Decimal(1), rounding=ROUND_HALF_EVEN))
    top, left = V.center_crop(new_h, new_w, S)
    assert (top, left) == (half_even(new_h - S), half_even(new_w - S))
    assert 0 <= top <= new_h - S and 0 <= left <= new_w - S


def test_the_pinned_integers():
    assert V.short_side_scale(240, 320, 224) == (224, 298) and V.short_side_scale(320, 240, 224) == (298, 224)          # 298.67 floors to 298
    assert V.short_side_scale(224, 299, 224) == (224, 299) and V.center_crop(224, 299, 224) == (0, 38)                  # 75 / 2 = 37.5 -> 38 (even)
    assert V.short_side_scale(224, 297, 224) == (224, 297) and V.center_crop(224, 297, 224) == (0, 36)                  # 73 / 2 = 36.5 -> 36 (even)
    assert V.center_crop(299, 224, 224) == (38, 0) and V.center_crop(224, 298, 224) == (0, 37)
    assert V.short_side_scale(64, 64, 32) == (32, 32) and V.center_crop(32, 32, 32) == (0, 0)
    assert V.short_side_scale(20, 27, 32) == (32, 43) and V.center_crop(32, 43, 32) == (0, 6)                           # upscaling; 5.5 -> 6
    assert V.short_side_scale(1, 50, 32) == (32, 1600) and V.center_crop(32, 1600, 32) == (0, 784)                      # a 1-pixel strip
    assert V.short_side_scale(64, 107, 32) == (32, 53) and V.center_crop(32, 53, 32) == (0, 10)                         # 10.5 -> 10 (even)
    # the floor is of the double product, whatever it is: 719 x 1279 at 224 is 398.4...
    assert V.short_side_scale(719, 1279, 224) == (224, 398)


# ---- VideoPreprocessor: what it refuses before anything reaches a device ---------------------------------------------------------------------------
def test_preprocessor_refusals():
    pre = V.VideoPreprocessor("cuda:0", 32, 8)
    assert (pre.size, pre.num_frames, pre.mean, pre.std) == (32, 8, V.OPENAI_MEAN, V.OPENAI_STD)
    ok = torch.zeros(3, 20, 27, 3, dtype=torch.uint8)
    bads = ["/data/a.mp4", "https://example.com/a.mp4", b"\x00\x00\x00\x18ftypmp42", ["/data/a.mp4"],
            torch.zeros(3, 8, 4, 4),                                      # float pixel_values of one clip: no decoded frames
            torch.zeros(8, 3, 20, 27, dtype=torch.uint8),                 # [T, 3, H, W]: another layout
            np.zeros((8, 3, 20, 27), dtype=np.uint8), np.zeros((3, 20, 27, 3), dtype=np.float32), torch.zeros(20, 27, 3, dtype=torch.uint8),
            torch.zeros(0, 20, 27, 3, dtype=torch.uint8), [], [ok, "a.mp4"], {"pixel_values": ok}, {"frames": "a.mp4"}, 7, None]
    for bad in bads:
        with pytest.raises(ValueError, match="Unsupported video content type"):
            pre(bad)
    with pytest.raises(ValueError, match="nothing in this engine decodes media"):
        pre("/data/a.mp4")
    for flip in ([True], [True, False, True], "yes", 1, [1, 0]):
        with pytest.raises(ValueError, match="`flip` is None, one bool, or a list with one bool per clip"):
            pre([ok, ok], flip=flip)
    # too large for the kernel's index arithmetic: the stated bound, before and after scaling
    with pytest.raises(ValueError, match=r"outside what mq_video_preprocess indexes.*\[1, 16384\]"):
        pre(torch.zeros(1, 1, 16385, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match=r"that would be 32 x 32000"):
        pre(torch.zeros(1, 1, 1000, 3, dtype=torch.uint8))
    for size, frames in ((0, 8), (4097, 8), (32, 0), (32, 4097)):
        with pytest.raises(ValueError, match="side of 1 to 4096"):
            V.VideoPreprocessor("cuda:0", size, frames)
    with pytest.raises(ValueError, match="three positive stds"):
        V.VideoPreprocessor("cuda:0", 32, 8, std=(0.2, 0.0, 0.2))


# ---- encode(..., VIDEO) and preprocessor(VIDEO): routing --------------------------------------------------------------------------------------------
class FakePre:
    def __init__(self):
        self.seen = []

    def __call__(self, clips, flip=None):
        self.seen.append([tuple(c["frames"].shape) if isinstance(c, dict) else tuple(c.shape) for c in clips])
        return {"pixel_values": torch.zeros(len(clips), 3, 8, 4, 4)}


class FakeLB:
    def __init__(self, video):
        self.calls, self.built = [], 0
        if video:
            self.video = object()

    def encode_video(self, px, normalize):
        self.calls.append((tuple(px.shape), normalize))
        return torch.zeros(px.shape[0], 4)

    def video_preprocessor(self):
        self.built += 1
        return FakePre()


def test_decoded_frames_are_routed_through_the_preprocessor():
    m = MM.MultimodalModel(NAME, dict(PROPS), "cuda:0")
    m.model, m.encoder = FakeLB(True), MM.LanguageBindEncoder(m)
    pre = m.preprocessor(Modality.VIDEO)
    assert isinstance(pre, FakePre) and m.preprocessor("video") is pre and m.model.built == 1
    a, b = torch.zeros(11, 20, 27, 3, dtype=torch.uint8), np.zeros((1, 33, 32, 3), dtype=np.uint8)
    assert m.encode(a, Modality.VIDEO).shape == (1, 4)
    assert m.encode([a, b], Modality.VIDEO, normalize=False).shape == (2, 4)
    assert m.encode({"frames": b}, Modality.VIDEO).shape == (1, 4) and m.encode([{"frames": a}, b], "video").shape == (2, 4)
    assert pre.seen == [[(11, 20, 27, 3)], [(11, 20, 27, 3), (1, 33, 32, 3)], [(1, 33, 32, 3)], [(11, 20, 27, 3), (1, 33, 32, 3)]]
    assert m.model.calls == [((1, 3, 8, 4, 4), True), ((2, 3, 8, 4, 4), False), ((1, 3, 8, 4, 4), True), ((2, 3, 8, 4, 4), True)]
    # pixel_values keep their way, and never see the preprocessor
    px = torch.zeros(2, 3, 8, 4, 4)
    assert m.encode([{"pixel_values": px}], Modality.VIDEO).shape == (2, 4) and m.encode(px, Modality.VIDEO).shape == (2, 4) and len(pre.seen) == 4
    # what video_pixel_values refused stays refused, with its message: URLs, a mixed list, a uint8 batch of pixel_values, other dicts
    for bad in ("https://example.com/a.mp4", ["a.mp4"], [], [a, {"pixel_values": px}], torch.zeros(2, 3, 8, 4, dtype=torch.float32), [{"pixels": a}],
                {"frames": a, "fps": 25}, torch.zeros(3, 8, 4, 4)):
        with pytest.raises(ValueError, match="Unsupported video content type: <class"):
            m.encode(bad, Modality.VIDEO)
    assert MM.raw_video_clips(px) is None and MM.raw_video_clips([]) is None and MM.raw_video_clips([a, px]) is None
    assert len(MM.raw_video_clips(b)) == 1 and MM.raw_video_clips(b)[0] is b


def test_a_model_without_a_video_part_has_no_video_preprocessor():
    m = MM.MultimodalModel(NAME, dict(PROPS), "cuda:0")
    m.model, m.encoder = FakeLB(False), MM.LanguageBindEncoder(m)
    assert m.preprocessor(Modality.VIDEO) is None and m.preprocessor("video") is None and m.model.built == 0
    # ... and decoded frames are judged as pixel_values there, as everything always was
    with pytest.raises(ValueError, match="Unsupported video content type"):
        m.encode(torch.zeros(11, 20, 27, 3, dtype=torch.uint8), Modality.VIDEO)


# ---- the entry point's argument checks (no launch: fake, never dereferenced pointers) ------------------------------------------------------------
def test_entry_point_judges_its_arguments():
    import ctypes as C
    lib = L.load()
    fake = 256
    mean, std, zero = (C.c_float * 3)(*V.OPENAI_MEAN), (C.c_float * 3)(*V.OPENAI_STD), (C.c_float * 3)(0.2, 0.0, 0.2)

    def refused(rc, *msgs):
        assert rc == -1
        err = lib.mq_last_error()
        for msg in msgs:
            assert msg in err, err

    call = lambda frames=fake, t_in=11, h=45, w=60, pick=fake, t=8, s=32, nh=32, nw=42, top=0, left=5, m=mean, sd=std, flip=0, out=fake: \
        lib.mq_video_preprocess(frames, t_in, h, w, pick, t, s, nh, nw, top, left, m, sd, flip, out, None)
    refused(call(h=0), b"mq_video_preprocess: frames of H=0")
    refused(call(w=16385), b"mq_video_preprocess: frames of H=45 x W=16385")
    refused(call(t_in=0), b"mq_video_preprocess: T_in=0")
    refused(call(t=0), b"mq_video_preprocess: T=0")
    refused(call(t=4097), b"mq_video_preprocess: T=4097")
    refused(call(s=0), b"mq_video_preprocess: S=0")
    refused(call(nh=31), b"mq_video_preprocess: the scaled frame new_h=31")
    refused(call(nw=16385), b"mq_video_preprocess: the scaled frame new_h=32 x new_w=16385")
    refused(call(left=11), b"mq_video_preprocess: the window at top=0, left=11")
    refused(call(top=1), b"mq_video_preprocess: the window at top=1")
    refused(call(left=-1), b"mq_video_preprocess: the window")
    refused(call(flip=2), b"mq_video_preprocess: flip=2")
    refused(call(sd=zero), b"mq_video_preprocess: mean[1]", b"std must be positive")
    for kw in ({"frames": None}, {"pick": None}, {"out": None}, {"m": None}, {"sd": None}):
        refused(call(**kw), b"mq_video_preprocess: null pointer")
    refused(call(pick=fake + 2), b"mq_video_preprocess:", b"4-byte aligned")
    assert "video" in L.NO_SCRATCH_UNITS

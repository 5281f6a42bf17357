"""The LanguageBind video front end on the GPU: mq_video_preprocess against the reference's transform chain restated in torch on the CPU, and decoded
frames end to end through encode(..., VIDEO) on a synthetic `Video_V1.5_FT` directory.

THE CHAIN (`chain`).  processing_video.py:20-93 with its transforms written out: np.linspace frame pick, `b t h w c -> c t h w`, x / 255,
NormalizeVideo (sub, div), pytorchvideo's short_side_scale = F.interpolate(size=(new_h, new_w), mode="bilinear", align_corners=False),
torchvision's center_crop slice, flip of the last axis.  Twice: float32, as the reference runs it, and float64.  The mean / std constants are the
float32 values in both (they are data, as the pixels are).

BOUND.  The yardstick is the float32 chain's largest absolute error against the float64 chain on the SAME frames; the kernel may err by at most 4
times that, or 1e-6 if that is larger — the rule mq_fbank got (tests/test_audio_gpu.py): both are a handful of fp32 roundings on values below 4 in
magnitude.  Both numbers are printed on a VIDEO_FRONTEND line.  Measured on an MI355X (float32 chain / kernel, max over T_in, flip and both
frame sets): 45 x 60 1.03e-5 / 3.4e-7, 60 x 45 1.01e-5 / 3.4e-7, 33 x 32 and 32 x 32 2.1e-7 / 2.1e-7, 20 x 27 3.7e-6 / 3.5e-7, 64 x 107
1.89e-5 / 2.9e-7 (DESIGN.md §3 "LanguageBind front ends").  The float32 chain loses most of its figure in its float32 source coordinate; the
kernel's is fp64.

CONTROLS.  Each mistake a port makes silently, made on purpose in the float64 chain: its distance from the true float64 chain is printed on a
VIDEO_CONTROL line and must be at least 1000 times the bound."""
import functools
import math

import numpy as np
import pytest
import torch

from marqo_amd import _lib as L
from marqo_amd.engine import video as V
from tests import languagebind_ref as LBR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
COS_TOL = 1e-3          # the figure tests/test_languagebind_gpu.py allows the video tower
S, T = 32, 8
SHAPES = [(45, 60), (60, 45), (33, 32), (32, 32), (20, 27), (64, 107)]
T_INS = (1, 8, 11)
FLOOR = 1e-6
IMAGENET = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))


# ---- the chain, with every mistake of the controls as a switch ------------------------------------------------------------------------------------
def chain(frames, dtype, flip=False, size=S, num_frames=T, swap_hw=False, ceil=False, half_up=False, align_corners=False, late_norm=None,
          pick_shift=0):
    """frames uint8 [T_in, H, W, 3] on the host -> `dtype` [3, num_frames, size, size]"""
    t_in, h, w = frames.shape[:3]
    idx = np.minimum(np.linspace(0, t_in - 1, num_frames, dtype=int) + pick_shift, t_in - 1)
    x = frames[torch.from_numpy(idx)].permute(3, 0, 1, 2).to(dtype)
    mean = torch.tensor(V.OPENAI_MEAN, dtype=torch.float32).to(dtype)[:, None, None, None]
    std = torch.tensor(V.OPENAI_STD, dtype=torch.float32).to(dtype)[:, None, None, None]
    x = x / 255.0
    if late_norm is None:
        x = (x - mean) / std
    rnd = math.ceil if ceil else math.floor
    hh, ww = (w, h) if swap_hw else (h, w)
    new_h, new_w = (int(rnd((float(hh) / ww) * size)), size) if ww < hh else (size, int(rnd((float(ww) / hh) * size)))
    x = torch.nn.functional.interpolate(x, size=(new_h, new_w), mode="bilinear", align_corners=align_corners)
    if late_norm is not None:          # (mean, std) applied to the blended pixels instead
        x = (x - torch.tensor(late_norm[0], dtype=torch.float32).to(dtype)[:, None, None, None]) / \
            torch.tensor(late_norm[1], dtype=torch.float32).to(dtype)[:, None, None, None]
    half = (lambda d: int(math.floor(d / 2.0 + 0.5))) if half_up else (lambda d: int(round(d / 2.0)))
    i, j = half(new_h - size), half(new_w - size)
    x = x[..., i:i + size, j:j + size]
    return (x.flip(-1) if flip else x).contiguous()


@functools.lru_cache(maxsize=None)
def make_frames(t_in, h, w, kind="random"):
    """uint8 [t_in, h, w, 3]: seeded noise, or a distinct ramp along every axis and in every channel (a transposed or shifted read shows)"""
    if kind == "random":
        g = torch.Generator().manual_seed(1000 * t_in + 10 * h + w)
        return torch.randint(0, 256, (t_in, h, w, 3), dtype=torch.uint8, generator=g)
    t, y, x, c = torch.meshgrid(torch.arange(t_in), torch.arange(h), torch.arange(w), torch.arange(3), indexing="ij")
    return ((17 * t + (3 + c) * y + (7 - 2 * c) * x + 50 * c) % 256).to(torch.uint8)


@functools.lru_cache(maxsize=None)
def references(t_in, h, w, kind, flip):
    """(float64 chain, float32 chain's max abs error against it): computed once per case, shared, never written to"""
    f = make_frames(t_in, h, w, kind)
    ref = chain(f, torch.float64, flip)
    yard = float((chain(f, torch.float32, flip).double() - ref).abs().max())
    return ref, yard


def _s():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope="module")
def lib():
    return L.load()


def _kernel(lib, frames, flip):
    """one clip through mq_video_preprocess itself, with a sentinel plane behind the output"""
    import ctypes as C
    t_in, h, w = frames.shape[:3]
    d_frames = frames.to(DEV).contiguous()
    pick = torch.tensor(V.pick_frames(t_in, T), dtype=torch.int32, device=DEV)
    new_h, new_w = V.short_side_scale(h, w, S)
    top, left = V.center_crop(new_h, new_w, S)
    out = torch.full((3 * T + 1, S, S), 7.0, dtype=torch.float32, device=DEV)
    mean, std = (C.c_float * 3)(*V.OPENAI_MEAN), (C.c_float * 3)(*V.OPENAI_STD)
    L.check(lib.mq_video_preprocess(d_frames.data_ptr(), t_in, h, w, pick.data_ptr(), T, S, new_h, new_w, top, left, mean, std, int(flip),
                                    out.data_ptr(), _s()), "mq_video_preprocess")
    torch.cuda.synchronize()
    assert bool((out[3 * T] == 7.0).all())
    return out[:3 * T].cpu().reshape(3, T, S, S)


# ---- 1. the kernel against the chain ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", SHAPES)
def test_kernel_against_the_fp64_chain(lib, h, w):
    worst_yard = worst_err = 0.0
    for t_in in T_INS:
        for kind in ("random", "ramp"):
            for flip in (False, True):
                ref, yard = references(t_in, h, w, kind, flip)
                got = _kernel(lib, make_frames(t_in, h, w, kind), flip)
                err = float((got.double() - ref).abs().max())
                bound = max(4 * yard, FLOOR)
                print(f"VIDEO_FRONTEND {h}x{w} T_in={t_in} {kind} flip={int(flip)} torch_fp32_err={yard:.3e} kernel_err={err:.3e} bound={bound:.3e}")
                assert got.shape == ref.shape and bool(torch.isfinite(got).all())
                assert err <= bound, (h, w, t_in, kind, flip, err, yard)
                worst_yard, worst_err = max(worst_yard, yard), max(worst_err, err)
    print(f"VIDEO_FRONTEND_WORST {h}x{w} torch_fp32_err={worst_yard:.3e} kernel_err={worst_err:.3e}")


def test_identity_scale_is_the_normalised_input_bit_for_bit(lib):
    """32 x 32 at S = 32: every source coordinate is a whole pixel, so the output is (u8 / 255 - mean) / std in float32, exactly"""
    for t_in in T_INS:
        f = make_frames(t_in, 32, 32)
        x = f[torch.from_numpy(np.linspace(0, t_in - 1, T, dtype=int))].permute(3, 0, 1, 2).to(torch.float32) / 255.0
        want = (x - torch.tensor(V.OPENAI_MEAN)[:, None, None, None]) / torch.tensor(V.OPENAI_STD)[:, None, None, None]
        assert torch.equal(_kernel(lib, f, False), want) and torch.equal(_kernel(lib, f, True), want.flip(-1))
        assert torch.equal(chain(f, torch.float32), want)


def test_a_batch_that_mixes_two_frame_sizes(lib):
    """VideoPreprocessor on a list: a host tensor, a device tensor and an ndarray of different sizes and lengths, one flipped"""
    pre = V.VideoPreprocessor(DEV, S, T)
    cases = [(11, 45, 60, True), (8, 64, 107, False), (1, 20, 27, False)]
    clips = [make_frames(*c[:3]) for c in cases]
    out = pre([clips[0], clips[1].to(DEV), {"frames": clips[2].numpy()}], flip=[c[3] for c in cases])["pixel_values"]
    torch.cuda.synchronize()
    assert out.shape == (3, 3, T, S, S) and out.dtype == torch.float32 and out.device.type == "cuda"
    for i, (t_in, h, w, flip) in enumerate(cases):
        ref, yard = references(t_in, h, w, "random", flip)
        err = float((out[i].cpu().double() - ref).abs().max())
        assert err <= max(4 * yard, FLOOR), (i, err, yard)
        assert torch.equal(out[i].cpu(), _kernel(lib, clips[i], flip))                   # the same kernel, whatever shares the call
    same = pre(clips[0], flip=True)["pixel_values"]
    assert torch.equal(same[0], out[0]) and torch.equal(pre([clips[0]])["pixel_values"][0].flip(-1), out[0])


# ---- 2. the controls: each mistake moves the chain by orders of magnitude more than the bound ---------------------------------------------------------
CONTROLS = [("swapped h / w in the scale rule", (45, 60), 11, False, dict(swap_hw=True)),
            ("ceil in place of floor", (45, 60), 11, False, dict(ceil=True)),
            ("round half up in place of half to even", (64, 107), 11, False, dict(half_up=True)),
            ("round half up in place of half to even", (33, 32), 11, False, dict(half_up=True)),
            ("align-corners coordinates", (45, 60), 11, False, dict(align_corners=True)),
            ("align-corners coordinates", (20, 27), 11, False, dict(align_corners=True)),
            ("normalising after the blend with a wrong constant (ImageNet's)", (45, 60), 11, False, dict(late_norm=IMAGENET)),
            ("an off-by-one frame pick", (45, 60), 11, False, dict(pick_shift=1)),
            ("an un-mirrored flip", (45, 60), 11, True, dict(flip=False))]


@pytest.mark.parametrize("what,hw,t_in,flip,mistake", CONTROLS)
def test_controls_are_visible(what, hw, t_in, flip, mistake):
    for kind in ("random", "ramp"):
        ref, yard = references(t_in, hw[0], hw[1], kind, flip)
        bound = max(4 * yard, FLOOR)
        wrong = chain(make_frames(t_in, hw[0], hw[1], kind), torch.float64, **dict(dict(flip=flip), **mistake))
        moved = float((wrong - ref).abs().max())
        print(f"VIDEO_CONTROL {what} {hw[0]}x{hw[1]} {kind}: moved={moved:.3e} bound={bound:.3e} ratio={moved / bound:.1e}")
        assert wrong.shape == ref.shape and moved >= 1000 * bound, (what, kind, moved, bound)


def test_late_normalisation_with_the_right_constant_is_the_same_picture():
    """the control above is about the constant: normalising after the blend is the same linear map (a port may do either)"""
    ref, yard = references(11, 45, 60, "random", False)
    late = chain(make_frames(11, 45, 60), torch.float64, late_norm=(V.OPENAI_MEAN, V.OPENAI_STD))
    assert float((late - ref).abs().max()) <= 1e-12


# ---- 3. end to end ---------------------------------------------------------------------------------------------------------------------------------
def _cos_err(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((1 - (a * b).sum(-1) / (a.norm(dim=-1) * b.norm(dim=-1))).max())


def test_decoded_frames_end_to_end(tmp_path, monkeypatch):
    from marqo_amd.s2_inference import s2_inference as SI
    from marqo_amd.s2_inference.enums import Modality
    monkeypatch.setenv("MARQO_MAX_CUDA_MODEL_MEMORY", "64")
    name = "LanguageBind/Video_V1.5_FT"
    (vcfg, vsd) = LBR.write_model(tmp_path, LBR.SMALL, T=T, image=False, seed=4)["video"]
    props = {"name": name, "dimensions": LBR.SMALL["D"], "type": "languagebind", "loader": "languagebind", "model_size": 1,
             "supported_modalities": ["video", "language"], "video_chunk_length": 20, "audio_chunk_length": 10, "localpath": str(tmp_path)}
    SI.clear_loaded_models()
    try:
        model, _ = SI.load_multimodal_model_and_get_preprocessors(name, dict(props), device=DEV)
        pre = model.preprocessor(Modality.VIDEO)
        assert isinstance(pre, V.VideoPreprocessor) and (pre.size, pre.num_frames) == (LBR.SMALL["S"], T) and model.preprocessor("video") is pre
        assert model.preprocessor(Modality.AUDIO) is None
        a, b = make_frames(30, 45, 60), make_frames(11, 64, 107)
        # one clip of 30 frames: the frames themselves, and their pixel_values, are the same call of the tower
        raw = model.encode(a, Modality.VIDEO)
        px = pre(a)["pixel_values"]
        assert raw.shape == (1, LBR.SMALL["D"]) and np.array_equal(raw, model.encode({"pixel_values": px}, Modality.VIDEO))
        assert np.array_equal(raw, model.encode({"frames": a.numpy()}, Modality.VIDEO))
        # a list of two clips of different sizes, against the CPU chain's pixel_values through the same tower and through the restatement
        both = model.encode([a, b.to(DEV)], Modality.VIDEO)
        cpu_px = torch.stack([chain(a, torch.float32), chain(b, torch.float32)])
        via_chain = model.encode({"pixel_values": cpu_px}, Modality.VIDEO)
        ref = LBR.embed(LBR.video_forward(vsd, vcfg, cpu_px), vsd, "video", True)
        e_chain, e_ref = _cos_err(both, via_chain), _cos_err(both, ref)
        print(f"VIDEO_END_TO_END max(1-cos) against the chain's pixel_values={e_chain:.2e} against the restatement={e_ref:.2e}")
        assert both.shape == (2, LBR.SMALL["D"]) and np.allclose(np.linalg.norm(both, axis=1), 1.0, atol=1e-5)
        assert e_chain <= COS_TOL and e_ref <= COS_TOL
        assert _cos_err(both[:1], raw) <= 1e-6                       # (a call of two clips may take other GEMM kernels than a call of one)
        # vectorise() takes them too; a URL stays the reference's ValueError
        vec = np.asarray(SI.vectorise(name, [a, b], model_properties=dict(props), device=DEV, modality=Modality.VIDEO))
        assert _cos_err(vec, ref) <= COS_TOL
        with pytest.raises(ValueError, match="Unsupported video content type"):
            SI.vectorise(name, ["https://example.com/clip.mp4"], model_properties=dict(props), device=DEV, modality=Modality.VIDEO)
    finally:
        SI.clear_loaded_models()

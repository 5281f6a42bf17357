"""ResNet CLIP image towers on the GPU (csrc/resnet.hip + the GEMMs): each new kernel against torch, whole towers at full depth against an fp32
restatement of OpenAI CLIP's ModifiedResNet (F.conv2d, F.batch_norm, F.avg_pool2d, F.multi_head_attention_forward, composed as the model does),
plus batch / chunk / input-kind consistency and vectorise() end to end."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from marqo_amd import _lib as L
from marqo_amd.engine import archs, synthetic, towers
from marqo_amd.engine.archs import OPENAI_DATASET_MEAN, OPENAI_DATASET_STD
from tests.convtower_ref import _torch_resnet      # the fp32 restatement of ModifiedResNet (it runs on the device of its input)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(autouse=True, scope="module")
def _fp32_reference():
    prev = (torch.backends.cuda.matmul.allow_tf32, torch.backends.cudnn.allow_tf32)
    torch.backends.cuda.matmul.allow_tf32 = torch.backends.cudnn.allow_tf32 = False
    yield
    torch.backends.cuda.matmul.allow_tf32, torch.backends.cudnn.allow_tf32 = prev


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def _cos_err(a, b):
    return float((1 - F.cosine_similarity(a.double().cpu(), b.double().cpu(), dim=-1)).max())


def _bf(t):
    return t.to(torch.bfloat16).float()


# ---- per kernel -------------------------------------------------------------------------------------------------------------------------------
def _conv3x3(x, w, b, Cout, ldy, relu):
    """x bf16 [n, H, W, Cin] on DEV -> bf16 [n H W, ldy] (sentinel-filled, columns >= Cout must come back untouched)"""
    n, H, W, Cin = x.shape
    wk = towers.resnet_conv3x3_weight(w, Cin, Cout).to(torch.bfloat16).to(DEV)
    y = torch.full((n * H * W, ldy), -7.0, dtype=torch.bfloat16, device=DEV)
    L.check(L.load().mq_resnet_conv3x3(x.data_ptr(), wk.data_ptr(), b.data_ptr(), y.data_ptr(), ldy, n, H, W, Cin, Cout, relu, _stream()))
    return y


@pytest.mark.parametrize("Cin,Cout,H", [(32, 32, 56), (40, 40, 14), (48, 48, 7), (64, 64, 56), (256, 256, 14), (1024, 1024, 7), (40, 128, 9),
                                        (1024, 256, 9), (48, 1024, 9), (256, 40, 7), (64, 48, 14), (1024, 64, 56)])
@pytest.mark.parametrize("relu", [1, 0])
def test_conv3x3_matches_conv2d(Cin, Cout, H, relu):
    g = torch.Generator().manual_seed(Cin * 7 + Cout + H)
    n = 3 if H < 56 else 2
    x = torch.randn(n, H, H, Cin, generator=g)
    x[1] += 50.0                           # a loud neighbour: any halo read across the image boundary shows up in images 0 and 2
    x = x.to(torch.bfloat16)
    w = _bf(torch.randn(Cout, Cin, 3, 3, generator=g) / (3 * Cin ** 0.5))
    b = (0.1 * torch.randn(Cout, generator=g)).to(DEV)
    ldy = Cout + 8
    y = _conv3x3(x.to(DEV), w, b, Cout, ldy, relu)
    ref = F.conv2d(x.double().permute(0, 3, 1, 2).to(DEV), w.double().to(DEV), b.double(), padding=1).permute(0, 2, 3, 1)
    if relu:
        ref = ref.clamp_min(0)
    out = y.float().reshape(n, H, H, ldy)
    assert bool((out[..., Cout:] == -7.0).all()), "columns past Cout were written"
    for i in range(n):
        scale = float(ref[i].abs().max())
        err = (out[i, ..., :Cout].double() - ref[i]).abs()
        bound = 2 ** -8 * ref[i].abs() + 2e-3 * scale
        assert bool((err <= bound).all()), f"image {i}: {int((err > bound).sum())} of {err.numel()} out of bound, max err {float(err.max()):.3g}"


def test_conv3x3_above_2g_bytes_of_activation():
    # 336 images of 224 x 224 x 64: the input (and the output) span 2.16e9 bytes; the last image must equal a call on it alone
    n, H, Cin, Cout = 336, 224, 64, 64
    g = torch.Generator().manual_seed(1)
    x = torch.empty(n, H, H, Cin, dtype=torch.bfloat16, device=DEV)
    x[:] = torch.randn(H, H, Cin, generator=g).to(torch.bfloat16).to(DEV)
    x[-1] = torch.randn(H, H, Cin, generator=g).to(torch.bfloat16).to(DEV)
    assert x.numel() * 2 > 2 ** 31
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / 24
    b = (0.1 * torch.randn(Cout, generator=g)).to(DEV)
    big = _conv3x3(x, w, b, Cout, Cout, 1)
    last = big[-H * H:].clone()
    del big
    one = _conv3x3(x[-1:].clone(), w, b, Cout, Cout, 1)
    assert torch.equal(last, one)


@pytest.mark.parametrize("M", [3, 50, 1000])
def test_gemm_relu_epilogues(M):
    lib = L.load()
    g = torch.Generator().manual_seed(M)
    N, K = 192, 256
    A = torch.randn(M, K, generator=g).to(torch.bfloat16).to(DEV)
    Wt = (torch.randn(N, K, generator=g) / 16).to(torch.bfloat16).to(DEV)
    bias = (0.1 * torch.randn(N, generator=g)).to(DEV)
    res = torch.randn(M, N, generator=g).to(torch.bfloat16).to(DEV)
    lin = A.double() @ Wt.double().t() + bias.double()
    out = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    L.check(lib.mq_gemm_bf16(A.data_ptr(), K, Wt.data_ptr(), K, bias.data_ptr(), None, out.data_ptr(), N, M, N, K, L.MQ_EPI_BIAS | L.MQ_EPI_RELU, _stream()))
    torch.testing.assert_close(out.double(), lin.clamp_min(0), rtol=2 ** -8, atol=2e-3)
    assert bool((out >= 0).all())
    out2 = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    L.check(lib.mq_gemm_bf16(A.data_ptr(), K, Wt.data_ptr(), K, bias.data_ptr(), res.data_ptr(), out2.data_ptr(), N, M, N, K,
                             L.MQ_EPI_BIAS | L.MQ_EPI_RESIDUAL | L.MQ_EPI_RELU, _stream()))
    torch.testing.assert_close(out2.double(), (lin + res.double()).clamp_min(0), rtol=2 ** -8, atol=4e-3)   # ReLU after the residual add


def _pixels(u8):
    mean = torch.tensor(OPENAI_DATASET_MEAN, device=DEV).view(1, 3, 1, 1)
    std = torch.tensor(OPENAI_DATASET_STD, device=DEV).view(1, 3, 1, 1)
    return (u8.to(DEV).permute(0, 3, 1, 2).float() / 255.0 - mean) / std


@pytest.mark.parametrize("S", [224, 36])
def test_stem_gather_u8_and_f32(S):
    lib = L.load()
    n = 3
    u8 = synthetic.natural_images_u8(n, S, S, seed=S).to(DEV)
    px = _pixels(u8)
    xp = F.pad(px, (1, 1, 1, 1))
    G = S // 2
    ref = torch.zeros(n, G, G, 64, device=DEV)
    for ky in range(3):
        for kx in range(3):
            t = ky * 3 + kx
            ref[..., 3 * t:3 * t + 3] = xp[:, :, ky:ky + S:2, kx:kx + S:2].permute(0, 2, 3, 1)
    mean, std = (ctypes.c_float * 3)(*OPENAI_DATASET_MEAN), (ctypes.c_float * 3)(*OPENAI_DATASET_STD)
    for is_u8, src in ((1, u8), (0, px.contiguous())):
        out = torch.full((n * G * G, 64), 9.0, dtype=torch.bfloat16, device=DEV)
        L.check(lib.mq_resnet_stem_gather(src.data_ptr(), is_u8, out.data_ptr(), n, S, ctypes.addressof(mean), ctypes.addressof(std), _stream()))
        torch.testing.assert_close(out.float(), ref.reshape(-1, 64), rtol=2 ** -8, atol=1e-6)


@pytest.mark.parametrize("C,H", [(64, 112), (256, 56), (2048, 14), (40, 10)])
def test_avgpool2_matches_torch(C, H):
    lib = L.load()
    g = torch.Generator().manual_seed(C + H)
    n = 3
    x = torch.randn(n, H, H, C, generator=g).to(torch.bfloat16).to(DEV)
    out = torch.empty(n * (H // 2) ** 2, C, dtype=torch.bfloat16, device=DEV)
    L.check(lib.mq_resnet_avgpool2(x.data_ptr(), out.data_ptr(), n, H, H, C, _stream()))
    ref = F.avg_pool2d(x.float().permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1).reshape(-1, C)
    torch.testing.assert_close(out.float(), ref, rtol=2 ** -8, atol=1e-6)


@pytest.mark.parametrize("C,HW", [(2048, 49), (2560, 81), (3072, 144), (4096, 196)])
def test_attnpool_tokens_and_attend_match_torch(C, HW):
    lib = L.load()
    g = torch.Generator().manual_seed(HW)
    n, T = 3, HW + 1
    x = torch.randn(n, HW, C, generator=g).to(torch.bfloat16).to(DEV)
    pos = (torch.randn(T, C, generator=g) / C ** 0.5).to(DEV)
    tok = torch.empty(n, T, C, dtype=torch.bfloat16, device=DEV)
    L.check(lib.mq_resnet_attnpool_tokens(x.data_ptr(), pos.data_ptr(), tok.data_ptr(), n, HW, C, _stream()))
    ref_tok = torch.cat([x.float().mean(1, keepdim=True), x.float()], 1) + pos
    torch.testing.assert_close(tok.float(), ref_tok, rtol=2 ** -8, atol=1e-5)
    q = (torch.randn(n, C, generator=g) / 4).to(torch.bfloat16).to(DEV)
    kv = torch.randn(n, T, 2 * C, generator=g).to(torch.bfloat16).to(DEV)
    out = torch.empty(n, C, dtype=torch.bfloat16, device=DEV)
    L.check(lib.mq_resnet_attnpool_attend(q.data_ptr(), kv.data_ptr(), out.data_ptr(), n, T, C, _stream()))
    H = C // 64
    qh = q.double().view(n, H, 1, 64)
    kh = kv[..., :C].double().view(n, T, H, 64).transpose(1, 2)
    vh = kv[..., C:].double().view(n, T, H, 64).transpose(1, 2)
    ref = (torch.softmax(qh @ kh.transpose(-1, -2), -1) @ vh).reshape(n, C)
    torch.testing.assert_close(out.double(), ref, rtol=2 ** -7, atol=2e-3)


# ---- the fp32 restatement of ModifiedResNet ---------------------------------------------------------------------------------------------------
def _bf16_exact_state_dict(sd):
    """the synthetic checkpoint made exactly representable on the tower's path: every convolution and attention-pool projection weight rounded
    to bf16, and every BatchNorm scale gamma / sqrt(var + eps) moved to the nearest power of two (gamma adjusted), so that the load-time fold
    w * scale rounds to bf16 without error.  The fp32 restatement then sees the very weights the tower multiplies with, and what is left between
    the two is the rounding of the activations — small against what differs between images, unlike the weight rounding, which shifts every
    image alike and hides errors in the image-dependent part"""
    out = dict(sd)
    for k, t in sd.items():
        if k.endswith(".running_var"):
            b = k[: -len("running_var")]
            std = torch.sqrt(t.double() + 1e-5)
            s = torch.exp2(torch.round(torch.log2(sd[b + "weight"].double() / std)))
            out[b + "weight"] = (s * std).float()
        elif k.endswith(".weight") and (t.ndim == 4 or ".attnpool." in k):
            out[k] = t.to(torch.bfloat16).float()
    return out


def _tower_errors(out, ref):
    """(max(1 - cos), max |out - ref| / min |ref - batch mean|): the second ratio measures the error against what differs between the images"""
    rel = float((out - ref).norm(dim=-1).max() / (ref - ref.mean(0, keepdim=True)).norm(dim=-1).min())
    return _cos_err(out, ref), rel


_CACHE = {}


def _tower(name):
    if name not in _CACHE:
        _CACHE.clear()
        torch.cuda.empty_cache()
        v, _ = archs.resolve_resnet_clip(name)
        sd = _bf16_exact_state_dict(synthetic.random_open_clip_state_dict(vision=v, text=None, seed=3))
        _CACHE[name] = (v, sd, towers.ResNetTower(v, sd, DEV))
    return _CACHE[name]


# the error against the between-image spread, measured on an MI355X with the bf16-exact weights: 0.06-0.26 for RN50 ... RN50x16; the errors
# that max(1 - cos) <= 5e-4 lets through measure 0.65-0.67 (positions left out), 1.07-32 (q_proj without the 64^-0.5 scale) and 2.0-2.2 (two
# images' outputs swapped) on RN50 / RN50x4 (profiles/r10a_resnet_gpu_tests.txt)
REL_BOUND = 0.4


# ---- full-depth towers ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n", [("RN50", 4), ("RN101", 3), ("RN50x4", 2), ("RN50x16", 2)])
def test_full_tower_matches_fp32_reference(name, n):
    v, sd, tw = _tower(name)
    u8 = synthetic.natural_images_u8(n, v.image_size, v.image_size, seed=7).to(DEV)
    out = tw.encode_u8(u8, normalize=False)
    with torch.no_grad():
        ref = _torch_resnet(sd, v, _pixels(u8))
    err, rel = _tower_errors(out, ref)
    # (random-init towers map every image close to one common direction, so max(1 - cos) alone cannot tell a wrong attention temperature or
    # missing positions from rounding; the error against the between-image spread can)
    print(f"{name}: max(1 - cos) vs fp32 = {err:.2e}, max |out - ref| / min |ref - batch mean| = {rel:.2e}")
    assert err <= 5e-4
    assert rel <= REL_BOUND
    normed = tw.encode_u8(u8)
    torch.testing.assert_close(normed, F.normalize(out, dim=-1), rtol=1e-5, atol=1e-6)


# ---- consistency ----------------------------------------------------------------------------------------------------------------------------------
def test_f32_input_equals_u8_input():
    v, sd, tw = _tower("RN50")
    u8 = synthetic.natural_images_u8(3, v.image_size, v.image_size, seed=11).to(DEV)
    assert torch.equal(tw.encode_u8(u8), tw.encode_f32(_pixels(u8)))


def test_one_image_alone_equals_it_inside_a_batch_of_64(tiled_gemm_only):
    v, sd, tw = _tower("RN50")
    u8 = synthetic.natural_images_u8(64, v.image_size, v.image_size, seed=12).to(DEV)
    batch = tw.encode_u8(u8)
    for i in (0, 37, 63):
        assert torch.equal(tw.encode_u8(u8[i:i + 1])[0], batch[i])


def test_chunked_calls_equal_one_call(tiled_gemm_only):
    v, sd, tw = _tower("RN50")
    per_image = L.load().mq_resnet_workspace_bytes(ctypes.byref(tw.cfg), 1)
    small = towers.ResNetTower(v, sd, DEV, max_workspace_bytes=int(2.5 * per_image))
    assert small.max_images_per_call == 2
    u8 = synthetic.natural_images_u8(5, v.image_size, v.image_size, seed=13).to(DEV)
    assert torch.equal(small.encode_u8(u8), tw.encode_u8(u8))


def test_fp8_is_refused():
    v, sd, _ = _tower("RN50")
    with pytest.raises(ValueError, match="bf16 only"):
        towers.ResNetTower(v, sd, DEV, precision="fp8")


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dims,S", [("RN50", 1024, 224), ("open_clip/RN50x4/openai", 640, 288)])
def test_vectorise_resnet_end_to_end(tmp_path, name, dims, S):
    from PIL import Image
    _CACHE.clear()
    torch.cuda.empty_cache()
    os.environ["MARQO_AMD_MODEL_DIR"] = str(tmp_path)
    os.environ["MARQO_AMD_SYNTHETIC_WEIGHTS"] = "1"
    from marqo_amd.s2_inference import s2_inference as s2i
    try:
        s2i.clear_loaded_models()
        rng = np.random.default_rng(3)
        pil = [Image.fromarray(rng.integers(0, 256, (300, 260, 3), dtype=np.uint8)), Image.fromarray(rng.integers(0, 256, (S, S, 3), dtype=np.uint8))]
        img = np.asarray(s2i.vectorise(name, pil, device=DEV, modality=s2i.Modality.IMAGE))
        txt = np.asarray(s2i.vectorise(name, ["a photo of a cat", "a dog"], device=DEV))
        assert img.shape == (2, dims) and txt.shape == (2, dims)
        assert np.allclose(np.linalg.norm(img, axis=1), 1, atol=1e-5) and np.allclose(np.linalg.norm(txt, axis=1), 1, atol=1e-5)
        key = s2i._create_model_cache_key(name, DEV, s2i.get_model_properties_from_registry(name))
        m = s2i.get_available_models()[key]["model"]
        assert isinstance(m.vision, towers.ResNetTower)
        assert m.text_arch.quick_gelu                      # OpenAI checkpoints: QuickGELU text tower
        px = torch.stack([m.preprocess(p) for p in pil]).to(DEV)
        assert tuple(px.shape) == (2, 3, S, S)
        tower_rows = m.vision.encode_f32(px).cpu().numpy()
        assert float(np.abs(img - tower_rows).max()) <= 1e-4
    finally:
        s2i.clear_loaded_models()
        os.environ.pop("MARQO_AMD_SYNTHETIC_WEIGHTS", None)
        os.environ.pop("MARQO_AMD_MODEL_DIR", None)

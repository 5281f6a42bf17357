"""ConvNeXt CLIP image towers on the GPU (csrc/convnext.hip + the GEMMs): each new kernel against torch, whole trunks + heads against an fp32
reference — transformers' ConvNextModel with the timm weights mapped onto its names (eps 1e-6), and for the 1e-5 xxlarge a short torch restatement
that is itself cross-checked against ConvNextModel — plus batch / chunk / input-kind consistency and vectorise() end to end."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from marqo_amd import _lib as L
from marqo_amd.engine import archs, synthetic, towers
from marqo_amd.engine.archs import OPENAI_DATASET_MEAN, OPENAI_DATASET_STD
from tests.convtower_ref import _head, _torch_trunk      # the fp32 restatements (they run on the device of their input)

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


# ---- per kernel -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,H", [(128, 7), (128, 80), (1536, 10), (1536, 16), (3072, 7), (3072, 10), (3072, 16), (128, 16)])
def test_dwconv_matches_conv2d_and_its_partials_finalise_to_row_stats(C, H):
    lib = L.load()
    g = torch.Generator().manual_seed(C + H)
    n = 1 if H > 40 else 2
    x = torch.randn(n, H, H, C, generator=g).to(torch.bfloat16).to(DEV)
    w = (torch.randn(C, 1, 7, 7, generator=g) / 7).to(DEV)
    b = (0.1 * torch.randn(C, generator=g)).to(DEV)
    taps = towers.convnext_dw_taps(w.cpu()).to(DEV)
    y = torch.empty_like(x)
    rows = n * H * H
    part = torch.full((C // 64, rows, 2), float("nan"), device=DEV)
    L.check(lib.mq_convnext_dwconv(x.data_ptr(), taps.data_ptr(), b.data_ptr(), y.data_ptr(), part.data_ptr(), n, H, H, C, _stream()))
    ref = F.conv2d(x.float().permute(0, 3, 1, 2), w, b, padding=3, groups=C).permute(0, 2, 3, 1)
    torch.testing.assert_close(y.float(), ref, rtol=2 ** -8, atol=1e-4)     # within the bf16 rounding of the stored values
    eps = 1e-6
    st = torch.empty(rows, 2, device=DEV)
    L.check(lib.mq_row_stats_finalize(part.data_ptr(), C // 64, st.data_ptr(), rows, C, eps, _stream()))
    if C <= 2048:
        st_ref = torch.empty(rows, 2, device=DEV)
        L.check(lib.mq_row_stats(y.data_ptr(), st_ref.data_ptr(), rows, C, eps, _stream()))
    else:
        yf = y.float().reshape(rows, C)
        st_ref = torch.stack([yf.mean(1), torch.rsqrt(yf.var(1, unbiased=False) + eps)], 1)
    torch.testing.assert_close(st, st_ref, rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("C,H", [(128, 64), (384, 20), (1536, 16)])
def test_downsample_gather_matches_torch(C, H):
    lib = L.load()
    g = torch.Generator().manual_seed(C)
    n, eps = 2, 1e-6
    x = (0.5 + torch.randn(n, H, H, C, generator=g)).to(torch.bfloat16).to(DEV)
    lg, lb = (1 + 0.1 * torch.randn(C, generator=g)).to(DEV), (0.1 * torch.randn(C, generator=g)).to(DEV)
    rows = n * H * H
    st = torch.empty(rows, 2, device=DEV)
    L.check(lib.mq_row_stats(x.data_ptr(), st.data_ptr(), rows, C, eps, _stream()))
    out = torch.empty(rows // 4, 4 * C, dtype=torch.bfloat16, device=DEV)
    L.check(lib.mq_convnext_downsample(x.data_ptr(), st.data_ptr(), lg.data_ptr(), lb.data_ptr(), out.data_ptr(), n, H, H, C, _stream()))
    ref = towers.convnext_downsample_gather(F.layer_norm(x.float(), (C,), lg, lb, eps))
    torch.testing.assert_close(out.float(), ref, rtol=2 ** -8, atol=2e-3)


@pytest.mark.parametrize("C,HW", [(1024, 49), (1536, 100), (3072, 64)])
def test_pool_ln_matches_torch(C, HW):
    lib = L.load()
    g = torch.Generator().manual_seed(HW)
    n, eps = 3, 1e-5
    x = (0.3 + torch.randn(n, HW, C, generator=g)).to(torch.bfloat16).to(DEV)
    lg, lb = (1 + 0.1 * torch.randn(C, generator=g)).to(DEV), (0.1 * torch.randn(C, generator=g)).to(DEV)
    of = torch.empty(n, C, device=DEV)
    ob = torch.empty(n, C, dtype=torch.bfloat16, device=DEV)
    L.check(lib.mq_convnext_pool_ln(x.data_ptr(), lg.data_ptr(), lb.data_ptr(), ob.data_ptr(), of.data_ptr(), n, HW, C, eps, _stream()))
    ref = F.layer_norm(x.float().mean(1), (C,), lg, lb, eps)
    torch.testing.assert_close(of, ref, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(ob.float(), ref, rtol=2 ** -8, atol=1e-4)


# ---- fp32 references ------------------------------------------------------------------------------------------------------------------------------
def _hf_convnext(sd, arch):
    """transformers' ConvNextModel in fp32 with the timm trunk's weights mapped onto its names (its LayerNorms inside the trunk use eps 1e-6)"""
    from transformers import ConvNextConfig, ConvNextModel
    cfg = ConvNextConfig(num_channels=3, patch_size=4, num_stages=4, hidden_sizes=list(arch.dims), depths=list(arch.depths), hidden_act="gelu",
                         layer_norm_eps=arch.ln_eps, layer_scale_init_value=1.0, drop_path_rate=0.0)
    m = ConvNextModel(cfg).eval()
    t, mapped = "visual.trunk.", {}
    for k, v in sd.items():
        if not k.startswith(t):
            continue
        k = k[len(t):]
        k = k.replace("stem.0.", "embeddings.patch_embeddings.").replace("stem.1.", "embeddings.layernorm.").replace("head.norm.", "layernorm.")
        k = k.replace("stages.", "encoder.stages.").replace(".downsample.", ".downsampling_layer.").replace(".blocks.", ".layers.")
        k = k.replace(".conv_dw.", ".dwconv.").replace(".norm.", ".layernorm.").replace(".mlp.fc1.", ".pwconv1.").replace(".mlp.fc2.", ".pwconv2.")
        k = k.replace(".gamma", ".layer_scale_parameter")
        mapped[k] = v
    m.load_state_dict(mapped, strict=True)
    return m.to(DEV)


def _pixels(u8):
    mean = torch.tensor(OPENAI_DATASET_MEAN, device=DEV).view(1, 3, 1, 1)
    std = torch.tensor(OPENAI_DATASET_STD, device=DEV).view(1, 3, 1, 1)
    return (u8.to(DEV).permute(0, 3, 1, 2).float() / 255.0 - mean) / std


_CACHE = {}


def _tower(name):
    if name not in _CACHE:
        _CACHE.clear()
        torch.cuda.empty_cache()
        v, _ = archs.resolve_open_clip(name)
        sd = synthetic.random_open_clip_state_dict(vision=v, text=None, seed=3)
        _CACHE[name] = (v, sd, towers.ConvNextTower(v, sd, DEV))
    return _CACHE[name]


# ---- full-depth trunks + heads ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n", [("convnext_base_w", 4), ("convnext_large_d_320", 3), ("convnext_xxlarge", 2)])
def test_full_tower_matches_fp32_reference(name, n):
    v, sd, tw = _tower(name)
    u8 = synthetic.natural_images_u8(n, v.image_size, v.image_size, seed=7).to(DEV)
    out = tw.encode_u8(u8, normalize=False)
    x = _pixels(u8)
    with torch.no_grad():
        if v.ln_eps == 1e-6:
            m = _hf_convnext(sd, v)
            pooled = m(pixel_values=x).pooler_output
            del m
        else:
            pooled = _torch_trunk(sd, v, x)
        ref = _head(sd, v, pooled)
    err = _cos_err(out, ref)
    print(f"{name}: max(1 - cos) vs fp32 = {err:.2e}")
    assert err <= 1e-3
    normed = tw.encode_u8(u8)
    torch.testing.assert_close(normed, F.normalize(out, dim=-1), rtol=1e-5, atol=1e-6)


def test_torch_restatement_matches_hf_convnext():
    # the restatement that checks the 1e-5 tower, itself checked against ConvNextModel where both take eps 1e-6 (a shallow base-width trunk)
    v = archs.ConvNextArch(64, (1, 1, 2, 1), (128, 256, 512, 1024), 1e-6, "linear", 512)
    sd = synthetic.random_open_clip_state_dict(vision=v, text=None, seed=5)
    x = _pixels(synthetic.natural_images_u8(2, 64, 64, seed=1))
    with torch.no_grad():
        a = _torch_trunk(sd, v, x)
        b = _hf_convnext(sd, v)(pixel_values=x).pooler_output
    torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-4)


# ---- consistency ----------------------------------------------------------------------------------------------------------------------------------
def test_f32_input_equals_u8_input():
    v, sd, tw = _tower("convnext_base_w")
    u8 = synthetic.natural_images_u8(3, v.image_size, v.image_size, seed=11).to(DEV)
    a = tw.encode_u8(u8)
    b = tw.encode_f32(_pixels(u8))
    assert float((a - b).abs().max()) <= 1e-5


def test_one_image_alone_equals_it_inside_a_batch_of_64(tiled_gemm_only):
    # (with the tiled GEMM family on every call: a one-image call's stage-3 and head GEMMs of <= 80 rows would otherwise take the skinny
    # kernels, whose k-summation order differs — bounded in the next test)
    v, sd, tw = _tower("convnext_base_w")
    u8 = synthetic.natural_images_u8(64, v.image_size, v.image_size, seed=12).to(DEV)
    batch = tw.encode_u8(u8)
    for i in (0, 37):
        one = tw.encode_u8(u8[i:i + 1])
        assert float((one[0] - batch[i]).abs().max()) <= 1e-4


def test_one_image_through_the_skinny_gemms_stays_close_to_the_batch():
    v, sd, tw = _tower("convnext_base_w")
    u8 = synthetic.natural_images_u8(64, v.image_size, v.image_size, seed=12).to(DEV)
    batch = tw.encode_u8(u8)
    for i in (0, 37):
        assert _cos_err(tw.encode_u8(u8[i:i + 1]), batch[i:i + 1]) <= 1e-5


def test_chunked_calls_equal_one_call(tiled_gemm_only):   # (its last chunk is one image: see the batch-of-64 test)
    v, sd, tw = _tower("convnext_base_w")
    per_image = L.load().mq_convnext_workspace_bytes(ctypes.byref(tw.cfg), 1)
    small = towers.ConvNextTower(v, sd, DEV, max_workspace_bytes=int(2.5 * per_image))
    assert small.max_images_per_call == 2
    u8 = synthetic.natural_images_u8(5, v.image_size, v.image_size, seed=13).to(DEV)
    assert float((small.encode_u8(u8) - tw.encode_u8(u8)).abs().max()) <= 1e-4


def test_fp8_is_refused():
    v, sd, _ = _tower("convnext_base_w")
    with pytest.raises(ValueError, match="bf16 only"):
        towers.ConvNextTower(v, sd, DEV, precision="fp8")


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------------
def test_vectorise_convnext_end_to_end(tmp_path):
    from PIL import Image
    _CACHE.clear()
    torch.cuda.empty_cache()
    os.environ["MARQO_AMD_MODEL_DIR"] = str(tmp_path)
    os.environ["MARQO_AMD_SYNTHETIC_WEIGHTS"] = "1"
    from marqo_amd.s2_inference import s2_inference as s2i
    try:
        s2i.clear_loaded_models()
        name = "open_clip/convnext_base_w/laion2b_s13b_b82k"
        rng = np.random.default_rng(3)
        pil = [Image.fromarray(rng.integers(0, 256, (300, 260, 3), dtype=np.uint8)), Image.fromarray(rng.integers(0, 256, (256, 256, 3), dtype=np.uint8))]
        img = np.asarray(s2i.vectorise(name, pil, device=DEV, modality=s2i.Modality.IMAGE))
        txt = np.asarray(s2i.vectorise(name, ["a photo of a cat", "a dog"], device=DEV))
        assert img.shape == (2, 640) and txt.shape == (2, 640)
        assert np.allclose(np.linalg.norm(img, axis=1), 1, atol=1e-5) and np.allclose(np.linalg.norm(txt, axis=1), 1, atol=1e-5)
        key = s2i._create_model_cache_key(name, DEV, s2i.get_model_properties_from_registry(name))
        m = s2i.get_available_models()[key]["model"]
        assert isinstance(m.vision, towers.ConvNextTower)
        px = torch.stack([m.preprocess(p) for p in pil]).to(DEV)
        assert tuple(px.shape) == (2, 3, 256, 256)
        tower_rows = m.vision.encode_f32(px).cpu().numpy()
        assert float(np.abs(img - tower_rows).max()) <= 1e-4
    finally:
        s2i.clear_loaded_models()
        os.environ.pop("MARQO_AMD_SYNTHETIC_WEIGHTS", None)
        os.environ.pop("MARQO_AMD_MODEL_DIR", None)

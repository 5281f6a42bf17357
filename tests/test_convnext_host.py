"""ConvNeXt CLIP towers, host side (no GPU): architecture table, registry names, synthetic checkpoint names, the load-time folds against the
unfolded fp32 computation, the hf-hub config resolution, and the compiled ISA of csrc/convnext.hip."""
import json
import os
import subprocess

import pytest
import torch
import torch.nn.functional as F

from marqo_amd.engine import archs, synthetic, towers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

# arch -> (image, depths, dims, eps, head, embed, (text width, heads, layers))
TABLE = {
    "convnext_base": (224, (3, 3, 27, 3), (128, 256, 512, 1024), 1e-6, "linear", 512, (512, 8, 12)),
    "convnext_base_w": (256, (3, 3, 27, 3), (128, 256, 512, 1024), 1e-6, "linear", 640, (640, 10, 12)),
    "convnext_base_w_320": (320, (3, 3, 27, 3), (128, 256, 512, 1024), 1e-6, "linear", 640, (640, 10, 12)),
    "convnext_large_d": (256, (3, 3, 27, 3), (192, 384, 768, 1536), 1e-6, "mlp", 768, (768, 12, 16)),
    "convnext_large_d_320": (320, (3, 3, 27, 3), (192, 384, 768, 1536), 1e-6, "mlp", 768, (768, 12, 16)),
    "convnext_xxlarge": (256, (3, 4, 30, 3), (384, 768, 1536, 3072), 1e-5, "linear", 1024, (1024, 16, 24)),
}

REGISTRY = {
    "open_clip/convnext_base/laion400m_s13b_b51k": 512,
    "open_clip/convnext_base_w/laion2b_s13b_b82k": 640,
    "open_clip/convnext_base_w/laion2b_s13b_b82k_augreg": 640,
    "open_clip/convnext_base_w/laion_aesthetic_s13b_b82k": 640,
    "open_clip/convnext_base_w_320/laion_aesthetic_s13b_b82k": 640,
    "open_clip/convnext_base_w_320/laion_aesthetic_s13b_b82k_augreg": 640,
    "open_clip/convnext_large_d/laion2b_s26b_b102k_augreg": 768,
    "open_clip/convnext_large_d_320/laion2b_s29b_b131k_ft": 768,
    "open_clip/convnext_large_d_320/laion2b_s29b_b131k_ft_soup": 768,
    "open_clip/convnext_xxlarge/laion2b_s34b_b82k_augreg": 1024,
    "open_clip/convnext_xxlarge/laion2b_s34b_b82k_augreg_rewind": 1024,
    "open_clip/convnext_xxlarge/laion2b_s34b_b82k_augreg_soup": 1024,
}


@pytest.mark.parametrize("name", sorted(TABLE))
def test_resolve_open_clip_convnext(name):
    S, depths, dims, eps, head, E, (tw, th, tl) = TABLE[name]
    v, t = archs.resolve_open_clip(name, "laion2b_s13b_b82k")
    assert isinstance(v, archs.ConvNextArch)
    assert (v.image_size, v.depths, v.dims, v.ln_eps, v.head, v.out_dim) == (S, depths, dims, eps, head, E)
    assert v.preprocessor is None and v.pool != "map"          # the loader picks the OpenCLIP transform
    assert (t.width, t.heads, t.layers, t.out_dim, t.mlp_dim, t.vocab, t.ctx) == (tw, th, tl, E, 4 * tw, 49408, 77)
    assert not t.quick_gelu and t.causal and t.prefix == ""
    assert v.gflop_per_image > 25


def test_resnet_stays_unsupported():
    with pytest.raises(KeyError):
        archs.resolve_open_clip("RN50")
    with pytest.raises(KeyError):
        archs.resolve_open_clip("RN50", "openai")


def test_gflop_per_image_matches_the_issue_table():
    # GEMM FLOPs + depthwise FLOPs per image (the depthwise part is 2 * 49 per output element)
    for name, total in (("convnext_base", 30.3 + 0.46), ("convnext_base_w", 39.5 + 0.60), ("convnext_large_d_320", 139 + 1.4),
                        ("convnext_xxlarge", 394 + 2.0)):
        assert archs.resolve_open_clip(name)[0].gflop_per_image == pytest.approx(total, rel=0.01)


def test_registry_has_the_twelve_convnext_names():
    from marqo_amd.s2_inference.model_registry import load_model_properties
    models = load_model_properties()["models"]
    for name, dims in REGISTRY.items():
        assert name in models, name
        p = models[name]
        assert p["dimensions"] == dims and p["type"] == "open_clip" and p["pretrained"] == name.split("/")[2]


def _expected_keys(arch):
    t, dims = "visual.trunk.", arch.dims
    keys = {t + "stem.0.weight": (dims[0], 3, 4, 4), t + "stem.0.bias": (dims[0],), t + "stem.1.weight": (dims[0],), t + "stem.1.bias": (dims[0],),
            t + "head.norm.weight": (dims[3],), t + "head.norm.bias": (dims[3],)}
    for i, (depth, C) in enumerate(zip(arch.depths, dims)):
        p = f"{t}stages.{i}."
        if i > 0:
            Cp = dims[i - 1]
            keys.update({p + "downsample.0.weight": (Cp,), p + "downsample.0.bias": (Cp,), p + "downsample.1.weight": (C, Cp, 2, 2),
                         p + "downsample.1.bias": (C,)})
        for j in range(depth):
            b = f"{p}blocks.{j}."
            keys.update({b + "conv_dw.weight": (C, 1, 7, 7), b + "conv_dw.bias": (C,), b + "norm.weight": (C,), b + "norm.bias": (C,),
                         b + "mlp.fc1.weight": (4 * C, C), b + "mlp.fc1.bias": (4 * C,), b + "mlp.fc2.weight": (C, 4 * C), b + "mlp.fc2.bias": (C,),
                         b + "gamma": (C,)})
    E = arch.out_dim
    if arch.head == "linear":
        keys["visual.head.proj.weight"] = (E, dims[3])
    else:
        keys.update({"visual.head.mlp.fc1.weight": (2 * E, dims[3]), "visual.head.mlp.fc1.bias": (2 * E,), "visual.head.mlp.fc2.weight": (E, 2 * E)})
    return keys


@pytest.mark.parametrize("name", ["convnext_base_w", "convnext_large_d"])
def test_synthetic_state_dict_has_timm_names(name):
    v, _ = archs.resolve_open_clip(name)
    sd = synthetic.random_open_clip_state_dict(vision=v, text=None, seed=0)
    want = _expected_keys(v)
    assert set(sd) == set(want)
    for k, shape in want.items():
        assert tuple(sd[k].shape) == shape, k
    g = torch.cat([sd[k] for k in sd if k.endswith(".gamma")])
    assert float(g.min()) >= 0.05 and float(g.max()) <= 0.5     # trained-like layer scales, not timm's 1e-6 init


def test_fold_ln_into_fc1_matches_unfolded():
    g = torch.Generator().manual_seed(0)
    C, R, eps = 256, 64, 1e-6
    # bf16-exact weight and power-of-two LayerNorm scales: the bf16 rounding of the folded weight is exact, so the fold must agree with the
    # unfolded fp32 computation to fp32 rounding
    W = torch.randn(4 * C, C, generator=g).to(torch.bfloat16).float() / 16
    b = torch.randn(4 * C, generator=g)
    ln_g = 2.0 ** torch.randint(-2, 3, (C,), generator=g).float()
    ln_b = torch.randn(C, generator=g)
    x = 1.5 + torch.randn(R, C, generator=g)
    ref = F.linear(F.layer_norm(x, (C,), ln_g, ln_b, eps), W, b)
    wf, bf, sf = towers.convnext_fold_ln_fc1(W, b, ln_g, ln_b)
    assert wf.dtype == torch.bfloat16
    mean = x.mean(1, keepdim=True)
    rstd = torch.rsqrt(x.var(1, unbiased=False, keepdim=True) + eps)
    out = rstd * (x @ wf.float().t() - mean * sf) + bf
    torch.testing.assert_close(out, ref, rtol=1e-5, atol=1e-4)


def test_fold_gamma_into_fc2_matches_unfolded():
    g = torch.Generator().manual_seed(1)
    C, R = 128, 32
    W, b, gamma, h = torch.randn(C, 4 * C, generator=g), torch.randn(C, generator=g), torch.rand(C, generator=g), torch.randn(R, 4 * C, generator=g)
    w2, b2 = towers.convnext_fold_gamma_fc2(W, b, gamma)
    torch.testing.assert_close(F.linear(h, w2, b2), gamma * F.linear(h, W, b), rtol=1e-4, atol=1e-4)


def test_downsample_permutation_and_gather_reproduce_strided_conv():
    g = torch.Generator().manual_seed(2)
    n, Cp, C, H = 2, 64, 128, 10
    x = torch.randn(n, Cp, H, H, generator=g)
    w, b = torch.randn(C, Cp, 2, 2, generator=g), torch.randn(C, generator=g)
    ref = F.conv2d(x, w, b, stride=2)                                               # [n, C, H/2, H/2]
    rows = towers.convnext_downsample_gather(x.permute(0, 2, 3, 1).contiguous())     # [n (H/2)^2, 4 Cp]
    out = F.linear(rows, towers.convnext_downsample_weight(w), b).reshape(n, H // 2, H // 2, C).permute(0, 3, 1, 2)
    torch.testing.assert_close(out, ref, rtol=1e-5, atol=1e-4)


def test_dw_taps_layout():
    w = torch.randn(192, 1, 7, 7)
    taps = towers.convnext_dw_taps(w)
    assert taps.shape == (49, 192)
    assert torch.equal(taps[3 * 7 + 5], w[:, 0, 3, 5])


def test_hf_hub_convnext_config_resolves(tmp_path):
    from marqo_amd.s2_inference.errors import InvalidModelPropertiesError
    from marqo_amd.s2_inference.open_clip_model import OPEN_CLIP
    m = object.__new__(OPEN_CLIP)
    cfg = {"model_cfg": {"embed_dim": 768, "vision_cfg": {"timm_model_name": "convnext_large", "timm_model_pretrained": False, "timm_pool": "",
                                                          "timm_proj": "mlp", "timm_drop": 0.0, "timm_drop_path": 0.1, "image_size": 320},
                         "text_cfg": {"context_length": 77, "vocab_size": 49408, "width": 768, "heads": 12, "layers": 16}}}
    (tmp_path / "open_clip_config.json").write_text(json.dumps(cfg))
    v, t = m._resolve_archs("hf-hub:acme/convnext-large-d-320", None, str(tmp_path))
    ref_v, ref_t = archs.resolve_open_clip("convnext_large_d_320")
    assert v == ref_v and t == ref_t
    cfg["model_cfg"]["vision_cfg"].update(timm_model_name="convnext_xxlarge", timm_proj="linear", image_size=256)
    cfg["model_cfg"].update(embed_dim=1024, text_cfg={"context_length": 77, "vocab_size": 49408, "width": 1024, "heads": 16, "layers": 24})
    (tmp_path / "open_clip_config.json").write_text(json.dumps(cfg))
    assert m._resolve_archs("hf-hub:acme/convnext-xxlarge", None, str(tmp_path)) == archs.resolve_open_clip("convnext_xxlarge")
    cfg["model_cfg"]["vision_cfg"]["timm_pool"] = "avg"
    (tmp_path / "open_clip_config.json").write_text(json.dumps(cfg))
    with pytest.raises(InvalidModelPropertiesError):
        m._resolve_archs("hf-hub:acme/convnext-xxlarge", None, str(tmp_path))


def test_convnext_kernels_compile_without_scratch(tmp_path):
    src = os.path.join(ROOT, "marqo_amd", "csrc", "convnext.hip")
    out = tmp_path / "convnext.s"
    res = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wall", "-Wno-unused-function", "-S", "--cuda-device-only",
                          "-o", str(out), src], capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stderr[-3000:]
    isa = out.read_text()
    for k in ("dwconv7_kernel", "ds_gather_kernel", "pool_ln_kernel"):
        assert k in isa
    assert "scratch_" not in isa
    assert "v_pk_fma_f32" in isa            # the depthwise taps accumulate in packed fp32 pairs
    assert "ds_read_b128" in isa            # 16-byte LDS reads of the staged tile

"""ResNet CLIP towers, host side (no GPU): the resolver and its FLOP table, the 18 registry names against the reference registry, the loader's
name mapping, the BatchNorm folds against the unfolded fp32 computation, the synthetic checkpoint names, the C ABI's argument checks and the
compiled ISA of csrc/resnet.hip."""
import ctypes
import json
import os
import re
import subprocess

import pytest
import torch
import torch.nn.functional as F

from marqo_amd.engine import archs, synthetic, towers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

# name -> (image, layers, w, (C, heads, tokens), embed, (text width, heads), GFLOP per image)
TABLE = {
    "RN50": (224, (3, 4, 6, 3), 64, (2048, 32, 50), 1024, (512, 8), 11.6),
    "RN101": (224, (3, 4, 23, 3), 64, (2048, 32, 50), 512, (512, 8), 19.0),
    "RN50x4": (288, (4, 6, 10, 6), 80, (2560, 40, 82), 640, (640, 10), 41.2),
    "RN50x16": (384, (6, 8, 18, 8), 96, (3072, 48, 145), 768, (768, 12), 145.7),
    "RN50x64": (448, (3, 15, 36, 10), 128, (4096, 64, 197), 1024, (1024, 16), 520.3),
}

REGISTRY = ["RN50", "RN101", "RN50x4", "RN50x16", "RN50x64"] + [
    f"open_clip/{a}/{t}" for a, tags in (("RN50", ("openai", "yfcc15m", "cc12m")), ("RN50-quickgelu", ("openai", "yfcc15m", "cc12m")),
                                         ("RN101", ("openai", "yfcc15m")), ("RN101-quickgelu", ("openai", "yfcc15m")), ("RN50x4", ("openai",)),
                                         ("RN50x16", ("openai",)), ("RN50x64", ("openai",))) for t in tags]


@pytest.mark.parametrize("name", sorted(TABLE))
def test_resolve_resnet_clip(name):
    S, layers, w, (C, heads, T), E, (tw, th), gflop = TABLE[name]
    v, t = archs.resolve_resnet_clip(name, "yfcc15m")
    assert isinstance(v, archs.ResNetArch)
    assert (v.image_size, v.layers, v.width, v.out_dim, v.heads, v.tokens) == (S, layers, w, E, heads, T)
    assert 32 * v.width == C and v.preprocessor is None and v.pool != "map"
    assert (t.width, t.heads, t.layers, t.out_dim, t.mlp_dim, t.vocab, t.ctx, t.prefix) == (tw, th, 12, E, 4 * tw, 49408, 77, "")
    assert not t.quick_gelu
    assert v.gflop_per_image == pytest.approx(gflop, abs=0.05)


def test_quickgelu_follows_the_open_clip_rule():
    assert archs.resolve_resnet_clip("RN50", "openai")[1].quick_gelu
    assert archs.resolve_resnet_clip("RN101-quickgelu", "yfcc15m")[1].quick_gelu
    assert not archs.resolve_resnet_clip("RN50", "cc12m")[1].quick_gelu
    with pytest.raises(KeyError):
        archs.resolve_resnet_clip("RN200")
    with pytest.raises(KeyError):                       # ResNet resolves only through its own resolver
        archs.resolve_open_clip("RN50", "openai")
    assert not set(archs.OPENAI_RESNET_NAMES) & set(archs.OPENAI_CLIP_NAMES)


def test_registry_has_the_eighteen_resnet_names_of_the_reference():
    from marqo_amd.s2_inference.model_registry import load_model_properties
    with open(os.path.join(ROOT, "tests", "golden", "ref_host.json"), encoding="utf-8") as f:
        ref = json.load(f)["registry_models"]
    models = load_model_properties()["models"]
    assert len(models) == 204
    for name in REGISTRY:
        assert name in models, name
        ours, theirs = models[name], ref[name]
        assert {"name", "dimensions", "type"} <= set(theirs)
        for field in ("name", "dimensions", "type", "pretrained"):
            assert ours.get(field) == theirs.get(field), (name, field)


def test_clip_and_open_clip_property_mapping(monkeypatch):
    from marqo_amd.s2_inference import open_clip_model as M
    seen = []
    monkeypatch.setattr(M.OPEN_CLIP, "__init__", lambda self, device=None, model_properties=None, model_auth=None: seen.append(model_properties))
    M.CLIP("RN50", device="cuda", embedding_dim=1024)
    M.CLIP("RN50x16", device="cuda", model_properties={"name": "RN50x16", "localpath": "/x.pt", "dimensions": 768})
    assert seen[0]["name"] == "open_clip/RN50/openai" and seen[0]["dimensions"] == 1024 and seen[0]["type"] == "clip"
    assert seen[1]["name"] == "RN50x16-quickgelu"
    m = object.__new__(M.OPEN_CLIP)
    v, t = m._resolve_archs("RN50x4", "openai", None)
    assert isinstance(v, archs.ResNetArch) and v.out_dim == 640 and t.quick_gelu
    v, t = m._resolve_archs("RN101-quickgelu", "yfcc15m", None)
    assert v.layers == (3, 4, 23, 3) and t.quick_gelu


def test_onnx_resnet_names_stay_refused():
    from marqo_amd.s2_inference.errors import InvalidModelPropertiesError
    from marqo_amd.s2_inference.open_clip_model import CLIP_ONNX
    for name in ("onnx32/openai/RN50", "onnx32/open_clip/RN50/openai", "onnx16/open_clip/RN101-quickgelu/yfcc15m"):
        with pytest.raises(InvalidModelPropertiesError):
            CLIP_ONNX(name, device="cuda", embedding_dim=1024)


def _bn_params(C, g):
    return (0.5 + torch.rand(C, generator=g), 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g), 0.5 + torch.rand(C, generator=g))


@pytest.mark.parametrize("k", [1, 3])
def test_bn_fold_matches_conv_then_batch_norm(k):
    g = torch.Generator().manual_seed(k)
    O, I = 48, 40
    w = torch.randn(O, I, k, k, generator=g) / (I * k * k) ** 0.5
    bw, bb, bm, bv = _bn_params(O, g)
    x = torch.randn(2, I, 9, 9, generator=g)
    ref = F.batch_norm(F.conv2d(x, w, padding=k // 2), bm, bv, bw, bb, False, 0.0, 1e-5)
    wf, bf = towers.resnet_fold_bn(w, bw, bb, bm, bv)
    torch.testing.assert_close(F.conv2d(x, wf, bf, padding=k // 2), ref, rtol=1e-5, atol=1e-5)


def test_conv3x3_weight_layout_reproduces_conv2d_as_a_gemm():
    # the (ky, kx, c) columns of the padded weight, against an explicit im2col of the zero-padded NHWC input
    g = torch.Generator().manual_seed(0)
    n, H, Cin, Cout, cin_p, cout_p = 2, 7, 40, 44, 64, 64
    x = torch.randn(n, Cin, H, H, generator=g)
    w, b = torch.randn(Cout, Cin, 3, 3, generator=g), torch.randn(Cout, generator=g)
    wk = towers.resnet_conv3x3_weight(w, cin_p, cout_p)
    assert wk.shape == (cout_p, 9 * cin_p)                    # 576: already a multiple of 64
    xp = F.pad(F.pad(x, (0, 0, 0, 0, 0, cin_p - Cin)).permute(0, 2, 3, 1), (0, 0, 1, 1, 1, 1))
    cols = torch.cat([xp[:, ky:ky + H, kx:kx + H, :] for ky in range(3) for kx in range(3)], -1).reshape(n * H * H, 9 * cin_p)
    out = (cols @ wk.t())[:, :Cout] + b
    torch.testing.assert_close(out, F.conv2d(x, w, b, padding=1).permute(0, 2, 3, 1).reshape(-1, Cout), rtol=1e-4, atol=1e-4)
    assert float(wk[Cout:].abs().max()) == 0.0
    assert towers.resnet_conv3x3_weight(torch.randn(40, 40, 3, 3), 40, 40).shape == (40, 384)   # 360 -> 384 zero columns


def test_stem_weight_layout():
    w = torch.randn(32, 3, 3, 3)
    s = towers.resnet_stem_weight(w)
    assert s.shape == (32, 64) and float(s[:, 27:].abs().max()) == 0.0
    assert torch.equal(s[:, (2 * 3 + 1) * 3 + 2], w[:, 2, 2, 1])


def _attnpool_from_operands(apw, x):
    """the tower's attention pool from its load-time operands, step by step as csrc/resnet.hip runs it (tokens, k | v of all tokens, q of token 0,
    one query per image and head, c_proj) — x [n, HW, C] -> [n, E]"""
    n, HW, C = x.shape
    tok = torch.cat([x.mean(1, keepdim=True), x], 1) + apw["pos"]
    kv = tok @ apw["kv_w"].t() + apw["kv_b"]
    q = tok[:, 0] @ apw["q_w"].t() + apw["q_b"]
    k, v = kv[..., :C].reshape(n, -1, C // 64, 64), kv[..., C:].reshape(n, -1, C // 64, 64)
    p = torch.softmax(torch.einsum("nhd,nthd->nht", q.reshape(n, C // 64, 64), k), -1)
    return torch.einsum("nht,nthd->nhd", p, v).reshape(n, C) @ apw["c_w"].t() + apw["c_b"]


@pytest.mark.parametrize("name", ["RN50", "RN50x4"])
def test_attnpool_operands_reproduce_multi_head_attention(name):
    # the loader's attention-pool operands (q scale folded, k | v stacked, positions) against F.multi_head_attention_forward on the raw weights
    v, _ = archs.resolve_resnet_clip(name)
    sd = synthetic.random_open_clip_state_dict(vision=v, text=None, seed=0)
    C, a = 32 * v.width, "visual.attnpool."
    x = torch.randn(3, v.tokens - 1, C, generator=torch.Generator().manual_seed(1))
    t = x.permute(1, 0, 2)
    t = torch.cat([t.mean(0, keepdim=True), t]) + sd[a + "positional_embedding"][:, None, :]
    ref, _ = F.multi_head_attention_forward(
        query=t[:1], key=t, value=t, embed_dim_to_check=C, num_heads=C // 64, q_proj_weight=sd[a + "q_proj.weight"],
        k_proj_weight=sd[a + "k_proj.weight"], v_proj_weight=sd[a + "v_proj.weight"], in_proj_weight=None,
        in_proj_bias=torch.cat([sd[a + "q_proj.bias"], sd[a + "k_proj.bias"], sd[a + "v_proj.bias"]]), bias_k=None, bias_v=None,
        add_zero_attn=False, dropout_p=0.0, out_proj_weight=sd[a + "c_proj.weight"], out_proj_bias=sd[a + "c_proj.bias"],
        use_separate_proj_weight=True, training=False, need_weights=False)
    apw = towers.resnet_attnpool_weights(sd, v)
    torch.testing.assert_close(_attnpool_from_operands(apw, x), ref[0], rtol=1e-4, atol=1e-4)
    # the two loader errors a cosine check of the whole tower cannot see: a wrong temperature, positions left out
    wrong_q = {**apw, "q_w": apw["q_w"] * 8, "q_b": apw["q_b"] * 8}
    no_pos = {**apw, "pos": torch.zeros_like(apw["pos"])}
    for bad in (wrong_q, no_pos):
        assert float((_attnpool_from_operands(bad, x) - ref[0]).abs().max()) > 1e-2


def _expected_keys(arch):
    v, w = "visual.", arch.width
    keys = {}

    def conv_bn(conv, bn, O, I, k):
        keys[conv + ".weight"] = (O, I, k, k)
        for s in ("weight", "bias", "running_mean", "running_var"):
            keys[f"{bn}.{s}"] = (O,)
        keys[bn + ".num_batches_tracked"] = ()

    conv_bn(v + "conv1", v + "bn1", w // 2, 3, 3)
    conv_bn(v + "conv2", v + "bn2", w // 2, w // 2, 3)
    conv_bn(v + "conv3", v + "bn3", w, w // 2, 3)
    inp = w
    for i, depth in enumerate(arch.layers):
        P = w << i
        for j in range(depth):
            p = f"{v}layer{i + 1}.{j}."
            conv_bn(p + "conv1", p + "bn1", P, inp, 1)
            conv_bn(p + "conv2", p + "bn2", P, P, 3)
            conv_bn(p + "conv3", p + "bn3", 4 * P, P, 1)
            if j == 0:
                conv_bn(p + "downsample.0", p + "downsample.1", 4 * P, inp, 1)
            inp = 4 * P
    C, a = 32 * w, v + "attnpool."
    keys[a + "positional_embedding"] = (arch.tokens, C)
    for n in ("q_proj", "k_proj", "v_proj"):
        keys.update({f"{a}{n}.weight": (C, C), f"{a}{n}.bias": (C,)})
    keys.update({a + "c_proj.weight": (arch.out_dim, C), a + "c_proj.bias": (arch.out_dim,)})
    return keys


@pytest.mark.parametrize("name", ["RN50", "RN50x4"])
def test_synthetic_state_dict_has_openai_names(name):
    v, _ = archs.resolve_resnet_clip(name)
    sd = synthetic.random_open_clip_state_dict(vision=v, text=None, seed=0)
    want = _expected_keys(v)
    assert set(sd) == set(want)
    for k, shape in want.items():
        assert tuple(sd[k].shape) == shape, k


def _lib_or_skip():
    from marqo_amd import _lib as L
    return L, L.load()


def test_abi_refuses_bad_shapes_with_a_message():
    L, lib = _lib_or_skip()
    p, q = ctypes.c_void_p(16), ctypes.c_void_p(4096)

    def refused(rc, text):
        assert rc == -1
        msg = lib.mq_last_error().decode()
        assert text in msg, msg

    refused(lib.mq_resnet_conv3x3(p, p, p, q, 64, 1, 7, 7, 36, 64, 1, None), "Cin=36")
    refused(lib.mq_resnet_conv3x3(p, p, p, q, 64, 1, 7, 7, 64, 62, 1, None), "Cout=62")
    refused(lib.mq_resnet_conv3x3(p, p, p, q, 32, 1, 7, 7, 64, 64, 1, None), "ldy=32")
    refused(lib.mq_resnet_conv3x3(p, p, p, q, 64, 1, 7, 7, 64, 64, 2, None), "relu=2")
    refused(lib.mq_resnet_conv3x3(p, p, p, q, 64, 1 << 20, 56, 56, 64, 64, 1, None), "exceed 2^30")
    refused(lib.mq_resnet_conv3x3(p, p, p, None, 64, 1, 7, 7, 64, 64, 1, None), "null operand")
    refused(lib.mq_resnet_stem_gather(p, 1, p, 1, 225, None, None, None), "S=225")
    refused(lib.mq_resnet_avgpool2(p, q, 1, 7, 7, 64, None), "H=7")
    refused(lib.mq_resnet_attnpool_tokens(p, p, p, 1, 256, 2048, None), "HW=256")
    refused(lib.mq_resnet_attnpool_attend(p, p, p, 1, 50, 2000, None), "C=2000")
    cfg = L.ResNetCfg(image_size=224, layers=(ctypes.c_int32 * 4)(3, 4, 6, 3), width=64, heads=31, out_dim=1024)
    assert lib.mq_resnet_workspace_bytes(ctypes.byref(cfg), 1) == 0       # heads must be 32 w / 64
    cfg.heads = 32
    assert lib.mq_resnet_workspace_bytes(ctypes.byref(cfg), 1) > 0
    # a width that is not a multiple of 16 would leave a stage output 4 w that the GEMMs cannot take as K: refused up front
    bad = L.ResNetCfg(image_size=224, layers=(ctypes.c_int32 * 4)(1, 1, 1, 1), width=40, heads=20, out_dim=512)
    assert lib.mq_resnet_workspace_bytes(ctypes.byref(bad), 1) == 0
    w = L.ResNetWeights(blocks=ctypes.cast(p, ctypes.POINTER(L.ResNetBlockWeights)))
    refused(lib.mq_encode_resnet_u8(ctypes.byref(bad), ctypes.byref(w), p, 1, q, 1, p, 1 << 40, None), "width multiple of 16")
    refused(lib.mq_encode_resnet_u8(ctypes.byref(cfg), ctypes.byref(L.ResNetWeights()), p, 1, p, 1, p, 1 << 40, None), "null argument")


def test_gemm_relu_flags_are_checked_without_a_gpu():
    L, lib = _lib_or_skip()
    p = ctypes.c_void_p(16)
    rc = lib.mq_gemm_bf16(p, 64, p, 64, p, None, p, 64, 128, 64, 64, L.MQ_EPI_RELU | L.MQ_EPI_GELU | L.MQ_EPI_BIAS, None)
    assert rc == -1 and b"flag combination" in lib.mq_last_error()


def test_resnet_kernels_compile_without_scratch(tmp_path):
    src = os.path.join(ROOT, "marqo_amd", "csrc", "resnet.hip")
    out = tmp_path / "resnet.s"
    res = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wall", "-Wno-unused-function", "-S", "--cuda-device-only",
                          "-I", os.path.join(ROOT, "include"), "-o", str(out), src], capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stderr[-3000:]
    isa = out.read_text()
    for k in ("conv3x3_kernel", "stem_gather_kernel", "avgpool2_kernel", "ap_tokens_kernel", "ap_attend_kernel"):
        assert k in isa
    assert "scratch_" not in isa
    # the conv kernels' own bodies: from each symbol's label to its .Lfunc_end
    bodies = [isa[m.start():isa.index(".Lfunc_end", m.start())] for m in re.finditer(r"^_Z\S*conv3x3_kernel\S*:", isa, re.M)]
    assert len(bodies) == 4                              # (BIAS, BIAS | RELU) x (MT 2, 4)
    conv = "".join(bodies)
    for body in bodies:
        assert "v_mfma_f32_16x16x32_bf16" in body        # the implicit GEMM runs on the MFMA path
        assert "global_load_lds_dwordx4" in body         # the A tile is gathered straight into LDS (no im2col buffer)

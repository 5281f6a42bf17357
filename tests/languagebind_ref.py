"""Restatement, synthetic weights and checkpoint writer for the LanguageBind tests (tests/test_languagebind_ref_host.py,
tests/test_languagebind_host.py, tests/test_languagebind_gpu.py).  A plain helper module: nothing here calls the library.

RESTATEMENT.  Pure torch, written from reading the reference (s2_inference/languagebind/video/modeling_video.py: embeddings :105-121, encoder layer
:191-257, vision transformer :736-771, text pooling :620-624; languagebind/__init__.py:54-64).  It is NOT pinned to an execution of the reference:
`oracle/ref_shim.py` stubs the `languagebind` package.  What it is pinned to: with `add_time_attn` off it equals transformers' CLIP classes on the same
weights (tests/test_languagebind_ref_host.py), and the temporal sub-block is four lines on top of that, using the reference's explicit rearranges
`(b t) n d <-> (b n) t d`.  fp32 by default, `dtype=torch.float64` for kernel checks.

STATE DICT.  Keys are the Hugging Face CLIP names the reference's classes define, including its spelling `vision_model.pre_layrnorm` and the
`[1, T, W]` temporal embeddings."""
import json
import math
import os

import torch

from tests import owl_ref

VIDEO_PART, IMAGE_PART = "LanguageBind_Video_V1.5_FT", "LanguageBind_Image"
CTX = 77
VOCAB = 512 + len(owl_ref.MERGES) + 2        # owl_ref.write_tokenizer_files: byte units, units + </w>, merges, SOT, EOT (EOT = the largest id)

# (vision W, heads, layers, S, P) / text (W, heads, layers) / projection
SMALL = dict(W=128, heads=2, layers=2, S=32, P=16, mlp=256, tW=128, theads=2, tlayers=2, tmlp=256, D=64)
LARGE = dict(W=1024, heads=16, layers=2, S=224, P=14, mlp=4096, tW=128, theads=2, tlayers=2, tmlp=256, D=64)


def config(shape=SMALL, T=8, add_time_attn=True, hidden_act="gelu"):
    """the `config.json` of one part, as a dict"""
    s = shape
    return {
        "model_type": "LanguageBindVideo" if add_time_attn else "LanguageBindImage",
        "projection_dim": s["D"], "logit_scale_init_value": 2.6592,
        "vision_config": {"hidden_size": s["W"], "num_hidden_layers": s["layers"], "num_attention_heads": s["heads"], "intermediate_size": s["mlp"],
                          "patch_size": s["P"], "image_size": s["S"], "num_frames": T if add_time_attn else 1, "add_time_attn": bool(add_time_attn),
                          "hidden_act": hidden_act, "layer_norm_eps": 1e-5, "num_channels": 3},
        "text_config": {"hidden_size": s["tW"], "num_hidden_layers": s["tlayers"], "num_attention_heads": s["theads"], "intermediate_size": s["tmlp"],
                        "vocab_size": VOCAB, "max_position_embeddings": CTX, "hidden_act": hidden_act, "layer_norm_eps": 1e-5,
                        "bos_token_id": VOCAB - 2, "eos_token_id": VOCAB - 1, "pad_token_id": VOCAB - 1},
    }


def synthetic_state_dict(cfg, seed=0, temporal_scale=1.0):
    """seeded fp32 weights in the checkpoint's key naming.  Linear weights 1.2 / sqrt(fan_in) so that tokens differ after two blocks; temporal
    embeddings of ordinary size — std 0.5 times `temporal_scale`, that of this checkpoint's class and position embeddings (the reference
    INITIALISES them at W ** -0.5; what matters here is that the frame order is visible) —; LayerNorm affine near (1, 0); logit_scale off its
    init so that the two parts of a model differ."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    v, t, D = cfg["vision_config"], cfg["text_config"], cfg["projection_dim"]
    sd = {}

    def linear(key, out_f, in_f, bias=True):
        sd[key + ".weight"] = rn(out_f, in_f) * (1.2 / math.sqrt(in_f))
        if bias:
            sd[key + ".bias"] = rn(out_f) * 0.1

    def norm(key, W):
        sd[key + ".weight"] = 1.0 + 0.1 * rn(W)
        sd[key + ".bias"] = 0.1 * rn(W)

    def layers(prefix, c, temporal):
        W, F = c["hidden_size"], c["intermediate_size"]
        for i in range(c["num_hidden_layers"]):
            p = f"{prefix}encoder.layers.{i}."
            for n in "qkv":
                linear(p + f"self_attn.{n}_proj", W, W)
            linear(p + "self_attn.out_proj", W, W)
            norm(p + "layer_norm1", W)
            norm(p + "layer_norm2", W)
            linear(p + "mlp.fc1", F, W)
            linear(p + "mlp.fc2", W, F)
            if temporal:
                for n in "qkv":
                    linear(p + f"temporal_attn.{n}_proj", W, W)
                linear(p + "temporal_attn.out_proj", W, W)
                norm(p + "temporal_layer_norm1", W)
                sd[p + "temporal_embedding"] = rn(1, c["num_frames"], W) * (0.5 * temporal_scale)

    W, P, S = v["hidden_size"], v["patch_size"], v["image_size"]
    sd["vision_model.embeddings.class_embedding"] = rn(W) * 0.5
    sd["vision_model.embeddings.patch_embedding.weight"] = rn(W, 3, P, P) * (1.0 / math.sqrt(3 * P * P))
    sd["vision_model.embeddings.position_embedding.weight"] = rn((S // P) ** 2 + 1, W) * 0.5
    norm("vision_model.pre_layrnorm", W)
    layers("vision_model.", v, bool(v.get("add_time_attn")))
    norm("vision_model.post_layernorm", W)
    linear("visual_projection", D, W, bias=False)
    tW = t["hidden_size"]
    sd["text_model.embeddings.token_embedding.weight"] = rn(t["vocab_size"], tW) * 0.5
    sd["text_model.embeddings.position_embedding.weight"] = rn(t["max_position_embeddings"], tW) * 0.5
    layers("text_model.", t, False)
    norm("text_model.final_layer_norm", tW)
    linear("text_projection", D, tW, bias=False)
    sd["logit_scale"] = torch.tensor(2.6592 + 0.25 * float(rn(1)))
    return sd


def write_part(directory, cfg, sd):
    """one part's checkpoint directory: config.json, pytorch_model.bin, the CLIP tokenizer's vocab.json + merges.txt"""
    os.makedirs(str(directory), exist_ok=True)
    with open(os.path.join(str(directory), "config.json"), "w") as f:
        json.dump(cfg, f)
    torch.save({k: v.clone() for k, v in sd.items()}, os.path.join(str(directory), "pytorch_model.bin"))
    assert owl_ref.write_tokenizer_files(directory) == VOCAB


def write_model(root, shape=SMALL, T=8, image=True, seed=0):
    """`localpath` of a LanguageBind model: one sub-directory per part -> {part: (cfg, sd)}"""
    parts = {"video": (config(shape, T, True), None)}
    if image:
        parts["image"] = (config(shape, T, False), None)
    out = {}
    for k, (kind, (cfg, _)) in enumerate(parts.items()):
        sd = synthetic_state_dict(cfg, seed=seed + 17 * k)
        write_part(os.path.join(str(root), VIDEO_PART if kind == "video" else IMAGE_PART), cfg, sd)
        out[kind] = (cfg, sd)
    return out


# ---- the forward passes ----------------------------------------------------------------------------------------------------------------------
def _act(name):
    if name == "quick_gelu":
        return lambda x: x * torch.sigmoid(1.702 * x)
    if name == "gelu":
        return torch.nn.functional.gelu
    raise ValueError(name)


def _ln(x, sd, key, eps, dt):
    return torch.nn.functional.layer_norm(x, (x.shape[-1],), sd[key + ".weight"].to(dt), sd[key + ".bias"].to(dt), eps)


def _lin(x, sd, key, dt):
    b = sd.get(key + ".bias")
    return torch.nn.functional.linear(x, sd[key + ".weight"].to(dt), None if b is None else b.to(dt))


def attention(x, sd, prefix, heads, dt, causal=False):
    """CLIPAttention on [batch, len, W]: q scaled by head_dim ** -0.5, softmax over the keys, out_proj"""
    B, Ln, W = x.shape
    hd = W // heads
    split = lambda y: y.reshape(B, Ln, heads, hd).transpose(1, 2)
    q, k, v = (split(_lin(x, sd, prefix + f"{n}_proj", dt)) for n in "qkv")
    s = (q * hd ** -0.5) @ k.transpose(2, 3)
    if causal:
        s = s + torch.full((Ln, Ln), float("-inf"), dtype=dt).triu(1)
    o = torch.softmax(s, dim=-1) @ v
    return _lin(o.transpose(1, 2).reshape(B, Ln, W), sd, prefix + "out_proj", dt)


def encoder_layer(x, sd, p, c, dt, T=1, temporal=False, causal=False):
    """x [(b t), n, W].  modeling_video.py:209-255: the temporal sub-block, then the CLIP block"""
    heads, eps = c["num_attention_heads"], c["layer_norm_eps"]
    if temporal:
        bt, n, W = x.shape
        b = bt // T
        to_bn = lambda y: y.reshape(b, T, n, W).transpose(1, 2).reshape(b * n, T, W)        # (b t) n d -> (b n) t d
        to_bt = lambda y: y.reshape(b, n, T, W).transpose(1, 2).reshape(b * T, n, W)        # (b n) t d -> (b t) n d
        if T != 1:
            x = to_bt(to_bn(x) + sd[p + "temporal_embedding"].to(dt)[:, :T, :])
        h = _ln(to_bn(x), sd, p + "temporal_layer_norm1", eps, dt)
        x = x + to_bt(attention(h, sd, p + "temporal_attn.", heads, dt))
    x = x + attention(_ln(x, sd, p + "layer_norm1", eps, dt), sd, p + "self_attn.", heads, dt, causal)
    h = _lin(_act(c["hidden_act"])(_lin(_ln(x, sd, p + "layer_norm2", eps, dt), sd, p + "mlp.fc1", dt)), sd, p + "mlp.fc2", dt)
    return x + h


def vision_forward(sd, cfg, pixels, T=1, dtype=torch.float32):
    """pixels [(b t), 3, S, S] in (b t) order -> pooled, projected [b, D] (not normalised): patch conv, class token, positions, pre_layrnorm, the
    layers, post_layernorm of the class rows, mean over the T frames of a clip, visual_projection"""
    c, dt = cfg["vision_config"], dtype
    W, P = c["hidden_size"], c["patch_size"]
    bt = pixels.shape[0]
    x = torch.nn.functional.conv2d(pixels.to(dt), sd["vision_model.embeddings.patch_embedding.weight"].to(dt), stride=P)
    x = x.flatten(2).transpose(1, 2)
    cls = sd["vision_model.embeddings.class_embedding"].to(dt).expand(bt, 1, W)
    x = torch.cat([cls, x], dim=1) + sd["vision_model.embeddings.position_embedding.weight"].to(dt)
    x = _ln(x, sd, "vision_model.pre_layrnorm", c["layer_norm_eps"], dt)
    temporal = bool(c.get("add_time_attn"))
    for i in range(c["num_hidden_layers"]):
        x = encoder_layer(x, sd, f"vision_model.encoder.layers.{i}.", c, dt, T=T, temporal=temporal)
    pooled = _ln(x[:, 0, :], sd, "vision_model.post_layernorm", c["layer_norm_eps"], dt)
    pooled = pooled.reshape(bt // T, T, W).mean(1)
    return _lin(pooled, sd, "visual_projection", dt)


def video_forward(sd, cfg, pixel_values, dtype=torch.float32):
    """pixel_values [b, 3, T, S, S] -> [b, D]"""
    b, ch, T, S, _ = pixel_values.shape
    frames = pixel_values.permute(0, 2, 1, 3, 4).reshape(b * T, ch, S, S)                   # b c t h w -> (b t) c h w
    return vision_forward(sd, cfg, frames, T=T, dtype=dtype)


def image_forward(sd, cfg, pixels, dtype=torch.float32):
    return vision_forward(sd, cfg, pixels, T=1, dtype=dtype)


def text_forward(sd, cfg, ids, dtype=torch.float32):
    """ids int64 [n, ctx] (SOT ... EOT, padded) -> [n, D] (not normalised): causal CLIP text model, pooled at the argmax id, text_projection"""
    c, dt = cfg["text_config"], dtype
    n, Ln = ids.shape
    x = sd["text_model.embeddings.token_embedding.weight"].to(dt)[ids] + sd["text_model.embeddings.position_embedding.weight"].to(dt)[:Ln]
    for i in range(c["num_hidden_layers"]):
        x = encoder_layer(x, sd, f"text_model.encoder.layers.{i}.", c, dt, causal=True)
    x = _ln(x, sd, "text_model.final_layer_norm", c["layer_norm_eps"], dt)
    return _lin(x[torch.arange(n), ids.argmax(dim=-1)], sd, "text_projection", dt)


def embed(features, sd, modality, normalize):
    """languagebind/__init__.py:59-63 then multimodal_model_load.py:298-299: unit rows, times exp(logit_scale) for everything but text, unit again
    when normalize"""
    out = features / features.norm(dim=-1, keepdim=True)
    if modality != "language":
        out = out * sd["logit_scale"].to(out.dtype).exp()
    return out / out.norm(dim=-1, keepdim=True) if normalize else out


# ---- temporal attention on the kernel's own layout ---------------------------------------------------------------------------------------------
def temporal_attention_rearranged(qkv, B, T, N, heads):
    """qkv [B T N, 3W] (any float dtype) -> (out, absout) float64 [B T N, W]: the rows regrouped `(b t) n -> (b n) t` by an explicit rearrange,
    softmax(q k^T / sqrt(hd)) v per head, and back.  absout = P |v|, what tests/attention_ref.py's budget takes."""
    W = qkv.shape[1] // 3
    hd = W // heads
    x = qkv.double().reshape(B, T, N, 3, heads, hd).permute(0, 2, 3, 4, 1, 5)          # b n 3 h t d
    q, k, v = x[:, :, 0], x[:, :, 1], x[:, :, 2]
    p = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(hd), dim=-1)
    back = lambda y: y.permute(0, 3, 1, 2, 4).reshape(B * T * N, W)                     # b n h t d -> (b t n) (h d)
    return back(p @ v), back(p @ v.abs())


def temporal_attention_strided(qkv, B, T, N, heads):
    """the same by strided indexing, the way the kernel walks the rows: for every (b, n) the T rows (b T + t) N + n"""
    W = qkv.shape[1] // 3
    hd = W // heads
    x = qkv.double()
    out = torch.zeros(B * T * N, W, dtype=torch.float64, device=qkv.device)
    absout = torch.zeros_like(out)
    for b in range(B):
        for n in range(N):
            rows = (b * T + torch.arange(T, device=qkv.device)) * N + n
            blk = x[rows]
            for h in range(heads):
                q, k, v = (blk[:, i * W + h * hd: i * W + (h + 1) * hd] for i in range(3))
                p = torch.softmax(q @ k.t() / math.sqrt(hd), dim=-1)
                out[rows, h * hd:(h + 1) * hd] = p @ v
                absout[rows, h * hd:(h + 1) * hd] = p @ v.abs()
    return out, absout


def score_magnitude(qkv, B, T, N, heads):
    """float64 [B T N, W]: for every output element, max over the keys j of sum_d |q_d k_jd| of its (query row, head) — what bounds the fp32
    rounding of that row's scores"""
    W = qkv.shape[1] // 3
    hd = W // heads
    x = qkv.double().abs().reshape(B, T, N, 3, heads, hd).permute(0, 2, 3, 4, 1, 5)
    s = (x[:, :, 0] @ x[:, :, 1].transpose(-1, -2)).amax(dim=-1)                         # b n h t
    return s.permute(0, 3, 1, 2).unsqueeze(-1).expand(B, T, N, heads, hd).reshape(B * T * N, W)


def make_clip(b, T, S, seed=0):
    """fp32 [b, 3, T, S, S]: smooth per-frame content that differs from frame to frame (normalised-pixel range)"""
    g = torch.Generator().manual_seed(500 + seed)
    base = torch.randn(b, 3, 1, S, S, generator=g)
    drift = torch.randn(b, 3, T, S, S, generator=g)
    ramp = torch.linspace(-1.0, 1.0, T).reshape(1, 1, T, 1, 1)
    return (0.6 * base + 0.6 * drift + 0.8 * ramp * torch.randn(b, 3, 1, S, S, generator=g)).contiguous()

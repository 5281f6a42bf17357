"""Random-init checkpoints of the supported architectures (there is no network for real weights).

Used by bench.py and by loaders when `model_properties["synthetic_seed"]` is given explicitly; the
tensors use the same names and shapes as real open_clip / HuggingFace checkpoints, so everything
downstream (layout conversion, kernels) is exercised exactly as with real weights.
"""
from __future__ import annotations

import math
from typing import Dict

import torch

from marqo_amd.engine.archs import BertArch, ClipTextArch, ConvNextArch, NllbTextArch, ResNetArch, VitArch

Tensor = torch.Tensor


def _ln(sd, name, W, g):
    sd[name + ".weight"] = 1.0 + 0.1 * torch.randn(W, generator=g)
    sd[name + ".bias"] = 0.05 * torch.randn(W, generator=g)


def _lin(sd, name, out_f, in_f, g, std):
    sd[name + ".weight"] = std * torch.randn(out_f, in_f, generator=g)
    sd[name + ".bias"] = 0.02 * torch.randn(out_f, generator=g)


def _resblocks(sd, prefix, layers, W, F, g):
    std = 0.6 / math.sqrt(W)
    for i in range(layers):
        p = f"{prefix}resblocks.{i}."
        _ln(sd, p + "ln_1", W, g)
        sd[p + "attn.in_proj_weight"] = std * torch.randn(3 * W, W, generator=g)
        sd[p + "attn.in_proj_bias"] = 0.02 * torch.randn(3 * W, generator=g)
        _lin(sd, p + "attn.out_proj", W, W, g, std)
        _ln(sd, p + "ln_2", W, g)
        _lin(sd, p + "mlp.c_fc", F, W, g, std)
        _lin(sd, p + "mlp.c_proj", W, F, g, std)


def _convnext_visual(sd, arch: ConvNextArch, g) -> None:
    """timm ConvNeXt trunk under visual.trunk.* + open_clip's projection head under visual.head.*.  The layer scales are trained-like,
    U(0.05, 0.5): with timm's 1e-6 init every block would be the identity and a parity check would prove nothing."""
    t, dims = "visual.trunk.", arch.dims
    sd[t + "stem.0.weight"] = torch.randn(dims[0], 3, 4, 4, generator=g) / math.sqrt(48)
    sd[t + "stem.0.bias"] = 0.02 * torch.randn(dims[0], generator=g)
    _ln(sd, t + "stem.1", dims[0], g)
    for i, (depth, C) in enumerate(zip(arch.depths, dims)):
        p = f"{t}stages.{i}."
        if i > 0:
            _ln(sd, p + "downsample.0", dims[i - 1], g)
            sd[p + "downsample.1.weight"] = torch.randn(C, dims[i - 1], 2, 2, generator=g) / math.sqrt(4 * dims[i - 1])
            sd[p + "downsample.1.bias"] = 0.02 * torch.randn(C, generator=g)
        for j in range(depth):
            b = f"{p}blocks.{j}."
            sd[b + "conv_dw.weight"] = torch.randn(C, 1, 7, 7, generator=g) / 7.0
            sd[b + "conv_dw.bias"] = 0.02 * torch.randn(C, generator=g)
            _ln(sd, b + "norm", C, g)
            _lin(sd, b + "mlp.fc1", 4 * C, C, g, 1.0 / math.sqrt(C))
            _lin(sd, b + "mlp.fc2", C, 4 * C, g, 1.0 / math.sqrt(4 * C))
            sd[b + "gamma"] = 0.05 + 0.45 * torch.rand(C, generator=g)
    _ln(sd, t + "head.norm", dims[3], g)
    C3, E = dims[3], arch.out_dim
    if arch.head == "linear":
        sd["visual.head.proj.weight"] = torch.randn(E, C3, generator=g) / math.sqrt(C3)
    else:
        _lin(sd, "visual.head.mlp.fc1", 2 * E, C3, g, 1.0 / math.sqrt(C3))
        sd["visual.head.mlp.fc2.weight"] = torch.randn(E, 2 * E, generator=g) / math.sqrt(2 * E)


def _bn(sd, name, C, g, scale=(0.5, 1.0)):
    """eval-mode BatchNorm with trained-like statistics: a running mean / variance that the conv output does not match exactly, and weights of
    `scale` (lo, hi) — the last BN of a residual branch gets small ones, as trained ResNets have them, so that 100+ blocks stay bounded"""
    lo, hi = scale
    sd[name + ".weight"] = lo + (hi - lo) * torch.rand(C, generator=g)
    sd[name + ".bias"] = 0.05 * torch.randn(C, generator=g)
    sd[name + ".running_mean"] = 0.1 * torch.randn(C, generator=g)
    sd[name + ".running_var"] = 0.5 + torch.rand(C, generator=g)
    sd[name + ".num_batches_tracked"] = torch.tensor(0)


def _conv(sd, name, O, I, k, g):
    sd[name + ".weight"] = torch.randn(O, I, k, k, generator=g) * math.sqrt(2.0 / (I * k * k))


def _resnet_visual(sd, arch: ResNetArch, g) -> None:
    """ModifiedResNet under visual.* (OpenAI CLIP / open_clip names): He-initialised convolutions, trained-like BatchNorm statistics"""
    v, w = "visual.", arch.width
    _conv(sd, v + "conv1", w // 2, 3, 3, g); _bn(sd, v + "bn1", w // 2, g)
    _conv(sd, v + "conv2", w // 2, w // 2, 3, g); _bn(sd, v + "bn2", w // 2, g)
    _conv(sd, v + "conv3", w, w // 2, 3, g); _bn(sd, v + "bn3", w, g)
    inp = w
    for i, depth in enumerate(arch.layers):
        P = w << i
        for j in range(depth):
            p = f"{v}layer{i + 1}.{j}."
            _conv(sd, p + "conv1", P, inp, 1, g); _bn(sd, p + "bn1", P, g)
            _conv(sd, p + "conv2", P, P, 3, g); _bn(sd, p + "bn2", P, g)
            _conv(sd, p + "conv3", 4 * P, P, 1, g); _bn(sd, p + "bn3", 4 * P, g, (0.05, 0.25))
            if (i > 0 and j == 0) or inp != 4 * P:
                _conv(sd, p + "downsample.0", 4 * P, inp, 1, g); _bn(sd, p + "downsample.1", 4 * P, g)
            inp = 4 * P
    C, E, ap = 32 * w, arch.out_dim, v + "attnpool."
    sd[ap + "positional_embedding"] = torch.randn(arch.tokens, C, generator=g) / math.sqrt(C)
    for name in ("q_proj", "k_proj", "v_proj"):
        _lin(sd, ap + name, C, C, g, 1.0 / math.sqrt(C))
    _lin(sd, ap + "c_proj", E, C, g, 1.0 / math.sqrt(C))


def random_open_clip_state_dict(vision: VitArch = None, text: ClipTextArch = None, seed: int = 0) -> Dict[str, Tensor]:
    """open_clip-named state dict for the given towers (either may be None)."""
    g = torch.Generator().manual_seed(seed)
    sd: Dict[str, Tensor] = {}
    if isinstance(vision, ConvNextArch):
        _convnext_visual(sd, vision, g)
    elif isinstance(vision, ResNetArch):
        _resnet_visual(sd, vision, g)
    elif vision is not None and vision.pool == "map":
        # timm SigLIP ViT as open_clip's visual.trunk (no class token, conv bias, attention-pool head)
        W, P, F, t = vision.width, vision.patch_size, vision.mlp_dim, "visual.trunk."
        std = 0.6 / math.sqrt(W)
        sd[t + "patch_embed.proj.weight"] = torch.randn(W, 3, P, P, generator=g) / math.sqrt(3 * P * P)
        sd[t + "patch_embed.proj.bias"] = 0.05 * torch.randn(W, generator=g)
        sd[t + "pos_embed"] = 0.3 * torch.randn(1, vision.tokens, W, generator=g)
        for i in range(vision.layers):
            p = f"{t}blocks.{i}."
            _ln(sd, p + "norm1", W, g)
            _lin(sd, p + "attn.qkv", 3 * W, W, g, std)
            _lin(sd, p + "attn.proj", W, W, g, std)
            _ln(sd, p + "norm2", W, g)
            _lin(sd, p + "mlp.fc1", F, W, g, std)
            _lin(sd, p + "mlp.fc2", W, F, g, std / 2)
        _ln(sd, t + "norm", W, g)
        a = t + "attn_pool."
        sd[a + "latent"] = torch.randn(1, 1, W, generator=g) / math.sqrt(W)
        _lin(sd, a + "q", W, W, g, std)
        _lin(sd, a + "kv", 2 * W, W, g, std)
        _lin(sd, a + "proj", W, W, g, std)
        _ln(sd, a + "norm", W, g)
        _lin(sd, a + "mlp.fc1", F, W, g, std)
        _lin(sd, a + "mlp.fc2", W, F, g, std / 2)
    elif vision is not None and getattr(vision, "eva", False):
        # timm Eva (eva02_*_clip_*) as open_clip's visual.trunk: separate q / k / v projections (no k bias), attn.norm, SwiGLU with its norm, head
        W, P, F, t = vision.width, vision.patch_size, vision.mlp_dim, "visual.trunk."
        std = 0.6 / math.sqrt(W)
        sd[t + "patch_embed.proj.weight"] = torch.randn(W, 3, P, P, generator=g) / math.sqrt(3 * P * P)
        sd[t + "patch_embed.proj.bias"] = 0.05 * torch.randn(W, generator=g)
        sd[t + "cls_token"] = 0.5 * torch.randn(1, 1, W, generator=g)
        sd[t + "pos_embed"] = 0.3 * torch.randn(1, vision.tokens, W, generator=g)
        for i in range(vision.layers):
            p = f"{t}blocks.{i}."
            _ln(sd, p + "norm1", W, g)
            _lin(sd, p + "attn.q_proj", W, W, g, std)
            sd[p + "attn.k_proj.weight"] = torch.randn(W, W, generator=g) * std
            _lin(sd, p + "attn.v_proj", W, W, g, std)
            _ln(sd, p + "attn.norm", W, g)
            _lin(sd, p + "attn.proj", W, W, g, std)
            _ln(sd, p + "norm2", W, g)
            _lin(sd, p + "mlp.fc1_g", F, W, g, 2 * std)
            _lin(sd, p + "mlp.fc1_x", F, W, g, 2 * std)
            _ln(sd, p + "mlp.norm", F, g)
            _lin(sd, p + "mlp.fc2", W, F, g, std / 2)
        _ln(sd, t + "norm", W, g)
        _lin(sd, t + "head", vision.out_dim, W, g, 1.0 / math.sqrt(W))
    elif vision is not None:
        W, P = vision.width, vision.patch_size
        sd["visual.conv1.weight"] = torch.randn(W, 3, P, P, generator=g) / math.sqrt(3 * P * P)
        sd["visual.class_embedding"] = 0.5 * torch.randn(W, generator=g)
        sd["visual.positional_embedding"] = 0.3 * torch.randn(vision.tokens, W, generator=g)
        if vision.ln_pre:
            _ln(sd, "visual.ln_pre", W, g)
        _resblocks(sd, "visual.transformer.", vision.layers, W, vision.mlp_dim, g)
        if vision.pool == "query":
            # CoCa: AttentionalPooler of width D = out_dim behind the trunk (256 learned queries; MultiheadAttention with kdim = vdim = W)
            D, a = vision.out_dim, "visual.attn_pool."
            sd[a + "query"] = torch.randn(256, D, generator=g)
            _ln(sd, a + "ln_q", D, g)
            _ln(sd, a + "ln_k", W, g)
            sd[a + "attn.q_proj_weight"] = torch.randn(D, D, generator=g) / math.sqrt(D)
            sd[a + "attn.k_proj_weight"] = torch.randn(D, W, generator=g) / math.sqrt(W)
            sd[a + "attn.v_proj_weight"] = torch.randn(D, W, generator=g) / math.sqrt(W)
            sd[a + "attn.in_proj_bias"] = 0.02 * torch.randn(3 * D, generator=g)
            _lin(sd, a + "attn.out_proj", D, D, g, 1.0 / math.sqrt(D))
            _ln(sd, "visual.ln_post", D, g)
            sd["visual.proj"] = torch.randn(D, D, generator=g) / math.sqrt(D)
        else:
            _ln(sd, "visual.ln_post", W, g)
            sd["visual.proj"] = torch.randn(W, vision.out_dim, generator=g) / math.sqrt(W)
    if isinstance(text, NllbTextArch):
        sd.update(random_nllb_text_state_dict(text, seed=seed + 1))
        sd["logit_scale"], sd["logit_bias"] = torch.tensor(math.log(10.0)), torch.tensor(-10.0)
    elif text is not None and hasattr(text, "bert"):
        # open_clip HFTextEncoder (CustomTextCLIP): HF-named encoder under text.transformer.*, projection MLP under text.proj.{0,2}
        for k, v in random_bert_state_dict(text.bert, seed=seed + 1).items():
            sd["text.transformer." + k] = v
        if text.bert.type_vocab == 1:
            sd["text.transformer.embeddings.token_type_embeddings.weight"] = sd["text.transformer.embeddings.token_type_embeddings.weight"][:1].clone()
        W, Hd = text.bert.width, text.proj_hidden
        sd["text.proj.0.weight"] = torch.randn(Hd, W, generator=g) / math.sqrt(W)
        sd["text.proj.2.weight"] = torch.randn(text.out_dim, Hd, generator=g) / math.sqrt(Hd)
        sd["logit_scale"] = torch.tensor(math.log(1 / 0.07))
    elif text is not None:
        W, px = text.width, text.prefix
        sd[px + "token_embedding.weight"] = 0.5 * torch.randn(text.vocab, W, generator=g)
        sd[px + "positional_embedding"] = 0.3 * torch.randn(text.ctx, W, generator=g)
        if getattr(text, "cls_embed", False):
            sd[px + "cls_emb"] = 0.5 * torch.randn(W, generator=g)
        _resblocks(sd, px + "transformer.", text.layers, W, text.mlp_dim, g)
        _ln(sd, px + "ln_final", W, g)
        if text.proj_bias:
            _lin(sd, px + "text_projection", text.out_dim, W, g, 1.0 / math.sqrt(W))
        else:
            sd[px + "text_projection"] = torch.randn(W, text.out_dim, generator=g) / math.sqrt(W)
        sd["logit_scale"] = torch.tensor(math.log(1 / 0.07))
    return sd


def random_dino_state_dict(arch: VitArch, seed: int = 0) -> Dict[str, Tensor]:
    """facebookresearch/dino VisionTransformer-named state dict (engine/dino.py; the 'dino-v1' / 'dino-v2' patch methods)"""
    g = torch.Generator().manual_seed(seed)
    W, P, F = arch.width, arch.patch_size, arch.mlp_dim
    std = 0.6 / math.sqrt(W)
    sd: Dict[str, Tensor] = {}
    sd["cls_token"] = 0.5 * torch.randn(1, 1, W, generator=g)
    sd["pos_embed"] = 0.3 * torch.randn(1, arch.tokens, W, generator=g)
    sd["patch_embed.proj.weight"] = torch.randn(W, 3, P, P, generator=g) / math.sqrt(3 * P * P)
    sd["patch_embed.proj.bias"] = 0.05 * torch.randn(W, generator=g)
    for i in range(arch.layers):
        p = f"blocks.{i}."
        _ln(sd, p + "norm1", W, g)
        _lin(sd, p + "attn.qkv", 3 * W, W, g, std)
        _lin(sd, p + "attn.proj", W, W, g, std)
        _ln(sd, p + "norm2", W, g)
        _lin(sd, p + "mlp.fc1", F, W, g, std)
        _lin(sd, p + "mlp.fc2", W, F, g, std / 2)
    _ln(sd, "norm", W, g)
    return sd


def random_nllb_text_state_dict(arch: NllbTextArch, seed: int = 0) -> Dict[str, Tensor]:
    """open_clip HFTextEncoder over a transformers M2M100Encoder (the NLLB-CLIP text tower): `text.transformer.*` + `text.proj.weight`.  The token
    table is small (M2M100 multiplies it by sqrt(width) = 32) so that the sinusoidal positions, of unit scale, stay visible in the sum."""
    g = torch.Generator().manual_seed(seed)
    W, F, t = arch.width, arch.mlp_dim, "text.transformer."
    std = 0.6 / math.sqrt(W)
    sd: Dict[str, Tensor] = {t + "embed_tokens.weight": (1.0 / math.sqrt(W)) * torch.randn(arch.vocab, W, generator=g)}
    for i in range(arch.layers):
        p = f"{t}layers.{i}."
        for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
            _lin(sd, p + "self_attn." + n, W, W, g, std)
        _ln(sd, p + "self_attn_layer_norm", W, g)
        _lin(sd, p + "fc1", F, W, g, std)
        _lin(sd, p + "fc2", W, F, g, 0.6 / math.sqrt(F))
        _ln(sd, p + "final_layer_norm", W, g)
    _ln(sd, t + "layer_norm", W, g)
    sd["text.proj.weight"] = torch.randn(arch.out_dim, W, generator=g) / math.sqrt(W)
    return sd


def random_bert_state_dict(arch: BertArch, seed: int = 0) -> Dict[str, Tensor]:
    """HuggingFace BertModel-named state dict."""
    g = torch.Generator().manual_seed(seed)
    W, F = arch.width, arch.mlp_dim
    std = 0.6 / math.sqrt(W)
    sd: Dict[str, Tensor] = {}
    if arch.glu or arch.rope_theta is not None:   # Alibaba-NLP NewModel naming (stella_en_400M_v5)
        sd["embeddings.word_embeddings.weight"] = 0.5 * torch.randn(arch.vocab, W, generator=g)
        sd["embeddings.token_type_embeddings.weight"] = 0.3 * torch.randn(2, W, generator=g)
        _ln(sd, "embeddings.LayerNorm", W, g)
        for i in range(arch.layers):
            p = f"encoder.layer.{i}."
            _lin(sd, p + "attention.qkv_proj", 3 * W, W, g, std)
            _lin(sd, p + "attention.o_proj", W, W, g, std)
            _ln(sd, p + "attn_ln", W, g)
            sd[p + "mlp.up_gate_proj.weight"] = std * torch.randn(2 * F, W, generator=g)
            _lin(sd, p + "mlp.down_proj", W, F, g, 0.6 / math.sqrt(F))
            _ln(sd, p + "mlp_ln", W, g)
        return sd
    sd["embeddings.word_embeddings.weight"] = 0.5 * torch.randn(arch.vocab, W, generator=g)
    sd["embeddings.position_embeddings.weight"] = 0.3 * torch.randn(arch.max_pos + arch.pos_offset, W, generator=g)
    mpnet = arch.rel_buckets > 0   # MPNetModel naming, no token types, one relative-position bias table
    if mpnet:
        sd["encoder.relative_attention_bias.weight"] = 0.5 * torch.randn(arch.rel_buckets, arch.heads, generator=g)
    else:
        sd["embeddings.token_type_embeddings.weight"] = 0.3 * torch.randn(2, W, generator=g)
    _ln(sd, "embeddings.LayerNorm", W, g)
    for i in range(arch.layers):
        p = f"encoder.layer.{i}."
        for n in (("attn.q", "attn.k", "attn.v") if mpnet else ("self.query", "self.key", "self.value")):
            _lin(sd, p + f"attention.{n}", W, W, g, std)
        _lin(sd, p + ("attention.attn.o" if mpnet else "attention.output.dense"), W, W, g, std)
        _ln(sd, p + ("attention.LayerNorm" if mpnet else "attention.output.LayerNorm"), W, g)
        _lin(sd, p + "intermediate.dense", F, W, g, std)
        _lin(sd, p + "output.dense", W, F, g, std)
        _ln(sd, p + "output.LayerNorm", W, g)
    return sd


def cross_encoder_state_dict(W: int, layers: int, heads: int, mlp: int, vocab: int, seed: int = 0, max_pos: int = 512,
                             pooler_std: float = 1.0, classifier_std: float = 8.0, attention_gain: float = 4.0) -> Dict[str, Tensor]:
    """HuggingFace BertForSequenceClassification-named state dict with one label: `bert.*` = random_bert_state_dict, plus the pooler
    and the classifier.  The pooler's pre-activation has a standard deviation of about pooler_std (its input, a LayerNorm output, has
    unit scale), so tanh is neither linear nor saturated; the classifier's weights are classifier_std / sqrt(W), which spreads the
    logits — a head whose logits all agree would hide an error of the tower.  The query / key weights are attention_gain times
    random_bert_state_dict's: its near-uniform attention averages the passage away and leaves every pair of one query almost the same
    [CLS] row (logits of 24 unrelated pairs then spread by 0.3; with the peaky attention and these scales by 1.4 or more, checked on
    the CPU against transformers in tests/test_rerank_host.py)."""
    arch = BertArch(vocab=vocab, max_pos=max_pos, width=W, layers=layers, heads=heads, mlp_dim=mlp)
    sd = {"bert." + k: v for k, v in random_bert_state_dict(arch, seed=seed).items()}
    for k in sd:
        if k.endswith(("attention.self.query.weight", "attention.self.key.weight")):
            sd[k] = sd[k] * attention_gain
    g = torch.Generator().manual_seed(seed + 7919)
    sd["bert.pooler.dense.weight"] = pooler_std / math.sqrt(W) * torch.randn(W, W, generator=g)
    sd["bert.pooler.dense.bias"] = 0.1 * torch.randn(W, generator=g)
    sd["classifier.weight"] = classifier_std / math.sqrt(W) * torch.randn(1, W, generator=g)
    sd["classifier.bias"] = 0.3 * torch.randn(1, generator=g)
    return sd


# ---- trained-like statistics (bench.py's fp8 row) -------------------------------------------------------------------------------------------
# N(0, s) weights never show a quantiser what a trained checkpoint does, and the load-time fp8 policy (towers.tune_fp8) decides on measured
# error: on random-init weights it moves 7 of ViT-L/14's 24 blocks to e4m3, on trained-like ones 13 + 8 MLP halves — the bench row on random
# weights under-states what a real checkpoint gets.  The recipe (the same one the parity fixtures use, written out here so
# that the product's bench does not lean on test infrastructure): LayerNorm gains log-normal with a handful of channels at 0.05 and 4, per-layer
# weight scale 0.7-1.6x, 1 % outlier output channels (4x), peaky attention (q / k rows 2x), and a class-token massive activation (~150 in two
# residual channels from block 2 on) that every later LayerNorm damps with a small gain.
def trained_like_open_clip_state_dict(vision: VitArch, seed: int = 0, massive_layer: int = 2, massive_value: float = 30.0,
                                      later_gain: float = 0.05) -> Dict[str, Tensor]:
    if vision.pool == "map":
        raise ValueError("trained_like_open_clip_state_dict: class-token ViTs only")
    sd = random_open_clip_state_dict(vision=vision, seed=seed)
    g = torch.Generator().manual_seed(seed + 7000)
    W, F, layers, pre = vision.width, vision.mlp_dim, vision.layers, "visual.transformer."
    base = 0.6 / math.sqrt(W)
    for i in range(layers):
        p = f"{pre}resblocks.{i}."
        for ln in ("ln_1", "ln_2"):
            gam = torch.exp(0.4 * torch.randn(W, generator=g))
            idx = torch.randperm(W, generator=g)
            gam[idx[:8]], gam[idx[8:16]] = 0.05, 4.0
            sd[p + ln + ".weight"] = gam
            sd[p + ln + ".bias"] = 0.3 * torch.randn(W, generator=g)
        scale = 0.7 + 0.9 * float(torch.rand(1, generator=g))
        for name, (n_out, n_in) in (("attn.in_proj_", (3 * W, W)), ("attn.out_proj.", (W, W)), ("mlp.c_fc.", (F, W)), ("mlp.c_proj.", (W, F))):
            std = base * scale * (math.sqrt(W / n_in) if n_in != W else 1.0)
            w = std * torch.randn(n_out, n_in, generator=g)
            w[torch.randperm(n_out, generator=g)[: max(1, n_out // 100)]] *= 4.0
            if name == "attn.in_proj_":
                w[: 2 * W] *= 2.0
            sd[p + name + "weight"] = w
            sd[p + name + "bias"] = 0.1 * torch.randn(n_out, generator=g)
    c0, targets, unit = 5, (W // 3, W // 2 + 1), 7
    sd["visual.class_embedding"][c0] = 20.0
    sd["visual.positional_embedding"][0, c0] = 0.0
    sd["visual.ln_pre.weight"][c0] = 1.0
    sd["visual.ln_pre.bias"][c0] = 0.0
    if layers > massive_layer:
        for i in range(layers):
            for ln in ("ln_1", "ln_2"):
                q = f"{pre}resblocks.{i}.{ln}."
                sd[q + "weight"][c0], sd[q + "bias"][c0] = later_gain, 0.0
                if i > massive_layer:
                    for c in targets:
                        sd[q + "weight"][c], sd[q + "bias"][c] = later_gain, 0.0
        p = f"{pre}resblocks.{massive_layer}."
        sd[p + "ln_2.weight"][c0] = 1.0
        sd[p + "mlp.c_fc.weight"][unit] = 0.0
        sd[p + "mlp.c_fc.weight"][unit, c0] = 1.0
        sd[p + "mlp.c_fc.bias"][unit] = -8.0
        sd[p + "mlp.c_proj.weight"][:, unit] = 0.0
        for c in targets:
            sd[p + "mlp.c_proj.weight"][c, unit] = massive_value
    sd["visual.ln_post.weight"] = torch.exp(0.4 * torch.randn(W, generator=g))
    sd["visual.ln_post.bias"] = 0.3 * torch.randn(W, generator=g)
    for c in (c0,) + tuple(targets):
        sd["visual.ln_post.weight"][c] = later_gain
    return sd


def natural_images_u8(n: int, height: int, width: int, seed: int = 0) -> Tensor:
    """uint8 HWC [n, height, width, 3] with natural-image statistics instead of white noise: 1/f amplitude spectrum with random phases, strongly
    correlated colour channels, an illumination gradient, a few flat patches with sharp edges (mean ~0.45, contrast ~0.22)"""
    import numpy as np
    rng = np.random.default_rng(seed + 9000)
    fy, fx = np.fft.fftfreq(height)[:, None], np.fft.rfftfreq(width)[None, :]
    f = np.sqrt(fy * fy + fx * fx)
    f[0, 0] = 1.0
    amp = 1.0 / f
    amp[0, 0] = 0.0
    out = np.empty((n, height, width, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:height, 0:width]

    def field():
        x = np.fft.irfft2(amp * np.exp(2j * np.pi * rng.random(amp.shape)), s=(height, width))
        return x / (x.std() + 1e-12)
    for i in range(n):
        shared = field()
        img = np.stack([0.85 * shared + 0.3 * field() for _ in range(3)], axis=-1)
        gy, gx = rng.uniform(-0.6, 0.6, 2)
        img += (gy * (yy / height - 0.5) + gx * (xx / width - 0.5))[..., None]
        img = 0.45 + 0.22 * img / (img.std() + 1e-12)
        for _ in range(int(rng.integers(2, 6))):
            h0, w0 = int(rng.integers(0, height - 8)), int(rng.integers(0, width - 8))
            h1, w1 = min(height, h0 + int(rng.integers(8, height // 2))), min(width, w0 + int(rng.integers(8, width // 2)))
            img[h0:h1, w0:w1] = 0.6 * img[h0:h1, w0:w1] + 0.4 * rng.random(3)
        out[i] = np.clip(img * 255.0 + 0.5, 0, 255).astype(np.uint8)
    return torch.from_numpy(out)

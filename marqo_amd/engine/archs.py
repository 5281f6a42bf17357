"""Architecture tables for the towers the engine runs.

Shapes are the published open_clip 2.24.0 model configs / HF BERT configs (third-party, not in the
reference tree; the reference only pins names and output dims in
src/marqo/s2_inference/model_registry.py:76-610,616-880).  Only towers whose attention head dim is
64 are runnable by the gfx950 attention kernel; the others are listed so that the error is explicit.
"""
from __future__ import annotations

from dataclasses import dataclass, replace
from typing import Optional, Tuple, Union

OPENAI_DATASET_MEAN = (0.48145466, 0.4578275, 0.40821073)  # clip_utils.py:32
OPENAI_DATASET_STD = (0.26862954, 0.26130258, 0.27577711)  # clip_utils.py:33


@dataclass(frozen=True)
class VitArch:
    image_size: int
    patch_size: int
    width: int
    layers: int
    heads: int
    mlp_dim: int
    out_dim: int
    quick_gelu: bool = False
    ln_eps: float = 1e-5
    pool: str = "cls"  # "cls": open_clip VisionTransformer (class token, ln_pre, ln_post(class token) @ proj);
    #                    "map": timm SigLIP ViT behind open_clip's TimmModel (no class token, no ln_pre, attention-pool head, no proj);
    #                    "avg": open_clip VisionTransformer with pool_type 'avg' + final_ln_after_pool (CLIPA): class token kept in the sequence,
    #                           mean of the PATCH tokens -> ln_post -> proj
    #                    "query": open_clip VisionTransformer + AttentionalPooler (CoCa): class token and ln_pre as in CLIP, every token runs every
    #                           block, one learned query attends over ln_k(tokens) in a pooler of width out_dim -> ln_post -> proj
    ln_pre: bool = True          # False: `no_ln_pre` (CLIPA)
    preprocessor: Optional[str] = None   # open_clip preprocess config of the registry entry when it is not the default ("CLIPA")
    pool_heads: int = 8          # pool "query": heads of the attentional pooler (attn_pooler_heads)
    # timm EVA02 CLIP towers behind open_clip's TimmModel (`visual.trunk.*`, model_registry.py:441-460; timm eva.py eva02_*_clip_*): class token, learned
    # absolute positions AND 2-D rotary positions on the patch tokens' q / k, conv bias, no ln_pre; blocks with separate q / k / v projections (no k
    # bias), a LayerNorm between attention and out-projection, SwiGLU MLP (hidden = mlp_dim, e.g. int(1024 * 4 * 2 / 3) = 2730) with a LayerNorm
    # behind the gate; norm(class token) -> head (a Linear WITH bias = the projection)
    eva: bool = False
    rope_ref_grid: int = 16      # eva: `ref_feat_shape` — rotary positions are grid index / grid * rope_ref_grid (the pre-training grid)
    rope_theta: float = 10000.0

    @property
    def tokens(self) -> int:
        return (self.image_size // self.patch_size) ** 2 + (0 if self.pool == "map" else 1)

    def rope_table(self):
        """eva: fp32 [patches, 2, head_dim] = (cos | sin) per patch position, timm's RotaryEmbeddingCat for in_pixels = False with `ref_feat_shape`
        (build_rotary_pos_embed / build_fourier_pos_embed / freq_bands, the torch ops in their order): head_dim // 4 bands
        1 / theta ** (k / (head_dim // 4)); positions t = arange(grid) / grid * ref_grid per axis; angles [y bands | x bands], each repeated twice
        (the interleaved pairs of apply_rot_embed_cat)."""
        import torch
        G, hd = self.image_size // self.patch_size, self.width // self.heads
        nb = hd // 4
        bands = 1.0 / (self.rope_theta ** (torch.arange(0, nb, 1, dtype=torch.int64).to(torch.float32) / nb))
        t = torch.arange(G, dtype=torch.float32) / G * self.rope_ref_grid
        grid = torch.stack(torch.meshgrid(t, t, indexing="ij"), dim=-1).unsqueeze(-1)     # [G, G, 2, 1]
        ang = grid * bands                                                                # [G, G, 2, nb]
        sin = ang.sin().reshape(G * G, -1).repeat_interleave(2, -1)
        cos = ang.cos().reshape(G * G, -1).repeat_interleave(2, -1)
        return torch.stack([cos, sin], dim=1).contiguous()

    @property
    def gflop_per_image(self) -> float:
        """Algorithmic FLOPs (2MNK per GEMM, attention 4 T^2 W per layer) — SURVEY.md §8(d)."""
        T, W, F = self.tokens, self.width, self.mlp_dim
        patch = 2 * (self.image_size // self.patch_size) ** 2 * W * 3 * self.patch_size ** 2
        layer = 2 * T * W * (3 * W) + 2 * T * W * W + 2 * (3 if self.eva else 2) * T * W * F + 4 * T * T * W
        if self.pool == "query":  # keys | values of every token at the pooler's width, one query, out-projection, final projection
            D = self.out_dim
            head = 2 * T * W * (2 * D) + 4 * T * D + 2 * D * D + 2 * D * D
        elif self.pool == "map":  # keys | values of every token, one query per head, proj + MLP on the pooled row
            head = 2 * T * W * (2 * W) + 4 * T * W + 2 * W * W + 2 * 2 * W * F
        else:
            head = 2 * W * self.out_dim
        return (patch + self.layers * layer + head) / 1e9


@dataclass(frozen=True)
class ConvNextArch:
    """timm ConvNeXt trunk behind open_clip's TimmModel with timm_pool "" (timm's head: global average pool -> LayerNorm) and open_clip's
    projection head (`visual.trunk.*`, `visual.head.*`): the open_clip convnext_* model configs (model_registry.py:274-339 in the reference)."""
    image_size: int
    depths: Tuple[int, int, int, int]
    dims: Tuple[int, int, int, int]
    ln_eps: float
    head: str                  # "linear": visual.head.proj (no bias); "mlp": visual.head.mlp.fc1 (+ bias) -> GELU -> fc2
    out_dim: int
    preprocessor: Optional[str] = None   # (the OpenCLIP transform: bicubic shortest-side resize, centre crop, OpenAI statistics)
    pool: str = "convnext"     # (read by the loaders: not "map", so the OpenCLIP preprocessing is selected)
    quick_gelu: bool = False   # (kept so that resolve_open_clip can `replace` it; the trunk's GELU is always erf)

    @property
    def gflop_per_image(self) -> float:
        """Algorithmic FLOPs: 2 MNK of every 1x1 convolution (stem, downsample, fc1, fc2, head) plus 2 * 49 per depthwise output."""
        G = self.image_size // 4
        f = 2 * G * G * self.dims[0] * 48
        for i, (d, C) in enumerate(zip(self.depths, self.dims)):
            if i > 0:
                f += 2 * G * G * C * 4 * self.dims[i - 1]
            f += d * (2 * G * G * C * 49 + 2 * 2 * G * G * C * 4 * C)
            G //= 2
        C3, E = self.dims[3], self.out_dim
        f += 2 * C3 * E if self.head == "linear" else 2 * C3 * 2 * E + 2 * 2 * E * E
        return f / 1e9


@dataclass(frozen=True)
class ResNetArch:
    """OpenAI CLIP's ModifiedResNet image tower (open_clip's is the same module and state dict): a 3-conv stem, four stages of Bottleneck
    blocks (planes w, 2w, 4w, 8w; expansion 4; anti-aliased strides by average pooling) and an AttentionPool2d head with one query
    (model_registry.py:16-140 in the reference)."""
    image_size: int
    layers: Tuple[int, int, int, int]
    width: int                 # w: the stem's output width
    out_dim: int
    preprocessor: Optional[str] = None   # (the OpenCLIP transform, as for the ViTs)
    pool: str = "resnet"
    quick_gelu: bool = False   # (kept so that the resolver can `replace` it; the image tower itself has no GELU)

    @property
    def heads(self) -> int:
        return 32 * self.width // 64

    @property
    def tokens(self) -> int:
        return (self.image_size // 32) ** 2 + 1

    @property
    def gflop_per_image(self) -> float:
        """2 MAC-FLOPs of every convolution, of the k / v projections of all tokens and of q / c_proj on token 0 (BN, ReLU, pooling and the
        attention scores not counted)."""
        S, w = self.image_size, self.width
        G = S // 2
        f = 2 * G * G * 9 * (3 * (w // 2) + (w // 2) * (w // 2) + (w // 2) * w)
        G //= 2
        inp = w
        for i, depth in enumerate(self.layers):
            P = w << i
            for j in range(depth):
                Go = G // 2 if (i > 0 and j == 0) else G
                f += 2 * G * G * inp * P + 2 * G * G * 9 * P * P + 2 * Go * Go * P * 4 * P
                if (i > 0 and j == 0) or inp != 4 * P:
                    f += 2 * Go * Go * inp * 4 * P
                G, inp = Go, 4 * P
        C, T = 32 * w, self.tokens
        f += 2 * T * 2 * C * C + 2 * C * C + 2 * C * self.out_dim
        return f / 1e9


@dataclass(frozen=True)
class ClipTextArch:
    vocab: int
    ctx: int
    width: int
    layers: int
    heads: int
    mlp_dim: int
    out_dim: int
    quick_gelu: bool = False
    ln_eps: float = 1e-5
    causal: bool = True       # False: SigLIP (no_causal_mask; every one of the ctx positions is run, pooled row = the last one)
    proj_bias: bool = False   # SigLIP: text_projection is a Linear with bias
    prefix: str = ""          # checkpoint key prefix: "" for CLIP, "text." under open_clip's CustomTextCLIP (SigLIP)
    pad_id: int = 0
    cls_embed: bool = False   # CoCa (open_clip TextTransformer embed_cls): ctx - 1 token positions + a learned class embedding appended behind the
    #                           padding (position ctx - 1); the class row is the pooled one, ln_final runs on it; keys under `text.`
    hf_tokenizer: Optional[str] = None   # open_clip HFTokenizer(<name>) instead of the CLIP BPE (CLIPA: "bert-base-uncased")
    strip_sep: bool = False              # HFTokenizer(strip_sep_token=True): [SEP] ids are replaced by 0 after tokenisation

    def gflop_per_text(self, tokens: Optional[int] = None) -> float:
        T, W, F = tokens or self.ctx, self.width, self.mlp_dim
        layer = 2 * T * W * (3 * W) + 2 * T * W * W + 2 * 2 * T * W * F + 4 * T * T * W
        return (self.layers * layer + 2 * W * self.out_dim) / 1e9


@dataclass(frozen=True)
class BertArch:
    vocab: int = 30522
    max_pos: int = 512
    width: int = 768
    layers: int = 12
    heads: int = 12
    mlp_dim: int = 3072
    ln_eps: float = 1e-12
    pos_offset: int = 0  # XLM-RoBERTa / RoBERTa checkpoints: position ids start at padding_idx + 1 = 2; max_pos counts USABLE positions
    # "NewModel" encoders (Alibaba-NLP/new-impl: stella_en_400M_v5 = the reference's hf_stella entry, gte-*-en-v1.5): rotary positions
    # instead of a learned table, packed qkv_proj, gated-GELU MLP (up_gate_proj [2F, W] without bias), post-LN
    rope_theta: Optional[float] = None       # None: learned absolute positions (BERT)
    rope_ntk_factor: Optional[float] = None  # rope_scaling {"type": "ntk", "factor": f}
    glu: bool = False
    type_vocab: int = 2
    # MPNet (sentence-transformers all-mpnet-base-*): the BERT post-LN encoder without token types, RoBERTa-style position offset, and one
    # T5-style relative-position bias table [rel_buckets, heads] shared by all layers (0 = no relative bias)
    rel_buckets: int = 0
    rel_max_distance: int = 128

    def rel_bias_table(self, weight):
        """`encoder.relative_attention_bias.weight` [rel_buckets, heads] -> fp32 [heads, 2 * max_pos - 1] indexed by (key - query) +
        max_pos - 1 and multiplied by sqrt(head_dim) (= divided by the softmax scale the attention kernel applies to the sum): MPNet's
        `compute_position_bias`, bucketed exactly as transformers' MPNetEncoder.relative_position_bucket (torch ops in the same order)."""
        import math
        import torch
        span = self.max_pos
        rel = torch.arange(-(span - 1), span, dtype=torch.long)           # key position - query position
        n = -rel
        nb = self.rel_buckets // 2
        ret = (n < 0).to(torch.long) * nb
        n = torch.abs(n)
        max_exact = nb // 2
        large = max_exact + (torch.log(n.float() / max_exact) / math.log(self.rel_max_distance / max_exact) * (nb - max_exact)).to(torch.long)
        large = torch.min(large, torch.full_like(large, nb - 1))
        bucket = ret + torch.where(n < max_exact, n, large)
        return (weight.detach().to(torch.float32)[bucket].t() * math.sqrt(self.width // self.heads)).contiguous()

    def rope_inv_freq(self):
        """[head_dim / 2] inverse frequencies exactly as NewModel builds them: base^-(2i/d); with NTK scaling the module re-derives
        its cache for max_pos * factor > max_pos at construction, which fixes base *= factor and inv_freq /= factor^(2/d) for every
        sequence length (NTKScalingRotaryEmbedding.__init__ -> _set_cos_sin_cache, mixed_b = None)."""
        import torch
        d = self.width // self.heads
        base = float(self.rope_theta) * (self.rope_ntk_factor or 1.0)
        inv = 1.0 / (base ** (torch.arange(0, d, 2, dtype=torch.float32) / d))
        if self.rope_ntk_factor:
            inv = inv / (self.rope_ntk_factor ** (2.0 / d))
        return inv

    def gflop_per_text(self, tokens: int) -> float:
        T, W, F = tokens, self.width, self.mlp_dim
        layer = 2 * T * W * (3 * W) + 2 * T * W * W + 2 * (3 if self.glu else 2) * T * W * F + 4 * T * T * W
        return self.layers * layer / 1e9


@dataclass(frozen=True)
class ModernBertArch:
    """transformers' ModernBertModel (model_type "modernbert"): pre-LN blocks without any bias, rotary positions with one base per layer kind, a
    gated-GELU MLP (mlp.Wi [2F, W] -> input, gate = chunk(2); Wo(gelu(input) * gate)), no attn_norm in layer 0, and `sliding` layers that attend
    only the keys within half_window = local_attention // 2 positions (inclusive on both sides)."""
    vocab: int = 50368
    max_pos: int = 8192
    width: int = 768
    layers: int = 22
    heads: int = 12
    mlp_dim: int = 1152
    ln_eps: float = 1e-5
    sliding: Tuple[bool, ...] = ()        # per layer: True = sliding_attention, False = full_attention
    half_window: int = 64
    theta_global: float = 160000.0
    theta_local: float = 10000.0

    def inv_freq(self, local: bool):
        """[head_dim / 2] inverse frequencies as ModernBertRotaryEmbedding.compute_default_rope_parameters builds them: base^-(2i/d)"""
        import torch
        d = self.width // self.heads
        base = self.theta_local if local else self.theta_global
        return 1.0 / (base ** (torch.arange(0, d, 2, dtype=torch.int64).to(torch.float32) / d))

    def gflop_per_text(self, tokens: int) -> float:
        T, W, F = tokens, self.width, self.mlp_dim
        full = 2 * T * W * (3 * W) + 2 * T * W * W + 2 * 3 * T * W * F
        attn = sum(4 * T * min(T, 2 * self.half_window + 1) * W if s else 4 * T * T * W for s in self.sliding)
        return (self.layers * full + attn) / 1e9


def modernbert_arch_from_hf_config(cfg: dict) -> ModernBertArch:
    """A local ModernBERT `config.json` -> ModernBertArch.  The layer kinds come from `layer_types`, else from `global_attn_every_n_layers` (layer i is
    full when i % n == 0); the rotary bases from `rope_parameters` {full_attention, sliding_attention}.rope_theta, else the older `global_rope_theta` /
    `local_rope_theta` keys, else 160000 / 10000."""
    for k in ("norm_bias", "attention_bias", "mlp_bias"):
        if cfg.get(k, False):
            raise KeyError(f"ModernBERT checkpoints with {k}=true are not supported (the tower runs bias-free blocks)")
    if cfg.get("hidden_activation", "gelu") != "gelu":
        raise KeyError(f"hidden_activation={cfg.get('hidden_activation')} unsupported")
    W, heads, layers = int(cfg["hidden_size"]), int(cfg["num_attention_heads"]), int(cfg["num_hidden_layers"])
    if heads < 1 or W != heads * 64:
        raise KeyError(f"ModernBERT runs 64-wide attention heads only: hidden_size / num_attention_heads = {W} / {heads} is not 64")
    F = int(cfg["intermediate_size"])
    if F % 64:
        raise KeyError(f"intermediate_size={F} must be a multiple of 64")
    kinds = cfg.get("layer_types")
    if kinds is None:
        n = int(cfg.get("global_attn_every_n_layers", 3))
        kinds = ["sliding_attention" if i % n else "full_attention" for i in range(layers)]
    if len(kinds) != layers or any(k not in ("full_attention", "sliding_attention") for k in kinds):
        raise KeyError(f"layer_types={kinds} must name full_attention / sliding_attention for each of the {layers} layers")
    rp = cfg.get("rope_parameters") or {}
    thetas = {}
    for kind, old, default in (("full_attention", "global_rope_theta", 160000.0), ("sliding_attention", "local_rope_theta", 10000.0)):
        sub = rp.get(kind) or {}
        if sub.get("rope_type", "default") != "default":
            raise KeyError(f"rope_parameters[{kind}].rope_type={sub.get('rope_type')} unsupported (default only)")
        thetas[kind] = float(sub.get("rope_theta", cfg.get(old, default)))
    if cfg.get("rope_scaling"):
        raise KeyError(f"rope_scaling={cfg.get('rope_scaling')} unsupported")
    return ModernBertArch(vocab=int(cfg["vocab_size"]), max_pos=min(int(cfg.get("max_position_embeddings", 8192)), 8192), width=W, layers=layers, heads=heads,
                          mlp_dim=F, ln_eps=float(cfg.get("norm_eps", 1e-5)), sliding=tuple(k == "sliding_attention" for k in kinds),
                          half_window=int(cfg.get("local_attention", 128)) // 2, theta_global=thetas["full_attention"],
                          theta_local=thetas["sliding_attention"])


@dataclass(frozen=True)
class QwenArch:
    """transformers' Qwen3Model / Qwen2Model (model_type "qwen3" / "qwen2") as the engine runs them: pre-norm decoder blocks with RMSNorm, `kv_heads` K/V
    heads shared by `heads` query heads (query head h reads K/V head h // (heads // kv_heads)), rotary positions, a gated-SiLU MLP and a causal mask.
    qk_norm: per-head RMSNorm of q and k in front of the rotary step (Qwen3); qkv_bias: biases on q / k / v_proj (Qwen2).  heads * head_dim need not be
    the width."""
    vocab: int = 151669
    max_pos: int = 8192
    width: int = 1024
    layers: int = 28
    heads: int = 16
    kv_heads: int = 8
    head_dim: int = 128
    mlp_dim: int = 3072
    rms_eps: float = 1e-6
    rope_theta: float = 1000000.0
    qk_norm: bool = True
    qkv_bias: bool = False

    def inv_freq(self):
        """[head_dim / 2] inverse frequencies as transformers' default rope initialisation builds them: theta^-(2i/d)"""
        import torch
        d = self.head_dim
        return 1.0 / (self.rope_theta ** (torch.arange(0, d, 2, dtype=torch.int64).to(torch.float32) / d))

    def gflop_per_text(self, tokens: int) -> float:
        T, W, F, A = tokens, self.width, self.mlp_dim, self.heads * self.head_dim
        layer = 2 * T * W * (A + 2 * self.kv_heads * self.head_dim) + 2 * T * A * W + 2 * 3 * T * W * F + 2 * T * T * A   # (causal: half of 4 T T A)
        return self.layers * layer / 1e9


def qwen_arch_from_hf_config(cfg: dict) -> QwenArch:
    """A local Qwen3 / Qwen2 `config.json` -> QwenArch.  rope_theta comes from `rope_parameters`, else the older top-level key.  Refused, each by the
    name of its key: a non-default rope_type, rope_scaling, use_sliding_window, layer_types other than full_attention, hidden_act other than silu,
    head_dim other than 64 / 128, hidden_size above 2048 (the 4B / 8B sizes)."""
    mtype = cfg.get("model_type")
    if mtype not in ("qwen3", "qwen2"):
        raise KeyError(f"model_type={mtype} is not a Qwen3 / Qwen2 model")
    if cfg.get("hidden_act", "silu") != "silu":
        raise KeyError(f"hidden_act={cfg.get('hidden_act')} unsupported (silu only)")
    rp = cfg.get("rope_parameters") or {}
    rtype = rp.get("rope_type", rp.get("type", "default"))
    if rtype != "default":
        raise KeyError(f"rope_parameters.rope_type={rtype} unsupported (default only)")
    if cfg.get("rope_scaling"):
        raise KeyError(f"rope_scaling={cfg.get('rope_scaling')} unsupported")
    if cfg.get("use_sliding_window", False):
        raise KeyError("use_sliding_window=true unsupported (full causal attention only)")
    W, heads, layers = int(cfg["hidden_size"]), int(cfg["num_attention_heads"]), int(cfg["num_hidden_layers"])
    kinds = cfg.get("layer_types")
    if kinds is not None and (len(kinds) != layers or any(k != "full_attention" for k in kinds)):
        raise KeyError(f"layer_types={kinds} unsupported (full_attention for each of the {layers} layers only)")
    kv = int(cfg.get("num_key_value_heads") or heads)
    if heads < 1 or kv < 1 or heads % kv:
        raise KeyError(f"num_attention_heads={heads} must be a multiple of num_key_value_heads={kv}")
    hd = int(cfg.get("head_dim") or W // heads)
    if hd not in (64, 128):
        raise KeyError(f"head_dim={hd} unsupported (64 or 128)")
    if W > 2048 or W % 64:
        raise KeyError(f"hidden_size={W} unsupported (a multiple of 64 up to 2048: the 4B / 8B sizes of this family are not served)")
    F = int(cfg["intermediate_size"])
    if F % 64:
        raise KeyError(f"intermediate_size={F} must be a multiple of 64")
    return QwenArch(vocab=int(cfg["vocab_size"]), max_pos=min(int(cfg.get("max_position_embeddings", 8192)), 8192), width=W, layers=layers, heads=heads,
                    kv_heads=kv, head_dim=hd, mlp_dim=F, rms_eps=float(cfg.get("rms_norm_eps", 1e-6)),
                    rope_theta=float(rp.get("rope_theta", cfg.get("rope_theta", 10000.0))), qk_norm=mtype == "qwen3",
                    qkv_bias=bool(cfg.get("attention_bias", mtype == "qwen2")))


@dataclass(frozen=True)
class LlamaArch:
    """transformers' MistralModel / LlamaModel (model_type "mistral" / "llama") as the engine runs them: QwenArch's block without q / k norm and without
    biases, up to 4096 wide.  window: Mistral's sliding_window — query i sees the keys j with i - window < j <= i — or None (no window: Llama, and the
    Mistral checkpoints whose config says null).  The defaults are Mistral-7B-v0.1's."""
    vocab: int = 32000
    max_pos: int = 8192
    width: int = 4096
    layers: int = 32
    heads: int = 32
    kv_heads: int = 8
    head_dim: int = 128
    mlp_dim: int = 14336
    rms_eps: float = 1e-5
    rope_theta: float = 10000.0
    window: Optional[int] = 4096
    qk_norm = False        # (the two switches tower_weights.qwen_state_dict reads: the tensors are Qwen's, minus the q / k norms and the biases)
    qkv_bias = False

    inv_freq = QwenArch.inv_freq

    def gflop_per_text(self, tokens: int) -> float:
        T, W, F, A = tokens, self.width, self.mlp_dim, self.heads * self.head_dim
        keys = min(T, self.window) if self.window else T
        layer = 2 * T * W * (A + 2 * self.kv_heads * self.head_dim) + 2 * T * A * W + 2 * 3 * T * W * F + 4 * T * keys * A - 2 * keys * keys * A
        return self.layers * layer / 1e9


def llama_arch_from_hf_config(cfg: dict) -> LlamaArch:
    """A local Mistral / Llama `config.json` -> LlamaArch.  rope_theta comes from `rope_parameters`, else the older top-level key.  Refused, each by the
    name of its key: rope_scaling or a non-default rope_type (Llama-3.1's llama3 scaling among them), hidden_act other than silu, attention_bias,
    mlp_bias, head_dim other than 64 / 128, hidden_size above 4096 or no multiple of 64, intermediate_size no multiple of 64, a sliding_window below 1.
    `sliding_window` null or absent: no window.  bert_arch_from_hf_config does not route here — it keeps refusing the two model types for the callers
    that run BERT-family encoders only (the cross-encoders); the `hf` loader selects them before it calls."""
    mtype = cfg.get("model_type")
    if mtype not in ("mistral", "llama"):
        raise KeyError(f"model_type={mtype} is not a Mistral / Llama model")
    if cfg.get("hidden_act", "silu") != "silu":
        raise KeyError(f"hidden_act={cfg.get('hidden_act')} unsupported (silu only)")
    rp = cfg.get("rope_parameters") or {}
    rtype = rp.get("rope_type", rp.get("type", "default"))
    if rtype != "default":
        raise KeyError(f"rope_parameters.rope_type={rtype} unsupported (default only)")
    if cfg.get("rope_scaling"):
        raise KeyError(f"rope_scaling={cfg.get('rope_scaling')} unsupported")
    if cfg.get("attention_bias", False):
        raise KeyError("attention_bias=true unsupported (bias-free projections only)")
    if cfg.get("mlp_bias", False):
        raise KeyError("mlp_bias=true unsupported (bias-free MLP only)")
    W, heads, layers = int(cfg["hidden_size"]), int(cfg["num_attention_heads"]), int(cfg["num_hidden_layers"])
    kv = int(cfg.get("num_key_value_heads") or heads)
    if heads < 1 or kv < 1 or heads % kv:
        raise KeyError(f"num_attention_heads={heads} must be a multiple of num_key_value_heads={kv}")
    hd = int(cfg.get("head_dim") or W // heads)
    if hd not in (64, 128):
        raise KeyError(f"head_dim={hd} unsupported (64 or 128)")
    if W > 4096 or W % 64:
        raise KeyError(f"hidden_size={W} unsupported (a multiple of 64 up to 4096)")
    F = int(cfg["intermediate_size"])
    if F % 64:
        raise KeyError(f"intermediate_size={F} must be a multiple of 64")
    window = cfg.get("sliding_window")
    if window is not None and (not isinstance(window, int) or isinstance(window, bool) or window < 1):
        raise KeyError(f"sliding_window={window} unsupported (a positive integer or null)")
    return LlamaArch(vocab=int(cfg["vocab_size"]), max_pos=min(int(cfg.get("max_position_embeddings", 8192)), 8192), width=W, layers=layers, heads=heads,
                     kv_heads=kv, head_dim=hd, mlp_dim=F, rms_eps=float(cfg.get("rms_norm_eps", 1e-6)),
                     rope_theta=float(rp.get("rope_theta", cfg.get("rope_theta", 10000.0))), window=window)


@dataclass(frozen=True)
class GemmaArch:
    """transformers' Gemma3TextModel with use_bidirectional_attention (model_type "gemma3_text": google/embeddinggemma-300m and its fine-tunes) as the
    engine runs it: blocks with an RMSNorm in front of and behind each sub-layer (weights applied as 1 + w), `kv_heads` K/V heads of width 256 shared by
    `heads` query heads, per-head q / k RMSNorm, rotary positions with one base per layer kind, a gated tanh-GELU MLP, the token table scaled by
    sqrt(width), no causal mask; `sliding` layers attend only the keys within half_window positions (inclusive on both sides)."""
    vocab: int = 262144
    max_pos: int = 2048
    width: int = 768
    layers: int = 24
    heads: int = 3
    kv_heads: int = 1
    head_dim: int = 256
    mlp_dim: int = 1152
    rms_eps: float = 1e-6
    sliding: Tuple[bool, ...] = ()        # per layer: True = sliding_attention, False = full_attention
    half_window: int = 256
    theta_global: float = 1000000.0
    theta_local: float = 10000.0
    query_pre_attn_scalar: float = 256.0

    @property
    def attn_scale(self) -> float:
        return float(self.query_pre_attn_scalar) ** -0.5

    def inv_freq(self, local: bool):
        """[head_dim / 2] inverse frequencies as transformers' default rope initialisation builds them: base^-(2i/d)"""
        import torch
        d = self.head_dim
        base = self.theta_local if local else self.theta_global
        return 1.0 / (base ** (torch.arange(0, d, 2, dtype=torch.int64).to(torch.float32) / d))

    def gflop_per_text(self, tokens: int) -> float:
        T, W, F, A = tokens, self.width, self.mlp_dim, self.heads * self.head_dim
        full = 2 * T * W * (A + 2 * self.kv_heads * self.head_dim) + 2 * T * A * W + 2 * 3 * T * W * F
        attn = sum(4 * T * min(T, 2 * self.half_window + 1) * A if s else 4 * T * T * A for s in self.sliding)
        return (self.layers * full + attn) / 1e9


def gemma_arch_from_hf_config(cfg: dict) -> GemmaArch:
    """A local EmbeddingGemma `config.json` (model_type "gemma3_text") -> GemmaArch.  The rotary bases come from the per-layer-type `rope_parameters`
    {full_attention, sliding_attention}.rope_theta of newer files, else from `rope_theta` / `rope_local_base_freq`, else 1e6 / 1e4; the layer kinds from
    `layer_types`, else from `sliding_window_pattern` (layer i is full when (i + 1) % pattern == 0, pattern 6 when absent).

    The window: the file says `sliding_window` (512 for the served checkpoint); transformers' Gemma3TextConfig turns that into sliding_window // 2 + 1 when
    use_bidirectional_attention is set and masks |i - j| < that, so half_window = sliding_window // 2 (256), inclusive.

    Refused, each by the name of its key: use_bidirectional_attention false or absent (the causal Gemma3 language models are not embedders), a non-null
    attn_logit_softcapping, rope_scaling or a non-default rope_type, head_dim other than 256, hidden_activation other than gelu_pytorch_tanh,
    max_position_embeddings above 8192, hidden_size above 2048."""
    mtype = cfg.get("model_type")
    if mtype != "gemma3_text":
        raise KeyError(f"model_type={mtype} is not a Gemma3 text model")
    if not cfg.get("use_bidirectional_attention", False):
        raise KeyError(f"use_bidirectional_attention={cfg.get('use_bidirectional_attention')} unsupported (the causal Gemma3 language models are not "
                       f"embedders: EmbeddingGemma checkpoints set it to true)")
    if cfg.get("attn_logit_softcapping") is not None:
        raise KeyError(f"attn_logit_softcapping={cfg.get('attn_logit_softcapping')} unsupported (null only)")
    act = cfg.get("hidden_activation", cfg.get("hidden_act", "gelu_pytorch_tanh"))
    if act != "gelu_pytorch_tanh":
        raise KeyError(f"hidden_activation={act} unsupported (gelu_pytorch_tanh only)")
    if cfg.get("rope_scaling"):
        raise KeyError(f"rope_scaling={cfg.get('rope_scaling')} unsupported")
    rp = cfg.get("rope_parameters") or {}
    thetas = {}
    for kind, old, default in (("full_attention", "rope_theta", 1000000.0), ("sliding_attention", "rope_local_base_freq", 10000.0)):
        sub = rp.get(kind) or {}
        rtype = sub.get("rope_type", sub.get("type", "default"))
        if rtype != "default" or sub.get("factor") is not None:
            raise KeyError(f"rope_parameters[{kind}].rope_type={rtype} unsupported (default, without scaling, only)")
        thetas[kind] = float(sub.get("rope_theta", cfg.get(old, default)))
    if rp.get("rope_type", rp.get("type", "default")) != "default" or rp.get("factor") is not None:
        raise KeyError(f"rope_parameters.rope_type={rp.get('rope_type', rp.get('type'))} unsupported (default, without scaling, only)")
    W, heads, layers = int(cfg["hidden_size"]), int(cfg["num_attention_heads"]), int(cfg["num_hidden_layers"])
    kv = int(cfg.get("num_key_value_heads") or heads)
    if heads < 1 or kv < 1 or heads % kv:
        raise KeyError(f"num_attention_heads={heads} must be a multiple of num_key_value_heads={kv}")
    hd = int(cfg.get("head_dim") or 256)
    if hd != 256:
        raise KeyError(f"head_dim={hd} unsupported (256 only)")
    if W > 2048 or W % 64:
        raise KeyError(f"hidden_size={W} unsupported (a multiple of 64 up to 2048)")
    F = int(cfg["intermediate_size"])
    if F % 64:
        raise KeyError(f"intermediate_size={F} must be a multiple of 64")
    max_pos = int(cfg.get("max_position_embeddings", 2048))
    if max_pos > 8192:
        raise KeyError(f"max_position_embeddings={max_pos} unsupported (at most 8192)")
    kinds = cfg.get("layer_types")
    if kinds is None:
        n = int(cfg.get("sliding_window_pattern", 6))
        kinds = ["sliding_attention" if (i + 1) % n else "full_attention" for i in range(layers)]
    if len(kinds) != layers or any(k not in ("full_attention", "sliding_attention") for k in kinds):
        raise KeyError(f"layer_types={kinds} must name full_attention / sliding_attention for each of the {layers} layers")
    sw = cfg.get("sliding_window", 4096)
    if any(k == "sliding_attention" for k in kinds) and (not isinstance(sw, int) or sw < 2):
        raise KeyError(f"sliding_window={sw} unsupported (an integer >= 2)")
    return GemmaArch(vocab=int(cfg["vocab_size"]), max_pos=max_pos, width=W, layers=layers, heads=heads, kv_heads=kv, head_dim=hd, mlp_dim=F,
                     rms_eps=float(cfg.get("rms_norm_eps", 1e-6)), sliding=tuple(k == "sliding_attention" for k in kinds),
                     half_window=int(sw) // 2 if isinstance(sw, int) else 0, theta_global=thetas["full_attention"],
                     theta_local=thetas["sliding_attention"], query_pre_attn_scalar=float(cfg.get("query_pre_attn_scalar", 256)))


@dataclass(frozen=True)
class GemmaCausalArch:
    """transformers' GemmaForCausalLM / GemmaModel (model_type "gemma": Gemma-2B, the body of BAAI/bge-reranker-v2-gemma) as the engine runs it: pre-norm
    decoder blocks with two RMSNorms (weights applied as 1 + w), `kv_heads` K/V heads of width 256 shared by `heads` query heads, rotary positions with
    one base, no q / k norm, no soft-capping, no sliding window, a gated tanh-GELU MLP, the token table scaled by sqrt(width), a causal mask."""
    vocab: int = 256000
    max_pos: int = 8192
    width: int = 2048
    layers: int = 18
    heads: int = 8
    kv_heads: int = 1
    head_dim: int = 256
    mlp_dim: int = 16384
    rms_eps: float = 1e-6
    rope_theta: float = 10000.0
    qk_norm: bool = False      # (the two switches qwen_state_dict reads: the tensors are Qwen's, minus the q / k norms and the biases)
    qkv_bias: bool = False

    @property
    def attn_scale(self) -> float:
        return float(self.head_dim) ** -0.5

    def inv_freq(self):
        """[head_dim / 2] inverse frequencies as transformers' default rope initialisation builds them: theta^-(2i/d)"""
        import torch
        d = self.head_dim
        return 1.0 / (self.rope_theta ** (torch.arange(0, d, 2, dtype=torch.int64).to(torch.float32) / d))

    def gflop_per_text(self, tokens: int) -> float:
        T, W, F, A = tokens, self.width, self.mlp_dim, self.heads * self.head_dim
        layer = 2 * T * W * (A + 2 * self.kv_heads * self.head_dim) + 2 * T * A * W + 2 * 3 * T * W * F + 2 * T * T * A   # (causal: half of 4 T T A)
        return self.layers * layer / 1e9


def gemma_causal_arch_from_hf_config(cfg: dict) -> GemmaCausalArch:
    """A local Gemma `config.json` (model_type "gemma") -> GemmaCausalArch.  rope_theta comes from `rope_parameters`, else the older top-level key.

    The activation: `hidden_activation` when the file has a non-null one, else `hidden_act`, else gelu_pytorch_tanh.  Only gelu_pytorch_tanh is served.
    The legacy spelling hidden_act="gelu" (with no hidden_activation) is REFUSED, because it does not name one function: transformers 4.39 .. 4.x ran
    the tanh form for it (with a warning), transformers 5.15 — the installed one — reads `hidden_act` alone and runs the erf form.

    Refused with a ValueError that names the key: model_type gemma2 / gemma3 / gemma3_text (and anything else), rope_scaling or a non-default rope_type,
    attention_bias true, another activation, head_dim other than 256, hidden_size above 2048 (the 7B), max_position_embeddings above 8192, a non-null
    attn_logit_softcapping / final_logit_softcapping / sliding_window (keys of the later families)."""
    mtype = cfg.get("model_type")
    if mtype in ("gemma2", "gemma3", "gemma3_text"):
        raise ValueError(f"model_type={mtype} is not served as a reranker (Gemma2 / Gemma3 are out of scope: only model_type 'gemma')")
    if mtype != "gemma":
        raise ValueError(f"model_type={mtype} is not a Gemma model")
    if cfg.get("rope_scaling"):
        raise ValueError(f"rope_scaling={cfg.get('rope_scaling')} unsupported")
    rp = cfg.get("rope_parameters") or {}
    rtype = rp.get("rope_type", rp.get("type", "default"))
    if rtype != "default" or rp.get("factor") is not None:
        raise ValueError(f"rope_parameters.rope_type={rtype} unsupported (default, without scaling, only)")
    if cfg.get("attention_bias", False):
        raise ValueError("attention_bias=true unsupported (bias-free projections only)")
    for key in ("attn_logit_softcapping", "final_logit_softcapping", "sliding_window"):
        if cfg.get(key) is not None:
            raise ValueError(f"{key}={cfg.get(key)} unsupported (a key of Gemma2 / Gemma3; null only)")
    key = "hidden_activation" if cfg.get("hidden_activation") is not None else "hidden_act"
    act = cfg.get(key, "gelu_pytorch_tanh")
    if act == "gelu" and key == "hidden_act":
        raise ValueError("hidden_act=gelu is ambiguous (transformers 4.x ran the tanh form for it, transformers 5 runs the erf form): write "
                         "hidden_activation=gelu_pytorch_tanh, what Gemma was trained with, into config.json")
    if act != "gelu_pytorch_tanh":
        raise ValueError(f"{key}={act} unsupported (gelu_pytorch_tanh only)")
    W, heads, layers = int(cfg["hidden_size"]), int(cfg["num_attention_heads"]), int(cfg["num_hidden_layers"])
    kv = int(cfg.get("num_key_value_heads") or heads)
    if heads < 1 or kv < 1 or heads % kv:
        raise ValueError(f"num_attention_heads={heads} must be a multiple of num_key_value_heads={kv}")
    hd = int(cfg.get("head_dim") or 256)
    if hd != 256:
        raise ValueError(f"head_dim={hd} unsupported (256 only)")
    if W > 2048 or W % 64:
        raise ValueError(f"hidden_size={W} unsupported (a multiple of 64 up to 2048: the 7B size of this family is not served)")
    F = int(cfg["intermediate_size"])
    if F % 64:
        raise ValueError(f"intermediate_size={F} must be a multiple of 64")
    max_pos = int(cfg.get("max_position_embeddings", 8192))
    if max_pos > 8192:
        raise ValueError(f"max_position_embeddings={max_pos} unsupported (at most 8192)")
    return GemmaCausalArch(vocab=int(cfg["vocab_size"]), max_pos=max_pos, width=W, layers=layers, heads=heads, kv_heads=kv, head_dim=hd, mlp_dim=F,
                           rms_eps=float(cfg.get("rms_norm_eps", 1e-6)), rope_theta=float(rp.get("rope_theta", cfg.get("rope_theta", 10000.0))))


@dataclass(frozen=True)
class T5Arch:
    """transformers' T5EncoderModel (model_type "t5": sentence-t5, gtr-t5, flan-t5 / T5 v1.1 encoder fine-tunes) as the engine runs it: pre-norm blocks with
    RMSNorms, bias-free Linears, `heads` attention heads of width head_dim (d_kv) whose total need not be `width` (d_model), no softmax scale, ONE
    relative-position bias table (block 0's) shared by every block, a ReLU MLP or (gated) a gated gelu_new one, no position table."""
    vocab: int = 32128
    max_pos: int = 8192                   # no position table: the longest sequence the attention kernel serves
    width: int = 768
    layers: int = 12
    heads: int = 12
    head_dim: int = 64
    mlp_dim: int = 3072
    rms_eps: float = 1e-6
    gated: bool = False                   # feed_forward_proj "gated-gelu" (T5 v1.1 / flan-t5)
    rel_buckets: int = 32
    max_distance: int = 128

    @property
    def inner(self) -> int:
        return self.heads * self.head_dim

    def bucket_of(self, relative_position):
        """transformers' T5Attention._relative_position_bucket(bidirectional=True), the same torch ops in the same order: int64 tensor of key - query ->
        int64 bucket ids"""
        import math
        import torch
        num_buckets = self.rel_buckets // 2
        relative_buckets = (relative_position > 0).to(torch.long) * num_buckets
        relative_position = torch.abs(relative_position)
        max_exact = num_buckets // 2
        is_small = relative_position < max_exact
        relative_position_if_large = max_exact + (
            torch.log(relative_position.float() / max_exact) / math.log(self.max_distance / max_exact) * (num_buckets - max_exact)
        ).to(torch.long)
        relative_position_if_large = torch.min(relative_position_if_large, torch.full_like(relative_position_if_large, num_buckets - 1))
        return relative_buckets + torch.where(is_small, relative_position, relative_position_if_large)

    def rel_bias_table(self, weight):
        """block 0's relative_attention_bias.weight [rel_buckets, heads] -> fp32 [heads, 2 D + 1], D = max_distance: entry (h, d + D) is the bias of
        key - query == d.  The bucket function is constant for |d| >= D, so the two ends stand for everything beyond (mq_attention_relbias clamps its
        index); that is checked here against the largest distance the engine serves."""
        import torch
        D = self.max_distance
        if tuple(weight.shape) != (self.rel_buckets, self.heads):
            raise ValueError(f"relative_attention_bias.weight {tuple(weight.shape)} is not [relative_attention_num_buckets={self.rel_buckets}, "
                             f"num_heads={self.heads}]")
        buckets = self.bucket_of(torch.arange(-D, D + 1, dtype=torch.long))
        far = self.bucket_of(torch.tensor([-self.max_pos, self.max_pos], dtype=torch.long))
        if int(buckets[0]) != int(far[0]) or int(buckets[-1]) != int(far[1]):
            raise ValueError(f"the bucket function of relative_attention_num_buckets={self.rel_buckets} / relative_attention_max_distance={D} is not "
                             f"constant from distance {D} on")
        return weight.detach().to(torch.float32)[buckets].t().contiguous()

    def gflop_per_text(self, tokens: int) -> float:
        T, W, F, A = tokens, self.width, self.mlp_dim, self.inner
        return self.layers * (2 * T * W * 3 * A + 2 * T * A * W + 4 * T * T * A + 2 * (3 if self.gated else 2) * T * W * F) / 1e9


def t5_arch_from_hf_config(cfg: dict) -> T5Arch:
    """A local T5 `config.json` (model_type "t5") -> T5Arch.  Refused, each by the name of its key: a feed_forward_proj other than relu / gated-gelu (or
    an is_gated_act / dense_act_fn that contradicts it), d_kv other than 64 / 128, d_model above 2048 or no multiple of 64, num_heads * d_kv above 4096,
    d_ff no multiple of 64, an odd relative_attention_num_buckets, relative_attention_max_distance outside [1, 1024]."""
    mtype = cfg.get("model_type")
    if mtype != "t5":
        raise KeyError(f"model_type={mtype} is not a T5 model")
    ffp = str(cfg.get("feed_forward_proj", "relu"))
    if ffp not in ("relu", "gated-gelu"):
        raise KeyError(f"feed_forward_proj={ffp} unsupported (relu or gated-gelu)")
    gated = ffp == "gated-gelu"
    if "is_gated_act" in cfg and bool(cfg["is_gated_act"]) != gated:
        raise KeyError(f"is_gated_act={cfg['is_gated_act']} contradicts feed_forward_proj={ffp}")
    act = cfg.get("dense_act_fn")
    if act is not None and act != ("gelu_new" if gated else "relu"):
        raise KeyError(f"dense_act_fn={act} unsupported with feed_forward_proj={ffp} ({'gelu_new' if gated else 'relu'} only)")
    W, hd, heads, F = int(cfg["d_model"]), int(cfg.get("d_kv", 64)), int(cfg["num_heads"]), int(cfg["d_ff"])
    if hd not in (64, 128):
        raise KeyError(f"d_kv={hd} unsupported (64 or 128)")
    if W > 2048 or W % 64 or W < 64:
        raise KeyError(f"d_model={W} unsupported (a multiple of 64 up to 2048)")
    if heads < 1 or heads * hd > 4096:
        raise KeyError(f"num_heads={heads} x d_kv={hd} unsupported (an inner width of at most 4096)")
    if F % 64 or F < 64:
        raise KeyError(f"d_ff={F} must be a multiple of 64")
    nb = int(cfg.get("relative_attention_num_buckets", 32))
    if nb < 4 or nb % 2:
        raise KeyError(f"relative_attention_num_buckets={nb} unsupported (an even number >= 4)")
    D = int(cfg.get("relative_attention_max_distance", 128))
    if not 1 <= D <= 1024 or D <= nb // 4:
        raise KeyError(f"relative_attention_max_distance={D} unsupported (above relative_attention_num_buckets / 4, at most 1024)")
    return T5Arch(vocab=int(cfg["vocab_size"]), width=W, layers=int(cfg["num_layers"]), heads=heads, head_dim=hd, mlp_dim=F,
                  rms_eps=float(cfg.get("layer_norm_epsilon", 1e-6)), gated=gated, rel_buckets=nb, max_distance=D)


@dataclass(frozen=True)
class JinaBertArch:
    """JinaBERT (jina-embeddings-v2-small-en / -base-en, their fine-tunes, MosaicBERT-style ALiBi encoders with the same block; config.json: model_type
    "bert" with position_embedding_type "alibi") as the engine runs it: post-LN blocks, Linears with biases, a bias-free gated erf-GELU MLP, no position
    table, a score bias of -slope_h |key - query|.  The block semantics restate the published architecture (the checkpoints are custom remote code)."""
    vocab: int = 30528
    max_pos: int = 8192                   # no position table: min(max_position_embeddings, what the attention kernel serves)
    width: int = 768
    layers: int = 12
    heads: int = 12
    head_dim: int = 64
    mlp_dim: int = 3072
    ln_eps: float = 1e-12
    type_vocab: int = 2

    def slopes(self) -> list:
        """the ALiBi slope of every head, in float64: for a power-of-two head count n, s = 2^(-8 / n) and head i gets s^(i + 1); otherwise, with p the
        largest power of two below n, the p slopes of p followed by the first n - p of slopes(2 p)[0::2]"""
        def pow2(n):
            s = 2.0 ** (-8.0 / n)
            return [s ** (i + 1) for i in range(n)]
        n = self.heads
        p = 1 << (n.bit_length() - 1)
        return pow2(n) if p == n else pow2(p) + pow2(2 * p)[0::2][:n - p]

    def gflop_per_text(self, tokens: int) -> float:
        T, W, F = tokens, self.width, self.mlp_dim
        return self.layers * (2 * T * W * 3 * W + 2 * T * W * W + 4 * T * T * W + 2 * 3 * T * W * F) / 1e9


def jina_bert_arch_from_hf_config(cfg: dict) -> JinaBertArch:
    """A local JinaBERT `config.json` (model_type "bert", position_embedding_type "alibi") -> JinaBertArch.  Refused, each by the name of its key: a
    feed_forward_type other than geglu, a hidden_act other than gelu, heads that are not 64 wide, a hidden_size above 2048, an intermediate_size that is no
    multiple of 64."""
    mtype, pet = cfg.get("model_type", "bert"), cfg.get("position_embedding_type", "absolute")
    if mtype != "bert" or pet != "alibi":
        raise KeyError(f"model_type={mtype} with position_embedding_type={pet} is not a JinaBERT model")
    fft = cfg.get("feed_forward_type", "original")
    if fft != "geglu":
        raise KeyError(f"feed_forward_type={fft} unsupported (geglu only)")
    if cfg.get("hidden_act", "gelu") != "gelu":
        raise KeyError(f"hidden_act={cfg.get('hidden_act')} unsupported (gelu only)")
    W, heads, F = int(cfg["hidden_size"]), int(cfg["num_attention_heads"]), int(cfg["intermediate_size"])
    if heads < 1 or W != heads * 64:
        raise KeyError(f"hidden_size={W} / num_attention_heads={heads} unsupported (64-wide heads only)")
    if W > 2048:
        raise KeyError(f"hidden_size={W} unsupported (at most 2048)")
    if F % 64 or F < 64:
        raise KeyError(f"intermediate_size={F} must be a multiple of 64")
    return JinaBertArch(vocab=int(cfg["vocab_size"]), max_pos=min(int(cfg.get("max_position_embeddings", 8192)), 8192), width=W,
                        layers=int(cfg["num_hidden_layers"]), heads=heads, mlp_dim=F, ln_eps=float(cfg.get("layer_norm_eps", 1e-12)),
                        type_vocab=int(cfg.get("type_vocab_size", 2)))


@dataclass(frozen=True)
class DebertaArch:
    """DeBERTa-v2 / -v3 (transformers DebertaV2Model, config.json model_type "deberta-v2") as the engine runs it for the one-label rerankers: post-LN BERT
    blocks with biases and an erf-GELU MLP, no position table and no type row, disentangled attention — content-to-content plus the c2p and p2c terms
    read from the projected, LayerNorm-ed `rel_embeddings` [2 span, W] through the log-bucket index of query - key — and a ContextPooler head."""
    vocab: int = 128100
    max_pos: int = 8192                   # no position table: what the attention kernel serves
    width: int = 768
    layers: int = 12
    heads: int = 12
    head_dim: int = 64
    mlp_dim: int = 3072
    ln_eps: float = 1e-7
    span: int = 256                       # S = position_buckets: rel_embeddings has 2 S rows
    max_rel: int = 512                    # max_relative_positions (below 1 in the config: max_position_embeddings)
    share_att_key: bool = True            # the position tables go through key_proj / query_proj (false: pos_key_proj / pos_query_proj)

    def idx_table(self, reach: int):
        """int32 [2 reach + 1]: entry d + reach = clamp(span + b(d), 0, 2 span - 1), b = the log bucket of the distance d = query - key — the row of the
        position tables both disentangled terms read.  The arithmetic is the modelling code's own, step for step in its dtypes (the integer quotient and
        the logarithms in fp32): a ceil(log(.)) formed in another precision moves a bucket with one ulp.  The kernel needs the table non-decreasing
        (a call touches only the window between the buckets of its longest sequence's two ends): checked here."""
        import torch
        S, mid = self.span, self.span // 2
        d = torch.arange(-int(reach), int(reach) + 1, dtype=torch.long)
        sign = torch.sign(d)
        a = torch.where((d < mid) & (d > -mid), torch.tensor(mid - 1).type_as(d), torch.abs(d))
        log_pos = torch.ceil(torch.log(a / mid) / torch.log(torch.tensor((self.max_rel - 1) / mid)) * (mid - 1)) + mid
        b = torch.where(a <= mid, d.type_as(log_pos), log_pos * sign).to(torch.long)
        t = (b + S).clamp(0, 2 * S - 1).to(torch.int32)
        if bool((t[1:] < t[:-1]).any()):
            raise ValueError(f"position_buckets={S} with max_relative_positions={self.max_rel}: the bucket index is not monotone in the distance")
        return t

    def gflop_per_text(self, tokens: int) -> float:
        T, W, F = tokens, self.width, self.mlp_dim
        win = min(2 * self.span, 2 * T - 1)
        return self.layers * (2 * T * W * 3 * W + 2 * T * W * W + 4 * T * T * W + 4 * T * win * W + 2 * 2 * T * W * F) / 1e9


def deberta_arch_from_hf_config(cfg: dict) -> DebertaArch:
    """A local DeBERTa-v2 / -v3 `config.json` -> DebertaArch.  Refused, each with a ValueError that names its key: model_type other than deberta-v2
    (DeBERTa v1 has another attention), relative_attention false, pos_att_type other than exactly {c2p, p2c}, position_biased_input true,
    conv_kernel_size > 0, norm_rel_ebd other than layer_norm, type_vocab_size > 0, embedding_size != hidden_size, pooler_hidden_size != hidden_size,
    pooler_hidden_act / hidden_act other than gelu, heads that are not 64 wide, hidden_size above 2048, position_buckets outside [2, 1024] (1: the
    bucket formula divides by position_buckets // 2), max_relative_positions too small for the log buckets, an intermediate_size that is no multiple
    of 64."""
    mtype = cfg.get("model_type")
    if mtype != "deberta-v2":
        raise ValueError(f"model_type={mtype!r} is not served (DeBERTa-v2 / -v3 only: model_type 'deberta-v2'; DeBERTa v1 has another attention)")
    if not cfg.get("relative_attention", False):
        raise ValueError("relative_attention=false is not served (the tower runs disentangled attention only)")
    pat = cfg.get("pos_att_type") or []
    if isinstance(pat, str):
        pat = [x.strip() for x in pat.lower().split("|") if x.strip()]
    if sorted(pat) != ["c2p", "p2c"]:
        raise ValueError(f"pos_att_type={cfg.get('pos_att_type')!r} is not served (exactly c2p and p2c)")
    if cfg.get("position_biased_input", True):
        raise ValueError("position_biased_input=true is not served (no absolute position table is added)")
    if int(cfg.get("conv_kernel_size", 0) or 0) > 0:
        raise ValueError(f"conv_kernel_size={cfg.get('conv_kernel_size')} is not served (no convolution layer)")
    nre = cfg.get("norm_rel_ebd", "none")
    if [x.strip() for x in str(nre).lower().split("|")] != ["layer_norm"]:
        raise ValueError(f"norm_rel_ebd={nre!r} is not served (layer_norm only)")
    if int(cfg.get("type_vocab_size", 0) or 0) > 0:
        raise ValueError(f"type_vocab_size={cfg.get('type_vocab_size')} is not served (no token-type row is added)")
    W, heads, F = int(cfg["hidden_size"]), int(cfg["num_attention_heads"]), int(cfg["intermediate_size"])
    if int(cfg.get("embedding_size", W) or W) != W:
        raise ValueError(f"embedding_size={cfg.get('embedding_size')} != hidden_size={W} is not served (no embedding projection)")
    if int(cfg.get("pooler_hidden_size", W) or W) != W:
        raise ValueError(f"pooler_hidden_size={cfg.get('pooler_hidden_size')} != hidden_size={W} is not served")
    if cfg.get("pooler_hidden_act", "gelu") != "gelu":
        raise ValueError(f"pooler_hidden_act={cfg.get('pooler_hidden_act')!r} is not served (gelu only)")
    if cfg.get("hidden_act", "gelu") != "gelu":
        raise ValueError(f"hidden_act={cfg.get('hidden_act')!r} is not served (gelu only)")
    if heads < 1 or W != heads * 64:
        raise ValueError(f"hidden_size={W} / num_attention_heads={heads} is not served (64-wide heads only)")
    if W > 2048:
        raise ValueError(f"hidden_size={W} is not served (at most 2048)")
    if F % 64 or F < 64:
        raise ValueError(f"intermediate_size={F} must be a multiple of 64")
    S = int(cfg.get("position_buckets", -1))
    if S < 2 or S > 1024:
        raise ValueError(f"position_buckets={S} is not served (2 .. 1024)")
    max_rel = int(cfg.get("max_relative_positions", -1))
    if max_rel < 1:
        max_rel = int(cfg["max_position_embeddings"])
    if max_rel - 1 <= S // 2:
        raise ValueError(f"max_relative_positions={max_rel} is not served with position_buckets={S} (the log buckets need max_relative_positions - 1 > "
                         f"position_buckets // 2)")
    return DebertaArch(vocab=int(cfg["vocab_size"]), max_pos=8192, width=W, layers=int(cfg["num_hidden_layers"]), heads=heads, mlp_dim=F,
                       ln_eps=float(cfg.get("layer_norm_eps", 1e-7)), span=S, max_rel=max_rel, share_att_key=bool(cfg.get("share_att_key", False)))


@dataclass(frozen=True)
class NomicBertArch:
    """NomicBERT (nomic-embed-text-v1 / -v1.5 / -v1-unsupervised, their fine-tunes, snowflake-arctic-embed-m-long; transformers NomicBertModel,
    model_type "nomic_bert") as the engine runs it: post-LN blocks with biased LayerNorms, bias-free Linears, a gated-SiLU MLP, full-width rotate-half
    rotary positions, a token-type row, no position table, plain bidirectional attention."""
    vocab: int = 30528
    max_pos: int = 8192                   # no position table: min(max_position_embeddings, what the attention kernel serves)
    width: int = 768
    layers: int = 12
    heads: int = 12
    head_dim: int = 64
    mlp_dim: int = 3072
    ln_eps: float = 1e-12
    type_vocab: int = 2
    rope_theta: float = 1000.0

    def inv_freq(self):
        """[head_dim / 2] inverse frequencies as NomicBertRotaryEmbedding.compute_default_rope_parameters builds them: theta^-(2i/d), in the plain
        order mq_rope reads (dims i and i + head_dim / 2 share entry i)"""
        import torch
        d = self.head_dim
        return 1.0 / (self.rope_theta ** (torch.arange(0, d, 2, dtype=torch.int64).to(torch.float32) / d))

    def gflop_per_text(self, tokens: int) -> float:
        T, W, F = tokens, self.width, self.mlp_dim
        return self.layers * (2 * T * W * 3 * W + 2 * T * W * W + 4 * T * T * W + 2 * 3 * T * W * F) / 1e9


# the hub's original NomicBERT config.json is GPT-2-style: its key -> transformers' key
_NOMIC_HUB_ALIASES = {"n_embd": "hidden_size", "n_head": "num_attention_heads", "n_layer": "num_hidden_layers", "n_inner": "intermediate_size",
                      "n_positions": "max_position_embeddings", "layer_norm_epsilon": "layer_norm_eps"}


def nomic_bert_arch_from_hf_config(cfg: dict) -> NomicBertArch:
    """A local NomicBERT `config.json` (model_type "nomic_bert") -> NomicBertArch, in either of two dialects.

    transformers' own keys (NomicBertConfig): hidden_size, num_hidden_layers, num_attention_heads, intermediate_size, hidden_act, max_position_embeddings,
    type_vocab_size, layer_norm_eps, rope_parameters {rope_theta, rope_type}, head_dim.  Refused, each by the name of its key: a hidden_act other than
    silu, a rope_parameters.rope_type other than default (dynamic / NTK scaling), a head_dim other than 64 or heads that are not 64 wide, a hidden_size
    above 2048, an intermediate_size that is no multiple of 64.  max_position_embeddings above 8192 is clamped to 8192.

    The hub's original GPT-2-style keys, taken when `hidden_size` is absent and `n_embd` is there — UNVERIFIED against a real hub file: the table is
    written from memory of the published checkpoints' config.json, no such file was at hand: n_embd, n_head, n_layer, n_inner (null: 4 n_embd),
    n_positions, layer_norm_epsilon, rotary_emb_base, rotary_emb_fraction, rotary_emb_interleaved, rotary_scaling_factor, activation_function,
    qkv_proj_bias, mlp_fc1_bias, mlp_fc2_bias, prenorm, use_rms_norm.  Refused by name: a bias set true, prenorm, use_rms_norm, rotary_emb_fraction
    other than 1, rotary_emb_interleaved, a non-null rotary_scaling_factor, an activation_function other than swiglu.  In both dialects the
    mixture-of-experts keys of nomic-embed-text-v2-moe (moe_every_n_layers > 0, num_experts > 1) are refused."""
    mtype = cfg.get("model_type")
    if mtype != "nomic_bert":
        raise KeyError(f"model_type={mtype} is not a NomicBERT model")
    if int(cfg.get("moe_every_n_layers") or 0) > 0:
        raise KeyError(f"moe_every_n_layers={cfg['moe_every_n_layers']} unsupported (mixture-of-experts NomicBERT, nomic-embed-text-v2-moe, is not served)")
    if int(cfg.get("num_experts") or 0) > 1:
        raise KeyError(f"num_experts={cfg['num_experts']} unsupported (mixture-of-experts NomicBERT, nomic-embed-text-v2-moe, is not served)")
    theta = 1000.0
    if "hidden_size" not in cfg and "n_embd" in cfg:
        for k in ("qkv_proj_bias", "mlp_fc1_bias", "mlp_fc2_bias"):
            if cfg.get(k, False):
                raise KeyError(f"{k}={cfg[k]} unsupported (the served block's Linears have no bias)")
        if cfg.get("prenorm", False):
            raise KeyError(f"prenorm={cfg['prenorm']} unsupported (post-LN blocks only)")
        if cfg.get("use_rms_norm", False):
            raise KeyError(f"use_rms_norm={cfg['use_rms_norm']} unsupported (LayerNorm only)")
        if float(cfg.get("rotary_emb_fraction", 1.0)) != 1.0:
            raise KeyError(f"rotary_emb_fraction={cfg['rotary_emb_fraction']} unsupported (the whole head is rotated)")
        if cfg.get("rotary_emb_interleaved", False):
            raise KeyError(f"rotary_emb_interleaved={cfg['rotary_emb_interleaved']} unsupported (rotate_half pairs only)")
        if cfg.get("rotary_scaling_factor") is not None:
            raise KeyError(f"rotary_scaling_factor={cfg['rotary_scaling_factor']} unsupported (dynamic NTK rope scaling is not served)")
        act = cfg.get("activation_function", "swiglu")
        if act != "swiglu":
            raise KeyError(f"activation_function={act} unsupported (swiglu only)")
        theta = float(cfg.get("rotary_emb_base", 1000.0))
        hub = cfg
        cfg = {k: v for k, v in hub.items() if k not in _NOMIC_HUB_ALIASES}
        cfg.update({new: hub[old] for old, new in _NOMIC_HUB_ALIASES.items() if hub.get(old) is not None})
        cfg.setdefault("intermediate_size", 4 * int(hub["n_embd"]))
        cfg["hidden_act"] = "silu"
    else:
        if cfg.get("hidden_act", "silu") != "silu":
            raise KeyError(f"hidden_act={cfg.get('hidden_act')} unsupported (silu only)")
        rp = cfg.get("rope_parameters") or {}
        rtype = rp.get("rope_type", rp.get("type", "default"))
        if rtype != "default":
            raise KeyError(f"rope_parameters.rope_type={rtype} unsupported (default only: dynamic / NTK rope scaling is not served)")
        theta = float(rp.get("rope_theta", cfg.get("rope_theta", 1000.0)))
    W, heads, F = int(cfg["hidden_size"]), int(cfg["num_attention_heads"]), int(cfg["intermediate_size"])
    hd = cfg.get("head_dim")
    if hd is not None and int(hd) != 64:
        raise KeyError(f"head_dim={hd} unsupported (64 only)")
    if heads < 1 or W != heads * 64:
        raise KeyError(f"hidden_size={W} / num_attention_heads={heads} unsupported (64-wide heads only)")
    if W > 2048:
        raise KeyError(f"hidden_size={W} unsupported (at most 2048)")
    if F % 64 or F < 64:
        raise KeyError(f"intermediate_size={F} must be a multiple of 64")
    if not theta > 0:
        raise KeyError(f"rope_theta={theta} must be positive")
    return NomicBertArch(vocab=int(cfg["vocab_size"]), max_pos=min(int(cfg.get("max_position_embeddings", 2048)), 8192), width=W,
                         layers=int(cfg["num_hidden_layers"]), heads=heads, mlp_dim=F, ln_eps=float(cfg.get("layer_norm_eps", 1e-12)),
                         type_vocab=int(cfg.get("type_vocab_size", 2)), rope_theta=theta)


@dataclass(frozen=True)
class JinaV3Arch:
    """jina-embeddings-v3 (transformers JinaEmbeddingsV3Model, model_type "jina_embeddings_v3") as the engine runs it: the NomicBERT block with biases on
    its four Linears and a plain fc1 -> erf-GELU -> fc2 MLP; post-LN, full-width rotate-half rotary positions, row 0 of the token-type table, no position
    table, plain bidirectional attention.  The task adapters are not part of the arch (engine/jina_v3.py::load_adapters)."""
    vocab: int = 250002
    max_pos: int = 8192                   # no position table: min(max_position_embeddings - 2, what the attention kernel serves)
    width: int = 1024
    layers: int = 24
    heads: int = 16
    head_dim: int = 64
    mlp_dim: int = 4096
    ln_eps: float = 1e-5
    type_vocab: int = 1
    rope_theta: float = 20000.0

    def inv_freq(self):
        """[head_dim / 2] inverse frequencies of the default rope parameters: theta^-(2i/d), in the plain order mq_rope reads"""
        import torch
        d = self.head_dim
        return 1.0 / (self.rope_theta ** (torch.arange(0, d, 2, dtype=torch.int64).to(torch.float32) / d))

    def gflop_per_text(self, tokens: int) -> float:
        T, W, F = tokens, self.width, self.mlp_dim
        return self.layers * (2 * T * W * 3 * W + 2 * T * W * W + 4 * T * T * W + 2 * 2 * T * W * F) / 1e9


def resolve_jina_v3(cfg: dict) -> JinaV3Arch:
    """A local `config.json` with model_type "jina_embeddings_v3" (transformers' JinaEmbeddingsV3Config keys: hidden_size, num_hidden_layers,
    num_attention_heads, intermediate_size, hidden_act, max_position_embeddings, type_vocab_size, layer_norm_eps, rope_parameters {rope_theta, rope_type})
    -> JinaV3Arch.  Refused, each by the name of its key: a hidden_act other than gelu, a rope_parameters.rope_type other than default, heads that are
    not 64 wide, a hidden_size above 2048, an intermediate_size that is no multiple of 64.  rope_theta defaults to 20000.  The longest sequence is
    min(max_position_embeddings - 2, 8192): the checkpoint's 8194 counts the two XLM-RoBERTa offset positions."""
    mtype = cfg.get("model_type")
    if mtype != "jina_embeddings_v3":
        raise KeyError(f"model_type={mtype} is not a Jina v3 model")
    if cfg.get("hidden_act", "gelu") != "gelu":
        raise KeyError(f"hidden_act={cfg.get('hidden_act')} unsupported (gelu only)")
    rp = cfg.get("rope_parameters") or {}
    rtype = rp.get("rope_type", rp.get("type", "default"))
    if rtype != "default":
        raise KeyError(f"rope_parameters.rope_type={rtype} unsupported (default only: rope scaling is not served)")
    theta = float(rp.get("rope_theta", cfg.get("rope_theta", 20000.0)))
    if not theta > 0:
        raise KeyError(f"rope_theta={theta} must be positive")
    W, heads, F = int(cfg["hidden_size"]), int(cfg["num_attention_heads"]), int(cfg["intermediate_size"])
    if heads < 1 or W != heads * 64:
        raise KeyError(f"hidden_size={W} / num_attention_heads={heads} unsupported (64-wide heads only)")
    if W > 2048:
        raise KeyError(f"hidden_size={W} unsupported (at most 2048)")
    if F % 64 or F < 64:
        raise KeyError(f"intermediate_size={F} must be a multiple of 64")
    max_pos = int(cfg.get("max_position_embeddings", 8194)) - 2
    if max_pos < 1:
        raise KeyError(f"max_position_embeddings={cfg.get('max_position_embeddings')} leaves no position (it counts two offset positions)")
    return JinaV3Arch(vocab=int(cfg["vocab_size"]), max_pos=min(max_pos, 8192), width=W, layers=int(cfg["num_hidden_layers"]), heads=heads, mlp_dim=F,
                      ln_eps=float(cfg.get("layer_norm_eps", 1e-5)), type_vocab=int(cfg.get("type_vocab_size", 1)), rope_theta=theta)


@dataclass(frozen=True)
class HfClipTextArch:
    """open_clip's HFTextEncoder text tower (CustomTextCLIP checkpoints `text.transformer.*` + `text.proj.*`): a Hugging Face encoder
    (XLM-RoBERTa here), masked-mean pooler, projection MLP Linear(W, hidden) -> GELU -> Linear(hidden, out_dim) without biases,
    hidden = (W + out_dim) // 2 (open_clip hf_model.py: proj "mlp", pooler "mean_pooler").  Texts are tokenised by the HF tokenizer
    padded to ctx = 77 with <pad>; attention mask = ids != pad_id."""
    bert: "BertArch"
    out_dim: int
    ctx: int = 77
    pad_id: int = 1
    quick_gelu: bool = False   # (the towers' activation is the HF encoder's own GELU; kept so that resolve_open_clip can `replace` it)
    causal: bool = False

    @property
    def proj_hidden(self) -> int:
        return (self.bert.width + self.out_dim) // 2

    @property
    def vocab(self) -> int:
        return self.bert.vocab

    @property
    def width(self) -> int:
        return self.bert.width

    def gflop_per_text(self, tokens: Optional[int] = None) -> float:
        return self.bert.gflop_per_text(tokens or self.ctx) + 2 * (self.bert.width + self.out_dim) * self.proj_hidden / 1e9


@dataclass(frozen=True)
class NllbTextArch:
    """The NLLB-CLIP text tower (hf-hub:visheratin/nllb-clip-*-siglip, model_registry.py:510-533 in the reference): open_clip's HFTextEncoder
    over the ENCODER of facebook/nllb-200-distilled-600M (12 layers, FFN 4096) / -1.3B (24 layers, FFN 8192) — a transformers M2M100 encoder:
    pre-LN blocks with a key-padding mask and a ReLU MLP, token embeddings scaled by sqrt(width), sinusoidal positions (first token at
    position padding_idx + 1 = 2), a final LayerNorm — then `cls_pooler` (position 0: the language-code token) and a `linear` projection without
    bias.  Checkpoint keys `text.transformer.{embed_tokens, layers.N.*, layer_norm}` + `text.proj.weight`.  Rows are
    [lang code] pieces + 1 ... </s> = 2, padded with <pad> = 1 to ctx; only the un-padded rows run."""
    vocab: int = 256206
    ctx: int = 77
    width: int = 1024
    layers: int = 12
    heads: int = 16
    mlp_dim: int = 4096
    out_dim: int = 768
    pad_id: int = 1
    ln_eps: float = 1e-5
    pos_offset: int = 2        # M2M100SinusoidalPositionalEmbedding: `offset` = 2 rows in front of the table, first token at padding_idx + 1
    src_lang: str = "eng_Latn"  # what open_clip's HFTokenizer gets from NllbTokenizer without a `src_lang`
    hf_model_name: str = "facebook/nllb-200-distilled-600M"

    def position_table(self):
        """fp32 [ctx, width]: row i = the sinusoidal embedding of position pos_offset + i, transformers' M2M100SinusoidalPositionalEmbedding.get_embedding
        (the torch ops in their order): half = width // 2 frequencies exp(-k * ln(10000) / (half - 1)), [sin | cos] halves.  A non-persistent buffer
        there, so no checkpoint carries it."""
        import math
        import torch
        half = self.width // 2
        emb = math.log(10000) / (half - 1)
        emb = torch.exp(torch.arange(half, dtype=torch.int64).float() * -emb)
        emb = torch.arange(self.pos_offset + self.ctx, dtype=torch.int64).float().unsqueeze(1) * emb.unsqueeze(0)
        emb = torch.cat([torch.sin(emb), torch.cos(emb)], dim=1).view(self.pos_offset + self.ctx, -1)
        if self.width % 2 == 1:
            emb = torch.cat([emb, torch.zeros(self.pos_offset + self.ctx, 1)], dim=1)
        return emb[self.pos_offset:].contiguous()

    def gflop_per_text(self, tokens: Optional[int] = None) -> float:
        T, W, F = tokens or self.ctx, self.width, self.mlp_dim
        layer = 2 * T * W * (3 * W) + 2 * T * W * W + 2 * 2 * T * W * F + 4 * T * T * W
        return (self.layers * layer + 2 * W * self.out_dim) / 1e9


_NLLB_BASE = NllbTextArch(layers=12, mlp_dim=4096, out_dim=768, hf_model_name="facebook/nllb-200-distilled-600M")
_NLLB_LARGE = NllbTextArch(layers=24, mlp_dim=8192, out_dim=1152, hf_model_name="facebook/nllb-200-distilled-1.3B")
NLLB_TEXT_ARCHS = {a.hf_model_name: a for a in (_NLLB_BASE, _NLLB_LARGE)}

_TEXT_B = ClipTextArch(vocab=49408, ctx=77, width=512, layers=12, heads=8, mlp_dim=2048, out_dim=512)
_TEXT_L = ClipTextArch(vocab=49408, ctx=77, width=768, layers=12, heads=12, mlp_dim=3072, out_dim=768)
_TEXT_B_PLUS = ClipTextArch(vocab=49408, ctx=77, width=640, layers=12, heads=10, mlp_dim=2560, out_dim=640)
_TEXT_H = ClipTextArch(vocab=49408, ctx=77, width=1024, layers=24, heads=16, mlp_dim=4096, out_dim=1024)
_TEXT_BIGG = ClipTextArch(vocab=49408, ctx=77, width=1280, layers=32, heads=20, mlp_dim=5120, out_dim=1280)

# SigLIP (open_clip model configs ViT-{B,L}-16-SigLIP*: timm vit_{base,large}_patch16_siglip_* + TextTransformer, ctx 64,
# 32k sentencepiece vocabulary, LayerNorm eps 1e-6 everywhere)
def _siglip(image_size: int, large: bool = False, so400m: bool = False) -> Tuple[VitArch, ClipTextArch]:
    W, Lyr, H, Fd = (1024, 24, 16, 4096) if large else (768, 12, 12, 3072)
    if so400m:  # shape-optimised 400M: 72-wide heads (run as 96), MLP 4304 (zero-padded to 4352 at load), patch 14
        W, Lyr, H, Fd = 1152, 27, 16, 4304
    return (VitArch(image_size, 14 if so400m else 16, W, Lyr, H, Fd, W, ln_eps=1e-6, pool="map"),
            ClipTextArch(vocab=32000, ctx=64, width=W, layers=Lyr, heads=H, mlp_dim=Fd, out_dim=W, ln_eps=1e-6, causal=False,
                         proj_bias=True, prefix="text.", pad_id=1))


# open_clip architecture name -> (vision, text)
OPEN_CLIP_ARCHS = {
    "ViT-B-32": (VitArch(224, 32, 768, 12, 12, 3072, 512), _TEXT_B),
    "ViT-B-32-256": (VitArch(256, 32, 768, 12, 12, 3072, 512), _TEXT_B),
    "ViT-B-16": (VitArch(224, 16, 768, 12, 12, 3072, 512), _TEXT_B),
    "ViT-B-16-plus-240": (VitArch(240, 16, 896, 12, 14, 3584, 640), _TEXT_B_PLUS),
    "ViT-L-14": (VitArch(224, 14, 1024, 24, 16, 4096, 768), _TEXT_L),
    "ViT-L-14-336": (VitArch(336, 14, 1024, 24, 16, 4096, 768), _TEXT_L),
    # 16 heads of 80 / 88 / 104: zero-padded to 96 / 96 / 112-wide heads at load (engine/tower_weights.py::_pad_heads)
    "ViT-H-14": (VitArch(224, 14, 1280, 32, 16, 5120, 1024), _TEXT_H),
    # CLIPs with a Hugging Face text tower: the ViT towers above with a RoBERTa / XLM-RoBERTa encoder (open_clip model configs
    # roberta-ViT-B-32, xlm-roberta-base-ViT-B-32, xlm-roberta-large-ViT-H-14; model_registry.py:257-273 in the reference)
    # CLIPA (open_clip ViT-L-14-CLIPA-336: no ln_pre, average pooling of the patch tokens with the final LayerNorm after it; unmasked text
    # tower with last-position pooling over bert-base-uncased WordPiece ids without [SEP], 32 positions; bilinear-squash preprocessing)
    "ViT-L-14-CLIPA-336": (VitArch(336, 14, 1024, 24, 16, 4096, 768, pool="avg", ln_pre=False, preprocessor="CLIPA"),
                           ClipTextArch(vocab=32000, ctx=32, width=768, layers=12, heads=12, mlp_dim=3072, out_dim=768, causal=False,
                                        hf_tokenizer="bert-base-uncased", strip_sep=True)),
    "roberta-ViT-B-32": (VitArch(224, 32, 768, 12, 12, 3072, 512, quick_gelu=True), "roberta-base:512"),   # (its model config sets quick_gelu)
    "xlm-roberta-base-ViT-B-32": (VitArch(224, 32, 768, 12, 12, 3072, 512), "xlmr-base:512"),
    "xlm-roberta-large-ViT-H-14": (VitArch(224, 14, 1280, 32, 16, 5120, 1024), "xlmr-large:1024"),
    "ViT-H-14-378": (VitArch(378, 14, 1280, 32, 16, 5120, 1024), _TEXT_H),  # 730 tokens: K / V stream through the LDS in pieces
    "ViT-g-14": (VitArch(224, 14, 1408, 40, 16, 6144, 1024), _TEXT_H),
    "ViT-bigG-14": (VitArch(224, 14, 1664, 48, 16, 8192, 1280), _TEXT_BIGG),
    # CoCa (model_registry.py:344-370; open_clip model configs coca_ViT-B-32 / coca_ViT-L-14): the contrastive half — the captioning decoder is not
    # part of an embedding
    "coca_ViT-B-32": (VitArch(224, 32, 768, 12, 12, 3072, 512, pool="query", pool_heads=8),
                      ClipTextArch(49408, 77, 512, 12, 8, 2048, 512, prefix="text.", cls_embed=True)),
    "coca_ViT-L-14": (VitArch(224, 14, 1024, 24, 16, 4096, 768, pool="query", pool_heads=8),
                      ClipTextArch(49408, 77, 768, 12, 12, 3072, 768, prefix="text.", cls_embed=True)),
    # EVA02-CLIP (model_registry.py:441-460; open_clip model configs EVA02-B-16 / EVA02-L-14 / EVA02-L-14-336: timm trunks eva02_base_patch16_clip_224,
    # eva02_large_patch14_clip_224 / _336; custom_text towers of the CLIP form under `text.`)
    "EVA02-B-16": (VitArch(224, 16, 768, 12, 12, 2048, 512, ln_eps=1e-6, ln_pre=False, eva=True),
                   ClipTextArch(49408, 77, 512, 12, 8, 2048, 512, prefix="text.")),
    "EVA02-L-14": (VitArch(224, 14, 1024, 24, 16, 2730, 768, ln_eps=1e-6, ln_pre=False, eva=True),
                   ClipTextArch(49408, 77, 768, 12, 12, 3072, 768, prefix="text.")),
    "EVA02-L-14-336": (VitArch(336, 14, 1024, 24, 16, 2730, 768, ln_eps=1e-6, ln_pre=False, eva=True),
                       ClipTextArch(49408, 77, 768, 12, 12, 3072, 768, prefix="text.")),
    # ConvNeXt CLIPs (model_registry.py:274-339; open_clip model configs convnext_*: timm convnext_{base,large,xxlarge} trunks, timm_pool "",
    # timm_proj linear / mlp).  The 1e-5 LayerNorm eps of xxlarge and the 16-layer text tower of large_d are from the timm / open_clip configs as
    # published (neither library is vendored here): DESIGN.md §5
    "convnext_base": (ConvNextArch(224, (3, 3, 27, 3), (128, 256, 512, 1024), 1e-6, "linear", 512), _TEXT_B),
    "convnext_base_w": (ConvNextArch(256, (3, 3, 27, 3), (128, 256, 512, 1024), 1e-6, "linear", 640), _TEXT_B_PLUS),
    "convnext_base_w_320": (ConvNextArch(320, (3, 3, 27, 3), (128, 256, 512, 1024), 1e-6, "linear", 640), _TEXT_B_PLUS),
    "convnext_large_d": (ConvNextArch(256, (3, 3, 27, 3), (192, 384, 768, 1536), 1e-6, "mlp", 768), replace(_TEXT_L, layers=16)),
    "convnext_large_d_320": (ConvNextArch(320, (3, 3, 27, 3), (192, 384, 768, 1536), 1e-6, "mlp", 768), replace(_TEXT_L, layers=16)),
    "convnext_xxlarge": (ConvNextArch(256, (3, 4, 30, 3), (384, 768, 1536, 3072), 1e-5, "linear", 1024), _TEXT_H),
    "ViT-B-16-SigLIP": _siglip(224), "ViT-B-16-SigLIP-256": _siglip(256), "ViT-B-16-SigLIP-384": _siglip(384),
    "ViT-B-16-SigLIP-512": _siglip(512),
    "ViT-SO400M-14-SigLIP": _siglip(224, so400m=True), "ViT-SO400M-14-SigLIP-384": _siglip(384, so400m=True),
    "ViT-L-16-SigLIP-256": _siglip(256, large=True), "ViT-L-16-SigLIP-384": _siglip(384, large=True),
    # NLLB-CLIP (model_registry.py:510-533; open_clip model configs nllb-clip-base-siglip / nllb-clip-large-siglip: the SigLIP image towers
    # vit_base_patch16_siglip_384 / vit_so400m_patch14_siglip_384 + the NLLB-200 encoder as HF text tower)
    "nllb-clip-base-siglip": (_siglip(384)[0], _NLLB_BASE),
    "nllb-clip-large-siglip": (_siglip(384, so400m=True)[0], _NLLB_LARGE),
}
# architectures the registry names but which the engine does not run (the message of the refusal)
UNSUPPORTED_HINT = ("this open_clip architecture is not runnable by the marqo_amd engine yet "
                    "(supported: " + ", ".join(sorted(OPEN_CLIP_ARCHS)) + " and their -quickgelu variants)")

# hf-hub repos the reference registry names (model_registry.py:483-494) -> the open_clip architecture their open_clip_config.json
# describes (used when that file is not on disk, e.g. with synthetic weights)
KNOWN_HF_HUB_ARCHS = {"hf-hub:Marqo/marqo-fashionCLIP": "ViT-B-16", "hf-hub:Marqo/marqo-fashionSigLIP": "ViT-B-16-SigLIP",
                      # (that the two `mrl` repos carry the model_cfg of the two `clip` ones is taken from the reference registry's dimensions:
                      # an open_clip_config.json on disk always wins — DESIGN.md §3, "NLLB-CLIP")
                      "hf-hub:visheratin/nllb-clip-base-siglip": "nllb-clip-base-siglip", "hf-hub:visheratin/nllb-siglip-mrl-base": "nllb-clip-base-siglip",
                      "hf-hub:visheratin/nllb-clip-large-siglip": "nllb-clip-large-siglip",
                      "hf-hub:visheratin/nllb-siglip-mrl-large": "nllb-clip-large-siglip"}

# ResNet CLIPs (model_registry.py:16-140; open_clip model configs RN50 ... RN50x64): resolved by resolve_resnet_clip only
_TEXT_RN = {512: ClipTextArch(49408, 77, 512, 12, 8, 2048, 1024), 640: ClipTextArch(49408, 77, 640, 12, 10, 2560, 640),
            768: ClipTextArch(49408, 77, 768, 12, 12, 3072, 768), 1024: ClipTextArch(49408, 77, 1024, 12, 16, 4096, 1024)}
RESNET_CLIP_ARCHS = {
    "RN50": (ResNetArch(224, (3, 4, 6, 3), 64, 1024), _TEXT_RN[512]),
    "RN101": (ResNetArch(224, (3, 4, 23, 3), 64, 512), replace(_TEXT_RN[512], out_dim=512)),
    "RN50x4": (ResNetArch(288, (4, 6, 10, 6), 80, 640), _TEXT_RN[640]),
    "RN50x16": (ResNetArch(384, (6, 8, 18, 8), 96, 768), _TEXT_RN[768]),
    "RN50x64": (ResNetArch(448, (3, 15, 36, 10), 128, 1024), _TEXT_RN[1024]),
}
# OpenAI `clip` ResNet names -> open_clip architecture (OpenAI checkpoints: QuickGELU text tower)
OPENAI_RESNET_NAMES = {"RN50": "RN50", "RN101": "RN101", "RN50x4": "RN50x4", "RN50x16": "RN50x16", "RN50x64": "RN50x64"}


def resolve_resnet_clip(arch_name: str, pretrained: Optional[str] = None) -> Tuple[ResNetArch, ClipTextArch]:
    """'RN50' / 'RN50-quickgelu' (+ pretrained tag) -> (vision, text) arch or KeyError.  QuickGELU as resolve_open_clip applies it: on for
    -quickgelu names and for the openai tag."""
    base, quick = arch_name, pretrained == "openai"
    if base.endswith("-quickgelu"):
        base, quick = base[: -len("-quickgelu")], True
    if base not in RESNET_CLIP_ARCHS:
        raise KeyError(f"{arch_name}: not a ResNet CLIP architecture")
    v, t = RESNET_CLIP_ARCHS[base]
    return replace(v, quick_gelu=quick), replace(t, quick_gelu=quick)


# facebookresearch/dino ViTs behind the 'dino-v1' / 'dino-v2' image patch methods (processing/DINO_utils.py:15-63, vision_transformer.py:248-259):
# (width, layers, heads, mlp_dim) at patch 16 or 8 and 224 px; class token, learned positions, conv bias, no ln_pre, erf-GELU, LayerNorm eps 1e-6
DINO_ARCHS = {"vit_small": (384, 12, 6, 1536), "vit_base": (768, 12, 12, 3072)}
DINO_MEAN, DINO_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)   # DINO_utils.py:76-77


def dino_arch(name: str = "vit_small", patch_size: int = 16, image_size: int = 224) -> VitArch:
    """'vit_small' | 'vit_base' at patch 16 | 8 -> the VitArch engine/dino.py runs (out_dim is the width: the tower has no projection)"""
    if name not in DINO_ARCHS:
        raise KeyError(f"{name} not found in {tuple(DINO_ARCHS)}")
    if patch_size not in (8, 16):
        raise KeyError(f"{patch_size} not found in (8, 16)")
    W, layers, heads, mlp = DINO_ARCHS[name]
    return VitArch(image_size=image_size, patch_size=patch_size, width=W, layers=layers, heads=heads, mlp_dim=mlp, out_dim=W, ln_eps=1e-6,
                   ln_pre=False)


# OpenAI `clip` names (clip_utils.py:295-492) -> open_clip architecture (always QuickGELU)
OPENAI_CLIP_NAMES = {"ViT-B/32": "ViT-B-32", "ViT-B/16": "ViT-B-16", "ViT-L/14": "ViT-L-14", "ViT-L/14@336px": "ViT-L-14-336"}


def resolve_open_clip(arch_name: str, pretrained: Optional[str] = None) -> Tuple[Union[VitArch, ConvNextArch], ClipTextArch]:
    """'ViT-B-32' / 'ViT-B-32-quickgelu' / 'convnext_base_w' (+ pretrained tag) -> (vision, text) arch or KeyError."""
    quick = False
    base = arch_name
    if base.endswith("-quickgelu"):
        base, quick = base[: -len("-quickgelu")], True
    if pretrained == "openai":  # OpenAI checkpoints were trained with QuickGELU
        quick = True
    if base not in OPEN_CLIP_ARCHS:
        raise KeyError(f"{arch_name}: {UNSUPPORTED_HINT}")
    v, t = OPEN_CLIP_ARCHS[base]
    quick = quick or v.quick_gelu
    if isinstance(t, str):   # HF text tower: "xlmr-<size>:<out_dim>" (BertArch is defined further down)
        size, out_dim = t.split(":")
        xl = {"roberta-base": BertArch(vocab=50265, max_pos=512, ln_eps=1e-5, pos_offset=2, type_vocab=1),
              "xlmr-base": BertArch(vocab=250002, max_pos=512, ln_eps=1e-5, pos_offset=2, type_vocab=1),
              "xlmr-large": BertArch(vocab=250002, max_pos=512, width=1024, layers=24, heads=16, mlp_dim=4096, ln_eps=1e-5, pos_offset=2,
                                     type_vocab=1)}[size]
        t = HfClipTextArch(bert=xl, out_dim=int(out_dim))
    if isinstance(t, NllbTextArch):   # (its activation is the encoder's own ReLU)
        return replace(v, quick_gelu=quick), t
    return replace(v, quick_gelu=quick), replace(t, quick_gelu=quick)


# HF repo id -> BERT arch for the BERT-family registry entries (model_registry.py:616-880)
_BERT_BASE = BertArch()
_BERT_SMALL = BertArch(width=384, layers=12, heads=12, mlp_dim=1536)  # 12 heads of 32 (zero-padded to 64 at load)
_BERT_LARGE = BertArch(width=1024, layers=24, heads=16, mlp_dim=4096)
_MINILM_L6 = BertArch(width=384, layers=6, heads=12, mlp_dim=1536)   # 12 heads of 32
_MPNET_BASE = BertArch(vocab=30527, max_pos=512, ln_eps=1e-5, pos_offset=2, type_vocab=0, rel_buckets=32)
HF_BERT_ARCHS = {
    "intfloat/e5-base-v2": _BERT_BASE, "intfloat/e5-base": _BERT_BASE,
    "intfloat/e5-small-v2": _BERT_SMALL, "intfloat/e5-small": _BERT_SMALL,
    "intfloat/e5-large-v2": _BERT_LARGE, "intfloat/e5-large": _BERT_LARGE,
    "BAAI/bge-base-en": _BERT_BASE, "BAAI/bge-base-en-v1.5": _BERT_BASE,
    "BAAI/bge-small-en": _BERT_SMALL, "BAAI/bge-small-en-v1.5": _BERT_SMALL,
    "BAAI/bge-large-en": _BERT_LARGE, "BAAI/bge-large-en-v1.5": _BERT_LARGE,
    "sentence-transformers/all-MiniLM-L6-v1": _MINILM_L6, "sentence-transformers/all-MiniLM-L6-v2": _MINILM_L6,
    "sentence-transformers/all-MiniLM-L12-v2": _BERT_SMALL,
    "flax-sentence-embeddings/all_datasets_v3_MiniLM-L12": _BERT_SMALL, "flax-sentence-embeddings/all_datasets_v4_MiniLM-L12": _BERT_SMALL,
    "flax-sentence-embeddings/all_datasets_v3_MiniLM-L6": _MINILM_L6, "flax-sentence-embeddings/all_datasets_v4_MiniLM-L6": _MINILM_L6,
    "intfloat/e5-small-unsupervised": _BERT_SMALL, "intfloat/e5-base-unsupervised": _BERT_BASE, "intfloat/e5-large-unsupervised": _BERT_LARGE,
    "Snowflake/snowflake-arctic-embed-m": _BERT_BASE, "Snowflake/snowflake-arctic-embed-m-v1.5": _BERT_BASE,
    "Snowflake/snowflake-arctic-embed-l": _BERT_LARGE, "llmrails/ember-v1": _BERT_LARGE, "avsolatorio/GIST-large-Embedding-v0": _BERT_LARGE,
    # Chinese BGE: BERT with the 21128-entry Chinese WordPiece vocabulary (small: 4 layers of width 512)
    "BAAI/bge-small-zh-v1.5": BertArch(vocab=21128, width=512, layers=4, heads=8, mlp_dim=2048),
    "BAAI/bge-base-zh-v1.5": BertArch(vocab=21128), "BAAI/bge-large-zh-v1.5": BertArch(vocab=21128, width=1024, layers=24, heads=16, mlp_dim=4096),
    # MPNet encoders (relative-position attention bias, no token types, position ids from 2; vocabulary = BERT's + <s> <pad> </s> <unk> ... <mask>)
    "sentence-transformers/all-mpnet-base-v1": _MPNET_BASE, "sentence-transformers/all-mpnet-base-v2": _MPNET_BASE,
    "flax-sentence-embeddings/all_datasets_v3_mpnet-base": _MPNET_BASE, "flax-sentence-embeddings/all_datasets_v4_mpnet-base": _MPNET_BASE,
    # XLM-RoBERTa encoders
    "sentence-transformers/stsb-xlm-r-multilingual": BertArch(vocab=250002, max_pos=512, ln_eps=1e-5, pos_offset=2),
    "intfloat/multilingual-e5-small": BertArch(vocab=250037, max_pos=512, width=384, layers=12, heads=12, mlp_dim=1536, ln_eps=1e-5, pos_offset=2),
    "intfloat/multilingual-e5-base": BertArch(vocab=250002, max_pos=512, ln_eps=1e-5, pos_offset=2),
    "intfloat/multilingual-e5-large": BertArch(vocab=250002, max_pos=512, width=1024, layers=24, heads=16, mlp_dim=4096, ln_eps=1e-5, pos_offset=2),
    "intfloat/multilingual-e5-large-instruct": BertArch(vocab=250002, max_pos=512, width=1024, layers=24, heads=16, mlp_dim=4096, ln_eps=1e-5, pos_offset=2),
}


# the reference's hf_stella registry entry (model_registry.py:898-904): NewModel-large, rope theta 160000 with NTK factor 2, 8192 positions
STELLA_EN_400M = BertArch(vocab=30528, max_pos=8192, width=1024, layers=24, heads=16, mlp_dim=4096, rope_theta=160000.0, rope_ntk_factor=2.0,
                          glu=True)
HF_BERT_ARCHS["Marqo/dunzhang-stella_en_400M_v5"] = STELLA_EN_400M


def bert_arch_from_hf_config(cfg: dict) -> Union[BertArch, ModernBertArch, QwenArch, GemmaArch, T5Arch, JinaBertArch, NomicBertArch]:
    """A local HF `config.json` -> the arch of the text encoder the `hf` loader builds.  model_type bert, or xlm-roberta / roberta (the same encoder
    with the position ids shifted by padding_idx + 1: the multilingual-e5 family), mpnet and `new` give a BertArch (engine/towers.py::BertTower);
    model_type modernbert gives a ModernBertArch (engine/modernbert.py::ModernBertTower) — callers that can only run a BertArch (the cross-encoders of
    engine/rerank.py, which select their model types before they call) must not pass one through; model_type qwen3 / qwen2 gives a QwenArch
    (engine/qwen.py::QwenTower), model_type gemma3_text a GemmaArch (engine/gemma.py::GemmaTower) and model_type t5 a T5Arch (engine/t5.py::T5Tower) under
    the same rule; so do model_type bert with position_embedding_type alibi, a JinaBertArch (engine/jina_bert.py::JinaBertTower), and model_type
    nomic_bert, a NomicBertArch (engine/nomic_bert.py::NomicBertTower).  Anything else: KeyError."""
    mtype = cfg.get("model_type", "bert")
    if mtype == "jina_embeddings_v3":   # transformers JinaEmbeddingsV3Model: jina-embeddings-v3 with its task adapters (engine/jina_v3.py::JinaV3Tower)
        return resolve_jina_v3(cfg)
    if mtype == "xlm-roberta" and cfg.get("lora_adaptations") is not None:
        raise KeyError("model_type=xlm-roberta with lora_adaptations is the original jina-embeddings-v3 repository's custom-code naming, which is not "
                       "served: bring the checkpoint in transformers' own form (model_type jina_embeddings_v3, jinaai/jina-embeddings-v3-hf)")
    if mtype == "nomic_bert":   # transformers NomicBertModel: nomic-embed-text-v1 / -v1.5, arctic-embed-m-long (engine/nomic_bert.py::NomicBertTower)
        return nomic_bert_arch_from_hf_config(cfg)
    if mtype == "t5":   # transformers T5EncoderModel: sentence-t5, gtr-t5, flan-t5 encoders (engine/t5.py::T5Tower)
        return t5_arch_from_hf_config(cfg)
    if mtype == "gemma3_text":   # transformers Gemma3TextModel with bidirectional attention: EmbeddingGemma (engine/gemma.py::GemmaTower)
        return gemma_arch_from_hf_config(cfg)
    if mtype in ("qwen3", "qwen2"):   # transformers Qwen3Model / Qwen2Model: decoder-style embedders (engine/qwen.py)
        return qwen_arch_from_hf_config(cfg)
    if mtype == "modernbert":   # transformers ModernBertModel: its own arch and tower (engine/modernbert.py)
        return modernbert_arch_from_hf_config(cfg)
    if mtype == "new":  # Alibaba-NLP/new-impl NewModel (custom remote code in the reference: hf_stella)
        if cfg.get("position_embedding_type", "rope") != "rope" or cfg.get("hidden_act", "gelu") != "gelu":
            raise KeyError("NewModel checkpoints are supported with rotary positions and the gated-GELU MLP")
        if cfg.get("layer_norm_type", "layer_norm") != "layer_norm" or not cfg.get("pack_qkv", True):
            raise KeyError("NewModel variants with rms_norm / unpacked qkv are not supported")
        rs = cfg.get("rope_scaling") or {}
        if rs and rs.get("type") != "ntk" or rs.get("mixed_b") is not None:
            raise KeyError(f"rope_scaling={rs} unsupported (ntk without mixed_b only)")
        return BertArch(vocab=cfg["vocab_size"], max_pos=cfg["max_position_embeddings"], width=cfg["hidden_size"],
                        layers=cfg["num_hidden_layers"], heads=cfg["num_attention_heads"], mlp_dim=cfg["intermediate_size"],
                        ln_eps=cfg.get("layer_norm_eps", 1e-12), rope_theta=float(cfg.get("rope_theta", 10000.0)),
                        rope_ntk_factor=float(rs["factor"]) if rs else None, glu=True, type_vocab=int(cfg.get("type_vocab_size", 2)))
    if mtype == "mpnet":   # sentence-transformers all-mpnet-base-v1 / -v2, flax all_datasets_v{3,4}_mpnet-base
        if cfg.get("hidden_act", "gelu") != "gelu":
            raise KeyError(f"hidden_act={cfg.get('hidden_act')} unsupported")
        off = int(cfg.get("pad_token_id", 1)) + 1
        return BertArch(vocab=cfg["vocab_size"], max_pos=cfg["max_position_embeddings"] - off, width=cfg["hidden_size"],
                        layers=cfg["num_hidden_layers"], heads=cfg["num_attention_heads"], mlp_dim=cfg["intermediate_size"],
                        ln_eps=cfg.get("layer_norm_eps", 1e-5), pos_offset=off, type_vocab=0,
                        rel_buckets=int(cfg.get("relative_attention_num_buckets", 32)))
    if mtype not in ("bert", "xlm-roberta", "roberta"):
        raise KeyError(f"model_type={mtype} is not a BERT-family encoder")
    if mtype == "bert" and cfg.get("position_embedding_type", "absolute") == "alibi":   # JinaBERT: jina-embeddings-v2 (engine/jina_bert.py::JinaBertTower)
        return jina_bert_arch_from_hf_config(cfg)
    if cfg.get("position_embedding_type", "absolute") != "absolute":
        raise KeyError("only absolute position embeddings are supported")
    if cfg.get("hidden_act", "gelu") != "gelu":
        raise KeyError(f"hidden_act={cfg.get('hidden_act')} unsupported")
    off = 0 if mtype == "bert" else int(cfg.get("pad_token_id", 1)) + 1
    return BertArch(vocab=cfg["vocab_size"], max_pos=cfg["max_position_embeddings"] - off, width=cfg["hidden_size"],
                    layers=cfg["num_hidden_layers"], heads=cfg["num_attention_heads"],
                    mlp_dim=cfg["intermediate_size"], ln_eps=cfg.get("layer_norm_eps", 1e-12 if mtype == "bert" else 1e-5),
                    pos_offset=off)


# ---- OWL-ViT (the image reranker: s2_inference/reranking/cross_encoders.py ReRankerOwl -> engine/owl.py) ---------------------------------------
@dataclass(frozen=True)
class OwlArch:
    """transformers' OwlViTConfig as the engine runs it: a CLIP ViT with pre_layernorm whose every token is kept, a 16-position CLIP text tower,
    and the detection heads.  The class head's dense0 maps the vision width to the TEXT width, and its rows are multiplied with projected text
    embeddings, so the query dimension is both the text width and the projection dimension."""
    image_size: int
    patch_size: int
    width: int
    layers: int
    heads: int
    mlp_dim: int
    text_width: int
    text_layers: int
    text_heads: int
    text_mlp_dim: int
    query_dim: int
    vocab: int = 49408
    ctx: int = 16
    quick_gelu: bool = True
    text_quick_gelu: bool = True
    ln_eps: float = 1e-5
    text_ln_eps: float = 1e-5

    @property
    def grid(self) -> int:
        return self.image_size // self.patch_size

    @property
    def tokens(self) -> int:
        return self.grid ** 2 + 1

    def vision(self) -> VitArch:
        return VitArch(image_size=self.image_size, patch_size=self.patch_size, width=self.width, layers=self.layers, heads=self.heads,
                       mlp_dim=self.mlp_dim, out_dim=self.width, quick_gelu=self.quick_gelu, ln_eps=self.ln_eps)

    def text(self) -> ClipTextArch:
        return ClipTextArch(vocab=self.vocab, ctx=self.ctx, width=self.text_width, layers=self.text_layers, heads=self.text_heads,
                            mlp_dim=self.text_mlp_dim, out_dim=self.query_dim, quick_gelu=self.text_quick_gelu, ln_eps=self.text_ln_eps)


def _owl(patch: int, image: int, large: bool = False) -> OwlArch:
    if large:
        return OwlArch(image, patch, 1024, 24, 16, 4096, 768, 12, 12, 3072, 768)
    return OwlArch(image, patch, 768, 12, 12, 3072, 512, 12, 8, 2048, 512)


# the three published checkpoints (the names ReRankerOwl maps its model names to)
OWL_ARCHS = {"google/owlvit-base-patch32": _owl(32, 768), "google/owlvit-base-patch16": _owl(16, 768),
             "google/owlvit-large-patch14": _owl(14, 840, large=True)}


def owl_arch_from_hf_config(cfg: dict, base: Optional[OwlArch] = None) -> OwlArch:
    """A local OWL-ViT `config.json` -> OwlArch.  Keys that the file leaves out take `base`'s values (the table entry of the checkpoint's
    name) or OwlViTConfig's defaults (= google/owlvit-base-patch32)."""
    if cfg.get("model_type") != "owlvit":
        raise KeyError(f"model_type={cfg.get('model_type')!r} is not 'owlvit'")
    b = base or OWL_ARCHS["google/owlvit-base-patch32"]
    v, t = cfg.get("vision_config") or {}, cfg.get("text_config") or {}
    acts = {"quick_gelu": True, "gelu": False}
    for side, c in (("vision", v), ("text", t)):
        if c.get("hidden_act", "quick_gelu") not in acts:
            raise KeyError(f"{side}_config.hidden_act={c.get('hidden_act')!r} unsupported (quick_gelu | gelu)")
    text_width = int(t.get("hidden_size", b.text_width))
    query_dim = int(cfg.get("projection_dim", b.query_dim))
    if query_dim != text_width:
        raise KeyError(f"projection_dim={query_dim} must equal text_config.hidden_size={text_width}: the class head multiplies rows of that width "
                       f"with the projected text embeddings")
    return OwlArch(image_size=int(v.get("image_size", b.image_size)), patch_size=int(v.get("patch_size", b.patch_size)),
                   width=int(v.get("hidden_size", b.width)), layers=int(v.get("num_hidden_layers", b.layers)),
                   heads=int(v.get("num_attention_heads", b.heads)), mlp_dim=int(v.get("intermediate_size", b.mlp_dim)),
                   text_width=text_width, text_layers=int(t.get("num_hidden_layers", b.text_layers)),
                   text_heads=int(t.get("num_attention_heads", b.text_heads)), text_mlp_dim=int(t.get("intermediate_size", b.text_mlp_dim)),
                   query_dim=query_dim, vocab=int(t.get("vocab_size", b.vocab)), ctx=int(t.get("max_position_embeddings", b.ctx)),
                   quick_gelu=acts[v.get("hidden_act", "quick_gelu")], text_quick_gelu=acts[t.get("hidden_act", "quick_gelu")],
                   ln_eps=float(v.get("layer_norm_eps", b.ln_eps)), text_ln_eps=float(t.get("layer_norm_eps", b.text_ln_eps)))


# ---- LanguageBind (the multimodal loader: s2_inference/multimodal_model_load.py -> engine/languagebind.py) --------------------------------------
@dataclass(frozen=True)
class LanguageBindArch:
    """One LanguageBind part (the reference's languagebind/{video,image}/configuration_*.py) as the engine runs it: a CLIP ViT with
    `pre_layrnorm` whose class rows are pooled, with `add_time_attn` a temporal sub-block in front of every layer and the mean over the
    `num_frames` class rows of a clip, and a 77-position CLIP text tower.  Both project to `projection_dim`.  An AUDIO part
    (languagebind/audio/configuration_audio.py) has `num_mel_bins` and `target_length` set: its picture is num_mel_bins x target_length
    (modeling_audio.py:769-771), `image_size` is then not what the tower runs on."""
    image_size: int
    patch_size: int
    width: int
    layers: int
    heads: int
    mlp_dim: int
    num_frames: int
    add_time_attn: bool
    text_width: int
    text_layers: int
    text_heads: int
    text_mlp_dim: int
    out_dim: int
    vocab: int = 49408
    ctx: int = 77
    quick_gelu: bool = False
    text_quick_gelu: bool = False
    ln_eps: float = 1e-5
    text_ln_eps: float = 1e-5
    num_mel_bins: int = 0
    target_length: int = 0
    audio_sample_rate: int = 16000
    audio_mean: float = 0.5
    audio_std: float = 0.5

    @property
    def is_audio(self) -> bool:
        return self.num_mel_bins != 0 and self.target_length != 0

    @property
    def image_hw(self) -> tuple:
        """(height, width) of the picture the vision side runs on"""
        return (self.num_mel_bins, self.target_length) if self.is_audio else (self.image_size, self.image_size)

    @property
    def grid(self) -> int:
        return self.image_size // self.patch_size

    @property
    def grid_h(self) -> int:
        return self.image_hw[0] // self.patch_size

    @property
    def grid_w(self) -> int:
        return self.image_hw[1] // self.patch_size

    @property
    def tokens(self) -> int:
        return self.grid_h * self.grid_w + 1

    def vision(self) -> VitArch:
        return VitArch(image_size=self.image_size, patch_size=self.patch_size, width=self.width, layers=self.layers, heads=self.heads,
                       mlp_dim=self.mlp_dim, out_dim=self.out_dim, quick_gelu=self.quick_gelu, ln_eps=self.ln_eps)

    def text(self) -> ClipTextArch:
        return ClipTextArch(vocab=self.vocab, ctx=self.ctx, width=self.text_width, layers=self.text_layers, heads=self.text_heads,
                            mlp_dim=self.text_mlp_dim, out_dim=self.out_dim, quick_gelu=self.text_quick_gelu, ln_eps=self.text_ln_eps)


def languagebind_arch_from_hf_config(cfg: dict) -> LanguageBindArch:
    """A local LanguageBind `config.json` -> LanguageBindArch.  Keys the file leaves out take the defaults of the reference's configuration
    classes (CLIP ViT-B/32-like sides, 512-wide projection, quick_gelu, one frame, no temporal attention; for the audio keys
    num_mel_bins 0, target_length 0 — both written as 0.0 there —, audio_sample_rate 16000, audio_mean 0.5, audio_std 0.5)."""
    v, t = cfg.get("vision_config") or {}, cfg.get("text_config") or {}
    acts = {"quick_gelu": True, "gelu": False}
    for side, c in (("vision", v), ("text", t)):
        if c.get("hidden_act", "quick_gelu") not in acts:
            raise KeyError(f"{side}_config.hidden_act={c.get('hidden_act')!r} unsupported (quick_gelu | gelu)")
    return LanguageBindArch(image_size=int(v.get("image_size", 224)), patch_size=int(v.get("patch_size", 32)), width=int(v.get("hidden_size", 768)),
                            layers=int(v.get("num_hidden_layers", 12)), heads=int(v.get("num_attention_heads", 12)),
                            mlp_dim=int(v.get("intermediate_size", 3072)), num_frames=int(v.get("num_frames", 1)),
                            add_time_attn=bool(v.get("add_time_attn", False)), text_width=int(t.get("hidden_size", 512)),
                            text_layers=int(t.get("num_hidden_layers", 12)), text_heads=int(t.get("num_attention_heads", 8)),
                            text_mlp_dim=int(t.get("intermediate_size", 2048)), out_dim=int(cfg.get("projection_dim", 512)),
                            vocab=int(t.get("vocab_size", 49408)), ctx=int(t.get("max_position_embeddings", 77)),
                            quick_gelu=acts[v.get("hidden_act", "quick_gelu")], text_quick_gelu=acts[t.get("hidden_act", "quick_gelu")],
                            ln_eps=float(v.get("layer_norm_eps", 1e-5)), text_ln_eps=float(t.get("layer_norm_eps", 1e-5)),
                            num_mel_bins=int(v.get("num_mel_bins", 0)), target_length=int(v.get("target_length", 0)),
                            audio_sample_rate=int(v.get("audio_sample_rate", 16000)), audio_mean=float(v.get("audio_mean", 0.5)),
                            audio_std=float(v.get("audio_std", 0.5)))

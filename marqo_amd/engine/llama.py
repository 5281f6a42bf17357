"""Mistral / Llama text tower: transformers' MistralModel / LlamaModel checkpoints (model_type "mistral" / "llama": e5-mistral-7b-instruct,
SFR-Embedding-Mistral, Linq-Embed-Mistral, Llama-2-shaped fine-tunes) -> HBM layout -> one mq_encode_llama call per batch of packed sequences
(csrc/llama.hip; the causal sliding-window grouped-query attention kernel: csrc/attention_gqa.hip).

bf16 GEMM operands, fp32 residual stream, 64- or 128-wide heads, widths up to 4096.  The block is the Qwen tower's without q / k norm and without biases,
so the checkpoint-to-tensor transform (names, the fused QKV and (up | gate) weights) is engine/tower_weights.py::qwen_state_dict and the weight structs
are the Qwen tower's."""
from __future__ import annotations

from typing import Dict

import torch

from marqo_amd import _lib as L
from marqo_amd.engine.archs import LlamaArch
from marqo_amd.engine.tower_weights import qwen_state_dict
from marqo_amd.engine.towers import _PackedTextTower, _check_precision

Tensor = torch.Tensor


class LlamaTower(_PackedTextTower):
    """Mistral / Llama decoder + last-token / mean pooling (+ L2); the call loop and the input checks are _PackedTextTower's."""
    family = "llama"

    def __init__(self, arch: LlamaArch, sd: Dict[str, Tensor], device: str, pooling: str = "last", precision: str = "bf16"):
        super().__init__(device)
        _check_precision(precision, ("bf16",), f"the Mistral / Llama tower runs on bf16 operands only (its RMSNorm / rotary / gated-SiLU blocks have no e4m3 "
                                               f"kernels), got precision {precision!r}")
        if arch.head_dim not in (64, 128):
            raise ValueError(f"the Mistral / Llama tower runs 64- or 128-wide attention heads only (head_dim {arch.head_dim})")
        if arch.heads < 1 or arch.kv_heads < 1 or arch.heads % arch.kv_heads:
            raise ValueError(f"heads {arch.heads} must be a multiple of kv_heads {arch.kv_heads}")
        if arch.width > 4096 or arch.width % 64:
            raise ValueError(f"the Mistral / Llama tower runs widths that are multiples of 64 up to 4096 (width {arch.width})")
        if arch.window is not None and arch.window < 1:
            raise ValueError(f"window must be at least 1 or None, got {arch.window}")
        if pooling not in ("last", "mean"):
            raise ValueError(f"pooling must be 'last' or 'mean', got {pooling!r}")
        self.precision, self.arch, self.pooling = precision, arch, pooling
        self._fp8 = None
        h = self._h
        t = qwen_state_dict(arch, sd, tower="Mistral / Llama")
        W = arch.width
        self._layers = (L.QwenLayer * arch.layers)()
        for l in range(arch.layers):
            p = f"layers.{l}."
            a = p + "self_attn."
            self._layers[l] = L.QwenLayer(
                input_norm_g=h.f32(t.pop(p + "input_layernorm.weight")), qkv_w=h.bf16(t.pop(a + "qkv.weight")), qkv_b=None, q_norm_g=None, k_norm_g=None,
                out_w=h.bf16(t.pop(a + "o_proj.weight")), post_norm_g=h.f32(t.pop(p + "post_attention_layernorm.weight")),
                ug_w=h.bf16(t.pop(p + "mlp.up_gate.weight")), down_w=h.bf16(t.pop(p + "mlp.down_proj.weight")))
        self.w = L.QwenWeights(tok_emb=h.f32(t["embed_tokens.weight"]), final_norm_g=h.f32(t["norm.weight"]), zeros=h.f32(torch.zeros(W)),
                               d_inv_freq=h.f32(arch.inv_freq()), layers=self._layers)
        self.cfg = L.LlamaCfg(width=W, layers=arch.layers, q_heads=arch.heads, kv_heads=arch.kv_heads, head_dim=arch.head_dim, mlp_dim=arch.mlp_dim,
                              vocab=arch.vocab, max_pos=arch.max_pos, pool=L.MQ_POOL_LAST if pooling == "last" else L.MQ_POOL_MEAN,
                              window=int(arch.window or 0), rms_eps=arch.rms_eps, reserved0=0)

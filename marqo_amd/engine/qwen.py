"""Qwen3 / Qwen2 text tower: transformers' Qwen3Model / Qwen2Model checkpoints (model_type "qwen3" / "qwen2": Qwen3-Embedding-0.6B,
gte-Qwen2-1.5B-instruct, Qwen2-0.5B fine-tunes) -> HBM layout -> one mq_encode_qwen call per batch of packed sequences (csrc/qwen.hip; the grouped-query
causal attention kernel: csrc/attention_gqa.hip).

bf16 GEMM operands, fp32 residual stream, 64- or 128-wide heads.  The checkpoint-to-tensor transform (names, the fused QKV and (up | gate) weights) is
engine/tower_weights.py::qwen_state_dict."""
from __future__ import annotations

from typing import Dict

import torch

from marqo_amd import _lib as L
from marqo_amd.engine.archs import QwenArch
from marqo_amd.engine.tower_weights import qwen_state_dict
from marqo_amd.engine.towers import _PackedTextTower, _check_precision

Tensor = torch.Tensor


class QwenTower(_PackedTextTower):
    """Qwen3 / Qwen2 decoder + last-token / mean pooling (+ L2); the call loop and the input checks are _PackedTextTower's."""
    family = "qwen"

    def __init__(self, arch: QwenArch, sd: Dict[str, Tensor], device: str, pooling: str = "last", precision: str = "bf16"):
        super().__init__(device)
        _check_precision(precision, ("bf16",), f"the Qwen tower runs on bf16 operands only (its RMSNorm / rotary / gated-SiLU blocks have no e4m3 kernels), "
                                               f"got precision {precision!r}")
        if arch.head_dim not in (64, 128):
            raise ValueError(f"the Qwen tower runs 64- or 128-wide attention heads only (head_dim {arch.head_dim})")
        if arch.heads < 1 or arch.kv_heads < 1 or arch.heads % arch.kv_heads:
            raise ValueError(f"heads {arch.heads} must be a multiple of kv_heads {arch.kv_heads}")
        if arch.width > 2048 or arch.width % 64:
            raise ValueError(f"the Qwen tower runs widths that are multiples of 64 up to 2048 (width {arch.width}: the 4B / 8B sizes are not served)")
        if pooling not in ("last", "mean"):
            raise ValueError(f"pooling must be 'last' or 'mean', got {pooling!r}")
        self.precision, self.arch, self.pooling = precision, arch, pooling
        self._fp8 = None
        h = self._h
        t = qwen_state_dict(arch, sd)
        W = arch.width
        self._layers = (L.QwenLayer * arch.layers)()
        for l in range(arch.layers):
            p = f"layers.{l}."
            a = p + "self_attn."
            self._layers[l] = L.QwenLayer(
                input_norm_g=h.f32(t[p + "input_layernorm.weight"]), qkv_w=h.bf16(t[a + "qkv.weight"]),
                qkv_b=h.f32(t[a + "qkv.bias"]) if arch.qkv_bias else None,
                q_norm_g=h.f32(t[a + "q_norm.weight"]) if arch.qk_norm else None, k_norm_g=h.f32(t[a + "k_norm.weight"]) if arch.qk_norm else None,
                out_w=h.bf16(t[a + "o_proj.weight"]), post_norm_g=h.f32(t[p + "post_attention_layernorm.weight"]),
                ug_w=h.bf16(t[p + "mlp.up_gate.weight"]), down_w=h.bf16(t[p + "mlp.down_proj.weight"]))
        self.w = L.QwenWeights(tok_emb=h.f32(t["embed_tokens.weight"]), final_norm_g=h.f32(t["norm.weight"]), zeros=h.f32(torch.zeros(W)),
                               d_inv_freq=h.f32(arch.inv_freq()), layers=self._layers)
        self.cfg = L.QwenCfg(width=W, layers=arch.layers, q_heads=arch.heads, kv_heads=arch.kv_heads, head_dim=arch.head_dim, mlp_dim=arch.mlp_dim,
                             vocab=arch.vocab, max_pos=arch.max_pos, pool=L.MQ_POOL_LAST if pooling == "last" else L.MQ_POOL_MEAN, rms_eps=arch.rms_eps)

"""Gemma2 text tower: transformers' Gemma2Model checkpoints (model_type "gemma2": BAAI/bge-multilingual-gemma2 and the Gemma-2-2B-shaped fine-tunes) ->
HBM layout -> one mq_encode_gemma2 call per batch of packed sequences (csrc/gemma2.hip; the soft-capped windowed causal grouped-query attention kernel:
csrc/attention_gqa256_softcap.hip).

bf16 GEMM operands, fp32 residual stream, 256-wide heads, widths up to 4096.  The checkpoint-to-tensor transform (names, the 1 + w norm weights, the fused
QKV and (up | gate) weights, the token table times sqrt(width)) is engine/tower_weights.py::gemma2_state_dict; the weight structs are the EmbeddingGemma
tower's, without q / k norm gains and with one inverse-frequency table."""
from __future__ import annotations

from typing import Dict

import torch

from marqo_amd import _lib as L
from marqo_amd.engine.archs import Gemma2Arch
from marqo_amd.engine.tower_weights import gemma2_state_dict
from marqo_amd.engine.towers import _PackedTextTower, _check_precision

Tensor = torch.Tensor


class Gemma2Tower(_PackedTextTower):
    """Gemma2 decoder + last-token / mean pooling (+ L2); the call loop and the input checks are _PackedTextTower's."""
    family = "gemma2"

    def __init__(self, arch: Gemma2Arch, sd: Dict[str, Tensor], device: str, pooling: str = "last", precision: str = "bf16"):
        super().__init__(device)
        _check_precision(precision, ("bf16",), f"the Gemma2 tower runs on bf16 operands only (its RMSNorm / rotary / gated tanh-GELU blocks have no e4m3 "
                                               f"kernels), got precision {precision!r}")
        # (the shape bounds — head_dim, heads, width, softcap — are gemma2_arch_from_hf_config's and mq_encode_gemma2's: not restated here)
        if len(arch.sliding) != arch.layers:
            raise ValueError(f"arch.sliding names {len(arch.sliding)} layers, the model has {arch.layers}")
        if pooling not in ("last", "mean"):
            raise ValueError(f"pooling must be 'last' or 'mean', got {pooling!r}")
        self.precision, self.arch, self.pooling = precision, arch, pooling
        self._fp8 = None
        h = self._h
        t = gemma2_state_dict(arch, sd)
        self._layers = (L.GemmaLayer * arch.layers)()
        for l in range(arch.layers):
            p = f"layers.{l}."
            a = p + "self_attn."
            self._layers[l] = L.GemmaLayer(
                input_norm_g=h.f32(t.pop(p + "input_layernorm.weight")), qkv_w=h.bf16(t.pop(a + "qkv.weight")), q_norm_g=None, k_norm_g=None,
                out_w=h.bf16(t.pop(a + "o_proj.weight")), post_attn_norm_g=h.f32(t.pop(p + "post_attention_layernorm.weight")),
                pre_ffn_norm_g=h.f32(t.pop(p + "pre_feedforward_layernorm.weight")), ug_w=h.bf16(t.pop(p + "mlp.up_gate.weight")),
                down_w=h.bf16(t.pop(p + "mlp.down_proj.weight")), post_ffn_norm_g=h.f32(t.pop(p + "post_feedforward_layernorm.weight")),
                sliding=1 if arch.sliding[l] else 0, reserved=0)
        self.w = L.GemmaWeights(tok_emb=h.f32(t["embed_tokens.weight"]), final_norm_g=h.f32(t["norm.weight"]), d_inv_freq_global=h.f32(arch.inv_freq()),
                                d_inv_freq_local=None, layers=self._layers)
        self.cfg = L.Gemma2Cfg(width=arch.width, layers=arch.layers, q_heads=arch.heads, kv_heads=arch.kv_heads, head_dim=arch.head_dim,
                               mlp_dim=arch.mlp_dim, vocab=arch.vocab, max_pos=arch.max_pos, window=int(arch.window) if any(arch.sliding) else 0,
                               pool=L.MQ_POOL_LAST if pooling == "last" else L.MQ_POOL_MEAN, rms_eps=arch.rms_eps, attn_scale=arch.attn_scale,
                               softcap=arch.softcap, reserved0=0)

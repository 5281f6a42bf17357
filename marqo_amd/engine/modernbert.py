"""ModernBERT text tower: transformers' ModernBertModel checkpoints (model_type "modernbert") -> HBM layout -> one mq_encode_modernbert call per
batch of packed sequences (csrc/modernbert.hip; the sliding layers' band kernel: csrc/attention_window.hip).

bf16 GEMM operands, fp32 residual stream, 64-wide heads.  The checkpoint-to-tensor transform (names, the swap of mlp.Wi's halves) is
engine/tower_weights.py::modernbert_state_dict."""
from __future__ import annotations

from typing import Dict

import torch

from marqo_amd import _lib as L
from marqo_amd.engine.archs import ModernBertArch
from marqo_amd.engine.tower_weights import modernbert_state_dict
from marqo_amd.engine.towers import _PackedTextTower, _check_precision

Tensor = torch.Tensor


class ModernBertTower(_PackedTextTower):
    """ModernBERT encoder + mean / CLS pooling (+ L2); the call loop and the input checks are _PackedTextTower's."""
    family = "modernbert"

    def __init__(self, arch: ModernBertArch, sd: Dict[str, Tensor], device: str, pooling: str = "mean", precision: str = "bf16"):
        super().__init__(device)
        _check_precision(precision, ("bf16",), f"the ModernBERT tower runs on bf16 operands only (its rotary / gated-GELU blocks have no e4m3 kernels), "
                                               f"got precision {precision!r}")
        if arch.heads < 1 or arch.width != arch.heads * 64:
            raise ValueError(f"the ModernBERT tower runs 64-wide attention heads only (width {arch.width}, heads {arch.heads})")
        if pooling not in ("mean", "cls"):
            raise ValueError(f"pooling must be 'mean' or 'cls', got {pooling!r}")
        if len(arch.sliding) != arch.layers:
            raise ValueError(f"arch.sliding names {len(arch.sliding)} layers, the model has {arch.layers}")
        self.precision, self.arch, self.pooling = precision, arch, pooling
        self._fp8 = None
        h = self._h
        t = modernbert_state_dict(arch, sd)
        W = arch.width
        self._layers = (L.ModernBertLayer * arch.layers)()
        for l in range(arch.layers):
            p = f"layers.{l}."
            self._layers[l] = L.ModernBertLayer(
                attn_norm_g=h.f32(t[p + "attn_norm.weight"]) if l > 0 else None, qkv_w=h.bf16(t[p + "attn.Wqkv.weight"]),
                out_w=h.bf16(t[p + "attn.Wo.weight"]), mlp_norm_g=h.f32(t[p + "mlp_norm.weight"]), wi_w=h.bf16(t[p + "mlp.Wi.weight"]),
                wo_w=h.bf16(t[p + "mlp.Wo.weight"]), sliding=1 if arch.sliding[l] else 0, reserved=0)
        self.w = L.ModernBertWeights(
            tok_emb=h.f32(t["embeddings.tok_embeddings.weight"]), emb_ln_g=h.f32(t["embeddings.norm.weight"]), final_ln_g=h.f32(t["final_norm.weight"]),
            zeros=h.f32(torch.zeros(W)), d_inv_freq_global=h.f32(arch.inv_freq(local=False)), d_inv_freq_local=h.f32(arch.inv_freq(local=True)),
            layers=self._layers)
        self.cfg = L.ModernBertCfg(width=W, layers=arch.layers, heads=arch.heads, mlp_dim=arch.mlp_dim, vocab=arch.vocab, max_pos=arch.max_pos,
                                   half_window=arch.half_window, pool=L.MQ_POOL_MEAN if pooling == "mean" else L.MQ_POOL_CLS, ln_eps=arch.ln_eps, reserved=0)

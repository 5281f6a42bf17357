"""NomicBERT text tower: nomic-embed-text-v1 / -v1.5 / -v1-unsupervised, their fine-tunes and snowflake-arctic-embed-m-long (config.json: model_type
"nomic_bert"; transformers' NomicBertModel tensor names or the hub's original ones) -> HBM layout -> one mq_encode_nomic_bert call per batch of packed
sequences (csrc/nomic_bert.hip; the sliced full attention kernel: csrc/attention_full.hip).

bf16 GEMM operands, fp32 residual stream, 64-wide heads, sequences up to 8192 tokens.  The checkpoint-to-tensor transform (the two namings, the fused
QKV and the (up | gate) stack) is engine/tower_weights.py::nomic_bert_state_dict; the rotary frequencies are NomicBertArch.inv_freq().  The block
semantics are pinned to transformers' NomicBertModel in float64 (tests/test_nomic_bert_host.py)."""
from __future__ import annotations

from typing import Dict

import torch

from marqo_amd import _lib as L
from marqo_amd.engine.archs import NomicBertArch
from marqo_amd.engine.tower_weights import nomic_bert_state_dict
from marqo_amd.engine.towers import _PackedTextTower, _check_precision

Tensor = torch.Tensor


class NomicBertTower(_PackedTextTower):
    """NomicBERT encoder + mean / CLS pooling (+ L2); the call loop and the input checks are _PackedTextTower's."""
    family = "nomic_bert"

    def __init__(self, arch: NomicBertArch, sd: Dict[str, Tensor], device: str, pooling: str = "mean", precision: str = "bf16"):
        super().__init__(device)
        _check_precision(precision, ("bf16",), f"the NomicBERT tower runs on bf16 operands only (its rotary / gated-SiLU blocks have no e4m3 kernels), "
                                               f"got precision {precision!r}")
        if arch.head_dim != 64 or arch.width != arch.heads * 64:
            raise ValueError(f"the NomicBERT tower runs 64-wide attention heads only (hidden_size {arch.width}, num_attention_heads {arch.heads})")
        if arch.width > 2048:
            raise ValueError(f"the NomicBERT tower runs widths up to 2048 (hidden_size {arch.width})")
        if pooling not in ("mean", "cls"):
            raise ValueError(f"pooling must be 'mean' or 'cls', got {pooling!r}")
        self.precision, self.arch, self.pooling = precision, arch, pooling
        self._fp8 = None
        h = self._h
        t = nomic_bert_state_dict(arch, sd)
        self._layers = (L.NomicBertLayer * arch.layers)()
        for l in range(arch.layers):
            p = f"layer.{l}."
            self._layers[l] = L.NomicBertLayer(qkv_w=h.bf16(t[p + "attn.qkv.weight"]), out_w=h.bf16(t[p + "attn.o.weight"]),
                                               attn_ln_g=h.f32(t[p + "attn_ln.weight"]), attn_ln_b=h.f32(t[p + "attn_ln.bias"]),
                                               ug_w=h.bf16(t[p + "mlp.up_gate.weight"]), down_w=h.bf16(t[p + "mlp.down.weight"]),
                                               mlp_ln_g=h.f32(t[p + "mlp_ln.weight"]), mlp_ln_b=h.f32(t[p + "mlp_ln.bias"]))
        self.w = L.NomicBertWeights(tok_emb=h.f32(t["word_embeddings.weight"]), type0=h.f32(t["type0"]), emb_ln_g=h.f32(t["emb_ln.weight"]),
                                    emb_ln_b=h.f32(t["emb_ln.bias"]), zeros=h.f32(torch.zeros(arch.width)), d_inv_freq=h.f32(arch.inv_freq()),
                                    layers=self._layers)
        self.cfg = L.NomicBertCfg(width=arch.width, layers=arch.layers, heads=arch.heads, head_dim=arch.head_dim, mlp_dim=arch.mlp_dim, vocab=arch.vocab,
                                  max_pos=arch.max_pos, pool=L.MQ_POOL_CLS if pooling == "cls" else L.MQ_POOL_MEAN, ln_eps=arch.ln_eps, reserved=0)

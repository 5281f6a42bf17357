"""DeBERTa-v2 / -v3 text tower: transformers' DebertaV2Model as the one-label rerankers configure it (config.json: model_type "deberta-v2") -> HBM layout ->
one mq_encode_deberta call per batch of packed sequences (csrc/deberta.hip; the disentangled attention kernel: csrc/attention_disentangled.hip).

bf16 GEMM operands, fp32 residual stream, 64-wide heads.  The checkpoint-to-tensor transform (names, the fused QKV, the projected position tables Kr / Qr
of every block) is engine/tower_weights.py::deberta_state_dict; the bucket index table is DebertaArch.idx_table(reach), built on the host from the
modelling code's own arithmetic and handed over on the device and on the host.  The tower is what the cross-encoder of engine/rerank.py stands on; DeBERTa
as an embedding model through `hf` / `sbert` is not served."""
from __future__ import annotations

import dataclasses
from typing import Dict

import torch

from marqo_amd import _lib as L
from marqo_amd.engine.archs import DebertaArch
from marqo_amd.engine.tower_weights import deberta_state_dict
from marqo_amd.engine.towers import _PackedTextTower, _check_precision

Tensor = torch.Tensor


class DebertaTower(_PackedTextTower):
    """DeBERTa encoder + CLS / mean pooling (+ L2); the call loop and the input checks are _PackedTextTower's.  `max_len` is the longest sequence the tower
    will be asked for: the index table reaches max_len - 1 tokens either way."""
    family = "deberta"

    def __init__(self, arch: DebertaArch, sd: Dict[str, Tensor], device: str, pooling: str = "cls", precision: str = "bf16", max_len: int = 512):
        super().__init__(device)
        _check_precision(precision, ("bf16",), f"the DeBERTa tower runs on bf16 operands only (its disentangled attention has no e4m3 kernel), got "
                                               f"precision {precision!r}")
        if arch.head_dim != 64 or arch.width != arch.heads * 64:
            raise ValueError(f"the DeBERTa tower runs 64-wide attention heads only (hidden_size {arch.width}, num_attention_heads {arch.heads})")
        if arch.width > 2048:
            raise ValueError(f"the DeBERTa tower runs widths up to 2048 (hidden_size {arch.width})")
        if not 1 <= arch.span <= 1024:
            raise ValueError(f"the DeBERTa tower runs position_buckets in 1 .. 1024 (got {arch.span})")
        if pooling not in ("mean", "cls"):
            raise ValueError(f"pooling must be 'mean' or 'cls', got {pooling!r}")
        max_len = int(min(max(int(max_len), 1), arch.max_pos, 8192))
        self.precision, self.pooling = precision, pooling
        self.arch = dataclasses.replace(arch, max_pos=max_len)
        self._fp8 = None
        h = self._h
        t = self.tensors = deberta_state_dict(arch, sd)
        self.reach = max_len - 1
        self._h_idx = arch.idx_table(self.reach).contiguous()          # (kept alive: the library reads it on the host in every call)
        self._d_idx = self._h_idx.to(self.device)
        self._layers = (L.DebertaLayer * arch.layers)()
        for l in range(arch.layers):
            p = f"layer.{l}."
            self._layers[l] = L.DebertaLayer(qkv_w=h.bf16(t[p + "attn.qkv.weight"]), qkv_b=h.f32(t[p + "attn.qkv.bias"]), out_w=h.bf16(t[p + "attn.o.weight"]),
                                             out_b=h.f32(t[p + "attn.o.bias"]), attn_ln_g=h.f32(t[p + "attn_ln.weight"]), attn_ln_b=h.f32(t[p + "attn_ln.bias"]),
                                             fc1_w=h.bf16(t[p + "mlp.fc1.weight"]), fc1_b=h.f32(t[p + "mlp.fc1.bias"]), fc2_w=h.bf16(t[p + "mlp.fc2.weight"]),
                                             fc2_b=h.f32(t[p + "mlp.fc2.bias"]), mlp_ln_g=h.f32(t[p + "mlp_ln.weight"]), mlp_ln_b=h.f32(t[p + "mlp_ln.bias"]),
                                             pos_key=h.bf16(t[p + "pos_key"]), pos_query=h.bf16(t[p + "pos_query"]))
        self.w = L.DebertaWeights(tok_emb=h.f32(t["word_embeddings.weight"]), emb_ln_g=h.f32(t["emb_ln.weight"]), emb_ln_b=h.f32(t["emb_ln.bias"]),
                                  d_idx=self._d_idx.data_ptr(), h_idx=self._h_idx.data_ptr(), layers=self._layers)
        self.cfg = L.DebertaCfg(width=arch.width, layers=arch.layers, heads=arch.heads, head_dim=arch.head_dim, mlp_dim=arch.mlp_dim, vocab=arch.vocab,
                                max_pos=max_len, pool=L.MQ_POOL_CLS if pooling == "cls" else L.MQ_POOL_MEAN, span=arch.span, reach=self.reach,
                                ln_eps=arch.ln_eps, reserved=0)

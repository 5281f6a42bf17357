"""ModernBERT text tower: transformers' ModernBertModel checkpoints (model_type "modernbert") -> HBM layout -> one mq_encode_modernbert call per
batch of packed sequences (csrc/modernbert.hip; the sliding layers' band kernel: csrc/attention_window.hip).

bf16 GEMM operands, fp32 residual stream, 64-wide heads.  The checkpoint-to-tensor transform (names, the swap of mlp.Wi's halves) is
engine/tower_weights.py::modernbert_state_dict."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import numpy as np
import torch

from marqo_amd import _lib as L
from marqo_amd.engine.archs import ModernBertArch
from marqo_amd.engine.tower_weights import modernbert_state_dict
from marqo_amd.engine.towers import _TextTowerBase, _check_precision, _host_i64, _large_call

Tensor = torch.Tensor


class ModernBertTower(_TextTowerBase):
    """ModernBERT encoder + mean / CLS pooling (+ L2), the interface of BertTower: encode_ids(ids, attention_mask, normalize)."""

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

    @property
    def out_width(self) -> int:
        return self.arch.width

    def release_unused_folded(self) -> int:
        return 0     # (no folded LayerNorm copies are made for this tower)

    def queue_rows_ids(self, ids_h: np.ndarray, mask_h: np.ndarray, normalize: bool = True) -> Optional[np.ndarray]:
        return None  # (the native request queue serves mq_encode_bert / mq_encode_clip_text: this tower keeps the direct path)

    def encode_ids(self, ids: Tensor, attention_mask: Tensor, normalize: bool = True) -> Tensor:
        """ids / attention_mask: int [n, S], right-padded.  Only mask == 1 tokens are run (padded keys are masked out of every real row in the
        reference, and padded rows are not pooled) -> fp32 [n, width] on the device."""
        if ids.shape != attention_mask.shape or ids.ndim != 2:
            raise ValueError("ids and attention_mask must both be [n, S]")
        ids_h, mask_h = _host_i64(ids), _host_i64(attention_mask)
        n, S = ids_h.shape
        lengths = mask_h.sum(axis=1)
        if bool((lengths < 1).any()):
            raise ValueError("every sequence needs at least one unmasked token")
        if not bool(((mask_h != 0) == (np.arange(S)[None, :] < lengths[:, None])).all()):
            raise ValueError("attention_mask must be right-padded (a prefix of ones per row)")
        if n and int(lengths.max()) > self.arch.max_pos:
            raise ValueError(f"sequence longer than max_position_embeddings={self.arch.max_pos}")
        out = torch.empty(n, self.arch.width, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device), _large_call(self.device, int(lengths.sum())):
            for a, b in self._chunks(lengths):
                d_packed, d_cu, cu = self._stage_host(ids_h, lengths, a, b)
                ws = self._workspace(self.lib.mq_modernbert_workspace_bytes(C.byref(self.cfg), d_packed.numel(), b - a))
                L.check(self.lib.mq_encode_modernbert(C.byref(self.cfg), C.byref(self.w), d_packed.data_ptr(), d_cu.data_ptr(), cu.data_ptr(), b - a,
                                                      out[a:b].data_ptr(), 1 if normalize else 0, ws.data_ptr(), ws.numel(), self._stream()),
                        "mq_encode_modernbert")
        return out

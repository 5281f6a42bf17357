"""Qwen3 / Qwen2 text tower: transformers' Qwen3Model / Qwen2Model checkpoints (model_type "qwen3" / "qwen2": Qwen3-Embedding-0.6B,
gte-Qwen2-1.5B-instruct, Qwen2-0.5B fine-tunes) -> HBM layout -> one mq_encode_qwen call per batch of packed sequences (csrc/qwen.hip; the grouped-query
causal attention kernel: csrc/attention_gqa.hip).

bf16 GEMM operands, fp32 residual stream, 64- or 128-wide heads.  The checkpoint-to-tensor transform (names, the fused QKV and (up | gate) weights) is
engine/tower_weights.py::qwen_state_dict."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import numpy as np
import torch

from marqo_amd import _lib as L
from marqo_amd.engine.archs import QwenArch
from marqo_amd.engine.tower_weights import qwen_state_dict
from marqo_amd.engine.towers import _TextTowerBase, _check_precision, _host_i64, _large_call

Tensor = torch.Tensor


class QwenTower(_TextTowerBase):
    """Qwen3 / Qwen2 decoder + last-token / mean pooling (+ L2), the interface of BertTower: encode_ids(ids, attention_mask, normalize)."""

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

    @property
    def out_width(self) -> int:
        return self.arch.width

    def release_unused_folded(self) -> int:
        return 0     # (no folded norm copies are made for this tower)

    def queue_rows_ids(self, ids_h: np.ndarray, mask_h: np.ndarray, normalize: bool = True) -> Optional[np.ndarray]:
        return None  # (the native request queue serves mq_encode_bert / mq_encode_clip_text: this tower keeps the direct path)

    def encode_ids(self, ids: Tensor, attention_mask: Tensor, normalize: bool = True) -> Tensor:
        """ids / attention_mask: int [n, S], right-padded.  Only mask == 1 tokens are run: under the causal mask a padded position behind the text cannot
        reach a real row, and neither pooling reads one -> fp32 [n, width] on the device."""
        if ids.shape != attention_mask.shape or ids.ndim != 2:
            raise ValueError("ids and attention_mask must both be [n, S]")
        ids_h, mask_h = _host_i64(ids), _host_i64(attention_mask)
        n, S = ids_h.shape
        lengths = mask_h.sum(axis=1)
        if bool((lengths < 1).any()):
            raise ValueError("every sequence needs at least one unmasked token")
        if not bool(((mask_h != 0) == (np.arange(S)[None, :] < lengths[:, None])).all()):
            raise ValueError("attention_mask must be right-padded (a prefix of ones per row); left-padded input is not served")
        if n and int(lengths.max()) > self.arch.max_pos:
            raise ValueError(f"sequence longer than max_position_embeddings={self.arch.max_pos}")
        out = torch.empty(n, self.arch.width, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device), _large_call(self.device, int(lengths.sum())):
            for a, b in self._chunks(lengths):
                d_packed, d_cu, cu = self._stage_host(ids_h, lengths, a, b)
                ws = self._workspace(self.lib.mq_qwen_workspace_bytes(C.byref(self.cfg), d_packed.numel(), b - a))
                L.check(self.lib.mq_encode_qwen(C.byref(self.cfg), C.byref(self.w), d_packed.data_ptr(), d_cu.data_ptr(), cu.data_ptr(), b - a,
                                                out[a:b].data_ptr(), 1 if normalize else 0, ws.data_ptr(), ws.numel(), self._stream()),
                        "mq_encode_qwen")
        return out

"""EmbeddingGemma text tower: transformers' Gemma3TextModel checkpoints with use_bidirectional_attention (model_type "gemma3_text":
google/embeddinggemma-300m and its fine-tunes) -> HBM layout -> one mq_encode_gemma call per batch of packed sequences (csrc/gemma.hip; the 256-wide
grouped-query band attention kernel: csrc/attention_gqa256.hip).

bf16 GEMM operands, fp32 residual stream, 256-wide heads.  The checkpoint-to-tensor transform (names, the 1 + w norm weights, the fused QKV and
(up | gate) weights) is engine/tower_weights.py::gemma_state_dict.  `dense`: the weights of sentence-transformers Dense modules (bias-free, identity
activation) applied to the pooled rows in front of the L2 normalisation — the `sbert` pipeline of the model card; the bare encoder (`hf`) has none."""
from __future__ import annotations

from typing import Dict, Sequence

import torch

from marqo_amd import _lib as L
from marqo_amd.engine.archs import GemmaArch
from marqo_amd.engine.tower_weights import gemma_state_dict
from marqo_amd.engine.towers import _PackedTextTower, _check_precision

Tensor = torch.Tensor


class GemmaTower(_PackedTextTower):
    """EmbeddingGemma encoder + mean / CLS pooling (+ Dense modules) (+ L2); the call loop and the input checks are _PackedTextTower's."""
    family = "gemma"

    def __init__(self, arch: GemmaArch, sd: Dict[str, Tensor], device: str, pooling: str = "mean", precision: str = "bf16",
                 dense: Sequence[Tensor] = ()):
        super().__init__(device)
        _check_precision(precision, ("bf16",), f"the Gemma tower runs on bf16 operands only (its RMSNorm / rotary / gated tanh-GELU blocks have no e4m3 "
                                               f"kernels), got precision {precision!r}")
        if arch.head_dim != 256:
            raise ValueError(f"the Gemma tower runs 256-wide attention heads only (head_dim {arch.head_dim})")
        if arch.heads < 1 or arch.kv_heads < 1 or arch.heads % arch.kv_heads:
            raise ValueError(f"heads {arch.heads} must be a multiple of kv_heads {arch.kv_heads}")
        if arch.width > 2048 or arch.width % 64:
            raise ValueError(f"the Gemma tower runs widths that are multiples of 64 up to 2048 (width {arch.width})")
        if len(arch.sliding) != arch.layers:
            raise ValueError(f"arch.sliding names {len(arch.sliding)} layers, the model has {arch.layers}")
        if pooling not in ("mean", "cls"):
            raise ValueError(f"pooling must be 'mean' or 'cls', got {pooling!r}")
        self.precision, self.arch, self.pooling = precision, arch, pooling
        self._fp8 = None
        h = self._h
        t = gemma_state_dict(arch, sd)
        W = arch.width
        self._layers = (L.GemmaLayer * arch.layers)()
        for l in range(arch.layers):
            p = f"layers.{l}."
            a = p + "self_attn."
            self._layers[l] = L.GemmaLayer(
                input_norm_g=h.f32(t[p + "input_layernorm.weight"]), qkv_w=h.bf16(t[a + "qkv.weight"]), q_norm_g=h.f32(t[a + "q_norm.weight"]),
                k_norm_g=h.f32(t[a + "k_norm.weight"]), out_w=h.bf16(t[a + "o_proj.weight"]),
                post_attn_norm_g=h.f32(t[p + "post_attention_layernorm.weight"]), pre_ffn_norm_g=h.f32(t[p + "pre_feedforward_layernorm.weight"]),
                ug_w=h.bf16(t[p + "mlp.up_gate.weight"]), down_w=h.bf16(t[p + "mlp.down_proj.weight"]),
                post_ffn_norm_g=h.f32(t[p + "post_feedforward_layernorm.weight"]), sliding=1 if arch.sliding[l] else 0, reserved=0)
        self.w = L.GemmaWeights(tok_emb=h.f32(t["embed_tokens.weight"]), final_norm_g=h.f32(t["norm.weight"]),
                                d_inv_freq_global=h.f32(arch.inv_freq(local=False)), d_inv_freq_local=h.f32(arch.inv_freq(local=True)), layers=self._layers)
        self.cfg = L.GemmaCfg(width=W, layers=arch.layers, q_heads=arch.heads, kv_heads=arch.kv_heads, head_dim=arch.head_dim, mlp_dim=arch.mlp_dim,
                              vocab=arch.vocab, max_pos=arch.max_pos, half_window=arch.half_window,
                              pool=L.MQ_POOL_CLS if pooling == "cls" else L.MQ_POOL_MEAN, rms_eps=arch.rms_eps, attn_scale=arch.attn_scale)
        # sentence-transformers Dense modules behind the pooling: weight [out, in], no bias, identity activation
        self._dense = []
        width = W
        for i, wt in enumerate(dense):
            if wt.ndim != 2 or wt.shape[1] != width or wt.shape[0] % 8 or wt.shape[1] % 8:
                raise ValueError(f"Dense module {i}: weight {tuple(wt.shape)} does not continue a row of width {width} (both sides multiples of 8)")
            self._dense.append((h.bf16(wt.detach().to(torch.float32)), int(wt.shape[0]), int(wt.shape[1])))
            width = int(wt.shape[0])
        self._out_width = width

    @property
    def out_width(self) -> int:
        return self._out_width

    def _tail(self):
        return self._apply_dense if self._dense else None

    def _apply_dense(self, rows: Tensor, normalize: bool) -> Tensor:
        """pooled fp32 [n, W] -> Dense modules on the bf16 GEMM (fp32 out) -> L2 when asked"""
        s = self._stream()
        x = rows
        for wp, n_out, n_in in self._dense:
            xb = x.to(torch.bfloat16).contiguous()
            y = torch.empty(x.shape[0], n_out, dtype=torch.float32, device=self.device)
            L.check(self.lib.mq_gemm_bf16(xb.data_ptr(), n_in, wp, n_in, None, None, y.data_ptr(), n_out, x.shape[0], n_out, n_in, L.MQ_EPI_OUT_F32, s),
                    "mq_gemm_bf16")
            x = y
        if normalize:
            L.check(self.lib.mq_l2_normalize(x.data_ptr(), x.data_ptr(), x.shape[0], x.shape[1], s), "mq_l2_normalize")
        return x

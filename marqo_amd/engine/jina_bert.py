"""JinaBERT text tower: jina-embeddings-v2-small-en / -base-en, their fine-tunes and MosaicBERT-style ALiBi encoders with the same block (config.json:
model_type "bert" with position_embedding_type "alibi") -> HBM layout -> one mq_encode_jina_bert call per batch of packed sequences (csrc/jina_bert.hip;
the ALiBi attention kernel: csrc/attention_alibi.hip).

bf16 GEMM operands, fp32 residual stream, 64-wide heads.  The checkpoint-to-tensor transform (names, the fused QKV and the (up | gate) reorder) is
engine/tower_weights.py::jina_bert_state_dict; the head slopes are JinaBertArch.slopes().  The block semantics restate the published architecture: the
checkpoints are custom remote code, and nothing here is pinned to a run of the original modelling code."""
from __future__ import annotations

from typing import Dict

import torch

from marqo_amd import _lib as L
from marqo_amd.engine.archs import JinaBertArch
from marqo_amd.engine.tower_weights import jina_bert_state_dict
from marqo_amd.engine.towers import _PackedTextTower, _check_precision

Tensor = torch.Tensor


class JinaBertTower(_PackedTextTower):
    """JinaBERT encoder + mean / CLS pooling (+ L2); the call loop and the input checks are _PackedTextTower's."""
    family = "jina_bert"

    def __init__(self, arch: JinaBertArch, sd: Dict[str, Tensor], device: str, pooling: str = "mean", precision: str = "bf16"):
        super().__init__(device)
        _check_precision(precision, ("bf16",), f"the JinaBERT tower runs on bf16 operands only (its ALiBi attention / gated-GELU blocks have no e4m3 "
                                               f"kernels), got precision {precision!r}")
        if arch.head_dim != 64 or arch.width != arch.heads * 64:
            raise ValueError(f"the JinaBERT tower runs 64-wide attention heads only (hidden_size {arch.width}, num_attention_heads {arch.heads})")
        if arch.width > 2048:
            raise ValueError(f"the JinaBERT tower runs widths up to 2048 (hidden_size {arch.width})")
        if pooling not in ("mean", "cls"):
            raise ValueError(f"pooling must be 'mean' or 'cls', got {pooling!r}")
        self.precision, self.arch, self.pooling = precision, arch, pooling
        self._fp8 = None
        h = self._h
        t = jina_bert_state_dict(arch, sd)
        self._layers = (L.JinaBertLayer * arch.layers)()
        for l in range(arch.layers):
            p = f"layer.{l}."
            self._layers[l] = L.JinaBertLayer(qkv_w=h.bf16(t[p + "attn.qkv.weight"]), qkv_b=h.f32(t[p + "attn.qkv.bias"]), out_w=h.bf16(t[p + "attn.o.weight"]),
                                              out_b=h.f32(t[p + "attn.o.bias"]), attn_ln_g=h.f32(t[p + "attn_ln.weight"]), attn_ln_b=h.f32(t[p + "attn_ln.bias"]),
                                              wg_w=h.bf16(t[p + "mlp.up_gate.weight"]), wo_w=h.bf16(t[p + "mlp.wo.weight"]), wo_b=h.f32(t[p + "mlp.wo.bias"]),
                                              mlp_ln_g=h.f32(t[p + "mlp_ln.weight"]), mlp_ln_b=h.f32(t[p + "mlp_ln.bias"]))
        self.w = L.JinaBertWeights(tok_emb=h.f32(t["word_embeddings.weight"]), type0=h.f32(t["type0"]), emb_ln_g=h.f32(t["emb_ln.weight"]),
                                   emb_ln_b=h.f32(t["emb_ln.bias"]), d_slopes=h.f32(torch.tensor(arch.slopes(), dtype=torch.float64).to(torch.float32)),
                                   layers=self._layers)
        self.cfg = L.JinaBertCfg(width=arch.width, layers=arch.layers, heads=arch.heads, head_dim=arch.head_dim, mlp_dim=arch.mlp_dim, vocab=arch.vocab,
                                 max_pos=arch.max_pos, pool=L.MQ_POOL_CLS if pooling == "cls" else L.MQ_POOL_MEAN, ln_eps=arch.ln_eps, reserved=0)

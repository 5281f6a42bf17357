"""Mixture-of-experts NomicBERT text tower: nomic-embed-text-v2-moe (config.json: model_type "nomic_bert" with moe_every_n_layers / num_experts /
moe_top_k; the hub's original tensor names) -> HBM layout -> one mq_encode_nomic_moe call per batch of packed sequences (csrc/nomic_moe.hip; the router,
the device-side plan and the grouped GEMM: csrc/moe.hip).

bf16 GEMM operands, fp32 residual stream, fp32 router weights (the router reads the fp32 stream), 64-wide heads, sequences up to 8192 tokens.  The
checkpoint-to-tensor transform (which blocks are routed, the per-expert slices, the w2 transpose) is engine/tower_weights.py::nomic_moe_state_dict; the
rotary frequencies are NomicMoeArch.inv_freq().  The block semantics are written from memory of the hub's modeling file and pinned to a float64
restatement of them (tests/nomic_moe_ref.py), not to the hub's code: no copy of it was at hand."""
from __future__ import annotations

from typing import Dict

import torch

from marqo_amd import _lib as L
from marqo_amd.engine.archs import NomicMoeArch
from marqo_amd.engine.tower_weights import nomic_moe_state_dict
from marqo_amd.engine.towers import _PackedTextTower, _check_precision

Tensor = torch.Tensor


class NomicMoeTower(_PackedTextTower):
    """MoE NomicBERT encoder + mean / CLS pooling (+ L2); the call loop and the input checks are _PackedTextTower's."""
    family = "nomic_moe"

    def __init__(self, arch: NomicMoeArch, sd: Dict[str, Tensor], device: str, pooling: str = "mean", precision: str = "bf16"):
        super().__init__(device)
        _check_precision(precision, ("bf16",), f"the mixture-of-experts NomicBERT tower runs on bf16 operands only (its rotary blocks and grouped GEMM have "
                                               f"no e4m3 kernels), got precision {precision!r}")
        if arch.head_dim != 64 or arch.width != arch.heads * 64:
            raise ValueError(f"the mixture-of-experts NomicBERT tower runs 64-wide attention heads only (n_embd {arch.width}, n_head {arch.heads})")
        if arch.width > 2048:
            raise ValueError(f"the mixture-of-experts NomicBERT tower runs widths up to 2048 (n_embd {arch.width})")
        if not 2 <= arch.experts <= 16 or arch.top_k not in (1, 2) or arch.top_k > arch.experts:
            raise ValueError(f"the mixture-of-experts NomicBERT tower routes to 1 or 2 of 2 .. 16 experts (num_experts {arch.experts}, moe_top_k {arch.top_k})")
        if pooling not in ("mean", "cls"):
            raise ValueError(f"pooling must be 'mean' or 'cls', got {pooling!r}")
        self.precision, self.arch, self.pooling = precision, arch, pooling
        self._fp8 = None
        h = self._h
        t = nomic_moe_state_dict(arch, sd)
        self._layers = (L.NomicMoeLayer * arch.layers)()
        self.routed_layers = tuple(l for l in range(arch.layers) if f"layer.{l}.moe.router.weight" in t)
        for l in range(arch.layers):
            p = f"layer.{l}."
            lay = dict(qkv_w=h.bf16(t[p + "attn.qkv.weight"]), qkv_b=h.f32(t[p + "attn.qkv.bias"]), out_w=h.bf16(t[p + "attn.o.weight"]),
                       out_b=h.f32(t[p + "attn.o.bias"]), attn_ln_g=h.f32(t[p + "attn_ln.weight"]), attn_ln_b=h.f32(t[p + "attn_ln.bias"]),
                       mlp_ln_g=h.f32(t[p + "mlp_ln.weight"]), mlp_ln_b=h.f32(t[p + "mlp_ln.bias"]))
            if l in self.routed_layers:
                lay.update(router_w=h.f32(t[p + "moe.router.weight"]), w1=h.bf16(t[p + "moe.w1"]), w2t=h.bf16(t[p + "moe.w2t"]),
                           experts_b=h.f32(t[p + "moe.bias"]))
            else:
                lay.update(fc1_w=h.bf16(t[p + "mlp.fc1.weight"]), fc1_b=h.f32(t[p + "mlp.fc1.bias"]), fc2_w=h.bf16(t[p + "mlp.fc2.weight"]),
                           fc2_b=h.f32(t[p + "mlp.fc2.bias"]))
            self._layers[l] = L.NomicMoeLayer(**lay)
        self.w = L.NomicMoeWeights(tok_emb=h.f32(t["word_embeddings.weight"]), type0=h.f32(t["type0"]), emb_ln_g=h.f32(t["emb_ln.weight"]),
                                   emb_ln_b=h.f32(t["emb_ln.bias"]), d_inv_freq=h.f32(arch.inv_freq()), layers=self._layers)
        self.cfg = L.NomicMoeCfg(width=arch.width, layers=arch.layers, heads=arch.heads, head_dim=arch.head_dim, mlp_dim=arch.mlp_dim, vocab=arch.vocab,
                                 max_pos=arch.max_pos, pool=L.MQ_POOL_CLS if pooling == "cls" else L.MQ_POOL_MEAN, ln_eps=arch.ln_eps,
                                 experts=arch.experts, top_k=arch.top_k, reserved=0)

"""Mistral / Llama text tower: transformers' MistralModel / LlamaModel checkpoints (model_type "mistral" / "llama": e5-mistral-7b-instruct,
SFR-Embedding-Mistral, Linq-Embed-Mistral, Llama-2-shaped fine-tunes) -> HBM layout -> one mq_encode_llama call per batch of packed sequences
(csrc/llama.hip; the causal sliding-window grouped-query attention kernel: csrc/attention_gqa.hip).

bf16 GEMM operands, fp32 residual stream, 64- or 128-wide heads, widths up to 4096.  weight_precision="e4m3" keeps a second, e4m3 copy of the four block
weights (one power-of-two scale per output row) that the query path streams instead of the bf16 one (csrc/gemm_small_w8.hip: W8A16, bf16 activations);
the bf16 copy is rewritten with the dequantised values, so every batch size embeds with the same model.  weight_precision="mxfp4" does the same with
OCP MX FP4 copies (e2m1 codes, one e8m0 scale per 32 consecutive k: 4.25 bits per weight; csrc/gemm_small_w4.hip: W4A16).  weight_precision="mxfp4-only"
keeps the MX FP4 copy ALONE: every block matrix is quantised on the device and its bf16 tensor dropped, batches too tall for the skinny kernel run the
tiled W4A16 GEMM (csrc/gemm_w4.hip), and the block weights take 0.27 x their bf16 bytes.  weight_precision="mxfp4-a8" loads and keeps exactly what
"mxfp4-only" does; a batch too tall for the skinny kernel quantises each block GEMM's input rows to MX FP8 (e4m3 codes, one e8m0 scale per 32 k) and runs
the W4A8 GEMM on the MX matrix instruction (csrc/gemm_w4a8.hip); shorter calls give "mxfp4-only"'s bits.  The block is the Qwen tower's without q / k norm and without biases,
so the checkpoint-to-tensor transform (names, the fused QKV and (up | gate) weights) is engine/tower_weights.py::qwen_state_dict and the weight structs
are the Qwen tower's."""
from __future__ import annotations

import ctypes as C
from typing import Dict

import torch

from marqo_amd import _lib as L
from marqo_amd.engine.archs import LlamaArch
from marqo_amd.engine.tower_weights import qwen_state_dict
from marqo_amd.engine.towers import _PackedTextTower, _check_precision

Tensor = torch.Tensor


class LlamaTower(_PackedTextTower):
    """Mistral / Llama decoder + last-token / mean pooling (+ L2); the call loop and the input checks are _PackedTextTower's."""
    family = "llama"

    def __init__(self, arch: LlamaArch, sd: Dict[str, Tensor], device: str, pooling: str = "last", precision: str = "bf16", weight_precision: str = "bf16"):
        super().__init__(device)
        if weight_precision not in ("bf16", "e4m3", "mxfp4", "mxfp4-only", "mxfp4-a8"):
            raise ValueError(f"weight_precision must be 'bf16' or 'e4m3' or 'mxfp4' or 'mxfp4-only' or 'mxfp4-a8', got {weight_precision!r}")
        _check_precision(precision, ("bf16",), f"the Mistral / Llama tower runs on bf16 operands only (its RMSNorm / rotary / gated-SiLU blocks have no e4m3 "
                                               f"kernels), got precision {precision!r}")
        if arch.head_dim not in (64, 128):
            raise ValueError(f"the Mistral / Llama tower runs 64- or 128-wide attention heads only (head_dim {arch.head_dim})")
        if arch.heads < 1 or arch.kv_heads < 1 or arch.heads % arch.kv_heads:
            raise ValueError(f"heads {arch.heads} must be a multiple of kv_heads {arch.kv_heads}")
        if arch.width > 4096 or arch.width % 64:
            raise ValueError(f"the Mistral / Llama tower runs widths that are multiples of 64 up to 4096 (width {arch.width})")
        if arch.window is not None and arch.window < 1:
            raise ValueError(f"window must be at least 1 or None, got {arch.window}")
        if pooling not in ("last", "mean"):
            raise ValueError(f"pooling must be 'last' or 'mean', got {pooling!r}")
        self.precision, self.arch, self.pooling, self.weight_precision = precision, arch, pooling, weight_precision
        self._fp8 = None
        h = self._h
        t = qwen_state_dict(arch, sd, tower="Mistral / Llama")
        W = arch.width
        self._layers = (L.QwenLayer * arch.layers)()
        only = weight_precision in ("mxfp4-only", "mxfp4-a8")
        host = {}   # "mxfp4-only" / "mxfp4-a8": the block matrices stay on the host until _quantize_mxfp4 takes them one at a time; the layers carry null pointers
        for l in range(arch.layers):
            p = f"layers.{l}."
            a = p + "self_attn."
            m = {"qkv": t.pop(a + "qkv.weight"), "out": t.pop(a + "o_proj.weight"), "ug": t.pop(p + "mlp.up_gate.weight"), "down": t.pop(p + "mlp.down_proj.weight")}
            if only:
                host[l] = m
            up = (lambda x: None) if only else h.bf16
            self._layers[l] = L.QwenLayer(
                input_norm_g=h.f32(t.pop(p + "input_layernorm.weight")), qkv_w=up(m["qkv"]), qkv_b=None, q_norm_g=None, k_norm_g=None,
                out_w=up(m["out"]), post_norm_g=h.f32(t.pop(p + "post_attention_layernorm.weight")), ug_w=up(m["ug"]), down_w=up(m["down"]))
        self.w = L.QwenWeights(tok_emb=h.f32(t["embed_tokens.weight"]), final_norm_g=h.f32(t["norm.weight"]), zeros=h.f32(torch.zeros(W)),
                               d_inv_freq=h.f32(arch.inv_freq()), layers=self._layers)
        self.cfg = L.LlamaCfg(width=W, layers=arch.layers, q_heads=arch.heads, kv_heads=arch.kv_heads, head_dim=arch.head_dim, mlp_dim=arch.mlp_dim,
                              vocab=arch.vocab, max_pos=arch.max_pos, pool=L.MQ_POOL_LAST if pooling == "last" else L.MQ_POOL_MEAN,
                              window=int(arch.window or 0), rms_eps=arch.rms_eps, reserved0=0)
        if weight_precision == "e4m3":
            self._quantize_e4m3()
        elif weight_precision == "mxfp4":
            self._quantize_mxfp4()
        elif only:
            self._quantize_mxfp4(host)

    def block_weight(self, layer: int, name: str) -> Tensor:
        """the bf16 device tensor of one block matrix ('qkv', 'out', 'ug', 'down') as the kernels read it (with weight_precision 'e4m3' / 'mxfp4': dequantised).
        'mxfp4-only' / 'mxfp4-a8' hold no such tensor: the matrix is decoded on demand from the codes — mq_gemm_w4 on rows of the identity, every output one
        product and therefore exact — into a fresh tensor (a test and debugging aid)"""
        if self.weight_precision not in ("mxfp4-only", "mxfp4-a8"):
            ptr = getattr(self._layers[layer], name + "_w")
            return next(t for t in self._h.tensors if t.data_ptr() == ptr)
        w4, sc, n, k = self._w4_blocks[layer, name]
        out = torch.empty(n, k, dtype=torch.bfloat16, device=self.device)
        with torch.cuda.device(self.device):
            for r0 in range(0, k, 1024):
                rows = min(1024, k - r0)
                eye = torch.zeros(rows, k, dtype=torch.bfloat16, device=self.device)
                eye[torch.arange(rows), torch.arange(r0, r0 + rows)] = 1
                wt = torch.empty(rows, n, dtype=torch.bfloat16, device=self.device)
                L.check(self.lib.mq_gemm_w4(eye.data_ptr(), k, w4.data_ptr(), w4.shape[1], sc.data_ptr(), sc.shape[1], None, None, wt.data_ptr(), n, rows, n, k, 0,
                                            self._stream()), "mq_gemm_w4")
                out[:, r0:r0 + rows] = wt.t()
            # a GEMM's sum starts at +0, so a -0 weight (code 8) comes back as +0: the sign of a zero is read from its code (the storage note of
            # csrc/gemm_small_w4.hip: byte g 16 + j 4 + i of a chunk holds k = j 32 + g 8 + i in its low nibble and k + 4 in its high one)
            b = w4.view(n, -1, 4, 4, 4)
            codes = torch.cat((b & 15, b >> 4), dim=-1).permute(0, 1, 3, 2, 4).reshape(n, -1)[:, :k]
            out[codes == 8] = -0.0
        return out

    def _quantize_e4m3(self) -> None:
        """the e4m3 copy of every layer's four matrices, made on the device from the uploaded bf16 weights, which are rewritten with the dequantised
        values (mq_quantize_weights_pow2): 1.5 x the weight memory, one model on the skinny and the tiled path"""
        a = self.arch
        if a.width % 64 or a.mlp_dim % 64 or (a.heads * a.head_dim) % 64:
            raise ValueError("weight_precision 'e4m3' needs width, mlp_dim and heads * head_dim to be multiples of 64")
        aw, qkvw = a.heads * a.head_dim, (a.heads + 2 * a.kv_heads) * a.head_dim
        shapes = (("qkv", qkvw, a.width), ("out", a.width, aw), ("ug", 2 * a.mlp_dim, a.width), ("down", a.width, a.mlp_dim))
        self._w8_layers = (L.W8Layer * a.layers)()
        with torch.cuda.device(self.device):
            for l in range(a.layers):
                for name, n, k in shapes:
                    w8 = torch.empty(n, k, dtype=torch.uint8, device=self.device)
                    sc = torch.empty(n, dtype=torch.float32, device=self.device)
                    L.check(self.lib.mq_quantize_weights_pow2(getattr(self._layers[l], name + "_w"), k, w8.data_ptr(), k, sc.data_ptr(), n, k, self._stream()),
                            "mq_quantize_weights_pow2")
                    self._h.tensors += [w8, sc]
                    setattr(self._w8_layers[l], name + "_w8", w8.data_ptr())
                    setattr(self._w8_layers[l], name + "_scale", sc.data_ptr())
            torch.cuda.current_stream(self.device).synchronize()
        self._entry = ("mq_encode_llama_w8", (self._w8_layers,))

    def _quantize_mxfp4(self, host=None) -> None:
        """the MXFP4 copy of every layer's four matrices (packed e2m1 codes, 64 bytes per 128-deep chunk of a row, and e8m0 block scales, 4 bytes per
        chunk), made on the device from the uploaded bf16 weights, which are rewritten with the dequantised values (mq_quantize_weights_mxfp4):
        1.27 x the weight memory, one model on the skinny and the tiled path.  host ("mxfp4-only"): {layer: {name: matrix}} not yet uploaded — each is
        uploaded, quantised and its bf16 tensor dropped before the next (peak overhead: one matrix); 68 bytes per 128-deep chunk of a row stay"""
        a = self.arch
        if a.width % 64 or a.mlp_dim % 64 or (a.heads * a.head_dim) % 64:
            raise ValueError(f"weight_precision {self.weight_precision!r} needs width, mlp_dim and heads * head_dim to be multiples of 64")
        aw, qkvw = a.heads * a.head_dim, (a.heads + 2 * a.kv_heads) * a.head_dim
        shapes = (("qkv", qkvw, a.width), ("out", a.width, aw), ("ug", 2 * a.mlp_dim, a.width), ("down", a.width, a.mlp_dim))
        self._w4_layers = (L.W4Layer * a.layers)()
        self._w4_blocks = {}
        with torch.cuda.device(self.device):
            for l in range(a.layers):
                for name, n, k in shapes:
                    chunks = (k + 127) // 128
                    w4 = torch.empty(n, chunks * 64, dtype=torch.uint8, device=self.device)
                    sc = torch.empty(n, chunks * 4, dtype=torch.uint8, device=self.device)
                    if host is not None and tuple(host[l][name].shape) != (n, k):
                        raise ValueError(f"layer {l} {name}: weight of shape {tuple(host[l][name].shape)}, expected {(n, k)}")
                    src = getattr(self._layers[l], name + "_w") if host is None else self._h.bf16(host[l].pop(name))
                    L.check(self.lib.mq_quantize_weights_mxfp4(src, k, w4.data_ptr(), chunks * 64, sc.data_ptr(), chunks * 4, n, k, self._stream()),
                            "mq_quantize_weights_mxfp4")
                    if host is not None:   # (the allocator hands the block on in stream order: behind the quantiser that reads it)
                        self._h.drop(src)
                        self._w4_blocks[l, name] = (w4, sc, n, k)
                    self._h.tensors += [w4, sc]
                    setattr(self._w4_layers[l], name + "_w4", w4.data_ptr())
                    setattr(self._w4_layers[l], name + "_scale", sc.data_ptr())
            torch.cuda.current_stream(self.device).synchronize()
        self._entry = ("mq_encode_llama_w4" if host is None else "mq_encode_llama_w4_only", (self._w4_layers,))
        if self.weight_precision == "mxfp4-a8":   # the same resident tensors; the workspace also holds the MX FP8 copy of a GEMM's input rows
            self._entry, self._workspace_query = ("mq_encode_llama_w4a8", (self._w4_layers,)), "mq_llama_w4a8_workspace_bytes"

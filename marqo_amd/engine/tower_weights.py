"""Checkpoint tensors -> the tensors the kernels read: every load-time transform of the towers (engine/towers.py) that needs no device.

Head and MLP padding, LayerNorm / BatchNorm / layer-scale folding, key renaming and the per-block hand-over to a `_Holder` (which may sit on
the CPU: tests/test_tower_weights_host.py runs the block loaders there).  The order in which tensors reach the holder is the allocation
order of a tower's weights on the device."""
from __future__ import annotations

import math
import os
from typing import Dict, List, Optional, Tuple

import torch

from marqo_amd import _lib as L

Tensor = torch.Tensor


class _Holder:
    """Keeps device tensors alive and hands out raw pointers."""

    def __init__(self, device: torch.device):
        self.device = device
        self.tensors: List[Tensor] = []

    def f32(self, t: Tensor) -> int:
        d = t.detach().to(device=self.device, dtype=torch.float32).contiguous()
        self.tensors.append(d)
        return d.data_ptr()

    def bf16(self, t: Tensor) -> int:
        d = t.detach().to(dtype=torch.float32).to(device=self.device).to(torch.bfloat16).contiguous()
        self.tensors.append(d)
        return d.data_ptr()

    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in self.tensors)

    def drop(self, ptr: int) -> int:
        """forget the tensor that starts at `ptr` (its HBM goes back to the allocator once nothing else holds it) -> bytes released"""
        for i, t in enumerate(self.tensors):
            if t.data_ptr() == ptr:
                del self.tensors[i]
                return t.numel() * t.element_size()
        return 0


def _need(sd: Dict[str, Tensor], key: str, shape: Optional[Tuple[int, ...]] = None) -> Tensor:
    if key not in sd:
        raise KeyError(f"checkpoint is missing tensor '{key}'")
    t = sd[key]
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"checkpoint tensor '{key}' has shape {tuple(t.shape)}, expected {tuple(shape)}")
    return t


def _head_dim(width: int, heads: int) -> int:
    """model head dim; the attention kernel runs 64- / 96- / 112- / 128-wide heads, anything else is zero-padded at load (_pad_heads)"""
    if heads < 1 or width % heads:
        raise ValueError(f"width {width} is not divisible by heads {heads}")
    d = width // heads
    if d > 128:
        raise ValueError(f"attention head dim must be <= 128 for the gfx950 attention kernel (width={width}, heads={heads}: {d})")
    return d


KERNEL_HEAD_DIMS = (64, 96, 112, 128)  # head strides csrc/attention.hip is instantiated for


def _kernel_head_dim(d: int, heads: int = 2) -> int:
    """head width the kernel runs for a model head dim d: the smallest instantiated stride >= d whose attention width heads * hp
    keeps the GEMM's K a multiple of 64: 32 / 16 -> 64 (e5-small, MiniLM), 80 / 88 -> 96 (ViT-H / g), 104 -> 112 (ViT-bigG)"""
    for hp in KERNEL_HEAD_DIMS:
        if hp >= d and (heads * hp) % 64 == 0:
            return hp
    return 128


def _pad_heads(qkv_w: Tensor, qkv_b: Tensor, out_w: Tensor, heads: int, d: int) -> Tuple[Tensor, Tensor, Tensor]:
    """[3W, W] / [3W] / [W, W] with d-wide heads -> [3*heads*hp, W] / [3*heads*hp] / [W, heads*hp] (hp = _kernel_head_dim): each
    head's Q / K / V rows and out-projection columns are zero-padded to hp (zero key / query dims add nothing to q.k, zero value
    dims meet zero out-proj columns), and Q is scaled by sqrt(hp / d) so that the kernel's 1/sqrt(hp) softmax scale equals the
    model's 1/sqrt(d)."""
    W = out_w.shape[0]
    hp = _kernel_head_dim(d, heads)
    q, k, v = qkv_w.float().view(3, heads, d, W).unbind(0)
    qb, kb, vb = qkv_b.float().view(3, heads, d).unbind(0)
    sc = (float(hp) / d) ** 0.5
    pad_w = lambda t: torch.nn.functional.pad(t, (0, 0, 0, hp - d)).reshape(heads * hp, W)
    pad_b = lambda t: torch.nn.functional.pad(t, (0, hp - d)).reshape(heads * hp)
    qkv_w2 = torch.cat([pad_w(q * sc), pad_w(k), pad_w(v)], 0)
    qkv_b2 = torch.cat([pad_b(qb * sc), pad_b(kb), pad_b(vb)], 0)
    out_w2 = torch.nn.functional.pad(out_w.float().view(W, heads, d), (0, hp - d)).reshape(W, heads * hp)
    return qkv_w2, qkv_b2, out_w2


def _ceil64(v: int) -> int:
    return (v + 63) // 64 * 64


def patch_embed_weight(sd: Dict[str, Tensor], key: str, W: int, P: int) -> Tensor:
    """the patch-embedding conv weight sd[key] [W, 3, P, P] -> fp32 [W, Kp]: the GEMM's operand, K = 3 P P columns in (c, ky, kx) order,
    zero-padded to Kp = the next multiple of 64 (the tiled GEMMs' k-step; callers read Kp from the result's shape)"""
    K = 3 * P * P
    return torch.nn.functional.pad(_need(sd, key, (W, 3, P, P)).detach().to(torch.float32).reshape(W, K), (0, _ceil64(K) - K))


def _pad_mlp(fc1_w: Tensor, fc1_b: Tensor, fc2_w: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    """MLP hidden sizes that are not a multiple of 64 (ViT-SO400M: 4304) are zero-padded: the extra hidden units are act(0 + 0) = 0
    for GELU / QuickGELU and meet zero fc2 columns — exact."""
    F = fc1_w.shape[0]
    Fp = _ceil64(F)
    if Fp == F:
        return fc1_w, fc1_b, fc2_w
    pad = torch.nn.functional.pad
    return pad(fc1_w.detach().float(), (0, 0, 0, Fp - F)), pad(fc1_b.detach().float(), (0, Fp - F)), pad(fc2_w.detach().float(), (0, Fp - F))


# LayerNorm folding of the pre-LN CLIP blocks (csrc/gemm_epilogue.h, MQ_EPI_LN_APPLY): the loaders prepare gamma-folded copies of the QKV / fc1
# weights (+ folded bias and column sums); on the bf16 residual stream the tiled GEMMs then read the stream itself and no LayerNorm kernel runs in
# front of them.  The un-folded weights stay for the small-call kernels (fused-LayerNorm skinny GEMMs) and the fp32-stream towers.
# MARQO_AMD_LN_FOLD=0: do not build the folded tensors (the towers then always launch their LayerNorms).
LN_FOLD = os.environ.get("MARQO_AMD_LN_FOLD", "1") != "0"


# per-block tensor names: open_clip ResidualAttentionBlock / timm Block (the SigLIP trunks)
_OPEN_CLIP_KEYS = dict(block="resblocks.{}.", ln1="ln_1", qkv_w="attn.in_proj_weight", qkv_b="attn.in_proj_bias", out="attn.out_proj",
                       ln2="ln_2", fc1="mlp.c_fc", fc2="mlp.c_proj")
_TIMM_KEYS = dict(block="blocks.{}.", ln1="norm1", qkv_w="attn.qkv.weight", qkv_b="attn.qkv.bias", out="attn.proj",
                  ln2="norm2", fc1="mlp.fc1", fc2="mlp.fc2")


def fold_layernorm(w: Tensor, b: Tensor, gamma: Tensor, beta: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    """A LayerNorm folded into the linear layer behind it (csrc/gemm_epilogue.h, MQ_EPI_LN_APPLY; mq_gemm_bf16_ln):
    LN(x) @ W^T + b = rstd * (x @ (g*W)^T - mean * colsum(g*W)) + (b + W @ beta)  -> (bf16 g*W [N, K], fp32 bias [N], fp32 colsum [N]).
    colsum is taken over the bf16-ROUNDED folded weight (what the MFMA multiplies), the bias in fp32 from the fp32 W.  Callers pass the tensors
    the block really runs (head- / MLP-padded where it pads)."""
    w32 = w.detach().to(torch.float32)
    wf = (w32 * gamma.detach().to(torch.float32).unsqueeze(0)).to(torch.bfloat16)
    return wf, b.detach().to(torch.float32) + w32 @ beta.detach().to(torch.float32), wf.to(torch.float32).sum(dim=1)


def _hand_over_fold(h: _Holder, b, name: str, w: Tensor, bias: Tensor, gamma: Tensor, beta: Tensor) -> None:
    """block fields <name>_wf / _sf / _bf = fold_layernorm(...), handed to the holder in that order"""
    wf, bf, sf = fold_layernorm(w, bias, gamma, beta)
    setattr(b, name + "_wf", h.bf16(wf))
    setattr(b, name + "_sf", h.f32(sf))
    setattr(b, name + "_bf", h.f32(bf))


def _clip_blocks(h: _Holder, sd, prefix: str, layers: int, W: int, F: int, heads: int, keys=_OPEN_CLIP_KEYS):
    d = _head_dim(W, heads)
    padded = d != _kernel_head_dim(d, heads)  # ViT-H / g / bigG: 80 / 88 / 104-wide heads run as 96 / 96 / 112
    arr = (L.BlockWeights * layers)()
    k = keys
    for i in range(layers):
        p = prefix + k["block"].format(i)
        b = arr[i]
        b.ln1_g = h.f32(_need(sd, p + k["ln1"] + ".weight", (W,)))
        b.ln1_b = h.f32(_need(sd, p + k["ln1"] + ".bias", (W,)))
        qkv_w, qkv_b = _need(sd, p + k["qkv_w"], (3 * W, W)), _need(sd, p + k["qkv_b"], (3 * W,))
        out_w = _need(sd, p + k["out"] + ".weight", (W, W))
        if padded:
            qkv_w, qkv_b, out_w = _pad_heads(qkv_w.detach(), qkv_b.detach(), out_w.detach(), heads, d)
        b.qkv_w, b.qkv_b, b.out_w = h.bf16(qkv_w), h.f32(qkv_b), h.bf16(out_w)
        b.out_b = h.f32(_need(sd, p + k["out"] + ".bias", (W,)))
        b.ln2_g = h.f32(_need(sd, p + k["ln2"] + ".weight", (W,)))
        b.ln2_b = h.f32(_need(sd, p + k["ln2"] + ".bias", (W,)))
        fc1_w, fc1_b, fc2_w = _pad_mlp(_need(sd, p + k["fc1"] + ".weight", (F, W)), _need(sd, p + k["fc1"] + ".bias", (F,)),
                                       _need(sd, p + k["fc2"] + ".weight", (W, F)))
        b.fc1_w, b.fc1_b, b.fc2_w = h.bf16(fc1_w), h.f32(fc1_b), h.bf16(fc2_w)
        b.fc2_b = h.f32(_need(sd, p + k["fc2"] + ".bias", (W,)))
        if LN_FOLD:   # ln_1 into the QKV GEMM, ln_2 into fc1
            for name, w_t, b_t, lg in (("qkv", qkv_w, qkv_b, k["ln1"]), ("fc1", fc1_w, fc1_b, k["ln2"])):
                _hand_over_fold(h, b, name, w_t, b_t, sd[p + lg + ".weight"], sd[p + lg + ".bias"])
    return arr


# EVA02 blocks: up * silu(gate) in the (up | gate) GEMM's epilogue (MQ_EPI_GLU; 0 = the round-5 form: the GEMM writes (up | gate), glu_ln_kernel multiplies)
EVA_GLU_EPILOGUE = os.environ.get("MARQO_AMD_EVA_GLU_EPILOGUE", "1") != "0"


def _eva_blocks(h: _Holder, sd, prefix: str, layers: int, W: int, F: int, heads: int):
    """timm EvaBlock tensors (eva.py; `blocks.{i}.`): norm1, attn.{q_proj, k_proj (no bias), v_proj} or the fused attn.qkv + q_bias / v_bias,
    attn.norm (the LayerNorm in front of attn.proj; absent without `scale_attn_inner`), attn.proj, norm2, mlp.{fc1_g, fc1_x, norm, fc2}
    (timm SwiGLU: fc2(norm(silu(fc1_g(x)) * fc1_x(x)))).  fc1 is stored as (up, gate) = (fc1_x, fc1_g) rows interleaved 16 by 16, the hidden width F zero-padded
    to a multiple of 64: silu(0) * 0 = 0 meets zero LayerNorm weights and zero fc2 columns — exact; the statistics run over F (mlp_ln_dim)."""
    if _head_dim(W, heads) != _kernel_head_dim(_head_dim(W, heads), heads):
        raise ValueError("EVA02 towers with heads that are not 64 / 96 / 112 / 128 wide are not runnable (rotary positions on padded heads)")
    Fp = _ceil64(F)
    pad = torch.nn.functional.pad
    arr = (L.BlockWeights * layers)()
    for i in range(layers):
        p = prefix + f"blocks.{i}."
        f32 = lambda k, shape: _need(sd, p + k, shape).detach().to(torch.float32)
        b = arr[i]
        b.ln1_g, b.ln1_b = h.f32(f32("norm1.weight", (W,))), h.f32(f32("norm1.bias", (W,)))
        if p + "attn.qkv.weight" in sd:
            qkv_w = f32("attn.qkv.weight", (3 * W, W))
            qb = f32("attn.q_bias", (W,)) if p + "attn.q_bias" in sd else torch.zeros(W)
            vb = f32("attn.v_bias", (W,)) if p + "attn.v_bias" in sd else torch.zeros(W)
        else:
            qkv_w = torch.cat([f32("attn.q_proj.weight", (W, W)), f32("attn.k_proj.weight", (W, W)), f32("attn.v_proj.weight", (W, W))], dim=0)
            qb = f32("attn.q_proj.bias", (W,)) if p + "attn.q_proj.bias" in sd else torch.zeros(W)
            vb = f32("attn.v_proj.bias", (W,)) if p + "attn.v_proj.bias" in sd else torch.zeros(W)
        qkv_b = torch.cat([qb, torch.zeros(W), vb])                                        # (keys carry no bias)
        b.qkv_w, b.qkv_b = h.bf16(qkv_w), h.f32(qkv_b)
        if p + "attn.norm.weight" in sd:
            b.attn_ln_g, b.attn_ln_b = h.f32(f32("attn.norm.weight", (W,))), h.f32(f32("attn.norm.bias", (W,)))
        b.out_w, b.out_b = h.bf16(f32("attn.proj.weight", (W, W))), h.f32(f32("attn.proj.bias", (W,)))
        b.ln2_g, b.ln2_b = h.f32(f32("norm2.weight", (W,))), h.f32(f32("norm2.bias", (W,)))
        up_w, up_b = f32("mlp.fc1_x.weight", (F, W)), f32("mlp.fc1_x.bias", (F,))
        gate_w, gate_b = f32("mlp.fc1_g.weight", (F, W)), f32("mlp.fc1_g.bias", (F,))
        # (up, gate) rows interleaved 16 by 16 (mq_encoder_cfg.mlp_glu = 2): a lane of the GEMM's epilogue then holds up AND gate of the same hidden
        # units and forms up * silu(gate) itself (MQ_EPI_GLU) — the (up | gate) tensor is never written
        il = (lambda u, g_: torch.stack([u.reshape(Fp // 16, 16, *u.shape[1:]), g_.reshape(Fp // 16, 16, *g_.shape[1:])], dim=1).reshape(2 * Fp, *u.shape[1:])) \
            if EVA_GLU_EPILOGUE else (lambda u, g_: torch.cat([u, g_], dim=0))
        fc1_w = il(pad(up_w, (0, 0, 0, Fp - F)), pad(gate_w, (0, 0, 0, Fp - F)))
        fc1_b = il(pad(up_b, (0, Fp - F)), pad(gate_b, (0, Fp - F)))
        b.fc1_w, b.fc1_b = h.bf16(fc1_w), h.f32(fc1_b)
        if p + "mlp.norm.weight" in sd:
            b.mlp_ln_g, b.mlp_ln_b = h.f32(pad(f32("mlp.norm.weight", (F,)), (0, Fp - F))), h.f32(pad(f32("mlp.norm.bias", (F,)), (0, Fp - F)))
        b.fc2_w, b.fc2_b = h.bf16(pad(f32("mlp.fc2.weight", (W, F)), (0, Fp - F))), h.f32(f32("mlp.fc2.bias", (W,)))
        if LN_FOLD:   # norm1 into the QKV GEMM, norm2 into the (up | gate) GEMM (as _clip_blocks)
            for name, w32, b32, lg in (("qkv", qkv_w, qkv_b, "norm1"), ("fc1", fc1_w, fc1_b, "norm2")):
                _hand_over_fold(h, b, name, w32, b32, f32(lg + ".weight", (W,)), f32(lg + ".bias", (W,)))
            # ... and the sub-LayerNorms into the GEMMs behind them (ABI 12, csrc/towers.hip block_eva): attn.norm into attn.proj, mlp.norm into mlp.fc2 (over
            # the padded hidden width: zero LayerNorm weights meet zero fc2 columns).  Their rows' statistics come from the attention kernel / the gated epilogue.
            subs = []
            if p + "attn.norm.weight" in sd:
                subs.append(("out", f32("attn.proj.weight", (W, W)), f32("attn.proj.bias", (W,)), f32("attn.norm.weight", (W,)), f32("attn.norm.bias", (W,))))
            if p + "mlp.norm.weight" in sd and EVA_GLU_EPILOGUE:
                subs.append(("fc2", pad(f32("mlp.fc2.weight", (W, F)), (0, Fp - F)), f32("mlp.fc2.bias", (W,)), pad(f32("mlp.norm.weight", (F,)), (0, Fp - F)),
                             pad(f32("mlp.norm.bias", (F,)), (0, Fp - F))))
            for sub in subs:
                _hand_over_fold(h, b, *sub)
    return arr


def _bert_blocks(h: _Holder, sd, prefix: str, layers: int, W: int, F: int, heads: int, new_model: bool = False, mpnet: bool = False):
    """post-LN HF encoder layers (`encoder.layer.{i}.`): BertModel / XLM-RoBERTa naming, MPNetModel naming (`mpnet`) or Alibaba-NLP NewModel naming
    (`new_model`: fused qkv_proj, (up | gate) MLP).  No LayerNorm is folded: post-LN blocks normalise behind their GEMMs."""
    hd = _head_dim(W, heads)
    arr = (L.BlockWeights * layers)()
    # checkpoint key names of the attention sub-block: (q, k, v, out-projection, LayerNorm)
    ak = ("attention.attn.q", "attention.attn.k", "attention.attn.v", "attention.attn.o", "attention.LayerNorm") if mpnet else \
         ("attention.self.query", "attention.self.key", "attention.self.value", "attention.output.dense", "attention.output.LayerNorm")
    for i in range(layers):
        p = prefix + f"encoder.layer.{i}."
        b = arr[i]
        if new_model:
            qkv_w = _need(sd, p + "attention.qkv_proj.weight", (3 * W, W)).detach().float()
            qkv_b = _need(sd, p + "attention.qkv_proj.bias", (3 * W,)).detach().float()
            b.qkv_w, b.qkv_b = h.bf16(qkv_w), h.f32(qkv_b)
            b.out_w = h.bf16(_need(sd, p + "attention.o_proj.weight", (W, W)))
            b.out_b = h.f32(_need(sd, p + "attention.o_proj.bias", (W,)))
            b.ln1_g, b.ln1_b = h.f32(_need(sd, p + "attn_ln.weight", (W,))), h.f32(_need(sd, p + "attn_ln.bias", (W,)))
            b.fc1_w = h.bf16(_need(sd, p + "mlp.up_gate_proj.weight", (2 * F, W)))      # rows [0, F) = up, [F, 2F) = gate
            b.fc1_b = h.f32(sd[p + "mlp.up_gate_proj.bias"]) if p + "mlp.up_gate_proj.bias" in sd else None
            b.fc2_w = h.bf16(_need(sd, p + "mlp.down_proj.weight", (W, F)))
            b.fc2_b = h.f32(_need(sd, p + "mlp.down_proj.bias", (W,)))
            b.ln2_g, b.ln2_b = h.f32(_need(sd, p + "mlp_ln.weight", (W,))), h.f32(_need(sd, p + "mlp_ln.bias", (W,)))
            continue
        qkv_w = torch.cat([_need(sd, p + f"{n}.weight", (W, W)).detach().float() for n in ak[:3]], 0)
        qkv_b = torch.cat([_need(sd, p + f"{n}.bias", (W,)).detach().float() for n in ak[:3]], 0)
        out_w = _need(sd, p + ak[3] + ".weight", (W, W)).detach().float()
        if hd != _kernel_head_dim(hd, heads):  # e5-small / bge-small / MiniLM: 12 heads of 32
            qkv_w, qkv_b, out_w = _pad_heads(qkv_w, qkv_b, out_w, heads, hd)
        b.qkv_w, b.qkv_b = h.bf16(qkv_w), h.f32(qkv_b)
        b.out_w = h.bf16(out_w)
        b.out_b = h.f32(_need(sd, p + ak[3] + ".bias", (W,)))
        b.ln1_g = h.f32(_need(sd, p + ak[4] + ".weight", (W,)))
        b.ln1_b = h.f32(_need(sd, p + ak[4] + ".bias", (W,)))
        b.fc1_w = h.bf16(_need(sd, p + "intermediate.dense.weight", (F, W)))
        b.fc1_b = h.f32(_need(sd, p + "intermediate.dense.bias", (F,)))
        b.fc2_w = h.bf16(_need(sd, p + "output.dense.weight", (W, F)))
        b.fc2_b = h.f32(_need(sd, p + "output.dense.bias", (W,)))
        b.ln2_g = h.f32(_need(sd, p + "output.LayerNorm.weight", (W,)))
        b.ln2_b = h.f32(_need(sd, p + "output.LayerNorm.bias", (W,)))
    return arr


def nllb_clip_state_dict(arch, sd: Dict[str, Tensor]) -> Dict[str, Tensor]:
    """The load-time transforms of the NLLB-CLIP text tower: open_clip HFTextEncoder / transformers M2M100Encoder tensors (`text.transformer.*`,
    `text.proj.weight`) -> the CLIP text tower's own names (fp32), so that everything but the ReLU runs on what exists:
      * token_embedding  = embed_tokens * sqrt(width)   (M2M100's embed_scale; row pad_id is never gathered: only un-padded rows run)
      * positional_embedding [ctx, width] = the sinusoidal table from position pos_offset on (arch.position_table(): a non-persistent buffer)
      * resblocks.N: q_proj | k_proj | v_proj packed into attn.in_proj_{weight, bias}; self_attn_layer_norm -> ln_1, final_layer_norm -> ln_2,
        fc1 / fc2 -> mlp.c_fc / mlp.c_proj; the encoder's layer_norm -> ln_final; text_projection [width, out_dim] = proj.weight^T (no bias)."""
    W, F = arch.width, arch.mlp_dim
    t = "text.transformer."
    f32 = lambda key, shape: _need(sd, key, shape).detach().to(torch.float32)
    out = {"token_embedding.weight": f32(t + "embed_tokens.weight", (arch.vocab, W)) * math.sqrt(W),
           "positional_embedding": arch.position_table(),
           "ln_final.weight": f32(t + "layer_norm.weight", (W,)), "ln_final.bias": f32(t + "layer_norm.bias", (W,)),
           "text_projection": f32("text.proj.weight", (arch.out_dim, W)).t().contiguous()}
    for i in range(arch.layers):
        p, o = f"{t}layers.{i}.", f"transformer.resblocks.{i}."
        out[o + "attn.in_proj_weight"] = torch.cat([f32(p + f"self_attn.{n}_proj.weight", (W, W)) for n in "qkv"], dim=0)
        out[o + "attn.in_proj_bias"] = torch.cat([f32(p + f"self_attn.{n}_proj.bias", (W,)) for n in "qkv"], dim=0)
        for src, dst, shape in (("self_attn.out_proj", "attn.out_proj", (W, W)), ("fc1", "mlp.c_fc", (F, W)), ("fc2", "mlp.c_proj", (W, F))):
            out[o + dst + ".weight"] = f32(p + src + ".weight", shape)
            out[o + dst + ".bias"] = f32(p + src + ".bias", shape[:1])
        for src, dst in (("self_attn_layer_norm", "ln_1"), ("final_layer_norm", "ln_2")):
            out[o + dst + ".weight"], out[o + dst + ".bias"] = f32(p + src + ".weight", (W,)), f32(p + src + ".bias", (W,))
    return out


# ---- ConvNeXt image towers (csrc/convnext.hip) ------------------------------------------------------------------------------------------------
# Load-time folds, as pure CPU-tensor functions (tests/test_convnext_host.py checks them against the unfolded fp32 computation).

def convnext_dw_taps(conv_dw_w: Tensor) -> Tensor:
    """conv_dw.weight [C, 1, 7, 7] -> fp32 [49, C] (tap-major: one tap's C channels are contiguous, as the kernel stages them)"""
    C = conv_dw_w.shape[0]
    return conv_dw_w.detach().to(torch.float32).reshape(C, 49).t().contiguous()


def convnext_fold_ln_fc1(fc1_w: Tensor, fc1_b: Tensor, ln_g: Tensor, ln_b: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    """The block's LayerNorm folded into fc1 (mq_gemm_bf16_ln): LN(x) @ W^T + b = rstd * (x @ (g*W)^T - mean * colsum) + (b + W @ beta)
    -> (bf16 g*W [4C, C], fp32 bias [4C], fp32 colsum of the ROUNDED folded weight [4C])"""
    return fold_layernorm(fc1_w, fc1_b, ln_g, ln_b)


def convnext_fold_gamma_fc2(fc2_w: Tensor, fc2_b: Tensor, gamma: Tensor) -> Tuple[Tensor, Tensor]:
    """gamma * (h @ W^T + b) = h @ (gamma[:, None] * W)^T + gamma * b  -> (fp32 weight [C, 4C], fp32 bias [C])"""
    g = gamma.detach().to(torch.float32)
    return fc2_w.detach().to(torch.float32) * g.unsqueeze(1), fc2_b.detach().to(torch.float32) * g


def convnext_downsample_weight(w: Tensor) -> Tensor:
    """downsample.1.weight [C_out, C_in, 2, 2] -> fp32 [C_out, 4 C_in] with columns in (ky, kx, c) order: the gather copies whole pixels"""
    return w.detach().to(torch.float32).permute(0, 2, 3, 1).reshape(w.shape[0], -1).contiguous()


def convnext_downsample_gather(x_nhwc: Tensor) -> Tensor:
    """the gather mq_convnext_downsample performs (without its LayerNorm), in torch: [n, H, W, C] -> [n (H/2) (W/2), 4 C], (ky, kx, c) columns"""
    n, H, W, C = x_nhwc.shape
    return x_nhwc.reshape(n, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(n * (H // 2) * (W // 2), 4 * C)


# ---- ResNet CLIP image towers (csrc/resnet.hip) -------------------------------------------------------------------------------------------------
RESNET_BN_EPS = 1e-5


resnet_pad64 = _ceil64     # channel count as the tower stores it: zero-padded to a multiple of 64 (the tiled GEMMs' k-step)


def resnet_fold_bn(conv_w: Tensor, bn_w: Tensor, bn_b: Tensor, bn_mean: Tensor, bn_var: Tensor, eps: float = RESNET_BN_EPS) -> Tuple[Tensor, Tensor]:
    """conv (no bias) followed by eval-mode BatchNorm -> one conv with a bias: w' = w * g / sqrt(var + eps) per output channel, b' = beta - mean * that"""
    s = bn_w.double() / torch.sqrt(bn_var.double() + eps)
    w = (conv_w.double() * s.view(-1, *([1] * (conv_w.dim() - 1)))).float()
    return w, (bn_b.double() - bn_mean.double() * s).float()


def resnet_conv3x3_weight(w: Tensor, cin: int, cout: int) -> Tensor:
    """[O, I, 3, 3] -> fp32 [cout, Kp]: column (ky * 3 + kx) * cin + c (mq_resnet_conv3x3), zero-padded to cin input / cout output channels and to
    Kp = 9 cin rounded up to a multiple of 64"""
    O, I = w.shape[:2]
    full = torch.zeros(cout, 3, 3, cin, dtype=torch.float32)
    full[:O, :, :, :I] = w.permute(0, 2, 3, 1).float()
    Kp = _ceil64(9 * cin)
    out = torch.zeros(cout, Kp, dtype=torch.float32)
    out[:, :9 * cin] = full.reshape(cout, 9 * cin)
    return out


def resnet_conv1x1_weight(w: Tensor, cin: int, cout: int) -> Tensor:
    """[O, I, 1, 1] -> fp32 [cout, cin], zero-padded"""
    O, I = w.shape[:2]
    out = torch.zeros(cout, cin, dtype=torch.float32)
    out[:O, :I] = w.reshape(O, I).float()
    return out


def resnet_stem_weight(w: Tensor) -> Tensor:
    """visual.conv1 [O, 3, 3, 3] -> fp32 [O, 64]: column (ky * 3 + kx) * 3 + c (mq_resnet_stem_gather's patch rows), zero past 27"""
    out = torch.zeros(w.shape[0], 64, dtype=torch.float32)
    out[:, :27] = w.permute(0, 2, 3, 1).reshape(w.shape[0], 27).float()
    return out


def resnet_pad_vec(v: Tensor, n: int) -> Tensor:
    out = torch.zeros(n, dtype=torch.float32)
    out[:v.numel()] = v.float()
    return out


def resnet_attnpool_weights(sd: Dict[str, Tensor], arch) -> Dict[str, Tensor]:
    """visual.attnpool.* -> the fp32 operands of the tower's attention pool (mq_resnet_weights): positions [T, C]; q_proj with the 64^-0.5 softmax
    scale folded into weight and bias (a power of two: the folded weight rounds to bf16 exactly as the unscaled one); k_proj and v_proj stacked into
    one [2C, C] projection; c_proj"""
    Cw, T, E, ap = 32 * arch.width, arch.tokens, arch.out_dim, "visual.attnpool."
    f32 = lambda k, shape: _need(sd, k, shape).detach().to(torch.float32)
    scale = 64 ** -0.5
    return {"pos": f32(ap + "positional_embedding", (T, Cw)),
            "q_w": f32(ap + "q_proj.weight", (Cw, Cw)) * scale, "q_b": f32(ap + "q_proj.bias", (Cw,)) * scale,
            "kv_w": torch.cat([f32(ap + "k_proj.weight", (Cw, Cw)), f32(ap + "v_proj.weight", (Cw, Cw))]),
            "kv_b": torch.cat([f32(ap + "k_proj.bias", (Cw,)), f32(ap + "v_proj.bias", (Cw,))]),
            "c_w": f32(ap + "c_proj.weight", (E, Cw)), "c_b": f32(ap + "c_proj.bias", (E,))}


def modernbert_state_dict(arch, sd: Dict[str, Tensor]) -> Dict[str, Tensor]:
    """transformers' ModernBertModel tensors (with or without a `model.` prefix; heads of task models are ignored) -> the fp32 tensors the tower
    hands to the kernels, under the checkpoint's own names.  `layers.N.mlp.Wi.weight` [2F, W] comes back with its halves SWAPPED: the module computes
    input, gate = Wi(x).chunk(2) and gelu(input) * gate, mq_glu computes up * act(gate) from (up | gate) — so the checkpoint's `gate` rows go first
    and its `input` rows (the ones GELU is applied to) second.  Layer 0 has no attn_norm (nn.Identity in the module): it is absent here too."""
    if "embeddings.tok_embeddings.weight" not in sd and "model.embeddings.tok_embeddings.weight" in sd:
        sd = {k[len("model."):]: v for k, v in sd.items() if k.startswith("model.")}
    W, F = arch.width, arch.mlp_dim
    f32 = lambda k, shape: _need(sd, k, shape).detach().to(torch.float32)
    if any(k.endswith(".bias") and (k.startswith("layers.") or k.startswith("embeddings.") or k.startswith("final_norm.")) for k in sd):
        raise ValueError("the ModernBERT tower runs bias-free blocks; this checkpoint carries bias tensors")
    out = {"embeddings.tok_embeddings.weight": f32("embeddings.tok_embeddings.weight", (arch.vocab, W)),
           "embeddings.norm.weight": f32("embeddings.norm.weight", (W,)), "final_norm.weight": f32("final_norm.weight", (W,))}
    for l in range(arch.layers):
        p = f"layers.{l}."
        if l > 0:
            out[p + "attn_norm.weight"] = f32(p + "attn_norm.weight", (W,))
        out[p + "attn.Wqkv.weight"] = f32(p + "attn.Wqkv.weight", (3 * W, W))
        out[p + "attn.Wo.weight"] = f32(p + "attn.Wo.weight", (W, W))
        out[p + "mlp_norm.weight"] = f32(p + "mlp_norm.weight", (W,))
        wi = f32(p + "mlp.Wi.weight", (2 * F, W))
        out[p + "mlp.Wi.weight"] = torch.cat([wi[F:], wi[:F]], 0)
        out[p + "mlp.Wo.weight"] = f32(p + "mlp.Wo.weight", (W, F))
    return out


def modernbert_head_tensors(sd: Dict[str, Tensor], W: int, classifier_bias: bool = False, norm_bias: bool = False):
    """(dense weight [W, W], dense bias [W] | None, norm weight [W], norm bias [W] | None, classifier weight [1, W], classifier bias [1]) of a
    ModernBertForSequenceClassification checkpoint, fp32: `head.dense.*`, `head.norm.*`, `classifier.*`.  The two optional biases are read when the
    config says they exist (classifier_bias / norm_bias); a tensor the config promises and the checkpoint lacks is an error that names it, and so is
    a bias the config denies."""
    def f32(k, shape):
        if k not in sd:
            raise ValueError(f"checkpoint is missing tensor '{k}'")
        return _need(sd, k, shape).detach().to(torch.float32)
    for flag, key, knob in ((classifier_bias, "head.dense.bias", "classifier_bias"), (norm_bias, "head.norm.bias", "norm_bias")):
        if not flag and key in sd:
            raise ValueError(f"{key} present but the config says {knob}=false")
    return (f32("head.dense.weight", (W, W)), f32("head.dense.bias", (W,)) if classifier_bias else None, f32("head.norm.weight", (W,)),
            f32("head.norm.bias", (W,)) if norm_bias else None, f32("classifier.weight", (1, W)), f32("classifier.bias", (1,)))


def qwen_state_dict(arch, sd: Dict[str, Tensor], tower: str = "Qwen") -> Dict[str, Tensor]:
    """transformers' Qwen3Model / Qwen2Model tensors (with or without a `model.` prefix; `lm_head.*` of the causal-LM classes is ignored) -> the fp32
    tensors the tower hands to the kernels.  Per layer the three projections are fused into `layers.N.self_attn.qkv.weight` [(Q + 2 KV) hd, W] = rows
    q_proj | k_proj | v_proj (and `.bias` when arch.qkv_bias), and the MLP's two input projections into `layers.N.mlp.up_gate.weight` [2F, W] = rows
    up_proj | gate_proj — mq_glu computes up * silu(gate) from (up | gate), the module down_proj(silu(gate_proj(x)) * up_proj(x)).  Everything else keeps the
    checkpoint's name.  `tower` names the family in the messages (the Mistral / Llama tower runs the same transform)."""
    if "embed_tokens.weight" not in sd and "model.embed_tokens.weight" in sd:
        sd = {k[len("model."):]: v for k, v in sd.items() if k.startswith("model.")}
    W, F, hd = arch.width, arch.mlp_dim, arch.head_dim
    A, KVW = arch.heads * hd, arch.kv_heads * hd
    f32 = lambda k, shape: _need(sd, k, shape).detach().to(torch.float32)
    out = {"embed_tokens.weight": f32("embed_tokens.weight", (arch.vocab, W)), "norm.weight": f32("norm.weight", (W,))}
    for l in range(arch.layers):
        p = f"layers.{l}."
        a = p + "self_attn."
        if not arch.qkv_bias and any((a + n + "_proj.bias") in sd for n in "qkv"):
            raise ValueError(f"{a}*_proj.bias present but the config says attention_bias=false")
        if (a + "o_proj.bias") in sd:
            raise ValueError(f"{a}o_proj.bias: the {tower} tower runs a bias-free output projection")
        out[p + "input_layernorm.weight"] = f32(p + "input_layernorm.weight", (W,))
        out[a + "qkv.weight"] = torch.cat([f32(a + "q_proj.weight", (A, W)), f32(a + "k_proj.weight", (KVW, W)), f32(a + "v_proj.weight", (KVW, W))], 0)
        if arch.qkv_bias:
            out[a + "qkv.bias"] = torch.cat([f32(a + "q_proj.bias", (A,)), f32(a + "k_proj.bias", (KVW,)), f32(a + "v_proj.bias", (KVW,))], 0)
        if arch.qk_norm:
            out[a + "q_norm.weight"] = f32(a + "q_norm.weight", (hd,))
            out[a + "k_norm.weight"] = f32(a + "k_norm.weight", (hd,))
        out[a + "o_proj.weight"] = f32(a + "o_proj.weight", (W, A))
        out[p + "post_attention_layernorm.weight"] = f32(p + "post_attention_layernorm.weight", (W,))
        out[p + "mlp.up_gate.weight"] = torch.cat([f32(p + "mlp.up_proj.weight", (F, W)), f32(p + "mlp.gate_proj.weight", (F, W))], 0)
        out[p + "mlp.down_proj.weight"] = f32(p + "mlp.down_proj.weight", (W, F))
    return out


def gemma_state_dict(arch, sd: Dict[str, Tensor]) -> Dict[str, Tensor]:
    """transformers' Gemma3TextModel tensors (with or without a `model.` prefix; `lm_head.*` is ignored) -> the fp32 tensors the tower hands to the
    kernels.  Every norm weight (the four of each block, q_norm, k_norm, the final one) comes back as 1 + w: Gemma3RMSNorm multiplies by (1 + weight), the
    kernels by their weight.  Per layer the three projections are fused into `layers.N.self_attn.qkv.weight` [(Q + 2 KV) hd, W] = rows q_proj | k_proj |
    v_proj and the MLP's two input projections into `layers.N.mlp.up_gate.weight` [2F, W] = rows up_proj | gate_proj — mq_glu_tanh computes
    up * gelu_tanh(gate) from (up | gate), the module down_proj(gelu_tanh(gate_proj(x)) * up_proj(x))."""
    if "embed_tokens.weight" not in sd and "model.embed_tokens.weight" in sd:
        sd = {k[len("model."):]: v for k, v in sd.items() if k.startswith("model.")}
    W, F, hd = arch.width, arch.mlp_dim, arch.head_dim
    A, KVW = arch.heads * hd, arch.kv_heads * hd
    f32 = lambda k, shape: _need(sd, k, shape).detach().to(torch.float32)
    norm = lambda k, shape: 1.0 + f32(k, shape)
    if any(k.endswith(".bias") and k.startswith("layers.") for k in sd):
        raise ValueError("the Gemma tower runs bias-free blocks; this checkpoint carries bias tensors")
    out = {"embed_tokens.weight": f32("embed_tokens.weight", (arch.vocab, W)), "norm.weight": norm("norm.weight", (W,))}
    for l in range(arch.layers):
        p = f"layers.{l}."
        a = p + "self_attn."
        for n in ("input_layernorm", "post_attention_layernorm", "pre_feedforward_layernorm", "post_feedforward_layernorm"):
            out[p + n + ".weight"] = norm(p + n + ".weight", (W,))
        out[a + "qkv.weight"] = torch.cat([f32(a + "q_proj.weight", (A, W)), f32(a + "k_proj.weight", (KVW, W)), f32(a + "v_proj.weight", (KVW, W))], 0)
        out[a + "q_norm.weight"] = norm(a + "q_norm.weight", (hd,))
        out[a + "k_norm.weight"] = norm(a + "k_norm.weight", (hd,))
        out[a + "o_proj.weight"] = f32(a + "o_proj.weight", (W, A))
        out[p + "mlp.up_gate.weight"] = torch.cat([f32(p + "mlp.up_proj.weight", (F, W)), f32(p + "mlp.gate_proj.weight", (F, W))], 0)
        out[p + "mlp.down_proj.weight"] = f32(p + "mlp.down_proj.weight", (W, F))
    return out


def gemma_causal_state_dict(arch, sd: Dict[str, Tensor]) -> Dict[str, Tensor]:
    """transformers' GemmaModel tensors (with or without a `model.` prefix; `lm_head.*` / `score.*` are ignored) -> the fp32 tensors the reranker tower
    hands to the kernels: qwen_state_dict's names and fusions (no q / k norm, no bias), then every norm weight as 1 + w (GemmaRMSNorm multiplies by
    1 + weight, the kernels by their weight) and the token table times sqrtf(width) — the fp32 product mq_encode_gemma forms per gathered row, formed
    once here (the same rounding).  The UNSCALED table is what a tied lm_head reads: engine/rerank.py takes its score row from `sd`, not from here."""
    if any(k.endswith(".bias") and ".layers." in "." + k for k in sd):
        raise ValueError("the Gemma reranker tower runs bias-free blocks; this checkpoint carries bias tensors")
    out = qwen_state_dict(arch, sd)
    for k in out:
        if k.endswith("layernorm.weight") or k == "norm.weight":
            out[k] = 1.0 + out[k]
    out["embed_tokens.weight"] = out["embed_tokens.weight"] * torch.tensor(float(arch.width) ** 0.5, dtype=torch.float32)
    return out


def t5_state_dict(arch, sd: Dict[str, Tensor]) -> Dict[str, Tensor]:
    """transformers' T5EncoderModel / T5Model / T5ForConditionalGeneration tensors -> the fp32 tensors the tower hands to the kernels.  The encoder's keys
    are taken with or without their `encoder.` prefix; the token table is `shared.weight`, else `encoder.embed_tokens.weight` / `embed_tokens.weight`;
    `decoder.*` and `lm_head.*` are ignored.  Per block l (`block.l.layer.0` = attention, `.layer.1` = MLP) the three projections are fused into
    `block.l.attn.qkv.weight` [3 A, W] = rows q | k | v; the ReLU MLP keeps `block.l.ff.wi.weight` [F, W]; the gated one fuses its two input projections
    into `block.l.ff.wi.weight` [2F, W] = rows wi_1 | wi_0 — mq_glu_tanh computes up * gelu_new(gate) from (up | gate), the module
    wo(gelu_new(wi_0(x)) * wi_1(x)).  `rel_bias` [heads, 2 D + 1] is arch.rel_bias_table of block 0's relative_attention_bias, the only one there is."""
    if "block.0.layer.0.SelfAttention.q.weight" not in sd and "encoder.block.0.layer.0.SelfAttention.q.weight" in sd:
        enc = {k[len("encoder."):]: v for k, v in sd.items() if k.startswith("encoder.")}
        if "shared.weight" in sd:
            enc["shared.weight"] = sd["shared.weight"]
        sd = enc
    W, F, A = arch.width, arch.mlp_dim, arch.inner
    f32 = lambda k, shape: _need(sd, k, shape).detach().to(torch.float32)
    tok = "shared.weight" if "shared.weight" in sd else "embed_tokens.weight"
    out = {"embed_tokens.weight": f32(tok, (arch.vocab, W)), "final_layer_norm.weight": f32("final_layer_norm.weight", (W,)),
           "rel_bias": arch.rel_bias_table(f32("block.0.layer.0.SelfAttention.relative_attention_bias.weight", (arch.rel_buckets, arch.heads)))}
    for l in range(arch.layers):
        a, m = f"block.{l}.layer.0.", f"block.{l}.layer.1."
        if l > 0 and (a + "SelfAttention.relative_attention_bias.weight") in sd:
            raise ValueError(f"{a}SelfAttention.relative_attention_bias.weight: a bias table per block (mt5 / umt5) is not served")
        out[f"block.{l}.attn_norm.weight"] = f32(a + "layer_norm.weight", (W,))
        out[f"block.{l}.attn.qkv.weight"] = torch.cat([f32(a + f"SelfAttention.{c}.weight", (A, W)) for c in "qkv"], 0)
        out[f"block.{l}.attn.o.weight"] = f32(a + "SelfAttention.o.weight", (W, A))
        out[f"block.{l}.ff_norm.weight"] = f32(m + "layer_norm.weight", (W,))
        if arch.gated:
            out[f"block.{l}.ff.wi.weight"] = torch.cat([f32(m + "DenseReluDense.wi_1.weight", (F, W)), f32(m + "DenseReluDense.wi_0.weight", (F, W))], 0)
        else:
            out[f"block.{l}.ff.wi.weight"] = f32(m + "DenseReluDense.wi.weight", (F, W))
        out[f"block.{l}.ff.wo.weight"] = f32(m + "DenseReluDense.wo.weight", (W, F))
    return out


def jina_bert_state_dict(arch, sd: Dict[str, Tensor]) -> Dict[str, Tensor]:
    """JinaBERT tensors (JinaBertModel, or JinaBertFor... with their `bert.` prefix) -> the fp32 tensors the tower hands to the kernels.  Per block l the
    three attention projections are fused into `layer.l.attn.qkv.weight` [3 W, W] / `.bias` [3 W] = rows query | key | value; `mlp.gated_layers.weight`
    [2F, W] holds the activated ("gated") half in rows [:F] and the linear half in rows [F:] — the module computes wo(gelu(x W[:F]^T) * x W[F:]^T) — and is
    reordered into `layer.l.mlp.up_gate.weight` = rows W[F:] | W[:F], (up | gate) as mq_glu reads it.  `type0` is row 0 of the token-type table (every
    token of a single text has type 0).  Ignored: `pooler.*`, a stray `embeddings.position_embeddings.weight`, `embeddings.position_ids`.  Refused: a
    state dict with `attention.self.layer_norm_q.*` / `layer_norm_k.*` — the qk-post-norm variants behind the -de / -es / -zh / -code checkpoints."""
    if "embeddings.word_embeddings.weight" not in sd and "bert.embeddings.word_embeddings.weight" in sd:
        sd = {k[len("bert."):]: v for k, v in sd.items() if k.startswith("bert.")}
    qk_norm = sorted(k for k in sd if ".attention.self.layer_norm_q." in k or ".attention.self.layer_norm_k." in k)
    if qk_norm:
        raise ValueError(f"'{qk_norm[0]}': the qk-post-norm JinaBERT variants (the jina-embeddings-v2-base-de / -es / -zh / -code checkpoints normalise "
                         f"query and key per head) are not served")
    W, F = arch.width, arch.mlp_dim
    f32 = lambda k, shape: _need(sd, k, shape).detach().to(torch.float32)
    out = {"word_embeddings.weight": f32("embeddings.word_embeddings.weight", (arch.vocab, W)),
           "type0": f32("embeddings.token_type_embeddings.weight", (arch.type_vocab, W))[0].contiguous(),
           "emb_ln.weight": f32("embeddings.LayerNorm.weight", (W,)), "emb_ln.bias": f32("embeddings.LayerNorm.bias", (W,))}
    for l in range(arch.layers):
        src, p = f"encoder.layer.{l}.", f"layer.{l}."
        out[p + "attn.qkv.weight"] = torch.cat([f32(src + f"attention.self.{c}.weight", (W, W)) for c in ("query", "key", "value")], 0)
        out[p + "attn.qkv.bias"] = torch.cat([f32(src + f"attention.self.{c}.bias", (W,)) for c in ("query", "key", "value")], 0)
        out[p + "attn.o.weight"] = f32(src + "attention.output.dense.weight", (W, W))
        out[p + "attn.o.bias"] = f32(src + "attention.output.dense.bias", (W,))
        out[p + "attn_ln.weight"] = f32(src + "attention.output.LayerNorm.weight", (W,))
        out[p + "attn_ln.bias"] = f32(src + "attention.output.LayerNorm.bias", (W,))
        g = f32(src + "mlp.gated_layers.weight", (2 * F, W))
        out[p + "mlp.up_gate.weight"] = torch.cat([g[F:], g[:F]], 0)
        out[p + "mlp.wo.weight"] = f32(src + "mlp.wo.weight", (W, F))
        out[p + "mlp.wo.bias"] = f32(src + "mlp.wo.bias", (W,))
        out[p + "mlp_ln.weight"] = f32(src + "mlp.layernorm.weight", (W,))
        out[p + "mlp_ln.bias"] = f32(src + "mlp.layernorm.bias", (W,))
    return out


def deberta_state_dict(arch, sd: Dict[str, Tensor]) -> Dict[str, Tensor]:
    """transformers' DebertaV2ForSequenceClassification tensors (`deberta.*` + `pooler.dense.*` + `classifier.*`) -> the fp32 tensors the tower hands to
    the kernels.  Per block l the three attention projections are fused into `layer.l.attn.qkv.weight` [3 W, W] / `.bias` [3 W] = rows query_proj |
    key_proj | value_proj.  The position tables depend on weights only and are folded here: rel = LayerNorm_encoder(encoder.rel_embeddings.weight)
    [2 S, W], and per block `layer.l.pos_key` = key_proj(rel) and `layer.l.pos_query` = query_proj(rel) when arch.share_att_key, else pos_key_proj(rel)
    / pos_query_proj(rel) — biases included, split into heads: [heads, 2 S, 64].  They are formed in float64 and stored as fp32 (the tower converts to
    bf16).  The head comes back as `pooler.weight` [W, W], `pooler.bias` [W], `classifier.weight` [1, W], `classifier.bias` [1].  Ignored:
    `lm_predictions.*`, `mask_predictions.*`, `deberta.embeddings.position_ids`."""
    W, F, S, H = arch.width, arch.mlp_dim, arch.span, arch.heads
    f32 = lambda k, shape: _need(sd, k, shape).detach().to(torch.float32)
    f64 = lambda k, shape: _need(sd, k, shape).detach().to(torch.float64)
    for k in ("deberta.embeddings.position_embeddings.weight", "deberta.embeddings.token_type_embeddings.weight", "deberta.embeddings.embed_proj.weight",
              "deberta.encoder.conv.conv.weight"):
        if k in sd:
            raise ValueError(f"'{k}' is present: the DeBERTa tower adds no position table, no type row, no embedding projection and no convolution")
    out = {"word_embeddings.weight": f32("deberta.embeddings.word_embeddings.weight", (arch.vocab, W)),
           "emb_ln.weight": f32("deberta.embeddings.LayerNorm.weight", (W,)), "emb_ln.bias": f32("deberta.embeddings.LayerNorm.bias", (W,))}
    rel = torch.nn.functional.layer_norm(f64("deberta.encoder.rel_embeddings.weight", (2 * S, W)), (W,), f64("deberta.encoder.LayerNorm.weight", (W,)),
                                         f64("deberta.encoder.LayerNorm.bias", (W,)), arch.ln_eps)
    names = ("key_proj", "query_proj") if arch.share_att_key else ("pos_key_proj", "pos_query_proj")
    for l in range(arch.layers):
        src, p = f"deberta.encoder.layer.{l}.", f"layer.{l}."
        att = src + "attention.self."
        out[p + "attn.qkv.weight"] = torch.cat([f32(att + f"{c}.weight", (W, W)) for c in ("query_proj", "key_proj", "value_proj")], 0)
        out[p + "attn.qkv.bias"] = torch.cat([f32(att + f"{c}.bias", (W,)) for c in ("query_proj", "key_proj", "value_proj")], 0)
        for dst, name in zip(("pos_key", "pos_query"), names):
            t = rel @ f64(att + name + ".weight", (W, W)).T + f64(att + name + ".bias", (W,))
            out[p + dst] = t.reshape(2 * S, H, W // H).transpose(0, 1).to(torch.float32).contiguous()
        out[p + "attn.o.weight"] = f32(src + "attention.output.dense.weight", (W, W))
        out[p + "attn.o.bias"] = f32(src + "attention.output.dense.bias", (W,))
        out[p + "attn_ln.weight"] = f32(src + "attention.output.LayerNorm.weight", (W,))
        out[p + "attn_ln.bias"] = f32(src + "attention.output.LayerNorm.bias", (W,))
        out[p + "mlp.fc1.weight"] = f32(src + "intermediate.dense.weight", (F, W))
        out[p + "mlp.fc1.bias"] = f32(src + "intermediate.dense.bias", (F,))
        out[p + "mlp.fc2.weight"] = f32(src + "output.dense.weight", (W, F))
        out[p + "mlp.fc2.bias"] = f32(src + "output.dense.bias", (W,))
        out[p + "mlp_ln.weight"] = f32(src + "output.LayerNorm.weight", (W,))
        out[p + "mlp_ln.bias"] = f32(src + "output.LayerNorm.bias", (W,))
    out["pooler.weight"], out["pooler.bias"] = f32("pooler.dense.weight", (W, W)), f32("pooler.dense.bias", (W,))
    out["classifier.weight"], out["classifier.bias"] = f32("classifier.weight", (1, W)), f32("classifier.bias", (1,))
    return out


def nomic_bert_state_dict(arch, sd: Dict[str, Tensor]) -> Dict[str, Tensor]:
    """NomicBERT tensors -> the fp32 tensors the tower hands to the kernels, from either naming (the correspondence is the "nomic_bert" entry of
    transformers' conversion_mapping.py):

      transformers' NomicBertModel            the hub's original checkpoints
      embeddings.LayerNorm                    emb_ln
      layers.l.self_attn.{q,k,v}_proj         encoder.layers.l.attn.Wqkv        [3 W, W], chunked along dim 0 into q, k, v
      layers.l.self_attn.o_proj               encoder.layers.l.attn.out_proj
      layers.l.mlp.up_proj / gate_proj        encoder.layers.l.mlp.fc11 / fc12
      layers.l.mlp.down_proj                  encoder.layers.l.mlp.fc2
      layers.l.post_attention_layernorm       encoder.layers.l.norm1
      layers.l.post_mlp_layernorm             encoder.layers.l.norm2

    (either with the task-head classes' `nomic_bert.` / `bert.` prefix).  Per block l: `layer.l.attn.qkv.weight` [3 W, W] = rows q | k | v;
    `layer.l.mlp.up_gate.weight` [2F, W] = rows up | gate, as mq_glu reads them (the module computes down(silu(gate(x)) * up(x))).  `type0` is row 0 of the
    token-type table.  Ignored: pooler, MLM-head and classifier tensors (`pooler.*`, `cls.*`, `classifier.*`), `embeddings.position_ids`, rotary
    `inv_freq` buffers.  Refused by name: a missing or mis-shaped tensor, and a bias on any Linear (the served block has none)."""
    for prefix in ("nomic_bert.", "bert."):
        if "embeddings.word_embeddings.weight" not in sd and prefix + "embeddings.word_embeddings.weight" in sd:
            sd = {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}
    hub = any(k.startswith("encoder.layers.") for k in sd) or "emb_ln.weight" in sd
    W, F = arch.width, arch.mlp_dim
    f32 = lambda k, shape: _need(sd, k, shape).detach().to(torch.float32)
    emb_ln = "emb_ln" if hub else "embeddings.LayerNorm"
    out = {"word_embeddings.weight": f32("embeddings.word_embeddings.weight", (arch.vocab, W)),
           "type0": f32("embeddings.token_type_embeddings.weight", (arch.type_vocab, W))[0].contiguous(),
           "emb_ln.weight": f32(emb_ln + ".weight", (W,)), "emb_ln.bias": f32(emb_ln + ".bias", (W,))}
    for l in range(arch.layers):
        p = f"layer.{l}."
        if hub:
            src = f"encoder.layers.{l}."
            linears = dict(qkv=src + "attn.Wqkv", o=src + "attn.out_proj", up=src + "mlp.fc11", gate=src + "mlp.fc12", down=src + "mlp.fc2")
            ln1, ln2 = src + "norm1", src + "norm2"
            out[p + "attn.qkv.weight"] = f32(linears["qkv"] + ".weight", (3 * W, W)).contiguous()
        else:
            src = f"layers.{l}."
            linears = dict(q=src + "self_attn.q_proj", k=src + "self_attn.k_proj", v=src + "self_attn.v_proj", o=src + "self_attn.o_proj",
                           up=src + "mlp.up_proj", gate=src + "mlp.gate_proj", down=src + "mlp.down_proj")
            ln1, ln2 = src + "post_attention_layernorm", src + "post_mlp_layernorm"
            out[p + "attn.qkv.weight"] = torch.cat([f32(linears[c] + ".weight", (W, W)) for c in ("q", "k", "v")], 0)
        for name in linears.values():
            if name + ".bias" in sd:
                raise ValueError(f"checkpoint tensor '{name}.bias' is unexpected: the NomicBERT block that is served has no bias on its Linears")
        out[p + "attn.o.weight"] = f32(linears["o"] + ".weight", (W, W))
        out[p + "attn_ln.weight"], out[p + "attn_ln.bias"] = f32(ln1 + ".weight", (W,)), f32(ln1 + ".bias", (W,))
        out[p + "mlp.up_gate.weight"] = torch.cat([f32(linears["up"] + ".weight", (F, W)), f32(linears["gate"] + ".weight", (F, W))], 0)
        out[p + "mlp.down.weight"] = f32(linears["down"] + ".weight", (W, F))
        out[p + "mlp_ln.weight"], out[p + "mlp_ln.bias"] = f32(ln2 + ".weight", (W,)), f32(ln2 + ".bias", (W,))
    return out

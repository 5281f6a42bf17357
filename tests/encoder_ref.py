"""Reference and rounding model of one encoder pass (csrc/towers.hip, encoder_forward_impl), for tests/test_encoder_ref_host.py and
tests/test_encoder_forms_gpu.py.  A plain helper module: nothing here calls the library, and everything runs on the device of its input.

The reference is a float64 restatement of the block formulas in the comments of towers.hip (and of oracle/towers.py, to which the host test pins
it) over a PACKED token stream [rows, W]: the sequences lie one after the other, `lens` holds their lengths.  It consumes the state dict the
engine's loaders consume (engine/tower_weights.py: _clip_blocks, _bert_blocks, _eva_blocks) and takes the operands as those loaders store them:
weight matrices rounded to bf16, biases and LayerNorm weights in fp32.  What is left between the reference and the kernels is arithmetic.

    exact(cfg, blocks, x0, lens)          rounds nothing: the float64 stream after every block
    model(cfg, blocks, x0, lens, form)    the same code, rounding to bf16 / fp32 exactly where the named form stores bf16 / fp32
    row_ratio(got, exact, model)          per row, the larger of |got - exact| / |model - exact| in the 2-norm and in the max-norm; the worst row

The model's distance from `exact` is the yardstick: the error a correct implementation of that form must make.  A kernel sums in another order
than the model and so has another rounding history of the same size; tests/test_patch_attn_gpu.py's MARGIN is the factor the project allows
between two such histories.  No row is skipped; a row whose yardstick is exactly zero is an error of the input choice (ZeroYardstick).

Where the forms round (x: the stream; h: the normalised operand; a: the attention output; f: the MLP hidden):
    pre-LN, fp32 stream     h = bf16(LN1 x)   qkv = bf16   p = bf16 (unnormalised, attention_ref)   a = bf16   x = fp32(x + out)   h = bf16(LN2 x)
                            f = bf16(act(fc1))   x = fp32(x + fc2)
    pre-LN, bf16 stream     the same with x = bf16(...)
    ... folded              no h: qkv = bf16(rstd * (x @ bf16(g * W)^T - mean * colsum) + (b + W beta)), the statistics of the bf16 rows (fold_layernorm)
    post-LN, fp32 stream    h = bf16(x)   x = fp32(x + out)   x = fp32(LN1 x), h = bf16(LN1 x)   ...   x = fp32(LN2 x), h = bf16(LN2 x)
    post-LN, rows <= 32     the same roundings (the LayerNorms ride in the skinny GEMMs' prologues; the normalised residual stays fp32)
    post-LN, bf16 stream    h = bf16(x)   h = bf16(h + out)   h = bf16(LN1 h)   h = bf16(h + fc2)   h = bf16(LN2 h), the last block x = fp32(LN2 h)
    rotary                  qkv = bf16 once more behind the rotation (in place on the bf16 buffer)
    gated MLP               (up | gate) = bf16, product = bf16 — in the GEMM's epilogue (mlp_glu = 2 on the tiled kernel) the product alone
    EVA sub-LayerNorms      a = bf16(LN a) and product = bf16(LN product), in place; folded (subln_fold): neither, the out-projection / fc2 run
                            bf16(g W) on the un-normalised bf16 rows as the folded QKV GEMM does

The e4m3 forms (Form.first8 is not None; tests/test_encoder_fp8_forms_gpu.py).  Blocks [first8, layers) run on e4m3 operands, the `mlp_extra` blocks in
front of first8 run their MLP half on them (pre-LN only), the blocks before keep the bf16 form of their stream.  The operands of an e4m3 GEMM are the
DEQUANTISED weights decode(w8) * ws[:, None] (f8_blocks), in `exact` as well: the weight quantiser is tests/test_fp8_gpu.py's, not this module's.
    h                       y = fp32(LN x);  sc = fp32(max|y| / 448) per row (1 for an all-zero row);  h = e4m3(fp32(y * fp32(1 / sc))) * sc    (rowops.hip, layernorm_fp8_kernel)
    qkv, p                  bf16, as in the bf16 forms
    a                       e4m3(fp32(o * fp32(1 / s_attn[l]))) * s_attn[l], saturating at +-448, from the fp32 quotient directly (attention_ref.budget(out_fp8=True))
    f                       e4m3(fp32(act(fc1) * fp32(1 / s_mlp[l]))) * s_mlp[l], saturating
    x, pre-LN               fp32, or bf16 on the bf16 stream
    post-LN                 x = fp32(LN ...) and h = the e4m3 rows + scales of the same LayerNorm; in front of the first e4m3 block h = rowquant(x) (no LayerNorm);
                            the stream is fp32 whatever residual_stream says (stream_post16 is a bf16-operand form)
`first8` is cut at the number of blocks of the call, and `mlp_extra` counts back from the cut value, as encoder_forward_impl does: a call of fewer
blocks than fp8_first_layer runs its LAST mlp_extra blocks' MLPs on e4m3.
Form.hist = 1 is a second rounding history of the same form: every GEMM sums fp32 partial products of 64-wide k chunks in fp32, the chunks in reverse order.
"""
import dataclasses
import math
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence

import torch

Tensor = torch.Tensor
F64 = torch.float64


class ZeroYardstick(ValueError):
    """a row of the model equals the exact reference: the input cannot measure that row"""


@dataclass
class Cfg:
    W: int
    heads: int
    F: int
    layers: int
    post_ln: bool = False
    act: str = "gelu"              # gelu | quick | relu | silu
    mask: int = 0                  # attention_ref.MASK_*
    glu: int = 0                   # 0 | 1 | 2 (the reference keeps (up | gate) un-interleaved: 2 is a storage layout)
    eps: float = 1e-5
    inv_freq: Optional[Tensor] = None       # fp32 [hd / 2]: rotate_half rotary by position in the sequence
    rope_table: Optional[Tensor] = None     # fp32 [T - rope_prefix, 2, hd] = (cos | sin), interleaved pairs (EVA02)
    rope_prefix: int = 0
    rel_bias: Optional[Tensor] = None       # [heads, 2 * span - 1]: the bias itself, entry d + span - 1 for key - query == d


@dataclass
class Form:
    name: str
    stream: str = "f32"            # "f32" | "bf16": what the residual stream is stored as
    fold: bool = False             # pre-LN: LN1 / LN2 folded into the QKV / fc1 GEMMs (bf16 stream only)
    glu_epi: bool = False          # gated MLP: the product is formed in the GEMM's epilogue, (up | gate) is never stored
    sub_fold: bool = False         # EVA: the sub-LayerNorms folded into the out-projection / fc2 GEMMs (bf16(g W) meets the un-normalised bf16 rows)
    first8: Optional[int] = None   # the first block on e4m3 operands (mq_encoder_cfg.fp8_first_layer); None: a bf16-operand form
    mlp_extra: int = 0             # blocks in front of first8 whose MLP half runs on e4m3 operands (fp8_mlp_extra)
    scales: Optional[Tensor] = None    # [layers, 2] static activation scales (attention output, MLP hidden): d_fp8_act_scale
    e4m3: bool = True              # False: the e4m3 stores switched off (tests/test_encoder_ref_host.py)
    rounds: bool = True            # False: every store switched off — the form's dataflow in float64
    hist: int = 0                  # 1: the GEMMs' sums in fp32 over reversed 64-wide k chunks (a second rounding history)


PRE_F32 = Form("pre_ln/f32")
PRE_BF16 = Form("pre_ln/bf16", stream="bf16")
PRE_BF16_FOLD = Form("pre_ln/bf16+fold", stream="bf16", fold=True)
POST_F32 = Form("post_ln/f32")
POST_SMALL = Form("post_ln_small")          # the roundings of POST_F32 (module docstring)
POST_BF16 = Form("post_ln_bf16", stream="bf16")
EVA_F32 = Form("eva/f32")
EVA_BF16_FOLD = Form("eva/bf16+fold", stream="bf16", fold=True)
EVA_BF16_FOLD_EPI = Form("eva/bf16+fold+glu_epi", stream="bf16", fold=True, glu_epi=True)
EVA_BF16_SUBFOLD = Form("eva/bf16+fold+glu_epi+subln_fold", stream="bf16", fold=True, glu_epi=True, sub_fold=True)
F8_PRE_F32 = Form("f8/pre_ln/f32", first8=0)
F8_PRE_BF16 = Form("f8/pre_ln/bf16", stream="bf16", first8=0)
F8_PRE_SPLIT = Form("f8/pre_ln/bf16+fold|split1", stream="bf16", fold=True, first8=1)
F8_PRE_SPLIT_MLP = Form("f8/pre_ln/bf16+fold|split2+mlp1", stream="bf16", fold=True, first8=2, mlp_extra=1)
F8_POST = Form("f8/post_ln", first8=0)
F8_POST_SPLIT = Form("f8/post_ln|split1", first8=1)      # (the stream stays fp32 under residual_stream = 1 as well)


# ---- operands ------------------------------------------------------------------------------------------------------------------------------

def _w16(t: Tensor) -> Tensor:
    return t.detach().float().to(torch.bfloat16).to(F64)


def _f32(t: Tensor) -> Tensor:
    return t.detach().float().to(F64)


def blocks_from_sd(kind: str, sd: Dict[str, Tensor], prefix: str, layers: int) -> List[dict]:
    """the tensors of `layers` blocks as the loaders store them (bf16-rounded matrices, fp32 vectors), in float64.  kind: "clip" (open_clip
    resblocks), "bert" (HF encoder.layer), "new_model" (fused qkv_proj, (up | gate) MLP), "eva" (timm EvaBlock).  `*_w32` keep the fp32 matrices
    the folded tensors are built from."""
    out = []
    for i in range(layers):
        b: dict = {}
        if kind == "clip":
            p = f"{prefix}resblocks.{i}."
            names = dict(ln1="ln_1", out="attn.out_proj", ln2="ln_2", fc1="mlp.c_fc", fc2="mlp.c_proj")
            qkv_w, qkv_b = sd[p + "attn.in_proj_weight"], sd[p + "attn.in_proj_bias"]
        elif kind == "bert":
            p = f"{prefix}encoder.layer.{i}."
            names = dict(ln1="attention.output.LayerNorm", out="attention.output.dense", ln2="output.LayerNorm", fc1="intermediate.dense", fc2="output.dense")
            qkv_w = torch.cat([sd[p + f"attention.self.{n}.weight"].float() for n in ("query", "key", "value")], 0)
            qkv_b = torch.cat([sd[p + f"attention.self.{n}.bias"].float() for n in ("query", "key", "value")], 0)
        elif kind == "new_model":
            p = f"{prefix}encoder.layer.{i}."
            names = dict(ln1="attn_ln", out="attention.o_proj", ln2="mlp_ln", fc1="mlp.up_gate_proj", fc2="mlp.down_proj")
            qkv_w, qkv_b = sd[p + "attention.qkv_proj.weight"], sd[p + "attention.qkv_proj.bias"]
        elif kind == "eva":
            p = f"{prefix}blocks.{i}."
            names = dict(ln1="norm1", out="attn.proj", ln2="norm2", fc1=None, fc2="mlp.fc2")
            W = sd[p + "attn.q_proj.weight"].shape[0]
            qkv_w = torch.cat([sd[p + f"attn.{n}_proj.weight"].float() for n in "qkv"], 0)
            qkv_b = torch.cat([sd[p + "attn.q_proj.bias"].float(), torch.zeros(W), sd[p + "attn.v_proj.bias"].float()])
        else:
            raise ValueError(kind)
        b["ln1_g"], b["ln1_b"] = _f32(sd[p + names["ln1"] + ".weight"]), _f32(sd[p + names["ln1"] + ".bias"])
        b["ln2_g"], b["ln2_b"] = _f32(sd[p + names["ln2"] + ".weight"]), _f32(sd[p + names["ln2"] + ".bias"])
        b["qkv_w"], b["qkv_b"], b["qkv_w32"] = _w16(qkv_w), _f32(qkv_b), _f32(qkv_w)
        b["out_w"], b["out_b"] = _w16(sd[p + names["out"] + ".weight"]), _f32(sd[p + names["out"] + ".bias"])
        b["out_w32"], b["fc2_w32"] = _f32(sd[p + names["out"] + ".weight"]), _f32(sd[p + names["fc2"] + ".weight"])
        if kind == "eva":   # (up | gate) = (fc1_x | fc1_g)
            fc1_w = torch.cat([sd[p + "mlp.fc1_x.weight"].float(), sd[p + "mlp.fc1_g.weight"].float()], 0)
            fc1_b = torch.cat([sd[p + "mlp.fc1_x.bias"].float(), sd[p + "mlp.fc1_g.bias"].float()], 0)
            for sub, key in (("attn_ln", "attn.norm"), ("mlp_ln", "mlp.norm")):
                if p + key + ".weight" in sd:
                    b[sub + "_g"], b[sub + "_b"] = _f32(sd[p + key + ".weight"]), _f32(sd[p + key + ".bias"])
        else:
            fc1_w = sd[p + names["fc1"] + ".weight"]
            fc1_b = sd.get(p + names["fc1"] + ".bias")
        b["fc1_w"], b["fc1_w32"] = _w16(fc1_w), _f32(fc1_w)
        b["fc1_b"] = _f32(fc1_b) if fc1_b is not None else None
        b["fc2_w"], b["fc2_b"] = _w16(sd[p + names["fc2"] + ".weight"]), _f32(sd[p + names["fc2"] + ".bias"])
        out.append(b)
    return out


def blocks_to(blocks: List[dict], device) -> List[dict]:
    return [{k: (v.to(device) if isinstance(v, Tensor) else v) for k, v in b.items()} for b in blocks]


# ---- the pass ------------------------------------------------------------------------------------------------------------------------------

class _Round:
    """the two stores of a form; the exact reference stores nothing"""

    def __init__(self, form: Optional[Form], mut_kind: Optional[str] = None):
        self.on = form is not None and form.rounds
        self.bf16_stream = self.on and form.stream == "bf16"
        self.e4m3 = self.on and form.e4m3
        self.truncate = mut_kind == "e4m3_truncate"
        self.saturate = mut_kind != "no_saturation"

    def _codes(self, v: Tensor) -> Tensor:       # fp32 values -> the e4m3 values they are stored as (float64)
        if not self.saturate:                    # (mutation: a conversion that does not saturate stores the NaN code for what lies above the format)
            v = torch.where(v.abs() > 464.0, torch.full_like(v, float("nan")), v)
        v = v.clamp(-448.0, 448.0)
        if not self.truncate:
            from tests.gemm_fp8_ref import rne_e4m3
            return rne_e4m3(v)
        ax = v.abs()                             # (mutation: the store drops the bits below the third mantissa bit)
        _, e = torch.frexp(ax)
        q = torch.ldexp(torch.ones_like(ax), (e - 1).clamp(min=-6) - 3)
        return torch.copysign(torch.floor(ax / q) * q, v)

    def q8(self, t: Tensor, scale) -> Tensor:    # an e4m3 store with a static scale, dequantised: what the consuming GEMM multiplies
        if not self.e4m3:
            return t
        s = float(torch.tensor(float(scale), dtype=torch.float32))
        inv = float(torch.tensor(1.0, dtype=torch.float32) / torch.tensor(s, dtype=torch.float32))
        return self._codes(self.f(self.f(t) * inv)) * s

    def rowq(self, y: Tensor):                   # e4m3 rows with a per-row scale (layernorm_fp8_kernel) -> (e4m3 values, scales [rows, 1])
        if not self.e4m3:
            return y, torch.ones(y.shape[0], 1, dtype=F64, device=y.device)
        y = self.f(y)
        mx = y.abs().amax(-1, keepdim=True)
        sc = torch.where(mx > 0, self.f(mx * float(torch.tensor(1.0 / 448.0, dtype=torch.float32))), torch.ones_like(mx))
        inv = self.f(1.0 / sc)
        return self._codes(self.f(y * inv)), sc

    def b(self, t: Tensor) -> Tensor:            # a bf16 store (from the fp32 value the kernel holds)
        return t.float().to(torch.bfloat16).to(F64) if self.on else t

    def f(self, t: Tensor) -> Tensor:            # an fp32 store
        return t.float().to(F64) if self.on else t

    def x(self, t: Tensor) -> Tensor:            # a store of the residual stream
        return self.b(t) if self.bf16_stream else self.f(t)


def _stats(x: Tensor, eps: float):
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    return mean, 1.0 / torch.sqrt(var + eps)


def _ln(x: Tensor, g: Tensor, b: Tensor, eps: float, stats=None) -> Tensor:
    mean, rstd = stats if stats is not None else _stats(x, eps)
    return (x - mean) * rstd * g + b


def _act(x: Tensor, act: str) -> Tensor:
    if act == "gelu":
        return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))
    if act == "quick":
        return x * torch.sigmoid(1.702 * x)
    if act == "relu":
        return torch.relu(x)
    if act == "silu":
        return x * torch.sigmoid(x)
    raise ValueError(act)


def _positions(lens: Sequence[int], device) -> Tensor:
    return torch.cat([torch.arange(ln, device=device) for ln in lens]) if lens else torch.zeros(0, dtype=torch.long, device=device)


def _rotary(cfg: Cfg, qkv: Tensor, lens: Sequence[int]) -> Tensor:
    """the rotations of include/marqo_hip.h (mq_encoder_cfg.d_rope_inv_freq / d_rope_table) on the Q and K thirds"""
    W, H = cfg.W, cfg.heads
    hd = W // H
    rows = qkv.shape[0]
    pos = _positions(lens, qkv.device)
    out = qkv.clone()
    for third in (0, 1):
        t = qkv[:, third * W:(third + 1) * W].reshape(rows, H, hd)
        if cfg.inv_freq is not None:      # rotate_half: (x1, x2) = (x[d], x[d + hd/2]) -> (x1 cos - x2 sin, x2 cos + x1 sin)
            ang = (pos.float()[:, None] * cfg.inv_freq.to(qkv.device).float()[None, :]).to(F64)      # the angle is an fp32 product (mq_rope)
            c, s = ang.cos()[:, None, :], ang.sin()[:, None, :]
            x1, x2 = t[..., :hd // 2], t[..., hd // 2:]
            r = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1)
        else:                             # interleaved pairs, per-element cos / sin from the table; the first rope_prefix rows of a sequence stay
            tab = cfg.rope_table.to(qkv.device).to(F64)
            idx = (pos - cfg.rope_prefix).clamp(min=0)
            c, s = tab[idx, 0][:, None, :], tab[idx, 1][:, None, :]
            rot = torch.stack([-t[..., 1::2], t[..., ::2]], -1).reshape(t.shape)
            r = torch.where((pos >= cfg.rope_prefix)[:, None, None], t * c + rot * s, t)
        out[:, third * W:(third + 1) * W] = r.reshape(rows, W)
    return out


def _attention(cfg: Cfg, qkv: Tensor, lens: Sequence[int], R: _Round, store=None) -> Tensor:
    """softmax(q k^T / sqrt(hd) [+ bias]) v per sequence and head.  Rounded as attention_ref.emulate describes the kernel: the unnormalised
    probabilities go to bf16 for the P V product, the normaliser sums them unrounded, the quotient is stored as bf16 — or by `store` (the e4m3 forms)."""
    store = store or R.b
    from tests import attention_ref as A
    W, H = cfg.W, cfg.heads
    hd = W // H
    out = torch.zeros(qkv.shape[0], W, dtype=F64, device=qkv.device)
    r0 = 0
    for ln in lens:
        if ln == 0:
            continue
        q, k, v = (t.reshape(ln, H, hd).transpose(0, 1) for t in qkv[r0:r0 + ln].split(W, dim=1))
        s = q @ k.transpose(1, 2) / math.sqrt(hd)
        if cfg.rel_bias is not None:
            span = (cfg.rel_bias.shape[1] + 1) // 2
            pos = torch.arange(ln, device=qkv.device)
            s = s + cfg.rel_bias.to(qkv.device).to(F64)[:, (pos[None, :] - pos[:, None]) + span - 1]
        s = s.masked_fill(~A.allowed(ln, cfg.mask, qkv.device), float("-inf"))
        p = torch.exp(s - s.max(-1, keepdim=True).values)
        o = (R.b(p) @ v) / p.sum(-1, keepdim=True)
        out[r0:r0 + ln] = store(o).transpose(0, 1).reshape(ln, W)
        r0 += ln
    return out


def _mm(x: Tensor, w: Tensor, hist: int = 0) -> Tensor:
    """x @ w^T; hist = 1: fp32 partial products of 64-wide k chunks, summed in fp32 from the last chunk to the first"""
    if not hist:
        return x @ w.T
    xf, wf = x.float(), w.float()
    acc = torch.zeros(x.shape[0], w.shape[0], dtype=torch.float32, device=x.device)
    for k0 in reversed(range(0, x.shape[1], 64)):
        acc = acc + xf[:, k0:k0 + 64] @ wf[:, k0:k0 + 64].T
    return acc.to(F64)


def _folded(x: Tensor, w32: Tensor, bias: Optional[Tensor], g: Tensor, beta: Tensor, eps: float, stats=None, hist: int = 0) -> Tensor:
    """engine/tower_weights.py fold_layernorm + MQ_EPI_LN_APPLY: rstd * (x @ bf16(g W)^T - mean * colsum) + (b + W beta)"""
    wf = (w32.float() * g.float()[None, :]).to(torch.bfloat16).to(F64)
    bf = ((bias.float() if bias is not None else 0) + w32.float() @ beta.float()).to(F64)
    mean, rstd = stats if stats is not None else _stats(x, eps)
    return rstd * (_mm(x, wf, hist) - mean * wf.sum(1)[None, :]) + bf


def _linear(x: Tensor, w: Tensor, b: Optional[Tensor], hist: int = 0) -> Tensor:
    y = _mm(x, w, hist)
    return y + b if b is not None else y


def _run(cfg: Cfg, blocks: List[dict], x0: Tensor, lens: Sequence[int], form: Optional[Form], layers: Optional[int] = None,
         sel: Optional[Tensor] = None, mut: Optional[dict] = None, rec: Optional[dict] = None) -> List[Tensor]:
    """the stream after every block.  `sel`: the last block updates these rows only (last_block_selected): the others keep the stream of the
    block before.  `mut`: ONE deliberate defect (tests/test_encoder_ref_host.py), {"kind": ..., "row": r}.  `rec`: filled with
    {(l, 0): max |attention output|, (l, 1): max |act(fc1)|} of every block, taken in front of the store (what d_fp8_act_amax accumulates)."""
    mut = mut or {}
    kind, mrow = mut.get("kind"), mut.get("row", 0)
    R = _Round(form, kind)
    layers = cfg.layers if layers is None else layers
    assert x0.dtype == F64 and x0.shape == (sum(lens), cfg.W)
    F = cfg.F
    hist = form.hist if form is not None else 0
    f8form = form is not None and form.first8 is not None
    first8 = min(form.first8, layers) if f8form else layers      # (cut at the call's blocks; mlp_extra counts back from the cut value)
    mlp_from = first8 - (form.mlp_extra if f8form else 0)
    assert not (f8form and cfg.post_ln and form.mlp_extra) and not (f8form and (cfg.glu or cfg.inv_freq is not None or cfg.rope_table is not None))
    post16 = cfg.post_ln and R.bf16_stream
    fold_form = form is not None and form.fold and not cfg.post_ln
    att_lens = list(lens)
    if kind == "seq_boundary":          # the first boundary lies one row late: row lens[0] is attended with the first sequence
        att_lens[0] += 1
        att_lens[1] -= 1

    def note(key, t):
        if rec is not None:
            rec[key] = max(rec.get(key, 0.0), float(t.abs().max()))

    def deq(h8):                        # the e4m3 rows as the consuming GEMM multiplies them: value times the row's scale
        v, sc = h8
        if kind == "row_scale_neighbour":
            sc = torch.roll(sc, -1, 0)
        return v * sc

    x = x0
    h = R.b(x0) if cfg.post_ln else None      # post-LN: the block input as the GEMM operand (mq_cast_bf16)
    h8 = R.rowq(x0) if (cfg.post_ln and first8 == 0) else None      # ... in front of an e4m3 block 0: mq_rowquant_fp8
    streams: List[Tensor] = []
    stale = {}
    for l in range(layers):
        b = blocks[l]
        last = l == layers - 1
        selected = sel is not None and last
        f8, mlp8 = l >= first8, l >= mlp_from
        fold, fold_mlp = fold_form and not f8, fold_form and not mlp8 and not selected      # (last_block_selected: LN2 + fc1 on the gathered rows, never folded)
        s_attn = s_mlp = None
        if f8form:
            sl = max(l - 1, 0) if kind == "prev_layer_scales" else l
            s_attn, s_mlp = form.scales[sl, 0], form.scales[sl, 1]
            if kind == "swap_scales":
                s_attn, s_mlp = s_mlp, s_attn
        if cfg.post_ln and f8 and l == first8 and l > 0:      # the bf16 block in front left bf16 rows: the first e4m3 block wants e4m3 rows + scales
            if kind == "skip_rowquant":     # h keeps the bf16 rows' bytes, read as [rows, W] e4m3 bytes; the scales were never written
                from tests.gemm_fp8_ref import decode
                raw = h.float().to(torch.bfloat16).contiguous().view(torch.uint8).reshape(-1)[: h.numel()].reshape(h.shape)
                h8 = (decode(raw), torch.ones(h.shape[0], 1, dtype=F64, device=h.device))
            else:
                h8 = R.rowq(x)
        x_in = (h if post16 else x)
        sc1 = None
        # ---- attention half
        if cfg.post_ln:
            qkv = R.b(_linear(deq(h8) if f8 else h, b["qkv_w"], b["qkv_b"], hist))
        else:
            st1 = _stats(x, cfg.eps)
            if kind == "stats0_neighbour" and l == 0:     # the first block's statistics handed in by the caller (the image tower's stats0), one row off
                st1 = (torch.roll(st1[0], -1, 0), torch.roll(st1[1], -1, 0))
            if kind == "stale_stats":
                if l == 0:
                    stale["st1"] = st1
                else:
                    m_, r_ = st1[0].clone(), st1[1].clone()
                    m_[mrow], r_[mrow] = stale["st1"][0][mrow], stale["st1"][1][mrow]
                    st1 = (m_, r_)
            if f8:
                h8 = R.rowq(_ln(x, b["ln1_g"], b["ln1_b"], cfg.eps, st1))
                sc1 = h8[1]
                qkv = R.b(_linear(deq(h8), b["qkv_w"], b["qkv_b"], hist))
            elif fold:
                qkv = R.b(_folded(x, b["qkv_w32"], b["qkv_b"], b["ln1_g"], b["ln1_b"], cfg.eps, st1, hist))
            else:
                qkv = R.b(_linear(R.b(_ln(x, b["ln1_g"], b["ln1_b"], cfg.eps, st1)), b["qkv_w"], b["qkv_b"], hist))
        if cfg.inv_freq is not None or cfg.rope_table is not None:
            qkv = R.b(_rotary(cfg, qkv, lens))

        def store_a(o, l=l, f8=f8, s_attn=s_attn):
            note((l, 0), o)
            return R.q8(o, s_attn) if f8 else R.b(o)

        a = _attention(cfg, qkv, att_lens, R, store_a)
        if kind == "gather_2wa" and selected and f8:      # the gather of the selected rows walks the e4m3 rows with a row pitch of 2 * Wa bytes
            a = a.clone()       # ... and past the middle of the buffer it reads what the workspace held: the test's sentinel byte 0xA5 = -0.203125
            far = 2 * sel >= a.shape[0]
            a[sel] = torch.where(far[:, None], torch.full_like(a[sel], -0.203125 * float(s_attn)), a[(2 * sel) % a.shape[0]])
        sub_fold = form is not None and form.sub_fold
        if "attn_ln_g" in b and sub_fold:
            proj = _folded(a, b["out_w32"], b["out_b"], b["attn_ln_g"], b["attn_ln_b"], cfg.eps, None, hist)
        else:
            if "attn_ln_g" in b:
                a = R.b(_ln(a, b["attn_ln_g"], b["attn_ln_b"], cfg.eps))
            proj = _linear(a, b["out_w"], b["out_b"], hist)
        res = x_in.clone()
        if kind == "drop_residual" and l == layers - 1:
            res[mrow] = 0
        t = R.x(res + proj)
        # ---- MLP half
        sc_ln1 = None
        if cfg.post_ln:
            n1 = _ln(t, b["ln1_g"], b["ln1_b"], cfg.eps)
            if f8:
                x1, h1_8 = R.f(n1), R.rowq(n1)
                sc_ln1 = h1_8[1]
                h1 = deq(h1_8)
            else:
                x1, h1 = (R.b(n1), R.b(n1)) if post16 else (R.f(n1), R.b(n1))
        else:
            x1 = t
            if mlp8:
                v2, sc2 = R.rowq(_ln(t, b["ln2_g"], b["ln2_b"], cfg.eps))
                if kind == "row_scale_ln1_for_ln2" and sc1 is not None:     # LN2's launch left the scales of LN1 in place
                    sc2 = sc1
                h1 = deq((v2, sc2))
            else:
                h1 = None if fold_mlp else R.b(_ln(t, b["ln2_g"], b["ln2_b"], cfg.eps))
        if kind == "ln2_neighbour" and selected and h1 is not None:
            h1 = h1.clone()
            h1[sel[mrow]] = h1[sel[(mrow + 1) % len(sel)]]
        if cfg.glu:
            ug = _folded(t, b["fc1_w32"], b["fc1_b"], b["ln2_g"], b["ln2_b"], cfg.eps, None, hist) if fold_mlp else _linear(h1, b["fc1_w"], b["fc1_b"], hist)
            if not (form is not None and form.glu_epi):
                ug = R.b(ug)
            prod = ug[:, :F] * _act(ug[:, F:], cfg.act)
            fc2_folded = "mlp_ln_g" in b and sub_fold
            if fc2_folded:
                f = R.b(prod)
            elif "mlp_ln_g" in b:
                f = R.b(_ln(R.b(prod) if (form is not None and form.glu_epi) else prod, b["mlp_ln_g"], b["mlp_ln_b"], cfg.eps))
            else:
                f = R.b(prod)
            if kind == "glu_stride":    # the product lies in the first F columns of a [rows, 2F] buffer (the gate behind it); fc2 walks it with a row stride of F
                buf = torch.cat([f, ug[:, F:]], 1).reshape(-1)
                f = buf[: f.shape[0] * F].reshape(f.shape[0], F)
        else:
            pre = _folded(t, b["fc1_w32"], b["fc1_b"], b["ln2_g"], b["ln2_b"], cfg.eps, None, hist) if fold_mlp else _linear(h1, b["fc1_w"], b["fc1_b"], hist)
            f = _act(pre, cfg.act)
            note((l, 1), f)
            f = R.q8(f, s_mlp) if mlp8 else R.b(f)
        if kind == "stale_fc1":
            if l == 0:
                stale["f"] = f
            else:
                f = f.clone()
                f[mrow] = stale["f"][mrow]
        if cfg.glu and fc2_folded:
            t2 = R.x(x1 + _folded(f, b["fc2_w32"], b["fc2_b"], b["mlp_ln_g"], b["mlp_ln_b"], cfg.eps, None, hist))
        else:
            t2 = R.x(x1 + _linear(f, b["fc2_w"], b["fc2_b"], hist))
        if cfg.post_ln:
            n2 = _ln(t2, b["ln2_g"], b["ln2_b"], cfg.eps)
            if f8:      # the LayerNorm rewrites the fp32 rows and leaves the e4m3 rows + scales for the next block
                x_new, h_new = R.f(n2), None
                v, sc = R.rowq(n2)
                h8 = (v, sc_ln1 if kind == "row_scale_ln1_for_ln2" else sc)
            elif post16:
                h_new = R.b(n2)
                x_new = R.f(n2) if last else h_new      # the last LayerNorm writes the fp32 rows
            else:
                x_new, h_new = R.f(n2), R.b(n2)
        else:
            x_new, h_new = t2, None
        if selected:
            keep = torch.ones(x.shape[0], dtype=torch.bool, device=x.device)
            keep[sel] = False
            prev = streams[-1] if streams else x0
            if kind == "scatter_all":       # the scatter writes a dense row range instead of the selected rows
                keep[int(sel.min()):int(sel.min()) + len(sel)] = False
            x_new = torch.where(keep[:, None], prev, x_new)
        x, h = x_new, h_new
        streams.append(x)
    return streams


def exact(cfg: Cfg, blocks: List[dict], x0: Tensor, lens: Sequence[int], layers: Optional[int] = None, rec: Optional[dict] = None) -> List[Tensor]:
    return _run(cfg, blocks, x0.to(F64), lens, None, layers, rec=rec)


def model(cfg: Cfg, blocks: List[dict], x0: Tensor, lens: Sequence[int], form: Form, layers: Optional[int] = None, sel: Optional[Tensor] = None,
          mut: Optional[dict] = None, rec: Optional[dict] = None) -> List[Tensor]:
    return _run(cfg, blocks, x0.to(F64), lens, form, layers, sel, mut, rec)


def row_ratio(got: Tensor, ex: Tensor, mod: Tensor, rows: Optional[Tensor] = None) -> dict:
    """for every row (or the rows given) the larger of |got - exact| / |model - exact| in the 2-norm and in the max-norm -> the worst row:
    dict(ratio, row, col (of the largest element error in that row), l2, linf).  Raises ZeroYardstick if a row of the model is exact."""
    got, ex, mod = got.to(F64), ex.to(F64), mod.to(F64)
    if rows is not None:
        got, ex, mod = got[rows], ex[rows], mod[rows]
    assert got.shape == ex.shape == mod.shape and got.dim() == 2 and got.shape[0] > 0
    e, y = got - ex, mod - ex
    y2, yi = y.norm(dim=1), y.abs().max(dim=1).values
    if not bool((y2 > 0).all()):
        bad = int((y2 == 0).nonzero()[0])
        raise ZeroYardstick(f"the model equals the exact reference in row {bad if rows is None else int(rows[bad])}: choose another input")
    e2, ei = e.norm(dim=1), e.abs().max(dim=1).values
    r = torch.maximum(e2 / y2, ei / yi)
    r = torch.where(torch.isfinite(r), r, torch.full_like(r, float("inf")))
    i = int(r.argmax())
    return dict(ratio=float(r[i]), row=i if rows is None else int(rows[i]), col=int(e[i].abs().argmax()), l2=float(e2[i] / y2[i]), linf=float(ei[i] / yi[i]))


# ---- seeded checkpoints in the loaders' naming, inputs and the cases both test files run ---------------------------------------------------

def make_sd(kind: str, layers: int, W: int, F: int, seed: int, fc1_bias: bool = True, sub_ln: bool = True, prefix: str = "t.",
            layer_gain: bool = False) -> Dict[str, Tensor]:
    """`layer_gain` (clip, bert): the V rows of block l times V_GAIN ** l, its fc1 times FC1_GAIN[kind] * V_GAIN ** l — the attention outputs and the MLP hiddens
    of the blocks, and with them the six static e4m3 scales, then lie a factor of two or more apart: a scale read from another slot is far off.  The
    out-projection and fc2 are divided by the same factors, so the blocks' updates of the stream keep their size; LN2's weight and bias times LN2_GAIN."""
    g = torch.Generator().manual_seed(seed)
    std = 0.6 / math.sqrt(W)
    sd: Dict[str, Tensor] = {}

    def lin(name, out_f, in_f, scale, bias=True):
        sd[name + ".weight"] = scale * torch.randn(out_f, in_f, generator=g)
        if bias:
            sd[name + ".bias"] = 0.02 * torch.randn(out_f, generator=g)

    def norm(name, dim):
        sd[name + ".weight"] = 1.0 + 0.1 * torch.randn(dim, generator=g)
        sd[name + ".bias"] = 0.05 * torch.randn(dim, generator=g)

    for i in range(layers):
        if kind == "clip":
            p = f"{prefix}resblocks.{i}."
            norm(p + "ln_1", W)
            sd[p + "attn.in_proj_weight"] = std * torch.randn(3 * W, W, generator=g)
            sd[p + "attn.in_proj_bias"] = 0.02 * torch.randn(3 * W, generator=g)
            lin(p + "attn.out_proj", W, W, std)
            norm(p + "ln_2", W)
            lin(p + "mlp.c_fc", F, W, std)
            lin(p + "mlp.c_proj", W, F, std / 2)
        elif kind == "bert":
            p = f"{prefix}encoder.layer.{i}."
            for n in ("query", "key", "value"):
                lin(p + "attention.self." + n, W, W, std)
            lin(p + "attention.output.dense", W, W, std)
            norm(p + "attention.output.LayerNorm", W)
            lin(p + "intermediate.dense", F, W, std)
            lin(p + "output.dense", W, F, std / 2)
            norm(p + "output.LayerNorm", W)
        elif kind == "new_model":
            p = f"{prefix}encoder.layer.{i}."
            lin(p + "attention.qkv_proj", 3 * W, W, std)
            lin(p + "attention.o_proj", W, W, std)
            norm(p + "attn_ln", W)
            lin(p + "mlp.up_gate_proj", 2 * F, W, 2 * std, bias=fc1_bias)
            lin(p + "mlp.down_proj", W, F, std / 2)
            norm(p + "mlp_ln", W)
        elif kind == "eva":
            p = f"{prefix}blocks.{i}."
            norm(p + "norm1", W)
            lin(p + "attn.q_proj", W, W, std)
            lin(p + "attn.k_proj", W, W, std, bias=False)
            lin(p + "attn.v_proj", W, W, std)
            if sub_ln:
                norm(p + "attn.norm", W)
            lin(p + "attn.proj", W, W, std)
            norm(p + "norm2", W)
            lin(p + "mlp.fc1_g", F, W, 2 * std)
            lin(p + "mlp.fc1_x", F, W, 2 * std)
            if sub_ln:
                norm(p + "mlp.norm", F)
            lin(p + "mlp.fc2", W, F, std / 2)
        else:
            raise ValueError(kind)
    # a massive activation, as trained towers have them: the first block's MLP adds OUTLIER to one channel, so the rows' (mean, rstd) of the second
    # block are far from the first block's — a block that reads stale statistics is then far off (tests/test_encoder_ref_host.py measures how far)
    if layer_gain:
        for i in range(layers):
            gv, gf = V_GAIN ** i, FC1_GAIN[kind] * V_GAIN ** i
            if kind == "clip":
                p = f"{prefix}resblocks.{i}."
                sd[p + "attn.in_proj_weight"][2 * W:] *= gv
                sd[p + "attn.in_proj_bias"][2 * W:] *= gv
                sd[p + "attn.out_proj.weight"] /= gv
                sd[p + "mlp.c_proj.weight"] /= gf
                fc1 = p + "mlp.c_fc"
            elif kind == "bert":
                p = f"{prefix}encoder.layer.{i}."
                sd[p + "attention.self.value.weight"] *= gv
                sd[p + "attention.self.value.bias"] *= gv
                sd[p + "attention.output.dense.weight"] /= gv
                sd[p + "output.dense.weight"] /= gf
                fc1 = p + "intermediate.dense"
            else:
                raise ValueError(kind)
            sd[fc1 + ".weight"] *= gf
            sd[fc1 + ".bias"] *= gf
            ln2 = p + ("ln_2" if kind == "clip" else "output.LayerNorm")      # LN2's rows twice the size of LN1's: their row scales are not interchangeable
            sd[ln2 + ".weight"] *= LN2_GAIN
            sd[ln2 + ".bias"] *= LN2_GAIN
    fc2 = dict(clip="resblocks.0.mlp.c_proj", bert="encoder.layer.0.output.dense", new_model="encoder.layer.0.mlp.down_proj", eva="blocks.0.mlp.fc2")[kind]
    sd[prefix + fc2 + ".bias"][OUTLIER_CHANNEL] += OUTLIER
    if layer_gain and kind == "bert":
        # (post-LN: the block's LayerNorm sees x + OUTLIER in every row alike — 24 units would make every row as peaked as its neighbour, and the rows' e4m3
        # scales equal; a smaller one leaves the rows' own strong channel, which make_input spreads, in charge)
        sd[prefix + fc2 + ".bias"][OUTLIER_CHANNEL] += F8_POST_OUTLIER - OUTLIER
    return sd


OUTLIER_CHANNEL, OUTLIER, F8_POST_OUTLIER = 5, 24.0, 6.0
V_GAIN, FC1_GAIN, LN2_GAIN = 64.0, dict(clip=4.0, bert=16.0), 2.0


def make_input(rows: int, W: int, seed: int, bf16: bool, spread: float = 0.0) -> Tensor:
    """fp32 [rows, W]: unit noise, one strong channel and a per-row offset (rows whose statistics differ: a LayerNorm that reads another row's
    (mean, rstd) is far off); rounded to bf16 where the caller hands a bf16 stream in, so that the reference starts from what the kernels read.
    `spread` (the e4m3 cases): the strong channel lowered by up to `spread` per row — how peaked a row is decides its largest normalised element, and
    with it the row's e4m3 scale: neighbouring rows then have scales far apart.  Lowered, not raised: with the first block's OUTLIER on top the channel
    stays below 32 in all but a few rows, as in the bf16 cases — one bf16 step of a stream value of 32 .. 64 is 0.25, more than every other channel's error
    of a row together, and whether the model and a correct kernel round such a value the same way is a coin toss the max-norm yardstick cannot referee"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, W, generator=g)
    x[:, OUTLIER_CHANNEL] += 6.0
    x += 0.75 * torch.randn(rows, 1, generator=g)
    x *= 1.0 + 0.5 * torch.rand(rows, 1, generator=g)
    if spread:
        x[:, OUTLIER_CHANNEL] -= spread * torch.rand(rows, generator=g)
    return x.to(torch.bfloat16).float() if bf16 else x


def rope_table(T: int, prefix: int, hd: int) -> Tensor:
    """[T - prefix, 2, hd] (cos | sin) of seeded angles, equal within an interleaved pair (what timm's RotaryEmbeddingCat produces)"""
    g = torch.Generator().manual_seed(77)
    ang = (torch.rand(T - prefix, hd // 2, generator=g) * 6.0).repeat_interleave(2, -1)
    return torch.stack([ang.cos(), ang.sin()], 1).contiguous()


PACKED = [1, 17, 70, 129]          # 217 rows
FIXED = [50] * 5                   # 250 rows


@dataclass
class Case:
    id: str
    kind: str                       # make_sd / blocks_from_sd kind
    form: Form
    lens: List[int]
    post_ln: bool = False
    act: str = "gelu"
    mask: int = 0
    glu: int = 0
    stream: int = 2                 # mq_encoder_cfg.residual_stream
    knobs: Dict[str, int] = field(default_factory=dict)
    rope: Optional[str] = None      # "inv_freq" | "table"
    rel_bias: bool = False
    fc1_bias: bool = True
    sub_ln: bool = True
    sel: Optional[str] = None       # "ends" (first, last and a middle row of the sequences) | "dense" (more than half of the rows)
    W: int = 128
    heads: int = 2
    F: int = 256
    layers: int = 2
    launches: Optional[tuple] = None    # (layernorm family, attention family, gather family) launches the form implies; None entries are not asserted
    seed: int = 0
    scale_div: float = 1.0          # e4m3 forms: every static scale divided by this (4: a share of the values saturates)
    q8: Optional[list] = None       # e4m3 forms: per block {name: (codes uint8 [n, k], scales fp32 [n])} as the engine quantised them (None: quantize_rows)

    @property
    def rows(self) -> int:
        return sum(self.lens)

    def eps(self) -> float:
        return 1e-6 if self.kind == "eva" else (1e-12 if self.post_ln else 1e-5)

    def sel_rows(self) -> Optional[List[int]]:
        if self.sel is None:
            return None
        if self.sel == "dense":
            return list(range(0, self.rows, 1))[: self.rows // 2 + 1]
        out, r0 = [], 0
        for ln in self.lens:        # the first and the last row of every sequence, and a row in its middle
            out += sorted({r0, r0 + ln // 2, r0 + ln - 1})
            r0 += ln
        return out

    def cfg(self) -> Cfg:
        hd = self.W // self.heads
        c = Cfg(W=self.W, heads=self.heads, F=self.F, layers=self.layers, post_ln=self.post_ln, act=self.act, mask=self.mask, glu=self.glu, eps=self.eps())
        if self.rope == "inv_freq":
            c.inv_freq = (1.0 / (10000.0 ** (torch.arange(0, hd, 2).float() / hd))).contiguous()
        if self.rope == "table":
            c.rope_table, c.rope_prefix = rope_table(self.lens[0], 1, hd), 1
        if self.rel_bias:
            span = max(self.lens)
            c.rel_bias = 0.5 * torch.randn(self.heads, 2 * span - 1, generator=torch.Generator().manual_seed(91))
        return c

    def sd(self) -> Dict[str, Tensor]:
        return make_sd(self.kind, self.layers, self.W, self.F, 100 + self.seed, self.fc1_bias, self.sub_ln, layer_gain=self.form.first8 is not None)

    def x0(self) -> Tensor:
        return make_input(self.rows, self.W, 200 + self.seed, bf16=(self.stream == 1 and not self.post_ln), spread=F8_SPREAD if self.form.first8 is not None else 0.0)


_TILED = dict(small_m_grouped=0)        # 217 / 250 rows leave the grouped skinny kernel for the tiled GEMMs (mq_gemm_small_grouped_ok false): the folds need them


def cases(small_m: int) -> List[Case]:
    """every case of tests/test_encoder_forms_gpu.py; `small_m` is the row limit of mq_gemm_small_ok as the knob getter reports it (80 unless
    the environment says otherwise).  The id names the branch and the predicate of towers.hip that sends the case there."""
    C = Case
    cs = [
        # block_pre_ln: !post_ln && !eva_form
        C("pre_ln-f32-gelu-packed217[stream_bf16=0]", "clip", PRE_F32, PACKED, launches=(4, 2, 0)),
        C("pre_ln-f32-quick-causal-fixed5x50[stream_bf16=0]", "clip", PRE_F32, FIXED, act="quick", mask=1, launches=(4, 2, 0)),
        C("pre_ln-f32-gelu-rows25[mq_gemm_small_ok(ln):LN-in-GEMM]", "clip", PRE_F32, [25], launches=(0, 2, 0)),
        C("pre_ln-f32-gelu-rows=small_m[mq_gemm_small_ok:last-inside]", "clip", PRE_F32, [small_m - 7, 7], launches=(None, 2, 0)),
        C("pre_ln-f32-gelu-rows=small_m+1[mq_gemm_small_grouped_ok:first-above-small]", "clip", PRE_F32, [small_m - 7, 8], launches=(4, 2, 0)),
        C("pre_ln-bf16-relu-packed217[residual_stream=1,ln_fold=0]", "clip", PRE_BF16, PACKED, act="relu", stream=1, knobs=dict(ln_fold=0, **_TILED), launches=(4, 2, 0)),
        C("pre_ln-bf16-gelu-packed217[grouped-skinny:fold_ok=0]", "clip", PRE_BF16, PACKED, stream=1, launches=(4, 2, 0)),
        C("pre_ln-bf16-gelu-causal-packed217[fold_ok,ln_fold=1:stats-pass]", "clip", PRE_BF16_FOLD, PACKED, mask=1, stream=1, knobs=dict(ln_fold=1, **_TILED),
          launches=(4, 2, 0)),
        C("pre_ln-bf16-gelu-fixed5x50[fold_ok,ln_fold=2,rs_finalize=0:x_has_partials]", "clip", PRE_BF16_FOLD, FIXED, stream=1,
          knobs=dict(ln_fold=2, rs_finalize=0, **_TILED), launches=(4, 2, 0)),
        C("pre_ln-bf16-quick-packed217[fold_ok,ln_fold=2,rs_finalize=1:band_ctr]", "clip", PRE_BF16_FOLD, PACKED, act="quick", stream=1,
          knobs=dict(ln_fold=2, rs_finalize=1, **_TILED), launches=(1, 2, 0)),
        # block_post_ln: post_ln && !small_post_ln && !post16
        C("post_ln-f32-gelu-packed217[post_ln,residual_stream=2]", "bert", POST_F32, PACKED, post_ln=True, launches=(5, 2, 0)),
        C("post_ln-f32-rope-glu1-bias-packed217[d_rope_inv_freq,mlp_glu=1]", "new_model", POST_F32, PACKED, post_ln=True, glu=1, rope="inv_freq",
          launches=(5, 2, 4)),
        C("post_ln-f32-rope-glu1-nobias-fixed5x50[fc1_b=NULL]", "new_model", POST_F32, FIXED, post_ln=True, glu=1, rope="inv_freq", fc1_bias=False,
          launches=(5, 2, 4)),
        C("post_ln-f32-relbias-packed217[d_rel_bias:mq_attention_bias]", "bert", POST_F32, PACKED, post_ln=True, rel_bias=True, launches=(5, 2, 0)),
        # block_post_ln_small: rows <= SMALL_LN_ROWS = 32 && mq_gemm_small_ok(..., ln)
        C("post_ln_small-rows25[rows<=SMALL_LN_ROWS]", "bert", POST_SMALL, [8, 17], post_ln=True, launches=(2, 2, 0)),
        C("post_ln_small-rows32[rows==SMALL_LN_ROWS]", "bert", POST_SMALL, [8, 17, 7], post_ln=True, launches=(2, 2, 0)),
        C("post_ln-f32-rows33[rows>SMALL_LN_ROWS:block_post_ln]", "bert", POST_F32, [8, 17, 8], post_ln=True, launches=(5, 2, 0)),
        # block_post_ln_bf16: stream_post16 && !mq_gemm_small_ok(rows, W, W)
        C("post_ln_bf16-gelu-packed217[stream_post16]", "bert", POST_BF16, PACKED, post_ln=True, stream=1, launches=(5, 2, 0)),
        C("post_ln-f32-rows33-stream1[mq_gemm_small_ok(rows,W,W):post16=0]", "bert", POST_F32, [8, 17, 8], post_ln=True, stream=1, launches=(5, 2, 0)),
        # block_eva: eva_form (mlp_glu || d_rope_table)
        C("eva-f32-glu2-rope1-subln-fixed5x50[eva_form,grouped-skinny:glu_epi=0]", "eva", EVA_F32, FIXED, act="silu", glu=2, rope="table",
          launches=(None, 2, 2)),
        C("eva-f32-glu1-rope1-nosubln-fixed5x50[mlp_glu=1:mq_glu]", "eva", EVA_F32, FIXED, act="silu", glu=1, rope="table", sub_ln=False, launches=(4, 2, 4)),
        C("eva-bf16-glu2-subln-fixed5x50[fold_ok,glu_epi,subln_fold=0]", "eva", EVA_BF16_FOLD_EPI, FIXED, act="silu", glu=2, rope="table", stream=1,
          knobs=dict(ln_fold=2, subln_fold=0, **_TILED), launches=(None, 2, 2)),
        C("eva-bf16-glu2-subln-fixed5x50[fold_attn_ln,fold_mlp_ln,subln_fold=1]", "eva", EVA_BF16_SUBFOLD, FIXED, act="silu", glu=2, rope="table", stream=1,
          knobs=dict(ln_fold=2, subln_fold=1, **_TILED), launches=(None, 2, 2)),
        # mq_encoder_forward_rows -> last_block_selected: has_sel && nsel * 2 <= rows && !mq_gemm_small_ok(rows, W, W)
        C("rows-pre_ln-f32-packed217[select_last,!post_ln]", "clip", PRE_F32, PACKED, sel="ends", launches=(3, 2, 3)),
        C("rows-pre_ln-bf16-packed217[select_last,stream_bf16]", "clip", PRE_BF16, PACKED, stream=1, sel="ends", launches=(3, 2, 3)),
        C("rows-post_ln-f32-packed217[select_last,post_ln]", "bert", POST_F32, PACKED, post_ln=True, sel="ends", launches=(5, 2, 3)),
        C("rows-post_ln_bf16-packed217[select_last,stream_post16]", "bert", POST_BF16, PACKED, post_ln=True, stream=1, sel="ends", launches=(5, 2, 3)),
        C("rows-pre_ln-f32-dense-packed217[nsel*2>rows:full-blocks]", "clip", PRE_F32, PACKED, sel="dense", launches=(4, 2, 0)),
        # one workgroup per image: attn_proj_fill_ok / panel_fill_ok (nseq * 4 >= 256 * 3) at the only width they exist for
        C("pre_ln-bf16-wide768-fixed192x16[attn_proj=1,panel_gemm=1,ln_fold=2]", "clip", PRE_BF16_FOLD, [16] * 192, stream=1,
          knobs=dict(ln_fold=2, attn_proj=1, panel_gemm=1), W=768, heads=12, F=3072, layers=1, launches=(1, 1, 0)),
    ]
    for i, c in enumerate(cs):
        c.seed = i
    return cs


# ---- the e4m3 forms ------------------------------------------------------------------------------------------------------------------------

F8_NAMES = ("qkv", "out", "fc1", "fc2")
F8_SPREAD = 28.0


def quantize_rows(w: Tensor):
    """per-row e4m3 quantisation of a bf16-valued matrix as quantize_rows_kernel (csrc/gemm_fp8.hip) writes it: (codes uint8, scales fp32).  For the host
    tests, which have no engine to read the codes back from; on the GPU the cases carry what _Fp8State quantised (Case.q8)."""
    wf = w.float()
    mx = wf.abs().amax(1)
    sc = torch.where(mx > 0, mx / 448.0, torch.ones_like(mx))
    inv = 1.0 / sc
    codes = (wf * inv[:, None]).clamp(-448.0, 448.0).cpu().to(torch.float8_e4m3fn).view(torch.uint8).to(w.device)
    return codes, sc


def quantize_blocks(blocks: List[dict]) -> List[dict]:
    return [{n: quantize_rows(b[n + "_w"]) for n in F8_NAMES} for b in blocks]


def f8_blocks(blocks: List[dict], q8: List[dict], first8: int, mlp_extra: int) -> List[dict]:
    """the operands of a call whose blocks [first8, ...) run on e4m3 weights (and the MLPs of the mlp_extra blocks in front): those matrices replaced
    by decode(w8) * ws[:, None]"""
    from tests.gemm_fp8_ref import decode
    out = []
    for l, b in enumerate(blocks):
        b = dict(b)
        names = F8_NAMES if l >= first8 else (("fc1", "fc2") if l >= first8 - mlp_extra else ())
        for n in names:
            codes, ws = q8[l][n]
            w = decode(codes.to(b[n + "_w"].device)) * ws.to(b[n + "_w"].device).to(F64)[:, None]
            assert w.shape == b[n + "_w"].shape and bool(torch.isfinite(w).all())
            b[n + "_w"] = w
        out.append(b)
    return out


def f8_cases() -> List[Case]:
    """the cases of tests/test_encoder_fp8_forms_gpu.py: 3 blocks of the shapes above; the id names what of towers.hip the case reaches"""
    C = Case
    fold = dict(ln_fold=2, **_TILED)
    cs = [
        C("f8-pre_ln-f32-gelu-packed217[block_fp8,first8=0]", "clip", F8_PRE_F32, PACKED),
        C("f8-pre_ln-bf16-quick-causal-fixed5x50[block_fp8,residual_stream=1:bf16-RMW]", "clip", F8_PRE_BF16, FIXED, act="quick", mask=1, stream=1),
        C("f8-pre_ln-bf16-gelu-packed217[first8=1,ln_fold=2,rs_finalize=0:nbk-cut]", "clip", F8_PRE_SPLIT, PACKED, stream=1, knobs=dict(rs_finalize=0, **fold)),
        C("f8-pre_ln-bf16-gelu-fixed5x50[first8=2,fp8_mlp_extra=1,ln_fold=2,rs_finalize=1]", "clip", F8_PRE_SPLIT_MLP, FIXED, stream=1,
          knobs=dict(rs_finalize=1, **fold)),
        C("f8-post_ln-gelu-packed217[first8=0:rowquant-up-front]", "bert", F8_POST, PACKED, post_ln=True),
        C("f8-post_ln-gelu-packed217[first8=1:rowquant-at-transition]", "bert", F8_POST_SPLIT, PACKED, post_ln=True),
        C("f8-post_ln-gelu-fixed5x50[first8=1,residual_stream=1:post16=0]", "bert", F8_POST_SPLIT, FIXED, post_ln=True, stream=1),
        C("f8-pre_ln-f32-gelu-packed217[scales/4:saturating]", "clip", F8_PRE_F32, PACKED, scale_div=4.0),
        # mq_encoder_forward_rows -> the e4m3 body of last_block_selected
        C("f8-rows-pre_ln-f32-packed217[select_last,f8]", "clip", F8_PRE_F32, PACKED, sel="ends"),
        C("f8-rows-pre_ln-bf16-packed217[select_last,f8,stream_bf16]", "clip", F8_PRE_BF16, PACKED, stream=1, sel="ends"),
        # ... and the selections that must NOT take it
        C("f8-rows-post_ln-packed217[post_ln:select_last=0]", "bert", F8_POST, PACKED, post_ln=True, sel="ends"),
    ]
    for i, c in enumerate(cs):
        c.seed, c.layers = 40 + i, 3
    return cs


def f8_setup(case: Case, device="cpu", layers: Optional[int] = None) -> dict:
    """operands, scales and form of an e4m3 case for a call of `layers` blocks.  The static scales come from the float64 reference of the FULL call,
    never from the code under test: s[l, k] = max |exact tensor| / 448 (the rule of engine/towers.py _Fp8State.fold at margin 1), divided by
    case.scale_div.  -> dict(cfg, blocks, x0, form, scales fp32 [layers, 2], amax_exact {(l, k): max})"""
    cfg = case.cfg()
    n = case.layers if layers is None else layers
    base = blocks_to(blocks_from_sd(case.kind, case.sd(), "t.", case.layers), device)
    q8 = case.q8 if case.q8 is not None else quantize_blocks(base)
    x0 = case.x0().to(device).to(F64)
    full = f8_blocks(base, q8, min(case.form.first8, case.layers), case.form.mlp_extra)
    rec: dict = {}
    exact(cfg, full, x0, case.lens, case.layers, rec)
    scales = torch.tensor([[rec[(l, 0)] / 448.0, rec[(l, 1)] / 448.0] for l in range(case.layers)], dtype=torch.float32) / case.scale_div
    blocks = full if n == case.layers else f8_blocks(base, q8, min(case.form.first8, n), case.form.mlp_extra)
    return dict(cfg=cfg, blocks=blocks, x0=x0, form=dataclasses.replace(case.form, scales=scales), scales=scales, amax_exact=rec)


def reference(case: Case, device="cpu", layers: Optional[int] = None):
    """(exact stream, model stream) after `layers` blocks (default: all) on `device`; with a row selection the model's last block updates the
    selected rows only (an e4m3 form on the post-LN blocks never selects: encoder_forward_impl's select_last)"""
    if case.form.first8 is not None:
        n = case.layers if layers is None else layers
        s = f8_setup(case, device, n)
        sel = case.sel_rows()
        selected = sel is not None and len(sel) * 2 <= case.rows and n == case.layers and not case.post_ln
        ex = exact(s["cfg"], s["blocks"], s["x0"], case.lens, n)[-1]
        mo = model(s["cfg"], s["blocks"], s["x0"], case.lens, s["form"], n, torch.tensor(sel, device=device) if selected else None)[-1]
        return ex, mo
    cfg = case.cfg()
    n = case.layers if layers is None else layers
    blocks = blocks_to(blocks_from_sd(case.kind, case.sd(), "t.", case.layers), device)
    x0 = case.x0().to(device).to(F64)
    sel = case.sel_rows()
    selected = sel is not None and len(sel) * 2 <= case.rows and n == case.layers
    ex = exact(cfg, blocks, x0, case.lens, n)[-1]
    mo = model(cfg, blocks, x0, case.lens, case.form, n, torch.tensor(sel, device=device) if selected else None)[-1]
    return ex, mo

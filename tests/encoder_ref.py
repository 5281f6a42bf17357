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
"""
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

    def __init__(self, form: Optional[Form]):
        self.on = form is not None
        self.bf16_stream = self.on and form.stream == "bf16"

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


def _attention(cfg: Cfg, qkv: Tensor, lens: Sequence[int], R: _Round) -> Tensor:
    """softmax(q k^T / sqrt(hd) [+ bias]) v per sequence and head.  Rounded as attention_ref.emulate describes the kernel: the unnormalised
    probabilities go to bf16 for the P V product, the normaliser sums them unrounded, the quotient is stored as bf16."""
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
        out[r0:r0 + ln] = R.b(o).transpose(0, 1).reshape(ln, W)
        r0 += ln
    return out


def _folded(x: Tensor, w32: Tensor, bias: Optional[Tensor], g: Tensor, beta: Tensor, eps: float, stats=None) -> Tensor:
    """engine/tower_weights.py fold_layernorm + MQ_EPI_LN_APPLY: rstd * (x @ bf16(g W)^T - mean * colsum) + (b + W beta)"""
    wf = (w32.float() * g.float()[None, :]).to(torch.bfloat16).to(F64)
    bf = ((bias.float() if bias is not None else 0) + w32.float() @ beta.float()).to(F64)
    mean, rstd = stats if stats is not None else _stats(x, eps)
    return rstd * (x @ wf.T - mean * wf.sum(1)[None, :]) + bf


def _linear(x: Tensor, w: Tensor, b: Optional[Tensor]) -> Tensor:
    y = x @ w.T
    return y + b if b is not None else y


def _run(cfg: Cfg, blocks: List[dict], x0: Tensor, lens: Sequence[int], form: Optional[Form], layers: Optional[int] = None,
         sel: Optional[Tensor] = None, mut: Optional[dict] = None) -> List[Tensor]:
    """the stream after every block.  `sel`: the last block updates these rows only (last_block_selected): the others keep the stream of the
    block before.  `mut`: ONE deliberate defect (tests/test_encoder_ref_host.py), {"kind": ..., "row": r}."""
    R = _Round(form)
    mut = mut or {}
    kind, mrow = mut.get("kind"), mut.get("row", 0)
    layers = cfg.layers if layers is None else layers
    assert x0.dtype == F64 and x0.shape == (sum(lens), cfg.W)
    F = cfg.F
    post16 = cfg.post_ln and R.bf16_stream
    fold = form is not None and form.fold and not cfg.post_ln
    att_lens = list(lens)
    if kind == "seq_boundary":          # the first boundary lies one row late: row lens[0] is attended with the first sequence
        att_lens[0] += 1
        att_lens[1] -= 1
    x = x0
    h = R.b(x0) if cfg.post_ln else None      # post-LN: the block input as the GEMM operand (mq_cast_bf16)
    streams: List[Tensor] = []
    stale = {}
    for l in range(layers):
        b = blocks[l]
        last = l == layers - 1
        selected = sel is not None and last
        x_in = (h if post16 else x)
        # ---- attention half
        if cfg.post_ln:
            qkv = R.b(_linear(h, b["qkv_w"], b["qkv_b"]))
        else:
            st1 = _stats(x, cfg.eps)
            if kind == "stale_stats":
                if l == 0:
                    stale["st1"] = st1
                else:
                    m_, r_ = st1[0].clone(), st1[1].clone()
                    m_[mrow], r_[mrow] = stale["st1"][0][mrow], stale["st1"][1][mrow]
                    st1 = (m_, r_)
            if fold:
                qkv = R.b(_folded(x, b["qkv_w32"], b["qkv_b"], b["ln1_g"], b["ln1_b"], cfg.eps, st1))
            else:
                qkv = R.b(_linear(R.b(_ln(x, b["ln1_g"], b["ln1_b"], cfg.eps, st1)), b["qkv_w"], b["qkv_b"]))
        if cfg.inv_freq is not None or cfg.rope_table is not None:
            qkv = R.b(_rotary(cfg, qkv, lens))
        a = _attention(cfg, qkv, att_lens, R)
        sub_fold = form is not None and form.sub_fold
        if "attn_ln_g" in b and sub_fold:
            proj = _folded(a, b["out_w32"], b["out_b"], b["attn_ln_g"], b["attn_ln_b"], cfg.eps)
        else:
            if "attn_ln_g" in b:
                a = R.b(_ln(a, b["attn_ln_g"], b["attn_ln_b"], cfg.eps))
            proj = _linear(a, b["out_w"], b["out_b"])
        res = x_in.clone()
        if kind == "drop_residual" and l == layers - 1:
            res[mrow] = 0
        t = R.x(res + proj)
        # ---- MLP half
        if cfg.post_ln:
            n1 = _ln(t, b["ln1_g"], b["ln1_b"], cfg.eps)
            x1, h1 = (R.b(n1), R.b(n1)) if post16 else (R.f(n1), R.b(n1))
        else:
            x1 = t
            h1 = None if fold else R.b(_ln(t, b["ln2_g"], b["ln2_b"], cfg.eps))
        if kind == "ln2_neighbour" and selected and h1 is not None:
            h1 = h1.clone()
            h1[sel[mrow]] = h1[sel[(mrow + 1) % len(sel)]]
        if cfg.glu:
            ug = _folded(t, b["fc1_w32"], b["fc1_b"], b["ln2_g"], b["ln2_b"], cfg.eps) if fold else _linear(h1, b["fc1_w"], b["fc1_b"])
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
            pre = _folded(t, b["fc1_w32"], b["fc1_b"], b["ln2_g"], b["ln2_b"], cfg.eps) if fold else _linear(h1, b["fc1_w"], b["fc1_b"])
            f = R.b(_act(pre, cfg.act))
        if kind == "stale_fc1":
            if l == 0:
                stale["f"] = f
            else:
                f = f.clone()
                f[mrow] = stale["f"][mrow]
        if cfg.glu and fc2_folded:
            t2 = R.x(x1 + _folded(f, b["fc2_w32"], b["fc2_b"], b["mlp_ln_g"], b["mlp_ln_b"], cfg.eps))
        else:
            t2 = R.x(x1 + _linear(f, b["fc2_w"], b["fc2_b"]))
        if cfg.post_ln:
            n2 = _ln(t2, b["ln2_g"], b["ln2_b"], cfg.eps)
            if post16:
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


def exact(cfg: Cfg, blocks: List[dict], x0: Tensor, lens: Sequence[int], layers: Optional[int] = None) -> List[Tensor]:
    return _run(cfg, blocks, x0.to(F64), lens, None, layers)


def model(cfg: Cfg, blocks: List[dict], x0: Tensor, lens: Sequence[int], form: Form, layers: Optional[int] = None, sel: Optional[Tensor] = None,
          mut: Optional[dict] = None) -> List[Tensor]:
    return _run(cfg, blocks, x0.to(F64), lens, form, layers, sel, mut)


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

def make_sd(kind: str, layers: int, W: int, F: int, seed: int, fc1_bias: bool = True, sub_ln: bool = True, prefix: str = "t.") -> Dict[str, Tensor]:
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
    fc2 = dict(clip="resblocks.0.mlp.c_proj", bert="encoder.layer.0.output.dense", new_model="encoder.layer.0.mlp.down_proj", eva="blocks.0.mlp.fc2")[kind]
    sd[prefix + fc2 + ".bias"][OUTLIER_CHANNEL] += OUTLIER
    return sd


OUTLIER_CHANNEL, OUTLIER = 5, 24.0


def make_input(rows: int, W: int, seed: int, bf16: bool) -> Tensor:
    """fp32 [rows, W]: unit noise, one strong channel and a per-row offset (rows whose statistics differ: a LayerNorm that reads another row's
    (mean, rstd) is far off); rounded to bf16 where the caller hands a bf16 stream in, so that the reference starts from what the kernels read"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, W, generator=g)
    x[:, OUTLIER_CHANNEL] += 6.0
    x += 0.75 * torch.randn(rows, 1, generator=g)
    x *= 1.0 + 0.5 * torch.rand(rows, 1, generator=g)
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
        return make_sd(self.kind, self.layers, self.W, self.F, 100 + self.seed, self.fc1_bias, self.sub_ln)

    def x0(self) -> Tensor:
        return make_input(self.rows, self.W, 200 + self.seed, bf16=(self.stream == 1 and not self.post_ln))


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


def reference(case: Case, device="cpu", layers: Optional[int] = None):
    """(exact stream, model stream) after `layers` blocks (default: all) on `device`; with a row selection the model's last block updates the
    selected rows only"""
    cfg = case.cfg()
    n = case.layers if layers is None else layers
    blocks = blocks_to(blocks_from_sd(case.kind, case.sd(), "t.", case.layers), device)
    x0 = case.x0().to(device).to(F64)
    sel = case.sel_rows()
    selected = sel is not None and len(sel) * 2 <= case.rows and n == case.layers
    ex = exact(cfg, blocks, x0, case.lens, n)[-1]
    mo = model(cfg, blocks, x0, case.lens, case.form, n, torch.tensor(sel, device=device) if selected else None)[-1]
    return ex, mo

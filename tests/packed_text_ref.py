"""Reference and rounding model of one pass of the three packed-token text towers — csrc/modernbert.hip (mq_encode_modernbert), csrc/qwen.hip
(mq_encode_qwen), csrc/gemma.hip (mq_encode_gemma) — for tests/test_packed_text_ref_host.py and tests/test_packed_text_forms_gpu.py.  A plain helper
module in the manner of tests/encoder_ref.py: nothing here calls the native library, and everything runs on the device of `ids`.  Of the engine's Python
only build() is used — it runs the loaders of engine/tower_weights.py, whose tensors are the operands — and the arch's own inv_freq().

The reference is a float64 restatement of the block formulas in the header comments of the three .hip files over a PACKED token stream [rows, W]: the
sequences lie one after the other, `lens` holds their lengths, `ids` [rows] the token ids.  It consumes the tensors the engine's loaders produce
(engine/tower_weights.py: modernbert_state_dict, qwen_state_dict, gemma_state_dict) as the towers store them: weight matrices rounded to bf16, norm
weights, the token table and Qwen2's QKV bias in fp32, Gemma's 1 + w already folded, ModernBERT's Wi halves already swapped, the fused QKV and
(up | gate) matrices.  What is left between the reference and the kernels is arithmetic.

    exact(family, arch, tensors, ids, lens, layers=None)     rounds nothing -> Pass: the float64 stream after every block, after the final norm, the pooled rows
    model(family, arch, tensors, ids, lens, layers=None, mut=None, hist=0)     the same code, rounding to bf16 / fp32 exactly where the tower stores bf16 / fp32
    row_ratio, ZeroYardstick     tests/encoder_ref.py's, re-exported: the yardstick is the model's distance from `exact`, per row

Where `model` rounds (x: the stream; h: the normalised operand; a: the attention output; o: Gemma's sub-layer output):
    x = fp32 (the token row; ModernBERT: fp32(LN tok), h = bf16(LN tok); Gemma: fp32(tok * fp32(sqrt W)))
    h = bf16(norm x)      qkv = bf16(h Wqkv^T (+ b))      (q | k) = bf16 once more behind the rotation / qk_norm_rope, in place (ONE rounding behind norm and rotation)
    p = bf16, un-normalised, for the P V product; the normaliser sums the unrounded p (tests/attention_ref.py)      a = bf16
    ModernBERT, Qwen:  x = fp32(x + a Wo^T) — the GEMM epilogue's fp32 accumulator plus residual, rounded once
    Gemma:  o = bf16(a Wo^T) ; x = fp32(x + norm(o)) ; h = bf16(norm x) from the fp32 x
    (up | gate) = bf16 ; product = bf16 ; the MLP's output enters x as the attention's does
    the final norm = fp32, in place ; Qwen under last-token pooling: the final norm of the pooled rows only, fp32
    pooling: mean = fp32(sum / len), cls / last = the row ; L2 = fp32(row / |row|)
Activations: ModernBERT erf-GELU, Qwen SiLU, Gemma tanh-GELU in the kernel's form x / (1 + exp(-2u)).  The rotary angle is float64 from the fp32 inverse
frequencies (tests/test_qwen_gpu.py::_qk_reference): the kernels' fp32 product position * inv_freq is part of what is measured.
hist = 1 is a second rounding history: every GEMM sums fp32 partial products of 64-wide k chunks in fp32, the chunks in reverse order (encoder_ref._mm).

Mutants (`mut=`, ONE deliberate defect of the host orchestration each; MUTANTS):
    local_gets_global / global_gets_local     the sliding layers take the global inverse frequencies / the full layers the local ones
    window_plus1 / window_minus1              half_window + 1 / - 1 on the sliding layers
    pattern_shift                             layer l takes the kind (sliding / full: band and frequencies) of layer l - 1, cyclically
    layer0_attn_norm                          ModernBERT: layer 0 normalises x once more (with layer 1's attn_norm weight) instead of taking the embedding's h
    next_norm_same_block                      Gemma: the h a block leaves for the next one is normalised with its OWN input_layernorm weight, not block l + 1's
    no_embed_scale                            Gemma: the token rows enter the stream without the factor sqrt(W)
    no_qkv_bias                               Qwen2: the QKV GEMM runs without its bias
    last_row_minus1                           Qwen, last-token pooling: the final norm gathers row len - 2 (row 0 of a one-token sequence)
    eps_x10                                   every norm's eps times ten
    stale_row                                 one token row (row // 2 of the batch) of the last block keeps the previous block's value
"""
import math
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence

import torch

from tests import encoder_ref as E
from tests.encoder_ref import ZeroYardstick, row_ratio      # noqa: F401  (the two test files take them from here)

Tensor = torch.Tensor
F64 = torch.float64
FAMILIES = ("modernbert", "qwen", "gemma")
MUTANTS = ("local_gets_global", "global_gets_local", "window_plus1", "window_minus1", "pattern_shift", "layer0_attn_norm", "next_norm_same_block",
           "no_embed_scale", "no_qkv_bias", "last_row_minus1", "eps_x10", "stale_row")
_FORM = E.Form("packed_text")        # the fp32 stream; every store of these towers is a plain bf16 or fp32 one


@dataclass
class Pass:
    blocks: List[Tensor]                 # the stream after every block, [rows, W] float64
    final: Tensor                        # ... after the final norm over every row
    pooled: Dict[tuple, Tensor] = field(default_factory=dict)       # (pool, normalize) -> [nseq, W]; pool in mean / cls / last


def operands(family: str, tensors: Dict[str, Tensor], device) -> Dict[str, Tensor]:
    """the loaders' fp32 tensors as the towers store them, in float64: matrices to bf16 (all but the token table), everything else fp32"""
    out = {}
    for k, v in tensors.items():
        is_matrix = v.dim() == 2 and "tok_embeddings" not in k and "embed_tokens" not in k
        out[k] = (E._w16(v) if is_matrix else E._f32(v)).to(device)
    return out


# ---- the row operations ---------------------------------------------------------------------------------------------------------------------------------

def _rms(x: Tensor, g: Tensor, eps: float) -> Tensor:
    return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * g


def _gelu_tanh(x: Tensor) -> Tensor:      # csrc/gemma.hip: x / (1 + exp(-2u)), u = sqrt(2 / pi) (x + 0.044715 x^3)
    u = math.sqrt(2.0 / math.pi) * (x * (1.0 + 0.044715 * (x * x)))
    return x / (1.0 + torch.exp(-2.0 * u))


def _rope(t: Tensor, pos: Tensor, inv_freq: Tensor) -> Tensor:
    """rotate_half on [rows, heads, hd]: (x1, x2) = (x[d], x[d + hd / 2]) -> (x1 cos - x2 sin, x2 cos + x1 sin), the angle in float64 from the fp32 frequencies"""
    hd = t.shape[-1]
    ang = pos.to(F64)[:, None] * inv_freq.to(F64)[None, :]
    c, s = ang.cos()[:, None, :], ang.sin()[:, None, :]
    x1, x2 = t[..., :hd // 2], t[..., hd // 2:]
    return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1)


def _qk_step(qkv: Tensor, pos: Tensor, Q: int, KV: int, hd: int, inv_freq: Tensor, R, q_g=None, k_g=None, eps: float = 0.0) -> Tensor:
    """mq_rope / mq_qk_norm_rope: the per-head RMSNorm (when given) and the rotation of the q and k parts, one store; v stays"""
    rows = qkv.shape[0]
    out = qkv.clone()
    for lo, n, g in ((0, Q, q_g), (Q * hd, KV, k_g)):
        t = qkv[:, lo:lo + n * hd].reshape(rows, n, hd)
        if g is not None:
            t = _rms(t, g, eps)
        out[:, lo:lo + n * hd] = R.b(_rope(t, pos, inv_freq)).reshape(rows, n * hd)
    return out


def _attention(qkv: Tensor, lens: Sequence[int], Q: int, KV: int, hd: int, scale: float, causal: bool, hw: int, R) -> Tensor:
    """softmax(q k^T scale) v per sequence and query head; query head h reads K/V head h // (Q / KV); hw > 0: keys within hw positions only.  Rounded as
    tests/attention_ref.py describes the kernels: bf16 un-normalised probabilities for P V, the normaliser from the unrounded ones, the quotient to bf16."""
    dev = qkv.device
    out = torch.zeros(qkv.shape[0], Q * hd, dtype=F64, device=dev)
    kvh = torch.arange(Q, device=dev) // (Q // KV)
    r0 = 0
    for ln in lens:
        blk = qkv[r0:r0 + ln]
        q = blk[:, :Q * hd].reshape(ln, Q, hd).transpose(0, 1)
        k = blk[:, Q * hd:(Q + KV) * hd].reshape(ln, KV, hd).transpose(0, 1)[kvh]
        v = blk[:, (Q + KV) * hd:].reshape(ln, KV, hd).transpose(0, 1)[kvh]
        i = torch.arange(ln, device=dev)
        ok = (i[None, :] <= i[:, None]) if causal else torch.ones(ln, ln, dtype=torch.bool, device=dev)
        if hw > 0:
            ok = ok & ((i[:, None] - i[None, :]).abs() <= hw)
        s = (q @ k.transpose(1, 2) * scale).masked_fill(~ok, float("-inf"))
        p = torch.exp(s - s.max(-1, keepdim=True).values)
        o = (R.b(p) @ v) / p.sum(-1, keepdim=True)
        out[r0:r0 + ln] = R.b(o).transpose(0, 1).reshape(ln, Q * hd)
        r0 += ln
    return out


def _kinds(arch, layers: int, kind: Optional[str]):
    """per layer (sliding?, local frequencies?, half_window) under the mutant `kind`"""
    sliding = list(getattr(arch, "sliding", ())) or [False] * arch.layers
    if kind == "pattern_shift":
        sliding = [sliding[(l - 1) % len(sliding)] for l in range(len(sliding))]
    hw = getattr(arch, "half_window", 0) + (1 if kind == "window_plus1" else -1 if kind == "window_minus1" else 0)
    out = []
    for l in range(layers):
        local = sliding[l]
        if (kind == "local_gets_global" and sliding[l]) or (kind == "global_gets_local" and not sliding[l]):
            local = not local
        out.append((sliding[l], local, hw if sliding[l] else 0))
    return out


# ---- the pass -------------------------------------------------------------------------------------------------------------------------------------------

def _run(family: str, arch, tensors: Dict[str, Tensor], ids: Tensor, lens: Sequence[int], rounds: bool, layers: Optional[int], mut: Optional[str],
         hist: int) -> Pass:
    assert family in FAMILIES and (mut is None or mut in MUTANTS)
    dev = ids.device
    lens = [int(n) for n in lens]
    assert ids.dim() == 1 and ids.shape[0] == sum(lens) and min(lens) >= 1
    layers = arch.layers if layers is None else layers
    t = operands(family, tensors, dev)
    R = E._Round(_FORM if rounds else None)
    hist = hist if rounds else 0
    mm = lambda x, w: E._mm(x, w, hist)
    W, F = arch.width, arch.mlp_dim
    pos = E._positions(lens, dev)
    ids = ids.long()
    eps = (arch.ln_eps if family == "modernbert" else arch.rms_eps) * (10.0 if mut == "eps_x10" else 1.0)
    kinds = _kinds(arch, layers, mut)
    streams: List[Tensor] = []

    if family == "modernbert":
        H, hd = arch.heads, 64
        Q = KV = H
        ln = lambda x, g: E._ln(x, g, 0.0, eps)
        freq = {loc: arch.inv_freq(local=loc).to(dev) for loc in (False, True)}
        e = ln(t["embeddings.tok_embeddings.weight"][ids], t["embeddings.norm.weight"])
        x, h = R.f(e), R.b(e)
        for l in range(layers):
            p = f"layers.{l}."
            _, local, hw = kinds[l]
            if l > 0:
                h = R.b(ln(x, t[p + "attn_norm.weight"]))
            elif mut == "layer0_attn_norm":
                h = R.b(ln(x, t["layers.1.attn_norm.weight"]))
            qkv = R.b(mm(h, t[p + "attn.Wqkv.weight"]))
            qkv = _qk_step(qkv, pos, Q, KV, hd, freq[local], R)
            a = _attention(qkv, lens, Q, KV, hd, 1.0 / math.sqrt(hd), False, hw, R)
            x = R.f(x + mm(a, t[p + "attn.Wo.weight"]))
            ug = R.b(mm(R.b(ln(x, t[p + "mlp_norm.weight"])), t[p + "mlp.Wi.weight"]))
            x = R.f(x + mm(R.b(ug[:, :F] * E._act(ug[:, F:], "gelu")), t[p + "mlp.Wo.weight"]))
            streams.append(x)
        final_g, norm = t["final_norm.weight"], ln
    elif family == "qwen":
        Q, KV, hd = arch.heads, arch.kv_heads, arch.head_dim
        norm = lambda x, g: _rms(x, g, eps)
        freq = arch.inv_freq().to(dev)
        x = R.f(t["embed_tokens.weight"][ids])
        for l in range(layers):
            p = f"layers.{l}."
            a_ = p + "self_attn."
            qkv = mm(R.b(norm(x, t[p + "input_layernorm.weight"])), t[a_ + "qkv.weight"])
            if arch.qkv_bias and mut != "no_qkv_bias":
                qkv = qkv + t[a_ + "qkv.bias"]
            qkv = R.b(qkv)
            qg, kg = (t[a_ + "q_norm.weight"], t[a_ + "k_norm.weight"]) if arch.qk_norm else (None, None)
            qkv = _qk_step(qkv, pos, Q, KV, hd, freq, R, qg, kg, eps)
            a = _attention(qkv, lens, Q, KV, hd, 1.0 / math.sqrt(hd), True, 0, R)
            x = R.f(x + mm(a, t[a_ + "o_proj.weight"]))
            ug = R.b(mm(R.b(norm(x, t[p + "post_attention_layernorm.weight"])), t[p + "mlp.up_gate.weight"]))
            x = R.f(x + mm(R.b(ug[:, :F] * E._act(ug[:, F:], "silu")), t[p + "mlp.down_proj.weight"]))
            streams.append(x)
        final_g = t["norm.weight"]
    else:
        Q, KV, hd = arch.heads, arch.kv_heads, arch.head_dim
        norm = lambda x, g: _rms(x, g, eps)
        freq = {loc: arch.inv_freq(local=loc).to(dev) for loc in (False, True)}
        scale = 1.0 if mut == "no_embed_scale" else float(torch.tensor(float(W), dtype=torch.float32).sqrt())     # sqrtf((float)W)
        x = R.f(t["embed_tokens.weight"][ids] * scale)
        h = R.b(norm(x, t["layers.0.input_layernorm.weight"]))
        for l in range(layers):
            p = f"layers.{l}."
            a_ = p + "self_attn."
            _, local, hw = kinds[l]
            qkv = R.b(mm(h, t[a_ + "qkv.weight"]))
            qkv = _qk_step(qkv, pos, Q, KV, hd, freq[local], R, t[a_ + "q_norm.weight"], t[a_ + "k_norm.weight"], eps)
            a = _attention(qkv, lens, Q, KV, hd, arch.attn_scale, False, hw, R)
            o = R.b(mm(a, t[a_ + "o_proj.weight"]))
            x = R.f(x + norm(o, t[p + "post_attention_layernorm.weight"]))
            ug = R.b(mm(R.b(norm(x, t[p + "pre_feedforward_layernorm.weight"])), t[p + "mlp.up_gate.weight"]))
            o = R.b(mm(R.b(ug[:, :F] * _gelu_tanh(ug[:, F:])), t[p + "mlp.down_proj.weight"]))
            x = R.f(x + norm(o, t[p + "post_feedforward_layernorm.weight"]))
            if l + 1 < layers:
                nxt = l if mut == "next_norm_same_block" else l + 1
                h = R.b(norm(x, t[f"layers.{nxt}.input_layernorm.weight"]))
            streams.append(x)
        final_g = t["norm.weight"]

    if mut == "stale_row":      # the row of the last block keeps what the block before left (the embedding's row behind a one-block call is not modelled)
        assert layers >= 2, "stale_row needs two blocks"
        last = streams[-1].clone()
        last[sum(lens) // 2] = streams[-2][sum(lens) // 2]
        streams[-1] = last
    x = streams[-1]
    final = R.f(norm(x, final_g))

    # ---- the pooled rows, with and without L2
    first = torch.tensor([sum(lens[:i]) for i in range(len(lens))], device=dev)
    lasti = first + torch.tensor(lens, device=dev) - 1
    seq_of = torch.repeat_interleave(torch.arange(len(lens), device=dev), torch.tensor(lens, device=dev))
    sums = torch.zeros(len(lens), W, dtype=F64, device=dev).index_add_(0, seq_of, final)
    pools = {"mean": R.f(sums / torch.tensor(lens, dtype=F64, device=dev)[:, None]), "cls": final[first]}
    gather = (lasti - 1).clamp(min=0) if mut == "last_row_minus1" else lasti
    gather = torch.maximum(gather, first)
    pools["last"] = R.f(norm(x[gather], final_g))       # (per row: the final norm of the gathered rows is the gathered rows of the final norm)
    pooled = {}
    for name, rows in pools.items():
        pooled[(name, 0)] = rows
        pooled[(name, 1)] = R.f(rows / rows.norm(dim=-1, keepdim=True))
    return Pass(blocks=streams, final=final, pooled=pooled)


def exact(family: str, arch, tensors: Dict[str, Tensor], ids: Tensor, lens: Sequence[int], layers: Optional[int] = None) -> Pass:
    return _run(family, arch, tensors, ids, lens, False, layers, None, 0)


def model(family: str, arch, tensors: Dict[str, Tensor], ids: Tensor, lens: Sequence[int], layers: Optional[int] = None, mut: Optional[str] = None,
          hist: int = 0) -> Pass:
    return _run(family, arch, tensors, ids, lens, True, layers, mut, hist)


# ---- seeded tiny checkpoints, batches and the cases both test files run -------------------------------------------------------------------------------

PACKED = E.PACKED                                   # [1, 17, 70, 129]
BAND_EDGES = [63, 64, 65]                           # the 64-query slices of csrc/attention_window.hip and csrc/attention_gqa256.hip
GQA_EDGES = [127, 128, 129]                         # the 128-query slices of csrc/attention_gqa.hip
POOLS = dict(modernbert=("mean", "cls"), qwen=("last", "mean"), gemma=("mean", "cls"))


@dataclass
class Case:
    id: str
    family: str
    cfg: dict                   # the HF config.json of the tiny checkpoint
    seed: int

    def batches(self):
        return (("packed217", PACKED), ("edges", GQA_EDGES if self.family == "qwen" else BAND_EDGES))


def _ref_module(family):
    from tests import gemma_ref, modernbert_ref, qwen_ref
    return dict(modernbert=modernbert_ref, qwen=qwen_ref, gemma=gemma_ref)[family]


def cases() -> List[Case]:
    from tests import gemma_ref as G, modernbert_ref as M, qwen_ref as Q
    cs = [
        # `big` of the plan is max(3 W, 2 F): 384 on either side at the tiny's F = 192
        Case("modernbert-tiny[F=192:3W==2F]", "modernbert", M.config_dict(), 0),
        Case("modernbert-F128[3W>2F]", "modernbert", M.config_dict(intermediate_size=128), 1),
        Case("modernbert-F256[3W<2F]", "modernbert", M.config_dict(intermediate_size=256), 2),
        Case("qwen-TINY3[qk_norm,hd128,qkv1024>2F]", "qwen", dict(Q.TINY3), 3),
        Case("qwen-TINY2[qkv_bias,hd64,qkv384<2F]", "qwen", dict(Q.TINY2), 4),
        Case("qwen-TINY64[heads*64!=W]", "qwen", dict(Q.TINY64), 5),
        Case("gemma-TINY[sliding,sliding,full]", "gemma", dict(G.TINY), 6),
        Case("gemma-TINY_SLIDING", "gemma", dict(G.TINY_SLIDING), 7),
        Case("gemma-TINY_FULL", "gemma", dict(G.TINY_FULL), 8),
        Case("gemma-F1024[2F>qkv1024]", "gemma", G.config_dict(G.TINY, intermediate_size=1024), 9),
    ]
    return cs


_built: Dict[str, dict] = {}


def build(case: Case) -> dict:
    """the seeded checkpoint of a case: dict(arch, sd = transformers' tensors with every Linear weight rounded to bf16 — what the towers store, so that the
    fp32 oracles of the *_ref modules and this module's reference start from the same operands —, tensors = the loader's output on that sd)"""
    if case.id not in _built:
        from marqo_amd.engine import archs, tower_weights as TW
        ref = _ref_module(case.family)
        sd = ref.state_dict_of(ref.hf_model(case.cfg, seed=case.seed))
        sd = {k: (v.to(torch.bfloat16).float() if (v.dim() == 2 and "tok_embeddings" not in k and "embed_tokens" not in k) else v.float()) for k, v in sd.items()}
        arch = archs.bert_arch_from_hf_config(case.cfg)
        loader = dict(modernbert=TW.modernbert_state_dict, qwen=TW.qwen_state_dict, gemma=TW.gemma_state_dict)[case.family]
        _built[case.id] = dict(arch=arch, sd=sd, tensors=loader(arch, sd))
    return _built[case.id]


def seqs_of(case: Case, lens: Sequence[int], seed: int = 3) -> List[Tensor]:
    return _ref_module(case.family).random_seqs(list(lens), case.cfg["vocab_size"], seed=seed)


def applies(mut: str, case: Case, arch) -> bool:
    """whether the mutant changes anything of this case's orchestration"""
    sliding = tuple(getattr(arch, "sliding", ()))
    if mut in ("local_gets_global", "window_plus1", "window_minus1"):
        return any(sliding)
    if mut == "global_gets_local":
        return case.family != "qwen" and not all(sliding)
    if mut == "pattern_shift":
        return any(sliding) and not all(sliding)
    if mut == "layer0_attn_norm":
        return case.family == "modernbert"
    if mut in ("next_norm_same_block", "no_embed_scale"):
        return case.family == "gemma"
    if mut == "no_qkv_bias":
        return case.family == "qwen" and arch.qkv_bias
    if mut == "last_row_minus1":
        return case.family == "qwen"
    return True


def views(p: Pass, pool: str) -> Tensor:
    """the stream the workspace's first slice holds behind a call with this pooling: the final norm runs in place over every row, except under Qwen's
    last-token pooling, where only the gathered rows take it"""
    return p.blocks[-1] if pool == "last" else p.final

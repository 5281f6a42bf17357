"""Helpers of the JinaBERT tests (tests/test_jina_bert_host.py, tests/test_attention_alibi_gpu.py, tests/test_jina_bert_gpu.py).  Nothing here calls the
library.

  - the float64 reference of attention with an ALiBi bias — scores = scale (q . k) - slope_h |k - q| — on the budget and input families of
    tests/attention_ref.py (imported, not changed), with four switchable faults of the bias, the bias-only inputs, and the slopes and cases the GPU file
    and the host file's precondition check share;
  - tiny configs (TINY_2H, TINY_3H), seeded random checkpoints in JinaBERT's tensor names, a WordPiece tokenizer.json trained in memory and a checkpoint
    directory as a user brings it;
  - exact / model: the float64 restatement of csrc/jina_bert.hip's block formula over a packed token stream, in the manner of tests/t5_ref.py (whose
    Pass and row_ratio are reused): `model` rounds to bf16 / fp32 exactly where the tower stores bf16 / fp32, `exact` rounds nothing.

JinaBERT is custom remote code whose modelling file is not available to these tests: the block formula restates the published architecture and is NOT
pinned to a run of the original code.  What can be pinned is: the slopes (against transformers' Bloom build_alibi_tensor, tests/test_jina_bert_host.py).

Where `model` rounds:  e = LN_emb(tok[ids] + type0): x = fp32(e), h = bf16(e) ; qkv = bf16(h Wqkv^T + b) ; p = bf16, un-normalised, for P V, the normaliser
sums the unrounded p ; a = bf16 ; y = fp32(x + a Wo^T + bo) (the GEMM epilogue's one store) ; n = LN_attn(y): x = fp32(n), h = bf16(n) ; (up | gate) = bf16 ;
product = bf16 ; y = fp32(x + product Wwo^T + bwo) ; n = LN_mlp(y): x = fp32(n), h = bf16(n) ; mean = fp32(sum / len) ; L2 = fp32(row / |row|).
hist = 1 is a second rounding history: every GEMM sums fp32 partial products of 64-wide k chunks in reverse order (encoder_ref._mm).

Mutants of the orchestration (`mut=`, MUTANTS):
    gate_swapped       the halves of mlp.gated_layers change places (up * gelu(gate) becomes gate * gelu(up))
    slopes_reversed    head h takes the slope of head heads - 1 - h
    bias_scaled        the bias is multiplied by the softmax scale 1 / sqrt(head_dim) as the q . k product is
    no_abs             the bias is -slope (k - q): keys in front of the query are favoured without bound
    pre_ln             the blocks run pre-LN: x += Wo attn(LN_attn(x)) ; x += mlp(LN_mlp(x))
"""
import json
import math
import os
from typing import Dict, List, Optional, Sequence

import torch

from tests import attention_ref as AR
from tests import encoder_ref as E
from tests.packed_text_ref import Pass, row_ratio      # noqa: F401

Tensor = torch.Tensor
F64 = torch.float64
SLICE = 64                 # queries per workgroup of csrc/attention_alibi.hip (four 16-query blocks)
LDS_KEYS = {64: 640}       # keys of K + V its LDS holds (nothing shares the 160 KiB)
MUTANTS = ("gate_swapped", "slopes_reversed", "bias_scaled", "no_abs", "pre_ln")
BIAS_FAULTS = ("index_plus1", "no_abs", "next_head_slope", "bias_scaled")
MIN_LOG2_P = -100.0        # the precondition of the cases that isolate single probabilities (readout, bias only)


# ---- attention with an ALiBi bias --------------------------------------------------------------------------------------------------------------------
def alibi_scores(q, k, slopes, scale, fault=None):
    """[heads, len, hd] float64 q and k -> [heads, len, len] float64 scores; `fault`: ONE deliberate fault of the bias (BIAS_FAULTS)"""
    ln, dev = q.shape[1], q.device
    pos = torch.arange(ln, device=dev)
    d = (pos[None, :] - pos[:, None]).to(F64)
    if fault == "index_plus1":
        d = d + 1
    dist = d if fault == "no_abs" else d.abs()
    sl = slopes.to(dev).double()
    if fault == "next_head_slope":
        sl = sl.roll(-1)
    bias = -sl[:, None, None] * dist[None]
    if fault == "bias_scaled":
        bias = bias * scale
    return q @ k.transpose(1, 2) * scale + bias


def alibi_reference(qkv_bf16, lens, heads, hd, slopes, scale, fault=None):
    """float64 attention with the ALiBi bias on the device of `qkv_bf16` -> (out, absout) = (P V, P |V|), float64 [rows, heads hd]; attention_ref.reference
    with its fixed scale and its table replaced (test_jina_bert_host.py holds the two equal where attention_ref.reference can express the bias)"""
    W, dev, rows = heads * hd, qkv_bf16.device, qkv_bf16.shape[0]
    assert qkv_bf16.dtype == torch.bfloat16 and qkv_bf16.shape[1] == 3 * W and rows == sum(lens) and tuple(slopes.shape) == (heads,)
    out = torch.zeros(rows, W, dtype=F64, device=dev)
    absout = torch.zeros(rows, W, dtype=F64, device=dev)
    r0 = 0
    for ln in lens:
        blk = qkv_bf16[r0:r0 + ln].double().reshape(1, ln, 3 * W)
        q, k, v = (AR._heads_of(t, heads, hd)[0] for t in blk.split(W, dim=2))
        p = torch.softmax(alibi_scores(q, k, slopes, scale, fault), dim=-1)
        out[r0:r0 + ln] = (p @ v).transpose(0, 1).reshape(ln, W)
        absout[r0:r0 + ln] = (p @ v.abs()).transpose(0, 1).reshape(ln, W)
        r0 += ln
    return out, absout


def min_log2_probability(qkv_bf16, lens, heads, hd, slopes, scale):
    """log2 of the smallest float64 softmax probability of the inputs"""
    W = heads * hd
    worst, r0 = 0.0, 0
    for ln in lens:
        blk = qkv_bf16[r0:r0 + ln].double().reshape(1, ln, 3 * W)
        q, k, _ = (AR._heads_of(t, heads, hd)[0] for t in blk.split(W, dim=2))
        worst = min(worst, float(torch.log_softmax(alibi_scores(q, k, slopes, scale), dim=-1).min()) / math.log(2.0))
        r0 += ln
    return worst


def alibi_table(slopes, span):
    """the bias as attention_ref.reference takes it: [heads, 2 span - 1], entry d + span - 1 for key - query == d"""
    d = torch.arange(-(span - 1), span, dtype=F64)
    return -slopes.double()[:, None] * d.abs()[None]


def slopes_of(heads):
    from marqo_amd.engine.archs import JinaBertArch
    return torch.tensor(JinaBertArch(heads=heads, width=64 * heads).slopes(), dtype=F64).float()


def real_slopes(heads):
    """the slope sets of the randn / peaked cases: the first `heads` values of the 8-head and of the 12-head list (2^-1, 2^-2, 2^-3 in both: the steep
    power-of-two ones), and the 12-head list's non-dyadic tail (2^-0.5, 2^-1.5, 2^-2.5: the steepest there are)"""
    return (("8h", slopes_of(8)[:heads]), ("12h", slopes_of(12)[:heads]), ("12h_tail", slopes_of(12)[8:8 + heads]))


def readout_slopes(max_len, heads):
    """distinct slopes 2^-k, 2^-(k + 1), .. for the cases that isolate single probabilities, k the smallest (>= 1) with 2^-k (max_len - 1) <= 44 nats:
    that leaves 25 of the 69.3 nats of 2^-100 to the spread of the q . k logits and to the normaliser.  These are values of the real lists (8 heads:
    2^-1 .. 2^-8).  The precondition itself is asserted on the very inputs by tests/test_jina_bert_host.py."""
    k = max(1, math.ceil(math.log2(max(max_len - 1, 1) / 44.0)))
    return torch.tensor([2.0 ** -(k + i) for i in range(heads)], dtype=torch.float32)


def bias_only_qkv(lens, heads, hd, device="cpu"):
    """q = k = 0 and attention_ref's `readout` V (one-hot codes of the key index): the output is softmax(bias row) applied to V"""
    rows, W = sum(lens), heads * hd
    v = AR.readout_v(lens, heads, hd).reshape(rows, W)
    return torch.cat([torch.zeros(rows, 2 * W), v], dim=1).to(torch.bfloat16).to(device)


def family_qkv(fam, lens, heads, hd, scale, seed, device="cpu"):
    """attention_ref.make_qkv; at scale 1.0 the 1 / sqrt(hd) rides in q (the logits are those of the 1 / sqrt(hd) calls, formed on the other path: raw
    unit-variance inputs at scale 1.0 underflow fp32, which the relative budget has no term for — tests/test_attention_relbias_gpu.py)"""
    qkv = AR.make_qkv(fam, lens, heads, hd, seed=seed)
    if scale == 1.0:
        qkv[:, :heads * hd] = (qkv[:, :heads * hd].float() * hd ** -0.5).to(torch.bfloat16)
    return qkv.to(device)


MIXED = [1, 15, 16, 17, 63, 64, 65, 129, 300]
EDGES = [SLICE - 1, SLICE, SLICE + 1, 2 * SLICE - 1, 2 * SLICE, 2 * SLICE + 1]
SCALES = (1.0, 64 ** -0.5)
BIAS_ONLY = ([300, 17], [65, 9], [700])


def readout_cases():
    """(tag, lens, heads, scale, seed, fixed) of every `readout` call of tests/test_attention_alibi_gpu.py: head width 64 throughout"""
    cs = []
    for heads in (2, 3):
        for scale in SCALES:
            cs.append(("mixed", MIXED, heads, scale, 64 + heads, False))
    for ln in EDGES:
        cs.append(("slice", [ln], 2, 1.0, ln, False))
    cs.append(("fixed77", [77] * 3, 2, 1.0, 77, True))
    cs.append(("fixed77", [77] * 3, 3, 64 ** -0.5, 78, True))
    cs.append(("long", [700], 2, 1.0, 700, False))
    cs.append(("long", [1300], 3, 64 ** -0.5, 1300, False))
    return cs


# ---- tiny checkpoints ---------------------------------------------------------------------------------------------------------------------------------
_COMMON = dict(model_type="bert", position_embedding_type="alibi", feed_forward_type="geglu", hidden_act="gelu", vocab_size=384, num_hidden_layers=2,
               max_position_embeddings=8192, layer_norm_eps=1e-12, type_vocab_size=2, pad_token_id=0)
TINY_2H = dict(_COMMON, hidden_size=128, num_attention_heads=2, intermediate_size=256)
TINY_3H = dict(_COMMON, hidden_size=192, num_attention_heads=3, intermediate_size=320)      # non-power-of-two slopes, F != 2 W
TINIES = {"TINY_2H": TINY_2H, "TINY_3H": TINY_3H}
TOWER_LENS = [1, 2, 64, 65, 200]


def config_dict(base, **over):
    return dict(base, **over)


def random_state_dict(cfg: dict, seed: int = 0, gain: float = 0.6, prefix: str = "") -> Dict[str, Tensor]:
    """seeded tensors in JinaBERT's names with working magnitudes (the gain of t5_ref.randomize): LayerNorm weights 1 + 0.1 N(0, 1), every bias
    0.1 N(0, 1), the token and type tables N(0, 1), Linear weights N(0, gain / sqrt(in)), query and key x 2 (so that q . k / 8 decides which keys a
    query reads next to the bias); every Linear weight rounded to bf16 — what the tower stores.  Also a pooler and a stray position table, to be ignored."""
    g = torch.Generator().manual_seed(5000 + seed)
    W, F, V = cfg["hidden_size"], cfg["intermediate_size"], cfg["vocab_size"]
    rn = lambda *shape: torch.randn(*shape, generator=g)
    lin = lambda out_f, in_f, mul=1.0: (rn(out_f, in_f) * (mul * gain / math.sqrt(in_f))).to(torch.bfloat16).float()
    sd = {"embeddings.word_embeddings.weight": rn(V, W), "embeddings.token_type_embeddings.weight": rn(cfg["type_vocab_size"], W),
          "embeddings.LayerNorm.weight": 1.0 + 0.1 * rn(W), "embeddings.LayerNorm.bias": 0.1 * rn(W),
          "embeddings.position_embeddings.weight": rn(16, W), "embeddings.position_ids": torch.arange(16)[None],
          "pooler.dense.weight": rn(W, W), "pooler.dense.bias": rn(W)}
    for l in range(cfg["num_hidden_layers"]):
        p = f"encoder.layer.{l}."
        for c in ("query", "key", "value"):
            sd[p + f"attention.self.{c}.weight"] = lin(W, W, 1.0 if c == "value" else 2.0)
            sd[p + f"attention.self.{c}.bias"] = 0.1 * rn(W)
        sd[p + "attention.output.dense.weight"], sd[p + "attention.output.dense.bias"] = lin(W, W), 0.1 * rn(W)
        sd[p + "attention.output.LayerNorm.weight"], sd[p + "attention.output.LayerNorm.bias"] = 1.0 + 0.1 * rn(W), 0.1 * rn(W)
        sd[p + "mlp.gated_layers.weight"] = lin(2 * F, W)
        sd[p + "mlp.wo.weight"], sd[p + "mlp.wo.bias"] = lin(W, F), 0.1 * rn(W)
        sd[p + "mlp.layernorm.weight"], sd[p + "mlp.layernorm.bias"] = 1.0 + 0.1 * rn(W), 0.1 * rn(W)
    return {prefix + k: v for k, v in sd.items()}


def random_seqs(lengths, vocab, seed=0):
    g = torch.Generator().manual_seed(9000 + seed)
    return [torch.randint(5, vocab, (n,), generator=g) for n in lengths]


# ---- a checkpoint directory as a user brings it -----------------------------------------------------------------------------------------------------
PAD, UNK, CLS, SEP, MASK = "[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"


def train_tokenizer(vocab_size=300):
    """a WordPiece `tokenizers.Tokenizer` (BERT normaliser and pre-tokeniser, lower-casing) trained from modernbert_ref.CORPUS in memory, [PAD] / [UNK] /
    [CLS] / [SEP] / [MASK] as ids 0 .. 4 and — as BERT's file — a TemplateProcessing of [CLS] $A [SEP]"""
    from tokenizers import Tokenizer, decoders, models, normalizers, pre_tokenizers, processors, trainers
    from tests.modernbert_ref import CORPUS
    tk = Tokenizer(models.WordPiece(unk_token=UNK))
    tk.normalizer = normalizers.BertNormalizer(lowercase=True)
    tk.pre_tokenizer = pre_tokenizers.BertPreTokenizer()
    tk.decoder = decoders.WordPiece()
    trainer = trainers.WordPieceTrainer(vocab_size=vocab_size, special_tokens=[PAD, UNK, CLS, SEP, MASK], show_progress=False)
    tk.train_from_iterator(CORPUS * 4, trainer)
    assert [tk.token_to_id(t) for t in (PAD, UNK, CLS, SEP, MASK)] == [0, 1, 2, 3, 4] and tk.get_vocab_size() <= 384
    tk.post_processor = processors.TemplateProcessing(single=f"{CLS} $A {SEP}", pair=f"{CLS} $A {SEP} $B:1 {SEP}:1", special_tokens=[(CLS, 2), (SEP, 3)])
    return tk


def write_checkpoint_dir(directory, cfg, sd, tokenizer=None, pooling=None):
    """config.json + model.safetensors (+ tokenizer.json, tokenizer_config.json naming the specials; + 1_Pooling/config.json when `pooling` is 'mean' / 'cls')"""
    from safetensors.torch import save_file
    os.makedirs(directory, exist_ok=True)
    with open(os.path.join(directory, "config.json"), "w") as f:
        json.dump(cfg, f)
    save_file({k: v.contiguous() for k, v in sd.items()}, os.path.join(directory, "model.safetensors"))
    if tokenizer is not None:
        tokenizer.save(os.path.join(directory, "tokenizer.json"))
        with open(os.path.join(directory, "tokenizer_config.json"), "w") as f:
            json.dump({"cls_token": CLS, "sep_token": SEP, "pad_token": PAD, "unk_token": UNK, "mask_token": MASK}, f)
    if pooling is not None:
        os.makedirs(os.path.join(directory, "1_Pooling"), exist_ok=True)
        with open(os.path.join(directory, "1_Pooling", "config.json"), "w") as f:
            json.dump({"word_embedding_dimension": cfg["hidden_size"], "pooling_mode_cls_token": pooling == "cls", "pooling_mode_mean_tokens": pooling == "mean"}, f)
    return directory


# ---- the float64 pass -------------------------------------------------------------------------------------------------------------------------------
_FORM = E.Form("jina_bert")


def operands(tensors: Dict[str, Tensor], device) -> Dict[str, Tensor]:
    """jina_bert_state_dict's fp32 tensors as the tower stores them, in float64: the weight matrices to bf16; the token table, biases and LayerNorm weights fp32"""
    return {k: (E._w16(v) if v.dim() == 2 and k != "word_embeddings.weight" else E._f32(v)).to(device) for k, v in tensors.items()}


def _attention(qkv, lens, H, hd, slopes, scale, R, fault=None):
    dev = qkv.device
    A = H * hd
    out = torch.zeros(qkv.shape[0], A, dtype=F64, device=dev)
    r0 = 0
    for ln in lens:
        blk = qkv[r0:r0 + ln]
        q, k, v = (blk[:, i * A:(i + 1) * A].reshape(ln, H, hd).transpose(0, 1) for i in range(3))
        s = alibi_scores(q, k, slopes, scale, fault)
        p = torch.exp(s - s.max(-1, keepdim=True).values)
        o = (R.b(p) @ v) / p.sum(-1, keepdim=True)
        out[r0:r0 + ln] = R.b(o).transpose(0, 1).reshape(ln, A)
        r0 += ln
    return out


def _run(arch, tensors, ids, lens, rounds, layers, mut, hist) -> Pass:
    assert mut is None or mut in MUTANTS
    dev = ids.device
    lens = [int(n) for n in lens]
    assert ids.dim() == 1 and ids.shape[0] == sum(lens) and min(lens) >= 1
    layers = arch.layers if layers is None else layers
    t = operands(tensors, dev)
    R = E._Round(_FORM if rounds else None)
    hist = hist if rounds else 0
    mm = lambda x, w: E._mm(x, w, hist)
    W, F, H, hd, eps = arch.width, arch.mlp_dim, arch.heads, arch.head_dim, arch.ln_eps
    slopes = torch.tensor(arch.slopes(), dtype=F64).float()          # what the tower uploads
    if mut == "slopes_reversed":
        slopes = slopes.flip(0)
    scale = float(torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(hd), dtype=torch.float32).sqrt())
    fault = mut if mut in ("bias_scaled", "no_abs") else None
    ln = lambda y, name: E._ln(y, t[name + ".weight"], t[name + ".bias"], eps)
    e = ln(t["word_embeddings.weight"][ids.long()] + t["type0"], "emb_ln")
    x, h = R.f(e), R.b(e)
    streams: List[Tensor] = []
    for l in range(layers):
        p = f"layer.{l}."
        if mut == "pre_ln":
            h = R.b(ln(x, p + "attn_ln"))
        qkv = R.b(mm(h, t[p + "attn.qkv.weight"]) + t[p + "attn.qkv.bias"])
        a = _attention(qkv, lens, H, hd, slopes, scale, R, fault)
        y = R.f(x + mm(a, t[p + "attn.o.weight"]) + t[p + "attn.o.bias"])
        if mut == "pre_ln":
            x, h = y, R.b(ln(y, p + "mlp_ln"))
        else:
            n = ln(y, p + "attn_ln")
            x, h = R.f(n), R.b(n)
        ug = R.b(mm(h, t[p + "mlp.up_gate.weight"]))
        up, gate = (ug[:, F:], ug[:, :F]) if mut == "gate_swapped" else (ug[:, :F], ug[:, F:])
        y = R.f(x + mm(R.b(up * E._act(gate, "gelu")), t[p + "mlp.wo.weight"]) + t[p + "mlp.wo.bias"])
        if mut == "pre_ln":
            x = y
        else:
            n = ln(y, p + "mlp_ln")
            x, h = R.f(n), R.b(n)
        streams.append(x)
    final = x                                     # no final norm
    first = torch.tensor([sum(lens[:i]) for i in range(len(lens))], device=dev)
    seq_of = torch.repeat_interleave(torch.arange(len(lens), device=dev), torch.tensor(lens, device=dev))
    sums = torch.zeros(len(lens), W, dtype=F64, device=dev).index_add_(0, seq_of, final)
    pools = {"mean": R.f(sums / torch.tensor(lens, dtype=F64, device=dev)[:, None]), "cls": final[first]}
    out = {}
    for name, rows in pools.items():
        out[(name, 0)] = rows
        out[(name, 1)] = R.f(rows / rows.norm(dim=-1, keepdim=True))
    return Pass(blocks=streams, final=final, pooled=out)


def exact(arch, tensors, ids, lens, layers: Optional[int] = None) -> Pass:
    return _run(arch, tensors, ids, lens, False, layers, None, 0)


def model(arch, tensors, ids, lens, layers: Optional[int] = None, mut: Optional[str] = None, hist: int = 0) -> Pass:
    return _run(arch, tensors, ids, lens, True, layers, mut, hist)


_built: Dict[str, dict] = {}


def build(name: str) -> dict:
    """the seeded checkpoint of TINIES[name]: dict(cfg, arch, sd, tensors = jina_bert_state_dict's output, seqs)"""
    if name not in _built:
        from marqo_amd.engine import archs, tower_weights as TW
        cfg = TINIES[name]
        arch = archs.bert_arch_from_hf_config(cfg)
        sd = random_state_dict(cfg, seed=1 + list(TINIES).index(name))
        _built[name] = dict(cfg=cfg, arch=arch, sd=sd, tensors=TW.jina_bert_state_dict(arch, sd), seqs=random_seqs(TOWER_LENS, cfg["vocab_size"], seed=3))
    return _built[name]

"""Helpers of the T5 encoder tests (tests/test_t5_host.py, tests/test_attention_relbias_gpu.py, tests/test_t5_gpu.py).  Nothing here calls the library.

  - the float64 reference of attention with a clamped relative-position bias — scores = scale (q . k) + table[h][clamp(k - q, -D, D) + D] — on the budget
    and input families of tests/attention_ref.py (imported, not changed), with three switchable faults of the bias lookup, and the bias-only inputs;
  - tiny random checkpoints (TINY_RELU, TINY_GATED, TINY_WIDE) of transformers' T5EncoderModel, fp32 on the CPU: the oracle of the tower tests;
  - a Unigram tokenizer.json trained in memory and a checkpoint directory as a user brings it (1_Pooling, 2_Dense, sentence_bert_config.json);
  - exact / model: the float64 restatement of csrc/t5.hip's block formula over a packed token stream, in the manner of tests/packed_text_ref.py (whose
    Pass, row_ratio and rounding helpers are reused): `model` rounds to bf16 / fp32 exactly where the tower stores bf16 / fp32, `exact` rounds nothing.

Where `model` rounds:  x = fp32(tok[ids]) ; h = bf16(rms(x) g) ; qkv = bf16(h Wqkv^T) ; p = bf16, un-normalised, for P V, the normaliser sums the unrounded
p ; a = bf16 ; x = fp32(x + a Wo^T) ; relu: hid = bf16(relu(h Wi^T)) ; gated: (up | gate) = bf16, product = bf16 (gelu_new in the kernel's form
x / (1 + exp(-2u))) ; x = fp32(x + hid Wo_ff^T) ; the final norm = fp32 ; mean = fp32(sum / len) ; L2 = fp32(row / |row|).
hist = 1 is a second rounding history: every GEMM sums fp32 partial products of 64-wide k chunks in reverse order (encoder_ref._mm).

Mutants of the orchestration (`mut=`, MUTANTS):
    bias_per_layer     every block looks its bias up in its OWN block: blocks 1 .. run without one (only block 0 carries the table)
    scaled             the scores are multiplied by 1 / sqrt(d_kv) (T5 applies no scale)
    wi_swapped         gated MLP: wi_0 and wi_1 change places (up * gelu_new(gate) becomes gate * gelu_new(up))
    eps_x10            every norm's eps times ten
    bias_sign          the table is read at query - key instead of key - query
"""
import json
import math
import os
from typing import Dict, List, Optional, Sequence

import torch

from tests import attention_ref as AR
from tests import encoder_ref as E
from tests import gemma_ref as G
from tests import qwen_ref as Q
from tests.packed_text_ref import Pass, row_ratio, _gelu_tanh, _rms      # noqa: F401

Tensor = torch.Tensor
F64 = torch.float64
SLICE = 64          # queries per workgroup of csrc/attention_relbias.hip (four 16-query blocks)
LDS_KEYS = {64: 576, 128: 256}      # keys of K + V its LDS holds next to the bias table
MUTANTS = ("bias_per_layer", "scaled", "wi_swapped", "eps_x10", "bias_sign")
BIAS_FAULTS = ("index_plus1", "sign", "clamp_minus1")


# ---- attention with a clamped relative bias --------------------------------------------------------------------------------------------------------------
def bias_index(ln, D, device="cpu", fault=None):
    """[query, key] int64: the table column of key - query, clamped to [-D, D] and shifted by D; `fault`: ONE deliberate fault of the lookup (BIAS_FAULTS)"""
    pos = torch.arange(ln, device=device)
    d = pos[None, :] - pos[:, None]
    if fault == "sign":
        d = -d
    if fault == "index_plus1":
        d = d + 1
    lim = D - 1 if fault == "clamp_minus1" else D
    return d.clamp(-lim, lim) + D


def relbias_reference(qkv_bf16, lens, heads, hd, table, D, scale, fault=None):
    """float64 attention with the clamped bias on the device of `qkv_bf16` -> (out, absout) = (P V, P |V|), float64 [rows, heads hd]; attention_ref.reference
    with its fixed scale and unclamped table replaced"""
    W, dev, rows = heads * hd, qkv_bf16.device, qkv_bf16.shape[0]
    assert qkv_bf16.dtype == torch.bfloat16 and qkv_bf16.shape[1] == 3 * W and rows == sum(lens) and tuple(table.shape) == (heads, 2 * D + 1)
    out = torch.zeros(rows, W, dtype=F64, device=dev)
    absout = torch.zeros(rows, W, dtype=F64, device=dev)
    tab = table.to(dev).double()
    r0 = 0
    for ln in lens:
        blk = qkv_bf16[r0:r0 + ln].double().reshape(1, ln, 3 * W)
        q, k, v = (AR._heads_of(t, heads, hd)[0] for t in blk.split(W, dim=2))
        s = q @ k.transpose(1, 2) * scale + tab[:, bias_index(ln, D, dev, fault)]
        p = torch.softmax(s, dim=-1)
        out[r0:r0 + ln] = (p @ v).transpose(0, 1).reshape(ln, W)
        absout[r0:r0 + ln] = (p @ v.abs()).transpose(0, 1).reshape(ln, W)
        r0 += ln
    return out, absout


def make_table(heads, D, seed=0, kind="randn"):
    """fp32 [heads, 2 D + 1].  `randn`: N(0, 1.5).  `distinct`: a permutation of 2 D + 1 equally spaced values in [-3, 3] per head — every column its own
    value, so +d and -d differ and so do neighbours"""
    g = torch.Generator().manual_seed(900 + seed)
    n = 2 * D + 1
    if kind == "randn":
        return 1.5 * torch.randn(heads, n, generator=g)
    return torch.stack([torch.linspace(-3.0, 3.0, n)[torch.randperm(n, generator=g)] for _ in range(heads)]).float()


def bias_only_qkv(lens, heads, hd, device="cpu"):
    """q = k = 0 and attention_ref's `readout` V (one-hot codes of the key index): the output is softmax(bias row) applied to V, one wrong key or sign shows"""
    rows, W = sum(lens), heads * hd
    v = AR.readout_v(lens, heads, hd).reshape(rows, W)
    return torch.cat([torch.zeros(rows, 2 * W), v], dim=1).to(torch.bfloat16).to(device)


# ---- tiny checkpoints -----------------------------------------------------------------------------------------------------------------------------------
_COMMON = dict(model_type="t5", vocab_size=384, d_model=128, d_ff=256, num_layers=2, relative_attention_num_buckets=32, relative_attention_max_distance=128,
               layer_norm_epsilon=1e-6, pad_token_id=0, eos_token_id=1, dropout_rate=0.0)
TINY_RELU = dict(_COMMON, num_heads=2, d_kv=64, feed_forward_proj="relu")
TINY_GATED = dict(_COMMON, num_heads=2, d_kv=64, feed_forward_proj="gated-gelu")
TINY_WIDE = dict(_COMMON, num_heads=3, d_kv=128, feed_forward_proj="relu")          # inner 384 != d_model 128
TINIES = {"TINY_RELU": TINY_RELU, "TINY_GATED": TINY_GATED, "TINY_WIDE": TINY_WIDE}

config_dict = Q.config_dict
state_dict_of = Q.state_dict_of
pad_batch = Q.pad_batch
pooled = G.pooled


def random_seqs(lengths, vocab, seed=0):
    g = torch.Generator().manual_seed(9000 + seed)
    return [torch.randint(2, vocab, (n,), generator=g) for n in lengths]


def hf_model(cfg: dict, seed: int = 0, gain: float = 0.6):
    """transformers' T5EncoderModel for the config dict: fp32, eval, weights from `randomize`"""
    import transformers
    kw = {k: v for k, v in cfg.items() if k != "model_type"}
    config = transformers.T5Config(**kw, is_encoder_decoder=False, use_cache=False)
    config._attn_implementation = "eager"
    model = transformers.T5EncoderModel(config).float().eval()
    randomize(model, seed, gain)
    return model


def randomize(model, seed, gain=0.6):
    """seeded weights with working magnitudes: norm weights 1 + 0.1 N(0, 1); token table 0.01 N(0, 1) — rows small enough that the eps of the first norm (1e-6 against a mean square of 1e-4) is seen; the bias table N(0, 1.5) (so that it decides which
    keys a query reads); Linear weights N(0, gain / sqrt(in)), k x 2 and q x 2 / sqrt(d_kv) — T5 applies no softmax scale, the checkpoints carry it in q"""
    g = torch.Generator().manual_seed(4000 + seed)
    hd = model.config.d_kv
    with torch.no_grad():
        for name, p in model.named_parameters():
            if p.ndim == 1:
                p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g))
            elif "relative_attention_bias" in name:
                p.copy_(1.5 * torch.randn(p.shape, generator=g))
            elif "shared" in name or "embed_tokens" in name:
                p.copy_(0.01 * torch.randn(p.shape, generator=g))
            else:
                p.copy_(torch.randn(p.shape, generator=g) * (gain / math.sqrt(p.shape[1])))
                if name.endswith("SelfAttention.k.weight"):
                    p.mul_(2.0)
                if name.endswith("SelfAttention.q.weight"):
                    p.mul_(2.0 / math.sqrt(hd))


def oracle_hidden_packed(model, seqs):
    """transformers' own last hidden state of every sequence on its own, no padding anywhere -> list of fp32 [len, W]"""
    with torch.no_grad():
        return [model(input_ids=s[None]).last_hidden_state[0] for s in seqs]


# ---- a checkpoint directory as a user brings it ---------------------------------------------------------------------------------------------------------
PAD, EOS, UNK = "<pad>", "</s>", "<unk>"


def train_tokenizer(vocab_size=300):
    """a Unigram `tokenizers.Tokenizer` (Metaspace pieces, as T5's SentencePiece model) trained from modernbert_ref.CORPUS in memory, <pad> / </s> / <unk>
    as ids 0 / 1 / 2 and — as T5's file — a TemplateProcessing that appends </s>"""
    from tokenizers import Tokenizer, decoders, models, pre_tokenizers, processors, trainers
    from tests.modernbert_ref import CORPUS
    tk = Tokenizer(models.Unigram())
    tk.pre_tokenizer = pre_tokenizers.Metaspace()
    tk.decoder = decoders.Metaspace()
    trainer = trainers.UnigramTrainer(vocab_size=vocab_size, special_tokens=[PAD, EOS, UNK], unk_token=UNK, show_progress=False)
    tk.train_from_iterator(CORPUS * 4, trainer)
    assert (tk.token_to_id(PAD), tk.token_to_id(EOS), tk.token_to_id(UNK)) == (0, 1, 2) and tk.get_vocab_size() <= 384
    tk.post_processor = processors.TemplateProcessing(single=f"$A {EOS}", pair=f"$A {EOS} $B:1 {EOS}:1", special_tokens=[(EOS, 1)])
    return tk


def write_checkpoint_dir(directory, model, tokenizer=None, pooling=None, dense=(), dense_bias=False, dense_activation="torch.nn.modules.linear.Identity",
                         max_seq_length=None):
    """gemma_ref.write_checkpoint_dir (config.json + model.safetensors, 1_Pooling, N_Dense + modules.json) with T5's tokenizer files (tokenizer.json,
    tokenizer_config.json naming <pad> / </s> / <unk>) and, when `max_seq_length` is given, sentence_bert_config.json"""
    G.write_checkpoint_dir(directory, model, None, pooling=pooling, dense=dense, dense_bias=dense_bias, dense_activation=dense_activation)
    if tokenizer is not None:
        tokenizer.save(os.path.join(directory, "tokenizer.json"))
        with open(os.path.join(directory, "tokenizer_config.json"), "w") as f:
            json.dump({"pad_token": PAD, "eos_token": EOS, "unk_token": UNK}, f)
    if max_seq_length is not None:
        with open(os.path.join(directory, "sentence_bert_config.json"), "w") as f:
            json.dump({"max_seq_length": int(max_seq_length), "do_lower_case": False}, f)
    return directory


# ---- the float64 pass ---------------------------------------------------------------------------------------------------------------------------------
_FORM = E.Form("t5")


def operands(tensors: Dict[str, Tensor], device) -> Dict[str, Tensor]:
    """t5_state_dict's fp32 tensors as the tower stores them, in float64: the weight matrices to bf16; the token table, the bias table and the norm weights fp32"""
    return {k: (E._w16(v) if v.dim() == 2 and k not in ("embed_tokens.weight", "rel_bias") else E._f32(v)).to(device) for k, v in tensors.items()}


def _attention(qkv, lens, H, hd, table, D, scale, R, sign=1):
    dev = qkv.device
    A = H * hd
    out = torch.zeros(qkv.shape[0], A, dtype=F64, device=dev)
    r0 = 0
    for ln in lens:
        blk = qkv[r0:r0 + ln]
        q, k, v = (blk[:, i * A:(i + 1) * A].reshape(ln, H, hd).transpose(0, 1) for i in range(3))
        s = q @ k.transpose(1, 2) * scale
        if table is not None:
            s = s + table[:, bias_index(ln, D, dev, "sign" if sign < 0 else None)]
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
    W, F, H, hd, D = arch.width, arch.mlp_dim, arch.heads, arch.head_dim, arch.max_distance
    eps = arch.rms_eps * (10.0 if mut == "eps_x10" else 1.0)
    scale = 1.0 / math.sqrt(hd) if mut == "scaled" else 1.0
    x = R.f(t["embed_tokens.weight"][ids.long()])
    streams: List[Tensor] = []
    for l in range(layers):
        p = f"block.{l}."
        table = None if (mut == "bias_per_layer" and l > 0) else t["rel_bias"]
        qkv = R.b(mm(R.b(_rms(x, t[p + "attn_norm.weight"], eps)), t[p + "attn.qkv.weight"]))
        a = _attention(qkv, lens, H, hd, table, D, scale, R, sign=-1 if mut == "bias_sign" else 1)
        x = R.f(x + mm(a, t[p + "attn.o.weight"]))
        h = R.b(_rms(x, t[p + "ff_norm.weight"], eps))
        if arch.gated:
            ug = R.b(mm(h, t[p + "ff.wi.weight"]))
            up, gate = (ug[:, F:], ug[:, :F]) if mut == "wi_swapped" else (ug[:, :F], ug[:, F:])
            hid = R.b(up * _gelu_tanh(gate))
        else:
            hid = R.b(torch.relu(mm(h, t[p + "ff.wi.weight"])))
        x = R.f(x + mm(hid, t[p + "ff.wo.weight"]))
        streams.append(x)
    final = R.f(_rms(x, t["final_layer_norm.weight"], eps))
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


def applies(mut: str, arch) -> bool:
    return arch.gated if mut == "wi_swapped" else True


_built: Dict[str, dict] = {}
TOWER_LENS = [1, 2, 64, 65, 200]


def build(name: str) -> dict:
    """the seeded checkpoint of TINIES[name]: dict(cfg, model = transformers' T5EncoderModel with every Linear weight rounded to bf16 — what the tower
    stores, so that the transformers oracle and the float64 pass start from the same operands —, arch, sd, tensors = t5_state_dict's output, seqs)"""
    if name not in _built:
        from marqo_amd.engine import archs, tower_weights as TW
        cfg = TINIES[name]
        m = hf_model(cfg, seed=1 + list(TINIES).index(name))
        with torch.no_grad():
            for n, p in m.named_parameters():
                if p.ndim == 2 and "shared" not in n and "embed_tokens" not in n and "relative_attention_bias" not in n:
                    p.copy_(p.to(torch.bfloat16).float())
        arch = archs.bert_arch_from_hf_config(cfg)
        sd = state_dict_of(m)
        _built[name] = dict(cfg=cfg, model=m, arch=arch, sd=sd, tensors=TW.t5_state_dict(arch, sd), seqs=random_seqs(TOWER_LENS, cfg["vocab_size"], seed=3))
    return _built[name]

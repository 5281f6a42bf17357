"""Helpers of the DeBERTa tests (tests/test_deberta_host.py, tests/test_attention_disentangled_gpu.py, tests/test_deberta_gpu.py).  Nothing here calls the
library.

  - the float64 reference of disentangled attention — scores = scale (Q K^T + c2p + p2c) with both position terms gathered through ONE index
    idx(query - key) — on the budget and input families of tests/attention_ref.py (imported, not changed);
  - tiny configs (TINIES), each a seeded transformers DebertaV2ForSequenceClassification with working magnitudes, and a checkpoint directory as a user
    brings it (config.json, model.safetensors, a tokenizer.json built in memory by the `tokenizers` library, tokenizer_config.json);
  - exact / model: the float64 restatement of csrc/deberta.hip's block formula and the ContextPooler head over a packed token stream, on the tensors of
    engine/tower_weights.py::deberta_state_dict.  `exact` rounds nothing; `model` rounds to bf16 / fp32 exactly where the tower stores bf16 / fp32.
    tests/test_deberta_host.py pins `exact` to transformers' own float64 pass.

Where `model` rounds:  e = LN_emb(tok[ids]): x = fp32(e), h = bf16(e) ; qkv = bf16(h Wqkv^T + b) ; Kr, Qr = bf16 (stored at load) ; the position scores
c2p = Q Kr^T and p2c = K Qr^T = fp32 (the strips) ; p = bf16, un-normalised, for P V, the normaliser sums the unrounded p ; a = bf16 ;
y = fp32(x + a Wo^T + bo) ; n = LN_attn(y): x = fp32(n), h = bf16(n) ; f = bf16(gelu(h W1^T + b1)) ; y = fp32(x + f W2^T + b2) ; n = LN_mlp(y): x = fp32(n),
h = bf16(n) ; pooled = the [CLS] rows of x ; head: bf16(pooled) Wp^T + bp = fp32, GELU and the classifier's dot product in float64 (fp32 in the kernel:
2^-24 terms).  Every weight matrix of a tiny checkpoint holds bf16 values already, so `exact` and transformers see the matrices the tower stores.

Mutants of `model` (`mut=`, MUTANTS):
    k_minus_q          the index is taken at key - query
    p2c_query_row      the p2c term is read at the QUERY row of K Qr^T (p2c[q, idx] for K_q) instead of the key row
    scale_1            the softmax scale is 1 / sqrt(head_dim) instead of 1 / sqrt(3 head_dim)
    rel_not_normed     Kr / Qr are projected from the raw rel_embeddings (no encoder LayerNorm)
    clamp_2s           the index is clamped to 2 S instead of 2 S - 1, and row 2 S wraps to row 0
    kr_qr_swapped      c2p reads Qr, p2c reads Kr
    pooler_tanh        the pooler's GELU is a tanh
"""
import json
import math
import os
from dataclasses import dataclass, field
from typing import Dict, List, Optional

import torch

from tests import attention_ref as AR
from tests import encoder_ref as E
from tests.packed_text_ref import row_ratio      # noqa: F401

Tensor = torch.Tensor
F64 = torch.float64
SLICE = 64                 # queries per workgroup of csrc/attention_disentangled.hip
LDS_KEYS = 512             # keys of K + V its LDS holds next to the index offsets
MUTANTS = ("k_minus_q", "p2c_query_row", "scale_1", "rel_not_normed", "clamp_2s", "kr_qr_swapped", "pooler_tanh")


# ---- the index --------------------------------------------------------------------------------------------------------------------------------------
def transformers_idx(T: int, S: int, max_rel: int) -> Tensor:
    """[T, T] long: clamp(build_relative_position(...) + S, 0, 2 S - 1) from transformers' own function, entry [q, k]"""
    from transformers.models.deberta_v2.modeling_deberta_v2 import build_relative_position
    z = torch.zeros(T, 1)
    return (build_relative_position(z, z, bucket_size=S, max_position=max_rel)[0] + S).clamp(0, 2 * S - 1)


def pair_index(table: Tensor, ln: int, reach: int, device=None) -> Tensor:
    """[ln, ln] long: table[reach + (query - key)] of an idx_table(reach)"""
    pos = torch.arange(ln)
    return table.long()[reach + (pos[:, None] - pos[None, :])].to(device or table.device)


# ---- disentangled attention on raw bf16 inputs (the kernel's test) ----------------------------------------------------------------------------------------
def disentangled_scores(q, k, kr, qr, idx, scale):
    """[H, ln, hd] float64 q, k; [H, 2S, hd] float64 kr, qr; idx [ln, ln] long -> [H, ln, ln] float64 scores"""
    H, ln, _ = q.shape
    c2p = torch.gather(q @ kr.transpose(1, 2), 2, idx[None].expand(H, ln, ln))                  # [H, q, idx(q - k)]
    p2c = torch.gather(k @ qr.transpose(1, 2), 2, idx.T[None].expand(H, ln, ln)).transpose(1, 2)  # row k of K Qr^T at idx(q - k), laid out [q, k]
    return (q @ k.transpose(1, 2) + c2p + p2c) * scale


def disentangled_reference(qkv_bf16, lens, heads, hd, kr_bf16, qr_bf16, table, reach, scale):
    """float64 attention on the device of `qkv_bf16` -> (out, absout, scores) = (P V, P |V|) float64 [rows, heads hd] and the list of [H, ln, ln] score
    tensors; kr / qr bf16 [heads, 2 S, hd]; table = the int32 index table of `reach`"""
    W, dev, rows = heads * hd, qkv_bf16.device, qkv_bf16.shape[0]
    assert qkv_bf16.dtype == torch.bfloat16 and qkv_bf16.shape[1] == 3 * W and rows == sum(lens)
    out = torch.zeros(rows, W, dtype=F64, device=dev)
    absout = torch.zeros(rows, W, dtype=F64, device=dev)
    kr, qr = kr_bf16.double().to(dev), qr_bf16.double().to(dev)
    scores, r0 = [], 0
    for ln in lens:
        blk = qkv_bf16[r0:r0 + ln].double().reshape(1, ln, 3 * W)
        q, k, v = (AR._heads_of(t, heads, hd)[0] for t in blk.split(W, dim=2))
        s = disentangled_scores(q, k, kr, qr, pair_index(table.cpu(), ln, reach, dev), scale)
        p = torch.softmax(s, dim=-1)
        out[r0:r0 + ln] = (p @ v).transpose(0, 1).reshape(ln, W)
        absout[r0:r0 + ln] = (p @ v.abs()).transpose(0, 1).reshape(ln, W)
        scores.append(s)
        r0 += ln
    return out, absout, scores


# ---- tiny checkpoints ---------------------------------------------------------------------------------------------------------------------------------
_COMMON = dict(model_type="deberta-v2", architectures=["DebertaV2ForSequenceClassification"], vocab_size=320, num_hidden_layers=2, relative_attention=True,
               pos_att_type=["c2p", "p2c"], position_biased_input=False, norm_rel_ebd="layer_norm", type_vocab_size=0, layer_norm_eps=1e-7,
               hidden_act="gelu", pooler_hidden_act="gelu", max_relative_positions=-1, num_labels=1, id2label={"0": "LABEL_0"}, label2id={"LABEL_0": 0},
               pad_token_id=0, pooler_dropout=0.0, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
_W128 = dict(_COMMON, hidden_size=128, num_attention_heads=2, intermediate_size=256, pooler_hidden_size=128)
TINIES = {
    "S4_SHARE": dict(_W128, position_buckets=4, max_position_embeddings=16, share_att_key=True),
    "S4_SPLIT": dict(_W128, position_buckets=4, max_position_embeddings=16, share_att_key=False),
    "S8_SHARE": dict(_W128, position_buckets=8, max_position_embeddings=64, share_att_key=True),
    "S8_SPLIT": dict(_W128, position_buckets=8, max_position_embeddings=64, share_att_key=False),
    "W192_3H": dict(_COMMON, hidden_size=192, num_attention_heads=3, intermediate_size=320, pooler_hidden_size=192, position_buckets=8,
                    max_position_embeddings=64, share_att_key=True),      # F != 2 W, three heads
}
BATCHES = ([1, 2, 64, 65, 130], [17, 100, 5])      # identity, log and clamped buckets all occur within 130 tokens at both (S, max_pos) settings
MAX_LEN = 1024                                     # the reach the test towers are built for (the 700-token sequence fits)
HEAD_GAIN = 3.0


def hf_model(cfg: dict, seed: int = 0):
    """transformers' DebertaV2ForSequenceClassification for the config dict, fp32, eval, with seeded working magnitudes: LayerNorm weights 1 + 0.1 N(0, 1),
    every bias 0.1 N(0, 1), the token table and rel_embeddings N(0, 1), Linear weights N(0, 0.6 / sqrt(in)) — query, key and the two position
    projections x 2, so that q . k, c2p and p2c (all three are products of LayerNorm-ed rows through such matrices: comparable by construction) decide
    together which keys a query reads — the classifier's row N(0, HEAD_GAIN / sqrt(W)).  Every matrix is rounded to bf16: what the tower stores."""
    from transformers import DebertaV2Config, DebertaV2ForSequenceClassification
    model = DebertaV2ForSequenceClassification(DebertaV2Config(**{k: v for k, v in cfg.items() if k != "architectures"})).eval()
    g = torch.Generator().manual_seed(7000 + seed)
    with torch.no_grad():
        for name, p in model.named_parameters():
            rn = torch.randn(p.shape, generator=g)
            if "LayerNorm.weight" in name:
                v = 1.0 + 0.1 * rn
            elif name.endswith(".bias"):
                v = 0.1 * rn
            elif "word_embeddings" in name or "rel_embeddings" in name:
                v = rn
            elif name == "classifier.weight":
                v = (rn * (HEAD_GAIN / math.sqrt(p.shape[1]))).to(torch.bfloat16).float()
            else:
                mul = 2.0 if any(s in name for s in ("query_proj", "key_proj", "value_proj", "attention.output.dense")) else 1.0
                v = (rn * (mul * 0.6 / math.sqrt(p.shape[1]))).to(torch.bfloat16).float()
            p.copy_(v)
    return model


def train_tokenizer(vocab_size: int):
    from tests.modernbert_ref import train_tokenizer as tt
    return tt(vocab_size)


def write_dir(directory, name: str = "S8_SHARE", seed: int = 0, tokenizer: bool = True, model_max_length: Optional[int] = None, **over):
    """config.json + model.safetensors (`deberta.*`, `pooler.*`, `classifier.*`) + tokenizer.json + tokenizer_config.json -> (config dict, the model)"""
    from tests.modernbert_ref import state_dict_of, write_checkpoint_dir
    cfg = dict(TINIES[name], **over)
    model = hf_model(TINIES[name], seed)
    write_checkpoint_dir(str(directory), cfg, state_dict_of(model), tokenizer=train_tokenizer(cfg["vocab_size"]) if tokenizer else None)
    if tokenizer and model_max_length is not None:
        p = os.path.join(str(directory), "tokenizer_config.json")
        with open(p) as f:
            j = json.load(f)
        j["model_max_length"] = int(model_max_length)
        with open(p, "w") as f:
            json.dump(j, f)
    return cfg, model


def random_seqs(lengths, vocab, seed=0):
    g = torch.Generator().manual_seed(9100 + seed)
    return [torch.randint(5, vocab, (n,), generator=g) for n in lengths]


# ---- the float64 pass -------------------------------------------------------------------------------------------------------------------------------
@dataclass
class Pass:
    blocks: List[Tensor]                 # the stream after every block, [rows, W] float64
    final: Tensor
    pooled: Tensor                       # the [CLS] rows, [nseq, W]
    logits: Tensor                       # [nseq]
    extra: Dict[str, Tensor] = field(default_factory=dict)


_FORM = E.Form("deberta")


def _gelu(x):
    return E._act(x, "gelu")


def _pos_tables(arch, sd: Dict[str, Tensor], l: int, normed: bool = True):
    """Kr, Qr float64 [H, 2 S, hd] of block l from the checkpoint's own tensors (the mutant that skips the encoder LayerNorm needs them again)"""
    W, S, H = arch.width, arch.span, arch.heads
    rel = sd["deberta.encoder.rel_embeddings.weight"].double()
    if normed:
        rel = torch.nn.functional.layer_norm(rel, (W,), sd["deberta.encoder.LayerNorm.weight"].double(), sd["deberta.encoder.LayerNorm.bias"].double(), arch.ln_eps)
    att = f"deberta.encoder.layer.{l}.attention.self."
    names = ("key_proj", "query_proj") if arch.share_att_key else ("pos_key_proj", "pos_query_proj")
    return tuple((rel @ sd[att + n + ".weight"].double().T + sd[att + n + ".bias"].double()).reshape(2 * S, H, W // H).transpose(0, 1) for n in names)


def _run(arch, tensors, ids, lens, rounds, layers, mut, hist, sd=None, reach=MAX_LEN - 1) -> Pass:
    assert mut is None or mut in MUTANTS
    dev = ids.device
    lens = [int(n) for n in lens]
    assert ids.dim() == 1 and ids.shape[0] == sum(lens) and min(lens) >= 1 and max(lens) <= reach + 1
    layers = arch.layers if layers is None else layers
    R = E._Round(_FORM if rounds else None)
    hist = hist if rounds else 0
    mm = lambda x, w: E._mm(x, w, hist)
    t = {k: v.double().to(dev) for k, v in tensors.items()}       # (the matrices hold bf16 values already: hf_model)
    W, H, hd, S, eps = arch.width, arch.heads, arch.head_dim, arch.span, arch.ln_eps
    table = arch.idx_table(reach)
    scale = 1.0 / math.sqrt((1.0 if mut == "scale_1" else 3.0) * hd)
    ln = lambda y, name: E._ln(y, t[name + ".weight"], t[name + ".bias"], eps)
    e = ln(t["word_embeddings.weight"][ids.long()], "emb_ln")
    x, h = R.f(e), R.b(e)
    streams: List[Tensor] = []
    for l in range(layers):
        p = f"layer.{l}."
        if mut == "rel_not_normed":
            kr, qr = (v.to(dev) for v in _pos_tables(arch, sd, l, normed=False))
        else:
            kr, qr = t[p + "pos_key"], t[p + "pos_query"]
        kr, qr = R.b(kr), R.b(qr)
        if mut == "kr_qr_swapped":
            kr, qr = qr, kr
        qkv = R.b(mm(h, t[p + "attn.qkv.weight"]) + t[p + "attn.qkv.bias"])
        a = torch.zeros(qkv.shape[0], W, dtype=F64, device=dev)
        r0 = 0
        for n in lens:
            blk = qkv[r0:r0 + n]
            q, k, v = (blk[:, i * W:(i + 1) * W].reshape(n, H, hd).transpose(0, 1) for i in range(3))
            idx = pair_index(table, n, reach, dev)
            if mut == "k_minus_q":
                idx = idx.T.contiguous()
            if mut == "clamp_2s":       # the unclamped bucket, clamped one row too far, wrapping
                from transformers.models.deberta_v2.modeling_deberta_v2 import build_relative_position
                z = torch.zeros(n, 1)
                raw = build_relative_position(z, z, bucket_size=S, max_position=arch.max_rel)[0] + S
                idx = (raw.clamp(0, 2 * S) % (2 * S)).to(dev)
            c2p = R.f(q @ kr.transpose(1, 2))                            # [H, n, 2S]: the fp32 strips
            p2c = R.f(k @ qr.transpose(1, 2))
            gi = idx[None].expand(H, n, n)
            c = torch.gather(c2p, 2, gi)
            if mut == "p2c_query_row":
                pc = torch.gather(p2c, 2, gi)                            # row QUERY of K Qr^T
            else:
                pc = torch.gather(p2c, 2, idx.T[None].expand(H, n, n)).transpose(1, 2)
            s = (q @ k.transpose(1, 2) + c + pc) * scale
            pr = torch.exp(s - s.max(-1, keepdim=True).values)
            o = (R.b(pr) @ v) / pr.sum(-1, keepdim=True)
            a[r0:r0 + n] = R.b(o).transpose(0, 1).reshape(n, W)
            r0 += n
        y = R.f(x + mm(a, t[p + "attn.o.weight"]) + t[p + "attn.o.bias"])
        nrm = ln(y, p + "attn_ln")
        x, h = R.f(nrm), R.b(nrm)
        f = R.b(_gelu(mm(h, t[p + "mlp.fc1.weight"]) + t[p + "mlp.fc1.bias"]))
        y = R.f(x + mm(f, t[p + "mlp.fc2.weight"]) + t[p + "mlp.fc2.bias"])
        nrm = ln(y, p + "mlp_ln")
        x, h = R.f(nrm), R.b(nrm)
        streams.append(x)
    first = torch.tensor([sum(lens[:i]) for i in range(len(lens))], device=dev)
    pooled = x[first]
    pre = R.f(mm(R.b(pooled), t["pooler.weight"]) + t["pooler.bias"])
    act = torch.tanh(pre) if mut == "pooler_tanh" else _gelu(pre)
    logits = act @ t["classifier.weight"].reshape(W) + t["classifier.bias"].reshape(())
    return Pass(blocks=streams, final=x, pooled=pooled, logits=logits)


def exact(arch, tensors, ids, lens, layers: Optional[int] = None, reach: int = MAX_LEN - 1) -> Pass:
    return _run(arch, tensors, ids, lens, False, layers, None, 0, reach=reach)


def model(arch, tensors, ids, lens, layers: Optional[int] = None, mut: Optional[str] = None, hist: int = 0, sd=None, reach: int = MAX_LEN - 1) -> Pass:
    return _run(arch, tensors, ids, lens, True, layers, mut, hist, sd=sd, reach=reach)


_built: Dict[str, dict] = {}


def build(name: str) -> dict:
    """the seeded checkpoint of TINIES[name]: dict(cfg, arch, hf = the transformers model, sd = its state dict, tensors = deberta_state_dict's output,
    batches = the two batches of packed sequences)"""
    if name not in _built:
        from marqo_amd.engine import archs, tower_weights as TW
        from tests.modernbert_ref import state_dict_of
        cfg = TINIES[name]
        arch = archs.deberta_arch_from_hf_config(cfg)
        hf = hf_model(cfg, seed=1 + list(TINIES).index(name))
        sd = state_dict_of(hf)
        _built[name] = dict(cfg=cfg, arch=arch, hf=hf, sd=sd, tensors=TW.deberta_state_dict(arch, sd),
                            batches=[random_seqs(b, cfg["vocab_size"], seed=3 + i) for i, b in enumerate(BATCHES)])
    return _built[name]


def scalar_ratio(got, ex, mo) -> float:
    """max |got - exact| / max |model - exact| over a vector of scalars (the logits): the stream bar's quantity for one number per sequence"""
    got, ex, mo = (torch.as_tensor(v, dtype=F64).cpu().reshape(-1) for v in (got, ex, mo))
    den = float((mo - ex).abs().max())
    num = float((got - ex).abs().max())
    return num / den if den > 0 else (0.0 if num == 0 else float("inf"))

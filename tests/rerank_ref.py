"""References, rounding budgets, float32 models with seeded faults and shared fixtures for the tests of text reranking (csrc/rerank.hip,
engine/rerank.py): tests/test_rerank_host.py, tests/test_rerank_gpu.py.  A plain helper module: nothing here calls the library.
u = 2**-24 throughout; half_ulp / ratio / the LayerNorm budget and model are rowops_ref's.

TYPED EMBEDDING (embed_tokens_typed_kernel).  Row r of sequence i, t = r - cu[i]:  x = (tok[id] + pos[t]) + type[ty]  in fp32, ids and type ids
clamped to their tables, then the two-pass LayerNorm of rowops_ref (ln_normalize_row, affine contracted to an fma).  Reference: the float64 sum
and the float64 LayerNorm of it.  The two additions round once each:  e_j = u (|tok + pos| + |x|).  An input error e moves a LayerNorm output by
g_j / sigma' (e_j - mean(e) - d_j (d . e) / (W sigma'^2)), and |d . e| / W <= sigma rms(e) (Cauchy-Schwarz), so
    P_j = |g_j| / sigma' (|e_j| + mean|e| + |d_j| rms(e) / sigma')
    B_j = 1.01 B_ln,j + P_j        B_ln = rowops_ref.reference_ln's budget at the exact sum; the 1 % covers evaluating it there instead of at the
                                   rounded sum (its terms move by O(u) relative).

HEAD (mq_score_head: mq_cast_bf16 -> mq_gemm_bf16(BIAS | OUT_F32) -> score_tail_kernel).  Reference: float64 on hb = RN_bf16(h) and on the bf16
pooler weights as stored (what gemm_ref does: the operands' rounding is the format, not an error of the kernel).
    p = hb Wp^T + bp       B_p = K u sum_k |hb_k Wp_jk| + u |p|                 gemm_ref: K fp32 additions in any order, one for the bias
    y = tanh(p)            B_y = B_p + 2 TANH_ULP u |y|                         tanh is 1-Lipschitz; tanhf is the device library's accurate one,
                                                                                 TANH_ULP = 5 (the OpenCL C bound its math library is built to)
    z = wc . y + bc        B_z = sum_j |wc_j| B_y,j + D u (sum_j |wc_j y_j| + |bc|)   D = W / 64 + 7: a lane's chain of W / 64 fmas, six butterfly
                                                                                 levels, the add of the bias
    s = 1 / (1 + exp(-z))  B_s = B_z / 4 + 12 u s + 1e-30                       sigmoid' <= 1 / 4; ds = s (1 - s) rel(exp): expf 3 ulp = 6 u, the add
                                                                                 u, the division 2.5 ulp = 5 u; the floor covers an overflowing exp
MODEL.  float32 numpy models of both (model_embed, model_head) with single faults: FAULTS_EMBED, FAULTS_HEAD.
"""
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rowops_ref as R  # noqa: E402

U = 2.0 ** -24
TANH_ULP = 5
FAULTS_EMBED = ("type_row_zero", "type_from_neighbour")
FAULTS_HEAD = ("no_tanh", "no_cls_bias", "prev_cls_row")


def _f64(a):
    return np.asarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=np.float64)


def _f32(a):
    return np.asarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=np.float32)


def _rows(ids, tids, cu, vocab, type_vocab):
    ids, tids, cu = (np.asarray(v, dtype=np.int64) for v in (ids, tids, cu))
    seq = np.searchsorted(cu, np.arange(cu[-1]), side="right") - 1
    return np.clip(ids, 0, vocab - 1), np.clip(tids, 0, type_vocab - 1), np.arange(cu[-1]) - cu[seq]


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def embed_case(W, lens, vocab=97, max_pos=80, type_vocab=2, seed=0, mixed=True):
    """tables and packed ids of unrelated random values; type ids 0 for the first part of a sequence, 1 after it (mixed), or all 0"""
    g = np.random.default_rng(1000 * seed + W)
    c = dict(tok=g.standard_normal((vocab, W)).astype(np.float32) * 0.5, pos=g.standard_normal((max_pos, W)).astype(np.float32) * 0.3,
             typ=g.standard_normal((type_vocab, W)).astype(np.float32) * 0.3, g=(1 + 0.1 * g.standard_normal(W)).astype(np.float32),
             b=(0.05 * g.standard_normal(W)).astype(np.float32), eps=1e-12)
    cu = np.zeros(len(lens) + 1, dtype=np.int32)
    np.cumsum(lens, out=cu[1:])
    c["cu"] = cu
    c["ids"] = g.integers(0, vocab, int(cu[-1])).astype(np.int32)
    tids = np.zeros(int(cu[-1]), dtype=np.int32)
    if mixed:
        for i, n in enumerate(lens):
            tids[cu[i] + (n + 1) // 2:cu[i + 1]] = 1
    c["tids"] = tids
    return c


def head_case(W, n, seed=0):
    """x fp32 [rows, W] (sequences of 1 .. 3 rows, unrelated rows), pooler (bf16 values) and classifier"""
    g = np.random.default_rng(2000 * seed + 7 * W + n)
    lens = 1 + (np.arange(n) % 3)
    cu = np.zeros(n + 1, dtype=np.int32)
    np.cumsum(lens, out=cu[1:])
    return dict(x=g.standard_normal((int(cu[-1]), W)).astype(np.float32), cu=cu,
                Wp=R.round_bf16(g.standard_normal((W, W)).astype(np.float32) / math.sqrt(W)), bp=(0.1 * g.standard_normal(W)).astype(np.float32),
                wc=(3.0 / math.sqrt(W) * g.standard_normal(W)).astype(np.float32), bc=0.37)


# ---- references and budgets ------------------------------------------------------------------------------------------------------------
def embed_reference(c):
    """(y, B): float64 [rows, W]"""
    W = c["tok"].shape[1]
    ids, tids, t = _rows(c["ids"], c["tids"], c["cu"], c["tok"].shape[0], c["typ"].shape[0])
    tp = _f64(c["tok"])[ids] + _f64(c["pos"])[t]
    x = tp + _f64(c["typ"])[tids]
    e = U * (np.abs(tp) + np.abs(x))
    y, B = R.reference_ln(torch.from_numpy(x), torch.from_numpy(_f32(c["g"])), torch.from_numpy(_f32(c["b"])), c["eps"])
    mu = x.mean(-1, keepdims=True)
    d = x - mu
    sp = np.sqrt((d * d).mean(-1, keepdims=True) + c["eps"])
    P = np.abs(_f64(c["g"]))[None, :] / sp * (e + e.mean(-1, keepdims=True) + np.abs(d) * np.sqrt((e * e).mean(-1, keepdims=True)) / sp)
    assert x.shape[1] == W
    return y.numpy(), 1.01 * B.numpy() + P


def head_reference(c):
    """(z, B_z, s, B_s): float64 [n]"""
    W = c["x"].shape[1]
    hb = R.round_bf16(_f32(c["x"])[np.asarray(c["cu"][:-1], dtype=np.int64)]).astype(np.float64)
    Wp, wc = _f64(c["Wp"]), _f64(c["wc"])
    p = hb @ Wp.T + _f64(c["bp"])
    Bp = W * U * (np.abs(hb) @ np.abs(Wp).T) + U * np.abs(p)
    y = np.tanh(p)
    By = Bp + 2 * TANH_ULP * U * np.abs(y)
    z = y @ wc + c["bc"]
    D = W // 64 + 7
    Bz = By @ np.abs(wc) + D * U * (np.abs(y) @ np.abs(wc) + abs(c["bc"]))
    s = 1.0 / (1.0 + np.exp(-z))
    return z, Bz, s, Bz / 4 + 12 * U * s + 1e-30


def ratio(got, ref, bound):
    return R.ratio(torch.from_numpy(np.asarray(got, dtype=np.float64)), torch.from_numpy(np.asarray(ref, dtype=np.float64)),
                   torch.from_numpy(np.asarray(bound, dtype=np.float64)))


# ---- float32 models ---------------------------------------------------------------------------------------------------------------------
def model_embed(c, fault=None):
    assert fault is None or fault in FAULTS_EMBED
    ids, tids, t = _rows(c["ids"], c["tids"], c["cu"], c["tok"].shape[0], c["typ"].shape[0])
    if fault == "type_row_zero":
        tids = np.zeros_like(tids)
    elif fault == "type_from_neighbour":
        tids = tids[np.minimum(np.arange(tids.size) + 1, tids.size - 1)]
    x = (_f32(c["tok"])[ids] + _f32(c["pos"])[t]) + _f32(c["typ"])[tids]
    return R.model_layernorm(x, c["g"], c["b"], c["eps"], form="generic", fma=True)[0]


def _fma(a, b, s):
    return (a.astype(np.float64) * b.astype(np.float64) + s.astype(np.float64)).astype(np.float32)


def model_head(c, fault=None):
    """(z, s) float32 [n]"""
    assert fault is None or fault in FAULTS_HEAD
    W = c["x"].shape[1]
    rows = np.asarray(c["cu"][:-1], dtype=np.int64)
    if fault == "prev_cls_row":
        rows = np.concatenate((rows[:1], rows[:-1]))
    hb = R.round_bf16(_f32(c["x"])[rows])
    p = hb @ _f32(c["Wp"]).T + _f32(c["bp"])
    y = p if fault == "no_tanh" else np.tanh(p)
    wc = _f32(c["wc"])
    acc = np.zeros((rows.size, 64), np.float32)
    for i in range(W // 64):
        acc = _fma(np.broadcast_to(wc[i * 64:(i + 1) * 64], acc.shape), y[:, i * 64:(i + 1) * 64], acc)
    z = R._butterfly(acc)
    if fault != "no_cls_bias":
        z = z + np.float32(c["bc"])
    with np.errstate(over="ignore"):
        return z, np.float32(1) / (np.float32(1) + np.exp(-z))


# ---- shared fixtures: a tiny WordPiece vocabulary, texts, synthetic checkpoint directories -------------------------------------------------
_SYL = [c + v for c in "bdfgklmnprstvz" for v in "aeiou"]
WORDS = [a + b for a in _SYL[:24] for b in _SYL[30:42]]                     # 288 lower-case words, each one piece
VOCAB = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]", *WORDS, "##s", "##ing", ".", ",", "?", "!"]
SHAPES = {"tinybert": dict(W=128, layers=2, heads=2, mlp=512), "minilm": dict(W=384, layers=6, heads=12, mlp=1536)}


def write_vocab(directory):
    p = os.path.join(str(directory), "vocab.txt")
    with open(p, "w", encoding="utf-8") as f:
        f.write("\n".join(VOCAB) + "\n")
    return p


def words(n, seed):
    g = np.random.default_rng(seed)
    return " ".join(WORDS[int(i)] for i in g.integers(0, len(WORDS), n))


def sentences(n_words, seed):
    """text of n_words words with a full stop every 5 words and the odd plural (a second piece)"""
    g = np.random.default_rng(seed)
    out = []
    for k in range(n_words):
        w = WORDS[int(g.integers(0, len(WORDS)))] + ("s" if g.integers(0, 5) == 0 else "")
        out.append((w.capitalize() if k % 5 == 0 else w) + ("." if k % 5 == 4 or k == n_words - 1 else ""))
    return " ".join(out)


def write_cross_encoder_dir(directory, shape, seed=0, equal_type_rows=False):
    """a local Hugging Face BertForSequenceClassification directory of synthetic weights -> its state dict"""
    from safetensors.torch import save_file
    from marqo_amd.engine import synthetic
    s = SHAPES[shape]
    os.makedirs(str(directory), exist_ok=True)
    sd = synthetic.cross_encoder_state_dict(s["W"], s["layers"], s["heads"], s["mlp"], vocab=len(VOCAB), seed=seed)
    if equal_type_rows:
        t = sd["bert.embeddings.token_type_embeddings.weight"]
        t[1] = t[0]
    save_file({k: v.contiguous() for k, v in sd.items()}, os.path.join(str(directory), "model.safetensors"))
    cfg = dict(architectures=["BertForSequenceClassification"], model_type="bert", vocab_size=len(VOCAB), hidden_size=s["W"],
               num_hidden_layers=s["layers"], num_attention_heads=s["heads"], intermediate_size=s["mlp"], max_position_embeddings=512,
               type_vocab_size=2, hidden_act="gelu", layer_norm_eps=1e-12, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1,
               position_embedding_type="absolute", pad_token_id=0, id2label={"0": "LABEL_0"}, label2id={"LABEL_0": 0}, num_labels=1)
    with open(os.path.join(str(directory), "config.json"), "w") as f:
        json.dump(cfg, f)
    with open(os.path.join(str(directory), "tokenizer_config.json"), "w") as f:
        json.dump(dict(do_lower_case=True, model_max_length=512, tokenizer_class="BertTokenizer"), f)
    write_vocab(directory)
    return sd


def fast_tokenizer(directory):
    from transformers import BertTokenizerFast
    return BertTokenizerFast.from_pretrained(str(directory), do_lower_case=True)     # (reads the directory's vocab.txt)


def hf_logits(directory, query, docs, max_length):
    """transformers.BertForSequenceClassification in fp32 on the CPU, fed as CrossEncoder.predict feeds it -> float64 [n]"""
    from transformers import BertForSequenceClassification
    model = BertForSequenceClassification.from_pretrained(str(directory), torch_dtype=torch.float32).eval()
    enc = fast_tokenizer(directory)([query.strip()] * len(docs), [d.strip() for d in docs], truncation="longest_first", max_length=max_length,
                                    padding=True, return_tensors="pt")
    with torch.no_grad():
        return model(**enc).logits[:, 0].double().numpy()

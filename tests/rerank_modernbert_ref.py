"""Reference, rounding budget, float32 model with seeded faults and fixtures for the tests of ModernBERT cross-encoders (csrc/rerank.hip
mq_score_head_ln / mq_score_pairs_modernbert, engine/rerank.py ModernBertCrossEncoderTower): tests/test_rerank_modernbert_host.py,
tests/test_rerank_modernbert_gpu.py.  A plain helper module: nothing here calls the library.  u = 2**-24; the LayerNorm budget, the butterfly and
the bf16 rounding are rowops_ref's, the construction is rerank_ref's.

HEAD (mq_score_head_ln: mq_cast_bf16 -> mq_gemm_bf16(BIAS | GELU | OUT_F32) -> score_tail_ln_kernel).  Reference: float64 on hb = RN_bf16(h) and on
the bf16 dense weights as stored (the operands' rounding is the format, not an error of the kernel), with the exact erf GELU.
    p = hb Wd^T + bd        B_p = W u sum_k |hb_k Wd_jk| + u |p|            W fp32 additions in any order, one for the bias (a head without a dense
                                                                            bias adds zeros: exact)
    a = gelu(p)             B_a = 1.13 B_p + GELU_ABS + GELU_REL |p|        |gelu'| <= 1.13.  The epilogue's GELU is common.h's gelu_erf2: x * (0.5 +
                                                                            xc Q(xc^2)), xc = clamp(x, +-4.5), a degree-8 polynomial in Horner form —
                                                                            an approximation of the function, so no ulp bound can be derived for it.
                                                                            GELU_ABS / GELU_REL are MEASURED (below) on `gelu_device`, the same fp32
                                                                            operations in numpy, against float64 erf.
    n = LN(a) g + b         an input error e moves n_j by  P_j = |g_j| / sigma' (|e_j| + mean|e| + |d_j| rms(e) / sigma')   (rerank_ref: typed embedding)
                            B_n = 1.01 B_ln + P                             B_ln = rowops_ref.reference_ln's budget at the exact a: a lane's chain of
                                                                            W / 64 elements, six butterfly levels and the divide are its D; the 1 %
                                                                            covers evaluating it at the exact row instead of the rounded one
    z = wc . n + bc         B_z = sum_j |wc_j| B_n,j + D u (sum_j |wc_j n_j| + |bc|)    D = W / 64 + 7: a lane's chain of W / 64 fmas, six butterfly
                                                                            levels, the add of the bias.  This is the LayerNorm's sensitivity
                                                                            rstd |g_j wc_j| folded into one bound on the logit.
    s = 1 / (1 + exp(-z))   B_s = B_z / 4 + 12 u s + 1e-30                  as rerank_ref
MODEL.  model_head_ln: float32 numpy model of the kernel (lane c holds columns c, c + 64, ...; two-pass variance; fma chains), with single faults
FAULTS_HEAD_LN.
"""
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rowops_ref as R  # noqa: E402
from tests import modernbert_ref as M  # noqa: E402

U = 2.0 ** -24
# MEASURED once on the CPU (measure_gelu() below, 2e6 points, |x| <= GELU_RANGE): worst |gelu_device(x) - gelu_float64(x)| for |x| <= 4.5 is
# 6.76e-05 (the polynomial's fit error); beyond the clamp the kernel's Phi stays at Phi(+-4.5), worst |error| / |x| = 3.29e-06.  Recorded with a
# margin of 5 %.  tests/test_rerank_modernbert_host.py::test_gelu_constants_are_the_measurement measures again and compares.
GELU_RANGE = 64.0
GELU_ABS = 7.1e-05
GELU_REL = 3.5e-06
GELU_LIP = 1.13
HEAD_NONZERO = 16
FAULTS_HEAD_LN = ("no_gelu", "ln_no_mean", "no_norm_bias", "no_cls_bias", "prev_row")


def _f64(a):
    return np.asarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=np.float64)


def _f32(a):
    return np.asarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=np.float32)


def _fma(a, b, s):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(s, np.float64)).astype(np.float32)


# ---- GELU ---------------------------------------------------------------------------------------------------------------------------------------
_Q = (3.036425686e-11, -3.314666682e-09, 1.590999455e-07, -4.451734438e-06, 8.142522511e-05, -1.037591685e-03, 9.585204319e-03, -6.598465809e-02,
      3.987126077e-01)


def gelu_device(x):
    """common.h gelu_erf2 in float32 numpy: the same operations in the same order (median clamp, one product, eight fmas, one fma, one product)"""
    x = _f32(x)
    xc = np.clip(x, np.float32(-4.5), np.float32(4.5))
    s = xc * xc
    q = np.full_like(x, np.float32(_Q[0]))
    for c in _Q[1:]:
        q = _fma(q, s, np.float32(c))
    return x * _fma(xc, q, np.float32(0.5))


def gelu_f64(x):
    x = torch.from_numpy(np.asarray(x, dtype=np.float64))
    return (0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))).numpy()


def measure_gelu(points=2_000_000):
    """(worst |error| for |x| <= 4.5, worst |error| / |x| for 4.5 < |x| <= GELU_RANGE) of gelu_device against float64"""
    x = np.linspace(-GELU_RANGE, GELU_RANGE, points).astype(np.float32)
    x = np.concatenate((x, np.linspace(-4.5, 4.5, points).astype(np.float32)))
    err = np.abs(gelu_device(x).astype(np.float64) - gelu_f64(x.astype(np.float64)))
    inside = np.abs(x) <= 4.5
    return float(err[inside].max()), float((err[~inside] / np.abs(x[~inside].astype(np.float64))).max())


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------------
def head_case(W, n, seed=0, dense_bias=True, norm_bias=True, offset=0.0):
    """pooled rows h fp32 [n, W] (unrelated rows), dense (bf16 values) (+ bias), LayerNorm weight (+ bias), classifier.  offset: a common value added
    to the dense bias, so that every column of a row of `a` sits at about `offset` (mean >> spread: what a one-pass variance gets wrong)"""
    g = np.random.default_rng(3000 * seed + 11 * W + n)
    # 16 non-zero weights per output column, at random inputs: the accumulation bound W u sum|hb Wd| is a worst case over W coherent terms, and with a
    # dense random matrix (sum|t| ~ sqrt(W) |p|) it grows to half the spread of the logits at W = 2048 — no fault of the head could exceed it
    Wd = np.zeros((W, W), np.float32)
    for j in range(W):
        Wd[j, g.choice(W, HEAD_NONZERO, replace=False)] = g.standard_normal(HEAD_NONZERO) / math.sqrt(HEAD_NONZERO)
    c = dict(h=g.standard_normal((n, W)).astype(np.float32), Wd=R.round_bf16(Wd),
             bd=(0.1 * g.standard_normal(W) + offset).astype(np.float32), g=(1 + 0.1 * g.standard_normal(W)).astype(np.float32),
             b=g.standard_normal(W).astype(np.float32), wc=(3.0 / math.sqrt(W) * g.standard_normal(W)).astype(np.float32), bc=0.37, eps=1e-5)
    if not dense_bias:
        c["bd"] = None
    if not norm_bias:
        c["b"] = None
    return c


# ---- reference and budget ---------------------------------------------------------------------------------------------------------------------------
def head_f64(h, Wd, bd, g, b, wc, bc, eps):
    """the head in float64 on the values as given (no operand rounding): -> logits [n]"""
    p = _f64(h) @ _f64(Wd).T + (0.0 if bd is None else _f64(bd))
    a = gelu_f64(p)
    mu = a.mean(-1, keepdims=True)
    d = a - mu
    nrm = d / np.sqrt((d * d).mean(-1, keepdims=True) + eps) * _f64(g) + (0.0 if b is None else _f64(b))
    return nrm @ _f64(wc).reshape(-1) + float(bc)


def _logit_budget(x, Wd, bd, g, b, wc, bc, eps, d_ln, d_dot, gelu_abs, gelu_rel):
    """(z, B_z) float64 [n] of the head on the float64 values x [n, W]: the docstring's chain with the LayerNorm's chain length d_ln (rowops_ref's D),
    the classifier's d_dot and the GELU's error gelu_abs + gelu_rel |p|"""
    W = x.shape[1]
    p = x @ Wd.T + (0.0 if bd is None else bd)
    Bp = W * U * (np.abs(x) @ np.abs(Wd).T) + U * np.abs(p)
    a = gelu_f64(p)
    e = GELU_LIP * Bp + gelu_abs + gelu_rel * np.abs(p)
    mu = a.mean(-1, keepdims=True)
    d = a - mu
    sp = np.sqrt((d * d).mean(-1, keepdims=True) + eps)
    y = d / sp * g + b
    c = d_ln * U * np.abs(a).mean(-1, keepdims=True)                       # rowops_ref.reference_ln's budget, with its D as a parameter
    rho = (d_ln / 2 + 4) * U + c * c / (2 * sp * sp)
    Bln = np.abs(g) / sp * (c + 2 * U * np.abs(d)) + np.abs(g * d) / sp * rho + 2 * U * np.abs(y)
    P = np.abs(g)[None, :] / sp * (e + e.mean(-1, keepdims=True) + np.abs(d) * np.sqrt((e * e).mean(-1, keepdims=True)) / sp)
    Bn = 1.01 * Bln + P
    z = y @ wc + bc
    return z, Bn @ np.abs(wc) + d_dot * U * (np.abs(y) @ np.abs(wc) + abs(bc)), p


def head_reference(c):
    """(z, B_z, s, B_s): float64 [n], the kernel's budget"""
    W = c["h"].shape[1]
    hb = R.round_bf16(_f32(c["h"])).astype(np.float64)
    z, Bz, p = _logit_budget(hb, _f64(c["Wd"]), None if c["bd"] is None else _f64(c["bd"]), _f64(c["g"]), np.zeros(W) if c["b"] is None else _f64(c["b"]),
                             _f64(c["wc"]), float(c["bc"]), c["eps"], R.chain(W), W // 64 + 7, GELU_ABS, GELU_REL)
    assert np.abs(p).max() <= GELU_RANGE, "the dense layer's output leaves the range the GELU constants were measured on"
    s = 1.0 / (1.0 + np.exp(-z))
    return z, Bz, s, Bz / 4 + 12 * U * s + 1e-30


def fp32_reference(h, Wd, bd, g, b, wc, bc, eps):
    """(z, B_z) of ANY fp32 evaluation of the head on the fp32 values as given (no operand rounding): every sum of K terms within K u sum|terms|
    (d_ln = W, d_dot = W + 1), an fp32 erf GELU within 4 u |p| (the cancellation of 1 + erf for negative p included) — the bound transformers' own
    head on the CPU is held to"""
    W = h.shape[1]
    z, Bz, _ = _logit_budget(_f64(h), _f64(Wd), None if bd is None else _f64(bd), _f64(g), np.zeros(W) if b is None else _f64(b), _f64(wc).reshape(-1),
                             float(bc), eps, W, W + 1, 0.0, 4 * U)
    return z, Bz


def ratio(got, ref, bound):
    return R.ratio(torch.from_numpy(np.asarray(got, dtype=np.float64)), torch.from_numpy(np.asarray(ref, dtype=np.float64)),
                   torch.from_numpy(np.asarray(bound, dtype=np.float64)))


# ---- float32 model ------------------------------------------------------------------------------------------------------------------------------------
def model_head_ln(c, fault=None):
    """(z, s) float32 [n]: the kernel's arithmetic, with ONE deliberate fault (FAULTS_HEAD_LN):
      no_gelu        the dense layer's pre-activation goes to the LayerNorm
      ln_no_mean     the LayerNorm does not subtract the mean (neither from the row nor inside the variance)
      no_norm_bias   head.norm.bias is not added
      no_cls_bias    classifier.bias is not added
      prev_row       pair i reads the pooled row of pair i - 1"""
    assert fault is None or fault in FAULTS_HEAD_LN
    n, W = c["h"].shape
    rows = np.arange(n)
    if fault == "prev_row":
        rows = np.concatenate((rows[:1], rows[:-1]))
    hb = R.round_bf16(_f32(c["h"])[rows])
    p = hb @ _f32(c["Wd"]).T + (np.float32(0) if c["bd"] is None else _f32(c["bd"]))
    a = p if fault == "no_gelu" else gelu_device(p)
    nc = W // 64
    col = lambda t, i: t[..., i * 64:(i + 1) * 64]
    s = np.zeros((n, 64), np.float32)
    for i in range(nc):
        s = s + col(a, i)
    mean = (R._butterfly(s) / np.float32(W))[:, None]
    if fault == "ln_no_mean":
        mean = np.zeros_like(mean)
    s2 = np.zeros((n, 64), np.float32)
    for i in range(nc):
        d = col(a, i) - mean
        s2 = _fma(d, d, s2)
    rstd = (np.float32(1) / np.sqrt(R._butterfly(s2) / np.float32(W) + np.float32(c["eps"])))[:, None].astype(np.float32)
    gam, wc = _f32(c["g"]), _f32(c["wc"])
    bet = np.zeros(W, np.float32) if c["b"] is None or fault == "no_norm_bias" else _f32(c["b"])
    acc = np.zeros((n, 64), np.float32)
    for i in range(nc):
        y = _fma((col(a, i) - mean) * rstd, np.broadcast_to(col(gam, i), (n, 64)), np.broadcast_to(col(bet, i), (n, 64)))
        acc = _fma(y, np.broadcast_to(col(wc, i), (n, 64)), acc)
    z = R._butterfly(acc)
    if fault != "no_cls_bias":
        z = z + np.float32(c["bc"])
    with np.errstate(over="ignore"):
        return z, np.float32(1) / (np.float32(1) + np.exp(-z))


# ---- a ModernBertForSequenceClassification directory as a user brings it ------------------------------------------------------------------------------
MAX_POS = 512      # (TINY serves 256 positions; the long pair of the GPU test has 300 tokens)
HEAD_GAIN = 3.0    # classifier.weight ~ N(0, HEAD_GAIN / sqrt(W)): reference logits of standard deviation ~1 and more over unrelated pairs


def classifier_config(pooling="cls", **over):
    return M.config_dict(max_position_embeddings=MAX_POS, num_labels=1, id2label={"0": "LABEL_0"}, label2id={"LABEL_0": 0}, classifier_pooling=pooling,
                         architectures=["ModernBertForSequenceClassification"], **over)


def hf_classifier(cfg: dict, seed: int = 0):
    """transformers' ModernBertForSequenceClassification for the config dict: eager attention, fp32, eval; modernbert_ref.randomize's weights, the
    classifier's row scaled to HEAD_GAIN, the optional biases 0.1 / 0.3 N(0, 1), classifier.bias 0.37"""
    from transformers import ModernBertConfig, ModernBertForSequenceClassification
    kw = {k: v for k, v in cfg.items() if k not in ("model_type", "architectures")}
    config = ModernBertConfig(**kw)
    config._attn_implementation = "eager"
    model = ModernBertForSequenceClassification(config).float().eval()
    M.randomize(model, seed)
    g = torch.Generator().manual_seed(5000 + seed)
    W = config.hidden_size
    with torch.no_grad():
        model.classifier.weight.copy_(torch.randn(1, W, generator=g) * (HEAD_GAIN / math.sqrt(W)))
        model.classifier.bias.fill_(0.37)
        for name, p in model.named_parameters():
            if name.endswith(".bias") and p.ndim == 1 and not name.startswith("classifier."):
                p.copy_((0.1 if "dense" in name else 0.3) * torch.randn(p.shape, generator=g))
    return model


def write_cross_encoder_dir(directory, pooling="cls", seed=0, tokenizer=True, drop=(), **over):
    """config.json + model.safetensors (`model.*`, `head.*`, `classifier.*`) + tokenizer.json + tokenizer_config.json -> (config dict, the model)"""
    cfg = classifier_config(pooling, **over)
    model = hf_classifier(cfg, seed)
    sd = {k: v for k, v in M.state_dict_of(model).items() if k not in drop}
    M.write_checkpoint_dir(str(directory), cfg, sd, tokenizer=M.train_tokenizer(cfg["vocab_size"]) if tokenizer else None)
    return cfg, model


WORDS = " ".join(M.CORPUS).replace(",", " ").replace(".", " ").split()


def sentence(n_words, seed):
    g = np.random.default_rng(seed)
    return " ".join(WORDS[int(i)] for i in g.integers(0, len(WORDS), n_words))


def pair_encodings(directory, query, docs, max_length):
    """the `tokenizers` library's own pair encoding of (query, doc): [CLS] q [SEP] d [SEP] with longest_first truncation -> list of id lists"""
    from tokenizers import Tokenizer
    from tokenizers.processors import TemplateProcessing
    tk = Tokenizer.from_file(os.path.join(str(directory), "tokenizer.json"))
    cls_id, sep_id = tk.token_to_id("[CLS]"), tk.token_to_id("[SEP]")
    tk.post_processor = TemplateProcessing(single="[CLS] $A [SEP]", pair="[CLS] $A [SEP] $B:0 [SEP]:0", special_tokens=[("[CLS]", cls_id), ("[SEP]", sep_id)])
    tk.no_padding()
    tk.enable_truncation(max_length=int(max_length), strategy="longest_first")
    return [e.ids for e in tk.encode_batch([(query.strip(), d.strip()) for d in docs], add_special_tokens=True)]


def hf_logits(model, encodings):
    """transformers' model in fp32 on the CPU on the given id lists, one pair at a time (no padding anywhere) -> float64 [n]"""
    out = []
    with torch.no_grad():
        for ids in encodings:
            t = torch.tensor([ids], dtype=torch.long)
            out.append(float(model(input_ids=t, attention_mask=torch.ones_like(t)).logits[0, 0]))
    return np.asarray(out, dtype=np.float64)


def read_json(path):
    with open(path) as f:
        return json.load(f)

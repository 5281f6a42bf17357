"""References, rounding budgets and shared fixtures for the tests of OWL-ViT image reranking (csrc/owl_head.hip, engine/owl.py,
s2_inference/reranking): tests/test_owl_host.py, tests/test_owl_gpu.py, tests/test_owl_shapes_gpu.py.  A plain helper module: nothing here calls the library.
u = 2**-24 throughout; reference_ln / half_ulp_bf16 / ratio are rowops_ref's.  All references are float64 NumPy on the exact input values.

MERGE + LAYERNORM (owl_merge_ln_kernel).  c = LN(x_0; post), p = LN(x_j; post), m = p c, f = LN(m; ln).  B_c, B_p: rowops_ref.reference_ln's
budget of the two-pass LayerNorm.  The product rounds once:  e_m = |p| B_c + |c| B_p + B_p B_c + u |m|.  An input error e moves a LayerNorm
output by g_j / sigma' (e_j - mean(e) - d_j (d . e) / (W sigma'^2)) and |d . e| / W <= sigma rms(e), so
    P_j = |g_j| / sigma' (|e_j| + mean|e| + |d_j| rms(e) / sigma')          B_f = 1.01 B_ln(m) + P      (+ half a bf16 ulp for the bf16 copy)
(the 1 % covers evaluating B_ln at the exact m instead of the rounded one, as in rerank_ref).

CLASS HEAD (owl_class_head_kernel), per row, D1 = ceil(Dq / 64) + 7, D2 = ceil(W / 64) + 7 (a lane's fma chain, six butterfly levels, one spare):
    |e|^2, |t|^2   positive terms: relative D1 u; the root halves it; sqrtf, the add of 1e-6f and the reciprocal one u each:  rn = (D1 / 2 + 3) u
    dot            B_dot = D1 u sum|e_j t_j|
    z = dot / ((|e| + 1e-6f)(|t| + 1e-6f))     B_z = B_dot / (ne nt) + |z| (2 rn + 3 u)
    shift, pre = f . w + b                     B_lin = D2 u (sum|f_j w_j| + |b|)
    scale = ELU(pre) + 1                       B_scale = B_lin + 6 u (|ELU(pre)| + 1)        ELU is 1-Lipschitz; expm1f 4 ulp, the add one
    logit = (z + shift) scale                  B = 1.01 ((B_z + B_shift + u |z + shift|) |scale| + |z + shift| B_scale) + u |logit|
    max over the queries                       B_max = max_q B_q (max is 1-Lipschitz in the sup norm); a masked query is exactly -FLT_MAX
    score = 1 / (1 + exp(-max))                B_s = B_max / 4 + 12 u s + 1e-30              as rerank_ref's sigmoid
    label                                      asserted where the best logit leads the second by more than their two budgets

BOX HEAD (owl_box_head_kernel), on the hidden rows' bf16 values as the GEMM's GELU epilogue stores them (the format, not an error).  z_o = h . w2_o + b2_o + bias_o:  B_z = (D2 + 2) u (sum|h_j w_j| + |b2| + |bias|);  s = sigmoid(z):  B_s = B_z / 4 +
12 u s;  x0 = (s_0 - s_2 / 2) t_w (and the three others alike):  B = (B_s0 + B_s2 / 2) t + 3 u (|s_0| + |s_2| / 2) t.

TOP-K.  Exact: np.argsort(-score, kind="stable") (ties to the lower patch), the scores and box rows copied bit for bit.
"""
import json
import math
import os
import sys
import zlib

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rowops_ref as R  # noqa: E402

U = 2.0 ** -24
EPS6 = float(np.float32(1e-6))
FLT_MIN_LOGIT = -float(np.finfo(np.float32).max)
CLIP_MEAN, CLIP_STD = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)
# name -> image, patch, vision / text width, heads, layers, MLP width.  The query dimension is the text width: the class head's dense0 maps
# to text_config.hidden_size and its rows meet text embeddings of projection_dim columns, so OwlViTForObjectDetection needs the two equal.
SHAPES = {"g3": dict(image=96, patch=32, W=128, heads=2, layers=2, mlp=256), "g5": dict(image=160, patch=32, W=128, heads=2, layers=2, mlp=256),
          # google/owlvit-base-patch32's geometry with one layer per encoder (P = 576, T = 577, Dq = 512): the chain at a served checkpoint's widths
          "b32x1": dict(image=768, patch=32, W=768, heads=12, layers=1, mlp=3072, text_W=512, text_heads=8, text_mlp=2048)}
TOY_SHAPES = ("g3", "g5")
CTX = 16


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64)))


def _ln(x, g, b, eps):
    """(y, B) float64 numpy: rowops_ref.reference_ln on fp32 affine values"""
    y, B = R.reference_ln(_t(x), _t(g), _t(b), eps)
    return y.numpy(), B.numpy()


def _ln_push(x, g, e, eps):
    """how far an elementwise input error e can move LayerNorm(x; g)"""
    mu = x.mean(-1, keepdims=True)
    d = x - mu
    sp = np.sqrt((d * d).mean(-1, keepdims=True) + eps)
    return np.abs(g)[None, :] / sp * (e + e.mean(-1, keepdims=True) + np.abs(d) * np.sqrt((e * e).mean(-1, keepdims=True)) / sp)


# ---- references and budgets ------------------------------------------------------------------------------------------------------------------
def merge_ln_reference(x, n, T, post_g, post_b, ln_g, ln_b, eps):
    """x [n T, W] -> (feats, B) float64 [n (T - 1), W]"""
    x = np.asarray(x, dtype=np.float64).reshape(n, T, -1)
    W = x.shape[-1]
    y, B = _ln(x.reshape(n * T, W), post_g, post_b, eps)
    y, B = y.reshape(n, T, W), B.reshape(n, T, W)
    c, Bc, p, Bp = y[:, :1], B[:, :1], y[:, 1:], B[:, 1:]
    m = (p * c).reshape(-1, W)
    e = (np.abs(p) * Bc + np.abs(c) * Bp + Bp * Bc).reshape(-1, W) + U * np.abs(m)
    f, Bf = _ln(m, ln_g, ln_b, eps)
    return f, 1.01 * Bf + _ln_push(m, np.asarray(ln_g, dtype=np.float64), e, eps)


def class_head_reference(e, f, t, mask, shift_w, shift_b, scale_w, scale_b, P):
    """e [rows, Dq] (dense0's output), f [rows, W], t [Q, Dq] or [n, Q, Dq], mask like t's leading dims or None
    -> dict(logits [rows, Q], B [rows, Q], best, B_best, score, B_score, label, label_sure) float64 / int"""
    e, f, t = (np.asarray(v, dtype=np.float64) for v in (e, f, t))
    rows, Dq = e.shape
    W = f.shape[1]
    n = rows // P
    if t.ndim == 2:
        t = np.broadcast_to(t, (n, *t.shape))
        mask = None if mask is None else np.broadcast_to(np.asarray(mask), (n, t.shape[1]))
    tq = np.repeat(t, P, axis=0)                                  # [rows, Q, Dq]
    D1, D2 = math.ceil(Dq / 64) + 7, math.ceil(W / 64) + 7
    ne, nt = np.sqrt((e * e).sum(-1)) + EPS6, np.sqrt((tq * tq).sum(-1)) + EPS6
    dot = np.einsum("rd,rqd->rq", e, tq)
    Bdot = D1 * U * np.einsum("rd,rqd->rq", np.abs(e), np.abs(tq))
    z = dot / (ne[:, None] * nt)
    rn = (D1 / 2 + 3) * U
    Bz = Bdot / (ne[:, None] * nt) + np.abs(z) * (2 * rn + 3 * U)
    sw, cw = np.asarray(shift_w, dtype=np.float64), np.asarray(scale_w, dtype=np.float64)
    shift, pre = f @ sw + shift_b, f @ cw + scale_b
    Bshift, Bpre = D2 * U * (np.abs(f) @ np.abs(sw) + abs(shift_b)), D2 * U * (np.abs(f) @ np.abs(cw) + abs(scale_b))
    elu = np.where(pre > 0, pre, np.expm1(np.minimum(pre, 0)))
    scale, Bscale = elu + 1, Bpre + 6 * U * (np.abs(elu) + 1)
    zs = z + shift[:, None]
    logits = zs * scale[:, None]
    B = 1.01 * ((Bz + Bshift[:, None] + U * np.abs(zs)) * np.abs(scale)[:, None] + np.abs(zs) * Bscale[:, None]) + U * np.abs(logits)
    if mask is not None:
        dead = np.repeat(np.asarray(mask) == 0, P, axis=0)
        logits, B = np.where(dead, FLT_MIN_LOGIT, logits), np.where(dead, 0.0, B)
    label = logits.argmax(-1)
    best = logits.max(-1)
    Bbest = B.max(-1)
    if logits.shape[1] > 1:
        order = np.sort(logits, axis=-1)
        sure = order[:, -1] - order[:, -2] > 2 * Bbest
    else:
        sure = np.ones(rows, dtype=bool)
    with np.errstate(over="ignore"):
        score = 1.0 / (1.0 + np.exp(-best))
    return dict(logits=logits, B=B, best=best, B_best=Bbest, score=score, B_score=Bbest / 4 + 12 * U * score + 1e-30, label=label, label_sure=sure,
                pre=pre)


def box_head_reference(h, w2, b2, bias, P, target):
    """h [rows, W], w2 [4, W], b2 [4], bias [P, 4], target (w, h) -> (pred cxcywh [rows, 4], boxes [rows, 4], B [rows, 4]) float64"""
    h, w2, b2, bias = (np.asarray(v, dtype=np.float64) for v in (h, w2, b2, bias))
    rows, W = h.shape
    D2 = math.ceil(W / 64) + 7
    bb = np.tile(bias, (rows // P, 1))
    z = h @ w2.T + b2[None, :] + bb
    Bz = (D2 + 2) * U * (np.abs(h) @ np.abs(w2).T + np.abs(b2)[None, :] + np.abs(bb))
    s = 1.0 / (1.0 + np.exp(-z))
    Bs = Bz / 4 + 12 * U * s
    tw, th = float(target[0]), float(target[1])
    sc = np.array([tw, th, tw, th])
    boxes = np.stack([s[:, 0] - s[:, 2] / 2, s[:, 1] - s[:, 3] / 2, s[:, 0] + s[:, 2] / 2, s[:, 1] + s[:, 3] / 2], axis=1) * sc
    half = np.stack([Bs[:, 0] + Bs[:, 2] / 2, Bs[:, 1] + Bs[:, 3] / 2] * 2, axis=1)
    mag = np.stack([s[:, 0] + s[:, 2] / 2, s[:, 1] + s[:, 3] / 2] * 2, axis=1)
    return s, boxes, (half + 3 * U * mag) * sc


def topk_reference(score, boxes, k):
    """score [n, P], boxes [n, P, 4] -> (scores [n, k], boxes [n, k, 4], patch [n, k]) with k clamped to P; NaN sorts last"""
    score, boxes = np.asarray(score), np.asarray(boxes)
    k = min(k, score.shape[1])
    key = np.where(np.isnan(score), -np.inf, score)
    idx = np.argsort(-key, axis=1, kind="stable")[:, :k]
    return np.take_along_axis(score, idx, 1), np.take_along_axis(boxes, idx[:, :, None], 1), idx.astype(np.int32)


def box_bias_reference(grid):
    """compute_box_bias as the model evaluates it, in float32 (at a coordinate of 1 the float32 log1p(-1 + 1e-4) is 1.7e-4 away from the
    float64 one: the constant is the model's, not an error of anybody's) -> float64 [grid * grid, 4] of those float32 values"""
    c = torch.arange(1, grid + 1, dtype=torch.float32) / grid
    xx, yy = torch.meshgrid(c, c, indexing="xy")
    xy = torch.clip(torch.stack((xx, yy), dim=-1).view(-1, 2), 0.0, 1.0)
    size = torch.full_like(xy, 1.0) / grid
    return torch.cat([torch.log(xy + 1e-4) - torch.log1p(-xy + 1e-4), torch.log(size + 1e-4) - torch.log1p(-size + 1e-4)], dim=-1).double().numpy()


def gelu(x):
    return 0.5 * x * (1.0 + np.vectorize(math.erf)(x / math.sqrt(2.0)))


def heads_reference(sd, hidden, query_embeds, mask, target, eps=1e-5):
    """the whole of what follows the encoders, float64 on fp32 weights: hidden [n, T, W] = the vision model's last_hidden_state, query_embeds
    [Q, Dq] -> dict(logits [n, P, Q], pred_boxes [n, P, 4] (cxcywh in 0..1), best [n, P], score [n, P], boxes [n, P, 4] in target pixels)"""
    w = lambda k: sd[k].detach().double().numpy()
    hidden = np.asarray(hidden, dtype=np.float64)
    n, T, W = hidden.shape
    P = T - 1
    f, _ = merge_ln_reference(hidden.reshape(n * T, W), n, T, w("owlvit.vision_model.post_layernorm.weight"), w("owlvit.vision_model.post_layernorm.bias"),
                              w("layer_norm.weight"), w("layer_norm.bias"), eps)
    e = f @ w("class_head.dense0.weight").T + w("class_head.dense0.bias")
    c = class_head_reference(e, f, query_embeds, mask, w("class_head.logit_shift.weight")[0], float(w("class_head.logit_shift.bias")[0]),
                             w("class_head.logit_scale.weight")[0], float(w("class_head.logit_scale.bias")[0]), P)
    h = gelu(gelu(f @ w("box_head.dense0.weight").T + w("box_head.dense0.bias")) @ w("box_head.dense1.weight").T + w("box_head.dense1.bias"))
    pred, boxes, _ = box_head_reference(h, w("box_head.dense2.weight"), w("box_head.dense2.bias"), box_bias_reference(int(round(math.sqrt(P)))), P, target)
    Q = c["logits"].shape[1]
    return dict(logits=c["logits"].reshape(n, P, Q), pred_boxes=pred.reshape(n, P, 4), best=c["best"].reshape(n, P), score=c["score"].reshape(n, P),
                boxes=boxes.reshape(n, P, 4), pre=c["pre"].reshape(n, P))


def ratio(got, ref, bound):
    return R.ratio(_t(got), _t(ref), _t(bound))


# ---- shared fixtures: a tiny CLIP BPE vocabulary, queries, images, synthetic checkpoint directories ------------------------------------------------
MERGES = [("c", "a"), ("ca", "t</w>"), ("d", "o"), ("do", "g</w>"), ("t", "h"), ("th", "e</w>"), ("o", "n</w>"), ("r", "e"), ("re", "d</w>")]
QUERY_SHORT = "the red cat on a dog"                       # 6 pieces: 8 tokens with SOT and EOT
QUERY_FULL = "a b c d e f g h i j k l m n"                 # 14 one-letter words: exactly 16 tokens
QUERY_LONG = QUERY_FULL + " o"                             # 17 tokens: refused


def write_tokenizer_files(directory):
    from marqo_amd.engine.tokenizers import _byte_to_unicode
    units = list(_byte_to_unicode().values())
    vocab = units + [u + "</w>" for u in units] + ["".join(m) for m in MERGES] + ["<|startoftext|>", "<|endoftext|>"]
    with open(os.path.join(str(directory), "vocab.json"), "w", encoding="utf-8") as f:
        json.dump({t: i for i, t in enumerate(vocab)}, f, ensure_ascii=False)
    with open(os.path.join(str(directory), "merges.txt"), "w", encoding="utf-8") as f:
        f.write("#version: 0.2\n" + "\n".join(" ".join(m) for m in MERGES) + "\n")
    return len(vocab)


def owl_config(shape):
    from transformers import OwlViTConfig
    s = SHAPES[shape]
    side = dict(hidden_size=s["W"], intermediate_size=s["mlp"], num_hidden_layers=s["layers"], num_attention_heads=s["heads"])
    text = dict(side, hidden_size=s.get("text_W", s["W"]), intermediate_size=s.get("text_mlp", s["mlp"]), num_attention_heads=s.get("text_heads", s["heads"]))
    vocab = 512 + len(MERGES) + 2
    return OwlViTConfig(text_config=dict(vocab_size=vocab, max_position_embeddings=CTX, bos_token_id=vocab - 2, eos_token_id=vocab - 1, pad_token_id=0,
                                         **text),
                        vision_config=dict(image_size=s["image"], patch_size=s["patch"], **side), projection_dim=text["hidden_size"])


def write_owl_dir(directory, shape, seed=0):
    """a local Hugging Face OwlViTForObjectDetection directory of seeded random weights.  Random-init heads give nearly constant (or saturated)
    outputs, so the heads are drawn here: unit-variance pre-activations, logit_scale's of both signs, box offsets of order one on the grid bias."""
    from transformers import OwlViTForObjectDetection
    os.makedirs(str(directory), exist_ok=True)
    torch.manual_seed(seed)
    model = OwlViTForObjectDetection(owl_config(shape)).eval()
    W = SHAPES[shape]["W"]
    Dq = SHAPES[shape].get("text_W", W)               # the text width = the projection = the query dimension
    g = torch.Generator().manual_seed(1000 + seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    with torch.no_grad():
        for name, p in model.named_parameters():       # encoders: wide enough that patches and queries differ after two blocks
            if "encoder.layers" in name and name.endswith("weight") and p.ndim == 2:
                p.copy_(rn(*p.shape) * (1.5 / math.sqrt(p.shape[1])))
            elif "encoder.layers" in name and name.endswith("bias") and "layer_norm" not in name:
                p.copy_(rn(*p.shape) * 0.1)
        model.owlvit.vision_model.embeddings.patch_embedding.weight.copy_(rn(W, 3, 32, 32) * 0.03)
        model.owlvit.vision_model.embeddings.position_embedding.weight.copy_(rn(*model.owlvit.vision_model.embeddings.position_embedding.weight.shape) * 0.3)
        model.owlvit.vision_model.embeddings.class_embedding.copy_(rn(W))
        model.owlvit.text_model.embeddings.token_embedding.weight.copy_(rn(*model.owlvit.text_model.embeddings.token_embedding.weight.shape))
        model.owlvit.text_model.embeddings.position_embedding.weight.copy_(rn(CTX, Dq) * 0.3)
        model.owlvit.text_projection.weight.copy_(rn(Dq, Dq) / math.sqrt(Dq))
        for ln in (model.owlvit.vision_model.pre_layernorm, model.owlvit.vision_model.post_layernorm, model.layer_norm, model.owlvit.text_model.final_layer_norm):
            ln.weight.copy_(1 + 0.1 * rn(ln.weight.shape[0]))
            ln.bias.copy_(0.1 * rn(ln.weight.shape[0]))
        ch, bh = model.class_head, model.box_head
        ch.dense0.weight.copy_(rn(Dq, W) / math.sqrt(W))
        ch.dense0.bias.copy_(0.1 * rn(Dq))
        ch.logit_shift.weight.copy_(rn(1, W) * (0.5 / math.sqrt(W)))
        ch.logit_shift.bias.fill_(-0.2)
        ch.logit_scale.weight.copy_(rn(1, W) * (1.5 / math.sqrt(W)))
        ch.logit_scale.bias.fill_(0.4)
        for lin in (bh.dense0, bh.dense1):
            lin.weight.copy_(rn(W, W) * (1.4 / math.sqrt(W)))
            lin.bias.copy_(0.1 * rn(W))
        bh.dense2.weight.copy_(rn(4, W) * (2.0 / math.sqrt(W)))
        bh.dense2.bias.copy_(torch.tensor([0.3, -0.3, 0.2, -0.2]))
    model.save_pretrained(str(directory), safe_serialization=True)
    write_tokenizer_files(directory)
    return model


def images(n, seed, size=(240, 240)):
    """n Pillow RGB images of `size` = (w, h): smooth colour fields with a bright blob at a place of its own, plus noise"""
    from PIL import Image
    g = np.random.default_rng(seed)
    w, h = size
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    out = []
    for i in range(n):
        cx, cy, r = g.uniform(0.1, 0.9) * w, g.uniform(0.1, 0.9) * h, g.uniform(0.08, 0.25) * min(w, h)
        base = np.stack([127 + 90 * np.sin(xx / w * g.uniform(2, 9) + g.uniform(0, 6)) * np.cos(yy / h * g.uniform(2, 9) + c) for c in range(3)], -1)
        blob = np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * r * r))[..., None] * g.uniform(-120, 120, 3)
        out.append(Image.fromarray(np.clip(base + blob + g.normal(0, 12, (h, w, 3)), 0, 255).astype(np.uint8), "RGB"))
    return out


def pixel_values(pil_images, S):
    """OwlViTImageProcessorPil at the model's size: Pillow bicubic squash to S x S, / 255, CLIP mean and std -> fp32 [n, 3, S, S]"""
    from transformers.models.owlvit.image_processing_pil_owlvit import OwlViTImageProcessorPil
    proc = OwlViTImageProcessorPil(size={"height": S, "width": S})
    return proc(images=list(pil_images), return_tensors="pt")["pixel_values"]


def hf_forward(model, ids, pix, target):
    """transformers' OwlViTForObjectDetection in fp32 on the CPU, one image at a time as the reference runs it; ids int64 [Q, 16] zero-padded
    -> dict(logits [n, P, Q], pred_boxes, best, score, boxes (corner format in target = (w, h) pixels), hidden [n, T, W], query_embeds [Q, Dq])"""
    from transformers.image_transforms import center_to_corners_format
    ids = torch.as_tensor(np.asarray(ids), dtype=torch.long)
    out = dict(logits=[], pred_boxes=[], hidden=[])
    with torch.no_grad():
        for i in range(pix.shape[0]):
            o = model(input_ids=ids, pixel_values=pix[i:i + 1], attention_mask=(ids > 0).long())
            out["logits"].append(o.logits[0])
            out["pred_boxes"].append(o.pred_boxes[0])
            out["hidden"].append(o.vision_model_output[0][0])
            q = o.text_embeds[0]
    r = {k: torch.stack(v).double().numpy() for k, v in out.items()}
    best = torch.stack(out["logits"]).max(-1).values
    tw, th = float(target[0]), float(target[1])
    r["best"], r["score"] = best.double().numpy(), torch.sigmoid(best).double().numpy()
    r["boxes"] = (center_to_corners_format(torch.stack(out["pred_boxes"])) * torch.tensor([tw, th, tw, th])).double().numpy()
    r["query_embeds"] = q.double().numpy()
    return r


def load_hf(directory):
    from transformers import OwlViTForObjectDetection
    return OwlViTForObjectDetection.from_pretrained(str(directory), torch_dtype=torch.float32).eval()


# ---- fixtures of the kernel tests at the served shapes (tests/test_owl_shapes_gpu.py runs them, tests/test_owl_host.py checks their premises) -----------
TOPK_P = (255, 256, 257, 576, 8191)                 # one below / at / one above one trip of the 256 threads, owlvit-base-patch32's, the limit
TOPK_KINDS = ("distinct", "ties", "nan")
TIE_VALUES = (0.0, 0.25, 0.5, 0.75, 1.0)            # a saturated sigmoid gives exactly 0.0f and 1.0f
NAN_BITS = (0x7FC00000, 0xFFC00000, 0x7FC00001, 0x7F800001, 0xFFFFFFFF)          # quiet, negative, with payload, signalling, all ones


def topk_ks(P):
    return sorted({min(k, P) for k in (1, 7, 256, 257, P)})


def topk_nan_patches(P):
    return sorted({0, 255, 256, P - 1} & set(range(P)))


def topk_fixture(kind, P):
    """score fp32 [3, P], boxes fp32 [3, P, 4].
    distinct: a permutation of P different values per image, the maximum moved to patch 0 / patch 256 (P // 2 where there is none) / patch P - 1.
    ties:     five values only, so nearly every rank is decided by the lower-patch rule; patch 0 and patch 256 hold the same value where both exist.
    nan:      image 0 distinct with NaNs (different bit patterns) at patches 0, 255, 256 and P - 1; image 1 all NaN; image 2 ties with a NaN in every
              seventh patch."""
    g = np.random.default_rng(P * 10 + TOPK_KINDS.index(kind))
    boxes = g.uniform(0, 240, (3, P, 4)).astype(np.float32)
    distinct = np.stack([(g.permutation(P) + 0.5) / (P + 1) for _ in range(3)]).astype(np.float32)
    for img, at in enumerate((0, 256 if P > 256 else P // 2, P - 1)):
        top = int(distinct[img].argmax())
        distinct[img, [at, top]] = distinct[img, [top, at]]
    ties = np.asarray(TIE_VALUES, dtype=np.float32)[g.integers(0, len(TIE_VALUES), (3, P))]
    if P > 256:
        ties[:, 256] = ties[:, 0]
    if kind == "distinct":
        return distinct, boxes
    if kind == "ties":
        return ties, boxes
    nan = lambda m: np.resize(np.asarray(NAN_BITS, dtype=np.uint32), m).view(np.float32)
    score = np.stack([distinct[0], nan(P), ties[2]])
    where = topk_nan_patches(P)
    score[0, where] = nan(len(where))
    score[2, ::7] = nan(len(score[2, ::7]))
    return score, boxes


MERGE_W = (4, 260, 768, 1024, 1280, 1536, 2048)     # MQ_DISPATCH_CH: CH = 1, 2 (one live lane in the second chunk), 3, 4, 6 via case 5, 6 via case 6, 8
MERGE_NT = ((1, 2), (3, 4))                         # one patch row; 9 rows: not a multiple of the 4 rows of a block
MERGE_CASES = [(n, T, W) for W in MERGE_W for n, T in MERGE_NT] + [(2, 577, 768)]
MERGE_CONST = 0.7                                   # the constant patch row's value: not a dyadic number, so its computed mean is a rounded one


def merge_fixture(n, T, W):
    """x fp32 [n T, W] and the two LayerNorms' (weight, bias): random rows of spread 0.3 .. 3 and mean -1 .. 1; image 0's class row has a mean 50 x its
    spread; the last patch row of the last image is constant where there is more than one patch row (index: merge_const_row)."""
    g = np.random.default_rng(100 * n + T + W)
    x = (g.standard_normal((n * T, W)) * g.uniform(0.3, 3.0, (n * T, 1)) + g.uniform(-1, 1, (n * T, 1))).astype(np.float32)
    z = g.standard_normal(W)
    x[0] = (0.5 * ((z - z.mean()) / z.std() + 50.0)).astype(np.float32)          # (the sample's own mean and spread: 50 at every W)
    if n * (T - 1) > 1:
        x[n * T - 1] = np.float32(MERGE_CONST)
    pg, lg = ((1 + 0.2 * g.standard_normal(W)).astype(np.float32) for _ in range(2))
    pb, lb = ((0.2 * g.standard_normal(W)).astype(np.float32) for _ in range(2))
    return x, pg, pb, lg, lb


def merge_const_row(n, T):
    """the output row of merge_fixture's constant patch row, or None"""
    return n * (T - 1) - 1 if n * (T - 1) > 1 else None


# (n, P, W, Dq, Q, per_image, tie): the query limit at owlvit-base-patch32's and owlvit-large-patch14's widths, and widths ragged against the 64 lanes
CLASS_CASES = {"base_q8": (2, 61, 768, 512, 8, 0, None), "base_q8_tie": (2, 61, 768, 512, 8, 0, (2, 5)), "large_q8_masked": (2, 61, 1024, 768, 8, 1, None),
               "ragged": (3, 7, 100, 70, 5, 1, None)}


def class_fixture(name):
    """dict(e, f, t, mask, sw, sb, cw, cb, n, P, W, Dq, Q, per_image, tie) of CLASS_CASES[name].  Row 3 of e is zero (a zero-norm embedding).  The
    masked case keeps only query 7 in image 0 and only query 0 in image 1.  tie = (a, b): query row b is a copy of query row a."""
    n, P, W, Dq, Q, per_image, tie = CLASS_CASES[name]
    g = np.random.default_rng(zlib.crc32(name.encode()))
    rows = n * P
    e = g.standard_normal((rows, Dq)).astype(np.float32)
    e[3] = 0.0
    f = g.standard_normal((rows, W)).astype(np.float32)
    t = g.standard_normal((n, Q, Dq) if per_image else (Q, Dq)).astype(np.float32)
    if tie:
        t[..., tie[1], :] = t[..., tie[0], :]
    mask = None
    if name == "large_q8_masked":
        mask = np.zeros((n, Q), dtype=np.int32)
        mask[0, 7] = mask[1, 0] = 1
    sw, cw = (g.standard_normal(W) / np.sqrt(W)).astype(np.float32), (1.5 * g.standard_normal(W) / np.sqrt(W)).astype(np.float32)
    return dict(e=e, f=f, t=t, mask=mask, sw=sw, sb=-0.2, cw=cw, cb=0.4, n=n, P=P, W=W, Dq=Dq, Q=Q, per_image=per_image, tie=tie)


def class_reference(fx):
    return class_head_reference(fx["e"], fx["f"], fx["t"], fx["mask"], fx["sw"], np.float32(fx["sb"]), fx["cw"], np.float32(fx["cb"]), fx["P"])


def sure_apart_from_twin(ref, twin):
    """label_sure with query column `twin` (an exact copy of another query) left out: the best logit leads every OTHER query by more than 2 B"""
    z = np.delete(ref["logits"], twin, axis=1)
    order = np.sort(z, axis=-1)
    return order[:, -1] - order[:, -2] > 2 * ref["B_best"]


BOX_TARGET = (320, 200)                             # not square: a swapped width and height shows
BOX_CASES = {"grid24": (2, 24, 768, False), "grid7": (2, 7, 1024, False), "grid3_ragged": (3, 3, 100, False), "grid24_same_rows": (2, 24, 768, True)}


def box_fixture(name):
    """dict(h (bf16 values in fp32) [n P, W], w2 [4, W], b2 [4], n, grid, P, W) of BOX_CASES[name].  same_rows: every row of h is one vector, scaled so
    that h . w2 stays of order one half: the rows then differ through the grid bias alone, and no sigmoid saturates."""
    n, grid, W, same = BOX_CASES[name]
    P = grid * grid
    g = np.random.default_rng(zlib.crc32(name.encode()))
    w2 = (2.0 * g.standard_normal((4, W)) / np.sqrt(W)).astype(np.float32)
    b2 = np.array([0.3, -0.3, 0.2, -0.2], dtype=np.float32)
    if same:
        h = np.tile(R.round_bf16((0.25 * np.abs(g.standard_normal((1, W)))).astype(np.float32)), (n * P, 1))
    else:
        h = R.round_bf16(np.abs(g.standard_normal((n * P, W))).astype(np.float32))
    return dict(h=h, w2=w2, b2=b2, n=n, grid=grid, P=P, W=W)


# the chain at owlvit-base-patch32's widths: 8 queries, the fourth empty (masked), the others from the tiny vocabulary
CHAIN_QUERIES = [QUERY_SHORT, "a cat", "the dog", "", "red", QUERY_FULL, "cat on the dog", "a red dog on a cat"]


def fake_detection(pixels_u8, P=9):
    """the injected detector of the plumbing tests: fixed scores [P] (all different) and boxes [P, 4] in the 240 x 240 working image, drawn
    from the image's own bytes"""
    g = np.random.default_rng(zlib.crc32(np.ascontiguousarray(pixels_u8, dtype=np.uint8).tobytes()))
    scores = (g.permutation(P) + g.uniform(0.1, 0.9, P)).astype(np.float32) / np.float32(P)
    xy = g.uniform(0, 120, (P, 2))
    boxes = np.concatenate([xy, xy + g.uniform(10, 120, (P, 2))], axis=1).astype(np.float32)
    return scores, boxes

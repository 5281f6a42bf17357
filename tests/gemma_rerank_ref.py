"""Helpers of the Gemma reranker tests (tests/test_gemma_rerank_host.py, tests/test_gemma_rerank_gpu.py).  Nothing here calls the library.

  - the float64 restatement of causal / prefix-sharing grouped-query attention at 256-wide heads with the softmax scale as an argument and two switchable
    faults (one future key admitted, the last prefix key dropped, for ONE query), on the layout and the budget of tests/qwen_ref.py /
    tests/attention_ref.py (imported, not changed), and a tile-order arithmetic model of csrc/attention_gqa256_causal.hip;
  - tiny seeded `GemmaForCausalLM` / `GemmaForSequenceClassification` models of transformers and their own float64 score of a whole per-pair sequence;
  - the plain-Python restatement of the input rows and a checkpoint directory as a user brings it (the tokenizer is tests/gemma_ref.py's)."""
import json
import os

import torch

from tests import gemma_ref as G
from tests import qwen_ref as Q

HD = 256
NW = 8              # waves per workgroup of the kernel
PIECE_KEYS = 128    # keys (two 64-key tiles) the LDS holds at 512-byte rows
PROMPT = ("Given a query A and a passage B, determine whether the passage contains an answer to the query by providing a prediction of either 'Yes' or "
          "'No'.")


# ---- attention in float64 -------------------------------------------------------------------------------------------------------------------------------
def prefix_reference(qkv_bf16, P, lens, q_heads, kv_heads, hd=HD, scale=None, fault=None):
    """float64 prefix attention on the device of `qkv_bf16` [P + sum(lens), (Q + 2 KV) hd]: rows [0, P) are the prefix, the segments follow; P = 0 is
    plain causal attention on the packed batch -> (out, absout) = (P V, P |V|), float64 [P + sum(lens), Q hd]; the prefix rows stay 0.
    fault = (kind, segment, t): the reference is WRONG for query t of that segment — "future": it also sees own key t + 1; "drop_prefix": it does not
    see prefix key P - 1."""
    Qh, KV, G_ = q_heads, kv_heads, q_heads // kv_heads
    dev, rows = qkv_bf16.device, qkv_bf16.shape[0]
    assert qkv_bf16.dtype == torch.bfloat16 and rows == P + sum(lens) and qkv_bf16.shape[1] == (Qh + 2 * KV) * hd
    scale = hd ** -0.5 if scale is None else scale
    out = torch.zeros(rows, Qh * hd, dtype=torch.float64, device=dev)
    absout = torch.zeros_like(out)
    _, pk, pv = Q.split_qkv(qkv_bf16[:P].double(), Qh, KV, hd)
    kvh = torch.arange(Qh, device=dev) // G_
    r0 = P
    for i, ln in enumerate(lens):
        q, k, v = Q.split_qkv(qkv_bf16[r0:r0 + ln].double(), Qh, KV, hd)
        k, v = torch.cat([pk, k], dim=1)[kvh], torch.cat([pv, v], dim=1)[kvh]                     # [Q, P + ln, hd]
        t = torch.arange(ln, device=dev)
        ok = torch.cat([torch.ones(ln, P, dtype=torch.bool, device=dev), t[None, :] <= t[:, None]], dim=1)
        if fault is not None and fault[1] == i:
            if fault[0] == "future":
                ok[fault[2], P + fault[2] + 1] = True
            elif fault[0] == "drop_prefix":
                ok[fault[2], P - 1] = False
            else:
                raise ValueError(fault)
        p = torch.softmax((q @ k.transpose(1, 2) * scale).masked_fill(~ok, float("-inf")), dim=-1)
        out[r0:r0 + ln] = (p @ v).transpose(0, 1).reshape(ln, Qh * hd)
        absout[r0:r0 + ln] = (p @ v.abs()).transpose(0, 1).reshape(ln, Qh * hd)
        r0 += ln
    return out, absout


def blocks_per_slice(G_):
    """16-query blocks of a slice of csrc/attention_gqa256_causal.hip: as many as one round of eight waves holds"""
    return 1 if G_ >= 8 else 8 // G_


def emulate_prefix(qkv_bf16, P, lens, q_heads, kv_heads, hd=HD, scale=None):
    """torch-CPU model of csrc/attention_gqa256_causal.hip's arithmetic in the kernel's order: per (segment, query head, 16-query block) the virtual key
    tiles — ceil(P / 64) prefix tiles (keys >= P of the last one masked), then the own tiles up to the block's last query (the diagonal one masked per
    key: key <= q, key < len) — in ascending order; attention_ref.emulate's softmax (fp32 raw scores, running max from -1e30, probabilities rounded to
    bf16 for P.V but summed unrounded, alpha rescale, o / l stored as bf16).  Keys past a range are copies of its last key.  The prefix rows stay 0."""
    Qh, KV, G_ = q_heads, kv_heads, q_heads // kv_heads
    x = qkv_bf16.cpu()
    out = torch.zeros(x.shape[0], Qh * hd, dtype=torch.bfloat16)
    scale = hd ** -0.5 if scale is None else scale
    c = torch.tensor(1.44269504088896340736, dtype=torch.float32) * torch.tensor(scale, dtype=torch.float32)
    npt = (P + 63) // 64
    if P:
        _, pk, pv = Q.split_qkv(x[:P].float(), Qh, KV, hd)
        pidx = torch.arange(npt * 64).clamp(max=P - 1)
        pk, pv = pk[:, pidx], pv[:, pidx]
    r0 = P
    for ln in lens:
        q, k, v = Q.split_qkv(x[r0:r0 + ln].float(), Qh, KV, hd)
        nkt = (ln + 63) // 64
        kidx = torch.arange(nkt * 64).clamp(max=ln - 1)
        k, v = k[:, kidx], v[:, kidx]
        for h in range(Qh):
            src = h // G_
            for qb0 in range(0, ln, 16):
                nq = min(16, ln - qb0)
                qi = torch.arange(qb0, qb0 + nq)[:, None]
                qq = q[h, qb0:qb0 + nq]
                m = torch.full((nq, 1), -1e30, dtype=torch.float32)
                l = torch.zeros(nq, 1, dtype=torch.float32)
                o = torch.zeros(nq, hd, dtype=torch.float32)
                last = min((qb0 + 15) // 64, (min(qb0 + 15, ln - 1)) // 64)
                for kt in list(range(npt)) + [npt + j for j in range(last + 1)]:
                    key = torch.arange(64)[None, :]
                    if kt < npt:
                        kk, vv = pk[src, kt * 64:kt * 64 + 64], pv[src, kt * 64:kt * 64 + 64]
                        valid = (kt * 64 + key < P).expand(nq, 64)
                    else:
                        j = kt - npt
                        kk, vv = k[src, j * 64:j * 64 + 64], v[src, j * 64:j * 64 + 64]
                        valid = (j * 64 + key < ln) & (j * 64 + key <= qi)
                    st = (qq @ kk.t()).masked_fill(~valid, float("-inf"))
                    m_new = torch.maximum(m, st.max(dim=-1, keepdim=True).values)
                    p = torch.exp2(st * c - m_new * c)
                    pb = p.to(torch.bfloat16).float()
                    alpha = torch.exp2((m - m_new) * c)
                    l = l * alpha + p.sum(-1, keepdim=True)
                    o = o * alpha + pb @ vv
                    m = m_new
                out[r0 + qb0:r0 + qb0 + nq, h * hd:(h + 1) * hd] = (o * (1.0 / l)).to(torch.bfloat16)
        r0 += ln
    return out


def loud_key_inputs(P, lens, q_heads, kv_heads, seg, t, seed=0, device="cpu"):
    """`randn` inputs in which, for query t of segment `seg` (query head 0), the first future key (own key t + 1) and the last prefix key (P - 1) are
    LOUD: each K row is 2 x that query's q (score 2 |q|^2 / 16, about 32 against N(0, 1) elsewhere) and its V row is + 100 (the future key) or - 100 (the prefix
    key) — the true output is about - 100, admitting the one gives about 0 and dropping the other the quiet keys' mean, against a budget of 2**-8 x
    about 200."""
    qkv = Q.make_gqa_qkv("randn", [P] + list(lens), q_heads, kv_heads, HD, seed=seed, device="cpu").clone()
    s0 = P + sum(lens[:seg])
    qv = qkv[s0 + t, :HD].float()
    kcol, vcol = q_heads * HD, (q_heads + kv_heads) * HD
    for row, loud in ((s0 + t + 1, 100.0), (P - 1, -100.0)):
        qkv[row, kcol:kcol + HD] = (2.0 * qv).to(torch.bfloat16)
        qkv[row, vcol:vcol + HD] = loud
    return qkv.to(device)


# ---- tiny models ------------------------------------------------------------------------------------------------------------------------------------------
_COMMON = dict(model_type="gemma", vocab_size=300, hidden_size=256, num_hidden_layers=2, head_dim=256, intermediate_size=512, max_position_embeddings=512,
               rms_norm_eps=1e-6, hidden_act="gelu_pytorch_tanh", hidden_activation="gelu_pytorch_tanh", attention_bias=False, tie_word_embeddings=False,
               pad_token_id=0, eos_token_id=1, bos_token_id=2, rope_parameters={"rope_type": "default", "rope_theta": 10000.0})
TINY81 = dict(_COMMON, num_attention_heads=8, num_key_value_heads=1)      # the checkpoint's group: 8 query heads over one K/V head; attention width 2048
TINY21 = dict(_COMMON, num_attention_heads=2, num_key_value_heads=1)      # attention width 512
TINIES = {"TINY81": TINY81, "TINY21": TINY21}


def hf_reranker(cfg: dict, kind: str, seed: int = 0, gain: float = 0.6):
    """transformers' GemmaForCausalLM (kind "lm") / GemmaForSequenceClassification with one label (kind "cls") for the config dict: eager attention,
    float64, eval, weights from gemma_ref.randomize (norm weights 0.1 N(0, 1), applied as 1 + w; lm_head / score included)"""
    import transformers
    kw = {k: v for k, v in cfg.items() if k not in ("model_type", "architectures", "hidden_activation")}
    if kind == "cls":
        kw.update(num_labels=1, pad_token_id=None)     # (no pad token: the head reads the LAST position of the one sequence it is given)
    config = transformers.GemmaConfig(**kw)
    config._attn_implementation = "eager"
    model = (transformers.GemmaForCausalLM if kind == "lm" else transformers.GemmaForSequenceClassification)(config).eval()
    G.randomize(model, seed, gain)
    return model.double()


def hf_pair_logits(model, kind: str, seqs, yes: int = 0):
    """transformers' own score of every whole sequence (1-D ids), one at a time: logits[yes] at the last position / the one label -> float64 [n]"""
    out = []
    with torch.no_grad():
        for s in seqs:
            z = model(input_ids=s[None].long()).logits
            out.append(z[0, -1, yes] if kind == "lm" else z[0, 0])
    return torch.stack(out).double()


def score_row(model, kind: str, yes: int = 0, dtype=torch.float64):
    w = (model.lm_head if kind == "lm" else model.score).weight.detach().to(dtype)
    return w[yes] if kind == "lm" else w[0]


# ---- input rows and checkpoint directory ------------------------------------------------------------------------------------------------------------------
def plain_rows(tk, bos, query, docs, prompt, max_length):
    """the reference's per-pair ids, restated in plain Python: every piece tokenised on its own, the query cut to 3/4 of the cap, the passage from the right"""
    enc = lambda s: list(tk.encode(s, add_special_tokens=False).ids)
    q = [bos] + enc("A: " + query)[:max_length * 3 // 4]
    sep = enc("\n")
    out = []
    for d in docs:
        room = max(max_length - len(q) - len(sep), 0)
        out.append(q + sep + enc("B: " + d)[:room] + sep + enc(prompt))
    return q, out


def write_reranker_dir(directory, cfg, model, kind, tokenizer, model_max_length=None, tied=False):
    """config.json (+ architectures, + num_labels / id2label for the one-label form) + model.safetensors + tokenizer.json + tokenizer_config.json; tied:
    lm_head.weight is left out of the file, as a checkpoint with tied embeddings stores it"""
    from safetensors.torch import save_file
    os.makedirs(directory, exist_ok=True)
    cfg = dict(cfg, architectures=["GemmaForCausalLM" if kind == "lm" else "GemmaForSequenceClassification"])
    if kind == "cls":
        cfg.update(num_labels=1, id2label={"0": "LABEL_0"})
    sd = {k: v.detach().float().contiguous() for k, v in model.state_dict().items() if not (tied and k == "lm_head.weight")}
    with open(os.path.join(directory, "config.json"), "w") as f:
        json.dump(cfg, f)
    save_file(sd, os.path.join(directory, "model.safetensors"))
    tokenizer.save(os.path.join(directory, "tokenizer.json"))
    with open(os.path.join(directory, "tokenizer_config.json"), "w") as f:
        json.dump({"pad_token": G.PAD, "eos_token": G.EOS, "bos_token": G.BOS, **({"model_max_length": model_max_length} if model_max_length else {})}, f)
    return directory

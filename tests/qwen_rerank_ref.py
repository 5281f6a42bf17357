"""Helpers of the Qwen3 reranker tests (tests/test_qwen_rerank_host.py, tests/test_qwen_rerank_gpu.py).  Nothing here calls the library.

  - the float64 restatement of prefix-sharing causal attention (the query at local position t of a segment sees the P prefix keys and its own keys 0 .. t),
    on the layout and the budget of tests/qwen_ref.py / tests/attention_ref.py;
  - tiny seeded `Qwen3ForCausalLM` / `Qwen3ForSequenceClassification` models of transformers (the TINY3 / TINY64 shapes of tests/qwen_ref.py), their
    own float64 score of a whole per-pair sequence, and the project's float64 reference of the pair score written from the block equations of
    csrc/qwen.hip;
  - a tokenizer.json with the pieces the template needs (NFC, the Qwen pre-tokeniser, <|im_start|> / <|im_end|>, "yes" / "no") and a checkpoint
    directory as a user brings it."""
import json
import math
import os

import torch

from tests import qwen_ref as Q

QWEN_PRETOKENIZE = (r"(?i:'s|'t|'re|'ve|'m|'ll|'d)|[^\r\n\p{L}\p{N}]?\p{L}+|\p{N}| ?[^\s\p{L}\p{N}]+[\r\n]*|\s*[\r\n]+|\s+(?!\S)|\s+")
SPECIALS = ("<|im_start|>", "<|im_end|>")


# ---- prefix attention in float64 ----------------------------------------------------------------------------------------------------------------------
def prefix_reference(qkv_bf16, P, lens, q_heads, kv_heads, hd):
    """float64 prefix attention on the device of `qkv_bf16` [P + sum(lens), (Q + 2 KV) hd]: rows [0, P) are the prefix, the segments follow
    -> (out, absout) = (P V, P |V|), float64 [P + sum(lens), Q hd]; the prefix rows stay 0 (the kernel under test does not write them)"""
    Qh, KV, G = q_heads, kv_heads, q_heads // kv_heads
    dev, rows = qkv_bf16.device, qkv_bf16.shape[0]
    assert qkv_bf16.dtype == torch.bfloat16 and rows == P + sum(lens) and qkv_bf16.shape[1] == (Qh + 2 * KV) * hd
    out = torch.zeros(rows, Qh * hd, dtype=torch.float64, device=dev)
    absout = torch.zeros_like(out)
    _, pk, pv = Q.split_qkv(qkv_bf16[:P].double(), Qh, KV, hd)
    kvh = torch.arange(Qh, device=dev) // G
    r0 = P
    for ln in lens:
        q, k, v = Q.split_qkv(qkv_bf16[r0:r0 + ln].double(), Qh, KV, hd)
        k, v = torch.cat([pk, k], dim=1)[kvh], torch.cat([pv, v], dim=1)[kvh]                     # [Q, P + ln, hd]
        t = torch.arange(ln, device=dev)
        ok = torch.cat([torch.ones(ln, P, dtype=torch.bool, device=dev), t[None, :] <= t[:, None]], dim=1)
        p = torch.softmax((q @ k.transpose(1, 2) / math.sqrt(hd)).masked_fill(~ok, float("-inf")), dim=-1)
        out[r0:r0 + ln] = (p @ v).transpose(0, 1).reshape(ln, Qh * hd)
        absout[r0:r0 + ln] = (p @ v.abs()).transpose(0, 1).reshape(ln, Qh * hd)
        r0 += ln
    return out, absout


# ---- tiny models ------------------------------------------------------------------------------------------------------------------------------------------
def hf_reranker(cfg: dict, kind: str, seed: int = 0, gain: float = 0.6):
    """transformers' Qwen3ForCausalLM (kind "lm") / Qwen3ForSequenceClassification with one label (kind "cls") for the config dict: eager attention,
    float64, eval, weights from qwen_ref.randomize (lm_head / score included; `gain` is its scale of the Linear weights)"""
    import transformers
    kw = {k: v for k, v in cfg.items() if k not in ("model_type", "architectures")}
    if kind == "cls":
        kw.update(num_labels=1, pad_token_id=None)     # (no pad token: the head reads the LAST position of the one sequence it is given)
    config = transformers.Qwen3Config(**kw)
    config._attn_implementation = "eager"
    model = (transformers.Qwen3ForCausalLM if kind == "lm" else transformers.Qwen3ForSequenceClassification)(config).eval()
    Q.randomize(model, seed, gain)
    return model.double()


def hf_pair_logits(model, kind: str, seqs, yes: int = 0, no: int = 0):
    """transformers' own score of every whole sequence (1-D ids), one at a time: logits[yes] - logits[no] at the last position / the one label -> float64 [n]"""
    out = []
    with torch.no_grad():
        for s in seqs:
            z = model(input_ids=s[None].long()).logits
            out.append(z[0, -1, yes] - z[0, -1, no] if kind == "lm" else z[0, 0])
    return torch.stack(out).double()


def score_row(model, kind: str, yes: int = 0, no: int = 0, dtype=torch.float64):
    """the one weight row the project folds at load (engine/rerank.py::qwen_score_row: the difference is formed in fp32 there), from the module's tensors"""
    w = (model.lm_head if kind == "lm" else model.score).weight.detach().to(dtype)
    return w[yes] - w[no] if kind == "lm" else w[0]


def _rms(x, g, eps):
    return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * g


def hidden64(sd, arch, ids):
    """the project's reference of the tower in float64: final-normed hidden states [len, W] of ONE sequence (1-D ids), from the block equations of
    csrc/qwen.hip on transformers' tensor names (prefix `model.`)"""
    f = lambda k: sd["model." + k].double()
    S, Qh, KV, hd = ids.numel(), arch.heads, arch.kv_heads, arch.head_dim
    x = f("embed_tokens.weight")[ids.long()]
    ang = torch.arange(S, dtype=torch.float64)[:, None] * arch.inv_freq().double()[None, :]
    cos, sin = torch.cat([ang, ang], -1).cos(), torch.cat([ang, ang], -1).sin()
    t = torch.arange(S)
    ok = t[None, :] <= t[:, None]
    for l in range(arch.layers):
        p = f"layers.{l}."
        a = p + "self_attn."
        h = _rms(x, f(p + "input_layernorm.weight"), arch.rms_eps)
        q, k, v = ((h @ f(a + f"{c}_proj.weight").t()).reshape(S, n, hd).transpose(0, 1) for c, n in (("q", Qh), ("k", KV), ("v", KV)))
        q, k = _rms(q, f(a + "q_norm.weight"), arch.rms_eps), _rms(k, f(a + "k_norm.weight"), arch.rms_eps)
        q, k = q * cos + Q._rot_half(q) * sin, k * cos + Q._rot_half(k) * sin
        k, v = k.repeat_interleave(Qh // KV, dim=0), v.repeat_interleave(Qh // KV, dim=0)
        s = (q @ k.transpose(1, 2) / math.sqrt(hd)).masked_fill(~ok, float("-inf"))
        x = x + (torch.softmax(s, -1) @ v).transpose(0, 1).reshape(S, Qh * hd) @ f(a + "o_proj.weight").t()
        h = _rms(x, f(p + "post_attention_layernorm.weight"), arch.rms_eps)
        x = x + ((h @ f(p + "mlp.up_proj.weight").t()) * torch.nn.functional.silu(h @ f(p + "mlp.gate_proj.weight").t())) @ f(p + "mlp.down_proj.weight").t()
    return _rms(x, f("norm.weight"), arch.rms_eps)


def pair_logits64(sd, arch, row, seqs):
    """the project's float64 reference of the pair score: the last final-normed row of every whole sequence . the score row -> float64 [n]"""
    return torch.stack([hidden64(sd, arch, s)[-1] @ row.double() for s in seqs])


# ---- tokenizer and checkpoint directory -----------------------------------------------------------------------------------------------------------------
def train_tokenizer(vocab_size=280, qwen_pretokenizer=True, normalizer="NFC"):
    """a byte-level BPE `tokenizers.Tokenizer` trained from modernbert_ref.CORPUS in memory, <|endoftext|> as id 0, no post-processor; then
    <|im_start|> / <|im_end|> as special tokens and "yes" / "no" as added tokens (all ids below 300, the tiny models' vocab).  qwen_pretokenizer: the Split
    regex of the Qwen files in front of ByteLevel (else ByteLevel's own GPT-2 regex); normalizer: "NFC" (as the Qwen files), "NFKC" or None."""
    from tokenizers import Regex, Tokenizer, decoders, models, normalizers, pre_tokenizers, trainers
    from tests.modernbert_ref import CORPUS
    tk = Tokenizer(models.BPE(unk_token=None))
    if normalizer:
        tk.normalizer = getattr(normalizers, normalizer)()
    if qwen_pretokenizer:
        tk.pre_tokenizer = pre_tokenizers.Sequence([pre_tokenizers.Split(Regex(QWEN_PRETOKENIZE), behavior="isolated", invert=False),
                                                    pre_tokenizers.ByteLevel(add_prefix_space=False, use_regex=False)])
    else:
        tk.pre_tokenizer = pre_tokenizers.ByteLevel(add_prefix_space=False)
    tk.decoder = decoders.ByteLevel()
    trainer = trainers.BpeTrainer(vocab_size=vocab_size, special_tokens=[Q.EOS], initial_alphabet=pre_tokenizers.ByteLevel.alphabet(), show_progress=False)
    tk.train_from_iterator(CORPUS * 4, trainer)
    tk.add_special_tokens(list(SPECIALS))
    tk.add_tokens(["yes", "no"])
    assert tk.get_vocab_size() <= 300
    return tk


def write_reranker_dir(directory, cfg, model, kind, tokenizer, model_max_length=None, tied=False):
    """config.json (+ architectures, + num_labels / id2label for the one-label form) + model.safetensors + tokenizer.json (+ tokenizer_config.json);
    tied: lm_head.weight is left out of the file, as a checkpoint with tied embeddings stores it"""
    from safetensors.torch import save_file
    os.makedirs(directory, exist_ok=True)
    cfg = dict(cfg, architectures=["Qwen3ForCausalLM" if kind == "lm" else "Qwen3ForSequenceClassification"])
    if kind == "cls":
        cfg.update(num_labels=1, id2label={"0": "LABEL_0"})
    sd = {k: v.detach().float().contiguous() for k, v in model.state_dict().items() if not (tied and k == "lm_head.weight")}
    with open(os.path.join(directory, "config.json"), "w") as f:
        json.dump(cfg, f)
    save_file(sd, os.path.join(directory, "model.safetensors"))
    tokenizer.save(os.path.join(directory, "tokenizer.json"))
    with open(os.path.join(directory, "tokenizer_config.json"), "w") as f:
        json.dump({"pad_token": Q.EOS, "eos_token": Q.EOS, **({"model_max_length": model_max_length} if model_max_length else {})}, f)
    return directory

"""Helpers of the NomicBERT tests (tests/test_nomic_bert_host.py, tests/test_attention_full_gpu.py, tests/test_nomic_bert_gpu.py).  Nothing here calls
the library.

  - the tiny config TINY and seeded checkpoints built at test time: transformers' own NomicBertModel(NomicBertConfig(...)) with working magnitudes
    (tiny_model), a directory as `save_pretrained` writes it (transformers' config keys; the tensors come out under the hub's ORIGINAL names, because
    save_pretrained reverses the library's conversion mapping), a directory with the same weights under transformers' module names (native_state_dict),
    and a directory under the hub's original names with a GPT-2-style config.json (hub_state_dict, hub_config), each with a WordPiece tokenizer.json
    trained in memory (tests/jina_bert_ref.py::train_tokenizer, imported);
  - exact / model: the float64 restatement of csrc/nomic_bert.hip's block formula over a packed token stream, in the manner of tests/jina_bert_ref.py
    (Pass and row_ratio of tests/packed_text_ref.py are reused): `model` rounds to bf16 / fp32 exactly where the tower stores bf16 / fp32, `exact`
    rounds nothing.  `exact` is pinned to transformers' NomicBertModel in float64 by tests/test_nomic_bert_host.py.

Where `model` rounds:  e = LN_emb(tok[ids] + type0): x = fp32(e), h = bf16(e) ; qkv = bf16(h Wqkv^T) ; (q | k) = bf16 once more behind the rotation, in
place ; p = bf16, un-normalised, for P V, the normaliser sums the unrounded p ; a = bf16 ; y = fp32(x + a Wo^T) (the GEMM epilogue's one store) ;
n = LN_attn(y): x = fp32(n), h = bf16(n) ; (up | gate) = bf16 ; product = bf16 ; y = fp32(x + product Wdown^T) ; n = LN_mlp(y): x = fp32(n), h = bf16(n) ;
mean = fp32(sum / len) ; L2 = fp32(row / |row|).  The rotary angle is the fp32 product float(t) * inv_freq[i] — what mq_rope forms and what transformers'
NomicBertRotaryEmbedding forms (it forces fp32) — and its cos / sin are float64.  hist = 1 is a second rounding history (encoder_ref._mm).

Mutants of the orchestration (`mut=`, MUTANTS):
    rope_skipped       q and k are not rotated
    rope_on_v          v is rotated as q and k are
    gate_swapped       up and gate change places (up * silu(gate) becomes gate * silu(up))
    gelu_for_silu      the gated product uses erf-GELU
    ln_before_add      the LayerNorm is applied to the sublayer's output, the residual is added behind it: x = x + LN(f(x))
    no_type_row        the token-type row is not added to the token embedding
    theta_10000        the rotary base is 10000 where the checkpoint says 1000
"""
import json
import math
import os
from typing import Dict, List, Optional

import torch

from tests import encoder_ref as E
from tests.jina_bert_ref import random_seqs, train_tokenizer      # noqa: F401
from tests.packed_text_ref import Pass, row_ratio      # noqa: F401

Tensor = torch.Tensor
F64 = torch.float64
SLICE = 64                 # queries per workgroup of csrc/attention_full.hip (four 16-query blocks)
LDS_KEYS = 640             # keys of K + V its LDS holds at 64-wide heads
MUTANTS = ("rope_skipped", "rope_on_v", "gate_swapped", "gelu_for_silu", "ln_before_add", "no_type_row", "theta_10000")

TINY = dict(hidden_size=128, num_attention_heads=2, num_hidden_layers=2, intermediate_size=192, vocab_size=384, max_position_embeddings=2048)
TOWER_LENS = [1, 7, 64, 65, 130]
PIN_LENS = [1, 2, 17, 64]


# ---- tiny checkpoints ---------------------------------------------------------------------------------------------------------------------------------
def tiny_model(seed: int = 0, gain: float = 0.6, **over):
    """transformers' NomicBertModel on TINY (fp32, eval) with seeded working magnitudes in place of the 0.02 initialisation, under which every block is
    nearly the identity: LayerNorm weights 1 + 0.1 N(0, 1), LayerNorm biases 0.1 N(0, 1), the token and type tables N(0, 1), Linear weights
    N(0, gain / sqrt(in)), q and k x 2 (so that q . k / 8 decides which keys a query reads); every Linear weight rounded to bf16 — what the tower stores"""
    from transformers import NomicBertConfig, NomicBertModel
    m = NomicBertModel(NomicBertConfig(**dict(TINY, **over))).eval()
    g = torch.Generator().manual_seed(7000 + seed)
    with torch.no_grad():
        for name, p in m.named_parameters():
            rn = torch.randn(p.shape, generator=g)
            if "layernorm" in name.lower():
                p.copy_(1.0 + 0.1 * rn if name.endswith("weight") else 0.1 * rn)
            elif "embeddings." in name:
                p.copy_(rn)
            else:
                mul = 2.0 if (".q_proj." in name or ".k_proj." in name) else 1.0
                p.copy_((rn * (mul * gain / math.sqrt(p.shape[1]))).to(torch.bfloat16).float())
    return m


def native_state_dict(m) -> Dict[str, Tensor]:
    """the tensors under transformers' module names (layers.N.self_attn.q_proj ...)"""
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


def hub_state_dict(native: Dict[str, Tensor]) -> Dict[str, Tensor]:
    """the same tensors under the hub's original names: the "nomic_bert" entry of transformers' conversion_mapping.py read from right to left (Wqkv is
    q, k, v stacked along dim 0), plus a pooler, an MLM head and a position_ids buffer, to be ignored"""
    out = {}
    layers = 1 + max(int(k.split(".")[1]) for k in native if k.startswith("layers."))
    for k, v in native.items():
        if k.startswith("embeddings.LayerNorm."):
            out["emb_ln." + k.rsplit(".", 1)[1]] = v
        elif k.startswith("embeddings."):
            out[k] = v
    ren = {"self_attn.o_proj": "attn.out_proj", "mlp.up_proj": "mlp.fc11", "mlp.gate_proj": "mlp.fc12", "mlp.down_proj": "mlp.fc2",
           "post_attention_layernorm": "norm1", "post_mlp_layernorm": "norm2"}
    for l in range(layers):
        src, dst = f"layers.{l}.", f"encoder.layers.{l}."
        out[dst + "attn.Wqkv.weight"] = torch.cat([native[src + f"self_attn.{c}_proj.weight"] for c in "qkv"], 0)
        for a, b in ren.items():
            for leaf in ("weight", "bias"):
                if src + f"{a}.{leaf}" in native:
                    out[dst + f"{b}.{leaf}"] = native[src + f"{a}.{leaf}"]
    W = native["embeddings.word_embeddings.weight"].shape[1]
    g = torch.Generator().manual_seed(1)
    out["pooler.dense.weight"], out["pooler.dense.bias"] = torch.randn(W, W, generator=g), torch.randn(W, generator=g)
    out["cls.predictions.transform.dense.weight"] = torch.randn(W, W, generator=g)
    out["embeddings.position_ids"] = torch.arange(16)[None]
    return out


def native_config(**over) -> dict:
    """config.json in transformers' own keys, as NomicBertConfig.save_pretrained writes them"""
    return dict(dict(TINY, model_type="nomic_bert", architectures=["NomicBertModel"], hidden_act="silu", head_dim=64, layer_norm_eps=1e-12,
                     type_vocab_size=2, pad_token_id=0, rope_parameters={"rope_theta": 1000.0, "rope_type": "default"}), **over)


def hub_config(**over) -> dict:
    """config.json in the hub's original GPT-2-style keys (written from memory of the published files; see nomic_bert_arch_from_hf_config)"""
    return dict(dict(model_type="nomic_bert", architectures=["NomicBertModel"], activation_function="swiglu", n_embd=TINY["hidden_size"],
                     n_head=TINY["num_attention_heads"], n_layer=TINY["num_hidden_layers"], n_inner=TINY["intermediate_size"],
                     n_positions=TINY["max_position_embeddings"], vocab_size=TINY["vocab_size"], type_vocab_size=2, layer_norm_epsilon=1e-12,
                     rotary_emb_base=1000, rotary_emb_fraction=1.0, rotary_emb_interleaved=False, rotary_scaling_factor=None, qkv_proj_bias=False,
                     mlp_fc1_bias=False, mlp_fc2_bias=False, prenorm=False, use_rms_norm=False, pad_vocab_size_multiple=64), **over)


def save_pretrained_dir(directory, m, tokenizer=None) -> str:
    """the directory transformers itself writes (config.json in its own keys, model.safetensors) + tokenizer.json"""
    os.makedirs(directory, exist_ok=True)
    m.save_pretrained(directory)
    if tokenizer is not None:
        write_tokenizer(directory, tokenizer)
    return str(directory)


def write_checkpoint_dir(directory, cfg, sd, tokenizer=None, pooling=None) -> str:
    """config.json (either dialect) + model.safetensors (+ tokenizer.json, tokenizer_config.json; + 1_Pooling/config.json when `pooling` is 'mean' / 'cls')"""
    from safetensors.torch import save_file
    os.makedirs(directory, exist_ok=True)
    with open(os.path.join(directory, "config.json"), "w") as f:
        json.dump(cfg, f)
    save_file({k: v.contiguous() for k, v in sd.items()}, os.path.join(directory, "model.safetensors"))
    if tokenizer is not None:
        write_tokenizer(directory, tokenizer)
    if pooling is not None:
        os.makedirs(os.path.join(directory, "1_Pooling"), exist_ok=True)
        with open(os.path.join(directory, "1_Pooling", "config.json"), "w") as f:
            json.dump({"word_embedding_dimension": cfg.get("hidden_size", cfg.get("n_embd")), "pooling_mode_cls_token": pooling == "cls",
                       "pooling_mode_mean_tokens": pooling == "mean"}, f)
    return str(directory)


def write_tokenizer(directory, tokenizer):
    from tests.jina_bert_ref import CLS, MASK, PAD, SEP, UNK
    tokenizer.save(os.path.join(directory, "tokenizer.json"))
    with open(os.path.join(directory, "tokenizer_config.json"), "w") as f:
        json.dump({"cls_token": CLS, "sep_token": SEP, "pad_token": PAD, "unk_token": UNK, "mask_token": MASK}, f)


# ---- the float64 pass -------------------------------------------------------------------------------------------------------------------------------
_FORM = E.Form("nomic_bert")


def operands(tensors: Dict[str, Tensor], device) -> Dict[str, Tensor]:
    """nomic_bert_state_dict's fp32 tensors as the tower stores them, in float64: the weight matrices to bf16; the token table and LayerNorm tensors fp32"""
    return {k: (E._w16(v) if v.dim() == 2 and k != "word_embeddings.weight" else E._f32(v)).to(device) for k, v in tensors.items()}


def _attention(qkv, lens, H, hd, scale, R):
    dev = qkv.device
    A = H * hd
    out = torch.zeros(qkv.shape[0], A, dtype=F64, device=dev)
    r0 = 0
    for ln in lens:
        blk = qkv[r0:r0 + ln]
        q, k, v = (blk[:, i * A:(i + 1) * A].reshape(ln, H, hd).transpose(0, 1) for i in range(3))
        s = q @ k.transpose(1, 2) * scale
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
    rows = ids.shape[0]
    inv_freq = arch.inv_freq()
    if mut == "theta_10000":
        inv_freq = 1.0 / (10000.0 ** (torch.arange(0, hd, 2, dtype=torch.int64).to(torch.float32) / hd))
    pos = E._positions(lens, dev)
    ang32 = pos.to(torch.float32)[:, None] * inv_freq.to(dev)[None, :]      # the fp32 product of mq_rope and of NomicBertRotaryEmbedding
    rot = lambda part: _rope_ang(part.reshape(rows, H, hd), ang32).reshape(rows, W)
    scale = float(torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(hd), dtype=torch.float32).sqrt())
    act = "gelu" if mut == "gelu_for_silu" else "silu"
    ln = lambda y, name: E._ln(y, t[name + ".weight"], t[name + ".bias"], eps)
    e0 = t["word_embeddings.weight"][ids.long()]
    e = ln(e0 if mut == "no_type_row" else e0 + t["type0"], "emb_ln")
    x, h = R.f(e), R.b(e)
    streams: List[Tensor] = []
    for l in range(layers):
        p = f"layer.{l}."
        qkv = R.b(mm(h, t[p + "attn.qkv.weight"]))
        q, k, v = qkv[:, :W], qkv[:, W:2 * W], qkv[:, 2 * W:]
        if mut != "rope_skipped":
            q, k = R.b(rot(q)), R.b(rot(k))
        if mut == "rope_on_v":
            v = R.b(rot(v))
        a = _attention(torch.cat([q, k, v], 1), lens, H, hd, scale, R)
        if mut == "ln_before_add":
            n = x + ln(R.f(mm(a, t[p + "attn.o.weight"])), p + "attn_ln")
        else:
            n = ln(R.f(x + mm(a, t[p + "attn.o.weight"])), p + "attn_ln")
        x, h = R.f(n), R.b(n)
        ug = R.b(mm(h, t[p + "mlp.up_gate.weight"]))
        up, gate = (ug[:, F:], ug[:, :F]) if mut == "gate_swapped" else (ug[:, :F], ug[:, F:])
        d = mm(R.b(up * E._act(gate, act)), t[p + "mlp.down.weight"])
        if mut == "ln_before_add":
            n = x + ln(R.f(d), p + "mlp_ln")
        else:
            n = ln(R.f(x + d), p + "mlp_ln")
        x, h = R.f(n), R.b(n)
        streams.append(x)
    final = x                                     # no final norm
    first = torch.tensor([sum(lens[:i]) for i in range(len(lens))], device=dev)
    seq_of = torch.repeat_interleave(torch.arange(len(lens), device=dev), torch.tensor(lens, device=dev))
    sums = torch.zeros(len(lens), W, dtype=F64, device=dev).index_add_(0, seq_of, final)
    pools = {"mean": R.f(sums / torch.tensor(lens, dtype=F64, device=dev)[:, None]), "cls": final[first]}
    out = {}
    for name, prow in pools.items():
        out[(name, 0)] = prow
        out[(name, 1)] = R.f(prow / prow.norm(dim=-1, keepdim=True))
    return Pass(blocks=streams, final=final, pooled=out)


def _rope_ang(t: Tensor, ang32: Tensor) -> Tensor:
    """rotate_half on [rows, heads, hd] with given fp32 angles [rows, hd / 2]: (x1, x2) = (x[d], x[d + hd / 2]) -> (x1 cos - x2 sin, x2 cos + x1 sin)"""
    hd = t.shape[-1]
    ang = ang32.to(F64)
    c, s = ang.cos()[:, None, :], ang.sin()[:, None, :]
    x1, x2 = t[..., :hd // 2], t[..., hd // 2:]
    return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1)


def exact(arch, tensors, ids, lens, layers: Optional[int] = None) -> Pass:
    return _run(arch, tensors, ids, lens, False, layers, None, 0)


def model(arch, tensors, ids, lens, layers: Optional[int] = None, mut: Optional[str] = None, hist: int = 0) -> Pass:
    return _run(arch, tensors, ids, lens, True, layers, mut, hist)


_built: Dict[str, dict] = {}


def build() -> dict:
    """the seeded tiny checkpoint, built once per process: dict(model = transformers' module, cfg = its config as a dict, arch, sd = the tensors under
    transformers' names, hub_sd = under the hub's names, tensors = nomic_bert_state_dict's output, seqs)"""
    if not _built:
        from marqo_amd.engine import archs, tower_weights as TW
        m = tiny_model()
        cfg = native_config()
        arch = archs.bert_arch_from_hf_config(cfg)
        sd = native_state_dict(m)
        _built.update(model=m, cfg=cfg, arch=arch, sd=sd, hub_sd=hub_state_dict(sd), tensors=TW.nomic_bert_state_dict(arch, sd),
                      seqs=random_seqs(TOWER_LENS, cfg["vocab_size"], seed=3))
    return _built

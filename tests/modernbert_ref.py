"""Helpers of the ModernBERT tests (tests/test_modernbert_host.py, tests/test_attention_window_gpu.py, tests/test_modernbert_gpu.py).  Nothing here calls
the library.

  - the float64 reference of windowed attention and an arithmetic model of csrc/attention_window.hip with switchable faults, on the conventions,
    budget and input families of tests/attention_ref.py (imported, not changed);
  - the project's fp32 oracle of the ModernBERT tower, written from the model's published structure: it is compared with transformers'
    ModernBertModel (eager attention) in the host tests and is the reference of the GPU tests;
  - tiny random checkpoints: configs, seeded weights, a directory as a user would bring it (config.json, weights, a tokenizer.json trained offline).

The window (established against transformers in tests/test_modernbert_host.py::test_window_edge_*): query i sees key j of its own sequence iff
|i - j| <= half_window, half_window = local_attention // 2 — inclusive on both sides."""
import json
import math
import os

import torch

from tests import attention_ref as AR

HS = 64
SLICE = 64          # queries per workgroup of the kernel (four 16-query blocks)
WINDOW_MUTANTS = ("left_long", "left_short", "right_long", "right_short", "edge_as_interior", "skip_tile", "halo_dropped")


# ---- windowed attention: reference and arithmetic model ------------------------------------------------------------------------------------------
def window_allowed(ln, hw, device="cpu"):
    q = torch.arange(ln, device=device)[:, None]
    k = torch.arange(ln, device=device)[None, :]
    return (k - q).abs() <= hw


def window_reference(qkv_bf16, lens, heads, hw):
    """float64 windowed attention on the device of `qkv_bf16` -> (out, absout) = (P V, P |V|), float64 [rows, W] (attention_ref.reference with the band)"""
    W = heads * HS
    dev = qkv_bf16.device
    rows = qkv_bf16.shape[0]
    assert qkv_bf16.dtype == torch.bfloat16 and qkv_bf16.shape[1] == 3 * W and rows == sum(lens)
    out = torch.zeros(rows, W, dtype=torch.float64, device=dev)
    absout = torch.zeros(rows, W, dtype=torch.float64, device=dev)
    r0 = 0
    for ln in lens:
        if ln == 0:
            continue
        blk = qkv_bf16[r0:r0 + ln].double().reshape(1, ln, 3 * W)
        q, k, v = (AR._heads_of(t, heads, HS) for t in blk.split(W, dim=2))
        s = (q @ k.transpose(2, 3) / math.sqrt(HS)).masked_fill(~window_allowed(ln, hw, dev), float("-inf"))
        p = torch.softmax(s, dim=-1)
        out[r0:r0 + ln] = (p @ v).transpose(1, 2).reshape(ln, W)
        absout[r0:r0 + ln] = (p @ v.abs()).transpose(1, 2).reshape(ln, W)
        r0 += ln
    return out, absout


def emulate_window(qkv_bf16, lens, heads, hw, mutant=None):
    """torch-CPU model of the band kernel's arithmetic, per (sequence, 16-query block), all heads in parallel — attention_ref.emulate's softmax (fp32 raw
    scores, 64-key tiles, running max from -1e30, probabilities rounded to bf16 for P.V but summed unrounded, alpha rescale, o / l stored as bf16) on the
    kernel's tile walk: block b of a sequence visits the tiles floor((16 b - hw) / 64) .. floor((min(16 b + 15, len - 1) + hw) / 64) clipped to the
    sequence; a tile inside the band of all 16 queries and inside the sequence is not masked, any other masks per key (key < len, |key - q| <= hw);
    keys past the sequence are copies of key len - 1.  The workgroup of 64-query slice s stages the tiles its four blocks visit; nothing else of that
    shows in the numbers.

    `mutant` switches ONE deliberate fault on (WINDOW_MUTANTS):
      left_long / left_short     the per-key test admits key q - hw - 1 / excludes key q - hw
      right_long / right_short   the per-key test admits key q + hw + 1 / excludes key q + hw
      edge_as_interior           a tile cut by the band's edge is treated as interior: no per-key band test (the end of the sequence is still respected)
      skip_tile                  a block does not visit the last tile of its walk when that tile lies beyond the block's own
      halo_dropped               a block visits only the tile of its own 64-query slice: the halo tiles of a split sequence are not there"""
    assert mutant is None or mutant in WINDOW_MUTANTS
    W = heads * HS
    x = qkv_bf16.cpu()
    out = torch.zeros(x.shape[0], W, dtype=torch.bfloat16)
    c = torch.tensor(1.44269504088896340736 / math.sqrt(HS), dtype=torch.float32)
    NEG = float("-inf")
    lo_w = hw + 1 if mutant == "left_long" else hw - 1 if mutant == "left_short" else hw
    hi_w = hw + 1 if mutant == "right_long" else hw - 1 if mutant == "right_short" else hw
    r0 = 0
    for ln in lens:
        if ln == 0:
            continue
        blk = x[r0:r0 + ln].float().reshape(1, ln, 3 * W)
        q, k, v = (AR._heads_of(t, heads, HS)[0] for t in blk.split(W, dim=2))     # [heads, ln, 64]
        nkt = (ln + 63) // 64
        kidx = torch.arange(nkt * 64).clamp(max=ln - 1)
        k, v = k[:, kidx], v[:, kidx]
        for qb0 in range(0, ln, 16):
            nq = min(16, ln - qb0)
            ql = qb0 + nq - 1
            t_lo = max(qb0 - hw, 0) // 64
            t_hi = min((ql + hw) // 64, nkt - 1) + 1
            tiles = list(range(t_lo, t_hi))
            if mutant == "skip_tile" and tiles[-1] > qb0 // 64:
                tiles = tiles[:-1]
            if mutant == "halo_dropped":
                tiles = [t for t in tiles if t == qb0 // SLICE]
            qi = torch.arange(qb0, qb0 + nq)[:, None]
            qq = q[:, qb0:qb0 + nq]
            m = torch.full((heads, nq, 1), -1e30, dtype=torch.float32)
            l = torch.zeros(heads, nq, 1, dtype=torch.float32)
            o = torch.zeros(heads, nq, HS, dtype=torch.float32)
            for kt in tiles:
                key = torch.arange(kt * 64, kt * 64 + 64)[None, :]
                st = qq @ k[:, kt * 64:kt * 64 + 64].transpose(1, 2)
                interior = kt * 64 >= qb0 + 15 - hw and kt * 64 + 63 <= qb0 + hw and kt * 64 + 63 < ln
                if not interior:
                    valid = key < ln
                    if mutant != "edge_as_interior":
                        valid = valid & (key >= qi - lo_w) & (key <= qi + hi_w)
                    st = st.masked_fill(~valid.expand(nq, 64)[None], NEG)
                m_new = torch.maximum(m, st.max(dim=-1, keepdim=True).values)
                p = torch.exp2(st * c - m_new * c)
                pb = p.to(torch.bfloat16).float()
                alpha = torch.exp2((m - m_new) * c)
                l = l * alpha + p.sum(-1, keepdim=True)
                o = o * alpha + pb @ v[:, kt * 64:kt * 64 + 64]
                m = m_new
            res = (o * (1.0 / l)).to(torch.bfloat16)
            out[r0 + qb0:r0 + qb0 + nq] = res.transpose(0, 1).reshape(nq, W)
        r0 += ln
    return out


# ---- the tower: configs, weights, fp32 oracle ----------------------------------------------------------------------------------------------------
TINY = dict(vocab_size=300, hidden_size=128, num_hidden_layers=4, num_attention_heads=2, intermediate_size=192, local_attention=16,
            max_position_embeddings=256, norm_eps=1e-5, pad_token_id=0, bos_token_id=1, eos_token_id=2, cls_token_id=1, sep_token_id=2)


def config_dict(**over):
    """a ModernBERT config.json as a dict (model_type and the TINY defaults, overridden by `over`; a value of None removes the key)"""
    d = dict(TINY, model_type="modernbert")
    d.update(over)
    return {k: v for k, v in d.items() if v is not None}


def hf_model(cfg: dict, seed: int = 0, gain: float = 0.6):
    """transformers' ModernBertModel for the config dict: eager attention, fp32, eval, weights from `randomize`"""
    from transformers import ModernBertConfig, ModernBertModel
    kw = {k: v for k, v in cfg.items() if k != "model_type"}
    config = ModernBertConfig(**kw)
    config._attn_implementation = "eager"
    model = ModernBertModel(config).float().eval()
    randomize(model, seed, gain)
    return model


def randomize(model, seed, gain=0.6):
    """seeded weights with working magnitudes (the library's init, std 0.02, leaves every softmax flat and every LayerNorm weight at 1), on the scales of
    the project's oracle for its other rotary / gated-GELU tower (oracle/towers.py::synthetic_new_model_state_dict, whose 3e-4 bar the GPU test takes over):
    Linear weights N(0, 0.6 / sqrt(in)) — Wqkv's q and k rows x 2, so that the rotary phases and the window matter to the softmax: attention logits of
    standard deviation ~1.4, as trained encoders have —, LayerNorm weights 1 + 0.1 N(0, 1), token table 0.5 N(0, 1).  `gain` replaces the 0.6: 1.5 is
    the sharp draw of tests/test_modernbert_gpu.py::test_error_by_depth (logits of standard deviation ~9, where the rounding of q and k shows)."""
    g = torch.Generator().manual_seed(1000 + seed)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if p.ndim == 1:
                p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g))
            elif "tok_embeddings" in name:
                p.copy_(0.5 * torch.randn(p.shape, generator=g))
            else:
                p.copy_(torch.randn(p.shape, generator=g) * (gain / math.sqrt(p.shape[1])))
                if name.endswith("Wqkv.weight"):
                    p[:2 * p.shape[1]] *= 2.0


def state_dict_of(model, prefix=""):
    return {prefix + k: v.detach().clone() for k, v in model.state_dict().items()}


def _ln(x, g, eps):
    return torch.nn.functional.layer_norm(x, (x.shape[-1],), g, None, eps)


def _rot_half(x):
    h = x.shape[-1] // 2
    return torch.cat([-x[..., h:], x[..., :h]], dim=-1)


def oracle_hidden(sd, arch, ids, mask=None, kernel_glu=False, bf16_qk=False):
    """The project's fp32 oracle of the tower: last hidden state [n, S, W] of right-padded ids [n, S] (mask [n, S] of 0 / 1, None = no padding; the rows
    of padded positions are computed but mean nothing).  `arch` = engine.archs.ModernBertArch, `sd` = transformers' tensor names without prefix.
    kernel_glu: `sd` is the LOADER's output (engine/tower_weights.py::modernbert_state_dict) and the MLP is computed as mq_glu does it — (up | gate) =
    Wi rows, up * gelu(gate) — which equals the module's gelu(input) * gate only if the loader has swapped the halves of mlp.Wi.
    bf16_qk: q and k (nothing else) are rounded to bf16 where the tower stores them — behind the QKV GEMM and again behind the rotation — so that the share
    of those two roundings in the tower's error can be read off on the host."""
    rb = (lambda t: t.to(torch.bfloat16).float()) if bf16_qk else (lambda t: t)
    n, S = ids.shape
    W, H = arch.width, arch.heads
    f = lambda k: sd[k].float()
    x = _ln(f("embeddings.tok_embeddings.weight")[ids], f("embeddings.norm.weight"), arch.ln_eps)
    pos = torch.arange(S, dtype=torch.float32)
    keyok = torch.ones(n, 1, 1, S, dtype=torch.bool) if mask is None else (mask != 0)[:, None, None, :]
    band = window_allowed(S, arch.half_window)[None, None]
    for l in range(arch.layers):
        p = f"layers.{l}."
        h = x if l == 0 else _ln(x, f(p + "attn_norm.weight"), arch.ln_eps)
        q, k, v = ((h @ f(p + "attn.Wqkv.weight").t()).reshape(n, S, 3, H, HS).permute(2, 0, 3, 1, 4))     # each [n, H, S, 64]
        ang = pos[:, None] * arch.inv_freq(local=arch.sliding[l])[None, :]
        cos, sin = torch.cat([ang, ang], -1).cos(), torch.cat([ang, ang], -1).sin()
        q, k = rb(q), rb(k)
        q, k = rb(q * cos + _rot_half(q) * sin), rb(k * cos + _rot_half(k) * sin)
        ok = keyok & band if arch.sliding[l] else keyok.expand(n, 1, S, S)
        s = (q @ k.transpose(2, 3) / math.sqrt(HS)).masked_fill(~ok, float("-inf"))
        prob = torch.nan_to_num(torch.softmax(s, -1))     # (a padded query row on a sliding layer may see no key at all: zeros, never NaN)
        a = (prob @ v).transpose(1, 2).reshape(n, S, W)
        x = x + a @ f(p + "attn.Wo.weight").t()
        inp, gate = (_ln(x, f(p + "mlp_norm.weight"), arch.ln_eps) @ f(p + "mlp.Wi.weight").t()).chunk(2, dim=-1)
        x = x + ((inp * torch.nn.functional.gelu(gate)) if kernel_glu else (torch.nn.functional.gelu(inp) * gate)) @ f(p + "mlp.Wo.weight").t()
    return _ln(x, f("final_norm.weight"), arch.ln_eps)


def oracle_hidden_packed(sd, arch, seqs, **kw):
    """the packed form: every sequence (1-D ids) on its own, no padding anywhere -> list of [len, W]"""
    return [oracle_hidden(sd, arch, s[None], **kw)[0] for s in seqs]


def first_layers(arch, k):
    """the model cut behind its k-th block (final_norm follows): the arch both the oracle and the tower take with the full state dict"""
    from dataclasses import replace
    return replace(arch, layers=k, sliding=tuple(arch.sliding[:k]))


def pooled(hidden_list, pooling="mean"):
    """list of [len, W] -> float64 [n, W], L2-normalised rows"""
    rows = torch.stack([(h.double().mean(0) if pooling == "mean" else h[0].double()) for h in hidden_list])
    return rows / rows.norm(dim=-1, keepdim=True)


def pad_batch(seqs, pad_id=0):
    S = max(len(s) for s in seqs)
    ids = torch.full((len(seqs), S), pad_id, dtype=torch.long)
    mask = torch.zeros(len(seqs), S, dtype=torch.long)
    for i, s in enumerate(seqs):
        ids[i, :len(s)] = s
        mask[i, :len(s)] = 1
    return ids, mask


def random_seqs(lengths, vocab, seed=0):
    g = torch.Generator().manual_seed(7000 + seed)
    return [torch.randint(3, vocab, (n,), generator=g) for n in lengths]


# ---- a checkpoint directory as a user brings it -------------------------------------------------------------------------------------------------------
CORPUS = ["the quick brown fox jumps over the lazy dog", "sliding window attention keeps long documents cheap", "a search engine ranks documents for a query",
          "rotary positions turn queries and keys by an angle", "gated linear units multiply two projections", "embeddings of sentences are pooled and normalised",
          "hello world", "tensor search with vectors", "Paris is the capital of France", "numbers 0 1 2 3 4 5 6 7 8 9 and punctuation , . ! ? ' -"]


def train_tokenizer(vocab_size=300):
    """a byte-level BPE `tokenizers.Tokenizer` trained from CORPUS in memory, with [PAD] [CLS] [SEP] [UNK] [MASK] as ids 0 .. 4 and the
    "[CLS] $A [SEP]" template — the shape of ModernBERT's tokenizer.json, no download"""
    from tokenizers import Tokenizer, decoders, models, pre_tokenizers, processors, trainers
    tk = Tokenizer(models.BPE(unk_token=None))
    tk.pre_tokenizer = pre_tokenizers.ByteLevel(add_prefix_space=False)
    tk.decoder = decoders.ByteLevel()
    specials = ["[PAD]", "[CLS]", "[SEP]", "[UNK]", "[MASK]"]
    trainer = trainers.BpeTrainer(vocab_size=vocab_size, special_tokens=specials, initial_alphabet=pre_tokenizers.ByteLevel.alphabet(), show_progress=False)
    tk.train_from_iterator(CORPUS * 4, trainer)
    tk.post_processor = processors.TemplateProcessing(single="[CLS] $A [SEP]", special_tokens=[("[CLS]", 1), ("[SEP]", 2)])
    return tk


def write_checkpoint_dir(directory, cfg, sd, tokenizer=None, safetensors=True):
    """config.json + model.safetensors (or pytorch_model.bin) + tokenizer.json (+ tokenizer_config.json naming the specials)"""
    os.makedirs(directory, exist_ok=True)
    with open(os.path.join(directory, "config.json"), "w") as f:
        json.dump(cfg, f)
    if safetensors:
        from safetensors.torch import save_file
        save_file({k: v.contiguous() for k, v in sd.items()}, os.path.join(directory, "model.safetensors"))
    else:
        torch.save(sd, os.path.join(directory, "pytorch_model.bin"))
    if tokenizer is not None:
        tokenizer.save(os.path.join(directory, "tokenizer.json"))
        with open(os.path.join(directory, "tokenizer_config.json"), "w") as f:
            json.dump({"cls_token": "[CLS]", "sep_token": "[SEP]", "pad_token": "[PAD]", "unk_token": "[UNK]", "mask_token": "[MASK]"}, f)
    return directory

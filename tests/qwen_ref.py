"""Helpers of the Qwen3 / Qwen2 tests (tests/test_qwen_host.py, tests/test_attention_gqa_gpu.py, tests/test_qwen_gpu.py).  Nothing here calls the library.

  - the float64 reference of grouped-query attention and a tile-order arithmetic model of csrc/attention_gqa.hip with switchable faults, on the budget,
    bf16 constants and input families of tests/attention_ref.py (imported, not changed);
  - tiny random checkpoints (TINY3, TINY2, TINY64), the project's fp32 oracle of the tower written from the block equations of csrc/qwen.hip — compared
    with transformers' Qwen3Model / Qwen2Model in the host tests, the reference of the GPU tests —, and a checkpoint directory as a user brings it.

Layout (the kernel's): `qkv` is bf16 [rows, (Q + 2 KV) hd] = (q | k | v), head h of each part at columns h hd ..; query head h reads K/V head h // G,
G = Q // KV (transformers' repeat_kv)."""
import json
import math
import os

import torch

from tests import attention_ref as AR

SLICE = 128         # queries per workgroup of the kernel (eight 16-query blocks)
LDS_KEYS = {64: 640, 128: 320}      # keys the LDS holds per head width
GQA_MUTANTS = ("kv_mod", "kv_zero", "causal_plus1", "causal_minus_self", "skip_tile", "dup_last", "slice_keys_short")


# ---- grouped-query attention: inputs, reference, arithmetic model ---------------------------------------------------------------------------------------
def split_qkv(x, Q, KV, hd):
    """[rows, (Q + 2 KV) hd] -> q [Q, rows, hd], k [KV, rows, hd], v [KV, rows, hd]"""
    rows = x.shape[0]
    q, k, v = x.split([Q * hd, KV * hd, KV * hd], dim=1)
    return (q.reshape(rows, Q, hd).transpose(0, 1), k.reshape(rows, KV, hd).transpose(0, 1), v.reshape(rows, KV, hd).transpose(0, 1))


def make_gqa_qkv(family, lens, Q, KV, hd, seed=0, device="cpu"):
    """bf16 [rows, (Q + 2 KV) hd] of one attention_ref family: q from a Q-head draw, k and v from a KV-head draw.  In the `readout` family K/V head j
    carries attention_ref.readout_v rolled by 3 j columns, so every K/V head has a distinct V and a query head that reads the wrong one shows it."""
    rows = sum(lens)
    a = AR.make_qkv(family, lens, Q, hd, seed=seed)
    b = AR.make_qkv(family, lens, KV, hd, seed=seed + 1000)
    q = a[:, :Q * hd]
    k, v = b[:, KV * hd:2 * KV * hd], b[:, 2 * KV * hd:]
    if family == "readout":
        v = torch.stack([torch.roll(AR.readout_v(lens, 1, hd)[:, 0], 3 * j, dims=1) for j in range(KV)], dim=1).reshape(rows, KV * hd).to(torch.bfloat16)
    return torch.cat([q, k, v], dim=1).contiguous().to(device)


def expand_kv(qkv, Q, KV, hd):
    """the same numbers on mq_attention's [rows, 3 Q hd] layout: K/V head h // G copied to query head h (repeat_interleave, as repeat_kv)"""
    rows, G = qkv.shape[0], Q // KV
    q, k, v = qkv.split([Q * hd, KV * hd, KV * hd], dim=1)
    rep = lambda t: t.reshape(rows, KV, hd).repeat_interleave(G, dim=1).reshape(rows, Q * hd)
    return torch.cat([q, rep(k), rep(v)], dim=1).contiguous()


def gqa_reference(qkv_bf16, lens, q_heads, kv_heads, hd, mask):
    """float64 grouped-query attention on the device of `qkv_bf16` -> (out, absout) = (P V, P |V|), float64 [rows, Q hd]"""
    Q, KV, G = q_heads, kv_heads, q_heads // kv_heads
    dev, rows = qkv_bf16.device, qkv_bf16.shape[0]
    assert qkv_bf16.dtype == torch.bfloat16 and qkv_bf16.shape[1] == (Q + 2 * KV) * hd and rows == sum(lens) and Q % KV == 0
    out = torch.zeros(rows, Q * hd, dtype=torch.float64, device=dev)
    absout = torch.zeros(rows, Q * hd, dtype=torch.float64, device=dev)
    r0 = 0
    for ln in lens:
        if ln == 0:
            continue
        q, k, v = split_qkv(qkv_bf16[r0:r0 + ln].double(), Q, KV, hd)
        kvh = torch.arange(Q, device=dev) // G
        s = (q @ k[kvh].transpose(1, 2) / math.sqrt(hd)).masked_fill(~AR.allowed(ln, mask, dev), float("-inf"))
        p = torch.softmax(s, dim=-1)
        out[r0:r0 + ln] = (p @ v[kvh]).transpose(0, 1).reshape(ln, Q * hd)
        absout[r0:r0 + ln] = (p @ v[kvh].abs()).transpose(0, 1).reshape(ln, Q * hd)
        r0 += ln
    return out, absout


def emulate_gqa(qkv_bf16, lens, q_heads, kv_heads, hd, mask, mutant=None):
    """torch-CPU model of csrc/attention_gqa.hip's arithmetic in the kernel's tile order, per (sequence, 128-query slice, 16-query block), all query heads
    in parallel: attention_ref.emulate's softmax (fp32 raw scores, 64-key tiles, running max from -1e30, probabilities rounded to bf16 for P.V but summed
    unrounded, alpha rescale, o / l stored as bf16).  The slice of queries [128 s, 128 s + 127] stages key tiles 0 .. floor(q_last / 64) under the causal
    mask (every tile of the sequence without one); a block visits the staged tiles up to the one of its last query (causal) or all of them; a tile is
    masked per key (key < len, causal: key <= q) when it is the ragged last one or reaches past the block's first query.  Keys past the sequence are
    copies of key len - 1.

    `mutant` switches ONE deliberate fault on (GQA_MUTANTS):
      kv_mod             query head h reads K/V head h % KV instead of h // G
      kv_zero            every query head reads K/V head 0
      causal_plus1       the causal test admits key q + 1
      causal_minus_self  the causal test excludes key q
      skip_tile          a block that visits two tiles or more does not visit tile 0
      dup_last           key `len` is admitted in the ragged tile: key len - 1 counted twice (shows where the causal test does not hide it: unmasked)
      slice_keys_short   a slice that stages two tiles or more stages one too few: its blocks never see the last of them"""
    assert mutant is None or mutant in GQA_MUTANTS
    Q, KV, G = q_heads, kv_heads, q_heads // kv_heads
    x = qkv_bf16.cpu()
    out = torch.zeros(x.shape[0], Q * hd, dtype=torch.bfloat16)
    c = torch.tensor(1.44269504088896340736 / math.sqrt(hd), dtype=torch.float32)
    causal = mask != AR.MASK_NONE
    heads = torch.arange(Q)
    kvh = heads % KV if mutant == "kv_mod" else torch.zeros(Q, dtype=torch.long) if mutant == "kv_zero" else heads // G
    r0 = 0
    for ln in lens:
        if ln == 0:
            continue
        q, k, v = split_qkv(x[r0:r0 + ln].float(), Q, KV, hd)
        nkt = (ln + 63) // 64
        kidx = torch.arange(nkt * 64).clamp(max=ln - 1)
        k, v = k[kvh][:, kidx], v[kvh][:, kidx]          # [Q, kp, hd]
        for qb0 in range(0, ln, 16):
            nq = min(16, ln - qb0)
            q0 = qb0 // SLICE * SLICE
            q_last = min(q0 + SLICE - 1, ln - 1)
            skt = q_last // 64 + 1 if causal else nkt
            if mutant == "slice_keys_short" and skt >= 2:
                skt -= 1
            kt_end = min((qb0 + 15) // 64 + 1, skt) if causal else skt
            tiles = list(range(kt_end))
            if mutant == "skip_tile" and len(tiles) >= 2:
                tiles = tiles[1:]
            qi = torch.arange(qb0, qb0 + nq)[:, None]
            qq = q[:, qb0:qb0 + nq]
            m = torch.full((Q, nq, 1), -1e30, dtype=torch.float32)
            l = torch.zeros(Q, nq, 1, dtype=torch.float32)
            o = torch.zeros(Q, nq, hd, dtype=torch.float32)
            for kt in tiles:
                key = torch.arange(kt * 64, kt * 64 + 64)[None, :]
                st = qq @ k[:, kt * 64:kt * 64 + 64].transpose(1, 2)
                need_mask = (kt == nkt - 1 and ln % 64 != 0) or (causal and kt * 64 + 63 > qb0)
                if need_mask:
                    valid = (key < (ln + 1 if mutant == "dup_last" else ln)).expand(nq, 64)
                    if causal:
                        lim = qi + 1 if mutant == "causal_plus1" else qi
                        valid = valid & ((key < lim) if mutant == "causal_minus_self" else (key <= lim))
                    st = st.masked_fill(~valid[None], float("-inf"))
                m_new = torch.maximum(m, st.max(dim=-1, keepdim=True).values)
                p = torch.exp2(st * c - m_new * c)
                pb = p.to(torch.bfloat16).float()
                alpha = torch.exp2((m - m_new) * c)
                l = l * alpha + p.sum(-1, keepdim=True)
                o = o * alpha + pb @ v[:, kt * 64:kt * 64 + 64]
                m = m_new
            res = (o * (1.0 / l)).to(torch.bfloat16)
            out[r0 + qb0:r0 + qb0 + nq] = res.transpose(0, 1).reshape(nq, Q * hd)
        r0 += ln
    return out


# ---- the tower: configs, weights, fp32 oracle ----------------------------------------------------------------------------------------------------------
_COMMON = dict(vocab_size=300, num_hidden_layers=3, max_position_embeddings=256, rms_norm_eps=1e-6, hidden_act="silu", tie_word_embeddings=False,
               pad_token_id=0, bos_token_id=0, eos_token_id=0)
TINY3 = dict(_COMMON, model_type="qwen3", hidden_size=256, num_attention_heads=4, num_key_value_heads=2, head_dim=128, intermediate_size=384,
             rope_parameters={"rope_type": "default", "rope_theta": 1000000.0})
TINY2 = dict(_COMMON, model_type="qwen2", hidden_size=256, num_attention_heads=4, num_key_value_heads=1, intermediate_size=384,
             rope_parameters={"rope_type": "default", "rope_theta": 10000.0})
TINY64 = dict(_COMMON, model_type="qwen3", hidden_size=128, num_attention_heads=4, num_key_value_heads=2, head_dim=64, intermediate_size=192,
              rope_parameters={"rope_type": "default", "rope_theta": 1000000.0})
TINIES = {"TINY3": TINY3, "TINY2": TINY2, "TINY64": TINY64}


def config_dict(base, **over):
    """a config.json as a dict: `base` overridden by `over`; a value of None removes the key"""
    d = dict(base)
    d.update(over)
    return {k: v for k, v in d.items() if v is not None}


def hf_model(cfg: dict, seed: int = 0, gain: float = 0.6):
    """transformers' Qwen3Model / Qwen2Model for the config dict: eager attention, fp32, eval, weights from `randomize`"""
    import transformers
    kw = {k: v for k, v in cfg.items() if k != "model_type"}
    Config, Model = ((transformers.Qwen3Config, transformers.Qwen3Model) if cfg["model_type"] == "qwen3" else (transformers.Qwen2Config, transformers.Qwen2Model))
    config = Config(**kw)
    config._attn_implementation = "eager"
    model = Model(config).float().eval()
    randomize(model, seed, gain)
    return model


def randomize(model, seed, gain=0.6):
    """seeded weights with working magnitudes, on the scales of modernbert_ref.randomize: Linear weights N(0, gain / sqrt(in)) — q_proj and k_proj x 2, so
    that the rotary phases and the causal edge matter to the softmax —, every norm weight (the blocks', the final one, q_norm and k_norm) 1 + 0.1 N(0, 1)
    so that a dropped norm is seen, biases 0.1 N(0, 1), token table 0.5 N(0, 1)"""
    g = torch.Generator().manual_seed(2000 + seed)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name.endswith(".bias"):
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
            elif p.ndim == 1:
                p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g))
            elif "embed_tokens" in name:
                p.copy_(0.5 * torch.randn(p.shape, generator=g))
            else:
                p.copy_(torch.randn(p.shape, generator=g) * (gain / math.sqrt(p.shape[1])))
                if name.endswith("q_proj.weight") or name.endswith("k_proj.weight"):
                    p.mul_(2.0)


def state_dict_of(model, prefix=""):
    return {prefix + k: v.detach().clone() for k, v in model.state_dict().items()}


def _rms(x, g, eps):
    return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * g


def _rot_half(x):
    h = x.shape[-1] // 2
    return torch.cat([-x[..., h:], x[..., :h]], dim=-1)


def oracle_hidden(sd, arch, ids, mask=None, kernel_glu=False, bf16_qk=False):
    """The project's fp32 oracle of the tower: last hidden state [n, S, W] of right-padded ids [n, S] (mask [n, S] of 0 / 1, None = no padding; the rows of
    padded positions are computed but mean nothing).  `arch` = engine.archs.QwenArch, `sd` = transformers' tensor names without prefix.
    kernel_glu: `sd` is the LOADER's output (engine/tower_weights.py::qwen_state_dict: fused qkv and (up | gate)) and the MLP is computed as mq_glu does
    it, up * silu(gate) over the halves of the fused weight — equal to the module's only if the loader put up_proj first.
    bf16_qk: q and k (nothing else) are rounded to bf16 where the tower stores them, behind the QKV GEMM and behind norm + rotation."""
    rb = (lambda t: t.to(torch.bfloat16).float()) if bf16_qk else (lambda t: t)
    n, S = ids.shape
    Q, KV, hd, F = arch.heads, arch.kv_heads, arch.head_dim, arch.mlp_dim
    G = Q // KV
    f = lambda k: sd[k].float()
    x = f("embed_tokens.weight")[ids]
    ang = torch.arange(S, dtype=torch.float32)[:, None] * arch.inv_freq()[None, :]
    cos, sin = torch.cat([ang, ang], -1).cos(), torch.cat([ang, ang], -1).sin()
    ok = AR.allowed(S, AR.MASK_CAUSAL)[None, None]
    if mask is not None:
        ok = ok & (mask != 0)[:, None, None, :]
    for l in range(arch.layers):
        p = f"layers.{l}."
        a = p + "self_attn."
        h = _rms(x, f(p + "input_layernorm.weight"), arch.rms_eps)
        if kernel_glu:
            qkv = h @ f(a + "qkv.weight").t() + (f(a + "qkv.bias") if arch.qkv_bias else 0.0)
            q, k, v = qkv.split([Q * hd, KV * hd, KV * hd], dim=-1)
        else:
            q, k, v = (h @ f(a + f"{c}_proj.weight").t() + (f(a + f"{c}_proj.bias") if arch.qkv_bias else 0.0) for c in "qkv")
        q, k, v = q.reshape(n, S, Q, hd).transpose(1, 2), k.reshape(n, S, KV, hd).transpose(1, 2), v.reshape(n, S, KV, hd).transpose(1, 2)
        q, k = rb(q), rb(k)
        if arch.qk_norm:
            q, k = _rms(q, f(a + "q_norm.weight"), arch.rms_eps), _rms(k, f(a + "k_norm.weight"), arch.rms_eps)
        q, k = rb(q * cos + _rot_half(q) * sin), rb(k * cos + _rot_half(k) * sin)
        k, v = k.repeat_interleave(G, dim=1), v.repeat_interleave(G, dim=1)
        s = (q @ k.transpose(2, 3) / math.sqrt(hd)).masked_fill(~ok, float("-inf"))
        at = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(n, S, Q * hd)
        x = x + at @ f(a + "o_proj.weight").t()
        h = _rms(x, f(p + "post_attention_layernorm.weight"), arch.rms_eps)
        if kernel_glu:
            up, gate = (h @ f(p + "mlp.up_gate.weight").t()).chunk(2, dim=-1)
        else:
            up, gate = h @ f(p + "mlp.up_proj.weight").t(), h @ f(p + "mlp.gate_proj.weight").t()
        x = x + (up * torch.nn.functional.silu(gate)) @ f(p + "mlp.down_proj.weight").t()
    return _rms(x, f("norm.weight"), arch.rms_eps)


def oracle_hidden_packed(sd, arch, seqs, **kw):
    """the packed form: every sequence (1-D ids) on its own, no padding anywhere -> list of [len, W]"""
    return [oracle_hidden(sd, arch, s[None], **kw)[0] for s in seqs]


def pooled(hidden_list, pooling="last", normalize=True):
    """list of [len, W] -> float64 [n, W]: the last row or the mean of every sequence, L2-normalised when asked"""
    rows = torch.stack([(h[-1].double() if pooling == "last" else h.double().mean(0)) for h in hidden_list])
    return rows / rows.norm(dim=-1, keepdim=True) if normalize else rows


def pad_batch(seqs, pad_id=0):
    S = max(len(s) for s in seqs)
    ids = torch.full((len(seqs), S), pad_id, dtype=torch.long)
    mask = torch.zeros(len(seqs), S, dtype=torch.long)
    for i, s in enumerate(seqs):
        ids[i, :len(s)] = s
        mask[i, :len(s)] = 1
    return ids, mask


def random_seqs(lengths, vocab, seed=0):
    g = torch.Generator().manual_seed(8000 + seed)
    return [torch.randint(1, vocab, (n,), generator=g) for n in lengths]


# ---- a checkpoint directory as a user brings it ---------------------------------------------------------------------------------------------------------
EOS = "<|endoftext|>"


def train_tokenizer(vocab_size=300, append_eos=True):
    """a byte-level BPE `tokenizers.Tokenizer` trained from modernbert_ref.CORPUS in memory, <|endoftext|> as id 0 and — as Qwen3-Embedding's file — a
    TemplateProcessing that appends it (append_eos=False: no post-processor, as the Qwen2 files); no [CLS] / [SEP] anywhere"""
    from tokenizers import Tokenizer, decoders, models, pre_tokenizers, processors, trainers
    from tests.modernbert_ref import CORPUS
    tk = Tokenizer(models.BPE(unk_token=None))
    tk.pre_tokenizer = pre_tokenizers.ByteLevel(add_prefix_space=False)
    tk.decoder = decoders.ByteLevel()
    trainer = trainers.BpeTrainer(vocab_size=vocab_size, special_tokens=[EOS], initial_alphabet=pre_tokenizers.ByteLevel.alphabet(), show_progress=False)
    tk.train_from_iterator(CORPUS * 4, trainer)
    if append_eos:
        tk.post_processor = processors.TemplateProcessing(single=f"$A {EOS}", pair=f"$A {EOS} $B:1 {EOS}:1", special_tokens=[(EOS, 0)])
    return tk


def write_checkpoint_dir(directory, cfg, sd, tokenizer=None, pooling=None, pad_token=EOS):
    """config.json + model.safetensors + tokenizer.json (+ tokenizer_config.json naming the pad token; + 1_Pooling/config.json when `pooling` is 'last' /
    'mean' / 'cls')"""
    from safetensors.torch import save_file
    os.makedirs(directory, exist_ok=True)
    with open(os.path.join(directory, "config.json"), "w") as f:
        json.dump(cfg, f)
    save_file({k: v.contiguous() for k, v in sd.items()}, os.path.join(directory, "model.safetensors"))
    if tokenizer is not None:
        tokenizer.save(os.path.join(directory, "tokenizer.json"))
        if pad_token is not None:
            with open(os.path.join(directory, "tokenizer_config.json"), "w") as f:
                json.dump({"pad_token": pad_token, "eos_token": EOS}, f)
    if pooling is not None:
        os.makedirs(os.path.join(directory, "1_Pooling"), exist_ok=True)
        with open(os.path.join(directory, "1_Pooling", "config.json"), "w") as f:
            json.dump({"word_embedding_dimension": cfg["hidden_size"], "pooling_mode_cls_token": pooling == "cls", "pooling_mode_mean_tokens": pooling == "mean",
                       "pooling_mode_lasttoken": pooling == "last"}, f)
    return directory

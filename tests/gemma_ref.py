"""Helpers of the EmbeddingGemma tests (tests/test_gemma_host.py, tests/test_attention_gqa256_gpu.py, tests/test_gemma_gpu.py).  Nothing here calls the
library.

  - the float64 reference of grouped-query BAND attention and a tile-order arithmetic model of csrc/attention_gqa256.hip with switchable faults, on the
    budget, bf16 constants and input families of tests/attention_ref.py and tests/qwen_ref.py (imported, not changed);
  - tiny random checkpoints (TINY, TINY_SLIDING, TINY_FULL), the project's fp32 oracle of the tower written from the block equations of csrc/gemma.hip —
    compared with transformers' Gemma3TextModel in the host tests, the reference of the GPU tests —, and a checkpoint directory as a user brings it;
  - the float64 tanh-GELU product and its budget.

Layout (the kernel's): `qkv` is bf16 [rows, (Q + 2 KV) hd] = (q | k | v), head h of each part at columns h hd ..; query head h reads K/V head h // G,
G = Q // KV.  half_window hw == 0: every key; hw > 0: query i sees keys j with |i - j| <= hw."""
import json
import math
import os

import torch

from tests import attention_ref as AR
from tests import qwen_ref as Q

HD = 256
SLICE = 64          # queries per workgroup of the kernel (four 16-query blocks)
NW = 8              # waves per workgroup: work items per round
PIECE_KEYS = 128    # keys (two 64-key tiles) the LDS holds at 512-byte rows
BAND_MUTANTS = ("kv_mod", "kv_zero", "lo_wide", "lo_narrow", "hi_wide", "hi_narrow", "skip_tile", "dup_tile", "stale_piece")


# ---- grouped-query band attention: inputs, reference, arithmetic model --------------------------------------------------------------------------------
def make_band_qkv(family, lens, Q_, KV, hd=HD, seed=0, device="cpu"):
    """qwen_ref.make_gqa_qkv at 256-wide heads (`readout`: one-hot V rows, a different roll per K/V head; `peaked`: sharp rows, V over four decades)"""
    return Q.make_gqa_qkv(family, lens, Q_, KV, hd, seed=seed, device=device)


def band_allowed(ln, hw, device="cpu"):
    """[ln, ln] bool: True where query i sees key j"""
    i = torch.arange(ln, device=device)
    if hw <= 0:
        return torch.ones(ln, ln, dtype=torch.bool, device=device)
    return (i[:, None] - i[None, :]).abs() <= hw


def band_gqa_reference(qkv_bf16, lens, q_heads, kv_heads, hd, hw, scale=None):
    """float64 grouped-query band attention on the device of `qkv_bf16` -> (out, absout) = (P V, P |V|), float64 [rows, Q hd]"""
    Qh, KV, G = q_heads, kv_heads, q_heads // kv_heads
    dev, rows = qkv_bf16.device, qkv_bf16.shape[0]
    assert qkv_bf16.dtype == torch.bfloat16 and qkv_bf16.shape[1] == (Qh + 2 * KV) * hd and rows == sum(lens) and Qh % KV == 0
    scale = hd ** -0.5 if scale is None else scale
    out = torch.zeros(rows, Qh * hd, dtype=torch.float64, device=dev)
    absout = torch.zeros(rows, Qh * hd, dtype=torch.float64, device=dev)
    r0 = 0
    for ln in lens:
        if ln == 0:
            continue
        q, k, v = Q.split_qkv(qkv_bf16[r0:r0 + ln].double(), Qh, KV, hd)
        kvh = torch.arange(Qh, device=dev) // G
        s = (q @ k[kvh].transpose(1, 2) * scale).masked_fill(~band_allowed(ln, hw, dev), float("-inf"))
        p = torch.softmax(s, dim=-1)
        out[r0:r0 + ln] = (p @ v[kvh]).transpose(0, 1).reshape(ln, Qh * hd)
        absout[r0:r0 + ln] = (p @ v[kvh].abs()).transpose(0, 1).reshape(ln, Qh * hd)
        r0 += ln
    return out, absout


def emulate_band(qkv_bf16, lens, q_heads, kv_heads, hd, hw, scale=None, mutant=None):
    """torch-CPU model of csrc/attention_gqa256.hip's arithmetic in the kernel's order, per (sequence, 64-query slice, work item = (query head of the
    group, 16-query block)): attention_ref.emulate's softmax (fp32 raw scores, 64-key tiles, running max from -1e30, probabilities rounded to bf16 for
    P.V but summed unrounded, alpha rescale, o / l stored as bf16).  The host turns `no band` (hw == 0) and a band that covers every sequence of the call
    (hw >= max(lens) - 1) into hw = 16384.  The slice of queries [64 s, 64 s + 63] stages key tiles floor((q0 - hw) / 64) .. floor((q_last + hw) / 64),
    clipped, in pieces of two tiles (one when the call needs no more than 64 keys), re-staged for every round of 8 work items; a block visits the tiles
    floor((qb0 - hw) / 64) .. floor((qb0 + 15 + hw) / 64) of every piece in ascending order; a tile is masked per key (key < len, |key - q| <= hw)
    unless it lies inside the band of all 16 queries and inside the sequence.  Keys past the sequence are copies of key len - 1.

    `mutant` switches ONE deliberate fault on (BAND_MUTANTS):
      kv_mod       query head h reads K/V head h % KV instead of h // G
      kv_zero      every query head reads K/V head 0
      lo_wide      the band admits key q - hw - 1            lo_narrow    the band excludes key q - hw
      hi_wide      the band admits key q + hw + 1            hi_narrow    the band excludes key q + hw
      skip_tile    a block that visits two tiles or more does not visit its first
      dup_tile     a block that visits two tiles or more visits its last twice
      stale_piece  in the second and later rounds the first piece is not re-staged: its tiles read what the previous round's last piece left in the LDS"""
    assert mutant is None or mutant in BAND_MUTANTS
    Qh, KV, G = q_heads, kv_heads, q_heads // kv_heads
    x = qkv_bf16.cpu()
    out = torch.zeros(x.shape[0], Qh * hd, dtype=torch.bfloat16)
    scale = hd ** -0.5 if scale is None else scale
    c = torch.tensor(1.44269504088896340736, dtype=torch.float32) * torch.tensor(scale, dtype=torch.float32)
    maxl = max(lens)
    hwk = 16384 if (hw == 0 or hw >= maxl - 1) else hw
    reach = 1 << 20 if hwk >= 16384 else 1 + 2 * ((hwk + 63) // 64)
    tpc = min(min(reach, (maxl + 63) // 64) * 64, PIECE_KEYS) // 64
    lo_d = {"lo_wide": 1, "lo_narrow": -1}.get(mutant, 0)
    hi_d = {"hi_wide": 1, "hi_narrow": -1}.get(mutant, 0)
    r0 = 0
    for ln in lens:
        if ln == 0:
            continue
        q, k, v = Q.split_qkv(x[r0:r0 + ln].float(), Qh, KV, hd)
        nkt = (ln + 63) // 64
        kidx = torch.arange(nkt * 64).clamp(max=ln - 1)
        k, v = k[:, kidx], v[:, kidx]          # [KV, kp, hd]
        for q0 in range(0, ln, SLICE):
            q_last = min(q0 + SLICE - 1, ln - 1)
            nblk = (q_last - q0) // 16 + 1
            kt_lo = max(q0 - hwk, 0) // 64
            kt_hi = min((q_last + hwk) // 64, nkt - 1) + 1
            nchunks = (kt_hi - kt_lo + tpc - 1) // tpc
            for item in range(G * nblk):
                rnd, gh, blk = item // NW, item // nblk, item % nblk
                for kvh_ in range(KV):
                    h = kvh_ * G + gh
                    src = h % KV if mutant == "kv_mod" else 0 if mutant == "kv_zero" else kvh_
                    qb0 = q0 + blk * 16
                    nq = min(16, ln - qb0)
                    ql = min(qb0 + 15, ln - 1)
                    bk_lo = max(qb0 - hwk, 0) // 64
                    bk_hi = min((ql + hwk) // 64, nkt - 1) + 1
                    tiles = list(range(max(bk_lo, kt_lo), min(bk_hi, kt_hi)))
                    if mutant == "skip_tile" and len(tiles) >= 2:
                        tiles = tiles[1:]
                    if mutant == "dup_tile" and len(tiles) >= 2:
                        tiles = tiles + tiles[-1:]
                    qi = torch.arange(qb0, qb0 + nq)[:, None]
                    qq = q[h, qb0:qb0 + nq]
                    m = torch.full((nq, 1), -1e30, dtype=torch.float32)
                    l = torch.zeros(nq, 1, dtype=torch.float32)
                    o = torch.zeros(nq, hd, dtype=torch.float32)
                    for kt in tiles:
                        dt = kt      # the tile whose K / V rows the LDS holds where tile kt is expected
                        if mutant == "stale_piece" and rnd >= 1 and nchunks > 1 and kt < kt_lo + tpc:
                            last0 = kt_lo + (nchunks - 1) * tpc
                            dt = min(last0 + (kt - kt_lo), kt_hi - 1) if last0 + (kt - kt_lo) < kt_hi else kt
                        key = torch.arange(kt * 64, kt * 64 + 64)[None, :]
                        st = qq @ k[src, dt * 64:dt * 64 + 64].t()
                        interior = kt * 64 >= qb0 + 15 - hwk and kt * 64 + 63 <= qb0 + hwk and kt * 64 + 63 < ln
                        if not interior:
                            valid = (key < ln) & (key >= qi - hwk - lo_d) & (key <= qi + hwk + hi_d)
                            st = st.masked_fill(~valid, float("-inf"))
                        m_new = torch.maximum(m, st.max(dim=-1, keepdim=True).values)
                        p = torch.exp2(st * c - m_new * c)
                        pb = p.to(torch.bfloat16).float()
                        alpha = torch.exp2((m - m_new) * c)
                        l = l * alpha + p.sum(-1, keepdim=True)
                        o = o * alpha + pb @ v[src, dt * 64:dt * 64 + 64]
                        m = m_new
                    out[r0 + qb0:r0 + qb0 + nq, h * hd:(h + 1) * hd] = (o * (1.0 / l)).to(torch.bfloat16)
        r0 += ln
    return out


# ---- the tanh-GELU gated product -------------------------------------------------------------------------------------------------------------------------
def glu_tanh_input(rows=64, F=256, seed=0):
    """bf16 [rows, 2F] = (up | gate): gate covers [-6, 6] densely — the negative tail is where the erf and tanh forms of GELU differ by several percent of
    their value (at x = -3: -0.00405 against -0.00364) —, up is N(0, 1)"""
    g = torch.Generator().manual_seed(500 + seed)
    up = torch.randn(rows, F, generator=g)
    gate = torch.linspace(-6.0, 6.0, rows * F).reshape(rows, F)[torch.randperm(rows, generator=g)]
    return torch.cat([up, gate], dim=1).to(torch.bfloat16)


def glu_tanh_reference(buf_bf16):
    """float64 up * gelu_tanh(gate) of a (up | gate) buffer -> (ref, gate) float64 [rows, F]"""
    F = buf_bf16.shape[1] // 2
    up, gate = buf_bf16[:, :F].double(), buf_bf16[:, F:].double()
    u = math.sqrt(2.0 / math.pi) * (gate + 0.044715 * gate ** 3)
    return up * gate * torch.sigmoid(2.0 * u), gate


def glu_tanh_budget(ref, gate):
    """Elementwise bound on |kernel - ref| for csrc/gemma.hip's glu_tanh_kernel, U = 2**-24:
      - the one rounding of the product to bf16: half a bf16 ulp of the value, 2**(floor(log2 |ref|) - 8);
      - the fp32 chain in front of it, relative to |ref|: u = c (x (1 + a x^2)) takes 5 roundings (x^2, a x^2, 1 + ., x ., c .) of terms of one sign, so
        |du / u| <= 5 U; t = exp(-2u) has |dt / t| <= 2 |u| 5 U + 2 U (expf within 2 ulp, generously); d(1 / (1 + t)) / (1 / (1 + t)) = t / (1 + t) dt / t
        <= |dt / t|; then 1 + t, the division, and the product with `up`: 3 U.  Together (10 |u| + 5) U |ref|."""
    U = 2.0 ** -24
    u = math.sqrt(2.0 / math.pi) * (gate + 0.044715 * gate ** 3)
    half_ulp = torch.where(ref != 0, torch.exp2(torch.floor(torch.log2(ref.abs().clamp(min=1e-300))) - 8.0), torch.zeros_like(ref))
    return half_ulp + (10.0 * u.abs() + 5.0) * U * ref.abs()


# ---- the tower: configs, weights, fp32 oracle ----------------------------------------------------------------------------------------------------------
_COMMON = dict(model_type="gemma3_text", vocab_size=300, hidden_size=128, num_attention_heads=2, num_key_value_heads=1, head_dim=256, intermediate_size=256,
               max_position_embeddings=512, rms_norm_eps=1e-6, hidden_activation="gelu_pytorch_tanh", query_pre_attn_scalar=256,
               use_bidirectional_attention=True, attn_logit_softcapping=None, final_logit_softcapping=None, pad_token_id=0, eos_token_id=1, bos_token_id=2,
               rope_theta=1000000.0, rope_local_base_freq=10000.0)
# on-disk spelling: sliding_window 8 -> half_window 4 (transformers: 8 // 2 + 1 = 5, |i - j| < 5)
TINY = dict(_COMMON, num_hidden_layers=3, sliding_window=8, sliding_window_pattern=3)                  # sliding, sliding, full
TINY_SLIDING = dict(_COMMON, num_hidden_layers=2, sliding_window=8, layer_types=["sliding_attention"] * 2)
TINY_FULL = dict(_COMMON, num_hidden_layers=2, sliding_window=8, layer_types=["full_attention"] * 2)
TINIES = {"TINY": TINY, "TINY_SLIDING": TINY_SLIDING, "TINY_FULL": TINY_FULL}

config_dict = Q.config_dict
state_dict_of = Q.state_dict_of
pad_batch = Q.pad_batch
random_seqs = Q.random_seqs


def hf_config(cfg: dict):
    import transformers
    kw = {k: v for k, v in cfg.items() if k != "model_type"}
    config = transformers.Gemma3TextConfig(**kw)
    config._attn_implementation = "eager"
    return config


def hf_model(cfg: dict, seed: int = 0, gain: float = 0.6):
    """transformers' Gemma3TextModel for the ON-DISK config dict: eager attention, fp32, eval, weights from `randomize`"""
    import transformers
    model = transformers.Gemma3TextModel(hf_config(cfg)).float().eval()
    randomize(model, seed, gain)
    return model


def randomize(model, seed, gain=0.6):
    """seeded weights with working magnitudes: Linear weights N(0, gain / sqrt(in)) — q_proj and k_proj x 2, so that the rotary phases and the band edge
    matter to the softmax —, every norm weight 0.1 N(0, 1) (applied as 1 + w: a dropped + 1 or a dropped norm is seen), token table 0.5 N(0, 1)"""
    g = torch.Generator().manual_seed(3000 + seed)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if p.ndim == 1:
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
            elif "embed_tokens" in name:
                p.copy_(0.5 * torch.randn(p.shape, generator=g))
            else:
                p.copy_(torch.randn(p.shape, generator=g) * (gain / math.sqrt(p.shape[1])))
                if name.endswith("q_proj.weight") or name.endswith("k_proj.weight"):
                    p.mul_(2.0)


def _rms(x, w, eps):
    return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * (1.0 + w)


def gelu_tanh(x):
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x.pow(3))))


def oracle_hidden(sd, arch, ids, mask=None):
    """The project's fp32 oracle of the tower: last hidden state [n, S, W] of right-padded ids [n, S] (mask [n, S] of 0 / 1, None = no padding; the rows of
    padded positions are computed but mean nothing).  `arch` = engine.archs.GemmaArch, `sd` = transformers' tensor names without prefix (norm weights as
    the checkpoint stores them: applied as 1 + w)."""
    n, S = ids.shape
    Qh, KV, hd = arch.heads, arch.kv_heads, arch.head_dim
    G = Qh // KV
    f = lambda k: sd[k].float()
    x = f("embed_tokens.weight")[ids] * torch.tensor(arch.width ** 0.5, dtype=torch.float32)
    pos = torch.arange(S, dtype=torch.float32)[:, None]
    trig = {}
    for local in (False, True):
        ang = pos * arch.inv_freq(local)[None, :]
        trig[local] = (torch.cat([ang, ang], -1).cos(), torch.cat([ang, ang], -1).sin())
    keys_ok = torch.ones(n, 1, 1, S, dtype=torch.bool) if mask is None else (mask != 0)[:, None, None, :]
    for l in range(arch.layers):
        p = f"layers.{l}."
        a = p + "self_attn."
        sliding = arch.sliding[l]
        cos, sin = trig[sliding]
        h = _rms(x, f(p + "input_layernorm.weight"), arch.rms_eps)
        q, k, v = (h @ f(a + f"{c}_proj.weight").t() for c in "qkv")
        q, k, v = q.reshape(n, S, Qh, hd).transpose(1, 2), k.reshape(n, S, KV, hd).transpose(1, 2), v.reshape(n, S, KV, hd).transpose(1, 2)
        q, k = _rms(q, f(a + "q_norm.weight"), arch.rms_eps), _rms(k, f(a + "k_norm.weight"), arch.rms_eps)
        q, k = q * cos + Q._rot_half(q) * sin, k * cos + Q._rot_half(k) * sin
        k, v = k.repeat_interleave(G, dim=1), v.repeat_interleave(G, dim=1)
        # (a padded query whose whole band is padding keeps its own key: its row means nothing, but it must stay finite — 0 x NaN is NaN in P @ V)
        ok = (keys_ok & band_allowed(S, arch.half_window if sliding else 0)[None, None]) | torch.eye(S, dtype=torch.bool)[None, None]
        s = (q @ k.transpose(2, 3) * arch.attn_scale).masked_fill(~ok, float("-inf"))
        at = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(n, S, Qh * hd)
        x = x + _rms(at @ f(a + "o_proj.weight").t(), f(p + "post_attention_layernorm.weight"), arch.rms_eps)
        h = _rms(x, f(p + "pre_feedforward_layernorm.weight"), arch.rms_eps)
        mlp = (gelu_tanh(h @ f(p + "mlp.gate_proj.weight").t()) * (h @ f(p + "mlp.up_proj.weight").t())) @ f(p + "mlp.down_proj.weight").t()
        x = x + _rms(mlp, f(p + "post_feedforward_layernorm.weight"), arch.rms_eps)
    return _rms(x, f("norm.weight"), arch.rms_eps)


def oracle_hidden_packed(sd, arch, seqs):
    """the packed form: every sequence (1-D ids) on its own, no padding anywhere -> list of [len, W]"""
    return [oracle_hidden(sd, arch, s[None])[0] for s in seqs]


def pooled(hidden_list, pooling="mean", normalize=True):
    """list of [len, W] -> float64 [n, W]: the first row or the mean of every sequence, L2-normalised when asked"""
    rows = torch.stack([(h[0].double() if pooling == "cls" else h.double().mean(0)) for h in hidden_list])
    return rows / rows.norm(dim=-1, keepdim=True) if normalize else rows


# ---- a checkpoint directory as a user brings it ---------------------------------------------------------------------------------------------------------
PAD, EOS, BOS = "<pad>", "<eos>", "<bos>"


def train_tokenizer(vocab_size=300):
    """a byte-level BPE `tokenizers.Tokenizer` trained from modernbert_ref.CORPUS in memory, <pad> / <eos> / <bos> as ids 0 / 1 / 2 and — as
    EmbeddingGemma's file — a TemplateProcessing that wraps a text in <bos> ... <eos>"""
    from tokenizers import Tokenizer, decoders, models, pre_tokenizers, processors, trainers
    from tests.modernbert_ref import CORPUS
    tk = Tokenizer(models.BPE(unk_token=None))
    tk.pre_tokenizer = pre_tokenizers.ByteLevel(add_prefix_space=False)
    tk.decoder = decoders.ByteLevel()
    trainer = trainers.BpeTrainer(vocab_size=vocab_size, special_tokens=[PAD, EOS, BOS], initial_alphabet=pre_tokenizers.ByteLevel.alphabet(), show_progress=False)
    tk.train_from_iterator(CORPUS * 4, trainer)
    tk.post_processor = processors.TemplateProcessing(single=f"{BOS} $A {EOS}", pair=f"{BOS} $A {EOS} $B:1 {EOS}:1", special_tokens=[(BOS, 2), (EOS, 1)])
    return tk


def write_checkpoint_dir(directory, model, tokenizer=None, pooling=None, dense=(), dense_bias=False, dense_activation="torch.nn.modules.linear.Identity"):
    """model.save_pretrained (config.json + model.safetensors) + tokenizer.json + tokenizer_config.json (+ 1_Pooling/config.json when `pooling` is 'mean'
    / 'cls'; + modules.json with Transformer, Pooling, one Dense module directory per weight [out, in] of `dense` — N_Dense/config.json +
    model.safetensors, as sentence-transformers writes them — and Normalize)"""
    from safetensors.torch import save_file
    os.makedirs(directory, exist_ok=True)
    model.save_pretrained(directory, safe_serialization=True)
    if tokenizer is not None:
        tokenizer.save(os.path.join(directory, "tokenizer.json"))
        with open(os.path.join(directory, "tokenizer_config.json"), "w") as f:
            json.dump({"pad_token": PAD, "eos_token": EOS, "bos_token": BOS}, f)
    W = model.config.hidden_size
    if pooling is not None:
        os.makedirs(os.path.join(directory, "1_Pooling"), exist_ok=True)
        with open(os.path.join(directory, "1_Pooling", "config.json"), "w") as f:
            json.dump({"word_embedding_dimension": W, "pooling_mode_cls_token": pooling == "cls", "pooling_mode_mean_tokens": pooling == "mean"}, f)
    if dense:
        mods = [{"idx": 0, "name": "0", "path": "", "type": "sentence_transformers.models.Transformer"},
                {"idx": 1, "name": "1", "path": "1_Pooling", "type": "sentence_transformers.models.Pooling"}]
        for i, wt in enumerate(dense):
            sub = f"{i + 2}_Dense"
            os.makedirs(os.path.join(directory, sub), exist_ok=True)
            with open(os.path.join(directory, sub, "config.json"), "w") as f:
                json.dump({"in_features": wt.shape[1], "out_features": wt.shape[0], "bias": dense_bias, "activation_function": dense_activation}, f)
            t = {"linear.weight": wt.contiguous()}
            if dense_bias:
                t["linear.bias"] = torch.zeros(wt.shape[0])
            save_file(t, os.path.join(directory, sub, "model.safetensors"))
            mods.append({"idx": i + 2, "name": str(i + 2), "path": sub, "type": "sentence_transformers.models.Dense"})
        mods.append({"idx": len(mods), "name": str(len(mods)), "path": f"{len(mods)}_Normalize", "type": "sentence_transformers.models.Normalize"})
        with open(os.path.join(directory, "modules.json"), "w") as f:
            json.dump(mods, f)
    return directory

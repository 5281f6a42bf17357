"""Helpers of the Mistral / Llama tests (tests/test_llama_host.py, tests/test_attention_gqa_window_gpu.py, tests/test_llama_rows_gpu.py,
tests/test_llama_gpu.py).  Nothing here calls the library.

  - the float64 reference of causal sliding-window grouped-query attention: tests/qwen_ref.py's gqa_reference under the mask transformers builds
    (masking_utils: sliding_window_overlay `kv_idx > q_idx - sliding_window` AND causal_mask_function `kv_idx <= q_idx`), on the budget, constants and input
    families of tests/attention_ref.py;
  - four tiny random checkpoints and the project's float64 oracle of the tower, written from the block equations of csrc/llama.hip and pinned to
    transformers' MistralModel / LlamaModel in float64 by tests/test_llama_host.py.  Tokenizer and checkpoint directory are tests/qwen_ref.py's.

Layout (the kernel's): `qkv` is bf16 [rows, (Q + 2 KV) hd] = (q | k | v); query head h reads K/V head h // (Q // KV)."""
import math

import torch

from tests import qwen_ref as Q

SLICE = Q.SLICE
LDS_KEYS = Q.LDS_KEYS


def window_allowed(ln, window, device="cpu"):
    """[query, key] boolean: query i sees key j iff i - window < j <= i (window None: causal)"""
    q = torch.arange(ln, device=device)[:, None]
    k = torch.arange(ln, device=device)[None, :]
    ok = k <= q
    return ok if window is None else ok & (k > q - window)


def gqa_window_reference(qkv_bf16, lens, q_heads, kv_heads, hd, window):
    """float64 attention on the device of `qkv_bf16` -> (out, absout) = (P V, P |V|), float64 [rows, Q hd]"""
    Qh, KV, G = q_heads, kv_heads, q_heads // kv_heads
    dev, rows = qkv_bf16.device, qkv_bf16.shape[0]
    assert qkv_bf16.dtype == torch.bfloat16 and qkv_bf16.shape[1] == (Qh + 2 * KV) * hd and rows == sum(lens) and Qh % KV == 0
    out = torch.zeros(rows, Qh * hd, dtype=torch.float64, device=dev)
    absout = torch.zeros(rows, Qh * hd, dtype=torch.float64, device=dev)
    kvh = torch.arange(Qh, device=dev) // G
    r0 = 0
    for ln in lens:
        q, k, v = Q.split_qkv(qkv_bf16[r0:r0 + ln].double(), Qh, KV, hd)
        s = (q @ k[kvh].transpose(1, 2) / math.sqrt(hd)).masked_fill(~window_allowed(ln, window, dev), float("-inf"))
        p = torch.softmax(s, dim=-1)
        out[r0:r0 + ln] = (p @ v[kvh]).transpose(0, 1).reshape(ln, Qh * hd)
        absout[r0:r0 + ln] = (p @ v[kvh].abs()).transpose(0, 1).reshape(ln, Qh * hd)
        r0 += ln
    return out, absout


# ---- the tower: configs, weights, float64 oracle -------------------------------------------------------------------------------------------------------
_COMMON = dict(vocab_size=300, num_hidden_layers=2, max_position_embeddings=512, rms_norm_eps=1e-5, hidden_act="silu", tie_word_embeddings=False,
               pad_token_id=0, bos_token_id=0, eos_token_id=0, rope_parameters={"rope_type": "default", "rope_theta": 10000.0})
M128 = dict(_COMMON, model_type="mistral", hidden_size=128, num_attention_heads=4, num_key_value_heads=2, head_dim=64, intermediate_size=192, sliding_window=48)
M2560 = dict(_COMMON, model_type="mistral", hidden_size=2560, num_attention_heads=4, num_key_value_heads=1, head_dim=128, intermediate_size=256,
             sliding_window=200)      # heads * head_dim = 512 != width
M4096 = dict(_COMMON, model_type="mistral", hidden_size=4096, num_attention_heads=2, num_key_value_heads=1, head_dim=128, intermediate_size=256,
             sliding_window=None)
L128 = dict(_COMMON, model_type="llama", hidden_size=128, num_attention_heads=2, num_key_value_heads=2, head_dim=64, intermediate_size=192,
            attention_bias=False, mlp_bias=False)
TINIES = {"M128": M128, "M2560": M2560, "M4096": M4096, "L128": L128}
LENGTHS = (1, 17, 70, 129, 300)


def hf_model(cfg: dict, seed: int = 0, dtype=torch.float64):
    """transformers' MistralModel / LlamaModel for the config dict: eager attention, eval, weights from qwen_ref.randomize"""
    import transformers
    kw = {k: v for k, v in cfg.items() if k != "model_type"}
    Config, Model = ((transformers.MistralConfig, transformers.MistralModel) if cfg["model_type"] == "mistral" else
                     (transformers.LlamaConfig, transformers.LlamaModel))
    config = Config(**kw)
    config._attn_implementation = "eager"
    model = Model(config).to(dtype).eval()
    Q.randomize(model, seed)
    return model


def _rms(x, g, eps):
    return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * g


def oracle_hidden(sd, arch, ids):
    """The project's float64 oracle of the tower on ONE unpadded sequence: ids [S] -> last hidden state [S, W].  `arch` = engine.archs.LlamaArch, `sd` =
    transformers' tensor names without prefix."""
    S = ids.shape[0]
    Qh, KV, hd = arch.heads, arch.kv_heads, arch.head_dim
    G = Qh // KV
    f = lambda k: sd[k].double()
    x = f("embed_tokens.weight")[ids]
    # (the rotary table is fp32 by definition: transformers' rotary module forms the angle, the cosine and the sine in float32 whatever the model's dtype)
    ang = torch.arange(S, dtype=torch.float32)[:, None] * arch.inv_freq()[None, :]
    cos, sin = torch.cat([ang, ang], -1).cos().double(), torch.cat([ang, ang], -1).sin().double()
    ok = window_allowed(S, arch.window)[None]
    for l in range(arch.layers):
        p = f"layers.{l}."
        a = p + "self_attn."
        h = _rms(x, f(p + "input_layernorm.weight"), arch.rms_eps)
        q, k, v = (h @ f(a + f"{c}_proj.weight").t() for c in "qkv")
        q, k, v = q.reshape(S, Qh, hd).transpose(0, 1), k.reshape(S, KV, hd).transpose(0, 1), v.reshape(S, KV, hd).transpose(0, 1)
        q, k = q * cos + Q._rot_half(q) * sin, k * cos + Q._rot_half(k) * sin
        k, v = k.repeat_interleave(G, dim=0), v.repeat_interleave(G, dim=0)
        s = (q @ k.transpose(1, 2) / math.sqrt(hd)).masked_fill(~ok, float("-inf"))
        at = (torch.softmax(s, -1) @ v).transpose(0, 1).reshape(S, Qh * hd)
        x = x + at @ f(a + "o_proj.weight").t()
        h = _rms(x, f(p + "post_attention_layernorm.weight"), arch.rms_eps)
        x = x + (h @ f(p + "mlp.up_proj.weight").t() * torch.nn.functional.silu(h @ f(p + "mlp.gate_proj.weight").t())) @ f(p + "mlp.down_proj.weight").t()
    return _rms(x, f("norm.weight"), arch.rms_eps)


_CACHE = {}


def tiny(name):
    """one tiny, built once per process and shared, never changed: cfg, float64 transformers model, arch, state dict, LENGTHS sequences, oracle rows"""
    if name not in _CACHE:
        from marqo_amd.engine import archs
        cfg = TINIES[name]
        with torch.no_grad():
            model = hf_model(cfg, seed=list(TINIES).index(name) + 1)
            arch = archs.llama_arch_from_hf_config(dict(cfg))
            sd = Q.state_dict_of(model)
            seqs = Q.random_seqs(list(LENGTHS), cfg["vocab_size"], seed=5)
            _CACHE[name] = dict(cfg=cfg, model=model, arch=arch, sd=sd, seqs=seqs, hidden=[oracle_hidden(sd, arch, s) for s in seqs])
    return _CACHE[name]


# ---- the token stream: float64 reference and rounding model of one mq_encode_llama pass, on the forms of tests/packed_text_ref.py -------------------------
def _stream_pass(arch, tensors, ids, lens, rounds, layers=None):
    """packed_text_ref._run's qwen form — the same helpers, the same stores (see that module's header) — without q / k norm and QKV bias and with the
    window: query i sees the keys j with i - window < j <= i, packed_text_ref._attention's causal band of hw = window - 1.  `tensors` = the loader's
    output (engine/tower_weights.py::qwen_state_dict).  -> packed_text_ref.Pass"""
    from tests import encoder_ref as E
    from tests import packed_text_ref as P
    dev = ids.device
    lens = [int(n) for n in lens]
    assert ids.dim() == 1 and ids.shape[0] == sum(lens) and min(lens) >= 1 and (arch.window is None or arch.window > 1)
    layers = arch.layers if layers is None else layers
    t = P.operands("qwen", tensors, dev)
    R = E._Round(P._FORM if rounds else None)
    mm = lambda x, w: E._mm(x, w, 0)
    W, F, Qh, KV, hd = arch.width, arch.mlp_dim, arch.heads, arch.kv_heads, arch.head_dim
    # (as mq_encode_llama: the band only when the window is smaller than the longest sequence of the call — the same keys either way)
    hw = arch.window - 1 if arch.window is not None and arch.window < max(lens) else 0
    pos = E._positions(lens, dev)
    ids = ids.long()
    norm = lambda x, g: P._rms(x, g, arch.rms_eps)
    freq = arch.inv_freq().to(dev)
    x = R.f(t["embed_tokens.weight"][ids])
    streams = []
    for l in range(layers):
        p = f"layers.{l}."
        a_ = p + "self_attn."
        qkv = R.b(mm(R.b(norm(x, t[p + "input_layernorm.weight"])), t[a_ + "qkv.weight"]))
        qkv = P._qk_step(qkv, pos, Qh, KV, hd, freq, R)
        a = P._attention(qkv, lens, Qh, KV, hd, 1.0 / math.sqrt(hd), True, hw, R)
        x = R.f(x + mm(a, t[a_ + "o_proj.weight"]))
        ug = R.b(mm(R.b(norm(x, t[p + "post_attention_layernorm.weight"])), t[p + "mlp.up_gate.weight"]))
        x = R.f(x + mm(R.b(ug[:, :F] * E._act(ug[:, F:], "silu")), t[p + "mlp.down_proj.weight"]))
        streams.append(x)
    final_g = t["norm.weight"]
    final = R.f(norm(x, final_g))
    first = torch.tensor([sum(lens[:i]) for i in range(len(lens))], device=dev)
    lasti = first + torch.tensor(lens, device=dev) - 1
    seq_of = torch.repeat_interleave(torch.arange(len(lens), device=dev), torch.tensor(lens, device=dev))
    sums = torch.zeros(len(lens), W, dtype=torch.float64, device=dev).index_add_(0, seq_of, final)
    pools = {"mean": R.f(sums / torch.tensor(lens, dtype=torch.float64, device=dev)[:, None]), "last": R.f(norm(x[lasti], final_g))}
    pooled = {}
    for name, rows in pools.items():
        pooled[(name, 0)] = rows
        pooled[(name, 1)] = R.f(rows / rows.norm(dim=-1, keepdim=True))
    return P.Pass(blocks=streams, final=final, pooled=pooled)


def stream_exact(arch, tensors, ids, lens, layers=None):
    return _stream_pass(arch, tensors, ids, lens, False, layers)


def stream_model(arch, tensors, ids, lens, layers=None):
    return _stream_pass(arch, tensors, ids, lens, True, layers)


_STREAM = {}


def stream_build(name):
    """the tiny as the stream tests run it: dict(arch, sd = the tiny's tensors with every Linear weight rounded to bf16 — what the tower stores —, tensors =
    the loader's output on that sd), built once"""
    if name not in _STREAM:
        from marqo_amd.engine import tower_weights as TW
        t = tiny(name)
        sd = {k: (v.to(torch.bfloat16).float() if (v.dim() == 2 and "embed_tokens" not in k) else v.float()) for k, v in t["sd"].items()}
        _STREAM[name] = dict(arch=t["arch"], sd=sd, tensors=TW.qwen_state_dict(t["arch"], sd))
    return _STREAM[name]

"""Mistral / Llama on the host (no GPU): the project's float64 oracle of the tower against transformers' MistralModel / LlamaModel in float64 (eager
attention, random weights from the four tiny configs of tests/llama_ref.py), the config parser and its refusals, the C ABI's argument checks with fake
pointers, the sharded safetensors loader, the `hf` dispatch through model_properties and the refusal of wide embeddings by combine.py.

Tolerance of the oracle comparison: both sides are float64 torch on the CPU computing the same graph; they differ by the association order of float64 sums.
ORACLE_ATOL = 1e-6, the bar of the sibling _ref files; the worst difference is printed as `LLAMA_ORACLE`."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from marqo_amd import _lib as L
from marqo_amd.engine import archs, checkpoint
from tests import llama_ref as LR
from tests import qwen_ref as Q

ORACLE_ATOL = 1e-6

# config.json of mistralai/Mistral-7B-v0.1 (the shape e5-mistral-7b-instruct, SFR-Embedding-Mistral and Linq-Embed-Mistral share) and of
# meta-llama/Llama-2-7b-hf: WRITTEN FROM MEMORY of the hub files, UNVERIFIED (no copy of either is at hand)
MISTRAL_7B = {"architectures": ["MistralModel"], "model_type": "mistral", "vocab_size": 32000, "hidden_size": 4096, "intermediate_size": 14336,
              "num_hidden_layers": 32, "num_attention_heads": 32, "num_key_value_heads": 8, "hidden_act": "silu", "max_position_embeddings": 32768,
              "rms_norm_eps": 1e-5, "rope_theta": 10000.0, "sliding_window": 4096, "tie_word_embeddings": False, "torch_dtype": "float16",
              "bos_token_id": 1, "eos_token_id": 2}
LLAMA2_7B = {"architectures": ["LlamaForCausalLM"], "model_type": "llama", "vocab_size": 32000, "hidden_size": 4096, "intermediate_size": 11008,
             "num_hidden_layers": 32, "num_attention_heads": 32, "num_key_value_heads": 32, "hidden_act": "silu", "max_position_embeddings": 4096,
             "rms_norm_eps": 1e-5, "rope_scaling": None, "attention_bias": False, "pretraining_tp": 1, "tie_word_embeddings": False, "bos_token_id": 1,
             "eos_token_id": 2}


# ---- the float64 oracle against transformers -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tuple(LR.TINIES))
def test_oracle_equals_transformers(name):
    t = LR.tiny(name)
    arch = t["arch"]
    assert isinstance(arch, archs.LlamaArch) and arch.window == t["cfg"].get("sliding_window") and not arch.qk_norm and not arch.qkv_bias
    worst = 0.0
    with torch.no_grad():
        for s, h in zip(t["seqs"], t["hidden"]):
            ref = t["model"](input_ids=s[None]).last_hidden_state[0]
            worst = max(worst, float((h - ref).abs().max()))
    print(f"LLAMA_ORACLE {name}: max |oracle - transformers| = {worst:.3e} over lengths {LR.LENGTHS} (bar {ORACLE_ATOL:.0e})")
    assert worst < ORACLE_ATOL
    if arch.window is not None:      # the window binds at these lengths: the causal oracle is far outside the bar, and so is a window off by one key
        s = t["seqs"][-1]
        for w in (None, arch.window + 1, arch.window - 1):
            other = LR.oracle_hidden(t["sd"], archs.LlamaArch(**{**arch.__dict__, "window": w}), s)
            assert float((other - t["hidden"][-1]).abs().max()) > 100 * ORACLE_ATOL, w


def test_window_mask_is_transformers_rule():
    """pins the tests' REFERENCE (llama_ref.window_allowed) to the installed transformers, not the library: it passes without the feature"""
    from transformers import masking_utils as MU
    fn = MU.sliding_window_causal_mask_function(5)
    ok = LR.window_allowed(12, 5)
    for i in range(12):
        for j in range(12):
            assert bool(fn(0, 0, torch.tensor(i), torch.tensor(j))) == bool(ok[i, j]), (i, j)
    assert bool(ok[7, 3]) and not bool(ok[7, 2]) and not bool(ok[7, 8])       # i - window < j <= i


# ---- the config parser -----------------------------------------------------------------------------------------------------------------------------------
def test_real_shaped_configs():
    a = archs.llama_arch_from_hf_config(MISTRAL_7B)
    assert a == archs.LlamaArch(vocab=32000, max_pos=8192, width=4096, layers=32, heads=32, kv_heads=8, head_dim=128, mlp_dim=14336, rms_eps=1e-5,
                                rope_theta=10000.0, window=4096)
    assert a == archs.LlamaArch()     # the defaults are this shape
    b = archs.llama_arch_from_hf_config(LLAMA2_7B)
    assert (b.width, b.heads, b.kv_heads, b.head_dim, b.mlp_dim, b.max_pos, b.window) == (4096, 32, 32, 128, 11008, 4096, None)
    c = archs.llama_arch_from_hf_config(dict(MISTRAL_7B, sliding_window=None, rope_theta=None, rope_parameters={"rope_type": "default", "rope_theta": 1e6}))
    assert c.window is None and c.rope_theta == 1e6
    assert abs(float(a.inv_freq()[1]) - 10000.0 ** (-2 / 128)) < 1e-7      # (fp32)
    assert a.gflop_per_text(512) > 0 and archs.LlamaArch(window=64).gflop_per_text(512) < archs.LlamaArch(window=None).gflop_per_text(512)


@pytest.mark.parametrize("over, what", [
    (dict(rope_scaling={"type": "linear", "factor": 2.0}), "rope_scaling="),
    (dict(rope_parameters={"rope_type": "llama3", "rope_theta": 500000.0, "factor": 8.0}), "rope_parameters.rope_type=llama3"),
    (dict(hidden_act="gelu"), "hidden_act=gelu"),
    (dict(attention_bias=True), "attention_bias=true"),
    (dict(mlp_bias=True), "mlp_bias=true"),
    (dict(head_dim=96), "head_dim=96"),
    (dict(hidden_size=4160, head_dim=128), "hidden_size=4160"),
    (dict(hidden_size=5120, head_dim=128), "hidden_size=5120"),
    (dict(intermediate_size=14000), "intermediate_size=14000"),
    (dict(num_key_value_heads=5), "num_key_value_heads=5"),
    (dict(sliding_window=0), "sliding_window=0"),
])
def test_refused_config_keys_are_named(over, what):
    with pytest.raises(KeyError, match=what):
        archs.llama_arch_from_hf_config(dict(MISTRAL_7B, **over))
    with pytest.raises(KeyError, match="not a Mistral / Llama model"):
        archs.llama_arch_from_hf_config(dict(MISTRAL_7B, model_type="mixtral"))
    with pytest.raises(KeyError, match="is not a BERT-family encoder"):      # the BERT-family parser (the cross-encoders' gate) keeps its refusal
        archs.bert_arch_from_hf_config(MISTRAL_7B)


# ---- the C ABI without a GPU -----------------------------------------------------------------------------------------------------------------------------
def test_entry_points_judge_their_arguments_before_any_launch():
    lib = L.load()
    fake = C.c_void_p(4096)

    def refused(rc, what, code=-1):
        assert rc == code and what in lib.mq_last_error(), (rc, lib.mq_last_error())
    win = lambda qkv=fake, out=fake, cu=fake, nseq=1, fl=0, mx=10, Qh=4, KV=2, hd=64, w=4: lib.mq_attention_gqa_window(qkv, out, cu, nseq, fl, mx, Qh, KV, hd, w, None)
    refused(win(qkv=None), b"mq_attention_gqa_window: null pointer")
    refused(win(out=None), b"mq_attention_gqa_window: null pointer")
    refused(win(hd=96), b"mq_attention_gqa_window: head_dim 96 unsupported")
    refused(win(Qh=6, KV=4), b"mq_attention_gqa_window: q_heads 6 must be a multiple of kv_heads 4")
    refused(win(w=0), b"mq_attention_gqa_window: window 0 must be at least 1")
    refused(win(w=-3), b"mq_attention_gqa_window: window -3")
    refused(win(cu=None), b"mq_attention_gqa_window: need fixed_len or cu_seqlens")
    refused(win(mx=8193), b"mq_attention_gqa_window: max sequence length 8193 unsupported")
    assert win(nseq=0) == 0          # nothing to do
    # the wide row kernels: multiples of 64 up to 4096; the narrow entry points keep their 2048
    refused(lib.mq_rmsnorm_wide(fake, None, fake, fake, None, 1, 4160, 1e-6, None), b"mq_rmsnorm_wide: W=4160 unsupported")
    refused(lib.mq_rmsnorm_wide(fake, None, fake, fake, None, 1, 2100, 1e-6, None), b"mq_rmsnorm_wide: W=2100 unsupported")
    refused(lib.mq_rmsnorm_wide(None, None, fake, fake, None, 1, 4096, 1e-6, None), b"mq_rmsnorm_wide: null pointer")
    refused(lib.mq_rmsnorm_wide(fake, None, fake, None, None, 1, 4096, 1e-6, None), b"mq_rmsnorm_wide: null pointer")
    refused(lib.mq_rmsnorm_wide(fake, None, fake, fake, None, 1 << 34, 4096, 1e-6, None), b"mq_rmsnorm_wide: grid too large")
    refused(lib.mq_rmsnorm(fake, None, fake, fake, None, 1, 4096, 1e-6, None), b"mq_rmsnorm: W=4096 unsupported")
    refused(lib.mq_embed_tokens_wide(fake, fake, 1, fake, fake, 4160, 10, None), b"mq_embed_tokens_wide: W=4160 unsupported")
    refused(lib.mq_embed_tokens_wide(fake, fake, 1, None, fake, 4096, 10, None), b"mq_embed_tokens_wide: null pointer")
    refused(lib.mq_embed_tokens_wide(fake, fake, 1, fake, fake, 4096, 0, None), b"mq_embed_tokens_wide: vocab 0")
    refused(lib.mq_pool_wide(fake, fake, 1, fake, 4160, 1, None), b"mq_pool_wide: W=4160 unsupported")
    refused(lib.mq_pool_wide(fake, None, 1, fake, 4096, 1, None), b"mq_pool_wide: null pointer")
    refused(lib.mq_pool(fake, fake, 1, fake, 4096, L.MQ_POOL_MEAN, 1, None), b"pool: W=4096 unsupported")
    # the tower
    assert C.sizeof(L.LlamaCfg) == 48
    mk = lambda **kw: L.LlamaCfg(**dict(dict(width=4096, layers=1, q_heads=32, kv_heads=8, head_dim=128, mlp_dim=14336, vocab=10, max_pos=64, pool=2, window=4096,
                                             rms_eps=1e-5), **kw))
    w = L.QwenWeights()
    enc = lambda cfg, w=w, ids=None, cu=None, hcu=None, nseq=0, out=fake, ws=None, nb=0: lib.mq_encode_llama(C.byref(cfg), C.byref(w), ids, cu, hcu, nseq, out, 1, ws, nb, None)
    for kw, what in ((dict(width=4160), b"width 4160 > 4096"), (dict(width=4100), b"width 4100 must be a multiple of 64"), (dict(head_dim=96), b"head_dim 96 unsupported"),
                     (dict(max_pos=9000), b"max_pos 9000"), (dict(mlp_dim=100), b"mlp_dim 100"), (dict(pool=1), b"bad pooling 1"),
                     (dict(q_heads=3), b"q_heads 3 must be a multiple"), (dict(window=-1), b"window -1")):
        refused(enc(mk(**kw)), b"mq_encode_llama: " + what)
    refused(lib.mq_encode_llama(None, C.byref(w), None, None, None, 0, fake, 1, None, 0, None), b"mq_encode_llama: null cfg")
    refused(lib.mq_encode_llama(C.byref(mk()), None, None, None, None, 0, fake, 1, None, 0, None), b"mq_encode_llama: null pointer")
    refused(enc(mk(), out=None), b"mq_encode_llama: null pointer")
    refused(enc(mk()), b"mq_encode_llama: null weight pointer")
    layers = (L.QwenLayer * 1)()
    full = L.QwenWeights(tok_emb=4096, final_norm_g=4096, zeros=4096, d_inv_freq=4096, layers=layers)
    refused(enc(mk(), w=full), b"mq_encode_llama: layer 0 has null weights")
    layers[0] = L.QwenLayer(input_norm_g=4096, qkv_w=4096, qkv_b=4096, out_w=4096, post_norm_g=4096, ug_w=4096, down_w=4096)
    refused(enc(mk(), w=full), b"mq_encode_llama: layer 0 carries a QKV bias or q / k norm weights")
    layers[0] = L.QwenLayer(input_norm_g=4096, qkv_w=4096, out_w=4096, post_norm_g=4096, ug_w=4096, down_w=4096)
    assert enc(mk(), w=full) == 0       # nseq = 0: nothing to do
    hcu = (C.c_int32 * 2)(0, 20)
    refused(enc(mk(), w=full, ids=None, cu=fake, hcu=hcu, nseq=1, ws=fake), b"mq_encode_llama: null input / workspace")
    refused(enc(mk(), w=full, ids=fake, cu=fake, hcu=(C.c_int32 * 2)(0, 65), nseq=1, ws=fake, nb=1 << 40), b"sequence lengths must be in [1, max_pos=64]")
    need = lib.mq_llama_workspace_bytes(C.byref(mk()), 20, 1)
    assert need >= 20 * (4096 * 6 + 2 * 14336 * 2 + 32 * 128 * 2) and lib.mq_llama_workspace_bytes(None, 20, 1) == 0
    refused(enc(mk(), w=full, ids=fake, cu=fake, hcu=hcu, nseq=1, ws=fake, nb=need - 1), b"mq_encode_llama: workspace", code=-3)
    assert lib.mq_abi_version() == 15


def test_torch_op_is_registered():
    ops = L.load_torch_ops()
    assert hasattr(ops, "mq_attention_gqa_window")
    with pytest.raises(NotImplementedError, match="'CPU' backend"):      # (registered for the GPU only: a CPU tensor fails in the dispatcher)
        ops.mq_attention_gqa_window(torch.zeros(4, 256, dtype=torch.bfloat16), torch.zeros(2, dtype=torch.int32), 4, 2, 1, 64, 2, torch.zeros(4, 128, dtype=torch.bfloat16))


# ---- the token-stream reference of the GPU test (tests/test_llama_forms_gpu.py) ---------------------------------------------------------------------------
def test_stream_reference_is_the_qwen_form_and_the_oracle():
    from tests import packed_text_ref as P
    for name in ("L128", "M128"):
        b = LR.stream_build(name)
        arch, lens = b["arch"], [1, 17, 70]
        seqs = Q.random_seqs(lens, arch.vocab, seed=7)
        ids = torch.cat(seqs)
        ex = LR.stream_exact(arch, b["tensors"], ids, lens)
        if arch.window is None:      # no window: packed_text_ref's qwen form runs the arch as it is — the same numbers, exact and rounded
            ref, mo, rmo = P.exact("qwen", arch, b["tensors"], ids, lens), LR.stream_model(arch, b["tensors"], ids, lens), P.model("qwen", arch, b["tensors"], ids, lens)
            assert torch.equal(ex.final, ref.final) and torch.equal(ex.blocks[0], ref.blocks[0]) and torch.equal(mo.final, rmo.final)
            assert all(torch.equal(ex.pooled[k], ref.pooled[k]) and torch.equal(mo.pooled[k], rmo.pooled[k]) for k in ex.pooled)
        # the transformers-pinned oracle on the same (bf16-rounded) weights; they differ by the rotary angle alone: float64 here, fp32 there
        worst, apart, r0 = 0.0, 0.0, 0
        causal = LR.stream_exact(archs.LlamaArch(**{**arch.__dict__, "window": None}), b["tensors"], ids, lens)
        for s in seqs:
            h = LR.oracle_hidden(b["sd"], arch, s)
            worst = max(worst, float((ex.final[r0:r0 + len(s)] - h).abs().max()))
            apart = max(apart, float((causal.final[r0:r0 + len(s)] - h).abs().max()))
            r0 += len(s)
        print(f"LLAMA_STREAM_REF {name}: max |stream_exact - oracle| = {worst:.3e} (bar 1e-4); the causal form against the windowed oracle {apart:.3e}")
        assert worst < 1e-4 and (arch.window is None or apart > 1e-2)


# ---- the sharded loader ----------------------------------------------------------------------------------------------------------------------------------
def test_sharded_checkpoint_loads_to_the_single_file_state_dict(tmp_path):
    t = LR.tiny("M128")
    single = Q.write_checkpoint_dir(str(tmp_path / "single"), t["cfg"], {"model." + k: v.float() for k, v in t["sd"].items()})
    sharded = str(tmp_path / "sharded")
    LR.hf_model(t["cfg"], seed=list(LR.TINIES).index("M128") + 1, dtype=torch.float32).save_pretrained(sharded, max_shard_size="200KB")     # (a fresh model: the cached tiny stays as it is)
    assert os.path.isfile(os.path.join(sharded, checkpoint.HF_SHARD_INDEX)) and not os.path.isfile(os.path.join(sharded, "model.safetensors"))
    with open(os.path.join(sharded, checkpoint.HF_SHARD_INDEX)) as f:
        shards = sorted(set(json.load(f)["weight_map"].values()))
    assert len(shards) >= 3
    assert checkpoint.find_hf_dir(sharded) == sharded
    strip = lambda sd: {(k[len("model."):] if k.startswith("model.") else k): v for k, v in sd.items()}
    _, a = checkpoint.load_hf_dir(single)
    cfg, b = checkpoint.load_hf_dir(sharded)
    a, b = strip(a), strip(b)
    assert cfg["model_type"] == "mistral" and set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)
    os.remove(os.path.join(sharded, shards[1]))
    with pytest.raises(checkpoint.ShardedCheckpointError, match=shards[1]):
        checkpoint.load_hf_dir(sharded)
    pickled = tmp_path / "pickled"
    pickled.mkdir()
    (pickled / "config.json").write_text(json.dumps(t["cfg"]))
    (pickled / checkpoint.HF_PICKLE_SHARD_INDEX).write_text(json.dumps({"weight_map": {}}))
    with pytest.raises(checkpoint.ShardedCheckpointError, match="pytorch_model.bin.index.json"):
        checkpoint.load_hf_dir(str(pickled))


# ---- the `hf` dispatch -----------------------------------------------------------------------------------------------------------------------------------
class _Captured(Exception):
    pass


def _model(props):
    from marqo_amd.s2_inference.hugging_face_model import HuggingFaceModel
    return HuggingFaceModel(model_properties=props, device="cuda:0")


def test_hf_loader_takes_mistral_and_llama_directories(tmp_path, monkeypatch):
    from marqo_amd.engine import llama as EL
    from marqo_amd.engine.tokenizers import HfJsonTokenizer
    from marqo_amd.s2_inference.errors import InvalidModelPropertiesError
    seen = {}

    def init(self, arch, sd, device, pooling="last", precision="bf16"):
        seen.update(arch=arch, sd=sd, pooling=pooling, precision=precision)
        raise _Captured()
    monkeypatch.setattr(EL.LlamaTower, "__init__", init)
    dirs = {}
    for name, pooling in (("M128", None), ("L128", "mean")):
        t = LR.tiny(name)
        dirs[name] = Q.write_checkpoint_dir(str(tmp_path / name), t["cfg"], {"model." + k: v.float() for k, v in t["sd"].items()}, Q.train_tokenizer(), pooling=pooling)
    for name, prop, want in (("M128", None, "last"), ("L128", None, "mean"), ("L128", "last", "last"), ("M128", "mean", "mean")):
        props = {"type": "hf", "name": dirs[name], "dimensions": 128, "tokens": 4096}
        if prop:
            props["poolingMethod"] = prop
        m = _model(props)
        with pytest.raises(_Captured):
            m._load_necessary_components()
        assert isinstance(seen["arch"], archs.LlamaArch) and seen["arch"] == LR.tiny(name)["arch"]
        assert isinstance(m._tokenizer, HfJsonTokenizer) and m._tokenizer.pad_id == 0 and m._tokenizer.cls_id is None
        assert seen["pooling"] == want and seen["precision"] == "bf16" and "model.embed_tokens.weight" in seen["sd"]
        assert m.model_properties.tokens == 512        # truncation at min(tokens, max_position_embeddings, 8192)
    d = dirs["M128"]
    with pytest.raises(InvalidModelPropertiesError, match="pooling_method 'cls' is not available for Mistral / Llama"):
        _model({"type": "hf", "name": d, "dimensions": 128, "poolingMethod": "cls"})._load_necessary_components()
    with pytest.raises(InvalidModelPropertiesError, match="'enginePrecision': 'fp8' is not available for Mistral / Llama"):
        _model({"type": "hf", "name": d, "dimensions": 128, "enginePrecision": "fp8"})._load_necessary_components()
    with pytest.raises(InvalidModelPropertiesError, match="'dimensions'=64 but the encoder width is 128"):
        _model({"type": "hf", "name": d, "dimensions": 64})._load_necessary_components()
    bad = Q.write_checkpoint_dir(str(tmp_path / "scaled"), dict(LR.M128, rope_scaling={"type": "linear", "factor": 2.0}), {"model.x": torch.zeros(1)}, Q.train_tokenizer())
    with pytest.raises(InvalidModelPropertiesError, match="rope_scaling="):
        _model({"type": "hf", "name": bad, "dimensions": 128})._load_necessary_components()


# ---- combine.py ------------------------------------------------------------------------------------------------------------------------------------------
def test_combine_refuses_wide_embeddings_by_name():
    from marqo_amd import combine
    for D in (2112, 4096):
        with pytest.raises(ValueError, match=f"embeddings of {D} dimensions are not served.*at most 2048.*weighted multimodal fields"):
            combine.combine_weighted(np.zeros((3, D), dtype=np.float32), [[(0, 1.0), (1, 2.0)]], combine.NORMALIZE)
        with pytest.raises(ValueError, match="are not served"):
            combine.combine_multimodal_fields([{"a": [0.0] * D, "b": [1.0] * D}], {"a": 1.0, "b": 2.0}, True)

"""Qwen3 / Qwen2 on the host (no GPU): the project's fp32 oracle of the tower against transformers' Qwen3Model / Qwen2Model (eager attention, fp32, random
weights from tiny configs), a tile-order arithmetic model of the grouped-query kernel whose deliberate faults leave the rounding budget of
tests/attention_ref.py, the loader (config parsing, refusals, pooling, tensor mapping) and the template-free mode of HfJsonTokenizer.

Tolerance of the oracle comparison: both sides are fp32 torch on the CPU computing the same graph; they differ by the association order of fp32 sums only.
Measured on right-padded batches of lengths [1, 17, 70] at the real rows: TINY3 1.43e-6, TINY2 0.0, TINY64 0.0 (|values| <= 4.4; transformers' own padded
and unpadded runs of one sequence differ by 2.1e-6).  ORACLE_ATOL = 3e-5 is 20 times the largest measurement."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from marqo_amd import _lib as L
from marqo_amd.engine import archs
from tests import attention_ref as AR
from tests import qwen_ref as Q

ORACLE_ATOL = 3e-5       # measured 1.43e-6 (TINY3), 0.0 (TINY2, TINY64)
# (q_heads, kv_heads, hd), packed lengths, mask: a subset of the GPU list (tests/test_attention_gqa_gpu.py) that shows every fault
SHAPES = [((4, 2, 128), [129, 1, 33], AR.MASK_CAUSAL), ((8, 1, 64), [63, 64, 65], AR.MASK_CAUSAL), ((14, 2, 64), [15, 16, 17], AR.MASK_NONE),
          ((4, 2, 128), [321], AR.MASK_CAUSAL), ((4, 4, 64), [641], AR.MASK_NONE), ((4, 2, 128), [127, 128, 129], AR.MASK_CAUSAL)]


@pytest.fixture(scope="module")
def models():
    return {k: Q.hf_model(cfg, seed=i + 1) for i, (k, cfg) in enumerate(Q.TINIES.items())}


# ---- the fp32 oracle against transformers ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tuple(Q.TINIES))
def test_oracle_equals_transformers(models, name):
    cfg, model = Q.TINIES[name], models[name]
    arch = archs.bert_arch_from_hf_config(cfg)
    assert isinstance(arch, archs.QwenArch) and arch.qk_norm == (cfg["model_type"] == "qwen3") and arch.qkv_bias == (cfg["model_type"] == "qwen2")
    seqs = Q.random_seqs([1, 17, 70], cfg["vocab_size"], seed=2)
    ids, mask = Q.pad_batch(seqs)
    with torch.no_grad():
        ref = model(input_ids=ids, attention_mask=mask).last_hidden_state
    got = Q.oracle_hidden(Q.state_dict_of(model), arch, ids, mask)
    d = max(float((got[i, :len(s)] - ref[i, :len(s)]).abs().max()) for i, s in enumerate(seqs))
    print(f"QWEN_ORACLE {name}: max |oracle - transformers| = {d:.3e} (bar {ORACLE_ATOL:.0e})")
    assert d < ORACLE_ATOL
    # the packed form (what the tower runs) gives the padded form's real rows: right padding cannot reach them under the causal mask
    for i, h in enumerate(Q.oracle_hidden_packed(Q.state_dict_of(model), arch, seqs)):
        assert float((h - got[i, :len(seqs[i])]).abs().max()) < ORACLE_ATOL
    # a dropped q_norm / k_norm, a dropped bias and the wrong K/V head are far outside the bar
    sd = Q.state_dict_of(model)
    if arch.qk_norm:
        ones = {k: torch.ones_like(v) if k.endswith("q_norm.weight") else v for k, v in sd.items()}
        assert float((Q.oracle_hidden(ones, arch, ids, mask)[2, :70] - ref[2, :70]).abs().max()) > 100 * ORACLE_ATOL
    else:
        nob = {k: torch.zeros_like(v) if k.endswith("k_proj.bias") else v for k, v in sd.items()}
        assert float((Q.oracle_hidden(nob, arch, ids, mask)[2, :70] - ref[2, :70]).abs().max()) > 100 * ORACLE_ATOL


# ---- the arithmetic model of the kernel and its faults -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cases():
    out = {}
    for i, (hs, lens, mask) in enumerate(SHAPES):
        qkv = Q.make_gqa_qkv("readout", lens, *hs, seed=3 + i)
        out[i] = (qkv, *Q.gqa_reference(qkv, lens, *hs, mask))
    return out


@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_arithmetic_model_stays_inside_the_budget(cases, i):
    hs, lens, mask = SHAPES[i]
    qkv, out, absout = cases[i]
    r = AR.worst_ratio(Q.emulate_gqa(qkv, lens, *hs, mask), out, absout)
    sharp = Q.make_gqa_qkv("peaked", lens, *hs, seed=30 + i)
    r2 = AR.worst_ratio(Q.emulate_gqa(sharp, lens, *hs, mask), *Q.gqa_reference(sharp, lens, *hs, mask))
    print(f"GQA_MODEL heads={hs} lens={lens} mask={mask} readout={r:.4f} peaked={r2:.4f}")
    assert r <= 1.0 and r2 <= 1.0


@pytest.mark.parametrize("mutant", Q.GQA_MUTANTS)
def test_every_fault_leaves_the_budget(cases, mutant):
    """each fault is far outside the margin the GPU test allows (1.25) on at least one of the shapes"""
    worst = 0.0
    for i, (hs, lens, mask) in enumerate(SHAPES):
        qkv, out, absout = cases[i]
        r = AR.worst_ratio(Q.emulate_gqa(qkv, lens, *hs, mask, mutant), out, absout)
        print(f"GQA_MUTANT {mutant} heads={hs} lens={lens} mask={mask} ratio={r:.1f}")
        worst = max(worst, r)
    assert worst > 50.0


def test_reference_equals_attention_ref_on_expanded_kv():
    """the float64 reference is attention_ref.reference on K/V copied to every query head of a group"""
    for hs, lens, mask in SHAPES[:3]:
        qkv = Q.make_gqa_qkv("randn", lens, *hs, seed=9)
        out, absout = Q.gqa_reference(qkv, lens, *hs, mask)
        o2, a2, _ = AR.reference(Q.expand_kv(qkv, *hs), lens, hs[0], hs[2], mask)
        assert float((out - o2).abs().max()) < 1e-12 and float((absout - a2).abs().max()) < 1e-12


# ---- the C ABI without a GPU -----------------------------------------------------------------------------------------------------------------------------
def test_entry_points_judge_their_arguments_before_any_launch():
    lib = L.load()
    fake = C.c_void_p(4096)

    def refused(rc, what):
        assert rc == -1 and what in lib.mq_last_error(), lib.mq_last_error()
    refused(lib.mq_attention_gqa(fake, fake, fake, 1, 0, 10, 4, 2, 96, 1, None), b"mq_attention_gqa: head_dim 96 unsupported")
    refused(lib.mq_attention_gqa(fake, fake, fake, 1, 0, 10, 6, 4, 64, 1, None), b"q_heads 6 must be a multiple of kv_heads 4")
    refused(lib.mq_attention_gqa(fake, fake, fake, 1, 0, 10, 4, 2, 64, L.MQ_MASK_CAUSAL_CLS, None), b"mask 2 unsupported")
    refused(lib.mq_attention_gqa(fake, fake, fake, 1, 0, 8193, 4, 2, 64, 1, None), b"max sequence length 8193 unsupported")
    refused(lib.mq_attention_gqa(fake, fake, None, 1, 0, 10, 4, 2, 64, 1, None), b"need fixed_len or cu_seqlens")
    assert lib.mq_attention_gqa(fake, fake, fake, 0, 0, 10, 4, 2, 64, 1, None) == 0          # nothing to do
    refused(lib.mq_rmsnorm(fake, None, fake, fake, None, 1, 2052, 1e-6, None), b"mq_rmsnorm: W=2052 unsupported")
    refused(lib.mq_qk_norm_rope(fake, fake, 1, 0, 4, 2, 96, None, None, 1e-6, fake, None), b"mq_qk_norm_rope: head_dim 96 unsupported")
    refused(lib.mq_qk_norm_rope(fake, fake, 1, 0, 4, 2, 64, fake, None, 1e-6, fake, None), b"come together or not at all")
    assert C.sizeof(L.QwenLayer) == 72 and C.sizeof(L.QwenWeights) == 40 and C.sizeof(L.QwenCfg) == 40 and L.MQ_POOL_LAST == 2
    w = L.QwenWeights()
    mk = lambda **kw: L.QwenCfg(**dict(dict(width=256, layers=1, q_heads=4, kv_heads=2, head_dim=128, mlp_dim=384, vocab=10, max_pos=64, pool=2, rms_eps=1e-6), **kw))
    for kw, what in ((dict(width=2560), b"width 2560 > 2048 (the 4B / 8B sizes"), (dict(head_dim=96), b"head_dim 96 unsupported"), (dict(max_pos=9000), b"max_pos 9000"),
                     (dict(mlp_dim=100), b"mlp_dim 100"), (dict(pool=1), b"bad pooling 1"), (dict(q_heads=3), b"q_heads 3 must be a multiple")):
        cfg = mk(**kw)
        refused(lib.mq_encode_qwen(C.byref(cfg), C.byref(w), None, None, None, 0, fake, 1, None, 0, None), b"mq_encode_qwen: " + what)
    assert lib.mq_abi_version() == 15


# ---- the loader ------------------------------------------------------------------------------------------------------------------------------------------
class _Captured(Exception):
    pass


@pytest.fixture(scope="module")
def ckpt(tmp_path_factory, models):
    d = str(tmp_path_factory.mktemp("qwen3"))
    Q.write_checkpoint_dir(d, Q.TINY3, Q.state_dict_of(models["TINY3"]), Q.train_tokenizer())
    return d


def _model(props):
    from marqo_amd.s2_inference.hugging_face_model import HuggingFaceModel
    return HuggingFaceModel(model_properties=props, device="cuda:0")


def _capture(monkeypatch):
    from marqo_amd.engine import qwen as EQ
    seen = {}

    def init(self, arch, sd, device, pooling="last", precision="bf16"):
        seen.update(arch=arch, sd=sd, pooling=pooling, precision=precision)
        raise _Captured()
    monkeypatch.setattr(EQ.QwenTower, "__init__", init)
    return seen


def test_hf_loader_takes_a_qwen3_directory(ckpt, tmp_path, monkeypatch, models):
    from marqo_amd.engine.tokenizers import HfJsonTokenizer
    from marqo_amd.s2_inference.errors import InvalidModelPropertiesError
    seen = _capture(monkeypatch)
    mean_dir = Q.write_checkpoint_dir(str(tmp_path / "mean"), Q.TINY3, Q.state_dict_of(models["TINY3"]), Q.train_tokenizer(), pooling="mean")
    last_dir = Q.write_checkpoint_dir(str(tmp_path / "last"), Q.TINY3, Q.state_dict_of(models["TINY3"]), Q.train_tokenizer(), pooling="last")
    for d, prop, want in ((ckpt, None, "last"), (mean_dir, None, "mean"), (last_dir, None, "last"), (mean_dir, "last", "last"), (ckpt, "mean", "mean")):
        props = {"type": "hf", "name": d, "dimensions": 256, "tokens": 4096}
        if prop:
            props["poolingMethod"] = prop
        m = _model(props)
        with pytest.raises(_Captured):
            m._load_necessary_components()
        assert isinstance(seen["arch"], archs.QwenArch) and seen["arch"] == archs.bert_arch_from_hf_config(Q.TINY3)
        assert isinstance(m._tokenizer, HfJsonTokenizer) and m._tokenizer.pad_id == 0 and m._tokenizer.cls_id is None
        assert seen["pooling"] == want and seen["precision"] == "bf16" and "embed_tokens.weight" in seen["sd"]
        assert m.model_properties.tokens == 256        # truncation at min(tokens, max_position_embeddings, 8192)
    with pytest.raises(InvalidModelPropertiesError, match="pooling_method 'cls' is not available for Qwen3 / Qwen2"):
        _model({"type": "hf", "name": ckpt, "dimensions": 256, "poolingMethod": "cls"})._load_necessary_components()
    with pytest.raises(InvalidModelPropertiesError, match="'enginePrecision': 'fp8' is not available for Qwen3 / Qwen2"):
        _model({"type": "hf", "name": ckpt, "dimensions": 256, "enginePrecision": "fp8"})._load_necessary_components()
    with pytest.raises(InvalidModelPropertiesError, match="'dimensions'=64 but the encoder width is 256"):
        _model({"type": "hf", "name": ckpt, "dimensions": 64})._load_necessary_components()
    with pytest.raises(InvalidModelPropertiesError, match="pooling_method must be 'mean' or 'cls'"):
        _model({"type": "hf", "name": ckpt, "dimensions": 256, "poolingMethod": "first"})


def test_cross_encoders_keep_refusing_the_family(ckpt):
    from marqo_amd.engine.rerank import CrossEncoderTower
    with pytest.raises(ValueError, match="model_type='qwen3' is not served as a cross-encoder"):
        CrossEncoderTower.from_dir(ckpt, "cuda:0")


def test_last_pooling_stays_refused_for_a_bert_directory(tmp_path):
    from marqo_amd.s2_inference.errors import InvalidModelPropertiesError
    d = str(tmp_path / "bert")
    os.makedirs(d)
    cfg = {"model_type": "bert", "vocab_size": 30, "max_position_embeddings": 32, "hidden_size": 64, "num_hidden_layers": 1, "num_attention_heads": 1,
           "intermediate_size": 128}
    with open(os.path.join(d, "config.json"), "w") as f:
        json.dump(cfg, f)
    from safetensors.torch import save_file
    save_file({"embeddings.word_embeddings.weight": torch.zeros(30, 64)}, os.path.join(d, "model.safetensors"))
    with open(os.path.join(d, "vocab.txt"), "w") as f:
        f.write("\n".join(["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"] + [f"w{i}" for i in range(25)]))
    with pytest.raises(InvalidModelPropertiesError, match="Original error pooling_method must be 'mean' or 'cls'"):
        _model({"type": "hf", "name": d, "dimensions": 64, "poolingMethod": "last"})._load_necessary_components()


@pytest.mark.parametrize("over,what", (
    (dict(rope_scaling={"type": "yarn", "factor": 4.0}), "rope_scaling="), (dict(rope_parameters={"rope_type": "yarn", "rope_theta": 1e6}), "rope_type=yarn"),
    (dict(use_sliding_window=True), "use_sliding_window=true"), (dict(layer_types=["full_attention", "sliding_attention", "full_attention"]), "layer_types="),
    (dict(hidden_act="gelu"), "hidden_act=gelu"), (dict(hidden_size=2560), "hidden_size=2560"), (dict(head_dim=96), "head_dim=96"),
    (dict(num_key_value_heads=3), "num_key_value_heads=3"), (dict(intermediate_size=100), "intermediate_size=100")))
def test_refused_config_keys_are_named(over, what):
    with pytest.raises(KeyError, match=what):
        archs.bert_arch_from_hf_config(Q.config_dict(Q.TINY3, **over))


def test_config_spellings():
    a = archs.bert_arch_from_hf_config(Q.config_dict(Q.TINY3, rope_parameters=None, rope_theta=5000.0, head_dim=None, num_attention_heads=2, rope_scaling=None))
    assert a.rope_theta == 5000.0 and a.head_dim == 128 and a.heads == 2 and a.kv_heads == 2
    assert archs.bert_arch_from_hf_config(Q.config_dict(Q.TINY2, attention_bias=False)).qkv_bias is False
    assert archs.bert_arch_from_hf_config(Q.config_dict(Q.TINY3, attention_bias=True)).qkv_bias is True
    assert archs.bert_arch_from_hf_config(Q.config_dict(Q.TINY3, max_position_embeddings=40960)).max_pos == 8192
    with pytest.raises(KeyError, match="is not a BERT-family encoder"):      # the other families keep their refusal
        archs.bert_arch_from_hf_config({"model_type": "mistral"})


@pytest.mark.parametrize("name", ("TINY3", "TINY2"))
def test_tensor_mapping_and_the_fused_row_order(models, name):
    from marqo_amd.engine.tower_weights import qwen_state_dict
    cfg, model = Q.TINIES[name], models[name]
    arch = archs.bert_arch_from_hf_config(cfg)
    sd = Q.state_dict_of(model)
    t = qwen_state_dict(arch, sd)
    a, F = "layers.1.self_attn.", arch.mlp_dim
    assert torch.equal(t[a + "qkv.weight"], torch.cat([sd[a + "q_proj.weight"], sd[a + "k_proj.weight"], sd[a + "v_proj.weight"]]))
    assert torch.equal(t["layers.1.mlp.up_gate.weight"][:F], sd["layers.1.mlp.up_proj.weight"]) and torch.equal(t["layers.1.mlp.up_gate.weight"][F:], sd["layers.1.mlp.gate_proj.weight"])
    assert ((a + "qkv.bias") in t) == arch.qkv_bias and ((a + "q_norm.weight") in t) == arch.qk_norm
    if arch.qkv_bias:
        assert torch.equal(t[a + "qkv.bias"], torch.cat([sd[a + "q_proj.bias"], sd[a + "k_proj.bias"], sd[a + "v_proj.bias"]]))
    seqs = Q.random_seqs([33], 300, seed=4)
    ref = Q.oracle_hidden_packed(sd, arch, seqs)[0]
    assert float((Q.oracle_hidden(t, arch, seqs[0][None], kernel_glu=True)[0] - ref).abs().max()) < ORACLE_ATOL
    pre = qwen_state_dict(arch, dict(Q.state_dict_of(model, "model."), **{"lm_head.weight": torch.zeros(2, 2)}))
    assert pre.keys() == t.keys() and all(torch.equal(pre[k], t[k]) for k in t)
    swapped = dict(sd)
    swapped["layers.1.mlp.up_proj.weight"], swapped["layers.1.mlp.gate_proj.weight"] = sd["layers.1.mlp.gate_proj.weight"], sd["layers.1.mlp.up_proj.weight"]
    moved = Q.oracle_hidden(qwen_state_dict(arch, swapped), arch, seqs[0][None], kernel_glu=True)[0]
    assert float((moved - ref).abs().max()) > 100 * ORACLE_ATOL
    with pytest.raises(KeyError, match="missing tensor 'layers.2.mlp.down_proj.weight'"):
        qwen_state_dict(arch, {k: v for k, v in sd.items() if k != "layers.2.mlp.down_proj.weight"})
    if not arch.qkv_bias:
        with pytest.raises(ValueError, match="attention_bias=false"):
            qwen_state_dict(arch, dict(sd, **{a + "q_proj.bias": torch.zeros(512)}))


# ---- the tokenizer -----------------------------------------------------------------------------------------------------------------------------------------
TEXTS = ["hello world", "", "a search engine ranks documents for a query " * 6, "naïve café, 12 + 3 = 15!", "<|endoftext|> inside"]


@pytest.mark.parametrize("append_eos", (True, False))
def test_plain_mode_gives_the_ids_of_pretrained_tokenizer_fast(tmp_path, append_eos):
    from transformers import PreTrainedTokenizerFast
    from marqo_amd.engine.tokenizers import HfJsonTokenizer
    d = str(tmp_path)
    Q.train_tokenizer(append_eos=append_eos).save(os.path.join(d, "tokenizer.json"))
    tok = HfJsonTokenizer.plain(d)         # no tokenizer_config.json: the pad token falls back to <|endoftext|>
    assert tok.pad_id == 0
    fast = PreTrainedTokenizerFast(tokenizer_file=os.path.join(d, "tokenizer.json"), pad_token=Q.EOS)
    for m in (12, 3, 64):
        want = fast(TEXTS, padding=True, truncation=True, max_length=m, return_tensors="np")
        got = tok(TEXTS, max_length=m)
        assert got["input_ids"].tolist() == want["input_ids"].tolist() and got["attention_mask"].tolist() == want["attention_mask"].tolist(), m
        lens = got["attention_mask"].sum(1)
        assert int(lens.max()) == min(m, int(lens.max())) and int(lens[2]) == m      # the long text is truncated to m
        if append_eos:       # the appended end token survives truncation, and the empty text is the end token alone
            assert all(got["input_ids"][i, lens[i] - 1] == 0 for i in range(len(TEXTS))) and int(lens[1]) == 1
        else:
            assert int(lens[1]) == 0
    with open(os.path.join(d, "tokenizer_config.json"), "w") as f:
        json.dump({"pad_token": {"content": "!"}}, f)
    assert HfJsonTokenizer.plain(d).pad_id == tok.tk.token_to_id("!")
    with open(os.path.join(d, "tokenizer_config.json"), "w") as f:
        json.dump({"pad_token": "<no such token>"}, f)
    with pytest.raises(ValueError, match="lacks the pad token"):
        HfJsonTokenizer.plain(d)


def test_template_mode_is_what_it_was(tmp_path):
    """HfJsonTokenizer(directory) on a ModernBERT-style file: [CLS] ... [SEP] rows, and a Qwen-style file is still refused there"""
    from tokenizers import Tokenizer
    from tests import modernbert_ref as M
    from marqo_amd.engine.tokenizers import HfJsonTokenizer
    d = str(tmp_path / "mb")
    os.makedirs(d)
    M.train_tokenizer().save(os.path.join(d, "tokenizer.json"))
    tok = HfJsonTokenizer(d)
    raw = Tokenizer.from_file(os.path.join(d, "tokenizer.json"))
    raw.enable_truncation(max_length=12)
    got = tok(TEXTS[:4], max_length=12)
    for i, t in enumerate(TEXTS[:4]):
        w = raw.encode(t).ids
        assert got["input_ids"][i, :len(w)].tolist() == w and w[0] == tok.cls_id == 1 and w[-1] == tok.sep_id == 2 and tok.pad_id == 0
    q = str(tmp_path / "qw")
    os.makedirs(q)
    Q.train_tokenizer().save(os.path.join(q, "tokenizer.json"))
    with pytest.raises(ValueError, match="lacks the special tokens"):
        HfJsonTokenizer(q)

"""ModernBERT on the host (no GPU): the window's edge as transformers draws it, the project's fp32 oracle of the tower against transformers'
ModernBertModel (eager attention, fp32, random weights from a tiny config), an arithmetic model of the band kernel whose deliberate faults leave the
rounding budget of tests/attention_ref.py, and the loader (config parsing, refusals, tensor mapping, tokenizer.json).

Tolerance of the oracle comparison: both sides are fp32 torch on the CPU computing the same graph; they differ by the order of fp32 sums only
(measured at most 9.5e-7 at |values| <= 4.2 after 4 blocks of K <= 192 GEMMs and nine LayerNorms; 1.1e-5 on a draw of weights 2.5 times larger).
ORACLE_ATOL = 2e-5 is 20 times the measurement — room for other BLAS builds' summation orders, still fp32 round-off at these magnitudes (~40 ulp of
4.2) — and four orders below what a wrong rotary base, window edge or MLP half moves (asserted below: more than 100 x ORACLE_ATOL)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from marqo_amd import _lib as L
from marqo_amd.engine import archs
from marqo_amd.engine.tower_weights import modernbert_state_dict
from tests import attention_ref as AR
from tests import modernbert_ref as M

ORACLE_ATOL = 2e-5
PACK = [1, 63, 64, 65, 128, 129, 193, 200]

CONFIGS = {
    # layer kinds from the default "every third" rule (full, sliding, sliding, full), default rotary bases
    "default": M.config_dict(),
    # the older spelling: global_attn_every_n_layers and the two theta keys, no layer_types / rope_parameters
    "old_keys": M.config_dict(global_attn_every_n_layers=2, global_rope_theta=50000.0, local_rope_theta=5000.0),
    # the newer spelling, and a layer_types list that is not "every third"
    "new_keys": M.config_dict(layer_types=["sliding_attention", "sliding_attention", "full_attention", "sliding_attention"],
                              rope_parameters={"full_attention": {"rope_type": "default", "rope_theta": 80000.0},
                                               "sliding_attention": {"rope_type": "default", "rope_theta": 2000.0}}),
}


@pytest.fixture(scope="module")
def models():
    return {k: M.hf_model(cfg, seed=i) for i, (k, cfg) in enumerate(CONFIGS.items())}


# ---- the window's edge ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("j", (0, 7, 20, 39))
def test_window_edge_is_inclusive_and_symmetric_in_transformers(j):
    """local_attention = 16: changing token j moves the first sliding layer's output at exactly the rows |i - j| <= 8"""
    cfg = M.config_dict(layer_types=["sliding_attention", "full_attention", "sliding_attention", "full_attention"])
    model = M.hf_model(cfg, seed=3).double()      # (fp64: a key with a probability of 1e-9 still moves its row)
    ids = M.random_seqs([40], cfg["vocab_size"], seed=1)[0][None]
    other = ids.clone()
    other[0, j] = (ids[0, j] + 17) % (cfg["vocab_size"] - 3) + 3
    with torch.no_grad():
        a = model(input_ids=ids, output_hidden_states=True).hidden_states[1][0]
        b = model(input_ids=other, output_hidden_states=True).hidden_states[1][0]
    moved = ((a - b).abs().max(dim=-1).values > 0).nonzero().flatten().tolist()
    assert moved == [i for i in range(40) if abs(i - j) <= 8], (j, moved)
    assert archs.bert_arch_from_hf_config(cfg).half_window == 8 and M.window_allowed(40, 8)[:, j].nonzero().flatten().tolist() == moved


# ---- the fp32 oracle against transformers ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CONFIGS))
def test_oracle_equals_transformers(models, name):
    cfg, model = CONFIGS[name], models[name]
    arch = archs.bert_arch_from_hf_config(cfg)
    assert arch == archs.bert_arch_from_hf_config(json.loads(json.dumps(model.config.to_dict())))      # the raw dict and transformers' own dump parse alike
    assert list(arch.sliding) == [t == "sliding_attention" for t in model.config.layer_types]
    assert arch.theta_global == model.config.rope_parameters["full_attention"]["rope_theta"]
    assert arch.theta_local == model.config.rope_parameters["sliding_attention"]["rope_theta"]
    if name == "default":
        assert arch.sliding == (False, True, True, False) and (arch.theta_global, arch.theta_local) == (160000.0, 10000.0)
    sd = M.state_dict_of(model)
    seqs = M.random_seqs([5, 40, 200, 17, 1], cfg["vocab_size"], seed=2)
    ids, mask = M.pad_batch(seqs)
    with torch.no_grad():
        ref = model(input_ids=ids, attention_mask=mask).last_hidden_state
    padded = M.oracle_hidden(sd, arch, ids, mask)
    packed = M.oracle_hidden_packed(sd, arch, seqs)
    for i, s in enumerate(seqs):
        e1 = float((padded[i, :len(s)] - ref[i, :len(s)]).abs().max())
        e2 = float((packed[i] - ref[i, :len(s)]).abs().max())
        print(f"MODERNBERT_ORACLE {name} len={len(s)} padded={e1:.2e} packed={e2:.2e} max|ref|={float(ref[i, :len(s)].abs().max()):.2f}")
        assert e1 < ORACLE_ATOL and e2 < ORACLE_ATOL
    # the oracle tells the variants apart: the wrong rotary base for the sliding layers moves it by far more than the tolerance
    from dataclasses import replace
    wrong = M.oracle_hidden_packed(sd, replace(arch, theta_local=arch.theta_global), seqs[2:3])[0]
    assert float((wrong - ref[2]).abs().max()) > 100 * ORACLE_ATOL


# ---- the band kernel's arithmetic model ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def readout_cases():
    """(hw, lens) -> (qkv, out, absout) of the read-out-V family: the packed batch at the three half-windows, one 705-token sequence at 64"""
    cases = {}
    for hw, lens in ((64, PACK), (8, PACK), (1, PACK), (64, [705])):
        qkv = AR.make_qkv("readout", lens, 2, 64, seed=hw + sum(lens))
        cases[(hw, tuple(lens))] = (qkv, *M.window_reference(qkv, lens, 2, hw))
    return cases


@pytest.mark.parametrize("hw,lens", ((64, PACK), (8, PACK), (1, PACK), (64, [705])))
def test_arithmetic_model_stays_inside_the_budget(readout_cases, hw, lens):
    qkv, out, absout = readout_cases[(hw, tuple(lens))]
    r = AR.worst_ratio(M.emulate_window(qkv, lens, 2, hw), out, absout)
    print(f"WINDOW_MODEL readout hw={hw} lens={lens} ratio={r:.4f}")
    assert r <= 1.0
    if lens == PACK:
        sharp = AR.make_qkv("peaked", lens, 2, 64, seed=hw)
        o2, a2 = M.window_reference(sharp, lens, 2, hw)
        r2 = AR.worst_ratio(M.emulate_window(sharp, lens, 2, hw), o2, a2)
        print(f"WINDOW_MODEL peaked hw={hw} ratio={r2:.4f}")
        assert r2 <= 1.0


@pytest.mark.parametrize("mutant", M.WINDOW_MUTANTS)
@pytest.mark.parametrize("hw,lens", ((64, PACK), (8, PACK), (1, PACK), (64, [705])))
def test_every_fault_leaves_the_budget(readout_cases, hw, lens, mutant):
    """one wrong key is visible on the read-out-V inputs the GPU test uses, at the margin the GPU test allows (1.25)"""
    qkv, out, absout = readout_cases[(hw, tuple(lens))]
    r = AR.worst_ratio(M.emulate_window(qkv, lens, 2, hw, mutant), out, absout)
    print(f"WINDOW_MUTANT {mutant} hw={hw} lens={lens} ratio={r:.1f}")
    assert r > 10.0


def test_full_window_is_full_attention():
    lens = [130, 7]
    qkv = AR.make_qkv("randn", lens, 2, 64, seed=5)
    out, absout, _ = AR.reference(qkv, lens, 2, 64, AR.MASK_NONE)
    o2, a2 = M.window_reference(qkv, lens, 2, 129)
    assert torch.equal(out, o2) and torch.equal(absout, a2)


# ---- the C ABI without a GPU -------------------------------------------------------------------------------------------------------------------------------
def test_window_entry_point_judges_its_arguments_before_any_launch():
    lib = L.load()
    fake = C.c_void_p(4096)

    def refused(rc, what):
        assert rc == -1 and what in lib.mq_last_error(), lib.mq_last_error()
    refused(lib.mq_attention_window(fake, fake, fake, 1, 0, 10, 96, 1, 4, None), b"mq_attention_window: 64-wide heads only")
    refused(lib.mq_attention_window(fake, fake, None, 1, 0, 10, 64, 1, 4, None), b"need fixed_len or cu_seqlens")
    refused(lib.mq_attention_window(fake, fake, fake, 1, 0, 10, 64, 1, -1, None), b"half_window -1 < 0")
    refused(lib.mq_attention_window(fake, fake, fake, 1, 0, 9000, 64, 1, 4, None), b"max sequence length 9000 unsupported")
    assert lib.mq_attention_window(fake, fake, fake, 0, 0, 10, 64, 1, 4, None) == 0          # nothing to do
    assert C.sizeof(L.ModernBertLayer) == 56 and C.sizeof(L.ModernBertWeights) == 56 and C.sizeof(L.ModernBertCfg) == 40
    cfg = L.ModernBertCfg(width=128, layers=1, heads=4, mlp_dim=192, vocab=10, max_pos=64, half_window=8, pool=0, ln_eps=1e-5)
    w = L.ModernBertWeights()
    refused(lib.mq_encode_modernbert(C.byref(cfg), C.byref(w), None, None, None, 0, fake, 1, None, 0, None), b"mq_encode_modernbert: 64-wide heads only")
    assert lib.mq_abi_version() == 15


# ---- the loader --------------------------------------------------------------------------------------------------------------------------------------------
class _Captured(Exception):
    pass


@pytest.fixture(scope="module")
def ckpt(tmp_path_factory, models):
    d = str(tmp_path_factory.mktemp("modernbert"))
    M.write_checkpoint_dir(d, CONFIGS["default"], M.state_dict_of(models["default"]), M.train_tokenizer())
    return d


def _model(props):
    from marqo_amd.s2_inference.hugging_face_model import HuggingFaceModel
    return HuggingFaceModel(model_properties=props, device="cuda:0")


def test_hf_loader_takes_a_modernbert_directory(ckpt, monkeypatch):
    from marqo_amd.engine import modernbert as EM
    from marqo_amd.engine.tokenizers import HfJsonTokenizer
    seen = {}

    def init(self, arch, sd, device, pooling="mean", precision="bf16"):
        seen.update(arch=arch, sd=sd, pooling=pooling, precision=precision)
        raise _Captured()
    monkeypatch.setattr(EM.ModernBertTower, "__init__", init)
    for pooling in ("mean", "cls"):
        m = _model({"type": "hf", "localpath": ckpt, "dimensions": 128, "poolingMethod": pooling, "tokens": 4096})
        with pytest.raises(_Captured):
            m._load_necessary_components()
        assert isinstance(seen["arch"], archs.ModernBertArch) and seen["arch"] == archs.bert_arch_from_hf_config(CONFIGS["default"])
        assert isinstance(m._tokenizer, HfJsonTokenizer) and seen["pooling"] == pooling and seen["precision"] == "bf16"
        assert "embeddings.tok_embeddings.weight" in seen["sd"] and m.model_properties.tokens == 256      # truncation at max_position_embeddings


def test_hf_loader_refusals(ckpt, tmp_path, monkeypatch, models):
    from marqo_amd.engine import modernbert as EM
    from marqo_amd.s2_inference.errors import InvalidModelPropertiesError
    monkeypatch.setattr(EM.ModernBertTower, "__init__", lambda *a, **k: (_ for _ in ()).throw(AssertionError("a refused checkpoint reached the tower")))
    with pytest.raises(InvalidModelPropertiesError, match="'enginePrecision': 'fp8' is not available for ModernBERT"):
        _model({"type": "hf", "localpath": ckpt, "dimensions": 128, "enginePrecision": "fp8"})._load_necessary_components()
    with pytest.raises(InvalidModelPropertiesError, match="'dimensions'=64 but the encoder width is 128"):
        _model({"type": "hf", "localpath": ckpt, "dimensions": 64})._load_necessary_components()
    narrow = M.write_checkpoint_dir(str(tmp_path / "narrow"), M.config_dict(num_attention_heads=4), M.state_dict_of(models["default"]), M.train_tokenizer())
    with pytest.raises(InvalidModelPropertiesError, match="64-wide attention heads only: hidden_size / num_attention_heads = 128 / 4 is not 64"):
        _model({"type": "hf", "localpath": narrow, "dimensions": 128})._load_necessary_components()
    for key in ("norm_bias", "attention_bias", "mlp_bias"):
        with pytest.raises(KeyError, match=f"{key}=true"):
            archs.bert_arch_from_hf_config(M.config_dict(**{key: True}))
    with pytest.raises(KeyError, match="rope_type=yarn"):
        archs.bert_arch_from_hf_config(M.config_dict(rope_parameters={"full_attention": {"rope_type": "yarn", "rope_theta": 1.0}}))
    with pytest.raises(KeyError, match="is not a BERT-family encoder"):      # the other families keep their refusal
        archs.bert_arch_from_hf_config({"model_type": "deberta-v2"})


def test_tensor_mapping_and_the_order_of_wi(models):
    """the loader's tensors, used as the kernels use them (up * gelu(gate) over (up | gate) = Wi rows), give the module's numbers — with or without a
    `model.` prefix — and swapping two checkpoint tensors moves them"""
    model, arch = models["default"], archs.bert_arch_from_hf_config(CONFIGS["default"])
    sd = M.state_dict_of(model)
    seqs = M.random_seqs([33], 300, seed=4)
    ref = M.oracle_hidden_packed(sd, arch, seqs)[0]
    t = modernbert_state_dict(arch, sd)
    F = arch.mlp_dim
    assert torch.equal(t["layers.2.mlp.Wi.weight"], torch.cat([sd["layers.2.mlp.Wi.weight"][F:], sd["layers.2.mlp.Wi.weight"][:F]]))
    assert "layers.0.attn_norm.weight" not in t and "layers.1.attn_norm.weight" in t
    got = M.oracle_hidden(t, arch, seqs[0][None], kernel_glu=True)[0]
    assert float((got - ref).abs().max()) < ORACLE_ATOL
    assert float((M.oracle_hidden(sd, arch, seqs[0][None], kernel_glu=True)[0] - ref).abs().max()) > 100 * ORACLE_ATOL      # un-swapped halves are visible
    pre = modernbert_state_dict(arch, dict(M.state_dict_of(model, "model."), **{"head.dense.weight": torch.zeros(2, 2)}))
    assert pre.keys() == t.keys() and all(torch.equal(pre[k], t[k]) for k in t)
    for a, b in (("layers.1.attn.Wo.weight", "layers.2.attn.Wo.weight"), ("layers.1.attn_norm.weight", "layers.1.mlp_norm.weight"),
                 ("embeddings.norm.weight", "final_norm.weight")):
        sw = dict(sd)
        sw[a], sw[b] = sd[b], sd[a]
        moved = M.oracle_hidden(modernbert_state_dict(arch, sw), arch, seqs[0][None], kernel_glu=True)[0]
        assert float((moved - ref).abs().max()) > 100 * ORACLE_ATOL, (a, b)
    with pytest.raises(KeyError, match="missing tensor 'layers.3.mlp.Wo.weight'"):
        modernbert_state_dict(arch, {k: v for k, v in sd.items() if k != "layers.3.mlp.Wo.weight"})
    with pytest.raises(ValueError, match="bias tensors"):
        modernbert_state_dict(arch, dict(sd, **{"layers.0.attn.Wo.bias": torch.zeros(128)}))


def test_tokenizer_json_gives_the_ids_of_the_tokenizers_library(ckpt):
    from tokenizers import Tokenizer
    from marqo_amd.engine.tokenizers import HfJsonTokenizer
    tok = HfJsonTokenizer(ckpt)
    raw = Tokenizer.from_file(os.path.join(ckpt, "tokenizer.json"))
    texts = ["hello world", "", "sliding window attention keeps long documents cheap " * 3, "naïve café, 12 + 3 = 15!", "[MASK] a [SEP] b"]
    for max_length in (None, 12, 3):
        if max_length:
            raw.enable_truncation(max_length=max_length)
        else:
            raw.no_truncation()
        want = [raw.encode(t).ids for t in texts]
        got = tok(texts, max_length=max_length)
        S = max(len(w) for w in want)
        assert got["input_ids"].shape == (len(texts), S) and got["input_ids"].dtype == np.int64
        for i, w in enumerate(want):
            assert got["input_ids"][i, :len(w)].tolist() == w and got["attention_mask"][i].tolist() == [1] * len(w) + [0] * (S - len(w))
            assert (got["input_ids"][i, len(w):] == tok.pad_id).all() and w[0] == tok.cls_id == 1 and w[-1] == tok.sep_id == 2
        if max_length:
            assert max(len(w) for w in want) == max_length
    assert tok("hello world")["input_ids"].shape[0] == 1

"""NomicBERT on the host: the config parser in both dialects and every refusal by its key, nomic_bert_state_dict on both tensor namings, the float64
restatement of the tower (tests/nomic_bert_ref.py::exact) against transformers' NomicBertModel in float64, the ctypes mirrors and the argument checks of
the C ABI (no GPU is touched: refusals return before any launch), the loader branch and the cross-encoder refusal.

  `exact` against float64 transformers on the packed lengths 1, 2, 17, 64: 1e-6 of max(1, |value|) on every element of the last hidden state, the bar
  tests/test_deberta_host.py holds its float64 pin to.  The known cause of a difference: transformers forms cos / sin of the rotary angle in fp32
  (6e-8) where `exact` takes them in float64 from the same fp32 angle.  Measured here: worst 2.0e-8 (NOMIC_EXACT lines).
  The orchestration mutants against the bar of the GPU test (4.0 x the float64 bf16 model's own error) on the host, smallest view:
  rope_skipped 85, rope_on_v 519, gate_swapped 121, gelu_for_silu 34, ln_before_add 1105, no_type_row 1312, theta_10000 88 (NOMIC_MUTANT lines);
  the model's second rounding history 1.19.
"""
import ctypes as C
import json
import os

import pytest
import torch

from marqo_amd import _lib as L
from marqo_amd.engine import archs, tower_weights as TW
from tests import nomic_bert_ref as N
from tests.test_patch_attn_gpu import MARGIN


# ---- the config parser --------------------------------------------------------------------------------------------------------------------------------
def test_bert_arch_from_hf_config_returns_a_nomic_bert_arch():
    """(raises KeyError: model_type=nomic_bert is not a BERT-family encoder, on the commit before this family was served)"""
    a = archs.bert_arch_from_hf_config({"model_type": "nomic_bert", "hidden_size": 768, "num_hidden_layers": 12, "num_attention_heads": 12,
                                        "intermediate_size": 3072, "vocab_size": 30528})
    assert isinstance(a, archs.NomicBertArch)
    assert (a.width, a.layers, a.heads, a.head_dim, a.mlp_dim, a.vocab, a.max_pos, a.rope_theta, a.ln_eps) == (768, 12, 12, 64, 3072, 30528, 2048, 1000.0, 1e-12)


def test_both_config_dialects_give_the_same_arch():
    a = archs.bert_arch_from_hf_config(N.native_config())
    b = archs.bert_arch_from_hf_config(N.hub_config())
    assert a == b and isinstance(b, archs.NomicBertArch)
    assert (a.width, a.layers, a.heads, a.mlp_dim, a.vocab, a.max_pos, a.type_vocab, a.rope_theta) == (128, 2, 2, 192, 384, 2048, 2, 1000.0)
    # the config transformers itself writes
    from transformers import NomicBertConfig
    c = archs.bert_arch_from_hf_config(NomicBertConfig(**N.TINY).to_dict())
    assert c == a
    # theta from either dialect; n_inner null is GPT-2's 4 n_embd
    assert archs.bert_arch_from_hf_config(N.native_config(rope_parameters={"rope_theta": 500.0, "rope_type": "default"})).rope_theta == 500.0
    assert archs.bert_arch_from_hf_config(N.hub_config(rotary_emb_base=500)).rope_theta == 500.0
    assert archs.bert_arch_from_hf_config(N.hub_config(n_inner=None)).mlp_dim == 512
    want = 1.0 / (1000.0 ** (torch.arange(0, 64, 2).float() / 64))
    assert torch.equal(a.inv_freq(), want) and a.inv_freq().dtype == torch.float32


def test_max_position_embeddings_is_clamped_to_8192():
    assert archs.bert_arch_from_hf_config(N.native_config(max_position_embeddings=32768)).max_pos == 8192
    assert archs.bert_arch_from_hf_config(N.hub_config(n_positions=32768)).max_pos == 8192
    assert archs.bert_arch_from_hf_config(N.native_config(max_position_embeddings=8192)).max_pos == 8192
    assert archs.bert_arch_from_hf_config(N.native_config(max_position_embeddings=512)).max_pos == 512


@pytest.mark.parametrize("over, what", (
    (dict(hidden_act="gelu"), "hidden_act=gelu"),
    (dict(rope_parameters={"rope_theta": 1000.0, "rope_type": "dynamic", "factor": 2.0}), "rope_parameters.rope_type=dynamic"),
    (dict(rope_parameters={"rope_theta": 1000.0, "rope_type": "linear", "factor": 2.0}), "rope_parameters.rope_type=linear"),
    (dict(head_dim=32), "head_dim=32"),
    (dict(num_attention_heads=4), "hidden_size=128 / num_attention_heads=4"),
    (dict(hidden_size=2112, num_attention_heads=33), "hidden_size=2112 unsupported"),
    (dict(intermediate_size=100), "intermediate_size=100"),
    (dict(moe_every_n_layers=2), "moe_every_n_layers=2"),
    (dict(num_experts=8), "num_experts=8"),
))
def test_native_dialect_refuses_by_key(over, what):
    with pytest.raises(KeyError, match=what.replace("(", "\\(")):
        archs.bert_arch_from_hf_config(N.native_config(**over))


@pytest.mark.parametrize("over, what", (
    (dict(qkv_proj_bias=True), "qkv_proj_bias=True"),
    (dict(mlp_fc1_bias=True), "mlp_fc1_bias=True"),
    (dict(mlp_fc2_bias=True), "mlp_fc2_bias=True"),
    (dict(prenorm=True), "prenorm=True"),
    (dict(use_rms_norm=True), "use_rms_norm=True"),
    (dict(rotary_emb_fraction=0.5), "rotary_emb_fraction=0.5"),
    (dict(rotary_emb_interleaved=True), "rotary_emb_interleaved=True"),
    (dict(rotary_scaling_factor=2), "rotary_scaling_factor=2"),
    (dict(activation_function="gelu"), "activation_function=gelu"),
    (dict(moe_every_n_layers=2), "moe_every_n_layers=2"),
    (dict(num_experts=8), "num_experts=8"),
    (dict(n_head=4), "hidden_size=128 / num_attention_heads=4"),
    (dict(n_embd=2112, n_head=33), "hidden_size=2112 unsupported"),
))
def test_hub_dialect_refuses_by_key(over, what):
    with pytest.raises(KeyError, match=what):
        archs.bert_arch_from_hf_config(N.hub_config(**over))


def test_neighbours_of_the_new_branch_keep_their_paths():
    with pytest.raises(KeyError, match="model_type=nomic_bert_v9 is not a BERT-family encoder"):
        archs.bert_arch_from_hf_config(dict(N.native_config(), model_type="nomic_bert_v9"))
    with pytest.raises(KeyError, match="is not a NomicBERT model"):
        archs.nomic_bert_arch_from_hf_config({"model_type": "bert"})
    plain = archs.bert_arch_from_hf_config(dict(model_type="bert", vocab_size=100, max_position_embeddings=64, hidden_size=128, num_hidden_layers=1,
                                                num_attention_heads=2, intermediate_size=256))
    assert isinstance(plain, archs.BertArch)


# ---- nomic_bert_state_dict ---------------------------------------------------------------------------------------------------------------------------
def test_the_two_tensor_namings_give_byte_identical_tensors():
    b = N.build()
    arch, W, F = b["arch"], 128, 192
    t_native = TW.nomic_bert_state_dict(arch, b["sd"])
    t_hub = TW.nomic_bert_state_dict(arch, b["hub_sd"])
    assert set(t_native) == set(t_hub) and len(t_native) == 4 + 8 * arch.layers
    for k in t_native:
        assert t_native[k].dtype == torch.float32 and torch.equal(t_native[k].view(torch.int32), t_hub[k].view(torch.int32)), k
    # ... and what save_pretrained writes (the hub's names, by the library's own reversed conversion mapping) gives them too
    for prefix in ("nomic_bert.", "bert."):
        t_pref = TW.nomic_bert_state_dict(arch, {prefix + k: v for k, v in b["sd"].items()})
        assert all(torch.equal(t_pref[k], t_native[k]) for k in t_native)
    sd = b["sd"]
    assert torch.equal(t_native["layer.1.attn.qkv.weight"], torch.cat([sd[f"layers.1.self_attn.{c}_proj.weight"] for c in "qkv"], 0))
    assert torch.equal(t_native["layer.0.mlp.up_gate.weight"][:F], sd["layers.0.mlp.up_proj.weight"])         # (up | gate): mq_glu's order
    assert torch.equal(t_native["layer.0.mlp.up_gate.weight"][F:], sd["layers.0.mlp.gate_proj.weight"])
    assert torch.equal(t_hub["layer.0.mlp.up_gate.weight"][:F], b["hub_sd"]["encoder.layers.0.mlp.fc11.weight"])  # fc11 = up, fc12 = gate
    assert torch.equal(t_native["type0"], sd["embeddings.token_type_embeddings.weight"][0])
    assert t_native["layer.0.mlp.down.weight"].shape == (W, F)


def test_save_pretrained_writes_the_hubs_names_and_they_load(tmp_path):
    from safetensors.torch import load_file
    b = N.build()
    d = N.save_pretrained_dir(str(tmp_path / "sp"), b["model"])
    sd = load_file(os.path.join(d, "model.safetensors"))
    assert "encoder.layers.0.attn.Wqkv.weight" in sd and "emb_ln.weight" in sd
    with open(os.path.join(d, "config.json")) as f:
        cfg = json.load(f)
    arch = archs.bert_arch_from_hf_config(cfg)
    assert arch == b["arch"]
    t = TW.nomic_bert_state_dict(arch, sd)
    assert all(torch.equal(t[k], b["tensors"][k]) for k in b["tensors"])


@pytest.mark.parametrize("naming", ("native", "hub"))
def test_missing_misshaped_and_bias_tensors_are_named(naming):
    b = N.build()
    arch = b["arch"]
    sd = b["sd"] if naming == "native" else b["hub_sd"]
    names = dict(native=("layers.1.mlp.down_proj", "layers.0.self_attn.o_proj", "layers.1.post_mlp_layernorm", "layers.0.self_attn.k_proj",
                         "embeddings.LayerNorm"),
                 hub=("encoder.layers.1.mlp.fc2", "encoder.layers.0.attn.out_proj", "encoder.layers.1.norm2", "encoder.layers.0.attn.Wqkv", "emb_ln"))[naming]
    down, o, ln2, qk, eln = names
    for key in (down + ".weight", ln2 + ".bias", eln + ".weight", "embeddings.token_type_embeddings.weight"):
        with pytest.raises(KeyError, match=f"missing tensor '{key}'"):
            TW.nomic_bert_state_dict(arch, {k: v for k, v in sd.items() if k != key})
    with pytest.raises(ValueError, match=f"'{down}.weight' has shape \\(192, 128\\), expected \\(128, 192\\)"):
        TW.nomic_bert_state_dict(arch, dict(sd, **{down + ".weight": sd[down + ".weight"].t().contiguous()}))
    with pytest.raises(ValueError, match=f"'{qk}.weight' has shape"):
        TW.nomic_bert_state_dict(arch, dict(sd, **{qk + ".weight": sd[qk + ".weight"][:64]}))
    for lin in (o, down, qk):
        with pytest.raises(ValueError, match=f"'{lin}.bias' is unexpected"):
            TW.nomic_bert_state_dict(arch, dict(sd, **{lin + ".bias": torch.zeros(128)}))


# ---- exact against transformers -----------------------------------------------------------------------------------------------------------------------
def test_exact_is_transformers_in_float64():
    """the packed lengths 1, 2, 17, 64: each sequence alone through NomicBertModel.double() (no padding, no mask), every row of the last hidden state"""
    b = N.build()
    m = b["model"].double()
    try:
        seqs = N.random_seqs(N.PIN_LENS, b["cfg"]["vocab_size"], seed=5)
        ex = N.exact(b["arch"], b["tensors"], torch.cat(seqs), N.PIN_LENS)
        worst, r0 = 0.0, 0
        for s in seqs:
            with torch.no_grad():
                ref = m(input_ids=s[None]).last_hidden_state[0]
            assert ref.dtype == torch.float64
            got = ex.final[r0:r0 + len(s)]
            err = float(((got - ref).abs() / ref.abs().clamp(min=1.0)).max())
            print(f"NOMIC_EXACT len={len(s)}: worst |exact - transformers| / max(1, |value|) = {err:.2e}")
            worst = max(worst, err)
            r0 += len(s)
        assert float(ex.final.abs().max()) > 1.0           # (working magnitudes: the comparison is not between two zeros)
        assert worst <= 1e-6, worst
    finally:
        m.float()


def test_exact_pools_as_the_reference_pipeline_pools():
    b = N.build()
    lens = [len(s) for s in b["seqs"]]
    ex = N.exact(b["arch"], b["tensors"], torch.cat(b["seqs"]), lens)
    r0 = 0
    for i, ln in enumerate(lens):
        rows = ex.final[r0:r0 + ln]
        assert torch.allclose(ex.pooled[("mean", 0)][i], rows.mean(0), rtol=0, atol=1e-12) and torch.equal(ex.pooled[("cls", 0)][i], rows[0])
        assert torch.allclose(ex.pooled[("mean", 1)][i], rows.mean(0) / rows.mean(0).norm(), rtol=0, atol=1e-12)
        r0 += ln


@pytest.fixture(scope="module")
def passes():
    b = N.build()
    lens = [len(s) for s in b["seqs"]]
    ids = torch.cat(b["seqs"])
    return dict(b=b, lens=lens, ids=ids, ex=N.exact(b["arch"], b["tensors"], ids, lens), mo=N.model(b["arch"], b["tensors"], ids, lens))


def _views(p, other):
    rs = {"stream": N.row_ratio(other.final, p["ex"].final, p["mo"].final)["ratio"]}
    rs.update({f"{k[0]}/l2={k[1]}": N.row_ratio(v, p["ex"].pooled[k], p["mo"].pooled[k])["ratio"] for k, v in other.pooled.items()})
    return rs


def test_second_rounding_history_is_inside_the_bar(passes):
    rs = _views(passes, N.model(passes["b"]["arch"], passes["b"]["tensors"], passes["ids"], passes["lens"], hist=1))
    print("NOMIC_HIST " + " ".join(f"{k}={v:.2f}" for k, v in rs.items()))
    assert max(rs.values()) <= MARGIN


@pytest.mark.parametrize("mut", N.MUTANTS)
def test_every_orchestration_mutant_leaves_the_bar(passes, mut):
    rs = _views(passes, N.model(passes["b"]["arch"], passes["b"]["tensors"], passes["ids"], passes["lens"], mut=mut))
    print(f"NOMIC_MUTANT {mut}: " + " ".join(f"{k}={v:.1f}" for k, v in rs.items()))
    assert min(rs.values()) > MARGIN, (mut, rs)


# ---- the C ABI without a GPU --------------------------------------------------------------------------------------------------------------------------
def test_struct_sizes_and_argument_checks():
    assert C.sizeof(L.NomicBertLayer) == 64 and C.sizeof(L.NomicBertWeights) == 56 and C.sizeof(L.NomicBertCfg) == 40      # the static_assert of csrc/nomic_bert.hip
    src = (L.CSRC_DIR / "nomic_bert.hip").read_text()
    assert "sizeof(mq_nomic_bert_layer) == 64 && sizeof(mq_nomic_bert_weights) == 56 && sizeof(mq_nomic_bert_cfg) == 40" in src
    lib = L.load()
    fake = C.c_void_p(4096)

    def refused(rc, what):
        assert rc == -1 and what in lib.mq_last_error(), lib.mq_last_error()
    af = lib.mq_attention_full
    refused(af(None, fake, fake, 1, 0, 10, 2, 64, 0.125, None), b"mq_attention_full: null pointer")
    refused(af(fake, None, fake, 1, 0, 10, 2, 64, 0.125, None), b"mq_attention_full: null pointer")
    refused(af(fake, fake, fake, 1, 0, 10, 2, 128, 0.125, None), b"mq_attention_full: head_dim 128 unsupported")
    refused(af(fake, fake, fake, 1, 0, 10, 2, 96, 0.125, None), b"mq_attention_full: head_dim 96 unsupported")
    refused(af(fake, fake, fake, 1, 0, 10, 0, 64, 0.125, None), b"heads 0 outside [1, 1024]")
    refused(af(fake, fake, fake, 1, 0, 10, 2, 64, 0.0, None), b"scale 0 must be positive")
    refused(af(fake, fake, fake, 1, 0, 10, 2, 64, -1.0, None), b"scale -1 must be positive")
    refused(af(fake, fake, None, 1, 0, 10, 2, 64, 0.125, None), b"need fixed_len or cu_seqlens")
    refused(af(fake, fake, fake, 1, 0, 8193, 2, 64, 0.125, None), b"max sequence length 8193 unsupported")
    refused(af(fake, fake, None, 1, 8193, 0, 2, 64, 0.125, None), b"max sequence length 8193 unsupported")
    refused(af(fake, fake, fake, 1, 0, 0, 2, 64, 0.125, None), b"max sequence length 0 unsupported")
    refused(af(fake, fake, fake, 1 << 31, 0, 1, 1, 64, 0.125, None), b"grid too large")
    assert af(fake, fake, fake, 0, 0, 10, 2, 64, 0.125, None) == 0          # nseq 0: nothing to do
    w = L.NomicBertWeights()
    mk = lambda **kw: L.NomicBertCfg(**dict(dict(width=128, layers=1, heads=2, head_dim=64, mlp_dim=256, vocab=10, max_pos=64, pool=L.MQ_POOL_MEAN, ln_eps=1e-12), **kw))
    for kw, what in ((dict(head_dim=128, heads=1), b"head_dim 128 unsupported"), (dict(width=2112, heads=33), b"width 2112"), (dict(width=100), b"width 100"),
                     (dict(heads=3), b"heads 3 x 64 is not the width 128"), (dict(mlp_dim=100), b"mlp_dim 100"), (dict(max_pos=9000), b"max_pos 9000"),
                     (dict(pool=L.MQ_POOL_LAST), b"bad pooling 2")):
        cfg = mk(**kw)
        refused(lib.mq_encode_nomic_bert(C.byref(cfg), C.byref(w), None, None, None, 0, fake, 1, None, 0, None), b"mq_encode_nomic_bert: " + what)
    cfg = mk()
    refused(lib.mq_encode_nomic_bert(C.byref(cfg), None, fake, fake, fake, 1, fake, 1, fake, 0, None), b"mq_encode_nomic_bert: null pointer")
    refused(lib.mq_encode_nomic_bert(C.byref(cfg), C.byref(w), fake, fake, fake, 1, fake, 1, fake, 0, None), b"mq_encode_nomic_bert: null weight pointer")
    layers = (L.NomicBertLayer * 1)(L.NomicBertLayer(*([4096] * 8)))
    full = dict(tok_emb=4096, type0=4096, emb_ln_g=4096, emb_ln_b=4096, zeros=4096, d_inv_freq=4096)
    w = L.NomicBertWeights(layers=layers, **full)
    assert lib.mq_encode_nomic_bert(C.byref(cfg), C.byref(w), None, None, None, 0, fake, 1, None, 0, None) == 0      # nseq 0: nothing to do
    for missing in ("zeros", "d_inv_freq", "type0"):
        w1 = L.NomicBertWeights(layers=layers, **{k: v for k, v in full.items() if k != missing})
        refused(lib.mq_encode_nomic_bert(C.byref(cfg), C.byref(w1), fake, fake, fake, 1, fake, 1, fake, 0, None), b"mq_encode_nomic_bert: null weight pointer")
    holed = (L.NomicBertLayer * 1)(L.NomicBertLayer(*([4096] * 7)))
    w2 = L.NomicBertWeights(layers=holed, **full)
    refused(lib.mq_encode_nomic_bert(C.byref(cfg), C.byref(w2), fake, fake, fake, 1, fake, 1, fake, 0, None), b"layer 0 has null weights")
    cu = (C.c_int32 * 3)(0, 5, 12)
    refused(lib.mq_encode_nomic_bert(C.byref(cfg), C.byref(w), None, fake, cu, 2, fake, 1, fake, 1 << 20, None), b"mq_encode_nomic_bert: null input / workspace")
    need = lib.mq_nomic_bert_workspace_bytes(C.byref(cfg), 12, 2)
    assert need >= 12 * 128 * 4 and lib.mq_nomic_bert_workspace_bytes(None, 12, 2) == 0 and lib.mq_nomic_bert_workspace_bytes(C.byref(cfg), 0, 2) == 0
    assert lib.mq_encode_nomic_bert(C.byref(cfg), C.byref(w), fake, fake, cu, 2, fake, 1, fake, need - 1, None) == -3      # MQ_ERR_WORKSPACE
    assert b"mq_encode_nomic_bert: workspace" in lib.mq_last_error()
    long = (C.c_int32 * 2)(0, 8193)
    refused(lib.mq_encode_nomic_bert(C.byref(mk(max_pos=8192)), C.byref(w), fake, fake, long, 1, fake, 1, fake, 1 << 40, None),
            b"sequence lengths must be in [1, max_pos=8192]")
    # the plan: x fp32 + h bf16 + a bf16 + max(3 W, 2 F) bf16, each slice 256-byte aligned
    assert lib.mq_nomic_bert_workspace_bytes(C.byref(mk(mlp_dim=320)), 12, 2) == need + 12 * (640 - 512) * 2
    assert lib.mq_abi_version() == L.ABI_VERSION == 15


def test_header_names_the_entry_points():
    text = L.HEADER_PATH.read_text()
    for name in ("mq_attention_full", "mq_encode_nomic_bert", "mq_nomic_bert_workspace_bytes"):
        assert name in text and name in L.EXPORTED_SYMBOLS
    for name in ("mq_nomic_bert_cfg", "mq_nomic_bert_layer", "mq_nomic_bert_weights"):
        assert f"}} {name};" in text
    assert "#define MQ_ABI_VERSION 15" in text
    assert "attention_full" in L.NO_SCRATCH_UNITS
    head = (L.CSRC_DIR / "attention_full.hip").read_text().split("#include")[0]
    assert "no VGPR / SGPR spill, no scratch" in head and "VGPRs" in head and "AGPRs" in head and "SGPRs" in head


# ---- the loader ---------------------------------------------------------------------------------------------------------------------------------------
class _Captured(Exception):
    pass


def _capture(monkeypatch):
    from marqo_amd.engine import nomic_bert as EN
    seen = {}

    def init(self, arch, sd, device, pooling="mean", precision="bf16"):
        seen.update(arch=arch, sd=sd, pooling=pooling, precision=precision)
        raise _Captured()
    monkeypatch.setattr(EN.NomicBertTower, "__init__", init)
    return seen


def _model(props):
    from marqo_amd.s2_inference.hugging_face_model import HuggingFaceModel
    return HuggingFaceModel(model_properties=props, device="cuda:0")


@pytest.fixture(scope="module")
def ckpts(tmp_path_factory):
    b, tk = N.build(), N.train_tokenizer()
    root = tmp_path_factory.mktemp("nomic")
    W = N.write_checkpoint_dir
    return dict(plain=N.save_pretrained_dir(str(root / "plain"), b["model"], tk),
                native=W(str(root / "native"), N.native_config(), b["sd"], tk),
                hub=W(str(root / "hub"), N.hub_config(), b["hub_sd"], tk, pooling="cls"),
                short=W(str(root / "short"), N.native_config(max_position_embeddings=48), b["sd"], tk),
                long=W(str(root / "long"), N.hub_config(n_positions=32768), b["hub_sd"], tk),
                scaled=W(str(root / "scaled"), N.hub_config(rotary_scaling_factor=2), b["hub_sd"], tk),
                biased=W(str(root / "biased"), N.native_config(), dict(b["sd"], **{"layers.0.mlp.up_proj.bias": torch.zeros(192)}), tk))


def test_hf_loader_takes_a_nomic_bert_directory(ckpts, monkeypatch):
    from marqo_amd.engine.tokenizers import HfJsonTokenizer
    from marqo_amd.s2_inference.errors import InvalidModelPropertiesError
    seen = _capture(monkeypatch)
    b = N.build()
    for d, prop, want, tokens, cap, trust in ((ckpts["plain"], None, "mean", 128, 128, False), (ckpts["native"], None, "mean", 128, 128, True),
                                              (ckpts["hub"], None, "cls", 128, 128, False), (ckpts["hub"], "mean", "mean", 9000, 2048, False),
                                              (ckpts["long"], None, "mean", 9000, 8192, False), (ckpts["plain"], "cls", "cls", 16, 16, False),
                                              (ckpts["short"], None, "mean", 128, 48, False)):
        props = {"type": "hf", "name": d, "dimensions": 128, "tokens": tokens}
        if trust:
            props["trustRemoteCode"] = True          # accepted and ignored: the family is native in transformers
        if prop:
            props["poolingMethod"] = prop
        m = _model(props)
        with pytest.raises(_Captured):
            m._load_necessary_components()
        assert isinstance(seen["arch"], archs.NomicBertArch) and seen["arch"].heads == 2 and seen["arch"].rope_theta == 1000.0
        assert isinstance(m._tokenizer, HfJsonTokenizer) and m._tokenizer.pad_id == 0
        assert seen["pooling"] == want and seen["precision"] == "bf16"
        assert m.model_properties.tokens == cap       # min(tokens, max_position_embeddings, 8192)
        t = TW.nomic_bert_state_dict(seen["arch"], seen["sd"])
        assert all(torch.equal(t[k], b["tensors"][k]) for k in b["tensors"])
    ok = {"type": "hf", "name": ckpts["plain"], "dimensions": 128}
    with pytest.raises(InvalidModelPropertiesError, match="'enginePrecision': 'fp8' is not available for NomicBERT encoders"):
        _model(dict(ok, enginePrecision="fp8"))._load_necessary_components()
    with pytest.raises(InvalidModelPropertiesError, match="Original error pooling_method must be 'mean' or 'cls'"):
        _model(dict(ok, poolingMethod="last"))._load_necessary_components()
    with pytest.raises(InvalidModelPropertiesError, match="'dimensions'=64 but the encoder width is 128"):
        _model(dict(ok, dimensions=64))._load_necessary_components()
    with pytest.raises(InvalidModelPropertiesError, match="rotary_scaling_factor=2 unsupported"):
        _model(dict(ok, name=ckpts["scaled"]))._load_necessary_components()


def test_a_bias_tensor_in_the_directory_is_refused_by_name(ckpts):
    from marqo_amd.s2_inference.errors import InvalidModelPropertiesError
    from marqo_amd.engine.nomic_bert import NomicBertTower
    seen = []
    orig = NomicBertTower.__init__
    try:
        def init(self, arch, sd, device, pooling="mean", precision="bf16"):
            seen.append(1)
            TW.nomic_bert_state_dict(arch, sd)       # (what the constructor runs first on the device; the refusal needs no GPU)
        NomicBertTower.__init__ = init
        with pytest.raises(InvalidModelPropertiesError, match="'layers.0.mlp.up_proj.bias' is unexpected"):
            _model({"type": "hf", "name": ckpts["biased"], "dimensions": 128})._load_necessary_components()
    finally:
        NomicBertTower.__init__ = orig
    assert seen


def test_the_tower_refuses_fp8_and_last_pooling_before_any_device_work():
    from marqo_amd.engine.nomic_bert import NomicBertTower
    src = (L.CSRC_DIR.parent / "engine" / "nomic_bert.py").read_text()
    assert "bf16 operands only" in src and "pooling must be 'mean' or 'cls'" in src
    assert NomicBertTower.family == "nomic_bert"
    assert all(f"mq_{n}" in L.EXPORTED_SYMBOLS for n in ("encode_nomic_bert", "nomic_bert_workspace_bytes"))


def test_cross_encoders_on_this_tower_are_refused(tmp_path):
    from marqo_amd.engine.rerank import CrossEncoderTower
    b = N.build()
    d = N.write_checkpoint_dir(str(tmp_path / "ce"), N.native_config(num_labels=1), b["sd"])
    with pytest.raises(ValueError, match="model_type='nomic_bert' \\(NomicBERT\\) is not served as a cross-encoder"):
        CrossEncoderTower.from_dir(d, "cuda:0")


def test_registry_is_unchanged():
    from marqo_amd.s2_inference import s2_inference as S
    mp = S.load_model_properties()
    assert len(mp["models"]) == 204 and len(mp["loaders"]) == 12 and not any("nomic" in n.lower() for n in mp["models"])

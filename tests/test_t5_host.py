"""T5 encoders on the host (no GPU): the config parser and its refusals, the tensor mapping with the fused QKV / (up | gate) row order, the clamped bias
table against transformers' own compute_bias, the float64 pass of tests/t5_ref.py against transformers' T5EncoderModel, the orchestration mutants that
pass must see, the loader wiring through `hf` and `sbert`, the token rows, the C ABI's struct sizes and argument checks, and the three faults of the bias
lookup the GPU test's bias-only inputs must see.

The clamp argument.  T5's bucket function is constant for |key - query| >= relative_attention_max_distance, so a table of 2 D + 1 columns read at
clamp(key - query, -D, D) + D is the bias at ANY length: test_bias_table_equals_compute_bias holds that exactly (torch.equal) against the library's
compute_bias(T, T) at T = 1, 9, 128, 129 and 600 — below, at and past D = 128.

Tolerance of the oracle comparison (ORACLE_ATOL, tests/test_qwen_host.py's): float64 `exact` against fp32 transformers on the same operands; measured
1.4e-6 .. 6.8e-6 on the three tinies at lengths 1, 2, 64, 65, 200.

Mutants (T5_MUTANT lines; bar = the GPU test's MARGIN 4.0): measured worst-view ratios over the three tinies — bias_per_layer 33 .. 144, scaled 139 .. 359,
wi_swapped 117 .. 246, eps_x10 16 .. 43, bias_sign 141 .. 409; the second rounding history (hist = 1) stays at 1.00 .. 1.33."""
import ctypes as C
import json
import os

import pytest
import torch

from marqo_amd import _lib as L
from marqo_amd.engine import archs
from tests import attention_ref as AR
from tests import t5_ref as T
from tests.test_patch_attn_gpu import MARGIN

ORACLE_ATOL = 3e-5


# ---- the config parser -------------------------------------------------------------------------------------------------------------------------------
def test_arch_from_config():
    a = archs.bert_arch_from_hf_config(T.TINY_RELU)
    assert isinstance(a, archs.T5Arch) and (a.width, a.heads, a.head_dim, a.inner, a.mlp_dim, a.layers, a.gated) == (128, 2, 64, 128, 256, 2, False)
    assert (a.rel_buckets, a.max_distance, a.rms_eps, a.max_pos, a.vocab) == (32, 128, 1e-6, 8192, 384)
    g = archs.bert_arch_from_hf_config(T.config_dict(T.TINY_GATED, is_gated_act=True, dense_act_fn="gelu_new"))
    assert g.gated
    w = archs.t5_arch_from_hf_config(T.TINY_WIDE)
    assert w.inner == 384 and w.width == 128 and w.head_dim == 128                   # inner != d_model
    small = archs.t5_arch_from_hf_config(T.config_dict(T.TINY_GATED, d_model=512, num_heads=6, d_kv=64, d_ff=1024))     # flan-t5-small
    assert small.inner == 384 and small.width == 512
    big = archs.t5_arch_from_hf_config(T.config_dict(T.TINY_RELU, d_model=1024, num_heads=32, d_kv=128, d_ff=16384))     # t5-3b
    assert big.inner == 4096
    with pytest.raises(KeyError, match="is not a BERT-family encoder"):      # the other families keep their refusal
        archs.bert_arch_from_hf_config({"model_type": "mt5"})


@pytest.mark.parametrize("over, what", [
    (dict(feed_forward_proj="gated-silu"), "feed_forward_proj=gated-silu"), (dict(feed_forward_proj="gelu"), "feed_forward_proj=gelu"),
    (dict(is_gated_act=True), "is_gated_act=True"), (dict(dense_act_fn="gelu"), "dense_act_fn=gelu"), (dict(d_kv=96), "d_kv=96"), (dict(d_kv=256), "d_kv=256"),
    (dict(d_model=4096), "d_model=4096"), (dict(d_model=2112), "d_model=2112"), (dict(d_model=200), "d_model=200"),
    (dict(num_heads=33, d_kv=128), "num_heads=33"), (dict(d_ff=100), "d_ff=100"), (dict(relative_attention_num_buckets=31), "relative_attention_num_buckets=31"),
    (dict(relative_attention_max_distance=2048), "relative_attention_max_distance=2048")])
def test_arch_parser_refuses_by_key(over, what):
    with pytest.raises(KeyError, match=what):
        archs.bert_arch_from_hf_config(T.config_dict(T.TINY_RELU, **over))


# ---- the tensor mapping ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tuple(T.TINIES))
def test_state_dict_mapping(name):
    from marqo_amd.engine.tower_weights import t5_state_dict
    b = T.build(name)
    arch, sd = b["arch"], b["sd"]
    t = b["tensors"]
    A, F = arch.inner, arch.mlp_dim
    a = "encoder.block.1.layer.0.SelfAttention."
    assert t["block.1.attn.qkv.weight"].shape == (3 * A, 128)
    assert torch.equal(t["block.1.attn.qkv.weight"], torch.cat([sd[a + "q.weight"], sd[a + "k.weight"], sd[a + "v.weight"]]))
    assert torch.equal(t["block.1.attn.o.weight"], sd[a + "o.weight"]) and t["block.1.attn.o.weight"].shape == (128, A)
    m = "encoder.block.0.layer.1.DenseReluDense."
    if arch.gated:      # (up | gate) = (wi_1 | wi_0): the module computes wo(gelu_new(wi_0 x) * wi_1 x)
        assert torch.equal(t["block.0.ff.wi.weight"], torch.cat([sd[m + "wi_1.weight"], sd[m + "wi_0.weight"]])) and t["block.0.ff.wi.weight"].shape == (2 * F, 128)
    else:
        assert torch.equal(t["block.0.ff.wi.weight"], sd[m + "wi.weight"])
    assert torch.equal(t["embed_tokens.weight"], sd["shared.weight"]) and torch.equal(t["final_layer_norm.weight"], sd["encoder.final_layer_norm.weight"])
    assert t["rel_bias"].shape == (arch.heads, 257) and t["rel_bias"].dtype == torch.float32
    # the bare spelling, the encoder's own token table, decoder tensors ignored
    bare = {k[len("encoder."):]: v for k, v in sd.items() if k.startswith("encoder.")}
    bare["decoder.block.0.layer.0.SelfAttention.q.weight"] = torch.zeros(1)
    bare["lm_head.weight"] = torch.zeros(1)
    t2 = t5_state_dict(arch, bare)
    assert set(t2) == set(t) and all(torch.equal(t2[k], t[k]) for k in t)
    full = dict(sd, **{"decoder.block.0.layer.0.SelfAttention.q.weight": torch.zeros(1), "lm_head.weight": torch.zeros(1)})
    full.pop("encoder.embed_tokens.weight")
    assert all(torch.equal(v, t[k]) for k, v in t5_state_dict(arch, full).items())
    with pytest.raises(KeyError, match="missing tensor 'block.1.layer.0.SelfAttention.k.weight'"):
        t5_state_dict(arch, {k: v for k, v in sd.items() if k != a + "k.weight"})
    with pytest.raises(ValueError, match="a bias table per block"):
        t5_state_dict(arch, dict(sd, **{a + "relative_attention_bias.weight": torch.zeros(32, arch.heads)}))


@pytest.mark.parametrize("name", ("TINY_RELU", "TINY_WIDE"))
def test_bias_table_equals_compute_bias(name):
    """the 2 D + 1 columns gathered at clamp(k - q, -D, D) ARE the library's bias, exactly, below, at and past D"""
    b = T.build(name)
    arch = b["arch"]
    attn = b["model"].encoder.block[0].layer[0].SelfAttention
    table = arch.rel_bias_table(attn.relative_attention_bias.weight)
    assert table.shape == (arch.heads, 2 * arch.max_distance + 1)
    for Tn in (1, 9, 128, 129, 600):
        with torch.no_grad():
            ref = attn.compute_bias(Tn, Tn)[0]                    # [heads, query, key]
        got = table[:, T.bias_index(Tn, arch.max_distance)]
        assert torch.equal(got, ref), Tn
    # a shifted or mirrored lookup is not the library's bias (a clamp at D - 1 is: T5's last bucket begins below D — that fault is the kernel test's, on a
    # table with a value of its own in every column)
    with torch.no_grad():
        ref = attn.compute_bias(300, 300)[0]
    for fault in ("index_plus1", "sign"):
        assert not torch.equal(table[:, T.bias_index(300, arch.max_distance, fault=fault)], ref), fault
    with pytest.raises(ValueError, match="is not \\[relative_attention_num_buckets=32"):
        arch.rel_bias_table(torch.zeros(16, arch.heads))


# ---- the float64 pass against transformers, and the mutants it must see -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def passes():
    out = {}
    for name in T.TINIES:
        b = T.build(name)
        lens = [len(s) for s in b["seqs"]]
        ids = torch.cat(b["seqs"])
        out[name] = dict(b, lens=lens, ids=ids, ex=T.exact(b["arch"], b["tensors"], ids, lens), mo=T.model(b["arch"], b["tensors"], ids, lens))
    return out


@pytest.mark.parametrize("name", tuple(T.TINIES))
def test_exact_pass_equals_transformers(passes, name):
    p = passes[name]
    ref = torch.cat(T.oracle_hidden_packed(p["model"], p["seqs"])).double()
    d = float((p["ex"].final - ref).abs().max())
    print(f"T5_ORACLE {name}: max |exact - transformers| = {d:.3e} (bar {ORACLE_ATOL:.0e})")
    assert d < ORACLE_ATOL
    # the padded batch gives the packed rows: padded keys are masked by the library
    ids, mask = T.pad_batch(p["seqs"])
    with torch.no_grad():
        hid = p["model"](input_ids=ids, attention_mask=mask).last_hidden_state
    r0 = 0
    for i, ln in enumerate(p["lens"]):
        assert float((hid[i, :ln].double() - ref[r0:r0 + ln]).abs().max()) < ORACLE_ATOL
        r0 += ln


def _views(ps):
    return [("block%d" % i, b) for i, b in enumerate(ps.blocks)] + [("final", ps.final)] + [("pooled/%s/l2=%d" % k, v) for k, v in ps.pooled.items()]


@pytest.mark.parametrize("name", tuple(T.TINIES))
def test_second_rounding_history_is_inside_the_bar(passes, name):
    p = passes[name]
    h1 = T.model(p["arch"], p["tensors"], p["ids"], p["lens"], hist=1)
    worst = 0.0
    for (view, got), (_, ex), (_, mo) in zip(_views(h1), _views(p["ex"]), _views(p["mo"])):
        r = T.row_ratio(got, ex, mo)["ratio"]
        print(f"T5_HIST1 {name} {view} ratio={r:.3f}")
        worst = max(worst, r)
    assert worst <= MARGIN


@pytest.mark.parametrize("name, mut", [(n, m) for n in T.TINIES for m in T.MUTANTS if m != "wi_swapped" or T.TINIES[n]["feed_forward_proj"] == "gated-gelu"])
def test_every_orchestration_mutant_leaves_the_bar(passes, name, mut):
    """what the GPU test's ratio check would measure for ONE defect of csrc/t5.hip's orchestration: every view it checks (the stream after every block,
    the final norm, the pooled rows) taken together must leave the bar"""
    p = passes[name]
    assert T.applies(mut, p["arch"])
    mm = T.model(p["arch"], p["tensors"], p["ids"], p["lens"], mut=mut)
    rs = {view: T.row_ratio(got, ex, mo)["ratio"] for (view, got), (_, ex), (_, mo) in zip(_views(mm), _views(p["ex"]), _views(p["mo"]))}
    print(f"T5_MUTANT {name} {mut}: " + " ".join(f"{k}={v:.1f}" for k, v in rs.items()))
    assert rs["final"] > 2 * MARGIN and min(v for k, v in rs.items() if k.startswith("pooled")) > 2 * MARGIN


# ---- the bias-only inputs of the GPU test see the faults of the lookup -----------------------------------------------------------------------------------
@pytest.mark.parametrize("hd, D, lens", [(64, 128, [300, 17]), (128, 4, [65, 9])])
def test_bias_only_inputs_see_every_fault_of_the_lookup(hd, D, lens):
    heads = 2
    qkv = T.bias_only_qkv(lens, heads, hd)
    table = T.make_table(heads, D, seed=1, kind="distinct")
    out, absout = T.relbias_reference(qkv, lens, heads, hd, table, D, 1.0)
    # the output is softmax(bias row) applied to V
    r0 = 0
    for ln in lens:
        p = torch.softmax(table.double()[:, T.bias_index(ln, D)], -1)
        v = qkv[r0:r0 + ln, 2 * heads * hd:].double().reshape(ln, heads, hd).transpose(0, 1)
        assert float(((p @ v).transpose(0, 1).reshape(ln, heads * hd) - out[r0:r0 + ln]).abs().max()) < 1e-12
        r0 += ln
    for fault in T.BIAS_FAULTS:
        wrong, _ = T.relbias_reference(qkv, lens, heads, hd, table, D, 1.0, fault=fault)
        r = AR.worst_ratio(wrong, out, absout)
        print(f"RELBIAS_FAULT hd={hd} D={D} lens={lens} {fault} ratio={r:.1f}")
        assert r > 50.0, fault


def test_reference_equals_attention_ref_with_an_unclamped_table():
    """with D >= the longest sequence nothing is clamped: attention_ref.reference with its own bias argument and scale 1 / sqrt(hs)"""
    lens, heads, hd, D = [70, 9], 2, 64, 80
    qkv = AR.make_qkv("randn", lens, heads, hd, seed=4)
    table = T.make_table(heads, D, seed=2)
    out, absout = T.relbias_reference(qkv, lens, heads, hd, table, D, hd ** -0.5)
    o2, a2, _ = AR.reference(qkv, lens, heads, hd, AR.MASK_NONE, bias=table)
    assert float((out - o2).abs().max()) < 1e-12 and float((absout - a2).abs().max()) < 1e-12


# ---- the C ABI without a GPU -----------------------------------------------------------------------------------------------------------------------------
def test_entry_points_judge_their_arguments_before_any_launch():
    lib = L.load()
    fake = C.c_void_p(4096)

    def refused(rc, what):
        assert rc == -1 and what in lib.mq_last_error(), lib.mq_last_error()
    rb = lib.mq_attention_relbias
    refused(rb(None, fake, fake, 1, 0, 10, 2, 64, fake, 128, 1.0, None), b"mq_attention_relbias: null pointer")
    refused(rb(fake, fake, fake, 1, 0, 10, 2, 64, None, 128, 1.0, None), b"mq_attention_relbias: null bias table")
    refused(rb(fake, fake, fake, 1, 0, 10, 2, 96, fake, 128, 1.0, None), b"mq_attention_relbias: head_dim 96 unsupported")
    refused(rb(fake, fake, fake, 1, 0, 10, 2, 64, fake, 0, 1.0, None), b"mq_attention_relbias: max_distance 0 outside [1, 1024]")
    refused(rb(fake, fake, fake, 1, 0, 10, 2, 64, fake, 1025, 1.0, None), b"max_distance 1025")
    refused(rb(fake, fake, fake, 1, 0, 10, 2, 64, fake, 128, 0.0, None), b"scale 0 must be positive")
    refused(rb(fake, fake, None, 1, 0, 10, 2, 64, fake, 128, 1.0, None), b"need fixed_len or cu_seqlens")
    refused(rb(fake, fake, fake, 1, 0, 8193, 2, 64, fake, 128, 1.0, None), b"max sequence length 8193 unsupported")
    refused(rb(fake, fake, None, 1, 8193, 0, 2, 64, fake, 128, 1.0, None), b"max sequence length 8193 unsupported")
    assert rb(fake, fake, fake, 0, 0, 10, 2, 64, fake, 128, 1.0, None) == 0          # nseq 0: nothing to do
    assert C.sizeof(L.T5Layer) == 48 and C.sizeof(L.T5Weights) == 40 and C.sizeof(L.T5Cfg) == 48
    w = L.T5Weights()
    mk = lambda **kw: L.T5Cfg(**dict(dict(width=128, layers=1, heads=2, head_dim=64, mlp_dim=256, vocab=10, max_pos=64, pool=L.MQ_POOL_MEAN, max_distance=128,
                                          gated=0, rms_eps=1e-6), **kw))
    for kw, what in ((dict(head_dim=96), b"head_dim (d_kv) 96 unsupported"), (dict(width=2112), b"width (d_model) 2112"), (dict(width=4096), b"width (d_model) 4096"),
                     (dict(heads=33, head_dim=128), b"inner width heads 33 x head_dim 128"), (dict(mlp_dim=100), b"mlp_dim 100"), (dict(max_pos=9000), b"max_pos 9000"),
                     (dict(pool=L.MQ_POOL_LAST), b"bad pooling 2"), (dict(max_distance=0), b"max_distance 0 outside [1, 1024]"), (dict(gated=2), b"gated 2")):
        cfg = mk(**kw)
        refused(lib.mq_encode_t5(C.byref(cfg), C.byref(w), None, None, None, 0, fake, 1, None, 0, None), b"mq_encode_t5: " + what)
    cfg = mk()
    refused(lib.mq_encode_t5(C.byref(cfg), None, fake, fake, fake, 1, fake, 1, fake, 0, None), b"mq_encode_t5: null pointer")
    refused(lib.mq_encode_t5(C.byref(cfg), C.byref(w), fake, fake, fake, 1, fake, 1, fake, 0, None), b"mq_encode_t5: null weight pointer")
    layers = (L.T5Layer * 1)(L.T5Layer(*([4096] * 6)))
    w = L.T5Weights(tok_emb=4096, final_norm_g=4096, zeros=4096, d_rel_bias=4096, layers=layers)
    assert lib.mq_encode_t5(C.byref(cfg), C.byref(w), None, None, None, 0, fake, 1, None, 0, None) == 0      # nseq 0: nothing to do
    cu = (C.c_int32 * 3)(0, 5, 12)
    refused(lib.mq_encode_t5(C.byref(cfg), C.byref(w), None, fake, cu, 2, fake, 1, fake, 1 << 20, None), b"mq_encode_t5: null input / workspace")
    need = lib.mq_t5_workspace_bytes(C.byref(cfg), 12, 2)
    assert need >= 12 * 128 * 4 and lib.mq_t5_workspace_bytes(None, 12, 2) == 0 and lib.mq_t5_workspace_bytes(C.byref(cfg), 0, 2) == 0
    assert lib.mq_encode_t5(C.byref(cfg), C.byref(w), fake, fake, cu, 2, fake, 1, fake, need - 1, None) == -3      # MQ_ERR_WORKSPACE
    assert b"mq_encode_t5: workspace" in lib.mq_last_error()
    long = (C.c_int32 * 2)(0, 8193)
    big = mk(max_pos=8192)
    refused(lib.mq_encode_t5(C.byref(big), C.byref(w), fake, fake, long, 1, fake, 1, fake, 1 << 40, None), b"sequence lengths must be in [1, max_pos=8192]")
    # the plan: x fp32 + h bf16 + a bf16 + max(3 A, F or 2 F) bf16, each slice 256-byte aligned; inner != d_model and the gated MLP move it
    assert lib.mq_t5_workspace_bytes(C.byref(mk(heads=3, head_dim=128)), 12, 2) > need
    assert lib.mq_t5_workspace_bytes(C.byref(mk(gated=1, mlp_dim=512)), 12, 2) > lib.mq_t5_workspace_bytes(C.byref(mk(mlp_dim=512)), 12, 2) == need + 12 * (512 - 384) * 2
    assert lib.mq_abi_version() == 15


def test_header_names_the_entry_points():
    text = L.HEADER_PATH.read_text()
    for name in ("mq_attention_relbias", "mq_encode_t5", "mq_t5_workspace_bytes", "mq_t5_cfg", "mq_t5_layer", "mq_t5_weights"):
        assert name in text and (not name.startswith("mq_t5_") or name.endswith("bytes") or f"}} {name};" in text), name
    assert "#define MQ_ABI_VERSION 15" in text
    for name in ("mq_attention_relbias", "mq_encode_t5", "mq_t5_workspace_bytes"):
        assert name in L.EXPORTED_SYMBOLS


# ---- the loaders -----------------------------------------------------------------------------------------------------------------------------------------
class _Captured(Exception):
    pass


def _capture(monkeypatch):
    from marqo_amd.engine import t5 as ET
    seen = {}

    def init(self, arch, sd, device, pooling="mean", precision="bf16", dense=()):
        seen.update(arch=arch, sd=sd, pooling=pooling, precision=precision, dense=list(dense))
        raise _Captured()
    monkeypatch.setattr(ET.T5Tower, "__init__", init)
    return seen


def _model(props):
    from marqo_amd.s2_inference.hugging_face_model import HuggingFaceModel
    return HuggingFaceModel(model_properties=props, device="cuda:0")


@pytest.fixture(scope="module")
def dense_w():
    return torch.randn(128, 128, generator=torch.Generator().manual_seed(21)) / 128 ** 0.5


@pytest.fixture(scope="module")
def ckpts(tmp_path_factory, dense_w):
    m, tk = T.build("TINY_RELU")["model"], T.train_tokenizer()
    root = tmp_path_factory.mktemp("t5")
    return dict(plain=T.write_checkpoint_dir(str(root / "plain"), m, tk),
                cls=T.write_checkpoint_dir(str(root / "cls"), m, tk, pooling="cls"),
                st=T.write_checkpoint_dir(str(root / "st"), m, tk, pooling="mean", dense=[dense_w], max_seq_length=40))


def test_hf_loader_takes_a_t5_directory(ckpts, monkeypatch):
    from marqo_amd.engine.tokenizers import HfJsonTokenizer
    from marqo_amd.s2_inference.errors import InvalidModelPropertiesError
    seen = _capture(monkeypatch)
    for d, prop, want, tokens, cap in ((ckpts["plain"], None, "mean", 128, 128), (ckpts["cls"], None, "cls", 128, 128), (ckpts["cls"], "mean", "mean", 9000, 8192),
                                       (ckpts["plain"], "cls", "cls", 16, 16), (ckpts["st"], None, "mean", 128, 40), (ckpts["st"], None, "mean", 24, 24)):
        props = {"type": "hf", "name": d, "dimensions": 128, "tokens": tokens}
        if prop:
            props["poolingMethod"] = prop
        m = _model(props)
        with pytest.raises(_Captured):
            m._load_necessary_components()
        assert isinstance(seen["arch"], archs.T5Arch) and seen["arch"] == archs.bert_arch_from_hf_config(T.TINY_RELU)
        assert isinstance(m._tokenizer, HfJsonTokenizer) and m._tokenizer.pad_id == 0 and m._tokenizer.cls_id is None
        assert seen["pooling"] == want and seen["precision"] == "bf16" and seen["dense"] == []      # `hf` is the bare encoder: no Dense module
        assert any(k.endswith("block.0.layer.0.SelfAttention.relative_attention_bias.weight") for k in seen["sd"])
        assert m.model_properties.tokens == cap       # min(tokens, sentence_bert_config.json max_seq_length, 8192)
    with pytest.raises(InvalidModelPropertiesError, match="'enginePrecision': 'fp8' is not available for T5 encoders"):
        _model({"type": "hf", "name": ckpts["plain"], "dimensions": 128, "enginePrecision": "fp8"})._load_necessary_components()
    with pytest.raises(InvalidModelPropertiesError, match="Original error pooling_method must be 'mean' or 'cls'"):
        _model({"type": "hf", "name": ckpts["plain"], "dimensions": 128, "poolingMethod": "last"})._load_necessary_components()
    with pytest.raises(InvalidModelPropertiesError, match="'dimensions'=64 but the encoder width is 128"):
        _model({"type": "hf", "name": ckpts["plain"], "dimensions": 64})._load_necessary_components()


def test_a_refused_config_is_the_loaders_error(ckpts, tmp_path):
    import shutil
    from marqo_amd.s2_inference.errors import InvalidModelPropertiesError
    d = str(tmp_path / "odd")
    shutil.copytree(ckpts["plain"], d)
    with open(os.path.join(d, "config.json")) as f:
        cfg = json.load(f)
    cfg["d_kv"] = 96
    with open(os.path.join(d, "config.json"), "w") as f:
        json.dump(cfg, f)
    with pytest.raises(InvalidModelPropertiesError, match="d_kv=96 unsupported"):
        _model({"type": "hf", "name": d, "dimensions": 128})._load_necessary_components()


def test_sbert_loader_picks_the_dense_module_up(ckpts, monkeypatch, dense_w, tmp_path):
    from marqo_amd.s2_inference.errors import InvalidModelPropertiesError
    from marqo_amd.s2_inference.sbert_utils import SBERT
    seen = _capture(monkeypatch)
    s = SBERT(ckpts["st"], device="cuda:0", embedding_dim=128)
    with pytest.raises(_Captured):
        s.load()
    assert seen["pooling"] == "mean" and len(seen["dense"]) == 1 and torch.equal(seen["dense"][0], dense_w)
    assert s.max_seq_length == 40 and s.model.model_properties.tokens == 40 and s.always_normalized
    s = SBERT(ckpts["cls"], device="cuda:0", embedding_dim=128)
    with pytest.raises(_Captured):
        s.load()
    assert seen["pooling"] == "cls" and seen["dense"] == [] and s.model.model_properties.tokens == 128
    m, tk = T.build("TINY_RELU")["model"], T.train_tokenizer()
    biased = T.write_checkpoint_dir(str(tmp_path / "biased"), m, tk, pooling="mean", dense=[dense_w], dense_bias=True)
    with pytest.raises(InvalidModelPropertiesError, match="Dense module 2_Dense has a bias"):
        SBERT(biased, device="cuda:0", embedding_dim=128).load()
    tanh = T.write_checkpoint_dir(str(tmp_path / "tanh"), m, tk, pooling="mean", dense=[dense_w], dense_activation="torch.nn.modules.activation.Tanh")
    with pytest.raises(InvalidModelPropertiesError, match="Dense module 2_Dense has activation"):
        SBERT(tanh, device="cuda:0", embedding_dim=128).load()


def test_token_rows_are_the_librarys(ckpts):
    """HfJsonTokenizer.plain on the directory: the `tokenizers` library's own ids, </s> appended by the file's post-processor and kept under truncation,
    right-padded with <pad>"""
    from tokenizers import Tokenizer
    from marqo_amd.engine.tokenizers import HfJsonTokenizer
    tk = HfJsonTokenizer.plain(ckpts["plain"], pad_fallback="<pad>")
    raw = Tokenizer.from_file(os.path.join(ckpts["plain"], "tokenizer.json"))
    texts = ["hello world", "a search engine ranks documents for a query " * 6, "", "Paris!"]
    for cap in (None, 12):
        if cap:
            raw.enable_truncation(max_length=cap)
        want = [raw.encode(x).ids for x in texts]
        got = tk(texts, max_length=cap)
        S = max(len(w) for w in want)
        assert got["input_ids"].shape == (4, S) and (cap is None or S == cap)
        for i, w in enumerate(want):
            assert w[-1] == 1 and list(got["input_ids"][i, :len(w)]) == w and int(got["attention_mask"][i].sum()) == len(w)
            assert bool((got["input_ids"][i, len(w):] == 0).all())
    assert want[2] == [1]          # the empty text is </s> alone

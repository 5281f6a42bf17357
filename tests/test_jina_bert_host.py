"""JinaBERT encoders on the host (no GPU): the ALiBi slopes against their closed form and against transformers' Bloom build_alibi_tensor, the config parser
and its refusals, the neighbours of the new branch in bert_arch_from_hf_config, the tensor mapping with the fused QKV / (up | gate) row order, the C ABI's
struct sizes and argument checks, the precondition of the GPU kernel test's readout and bias-only inputs, the faults of the bias those inputs must see,
the orchestration mutants the float64 pass of tests/jina_bert_ref.py must see, and the loader wiring through `hf`.

The block semantics are restated from the published architecture; the original modelling code is not available to these tests and nothing here is pinned
to a run of it.  The slopes are the one formula with a library oracle.

Fault sensitivity (ALIBI_FAULT lines; bar = the GPU test's MARGIN 1.25 x budget), measured worst ratios on the bias-only inputs [300, 17] / [65, 9] /
[700]:  index_plus1 32 / 133 / 16   no_abs 2.0e4 / 1.4e15 / 1.8e3   next_head_slope 3.4e3 / 5.0e8 / 432   bias_scaled 3.1e4 / 1.9e13 / 1.5e3.  Nothing
was fixed in advance: the assertion is that each leaves the bar.

Mutants (JINA_MUTANT lines; bar = 2 x the GPU test's MARGIN 4.0), the smallest ratio among the views asserted (the stream after the last block, the four
pooled outputs), TINY_2H / TINY_3H:  gate_swapped 185 / 159   slopes_reversed 38 / 32   bias_scaled 23 / 40   no_abs 9.5 / 13   pre_ln 427 / 287; the
second rounding history (hist = 1) stays at 1.00 .. 1.64."""
import ctypes as C
import math

import pytest
import torch

from marqo_amd import _lib as L
from marqo_amd.engine import archs
from tests import attention_ref as AR
from tests import jina_bert_ref as J
from tests.test_attention_gpu import MARGIN as KERNEL_MARGIN
from tests.test_patch_attn_gpu import MARGIN


# ---- the slopes ---------------------------------------------------------------------------------------------------------------------------------------
def _slopes(n):
    return archs.JinaBertArch(heads=n, width=64 * n).slopes()


def test_slopes_known_answers():
    assert _slopes(2) == pytest.approx([2.0 ** -4, 2.0 ** -8], rel=1e-14)
    assert _slopes(8) == pytest.approx([2.0 ** -i for i in range(1, 9)], rel=1e-14)
    assert _slopes(12) == pytest.approx([2.0 ** -i for i in range(1, 9)] + [2.0 ** -0.5, 2.0 ** -1.5, 2.0 ** -2.5, 2.0 ** -3.5], rel=1e-14)
    assert _slopes(3) == pytest.approx([2.0 ** -4, 2.0 ** -8, 2.0 ** -2], rel=1e-14)
    assert _slopes(1) == pytest.approx([2.0 ** -8], rel=1e-14)


def test_slopes_equal_blooms_build_alibi_tensor():
    """Bloom's tensor is slopes[h] * position: column 1 of an all-ones mask is the slope (fp32 arithmetic in the library: one part in 1e6)"""
    bloom = pytest.importorskip("transformers.models.bloom.modeling_bloom")
    for n in range(1, 17):
        t = bloom.build_alibi_tensor(torch.ones(1, 3, dtype=torch.long), n, torch.float32)      # [n, 1, 3]: slope * (0, 1, 2)
        assert t.shape == (n, 1, 3)
        assert t[:, 0, 1].double().tolist() == pytest.approx(_slopes(n), rel=2e-6), n
        assert t[:, 0, 2].double().tolist() == pytest.approx([2 * s for s in _slopes(n)], rel=2e-6), n


# ---- the config parser ------------------------------------------------------------------------------------------------------------------------------
def test_arch_from_config():
    a = archs.bert_arch_from_hf_config(J.TINY_2H)
    assert isinstance(a, archs.JinaBertArch)
    assert (a.width, a.heads, a.head_dim, a.mlp_dim, a.layers, a.vocab, a.max_pos, a.ln_eps, a.type_vocab) == (128, 2, 64, 256, 2, 384, 8192, 1e-12, 2)
    b = archs.jina_bert_arch_from_hf_config(J.TINY_3H)
    assert (b.width, b.heads, b.mlp_dim) == (192, 3, 320)
    assert archs.bert_arch_from_hf_config(J.config_dict(J.TINY_2H, max_position_embeddings=512)).max_pos == 512
    assert archs.bert_arch_from_hf_config(J.config_dict(J.TINY_2H, max_position_embeddings=16384)).max_pos == 8192
    base = archs.bert_arch_from_hf_config(J.config_dict(J.TINY_2H, hidden_size=768, num_attention_heads=12, intermediate_size=3072, num_hidden_layers=12,
                                                        vocab_size=30528))       # jina-embeddings-v2-base-en
    assert (base.width, base.heads, base.mlp_dim, base.layers) == (768, 12, 3072, 12) and len(base.slopes()) == 12
    cfg = {k: v for k, v in J.TINY_2H.items() if k != "model_type"}      # model_type defaults to bert
    assert isinstance(archs.bert_arch_from_hf_config(cfg), archs.JinaBertArch)


@pytest.mark.parametrize("over, what", [
    (dict(feed_forward_type="original"), "feed_forward_type=original"), (dict(feed_forward_type="reglu"), "feed_forward_type=reglu"),
    (dict(hidden_act="relu"), "hidden_act=relu"), (dict(num_attention_heads=4), "hidden_size=128 / num_attention_heads=4"),
    (dict(hidden_size=2112, num_attention_heads=33), "hidden_size=2112"), (dict(intermediate_size=100), "intermediate_size=100")])
def test_arch_parser_refuses_by_key(over, what):
    with pytest.raises(KeyError, match=what):
        archs.bert_arch_from_hf_config(J.config_dict(J.TINY_2H, **over))


def test_a_config_without_feed_forward_type_is_refused_by_that_key():
    with pytest.raises(KeyError, match="feed_forward_type="):
        archs.bert_arch_from_hf_config({k: v for k, v in J.TINY_2H.items() if k != "feed_forward_type"})


def test_neighbours_of_the_new_branch_keep_their_paths():
    plain = dict(model_type="bert", vocab_size=100, max_position_embeddings=512, hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256)
    a = archs.bert_arch_from_hf_config(plain)
    assert isinstance(a, archs.BertArch) and a == archs.bert_arch_from_hf_config(dict(plain, position_embedding_type="absolute"))
    for pet in ("relative_key", "relative_key_query"):
        with pytest.raises(KeyError, match="only absolute position embeddings are supported"):
            archs.bert_arch_from_hf_config(dict(plain, position_embedding_type=pet))
    for mtype in ("xlm-roberta", "roberta"):      # alibi is JinaBERT's under model_type bert only
        with pytest.raises(KeyError, match="only absolute position embeddings are supported"):
            archs.bert_arch_from_hf_config(dict(plain, model_type=mtype, position_embedding_type="alibi"))
    with pytest.raises(KeyError, match="is not a JinaBERT model"):
        archs.jina_bert_arch_from_hf_config(plain)


# ---- the tensor mapping -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tuple(J.TINIES))
def test_state_dict_mapping(name):
    from marqo_amd.engine.tower_weights import jina_bert_state_dict
    b = J.build(name)
    arch, sd, t = b["arch"], b["sd"], b["tensors"]
    W, F = arch.width, arch.mlp_dim
    a = "encoder.layer.1.attention.self."
    assert t["layer.1.attn.qkv.weight"].shape == (3 * W, W) and t["layer.1.attn.qkv.bias"].shape == (3 * W,)
    assert torch.equal(t["layer.1.attn.qkv.weight"], torch.cat([sd[a + "query.weight"], sd[a + "key.weight"], sd[a + "value.weight"]]))
    assert torch.equal(t["layer.1.attn.qkv.bias"], torch.cat([sd[a + "query.bias"], sd[a + "key.bias"], sd[a + "value.bias"]]))
    g = sd["encoder.layer.0.mlp.gated_layers.weight"]
    assert t["layer.0.mlp.up_gate.weight"].shape == (2 * F, W)
    assert torch.equal(t["layer.0.mlp.up_gate.weight"][:F], g[F:]) and torch.equal(t["layer.0.mlp.up_gate.weight"][F:], g[:F])      # (up | gate) = (W[F:] | W[:F])
    assert torch.equal(t["layer.0.attn.o.weight"], sd["encoder.layer.0.attention.output.dense.weight"])
    assert torch.equal(t["layer.1.mlp_ln.bias"], sd["encoder.layer.1.mlp.layernorm.bias"])
    assert torch.equal(t["type0"], sd["embeddings.token_type_embeddings.weight"][0]) and t["type0"].shape == (W,)
    assert torch.equal(t["word_embeddings.weight"], sd["embeddings.word_embeddings.weight"])
    assert not any("pooler" in k or "position" in k for k in t)
    # the `bert.` prefix of the task-head classes
    t2 = jina_bert_state_dict(arch, {"bert." + k: v for k, v in sd.items()})
    assert set(t2) == set(t) and all(torch.equal(t2[k], t[k]) for k in t)
    with pytest.raises(KeyError, match="missing tensor 'encoder.layer.1.attention.self.key.weight'"):
        jina_bert_state_dict(arch, {k: v for k, v in sd.items() if k != a + "key.weight"})
    with pytest.raises(ValueError, match="mlp.gated_layers.weight' has shape"):
        jina_bert_state_dict(arch, dict(sd, **{"encoder.layer.0.mlp.gated_layers.weight": g[:F]}))
    for n in ("layer_norm_q", "layer_norm_k"):
        with pytest.raises(ValueError, match="qk-post-norm JinaBERT variants .*-de / -es / -zh / -code"):
            jina_bert_state_dict(arch, dict(sd, **{a + n + ".weight": torch.ones(W)}))


# ---- the C ABI without a GPU --------------------------------------------------------------------------------------------------------------------------
def test_struct_sizes_and_argument_checks():
    assert C.sizeof(L.JinaBertLayer) == 88 and C.sizeof(L.JinaBertWeights) == 48 and C.sizeof(L.JinaBertCfg) == 40      # the static_assert of csrc/jina_bert.hip
    lib = L.load()
    fake = C.c_void_p(4096)

    def refused(rc, what):
        assert rc == -1 and what in lib.mq_last_error(), lib.mq_last_error()
    al = lib.mq_attention_alibi
    refused(al(None, fake, fake, 1, 0, 10, 2, 64, fake, 1.0, None), b"mq_attention_alibi: null pointer")
    refused(al(fake, fake, fake, 1, 0, 10, 2, 64, None, 1.0, None), b"mq_attention_alibi: null slopes")
    refused(al(fake, fake, fake, 1, 0, 10, 2, 128, fake, 1.0, None), b"mq_attention_alibi: head_dim 128 unsupported")
    refused(al(fake, fake, fake, 1, 0, 10, 2, 96, fake, 1.0, None), b"mq_attention_alibi: head_dim 96 unsupported")
    refused(al(fake, fake, fake, 1, 0, 10, 0, 64, fake, 1.0, None), b"heads 0 outside [1, 1024]")
    refused(al(fake, fake, fake, 1, 0, 10, 2, 64, fake, 0.0, None), b"scale 0 must be positive")
    refused(al(fake, fake, None, 1, 0, 10, 2, 64, fake, 1.0, None), b"need fixed_len or cu_seqlens")
    refused(al(fake, fake, fake, 1, 0, 8193, 2, 64, fake, 1.0, None), b"max sequence length 8193 unsupported")
    refused(al(fake, fake, None, 1, 8193, 0, 2, 64, fake, 1.0, None), b"max sequence length 8193 unsupported")
    assert al(fake, fake, fake, 0, 0, 10, 2, 64, fake, 1.0, None) == 0          # nseq 0: nothing to do
    w = L.JinaBertWeights()
    mk = lambda **kw: L.JinaBertCfg(**dict(dict(width=128, layers=1, heads=2, head_dim=64, mlp_dim=256, vocab=10, max_pos=64, pool=L.MQ_POOL_MEAN, ln_eps=1e-12), **kw))
    for kw, what in ((dict(head_dim=128, heads=1), b"head_dim 128 unsupported"), (dict(width=2112, heads=33), b"width 2112"), (dict(width=100), b"width 100"),
                     (dict(heads=3), b"heads 3 x 64 is not the width 128"), (dict(mlp_dim=100), b"mlp_dim 100"), (dict(max_pos=9000), b"max_pos 9000"),
                     (dict(pool=L.MQ_POOL_LAST), b"bad pooling 2")):
        cfg = mk(**kw)
        refused(lib.mq_encode_jina_bert(C.byref(cfg), C.byref(w), None, None, None, 0, fake, 1, None, 0, None), b"mq_encode_jina_bert: " + what)
    cfg = mk()
    refused(lib.mq_encode_jina_bert(C.byref(cfg), None, fake, fake, fake, 1, fake, 1, fake, 0, None), b"mq_encode_jina_bert: null pointer")
    refused(lib.mq_encode_jina_bert(C.byref(cfg), C.byref(w), fake, fake, fake, 1, fake, 1, fake, 0, None), b"mq_encode_jina_bert: null weight pointer")
    layers = (L.JinaBertLayer * 1)(L.JinaBertLayer(*([4096] * 11)))
    w = L.JinaBertWeights(tok_emb=4096, type0=4096, emb_ln_g=4096, emb_ln_b=4096, d_slopes=4096, layers=layers)
    assert lib.mq_encode_jina_bert(C.byref(cfg), C.byref(w), None, None, None, 0, fake, 1, None, 0, None) == 0      # nseq 0: nothing to do
    holed = (L.JinaBertLayer * 1)(L.JinaBertLayer(*([4096] * 10)))
    w2 = L.JinaBertWeights(tok_emb=4096, type0=4096, emb_ln_g=4096, emb_ln_b=4096, d_slopes=4096, layers=holed)
    refused(lib.mq_encode_jina_bert(C.byref(cfg), C.byref(w2), fake, fake, fake, 1, fake, 1, fake, 0, None), b"layer 0 has null weights")
    cu = (C.c_int32 * 3)(0, 5, 12)
    refused(lib.mq_encode_jina_bert(C.byref(cfg), C.byref(w), None, fake, cu, 2, fake, 1, fake, 1 << 20, None), b"mq_encode_jina_bert: null input / workspace")
    need = lib.mq_jina_bert_workspace_bytes(C.byref(cfg), 12, 2)
    assert need >= 12 * 128 * 4 and lib.mq_jina_bert_workspace_bytes(None, 12, 2) == 0 and lib.mq_jina_bert_workspace_bytes(C.byref(cfg), 0, 2) == 0
    assert lib.mq_encode_jina_bert(C.byref(cfg), C.byref(w), fake, fake, cu, 2, fake, 1, fake, need - 1, None) == -3      # MQ_ERR_WORKSPACE
    assert b"mq_encode_jina_bert: workspace" in lib.mq_last_error()
    long = (C.c_int32 * 2)(0, 8193)
    refused(lib.mq_encode_jina_bert(C.byref(mk(max_pos=8192)), C.byref(w), fake, fake, long, 1, fake, 1, fake, 1 << 40, None),
            b"sequence lengths must be in [1, max_pos=8192]")
    # the plan: x fp32 + h bf16 + a bf16 + max(3 W, 2 F) bf16, each slice 256-byte aligned
    assert lib.mq_jina_bert_workspace_bytes(C.byref(mk(mlp_dim=320)), 12, 2) == need + 12 * (640 - 512) * 2
    assert lib.mq_abi_version() == 15


def test_header_names_the_entry_points():
    text = L.HEADER_PATH.read_text()
    for name in ("mq_attention_alibi", "mq_encode_jina_bert", "mq_jina_bert_workspace_bytes"):
        assert name in text and name in L.EXPORTED_SYMBOLS
    for name in ("mq_jina_bert_cfg", "mq_jina_bert_layer", "mq_jina_bert_weights"):
        assert f"}} {name};" in text
    assert "#define MQ_ABI_VERSION 15" in text


# ---- the inputs of the GPU kernel test ----------------------------------------------------------------------------------------------------------------
def test_reference_equals_attention_ref_where_that_can_express_the_bias():
    """attention_ref.reference takes an unclamped table and the scale 1 / sqrt(hs): the ALiBi bias as such a table gives the same numbers"""
    lens, heads, hd = [70, 9], 3, 64
    qkv = AR.make_qkv("randn", lens, heads, hd, seed=4)
    slopes = J.slopes_of(12)[8:11]
    out, absout = J.alibi_reference(qkv, lens, heads, hd, slopes, hd ** -0.5)
    o2, a2, _ = AR.reference(qkv, lens, heads, hd, AR.MASK_NONE, bias=J.alibi_table(slopes, 70))
    assert float((out - o2).abs().max()) < 1e-12 and float((absout - a2).abs().max()) < 1e-12


def test_readout_and_bias_only_inputs_keep_every_probability_above_2_pow_minus_100():
    """the precondition of the cases of tests/test_attention_alibi_gpu.py that isolate single probabilities, on exactly their inputs"""
    hd = 64
    for tag, lens, heads, scale, seed, _ in J.readout_cases():
        qkv = J.family_qkv("readout", lens, heads, hd, scale, seed)
        lo = J.min_log2_probability(qkv, lens, heads, hd, J.readout_slopes(max(lens), heads), scale)
        print(f"ALIBI_MINP readout {tag} heads={heads} scale={scale:.4f} lens={lens} log2(min p)={lo:.1f}")
        assert lo >= J.MIN_LOG2_P, (tag, lens, heads, lo)
    for lens in J.BIAS_ONLY:
        qkv = J.bias_only_qkv(lens, 2, hd)
        lo = J.min_log2_probability(qkv, lens, 2, hd, J.readout_slopes(max(lens), 2), 1.0)
        print(f"ALIBI_MINP bias_only lens={lens} log2(min p)={lo:.1f}")
        assert lo >= J.MIN_LOG2_P, (lens, lo)


def test_readout_slopes_are_distinct_values_of_the_real_lists():
    for n in (1, 64, 77, 300, 700, 1300):
        s = J.readout_slopes(n, 3).tolist()
        assert len(set(s)) == 3 and all(math.log2(v) == round(math.log2(v)) and -8 <= math.log2(v) <= -1 for v in s), (n, s)


@pytest.mark.parametrize("lens", J.BIAS_ONLY)
def test_bias_only_inputs_see_every_fault_of_the_bias(lens):
    heads, hd = 2, 64
    qkv = J.bias_only_qkv(lens, heads, hd)
    slopes = J.readout_slopes(max(lens), heads)
    out, absout = J.alibi_reference(qkv, lens, heads, hd, slopes, 1.0)
    # the output is softmax(bias row) applied to V
    r0 = 0
    for ln in lens:
        pos = torch.arange(ln)
        p = torch.softmax(-slopes.double()[:, None, None] * (pos[None, :] - pos[:, None]).abs().double()[None], -1)
        v = qkv[r0:r0 + ln, 2 * heads * hd:].double().reshape(ln, heads, hd).transpose(0, 1)
        assert float(((p @ v).transpose(0, 1).reshape(ln, heads * hd) - out[r0:r0 + ln]).abs().max()) < 1e-12
        r0 += ln
    for fault in J.BIAS_FAULTS:
        wrong, _ = J.alibi_reference(qkv, lens, heads, hd, slopes, hd ** -0.5 if fault == "bias_scaled" else 1.0, fault=fault)
        r = AR.worst_ratio(wrong, out, absout)
        print(f"ALIBI_FAULT lens={lens} {fault} ratio={r:.1f}")
        assert r > KERNEL_MARGIN, fault


# ---- the float64 pass and the mutants it must see -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def passes():
    out = {}
    for name in J.TINIES:
        b = J.build(name)
        lens = [len(s) for s in b["seqs"]]
        ids = torch.cat(b["seqs"])
        out[name] = dict(b, lens=lens, ids=ids, ex=J.exact(b["arch"], b["tensors"], ids, lens), mo=J.model(b["arch"], b["tensors"], ids, lens))
    return out


def _views(ps):
    return [("block%d" % i, b) for i, b in enumerate(ps.blocks)] + [("pooled/%s/l2=%d" % k, v) for k, v in ps.pooled.items()]


@pytest.mark.parametrize("name", tuple(J.TINIES))
def test_second_rounding_history_is_inside_the_bar(passes, name):
    p = passes[name]
    h1 = J.model(p["arch"], p["tensors"], p["ids"], p["lens"], hist=1)
    worst = 0.0
    for (view, got), (_, ex), (_, mo) in zip(_views(h1), _views(p["ex"]), _views(p["mo"])):
        r = J.row_ratio(got, ex, mo)["ratio"]
        print(f"JINA_HIST1 {name} {view} ratio={r:.3f}")
        worst = max(worst, r)
    assert worst <= MARGIN


@pytest.mark.parametrize("name, mut", [(n, m) for n in J.TINIES for m in J.MUTANTS])
def test_every_orchestration_mutant_leaves_the_bar(passes, name, mut):
    """what the GPU test's ratio check would measure for ONE defect of csrc/jina_bert.hip's orchestration: the last stream and the pooled rows it checks"""
    p = passes[name]
    mm = J.model(p["arch"], p["tensors"], p["ids"], p["lens"], mut=mut)
    rs = {view: J.row_ratio(got, ex, mo)["ratio"] for (view, got), (_, ex), (_, mo) in zip(_views(mm), _views(p["ex"]), _views(p["mo"]))}
    print(f"JINA_MUTANT {name} {mut}: " + " ".join(f"{k}={v:.1f}" for k, v in rs.items()))
    assert rs["block1"] > 2 * MARGIN and min(v for k, v in rs.items() if k.startswith("pooled")) > 2 * MARGIN


def test_the_exact_pass_is_the_formula_written_out():
    """one block of TINY_2H on one 5-token sequence, straight from the published block formula (module order, gated_layers' activated half in rows [:F]) in plain torch"""
    b = J.build("TINY_2H")
    arch, sd = b["arch"], b["sd"]
    ids = torch.tensor([7, 9, 11, 300, 42])
    W, F, H = arch.width, arch.mlp_dim, arch.heads
    d = {k: v.double() for k, v in sd.items() if v.is_floating_point()}
    ln = lambda y, n: torch.nn.functional.layer_norm(y, (W,), d[n + ".weight"], d[n + ".bias"], arch.ln_eps)
    x = ln(d["embeddings.word_embeddings.weight"][ids] + d["embeddings.token_type_embeddings.weight"][0], "embeddings.LayerNorm")
    p = "encoder.layer.0."
    q, k, v = ((x @ d[p + f"attention.self.{c}.weight"].T + d[p + f"attention.self.{c}.bias"]).reshape(5, H, 64).transpose(0, 1) for c in ("query", "key", "value"))
    pos = torch.arange(5)
    bias = -torch.tensor(arch.slopes()).float().double()[:, None, None] * (pos[None, :] - pos[:, None]).abs()[None]
    a = (torch.softmax(q @ k.transpose(1, 2) / 8.0 + bias, -1) @ v).transpose(0, 1).reshape(5, W)
    x = ln(a @ d[p + "attention.output.dense.weight"].T + d[p + "attention.output.dense.bias"] + x, p + "attention.output.LayerNorm")
    hg = x @ d[p + "mlp.gated_layers.weight"].T
    m = torch.nn.functional.gelu(hg[:, :F]) * hg[:, F:]
    x = ln(m @ d[p + "mlp.wo.weight"].T + d[p + "mlp.wo.bias"] + x, p + "mlp.layernorm")
    ex = J.exact(arch, b["tensors"], ids, [5], layers=1)
    assert float((ex.final - x).abs().max()) < 1e-10


# ---- the loader ---------------------------------------------------------------------------------------------------------------------------------------
class _Captured(Exception):
    pass


def _capture(monkeypatch):
    from marqo_amd.engine import jina_bert as EJ
    seen = {}

    def init(self, arch, sd, device, pooling="mean", precision="bf16"):
        seen.update(arch=arch, sd=sd, pooling=pooling, precision=precision)
        raise _Captured()
    monkeypatch.setattr(EJ.JinaBertTower, "__init__", init)
    return seen


def _model(props):
    from marqo_amd.s2_inference.hugging_face_model import HuggingFaceModel
    return HuggingFaceModel(model_properties=props, device="cuda:0")


@pytest.fixture(scope="module")
def ckpts(tmp_path_factory):
    b, tk = J.build("TINY_2H"), J.train_tokenizer()
    root = tmp_path_factory.mktemp("jina")
    return dict(plain=J.write_checkpoint_dir(str(root / "plain"), b["cfg"], b["sd"], tk),
                cls=J.write_checkpoint_dir(str(root / "cls"), b["cfg"], b["sd"], tk, pooling="cls"),
                short=J.write_checkpoint_dir(str(root / "short"), J.config_dict(b["cfg"], max_position_embeddings=48), b["sd"], tk),
                odd=J.write_checkpoint_dir(str(root / "odd"), J.config_dict(b["cfg"], feed_forward_type="original"), b["sd"], tk))


def test_hf_loader_takes_a_jina_bert_directory(ckpts, monkeypatch):
    from marqo_amd.engine.tokenizers import HfJsonTokenizer
    from marqo_amd.s2_inference.errors import InvalidModelPropertiesError
    seen = _capture(monkeypatch)
    for d, prop, want, tokens, cap in ((ckpts["plain"], None, "mean", 128, 128), (ckpts["cls"], None, "cls", 128, 128), (ckpts["cls"], "mean", "mean", 9000, 8192),
                                       (ckpts["plain"], "cls", "cls", 16, 16), (ckpts["short"], None, "mean", 128, 48)):
        props = {"type": "hf", "name": d, "dimensions": 128, "tokens": tokens, "trustRemoteCode": True}
        if prop:
            props["poolingMethod"] = prop
        m = _model(props)
        with pytest.raises(_Captured):
            m._load_necessary_components()
        assert isinstance(seen["arch"], archs.JinaBertArch) and seen["arch"].heads == 2
        assert isinstance(m._tokenizer, HfJsonTokenizer) and m._tokenizer.pad_id == 0 and m._tokenizer.cls_id is None
        assert seen["pooling"] == want and seen["precision"] == "bf16"
        assert m.model_properties.tokens == cap       # min(tokens, max_position_embeddings, 8192)
    ok = {"type": "hf", "name": ckpts["plain"], "dimensions": 128, "trustRemoteCode": True}
    with pytest.raises(InvalidModelPropertiesError, match="custom-code \\(JinaBERT\\) checkpoint: the reference loads it only with 'trustRemoteCode': True"):
        _model({k: v for k, v in ok.items() if k != "trustRemoteCode"})._load_necessary_components()
    with pytest.raises(InvalidModelPropertiesError, match="'enginePrecision': 'fp8' is not available for JinaBERT encoders"):
        _model(dict(ok, enginePrecision="fp8"))._load_necessary_components()
    with pytest.raises(InvalidModelPropertiesError, match="Original error pooling_method must be 'mean' or 'cls'"):
        _model(dict(ok, poolingMethod="last"))._load_necessary_components()
    with pytest.raises(InvalidModelPropertiesError, match="'dimensions'=64 but the encoder width is 128"):
        _model(dict(ok, dimensions=64))._load_necessary_components()
    with pytest.raises(InvalidModelPropertiesError, match="feed_forward_type=original unsupported"):
        _model(dict(ok, name=ckpts["odd"]))._load_necessary_components()


def test_token_rows_are_the_librarys(ckpts):
    """HfJsonTokenizer.plain on the directory: the `tokenizers` library's own ids, [CLS] .. [SEP] from the file's post-processor and kept under
    truncation, right-padded with [PAD]"""
    import os
    from tokenizers import Tokenizer
    from marqo_amd.engine.tokenizers import HfJsonTokenizer
    tk = HfJsonTokenizer.plain(ckpts["plain"], pad_fallback="[PAD]")
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
            assert w[0] == 2 and w[-1] == 3 and list(got["input_ids"][i, :len(w)]) == w and int(got["attention_mask"][i].sum()) == len(w)
            assert bool((got["input_ids"][i, len(w):] == 0).all())
    assert want[2] == [2, 3]          # the empty text is [CLS] [SEP]


def test_cross_encoders_on_this_tower_are_refused(tmp_path):
    from marqo_amd.engine.rerank import CrossEncoderTower
    b = J.build("TINY_2H")
    d = J.write_checkpoint_dir(str(tmp_path / "ce"), J.config_dict(b["cfg"], num_labels=1), b["sd"])
    with pytest.raises(ValueError, match="position_embedding_type='alibi' \\(JinaBERT\\) is not served as a cross-encoder"):
        CrossEncoderTower.from_dir(d, "cuda:0")


def test_registry_is_unchanged():
    from marqo_amd.s2_inference import s2_inference as S
    mp = S.load_model_properties()
    assert len(mp["models"]) == 204 and len(mp["loaders"]) == 12 and not any("jina" in n.lower() for n in mp["models"])

"""ModernBERT cross-encoders on the host (no GPU): the float64 model of the classification head against transformers' own head, the float32 model
of the kernel inside the GPU test's budget and its seeded faults outside it, the measured GELU constants, the loader's decisions, the pair layout
against the `tokenizers` library's own pair encoding, and the argument checks of mq_score_head_ln / mq_score_pairs_modernbert through ctypes."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from marqo_amd import _lib as L
from marqo_amd.engine import rerank as ER
from marqo_amd.engine.rerank import CrossEncoderTower, ModernBertCrossEncoderTower, hf_rows, pair_lengths
from tests import modernbert_ref as M
from tests import rerank_modernbert_ref as RM

GPU_WIDTHS = (64, 128, 1024, 2048)     # the widths of tests/test_rerank_modernbert_gpu.py::test_score_head_ln


# ---- the float64 head is transformers' head -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pooling", ["cls", "mean"])
@pytest.mark.parametrize("biases", [False, True])
def test_float64_head_is_transformers_head(pooling, biases):
    """ModernBertForSequenceClassification applies head (dense, GELU, LayerNorm), dropout and classifier to the pooled row; the pooling setting does not
    reach the head.  fp32 transformers must sit inside the fp32 rounding bound of the float64 model."""
    cfg = RM.classifier_config(pooling, classifier_bias=biases, norm_bias=biases)
    model = RM.hf_classifier(cfg, seed=3)
    sd = model.state_dict()
    assert ("head.dense.bias" in sd) == biases and ("head.norm.bias" in sd) == biases and "classifier.bias" in sd
    h = torch.randn(33, cfg["hidden_size"], generator=torch.Generator().manual_seed(1)) * 1.5
    with torch.no_grad():
        got = model.classifier(model.drop(model.head(h)))[:, 0].double().numpy()
    args = (h, sd["head.dense.weight"], sd.get("head.dense.bias"), sd["head.norm.weight"], sd.get("head.norm.bias"), sd["classifier.weight"],
            float(sd["classifier.bias"][0]), cfg["norm_eps"])
    z, Bz = RM.fp32_reference(*args)
    assert np.array_equal(z, RM.head_f64(*args))
    r = RM.ratio(got, z, Bz)
    print(f"float64 head vs transformers ({pooling}, biases {biases}): worst |fp32 - fp64| / fp32 bound = {r:.3f}; worst bound {Bz.max():.2e}, std of the logits {z.std():.2f}")
    assert r <= 1.0 and Bz.max() < 1e-2 * z.std()        # (the bound is below 1 % of the spread: a head of another structure is far outside)


def test_gelu_constants_are_the_measurement():
    """GELU_ABS / GELU_REL (MEASURED) hold on a fresh measurement and are not slack: within 10 % of it"""
    a, r = RM.measure_gelu(400_000)
    print(f"gelu_device against float64 erf: worst |error| inside the clamp {a:.3e}, worst |error| / |x| beyond it {r:.3e}")
    assert a <= RM.GELU_ABS <= 1.1 * a and r <= RM.GELU_REL <= 1.1 * r
    x = np.linspace(-6, 6, 1001).astype(np.float32)
    assert np.abs(RM.gelu_device(x) - torch.nn.functional.gelu(torch.from_numpy(x)).numpy()).max() <= RM.GELU_ABS + 6 * RM.GELU_REL


# ---- the float32 model of the kernel: inside the budget; its faults are not ---------------------------------------------------------------------
@pytest.mark.parametrize("W", GPU_WIDTHS)
def test_head_model_is_inside_the_budget_and_faults_are_not(W):
    c = RM.head_case(W, 67, seed=2)
    z, Bz, s, Bs = RM.head_reference(c)
    mz, ms = RM.model_head_ln(c)
    assert RM.ratio(mz, z, Bz) <= 1.0 and RM.ratio(ms, s, Bs) <= 1.0
    for fault in RM.FAULTS_HEAD_LN:        # named input: unrelated rows, both biases, classifier bias 0.37
        fz, _ = RM.model_head_ln(c, fault)
        r = RM.ratio(fz, z, Bz)
        print(f"W={W} {fault}: {r:.1f} x the budget")
        assert r > 1.25, fault
    for kw in (dict(dense_bias=False, norm_bias=False), dict(offset=40.0)):
        c = RM.head_case(W, 5, seed=2, **kw)
        z, Bz, s, Bs = RM.head_reference(c)
        mz, ms = RM.model_head_ln(c)
        assert RM.ratio(mz, z, Bz) <= 1.0 and RM.ratio(ms, s, Bs) <= 1.0, kw


# ---- from_dir's decisions -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def no_tower(monkeypatch):
    """the tower's constructor replaced by a recorder: the loader's decisions are read off its arguments"""
    seen = {}

    def init(self, arch, sd, device, tokenizer, **kw):
        seen.update(arch=arch, sd=sd, tokenizer=tokenizer, **kw)
    monkeypatch.setattr(ModernBertCrossEncoderTower, "__init__", init)
    return seen


@pytest.mark.parametrize("pooling", ["cls", "mean", None])
def test_from_dir_dispatches_modernbert_and_reads_the_pooling(tmp_path, no_tower, pooling):
    cfg, _ = RM.write_cross_encoder_dir(tmp_path, pooling or "cls")
    if pooling is None:          # the key's default is transformers' config class's: "cls"
        cfg = {k: v for k, v in cfg.items() if k != "classifier_pooling"}
        with open(tmp_path / "config.json", "w") as f:
            json.dump(cfg, f)
    t = CrossEncoderTower.from_dir(str(tmp_path), "cpu")
    assert isinstance(t, ModernBertCrossEncoderTower)
    assert no_tower["pooling"] == (pooling or "cls") and no_tower["classifier_bias"] is False and no_tower["norm_bias"] is False
    assert no_tower["arch"].max_pos == RM.MAX_POS and no_tower["model_max_length"] == RM.MAX_POS      # (no model_max_length in tokenizer_config.json)
    assert no_tower["tokenizer"].cls_id == 1 and no_tower["tokenizer"].sep_id == 2
    assert "head.norm.weight" in no_tower["sd"] and "model.final_norm.weight" in no_tower["sd"]


def test_from_dir_reads_model_max_length(tmp_path, no_tower):
    RM.write_cross_encoder_dir(tmp_path)
    p = tmp_path / "tokenizer_config.json"
    p.write_text(json.dumps(dict(RM.read_json(p), model_max_length=128)))
    CrossEncoderTower.from_dir(str(tmp_path), "cpu")
    assert no_tower["model_max_length"] == 128


@pytest.mark.parametrize("over, message", [
    (dict(num_labels=3, id2label=None, label2id=None), "num_labels=3 is not served as a cross-encoder"),
    (dict(classifier_activation="relu"), "classifier_activation='relu' is not served"),
    (dict(classifier_pooling="max"), "classifier_pooling='max' must be 'cls' or 'mean'"),
    (dict(num_attention_heads=4), "64-wide attention heads only"),
    (dict(attention_bias=True), "attention_bias=true are not supported"),
])
def test_from_dir_refuses(tmp_path, no_tower, over, message):
    cfg, _ = RM.write_cross_encoder_dir(tmp_path)
    cfg.update(over)
    with open(tmp_path / "config.json", "w") as f:
        json.dump({k: v for k, v in cfg.items() if v is not None}, f)
    with pytest.raises(ValueError, match=message):
        CrossEncoderTower.from_dir(str(tmp_path), "cpu")
    assert not no_tower, "a refused checkpoint reached the tower"


def test_from_dir_refuses_a_rope_type_it_does_not_run(tmp_path, no_tower):
    cfg, _ = RM.write_cross_encoder_dir(tmp_path)
    cfg["rope_parameters"] = {"full_attention": {"rope_type": "yarn", "rope_theta": 160000.0}, "sliding_attention": {"rope_type": "default", "rope_theta": 10000.0}}
    with open(tmp_path / "config.json", "w") as f:
        json.dump(cfg, f)
    with pytest.raises(ValueError, match="rope_type=yarn unsupported"):
        CrossEncoderTower.from_dir(str(tmp_path), "cpu")


def test_a_missing_head_tensor_is_named(tmp_path):
    """the real constructor: the head is read before anything touches a device"""
    RM.write_cross_encoder_dir(tmp_path, drop=("head.norm.weight",))
    with pytest.raises(ValueError, match="checkpoint is missing tensor 'head.norm.weight'"):
        CrossEncoderTower.from_dir(str(tmp_path), "cpu")


def test_a_missing_tokenizer_json_is_named(tmp_path, no_tower):
    from marqo_amd.s2_inference.errors import RerankerError
    from marqo_amd.s2_inference.reranking.cross_encoders import load_cross_encoder_model
    RM.write_cross_encoder_dir(tmp_path, tokenizer=False)
    with pytest.raises(ValueError, match="tokenizer.json, which is not there"):
        CrossEncoderTower.from_dir(str(tmp_path), "cpu")
    with pytest.raises(RerankerError, match="tokenizer.json, which is not there"):
        load_cross_encoder_model(str(tmp_path), "cpu")
    assert not no_tower


def test_other_model_types_keep_their_refusal(tmp_path):
    RM.write_cross_encoder_dir(tmp_path)
    cfg = dict(RM.read_json(tmp_path / "config.json"), model_type="deberta-v2")
    with open(tmp_path / "config.json", "w") as f:
        json.dump(cfg, f)
    with pytest.raises(ValueError) as e:
        CrossEncoderTower.from_dir(str(tmp_path), "cpu")
    assert str(e.value) == f"{tmp_path}: model_type='deberta-v2' is not served as a cross-encoder (only 'bert', 'xlm-roberta' and 'roberta')"


# ---- pair layout ---------------------------------------------------------------------------------------------------------------------------------------
def _pack_on_the_host(q_row, q_len, d_rows, d_lens, cap, cls_id, sep_id):
    """what mq_pair_plan_n / mq_pack_pairs (specials = 3) build from the singly-tokenised rows: pieces start at column 1, lengths count both specials"""
    la = int(q_len) - 2
    a, b = pair_lengths(la, np.asarray(d_lens) - 2, cap, 3)
    return [[cls_id, *q_row[1:1 + int(x)].tolist(), sep_id, *d_rows[i, 1:1 + int(y)].tolist(), sep_id] for i, (x, y) in enumerate(zip(a, b))]


@pytest.mark.parametrize("cap", [8, 9, 64])
def test_pair_layout_is_the_tokenizers_librarys(tmp_path, cap):
    from marqo_amd.engine.tokenizers import HfJsonTokenizer
    M.train_tokenizer(300).save(str(tmp_path / "tokenizer.json"))
    tok = HfJsonTokenizer(str(tmp_path))
    texts = ["", "fox", "hello world", "the quick brown fox", "a search engine ranks documents for a query",
             "rotary positions turn queries and keys by an angle , gated linear units multiply two projections . " * 2]
    seen = set()
    for query in texts:
        q_rows, q_len = hf_rows(tok, [query], None)
        la = int(q_len[0]) - 2
        ld = cap if la <= cap - 2 else la + 2           # (_PairScorer.score)
        d_rows, d_lens = hf_rows(tok, texts, ld)
        assert d_rows.shape == (len(texts), ld) and d_rows.dtype == np.int32 and (d_rows[:, 0] == tok.cls_id).all()
        assert all(d_rows[i, n - 1] == tok.sep_id and (d_rows[i, n:] == tok.pad_id).all() for i, n in enumerate(d_lens))
        mine = _pack_on_the_host(q_rows[0], q_len[0], d_rows, d_lens, cap, tok.cls_id, tok.sep_id)
        theirs = RM.pair_encodings(tmp_path, query, texts, cap)
        assert mine == theirs, (query, cap)
        for n in d_lens:
            lb = int(n) - 2
            seen.add(("empty" if min(la, lb) == 0 else "fits" if la + lb + 3 <= cap else "q>d" if la > lb else "q=d" if la == lb else "q<d"))
    assert seen >= {"empty", "q>d", "q=d", "q<d"} and (cap == 8 or "fits" in seen), seen


# ---- the library's argument checks (no launch) -----------------------------------------------------------------------------------------------------------
def test_new_entry_points_report_argument_errors_without_a_gpu():
    lib = L.load()
    fake = 256

    def refused(rc, msg):
        assert rc == -1 and msg in lib.mq_last_error(), (rc, lib.mq_last_error())

    assert C.sizeof(L.ScoreHeadLnWeights) == 48
    head = L.ScoreHeadLnWeights(dense_w=fake, dense_b=None, norm_g=fake, norm_b=None, cls_w=fake, cls_b=0.0, ln_eps=1e-5)
    refused(lib.mq_score_head_ln(fake, 1, 128, None, fake, None, fake, 1 << 20, None), b"mq_score_head_ln: null head")
    refused(lib.mq_score_head_ln(fake, 1, 96, C.byref(head), fake, None, fake, 1 << 20, None), b"mq_score_head_ln: W=96")
    refused(lib.mq_score_head_ln(fake, 1, 2112, C.byref(head), fake, None, fake, 1 << 20, None), b"mq_score_head_ln: W=2112")
    refused(lib.mq_score_head_ln(fake, 0, 128, C.byref(head), fake, None, fake, 1 << 20, None), b"mq_score_head_ln: n=0")
    refused(lib.mq_score_head_ln(None, 1, 128, C.byref(head), fake, None, fake, 1 << 20, None), b"mq_score_head_ln: null input")
    refused(lib.mq_score_head_ln(fake, 1, 128, C.byref(L.ScoreHeadLnWeights(dense_w=fake, cls_w=fake)), fake, None, fake, 1 << 20, None),
            b"mq_score_head_ln: null weight pointer")
    assert lib.mq_score_head_ln(fake, 1, 128, C.byref(head), fake, None, fake, 16, None) == -3 and b"workspace" in lib.mq_last_error()
    assert lib.mq_score_head_ln_workspace_bytes(5, 128) >= 5 * 128 * 6 + 128 * 4 and lib.mq_score_head_ln_workspace_bytes(0, 128) == 0

    cfg = L.ModernBertCfg(width=128, layers=1, heads=2, mlp_dim=192, vocab=10, max_pos=64, half_window=8, pool=L.MQ_POOL_CLS, ln_eps=1e-5)
    w = L.ModernBertWeights()
    n = lib.mq_score_pairs_modernbert_workspace_bytes(C.byref(cfg), 100, 3)
    assert n >= lib.mq_modernbert_workspace_bytes(C.byref(cfg), 100, 3) + 3 * 128 * 4 + lib.mq_score_head_ln_workspace_bytes(3, 128)
    cu = np.asarray([0, 70], dtype=np.int32)
    call = lambda cfg_, head_, nseq, cu_=cu: lib.mq_score_pairs_modernbert(C.byref(cfg_), C.byref(w), head_, fake, fake, cu_.ctypes.data, nseq, fake, None, None,
                                                                           fake, n, None)
    refused(call(cfg, None, 1), b"mq_score_pairs_modernbert: null head")
    refused(call(cfg, C.byref(head), 0), b"mq_score_pairs_modernbert: nseq=0")
    refused(call(cfg, C.byref(head), 1), b"mq_score_pairs_modernbert: sequence lengths must be in [1, max_pos=64]")
    bad_pool = L.ModernBertCfg(width=128, layers=1, heads=2, mlp_dim=192, vocab=10, max_pos=64, half_window=8, pool=L.MQ_POOL_LAST, ln_eps=1e-5)
    refused(call(bad_pool, C.byref(head), 1), b"mq_score_pairs_modernbert: bad pooling 2")
    wide = L.ModernBertCfg(width=96, layers=1, heads=2, mlp_dim=192, vocab=10, max_pos=64, half_window=8, pool=L.MQ_POOL_CLS, ln_eps=1e-5)
    refused(call(wide, C.byref(head), 1), b"mq_score_pairs_modernbert: W=96")
    # what the encoder refuses it refuses here too, under its own name: null weights are judged before any launch
    refused(call(cfg, C.byref(head), 1, np.asarray([0, 7], dtype=np.int32)), b"mq_encode_modernbert: null weight pointer")
    assert os.path.isfile(L.HEADER_PATH) and "mq_score_pairs_modernbert" in open(L.HEADER_PATH).read()
    assert ER._PairScorer.score is CrossEncoderTower.score is ModernBertCrossEncoderTower.score      # ONE scoring loop

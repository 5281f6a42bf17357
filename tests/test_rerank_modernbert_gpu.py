"""ModernBERT cross-encoders on the GPU (csrc/rerank.hip mq_score_head_ln / mq_score_pairs_modernbert, engine/rerank.py
ModernBertCrossEncoderTower, s2_inference/reranking): the head against the float64 model and budget of tests/rerank_modernbert_ref.py, the wiring
against mq_encode_modernbert and mq_score_head_ln bit for bit, score() against transformers' ModernBertForSequenceClassification on the `tokenizers`
library's pair encoding, and the public call.  Outputs sit inside guard-filled buffers."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from marqo_amd import _lib as L
from marqo_amd.engine.rerank import CrossEncoderTower, ModernBertCrossEncoderTower
from tests import rerank_modernbert_ref as RM

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# Worst |logit - fp32 transformers logit| over the pairs of test_score_matches_transformers (24 pairs at max_length 64 — three queries against eight
# documents each — and one pair at 300 tokens), per pooling, as MEASURED on the MI355X on the first run of this test.  The tolerance is twice the
# measurement: tile plans and batch compositions differ in summation order.  It must stay below a quarter of the standard deviation of the reference
# logits (asserted): the reference logits spread by 1.029 (cls) and 1.529 (mean), so 0.040 < 0.257 and 0.066 < 0.382.  The pair at 300 tokens was
# off by 3.0e-03 (cls) and 2.8e-02 (mean); a shuffled call returned the same bits.
LOGIT_ERR_MEASURED = {"cls": 1.9868e-02, "mean": 3.3100e-02}
LOGIT_TOL = {k: 2 * v for k, v in LOGIT_ERR_MEASURED.items()}


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def _sync_check(rc, what):
    L.check(rc, what)
    torch.cuda.synchronize(DEV)


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)


def _f32(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _head_of(c, keep):
    """mq_score_head_ln_weights of a rerank_modernbert_ref.head_case; `keep` holds the device tensors alive"""
    wd = torch.from_numpy(c["Wd"]).to(torch.bfloat16).to(DEV)          # (bf16 values already: exact)
    bd, g, b, wc = _f32(c["bd"]), _f32(c["g"]), _f32(c["b"]), _f32(c["wc"])
    keep.extend((wd, bd, g, b, wc))
    return L.ScoreHeadLnWeights(dense_w=wd.data_ptr(), dense_b=L.ptr(bd), norm_g=g.data_ptr(), norm_b=L.ptr(b), cls_w=wc.data_ptr(), cls_b=c["bc"],
                                ln_eps=c["eps"])


def _run_head(c, with_scores=True):
    """-> (logits, scores | None) numpy [n], after checking the guards around both outputs"""
    lib = L.load()
    n, W = c["h"].shape
    keep = []
    head = _head_of(c, keep)
    h = _f32(c["h"])
    out = torch.full((2, n + 4), float("nan"), dtype=torch.float32, device=DEV)
    ws = torch.empty(lib.mq_score_head_ln_workspace_bytes(n, W) + 256, dtype=torch.uint8, device=DEV)
    _sync_check(lib.mq_score_head_ln(h.data_ptr(), n, W, C.byref(head), out[0, 2:].data_ptr(), out[1, 2:].data_ptr() if with_scores else None,
                                     ws.data_ptr(), ws.numel(), _stream()), "mq_score_head_ln")
    assert bool(out[:, :2].isnan().all()) and bool(out[:, 2 + n:].isnan().all()), "a guard word changed"
    if not with_scores:
        assert bool(out[1].isnan().all()), "scores were written although none were asked for"
    got = out[:, 2:2 + n].cpu().numpy()
    return got[0], (got[1] if with_scores else None)


# ---- head ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [64, 128, 1024, 2048])          # one column per lane, two per lane, ..., the upper limit
@pytest.mark.parametrize("n", [1, 3, 4, 5, 67])               # less than one workgroup of 4 waves, exactly one, one more, a ragged last block
def test_score_head_ln(W, n):
    for dense_bias, norm_bias in ((True, True), (False, False), (True, False), (False, True)):
        c = RM.head_case(W, n, seed=4, dense_bias=dense_bias, norm_bias=norm_bias)
        z, Bz, s, Bs = RM.head_reference(c)
        logits, scores = _run_head(c)
        rz, rs = RM.ratio(logits, z, Bz), RM.ratio(scores, s, Bs)
        print(f"score_head_ln W={W} n={n} dense bias {dense_bias} norm bias {norm_bias}: worst / budget logits {rz:.3f} sigmoid {rs:.3f}")
        assert rz <= 1.0 and rs <= 1.0
        only, none = _run_head(c, with_scores=False)        # no sigmoid asked for: the same logits, nothing else written
        assert none is None and np.array_equal(only.view(np.int32), logits.view(np.int32))


@pytest.mark.parametrize("W", [64, 1024])
def test_score_head_ln_rows_of_large_common_offset(W):
    """every column of a row of the GELU output sits at about 40 with a spread of about 1: what a one-pass variance gets wrong"""
    c = RM.head_case(W, 5, seed=5, offset=40.0)
    z, Bz, s, Bs = RM.head_reference(c)
    logits, scores = _run_head(c)
    rz, rs = RM.ratio(logits, z, Bz), RM.ratio(scores, s, Bs)
    print(f"score_head_ln W={W} offset 40: worst / budget logits {rz:.3f} sigmoid {rs:.3f}")
    assert rz <= 1.0 and rs <= 1.0


# ---- wiring --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ckpt(tmp_path_factory):
    """one directory and its transformers model per pooling"""
    out = {}
    for pooling in ("cls", "mean"):
        d = str(tmp_path_factory.mktemp("mbce_" + pooling))
        cfg, model = RM.write_cross_encoder_dir(d, pooling, seed=0)
        out[pooling] = dict(dir=d, cfg=cfg, model=model)
    return out


@pytest.fixture(scope="module")
def towers(ckpt):
    cache = {}

    def get(pooling):
        if pooling not in cache:
            cache[pooling] = CrossEncoderTower.from_dir(ckpt[pooling]["dir"], DEV)
        return cache[pooling]
    return get


@pytest.mark.parametrize("pooling", ["mean", "cls"])
def test_score_pairs_pooled_rows_are_mq_encode_modernberts(towers, pooling):
    """TINY: 4 layers, 2 heads, local_attention 16; lengths 5 .. 130: the band kernel and full attention both run, one sequence crosses a 64-query slice"""
    t = towers(pooling)
    assert isinstance(t, ModernBertCrossEncoderTower) and t.pooling == pooling and t.cfg.pool == (L.MQ_POOL_MEAN if pooling == "mean" else L.MQ_POOL_CLS)
    assert t.arch.layers == 4 and t.arch.heads == 2 and t.arch.half_window == 8
    lib, W = t.lib, t.arch.width
    lens = [5, 17, 64, 65, 130]
    n = len(lens)
    cu_np = np.zeros(n + 1, dtype=np.int32)
    np.cumsum(lens, out=cu_np[1:])
    rows = int(cu_np[-1])
    ids = _i32(np.random.default_rng(11).integers(3, t.arch.vocab, rows))
    cu, d_cu = torch.from_numpy(cu_np), _i32(cu_np)
    out = torch.full((3, n + 2), float("nan"), dtype=torch.float32, device=DEV)
    pooled = torch.full((n + 1, W), float("nan"), dtype=torch.float32, device=DEV)
    with torch.cuda.device(DEV):
        ws = torch.empty(lib.mq_score_pairs_modernbert_workspace_bytes(C.byref(t.cfg), rows, n) + 256, dtype=torch.uint8, device=DEV)
        t.score_packed(ids, d_cu, cu, out[0, 1:], out[1, 1:], pooled, ws)
        ref = torch.full((n, W), float("nan"), dtype=torch.float32, device=DEV)
        ws2 = torch.empty(lib.mq_modernbert_workspace_bytes(C.byref(t.cfg), rows, n) + 256, dtype=torch.uint8, device=DEV)
        L.check(lib.mq_encode_modernbert(C.byref(t.cfg), C.byref(t.w), ids.data_ptr(), d_cu.data_ptr(), cu.data_ptr(), n, ref.data_ptr(), 0, ws2.data_ptr(),
                                         ws2.numel(), _stream()), "mq_encode_modernbert")
        ws3 = torch.empty(lib.mq_score_head_ln_workspace_bytes(n, W) + 256, dtype=torch.uint8, device=DEV)
        L.check(lib.mq_score_head_ln(ref.data_ptr(), n, W, C.byref(t.head), out[2, 1:].data_ptr(), None, ws3.data_ptr(), ws3.numel(), _stream()),
                "mq_score_head_ln")
        torch.cuda.synchronize(DEV)
    assert bool(torch.isfinite(ref).all())
    assert torch.equal(pooled[:n], ref) and torch.equal(pooled[:n].view(torch.int32), ref.view(torch.int32)), \
        "the pooled rows differ from mq_encode_modernbert(normalize = 0)"
    assert torch.equal(out[0, 1:1 + n].view(torch.int32), out[2, 1:1 + n].view(torch.int32)), "the logits differ from mq_score_head_ln on the pooled rows"
    assert bool(pooled[n].isnan().all()) and bool(out[:, 0].isnan().all()) and bool(out[:, -1].isnan().all())
    assert bool(torch.isfinite(out[:2, 1:1 + n]).all())


# ---- end to end -------------------------------------------------------------------------------------------------------------------------------------------
def _pairs():
    """three queries against eight documents each: 24 pairs of 11 .. 64 tokens at max_length 64 (some cut)"""
    out = []
    for qi in range(3):
        docs = [RM.sentence(1 + 2 * i, 50 + 8 * qi + i) for i in range(8)]
        docs[3] = "  " + docs[3] + " \n"                   # stripped, as CrossEncoder strips
        out.append((RM.sentence(2 + 3 * qi, 9 + qi), docs))
    return out


@pytest.fixture(scope="module")
def references(ckpt):
    """fp32 transformers logits on the `tokenizers` library's pair encoding, computed once per pooling"""
    out = {}
    for pooling, k in ckpt.items():
        short = [RM.hf_logits(k["model"], RM.pair_encodings(k["dir"], q, docs, 64)) for q, docs in _pairs()]
        long_q, long_d = RM.sentence(20, 77), RM.sentence(400, 78)
        enc = RM.pair_encodings(k["dir"], long_q, [long_d], 300)
        assert len(enc[0]) == 300
        out[pooling] = dict(short=short, long=RM.hf_logits(k["model"], enc), long_pair=(long_q, long_d))
    return out


@pytest.mark.parametrize("pooling", ["cls", "mean"])
def test_score_matches_transformers(towers, references, pooling):
    t, ref = towers(pooling), references[pooling]
    errs, moved, all_ref = [], [], np.concatenate(ref["short"])
    for (query, docs), z in zip(_pairs(), ref["short"]):
        logits, scores = t.score(query, docs, 64)
        assert logits.dtype == np.float32 and logits.shape == (8,) and scores.shape == (8,)
        assert np.allclose(scores, 1.0 / (1.0 + np.exp(-logits.astype(np.float64))), rtol=0, atol=1e-6)
        errs.append(float(np.abs(logits - z).max()))
        perm = np.random.default_rng(5).permutation(8)            # a shuffled input: the results come back in the order of `docs`
        shuffled, _ = t.score(query, [docs[i] for i in perm], 64)
        moved.append(float(np.abs(shuffled - logits[perm]).max()))
    long_q, long_d = ref["long_pair"]
    logit_long, _ = t.score(long_q, [long_d], 300)
    err_long = float(np.abs(logit_long - ref["long"]).max())
    err, std = max(max(errs), err_long), float(all_ref.std())
    print(f"ModernBERT cross-encoder ({pooling}): worst |logit - fp32 transformers| = {err:.4e} (at 300 tokens {err_long:.4e}); "
          f"std of the reference logits = {std:.3f}; worst |logit - logit of the shuffled call| = {max(moved):.3e}")
    assert std >= 1.0
    assert LOGIT_TOL[pooling] < std / 4, "finding: the tolerance is not below a quarter of the spread of the logits"
    assert err <= LOGIT_TOL[pooling]
    assert max(moved) <= LOGIT_TOL[pooling], "the results are not in the order of `docs`"


# ---- the public call ------------------------------------------------------------------------------------------------------------------------------------------
def test_rerank_search_results_on_the_engine(ckpt, monkeypatch):
    from marqo_amd.s2_inference.reranking.rerank import rerank_search_results
    from marqo_amd.s2_inference.s2_inference import _create_model_cache_key, get_available_models
    k = ckpt["mean"]
    name, query = k["dir"], RM.sentence(5, 1)
    texts = [RM.sentence(3 + 2 * i, 400 + i) for i in range(6)]          # one sentence per field: one chunk per hit
    z = RM.hf_logits(k["model"], RM.pair_encodings(name, query, texts, 512))
    gaps = np.diff(np.sort(z))
    assert gaps.min() > 2 * LOGIT_TOL["mean"], f"the fixture's logits are closer than the tolerance can tell apart: {np.sort(z)}"
    hits = [{"_id": f"doc{i}", "body": texts[i], "_score": 0.5 + 0.01 * i} for i in range(6)]
    result = {"hits": copy.deepcopy(hits), "limit": 6}
    rerank_search_results(result, query, name, DEV)
    key = _create_model_cache_key(name, DEV)
    assert key in get_available_models()
    model = get_available_models()[key]["model"]
    assert isinstance(model.tower, ModernBertCrossEncoderTower)
    assert [h["_id"] for h in result["hits"]] == [f"doc{i}" for i in np.argsort(-z)], "the reranked order is not the order of the transformers logits"
    for h in result["hits"]:
        i = int(h["_id"][3:])
        assert abs(h["_score"] - 1.0 / (1.0 + np.exp(-z[i]))) <= LOGIT_TOL["mean"] / 4 + 1e-6       # (sigmoid' <= 1 / 4)
        assert h["_highlights"] == [{"body": texts[i]}]
    # a second call finds the model in the cache: nothing is loaded
    monkeypatch.setattr(CrossEncoderTower, "from_dir", classmethod(lambda cls, *a, **kw: (_ for _ in ()).throw(AssertionError("loaded twice"))))
    again = {"hits": copy.deepcopy(hits)}
    rerank_search_results(again, query, name, DEV)
    assert get_available_models()[key]["model"] is model
    assert [(h["_id"], h["_score"]) for h in again["hits"]] == [(h["_id"], h["_score"]) for h in result["hits"]]
    del get_available_models()[key]

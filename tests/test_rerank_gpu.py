"""Text reranking on the GPU (csrc/rerank.hip, engine/rerank.py, s2_inference/reranking): pair packing against BertTokenizerFast, the typed
embedding and the head against the budgets of tests/rerank_ref.py, the wiring of mq_score_pairs_bert against mq_encode_bert bit for bit,
CrossEncoderTower.score against transformers' BertForSequenceClassification, and the public call.  Outputs sit inside guard-filled buffers."""
import copy
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rerank_ref as RR  # noqa: E402
from marqo_amd import _lib as L  # noqa: E402
from marqo_amd.engine.rerank import CrossEncoderTower, pair_lengths  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = -7777

# Worst |logit - fp32 transformers logit| over the pairs of test_score_matches_transformers (24 pairs at max_length 64 and one at 512), as MEASURED
# on the MI355X on the first run of this test, per shape; both towers took the bf16 residual stream at load.  The reference logits spread by 1.526
# (tinybert) and 2.130 (minilm), so the error is 9 % and 12 % of the spread; minilm's worst pair is the one at 512 tokens.  The tolerance is twice
# the measurement: tile plans and batch compositions differ in summation order.  It must stay below a quarter of the standard deviation of the
# reference logits (asserted): 0.263 < 0.381 and 0.507 < 0.533.
LOGIT_ERR_MEASURED = {"tinybert": 1.3170e-01, "minilm": 2.5338e-01}
LOGIT_TOL = {k: 2 * v for k, v in LOGIT_ERR_MEASURED.items()}


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def _sync_check(rc, what):
    L.check(rc, what)
    torch.cuda.synchronize(DEV)


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)


def _f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _guarded_i32(n, pad=8):
    return torch.full((n + 2 * pad,), GUARD, dtype=torch.int32, device=DEV), pad


def _guards_intact(buf, pad, n):
    return bool((buf[:pad] == GUARD).all()) and bool((buf[pad + n:] == GUARD).all())


@pytest.fixture(scope="module")
def dirs(tmp_path_factory):
    root = tmp_path_factory.mktemp("ce")
    out = {}
    for shape in RR.SHAPES:
        out[shape] = str(root / shape)
        RR.write_cross_encoder_dir(out[shape], shape, seed=0)
        out[shape + "_eq"] = str(root / (shape + "_eq"))
        RR.write_cross_encoder_dir(out[shape + "_eq"], shape, seed=0, equal_type_rows=True)
    return out


@pytest.fixture(scope="module")
def towers(dirs):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = CrossEncoderTower.from_dir(dirs[name], DEV)
        return cache[name]
    return get


# ---- pack ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_length", [16, 64])
def test_pack_pairs_equals_the_fast_tokenizer(tmp_path, max_length):
    from marqo_amd.engine.gpu_tokenizers import DeviceWordPieceTokenizer
    from marqo_amd.engine.tokenizers import WordPieceTokenizer
    lib = L.load()
    RR.write_vocab(tmp_path)
    host = WordPieceTokenizer(str(tmp_path))
    dtok = DeviceWordPieceTokenizer(host, DEV)
    hf = RR.fast_tokenizer(tmp_path)
    n, lbs = 40, (0, 1, 6, 13, 14, 61, 200)
    docs = [RR.words(lbs[i % len(lbs)], seed=300 + i) for i in range(n)]
    for la in (0, 1, 5, 6, 7, 30):
        query = RR.words(la, seed=200 + la)
        d_q, qlen = dtok.encode_device([query], max(len(query) + 2, 4))
        assert int(qlen[0]) - 2 == la
        ld = max_length if la <= max_length - 2 else la + 2
        d_docs, dlen = dtok.encode_device(docs, ld)
        dlen = dlen.numpy()
        a, b = pair_lengths(la, dlen - 2, max_length)
        total = a + b + 3
        cu = np.zeros(n + 1, dtype=np.int32)
        np.cumsum(total, out=cu[1:])
        rows = int(cu[-1])
        (ka, p), (kb, _), (kt, _) = _guarded_i32(n), _guarded_i32(n), _guarded_i32(n)
        (ids, q), (types, _) = _guarded_i32(rows), _guarded_i32(rows)
        d_query = d_q[0, 1:1 + la].contiguous()
        d_docs, d_dlen, d_cu = d_docs.contiguous(), _i32(dlen), _i32(cu)
        L.check(lib.mq_pair_plan(la, d_dlen.data_ptr(), n, ld, max_length, ka[p:].data_ptr(), kb[p:].data_ptr(), kt[p:].data_ptr(), _stream()),
                "mq_pair_plan")
        _sync_check(lib.mq_pack_pairs(d_query.data_ptr() if la else None, la, d_docs.data_ptr(), ld, ka[p:].data_ptr(), kb[p:].data_ptr(),
                                      d_cu.data_ptr(), n, host.cls_id, host.sep_id, ids[q:].data_ptr(), types[q:].data_ptr(), rows, _stream()),
                    "mq_pack_pairs")
        enc = hf([query] * n, docs, truncation="longest_first", max_length=max_length)
        assert ka[p:p + n].cpu().tolist() == a.tolist() and kb[p:p + n].cpu().tolist() == b.tolist() and kt[p:p + n].cpu().tolist() == total.tolist()
        assert [len(e) for e in enc["input_ids"]] == total.tolist(), (la, max_length)
        assert ids[q:q + rows].cpu().tolist() == [t for e in enc["input_ids"] for t in e], (la, max_length)
        assert types[q:q + rows].cpu().tolist() == [t for e in enc["token_type_ids"] for t in e], (la, max_length)
        for buf, pad, m in ((ka, p, n), (kb, p, n), (kt, p, n), (ids, q, rows), (types, q, rows)):
            assert _guards_intact(buf, pad, m), "a guard word changed"
    assert lib.mq_pair_plan(3, 256, 1, 16, 3, 256, 256, 256, None) == -1       # max_length < 4 is refused


# ---- typed embedding ---------------------------------------------------------------------------------------------------------------------------
def _embed_typed(c, tids, W):
    lib = L.load()
    rows = int(c["cu"][-1])
    x = torch.full((rows + 2, W), float("nan"), dtype=torch.float32, device=DEV)
    keep = [_i32(c["ids"]), _i32(tids), _i32(c["cu"]), _f32(c["tok"]), _f32(c["pos"]), _f32(c["typ"]), _f32(c["g"]), _f32(c["b"])]
    ids, t, cu, tok, pos, typ, g, b = keep
    _sync_check(lib.mq_embed_tokens_typed(ids.data_ptr(), t.data_ptr(), cu.data_ptr(), len(c["cu"]) - 1, tok.data_ptr(), pos.data_ptr(), typ.data_ptr(),
                                          c["typ"].shape[0], g.data_ptr(), b.data_ptr(), x.data_ptr(), None, W, c["tok"].shape[0], c["eps"], 0,
                                          _stream()), "mq_embed_tokens_typed")
    assert bool(x[rows:].isnan().all()), "rows past the call changed"
    return x[:rows]


@pytest.mark.parametrize("W", [128, 384, 1024])
def test_embed_tokens_typed(W):
    lib = L.load()
    lens = [1, 3, 64, 65]
    c = RR.embed_case(W, lens, seed=3)
    rows = int(c["cu"][-1])
    # all types 0: the bits of mq_embed_tokens
    zero = _embed_typed(c, np.zeros(rows, np.int32), W)
    plain = torch.full((rows, W), float("nan"), dtype=torch.float32, device=DEV)
    ids, cu, tok, pos, typ, g, b = _i32(c["ids"]), _i32(c["cu"]), _f32(c["tok"]), _f32(c["pos"]), _f32(c["typ"]), _f32(c["g"]), _f32(c["b"])
    _sync_check(lib.mq_embed_tokens(ids.data_ptr(), cu.data_ptr(), len(lens), tok.data_ptr(), pos.data_ptr(), typ[0].data_ptr(), g.data_ptr(), b.data_ptr(),
                                    plain.data_ptr(), None, W, c["tok"].shape[0], c["eps"], 0, _stream()), "mq_embed_tokens")
    assert torch.equal(zero.view(torch.int32), plain.view(torch.int32)), "all-zero type ids must reproduce mq_embed_tokens bit for bit"
    # mixed types: the budget, element by element
    y, B = RR.embed_reference(c)
    got = _embed_typed(c, c["tids"], W)
    r = RR.ratio(got.cpu().numpy(), y, B)
    print(f"embed_tokens_typed W={W}: worst |kernel - fp64| / budget = {r:.3f}")
    assert r <= 1.0
    # out-of-range type ids clamp to the table
    wild = c["tids"].copy()
    wild[wild == 1] = 5
    wild[::7] = np.where(c["tids"][::7] == 0, -3, wild[::7])
    assert torch.equal(_embed_typed(c, wild, W).view(torch.int32), got.view(torch.int32))


# ---- head ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [128, 384, 1024])
@pytest.mark.parametrize("n", [1, 5, 64, 65])
def test_score_head(W, n):
    lib = L.load()
    c = RR.head_case(W, n, seed=4)
    h = _f32(c["x"][np.asarray(c["cu"][:-1], dtype=np.int64)])
    wp = torch.from_numpy(c["Wp"]).to(torch.bfloat16).to(DEV)          # (bf16 values already: exact)
    bp, wc = _f32(c["bp"]), _f32(c["wc"])
    head = L.ScoreHeadWeights(pooler_w=wp.data_ptr(), pooler_b=bp.data_ptr(), cls_w=wc.data_ptr(), cls_b=c["bc"], type_vocab=2)
    out = torch.full((2, n + 4), float("nan"), dtype=torch.float32, device=DEV)
    ws = torch.empty(lib.mq_score_head_workspace_bytes(n, W) + 256, dtype=torch.uint8, device=DEV)
    _sync_check(lib.mq_score_head(h.data_ptr(), n, W, C.byref(head), out[0, 2:].data_ptr(), out[1, 2:].data_ptr(), ws.data_ptr(), ws.numel(), _stream()),
                "mq_score_head")
    assert bool(out[:, :2].isnan().all()) and bool(out[:, 2 + n:].isnan().all()), "a guard word changed"
    z, Bz, s, Bs = RR.head_reference(c)
    got = out[:, 2:2 + n].cpu().numpy()
    rz, rs = RR.ratio(got[0], z, Bz), RR.ratio(got[1], s, Bs)
    print(f"score_head W={W} n={n}: worst / budget logits {rz:.3f} sigmoid {rs:.3f}")
    assert rz <= 1.0 and rs <= 1.0
    only = torch.full((n + 2,), float("nan"), dtype=torch.float32, device=DEV)     # no sigmoid asked for: the same logits, nothing else written
    _sync_check(lib.mq_score_head(h.data_ptr(), n, W, C.byref(head), only[1:].data_ptr(), None, ws.data_ptr(), ws.numel(), _stream()), "mq_score_head")
    assert torch.equal(only[1:1 + n].view(torch.int32), out[0, 2:2 + n].view(torch.int32)) and bool(only[0].isnan()) and bool(only[-1].isnan())


# ---- wiring --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["tinybert", "minilm"])
def test_score_pairs_cls_rows_are_mq_encode_berts(towers, shape):
    """equal type rows: the typed embedding adds what mq_encode_bert adds, so the final [CLS] rows must agree bit for bit"""
    t = towers(shape + "_eq")
    lib, W = t.lib, t.arch.width
    lens = [4, 5, 17, 63, 64, 65, 128, 257, 512]
    n = len(lens)
    cu_np = np.zeros(n + 1, dtype=np.int32)
    np.cumsum(lens, out=cu_np[1:])
    rows = int(cu_np[-1])
    g = np.random.default_rng(11)
    ids = _i32(g.integers(5, len(RR.VOCAB), rows))
    tids = _i32(np.concatenate([(np.arange(m) >= (m + 1) // 2).astype(np.int32) for m in lens]))
    cu, d_cu = torch.from_numpy(cu_np), _i32(cu_np)
    out = torch.full((3, n + 2), float("nan"), dtype=torch.float32, device=DEV)
    cls_rows = torch.full((n + 1, W), float("nan"), dtype=torch.float32, device=DEV)
    with torch.cuda.device(DEV):
        ws = torch.empty(lib.mq_score_pairs_workspace_bytes(C.byref(t.cfg), rows, n) + 256, dtype=torch.uint8, device=DEV)
        t.score_packed(ids, tids, d_cu, cu, out[0, 1:], out[1, 1:], cls_rows, ws)
        ref = torch.full((n, W), float("nan"), dtype=torch.float32, device=DEV)
        ws2 = torch.empty(lib.mq_bert_workspace_bytes(C.byref(t.cfg), rows, n) + 256, dtype=torch.uint8, device=DEV)
        L.check(lib.mq_encode_bert(C.byref(t.cfg), C.byref(t.w), ids.data_ptr(), d_cu.data_ptr(), cu.data_ptr(), n, ref.data_ptr(), 0, ws2.data_ptr(),
                                   ws2.numel(), _stream()), "mq_encode_bert")
        torch.cuda.synchronize(DEV)
    assert t.cfg.pool == L.MQ_POOL_CLS
    assert bool(torch.isfinite(ref).all())
    assert torch.equal(cls_rows[:n].view(torch.int32), ref.view(torch.int32)), "the [CLS] rows differ from mq_encode_bert(pool=CLS, normalize=0)"
    assert bool(cls_rows[n].isnan().all()) and bool(out[:, 0].isnan().all()) and bool(out[:, -1].isnan().all()) and bool(out[2].isnan().all())
    assert bool(torch.isfinite(out[:2, 1:1 + n]).all())


# ---- end to end -------------------------------------------------------------------------------------------------------------------------------------------
def _pairs():
    query = RR.sentences(6, seed=9)
    docs = [RR.sentences(4 + 3 * i, seed=50 + i) for i in range(24)]
    docs[3] = "  " + docs[3] + " \n"                   # stripped, as CrossEncoder strips
    return query, docs


@pytest.mark.parametrize("shape", ["tinybert", "minilm"])
def test_score_matches_transformers(dirs, towers, shape):
    t = towers(shape)
    query, docs = _pairs()
    ref = RR.hf_logits(dirs[shape], query, docs, 64)
    logits, scores = t.score(query, docs, 64)
    long_q, long_d = RR.sentences(40, seed=77), RR.sentences(700, seed=78)
    ref_long = RR.hf_logits(dirs[shape], long_q, [long_d], 512)
    logit_long, _ = t.score(long_q, [long_d], 512)
    assert logits.dtype == np.float32 and logits.shape == (24,) and scores.shape == (24,)
    err = float(max(np.abs(logits - ref).max(), np.abs(logit_long - ref_long).max()))
    std = float(ref.std())
    print(f"cross-encoder {shape}: worst |logit - fp32 transformers| = {err:.4e} (at 512 tokens {float(np.abs(logit_long - ref_long).max()):.4e}); "
          f"std of the reference logits = {std:.3f}; residual stream {t.residual_stream}")
    assert np.allclose(scores, 1.0 / (1.0 + np.exp(-logits.astype(np.float64))), rtol=0, atol=1e-6)
    assert std >= 1.0
    assert LOGIT_TOL[shape] < std / 4, "finding: the tolerance is not below a quarter of the spread of the logits"
    assert err <= LOGIT_TOL[shape]


# ---- the public call ------------------------------------------------------------------------------------------------------------------------------------------
def test_rerank_search_results_on_the_engine(dirs, monkeypatch):
    from marqo_amd.s2_inference.processing.text import split_text
    from marqo_amd.s2_inference.reranking import cross_encoders
    from marqo_amd.s2_inference.reranking.rerank import rerank_search_results
    from marqo_amd.s2_inference.s2_inference import _create_model_cache_key, get_available_models
    name, query = dirs["tinybert"], RR.sentences(5, seed=1)
    hits = [{"_id": f"doc{i}", "title": RR.sentences(7 + 4 * i, seed=400 + i), "body": RR.sentences(23 - 3 * i, seed=500 + i), "_score": 0.5 + 0.01 * i}
            for i in range(6)]
    result = {"hits": copy.deepcopy(hits), "limit": 6}
    rerank_search_results(result, query, name, DEV)
    key = _create_model_cache_key(name, DEV)
    assert key in get_available_models()
    model = get_available_models()[key]["model"]
    # the chunks in the order the reranker scores them: field by field, hit by hit
    rows = [(h["_id"], f, ch) for f in ("title", "body") for h in hits for ch in split_text(h[f], split_length=2, split_overlap=0, split_by="sentence")]
    logits, scores = model.tower.score(query, [r[2] for r in rows], 512)
    assert np.allclose(scores, 1.0 / (1.0 + np.exp(-logits.astype(np.float64))), rtol=0, atol=1e-6)
    got = {h["_id"]: h for h in result["hits"]}
    assert len(got) == 6 and len(result["hits"]) == 6
    for h in hits:
        mine = [k for k, r in enumerate(rows) if r[0] == h["_id"]]
        win = max(mine, key=lambda k: scores[k])
        out = got[h["_id"]]
        assert np.float32(out["_score"]).view(np.int32) == scores[win].view(np.int32) and out["_score"] == float(scores[win])
        assert out["_highlights"] == [{rows[win][1]: rows[win][2]}]
        assert not any(k in out for k in ("_rerank_id", "_reranked_score", "_reranked_highlights"))
    order = [h["_score"] for h in result["hits"]]
    assert order == sorted(order, reverse=True) and len(set(order)) == 6
    # a second call finds the model in the cache: nothing is loaded
    monkeypatch.setattr(CrossEncoderTower, "from_dir", classmethod(lambda cls, *a, **k: (_ for _ in ()).throw(AssertionError("loaded twice"))))
    again = {"hits": copy.deepcopy(hits)}
    rerank_search_results(again, query, name, DEV)
    assert get_available_models()[key]["model"] is model
    assert [(h["_id"], h["_score"]) for h in again["hits"]] == [(h["_id"], h["_score"]) for h in result["hits"]]
    del get_available_models()[key]
    assert cross_encoders.load_cross_encoder_model is not None

"""XLM-RoBERTa cross-encoders on the GPU (csrc/rerank.hip mq_pair_plan_n / mq_pack_pairs_xlmr / mq_score_pairs_xlmr, engine/rerank.py): the packed
pairs against the pair oracle of tests/rerank_xlmr_ref.py, the final <s> rows and the logits against transformers' own
XLMRobertaForSequenceClassification in fp32, the public call, and the BERT path bit for bit through the old entry points.  On the parent of this
feature the load itself raises ("... is not served as a cross-encoder (only 'bert')"), so every test that needs the tower fails there."""
import copy
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rerank_ref as RR  # noqa: E402
import rerank_xlmr_ref as XR  # noqa: E402
from marqo_amd import _lib as L  # noqa: E402
from marqo_amd.engine.rerank import BERT, XLMR, CrossEncoderTower, pair_lengths  # noqa: E402
from tests import test_rerank_gpu as BERT_GPU  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = -7777

# The bound tests/test_rerank_gpu.py uses for the BERT head on its tiny checkpoint (twice its measured 1.317e-01): both are bf16-operand,
# fp32-accumulate towers of width 128 and 2 layers under the same weight recipe.
# Measured here on the MI355X on the first run: worst |logit - fp32 logit| = 5.82e-02 over the 8 pairs, inside that bound, which stays.
LOGIT_TOL = BERT_GPU.LOGIT_TOL["tinybert"]
# 1 - cos of a final <s> row against the fp32 model: the project's tolerance for a bf16 tower against its fp32 reference
# (tests/test_towers_gpu.py COS_TOL).  MUTATION NOTE: with the position table read from row 0 instead of row 2 (offset 0), the same three rows
# give 1 - cos = 2.32e-01 / 2.30e-01 / 2.09e-01 on this checkpoint (measured once on the fp32 model with the table shifted by two rows), so the
# bound lies two orders of magnitude below what the fault produces.
ROW_COS_TOL = 1e-3
PAIRS_SEED = 95          # chosen on the CPU: of the seven adjacent gaps of the oracle's sorted logits, one is below 2 * LOGIT_TOL


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)


def _guarded_i32(n, pad=8):
    return torch.full((n + 2 * pad,), GUARD, dtype=torch.int32, device=DEV), pad


def _guards_intact(buf, pad, n):
    return bool((buf[:pad] == GUARD).all()) and bool((buf[pad + n:] == GUARD).all())


@pytest.fixture(scope="module")
def ckpt(tmp_path_factory):
    """the checkpoint directory (with a stray roberta.pooler.*), the fp32 model, the host tokeniser, one-piece words, the pair oracle"""
    from marqo_amd.engine.tokenizers import XlmRobertaTokenizer
    d = str(tmp_path_factory.mktemp("xlmr_ce"))
    XR.write_dir(d, seed=0, stray_pooler=True)
    tok = XlmRobertaTokenizer(d)
    oracle = XR.pair_oracle(d, tok)
    print(f"pair oracle: {XR.PAIR_ORACLE}")
    return dict(dir=d, model=XR.load_model(d), tok=tok, words=XR.one_piece_words(tok), oracle=oracle)


@pytest.fixture(scope="module")
def tower(ckpt):
    t = CrossEncoderTower.from_dir(ckpt["dir"], DEV)      # on the parent commit: ValueError "... (only 'bert')"
    assert t.family is XLMR and t.arch.pos_offset == 2 and t.arch.type_vocab == 1
    assert t.model_max_length == XR.USABLE == 64, "model_max_length 512 of tokenizer_config.json is capped by the usable positions"
    return t


# ---- pack ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_length", [5, 16, 64])
def test_pack_pairs_xlmr_equals_the_pair_oracle(ckpt, max_length):
    """n = 5 documents of 0, 1, cut, cut + 1 and >= ld - 2 pieces (a full row), where cut = B - la when the query leaves room (la < B) and the
    document's share B - B // 2 of a pair cut on both sides otherwise; Lq = 1 and 20"""
    from marqo_amd.engine.gpu_tokenizers import DeviceSentencePieceTokenizer
    lib = L.load()
    tok, words, oracle = ckpt["tok"], ckpt["words"], ckpt["oracle"]
    dtok = DeviceSentencePieceTokenizer(tok, DEV)
    B, n = max_length - 4, 5
    for la in (1, 20):
        cut = B - la if la < B else B - B // 2
        lbs = (0, 1, cut, cut + 1, 200)
        query = XR.text_of(words, la, seed=200 + la)
        docs = [XR.text_of(words, lb, seed=300 + 7 * i + la) for i, lb in enumerate(lbs)]
        d_q, qlen = dtok.encode_device([query], 4 * len(query) + 4)
        assert int(qlen[0]) - 2 == la
        ld = max_length if la <= max_length - 2 else la + 2
        d_docs, dlen = dtok.encode_device(docs, ld)
        dlen = dlen.numpy()
        assert dlen.tolist() == [min(lb, ld - 2) + 2 for lb in lbs] and int(dlen[-1]) == ld, "the last row is full"
        a, b = pair_lengths(la, dlen - 2, max_length, 4)
        (ka, p), (kb, _), (kt, _) = _guarded_i32(n), _guarded_i32(n), _guarded_i32(n)
        d_docs, d_dlen = d_docs.contiguous(), _i32(dlen)
        L.check(lib.mq_pair_plan_n(la, d_dlen.data_ptr(), n, ld, max_length, 4, ka[p:].data_ptr(), kb[p:].data_ptr(), kt[p:].data_ptr(), _stream()),
                "mq_pair_plan_n")
        total = kt[p:p + n].cpu().numpy()
        cu = np.zeros(n + 1, dtype=np.int32)
        np.cumsum(total, out=cu[1:])
        rows = int(cu[-1])
        want = oracle(query, docs, max_length)
        assert cu.tolist() == np.concatenate(([0], np.cumsum([len(w) for w in want]))).tolist(), (la, max_length)
        assert ka[p:p + n].cpu().tolist() == a.tolist() and kb[p:p + n].cpu().tolist() == b.tolist() and total.tolist() == (a + b + 4).tolist()
        # the output ends `rows` words into a buffer whose tail is a guard: the kernel is told the true `rows`, and also one row less
        for told in (rows, rows - 1):
            ids, q = _guarded_i32(rows)
            d_query, d_cu = d_q[0, 1:1 + la].contiguous(), _i32(cu)
            L.check(lib.mq_pack_pairs_xlmr(d_query.data_ptr(), la, d_docs.data_ptr(), ld, ka[p:].data_ptr(), kb[p:].data_ptr(), d_cu.data_ptr(), n,
                                           tok.cls_id, tok.sep_id, ids[q:].data_ptr(), told, _stream()), "mq_pack_pairs_xlmr")
            torch.cuda.synchronize(DEV)
            flat = [t for w in want for t in w]
            assert ids[q:q + told].cpu().tolist() == flat[:told], (la, max_length, told)
            assert _guards_intact(ids, q, told), "a word at or beyond `rows` changed"
        for buf in (ka, kb, kt):
            assert _guards_intact(buf, p, n), "a guard word changed"
    # an empty query: <s> </s> </s> d </s>
    d_docs, dlen = dtok.encode_device([XR.text_of(words, 3, seed=1), ""], max_length)
    dlen = dlen.numpy()
    a, b = pair_lengths(0, dlen - 2, max_length, 4)
    cu = np.concatenate(([0], np.cumsum(a + b + 4))).astype(np.int32)
    ids, q = _guarded_i32(int(cu[-1]))
    d_docs, d_a, d_b, d_cu = d_docs.contiguous(), _i32(a), _i32(b), _i32(cu)
    L.check(lib.mq_pack_pairs_xlmr(None, 0, d_docs.data_ptr(), max_length, d_a.data_ptr(), d_b.data_ptr(), d_cu.data_ptr(), 2, tok.cls_id, tok.sep_id,
                                   ids[q:].data_ptr(), int(cu[-1]), _stream()), "mq_pack_pairs_xlmr")
    torch.cuda.synchronize(DEV)
    want = oracle("", [XR.text_of(words, 3, seed=1), ""], max_length)
    assert ids[q:q + int(cu[-1])].cpu().tolist() == [t for w in want for t in w] and want[1] == [0, 2, 2, 2]
    assert _guards_intact(ids, q, int(cu[-1]))


# ---- positions ------------------------------------------------------------------------------------------------------------------------------------
def _score_packed(t, seqs, typed_ids=None):
    n = len(seqs)
    cu_np = np.concatenate(([0], np.cumsum([len(s) for s in seqs]))).astype(np.int32)
    rows = int(cu_np[-1])
    ids, d_cu, cu = _i32(np.concatenate(seqs)), _i32(cu_np), torch.from_numpy(cu_np)
    out = torch.full((2, n + 2), float("nan"), dtype=torch.float32, device=DEV)
    cls_rows = torch.full((n + 1, t.arch.width), float("nan"), dtype=torch.float32, device=DEV)
    with torch.cuda.device(DEV):
        ws = torch.empty(t.lib.mq_score_pairs_workspace_bytes(C.byref(t.cfg), rows, n) + 256, dtype=torch.uint8, device=DEV)
        t.score_packed(ids, typed_ids, d_cu, cu, out[0, 1:], out[1, 1:], cls_rows, ws)
        torch.cuda.synchronize(DEV)
    assert bool(cls_rows[n].isnan().all()) and bool(out[:, 0].isnan().all()) and bool(out[:, -1].isnan().all()), "a guard word changed"
    return out[0, 1:1 + n].cpu().numpy(), cls_rows[:n].cpu().numpy()


def test_position_ids_run_from_the_offset_over_the_whole_pair(ckpt, tower):
    """the final <s> rows of pairs of 5, 63 and 64 tokens (64: the last usable position, table row 65) against the fp32 model, whose position
    ids are create_position_ids_from_input_ids' 2, 3, ... over the whole unpadded pair"""
    g = np.random.default_rng(7)
    V = ckpt["tok"].vocab_size
    seqs = []
    for total in (5, 63, 64):
        a = (total - 4) // 3
        p = g.integers(4, V - 1, total - 4).tolist()
        seqs.append([XR.CLS, *p[:a], XR.SEP, XR.SEP, *p[a:], XR.SEP])
    assert [len(s) for s in seqs] == [5, 63, 64]
    _, want = XR.hf_forward(ckpt["model"], seqs)
    _, got = _score_packed(tower, seqs)
    cos = (got * want).sum(-1) / (np.linalg.norm(got, axis=-1) * np.linalg.norm(want, axis=-1))
    print("final <s> rows, 1 - cos against the fp32 model at totals 5 / 63 / 64: " + " ".join(f"{1 - c:.3e}" for c in cos))
    assert float((1 - cos).max()) <= ROW_COS_TOL
    with pytest.raises(L.MarqoHipError, match="sequence lengths must be in"):          # a 65th token has no position row
        _score_packed(tower, [seqs[2] + [XR.SEP]])
    with pytest.raises(ValueError, match="no token-type ids"):
        _score_packed(tower, seqs, typed_ids=_i32(np.zeros(132)))


# ---- logits ---------------------------------------------------------------------------------------------------------------------------------------
def _pairs(words):
    query = XR.sentences(words, 6, 1000 + PAIRS_SEED)
    docs = [XR.sentences(words, k, 2000 + 10 * PAIRS_SEED + i) for i, k in enumerate((3, 9, 14, 22, 37, 55, 70, 120))]
    docs[2] = "  " + docs[2] + " \n"                   # stripped, as CrossEncoder strips
    return query, docs


def test_logits_match_transformers(ckpt, tower):
    query, docs = _pairs(ckpt["words"])
    seqs = ckpt["oracle"](query.strip(), [d.strip() for d in docs], 64)
    lens = [len(s) for s in seqs]
    assert min(lens) < 20 and lens.count(64) >= 3, lens                   # mixed lengths, some truncated
    ref, _ = XR.hf_forward(ckpt["model"], seqs)
    logits, scores = tower.score(query, docs, 512)                        # (512 is lowered to the model's 64)
    assert logits.dtype == np.float32 and logits.shape == (8,) and scores.shape == (8,)
    err = float(np.abs(logits - ref).max())
    print(f"xlm-r cross-encoder: worst |logit - fp32 transformers| = {err:.4e} (bound {LOGIT_TOL:.4e}); std of the reference logits = "
          f"{float(ref.std()):.3f}; residual stream {tower.residual_stream}; pair oracle: {XR.PAIR_ORACLE}")
    assert np.allclose(scores, 1.0 / (1.0 + np.exp(-logits.astype(np.float64))), rtol=0, atol=1e-6)
    assert err <= LOGIT_TOL
    order = np.argsort(ref)
    gaps = np.diff(ref[order])
    left_out = int((gaps <= 2 * LOGIT_TOL).sum())
    assert left_out <= 1, f"{left_out} of the seven adjacent gaps of the oracle are below twice the bound: choose another PAIRS_SEED"
    for k in np.nonzero(gaps > 2 * LOGIT_TOL)[0]:
        assert logits[order[k]] < logits[order[k + 1]], (k, ref[order], logits[order])
    # the same pairs one at a time and in another order: the same scores to within the bound (batch composition changes summation order)
    single = np.asarray([tower.score(query, [d], 64)[0][0] for d in docs[::-1]])[::-1]
    assert float(np.abs(single - ref).max()) <= LOGIT_TOL
    assert tower.score(query, [], 64)[0].shape == (0,)
    with pytest.raises(ValueError, match="at least 5"):
        tower.score(query, docs, 4)
    # empty texts: the pair keeps its four specials
    e_ref, _ = XR.hf_forward(ckpt["model"], ckpt["oracle"]("", ["", docs[1].strip()], 64) + ckpt["oracle"](query, ["  "], 64))
    e_got = np.concatenate((tower.score("", ["", docs[1]], 64)[0], tower.score(query, ["  "], 64)[0]))
    print(f"empty query / document: worst |logit - fp32| = {float(np.abs(e_got - e_ref).max()):.4e}")
    assert float(np.abs(e_got - e_ref).max()) <= LOGIT_TOL


# ---- the public call ----------------------------------------------------------------------------------------------------------------------------------
def test_rerank_search_results_with_an_xlmr_directory(ckpt):
    """the order of the hits, `_score` and `_highlights` as they follow from the ORACLE's scores through split_text and the best-chunk-per-hit
    rule (the plumbing tests/test_rerank_gpu.py's end-to-end test computes with): a chunk or a hit may change places only where the oracle's
    logits are closer than twice the bound, and the canned result (chosen on the CPU) has no such place"""
    from marqo_amd.s2_inference.processing.text import split_text
    from marqo_amd.s2_inference.reranking.rerank import rerank_search_results
    from marqo_amd.s2_inference.s2_inference import _create_model_cache_key, get_available_models
    words, name = ckpt["words"], ckpt["dir"]
    query, hits = XR.canned_search(words)
    result = {"hits": copy.deepcopy(hits), "limit": len(hits)}
    rerank_search_results(result, query, name, DEV)
    key = _create_model_cache_key(name, DEV)
    assert key in get_available_models()
    try:
        rows = [(h["_id"], f, ch) for f in ("title", "body") for h in hits for ch in split_text(h[f], split_length=2, split_overlap=0, split_by="sentence")]
        z, _ = XR.hf_forward(ckpt["model"], ckpt["oracle"](query, [r[2].strip() for r in rows], 64))
        s = 1.0 / (1.0 + np.exp(-z))
        best = {}
        for h in hits:
            mine = sorted((k for k, r in enumerate(rows) if r[0] == h["_id"]), key=lambda k: -z[k])
            assert len(mine) >= 3 and z[mine[0]] - z[mine[1]] > 2 * LOGIT_TOL, "the canned result must be decisive within every hit"
            best[h["_id"]] = mine[0]
        want_order = sorted(best, key=lambda i: -z[best[i]])
        tops = np.asarray([z[best[i]] for i in want_order])
        assert float(-np.diff(tops).max()) > 2 * LOGIT_TOL, "the canned result must be decisive between the hits"
        assert [h["_id"] for h in result["hits"]] == want_order
        worst = 0.0
        for h in result["hits"]:
            k = best[h["_id"]]
            assert h["_highlights"] == [{rows[k][1]: rows[k][2]}]
            worst = max(worst, abs(h["_score"] - s[k]))
            assert not any(f in h for f in ("_rerank_id", "_reranked_score", "_reranked_highlights"))
        print(f"rerank_search_results: worst |_score - sigmoid(fp32 logit)| = {worst:.4e} (bound {LOGIT_TOL / 4:.4e})")
        assert worst <= LOGIT_TOL / 4                    # sigmoid' <= 1 / 4
    finally:
        del get_available_models()[key]


# ---- unchanged behaviour: BERT ----------------------------------------------------------------------------------------------------------------------------
def test_bert_logits_are_the_old_entry_points_bits(tmp_path):
    """a BERT cross-encoder through score() (mq_pair_plan_n with three specials, the shared scoring function) and through the entry points as they
    were (mq_pair_plan, mq_pack_pairs, mq_score_pairs_bert) on the same batch: the same bits.  With equal type rows, mq_score_pairs_xlmr (no
    type ids) gives those bits as well: one function serves both."""
    RR.write_cross_encoder_dir(str(tmp_path), "tinybert", seed=0, equal_type_rows=True)
    t = CrossEncoderTower.from_dir(str(tmp_path), DEV)
    assert t.family is BERT
    lib, tok = t.lib, t.tokenizer
    query = RR.sentences(6, seed=9)
    docs = [RR.sentences(4 + 5 * i, seed=50 + i) for i in range(16)]
    new_logits, new_scores = t.score(query, docs, 64)
    with torch.cuda.device(DEV):
        d_q, qlen = t.device_tokenizer.encode_device([query], len(query) + 2)
        la = int(qlen[0]) - 2
        d_docs, dlen = t.device_tokenizer.encode_device(docs, 64)
        dlen = dlen.numpy()
        a, b = pair_lengths(la, dlen - 2, 64)
        total = a + b + 3
        order = np.argsort(-total, kind="stable")
        n = len(docs)
        cu_np = np.concatenate(([0], np.cumsum(total[order]))).astype(np.int32)
        rows = int(cu_np[-1])
        d_docs = d_docs.index_select(0, torch.from_numpy(order).to(DEV)).contiguous()
        d_dlen, d_cu, cu = _i32(dlen[order]), _i32(cu_np), torch.from_numpy(cu_np)
        plan = torch.empty(3, n, dtype=torch.int32, device=DEV)
        ids = torch.empty(2, rows, dtype=torch.int32, device=DEV)
        d_query = d_q[0, 1:1 + la].contiguous()
        L.check(lib.mq_pair_plan(la, d_dlen.data_ptr(), n, 64, 64, plan[0].data_ptr(), plan[1].data_ptr(), plan[2].data_ptr(), _stream()), "mq_pair_plan")
        L.check(lib.mq_pack_pairs(d_query.data_ptr(), la, d_docs.data_ptr(), 64, plan[0].data_ptr(), plan[1].data_ptr(), d_cu.data_ptr(), n, tok.cls_id,
                                  tok.sep_id, ids[0].data_ptr(), ids[1].data_ptr(), rows, _stream()), "mq_pack_pairs")
        out = torch.full((4, n), float("nan"), dtype=torch.float32, device=DEV)
        ws = torch.empty(lib.mq_score_pairs_workspace_bytes(C.byref(t.cfg), rows, n) + 256, dtype=torch.uint8, device=DEV)
        L.check(lib.mq_score_pairs_bert(C.byref(t.cfg), C.byref(t.w), C.byref(t.head), ids[0].data_ptr(), ids[1].data_ptr(), d_cu.data_ptr(),
                                        cu.data_ptr(), n, out[0].data_ptr(), out[1].data_ptr(), None, ws.data_ptr(), ws.numel(), _stream()),
                "mq_score_pairs_bert")
        L.check(lib.mq_score_pairs_xlmr(C.byref(t.cfg), C.byref(t.w), C.byref(t.head), ids[0].data_ptr(), d_cu.data_ptr(), cu.data_ptr(), n,
                                        out[2].data_ptr(), out[3].data_ptr(), None, ws.data_ptr(), ws.numel(), _stream()), "mq_score_pairs_xlmr")
        torch.cuda.synchronize(DEV)
    assert plan[2].cpu().tolist() == total[order].tolist()
    old = out.cpu().numpy()
    inv = np.empty(n, dtype=np.int64)
    inv[order] = np.arange(n)
    assert np.isfinite(old).all()
    assert np.array_equal(old[0][inv].view(np.int32), new_logits.view(np.int32)), "score() left the bits of the old entry points"
    assert np.array_equal(old[1][inv].view(np.int32), new_scores.view(np.int32))
    assert np.array_equal(old[2].view(np.int32), old[0].view(np.int32)) and np.array_equal(old[3].view(np.int32), old[1].view(np.int32))

"""Text reranking without a GPU: the truncation rule against the fast tokenizer, the result plumbing against the reference's own code, the
float32 models of the typed embedding and of the head against the budgets of tests/rerank_ref.py (and that each seeded fault leaves them),
name handling, and the library's argument checks."""
import copy
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rerank_ref as RR  # noqa: E402
import rerank_ref_cases as CASES  # noqa: E402
from marqo_amd import _lib as L  # noqa: E402
from marqo_amd.engine.rerank import pair_lengths  # noqa: E402
from marqo_amd.s2_inference.errors import RerankerError  # noqa: E402
from marqo_amd.s2_inference.reranking import cross_encoders, rerank  # noqa: E402
from oracle import ref_shim  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- truncation rule ---------------------------------------------------------------------------------------------------------------------
def test_pair_lengths_is_the_fast_tokenizers_longest_first(tmp_path):
    """la, lb in 0 .. 13, max_length in {4, 5, 8, 9, 16, 17}: lengths and token_type_ids of BertTokenizerFast's batch pair calls"""
    RR.write_vocab(tmp_path)
    tok = RR.fast_tokenizer(tmp_path)
    rng = range(14)
    a_texts = [RR.words(la, seed=la) for la in rng for _ in rng]
    b_texts = [RR.words(lb, seed=100 + lb) for _ in rng for lb in rng]
    bad = []
    for max_length in (4, 5, 8, 9, 16, 17):
        enc = tok(a_texts, b_texts, truncation="longest_first", max_length=max_length)
        k = 0
        for la in rng:
            for lb in rng:
                a, b = pair_lengths(la, lb, max_length)
                if len(enc["input_ids"][k]) != a + b + 3 or enc["token_type_ids"][k] != [0] * (a + 2) + [1] * (b + 1):
                    bad.append((max_length, la, lb, a, b, enc["token_type_ids"][k]))
                k += 1
    assert not bad, bad[:5]
    va, vb = pair_lengths(np.arange(14)[:, None], np.arange(14)[None, :], 9)   # the array form is the scalar form
    assert all((int(va[i, j]), int(vb[i, j])) == pair_lengths(i, j, 9) for i in rng for j in rng)
    with pytest.raises(ValueError):
        pair_lengths(3, 3, 3)


# ---- plumbing against the reference's own code -------------------------------------------------------------------------------------------------
class _Scorer:
    def predict(self, pairs):
        return np.asarray([CASES.crc_score(q, c) for q, c in pairs], dtype=np.float64)


def _ours(case):
    result = copy.deepcopy(case["search_result"])
    try:
        ret = rerank.rerank_search_results(result, case["query"], "injected", "cpu", **case["kwargs"])
        return {"result": result, "returned_input": ret is result}
    except Exception as e:  # noqa: BLE001
        return {"raises": type(e).__name__}


def _blank_fresh_ids(result, case):
    """a hit without `_id` gets a fresh uuid as `_rerank_id`: its value is not compared"""
    with_id = {h["_id"] for h in case["search_result"]["hits"] if "_id" in h}
    for h in result["hits"]:
        if "_rerank_id" in h and h["_rerank_id"] not in with_id:
            h["_rerank_id"] = "<uuid>"
    return result


@pytest.fixture(scope="module")
def reference_side(tmp_path_factory):
    if not ref_shim.available():
        pytest.skip("the reference tree is not present on this machine")
    p = tmp_path_factory.mktemp("rerank") / "cases.json"
    p.write_text(json.dumps(CASES.cases()))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), MARQO_AMD_HOST_ERRORS="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "rerank_ref_plumbing.py"), str(p)], capture_output=True, text=True, env=env,
                       timeout=300)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert r.returncode == 0 and lines, r.stderr[-3000:]
    return json.loads(lines[-1])


def test_plumbing_matches_the_reference(reference_side, monkeypatch):
    monkeypatch.setattr(cross_encoders, "load_cross_encoder_model", lambda model_name, device, max_length=512: {"model": _Scorer()})
    cases = CASES.cases()
    assert set(reference_side) == set(cases)
    for name, case in cases.items():
        ref, got = reference_side[name], _ours(case)
        if "raises" in ref:
            assert got == {"raises": "RerankerError"} and ref["raises"] == "RerankerError", (name, ref, got)
            continue
        assert "result" in got, (name, got)
        got = json.loads(json.dumps(got, default=float))
        assert _blank_fresh_ids(got["result"], case) == _blank_fresh_ids(ref["result"], case), name
        assert got["returned_input"] == ref["returned_input"], name
    # what the cases are there for
    assert reference_side["attributes_no_hit_has"]["returned_input"] and reference_side["attributes_no_hit_has"]["result"] == cases["attributes_no_hit_has"]["search_result"]
    assert reference_side["two_highlights_one_row"] == {"raises": "RerankerError"}
    assert isinstance(reference_side["two_highlights"]["result"]["hits"][0]["_score"], list)
    assert "_rerank_id" in reference_side["keep_original"]["result"]["hits"][0] and "_rerank_id" not in reference_side["all_fields"]["result"]["hits"][0]


def test_plumbing_known_answers(monkeypatch):
    """the same code without the reference tree: best chunk per hit, descending order, working keys removed"""
    monkeypatch.setattr(cross_encoders, "load_cross_encoder_model", lambda model_name, device, max_length=512: {"model": _Scorer()})
    case = CASES.cases()["all_fields"]
    r = copy.deepcopy(case["search_result"])
    assert rerank.rerank_search_results(r, case["query"], "injected", "cpu") is None
    from marqo_amd.s2_inference.processing.text import split_text
    for hit in r["hits"]:
        rows = [(CASES.crc_score(case["query"], ch), f, ch) for f in ("title", "body") for ch in split_text(hit[f], split_length=2, split_overlap=0)]
        s, f, ch = max(rows)
        assert hit["_score"] == s and hit["_highlights"] == [{f: ch}]
        assert not any(k in hit for k in ("_rerank_id", "_reranked_score", "_reranked_highlights"))
    assert [h["_score"] for h in r["hits"]] == sorted((h["_score"] for h in r["hits"]), reverse=True)
    one = CASES.cases()["two_highlights_one_row"]
    with pytest.raises(RerankerError):
        rerank.rerank_search_results(copy.deepcopy(one["search_result"]), one["query"], "injected", "cpu", **one["kwargs"])
    assert rerank._check_searchable_fields_in_results({"hits": [{"a": 1}]}, ["b"]) is False
    assert rerank._check_searchable_fields_in_results({"hits": [{"a": 1}]}, None) is True
    assert cross_encoders.get_default_text_processing_parameters() == {"split_length": 2, "split_overlap": 0, "split_method": "sentence"}


# ---- names ---------------------------------------------------------------------------------------------------------------------------------
def test_names_that_are_not_served_and_the_testing_model():
    r = {"hits": [{"_id": "a", "t": "One. Two. Three."}, {"_id": "b", "t": "Four."}]}
    with pytest.raises(RerankerError, match="image reranker is not served"):
        rerank.rerank_search_results(copy.deepcopy(r), "q", "owl/ViT-B/32", "cpu", searchable_attributes=["t"])
    with pytest.raises(RerankerError, match="'onnx/' prefix is not served"):
        rerank.rerank_search_results(copy.deepcopy(r), "q", "onnx/cross-encoder/ms-marco-MiniLM-L-6-v2", "cpu")
    with pytest.raises(RerankerError, match="no local checkpoint.*cross-encoder/not-on-this-disk"):
        rerank.rerank_search_results(copy.deepcopy(r), "q", "cross-encoder/not-on-this-disk", "cuda")
    model = cross_encoders.load_cross_encoder_model("_testing", "cpu")["model"]
    s = model.predict([["q", "a"], ["q", "b"], ["q", "c"]])
    assert len(s) == 3 and all(isinstance(float(v), float) and 0 <= v < 1 for v in s)
    from marqo_amd.s2_inference.s2_inference import _create_model_cache_key, get_available_models
    assert _create_model_cache_key("_testing", "cpu") in get_available_models()
    out = copy.deepcopy(r)
    rerank.rerank_search_results(out, "q", "_testing", "cpu")
    assert all(0 <= h["_score"] < 1 and list(h["_highlights"][0]) == ["t"] for h in out["hits"])


def test_product_reranking_does_not_import_pandas():
    code = "import sys; import marqo_amd.s2_inference.reranking.rerank, marqo_amd.engine.rerank; sys.exit(1 if 'pandas' in sys.modules else 0)"
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    assert subprocess.run([sys.executable, "-c", code], env=env, timeout=300).returncode == 0


# ---- float32 models against the budgets; seeded faults ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [128, 384, 1024])
def test_embed_model_is_inside_the_budget_and_faults_are_not(W):
    c = RR.embed_case(W, [1, 3, 64, 65], seed=1)
    y, B = RR.embed_reference(c)
    assert RR.ratio(RR.model_embed(c), y, B) <= 1.0
    for fault in RR.FAULTS_EMBED:       # named input: mixed type ids, two distinct type rows
        assert RR.ratio(RR.model_embed(c, fault), y, B) > 1.25, fault
    z = RR.embed_case(W, [1, 3, 64, 65], seed=1, mixed=False)
    assert np.array_equal(RR.model_embed(z), RR.model_embed(z, "type_row_zero"))   # all-zero type ids: the fault is the function


@pytest.mark.parametrize("W", [128, 384, 1024])
def test_head_model_is_inside_the_budget_and_faults_are_not(W):
    c = RR.head_case(W, 65, seed=2)
    z, Bz, s, Bs = RR.head_reference(c)
    mz, ms = RR.model_head(c)
    assert RR.ratio(mz, z, Bz) <= 1.0 and RR.ratio(ms, s, Bs) <= 1.0
    for fault in RR.FAULTS_HEAD:        # named input: unrelated rows, classifier bias 0.37
        fz, _ = RR.model_head(c, fault)
        assert RR.ratio(fz, z, Bz) > 1.25, fault


def test_synthetic_cross_encoder_logits_spread():
    """the builder's scales: reference logits over unrelated pairs have a standard deviation of at least 1 (fp32 transformers on the CPU)"""
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        RR.write_cross_encoder_dir(d, "tinybert", seed=0)
        docs = [RR.sentences(4 + 3 * i, seed=50 + i) for i in range(24)]
        z = RR.hf_logits(d, RR.sentences(6, seed=9), docs, 64)
    assert z.std() >= 1.0, z.std()


# ---- the library's argument checks (no launch) ------------------------------------------------------------------------------------------------
def test_argument_errors_are_reported_without_a_gpu():
    lib = L.load()
    fake = 256

    def refused(rc, msg):
        assert rc == -1 and msg in lib.mq_last_error(), (rc, lib.mq_last_error())

    refused(lib.mq_pair_plan(3, fake, 1, 16, 3, fake, fake, fake, None), b"max_length=3 must be >= 4")
    refused(lib.mq_pair_plan(3, fake, 1, 1, 16, fake, fake, fake, None), b"mq_pair_plan: bad shape")
    refused(lib.mq_pack_pairs(fake, 3, None, 16, fake, fake, fake, 1, 2, 3, fake, fake, 10, None), b"mq_pack_pairs: null pointer")
    refused(lib.mq_embed_tokens_typed(fake, fake, fake, 1, fake, None, fake, 2, None, None, fake, None, 770, 100, 1e-12, 0, None),
            b"embed_tokens_typed: W=770 unsupported")
    refused(lib.mq_embed_tokens_typed(fake, fake, fake, 1, fake, None, fake, 0, None, None, fake, None, 768, 100, 1e-12, 0, None), b"type_vocab=0")
    head = L.ScoreHeadWeights(pooler_w=fake, pooler_b=fake, cls_w=fake, cls_b=0.0, type_vocab=2)
    refused(lib.mq_score_head(fake, 1, 100, C.byref(head), fake, None, fake, 1 << 20, None), b"mq_score_head: W=100")
    assert lib.mq_score_head(fake, 1, 128, C.byref(head), fake, None, fake, 16, None) == -3 and b"workspace" in lib.mq_last_error()
    assert lib.mq_score_head_workspace_bytes(5, 128) >= 5 * 128 * 6 and lib.mq_score_head_workspace_bytes(0, 128) == 0
    cfg = L.BertCfg(enc=L.EncoderCfg(width=128, layers=2, heads=2, mlp_dim=512, act=1, post_ln=1, mask=0, ln_eps=1e-12), vocab=100, max_pos=512, pool=1)
    w = L.BertWeights(word_emb=fake, pos_emb=fake, type_emb=fake, emb_ln_g=fake, emb_ln_b=fake)
    n = lib.mq_score_pairs_workspace_bytes(C.byref(cfg), 100, 3)
    assert n > lib.mq_bert_workspace_bytes(C.byref(cfg), 100, 3)
    cfg.enc.precision = L.MQ_PREC_FP8
    refused(lib.mq_score_pairs_bert(C.byref(cfg), C.byref(w), C.byref(head), fake, fake, fake, fake, 1, fake, None, None, fake, n, None),
            b"bf16 encoders only")
    assert C.sizeof(L.ScoreHeadWeights) == 32

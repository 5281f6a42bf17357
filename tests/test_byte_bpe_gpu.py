"""GPT-2 / RoBERTa byte-level BPE on the GPU (csrc/tokenize.hip mq_tokenize_byte_bpe, engine/gpu_tokenizers.py DeviceByteBpeTokenizer) and what it
opens: `hf` RoBERTa embedding models and RoBERTa cross-encoders, each against transformers' own fp32
model over the ids of the host tokeniser of record.  On the parent of this feature there is no device tokeniser and the loaders refuse or crash."""
import copy

import numpy as np
import pytest
import torch

from tests import byte_bpe_ref as BR
from tests import rerank_xlmr_ref as XR
from tests import test_rerank_xlmr_gpu as XLMR_GPU
from tests import test_towers_gpu as TOWERS_GPU
from marqo_amd.engine.tokenizers import RobertaBpeTokenizer

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# 1 - cos of a mean-pooled, normalised embedding against the fp32 model: the bound tests/test_towers_gpu.py::test_golden_xlm_roberta_small holds
# the same encoder (XLM-R's: position ids from padding_idx + 1) to in bf16
EMB_COS_TOL = TOWERS_GPU.COS_TIGHT
# |logit - fp32 logit|: the bound tests/test_rerank_xlmr_gpu.py holds the XLM-R cross-encoder of the same sizes and weight recipe to
LOGIT_TOL = XLMR_GPU.LOGIT_TOL


@pytest.fixture(scope="module")
def tok_dir(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("byte_bpe"))
    BR.write_tokenizer_files(d)
    return d


@pytest.fixture(scope="module")
def tok(tok_dir):
    return RobertaBpeTokenizer(tok_dir)


@pytest.fixture(scope="module")
def dtok(tok):
    from marqo_amd.engine.gpu_tokenizers import DeviceByteBpeTokenizer
    return DeviceByteBpeTokenizer(tok, DEV)


def _expected(tok, texts, max_length):
    rows = [tok.encode(t, max_length) for t in texts]
    ids = np.full((len(texts), max_length), tok.pad_id, dtype=np.int32)
    for i, r in enumerate(rows):
        ids[i, :len(r)] = r
    return ids, np.asarray([len(r) for r in rows], dtype=np.int64)


# ---- device against host --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_length", [512, 8])
def test_device_equals_host(tok, dtok, max_length):
    """fixed cases + 2 000 fuzz texts, with a special-token text and a 129-byte pre-token mixed in: both routes patch one matrix"""
    texts = BR.FIXED_CASES + ["a <s> b </s>", BR.LONG_HOST, "fill the <mask> in"] + BR.fuzz_texts(77, 2000) + [BR.LONG_HOST + " again", "fox dog " * 300, "<pad> last"]
    want_ids, want_lens = _expected(tok, texts, max_length)
    ids, lens = dtok.encode_device(texts, max_length)
    assert ids.dtype == torch.int32 and ids.shape == (len(texts), max_length) and ids.device.type == "cuda" and lens.dtype == torch.int64
    got = ids.cpu().numpy()
    bad = np.nonzero((got != want_ids).any(axis=1) | (lens.numpy() != want_lens))[0]
    assert bad.size == 0, [(texts[i], got[i, :12].tolist(), want_ids[i, :12].tolist()) for i in bad[:3]]
    assert (want_lens == max_length).any() and (want_lens == 2).any() and (want_lens < max_length).any()


def test_small_batches_and_the_drop_in_call(tok, dtok):
    ids, lens = dtok.encode_device([], 16)
    assert ids.shape == (0, 16) and lens.shape == (0,)
    for text in ("I'll search the index", "", BR.LONG_HOST, "a </s> b"):
        ids, lens = dtok.encode_device([text], 16)
        want_ids, want_lens = _expected(tok, [text], 16)
        assert np.array_equal(ids.cpu().numpy(), want_ids) and lens.tolist() == want_lens.tolist(), text
    batch = ["the quick brown fox", "a  b", "", "x " * 40]
    for ml in (None, 12):
        got, want = dtok(batch, max_length=ml), tok(batch, max_length=ml)
        assert np.array_equal(got["input_ids"], want["input_ids"]) and np.array_equal(got["attention_mask"], want["attention_mask"])
    with pytest.raises(Exception, match="max_length"):
        dtok.encode_device(["a"], 1)


# ---- hf embedding model -------------------------------------------------------------------------------------------------------------------------------
def test_hf_roberta_embeddings(tmp_path, monkeypatch):
    from marqo_amd.s2_inference import s2_inference as s2i
    d = str(tmp_path / "roberta_enc")
    model = BR.write_encoder_dir(d, seed=0)
    tok = RobertaBpeTokenizer(d)
    monkeypatch.setenv("MARQO_MAX_CUDA_MODEL_MEMORY", "64")
    props = {"type": "hf", "name": d, "dimensions": 128, "tokens": 32}
    texts = [BR.text_of(k, seed=10 + k) for k in (1, 3, 8, 20, 30, 45)] + ["I'll rank 1000 documents, won't I?", "naïve café über straße", "a  b \n c"]
    rows = [tok.encode(t, 32) for t in texts]
    assert any(len(r) == 32 for r in rows) and any(len(r) < 10 for r in rows)
    ref = BR.mean_pooled(model, rows)
    try:
        s2i.clear_loaded_models()
        out = np.asarray(s2i.vectorise("roberta-bpe-test", texts, model_properties=props, device=DEV), dtype=np.float64)
        loaded = next(iter(s2i._available_models.values()))[s2i.AvailableModelsKey.model]
        from marqo_amd.engine.gpu_tokenizers import DeviceByteBpeTokenizer
        assert isinstance(loaded._device_tokenizer, DeviceByteBpeTokenizer) and isinstance(loaded._tokenizer, RobertaBpeTokenizer)
        one = np.asarray(s2i.vectorise("roberta-bpe-test", texts[3], model_properties=props, device=DEV), dtype=np.float64)
    finally:
        s2i.clear_loaded_models()
    assert out.shape == (len(texts), 128)
    err = 1 - (out * ref).sum(-1) / np.linalg.norm(out, axis=-1)
    print("hf roberta: 1 - cos against the fp32 model: " + " ".join(f"{e:.2e}" for e in err) + f" (bound {EMB_COS_TOL:.1e})")
    np.testing.assert_allclose(np.linalg.norm(out, axis=-1), 1.0, atol=1e-5)
    assert float(err.max()) < EMB_COS_TOL
    assert float(1 - (one[0] * ref[3]).sum() / np.linalg.norm(one[0])) < EMB_COS_TOL      # the single-query route tokenises on the host


# ---- reranker -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ce(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("roberta_ce"))
    model = BR.write_cross_encoder_dir(d, seed=0)
    return dict(dir=d, model=model, tok=RobertaBpeTokenizer(d), hf=BR.hf_tokenizer(d))


@pytest.fixture(scope="module")
def tower(ce):
    from marqo_amd.engine.gpu_tokenizers import DeviceByteBpeTokenizer
    from marqo_amd.engine.rerank import XLMR, CrossEncoderTower
    t = CrossEncoderTower.from_dir(ce["dir"], DEV)
    assert t.family is XLMR and isinstance(t.device_tokenizer, DeviceByteBpeTokenizer) and t.model_max_length == XR.USABLE
    return t


def _docs(tok, la, max_length):
    """12 documents (prefixes of one text) whose piece counts straddle the cut at B - la (B = max_length - 4): one empty, one of one piece,
    cut - 2 .. cut + 2, B and B + 1 (longer than the whole budget), and two that fill any row"""
    B = max_length - 4
    cut = B - la
    assert cut >= 3, "the query leaves room for the document"
    base = BR.text_of(80, seed=500 + max_length)
    by_count = {}
    for c in range(len(base) + 1):
        t = base[:c].strip()
        by_count.setdefault(len(tok.encode(t)) - 2, t)
    wanted = [0, 1, cut - 2, cut - 1, cut, cut + 1, cut + 2, B, B + 1, 2 * max_length, 3 * max_length]
    have = np.asarray(sorted(by_count))
    counts = sorted({int(have[np.abs(have - n).argmin()]) for n in wanted})        # (a prefix one character longer can have FEWER pieces: nearest)
    assert 0 in counts and any(cut - 2 <= n < cut for n in counts) and any(cut < n <= cut + 2 for n in counts), (cut, counts)
    assert any(n > B for n in counts) and any(n >= 2 * max_length for n in counts), (B, counts)
    return [by_count[n] for n in counts] + [base]


@pytest.mark.parametrize("max_length", [16, 64])
def test_cross_encoder_pairs_and_logits(ce, tower, max_length):
    """the packed ids exactly against RobertaTokenizer's pair call, the logits against the fp32 model on those pairs"""
    import ctypes as C
    from marqo_amd import _lib as L
    from marqo_amd.engine.rerank import pair_lengths
    tok, hf = ce["tok"], ce["hf"]
    query = "lazy fox?"
    la = len(tok.encode(query)) - 2
    docs = _docs(tok, la, max_length)
    assert 9 <= len(docs) <= 12 and "" in docs
    want = hf([query] * len(docs), docs, truncation="longest_first", max_length=max_length)["input_ids"]
    host_pairs = []
    q = tok.encode(query)[1:-1]
    for d in docs:
        p = tok.encode(d)[1:-1]
        a, b = pair_lengths(len(q), len(p), max_length, 4)
        host_pairs.append([tok.cls_id, *q[:a], tok.sep_id, tok.sep_id, *p[:b], tok.sep_id])
    assert host_pairs == want, "the pairs the host tokeniser of record packs are transformers' pairs"
    assert min(len(w) for w in want) < max_length and sum(len(w) == max_length for w in want) >= 2
    # the packed ids of the device route (tokenise -> plan -> pack), exactly
    lib = tower.lib
    stream = torch.cuda.current_stream(DEV).cuda_stream
    with torch.cuda.device(DEV):
        d_q, qlen = tower._tokenize_query(query)
        assert int(qlen[0]) - 2 == la and d_q.shape[1] == len(query.encode()) + 2
        ld = max_length if la <= max_length - 2 else la + 2
        d_docs, dlen = tower._tokenize(docs, ld)
        n = len(docs)
        d_dlen = torch.from_numpy(dlen.astype(np.int32)).to(DEV)
        plan = torch.empty(3, n, dtype=torch.int32, device=DEV)
        L.check(lib.mq_pair_plan_n(la, d_dlen.data_ptr(), n, ld, max_length, 4, plan[0].data_ptr(), plan[1].data_ptr(), plan[2].data_ptr(), stream),
                "mq_pair_plan_n")
        total = plan[2].cpu().numpy()
        cu = np.concatenate(([0], np.cumsum(total))).astype(np.int32)
        rows = int(cu[-1])
        d_cu = torch.from_numpy(cu).to(DEV)
        packed = torch.full((rows + 8,), -7777, dtype=torch.int32, device=DEV)
        d_query = d_q[0, 1:1 + la].contiguous()
        L.check(lib.mq_pack_pairs_xlmr(d_query.data_ptr(), la, d_docs.data_ptr(), ld, plan[0].data_ptr(), plan[1].data_ptr(), d_cu.data_ptr(), n,
                                       tok.cls_id, tok.sep_id, packed.data_ptr(), rows, stream), "mq_pack_pairs_xlmr")
        torch.cuda.synchronize(DEV)
    assert packed[:rows].cpu().tolist() == [t for w in want for t in w] and bool((packed[rows:] == -7777).all())
    # the logits
    ref, _ = XR.hf_forward(ce["model"], want)
    logits, scores = tower.score(query, docs, max_length)
    err = float(np.abs(logits - ref).max())
    print(f"roberta cross-encoder at max_length {max_length}: worst |logit - fp32 transformers| = {err:.4e} (bound {LOGIT_TOL:.4e}); std of the "
          f"reference logits = {float(ref.std()):.3f}")
    assert logits.dtype == np.float32 and logits.shape == (len(docs),)
    assert np.allclose(scores, 1.0 / (1.0 + np.exp(-logits.astype(np.float64))), rtol=0, atol=1e-6)
    assert err <= LOGIT_TOL


def test_rerank_search_results_with_a_roberta_directory(ce):
    from marqo_amd.s2_inference.processing.text import split_text
    from marqo_amd.s2_inference.reranking.rerank import rerank_search_results
    from marqo_amd.s2_inference.s2_inference import _create_model_cache_key, get_available_models
    tok, hf, name = ce["tok"], ce["hf"], ce["dir"]
    query = "silver river in winter"
    hits = [{"_id": f"doc{i}", "title": BR.text_of(4 + i, seed=900 + i).capitalize() + ".",
             "body": " ".join(BR.text_of(5, seed=950 + 10 * i + j).capitalize() + "." for j in range(4)), "_score": 0.5} for i in range(3)]
    result = {"hits": copy.deepcopy(hits), "limit": len(hits)}
    rerank_search_results(result, query, name, DEV)
    key = _create_model_cache_key(name, DEV)
    try:
        rows = [(h["_id"], f, ch) for f in ("title", "body") for h in hits for ch in split_text(h[f], split_length=2, split_overlap=0, split_by="sentence")]
        pairs = hf([query] * len(rows), [r[2].strip() for r in rows], truncation="longest_first", max_length=XR.USABLE)["input_ids"]
        z, _ = XR.hf_forward(ce["model"], pairs)
        s = 1.0 / (1.0 + np.exp(-z))
        assert sorted(h["_id"] for h in result["hits"]) == sorted(h["_id"] for h in hits)
        worst = 0.0
        for h in result["hits"]:
            (field, chunk), = h["_highlights"][0].items()
            k = next(i for i, r in enumerate(rows) if r == (h["_id"], field, chunk))
            worst = max(worst, abs(h["_score"] - s[k]))
            best = max(z[i] for i, r in enumerate(rows) if r[0] == h["_id"])
            assert z[k] >= best - 2 * LOGIT_TOL, "the highlight is the hit's best chunk, to within the bound"
        print(f"rerank_search_results (roberta): worst |_score - sigmoid(fp32 logit)| = {worst:.4e} (bound {LOGIT_TOL / 4:.4e})")
        assert worst <= LOGIT_TOL / 4                    # sigmoid' <= 1 / 4
    finally:
        get_available_models().pop(key, None)


# ---- open_clip/roberta-ViT-B-32 -------------------------------------------------------------------------------------------------------------------------
def test_rows_of_the_open_clip_hf_tokenizer(tok, dtok):
    """the roberta-base text tower's loader keeps the host tokeniser (tests/test_s2_inference_gpu.py pins that); what it would get from the device is
    the same rows: cleaned on the host first, <s> ids </s> padded with <pad> to the context length"""
    from marqo_amd.engine.tokenizers import _clean_text
    from marqo_amd.s2_inference.open_clip_model import HfClipTokenizer
    host = HfClipTokenizer(tok, 77)
    texts = BR.FIXED_CASES[:24] + [BR.text_of(k, seed=k) for k in (2, 9, 40, 120)] + ["a &amp; b  <s> c", BR.LONG_HOST]
    ids, lens = dtok.encode_device([_clean_text(t) for t in texts], 77)
    want = host(texts)
    assert np.array_equal(ids.cpu().numpy(), want) and lens.tolist() == (want != host.pad_id).sum(1).tolist()

"""The DeBERTa tower and reranker on the GPU: mq_score_pairs_deberta / mq_encode_deberta through engine/rerank.py::DebertaCrossEncoderTower against the
float64 passes of tests/deberta_ref.py (`exact`, which tests/test_deberta_host.py pins to transformers' own float64 model, and `model`, the same pass
rounded where the tower stores bf16 / fp32), and `rerank_search_results` against fp32 transformers.

Bars:
  every stream row after the first and after the last block, the pooled [CLS] rows and the logits, for every tiny and both batches of packed pairs:
  max(|got - exact| / |model - exact|) <= MARGIN = 4.0 (imported as tests/test_jina_bert_gpu.py imports it) — per row in the 2- and the inf-norm for the
  rows (packed_text_ref.row_ratio), over the batch for the logits (deberta_ref.scalar_ratio).  The yardstick is the float64 model's own distance from
  `exact`; it is never derived from the kernel's output.
  End to end: |logit - fp32 transformers' logit| <= LOGIT_TOL["cls"] = 0.0397 of tests/test_rerank_modernbert_gpu.py (imported, not copied), and the
  order of the hits equals the reference's.

The stream is read from the first slice of the workspace (off_x is the plan's first take); the workspace is exactly
mq_score_pairs_deberta_workspace_bytes long in front of a sentinel tail, the outputs sit between guard words.

One 700-token sequence goes through the tower (two pieces through the attention kernel's 512-key LDS image, far past the clamp of the buckets).

Measured on an MI355X (DEBERTA_WORST / DEBERTA_E2E lines), worst ratio, stream after block 1 / 2, pooled 1 / 2, logit 1 / 2 (bar 4.0):
    S4_SHARE 1.44 / 1.78, 1.15 / 1.30, 1.07 / 1.53    S4_SPLIT 1.45 / 1.98, 1.01 / 1.15, 1.00 / 0.82    S8_SHARE 1.67 / 2.35, 1.04 / 1.31, 1.06 / 1.06
    S8_SPLIT 1.49 / 1.74, 1.01 / 1.12, 1.61 / 1.87    W192_3H 1.39 / 1.92, 1.03 / 1.10, 1.08 / 1.49;  the 700-token sequence: stream 1.90, pooled 1.17.
  End to end: worst |logit - fp32 transformers| 7.74e-3, with the pairs cut at 24 tokens 4.68e-3 (bar 0.0397: the tinies stay inside the imported bar);
  worst |score - sigmoid(reference logit)| 1.8e-3; reference logits -0.446 .. 0.498, neighbours more than 0.119 apart.
"""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from marqo_amd import _lib as L
from tests import attention_ref as A
from tests import deberta_ref as D
from tests import rerank_modernbert_ref as RM
from tests.test_patch_attn_gpu import MARGIN
from tests.test_rerank_modernbert_gpu import LOGIT_TOL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _s():
    return torch.cuda.current_stream().cuda_stream


def _tower(name):
    from marqo_amd.engine.rerank import DebertaCrossEncoderTower
    b = D.build(name)
    return b, DebertaCrossEncoderTower(b["arch"], b["sd"], DEV, tokenizer=None, model_max_length=D.MAX_LEN)


def _score(lib, tower, cfg, ids, lens, short=0):
    """one guarded mq_score_pairs_deberta call -> (rc, stream x [rows, W], pooled [nseq, W], logits [nseq], scores [nseq])"""
    rows, nseq, W = sum(lens), len(lens), cfg.width
    d_ids = ids.to(torch.int32).to(DEV).contiguous()
    cu_h = A.cu_seqlens(lens)
    d_cu = cu_h.to(DEV)
    need = lib.mq_score_pairs_deberta_workspace_bytes(C.byref(cfg), rows, nseq)
    ws = torch.full((need + 4096,), 0xA5, dtype=torch.uint8, device=DEV)
    out = torch.full((2, nseq + 2), float("nan"), dtype=torch.float32, device=DEV)
    pooled = torch.full((nseq + 1, W), float("nan"), dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    rc = lib.mq_score_pairs_deberta(C.byref(cfg), C.byref(tower.w), C.byref(tower.head), d_ids.data_ptr(), d_cu.data_ptr(), cu_h.data_ptr(), nseq,
                                    out[0, 1:].data_ptr(), out[1, 1:].data_ptr(), pooled.data_ptr(), ws.data_ptr(), need - short, _s())
    torch.cuda.synchronize()
    assert bool((ws[need:] == 0xA5).all()), "the workspace was written past mq_score_pairs_deberta_workspace_bytes"
    assert bool(out[:, 0].isnan().all()) and bool(out[:, -1].isnan().all()) and bool(pooled[nseq].isnan().all()), "a guard word changed"
    if rc != 0:
        return rc, ws[:need], pooled, out, None
    x = ws[:rows * W * 4].view(torch.float32).view(rows, W)
    assert bool(torch.isfinite(x).all())
    assert torch.equal(x[d_cu[:-1].long()].view(torch.int32), pooled[:nseq].view(torch.int32)), "the pooled rows are not the [CLS] rows of the stream"
    return rc, x, pooled[:nseq], out[0, 1:1 + nseq], out[1, 1:1 + nseq]


@pytest.mark.parametrize("name", tuple(D.TINIES))
def test_stream_pooled_rows_and_logits_against_float64(name):
    lib = L.load()
    b, tower = _tower(name)
    arch = b["arch"]
    worst = {}
    for bi, seqs in enumerate(b["batches"]):
        lens, ids = [len(s) for s in seqs], torch.cat(seqs)
        for layers in (1, arch.layers):
            ex = D.exact(arch, b["tensors"], ids.to(DEV), lens, layers)
            mo = D.model(arch, b["tensors"], ids.to(DEV), lens, layers)
            cfg = type(tower.cfg).from_buffer_copy(tower.cfg)
            cfg.layers = layers
            rc, x, pooled, logits, scores = _score(lib, tower, cfg, ids, lens)
            L.check(rc, "mq_score_pairs_deberta")
            rs = D.row_ratio(x, ex.final, mo.final)
            rp = D.row_ratio(pooled, ex.pooled, mo.pooled)
            rl = D.scalar_ratio(logits, ex.logits, mo.logits)
            assert torch.allclose(scores.double(), torch.sigmoid(logits.double()), rtol=0, atol=1e-6)
            print(f"DEBERTA_RATIO {name} batch={bi} layers={layers} stream={rs['ratio']:.3f} (row {rs['row']} col {rs['col']}) pooled={rp['ratio']:.3f} "
                  f"logit={rl:.3f} (|model - exact| logits {float((mo.logits - ex.logits).abs().max()):.2e})")
            worst[f"stream{layers}"] = max(worst.get(f"stream{layers}", 0.0), rs["ratio"])
            worst[f"pooled{layers}"] = max(worst.get(f"pooled{layers}", 0.0), rp["ratio"])
            worst[f"logit{layers}"] = max(worst.get(f"logit{layers}", 0.0), rl)
    print(f"DEBERTA_WORST {name}: " + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= MARGIN, worst


def test_a_700_token_sequence_goes_through_the_tower():
    lib = L.load()
    b, tower = _tower("S8_SHARE")
    arch, lens = b["arch"], [700]
    assert lens[0] > D.LDS_KEYS
    ids = D.random_seqs(lens, arch.vocab, seed=11)[0]
    ex = D.exact(arch, b["tensors"], ids.to(DEV), lens)
    mo = D.model(arch, b["tensors"], ids.to(DEV), lens)
    rc, x, pooled, logits, _ = _score(lib, tower, tower.cfg, ids, lens)
    L.check(rc, "mq_score_pairs_deberta")
    rs = D.row_ratio(x, ex.final, mo.final)
    rp = D.row_ratio(pooled, ex.pooled, mo.pooled)
    print(f"DEBERTA_RATIO S8_SHARE lens=[700] stream={rs['ratio']:.3f} (row {rs['row']} col {rs['col']}) pooled={rp['ratio']:.3f} "
          f"logit err {float((logits.double().cpu() - ex.logits.cpu()).abs().max()):.2e} (model {float((mo.logits - ex.logits).abs().max()):.2e})")
    assert max(rs["ratio"], rp["ratio"]) <= MARGIN


def test_a_workspace_one_byte_short_is_refused_and_nothing_is_written():
    lib = L.load()
    b, tower = _tower("S8_SHARE")
    seqs = b["batches"][1]
    rc, ws, pooled, out, _ = _score(lib, tower, tower.cfg, torch.cat(seqs), [len(s) for s in seqs], short=1)
    assert rc == -3 and b"mq_score_pairs_deberta: workspace" in lib.mq_last_error(), f"a workspace one byte short: rc {rc}, not MQ_ERR_WORKSPACE"
    assert bool((ws == 0xA5).all()) and bool(out.isnan().all()) and bool(pooled.isnan().all())
    # and the encoder's own entry point
    lens = [len(s) for s in seqs]
    rows, nseq = sum(lens), len(lens)
    need = lib.mq_deberta_workspace_bytes(C.byref(tower.cfg), rows, nseq)
    arch = b["arch"]
    assert need >= rows * arch.width * (4 + 2 + 2) + rows * 3 * arch.width * 2
    ws = torch.full((need,), 0xA5, dtype=torch.uint8, device=DEV)
    o = torch.full((nseq, arch.width), float("nan"), dtype=torch.float32, device=DEV)
    cu_h = A.cu_seqlens(lens)
    d_cu, d_ids = cu_h.to(DEV), torch.cat(seqs).to(torch.int32).to(DEV)
    rc = lib.mq_encode_deberta(C.byref(tower.cfg), C.byref(tower.w), d_ids.data_ptr(), d_cu.data_ptr(), cu_h.data_ptr(), nseq, o.data_ptr(), 0, ws.data_ptr(),
                               need - 1, _s())
    torch.cuda.synchronize()
    assert rc == -3 and b"mq_encode_deberta: workspace" in lib.mq_last_error()
    assert bool((ws == 0xA5).all()) and bool(o.isnan().all())


# ---- end to end -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ckpt(tmp_path_factory):
    d = tmp_path_factory.mktemp("deberta") / "reranker"
    cfg, model = D.write_dir(d, "S8_SHARE", seed=4)
    return dict(dir=str(d), cfg=cfg, model=model)


def test_rerank_search_results_on_the_engine(ckpt):
    """six hits reranked through the public call, and the same pairs cut at max_length 24 through the tower: logits against fp32 transformers on the pairs the
    fast tokenizer forms"""
    from marqo_amd.engine.rerank import DebertaCrossEncoderTower
    from marqo_amd.s2_inference.reranking.rerank import rerank_search_results
    from marqo_amd.s2_inference.s2_inference import _create_model_cache_key, get_available_models
    name, query = ckpt["dir"], RM.sentence(5, 1)
    tol = LOGIT_TOL["cls"]
    # one sentence per field (one chunk per hit).  Six of forty candidates, chosen by the REFERENCE's logits alone so that neighbours lie more than three
    # bars apart: the same query in front of every document leaves a tiny random model's logits close together, and an order nobody can tell apart
    # within the bar would test nothing
    cand = [RM.sentence(2 + 3 * i, 400 + i) for i in range(40)]
    zc = RM.hf_logits(ckpt["model"], RM.pair_encodings(name, query, cand, 512))
    pick = []
    for i in np.argsort(zc):
        if not pick or zc[i] - zc[pick[-1]] > 3 * tol:
            pick.append(int(i))
    assert len(pick) >= 6, f"the fixture's logits are closer than the tolerance can tell apart: {np.sort(zc)}"
    pick = sorted(pick[:6])                                              # (in the candidates' order, not sorted by logit)
    texts, z = [cand[i] for i in pick], zc[pick]
    hits = [{"_id": f"doc{i}", "body": texts[i], "_score": 0.5 + 0.01 * i} for i in range(6)]
    result = {"hits": copy.deepcopy(hits), "limit": 6}
    rerank_search_results(result, query, name, DEV)
    key = _create_model_cache_key(name, DEV)
    model = get_available_models()[key]["model"]
    try:
        assert isinstance(model.tower, DebertaCrossEncoderTower)
        got = {h["_id"]: h["_score"] for h in result["hits"]}
        err_s = max(abs(got[f"doc{i}"] - 1.0 / (1.0 + np.exp(-z[i]))) for i in range(6))
        logits, scores = model.tower.score(query, texts, 512)
        err = float(np.abs(logits - z).max())
        enc = RM.pair_encodings(name, query, texts, 24)
        full = RM.pair_encodings(name, query, texts, 512)
        assert all(len(e) == 24 for e in enc) and min(len(e) for e in full) > 24 and len({len(e) for e in full}) > 1      # every pair is cut
        z_cut = RM.hf_logits(ckpt["model"], enc)
        cut, _ = model.tower.score(query, texts, 24)
        err_cut = float(np.abs(cut - z_cut).max())
        print(f"DEBERTA_E2E worst |logit - fp32 transformers| = {err:.4e} (cut at 24 tokens: {err_cut:.4e}); worst |score - sigmoid| = {err_s:.3e}; "
              f"reference logits {np.round(np.sort(z), 3)}; bar {tol:.4f}")
        assert err <= tol and err_cut <= tol
        assert err_s <= tol / 4 + 1e-6       # (sigmoid' <= 1 / 4)
        assert np.diff(np.sort(z)).min() > 2 * tol, f"the fixture's logits are closer than the tolerance can tell apart: {np.sort(z)}"
        assert [h["_id"] for h in result["hits"]] == [f"doc{i}" for i in np.argsort(-z)], "the reranked order is not the order of the transformers logits"
        for h in result["hits"]:
            assert h["_highlights"] == [{"body": texts[int(h["_id"][3:])]}]
    finally:
        del get_available_models()[key]

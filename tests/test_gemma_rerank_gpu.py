"""The Gemma reranker on the GPU: mq_attention_gqa256_causal / mq_attention_gqa256_prefix (csrc/attention_gqa256_causal.hip) against float64,
GemmaRerankerTower (mq_score_gemma_pairs through engine/rerank.py) against transformers' own float64 GemmaForCausalLM / GemmaForSequenceClassification
(tests/gemma_rerank_ref.py), and `rerank_search_results` from a local checkpoint directory.

Bars:
  kernel: |kernel - float64| <= 1.25 x budget, budget = 2**-8 (P|V| + |out|): the bar and margin of tests/test_attention_gpu.py (imported, as
      tests/test_attention_gqa256_gpu.py imports them); references tests/gemma_rerank_ref.py::prefix_reference (equal to qwen_ref.gqa_reference on
      [prefix | segment] to 1e-12 on the host) and qwen_ref.gqa_reference (causal).  prefix_len = 0 equals mq_attention_gqa256_causal bit for bit; the
      torch op equals the C entry point bit for bit; grouped against expanded K/V within twice the budget (test_cross_checks_on_expanded_kv's form).
  one wrong key: on tests/gemma_rerank_ref.py::loud_key_inputs the kernel is within the bar of the true reference and outside the bar of a reference that
      admits the first future key or drops the last prefix key for one query (tests/test_gemma_rerank_host.py shows the two are that far apart).
  tower: err(shared) <= 1.5 x err(unshared), both max |logit - float64 transformers| over 24 documents of 1 .. 200 tokens (DOC_LENS) — the assertion and
      bar of tests/test_qwen_rerank_gpu.py::test_shared_run_against_float64_transformers; ranking and the end-to-end run use that file's forms too.

Measured values are printed as `GEMMARR_*` lines.  Measured on an MI355X: kernel worst ratio 0.9957 over every case (bar 1.25); grouped against expanded
K/V 0.0000 - the same bits - (bar 2.5); against the other scale's reference 539 or more; one wrong key: true reference 0.79 / 0.83, future key admitted
256, last prefix key dropped 4.0e4 / 3.8e4 (P = 65 / 130).  Tower, max |logit - float64| unshared / shared over 24 documents (bar 1.5 x unshared):
TINY81 lm 1.88e-4 / 1.98e-4, TINY21 lm 2.74e-4 / 3.45e-4, TINY21 cls 2.20e-4 / 2.27e-4 (over the first four documents alone TINY81 gave 8.1e-5 / 1.28e-4:
see DOC_LENS); one document per batch differs from one batch by at most 5.8e-5.  Ranking: error 3.0e-4, 24 of 24 documents more than twice that apart,
same order.  End to end (gain-1.5 models): unshared logit error over 40 candidates 3.4e-2 (lm) / 2.2e-2 (cls); scores within 4.6e-3 / 1.0e-3 (bars
1.3e-2 / 8.3e-3); another prompt 2.0e-2 / 3.8e-2 (bars 3.1e-2 / 7.7e-2)."""
import copy
import math

import numpy as np
import pytest
import torch

from marqo_amd import _lib as L
from marqo_amd.engine import archs
from tests import attention_ref as R
from tests import gemma_ref as G
from tests import gemma_rerank_ref as GR
from tests import qwen_ref as Q
from tests.test_attention_gpu import MARGIN

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 64
HD = GR.HD
SCALE = HD ** -0.5
HEADS = [(8, 1), (3, 1), (2, 2), (16, 2)]
PACKED = [1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 300]     # around the 16-query block, the 64-key tile, the 128-key piece (crossed twice by 300)
PREFIXES = (1, 63, 64, 65, 130)
SEGMENTS = [1, 17, 64, 65, 200]
FILL = 0x5A5A


@pytest.fixture(scope="module")
def lib():
    return L.load()


def _s():
    return torch.cuda.current_stream().cuda_stream


def _cu(P, lens):
    return torch.tensor([P] + [P + int(c) for c in np.cumsum(lens)], dtype=torch.int32, device="cuda")


def _guarded(rows, W):
    raw = torch.full(((rows + 2 * GUARD) * W,), FILL, dtype=torch.int16, device="cuda")
    return raw, raw[GUARD * W:(GUARD + rows) * W].view(torch.bfloat16).view(rows, W)


def _check_guards(raw, rows, W, P=0):
    n = GUARD * W
    assert bool((raw[:n] == FILL).all()) and bool((raw[n + rows * W:] == FILL).all()), "a guard row was written"
    assert bool((raw[n:n + P * W] == FILL).all()), "a prefix row of out was written"


def _run_prefix(lib, qkv, P, lens, hs, scale=SCALE):
    Qh, KV = hs
    W, rows = Qh * HD, qkv.shape[0]
    raw, out = _guarded(rows, W)
    L.check(lib.mq_attention_gqa256_prefix(qkv.data_ptr(), out.data_ptr(), _cu(P, lens).data_ptr(), len(lens), P, max(lens), Qh, KV, HD, scale, _s()),
            "mq_attention_gqa256_prefix")
    torch.cuda.synchronize()
    _check_guards(raw, rows, W, P)
    return out


def _run_causal(lib, qkv, lens, hs, fixed=False, scale=SCALE):
    Qh, KV = hs
    W, rows = Qh * HD, qkv.shape[0]
    raw, out = _guarded(rows, W)
    if fixed:
        assert len(set(lens)) == 1
        cu, fl, mx = None, lens[0], 0
    else:
        cu, fl, mx = R.cu_seqlens(lens, "cuda"), 0, max(lens)
    L.check(lib.mq_attention_gqa256_causal(qkv.data_ptr(), out.data_ptr(), L.ptr(cu), len(lens), fl, mx, Qh, KV, HD, scale, _s()), "mq_attention_gqa256_causal")
    torch.cuda.synchronize()
    _check_guards(raw, rows, W)
    return out


def _assert_causal(tag, lib, hs, lens, fixed=False):
    for fam in ("readout", "peaked"):
        qkv = G.make_band_qkv(fam, lens, *hs, seed=sum(lens) + hs[0], device="cuda")
        got = _run_causal(lib, qkv, lens, hs, fixed)
        out, absout = Q.gqa_reference(qkv, lens, *hs, HD, R.MASK_CAUSAL)
        w = R.worst_coords(got, out, absout, lens, hs[0], HD)
        print(f"GEMMARR_RATIO {tag} heads={hs} family={fam} lens={lens} ratio={w['ratio']:.4f}")
        assert w["ratio"] <= MARGIN, (tag, hs, fam, lens, w)


def _assert_prefix(tag, lib, hs, P, lens):
    for fam in ("readout", "peaked"):
        qkv = G.make_band_qkv(fam, [P] + lens, *hs, seed=P + sum(lens) + hs[0], device="cuda")
        got = _run_prefix(lib, qkv, P, lens, hs)
        out, absout = GR.prefix_reference(qkv, P, lens, *hs)
        w = R.worst_coords(got[P:], out[P:], absout[P:], lens, hs[0], HD)
        print(f"GEMMARR_RATIO {tag} heads={hs} P={P} family={fam} lens={lens} ratio={w['ratio']:.4f}")
        assert w["ratio"] <= MARGIN, (tag, hs, P, fam, lens, w)


# ---- the kernel -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hs", HEADS)
def test_packed_causal_batches_within_the_rounding_budget(lib, hs):
    _assert_causal("packed", lib, hs, PACKED)


@pytest.mark.parametrize("hs", ((8, 1), (3, 1)))
def test_fixed_length_entry(lib, hs):
    _assert_causal("fixed", lib, hs, [65] * 3, fixed=True)


@pytest.mark.parametrize("hs", HEADS)
@pytest.mark.parametrize("P", PREFIXES)
def test_prefix_attention_within_the_rounding_budget(lib, hs, P):
    """P = 130 with the 200-token segment streams both the prefix (three tiles) and the segment (four) through the LDS in pieces of two"""
    _assert_prefix("prefix", lib, hs, P, SEGMENTS)


@pytest.mark.parametrize("hs", HEADS)
def test_without_a_prefix_the_bits_of_the_causal_entry(lib, hs):
    for fam in ("readout", "peaked"):
        qkv = G.make_band_qkv(fam, PACKED, *hs, seed=5, device="cuda")
        got = _run_prefix(lib, qkv, 0, PACKED, hs)
        ref = _run_causal(lib, qkv, PACKED, hs)
        assert torch.equal(got.view(torch.int16), ref.view(torch.int16))


def test_torch_op_forwards_to_the_same_kernel(lib):
    hs, P, lens = (8, 1), 65, [17, 70]
    qkv = G.make_band_qkv("peaked", [P] + lens, *hs, seed=9, device="cuda")
    ref = _run_prefix(lib, qkv, P, lens, hs)
    out = torch.zeros_like(ref)
    L.load_torch_ops().mq_attention_gqa256_prefix(qkv, _cu(P, lens), P, max(lens), *hs, HD, SCALE, out)
    torch.cuda.synchronize()
    assert torch.equal(out[P:].view(torch.int16), ref[P:].view(torch.int16)) and not bool(out[:P].any())


def test_the_scale_is_the_argument(lib):
    """two scales, two references, each met by its own run and missed by the other's"""
    hs, P, lens = (8, 1), 65, [129, 1, 33]
    qkv = G.make_band_qkv("readout", [P] + lens, *hs, seed=5, device="cuda")
    refs = {sc: GR.prefix_reference(qkv, P, lens, *hs, scale=sc) for sc in (SCALE, 0.125)}
    for sc in refs:
        got = _run_prefix(lib, qkv, P, lens, hs, scale=sc)
        own = R.worst_ratio(got[P:], refs[sc][0][P:], refs[sc][1][P:])
        other = max(R.worst_ratio(got[P:], o[P:], a[P:]) for s2, (o, a) in refs.items() if s2 != sc)
        print(f"GEMMARR_RATIO scale={sc}: {own:.4f} (against the other scale's reference: {other:.1f})")
        assert own <= MARGIN and other > 10 * MARGIN
    cz = G.make_band_qkv("readout", lens, *hs, seed=6, device="cuda")
    got = _run_causal(lib, cz, lens, hs, scale=0.125)
    assert R.worst_ratio(got, *GR.prefix_reference(cz, 0, lens, *hs, scale=0.125)) <= MARGIN


@pytest.mark.parametrize("hs", ((8, 1), (16, 2)))
def test_cross_checks_on_expanded_kv(lib, hs):
    """K/V copied to every query head of its group on the host (the kernel then runs with G = 1: eight blocks per slice, another item-to-wave map):
    each run within the budget of the same reference, so they agree within twice the budget"""
    Qh, KV = hs
    P, lens = 65, [129, 1, 33, 200]
    for fam in ("readout", "peaked"):
        qkv = G.make_band_qkv(fam, [P] + lens, *hs, seed=77, device="cuda")
        got = _run_prefix(lib, qkv, P, lens, hs)[P:]
        wide = Q.expand_kv(qkv, Qh, KV, HD)
        full = _run_prefix(lib, wide, P, lens, (Qh, Qh))[P:]
        out, absout = GR.prefix_reference(wide, P, lens, Qh, Qh)
        out, absout = out[P:], absout[P:]
        r1, r2 = R.worst_ratio(got, out, absout), R.worst_ratio(full, out, absout)
        worst = R.worst_ratio(got, full.double(), absout + (out.abs() - full.double().abs()))     # |got - full| over the REFERENCE's budget
        print(f"GEMMARR_RATIO cross heads={hs} family={fam}: grouped {r1:.4f} expanded {r2:.4f} grouped-vs-expanded {worst:.4f} (bar {2 * MARGIN})")
        assert r1 <= MARGIN and r2 <= MARGIN and worst <= 2 * MARGIN


@pytest.mark.parametrize("P", (65, 130))
def test_one_wrong_key_is_visible(lib, P):
    hs, lens, seg, t = (8, 1), [20, 70, 20], 1, 37
    qkv = GR.loud_key_inputs(P, lens, *hs, seg, t, seed=P, device="cuda")
    got = _run_prefix(lib, qkv, P, lens, hs)
    out, absout = GR.prefix_reference(qkv, P, lens, *hs)
    r = R.worst_ratio(got[P:], out[P:], absout[P:])
    print(f"GEMMARR_KEY P={P}: against the true reference {r:.4f}")
    assert r <= MARGIN
    for kind in ("future", "drop_prefix"):
        bad, badabs = GR.prefix_reference(qkv, P, lens, *hs, fault=(kind, seg, t))
        miss = R.worst_ratio(got[P:], bad[P:], badabs[P:])
        print(f"GEMMARR_KEY P={P} {kind}: against the faulty reference {miss:.1f} (must exceed {MARGIN})")
        assert miss > MARGIN, kind


def test_bad_arguments_launch_nothing(lib):
    hs, P, lens = (4, 2), 10, [20]
    qkv = G.make_band_qkv("randn", [P] + lens, *hs, seed=1, device="cuda")
    out = torch.full((30, 4 * HD), 7.0, dtype=torch.bfloat16, device="cuda")
    cu = _cu(P, lens)
    pre = lambda P_, mx, Qh, KV, hd, q=qkv.data_ptr(), o=out.data_ptr(): lib.mq_attention_gqa256_prefix(q, o, cu.data_ptr(), 1, P_, mx, Qh, KV, hd, SCALE, _s())
    cau = lambda mx, Qh, KV, hd, q=qkv.data_ptr(), o=out.data_ptr(): lib.mq_attention_gqa256_causal(q, o, cu.data_ptr(), 1, 0, mx, Qh, KV, hd, SCALE, _s())
    for call, what in ((lambda: pre(P, 20, 4, 2, 128), b"head_dim 128 unsupported"), (lambda: pre(P, 20, 6, 4, 256), b"q_heads 6 must be a multiple of kv_heads 4"),
                       (lambda: pre(-1, 20, 4, 2, 256), b"prefix_len -1"), (lambda: pre(8000, 193, 4, 2, 256), b"exceeds 8192"),
                       (lambda: pre(P, 8193, 4, 2, 256), b"8193"), (lambda: pre(P, 20, 4, 2, 256, q=None), b"null pointer"),
                       (lambda: pre(P, 20, 4, 2, 256, o=None), b"null pointer"), (lambda: cau(20, 4, 2, 128), b"head_dim 128 unsupported"),
                       (lambda: cau(20, 6, 4, 256), b"q_heads 6 must be a multiple of kv_heads 4"), (lambda: cau(8193, 4, 2, 256), b"8193"),
                       (lambda: cau(20, 4, 2, 256, q=None), b"null pointer")):
        rc = call()
        assert rc == -1 and what in lib.mq_last_error(), (rc, what, lib.mq_last_error())
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


# ---- the tower ------------------------------------------------------------------------------------------------------------------------------------------
# The bar compares two maxima of rounding noise (the two runs round the same quantities in the same places; only the softmax accumulation order differs).
# The maximum over FOUR documents is a poor statistic for that: with these models both errors are about 1e-4 on logits of about 1, and the larger of four
# draws of the same noise lies a factor 1.5 above another such draw every few tries.  So the lengths 1, 17, 70, 200 of the Qwen test are kept and twenty
# more documents (5, 14, ..., 176 tokens) are scored with them: both maxima then sit in the same tail.  The bar stays 1.5.
DOC_LENS = [1, 17, 70, 200] + [5 + 9 * i for i in range(20)]
P_TOWER = 37        # (37 + 200 <= 512 positions of the tiny configs; not a multiple of 64)


@pytest.fixture(scope="module")
def towers():
    from marqo_amd.engine.rerank import GemmaRerankerTower
    tk = G.train_tokenizer()
    yes = tk.encode("Yes", add_special_tokens=False).ids[0]
    out = {}
    for i, (name, kind) in enumerate((("TINY81", "lm"), ("TINY21", "lm"), ("TINY21", "cls"))):
        cfg = GR.TINIES[name]
        model = GR.hf_reranker(cfg, kind, seed=7 + i)
        arch = archs.gemma_causal_arch_from_hf_config(cfg)
        sd = {k: v.float() for k, v in model.state_dict().items()}
        tower = GemmaRerankerTower(arch, sd, DEV, tk, GR.score_row(model, kind, yes, torch.float32), bos_id=2)
        shared = Q.random_seqs([P_TOWER], cfg["vocab_size"], seed=20 + i)[0]
        segs = Q.random_seqs(DOC_LENS, cfg["vocab_size"], seed=30 + i)
        ref = GR.hf_pair_logits(model, kind, [torch.cat([shared, s]) for s in segs], yes).numpy()
        out[(name, kind)] = dict(cfg=cfg, model=model, tower=tower, shared=shared, segs=segs, ref=ref, yes=yes, kind=kind)
    return out


def _np(t):
    return t.numpy().astype(np.int32)


@pytest.mark.parametrize("key", (("TINY81", "lm"), ("TINY21", "lm"), ("TINY21", "cls")))
def test_shared_run_against_float64_transformers(towers, key):
    t = towers[key]
    tower, shared, segs, ref = t["tower"], t["shared"], t["segs"], t["ref"]
    whole = [_np(torch.cat([shared, s])) for s in segs]
    z_un, s_un = tower.score_rows(np.zeros(0, np.int32), whole)
    z_sh, s_sh = tower.score_rows(_np(shared), [_np(s) for s in segs])
    e_un, e_sh = float(np.abs(z_un - ref).max()), float(np.abs(z_sh - ref).max())
    print(f"GEMMARR_TOWER {key}: logits {ref.round(4).tolist()} err unshared={e_un:.3e} shared={e_sh:.3e} (bar 1.5 x unshared = {1.5 * e_un:.3e}) "
          f"per doc unshared={np.abs(z_un - ref).round(5).tolist()} shared={np.abs(z_sh - ref).round(5).tolist()}")
    assert e_sh <= 1.5 * e_un
    assert float(np.abs(ref).max()) > 10 * e_un        # (the logits are not noise: the reference is met, not merely approached from nothing)
    np.testing.assert_allclose(s_sh, 1.0 / (1.0 + np.exp(-z_sh.astype(np.float64))), atol=2e-7)
    # batches of one document each (the prefix is recomputed per batch) and a permuted call give the same bits
    tower.max_rows_per_call, keep = 1, tower.max_rows_per_call
    try:
        z_one, _ = tower.score_rows(_np(shared), [_np(s) for s in segs])
    finally:
        tower.max_rows_per_call = keep
    perm = [2, 0, 3, 1] + list(range(4, len(segs)))
    z_perm, _ = tower.score_rows(_np(shared), [_np(segs[i]) for i in perm])
    assert np.array_equal(z_perm, z_sh[perm])
    print(f"GEMMARR_TOWER {key}: one document per batch differs from one batch by {float(np.abs(z_one - z_sh).max()):.3e}")
    assert float(np.abs(z_one - ref).max()) <= 1.5 * e_un


def test_ranking_follows_the_reference(towers):
    t = towers[("TINY81", "lm")]
    tower, shared = t["tower"], t["shared"]
    cand = Q.random_seqs([5 + 3 * i for i in range(24)], t["cfg"]["vocab_size"], seed=77)
    ref = GR.hf_pair_logits(t["model"], t["kind"], [torch.cat([shared, s]) for s in cand], t["yes"]).numpy()
    got, _ = tower.score_rows(_np(shared), [_np(s) for s in cand])
    err = float(np.abs(got - ref).max())
    pick = []
    for i in np.argsort(ref):
        if not pick or ref[i] - ref[pick[-1]] > 2 * err:
            pick.append(int(i))
    print(f"GEMMARR_RANK measured error {err:.3e}; {len(pick)} of 24 documents lie more than twice that apart")
    assert len(pick) >= 6
    pick = sorted(pick)
    assert np.array_equal(np.argsort(got[pick]), np.argsort(ref[pick]))


# ---- from a checkpoint directory ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("lm", "cls"))
def test_rerank_search_results_on_the_engine(tmp_path, kind):
    """the yardstick of tests/test_qwen_rerank_gpu.py: the error of the unshared run (score_rows with no shared rows) on the SAME pairs against the same
    float64 model, times 1.5; the scores within a quarter of that (the sigmoid's slope is at most 1/4); hits chosen by the REFERENCE's logits more than
    twice the bar apart come back in the reference's order"""
    from marqo_amd.engine.rerank import GEMMA_RERANK_PROMPT, GemmaRerankerTower
    from marqo_amd.s2_inference.reranking.rerank import rerank_search_results
    from marqo_amd.s2_inference.s2_inference import _create_model_cache_key, get_available_models
    from tests import rerank_modernbert_ref as RM
    cfg = Q.config_dict(GR.TINY21, max_position_embeddings=2048)
    model = GR.hf_reranker(cfg, kind, seed=3, gain=1.5)
    tk = G.train_tokenizer()
    yes = tk.encode("Yes", add_special_tokens=False).ids[0]
    name = GR.write_reranker_dir(str(tmp_path / "reranker"), cfg, model, kind, tk, tied=False)
    query = RM.sentence(5, 1)
    direct = GemmaRerankerTower.from_dir(name, DEV)
    cand = [RM.sentence(2 + 3 * i, 400 + i) for i in range(40)]          # one sentence per field: one chunk per hit
    q, whole = GR.plain_rows(tk, 2, query, cand, GEMMA_RERANK_PROMPT, 512)
    seqs = [torch.tensor(w) for w in whole]
    zc = GR.hf_pair_logits(model, kind, seqs, yes).numpy()
    e_un = float(np.abs(direct.score_rows(np.zeros(0, np.int32), [_np(s) for s in seqs])[0] - zc).max())
    pick = []
    for i in np.argsort(zc):
        if not pick or zc[i] - zc[pick[-1]] > 3 * e_un:
            pick.append(int(i))
    assert len(pick) >= 6, f"the fixture's logits are closer than the error {e_un} can tell apart: {np.sort(zc)}"
    pick = sorted(pick[:6])
    texts, z = [cand[i] for i in pick], zc[pick]
    hits = [{"_id": f"doc{i}", "body": texts[i], "_score": 0.5 + 0.01 * i} for i in range(6)]
    result = {"hits": copy.deepcopy(hits), "limit": 6}
    rerank_search_results(result, query, name, DEV)
    key = _create_model_cache_key(name, DEV)
    served = get_available_models()[key]["model"]
    try:
        tower = served.tower
        assert isinstance(tower, GemmaRerankerTower) and tower.last_prefix_len == len(q)
        got = {h["_id"]: h["_score"] for h in result["hits"]}
        err_s = max(abs(got[f"doc{i}"] - 1.0 / (1.0 + math.exp(-z[i]))) for i in range(6))
        print(f"GEMMARR_E2E {kind}: unshared logit error over 40 candidates {e_un:.3e}; max |score - sigmoid(float64 logit)| = {err_s:.3e} "
              f"(bar 1.5 x that / 4 = {1.5 * e_un / 4:.3e}); shared prefix of {tower.last_prefix_len} tokens")
        assert err_s <= 1.5 * e_un / 4
        assert [h["_id"] for h in result["hits"]] == [f"doc{i}" for i in np.argsort(-z)]
        # another prompt is another score, and the reference's
        _, whole_i = GR.plain_rows(tk, 2, query, texts, "answer Yes or No", 512)
        zi = GR.hf_pair_logits(model, kind, [torch.tensor(w) for w in whole_i], yes).numpy()
        lg, _ = tower.score(query, texts, 512, instruction="answer Yes or No")
        bar = 1.5 * float(np.abs(tower.score_rows(np.zeros(0, np.int32), [np.asarray(w, np.int32) for w in whole_i])[0] - zi).max())
        print(f"GEMMARR_E2E {kind} prompt: logit error {float(np.abs(lg - zi).max()):.3e} (bar 1.5 x unshared = {bar:.3e})")
        assert float(np.abs(lg - zi).max()) <= bar and float(np.abs(zi - z).max()) > 3 * e_un
    finally:
        get_available_models().pop(key, None)

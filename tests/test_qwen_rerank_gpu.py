"""The Qwen3 reranker on the GPU: mq_attention_gqa_prefix and mq_qk_norm_rope_at against float64, QwenRerankerTower (mq_score_qwen_pairs through
engine/rerank.py) against transformers' own float64 Qwen3ForCausalLM / Qwen3ForSequenceClassification (tests/qwen_rerank_ref.py, pinned to the project's
float64 reference in tests/test_qwen_rerank_host.py), and `rerank_search_results` from a local checkpoint directory.

Bars:
  mq_attention_gqa_prefix: |kernel - float64| <= 1.25 x budget, budget = 2**-8 (P|V| + |out|): the bar and margin of tests/test_attention_gqa_gpu.py
      (imported), the reference tests/qwen_rerank_ref.py::prefix_reference (equal to qwen_ref.gqa_reference on [prefix | segment] to 1e-12 on the host).
      With prefix_len = 0 the output equals mq_attention_gqa's (MQ_MASK_CAUSAL) bit for bit.
  one wrong key: a dominating key the query may see (the last prefix key, its own key) moves the output by more than 10 (V = 100 there); one it may
      not see (row P of the buffer = the first masked slot of the partial prefix tile and a neighbour's key, the neighbours' last / first keys) leaves the
      segment's output unchanged bit for bit.
  mq_qk_norm_rope_at: the budget of tests/test_qwen_gpu.py with t replaced by offset + t, margin 1.25 (imported); offset 0 equals mq_qk_norm_rope bit for bit.
  tower: err(shared) <= 1.5 x err(unshared), both max |logit - float64 transformers| over the documents of token lengths 1, 17, 70, 200; the unshared
      run (prefix_len = 0) is mq_encode_qwen's tower plus the head.  The shared run rounds the same quantities in the same places; only the order of the
      softmax accumulation over prefix and own tiles differs.
  ranking: documents whose float64 logits lie more than twice the measured error apart rank as the reference ranks them.
  end to end: the same yardstick — logit errors of the engine's shared runs <= 1.5 x the error of the unshared run of the same pairs, the scores within a
      quarter of that (the sigmoid's slope is at most 1/4), hits chosen by the REFERENCE's logits more than twice the bar apart in the reference's order;
      where the engine must take the unshared path (a cap inside the shared part, a leading combining mark) its logits are per-pair scoring's bit for bit.

Measured values are printed as `QWENRR_*` lines.  Measured on an MI355X: mq_attention_gqa_prefix worst ratio 0.9839 over every case (bar 1.25), the case
through two LDS pieces 0.81; a visible dominating key moves the output by 100.2 or more; mq_qk_norm_rope_at 1.00 at every offset, 8000 included.  Tower,
max |logit - float64| unshared / shared (bar 1.5 x unshared): TINY3 lm 4.48e-3 / 3.07e-3, TINY64 lm 4.99e-3 / 4.85e-3, TINY64 cls 3.31e-3 / 3.13e-3;
one document per batch differs from one batch by at most 1.1e-3.  Ranking: error 4.5e-3, 23 of 24 documents more than twice that apart, same order.
End to end (gain-1.5 model): unshared logit error over 40 candidates 4.44e-2; scores within 3.9e-3 (bar 1.67e-2); another instruction 4.91e-2 (bar
5.59e-2); cut at the cap 4.62e-2 (bar 6.38e-2)."""
import copy
import math

import numpy as np
import pytest
import torch

from marqo_amd import _lib as L
from marqo_amd.engine import archs
from tests import attention_ref as R
from tests import qwen_ref as Q
from tests import qwen_rerank_ref as QR
from tests import rowops_ref as RR
from tests.test_attention_gpu import MARGIN
from tests.test_qwen_gpu import MARGIN as ROW_MARGIN, U

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 64
HEADS = [(4, 2, 128), (4, 1, 64), (7, 1, 64), (2, 2, 64), (8, 1, 64)]   # groups of 2, 4, 7 (an idle wave), 1 (no grouping) and 8 (a full round)
PREFIXES = (1, 63, 64, 65, 200)
SEGMENTS = [1, 15, 16, 17, 64, 65, 129]
NAN16 = 0x7FC0      # a bf16 NaN as int16


@pytest.fixture(scope="module")
def lib():
    return L.load()


def _s():
    return torch.cuda.current_stream().cuda_stream


def _cu(P, lens):
    return torch.tensor([P] + [P + int(c) for c in np.cumsum(lens)], dtype=torch.int32, device="cuda")


def _run_prefix(lib, qkv, P, lens, hs):
    """mq_attention_gqa_prefix on an output of NaN rows between NaN guard rows -> the [rows, W] view; the guards and the prefix rows are checked untouched"""
    Qh, KV, hd = hs
    W, rows = Qh * hd, qkv.shape[0]
    raw = torch.full(((rows + 2 * GUARD) * W,), NAN16, dtype=torch.int16, device="cuda")
    out = raw[GUARD * W:(GUARD + rows) * W].view(torch.bfloat16).view(rows, W)
    L.check(lib.mq_attention_gqa_prefix(qkv.data_ptr(), out.data_ptr(), _cu(P, lens).data_ptr(), len(lens), P, max(lens), Qh, KV, hd, _s()), "mq_attention_gqa_prefix")
    torch.cuda.synchronize()
    n = GUARD * W
    assert bool((raw[:n] == NAN16).all()) and bool((raw[n + rows * W:] == NAN16).all()), "a guard row was written"
    assert bool((raw[n:n + P * W] == NAN16).all()), "a prefix row of out was written"
    assert not bool(out[P:].isnan().any()), "a segment row was left unwritten"
    return out


def _assert_parity(tag, lib, hs, P, lens):
    worst = 0.0
    for fam in ("readout", "peaked"):
        qkv = Q.make_gqa_qkv(fam, [P] + lens, *hs, seed=P + sum(lens) + hs[0], device="cuda")
        got = _run_prefix(lib, qkv, P, lens, hs)
        out, absout = QR.prefix_reference(qkv, P, lens, *hs)
        w = R.worst_coords(got[P:], out[P:], absout[P:], lens, hs[0], hs[2])
        print(f"QWENRR_RATIO {tag} heads={hs} P={P} family={fam} lens={lens} ratio={w['ratio']:.4f}")
        assert w["ratio"] <= MARGIN, (tag, hs, P, fam, lens, w)
        worst = max(worst, w["ratio"])
    return worst


# ---- mq_attention_gqa_prefix ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hs", HEADS)
@pytest.mark.parametrize("P", PREFIXES)
def test_prefix_attention_within_the_rounding_budget(lib, hs, P):
    _assert_parity("packed", lib, hs, P, SEGMENTS)


def test_prefix_and_segment_streamed_through_the_lds_in_pieces(lib):
    """128-wide heads hold 320 keys: 5 prefix tiles + 3 own tiles go through in two pieces, the second one holding the prefix's partial last tile"""
    assert (300 + 63) // 64 * 64 + 192 > Q.LDS_KEYS[128]
    _assert_parity("pieces", lib, (4, 2, 128), 300, [130])
    _assert_parity("pieces", lib, (4, 2, 128), 300, [130, 17, 200])


@pytest.mark.parametrize("hs", HEADS)
def test_without_a_prefix_the_bits_of_the_causal_kernel(lib, hs):
    Qh, KV, hd = hs
    lens = SEGMENTS + [Q.LDS_KEYS[hd] + 1]
    for fam in ("readout", "peaked"):
        qkv = Q.make_gqa_qkv(fam, lens, *hs, seed=5, device="cuda")
        got = _run_prefix(lib, qkv, 0, lens, hs)
        ref = torch.zeros_like(got)
        L.check(lib.mq_attention_gqa(qkv.data_ptr(), ref.data_ptr(), R.cu_seqlens(lens, "cuda").data_ptr(), len(lens), 0, max(lens), Qh, KV, hd, L.MQ_MASK_CAUSAL, _s()),
                "mq_attention_gqa")
        torch.cuda.synchronize()
        assert torch.equal(got.view(torch.int16), ref.view(torch.int16))


def test_torch_op_forwards_to_the_same_kernel(lib):
    hs, P, lens = (4, 2, 128), 65, [17, 70]
    qkv = Q.make_gqa_qkv("peaked", [P] + lens, *hs, seed=9, device="cuda")
    ref = _run_prefix(lib, qkv, P, lens, hs)
    out = torch.zeros_like(ref)
    L.load_torch_ops().mq_attention_gqa_prefix(qkv, _cu(P, lens), P, max(lens), *hs, out)
    torch.cuda.synchronize()
    assert torch.equal(out[P:].view(torch.int16), ref[P:].view(torch.int16)) and not bool(out[:P].any())


@pytest.mark.parametrize("hs", ((4, 2, 128), (7, 1, 64)))
@pytest.mark.parametrize("P", (65, 200))
def test_one_wrong_key_is_visible(lib, hs, P):
    """segment 1 of three; head 0 (K/V head 0).  A key gets a dominating score for query t of segment 1 when its K row is 4 x that query's q (score
    4 |q|^2 / sqrt(hd), about 45 against N(0, 1) elsewhere) and its V row is 100."""
    Qh, KV, hd = hs
    lens = [70, 70, 70]
    base = Q.make_gqa_qkv("randn", [P] + lens, *hs, seed=P, device="cuda")
    out0 = _run_prefix(lib, base, P, lens, hs)
    s1, t = P + 70, 37
    qv = base[s1 + t, :hd].float()
    kcol, vcol = Qh * hd, (Qh + KV) * hd

    def with_key(row):
        x = base.clone()
        x[row, kcol:kcol + hd] = (4.0 * qv).to(torch.bfloat16)
        x[row, vcol:vcol + hd] = 100.0
        return _run_prefix(lib, x, P, lens, hs)

    seg1 = slice(s1, s1 + 70)
    for name, row in (("last prefix key", P - 1), ("own key t", s1 + t)):
        moved = float((with_key(row)[s1 + t, :hd].float() - out0[s1 + t, :hd].float()).abs().max())
        print(f"QWENRR_KEY heads={hs} P={P} {name}: output moved by {moved:.1f}")
        assert moved > 10.0, name
    # row P of the buffer: the first masked slot of the partial prefix tile, and segment 0's first key; segment 0's last key; segment 2's first key;
    # segment 1's own key t + 1 (the causal edge)
    for name, row in (("row P", P), ("last key of segment 0", s1 - 1), ("first key of segment 2", s1 + 70)):
        got = with_key(row)
        assert torch.equal(got[seg1].view(torch.int16), out0[seg1].view(torch.int16)), name
    got = with_key(s1 + t + 1)
    assert torch.equal(got[s1:s1 + t + 1].view(torch.int16), out0[s1:s1 + t + 1].view(torch.int16)), "own key t + 1"


def test_bad_arguments_launch_nothing(lib):
    hs, P, lens = (4, 2, 64), 10, [20]
    qkv = Q.make_gqa_qkv("randn", [P] + lens, *hs, seed=1, device="cuda")
    out = torch.full((30, 256), 7.0, dtype=torch.bfloat16, device="cuda")
    cu = _cu(P, lens)
    for args, what in (((P, 20, 4, 2, 96), b"head_dim 96"), ((P, 20, 6, 4, 64), b"q_heads 6 must be a multiple of kv_heads 4"), ((-1, 20, 4, 2, 64), b"prefix_len -1"),
                       ((8000, 193, 4, 2, 64), b"exceeds 8192"), ((P, 8193, 4, 2, 64), b"8193")):
        assert lib.mq_attention_gqa_prefix(qkv.data_ptr(), out.data_ptr(), cu.data_ptr(), 1, *args, _s()) == -1 and what in lib.mq_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


# ---- mq_qk_norm_rope_at ----------------------------------------------------------------------------------------------------------------------------------
def _rope_case(lib, lens, Qh, KV, hd, norm, theta, offset):
    g = torch.Generator().manual_seed(hd + Qh + offset)
    rows, wq = sum(lens), (Qh + KV) * hd
    qkv = (torch.randn(rows, (Qh + 2 * KV) * hd, generator=g) * 2.0).to(torch.bfloat16).to("cuda")
    qg = (1.0 + 0.3 * torch.randn(hd, generator=g)).to("cuda") if norm else None
    kg = (1.0 + 0.3 * torch.randn(hd, generator=g)).to("cuda") if norm else None
    inv = (1.0 / (theta ** (torch.arange(0, hd, 2, dtype=torch.int64).float() / hd))).to("cuda")
    eps = 1e-6
    cu = R.cu_seqlens(lens, "cuda")
    work = qkv.clone()
    L.check(lib.mq_qk_norm_rope_at(work.data_ptr(), cu.data_ptr(), len(lens), 0, Qh, KV, hd, L.ptr(qg), L.ptr(kg), eps, inv.data_ptr(), offset, _s()), "mq_qk_norm_rope_at")
    torch.cuda.synchronize()
    assert torch.equal(work[:, wq:].view(torch.int16), qkv[:, wq:].view(torch.int16)), "V was touched"
    if offset == 0:
        same = qkv.clone()
        L.check(lib.mq_qk_norm_rope(same.data_ptr(), cu.data_ptr(), len(lens), 0, Qh, KV, hd, L.ptr(qg), L.ptr(kg), eps, inv.data_ptr(), _s()), "mq_qk_norm_rope")
        torch.cuda.synchronize()
        assert torch.equal(work.view(torch.int16), same.view(torch.int16))
    # float64 from the bf16 input, the budget of tests/test_qwen_gpu.py::_qk_reference with the position offset + t
    x = qkv[:, :wq].double().reshape(rows, Qh + KV, hd)
    if norm:
        gam = torch.cat([qg.double()[None].expand(Qh, hd), kg.double()[None].expand(KV, hd)])[None]
        x = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * gam
    t = torch.cat([torch.arange(ln, device="cuda") for ln in lens]).double() + offset
    ang = t[:, None] * inv.double()[None, :]
    cos, sin = ang.cos()[:, None, :], ang.sin()[:, None, :]
    a, b = x[..., :hd // 2], x[..., hd // 2:]
    y = torch.cat([a * cos - b * sin, b * cos + a * sin], dim=-1)
    bound = (a * a + b * b).sqrt() * (ang.abs()[:, None, :] + 24.0) * U
    B = torch.cat([bound, bound], dim=-1) + RR.half_ulp_bf16(y)
    r = RR.ratio(work[:, :wq], y.reshape(rows, -1), B.reshape(rows, -1))
    print(f"QWENRR_RATIO qk_norm_rope_at offset={offset} lens={lens} heads=({Qh},{KV},{hd}) norm={norm} ratio={r:.4f}")
    assert r <= ROW_MARGIN


@pytest.mark.parametrize("hd", (64, 128))
@pytest.mark.parametrize("offset", (0, 1, 65, 8000))
def test_qk_norm_rope_at_an_offset(lib, hd, offset):
    _rope_case(lib, [1, 17, 70], 4, 2, hd, True, 1e6, offset)
    _rope_case(lib, [1, 17, 70], 7, 1, hd, False, 1e4, offset)


# ---- the tower ------------------------------------------------------------------------------------------------------------------------------------------
DOC_LENS = [1, 17, 70, 200]
P_TOWER = 37        # (37 + 200 <= 256 positions of the tiny configs; not a multiple of 64)


@pytest.fixture(scope="module")
def towers():
    from marqo_amd.engine.rerank import QwenRerankerTower
    tk = QR.train_tokenizer()
    yes, no = tk.token_to_id("yes"), tk.token_to_id("no")
    out = {}
    for i, (name, cfg, kind) in enumerate((("TINY3", Q.TINY3, "lm"), ("TINY64", Q.TINY64, "lm"), ("TINY64", Q.TINY64, "cls"))):
        model = QR.hf_reranker(cfg, kind, seed=7 + i)
        arch = archs.qwen_arch_from_hf_config(cfg)
        sd = {k: v.float() for k, v in model.state_dict().items()}
        tower = QwenRerankerTower(arch, sd, DEV, tk, QR.score_row(model, kind, yes, no, torch.float32))
        shared = Q.random_seqs([P_TOWER], cfg["vocab_size"], seed=20 + i)[0]
        segs = Q.random_seqs(DOC_LENS, cfg["vocab_size"], seed=30 + i)
        ref = QR.hf_pair_logits(model, kind, [torch.cat([shared, s]) for s in segs], yes, no).numpy()
        out[(name, kind)] = dict(cfg=cfg, model=model, tower=tower, shared=shared, segs=segs, ref=ref, yes=yes, no=no, kind=kind)
    return out


def _np(t):
    return t.numpy().astype(np.int32)


@pytest.mark.parametrize("key", (("TINY3", "lm"), ("TINY64", "lm"), ("TINY64", "cls")))
def test_shared_run_against_float64_transformers(towers, key):
    t = towers[key]
    tower, shared, segs, ref = t["tower"], t["shared"], t["segs"], t["ref"]
    whole = [_np(torch.cat([shared, s])) for s in segs]
    z_un, s_un = tower.score_rows(np.zeros(0, np.int32), whole)
    z_sh, s_sh = tower.score_rows(_np(shared), [_np(s) for s in segs])
    e_un, e_sh = float(np.abs(z_un - ref).max()), float(np.abs(z_sh - ref).max())
    print(f"QWENRR_TOWER {key}: logits {ref.round(4).tolist()} err unshared={e_un:.3e} shared={e_sh:.3e} (bar 1.5 x unshared = {1.5 * e_un:.3e}) "
          f"per doc unshared={np.abs(z_un - ref).round(5).tolist()} shared={np.abs(z_sh - ref).round(5).tolist()}")
    assert e_sh <= 1.5 * e_un
    np.testing.assert_allclose(s_sh, 1.0 / (1.0 + np.exp(-z_sh.astype(np.float64))), atol=2e-7)
    # batches of one document each (the prefix is recomputed per batch) and a permuted call give the same bits
    tower.max_rows_per_call, keep = 1, tower.max_rows_per_call
    try:
        z_one, _ = tower.score_rows(_np(shared), [_np(s) for s in segs])
    finally:
        tower.max_rows_per_call = keep
    perm = [2, 0, 3, 1]
    z_perm, _ = tower.score_rows(_np(shared), [_np(segs[i]) for i in perm])
    assert np.array_equal(z_perm, z_sh[perm])
    print(f"QWENRR_TOWER {key}: one document per batch differs from one batch by {float(np.abs(z_one - z_sh).max()):.3e}")
    assert float(np.abs(z_one - ref).max()) <= 1.5 * e_un


def test_ranking_follows_the_reference(towers):
    t = towers[("TINY3", "lm")]
    tower, shared = t["tower"], t["shared"]
    cand = Q.random_seqs([5 + 3 * i for i in range(24)], t["cfg"]["vocab_size"], seed=77)
    ref = QR.hf_pair_logits(t["model"], t["kind"], [torch.cat([shared, s]) for s in cand], t["yes"], t["no"]).numpy()
    got, _ = tower.score_rows(_np(shared), [_np(s) for s in cand])
    err = float(np.abs(got - ref).max())
    pick = []
    for i in np.argsort(ref):
        if not pick or ref[i] - ref[pick[-1]] > 2 * err:
            pick.append(int(i))
    print(f"QWENRR_RANK measured error {err:.3e}; {len(pick)} of 24 documents lie more than twice that apart")
    assert len(pick) >= 6
    pick = sorted(pick)
    assert np.array_equal(np.argsort(got[pick]), np.argsort(ref[pick]))


# ---- from a checkpoint directory ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ckpt(tmp_path_factory):
    cfg = Q.config_dict(Q.TINY64, max_position_embeddings=2048)
    # (gain 1.5: behind the template's 29 suffix tokens a document moves the logit of the 0.6 models by 0.2 over forty candidates, too little to tell six
    # hits apart at the bar below; at 1.5 the candidates spread over 1.9)
    model = QR.hf_reranker(cfg, "lm", seed=3, gain=1.5)
    tk = QR.train_tokenizer()
    d = QR.write_reranker_dir(str(tmp_path_factory.mktemp("qwen3rr") / "reranker"), cfg, model, "lm", tk)
    return dict(dir=d, cfg=cfg, model=model, tk=tk)


def _reference_logits(ckpt, query, docs, max_length, instruction=None):
    """the model card's recipe on the host: prefix + ids(body)[:max_length - len(prefix) - len(suffix)] + suffix, one pair at a time, float64
    -> (logits, the pairs' ids)"""
    from marqo_amd.engine import rerank as E
    tk = ckpt["tk"]
    enc = lambda s: tk.encode(s, add_special_tokens=False).ids
    pre, suf = enc(E.QWEN_RERANK_PREFIX), enc(E.QWEN_RERANK_SUFFIX)
    head = E.qwen_rerank_head(E.QWEN_RERANK_INSTRUCTION if instruction is None else instruction, query)
    seqs = [torch.tensor(pre + enc(head + " " + d)[:max_length - len(pre) - len(suf)] + suf) for d in docs]
    return QR.hf_pair_logits(ckpt["model"], "lm", seqs, tk.token_to_id("yes"), tk.token_to_id("no")).numpy(), seqs


def test_rerank_search_results_on_the_engine(ckpt):
    """The yardstick of every comparison is the tower bar above: the error of the unshared run (score_rows with no shared rows: mq_encode_qwen's tower
    plus the head) on the SAME pairs against the same float64 model, times 1.5.  Where the engine itself must take the unshared path, its logits are
    that run's bit for bit."""
    from marqo_amd.engine.rerank import QwenRerankerTower
    from marqo_amd.s2_inference.reranking.rerank import rerank_search_results
    from marqo_amd.s2_inference.s2_inference import _create_model_cache_key, get_available_models
    from tests import rerank_modernbert_ref as RM
    name, query = ckpt["dir"], RM.sentence(5, 1)
    direct = QwenRerankerTower.from_dir(name, DEV)
    unshared = lambda seqs: direct.score_rows(np.zeros(0, np.int32), [_np(s) for s in seqs])[0]
    cand = [RM.sentence(2 + 3 * i, 400 + i) for i in range(40)]          # one sentence per field: one chunk per hit
    zc, seqs_c = _reference_logits(ckpt, query, cand, 512)
    e_un = float(np.abs(unshared(seqs_c) - zc).max())
    pick = []
    for i in np.argsort(zc):      # hits the bar can tell apart: float64 logits more than 2 x (1.5 x the unshared error) from their neighbours
        if not pick or zc[i] - zc[pick[-1]] > 3 * e_un:
            pick.append(int(i))
    assert len(pick) >= 6, f"the fixture's logits are closer than the error {e_un} can tell apart: {np.sort(zc)}"
    pick = sorted(pick[:6])
    texts, z = [cand[i] for i in pick], zc[pick]
    hits = [{"_id": f"doc{i}", "body": texts[i], "_score": 0.5 + 0.01 * i} for i in range(6)]
    result = {"hits": copy.deepcopy(hits), "limit": 6}
    rerank_search_results(result, query, name, DEV)
    key = _create_model_cache_key(name, DEV)
    model = get_available_models()[key]["model"]
    try:
        tower = model.tower
        assert isinstance(tower, QwenRerankerTower) and tower.last_prefix_len > 0
        got = {h["_id"]: h["_score"] for h in result["hits"]}
        err_s = max(abs(got[f"doc{i}"] - 1.0 / (1.0 + math.exp(-z[i]))) for i in range(6))
        print(f"QWENRR_E2E unshared logit error over 40 candidates {e_un:.3e}; max |score - sigmoid(float64 logit)| = {err_s:.3e} "
              f"(bar 1.5 x that / 4 = {1.5 * e_un / 4:.3e}: the sigmoid's slope is at most 1/4); shared prefix of {tower.last_prefix_len} tokens")
        assert err_s <= 1.5 * e_un / 4
        assert [h["_id"] for h in result["hits"]] == [f"doc{i}" for i in np.argsort(-z)]
        assert all(h["_highlights"] == [{"body": texts[int(h["_id"][3:])]}] for h in result["hits"])

        def shared_case(tag, max_length, **kw):
            zr, seqs = _reference_logits(ckpt, query, texts, max_length, **kw)
            bar = 1.5 * float(np.abs(unshared(seqs) - zr).max())
            lg, _ = tower.score(query, texts, max_length, **kw)
            err = float(np.abs(lg - zr).max())
            print(f"QWENRR_E2E {tag}: logit error {err:.3e} (bar 1.5 x unshared = {bar:.3e}), shared prefix {tower.last_prefix_len}")
            assert tower.last_prefix_len > 0 and err <= bar
            return zr, seqs
        # another instruction is another score, and the reference's
        zi, _ = shared_case("instruction", 512, instruction="find the recipe")
        assert float(np.abs(zi - z).max()) > 3 * e_un
        # truncation: every pair over the cap is cut as the reference cuts it (the shared part + four document tokens)
        shared, _ = tower.rows_for(query, texts, 512)
        cap = int(shared.size) + len(tower.suffix_ids) + 4
        _, seqs_cut = shared_case("cut", cap)
        assert all(len(s) == cap for s in seqs_cut) and min(len(s) for s in _reference_logits(ckpt, query, texts, 512)[1]) > cap
        # a cap the shared part alone reaches, and a leading combining mark: the unshared path, the bits of per-pair scoring
        small = int(shared.size) + len(tower.suffix_ids) - 2
        for tag, docs, ml in (("cap inside the shared part", texts, small), ("combining mark", ["\u0301" + texts[0], texts[1]], 512)):
            zr, seqs = _reference_logits(ckpt, query, docs, ml)
            lg, _ = tower.score(query, docs, ml)
            assert tower.last_prefix_len == 0 and np.array_equal(lg, unshared(seqs)), tag
            assert ml == 512 or all(len(s) == ml for s in seqs)
            print(f"QWENRR_E2E {tag}: unshared, logit error {float(np.abs(lg - zr).max()):.3e}")
    finally:
        get_available_models().pop(key, None)

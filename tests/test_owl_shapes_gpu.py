"""The four OWL-ViT head kernels (csrc/owl_head.hip) at the shapes the served checkpoints run, against the float64 references and budgets of
tests/owl_ref.py, through the C ABI, every output inside guard-filled buffers; then the whole chain once at owlvit-base-patch32's widths.  The
fixtures are owl_ref's (tests/test_owl_host.py checks their premises on the CPU); tests/test_owl_gpu.py holds the toy-shape tests.

    mq_owl_topk        P one below / at / above one trip of the 256 threads, 576 and the limit 8191; k up to P: exact, every element, NaN bits included
    mq_owl_merge_ln    every MQ_DISPATCH_CH branch (CH = 1, 2, 3, 4, 6 twice, 8), one patch row and 9 rows, and T = 577; row indexing bit for bit
    mq_owl_class_head  Q = 8 at (W, Dq) = (768, 512) and (1024, 768), widths ragged against 64, an exact tie between two queries, one-hot masks
    mq_owl_box_head    grids 24, 7, 3, a non-square target, and rows that differ through the grid bias alone

Worst |kernel - float64| / budget seen on the MI355X (printed by the tests):
    merge_ln    fp32 0.047, bf16 0.998 (a bf16 output next to a rounding tie uses its half ulp); the constant row 0.028; the offset class row's image 0.010
    class_head  logit 0.022, score 0.038        box_head  0.030
The fp32 budgets are worst-case bounds (a chain of D roundings counted as D u); random rows use a few per cent of them.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import owl_ref as O  # noqa: E402
import rowops_ref as R  # noqa: E402
from marqo_amd import _lib as L  # noqa: E402
from test_owl_gpu import DEV, _f32, _guarded, _guards_intact, _i32, _stream, _sync_check  # noqa: E402

pytestmark = pytest.mark.gpu
TARGET = (240, 240)
CHAIN_SHAPE = "b32x1"
# Image seeds of the chain test, chosen on the CPU: the oracle alone decides the top-1 patch of both images by more than twice the tolerance
# (tests/test_owl_host.py asserts it).
CHAIN_IMAGE_SEEDS = (85, 52)
# Worst |max-over-queries logit - fp32 transformers| and worst |box coordinate - fp32 transformers| (pixels of the 240 x 240 frame) over the 2 images
# x 576 patches of test_chain_at_base_patch32_widths, as MEASURED on the MI355X on the first run of that test.  The tolerance is twice the
# measurement (tile plans differ in summation order) and must stay below a quarter of the standard deviation of the oracle's logits (asserted).
# The oracle's logits spread by 0.953, so the error is 5 % of the spread (0.098 < 0.238); the boxes are off by 1.3 % of the frame.  The oracle's top-1
# margins on the two images are 2.29 and 1.60.
LOGIT_ERR_MEASURED = 4.9198e-02
BOX_ERR_MEASURED = 3.0748e+00
LOGIT_TOL = 2 * LOGIT_ERR_MEASURED
BOX_TOL = 2 * BOX_ERR_MEASURED


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


# ---- top-k -----------------------------------------------------------------------------------------------------------------------------------------------
def _topk(lib, score, boxes, k):
    """launch inside guards -> (rc, scores [n, k], boxes [n, k, 4], patch [n, k], guards intact, outputs untouched)"""
    n, P = score.shape
    (sbuf, ts), (bbuf, tb), (pbuf, tp) = _guarded(n, k, pad=4), _guarded(n * k, 4, pad=4), _guarded(n, k, torch.int32, pad=4)
    d_s, d_b = _f32(score), _f32(boxes)
    rc = lib.mq_owl_topk(d_s.data_ptr(), d_b.data_ptr(), n, P, k, ts.data_ptr(), tb.data_ptr(), tp.data_ptr(), _stream())
    torch.cuda.synchronize(DEV)
    intact = _guards_intact(sbuf, n, pad=4) and _guards_intact(bbuf, n * k, pad=4) and _guards_intact(pbuf, n, pad=4)
    untouched = bool(ts.isnan().all()) and bool(tb.isnan().all()) and bool((tp == -7777).all())
    return rc, ts.cpu().numpy(), tb.cpu().numpy().reshape(n, k, 4), tp.cpu().numpy(), intact, untouched


@pytest.mark.parametrize("kind", O.TOPK_KINDS)
@pytest.mark.parametrize("P", O.TOPK_P)
def test_topk_is_exact(P, kind):
    lib = L.load()
    score, boxes = O.topk_fixture(kind, P)
    for k in O.topk_ks(P):
        rc, ts, tb, tp, intact, _ = _topk(lib, score, boxes, k)
        L.check(rc, "mq_owl_topk")
        assert intact, "a guard row changed"
        rs, rb, rp = O.topk_reference(score, boxes, k)
        assert rp.shape == (3, k)
        assert np.array_equal(tp, rp), f"P={P} k={k} {kind}: the patch numbers must be exact"
        assert np.array_equal(_bits(ts), _bits(rs)) and np.array_equal(_bits(tb), _bits(rb)), f"P={P} k={k} {kind}: scores and boxes bit for bit"
    # what the reference must have said for k = P (the last k of the loop): the properties by name, not through argsort
    assert k == P
    if kind == "distinct":
        assert tuple(tp[:, 0]) == (0, 256 if P > 256 else P // 2, P - 1)
    elif kind == "ties":
        for img in range(3):
            pairs = list(zip(-ts[img].astype(np.float64), tp[img]))
            assert pairs == sorted(pairs), "descending, and a tie lists the lower patch first"
    else:
        where = O.topk_nan_patches(P)
        assert list(tp[0, P - len(where):]) == where, "the NaNs take the last ranks in patch order"
        assert np.array_equal(_bits(ts[0, P - len(where):]), _bits(score[0, where])) and not np.isnan(ts[0, :P - len(where)]).any()
        assert np.array_equal(tp[1], np.arange(P)), "an image of NaNs alone keeps its patch order"
        assert np.array_equal(_bits(ts[1]), _bits(score[1]))


@pytest.mark.parametrize("P,k,msg", [(8192, 1, b"P=8192"), (576, 577, b"k=577"), (8191, 8192, b"k=8192")])
def test_topk_refuses_and_writes_nothing(P, k, msg):
    lib = L.load()
    g = np.random.default_rng(1)
    rc, _, _, _, intact, untouched = _topk(lib, g.uniform(0, 1, (2, P)).astype(np.float32), np.zeros((2, P, 4), np.float32), k)
    assert rc == -1 and msg in lib.mq_last_error()
    assert intact and untouched, "a refused call wrote to its outputs"


# ---- merge + LayerNorm -----------------------------------------------------------------------------------------------------------------------------------
def _merge(lib, x, pg, pb, lg, lb, n, T, W, bf16=True):
    rows = n * (T - 1)
    (fb_buf, fb), (ff_buf, ff) = _guarded(rows, W, torch.bfloat16), _guarded(rows, W)
    keep = [_f32(v) for v in (x, pg, pb, lg, lb)]
    _sync_check(lib.mq_owl_merge_ln(*(k.data_ptr() for k in keep), fb.data_ptr() if bf16 else None, ff.data_ptr(), n, T, W, 1e-5, _stream()), "mq_owl_merge_ln")
    assert _guards_intact(ff_buf, rows) and _guards_intact(fb_buf, rows), "a guard row changed"
    assert bf16 or bool(fb.float().isnan().all())
    return ff.cpu().numpy(), fb.float().cpu().numpy()


@pytest.mark.parametrize("n,T,W", O.MERGE_CASES)
def test_merge_ln_every_chunk_count(n, T, W):
    lib = L.load()
    x, pg, pb, lg, lb = O.merge_fixture(n, T, W)
    ff, fb = _merge(lib, x, pg, pb, lg, lb, n, T, W)
    f, B = O.merge_ln_reference(x, n, T, pg, pb, lg, lb, 1e-5)
    assert np.isfinite(B).all()
    r32 = O.ratio(ff, f, B)
    r16 = O.ratio(fb, f, B + R.half_ulp_bf16(torch.from_numpy(f)).numpy())
    c = O.merge_const_row(n, T)
    rc = O.ratio(ff[c], f[c], B[c]) if c is not None else 0.0
    r0 = O.ratio(ff[:T - 1], f[:T - 1], B[:T - 1])
    print(f"OWL_SHAPES merge_ln n={n} T={T} W={W}: worst |kernel - fp64| / budget fp32 {r32:.3f} bf16 {r16:.3f}; constant row {rc:.3f}; offset class row's image {r0:.3f}")
    assert r32 <= 1.0 and r16 <= 1.0


def test_merge_ln_refuses_too_wide_a_row():
    lib = L.load()
    buf, ff = _guarded(9, 2052)
    x = torch.zeros(12, 2052, device=DEV)
    v = torch.zeros(2052, device=DEV)
    rc = lib.mq_owl_merge_ln(x.data_ptr(), v.data_ptr(), v.data_ptr(), v.data_ptr(), v.data_ptr(), None, ff.data_ptr(), 3, 4, 2052, 1e-5, _stream())
    torch.cuda.synchronize(DEV)
    assert rc == -1 and b"W=2052" in lib.mq_last_error()
    assert bool(buf.isnan().all()), "a refused call wrote to its output"


def test_merge_ln_rows_read_their_own_image():
    """bit for bit at (n, T, W) = (3, 5, 768): an element of image 1's class row reaches all 4 rows of image 1 and no other; an element of one patch
    row reaches that output row alone"""
    lib = L.load()
    n, T, W = 3, 5, 768
    x, pg, pb, lg, lb = O.merge_fixture(n, T, W)
    base, _ = _merge(lib, x, pg, pb, lg, lb, n, T, W, bf16=False)
    changed = lambda out: sorted(set(np.nonzero((_bits(out) != _bits(base)).any(axis=1))[0].tolist()))
    y = x.copy()
    y[1 * T, 300] += np.float32(0.5)                    # image 1's class row (a column of the second chunk)
    assert changed(_merge(lib, y, pg, pb, lg, lb, n, T, W, bf16=False)[0]) == [4, 5, 6, 7]
    for img, p in ((0, 0), (1, 2), (2, 3)):
        y = x.copy()
        y[img * T + 1 + p, 701] += np.float32(0.5)      # (a column of the third chunk)
        assert changed(_merge(lib, y, pg, pb, lg, lb, n, T, W, bf16=False)[0]) == [img * (T - 1) + p]


# ---- class head -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(O.CLASS_CASES))
def test_class_head_at_the_query_limit(name):
    lib = L.load()
    fx = O.class_fixture(name)
    ref = O.class_reference(fx)
    n, P, W, Dq, Q, rows = fx["n"], fx["P"], fx["W"], fx["Dq"], fx["Q"], fx["n"] * fx["P"]
    (sbuf, score), (lbuf, logit), (abuf, label) = _guarded(1, rows), _guarded(1, rows), _guarded(1, rows, torch.int32)
    keep = [_f32(fx["e"]), _f32(fx["f"]), _f32(fx["t"]), None if fx["mask"] is None else _i32(fx["mask"]), _f32(fx["sw"]), _f32(fx["cw"])]
    _sync_check(lib.mq_owl_class_head(keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), L.ptr(keep[3]), fx["per_image"], keep[4].data_ptr(),
                                      fx["sb"], keep[5].data_ptr(), fx["cb"], score.data_ptr(), logit.data_ptr(), label.data_ptr(), n, P, W, Dq, Q,
                                      _stream()), "mq_owl_class_head")
    assert _guards_intact(sbuf, 1) and _guards_intact(lbuf, 1) and _guards_intact(abuf, 1), "a guard row changed"
    got_z, got_s, got_a = logit[0].cpu().numpy(), score[0].cpu().numpy(), label[0].cpu().numpy()
    rz, rs = O.ratio(got_z, ref["best"], ref["B_best"]), O.ratio(got_s, ref["score"], ref["B_score"])
    sure = ref["label_sure"] if fx["tie"] is None else O.sure_apart_from_twin(ref, fx["tie"][1])
    print(f"OWL_SHAPES class_head {name}: worst / budget logit {rz:.3f} score {rs:.3f}; rows with a sure label {int(sure.sum())}/{rows}")
    assert rz <= 1.0 and rs <= 1.0
    assert np.isfinite(got_z[3]) and sure.sum() * 4 >= rows * 3
    assert (got_a[sure] == ref["label"][sure]).all()
    if fx["mask"] is not None:
        assert (got_a[:P] == 7).all() and (got_a[P:] == 0).all(), "one live query per image: its number is the label"
    if fx["tie"] is not None:
        a, b = fx["tie"]
        assert not (ref["label"] == b).any() and (ref["label"] == a).sum() >= rows // 8, "argmax names the lower of two equal queries"
        assert not (got_a == b).any(), "of two equal queries the lower index wins"
        assert (got_a[sure & (ref["label"] == a)] == a).all()


# ---- box head -----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(O.BOX_CASES))
def test_box_head_at_served_grids(name):
    from marqo_amd.engine.owl import box_bias
    lib = L.load()
    fx = O.box_fixture(name)
    n, P, W, rows = fx["n"], fx["P"], fx["W"], fx["n"] * fx["P"]
    bias = box_bias(fx["grid"]).numpy()
    d_bias = torch.full((P + 1, 4), float("nan"), dtype=torch.float32, device=DEV)      # a row past the table reads NaN, not a neighbour's memory
    d_bias[:P] = _f32(bias)
    buf, boxes = _guarded(rows, 4, pad=4)
    keep = [_f32(fx["h"]).to(torch.bfloat16), _f32(fx["w2"]), _f32(fx["b2"]), d_bias]
    _sync_check(lib.mq_owl_box_head(*(k.data_ptr() for k in keep), boxes.data_ptr(), n, P, W, float(O.BOX_TARGET[0]), float(O.BOX_TARGET[1]), _stream()),
                "mq_owl_box_head")
    assert _guards_intact(buf, rows, pad=4), "a guard row changed"
    _, ref, B = O.box_head_reference(fx["h"], fx["w2"], fx["b2"], bias, P, O.BOX_TARGET)
    got = boxes.cpu().numpy()
    r = O.ratio(got, ref, B)
    print(f"OWL_SHAPES box_head {name} target={O.BOX_TARGET}: worst |kernel - fp64| / budget = {r:.3f}")
    assert r <= 1.0
    if O.BOX_CASES[name][3]:
        assert np.array_equal(_bits(got[P:]), _bits(got[:P])), "equal hidden rows: image 1's boxes are image 0's"


# ---- the chain at owlvit-base-patch32's widths ---------------------------------------------------------------------------------------------------------------------
def chain_images():
    return [O.images(1, seed=s)[0] for s in CHAIN_IMAGE_SEEDS]


def test_chain_at_base_patch32_widths(tmp_path):
    from marqo_amd.engine.owl import OwlTower
    d = str(tmp_path / "owlvit-b32x1")
    O.write_owl_dir(d, CHAIN_SHAPE, seed=0)
    t = OwlTower.from_dir(d, DEV)
    assert (t.patches, t.arch.tokens, t.arch.width, t.arch.query_dim) == (576, 577, 768, 512)
    model = O.load_hf(d)
    pil = chain_images()
    u8 = torch.from_numpy(np.stack([np.asarray(im) for im in pil]))
    live = [i for i, q in enumerate(O.CHAIN_QUERIES) if q]
    assert len(O.CHAIN_QUERIES) == 8 and len(live) == 7
    ids = np.zeros((8, O.CTX), dtype=np.int64)                 # the empty query is an all-zero id row: the oracle masks it
    ids[live] = t.query_ids([O.CHAIN_QUERIES[i] for i in live])
    ref = O.hf_forward(model, ids, O.pixel_values(pil, t.arch.image_size), TARGET)
    score, logit, label, boxes = t.detect_all(O.CHAIN_QUERIES, u8, TARGET)
    ts, tb, tp = (v.cpu().numpy() for v in t.topk(score, boxes, 300))
    score, logit, label, boxes = (v.cpu().numpy() for v in (score, logit, label, boxes))
    assert score.shape == (2, 576) and boxes.shape == (2, 576, 4) and not (label == 3).any()
    assert np.allclose(score, 1.0 / (1.0 + np.exp(-logit.astype(np.float64))), rtol=0, atol=1e-6)
    worst_z, worst_b = float(np.abs(logit - ref["best"]).max()), float(np.abs(boxes - ref["boxes"]).max())
    srt = np.sort(ref["best"], axis=1)
    margin, std = srt[:, -1] - srt[:, -2], float(ref["best"].std())
    print(f"OWL_SHAPES chain {CHAIN_SHAPE}: worst |logit - fp32 transformers| = {worst_z:.4e}; worst |box - fp32 transformers| = {worst_b:.4e} px; std of the "
          f"oracle's logits = {std:.3f}; the oracle's top-1 margins {margin}; labels {np.bincount(label.ravel(), minlength=8)}")
    rs, rb, rp = O.topk_reference(score, boxes, 300)           # on the kernel's own scores: exact
    assert np.array_equal(tp, rp) and np.array_equal(_bits(ts), _bits(rs)) and np.array_equal(_bits(tb), _bits(rb))
    assert LOGIT_TOL < std / 4, "finding: the tolerance is not below a quarter of the spread of the logits"
    assert worst_z <= LOGIT_TOL and worst_b <= BOX_TOL
    ok = margin > 2 * LOGIT_TOL
    assert ok.all(), "the image seeds are chosen so that the oracle decides both images"
    assert np.array_equal(tp[:, 0], ref["best"].argmax(1))

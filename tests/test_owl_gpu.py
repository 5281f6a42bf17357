"""OWL-ViT image reranking on the GPU (csrc/owl_head.hip, engine/owl.py, s2_inference/reranking): the four kernels against the float64 references
and budgets of tests/owl_ref.py, the image path against Pillow and OwlViTImageProcessorPil, the whole tower against transformers'
OwlViTForObjectDetection in fp32, and the public call.  Outputs sit inside guard-filled buffers."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import owl_ref as O  # noqa: E402
import rowops_ref as R  # noqa: E402
from marqo_amd import _lib as L  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TARGET = (240, 240)
TOWER_SEED = 0
# Image seeds of the tower tests, chosen on the CPU so that the ORACLE ALONE decides the top-1 patch by far more than twice the tolerance on five of
# the six images of a shape (margins 0.93 .. 1.9 for both queries; tests/test_owl_host.py asserts it); the sixth is an arbitrary one.
IMAGE_SEEDS = {"g3": (291, 173, 171, 151, 230, 5), "g5": (332, 210, 334, 285, 212, 5)}

# Worst |max-over-queries logit - fp32 transformers| and worst |box coordinate - fp32 transformers| (pixels of the 240 x 240 working image) over
# the 6 images x 2 queries (8 and 16 tokens) of test_tower_matches_transformers, as MEASURED on the MI355X on the first run of this test with
# these images, per shape.  The oracle's logits spread by 1.311 (g3) and 1.260 (g5), so the error is 9 % and 6 % of the spread; the boxes are off by
# 1.2 % and 2.2 % of the frame.  The tolerance is twice the measurement: tile plans and batch compositions differ in summation order (g3's 54 patch
# rows take the skinny GEMMs, g5's 150 the tiled ones).  The logit tolerance must stay below a quarter of the standard deviation of the oracle's
# logits (asserted): 0.231 < 0.328 and 0.147 < 0.315.
LOGIT_ERR_MEASURED = {"g3": 1.1556e-01, "g5": 7.3314e-02}
BOX_ERR_MEASURED = {"g3": 2.9597e+00, "g5": 5.3881e+00}
LOGIT_TOL = {k: 2 * v for k, v in LOGIT_ERR_MEASURED.items()}
BOX_TOL = {k: 2 * v for k, v in BOX_ERR_MEASURED.items()}


def tower_images(shape):
    return [O.images(1, seed=s)[0] for s in IMAGE_SEEDS[shape]]


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def _sync_check(rc, what):
    L.check(rc, what)
    torch.cuda.synchronize(DEV)


def _f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)


def _guarded(rows, cols, dtype=torch.float32, pad=2):
    """[rows + 2 pad, cols] of NaN (int32: -7777) whose middle the kernel writes -> (buffer, view of the middle)"""
    fill = -7777 if dtype == torch.int32 else float("nan")
    buf = torch.full((rows + 2 * pad, cols), fill, dtype=dtype, device=DEV)
    return buf, buf[pad:pad + rows]


def _guards_intact(buf, rows, pad=2):
    edge = torch.cat([buf[:pad], buf[pad + rows:]])
    return bool((edge == -7777).all()) if buf.dtype == torch.int32 else bool(edge.float().isnan().all())


# ---- merge + LayerNorm ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [128, 192])
@pytest.mark.parametrize("T", [10, 26])
@pytest.mark.parametrize("n", [1, 3])
def test_merge_ln(n, T, W):
    lib = L.load()
    g = np.random.default_rng(100 * n + T + W)
    x = (g.standard_normal((n * T, W)) * g.uniform(0.3, 3.0, (n * T, 1)) + g.uniform(-1, 1, (n * T, 1))).astype(np.float32)
    pg, lg = ((1 + 0.2 * g.standard_normal(W)).astype(np.float32) for _ in range(2))
    pb, lb = ((0.2 * g.standard_normal(W)).astype(np.float32) for _ in range(2))
    rows = n * (T - 1)
    (fb_buf, fb), (ff_buf, ff) = _guarded(rows, W, torch.bfloat16), _guarded(rows, W)
    keep = [_f32(v) for v in (x, pg, pb, lg, lb)]
    _sync_check(lib.mq_owl_merge_ln(*(k.data_ptr() for k in keep), fb.data_ptr(), ff.data_ptr(), n, T, W, 1e-5, _stream()), "mq_owl_merge_ln")
    assert _guards_intact(fb_buf, rows) and _guards_intact(ff_buf, rows), "a guard row changed"
    f, B = O.merge_ln_reference(x, n, T, pg, pb, lg, lb, 1e-5)
    r32 = O.ratio(ff.cpu().numpy(), f, B)
    r16 = O.ratio(fb.float().cpu().numpy(), f, B + R.half_ulp_bf16(torch.from_numpy(f)).numpy())
    print(f"merge_ln n={n} T={T} W={W}: worst |kernel - fp64| / budget fp32 {r32:.3f} bf16 {r16:.3f}")
    assert r32 <= 1.0 and r16 <= 1.0
    only = torch.full((rows, W), float("nan"), dtype=torch.float32, device=DEV)        # one output alone: the same bits
    _sync_check(lib.mq_owl_merge_ln(*(k.data_ptr() for k in keep), None, only.data_ptr(), n, T, W, 1e-5, _stream()), "mq_owl_merge_ln")
    assert torch.equal(only.view(torch.int32), ff.contiguous().view(torch.int32))
    assert lib.mq_owl_merge_ln(256, 256, 256, 256, 256, 256, None, 1, 1, W, 1e-5, None) == -1 and b"T=1" in lib.mq_last_error()
    assert lib.mq_owl_merge_ln(256, 256, 256, 256, 256, 256, None, 1, T, 130, 1e-5, None) == -1 and b"W=130" in lib.mq_last_error()


# ---- class head -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q,per_image", [(1, 0), (3, 0), (3, 1)])
def test_class_head(Q, per_image):
    lib = L.load()
    n, P, W, Dq = 2, 25, 192, 128
    rows = n * P
    g = np.random.default_rng(7 + Q + per_image)
    e = g.standard_normal((rows, Dq)).astype(np.float32)
    e[3] = 0.0                                                   # a zero-norm embedding row
    f = g.standard_normal((rows, W)).astype(np.float32)
    t = g.standard_normal((n, Q, Dq) if per_image else (Q, Dq)).astype(np.float32)
    mask = None
    if Q == 3:
        mask = np.ones(t.shape[:-1], dtype=np.int32)
        mask[..., 1] = 0                                         # one masked query (its embedding is what an all-zero id row gives: anything)
        if per_image:
            mask[1] = (0, 1, 1)
    sw, cw = (g.standard_normal(W) / np.sqrt(W)).astype(np.float32), (1.5 * g.standard_normal(W) / np.sqrt(W)).astype(np.float32)
    sb, cb = -0.2, 0.4
    ref = O.class_head_reference(e, f, t, mask, sw, np.float32(sb), cw, np.float32(cb), P)
    assert (ref["pre"] < -0.5).any() and (ref["pre"] > 0.5).any(), "the fixture must reach both ELU branches"
    (sbuf, score), (lbuf, logit), (abuf, label) = _guarded(1, rows), _guarded(1, rows), _guarded(1, rows, torch.int32)
    keep = [_f32(e), _f32(f), _f32(t), None if mask is None else _i32(mask), _f32(sw), _f32(cw)]
    _sync_check(lib.mq_owl_class_head(keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), L.ptr(keep[3]), per_image, keep[4].data_ptr(), sb,
                                      keep[5].data_ptr(), cb, score.data_ptr(), logit.data_ptr(), label.data_ptr(), n, P, W, Dq, Q, _stream()),
                "mq_owl_class_head")
    assert _guards_intact(sbuf, 1) and _guards_intact(lbuf, 1) and _guards_intact(abuf, 1), "a guard row changed"
    got_z, got_s, got_a = logit[0].cpu().numpy(), score[0].cpu().numpy(), label[0].cpu().numpy()
    rz, rs = O.ratio(got_z, ref["best"], ref["B_best"]), O.ratio(got_s, ref["score"], ref["B_score"])
    print(f"class_head Q={Q} per_image={per_image}: worst / budget logit {rz:.3f} score {rs:.3f}; rows with a sure label {int(ref['label_sure'].sum())}/{rows}")
    assert rz <= 1.0 and rs <= 1.0
    assert np.isfinite(got_z[3]) and ref["label_sure"].sum() >= rows * 3 // 4
    assert (got_a[ref["label_sure"]] == ref["label"][ref["label_sure"]]).all()
    if Q == 3:
        assert not (got_a == 1).any() if not per_image else (not (got_a[:P] == 1).any() and not (got_a[P:] == 0).any())
        # every query masked: the dtype minimum, a score of exactly 0, label 0
        zero = _i32(np.zeros_like(mask))
        _sync_check(lib.mq_owl_class_head(keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), zero.data_ptr(), per_image, keep[4].data_ptr(), sb,
                                          keep[5].data_ptr(), cb, score.data_ptr(), logit.data_ptr(), label.data_ptr(), n, P, W, Dq, Q, _stream()),
                    "mq_owl_class_head")
        assert bool((logit[0] == -torch.finfo(torch.float32).max).all()) and bool((score[0] == 0).all()) and bool((label[0] == 0).all())
    assert lib.mq_owl_class_head(256, 256, 256, None, 0, 256, 0.0, 256, 0.0, 256, 256, 256, 1, P, W, Dq, 9, None) == -1 and b"Q=9" in lib.mq_last_error()


# ---- box head ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("target", [(240, 240), (320, 200)])
@pytest.mark.parametrize("grid", [3, 5])
def test_box_head(grid, target):
    from marqo_amd.engine.owl import box_bias
    lib = L.load()
    n, P, W = 2, grid * grid, 192
    rows = n * P
    g = np.random.default_rng(31 + grid)
    h = R.round_bf16(np.abs(g.standard_normal((rows, W))).astype(np.float32))      # (bf16 values: the GELU epilogue's output format, exact)
    w2 = (2.0 * g.standard_normal((4, W)) / np.sqrt(W)).astype(np.float32)
    b2 = np.array([0.3, -0.3, 0.2, -0.2], dtype=np.float32)
    bias = box_bias(grid).numpy()
    assert np.array_equal(bias.astype(np.float64), O.box_bias_reference(grid)), "the grid bias is the model's float32 constant"
    buf, boxes = _guarded(rows, 4, pad=4)
    keep = [_f32(h).to(torch.bfloat16), _f32(w2), _f32(b2), _f32(bias)]
    _sync_check(lib.mq_owl_box_head(*(k.data_ptr() for k in keep), boxes.data_ptr(), n, P, W, float(target[0]), float(target[1]), _stream()),
                "mq_owl_box_head")
    assert _guards_intact(buf, rows, pad=4), "a guard row changed"
    pred, ref, B = O.box_head_reference(h, w2, b2, bias, P, target)
    r = O.ratio(boxes.cpu().numpy(), ref, B)
    print(f"box_head grid={grid} target={target}: worst |kernel - fp64| / budget = {r:.3f}")
    assert r <= 1.0
    last_col = pred.reshape(n, grid, grid, 4)[:, :, -1, 0]
    assert (last_col > 0.99).all() and (pred[:, 0] < 0.9).any(), "edge cells must sit at the end of the grid bias, others inside"
    assert lib.mq_owl_box_head(256, 256, 256, 256, 256, 1, 0, W, 1.0, 1.0, None) == -1 and b"bad shape" in lib.mq_last_error()


# ---- top-k ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 3, 25, 31])
def test_topk(k):
    lib = L.load()
    n, T = 3, 26
    P = T - 1
    g = np.random.default_rng(5)
    score = g.uniform(0.05, 0.8, (n, P)).astype(np.float32)
    score[0, 0], score[1, 12], score[2, P - 1] = 0.95, 0.96, 0.97          # maxima at the first, a middle and the last patch
    score[1, 20] = score[1, 4] = np.float32(0.9)                            # an exact tie in second place: the lower patch first
    score[2, 3] = score[2, P - 1]                                           # ... and one for the first place
    boxes = g.uniform(0, 240, (n, P, 4)).astype(np.float32)
    kk = min(k, P)                                                          # (the engine clamps; the entry point refuses k > P)
    (sbuf, ts), (bbuf, tb), (pbuf, tp) = _guarded(n, kk, pad=4), _guarded(n * kk, 4, pad=4), _guarded(n, kk, torch.int32, pad=4)
    d_s, d_b = _f32(score), _f32(boxes)
    _sync_check(lib.mq_owl_topk(d_s.data_ptr(), d_b.data_ptr(), n, P, kk, ts.data_ptr(), tb.data_ptr(), tp.data_ptr(), _stream()), "mq_owl_topk")
    assert _guards_intact(sbuf, n, pad=4) and _guards_intact(bbuf, n * kk, pad=4) and _guards_intact(pbuf, n, pad=4), "a guard row changed"
    rs, rb, rp = O.topk_reference(score, boxes, k)
    assert rs.shape == (n, kk)
    assert np.array_equal(tp.cpu().numpy(), rp), "the patch numbers must be exact"
    assert np.array_equal(ts.cpu().numpy().view(np.int32), rs.view(np.int32)) and np.array_equal(tb.cpu().numpy().reshape(n, kk, 4).view(np.int32), rb.view(np.int32))
    assert rp[0, 0] == 0 and rp[1, 0] == 12 and rp[2, 0] == 3 and (kk < 2 or (rp[2, 1] == P - 1 and (kk < 3 or tuple(rp[1, 1:3]) == (4, 20))))
    if k > P:
        assert lib.mq_owl_topk(d_s.data_ptr(), d_b.data_ptr(), n, P, k, ts.data_ptr(), tb.data_ptr(), tp.data_ptr(), _stream()) == -1
        assert b"k=31" in lib.mq_last_error()


# ---- fixtures of the tower tests --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dirs(tmp_path_factory):
    root = tmp_path_factory.mktemp("owl")
    out = {}
    for shape in O.TOY_SHAPES:
        out[shape] = str(root / "hf" / "google" / ("owlvit-base-patch32" if shape == "g5" else "owlvit-" + shape))
        O.write_owl_dir(out[shape], shape, seed=TOWER_SEED)
    out["root"] = str(root)
    return out


@pytest.fixture(scope="module")
def towers(dirs):
    from marqo_amd.engine.owl import OwlTower
    cache = {}

    def get(shape):
        if shape not in cache:
            cache[shape] = OwlTower.from_dir(dirs[shape], DEV)
        return cache[shape]
    return get


# ---- image path ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(240, 240), (200, 150)])
def test_image_path_is_pillows(towers, size):
    from PIL import Image
    t = towers("g5")
    S = t.arch.image_size
    pil = O.images(2, seed=11, size=size)
    u8 = torch.from_numpy(np.stack([np.asarray(im) for im in pil])).to(DEV)
    with torch.cuda.device(DEV):
        got = t.resize(u8)
        px = torch.empty(2, 3, S, S, dtype=torch.float32, device=DEV)
        _sync_check(t.lib.mq_to_tensor_normalize(got.data_ptr(), px.data_ptr(), 2, S, t.mean, t.std, _stream()), "mq_to_tensor_normalize")
    want = np.stack([np.asarray(im.resize((S, S), Image.BICUBIC)) for im in pil])
    assert np.array_equal(got.cpu().numpy(), want), "the S x S image must equal Pillow's bicubic resize bit for bit"
    ref = O.pixel_values(pil, S).double().numpy()
    err = np.abs(px.cpu().double().numpy() - ref).max()
    tol = 4 * O.U * np.abs(ref).max()             # b / 255, - mean, / std in fp32 on either side: a few roundings of values below 2.7
    print(f"pixel_values {size}: worst |engine - OwlViTImageProcessorPil| = {err:.3e} (tolerance {tol:.3e})")
    assert err <= tol


# ---- whole tower ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["g3", "g5"])
def test_tower_matches_transformers(dirs, towers, shape):
    t = towers(shape)
    model = O.load_hf(dirs[shape])
    pil = tower_images(shape)
    pix = O.pixel_values(pil, t.arch.image_size)
    u8 = torch.from_numpy(np.stack([np.asarray(im) for im in pil]))
    worst_z = worst_b = 0.0
    sure = agree = total = 0
    stds = []
    for q in (O.QUERY_SHORT, O.QUERY_FULL):
        ids = t.query_ids([q])
        assert (q != O.QUERY_FULL) or int((ids > 0).sum()) == 16
        ref = O.hf_forward(model, ids, pix, TARGET)
        score, logit, label, boxes = (v.cpu().numpy() for v in t.detect_all(q, u8, TARGET))
        assert score.shape == (6, t.patches) and boxes.shape == (6, t.patches, 4) and not label.any()
        assert np.allclose(score, 1.0 / (1.0 + np.exp(-logit.astype(np.float64))), rtol=0, atol=1e-6)
        worst_z, worst_b = max(worst_z, float(np.abs(logit - ref["best"]).max())), max(worst_b, float(np.abs(boxes - ref["boxes"]).max()))
        stds.append(float(ref["best"].std()))
        srt = np.sort(ref["best"], axis=1)
        ok = srt[:, -1] - srt[:, -2] > 2 * LOGIT_TOL[shape]
        ts, tb, tp = t.detect(q, u8, k=3, target_size=TARGET)
        assert np.array_equal(tp[:, 0], logit.argmax(1)) and np.array_equal(ts, np.take_along_axis(score, tp.astype(np.int64), 1))
        sure, total = sure + int(ok.sum()), total + ok.size
        agree += int((tp[ok, 0] == ref["best"].argmax(1)[ok]).sum())
    print(f"owl {shape}: worst |logit - fp32 transformers| = {worst_z:.4e}; worst |box - fp32 transformers| = {worst_b:.4e} px; std of the oracle's "
          f"logits = {min(stds):.3f}; images with a top-1 margin above twice the tolerance {sure}/{total}, top-1 patch agrees on {agree}")
    assert LOGIT_TOL[shape] < min(stds) / 4, "finding: the tolerance is not below a quarter of the spread of the logits"
    assert worst_z <= LOGIT_TOL[shape] and worst_b <= BOX_TOL[shape]
    assert sure * 4 >= total * 3 and agree == sure


def test_query_limit(towers):
    t = towers("g3")
    assert t.query_ids([O.QUERY_FULL]).shape == (1, 16)
    with pytest.raises(ValueError, match="at most 16"):
        t.detect(O.QUERY_LONG, np.zeros((1, 240, 240, 3), np.uint8))


def test_configurations_the_kernels_cannot_run_are_refused(dirs, tmp_path):
    import json
    import shutil
    from marqo_amd.engine.owl import OwlTower
    d = str(tmp_path / "narrow_heads")
    shutil.copytree(dirs["g3"], d)
    cfg = json.load(open(os.path.join(d, "config.json")))
    cfg["vision_config"]["num_attention_heads"] = 4            # 32-wide heads
    json.dump(cfg, open(os.path.join(d, "config.json"), "w"))
    with pytest.raises(ValueError, match="64-wide attention heads"):
        OwlTower.from_dir(d, DEV)
    os.remove(os.path.join(d, "merges.txt"))
    with pytest.raises(FileNotFoundError, match="merges.txt"):
        OwlTower.from_dir(d, DEV)


# ---- the public call -----------------------------------------------------------------------------------------------------------------------------------------
def test_rerank_search_results_on_the_engine(dirs, tmp_path, monkeypatch):
    from PIL import Image
    from marqo_amd.engine.owl import OwlTower
    from marqo_amd.s2_inference.processing.image import rescale_box
    from marqo_amd.s2_inference.reranking.rerank import rerank_search_results
    from marqo_amd.s2_inference.s2_inference import _create_model_cache_key, get_available_models
    monkeypatch.setenv("MARQO_AMD_MODEL_DIR", dirs["root"])
    sizes = [(240, 240), (320, 200), (100, 180), (64, 64), (500, 333), (240, 120)]
    paths = []
    for i, (im, size) in enumerate(zip(tower_images("g5"), sizes)):
        im = im.resize(size)
        im = im.convert("L") if i == 2 else (im.convert("RGBA") if i == 4 else im)
        paths.append(str(tmp_path / f"im{i}.png"))
        im.save(paths[-1])
    hits = [{"_id": f"doc{i}", "image": p, "title": f"t{i}", "_score": 0.5 + 0.01 * i} for i, p in enumerate(paths)]
    result = {"hits": copy.deepcopy(hits), "limit": 6}
    name, query = "owl/ViT-B/32", O.QUERY_SHORT
    rerank_search_results(result, query, name, DEV, searchable_attributes=["image", "title"])
    key = _create_model_cache_key("google/owlvit-base-patch32", DEV)
    assert key in get_available_models()
    tower = get_available_models()[key]["model"]
    assert isinstance(tower, OwlTower) and tower.arch.grid == 5
    # the oracle on the same working images
    work = [Image.open(p).resize(TARGET).convert("RGB") for p in paths]
    ref = O.hf_forward(O.load_hf(dirs["g5"]), tower.query_ids([query]), O.pixel_values(work, tower.arch.image_size), TARGET)
    tol = LOGIT_TOL["g5"]
    srt = np.sort(ref["best"], axis=1)
    got = {h["_id"]: h for h in result["hits"]}
    assert len(got) == 6 and len(result["hits"]) == 6
    for i, (h, size) in enumerate(zip(hits, sizes)):
        out = got[h["_id"]]
        assert isinstance(out["_score"], float) and abs(out["_score"] - ref["score"][i].max()) <= tol / 4     # sigmoid' <= 1 / 4
        (field, box), = out["_highlights"][0].items()
        assert field == "image" and len(out["_highlights"]) == 1 and len(box) == 4
        if srt[i, -1] - srt[i, -2] > 2 * tol:
            want = rescale_box(ref["boxes"][i, ref["best"][i].argmax()].tolist(), TARGET, size)
            assert np.abs(np.asarray(box) - np.asarray(want)).max() <= BOX_TOL["g5"] * max(size[0] / 240, size[1] / 240)
        assert not any(k in out for k in ("_rerank_id", "_reranked_score", "_reranked_highlights"))
    order = [h["_score"] for h in result["hits"]]
    assert order == sorted(order, reverse=True)
    want_order = np.argsort(-ref["score"].max(1))
    for a, b in zip(want_order[:-1], want_order[1:]):     # two hits the oracle separates by more than both errors keep their order
        if ref["score"][a].max() - ref["score"][b].max() > tol / 2:
            assert order.index(got[f"doc{a}"]["_score"]) < order.index(got[f"doc{b}"]["_score"])
    # a second call finds the model in the cache: nothing is loaded
    monkeypatch.setattr(OwlTower, "from_dir", classmethod(lambda cls, *a, **k: (_ for _ in ()).throw(AssertionError("loaded twice"))))
    again = {"hits": copy.deepcopy(hits)}
    rerank_search_results(again, query, name, DEV, searchable_attributes=["image"])
    assert [(h["_id"], h["_score"]) for h in again["hits"]] == [(h["_id"], h["_score"]) for h in result["hits"]]
    del get_available_models()[key]

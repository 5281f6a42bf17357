"""OWL-ViT image reranking without a GPU: the float64 references of tests/owl_ref.py against transformers' OwlViTForObjectDetection, the
conditions the synthetic checkpoints must meet, names, attribute rules, the missing checkpoint, the 16-token limit, the result plumbing against
the reference's own code, and the library's argument checks."""
import copy
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import owl_ref as O  # noqa: E402
import test_owl_gpu as G  # noqa: E402  (the measured tolerances and the seeds of the tower tests)
import test_owl_shapes_gpu as S  # noqa: E402  (... and of the chain at owlvit-base-patch32's widths)
from marqo_amd import _lib as L  # noqa: E402
from marqo_amd.engine import archs  # noqa: E402
from marqo_amd.engine.hf_clip import load_tokenizer  # noqa: E402
from marqo_amd.engine.owl import OwlTower, box_bias  # noqa: E402
from marqo_amd.s2_inference.errors import RerankerError, RerankerNameError  # noqa: E402
from marqo_amd.s2_inference.reranking import cross_encoders, rerank  # noqa: E402
from oracle import ref_shim  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TARGET = (240, 240)


@pytest.fixture(scope="module")
def oracle(tmp_path_factory):
    """per shape: the checkpoint directory, the fp32 model, and its outputs on the tower tests' images for both queries"""
    root = tmp_path_factory.mktemp("owl_host")
    out = {}
    for shape in O.TOY_SHAPES:
        d = str(root / shape)
        O.write_owl_dir(d, shape, seed=G.TOWER_SEED)
        model, tok = O.load_hf(d), load_tokenizer(d, O.CTX)
        stub = types.SimpleNamespace(arch=archs.owl_arch_from_hf_config(json.load(open(os.path.join(d, "config.json")))), tokenizer=tok)
        pix = O.pixel_values(G.tower_images(shape), O.SHAPES[shape]["image"])
        runs = {q: O.hf_forward(model, OwlTower.query_ids(stub, [q]), pix, TARGET) for q in (O.QUERY_SHORT, O.QUERY_FULL)}
        out[shape] = dict(dir=d, model=model, stub=stub, runs=runs)
    return out


# ---- the references are the installed model's arithmetic -------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["g3", "g5"])
def test_references_match_transformers(oracle, shape):
    """From the model's own last_hidden_state and query_embeds, float64 against fp32.  Every output is a chain of W-term dot products of O(1)
    values behind LayerNorms: fp32 summation of W terms is within W u of the sum of the absolute products, which the unit-variance features and
    1 / sqrt(W)-scaled weights keep below ~4 max(1, |value|), so 4 W u max(1, max|logit|) bounds a logit; sigmoid' <= 1 / 4 carries the same bound
    (without the magnitude) to pred_boxes and scores, and the target size multiplies it for the boxes, plus their own product's rounding."""
    o = oracle[shape]
    W = O.SHAPES[shape]["W"]
    for q, r in o["runs"].items():
        mine = O.heads_reference(o["model"].state_dict(), r["hidden"], r["query_embeds"], None, TARGET)
        tol = 4 * W * O.U * max(1.0, float(np.abs(r["logits"]).max()))
        assert mine["logits"].shape == r["logits"].shape == (6, (O.SHAPES[shape]["image"] // 32) ** 2, 1)
        assert np.abs(mine["logits"] - r["logits"]).max() <= tol
        assert np.abs(mine["best"] - r["best"]).max() <= tol
        assert np.abs(mine["pred_boxes"] - r["pred_boxes"]).max() <= 4 * W * O.U
        assert np.abs(mine["score"] - r["score"]).max() <= 4 * W * O.U
        assert np.abs(mine["boxes"] - r["boxes"]).max() <= 240 * (4 * W * O.U + 4 * O.U)
    G1 = int(round(np.sqrt(r["logits"].shape[1])))
    assert np.abs(box_bias(G1).numpy() - o["model"].box_bias.numpy()).max() == 0.0
    assert np.abs(O.box_bias_reference(G1) - o["model"].box_bias.double().numpy()).max() == 0.0


@pytest.mark.parametrize("shape", ["g3", "g5"])
def test_fixture_is_not_degenerate(oracle, shape):
    o = oracle[shape]
    for q, r in o["runs"].items():
        mine = O.heads_reference(o["model"].state_dict(), r["hidden"], r["query_embeds"], None, TARGET)
        assert r["best"].std() >= 0.5, "the reference logits must spread"
        assert (mine["pre"] < 0).mean() >= 0.05 and (mine["pre"] > 0).mean() >= 0.05, "both ELU branches must occur"
        cx = r["pred_boxes"][..., 0]
        assert ((cx > 0.05) & (cx < 0.95)).any() and (cx > 0.99).any(), "boxes inside and at the end of the grid bias"
        # the oracle alone: the top-1 patch is decided by more than twice the GPU tolerance on three quarters of the images
        srt = np.sort(r["best"], axis=1)
        assert (srt[:, -1] - srt[:, -2] > 2 * G.LOGIT_TOL[shape]).sum() * 4 >= 6 * 3, (shape, q, srt[:, -1] - srt[:, -2])
        assert G.LOGIT_TOL[shape] < r["best"].std() / 4
    assert len(OwlTower.query_ids(o["stub"], [O.QUERY_SHORT])[0].nonzero()[0]) == 8


def test_topk_reference_ties_and_clamp():
    s = np.array([[0.2, 0.9, 0.9, 0.1]], dtype=np.float32)
    b = np.arange(16, dtype=np.float32).reshape(1, 4, 4)
    ts, tb, tp = O.topk_reference(s, b, 9)
    assert tp.tolist() == [[1, 2, 0, 3]] and ts.tolist() == [[np.float32(0.9), np.float32(0.9), np.float32(0.2), np.float32(0.1)]] and tb[0, 0].tolist() == [4, 5, 6, 7]


# ---- premises of the fixtures of tests/test_owl_shapes_gpu.py --------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [24, 48, 60])
def test_box_bias_at_the_served_grids(grid):
    assert {a.grid for a in archs.OWL_ARCHS.values()} == {24, 48, 60}
    got = box_bias(grid)
    assert got.dtype == O.torch.float32 and tuple(got.shape) == (grid * grid, 4)
    assert np.array_equal(got.numpy().astype(np.float64), O.box_bias_reference(grid)), "the grid bias is the model's float32 constant, exactly"


@pytest.mark.parametrize("P", O.TOPK_P)
def test_topk_fixtures_hold_what_they_promise(P):
    d, _ = O.topk_fixture("distinct", P)
    assert all(len(set(row.tolist())) == P for row in d), "distinct scores"
    assert tuple(d.argmax(1)) == (0, 256 if P > 256 else P // 2, P - 1)
    t, _ = O.topk_fixture("ties", P)
    assert set(np.unique(t).tolist()) == set(O.TIE_VALUES) and np.float32(1.0) in t and np.float32(0.0) in t
    assert len(O.topk_ks(P)) >= 3 and O.topk_ks(P)[-1] == P
    if P > 256:
        for row in t:       # a tie between two threads' patches on either side of the first trip, and one within a thread (a and a + 256)
            assert any(row[a] == row[b] for a in range(0, 256, 37) for b in range(256, P)), "no tie a < 256 <= b"
            assert row[0] == row[256], "no tie between a and a + 256"
    s, _ = O.topk_fixture("nan", P)
    assert sorted(np.nonzero(np.isnan(s[0]))[0].tolist()) == O.topk_nan_patches(P) and np.isnan(s[1]).all() and np.isnan(s[2]).sum() == len(range(0, P, 7))
    assert len(set(s[1].view(np.uint32)[:5].tolist())) == 5, "NaNs of different bit patterns"
    rs, _, rp = O.topk_reference(s, np.zeros((3, P, 4), np.float32), P)
    assert rp[0, -len(O.topk_nan_patches(P)):].tolist() == O.topk_nan_patches(P) and rp[1].tolist() == list(range(P))
    assert not np.isnan(rs[0, :P - len(O.topk_nan_patches(P))]).any()


@pytest.mark.parametrize("n,T,W", O.MERGE_CASES)
def test_merge_budget_of_the_offset_and_the_constant_row(n, T, W):
    """The class row of image 0 has a mean 50 x its spread: its LayerNorm's budget carries the mean's error c = D u A with A = 50 sigma, so
    B_c ~ |g| 50 D u (1e-4 at D = 40), and every row of image 0 inherits it through |p| B_c.

    The constant patch row x = a has d = 0 and sigma' = sqrt(eps), so rowops_ref.reference_ln gives it exactly
        B_p,j = |pg_j| D u |a| / sqrt(eps) + 2 u |pb_j|                 D = ceil(W / 64) + 8
    This is no slack.  The kernel's mean of W copies of a rounded a is off by up to D u |a|; EVERY deviation of the row is that one error, and
    rstd = 1 / sqrt(eps) = 316 multiplies it: p_j = pb_j + pg_j s with one s, |s| <= D u |a| / sqrt(eps) (8e-4 at W = 2048, a = 0.7).  The product
    with the class row scales it by |c_j| (up to ~3) and the last LayerNorm by |lg_j| / sigma'(m) (2 + |d_j| / sigma'(m)), where m = pb c has a
    spread of only ~0.2 (the bias's): about 1e-2 at W = 768 and 4e-2 at W = 2048, for outputs whose spread is 1.  So the budget of that row cannot be
    1e-3 max|ln bias| (6e-4) unless |a| is below 0.03; it has to be what the two-pass algorithm's amplification makes it.  Asserted: B_p equals the
    closed form, the row's budget is finite, below 5 % of the spread of the row's own output (a row that took another row's statistics, or skipped a
    LayerNorm, is off by the spread itself), and within the closed form carried through the last LayerNorm's push."""
    x, pg, pb, lg, lb = O.merge_fixture(n, T, W)
    f, B = O.merge_ln_reference(x, n, T, pg, pb, lg, lb, 1e-5)
    assert np.isfinite(B).all() and (B > 0).all()
    x0 = x[0].astype(np.float64)
    assert 49 * x0.std() < abs(x0.mean()) < 51 * x0.std(),"image 0's class row: a mean of 50 x the spread"
    assert B[:T - 1].max() < 0.01 * f[:T - 1].std(), "the offset class row leaves its image a budget of under 1 % of the outputs' spread"
    r = O.merge_const_row(n, T)
    if r is None:
        return
    a, D, se = float(np.float32(O.MERGE_CONST)), int(np.ceil(W / 64)) + 8, np.sqrt(1e-5)
    assert (x[n * T - 1] == np.float32(O.MERGE_CONST)).all()
    _, Bp = O._ln(x[n * T - 1:], pg, pb, 1e-5)
    lead = np.abs(pg.astype(np.float64)) * D * O.U * a / se + 2 * O.U * np.abs(pb.astype(np.float64))
    assert np.allclose(Bp[0], lead, rtol=1e-9, atol=0)
    assert B[r].max() < 0.05 * f[r].std()
    # carried through: e_j <= |c_j| lead_j + (|pb_j| + lead_j) B_c,j + u |m_j|, then owl_ref's push of the last LayerNorm
    c, Bc = O._ln(x[(n - 1) * T:(n - 1) * T + 1], pg, pb, 1e-5)
    m = pb.astype(np.float64) * c[0]
    e = np.abs(c[0]) * lead + (np.abs(pb) + lead) * Bc[0] + O.U * np.abs(m)
    _, Bm = O._ln(m[None], lg, lb, 1e-5)
    bound = 1.01 * Bm[0] + O._ln_push(m[None], lg.astype(np.float64), e[None], 1e-5)[0]
    assert (B[r] <= bound * (1 + 1e-9)).all() and (B[r] >= 0.99 * bound).all(), "the constant row's budget is the derived one"


@pytest.mark.parametrize("name", list(O.CLASS_CASES))
def test_class_fixtures_decide_their_labels(name):
    fx = O.class_fixture(name)
    ref = O.class_reference(fx)
    rows = fx["n"] * fx["P"]
    assert (ref["pre"] < -0.5).any() and (ref["pre"] > 0.5).any(), "the fixture must reach both ELU branches"
    assert not fx["e"][3].any() and np.isfinite(ref["best"][3]), "the zero-norm embedding row"
    sure = ref["label_sure"] if fx["tie"] is None else O.sure_apart_from_twin(ref, fx["tie"][1])
    assert sure.sum() * 4 >= rows * 3, "three quarters of the rows must have a sure label"
    assert fx["Q"] == 8 or (fx["W"] % 64 and fx["Dq"] % 64), "the query limit, or widths ragged against the 64 lanes"
    if fx["mask"] is not None:
        assert (ref["label"][:fx["P"]] == 7).all() and (ref["label"][fx["P"]:] == 0).all() and ref["label_sure"].all()
    if fx["tie"] is not None:
        a, b = fx["tie"]
        assert np.array_equal(ref["logits"][:, a], ref["logits"][:, b]) and not (ref["label"] == b).any()
        assert (sure & (ref["label"] == a)).sum() >= rows // 8, "rows that the tied pair wins, surely ahead of the other six"
    else:
        assert len(np.unique(ref["label"][ref["label_sure"]])) >= min(fx["Q"], 5) or fx["mask"] is not None, "several queries win somewhere"


def test_box_fixture_of_equal_rows_tells_every_patch_apart():
    fx = O.box_fixture("grid24_same_rows")
    P = fx["P"]
    assert (fx["h"] == fx["h"][0]).all()
    pred, boxes, B = O.box_head_reference(fx["h"], fx["w2"], fx["b2"], box_bias(24).numpy(), P, O.BOX_TARGET)
    assert np.array_equal(boxes[:P], boxes[P:])
    b = boxes[:P]
    assert (np.abs(b[1:] - b[:-1]).max(-1) > 100 * B.max()).all(), "neighbouring patches differ by more than 100 x the budget"
    apart = np.abs(b[:, None, :] - b[None, :, :]).max(-1) + np.diag(np.full(P, np.inf))
    assert apart.min() > 100 * B.max(), "so do any two patches: no mix-up of bias rows fits the budget"
    assert pred.min() > 0.01 and pred.max() < 0.9999, "no sigmoid saturates"


@pytest.fixture(scope="module")
def chain_oracle(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("owl_chain") / S.CHAIN_SHAPE)
    O.write_owl_dir(d, S.CHAIN_SHAPE, seed=0)
    model, tok = O.load_hf(d), load_tokenizer(d, O.CTX)
    stub = types.SimpleNamespace(arch=archs.owl_arch_from_hf_config(json.load(open(os.path.join(d, "config.json")))), tokenizer=tok)
    live = [i for i, q in enumerate(O.CHAIN_QUERIES) if q]
    ids = np.zeros((len(O.CHAIN_QUERIES), O.CTX), dtype=np.int64)
    ids[live] = OwlTower.query_ids(stub, [O.CHAIN_QUERIES[i] for i in live])
    return stub, O.hf_forward(model, ids, O.pixel_values(S.chain_images(), O.SHAPES[S.CHAIN_SHAPE]["image"]), TARGET)


def test_chain_shape_is_base_patch32s_and_the_oracle_decides_both_images(chain_oracle):
    stub, r = chain_oracle
    a, served = stub.arch, archs.OWL_ARCHS["google/owlvit-base-patch32"]
    assert (a.image_size, a.patch_size, a.width, a.heads, a.mlp_dim, a.text_width, a.query_dim, a.ctx, a.tokens, a.layers) == \
        (served.image_size, served.patch_size, served.width, served.heads, served.mlp_dim, served.text_width, served.query_dim, served.ctx, 577, 1)
    assert r["logits"].shape == (2, 576, 8) and (r["logits"][..., 3] < -1e30).all(), "the empty query is masked by the oracle too"
    assert len(np.unique(r["logits"].argmax(-1))) >= 4, "several queries win somewhere"
    assert r["best"].std() >= 0.5, "the reference logits must spread"
    srt = np.sort(r["best"], axis=1)
    assert S.LOGIT_TOL < r["best"].std() / 4
    assert (srt[:, -1] - srt[:, -2] > 2 * S.LOGIT_TOL).all(), srt[:, -1] - srt[:, -2]


# ---- names, attributes, checkpoints, the query limit ---------------------------------------------------------------------------------------------
def test_arch_table_and_names():
    assert {k: (a.tokens, a.width, a.query_dim) for k, a in archs.OWL_ARCHS.items()} == {
        "google/owlvit-base-patch32": (577, 768, 512), "google/owlvit-base-patch16": (2305, 768, 512), "google/owlvit-large-patch14": (3601, 1024, 768)}
    for name, mapped in (("owl/ViT-B/32", "google/owlvit-base-patch32"), ("owl/ViT-B/16", "google/owlvit-base-patch16"),
                         ("owl/ViT-L/14", "google/owlvit-large-patch14"), ("google/owlvit-large-patch14", "google/owlvit-large-patch14")):
        assert cross_encoders.ReRankerOwl(name, "cpu", TARGET)._model_map[name] == mapped
    with pytest.raises(RerankerNameError, match="could not find model_name=owl/ViT-H/14"):
        cross_encoders.ReRankerOwl("owl/ViT-H/14", "cpu", TARGET)
    with pytest.raises(RerankerError, match="could not find model_name=owl/ViT-H/14"):
        rerank.rerank_search_results({"hits": [{"_id": "a", "image": "x.png"}]}, "q", "owl/ViT-H/14", "cpu", searchable_attributes=["image"])
    with pytest.raises(KeyError, match="projection_dim=64 must equal"):
        archs.owl_arch_from_hf_config(dict(model_type="owlvit", projection_dim=64, text_config=dict(hidden_size=128)))
    a = archs.owl_arch_from_hf_config(dict(model_type="owlvit", vision_config=dict(patch_size=16)), archs.OWL_ARCHS["google/owlvit-base-patch16"])
    assert a == archs.OWL_ARCHS["google/owlvit-base-patch16"]


def test_searchable_attribute_rules(monkeypatch):
    r = {"hits": [{"_id": "a", "image": "x.png"}]}
    for bad in (None, [], (), ""):
        with pytest.raises(RerankerError, match="expected list of strings for owl/ViT-B/32"):
            rerank.rerank_search_results(copy.deepcopy(r), "q", "owl/ViT-B/32", "cpu", searchable_attributes=bad)
    assert rerank.rerank_search_results(copy.deepcopy(r), "q", "owl/ViT-B/32", "cpu", searchable_attributes=["nothing"]) == r     # no hit holds it: untouched
    seen = {}

    class Spy(cross_encoders.ReRankerOwl):
        def rerank(self, query, results, image_attributes, num_highlights=1):
            seen.update(attributes=image_attributes, num_highlights=num_highlights, size=self.image_size)
    monkeypatch.setattr(rerank, "ReRankerOwl", Spy)
    rerank.rerank_search_results(copy.deepcopy(r), "q", "owl/ViT-B/32", "cpu", searchable_attributes=["image", "title"], num_highlights=3)
    assert seen == dict(attributes=["image"], num_highlights=1, size=(240, 240))


def test_missing_checkpoint_and_unreadable_images(tmp_path, monkeypatch):
    monkeypatch.setenv("MARQO_AMD_MODEL_DIR", str(tmp_path))
    monkeypatch.setenv("HF_HOME", str(tmp_path / "hf_home"))
    r = {"hits": [{"_id": "a", "image": str(tmp_path / "not-there.png")}]}
    with pytest.raises(RerankerError, match="google/owlvit-base-patch16: the OWL-ViT image reranker is not served without a local checkpoint.*never downloads"):
        rerank.rerank_search_results(copy.deepcopy(r), "q", "owl/ViT-B/16", "cpu", searchable_attributes=["image"])     # (the model loads before any image opens)
    # a directory that is there but is not OWL-ViT
    d = tmp_path / "hf" / "google" / "owlvit-base-patch32"
    d.mkdir(parents=True)
    (d / "config.json").write_text(json.dumps({"model_type": "bert"}))
    (d / "model.safetensors").write_bytes(b"\x08\x00\x00\x00\x00\x00\x00\x00{}      ")
    with pytest.raises(RerankerError, match="cannot load the image reranker google/owlvit-base-patch32.*not 'owlvit'"):
        rerank.rerank_search_results(copy.deepcopy(r), "q", "owl/ViT-B/32", "cpu", searchable_attributes=["image"])
    # with a model, an image pointer that is neither a file nor a URL is the reference's UnidentifiedImageError -> RerankerError
    monkeypatch.setattr(cross_encoders, "load_owl_vit", lambda model_name, device: {"model": _Fake()})
    with pytest.raises(RerankerError, match="not a local file or a valid url"):
        rerank.rerank_search_results(copy.deepcopy(r), "q", "owl/ViT-B/32", "cpu", searchable_attributes=["image"])


def test_query_limit(oracle, tmp_path, monkeypatch):
    stub = oracle["g3"]["stub"]
    ids = OwlTower.query_ids(stub, [O.QUERY_FULL, O.QUERY_SHORT])
    assert ids.shape == (2, 16) and (ids[0] > 0).all() and ids[0, 0] == stub.tokenizer.sot_id and ids[0, 15] == stub.tokenizer.eot_id == ids[1].max()
    with pytest.raises(ValueError, match="17 tokens.*at most 16"):
        OwlTower.query_ids(stub, [O.QUERY_LONG])

    class Limited(_Fake):
        def detect(self, query, images_u8, k=1, target_size=(240, 240)):
            OwlTower.query_ids(stub, [query])
            return super().detect(query, images_u8, k, target_size)
    monkeypatch.setattr(cross_encoders, "load_owl_vit", lambda model_name, device: {"model": Limited()})
    p = str(tmp_path / "a.png")
    O.images(1, seed=1)[0].save(p)
    r = {"hits": [{"_id": "a", "image": p}]}
    with pytest.raises(RerankerError, match="at most 16"):
        rerank.rerank_search_results(copy.deepcopy(r), O.QUERY_LONG, "owl/ViT-B/32", "cpu", searchable_attributes=["image"])
    rerank.rerank_search_results(r, O.QUERY_FULL, "owl/ViT-B/32", "cpu", searchable_attributes=["image"])
    assert isinstance(r["hits"][0]["_score"], float)


def test_tokenizer_files_must_agree(tmp_path):
    O.write_tokenizer_files(tmp_path)
    tok = load_tokenizer(str(tmp_path), 16)
    assert tok.eot_id == 512 + len(O.MERGES) + 1 and tok.encode("the cat") == [tok.encoder["the</w>"], tok.encoder["cat</w>"]]
    v = json.load(open(tmp_path / "vocab.json"))
    v["cat</w>"], v["dog</w>"] = v["dog</w>"], v["cat</w>"]
    (tmp_path / "vocab.json").write_text(json.dumps(v))
    with pytest.raises(ValueError, match="does not number the tokens"):
        load_tokenizer(str(tmp_path), 16)


def test_product_reranking_does_not_import_pandas():
    code = ("import sys; import marqo_amd.s2_inference.reranking.rerank, marqo_amd.s2_inference.reranking.cross_encoders, marqo_amd.engine.owl; "
            "sys.exit(1 if 'pandas' in sys.modules else 0)")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    assert subprocess.run([sys.executable, "-c", code], env=env, timeout=300).returncode == 0


# ---- plumbing against the reference's own code ---------------------------------------------------------------------------------------------------
class _Fake:
    """the injected detector: per image the fixed scores and boxes of owl_ref.fake_detection, best first"""

    def detect(self, query, images_u8, k=1, target_size=(240, 240)):
        assert tuple(target_size) == (240, 240) and images_u8.dtype == np.uint8 and images_u8.shape[1:] == (240, 240, 3)
        s, b = zip(*[O.fake_detection(im) for im in images_u8])
        return O.topk_reference(np.stack(s), np.stack(b), k)


def _cases(root):
    sizes = [(240, 240), (320, 200), (100, 180), (64, 48)]
    paths = []
    for i, (im, size) in enumerate(zip(O.images(4, seed=21), sizes)):
        paths.append(os.path.join(str(root), f"im{i}.png"))
        im.resize(size).save(paths[-1])
    hit = lambda i, p, **kw: {"_id": f"doc{i}", "image": p, "title": f"title {i}", "_score": 0.9 - 0.1 * i, "_highlights": {"title": f"title {i}"}, **kw}
    many = [hit(i, p) for i, p in enumerate(paths)]
    shared = [hit(0, paths[1]), hit(1, paths[2]), hit(2, paths[1])]
    no_field = many[:2] + [{"_id": "bare", "title": "no image here", "_score": 0.3}] + many[2:]
    base = dict(query="a cat", model_name="owl/ViT-B/32", attributes=["image"])
    return {
        "one_hit": dict(base, search_result={"hits": many[:1]}, num_highlights=1),
        "several": dict(base, search_result={"hits": many, "limit": 10}, num_highlights=1),
        "several_three_highlights": dict(base, search_result={"hits": many}, num_highlights=3),
        "hit_without_the_field": dict(base, search_result={"hits": no_field}, num_highlights=1),
        "shared_pointer": dict(base, search_result={"hits": shared}, num_highlights=1),
        "shared_pointer_three_highlights": dict(base, search_result={"hits": shared}, num_highlights=3),
        "no_ids": dict(base, search_result={"hits": [{k: v for k, v in h.items() if k != "_id"} for h in many[:2]]}, num_highlights=1, model_name="google/owlvit-base-patch16"),
    }


def _ours(case):
    result = copy.deepcopy(case["search_result"])
    r = cross_encoders.ReRankerOwl(model_name=case["model_name"], device="cpu", image_size=TARGET)
    r.rerank(query=case["query"], results=result, image_attributes=case["attributes"], num_highlights=case["num_highlights"])
    working = json.loads(json.dumps(result, default=float))
    rerank.cleanup_final_reranked_results(result)
    return {"working": working, "result": json.loads(json.dumps(result, default=float))}


def _blank_fresh_ids(result):
    for h in result["hits"]:
        if "_id" not in h and "_rerank_id" in h:
            h["_rerank_id"] = "<uuid>"
    return result


@pytest.fixture(scope="module")
def plumbing(tmp_path_factory):
    root = tmp_path_factory.mktemp("owl_plumbing")
    return root, _cases(root)


def test_plumbing_matches_the_reference(plumbing, monkeypatch):
    if not ref_shim.available():
        pytest.skip("the reference tree is not present on this machine")
    root, cases = plumbing
    p = root / "cases.json"
    p.write_text(json.dumps(cases))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), MARQO_AMD_HOST_ERRORS="0")
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "owl_ref_plumbing.py"), str(p)], capture_output=True, text=True, env=env, timeout=300)
    lines = [ln for ln in run.stdout.splitlines() if ln.startswith("{")]
    assert run.returncode == 0 and lines, run.stderr[-3000:]
    reference_side = json.loads(lines[-1])
    monkeypatch.setattr(cross_encoders, "load_owl_vit", lambda model_name, device: {"model": _Fake()})
    assert set(reference_side) == set(cases)
    for name, case in cases.items():
        ref, got = reference_side[name], _ours(case)
        assert "raises" not in ref, (name, ref)
        for stage in ("working", "result"):
            assert _blank_fresh_ids(got[stage]) == _blank_fresh_ids(ref[stage]), (name, stage)
    assert isinstance(reference_side["several_three_highlights"]["result"]["hits"][0]["_score"], list)
    assert len(reference_side["hit_without_the_field"]["result"]["hits"]) == 4


def test_plumbing_known_answers(plumbing, monkeypatch):
    """the same code without the reference tree: the best box per hit in the original image's pixels, descending order"""
    from PIL import Image
    _, cases = plumbing
    monkeypatch.setattr(cross_encoders, "load_owl_vit", lambda model_name, device: {"model": _Fake()})
    for name, k in (("several", 1), ("shared_pointer_three_highlights", 3)):
        case = cases[name]
        out = _ours(case)["working"]
        assert [h["_reranked_score"] for h in out["hits"]] == sorted((h["_reranked_score"] for h in out["hits"]), reverse=True)
        for h in out["hits"]:
            im = Image.open(h["image"])
            s, b = O.fake_detection(np.asarray(im.resize(TARGET).convert("RGB")))
            ts, tb, _ = O.topk_reference(s[None], b[None], k)
            fx, fy = im.size[0] / 240, im.size[1] / 240
            want = [[float(x0) * fx, float(y0) * fy, float(x1) * fx, float(y1) * fy] for x0, y0, x1, y1 in tb[0]]
            if k == 1:
                assert h["_reranked_score"] == float(ts[0, 0]) and h["_reranked_highlights"] == [{"image": want[0]}]
            else:     # two hits share this image or not: the frame merge shows a hit its image's rows once per hit that points at it
                copies = sum(1 for o in case["search_result"]["hits"] if o["image"] == h["image"])
                rows = sorted([(float(v), w) for v, w in zip(ts[0], want)] * copies, key=lambda r: -r[0])[:k]
                assert h["_reranked_score"] == [r[0] for r in rows] and h["_reranked_highlights"] == [{"image": r[1]} for r in rows]


# ---- the library's argument checks (no launch) ------------------------------------------------------------------------------------------------------
def test_argument_errors_are_reported_without_a_gpu():
    lib = L.load()
    fake = 256

    def refused(rc, msg):
        assert rc == -1 and msg in lib.mq_last_error(), (rc, lib.mq_last_error())

    refused(lib.mq_owl_merge_ln(fake, fake, fake, fake, fake, fake, None, 1, 10, 2052, 1e-5, None), b"mq_owl_merge_ln: W=2052")
    refused(lib.mq_owl_merge_ln(fake, fake, fake, fake, fake, None, None, 1, 10, 128, 1e-5, None), b"mq_owl_merge_ln: null pointer")
    refused(lib.mq_owl_merge_ln(fake, fake, fake, fake, fake, fake, None, 1, 8193, 128, 1e-5, None), b"T=8193")
    refused(lib.mq_owl_class_head(fake, fake, fake, None, 0, fake, 0.0, fake, 0.0, fake, fake, fake, 1, 9, 128, 64, 0, None), b"Q=0 must be in [1, 8]")
    refused(lib.mq_owl_class_head(fake, fake, None, None, 0, fake, 0.0, fake, 0.0, fake, fake, fake, 1, 9, 128, 64, 1, None), b"mq_owl_class_head: null pointer")
    refused(lib.mq_owl_box_head(fake, fake, fake, None, fake, 1, 9, 128, 240.0, 240.0, None), b"mq_owl_box_head: null pointer")
    refused(lib.mq_owl_topk(fake, fake, 1, 9, 0, fake, fake, fake, None), b"k=0 must be in [1, P=9]")
    refused(lib.mq_owl_topk(fake, fake, 1, 9, 10, fake, fake, fake, None), b"k=10 must be in [1, P=9]")
    refused(lib.mq_owl_topk(fake, fake, 1, 8192, 1, fake, fake, fake, None), b"P=8192")
    assert lib.mq_owl_topk(None, None, 0, 9, 1, None, None, None, None) == 0      # nothing to do

"""tests/dino_ref.py held against installed third-party code and hand-computed answers (no GPU): the restated DINO tower against
transformers.ViTModel (and the reference's own vision_transformer.py where that tree exists), the class-token attention budget against the float32
model of the kernel and its mutants, the map -> boxes step against grids written out by hand, the box pipeline against hand-computed cases."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import attention_ref as A
from tests import dino_ref as D
from marqo_amd.engine import synthetic
from marqo_amd.s2_inference.processing import image as I

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the tower ----------------------------------------------------------------------------------------------------------------------------------
def _hf_state_dict(sd, arch):
    W = arch.width
    out = {"embeddings.cls_token": sd["cls_token"], "embeddings.position_embeddings": sd["pos_embed"],
           "embeddings.patch_embeddings.projection.weight": sd["patch_embed.proj.weight"],
           "embeddings.patch_embeddings.projection.bias": sd["patch_embed.proj.bias"],
           "layernorm.weight": sd["norm.weight"], "layernorm.bias": sd["norm.bias"]}
    for i in range(arch.layers):
        p, h = f"blocks.{i}.", f"layers.{i}."
        for j, n in enumerate(("q_proj", "k_proj", "v_proj")):
            out[h + f"attention.{n}.weight"] = sd[p + "attn.qkv.weight"][j * W:(j + 1) * W]
            out[h + f"attention.{n}.bias"] = sd[p + "attn.qkv.bias"][j * W:(j + 1) * W]
        for a, b in (("attention.o_proj", "attn.proj"), ("layernorm_before", "norm1"), ("layernorm_after", "norm2"), ("mlp.fc1", "mlp.fc1"),
                     ("mlp.fc2", "mlp.fc2")):
            out[h + a + ".weight"], out[h + a + ".bias"] = sd[p + b + ".weight"], sd[p + b + ".bias"]
    return out


def test_restated_tower_agrees_with_transformers_vit():
    from transformers import ViTConfig, ViTModel
    arch = D.tiny_arch()
    sd = synthetic.random_dino_state_dict(arch, seed=5)
    cfg = ViTConfig(hidden_size=arch.width, num_hidden_layers=arch.layers, num_attention_heads=arch.heads, intermediate_size=arch.mlp_dim,
                    image_size=arch.image_size, patch_size=arch.patch_size, hidden_act="gelu", layer_norm_eps=arch.ln_eps, qkv_bias=True,
                    hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, attn_implementation="eager")
    model = ViTModel(cfg, add_pooling_layer=False).eval().double()
    missing = model.load_state_dict({k: v.double() for k, v in _hf_state_dict(sd, arch).items()}, strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    px = D.normalize_u8(D.synthetic_images_u8(3, arch.image_size, seed=1))
    with torch.no_grad():
        want = model(pixel_values=px, output_attentions=True).attentions[-1]
    got = D.last_selfattention(sd, arch, px, torch.float64)
    assert got.shape == want.shape == (3, arch.heads, arch.tokens, arch.tokens)
    # the installed eager attention takes its softmax in float32 whatever the model's dtype: 2**-24 relative on scores of a few units and on the
    # sum, ~1e-8 on probabilities of ~0.05 (measured 1.6e-8).  A structural slip (eps, GELU form, a bias, the scale) moves them by 1e-4 and more; the
    # reference's own module, in float64 throughout, is held to 1e-12 below
    assert float((got - want).abs().max()) < 1e-6
    assert torch.equal(D.cls_attention(sd, arch, D.synthetic_images_u8(3, arch.image_size, seed=1)), got[:, :, 0, 1:])


_REF_SCRIPT = r"""
import sys
sys.path.insert(0, sys.argv[1])
from oracle import ref_shim
ref_shim.install()
import torch
from functools import partial
try:
    from marqo.s2_inference.processing import vision_transformer as vt
except ImportError as e:            # the reference's own module (or what it imports) is not importable here: the one case that skips
    print(f"{type(e).__name__}: {e}", file=sys.stderr)
    sys.exit(77)
blob = torch.load(sys.argv[2])
a = blob["arch"]
m = vt.VisionTransformer(img_size=[a["image_size"]], patch_size=a["patch_size"], embed_dim=a["width"], depth=a["layers"], num_heads=a["heads"],
                         mlp_ratio=a["mlp_dim"] / a["width"], qkv_bias=True, norm_layer=partial(torch.nn.LayerNorm, eps=1e-6)).eval().double()
m.load_state_dict({k: v.double() for k, v in blob["sd"].items()}, strict=True)
with torch.no_grad():
    torch.save(m.get_last_selfattention(blob["px"]), sys.argv[3])
"""


@pytest.mark.skipif(not os.path.isdir("/root/reference/src/marqo"), reason="no reference tree on this machine")
def test_restated_tower_agrees_with_the_reference_module(tmp_path):
    """the reference's own vision_transformer.py, imported under oracle/ref_shim.py in a process of its own (the shim rebinds pydantic)"""
    arch = D.tiny_arch()
    sd = synthetic.random_dino_state_dict(arch, seed=6)
    px = D.normalize_u8(D.synthetic_images_u8(2, arch.image_size, seed=2))
    inp, outp = str(tmp_path / "in.pt"), str(tmp_path / "out.pt")
    torch.save({"arch": dict(image_size=arch.image_size, patch_size=arch.patch_size, width=arch.width, layers=arch.layers, heads=arch.heads,
                             mlp_dim=arch.mlp_dim), "sd": sd, "px": px}, inp)
    res = subprocess.run([sys.executable, "-c", _REF_SCRIPT, ROOT, inp, outp], capture_output=True, text=True, timeout=300)
    if res.returncode == 77:      # only the import of the reference's module itself; a failing shim or any other error fails the test below
        pytest.skip("the reference's vision_transformer.py does not import under the shim here: " + res.stderr.strip().splitlines()[-1])
    assert res.returncode == 0, res.stderr[-2000:]
    want = torch.load(outp)
    assert float((D.last_selfattention(sd, arch, px, torch.float64) - want).abs().max()) < 1e-12


def test_bf16_simulation_rounds_what_it_says():
    arch = D.tiny_arch()
    sd = D.bf16_weights(synthetic.random_dino_state_dict(arch, seed=7))
    u8 = D.synthetic_images_u8(2, arch.image_size, seed=3)
    ref, sim = D.cls_attention(sd, arch, u8, torch.float64), D.cls_attention(sd, arch, u8, torch.float32, bf16_sim=True)
    err = float((sim.double() - ref).abs().max())
    assert 1e-6 < err < 5e-3          # bf16 has 8 bits: visible, and small against probabilities of ~1 / 17
    assert float((D.cls_attention(sd, arch, u8, torch.float32).double() - ref).abs().max()) < 1e-6


# ---- mq_attention_cls_probs: reference, budget, model, mutants -------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["randn", "peaked", "readout"])
def test_cls_reference_is_row_zero_of_the_attention_reference(family):
    T, heads, nseq = 17, 6, 3
    qkv = A.make_qkv(family, [T] * nseq, heads, 64, seed=11)
    _, _, P = A.reference(qkv, [T] * nseq, heads, 64, A.MASK_NONE, keep_p=True)
    p, _, _ = D.cls_probs_reference(qkv, nseq, T, heads)
    for s in range(nseq):
        assert float((p[s] - P[s][:, 0, :]).abs().max()) < 1e-14


@pytest.mark.parametrize("family", ["randn", "peaked", "readout"])
@pytest.mark.parametrize("T", [2, 17, 197, 785])
def test_budget_holds_for_the_fp32_model_of_the_kernel(family, T):
    for heads, nseq in ((2, 3), (6, 1), (12, 1)):
        qkv = A.make_qkv(family, [T] * nseq, heads, 64, seed=T + heads)
        for key in (None, T - 1, 0):
            x = qkv if key is None else D.raise_key(qkv, nseq, T, heads, key)
            r = D.cls_probs_ratio(D.emulate_cls_probs(x, nseq, T, heads), x, nseq, T, heads)
            assert r <= 1.0, (family, T, heads, nseq, key, r)


@pytest.mark.parametrize("family", ["randn", "peaked", "readout"])
@pytest.mark.parametrize("T", [17, 197, 785])
def test_budget_sees_the_mutants_on_the_raised_key_case(family, T):
    """a last key that is dropped or counted twice, and a class key left out of the denominator, each leave the budget once that key's score stands out"""
    heads, nseq = 6, 2
    qkv = A.make_qkv(family, [T] * nseq, heads, 64, seed=3 * T)
    last, cls = D.raise_key(qkv, nseq, T, heads, T - 1), D.raise_key(qkv, nseq, T, heads, 0)
    for mutant, x in (("drop_last", last), ("dup_last", last), ("cls_out", cls)):
        assert D.cls_probs_ratio(D.emulate_cls_probs(x, nseq, T, heads), x, nseq, T, heads) <= 1.0
        r = D.cls_probs_ratio(D.emulate_cls_probs(x, nseq, T, heads, mutant), x, nseq, T, heads)
        assert r > 10.0, (family, T, mutant, r)


# ---- maps -> boxes: known answers ---------------------------------------------------------------------------------------------------------------------
def _grid(rows):
    return np.array([[c == "#" for c in r] for r in rows])


HAND_GRIDS = {
    # a blob inside a ring's hole: RETR_EXTERNAL reports the ring alone
    "nested": (["........", ".######.", ".#....#.", ".#.##.#.", ".#.##.#.", ".#....#.", ".######.", "........"], [(1, 1, 7, 7)]),
    # two blobs that touch only diagonally are one 8-connected component
    "diagonal": (["......", ".##...", ".##...", "...##.", "...##.", "......"], [(1, 1, 5, 5)]),
    # a blob on the frame, and a second one: raster order of the first cells
    "frame": (["##....", "##....", "......", "....#.", "......", "......"], [(0, 0, 2, 2), (4, 3, 5, 4)]),
    # a ring through diagonal links still closes its hole (the background inside is not 4-connected to the outside)
    "diamond": (["...#...", "..#.#..", ".#.#.#.", "..#.#..", "...#...", ".......", "......."], [(1, 0, 6, 5)]),
    "full": (["####", "####", "####", "####"], [(0, 0, 4, 4)]),
    "empty": (["....", "....", "....", "...."], []),
}


@pytest.mark.parametrize("name", sorted(HAND_GRIDS))
def test_external_boxes_known_answers(name):
    rows, want = HAND_GRIDS[name]
    assert D.external_boxes(_grid(rows)) == want
    assert D.propagate_boxes(_grid(rows)) == want


def test_label_propagation_model_equals_the_scipy_restatement_on_random_grids():
    rng = np.random.default_rng(0)
    for G in (4, 7, 14, 28, 32):
        for dens in (0.2, 0.4, 0.5, 0.6, 0.8):
            for _ in range(20):
                fg = rng.random((G, G)) < dens
                assert D.external_boxes(fg) == D.propagate_boxes(fg)


def test_constant_map_gives_threshold_zero_and_one_full_box():
    x = np.full((14, 14), 0.004, dtype=np.float32)
    boxes, t, tie = D.map_boxes(x)
    assert (t, tie, boxes) == (0, False, [(0, 0, 14, 14)])     # every pixel at 255: no bin splits two classes, max_val stays 0, and 255 > 0


def test_two_level_map_decides_otsu_without_ties():
    x = np.full((6, 6), 0.01, dtype=np.float32)
    x[1:3, 2:5] = 0.04                                   # levels trunc(0.25 * 255) = 63 and 255
    assert sorted(set(D.rescale_u8(x).reshape(-1).tolist())) == [63, 255]
    boxes, t, tie = D.map_boxes(x)
    assert (t, tie, boxes) == (63, False, [(2, 1, 5, 3)])   # the variance is the same for every threshold in 63 .. 254; the first strict maximum is 63


def test_otsu_threshold_is_the_upsampled_images():
    """integer counts: the histogram of the image upsampled by 16 is 256 times the grid's, and the scale 1 / N absorbs that exactly"""
    rng = np.random.default_rng(1)
    for _ in range(20):
        u8 = rng.integers(0, 256, (14, 14)).astype(np.uint8)
        assert D.otsu(u8, 16)[0] == D.otsu(u8, 1)[0] == D.otsu(np.kron(u8, np.ones((8, 8), dtype=np.uint8)), 2)[0]


def test_mean_over_heads_is_numpys():
    p = D.smooth_maps(6, 14, 0) * np.where(np.arange(6)[:, None, None] % 2 == 0, 1, -1).astype(np.float32)
    assert np.array_equal(D.maps_from_probs(p, 0)[0], np.abs(p).mean(0))
    maps = D.maps_from_probs(p, 1)
    assert len(maps) == 6 and float(maps[1].max()) == 0.0 and np.array_equal(maps[0], p[0])


def test_seeded_smooth_maps_stay_under_the_tie_cap():
    """the GPU test may leave out maps whose Otsu curve ties within double rounding, at most 2 % of them: the seeds it uses stay under that here"""
    total = ties = 0
    for G in (4, 14, 28):
        for seed in range(12):
            for mode in (0, 1):
                for _, _, tie in D.probs_boxes(D.smooth_maps(6, G, seed), mode):
                    total, ties = total + 1, ties + bool(tie)
    assert total == 3 * 12 * 7 and ties <= 0.02 * total, (ties, total)


# ---- the box pipeline -----------------------------------------------------------------------------------------------------------------------------
def test_box_pipeline_hand_cases():
    # areas on the 224 px maps: 112 x 112 = 12544 (kept), 48 x 48 = 2304 (< 3600: filtered), 224 x 48 (aspect 4.67: filtered), 64 x 64 = 4096 (kept)
    boxes = [(0, 0, 112, 112), (16, 16, 64, 64), (0, 176, 224, 224), (128, 128, 192, 192)]
    want = [(0.0, 0.0, 112.0, 112.0), (128.0, 128.0, 192.0, 192.0)]
    assert D.box_pipeline(boxes) == want
    got, scores = I.box_pipeline(boxes, I.calc_area(boxes, (240, 240)), (240, 240))
    assert [tuple(float(v) for v in b) for b in got] == want
    # the 240-vs-224 quirk: a box that covers the whole 224 px map scores 224^2 / 240^2, not 1, and is not stretched to 240
    assert I.calc_area([(0, 0, 224, 224)], (240, 240)) == [224 * 224 / (240 * 240.0)]
    assert D.box_pipeline([(0, 0, 224, 224)]) == [(0.0, 0.0, 224.0, 224.0)]


def test_nms_keeps_the_larger_of_two_overlapping_boxes_and_ties_keep_input_order():
    a, b, c = (0, 0, 160, 160), (16, 16, 160, 160), (0, 0, 96, 96)      # IoU(a, b) = 144^2 / 160^2 = 0.81 > 0.6; IoU(a, c) = 0.36
    assert D.box_pipeline([b, a, c]) == [tuple(map(float, a)), tuple(map(float, c))]
    assert I.nms([b, a, c], I.calc_area([b, a, c], (240, 240)), 0.6) == [1, 2]
    assert I.nms([a, a], [0.5, 0.5], 0.6) == [0] and I.nms([c, (100, 100, 200, 200)], [0.3, 0.3], 0.6) == [0, 1]


def test_keep_top_k_never_truncates():
    """_keep_top_k only acts when top_k EXCEEDS the number of boxes, where _keep_topk returns its input: 12 disjoint boxes all survive top_k = 10"""
    boxes = [(x, y, x + 64, y + 64) for y in (0, 72, 144) for x in (0, 72, 144)] + [(0, 0, 224, 100), (0, 110, 224, 224), (100, 0, 224, 224)]
    assert len(D.box_pipeline(boxes, iou=1.0)) == 12
    got, _ = I.box_pipeline(boxes, I.calc_area(boxes, (240, 240)), (240, 240), iou_thresh=1.0, top_k=10)
    assert len(got) == 12
    assert I._keep_topk(list(range(12)), k=10) == list(range(10)) and I._keep_topk([1, 2], k=0) == []


def test_small_box_replacement_and_clipping():
    assert I.replace_small_boxes([(10, 10, 30, 30)], min_area=3600, new_size=(100, 100)) == [(-30.0, -30.0, 70.0, 70.0)]
    assert [tuple(float(v) for v in b) for b in I.clip_boxes([(-30.0, -30.0, 70.0, 300.0)], 0, 0, 240, 240)] == [(0.0, 0.0, 70.0, 240.0)]
    assert I.filter_boxes([(0, 0, 61, 60), (0, 0, 60, 60), (0, 0, 40, 160)], min_area=3600) == [0]


def test_dino_methods_dispatch_and_detectors_stay_refused(monkeypatch, tmp_path):
    from PIL import Image
    from marqo_amd.s2_inference.errors import ChunkerError
    img = Image.new("RGB", (32, 32))
    for m in ("frcnn", "yolox", "fastercnn", "marqo-yolo"):
        with pytest.raises(ChunkerError, match="needs a detector model"):
            I.chunk_image(img, "cuda", m)
    monkeypatch.delenv(I.DINO_CHECKPOINT_ENV, raising=False)
    monkeypatch.setattr(torch.hub, "get_dir", lambda: str(tmp_path))
    for m in ("dino-v1", "dino-v2", "dino/v1", "dino/v2"):
        with pytest.raises(ChunkerError, match="MARQO_DINO_CHECKPOINT.*dino_deitsmall16_pretrain.pth"):
            I.chunk_image(img, "cuda", m)
    with pytest.raises(ValueError):
        I.chunk_images_to_tensors([img], None, "dino-v2")


def test_new_entry_points_report_argument_errors_without_a_gpu():
    from marqo_amd import _lib as L
    lib, fake = L.load(), 256

    def refused(rc, msg):
        assert rc == -1 and msg in lib.mq_last_error(), lib.mq_last_error()

    refused(lib.mq_attention_cls_probs(None, fake, 1, 17, 128, 2, None), b"attention_cls_probs: null pointer")
    refused(lib.mq_attention_cls_probs(fake, fake, 1, 1, 128, 2, None), b"T=1 unsupported")
    refused(lib.mq_attention_cls_probs(fake, fake, 1, 17, 192, 2, None), b"W=192 must be heads=2 * 64")
    refused(lib.mq_attn_boxes(fake, 1, 6, 33, 0, fake, fake, 4, None), b"G=33 unsupported")
    refused(lib.mq_attn_boxes(fake, 1, 6, 14, 0, fake, fake, 0, None), b"max_boxes=0")
    refused(lib.mq_attn_boxes(fake, 1, 6, 14, 2, fake, fake, 4, None), b"mode=2")
    refused(lib.mq_attn_boxes(fake, 1, 6, 14, 0, None, fake, 4, None), b"attn_boxes: null pointer")
    assert lib.mq_attn_boxes(fake, 0, 6, 14, 0, fake, fake, 4, None) == 0 and lib.mq_attention_cls_probs(fake, fake, 0, 17, 128, 2, None) == 0


def test_two_group_checkpoint_gives_maps_with_a_gap_at_the_threshold():
    """the synthetic checkpoint of the tower's box test: every map's boxes are those of the image's own bright-patch mask, and the gap between the two
    groups of cells is an order of magnitude above what the bf16-operand simulation moves a cell by"""
    arch = D.tiny_arch()
    sd = D.bf16_weights(D.two_group_state_dict(arch, seed=1))
    u8, masks = D.two_group_images_u8(4, arch.image_size, arch.patch_size, seed=3)
    ref = D.cls_attention(sd, arch, u8, torch.float64)
    sim = D.cls_attention(sd, arch, u8, torch.float32, bf16_sim=True)
    bound = 4.0 * float((sim.double() - ref).abs().max())
    G = arch.image_size // arch.patch_size
    for i in range(4):
        for mode in (0, 1):
            pr, ps = (t[i].reshape(arch.heads, G, G).float().numpy() for t in (ref, sim))
            for (br, t, tie), (bs, _, _), x in zip(D.probs_boxes(pr, mode), D.probs_boxes(ps, mode), D.maps_from_probs(pr, mode)):
                r = x.astype(np.float64) / float(x.max()) * 255.0
                half_gap = (r[r >= t + 1].min() - r[r < t + 1].max()) / 2
                assert not tie and br == bs == D.external_boxes(masks[i])
                assert half_gap > 10 * 255.0 * bound / float(x.max())

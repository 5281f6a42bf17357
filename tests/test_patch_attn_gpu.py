"""csrc/patch_attn.hip, engine/dino.py and the 'dino-v1' / 'dino-v2' patch methods on the GPU, against tests/dino_ref.py.

mq_attention_cls_probs: row 0 of attention_ref.reference(..., keep_p=True), keys 1 .. T - 1, inside the budget dino_ref derives from the kernel's arithmetic
(no tuned constant; tests/test_dino_ref_host.py shows on the CPU that the float32 model of the kernel stays inside it and that a dropped or doubled
last key and a class key left out of the denominator do not).
mq_attn_boxes: exact integer equality with the SciPy restatement, box lists in order and counts.
DinoTower: probabilities against the float64 reference on the bf16-rounded weights, inside MARGIN x the error the reference's own bf16-operand
simulation shows on the same inputs; boxes exactly those of the restated box step on the tower's own probabilities, and those of the reference's
probabilities wherever the threshold margin exceeds the probability bound.

The figures measured on an MI355X are recorded in DESIGN.md §5 (attention-based patching)."""
import numpy as np
import pytest
import torch

from tests import attention_ref as A
from tests import dino_ref as D

pytestmark = pytest.mark.gpu

MARGIN = 4.0    # accumulation order: the engine's GEMMs and LayerNorms sum in another order than the simulation, and two independent rounding
#                 histories of the same size differ by up to twice either one's distance from the exact value; x 2 again for the maximum over a few
#                 thousand probabilities falling on another element


@pytest.fixture(scope="module")
def lib():
    from marqo_amd import _lib as L
    return L.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _check(lib, rc, what):
    from marqo_amd import _lib as L
    L.check(rc, what)
    torch.cuda.synchronize()


def _cls_probs(lib, qkv, nseq, T, heads):
    """-> fp32 [nseq, heads, T - 1] on the CPU; the buffer carries a guard row that must come back untouched"""
    n = nseq * heads * (T - 1)
    out = torch.full((n + 64,), float("nan"), dtype=torch.float32, device="cuda")
    d = qkv.cuda().contiguous()
    _check(lib, lib.mq_attention_cls_probs(d.data_ptr(), out.data_ptr(), nseq, T, heads * 64, heads, _stream()), "mq_attention_cls_probs")
    assert bool(torch.isnan(out[n:]).all()), "wrote past [nseq, heads, T - 1]"
    return out[:n].reshape(nseq, heads, T - 1).cpu()


# ---- mq_attention_cls_probs -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nseq", [1, 3])
@pytest.mark.parametrize("heads", [2, 6, 12])
@pytest.mark.parametrize("T", [2, 17, 197, 785])
@pytest.mark.parametrize("family", ["randn", "peaked", "readout"])
def test_cls_probs_against_the_attention_reference(lib, monkeypatch, family, T, heads, nseq):
    monkeypatch.setattr(A, "KEEP_P_ROWS", 1024)      # the reference hands its probabilities out for sequences up to this long
    qkv = A.make_qkv(family, [T] * nseq, heads, 64, seed=100 + T + heads + nseq)
    got = _cls_probs(lib, qkv, nseq, T, heads)
    _, _, P = A.reference(qkv.cuda(), [T] * nseq, heads, 64, A.MASK_NONE, keep_p=True)
    want = torch.stack([P[s][:, 0, :] for s in range(nseq)]).cpu()                        # [nseq, heads, T], float64
    p, Aq, t = D.cls_probs_reference(qkv, nseq, T, heads)
    assert float((p - want).abs().max()) < 1e-13                                         # the budget's reference IS the attention reference's row 0
    ratio = float(((got.double() - want[..., 1:]).abs() / D.cls_probs_budget(p, Aq, t)[..., 1:]).max())
    print(f"cls_probs {family} T={T} heads={heads} nseq={nseq}: worst |err| / budget = {ratio:.3f}")
    assert torch.isfinite(got).all() and ratio <= 1.0


@pytest.mark.parametrize("key", ["class", "last"])
@pytest.mark.parametrize("T", [17, 197, 785])
def test_cls_probs_with_one_key_raised(lib, T, key):
    """the case on which the host test shows the budget catching a dropped / doubled last key and a class key outside the denominator"""
    heads, nseq = 6, 2
    qkv = D.raise_key(A.make_qkv("randn", [T] * nseq, heads, 64, seed=3 * T), nseq, T, heads, 0 if key == "class" else T - 1)
    got = _cls_probs(lib, qkv, nseq, T, heads)
    ratio = D.cls_probs_ratio(got, qkv, nseq, T, heads)
    p, _, _ = D.cls_probs_reference(qkv, nseq, T, heads)
    print(f"cls_probs raised {key} key T={T}: worst |err| / budget = {ratio:.3f}, raised key's share {float(p[..., 0 if key == 'class' else T - 1].min()):.3f}")
    assert ratio <= 1.0
    assert float(p[..., 0 if key == "class" else T - 1].min()) > 0.2      # the raised key does stand out


# ---- mq_attn_boxes ------------------------------------------------------------------------------------------------------------------------------------
def _attn_boxes(lib, probs, mode, max_boxes=None):
    """probs float32 ndarray [n, heads, G, G] -> per image, per map: list of (x1, y1, x2, y2) in grid cells, and the counts"""
    n, heads, G, _ = probs.shape
    maps = 1 if mode == 0 else heads
    mb = max_boxes or ((G + 1) // 2) ** 2
    d = torch.from_numpy(np.ascontiguousarray(probs, dtype=np.float32)).cuda()
    boxes = torch.full((n * maps * mb * 4 + 16,), -7, dtype=torch.int32, device="cuda")
    counts = torch.full((n * maps + 16,), -7, dtype=torch.int32, device="cuda")
    _check(lib, lib.mq_attn_boxes(d.data_ptr(), n, heads, G, mode, boxes.data_ptr(), counts.data_ptr(), mb, _stream()), "mq_attn_boxes")
    assert bool((boxes[n * maps * mb * 4:] == -7).all()) and bool((counts[n * maps:] == -7).all()), "wrote past the outputs"
    b, c = boxes[:n * maps * mb * 4].reshape(n, maps, mb, 4).cpu().numpy(), counts[:n * maps].reshape(n, maps).cpu().numpy()
    return [[[tuple(int(v) for v in b[i, m, k]) for k in range(min(int(c[i, m]), mb))] for m in range(maps)] for i in range(n)], c


def _hand_probs(rows, heads):
    g = np.array([[0.04 if ch == "#" else 0.01 for ch in r] for r in rows], dtype=np.float32)
    return np.stack([g] * heads)


HAND = {   # the grids of tests/test_dino_ref_host.py
    "nested": (["........", ".######.", ".#....#.", ".#.##.#.", ".#.##.#.", ".#....#.", ".######.", "........"], [(1, 1, 7, 7)]),
    "diagonal": (["......", ".##...", ".##...", "...##.", "...##.", "......"], [(1, 1, 5, 5)]),
    "frame": (["##....", "##....", "......", "....#.", "......", "......"], [(0, 0, 2, 2), (4, 3, 5, 4)]),
    "diamond": (["...#...", "..#.#..", ".#.#.#.", "..#.#..", "...#...", ".......", "......."], [(1, 0, 6, 5)]),
    "constant": (["####", "####", "####", "####"], [(0, 0, 4, 4)]),
}


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", sorted(HAND))
def test_attn_boxes_hand_grids(lib, name, mode):
    rows, want = HAND[name]
    p = _hand_probs(rows, 3)[None]
    got, counts = _attn_boxes(lib, p, mode)
    assert [r[0] for r in D.probs_boxes(p[0], mode)] == [want] * (1 if mode == 0 else 3)      # the restatement gives the hand answer ...
    assert got[0] == [want] * (1 if mode == 0 else 3) and counts.tolist() == [[len(want)] * (1 if mode == 0 else 3)]   # ... and so does the kernel


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("G", [4, 14, 28])
def test_attn_boxes_smooth_random_maps(lib, G, mode):
    heads, seeds = 6, range(12)
    p = np.stack([D.smooth_maps(heads, G, s) for s in seeds])
    if mode == 1:
        p[::2, 1, :2, :2] *= -1.0    # a corner of negatives: zeroed in 'pos' mode
    got, counts = _attn_boxes(lib, p, mode)
    total = ties = 0
    for i in range(len(seeds)):
        want = D.probs_boxes(p[i], mode)
        for m, (boxes, t, tie) in enumerate(want):
            total += 1
            if tie:
                ties += 1
                continue
            assert got[i][m] == boxes and int(counts[i, m]) == len(boxes), (G, mode, i, m, t, got[i][m], boxes)
    print(f"attn_boxes G={G} mode={mode}: {total} maps, {ties} left out as Otsu ties")
    assert ties <= 0.02 * total


def test_attn_boxes_counts_past_max_boxes(lib):
    rows = ["#.#.#.", "......", "#.#.#.", "......", "#.#.#.", "......"]        # 9 isolated cells
    p = _hand_probs(rows, 2)[None]
    got, counts = _attn_boxes(lib, p, 0, max_boxes=4)
    assert counts.tolist() == [[9]] and got[0][0] == [(0, 0, 1, 1), (2, 0, 3, 1), (4, 0, 5, 1), (0, 2, 1, 3)]


@pytest.mark.parametrize("mode", [0, 1])
def test_attn_boxes_map_without_a_positive_cell(lib, mode):
    """maximum 0: the rescale is 0 / 0, which the kernel maps to level 0 everywhere -> threshold 0, no foreground, no box (include/marqo_hip.h).  Image 1
    is an ordinary map, to see that the empty one disturbs nothing beside it."""
    G, heads = 6, 3
    p = np.zeros((2, heads, G, G), dtype=np.float32)
    if mode == 1:
        p[0, 1] = -0.01                                 # 'pos' mode zeroes negatives: still nothing positive
    p[1] = _hand_probs(HAND["diagonal"][0], heads)
    got, counts = _attn_boxes(lib, p, mode)
    maps = 1 if mode == 0 else heads
    assert got[0] == [[]] * maps and got[1] == [HAND["diagonal"][1]] * maps
    assert counts.tolist() == [[0] * maps, [1] * maps]


# ---- DinoTower ------------------------------------------------------------------------------------------------------------------------------------------
def _arch(shape):
    from marqo_amd.engine import archs
    return D.tiny_arch() if shape == "tiny" else archs.dino_arch("vit_small", 16)


_tower_cache = {}
KINDS = ("random", "two_group")   # random weights drive every block at full strength (flat maps); the two-group checkpoint gives maps with a gap at the threshold


def _tower_case(shape, kind):
    """(arch, tower, images, engine probabilities, float64 reference, probability bound, bright-patch masks or None) — computed once per case"""
    if (shape, kind) not in _tower_cache:
        from marqo_amd.engine import dino, synthetic
        arch = _arch(shape)
        n = 4 if shape == "tiny" else 2
        if kind == "random":
            sd, u8, masks = synthetic.random_dino_state_dict(arch, seed=1), D.synthetic_images_u8(n, arch.image_size, seed=3), None
        else:
            sd = D.two_group_state_dict(arch, seed=1)
            u8, masks = D.two_group_images_u8(n, arch.image_size, arch.patch_size, seed=3)
        tower = dino.DinoTower(arch, sd, "cuda")
        got = tower.probs(u8.cuda())
        torch.cuda.synchronize()
        rsd = D.bf16_weights(sd)
        ref = D.cls_attention(rsd, arch, u8, torch.float64)
        sim = D.cls_attention(rsd, arch, u8, torch.float32, bf16_sim=True)
        bound = MARGIN * float((sim.double() - ref).abs().max())
        _tower_cache[(shape, kind)] = (arch, tower, u8, got, ref, bound, masks)
    return _tower_cache[(shape, kind)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", ["tiny", "vit_small"])
def test_dino_tower_probabilities(shape, kind):
    arch, tower, u8, got, ref, bound, _ = _tower_case(shape, kind)
    assert got.shape == ref.shape == (u8.shape[0], arch.heads, arch.tokens - 1)
    err = float((got.cpu().double() - ref).abs().max())
    print(f"DinoTower {shape} {kind}: max |p - reference| = {err:.3e}, bound = {MARGIN} x {bound / MARGIN:.3e} (reference vs its bf16 simulation), "
          f"max p = {float(ref.max()):.4f}")
    assert err <= bound
    assert float((got.sum(-1) - 1).max()) <= 1e-6 and float(got.min()) >= 0     # the class key's share is missing from each row, nothing else


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", ["tiny", "vit_small"])
def test_dino_tower_boxes_are_the_box_step_of_its_probabilities(shape, kind, mode):
    arch, tower, u8, got, _, _, _ = _tower_case(shape, kind)
    G, P = tower.grid, arch.patch_size
    boxes, counts = tower.boxes(u8.cuda(), mode)
    torch.cuda.synchronize()
    boxes, counts, p = boxes.cpu().numpy(), counts.cpu().numpy(), got.cpu().numpy().reshape(-1, arch.heads, G, G)
    total = ties = 0
    for i in range(u8.shape[0]):
        for m, (want, t, tie) in enumerate(D.probs_boxes(p[i], mode, P)):
            total += 1
            if tie:
                ties += 1
                continue
            assert int(counts[i, m]) == len(want)
            assert [tuple(int(v) for v in boxes[i, m, k]) for k in range(len(want))] == [tuple(P * v for v in b) for b in want]
    print(f"DinoTower {shape} {kind} mode {mode}: {total} maps, {ties} left out as Otsu ties")
    assert ties <= 0.02 * total       # the same cap as for the smooth maps: with at most 12 maps here, no tie at all


def _decided(shape, kind, mode):
    """per (image, map): (decided, engine boxes == reference boxes, reference boxes).  A map is decided when no cell can change side of the threshold
    under the probability bound: half the gap, in uint8 levels before truncation, between the lowest foreground cell and the highest background cell
    exceeds what the bound moves x / max * 255 by.  (Otsu's first strict maximum always sits ON an occupied level, so the distance from the threshold to
    the nearest level is below one level for every map; the half gap is what the bound needs to guarantee equal masks.)"""
    arch, tower, u8, got, ref, bound, _ = _tower_case(shape, kind)
    G = tower.grid
    pe, pr = got.cpu().numpy().reshape(-1, arch.heads, G, G), ref.float().numpy().reshape(-1, arch.heads, G, G)
    out = []
    for i in range(u8.shape[0]):
        for (be, _, _), (br, t, _), x in zip(D.probs_boxes(pe[i], mode), D.probs_boxes(pr[i], mode), D.maps_from_probs(pr[i], mode)):
            r = x.astype(np.float64) / float(x.max()) * 255.0
            lo, hi = r[r < t + 1], r[r >= t + 1]
            half_gap = (hi.min() - lo.max()) / 2 if len(lo) and len(hi) else 255.0
            moved = 255.0 * bound / float(x.max()) * (1 + (t + 1) / 255.0)       # x and max(x) each move by the bound
            out.append((half_gap > moved, be == br, br, i))
    return out


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", ["tiny", "vit_small"])
def test_dino_tower_boxes_equal_the_references_where_the_margin_decides(shape, kind, mode):
    res = _decided(shape, kind, mode)
    print(f"DinoTower {shape} {kind} mode {mode}: {len(res)} maps, {sum(r[0] for r in res)} decided, {sum(r[1] for r in res)} with the reference's boxes")
    assert all(same for decided, same, _, _ in res if decided)
    masks = _tower_case(shape, kind)[6]
    if masks is not None:       # the two-group checkpoint attends to the bright patches: the boxes are those of the images' own masks
        assert all(br == D.external_boxes(masks[i]) for _, _, br, i in res)


@pytest.mark.parametrize("shape", ["tiny", "vit_small"])
def test_dino_tower_undecided_share_is_capped(shape):
    """At most 10 % of the maps may be left out of the comparison above.  Held on the two-group checkpoint, whose maps, like a trained DINO's, have a gap
    at the threshold (half gaps of 112 - 121 levels against 6 - 10 moved by the bound).  On random weights the cap cannot be met by any bf16 engine, nor
    by the reference's own bf16 simulation: the maps are nearly flat (ViT-S/16: max p 0.0126 against a mean of 0.0051), 196 cells over ~255 levels sit
    about one level apart, and the bound (4 x 3.6e-5, i.e. 4 x 0.5 % of the maximum) moves a cell by 4 - 11 levels — 14 of 14 maps undecided there
    (printed below; the boxes still agree with the reference's on most of them)."""
    for kind in KINDS:
        res = _decided(shape, kind, 0) + _decided(shape, kind, 1)
        print(f"DinoTower {shape} {kind}: {sum(not r[0] for r in res)} of {len(res)} maps undecided, {sum(r[1] for r in res)} with the reference's boxes")
    res = _decided(shape, "two_group", 0) + _decided(shape, "two_group", 1)
    left_out = sum(not r[0] for r in res)
    assert left_out <= 0.10 * len(res), f"{left_out} of {len(res)} maps undecided"


# ---- chunk_image end to end ---------------------------------------------------------------------------------------------------------------------------
def test_chunk_image_dino_end_to_end(tmp_path, monkeypatch):
    from PIL import Image
    from marqo_amd.engine import archs, synthetic
    from marqo_amd.s2_inference.processing import image as I
    from marqo_amd.s2_inference.s2_inference import _create_model_cache_key, get_available_models
    arch = archs.dino_arch("vit_small", 16)
    ckpt = str(tmp_path / "dino_deitsmall16_pretrain.pth")
    torch.save(synthetic.random_dino_state_dict(arch, seed=2), ckpt)
    monkeypatch.setenv(I.DINO_CHECKPOINT_ENV, ckpt)
    key = _create_model_cache_key("vit_small", "cuda")
    get_available_models().pop(key, None)
    loads = []
    real_load = I._load_DINO_model
    monkeypatch.setattr(I, "_load_DINO_model", lambda *a, **k: (loads.append(a), real_load(*a, **k))[1])
    pil = Image.fromarray(D.synthetic_images_u8(1, 200, seed=9)[0].numpy()[:150], "RGB")         # 200 x 150: neither square nor the working size
    try:
        for method, mode in (("dino-v2", 1), ("dino-v1", 0)):
            patches, bboxes = I.chunk_image(pil, "cuda", method)
            tower = get_available_models()[key]["model"][0]
            work = pil.convert("RGB").resize((240, 240))                                          # Pillow's own resamplers: the engine's are bit-exact
            u8 = torch.from_numpy(np.asarray(work.resize((224, 224), Image.BILINEAR))).unsqueeze(0)
            boxes, counts = tower.boxes(u8.cuda(), mode)
            boxes, counts = boxes[0].cpu().numpy(), counts[0].cpu().numpy()
            raw = [tuple(int(v) for v in boxes[m, k]) for m in range(boxes.shape[0]) for k in range(int(counts[m]))]
            want = [(0, 0, 240, 240)] + D.box_pipeline(raw)
            assert patches[0].size == (240, 240) and np.array_equal(np.asarray(patches[0]), np.asarray(work))
            assert len(patches) == len(bboxes) == len(want) and len(raw) >= 1
            for bb, w, patch in zip(bboxes, want, patches):
                assert bb == pytest.approx([w[0] * 200 / 240, w[1] * 150 / 240, w[2] * 200 / 240, w[3] * 150 / 240], abs=1e-9)
                assert 0 <= bb[0] <= bb[2] <= 200 and 0 <= bb[1] <= bb[3] <= 150
                assert patch.size == (int(w[2] - w[0]), int(w[3] - w[1]))
            print(f"chunk_image {method}: {len(raw)} raw boxes -> {len(want) - 1} patches besides the whole image")
        assert len(loads) == 1                                                                    # the second call found the model in the cache
    finally:
        get_available_models().pop(key, None)

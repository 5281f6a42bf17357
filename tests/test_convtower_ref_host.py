"""tests/convtower_ref.py on the CPU: what tests/test_convtower_forms_gpu.py rests on.

1. The exact references are the restatements the project already trusts: with the matrices left un-rounded, convnext_exact agrees with _head(_torch_trunk)
   and resnet_exact with _torch_resnet (the fp32 torch restatements the full-size GPU tests compare with, themselves pinned to transformers' ConvNextModel
   and composed from torch.nn.functional as OpenAI's ModifiedResNet is) on every configuration, to fp32 round-off.  So the load-time folds, the paddings
   and the dataflow of the reference are those of the module; rounding the matrices to bf16 is one switch on top (convnext_operands / resnet_operands).
2. The yardstick is usable on every input the GPU file runs: the model differs from `exact` in every output row and in every row of the last stage's
   stream of every configuration and batch size — no ZeroYardstick — and measures 1.0 against itself.
3. The bar sees the defects this suite is there for.  Each is injected into `model`, one at a time, on the GPU file's own inputs (n = 3), and
   max(row_ratio of the output rows, row_ratio of the last stage's stream) — the two things the GPU file asserts — must exceed MARGIN = 4.
   Measured, smallest .. largest over the configurations (output rows | stream rows; 1 where the defect lies behind the stream):
     ConvNeXt  gamma_dropped (the block in the middle of the walk)   62 .. 105 | 68 .. 101
               dw_border_replicated (stage 0 only)                   21 .. 75 | 17 .. 71
               ds_taps_xy                                            156 .. 263 | 186 .. 306
               pool_positions (the pool leaves the last one out)     93 .. 200 | 1
               eps_swapped (1e-5 <-> 1e-6), the dim-stem case        66 | 63          every other case: NOT SEEN, 1.08 .. 1.73 | 1.02 .. 1.57
               pool_divisor (HW + 1)                                 NOT SEEN: 0.99 .. 1.02 | 1
               quick_gelu                                            NOT SEEN: 1.56 .. 2.80 | 1.30 .. 1.72
     ResNet    relu_before_add                                       983 .. 2070 | 735 .. 1130
               identity_not_pooled                                   62 .. 250 | 107 .. 407
               avgpool_divisor (3)                                   440 .. 1300 | 383 .. 623
               pad_nan (widths 16, 80; width 64 pads nothing)        inf | inf
               no_positions                                          17 .. 71 | 1
               q_unscaled                                            16 .. 60 | 1
               images_swapped                                        17 .. 38 | 1
               ds_by_padded_width (width 16; the walk as it was)     126 .. 222 | 119 .. 212          widths 64, 80: the same walk, 1 | 1
               pad_not_zero (finite)                                 NOT SEEN: 1 | 1 exactly
   What this test cannot see, and why (each asserted below, so that this stays true):
     eps_swapped on trained-like weights.  Every LayerNorm of those towers sees rows of variance 0.1 .. 10, where 1e-5 against 1e-6 moves rstd by 5e-6 / variance
       relative: three orders of magnitude below one bf16 rounding (2^-9) of the same value, in ANY bf16 walk.  The dim-stem case (convtower_ref.convnext_cases:
       the stem convolution times 2^-10, so the stem LayerNorm's rows have a variance of the order of eps) is there to show it, and does.
     pool_divisor.  The pooled mean goes straight into head.norm, and a LayerNorm is invariant under a scale of its row (up to eps): a wrong divisor alone
       cannot reach the output.  A wrong SET of positions can, and does (pool_positions).
     quick_gelu.  x sigmoid(1.702 x) and the erf GELU differ by at most 0.02, 1 % of a unit pre-activation.  Behind fc2 and a layer scale of 0.05 .. 0.5 that is
       the size of the bf16 rounding of the stream it is added to, and in the mlp head of the fp32 output's inherited rounding: 1.3 .. 2.8 yardsticks, inside
       the factor allowed between two rounding histories.  Larger layer scales do not help (x 8: 3.98 — the stream grows with them).  The activation is held
       to a per-element budget where it is computed, in the GEMM epilogues (tests/test_gemm_parity_gpu.py).
     pad_not_zero with FINITE garbage.  A padded channel only ever meets weight columns that the loader wrote as zeros (conv1, conv2, conv3 and the
       downsample read it as K; the residual add happens at the un-padded width 4 P), so a finite value there is multiplied away exactly.  That is the
       design, not a blind spot of the measure: only a non-finite value survives (0 x NaN).  The GPU file therefore fills the workspace with 0xFF bytes
       (bf16 and fp32 NaN): a padded channel the walk reads without having written it comes back as the pad_nan case.
   The seeded ResNet checkpoints carry q_proj and k_proj weights times 4 (convtower_ref.resnet_sd): with the seeded ones the scores are a few hundredths and the
   softmax uniform at any temperature — q_unscaled measured 1.3 .. 5.5 there.
"""
import pytest
import torch

from tests import convtower_ref as T
from tests.convtower_ref import MARGIN, ZeroYardstick, row_ratio

N = 3       # the batch the GPU file runs (its n = 1 is a prefix of it: images do not see each other)

_CNX = {c[0]: c for c in T.convnext_cases()}
_RN = {c[0]: c for c in T.resnet_cases()}
_cache = {}


def _cnx(cid, n=N):
    key = ("cnx", cid, n)
    if key not in _cache:
        _, arch, b2, seed, stem = _CNX[cid]
        sd = T.convnext_sd(arch, b2, seed, stem)
        ops = T.convnext_operands(arch, sd)
        px = T.normalise(T.images(n, arch.image_size, seed))
        _cache[key] = (arch, sd, ops, px, T.convnext_exact(arch, ops, px), T.convnext_model(arch, ops, px))
    return _cache[key]


def _rn(cid, n=N):
    key = ("rn", cid, n)
    if key not in _cache:
        _, arch, seed = _RN[cid]
        sd = T.resnet_sd(arch, seed)
        ops = T.resnet_operands(arch, sd)
        px = T.normalise(T.images(n, arch.image_size, seed))
        _cache[key] = (arch, sd, ops, px, T.resnet_exact(arch, ops, px), T.resnet_model(arch, ops, px))
    return _cache[key]


# fp32 restatements against float64: 6e-8 per operation; the longest sums run over K = 4 C = 2048 (ConvNeXt fc2) and K = 9 P = 5760 (ResNet conv2 at
# width 80) products, whose fp32 accumulation errs by about sqrt(K) 6e-8 = 3e-6 .. 5e-6 of the row's scale, a dozen such layers deep
PIN = 2e-5


def _pin(name, got, want):
    scale = max(1.0, float(want.abs().max()))
    err = float((got - want.double()).abs().max())
    print(f"CONVTOWER_PIN {name}: max |exact - fp32 restatement| = {err:.3e} (scale {scale:.2f}, bound {PIN * scale:.3e})")
    assert err <= PIN * scale


@pytest.mark.parametrize("cid", list(_CNX))
def test_convnext_exact_is_the_fp32_restatement(cid):
    _, arch, b2, seed, stem = _CNX[cid]
    sd = T.convnext_sd(arch, b2, seed, stem)
    px = T.normalise(T.images(2, arch.image_size, seed))
    with torch.no_grad():
        want = T._head(sd, arch, T._torch_trunk(sd, arch, px))
    got, _ = T.convnext_exact(arch, T.convnext_operands(arch, sd, round_matrices=False), px)
    _pin(cid, got, want)


@pytest.mark.parametrize("cid", list(_RN))
def test_resnet_exact_is_the_fp32_restatement(cid):
    _, arch, seed = _RN[cid]
    sd = T.resnet_sd(arch, seed)
    px = T.normalise(T.images(2, arch.image_size, seed))
    with torch.no_grad():
        want = T._torch_resnet(sd, arch, px)
    got, _ = T.resnet_exact(arch, T.resnet_operands(arch, sd, round_matrices=False), px)
    _pin(cid, got, want)


def _yardstick(name, ex, mo):
    for what, e, m in (("output", ex[0], mo[0]), ("stream", ex[1], mo[1])):
        y = (m - e).norm(dim=1)
        r = row_ratio(m, e, m)          # raises ZeroYardstick if a row of the model is exact
        print(f"CONVTOWER_YARDSTICK {name} {what}: {tuple(e.shape)} row error of the model min {float(y.min()):.3e} median {float(y.median()):.3e} max {float(y.max()):.3e}")
        assert float(y.min()) > 0 and r["ratio"] == 1.0 and bool(torch.isfinite(m).all())


@pytest.mark.parametrize("cid", list(_CNX))
def test_convnext_yardstick_is_positive_in_every_row(cid):
    _, _, _, px, ex, mo = _cnx(cid)
    assert len({px[i].numpy().tobytes() for i in range(N)}) == N       # images that differ from each other
    _yardstick(cid, ex, mo)


@pytest.mark.parametrize("cid", list(_RN))
def test_resnet_yardstick_is_positive_in_every_row(cid):
    _, _, _, px, ex, mo = _rn(cid)
    assert len({px[i].numpy().tobytes() for i in range(N)}) == N
    _yardstick(cid, ex, mo)


def test_yardstick_is_positive_on_the_large_batches():
    cid = T.convnext_cases()[0][0]
    _, _, _, _, ex, mo = _cnx(cid, T.CNX_BIG_N)
    _yardstick(f"{cid} n={T.CNX_BIG_N}", ex, mo)
    cid = T.resnet_cases()[0][0]
    _, _, _, _, ex, mo = _rn(cid, T.RN_BIG_N)
    _yardstick(f"{cid} n={T.RN_BIG_N}", ex, mo)


def test_a_batch_is_a_prefix_of_a_larger_one():
    assert torch.equal(T.images(1, 32, 5), T.images(3, 32, 5)[:1]) and torch.equal(T.images(3, 64, 6), T.images(5, 64, 6)[:3])


def _seen(name, mutant, ex, mo):
    ro = row_ratio(mutant[0], ex[0], mo[0])["ratio"]
    rs = row_ratio(mutant[1], ex[1], mo[1])["ratio"]
    print(f"CONVTOWER_MUTATION {name}: output rows {ro:.3g}, stream rows {rs:.3g} (bar {MARGIN})")
    return ro, rs


_RN_BLIND = ("pad_not_zero",)


@pytest.mark.parametrize("mut", T.CNX_MUTATIONS)
@pytest.mark.parametrize("cid", list(_CNX))
def test_convnext_mutation_leaves_the_bar(cid, mut):
    arch, _, ops, px, ex, mo = _cnx(cid)
    ro, rs = _seen(f"convnext {cid} {mut}", T.convnext_model(arch, ops, px, mut), ex, mo)
    blind = mut in ("pool_divisor", "quick_gelu") or (mut == "eps_swapped" and not cid.endswith("dimstem"))
    if blind:       # (module docstring: what this test cannot see, and why — asserted, so that the docstring stays true)
        assert max(ro, rs) <= MARGIN
        return
    assert max(ro, rs) > MARGIN
    if mut == "pool_positions":
        assert rs == 1.0 and ro > MARGIN       # behind the stream: the output rows alone show it


@pytest.mark.parametrize("mut", T.RN_MUTATIONS)
@pytest.mark.parametrize("cid", list(_RN))
def test_resnet_mutation_leaves_the_bar(cid, mut):
    arch, _, ops, px, ex, mo = _rn(cid)
    ro, rs = _seen(f"resnet {cid} {mut}", T.resnet_model(arch, ops, px, mut), ex, mo)
    padded = arch.width % 64 != 0
    if mut in _RN_BLIND:        # (module docstring: finite garbage in a padded channel meets zero weights — exactly invisible)
        assert ro == 1.0 and rs == 1.0
        return
    if mut == "pad_nan" and not padded:
        assert ro == 1.0 and rs == 1.0      # width 64: nothing is padded
        return
    if mut == "ds_by_padded_width" and arch.width != 16:
        assert ro == 1.0 and rs == 1.0      # pad64(w) == 4 w at w = 16 only
        return
    if mut in ("no_positions", "q_unscaled", "images_swapped"):
        assert rs == 1.0
        assert ro > MARGIN
        return
    assert max(ro, rs) > MARGIN


def test_zero_yardstick_is_an_error():
    ex = torch.randn(4, 8, dtype=torch.float64)
    mo = ex + 1e-3
    mo[2] = ex[2]
    with pytest.raises(ZeroYardstick):
        row_ratio(ex, ex, mo)

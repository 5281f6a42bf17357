"""What the attention tests' rounding budget can and cannot see, shown without a GPU (tests/attention_ref.py).

1. The arithmetic model of csrc/attention.hip (`emulate`: 64-key tiles, online softmax, probabilities rounded to bf16 for P.V, bf16 store) stays within
   1.0 x budget of the float64 reference on every input family, mask, head stride and length the GPU tests use: the bound u * (P|V| + |out|) holds for the
   design itself, so a kernel outside 1.25 x budget is wrong and not merely rounding differently.
2. The same model with ONE deliberate fault (a `mutant=` switch, not a copy) leaves 1.25 x budget on the `readout` inputs: the budget and the inputs have
   the discriminating power the GPU tests rely on.  The one exception is called out at its test."""
import functools

import pytest
import torch

from tests import attention_ref as R

LENS = [1, 2, 15, 16, 17, 63, 64, 65, 77, 80, 81, 257, 320, 321, 640, 641, 1024]
HEADS = 3    # the ramp families give each of three heads its own slope
MASKS = (R.MASK_NONE, R.MASK_CAUSAL, R.MASK_CAUSAL_CLS)


def _cases():
    for fam in R.FAMILIES:
        for hs in (64, 96, 112, 128):
            if fam == "padded_heads":
                for real in R.REAL_DIMS.get(hs, ()):
                    yield fam, hs, real
            else:
                yield fam, hs, None


@functools.lru_cache(maxsize=None)
def _inputs(fam, hs, real, mask):
    qkv = R.make_qkv(fam, LENS, HEADS, hs, seed=hs + len(fam), real=real)
    out, absout, _ = R.reference(qkv, LENS, HEADS, hs, mask)
    return qkv, out, absout


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("fam,hs,real", list(_cases()))
def test_model_of_the_kernel_stays_inside_the_budget(fam, hs, real, mask):
    qkv, out, absout = _inputs(fam, hs, real, mask)
    got = R.emulate(qkv, LENS, HEADS, hs, mask)
    assert torch.isfinite(got.float()).all()
    w = R.worst_coords(got, out, absout, LENS, HEADS, hs)
    print(f"{fam} hs={hs} real={real} mask={mask}: worst |emulate - reference| / budget = {w['ratio']:.3f} at {w}")
    assert w["ratio"] <= 1.0, w
    if real is not None:      # zero V columns give exactly zero outputs
        assert (got.view(-1, HEADS, hs)[:, :, real:] == 0).all()


def _mutant_ratio(mutant, fam, hs, mask):
    qkv, out, absout = _inputs(fam, hs, None, mask)
    return R.worst_ratio(R.emulate(qkv, LENS, HEADS, hs, mask, mutant=mutant), out, absout)


@pytest.mark.parametrize("hs", (64, 128))
@pytest.mark.parametrize("mutant,mask", [("dup_last", R.MASK_NONE), ("causal_plus1", R.MASK_CAUSAL), ("causal_plus1", R.MASK_CAUSAL_CLS),
                                         ("causal_minus_self", R.MASK_CAUSAL), ("cls_drop", R.MASK_CAUSAL_CLS), ("skip_tile", R.MASK_NONE),
                                         ("skip_tile", R.MASK_CAUSAL), ("l_no_alpha", R.MASK_NONE), ("l_no_alpha", R.MASK_CAUSAL),
                                         ("o_no_alpha", R.MASK_NONE), ("o_no_alpha", R.MASK_CAUSAL)])
def test_single_faults_leave_the_budget_on_readout_inputs(mutant, mask, hs):
    r = _mutant_ratio(mutant, "readout", hs, mask)
    print(f"mutant {mutant} mask={mask} hs={hs}: readout worst ratio {r:.3g}")
    assert not r <= 1.25, r      # (a NaN / inf output counts as caught)


@pytest.mark.parametrize("fam", ("randn", "peaked", "ramp_up"))
@pytest.mark.parametrize("mutant,mask", [("dup_last", R.MASK_NONE), ("causal_plus1", R.MASK_CAUSAL), ("cls_drop", R.MASK_CAUSAL_CLS),
                                         ("skip_tile", R.MASK_NONE), ("l_no_alpha", R.MASK_NONE), ("o_no_alpha", R.MASK_NONE)])
def test_single_faults_on_the_other_families(mutant, mask, fam):
    """not every family sees every fault (ramp_up puts no weight on an early tile: skipping it changes nothing there) — each fault is seen by at least one of
    them besides `readout`, and which is printed"""
    r = _mutant_ratio(mutant, fam, 64, mask)
    print(f"mutant {mutant} mask={mask}: {fam} worst ratio {r:.3g}")
    if (mutant, fam) != ("skip_tile", "ramp_up"):
        assert not r <= 1.25, r


def test_class_row_self_exclusion_is_guarded_at_length_one():
    """MASK_CAUSAL_CLS at len == 1: the only row would see nothing.  The guarded model returns V[0]; the unguarded mutant returns nothing finite."""
    for hs in (64, 128):
        qkv = R.make_qkv("randn", [1, 1, 5], 2, hs, seed=3)
        W = 2 * hs
        good = R.emulate(qkv, [1, 1, 5], 2, hs, R.MASK_CAUSAL_CLS)
        assert torch.isfinite(good.float()).all()
        assert torch.equal(good[:2], qkv[:2, 2 * W:])
        out, _, P = R.reference(qkv, [1, 1, 5], 2, hs, R.MASK_CAUSAL_CLS, keep_p=True)
        assert torch.equal(out[:2], qkv[:2, 2 * W:].double()) and float(P[0][0, 0, 0]) == 1.0 and float(P[2][0, 4, 4]) == 0.0
        bad = R.emulate(qkv, [1, 1, 5], 2, hs, R.MASK_CAUSAL_CLS, mutant="cls_len1")
        assert not torch.isfinite(bad[:2].float()).any()
        assert torch.equal(bad[2:], good[2:])


def test_normaliser_from_rounded_probabilities_is_not_distinguished():
    """THE PERMITTED EXCEPTION.  Summing the normaliser from the bf16-rounded probabilities (instead of the fp32 ones, as the kernel does) moves numerator and
    denominator together: it is a design choice of the same error class, and the budget does not tell the two apart.  This test documents that: the mutant stays
    inside 1.25 x budget on every family (it may exceed 1.0: the derivation assumes the unrounded sum)."""
    worst = 0.0
    for fam in ("randn", "peaked", "readout", "ramp_up", "ramp_down"):
        for mask in (R.MASK_NONE, R.MASK_CAUSAL):
            r = _mutant_ratio("l_from_bf16", fam, 64, mask)
            print(f"mutant l_from_bf16 mask={mask}: {fam} worst ratio {r:.3f}")
            worst = max(worst, r)
    assert worst <= 1.25, worst


def test_reference_masks_and_packing():
    """the reference itself: rows of P sum to 1 over exactly the admitted keys, sequences do not see each other, empty sequences are skipped"""
    lens = [0, 5, 0, 0, 7, 0]
    qkv = R.make_qkv("randn", lens, 2, 64, seed=1)
    for mask in MASKS:
        out, absout, P = R.reference(qkv, lens, 2, 64, mask, keep_p=True)
        assert len(P) == len(lens) and out.shape == (12, 128)
        for ln, p in zip(lens, P):
            assert p.shape == (2, ln, ln)
            if ln:
                ok = R.allowed(ln, mask)
                assert torch.allclose(p.sum(-1), torch.ones(2, ln, dtype=torch.float64)) and (p[:, ~ok] == 0).all() and (p[:, ok] > 0).all()
        alone, _, _ = R.reference(qkv[5:].contiguous(), [7], 2, 64, mask)
        assert torch.equal(alone, out[5:])
        assert (absout >= out.abs() - 1e-15).all()
    ok = R.allowed(4, R.MASK_CAUSAL_CLS)
    assert ok.tolist() == [[True, False, False, False], [True, True, False, False], [True, True, True, False], [True, True, True, False]]
    assert R.allowed(1, R.MASK_CAUSAL_CLS).tolist() == [[True]]


def test_readout_values_expose_each_key():
    """`readout`: for len <= hs the output IS the probability row; the reserved last column belongs to the last key alone"""
    lens = [50, 64, 78]
    qkv = R.make_qkv("readout", lens, 1, 64, seed=2)
    out, _, P = R.reference(qkv, lens, 1, 64, R.MASK_NONE, keep_p=True)
    assert torch.allclose(out[:50, :50], P[0][0], atol=0, rtol=1e-15) and (out[:50, 50:] == 0).all()
    assert torch.allclose(out[50:114].roll(-1, 1), P[1][0], atol=0, rtol=1e-15)          # sequence 1 is shifted by one column
    v = R.readout_v(lens, 1, 64, reserve_last=True)
    for r_last in (49, 113, 191):
        assert v[r_last, 0].tolist() == [0.0] * 63 + [1.0]
    assert (v[:, 0, 63].sum() == 3) and (v[:, 0, :63].sum(-1)[[0, 48, 50, 112, 114]] == 1).all()

"""What the row-kernel tests' rounding budgets can and cannot see, shown without a GPU (tests/rowops_ref.py).

1. The float32 model of the LayerNorm kernels (generic: 4 elements per lane and chunk; wide: 8), of the one-pass finalise and of the L2 kernel stays
   within 1.0 x budget of the float64 reference on every input family, at 15 widths, eps 1e-5 and 1e-12, fp32 and bf16-exact inputs, with and without
   the fma contraction of the compiler: a kernel outside 1.25 x budget is wrong and not merely rounding differently.
   Worst ratios seen here (printed by the tests): see the comments at the tests.
2. The same model with ONE deliberate fault leaves 1.25 x budget on the families named in FAULT_CASES."""
import functools

import numpy as np
import pytest
import torch

from tests import rowops_ref as R

ROWS = 24
EPS = (1e-5, 1e-12)


@functools.lru_cache(maxsize=None)
def _inputs(fam, W, bf16, eps):
    x, g, b = R.make_rows(fam, ROWS, W, seed=3, bf16=bf16)
    y, B = R.reference_ln(x, g, b, eps)
    return x, g, b, y, B


def _model_ratio(fam, W, bf16, eps, form, fault=None, out_bf16=False, fma=False):
    x, g, b, y, B = _inputs(fam, W, bf16, eps)
    got, _, _ = R.model_layernorm(x.float().numpy(), g.numpy(), b.numpy(), eps, form=form, fault=fault, out_bf16=out_bf16, fma=fma)
    return R.ratio(torch.from_numpy(got), y, B + R.half_ulp_bf16(y) if out_bf16 else B)


def _forms(W):
    return ("generic", "wide") if W % 8 == 0 and W <= 1024 else ("generic",)


# worst ratio over the whole matrix (fp32 output): 0.48; per family randn 0.48, offset 0.40, outlier 0.47, const 0.04, rowscale 0.46.
# bf16 output: 1.000 (a value next to a rounding tie uses the whole half ulp, as it must)
@pytest.mark.parametrize("bf16", (False, True))
@pytest.mark.parametrize("fam", R.FAMILIES)
def test_model_of_the_layernorm_kernels_stays_inside_the_budget(fam, bf16):
    worst = {}
    for W in R.HOST_WIDTHS:
        for eps in EPS:
            for form in _forms(W):
                for fma in (False, True):
                    for out_bf16 in (False, True):
                        r = _model_ratio(fam, W, bf16, eps, form, out_bf16=out_bf16, fma=fma)
                        assert r <= 1.0, (fam, W, eps, form, fma, out_bf16, r)
                        worst[out_bf16] = max(worst.get(out_bf16, 0.0), r)
    print(f"LN_MODEL family={fam} bf16_in={bf16} worst ratio: fp32 out {worst[False]:.3f}, bf16 out {worst[True]:.3f}")


# worst ratios: mean 0.05 of c (rowscale), rstd 0.24 of rho (outlier)
@pytest.mark.parametrize("fam", R.FAMILIES)
def test_model_statistics_stay_inside_c_and_rho(fam):
    wm = wr = 0.0
    for W in (8, 504, 520, 1024, 1032, 1536, 2048):
        for eps in EPS:
            x, g, b = R.make_rows(fam, ROWS, W, seed=5, bf16=True)
            mu, rstd, c, rho = R.stats_budget(x, eps)
            for fma in (False, True):
                _, m, r = R.model_layernorm(x.float().numpy(), g.numpy(), b.numpy(), eps, form="wide" if W <= 1024 else "generic", fma=fma)
                rm = R.ratio(torch.from_numpy(m), mu, c)
                rr = R.ratio(torch.from_numpy(r), rstd, rho * rstd)
                assert rm <= 1.0 and rr <= 1.0, (fam, W, eps, rm, rr)
                wm, wr = max(wm, rm), max(wr, rr)
    print(f"STATS_MODEL family={fam} worst ratio: mean {wm:.3f}, rstd {wr:.3f}")


# (fault, form, W, eps, bf16 output, the families on which it must leave 1.25 x budget).  Measured ratios (fp32 / bf16-exact input):
#   (a) one_pass            W = 768: offset 13.2 / 8.6, rowscale 17.7 / 25.5 (its rows with |mean| >> sigma); W = 1024 wide: offset 9.5 / 4.9, rowscale 13 / 14
#   (b) no_eps              const inf (0 * inf), rowscale 715 at W = 768, 4.3e3 at W = 512 (sigma = 1e-2 against eps = 1e-5)
#   (c) padded_width        W = 260 runs as 512: randn 6.0e5, offset 1.2e5, outlier 4.7e5, const 1.7e3, rowscale 6.6e5
#   (d) prev_row_mean       rowscale 5.1e5, randn 7.3e4 (the sample means of two rows differ by sigma / sqrt(W)), outlier 7.3e4, offset 1.3e3
#   (e) gamma_other_half    W = 1024: randn 9.8e7, offset 2.3e7, outlier 1.5e8, const 1.5e5, rowscale 9.3e7
#   (f) bf16_truncate       2.0 on every family but const (1.87): the full ulp against the half of it
#   (g) skip_ragged_chunk   W = 260 (the last chunk covers 1 of 64 lanes): randn 2.8e4, offset 3.2e4, rowscale 3.1e4
# What stays inside is listed in test_documented_exceptions_faults_that_stay_inside.
FAULT_CASES = [
    ("one_pass", "generic", 768, 1e-5, False, ("offset", "rowscale")),
    ("one_pass", "wide", 1024, 1e-5, False, ("offset", "rowscale")),
    ("no_eps", "generic", 768, 1e-5, False, ("const", "rowscale")),
    ("no_eps", "wide", 512, 1e-5, False, ("const", "rowscale")),
    ("padded_width", "generic", 260, 1e-5, False, ("randn", "offset", "outlier", "const", "rowscale")),
    ("padded_width", "generic", 1028, 1e-5, False, ("randn", "offset", "rowscale")),
    ("padded_width", "wide", 520, 1e-5, False, ("randn", "offset", "rowscale")),
    ("prev_row_mean", "wide", 1024, 1e-5, False, ("rowscale", "randn", "offset", "outlier")),
    ("prev_row_mean", "generic", 768, 1e-5, True, ("rowscale", "randn")),
    ("gamma_other_half", "wide", 1024, 1e-5, False, R.FAMILIES),
    ("gamma_other_half", "wide", 8, 1e-5, True, ("randn", "offset", "outlier", "rowscale")),
    ("bf16_truncate", "generic", 768, 1e-5, True, R.FAMILIES),
    ("bf16_truncate", "wide", 512, 1e-12, True, ("randn", "offset", "outlier", "rowscale")),
    ("skip_ragged_chunk", "generic", 260, 1e-5, False, ("randn", "offset", "rowscale")),
    ("skip_ragged_chunk", "wide", 520, 1e-5, False, ("randn", "offset", "rowscale")),
]


@pytest.mark.parametrize("fault,form,W,eps,out_bf16,fams", FAULT_CASES)
def test_single_faults_leave_the_budget(fault, form, W, eps, out_bf16, fams):
    seen = {}
    for fam in R.FAMILIES:
        for bf16 in (False, True):
            assert _model_ratio(fam, W, bf16, eps, form, out_bf16=out_bf16) <= 1.0          # the unfaulted model at the same point
            seen[(fam, bf16)] = _model_ratio(fam, W, bf16, eps, form, fault=fault, out_bf16=out_bf16)
    print(f"LN_FAULT {fault} form={form} W={W} eps={eps} bf16_out={out_bf16}: " + "  ".join(f"{f}{'/bf16' if h else ''} {r:.3g}" for (f, h), r in seen.items()))
    for fam in fams:
        for bf16 in (False, True):
            assert seen[(fam, bf16)] > 1.25, (fault, fam, bf16, seen[(fam, bf16)])


def test_documented_exceptions_faults_that_stay_inside():
    """NOT caught, and why (so that nobody takes the families for more than they are):
    one_pass on `randn` and `outlier` (E[x^2] / sigma^2 is 1.25 / 1 + 3600 / W: no cancellation to speak of; ratios 0.39 / 0.43) and on `const` in the
    LayerNorm OUTPUT (x - mean is exactly 0 there and multiplies whatever rstd came out; the finalise tests check rstd itself on `const`);
    no_eps on `randn` (eps is 1e-6 of the variance; 0.54); prev_row_mean on `const` (every row has the same mean); gamma_other_half at W = 4 (there is
    no other half); skip_ragged_chunk and padded_width at widths that fill their chunks (W = 512: the faults are no-ops); and bf16_truncate on `const`
    at eps = 1e-12 (0.53: sigma' = 1e-6 makes the budget c / sigma' as wide as the outputs, a bf16 ulp disappears in it; one_pass and prev_row_mean stay
    inside there for the reason they do at eps = 1e-5; no_eps (inf) and gamma_other_half (94) are caught there too)."""
    for fam in ("randn", "outlier", "const"):
        assert _model_ratio(fam, 768, False, 1e-5, "generic", fault="one_pass") <= 1.25
    assert _model_ratio("randn", 768, False, 1e-5, "generic", fault="no_eps") <= 1.25
    assert _model_ratio("const", 768, False, 1e-5, "generic", fault="prev_row_mean") <= 1.25
    assert _model_ratio("randn", 4, False, 1e-5, "generic", fault="gamma_other_half") <= 1.0
    for fault in ("bf16_truncate", "one_pass", "prev_row_mean"):
        assert _model_ratio("const", 512, True, 1e-12, "wide", fault=fault, out_bf16=True) <= 1.25
    for fault in ("no_eps", "gamma_other_half"):
        assert _model_ratio("const", 768, False, 1e-12, "generic", fault=fault) > 1.25
    for fault in ("skip_ragged_chunk", "padded_width"):
        assert _model_ratio("randn", 512, False, 1e-5, "generic", fault=fault) == _model_ratio("randn", 512, False, 1e-5, "generic")


# ---- the one-pass finalise ---------------------------------------------------------------------------------------------------------------
FIN_SLOTS = (1, 7, 8, 9, 12, 26, 32)


def _finalize_ratios(fam, nslots, W, eps, first8=False):
    x, _, _ = R.make_rows(fam, ROWS, W, seed=11)
    p = R.make_partials(x, nslots)
    mu, t, cf, bt = R.finalize_reference(p, W, eps)
    mean, rstd = R.model_finalize(p.numpy(), W, eps, first8=first8)
    assert np.isfinite(mean).all() and np.isfinite(rstd).all()
    that = torch.from_numpy(rstd).double() ** -2
    return R.ratio(torch.from_numpy(mean), mu, cf), R.ratio(that, t, bt)


# worst ratios: mean 0.43 of c_f, t = rstd^-2 0.40 of its bound (both on `outlier`); const: 0.20 / 0.12
@pytest.mark.parametrize("fam", R.FAMILIES)
def test_model_of_the_finalise_stays_inside_its_budget(fam):
    wm = wt = 0.0
    for nslots in FIN_SLOTS:
        for W in (64, 768, 1280):
            for eps in EPS:
                rm, rt = _finalize_ratios(fam, nslots, W, eps)
                assert rm <= 1.0 and rt <= 1.0, (fam, nslots, W, eps, rm, rt)
                wm, wt = max(wm, rm), max(wt, rt)
    print(f"FIN_MODEL family={fam} worst ratio: mean {wm:.3f}, t {wt:.3f}")


# (h) only the first 8 slots summed: invisible up to 8 slots (the documented exception: there is nothing to drop), 9 slots: the mean is 1.7e5 .. 2.8e5 budgets off on every family, t 2.6e4 .. 1.3e5
@pytest.mark.parametrize("nslots", (9, 12, 26, 32))
def test_finalise_that_sums_eight_slots_leaves_the_budget(nslots):
    for fam in R.FAMILIES:
        rm, rt = _finalize_ratios(fam, nslots, 768, 1e-5, first8=True)
        print(f"FIN_FAULT first8 nslots={nslots} family={fam}: mean {rm:.3g}, t {rt:.3g}")
        assert rm > 1.25, (fam, nslots, rm)
    for n in (1, 7, 8):
        assert _finalize_ratios("randn", n, 768, 1e-5, first8=True) == _finalize_ratios("randn", n, 768, 1e-5)


# ---- L2 ----------------------------------------------------------------------------------------------------------------------------------
# worst ratio 0.38
def test_model_of_the_l2_kernel_stays_inside_its_budget():
    worst = 0.0
    for D in (1, 63, 64, 65, 512, 1000):
        for fam in ("randn", "offset", "outlier", "rowscale"):
            x, _, _ = R.make_rows(fam, ROWS, D, seed=2)
            y, b = R.reference_l2(x)
            worst = max(worst, R.ratio(torch.from_numpy(R.model_l2(x.numpy())), y, b))
    print(f"L2_MODEL worst ratio {worst:.3f}")
    assert worst <= 1.0


# ---- helpers of the fp8 checks -----------------------------------------------------------------------------------------------------------
def test_e4m3_tie_distance_and_code_steps():
    vals = torch.tensor([0.0, 2.0 ** -10, 2.0 ** -9, 1.0, 1.0625, 1.125, 17.0, 18.0, 416.0, 432.0, 448.0, 500.0], dtype=torch.float64)
    want = torch.tensor([2.0 ** -10, 0.0, 2.0 ** -10, 0.0625, 0.0, 0.0625, 0.0, 1.0, 16.0, 0.0, float("inf"), float("inf")], dtype=torch.float64)
    assert torch.equal(R.e4m3_tie_distance(vals), want) and torch.equal(R.e4m3_tie_distance(-vals), want)
    # every e4m3 value is its own code, neighbours are one signed step apart, and +-0 are the same step
    codes = torch.arange(0, 0x7F, dtype=torch.uint8)
    v = codes.view(torch.float8_e4m3fn).double()
    assert torch.equal(R.e4m3_codes(v), codes) and torch.equal(R.e4m3_codes(-v)[1:], codes[1:] | 0x80)
    assert torch.equal(R.e4m3_signed(codes), torch.arange(0, 0x7F, dtype=torch.int32))
    assert torch.equal(R.e4m3_signed(codes | 0x80), -torch.arange(0, 0x7F, dtype=torch.int32))
    assert (v[1:] > v[:-1]).all()


def test_bf16_half_ulp_and_rounding():
    y = torch.tensor([0.0, 1.0, 1.99, 2.0, -3.0, 2.0 ** -20], dtype=torch.float64)
    assert torch.equal(R.half_ulp_bf16(y), torch.tensor([0.0, 2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 2.0 ** -7, 2.0 ** -28], dtype=torch.float64))
    x = torch.randn(4096) * 5
    assert np.array_equal(R.round_bf16(x.numpy()), x.to(torch.bfloat16).float().numpy())
    assert (np.abs(R.round_bf16(x.numpy(), truncate=True)) <= np.abs(x.numpy())).all()

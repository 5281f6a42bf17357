"""What the fp8 GEMM parity tests' checks can and cannot see, shown without a GPU (tests/gemm_fp8_ref.py).

1. The integer constructions are exact: the fp32 matmul of every integer case equals its float64 one and itself under a random permutation of K, and
   every sparse bf16-output value survives .to(bfloat16) unchanged.
2. The clean fp32 model (torch on the CPU) passes every check of tests/test_gemm_fp8_parity_gpu.py on every shape that test uses: the exact-integer
   comparison, 1.0 x the per-element budget, the permitted e4m3 codes on every element, the amax bounds.
3. On every one of those cases at least 0.70 of the elements of an e4m3 output have a single permitted value (printed: the smallest share per family).
4. The same model with ONE seeded fault (gemm_fp8_ref.FAULTS, (a) .. (o)) is caught by the check that owns it, at the smallest and at the largest shape.
5. permitted_codes agrees with a brute-force scan of all 254 finite codes."""
import pytest
import torch

from tests import gemm_fp8_ref as R

B, G, Q, RS, F, P8 = R.BIAS, R.GELU, R.QUICK, R.RES, R.F32, R.FP8
MARGIN = 1.25

SMALLEST, LARGEST = (33, 4, 128, 64), (385, 512, 1024, 192)          # (M, N, K, rows of the row tile that runs it)


def _gpu_shapes():
    s = {x for mt in R.TILED_MT for x in R.tiled_shapes(mt)} | set(R.big_shapes()) | {R.cgroup_shape(4)}
    return sorted(s)


def _long_shapes():
    return sorted({(32 * mt + 1, 132, R.LONG_K) for mt in R.TILED_MT} | {(193, 260, R.LONG_K)})


def verdict(flags, c, rowscale, got, out_scale=None):
    """the GPU test's checks on one launch's results: (passes, figure) — exact cases: equality (fp32 / bf16) or every code permitted and amax inside;
    random cases: ratio <= 1.25 or the same code and amax checks"""
    r = R.reference(flags, c, rowscale, out_scale)
    if flags & P8:
        ok = bool(R.codes_permitted(got["codes"], r["lo"], r["hi"]).all())
        return ok and R.amax_ok(got["amax"], r), r["determined"]
    if c["exact"]:
        return torch.equal(got["out"].double(), r["ref"]), 0.0
    q = R.ratio(got["out"], r["ref"], r["bound"])
    return q <= MARGIN, q


def _case_for(flags, M, N, K, kind):
    if kind == "rand":
        return R.rand_case(R.family_for(M, N, K), M, N, K)
    if kind == "int1":
        return R.int_case("sparse_one", M, N, K)
    return R.int_case("dense" if flags & F else "sparse_pos" if flags & P8 else "sparse", M, N, K)


def _out_scales(flags, c, rowscale, kind):
    """both out_scales; the one-non-zero integer case runs with max|ref| / 448 only (gemm_fp8_ref docstring)"""
    if not flags & P8:
        return (None,)
    return R.out_scales(flags, c, rowscale)[:1 if kind == "int1" else 2]


@pytest.fixture(scope="module")
def sweep():
    """the clean model through every check on every GPU shape, once: (failures, worst ratio per form, smallest determined share per family / 'int')"""
    fails, worst, share = [], {}, {}
    for (M, N, K) in _gpu_shapes():
        cases = {"dense": R.int_case("dense", M, N, K), "sparse": R.int_case("sparse", M, N, K), "sparse_pos": R.int_case("sparse_pos", M, N, K), "int1": R.int_case("sparse_one", M, N, K),
                 "rand": R.rand_case(R.family_for(M, N, K), M, N, K)}
        for flags in R.FORMS:
            for rowscale in (True, False):
                for kind in ("int", "rand") + (("int1",) if flags == B | G | P8 and rowscale else ()):
                    c = cases[kind] if kind in ("rand", "int1") else cases["dense" if flags & F else "sparse_pos" if flags & P8 else "sparse"]
                    for osc in _out_scales(flags, c, rowscale, kind):
                        got = R.model(flags, c, rowscale, osc)
                        r = R.reference(flags, c, rowscale, osc)
                        if flags & P8:
                            fam = kind if kind != "rand" else R.family_for(M, N, K)
                            share[fam] = min(share.get(fam, 1.0), r["determined"])
                            if r["determined"] < 0.70:
                                fails.append(("determined", hex(flags), rowscale, kind, M, N, K, osc, r["determined"]))
                            if not bool(R.codes_permitted(got["codes"], r["lo"], r["hi"]).all()):
                                fails.append(("codes", hex(flags), rowscale, kind, M, N, K, osc, R.first_bad_code(got["codes"], r, 64, 128)))
                            if not R.amax_ok(got["amax"], r):
                                fails.append(("amax", hex(flags), rowscale, kind, M, N, K, osc, got["amax"], r["amax_lo"], r["amax_hi"]))
                        elif kind == "int":
                            if not torch.equal(got["out"].double(), r["ref"]):
                                fails.append(("int", hex(flags), rowscale, M, N, K, R.first_difference(got["out"], r["ref"], 64, 128)))
                        else:
                            q = R.ratio(got["out"], r["ref"], r["bound"])
                            worst[flags] = max(worst.get(flags, 0.0), q)
                            if q > 1.0:
                                fails.append(("budget", hex(flags), rowscale, M, N, K, q, R.worst(got["out"], r)))
    return fails, worst, share


def test_integer_constructions_are_exact():
    shapes = [s for s in _gpu_shapes() if s[0] in (33, 65, 193, 385)] + _long_shapes()
    for (M, N, K) in shapes:
        dense = R.int_case("dense", M, N, K)
        A, W = dense["A"].float(), dense["W"].float()
        assert float(A.abs().max()) <= 4 and float(W.abs().max()) <= 4 and torch.equal(A, A.round()) and torch.equal(W, W.round())
        acc = A @ W.t()
        assert torch.equal(acc.double(), A.double() @ W.double().t()), (M, N, K)
        perm = torch.randperm(K, generator=torch.Generator().manual_seed(K + M))
        assert torch.equal(A[:, perm] @ W[:, perm].t(), acc), (M, N, K)
        if K == R.LONG_K:
            continue
        sparse = R.int_case("sparse", M, N, K)
        As = sparse["A"].float()
        assert int((As != 0).sum(1).max()) <= 4 and int((As != 0).sum(1).min()) >= 1
        if K >= 1024:
            assert bool((As.view(M, K // 128, 128) != 0).any(-1).any(0).all()), "the sparse rows together reach every k-step"
        assert torch.equal(As @ sparse["W"].float().t(), (As.double() @ sparse["W"].double().t()).float())
        for rowscale in (True, False):
            for flags in (F, B | RS | F):
                ref = R.reference(flags, dense, rowscale)["ref"]
                assert torch.equal(ref, ref.float().double()) and float(ref.abs().max()) < 2 ** 24
            for flags in (B, B | RS):
                ref = R.reference(flags, sparse, rowscale)["ref"]
                assert torch.equal(ref, ref.to(torch.bfloat16).double()) and float(ref.abs().max()) <= 200, (hex(flags), M, N, K)


def test_clean_model_passes_every_check_on_every_gpu_shape(sweep):
    fails, worst, _ = sweep
    print("GEMM_FP8_REF clean model, worst ratio per form: " + "  ".join(f"{hex(k)} {v:.3f}" for k, v in worst.items()))
    assert not [f for f in fails if f[0] != "determined"], fails[:5]


def test_most_e4m3_elements_have_a_single_permitted_code(sweep):
    fails, _, share = sweep
    print("GEMM_FP8_REF smallest share of elements with a single permitted e4m3 value: " + "  ".join(f"{k} {v:.3f}" for k, v in sorted(share.items())))
    assert set(share) == set(R.FAMILIES) | {"int", "int1"}
    assert not [f for f in fails if f[0] == "determined"], [f for f in fails if f[0] == "determined"][:5]


def test_long_k_integer_cases_pass_on_the_clean_model():
    for (M, N, K) in _long_shapes():
        c = R.int_case("dense", M, N, K)
        for rowscale in (True, False):
            for flags in (F, B | RS | F):
                assert verdict(flags, c, rowscale, R.model(flags, c, rowscale))[0]


# fault -> the checks that own it: (kind of case, flag set, per-row a_scale).  Each runs at the smallest and at the largest shape of the GPU test, with that
# test's own inputs; an e4m3 form runs with both out_scales and counts as caught only if it is caught with each.
OWNERS = {
    "drop_product": [("int", F, True), ("int", B | RS | F, False), ("rand", F, True)],
    "drop_kstep_ragged": [("int", F, True), ("int", B | RS | F, False)],
    "swap_kchunks": [("int", F, True), ("int", B | RS | F, False)],
    "a_scale_row1": [("int", F, True), ("rand", B, True)],
    "w_scale_shift4": [("int", F, True), ("int", B, False), ("rand", B | RS | F, True)],
    "bias_shift4": [("int", B, True), ("int", B | RS | F, False)],
    "residual_row16": [("int", B | RS | F, True), ("int", B | RS, False)],
    "bf16_truncate": [("rand", B, True), ("rand", B | RS, False)],
    "tanh_gelu": [("int1", B | G | P8, True)],
    "gelu_for_quick": [("rand", B | Q | P8, False)],          # (per-row scales at the smallest shape: `outlier` arguments, where the two saturate alike)
    "fp8_truncate": [("int", B | G | P8, True), ("rand", B | Q | P8, False)],
    "fp8_swap_halves": [("int", B | G | P8, True), ("rand", B | Q | P8, False)],
    "fp8_multiply_scale": [("int", B | Q | P8, True), ("rand", B | G | P8, False)],
    "scalar_reads_row": [("int", F, False), ("int", B, False), ("int", B | G | P8, False)],
}


def test_every_fault_has_an_owner():
    assert set(OWNERS) | {"amax_pad_column"} == set(R.FAULTS)
    for f in ("drop_product", "drop_kstep_ragged", "swap_kchunks", "scalar_reads_row"):
        assert OWNERS[f][0][0] == "int" and not OWNERS[f][0][1] & P8          # at least the exact-integer comparison


@pytest.mark.parametrize("fault", [f for f in R.FAULTS if f != "amax_pad_column"])
def test_seeded_fault_is_caught_by_the_check_that_owns_it(fault):
    # (i): a 16 x 4 sub-tile holds too few arguments in [-3.5, -2.5], where alone the e4m3 output can tell the two GELUs apart: the smallest shape of 64 columns
    for (M, N, K, BM) in ((33, 64, 128, 64) if fault == "tanh_gelu" else SMALLEST, LARGEST):
        for kind, flags, rowscale in OWNERS[fault]:
            c = _case_for(flags, M, N, K, kind)
            for osc in _out_scales(flags, c, rowscale, kind):
                ok0, fig0 = verdict(flags, c, rowscale, R.model(flags, c, rowscale, osc, BM=BM), osc)
                ok, fig = verdict(flags, c, rowscale, R.model(flags, c, rowscale, osc, fault=fault, BM=BM), osc)
                assert ok0 and not ok, (fault, kind, hex(flags), rowscale, (M, N, K), osc, fig0, fig)
                print(f"GEMM_FP8_REF fault {fault}: caught on the {kind} case, flags {hex(flags)} rowscale={rowscale} at {(M, N, K)} out_scale {osc} (figure {fig:.3f})")


def test_amax_over_a_pad_column_is_caught_by_the_amax_bounds():
    """fault (o): the pad column's value (weight row N - 1 under the scale and bias that lie behind the arrays) exceeds the valid maximum on these cases"""
    for (M, N, K, BM) in (SMALLEST, LARGEST):
        for kind, flags in (("int", B | G | P8), ("rand", B | Q | P8)):
            c = _case_for(flags, M, N, K, kind)
            for rowscale in (True, False):
                for osc in R.out_scales(flags, c, rowscale):
                    r = R.reference(flags, c, rowscale, osc)
                    clean, bad = R.model(flags, c, rowscale, osc), R.model(flags, c, rowscale, osc, fault="amax_pad_column")
                    assert torch.equal(clean["codes"], bad["codes"])
                    assert R.amax_ok(clean["amax"], r) and bad["amax"] > r["amax_hi"] and not R.amax_ok(bad["amax"], r), (kind, M, N, K, bad["amax"], r["amax_hi"])


def test_permitted_codes_against_a_scan_of_all_finite_codes():
    codes = torch.tensor([c for c in range(256) if (c & 0x7F) != 0x7F], dtype=torch.uint8)
    vals = R.decode(codes)
    assert codes.numel() == 254 and bool(torch.isfinite(vals).all()) and float(vals.abs().max()) == 448.0
    even = (codes & 1) == 0
    g = torch.Generator().manual_seed(5)
    x = torch.cat([torch.randn(1500, generator=g, dtype=torch.float64) * 3, (torch.rand(1500, generator=g, dtype=torch.float64) - 0.5) * 0.1,
                   (torch.rand(1000, generator=g, dtype=torch.float64) - 0.5) * 1200, 0.5 * (vals[:-1] + vals[1:]), vals,
                   torch.tensor([0.0, -0.0, 2.0 ** -10, -(2.0 ** -10), 3 * 2.0 ** -10, 2.0 ** -11, 464.0, -464.0, 1e9])])
    for osc in (0.05, 0.0123, 1.7):
        t = (x / osc).clamp(-448, 448)
        d = (t[:, None] - vals[None, :]).abs()
        best = d.min(1, keepdim=True).values
        tie = d == best
        pick = torch.where(tie & even[None, :], 2, torch.where(tie, 1, 0)).argmax(1)      # the nearest; of two equally near, the even one
        lo, hi = R.permitted_codes(x, torch.zeros_like(x), osc)
        assert torch.equal(lo, hi) or torch.equal(R.decode(lo), R.decode(hi))
        assert torch.equal(R.decode(lo), vals[pick]), osc
        assert bool(R.codes_permitted(codes[pick], lo, hi).all())
        # with a budget: the ends are the roundings of the two ends, every code between them (in value order) is permitted and no other
        Bx = torch.rand(x.shape, generator=g, dtype=torch.float64) * 0.02
        lo, hi = R.permitted_codes(x, Bx, osc)
        lo0, _ = R.permitted_codes(x - Bx, torch.zeros_like(x), osc)
        _, hi0 = R.permitted_codes(x + Bx, torch.zeros_like(x), osc)
        assert torch.equal(lo, lo0) and torch.equal(hi, hi0)
        inside = R.codes_permitted(codes[None, :].expand(x.numel(), -1), lo[:, None], hi[:, None])
        want = (R.decode(lo)[:, None] <= vals[None, :]) & (vals[None, :] <= R.decode(hi)[:, None])
        assert torch.equal(inside, want) and bool(inside.any(1).all())
    nan = torch.tensor([0x7F, 0xFF], dtype=torch.uint8)
    assert not bool(R.codes_permitted(nan, torch.tensor([0x80, 0x80], dtype=torch.uint8).fill_(0xFE), torch.tensor([0x7E, 0x7E], dtype=torch.uint8)).any())

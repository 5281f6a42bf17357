"""What the GEMM parity tests' checks can and cannot see, shown without a GPU (tests/gemm_ref.py).

1. The integer constructions are exact: the float64 reference equals its own fp32 / bf16 rounding on every flag set, the partial sums stay below 2^24,
   and the fp32 model reproduces them to the bit.
2. The clean fp32 model (torch on the CPU) stays within 1.0 x budget of the float64 reference for every input family, flag set and shape of
   tests/test_gemm_parity_gpu.py: a kernel outside 1.25 x budget is wrong and not merely rounding differently.  The worst ratios are printed and
   recorded in the comments at the tests.
3. The same model with ONE seeded fault (gemm_ref.FAULTS, (a) .. (k)) is caught by the check that owns it — the exact-integer comparison, or a budget
   ratio above 1.25 — on one of the GPU test's own shapes."""
import pytest
import torch

from tests import gemm_ref as R

B, G, Q, RS, F, ST, LN, GLU, RELU = R.BIAS, R.GELU, R.QUICK, R.RES, R.F32, R.ROW_STATS, R.LN, R.GLU, R.RELU

INT_F32 = (F, B | F, B | RS | F)
INT_BF16 = (0, B, B | RS, B | RELU, B | RS | RELU, B | RS | ST)
INT_LN = (B | LN, B | RELU | LN, B | RS | LN | ST)
BUDGET = (F, B, B | G, B | Q, B | RS | F, B | RS | ST, B | LN, B | G | LN, B | Q | LN, B | RS | LN | ST)
BUDGET_GLU = (B | GLU, B | GLU | LN, B | GLU | LN | ST)


def _tiled_shapes():
    ms = sorted({m for mt in R.TILED_MT for m in R.tiled_m(mt)})
    return [(M, N, K) for M in ms for N in R.TILED_N for K in R.tiled_k()]


def _big_shapes():
    return [(M, N, K) for M in R.BIG_M for N in R.BIG_N for K in R.tiled_k(big=True)]


def _skinny_shapes():
    return [(M, N, K) for M in R.SKINNY_M for N in R.TILED_N for K in R.SKINNY_K]


def _glu_shapes():
    ms = sorted({m for mt in R.TILED_MT for m in R.tiled_m(mt)})
    return [(M, N, K) for M in ms for N in R.GLU_N for K in R.tiled_k()] + [(M, 288, K) for M in R.BIG_M for K in R.tiled_k(big=True)]


def test_ring_depth_is_read_from_the_kernel_source():
    assert R.ring_depth() >= 2 and 64 in R.tiled_k() and 1024 in R.tiled_k() and R.tiled_k(big=True) == (1024,)


def _stats_ratio(out, part, flags):
    s1, s2, b1, b2 = R.slot_reference(out, 32 if flags & GLU else 64)
    return max(R.ratio(part[..., 0], s1, b1), R.ratio(part[..., 1], s2, b2))


def _int_equal(flags, c, fault=None, BM=64):
    """does the (faulty) model pass the exact-integer check of the GPU test: output and, with row statistics, partials"""
    r = R.reference(flags, c)
    out, part = R.model(flags, c, fault=fault, BM=BM)
    ok = torch.equal(out.double(), r["ref"])
    if part is not None:
        s1, s2, _, _ = R.slot_reference(r["ref"], 64)
        ok = ok and torch.equal(part[..., 0].double(), s1) and torch.equal(part[..., 1].double(), s2)
    return ok


def test_integer_constructions_are_exact():
    shapes = [s for s in _tiled_shapes() if s[0] in (33, 65, 193)] + _big_shapes()[:2] + [s for s in _skinny_shapes() if s[0] in (1, 81)]
    top = 0.0
    for (M, N, K) in shapes:
        dense, sparse, ln4 = R.int_case("dense", M, N, K), R.int_case("sparse", M, N, K), R.int_case("sparse", M, N, K, nnz=4)
        assert int((sparse["A"] != 0).sum(1).max()) <= 8 and int((ln4["A"] != 0).sum(1).max()) <= 4 and int((sparse["A"] != 0).sum(1).min()) >= 1
        if K >= 512 and M >= 16:
            steps = (sparse["A"].float().view(M, K // 64, 64) != 0).any(-1).any(0)
            assert bool(steps.all()), "the sparse rows together reach every k-step"
        for sets, c in ((INT_F32, dense), (INT_BF16, sparse), (INT_LN, ln4)):
            for flags in sets:
                ref = R.reference(flags, c)["ref"]
                rounded = ref.float().double() if flags & F else ref.to(torch.bfloat16).double()
                assert torch.equal(ref, rounded), (hex(flags), M, N, K)
                assert float(ref.abs().max()) < (2 ** 24 if flags & F else 256)
                if flags & ST:
                    s1, s2, _, _ = R.slot_reference(ref, 64)
                    top = max(top, float(s2.max()), float(s1.abs().max()))
                    assert float(s2.max()) * 4 < 2 ** 24 and torch.equal(s2, s2.float().double()) and torch.equal(s1, s1.float().double())    # (x 4: quarters, in the LN form)
                assert _int_equal(flags, c), (hex(flags), M, N, K)
    print(f"GEMM_REF integer constructions: largest partial {top:.0f} (2^24 = {2 ** 24})")


# worst ratios of the clean model (printed as GEMM_REF clean ...): fp32 output 0.086 randn, 0.146 outlier, 0.056 offset; bf16 output 0.999 / 1.000 / 0.998;
# gated 0.993 / 0.997 / 0.993; partials 0.071 / 0.065 / 0.070
@pytest.mark.parametrize("family", R.FAMILIES)
def test_clean_model_stays_inside_its_own_budget(family):
    """worst ratio per flag set, printed; every one <= 1.0"""
    worst, pre = {}, {}
    shapes = [(s, BUDGET) for s in _tiled_shapes() + _big_shapes() + _skinny_shapes()] + [(s, BUDGET_GLU) for s in _glu_shapes()]
    for (M, N, K), sets in shapes:
        if K % 64:
            sets = tuple(f for f in sets if not f & (LN | ST))          # (K = 32, 96 are shapes of the skinny kernels, which have neither)
        c = R.rand_case(family, M, N, K)
        for flags in sets:
            r = R.reference(flags, c)
            out, part = R.model(flags, c)
            q = R.ratio(out, r["ref"], r["bound"])
            assert q <= 1.0, (family, hex(flags), M, N, K, q, R.worst(out, r))
            worst[flags] = max(worst.get(flags, 0.0), q)
            pre[flags] = min(pre.get(flags, 1.0), r["pre"])
            if part is not None:
                qs = _stats_ratio(out, part, flags)
                assert qs <= 1.0, (family, hex(flags), M, N, K, "partials", qs)
                worst["partials"] = max(worst.get("partials", 0.0), qs)
    print(f"GEMM_REF clean {family}: " + "  ".join(f"{k if isinstance(k, str) else hex(k)} {v:.3f}" for k, v in worst.items()))
    print(f"GEMM_REF clean {family}: smallest fraction of elements with B below half a bf16 ulp: " + "  ".join(f"{hex(k)} {v:.2f}" for k, v in pre.items() if not k & F))


def test_budget_stays_where_the_arithmetic_puts_it_and_the_half_ulp_precondition_holds_above_it():
    """randn family, BIAS only (gemm_ref docstring): B <= K u (0.6366 sqrt K + 6.2) + 8 u on every element, and B is below half a bf16 ulp of the reference —
    the precondition of the bound B + half_ulp_bf16(ref) — on every element whose half ulp is above that cap: |ref| >= 2^-5 at K = 64, 0.5 at 512, 1 at 768 and 1024"""
    assert [min(2.0 ** e for e in range(-12, 4) if 2.0 ** (e - 9) > R.randn_budget_cap(K)) for K in (64, 512, 768, 1024)] == [2.0 ** -5, 0.5, 1.0, 1.0]
    seen = 0
    for (M, N, K) in _tiled_shapes() + _big_shapes() + [s for s in _skinny_shapes() if s[2] % 64 == 0]:
        r = R.reference(B, R.rand_case("randn", M, N, K))
        cap = R.randn_budget_cap(K)
        assert float(r["B"].max()) <= cap, (M, N, K, float(r["B"].max()), cap)
        hu = R.half_ulp_bf16(r["ref"])
        must = hu > cap
        assert bool((r["B"] < hu)[must].all()), (M, N, K)
        seen += int(must.sum())
    assert seen > 100000


# fault -> the checks that own it: (kind, flag set, input form / family, (M, N, K), rows of the plan's row tile).  Every shape is one of the GPU test's, and
# so are the inputs: the cases are generated on the CPU with the GPU test's seed and, where the GPU test runs one family per shape ("auto": the plain, the
# row-statistics and the gated forms), in that family; the LayerNorm-fold entry points run all three families at every shape.
OWNERS = {
    "drop_product": [("int", B | F, "dense", (65, 132, 192), 64), ("budget", F, "auto", (65, 132, 192), 64), ("budget", F, "auto", (127, 260, 1024), 128)],
    "drop_kstep_ragged": [("int", F, "dense", (65, 64, 192), 64), ("int", B, "sparse", (65, 64, 192), 64), ("budget", F, "auto", (129, 64, 1024), 128)],
    "bias_shift4": [("int", B, "sparse", (33, 64, 64), 64), ("int", B | F, "dense", (33, 64, 64), 64)],
    "residual_row16": [("int", B | RS | F, "dense", (33, 64, 64), 64), ("int", B | RS, "sparse", (33, 64, 64), 64), ("int", B | RS | LN | ST, "ln4", (33, 64, 64), 64)],
    "bf16_truncate": [("budget", B, "auto", (33, 64, 64), 64)],
    "tanh_gelu": [("budget", B | G, "auto", (33, 64, 64), 64), ("budget", B | G | LN, "randn", (33, 64, 64), 64)],
    "stats_unrounded": [("stats", B | RS | ST, "auto", (33, 132, 64), 64), ("stats", B | GLU | LN | ST, "auto", (33, 96, 64), 64)],
    "slot_pad_column": [("int", B | RS | ST, "sparse", (33, 132, 64), 64), ("stats", B | RS | ST, "auto", (33, 132, 64), 64)],
    "ln_neighbour_row": [("int", B | LN, "ln4", (33, 64, 64), 64), ("budget", B | LN, "offset", (33, 64, 64), 64)],
    "glu_swap": [("budget", B | GLU, "auto", (33, 96, 64), 64), ("budget", B | GLU | LN, "auto", (33, 96, 64), 64)],
    "relu_before_residual": [("int", B | RS | RELU, "sparse", (33, 64, 64), 64)],
}


def test_every_fault_has_an_owner_and_every_owner_shape_is_a_gpu_shape():
    assert set(OWNERS) == set(R.FAULTS)
    known = set(_tiled_shapes() + _big_shapes() + _skinny_shapes() + _glu_shapes())
    for owners in OWNERS.values():
        assert all(o[3] in known for o in owners)


@pytest.mark.parametrize("fault", R.FAULTS)
def test_seeded_fault_is_caught_by_the_check_that_owns_it(fault):
    for kind, flags, form, (M, N, K), BM in OWNERS[fault]:
        if kind == "int":
            c = R.int_case("sparse", M, N, K, nnz=4) if form == "ln4" else R.int_case(form, M, N, K)
            assert _int_equal(flags, c, BM=BM)
            assert not _int_equal(flags, c, fault=fault, BM=BM), (fault, hex(flags), M, N, K)
            print(f"GEMM_REF fault {fault}: caught by the exact-integer comparison, flags {hex(flags)} at {(M, N, K)}")
            continue
        c = R.rand_case(R.family_for(M, N, K) if form == "auto" else form, M, N, K)
        r = R.reference(flags, c)
        clean, cpart = R.model(flags, c, BM=BM)
        out, part = R.model(flags, c, fault=fault, BM=BM)
        if kind == "budget":
            q0, q = R.ratio(clean, r["ref"], r["bound"]), R.ratio(out, r["ref"], r["bound"])
        else:                                            # the row statistics against the values the launch stored
            q0, q = _stats_ratio(clean, cpart, flags), _stats_ratio(out, part, flags)
        assert q0 <= 1.0 and q > 1.25, (fault, kind, hex(flags), M, N, K, q0, q)
        print(f"GEMM_REF fault {fault}: {kind} ratio {q:.2f} (clean {q0:.3f}), flags {hex(flags)} at {(M, N, K)}")


def test_interleave_helper_is_the_layout_the_gated_reference_reads():
    g = torch.Generator().manual_seed(3)
    M, Fh, K = 5, 48, 64
    A = torch.randn(M, K, generator=g).to(torch.bfloat16)
    Wu, Wg = torch.randn(Fh, K, generator=g).to(torch.bfloat16), torch.randn(Fh, K, generator=g).to(torch.bfloat16)
    bu, bg = torch.randn(Fh, generator=g), torch.randn(Fh, generator=g)
    c = dict(A=A, W=R.interleave16(Wu, Wg), bias=R.interleave16(bu, bg))
    up, gate = A.double() @ Wu.double().t() + bu.double(), A.double() @ Wg.double().t() + bg.double()
    want = up * gate * torch.sigmoid(gate)
    assert torch.allclose(R.reference(B | GLU, c)["ref"], want, rtol=1e-13, atol=1e-13)

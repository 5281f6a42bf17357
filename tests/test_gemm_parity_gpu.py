"""The bf16 GEMM family against exact-integer expectations and a budgeted float64 reference (tests/gemm_ref.py), through the C ABI, on every tile plan
the default path can reach: the tiled kernels (csrc/gemm_bf16.hip, csrc/gemm_epilogue.h; mq_gemm_bf16 / _ln / _rs / _lnrs) at tile heights 2, 4, 5, 6,
the 256 x 256 tile and the default plan, and the skinny kernels (csrc/gemm_small.hip) in one row group and in several.

Shapes are the smallest at which a branch can go wrong: M one below / one above a row tile, N in {4, 64, 132, 260} (less than a lane group, one wave,
ragged last column tile and not a multiple of 8), K / 64 in {1, 2, 3, D, D + 1, 16} with D the LDS ring's depth.  Every flag set of mq_gemm_bf16, _rs,
_lnrs (residual form), mq_gemm_small_bf16 and the integer sets of _ln runs with ldc = N and with ldc = N + 4, fp32 and bf16 output alike (the fp32
residual lives at the same stride): the output is pre-filled, and the two guard rows and the four guard columns must keep their fill.  For bf16
one of the two strides is a multiple of 8 (16-byte stores, with the low-half branch where N % 8 == 4), the other is not (8-byte stores).  The gated
form runs with ldc = N / 2 (no guard columns) and ldc = N; the budgeted _ln cases run packed.

Integer cases must equal the integer reference (torch.equal); random cases stay within 1.25 x the per-element budget.  No element is skipped or masked.

Worst ratios seen on the MI355X (printed as GEMM_PARITY ...), accumulate constant c = 1:
    mq_gemm_bf16        fp32 out 0.053 (tiled), bf16 out 0.999, GLU 0.996;  the 256 x 256 tile 0.003 / 0.958 / 0.811
    mq_gemm_small_bf16  fp32 out 0.094, bf16 out 0.999
    mq_gemm_bf16_ln     0.999, GLU 0.996        mq_gemm_bf16_rs   stream 0.999, partials 0.036
    mq_gemm_bf16_lnrs   stream 1.000, GLU 0.996, partials 0.056
(a bf16 output next to a rounding tie uses the whole half ulp, as it must: the fp32 figures show the margin of the arithmetic itself)
    erf-GELU sweep 6.445e-05 absolute (contract 7e-5);  QuickGELU 1.163e-07 relative;  SiLU 0.0"""
import contextlib

import pytest
import torch

from marqo_amd import _lib as L
from tests import gemm_ref as R
from tests.knobs import tuned

pytestmark = pytest.mark.gpu

B, G, Q, RS, F, LN, GLU, RELU = R.BIAS, R.GELU, R.QUICK, R.RES, R.F32, R.LN, R.GLU, R.RELU
MARGIN = 1.25
FILL = 7.0
DEV = "cuda"

# flag sets: the exact-integer test runs all of INT_SETS, the budget test BUDGET_SETS
INT_SETS = (0, F, B, B | F, B | RS | F, B | RS, B | RELU, B | RS | RELU)
BUDGET_SETS = (F, B, B | G, B | Q, B | RS | F, B | RS)
LN_INT_SETS = (B, B | RELU)
LN_BUDGET_SETS = (B, B | G, B | Q)

PLANS = [("mt2", dict(gemm_nh=1, gemm_mt=2), 2), ("mt4", dict(gemm_nh=1, gemm_mt=4), 4), ("mt5", dict(gemm_nh=1, gemm_mt=5), 5), ("mt6", dict(gemm_nh=1, gemm_mt=6), 6),
         ("mt4_cgroup0", dict(gemm_nh=1, gemm_mt=4, gemm_cgroup=0), 4), ("mt4_cgroup8", dict(gemm_nh=1, gemm_mt=4, gemm_cgroup=8), 4),
         ("big", dict(gemm_nh=3), 8), ("default", dict(gemm_nh=0), 2)]    # (the default plan takes the 64-row tile for problems of one round)
PLAN_IDS = [p[0] for p in PLANS]


def _s():
    return torch.cuda.current_stream().cuda_stream


def plan(**kw):
    """the tiled family under the given knobs (the skinny kernels off); every knob back where it was afterwards"""
    return tuned(small_m=0, small_m_grouped=0, **kw)


def _probe_bits():
    """default-plan GEMMs whose bits depend on the kernel family that runs them: 40 rows (skinny), 200 (row groups), 400 (tiled).
    What this can see: small_m and small_m_grouped away from their defaults (the skinny kernels add the k-chunks in another order).  What it cannot:
    gemm_mt, gemm_nh and gemm_cgroup — every tiled plan gives the same bits by design (csrc/gemm_bf16.hip), so for those the guarantee is the
    try / finally of tests/knobs.tuned under plan(), which puts every key it set back whatever happened inside."""
    lib = L.load()
    g = torch.Generator(device=DEV).manual_seed(99)
    outs = []
    for M in (40, 200, 400):
        A = torch.randn(M, 768, device=DEV, generator=g).to(torch.bfloat16)
        W = (torch.randn(260, 768, device=DEV, generator=g) / 28).to(torch.bfloat16)
        b = torch.randn(260, device=DEV, generator=g)
        out = torch.empty(M, 260, device=DEV, dtype=torch.bfloat16)
        L.check(lib.mq_gemm_bf16(A.data_ptr(), 768, W.data_ptr(), 768, b.data_ptr(), 0, out.data_ptr(), 260, M, 260, 768, B, _s()))
        outs.append(out.view(torch.int16).cpu())
    return outs


@pytest.fixture(scope="module", autouse=True)
def knobs_back_at_their_defaults():
    before = _probe_bits()
    yield
    after = _probe_bits()
    assert all(torch.equal(a, b) for a, b in zip(before, after)), "a knob was left away from its default"


# ---- one launch through the C ABI, with guards ---------------------------------------------------------------------------------------------
def launch(entry, flags, c, ldc=None, lda=None):
    """runs one entry point on the case's operands; returns (out [M, Nout] as stored, partials [nslots, M, 2] or None).  Asserts that the guard rows,
    the guard columns (ldc > N) and the tail of the partials buffer keep their fill, and that every partial was written."""
    lib = L.load()
    A, W = c["A"], c["W"]
    M, K = A.shape
    N = W.shape[0]
    n_out = N // 2 if flags & GLU else N
    ldc = n_out if ldc is None else ldc
    if lda is not None:                                   # rows K apart become rows lda apart, the gap holds values that must not be read
        buf = torch.full((M, lda), 1.0e4, device=DEV, dtype=torch.bfloat16)
        buf[:, :K] = A
        A = buf
    lda = A.stride(0)
    f32 = bool(flags & F)
    out = torch.full((M + 2, ldc), FILL, device=DEV, dtype=torch.float32 if f32 else torch.bfloat16)
    res_ptr = 0
    if flags & RS:
        if f32:
            res = torch.full((M + 2, ldc), 1.0e4, device=DEV)
            res[:M, :N] = c["res"]
            res_ptr = res.data_ptr()
        else:                                             # the bf16 stream is updated in place
            out[:M, :N] = c["res"].to(torch.bfloat16)
            res_ptr = out.data_ptr()
    part = None
    if entry in ("rs", "lnrs"):
        ns = (N + 63) // 64
        part = torch.full((ns * M * 2 + 64,), float("nan"), device=DEV)
    stats = torch.stack([c["mean"], c["rstd"]], dim=1).contiguous() if entry in ("ln", "lnrs") else None
    a, w, bias = A.data_ptr(), W.data_ptr(), c["bias"].data_ptr() if flags & B else 0
    if entry == "gemm":
        rc = lib.mq_gemm_bf16(a, lda, w, K, bias, res_ptr, out.data_ptr(), ldc, M, N, K, flags, _s())
    elif entry == "small":
        rc = lib.mq_gemm_small_bf16(a, lda, w, K, bias, res_ptr, out.data_ptr(), ldc, M, N, K, flags, _s())
    elif entry == "ln":
        rc = lib.mq_gemm_bf16_ln(a, lda, w, K, bias, c["colsum"].data_ptr(), stats.data_ptr(), out.data_ptr(), ldc, M, N, K, flags, _s())
    elif entry == "rs":
        rc = lib.mq_gemm_bf16_rs(a, lda, w, K, bias, res_ptr, out.data_ptr(), ldc, M, N, K, flags, part.data_ptr(), _s())
    else:
        rc = lib.mq_gemm_bf16_lnrs(a, lda, w, K, bias, c["colsum"].data_ptr(), stats.data_ptr(), res_ptr, out.data_ptr(), ldc, M, N, K, flags, part.data_ptr(), _s())
    L.check(rc, f"{entry} flags={flags:#x} M={M} N={N} K={K}")
    what = (entry, hex(flags), M, N, K, ldc)
    assert bool((out[M:] == FILL).all()), ("rows past M were written", what)
    assert bool((out[:M, n_out:] == FILL).all()), ("columns past N were written", what)
    if part is not None:
        assert bool(torch.isnan(part[ns * M * 2:]).all()), ("partials past [nslots][M] were written", what)
        part = part[:ns * M * 2].view(ns, M, 2)
        assert not bool(torch.isnan(part).any()), ("a (row, slot) partial was not written", what)
    return out[:M, :n_out], part


def _ldcs(flags, n_out):
    """every flag set runs packed and with ldc = N + 4: guard columns for both output types, the fp32 residual at the same stride as the ABI defines;
    for bf16 one of the two strides is a multiple of 8 (16-byte stores) and the other is not"""
    return (n_out, n_out + 4)


def _ref_flags(entry, flags):
    return flags | (LN if entry in ("ln", "lnrs") else 0)


def check_int(entry, flags, c, BM, BN, ldc=None, lda=None):
    r = R.reference(_ref_flags(entry, flags), c)
    out, part = launch(entry, flags, c, ldc, lda)
    what = (entry, hex(flags), tuple(c["A"].shape), tuple(c["W"].shape), ldc, lda)
    assert torch.equal(out.double(), r["ref"]), (what, R.first_difference(out, r["ref"], BM, BN))
    if part is not None:
        s1, s2, _, _ = R.slot_reference(r["ref"], 64)
        assert torch.equal(part[..., 0].double(), s1) and torch.equal(part[..., 1].double(), s2), (what, "partials", R.first_difference(part[..., 0].t(), s1.t(), BM, 1))


def check_budget(entry, flags, c, seen, ldc=None, lda=None):
    r = R.reference(_ref_flags(entry, flags), c)
    out, part = launch(entry, flags, c, ldc, lda)
    what = (entry, hex(flags), tuple(c["A"].shape), tuple(c["W"].shape), ldc, lda)
    q = R.ratio(out, r["ref"], r["bound"])
    seen[(entry, flags)] = max(seen.get((entry, flags), 0.0), q)
    assert q <= MARGIN, (what, q, R.worst(out, r))
    if part is not None:
        s1, s2, b1, b2 = R.slot_reference(out, 32 if flags & GLU else 64)
        q1, q2 = R.ratio(part[..., 0], s1, b1), R.ratio(part[..., 1], s2, b2)
        seen[(entry, "partials")] = max(seen.get((entry, "partials"), 0.0), q1, q2)
        assert q1 <= MARGIN and q2 <= MARGIN, (what, "partials", q1, q2)


def _report(tag, seen):
    print(f"GEMM_PARITY {tag}: " + "  ".join(f"{e}/{f if isinstance(f, str) else hex(f)} {q:.3f}" for (e, f), q in sorted(seen.items(), key=str)))


def _tiled_shapes(name, mt):
    if name == "big":
        return [(M, N, K) for M in R.BIG_M for N in R.BIG_N for K in R.tiled_k(big=True)], [(M, 288, K) for M in R.BIG_M for K in R.tiled_k(big=True)]
    ms = R.tiled_m(mt)
    shapes = [(M, N, K) for M in ms for N in R.TILED_N for K in R.tiled_k()]
    if "cgroup" in name:                                  # the L2-grouped walk needs more than 8 column tiles and 16 row tiles: the smallest such problem
        shapes = [(M, N, K) for (M, N, K) in shapes if K in (64, 192)] + [(32 * mt * 15 + 1, 1028, 128)]
    return shapes, [(M, N, K) for M in ms for N in R.GLU_N for K in R.tiled_k()]


def _choose_mt(M, N):
    """the tile height of the default plan (csrc/gemm_sched.h, choose_mt: fewest rounds of 512 resident tiles times (height + 1.25))"""
    best, cost = 4, 1e30
    for mt in (2, 4, 5, 6):
        tiles = -(-M // (32 * mt)) * -(-N // 128)
        c = -(-tiles // 512) * (mt + 1.25)
        if c < cost - 1e-9:
            best, cost = mt, c
    return best


def _tile(name, mt, M, N, K, entry="gemm", flags=0):
    """(BM, BN) of the tile a launch runs on, for the failure text: the forced height, the default plan's choice, 5 instead of 6 for the residual
    form of _lnrs (csrc/gemm_bf16.hip, launch_narrow), 256 x 256 for the big tile"""
    if name == "big":
        return 256, 256
    if name == "default":
        mt = _choose_mt(M, N)
    if entry == "lnrs" and flags & RS and mt == 6:
        mt = 5
    return 32 * mt, 128


# ---- the tiled family ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,knobs,mt", PLANS, ids=PLAN_IDS)
def test_tiled_plans_give_the_exact_integers(name, knobs, mt):
    shapes, _ = _tiled_shapes(name, mt)
    with plan(**knobs):
        for (M, N, K) in shapes:
            BM, BN = _tile(name, mt, M, N, K)
            BM_lnrs = _tile(name, mt, M, N, K, "lnrs", B | RS)[0]
            dense, sparse, ln4 = R.int_case("dense", M, N, K, device=DEV), R.int_case("sparse", M, N, K, device=DEV), R.int_case("sparse", M, N, K, device=DEV, nnz=4)
            for flags in INT_SETS:
                for ldc in _ldcs(flags, N):
                    check_int("gemm", flags, dense if flags & F else sparse, BM, BN, ldc)
            for flags in LN_INT_SETS:
                for ldc in _ldcs(flags, N):
                    check_int("ln", flags, ln4, BM, BN, ldc)
            for ldc in _ldcs(B | RS, N):
                check_int("rs", B | RS, sparse, BM, BN, ldc)
                check_int("lnrs", B | RS, ln4, BM_lnrs, BN, ldc)
        # rows lda > K apart, once per output type
        M, N, K = shapes[len(shapes) // 2]
        BM, BN = _tile(name, mt, M, N, K)
        check_int("gemm", B | F, R.int_case("dense", M, N, K, device=DEV), BM, BN, ldc=N + 4, lda=K + 8)
        check_int("gemm", B | RS, R.int_case("sparse", M, N, K, device=DEV), BM, BN, ldc=N + 4, lda=K + 8)


@pytest.mark.parametrize("name,knobs,mt", PLANS, ids=PLAN_IDS)
def test_tiled_plans_stay_inside_the_budget(name, knobs, mt):
    shapes, glu_shapes = _tiled_shapes(name, mt)
    seen = {}
    with plan(**knobs):
        for (M, N, K) in shapes:
            c = R.rand_case(R.family_for(M, N, K), M, N, K, device=DEV)
            for flags in BUDGET_SETS:
                for ldc in _ldcs(flags, N):
                    check_budget("gemm", flags, c, seen, ldc)
            for fam in R.FAMILIES:
                cl = c if fam == R.family_for(M, N, K) else R.rand_case(fam, M, N, K, device=DEV)
                for flags in LN_BUDGET_SETS:
                    check_budget("ln", flags, cl, seen)
                check_budget("lnrs", B | RS, cl, seen)
            check_budget("rs", B | RS, c, seen)
        for (M, N, K) in glu_shapes:
            c = R.rand_case(R.family_for(M, N, K), M, N, K, device=DEV)
            for ldc in (N // 2, N):
                check_budget("gemm", B | GLU, c, seen, ldc)
                check_budget("ln", B | GLU, c, seen, ldc)
                check_budget("lnrs", B | GLU, c, seen, ldc)
        M, N, K = shapes[len(shapes) // 2]
        c = R.rand_case("randn", M, N, K, device=DEV)
        check_budget("gemm", B | F, c, seen, ldc=N + 4, lda=K + 8)
        check_budget("gemm", B | RS, c, seen, ldc=N + 4, lda=K + 8)
    _report(name, seen)


# ---- the skinny family -----------------------------------------------------------------------------------------------------------------------
def _skinny_tile(M):
    mt_all = (M + 15) // 16
    groups = (mt_all + 4) // 5
    return 16 * ((mt_all + groups - 1) // groups), 16


@pytest.mark.parametrize("M", R.SKINNY_M)
def test_skinny_kernels_give_the_exact_integers(M):
    BM, BN = _skinny_tile(M)
    for N in R.TILED_N:
        for K in R.SKINNY_K:
            dense = R.int_case("dense", M, N, K, device=DEV)
            sparse = R.int_case("sparse", M, N, K, device=DEV)
            for flags in INT_SETS:
                if flags == B | RS | RELU:                # (refused by the skinny entry point: the test below)
                    continue
                for ldc in _ldcs(flags, N):
                    check_int("small", flags, dense if flags & F else sparse, BM, BN, ldc)
    c = R.int_case("dense", M, 132, 192, device=DEV)
    check_int("small", B | F, c, BM, BN, ldc=136, lda=200)
    check_int("small", B | RS, R.int_case("sparse", M, 132, 192, device=DEV), BM, BN, ldc=136, lda=200)


def test_skinny_kernels_refuse_relu_on_top_of_a_residual():
    """MQ_EPI_BIAS | MQ_EPI_RESIDUAL | MQ_EPI_RELU is an epilogue of the tiled family only (mq_gemm_bf16 sends it there at any row count): the skinny
    entry point has to refuse it and leave the output alone, not run another epilogue in its place"""
    lib = L.load()
    c = R.int_case("sparse", 17, 64, 64, device=DEV)
    out = c["res"].to(torch.bfloat16)
    keep = out.clone()
    assert lib.mq_gemm_small_bf16(c["A"].data_ptr(), 64, c["W"].data_ptr(), 64, c["bias"].data_ptr(), out.data_ptr(), out.data_ptr(), 64, 17, 64, 64, B | RS | RELU, _s()) != 0
    torch.cuda.synchronize()
    assert torch.equal(out, keep)
    # ... and the public entry point computes it, on the tiled kernels, whatever the knobs say about small calls
    r = R.reference(B | RS | RELU, c)
    got, _ = launch("gemm", B | RS | RELU, c)
    assert torch.equal(got.double(), r["ref"]), R.first_difference(got, r["ref"], 128, 128)


@pytest.mark.parametrize("M", R.SKINNY_M)
def test_skinny_kernels_stay_inside_the_budget(M):
    seen = {}
    for N in R.TILED_N:
        for K in R.SKINNY_K:
            c = R.rand_case(R.family_for(M, N, K), M, N, K, device=DEV)
            for flags in BUDGET_SETS:
                for ldc in _ldcs(flags, N):
                    check_budget("small", flags, c, seen, ldc)
    c = R.rand_case("randn", M, 132, 192, device=DEV)
    check_budget("small", B | F, c, seen, ldc=136, lda=200)
    check_budget("small", B | RS, c, seen, ldc=136, lda=200)
    _report(f"skinny M={M}", seen)


# ---- activation isolation sweep ----------------------------------------------------------------------------------------------------------------
def _sweep_grid():
    """every bf16 value of magnitude 2^-9 .. 12, +-0, +-tiny, +-60, as rows of 64; with the fp32 offsets of `bias` the arguments cover [-12, 12] densely"""
    bits = torch.arange(0, 1 << 15, dtype=torch.int32)
    v = (bits << 16).view(torch.float32)
    v = v[(v >= 2.0 ** -9) & (v <= 12.0)]
    v = torch.cat([v, -v, torch.tensor([0.0, -0.0, 2.0 ** -120, -(2.0 ** -120), 1e-30, -1e-30, 60.0, -60.0])])
    pad = (-v.numel()) % 64
    v = torch.cat([v, v[:pad]])
    return v.view(-1, 64).to(torch.bfloat16).to(DEV)


def _sweep(kind):
    """(argument x as the kernel forms it — the exact fp32 a + b —, stored bf16 output) for kind in gelu / quick / silu, on the default plan"""
    lib = L.load()
    A = _sweep_grid()
    M, K, N = A.shape[0], 64, 512
    W = torch.zeros(N, K, device=DEV)
    W[torch.arange(N), torch.arange(N) % 64] = 1.0
    bias = ((torch.arange(N, device=DEV, dtype=torch.float32) * 0.6180339887) % 1.0 - 0.5) * 0.0625     # offsets up to half the widest bf16 gap (2^-4 near 12)
    x = A.float()[:, torch.arange(N, device=DEV) % 64] + bias[None, :]
    if kind == "silu":                                    # up = 0 + 1 exactly, gate = the grid: the stored product is silu(gate) rounded
        Wi, bi = R.interleave16(torch.zeros_like(W), W), R.interleave16(torch.ones_like(bias), bias)
        out = torch.full((M, N), FILL, device=DEV, dtype=torch.bfloat16)
        L.check(lib.mq_gemm_bf16(A.data_ptr(), K, Wi.to(torch.bfloat16).data_ptr(), K, bi.data_ptr(), 0, out.data_ptr(), N, M, 2 * N, K, B | GLU, _s()))
        return x, out
    out = torch.full((M, N), FILL, device=DEV, dtype=torch.bfloat16)
    L.check(lib.mq_gemm_bf16(A.data_ptr(), K, W.to(torch.bfloat16).data_ptr(), K, bias.data_ptr(), 0, out.data_ptr(), N, M, N, K, B | (G if kind == "gelu" else Q), _s()))
    return x, out


def _sweep_excess(kind):
    """(x, y float64, what |stored - y| leaves above half a bf16 ulp of y) per element"""
    x, out = _sweep(kind)
    xd = x.double()
    y = {"gelu": R._gelu64(xd), "quick": xd * torch.sigmoid(1.702 * xd), "silu": xd * torch.sigmoid(xd)}[kind]
    assert bool(torch.isfinite(out.float()).all())
    return xd, y, ((out.double() - y).abs() - R.half_ulp_bf16(y)).clamp(min=0)


def test_gelu_epilogue_keeps_the_contract_of_its_polynomial():
    """|gelu_erf2(x) - gelu(x)| <= 7e-5 (csrc/common.h) on a dense grid of arguments, read through the bf16 output with half an ulp allowed"""
    for tiled in (False, True):
        with (plan() if tiled else contextlib.nullcontext()):
            x, y, ex = _sweep_excess("gelu")
        i = int(ex.argmax())
        print(f"GEMM_PARITY gelu sweep (tiled={tiled}): {ex.numel()} arguments, worst |error| above half an ulp {float(ex.max()):.3e} at x = {float(x.flatten()[i])!r}")
        assert float(ex.max()) <= R.GELU_ABS


@pytest.mark.parametrize("kind", ["quick", "silu"])
def test_sigmoid_activations_keep_the_measured_relative_error(kind):
    """the measurement behind gemm_ref.QUICK_REL / SILU_REL: worst relative error of quick_gelu / silu against the float64 function where the function
    is at least 1e-30 in magnitude (below that: absolute, 1e-30).  The recorded figure must still hold, and twice it must stay below 2^-10."""
    worst = 0.0
    for tiled in (False, True):
        if kind == "silu" and not tiled:
            continue                                      # (the gated epilogue exists in the tiled family only)
        with (plan() if tiled else contextlib.nullcontext()):
            x, y, ex = _sweep_excess(kind)
        big = y.abs() >= R.ACT_FLOOR
        assert float(ex[~big].max() if bool((~big).any()) else 0.0) <= R.ACT_FLOOR
        rel = torch.where(big, ex / y.abs().clamp(min=R.ACT_FLOOR), torch.zeros_like(ex))
        i = int(rel.argmax())
        print(f"GEMM_PARITY {kind} sweep (tiled={tiled}): {ex.numel()} arguments, worst relative error above half an ulp {float(rel.max()):.3e} at x = {float(x.flatten()[i])!r}")
        worst = max(worst, float(rel.max()))
    recorded = R.QUICK_REL if kind == "quick" else R.SILU_REL
    assert recorded is not None and worst <= max(recorded, R.ACT_RESOLUTION) and 2 * recorded <= R.ACT_REL_LIMIT, (worst, recorded)

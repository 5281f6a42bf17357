"""The fp8 (e4m3) GEMM against exact-integer expectations and a budgeted float64 reference (tests/gemm_fp8_ref.py), through the C ABI (mq_gemm_fp8,
csrc/gemm_fp8.hip), on every tile plan: tile heights 2, 4, 5, 6, the L2-grouped walk off and on, the 192 x 256 tile of 8 waves and the default plan.

Shapes are the smallest at which a branch can go wrong: M one below / one above a row tile (and 33), N in {4, 64, 132, 260} (big tile: 260, 512),
K / 128 in {1, 2, 3, 8} (prologue only, equal to the two-stage ring, one past it, steady state), one dense integer case at K = 4096 per plan.  All six
epilogue forms run with per-row and with scalar a_scale.  The output is pre-filled: two guard rows, and guard columns where ldc > N, must keep their
fill.  fp32 output: ldc = N and N + 4, the fp32 residual at the same stride with its gap poisoned.  bf16 output: N and N + 4 (one of them a multiple of
8: the widened store with its low-half branch; the other the 8-byte store), the bf16 residual updated in place.  e4m3 output: ldc = N rounded up to 16
(the widened store, dword by dword at the ragged right edge), that + 4 (the narrow store) and the first again with the base 8 bytes off (narrow through
the alignment test); out_scale = max|ref| / 448 and 0.05.  w_scale and bias are followed by poisoned entries.  One pass per plan runs with lda = ldw =
K + 16, the gaps filled with the code of 448.

Integer cases must equal the integer reference (torch.equal); random cases stay within 1.25 x the per-element budget; every e4m3 code must be one of
the permitted codes of its element (none skipped or masked); amax must lie inside its bounds, keep a larger pre-set value and leave 0.

Worst ratios seen on the MI355X (printed as GEMM_FP8_PARITY ...):
    plan            OUT_F32  BIAS|RES|F32  BIAS (bf16)  BIAS|RES (bf16)   error / B_acc of OUT_F32
    mt2             0.352    0.352         0.992        0.994             0.352
    mt4             0.478    0.478         0.991        0.997             0.478
    mt5             0.382    0.382         0.990        0.995             0.382
    mt6             0.433    0.432         0.992        0.995             0.433
    mt4_cgroup0/8   0.500    0.500         0.996        0.998             0.500
    big (192 x 256) 0.433    0.432         0.994        0.997             0.433
    default         0.478    0.478         0.991        0.997             0.478
(C8 = 128; with C8 = 1 the fp32 form stood at 42.8 .. 58.5: tests/gemm_fp8_ref.py, MEASURED.  A bf16 output next to a rounding tie uses the whole half
ulp, as it must.  The two e4m3 forms have no ratio: every code was one of its element's permitted codes, every amax inside its bounds, and every
integer case exact, on every plan.)"""
import pytest
import torch

from marqo_amd import _lib as L
from tests import gemm_fp8_ref as R
from tests.knobs import tuned

pytestmark = pytest.mark.gpu

B, G, Q, RS, F, P8 = R.BIAS, R.GELU, R.QUICK, R.RES, R.F32, R.FP8
MARGIN = 1.25
FILL = 7.0
FILL8 = 0x55
GAP8 = 0x7E          # the code of 448: what lies between the rows of A and W where lda, ldw > K
DEV = "cuda"

PLANS = [("mt2", dict(gemm_nh=1, gemm_mt=2), 2), ("mt4", dict(gemm_nh=1, gemm_mt=4), 4), ("mt5", dict(gemm_nh=1, gemm_mt=5), 5), ("mt6", dict(gemm_nh=1, gemm_mt=6), 6),
         ("mt4_cgroup0", dict(gemm_nh=1, gemm_mt=4, gemm_cgroup=0), 4), ("mt4_cgroup8", dict(gemm_nh=1, gemm_mt=4, gemm_cgroup=8), 4),
         ("big", dict(gemm_mt=0, gemm_nh=3), 0), ("default", dict(), 0)]
PLAN_IDS = [p[0] for p in PLANS]

_CASES = {}


def _s():
    return torch.cuda.current_stream().cuda_stream


def case(kind, M, N, K):
    """one case per (kind, M, N, K), made on the CPU, kept on the GPU with its references"""
    key = (kind, M, N, K)
    if key not in _CASES:
        c = R.rand_case(R.family_for(M, N, K), M, N, K, device=DEV) if kind == "rand" else R.int_case(kind, M, N, K, device=DEV)
        c["_sw"] = torch.cat([c["sw"], torch.full((4,), R.SW_PAD, device=DEV)])
        c["_bias"] = torch.cat([c["bias"], torch.full((4,), R.BIAS_PAD, device=DEV)])
        _CASES[key] = c
    return _CASES[key]


def _probe_bits():
    """a default-plan fp8 GEMM whose bits a knob left behind could change only through a fault; what guarantees the knobs is the try / finally of
    tests/knobs.tuned (every tiled plan gives the same bits by design), this notices a library left in a state that no longer computes"""
    lib = L.load()
    g = torch.Generator(device=DEV).manual_seed(98)
    A8 = torch.randint(0, 0x78, (400, 256), dtype=torch.uint8, device=DEV, generator=g)
    W8 = torch.randint(0, 0x78, (260, 256), dtype=torch.uint8, device=DEV, generator=g)
    sa, sw = torch.rand(400, device=DEV, generator=g) + 0.5, torch.rand(260, device=DEV, generator=g) * 0.01
    out = torch.empty(400, 260, device=DEV)
    L.check(lib.mq_gemm_fp8(A8.data_ptr(), 256, W8.data_ptr(), 256, sa.data_ptr(), 1, sw.data_ptr(), 0, 0, out.data_ptr(), 260, 0, 0, 400, 260, 256, F, _s()))
    return out.view(torch.int32).cpu()


@pytest.fixture(scope="module", autouse=True)
def knobs_back_at_their_defaults():
    from tests.knobs import get
    keys = ("gemm_mt", "gemm_nh", "gemm_cgroup")
    was, before = {k: get(k) for k in keys}, _probe_bits()
    yield
    assert {k: get(k) for k in keys} == was, "a knob was left away from its default"
    assert torch.equal(before, _probe_bits())
    _CASES.clear()


# ---- one launch through the C ABI, with guards ---------------------------------------------------------------------------------------------
def _strided(codes, ld):
    buf = torch.full((codes.shape[0], ld), GAP8, dtype=torch.uint8, device=DEV)
    buf[:, :codes.shape[1]] = codes.view(torch.uint8)
    return buf


def launch(flags, c, rowscale, ldc, out_scale=None, amax0=0.0, base_off=0, pad_k=0):
    """runs mq_gemm_fp8 on the case's operands; returns (out [M, N] as stored — e4m3: the codes —, amax or None).  Asserts that the guard rows, the guard
    columns (ldc > N) and, for e4m3, the bytes around the buffer keep their fill."""
    lib = L.load()
    A, W = c["A"], c["W"]
    M, K = A.shape
    N = W.shape[0]
    if pad_k:
        key = ("_strided", pad_k)
        if key not in c:
            c[key] = (_strided(A, K + pad_k), _strided(W, K + pad_k))
        A, W = c[key]
    lda, ldw = A.stride(0), W.stride(0)
    res_ptr, amax, raw = 0, None, None
    if flags & P8:
        raw = torch.full(((M + 2) * ldc + 32,), FILL8, dtype=torch.uint8, device=DEV)
        out = raw[base_off:base_off + (M + 2) * ldc].view(M + 2, ldc)
        amax = torch.full((1,), amax0, device=DEV)
        osc = torch.full((1,), out_scale, device=DEV)
        fill = FILL8
    else:
        out = torch.full((M + 2, ldc), FILL, device=DEV, dtype=torch.float32 if flags & F else torch.bfloat16)
        fill = FILL
        if flags & RS:
            if flags & F:
                res = torch.full((M + 2, ldc), 1.0e4, device=DEV)
                res[:M, :N] = c["res"]
                res_ptr = res.data_ptr()
            else:                                             # the bf16 stream is updated in place
                out[:M, :N] = c["res"].to(torch.bfloat16)
                res_ptr = out.data_ptr()
    rc = lib.mq_gemm_fp8(A.data_ptr(), lda, W.data_ptr(), ldw, (c["sa"] if rowscale else c["sa1"]).data_ptr(), 1 if rowscale else 0, c["_sw"].data_ptr(),
                         c["_bias"].data_ptr() if flags & B else 0, res_ptr, out.data_ptr(), ldc, osc.data_ptr() if flags & P8 else 0, L.ptr(amax),
                         M, N, K, flags, _s())
    what = (hex(flags), "rowscale" if rowscale else "scalar", M, N, K, ldc, base_off, pad_k)
    L.check(rc, str(what))
    ok = (out[M:] == fill).all() & (out[:M, N:] == fill).all()
    if raw is not None:
        ok = ok & (raw[:base_off] == FILL8).all() & (raw[base_off + (M + 2) * ldc:] == FILL8).all()
    if not bool(ok):
        assert bool((out[M:] == fill).all()), ("rows past M were written", what)
        assert bool((out[:M, N:] == fill).all()), ("columns past N were written", what)
        raise AssertionError(("bytes around the output buffer were written", what))
    return out[:M, :N], (float(amax) if amax is not None else None)


def _strides(flags, N):
    """(ldc, byte offset of the base) per launch of a form"""
    if flags & P8:
        n16 = (N + 15) // 16 * 16
        return ((n16, 0), (n16 + 4, 0), (n16, 8))
    return ((N, 0), (N + 4, 0))


def _tile(name, mt, M, N):
    if name == "big" and N >= 256:
        return 192, 256
    if mt == 0:                                               # csrc/gemm_sched.h, choose_mt (the default plan keeps these small problems off the big tile)
        best, cost = 4, 1e30
        for cand in (2, 4, 5, 6):
            tiles = -(-M // (32 * cand)) * -(-N // 128)
            cst = -(-tiles // 512) * (cand + 1.25)
            if cst < cost - 1e-9:
                best, cost = cand, cst
        mt = best
    return 32 * mt, 128


def check(flags, c, rowscale, tile, seen, pad_k=0):
    """one form on one case at every stride (e4m3: and both out_scales): the exact-integer comparison or the budget, the code and amax checks"""
    M, K = c["A"].shape
    N = c["W"].shape[0]
    BM, BN = tile
    oscs = R.out_scales(flags, c, rowscale) if flags & P8 else (None,)
    if c.get("one_scale"):
        oscs = oscs[:1]
    for osc in oscs:
        r = R.reference(flags, c, rowscale, osc)
        strides = _strides(flags, N)[:1] if pad_k else _strides(flags, N)
        for ldc, off in strides:
            what = (hex(flags), "rowscale" if rowscale else "scalar", (M, N, K), "ldc", ldc, "offset", off, "out_scale", osc, "pad_k", pad_k)
            out, amax = launch(flags, c, rowscale, ldc, osc, base_off=off, pad_k=pad_k)
            if flags & P8:
                assert bool(R.codes_permitted(out, r["lo"], r["hi"]).all()), (what, R.first_bad_code(out, r, BM, BN))
                assert amax != 0.0 and R.amax_ok(amax, r), (what, "amax", amax, r["amax_lo"], r["amax_hi"])
            elif c["exact"]:
                assert torch.equal(out.double(), r["ref"]), (what, R.first_difference(out, r["ref"], BM, BN))
            else:
                q = R.ratio(out, r["ref"], r["bound"])
                seen[flags] = max(seen.get(flags, 0.0), q)
                if flags == F:
                    qa = R.ratio(out, r["ref"], r["B_acc"])
                    seen["acc"] = max(seen.get("acc", 0.0), qa)
                assert q <= MARGIN, (what, q, R.worst(out, r), R.tile_coords(*divmod(int(((out.double() - r["ref"]).abs() / r["bound"]).argmax()), N), BM, BN))
        if flags & P8:                                        # a cell pre-set above the maximum keeps its value: the kernel takes a maximum
            keep = float(torch.tensor(2.0 * r["amax_hi"] + 1.0, dtype=torch.float32))
            _, amax = launch(flags, c, rowscale, _strides(flags, N)[0][0], osc, amax0=keep, pad_k=pad_k)
            assert amax == keep, (hex(flags), (M, N, K), "amax pre-set to", keep, "became", amax)


def _shapes(name, mt):
    if name == "big":
        return R.big_shapes()
    shapes = R.tiled_shapes(mt if mt else 4)
    if "cgroup" in name:
        shapes = shapes + [R.cgroup_shape(mt)]
    return shapes


def _int_case_for(flags, M, N, K):
    return case("dense" if flags & F else "sparse_pos" if flags & P8 else "sparse", M, N, K)


def _report(name, kind, seen):
    print(f"GEMM_FP8_PARITY {name} {kind} worst ratio: " + "  ".join(f"{k if isinstance(k, str) else hex(k)} {q:.3f}" for k, q in sorted(seen.items(), key=str)))


@pytest.mark.parametrize("name,knobs,mt", PLANS, ids=PLAN_IDS)
def test_plans_give_the_exact_integers(name, knobs, mt):
    shapes = _shapes(name, mt)
    with tuned(**knobs):
        for (M, N, K) in shapes:
            tile = _tile(name, mt, M, N)
            for flags in R.FORMS:
                for rowscale in (True, False):
                    check(flags, _int_case_for(flags, M, N, K), rowscale, tile, {})
            one = case("sparse_one", M, N, K)                 # (tests/gemm_fp8_ref.py: the case that tells tanh-GELU from erf-GELU)
            one["one_scale"] = True
            check(B | G | P8, one, True, tile, {})
        # long K: one dense integer case
        M, N = (193, 260) if name == "big" else (32 * (mt if mt else 4) + 1, 132)
        for flags in (F, B | RS | F):
            for rowscale in (True, False):
                check(flags, case("dense", M, N, R.LONG_K), rowscale, _tile(name, mt, M, N), {})
        # rows lda = ldw = K + 16 apart
        M, N, K = shapes[len(shapes) // 2]
        for flags in R.FORMS:
            for rowscale in (True, False):
                check(flags, _int_case_for(flags, M, N, K), rowscale, _tile(name, mt, M, N), {}, pad_k=16)


@pytest.mark.parametrize("name,knobs,mt", PLANS, ids=PLAN_IDS)
def test_plans_stay_inside_the_budget(name, knobs, mt):
    shapes = _shapes(name, mt)
    seen = {}
    with tuned(**knobs):
        for (M, N, K) in shapes:
            c = case("rand", M, N, K)
            for flags in R.FORMS:
                for rowscale in (True, False):
                    check(flags, c, rowscale, _tile(name, mt, M, N), seen)
        M, N, K = shapes[len(shapes) // 2]
        for flags in R.FORMS:
            for rowscale in (True, False):
                check(flags, case("rand", M, N, K), rowscale, _tile(name, mt, M, N), seen, pad_k=16)
    _report(name, "budget", seen)

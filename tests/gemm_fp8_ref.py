"""Reference, rounding budgets, inputs and a CPU model with single seeded faults for the tests of the fp8 (OCP e4m3) GEMM (csrc/gemm_fp8.hip,
mq_gemm_fp8): tests/test_gemm_fp8_ref_host.py, tests/test_gemm_fp8_parity_gpu.py.  A plain helper module: nothing here calls the library.
half_ulp_bf16, ratio, _gen, tile_coords, first_difference, the flag constants and the measured activation constants are tests/gemm_ref.py's.
e4m3 is torch.float8_e4m3fn, encoded and decoded on the CPU; no operand holds a NaN code ((c & 0x7F) == 0x7F).  Inputs are made on the CPU with
seeded generators and moved, so the host test and the GPU test see the same data.

    out[m, n] = epi( (sum_k a_mk w_nk) * sa * sw_n ),   sa = a_scale[m] (per row) or a_scale[0] (scalar)

EXACT-INTEGER INPUTS (int_case).  A and W hold integers in [-4, 4] as e4m3 codes: each is exact in e4m3, every product is an integer of |p| <= 16.
a_scale per row is in {1, 2} (or the scalar 2), w_scale per column in {0.5, 1}: s = sa sw is in {0.5, 1, 2}, a power of two, exact.
  dense  (fp32 output), K <= 4096: |acc| <= 16 K = 65 536, |s acc| <= 2^17; + an integer bias in [-8, 8] + an integer fp32 residual in [-64, 64]:
         far below 2^24, exact whatever the order of the additions.
  sparse (bf16 output): every row of A has at most nnz = 4 non-zeros, the j-th of row m in k-step (m + j * max(nk // 8, 1)) % nk (nk = K / 128) at a
         seeded random position of that step, so the rows together reach every k-step.  |acc| <= 64, so |s acc| <= 128.
         s = 2:   an integer of |v| <= 128 + 8 + 64 = 200 < 256.
         s = 1:   an integer of |v| <= 64 + 8 + 64 = 136.
         s = 0.5: a multiple of 1/2 with |v| <= 32 + 8 + 64 = 104 < 128.
         Either way at most 8 significant bits: every stored bf16 is exact.  (No (sa, sw) pair has to be left out for that: s = 2 is the first line.)
  All operands are seeded random integers, unrelated from row to row and column to column: a transposed, shifted or neighbouring read of A, W,
  a_scale, w_scale, bias or residual does not reproduce the answer.
  The scaled MFMA aligns the 128 products of a block before it adds them.  With |p| <= 16 and a block sum <= 2048 any internal width of 12 bits or
  more keeps a block exact (what the MI355X did: MEASURED).
  Behind an activation (the two e4m3-output forms) the sparse inputs give an exact pre-activation value of |x| <= 136, so B is the activation's
  own term alone: the sharpest e4m3 cases.  (The 7e-5 of the erf-GELU polynomial holds there: beyond its clamp at +-4.5 Phi stays within 1.4e-7
  of 0 / 1, which is 1.9e-5 at |x| = 136.)

RANDOM INPUTS WITH A PER-ELEMENT BUDGET (rand_case, reference).  u = 2^-24.  Families:
    randn    A = e4m3(N(0, 1)), W = e4m3(N(0, 1)), w_scale about 1 / sqrt K
    codes    uniform over the finite codes with the top exponent bit cleared (magnitudes 2^-9 .. 1.875), as tests/test_fp8_gpu.py has them
    outlier  randn with one column of A at 40
a_scale in [0.5, 1.5] (scalar: 0.75), w_scale in [0.5, 1.5] / sqrt K, bias 0.5 N(0, 1) + 1 (the offset: E4M3 OUTPUT below), residual 2 N(0, 1) + 0.5.  The reference is float64 on the
decoded operands.  e4m3 x e4m3 products are exact in fp32; the hardware's block sum of 128 aligned products does not round once per addition, so
the accumulate budget has two terms — the alignment of a block's products to its largest one, and the K / 128 fp32 additions of block sums:
    B_acc = s ( C8 u sum_blocks 128 max_{k in block} |a_mk w_nk|  +  (K / 128) u sum_k |a_mk w_nk| )          C8: MEASURED
Every further operation adds u |result| and passes the incoming budget on, as in tests/gemm_ref.py:
    scaling    x = acc (sa sw):        B = B_acc + 2 u |x|          (the product of the scales and the product with it)
    bias, residual                     B = B + u |x|
    erf-GELU                           B = 1.13 B + 7e-5
    QuickGELU                          B = 1.10 B + 2 max(QUICK_REL, ACT_RESOLUTION) |y| + 1e-30
    bf16 output                        bound = B + half a bf16 ulp, in the two forms of gemm_ref.reference
On the exact-integer inputs B_acc and the scaling, bias and residual terms are 0 (every one of those operations is exact).
K <= 1024 in the budgeted cases; long K (4096) belongs to the exact-integer test, for the reason gemm_ref.py gives.

E4M3 OUTPUT.  No element is skipped or masked, near-ties included.  The kernel's value before the division lies in [ref - B, ref + B]; the kernel
multiplies by fl(1 / out_scale) (a correctly rounded reciprocal and one product: 2 u relative, added to B), clamps to +-448 and rounds to nearest
even.  Rounding is monotonic, so the stored code must lie, in value order, between RNE(clamp448((ref - B) / out_scale)) and
RNE(clamp448((ref + B) / out_scale)): permitted_codes returns the two ends (rounded in float64 by the definition of the format, not through a
float32 conversion), codes_permitted tests membership by decoded value (+0 and -0 are one value; a NaN code is never permitted).
out_scale is max|ref| / 448 and a fixed 0.05: never 1, never a power of two alone.  `determined` is the share of elements whose interval is a
single value; the host test asserts >= 0.70 on every case the GPU test uses (MEASURED: the smallest per family).  The erf-GELU's 7e-5 absolute is
more than half the smallest e4m3 step at out_scale 0.05 (2^-10 x 0.05 = 4.9e-5), so an output of gelu(x) = 0 for x << 0 has three permitted values
(-2^-9, 0, 2^-9).  With symmetric integer sums half the outputs are such, and the `outlier` column at 40 made them 40 % (shares 0.39 and 0.60).  So the
inputs of those cases — not the cap — lean positive: the integer form behind an activation (`sparse_pos`) has A's non-zeros in [1, 4] and W's
values below -1 mirrored (W in {-1, 0, 1} once, {2, 3, 4} twice as often), the weights that meet the outlier column are positive, and the
random families' bias has an offset of 1 (with C8 = 128 and a bias centred on 0 the small negative GELU outputs of the N = 4 cases brought
`randn` to 0.68 and `outlier` to 0.66).
What that costs: with sums that large almost every GELU argument is beyond +-4.5, where tanh-GELU and erf-GELU agree, and on the random cases their
difference (<= 4.7e-4) hides behind the e4m3 step.  Fault (i) is visible only where x is in about [-3.5, -2.5] (relative difference 2 .. 30 %).  So the
erf-GELU form runs one more integer case, `sparse_one`: sparse_pos with ONE non-zero per row and a bias in [-2, 2] (with [-8, 8] every column of
bias <= -5 is one of the three-valued zeros above: share 0.45), x = s a w + bias spread over the half-integers of [-10, 34].  It runs with
out_scale = max|ref| / 448 and per-row a_scale only (the scalar 2 doubles every product and with it the share of three-valued zeros).
amax: max(|ref| - B) <= amax <= max(|ref| + B) over the valid elements (B before the division); a cell pre-set above that keeps its value, a
cell pre-set to 0 does not stay 0.

MEASURED on the MI355X (gfx950) by tests/test_gemm_fp8_parity_gpu.py:
    exact integers   every plan, form and shape gave the exact integers with operands in [-4, 4], K = 128 .. 4096: the block sum of 128 aligned products
                     kept them whole, the value range was not narrowed.
    C8 = 128         the first run of the plain fp32-output form (flags OUT_F32) with C8 = 1 gave a worst error / B_acc of 42.8 .. 58.5 by plan (the plans
                     differ in their shapes, not in their bits: the same shape gave the same ratio on each), 15.6 already at (33, 4, 128) — on every plan
                     alike, so this is the hardware's block arithmetic.  Solved for the constant, (error - the other terms) / (s u sum_blocks 128 max|a w|)
                     was at most 63.9 (`codes`, (1921, 1028, 128), scalar a_scale; 61.1 at (129, 132, 128); 48.6 in `outlier` at K = 1024): the aligned
                     products keep about 24 - 6 = 18 bits below the block's largest.  C8 = the next power of two above 2 x 63.9 = 128 = 2^7, inside the
                     2^8 limit.  Worst ratios with it: the docstring of tests/test_gemm_fp8_parity_gpu.py.
    determined       smallest share of e4m3 elements with a single permitted value, per family, with C8 = 128 (tests/test_gemm_fp8_ref_host.py prints
                     it): randn 0.818, codes 0.917, outlier 0.873, integer 0.719, one-non-zero integer 0.709.

MODEL.  model(): torch fp32 on the CPU in the kernel's order — the matmul of the decoded operands, v * (sa * sw), bias, activation, residual,
round-to-nearest-even bf16 or clamp448(v * fl(1 / out_scale)) -> e4m3 — with switchable single faults (FAULTS), each confined to one element or
one 16 x 16 sub-tile.  sw and bias are read through 4 poisoned entries past N (SW_PAD, BIAS_PAD: the GPU test lays the same poison behind them):
    (a) drop_product          one product missing from one element
    (b) drop_kstep_ragged     the last k-step (128) missing on the ragged last row tile, one sub-tile wide
    (c) swap_kchunks          two 16-byte k-chunks of one A row exchanged (a swizzle slip)
    (d) a_scale_row1          a_scale of row m + 1
    (e) w_scale_shift4        w_scale read 4 columns off
    (f) bias_shift4           bias read 4 columns off
    (g) residual_row16        residual of row m + 16
    (h) bf16_truncate         truncation instead of round-to-nearest
    (i) tanh_gelu             tanh-GELU in place of erf-GELU
    (j) gelu_for_quick        erf-GELU where QuickGELU is asked
    (k) fp8_truncate          e4m3 truncation instead of round-to-nearest-even
    (l) fp8_swap_halves       the two 8-code halves of one 16-column group exchanged in the e4m3 store
    (m) fp8_multiply_scale    value times out_scale instead of divided by it
    (n) scalar_reads_row      scalar mode reading a_scale[m] instead of a_scale[0]
    (o) amax_pad_column       amax taken over a clamped pad column as well (weight row N - 1, scale and bias from behind the arrays)
Owners (tests/test_gemm_fp8_ref_host.py): (a), (b), (c), (n) the exact-integer comparison (and more); (h), (k), (l), (m) the stored-value and code
checks; (o) the amax bounds; the rest either.
"""
import torch

from tests.gemm_ref import (ACT_FLOOR, BIAS, F32, GELU, GELU_ABS, LIP_GELU, LIP_SIG, QUICK, QUICK_REL, RES, U, _act_rel, _gelu64, _gen, _randint,   # noqa: F401
                            first_difference, half_ulp_bf16, ratio, tile_coords)

FP8 = 32             # MQ_EPI_OUT_FP8 (include/marqo_hip.h)
E4M3 = torch.float8_e4m3fn
C8 = 128             # the block-alignment constant of B_acc; see MEASURED
C8_LIMIT = 2 ** 8    # above this (fewer than 16 aligned bits) the figure is a finding, not a budget
FIXED_OUT_SCALE = 0.05
SW_PAD, BIAS_PAD = 16.0, 3.0      # what lies in the 4 entries behind w_scale and bias

FAMILIES = ("randn", "codes", "outlier")
FAULTS = ("drop_product", "drop_kstep_ragged", "swap_kchunks", "a_scale_row1", "w_scale_shift4", "bias_shift4", "residual_row16", "bf16_truncate", "tanh_gelu",
          "gelu_for_quick", "fp8_truncate", "fp8_swap_halves", "fp8_multiply_scale", "scalar_reads_row", "amax_pad_column")
# the six epilogue forms of mq_gemm_fp8
FORMS = (F32, BIAS, BIAS | GELU | FP8, BIAS | QUICK | FP8, BIAS | RES | F32, BIAS | RES)

# ---- the shapes of the GPU test (the host test runs on these) ---------------------------------------------------------------------------------
TILED_MT = (2, 4, 5, 6)
TILED_N = (4, 64, 132, 260)
BIG_M, BIG_N = (191, 193, 385), (260, 512)
KS = (128, 256, 384, 1024)        # K / 128 = 1, 2, 3, 8: prologue only, equal to the two-stage ring, one past it, steady state
LONG_K = 4096


def tiled_m(mt):
    return (33, 32 * mt - 1, 32 * mt + 1)


def tiled_shapes(mt):
    return [(M, N, K) for M in tiled_m(mt) for N in TILED_N for K in KS]


def big_shapes():
    return [(M, N, K) for M in BIG_M for N in BIG_N for K in KS]


def cgroup_shape(mt):
    """the smallest problem the L2-grouped walk takes: more than 8 column tiles and 16 row tiles (csrc/gemm_sched.h, set_tiles_m)"""
    return (32 * mt * 15 + 1, 1028, 128)


def family_for(M, N, K):
    return FAMILIES[(M + N // 4 + K // 128) % 3]


# ---- e4m3 -------------------------------------------------------------------------------------------------------------------------------------
def decode(codes):
    """uint8 codes -> float64 values (NaN for the two NaN codes)"""
    return codes.view(E4M3).float().double()


def encode(x):
    """values exactly representable in e4m3 -> uint8 codes"""
    c = x.float().cpu().to(E4M3)                     # (the conversion runs on the CPU wherever x lives)
    assert torch.equal(c.float(), x.float().cpu()), "encode(): a value is not an e4m3 value"
    return c.view(torch.uint8).to(x.device)


def rne_e4m3(x):
    """float64 -> the nearest e4m3 value (ties to the even mantissa), float64; |x| <= 448.  By the definition of the format: 3 mantissa bits, the
    smallest normal binade 2^-6, below it the subnormals' quantum 2^-9"""
    ax = x.abs()
    _, e = torch.frexp(ax)                                  # ax = m 2^e, m in [0.5, 1): the binade is 2^(e - 1)
    q = torch.ldexp(torch.ones_like(ax), (e - 1).clamp(min=-6) - 3)
    return torch.copysign(torch.round(ax / q) * q, x)       # (torch.round: half to even)


def permitted_codes(ref, B, out_scale):
    """(lo, hi) uint8: the codes of RNE(clamp448((ref - B) / out_scale)) and RNE(clamp448((ref + B) / out_scale))"""
    lo = rne_e4m3(((ref.double() - B) / out_scale).clamp(-448, 448))
    hi = rne_e4m3(((ref.double() + B) / out_scale).clamp(-448, 448))
    return encode(lo), encode(hi)


def codes_permitted(codes, lo, hi):
    """bool per element: the stored code's value lies between the two ends' values (a NaN code: never)"""
    v = decode(codes)
    return (decode(lo) <= v) & (v <= decode(hi))


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------------
def _to(c, device):
    return {k: (v.to(device) if isinstance(v, torch.Tensor) else v) for k, v in c.items()}


def int_case(form, M, N, K, seed=0, device="cpu", nnz=4):
    """exact-integer operands (module docstring): dict A, W (e4m3), sa [M], sa1 [1], sw [N], bias [N], res [M, N] (fp32; the bf16 residual is
    res.bfloat16(), exact), exact = True"""
    g = _gen(17, M, N, K, seed, nnz)
    W = _randint(-4, 4, (N, K), g, "cpu")
    if form == "dense":
        assert K <= 4096
        A = _randint(-4, 4, (M, K), g, "cpu")
    else:
        assert form in ("sparse", "sparse_pos", "sparse_one") and K % 128 == 0
        if form != "sparse":                           # (behind an activation: mostly positive sums, module docstring)
            W = torch.where(W < -1, -W, W)
            nnz = 1 if form == "sparse_one" else nnz
        nk = K // 128
        A = torch.zeros(M, K, dtype=torch.int64)
        rows = torch.arange(M)
        for j in range(nnz):
            step = (rows + j * max(nk // 8, 1)) % nk
            pos = _randint(0, 127, (M,), g, "cpu")
            val, sign = _randint(1, 4, (M,), g, "cpu"), 2 * _randint(0, 1, (M,), g, "cpu") - 1
            A[rows, step * 128 + pos] = val * sign if form == "sparse" else val
    lim = 2 if form == "sparse_one" else 8
    sa = torch.tensor([1.0, 2.0])[_randint(0, 1, (M,), g, "cpu")]
    sw = torch.tensor([0.5, 1.0])[_randint(0, 1, (N,), g, "cpu")]
    return _to(dict(A=A.float().to(E4M3), W=W.float().to(E4M3), sa=sa, sa1=torch.tensor([2.0]), sw=sw, bias=_randint(-lim, lim, (N,), g, "cpu").float(),
                    res=_randint(-64, 64, (M, N), g, "cpu").float(), exact=True), device)


def rand_case(family, M, N, K, seed=0, device="cpu"):
    """random operands of one family (module docstring); exact = False"""
    g = _gen(19, M, N, K, seed, FAMILIES.index(family))
    if family == "codes":
        ops = []
        for rows in (M, N):
            c = torch.randint(0, 256, (rows, K), generator=g, dtype=torch.uint8)
            c[(c & 0x7F) == 0x7F] = 0x30
            ops.append((c & 0xBF).view(E4M3))
        A, W = ops
    else:
        a = torch.randn(M, K, generator=g)
        if family == "outlier":
            a[:, (3 * K) // 7] = 40.0
        w = torch.randn(N, K, generator=g)
        if family == "outlier":                          # (its weights positive: module docstring, E4M3 OUTPUT)
            w[:, (3 * K) // 7] = w[:, (3 * K) // 7].abs()
        A, W = a.to(E4M3), w.to(E4M3)
    sa = torch.rand(M, generator=g) + 0.5
    sw = (torch.rand(N, generator=g) + 0.5) / K ** 0.5
    return _to(dict(A=A, W=W, sa=sa, sa1=torch.tensor([0.75]), sw=sw, bias=0.5 * torch.randn(N, generator=g) + 1.0, res=2.0 * torch.randn(M, N, generator=g) + 0.5,
                    exact=False), device)


def residual_of(flags, c):
    return c["res"] if flags & F32 else c["res"].to(torch.bfloat16)


# ---- reference and budgets --------------------------------------------------------------------------------------------------------------------
def _sums64(c):
    """float64 acc = A W^T, S = |A| |W|^T and P = sum over the 128-blocks of 128 max_k |a w| (fp32 products of e4m3 values are exact), cached"""
    if "_acc64" not in c:
        A, W = c["A"], c["W"]
        Ad, Wd = A.float().double(), W.float().double()
        c["_acc64"], c["_S"] = Ad @ Wd.t(), Ad.abs() @ Wd.abs().t()
        if c["exact"]:
            c["_P"] = None
        else:
            Af, Wf = A.float().abs(), W.float().abs()
            M, K = Af.shape
            N = Wf.shape[0]
            P = torch.zeros(M, N, dtype=torch.float64, device=Af.device)
            rows = max(1, (1 << 22) // N)                                  # M x N x 128 products at a time, at most 2^29 of them
            for b in range(K // 128):
                wb = Wf[None, :, b * 128:(b + 1) * 128]
                for r0 in range(0, M, rows):
                    P[r0:r0 + rows] += (Af[r0:r0 + rows, None, b * 128:(b + 1) * 128] * wb).amax(-1).double()
            c["_P"] = 128.0 * P
    return c["_acc64"], c["_S"], c["_P"]


def out_scales(flags, c, rowscale):
    """the two out_scale values of an e4m3-output launch: max|ref| / 448 (as the fp32 the kernel receives) and 0.05"""
    r = reference(flags & ~FP8 | F32, c, rowscale)["ref"]
    return (float(torch.tensor(float(r.abs().max()) / 448.0, dtype=torch.float32)), float(torch.tensor(FIXED_OUT_SCALE, dtype=torch.float32)))


def reference(flags, c, rowscale=True, out_scale=None, c8=None):
    """float64 reference and budget of one form on a case: dict ref, B (before the output rounding), bound (fp32: B; bf16: B + half an ulp), B_acc;
    e4m3 output: lo, hi (permitted_codes), determined (share of single-value intervals), amax_lo, amax_hi"""
    key = ("_r", flags, rowscale, out_scale, c8)
    if key in c:
        return c[key]
    acc, S, P = _sums64(c)
    K = c["A"].shape[1]
    sa = c["sa"].double()[:, None] if rowscale else c["sa1"].double().reshape(1, 1)
    s = sa * c["sw"].double()[None, :]
    x = s * acc
    if c["exact"]:
        B_acc = torch.zeros_like(x)
        B = B_acc
        rnd = 0.0                                                          # scaling, bias and residual are exact there
    else:
        B_acc = s * ((C8 if c8 is None else c8) * U * P + (K // 128) * U * S)
        B = B_acc + 2 * U * x.abs()
        rnd = U
    if flags & BIAS:
        x = x + c["bias"].double()[None, :]
        B = B + rnd * x.abs()
    if flags & GELU:
        x, B = _gelu64(x), LIP_GELU * B + GELU_ABS
    if flags & QUICK:
        x = x * torch.sigmoid(1.702 * x)
        B = LIP_SIG * B + _act_rel(QUICK_REL, "QUICK_REL") * x.abs() + ACT_FLOOR
    if flags & RES:
        x = x + residual_of(flags, c).double()
        B = B + rnd * x.abs()
    if flags & F32:
        r = dict(ref=x, B=B, bound=B, B_acc=B_acc)
    elif flags & FP8:
        assert out_scale is not None
        Bq = B + 2 * U * (x.abs() + B)
        lo, hi = permitted_codes(x, Bq, out_scale)
        r = dict(ref=x, B=B, bound=Bq, B_acc=B_acc, lo=lo, hi=hi, determined=float((decode(lo) == decode(hi)).double().mean()),
                 amax_lo=float((x.abs() - B).max()), amax_hi=float((x.abs() + B).max()))
    else:
        hu = half_ulp_bf16(x)
        r = dict(ref=x, B=B, bound=B + torch.where(B < hu, hu, half_ulp_bf16(x.abs() + B)), B_acc=B_acc)
    c[key] = r
    return r


def worst(got, r):
    """text: the worst element of a budgeted comparison, its coordinates and budget terms"""
    err = (got.double() - r["ref"]).abs() / r["bound"]
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    i = int(err.argmax())
    m, n = divmod(i, err.shape[1])
    return (f"worst (m={m}, n={n}): got {float(got[m, n])!r} ref {float(r['ref'][m, n])!r} B_acc {float(r['B_acc'][m, n]):.3e} B {float(r['B'][m, n]):.3e} "
            f"bound {float(r['bound'][m, n]):.3e}")


def first_bad_code(codes, r, BM, BN):
    """text for a failed permitted-code check: how many, the first one, where it sits in the tile plan"""
    bad = ~codes_permitted(codes, r["lo"], r["hi"])
    idx = torch.nonzero(bad)
    if idx.numel() == 0:
        return "every code permitted"
    m, n = int(idx[0, 0]), int(idx[0, 1])
    return (f"{int(bad.sum())} of {bad.numel()} codes outside their interval, first at (m={m}, n={n}): got {int(codes[m, n]):#04x} = {float(decode(codes[m, n])):g}, "
            f"permitted {float(decode(r['lo'][m, n])):g} .. {float(decode(r['hi'][m, n])):g} (ref {float(r['ref'][m, n])!r}, B {float(r['bound'][m, n]):.3e}); "
            f"{tile_coords(m, n, BM, BN)}")


def amax_ok(amax, r):
    return r["amax_lo"] <= amax <= r["amax_hi"]


# ---- the CPU model with single faults -----------------------------------------------------------------------------------------------------------
def _truncate_bf16(v):
    return (v.contiguous().view(torch.int32) & -65536).view(torch.float32)


def _truncate_e4m3(x):
    """float32 (|x| <= 448) -> e4m3 value towards zero"""
    ax = x.double().abs()
    _, e = torch.frexp(ax)
    q = torch.ldexp(torch.ones_like(ax), (e - 1).clamp(min=-6) - 3)
    return torch.copysign(torch.floor(ax / q) * q, x.double()).float()


def _quick32(v):
    return v * torch.sigmoid(1.702 * v)


def model(flags, c, rowscale=True, out_scale=None, fault=None, BM=64):
    """torch fp32 model of one launch on the CPU: dict out (float32 [M, N]: the stored fp32 / bf16 values, or the decoded e4m3 codes), codes (uint8, e4m3
    output only), amax (float, e4m3 output only).  BM = rows of the plan's row tile (it only places fault (b))."""
    assert fault is None or fault in FAULTS
    if "_A32" not in c:
        c["_A32"], c["_W32"] = c["A"].float().cpu(), c["W"].float().cpu()
        c["_acc32"] = c["_A32"] @ c["_W32"].t()
    A, W = c["_A32"], c["_W32"]
    M, K = A.shape
    N = W.shape[0]
    rows, cols = slice(0, min(16, M)), slice(0, min(16, N))          # the sub-tile a fault lives in
    ridx, cidx = torch.arange(rows.stop), torch.arange(cols.stop)
    acc = c["_acc32"].clone()
    if fault == "drop_product":
        m, n = min(M - 1, 5), min(N - 1, 3)
        k = int((A[m] * W[n]).abs().argmax())
        acc[m, n] = acc[m, n] - A[m, k] * W[n, k]
    if fault == "drop_kstep_ragged":
        r0 = (M - 1) // BM * BM
        acc[r0:, cols] = acc[r0:, cols] - A[r0:, K - 128:] @ W[cols, K - 128:].t()
    if fault == "swap_kchunks":
        m = min(M - 1, 5)
        k0 = int(A[m].abs().argmax()) // 16 * 16
        k1 = (k0 + 32) % K
        a = A[m].clone()
        a[k0:k0 + 16], a[k1:k1 + 16] = A[m, k1:k1 + 16], A[m, k0:k0 + 16]
        acc[m] = a @ W.t()
    sa_rows = c["sa"].cpu() if rowscale else c["sa1"].cpu().expand(M)
    if fault == "a_scale_row1":
        sa_rows = sa_rows.clone()
        sa_rows[rows] = (c["sa"].cpu() if rowscale else c["sa1"].cpu().expand(M))[(ridx + 1) % M]
    if fault == "scalar_reads_row":
        assert not rowscale, "fault (n) lives in the scalar mode"
        sa_rows = sa_rows.clone()
        sa_rows[rows] = c["sa"].cpu()[rows]
    sw_pad = torch.cat([c["sw"].cpu(), torch.full((4,), SW_PAD)])
    bias_pad = torch.cat([c["bias"].cpu(), torch.full((4,), BIAS_PAD)])
    sw = sw_pad[:N][None, :].expand(M, N).clone()
    if fault == "w_scale_shift4":
        sw[rows, cols] = sw_pad[cidx + 4][None, :]
    v = acc * (sa_rows[:, None] * sw)
    pad = acc[:, N - 1] * (sa_rows * SW_PAD)                          # what a lane computes for a pad column before the `n < N` test drops it
    if flags & BIAS:
        b = bias_pad[:N][None, :].expand(M, N).clone()
        if fault == "bias_shift4":
            b[rows, cols] = bias_pad[cidx + 4][None, :]
        v = v + b
        pad = pad + BIAS_PAD
    if flags & GELU:
        g = torch.nn.functional.gelu(v)
        if fault == "tanh_gelu":
            g[rows, cols] = torch.nn.functional.gelu(v[rows, cols], approximate="tanh")
        v, pad = g, torch.nn.functional.gelu(pad)
    if flags & QUICK:
        q = _quick32(v)
        if fault == "gelu_for_quick":
            q[rows, cols] = torch.nn.functional.gelu(v[rows, cols])
        v, pad = q, _quick32(pad)
    if flags & RES:
        r = residual_of(flags, c).float().cpu()
        if fault == "residual_row16":
            r = r.clone()
            r[rows, cols] = r[(ridx + 16) % M][:, cols]
        v = v + r
    if flags & F32:
        return dict(out=v)
    if flags & FP8:
        inv = 1.0 / torch.tensor(out_scale, dtype=torch.float32)
        t = (v * inv).clamp(-448, 448)
        if fault == "fp8_multiply_scale":
            t[rows, cols] = (v[rows, cols] * torch.tensor(out_scale, dtype=torch.float32)).clamp(-448, 448)
        codes = t.to(E4M3).view(torch.uint8)
        if fault == "fp8_truncate":
            codes[rows, cols] = _truncate_e4m3(t[rows, cols]).to(E4M3).view(torch.uint8)
        if fault == "fp8_swap_halves":                                # columns past N hold the code of 0 (w_scale and bias read as 0 there)
            wide = torch.zeros(rows.stop, 16, dtype=torch.uint8)
            wide[:, :cols.stop] = codes[rows, cols]
            codes[rows, cols] = torch.cat([wide[:, 8:], wide[:, :8]], dim=1)[:, :cols.stop]
        amax = float(v.abs().max())
        if fault == "amax_pad_column":
            amax = max(amax, float(pad[rows].abs().max()))
        return dict(out=codes.view(E4M3).float(), codes=codes, amax=amax)
    out = v.to(torch.bfloat16).float()
    if fault == "bf16_truncate":
        out[rows, cols] = _truncate_bf16(v[rows, cols])
    return dict(out=out)

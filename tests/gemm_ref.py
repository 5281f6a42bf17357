"""Reference, rounding budgets, inputs and a CPU model with single seeded faults for the tests of the bf16 GEMM family (csrc/gemm_bf16.hip,
csrc/gemm_epilogue.h, csrc/gemm_small.hip and the _ln / _rs / _lnrs entry points): tests/test_gemm_ref_host.py, tests/test_gemm_parity_gpu.py.
A plain helper module: nothing here calls the library.  half_ulp_bf16 and ratio are rowops_ref's.

EXACT-INTEGER INPUTS (int_case).  Small integers make every product and every partial sum exact in fp32, so the order of accumulation cannot
matter and the expected output is known to the bit.
  dense  (fp32 output):  A, W in [-4, 4], K <= 1024: |sum| <= 16 K <= 16384; + bias in [-8, 8] + fp32 residual in [-64, 64]: far below 2^24.
  sparse (bf16 output):  every row of A has at most `nnz` = 8 non-zeros in [-4, 4] \\ {0}, the j-th of row m in k-step (m + j * max(nk // 8, 1)) % nk
         (nk = K / 64) at a seeded random position of that step, so the rows together reach every k-step; W in [-4, 4]:
         |acc| <= 8 * 16 = 128, + |bias| <= 8, + |bf16 residual| <= 64: |value| <= 200 < 256 = 2^8, an integer of at most 8 significant bits:
         every stored bf16 is exact, ReLU keeps that.
  row statistics of the sparse form: a slot's sum of 64 integers of |v| <= 200 is <= 12 800, its sum of squares <= 64 * 200^2 = 2.56e6 < 2^24:
         both exact in fp32 in any order (columns past N count as zero).
  LayerNorm fold (the caller hands in (mean, rstd) and colsum): nnz = 4, so |acc| <= 64; mean in [-2, 2], colsum in [-6, 6] (|mean colsum| <= 12),
         rstd in {0.5, 1, 2}: t = acc - mean colsum is an integer of |t| <= 76 (exact with or without the compiler's fma), rstd t a multiple of
         1/2 with |rstd t| <= 152; + bias: <= 160; + residual (_lnrs): <= 224 < 256.  Where rstd = 0.5 the value is a multiple of 1/2 of
         magnitude <= 38 + 8 + 64 = 110 < 128: 7 integer bits + 1 fraction bit = 8 significant bits.  Exact in bf16 either way.  The partials are
         then sums of multiples of 1/2 (<= 64 * 224 = 14 336 = 28 672 halves) and of 1/4 (<= 64 * 224^2 = 3.2e6 = 1.3e7 quarters < 2^24): exact.
  All operands are seeded random integers, unrelated from row to row and column to column: a transposed, shifted or neighbouring-row read of A,
  W, bias, residual, mean, rstd or colsum does not reproduce the answer.

RANDOM INPUTS WITH A PER-ELEMENT BUDGET (rand_case, reference).  u = 2^-24.  The reference is float64 on the bf16-rounded operands (and on the
fp32 bias / residual / mean / rstd / colsum as the kernel receives them).  bf16 x bf16 products are exact in fp32, so only the K additions round:
    B_acc[m, n] = c K u sum_k |a_mk w_nk|            c = C_ACC = 1: round to nearest, any order of the K additions.
    (what the MI355X needed: MEASURED below)
Every further operation adds u |result| (one rounding) and passes the incoming budget on:
    LN apply   x = rstd (acc - mean colsum):   B = rstd (B_acc + 2 u |mean colsum| + u |acc - mean colsum|)   (product, subtraction, scaling)
    bias       x = x + bias:                   B = B + u |x|
    erf-GELU   y = gelu(x):                    B = 1.13 B + 7e-5        1.13 >= sup |gelu'| = 1.1290 (at x = sqrt 2 ... 1.41); 7e-5 absolute is the
                                                                        contract of the polynomial stated in csrc/common.h (gelu_erf2)
    QuickGELU  y = x sigmoid(1.702 x):         B = 1.10 B + 2 QUICK_REL |y| + 1e-30     1.10 >= sup |d/dx x sigmoid(a x)| = 1.0998 for every a > 0
    residual   x = x + r:                      B = B + u |x|
    ReLU       1-Lipschitz:                    B unchanged
    GLU        y = up silu(gate):              B_s = 1.10 B_gate + 2 SILU_REL |s| + 1e-30,  B = |s| B_up + |up| B_s + B_up B_s + u |y|
QUICK_REL and SILU_REL are the relative errors of quick_gelu / silu (__expf and v_rcp_f32) MEASURED by the activation isolation sweep of
tests/test_gemm_parity_gpu.py against the float64 function; the budget uses twice the measured maximum because the sweep is finite.  The 1e-30
floor covers arguments whose exponential overflows (x = -60: the kernel returns -0, the function -2.7e-43).
bf16 output.  The stored value is RN_bf16(v) with |v - ref| <= B, so |stored - ref| <= B + half_ulp_bf16(v) <= B + half_ulp_bf16(|ref| + B), which
holds without any precondition (half an ulp grows with the magnitude).  Where B < half_ulp_bf16(ref) — the precondition of the shorter form
B + half_ulp_bf16(ref) — a value cannot leave ref's binade without rounding onto the binade's edge, and the shorter form is used.  That
precondition cannot be asserted on every element: B_acc is relative to sum |a w|, not to |ref| — at K = 768 with A ~ N(0, 1), W ~ N(0, 1/K),
sum |a w| = 17.7 and B_acc = 8.1e-4, more than half a bf16 ulp (2^-11 = 4.9e-4 in [0.25, 0.5)) wherever |ref| < 0.5, which is more than a third of
a standard normal output (and the GELU term of 7e-5 exceeds half an ulp for |y| < 0.03).  What CAN be asserted is that the budget is no larger than
this arithmetic says: in the randn family sum |a w| has mean 0.6366 sqrt K and standard deviation 0.77 (K terms |a||w| of mean 0.6366 / sqrt K
and variance (1 - 4 / pi^2) / K), so B <= randn_budget_cap(K) = K u (0.6366 sqrt K + 6.2) + 8 u for the BIAS-only flag set (8 standard deviations: the terms are products
of half-normals, heavy-tailed, and the tests look at 10^6 elements; 8 u covers the add of the bias for |x| <= 8), and the precondition
holds on every element whose own half ulp is above that cap: |ref| >= 2^-5 at K = 64, >= 0.5 at K = 512, >= 1 at K = 768 (cap 1.09e-3) and 1024.  The host test
asserts both, so a budget that quietly grows past half an ulp is noticed.  `reference` returns the fraction of elements on which it holds; the host test prints the
smallest per flag set (BIAS: 0.25 .. 0.62 by family, behind an activation 0.00 .. 0.16).
Row statistics (MQ_EPI_ROW_STATS): against float64 sums of the STORED bf16 values of a slot, budget 64 u sum |v| and 64 u sum v^2.
K <= 1024 in the budgeted cases: a dropped product is about sum |a w| / K, the budget K u sum |a w|: their quotient 1 / (K^2 u) is 28 at K = 768
and 1 at K = 4096.  Long K belongs to the exact-integer test.

MEASURED on the MI355X (gfx950) by tests/test_gemm_parity_gpu.py:
    C_ACC = 1  round to nearest was enough: the first run of the plain fp32-output form (flags OUT_F32) gave a worst ratio of 0.050 on the tiled kernels
               (every plan) and 0.085 on the skinny ones, so c = 2 was never tried.  Worst fp32-output ratio of any flag set: 0.094.
    erf-GELU   worst |error| 6.445e-05 (at x = -4.452, next to the polynomial's clamp), on the skinny and the tiled kernels: inside the 7e-5 contract.
    QUICK_REL  1.163e-07 (at x = -10.80) on the skinny and the tiled kernels;  SILU_REL  0.0 (no argument left half an ulp).
    No fp32-output form of these epilogues exists, so the sweep reads them through the bf16 output with half an ulp allowed: it sees an error only where it
    carries a value across a rounding tie, which makes the figure a lower bound.  An error of relative size e carries about n e / 2^-8 of n arguments
    across (2^-8: the widest relative bf16 gap), so n = 26 112 arguments resolve e >= ACT_RESOLUTION = 2^-8 / 26 112 = 1.5e-7 and nothing below.  The
    activation term is therefore 2 max(measured, ACT_RESOLUTION) = 3.0e-7 relative for both — five orders of magnitude below the 2^-10 at which an
    inaccurate activation would have to be raised as a finding.  The resolution argument is a heuristic, and the figure is NOT a bound on the fp32
    activation: the rounding of the argument 1.702 x alone moves the exponential by |1.702 x| u relative, about 1e-6 at x = -10.  It serves only
    because every consumer of these epilogues is a bf16 output, whose half ulp (2e-3 .. 4e-3 relative) is in the bound next to it; an fp32-output
    form of QuickGELU or the gated product, should one be added, needs a measurement of its own before this module may budget it.

MODEL.  model(): torch fp32 on the CPU — the matmul of the rounded operands, the epilogue in the kernel's order, round-to-nearest-even bf16 — with
switchable single faults (FAULTS), each applied to one element or one 16 x 16 sub-tile only:
    (a) drop_product            one product missing from one element
    (b) drop_kstep_ragged       the last k-step missing on the ragged (last) row tile, one 16-column sub-tile wide
    (c) bias_shift4             bias read 4 columns off
    (d) residual_row16          residual of row m + 16
    (e) bf16_truncate           truncation instead of round-to-nearest
    (f) tanh_gelu               tanh-GELU in place of erf-GELU
    (g) stats_unrounded         row statistics of the unrounded values
    (h) slot_pad_column         the last slot's partial includes a column >= N (the clamped weight row's value)
    (i) ln_neighbour_row        (mean, rstd) of row m + 1
    (j) glu_swap                gate and up swapped within one 16-unit block
    (k) relu_before_residual    ReLU before the residual add instead of after
"""
import math
import os
import re

import torch

from tests.rowops_ref import half_ulp_bf16, ratio  # noqa: F401  (re-exported: the tests take them from here)

U = 2.0 ** -24
# the flags of include/marqo_hip.h
BIAS, GELU, QUICK, RES, F32, ROW_STATS, LN, GLU, RELU = 1, 2, 4, 8, 16, 64, 128, 256, 512

C_ACC = 1            # round-to-nearest accumulate; see MEASURED
GELU_ABS = 7e-5      # csrc/common.h, gelu_erf2
LIP_GELU = 1.13
LIP_SIG = 1.10
QUICK_REL = 1.2e-7   # measured 1.163e-07 (MEASURED)
SILU_REL = 0.0       # measured 0.0: no argument of the sweep left half an ulp (MEASURED)
ACT_RESOLUTION = 2.0 ** -8 / 26112   # 1.5e-7: what the sweep can resolve (MEASURED); the budget takes max(measured, this)
ACT_FLOOR = 1e-30
ACT_REL_LIMIT = 2.0 ** -10   # twice a measured activation error above a quarter of a bf16 half-ulp is a finding, not a budget

FAMILIES = ("randn", "outlier", "offset")
FAULTS = ("drop_product", "drop_kstep_ragged", "bias_shift4", "residual_row16", "bf16_truncate", "tanh_gelu", "stats_unrounded", "slot_pad_column",
          "ln_neighbour_row", "glu_swap", "relu_before_residual")

# ---- the shapes of the GPU test (the host test shows its faults on these) ---------------------------------------------------------------
TILED_MT = (2, 4, 5, 6)
TILED_N = (4, 64, 132, 260)
GLU_N = (32, 96, 288)
BIG_M, BIG_N = (255, 257, 513), (260, 512)
SKINNY_M = (1, 17, 80, 81, 161)
SKINNY_K = (32, 64, 96, 128, 192, 1024)     # K % 32 == 0 there; 96: fewer k-chunks than waves; 1024 with N <= 1024: the 8-wave form


def ring_depth():
    """stages of the LDS ring of gemm_nt_kernel, read from the launch code's LDS size (stages x (BM + BN) rows of BK bf16)"""
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "marqo_amd", "csrc", "gemm_bf16.hip")
    with open(src) as f:
        m = re.search(r"constexpr int LDS = (\d+) \* \(BM \+ BN\) \* BK \* 2;", f.read())
    assert m, "gemm_bf16.hip: the LDS size expression has changed; update ring_depth()"
    return int(m.group(1))


def tiled_k(big=False):
    """K values: prologue only, a pipeline shorter than / equal to / one past the ring, steady state"""
    D = ring_depth()
    ks = sorted({64 * s for s in (1, 2, 3, D, D + 1, 16)})
    return tuple(k for k in ks if k >= 512) if big else tuple(ks)


def tiled_m(mt):
    return (33, 32 * mt - 1, 32 * mt + 1)


def tile_coords(m, n, BM, BN):
    return f"row tile {m // BM} column tile {n // BN} sub-tile ({(m % BM) // 16}, {(n % BN) // 16}) lane row {m % 16} column {n % 16}"


def first_difference(got, ref, BM, BN):
    """text for an exact comparison that failed: the first differing (m, n) and where it sits in the tile plan"""
    bad = (got.double() != ref.double()) | ~torch.isfinite(got.double())
    idx = torch.nonzero(bad)
    if idx.numel() == 0:
        return "equal"
    m, n = int(idx[0, 0]), int(idx[0, 1])
    return f"{int(bad.sum())} of {bad.numel()} differ, first at (m={m}, n={n}): got {float(got[m, n])} want {float(ref[m, n])}; {tile_coords(m, n, BM, BN)}"


def interleave16(up, gate):
    """[F, ...] up and gate rows -> [2F, ...] as MQ_EPI_GLU takes them: rows 32 j .. 32 j + 15 = up units 16 j .. 16 j + 15, the next 16 their gates"""
    F = up.shape[0]
    assert F % 16 == 0 and gate.shape == up.shape
    return torch.stack([up.reshape(F // 16, 16, *up.shape[1:]), gate.reshape(F // 16, 16, *gate.shape[1:])], dim=1).reshape(2 * F, *up.shape[1:]).contiguous()


# ---- inputs -------------------------------------------------------------------------------------------------------------------------------
def _gen(*key):
    """a CPU generator: inputs are made on the CPU and moved, so the host test and the GPU test see the same data"""
    s = 0
    for v in key:
        s = (s * 1000003 + int(v)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


def _to(c, device):
    return {k: v.to(device) for k, v in c.items()}


def family_for(M, N, K):
    """the input family the budget tests of the plain and the gated GEMM use at a shape (the LayerNorm-fold entry points run all three)"""
    return FAMILIES[(M + N // 4 + K // 32) % 3]


def _randint(lo, hi, shape, g, device):
    return torch.randint(lo, hi + 1, shape, generator=g, device=device)


def int_case(form, M, N, K, seed=0, device="cpu", nnz=8):
    """exact-integer operands (module docstring): dict A, W (bf16), bias, res (fp32; the bf16 residual is res.bfloat16(), exact), mean, rstd, colsum (fp32)"""
    target, device = device, "cpu"
    g = _gen(11, M, N, K, seed, nnz)
    W = _randint(-4, 4, (N, K), g, device)
    if form == "dense":
        assert K <= 1024
        A = _randint(-4, 4, (M, K), g, device)
    else:
        assert form == "sparse" and K % 32 == 0
        sw = 64 if K % 64 == 0 else 32                 # (the skinny kernels also take K % 64 == 32: steps of 32 there)
        nk = K // sw
        A = torch.zeros(M, K, dtype=torch.int64, device=device)
        rows = torch.arange(M, device=device)
        for j in range(nnz):
            step = (rows + j * max(nk // 8, 1)) % nk
            pos = _randint(0, sw - 1, (M,), g, device)
            val = _randint(1, 4, (M,), g, device) * (2 * _randint(0, 1, (M,), g, device) - 1)
            A[rows, step * sw + pos] = val
    rstd = torch.tensor([0.5, 1.0, 2.0], device=device)[_randint(0, 2, (M,), g, device)]
    return _to(dict(A=A.to(torch.bfloat16), W=W.to(torch.bfloat16), bias=_randint(-8, 8, (N,), g, device).float(), res=_randint(-64, 64, (M, N), g, device).float(),
                    mean=_randint(-2, 2, (M,), g, device).float(), rstd=rstd, colsum=_randint(-6, 6, (N,), g, device).float()), target)


def rand_case(family, M, N, K, seed=0, device="cpu"):
    """random operands: A ~ N(0, 1) (`outlier`: one column + 40; `offset`: row mean = 3 sigma), W ~ N(0, 1 / K), both rounded to bf16; (mean, rstd) are the
    statistics of the rounded rows (eps 1e-5) and colsum the row sums of the rounded weight, each rounded to the fp32 the kernel receives"""
    target, device = device, "cpu"
    g = _gen(13, M, N, K, seed, FAMILIES.index(family))
    a = torch.randn(M, K, generator=g, device=device)
    if family == "outlier":
        a[:, (3 * K) // 7] += 40.0
    elif family == "offset":
        a = a + 3.0
    A = a.to(torch.bfloat16)
    W = (torch.randn(N, K, generator=g, device=device) / K ** 0.5).to(torch.bfloat16)
    bias = 0.5 * torch.randn(N, generator=g, device=device)
    res = 2.0 * torch.randn(M, N, generator=g, device=device) + 0.5
    Ad = A.double()
    mean = Ad.mean(1)
    rstd = 1.0 / torch.sqrt(((Ad - mean[:, None]) ** 2).mean(1) + 1e-5)
    return _to(dict(A=A, W=W, bias=bias, res=res, mean=mean.float(), rstd=rstd.float(), colsum=W.double().sum(1).float()), target)


def randn_budget_cap(K):
    """upper bound of B for the BIAS-only flag set in the randn family (module docstring): K u (0.6366 sqrt K + 6.2) + 8 u"""
    return K * U * (0.6366 * math.sqrt(K) + 6.2) + 8 * U


def residual_of(flags, c):
    """the residual operand a flag set reads: fp32 next to an fp32 output, else the bf16 stream"""
    return c["res"] if flags & F32 else c["res"].to(torch.bfloat16)


# ---- reference and budgets ----------------------------------------------------------------------------------------------------------------
def _sums64(c):
    if "_acc64" not in c:
        Ad, Wd = c["A"].double(), c["W"].double()
        c["_acc64"], c["_S"] = Ad @ Wd.t(), Ad.abs() @ Wd.abs().t()
    return c["_acc64"], c["_S"]


def _gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def _act_rel(v, name):
    assert v is not None, f"{name} has not been measured yet (activation isolation sweep)"
    assert 2.0 * v <= ACT_REL_LIMIT, f"twice the measured {name} = {2 * v:.3e} exceeds 2^-10: a finding, not a budget"
    return 2.0 * max(v, ACT_RESOLUTION)


def reference(flags, c, c_acc=None):
    """float64 reference and budget of one flag set on a case: dict ref, B (before the output rounding), bound (B, or B + half a bf16 ulp), B_acc, pre
    (fraction of elements with B below half a bf16 ulp of ref; 1.0 for fp32 output)"""
    acc, S = _sums64(c)
    K = c["A"].shape[1]
    B_acc = (C_ACC if c_acc is None else c_acc) * K * U * S
    x, B = acc, B_acc
    if flags & LN:
        mean, rstd, cs = c["mean"].double()[:, None], c["rstd"].double()[:, None], c["colsum"].double()[None, :]
        mc = mean * cs
        t = acc - mc
        x, B = rstd * t, rstd * (B + 2 * U * mc.abs() + U * t.abs())
    if flags & BIAS:
        x = x + c["bias"].double()[None, :]
        B = B + U * x.abs()
    if flags & GELU:
        x, B = _gelu64(x), LIP_GELU * B + GELU_ABS
    if flags & QUICK:
        x = x * torch.sigmoid(1.702 * x)
        B = LIP_SIG * B + _act_rel(QUICK_REL, "QUICK_REL") * x.abs() + ACT_FLOOR
    if flags & RES:
        x = x + residual_of(flags, c).double()
        B = B + U * x.abs()
    if flags & RELU:
        x = x.clamp(min=0)
    if flags & GLU:
        M, N = x.shape
        x4, B4 = x.view(M, N // 32, 2, 16), B.view(M, N // 32, 2, 16)
        up, gate, Bu, Bg = x4[:, :, 0].reshape(M, N // 2), x4[:, :, 1].reshape(M, N // 2), B4[:, :, 0].reshape(M, N // 2), B4[:, :, 1].reshape(M, N // 2)
        s = gate * torch.sigmoid(gate)
        Bs = LIP_SIG * Bg + _act_rel(SILU_REL, "SILU_REL") * s.abs() + ACT_FLOOR
        x = up * s
        B = s.abs() * Bu + up.abs() * Bs + Bu * Bs + U * x.abs()
    if flags & F32:
        return dict(ref=x, B=B, bound=B, B_acc=B_acc, pre=1.0)
    hu = half_ulp_bf16(x)
    pre = B < hu
    bound = B + torch.where(pre, hu, half_ulp_bf16(x.abs() + B))
    return dict(ref=x, B=B, bound=bound, B_acc=B_acc, pre=float(pre.double().mean()))


def slot_reference(stored, width):
    """float64 (sum, sum of squares) of the stored values per `width`-column slot, slot-major [nslots, M], and their budgets; columns past the end count as zero"""
    M, N = stored.shape
    ns = (N + width - 1) // width
    pad = torch.zeros(M, ns * width, dtype=torch.float64, device=stored.device)
    pad[:, :N] = stored.double()
    pad = pad.view(M, ns, width)
    s1, s2, a1 = pad.sum(-1).t(), (pad * pad).sum(-1).t(), pad.abs().sum(-1).t()
    return s1, s2, 64 * U * a1, 64 * U * s2


def worst(got, r):
    """text: the worst element of a budgeted comparison, its coordinates and budget terms"""
    err = (got.double() - r["ref"]).abs() / r["bound"]
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    i = int(err.argmax())
    m, n = divmod(i, err.shape[1])
    b_acc = f"B_acc {float(r['B_acc'][m, n]):.3e} " if r["B_acc"].shape == err.shape else ""      # (GLU: two accumulators per output)
    return f"worst (m={m}, n={n}): got {float(got[m, n])!r} ref {float(r['ref'][m, n])!r} {b_acc}B {float(r['B'][m, n]):.3e} bound {float(r['bound'][m, n]):.3e}"


# ---- the CPU model with single faults ------------------------------------------------------------------------------------------------------
def _truncate_bf16(v):
    return (v.contiguous().view(torch.int32) & -65536).view(torch.float32)


def model(flags, c, fault=None, BM=64):
    """torch fp32 model of one launch on the CPU: (out float32 [M, N] (GLU: [M, N / 2]) holding the stored values, partials [nslots, M, 2] or None).
    BM = rows of the plan's row tile (it only places fault (b))."""
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
        acc[r0:, cols] = acc[r0:, cols] - A[r0:, K - 64:] @ W[cols, K - 64:].t()
    v = acc
    if flags & LN:
        mean, rstd = c["mean"].cpu(), c["rstd"].cpu()
        if fault == "ln_neighbour_row":
            src = torch.arange(M)
            src[rows] = (ridx + 1) % M
            mean, rstd = mean[src], rstd[src]
        v = rstd[:, None] * (v - mean[:, None] * c["colsum"].cpu()[None, :])
    if flags & BIAS:
        b = c["bias"].cpu()[None, :].expand(M, N).clone()
        if fault == "bias_shift4":
            b[rows, cols] = c["bias"].cpu()[(cidx + 4) % N][None, :]
        v = v + b
    if flags & GELU:
        g = torch.nn.functional.gelu(v)
        if fault == "tanh_gelu":
            g[rows, cols] = torch.nn.functional.gelu(v[rows, cols], approximate="tanh")
        v = g
    if flags & QUICK:
        v = v * torch.sigmoid(1.702 * v)
    if flags & RES:
        r = residual_of(flags, c).float().cpu()
        if fault == "residual_row16":
            r = r.clone()
            r[rows, cols] = r[(ridx + 16) % M][:, cols]
        w = v + r
        if flags & RELU:
            w = w.clamp(min=0)
            if fault == "relu_before_residual":
                w[rows, cols] = v[rows, cols].clamp(min=0) + r[rows, cols]
        v = w
    elif flags & RELU:
        v = v.clamp(min=0)
    if flags & GLU:
        v4 = v.view(M, N // 32, 2, 16)
        up, gate = v4[:, :, 0].clone(), v4[:, :, 1].clone()
        if fault == "glu_swap":
            up[rows, 0], gate[rows, 0] = v4[rows, 0, 1], v4[rows, 0, 0]
        v = (up * (gate * torch.sigmoid(gate))).reshape(M, N // 2)
    if flags & F32:
        return v, None
    out = v.to(torch.bfloat16).float()
    if fault == "bf16_truncate":
        out[rows, cols] = _truncate_bf16(v[rows, cols])
    if not flags & ROW_STATS:
        return out, None
    width = 32 if flags & GLU else 64
    src = out.clone()
    if fault == "stats_unrounded":
        src[rows, :width] = v[rows, :width]
    Nv = src.shape[1]
    ns = (Nv + width - 1) // width
    pad = torch.zeros(M, ns * width)
    pad[:, :Nv] = src
    if fault == "slot_pad_column":
        assert Nv % width, "fault (h) needs a ragged last slot"
        pad[rows, Nv] = src[rows, Nv - 1]
    pad = pad.view(M, ns, width)
    return out, torch.stack([pad.sum(-1).t(), (pad * pad).sum(-1).t()], dim=-1).contiguous()

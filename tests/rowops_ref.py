"""Reference, rounding budgets, arithmetic model and input families for the tests of csrc/rowops.hip (tests/test_rowops_ref_host.py,
tests/test_rowops_gpu.py, tests/test_kernels_gpu.py).  A plain helper module: nothing here calls the library.

REFERENCE.  float64 LayerNorm / (mean, rstd) / L2 normalisation of the exact input values (torch, on whatever device the input is on; fp32 and
bf16 values are exact in float64).

BUDGET of the two-pass LayerNorm kernels (layernorm_kernel, layernorm_bf16in_kernel, row_stats_bf16_kernel, ln_normalize_row).  u = 2**-24,
D = ceil(W / 64) + 8 is the longest chain of additions a sum goes through (a lane's own elements, six butterfly levels, the divide).  With the exact
per-row mean mu, deviations d = x - mu, sigma' = sqrt(var + eps) and A = mean|x|:
    c     = D u A                                  bounds the error of the mean
    rho   = (D / 2 + 4) u + c^2 / (2 sigma'^2)     bounds the relative error of rstd (a mean error shifts every deviation alike, so it enters the
                                                   variance only as c^2; D u on the sum of squares halves under the square root; 4 u: the squaring,
                                                   the divide, the add of eps and rsqrtf)
    B_j   = |g_j| / sigma' (c + 2 u |d_j|) + |g_j d_j| / sigma' rho + 2 u |y_j|
fp32 output: B.  bf16 output: B + half a bf16 ulp of the reference value (valid while B is below that half ulp, which is what makes a value cross
into the next binade impossible without B noticing).  mq_row_stats: mean within c, rstd within rho (relative).

BUDGET of the one-pass finalise (row_stats_finalize_kernel + mq_finalize_stats).  Its inputs are the n = nslots fp32 partial sums (p1_k, p2_k) of a
row; the reference is float64 on those same partials, mu = S1 / W, var = max(S2 / W - mu^2, 0) (the clamp is the kernel's contract: exact partials
of real rows never give less, rounded ones do).  The kernel adds n terms one after the other (<= (n - 1) u relative to sum|p|), multiplies by
fl(1 / W) (2 u), and forms var with one fma (u):
    c_f      = (n + 2) u sum|p1_k| / W                                         error of the mean
    delta_t  = (n + 2) u S2 / W  +  2 |mu| c_f + c_f^2  +  u |var|             error of var: the first term is the cancellation, (n + 2) u E[x^2]
    t = var + eps = sigma'^2,  rstd = t^-1/2:   rho_f = delta_t / (2 sigma'^2) + 3 u   to first order  — it carries E[x^2] / sigma'^2.
The first-order form is useless where delta_t > sigma'^2 (a constant row: var = 0, the computed one-pass variance comes out slightly negative and is
clamped), so the assertion is made on t_hat = rstd_hat^-2, where the bound is linear and holds without linearisation (max(., 0) is 1-Lipschitz):
    |t_hat - t| <= delta_t + 6 u (t + delta_t)              (6 u: add of eps, rsqrtf at 2 u counted twice through the square, slack of one)

BUDGET of l2norm_kernel.  The sum of squares has only positive terms: relative error (ceil(D / 64) + 7) u =: Dl u (a lane's chain, one squaring, six
levels); the square root halves it; sqrtf, the reciprocal and the final product add one u each and one is kept spare:
    |out_j - y_j| <= (Dl / 2 + 4) u |y_j|

MODEL.  model_layernorm / model_finalize: float32 numpy models of the kernels' arithmetic (per-lane chains in chunk order, the xor butterfly,
two-pass variance, divide by W), `form` = "generic" (4 elements per lane and chunk) or "wide" (8), with switchable single faults (FAULTS).
"""
import math

import numpy as np
import torch

U = 2.0 ** -24
FAMILIES = ("randn", "offset", "outlier", "const", "rowscale")
FAULTS = ("one_pass", "no_eps", "padded_width", "prev_row_mean", "gamma_other_half", "bf16_truncate", "skip_ragged_chunk")   # (a) .. (g); (h): model_finalize(first8=True)
HOST_WIDTHS = (4, 8, 12, 252, 256, 260, 512, 520, 768, 1024, 1028, 1280, 1540, 1664, 2048)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
def make_rows(family, rows, W, seed=0, device="cpu", bf16=False):
    """(x [rows, W] fp32 or bf16, gamma [W], beta [W]); gamma and beta are random and distinct per column in every family"""
    g = torch.Generator(device=device).manual_seed(1000 * seed + 7 * W + rows)
    n = torch.randn(rows, W, device=device, generator=g)
    if family == "randn":
        x = n * 3 + 1.5
    elif family == "offset":            # mean = 50 sigma
        x = n * 0.5 + 25.0
    elif family == "outlier":           # one column + 60
        x = n.clone()
        x[:, (3 * W) // 7] += 60.0
    elif family == "const":             # var = 0; the one-pass variance comes out slightly negative
        x = torch.full_like(n, 3.3)
    elif family == "rowscale":          # per-row sigma 1e-2 .. 1e2, per-row mean -5 .. 5, neighbours unrelated: a row that takes another row's statistics shows
        t = torch.linspace(0, 1, rows, device=device) if rows > 1 else torch.full((1,), 0.5, device=device)
        sig = 10.0 ** (4 * t[torch.randperm(rows, device=device, generator=g)] - 2)
        mu = 10 * t[torch.randperm(rows, device=device, generator=g)] - 5
        x = n * sig[:, None] + mu[:, None]
    else:
        raise ValueError(family)
    gam = torch.randn(W, device=device, generator=g)
    bet = torch.randn(W, device=device, generator=g)
    return (x.to(torch.bfloat16) if bf16 else x.contiguous()), gam, bet


# ---- reference and budgets ---------------------------------------------------------------------------------------------------------------
def row_moments(x, eps):
    """exact per-row (mu, d, sigma', A) in float64"""
    x = x.double()
    mu = x.mean(-1, keepdim=True)
    d = x - mu
    sp = ((d * d).mean(-1, keepdim=True) + eps).sqrt()
    return mu, d, sp, x.abs().mean(-1, keepdim=True)


def chain(W):
    return math.ceil(W / 64) + 8


def stats_budget(x, eps):
    """(mu, rstd, c, rho): exact mean and rstd [rows] and their bounds (c absolute, rho relative)"""
    mu, _, sp, A = row_moments(x, eps)
    D = chain(x.shape[-1])
    c = D * U * A
    rho = (D / 2 + 4) * U + c * c / (2 * sp * sp)
    return mu[:, 0], 1.0 / sp[:, 0], c[:, 0], rho[:, 0]


def reference_ln(x, gam, bet, eps):
    """(y, B): float64 LayerNorm [rows, W] and the elementwise budget of an fp32 output"""
    mu, d, sp, A = row_moments(x, eps)
    g, b = gam.double(), bet.double()
    y = d / sp * g + b
    D = chain(x.shape[-1])
    c = D * U * A
    rho = (D / 2 + 4) * U + c * c / (2 * sp * sp)
    B = g.abs() / sp * (c + 2 * U * d.abs()) + (g * d).abs() / sp * rho + 2 * U * y.abs()
    return y, B


def half_ulp_bf16(y):
    """half a bf16 ulp (8 significant bits) of |y|, float64; 0 at 0"""
    _, ex = torch.frexp(y.double().abs())           # |y| = m 2^ex, m in [0.5, 1): ulp = 2^(ex - 8)
    h = torch.ldexp(torch.ones_like(y, dtype=torch.float64), ex.clamp(min=-125) - 9)
    return torch.where(y == 0, torch.zeros_like(h), h)


def ratio(got, ref, bound):
    """worst |got - ref| / bound (float64); an element with bound 0 must be exact (ratio inf otherwise), non-finite `got` gives inf"""
    err = (got.double() - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    r = torch.where(torch.isfinite(got.double()), r, torch.full_like(r, float("inf")))
    return float(r.max()) if r.numel() else 0.0


def finalize_reference(partials, W, eps):
    """partials fp32 [nslots, rows, 2] (slot-major, as the residual GEMM writes them) -> (mu, t = max(var, 0) + eps, c_f, bound on |t_hat - t|), float64 [rows]"""
    p = partials.double()
    n = p.shape[0]
    S1, S2 = p[..., 0].sum(0), p[..., 1].sum(0)
    mu = S1 / W
    var = (S2 / W - mu * mu).clamp(min=0)
    cf = (n + 2) * U * p[..., 0].abs().sum(0) / W
    dt = (n + 2) * U * p[..., 1].abs().sum(0) / W + 2 * mu.abs() * cf + cf * cf + U * var
    t = var + eps
    return mu, t, cf, dt + 6 * U * (t + dt)


def make_partials(x, nslots):
    """the (sum, sum of squares) of `nslots` column bands of every row, computed in float64 and rounded to fp32: [nslots, rows, 2].  The bands are
    uneven on purpose (the first takes what the others leave)."""
    rows, W = x.shape
    xd = x.double()
    edges = [0] + [W - (nslots - 1 - k) * (W // nslots) for k in range(nslots)]
    out = torch.empty(nslots, rows, 2, dtype=torch.float64, device=x.device)
    for k in range(nslots):
        band = xd[:, edges[k]:edges[k + 1]]
        out[k, :, 0] = band.sum(-1)
        out[k, :, 1] = (band * band).sum(-1)
    return out.float()


def reference_l2(x):
    """(y, bound): x / ||x|| in float64 (an all-zero row gives 0 / 0 = NaN, as torch's `x / x.norm(dim=-1, keepdim=True)` does)"""
    xd = x.double()
    y = xd / xd.norm(dim=-1, keepdim=True)
    Dl = math.ceil(x.shape[-1] / 64) + 7
    return y, (Dl / 2 + 4) * U * y.abs()


# e4m3 (fn) codes ----------------------------------------------------------------------------------------------------------------------------
def e4m3_tie_distance(r):
    """distance (float64) of r from the nearest e4m3 rounding tie (the midpoint of two neighbouring e4m3 values); values beyond 448 count as far (they saturate)"""
    a = r.double().abs()
    _, ex = torch.frexp(a.clamp(min=2.0 ** -20))
    sp = torch.ldexp(torch.ones_like(a), (ex - 1).clamp(min=-6) - 3)      # spacing of the binade of |r|; 2^-9 in the subnormal range
    q = a / sp
    dist = ((q - q.floor()) - 0.5).abs() * sp
    return torch.where(a >= 448, torch.full_like(dist, float("inf")), dist)


def e4m3_signed(codes):
    """e4m3 byte codes -> signed step index (+-0 both 0): neighbouring values differ by 1"""
    c = codes.to(torch.int32)
    return torch.where((c & 0x80) != 0, -(c & 0x7F), c & 0x7F)


def e4m3_codes(r):
    """round-to-nearest-even e4m3 codes (uint8) of float64 values, saturating at +-448 (torch's conversion, on the CPU)"""
    return r.float().clamp(-448, 448).cpu().to(torch.float8_e4m3fn).view(torch.uint8)


# ---- float32 model of the kernels ----------------------------------------------------------------------------------------------------------
def _f32(a):
    return np.asarray(a, dtype=np.float32)


def round_bf16(y, truncate=False):
    u = _f32(y).view(np.uint32).astype(np.uint64)
    if not truncate:
        u = u + 0x7FFF + ((u >> 16) & 1)
    return (u & 0xFFFF0000).astype(np.uint32).view(np.float32)


def _butterfly(a):
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        a = a + a[:, lanes ^ o]
    return a[:, 0]


def dispatch_chunks(W, form):
    """chunks per lane of the instantiation that runs width W (MQ_DISPATCH_CH: 5 runs as 6, 7 as 8; the 16-byte form has 1 or 2)"""
    k = 4 if form == "generic" else 8
    ch = (W // k + 63) // 64
    return k, ch, ({5: 6, 7: 8}.get(ch, ch) if form == "generic" else ch)


def model_layernorm(x, gam, bet, eps, form="generic", fault=None, out_bf16=False, fma=False):
    """float32 model: returns (y [rows, W] float32 — rounded to bf16 values when out_bf16 —, mean [rows], rstd [rows]).  fma: the sum of squared
    deviations and the affine are contracted as hipcc contracts them (emulated through float64: a float32 product is exact there)."""
    assert fault is None or fault in FAULTS
    x, gam, bet = _f32(x), _f32(gam), _f32(bet)
    rows, W = x.shape
    k, ch, ch_inst = dispatch_chunks(W, form)
    assert W % k == 0
    nch = W // k
    pad = np.zeros((rows, ch * 64 * k), np.float32)
    pad[:, :W] = x
    v = pad.reshape(rows, ch, 64, k)                                    # chunk c = lane + 64 i holds elements c k .. c k + k - 1
    valid = (np.arange(ch)[:, None] * 64 + np.arange(64)[None, :]) < nch  # [ch, 64]
    if fault == "skip_ragged_chunk" and nch % 64:
        valid = valid.copy()
        valid[ch - 1] = False
    wdiv = np.float32(64 * k * ch_inst if fault == "padded_width" else W)
    eps = np.float32(eps)

    s1 = np.zeros((rows, 64), np.float32)
    for i in range(ch):
        c = v[:, i]
        grp = (c[..., 0] + c[..., 1]) + (c[..., 2] + c[..., 3])
        if k == 8:
            grp = grp + ((c[..., 4] + c[..., 5]) + (c[..., 6] + c[..., 7]))
        s1 = np.where(valid[i], s1 + grp, s1)
    mean = _butterfly(s1) / wdiv
    if fault == "prev_row_mean":                                        # the second row of a two-row wave takes the first row's mean
        mean = mean.copy()
        mean[1::2] = mean[0::2][:rows // 2]
    m = mean[:, None]

    def acc(s, a):                                                     # s + a * a
        return (s.astype(np.float64) + a.astype(np.float64) * a.astype(np.float64)).astype(np.float32) if fma else s + a * a

    s2 = np.zeros((rows, 64), np.float32)
    for i in range(ch):
        for e in range(k):
            t = v[:, i, :, e] if fault == "one_pass" else v[:, i, :, e] - m
            s2 = np.where(valid[i], acc(s2, t), s2)
    var = _butterfly(s2) / wdiv
    if fault == "one_pass":
        var = var - mean * mean
    with np.errstate(all="ignore"):
        rstd = np.float32(1) / np.sqrt(var if fault == "no_eps" else var + eps)
        cols = np.arange(W) ^ 4 if (fault == "gamma_other_half" and W % 8 == 0) else np.arange(W)
        gg, bb = gam[cols][None, :], bet[cols][None, :]
        t = (x - m) * rstd[:, None]
        y = (t.astype(np.float64) * gg.astype(np.float64) + bb.astype(np.float64)).astype(np.float32) if fma else t * gg + bb
    if out_bf16:
        y = round_bf16(y, truncate=fault == "bf16_truncate")
    return y, mean, rstd


def model_finalize(partials, W, eps, first8=False):
    """float32 model of row_stats_finalize_kernel: slot-order sums, mean = s1 fl(1 / W), var = fma(-mean, mean, s2 fl(1 / W)), rsqrt(max(var, 0) + eps).
    first8 = fault (h): only the first 8 slots are summed."""
    p = _f32(partials)
    n = min(p.shape[0], 8) if first8 else p.shape[0]
    s1 = np.zeros(p.shape[1], np.float32)
    s2 = np.zeros(p.shape[1], np.float32)
    for k in range(n):
        s1 = s1 + p[k, :, 0]
        s2 = s2 + p[k, :, 1]
    inv_w = np.float32(1) / np.float32(W)
    mean = s1 * inv_w
    var = ((s2 * inv_w).astype(np.float64) - mean.astype(np.float64) * mean.astype(np.float64)).astype(np.float32)
    rstd = np.float32(1) / np.sqrt(np.maximum(var, np.float32(0)) + np.float32(eps))
    return mean, rstd


def model_l2(x):
    """float32 model of l2norm_kernel: lane c sums columns c, c + 64, ..; butterfly; 1 / sqrt; product"""
    x = _f32(x)
    rows, D = x.shape
    pad = np.zeros((rows, -(-D // 64) * 64), np.float32)
    pad[:, :D] = x
    s = np.zeros((rows, 64), np.float32)
    for i in range(pad.shape[1] // 64):
        c = pad[:, i * 64:(i + 1) * 64]
        s = s + c * c
    with np.errstate(all="ignore"):
        inv = np.float32(1) / np.sqrt(_butterfly(s))
        return x * inv[:, None]

"""Reference, rounding budgets, arithmetic models and input families for the tests of the convolutional towers' kernels, csrc/convnext.hip and
csrc/resnet.hip (tests/test_conv_ref_host.py, tests/test_conv_kernels_gpu.py).  A plain helper module: nothing here calls the library.

REFERENCE.  float64 restatements on the exact input values (bf16, fp32 and uint8 values are exact in float64), written as plain indexing over
padded arrays; tests/test_conv_ref_host.py cross-checks them against torch.nn.functional in float64 on the CPU.

BUDGETS, per element, u = 2**-24.  hb(r, B) is half a bf16 ulp of |r| + B: the value the kernel rounds is within B of r, so that is the largest
half ulp its store can add, with no condition on B (rowops_ref adds the half ulp of r itself, valid while B stays below it).

  conv3x3    S = sum |x w| over the 9 Cin products, pre = the sum + bias before the ReLU.  bf16 x bf16 products are exact in fp32.  How the MFMA
             orders and rounds its internal additions is not visible in the source: each of the 9 Cin additions is bounded by 2 u relative to S
             (truncation included), the bias add by u |pre|; the ReLU is 1-Lipschitz:      B = 18 Cin u S + u |pre|,   + hb(ref, B)
  dwconv7    a chain of 49 fmas that starts at the bias, one rounding each:                 B = 49 u (S + |bias|),      + hb(ref, B)
  partials   reference = float64 sum and sum of squares of the 64 bf16 values the kernel STORED (y is read back).  A lane adds 8 values (four
             pair sums into a chain: at most 8 roundings on a value's way; the squares: 8 fmas), then three shuffle levels:
                                                                                           B1 = 11 u sum |v|,  B2 = 11 u sum v^2
  avgpool2   (a + b) + (c + d): every value passes two additions; the quarter is exact:    B = 2 u (|a| + |b| + |c| + |d|) / 4,  + hb
  ds gather  t = (x - mean) rstd g takes three roundings, the add of beta one (or one fma): B = 3 u |t| + u |y|,  + hb
             (mean, rstd) are INPUTS here: the reference uses the same fp32 values, so the gather is checked without mq_row_stats.
  stem u8    v = b / 255 (u), v - mean (u), / std (u); an error of the numerator is divided by |std|:
                                                                                           B = u (|v| + |v - mean|) / |std| + 2 u |y|,  + hb
  stem f32   the value is only rounded:                                                    B = 0,  + hb (= half a bf16 ulp of the input)
  ap_tokens  row 0: an HW-term chain (HW u relative to sum |x|), fl(1 / HW) and the product (2 u), the add of pos (u |y|):
                                                                                           B = (HW + 2) u sum |x| / HW + u |y|,  + hb
             rows 1..: one add:                                                            B = u |y|,  + hb
  pool_ln    the pooled means m_c carry e_c = (HW + 2) u mean_p |x_pc|.  The two-pass LayerNorm over them has rowops_ref's budget form with the chain
             D = ceil(C / 256) + 10 of this kernel (256 threads: a thread's own elements, six butterfly levels, two adds of the four wave sums,
             the divide, one spare) evaluated on the exact means; an input error e moves the output by at most
                 |g_c| / s' (|e_c| + mean |e|) + |g_c d_c| / s'^2 rms(e)        (to first order; both terms carry (1 + 4 max |e| / s') for the rest)
  ap_attend  scores: a 64-term fma chain, ds_t = 64 u sum_d |q_d k_td| absolute.  x_t = s_t - max s <= 0 is one subtraction (u |x_t|); __expf(x)
             is v_exp_f32(x log2(e)): the rounded constant and the product move the argument by 2 u |x| log2(e), i.e. the result by 2 u |x|
             relative, and the instruction itself is good to one ulp (2 u) — the figure attention_ref's budget counts under "everything else
             is fp32".  The max itself cancels between the numerator and the denominator.  So probability t is off by
                 eta_t = 2 ds_t + (3 |x_t| + 4) u        relative  (2 ds: the score's own error and that of the max it is measured from),
             the T-term fma chain of the weighted sum by T u P|V|, the lane chains and six levels of the normaliser by (ceil(T / 64) + 6) u, the
             divide by u:      B = sum_t P_t eta_t (|v_t| + |out|) + (T + 1) u P|V| + (ceil(T / 64) + 8) u |out|,  + hb

FAMILIES (FAMILIES_MAP for the spatial kernels, FAMILIES_ATTEND for ap_attend; `offset` and `rowscale` of rowops_ref.make_rows for pool_ln and the ds
gather).  Values are drawn so that neighbours differ: any wrong index changes the value.
  randn       N(0, 1)
  loud_image  odd-numbered images carry + 50: a halo or a row read across an image boundary shows up in the neighbours
  ramp        ((37 img + 11 y + 5 x + 3 c) mod 127) - 63, exact in bf16; conv3x3 pairs it with integer weights -2 .. 2 and the depthwise taps with
              multiples of 1 / 8, so the kernel's fp32 sums are exact too and a transposed or shifted read is off by whole units
  edge        non-zero only in the outermost ring of pixels: the padding masks
  peaked      (ap_attend) one key per head and image scores about 30 above the rest, at position (7 img + 13 head) mod T
  offset      (ap_attend) scores 80 +- 10 (q = 1.25, k = 1 + N(0, 1)): the largest pass 88.7, where exp leaves fp32, so a missing max-subtraction
              overflows; the exact softmax is unaffected
  one_loud_value  (ap_attend) V of one token per image is x 1000: one wrong key is visible, as in the attention tests

The conv3x3 weights carry the value 3 in the K padding (columns 9 Cin .. Kp - 1).  The kernel feeds zeros for those k whatever the weight holds; with
zeros in the weight too (as the loader leaves them) a padding tap that read real pixels would be multiplied away and stay invisible.

MODELS.  float32 numpy models of each kernel's indexing and order of operations (fp32 fmas emulated through float64, where a product of a bf16 and an
fp32 value is exact), each with ONE switchable fault (FAULTS).  Faulty indices that leave the array are clamped to it: the models must not fault.
"""
import math

import numpy as np
import torch

from tests import rowops_ref as R

U = R.U
FAMILIES_MAP = ("randn", "loud_image", "ramp", "edge")
FAMILIES_ROWS = ("randn", "loud_image", "ramp", "offset", "rowscale")
FAMILIES_ATTEND = ("randn", "loud_image", "ramp", "peaked", "offset", "one_loud_value")
FAULTS = {
    "conv3x3": ("hw_swap", "halo_neighbour", "drop_right", "tap_transposed", "walk_once", "kpad_tap0"),
    "dwconv7": ("hw_swap", "halo_neighbour", "partials_pixel_major", "partials_unrounded"),
    "avgpool2": ("hw_swap", "second_row_at_h"),
    "ds_gather": ("hw_swap", "quadrant_kx_ky"),
    "stem_gather": ("hw_swap", "mean0", "origin_2oy"),
    "ap_attend": ("no_max", "head_stride_c", "skip_tail"),
}

# ---- the shapes of the GPU test (the host test runs the models on the same) ----------------------------------------------------------------------
CONV_HW = ((1, 1), (1, 9), (5, 3), (7, 7), (6, 11))
CONV_N = (1, 3, 9)
CONV_CIN = (8, 16, 24, 40, 64, 72, 136)
CONV_COUT = (4, 36, 128, 132, 260)
CONV_STORE = ("ldy=cout", "ldy=cout+4", "misaligned")
# 35 shapes, each run at both tile heights (70 cases): 5 and 7 are coprime, so every (H, W) meets every Cin; i = 2, 17, 32 are n = 9 at (5, 3),
# M = 135: one 64-row tile spans five images
CONV_CASES = tuple(dict(H=CONV_HW[i % 5][0], W=CONV_HW[i % 5][1], n=CONV_N[i % 3], Cin=CONV_CIN[i % 7], Cout=CONV_COUT[(i + i // 5) % 5],
                        relu=i % 2, store=CONV_STORE[(i + i // 3) % 3]) for i in range(35))
DW_HW = ((1, 1), (3, 5), (8, 16), (9, 17), (7, 33), (20, 6))
DW_C = (64, 128, 192)
DW_N = (1, 3)
POOL2_HW = ((2, 2), (2, 6), (6, 4))
POOL2_C = (8, 72, 264)
POOL2_N = 3
POOL_LN_C = (8, 264, 2048, 3072)
POOL_LN_HW = (1, 7, 49)
STEM_S = (2, 4, 6, 34)
STEM_N = 3
STEM_NORMS = (((0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)), ((0.5, 0.25, 0.75), (0.5, 0.25, 0.125)),
              ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225)))
TOK_HW = (1, 3, 255)
TOK_C = (8, 264, 2056)
ATT_T = (1, 63, 64, 65, 256)
ATT_C = (64, 192)
ATT_N = 3


def _seed(*key):
    s = 17
    for k in key:
        s = (s * 1000003 + int(k)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------------
def make_map(family, n, H, W, C, seed=0):
    """bf16 [n, H, W, C] on the CPU"""
    assert family in FAMILIES_MAP
    g = _seed(seed, n, H, W, C, FAMILIES_MAP.index(family))
    x = torch.randn(n, H, W, C, generator=g)
    if family == "loud_image":
        x[1::2] += 50.0
    elif family == "ramp":
        i, y, xx, c = torch.meshgrid(torch.arange(n), torch.arange(H), torch.arange(W), torch.arange(C), indexing="ij")
        x = ((37 * i + 11 * y + 5 * xx + 3 * c) % 127 - 63).float()
    elif family == "edge":
        x = x + torch.sign(x)                      # no value near zero on the ring
        if H > 2 and W > 2:
            x[:, 1:-1, 1:-1] = 0.0
    return x.to(torch.bfloat16)


def make_rows_bf16(family, n, rows_per_image, C, seed=0):
    """bf16 [n * rows_per_image, C] for the kernels that see rows only (ds gather, pool_ln, ap_tokens): FAMILIES_ROWS"""
    rows = n * rows_per_image
    if family in ("offset", "rowscale"):
        return R.make_rows(family, rows, C, seed=seed, bf16=True)[0]
    return make_map(family, n, rows_per_image, 1, C, seed).reshape(rows, C)


def make_conv_weights(family, Cin, Cout, seed=0):
    """(wk float32 [Cout, Kp] of bf16 values in the layout of tower_weights.resnet_conv3x3_weight — column (ky * 3 + kx) * Cin + c — with 3.0 in the K
    padding, bias fp32 [Cout])"""
    g = _seed(seed, Cin, Cout, 99)
    Kp = (9 * Cin + 63) // 64 * 64
    w = torch.randn(Cout, 9 * Cin, generator=g)
    w = torch.round(w).clamp(-2, 2) if family == "ramp" else w / (3 * Cin ** 0.5)
    wk = torch.full((Cout, Kp), 3.0)
    wk[:, :9 * Cin] = w
    b = 0.1 * torch.randn(Cout, generator=g)
    if family == "ramp":
        b = torch.round(b * 40)
    return wk.to(torch.bfloat16).float(), b


def make_dw_weights(family, C, seed=0):
    """(taps fp32 [49, C] as tower_weights.convnext_dw_taps lays them out, bias fp32 [C])"""
    g = _seed(seed, C, 98)
    taps = torch.randn(49, C, generator=g) / 7
    b = 0.1 * torch.randn(C, generator=g)
    if family == "ramp":
        taps, b = torch.round(taps * 56).clamp(-16, 16) / 8, torch.round(b * 40)
    return taps.contiguous(), b


def make_stem_pixels(family, n, S, seed=0):
    """uint8 [n, S, S, 3]"""
    g = _seed(seed, n, S, 97)
    x = torch.randint(0, 256, (n, S, S, 3), generator=g)
    if family == "loud_image":
        x = x % 56
        x[1::2] += 200
    elif family == "ramp":
        i, y, xx, c = torch.meshgrid(torch.arange(n), torch.arange(S), torch.arange(S), torch.arange(3), indexing="ij")
        x = (31 * i + 7 * y + 3 * xx + 11 * c) % 256
    elif family == "edge":
        x = x.clamp(min=1)
        if S > 2:
            x[:, 1:-1, 1:-1] = 0
    return x.to(torch.uint8)


def stem_f32_of_u8(u8, mean, std):
    """the float32 (b / 255 - mean) / std of uint8 [n, S, S, 3], as [n, 3, S, S]: what stem_gather_kernel<true> computes before it rounds"""
    m = torch.tensor(mean, dtype=torch.float32).view(1, 1, 1, 3)
    s = torch.tensor(std, dtype=torch.float32).view(1, 1, 1, 3)
    return ((u8.float() / 255.0 - m) / s).permute(0, 3, 1, 2).contiguous()


def make_attend(family, n, T, C, seed=0):
    """(q bf16 [n, C], kv bf16 [n, T, 2 C])"""
    assert family in FAMILIES_ATTEND
    g = _seed(seed, n, T, C, FAMILIES_ATTEND.index(family))
    heads = C // 64
    q = torch.randn(n, heads, 64, generator=g) / 4
    k = torch.randn(n, T, heads, 64, generator=g)
    v = torch.randn(n, T, heads, 64, generator=g)
    if family == "loud_image":
        v[1::2] += 50.0
    elif family == "ramp":
        i, t, h, d = torch.meshgrid(torch.arange(n), torch.arange(T), torch.arange(heads), torch.arange(64), indexing="ij")
        v = ((37 * i + 11 * t + 5 * h + 3 * d) % 127 - 63).float()
    elif family == "peaked":
        for i in range(n):
            for h in range(heads):
                k[i, (7 * i + 13 * h) % T, h] += 30.0 * q[i, h] / (q[i, h] * q[i, h]).sum()
    elif family == "offset":
        q = torch.full_like(q, 1.25)
        k = k + 1.0
    elif family == "one_loud_value":
        for i in range(n):
            v[i, (5 * i + 3) % T] *= 1000.0
    kv = torch.cat([k.reshape(n, T, C), v.reshape(n, T, C)], dim=2)
    return q.reshape(n, C).to(torch.bfloat16), kv.to(torch.bfloat16)


# ---- references and budgets (float64, on the device of the inputs) ------------------------------------------------------------------------------------
def hb(ref, B):
    return R.half_ulp_bf16(ref.abs() + B)


def ratio(got, ref, bound):
    return R.ratio(got, ref, bound)


def _pad_hw(x, p):
    n, H, W, C = x.shape
    out = torch.zeros(n, H + 2 * p, W + 2 * p, C, dtype=torch.float64, device=x.device)
    out[:, p:p + H, p:p + W] = x.double()
    return out


def reference_conv3x3(x, wk, bias, relu):
    """x bf16 [n, H, W, Cin], wk [Cout, Kp], bias [Cout] -> (ref, bound) float64 [n H W, Cout]; the K padding of wk is not read"""
    n, H, W, Cin = x.shape
    xp = _pad_hw(x, 1)
    w = wk.double().to(x.device)
    pre = bias.double().to(x.device)[None, :].repeat(n * H * W, 1)
    S = torch.zeros_like(pre)
    for ky in range(3):
        for kx in range(3):
            t = ky * 3 + kx
            xs = xp[:, ky:ky + H, kx:kx + W].reshape(n * H * W, Cin)
            wt = w[:, t * Cin:(t + 1) * Cin]
            pre += xs @ wt.t()
            S += xs.abs() @ wt.abs().t()
    ref = pre.clamp_min(0) if relu else pre
    B = 18 * Cin * U * S + U * pre.abs()
    return ref, B + hb(ref, B)


def reference_dwconv(x, taps, bias):
    """x bf16 [n, H, W, C], taps [49, C] (tap ky * 7 + kx), bias [C] -> (ref, bound) float64 [n, H, W, C]"""
    n, H, W, C = x.shape
    xp = _pad_hw(x, 3)
    t = taps.double().to(x.device)
    ref = bias.double().to(x.device).expand(n, H, W, C).clone()
    S = ref.abs()
    for ky in range(7):
        for kx in range(7):
            term = xp[:, ky:ky + H, kx:kx + W] * t[ky * 7 + kx]
            ref += term
            S += term.abs()
    B = 49 * U * S
    return ref, B + hb(ref, B)


def reference_partials(y):
    """y bf16 [rows, C] as the kernel stored it -> (ref, bound) float64 [C / 64, rows, 2]"""
    rows, C = y.shape
    v = y.double().reshape(rows, C // 64, 64).transpose(0, 1)
    ref = torch.stack([v.sum(-1), (v * v).sum(-1)], -1)
    return ref, 11 * U * torch.stack([v.abs().sum(-1), (v * v).sum(-1)], -1)


def _quads(x):
    """[n, H, W, C] -> the four pixels of every 2x2 window, [(ky, kx)][n, H/2, W/2, C]"""
    return [x[:, ky::2, kx::2] for ky in range(2) for kx in range(2)]


def reference_avgpool2(x):
    """-> (ref, bound) float64 [n (H/2) (W/2), C]"""
    C = x.shape[-1]
    q = _quads(x.double())
    ref = (q[0] + q[1] + q[2] + q[3]) / 4
    B = 2 * U * (q[0].abs() + q[1].abs() + q[2].abs() + q[3].abs()) / 4
    return ref.reshape(-1, C), (B + hb(ref, B)).reshape(-1, C)


def stats_f32(x, eps):
    """x bf16 [n, H, W, C] -> fp32 [n H W, 2]: float64 (mean, rstd) of every pixel, rounded to fp32"""
    xd = x.double().reshape(-1, x.shape[-1])
    mu = xd.mean(-1)
    return torch.stack([mu, 1.0 / ((xd - mu[:, None]).pow(2).mean(-1) + eps).sqrt()], -1).float()


def reference_ds_gather(x, stats, g, b):
    """x bf16 [n, H, W, C], stats fp32 [n H W, 2] -> (ref, bound) float64 [n (H/2) (W/2), 4 C], column (ky * 2 + kx) * C + c"""
    n, H, W, C = x.shape
    st = stats.double().reshape(n, H, W, 2)
    t = (x.double() - st[..., :1]) * st[..., 1:] * g.double()
    y = t + b.double()
    B = 3 * U * t.abs() + U * y.abs()
    B = B + hb(y, B)
    cat = lambda a: torch.cat(_quads(a), dim=-1).reshape(-1, 4 * C)
    return cat(y), cat(B)


def reference_stem(pixels, is_u8, mean=None, std=None):
    """pixels uint8 [n, S, S, 3] or fp32 [n, 3, S, S] -> (ref, bound) float64 [n (S/2)^2, 64]: column (ky * 3 + kx) * 3 + c = the normalised pixel
    (2 oy + ky - 1, 2 ox + kx - 1), zero outside the image and from column 27 on (ref and bound both 0 there: those must be exact)"""
    if is_u8:
        m = torch.tensor(mean, dtype=torch.float32, device=pixels.device).double()
        s = torch.tensor(std, dtype=torch.float32, device=pixels.device).double()
        v = pixels.double() / 255
        y = (v - m) / s
        B = U * (v.abs() + (v - m).abs()) / s.abs() + 2 * U * y.abs()
    else:
        y = pixels.double().permute(0, 2, 3, 1)
        B = torch.zeros_like(y)
    B = B + hb(y, B)
    n, S = y.shape[:2]
    G = S // 2
    yp = torch.zeros(n, S + 2, S + 2, 3, dtype=torch.float64, device=y.device)
    Bp = torch.zeros_like(yp)
    yp[:, 1:-1, 1:-1], Bp[:, 1:-1, 1:-1] = y, B
    ref = torch.zeros(n, G, G, 64, dtype=torch.float64, device=y.device)
    bound = torch.zeros_like(ref)
    for ky in range(3):
        for kx in range(3):
            t = ky * 3 + kx
            ref[..., 3 * t:3 * t + 3] = yp[:, ky:ky + S:2, kx:kx + S:2]
            bound[..., 3 * t:3 * t + 3] = Bp[:, ky:ky + S:2, kx:kx + S:2]
    return ref.reshape(-1, 64), bound.reshape(-1, 64)


def reference_tokens(x, pos):
    """x bf16 [n, HW, C], pos fp32 [HW + 1, C] -> (ref, bound) float64 [n, HW + 1, C]"""
    xd, p = x.double(), pos.double()
    HW = x.shape[1]
    ref = torch.cat([xd.mean(1, keepdim=True), xd], 1) + p
    B = U * ref.abs()
    B[:, 0] += (HW + 2) * U * xd.abs().sum(1) / HW
    return ref, B + hb(ref, B)


def pool_chain(C):
    return math.ceil(C / 256) + 10


def reference_pool_ln(x, g, b, eps):
    """x bf16 [n, HW, C] -> (ref, bound of the fp32 output) float64 [n, C]; the bf16 output adds hb(ref, bound)"""
    xd = x.double()
    n, HW, C = xd.shape
    m = xd.mean(1)
    e = (HW + 2) * U * xd.abs().mean(1)
    mu, d, sp, A = R.row_moments(m, eps)
    gd, bd = g.double(), b.double()
    y = d / sp * gd + bd
    D = pool_chain(C)
    c = D * U * A
    rho = (D / 2 + 4) * U + c * c / (2 * sp * sp)
    B = gd.abs() / sp * (c + 2 * U * d.abs()) + (gd * d).abs() / sp * rho + 2 * U * y.abs()
    rms = e.pow(2).mean(-1, keepdim=True).sqrt()
    Bin = gd.abs() / sp * (e + e.mean(-1, keepdim=True)) + (gd * d).abs() / (sp * sp) * rms
    return y, B + Bin * (1 + 4 * e.max(-1, keepdim=True).values / sp)


def reference_attend(q, kv):
    """q bf16 [n, C], kv bf16 [n, T, 2 C] -> (ref, bound) float64 [n, C]"""
    n, T, C2 = kv.shape
    C, Hh = C2 // 2, C2 // 128
    qd = q.double().reshape(n, Hh, 1, 64)
    k = kv[..., :C].double().reshape(n, T, Hh, 64).transpose(1, 2)             # [n, heads, T, 64]
    v = kv[..., C:].double().reshape(n, T, Hh, 64).transpose(1, 2)
    s = (qd * k).sum(-1)                                                       # [n, heads, T]
    ds = 64 * U * (qd * k).abs().sum(-1)
    x = s - s.max(-1, keepdim=True).values
    P = torch.softmax(s, -1)
    eta = 2 * ds + (3 * x.abs() + 4) * U
    out = (P[..., None] * v).sum(2)                                            # [n, heads, 64]
    PV = (P[..., None] * v.abs()).sum(2)
    B = ((P * eta)[..., None] * (v.abs() + out.abs()[:, :, None])).sum(2) + (T + 1) * U * PV + (math.ceil(T / 64) + 8) * U * out.abs()
    out, B = out.reshape(n, C), B.reshape(n, C)
    return out, B + hb(out, B)


# ---- float32 models ---------------------------------------------------------------------------------------------------------------------------
round_bf16 = R.round_bf16


def _np(t):
    return t.float().numpy() if isinstance(t, torch.Tensor) else np.asarray(t, dtype=np.float32)


def _fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _take(flat, idx):
    return np.take(flat, idx, mode="clip")


def _check_fault(kernel, fault):
    assert fault is None or fault in FAULTS[kernel], (kernel, fault)


def model_conv3x3(x, wk, bias, relu, fault=None):
    """conv3x3_kernel: per-row 9-bit tap mask; a lane's 16-byte chunk of a k-step is 8 channels of ONE tap, (tap, c) walking by 64 per k-step; taps >= 9
    (K padding) and rows >= M read the zero line; one fp32 rounding per 32-wide MFMA; bias, ReLU, bf16.  -> float32 [M, Cout] of bf16 values"""
    _check_fault("conv3x3", fault)
    xn, w, bn = _np(x), _np(wk), _np(bias)
    n, H, W, Cin = xn.shape
    M, Kp = n * H * W, w.shape[1]
    flat = xn.reshape(-1)
    BM = 64
    Mp = -(-M // BM) * BM
    r = np.arange(Mp)
    rem = r % (H * W)
    if fault == "hw_swap":
        yy = rem // H
        xx = rem - yy * H
    else:
        yy = rem // W
        xx = rem - yy * W

    def dydx(t):
        return (t % 3 - 1, t // 3 - 1) if fault == "tap_transposed" else (t // 3 - 1, t % 3 - 1)

    mask = np.zeros((Mp, 9), bool)
    for t in range(9):
        dy, dx = dydx(t)
        iy, ix = yy + dy, xx + dx
        okx = (ix >= 0) & (ix < (W - 1 if fault == "drop_right" else W))
        oky = ((r + dy * W + dx >= 0) & (r + dy * W + dx < M)) if fault == "halo_neighbour" else ((iy >= 0) & (iy < H))
        mask[:, t] = okx & oky & (r < M)
    A = np.zeros((Mp, Kp), np.float32)
    for l in range(8):                                                          # the logical 16-byte chunk a lane stages
        tap = (l * 8) // Cin
        cc = l * 8 - tap * Cin
        for ks in range(Kp // 64):
            in_k = tap < 9
            if in_k or fault == "kpad_tap0":
                t = tap if in_k else 0
                dy, dx = dydx(t)
                idx = ((r + dy * W + dx) * Cin + cc)[:, None] + np.arange(8)[None, :]
                A[:, ks * 64 + l * 8:ks * 64 + l * 8 + 8] = np.where(mask[:, t][:, None], _take(flat, idx), np.float32(0))
            cc += 64
            if fault == "walk_once":
                if cc >= Cin:
                    cc -= Cin
                    tap += 1
            else:
                while cc >= Cin:
                    cc -= Cin
                    tap += 1
    acc = np.zeros((Mp, w.shape[0]), np.float32)
    for k0 in range(0, Kp, 32):
        acc = (acc.astype(np.float64) + A[:, k0:k0 + 32].astype(np.float64) @ w[:, k0:k0 + 32].astype(np.float64).T).astype(np.float32)
    out = acc + bn[None, :]
    if relu:
        out = np.maximum(out, np.float32(0))
    return round_bf16(out[:M])                                                  # the row guard: rows >= M are not stored


def model_dwconv(x, taps, bias, fault=None):
    """dwconv7_kernel: 8 x 16 output tiles with a 3-pixel halo staged with zero padding, bias first, 49 fmas in (ky, kx) order, bf16; the partials of the
    STORED values: a lane's 8 channels as four pair sums / eight fmas, three xor levels over the 8 lanes of a 64-channel slot, slot-major.
    -> (y float32 [n, H, W, C] of bf16 values, partials float32 [C / 64, n H W, 2] — NaN where nothing was written)"""
    _check_fault("dwconv7", fault)
    xn, tn, bn = _np(x), _np(taps), _np(bias)
    n, H, W, C = xn.shape
    rows, nslots = n * H * W, C // 64
    flat = xn.reshape(rows, C)
    y = np.full((rows, C), np.nan, np.float32)
    part = np.full((nslots * rows, 2), np.nan, np.float32)
    lanes = np.arange(8)
    for img in range(n):
        for ty0 in range(0, H, 8):
            for tx0 in range(0, W, 16):
                iy = (ty0 - 3 + np.arange(14))[:, None]
                ix = (tx0 - 3 + np.arange(22))[None, :]
                pix = (img * H + iy) * W + ix if fault != "hw_swap" else (img * H * W + iy * H + ix)
                okx = (ix >= 0) & (ix < W)
                oky = ((pix >= 0) & (pix < rows)) if fault == "halo_neighbour" else ((iy >= 0) & (iy < H))
                tile = np.where((okx & oky)[..., None], flat[np.clip(pix, 0, rows - 1)], np.float32(0))      # [14, 22, C]
                acc = np.broadcast_to(bn, (8, 16, C)).astype(np.float32)
                for ky in range(7):
                    for kx in range(7):
                        acc = _fma(tile[ky:ky + 8, kx:kx + 16], tn[ky * 7 + kx][None, None, :], acc)
                st = round_bf16(acc)
                v = (acc if fault == "partials_unrounded" else st).reshape(8, 16, nslots, 8, 8)               # [.., slot, lane, its 8 channels]
                s1 = np.zeros(v.shape[:-1], np.float32)
                s2 = np.zeros(v.shape[:-1], np.float32)
                for k in range(4):
                    s1 = s1 + (v[..., 2 * k] + v[..., 2 * k + 1])
                    s2 = _fma(v[..., 2 * k], v[..., 2 * k], _fma(v[..., 2 * k + 1], v[..., 2 * k + 1], s2))
                for o in (1, 2, 4):
                    s1 = s1 + s1[..., lanes ^ o]
                    s2 = s2 + s2[..., lanes ^ o]
                for oy in range(min(8, H - ty0)):
                    for ox in range(min(16, W - tx0)):
                        prow = (img * H + ty0 + oy) * W + tx0 + ox
                        y[prow] = st[oy, ox]
                        for slot in range(nslots):
                            at = prow * nslots + slot if fault == "partials_pixel_major" else slot * rows + prow
                            part[at] = (s1[oy, ox, slot, 0], s2[oy, ox, slot, 0])
    return y.reshape(n, H, W, C), part.reshape(nslots, rows, 2)


def _out_rows(n, H, W, fault):
    """(img, oy, ox) of every output row of the two 2x2 kernels"""
    Ho, Wo = H // 2, W // 2
    orow = np.arange(n * Ho * Wo)
    img = orow // (Ho * Wo)
    rem = orow - img * Ho * Wo
    div = Ho if fault == "hw_swap" else Wo
    oy = rem // div
    return img, oy, rem - oy * div


def model_avgpool2(x, fault=None):
    """avgpool2_kernel: ((a + b) + (c + d)) * 0.25 with c, d one input row (W pixels) below -> float32 [n (H/2) (W/2), C] of bf16 values"""
    _check_fault("avgpool2", fault)
    xn = _np(x)
    n, H, W, C = xn.shape
    flat = xn.reshape(-1, C)
    img, oy, ox = _out_rows(n, H, W, fault)
    i0 = (img * H + 2 * oy) * W + 2 * ox
    step = H if fault == "second_row_at_h" else W
    px = lambda i: flat[np.clip(i, 0, flat.shape[0] - 1)]
    return round_bf16(((px(i0) + px(i0 + 1)) + (px(i0 + step) + px(i0 + step + 1))) * np.float32(0.25))


def model_ds_gather(x, stats, g, b, fault=None, fma=False):
    """ds_gather_kernel: quadrant q = ky * 2 + kx of output row (img, oy, ox) is input pixel (2 oy + ky, 2 ox + kx), ((x - mean) * rstd) * g + b
    (fma: the last product and the add contracted) -> float32 [n (H/2) (W/2), 4 C] of bf16 values"""
    _check_fault("ds_gather", fault)
    xn, sn, gn, bn = _np(x), _np(stats), _np(g), _np(b)
    n, H, W, C = xn.shape
    flat = xn.reshape(-1, C)
    img, oy, ox = _out_rows(n, H, W, fault)
    out = np.zeros((img.size, 4 * C), np.float32)
    for q in range(4):
        ky, kx = (q & 1, q >> 1) if fault == "quadrant_kx_ky" else (q >> 1, q & 1)
        irow = np.clip((img * H + 2 * oy + ky) * W + 2 * ox + kx, 0, flat.shape[0] - 1)
        t = (flat[irow] - sn[irow, :1]) * sn[irow, 1:]
        out[:, q * C:(q + 1) * C] = _fma(t, gn[None, :], np.broadcast_to(bn, t.shape)) if fma else t * gn + bn
    return round_bf16(out)


def model_stem(pixels, is_u8, mean=None, std=None, fault=None):
    """stem_gather_kernel<U8>: one output row per (img, oy, ox), 27 taps of pixel (2 oy + ky - 1, 2 ox + kx - 1), zeros outside and from column 27 on
    -> float32 [n (S/2)^2, 64] of bf16 values"""
    _check_fault("stem_gather", fault)
    if is_u8:
        px = pixels.numpy().astype(np.float32)                                        # [n, S, S, 3]
        m, s = np.asarray(mean, np.float32), np.asarray(std, np.float32)
        if fault == "mean0":
            m = np.full(3, m[0], np.float32)
        val = (px / np.float32(255.0) - m) / s
    else:
        val = np.ascontiguousarray(_np(pixels).transpose(0, 2, 3, 1))
    n, S = val.shape[:2]
    G = S // 2
    r = np.arange(n * G * G)
    img = r // (G * G)
    rem = r - img * G * G
    oy = rem // G
    ox = rem - oy * G
    if fault == "hw_swap":
        oy, ox = ox, oy
    out = np.zeros((r.size, 64), np.float32)
    lift = 0 if fault == "origin_2oy" else 1
    for t in range(9):
        iy, ix = 2 * oy + t // 3 - lift, 2 * ox + t % 3 - 1
        ok = (iy >= 0) & (iy < S) & (ix >= 0) & (ix < S)
        out[:, 3 * t:3 * t + 3] = np.where(ok[:, None], val[img, np.clip(iy, 0, S - 1), np.clip(ix, 0, S - 1)], np.float32(0))
    return round_bf16(out)


def model_tokens(x, pos):
    """ap_tokens_kernel: row 0 = (sequential fp32 sum over the pixels) * fl(1 / HW) + pos[0], row 1 + p = x[p] + pos[1 + p]"""
    xn, pn = _np(x), _np(pos)
    n, HW, C = xn.shape
    s = np.zeros((n, C), np.float32)
    for p in range(HW):
        s = s + xn[:, p]
    inv = np.float32(1.0) / np.float32(HW)
    return round_bf16(np.concatenate([(s * inv + pn[0])[:, None], xn + pn[None, 1:]], 1))


def _block_sum256(v):
    """[n, C] -> [n]: thread c % 256 chains its elements, six xor levels per wave, (w0 + w1) + (w2 + w3)"""
    n, C = v.shape
    pad = np.zeros((n, -(-C // 256) * 256), np.float32)
    pad[:, :C] = v
    s = np.zeros((n, 256), np.float32)
    for i in range(pad.shape[1] // 256):
        s = s + pad[:, i * 256:(i + 1) * 256]
    w = np.stack([R._butterfly(s[:, k * 64:(k + 1) * 64]) for k in range(4)], 1)
    return (w[:, 0] + w[:, 1]) + (w[:, 2] + w[:, 3])


def model_pool_ln(x, g, b, eps):
    """pool_ln_kernel -> float32 [n, C] (the fp32 output; the bf16 output is its rounding)"""
    xn, gn, bn = _np(x), _np(g), _np(b)
    n, HW, C = xn.shape
    s = np.zeros((n, C), np.float32)
    for p in range(HW):
        s = s + xn[:, p]
    m = s * (np.float32(1.0) / np.float32(HW))
    mean = _block_sum256(m) / np.float32(C)
    d = m - mean[:, None]
    rstd = np.float32(1) / np.sqrt(_block_sum256(d * d) / np.float32(C) + np.float32(eps))
    return d * rstd[:, None] * gn + bn


def model_attend(q, kv, fault=None):
    """ap_attend_kernel: one wave per (image, head); lane = key for the scores (a 64-term fma chain), the max over all keys, exp(s - max), the lanes' own
    sums and six xor levels; lane = column for the T-term fma chain of the weighted sum; o / sum, bf16 -> float32 [n, C] of bf16 values"""
    _check_fault("ap_attend", fault)
    qn, kvn = _np(q), _np(kv)
    n, T, C2 = kvn.shape
    C, Hh = C2 // 2, C2 // 128
    flat = kvn.reshape(-1)
    img = np.arange(n)[:, None, None, None]
    h = np.arange(Hh)[None, :, None, None]
    t = np.arange(T)[None, None, :, None]
    d = np.arange(64)[None, None, None, :]
    hk = h * (C if fault == "head_stride_c" else 64)
    k = _take(flat, (img * T + t) * C2 + hk + d)                                       # [n, heads, T, 64]
    v = _take(flat, (img * T + t) * C2 + C + h * 64 + d)
    qh = qn.reshape(n, Hh, 1, 64)
    s = np.zeros((n, Hh, T), np.float32)
    for j in range(64):
        s = _fma(np.broadcast_to(qh[..., j], s.shape), k[..., j], s)
    Te = T - T % 64 if fault == "skip_tail" else T
    with np.errstate(all="ignore"):
        mx = s[..., :Te].max(-1, keepdims=True) if Te else np.full((n, Hh, 1), -np.inf, np.float32)
        e = np.exp(s if fault == "no_max" else s - mx).astype(np.float32)
        e[..., Te:] = 0
        pad = np.zeros((n, Hh, -(-T // 64) * 64), np.float32)
        pad[..., :T] = e
        lane = np.zeros((n, Hh, 64), np.float32)
        for i in range(pad.shape[-1] // 64):
            lane = lane + pad[..., i * 64:(i + 1) * 64]
        tot = R._butterfly(lane.reshape(-1, 64)).reshape(n, Hh, 1)
        o = np.zeros((n, Hh, 64), np.float32)
        for tt in range(Te):
            o = _fma(np.broadcast_to(e[..., tt:tt + 1], o.shape), v[:, :, tt], o)
        return round_bf16((o / tot).reshape(n, C))

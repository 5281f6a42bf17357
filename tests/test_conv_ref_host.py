"""What the budgets of the convolutional towers' kernel tests can and cannot see, shown without a GPU (tests/conv_ref.py).

1. The float32 models of conv3x3, dwconv7 (values and partials), avgpool2, the downsample gather, the stem gather, the attention-pool tokens, the
   pooled LayerNorm and the single-query attention stay within 1.0 x budget of the float64 references on every shape and family that
   tests/test_conv_kernels_gpu.py runs (the worst ratios are printed, and quoted at the tests).
2. Each model with ONE deliberate fault leaves 1.25 x budget on the case FAULT_CASES names for it.
3. The float64 references equal torch.nn.functional in float64 on the CPU."""
import functools

import pytest
import torch
import torch.nn.functional as F

from marqo_amd.engine import tower_weights
from tests import conv_ref as K
from tests import rowops_ref as R

T = torch.from_numpy
EPS_DS = 1e-6


def _report(name, worst):
    print(f"CONV_MODEL kernel={name} worst ratio: " + "  ".join(f"{f} {r:.3f}" for f, r in sorted(worst.items())))


# ---- case runners: (kernel, shape, family, fault) -> worst |model - fp64| / budget ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _conv_inputs(H, W, n, Cin, Cout, relu, fam):
    x = K.make_map(fam, n, H, W, Cin, seed=1)
    wk, b = K.make_conv_weights(fam, Cin, Cout, seed=1)
    return x, wk, b, K.reference_conv3x3(x, wk, b, relu)


def conv_ratio(H, W, n, Cin, Cout, relu, fam, fault=None):
    x, wk, b, (ref, B) = _conv_inputs(H, W, n, Cin, Cout, relu, fam)
    return K.ratio(T(K.model_conv3x3(x, wk, b, relu, fault)), ref, B)


def dw_ratios(H, W, n, C, fam, fault=None):
    """(y, partials): partials against the sums of the values the MODEL stored; an element that was not written, or one written outside, gives inf"""
    x = K.make_map(fam, n, H, W, C, seed=2)
    taps, b = K.make_dw_weights(fam, C, seed=2)
    ref, B = K.reference_dwconv(x, taps, b)
    y, part = K.model_dwconv(x, taps, b, fault)
    pref, pB = K.reference_partials(T(y).reshape(-1, C).to(torch.bfloat16))
    return K.ratio(T(y), ref, B), K.ratio(T(part), pref, pB)


def pool2_ratio(H, W, C, fam, fault=None):
    x = K.make_map(fam, K.POOL2_N, H, W, C, seed=3)
    ref, B = K.reference_avgpool2(x)
    return K.ratio(T(K.model_avgpool2(x, fault)), ref, B)


def ds_ratio(H, W, C, fam, fault=None, fma=False):
    n = K.POOL2_N
    x = K.make_rows_bf16(fam, n, H * W, C, seed=4).reshape(n, H, W, C)
    g, b = R.make_rows("randn", 1, C, seed=4)[1:]
    st = K.stats_f32(x, EPS_DS)
    ref, B = K.reference_ds_gather(x, st, g, b)
    return K.ratio(T(K.model_ds_gather(x, st, g, b, fault, fma)), ref, B)


def stem_ratio(S, fam, norm, is_u8, fault=None):
    mean, std = K.STEM_NORMS[norm]
    u8 = K.make_stem_pixels(fam, K.STEM_N, S, seed=5)
    px = u8 if is_u8 else K.stem_f32_of_u8(u8, mean, std)
    ref, B = K.reference_stem(px, is_u8, mean, std)
    return K.ratio(T(K.model_stem(px, is_u8, mean, std, fault)), ref, B)


def attend_ratio(Tk, C, fam, fault=None):
    q, kv = K.make_attend(fam, K.ATT_N, Tk, C, seed=6)
    ref, B = K.reference_attend(q, kv)
    return K.ratio(T(K.model_attend(q, kv, fault)), ref, B)


# ---- 1. the fault-free models stay inside ------------------------------------------------------------------------------------------------------------
# Worst ratios seen here (printed by the tests).  A bf16 output next to a rounding tie uses the whole half ulp, as it must, so ~1.00 is the expected
# figure for the bf16 stores; the fp32 quantities show what the arithmetic itself uses:
#   conv3x3 randn 0.993, loud_image 0.996, ramp 0.997, edge 0.999; dwconv7 0.999 on all four; its partials randn 0.217, loud_image 0.204, ramp 0.198,
#   edge 0.209; avgpool2 1.000 (exact ties; ramp 0: exact); ds gather, stem gather, ap_tokens, pool_ln (bf16 out) 0.999 - 1.000;
#   ap_attend randn 0.942, loud_image 0.943, ramp 0.934, peaked 0.000 (the winning key's value is the output), offset 0.687, one_loud_value 0.947
def test_conv_cases_cover_every_value():
    for key, vals in (("Cin", K.CONV_CIN), ("Cout", K.CONV_COUT), ("n", K.CONV_N), ("relu", (0, 1)), ("store", K.CONV_STORE)):
        assert {c[key] for c in K.CONV_CASES} == set(vals), key
    assert {(c["H"], c["W"], c["Cin"]) for c in K.CONV_CASES} == {(h, w, ci) for h, w in K.CONV_HW for ci in K.CONV_CIN}
    assert any(c["n"] * c["H"] * c["W"] == 135 for c in K.CONV_CASES) and any(c["n"] * c["H"] * c["W"] < 64 for c in K.CONV_CASES)
    # both store widths at a Cout that is a multiple of 8 and at one that is not
    assert {(c["Cout"] % 8 == 0, c["store"]) for c in K.CONV_CASES} == {(a, s) for a in (True, False) for s in K.CONV_STORE}


def test_model_of_conv3x3_stays_inside_the_budget():
    worst = {}
    for c in K.CONV_CASES:
        for fam in K.FAMILIES_MAP:
            r = conv_ratio(c["H"], c["W"], c["n"], c["Cin"], c["Cout"], c["relu"], fam)
            assert r <= 1.0, (c, fam, r)
            worst[fam] = max(worst.get(fam, 0.0), r)
    _report("conv3x3", worst)


def test_model_of_dwconv7_and_its_partials_stays_inside_the_budget():
    wy, wp = {}, {}
    for H, W in K.DW_HW:
        for C in K.DW_C:
            for n in K.DW_N:
                for fam in K.FAMILIES_MAP:
                    ry, rp = dw_ratios(H, W, n, C, fam)
                    assert ry <= 1.0 and rp <= 1.0, (H, W, C, n, fam, ry, rp)
                    wy[fam], wp[fam] = max(wy.get(fam, 0.0), ry), max(wp.get(fam, 0.0), rp)
    _report("dwconv7", wy)
    _report("dwconv7_partials", wp)


def test_models_of_avgpool2_and_the_downsample_gather_stay_inside_the_budget():
    wa, wd = {}, {}
    for H, W in K.POOL2_HW:
        for C in K.POOL2_C:
            for fam in K.FAMILIES_MAP:
                r = pool2_ratio(H, W, C, fam)
                assert r <= 1.0, (H, W, C, fam, r)
                wa[fam] = max(wa.get(fam, 0.0), r)
            for fam in K.FAMILIES_ROWS:
                for fma in (False, True):
                    r = ds_ratio(H, W, C, fam, fma=fma)
                    assert r <= 1.0, (H, W, C, fam, fma, r)
                    wd[fam] = max(wd.get(fam, 0.0), r)
    _report("avgpool2", wa)
    _report("ds_gather", wd)


def test_model_of_the_stem_gather_stays_inside_the_budget():
    worst = {}
    for S in K.STEM_S:
        for fam in K.FAMILIES_MAP:
            for norm in range(3):
                for is_u8 in (True, False):
                    r = stem_ratio(S, fam, norm, is_u8)
                    assert r <= 1.0, (S, fam, norm, is_u8, r)
                    worst[fam] = max(worst.get(fam, 0.0), r)
    _report("stem_gather", worst)


def test_model_of_the_attention_pool_tokens_stays_inside_the_budget():
    worst = {}
    for HW in K.TOK_HW:
        for C in K.TOK_C:
            for fam in K.FAMILIES_ROWS:
                x = K.make_rows_bf16(fam, 3, HW, C, seed=7).reshape(3, HW, C)
                pos = torch.randn(HW + 1, C, generator=torch.Generator().manual_seed(HW + C)) / C ** 0.5
                ref, B = K.reference_tokens(x, pos)
                r = K.ratio(T(K.model_tokens(x, pos)), ref, B)
                assert r <= 1.0, (HW, C, fam, r)
                worst[fam] = max(worst.get(fam, 0.0), r)
    _report("ap_tokens", worst)


def test_model_of_pool_ln_stays_inside_the_budget():
    worst = {}
    for C in K.POOL_LN_C:
        for HW in K.POOL_LN_HW:
            for fam in K.FAMILIES_ROWS:
                for eps in (1e-5, 1e-6):
                    x = K.make_rows_bf16(fam, 3, HW, C, seed=8).reshape(3, HW, C)
                    g, b = R.make_rows("randn", 1, C, seed=8)[1:]
                    ref, B = K.reference_pool_ln(x, g, b, eps)
                    got = T(K.model_pool_ln(x, g, b, eps))
                    r = max(K.ratio(got, ref, B), K.ratio(got.to(torch.bfloat16), ref, B + K.hb(ref, B)))
                    assert r <= 1.0, (C, HW, fam, eps, r)
                    worst[fam] = max(worst.get(fam, 0.0), r)
    _report("pool_ln", worst)


def test_model_of_the_single_query_attention_stays_inside_the_budget():
    worst = {}
    for Tk in K.ATT_T:
        for C in K.ATT_C:
            for fam in K.FAMILIES_ATTEND:
                r = attend_ratio(Tk, C, fam)
                assert r <= 1.0, (Tk, C, fam, r)
                worst[fam] = max(worst.get(fam, 0.0), r)
    _report("ap_attend", worst)


# ---- 2. single faults leave 1.25 x budget ------------------------------------------------------------------------------------------------------------
CONV = lambda i: tuple(K.CONV_CASES[i][k] for k in ("H", "W", "n", "Cin", "Cout", "relu"))
# (kernel, fault, the named case: arguments of the runner, family).  Every shape is one the GPU test runs; CONV(i) = (H, W, n, Cin, Cout, relu) of
# conv_ref.CONV_CASES[i]: 1 = 1x9 n 3 Cin 16, 2 = 5x3 n 9 Cin 24 (a tile spans five images), 14 = 6x11 n 9 Cin 8, 24 = 6x11 Cin 40, 28 = 7x7 Cin 8, 33 = 7x7 Cin 72
FAULT_CASES = [
    ("conv3x3", "hw_swap", CONV(24), "ramp"),
    ("conv3x3", "hw_swap", CONV(2), "randn"),
    ("conv3x3", "halo_neighbour", CONV(2), "loud_image"),
    ("conv3x3", "drop_right", CONV(1), "edge"),
    ("conv3x3", "tap_transposed", CONV(33), "randn"),
    ("conv3x3", "walk_once", CONV(14), "randn"),
    ("conv3x3", "walk_once", CONV(2), "ramp"),
    ("conv3x3", "kpad_tap0", CONV(28), "randn"),
    ("dwconv7", "hw_swap", (7, 33, 3, 64), "ramp"),
    ("dwconv7", "hw_swap", (20, 6, 1, 128), "randn"),
    ("dwconv7", "halo_neighbour", (3, 5, 3, 64), "loud_image"),
    ("dwconv7_partials", "partials_pixel_major", (9, 17, 1, 128), "randn"),
    ("dwconv7_partials", "partials_unrounded", (8, 16, 1, 64), "randn"),
    ("avgpool2", "hw_swap", (2, 6, 72), "ramp"),
    ("avgpool2", "second_row_at_h", (6, 4, 8), "randn"),
    ("ds_gather", "hw_swap", (6, 4, 72), "rowscale"),
    ("ds_gather", "quadrant_kx_ky", (2, 2, 8), "randn"),
    ("stem_gather", "hw_swap", (4, "ramp", 0, True), None),
    ("stem_gather", "mean0", (2, "randn", 1, True), None),
    ("stem_gather", "origin_2oy", (6, "edge", 2, False), None),
    ("ap_attend", "no_max", (256, 192), "offset"),
    ("ap_attend", "head_stride_c", (65, 192), "randn"),
    ("ap_attend", "skip_tail", (65, 192), "randn"),
    ("ap_attend", "skip_tail", (63, 192), "one_loud_value"),
]


def _run(kernel, args, fam, fault):
    if kernel == "conv3x3":
        return conv_ratio(*args, fam, fault)
    if kernel == "dwconv7":
        return dw_ratios(*args, fam, fault)[0]
    if kernel == "dwconv7_partials":
        return dw_ratios(*args, fam, fault)[1]
    if kernel == "avgpool2":
        return pool2_ratio(*args, fam, fault)
    if kernel == "ds_gather":
        return ds_ratio(*args, fam, fault)
    if kernel == "stem_gather":
        return stem_ratio(*args, fault=fault)
    return attend_ratio(*args, fam, fault)


def test_the_conv3x3_fault_cases_are_shapes_of_the_gpu_test():
    shapes = {CONV(i) for i in range(len(K.CONV_CASES))}
    for kernel, _, args, _ in FAULT_CASES:
        if kernel == "conv3x3":
            assert args in shapes, args


def test_every_listed_fault_has_a_case():
    have = {(k.replace("_partials", ""), f) for k, f, _, _ in FAULT_CASES}
    assert have == {(k, f) for k, fs in K.FAULTS.items() for f in fs}


@pytest.mark.parametrize("kernel,fault,args,fam", FAULT_CASES)
def test_single_faults_leave_the_budget(kernel, fault, args, fam):
    clean, bad = _run(kernel, args, fam, None), _run(kernel, args, fam, fault)
    print(f"CONV_FAULT kernel={kernel} fault={fault} case={args} family={fam}: clean {clean:.3f}, faulty {bad:.3g}")
    assert clean <= 1.0
    assert bad > 1.25, (kernel, fault, args, fam, bad)


def test_documented_exceptions_faults_that_stay_inside():
    """NOT caught, and why: hw_swap on a square map (the fault is a no-op: what the first-draft tests could not see); kpad_tap0 at Cin = 64 (9 Cin is a
    multiple of 64: there is no K padding); walk_once at Cin = 64 and 72 (one step per k-step is right from Cin = 64 on); no_max on `randn` (scores of a
    few units: exp stays in range and the softmax is the same number); skip_tail at T = 64 and 256 (no tail)."""
    assert conv_ratio(*CONV(18), "ramp", "hw_swap") == conv_ratio(*CONV(18), "ramp")
    assert conv_ratio(*CONV(18), "randn", "kpad_tap0") == conv_ratio(*CONV(18), "randn")
    assert conv_ratio(*CONV(18), "randn", "walk_once") <= 1.0
    assert conv_ratio(*CONV(5), "randn", "walk_once") <= 1.0
    assert attend_ratio(65, 64, "randn", "no_max") <= 1.25
    for Tk in (64, 256):
        assert attend_ratio(Tk, 64, "peaked", "skip_tail") == attend_ratio(Tk, 64, "peaked")


# ---- 3. the float64 references against torch.nn.functional --------------------------------------------------------------------------------------------
def _close(a, b, tol=1e-12):
    assert a.shape == b.shape
    assert float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


@pytest.mark.parametrize("n,H,W,Cin,Cout", [(2, 5, 3, 24, 36), (3, 6, 11, 8, 4)])
def test_reference_conv3x3_is_conv2d(n, H, W, Cin, Cout):
    g = torch.Generator().manual_seed(H * W)
    x = torch.randn(n, H, W, Cin, generator=g).to(torch.bfloat16)
    w = torch.randn(Cout, Cin, 3, 3, generator=g).to(torch.bfloat16).float()
    b = torch.randn(Cout, generator=g)
    wk = tower_weights.resnet_conv3x3_weight(w, Cin, Cout)
    wk[:, 9 * Cin:] = 3.0
    for relu in (0, 1):
        ref, _ = K.reference_conv3x3(x, wk, b, relu)
        want = F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), b.double(), padding=1).permute(0, 2, 3, 1).reshape(-1, Cout)
        _close(ref, want.clamp_min(0) if relu else want)


@pytest.mark.parametrize("n,H,W,C", [(2, 3, 5, 64), (1, 9, 17, 128)])
def test_reference_dwconv_is_grouped_conv2d(n, H, W, C):
    g = torch.Generator().manual_seed(H * W)
    x = torch.randn(n, H, W, C, generator=g).to(torch.bfloat16)
    w = torch.randn(C, 1, 7, 7, generator=g)
    b = torch.randn(C, generator=g)
    ref, _ = K.reference_dwconv(x, tower_weights.convnext_dw_taps(w), b)
    _close(ref, F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), b.double(), padding=3, groups=C).permute(0, 2, 3, 1))


@pytest.mark.parametrize("n,H,W,C", [(3, 2, 6, 8), (2, 6, 4, 72)])
def test_reference_avgpool2_and_ds_gather_are_avg_pool2d_and_layer_norm(n, H, W, C):
    g = torch.Generator().manual_seed(H * W)
    x = (0.5 + torch.randn(n, H, W, C, generator=g)).to(torch.bfloat16)
    ref, _ = K.reference_avgpool2(x)
    _close(ref, F.avg_pool2d(x.double().permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1).reshape(-1, C))
    lg, lb = torch.randn(C, generator=g), torch.randn(C, generator=g)
    ref, _ = K.reference_ds_gather(x, K.stats_f32(x, EPS_DS), lg, lb)
    want = tower_weights.convnext_downsample_gather(F.layer_norm(x.double(), (C,), lg.double(), lb.double(), EPS_DS))
    _close(ref, want, tol=1e-6)           # (the statistics are rounded to fp32 on purpose: they are the kernel's input)


@pytest.mark.parametrize("S,norm", [(4, 0), (6, 1)])
def test_reference_stem_is_the_stride_2_unfold(S, norm):
    mean, std = K.STEM_NORMS[norm]
    u8 = K.make_stem_pixels("randn", 2, S, seed=S)
    px = K.stem_f32_of_u8(u8, mean, std)
    ref, _ = K.reference_stem(px, False)
    cols = F.unfold(px.double(), 3, padding=1, stride=2)                    # [n, 3 * 9, G * G], row c * 9 + t
    want = cols.reshape(2, 3, 9, -1).permute(0, 3, 2, 1).reshape(-1, 27)
    _close(ref[:, :27], want)
    assert bool((ref[:, 27:] == 0).all())
    ref8, _ = K.reference_stem(u8, True, mean, std)
    _close(ref8, ref, tol=1e-6)


@pytest.mark.parametrize("n,HW,C", [(2, 7, 264), (3, 49, 8)])
def test_reference_pool_ln_and_tokens_are_layer_norm_and_mean(n, HW, C):
    g = torch.Generator().manual_seed(HW)
    x = torch.randn(n, HW, C, generator=g).to(torch.bfloat16)
    lg, lb = torch.randn(C, generator=g), torch.randn(C, generator=g)
    ref, _ = K.reference_pool_ln(x, lg, lb, 1e-5)
    _close(ref, F.layer_norm(x.double().mean(1), (C,), lg.double(), lb.double(), 1e-5))
    pos = torch.randn(HW + 1, C, generator=g)
    ref, _ = K.reference_tokens(x, pos)
    _close(ref, torch.cat([x.double().mean(1, keepdim=True), x.double()], 1) + pos.double())


@pytest.mark.parametrize("n,Tk,C", [(2, 5, 64), (3, 65, 192)])
def test_reference_attend_is_multi_head_attention_forward(n, Tk, C):
    q, kv = K.make_attend("randn", n, Tk, C, seed=Tk)
    ref, _ = K.reference_attend(q, kv)
    eye, zero = torch.eye(C, dtype=torch.float64), torch.zeros(3 * C, dtype=torch.float64)
    # the kernel's q already carries the 1 / 8 scale that multi_head_attention_forward applies itself: give it 8 q
    out, _ = F.multi_head_attention_forward(
        query=8 * q.double()[None], key=kv[..., :C].double().transpose(0, 1), value=kv[..., C:].double().transpose(0, 1), embed_dim_to_check=C,
        num_heads=C // 64, in_proj_weight=None, in_proj_bias=zero, bias_k=None, bias_v=None, add_zero_attn=False, dropout_p=0.0, out_proj_weight=eye,
        out_proj_bias=None, use_separate_proj_weight=True, q_proj_weight=eye, k_proj_weight=eye, v_proj_weight=eye, training=False, need_weights=False)
    _close(ref, out[0])

"""The kernels of the convolutional towers through the C ABI — mq_resnet_conv3x3 (both tile heights, both store widths), mq_convnext_dwconv and its
partials, mq_convnext_downsample, mq_resnet_avgpool2, mq_convnext_pool_ln, mq_resnet_stem_gather, mq_resnet_attnpool_tokens / _attend — on non-square
maps and at their edges, against the float64 references of tests/conv_ref.py.  Every assertion is elementwise  |kernel - reference| <= budget  over
ALL elements, with the budgets derived in conv_ref's docstring (tests/test_conv_ref_host.py shows that float32 models of the kernels stay within them
and that single indexing and arithmetic faults leave them by factors of hundreds and more on the shapes run here).

Every output is a window of a NaN-filled buffer: the columns from Cout to ldy, a guard in front of the first row and GUARD rows behind the last one must
come back bit for bit.  The shapes are the smallest at which each path can still go wrong (tests/test_convnext_gpu.py and tests/test_resnet_gpu.py keep
the towers' own shapes).

Every comparison notes its worst ratio; the module ends with one `CONV_WORST` line per (kernel, family) (run with -s)."""
import ctypes

import pytest
import torch

from marqo_amd import _lib as L
from tests import conv_ref as K
from tests import rowops_ref as R
from tests.knobs import tuned

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 4          # rows behind the output
FRONT = 64         # elements in front of it (a multiple of 16 bytes for every dtype used)
WORST = {}


@pytest.fixture(scope="module")
def lib():
    lib = L.load()
    yield lib
    for (kernel, fam), r in sorted(WORST.items()):
        print(f"CONV_WORST kernel={kernel} family={fam} ratio={r:.4f}")


def _s():
    return torch.cuda.current_stream().cuda_stream


def _note(kernel, fam, r):
    WORST[(kernel, fam)] = max(WORST.get((kernel, fam), 0.0), r)


def _hold(kernel, fam, got, ref, bound, what):
    r = K.ratio(got.cpu(), ref, bound)
    _note(kernel, fam, r)
    assert r <= 1.0, (kernel, fam, what, r)


class Window:
    """rows x cols of `dtype` with row stride ld, `shift` elements off a 16-byte line, inside a NaN-filled buffer"""

    def __init__(self, rows, cols, dtype, ld=None, shift=0):
        self.rows, self.cols, self.ld, self.start = rows, cols, ld or cols, FRONT + shift
        self.raw = torch.full((self.start + (rows + GUARD) * self.ld,), float("nan"), dtype=dtype, device=DEV)
        self.bits = self.raw.view(torch.int16 if self.raw.element_size() == 2 else torch.int32)
        self.sentinel = self.bits[0].item()

    def ptr(self):
        return self.raw.data_ptr() + self.start * self.raw.element_size()

    def _body(self, t):
        return t[self.start:self.start + self.rows * self.ld].view(self.rows, self.ld)

    def out(self):
        return self._body(self.raw)[:, :self.cols]

    def outside_intact(self):
        torch.cuda.synchronize()
        tail = self.bits[self.start + self.rows * self.ld:]
        return bool((self.bits[:self.start] == self.sentinel).all()) and bool((tail == self.sentinel).all()) and \
            bool((self._body(self.bits)[:, self.cols:] == self.sentinel).all())

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.bits == self.sentinel).all())


# ---- mq_resnet_conv3x3 -----------------------------------------------------------------------------------------------------------------------------
_CONV_CACHE = {}


def _conv_case(i, fam):
    """(x, wk, bias on the device, reference, bound) of conv_ref.CONV_CASES[i], computed once for both tile heights"""
    if (i, fam) not in _CONV_CACHE:
        c = K.CONV_CASES[i]
        x = K.make_map(fam, c["n"], c["H"], c["W"], c["Cin"], seed=1)
        wk, b = K.make_conv_weights(fam, c["Cin"], c["Cout"], seed=1)
        _CONV_CACHE[(i, fam)] = (x.to(DEV), wk.to(torch.bfloat16).to(DEV), b.to(DEV)) + K.reference_conv3x3(x, wk, b, c["relu"])
    return _CONV_CACHE[(i, fam)]


def _conv_call(lib, x, wk, b, Cout, relu, store="ldy=cout"):
    n, H, W, Cin = x.shape
    win = Window(n * H * W, Cout, torch.bfloat16, ld=Cout + 4 if store == "ldy=cout+4" else Cout, shift=4 if store == "misaligned" else 0)
    assert win.ptr() % 16 == (8 if store == "misaligned" else 0)
    L.check(lib.mq_resnet_conv3x3(x.data_ptr(), wk.data_ptr(), b.data_ptr(), win.ptr(), win.ld, n, H, W, Cin, Cout, relu, _s()))
    assert win.outside_intact(), (tuple(x.shape), Cout, store)
    return win.out()


@pytest.mark.parametrize("mt", (2, 4))
@pytest.mark.parametrize("i", range(len(K.CONV_CASES)))
def test_conv3x3_both_tile_heights_and_store_widths(lib, i, mt):
    """conv3x3_kernel<FLAGS, 2> and <FLAGS, 4> (mq_tune gemm_mt) on every case of conv_ref.CONV_CASES: non-square maps, maps below one tile, a tile that
    spans five images, Cin of 8 / 16 / 24 (several taps per k-step), the wide store (ldy % 8 == 0 on a 16-byte line) and the narrow one"""
    c = K.CONV_CASES[i]
    with tuned(gemm_mt=mt):
        for fam in K.FAMILIES_MAP:
            x, wk, b, ref, bound = _conv_case(i, fam)
            y = _conv_call(lib, x, wk, b, c["Cout"], c["relu"], c["store"])
            _hold(f"conv3x3/mt{mt}", fam, y, ref, bound, c)


def test_conv3x3_unforced_dispatch_runs_the_tile_heights_that_were_compared(lib):
    """With the knob at 0 the entry point picks MT = 4 from more than 512 MT = 2 tiles on (n = 9, 64 x 64, Cin 8, Cout 4: 36 864 rows = 576 tiles; 8 images
    are exactly 512 tiles, one round, and still MT = 2) and MT = 2 below: the unforced calls must give the bits of the forced ones — and the large one
    is held to the budget itself, since both tile heights add a row's k-steps in the same order and their bits may well agree."""
    for n, H, W, forced in ((9, 64, 64, 4), (3, 5, 3, 2)):
        x = K.make_map("loud_image", n, H, W, 8, seed=9)
        wk, b = K.make_conv_weights("loud_image", 8, 4, seed=9)
        ref, bound = K.reference_conv3x3(x, wk, b, 1)
        xd, wd, bd = x.to(DEV), wk.to(torch.bfloat16).to(DEV), b.to(DEV)
        auto = _conv_call(lib, xd, wd, bd, 4, 1)
        with tuned(gemm_mt=forced):
            pinned = _conv_call(lib, xd, wd, bd, 4, 1)
        assert torch.equal(auto, pinned)
        _hold("conv3x3/auto", "loud_image", auto, ref, bound, (n, H, W))


def test_conv3x3_refuses_bad_arguments_and_leaves_the_output_alone(lib):
    x = K.make_map("randn", 1, 5, 3, 16, seed=1).to(DEV)
    wk, b = K.make_conv_weights("randn", 16, 8, seed=1)
    wk, b = wk.to(torch.bfloat16).to(DEV), b.to(DEV)
    win = Window(15, 8, torch.bfloat16)
    call = lambda xp, yp, ldy, Cin, Cout, relu: lib.mq_resnet_conv3x3(xp, wk.data_ptr(), b.data_ptr(), yp, ldy, 1, 5, 3, Cin, Cout, relu, _s())
    before = x.clone()
    for what, args in (("Cin = 12", (x.data_ptr(), win.ptr(), 8, 12, 8, 0)), ("Cout = 6", (x.data_ptr(), win.ptr(), 8, 16, 6, 0)),
                       ("ldy < Cout", (x.data_ptr(), win.ptr(), 4, 16, 8, 0)), ("d_x == d_y", (x.data_ptr(), x.data_ptr(), 8, 16, 8, 0)),
                       ("relu = 2", (x.data_ptr(), win.ptr(), 8, 16, 8, 2))):
        assert call(*args) != L.MQ_OK and b"mq_resnet_conv3x3" in lib.mq_last_error(), what
        assert win.untouched() and torch.equal(x, before), what
    assert call(x.data_ptr(), win.ptr(), 8, 16, 8, 1) == L.MQ_OK and win.outside_intact()


# ---- mq_convnext_dwconv ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", K.DW_HW)
def test_dwconv7_values_partials_and_finalised_statistics(lib, H, W):
    """maps smaller than the halo, exactly one 8 x 16 tile, one past it both ways, several tiles in one direction only.  y against the float64
    convolution; the slot-major partials against the float64 sums of the values y holds, nothing written outside [C / 64, n H W]; the finalised
    (mean, rstd) against rowops_ref's finalise budget on those partials"""
    eps = 1e-6
    for C in K.DW_C:
        for n in K.DW_N:
            for fam in K.FAMILIES_MAP:
                x = K.make_map(fam, n, H, W, C, seed=2)
                taps, b = K.make_dw_weights(fam, C, seed=2)
                ref, bound = K.reference_dwconv(x, taps, b)
                rows, nslots = n * H * W, C // 64
                xd, td, bd = x.to(DEV), taps.to(DEV), b.to(DEV)
                y = Window(rows, C, torch.bfloat16)
                part = Window(nslots, rows * 2, torch.float32)
                L.check(lib.mq_convnext_dwconv(xd.data_ptr(), td.data_ptr(), bd.data_ptr(), y.ptr(), part.ptr(), n, H, W, C, _s()))
                assert y.outside_intact() and part.outside_intact(), (H, W, C, n, fam)
                what = (H, W, C, n)
                _hold("dwconv7", fam, y.out(), ref.reshape(rows, C), bound.reshape(rows, C), what)
                p = part.out().reshape(nslots, rows, 2)
                pref, pbound = K.reference_partials(y.out().cpu())
                _hold("dwconv7_partials", fam, p, pref, pbound, what)
                st = Window(rows, 2, torch.float32)
                L.check(lib.mq_row_stats_finalize(part.ptr(), nslots, st.ptr(), rows, C, eps, _s()))
                assert st.outside_intact()
                mu, t, cf, bt = R.finalize_reference(p.cpu(), C, eps)
                _hold("dwconv7_finalised_mean", fam, st.out()[:, 0], mu, cf, what)
                _hold("dwconv7_finalised_rstd", fam, st.out()[:, 1].double() ** -2, t, bt, what)


# ---- mq_convnext_downsample, mq_resnet_avgpool2 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", K.POOL2_HW)
def test_avgpool2_and_downsample_gather_on_non_square_maps(lib, H, W):
    n, eps = K.POOL2_N, 1e-6
    orows = n * (H // 2) * (W // 2)
    for C in K.POOL2_C:
        for fam in K.FAMILIES_MAP:
            x = K.make_map(fam, n, H, W, C, seed=3)
            ref, bound = K.reference_avgpool2(x)
            xd = x.to(DEV)
            out = Window(orows, C, torch.bfloat16)
            L.check(lib.mq_resnet_avgpool2(xd.data_ptr(), out.ptr(), n, H, W, C, _s()))
            assert out.outside_intact()
            _hold("avgpool2", fam, out.out(), ref, bound, (H, W, C))
        for fam in K.FAMILIES_ROWS:
            x = K.make_rows_bf16(fam, n, H * W, C, seed=4).reshape(n, H, W, C)
            g, b = R.make_rows("randn", 1, C, seed=4)[1:]
            st = K.stats_f32(x, eps)               # float64 statistics rounded to fp32, not mq_row_stats: the gather alone is under test
            ref, bound = K.reference_ds_gather(x, st, g, b)
            xd, sd, gd, bd = x.to(DEV), st.to(DEV), g.to(DEV), b.to(DEV)
            out = Window(orows, 4 * C, torch.bfloat16)
            L.check(lib.mq_convnext_downsample(xd.data_ptr(), sd.data_ptr(), gd.data_ptr(), bd.data_ptr(), out.ptr(), n, H, W, C, _s()))
            assert out.outside_intact()
            _hold("ds_gather", fam, out.out(), ref, bound, (H, W, C))


# ---- mq_convnext_pool_ln ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", K.POOL_LN_C)
def test_pool_ln_every_width_class_and_output_combination(lib, C):
    """C = 8 (most threads idle), 264 (a ragged second trip), 2048, 3072 (the LDS row's limit); bf16 only (what the tower asks), fp32 only, both —
    which must give the bits of the single-output calls"""
    n = 3
    for HW in K.POOL_LN_HW:
        for fam in K.FAMILIES_ROWS:
            for eps in (1e-5, 1e-6):
                x = K.make_rows_bf16(fam, n, HW, C, seed=8).reshape(n, HW, C)
                g, b = R.make_rows("randn", 1, C, seed=8)[1:]
                ref, bound = K.reference_pool_ln(x, g, b, eps)
                xd, gd, bd = x.to(DEV), g.to(DEV), b.to(DEV)
                got = {}
                for outs in ("bf16", "f32", "both"):
                    ob = Window(n, C, torch.bfloat16) if outs != "f32" else None
                    of = Window(n, C, torch.float32) if outs != "bf16" else None
                    L.check(lib.mq_convnext_pool_ln(xd.data_ptr(), gd.data_ptr(), bd.data_ptr(), ob.ptr() if ob else 0, of.ptr() if of else 0, n, HW, C,
                                                    eps, _s()))
                    assert (ob is None or ob.outside_intact()) and (of is None or of.outside_intact())
                    got[outs] = (ob.out() if ob else None, of.out() if of else None)
                _hold("pool_ln/fp32_out", fam, got["f32"][1], ref, bound, (C, HW, eps))
                _hold("pool_ln/bf16_out", fam, got["bf16"][0], ref, bound + K.hb(ref, bound), (C, HW, eps))
                assert torch.equal(got["both"][0], got["bf16"][0]) and torch.equal(got["both"][1], got["f32"][1])


# ---- mq_resnet_stem_gather ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", K.STEM_S)
def test_stem_gather_at_the_border(lib, S):
    """S = 2 and 4: every output row touches the border.  The u8 entry against (b / 255 - mean) / std in float64 with three sets of means and stds, the
    f32 entry against its own input; columns 27 .. 63 exactly zero (reference and budget are both 0 there); and the two entries bit for bit equal
    when the f32 input is the float32 (b / 255 - mean) / std of the u8 input"""
    n = K.STEM_N
    rows = n * (S // 2) ** 2
    for fam in K.FAMILIES_MAP:
        u8 = K.make_stem_pixels(fam, n, S, seed=5)
        for mean, std in K.STEM_NORMS:
            cm, cs = (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std)
            px = K.stem_f32_of_u8(u8, mean, std)
            got = []
            for is_u8, src in ((1, u8), (0, px)):
                ref, bound = K.reference_stem(src, bool(is_u8), mean, std)
                sd = src.to(DEV)
                out = Window(rows, 64, torch.bfloat16)
                L.check(lib.mq_resnet_stem_gather(sd.data_ptr(), is_u8, out.ptr(), n, S, ctypes.addressof(cm), ctypes.addressof(cs), _s()))
                assert out.outside_intact()
                _hold("stem_gather/" + ("u8" if is_u8 else "f32"), fam, out.out(), ref, bound, (S, mean))
                assert bool((out.out()[:, 27:].view(torch.int16) == 0).all())
                got.append(out.out())
            assert torch.equal(got[0], got[1]), (S, fam, mean)


# ---- mq_resnet_attnpool_tokens / _attend ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", K.TOK_C)
@pytest.mark.parametrize("HW", K.TOK_HW)
def test_attnpool_tokens(lib, HW, C):
    """HW = 1 (the mean is the pixel), 3, 255 (T = AP_MAX_T); C = 2056 gives the 256-thread loop a second, ragged trip"""
    n = 3
    pos = torch.randn(HW + 1, C, generator=torch.Generator().manual_seed(HW + C)) / C ** 0.5
    pd = pos.to(DEV)
    for fam in K.FAMILIES_ROWS:
        x = K.make_rows_bf16(fam, n, HW, C, seed=7).reshape(n, HW, C)
        ref, bound = K.reference_tokens(x, pos)
        xd = x.to(DEV)
        tok = Window(n * (HW + 1), C, torch.bfloat16)
        L.check(lib.mq_resnet_attnpool_tokens(xd.data_ptr(), pd.data_ptr(), tok.ptr(), n, HW, C, _s()))
        assert tok.outside_intact()
        _hold("ap_tokens", fam, tok.out(), ref.reshape(-1, C), bound.reshape(-1, C), (HW, C))


@pytest.mark.parametrize("T", K.ATT_T)
def test_attnpool_attend_softmax_edges(lib, T):
    """T = 1, around the 64-lane stride, and AP_MAX_T; `peaked` puts the winning key at a position that depends on head and image, `offset` needs the
    max-subtraction, `one_loud_value` shows a single wrong key"""
    n = K.ATT_N
    for C in K.ATT_C:
        for fam in K.FAMILIES_ATTEND:
            q, kv = K.make_attend(fam, n, T, C, seed=6)
            ref, bound = K.reference_attend(q, kv)
            qd, kd = q.to(DEV), kv.to(DEV)
            out = Window(n, C, torch.bfloat16)
            L.check(lib.mq_resnet_attnpool_attend(qd.data_ptr(), kd.data_ptr(), out.ptr(), n, T, C, _s()))
            assert out.outside_intact()
            _hold("ap_attend", fam, out.out(), ref, bound, (T, C))


def test_attnpool_attend_refuses_too_many_keys_and_partial_heads(lib):
    q, kv = K.make_attend("randn", 1, 257, 192, seed=1)
    qd, kd = q.to(DEV), kv.to(DEV)
    out = Window(1, 192, torch.bfloat16)
    assert lib.mq_resnet_attnpool_attend(qd.data_ptr(), kd.data_ptr(), out.ptr(), 1, 257, 192, _s()) != L.MQ_OK and out.untouched()
    assert lib.mq_resnet_attnpool_attend(qd.data_ptr(), kd.data_ptr(), out.ptr(), 1, 256, 96, _s()) != L.MQ_OK and out.untouched()

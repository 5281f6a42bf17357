"""csrc/attention_gqa256.hip through the C ABI (mq_attention_gqa_band) against the float64 grouped-query band reference of tests/gemma_ref.py on the device.
The assertion is that of tests/test_attention_gpu.py, whose bar is imported:  |kernel - reference| <= 1.25 x budget,  budget = 2**-8 * (P|V| + |out|)
(attention_ref.budget, derived from the kernel's arithmetic; tests/test_gemma_host.py shows that the tile-order model of this kernel stays within 1.0 x on
these inputs and that the wrong K/V head, a band edge off by one key on either side, a skipped tile, a tile visited twice and a piece that is not
re-staged leave it by 50 x or more).

Inputs: `readout` (one-hot V rows, a different roll per K/V head: one wrong key or one wrong K/V head is one wrong column) and `peaked` (sharp softmax rows, V
over four decades).  Head shapes (q_heads, kv_heads) at head_dim 256: (3, 1) = the checkpoint's, (2, 2) = no K/V head shared, (4, 2) = the K/V head index
matters.  half_window 0 (every key), 1, 16, 64, 256.  Lengths (tests/test_gemma_host.py::gpu_cases): a single token; around one 16-query block; around the
64-key tile = the 64-query slice of the kernel; a packed mix; around the 128 keys of one LDS piece; one under, at and over hw and 2 hw + 1, where the
band first stops covering the sequence; 600 / 601 tokens at hw 64 and 256, where whole tiles fall outside a block's band and are skipped.

Every output buffer sits between 64 guard rows of a sentinel pattern, checked after every call.  The worst ratios are printed as `GQA256_RATIO` lines.
Measured on an MI355X: worst ratio 0.9708 over every case (bar 1.25); grouped against expanded K/V 0.0000 — the same bits — (bar 2.5)."""
import pytest
import torch

from marqo_amd import _lib as L
from tests import attention_ref as R
from tests import gemma_ref as G
from tests import qwen_ref as Q
from tests.test_attention_gpu import MARGIN
from tests.test_gemma_host import HEADS, gpu_cases

pytestmark = pytest.mark.gpu

GUARD = 64
HD = G.HD
SCALE = HD ** -0.5


@pytest.fixture(scope="module")
def lib():
    return L.load()


def _s():
    return torch.cuda.current_stream().cuda_stream


def _run(lib, qkv, lens, hs, hw, fixed=False, scale=SCALE):
    """mq_attention_gqa_band on a guarded output"""
    Qh, KV = hs
    W, rows = Qh * HD, qkv.shape[0]
    raw = torch.full(((rows + 2 * GUARD) * W,), 0x5A5A, dtype=torch.int16, device="cuda")
    out = raw[GUARD * W:(GUARD + rows) * W].view(torch.bfloat16).view(rows, W)
    if fixed:
        assert len(set(lens)) == 1
        cu, fl, mx = None, lens[0], 0
    else:
        cu, fl, mx = R.cu_seqlens(lens, "cuda"), 0, max(lens)
    L.check(lib.mq_attention_gqa_band(qkv.data_ptr(), out.data_ptr(), L.ptr(cu), len(lens), fl, mx, Qh, KV, HD, hw, scale, _s()), "mq_attention_gqa_band")
    torch.cuda.synchronize()
    n = GUARD * W
    assert bool((raw[:n] == 0x5A5A).all()) and bool((raw[n + rows * W:] == 0x5A5A).all()), "a guard row was written"
    return out


def _assert_parity(tag, lib, hs, hw, lens, fixed=False):
    for fam in ("readout", "peaked"):
        qkv = G.make_band_qkv(fam, lens, *hs, seed=sum(lens) + hs[0], device="cuda")
        got = _run(lib, qkv, lens, hs, hw, fixed)
        out, absout = G.band_gqa_reference(qkv, lens, *hs, HD, hw)
        w = R.worst_coords(got, out, absout, lens, hs[0], HD)
        print(f"GQA256_RATIO {tag} heads={hs} hw={hw} family={fam} lens={lens} ratio={w['ratio']:.4f}")
        assert w["ratio"] <= MARGIN, (tag, hs, hw, fam, lens, w)


@pytest.mark.parametrize("hs", HEADS)
def test_packed_batches_within_the_rounding_budget(lib, hs):
    cases = [c for c in gpu_cases() if c[0] == hs]
    assert cases
    for _, hw, lens in cases:
        _assert_parity("packed", lib, hs, hw, lens)


@pytest.mark.parametrize("hw", (0, 16))
def test_fixed_length_entry(lib, hw):
    _assert_parity("fixed", lib, (3, 1), hw, [70] * 3, fixed=True)


def test_the_scale_is_the_argument(lib):
    """query_pre_attn_scalar need not be the head width: scale 1 / 8 against the float64 reference at that scale"""
    hs, lens, hw = (3, 1), [129, 1, 33], 16
    qkv = G.make_band_qkv("readout", lens, *hs, seed=5, device="cuda")
    got = _run(lib, qkv, lens, hs, hw, scale=0.125)
    out, absout = G.band_gqa_reference(qkv, lens, *hs, HD, hw, scale=0.125)
    r = R.worst_ratio(got, out, absout)
    wrong = R.worst_ratio(got, *G.band_gqa_reference(qkv, lens, *hs, HD, hw))
    print(f"GQA256_RATIO scale=1/8: {r:.4f} (against the 1/16 reference: {wrong:.1f})")
    assert r <= MARGIN and wrong > 10 * MARGIN


@pytest.mark.parametrize("hs", HEADS)
def test_cross_checks_on_expanded_kv(lib, hs):
    """K/V copied to every query head of its group on the host (the kernel then runs with one query head per K/V head): without a band against
    qwen_ref.gqa_reference (float64, unmasked), with a band against band_gqa_reference of the expanded layout.  Kernel on the grouped layout and kernel
    on the expanded layout are each within the budget of the same reference, so they agree within twice the budget — the h / G mapping against the
    kernel's own one-to-one path"""
    Qh, KV = hs
    lens = [129, 1, 33, 200]
    for hw in (0, 16):
        for fam in ("readout", "peaked"):
            qkv = G.make_band_qkv(fam, lens, *hs, seed=77, device="cuda")
            got = _run(lib, qkv, lens, hs, hw)
            wide = Q.expand_kv(qkv, Qh, KV, HD)
            full = _run(lib, wide, lens, (Qh, Qh), hw)
            if hw == 0:
                out, absout = Q.gqa_reference(wide, lens, Qh, Qh, HD, R.MASK_NONE)
            else:
                out, absout = G.band_gqa_reference(wide, lens, Qh, Qh, HD, hw)
            r1, r2 = R.worst_ratio(got, out, absout), R.worst_ratio(full, out, absout)
            worst = R.worst_ratio(got, full.double(), absout + (out.abs() - full.double().abs()))     # |got - full| over the REFERENCE's budget
            print(f"GQA256_RATIO cross heads={hs} hw={hw} family={fam}: grouped {r1:.4f} expanded {r2:.4f} grouped-vs-expanded {worst:.4f} (bar {2 * MARGIN})")
            assert r1 <= MARGIN and r2 <= MARGIN and worst <= 2 * MARGIN


def test_bad_arguments_launch_nothing(lib):
    hs, lens = (4, 2), [20]
    qkv = G.make_band_qkv("randn", lens, *hs, seed=1, device="cuda")
    out = torch.full((20, 4 * HD), 7.0, dtype=torch.bfloat16, device="cuda")
    cu = R.cu_seqlens(lens, "cuda")
    for args, what in (((4, 2, 128, 0, SCALE), b"head_dim 128 unsupported"), ((6, 4, 256, 0, SCALE), b"q_heads 6 must be a multiple of kv_heads 4"),
                       ((4, 2, 256, -1, SCALE), b"half_window -1"), ((4, 2, 256, 0, 0.0), b"softmax scale")):
        assert lib.mq_attention_gqa_band(qkv.data_ptr(), out.data_ptr(), cu.data_ptr(), 1, 0, 20, *args, _s()) == -1 and what in lib.mq_last_error()
    assert lib.mq_attention_gqa_band(qkv.data_ptr(), out.data_ptr(), cu.data_ptr(), 1, 0, 8193, 4, 2, 256, 0, SCALE, _s()) == -1 and b"8193" in lib.mq_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())

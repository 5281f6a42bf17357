"""csrc/attention_window.hip through the C ABI (mq_attention_window) against the float64 windowed reference of tests/modernbert_ref.py on the device.
The assertion is that of tests/test_attention_gpu.py:  |kernel - reference| <= 1.25 x budget,  budget = 2**-8 * (P|V| + |out|) (attention_ref.budget, derived
from the kernel's arithmetic; tests/test_modernbert_host.py shows that the arithmetic model of the band kernel stays within 1.0 x on these inputs and that
a window off by one key on either side, an edge tile taken as interior, a skipped tile and a dropped halo leave it by one to four orders of magnitude).

Inputs: `readout` (one-hot V rows: the output holds the probabilities themselves, so one wrong key is one wrong column) and `peaked` (sharp softmax rows, V
over four decades).  Shapes: half-windows 64 / 8 / 1 on a packed batch whose lengths put the band's edges on and off the 64-key tile boundaries and the
sequence ends on and off the 64-query slice boundaries; 705 tokens (12 slices per head; with half-window 300 the band of a slice is wider than the 640 keys
the LDS holds and streams through it in two pieces); the fixed-length entry at T = 130; a window that covers every sequence, which must equal mq_attention.

Every output buffer sits between 64 guard rows of a sentinel pattern on either side, checked after every call.  The worst ratios are printed as
`WINDOW_RATIO` lines."""
import pytest
import torch

from marqo_amd import _lib as L
from tests import attention_ref as R
from tests import modernbert_ref as M

pytestmark = pytest.mark.gpu

MARGIN = 1.25
GUARD = 64
HEADS = 2
PACK = [1, 63, 64, 65, 128, 129, 193, 200]


@pytest.fixture(scope="module")
def lib():
    return L.load()


def _s():
    return torch.cuda.current_stream().cuda_stream


def _run(lib, qkv, lens, hw, heads=HEADS, window=True):
    """mq_attention_window (or mq_attention, unmasked) on a guarded output; equal lengths go through the fixed-length entry"""
    W = heads * 64
    rows = qkv.shape[0]
    raw = torch.full(((rows + 2 * GUARD) * W,), 0x5A5A, dtype=torch.int16, device="cuda")
    out = raw[GUARD * W:(GUARD + rows) * W].view(torch.bfloat16).view(rows, W)
    if len(set(lens)) == 1:
        cu, nseq, fixed, mx = None, len(lens), lens[0], lens[0]
    else:
        cu, nseq, fixed, mx = R.cu_seqlens(lens, "cuda"), len(lens), 0, max(lens)
    if window:
        L.check(lib.mq_attention_window(qkv.data_ptr(), out.data_ptr(), L.ptr(cu), nseq, fixed, mx, W, heads, hw, _s()), "mq_attention_window")
    else:
        L.check(lib.mq_attention(qkv.data_ptr(), out.data_ptr(), L.ptr(cu), nseq, fixed, mx, W, heads, R.MASK_NONE, _s()), "mq_attention")
    torch.cuda.synchronize()
    n = GUARD * W
    assert bool((raw[:n] == 0x5A5A).all()) and bool((raw[n + rows * W:] == 0x5A5A).all()), "a guard row was written"
    return out


def _assert_parity(tag, fam, got, qkv, lens, hw, heads=HEADS):
    out, absout = M.window_reference(qkv, lens, heads, hw)
    w = R.worst_coords(got, out, absout, lens, heads, 64)
    print(f"WINDOW_RATIO {tag} family={fam} hw={hw} lens={lens} ratio={w['ratio']:.4f}")
    assert w["ratio"] <= MARGIN, (tag, fam, hw, w)


@pytest.mark.parametrize("fam", ("readout", "peaked"))
@pytest.mark.parametrize("hw", (64, 8, 1))
def test_packed_batch_within_the_rounding_budget(lib, hw, fam):
    qkv = R.make_qkv(fam, PACK, HEADS, 64, seed=hw + 1, device="cuda")
    _assert_parity("packed", fam, _run(lib, qkv, PACK, hw), qkv, PACK, hw)


@pytest.mark.parametrize("fam", ("readout", "peaked"))
@pytest.mark.parametrize("hw", (64, 300, 0))
def test_a_sequence_longer_than_the_lds_holds(lib, hw, fam):
    """705 tokens: 12 slices per head, each with its halo; hw = 300: 11 tiles per slice, two pieces through the LDS; hw = 0: every query sees itself alone"""
    lens = [705]
    qkv = R.make_qkv(fam, lens, HEADS, 64, seed=hw + 2, device="cuda")
    _assert_parity("long", fam, _run(lib, qkv, lens, hw), qkv, lens, hw)


@pytest.mark.parametrize("hw", (64, 8))
def test_fixed_length_entry(lib, hw):
    lens = [130] * 3
    for fam in ("readout", "peaked"):
        qkv = R.make_qkv(fam, lens, HEADS, 64, seed=hw + 3, device="cuda")
        _assert_parity("fixed", fam, _run(lib, qkv, lens, hw), qkv, lens, hw)


@pytest.mark.parametrize("lens,hw", ((PACK, 199), (PACK, 4096), ([130] * 2, 129)))
def test_a_window_over_the_whole_sequence_is_mq_attention(lib, lens, hw):
    for fam in ("readout", "peaked"):
        qkv = R.make_qkv(fam, lens, HEADS, 64, seed=hw + 4, device="cuda")
        got = _run(lib, qkv, lens, hw)
        out, absout, _ = R.reference(qkv, lens, HEADS, 64, R.MASK_NONE)
        r = R.worst_ratio(got, out, absout)
        full = _run(lib, qkv, lens, 0, window=False)
        print(f"WINDOW_RATIO whole family={fam} hw={hw} lens={lens} ratio={r:.4f} against mq_attention: {R.worst_ratio(got, full.double(), absout):.4f}")
        assert r <= MARGIN and R.worst_ratio(got, full.double(), absout) <= MARGIN


_GROWING = r"""
import torch
from marqo_amd import _lib as L
from tests import attention_ref as R
from tests import modernbert_ref as M
lib = L.load()
lens, heads = [705], 2
for hw in (100, 160, 300):      # 5, 7 and 10 tiles of LDS: 80 KiB, 112 KiB, 160 KiB — each call asks for more than the one before
    qkv = R.make_qkv("readout", lens, heads, 64, seed=hw, device="cuda")
    out = torch.zeros(705, heads * 64, dtype=torch.bfloat16, device="cuda")
    L.check(lib.mq_attention_window(qkv.data_ptr(), out.data_ptr(), R.cu_seqlens(lens, "cuda").data_ptr(), 1, 0, 705, heads * 64, heads, hw,
                                    torch.cuda.current_stream().cuda_stream), "mq_attention_window")
    torch.cuda.synchronize()
    ref, absout = M.window_reference(qkv, lens, heads, hw)
    print(f"WINDOW_RATIO growing hw={hw} ratio={R.worst_ratio(out, ref, absout):.4f}")
"""


def test_lds_request_that_grows_from_call_to_call():
    """The kernel's dynamic-LDS limit is raised once per process and device, and the LDS a call asks for depends on its window: in a process of its own
    (what an earlier test of this file has opted into must not help), a call above 64 KiB is followed by calls that ask for more.  Each must launch and
    stay inside the budget."""
    import os
    import re
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = subprocess.run([sys.executable, "-c", _GROWING], cwd=root, capture_output=True, text=True, timeout=120)
    print(res.stdout)
    assert res.returncode == 0, res.stderr[-2000:]
    ratios = [float(r) for r in re.findall(r"WINDOW_RATIO growing hw=\d+ ratio=([0-9.]+)", res.stdout)]
    assert len(ratios) == 3 and max(ratios) <= MARGIN, res.stdout


def test_one_key_short_of_the_whole_sequence_runs_the_band_kernel(lib):
    """hw = T - 2: the band kernel itself at its widest (only the two corner pairs (0, T-1), (T-1, 0) are outside), 12 heads"""
    lens, hw = [200], 198
    qkv = R.make_qkv("readout", lens, 12, 64, seed=9, device="cuda")
    _assert_parity("widest", "readout", _run(lib, qkv, lens, hw, heads=12), qkv, lens, hw, heads=12)

"""csrc/attention_gqa.hip through the C ABI (mq_attention_gqa) against the float64 grouped-query reference of tests/qwen_ref.py on the device.  The
assertion is that of tests/test_attention_gpu.py, whose bar is imported:  |kernel - reference| <= 1.25 x budget,  budget = 2**-8 * (P|V| + |out|)
(attention_ref.budget, derived from the kernel's arithmetic; tests/test_qwen_host.py shows that the tile-order model of this kernel stays within 1.0 x on
these inputs and that the wrong K/V head, a causal edge off by one key, a skipped or unstaged tile and a key counted twice leave it by 50 x or more).

Inputs: `readout` (one-hot V rows, a different roll per K/V head: one wrong key or one wrong K/V head is one wrong column) and `peaked` (sharp softmax rows, V
over four decades).  Head shapes (q_heads, kv_heads, head_dim): (4, 4, 64) = one query head per K/V head, (4, 2, 128), (8, 1, 64), (14, 2, 64) = a group
of seven (Qwen2-0.5B), (16, 8, 128) (Qwen3-Embedding-0.6B).  Lengths: a single token; around one 16-query block and one 64-key tile; a packed mix; around the
128-query slice boundary of the kernel (127, 128, 129); one key under and one over what the LDS holds (319 / 321 at head_dim 128, 639 / 641 at 64: above
it a slice's keys go through the LDS in two pieces).  Causal on every shape, unmasked on a subset.

Every output buffer sits between 64 guard rows of a sentinel pattern, checked after every call.  The worst ratios are printed as `GQA_RATIO` lines.
Measured on an MI355X: worst ratio 0.9927 over every case (bar 1.25); against mq_attention on expanded K/V 0.0000 — the two kernels give the same bits —
(bar 2.5)."""
import pytest
import torch

from marqo_amd import _lib as L
from tests import attention_ref as R
from tests import qwen_ref as Q
from tests.test_attention_gpu import MARGIN

pytestmark = pytest.mark.gpu

GUARD = 64
HEADS = [(4, 4, 64), (4, 2, 128), (8, 1, 64), (14, 2, 64), (16, 8, 128)]
PACKS = [[1], [15, 16, 17], [63, 64, 65], [129, 1, 33], [Q.SLICE - 1, Q.SLICE, Q.SLICE + 1]]
UNMASKED = [[15, 16, 17], [129, 1, 33], [Q.SLICE - 1, Q.SLICE, Q.SLICE + 1]]


@pytest.fixture(scope="module")
def lib():
    return L.load()


def _s():
    return torch.cuda.current_stream().cuda_stream


def _run(lib, qkv, lens, hs, mask, fixed=False):
    """mq_attention_gqa on a guarded output"""
    Qh, KV, hd = hs
    W, rows = Qh * hd, qkv.shape[0]
    raw = torch.full(((rows + 2 * GUARD) * W,), 0x5A5A, dtype=torch.int16, device="cuda")
    out = raw[GUARD * W:(GUARD + rows) * W].view(torch.bfloat16).view(rows, W)
    if fixed:
        assert len(set(lens)) == 1
        cu, fl, mx = None, lens[0], 0
    else:
        cu, fl, mx = R.cu_seqlens(lens, "cuda"), 0, max(lens)
    L.check(lib.mq_attention_gqa(qkv.data_ptr(), out.data_ptr(), L.ptr(cu), len(lens), fl, mx, Qh, KV, hd, mask, _s()), "mq_attention_gqa")
    torch.cuda.synchronize()
    n = GUARD * W
    assert bool((raw[:n] == 0x5A5A).all()) and bool((raw[n + rows * W:] == 0x5A5A).all()), "a guard row was written"
    return out


def _assert_parity(tag, lib, hs, lens, mask, fixed=False):
    for fam in ("readout", "peaked"):
        qkv = Q.make_gqa_qkv(fam, lens, *hs, seed=sum(lens) + hs[0], device="cuda")
        got = _run(lib, qkv, lens, hs, mask, fixed)
        out, absout = Q.gqa_reference(qkv, lens, *hs, mask)
        w = R.worst_coords(got, out, absout, lens, hs[0], hs[2])
        print(f"GQA_RATIO {tag} heads={hs} mask={mask} family={fam} lens={lens} ratio={w['ratio']:.4f}")
        assert w["ratio"] <= MARGIN, (tag, hs, mask, fam, lens, w)


@pytest.mark.parametrize("hs", HEADS)
def test_causal_packed_batches_within_the_rounding_budget(lib, hs):
    for lens in PACKS:
        _assert_parity("causal", lib, hs, lens, R.MASK_CAUSAL)


@pytest.mark.parametrize("hs", HEADS)
def test_unmasked_packed_batches_within_the_rounding_budget(lib, hs):
    for lens in UNMASKED:
        _assert_parity("unmasked", lib, hs, lens, R.MASK_NONE)


@pytest.mark.parametrize("hs", HEADS)
@pytest.mark.parametrize("mask", (R.MASK_CAUSAL, R.MASK_NONE))
def test_one_key_under_and_over_what_the_lds_holds(lib, hs, mask):
    cap = Q.LDS_KEYS[hs[2]]
    for lens in ([cap - 1], [cap + 1], [cap + 1, 70]):
        _assert_parity("lds", lib, hs, lens, mask)


@pytest.mark.parametrize("hs", ((4, 2, 128), (14, 2, 64)))
def test_fixed_length_entry(lib, hs):
    for mask in (R.MASK_CAUSAL, R.MASK_NONE):
        _assert_parity("fixed", lib, hs, [33] * 3, mask, fixed=True)


@pytest.mark.parametrize("hs", HEADS)
def test_agrees_with_mq_attention_on_expanded_kv(lib, hs):
    """K/V copied to every query head of its group on the host: mq_attention(MQ_MASK_CAUSAL) on the [rows, 3 W] layout and mq_attention_gqa are each within
    the budget of the same float64 reference, so they agree within twice the budget — the layout and the h / G mapping against the project's own kernel"""
    Qh, KV, hd = hs
    lens = [129, 1, 33, Q.LDS_KEYS[hd] + 1]
    for fam in ("readout", "peaked"):
        qkv = Q.make_gqa_qkv(fam, lens, *hs, seed=77, device="cuda")
        got = _run(lib, qkv, lens, hs, R.MASK_CAUSAL)
        wide = Q.expand_kv(qkv, *hs)
        full = torch.zeros(sum(lens), Qh * hd, dtype=torch.bfloat16, device="cuda")
        L.check(lib.mq_attention(wide.data_ptr(), full.data_ptr(), R.cu_seqlens(lens, "cuda").data_ptr(), len(lens), 0, max(lens), Qh * hd, Qh, R.MASK_CAUSAL, _s()),
                "mq_attention")
        torch.cuda.synchronize()
        out, absout = Q.gqa_reference(qkv, lens, *hs, R.MASK_CAUSAL)
        worst = R.worst_ratio(got, full.double(), absout + (out.abs() - full.double().abs()))      # |got - full| over the REFERENCE's budget u (P|V| + |out|)
        print(f"GQA_RATIO cross heads={hs} family={fam} against mq_attention: {worst:.4f} (bar {2 * MARGIN})")
        assert worst <= 2 * MARGIN


def test_bad_arguments_launch_nothing(lib):
    hs, lens = (4, 2, 64), [20]
    qkv = Q.make_gqa_qkv("randn", lens, *hs, seed=1, device="cuda")
    out = torch.full((20, 256), 7.0, dtype=torch.bfloat16, device="cuda")
    cu = R.cu_seqlens(lens, "cuda")
    for args, what in (((4, 2, 96, 1), b"head_dim 96"), ((6, 4, 64, 1), b"q_heads 6 must be a multiple of kv_heads 4"), ((4, 2, 64, L.MQ_MASK_CAUSAL_CLS), b"mask 2 unsupported")):
        assert lib.mq_attention_gqa(qkv.data_ptr(), out.data_ptr(), cu.data_ptr(), 1, 0, 20, *args, _s()) == -1 and what in lib.mq_last_error()
    assert lib.mq_attention_gqa(qkv.data_ptr(), out.data_ptr(), cu.data_ptr(), 1, 0, 8193, 4, 2, 64, 1, _s()) == -1 and b"8193" in lib.mq_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


_GROWING = r"""
import torch
from marqo_amd import _lib as L
from tests import attention_ref as R
from tests import qwen_ref as Q
lib = L.load()
for hs in ((4, 2, 128), (8, 1, 64)):
    for ln in (100, 200, Q.LDS_KEYS[hs[2]] + 1):      # hd 128: 64 KiB (no opt-in), 128 KiB, 160 KiB; hd 64: 32 KiB, 64 KiB, 160 KiB — each call asks for more
        qkv = Q.make_gqa_qkv("readout", [ln], *hs, seed=ln, device="cuda")
        out = torch.zeros(ln, hs[0] * hs[2], dtype=torch.bfloat16, device="cuda")
        L.check(lib.mq_attention_gqa(qkv.data_ptr(), out.data_ptr(), R.cu_seqlens([ln], "cuda").data_ptr(), 1, 0, ln, *hs, 1, torch.cuda.current_stream().cuda_stream),
                "mq_attention_gqa")
        torch.cuda.synchronize()
        ref, absout = Q.gqa_reference(qkv, [ln], *hs, 1)
        print(f"GQA_RATIO growing hd={hs[2]} len={ln} ratio={R.worst_ratio(out, ref, absout):.4f}")
"""


def test_lds_request_that_grows_from_call_to_call():
    """The kernel's dynamic-LDS limit is raised once per process, device and instantiation, and the LDS a call asks for depends on its longest sequence: in a
    process of its own (what an earlier test of this file has opted into must not help), a small request is followed by larger ones.  Each must launch
    and stay inside the budget."""
    import os
    import re
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = subprocess.run([sys.executable, "-c", _GROWING], cwd=root, capture_output=True, text=True, timeout=120)
    print(res.stdout)
    assert res.returncode == 0, res.stderr[-2000:]
    ratios = [float(r) for r in re.findall(r"GQA_RATIO growing hd=\d+ len=\d+ ratio=([0-9.]+)", res.stdout)]
    assert len(ratios) == 6 and max(ratios) <= MARGIN, res.stdout

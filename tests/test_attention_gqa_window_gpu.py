"""mq_attention_gqa_window (csrc/attention_gqa.hip) through the C ABI against the float64 causal sliding-window reference of tests/llama_ref.py on the
device.  The assertion is that of tests/test_attention_gqa_gpu.py, whose bar is imported:  |kernel - reference| <= 1.25 x budget,
budget = 2**-8 * (P|V| + |out|)  (attention_ref.budget).  Query i sees the keys j with i - window < j <= i (transformers' masking_utils).

Cases: head_dim 64 and 128; (q_heads, kv_heads) (4, 2), (7, 1) = a group of seven, (2, 2) = no grouping, (8, 1) = a group that fills a round of waves; one packed call of lengths 1, 17, 129, 300 and
one fixed-length call; windows 1, 16 (the lower edge inside a 16-query block), 63 / 64 / 65 (on and on either side of a 64-key tile boundary), 128 (a
slice boundary) and 200; and one length past twice what the LDS holds with a window of more than the LDS holds, so that a slice's band goes through the
LDS in two pieces.  Inputs: `readout` (one-hot V rows: one wrong key is one wrong column) and `peaked`.

One-wrong-key checks in the kernel's own output: a change of K or V at key i - window (just outside the band) and at key i + 1 leaves row i bit for bit,
a change at key i - window + 1 (the band's first key) does not — at queries on both sides of a slice boundary.  A window of at least the sequence gives
the bits of mq_attention_gqa under MQ_MASK_CAUSAL.  Every output sits between guard rows; the input is compared with its copy after every call.
The worst ratios are printed as `GQAW_RATIO` lines."""
import pytest
import torch

from marqo_amd import _lib as L
from tests import attention_ref as R
from tests import llama_ref as LR
from tests import qwen_ref as Q
from tests.test_attention_gpu import MARGIN

pytestmark = pytest.mark.gpu

GUARD = 64
HEADS = [(4, 2), (7, 1), (2, 2), (8, 1)]
WINDOWS = (1, 16, 63, 64, 65, 128, 200)
PACK = [1, 17, 129, 300]


@pytest.fixture(scope="module")
def lib():
    return L.load()


def _s():
    return torch.cuda.current_stream().cuda_stream


def _run(lib, qkv, lens, hs, window, fixed=False):
    """mq_attention_gqa_window on a guarded output; the input must come back as it went in (V included)"""
    Qh, KV, hd = hs
    W, rows = Qh * hd, qkv.shape[0]
    raw = torch.full(((rows + 2 * GUARD) * W,), 0x5A5A, dtype=torch.int16, device="cuda")
    out = raw[GUARD * W:(GUARD + rows) * W].view(torch.bfloat16).view(rows, W)
    before = qkv.clone()
    if fixed:
        assert len(set(lens)) == 1
        cu, fl, mx = None, lens[0], 0
    else:
        cu, fl, mx = R.cu_seqlens(lens, "cuda"), 0, max(lens)
    L.check(lib.mq_attention_gqa_window(qkv.data_ptr(), out.data_ptr(), L.ptr(cu), len(lens), fl, mx, Qh, KV, hd, window, _s()), "mq_attention_gqa_window")
    torch.cuda.synchronize()
    n = GUARD * W
    assert bool((raw[:n] == 0x5A5A).all()) and bool((raw[n + rows * W:] == 0x5A5A).all()), "a guard row was written"
    assert torch.equal(qkv.view(torch.int16), before.view(torch.int16)), "the input (q, k or v) was written"
    return out


def _assert_parity(tag, lib, hs, lens, window, fixed=False):
    worst = 0.0
    for fam in ("readout", "peaked"):
        qkv = Q.make_gqa_qkv(fam, lens, *hs, seed=sum(lens) + hs[0] + window, device="cuda")
        got = _run(lib, qkv, lens, hs, window, fixed)
        out, absout = LR.gqa_window_reference(qkv, lens, *hs, window)
        w = R.worst_coords(got, out, absout, lens, hs[0], hs[2])
        print(f"GQAW_RATIO {tag} heads={hs} window={window} family={fam} lens={lens} ratio={w['ratio']:.4f}")
        assert w["ratio"] <= MARGIN, (tag, hs, window, fam, lens, w)
        worst = max(worst, w["ratio"])
    return worst


@pytest.mark.parametrize("hd", (64, 128))
@pytest.mark.parametrize("qkv_heads", HEADS)
def test_windows_within_the_rounding_budget(lib, hd, qkv_heads):
    hs = (*qkv_heads, hd)
    worst = max(_assert_parity("packed", lib, hs, PACK, w) for w in WINDOWS)
    print(f"GQAW_RATIO worst heads={hs}: {worst:.4f} (bar {MARGIN})")


@pytest.mark.parametrize("hd", (64, 128))
def test_fixed_length_entry(lib, hd):
    for w in (16, 65):
        _assert_parity("fixed", lib, (4, 2, hd), [70] * 3, w, fixed=True)


@pytest.mark.parametrize("hd", (64, 128))
def test_a_band_that_goes_through_the_lds_in_two_pieces(lib, hd):
    cap = LR.LDS_KEYS[hd]          # the kernel's kpad cap: 320 keys at head_dim 128, 640 at 64
    _assert_parity("pieces", lib, (4, 2, hd), [2 * cap + 60, 70], cap + 80)


@pytest.mark.parametrize("hd", (64, 128))
@pytest.mark.parametrize("i", (LR.SLICE - 1, LR.SLICE, 299))
def test_one_wrong_key_on_either_edge_of_the_band(lib, hd, i):
    hs, lens, window = (4, 2, hd), [33, 300], 100
    Qh, KV, _ = hs
    qkv = Q.make_gqa_qkv("randn", lens, *hs, seed=i, device="cuda")
    base = _run(lib, qkv, lens, hs, window).clone()
    row = lens[0] + i
    kcols, vcols = slice(Qh * hd, (Qh + KV) * hd), slice((Qh + KV) * hd, (Qh + 2 * KV) * hd)
    for j, seen in ((i - window, False), (i - window + 1, True), (i, True), (i + 1, False)):
        if j >= lens[1]:
            continue
        for cols, what in ((kcols, "K"), (vcols, "V")):
            other = qkv.clone()
            other[lens[0] + j, cols] = (-other[lens[0] + j, cols].float() + 3.0).to(torch.bfloat16)
            got = _run(lib, other, lens, hs, window)
            same = torch.equal(got[row].view(torch.int16), base[row].view(torch.int16))
            assert same != seen, f"query {i}, {what} of key {j} changed: row {'kept' if same else 'changed'} its bits, the key is {'inside' if seen else 'outside'} the band"
            assert torch.equal(got[:lens[0]].view(torch.int16), base[:lens[0]].view(torch.int16)), "another sequence changed"


@pytest.mark.parametrize("hd", (64, 128))
def test_a_window_of_the_whole_sequence_gives_the_causal_kernels_bits(lib, hd):
    cap = LR.LDS_KEYS[hd]
    for qkv_heads in HEADS:
        hs = (*qkv_heads, hd)
        for lens in (PACK, [cap + 70, 129]):
            qkv = Q.make_gqa_qkv("peaked", lens, *hs, seed=9, device="cuda")
            causal = torch.zeros(sum(lens), hs[0] * hd, dtype=torch.bfloat16, device="cuda")
            L.check(lib.mq_attention_gqa(qkv.data_ptr(), causal.data_ptr(), R.cu_seqlens(lens, "cuda").data_ptr(), len(lens), 0, max(lens), *hs, R.MASK_CAUSAL, _s()),
                    "mq_attention_gqa")
            for window in (max(lens), max(lens) + 1, 8192, 2 ** 31 - 1):
                assert torch.equal(_run(lib, qkv, lens, hs, window).view(torch.int16), causal.view(torch.int16)), (hs, lens, window)
            # ... and half of it is another result (the comparison can see a window that binds)
            assert not torch.equal(_run(lib, qkv, lens, hs, max(lens) // 2).view(torch.int16), causal.view(torch.int16))


def test_torch_op_gives_the_c_abis_bits(lib):
    hs, lens = (4, 2, 64), [17, 129]
    qkv = Q.make_gqa_qkv("randn", lens, *hs, seed=4, device="cuda")
    out = torch.zeros(sum(lens), 256, dtype=torch.bfloat16, device="cuda")
    L.load_torch_ops().mq_attention_gqa_window(qkv, R.cu_seqlens(lens, "cuda"), max(lens), *hs, 40, out)
    assert torch.equal(out.view(torch.int16), _run(lib, qkv, lens, hs, 40).view(torch.int16))


def test_bad_arguments_launch_nothing(lib):
    hs, lens = (4, 2, 64), [20]
    qkv = Q.make_gqa_qkv("randn", lens, *hs, seed=1, device="cuda")
    out = torch.full((20, 256), 7.0, dtype=torch.bfloat16, device="cuda")
    cu = R.cu_seqlens(lens, "cuda")
    for args, what in (((4, 2, 96, 4), b"head_dim 96"), ((6, 4, 64, 4), b"q_heads 6 must be a multiple of kv_heads 4"), ((4, 2, 64, 0), b"window 0")):
        assert lib.mq_attention_gqa_window(qkv.data_ptr(), out.data_ptr(), cu.data_ptr(), 1, 0, 20, *args, _s()) == -1 and what in lib.mq_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())

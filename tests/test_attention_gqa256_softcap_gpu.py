"""mq_attention_gqa256_softcap (csrc/attention_gqa256_softcap.hip) against float64 on the device — cap, windowed causal mask, softmax — under
tests/test_attention_gpu.py's assertion and bar:  |kernel - reference| <= MARGIN x attention_ref.budget.  The cap adds only fp32 error (the kernel's header:
at most 2**-21 cap in the score), so it has no allowance.  Heads (16, 1) takes two rounds; lengths sit around the 16-query block, the 64-key tile and
the wrap of the two-buffer ring (128, 193); 300 keys at window 64 leave whole tiles below a block's band.  Every output lies between 64 guard rows.
Measured on an MI355X: GQA256SC_RATIO worst 0.9922 over every parity case; saturated rows 0.47 (-cap) / 0.50 (+cap) at 1000 keys, 0.79 at 8192 keys and
cap 64; cap 4 against the uncapped reference 310 x (readout) / 216 127 x (peaked), window 16 against window 17 128 x / 317 x (bar 12.5)."""
import pytest
import torch

from marqo_amd import _lib as L
from tests import attention_ref as R
from tests import gemma_ref as G
from tests import qwen_ref as Q
from tests.test_attention_gpu import MARGIN

pytestmark = pytest.mark.gpu

GUARD, HD, SCALE, STREAM = 64, 256, 256 ** -0.5, lambda: torch.cuda.current_stream().cuda_stream
LENS = ([1], [15], [16], [17], [63], [64], [65], [127], [128], [129], [193], [129, 1, 33, 200])


def reference(qkv, lens, Qh, KV, cap, window):
    # float64 on the device of qkv -> (out, absout) = (P V, P |V|); cap 0: no cap; window 0: plain causal
    out = torch.zeros(qkv.shape[0], Qh * HD, dtype=torch.float64, device=qkv.device)
    absout, r0 = torch.zeros_like(out), 0
    kvh = torch.arange(Qh, device=qkv.device) // (Qh // KV)
    for ln in lens:
        q, k, v = Q.split_qkv(qkv[r0:r0 + ln].double(), Qh, KV, HD)
        s = q @ k[kvh].transpose(1, 2) * SCALE
        s = cap * torch.tanh(s / cap) if cap > 0 else s
        i = torch.arange(ln, device=qkv.device)
        ok = (i[None, :] <= i[:, None]) & ((i[None, :] > i[:, None] - window) if window > 0 else True)
        p = torch.softmax(s.masked_fill(~ok, float("-inf")), dim=-1)
        out[r0:r0 + ln] = (p @ v[kvh]).transpose(0, 1).reshape(ln, Qh * HD)
        absout[r0:r0 + ln] = (p @ v[kvh].abs()).transpose(0, 1).reshape(ln, Qh * HD)
        r0 += ln
    return out, absout


def run(qkv, lens, hs, cap, window, fixed=False):
    W, rows = hs[0] * HD, qkv.shape[0]
    raw = torch.full(((rows + 2 * GUARD) * W,), 0x5A5A, dtype=torch.int16, device="cuda")
    out = raw[GUARD * W:(GUARD + rows) * W].view(torch.bfloat16).view(rows, W)
    cu, fl, mx = (None, lens[0], 0) if fixed else (R.cu_seqlens(lens, "cuda"), 0, max(lens))
    L.check(L.load().mq_attention_gqa256_softcap(qkv.data_ptr(), out.data_ptr(), L.ptr(cu), len(lens), fl, mx, *hs, HD, window, cap, SCALE, STREAM()), "softcap")
    torch.cuda.synchronize()
    assert bool((raw[:GUARD * W] == 0x5A5A).all()) and bool((raw[(GUARD + rows) * W:] == 0x5A5A).all()), "a guard row was written"
    return out


def parity(hs, cap, window, lens, fixed=False):
    worst = 0.0
    for fam in ("readout", "peaked"):
        qkv = G.make_band_qkv(fam, lens, *hs, seed=sum(lens) + hs[0], device="cuda")
        w = R.worst_coords(run(qkv, lens, hs, cap, window, fixed), *reference(qkv, lens, *hs, cap, window), lens, hs[0], HD)
        assert w["ratio"] <= MARGIN, (hs, cap, window, fam, lens, w)
        worst = max(worst, w["ratio"])
    return worst


@pytest.mark.parametrize("hs", ((2, 1), (4, 2), (2, 2), (8, 1), (16, 1)))
@pytest.mark.parametrize("cap", (50.0, 4.0))
def test_within_the_rounding_budget(hs, cap):
    worst = max(*(parity(hs, cap, window, lens) for lens in LENS for window in (0, 1, 16, 64, 100)), parity(hs, cap, 64, [300]), parity(hs, cap, 16, [70] * 3, fixed=True))
    print(f"GQA256SC_RATIO heads={hs} cap={cap}: worst ratio {worst:.4f} (bar {MARGIN})")


def test_the_cap_and_the_window_are_applied():
    hs, lens = (4, 2), [129, 1, 33, 200]
    for fam in ("readout", "peaked"):
        qkv = G.make_band_qkv(fam, lens, *hs, seed=7, device="cuda")
        nocap = R.worst_ratio(run(qkv, lens, hs, 4.0, 0), *reference(qkv, lens, *hs, 0.0, 0))
        w17 = R.worst_ratio(run(qkv, lens, hs, 4.0, 16), *reference(qkv, lens, *hs, 4.0, 17))
        print(f"GQA256SC_RATIO family={fam}: cap 4 against no cap {nocap:.1f}, window 16 against window 17 {w17:.1f} (both must exceed {10 * MARGIN})")
        assert nocap > 10 * MARGIN and w17 > 10 * MARGIN


@pytest.mark.parametrize("ln,cap,sign", ((1000, 50.0, -1.0), (1000, 50.0, 1.0), (8192, 64.0, 1.0)))
def test_saturated_rows_stay_finite(ln, cap, sign):
    """q and k constant vectors, scaled score +-256: every score at -cap or at +cap; 8192 keys at cap 64 is the edge of the kernel's range bound"""
    q, k = torch.zeros(ln, HD), torch.zeros(ln, HD)
    q[:, :64], k[:, :64] = 8.0, sign * 8.0
    qkv = torch.cat([q, k, torch.randn(ln, HD, generator=torch.Generator().manual_seed(1))], 1).to(torch.bfloat16).cuda()
    got = run(qkv, [ln], (1, 1), cap, 0)
    r = R.worst_ratio(got, *reference(qkv, [ln], 1, 1, cap, 0))
    print(f"GQA256SC_RATIO saturated len={ln} cap={cap} sign={sign:+.0f}: {r:.4f}")
    assert bool(torch.isfinite(got.float()).all()) and r <= MARGIN


def test_bad_arguments_launch_nothing():
    lib = L.load()
    qkv = G.make_band_qkv("randn", [20], 4, 2, seed=1, device="cuda")
    out, cu = torch.full((20, 4 * HD), 7.0, dtype=torch.bfloat16, device="cuda"), R.cu_seqlens([20], "cuda")
    for (hd, win, cap, mx), what in (((128, 0, 50.0, 20), b"head_dim 128 unsupported"), ((256, 0, 0.0, 20), b"softcap 0 unsupported"),
                                     ((256, 0, 65.0, 20), b"softcap 65 unsupported"), ((256, -1, 50.0, 20), b"window -1"),
                                     ((256, 0, 50.0, 8193), b"max sequence length 8193 unsupported")):
        assert lib.mq_attention_gqa256_softcap(qkv.data_ptr(), out.data_ptr(), cu.data_ptr(), 1, 0, mx, 4, 2, hd, win, cap, SCALE, STREAM()) == -1
        assert what in lib.mq_last_error(), lib.mq_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())

"""csrc/attention_full.hip through the C ABI (mq_attention_full) against the float64 attention of tests/attention_ref.py (reference, MASK_NONE), on the
device.  The assertion is elementwise, tests/test_attention_gpu.py's:  |kernel - reference| <= 1.25 x budget, budget = 2**-8 (P|V| + |out|)
(attention_ref.budget, derived from the bf16-P / fp32-normaliser arithmetic this kernel shares with mq_attention; the 1.25 is that file's allowance for the
fp32 terms the derivation neglects, the bar of tests/test_attention_alibi_gpu.py — not a fitted number).  The scale passed is 1 / sqrt(64), the
reference's.

Shapes (head width 64, the only one the kernel takes), 1 and 3 heads:
  the packed lengths 1, 15, 16, 17, 63, 64, 65, 128, 129, 640, 641, 1300 in ONE call — 640 / 641: the edge of the resident LDS image (one piece / two);
  1300: two re-stagings and a ragged last piece (640 + 640 + 20 keys) — over the families randn, peaked, readout, ramp_up, ramp_down;
  one fixed-length call, fixed_len 65 x 3.

One wrong key (the construction of tests/test_attention_gpu.py's class-row test: a value column only one position can produce).  In a pack
[65, L, 129] the marker keys of the middle sequence — its first key, its last key, the keys on either side of every 64-key tile edge (63 | 64, 127 | 128,
...; 639 | 640 is the LDS image's edge among them) — each own one value column: V[key, col] = 1 for that key alone, 0 for every other key of every
sequence.  Output column col of a query of that sequence is then the probability of that one key: it must be positive and within the budget, which
for this column is 2 * 2**-8 of the probability itself — a dropped, duplicated or shifted key is off by 128 x the budget (asserted on the reference:
zeroing the column leaves the bar by that much).  The neighbouring sequences carry no marker: their marker columns must be EXACTLY 0.0, so a read
across cu_seqlens in either direction shows; and the marked sequence's rows must not depend on its neighbours, bit for bit.  L = 1300 and L = 641.

Argument refusals (error code + mq_last_error, no launch, output untouched) are checked here on the device and in tests/test_nomic_bert_host.py
without one.  Every output buffer sits between 64 guard rows of a sentinel pattern, checked after every call.

Measured on an MI355X (FULL_RATIO lines), worst |kernel - reference| / budget:
    randn / peaked / readout / ramp_up / ramp_down, the packed lengths: 0.53 / 0.85 / 0.94 / 0.46 / 0.46    fixed_len 65 (randn / readout): 0.45 / 0.93
    markers: 0.94 (1300), 0.92 (641).  Nothing exceeds 1.0: the 1.25 allowance is unused."""
import pytest
import torch

from marqo_amd import _lib as L
from tests import attention_ref as R
from tests.test_attention_gpu import GUARD, MARGIN, Guarded      # noqa: F401

pytestmark = pytest.mark.gpu

HD = 64
SCALE = 64 ** -0.5
LENS = [1, 15, 16, 17, 63, 64, 65, 128, 129, 640, 641, 1300]
FAMILIES = ("randn", "peaked", "readout", "ramp_up", "ramp_down")


@pytest.fixture(scope="module")
def lib():
    return L.load()


def _s():
    return torch.cuda.current_stream().cuda_stream


def _run(lib, qkv, lens, heads, fixed=False):
    """one call on a guarded output -> bf16 [rows, heads hd]"""
    g = Guarded(qkv.shape[0], heads * HD)
    if fixed:
        assert len(set(lens)) == 1
        rc = lib.mq_attention_full(qkv.data_ptr(), g.ptr(), None, len(lens), lens[0], 0, heads, HD, SCALE, _s())
    else:
        cu = R.cu_seqlens(lens, "cuda")
        rc = lib.mq_attention_full(qkv.data_ptr(), g.ptr(), cu.data_ptr(), len(lens), 0, max(lens), heads, HD, SCALE, _s())
    L.check(rc, "mq_attention_full")
    torch.cuda.synchronize()
    assert g.guards_intact()
    return g.out


def _check(lib, tag, fam, lens, heads, seed, fixed=False):
    qkv = R.make_qkv(fam, lens, heads, HD, seed=seed, device="cuda")
    got = _run(lib, qkv, lens, heads, fixed)
    out, absout, _ = R.reference(qkv, lens, heads, HD, R.MASK_NONE)
    w = R.worst_coords(got, out, absout, lens, heads, HD)
    print(f"FULL_RATIO {tag} family={fam} heads={heads} lens={lens} ratio={w['ratio']:.4f} (seq {w['seq']} len {w['len']} query {w['query']})")
    assert w["ratio"] <= MARGIN, (tag, fam, w)
    return got, qkv


@pytest.mark.parametrize("heads", (1, 3))
def test_packed_lengths_within_the_rounding_budget(lib, heads):
    for fam in FAMILIES:
        _check(lib, "packed", fam, LENS, heads, seed=640 + heads)


@pytest.mark.parametrize("heads", (1, 3))
def test_fixed_len_65(lib, heads):
    for fam in ("randn", "readout"):
        got, qkv = _check(lib, "fixed65", fam, [65] * 3, heads, seed=65 + heads, fixed=True)
        packed = _run(lib, qkv, [65] * 3, heads)        # the same sequences through cu_seqlens: identical bits
        assert torch.equal(got.view(torch.int16), packed.view(torch.int16))


def _marker_keys(ln):
    keys = {0, ln - 1}
    for edge in range(64, ln, 64):
        keys.update((edge - 1, edge))
    return sorted(keys)


@pytest.mark.parametrize("heads", (1, 3))
@pytest.mark.parametrize("ln", (1300, 641))
def test_one_wrong_key_shows(lib, ln, heads):
    lens = [65, ln, 129]
    W = heads * HD
    keys = _marker_keys(ln)
    assert len(keys) <= HD - 8 and {0, ln - 1, 63, 64, 639, 640} <= set(keys)
    g = torch.Generator().manual_seed(ln + heads)
    rows = sum(lens)
    q = torch.randn(rows, heads, HD, generator=g)
    k = torch.randn(rows, heads, HD, generator=g)
    v = torch.zeros(rows, heads, HD)
    nm = len(keys)
    v[:, :, nm:] = torch.randn(rows, heads, HD - nm, generator=g)      # the columns behind the markers: dense values in every sequence
    r1 = lens[0]
    for col, key in enumerate(keys):
        v[r1 + key, :, col] = 1.0
    qkv = torch.cat([q.reshape(rows, W), k.reshape(rows, W), v.reshape(rows, W)], 1).to(torch.bfloat16).cuda()
    got = _run(lib, qkv, lens, heads)
    out, absout, _ = R.reference(qkv, lens, heads, HD, R.MASK_NONE)
    w = R.worst_coords(got, out, absout, lens, heads, HD)
    print(f"FULL_RATIO markers heads={heads} lens={lens} keys={nm} ratio={w['ratio']:.4f} (seq {w['seq']} query {w['query']} col {w['col']})")
    assert w["ratio"] <= MARGIN, w
    gv = got.view(rows, heads, HD).float()
    mid = gv[r1:r1 + ln, :, :nm]
    assert bool((mid > 0).all()), "a marker key's probability is missing from a query of its sequence"
    assert bool((gv[:r1, :, :nm] == 0).all()) and bool((gv[r1 + ln:, :, :nm] == 0).all()), "a neighbouring sequence read a marker key"
    # the measure sees one dropped key: with any one marker column zeroed, the reference itself is 128 x the budget away
    dropped = out.clone().view(rows, heads, HD)
    dropped[r1:r1 + ln, :, nm // 2] = 0
    assert R.worst_ratio(dropped.view(rows, W), out, absout) > 100
    # the marked sequence alone: the same bits (nothing of a neighbour enters)
    alone = _run(lib, qkv[r1:r1 + ln].contiguous(), [ln], heads)
    assert torch.equal(alone.view(torch.int16), got[r1:r1 + ln].view(torch.int16))


def test_argument_refusals_launch_nothing(lib):
    heads, W = 2, 128
    qkv = R.make_qkv("randn", [16], heads, HD, seed=1, device="cuda")
    cu = R.cu_seqlens([16], "cuda")
    g = Guarded(16, W)
    q, o, c, s = qkv.data_ptr(), g.ptr(), cu.data_ptr(), _s()
    af = lib.mq_attention_full
    calls = [
        ("mq_attention_full: null pointer", lambda: af(0, o, c, 1, 0, 16, heads, HD, SCALE, s)),
        ("mq_attention_full: null pointer", lambda: af(q, 0, c, 1, 0, 16, heads, HD, SCALE, s)),
        ("head_dim 128 unsupported", lambda: af(q, o, c, 1, 0, 16, 1, 128, SCALE, s)),
        ("head_dim 32 unsupported", lambda: af(q, o, c, 1, 0, 16, 4, 32, SCALE, s)),
        ("heads 0 outside [1, 1024]", lambda: af(q, o, c, 1, 0, 16, 0, HD, SCALE, s)),
        ("scale 0 must be positive", lambda: af(q, o, c, 1, 0, 16, heads, HD, 0.0, s)),
        ("need fixed_len or cu_seqlens", lambda: af(q, o, 0, 1, 0, 16, heads, HD, SCALE, s)),
        ("max sequence length 8193 unsupported", lambda: af(q, o, c, 1, 0, 8193, heads, HD, SCALE, s)),
        ("max sequence length 0 unsupported", lambda: af(q, o, c, 1, 0, 0, heads, HD, SCALE, s)),
        ("grid too large", lambda: af(q, o, c, 1 << 31, 1, 1, 1, HD, SCALE, s)),
    ]
    for fragment, call in calls:
        rc = call()
        assert rc == -1, fragment
        assert fragment in lib.mq_last_error().decode(), (fragment, lib.mq_last_error())
        torch.cuda.synchronize()
        assert g.untouched(), fragment
    assert af(q, o, c, 0, 0, 16, heads, HD, SCALE, s) == 0          # no sequences: nothing is written
    torch.cuda.synchronize()
    assert g.untouched()
    L.check(af(q, o, c, 1, 0, 16, heads, HD, SCALE, s))             # and the same geometry with valid arguments runs
    torch.cuda.synchronize()
    assert g.guards_intact() and not g.untouched()
    out, absout, _ = R.reference(qkv, [16], heads, HD, R.MASK_NONE)
    assert R.worst_ratio(g.out, out, absout) <= MARGIN

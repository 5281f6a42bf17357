"""csrc/attention_disentangled.hip through the C ABI (mq_attention_disentangled) against the float64 disentangled attention of tests/deberta_ref.py, on the
device.  The assertion is elementwise, tests/test_attention_gpu.py's:  |kernel - reference| <= MARGIN x budget with MARGIN = 1.25 imported from there and
budget = 2**-8 (P|V| + |out|) (attention_ref.budget, derived from the bf16-P / fp32-normaliser arithmetic this kernel shares with its siblings).

The fp32 position terms need no budget term of their own.  A strip value is an fp32 MFMA sum of 64 exact bf16 x bf16 products: within 64 x 2^-24 of
sum |terms|, the same kind and size of error as the q . k accumulation the budget's derivation already counts among "everything else is fp32 and two
orders of magnitude smaller".  The score is then (q . k + (c + p)) x scale: three more fp32 roundings, each 2^-24 of a sum of magnitude <= 60 on these
inputs, i.e. <= 1.1e-5 in the exponent — a relative error of the probability 350 times below bf16's 2^-8.  That sits inside the 1.25 the siblings' tests
allow for the neglected fp32 terms.  Had the strips been bf16 the exponent would carry 2^-9 |c2p| ~ 0.05: 13 times the budget.

The index table is the host-built one (DebertaArch.idx_table), int32.  Shapes (head width 64, the only one the kernel takes):
  packed lengths 1, 15, 16, 17, 63, 64, 65, 129, 200 in ONE call on 2 and 3 heads with S = 8 / max_relative_positions 64 (the table clamps from |d| = 64
  on: lengths 65 .. 200 are past the clamp); fixed_len 77 x 3; S = 256 / 512 at one 512-token sequence (a window of 511 buckets: strips of 512 values, the widest);
  700 and 1300 tokens (two and three pieces through the 512-key LDS image, far past the clamp).
One wrong entry: the sign of ONE Kr row, then ONE Qr row is flipped, then ONE d_idx entry is pointed at another bucket: the (query, head) rows that read
nothing of it come back bit for bit, the call still meets the float64 reference built with the same fault, and the rows the reference says move beyond
(2 MARGIN + 1) budgets do move beyond one budget.
Position only: q lives in dims 0 .. 31 and k in dims 32 .. 63, so q . k = 0 exactly and the output is softmax(scale (c2p + p2c)) V.
Every output buffer sits between 64 guard rows of a sentinel pattern and the workspace is exactly mq_attention_disentangled_workspace_bytes long, in
front of a sentinel tail; both are checked after every call.

Measured on an MI355X (DISENT_RATIO lines), worst |kernel - reference| / budget:
    mixed lengths randn / peaked: 2 heads 0.52 / 0.87, 3 heads 0.55 / 0.83    fixed_len 77 0.47 / 0.84    256 buckets at 512 tokens 0.25
    700 tokens 0.19, 1300 tokens 0.26    position only 0.54    one wrong entry 0.46 (the faulted calls against their own reference: 0.46)
    one flipped Kr row / Qr row: 108 (row, head) outputs read it and 108 changed (97 / 107 beyond 3.5 budgets); one d_idx entry: 180 and 180 (82).
Nothing exceeds 1.0: the 1.25 allowance is unused.
"""
import pytest
import torch

from marqo_amd import _lib as L
from marqo_amd.engine.archs import DebertaArch
from tests import attention_ref as R
from tests import deberta_ref as D
from tests.test_attention_gpu import GUARD, MARGIN, Guarded      # noqa: F401

pytestmark = pytest.mark.gpu

HD = 64
MIXED = [1, 15, 16, 17, 63, 64, 65, 129, 200]
SMALL = DebertaArch(span=8, max_rel=64)
WIDE = DebertaArch(span=256, max_rel=512)


@pytest.fixture(scope="module")
def lib():
    return L.load()


def _s():
    return torch.cuda.current_stream().cuda_stream


def _tables(arch, heads, seed):
    g = torch.Generator().manual_seed(400 + seed)
    kr = torch.randn(heads, 2 * arch.span, HD, generator=g).to(torch.bfloat16).cuda()
    qr = torch.randn(heads, 2 * arch.span, HD, generator=g).to(torch.bfloat16).cuda()
    return kr, qr


def _window(table, reach, maxl):
    return int(table[reach - (maxl - 1)]), int(table[reach + (maxl - 1)])


def _run(lib, qkv, lens, heads, kr, qr, table, reach, span, scale, fixed=False, fill=0xA5):
    """one call on a guarded output and an exact-length workspace -> bf16 [rows, heads hd]"""
    rows, maxl = qkv.shape[0], max(lens)
    g = Guarded(rows, heads * HD)
    lo, hi = _window(table, reach, maxl)
    need = lib.mq_attention_disentangled_workspace_bytes(rows, heads, lo, hi)
    assert need == rows * heads * 2 * ((hi - lo + 1 + 15) // 16 * 16) * 4
    ws = torch.full((need + 4096,), fill, dtype=torch.uint8, device="cuda")
    d_idx = table.to(torch.int32).cuda().contiguous()
    if fixed:
        assert len(set(lens)) == 1
        rc = lib.mq_attention_disentangled(qkv.data_ptr(), g.ptr(), None, len(lens), rows, lens[0], 0, heads, HD, kr.data_ptr(), qr.data_ptr(), d_idx.data_ptr(),
                                           reach, span, lo, hi, scale, ws.data_ptr(), need, _s())
    else:
        cu = R.cu_seqlens(lens, "cuda")
        rc = lib.mq_attention_disentangled(qkv.data_ptr(), g.ptr(), cu.data_ptr(), len(lens), rows, 0, maxl, heads, HD, kr.data_ptr(), qr.data_ptr(),
                                           d_idx.data_ptr(), reach, span, lo, hi, scale, ws.data_ptr(), need, _s())
    L.check(rc, "mq_attention_disentangled")
    torch.cuda.synchronize()
    assert g.guards_intact()
    assert bool((ws[need:] == fill).all()), "the workspace was written past mq_attention_disentangled_workspace_bytes"
    return g.out


def _check(lib, tag, fam, arch, lens, heads, seed=0, fixed=False, qkv=None, tables=None, table=None):
    reach = max(lens) - 1 + 7          # (a table longer than the call needs: the kernel indexes it from its middle)
    table = arch.idx_table(reach) if table is None else table
    scale = (3 * HD) ** -0.5
    if qkv is None:
        qkv = R.make_qkv(fam, lens, heads, HD, seed=seed).cuda()
    kr, qr = tables if tables is not None else _tables(arch, heads, seed)
    got = _run(lib, qkv, lens, heads, kr, qr, table, reach, arch.span, scale, fixed)
    out, absout, _ = D.disentangled_reference(qkv, lens, heads, HD, kr, qr, table, reach, scale)
    w = R.worst_coords(got, out, absout, lens, heads, HD)
    print(f"DISENT_RATIO {tag} family={fam} heads={heads} S={arch.span} max_rel={arch.max_rel} lens={lens} ratio={w['ratio']:.4f}")
    assert w["ratio"] <= MARGIN, (tag, fam, w)
    return got, out, absout, (qkv, kr, qr, table, reach, scale)


@pytest.mark.parametrize("heads", (2, 3))
def test_mixed_packed_lengths_past_the_clamp(lib, heads):
    t = SMALL.idx_table(199)
    assert int(t[0]) == 0 and int(t[-1]) == 15 and int(t[199 - 63]) == 1 and int(t[199 + 63]) == 15      # clamped from |d| = 64 on
    for fam in ("randn", "peaked"):
        _check(lib, "mixed", fam, SMALL, MIXED, heads, seed=64 + heads)


def test_fixed_len_77(lib):
    for heads, fam in ((2, "randn"), (3, "peaked")):
        _check(lib, "fixed77", fam, SMALL, [77] * 3, heads, seed=77 + heads, fixed=True)


def test_256_buckets_at_512_tokens(lib):
    t = WIDE.idx_table(511)
    assert int(t[0]) == 1 and int(t[-1]) == 511      # 511 of the 512 buckets are inside the window (bucket 0 is reached from |d| = 512 on)
    _check(lib, "wide", "randn", WIDE, [512], 2, seed=512)


@pytest.mark.parametrize("ln, heads, pieces", ((700, 2, 2), (1300, 3, 3)))
def test_sequences_longer_than_the_lds_holds(lib, ln, heads, pieces):
    assert -(-(-(-ln // 64) * 64) // D.LDS_KEYS) == pieces
    _check(lib, "long", "randn", SMALL, [ln], heads, seed=ln)


def test_position_only(lib):
    """q . k = 0 through orthogonal halves: the result is the two gathered terms alone"""
    lens, heads = [100, 65, 9], 2
    qkv = R.make_qkv("randn", lens, heads, HD, seed=9).cuda()
    W = heads * HD
    q, k = qkv[:, :W].view(-1, heads, HD), qkv[:, W:2 * W].view(-1, heads, HD)
    q[:, :, 32:] = 0
    k[:, :, :32] = 0
    assert float((q.double() * k.double()).abs().sum()) == 0.0
    _, _, _, (qkv, kr, qr, table, reach, scale) = _check(lib, "position_only", "randn", SMALL, lens, heads, qkv=qkv)
    _, _, scores = D.disentangled_reference(qkv, lens, heads, HD, kr, qr, table, reach, scale)
    assert float(scores[0].std()) > 0.3, "the position terms alone must decide the probabilities"


def _moved(a, b, heads):
    """[rows, heads] bool: which (query row, head) outputs differ in any bit"""
    return (a.view(torch.int16) != b.view(torch.int16)).view(a.shape[0], heads, HD).any(-1)


def test_one_wrong_entry(lib):
    lens, heads, arch = [100, 30], 2, SMALL
    got, out, absout, (qkv, kr, qr, table, reach, scale) = _check(lib, "one_wrong", "randn", arch, lens, heads, seed=21)
    bud = R.budget(out, absout)
    pos = [torch.arange(n) for n in lens]
    pair_idx = [D.pair_index(table, n, reach) for n in lens]
    hh, j = 1, int(table[reach + 20])                   # the log bucket of d = +20 on head 1
    assert 8 < j < 15
    reads_j = torch.cat([(pi == j).any(1) for pi in pair_idx])           # per query row: some key at a distance of that bucket
    assert 0 < int(reads_j.sum()) < sum(lens)
    cases = []
    kr2 = kr.clone(); kr2[hh, j] = -kr2[hh, j]
    cases.append(("Kr row", kr2, qr, table, reads_j, hh))
    qr2 = qr.clone(); qr2[hh, j] = -qr2[hh, j]
    cases.append(("Qr row", kr, qr2, table, reads_j, hh))
    t2 = table.clone(); t2[reach + 20] = 2 * arch.span - 1 - j           # one distance reads another bucket, on every head
    reads_d = torch.cat([p >= 20 for p in pos])
    cases.append(("d_idx entry", kr, qr, t2, reads_d, None))
    for name, a, b, t, readers, head in cases:
        got2 = _run(lib, qkv, lens, heads, a, b, t, reach, arch.span, scale)
        out2, absout2, _ = D.disentangled_reference(qkv, lens, heads, HD, a, b, t, reach, scale)
        w = R.worst_coords(got2, out2, absout2, lens, heads, HD)
        print(f"DISENT_RATIO one_wrong/{name} ratio={w['ratio']:.4f}")
        assert w["ratio"] <= MARGIN, (name, w)
        expect = readers[:, None].expand(-1, heads).clone()
        if head is not None:
            expect[:, [h for h in range(heads) if h != head]] = False
        moved = _moved(got.cpu(), got2.cpu(), heads)
        assert not bool((moved & ~expect).any()), f"{name}: a row that reads nothing of the entry changed"
        # where the float64 reference moves by more than (2 MARGIN + 1) budgets, two kernels that each sit within MARGIN budgets of their reference
        # differ by more than one budget: |got2 - got| >= |out2 - out| - MARGIN bud2 - MARGIN bud
        both = torch.maximum(bud, R.budget(out2, absout2))
        big_el = (out2 - out).abs() > (2 * MARGIN + 1) * both
        big = big_el.view(-1, heads, HD).any(-1).cpu()
        assert int(big.sum()) > 0 and not bool((big & ~expect).any())
        assert bool(((got2.double() - got.double()).abs() > both)[big_el].all()), f"{name}: an element the entry decides did not move beyond the budget"
        print(f"DISENT one_wrong/{name}: {int(expect.sum())} (row, head) outputs read it, {int(moved.sum())} changed, {int(big.sum())} beyond {2 * MARGIN + 1} budgets")


def test_empty_call_writes_nothing(lib):
    g = Guarded(4, 128)
    kr, qr = _tables(SMALL, 2, 0)
    t = SMALL.idx_table(7).cuda()
    ws = torch.full((4096,), 0xA5, dtype=torch.uint8, device="cuda")
    qkv = torch.zeros(4, 384, dtype=torch.bfloat16, device="cuda")
    assert lib.mq_attention_disentangled(qkv.data_ptr(), g.ptr(), None, 0, 0, 4, 0, 2, 64, kr.data_ptr(), qr.data_ptr(), t.data_ptr(), 7, 8, 1, 15, 0.07,
                                         ws.data_ptr(), 4096, _s()) == 0
    torch.cuda.synchronize()
    assert g.untouched() and bool((ws == 0xA5).all())


def test_argument_checks_and_a_workspace_one_byte_short(lib):
    lens, heads = [40, 9], 2
    rows, reach = sum(lens), 39
    t = SMALL.idx_table(reach)
    lo, hi = _window(t, reach, 40)
    d_idx = t.cuda()
    kr, qr = _tables(SMALL, heads, 1)
    qkv = R.make_qkv("randn", lens, heads, HD, seed=1).cuda()
    cu = R.cu_seqlens(lens, "cuda")
    g = Guarded(rows, heads * HD)
    need = lib.mq_attention_disentangled_workspace_bytes(rows, heads, lo, hi)
    ws = torch.full((need,), 0xA5, dtype=torch.uint8, device="cuda")

    def call(**o):
        a = dict(qkv=qkv.data_ptr(), nseq=2, rows=rows, maxl=40, hd=64, kr=kr.data_ptr(), qr=qr.data_ptr(), idx=d_idx.data_ptr(), reach=reach, span=8, ws=need)
        a.update(o)
        return lib.mq_attention_disentangled(a["qkv"], g.ptr(), cu.data_ptr(), a["nseq"], a["rows"], 0, a["maxl"], heads, a["hd"], a["kr"], a["qr"], a["idx"],
                                             a["reach"], a["span"], lo, hi, 0.07, ws.data_ptr(), a["ws"], _s())
    for o, word in ((dict(hd=128), b"head_dim"), (dict(span=0), b"span"), (dict(span=1025), b"span"), (dict(kr=None), b"null position table"),
                    (dict(qr=None), b"null position table"), (dict(idx=None), b"null position table"), (dict(maxl=41), b"reach")):
        assert call(**o) == -1 and word in lib.mq_last_error(), (o, lib.mq_last_error())
    assert call(ws=need - 1) == -3 and b"mq_attention_disentangled: workspace" in lib.mq_last_error()
    torch.cuda.synchronize()
    assert g.untouched() and bool((ws == 0xA5).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert g.guards_intact()


def test_the_result_does_not_depend_on_what_the_workspace_held(lib):
    lens, heads = [129, 17], 3
    reach = 128
    t = SMALL.idx_table(reach)
    kr, qr = _tables(SMALL, heads, 2)
    qkv = R.make_qkv("randn", lens, heads, HD, seed=2).cuda()
    a = _run(lib, qkv, lens, heads, kr, qr, t, reach, 8, 0.07, fill=0x00)
    b = _run(lib, qkv, lens, heads, kr, qr, t, reach, 8, 0.07, fill=0xFF)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))

"""csrc/attention_relbias.hip through the C ABI (mq_attention_relbias) against the float64 attention of tests/attention_ref.py extended by the clamped bias
(tests/t5_ref.py::relbias_reference), on the device.  The assertion is elementwise, tests/test_attention_gpu.py's:  |kernel - reference| <= 1.25 x budget,
budget = 2**-8 (P|V| + |out|) (attention_ref.budget, derived from the bf16-P / fp32-normaliser arithmetic this kernel shares; the 1.25 is that file's
allowance for the fp32 terms the derivation neglects — here one more fp32 FMA per score, scale (q . k) + bias — not a fitted number).

Shapes: head widths 64 and 128; 2 and 3 heads; the packed lengths 1, 15, 16, 17, 63, 64, 65, 129, 300 in ONE call (63 / 64 / 65: the 64-query slice of
the kernel; 300 passes the clamp on both sides at D = 128 and takes the one-value path of whole tiles); one 700-token sequence at 64 and one 330-token
sequence at 128, past the 576 / 256 keys the LDS holds next to the bias table, so K / V stream through in pieces; fixed_len 77; D = 128 and D = 4; scale
1.0 and 1 / sqrt(hd).  Families `randn`, `peaked`, `readout` of attention_ref.

The inputs at scale 1.0 carry 1 / sqrt(hd) in q, as T5 checkpoints do (the model applies no softmax scale: training puts it into the q projection).  The
families' unit-variance q and k taken raw give scores of standard deviation sqrt(hd): at hd = 128 a `readout` column then holds ONE probability as small
as 2.8e-39 in float64 — below fp32's normal range, where v_exp_f32 returns 0 — and the budget, which is relative, has no term for that underflow (the
first GPU run of this file measured exactly that element: got 0.0, reference 2.8e-39, every other family and shape inside 1.0).  With the scale in q the
logits are those of the 1 / sqrt(hd) calls, formed on the other path: scale inside the operand, not in the kernel's FMA.

The bias-only case: q = k = 0, one-hot V codes of the key index, a table with a value of its own in every column: the output is softmax(bias row) applied
to V.  tests/test_t5_host.py shows on the same inputs that an index off by one, a mirrored sign and a clamp at D - 1 leave the budget by more than 50 x.

Every output buffer sits between 64 guard rows of a sentinel pattern, checked after every call.

Measured on an MI355X (RELBIAS_RATIO lines), worst |kernel - reference| / budget:
    head width 64 / 128:  mixed lengths 0.93 / 0.96    long sequences (700 / 330) 0.86 / 0.88    fixed_len 77 0.92 / 0.94    slice edges 0.95 / 0.95
    bias only 0.90 / 0.95.  Nothing exceeds 1.0: the 1.25 allowance is unused."""
import pytest
import torch

from marqo_amd import _lib as L
from tests import attention_ref as R
from tests import t5_ref as T
from tests.test_attention_gpu import GUARD, MARGIN, Guarded      # noqa: F401

pytestmark = pytest.mark.gpu

MIXED = [1, 15, 16, 17, 63, 64, 65, 129, 300]
FAMS = ("randn", "peaked", "readout")


@pytest.fixture(scope="module")
def lib():
    return L.load()


def _s():
    return torch.cuda.current_stream().cuda_stream


def _run(lib, qkv, lens, heads, hd, table, D, scale, fixed=False):
    """one call on a guarded output -> bf16 [rows, heads hd]"""
    g = Guarded(qkv.shape[0], heads * hd)
    d_table = table.to("cuda").contiguous()
    if fixed:
        assert len(set(lens)) == 1
        rc = lib.mq_attention_relbias(qkv.data_ptr(), g.ptr(), None, len(lens), lens[0], 0, heads, hd, d_table.data_ptr(), D, scale, _s())
    else:
        cu = R.cu_seqlens(lens, "cuda")
        rc = lib.mq_attention_relbias(qkv.data_ptr(), g.ptr(), cu.data_ptr(), len(lens), 0, max(lens), heads, hd, d_table.data_ptr(), D, scale, _s())
    L.check(rc, "mq_attention_relbias")
    torch.cuda.synchronize()
    assert g.guards_intact()
    return g.out


def _check(lib, tag, fam, lens, heads, hd, D, scale, seed=0, fixed=False, qkv=None, table=None):
    if qkv is None:
        qkv = R.make_qkv(fam, lens, heads, hd, seed=seed, device="cuda")
        if scale == 1.0:      # the checkpoint's convention: 1 / sqrt(hd) rides in q (module docstring); the reference reads the same bf16 numbers
            qkv[:, :heads * hd] = (qkv[:, :heads * hd].float() * hd ** -0.5).to(torch.bfloat16)
    table = T.make_table(heads, D, seed=seed) if table is None else table
    got = _run(lib, qkv, lens, heads, hd, table, D, scale, fixed)
    out, absout = T.relbias_reference(qkv, lens, heads, hd, table, D, scale)
    w = R.worst_coords(got, out, absout, lens, heads, hd)
    print(f"RELBIAS_RATIO {tag} family={fam} hd={hd} heads={heads} D={D} scale={scale:.4f} lens={lens} ratio={w['ratio']:.4f}")
    assert w["ratio"] <= MARGIN, (tag, fam, w)


@pytest.mark.parametrize("D", (128, 4))
@pytest.mark.parametrize("hd, heads", ((64, 2), (64, 3), (128, 2), (128, 3)))
def test_mixed_packed_lengths(lib, hd, heads, D):
    for fam in FAMS:
        for scale in (1.0, hd ** -0.5):
            _check(lib, "mixed", fam, MIXED, heads, hd, D, scale, seed=hd + heads + D)


@pytest.mark.parametrize("hd, ln", ((64, 700), (128, 330)))
def test_sequences_longer_than_the_lds_holds(lib, hd, ln):
    """past the 576 / 256 keys of the LDS image: the sequence streams through in two pieces, for every one of its 64-query slices"""
    assert ln > T.LDS_KEYS[hd]
    for fam in FAMS:
        for D, scale, heads in ((128, 1.0, 2), (4, hd ** -0.5, 3)):
            _check(lib, "long", fam, [ln], heads, hd, D, scale, seed=ln)


@pytest.mark.parametrize("hd", (64, 128))
def test_fixed_len_77(lib, hd):
    for fam in FAMS:
        _check(lib, "fixed77", fam, [77] * 3, 2, hd, 128, 1.0, seed=77, fixed=True)
        _check(lib, "fixed77", fam, [77] * 3, 3, hd, 4, hd ** -0.5, seed=78, fixed=True)


@pytest.mark.parametrize("hd", (64, 128))
def test_query_slice_boundaries(lib, hd):
    """lengths slice - 1, slice, slice + 1 and their doubles, each alone in a call (max_len sets the number of slices launched) and packed together"""
    S = T.SLICE
    for ln in (S - 1, S, S + 1, 2 * S - 1, 2 * S, 2 * S + 1):
        _check(lib, "slice", "readout", [ln], 2, hd, 128, 1.0, seed=ln)
    _check(lib, "slice", "randn", [S - 1, S, S + 1, 2 * S + 1, 1], 3, hd, 4, 1.0, seed=5)


@pytest.mark.parametrize("hd, D, lens", ((64, 128, [300, 17]), (128, 4, [65, 9]), (64, 4, [700]), (128, 128, [330, 1])))
def test_bias_only(lib, hd, D, lens):
    """q = k = 0: the output is softmax(bias row) applied to one-hot V codes; the inputs of tests/test_t5_host.py's fault check and two longer ones"""
    heads = 2
    qkv = T.bias_only_qkv(lens, heads, hd, device="cuda")
    table = T.make_table(heads, D, seed=1, kind="distinct")
    for scale in (1.0, hd ** -0.5):      # (q . k is 0: the scale must not matter)
        _check(lib, "bias_only", "readout", lens, heads, hd, D, scale, qkv=qkv, table=table)
    a = _run(lib, qkv, lens, heads, hd, table, D, 1.0)
    b = _run(lib, qkv, lens, heads, hd, table, D, hd ** -0.5)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))


def test_empty_call_writes_nothing(lib):
    g = Guarded(4, 128)
    t = torch.zeros(2, 257, device="cuda")
    qkv = torch.zeros(4, 384, dtype=torch.bfloat16, device="cuda")
    assert lib.mq_attention_relbias(qkv.data_ptr(), g.ptr(), None, 0, 4, 0, 2, 64, t.data_ptr(), 128, 1.0, _s()) == 0
    torch.cuda.synchronize()
    assert g.untouched()

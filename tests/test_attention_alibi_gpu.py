"""csrc/attention_alibi.hip through the C ABI (mq_attention_alibi) against the float64 attention of tests/attention_ref.py extended by the ALiBi bias
(tests/jina_bert_ref.py::alibi_reference), on the device.  The assertion is elementwise, tests/test_attention_gpu.py's:  |kernel - reference| <= 1.25 x
budget, budget = 2**-8 (P|V| + |out|) (attention_ref.budget, derived from the bf16-P / fp32-normaliser arithmetic this kernel shares; the 1.25 is that
file's allowance for the fp32 terms the derivation neglects — here one fp32 multiply and one FMA per score, scale (q . k) - slope |k - q|, the term
tests/test_attention_relbias_gpu.py already argues for — not a fitted number).

Shapes (head width 64, the only one the kernel takes): 2 and 3 heads; the packed lengths 1, 15, 16, 17, 63, 64, 65, 129, 300 in ONE call; the slice edges
63, 64, 65, 127, 128, 129, each alone in a call (max_len sets the number of slices launched) and packed together; fixed_len 77 x 3; one 700-token sequence
(two pieces through the 640-key LDS image) and one 1300-token sequence (three pieces); scale 1.0 and 1 / sqrt(64).  At scale 1.0 the 1 / sqrt(hd) rides in
q (tests/jina_bert_ref.py::family_qkv, the convention of tests/test_attention_relbias_gpu.py and the reason recorded there).

Families and slopes.  `randn` and `peaked` run with the real slopes: the first 2 or 3 values of the 8-head and of the 12-head list (2^-1, 2^-2, 2^-3) and
the 12-head list's tail (2^-0.5, 2^-1.5, 2^-2.5: the steepest, and not powers of two).  `readout` and the bias-only inputs isolate single probabilities;
the budget is relative and has no term for fp32 underflow (the relbias docstring), so those cases take slopes that keep the smallest float64 probability
of their inputs at or above 2^-100 (jina_bert_ref.readout_slopes) — a precondition, not a tolerance, asserted on the CPU for exactly these inputs by
tests/test_jina_bert_host.py::test_readout_and_bias_only_inputs_keep_every_probability_above_2_pow_minus_100.

The bias-only case: q = k = 0, one-hot V codes of the key index, a slope of its own per head: the output is softmax(-slope |k - q|) applied to V, and it
must not depend on the scale, bit for bit.  tests/test_jina_bert_host.py shows on the same inputs that a distance off by one, a missing |.|, the next
head's slope and a bias multiplied by the scale each leave the budget.

Every output buffer sits between 64 guard rows of a sentinel pattern, checked after every call.

Measured on an MI355X (ALIBI_RATIO lines), worst |kernel - reference| / budget:
    randn / peaked / readout:  mixed lengths 0.76 / 0.91 / 0.96    slice edges 0.70 / 0.87 / 0.96    fixed_len 77 0.71 / 0.88 / 0.96
    long sequences (700, 1300) 0.73 / 0.94 / 0.88    bias only 0.94.  Nothing exceeds 1.0: the 1.25 allowance is unused."""
import pytest
import torch

from marqo_amd import _lib as L
from tests import attention_ref as R
from tests import jina_bert_ref as J
from tests.test_attention_gpu import GUARD, MARGIN, Guarded      # noqa: F401

pytestmark = pytest.mark.gpu

HD = 64


@pytest.fixture(scope="module")
def lib():
    return L.load()


def _s():
    return torch.cuda.current_stream().cuda_stream


def _run(lib, qkv, lens, heads, slopes, scale, fixed=False):
    """one call on a guarded output -> bf16 [rows, heads hd]"""
    g = Guarded(qkv.shape[0], heads * HD)
    d_slopes = slopes.to(torch.float32).to("cuda").contiguous()
    if fixed:
        assert len(set(lens)) == 1
        rc = lib.mq_attention_alibi(qkv.data_ptr(), g.ptr(), None, len(lens), lens[0], 0, heads, HD, d_slopes.data_ptr(), scale, _s())
    else:
        cu = R.cu_seqlens(lens, "cuda")
        rc = lib.mq_attention_alibi(qkv.data_ptr(), g.ptr(), cu.data_ptr(), len(lens), 0, max(lens), heads, HD, d_slopes.data_ptr(), scale, _s())
    L.check(rc, "mq_attention_alibi")
    torch.cuda.synchronize()
    assert g.guards_intact()
    return g.out


def _check(lib, tag, fam, lens, heads, slopes, scale, seed=0, fixed=False, qkv=None, sname=""):
    if qkv is None:
        qkv = J.family_qkv(fam, lens, heads, HD, scale, seed, device="cuda")
    got = _run(lib, qkv, lens, heads, slopes, scale, fixed)
    out, absout = J.alibi_reference(qkv, lens, heads, HD, slopes, scale)
    w = R.worst_coords(got, out, absout, lens, heads, HD)
    print(f"ALIBI_RATIO {tag} family={fam} heads={heads} slopes={sname or [float(x) for x in slopes]} scale={scale:.4f} lens={lens} ratio={w['ratio']:.4f}")
    assert w["ratio"] <= MARGIN, (tag, fam, w)


def _real(lib, tag, lens, heads, scale, seed, fixed=False, fams=("randn", "peaked")):
    for fam in fams:
        for sname, slopes in J.real_slopes(heads):
            _check(lib, tag, fam, lens, heads, slopes, scale, seed=seed, fixed=fixed, sname=sname)


def _readout(lib, tag):
    n = 0
    for t, lens, heads, scale, seed, fixed in J.readout_cases():
        if t == tag:
            _check(lib, tag, "readout", lens, heads, J.readout_slopes(max(lens), heads), scale, seed=seed, fixed=fixed)
            n += 1
    assert n


@pytest.mark.parametrize("heads", (2, 3))
def test_mixed_packed_lengths(lib, heads):
    for scale in J.SCALES:
        _real(lib, "mixed", J.MIXED, heads, scale, seed=64 + heads)
    _readout(lib, "mixed")


def test_query_slice_boundaries(lib):
    """lengths slice - 1, slice, slice + 1 and their doubles, each alone in a call and packed together"""
    _readout(lib, "slice")
    for ln in J.EDGES:
        _real(lib, "slice", [ln], 2, 64 ** -0.5, seed=ln, fams=("randn",))
    _real(lib, "slice", J.EDGES + [1], 3, 1.0, seed=5)


def test_fixed_len_77(lib):
    _real(lib, "fixed77", [77] * 3, 2, 1.0, seed=77, fixed=True)
    _real(lib, "fixed77", [77] * 3, 3, 64 ** -0.5, seed=78, fixed=True)
    _readout(lib, "fixed77")


@pytest.mark.parametrize("ln, heads, scale, pieces", ((700, 2, 1.0, 2), (1300, 3, 64 ** -0.5, 3)))
def test_sequences_longer_than_the_lds_holds(lib, ln, heads, scale, pieces):
    """past the 640 keys of the LDS image: the sequence streams through in two (700) and three (1300) pieces, for every one of its 64-query slices"""
    assert -(-(-(-ln // 64) * 64) // J.LDS_KEYS[HD]) == pieces
    _real(lib, "long", [ln], heads, scale, seed=ln)
    _readout(lib, "long")


@pytest.mark.parametrize("lens", J.BIAS_ONLY)
def test_bias_only(lib, lens):
    """q = k = 0: the output is softmax(-slope |k - q|) applied to one-hot V codes, whatever the scale, bit for bit"""
    heads = 2
    qkv = J.bias_only_qkv(lens, heads, HD, device="cuda")
    slopes = J.readout_slopes(max(lens), heads)
    for scale in J.SCALES:
        _check(lib, "bias_only", "readout", lens, heads, slopes, scale, qkv=qkv)
    a = _run(lib, qkv, lens, heads, slopes, 1.0)
    b = _run(lib, qkv, lens, heads, slopes, 64 ** -0.5)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))


def test_empty_call_writes_nothing(lib):
    g = Guarded(4, 128)
    sl = torch.ones(2, device="cuda")
    qkv = torch.zeros(4, 384, dtype=torch.bfloat16, device="cuda")
    assert lib.mq_attention_alibi(qkv.data_ptr(), g.ptr(), None, 0, 4, 0, 2, 64, sl.data_ptr(), 1.0, _s()) == 0
    torch.cuda.synchronize()
    assert g.untouched()

"""The three kernels of csrc/colbert.hip against float64 on the same bf16 operands; budgets from the kernels' arithmetic, bar 1.25 (u32 = 2**-24, u16 = 2**-8):
  mq_maxsim            a dot product is an fp32 chain of D exact products: <= D u32 sum_k |q_k d_k|; a maximum of perturbed values is off by at most the
                       largest of those; the sum of Lq maxima adds <= Lq u32 sum_i |max_i|
  mq_colbert_project   y and its norm in fp32 (<= W u32 |L| |x| per element), ONE bf16 rounding: u16 |out| + W u32 (|L| |x|) / ||y|| + the norm's own
                       relative error on |out|
  mq_attention_keyprefix   tests/attention_ref.py's budget u16 (P|V| + |out|), the softmax over keys [0, n_keys)"""
import math

import pytest
import torch

from marqo_amd import _lib as L
from tests import attention_ref as R

pytestmark = pytest.mark.gpu
MARGIN, U32, U16 = 1.25, 2.0 ** -24, 2.0 ** -8
LENS = [1, 15, 16, 17, 63, 64, 65, 200]


@pytest.fixture(scope="module")
def lib():
    return L.load()


def _s():
    return torch.cuda.current_stream().cuda_stream


def _unit(n, D, seed):
    x = torch.randn(n, D, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    return (x / x.norm(dim=1, keepdim=True)).to(torch.bfloat16).cuda()


def _maxsim(lib, q, docs, lens, keep):
    cu = R.cu_seqlens(lens, "cuda")
    out = torch.full((len(lens),), float("nan"), device="cuda")
    L.check(lib.mq_maxsim(q.data_ptr(), docs.data_ptr(), cu.data_ptr(), keep.data_ptr(), len(lens), docs.shape[0], q.shape[0], q.shape[1], out.data_ptr(),
                          _s()), "mq_maxsim")
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("D", (64, 96, 128))
@pytest.mark.parametrize("Lq", (1, 31, 32, 64))
def test_maxsim_within_budget_and_bits_do_not_depend_on_neighbours(lib, Lq, D):
    q, docs = _unit(Lq, D, 7 * Lq + D), _unit(sum(LENS), D, Lq + D)
    keep = (torch.rand(sum(LENS), generator=torch.Generator().manual_seed(D)) > 0.2).to(torch.uint8).cuda()
    keep[R.cu_seqlens(LENS, "cuda")[:-1].long()] = 1         # every document keeps its first token
    got, r0, worst = _maxsim(lib, q, docs, LENS, keep), 0, 0.0
    for i, ln in enumerate(LENS):
        d, k = docs[r0:r0 + ln], keep[r0:r0 + ln]
        m = (q.double() @ d.double().t()).masked_fill(~k.bool()[None], float("-inf")).max(dim=1).values
        a = (q.double().abs() @ d.double().abs().t()).masked_fill(~k.bool()[None], 0.0).max(dim=1).values
        worst = max(worst, float((got[i].double() - m.sum()).abs() / (U32 * (D * a.sum() + Lq * m.abs().sum()))))
        assert torch.equal(_maxsim(lib, q, d.clone(), [ln], k.clone()).view(torch.int32), got[i:i + 1].view(torch.int32)), (i, ln)   # alone: the same bits
        r0 += ln
    print(f"MAXSIM_RATIO Lq={Lq} D={D} ratio={worst:.4f}")
    assert worst <= MARGIN


@pytest.mark.parametrize("ln", (17, 64, 65, 130))
@pytest.mark.parametrize("plant", ("last_kept", "next_document", "excluded", "excluded_negative"))
def test_maxsim_sees_one_wrong_token(lib, plant, ln):
    """q = e0 (one query row): the score IS the winning token's first coordinate"""
    q = torch.zeros(1, 64, dtype=torch.bfloat16, device="cuda")
    q[0, 0] = 1.0
    docs = torch.zeros(ln + 3, 64, dtype=torch.bfloat16, device="cuda")
    docs[:, 0] = -0.25 if plant == "excluded_negative" else 0.25
    keep = torch.ones(ln + 3, dtype=torch.uint8, device="cuda")
    want = [float(docs[0, 0])] * 2
    if plant == "last_kept":            # the winner is the last kept token; the document's last token is excluded
        keep[ln - 1] = 0
        docs[ln - 2, 0], want[0] = 0.75, 0.75
    elif plant == "next_document":
        docs[ln, 0], want[1] = 0.875, 0.875
    else:
        keep[ln // 2] = 0
        docs[ln // 2, 0] = 0.875
    assert _maxsim(lib, q, docs, [ln, 3], keep).tolist() == want


@pytest.mark.parametrize("rows", (1, 63, 65))
@pytest.mark.parametrize("W,D", ((384, 96), (384, 128), (768, 96), (768, 128)))
def test_project_within_budget(lib, W, D, rows):
    g = torch.Generator().manual_seed(W + D + rows)
    x = torch.randn(rows, W, generator=g) * 3.0
    x[rows // 2] *= float(rows == 1)                              # one all-zero row (not the only row)
    lw = (torch.randn(D, W, generator=g) / math.sqrt(W)).to(torch.bfloat16)
    out = torch.full((rows + 2, D), 7.0, dtype=torch.bfloat16, device="cuda")
    xc, lc = x.cuda(), lw.cuda()
    L.check(lib.mq_colbert_project(xc.data_ptr(), lc.data_ptr(), out[1:].data_ptr(), rows, W, D, 1e-12, _s()), "mq_colbert_project")
    torch.cuda.synchronize()
    assert (out[0] == 7.0).all() and (out[-1] == 7.0).all() and torch.isfinite(out.float()).all()
    xb, ld = x.to(torch.bfloat16).double(), lw.double()
    y, ay = xb @ ld.t(), xb.abs() @ ld.abs().t()
    nrm = y.norm(dim=1, keepdim=True).clamp_min(1e-12)
    rel_norm = W * U32 * (ay.norm(dim=1, keepdim=True) / nrm) + 4 * U32     # the norm's own relative error: accumulation + sqrt / max / divide
    bud = U16 * (y / nrm).abs() + W * U32 * ay / nrm + rel_norm * (y / nrm).abs()
    err, ok = (out[1:-1].cpu().double() - y / nrm).abs(), bud > 0
    ratio = (err[ok] / bud[ok]).max().item() if ok.any() else 0.0
    print(f"PROJECT_RATIO W={W} D={D} rows={rows} ratio={ratio:.4f}")
    assert ratio <= MARGIN and (err[~ok] == 0).all()              # (the zero row's budget is zero: it must come out exactly zero)


def _keyprefix(lib, qkv, lens, nkeys, W, heads):
    cu, nk = R.cu_seqlens(lens), torch.tensor(nkeys, dtype=torch.int32)
    d_cu, d_nk = cu.cuda(), nk.cuda()
    out = torch.zeros(qkv.shape[0], W, dtype=torch.bfloat16, device="cuda")
    L.check(lib.mq_attention_keyprefix(qkv.data_ptr(), out.data_ptr(), d_cu.data_ptr(), cu.data_ptr(), d_nk.data_ptr(), nk.data_ptr(), len(lens), W, heads,
                                       _s()), "mq_attention_keyprefix")
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("real", (64, 32))
@pytest.mark.parametrize("lens,nkeys", (([32], [3]), ([32], [31]), ([32], [32]), ([64], [5]), ([32, 17], [7, 17])))
def test_keyprefix_within_budget_and_blind_to_the_first_excluded_key(lib, lens, nkeys, real):
    heads, hs = 2, 64                  # 32-wide heads run zero-padded to 64, as the loader leaves them
    W = heads * hs
    qkv = R.make_qkv("peaked", lens, heads, hs, seed=sum(lens) + sum(nkeys), device="cuda", real=real if real < hs else None)
    got = _keyprefix(lib, qkv, lens, nkeys, W, heads)
    out, absout, planted, r0 = torch.zeros(sum(lens), W, dtype=torch.float64), torch.zeros(sum(lens), W, dtype=torch.float64), qkv.clone(), 0
    for ln, nk in zip(lens, nkeys):     # float64 softmax over keys [0, nk); a key and a value nobody may see planted at key nk
        q, k, v = (t.reshape(ln, heads, hs).transpose(0, 1) for t in qkv[r0:r0 + ln].cpu().double().split(W, dim=1))
        p = torch.softmax((q @ k[:, :nk].transpose(1, 2)) / math.sqrt(hs), dim=-1)
        out[r0:r0 + ln] = (p @ v[:, :nk]).transpose(0, 1).reshape(ln, W)
        absout[r0:r0 + ln] = (p @ v[:, :nk].abs()).transpose(0, 1).reshape(ln, W)
        if nk < ln:
            planted[r0 + nk, W:] = 60.0
        r0 += ln
    ratio = R.worst_ratio(got.cpu(), out, absout)
    print(f"KEYPREFIX_RATIO lens={lens} n_keys={nkeys} real={real} ratio={ratio:.4f}")
    assert ratio <= MARGIN and torch.equal(_keyprefix(lib, planted, lens, nkeys, W, heads), got)
    if nkeys == lens:                   # full attention: within mq_attention(MQ_MASK_NONE)'s budget on the same input
        fo, fa, _ = R.reference(qkv, lens, heads, hs, R.MASK_NONE)
        assert R.worst_ratio(got.cpu(), fo.cpu(), fa.cpu()) <= MARGIN

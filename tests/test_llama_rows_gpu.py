"""The row kernels of the Mistral / Llama tower for rows up to 4096 wide (csrc/llama.hip) on the GPU, against float64.

Budgets (u = 2**-24, margin 1.25 as in tests/test_qwen_gpu.py for the terms a derivation neglects):
  mq_rmsnorm_wide: tests/test_qwen_gpu.py's for mq_rmsnorm, |y| (D / 2 + 7) u with D = rowops_ref.chain(W) = ceil(W / 64) + 8 — a lane sums its W / 256
      chunk sums one after the other and the wave adds six butterfly levels, which D covers at every W up to 4096; bf16 output: plus half a bf16 ulp.
      At W <= 2048 the entry point is mq_rmsnorm: torch.equal.
  mq_embed_tokens_wide: a copy, bit-exact.
  mean tail (mq_pool_wide): a column's mean is a first-to-last sum of len terms and one division: |dm| <= (len + 1) u mean_t |x_t| =: Bm.  With L2:
      y = m / n, n = ||m||; the sum of squares runs over 16 terms per thread, six butterfly levels and three adds across the waves (chain 25, halved by
      the square root), plus the square root, the reciprocal and the product: |dy| <= Bm / n + |y| ||Bm|| / n + |y| (25 / 2 + 4) u.
  last tail (mq_last_rows, mq_rmsnorm_wide through the row index, mq_l2_normalize — the calls mq_encode_llama makes): with B the rmsnorm budget of the
      row y and n = ||y||: |dz| <= B / n + |z| ||B|| / n + |z| (D / 2 + 4) u (mq_l2_normalize sums W / 64 terms per lane and six levels: within D).

Measured values are printed as `LLAMA_RATIO` lines."""
import numpy as np
import pytest
import torch

from marqo_amd import _lib as L
from tests import rowops_ref as RR

pytestmark = pytest.mark.gpu

MARGIN = 1.25
U = 2.0 ** -24
EPS = 1e-5


@pytest.fixture(scope="module")
def lib():
    return L.load()


def _s():
    return torch.cuda.current_stream().cuda_stream


def _cu(lens):
    return torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32, device="cuda")


@pytest.mark.parametrize("W", (64, 2048, 2112, 2560, 4096))
@pytest.mark.parametrize("rows", (1, 67))
def test_rmsnorm_wide_against_float64(lib, W, rows):
    for fam in ("randn", "rowscale"):
        x, g, _ = RR.make_rows(fam, 80, W, seed=3, device="cuda")
        for idx in (None, torch.randperm(80, device="cuda")[:rows].to(torch.int32)):
            xs = x[:rows] if idx is None else x[idx.long()]
            y = xs.double() * torch.rsqrt(xs.double().pow(2).mean(-1, keepdim=True) + EPS) * g.double()
            B = y.abs() * (RR.chain(W) / 2 + 7) * U
            ob = torch.full((rows + 2, W), float("nan"), dtype=torch.bfloat16, device="cuda")
            of = torch.full((rows + 2, W), float("nan"), dtype=torch.float32, device="cuda")
            L.check(lib.mq_rmsnorm_wide(x.data_ptr(), L.ptr(idx), g.data_ptr(), ob[1:].data_ptr(), of[1:].data_ptr(), rows, W, EPS, _s()), "mq_rmsnorm_wide")
            torch.cuda.synchronize()
            assert bool(ob[0].isnan().all()) and bool(ob[-1].isnan().all()) and bool(of[0].isnan().all()) and bool(of[-1].isnan().all())
            rf, rb = RR.ratio(of[1:-1], y, B), RR.ratio(ob[1:-1], y, B + RR.half_ulp_bf16(y))
            print(f"LLAMA_RATIO rmsnorm_wide family={fam} rows={rows} W={W} gather={idx is not None} fp32_out={rf:.4f} bf16_out={rb:.4f}")
            assert rf <= MARGIN and rb <= MARGIN
            # either output alone, and in place on the fp32 rows (the tower's mean-pooling tail)
            only = torch.empty(rows, W, dtype=torch.float32, device="cuda")
            L.check(lib.mq_rmsnorm_wide(x.data_ptr(), L.ptr(idx), g.data_ptr(), None, only.data_ptr(), rows, W, EPS, _s()), "mq_rmsnorm_wide")
            assert torch.equal(only, of[1:-1])
            onlyb = torch.empty(rows, W, dtype=torch.bfloat16, device="cuda")
            L.check(lib.mq_rmsnorm_wide(x.data_ptr(), L.ptr(idx), g.data_ptr(), onlyb.data_ptr(), None, rows, W, EPS, _s()), "mq_rmsnorm_wide")
            assert torch.equal(onlyb.view(torch.int16), ob[1:-1].view(torch.int16))
            if idx is None:
                inplace = x[:rows].clone()
                L.check(lib.mq_rmsnorm_wide(inplace.data_ptr(), None, g.data_ptr(), None, inplace.data_ptr(), rows, W, EPS, _s()), "mq_rmsnorm_wide")
                assert torch.equal(inplace, of[1:-1])
            if W <= 2048:       # the narrow entry point's bits
                nf = torch.empty(rows, W, dtype=torch.float32, device="cuda")
                nb = torch.empty(rows, W, dtype=torch.bfloat16, device="cuda")
                L.check(lib.mq_rmsnorm(x.data_ptr(), L.ptr(idx), g.data_ptr(), nb.data_ptr(), nf.data_ptr(), rows, W, EPS, _s()), "mq_rmsnorm")
                assert torch.equal(nf, of[1:-1]) and torch.equal(nb.view(torch.int16), ob[1:-1].view(torch.int16))


@pytest.mark.parametrize("W", (2048, 2112, 4096))
def test_wide_token_gather_is_exact(lib, W):
    vocab, lens = 50, [1, 17, 70, 5]
    g = torch.Generator().manual_seed(W)
    table = torch.randn(vocab, W, generator=g).to("cuda")
    ids = torch.randint(0, vocab, (sum(lens),), generator=g).to(torch.int32)
    ids[0], ids[1], ids[5], ids[-1] = 0, vocab - 1, vocab - 1, 0
    ids = ids.to("cuda")
    x = torch.full((sum(lens) + 2, W), float("nan"), device="cuda")
    L.check(lib.mq_embed_tokens_wide(ids.data_ptr(), _cu(lens).data_ptr(), len(lens), table.data_ptr(), x[1:].data_ptr(), W, vocab, _s()), "mq_embed_tokens_wide")
    torch.cuda.synchronize()
    assert bool(x[0].isnan().all()) and bool(x[-1].isnan().all())
    assert torch.equal(x[1:-1], table[ids.long()])
    # ids outside the table are clamped to it, as mq_embed_tokens clamps them
    wild = ids.clone()
    wild[2], wild[3] = -7, vocab + 9
    L.check(lib.mq_embed_tokens_wide(wild.data_ptr(), _cu(lens).data_ptr(), len(lens), table.data_ptr(), x[1:].data_ptr(), W, vocab, _s()), "mq_embed_tokens_wide")
    assert torch.equal(x[1:-1], table[wild.long().clamp(0, vocab - 1)])


@pytest.mark.parametrize("W", (2048, 2112, 4096))
@pytest.mark.parametrize("normalize", (True, False))
def test_mean_tail_against_float64(lib, W, normalize):
    lens = [1, 17, 70]
    for fam in ("randn", "rowscale"):
        x, _, _ = RR.make_rows(fam, sum(lens), W, seed=5, device="cuda")
        cu = _cu(lens)
        out = torch.full((len(lens) + 2, W), float("nan"), device="cuda")
        L.check(lib.mq_pool_wide(x.data_ptr(), cu.data_ptr(), len(lens), out[1:].data_ptr(), W, int(normalize), _s()), "mq_pool_wide")
        torch.cuda.synchronize()
        assert bool(out[0].isnan().all()) and bool(out[-1].isnan().all())
        parts = x.double().split(lens)
        m = torch.stack([p.mean(0) for p in parts])
        Bm = torch.stack([(len(p) + 1) * U * p.abs().mean(0) for p in parts])
        if normalize:
            n = m.norm(dim=-1, keepdim=True)
            ref = m / n
            B = Bm / n + ref.abs() * Bm.norm(dim=-1, keepdim=True) / n + ref.abs() * (25 / 2 + 4) * U
        else:
            ref, B = m, Bm
        r = RR.ratio(out[1:-1], ref, B)
        print(f"LLAMA_RATIO mean_tail family={fam} W={W} normalize={normalize} ratio={r:.4f}")
        assert r <= MARGIN
        if W <= 2048:       # the narrow entry point's bits
            narrow = torch.empty(len(lens), W, device="cuda")
            L.check(lib.mq_pool(x.data_ptr(), cu.data_ptr(), len(lens), narrow.data_ptr(), W, L.MQ_POOL_MEAN, int(normalize), _s()), "mq_pool")
            assert torch.equal(narrow, out[1:-1])


@pytest.mark.parametrize("W", (2112, 4096))
@pytest.mark.parametrize("normalize", (True, False))
def test_last_tail_against_float64(lib, W, normalize):
    """the calls mq_encode_llama makes under MQ_POOL_LAST: the last row of every sequence through the row index, normalised alone, then L2"""
    lens = [1, 17, 70]
    for fam in ("randn", "rowscale"):
        x, g, _ = RR.make_rows(fam, sum(lens), W, seed=6, device="cuda")
        cu = _cu(lens)
        last = torch.full((len(lens),), -1, dtype=torch.int32, device="cuda")
        out = torch.full((len(lens) + 2, W), float("nan"), device="cuda")
        L.check(lib.mq_last_rows(cu.data_ptr(), last.data_ptr(), len(lens), _s()), "mq_last_rows")
        L.check(lib.mq_rmsnorm_wide(x.data_ptr(), last.data_ptr(), g.data_ptr(), None, out[1:].data_ptr(), len(lens), W, EPS, _s()), "mq_rmsnorm_wide")
        if normalize:
            L.check(lib.mq_l2_normalize(out[1:].data_ptr(), out[1:].data_ptr(), len(lens), W, _s()), "mq_l2_normalize")
        torch.cuda.synchronize()
        assert last.tolist() == [0, 17, 87] and bool(out[0].isnan().all()) and bool(out[-1].isnan().all())
        xs = x[last.long()].double()
        y = xs * torch.rsqrt(xs.pow(2).mean(-1, keepdim=True) + EPS) * g.double()
        B = y.abs() * (RR.chain(W) / 2 + 7) * U
        if normalize:
            n = y.norm(dim=-1, keepdim=True)
            ref = y / n
            B = B / n + ref.abs() * B.norm(dim=-1, keepdim=True) / n + ref.abs() * (RR.chain(W) / 2 + 4) * U
        else:
            ref = y
        r = RR.ratio(out[1:-1], ref, B)
        print(f"LLAMA_RATIO last_tail family={fam} W={W} normalize={normalize} ratio={r:.4f}")
        assert r <= MARGIN

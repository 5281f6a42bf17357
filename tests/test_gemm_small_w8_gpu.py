"""mq_gemm_small_w8 and mq_quantize_weights_pow2 (csrc/gemm_small_w8.hip) through torch.ops.marqo_hip: every code's decode bit for bit; parity against float64
under tests/gemm_ref.py's per-element budget (`reference` takes the dequantised weight as its bf16 W, which it is exactly) and that family's bar; the quantiser
against tests/w8_ref.py; the refusals."""
import pytest
import torch

from marqo_amd import _lib as L
from tests import gemm_ref as G
from tests import w8_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MARGIN = 1.25     # tests/test_gemm_parity_gpu.py
EPILOGUES = (0, G.BIAS, G.BIAS | G.RES | G.F32)


@pytest.fixture(scope="module")
def ops():
    return L.load_torch_ops()


@pytest.mark.parametrize("k0", (0, 9, 63))   # the first half-fragment, the second half-fragment, the last lane group
def test_every_code_decodes_exactly(ops, k0):
    codes = torch.arange(256, dtype=torch.uint8)
    codes[0x7f] = codes[0xff] = 0
    scale = torch.tensor([2.0 ** -9, 1.0, 2.0 ** 3]).repeat(86)[:256]
    A = torch.zeros(1, 64, dtype=torch.bfloat16)
    A[0, k0] = 1.0
    out = ops.mq_gemm_small_w8(A.to(DEV), codes[:, None].repeat(1, 64).contiguous().to(DEV), scale.to(DEV), None, None, 0).cpu()
    # the row's one non-zero product, as the float64 sum gives it (code 0x80: -0 + 0 = +0, as in any GEMM), rounded to bf16
    want = (A.double() @ (R.TABLE[codes.long()] * scale.double())[:, None].repeat(1, 64).t()).to(torch.bfloat16)
    bad = (out.view(torch.int16) != want.view(torch.int16)).nonzero()
    assert bad.numel() == 0, f"code {int(bad[0, 1]):#x}: got {float(out[0, bad[0, 1]])!r} want {float(want[0, bad[0, 1]])!r}"


@pytest.mark.parametrize("K", (64, 192, 1024))            # fewer chunks than waves, chunks ragged over the waves, a long walk
@pytest.mark.parametrize("M", (1, 17, 80, 81, 161))       # one row, a ragged second tile, the top of one group, the first grouped call, a ragged group
def test_parity_against_float64(ops, M, K):
    for N in (4, 16, 132):                                # a guarded slice, one full slice, a ragged last slice
        c = G.rand_case(G.family_for(M, N, K), M, N, K, device=DEV)
        codes, scale, deq = R.quantize(c["W"])
        c["W"] = deq.to(DEV)
        for flags in EPILOGUES:
            got = ops.mq_gemm_small_w8(c["A"], codes.to(DEV), scale.to(DEV), c["bias"] if flags & G.BIAS else None, c["res"] if flags & G.RES else None, flags)
            r = G.reference(flags, c)
            worst = G.ratio(got, r["ref"], r["bound"])
            print(f"W8_PARITY M={M} N={N} K={K} flags={flags:#x} ratio={worst:.3f}")
            assert worst <= MARGIN, G.worst(got, r)


def test_quantiser_matches_the_python_restatement(ops):
    g = torch.Generator().manual_seed(3)
    W = (torch.randn(7, 192, generator=g) * 0.05).to(torch.bfloat16)
    W[1] = 0                                   # an all-zero row
    W[2, 5] = 448.0 * 2.0 ** -6                # absmax exactly 448 x 2^k
    W[3, 100] = 300.0                          # an outlier: the rest of the row falls into the subnormal codes
    W[4, 0] = -450.0 * 2.0 ** -6               # the next bf16 past that edge: the next scale
    codes, scale, deq = R.quantize(W)
    Wd = W.to(DEV)
    got8, gots = ops.mq_quantize_weights_pow2(Wd)
    assert torch.equal(gots.cpu(), scale), (gots.cpu(), scale)
    assert torch.equal(got8.cpu(), codes), (got8.cpu() != codes).nonzero()[:4]
    assert torch.equal(Wd.cpu().view(torch.int16), deq.view(torch.int16))


def test_refusals():
    lib, fake = L.load(), 256     # (a non-null operand address: never dereferenced, the argument check fails first)
    assert lib.mq_gemm_small_w8(fake, 96, fake, 96, fake, None, None, fake, 16, 1, 16, 96, 0, None) == -1
    assert b"mq_gemm_small_w8: K=96 must be a multiple of 64" in lib.mq_last_error()
    assert lib.mq_gemm_small_w8(fake, 64, fake, 64, fake, fake, None, fake, 16, 1, 16, 64, L.MQ_EPI_BIAS | L.MQ_EPI_GELU, None) == -1
    assert b"mq_gemm_small_w8: unsupported epilogue flag combination" in lib.mq_last_error()
    assert lib.mq_gemm_small_w8_ok(80, 16, 64) == 1 and lib.mq_gemm_small_w8_ok(80, 16, 96) == 0 and lib.mq_gemm_small_w8_ok(100000, 16, 64) == 0

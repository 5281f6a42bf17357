"""mq_gemm_w4 (csrc/gemm_w4.hip: the tiled MXFP4 W4A16 GEMM) through torch.ops.marqo_hip: every code's decode bit for bit under three block scales;
parity against float64 under tests/gemm_ref.py's per-element budget on weights whose blocks carry different scales inside a row, at the edges of the
128 x 256 tile and of the three-stage ring; a row's bits whatever the call it stands in; the refusals."""
import pytest
import torch

from marqo_amd import _lib as L
from tests import gemm_ref as G
from tests import w4_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MARGIN = 1.25     # tests/test_gemm_parity_gpu.py
BM, BN = 128, 256  # the kernel's tile (8 waves x 32 columns against 8 row tiles)
EPILOGUES = (0, G.BIAS, G.BIAS | G.RES | G.F32)


@pytest.fixture(scope="module")
def ops():
    return L.load_torch_ops()


def quantised_case(ops, M, N, K):
    """a random case whose weight has block magnitudes over seven octaves inside every row, its codes and scales; c["W"] is the dequantised weight"""
    c = G.rand_case(G.family_for(M, N, K), M, N, K, device=DEV)
    octave = (torch.arange(N)[:, None] + 3 * torch.arange(K // 32)[None, :]) % 7 - 3
    Wd = (c["W"].cpu().float().view(N, K // 32, 32) * torch.pow(2.0, octave)[:, :, None]).view(N, K).to(torch.bfloat16).to(DEV)
    w4, sc = ops.mq_quantize_weights_mxfp4(Wd)
    c["W"] = Wd
    return c, w4, sc


# the probe positions of tests/test_gemm_small_w4_gpu.py (every nibble position of the storage, the second chunk's padded half included)
@pytest.mark.parametrize("k0", (0, 5, 31, 42, 127, 163))
def test_every_code_decodes_exactly(ops, k0):
    K, scales = 192, (2.0 ** -100, 1.0, 2.0 ** 100)
    code = torch.arange(16).repeat_interleave(3)
    s = torch.tensor(scales, dtype=torch.float64).repeat(16)
    W = (torch.where(code >= 8, -1.0, 1.0) * R.GRID[code % 8] * s)[:, None].repeat(1, K)
    W[:, (k0 + 16) % 32::32] = 6.0 * s[:, None]            # one full-scale element per block, away from the probe, pins the block's scale to s
    W = W.to(torch.bfloat16)
    A = torch.zeros(1, K, dtype=torch.bfloat16)
    A[0, k0] = 1.0
    w4, sc = ops.mq_quantize_weights_mxfp4(W.to(DEV))
    out = ops.mq_gemm_w4(A.to(DEV), w4, sc, None, None, 0).cpu()
    want = (A.double() @ W.double().t()).to(torch.bfloat16)
    bad = (out.view(torch.int16) != want.view(torch.int16)).nonzero()
    assert bad.numel() == 0, f"row {int(bad[0, 1])} (code {int(code[bad[0, 1]])}): got {float(out[0, bad[0, 1]])!r} want {float(want[0, bad[0, 1]])!r}"


@pytest.mark.parametrize("flags", EPILOGUES)
@pytest.mark.parametrize("K", (64, 192, 1024))                        # half a chunk; a ragged last chunk, fewer chunks than ring stages; a walk that wraps the ring
@pytest.mark.parametrize("M", (1, BM - 1, BM + 1, 2 * BM + 17))      # one row, each side of a tile edge, a ragged third tile row
def test_parity_against_float64(ops, M, K, flags):
    for N in (4, BN - 4, BN + 4):                                     # one guarded slice, a nearly full tile, a ragged second tile column
        c, w4, sc = quantised_case(ops, M, N, K)
        got = ops.mq_gemm_w4(c["A"], w4, sc, c["bias"] if flags & G.BIAS else None, c["res"] if flags & G.RES else None, flags)
        r = G.reference(flags, c)
        worst = G.ratio(got, r["ref"], r["bound"])
        print(f"W4_TILED_PARITY M={M} N={N} K={K} flags={flags:#x} ratio={worst:.3f}")
        assert worst <= MARGIN, G.worst(got, r)


def test_a_rows_bits_do_not_depend_on_the_call(ops):
    M, row = 2 * BM + 17, BM + 3
    c, w4, sc = quantised_case(ops, M, BN + 4, 1024)
    whole = ops.mq_gemm_w4(c["A"], w4, sc, None, None, 0)[row].cpu()
    alone = ops.mq_gemm_w4(c["A"][row:row + 1].contiguous(), w4, sc, None, None, 0)[0].cpu()
    assert torch.equal(whole.view(torch.int16), alone.view(torch.int16))


def test_refusals():
    lib, fake = L.load(), 256     # (a non-null operand address: never dereferenced, the argument check fails first)
    assert lib.mq_gemm_w4(fake, 96, fake, 64, fake, 4, None, None, fake, 16, 1, 16, 96, 0, None) == -1
    assert b"mq_gemm_w4: K=96 must be a multiple of 64" in lib.mq_last_error()
    assert lib.mq_gemm_w4(fake, 64, fake, 64, fake, 4, fake, None, fake, 16, 1, 16, 64, L.MQ_EPI_BIAS | L.MQ_EPI_GELU, None) == -1
    assert b"mq_gemm_w4: unsupported epilogue flag combination" in lib.mq_last_error()
    assert lib.mq_gemm_w4(fake, 192, fake, 96, fake, 8, None, None, fake, 16, 1, 16, 192, 0, None) == -1
    assert b"mq_gemm_w4: ld4=96 must be a multiple of 16 and at least 128" in lib.mq_last_error()

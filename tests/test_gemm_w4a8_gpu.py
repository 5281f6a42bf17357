"""mq_quantize_rows_mxfp8 + mq_gemm_w4a8 (csrc/gemm_w4a8.hip: MXFP8 activations x MXFP4 weights on the MX matrix instruction) through
torch.ops.marqo_hip: the quantiser bit for bit through an identity weight; every weight position, code and scale bit for bit through identity
activations; parity against float64 on the dequantised operands under tests/gemm_ref.py's per-element budget at the edges of the 128 x 256 tile and
of the three-stage ring; a row's bits whatever the call it stands in; the refusals.

Parity, measured on an MI355X: under an fp32 sum's budget (c_acc = 1) the worst ratio was 44.3 (K = 64, M = 273, N = 260, fp32 out) while both
bit-for-bit tests passed: the instruction's 128-deep sum is not an fp32 sum; its error stayed near 2^-13 of the sum of magnitudes whatever K (smallest
passing integer c_acc: 46 at K = 64, 7 at 192, 2 at 1024).  C_ACC = 46 is the smallest integer with every ratio <= 1.0; MARGIN is the siblings'"""
import pytest
import torch

from marqo_amd import _lib as L
from tests import a8_ref as R8
from tests import gemm_ref as G
from tests.test_gemm_w4_gpu import BM, BN, EPILOGUES, MARGIN, quantised_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C_ACC = 46     # measured: the docstring


@pytest.fixture(scope="module")
def ops():
    return L.load_torch_ops()


def bits(t):
    return (t.cpu().double() + 0.0).to(torch.bfloat16).view(torch.int16)     # (a GEMM's sum starts at +0: a -0 operand comes back as +0)


def a8_gemm(ops, A, w4, sc, bias=None, res=None, flags=0):
    return ops.mq_gemm_w4a8(ops.mq_quantize_rows_mxfp8(A), A.shape[0], A.shape[1], w4, sc, bias, res, flags)


@pytest.mark.parametrize("K", (64, 192))     # half a chunk; a whole chunk and a half one, whose padding is read
def test_the_quantiser_bit_for_bit(ops, K):
    g = torch.Generator().manual_seed(K)
    A = torch.randn(6, K // 32, 32, generator=g) * torch.pow(2.0, torch.randint(-12, 13, (6, K // 32, 1), generator=g).float())   # octaves inside a row
    A[1, 0] = 0.0                                                        # an all-zero block
    small = torch.rand(32, generator=g) * 2 - 1
    for row, k in ((2, -9), (3, 0), (4, 5)):                             # absmax exactly at 448 x 2^k, and one bf16 step above it (450 x 2^k)
        A[row, 0], A[row, 1] = small * 2.0 ** k, small * 2.0 ** k
        A[row, 0, 5], A[row, 1, 20] = 448.0 * 2.0 ** k, -450.0 * 2.0 ** k
    A[5, 0] = 0.0                                                        # e4m3 subnormals (steps of 2^-9 under a unit scale), ties among them
    A[5, 0, :9] = torch.tensor([448.0, 2.0 ** -7, 2.0 ** -9, 3 * 2.0 ** -10, 2.0 ** -10, 5 * 2.0 ** -10, -7 * 2.0 ** -9, 2.0 ** -11, 1.75 * 2.0 ** -6])
    A = A.view(6, K).to(torch.bfloat16)
    scale, deq = R8.quantize(A)
    assert scale[1:6, 0].tolist() == [127, 118, 127, 132, 127] and scale[2:5, 1].tolist() == [119, 128, 133]
    w4, sc = ops.mq_quantize_weights_mxfp4(torch.eye(K, dtype=torch.bfloat16, device=DEV))
    got = a8_gemm(ops, A.to(DEV), w4, sc)
    bad = (bits(got) != bits(deq)).nonzero()
    assert bad.numel() == 0, f"{len(bad)} differ, first (row {int(bad[0, 0])}, k {int(bad[0, 1])}): got {float(got[tuple(bad[0])])!r} want {float(deq[tuple(bad[0])])!r}"


def test_every_weight_position_code_and_scale_exact(ops):
    K, N = 192, BN + 4
    c, w4, sc = quantised_case(ops, 1, N, K)
    got = a8_gemm(ops, torch.eye(K, dtype=torch.bfloat16, device=DEV), w4, sc)
    bad = (bits(got) != bits(c["W"].t())).nonzero()
    assert bad.numel() == 0, f"{len(bad)} differ, first (k {int(bad[0, 0])}, n {int(bad[0, 1])})"


@pytest.mark.parametrize("flags", EPILOGUES)
@pytest.mark.parametrize("K", (64, 192, 1024))                        # half a chunk; a ragged last chunk, fewer chunks than ring stages; a walk that wraps the ring
@pytest.mark.parametrize("M", (1, BM - 1, BM + 1, 2 * BM + 17))      # one row, each side of a tile edge, a ragged third tile row
def test_parity_against_float64_of_the_dequantised_operands(ops, M, K, flags):
    for N in (4, BN - 4, BN + 4):                                     # one guarded slice, a nearly full tile, a ragged second tile column
        c, w4, sc = quantised_case(ops, M, N, K)
        got = a8_gemm(ops, c["A"], w4, sc, c["bias"] if flags & G.BIAS else None, c["res"] if flags & G.RES else None, flags)
        c["A"] = R8.quantize(c["A"])[1].to(DEV)
        r = G.reference(flags, c, c_acc=C_ACC)
        worst = G.ratio(got, r["ref"], r["bound"])
        print(f"W4A8_PARITY M={M} N={N} K={K} flags={flags:#x} ratio={worst:.3f}")
        assert worst <= MARGIN, G.worst(got, r)


def test_a_rows_bits_do_not_depend_on_the_call(ops):
    M, row = 2 * BM + 17, BM + 3
    c, w4, sc = quantised_case(ops, M, BN + 4, 1024)
    whole = a8_gemm(ops, c["A"], w4, sc)[row].cpu()
    alone = a8_gemm(ops, c["A"][row:row + 1].contiguous(), w4, sc)[0].cpu()
    assert torch.equal(whole.view(torch.int16), alone.view(torch.int16))


def test_refusals():
    lib, fake = L.load(), 256     # (a non-null operand address: never dereferenced, the argument check fails first)
    assert lib.mq_gemm_w4a8(fake, 128, fake, 64, fake, 4, None, None, fake, 16, 1, 16, 96, 0, None) == -1
    assert b"mq_gemm_w4a8: K=96 must be a multiple of 64" in lib.mq_last_error()
    assert lib.mq_gemm_w4a8(fake, 128, fake, 64, fake, 4, fake, None, fake, 16, 1, 16, 64, L.MQ_EPI_BIAS | L.MQ_EPI_GELU, None) == -1
    assert b"mq_gemm_w4a8: unsupported epilogue flag combination" in lib.mq_last_error()
    assert lib.mq_gemm_w4a8(fake, 256, fake, 96, fake, 8, None, None, fake, 16, 1, 16, 192, 0, None) == -1
    assert b"mq_gemm_w4a8: ld4=96 must be a multiple of 16 and at least 128" in lib.mq_last_error()
    assert lib.mq_gemm_w4a8(fake, 192, fake, 128, fake, 8, None, None, fake, 16, 1, 16, 192, 0, None) == -1
    assert b"mq_gemm_w4a8: ld8=192 must be a multiple of 16 and at least 256" in lib.mq_last_error()

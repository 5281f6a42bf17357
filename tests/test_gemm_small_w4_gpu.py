"""mq_gemm_small_w4 and mq_quantize_weights_mxfp4 (csrc/gemm_small_w4.hip) through torch.ops.marqo_hip: every code's decode bit for bit under three block
scales; parity against float64 under tests/gemm_ref.py's per-element budget (`reference` takes the dequantised weight as its bf16 W, which it is exactly) and
that family's bar, on weights whose blocks carry different scales inside a row; the quantiser against tests/w4_ref.py; the refusals."""
import pytest
import torch

from marqo_amd import _lib as L
from tests import gemm_ref as G
from tests import w4_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MARGIN = 1.25     # tests/test_gemm_parity_gpu.py
EPILOGUES = (0, G.BIAS, G.BIAS | G.RES | G.F32)


@pytest.fixture(scope="module")
def ops():
    return L.load_torch_ops()


# The kernel's layout: k = chunk 128 + block 32 + lane group 8 + e; the codes e = 0 .. 3 sit in the low nibbles of a dword's bytes 0 .. 3, e = 4 .. 7 in the
# high nibbles.  0: first block, first lane group, low nibble of byte 0;  5: high nibble of byte 1;  31: last lane group, high nibble of the last byte;
# 42: second block of the chunk, lane group 1, low nibble;  127: last block, last lane group;  163: the padded half chunk, its second block, low nibble of byte 3.
@pytest.mark.parametrize("k0", (0, 5, 31, 42, 127, 163))
def test_every_code_decodes_exactly(ops, k0):
    K, scales = 192, (2.0 ** -100, 1.0, 2.0 ** 100)       # 0.5 x 2^-100 is the smallest value the clamped format holds, 6 x 2^100 the largest
    code = torch.arange(16).repeat_interleave(3)
    s = torch.tensor(scales, dtype=torch.float64).repeat(16)
    value = torch.where(code >= 8, -1.0, 1.0) * R.GRID[code % 8] * s
    W = value[:, None].repeat(1, K)
    W[:, (k0 + 16) % 32::32] = 6.0 * s[:, None]            # one full-scale element per block, away from the probe, pins the block's scale to s
    W = W.to(torch.bfloat16)
    A = torch.zeros(1, K, dtype=torch.bfloat16)
    A[0, k0] = 1.0
    Wd = W.to(DEV)
    w4, sc = ops.mq_quantize_weights_mxfp4(Wd)
    assert torch.equal(Wd.cpu().view(torch.int16), W.view(torch.int16))                       # every value is on the grid: the rewrite changes no bit (-0 included)
    assert torch.equal(sc.cpu()[:, :K // 32].double(), (127 + torch.log2(s))[:, None].repeat(1, K // 32))
    out = ops.mq_gemm_small_w4(A.to(DEV), w4, sc, None, None, 0).cpu()
    want = (A.double() @ W.double().t()).to(torch.bfloat16)      # the row's one non-zero product as the float64 sum gives it (code 8: -0 + 0 = +0, as in any GEMM)
    bad = (out.view(torch.int16) != want.view(torch.int16)).nonzero()
    assert bad.numel() == 0, f"row {int(bad[0, 1])} (code {int(code[bad[0, 1]])}): got {float(out[0, bad[0, 1]])!r} want {float(want[0, bad[0, 1]])!r}"


@pytest.mark.parametrize("K", (64, 192, 1024))            # half a chunk, a ragged last chunk and fewer chunks than waves, a long walk
@pytest.mark.parametrize("M", (1, 17, 80, 81, 161))       # one row, a ragged second tile, the top of one group, the first grouped call, a ragged group
def test_parity_against_float64(ops, M, K):
    for N in (4, 16, 132):                                # a guarded slice, one full slice, a ragged last slice
        c = G.rand_case(G.family_for(M, N, K), M, N, K, device=DEV)
        octave = (torch.arange(N)[:, None] + 3 * torch.arange(K // 32)[None, :]) % 7 - 3      # block magnitudes over seven octaves inside every row
        W = (c["W"].cpu().float().view(N, K // 32, 32) * torch.pow(2.0, octave)[:, :, None]).view(N, K).to(torch.bfloat16)
        Wd = W.to(DEV)
        w4, sc = ops.mq_quantize_weights_mxfp4(Wd)
        assert len(set(sc.cpu()[0, :K // 32].tolist())) > 1
        c["W"] = Wd                                       # the dequantised weight
        for flags in EPILOGUES:
            got = ops.mq_gemm_small_w4(c["A"], w4, sc, c["bias"] if flags & G.BIAS else None, c["res"] if flags & G.RES else None, flags)
            r = G.reference(flags, c)
            worst = G.ratio(got, r["ref"], r["bound"])
            print(f"W4_PARITY M={M} N={N} K={K} flags={flags:#x} ratio={worst:.3f}")
            assert worst <= MARGIN, G.worst(got, r)


def test_quantiser_matches_the_python_restatement(ops):
    g = torch.Generator().manual_seed(3)
    W = (torch.randn(8, 192, generator=g) * 0.01 * torch.pow(2.0, torch.arange(8.0))[:, None]).to(torch.bfloat16)
    W[1, 0:32] = 0                                        # an all-zero block
    W[2:4, 32:96] = W[0, 32:96] * 0.25                    # (two quiet blocks for the edges below)
    W[2, 32 + 5] = 6.0 * 2.0 ** -6                        # a block whose absmax is exactly 6 x 2^k
    W[3, 64 + 9] = -6.03125 * 2.0 ** -6                   # the next bf16 past that edge: the next scale
    W[4, 100] = 300.0                                     # an outlier: the rest of its block falls to 0 / 0.5
    W[5, 160:176] = torch.tensor([6.0, 2.5, -2.5, 0.25, 1.25, 1.75, 3.5, 5.0, 0.75, -0.25, 4.5, -5.0, 2.25, 2.75, -0.0, 0.0]).to(torch.bfloat16)   # scale 1: exact ties
    codes, scale, deq = R.quantize(W)
    assert [float(v) for v in deq[5, 160:170]] == [6.0, 2.0, -2.0, 0.0, 1.0, 2.0, 4.0, 4.0, 1.0, -0.0] and int(scale[5, 5]) == 127
    Wd = W.to(DEV)
    w4, sc = ops.mq_quantize_weights_mxfp4(Wd)
    assert torch.equal(sc.cpu()[:, :6], scale), (sc.cpu()[:, :6], scale)
    assert torch.equal(Wd.cpu().view(torch.int16), deq.view(torch.int16)), (Wd.cpu().view(torch.int16) != deq.view(torch.int16)).nonzero()[:4]
    # the packed codes, as the kernel reads them: an identity A returns decode(code) x scale of every element
    seen = ops.mq_gemm_small_w4(torch.eye(192, dtype=torch.bfloat16, device=DEV), w4, sc, None, None, 0).cpu().double().t()
    want = torch.where(codes >= 8, -1.0, 1.0) * R.GRID[(codes % 8).long()] * torch.pow(2.0, scale.double() - 127).repeat_interleave(32, dim=1)
    assert torch.equal(seen, want), (seen != want).nonzero()[:4]


def test_refusals():
    lib, fake = L.load(), 256     # (a non-null operand address: never dereferenced, the argument check fails first)
    assert lib.mq_gemm_small_w4(fake, 96, fake, 64, fake, 4, None, None, fake, 16, 1, 16, 96, 0, None) == -1
    assert b"mq_gemm_small_w4: K=96 must be a multiple of 64" in lib.mq_last_error()
    assert lib.mq_gemm_small_w4(fake, 64, fake, 64, fake, 4, fake, None, fake, 16, 1, 16, 64, L.MQ_EPI_BIAS | L.MQ_EPI_GELU, None) == -1
    assert b"mq_gemm_small_w4: unsupported epilogue flag combination" in lib.mq_last_error()
    assert lib.mq_gemm_small_w4(fake, 192, fake, 96, fake, 8, None, None, fake, 16, 1, 16, 192, 0, None) == -1
    assert b"mq_gemm_small_w4: ld4=96 must be a multiple of 16 and at least 128" in lib.mq_last_error()
    assert lib.mq_gemm_small_w4_ok(80, 16, 64) == 1 and lib.mq_gemm_small_w4_ok(80, 16, 96) == 0 and lib.mq_gemm_small_w4_ok(100000, 16, 64) == 0

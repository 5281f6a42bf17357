"""The MXFP8 activation format in plain Python (csrc/gemm_w4a8.hip states it; nothing here calls the library): e4m3fn codes, one e8m0 power-of-two
scale per block of 32 consecutive k.  Values only: how the library orders the bytes is its own business.  tests/test_gemm_w4a8_gpu.py."""
import torch

from tests.w8_ref import TABLE

BLOCK = 32


def scale_exponents(absmax: torch.Tensor) -> torch.Tensor:
    """ceil(log2(absmax / 448)), 0 for 0, kept inside [-100, 100]; through frexp: absmax = f 2^e, f in [0.5, 1), and 448 = 0.875 x 2^9"""
    f, e = torch.frexp(absmax.double())
    return torch.where(absmax == 0, 0, torch.where(f <= 0.875, e - 9, e - 8).clamp(-100, 100))


def quantize(A: torch.Tensor):
    """A bf16 [M, K], K % 32 == 0 -> (e8m0 scale bytes uint8 [M, K / 32], dequantised bf16 [M, K] = decode(code) x scale, exact), on the CPU"""
    A = A.detach().cpu()
    M, K = A.shape
    blocks = A.double().view(M, K // BLOCK, BLOCK)
    ex = scale_exponents(blocks.abs().amax(dim=2))
    scale = torch.pow(2.0, ex.double())[:, :, None]
    codes = (blocks / scale).float().to(torch.float8_e4m3fn).view(torch.uint8)      # (a division by a power of two: exact; the cast is RNE)
    deq = TABLE[codes.long()] * scale
    assert bool(torch.isfinite(deq).all()) and torch.equal(deq.to(torch.bfloat16).double(), deq)
    return (ex + 127).to(torch.uint8), deq.view(M, K).to(torch.bfloat16)

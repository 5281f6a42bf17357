"""The MXFP4 weight format in plain Python (csrc/gemm_small_w4.hip states it; nothing here calls the library): the e2m1 grid, the e8m0 block scale, the
quantiser.  Values only: how the library packs codes into bytes is its own business.  tests/test_gemm_small_w4_gpu.py, tests/test_llama_w4_gpu.py,
tests/test_weight_precision_mxfp4_host.py."""
import math

import torch

BLOCK = 32
GRID = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], dtype=torch.float64)     # magnitude index 0 .. 7 = the code's e.e.m bits; bit 3 is the sign


def scale_exponent(absmax: float) -> int:
    """ceil(log2(absmax / 6)), 0 for 0, kept inside [-100, 100]; through frexp: absmax = f 2^e, f in [0.5, 1), and 6 = 0.75 x 2^3"""
    if absmax == 0:
        return 0
    f, e = math.frexp(absmax)
    return min(max(e - 3 if f <= 0.75 else e - 2, -100), 100)


def quantize(W: torch.Tensor):
    """W bf16 [N, K], K % 32 == 0 -> (codes uint8 [N, K] in 0 .. 15, e8m0 scale bytes uint8 [N, K / 32], dequantised bf16 [N, K] = decode x scale, exact),
    on the CPU.  Round to nearest grid point; of two equally near ones, the one with the even index (mantissa bit 0)."""
    W = W.detach().cpu()
    N, K = W.shape
    blocks = W.double().view(N, K // BLOCK, BLOCK)
    ex = torch.tensor([[scale_exponent(float(v)) for v in row] for row in blocks.abs().amax(dim=2)], dtype=torch.float64)
    scale = torch.pow(2.0, ex)[:, :, None]
    dist = ((blocks.abs() / scale)[..., None] - GRID).abs()                  # (a division by a power of two: exact)
    nearest = dist == dist.amin(dim=-1, keepdim=True)
    index = (nearest * (2 - torch.arange(8) % 2)).argmax(dim=-1)             # a tie is between neighbours: the even one scores 2, the odd one 1
    deq = torch.where(torch.signbit(blocks), -1.0, 1.0) * GRID[index] * scale
    assert bool(torch.isfinite(deq).all()) and torch.equal(deq.to(torch.bfloat16).double(), deq)
    codes = (index + 8 * torch.signbit(blocks)).to(torch.uint8).view(N, K)
    return codes, (ex + 127).to(torch.uint8), deq.view(N, K).to(torch.bfloat16)

"""The W8A16 weight format in plain Python (csrc/gemm_small_w8.hip states it; nothing here calls the library): the e4m3fn decode table from the format's
definition, the power-of-two row scale, the quantiser.  tests/test_gemm_small_w8_gpu.py, tests/test_llama_w8_gpu.py, tests/test_weight_precision_host.py."""
import math

import torch


def decode(code: int) -> float:
    """e4m3fn: 1 sign, 4 exponent (bias 7), 3 mantissa bits; no infinities, NaN = S.1111.111; subnormals m / 8 * 2^-6"""
    s, e, m = code >> 7, (code >> 3) & 15, code & 7
    if e == 15 and m == 7:
        return math.nan
    v = m / 8.0 * 2.0 ** -6 if e == 0 else (1.0 + m / 8.0) * 2.0 ** (e - 7)
    return -v if s else v


TABLE = torch.tensor([decode(c) for c in range(256)], dtype=torch.float64)


def pow2_scale(absmax: float) -> float:
    """2^ceil(log2(absmax / 448)), 1 for 0, never below 2^-100; through frexp: absmax = f 2^e, f in [0.5, 1), and 448 = 0.875 x 2^9"""
    if absmax == 0:
        return 1.0
    f, e = math.frexp(absmax)
    return 2.0 ** max(e - 9 if f <= 0.875 else e - 8, -100)


def quantize(W: torch.Tensor):
    """W bf16 [N, K] -> (codes uint8 [N, K], scale fp32 [N], dequantised bf16 [N, K] = decode(code) * scale, exact), on the CPU"""
    W = W.detach().cpu()
    scale = torch.tensor([pow2_scale(float(v)) for v in W.float().abs().amax(dim=1)], dtype=torch.float64)
    codes = (W.double() / scale[:, None]).float().to(torch.float8_e4m3fn).view(torch.uint8)     # (a division by a power of two: exact; the cast is RNE)
    deq = TABLE[codes.long()] * scale[:, None]
    assert bool(torch.isfinite(deq).all()) and torch.equal(deq.to(torch.bfloat16).double(), deq)
    return codes, scale.float(), deq.to(torch.bfloat16)

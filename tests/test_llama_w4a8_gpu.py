"""LlamaTower(weight_precision="mxfp4-a8") / mq_encode_llama_w4a8: what "mxfp4-only" keeps resident, MX FP8 activations on the tall calls.  Short calls
against the "mxfp4-only" tower bit for bit; the tall call through the W4A8 GEMM: other bits, and pooled rows close to tests/llama_ref.py's float64
stream of the dequantised model; what stays resident.

The tall call's distance (largest 1 - cos over its pooled rows against the float64 stream), measured on an MI355X: 5.4e-4 with
"mxfp4-a8", 3.0e-6 with "mxfp4-only" on the same call (e4m3 activations carry 4 significant bits).  BAR = 3 x 5.4e-4 rounded up to one digit."""
import pytest
import torch

from tests import llama_ref as LR
from tests import qwen_ref as Q
from tests.test_llama_w4_gpu import CALLS, MATRICES, NAME
from tests.test_llama_w4_only_gpu import test_only_the_codes_and_scales_stay_resident as resident

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BAR = 2e-3


@pytest.fixture(scope="module")
def built():
    from marqo_amd.engine.llama import LlamaTower
    b = LR.stream_build(NAME)
    tower = LlamaTower(b["arch"], b["sd"], DEV, pooling="last", weight_precision="mxfp4-a8")
    only = LlamaTower(b["arch"], b["sd"], DEV, pooling="last", weight_precision="mxfp4-only")
    tensors = dict(b["tensors"])
    for l in range(b["arch"].layers):
        for short, key in MATRICES.items():
            tensors[f"layers.{l}.{key}"] = tower.block_weight(l, short).float().cpu()
    seqs = {n: s for n, s in zip((9, 30, 25, 300), Q.random_seqs([9, 30, 25, 300], b["arch"].vocab, seed=11))}
    runs = []
    for lens in CALLS:
        batch = Q.pad_batch([seqs[n] for n in lens])
        runs.append(dict(got=tower.encode_ids(*batch, normalize=True).cpu(), only=only.encode_ids(*batch, normalize=True).cpu()))
    ex = LR.stream_exact(b["arch"], tensors, torch.cat([seqs[n] for n in CALLS[-1]]).to(DEV), CALLS[-1]).pooled[("last", 1)].cpu()
    return dict(tower=tower, b=b, runs=runs, ex=ex)


@pytest.mark.parametrize("call", (0, 1))
def test_short_calls_give_the_mxfp4_only_towers_bits(built, call):
    r = built["runs"][call]
    assert torch.equal(r["got"].view(torch.int32), r["only"].view(torch.int32))


def test_the_tall_call_runs_the_w4a8_gemm_and_stays_close(built):
    r = built["runs"][-1]
    assert not torch.equal(r["got"].view(torch.int32), r["only"].view(torch.int32))
    d8, d16 = (float((1.0 - torch.nn.functional.cosine_similarity(r[k].double(), built["ex"].double(), dim=1)).max()) for k in ("got", "only"))
    print(f"LLAMA_W4A8 lens={list(CALLS[-1])} 1-cos: mxfp4-a8 {d8:.3e}, mxfp4-only {d16:.3e} (bar {BAR})")
    assert d8 <= BAR


def test_only_the_codes_and_scales_stay_resident(built):
    resident(built)     # tests/test_llama_w4_only_gpu.py's two assertions, on this mode's tower

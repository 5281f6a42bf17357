"""LlamaTower(weight_precision="mxfp4-only") / mq_encode_llama_w4_only: no bf16 block matrix resident.  Pooled rows against tests/llama_ref.py's float64
reference on the dequantised weights read through block_weight (decoded on demand from the codes), on the skinny path and on the tiled W4A16 path,
under test_llama_forms_gpu.py's bar; block_weight against the Python quantiser; short calls against the "mxfp4" tower, bit for bit; what stays resident."""
import pytest
import torch

from tests import knobs
from tests import llama_ref as LR
from tests import packed_text_ref as P
from tests import qwen_ref as Q
from tests import w4_ref as R
from tests.test_llama_w4_gpu import CALLS, MATRICES, NAME
from tests.test_patch_attn_gpu import MARGIN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def built():
    from marqo_amd.engine.llama import LlamaTower
    b = LR.stream_build(NAME)
    tower = LlamaTower(b["arch"], b["sd"], DEV, pooling="last", weight_precision="mxfp4-only")
    both = LlamaTower(b["arch"], b["sd"], DEV, pooling="last", weight_precision="mxfp4")
    tensors = dict(b["tensors"])
    for l in range(b["arch"].layers):
        for short, key in MATRICES.items():
            tensors[f"layers.{l}.{key}"] = tower.block_weight(l, short).float().cpu()
    assert sum(CALLS[-1]) > knobs.get("small_m_grouped") and sum(CALLS[1]) < 80
    seqs = {n: s for n, s in zip((9, 30, 25, 300), Q.random_seqs([9, 30, 25, 300], b["arch"].vocab, seed=11))}
    runs = []
    for lens in CALLS:
        ids = torch.cat([seqs[n] for n in lens])
        batch = Q.pad_batch([seqs[n] for n in lens])
        runs.append(dict(lens=lens, got=tower.encode_ids(*batch, normalize=True).cpu(), both=both.encode_ids(*batch, normalize=True).cpu(),
                         ex=LR.stream_exact(b["arch"], tensors, ids.to(DEV), lens).pooled[("last", 1)].cpu(),
                         mo=LR.stream_model(b["arch"], tensors, ids.to(DEV), lens).pooled[("last", 1)].cpu()))
    return dict(tower=tower, b=b, runs=runs)


@pytest.mark.parametrize("call", range(len(CALLS)))
def test_pooled_rows_against_float64_of_the_dequantised_model(built, call):
    r = built["runs"][call]
    w = P.row_ratio(r["got"], r["ex"], r["mo"])
    print(f"LLAMA_W4_ONLY lens={list(r['lens'])} ratio={w['ratio']:.3f} (row {w['row']}: l2 {w['l2']:.3f} linf {w['linf']:.3f}; bar {MARGIN})")
    assert w["ratio"] <= MARGIN, w


def test_block_weight_is_the_python_quantisers(built):
    for l in range(built["b"]["arch"].layers):
        for short, key in MATRICES.items():
            deq = R.quantize(built["b"]["tensors"][f"layers.{l}.{key}"].to(torch.bfloat16))[2]
            assert torch.equal(built["tower"].block_weight(l, short).cpu().view(torch.int16), deq.view(torch.int16)), (l, short)


@pytest.mark.parametrize("call", (0, 1))
def test_short_calls_give_the_mxfp4_towers_bits(built, call):
    r = built["runs"][call]
    assert torch.equal(r["got"].view(torch.int32), r["both"].view(torch.int32))


def test_only_the_codes_and_scales_stay_resident(built):
    a, tower = built["b"]["arch"], built["tower"]
    aw, qkvw = a.heads * a.head_dim, (a.heads + 2 * a.kv_heads) * a.head_dim
    shapes = {"qkv": (qkvw, a.width), "out": (a.width, aw), "ug": (2 * a.mlp_dim, a.width), "down": (a.width, a.mlp_dim)}
    kept = [t for t in tower._h.tensors if t.dtype == torch.bfloat16 and tuple(t.shape) in set(shapes.values())]
    assert not kept, [tuple(t.shape) for t in kept]
    blocks = sum(t.numel() for t in tower._h.tensors if t.dtype == torch.uint8)
    assert blocks == a.layers * sum(n * ((k + 127) // 128) * 68 for n, k in shapes.values())

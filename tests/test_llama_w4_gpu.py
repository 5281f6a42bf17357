"""LlamaTower(weight_precision="mxfp4") / mq_encode_llama_w4: pooled rows against tests/llama_ref.py's float64 reference on the DEQUANTISED weights read back
from the tower, on the W4A16 skinny path and on the tiled path over the bf16 copy, under test_llama_forms_gpu.py's bar (4.0 x the bf16 model's own error);
a sequence alone and inside a batch, bit for bit.  The config (width 128, MLP 192, 4 / 2 heads of 64) walks a whole chunk, a half chunk and two chunks."""
import pytest
import torch

from tests import knobs
from tests import llama_ref as LR
from tests import packed_text_ref as P
from tests import qwen_ref as Q
from tests import w4_ref as R
from tests.test_patch_attn_gpu import MARGIN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAME = "M128"
MATRICES = {"qkv": "self_attn.qkv.weight", "out": "self_attn.o_proj.weight", "ug": "mlp.up_gate.weight", "down": "mlp.down_proj.weight"}
CALLS = ((9,), (30, 9, 25), (300, 30, 9))     # skinny, skinny, tiled: 339 rows


@pytest.fixture(scope="module")
def built():
    """the tower, the loader's tensors with the four block matrices replaced by the tower's dequantised bf16 copies, and the calls' pooled rows"""
    from marqo_amd.engine.llama import LlamaTower
    b = LR.stream_build(NAME)
    tower = LlamaTower(b["arch"], b["sd"], DEV, pooling="last", weight_precision="mxfp4")
    tensors = dict(b["tensors"])
    for l in range(b["arch"].layers):
        for short, key in MATRICES.items():
            tensors[f"layers.{l}.{key}"] = tower.block_weight(l, short).float().cpu()
    assert sum(CALLS[-1]) > knobs.get("small_m_grouped") and sum(CALLS[1]) < 80
    seqs = {n: s for n, s in zip((9, 30, 25, 300), Q.random_seqs([9, 30, 25, 300], b["arch"].vocab, seed=11))}
    runs = []
    for lens in CALLS:
        ids = torch.cat([seqs[n] for n in lens])
        got = tower.encode_ids(*Q.pad_batch([seqs[n] for n in lens]), normalize=True).cpu()
        ex = LR.stream_exact(b["arch"], tensors, ids.to(DEV), lens).pooled[("last", 1)].cpu()
        mo = LR.stream_model(b["arch"], tensors, ids.to(DEV), lens).pooled[("last", 1)].cpu()
        runs.append(dict(lens=lens, got=got, ex=ex, mo=mo))
    return dict(tower=tower, b=b, runs=runs)


def test_the_bf16_copy_is_the_python_quantisers(built):
    for l in range(built["b"]["arch"].layers):
        for short, key in MATRICES.items():
            deq = R.quantize(built["b"]["tensors"][f"layers.{l}.{key}"].to(torch.bfloat16))[2]
            assert torch.equal(built["tower"].block_weight(l, short).cpu().view(torch.int16), deq.view(torch.int16)), (l, short)


@pytest.mark.parametrize("call", range(len(CALLS)))
def test_pooled_rows_against_float64_of_the_dequantised_model(built, call):
    r = built["runs"][call]
    w = P.row_ratio(r["got"], r["ex"], r["mo"])
    print(f"LLAMA_W4 lens={list(r['lens'])} ratio={w['ratio']:.3f} (row {w['row']}: l2 {w['l2']:.3f} linf {w['linf']:.3f}; bar {MARGIN})")
    assert w["ratio"] <= MARGIN, w


def test_a_sequence_alone_and_inside_a_batch_is_bit_identical(built):
    alone, batch = built["runs"][0], built["runs"][1]
    assert torch.equal(alone["got"][0].view(torch.int32), batch["got"][1].view(torch.int32))

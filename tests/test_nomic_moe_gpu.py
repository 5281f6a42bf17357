"""The mixture-of-experts NomicBERT tower on the GPU: NomicMoeTower (mq_encode_nomic_moe) against the float64 pass of tests/nomic_moe_ref.py — every row of
the token stream after every block and the pooled rows; bar as tests/test_nomic_bert_gpu.py: the worst row of max(|got - exact|_2 / |model - exact|_2,
the same in the inf norm) <= 4.0, the yardstick being the float64 bf16 model's own error — and `vectorise` (`hf`, a directory in the hub's naming written
here) against the same model in fp32 torch, 1 - cos < COS_TOL = 3e-4.  Before any device value is read the CPU asserts that `exact` and `model` route
every row alike and that the smallest deciding logit gap is at least 8 x the largest logit difference between the passes (264 x / 11.9 x in layers 1 / 3).
Tiny model: W 128, 2 heads, F 192, E 4, k 2, 4 layers (1 and 3 routed); lengths 1, 7, 64, 65, 130 in one batch; mean and CLS pooling.
Measured on an MI355X (MOE_RATIO lines): worst row ratio, stream after block 1 / 2 / 3 / 4: 1.36 / 1.69 / 1.69 / 1.92, pooled mean 1.39, cls 1.32 (bar 4.0);
vectorise worst 1 - cos against fp32 torch 9.7e-7 (bar 3e-4)."""
import ctypes as C

import pytest
import torch

from marqo_amd import _lib as L
from tests import attention_ref as A
from tests import nomic_moe_ref as M
from tests.test_modernbert_gpu import COS_TOL
from tests.test_patch_attn_gpu import MARGIN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_POOL = dict(mean=L.MQ_POOL_MEAN, cls=L.MQ_POOL_CLS)


def test_every_stream_row_against_float64():
    from marqo_amd.engine.nomic_moe import NomicMoeTower
    lib = L.load()
    b = M.build()
    arch, ids = b["arch"], torch.cat(b["seqs"])
    lens = [len(s) for s in b["seqs"]]
    assert lens == [1, 7, 64, 65, 130]
    re, rm = {}, {}
    full = (M.exact(arch, b["tensors"], ids, lens, rec=re), M.model(arch, b["tensors"], ids, lens, rec=rm))
    assert sorted(re) == [1, 3]
    for l in re:        # on the CPU, before any device value: the two passes route alike, by a margin
        assert torch.equal(re[l]["top_e"], rm[l]["top_e"])
        gap = min(float(re[l]["gap"].min()), float(rm[l]["gap"].min()))
        assert gap >= 8 * float((re[l]["logits"] - rm[l]["logits"]).abs().max()), (l, gap)
    tower = NomicMoeTower(arch, b["sd"], DEV, pooling="mean")
    assert tower.routed_layers == (1, 3)
    rows, nseq, W = sum(lens), len(lens), arch.width
    d_ids, cu_h = ids.to(torch.int32).to(DEV).contiguous(), A.cu_seqlens(lens)
    d_cu = cu_h.to(DEV)
    worst = {}
    for layers in range(1, arch.layers + 1):
        ex, mo = (M.exact(arch, b["tensors"], ids, lens, layers), M.model(arch, b["tensors"], ids, lens, layers)) if layers < arch.layers else full
        for pool in ("mean", "cls"):
            cfg = type(tower.cfg).from_buffer_copy(tower.cfg)
            cfg.layers, cfg.pool = layers, _POOL[pool]
            need = lib.mq_nomic_moe_workspace_bytes(C.byref(cfg), rows, nseq)
            ws = torch.full((need + 4096,), 0xA5, dtype=torch.uint8, device=DEV)
            out = torch.full((nseq + 2, W), float("nan"), dtype=torch.float32, device=DEV)
            L.check(lib.mq_encode_nomic_moe(C.byref(cfg), C.byref(tower.w), d_ids.data_ptr(), d_cu.data_ptr(), cu_h.data_ptr(), nseq, out[1:].data_ptr(), 1,
                                            ws.data_ptr(), need, torch.cuda.current_stream().cuda_stream), "mq_encode_nomic_moe")
            torch.cuda.synchronize()
            assert bool((ws[need:] == 0xA5).all()), "the workspace was written past mq_nomic_moe_workspace_bytes"
            assert bool(out[0].isnan().all()) and bool(out[-1].isnan().all()), "a guard row of d_out was written"
            x = ws[:rows * W * 4].view(torch.float32).view(rows, W)
            rs = M.row_ratio(x.cpu(), ex.final, mo.final)
            rp = M.row_ratio(out[1:-1].cpu(), ex.pooled[(pool, 1)], mo.pooled[(pool, 1)])
            print(f"MOE_RATIO tower layers={layers} pool={pool} stream={rs['ratio']:.3f} (row {rs['row']} col {rs['col']}) pooled={rp['ratio']:.3f}")
            worst[f"stream{layers}"] = max(worst.get(f"stream{layers}", 0.0), rs["ratio"])
            worst[f"pooled_{pool}"] = max(worst.get(f"pooled_{pool}", 0.0), rp["ratio"])
    print("MOE_RATIO tower worst: " + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= MARGIN, worst


TEXTS = ["hello world", "a router sends every token to two of the experts and adds what they return", "a search engine ranks documents for a query " * 8]
TOKENS = 48


@pytest.fixture(scope="module")
def directory(tmp_path_factory):
    b = M.build()
    return M.write_checkpoint_dir(str(tmp_path_factory.mktemp("nomic_moe") / "moe"), b["cfg"], b["sd"], M.train_tokenizer())


@pytest.mark.parametrize("over,what", ((dict(trustRemoteCode=False), "trustRemoteCode"), (dict(enginePrecision="fp8"), "fp8"), (dict(poolingMethod="last"), "pooling")))
def test_the_loader_refuses(directory, over, what):
    from marqo_amd.s2_inference.errors import InvalidModelPropertiesError
    from marqo_amd.s2_inference.hugging_face_model import HuggingFaceModel
    props = dict({"type": "hf", "name": directory, "dimensions": 128, "tokens": TOKENS, "trustRemoteCode": True}, **over)
    with pytest.raises(InvalidModelPropertiesError, match=what):
        HuggingFaceModel(model_properties=props, device=DEV)._load_necessary_components()


def test_vectorise_from_a_local_directory(directory, monkeypatch):
    """(refused on the commit before this family was served: num_experts / moe_every_n_layers)"""
    from tokenizers import Tokenizer
    from marqo_amd.s2_inference import s2_inference as s2i
    b = M.build()
    monkeypatch.setenv("MARQO_MAX_CUDA_MODEL_MEMORY", "64")
    props = {"type": "hf", "name": directory, "dimensions": 128, "tokens": TOKENS, "trustRemoteCode": True}
    try:
        s2i.clear_loaded_models()
        out = torch.tensor(s2i.vectorise("nomic-moe-test", TEXTS, model_properties=props, device=DEV, normalize_embeddings=True), dtype=torch.float64)
    finally:
        s2i.clear_loaded_models()
    raw = Tokenizer.from_file(directory + "/tokenizer.json")
    raw.enable_truncation(max_length=TOKENS)
    ref = torch.stack([M.torch_fp32(b["cfg"], b["sd"], torch.tensor(raw.encode(t).ids), "mean", True) for t in TEXTS]).double()
    e = 1 - (out * ref).sum(-1) / (out.norm(dim=-1) * ref.norm(dim=-1))
    print("MOE_RATIO vectorise 1 - cos against fp32 torch: " + " ".join(f"{float(v):.2e}" for v in e) + f" (bound {COS_TOL:.0e})")
    assert out.shape == (3, 128) and float(e.max()) < COS_TOL

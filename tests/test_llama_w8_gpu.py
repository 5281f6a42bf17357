"""LlamaTower(weight_precision="e4m3") / mq_encode_llama_w8: pooled rows against tests/llama_ref.py's float64 reference on the DEQUANTISED weights read back
from the tower, on the W8A16 skinny path and on the tiled path over the bf16 copy, under test_llama_forms_gpu.py's bar (4.0 x the bf16 model's own error);
the same text alone and inside the large call (one model on both paths); `vectorise`."""
import json

import pytest
import torch

from tests import knobs
from tests import llama_ref as LR
from tests import packed_text_ref as P
from tests import qwen_ref as Q
from tests import w8_ref as R
from tests.test_patch_attn_gpu import MARGIN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAME = "M128"
MATRICES = {"qkv": "self_attn.qkv.weight", "out": "self_attn.o_proj.weight", "ug": "mlp.up_gate.weight", "down": "mlp.down_proj.weight"}
CALLS = ((9,), (30, 17, 25), (300, 30, 9))     # skinny, skinny, tiled: 339 rows


@pytest.fixture(scope="module")
def built():
    """the tower, the loader's tensors with the four block matrices replaced by the tower's dequantised bf16 copies, and the calls' pooled rows"""
    from marqo_amd.engine.llama import LlamaTower
    b = LR.stream_build(NAME)
    tower = LlamaTower(b["arch"], b["sd"], DEV, pooling="last", weight_precision="e4m3")
    tensors = dict(b["tensors"])
    for l in range(b["arch"].layers):
        for short, key in MATRICES.items():
            tensors[f"layers.{l}.{key}"] = tower.block_weight(l, short).float().cpu()
    assert CALLS[-1][-1] == CALLS[0][0] and sum(CALLS[-1]) > knobs.get("small_m_grouped") and sum(CALLS[1]) < 80
    seqs = {n: s for n, s in zip((9, 30, 17, 25, 300), Q.random_seqs([9, 30, 17, 25, 300], b["arch"].vocab, seed=11))}
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
    print(f"LLAMA_W8 lens={list(r['lens'])} ratio={w['ratio']:.3f} (row {w['row']}: l2 {w['l2']:.3f} linf {w['linf']:.3f}; bar {MARGIN})")
    assert w["ratio"] <= MARGIN, w


def test_a_text_alone_and_inside_the_large_call_is_one_model(built):
    alone, large = built["runs"][0], built["runs"][-1]
    d = alone["got"][0].double() - large["got"][-1].double()
    y = large["mo"][-1].double() - large["ex"][-1].double()
    ratio = max(float(d.norm() / y.norm()), float(d.abs().max() / y.abs().max()))
    print(f"LLAMA_W8 alone vs inside {list(large['lens'])}: {ratio:.3f} of the model's own error (bar {MARGIN})")
    assert ratio <= MARGIN


def test_vectorise_takes_the_property_for_llama_and_refuses_it_elsewhere(tmp_path, monkeypatch):
    from safetensors.torch import save_file
    from marqo_amd.s2_inference import s2_inference as s2i
    from marqo_amd.s2_inference.errors import InvalidModelPropertiesError, ModelLoadError
    t = LR.tiny(NAME)
    d = Q.write_checkpoint_dir(str(tmp_path / "ckpt"), t["cfg"], {"model." + k: v.float() for k, v in t["sd"].items()}, Q.train_tokenizer())
    monkeypatch.setenv("MARQO_MAX_CUDA_MODEL_MEMORY", "64")
    props = {"type": "hf", "name": d, "dimensions": 128, "tokens": 64, "weightPrecision": "e4m3"}
    bert = tmp_path / "bert"
    bert.mkdir()
    (bert / "config.json").write_text(json.dumps(dict(model_type="bert", vocab_size=100, max_position_embeddings=64, hidden_size=128, num_hidden_layers=2,
                                                      num_attention_heads=2, intermediate_size=256, hidden_act="gelu", layer_norm_eps=1e-12)))
    save_file({"x": torch.zeros(1)}, str(bert / "model.safetensors"))
    try:
        s2i.clear_loaded_models()
        out = torch.tensor(s2i.vectorise("mistral-w8", ["a short query", "another, somewhat longer text about foxes"], model_properties=props, device=DEV))
        assert out.shape == (2, 128) and bool(torch.isfinite(out).all()) and float((out.norm(dim=1) - 1).abs().max()) < 1e-5
        for mp, what in ((dict(props, name=str(bert)), "'weightPrecision': 'e4m3' is available for Mistral / Llama"),
                         (dict(props, weightPrecision="int4"), "'weightPrecision' must be 'bf16' or 'e4m3'")):
            with pytest.raises(ModelLoadError, match=what) as e:      # (vectorise reports a loader's refusal as a ModelLoadError that carries it)
                s2i.vectorise("w8-refused", ["a"], model_properties=mp, device=DEV)
            assert isinstance(e.value.__cause__, InvalidModelPropertiesError)
    finally:
        s2i.clear_loaded_models()

"""The Mistral / Llama tower on the GPU: LlamaTower (mq_encode_llama through engine/llama.py) against the project's float64 oracle (tests/llama_ref.py,
itself equal to transformers' MistralModel / LlamaModel in float64 to 1e-6: tests/test_llama_host.py), and `vectorise` from a local checkpoint directory
with model_type "mistral" against fp32 transformers.

Four tinies of 2 layers: M128 (width 128, 4 / 2 heads of 64, window 48), M2560 (width 2560 through the wide row kernels, 4 / 1 heads of 128 so that
heads x head_dim != width, window 200), M4096 (width 4096, no window), L128 (a Llama: no window, no grouping).  One packed call of lengths 1, 17, 70, 129
and 300: both windows bind, 300 tokens are three query slices.  Bar: 1 - cos < 3e-4 on the pooled rows, the project's bf16 tower bar
(tests/test_modernbert_gpu.py), for both poolings with and without L2; a permuted batch gives the permuted rows bit for bit.

Measured values are printed as `LLAMA_COS` lines."""
import os

import numpy as np
import pytest
import torch

from tests import llama_ref as LR
from tests import qwen_ref as Q
from tests.test_modernbert_gpu import COS_TOL

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _err(out, ref):
    out = out.double().cpu()
    return 1 - (out * ref).sum(-1) / (out.norm(dim=-1) * ref.norm(dim=-1))


@pytest.mark.parametrize("name", tuple(LR.TINIES))
@pytest.mark.parametrize("pooling", ("last", "mean"))
def test_tiny_tower_against_the_oracle(name, pooling):
    from marqo_amd.engine.llama import LlamaTower
    t = LR.tiny(name)
    tower = LlamaTower(t["arch"], t["sd"], DEV, pooling=pooling)
    ids, mask = Q.pad_batch(t["seqs"])
    for normalize in (True, False):
        out = tower.encode_ids(ids, mask, normalize=normalize)
        ref = Q.pooled(t["hidden"], pooling, normalize)
        e = _err(out, ref)
        print(f"LLAMA_COS {name} {pooling} normalize={normalize}: " + " ".join(f"{float(v):.2e}" for v in e) + f" (bound {COS_TOL:.0e})")
        assert float(e.max()) < COS_TOL, (name, pooling, e.tolist())
        norms = out.double().cpu().norm(dim=-1)
        if normalize:
            np.testing.assert_allclose(norms.numpy(), 1.0, atol=1e-5)
        else:
            np.testing.assert_allclose(norms.numpy(), ref.norm(dim=-1).numpy(), rtol=2e-2)
        perm = torch.tensor([3, 0, 4, 1, 2])
        assert torch.equal(tower.encode_ids(ids[perm], mask[perm], normalize=normalize), out[perm])


def test_the_window_is_what_the_tower_runs():
    """the same weights under no window are another model at these lengths: the windowed tower is outside the bar of the causal oracle's long rows, so the
    bar above can tell the two apart"""
    from marqo_amd.engine import archs
    from marqo_amd.engine.llama import LlamaTower
    t = LR.tiny("M128")
    ids, mask = Q.pad_batch(t["seqs"])
    tower = LlamaTower(t["arch"], t["sd"], DEV, pooling="last")
    out = tower.encode_ids(ids, mask)
    causal = archs.LlamaArch(**{**t["arch"].__dict__, "window": None})
    ref = Q.pooled([LR.oracle_hidden(t["sd"], causal, s) for s in t["seqs"]], "last", True)
    e = _err(out, ref)
    print("LLAMA_COS M128 windowed tower against the causal oracle: " + " ".join(f"{float(v):.2e}" for v in e))
    assert float(e[:2].max()) < COS_TOL and float(e[2:].min()) > COS_TOL     # lengths 1 and 17 fit the window of 48; 70, 129 and 300 do not
    # a call whose sequences all fit the window: the causal kernel either way, the same bits
    assert torch.equal(LlamaTower(causal, t["sd"], DEV, pooling="last").encode_ids(ids[:2], mask[:2]), tower.encode_ids(ids[:2], mask[:2]))


def test_vectorise_from_a_local_directory(tmp_path, monkeypatch):
    from tokenizers import Tokenizer
    from marqo_amd.engine.llama import LlamaTower
    from marqo_amd.s2_inference import s2_inference as s2i
    t = LR.tiny("M128")
    d = Q.write_checkpoint_dir(str(tmp_path / "ckpt"), t["cfg"], {"model." + k: v.float() for k, v in t["sd"].items()}, Q.train_tokenizer())
    monkeypatch.setenv("MARQO_MAX_CUDA_MODEL_MEMORY", "64")
    props = {"type": "hf", "name": d, "dimensions": 128, "tokens": 64}
    texts = ["hello world", "a sliding window keeps the last keys of a long text", "a search engine ranks documents for a query " * 8, ""]
    raw = Tokenizer.from_file(os.path.join(d, "tokenizer.json"))
    raw.enable_truncation(max_length=64)
    rows = [torch.tensor(raw.encode(x).ids) for x in texts]
    assert max(len(r) for r in rows) == 64 and min(len(r) for r in rows) == 1 and all(int(r[-1]) == 0 for r in rows)
    try:
        s2i.clear_loaded_models()
        out = torch.tensor(s2i.vectorise("mistral-test", texts, model_properties=props, device=DEV), dtype=torch.float64)
    finally:
        s2i.clear_loaded_models()
    assert out.shape == (4, 128)
    np.testing.assert_allclose(out.norm(dim=-1).numpy(), 1.0, atol=1e-5)
    ids, mask = Q.pad_batch(rows)
    direct = LlamaTower(t["arch"], t["sd"], DEV, pooling="last").encode_ids(ids, mask).double().cpu()
    assert torch.equal(out, direct)
    model = LR.hf_model(t["cfg"], seed=list(LR.TINIES).index("M128") + 1, dtype=torch.float32)
    with torch.no_grad():      # fp32 transformers on the CPU: right-padded batch, the last real token of every row
        hid = model(input_ids=ids, attention_mask=mask).last_hidden_state
    ref = torch.stack([hid[i, len(r) - 1].double() for i, r in enumerate(rows)])
    e = _err(out, ref)
    print("LLAMA_COS vectorise against transformers: " + " ".join(f"{float(v):.2e}" for v in e) + f" (bound {COS_TOL:.0e})")
    assert float(e.max()) < COS_TOL

"""The ModernBERT tower on the GPU (mq_encode_modernbert through engine/modernbert.py) against the project's fp32 oracle (tests/modernbert_ref.py, itself equal
to transformers' ModernBertModel to fp32 round-off: tests/test_modernbert_host.py).

The bar: max 1 - cos < 3e-4 on the pooled, L2-normalised rows, with unit norms — the bar tests/test_stella.py sets for this project's other bf16 rotary /
gated-GELU tower.  The measured values are printed as `MODERNBERT_COS` lines."""
import os

import numpy as np
import pytest
import torch

from marqo_amd.engine import archs
from tests import modernbert_ref as M

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
COS_TOL = 3e-4


def _err(out, ref):
    out = out.double().cpu()
    return 1 - (out * ref).sum(-1) / out.norm(dim=-1)


def _check(tag, tower_rows, ref):
    e = _err(tower_rows, ref)
    print(f"MODERNBERT_COS {tag}: " + " ".join(f"{float(v):.2e}" for v in e) + f" (bound {COS_TOL:.0e})")
    np.testing.assert_allclose(tower_rows.double().cpu().norm(dim=-1).numpy(), 1.0, atol=1e-5)
    assert float(e.max()) < COS_TOL, (tag, e.tolist())


@pytest.fixture(scope="module")
def tiny():
    cfg = M.config_dict()
    model = M.hf_model(cfg, seed=0)
    arch = archs.bert_arch_from_hf_config(cfg)
    sd = M.state_dict_of(model)
    seqs = M.random_seqs([5, 17, 64, 65, 129, 200, 33, 100], cfg["vocab_size"], seed=3)
    return dict(cfg=cfg, arch=arch, sd=sd, seqs=seqs, hidden=M.oracle_hidden_packed(sd, arch, seqs))


@pytest.mark.parametrize("pooling", ("mean", "cls"))
def test_tiny_tower_against_the_oracle(tiny, pooling):
    """4 layers (full, sliding, sliding, full; layer 0 without attn_norm), 2 heads of 64, F = 192, half-window 8, lengths 5 .. 200 in one packed call"""
    from marqo_amd.engine.modernbert import ModernBertTower
    tower = ModernBertTower(tiny["arch"], tiny["sd"], DEV, pooling=pooling)
    ids, mask = M.pad_batch(tiny["seqs"])
    out = tower.encode_ids(ids, mask)
    _check(f"tiny {pooling}", out, M.pooled(tiny["hidden"], pooling))
    raw = tower.encode_ids(ids[:2], mask[:2], normalize=False).double().cpu()      # un-normalised rows are the pooled hidden states themselves
    want = torch.stack([(h.double().mean(0) if pooling == "mean" else h[0].double()) for h in tiny["hidden"][:2]])
    assert float((1 - torch.nn.functional.cosine_similarity(raw, want)).max()) < COS_TOL


def test_checkpoint_shape_at_two_layers():
    """width 768, 12 heads, F = 1152, local_attention = 128 (the published half-window of 64), a full and a sliding layer; 300 and 90 tokens: slices with a
    halo on both sides, tiles inside the band and tiles cut by it"""
    from marqo_amd.engine.modernbert import ModernBertTower
    cfg = M.config_dict(hidden_size=768, num_attention_heads=12, intermediate_size=1152, local_attention=128, num_hidden_layers=2,
                        max_position_embeddings=512)
    model = M.hf_model(cfg, seed=5)
    arch = archs.bert_arch_from_hf_config(cfg)
    assert arch.half_window == 64 and arch.sliding == (False, True)
    sd = M.state_dict_of(model)
    seqs = M.random_seqs([300, 90], cfg["vocab_size"], seed=6)
    ids, mask = M.pad_batch(seqs)
    out = ModernBertTower(arch, sd, DEV).encode_ids(ids, mask)
    _check("768x12 2 layers", out, M.pooled(M.oracle_hidden_packed(sd, arch, seqs)))


@pytest.mark.parametrize("pooling", ("mean", "cls"))
def test_vectorise_from_a_local_directory(tiny, tmp_path, monkeypatch, pooling):
    from tokenizers import Tokenizer
    from marqo_amd.s2_inference import s2_inference as s2i
    d = M.write_checkpoint_dir(str(tmp_path / "ckpt"), tiny["cfg"], {"model." + k: v for k, v in tiny["sd"].items()}, M.train_tokenizer())
    monkeypatch.setenv("MARQO_MAX_CUDA_MODEL_MEMORY", "64")
    props = {"type": "hf", "localpath": d, "dimensions": 128, "poolingMethod": pooling, "tokens": 64}
    texts = ["hello world", "sliding window attention keeps long documents cheap", "a search engine ranks documents for a query " * 8, "naïve café", ""]
    raw = Tokenizer.from_file(os.path.join(d, "tokenizer.json"))
    raw.enable_truncation(max_length=64)
    rows = [torch.tensor(raw.encode(t).ids) for t in texts]
    assert max(len(r) for r in rows) == 64 and min(len(r) for r in rows) == 2
    ref = M.pooled(M.oracle_hidden_packed(tiny["sd"], tiny["arch"], rows), pooling)
    try:
        s2i.clear_loaded_models()
        out = torch.tensor(s2i.vectorise("modernbert-test", texts, model_properties=props, device=DEV), dtype=torch.float64)
        one = torch.tensor(s2i.vectorise("modernbert-test", texts[1], model_properties=props, device=DEV), dtype=torch.float64)
    finally:
        s2i.clear_loaded_models()
    assert out.shape == (len(texts), 128)
    _check(f"vectorise {pooling}", out, ref)
    assert float(_err(one, ref[1:2]).max()) < COS_TOL


@pytest.mark.parametrize("gain", (0.6, 1.5))
def test_error_by_depth(tiny, gain):
    """Where the tower's error enters: the model cut behind block k = 1 .. 4 (final_norm, mean pooling), tower against oracle — and, on the host, the oracle
    with only q and k rounded to bf16 where the tower stores them, against the plain oracle.  gain 0.6 is the suite's draw (attention logits of standard
    deviation ~1.4) and is held to the bar at every depth.  gain 1.5 (Linear weights 2.5 times larger: logits of standard deviation ~9, softmax rows close
    to one-hot) is printed, not asserted.  Measured on an MI355X, max 1 - cos after 1 / 2 / 3 / 4 blocks (full, sliding, sliding, full):
        gain 0.6   tower 1.4e-6 / 2.9e-6 / 4.0e-6 / 5.6e-6     fp32 oracle with bf16 q, k 1.4e-7 / 3.1e-7 / 5.0e-7 / 6.4e-7
        gain 1.5   tower 9.3e-5 / 4.7e-4 / 1.4e-3 / 5.7e-3     fp32 oracle with bf16 q, k 4.0e-5 / 2.2e-4 / 5.4e-4 / 1.8e-3
    No single layer lets the error in: it is there after block 0 and grows by 3 to 5 times per block on the sharp draw, full and sliding blocks alike
    (every block's attention amplifies what reaches it), and an fp32 model in which nothing but q and k is rounded to bf16 already shows 30 - 45 % of it."""
    from marqo_amd.engine.modernbert import ModernBertTower
    cfg, seqs = tiny["cfg"], tiny["seqs"]
    if gain == 0.6:
        arch, sd = tiny["arch"], tiny["sd"]
    else:
        arch, sd = tiny["arch"], M.state_dict_of(M.hf_model(cfg, seed=0, gain=gain))
    ids, mask = M.pad_batch(seqs)
    for k in range(1, arch.layers + 1):
        cut = M.first_layers(arch, k)
        ref = M.pooled(M.oracle_hidden_packed(sd, cut, seqs))
        e_tower = float(_err(ModernBertTower(cut, sd, DEV).encode_ids(ids, mask), ref).max())
        e_qk = float(_err(M.pooled(M.oracle_hidden_packed(sd, cut, seqs, bf16_qk=True)).float(), ref).max())
        print(f"MODERNBERT_DEPTH gain={gain} blocks={k} ({'sliding' if cut.sliding[-1] else 'full'}): tower {e_tower:.2e}   fp32 oracle with bf16 q, k {e_qk:.2e}")
        if gain == 0.6:
            assert e_tower < COS_TOL, (k, e_tower)

"""The T5 encoder tower on the GPU: T5Tower (mq_encode_t5 through engine/t5.py) and `vectorise` (`hf`, `sbert`) against transformers' T5EncoderModel in
fp32 on the CPU, and every row of the token stream after every block against the float64 pass of tests/t5_ref.py.

Bars:
  pooled rows against the transformers oracle: 1 - cos < 3e-4, the project's bf16 tower bar (COS_TOL of tests/test_modernbert_gpu.py / test_gemma_gpu.py).
  the stream after every block (cfg.layers = 1 .. layers: the final norm runs in place, so the slice holds norm(stream after block l)), and the pooled
  rows: the worst row of  max(|got - exact|_2 / |model - exact|_2, |got - exact|_inf / |model - exact|_inf)  <= MARGIN = 4.0 — the bar
  tests/test_packed_text_forms_gpu.py holds the merged packed towers to for the same quantity (tests/test_patch_attn_gpu.py's MARGIN).  The yardstick is
  the float64 model's own distance from `exact`; it is never derived from the kernel's output.  tests/test_t5_host.py shows that the model's second
  rounding history stays at 1.00 .. 1.33 on these inputs and that five defects of the orchestration leave the bar (16 .. 409).

The stream is read from the first slice of the workspace (off_x is the plan's first take), as tests/test_packed_text_forms_gpu.py reads it; pooling that
slice with mq_pool must reproduce d_out bit for bit before any ratio is measured.

Lengths 1, 2, 64, 65 and 200 in one batch (64 / 65: the kernel's 64-query slice; 200 passes the clamp at D = 128).

Measured on an MI355X (T5_RATIO / T5_COS lines; the first GPU run needed no other bar than the packed towers' 4.0):
  worst row ratio, stream after block 1 / after block 2 / pooled:  TINY_RELU 1.66 / 1.51 / 1.18   TINY_GATED 1.46 / 1.62 / 1.22   TINY_WIDE 1.41 / 1.76 / 1.25
  worst 1 - cos against transformers:  TINY_RELU 1.2e-5   TINY_GATED 1.3e-4   TINY_WIDE 3.5e-5;  vectorise 4.6e-6 (hf), 6.9e-6 (sbert, through 2_Dense)
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from marqo_amd import _lib as L
from tests import attention_ref as A
from tests import t5_ref as T
from tests.test_modernbert_gpu import COS_TOL
from tests.test_patch_attn_gpu import MARGIN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_POOL = dict(mean=L.MQ_POOL_MEAN, cls=L.MQ_POOL_CLS)


def _err(out, ref):
    out = out.double().cpu()
    return 1 - (out * ref).sum(-1) / (out.norm(dim=-1) * ref.norm(dim=-1))


@pytest.fixture(scope="module")
def oracles():
    """transformers' hidden states of every tiny on the batch, computed once"""
    return {name: T.oracle_hidden_packed(T.build(name)["model"], T.build(name)["seqs"]) for name in T.TINIES}


@pytest.mark.parametrize("name", tuple(T.TINIES))
@pytest.mark.parametrize("pooling", ("mean", "cls"))
def test_tiny_tower_against_transformers(oracles, name, pooling):
    from marqo_amd.engine.t5 import T5Tower
    b = T.build(name)
    tower = T5Tower(b["arch"], b["sd"], DEV, pooling=pooling)
    ids, mask = T.pad_batch(b["seqs"])
    for normalize in (True, False):
        out = tower.encode_ids(ids, mask, normalize=normalize)
        ref = T.pooled(oracles[name], pooling, normalize)
        e = _err(out, ref)
        print(f"T5_COS {name} {pooling} normalize={normalize}: " + " ".join(f"{float(v):.2e}" for v in e) + f" (bound {COS_TOL:.0e})")
        assert float(e.max()) < COS_TOL, (name, pooling, e.tolist())
        norms = out.double().cpu().norm(dim=-1)
        if normalize:
            np.testing.assert_allclose(norms.numpy(), 1.0, atol=1e-5)
        else:
            np.testing.assert_allclose(norms.numpy(), ref.norm(dim=-1).numpy(), rtol=2e-2)
        perm = torch.tensor([3, 0, 4, 1, 2])
        assert torch.equal(tower.encode_ids(ids[perm], mask[perm], normalize=normalize), out[perm])


@pytest.mark.parametrize("name", tuple(T.TINIES))
def test_every_stream_row_against_float64(name):
    from marqo_amd.engine.t5 import T5Tower
    lib = L.load()
    b = T.build(name)
    arch = b["arch"]
    tower = T5Tower(arch, b["sd"], DEV, pooling="mean")
    lens = [len(s) for s in b["seqs"]]
    ids = torch.cat(b["seqs"])
    rows, nseq, W = sum(lens), len(lens), arch.width
    d_ids = ids.to(torch.int32).to(DEV).contiguous()
    cu_h = A.cu_seqlens(lens)
    d_cu = cu_h.to(DEV)
    s = lambda: torch.cuda.current_stream().cuda_stream
    worst = {}
    for layers in range(1, arch.layers + 1):
        ex = T.exact(arch, b["tensors"], ids.to(DEV), lens, layers)
        mo = T.model(arch, b["tensors"], ids.to(DEV), lens, layers)
        for pool in ("mean", "cls"):
            for normalize in (0, 1):
                cfg = type(tower.cfg).from_buffer_copy(tower.cfg)
                cfg.layers, cfg.pool = layers, _POOL[pool]
                need = lib.mq_t5_workspace_bytes(C.byref(cfg), rows, nseq)
                ws = torch.full((need + 4096,), 0xA5, dtype=torch.uint8, device=DEV)
                out = torch.full((nseq + 2, W), float("nan"), dtype=torch.float32, device=DEV)
                torch.cuda.synchronize()
                L.check(lib.mq_encode_t5(C.byref(cfg), C.byref(tower.w), d_ids.data_ptr(), d_cu.data_ptr(), cu_h.data_ptr(), nseq, out[1:].data_ptr(), normalize,
                                         ws.data_ptr(), need, s()), "mq_encode_t5")
                torch.cuda.synchronize()
                assert bool((ws[need:] == 0xA5).all()), "the workspace was written past mq_t5_workspace_bytes"
                assert bool(out[0].isnan().all()) and bool(out[-1].isnan().all()), "a guard row of d_out was written"
                x = ws[:rows * W * 4].view(torch.float32).view(rows, W)
                again = torch.empty(nseq, W, dtype=torch.float32, device=DEV)
                L.check(lib.mq_pool(x.data_ptr(), d_cu.data_ptr(), nseq, again.data_ptr(), W, _POOL[pool], normalize, s()), "mq_pool")
                torch.cuda.synchronize()
                assert torch.equal(again.view(torch.int32), out[1:-1].view(torch.int32)), "the stream is not the workspace's first slice: no parity was measured"
                assert bool(torch.isfinite(x).all())
                rs = T.row_ratio(x, ex.final, mo.final)
                rp = T.row_ratio(out[1:-1], ex.pooled[(pool, normalize)], mo.pooled[(pool, normalize)])
                print(f"T5_RATIO {name} layers={layers} pool={pool} l2={normalize} stream={rs['ratio']:.3f} (row {rs['row']} col {rs['col']}) pooled={rp['ratio']:.3f}")
                worst[f"stream{layers}"] = max(worst.get(f"stream{layers}", 0.0), rs["ratio"])
                worst["pooled"] = max(worst.get("pooled", 0.0), rp["ratio"])
                rc = lib.mq_encode_t5(C.byref(cfg), C.byref(tower.w), d_ids.data_ptr(), d_cu.data_ptr(), cu_h.data_ptr(), nseq, out[1:].data_ptr(), normalize,
                                      ws.data_ptr(), need - 1, s())
                assert rc == -3, f"a workspace one byte short: rc {rc}, not MQ_ERR_WORKSPACE"
    print(f"T5_WORST {name}: " + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= MARGIN, worst


# ---- vectorise ------------------------------------------------------------------------------------------------------------------------------------------
TEXTS = ["hello world", "sliding windows see only their neighbours", "a search engine ranks documents for a query " * 8, ""]


@pytest.fixture(scope="module")
def ckpt(tmp_path_factory):
    """TINY_RELU as a user brings it: save_pretrained + tokenizer.json + 1_Pooling + a 2_Dense that is not the identity + sentence_bert_config.json"""
    import transformers
    g = torch.Generator().manual_seed(17)
    dense = [torch.randn(128, 128, generator=g) / 128 ** 0.5]
    d = T.write_checkpoint_dir(str(tmp_path_factory.mktemp("t5") / "ckpt"), T.build("TINY_RELU")["model"], T.train_tokenizer(), pooling="mean", dense=dense,
                               max_seq_length=64)
    model = transformers.T5EncoderModel.from_pretrained(d).float().eval()
    return dict(dir=d, model=model, dense=dense)


def _reference_rows(ckpt, tokens=64):
    from tokenizers import Tokenizer
    raw = Tokenizer.from_file(os.path.join(ckpt["dir"], "tokenizer.json"))
    raw.enable_truncation(max_length=tokens)
    rows = [torch.tensor(raw.encode(x).ids) for x in TEXTS]
    assert max(len(r) for r in rows) == tokens and min(len(r) for r in rows) == 1 and all(int(r[-1]) == 1 for r in rows)
    ids, mask = T.pad_batch(rows)
    with torch.no_grad():
        hid = ckpt["model"](input_ids=ids, attention_mask=mask).last_hidden_state
    return torch.stack([hid[i, :len(r)].double().mean(0) for i, r in enumerate(rows)])


@pytest.mark.parametrize("kind", ("hf", "sbert"))
def test_vectorise_from_a_local_directory(ckpt, monkeypatch, kind):
    from marqo_amd.s2_inference import s2_inference as s2i
    monkeypatch.setenv("MARQO_MAX_CUDA_MODEL_MEMORY", "64")
    props = {"type": kind, "name": ckpt["dir"], "dimensions": 128, "tokens": 64}
    try:
        s2i.clear_loaded_models()
        out = torch.tensor(s2i.vectorise(f"t5-test-{kind}", TEXTS, model_properties=props, device=DEV), dtype=torch.float64)
    finally:
        s2i.clear_loaded_models()
    assert out.shape == (4, 128)
    np.testing.assert_allclose(out.norm(dim=-1).numpy(), 1.0, atol=1e-5)
    ref = _reference_rows(ckpt)
    if kind == "sbert":      # the SentenceTransformer pipeline: Pooling -> 2_Dense -> Normalize
        ref = ref @ ckpt["dense"][0].double().t()
    e = _err(out, ref)
    print(f"T5_COS vectorise {kind} against transformers: " + " ".join(f"{float(v):.2e}" for v in e) + f" (bound {COS_TOL:.0e})")
    assert float(e.max()) < COS_TOL
    if kind == "sbert":      # and the Dense module is not the identity: the bare encoder's rows are elsewhere
        assert float(_err(out, _reference_rows(ckpt)).min()) > 100 * COS_TOL

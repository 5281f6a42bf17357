"""The JinaBERT tower on the GPU: JinaBertTower (mq_encode_jina_bert through engine/jina_bert.py) and `vectorise` (`hf`) against the float64 pass of
tests/jina_bert_ref.py — every row of the final token stream and the pooled rows.  There is no library oracle: the checkpoints are custom remote code, the
block semantics restate the published architecture and are not pinned to a run of the original modelling code (tests/test_jina_bert_host.py pins the
slopes to transformers' Bloom and writes the formula out once in plain torch).

Bars (those of tests/test_t5_gpu.py):
  the stream (cfg.layers = 1 .. layers: the tower has no final norm, so the workspace's first slice holds the stream after block l) and the pooled rows:
  the worst row of  max(|got - exact|_2 / |model - exact|_2, |got - exact|_inf / |model - exact|_inf)  <= MARGIN = 4.0 — the bar
  tests/test_packed_text_forms_gpu.py holds the merged packed towers to for the same quantity.  The yardstick is the float64 model's own distance from
  `exact`; it is never derived from the kernel's output.  Each mutant of the model (gate_swapped, slopes_reversed, bias_scaled, no_abs, pre_ln) is shown,
  on the device and on the same inputs, to leave that bar in the stream and in every pooled view.
  `vectorise` against the float64 `exact` pass fed the `tokenizers` library's ids: 1 - cos < 3e-4, the project's bf16 tower bar (COS_TOL).

The stream is read from the first slice of the workspace (off_x is the plan's first take), as tests/test_packed_text_forms_gpu.py reads it; pooling that
slice with mq_pool must reproduce d_out bit for bit before any ratio is measured.

Lengths 1, 2, 64, 65 and 200 in one batch (64 / 65: the kernel's 64-query slice); one 700-token sequence (past the 640 keys of the attention kernel's LDS
image: K / V stream through in two pieces inside the tower).

Measured on an MI355X (JINA_RATIO / JINA_COS lines):
  worst row ratio, stream after block 1 / after block 2 / pooled:  TINY_2H 1.90 / 1.92 / 1.23   TINY_3H 1.59 / 1.58 / 1.06;  the 700-token sequence:
  stream 1.70, pooled 1.00 (bar 4.0).  The mutants on the device, smallest view: gate_swapped 159, slopes_reversed 32, bias_scaled 23, no_abs 9.5,
  pre_ln 287.  vectorise worst 1 - cos against the float64 pass: 9.1e-7 (mean), 8.7e-7 (cls) (bar 3e-4).
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from marqo_amd import _lib as L
from tests import attention_ref as A
from tests import jina_bert_ref as J
from tests.test_modernbert_gpu import COS_TOL
from tests.test_patch_attn_gpu import MARGIN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_POOL = dict(mean=L.MQ_POOL_MEAN, cls=L.MQ_POOL_CLS)


def _err(out, ref):
    out = out.double().cpu()
    ref = ref.double().cpu()
    return 1 - (out * ref).sum(-1) / (out.norm(dim=-1) * ref.norm(dim=-1))


def _s():
    return torch.cuda.current_stream().cuda_stream


def _call(lib, tower, cfg, d_ids, d_cu, cu_h, rows, nseq, normalize):
    """one guarded mq_encode_jina_bert call -> (stream x [rows, W], pooled [nseq, W], the workspace, its size)"""
    W = cfg.width
    need = lib.mq_jina_bert_workspace_bytes(C.byref(cfg), rows, nseq)
    ws = torch.full((need + 4096,), 0xA5, dtype=torch.uint8, device=DEV)
    out = torch.full((nseq + 2, W), float("nan"), dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    L.check(lib.mq_encode_jina_bert(C.byref(cfg), C.byref(tower.w), d_ids.data_ptr(), d_cu.data_ptr(), cu_h.data_ptr(), nseq, out[1:].data_ptr(), normalize,
                                    ws.data_ptr(), need, _s()), "mq_encode_jina_bert")
    torch.cuda.synchronize()
    assert bool((ws[need:] == 0xA5).all()), "the workspace was written past mq_jina_bert_workspace_bytes"
    assert bool(out[0].isnan().all()) and bool(out[-1].isnan().all()), "a guard row of d_out was written"
    x = ws[:rows * W * 4].view(torch.float32).view(rows, W)
    again = torch.empty(nseq, W, dtype=torch.float32, device=DEV)
    L.check(lib.mq_pool(x.data_ptr(), d_cu.data_ptr(), nseq, again.data_ptr(), W, cfg.pool, normalize, _s()), "mq_pool")
    torch.cuda.synchronize()
    assert torch.equal(again.view(torch.int32), out[1:-1].view(torch.int32)), "the stream is not the workspace's first slice: no parity was measured"
    assert bool(torch.isfinite(x).all())
    return x, out[1:-1], need


@pytest.mark.parametrize("name", tuple(J.TINIES))
def test_every_stream_row_against_float64(name):
    from marqo_amd.engine.jina_bert import JinaBertTower
    lib = L.load()
    b = J.build(name)
    arch = b["arch"]
    tower = JinaBertTower(arch, b["sd"], DEV, pooling="mean")
    lens = [len(s) for s in b["seqs"]]
    ids = torch.cat(b["seqs"])
    rows, nseq = sum(lens), len(lens)
    d_ids = ids.to(torch.int32).to(DEV).contiguous()
    cu_h = A.cu_seqlens(lens)
    d_cu = cu_h.to(DEV)
    worst = {}
    for layers in range(1, arch.layers + 1):
        ex = J.exact(arch, b["tensors"], ids.to(DEV), lens, layers)
        mo = J.model(arch, b["tensors"], ids.to(DEV), lens, layers)
        for pool in ("mean", "cls"):
            for normalize in (0, 1):
                cfg = type(tower.cfg).from_buffer_copy(tower.cfg)
                cfg.layers, cfg.pool = layers, _POOL[pool]
                x, pooled, _ = _call(lib, tower, cfg, d_ids, d_cu, cu_h, rows, nseq, normalize)
                rs = J.row_ratio(x, ex.final, mo.final)
                rp = J.row_ratio(pooled, ex.pooled[(pool, normalize)], mo.pooled[(pool, normalize)])
                print(f"JINA_RATIO {name} layers={layers} pool={pool} l2={normalize} stream={rs['ratio']:.3f} (row {rs['row']} col {rs['col']}) pooled={rp['ratio']:.3f}")
                worst[f"stream{layers}"] = max(worst.get(f"stream{layers}", 0.0), rs["ratio"])
                worst["pooled"] = max(worst.get("pooled", 0.0), rp["ratio"])
    print(f"JINA_WORST {name}: " + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= MARGIN, worst
    # every mutant of the model leaves the bar on these inputs, in the stream and in every pooled view (ex / mo: the full depth, from the last turn)
    for mut in J.MUTANTS:
        mm = J.model(arch, b["tensors"], ids.to(DEV), lens, mut=mut)
        rs = {"stream": J.row_ratio(mm.final, ex.final, mo.final)["ratio"]}
        rs.update({f"{k[0]}/l2={k[1]}": J.row_ratio(v, ex.pooled[k], mo.pooled[k])["ratio"] for k, v in mm.pooled.items()})
        print(f"JINA_MUTANT {name} {mut}: " + " ".join(f"{k}={v:.1f}" for k, v in rs.items()))
        assert min(rs.values()) > MARGIN, (mut, rs)


def test_a_700_token_sequence_streams_through_the_towers_attention():
    from marqo_amd.engine.jina_bert import JinaBertTower
    lib = L.load()
    b = J.build("TINY_2H")
    arch = b["arch"]
    lens = [700]
    assert lens[0] > J.LDS_KEYS[arch.head_dim]
    tower = JinaBertTower(arch, b["sd"], DEV, pooling="mean")
    ids = J.random_seqs(lens, arch.vocab, seed=11)[0]
    d_ids = ids.to(torch.int32).to(DEV).contiguous()
    cu_h = A.cu_seqlens(lens)
    ex = J.exact(arch, b["tensors"], ids.to(DEV), lens)
    mo = J.model(arch, b["tensors"], ids.to(DEV), lens)
    cfg = type(tower.cfg).from_buffer_copy(tower.cfg)
    x, pooled, _ = _call(lib, tower, cfg, d_ids, cu_h.to(DEV), cu_h, 700, 1, 1)
    rs = J.row_ratio(x, ex.final, mo.final)
    rp = J.row_ratio(pooled, ex.pooled[("mean", 1)], mo.pooled[("mean", 1)])
    print(f"JINA_RATIO TINY_2H lens=[700] stream={rs['ratio']:.3f} (row {rs['row']} col {rs['col']}) pooled={rp['ratio']:.3f}")
    assert max(rs["ratio"], rp["ratio"]) <= MARGIN


def test_a_workspace_one_byte_short_is_refused_and_nothing_is_written():
    from marqo_amd.engine.jina_bert import JinaBertTower
    lib = L.load()
    b = J.build("TINY_2H")
    tower = JinaBertTower(b["arch"], b["sd"], DEV, pooling="mean")
    lens = [len(s) for s in b["seqs"]]
    rows, nseq, W = sum(lens), len(lens), b["arch"].width
    d_ids = torch.cat(b["seqs"]).to(torch.int32).to(DEV).contiguous()
    cu_h = A.cu_seqlens(lens)
    d_cu = cu_h.to(DEV)
    need = lib.mq_jina_bert_workspace_bytes(C.byref(tower.cfg), rows, nseq)
    assert need >= rows * W * (4 + 2 + 2) + rows * max(3 * W, 2 * b["arch"].mlp_dim) * 2
    ws = torch.full((need,), 0xA5, dtype=torch.uint8, device=DEV)
    out = torch.full((nseq, W), float("nan"), dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    rc = lib.mq_encode_jina_bert(C.byref(tower.cfg), C.byref(tower.w), d_ids.data_ptr(), d_cu.data_ptr(), cu_h.data_ptr(), nseq, out.data_ptr(), 1,
                                 ws.data_ptr(), need - 1, _s())
    torch.cuda.synchronize()
    assert rc == -3 and b"mq_encode_jina_bert: workspace" in lib.mq_last_error(), f"a workspace one byte short: rc {rc}, not MQ_ERR_WORKSPACE"
    assert bool((ws == 0xA5).all()) and bool(out.isnan().all())


# ---- vectorise ------------------------------------------------------------------------------------------------------------------------------------------
TEXTS = ["hello world", "attention with linear biases favours the near keys", "a search engine ranks documents for a query " * 8, ""]
TOKENS = 48


@pytest.fixture(scope="module")
def ckpts(tmp_path_factory):
    """TINY_3H as a user brings it: config.json + model.safetensors (under the `bert.` prefix of the task-head classes) + a WordPiece tokenizer.json;
    one directory without 1_Pooling, one that names cls pooling"""
    b, tk = J.build("TINY_3H"), J.train_tokenizer()
    sd = {"bert." + k: v for k, v in b["sd"].items()}
    root = tmp_path_factory.mktemp("jina")
    return dict(mean=J.write_checkpoint_dir(str(root / "mean"), b["cfg"], sd, tk), cls=J.write_checkpoint_dir(str(root / "cls"), b["cfg"], sd, tk, pooling="cls"))


def _reference_rows(directory, pooling, normalize):
    from tokenizers import Tokenizer
    raw = Tokenizer.from_file(os.path.join(directory, "tokenizer.json"))
    raw.enable_truncation(max_length=TOKENS)
    rows = [torch.tensor(raw.encode(x).ids) for x in TEXTS]
    assert max(len(r) for r in rows) == TOKENS and min(len(r) for r in rows) == 2 and all(int(r[0]) == 2 and int(r[-1]) == 3 for r in rows)
    b = J.build("TINY_3H")
    ex = J.exact(b["arch"], b["tensors"], torch.cat(rows), [len(r) for r in rows])
    return ex.pooled[(pooling, 1 if normalize else 0)]


@pytest.mark.parametrize("pooling", ("mean", "cls"))
@pytest.mark.parametrize("normalize", (True, False))
def test_vectorise_from_a_local_directory(ckpts, monkeypatch, pooling, normalize):
    from marqo_amd.s2_inference import s2_inference as s2i
    monkeypatch.setenv("MARQO_MAX_CUDA_MODEL_MEMORY", "64")
    props = {"type": "hf", "name": ckpts[pooling], "dimensions": 192, "tokens": TOKENS, "trustRemoteCode": True}
    try:
        s2i.clear_loaded_models()
        out = torch.tensor(s2i.vectorise(f"jina-test-{pooling}", TEXTS, model_properties=props, device=DEV, normalize_embeddings=normalize), dtype=torch.float64)
    finally:
        s2i.clear_loaded_models()
    assert out.shape == (4, 192)
    ref = _reference_rows(ckpts[pooling], pooling, normalize)
    e = _err(out, ref)
    print(f"JINA_COS vectorise {pooling} normalize={normalize} against the float64 pass: " + " ".join(f"{float(v):.2e}" for v in e) + f" (bound {COS_TOL:.0e})")
    assert float(e.max()) < COS_TOL
    if normalize:
        np.testing.assert_allclose(out.norm(dim=-1).numpy(), 1.0, atol=1e-5)
    else:
        np.testing.assert_allclose(out.norm(dim=-1).numpy(), ref.norm(dim=-1).numpy(), rtol=2e-2)
    other = _reference_rows(ckpts[pooling], "cls" if pooling == "mean" else "mean", normalize)      # and the other pooling's rows are elsewhere
    assert float(_err(out, other)[:3].min()) > 10 * COS_TOL

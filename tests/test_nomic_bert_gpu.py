"""The NomicBERT tower on the GPU: NomicBertTower (mq_encode_nomic_bert through engine/nomic_bert.py) against the float64 pass of tests/nomic_bert_ref.py —
every row of the token stream after every block and the pooled rows — and `vectorise` (`hf`) against fp32 transformers (NomicBertModel, mean pool + L2,
on the same token ids).  The float64 pass itself is pinned to transformers' NomicBertModel in float64 by tests/test_nomic_bert_host.py.

Bars (those of tests/test_jina_bert_gpu.py):
  the stream (cfg.layers = 1 .. layers: the tower has no final norm, so the workspace's first slice holds the stream after block l) and the pooled rows:
  the worst row of  max(|got - exact|_2 / |model - exact|_2, |got - exact|_inf / |model - exact|_inf)  <= MARGIN = 4.0.  The yardstick is the float64
  bf16 model's own distance from `exact`; it is never derived from the kernel's output.  Each mutant of the model (rope_skipped, rope_on_v, gate_swapped,
  gelu_for_silu, ln_before_add, no_type_row, theta_10000) is shown, on the device and on the same inputs, to leave that bar in the stream and in every
  pooled view.
  `vectorise` against fp32 transformers: 1 - cos < 3e-4, the project's bf16 tower bar (COS_TOL).

The stream is read from the first slice of the workspace (off_x is the plan's first take); pooling that slice with mq_pool must reproduce d_out bit for
bit before any ratio is measured.

Lengths 1, 7, 64, 65 and 130 in one batch (64 / 65: the kernel's 64-query slice; 130: three slices, a ragged third key tile); one 700-token sequence
(past the 640 keys of the attention kernel's LDS image: K / V stream through in two pieces inside the tower).  Mean and CLS pooling, with and without L2.

Measured on an MI355X (NOMIC_RATIO / NOMIC_MUTANT / NOMIC_COS lines):
  worst row ratio, stream after block 1 / after block 2 / pooled mean / pooled cls: 1.41 / 1.55 / 1.11 / 1.28; the 700-token sequence: stream 1.93,
  pooled 1.07 (mean) 1.04 (cls) (bar 4.0).  The mutants on the device, smallest view: rope_skipped 85, rope_on_v 519, gate_swapped 121,
  gelu_for_silu 34, ln_before_add 1105, no_type_row 1312, theta_10000 88.  vectorise worst 1 - cos against fp32 transformers: 9.2e-7 (mean),
  1.3e-6 (cls) (bar 3e-4).
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from marqo_amd import _lib as L
from tests import attention_ref as A
from tests import nomic_bert_ref as N
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
    """one guarded mq_encode_nomic_bert call -> (stream x [rows, W], pooled [nseq, W], the workspace size)"""
    W = cfg.width
    need = lib.mq_nomic_bert_workspace_bytes(C.byref(cfg), rows, nseq)
    ws = torch.full((need + 4096,), 0xA5, dtype=torch.uint8, device=DEV)
    out = torch.full((nseq + 2, W), float("nan"), dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    L.check(lib.mq_encode_nomic_bert(C.byref(cfg), C.byref(tower.w), d_ids.data_ptr(), d_cu.data_ptr(), cu_h.data_ptr(), nseq, out[1:].data_ptr(), normalize,
                                     ws.data_ptr(), need, _s()), "mq_encode_nomic_bert")
    torch.cuda.synchronize()
    assert bool((ws[need:] == 0xA5).all()), "the workspace was written past mq_nomic_bert_workspace_bytes"
    assert bool(out[0].isnan().all()) and bool(out[-1].isnan().all()), "a guard row of d_out was written"
    x = ws[:rows * W * 4].view(torch.float32).view(rows, W)
    again = torch.empty(nseq, W, dtype=torch.float32, device=DEV)
    L.check(lib.mq_pool(x.data_ptr(), d_cu.data_ptr(), nseq, again.data_ptr(), W, cfg.pool, normalize, _s()), "mq_pool")
    torch.cuda.synchronize()
    assert torch.equal(again.view(torch.int32), out[1:-1].view(torch.int32)), "the stream is not the workspace's first slice: no parity was measured"
    assert bool(torch.isfinite(x).all())
    return x, out[1:-1], need


def test_every_stream_row_against_float64():
    from marqo_amd.engine.nomic_bert import NomicBertTower
    lib = L.load()
    b = N.build()
    arch = b["arch"]
    tower = NomicBertTower(arch, b["sd"], DEV, pooling="mean")
    lens = [len(s) for s in b["seqs"]]
    assert lens == [1, 7, 64, 65, 130]
    ids = torch.cat(b["seqs"])
    rows, nseq = sum(lens), len(lens)
    d_ids = ids.to(torch.int32).to(DEV).contiguous()
    cu_h = A.cu_seqlens(lens)
    d_cu = cu_h.to(DEV)
    worst = {}
    for layers in range(1, arch.layers + 1):
        ex = N.exact(arch, b["tensors"], ids.to(DEV), lens, layers)
        mo = N.model(arch, b["tensors"], ids.to(DEV), lens, layers)
        for pool in ("mean", "cls"):
            for normalize in (0, 1):
                cfg = type(tower.cfg).from_buffer_copy(tower.cfg)
                cfg.layers, cfg.pool = layers, _POOL[pool]
                x, pooled, _ = _call(lib, tower, cfg, d_ids, d_cu, cu_h, rows, nseq, normalize)
                rs = N.row_ratio(x, ex.final, mo.final)
                rp = N.row_ratio(pooled, ex.pooled[(pool, normalize)], mo.pooled[(pool, normalize)])
                print(f"NOMIC_RATIO layers={layers} pool={pool} l2={normalize} stream={rs['ratio']:.3f} (row {rs['row']} col {rs['col']}) pooled={rp['ratio']:.3f}")
                worst[f"stream{layers}"] = max(worst.get(f"stream{layers}", 0.0), rs["ratio"])
                worst[f"pooled_{pool}"] = max(worst.get(f"pooled_{pool}", 0.0), rp["ratio"])
    print("NOMIC_WORST: " + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= MARGIN, worst
    # every mutant of the model leaves the bar on these inputs, in the stream and in every pooled view (ex / mo: the full depth, from the last turn)
    for mut in N.MUTANTS:
        mm = N.model(arch, b["tensors"], ids.to(DEV), lens, mut=mut)
        rs = {"stream": N.row_ratio(mm.final, ex.final, mo.final)["ratio"]}
        rs.update({f"{k[0]}/l2={k[1]}": N.row_ratio(v, ex.pooled[k], mo.pooled[k])["ratio"] for k, v in mm.pooled.items()})
        print(f"NOMIC_MUTANT {mut}: " + " ".join(f"{k}={v:.1f}" for k, v in rs.items()))
        assert min(rs.values()) > MARGIN, (mut, rs)


def test_a_700_token_sequence_streams_through_the_towers_attention():
    from marqo_amd.engine.nomic_bert import NomicBertTower
    lib = L.load()
    b = N.build()
    arch = b["arch"]
    lens = [700]
    assert N.LDS_KEYS < lens[0] <= arch.max_pos
    ids = N.random_seqs(lens, arch.vocab, seed=11)[0]
    d_ids = ids.to(torch.int32).to(DEV).contiguous()
    cu_h = A.cu_seqlens(lens)
    ex = N.exact(arch, b["tensors"], ids.to(DEV), lens)
    mo = N.model(arch, b["tensors"], ids.to(DEV), lens)
    for pool in ("mean", "cls"):
        tower = NomicBertTower(arch, b["sd"], DEV, pooling=pool)
        cfg = type(tower.cfg).from_buffer_copy(tower.cfg)
        x, pooled, _ = _call(lib, tower, cfg, d_ids, cu_h.to(DEV), cu_h, 700, 1, 1)
        rs = N.row_ratio(x, ex.final, mo.final)
        rp = N.row_ratio(pooled, ex.pooled[(pool, 1)], mo.pooled[(pool, 1)])
        print(f"NOMIC_RATIO lens=[700] pool={pool} stream={rs['ratio']:.3f} (row {rs['row']} col {rs['col']}) pooled={rp['ratio']:.3f}")
        assert max(rs["ratio"], rp["ratio"]) <= MARGIN


def test_both_tensor_namings_give_bit_identical_embeddings():
    from marqo_amd.engine.nomic_bert import NomicBertTower
    b = N.build()
    lens = [len(s) for s in b["seqs"]]
    S = max(lens)
    ids = torch.zeros(len(lens), S, dtype=torch.int64)
    mask = torch.zeros(len(lens), S, dtype=torch.int64)
    for i, s in enumerate(b["seqs"]):
        ids[i, :len(s)], mask[i, :len(s)] = s, 1
    outs = []
    for sd in (b["sd"], b["hub_sd"]):
        tower = NomicBertTower(b["arch"], sd, DEV, pooling="mean")
        outs.append(tower.encode_ids(ids, mask, normalize=True).clone())
    torch.cuda.synchronize()
    assert bool(torch.isfinite(outs[0]).all()) and torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))


def test_a_workspace_one_byte_short_is_refused_and_nothing_is_written():
    from marqo_amd.engine.nomic_bert import NomicBertTower
    lib = L.load()
    b = N.build()
    tower = NomicBertTower(b["arch"], b["sd"], DEV, pooling="mean")
    lens = [len(s) for s in b["seqs"]]
    rows, nseq, W = sum(lens), len(lens), b["arch"].width
    d_ids = torch.cat(b["seqs"]).to(torch.int32).to(DEV).contiguous()
    cu_h = A.cu_seqlens(lens)
    d_cu = cu_h.to(DEV)
    need = lib.mq_nomic_bert_workspace_bytes(C.byref(tower.cfg), rows, nseq)
    assert need >= rows * W * (4 + 2 + 2) + rows * max(3 * W, 2 * b["arch"].mlp_dim) * 2
    ws = torch.full((need,), 0xA5, dtype=torch.uint8, device=DEV)
    out = torch.full((nseq, W), float("nan"), dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    rc = lib.mq_encode_nomic_bert(C.byref(tower.cfg), C.byref(tower.w), d_ids.data_ptr(), d_cu.data_ptr(), cu_h.data_ptr(), nseq, out.data_ptr(), 1,
                                  ws.data_ptr(), need - 1, _s())
    torch.cuda.synchronize()
    assert rc == -3 and b"mq_encode_nomic_bert: workspace" in lib.mq_last_error(), f"a workspace one byte short: rc {rc}, not MQ_ERR_WORKSPACE"
    assert bool((ws == 0xA5).all()) and bool(out.isnan().all())


# ---- vectorise ------------------------------------------------------------------------------------------------------------------------------------------
TEXTS = ["hello world", "rotary positions turn every pair of dimensions by the token's index", "a search engine ranks documents for a query " * 8, ""]
TOKENS = 48


@pytest.fixture(scope="module")
def ckpts(tmp_path_factory):
    """the tiny checkpoint as a user brings it: the directory transformers' save_pretrained writes + a WordPiece tokenizer.json (no 1_Pooling: mean), and
    the hub's original tensor names behind a GPT-2-style config.json with a 1_Pooling that names cls"""
    b, tk = N.build(), N.train_tokenizer()
    root = tmp_path_factory.mktemp("nomic")
    return dict(mean=N.save_pretrained_dir(str(root / "mean"), b["model"], tk),
                cls=N.write_checkpoint_dir(str(root / "cls"), N.hub_config(), b["hub_sd"], tk, pooling="cls"))


def _transformers_rows(directory, pooling, normalize):
    """fp32 transformers on the `tokenizers` library's ids, one text at a time (no padding): mean / first row of last_hidden_state (+ L2)"""
    from tokenizers import Tokenizer
    raw = Tokenizer.from_file(os.path.join(directory, "tokenizer.json"))
    raw.enable_truncation(max_length=TOKENS)
    rows = [torch.tensor(raw.encode(x).ids) for x in TEXTS]
    assert max(len(r) for r in rows) == TOKENS and min(len(r) for r in rows) == 2 and all(int(r[0]) == 2 and int(r[-1]) == 3 for r in rows)
    m = N.build()["model"].float()
    out = []
    with torch.no_grad():
        for r in rows:
            hs = m(input_ids=r[None]).last_hidden_state[0]
            assert hs.dtype == torch.float32
            v = hs.mean(0) if pooling == "mean" else hs[0]
            out.append(v / v.norm() if normalize else v)
    return torch.stack(out).double()


def test_the_hf_loader_loads_the_directory(ckpts, monkeypatch):
    """(refused on the commit before this family was served: model_type=nomic_bert is not a BERT-family encoder)"""
    from marqo_amd.engine.nomic_bert import NomicBertTower
    from marqo_amd.s2_inference.hugging_face_model import HuggingFaceModel
    m = HuggingFaceModel(model_properties={"type": "hf", "name": ckpts["mean"], "dimensions": 128, "tokens": TOKENS}, device=DEV)
    m._load_necessary_components()
    assert isinstance(m._model, NomicBertTower) and m._pooling_func == "mean" and m._model.arch.rope_theta == 1000.0


@pytest.mark.parametrize("pooling", ("mean", "cls"))
@pytest.mark.parametrize("normalize", (True, False))
def test_vectorise_from_a_local_directory(ckpts, monkeypatch, pooling, normalize):
    from marqo_amd.s2_inference import s2_inference as s2i
    monkeypatch.setenv("MARQO_MAX_CUDA_MODEL_MEMORY", "64")
    props = {"type": "hf", "name": ckpts[pooling], "dimensions": 128, "tokens": TOKENS}
    try:
        s2i.clear_loaded_models()
        out = torch.tensor(s2i.vectorise(f"nomic-test-{pooling}", TEXTS, model_properties=props, device=DEV, normalize_embeddings=normalize), dtype=torch.float64)
    finally:
        s2i.clear_loaded_models()
    assert out.shape == (4, 128)
    ref = _transformers_rows(ckpts[pooling], pooling, normalize)
    e = _err(out, ref)
    print(f"NOMIC_COS vectorise {pooling} normalize={normalize} against fp32 transformers: " + " ".join(f"{float(v):.2e}" for v in e) + f" (bound {COS_TOL:.0e})")
    assert float(e.max()) < COS_TOL
    if normalize:
        np.testing.assert_allclose(out.norm(dim=-1).numpy(), 1.0, atol=1e-5)
    else:
        np.testing.assert_allclose(out.norm(dim=-1).numpy(), ref.norm(dim=-1).numpy(), rtol=2e-2)
    other = _transformers_rows(ckpts[pooling], "cls" if pooling == "mean" else "mean", normalize)      # and the other pooling's rows are elsewhere
    assert float(_err(out, other)[:3].min()) > 10 * COS_TOL

"""The Jina v3 tower on the GPU: JinaV3Tower (mq_encode_jina_v3 through engine/jina_v3.py) against the float64 pass of tests/jina_v3_ref.py — every row
of the token stream and the pooled rows of ONE batch that mixes three task adapters and a sequence without adapter — and `vectorise` (`hf`, loraTask)
against fp32 transformers with the adapter merged into its weights.  The float64 pass itself is pinned to transformers' JinaEmbeddingsV3Model (base and
merged) in float64 by tests/test_jina_v3_host.py.

Bars (those of tests/test_nomic_bert_gpu.py):
  the stream (the workspace's first slice) and the pooled rows: the worst row of  max(|got - exact|_2 / |model - exact|_2, |got - exact|_inf /
  |model - exact|_inf)  <= MARGIN = 4.0.  The yardstick is the float64 bf16 model's own distance from `exact`; it is never derived from the kernel's output.
  `vectorise` against fp32 transformers: 1 - cos < 3e-4, the project's bf16 tower bar (COS_TOL).

Lengths 1, 64, 65 and 700 in one batch (64 / 65: the attention kernel's 64-query slice and the LoRA kernels' tile edges; 700: past the 640 keys of the
attention kernel's LDS image) with the tasks retrieval.query, classification, none, retrieval.passage.  The sequence without adapter must come out of the
mixed batch with the bits it has in a batch where nobody has an adapter.

Measured on an MI355X (JINA3_RATIO / JINA3_COS lines): the mixed batch, worst row ratio stream 3.06, pooled mean 1.35, pooled cls 1.11; the same
batch with no adapter anywhere 1.68; a tower without adapters 1.77 (stream) 1.09 (pooled) (bar 4.0); the base model on the adapter rows 768.  vectorise
worst 1 - cos against fp32 transformers: 8.7e-6 (loraTask retrieval.passage, merged weights), 1.1e-6 (base) (bar 3e-4)."""
import ctypes as C
import os

import pytest
import torch

from marqo_amd import _lib as L
from tests import attention_ref as A
from tests import jina_v3_ref as N
from tests.test_modernbert_gpu import COS_TOL
from tests.test_patch_attn_gpu import MARGIN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LENS = [1, 64, 65, 700]
TASKS = ["retrieval.query", "classification", None, "retrieval.passage"]


def _s():
    return torch.cuda.current_stream().cuda_stream


def _call(lib, tower, d_ids, cu_h, tasks, normalize, pool):
    """one guarded mq_encode_jina_v3 call -> (stream x [rows, W], pooled [nseq, W])"""
    cfg = type(tower.cfg).from_buffer_copy(tower.cfg)
    cfg.pool = pool
    W, rows, nseq = cfg.width, int(cu_h[-1]), cu_h.numel() - 1
    d_cu = cu_h.to(DEV)
    th = torch.from_numpy(tower.task_ids(tasks, nseq))
    d_task = th.to(DEV)
    need = lib.mq_jina_v3_workspace_bytes(C.byref(cfg), rows, nseq)
    ws = torch.full((need + 4096,), 0xA5, dtype=torch.uint8, device=DEV)
    out = torch.full((nseq + 2, W), float("nan"), dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    L.check(lib.mq_encode_jina_v3(C.byref(cfg), C.byref(tower.w), C.byref(tower.lora) if tower.lora is not None else None, d_ids.data_ptr(), d_cu.data_ptr(),
                                  cu_h.data_ptr(), d_task.data_ptr(), th.data_ptr(), nseq, out[1:].data_ptr(), normalize, ws.data_ptr(), need, _s()),
            "mq_encode_jina_v3")
    torch.cuda.synchronize()
    assert bool((ws[need:] == 0xA5).all()), "the workspace was written past mq_jina_v3_workspace_bytes"
    assert bool(out[0].isnan().all()) and bool(out[-1].isnan().all()), "a guard row of d_out was written"
    x = ws[:rows * W * 4].view(torch.float32).view(rows, W).clone()
    again = torch.empty(nseq, W, dtype=torch.float32, device=DEV)
    L.check(lib.mq_pool(x.data_ptr(), d_cu.data_ptr(), nseq, again.data_ptr(), W, cfg.pool, normalize, _s()), "mq_pool")
    torch.cuda.synchronize()
    assert torch.equal(again.view(torch.int32), out[1:-1].view(torch.int32)), "the stream is not the workspace's first slice: no parity was measured"
    assert bool(torch.isfinite(x).all())
    return x, out[1:-1].clone()


@pytest.fixture(scope="module")
def batch():
    b = N.build()
    ids = torch.cat(N.random_seqs(LENS, b["cfg"]["vocab_size"], seed=3))
    return dict(b=b, ids=ids, d_ids=ids.to(torch.int32).to(DEV).contiguous(), cu_h=A.cu_seqlens(LENS))


def test_a_mixed_batch_against_float64_and_the_no_adapter_sequence_bit_for_bit(batch):
    from marqo_amd.engine.jina_v3 import JinaV3Tower
    lib = L.load()
    b = batch["b"]
    arch = b["arch"]
    tower = JinaV3Tower(arch, b["sd"], DEV, pooling="mean", adapters=b["lora"])
    tid = [int(t) for t in tower.task_ids(TASKS, len(LENS))]
    assert sorted(tid) == [-1, 0, 1, 3] or len(set(tid)) == 4
    args = (arch, b["tensors"], b["lora"].t, batch["ids"].to(DEV), LENS, tid)
    ex, mo = N.exact(*args), N.model(*args)
    base = N.exact(arch, b["tensors"], None, batch["ids"].to(DEV), LENS, None)
    worst = {}
    for pool in ("mean", "cls"):
        for normalize in (0, 1):
            x, pooled = _call(lib, tower, batch["d_ids"], batch["cu_h"], TASKS, normalize, L.MQ_POOL_MEAN if pool == "mean" else L.MQ_POOL_CLS)
            rs = N.row_ratio(x, ex.final, mo.final)
            rp = N.row_ratio(pooled, ex.pooled[(pool, normalize)], mo.pooled[(pool, normalize)])
            print(f"JINA3_RATIO mixed pool={pool} l2={normalize} stream={rs['ratio']:.3f} (row {rs['row']} col {rs['col']}) pooled={rp['ratio']:.3f}")
            worst["stream"] = max(worst.get("stream", 0.0), rs["ratio"])
            worst[f"pooled_{pool}"] = max(worst.get(f"pooled_{pool}", 0.0), rp["ratio"])
    print("JINA3_WORST: " + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= MARGIN, worst
    # the base model on the adapter rows is far outside the bar (the adapters are not a perturbation the bar would absorb) ...
    r0 = sum(LENS[:3])
    far = N.row_ratio(base.final[r0:], ex.final[r0:], mo.final[r0:])["ratio"]
    print(f"JINA3_RATIO the base model on the adapter rows: {far:.1f}")
    assert far > 10 * MARGIN
    # ... and the sequence without adapter has, in the mixed batch, the bits of a batch where nobody has an adapter
    xm, pm = _call(lib, tower, batch["d_ids"], batch["cu_h"], TASKS, 1, L.MQ_POOL_MEAN)
    xb, pb = _call(lib, tower, batch["d_ids"], batch["cu_h"], [None] * 4, 1, L.MQ_POOL_MEAN)
    a, z = sum(LENS[:2]), sum(LENS[:3])
    assert torch.equal(xm[a:z].view(torch.int32), xb[a:z].view(torch.int32)) and torch.equal(pm[2].view(torch.int32), pb[2].view(torch.int32))
    assert not torch.equal(xm[z:].view(torch.int32), xb[z:].view(torch.int32))
    rb = N.row_ratio(xb, base.final, N.model(arch, b["tensors"], b["lora"].t, batch["ids"].to(DEV), LENS, [-1] * 4).final)
    print(f"JINA3_RATIO nobody has an adapter: stream={rb['ratio']:.3f}")
    assert rb["ratio"] <= MARGIN


def test_a_tower_without_adapters_is_the_base_model(batch):
    from marqo_amd.engine.jina_v3 import JinaV3Tower
    lib = L.load()
    b = batch["b"]
    arch = b["arch"]
    tower = JinaV3Tower(arch, b["sd"], DEV, pooling="mean")
    assert tower.lora is None
    ex = N.exact(arch, b["tensors"], None, batch["ids"].to(DEV), LENS, None)
    mo = N.model(arch, b["tensors"], None, batch["ids"].to(DEV), LENS, None)
    x, pooled = _call(lib, tower, batch["d_ids"], batch["cu_h"], None, 1, L.MQ_POOL_MEAN)
    rs, rp = N.row_ratio(x, ex.final, mo.final), N.row_ratio(pooled, ex.pooled[("mean", 1)], mo.pooled[("mean", 1)])
    print(f"JINA3_RATIO base stream={rs['ratio']:.3f} pooled={rp['ratio']:.3f}")
    assert max(rs["ratio"], rp["ratio"]) <= MARGIN
    with pytest.raises(ValueError, match="unknown LoRA task 'separation': this checkpoint has no adapters"):
        tower.task_ids(["separation"], 1)


def test_encode_takes_one_task_per_sequence(batch):
    from marqo_amd.engine.jina_v3 import JinaV3Tower
    b = batch["b"]
    tower = JinaV3Tower(b["arch"], b["sd"], DEV, pooling="mean", adapters=b["lora"], default_task="separation")
    seqs = N.random_seqs([5, 9, 3], b["cfg"]["vocab_size"], seed=4)
    ids = torch.ones(3, 9, dtype=torch.int64)
    mask = torch.zeros(3, 9, dtype=torch.int64)
    for i, s in enumerate(seqs):
        ids[i, :len(s)], mask[i, :len(s)] = s, 1
    mixed = tower.encode(ids, mask, tasks=["retrieval.query", None, "separation"])
    default = tower.encode_ids(ids, mask)
    none = tower.encode(ids, mask, tasks=[None] * 3)
    torch.cuda.synchronize()
    assert torch.equal(mixed[2], default[2]) and torch.equal(mixed[1], none[1])
    assert not torch.equal(mixed[0], default[0]) and not torch.equal(default[1], none[1])
    with pytest.raises(ValueError, match="unknown LoRA task 'summarise'"):
        tower.encode(ids, mask, tasks=["summarise", None, None])


# ---- vectorise ------------------------------------------------------------------------------------------------------------------------------------------
TEXTS = ["hello world", "low rank adapters change a linear map by a thin product", "queries and passages share one batch " * 8, ""]
TOKENS = 48


@pytest.fixture(scope="module")
def ckpt(tmp_path_factory):
    """the tiny checkpoint as a user brings it: the directory transformers' save_pretrained writes + a unigram tokenizer.json + one PEFT folder per task"""
    b, tk = N.build(), N.train_tokenizer()
    d = str(tmp_path_factory.mktemp("jina3") / "ckpt")
    b["model"].save_pretrained(d)
    N.write_tokenizer(d, tk)
    for task in N.TASKS:
        N.write_adapter_dir(os.path.join(d, task), b["adapters"][task])
    return d


def _transformers_rows(directory, task, normalize):
    """fp32 transformers with the task's adapter merged, on the `tokenizers` library's ids, one text at a time (no padding): mean of last_hidden_state"""
    from tokenizers import Tokenizer
    raw = Tokenizer.from_file(os.path.join(directory, "tokenizer.json"))
    raw.enable_truncation(max_length=TOKENS)
    rows = [torch.tensor(raw.encode(x).ids) for x in TEXTS]
    assert max(len(r) for r in rows) == TOKENS and min(len(r) for r in rows) == 2 and all(int(r[0]) == 0 and int(r[-1]) == 2 for r in rows)
    b = N.build()
    m = N.merged_model(b["model"], b["adapters"][task] if task else None, dtype=torch.float32)
    out = []
    with torch.no_grad():
        for r in rows:
            v = m(input_ids=r[None]).last_hidden_state[0].mean(0)
            out.append(v / v.norm() if normalize else v)
    return torch.stack(out).double()


def _err(out, ref):
    return 1 - (out * ref).sum(-1) / (out.norm(dim=-1) * ref.norm(dim=-1))


@pytest.mark.parametrize("task", ("retrieval.passage", None))
def test_vectorise_from_a_local_directory(ckpt, monkeypatch, task):
    from marqo_amd.s2_inference import s2_inference as s2i
    monkeypatch.setenv("MARQO_MAX_CUDA_MODEL_MEMORY", "64")
    props = {"type": "hf", "name": ckpt, "dimensions": 128, "tokens": TOKENS}
    if task:
        props["loraTask"] = task
    try:
        s2i.clear_loaded_models()
        out = torch.tensor(s2i.vectorise(f"jina3-test-{task}", TEXTS, model_properties=props, device=DEV, normalize_embeddings=True), dtype=torch.float64)
    finally:
        s2i.clear_loaded_models()
    assert out.shape == (4, 128)
    ref = _transformers_rows(ckpt, task, True)
    e = _err(out, ref)
    print(f"JINA3_COS vectorise loraTask={task} against fp32 transformers (merged): " + " ".join(f"{float(v):.2e}" for v in e) + f" (bound {COS_TOL:.0e})")
    assert float(e.max()) < COS_TOL
    other = _transformers_rows(ckpt, None if task else "retrieval.passage", True)      # and the other model's rows are elsewhere
    assert float(_err(out, other).min()) > 10 * COS_TOL

"""The Qwen3 / Qwen2 row kernels and tower on the GPU: mq_rmsnorm and mq_qk_norm_rope against float64, QwenTower (mq_encode_qwen through engine/qwen.py)
against the project's fp32 oracle (tests/qwen_ref.py, itself equal to transformers' Qwen3Model / Qwen2Model to fp32 round-off: tests/test_qwen_host.py),
and `vectorise` from a local checkpoint directory.

Budgets (u = 2**-24, margin 1.25 as in tests/test_rowops_gpu.py for the terms a derivation neglects):
  mq_rmsnorm, fp32 output: |y| (D / 2 + 7) u with D = ceil(W / 64) + 8, the longest chain of additions of the sum of squares (rowops_ref.chain): the sum
      has only positive terms, so D u relative, halved by the square root; 4 u for the squaring, the divide, the add of eps and rsqrtf; 3 u for the two
      products and one spare.  bf16 output: that plus half a bf16 ulp of the reference value (one rounding).
  mq_qk_norm_rope: with (a, b) the normalised pair a lane rotates and hyp = sqrt(a^2 + b^2): hyp (t f + 24) u + half a bf16 ulp.  t f u is the fp32
      product float(t) * inv_freq[i] (relative u on an angle of up to 8191 rad: 4.9e-4 rad at t = 8191, f = 1; a rotation moves a point by hyp per
      radian); 24 u covers the head's RMS (HD / 4-term chains and five butterfly levels, halved: <= 8 u), sincosf (<= 4 u), the norm's two products and the
      rotation's three operations (<= 6 u), and a spare.  The reference forms the angle in float64 from the fp32 inv_freq, so the test sees the kernel's
      angle error, and rounds nothing before the end, as the kernel.
  tower: 1 - cos < 3e-4 on the pooled rows, the project's bf16 tower bar (tests/test_modernbert_gpu.py).

Measured values are printed as `QWEN_RATIO` / `QWEN_COS` lines.  On an MI355X: mq_rmsnorm 0.26 (fp32 output) / 1.00 (bf16 output: the half ulp itself) of
the budget; mq_qk_norm_rope 1.00, positions up to 8191 included; tower max 1 - cos 9.3e-6 (TINY64, mean pooling); vectorise against transformers 8.7e-6."""
import math
import os

import numpy as np
import pytest
import torch

from marqo_amd import _lib as L
from marqo_amd.engine import archs
from tests import qwen_ref as Q
from tests import rowops_ref as RR
from tests.test_modernbert_gpu import COS_TOL

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MARGIN = 1.25
U = 2.0 ** -24


@pytest.fixture(scope="module")
def lib():
    return L.load()


def _s():
    return torch.cuda.current_stream().cuda_stream


# ---- mq_rmsnorm ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", (4, 256, 896, 2048))
@pytest.mark.parametrize("rows", (1, 67))
def test_rmsnorm_against_float64(lib, W, rows):
    eps = 1e-6
    for fam in ("randn", "rowscale"):
        x, g, _ = RR.make_rows(fam, 80, W, seed=3, device="cuda")
        for idx in (None, torch.randperm(80, device="cuda")[:rows].to(torch.int32)):
            xs = x[:rows] if idx is None else x[idx.long()]
            y = xs.double() * torch.rsqrt(xs.double().pow(2).mean(-1, keepdim=True) + eps) * g.double()
            B = y.abs() * (RR.chain(W) / 2 + 7) * U
            ob = torch.full((rows + 2, W), float("nan"), dtype=torch.bfloat16, device="cuda")
            of = torch.full((rows + 2, W), float("nan"), dtype=torch.float32, device="cuda")
            L.check(lib.mq_rmsnorm(x.data_ptr(), L.ptr(idx), g.data_ptr(), ob[1:].data_ptr(), of[1:].data_ptr(), rows, W, eps, _s()), "mq_rmsnorm")
            torch.cuda.synchronize()
            assert bool(ob[0].isnan().all()) and bool(ob[-1].isnan().all()) and bool(of[0].isnan().all()) and bool(of[-1].isnan().all())
            rf, rb = RR.ratio(of[1:-1], y, B), RR.ratio(ob[1:-1], y, B + RR.half_ulp_bf16(y))
            print(f"QWEN_RATIO rmsnorm family={fam} rows={rows} W={W} gather={idx is not None} fp32_out={rf:.4f} bf16_out={rb:.4f}")
            assert rf <= MARGIN and rb <= MARGIN
            # either output alone, and in place on the fp32 rows (the tower's mean-pooling tail)
            only = torch.empty(rows, W, dtype=torch.float32, device="cuda")
            L.check(lib.mq_rmsnorm(x.data_ptr(), L.ptr(idx), g.data_ptr(), None, only.data_ptr(), rows, W, eps, _s()), "mq_rmsnorm")
            assert torch.equal(only, of[1:-1])
            if idx is None:
                inplace = x[:rows].clone()
                L.check(lib.mq_rmsnorm(inplace.data_ptr(), None, g.data_ptr(), None, inplace.data_ptr(), rows, W, eps, _s()), "mq_rmsnorm")
                assert torch.equal(inplace, of[1:-1])


# ---- mq_qk_norm_rope ----------------------------------------------------------------------------------------------------------------------------------
def _qk_reference(qkv, lens, Qh, KV, hd, qg, kg, eps, inv_freq):
    """float64 from the bf16 input: (y, budget) over the q and k columns [rows, (Qh + KV) hd]"""
    rows = qkv.shape[0]
    x = qkv[:, :(Qh + KV) * hd].double().reshape(rows, Qh + KV, hd)
    if qg is not None:
        gam = torch.cat([qg.double()[None].expand(Qh, hd), kg.double()[None].expand(KV, hd)])[None]
        x = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * gam
    t = torch.cat([torch.arange(ln, device=qkv.device) for ln in lens]).double()
    ang = t[:, None] * inv_freq.double()[None, :]                          # [rows, hd / 2]: exact product of the fp32 frequencies
    cos, sin = ang.cos()[:, None, :], ang.sin()[:, None, :]
    a, b = x[..., :hd // 2], x[..., hd // 2:]
    y = torch.cat([a * cos - b * sin, b * cos + a * sin], dim=-1)
    hyp = (a * a + b * b).sqrt()
    bound = hyp * (ang.abs()[:, None, :] + 24.0) * U
    B = torch.cat([bound, bound], dim=-1) + RR.half_ulp_bf16(y)
    return y.reshape(rows, -1), B.reshape(rows, -1)


def _qk_case(lib, tag, lens, Qh, KV, hd, norm, theta, fixed=False):
    g = torch.Generator().manual_seed(hd + Qh + len(lens))
    rows, wq = sum(lens), (Qh + KV) * hd
    qkv = (torch.randn(rows, (Qh + 2 * KV) * hd, generator=g) * 2.0).to(torch.bfloat16).to("cuda")
    qg = (1.0 + 0.3 * torch.randn(hd, generator=g)).to("cuda") if norm else None
    kg = (1.0 + 0.3 * torch.randn(hd, generator=g)).to("cuda") if norm else None
    inv = (1.0 / (theta ** (torch.arange(0, hd, 2, dtype=torch.int64).float() / hd))).to("cuda")
    eps = 1e-6
    y, B = _qk_reference(qkv, lens, Qh, KV, hd, qg, kg, eps, inv)
    work = qkv.clone()
    cu = None if fixed else torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32, device="cuda")
    L.check(lib.mq_qk_norm_rope(work.data_ptr(), L.ptr(cu), len(lens), lens[0] if fixed else 0, Qh, KV, hd, L.ptr(qg), L.ptr(kg), eps, inv.data_ptr(), _s()),
            "mq_qk_norm_rope")
    torch.cuda.synchronize()
    assert torch.equal(work[:, wq:].view(torch.int16), qkv[:, wq:].view(torch.int16)), "V was touched"
    r = RR.ratio(work[:, :wq], y, B)
    print(f"QWEN_RATIO qk_norm_rope {tag} lens={lens if len(lens) < 6 else len(lens)} heads=({Qh},{KV},{hd}) norm={norm} ratio={r:.4f}")
    assert r <= MARGIN


@pytest.mark.parametrize("hd", (64, 128))
@pytest.mark.parametrize("norm", (True, False))
def test_qk_norm_rope_against_float64(lib, hd, norm):
    _qk_case(lib, "packed", [1, 17, 70], 4, 2, hd, norm, 1e6)
    _qk_case(lib, "packed", [1, 17, 70], 7, 1, hd, norm, 1e4)        # (an odd number of (row, head) units: ragged last step of a block)
    _qk_case(lib, "fixed", [33, 33, 33], 4, 2, hd, norm, 1e4, fixed=True)


@pytest.mark.parametrize("hd", (64, 128))
def test_qk_norm_rope_at_positions_up_to_8191(lib, hd):
    _qk_case(lib, "long", [8192], 1, 1, hd, True, 1e6)
    _qk_case(lib, "long", [8192], 1, 1, hd, False, 1e4)


# ---- the tower ------------------------------------------------------------------------------------------------------------------------------------------
def _err(out, ref):
    out = out.double().cpu()
    return 1 - (out * ref).sum(-1) / (out.norm(dim=-1) * ref.norm(dim=-1))


@pytest.fixture(scope="module")
def tinies():
    out = {}
    for i, (name, cfg) in enumerate(Q.TINIES.items()):
        model = Q.hf_model(cfg, seed=i + 1)
        arch = archs.bert_arch_from_hf_config(cfg)
        sd = Q.state_dict_of(model)
        seqs = Q.random_seqs([1, 17, 70, 129], cfg["vocab_size"], seed=3)
        out[name] = dict(cfg=cfg, model=model, arch=arch, sd=sd, seqs=seqs, hidden=Q.oracle_hidden_packed(sd, arch, seqs))
    return out


@pytest.mark.parametrize("name", tuple(Q.TINIES))
@pytest.mark.parametrize("pooling", ("last", "mean"))
def test_tiny_tower_against_the_oracle(tinies, name, pooling):
    """3 layers; TINY3: 4 query / 2 K/V heads of 128 with qk-norm, TINY2: 4 / 1 heads of 64 with QKV biases, TINY64: 4 x 64 != width 128; lengths 1, 17, 70
    and 129 (two query slices) in one packed call; a permuted batch gives the permuted rows bit for bit"""
    from marqo_amd.engine.qwen import QwenTower
    t = tinies[name]
    tower = QwenTower(t["arch"], t["sd"], DEV, pooling=pooling)
    ids, mask = Q.pad_batch(t["seqs"])
    for normalize in (True, False):
        out = tower.encode_ids(ids, mask, normalize=normalize)
        ref = Q.pooled(t["hidden"], pooling, normalize)
        e = _err(out, ref)
        print(f"QWEN_COS {name} {pooling} normalize={normalize}: " + " ".join(f"{float(v):.2e}" for v in e) + f" (bound {COS_TOL:.0e})")
        assert float(e.max()) < COS_TOL, (name, pooling, e.tolist())
        norms = out.double().cpu().norm(dim=-1)
        if normalize:
            np.testing.assert_allclose(norms.numpy(), 1.0, atol=1e-5)
        else:
            np.testing.assert_allclose(norms.numpy(), ref.norm(dim=-1).numpy(), rtol=2e-2)
        perm = torch.tensor([2, 0, 3, 1])
        assert torch.equal(tower.encode_ids(ids[perm], mask[perm], normalize=normalize), out[perm])


def test_vectorise_from_a_local_directory(tinies, tmp_path, monkeypatch):
    from tokenizers import Tokenizer
    from marqo_amd.engine.qwen import QwenTower
    from marqo_amd.s2_inference import s2_inference as s2i
    t = tinies["TINY3"]
    d = Q.write_checkpoint_dir(str(tmp_path / "ckpt"), t["cfg"], {"model." + k: v for k, v in t["sd"].items()}, Q.train_tokenizer())
    monkeypatch.setenv("MARQO_MAX_CUDA_MODEL_MEMORY", "64")
    props = {"type": "hf", "name": d, "dimensions": 256, "tokens": 64}
    texts = ["hello world", "grouped query attention shares keys and values", "a search engine ranks documents for a query " * 8, ""]
    raw = Tokenizer.from_file(os.path.join(d, "tokenizer.json"))
    raw.enable_truncation(max_length=64)
    rows = [torch.tensor(raw.encode(x).ids) for x in texts]
    assert max(len(r) for r in rows) == 64 and min(len(r) for r in rows) == 1 and all(int(r[-1]) == 0 for r in rows)
    try:
        s2i.clear_loaded_models()
        out = torch.tensor(s2i.vectorise("qwen3-test", texts, model_properties=props, device=DEV), dtype=torch.float64)
    finally:
        s2i.clear_loaded_models()
    assert out.shape == (4, 256)
    np.testing.assert_allclose(out.norm(dim=-1).numpy(), 1.0, atol=1e-5)
    ids, mask = Q.pad_batch(rows)
    direct = QwenTower(t["arch"], t["sd"], DEV, pooling="last").encode_ids(ids, mask).double().cpu()
    assert torch.equal(out, direct)
    with torch.no_grad():      # transformers on the CPU: right-padded batch, the last real token of every row
        hid = t["model"](input_ids=ids, attention_mask=mask).last_hidden_state
    ref = torch.stack([hid[i, len(r) - 1].double() for i, r in enumerate(rows)])
    e = _err(out, ref)
    print("QWEN_COS vectorise against transformers: " + " ".join(f"{float(v):.2e}" for v in e) + f" (bound {COS_TOL:.0e})")
    assert float(e.max()) < COS_TOL

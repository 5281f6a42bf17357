"""mq_rmsnorm_add_norm_wide against float64, and Gemma2Tower (mq_encode_gemma2) and `vectorise` from a written checkpoint directory against the seeded tiny
float64 transformers Gemma2Models of tests/test_gemma2_host.py (which shows that removing the cap or widening the window moves these rows by > 10 x the bar).
Row kernel: the budgets of tests/test_gemma_gpu.py::test_rmsnorm_add_norm_against_float64 (derived in that file's docstring) with D the new kernel's own
longest chain of additions: a lane adds its ceil(W / 256) chunk terms one after the other, each ((a^2 + b^2) + (c^2 + d^2)) two additions deep, and the
butterfly has six levels — D = ceil(W / 256) + 8 <= 24 (rowops_ref.chain(W) = ceil(W / 64) + 8 would be the wider bound).  At W = 2048 the call is
mq_rmsnorm_add_norm's, bit for bit.  Tower: 1 - cos < COS_TOL on the pooled rows.
Measured on an MI355X: row kernel 0.98 (stream) / 1.00 (bf16 output); tower worst 1 - cos 1.7e-5, vectorise 7.8e-6."""
import copy
import math

import pytest
import torch

from marqo_amd import _lib as L
from marqo_amd.engine import archs
from tests import gemma_ref as G
from tests import rowops_ref as RR
from tests import test_gemma2_host as G2
from tests.test_modernbert_gpu import COS_TOL

pytestmark = pytest.mark.gpu

DEV, MARGIN, U, EPS = "cuda:0", 1.25, 2.0 ** -24, 1e-6


def _add_norm(name, x, o, g1, g2, h, W):   # x, h: [rows + 1, W] slices whose last row is a NaN guard (as is the row in front of them)
    L.check(getattr(L.load(), name)(x.data_ptr(), o.data_ptr(), g1.data_ptr(), L.ptr(g2), L.ptr(h), o.shape[0], W, EPS, torch.cuda.current_stream().cuda_stream), name)
    torch.cuda.synchronize()


def _rows(fam, rows, W):
    x0, g1, _ = RR.make_rows(fam, rows, W, seed=3, device="cuda")
    o0, g2, _ = RR.make_rows(fam, rows, W, seed=4, device="cuda")
    x = torch.full((rows + 2, W), float("nan"), dtype=torch.float32, device="cuda")
    x[1:rows + 1] = x0
    return x, (o0 * 3.0).to(torch.bfloat16), g1, g2, torch.full((rows + 2, W), float("nan"), dtype=torch.bfloat16, device="cuda")


@pytest.mark.parametrize("W", (2112, 3584, 4096))
@pytest.mark.parametrize("rows", (1, 67))
def test_rmsnorm_add_norm_wide_against_float64(W, rows):
    D = math.ceil(W / 256) + 8
    for fam in ("randn", "rowscale"):
        x, o, g1, g2, h = _rows(fam, rows, W)
        od, xd, only = o.double(), x[1:rows + 1].double(), x.clone()
        y = od * torch.rsqrt(od.pow(2).mean(-1, keepdim=True) + EPS) * g1.double()
        x1 = xd + y
        r = torch.rsqrt(x1.pow(2).mean(-1, keepdim=True) + EPS)
        hd = x1 * r * g2.double()
        Bx = y.abs() * (D / 2 + 7) * U + x1.abs() * U
        Bh = (hd.abs() * (D / 2 + 7) * U + r * g2.double().abs() * Bx + hd.abs() * (x1.abs() * Bx).sum(-1, keepdim=True) / x1.pow(2).sum(-1, keepdim=True)
              + RR.half_ulp_bf16(hd))
        _add_norm("mq_rmsnorm_add_norm_wide", x[1:], o, g1, g2, h[1:], W)
        assert all(bool(t[i].isnan().all()) for t in (x, h) for i in (0, rows + 1)), "a guard row was written"
        rx, rh = RR.ratio(x[1:rows + 1], x1, Bx), RR.ratio(h[1:rows + 1], hd, Bh)
        print(f"GEMMA2_RATIO rmsnorm_add_norm_wide family={fam} rows={rows} W={W} stream={rx:.4f} bf16_out={rh:.4f}")
        assert rx <= MARGIN and rh <= MARGIN
        _add_norm("mq_rmsnorm_add_norm_wide", only[1:], o, g1, None, None, W)   # without the second norm: the same stream, bit for bit
        assert torch.equal(only[1:rows + 1], x[1:rows + 1])


def test_rmsnorm_add_norm_wide_at_2048_is_the_narrow_call():
    xa, o, g1, g2, ha = _rows("randn", 67, 2048)
    xb, hb = xa.clone(), ha.clone()
    _add_norm("mq_rmsnorm_add_norm_wide", xa[1:], o, g1, g2, ha[1:], 2048)
    _add_norm("mq_rmsnorm_add_norm", xb[1:], o, g1, g2, hb[1:], 2048)
    assert torch.equal(xa[1:68], xb[1:68]) and torch.equal(ha[1:68], hb[1:68])


@pytest.fixture(scope="module")
def models():
    return {name: (cfg, G2.hf_model(cfg), G.random_seqs(G2.LENS, 300, seed=3)) for name, cfg in G2.CONFIGS.items()}


@pytest.mark.parametrize("name", tuple(G2.CONFIGS))
@pytest.mark.parametrize("pooling", ("last", "mean"))
def test_tiny_tower_against_transformers(models, name, pooling):
    from marqo_amd.engine.gemma2 import Gemma2Tower
    cfg, model, seqs = models[name]
    tower = Gemma2Tower(archs.gemma2_arch_from_hf_config(cfg), G.state_dict_of(model), DEV, pooling=pooling)
    (ids, mask), ref = G.pad_batch(seqs), G2.pooled_rows(model, seqs, pooling)
    for normalize in (True, False):
        out = tower.encode_ids(ids, mask, normalize=normalize)
        e = G2.cos_err(out, ref)
        print(f"GEMMA2_COS {name} {pooling} normalize={normalize}: " + " ".join(f"{float(v):.2e}" for v in e) + f" (bound {COS_TOL:.0e})")
        assert float(e.max()) < COS_TOL, (name, pooling, e.tolist())


TEXTS = ["hello world", "sliding windows see only their neighbours", "a search engine ranks documents for a query " * 8, ""]


@pytest.mark.parametrize("pooling", ("last", "mean"))
def test_vectorise_from_a_local_directory(models, tmp_path, monkeypatch, pooling):
    import transformers
    from tokenizers import Tokenizer
    from marqo_amd.s2_inference import s2_inference as s2i
    d = G.write_checkpoint_dir(str(tmp_path / "ckpt"), copy.deepcopy(models["TINY"][1]).float(), G.train_tokenizer())
    model = transformers.Gemma2Model.from_pretrained(d, attn_implementation="eager").double().eval()   # the reference: what the directory holds
    raw = Tokenizer.from_file(d + "/tokenizer.json")
    raw.enable_truncation(max_length=64)
    rows = [torch.tensor(raw.encode(x).ids) for x in TEXTS]   # (64 tokens at the longest, <bos> <eos> alone for the empty text)
    monkeypatch.setenv("MARQO_MAX_CUDA_MODEL_MEMORY", "64")
    props = {"type": "hf", "name": d, "dimensions": 128, "tokens": 64, **({"poolingMethod": "mean"} if pooling == "mean" else {})}
    try:
        s2i.clear_loaded_models()
        out = torch.tensor(s2i.vectorise(f"gemma2-test-{pooling}", TEXTS, model_properties=props, device=DEV), dtype=torch.float64)
    finally:
        s2i.clear_loaded_models()
    e = G2.cos_err(out, G2.pooled_rows(model, rows, pooling))
    print(f"GEMMA2_COS vectorise {pooling} against transformers: " + " ".join(f"{float(v):.2e}" for v in e) + f" (bound {COS_TOL:.0e})")
    assert out.shape == (4, 128) and float(e.max()) < COS_TOL and torch.allclose(out.norm(dim=-1), torch.ones(4, dtype=torch.float64), atol=1e-5)

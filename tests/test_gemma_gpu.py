"""The EmbeddingGemma row kernels and tower on the GPU: mq_rmsnorm_add_norm, mq_qk_norm_rope at head_dim 256 and mq_glu_tanh against float64, GemmaTower
(mq_encode_gemma through engine/gemma.py) against the project's fp32 oracle (tests/gemma_ref.py, itself equal to transformers' Gemma3TextModel to fp32
round-off: tests/test_gemma_host.py), and `vectorise` (`hf` and `sbert`) from a local checkpoint directory.

Budgets (U = 2**-24, margin 1.25 as in tests/test_qwen_gpu.py for the terms a derivation neglects; D = rowops_ref.chain(W), the longest chain of additions
of a row's sum of squares):
  mq_rmsnorm_add_norm, the fp32 stream x' = x + y, y = rmsnorm(o; g_post):  B_x = |y| (D / 2 + 7) U + |x'| U.  The first term is mq_rmsnorm's fp32-output
      budget (tests/test_qwen_gpu.py: D U relative on a sum of positive terms, halved by the square root; 4 U for the squaring, the divide, eps and
      rsqrtf; 3 U for the two products and a spare) — the bf16 input is exact in fp32 —, the second the rounding of the addition.
  its bf16 output h = rmsnorm(x'; g_next):  B_h = |h| (D / 2 + 7) U + r |g_next| B_x + |h| (|x'| . B_x) / (x' . x') + half a bf16 ulp of h, r = the row's
      rsqrt.  The kernel normalises ITS x', which differs from the reference's by up to B_x per element: the second term is that difference through
      the product with r g, the third through r itself (d r / r = - (x . dx) / (x . x)).
  mq_qk_norm_rope at head_dim 256: the formula of tests/test_qwen_gpu.py, hyp (t f + 24) U + half a bf16 ulp.  Its 24 U allowed <= 8 U for the head's RMS;
      at 256 a lane sums 4 squares and the butterfly has six levels: a chain of 9 additions, halved by the square root, 4.5 U.  Positions up to 8191, the
      largest the tower serves (max_pos <= 8192).
  mq_glu_tanh: gemma_ref.glu_tanh_budget (half a bf16 ulp of the reference + (10 |u| + 5) U |ref|, derived there), bar 1.0: nothing is neglected.  On
      this input the erf form is 17000 x outside (tests/test_gemma_host.py).
  tower: 1 - cos < 3e-4 on the pooled rows, the project's bf16 tower bar (tests/test_modernbert_gpu.py).

Measured values are printed as `GEMMA_RATIO` / `GEMMA_COS` lines.  On an MI355X: mq_rmsnorm_add_norm 0.97 (stream) / 1.00 (bf16 output: the half ulp
itself); mq_qk_norm_rope at 256 1.00, 1.12 at positions up to 8191; mq_glu_tanh 0.9998 (the erf form 4.5e6); tower max 1 - cos 5.8e-6 (TINY_FULL, mean
pooling); vectorise against transformers 2.8e-6 (hf), 8.8e-6 (sbert)."""
import os

import numpy as np
import pytest
import torch

from marqo_amd import _lib as L
from marqo_amd.engine import archs
from tests import gemma_ref as G
from tests import rowops_ref as RR
from tests.test_modernbert_gpu import COS_TOL
from tests.test_qwen_gpu import _qk_case

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MARGIN = 1.25
U = 2.0 ** -24


@pytest.fixture(scope="module")
def lib():
    return L.load()


def _s():
    return torch.cuda.current_stream().cuda_stream


# ---- mq_rmsnorm_add_norm ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", (4, 128, 768, 2048))
@pytest.mark.parametrize("rows", (1, 67))
def test_rmsnorm_add_norm_against_float64(lib, W, rows):
    eps = 1e-6
    for fam in ("randn", "rowscale"):
        x0, g1, _ = RR.make_rows(fam, rows, W, seed=3, device="cuda")
        o0, g2, _ = RR.make_rows(fam, rows, W, seed=4, device="cuda")
        o = (o0 * 3.0).to(torch.bfloat16)
        od, xd = o.double(), x0.double()
        y = od * torch.rsqrt(od.pow(2).mean(-1, keepdim=True) + eps) * g1.double()
        x1 = xd + y
        r = torch.rsqrt(x1.pow(2).mean(-1, keepdim=True) + eps)
        h = x1 * r * g2.double()
        Bx = y.abs() * (RR.chain(W) / 2 + 7) * U + x1.abs() * U
        Bh = (h.abs() * (RR.chain(W) / 2 + 7) * U + r * g2.double().abs() * Bx
              + h.abs() * (x1.abs() * Bx).sum(-1, keepdim=True) / x1.pow(2).sum(-1, keepdim=True) + RR.half_ulp_bf16(h))
        xw = torch.full((rows + 2, W), float("nan"), dtype=torch.float32, device="cuda")
        xw[1:-1] = x0
        hw_ = torch.full((rows + 2, W), float("nan"), dtype=torch.bfloat16, device="cuda")
        L.check(lib.mq_rmsnorm_add_norm(xw[1:].data_ptr(), o.data_ptr(), g1.data_ptr(), g2.data_ptr(), hw_[1:].data_ptr(), rows, W, eps, _s()), "mq_rmsnorm_add_norm")
        torch.cuda.synchronize()
        assert bool(xw[0].isnan().all()) and bool(xw[-1].isnan().all()) and bool(hw_[0].isnan().all()) and bool(hw_[-1].isnan().all())
        rx, rh = RR.ratio(xw[1:-1], x1, Bx), RR.ratio(hw_[1:-1], h, Bh)
        print(f"GEMMA_RATIO rmsnorm_add_norm family={fam} rows={rows} W={W} stream={rx:.4f} bf16_out={rh:.4f}")
        assert rx <= MARGIN and rh <= MARGIN
        # without the second norm: the same stream, bit for bit, and nothing else written
        only = x0.clone()
        L.check(lib.mq_rmsnorm_add_norm(only.data_ptr(), o.data_ptr(), g1.data_ptr(), None, None, rows, W, eps, _s()), "mq_rmsnorm_add_norm")
        assert torch.equal(only, xw[1:-1])
    assert lib.mq_rmsnorm_add_norm(only.data_ptr(), o.data_ptr(), g1.data_ptr(), g2.data_ptr(), None, rows, W, eps, _s()) == -1
    assert b"come together" in lib.mq_last_error()


# ---- mq_qk_norm_rope at head_dim 256 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", (True, False))
def test_qk_norm_rope_256_against_float64(lib, norm):
    _qk_case(lib, "packed", [1, 17, 70], 3, 1, 256, norm, 1e6)
    _qk_case(lib, "packed", [1, 17, 70], 4, 2, 256, norm, 1e4)
    _qk_case(lib, "fixed", [33, 33, 33], 2, 2, 256, norm, 1e4, fixed=True)


def test_qk_norm_rope_256_at_positions_up_to_8191(lib):
    _qk_case(lib, "long", [8192], 1, 1, 256, True, 1e6)
    _qk_case(lib, "long", [8192], 1, 1, 256, True, 1e4)


# ---- mq_glu_tanh ----------------------------------------------------------------------------------------------------------------------------------------
def test_glu_tanh_against_float64(lib):
    buf = G.glu_tanh_input().to("cuda")
    ref, gate = G.glu_tanh_reference(buf)
    bud = G.glu_tanh_budget(ref, gate)
    rows, F = buf.shape[0], buf.shape[1] // 2
    work = buf.clone()
    L.check(lib.mq_glu_tanh(work.data_ptr(), rows, F, _s()), "mq_glu_tanh")
    torch.cuda.synchronize()
    assert torch.equal(work[:, F:].view(torch.int16), buf[:, F:].view(torch.int16)), "the gate half was touched"
    ok = bud > 0
    r = float(((work[:, :F].double() - ref).abs()[ok] / bud[ok]).max())
    assert bool((work[:, :F].double()[~ok] == 0).all())
    # the erf form through the same layout (mq_glu, MQ_ACT_GELU) is far outside on this input
    erf = buf.clone()
    L.check(lib.mq_glu(erf.data_ptr(), rows, F, L.MQ_ACT_GELU, 0, _s()), "mq_glu")
    torch.cuda.synchronize()
    r_erf = float(((erf[:, :F].double() - ref).abs()[ok] / bud[ok]).max())
    print(f"GEMMA_RATIO glu_tanh ratio={r:.4f} (bar 1.0); the erf form: {r_erf:.1f}")
    assert r <= 1.0 and r_erf > 10.0


# ---- the tower ------------------------------------------------------------------------------------------------------------------------------------------
def _err(out, ref):
    out = out.double().cpu()
    return 1 - (out * ref).sum(-1) / (out.norm(dim=-1) * ref.norm(dim=-1))


@pytest.fixture(scope="module")
def tinies():
    out = {}
    for i, (name, cfg) in enumerate(G.TINIES.items()):
        model = G.hf_model(cfg, seed=i + 1)
        arch = archs.bert_arch_from_hf_config(cfg)
        sd = G.state_dict_of(model)
        seqs = G.random_seqs([1, 17, 70, 150], cfg["vocab_size"], seed=3)
        out[name] = dict(cfg=cfg, model=model, arch=arch, sd=sd, seqs=seqs, hidden=G.oracle_hidden_packed(sd, arch, seqs))
    return out


@pytest.mark.parametrize("name", tuple(G.TINIES))
@pytest.mark.parametrize("pooling", ("mean", "cls"))
def test_tiny_tower_against_the_oracle(tinies, name, pooling):
    """2 query heads on 1 K/V head of 256, width 128, half_window 4 (2 hw + 1 = 9: the band matters from 10 tokens on); TINY: sliding, sliding, full;
    lengths 1, 17, 70 (two query slices) and 150 (three) in one packed call; a permuted batch gives the permuted rows bit for bit"""
    from marqo_amd.engine.gemma import GemmaTower
    t = tinies[name]
    tower = GemmaTower(t["arch"], t["sd"], DEV, pooling=pooling)
    ids, mask = G.pad_batch(t["seqs"])
    for normalize in (True, False):
        out = tower.encode_ids(ids, mask, normalize=normalize)
        ref = G.pooled(t["hidden"], pooling, normalize)
        e = _err(out, ref)
        print(f"GEMMA_COS {name} {pooling} normalize={normalize}: " + " ".join(f"{float(v):.2e}" for v in e) + f" (bound {COS_TOL:.0e})")
        assert float(e.max()) < COS_TOL, (name, pooling, e.tolist())
        norms = out.double().cpu().norm(dim=-1)
        if normalize:
            np.testing.assert_allclose(norms.numpy(), 1.0, atol=1e-5)
        else:
            np.testing.assert_allclose(norms.numpy(), ref.norm(dim=-1).numpy(), rtol=2e-2)
        perm = torch.tensor([2, 0, 3, 1])
        assert torch.equal(tower.encode_ids(ids[perm], mask[perm], normalize=normalize), out[perm])


def test_the_band_is_a_band(tinies):
    """Two sliding layers of half_window 4: row 0 of a sequence depends on tokens 0 .. 8 and on nothing else.  With CLS pooling the tower returns row 0:
    another token at position 60 leaves it bit for bit, another token at position 8 moves it; in the all-full model position 60 moves it."""
    from marqo_amd.engine.gemma import GemmaTower
    base = G.random_seqs([100], 300, seed=11)[0]
    far, near = base.clone(), base.clone()
    far[60] = (int(base[60]) + 7) % 299 + 1
    near[8] = (int(base[8]) + 7) % 299 + 1
    ids, mask = torch.stack([base, far, near]), torch.ones(3, 100, dtype=torch.long)
    t = tinies["TINY_SLIDING"]
    out = GemmaTower(t["arch"], t["sd"], DEV, pooling="cls").encode_ids(ids, mask, normalize=False)
    assert torch.equal(out[0], out[1]), "a token outside the band moved a sliding-only model's row"
    assert float((out[0] - out[2]).abs().max()) > 1e-3, "a token inside the band did not move the row"
    t = tinies["TINY_FULL"]
    out = GemmaTower(t["arch"], t["sd"], DEV, pooling="cls").encode_ids(ids, mask, normalize=False)
    assert float((out[0] - out[1]).abs().max()) > 1e-3, "a far token did not move an all-full model's row"
    print("GEMMA_COS band: far token leaves the sliding model's row 0 bit for bit, moves the full model's")


# ---- vectorise ------------------------------------------------------------------------------------------------------------------------------------------
TEXTS = ["hello world", "sliding windows see only their neighbours", "a search engine ranks documents for a query " * 8, ""]


@pytest.fixture(scope="module")
def ckpt(tinies, tmp_path_factory):
    """the TINY model as a user brings it: save_pretrained + tokenizer.json + 1_Pooling + two Dense modules (128 -> 256 -> 128); the reference is
    transformers loading that directory"""
    import transformers
    g = torch.Generator().manual_seed(17)
    dense = [torch.randn(256, 128, generator=g) / 128 ** 0.5, torch.randn(128, 256, generator=g) / 256 ** 0.5]
    d = G.write_checkpoint_dir(str(tmp_path_factory.mktemp("gemma") / "ckpt"), tinies["TINY"]["model"], G.train_tokenizer(), pooling="mean", dense=dense)
    model = transformers.Gemma3TextModel.from_pretrained(d, attn_implementation="eager").float().eval()
    return dict(dir=d, model=model, dense=dense)


def _reference_rows(ckpt, tokens=64):
    from tokenizers import Tokenizer
    raw = Tokenizer.from_file(os.path.join(ckpt["dir"], "tokenizer.json"))
    raw.enable_truncation(max_length=tokens)
    rows = [torch.tensor(raw.encode(x).ids) for x in TEXTS]
    assert max(len(r) for r in rows) == tokens and min(len(r) for r in rows) == 2 and all(int(r[0]) == 2 and int(r[-1]) == 1 for r in rows)
    ids, mask = G.pad_batch(rows)
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
        out = torch.tensor(s2i.vectorise(f"gemma-test-{kind}", TEXTS, model_properties=props, device=DEV), dtype=torch.float64)
    finally:
        s2i.clear_loaded_models()
    assert out.shape == (4, 128)
    np.testing.assert_allclose(out.norm(dim=-1).numpy(), 1.0, atol=1e-5)
    ref = _reference_rows(ckpt)
    if kind == "sbert":      # the SentenceTransformer pipeline: Pooling -> 2_Dense -> 3_Dense -> Normalize
        ref = ref @ ckpt["dense"][0].double().t() @ ckpt["dense"][1].double().t()
    e = _err(out, ref)
    print(f"GEMMA_COS vectorise {kind} against transformers: " + " ".join(f"{float(v):.2e}" for v in e) + f" (bound {COS_TOL:.0e})")
    assert float(e.max()) < COS_TOL
    if kind == "sbert":      # and the Dense modules are not the identity: the bare encoder's rows are elsewhere
        assert float(_err(out, _reference_rows(ckpt)).min()) > 100 * COS_TOL


def test_loader_refusals(ckpt, tinies, tmp_path):
    from marqo_amd.s2_inference.errors import InvalidModelPropertiesError
    from marqo_amd.s2_inference.hugging_face_model import HuggingFaceModel
    from marqo_amd.s2_inference.sbert_utils import SBERT
    d = ckpt["dir"]
    with pytest.raises(InvalidModelPropertiesError, match="'enginePrecision': 'fp8' is not available for EmbeddingGemma"):
        HuggingFaceModel(model_properties={"type": "hf", "name": d, "dimensions": 128, "enginePrecision": "fp8"}, device=DEV)._load_necessary_components()
    with pytest.raises(InvalidModelPropertiesError, match="pooling_method must be"):
        HuggingFaceModel(model_properties={"type": "hf", "name": d, "dimensions": 128, "poolingMethod": "last"}, device=DEV)._load_necessary_components()
    with pytest.raises(InvalidModelPropertiesError, match="'dimensions'=64 but the encoder width is 128"):
        HuggingFaceModel(model_properties={"type": "hf", "name": d, "dimensions": 64}, device=DEV)._load_necessary_components()
    biased = G.write_checkpoint_dir(str(tmp_path / "biased"), tinies["TINY"]["model"], G.train_tokenizer(), pooling="mean", dense=ckpt["dense"], dense_bias=True)
    with pytest.raises(InvalidModelPropertiesError, match="Dense module 2_Dense has a bias"):
        SBERT(biased, device=DEV, embedding_dim=128).load()
    tanh = G.write_checkpoint_dir(str(tmp_path / "tanh"), tinies["TINY"]["model"], G.train_tokenizer(), pooling="mean", dense=ckpt["dense"],
                                  dense_activation="torch.nn.modules.activation.Tanh")
    with pytest.raises(InvalidModelPropertiesError, match="Dense module 2_Dense has activation"):
        SBERT(tanh, device=DEV, embedding_dim=128).load()

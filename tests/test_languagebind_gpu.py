"""LanguageBind on the GPU: the three kernels of csrc/temporal.hip against float64 computed from the same inputs, the video tower against the
restatement (tests/languagebind_ref.py), and vectorise() end to end on a synthetic checkpoint directory.
The tower's row-level bars — every stream row against float64 — are in tests/test_languagebind_passes_gpu.py; here it is held at the pooled output.

BOUND of mq_temporal_attention.  The kernel keeps its probabilities in fp32 (they are never rounded to bf16: there is no MFMA operand to feed), so
of the budget tests/attention_ref.py derives for mq_attention, u (P|V| + |out|) with u = 2**-8, the probability term u P|V| does not apply and what
remains is the bf16 rounding of the stored value, u |out| (taken from its functions: budget(...) - budget(..., out_fp8=True)), with the factor
1.25 its callers allow.  That term alone cannot bound ANY fp32 kernel where an output cancels (|out| << P|V|: the fp32 roundings are relative to
P|V|, not to |out|; in mq_attention's budget they hide inside u P|V|), so the fp32 arithmetic gets its own term, derived and not tuned, e P|V| with
    e = (2 * 69 / 8 * S + 2 T + 8) * 2**-24
  - S = max over the keys of sum_d |q_d k_jd| of the row: a score is 64 exact bf16 x bf16 products summed in fp32 through 16 fused adds per lane
    and two butterfly levels, then scaled, less the maximum, times log2(e) / 8: at most 69 roundings of magnitude <= 2**-24 S, divided by
    sqrt(64) = 8 in the exponent; a probability and the normaliser each carry that once (2 x);
  - 2 T + 8: the T-term sums of the normaliser and of P V (fused), exp2, the reciprocal, the final product.
For randn inputs e is ~1e-5, against 1.25 u = 4.9e-3 for the probability term it replaces: the bound asked here is the tighter one everywhere."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

from marqo_amd import _lib as L
from tests import attention_ref as A
from tests import languagebind_ref as LBR
from tests import rowops_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MARGIN = 1.25           # the factor the callers of attention_ref.budget / rowops_ref.reference_ln allow (tests/test_attention_gpu.py, tests/test_rowops_gpu.py)
COS_TOL = 1e-3          # the project's bf16 tower bound
EPS = 1e-5


def _s():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope="module")
def lib():
    return L.load()


# ---- 1. mq_temporal_attention ---------------------------------------------------------------------------------------------------------------
def _qkv(B, T, N, heads, seed, edge=True):
    g = torch.Generator().manual_seed(seed)
    W = heads * 64
    x = torch.randn(B * T * N, 3, heads, 64, generator=g)
    if edge and T > 1:
        x[0, 0] *= 12.0                  # the first query row: large-magnitude scores, a softmax near one-hot
        x[N * (T - 1) + N - 1, 0] = 0.0  # the last token's last frame of clip 0: all scores equal (0) -> a plain mean of the T values
    return x.reshape(B * T * N, 3 * W).to(torch.bfloat16).to(DEV)


def _attention_ratio(lib, qkv, B, T, N, heads):
    W = heads * 64
    out = torch.empty(B * T * N, W, dtype=torch.bfloat16, device=DEV)
    L.check(lib.mq_temporal_attention(qkv.data_ptr(), out.data_ptr(), B, T, N, W, heads, _s()), "mq_temporal_attention")
    torch.cuda.synchronize()
    ref, absref = LBR.temporal_attention_rearranged(qkv, B, T, N, heads)
    rounding = A.budget(ref, absref) - A.budget(ref, absref, out_fp8=True)          # u |out|: the bf16 store
    e = (2 * 69 / 8 * LBR.score_magnitude(qkv, B, T, N, heads) + 2 * T + 8) * 2.0 ** -24
    bound = MARGIN * rounding + e * absref
    assert bool((bound <= MARGIN * A.budget(ref, absref)).all())                       # never looser than mq_attention's own budget
    return R.ratio(out, ref, bound), out


@pytest.mark.parametrize("T", [1, 2, 3, 8, 16])
def test_temporal_attention_against_fp64(lib, T):
    for N in (1, 5, 257):
        for B in (1, 3):
            r, _ = _attention_ratio(lib, _qkv(B, T, N, 2, seed=T * 1000 + N * 10 + B), B, T, N, 2)
            print(f"TEMPORAL_ATTENTION_RATIO W=128 heads=2 T={T} N={N} B={B} ratio={r:.4f}")
            assert r <= 1.0, (T, N, B, r)


def test_temporal_attention_at_the_model_width(lib):
    r, _ = _attention_ratio(lib, _qkv(1, 8, 257, 16, seed=7), 1, 8, 257, 16)
    print(f"TEMPORAL_ATTENTION_RATIO W=1024 heads=16 T=8 N=257 B=1 ratio={r:.4f}")
    assert r <= 1.0, r


def test_temporal_attention_edge_rows(lib):
    """the all-equal row is the mean of the T values; the large-magnitude row is (nearly) one value"""
    B, T, N, heads = 1, 8, 5, 2
    qkv = _qkv(B, T, N, heads, seed=3)
    r, out = _attention_ratio(lib, qkv, B, T, N, heads)
    assert r <= 1.0
    W = heads * 64
    rows = torch.arange(T, device=DEV) * N + (N - 1)
    mean = qkv[rows, 2 * W:].double().mean(0)
    got = out[N * (T - 1) + N - 1].double()
    assert float(((got - mean).abs() / (MARGIN * A.U * mean.abs() + 16 * 2.0 ** -24 * qkv[rows, 2 * W:].double().abs().mean(0))).max()) <= 1.0


@pytest.mark.parametrize("T,W,heads", [(17, 128, 2), (8, 64, 2)])
def test_temporal_attention_refuses_what_it_does_not_run(lib, T, W, heads):
    N = 3
    qkv = torch.zeros(T * N, 3 * W, dtype=torch.bfloat16, device=DEV)
    out = torch.full((T * N, W), 7.0, dtype=torch.bfloat16, device=DEV)
    rc = lib.mq_temporal_attention(qkv.data_ptr(), out.data_ptr(), 1, T, N, W, heads, _s())
    torch.cuda.synchronize()
    assert rc != L.MQ_OK and b"mq_temporal_attention" in lib.mq_last_error()
    assert bool((out == 7.0).all())


# ---- 2. a wrong frame is visible ----------------------------------------------------------------------------------------------------------
def test_one_changed_frame_changes_exactly_its_token(lib):
    B, T, N, heads = 2, 8, 5, 2
    W = heads * 64
    qkv = _qkv(B, T, N, heads, seed=11, edge=False)
    _, base = _attention_ratio(lib, qkv, B, T, N, heads)
    b, t, n = 1, 3, 2
    qkv2 = qkv.clone()
    qkv2[(b * T + t) * N + n, W:] = (qkv[(b * T + t) * N + n, W:].float() * -1.5 + 0.25).to(torch.bfloat16)       # K and V of one (b, t, n) row
    _, moved = _attention_ratio(lib, qkv2, B, T, N, heads)
    diff = (base.view(torch.int16) != moved.view(torch.int16))
    want = torch.zeros(B * T * N, dtype=torch.bool, device=DEV)
    want[(b * T + torch.arange(T, device=DEV)) * N + n] = True
    assert torch.equal(diff.any(dim=1), want)                                      # exactly the T rows of that (b, n); no other row by a bit
    assert bool(diff[want].reshape(T, heads, 64).any(dim=2).all())                 # ... at every head


# ---- 3. mq_temporal_embed_ln --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [128, 1024])
@pytest.mark.parametrize("T", [1, 8])
def test_temporal_embed_ln(lib, W, T):
    B, N = 2, 5
    rows = B * T * N
    x, g, b = R.make_rows("randn", rows, W, seed=T, device=DEV)
    temb = torch.randn(T, W, device=DEV, generator=torch.Generator(device=DEV).manual_seed(W + T)) * 0.5
    stream = x.clone()
    out = torch.empty(rows, W, dtype=torch.bfloat16, device=DEV)
    L.check(lib.mq_temporal_embed_ln(stream.data_ptr(), temb.data_ptr(), g.data_ptr(), b.data_ptr(), out.data_ptr(), B, T, N, W, EPS, _s()),
            "mq_temporal_embed_ln")
    torch.cuda.synchronize()
    t_of_row = (torch.arange(rows, device=DEV) // N) % T
    want = x if T == 1 else x + temb[t_of_row]                                      # one fp32 add; T == 1: the stream is unchanged
    assert torch.equal(stream, want)
    y, Bd = R.reference_ln(want, g, b, EPS)
    r = R.ratio(out, y, Bd + R.half_ulp_bf16(y))
    print(f"TEMPORAL_EMBED_LN_RATIO W={W} T={T} ratio={r:.4f}")
    assert r <= MARGIN, r


# ---- 4. clip-layout patchify ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,P,T,B", [(32, 16, 3, 2), (224, 14, 8, 1)])
def test_patchify_clip_is_patchify_of_the_frames(lib, S, P, T, B):
    Kp = (3 * P * P + 63) // 64 * 64
    G = S // P
    clip = LBR.make_clip(B, T, S, seed=S).to(DEV)
    frames = clip.permute(0, 2, 1, 3, 4).reshape(B * T, 3, S, S).contiguous()
    got = torch.full((B * T * G * G, Kp), 3.0, dtype=torch.bfloat16, device=DEV)
    want = torch.full((B * T * G * G, Kp), 5.0, dtype=torch.bfloat16, device=DEV)
    one = (C.c_float * 3)(1.0, 1.0, 1.0)
    L.check(lib.mq_patchify_clip(clip.data_ptr(), got.data_ptr(), B, T, S, P, Kp, _s()), "mq_patchify_clip")
    L.check(lib.mq_patchify(frames.data_ptr(), 0, want.data_ptr(), B * T, S, P, Kp, C.addressof(one), C.addressof(one), _s()), "mq_patchify")
    torch.cuda.synchronize()
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))


# ---- 5. / 6. the tower against the restatement ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tower_case(shape_name, T, B):
    """(tower, cfg, sd, clip, restatement's unit rows): built once per case and shared"""
    from marqo_amd.engine import archs
    from marqo_amd.engine.languagebind import LanguageBindVideoTower
    shape = getattr(LBR, shape_name)
    cfg = LBR.config(shape, T=T)
    sd = LBR.synthetic_state_dict(cfg, seed=T)
    clip = LBR.make_clip(B, T, shape["S"], seed=B)
    ref = LBR.embed(LBR.video_forward(sd, cfg, clip), sd, "video", True)
    tower = LanguageBindVideoTower(archs.languagebind_arch_from_hf_config(cfg), sd, DEV)
    return tower, cfg, sd, clip, ref


def _cos_err(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((1 - (a * b).sum(-1) / (a.norm(dim=-1) * b.norm(dim=-1))).max())


@pytest.mark.parametrize("shape_name,T,B", [("SMALL", 3, 3), ("SMALL", 8, 1), ("LARGE", 8, 1)])
def test_video_tower_against_the_restatement(shape_name, T, B):
    tower, cfg, sd, clip, ref = _tower_case(shape_name, T, B)
    out = tower.encode_clips(clip.to(DEV))
    torch.cuda.synchronize()
    e = _cos_err(out, ref)
    print(f"LANGUAGEBIND_TOWER shape={shape_name} T={T} B={B} max(1-cos)={e:.2e}")
    assert out.shape == (B, cfg["projection_dim"]) and bool(torch.isfinite(out).all())
    assert e <= COS_TOL, e
    raw = tower.encode_clips(clip, normalize=False)                  # (a host tensor in; the un-normalised rows point the same way)
    assert _cos_err(raw, out) <= 1e-6


def test_frame_order_matters():
    """the same clip with its frames reversed moves the embedding by more than the tower's bf16 noise (measured above against the restatement, and
    bounded by COS_TOL): no shortcut that averages per-frame image embeddings passes"""
    tower, cfg, sd, clip, ref = _tower_case("SMALL", 8, 1)
    a = tower.encode_clips(clip)
    r = tower.encode_clips(clip.flip(2))
    torch.cuda.synchronize()
    noise, moved = _cos_err(a, ref), _cos_err(a, r)
    want = _cos_err(ref, LBR.embed(LBR.video_forward(sd, cfg, clip.flip(2)), sd, "video", True))
    print(f"LANGUAGEBIND_FRAME_ORDER noise={noise:.2e} moved={moved:.2e} restatement_moved={want:.2e}")
    assert moved > max(COS_TOL, 10 * noise), (moved, noise)
    assert abs(moved - want) <= 2 * COS_TOL


# ---- 7. end to end ----------------------------------------------------------------------------------------------------------------------------
def _props(name, root):
    return {"name": name, "dimensions": LBR.SMALL["D"], "type": "languagebind", "loader": "languagebind", "model_size": 1,
            "supported_modalities": ["video", "language", "image"], "video_chunk_length": 20, "audio_chunk_length": 10, "localpath": str(root)}


def test_vectorise_end_to_end(tmp_path, monkeypatch):
    from PIL import Image
    from marqo_amd.engine.hf_clip import load_tokenizer
    from marqo_amd.s2_inference import s2_inference as S
    from marqo_amd.s2_inference.enums import Modality
    monkeypatch.setenv("MARQO_MAX_CUDA_MODEL_MEMORY", "64")
    name, T = "LanguageBind/Video_V1.5_FT_Image", 8
    parts = LBR.write_model(tmp_path, LBR.SMALL, T=T, image=True, seed=4)
    (vcfg, vsd), (icfg, isd) = parts["video"], parts["image"]
    props = _props(name, tmp_path)
    S.clear_loaded_models()
    try:
        vec = lambda content, modality, norm: np.asarray(S.vectorise(name, content, model_properties=dict(props), device=DEV, modality=modality,
                                                                     normalize_embeddings=norm))
        norms = lambda a: np.linalg.norm(a, axis=1)
        # video: two pixel_values dicts, one on the host and one on the device; every item is encoded
        c1, c2 = LBR.make_clip(1, T, LBR.SMALL["S"], seed=1), LBR.make_clip(2, T, LBR.SMALL["S"], seed=2)
        clips = [{"pixel_values": c1}, {"pixel_values": c2.to(DEV)}]
        v_unit, v_raw = vec(clips, Modality.VIDEO, True), vec(clips, Modality.VIDEO, False)
        assert v_unit.shape == (3, LBR.SMALL["D"]) and np.allclose(norms(v_unit), 1.0, atol=1e-5)
        assert np.allclose(norms(v_raw), math.exp(float(vsd["logit_scale"])), rtol=1e-5)
        ref_v = LBR.embed(LBR.video_forward(vsd, vcfg, torch.cat([c1, c2])), vsd, "video", True)
        assert _cos_err(torch.from_numpy(v_unit), ref_v) <= COS_TOL
        assert _cos_err(torch.from_numpy(vec(c2, Modality.VIDEO, True)), ref_v[1:]) <= COS_TOL           # the tensor itself
        # image: PIL images through the GPU preprocessing, and a preprocessed batch against the restatement
        rng = np.random.default_rng(0)
        pil = [Image.fromarray(rng.integers(0, 256, (40, 50, 3), dtype=np.uint8)), Image.fromarray(rng.integers(0, 256, (33, 32, 3), dtype=np.uint8))]
        i_unit, i_raw = vec(pil, Modality.IMAGE, True), vec(pil, Modality.IMAGE, False)
        assert i_unit.shape == (2, LBR.SMALL["D"]) and np.allclose(norms(i_unit), 1.0, atol=1e-5)
        assert np.allclose(norms(i_raw), math.exp(float(isd["logit_scale"])), rtol=1e-5)
        px = torch.randn(2, 3, LBR.SMALL["S"], LBR.SMALL["S"], generator=torch.Generator().manual_seed(9))
        assert _cos_err(torch.from_numpy(vec(px, Modality.IMAGE, True)), LBR.image_forward(isd, icfg, px)) <= COS_TOL
        # text: the LAST part's tower (the image part's); unit rows whatever normalize says
        texts = ["the red cat on a dog", "a dog"]
        t_unit, t_raw = vec(texts, Modality.TEXT, True), vec(texts, Modality.TEXT, False)
        assert np.allclose(norms(t_unit), 1.0, atol=1e-5) and np.allclose(norms(t_raw), 1.0, atol=1e-5)
        assert _cos_err(torch.from_numpy(vec(texts[0], Modality.TEXT, True)), torch.from_numpy(t_unit[:1])) <= 3e-5
        tok = load_tokenizer(str(tmp_path / LBR.IMAGE_PART), LBR.CTX)
        ids = torch.full((len(texts), LBR.CTX), tok.eot_id, dtype=torch.int64)        # the reference pads with its EOS id
        for i, t in enumerate(texts):
            row = [tok.sot_id] + tok.encode(t) + [tok.eot_id]
            ids[i, :len(row)] = torch.tensor(row)
        ref_t = LBR.embed(LBR.text_forward(isd, icfg, ids), isd, "language", True)
        # text x video cosine matrix against the restatement's
        got = t_unit @ v_unit.T
        assert float(np.abs(got - (ref_t @ ref_v.T).numpy()).max()) <= 2e-3
        # bad video content: the reference's ValueError
        with pytest.raises(ValueError, match="Unsupported video content type"):
            S.vectorise(name, ["https://example.com/clip.mp4"], model_properties=dict(props), device=DEV, modality=Modality.VIDEO)
        model, pre = S.load_multimodal_model_and_get_preprocessors(name, dict(props), device=DEV)
        assert pre["video"] is None and pre["audio"] is None
    finally:
        S.clear_loaded_models()


def test_video_modality_on_a_clip_model_is_unchanged(tmp_path, monkeypatch):
    """an open_clip model still drops the modality (DefaultEncoder): texts labelled VIDEO come out as its text embeddings, as before"""
    from marqo_amd.s2_inference import s2_inference as S
    from marqo_amd.s2_inference.enums import Modality
    from tests.test_s2_inference_gpu import _tiny_clip
    monkeypatch.setenv("MARQO_AMD_MODEL_DIR", str(tmp_path))
    monkeypatch.setenv("MARQO_MAX_CUDA_MODEL_MEMORY", "64")
    props = _tiny_clip(tmp_path)[0]
    S.clear_loaded_models()
    try:
        texts = ["a photo of a cat", "marqo is a tensor search engine"]
        as_text = np.asarray(S.vectorise("tiny-clip", texts, model_properties=props, device=DEV))
        as_video = np.asarray(S.vectorise("tiny-clip", texts, model_properties=props, device=DEV, modality=Modality.VIDEO))
        assert as_video.shape == (2, 64) and float(np.abs(as_video - as_text).max()) <= 1e-6
        model = S.get_available_models()[S._create_model_cache_key("tiny-clip", DEV, props)]["model"]
        assert isinstance(S.get_encoder(model), S.DefaultEncoder)
    finally:
        S.clear_loaded_models()

"""The LanguageBind audio part on the GPU: the three kernels of csrc/audio.hip against the restatements of tests/audio_ref.py, the audio tower
against the fp32 restatement, and vectorise() end to end on a synthetic `Audio_FT_Image` directory.
The tower's row-level bars — every stream row against float64 — are in tests/test_languagebind_passes_gpu.py; here it is held at the pooled output.

BOUND of mq_fbank.  The yardstick is what the same formula gives in torch float32 on the CPU (AR.fbank_torch, every step in float32 in torchaudio's
order): its largest absolute error against the float64 reference on the SAME waveform.  The kernel may err by at most 4 times that.  Both numbers
are printed on an AUDIO_FBANK line.  Measured on an MI355X (yardstick / kernel): 112 filters 3.1e-5 / 2.3e-7 (n = 400), 5.3e-5 / 2.3e-7 (559),
4.2e-5 / 3.9e-7 (560), 1.2e-4 / 4.8e-7 (16 007); 16 filters 4.8e-6 / 2.3e-7, 1.5e-6 / 2.3e-7, 9.0e-6 / 2.3e-7, 9.6e-6 / 2.4e-7.  The kernel's interior
is fp64, so its error is the rounding of the stored float32: half an ulp, 2.4e-7 for 4 <= |log| < 8 and 4.8e-7 up to 16."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

from marqo_amd import _lib as L
from tests import audio_ref as AR
from tests import languagebind_ref as LBR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
COS_TOL = 1e-3          # the project's bf16 tower bound (tests/test_languagebind_gpu.py)
LOG_EPS = np.float32(np.log(np.float64(AR.EPS32)))
MEAN, STD = -4.2677393, 4.5689974


def _s():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope="module")
def lib():
    return L.load()


def _fbank(lib, wave, bins):
    """wave: host float32 [n] or [channels, n] -> host float32 [m, bins], with sentinel rows behind the output checked"""
    w = wave.to(DEV).contiguous()
    m = AR.num_frames(w.shape[-1])
    out = torch.full((m + 1, bins), 7.0, dtype=torch.float32, device=DEV)
    ws = torch.zeros(L.MQ_FBANK_WS_BYTES, dtype=torch.uint8, device=DEV)
    L.check(lib.mq_fbank(w.data_ptr(), w.shape[-1], w.numel(), 16000, bins, out.data_ptr(), ws.data_ptr(), _s()), "mq_fbank")
    torch.cuda.synchronize()
    assert bool((out[m] == 7.0).all())
    return out[:m].cpu()


# ---- 1. mq_fbank -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [400, 559, 560, 16000 + 7])
@pytest.mark.parametrize("bins", [112, 16])
def test_fbank_against_fp64(lib, bins, n):
    wave = AR.make_waveform(n, seed=n + bins)
    ref = AR.fbank_ref(wave.numpy(), bins)
    yard = float(np.abs(AR.fbank_torch(wave, bins, torch.float32).numpy().astype(np.float64) - ref).max())
    got = _fbank(lib, wave, bins)
    err = float(np.abs(got.numpy().astype(np.float64) - ref).max())
    print(f"AUDIO_FBANK bins={bins} n={n} frames={ref.shape[0]} torch_fp32_err={yard:.3e} kernel_err={err:.3e} ratio={err / yard:.3f}")
    assert got.shape == ref.shape and bool(torch.isfinite(got).all())
    assert err <= 4 * yard, (err, yard)


@pytest.mark.parametrize("bins", [112, 16])
def test_fbank_of_silence_is_the_floor(lib, bins):
    for n in (400, 16000 + 7):
        z = torch.zeros(n)
        assert bool((AR.fbank_ref(z.numpy(), bins) == np.log(np.float64(AR.EPS32))).all())
        got = _fbank(lib, z, bins).numpy()
        assert got.shape == (AR.num_frames(n), bins) and bool((got == LOG_EPS).all())


def test_fbank_of_two_channels_frames_channel_zero(lib):
    """the mean is the whole tensor's, the frames are channel 0's"""
    wave = AR.make_waveform(2000, seed=5, channels=2)
    wave[1] += 0.3                                     # a second channel with another offset: it moves the mean and nothing else
    ref = AR.fbank_ref(wave.numpy(), 16)
    yard = float(np.abs(AR.fbank_torch(wave, 16, torch.float32).numpy().astype(np.float64) - ref).max())
    err = float(np.abs(_fbank(lib, wave, 16).numpy().astype(np.float64) - ref).max())
    print(f"AUDIO_FBANK bins=16 n=2000 channels=2 torch_fp32_err={yard:.3e} kernel_err={err:.3e}")
    assert err <= 4 * yard


def test_fbank_frame_indexing(lib):
    """a unit impulse at sample 160 k + 200, the middle of frame k, on low noise: the largest row-to-row change lands at frame k"""
    n = 16000 + 7
    m = AR.num_frames(n)
    base = 1e-3 * torch.randn(n, generator=torch.Generator().manual_seed(3))
    quiet = _fbank(lib, base, 16)
    for k in (0, m // 2, m - 1):
        wave = base.clone()
        wave[k * 160 + 200] += 1.0
        rows = _fbank(lib, wave, 16)
        change = (rows - quiet).abs().amax(dim=1)
        assert int(change.argmax()) == k, (k, int(change.argmax()))
        # ... and only the three frames whose 400 samples hold it change much at all (frames k - 1, k, k + 1)
        far = torch.ones(m, dtype=torch.bool)
        far[max(0, k - 1):k + 2] = False
        assert float(change[far].max()) < 0.5 * float(change[k])


# ---- 2. mq_mel_fusion ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,starts", [(7, (0, 0, 0)), (40, (0, 0, 0)), (41, (0, 0, 1)), (100, (0, 30, 60))])
def test_mel_fusion(lib, m, starts):
    bins, L_ = 16, 40
    rows = (4.0 * torch.randn(m, bins, generator=torch.Generator().manual_seed(m)) - 4.0).contiguous()
    want = AR.fusion_ref(rows, L_, np.float32(MEAN), np.float32(STD), starts)          # float32 throughout, the kernel's expression order
    assert want.dtype == torch.float32
    out = torch.full((3 * bins + 1, L_), 7.0, dtype=torch.float32, device=DEV)         # (a sentinel row behind the picture)
    d_rows = rows.to(DEV)
    L.check(lib.mq_mel_fusion(d_rows.data_ptr(), m, bins, starts[0], starts[1], starts[2], MEAN, STD, out.data_ptr(), L_, _s()), "mq_mel_fusion")
    torch.cuda.synchronize()
    assert bool((out[3 * bins] == 7.0).all())
    got = out[:3 * bins].cpu().reshape(3, bins, L_)
    ulp = torch.from_numpy(np.spacing(np.abs(want.numpy())))
    assert bool(((got - want).abs() <= ulp).all())
    print(f"AUDIO_FUSION m={m} starts={starts} exact={bool(torch.equal(got, want))}")


def test_mel_fusion_of_a_picture_wider_than_one_tile(lib):
    """bins and L that are no multiple of the 32 x 32 tile, several tiles each way"""
    bins, L_, m = 112, 75, 100
    rows = torch.randn(m, bins, generator=torch.Generator().manual_seed(1)).contiguous()
    want = AR.fusion_ref(rows, L_, np.float32(0.5), np.float32(0.5), (0, 12, 25))
    out = torch.full((3 * bins + 1, L_), 7.0, dtype=torch.float32, device=DEV)
    d_rows = rows.to(DEV)
    L.check(lib.mq_mel_fusion(d_rows.data_ptr(), m, bins, 0, 12, 25, 0.5, 0.5, out.data_ptr(), L_, _s()), "mq_mel_fusion")
    torch.cuda.synchronize()
    got = out[:3 * bins].cpu().reshape(3, bins, L_)
    assert bool((out[3 * bins] == 7.0).all()) and bool(((got - want).abs() <= torch.from_numpy(np.spacing(np.abs(want.numpy())))).all())


# ---- 3. mq_patchify_rect -----------------------------------------------------------------------------------------------------------------------------
def _unfold(px, P, Kp):
    """fp32 [n, 3, H, Wd] -> bf16 [n Gh Gw, Kp]: rows (img, py, px), columns c P^2 + ky P + kx, zero-padded"""
    n = px.shape[0]
    cols = torch.nn.functional.unfold(px, kernel_size=P, stride=P)               # [n, 3 P P, Gh Gw], patches row-major
    rows = cols.transpose(1, 2).reshape(-1, 3 * P * P)
    return torch.nn.functional.pad(rows, (0, Kp - 3 * P * P)).to(torch.bfloat16)


@pytest.mark.parametrize("H,Wd,P,Kp,n", [(16, 40, 8, 192, 3), (28, 14, 14, 640, 2)])
def test_patchify_rect(lib, H, Wd, P, Kp, n):
    px = AR.make_spectrograms(n, H, Wd, seed=H)
    rows = n * (H // P) * (Wd // P)
    got = torch.full((rows + 1, Kp), 3.0, dtype=torch.bfloat16, device=DEV)
    d_px = px.to(DEV)
    L.check(lib.mq_patchify_rect(d_px.data_ptr(), got.data_ptr(), n, H, Wd, P, Kp, _s()), "mq_patchify_rect")
    torch.cuda.synchronize()
    assert bool((got[rows] == 3.0).all())
    want = _unfold(px, P, Kp)
    assert torch.equal(got[:rows].cpu().view(torch.int16), want.view(torch.int16))
    assert bool((got[:rows, 3 * P * P:] == 0).all())


def test_patchify_rect_of_a_square_is_patchify(lib):
    n, S, P, Kp = 2, 32, 16, 768
    px = AR.make_spectrograms(n, S, S, seed=2).to(DEV)
    got = torch.full((n * 4, Kp), 3.0, dtype=torch.bfloat16, device=DEV)
    want = torch.full((n * 4, Kp), 5.0, dtype=torch.bfloat16, device=DEV)
    one = (C.c_float * 3)(1.0, 1.0, 1.0)
    L.check(lib.mq_patchify_rect(px.data_ptr(), got.data_ptr(), n, S, S, P, Kp, _s()), "mq_patchify_rect")
    L.check(lib.mq_patchify(px.data_ptr(), 0, want.data_ptr(), n, S, P, Kp, C.addressof(one), C.addressof(one), _s()), "mq_patchify")
    torch.cuda.synchronize()
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))


# ---- 4. the tower ------------------------------------------------------------------------------------------------------------------------------------
def _cos_err(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((1 - (a * b).sum(-1) / (a.norm(dim=-1) * b.norm(dim=-1))).max())


@functools.lru_cache(maxsize=None)
def _tower_case():
    from marqo_amd.engine import archs
    from marqo_amd.engine.languagebind import LanguageBindAudioTower
    cfg = AR.config()
    sd = AR.synthetic_state_dict(cfg, seed=3)
    px = AR.make_spectrograms(3, AR.SMALL["bins"], AR.SMALL["L"], seed=1)
    ref = LBR.embed(AR.audio_forward(sd, cfg, px), sd, "audio", True)
    return LanguageBindAudioTower(archs.languagebind_arch_from_hf_config(cfg), sd, DEV), cfg, sd, px, ref


def test_audio_tower_against_the_restatement():
    tower, cfg, sd, px, ref = _tower_case()
    out = tower.encode_spectrograms(px.to(DEV))
    torch.cuda.synchronize()
    e = _cos_err(out, ref)
    print(f"AUDIO_TOWER bins=16 L=40 P=8 B=3 max(1-cos)={e:.2e}")
    assert out.shape == (3, cfg["projection_dim"]) and bool(torch.isfinite(out).all())
    assert float((out.norm(dim=-1) - 1).abs().max()) <= 1e-5
    assert e <= COS_TOL, e
    raw = tower.encode_spectrograms(px, normalize=False)               # (a host tensor in; the un-normalised rows point the same way)
    assert _cos_err(raw, out) <= 1e-6
    with pytest.raises(ValueError, match=r"\[b, 3, 16, 40\]"):
        tower.encode_spectrograms(px.transpose(2, 3).contiguous())


def test_a_transposed_grid_is_visible():
    """the same numbers with the picture's two axes swapped and reshaped back: what a tower that walked the grid column-first would see"""
    tower, cfg, sd, px, ref = _tower_case()
    swapped = px.transpose(2, 3).contiguous().reshape(px.shape)
    a, t = tower.encode_spectrograms(px), tower.encode_spectrograms(swapped)
    torch.cuda.synchronize()
    noise, moved = _cos_err(a, ref), _cos_err(a, t)
    want = _cos_err(ref, LBR.embed(AR.audio_forward(sd, cfg, swapped), sd, "audio", True))
    print(f"AUDIO_GRID_ORDER noise={noise:.2e} moved={moved:.2e} restatement_moved={want:.2e}")
    assert moved > max(COS_TOL, 10 * noise), (moved, noise)
    assert abs(moved - want) <= 2 * COS_TOL


def test_a_checkpoint_with_square_positions_is_refused():
    from marqo_amd.engine import archs
    from marqo_amd.engine.languagebind import LanguageBindAudioTower
    cfg = AR.config()
    sd = dict(AR.synthetic_state_dict(cfg, seed=3))
    sd["vision_model.embeddings.position_embedding.weight"] = torch.zeros(5, AR.SMALL["W"])
    with pytest.raises(ValueError, match="5 rows.*needs 11"):
        LanguageBindAudioTower(archs.languagebind_arch_from_hf_config(cfg), sd, DEV)


# ---- 5. end to end -----------------------------------------------------------------------------------------------------------------------------------
def test_vectorise_audio_end_to_end(tmp_path, monkeypatch):
    from marqo_amd.engine.audio import AudioPreprocessor, default_starts
    from marqo_amd.engine.hf_clip import load_tokenizer
    from marqo_amd.s2_inference import s2_inference as S
    from marqo_amd.s2_inference.enums import Modality
    monkeypatch.setenv("MARQO_MAX_CUDA_MODEL_MEMORY", "64")
    name = "LanguageBind/Audio_FT_Image"
    parts = AR.write_model(tmp_path, image=True, seed=4)
    (acfg, asd), (icfg, isd) = parts["audio"], parts["image"]
    bins, L_ = AR.SMALL["bins"], AR.SMALL["L"]
    props = {"name": name, "dimensions": AR.SMALL["D"], "type": "languagebind", "loader": "languagebind", "model_size": 1,
             "supported_modalities": ["audio", "language", "image"], "video_chunk_length": 20, "audio_chunk_length": 10, "localpath": str(tmp_path)}
    S.clear_loaded_models()
    try:
        vec = lambda content, modality, norm: np.asarray(S.vectorise(name, content, model_properties=dict(props), device=DEV, modality=modality,
                                                                     normalize_embeddings=norm))
        norms = lambda a: np.linalg.norm(a, axis=1)
        model, pre = S.load_multimodal_model_and_get_preprocessors(name, dict(props), device=DEV)
        assert isinstance(pre["audio"], AudioPreprocessor) and pre["audio"] is model.preprocessor(Modality.AUDIO) and pre["video"] is None
        # one second of sound: 98 log-mel rows against target_length 40, the long-clip path with the default starts
        waves = [AR.make_waveform(16000, seed=1), AR.make_waveform(16000, seed=2)]
        px = pre["audio"](waves)["pixel_values"]
        assert px.shape == (2, 3, bins, L_) and px.dtype == torch.float32 and px.device.type == "cuda"
        starts = default_starts(98, L_)
        assert starts == (9, 29, 49)
        ref_px = torch.stack([AR.fusion_ref(torch.from_numpy(AR.fbank_ref(w.numpy(), bins)), L_, MEAN, STD, starts) for w in waves]).float()
        assert float((px.cpu() - ref_px).abs().max()) <= 1e-5            # (pictures of magnitude ~1 in float32: a few ulp of 1.2e-7 each way)
        # explicit starts reproduce any draw; a (waveform, rate) pair and an ndarray are the same waveform
        drawn = pre["audio"]((waves[0].numpy(), 16000), starts=(0, 58, 3))["pixel_values"]
        want = AR.fusion_ref(torch.from_numpy(AR.fbank_ref(waves[0].numpy(), bins)), L_, MEAN, STD, (0, 58, 3)).float()
        assert float((drawn[0].cpu() - want).abs().max()) <= 1e-5
        # a short clip: repeated to length
        short = pre["audio"](waves[1][:2000])["pixel_values"]
        want = AR.fusion_ref(torch.from_numpy(AR.fbank_ref(waves[1][:2000].numpy(), bins)), L_, MEAN, STD).float()
        assert float((short[0].cpu() - want).abs().max()) <= 1e-5
        # the embeddings: unit rows with normalize, exp(logit_scale) of the audio part without; the reference chain within the tower's bound
        content = [{"pixel_values": px}]
        a_unit, a_raw = vec(content, Modality.AUDIO, True), vec(content, Modality.AUDIO, False)
        assert a_unit.shape == (2, AR.SMALL["D"]) and np.allclose(norms(a_unit), 1.0, atol=1e-5)
        assert np.allclose(norms(a_raw), math.exp(float(asd["logit_scale"])), rtol=1e-5)
        ref_a = LBR.embed(AR.audio_forward(asd, acfg, ref_px), asd, "audio", True)
        e = _cos_err(torch.from_numpy(a_unit), ref_a)
        print(f"AUDIO_END_TO_END max(1-cos)={e:.2e}")
        assert e <= COS_TOL
        assert _cos_err(torch.from_numpy(vec([{"pixel_values": px[:1].cpu()}, {"pixel_values": px[1:]}], Modality.AUDIO, True)), ref_a) <= COS_TOL
        # text: the LAST part's tower (the image part's)
        texts = ["the red cat on a dog", "a dog"]
        t_unit = vec(texts, Modality.TEXT, True)
        tok = load_tokenizer(str(tmp_path / LBR.IMAGE_PART), LBR.CTX)
        ids = torch.full((len(texts), LBR.CTX), tok.eot_id, dtype=torch.int64)
        for i, t in enumerate(texts):
            row = [tok.sot_id] + tok.encode(t) + [tok.eot_id]
            ids[i, :len(row)] = torch.tensor(row)
        ref_t = LBR.embed(LBR.text_forward(isd, icfg, ids), isd, "language", True)
        assert np.allclose(norms(t_unit), 1.0, atol=1e-5) and _cos_err(torch.from_numpy(t_unit), ref_t) <= COS_TOL
        assert float(np.abs(t_unit @ a_unit.T - (ref_t @ ref_a.T).numpy()).max()) <= 2e-3
        # what is no spectrogram of this model
        for bad in (["https://example.com/a.wav"], [{"pixel_values": px.transpose(2, 3).contiguous()}]):
            with pytest.raises(ValueError, match="Unsupported audio content type"):
                S.vectorise(name, bad, model_properties=dict(props), device=DEV, modality=Modality.AUDIO)
    finally:
        S.clear_loaded_models()


def test_audio_only_name_uses_the_audio_parts_text_tower(tmp_path, monkeypatch):
    """`LanguageBind/Audio_FT`: the last part is the audio part, so its vocab.json / merges.txt and text_model.* are the model's"""
    from marqo_amd.engine.hf_clip import load_tokenizer
    from marqo_amd.s2_inference import s2_inference as S
    from marqo_amd.s2_inference.enums import Modality
    monkeypatch.setenv("MARQO_MAX_CUDA_MODEL_MEMORY", "64")
    name = "LanguageBind/Audio_FT"
    acfg, asd = AR.write_model(tmp_path, image=False, seed=6)["audio"]
    props = {"name": name, "dimensions": AR.SMALL["D"], "type": "languagebind", "loader": "languagebind", "model_size": 1,
             "supported_modalities": ["audio", "language"], "video_chunk_length": 20, "audio_chunk_length": 10, "localpath": str(tmp_path)}
    S.clear_loaded_models()
    try:
        texts = ["a dog"]
        t_unit = np.asarray(S.vectorise(name, texts, model_properties=dict(props), device=DEV, modality=Modality.TEXT))
        tok = load_tokenizer(str(tmp_path / AR.AUDIO_PART), LBR.CTX)
        ids = torch.full((1, LBR.CTX), tok.eot_id, dtype=torch.int64)
        row = [tok.sot_id] + tok.encode(texts[0]) + [tok.eot_id]
        ids[0, :len(row)] = torch.tensor(row)
        ref_t = LBR.embed(LBR.text_forward(asd, acfg, ids), asd, "language", True)
        assert _cos_err(torch.from_numpy(t_unit), ref_t) <= COS_TOL
        with pytest.raises(ValueError, match="has no image part"):
            S.vectorise(name, [torch.zeros(3, 32, 32)], model_properties=dict(props), device=DEV, modality=Modality.IMAGE)
    finally:
        S.clear_loaded_models()

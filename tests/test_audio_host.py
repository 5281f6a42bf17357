"""The LanguageBind audio part without a GPU: arch parsing of an audio config, the restatements of tests/audio_ref.py against each other and
against a second statement of the reference's crop draw, the default-start rule, what AudioPreprocessor and encode(..., AUDIO) accept and refuse, the
loader with and without the audio part's directory, and the argument checks of the three entry points of csrc/audio.hip."""
import numpy as np
import pytest
import torch

from marqo_amd import _lib as L
from marqo_amd.engine import archs
from marqo_amd.engine import audio as A
from marqo_amd.engine import languagebind as LB
from marqo_amd.s2_inference import multimodal_model_load as MM
from marqo_amd.s2_inference import s2_inference as S
from marqo_amd.s2_inference.enums import Modality
from marqo_amd.s2_inference.errors import InvalidModelPropertiesError, ModelLoadError
from tests import audio_ref as AR
from tests import languagebind_ref as LBR

AUDIO_NAMES = ("LanguageBind/Video_V1.5_FT_Audio_FT_Image", "LanguageBind/Video_V1.5_FT_Audio_FT", "LanguageBind/Audio_FT_Image", "LanguageBind/Audio_FT")


def props(name, **extra):
    mods = [m for m, part in (("video", "Video"), ("audio", "Audio"), ("language", ""), ("image", "Image")) if part in name]
    return dict({"name": name, "dimensions": 64, "type": "languagebind", "loader": "languagebind", "model_size": 1, "supported_modalities": mods,
                 "video_chunk_length": 20, "audio_chunk_length": 10}, **extra)


# ---- arch ------------------------------------------------------------------------------------------------------------------------------------------
def test_arch_of_an_audio_config():
    a = archs.languagebind_arch_from_hf_config(AR.config())
    assert a.is_audio and (a.num_mel_bins, a.target_length, a.audio_sample_rate) == (16, 40, 16000)
    assert (a.audio_mean, a.audio_std) == (-4.2677393, 4.5689974)
    assert (a.grid_h, a.grid_w, a.tokens, a.image_hw) == (2, 5, 11, (16, 40)) and AR.tokens(AR.config()) == 11
    assert not a.add_time_attn and a.num_frames == 1
    # the released checkpoint's picture: 112 x 1036 at patch 14
    big = archs.languagebind_arch_from_hf_config(AR.config(dict(AR.SMALL, P=14, bins=112, L=1036)))
    assert (big.grid_h, big.grid_w, big.tokens) == (8, 74, 593)


def test_square_parts_are_unchanged():
    for add in (True, False):
        a = archs.languagebind_arch_from_hf_config(LBR.config(LBR.SMALL, add_time_attn=add))
        assert not a.is_audio and (a.num_mel_bins, a.target_length, a.audio_sample_rate, a.audio_mean, a.audio_std) == (0, 0, 16000, 0.5, 0.5)
        assert (a.grid, a.grid_h, a.grid_w, a.tokens, a.image_hw) == (2, 2, 2, 5, (32, 32))
    # one of the two audio keys alone does not make an audio part (modeling_audio.py:769)
    half = LBR.config(LBR.SMALL, add_time_attn=False)
    half["vision_config"]["num_mel_bins"] = 16
    assert archs.languagebind_arch_from_hf_config(half).tokens == 5


# ---- the restatements ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bins", [112, 16])
def test_the_two_fbank_restatements_agree(bins):
    for n, channels in ((400, None), (559, None), (560, None), (4000 + 7, None), (1200, 2)):
        w = AR.make_waveform(n, seed=n + bins, channels=channels)
        ref = AR.fbank_ref(w.numpy(), bins)
        assert ref.shape == (AR.num_frames(n), bins)
        y64 = AR.fbank_torch(w, bins, torch.float64).numpy()
        assert float(np.abs(y64 - ref).max()) <= 1e-9
        y32 = AR.fbank_torch(w, bins, torch.float32).numpy()
        assert y32.dtype == np.float32 and float(np.abs(y32 - ref).max()) <= 1e-2        # (float32: the same numbers, coarsely)
    assert AR.num_frames(559) == 1 and AR.num_frames(560) == 2 and AR.num_frames(16000) == 98 and AR.num_frames(160000) == 998
    # the bank leaves out DC, and between the first and the last centre (134 Hz and 6.8 kHz for 16 filters) the two triangles over a bin sum to 1
    banks = AR.mel_banks_ref(16)
    assert banks.shape == (16, 256) and banks[:, 0].max() == 0.0 and float(banks.max()) <= 1.0
    assert float(np.abs(banks.sum(0)[5:215] - 1.0).max()) <= 1e-12 and bool(((banks > 0).sum(0) <= 2).all())


def test_fbank_of_silence_is_the_floor():
    z = torch.zeros(1000)
    want = np.log(np.float64(AR.EPS32))
    assert bool((AR.fbank_ref(z.numpy(), 16) == want).all())
    assert bool((AR.fbank_torch(z, 16, torch.float32).numpy() == np.float32(want)).all())


def test_fbank_ref_against_torchaudio():
    """parity of the restatement with torchaudio itself, where it is installed"""
    torchaudio = pytest.importorskip("torchaudio")
    for bins in (112, 16):
        w = AR.make_waveform(16000 + 7, seed=bins)
        x = w.clone().unsqueeze(0)
        x -= x.mean()
        got = torchaudio.compliance.kaldi.fbank(x, htk_compat=True, sample_frequency=16000, use_energy=False, window_type="hanning", num_mel_bins=bins,
                                                dither=0.0, frame_length=25, frame_shift=10)
        ours32 = AR.fbank_torch(w, bins, torch.float32)
        ref = AR.fbank_ref(w.numpy(), bins)
        yard = float(np.abs(ours32.numpy().astype(np.float64) - ref).max())
        assert got.shape == ours32.shape
        assert float(np.abs(got.numpy().astype(np.float64) - ref).max()) <= 4 * yard


def _crops_as_the_reference_draws_them(rows, L, mean, std, pick):
    """a second statement of AudioTransform.waveform2melspec, with np.random.choice replaced by `pick` through monkeypatching by the caller"""
    total = rows.shape[0]
    if total > L:
        thirds = np.array_split(list(range(0, total - L + 1)), 3)
        thirds = [t if len(t) else [0] for t in thirds]
        idx = [int(np.random.choice(t)) for t in thirds]
        fused = torch.stack([rows[i:i + L] for i in idx])
    elif total < L:
        tiled = rows.repeat(int(L / total) + 1, 1)[:L]
        fused, idx = torch.stack([tiled] * 3), [0, 0, 0]
    else:
        fused, idx = torch.stack([rows] * 3), [0, 0, 0]
    return (fused.transpose(1, 2) - mean) / (std * 2), tuple(idx)


@pytest.mark.parametrize("m", [7, 39, 40, 41, 42, 100])
@pytest.mark.parametrize("which", ["first", "last", "middle"])
def test_fusion_ref_against_the_draw(monkeypatch, m, which):
    L_, bins = 40, 16
    pick = {"first": lambda r: r[0], "last": lambda r: r[-1], "middle": lambda r: r[(len(r) - 1) // 2]}[which]
    monkeypatch.setattr(np.random, "choice", pick)
    rows = torch.randn(m, bins, generator=torch.Generator().manual_seed(m))
    want, idx = _crops_as_the_reference_draws_them(rows, L_, -4.27, 4.57, pick)
    got = AR.fusion_ref(rows, L_, -4.27, 4.57, idx)
    assert got.shape == (3, bins, L_) and torch.equal(got, want)
    if which == "middle":
        assert A.default_starts(m, L_) == idx                         # the engine's default is the middle element of each third
    if m > L_:
        assert all(0 <= i <= m - L_ for i in idx)
        # the picture's column t of crop c is row idx[c] + t
        assert torch.equal(got[2, :, 3], (rows[idx[2] + 3] + 4.27) / (4.57 * 2))
    else:
        assert torch.equal(got[1, :, L_ - 1], (rows[(L_ - 1) % m] + 4.27) / (4.57 * 2))      # repeated to length: row t mod m


def test_default_starts():
    assert A.default_starts(40, 40) == (0, 0, 0) and A.default_starts(7, 40) == (0, 0, 0)
    assert A.default_starts(41, 40) == (0, 1, 0)              # range(0, 2) splits into [0], [1], []: the empty third falls back to 0
    assert A.default_starts(42, 40) == (0, 1, 2)
    assert A.default_starts(100, 40) == (10, 30, 50)          # 61 starts: thirds of 21, 20, 20 -> their middles
    assert A.default_starts(98, 40) == (9, 29, 49)            # 59 starts: 20, 20, 19
    assert A.num_frames(399) == 0 and A.num_frames(400) == 1 and A.num_frames(16000) == 98
    m, L_ = 5000, 1036
    assert all(0 <= s <= m - L_ for s in A.default_starts(m, L_))


# ---- AudioPreprocessor: what it refuses before anything reaches a device ---------------------------------------------------------------------------
def test_preprocessor_refusals():
    pre = A.AudioPreprocessor("cuda:0", 16, 40, 16000, -4.27, 4.57)
    w = AR.make_waveform(1000)
    with pytest.raises(ValueError, match="44100 Hz.*16000 Hz.*no resampler"):
        pre((w, 44100))
    for bad in ("/data/a.wav", "https://example.com/a.mp3", b"RIFF....WAVE", ["/data/a.wav"]):
        with pytest.raises(ValueError, match="Unsupported audio content type"):
            pre(bad)
    with pytest.raises(ValueError, match="399 samples is shorter than one 400-sample frame"):
        pre(w[:399])
    with pytest.raises(ValueError, match="shorter than one"):
        pre([w, (w[:10].numpy(), 16000)])
    for bad in (torch.zeros(2, 3, 1000), torch.zeros(1000, dtype=torch.int16), 7, None, []):
        with pytest.raises(ValueError, match="Unsupported audio content type"):
            pre(bad)
    with pytest.raises(ValueError, match="starts"):
        pre(AR.make_waveform(16000), starts=(0, 1))
    with pytest.raises(ValueError, match=r"outside \[0, 58\]"):
        pre(AR.make_waveform(16000), starts=(0, 30, 59))         # 98 rows: 58 + 40 == 98 is the last legal start
    with pytest.raises(ValueError, match="repeated to length, not cropped"):
        pre(w, starts=(0, 0, 1))
    with pytest.raises(ValueError, match="16000 Hz only"):
        A.AudioPreprocessor("cuda:0", 16, 40, 44100)
    with pytest.raises(ValueError, match="mel bins"):
        A.AudioPreprocessor("cuda:0", 129, 40)


# ---- encode(..., AUDIO): routing ---------------------------------------------------------------------------------------------------------------------
def test_audio_content_routing():
    class FakeLB:
        def __init__(self, audio):
            self.calls = []
            if audio:
                self.audio = type("T", (), {"arch": archs.languagebind_arch_from_hf_config(AR.config())})()

        def encode_audio(self, px, normalize):
            self.calls.append((tuple(px.shape), normalize))
            return torch.zeros(px.shape[0], 4)

        def audio_preprocessor(self):
            return "the preprocessor"

    name = AUDIO_NAMES[2]
    m = MM.MultimodalModel(name, props(name), "cuda:0")
    m.model, m.encoder = FakeLB(True), MM.LanguageBindEncoder(m)
    a, b = torch.zeros(1, 3, 16, 40), torch.ones(2, 3, 16, 40)
    assert m.encode([{"pixel_values": a}, {"pixel_values": b}], Modality.AUDIO, normalize=False).shape == (3, 4)     # every item
    assert m.encode({"pixel_values": b}, Modality.AUDIO).shape == (2, 4) and m.encode(a, "audio").shape == (1, 4)
    assert m.model.calls == [((1, 3, 16, 40), False), ((2, 3, 16, 40), False), ((2, 3, 16, 40), True), ((1, 3, 16, 40), True)]
    for bad in ("https://example.com/a.wav", ["a.wav"], [], torch.zeros(1, 3, 40, 16), torch.zeros(3, 16, 40), [{"pixel_values": torch.zeros(1, 3, 8, 16, 40)}],
                [{"pixels": a}]):
        with pytest.raises(ValueError, match="Unsupported audio content type"):
            m.encode(bad, Modality.AUDIO)
    assert m.preprocessor(Modality.AUDIO) == "the preprocessor" and m.preprocessor(Modality.VIDEO) is None and m.preprocessor(Modality.IMAGE) is None
    # a model without an audio part: the reference's ValueError, and no preprocessor
    m.model, m.encoder = FakeLB(False), MM.LanguageBindEncoder(m)
    with pytest.raises(ValueError, match="Unsupported audio content type"):
        m.encode([{"pixel_values": a}], Modality.AUDIO)
    assert m.preprocessor(Modality.AUDIO) is None
    assert Modality.AUDIO in MM.SERVED_MODALITIES


# ---- the loader ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", AUDIO_NAMES)
def test_audio_name_without_its_directory(tmp_path, name):
    """the audio part's directory is looked for first: without it the properties are invalid, whatever else is (not) there"""
    (tmp_path / LBR.IMAGE_PART).mkdir()
    for lp in (None, str(tmp_path / "absent"), str(tmp_path)):
        with pytest.raises(InvalidModelPropertiesError, match=AR.AUDIO_PART):
            S._load_model(name, props(name, **({"localpath": lp} if lp else {})), device="cuda:0", calling_func="unit_test")
    (tmp_path / AR.AUDIO_PART).mkdir()                        # a directory that is no checkpoint
    with pytest.raises(InvalidModelPropertiesError, match="config.json"):
        S._load_model(name, props(name, localpath=str(tmp_path)), device="cuda:0", calling_func="unit_test")


def test_audio_name_with_its_directory_builds_the_model(tmp_path, monkeypatch):
    seen = {}

    class FakeModel:
        audio = object()

        def __init__(self, name, localpath, device, precision="bf16"):
            seen.update(name=name, localpath=localpath, device=device)

        def audio_preprocessor(self):
            return "pre"

    monkeypatch.setattr(LB, "LanguageBindModel", FakeModel)
    cfg = AR.config()
    AR.write_part(tmp_path / AR.AUDIO_PART, cfg, AR.synthetic_state_dict(cfg))
    name = "LanguageBind/Audio_FT"
    m = S._load_model(name, props(name, localpath=str(tmp_path)), device="cuda:0", calling_func="unit_test")
    assert isinstance(m, MM.MultimodalModel) and isinstance(m.model, FakeModel) and seen == dict(name=name, localpath=str(tmp_path), device="cuda:0")
    assert m.clip_type == {"audio": "LanguageBind_Audio_FT"}
    assert m.preprocessor(Modality.AUDIO) == "pre" and m.preprocessor(Modality.VIDEO) is None
    # fp8 stays refused, and a video part that is missing next to a present audio part is still the load error
    with pytest.raises(InvalidModelPropertiesError, match="bf16"):
        S._load_model(name, props(name, localpath=str(tmp_path), enginePrecision="fp8"), device="cuda:0", calling_func="unit_test")
    monkeypatch.undo()
    both = "LanguageBind/Video_V1.5_FT_Audio_FT"
    with pytest.raises(ModelLoadError, match="LanguageBind_Video_V1.5_FT"):
        S._load_model(both, props(both, localpath=str(tmp_path)), device="cuda:0", calling_func="unit_test")


def test_audio_tower_refuses_what_is_no_audio_part():
    """checked before anything is put on a device"""
    cfg = AR.config()
    sd = AR.synthetic_state_dict(cfg)
    arch = archs.languagebind_arch_from_hf_config
    with pytest.raises(ValueError, match="num_mel_bins"):
        LB.LanguageBindAudioTower(arch(LBR.config(LBR.SMALL, add_time_attn=False)), sd, "cuda:0")
    with pytest.raises(ValueError, match="add_time_attn = True"):
        LB.LanguageBindAudioTower(arch(AR.config(add_time_attn=True)), sd, "cuda:0")
    with pytest.raises(ValueError, match="num_frames = 8"):
        LB.LanguageBindAudioTower(arch(AR.config(num_frames=8)), sd, "cuda:0")
    with pytest.raises(ValueError, match="16 x 44"):          # 44 % 8: no whole grid
        LB.LanguageBindAudioTower(arch(AR.config(dict(AR.SMALL, L=44))), sd, "cuda:0")


# ---- the entry points' argument checks (no launch: fake, never dereferenced pointers) ---------------------------------------------------------------
def test_entry_points_judge_their_arguments():
    lib = L.load()
    fake = 256

    def refused(rc, *msgs):
        assert rc == -1
        err = lib.mq_last_error()
        for msg in msgs:
            assert msg in err, err

    refused(lib.mq_fbank(fake, 16000, 16000, 16000, 0, fake, fake, None), b"mq_fbank: bins=0")
    refused(lib.mq_fbank(fake, 16000, 16000, 16000, 129, fake, fake, None), b"mq_fbank: bins=129")
    refused(lib.mq_fbank(fake, 399, 399, 16000, 16, fake, fake, None), b"mq_fbank: n=399")
    refused(lib.mq_fbank(fake, 16000, 16000, 44100, 16, fake, fake, None), b"mq_fbank: sample_rate=44100")
    refused(lib.mq_fbank(fake, 16000, 15999, 16000, 16, fake, fake, None), b"mq_fbank: n=16000, n_mean=15999")
    for args in ((None, fake, fake), (fake, None, fake), (fake, fake, None)):
        refused(lib.mq_fbank(args[0], 16000, 16000, 16000, 16, args[1], args[2], None), b"mq_fbank: null pointer")
    refused(lib.mq_fbank(fake, 16000, 16000, 16000, 16, fake, fake + 4, None), b"mq_fbank:", b"8-byte aligned")
    refused(lib.mq_mel_fusion(fake, 98, 0, 0, 0, 0, 0.5, 0.5, fake, 40, None), b"mq_mel_fusion: bins=0")
    refused(lib.mq_mel_fusion(fake, 98, 129, 0, 0, 0, 0.5, 0.5, fake, 40, None), b"mq_mel_fusion: bins=129")
    refused(lib.mq_mel_fusion(fake, 0, 16, 0, 0, 0, 0.5, 0.5, fake, 40, None), b"mq_mel_fusion: m=0")
    refused(lib.mq_mel_fusion(fake, 98, 16, 0, 98, 0, 0.5, 0.5, fake, 40, None), b"mq_mel_fusion: start[1]=98")
    refused(lib.mq_mel_fusion(fake, 98, 16, 0, 0, -1, 0.5, 0.5, fake, 40, None), b"mq_mel_fusion: start[2]=-1")
    refused(lib.mq_mel_fusion(fake, 98, 16, 0, 0, 0, 0.5, 0.0, fake, 40, None), b"mq_mel_fusion:", b"std")
    refused(lib.mq_mel_fusion(fake, 98, 16, 0, 0, 0, 0.5, 0.5, fake, 0, None), b"mq_mel_fusion: L=0")
    refused(lib.mq_mel_fusion(None, 98, 16, 0, 0, 0, 0.5, 0.5, fake, 40, None), b"mq_mel_fusion: null pointer")
    refused(lib.mq_mel_fusion(fake, 98, 16, 0, 0, 0, 0.5, 0.5, None, 40, None), b"mq_mel_fusion: null pointer")
    refused(lib.mq_patchify_rect(fake, fake, 1, 20, 40, 8, 192, None), b"mq_patchify_rect: H=20")
    refused(lib.mq_patchify_rect(fake, fake, 1, 16, 44, 8, 192, None), b"mq_patchify_rect:", b"Wd=44")
    refused(lib.mq_patchify_rect(fake, fake, 1, 16, 40, 8, 188, None), b"mq_patchify_rect: Kp=188")
    refused(lib.mq_patchify_rect(fake, fake, 1, 16, 40, 8, 184, None), b"mq_patchify_rect: Kp=184")
    refused(lib.mq_patchify_rect(None, fake, 1, 16, 40, 8, 192, None), b"mq_patchify_rect: null pointer")
    refused(lib.mq_patchify_rect(fake, None, 1, 16, 40, 8, 192, None), b"mq_patchify_rect: null pointer")
    assert lib.mq_patchify_rect(None, None, 0, 16, 40, 8, 192, None) == 0           # nothing to do
    assert "audio" in L.NO_SCRATCH_UNITS and L.MQ_FBANK_WS_BYTES == 2048

"""The audio resampler without a GPU: the polyphase tap table of engine/audio.py against the fp64 restatement of tests/resample_ref.py, the two
restatements against each other (and against torchaudio where it is installed), the output-length rule, what AudioPreprocessor does with a rate with
and without the opt-in, the cap on the table, the `resampleAudio` model property, and mq_resample's argument checks."""
import math

import numpy as np
import pytest
import torch

from marqo_amd import _lib as L
from marqo_amd.engine import audio as A
from marqo_amd.s2_inference import multimodal_model_load as MM
from marqo_amd.s2_inference.enums import Modality
from marqo_amd.s2_inference.errors import InvalidModelPropertiesError
from tests import audio_ref as AR
from tests import resample_ref as RR

SHAPES = {(44100, 16000): (441, 160, 17, 475), (48000, 16000): (3, 1, 19, 41), (22050, 16000): (441, 320, 9, 459), (8000, 16000): (1, 2, 7, 15),
          (32000, 16000): (2, 1, 13, 28)}


# ---- the table ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", RR.PAIRS)
def test_tap_table_against_the_restatement(pair):
    o, n, width, K = SHAPES[pair]
    assert A.resample_plan(*pair) == (o, n, width) and RR.plan(*pair)[:2] + RR.plan(*pair)[3:] == (o, n, width, K)
    taps = A.resample_taps(*pair)
    ref = RR.taps_ref(*pair)
    assert taps.dtype == np.float64 and taps.shape == ref.shape == (n, K)
    assert float(np.abs(taps - ref).max()) <= 1e-12
    # the reduced pair gives the same table: the rates enter through o and n only
    assert np.array_equal(A.resample_taps(o, n), taps)
    # DC gain: every phase sums to 1 within the filter's own ripple (a Hann-windowed sinc of 6 zero crossings cut at 0.99 of Nyquist: the sum
    # over the taps is the filter's response at DC sampled on a grid of 1 / o, off 1 by the aliased stop-band, below 1e-3 for every pair here)
    sums = taps.sum(axis=1)
    print(f"RESAMPLE_TAPS {pair[0]}->{pair[1]} o={o} n={n} width={width} K={K} phase sums in [{sums.min():.6f}, {sums.max():.6f}]")
    assert float(np.abs(sums - 1.0).max()) <= 1e-3
    # phase 0 peaks at the tap over its own input sample, k = width
    assert int(np.abs(taps[0]).argmax()) == width


def test_plan_widths_follow_the_formula():
    for orig, new in RR.PAIRS + ((11025, 16000), (96000, 16000), (16000, 8000)):
        g = math.gcd(orig, new)
        o, n = orig // g, new // g
        assert A.resample_plan(orig, new) == (o, n, int(math.ceil(6 * o / (min(o, n) * 0.99))))


@pytest.mark.parametrize("pair", RR.PAIRS)
def test_output_length_rule(pair):
    o, n = SHAPES[pair][:2]
    for length in RR.lengths(*pair) + [1, 2, 1000, 160000]:
        want = -((-n * length) // o)                                   # ceil(n len / o) in integers
        assert A.resample_length(length, *pair) == want == RR.out_length(length, *pair)
        assert RR.resample_ref(np.zeros(length), *pair).shape == (want,)
        # the frames the padded waveform holds cover it: floor(len / o) + 1 frames of n phases
        assert (length // o + 1) * n >= want


# ---- the restatements --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", RR.PAIRS)
def test_the_two_restatements_agree(pair):
    for length in RR.lengths(*pair):
        w = RR.make_wave(length, *pair, seed=length)
        ref = RR.resample_ref(w.numpy(), *pair)
        y64 = RR.resample_torch(w, *pair, dtype=torch.float64).numpy()
        assert y64.shape == ref.shape and float(np.abs(y64 - ref).max()) <= 1e-12
        y32 = RR.resample_torch(w, *pair, dtype=torch.float32).numpy()
        assert y32.dtype == np.float32 and float(np.abs(y32 - ref).max()) <= 1e-4       # (float32: the same numbers, coarsely)
    w2 = RR.make_wave(700, *pair, seed=2, channels=2)
    ref2 = RR.resample_ref(w2.numpy(), *pair)
    assert ref2.shape[0] == 2 and float(np.abs(ref2[1] - RR.resample_ref(w2[1].numpy(), *pair)).max()) <= 1e-13      # every channel on its own


def test_a_tone_in_the_passband_keeps_its_amplitude():
    """1 kHz at 44.1 kHz comes out as 1 kHz at 16 kHz: the restatement resamples, it does not merely filter"""
    n = 44100 // 5
    x = np.sin(2 * np.pi * 1000.0 * np.arange(n) / 44100.0)
    y = RR.resample_ref(x, 44100, 16000)
    want = np.sin(2 * np.pi * 1000.0 * np.arange(y.shape[0]) / 16000.0)
    assert float(np.abs(y - want)[100:-100].max()) <= 2e-3


def test_resample_ref_against_torchaudio():
    """parity of the restatement with torchaudio itself, where it is installed"""
    torchaudio = pytest.importorskip("torchaudio")
    for pair in RR.PAIRS:
        w = RR.make_wave(int(0.2 * pair[0]) + 7, *pair, seed=1, channels=2)
        got = torchaudio.functional.resample(w.double(), *pair).numpy()
        ref = RR.resample_ref(w.numpy(), *pair)
        assert got.shape == ref.shape and float(np.abs(got - ref).max()) <= 1e-9


# ---- rates: AudioPreprocessor with and without the opt-in, the cap -------------------------------------------------------------------------------
def test_rate_handling_before_anything_reaches_a_device():
    w = AR.make_waveform(4000)
    plain = A.AudioPreprocessor("cuda:0", 16, 40, 16000, -4.27, 4.57)
    assert plain.resample is False
    with pytest.raises(ValueError, match="44100 Hz.*16000 Hz.*no resampler"):          # exactly as before the resampler existed
        plain((w, 44100))
    opt = A.AudioPreprocessor("cuda:0", 16, 40, 16000, -4.27, 4.57, resample=True)
    assert opt.resample is True
    item, rate = opt._waveform((w, 44100))                                              # accepted: judged on the host, nothing moved
    assert item is w and rate == 44100
    assert opt._waveform((w, 16000))[1] == 16000 and opt._waveform(w)[1] == 16000
    # 1102 samples at 44.1 kHz are 400 at 16 kHz, one frame; 1101 are 399.46 -> ceil 400 too; 1099 are 399
    assert A.resample_length(1102, 44100, 16000) == 400 and A.resample_length(1099, 44100, 16000) == 399
    opt._waveform((w[:1102], 44100))
    with pytest.raises(ValueError, match=r"399 samples \(1099 at 44100 Hz\) is shorter than one 400-sample frame"):
        opt((w[:1099], 44100))
    # a prime rate: the table cap, with the figures
    with pytest.raises(ValueError, match=r"44101 Hz to 16000 Hz is not served.*over the cap of 2097152 entries"):
        opt((w, 44101))
    with pytest.raises(ValueError, match="not served"):
        A.resample_taps(44101, 16000)
    with pytest.raises(ValueError, match="not served"):
        A.resample(w, 44101, 16000, "cuda:0")
    # what was refused stays refused with the opt-in
    for bad in ("/data/a.wav", b"RIFF....WAVE", torch.zeros(1000, dtype=torch.int16), []):
        with pytest.raises(ValueError, match="Unsupported audio content type"):
            opt(bad)
    with pytest.raises(ValueError, match="16000 Hz only"):
        A.AudioPreprocessor("cuda:0", 16, 40, 44100, resample=True)
    for bad in ((w.numpy().astype(np.int16), 44100, 16000), (torch.zeros(2, 3, 10), 44100, 16000), (torch.zeros(0), 44100, 16000)):
        with pytest.raises(ValueError, match="a waveform to resample"):
            A.resample(bad[0], bad[1], bad[2], "cuda:0")
    with pytest.raises(ValueError, match="positive integers"):
        A.resample(w, 0, 16000, "cuda:0")


def test_the_resample_audio_property_reaches_the_preprocessor():
    class FakeLB:
        audio = object()

        def __init__(self):
            self.asked = []

        def audio_preprocessor(self, resample=False):
            self.asked.append(resample)
            return ("pre", resample)

    name = "LanguageBind/Audio_FT"
    props = {"name": name, "dimensions": 64, "type": "languagebind", "loader": "languagebind", "model_size": 1,
             "supported_modalities": ["audio", "language"], "video_chunk_length": 20, "audio_chunk_length": 10}
    for extra, want in (({}, False), ({"resampleAudio": False}, False), ({"resampleAudio": True}, True)):
        m = MM.MultimodalModel(name, dict(props, **extra), "cuda:0")
        assert m.resample_audio is want
        m.model, m.encoder = FakeLB(), MM.LanguageBindEncoder(m)
        assert m.preprocessor(Modality.AUDIO) == ("pre", want) and m.preprocessor(Modality.AUDIO) == ("pre", want)
        assert m.model.asked == [want]                                                  # built once
    with pytest.raises(InvalidModelPropertiesError, match="resampleAudio"):
        MM.MultimodalModel(name, dict(props, resampleAudio="yes"), "cuda:0")


# ---- the entry point's argument checks (no launch: fake, never dereferenced pointers) ------------------------------------------------------------
def test_entry_point_judges_its_arguments():
    lib = L.load()
    fake = 256

    def refused(rc, *msgs):
        assert rc == -1
        err = lib.mq_last_error()
        for msg in msgs:
            assert msg in err, err

    refused(lib.mq_resample(fake, 1, 1000, fake, 0, 160, 17, fake, None), b"mq_resample: o=0")
    refused(lib.mq_resample(fake, 1, 1000, fake, 441, 160, 0, fake, None), b"mq_resample:", b"width=0")
    refused(lib.mq_resample(fake, 1, 1000, fake, 882, 320, 17, fake, None), b"mq_resample: o=882, n=320", b"coprime")
    refused(lib.mq_resample(fake, 1, 1000, fake, 1, 1, 7, fake, None), b"mq_resample: o == n")
    refused(lib.mq_resample(fake, 1, 1000, fake, 44101, 16000, 17, fake, None), b"mq_resample:", b"is not served")
    refused(lib.mq_resample(fake, 1, 1000, fake, 12289, 1, 1, fake, None), b"mq_resample:", b"is not served")
    refused(lib.mq_resample(fake, 0, 1000, fake, 441, 160, 17, fake, None), b"mq_resample: channels=0")
    refused(lib.mq_resample(fake, 1, 0, fake, 441, 160, 17, fake, None), b"mq_resample: channels=1, len=0")
    for args in ((None, fake, fake), (fake, None, fake), (fake, fake, None)):
        refused(lib.mq_resample(args[0], 1, 1000, args[1], 441, 160, 17, args[2], None), b"mq_resample: null pointer")
    refused(lib.mq_resample(fake, 1, 1000, fake + 4, 441, 160, 17, fake, None), b"mq_resample:", b"8-byte aligned")
    assert L.MQ_RESAMPLE_MAX_TAPS == A.MAX_TAPS == 1 << 21

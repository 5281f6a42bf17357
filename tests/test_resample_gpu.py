"""The audio resampler on the GPU: mq_resample against the fp64 restatement of tests/resample_ref.py, and a 44.1 kHz waveform end to end through
AudioPreprocessor(resample=True).

BOUND.  The yardstick is torch's own float32 evaluation of the algorithm on the CPU (RR.resample_torch: the kernel built in float32, F.conv1d in
float32, as torchaudio runs it on a float32 waveform): its largest absolute error against the float64 reference over the inputs of a RATE PAIR (the
five edge lengths and the two-channel input, `yardstick`).  The kernel may err by at most 4 times that on any of them.  Per pair and not per
waveform, decided before the kernel ran: the shortest edge lengths of the pairs with o <= 3 have one to four output samples, and the largest of
so few rounding errors is no measure of an evaluation's precision (for one sample it is a single draw between 0 and half an ulp; it is 0 for
32000 -> 16000 at one sample).  All inputs of a pair have the same amplitude, so its longest input measures the float32 evaluation for all of
them.  Both numbers are printed on an AUDIO_RESAMPLE line, the per-waveform figure of the float32 evaluation next to them.  The kernel's table and sums are fp64, so its error is the
rounding of the stored float32: half an ulp, 3.0e-8 for 0.5 <= |y| < 1.  Measured on an MI355X
(float32 evaluation / kernel): 44100 -> 16000 7.4e-6 / 3.0e-8, 48000 1.7e-7 / 3.0e-8, 22050 2.09e-5 / 3.0e-8, 8000 1.7e-7 / 4.4e-8, 32000
2.2e-7 / 3.0e-8 (DESIGN.md §3 "LanguageBind front ends").

CONTROLS.  Three mistakes made on purpose in the float64 restatement; each must move it by at least 100 times the bound (AUDIO_RESAMPLE_CONTROL
lines)."""
import functools

import numpy as np
import pytest
import torch

from marqo_amd import _lib as L
from marqo_amd.engine import audio as A
from tests import audio_ref as AR
from tests import resample_ref as RR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MEAN, STD = -4.2677393, 4.5689974
TWO_CHANNEL = ((44100, 16000), (8000, 16000))


@functools.lru_cache(maxsize=None)
def case(pair, length, channels=None):
    """(waveform, float64 reference, float32 torch evaluation's max abs error): computed once, shared, never written to"""
    w = RR.make_wave(length, *pair, seed=length, channels=channels)
    ref = RR.resample_ref(w.numpy(), *pair)
    yard = float(np.abs(RR.resample_torch(w, *pair, dtype=torch.float32).numpy().astype(np.float64) - ref).max())
    return w, ref, yard


@functools.lru_cache(maxsize=None)
def yardstick(pair):
    two = [case(pair, int(0.2 * pair[0]) + 7, 2)[2]] if pair in TWO_CHANNEL else []
    return max([case(pair, length)[2] for length in RR.lengths(*pair)] + two)


def _resample(wave, pair):
    """mq_resample itself on a host waveform, with sentinel samples behind the output"""
    lib = L.load()
    o, n, width = A.resample_plan(*pair)
    taps = torch.from_numpy(A.resample_taps(*pair)).to(DEV)
    w = wave.to(DEV).contiguous()
    channels, length = (1, w.shape[0]) if w.ndim == 1 else w.shape
    m = A.resample_length(length, *pair)
    out = torch.full((channels * m + 64,), 7.0, dtype=torch.float32, device=DEV)
    L.check(lib.mq_resample(w.data_ptr(), channels, length, taps.data_ptr(), o, n, width, out.data_ptr(), torch.cuda.current_stream().cuda_stream),
            "mq_resample")
    torch.cuda.synchronize()
    assert bool((out[channels * m:] == 7.0).all())
    got = out[:channels * m].cpu()
    return got if wave.ndim == 1 else got.reshape(channels, m)


@pytest.mark.parametrize("pair", RR.PAIRS)
def test_resample_against_fp64(pair):
    for length in RR.lengths(*pair):
        w, ref, yard = case(pair, length)
        got = _resample(w, pair)
        err = float(np.abs(got.numpy().astype(np.float64) - ref).max())
        print(f"AUDIO_RESAMPLE {pair[0]}->{pair[1]} len={length} out={ref.shape[-1]} torch_fp32_err={yardstick(pair):.3e} (this waveform {yard:.3e}) "
              f"kernel_err={err:.3e} ratio={err / yardstick(pair):.3f}")
        assert tuple(got.shape) == ref.shape and bool(torch.isfinite(got).all())
        assert err <= 4 * yardstick(pair), (pair, length, err, yardstick(pair))
        assert torch.equal(A.resample(w, pair[0], pair[1], DEV).cpu(), got)                     # the public function is the same launch


@pytest.mark.parametrize("pair", TWO_CHANNEL)
def test_two_channels_are_resampled_each_on_its_own(pair):
    length = int(0.2 * pair[0]) + 7
    w, ref, yard = case(pair, length, 2)
    got = A.resample(w.numpy(), pair[0], pair[1], DEV)                                          # (an ndarray in)
    torch.cuda.synchronize()
    err = float(np.abs(got.cpu().numpy().astype(np.float64) - ref).max())
    print(f"AUDIO_RESAMPLE {pair[0]}->{pair[1]} len={length} channels=2 torch_fp32_err={yardstick(pair):.3e} (this waveform {yard:.3e}) kernel_err={err:.3e}")
    assert tuple(got.shape) == ref.shape == (2, A.resample_length(length, *pair)) and err <= 4 * yardstick(pair)
    assert torch.equal(got[1].cpu(), _resample(w[1].contiguous(), pair)) and torch.equal(got.cpu(), _resample(w, pair))


def test_equal_rates_are_the_waveform():
    w = AR.make_waveform(1000)
    assert torch.equal(A.resample(w, 16000, 16000, DEV).cpu(), w) and torch.equal(A.resample(w, 32000, 32000, DEV).cpu(), w)


@pytest.mark.parametrize("pair", RR.PAIRS)
def test_controls_are_visible(pair):
    """what a wrong port computes, in float64: the table with its phases in reverse order, `width` zeros on both sides (no `+ o` behind), the
    output left uncut.  Samples a variant does not produce count as missing (zero); samples it produces beyond the true length count in full."""
    o, n = RR.plan(*pair)[:2]
    length = (int(0.2 * pair[0]) // o) * o          # a whole number of input frames: the uncut output is one frame (n samples) too long

    def moved(variant, ref):
        m = max(variant.shape[0], ref.shape[0])
        pad = lambda y: np.concatenate([y, np.zeros(m - y.shape[0])])
        return float(np.abs(pad(variant) - pad(ref)).max())

    w, ref, yard = case(pair, length)
    controls = {"a dropped trailing cut": (RR.resample_ref(w.numpy(), *pair, cut=False), ref, yard)}
    assert controls["a dropped trailing cut"][0].shape[0] == ref.shape[0] + n
    if n > 1:        # (one phase has no order)
        controls["phase order reversed"] = (RR.resample_ref(w.numpy(), *pair, taps=RR.taps_ref(*pair)[::-1]), ref, yard)
    if o > 1:        # (at o == 1 the frame those zeros make room for is cut off anyway: the same output, no mistake)
        w2, ref2, yard2 = case(pair, length + (o + 1) // 2)             # a last input frame that is not whole: its outputs need the zeros behind
        controls["padding of width on both sides"] = (RR.resample_ref(w2.numpy(), *pair, pad_behind=RR.plan(*pair)[3]), ref2, yard2)
        assert controls["padding of width on both sides"][0].shape[0] < ref2.shape[0]
    for what, (variant, ref, yard) in controls.items():
        d, bound = moved(variant, ref), 4 * yard
        print(f"AUDIO_RESAMPLE_CONTROL {pair[0]}->{pair[1]} {what}: out={variant.shape[0]} (true {ref.shape[0]}) moved={d:.3e} bound={bound:.3e} "
              f"ratio={d / bound:.1e}")
        assert d >= 100 * bound, (pair, what, d, bound)


# ---- end to end ------------------------------------------------------------------------------------------------------------------------------------
def test_a_44100_hz_waveform_through_the_preprocessor():
    """resample, then the fbank and the fusion that were there: against the fp64 resample restatement followed by tests/audio_ref.py's fbank
    restatement, within the fbank test's bound carried to the picture — 4 times what the float32 fbank restatement loses on the same 16 kHz
    waveform, divided by the picture's 2 audio_std — and within the 1e-5 tests/test_audio_gpu.py::test_vectorise_audio_end_to_end asks of pictures"""
    bins, L_ = 16, 40
    pre = A.AudioPreprocessor(DEV, bins, L_, 16000, MEAN, STD, resample=True)
    pair = (44100, 16000)
    long_, short = RR.make_wave(44100, *pair, seed=1), RR.make_wave(6000, *pair, seed=2, channels=2)
    px = pre([(long_, 44100), (short.numpy(), 44100), (AR.make_waveform(16000, seed=3), 16000)])["pixel_values"]
    torch.cuda.synchronize()
    assert px.shape == (3, 3, bins, L_) and px.dtype == torch.float32 and px.device.type == "cuda"

    yards = []

    def picture(wave16k):
        ref = AR.fbank_ref(wave16k, bins)
        yards.append(float(np.abs(AR.fbank_torch(torch.from_numpy(wave16k), bins, torch.float32).numpy().astype(np.float64) - ref).max()))
        rows = torch.from_numpy(ref)
        return AR.fusion_ref(rows, L_, MEAN, STD, A.default_starts(rows.shape[0], L_))

    want = torch.stack([picture(RR.resample_ref(long_.numpy(), *pair)), picture(RR.resample_ref(short.numpy(), *pair)),
                        picture(AR.make_waveform(16000, seed=3).numpy().astype(np.float64))])
    err = (px.cpu().double() - want).abs().amax(dim=(1, 2, 3))
    for i, what in enumerate(("1 s mono at 44.1 kHz", "0.14 s stereo at 44.1 kHz", "1 s at 16 kHz")):
        bound = min(1e-5, 4 * yards[i] / (2 * STD))
        print(f"AUDIO_RESAMPLE_END_TO_END {what}: picture max abs error {float(err[i]):.2e}, bound {bound:.2e} (float32 fbank restatement loses {yards[i]:.2e})")
        assert float(err[i]) <= bound, (what, float(err[i]), bound)
    # without the opt-in the same call is refused, as it always was
    with pytest.raises(ValueError, match="no resampler"):
        A.AudioPreprocessor(DEV, bins, L_, 16000, MEAN, STD)((long_, 44100))

"""Restatement of torchaudio.functional.resample for the resampler tests (tests/test_resample_host.py, tests/test_resample_gpu.py).  A plain helper
module: nothing here calls the library.

torchaudio is not a dependency of this project, so the reference for mq_resample is written here from its published algorithm at its defaults
(resampling_method "sinc_interp_hann", lowpass_filter_width 6, rolloff 0.99).  Twice, as tests/audio_ref.py does for the fbank: `resample_ref` in
numpy float64, a plain loop-free gather and dot product per output sample — the yardstick —, and `resample_torch` in torch ops of a chosen dtype in
the order torchaudio evaluates them (kernel built in that dtype, zero padding, F.conv1d with stride o, transpose, cut).  float32 it is the measure of
what an fp32 evaluation loses, float64 it must agree with `resample_ref`.  Parity with torchaudio ITSELF is checked only where torchaudio is
installed (tests/test_resample_host.py::test_resample_ref_against_torchaudio)."""
import functools
import math

import numpy as np
import torch

WIDTH6, ROLLOFF = 6, 0.99
PAIRS = ((44100, 16000), (48000, 16000), (22050, 16000), (8000, 16000), (32000, 16000))


def plan(orig, new):
    """(o, n, base, width, K)"""
    g = math.gcd(orig, new)
    o, n = orig // g, new // g
    base = min(o, n) * ROLLOFF
    width = int(math.ceil(WIDTH6 * o / base))
    return o, n, base, width, 2 * width + o


def out_length(length, orig, new):
    o, n = plan(orig, new)[:2]
    return int(math.ceil(n * length / o))


@functools.lru_cache(maxsize=None)
def taps_ref(orig, new):
    """float64 [n, K] (computed once per pair; read-only): taps[p][k] = sinc(t) cos^2(pi t / 12) base / o at t = clamp((-p / n + (k - width) / o) base, -6, 6), entry by entry"""
    o, n, base, width, K = plan(orig, new)
    out = np.empty((n, K), dtype=np.float64)
    for p in range(n):
        for k in range(K):
            t = (-p / n + (k - width) / o) * base
            t = max(-float(WIDTH6), min(float(WIDTH6), t))
            win = math.cos(t * math.pi / WIDTH6 / 2) ** 2
            t *= math.pi
            out[p, k] = (1.0 if t == 0.0 else math.sin(t) / t) * win * (base / o)
    out.setflags(write=False)
    return out


def resample_ref(wave, orig, new, taps=None, pad_behind=None, cut=True):
    """wave [len] or [channels, len] (any float dtype) -> float64 of the same rank, ceil(n len / o) samples per channel.  `taps`, `pad_behind` and
    `cut` exist for the tests' controls: another table, another count of zeros behind the waveform, the output left uncut."""
    o, n, base, width, K = plan(orig, new)
    x = np.asarray(wave, dtype=np.float64)
    one_d = x.ndim == 1
    x = x[None, :] if one_d else x
    taps = taps_ref(orig, new) if taps is None else np.asarray(taps, dtype=np.float64)
    behind = width + o if pad_behind is None else pad_behind
    xp = np.concatenate([np.zeros((x.shape[0], width)), x, np.zeros((x.shape[0], behind))], axis=1)
    frames = (xp.shape[1] - K) // o + 1
    win = xp[:, np.arange(frames)[:, None] * o + np.arange(K)[None, :]]                 # [channels, frames, K]
    y = np.einsum("cfk,pk->cfp", win, taps).reshape(x.shape[0], frames * n)
    if cut:
        y = y[:, :out_length(x.shape[1], orig, new)]
    return np.ascontiguousarray(y[0] if one_d else y)


def resample_torch(wave, orig, new, dtype=torch.float32):
    """the same in torch ops of `dtype` on the CPU, in torchaudio's order"""
    o, n, base, width, K = plan(orig, new)
    x = torch.as_tensor(wave).detach().cpu().to(dtype)
    one_d = x.ndim == 1
    x = x[None, :] if one_d else x
    idx = torch.arange(-width, width + o, dtype=dtype)[None, None] / o
    t = torch.arange(0, -n, -1, dtype=dtype)[:, None, None] / n + idx
    t *= base
    t = t.clamp_(-WIDTH6, WIDTH6)
    window = torch.cos(t * math.pi / WIDTH6 / 2) ** 2
    t *= math.pi
    kernels = torch.where(t == 0, torch.tensor(1.0, dtype=dtype), t.sin() / t)
    kernels *= window * (base / o)
    length = x.shape[1]
    xp = torch.nn.functional.pad(x, (width, width + o))
    y = torch.nn.functional.conv1d(xp[:, None], kernels, stride=o)
    y = y.transpose(1, 2).reshape(x.shape[0], -1)[..., :out_length(length, orig, new)]
    return (y[0] if one_d else y).contiguous()


def make_wave(length, orig, new, seed=0, channels=None):
    """float32 [len] (or [channels, len]): seeded Gaussian noise of amplitude 0.2 plus a sine of amplitude 0.5 at 0.45 of the NEW rate (just under
    its Nyquist: in the filter's passband for a downsampling pair, and what aliases first if the phases are confused)"""
    g = np.random.default_rng(4000 + seed)
    shape = (length,) if channels is None else (channels, length)
    t = np.arange(length, dtype=np.float64) / orig
    x = 0.2 * g.standard_normal(shape) + 0.5 * np.sin(2 * np.pi * (0.45 * min(new, orig)) * t + g.uniform(0, 2 * np.pi))
    return torch.from_numpy(x.astype(np.float32))


def lengths(orig, new):
    """the edge lengths of a pair: fewer samples than o, exactly o, o + 1, a length whose output length the ceil decides (n len not a multiple of o),
    and about 0.2 s"""
    o, n = plan(orig, new)[:2]
    out = [max(1, o - 1), o, o + 1, 3 * o + 1 if o > 1 else 3, int(0.2 * orig) + 7]
    return sorted(set(out))

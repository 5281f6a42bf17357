"""The LanguageBind audio front end on the GPU: waveforms -> the `pixel_values` [b, 3, num_mel_bins, target_length] its audio tower takes
(reference: s2_inference/languagebind/audio/processing_audio.py, AudioTransform).

    [mq_resample (opt-in: a waveform at another rate -> 16 kHz, torchaudio.functional.resample at its defaults as a polyphase filter) ->]
    mq_fbank (whole-tensor mean, Kaldi fbank as torchaudio.compliance.kaldi.fbank computes it for the reference's arguments -> log-mel rows [m, bins])
    -> mq_mel_fusion (three crops of a long clip, or the clip repeated to length; transposed to [bins, L]; (x - audio_mean) / (2 audio_std))

Both run on the current stream of the calling thread; a call allocates the rows, the picture and 2 KB of scratch through PyTorch's allocator.

RESAMPLING (`resample`, `resample_taps`, `AudioPreprocessor(..., resample=True)`).  With o = orig / gcd, n = new / gcd, base = 0.99 min(o, n)
and width = ceil(6 o / base), phase p of the filter has the 2 width + o taps sinc(t) cos^2(pi t / 12) base / o at
t = clamp((-p / n + k / o) base, -6, 6), k = -width .. width + o - 1; the waveform gets `width` zeros in front and `width + o` behind, output
f n + p is the dot product of phase p with the samples from f o on, and the output is cut to ceil(n len / o) samples.  The table is built once per
rate pair in fp64 on the host, cached, and kept on the device in fp64.  A pair whose table would have more than MAX_TAPS entries (rates that share
too small a divisor: 44101 Hz against 16000 would need 706 million) is refused.

What is NOT here, and what differs from the reference:
  * decoding: a waveform is a float tensor or ndarray.  Paths, URLs and bytes are refused (nothing in this engine decodes media, exactly as for
    video);
  * resampling WITHOUT the opt-in: an AudioPreprocessor built without `resample=True` refuses a (waveform, rate) pair at any rate but the
    checkpoint's `audio_sample_rate` (16000), as it always has (the reference resamples whatever it is given);
  * the RANDOM crop of a long clip.  For m > target_length rows the reference splits range(0, m - L + 1) into thirds (np.array_split) and draws ONE
    RANDOM start from each (np.random.choice; `[0]` for an empty third): the same file gives a different picture at every call.  This front end takes
    the MIDDLE element of each third, r[(len(r) - 1) // 2], and accepts explicit `starts` so that a caller can reproduce any draw.  (The
    reference's video processor has the same kind of randomness, a random horizontal flip: s2_inference/multimodal_model_load.py.)  Marqo chunks
    audio into `audio_chunk_length` = 10 s pieces, 998 rows against the released checkpoint's 1036: there the clip is repeated to length and no
    crop is drawn at all.
"""
from __future__ import annotations

import math
import threading
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from marqo_amd import _lib as L

Tensor = torch.Tensor
FRAME, SHIFT, MAX_BINS, SERVED_RATE = 400, 160, 128, 16000     # mq_fbank
LOWPASS_WIDTH, ROLLOFF = 6, 0.99                               # torchaudio.functional.resample's defaults
MAX_TAPS, MAX_TAP_ROW = L.MQ_RESAMPLE_MAX_TAPS, 12288          # mq_resample: entries of the table, and of one phase


def num_frames(n: int) -> int:
    """rows Kaldi's snip_edges framing cuts from n samples"""
    return 0 if n < FRAME else 1 + (n - FRAME) // SHIFT


def default_starts(m: int, L_: int) -> Tuple[int, int, int]:
    """the three crop starts for m rows and a picture of L_ frames: (0, 0, 0) when nothing is cropped (m <= L_), else the middle element of each
    third of range(0, m - L_ + 1) as np.array_split cuts it (the first `total % 3` thirds are one longer), 0 for an empty third"""
    if m <= L_:
        return (0, 0, 0)
    total = m - L_ + 1
    out, lo = [], 0
    for k in range(3):
        size = total // 3 + (1 if k < total % 3 else 0)
        out.append(lo + (size - 1) // 2 if size else 0)
        lo += size
    return tuple(out)


# ---- resampling -------------------------------------------------------------------------------------------------------------------------------
def resample_plan(orig_freq: int, new_freq: int) -> Tuple[int, int, int]:
    """(o, n, width) of a rate pair: the reduced rates and the filter's half width in input samples; refuses a pair whose table is over the cap"""
    if isinstance(orig_freq, bool) or isinstance(new_freq, bool) or not isinstance(orig_freq, (int, np.integer)) or \
            not isinstance(new_freq, (int, np.integer)) or orig_freq < 1 or new_freq < 1:
        raise ValueError(f"sample rates are positive integers (orig_freq = {orig_freq!r}, new_freq = {new_freq!r})")
    g = math.gcd(int(orig_freq), int(new_freq))
    o, n = int(orig_freq) // g, int(new_freq) // g
    width = int(math.ceil(LOWPASS_WIDTH * o / (min(o, n) * ROLLOFF)))
    taps = n * (2 * width + o)
    if taps > MAX_TAPS or 2 * width + o > MAX_TAP_ROW:
        raise ValueError(f"resampling {orig_freq} Hz to {new_freq} Hz is not served: the two rates reduce to {o} / {n} only (greatest common divisor "
                         f"{g}), and the polyphase table of {n} phases x {2 * width + o} taps = {taps} entries is over the cap of {MAX_TAPS} entries "
                         f"({MAX_TAP_ROW} per phase); resample to a rate that shares a larger divisor with {new_freq} first")
    return o, n, width


def resample_length(length: int, orig_freq: int, new_freq: int) -> int:
    """samples torchaudio.functional.resample returns for `length`: ceil(new_freq length / orig_freq)"""
    g = math.gcd(int(orig_freq), int(new_freq))
    o, n = int(orig_freq) // g, int(new_freq) // g
    return -((-n * int(length)) // o)


def resample_taps(orig_freq: int, new_freq: int) -> np.ndarray:
    """float64 [n, 2 width + o]: the polyphase table of torchaudio's sinc_interp_hann kernel for a rate pair"""
    o, n, width = resample_plan(orig_freq, new_freq)
    base = min(o, n) * ROLLOFF
    idx = np.arange(-width, width + o, dtype=np.float64)[None, :] / o
    t = np.clip((np.arange(0, -n, -1, dtype=np.float64)[:, None] / n + idx) * base, -LOWPASS_WIDTH, LOWPASS_WIDTH)
    window = np.cos(t * math.pi / LOWPASS_WIDTH / 2) ** 2
    t = t * math.pi
    sinc = np.where(t == 0.0, 1.0, np.sin(t) / np.where(t == 0.0, 1.0, t))
    return np.ascontiguousarray(sinc * window * (base / o))


_tap_cache: Dict[Tuple[int, int, str], Tuple[Tensor, int, int, int]] = {}
_tap_lock = threading.Lock()


def _device_taps(orig_freq: int, new_freq: int, device: str) -> Tuple[Tensor, int, int, int]:
    """(table on the device, o, n, width), built once per (reduced rate pair, device)"""
    o, n, width = resample_plan(orig_freq, new_freq)
    key = (o, n, str(device))
    with _tap_lock:
        hit = _tap_cache.get(key)
        if hit is None:
            hit = _tap_cache[key] = (torch.from_numpy(resample_taps(o, n)).to(device), o, n, width)
    return hit


def resample(waveform, orig_freq: int, new_freq: int, device: str) -> Tensor:
    """torchaudio.functional.resample(waveform, orig_freq, new_freq) at its defaults on the GPU: a float tensor / ndarray [len] or [channels, len]
    (host or device) -> fp32 of the same rank on the device, ceil(new_freq len / orig_freq) samples per channel; every channel is resampled on its
    own.  Equal rates: the waveform itself, as fp32 on the device."""
    if isinstance(waveform, np.ndarray):
        waveform = torch.from_numpy(np.ascontiguousarray(waveform))
    if not isinstance(waveform, torch.Tensor) or not waveform.is_floating_point() or waveform.ndim not in (1, 2) or waveform.numel() < 1:
        got = f"{waveform.dtype} {tuple(waveform.shape)}" if isinstance(waveform, torch.Tensor) else type(waveform).__name__
        raise ValueError(f"a waveform to resample is a non-empty float tensor or ndarray [len] or [channels, len], got {got}")
    o, n, width = resample_plan(orig_freq, new_freq)
    with torch.cuda.device(device):
        w = waveform.detach().to(device=device, dtype=torch.float32, non_blocking=True).contiguous()
        if o == n:
            return w
        taps = _device_taps(orig_freq, new_freq, device)[0]
        channels, length = (1, w.shape[0]) if w.ndim == 1 else w.shape
        out = torch.empty(*w.shape[:-1], resample_length(length, o, n), dtype=torch.float32, device=device)
        s = torch.cuda.current_stream(device).cuda_stream
        L.check(L.load().mq_resample(w.data_ptr(), channels, length, taps.data_ptr(), o, n, width, out.data_ptr(), s), "mq_resample")
    return out


class AudioPreprocessor:
    """`__call__(waveforms, starts=None)` -> {"pixel_values": fp32 [b, 3, bins, L] on the device}.  A waveform is a 1-D float tensor / ndarray, a
    [channels, n] one (the mean of the whole tensor is subtracted, then channel 0 is framed: the reference plus Kaldi), or a (waveform, sample_rate)
    pair; `waveforms` is one of these or a list of them.  `starts`: None, one triple of row indices (for every item), or a list with a triple or
    None per item.  `resample=True`: a pair at another rate than the model's is resampled to it first (every channel), as the reference does;
    without it such a pair is refused."""

    def __init__(self, device: str, num_mel_bins: int, target_length: int, sample_rate: int = SERVED_RATE, mean: float = 0.5, std: float = 0.5,
                 resample: bool = False):
        if sample_rate != SERVED_RATE:
            raise ValueError(f"the audio front end serves {SERVED_RATE} Hz only (25 ms frames of {FRAME} samples every {SHIFT}); "
                             f"the checkpoint's audio_sample_rate is {sample_rate}")
        if not 1 <= num_mel_bins <= MAX_BINS or target_length < 1 or not std > 0:
            raise ValueError(f"the audio front end takes 1 to {MAX_BINS} mel bins, a positive target_length and a positive audio_std "
                             f"(num_mel_bins = {num_mel_bins}, target_length = {target_length}, audio_std = {std})")
        self.device, self.bins, self.length, self.sample_rate, self.mean, self.std = device, num_mel_bins, target_length, sample_rate, float(mean), float(std)
        self.resample = bool(resample)

    # ---- host side: what is accepted ---------------------------------------------------------------------------------------------------------
    def _waveform(self, item) -> Tuple[Tensor, int]:
        """one item -> (a host or device float tensor [n] or [channels, n], its rate), checked; nothing is moved yet"""
        rate = self.sample_rate
        if isinstance(item, tuple) and len(item) == 2 and isinstance(item[1], (int, np.integer)) and not isinstance(item[1], bool):
            item, rate = item[0], int(item[1])
            if rate != self.sample_rate and self.resample:
                resample_plan(rate, self.sample_rate)         # (refuses a pair over the table cap before anything reaches a device)
            elif rate != self.sample_rate:
                raise ValueError(f"the waveform's sample rate is {int(rate)} Hz, the model's is {self.sample_rate} Hz: resample it first "
                                 f"(there is no resampler in this engine)")
        if isinstance(item, (str, bytes, bytearray)):
            what = "bytes" if not isinstance(item, str) else repr(item if len(item) <= 80 else item[:77] + "...")
            raise ValueError(f"Unsupported audio content type: {type(item)}: {what} — nothing in this engine decodes media; pass the waveform "
                             f"(float samples at {self.sample_rate} Hz)")
        if isinstance(item, np.ndarray):
            item = torch.from_numpy(np.ascontiguousarray(item))
        if not isinstance(item, torch.Tensor) or not item.is_floating_point() or item.ndim not in (1, 2):
            got = f"{item.dtype} {tuple(item.shape)}" if isinstance(item, torch.Tensor) else type(item).__name__
            raise ValueError(f"Unsupported audio content type: a waveform is a float tensor or ndarray [n] or [channels, n], got {got}")
        n = item.shape[-1] if rate == self.sample_rate else resample_length(item.shape[-1], rate, self.sample_rate)
        if n < FRAME or item.shape[0] < 1:
            raise ValueError(f"a waveform of {n} samples{'' if rate == self.sample_rate else f' ({item.shape[-1]} at {rate} Hz)'} is shorter than "
                             f"one {FRAME}-sample frame (25 ms at {self.sample_rate} Hz): it has no log-mel row")
        return item, rate

    def _starts(self, starts, count: int, frames: Sequence[int]) -> List[Tuple[int, int, int]]:
        is_triple = lambda s: isinstance(s, (tuple, list, np.ndarray)) and len(s) == 3 and all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in s)
        if starts is None:
            per_item = [None] * count
        elif is_triple(starts):
            per_item = [starts] * count
        elif isinstance(starts, (list, tuple)) and len(starts) == count and all(s is None or is_triple(s) for s in starts):
            per_item = list(starts)
        else:
            raise ValueError(f"`starts` is None, three row indices, or a list with three row indices (or None) per waveform ({count} here), got {starts!r}")
        out = []
        for s, m in zip(per_item, frames):
            if s is None:
                s = default_starts(m, self.length)
            s = tuple(int(v) for v in s)
            last = max(0, m - self.length)
            if any(v < 0 or v > last for v in s):
                raise ValueError(f"crop starts {s} are outside [0, {last}] ({m} log-mel rows, target_length {self.length}"
                                 f"{': a clip this short is repeated to length, not cropped' if m <= self.length else ''})")
            out.append(s)
        return out

    # ---- the call -------------------------------------------------------------------------------------------------------------------------------
    def __call__(self, waveforms, starts=None):
        items = list(waveforms) if isinstance(waveforms, list) else [waveforms]
        if not items:
            raise ValueError("Unsupported audio content type: an empty list of waveforms")
        checked = [self._waveform(it) for it in items]
        waves = [w if r == self.sample_rate else resample(w, r, self.sample_rate, self.device) for w, r in checked]
        frames = [num_frames(w.shape[-1]) for w in waves]
        crops = self._starts(starts, len(waves), frames)
        lib, dev = L.load(), self.device
        with torch.cuda.device(dev):
            s = torch.cuda.current_stream(dev).cuda_stream
            out = torch.empty(len(waves), 3, self.bins, self.length, dtype=torch.float32, device=dev)
            ws = torch.empty(L.MQ_FBANK_WS_BYTES, dtype=torch.uint8, device=dev)
            for i, (w, m, c) in enumerate(zip(waves, frames, crops)):
                w = w.detach().to(device=dev, dtype=torch.float32, non_blocking=True).contiguous()
                mel = torch.empty(m, self.bins, dtype=torch.float32, device=dev)
                L.check(lib.mq_fbank(w.data_ptr(), w.shape[-1], w.numel(), self.sample_rate, self.bins, mel.data_ptr(), ws.data_ptr(), s), "mq_fbank")
                L.check(lib.mq_mel_fusion(mel.data_ptr(), m, self.bins, c[0], c[1], c[2], self.mean, self.std, out[i].data_ptr(), self.length, s),
                        "mq_mel_fusion")
        return {"pixel_values": out}

"""The LanguageBind audio front end on the GPU: 16 kHz waveforms -> the `pixel_values` [b, 3, num_mel_bins, target_length] its audio tower takes
(reference: s2_inference/languagebind/audio/processing_audio.py, AudioTransform).

    mq_fbank (whole-tensor mean, Kaldi fbank as torchaudio.compliance.kaldi.fbank computes it for the reference's arguments -> log-mel rows [m, bins])
    -> mq_mel_fusion (three crops of a long clip, or the clip repeated to length; transposed to [bins, L]; (x - audio_mean) / (2 audio_std))

Both run on the current stream of the calling thread; a call allocates the rows, the picture and 2 KB of scratch through PyTorch's allocator.

What is NOT here, and what differs from the reference:
  * decoding and resampling: a waveform is a float tensor or ndarray at the checkpoint's `audio_sample_rate` (16000).  Paths, URLs and bytes are
    refused (nothing in this engine decodes media, exactly as for video), and so is any other rate (the reference resamples; there is no resampler
    here);
  * the RANDOM crop of a long clip.  For m > target_length rows the reference splits range(0, m - L + 1) into thirds (np.array_split) and draws ONE
    RANDOM start from each (np.random.choice; `[0]` for an empty third): the same file gives a different picture at every call.  This front end takes
    the MIDDLE element of each third, r[(len(r) - 1) // 2], and accepts explicit `starts` so that a caller can reproduce any draw.  (The
    reference's video processor has the same kind of randomness, a random horizontal flip: s2_inference/multimodal_model_load.py.)  Marqo chunks
    audio into `audio_chunk_length` = 10 s pieces, 998 rows against the released checkpoint's 1036: there the clip is repeated to length and no
    crop is drawn at all.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from marqo_amd import _lib as L

Tensor = torch.Tensor
FRAME, SHIFT, MAX_BINS, SERVED_RATE = 400, 160, 128, 16000     # mq_fbank


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


class AudioPreprocessor:
    """`__call__(waveforms, starts=None)` -> {"pixel_values": fp32 [b, 3, bins, L] on the device}.  A waveform is a 1-D float tensor / ndarray, a
    [channels, n] one (the mean of the whole tensor is subtracted, then channel 0 is framed: the reference plus Kaldi), or a (waveform, sample_rate)
    pair; `waveforms` is one of these or a list of them.  `starts`: None, one triple of row indices (for every item), or a list with a triple or
    None per item."""

    def __init__(self, device: str, num_mel_bins: int, target_length: int, sample_rate: int = SERVED_RATE, mean: float = 0.5, std: float = 0.5):
        if sample_rate != SERVED_RATE:
            raise ValueError(f"the audio front end serves {SERVED_RATE} Hz only (25 ms frames of {FRAME} samples every {SHIFT}); "
                             f"the checkpoint's audio_sample_rate is {sample_rate}")
        if not 1 <= num_mel_bins <= MAX_BINS or target_length < 1 or not std > 0:
            raise ValueError(f"the audio front end takes 1 to {MAX_BINS} mel bins, a positive target_length and a positive audio_std "
                             f"(num_mel_bins = {num_mel_bins}, target_length = {target_length}, audio_std = {std})")
        self.device, self.bins, self.length, self.sample_rate, self.mean, self.std = device, num_mel_bins, target_length, sample_rate, float(mean), float(std)

    # ---- host side: what is accepted ---------------------------------------------------------------------------------------------------------
    def _waveform(self, item) -> Tensor:
        """one item -> a host or device float tensor [n] or [channels, n], checked; nothing is moved yet"""
        if isinstance(item, tuple) and len(item) == 2 and isinstance(item[1], (int, np.integer)) and not isinstance(item[1], bool):
            item, rate = item
            if int(rate) != self.sample_rate:
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
        if item.shape[-1] < FRAME or item.shape[0] < 1:
            raise ValueError(f"a waveform of {item.shape[-1]} samples is shorter than one {FRAME}-sample frame (25 ms at {self.sample_rate} Hz): "
                             f"it has no log-mel row")
        return item

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
        waves = [self._waveform(it) for it in items]
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

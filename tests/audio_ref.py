"""Restatements, synthetic weights and inputs for the LanguageBind audio tests (tests/test_audio_host.py, tests/test_audio_gpu.py).  A plain helper
module: nothing here calls the library.

FBANK.  torchaudio is not a dependency of this project, so the reference for mq_fbank is written here from the algorithm of
torchaudio.compliance.kaldi.fbank for the arguments the reference passes (sample_frequency 16000, frame_length 25, frame_shift 10, window_type
"hanning", dither 0, use_energy False, htk_compat True, every other argument at its default: snip_edges, remove_dc_offset, preemphasis 0.97,
round_to_power_of_two, low_freq 20, high_freq 0, use_power, use_log_fbank, vtln_warp 1), with the reference's `audio_data -= audio_data.mean()` in
front (languagebind/audio/processing_audio.py:96-110).  Twice: `fbank_ref` in numpy float64 with np.fft.rfft, and `fbank_torch` in torch ops of a
chosen dtype in the order torchaudio evaluates them (the filter matrix in that dtype too, dense, with the zero Nyquist column) — float32 it is the
yardstick of the kernel's error, float64 it must agree with `fbank_ref`.  Parity with torchaudio ITSELF is checked only where torchaudio is installed
(tests/test_audio_host.py::test_fbank_ref_against_torchaudio).

FUSION.  `fusion_ref` is the picture the reference's AudioTransform.waveform2melspec builds from the log-mel rows, with the three crop starts passed
in where the reference draws them at random.

TOWER.  The audio part is a CLIP ViT over a picture that is not square: tests/languagebind_ref.py's `vision_forward` runs it as it stands (its patch
conv and position add do not assume a square grid); what differs is the config and the length of the position embedding."""
import math
import os

import numpy as np
import torch

from tests import languagebind_ref as LBR

AUDIO_PART = "LanguageBind_Audio_FT"
RATE, FRAME, SHIFT, NFFT = 16000, 400, 160, 512
EPS32 = float(np.finfo(np.float32).eps)

# the synthetic audio part: vision (W, heads, layers, P) over a num_mel_bins x target_length picture; text side and projection as LBR.SMALL
SMALL = dict(LBR.SMALL, P=8, bins=16, L=40)


def mel(f):
    return 1127.0 * np.log(1.0 + np.asarray(f, dtype=np.float64) / 700.0)


def num_frames(n):
    return 1 + (n - FRAME) // SHIFT


# ---- fbank, numpy float64 -------------------------------------------------------------------------------------------------------------------------
def mel_banks_ref(bins):
    """float64 [bins, 256]: triangles linear in mel between 20 Hz and 8 kHz; column k is the FFT bin at k * 31.25 Hz"""
    lo, hi = mel(20.0), mel(RATE / 2)
    delta = (hi - lo) / (bins + 1)
    left = lo + np.arange(bins, dtype=np.float64)[:, None] * delta
    m = mel(np.arange(NFFT // 2, dtype=np.float64) * (RATE / NFFT))[None, :]
    up, down = (m - left) / delta, (left + 2 * delta - m) / delta
    return np.maximum(0.0, np.minimum(up, down))


def fbank_ref(wave, bins):
    """wave [n] or [channels, n] (any float dtype) -> float64 [m, bins]"""
    x = np.asarray(wave, dtype=np.float64)
    x = x - x.mean()
    if x.ndim == 2:
        x = x[0]
    m = num_frames(x.shape[0])
    assert m >= 1
    fr = x[np.arange(m)[:, None] * SHIFT + np.arange(FRAME)[None, :]]
    fr = fr - fr.mean(axis=1, keepdims=True)
    fr = fr - 0.97 * np.concatenate([fr[:, :1], fr[:, :-1]], axis=1)
    fr = fr * (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(FRAME) / (FRAME - 1)))[None, :]
    power = np.abs(np.fft.rfft(fr, n=NFFT, axis=1)[:, :NFFT // 2]) ** 2
    return np.log(np.maximum(power @ mel_banks_ref(bins).T, EPS32))


# ---- fbank, torch ops of one dtype in torchaudio's order -----------------------------------------------------------------------------------------
def fbank_torch(wave, bins, dtype=torch.float32):
    """wave tensor [n] or [channels, n] -> `dtype` [m, bins], every step evaluated in `dtype` on the CPU"""
    x = torch.as_tensor(wave).detach().cpu().to(dtype).clone()
    x -= x.mean()
    if x.ndim == 2:
        x = x[0]
    m = num_frames(x.shape[0])
    fr = x.as_strided((m, FRAME), (SHIFT, 1))
    fr = fr - fr.mean(dim=1, keepdim=True)
    shifted = torch.nn.functional.pad(fr.unsqueeze(0), (1, 0), mode="replicate").squeeze(0)
    fr = fr - 0.97 * shifted[:, :-1]
    fr = fr * torch.hann_window(FRAME, periodic=False, dtype=dtype).unsqueeze(0)
    fr = torch.nn.functional.pad(fr, (0, NFFT - FRAME))
    spectrum = torch.fft.rfft(fr).abs().pow(2.0)
    # the filter matrix: scalar ends in Python floats, everything per bin in `dtype`
    lo, hi = 1127.0 * math.log(1.0 + 20.0 / 700.0), 1127.0 * math.log(1.0 + (RATE / 2) / 700.0)
    delta = (hi - lo) / (bins + 1)
    b = torch.arange(bins, dtype=dtype).unsqueeze(1)
    left, center, right = lo + b * delta, lo + (b + 1.0) * delta, lo + (b + 2.0) * delta
    mk = (1127.0 * (1.0 + (RATE / NFFT) * torch.arange(NFFT // 2, dtype=dtype) / 700.0).log()).unsqueeze(0)
    banks = torch.max(torch.zeros(1, dtype=dtype), torch.min((mk - left) / (center - left), (right - mk) / (right - center)))
    banks = torch.nn.functional.pad(banks, (0, 1))
    return torch.max(torch.mm(spectrum, banks.T), torch.tensor(EPS32, dtype=dtype)).log()


# ---- the three-crop picture ------------------------------------------------------------------------------------------------------------------------
def fusion_ref(mel_rows, L, mean, std, starts=(0, 0, 0)):
    """mel_rows tensor [m, bins] -> [3, bins, L] in its dtype.  More rows than L: the three crops of L rows at `starts`; fewer: the rows tiled
    int(L / m) + 1 times and cut to L, three times over; exactly L: the rows three times over.  Then frames last, then (x - mean) / (std * 2)."""
    m = mel_rows.shape[0]
    if m > L:
        assert all(0 <= s and s + L <= m for s in starts), (starts, m, L)
        fused = torch.stack([mel_rows[s:s + L, :] for s in starts], dim=0)
    else:
        assert tuple(starts) == (0, 0, 0)
        rows = mel_rows.repeat(int(L / m) + 1, 1)[:L, :] if m < L else mel_rows
        fused = torch.stack([rows, rows, rows], dim=0)
    return (fused.transpose(1, 2) - mean) / (std * 2)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------------------
def make_waveform(n, seed=0, channels=None):
    """float32 [n] (or [channels, n]): three tones at seeded frequencies, amplitudes and phases, Gaussian noise of amplitude 0.1, DC offset 0.05"""
    g = np.random.default_rng(1000 + seed)
    t = np.arange(n, dtype=np.float64) / RATE
    shape = (n,) if channels is None else (channels, n)
    x = 0.05 + 0.1 * g.standard_normal(shape)
    for _ in range(3):
        f, a, ph = g.uniform(80.0, 6000.0), g.uniform(0.05, 0.15), g.uniform(0.0, 2 * np.pi)
        x = x + a * np.sin(2 * np.pi * f * t + ph)
    return torch.from_numpy(x.astype(np.float32))


# ---- the audio part: config, weights, directory, forward -------------------------------------------------------------------------------------------
def config(shape=SMALL, mean=-4.2677393, std=4.5689974, rate=RATE, **vision):
    """the `config.json` of an audio part, as a dict (the released checkpoint's audio_mean / audio_std by default)"""
    cfg = LBR.config(shape, add_time_attn=False)
    cfg["model_type"] = "LanguageBindAudio"
    cfg["vision_config"].update({"num_mel_bins": shape["bins"], "target_length": shape["L"], "audio_sample_rate": rate, "audio_mean": mean,
                                 "audio_std": std, "image_size": 224}, **vision)
    return cfg


def tokens(cfg):
    v = cfg["vision_config"]
    return (v["num_mel_bins"] // v["patch_size"]) * (v["target_length"] // v["patch_size"]) + 1


def synthetic_state_dict(cfg, seed=0):
    """LBR.synthetic_state_dict with the position embedding at the rectangular grid's length (what a saved audio checkpoint holds)"""
    sd = LBR.synthetic_state_dict(dict(cfg, vision_config=dict(cfg["vision_config"], image_size=cfg["vision_config"]["patch_size"])), seed=seed)
    g = torch.Generator().manual_seed(7000 + seed)
    sd["vision_model.embeddings.position_embedding.weight"] = torch.randn(tokens(cfg), cfg["vision_config"]["hidden_size"], generator=g) * 0.5
    return sd


def write_part(directory, cfg, sd):
    LBR.write_part(directory, cfg, sd)


def write_model(root, image=True, seed=0, shape=SMALL):
    """`localpath` of an `Audio_FT[_Image]`-shaped model: the audio part's directory and, with `image`, the image part's -> {part: (cfg, sd)}"""
    out = {"audio": (config(shape), None)}
    if image:
        out["image"] = (LBR.config(LBR.SMALL, add_time_attn=False), None)
    for k, kind in enumerate(list(out)):
        cfg = out[kind][0]
        sd = synthetic_state_dict(cfg, seed=seed) if kind == "audio" else LBR.synthetic_state_dict(cfg, seed=seed + 17 * k)
        write_part(os.path.join(str(root), AUDIO_PART if kind == "audio" else LBR.IMAGE_PART), cfg, sd)
        out[kind] = (cfg, sd)
    return out


def audio_forward(sd, cfg, pixel_values, dtype=torch.float32):
    """pixel_values [b, 3, bins, L] -> pooled, projected [b, D] (not normalised)"""
    return LBR.vision_forward(sd, cfg, pixel_values, T=1, dtype=dtype)


def make_spectrograms(b, bins, L, seed=0):
    """fp32 [b, 3, bins, L] in the range of a normalised picture, with structure along both axes (rows and columns are not exchangeable)"""
    g = torch.Generator().manual_seed(900 + seed)
    f, t = torch.linspace(-1.0, 1.0, bins).reshape(1, 1, bins, 1), torch.linspace(0.0, 6.0, L).reshape(1, 1, 1, L)
    return (0.5 * torch.randn(b, 3, bins, L, generator=g) + 0.6 * f * torch.randn(b, 3, 1, 1, generator=g) + 0.5 * torch.sin(t * (1.0 + f))).contiguous()

"""LanguageBind video / audio / image / text embeddings: the model family behind the reference's `languagebind` loader (s2_inference/languagebind/,
s2_inference/multimodal_model_load.py).

LanguageBind_Video_V1.5_FT is a CLIP ViT-L/14 over the T = 8 frames of a clip with a temporal sub-block in front of every layer
(languagebind/video/modeling_video.py:209-231), the mean of the T class rows as pooled output (:768-771) and a CLIP text tower.  The reference
regroups the whole activation `(b t) n d <-> (b n) t d` four times per layer; here the rows stay in the spatial blocks' frame-major order
r = (b T + t) N + n from the first layer to the last, and the temporal attention reads its T rows at their stride:

    mq_patchify_clip (reads `b c t h w` directly) -> mq_gemm_bf16 (conv as GEMM) -> mq_vit_assemble (class token + positions + pre_layrnorm)
    per layer:  mq_temporal_embed_ln (x += temporal_embedding[t] in the fp32 stream, temporal_layer_norm1 -> bf16)
                -> mq_gemm_bf16 (temporal q | k | v + bias) -> mq_temporal_attention (across the T frames of every token and head)
                -> mq_gemm_bf16 (temporal out_proj + bias + residual, in place on the stream)
                -> mq_encoder_forward on this one block (layer_norm1, self_attn, layer_norm2, mlp)
    head:       mq_cls_rows -> mq_layernorm (post_layernorm of the B T class rows) -> mq_gemm_bf16 (visual_projection) -> mq_avg_tokens (mean over
                the T frames of a clip; the projection is linear, so it commutes with the reference's mean-then-project) -> mq_l2_normalize

Everything of a call runs on one stream; the scratch of the per-layer path is allocated once per call, in front of the first layer.  The residual
stream is fp32 (the temporal embedding is added into it with one fp32 add, as the reference keeps the sum in its stream).  bf16 operands only.

The audio part (`LanguageBind_Audio_FT`, languagebind/audio/modeling_audio.py:767-811) is the same CLIP ViT over ONE picture that is not
square: image_size = [num_mel_bins, target_length], 112 x 1036 at patch 14 for the released checkpoint, an 8 x 74 grid of 593 tokens, one frame,
no temporal attention.  Its positions are already in the checkpoint at that length (the reference resizes them at construction, before the
weights load), so nothing is interpolated here:

    mq_patchify_rect (fp32 [b, 3, bins, L] -> im2col rows in (py, px) order) -> mq_gemm_bf16 -> mq_vit_assemble -> mq_encoder_forward (all blocks)
    -> mq_cls_rows -> mq_layernorm (post_layernorm) -> mq_gemm_bf16 (visual_projection) -> mq_l2_normalize

The picture comes from engine/audio.py (an opt-in resampler, Kaldi fbank and the three-crop fusion on the GPU) or from the caller's own
preprocessing; a clip's `pixel_values` come from engine/video.py (decoded uint8 frames: frame pick, normalisation, short-side scale, centre crop on
the GPU) or from the caller's.

The image part (`LanguageBind_Image`, no temporal attention) is a plain CLIP ViT under Hugging Face names and runs on `towers.VitTower`; the
text tower is `towers.ClipTextTower` on 77 positions, packed up to the EOT as everywhere in this engine.
"""
from __future__ import annotations

import os
from typing import Dict, Optional

import numpy as np
import torch

from marqo_amd import _lib as L
from marqo_amd.engine import archs, checkpoint
from marqo_amd.engine.archs import LanguageBindArch
from marqo_amd.engine.hf_clip import clip_state_dict, clip_text_state_dict, load_tokenizer
from marqo_amd.engine.tokenizers import ClipBpeTokenizer
from marqo_amd.engine.towers import ClipTextTower, VitTower, _check_precision, _need, request_stream
from marqo_amd.engine.vit_tokens import VitTokenTower

Tensor = torch.Tensor
MAX_FRAMES = 16        # mq_temporal_attention

# the reference's part tables (multimodal_model_load.py:71-100), in its dict order: the LAST part's text tower is the model's
# (languagebind/__init__.py:41-49)
MODEL_PARTS = {
    "LanguageBind/Video_V1.5_FT_Audio_FT_Image": {"video": "LanguageBind_Video_V1.5_FT", "audio": "LanguageBind_Audio_FT", "image": "LanguageBind_Image"},
    "LanguageBind/Video_V1.5_FT_Audio_FT": {"video": "LanguageBind_Video_V1.5_FT", "audio": "LanguageBind_Audio_FT"},
    "LanguageBind/Video_V1.5_FT_Image": {"video": "LanguageBind_Video_V1.5_FT", "image": "LanguageBind_Image"},
    "LanguageBind/Audio_FT_Image": {"audio": "LanguageBind_Audio_FT", "image": "LanguageBind_Image"},
    "LanguageBind/Audio_FT": {"audio": "LanguageBind_Audio_FT"},
    "LanguageBind/Video_V1.5_FT": {"video": "LanguageBind_Video_V1.5_FT"},
}


def vision_state_dict(sd: Dict[str, Tensor], arch: LanguageBindArch) -> Dict[str, Tensor]:
    """the vision side of a part under the reference's Hugging Face names (`vision_model.embeddings.*`, `vision_model.pre_layrnorm` — its
    spelling —, `vision_model.encoder.layers.N.*`, `vision_model.post_layernorm`, `visual_projection.weight`) -> open_clip's `visual.*` names as
    VitTower loads them"""
    v, W = "vision_model.", arch.width
    out = {"visual." + k: t for k, t in clip_state_dict(sd, v, arch.layers).items()}
    out["visual.conv1.weight"] = _need(sd, v + "embeddings.patch_embedding.weight", (W, 3, arch.patch_size, arch.patch_size))
    out["visual.class_embedding"] = _need(sd, v + "embeddings.class_embedding", (W,))
    out["visual.positional_embedding"] = _need(sd, v + "embeddings.position_embedding.weight", (arch.tokens, W))
    out["visual.ln_pre.weight"], out["visual.ln_pre.bias"] = _need(sd, v + "pre_layrnorm.weight", (W,)), _need(sd, v + "pre_layrnorm.bias", (W,))
    out["visual.ln_post.weight"], out["visual.ln_post.bias"] = _need(sd, v + "post_layernorm.weight", (W,)), _need(sd, v + "post_layernorm.bias", (W,))
    out["visual.proj"] = _need(sd, "visual_projection.weight", (arch.out_dim, W)).detach().to(torch.float32).t().contiguous()
    return out


def temporal_weights(sd: Dict[str, Tensor], arch: LanguageBindArch, layer: int) -> Dict[str, Tensor]:
    """the temporal sub-block of one layer as fp32 host tensors: qkv_w [3W, W] (q | k | v packed), qkv_b [3W], out_w [W, W], out_b [W],
    ln_g / ln_b [W], temb [T, W] (the checkpoint's [1, T, W])"""
    p, W, T = f"vision_model.encoder.layers.{layer}.", arch.width, arch.num_frames
    f32 = lambda k, shape: _need(sd, p + k, shape).detach().to(torch.float32)
    return {"qkv_w": torch.cat([f32(f"temporal_attn.{n}_proj.weight", (W, W)) for n in "qkv"], dim=0),
            "qkv_b": torch.cat([f32(f"temporal_attn.{n}_proj.bias", (W,)) for n in "qkv"], dim=0),
            "out_w": f32("temporal_attn.out_proj.weight", (W, W)), "out_b": f32("temporal_attn.out_proj.bias", (W,)),
            "ln_g": f32("temporal_layer_norm1.weight", (W,)), "ln_b": f32("temporal_layer_norm1.bias", (W,)),
            "temb": f32("temporal_embedding", (1, T, W))[0].contiguous()}


class LanguageBindVideoTower(VitTokenTower):
    """`LanguageBindVideo` vision side (`vision_model.*`, `visual_projection.weight`) -> one embedding per clip.  bf16 operands only."""

    def __init__(self, arch: LanguageBindArch, sd: Dict[str, Tensor], device: str, precision: str = "bf16"):
        # one block per mq_encoder_forward call: the temporal sub-block sits between the blocks
        super().__init__(device, arch, precision, 1, frames=arch.num_frames)
        W, T = arch.width, arch.num_frames
        if not arch.add_time_attn:
            raise ValueError("LanguageBindVideoTower is the tower with temporal attention (vision_config.add_time_attn); a part without it is a CLIP ViT")
        if not 1 <= T <= MAX_FRAMES or arch.out_dim % 4 or arch.out_dim > 2048:
            raise ValueError(f"LanguageBindVideoTower takes 1 to {MAX_FRAMES} frames per clip and a projection dimension that is a multiple of 4, at most "
                             f"2048 (the checkpoint has num_frames = {T}, projection_dim = {arch.out_dim})")
        h = self._h
        self._load_hf_vit(sd, "vision_model.", "pre_layrnorm")
        self._proj = h.bf16(_need(sd, "visual_projection.weight", (arch.out_dim, W)))
        self._temporal = []
        for i in range(arch.layers):
            t = temporal_weights(sd, arch, i)
            self._temporal.append({k: (h.bf16(t[k]) if k in ("qkv_w", "out_w") else h.f32(t[k])) for k in t})

    def _forward(self, px: Tensor, out: Tensor, normalize: bool) -> None:
        """px fp32 [b, 3, T, S, S] on the device (contiguous) -> out fp32 [b, D]"""
        lib, a, s, dev = self.lib, self.arch, self._stream(), self.device
        b, W, T, N, D = px.shape[0], a.width, a.num_frames, a.tokens, a.out_dim
        frames, rows, G2 = b * T, b * T * N, a.grid ** 2
        bf16 = lambda *shape: torch.empty(*shape, dtype=torch.bfloat16, device=dev)
        f32 = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
        patches = bf16(frames * G2, self.Kp)
        L.check(lib.mq_patchify_clip(px.data_ptr(), patches.data_ptr(), b, T, a.image_size, a.patch_size, self.Kp, s), "mq_patchify_clip")
        x = self._tokens(patches, frames)
        del patches
        # the per-layer path's scratch, once per call
        xn, qkv, att = bf16(rows, W), bf16(rows, 3 * W), bf16(rows, W)
        ws = self._encoder_workspace(frames)
        res = L.MQ_EPI_BIAS | L.MQ_EPI_RESIDUAL | L.MQ_EPI_OUT_F32
        for i in range(a.layers):
            t = self._temporal[i]
            L.check(lib.mq_temporal_embed_ln(x.data_ptr(), t["temb"], t["ln_g"], t["ln_b"], xn.data_ptr(), b, T, N, W, a.ln_eps, s),
                    "mq_temporal_embed_ln")
            L.check(lib.mq_gemm_bf16(xn.data_ptr(), W, t["qkv_w"], W, t["qkv_b"], None, qkv.data_ptr(), 3 * W, rows, 3 * W, W, L.MQ_EPI_BIAS, s),
                    "mq_gemm_bf16")
            L.check(lib.mq_temporal_attention(qkv.data_ptr(), att.data_ptr(), b, T, N, W, a.heads, s), "mq_temporal_attention")
            L.check(lib.mq_gemm_bf16(att.data_ptr(), W, t["out_w"], W, t["out_b"], x.data_ptr(), x.data_ptr(), W, rows, W, W, res, s), "mq_gemm_bf16")
            self._encoder(x, frames, ws, first=i)
        cls_rows = torch.empty(frames, dtype=torch.int32, device=dev)
        cls_ln, proj = bf16(frames, W), f32(frames, D)
        pooled = out if not normalize else f32(b, D)
        L.check(lib.mq_cls_rows(cls_rows.data_ptr(), frames, N, s), "mq_cls_rows")
        L.check(lib.mq_layernorm(x.data_ptr(), cls_rows.data_ptr(), self._post[0], self._post[1], cls_ln.data_ptr(), None, frames, W, a.ln_eps, s),
                "mq_layernorm")
        L.check(lib.mq_gemm_bf16(cls_ln.data_ptr(), W, self._proj, W, None, None, proj.data_ptr(), D, frames, D, W, L.MQ_EPI_OUT_F32, s), "mq_gemm_bf16")
        L.check(lib.mq_avg_tokens(proj.data_ptr(), 0, pooled.data_ptr(), b, T, 0, D, s), "mq_avg_tokens")
        if normalize:
            L.check(lib.mq_l2_normalize(pooled.data_ptr(), out.data_ptr(), b, D, s), "mq_l2_normalize")

    def encode_clips(self, pixel_values: Tensor, normalize: bool = True) -> Tensor:
        """preprocessed fp32 [b, 3, T, S, S] (`pixel_values`, host or device) -> fp32 [b, D] on the device: visual_projection(mean over the frames
        of post_layernorm(class rows)), divided by its norm when `normalize`"""
        a = self.arch
        want = (3, a.num_frames, a.image_size, a.image_size)
        if not isinstance(pixel_values, torch.Tensor) or pixel_values.ndim != 5 or tuple(pixel_values.shape[1:]) != want:
            got = tuple(pixel_values.shape) if isinstance(pixel_values, torch.Tensor) else type(pixel_values).__name__
            raise ValueError(f"expected pixel_values [b, 3, {a.num_frames}, {a.image_size}, {a.image_size}] (b c t h w; the checkpoint's num_frames), got {got}")
        with torch.cuda.device(self.device):
            px = pixel_values.to(device=self.device, dtype=torch.float32, non_blocking=True).contiguous()
            n = px.shape[0]
            out = torch.empty(n, a.out_dim, dtype=torch.float32, device=self.device)
            for i in range(0, n, self.max_items_per_call):
                j = min(n, i + self.max_items_per_call)
                self._forward(px[i:j], out[i:j], bool(normalize))
        return out


class LanguageBindAudioTower(VitTokenTower):
    """`LanguageBindAudio` vision side (`vision_model.*`, `visual_projection.weight`) -> one embedding per spectrogram picture
    [3, num_mel_bins, target_length].  bf16 operands only."""

    def __init__(self, arch: LanguageBindArch, sd: Dict[str, Tensor], device: str, precision: str = "bf16"):
        if not arch.is_audio:
            raise ValueError("LanguageBindAudioTower is the tower of an audio part: vision_config.num_mel_bins and vision_config.target_length must "
                             f"be set (they are {arch.num_mel_bins} and {arch.target_length})")
        if arch.add_time_attn or arch.num_frames != 1:
            raise ValueError(f"an audio part is one picture without temporal attention (the checkpoint has add_time_attn = {arch.add_time_attn}, "
                             f"num_frames = {arch.num_frames})")
        if arch.num_mel_bins % arch.patch_size or arch.target_length % arch.patch_size:
            raise ValueError(f"the {arch.num_mel_bins} x {arch.target_length} picture of this audio part is no whole grid of {arch.patch_size}-pixel patches")
        super().__init__(device, arch, precision, arch.layers)
        W = arch.width
        if arch.out_dim % 4 or arch.out_dim > 2048:
            raise ValueError(f"LanguageBindAudioTower takes a projection dimension that is a multiple of 4, at most 2048 (the checkpoint has {arch.out_dim})")
        pos = _need(sd, "vision_model.embeddings.position_embedding.weight")
        if pos.ndim != 2 or pos.shape[0] != arch.tokens:
            raise ValueError(f"the checkpoint's position_embedding has {pos.shape[0]} rows, the {arch.grid_h} x {arch.grid_w} grid of a "
                             f"{arch.num_mel_bins} x {arch.target_length} picture at patch {arch.patch_size} needs {arch.tokens} (the reference resizes "
                             f"the positions before it loads the weights: a saved audio checkpoint already has them; nothing is interpolated here)")
        self._load_hf_vit(sd, "vision_model.", "pre_layrnorm")
        self._proj = self._h.bf16(_need(sd, "visual_projection.weight", (arch.out_dim, W)))

    def _forward(self, px: Tensor, out: Tensor, normalize: bool) -> None:
        """px fp32 [b, 3, bins, L] on the device (contiguous) -> out fp32 [b, D]"""
        lib, a, s, dev = self.lib, self.arch, self._stream(), self.device
        b, W, N, D = px.shape[0], a.width, a.tokens, a.out_dim
        patches = self._patchify_f32(px)
        x = self._tokens(patches, b)
        del patches
        self._encoder(x, b, self._encoder_workspace(b))
        cls_rows = torch.empty(b, dtype=torch.int32, device=dev)
        cls_ln = torch.empty(b, W, dtype=torch.bfloat16, device=dev)
        proj = out if not normalize else torch.empty(b, D, dtype=torch.float32, device=dev)
        L.check(lib.mq_cls_rows(cls_rows.data_ptr(), b, N, s), "mq_cls_rows")
        L.check(lib.mq_layernorm(x.data_ptr(), cls_rows.data_ptr(), self._post[0], self._post[1], cls_ln.data_ptr(), None, b, W, a.ln_eps, s), "mq_layernorm")
        L.check(lib.mq_gemm_bf16(cls_ln.data_ptr(), W, self._proj, W, None, None, proj.data_ptr(), D, b, D, W, L.MQ_EPI_OUT_F32, s), "mq_gemm_bf16")
        if normalize:
            L.check(lib.mq_l2_normalize(proj.data_ptr(), out.data_ptr(), b, D, s), "mq_l2_normalize")

    def encode_spectrograms(self, pixel_values: Tensor, normalize: bool = True) -> Tensor:
        """preprocessed fp32 [b, 3, bins, L] (`pixel_values`, host or device) -> fp32 [b, D] on the device: visual_projection(post_layernorm(class
        row)), divided by its norm when `normalize`"""
        a = self.arch
        want = (3, a.num_mel_bins, a.target_length)
        if not isinstance(pixel_values, torch.Tensor) or pixel_values.ndim != 4 or tuple(pixel_values.shape[1:]) != want:
            got = tuple(pixel_values.shape) if isinstance(pixel_values, torch.Tensor) else type(pixel_values).__name__
            raise ValueError(f"expected pixel_values [b, 3, {a.num_mel_bins}, {a.target_length}] (the checkpoint's num_mel_bins x target_length), got {got}")
        with torch.cuda.device(self.device):
            px = pixel_values.to(device=self.device, dtype=torch.float32, non_blocking=True).contiguous()
            n = px.shape[0]
            out = torch.empty(n, a.out_dim, dtype=torch.float32, device=self.device)
            for i in range(0, n, self.max_items_per_call):
                j = min(n, i + self.max_items_per_call)
                self._forward(px[i:j], out[i:j], bool(normalize))
        return out


class LanguageBindModel:
    """The parts of one LanguageBind model name on one device: video tower, audio tower, image tower (each when the name has that part), the text
    tower of the LAST part in the reference's order (the image part's when present, else the audio part's, else the video part's), its tokenizer,
    and each part's logit_scale."""

    def __init__(self, name: str, localpath: str, device: str, precision: str = "bf16"):
        if name not in MODEL_PARTS:
            raise ValueError(f"Unsupported LanguageBind model: {name}")
        parts = MODEL_PARTS[name]
        _check_precision(precision, ("bf16",), f"LanguageBind models run on bf16 operands only ('enginePrecision': {precision!r} is not supported)")
        if not localpath or not os.path.isdir(localpath):
            raise FileNotFoundError(f"{name}: `localpath` must be a directory with one sub-directory per part ({', '.join(parts.values())}); "
                                    f"got {localpath!r}.  Weights are read from disk only")
        self.name, self.parts, self.device = name, dict(parts), device
        self.logit_scale: Dict[str, float] = {}
        self.video: Optional[LanguageBindVideoTower] = None
        self.audio: Optional[LanguageBindAudioTower] = None
        self.image: Optional[VitTower] = None
        last_dir = last_sd = last_arch = None
        for kind, part in parts.items():
            d = os.path.join(localpath, part)
            if not os.path.isdir(d) or not os.path.isfile(os.path.join(d, "config.json")) or \
                    checkpoint._first_existing(d, checkpoint.HF_WEIGHT_FILES) is None:
                raise FileNotFoundError(f"{name}: the {kind} part's checkpoint directory {d} (config.json + {' | '.join(checkpoint.HF_WEIGHT_FILES)}) was not found")
            cfg, sd = checkpoint.load_hf_dir(d)
            try:
                arch = archs.languagebind_arch_from_hf_config(cfg)
            except KeyError as e:
                raise ValueError(f"{d}: {e.args[0] if e.args else e}") from e
            if kind == "video":
                self.video = LanguageBindVideoTower(arch, sd, device)
            elif kind == "audio":
                try:
                    self.audio = LanguageBindAudioTower(arch, sd, device)
                except ValueError as e:
                    raise ValueError(f"{d}: {e}") from e
            else:
                if arch.add_time_attn:
                    raise ValueError(f"{d}: the image part must not have temporal attention (vision_config.add_time_attn)")
                self.image = VitTower(arch.vision(), vision_state_dict(sd, arch), device)
            self.logit_scale[kind] = float(_need(sd, "logit_scale").detach().to(torch.float32).reshape(()))
            last_dir, last_sd, last_arch = d, sd, arch
        self.arch = last_arch
        self.out_dim = last_arch.out_dim
        self.tokenizer: ClipBpeTokenizer = load_tokenizer(last_dir, last_arch.ctx)
        if self.tokenizer.eot_id >= last_arch.vocab:
            raise ValueError(f"the tokenizer's EOT id {self.tokenizer.eot_id} is outside the model's vocabulary of {last_arch.vocab}")
        self.text = ClipTextTower(last_arch.text(), clip_text_state_dict(last_sd, "text_model.", "text_projection.weight", last_arch.text()), device)
        self.text.release_unused_folded()

    # ---- text ----------------------------------------------------------------------------------------------------------------------------------
    def token_ids(self, texts) -> np.ndarray:
        """-> int64 [n, ctx]: SOT ids EOT, zero-padded, truncated to ctx positions with the EOT kept (the reference's tokenizer call:
        max_length = 77, truncation, multimodal_model_load.py:257; its padding id is the EOT's, which the causal mask keeps from the pooled row)"""
        tok, ctx = self.tokenizer, self.arch.ctx
        out = np.zeros((len(texts), ctx), dtype=np.int64)
        for i, t in enumerate(texts):
            if not isinstance(t, str):
                raise TypeError(f"a LanguageBind text is a string, found {type(t).__name__}")
            ids = [tok.sot_id] + tok.encode(t)[:ctx - 2] + [tok.eot_id]
            out[i, :len(ids)] = ids
        return out

    def encode_text(self, texts, normalize: bool = True) -> Tensor:
        """-> fp32 [n, D] unit rows on the device (a text row is the unit vector whatever `normalize` says: languagebind/__init__.py:59-62)"""
        dev = self.text.device
        with request_stream(dev, device_output=True):
            return self.text.encode_ids(torch.from_numpy(self.token_ids(list(texts))), normalize=True).to(dev, non_blocking=True)

    # ---- video / audio / image ----------------------------------------------------------------------------------------------------------------------
    def _scaled(self, unit: Tensor, kind: str, normalize: bool) -> Tensor:
        """languagebind/__init__.py:59-63, multimodal_model_load.py:298-299: the unit row times exp(logit_scale) of its part; unit again with
        `normalize` (the row IS the unit vector then: it is not scaled and divided again)"""
        return unit if normalize else unit * float(np.exp(np.float32(self.logit_scale[kind])))     # (a scalar factor on [n, D]: no FLOP of the towers)

    def encode_video(self, pixel_values: Tensor, normalize: bool = True) -> Tensor:
        if self.video is None:
            raise ValueError(f"{self.name} has no video part")
        with request_stream(self.video.device, device_output=True):
            return self._scaled(self.video.encode_clips(pixel_values, normalize=True), "video", normalize)

    def encode_audio(self, pixel_values: Tensor, normalize: bool = True) -> Tensor:
        """preprocessed fp32 [b, 3, num_mel_bins, target_length] -> fp32 [b, D] on the device"""
        if self.audio is None:
            raise ValueError(f"{self.name} has no audio part")
        with request_stream(self.audio.device, device_output=True):
            return self._scaled(self.audio.encode_spectrograms(pixel_values, normalize=True), "audio", normalize)

    def audio_preprocessor(self, resample: bool = False):
        """engine/audio.py's front end for this model's audio part (waveforms -> `pixel_values`), None without one.  `resample`: a (waveform, rate)
        pair at another rate than the checkpoint's is resampled on the GPU where it is refused otherwise"""
        if self.audio is None:
            return None
        from marqo_amd.engine.audio import AudioPreprocessor
        a = self.audio.arch
        return AudioPreprocessor(str(self.audio.device), a.num_mel_bins, a.target_length, a.audio_sample_rate, a.audio_mean, a.audio_std,
                                 resample=bool(resample))

    def video_preprocessor(self):
        """engine/video.py's front end for this model's video part (decoded uint8 frames -> `pixel_values`), None without one.  The side and the
        frame count are the checkpoint's `image_size` and `num_frames` (the reference hard-codes 224; the released checkpoints are 224)"""
        if self.video is None:
            return None
        from marqo_amd.engine.video import VideoPreprocessor
        a = self.video.arch
        return VideoPreprocessor(str(self.video.device), a.image_size, a.num_frames)

    def encode_image_u8(self, u8: Tensor, normalize: bool = True) -> Tensor:
        """uint8 [n, S, S, 3] on the device (resized and cropped) -> fp32 [n, D] on the device"""
        if self.image is None:
            raise ValueError(f"{self.name} has no image part")
        with request_stream(self.image.device, device_output=True):
            return self._scaled(self.image.encode_u8(u8, normalize=True), "image", normalize)

    def encode_image_f32(self, pixels: Tensor, normalize: bool = True) -> Tensor:
        """preprocessed fp32 [n, 3, S, S] -> fp32 [n, D] on the device"""
        if self.image is None:
            raise ValueError(f"{self.name} has no image part")
        with request_stream(self.image.device, device_output=True):
            return self._scaled(self.image.encode_f32(pixels, normalize=True), "image", normalize)

"""The `languagebind` loader: the engine's `MultimodalModel` and `LanguageBindEncoder` (reference: s2_inference/multimodal_model_load.py:42-115,
204-311; the model itself: s2_inference/languagebind/__init__.py:33-64).  Written from the behaviour, not from the text, of those classes.

What is served: all six names of the reference's part table (`LanguageBind/Video_V1.5_FT`, `..._Image`, `..._Audio_FT`, `..._Audio_FT_Image`,
`LanguageBind/Audio_FT`, `LanguageBind/Audio_FT_Image`) on the HIP towers of engine/languagebind.py, modalities VIDEO, AUDIO, IMAGE and TEXT, bf16.
AUDIO content is the `pixel_values` [b, 3, num_mel_bins, target_length] of the reference's audio processor; `preprocessor(Modality.AUDIO)` of a
model with an audio part is engine/audio.py's AudioPreprocessor, which makes them on the GPU from 16 kHz waveforms (Kaldi fbank, the three-crop
fusion) — and, with `"resampleAudio": true` in model_properties, from (waveform, rate) pairs at any rate its polyphase resampler serves.  VIDEO
content is `pixel_values` [b, 3, T, S, S], or the decoded frames themselves: a uint8 [T_in, H, W, 3] tensor or ndarray, a list of them, or
`{"frames": ...}` dicts, which engine/video.py's VideoPreprocessor (`preprocessor(Modality.VIDEO)` of a model with a video part) turns into
`pixel_values` on the GPU.  What is not:
  * decoding media: no video / audio decoder is a dependency of this engine; paths, URLs and bytes are refused.  Without `resampleAudio` a
    waveform at another rate than the checkpoint's is refused;
  * the reference's randomness: its video processor applies a RANDOM horizontal flip, and its audio processor draws the three crop starts of a
    clip longer than target_length at RANDOM.  VideoPreprocessor never flips unless told to (`flip`); AudioPreprocessor takes the middle of each
    third and accepts explicit `starts` (engine/video.py, engine/audio.py);
  * fp8 ('enginePrecision': 'fp8' is refused like the ConvNeXt towers: bf16 only);
  * downloads: `localpath` in model_properties names a directory with one sub-directory per part (LanguageBind_Video_V1.5_FT,
    LanguageBind_Audio_FT, LanguageBind_Image), each a Hugging Face checkpoint directory (config.json, model.safetensors | pytorch_model.bin,
    vocab.json, merges.txt).

The names are reached through `model_properties` (the reference's registry dict for the name, plus `localpath`), as the NLLB-CLIP names are: the
registry's 204 names and 12 loader keys are pinned by tests.  `s2_inference._load_model`, `validate_model_properties` and `get_encoder`
special-case `type == "languagebind"` where the reference does (s2_inference.py:173,382,539).

One difference from the reference: for a list of `pixel_values` dicts EVERY item is encoded (the reference reads `content[0]` only,
multimodal_model_load.py:285-287); for a one-item list the result is the same.
"""
from __future__ import annotations

import threading
from typing import Any, Dict, List, Optional

import numpy as np
import torch

from marqo_amd.s2_inference.enums import Modality
from marqo_amd.s2_inference.errors import InvalidModelPropertiesError, ModelLoadError

SERVED_MODALITIES = (Modality.VIDEO, Modality.AUDIO, Modality.IMAGE, Modality.TEXT)


class MultimodalModelProperties:
    """multimodal_model_load.py:42-49 (a pydantic model there): name, loader, supported_modalities, dimensions, video_chunk_length and
    audio_chunk_length are required; `type` defaults to "multimodal"; other keys (localpath, model_size, ...) are ignored here"""
    REQUIRED = ("name", "loader", "supported_modalities", "dimensions", "video_chunk_length", "audio_chunk_length")

    def __init__(self, **p: Any):
        missing = [k for k in self.REQUIRED if k not in p]
        if missing:
            raise InvalidModelPropertiesError(f"model_properties of a multimodal model has missing key(s) {missing}; required: {list(self.REQUIRED)}")
        if not isinstance(p["name"], str) or not isinstance(p["loader"], str):
            raise InvalidModelPropertiesError("model_properties 'name' and 'loader' of a multimodal model must be strings")
        try:
            self.supported_modalities: List[Modality] = [Modality(m) for m in p["supported_modalities"]]
        except (ValueError, TypeError) as e:
            raise InvalidModelPropertiesError(f"model_properties 'supported_modalities' must be a list of {[m.value for m in Modality]}: {e}") from e
        for k in ("dimensions", "video_chunk_length", "audio_chunk_length"):
            if isinstance(p[k], bool) or not isinstance(p[k], int):
                raise InvalidModelPropertiesError(f"model_properties '{k}' of a multimodal model must be an integer, received {p[k]!r}")
        self.name, self.loader, self.dimensions = p["name"], p["loader"], p["dimensions"]
        self.type = p.get("type", "multimodal")
        self.video_chunk_length, self.audio_chunk_length = p["video_chunk_length"], p["audio_chunk_length"]


class MultimodalModel:
    """multimodal_model_load.py:52-115.  `model` is the engine's LanguageBindModel (the towers), `encoder` the LanguageBindEncoder in front of it."""

    def __init__(self, model_name: str, model_properties: Dict[str, Any], device: str):
        self.model_name = model_name
        self.model_properties = dict(model_properties)
        self.properties = MultimodalModelProperties(**model_properties)
        self.device = device
        self.model = None
        self.encoder = None
        self.clip_type: Optional[Dict[str, str]] = None
        resample = self.model_properties.get("resampleAudio", False)
        if not isinstance(resample, bool):
            raise InvalidModelPropertiesError(f"model_properties 'resampleAudio' must be true or false, received {resample!r}")
        self.resample_audio = resample      # AudioPreprocessor resamples a waveform at another rate than the checkpoint's (off: it refuses it)

    def _load_multimodal_model(self):
        if self.properties.loader == "languagebind":
            return self._load_languagebind_model()
        raise ValueError(f"Unsupported loader: {self.properties.loader}")

    def _load_languagebind_model(self):
        """A name with an audio part is served when `<localpath>/LanguageBind_Audio_FT` is a checkpoint directory, and that directory is looked
        for FIRST.  Without it the name is refused with InvalidModelPropertiesError, where a missing video or image directory is a
        ModelLoadError: the audio names were refused as invalid properties before this engine had an audio tower, and every caller who has no
        audio checkpoint keeps seeing exactly that — the properties name a part that `localpath` does not hold — while the names that were
        always served keep their load error."""
        import os
        from marqo_amd.engine import checkpoint
        from marqo_amd.engine import languagebind as LB
        if self.model_name not in LB.MODEL_PARTS:
            raise ValueError(f"Unsupported LanguageBind model: {self.model_name}")
        parts = LB.MODEL_PARTS[self.model_name]
        if "audio" in parts:
            root = self.model_properties.get("localpath")
            d = os.path.join(str(root), parts["audio"]) if root else None
            if d is None or not os.path.isfile(os.path.join(d, "config.json")) or checkpoint._first_existing(d, checkpoint.HF_WEIGHT_FILES) is None:
                raise InvalidModelPropertiesError(
                    f"{self.model_name}: its audio part {parts['audio']} needs the checkpoint directory "
                    f"{d if d else '<localpath>/' + parts['audio']} (config.json + {' | '.join(checkpoint.HF_WEIGHT_FILES)}), which was not found"
                    f"{'' if root else ' (model_properties has no `localpath`)'}; the names without an audio part are "
                    f"{[n for n, p in LB.MODEL_PARTS.items() if 'audio' not in p]}")
        precision = str(self.model_properties.get("enginePrecision", "bf16")).lower()
        if precision != "bf16":
            raise InvalidModelPropertiesError(f"{self.model_name}: LanguageBind towers run on bf16 operands only ('enginePrecision': {precision!r} is not supported)")
        self.clip_type = dict(parts)
        try:
            return LB.LanguageBindModel(self.model_name, self.model_properties.get("localpath"), self.device)
        except FileNotFoundError as e:
            raise ModelLoadError(f"Unable to load {self.model_name}: {e}") from e

    def load(self) -> None:
        self.model = self._load_multimodal_model()
        self.encoder = LanguageBindEncoder(self)

    def preprocessor(self, modality):
        if self.encoder is None:
            raise ValueError("Model has not been loaded yet. Call _load_model() first.")
        return self.encoder.preprocessor(modality)

    def encode(self, content, modality, **kwargs):
        if self.encoder is None:
            raise ValueError("Model has not been loaded yet. Call _load_model() first.")
        return self.encoder.encode(content, modality, **kwargs)


def raw_video_clips(content) -> Optional[list]:
    """VIDEO content that is decoded frames -> the list of clips for engine/video.py's VideoPreprocessor, None for anything else (which is then
    judged as `pixel_values`, with the messages it always had): one uint8 [T_in, H, W, 3] tensor / ndarray, one {"frames": such an array} dict, or a
    non-empty list of these"""
    is_u8 = lambda x: (isinstance(x, torch.Tensor) and x.dtype == torch.uint8 and x.ndim == 4) or \
        (isinstance(x, np.ndarray) and x.dtype == np.uint8 and x.ndim == 4)
    is_clip = lambda x: is_u8(x) or (isinstance(x, dict) and set(x) == {"frames"} and is_u8(x["frames"]))
    if is_clip(content):
        return [content]
    if isinstance(content, (list, tuple)) and len(content) > 0 and all(is_clip(x) for x in content):
        return list(content)
    return None


def video_pixel_values(content, modality: Modality = Modality.VIDEO, ndim: int = 5, tail: Optional[tuple] = None) -> List[torch.Tensor]:
    """What VIDEO content may be -> the list of `pixel_values` tensors to encode, each [b, 3, T, S, S], in order:
    a list of dicts with a `pixel_values` tensor (what the reference's caller hands over, multimodal_model_load.py:285-287; every item, not only
    the first), one such dict, or such a tensor itself.  Anything else — URLs included: nothing here decodes media — raises ValueError with the
    reference's message (:291).  AUDIO content is the same with ndim = 4 and `tail` the shape behind the batch axis."""
    bad = lambda: ValueError(f"Unsupported {modality.value} content type: {type(content)}, content: {content}")
    if isinstance(content, torch.Tensor):
        items = [content]
    elif isinstance(content, dict):
        items = [content]
    elif isinstance(content, (list, tuple)) and len(content) > 0:
        items = list(content)
    else:
        raise bad()
    out = []
    for it in items:
        if isinstance(it, dict) and isinstance(it.get("pixel_values"), torch.Tensor):
            it = it["pixel_values"]
        if not isinstance(it, torch.Tensor) or it.ndim != ndim or (tail is not None and tuple(it.shape[1:]) != tuple(tail)):
            raise bad()
        out.append(it)
    return out


class LanguageBindEncoder:
    """multimodal_model_load.py:204-311 on the engine's towers.  encode(content, modality, normalize) -> np.ndarray fp32 [n, D]:
    with normalize every row is unit; without, a video, audio or image row is the unit vector times exp(logit_scale) of its part and a text row
    is the unit vector (languagebind/__init__.py:59-63)."""

    def __init__(self, model: MultimodalModel):
        self.model = model
        self._local = threading.local()
        self._audio_pre = None
        self._video_pre = None

    def preprocessor(self, modality):
        """The reference returns its video / audio / image processor objects here.  AUDIO on a model with an audio part: the engine's
        AudioPreprocessor (waveforms -> `pixel_values` on the GPU; with `resampleAudio` in model_properties at any served rate, else at the
        checkpoint's).  VIDEO on a model with a video part: the engine's VideoPreprocessor (decoded uint8 frames -> `pixel_values` on the GPU).
        Neither decodes anything.  Everything else: None"""
        lb = self.model.model
        if modality in (Modality.VIDEO, Modality.VIDEO.value) and getattr(lb, "video", None) is not None:
            if self._video_pre is None:
                self._video_pre = lb.video_preprocessor()
            return self._video_pre
        if modality not in (Modality.AUDIO, Modality.AUDIO.value) or getattr(lb, "audio", None) is None:
            return None
        if self._audio_pre is None:
            self._audio_pre = lb.audio_preprocessor(resample=True) if self.model.resample_audio else lb.audio_preprocessor()
        return self._audio_pre

    def _image_pre(self):
        p = getattr(self._local, "pre", None)
        if p is None:
            from marqo_amd.engine.preprocess import ImagePreprocessor
            lb = self.model.model
            p = self._local.pre = ImagePreprocessor(str(lb.image.device), lb.image.arch.image_size)
        return p

    def _encode_images(self, content, normalize: bool, image_download_headers: Optional[dict]) -> torch.Tensor:
        """what the image loaders accept (PIL image, path or URL, uint8 ndarray, preprocessed tensor; one or a list): Resize(S, bicubic) +
        CenterCrop(S) + the OpenAI mean / std of the reference's LanguageBindImageProcessor, on the GPU"""
        from marqo_amd.s2_inference.image_input import format_and_load_CLIP_image, pil_to_pixels
        lb = self.model.model
        if lb.image is None:
            raise ValueError(f"{self.model.model_name} has no image part")
        if isinstance(content, torch.Tensor) and content.ndim == 4:
            return lb.encode_image_f32(content, normalize)
        items = list(content) if isinstance(content, (list, tuple)) else [content]
        loaded = [i if isinstance(i, np.ndarray) and i.dtype == np.uint8 and i.ndim == 3 and i.shape[2] == 3
                  else format_and_load_CLIP_image(i, image_download_headers or {}) for i in items]
        if all(isinstance(i, torch.Tensor) for i in loaded):
            return lb.encode_image_f32(torch.stack([t.to(lb.image.device) for t in loaded]), normalize)
        if any(isinstance(i, torch.Tensor) for i in loaded):
            raise ValueError("a list of images is either all preprocessed tensors or none")
        with torch.cuda.device(lb.image.device):
            u8 = self._image_pre().resize_crop_u8([i if isinstance(i, np.ndarray) else pil_to_pixels(i) for i in loaded])
        return lb.encode_image_u8(u8, normalize)

    def encode(self, content, modality, normalize=True, image_download_headers: Optional[dict] = None, **kwargs):
        lb = self.model.model
        if lb is None:
            raise ValueError("Model has not been loaded yet. Call _load_model() first.")
        modality = Modality(modality) if not isinstance(modality, Modality) else modality
        if modality == Modality.TEXT:
            texts = [content] if isinstance(content, str) else list(content)
            out = lb.encode_text(texts, bool(normalize))
        elif modality == Modality.IMAGE:
            out = self._encode_images(content, bool(normalize), image_download_headers)
        elif modality == Modality.VIDEO:
            clips = raw_video_clips(content) if getattr(lb, "video", None) is not None else None
            if clips is not None:        # decoded frames: the GPU front end makes their pixel_values
                out = lb.encode_video(self.preprocessor(Modality.VIDEO)(clips)["pixel_values"], bool(normalize))
            else:
                out = torch.cat([lb.encode_video(px, bool(normalize)) for px in video_pixel_values(content, modality)], dim=0)
        elif modality == Modality.AUDIO and getattr(lb, "audio", None) is not None:
            a = lb.audio.arch
            spectrograms = video_pixel_values(content, modality, ndim=4, tail=(3, a.num_mel_bins, a.target_length))
            out = torch.cat([lb.encode_audio(px, bool(normalize)) for px in spectrograms], dim=0)
        else:
            raise ValueError(f"Unsupported {modality.value} content type: {type(content)}, content: {content}")
        return out.cpu().numpy()

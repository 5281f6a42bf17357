"""`hf` / `hf_stella` loaders of the engine.

Drop-in for HuggingFaceModel (src/marqo/core/inference/embedding_models/hugging_face_model.py:24-214): same ctor,
load(), encode(sentence, normalize=True, **kwargs) -> np.ndarray[N, D] fp32.  Tokenisation keeps the reference's flags
(padding=True, truncation=True, max_length=tokens, :179-185); the BERT encoder, masked mean / CLS pooling (:205-214) and
F.normalize (:194-195) run in libmarqo_hip.so on packed (un-padded) sequences.
"""
from __future__ import annotations

import os
import threading
from typing import List, Optional, Union

import numpy as np
import torch

from marqo_amd import _lib as L
from marqo_amd.engine import archs, checkpoint, synthetic
from marqo_amd.engine.gpu_tokenizers import prefers_host
from marqo_amd.engine.towers import request_stream
from marqo_amd.engine.tokenizers import RobertaBpeTokenizer, SyntheticTokenizer, WordPieceTokenizer, XlmRobertaTokenizer
from marqo_amd.s2_inference.abstract_models import AbstractEmbeddingModel
from marqo_amd.s2_inference.errors import InternalError, InvalidModelPropertiesError, ModelLoadError


class HuggingFaceModelProperties:
    """Validated view of model_properties (reference: hugging_face_model_properties.py:40-137)."""

    POOLING_ERROR = "pooling_method must be 'mean' or 'cls'"

    def __init__(self, **p):
        dims = p.get("dimensions")
        if not isinstance(dims, int) or dims < 1:
            raise ValueError("'dimensions' must be a positive integer")
        self.dimensions: int = dims
        self.type: str = p.get("type")
        if self.type not in ("hf", "hf_stella"):
            raise ValueError("The type of the model should be 'hf' or 'hf_stella'.")
        self.name: Optional[str] = p.get("name")
        # engine extension: `localpath` = a checkpoint directory on disk (config.json + weights + tokenizer files), as the open_clip loader takes
        # one; it is looked up exactly like a directory given as `name`
        self.localpath: Optional[str] = p.get("localpath")
        if self.localpath is not None:
            if not isinstance(self.localpath, str) or not self.localpath:
                raise ValueError("'localpath' must be a directory path")
            if self.name is None:
                self.name = self.localpath
        self.tokens: int = int(p.get("tokens", 128))
        self.url: Optional[str] = p.get("url")
        self.model_location = p.get("model_location", p.get("modelLocation"))
        if self.url and self.model_location:
            raise ValueError("Only one of 'url' and 'model_location' should be provided.")
        if not self.name and not (self.url or self.model_location):
            raise ValueError("At least one of 'name', 'url', or 'model_location' should be provided.")
        pm = p.get("pooling_method", p.get("poolingMethod"))
        if pm is not None and pm not in ("mean", "cls", "last"):
            raise ValueError(self.POOLING_ERROR)
        # None: inferred at load from 1_Pooling/config.json, default mean.  'last' (last-token pooling) is taken by the decoder-style checkpoints (Qwen3 / Qwen2, Mistral / Llama) only:
        # the other families refuse it at load with the same text
        self.pooling_method: Optional[str] = pm
        self.trust_remote_code: bool = bool(p.get("trust_remote_code", p.get("trustRemoteCode", False)))
        # engine extension: operand type of the encoder-block GEMMs, "bf16" (default) or "fp8" (e4m3 MX-MFMA; calibrated at load on
        # fixed seeded inputs, 'fp8Budget' bounds the error), see open_clip_model.OpenCLIPModelProperties
        self.engine_precision: str = p.get("enginePrecision", p.get("engine_precision", os.environ.get("MARQO_AMD_PRECISION", "bf16")))
        if self.engine_precision not in ("bf16", "fp8"):
            raise ValueError("'enginePrecision' must be 'bf16' or 'fp8'")
        b = p.get("fp8Budget", p.get("fp8_budget"))
        if b is not None and not (isinstance(b, (int, float)) and b > 0):
            raise ValueError("'fp8Budget' must be a positive number")
        self.fp8_budget: Optional[float] = None if b is None else float(b)
        # engine extension (Jina v3 checkpoints): 'loraTask' = the task adapter every text of this model runs (None: the base model, what the
        # reference's AutoModel returns), 'loraAdapters' = {task name: PEFT adapter directory} on top of the checkpoint's own adapter sub-directories
        self.lora_task: Optional[str] = p.get("loraTask", p.get("lora_task"))
        if self.lora_task is not None and (not isinstance(self.lora_task, str) or not self.lora_task):
            raise ValueError("'loraTask' must be a task name")
        self.lora_adapters: Optional[dict] = p.get("loraAdapters", p.get("lora_adapters"))
        if self.lora_adapters is not None and not (isinstance(self.lora_adapters, dict) and
                                                   all(isinstance(k, str) and isinstance(v, str) and k and v for k, v in self.lora_adapters.items())):
            raise ValueError("'loraAdapters' must map task names to adapter directories")

    def dict(self) -> dict:
        return dict(self.__dict__)


class HuggingFaceModel(AbstractEmbeddingModel):
    supports_dynamic_batching = True
    _requires_trust_remote_code = False
    _check_dimensions = True

    def __init__(self, model_properties: dict, device: str, model_auth=None, model_flags=None, tokenizer_flags=None):
        super().__init__(model_properties, device, model_auth)
        self.model_properties = self._build_model_properties(model_properties or {})
        self._model = None
        self._tokenizer = None
        self._pooling_func = None
        self.weights_source = None
        self._calib_lock = threading.Lock()

    def _build_model_properties(self, model_properties: dict) -> HuggingFaceModelProperties:
        try:
            parsed = HuggingFaceModelProperties(**model_properties)
        except (ValueError, TypeError) as e:
            raise InvalidModelPropertiesError(f"Invalid model properties: {model_properties}. Original error {e}") from e
        if self._requires_trust_remote_code and not parsed.trust_remote_code:
            raise InvalidModelPropertiesError("The specified model requires the 'trustRemoteCode' attribute to be set to True. "
                                              "Setting this attribute to True may have security implications.")
        return parsed

    def _check_loaded_components(self):
        if self._model is None:
            raise InternalError("Model is not loaded!")
        if self._tokenizer is None:
            raise InternalError("Tokenizer is not loaded!")
        if self._pooling_func is None:
            raise InternalError("Pooling function is not loaded!")

    def _load_necessary_components(self):
        if not str(self.device).startswith("cuda"):
            raise L.MarqoHipUnavailableError(
                f"marqo_amd runs its towers on an AMD GPU only (device 'cuda' / 'cuda:N' on ROCm); got {self.device!r}")
        from marqo_amd.engine import towers
        props = self.model_properties
        if not props.name:
            raise ModelLoadError("downloading model archives ('url' / 'model_location') is control-plane work outside the marqo_amd "
                                 "engine; unpack the archive on disk and pass its directory as 'name'")
        directory = checkpoint.find_hf_dir(props.name)
        if directory is not None:
            try:   # (a sharded checkpoint's tensors go to the device shard by shard)
                cfg, sd = checkpoint.load_hf_dir(directory, device=self.device)
            except checkpoint.ShardedCheckpointError as e:   # a shard the index names is missing, torch-pickle shards (single-file directories: as before)
                raise ModelLoadError(f"{props.name}: {e}") from e
            try:
                # (Mistral / Llama are selected here: bert_arch_from_hf_config keeps refusing them for the callers that run BERT-family encoders only)
                arch = archs.llama_arch_from_hf_config(cfg) if cfg.get("model_type") in ("mistral", "llama") else archs.bert_arch_from_hf_config(cfg)
            except KeyError as e:
                raise InvalidModelPropertiesError(f"{props.name}: {e}. Only BERT-family encoders run on the marqo_amd engine.") from e
            if isinstance(arch, archs.ModernBertArch):
                self._load_modernbert(directory, arch, sd)
                return
            if isinstance(arch, archs.QwenArch):
                self._load_qwen(directory, arch, cfg, sd)
                return
            if isinstance(arch, archs.LlamaArch):
                self._load_llama(directory, arch, cfg, sd)
                return
            if isinstance(arch, archs.GemmaArch):
                self._load_gemma(directory, arch, sd)
                return
            if isinstance(arch, archs.T5Arch):
                self._load_t5(directory, arch, sd)
                return
            if isinstance(arch, archs.JinaBertArch):
                self._load_jina_bert(directory, arch, sd)
                return
            if isinstance(arch, archs.NomicBertArch):
                self._load_nomic_bert(directory, arch, sd)
                return
            if isinstance(arch, archs.JinaV3Arch):
                self._load_jina_v3(directory, arch, sd)
                return
            if (arch.glu or arch.rope_theta is not None) and not props.trust_remote_code:
                # a NewModel checkpoint is custom remote code to the reference's AutoModel: refused unless trustRemoteCode is set
                raise InvalidModelPropertiesError(f"{props.name} is a custom-code (NewModel) checkpoint: the reference loads it only with "
                                                  f"'trustRemoteCode': True (type 'hf_stella')")
            if os.path.isfile(os.path.join(directory, "sentencepiece.bpe.model")):  # XLM-RoBERTa checkpoints (multilingual-e5)
                self._tokenizer = XlmRobertaTokenizer(directory)
            elif all(os.path.isfile(os.path.join(directory, f)) for f in ("vocab.json", "merges.txt")) and \
                    not os.path.isfile(os.path.join(directory, "vocab.txt")):
                # RoBERTa checkpoints (all-roberta-large-v1, all-distilroberta-v1 ...): GPT-2 byte-level BPE
                if self._adds_prefix_space(directory):
                    raise InvalidModelPropertiesError(f"{props.name}: its tokenizer_config.json sets add_prefix_space, which the byte-level BPE "
                                                      f"tokeniser of the marqo_amd engine does not implement")
                try:
                    self._tokenizer = RobertaBpeTokenizer(directory)
                except ValueError as e:   # a vocab.json without <s> / <pad> / </s> / <unk>
                    raise InvalidModelPropertiesError(f"{props.name}: {e}") from e
            elif arch.rel_buckets:
                # MPNetTokenizer = BERT's basic + WordPiece tokenisation around "<s> ... </s>" (transformers tokenization_mpnet.py); the
                # special-token spellings come from the checkpoint's tokenizer_config.json / special_tokens_map.json
                self._tokenizer = WordPieceTokenizer(directory, do_lower_case=self._do_lower_case(directory),
                                                     **self._special_tokens(directory, unk="[UNK]", cls="<s>", sep="</s>", pad="<pad>", mask="<mask>"))
            else:
                self._tokenizer = WordPieceTokenizer(directory, do_lower_case=self._do_lower_case(directory))
            self.weights_source = directory
        elif checkpoint.synthetic_weights_enabled() and props.name in archs.HF_BERT_ARCHS:
            arch = archs.HF_BERT_ARCHS[props.name]
            sd = synthetic.random_bert_state_dict(arch, seed=0)
            self._tokenizer = SyntheticTokenizer("bert", arch.vocab)  # (for XLM-R archs too: ids only need to be in range)
            self.weights_source = "synthetic(seed=0)"
        else:
            raise InvalidModelPropertiesError(
                f"Marqo encountered an error loading the Hugging Face model, modelProperties={props.dict()}. No local copy under "
                f"{checkpoint.model_dir()} or the Hugging Face cache (there is no network download in the marqo_amd engine).")
        if self._check_dimensions and arch.width != props.dimensions:
            raise InvalidModelPropertiesError(f"'dimensions'={props.dimensions} but the encoder width is {arch.width}")
        self._refuse_last_pooling()
        pooling = props.pooling_method or checkpoint.read_pooling_config(directory) or "mean"
        self.arch = arch
        try:
            self._model = towers.BertTower(arch, sd, self.device, pooling=pooling, precision=props.engine_precision)
        except ValueError as e:  # e.g. fp8 needs width / mlp_dim multiples of 128
            raise InvalidModelPropertiesError(str(e)) from e
        self._pooling_func = pooling
        if props.engine_precision == "fp8":   # deterministic load-time calibration on fixed seeded inputs (see open_clip_model.py)
            self._model.tune_fp8_default(props.fp8_budget)
        self._model.release_unused_folded()
        # K14: WordPiece on the device for ASCII texts (identical ids; the host tokeniser stays the definition of record and
        # handles every other text).  MARQO_AMD_HOST_TOKENIZER=1 keeps everything on the host.
        self._device_tokenizer = None
        if isinstance(self._tokenizer, WordPieceTokenizer) and os.environ.get("MARQO_AMD_HOST_TOKENIZER", "0") != "1":
            from marqo_amd.engine.gpu_tokenizers import DeviceWordPieceTokenizer
            self._device_tokenizer = DeviceWordPieceTokenizer(self._tokenizer, self.device)
        elif isinstance(self._tokenizer, XlmRobertaTokenizer) and os.environ.get("MARQO_AMD_HOST_TOKENIZER", "0") != "1":
            from marqo_amd.engine.gpu_tokenizers import DeviceSentencePieceTokenizer
            try:   # unigram Viterbi on the device (multilingual-e5); models it cannot express (byte fallback ...) stay on the host
                self._device_tokenizer = DeviceSentencePieceTokenizer(self._tokenizer, self.device)
            except ValueError:
                self._device_tokenizer = None
        elif isinstance(self._tokenizer, RobertaBpeTokenizer) and os.environ.get("MARQO_AMD_HOST_TOKENIZER", "0") != "1":
            from marqo_amd.engine.gpu_tokenizers import DeviceByteBpeTokenizer
            try:   # byte-level BPE on the device; a vocabulary whose merges ids cannot express stays on the host
                self._device_tokenizer = DeviceByteBpeTokenizer(self._tokenizer, self.device)
            except ValueError:
                self._device_tokenizer = None

    def _load_modernbert(self, directory: str, arch, sd) -> None:
        """a transformers ModernBertModel checkpoint (model_type "modernbert"; no remote code in the reference either): host tokenisation by the
        `tokenizers` library from the directory's tokenizer.json, the tower of engine/modernbert.py.  bf16 operands only."""
        from marqo_amd.engine.modernbert import ModernBertTower
        from marqo_amd.engine.tokenizers import HfJsonTokenizer
        self._refuse_fp8("ModernBERT encoders (their rotary / gated-GELU blocks run on bf16 operands only)")
        self._check_width(arch.width)
        self._finish_packed(directory, arch, arch.max_pos, ModernBertTower, sd,
                            lambda: HfJsonTokenizer(directory, **self._special_tokens(directory, cls="[CLS]", sep="[SEP]", pad="[PAD]")))

    def _refuse_last_pooling(self) -> None:
        """'last' is the pooling of the decoder-style checkpoints only: every other family refuses it as the property parser did before it knew the word"""
        if self.model_properties.pooling_method == "last":
            raise InvalidModelPropertiesError(f"Invalid model properties: {self.model_properties.dict()}. Original error "
                                              f"{HuggingFaceModelProperties.POOLING_ERROR}")

    # ---- what the loaders of the packed-token families (ModernBERT, Qwen, Gemma, T5, JinaBERT, NomicBERT) share -------------------------------------
    def _refuse_fp8(self, family: str) -> None:
        props = self.model_properties
        if props.engine_precision == "fp8":
            raise InvalidModelPropertiesError(f"{props.name}: 'enginePrecision': 'fp8' is not available for {family}")

    def _check_width(self, width: int) -> None:
        props = self.model_properties
        if self._check_dimensions and width != props.dimensions:
            raise InvalidModelPropertiesError(f"'dimensions'={props.dimensions} but the encoder width is {width}")

    def _finish_packed(self, directory: str, arch, max_tokens: int, tower, sd, tokenizer, pooling: Optional[str] = None, **tower_args) -> None:
        """the tokenizer (`tokenizer()`: an HfJsonTokenizer), the truncation length, the pooling — None: the BERT rule (the property, 'last' refused, else
        1_Pooling/config.json, else mean) — and the tower; a ValueError / KeyError of either constructor (a tokenizer.json without the expected tokens, a
        missing / mis-shaped / unexpected tensor, a Dense module that does not fit) is the caller's InvalidModelPropertiesError.  These families have no
        GPU tokeniser (the byte-level BPE one does not implement their added-token handling)."""
        props = self.model_properties
        try:
            self._tokenizer = tokenizer()
        except ValueError as e:
            raise InvalidModelPropertiesError(f"{props.name}: {e}") from e
        props.tokens = min(props.tokens, max_tokens)
        if pooling is None:
            self._refuse_last_pooling()
            pooling = props.pooling_method or checkpoint.read_pooling_config(directory) or "mean"
        self.arch = arch
        self.weights_source = directory
        try:
            self._model = tower(arch, sd, self.device, pooling=pooling, precision=props.engine_precision, **tower_args)
        except (ValueError, KeyError) as e:
            raise InvalidModelPropertiesError(f"{props.name}: {e}") from e
        self._pooling_func = pooling
        self._device_tokenizer = None

    def _load_qwen(self, directory: str, arch, cfg: dict, sd) -> None:
        """a transformers Qwen3Model / Qwen2Model checkpoint (model_type "qwen3" / "qwen2": Qwen3-Embedding-0.6B, gte-Qwen2-1.5B-instruct ...; AutoModel in
        the reference): host tokenisation by the `tokenizers` library from the directory's tokenizer.json with the file's own post-processor, the tower
        of engine/qwen.py.  Pooling: the property, else 1_Pooling/config.json (last token / mean), else last token.  bf16 operands only."""
        from marqo_amd.engine.qwen import QwenTower
        self._load_decoder(directory, arch, cfg, sd, QwenTower, "Qwen3 / Qwen2 encoders")

    def _load_llama(self, directory: str, arch, cfg: dict, sd) -> None:
        """a transformers MistralModel / LlamaModel checkpoint (model_type "mistral" / "llama": e5-mistral-7b-instruct, SFR-Embedding-Mistral,
        Linq-Embed-Mistral ...; AutoModel in the reference), loaded as the Qwen checkpoints are: the file's own post-processor decides what is appended
        to a text (the </s> that e5-mistral's model card appends by hand is the caller's business unless tokenizer.json adds it), the tower of
        engine/llama.py.  Pooling: the property, else 1_Pooling/config.json (last token / mean), else last token.  bf16 operands only."""
        from marqo_amd.engine.llama import LlamaTower
        self._load_decoder(directory, arch, cfg, sd, LlamaTower, "Mistral / Llama encoders", pad_fallback="</s>")

    def _load_decoder(self, directory: str, arch, cfg: dict, sd, tower, family: str, **tokenizer_args) -> None:
        """what the decoder-style families share: fp8 refused, the width checked, last-token / mean pooling resolved, right-padded input truncated at
        min(tokens, max_position_embeddings, 8192); tokenizer_args: HfJsonTokenizer.plain's (the pad token to fall back to: a pad position never reaches a row)"""
        import json
        from marqo_amd.engine.tokenizers import HfJsonTokenizer
        props = self.model_properties
        self._refuse_fp8(f"{family} (their RMSNorm / rotary / gated-SiLU blocks run on bf16 operands only)")
        self._check_width(arch.width)
        pooling = props.pooling_method
        if pooling is None:
            try:
                with open(os.path.join(directory, "1_Pooling", "config.json")) as f:
                    pc = json.load(f)
            except (OSError, ValueError):
                pc = None
            if isinstance(pc, dict):
                pooling = "last" if pc.get("pooling_mode_lasttoken") is True else "mean" if pc.get("pooling_mode_mean_tokens") is True else None
        pooling = pooling or "last"
        if pooling not in ("last", "mean"):
            raise InvalidModelPropertiesError(f"{props.name}: pooling_method {pooling!r} is not available for {family} ('last' or 'mean')")
        self._finish_packed(directory, arch, min(int(cfg.get("max_position_embeddings", 8192)), 8192), tower, sd,
                            lambda: HfJsonTokenizer.plain(directory, **tokenizer_args), pooling=pooling)

    # sentence-transformers Dense module directories (relative to the checkpoint) to apply behind the pooling: set by the `sbert` loader for an
    # EmbeddingGemma or a T5 encoder pipeline, empty for `hf` (AutoModel in the reference: the bare encoder)
    _dense_modules = ()

    def _read_dense_modules(self, directory: str) -> list:
        try:
            return [self._read_dense_module(directory, d) for d in self._dense_modules]
        except (OSError, ValueError, KeyError) as e:
            raise InvalidModelPropertiesError(f"{self.model_properties.name}: {e}") from e

    def _load_t5(self, directory: str, arch, sd) -> None:
        """a transformers T5EncoderModel checkpoint (model_type "t5": sentence-t5, gtr-t5, flan-t5 / T5 v1.1 encoder fine-tunes; the decoder tensors of a
        full T5 checkpoint are ignored): host tokenisation by the `tokenizers` library from the directory's tokenizer.json with the file's own
        post-processor (which appends </s>), right-padded with the file's <pad>, truncated at min(tokens, sentence_bert_config.json max_seq_length, 8192);
        the tower of engine/t5.py.  Pooling: the property, else 1_Pooling/config.json, else mean.  bf16 operands only."""
        import json
        from marqo_amd.engine.t5 import T5Tower
        from marqo_amd.engine.tokenizers import HfJsonTokenizer
        self._refuse_fp8("T5 encoders (their RMSNorm / relative-bias attention blocks run on bf16 operands only)")
        dense = self._read_dense_modules(directory)
        self._check_width(dense[-1].shape[0] if dense else arch.width)
        cap = arch.max_pos
        try:
            with open(os.path.join(directory, "sentence_bert_config.json")) as f:
                st_len = json.load(f).get("max_seq_length")
            if isinstance(st_len, int) and st_len >= 1:
                cap = min(cap, st_len)
        except (OSError, ValueError, AttributeError):
            pass
        self._finish_packed(directory, arch, cap, T5Tower, sd, lambda: HfJsonTokenizer.plain(directory, pad_fallback="<pad>"), dense=dense)

    def _load_jina_bert(self, directory: str, arch, sd) -> None:
        """a JinaBERT checkpoint (model_type "bert" with position_embedding_type "alibi": jina-embeddings-v2-small-en / -base-en and their fine-tunes;
        custom remote code to the reference's AutoModel, so refused unless trustRemoteCode is set): host tokenisation by the `tokenizers` library from the
        directory's tokenizer.json with the file's own post-processor ([CLS] ... [SEP]), right-padded with [PAD], truncated at min(tokens,
        max_position_embeddings, 8192); the tower of engine/jina_bert.py.  Pooling: the property, else 1_Pooling/config.json, else mean.  bf16 operands
        only; no GPU tokeniser and no native request queue for this family."""
        from marqo_amd.engine.jina_bert import JinaBertTower
        from marqo_amd.engine.tokenizers import HfJsonTokenizer
        props = self.model_properties
        if not props.trust_remote_code:
            raise InvalidModelPropertiesError(f"{props.name} is a custom-code (JinaBERT) checkpoint: the reference loads it only with "
                                              f"'trustRemoteCode': True")
        self._refuse_fp8("JinaBERT encoders (their ALiBi attention / gated-GELU blocks run on bf16 operands only)")
        self._check_width(arch.width)
        self._finish_packed(directory, arch, arch.max_pos, JinaBertTower, sd, lambda: HfJsonTokenizer.plain(directory, pad_fallback="[PAD]"))

    def _load_nomic_bert(self, directory: str, arch, sd) -> None:
        """a NomicBERT checkpoint (model_type "nomic_bert": nomic-embed-text-v1 / -v1.5 / -v1-unsupervised, snowflake-arctic-embed-m-long and their
        fine-tunes, in transformers' tensor names or the hub's original ones; native in transformers, so trustRemoteCode is not required — it is accepted
        and ignored): host tokenisation by the `tokenizers` library from the directory's tokenizer.json with the file's own post-processor
        ([CLS] ... [SEP]), right-padded with [PAD], truncated at min(tokens, max_position_embeddings, 8192); the tower of engine/nomic_bert.py.  Pooling:
        the property, else 1_Pooling/config.json, else mean.  The search_query: / search_document: prefixes are the caller's text_query_prefix /
        text_chunk_prefix; v1.5's Matryoshka truncation is not applied (the full vector is returned).  bf16 operands only; no GPU tokeniser and no
        native request queue for this family."""
        from marqo_amd.engine.nomic_bert import NomicBertTower
        from marqo_amd.engine.tokenizers import HfJsonTokenizer
        self._refuse_fp8("NomicBERT encoders (their rotary / gated-SiLU blocks run on bf16 operands only)")
        self._check_width(arch.width)
        self._finish_packed(directory, arch, arch.max_pos, NomicBertTower, sd, lambda: HfJsonTokenizer.plain(directory, pad_fallback="[PAD]"))

    def _load_jina_v3(self, directory: str, arch, sd) -> None:
        """a Jina v3 checkpoint in transformers' own form (model_type "jina_embeddings_v3": jinaai/jina-embeddings-v3-hf; native in transformers, so
        trustRemoteCode is not required — it is accepted and ignored): host tokenisation by the `tokenizers` library from the directory's tokenizer.json
        with the file's own post-processor (<s> ... </s>), right-padded with <pad>, truncated at min(tokens, max_position_embeddings - 2, 8192); the tower
        of engine/jina_v3.py.  Pooling: the property, else 1_Pooling/config.json, else mean.  Task adapters: every sub-directory of the checkpoint with
        adapter_config.json + adapter_model.safetensors (PEFT's layout), and the directories of 'loraAdapters'; the task is the directory's name / the
        dict's key.  'loraTask' selects the adapter of every text (encode(..., task=...) overrides it per call); with neither the base model runs.  The
        Matryoshka truncation of the model card is not applied (the full vector is returned).  bf16 operands only; no GPU tokeniser and no native
        request queue for this family."""
        from marqo_amd.engine import jina_v3
        from marqo_amd.engine.tokenizers import HfJsonTokenizer
        props = self.model_properties
        self._refuse_fp8("Jina v3 encoders (their rotary blocks and LoRA corrections run on bf16 operands only)")
        self._check_width(arch.width)
        dirs = jina_v3.find_adapter_dirs(directory)
        dirs.update(props.lora_adapters or {})
        try:
            adapters = jina_v3.load_adapters(arch, dirs)
        except (ValueError, OSError) as e:
            raise InvalidModelPropertiesError(f"{props.name}: {e}") from e
        self._finish_packed(directory, arch, arch.max_pos, jina_v3.JinaV3Tower, sd, lambda: HfJsonTokenizer.plain(directory, pad_fallback="<pad>"),
                            adapters=adapters, default_task=props.lora_task)

    def _load_gemma(self, directory: str, arch, sd) -> None:
        """a transformers Gemma3TextModel checkpoint with use_bidirectional_attention (model_type "gemma3_text": google/embeddinggemma-300m and its
        fine-tunes; AutoModel in the reference): host tokenisation by the `tokenizers` library from the directory's tokenizer.json with the file's own
        post-processor (<bos> ... <eos>), right-padded, truncated at min(tokens, max_position_embeddings); the tower of engine/gemma.py.  Pooling: the
        property, else 1_Pooling/config.json, else mean.  The task prompts of the model card stay the caller's text_query_prefix / text_chunk_prefix.
        bf16 operands only."""
        from marqo_amd.engine.gemma import GemmaTower
        from marqo_amd.engine.tokenizers import HfJsonTokenizer
        self._refuse_fp8("EmbeddingGemma encoders (their RMSNorm / rotary / gated tanh-GELU blocks run on bf16 operands only)")
        dense = self._read_dense_modules(directory)
        self._check_width(dense[-1].shape[0] if dense else arch.width)
        self._finish_packed(directory, arch, arch.max_pos, GemmaTower, sd, lambda: HfJsonTokenizer.plain(directory, pad_fallback="<pad>"), dense=dense)

    @staticmethod
    def _read_dense_module(directory: str, sub: str):
        """one sentence-transformers Dense module directory -> its weight [out, in]; a bias or a non-identity activation is refused (ValueError)"""
        import json
        from safetensors.torch import load_file
        d = os.path.join(directory, sub)
        with open(os.path.join(d, "config.json")) as f:
            dc = json.load(f)
        act = str(dc.get("activation_function", "torch.nn.modules.linear.Identity"))
        if dc.get("bias", False):
            raise ValueError(f"Dense module {sub} has a bias: only bias-free Dense modules with identity activation are served")
        if not act.endswith("Identity"):
            raise ValueError(f"Dense module {sub} has activation {act}: only bias-free Dense modules with identity activation are served")
        t = load_file(os.path.join(d, "model.safetensors"))
        if "linear.bias" in t:
            raise ValueError(f"Dense module {sub} has a bias: only bias-free Dense modules with identity activation are served")
        if "linear.weight" not in t:
            raise KeyError(f"Dense module {sub}: model.safetensors has no 'linear.weight'")
        w = t["linear.weight"]
        if tuple(w.shape) != (int(dc.get("out_features", w.shape[0])), int(dc.get("in_features", w.shape[1]))):
            raise ValueError(f"Dense module {sub}: linear.weight {tuple(w.shape)} does not match its config.json")
        return w

    @staticmethod
    def _adds_prefix_space(directory: str) -> bool:
        import json
        p = os.path.join(directory, "tokenizer_config.json")
        if os.path.isfile(p):
            try:
                with open(p) as f:
                    return bool(json.load(f).get("add_prefix_space", False))
            except (OSError, ValueError, AttributeError):
                pass
        return False

    @staticmethod
    def _special_tokens(directory: str, **defaults) -> dict:
        """unk / cls / sep / pad / mask spellings of a checkpoint (tokenizer_config.json, then special_tokens_map.json), else the family's"""
        import json
        out = dict(defaults)
        for name in ("special_tokens_map.json", "tokenizer_config.json"):
            p = os.path.join(directory, name)
            if not os.path.isfile(p):
                continue
            try:
                with open(p) as f:
                    j = json.load(f)
            except (OSError, ValueError):
                continue
            for k in out:
                v = j.get(k + "_token")
                if isinstance(v, dict):   # AddedToken serialisation
                    v = v.get("content")
                if isinstance(v, str) and v:
                    out[k] = v
        return out

    @staticmethod
    def _do_lower_case(directory: str) -> bool:
        import json
        for name in ("tokenizer_config.json",):
            p = os.path.join(directory, name)
            if os.path.isfile(p):
                try:
                    with open(p) as f:
                        return bool(json.load(f).get("do_lower_case", True))
                except (OSError, ValueError):
                    pass
        return True

    def native_queue_takes(self, texts) -> bool:
        """True when `encode(texts)` goes through the tower's native request queue (engine/native_queue.py): `vectorise()` then leaves the merging
        of concurrent calls to it instead of the Python coalescer (host-tokenised small calls only)"""
        from marqo_amd.engine import native_queue as NQ
        if not NQ.ENABLED or self._model is None or not hasattr(self._model, "_small_call"):
            return False
        texts = [texts] if isinstance(texts, str) else texts
        if not (1 <= len(texts) <= NQ.MAX_SEQS) or not all(isinstance(t, str) for t in texts):
            return False
        return getattr(self, "_device_tokenizer", None) is None or prefers_host(texts)

    def encode(self, sentence: Union[str, List[str]], normalize=True, **kwargs) -> np.ndarray:
        """-> np.ndarray [n, D] fp32 (hugging_face_model.py:172-203); engine extension `return_device=True`: the same rows as a device
        tensor.  Other kwargs the callers pass (`modality`, `infer`, `image_download_headers`) are tolerated and ignored."""
        if isinstance(sentence, str):
            sentence = [sentence]
        if self._model is None:
            self.load()
        return_device = bool(kwargs.get("return_device", False))
        tok = None
        if not return_device and self.native_queue_takes(sentence):
            # a request thread's small call: tokenise here, hand the ids to the tower's native queue, block outside the interpreter; a LONE single
            # query comes back None and replays its captured graph below (with the ids made here)
            tok = self._tokenizer(sentence, max_length=self.model_properties.tokens)
            rows = self._model.queue_rows_ids(tok["input_ids"], tok["attention_mask"], bool(normalize))
            if rows is not None:
                return rows
        with request_stream(self.device, device_output=return_device):
            if tok is None and getattr(self, "_device_tokenizer", None) is not None and not prefers_host(sentence):
                d_ids, lens = self._device_tokenizer.encode_device(sentence, self.model_properties.tokens)
                out = self._model.encode_device(d_ids, lens, normalize=bool(normalize))
            else:
                if tok is None:
                    tok = self._tokenizer(sentence, max_length=self.model_properties.tokens)
                ids, mask = torch.from_numpy(tok["input_ids"]), torch.from_numpy(tok["attention_mask"])
                if kwargs.get("task") is not None:   # one task adapter for this call's texts (Jina v3; any other family has no adapters to name)
                    if not hasattr(self._model, "task_ids"):
                        raise InvalidModelPropertiesError(f"{self.model_properties.name}: encode(task={kwargs['task']!r}) needs a checkpoint with LoRA task "
                                                          f"adapters (model_type jina_embeddings_v3)")
                    try:
                        out = self._model.encode(ids, mask, [kwargs["task"]] * len(sentence), normalize=bool(normalize))
                    except ValueError as e:   # an unknown task name
                        raise InvalidModelPropertiesError(f"{self.model_properties.name}: {e}") from e
                else:
                    out = self._model.encode_ids(ids, mask, normalize=bool(normalize))
            return out if return_device else out.cpu().numpy()


class HuggingFaceStellaModel(HuggingFaceModel):
    """hf_stella (hugging_face_stella_model.py:9-23): the reference loads `Marqo/dunzhang-stella_en_400M_v5` through
    AutoModel(trust_remote_code=True, use_memory_efficient_attention=False, unpad_inputs=False) — Alibaba-NLP's `NewModel` encoder
    (rotary positions, packed qkv, gated-GELU MLP, post-LN) — and keeps HuggingFaceModel.encode as is: tokenizer -> last_hidden_state
    -> mean pooling -> F.normalize (the sentence-transformers `2_Dense` head is NOT applied: AutoModel returns the bare encoder, and
    the registry's 1024 dimensions are its hidden size).  The engine runs that encoder natively (engine/towers.py::BertTower with
    BertArch.glu / rope_theta; kernels rope_kernel / glu_kernel): no remote code is executed, `trustRemoteCode` is only validated like
    the reference validates it."""
    _requires_trust_remote_code = True

"""`ReRankerText`: scores every (query, chunk of a field) pair of a search result with a cross-encoder and keeps the best chunks per hit.
`ReRankerOwl`: scores every hit's image against the query with OWL-ViT and keeps the best boxes per hit.

The reference (s2_inference/reranking/cross_encoders.py:224-338, model_utils.py:242-273) does this on pandas frames around a
sentence-transformers `CrossEncoder`; here the bookkeeping is plain Python (the product does not import pandas) with the same observable
behaviour, and the scores come from engine/rerank.py CrossEncoderTower (csrc/rerank.hip) with sigmoid as the activation, which is what the
reference always constructs its CrossEncoder with.  The image reranker (cross_encoders.py:341-461, model_utils.py:305-430) runs transformers'
OwlViTForObjectDetection one image at a time there; here all images of a search go through engine/owl.py OwlTower (csrc/owl_head.hip) at once.
"""
from __future__ import annotations

import datetime
import functools
import logging
import math
import os
import threading
import uuid
from collections import defaultdict
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

from marqo_amd.s2_inference.enums import AvailableModelsKey
from marqo_amd.s2_inference.errors import RerankerError, RerankerNameError
from marqo_amd.s2_inference.processing import image as image_processor
from marqo_amd.s2_inference.processing import text as text_processor
from marqo_amd.s2_inference.reranking.configs import get_default_text_processing_parameters
from marqo_amd.s2_inference.reranking.enums import Columns, ResultsFields

logger = logging.getLogger(__name__)

_load_lock = threading.Lock()


# ---- models --------------------------------------------------------------------------------------------------------------------------
class DummyModel:
    """'_testing': uniform random scores, as the reference's DummyModel"""

    def predict(self, inputs: Sequence) -> np.ndarray:
        return np.random.rand(len(inputs))


class EngineCrossEncoder:
    """predict() of sentence-transformers' CrossEncoder on the engine: [[query, passage], ...] -> sigmoid(logit) fp32 [n]"""

    def __init__(self, directory: str, device: str, max_length: int = 512):
        from marqo_amd.engine.rerank import load_cross_encoder_tower
        self.tower = load_cross_encoder_tower(directory, device)     # (by the directory's model_type: BERT-family towers, the DeBERTa, the Qwen3 or the Gemma tower)
        # (model_utils.py:266-270: a max_length above the tokenizer's model_max_length is lowered to it)
        self.max_length = min(int(max_length), self.tower.model_max_length)
        self.weights_source = directory

    def predict(self, inputs: Sequence[Sequence[str]], instruction: Optional[str] = None) -> np.ndarray:
        """`instruction`: the task description of an instruction-following reranker (the Qwen3 rerankers; the Gemma rerankers' prompt; None = the tower's default).  A tower
        whose template has no instruction refuses one."""
        kw = {}
        if instruction is not None:
            if not hasattr(self.tower, "instruction"):
                raise ValueError(f"{type(self.tower).__name__} takes no instruction (only the Qwen3 and Gemma rerankers do)")
            kw["instruction"] = instruction
        scores = np.zeros(len(inputs), dtype=np.float32)
        by_query: Dict[str, List[int]] = {}
        for i, pair in enumerate(inputs):
            if len(pair) != 2 or not isinstance(pair[0], str) or not isinstance(pair[1], str):
                raise TypeError(f"expected [query, text] pairs of strings, found {pair!r}")
            by_query.setdefault(pair[0], []).append(i)
        for query, idx in by_query.items():       # (one query per search: one pass)
            scores[idx] = self.tower.score(query, [inputs[i][1] for i in idx], self.max_length, **kw)[1]
        return scores


def _checkpoint_candidates(name: str) -> List[str]:
    from marqo_amd.engine import checkpoint
    return [name, os.path.join(checkpoint.model_dir(), "hf", *name.split("/")), os.path.join(checkpoint.model_dir(), *name.split("/")),
            *checkpoint._hub_cache_dirs(name)]


def load_cross_encoder_model(model_name: str, device: str, max_length: int = 512) -> Dict[str, Any]:
    """the reference's load_sbert_cross_encoder_model: the model lives in the model cache under _create_model_cache_key(model_name, device),
    so LRU ejection and get_loaded_models cover it.  The checkpoint is looked up where HuggingFaceModel looks `name` up; never downloaded."""
    from marqo_amd.engine import checkpoint
    from marqo_amd.s2_inference.s2_inference import _create_model_cache_key, get_available_models
    key = _create_model_cache_key(model_name, device)
    models = get_available_models()
    entry = models.get(key)
    if entry is None:
        with _load_lock:
            entry = models.get(key)
            if entry is None:
                logger.info(f"loading {model_name} on device {device} and adding to cache...")
                if model_name == "_testing":
                    model = DummyModel()
                elif model_name.startswith("onnx/"):
                    raise RerankerError(f"{model_name}: the 'onnx/' prefix (optimum / onnxruntime cross-encoders) is not served by the marqo_amd "
                                        f"engine; name the Hugging Face checkpoint itself")
                else:
                    directory = checkpoint.find_hf_dir(model_name)
                    if directory is None:
                        raise RerankerError(f"no local checkpoint for the reranker {model_name}: looked for config.json + model.safetensors | "
                                            f"pytorch_model.bin under {_checkpoint_candidates(model_name)} (the marqo_amd engine never downloads)")
                    try:
                        model = EngineCrossEncoder(directory, device, max_length)
                    except (ValueError, KeyError, FileNotFoundError) as e:
                        raise RerankerError(f"cannot load the reranker {model_name} from {directory}: {e}") from e
                entry = models[key] = {AvailableModelsKey.model: model, AvailableModelsKey.most_recently_used_time: datetime.datetime.now()}
    else:
        entry[AvailableModelsKey.most_recently_used_time] = datetime.datetime.now()
    return {"model": entry[AvailableModelsKey.model]}


# ---- result bookkeeping -------------------------------------------------------------------------------------------------------------------
def _is_missing(v: Any) -> bool:
    """a field a hit does not hold, or holds as None / NaN (what a frame built from the hits would show as NA)"""
    return v is None or (isinstance(v, float) and math.isnan(v))


class FormattedResults:
    """the hits as rows for the model: every hit gets its `_rerank_id` (`_id`, or a fresh uuid); with `searchable_fields` given as a list
    only the hits that hold all of them are kept; `searchable_fields` ends up as the hits' own field names (those not starting with '_')
    in order of first appearance"""

    def __init__(self, results: Dict, searchable_fields: Optional[List[str]] = None):
        self.results = results
        for hit in results[ResultsFields.hits]:
            hit[ResultsFields.reranked_id] = hit[ResultsFields.id] if ResultsFields.id in hit else str(uuid.uuid4())
        if searchable_fields is not None and isinstance(searchable_fields, list):
            results[ResultsFields.hits] = [h for h in results[ResultsFields.hits] if all(s in h for s in searchable_fields)]
        self.columns: List[str] = list(dict.fromkeys(k for hit in results[ResultsFields.hits] for k in hit))
        self.searchable_fields = [c for c in self.columns if not c.startswith("_")]

    def format_for_model(self, searchable_fields: List[str], query: Optional[str] = None) -> List[Dict[str, Any]]:
        """one row per (field, hit) whose content is there, field by field"""
        rows = []
        for field in searchable_fields:
            if field not in self.columns:
                raise KeyError(f"field {field!r} is in none of the hits")
            for hit in self.results[ResultsFields.hits]:
                content = hit.get(field)
                if _is_missing(content):
                    continue
                rows.append({Columns.query: query, Columns.field_content: content, ResultsFields.reranked_id: hit[ResultsFields.reranked_id],
                             Columns.original_field_name: field, ResultsFields.original_score: hit.get(ResultsFields.original_score, 1.0)})
        return rows


class ReRanker:
    def __init__(self):
        self.results = None
        self.formatted_results = None
        self.inputs: List[Dict[str, Any]] = []
        self.num_highlights = 1

    def load_model(self):
        pass

    def format_results(self, results: Dict, query: Optional[str] = None, searchable_fields: Optional[List[str]] = None):
        self.results = results
        self.formatted_results = FormattedResults(results, searchable_fields=searchable_fields)

    @staticmethod
    def _prepare_inputs(rows: List[Dict[str, Any]]) -> List[List[str]]:
        return [[r[Columns.query], r[Columns.field_content]] for r in rows]

    def get_reranked_results(self, score_column: str = ResultsFields.reranker_score, highlight_content_column: str = Columns.field_content):
        """per hit the `num_highlights` best rows -> `_reranked_score` (a number, or a list of them from 2 highlights on) and
        `_reranked_highlights` ([{field: chunk}, ...]); then the hits in descending order of that score"""
        groups: Dict[Any, List[Dict[str, Any]]] = defaultdict(list)
        for row in self.inputs:
            groups[row[ResultsFields.reranked_id]].append(row)
        top = {rid: sorted(rows, key=lambda r: r[score_column], reverse=True)[:self.num_highlights] for rid, rows in groups.items()}
        for hit in self.results[ResultsFields.hits]:
            rid = hit[ResultsFields.reranked_id]
            if rid not in top:
                raise KeyError(f"hit {rid!r} has nothing to score in the searchable fields")
            best = top[rid]
            if self.num_highlights == 1:
                hit[ResultsFields.reranker_score] = best[0][score_column]
                hit[ResultsFields.highlights_reranked] = [{best[0][Columns.original_field_name]: best[0][highlight_content_column]}]
            else:
                if len(best) < 2:   # (the reference fails here too: it asks a single score for its `.values`)
                    raise ValueError(f"hit {rid!r} has one scored chunk, {self.num_highlights} highlights were asked for")
                hit[ResultsFields.reranker_score] = [r[score_column] for r in best]
                hit[ResultsFields.highlights_reranked] = [{r[Columns.original_field_name]: r[highlight_content_column]} for r in best]
        self.results[ResultsFields.hits] = sorted(self.results[ResultsFields.hits], key=lambda h: h[ResultsFields.reranker_score], reverse=True)


class ReRankerText(ReRanker):
    """reranking with a Hugging Face cross-encoder (Bert / XLMRoberta / Roberta / ModernBert / DebertaV2 ForSequenceClassification with one logit) or
    a Qwen3 reranker (Qwen3ForCausalLM judged by yes / no, or its one-logit conversion) or a Gemma reranker (GemmaForCausalLM judged by `Yes`, or its
    one-logit conversion); `instruction` (the Qwen3 and Gemma rerankers only) replaces the template's default task description / prompt"""

    def __init__(self, model_name: str, device: str, max_length: int = 512, num_highlights: int = 1,
                 split_params: Optional[Dict] = get_default_text_processing_parameters(), instruction: Optional[str] = None):
        super().__init__()
        self.instruction = instruction
        self.model_name = model_name
        self.device = device
        self.max_length = max_length
        self.num_highlights = num_highlights
        self.split_params = split_params
        self.model = None
        self.split_length = self.split_overlap = self.split_method = None
        if isinstance(split_params, (dict, defaultdict)):
            self.split_length, self.split_overlap, self.split_method = (split_params[k] for k in ("split_length", "split_overlap", "split_method"))

    def load_model(self) -> None:
        self.model = load_cross_encoder_model(model_name=self.model_name, device=self.device, max_length=self.max_length)["model"]

    def explode_nested_content_field(self, rows: List[Dict[str, Any]]) -> List[Dict[str, Any]]:
        """one row per chunk of a row's content (chunked as indexing chunks text), the unchunked text kept beside it"""
        out = []
        for row in rows:
            chunks = text_processor.split_text(row[Columns.field_content], split_length=self.split_length, split_overlap=self.split_overlap,
                                               split_by=self.split_method)
            for chunk in chunks if len(chunks) else [None]:
                out.append({**row, Columns.field_content: chunk, Columns.field_content_original: row[Columns.field_content]})
        return out

    def rerank(self, query: str, results: Dict, searchable_attributes: Optional[List[str]] = None) -> None:
        self.results = results
        self.searchable_attributes = searchable_attributes
        if not isinstance(results, (dict, defaultdict)):
            raise TypeError(f"expected a dict or defaultdict, received {type(results)}")
        if len(results[ResultsFields.hits]) == 0:
            logger.warning("empty results for re-ranking. returning doing nothing...")
            return
        if self.model is None:
            self.load_model()
        self.format_results(results)
        if self.searchable_attributes is None:
            self.searchable_attributes = self.formatted_results.searchable_fields
        self.inputs = self.formatted_results.format_for_model(self.searchable_attributes, query=query)
        if self.split_params is not None:
            n = len(self.inputs)
            self.inputs = self.explode_nested_content_field(self.inputs)
            logger.info(f"chunking field content, went from length {n} to {len(self.inputs)}")
        self.model_inputs = self._prepare_inputs(self.inputs)
        extra = {} if self.instruction is None else {"instruction": self.instruction}
        self.scores = [float(s) for s in np.asarray(self.model.predict(self.model_inputs, **extra)).reshape(-1)]
        if len(self.scores) != len(self.inputs):
            raise RuntimeError(f"the model returned {len(self.scores)} scores for {len(self.inputs)} pairs")
        for row, s in zip(self.inputs, self.scores):
            row[ResultsFields.reranker_score] = s
            orig = row[ResultsFields.original_score]
            if isinstance(orig, (int, float)):    # kept for a hybrid ranking, as in the reference; nothing reads them yet
                row[ResultsFields.hybrid_score_multiply] = max(orig, 1e-3) * max(s, 1e-3)
                row[ResultsFields.hybrid_score_add] = orig + s
        self.get_reranked_results()


# ---- image reranking: OWL-ViT -------------------------------------------------------------------------------------------------------------------
OWL_MODEL_MAP = {
    "google/owlvit-base-patch32": "google/owlvit-base-patch32",
    "google/owlvit-base-patch16": "google/owlvit-base-patch16",
    "google/owlvit-large-patch14": "google/owlvit-large-patch14",
    "owl/ViT-B/32": "google/owlvit-base-patch32",
    "owl/ViT-B/16": "google/owlvit-base-patch16",
    "owl/ViT-L/14": "google/owlvit-large-patch14",
}


def load_owl_vit(model_name: str, device: str) -> Dict[str, Any]:
    """the reference's load_owl_vit for a mapped `google/owlvit-*` name: the tower lives in the model cache under
    _create_model_cache_key(model_name, device); its checkpoint is looked up where HuggingFaceModel looks a name up, never downloaded"""
    from marqo_amd.engine import checkpoint
    from marqo_amd.s2_inference.s2_inference import _create_model_cache_key, get_available_models
    key = _create_model_cache_key(model_name, device)
    models = get_available_models()
    entry = models.get(key)
    if entry is None:
        with _load_lock:
            entry = models.get(key)
            if entry is None:
                logger.info(f"loading {model_name} on device {device} and adding to cache...")
                directory = checkpoint.find_hf_dir(model_name)
                if directory is None:
                    raise RerankerError(f"{model_name}: the OWL-ViT image reranker is not served without a local checkpoint: looked for config.json + "
                                        f"model.safetensors | pytorch_model.bin under {_checkpoint_candidates(model_name)} (the marqo_amd engine "
                                        f"never downloads)")
                from marqo_amd.engine.owl import OwlTower
                try:
                    model = OwlTower.from_dir(directory, device, name=model_name)
                except (ValueError, KeyError, FileNotFoundError) as e:
                    raise RerankerError(f"cannot load the image reranker {model_name} from {directory}: {e}") from e
                entry = models[key] = {AvailableModelsKey.model: model, AvailableModelsKey.most_recently_used_time: datetime.datetime.now()}
    else:
        entry[AvailableModelsKey.most_recently_used_time] = datetime.datetime.now()
    return {"model": entry[AvailableModelsKey.model]}


@functools.lru_cache
def _load_image(filename: str, size: Optional[Tuple[int, int]] = None):
    """(the working image, its original size); cached by (pointer, size) as in the reference"""
    from marqo_amd.s2_inference.image_input import load_image_from_path
    im = load_image_from_path(filename, {})
    original_size = im.size
    if size is not None:
        im = im.resize(size).convert("RGB")
    return im, original_size


class ReRankerOwl(ReRanker):
    """reranking of image fields with OWL-ViT: a hit's score is the score of its image's best box for the query, its highlight that box in
    the pixels of the original image"""

    def __init__(self, model_name: str, device: str, image_size: Tuple[int, int]):
        super().__init__()
        self.model_name = model_name
        self.device = device
        self.image_size = image_size
        self.model = None
        self.image_attributes = None
        self.num_highlights = None
        self._model_map = dict(OWL_MODEL_MAP)
        if self.model_name not in self._model_map:
            raise RerankerNameError(f"could not find model_name={self.model_name} in mappings {list(self._model_map.keys())}")

    def load_model(self) -> None:
        self._remapped_name = self._model_map[self.model_name]
        logger.info(f"loading model={self._remapped_name} from input name={self.model_name} to device {self.device}")
        self.model = load_owl_vit(self._remapped_name, device=self.device)["model"]

    @staticmethod
    def load_images(content: Sequence[str], size: Tuple[int, int]):
        """-> (working images, original sizes), through the loader every image model uses"""
        if not len(content):
            return (), ()
        images, original_size = zip(*[_load_image(f, size=size) for f in content])
        return images, original_size

    def rerank(self, query: str, results: Dict, image_attributes: List, num_highlights: int = 1) -> None:
        self.results = results
        self.image_attributes = image_attributes
        self.num_highlights = num_highlights
        if not isinstance(results, (dict, defaultdict)):
            raise TypeError(f"expected a dict or defaultdict, received {type(results)}")
        if len(results[ResultsFields.hits]) == 0:
            logger.warning("empty results for re-ranking. returning doing nothing...")
            return
        if self.model is None:
            self.load_model()
        self.format_results(results, searchable_fields=image_attributes)
        self.inputs = self.formatted_results.format_for_model(self.image_attributes, query=query)
        self.model_inputs = self._prepare_inputs(self.inputs)
        image_names = [pair[1] for pair in self.model_inputs]
        self.images, self.original_sizes = self.load_images(image_names, self.image_size)
        # every image of the search in one detect(): scores [n, k], boxes [n, k, 4] in the working image's pixels, best first
        pixels = np.stack([np.asarray(im, dtype=np.uint8) for im in self.images]) if len(self.images) else np.zeros((0, *self.image_size[::-1], 3), np.uint8)
        try:
            scores, boxes, _ = self.model.detect(query, pixels, k=num_highlights, target_size=self.image_size)
        except ValueError as e:        # (a query beyond the model's 16 positions)
            raise RerankerError(str(e)) from e
        boxes_scores = []
        for i, (content, orig_size) in enumerate(zip(image_names, self.original_sizes)):
            for j in range(scores.shape[1]):
                box = [float(v) for v in boxes[i, j]]
                boxes_scores.append({Columns.bbox: box, ResultsFields.reranker_score: float(scores[i, j]), Columns.field_content: content,
                                     Columns.bbox_original: list(image_processor.rescale_box(box, self.image_size, orig_size))})
        # merged back by the image pointer, as the reference's frame merge does: a box row meets every hit row with its image, so two hits that
        # share an image each see that image's rows once per hit
        by_content: Dict[Any, List[Dict[str, Any]]] = defaultdict(list)
        for row in self.inputs:
            by_content[row[Columns.field_content]].append(row)
        self.inputs = [{**row, **bs} for bs in boxes_scores for row in by_content[bs[Columns.field_content]]]
        self.get_reranked_results(highlight_content_column=Columns.bbox_original)

"""Entry point of reranking: `rerank_search_results` rescoring a search result in place with a text cross-encoder or, for the `owl` names,
with OWL-ViT on the hits' images (the reference's s2_inference/reranking/rerank.py, called from tensor_search.search(..., reranker=...))."""
from __future__ import annotations

import logging
from typing import Dict, List, Optional

from PIL import UnidentifiedImageError

from marqo_amd.s2_inference.errors import RerankerError, RerankerNameError
from marqo_amd.s2_inference.reranking.cross_encoders import ReRankerOwl, ReRankerText
from marqo_amd.s2_inference.reranking.enums import ResultsFields

logger = logging.getLogger(__name__)


def rerank_search_results(search_result: Dict, query: str, model_name: str, device: str, searchable_attributes: Optional[List[str]] = None,
                          num_highlights: int = 1, overwrite_original_scores_highlights: bool = True) -> None:
    """Rescore the hits of `search_result` against `query` and reorder them, in place.  A result none of whose hits holds any of the
    searchable attributes is handed back untouched.  A name containing 'owl' runs OWL-ViT detection over the image field named by the first
    searchable attribute: a hit's score is its best box's, its highlight that box in the original image's pixels (one box per hit: as in the
    reference, `num_highlights` does not reach the image reranker).  The 'onnx/' prefix is refused."""
    owl = "owl" in model_name.lower()
    # the image reranker needs the image's location: one field, named by the caller.  (Judged in front of the field check, so that every empty
    # form is refused; the reference's field check hands an empty LIST back untouched before its own refusal is reached.)
    if owl and searchable_attributes in (None, [], (), ""):
        raise RerankerError(message=f"found searchable_attributes={searchable_attributes} but expected list of strings for {model_name}")
    if not _check_searchable_fields_in_results(search_results=search_result, searchable_fields=searchable_attributes):
        return search_result
    if owl:
        if len(searchable_attributes) > 1:
            logger.info(f"currently only a single attribute can be reranked over for {model_name}. taking the first field "
                        f"{[searchable_attributes[0]]} from {searchable_attributes}")
            searchable_attributes = [searchable_attributes[0]]
        try:
            reranker = ReRankerOwl(model_name=model_name, device=device, image_size=(240, 240))
            reranker.rerank(query=query, results=search_result, image_attributes=searchable_attributes)
        except (UnidentifiedImageError, RerankerNameError) as e:
            raise RerankerError(message=str(e)) from e
        if overwrite_original_scores_highlights:
            cleanup_final_reranked_results(search_result)
        return
    if model_name.startswith("onnx/"):
        raise RerankerError(message=f"{model_name}: the 'onnx/' prefix is not served by the marqo_amd engine; name the Hugging Face "
                                    f"cross-encoder checkpoint itself")
    try:
        reranker = ReRankerText(model_name=model_name, device=device, num_highlights=num_highlights)
        reranker.rerank(query=query, results=search_result, searchable_attributes=searchable_attributes)
    except Exception as e:
        raise RerankerError(message=str(e)) from e
    if overwrite_original_scores_highlights:
        cleanup_final_reranked_results(search_result)


def _check_searchable_fields_in_results(search_results: Dict, searchable_fields: Optional[List[str]] = None) -> bool:
    """True when there is something to rerank: no attribute list at all, or at least one hit that holds one of the listed fields"""
    if searchable_fields is None:
        return True
    return any(any(field in hit for field in searchable_fields) for hit in search_results[ResultsFields.hits])


def cleanup_final_reranked_results(reranked_results: Dict) -> None:
    """fold what reranking wrote into the hits' public keys: `_score` and `_highlights` take the reranked values, the working keys go"""
    for hit in reranked_results[ResultsFields.hits]:
        if ResultsFields.reranker_score in hit:
            hit[ResultsFields.original_score] = hit.pop(ResultsFields.reranker_score)
        if ResultsFields.highlights_reranked in hit:
            hit[ResultsFields.highlights] = hit.pop(ResultsFields.highlights_reranked)
        hit.pop(ResultsFields.reranked_id, None)

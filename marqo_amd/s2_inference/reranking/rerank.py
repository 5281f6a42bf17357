"""Entry point of reranking: `rerank_search_results` rescoring a search result in place with a cross-encoder
(the reference's s2_inference/reranking/rerank.py, called from tensor_search.search(..., reranker=...))."""
from __future__ import annotations

from typing import Dict, List, Optional

from marqo_amd.s2_inference.errors import RerankerError, RerankerNameError  # noqa: F401  (RerankerNameError: part of the module's surface)
from marqo_amd.s2_inference.reranking.cross_encoders import ReRankerText
from marqo_amd.s2_inference.reranking.enums import ResultsFields


def rerank_search_results(search_result: Dict, query: str, model_name: str, device: str, searchable_attributes: Optional[List[str]] = None,
                          num_highlights: int = 1, overwrite_original_scores_highlights: bool = True) -> None:
    """Rescore the hits of `search_result` against `query` and reorder them, in place.  A result none of whose hits holds any of the
    searchable attributes is handed back untouched.  Text cross-encoders only: the OWL-ViT image reranker and the 'onnx/' prefix are refused."""
    if not _check_searchable_fields_in_results(search_results=search_result, searchable_fields=searchable_attributes):
        return search_result
    if "owl" in model_name.lower():
        raise RerankerError(message=f"{model_name}: the OWL-ViT image reranker is not served by the marqo_amd engine (text cross-encoders only)")
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

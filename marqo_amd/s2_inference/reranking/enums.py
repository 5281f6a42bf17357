"""Key names the reranking step reads from and writes into a search result (the reference's s2_inference/reranking/enums.py names)."""


class ResultsFields:
    """keys of a search result and of its hits"""
    hits = "hits"
    id = "_id"
    original_score = "_score"
    highlights = "_highlights"
    # written while reranking; the last step folds them into _score / _highlights and removes them
    reranked_id = "_rerank_id"
    reranker_score = "_reranked_score"
    highlights_reranked = "_reranked_highlights"
    hybrid_score_multiply = "_score_multiply"
    hybrid_score_add = "_score_add"


class Columns:
    """names of the per-row values of the scoring table (one row per hit, field and chunk)"""
    query = "query"
    field_content = "field_content"
    field_content_original = "field_content_original"
    field_name = "field_name"
    original_field_name = "original_field_name"
    bbox = "bbox"
    bbox_original = "bbox_original"
    original_size = "original_size"

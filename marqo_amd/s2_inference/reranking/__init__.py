"""Text reranking of search results with a cross-encoder on the engine's BERT tower (`rerank.rerank_search_results`)."""

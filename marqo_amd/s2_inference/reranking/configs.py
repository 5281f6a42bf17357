"""Defaults of the reranking step."""
from typing import Dict


def get_default_text_processing_parameters() -> Dict:
    """how a field's text is cut into the chunks that are scored: two sentences per chunk, no overlap (processing/text.split_text)"""
    return dict(split_length=2, split_overlap=0, split_method="sentence")

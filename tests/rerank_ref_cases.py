"""The plumbing cases of tests/test_rerank_host.py, shared with tests/rerank_ref_plumbing.py (the reference's side), and the injected scorer:
a deterministic function of (query, chunk) without ties."""
import zlib

QUERY = "what is a good sentence?"


def crc_score(query: str, chunk: str) -> float:
    return (zlib.crc32((query + "\0" + chunk).encode("utf-8")) + 0.5) / 2.0 ** 32


def _hits():
    return [
        {"_id": "d1", "title": "One sentence here. Another one follows. A third closes it. And a fourth.", "body": "Short body text.",
         "_score": 0.61, "_highlights": {"title": "One sentence here."}},
        {"_id": "d2", "title": "Completely different title. With two parts.", "body": "The body speaks. It has three. Sentences in all.",
         "_score": 0.58, "_highlights": {"body": "The body speaks."}},
        {"_id": "d3", "title": "Last title. Of the three. Documents we have. Here today. And more.", "body": "Body one. Body two. Body three.",
         "_score": 0.40, "_highlights": []},
    ]


def cases():
    """name -> {search_result, query, kwargs}"""
    c = {}
    c["all_fields"] = dict(search_result={"hits": _hits(), "limit": 10, "query": QUERY}, kwargs={})
    c["attribute_list"] = dict(search_result={"hits": _hits()}, kwargs={"searchable_attributes": ["body"]})
    c["two_attributes"] = dict(search_result={"hits": _hits()}, kwargs={"searchable_attributes": ["body", "title"]})
    c["attributes_no_hit_has"] = dict(search_result={"hits": _hits()}, kwargs={"searchable_attributes": ["nothing", "nowhere"]})
    missing = _hits()
    del missing[1]["body"]
    missing[2]["title"] = None
    c["hits_missing_a_field"] = dict(search_result={"hits": missing}, kwargs={})
    c["hits_missing_a_listed_field"] = dict(search_result={"hits": missing}, kwargs={"searchable_attributes": ["title", "body"]})
    no_id = _hits()
    del no_id[0]["_id"]
    c["hit_without_id"] = dict(search_result={"hits": no_id}, kwargs={})
    c["hit_without_id_keep"] = dict(search_result={"hits": no_id}, kwargs={"overwrite_original_scores_highlights": False})
    c["empty_hits"] = dict(search_result={"hits": []}, kwargs={})
    c["empty_hits_with_list"] = dict(search_result={"hits": []}, kwargs={"searchable_attributes": ["title"]})
    c["keep_original"] = dict(search_result={"hits": _hits()}, kwargs={"overwrite_original_scores_highlights": False})
    c["two_highlights"] = dict(search_result={"hits": _hits()}, kwargs={"num_highlights": 2})
    c["two_highlights_keep"] = dict(search_result={"hits": _hits()}, kwargs={"num_highlights": 2, "overwrite_original_scores_highlights": False})
    one_row = _hits()
    one_row[1] = {"_id": "d2", "title": "Only one chunk.", "_score": 0.5}
    c["two_highlights_one_row"] = dict(search_result={"hits": one_row}, kwargs={"num_highlights": 2, "searchable_attributes": ["title"]})
    nothing = _hits()
    nothing[2] = {"_id": "d3", "other": "A field. That is not listed.", "_score": 0.1}
    c["hit_with_nothing_to_score"] = dict(search_result={"hits": nothing}, kwargs={"searchable_attributes": ["title"]})
    for v in c.values():
        v["query"] = QUERY
    return c

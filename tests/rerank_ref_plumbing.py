"""Run by tests/test_rerank_host.py in a FRESH interpreter: the reference's own rerank_search_results (pandas and all) under oracle/ref_shim.py,
with its cross-encoder loader replaced by the injected scorer of tests/rerank_ref_cases.  argv[1]: a JSON file of cases -> one JSON line
with, per case, the result dict (or the error's class name) and whether the function handed the result back untouched.  Test infrastructure;
never imported by the product."""
import copy
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main() -> int:
    from oracle import ref_shim
    from marqo_amd.s2_inference.processing import text as product_text
    ref_shim.install(sent_tokenize=product_text._sentences, word_tokenize=product_text._WORD.findall)
    from marqo.s2_inference.reranking import cross_encoders, rerank
    from rerank_ref_cases import crc_score

    class Scorer:
        def predict(self, pairs):
            return np.asarray([crc_score(q, c) for q, c in pairs], dtype=np.float64)

    cross_encoders.load_sbert_cross_encoder_model = lambda model_name, device, max_length=512: {"model": Scorer()}
    with open(sys.argv[1]) as f:
        cases = json.load(f)
    out = {}
    for name, case in cases.items():
        result = copy.deepcopy(case["search_result"])
        try:
            ret = rerank.rerank_search_results(result, case["query"], "injected", "cpu", **case["kwargs"])
            out[name] = {"result": result, "returned_input": ret is result}
        except Exception as e:  # noqa: BLE001 - the class name is the finding
            out[name] = {"raises": type(e).__name__}
    print(json.dumps(out, default=float))
    return 0


if __name__ == "__main__":
    sys.exit(main())

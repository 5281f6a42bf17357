"""Run by tests/test_owl_host.py in a FRESH interpreter: the reference's own ReRankerOwl bookkeeping (pandas and all) under oracle/ref_shim.py, with
its model replaced by the injected detector of tests/owl_ref.fake_detection.  argv[1]: a JSON file of cases -> one JSON line with, per case, the
result dict as `rerank` leaves it and as the entry point's clean-up leaves it (or the error's class name).  Test infrastructure; never imported
by the product."""
import copy
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main() -> int:
    from oracle import ref_shim
    ref_shim.install()
    import torch
    from marqo.s2_inference.reranking import cross_encoders, rerank
    from owl_ref import fake_detection

    class Inputs:
        def __init__(self, image):
            self.image = image

        def to(self, device):
            return self

    class Processor:
        post_process = None

    def predict(model, processed_inputs, post_process_function, size):
        scores, boxes = fake_detection(np.asarray(processed_inputs.image, dtype=np.uint8))
        return [{"boxes": torch.from_numpy(boxes), "scores": torch.from_numpy(scores), "labels": torch.zeros(len(scores), dtype=torch.long)}]

    cross_encoders.load_owl_vit = lambda model_name, device: {"model": object(), "processor": Processor()}
    cross_encoders._process_owl_inputs = lambda processor, texts, images: Inputs(images)
    cross_encoders._predict_owl = predict
    with open(sys.argv[1]) as f:
        cases = json.load(f)
    out = {}
    for name, case in cases.items():
        result = copy.deepcopy(case["search_result"])
        try:
            r = cross_encoders.ReRankerOwl(model_name=case["model_name"], device="cpu", image_size=(240, 240))
            r.rerank(query=case["query"], results=result, image_attributes=case["attributes"], num_highlights=case["num_highlights"])
            working = json.loads(json.dumps(result, default=float))
            rerank.cleanup_final_reranked_results(result)
            out[name] = {"working": working, "result": result}
        except Exception as e:  # noqa: BLE001 - the class name is the finding
            out[name] = {"raises": type(e).__name__}
    print(json.dumps(out, default=float))
    return 0


if __name__ == "__main__":
    sys.exit(main())

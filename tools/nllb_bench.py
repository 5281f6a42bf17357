#!/usr/bin/env python
"""NLLB-CLIP text path: the HIP text tower against the same M2M100 encoder run by torch in bf16 on the same GPU in the same run (1 024 texts of
mixed length; one text), and device against host SentencePiece-BPE tokenisation in texts/s (a BPE model trained on the spot: no NLLB vocabulary
ships with the repository).  Prints one JSON line.   python tools/nllb_bench.py [--size base|large] [--texts 1024] [--reps 10]"""
import argparse
import json
import os
import sys
import tempfile
import time
from dataclasses import replace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append(time.perf_counter() - t0)
    return float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="base", choices=["base", "large"])
    ap.add_argument("--texts", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--vocab", type=int, default=32000, help="rows of the token table (the gather does not depend on it; NLLB-200 has 256206)")
    a = ap.parse_args()
    from marqo_amd.engine import archs, towers
    from marqo_amd.engine.gpu_tokenizers import DeviceSentencePieceTokenizer
    from marqo_amd.engine.tokenizers import NllbTokenizer
    from tests import nllb_util as U
    dev = "cuda:0"
    name = "facebook/nllb-200-distilled-600M" if a.size == "base" else "facebook/nllb-200-distilled-1.3B"
    arch = replace(archs.NLLB_TEXT_ARCHS[name], vocab=a.vocab)
    enc = U.m2m100_encoder(a.vocab, arch.layers, arch.mlp_dim, seed=1)
    sd, proj = U.checkpoint_of(enc, arch.out_dim, seed=1)
    rng = np.random.default_rng(0)
    lengths = rng.integers(3, 78, size=a.texts).tolist()
    ids = U.rows(lengths, a.vocab, 77, seed=2)
    tw = towers.NllbTextTower(arch, sd, dev)
    tw.release_unused_folded()
    enc_bf = enc.to(device=dev, dtype=torch.bfloat16)
    proj_bf = proj.to(device=dev, dtype=torch.bfloat16)
    d_ids = ids.to(dev)
    mask = (d_ids != 1).long()

    @torch.no_grad()
    def torch_run(i=d_ids, m=mask):
        return enc_bf(input_ids=i, attention_mask=m).last_hidden_state[:, 0] @ proj_bf.t()
    res = {"tool": "nllb_bench", "size": a.size, "device": torch.cuda.get_device_name(0), "texts": a.texts, "tokens": int(sum(lengths)),
           "residual_stream": tw.residual_stream}
    t_ours = timed(lambda: tw.encode_ids(ids, normalize=False), a.reps)
    t_torch = timed(torch_run, a.reps)
    res["tower_batch_ms"] = {"hip": round(t_ours * 1e3, 3), "torch_bf16_padded": round(t_torch * 1e3, 3)}
    res["tower_batch_texts_per_s"] = {"hip": round(a.texts / t_ours), "torch_bf16_padded": round(a.texts / t_torch)}
    one = ids[5:6, :lengths[5]]
    d_one = one.to(dev)
    t1 = timed(lambda: tw.encode_ids(one, normalize=False), 50)
    t1t = timed(lambda: torch_run(d_one, torch.ones_like(d_one)), 50)
    res["tower_one_text_ms"] = {"hip": round(t1 * 1e3, 3), "torch_bf16": round(t1t * 1e3, 3), "tokens": int(lengths[5])}
    with tempfile.TemporaryDirectory() as d:
        host = NllbTokenizer(U.train_bpe(d, vocab_size=4000))
        devtok = DeviceSentencePieceTokenizer(host, dev)
        texts = U.corpus(5, a.texts)
        t_dev = timed(lambda: devtok.encode_device(texts, 77), a.reps)
        t0 = time.perf_counter()
        for _ in range(3):
            host(texts, max_length=77)
        t_host = (time.perf_counter() - t0) / 3
        res["tokenize_texts_per_s"] = {"device": round(a.texts / t_dev), "host": round(a.texts / t_host)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()

"""ColbertTower end to end against a float64 restatement over a transformers BertModel: a seeded 2-layer checkpoint directory (W 128, 2 heads) with
artifact.metadata, one query against documents of 1, 16, 17 and 70 pieces (the last longer than doc_maxlen) and a punctuation-only one.
  exact   the BertModel in float64 on the fp32 weights (the query's [MASK] rows masked as KEYS through attention_mask), linear, L2
  model   the same with the engine's bf16 roundings: every Linear's weight and input, q / k / v outputs, the unit rows themselves
Bars: every token row within 4.0 x the model's own error (encoder_ref.row_ratio); scores within TOL = 4.0 x query_maxlen x (worst query-row + worst
document-row error of the model, 2-norm): |q.d - q'.d'| <= |q - q'| + |d - d'| for unit rows, a maximum moves by at most that, the score sums
query_maxlen maxima.  On an MI355X: rows <= 1.69, scores within 0.03 (TOL 1.41), the flag moves every score by 13.6 .. 19.7."""
import json
import os
import string

import numpy as np
import pytest
import torch

from tests import encoder_ref as E
from tests import rerank_ref as RR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VOCAB = RR.VOCAB + ["[unused0]", "[unused1]", ";"]
QMAX, DMAX, DIM, W = 32, 40, 128, 128
CFG = dict(model_type="bert", vocab_size=len(VOCAB), hidden_size=W, num_hidden_layers=2, num_attention_heads=2, intermediate_size=512,
           max_position_embeddings=512, type_vocab_size=2, hidden_act="gelu", layer_norm_eps=1e-12, hidden_dropout_prob=0.0,
           attention_probs_dropout_prob=0.0, position_embedding_type="absolute", pad_token_id=0)
QUERY = RR.words(2, seed=3)          # 5 unpadded rows: 27 of the 32 query rows are [MASK] padding
DOCS = [RR.WORDS[5], RR.words(16, seed=11), RR.words(17, seed=12), RR.words(70, seed=13), ". , ; ! ?", RR.words(9, seed=14) + " , " + RR.words(3, seed=15)]


def _write(directory, attend):
    from safetensors.torch import save_file
    from marqo_amd.engine import synthetic
    os.makedirs(directory)
    # Random-init scales leave a row to its own embedding (the residual): the float64 scores of the two attend_to_mask_tokens settings then lie
    # 0.2 .. 1.7 apart, inside TOL.  With the value path 4 x as strong they lie 13 .. 20 apart (TOL 1.4): computed on the reference alone.
    sd = synthetic.cross_encoder_state_dict(W, 2, 2, 512, vocab=len(VOCAB), seed=5, attention_gain=1.0)
    sd = {k: v * 4.0 if k.endswith(("attention.self.value.weight", "attention.output.dense.weight")) else v
          for k, v in sd.items() if k.startswith("bert.") and ".pooler." not in k}
    sd["linear.weight"] = torch.randn(DIM, W, generator=torch.Generator().manual_seed(6)) / W ** 0.5
    save_file({k: v.contiguous() for k, v in sd.items()}, os.path.join(directory, "model.safetensors"))
    meta = dict(query_maxlen=QMAX, doc_maxlen=DMAX, dim=DIM, similarity="cosine", mask_punctuation=True, attend_to_mask_tokens=attend)
    for name, obj in (("config.json", CFG), ("tokenizer_config.json", dict(do_lower_case=True, model_max_length=512)), ("artifact.metadata", meta)):
        with open(os.path.join(directory, name), "w") as f:
            json.dump(obj, f)
    with open(os.path.join(directory, "vocab.txt"), "w", encoding="utf-8") as f:
        f.write("\n".join(VOCAB) + "\n")
    return sd


def _bf16(t):
    return t.to(torch.bfloat16).to(torch.float64)


def _reference(sd, rows, n_keys, rounded):
    """unit rows float64 [len, DIM] of every id row (rows[i] attends keys [0, n_keys[i]))"""
    from transformers import BertConfig, BertModel
    model = BertModel(BertConfig(**CFG), add_pooling_layer=False).double().eval()
    model.load_state_dict({k[5:]: v.double() for k, v in sd.items() if k.startswith("bert.")}, strict=False)
    rnd = _bf16 if rounded else (lambda t: t)
    for name, m in model.named_modules() if rounded else ():
        if isinstance(m, torch.nn.Linear):
            m.weight.data = _bf16(m.weight.data)
            m.register_forward_pre_hook(lambda mod, a: (_bf16(a[0]),))
            if name.endswith((".query", ".key", ".value")):
                m.register_forward_hook(lambda mod, a, out: _bf16(out))
    out = []
    with torch.no_grad():
        for ids, nk in zip(rows, n_keys):
            mask = (torch.arange(len(ids)) < nk).long()[None]
            y = rnd(model(input_ids=torch.tensor(ids)[None].long(), attention_mask=mask).last_hidden_state[0]) @ rnd(sd["linear.weight"].double()).t()
            out.append(rnd(y / y.norm(dim=1, keepdim=True).clamp_min(1e-12)))
    return out


def _scores(q, docs, keeps):
    return np.asarray([float((q @ d.t()).masked_fill(~k[None], float("-inf")).max(dim=1).values.sum()) for d, k in zip(docs, keeps)])


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    from marqo_amd.engine.rerank import ColbertTower, load_cross_encoder_tower
    root = tmp_path_factory.mktemp("colbert")
    dirs = {a: str(root / f"attend_{int(a)}") for a in (False, True)}
    sd = [_write(dirs[a], a) for a in (False, True)][0]
    tower = load_cross_encoder_tower(dirs[False], DEV)
    assert isinstance(tower, ColbertTower)
    q_row, nk = tower.query_row(QUERY)
    d_ids, d_len = tower.doc_rows(DOCS, DMAX)
    rows = [q_row.tolist()] + [d_ids[i, :int(n)].cpu().tolist() for i, n in enumerate(d_len)]
    assert [len(r) for r in rows] == [QMAX, 4, 19, 20, DMAX, 8, 16] and nk == 5
    skip = {VOCAB.index(c) for c in string.punctuation if c in VOCAB}
    keeps = [torch.tensor([i not in skip for i in r]) for r in rows[1:]]
    assert int(keeps[4].sum()) == 3                     # [CLS] [D] [SEP] of the punctuation-only document
    n_keys = [nk] + [len(r) for r in rows[1:]]
    ex, mo = _reference(sd, rows, n_keys, False), _reference(sd, rows, n_keys, True)
    err = [float((m - e).norm(dim=1).max()) for m, e in zip(mo, ex)]
    ex_attend = _reference(sd, rows[:1], [QMAX], False)[0]
    return dict(dirs=dirs, tower=tower, ex=ex, mo=mo, tol=4.0 * QMAX * (err[0] + max(err[1:])), ref=_scores(ex[0], ex[1:], keeps),
                ref_attend=_scores(ex_attend, ex[1:], keeps))


def test_token_rows_and_scores_against_float64(case):
    maxsim, scaled, q_emb, d_embs = case["tower"].score(QUERY, DOCS, return_embeddings=True)
    for i, got in enumerate([q_emb] + d_embs):
        r = E.row_ratio(got.cpu().double(), case["ex"][i], case["mo"][i])
        print(f"COLBERT_ROWS seq={i} rows={got.shape[0]} ratio={r['ratio']:.3f}")
        assert r["ratio"] <= 4.0, (i, r)
    print(f"COLBERT_SCORES got={maxsim.tolist()} ref={case['ref'].tolist()} tol={case['tol']:.3e}")
    assert np.abs(maxsim.astype(np.float64) - case["ref"]).max() <= case["tol"]
    assert np.array_equal(scaled, maxsim / np.float32(QMAX))


def test_attend_to_mask_tokens_changes_the_scores(case):
    """the key prefix is exercised: with the [MASK] rows as keys EVERY document's score moves by more than TOL, and lands on its own float64 reference"""
    from marqo_amd.engine.rerank import load_cross_encoder_tower
    other = load_cross_encoder_tower(case["dirs"][True], DEV).score(QUERY, DOCS)[0]
    moved = np.abs(other - case["tower"].score(QUERY, DOCS)[0])
    print(f"COLBERT_FLIP moved={moved.tolist()} tol={case['tol']:.3e}")
    assert np.abs(other.astype(np.float64) - case["ref_attend"]).max() <= case["tol"] and moved.min() > case["tol"]


def test_ranking_through_rerank_search_results(case):
    from marqo_amd.s2_inference.reranking.rerank import rerank_search_results
    from marqo_amd.s2_inference.s2_inference import _create_model_cache_key, get_available_models
    name, ref = case["dirs"][False], case["ref"]
    idx = [0, 1, 2, 3, 5]               # (the punctuation-only document is several empty sentences to the result plumbing's splitter)
    result = {"hits": [{"_id": str(i), "body": DOCS[i], "_score": 0.1} for i in idx], "limit": len(idx)}
    rerank_search_results(result, QUERY, name, DEV, searchable_attributes=["body"])
    del get_available_models()[_create_model_cache_key(name, DEV)]
    got = [int(h["_id"]) for h in result["hits"]]
    pairs = [(i, j) for i in idx for j in idx if ref[i] - ref[j] > case["tol"]]     # float64 scores separated by more than the tolerance
    assert len(pairs) >= 4 and all(got.index(i) < got.index(j) for i, j in pairs), (got, ref.tolist(), pairs)

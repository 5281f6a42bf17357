"""Host half of the ColBERT reranker (engine/rerank.py): id rows and keep table against hand-written rows, layout detection, refusals by key."""
import os

import numpy as np
import pytest
import torch

from marqo_amd.engine import rerank as RK
from tests import rerank_ref as RR

CLS, SEP, MASK, Q, D = 2, 3, 4, 9, 10
BERT = ["bert.embeddings.word_embeddings.weight", "bert.encoder.layer.0.output.dense.weight"]


@pytest.mark.parametrize("pieces,qmax,row,n", (
    ([20, 21], 8, [CLS, Q, 20, 21, SEP, MASK, MASK, MASK], 5),
    ([20, 21, 22, 23, 24], 8, [CLS, Q, 20, 21, 22, 23, 24, SEP], 8),
    ([20, 21, 22, 23, 24, 25, 26], 8, [CLS, Q, 20, 21, 22, 23, 24, SEP], 8),          # cut with [SEP] kept
    ([], 4, [CLS, Q, SEP, MASK], 3)))
def test_query_row(pieces, qmax, row, n):
    got, length = RK.colbert_query_row(pieces, qmax, CLS, SEP, MASK, Q)
    assert got.dtype == np.int32 and got.tolist() == row and length == n


def test_document_rows_and_skip_table():
    ids = torch.tensor([[CLS, 20, 21, SEP, 0], [CLS, SEP, 0, 0, 0]], dtype=torch.int32)
    assert RK.colbert_doc_rows(ids, D).tolist() == [[CLS, D, 20, 21, SEP, 0], [CLS, D, SEP, 0, 0, 0]]
    vocab = {"[PAD]": 0, "a": 1, ".": 2, "##.": 3, "!": 4, "...": 5, "~": 99}
    assert RK.colbert_skip_table(vocab, 8).tolist() == [0, 0, 1, 0, 1, 0, 0, 0]      # single characters only; ids past the table are ignored


@pytest.mark.parametrize("meta,shape,key", ((dict(similarity="l2"), (128, 768), "similarity"), (dict(dim=32), (32, 768), "dim"), ({}, (100, 768), "dim"),
                                            (dict(dim=64), (128, 768), "dim"), (dict(query_maxlen=65), (128, 768), "query_maxlen")))
def test_settings_refusals_name_the_key(meta, shape, key):
    with pytest.raises(ValueError, match=key):
        RK.colbert_settings(meta, shape, 768)


def test_settings_and_layout_detection(tmp_path):
    assert RK.colbert_settings(None, (128, 768), 768) == RK.ColbertSettings(32, 180, 128, True, False)
    meta = dict(query_maxlen=64, doc_maxlen=300, dim=96, mask_punctuation=False, attend_to_mask_tokens=True)
    assert RK.colbert_settings(meta, (96, 384), 384) == RK.ColbertSettings(64, 300, 96, False, True)
    d = str(tmp_path)
    assert RK.colbert_layout(d, dict(model_type="bert"), BERT + ["linear.weight"]) is True
    with pytest.raises(ValueError, match="model_type='xlm-roberta'"):
        RK.colbert_layout(d, dict(model_type="xlm-roberta"), ["roberta.embeddings.word_embeddings.weight", "linear.weight"])
    os.mkdir(os.path.join(d, "1_Dense"))
    with pytest.raises(ValueError, match="1_Dense"):
        RK.colbert_layout(d, dict(model_type="modernbert"), ["model.embeddings.tok_embeddings.weight"])
    assert RK.colbert_layout(d, dict(model_type="bert"), BERT + ["linear.weight", "classifier.weight"]) is False    # a classifier: a cross-encoder, 1_Dense or not


def test_one_label_bert_directory_still_loads_as_cross_encoder(tmp_path, monkeypatch):
    RR.write_cross_encoder_dir(tmp_path, "tinybert")
    seen = {}
    monkeypatch.setattr(RK.CrossEncoderTower, "__init__", lambda self, arch, sd, device, tok, **kw: seen.update(keys=set(sd), kw=kw))
    monkeypatch.setattr(RK.ColbertTower, "_from_loaded", classmethod(lambda cls, *a: pytest.fail("taken for a ColBERT")))
    tower = RK.load_cross_encoder_tower(str(tmp_path), "cuda:0")
    assert type(tower) is RK.CrossEncoderTower and "classifier.weight" in seen["keys"] and seen["kw"]["family"] is RK.BERT


def test_missing_marker_token_is_refused_before_any_gpu_work():
    from marqo_amd.engine import archs
    from marqo_amd.engine.tokenizers import WordPieceTokenizer
    tok = WordPieceTokenizer(["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]", "[unused0]", "a"])
    arch = archs.bert_arch_from_hf_config(dict(model_type="bert", vocab_size=7, hidden_size=128, num_hidden_layers=1, num_attention_heads=2,
                                               intermediate_size=256, max_position_embeddings=64))
    with pytest.raises(ValueError, match=r"\[unused1\]"):
        RK.ColbertTower(arch, {}, "cuda:0", tok, RK.ColbertSettings())

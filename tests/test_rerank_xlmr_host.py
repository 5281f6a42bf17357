"""XLM-RoBERTa cross-encoders without a GPU: the weight names of the head against transformers' own RobertaClassificationHead, what
CrossEncoderTower.from_dir accepts and refuses, the pair plan with four special tokens against the fast tokenizer, and the argument checks of
the new entry points."""
import ctypes as C
import json
import os
import shutil
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rerank_ref as RR  # noqa: E402
import rerank_xlmr_ref as XR  # noqa: E402
from marqo_amd import _lib as L  # noqa: E402
from marqo_amd.engine import rerank as ER  # noqa: E402
from marqo_amd.engine.tokenizers import WordPieceTokenizer, XlmRobertaTokenizer  # noqa: E402

W = XR.SHAPE["W"]


@pytest.fixture(scope="module")
def ckpt(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("xlmr_ce"))
    model = XR.write_dir(d, seed=0, stray_pooler=True)
    return d, model


# ---- weight names -----------------------------------------------------------------------------------------------------------------------------
def _head(dense_w, dense_b, out_w, out_b, h):
    return (torch.tanh(h @ dense_w.T + dense_b) @ out_w.T + out_b)[:, 0]


def test_head_names_are_roberta_classification_heads(ckpt):
    """classifier.dense / classifier.out_proj land in the head: tanh(Linear) . w + b over them is transformers' RobertaClassificationHead on the
    same rows, and exchanging either pair of tensors is seen"""
    from marqo_amd.engine import checkpoint
    d, model = ckpt
    _, sd = checkpoint.load_hf_dir(d)
    assert "roberta.pooler.dense.weight" in sd, "the fixture carries a stray pooler"
    dw, db, ow, ob = ER.head_tensors(sd, ER.XLMR, W)
    assert torch.equal(dw, sd["classifier.dense.weight"]) and torch.equal(ow, sd["classifier.out_proj.weight"])
    assert not torch.equal(dw, sd["roberta.pooler.dense.weight"]), "the stray pooler is not the head"
    h = torch.randn(6, W, generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        ref = model.classifier(h[:, None, :])[:, 0]
    ours = _head(dw.float(), db.float(), ow.float(), ob.float(), h)
    assert torch.allclose(ours, ref, rtol=0, atol=1e-5), float((ours - ref).abs().max())
    spread = float(ref.std())
    # a swapped weight (the stray pooler's, or the dense weight transposed) or bias (the pooler's) moves the logits by far more than rounding
    for name, args in (("pooler weight", (sd["roberta.pooler.dense.weight"].float(), db.float())), ("transposed", (dw.float().T, db.float())),
                       ("pooler bias", (dw.float(), sd["roberta.pooler.dense.bias"].float()))):
        off = float((_head(args[0], args[1], ow.float(), ob.float(), h) - ref).abs().max())
        assert off > 0.05 * spread, (name, off, spread)
    # dense and out_proj exchanged do not fit: the shapes are checked by name
    swapped = dict(sd)
    swapped["classifier.dense.bias"], swapped["classifier.out_proj.weight"] = sd["classifier.out_proj.weight"], sd["classifier.dense.bias"]
    with pytest.raises(ValueError, match="classifier.dense.bias"):
        ER.head_tensors(swapped, ER.XLMR, W)
    for gone in ("classifier.out_proj.weight", "classifier.out_proj.bias"):
        with pytest.raises(KeyError, match=gone.replace(".", r"\.")):
            ER.head_tensors({k: v for k, v in sd.items() if k != gone}, ER.XLMR, W)
    # the BERT family reads its own names and finds none of them here
    with pytest.raises(KeyError, match=r"bert\.pooler\.dense\.weight"):
        ER.head_tensors(sd, ER.BERT, W)


# ---- from_dir: families and refusals --------------------------------------------------------------------------------------------------------------
class _Captured(Exception):
    pass


@pytest.fixture()
def capture(monkeypatch):
    """from_dir up to the constructor: what it would build, without a device"""
    seen = {}

    def init(self, arch, sd, device, tokenizer, model_max_length=512, family=ER.BERT):
        seen.update(arch=arch, sd=sd, tokenizer=tokenizer, model_max_length=model_max_length, family=family)
        raise _Captured()
    monkeypatch.setattr(ER.CrossEncoderTower, "__init__", init)
    return seen


def _edit_config(d, **changes):
    p = os.path.join(d, "config.json")
    with open(p) as f:
        cfg = json.load(f)
    cfg.update(changes)
    with open(p, "w") as f:
        json.dump(cfg, f)


def test_from_dir_takes_xlm_roberta_and_sentencepiece_roberta(ckpt, capture, tmp_path):
    d, _ = ckpt
    with pytest.raises(_Captured):
        ER.CrossEncoderTower.from_dir(d, "cuda:0")
    a = capture["arch"]
    assert capture["family"] is ER.XLMR and isinstance(capture["tokenizer"], XlmRobertaTokenizer)
    assert (a.pos_offset, a.max_pos, a.type_vocab, a.width, a.layers, a.heads, a.mlp_dim) == (2, XR.USABLE, 1, W, 2, 2, 256)
    assert capture["model_max_length"] == 512                      # (the constructor caps it by the usable positions: GPU test)
    assert capture["tokenizer"].vocab_size == a.vocab
    # the same directory under model_type roberta: served, because the SentencePiece model is there
    rb = str(tmp_path / "rb")
    shutil.copytree(d, rb)
    _edit_config(rb, model_type="roberta")
    with pytest.raises(_Captured):
        ER.CrossEncoderTower.from_dir(rb, "cuda:0")
    assert capture["family"] is ER.XLMR and capture["arch"].pos_offset == 2


def test_from_dir_refusals(ckpt, capture, tmp_path):
    d, _ = ckpt
    three = str(tmp_path / "three")
    shutil.copytree(d, three)
    _edit_config(three, num_labels=3, id2label={"0": "a", "1": "b", "2": "c"}, label2id={"a": 0, "b": 1, "c": 2})
    with pytest.raises(ValueError, match="num_labels=3 is not served"):
        ER.CrossEncoderTower.from_dir(three, "cuda:0")
    bpe = str(tmp_path / "bpe")
    shutil.copytree(d, bpe)
    os.remove(os.path.join(bpe, "sentencepiece.bpe.model"))
    for f, text in (("vocab.json", "{}"), ("merges.txt", "#version: 0.2\n")):
        with open(os.path.join(bpe, f), "w") as fh:
            fh.write(text)
    _edit_config(bpe, model_type="roberta")
    with pytest.raises(ValueError, match="byte-level BPE tokeniser.*is not served"):
        ER.CrossEncoderTower.from_dir(bpe, "cuda:0")
    deb = str(tmp_path / "deberta")
    shutil.copytree(d, deb)
    _edit_config(deb, model_type="deberta-v2")
    with pytest.raises(ValueError, match="model_type='deberta-v2' is not served as a cross-encoder"):
        ER.CrossEncoderTower.from_dir(deb, "cuda:0")
    assert not capture, "a refused directory reached the constructor"


def test_bert_directories_take_the_old_path(capture, tmp_path):
    sd = RR.write_cross_encoder_dir(tmp_path, "tinybert", seed=0)
    with pytest.raises(_Captured):
        ER.CrossEncoderTower.from_dir(str(tmp_path), "cuda:0")
    assert capture["family"] is ER.BERT and isinstance(capture["tokenizer"], WordPieceTokenizer)
    assert capture["arch"].pos_offset == 0 and capture["arch"].type_vocab == 2 and capture["model_max_length"] == 512
    pw, pb, cw, cb = ER.head_tensors(capture["sd"], ER.BERT, 128)
    assert torch.equal(pw, sd["bert.pooler.dense.weight"]) and torch.equal(cw, sd["classifier.weight"]) and cb.shape == (1,) and pb.shape == (128,)
    assert (ER.BERT.specials, ER.BERT.typed, ER.XLMR.specials, ER.XLMR.typed) == (3, True, 4, False)


def test_reranker_error_reads_right_for_the_new_family(ckpt, tmp_path):
    from marqo_amd.s2_inference.errors import RerankerError
    from marqo_amd.s2_inference.reranking import cross_encoders
    d, _ = ckpt
    bpe = str(tmp_path / "bpe")
    shutil.copytree(d, bpe)
    os.remove(os.path.join(bpe, "sentencepiece.bpe.model"))
    open(os.path.join(bpe, "merges.txt"), "w").close()
    with pytest.raises(RerankerError, match="cannot load the reranker .* byte-level BPE tokeniser"):
        cross_encoders.load_cross_encoder_model(bpe, "cuda:0")


# ---- pair plan with four specials ---------------------------------------------------------------------------------------------------------------------
def test_pair_lengths_with_four_specials(ckpt):
    """pair_lengths(.., specials=4) against the pair oracle (ids, not only lengths) and against the rule written out in rerank_xlmr_ref; with
    B = max_length - 4 it is the three-special rule one token earlier"""
    d, _ = ckpt
    tok = XlmRobertaTokenizer(d)
    words = XR.one_piece_words(tok)
    assert len(words) >= 20
    oracle = XR.pair_oracle(d, tok)
    print(f"pair oracle: {XR.PAIR_ORACLE}")
    cases = []
    for max_length in (5, 6, 16, 17, 64):
        B = max_length - 4
        pairs = {(la, B - 1 - la) for la in (0, 1, B // 2) if B - 1 - la >= 0}                         # la + lb = B - 1
        pairs |= {(la, B - la) for la in (0, 1, B // 2, B)} | {(la, B + 1 - la) for la in (0, 1, B // 2, B + 1)}     # = B, = B + 1
        pairs |= {(B, B), (B + 1, B + 1), (B // 2 + 1, B // 2 + 1), (40, 40)}                          # ties
        pairs |= {(B + 1, B + 5), (B + 5, B + 1), (B + 3, 90), (90, B + 3)}                            # the shorter text is longer than B
        pairs |= {(0, 0), (3, 0), (B + 2, 0), (0, B + 2), (1, 90), (90, 1)}                            # an empty document / query
        cases += [(max_length, la, lb) for la, lb in sorted(pairs)]
    assert any(m == 5 for m, _, _ in cases)
    bad = []
    for max_length, la, lb in cases:
        q, doc = XR.text_of(words, la, seed=la), XR.text_of(words, lb, seed=100 + lb)
        qp, dp = tok.encode(q)[1:-1], tok.encode(doc)[1:-1]
        assert (len(qp), len(dp)) == (la, lb)
        a, b = ER.pair_lengths(la, lb, max_length, 4)
        want = oracle(q, [doc], max_length)[0]
        if want != [XR.CLS, *qp[:a], XR.SEP, XR.SEP, *dp[:b], XR.SEP] or (a, b) != XR.longest_first(la, lb, max_length):
            bad.append((max_length, la, lb, a, b, len(want)))
        assert (a, b) == ER.pair_lengths(la, lb, max_length - 1), "four specials at max_length = three specials at max_length - 1"
        assert len(want) <= max_length
    assert not bad, bad[:5]
    va, vb = ER.pair_lengths(np.arange(20)[:, None], np.arange(20)[None, :], 16, 4)
    assert all((int(va[i, j]), int(vb[i, j])) == XR.longest_first(i, j, 16) for i in range(20) for j in range(20))
    with pytest.raises(ValueError, match="at least 5"):
        ER.pair_lengths(3, 3, 4, 4)
    assert ER.pair_lengths(3, 3, 4) == (0, 1)                                       # three specials: unchanged


# ---- the library's argument checks (no launch) ----------------------------------------------------------------------------------------------------------
def test_argument_errors_are_reported_without_a_gpu():
    lib = L.load()
    fake = 256

    def refused(rc, msg):
        assert rc == -1 and msg in lib.mq_last_error(), (rc, lib.mq_last_error())

    refused(lib.mq_pair_plan_n(3, fake, 1, 16, 4, 4, fake, fake, fake, None), b"max_length=4 must be >= 5")
    refused(lib.mq_pair_plan_n(3, fake, 1, 16, 16, 9, fake, fake, fake, None), b"specials=9")
    refused(lib.mq_pair_plan_n(3, fake, 1, 1, 16, 4, fake, fake, fake, None), b"mq_pair_plan: bad shape")
    assert lib.mq_pair_plan_n(3, None, 0, 16, 16, 4, None, None, None, None) == 0        # no pairs: nothing to do
    refused(lib.mq_pack_pairs_xlmr(fake, 3, None, 16, fake, fake, fake, 1, 0, 2, fake, 10, None), b"mq_pack_pairs_xlmr: null pointer")
    refused(lib.mq_pack_pairs_xlmr(None, 3, fake, 16, fake, fake, fake, 1, 0, 2, fake, 10, None), b"mq_pack_pairs_xlmr: null pointer")
    refused(lib.mq_pack_pairs_xlmr(fake, 3, fake, 1, fake, fake, fake, 1, 0, 2, fake, 10, None), b"mq_pack_pairs_xlmr: bad shape")
    head = L.ScoreHeadWeights(pooler_w=fake, pooler_b=fake, cls_w=fake, cls_b=0.0, type_vocab=1)
    cfg = L.BertCfg(enc=L.EncoderCfg(width=128, layers=2, heads=2, mlp_dim=256, act=1, post_ln=1, mask=0, ln_eps=1e-5), vocab=100, max_pos=64, pool=1)
    w = L.BertWeights(word_emb=fake, pos_emb=fake, type_emb=fake, emb_ln_g=fake, emb_ln_b=fake)
    n = lib.mq_score_pairs_workspace_bytes(C.byref(cfg), 100, 3)
    cu = np.asarray([0, 65], dtype=np.int32)          # one sequence beyond the 64 usable positions
    refused(lib.mq_score_pairs_xlmr(C.byref(cfg), C.byref(w), C.byref(head), fake, fake, cu.ctypes.data, 1, fake, None, None, fake, n, None),
            b"mq_score_pairs_xlmr: sequence lengths must be in [1, max_pos=64]")
    cfg.enc.precision = L.MQ_PREC_FP8
    refused(lib.mq_score_pairs_xlmr(C.byref(cfg), C.byref(w), C.byref(head), fake, fake, fake, 1, fake, None, None, fake, n, None),
            b"mq_score_pairs_xlmr: bf16 encoders only")

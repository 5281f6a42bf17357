"""GPT-2 / RoBERTa byte-level BPE without a GPU: the product algorithm (csrc/tokenize_algo.h, compiled with g++ from
csrc/tokenize_byte_bpe_host.cpp) against the host tokeniser of record and against transformers.RobertaTokenizer, the table builder's refusals,
the scope test, and what the loaders pick for a directory with vocab.json + merges.txt.  On the parent of this feature there is no host source,
no table builder, and the loaders refuse or crash on such a directory."""
import json
import os
import shutil

import numpy as np
import pytest
import regex

from tests import byte_bpe_ref as BR
from marqo_amd.engine import rerank as ER
from marqo_amd.engine.tokenizers import RobertaBpeTokenizer, _byte_to_unicode

MAX_LENGTHS = (512, 16, 3, 2)
FUZZ_N = 5000
HOST_SHARE_CAP = 0.02


@pytest.fixture(scope="module")
def tok_dir(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("byte_bpe"))
    BR.write_tokenizer_files(d)
    return d


@pytest.fixture(scope="module")
def tok(tok_dir):
    return RobertaBpeTokenizer(tok_dir)


@pytest.fixture(scope="module")
def algo(tok, tmp_path_factory):
    return BR.HostAlgorithm(tok, tmp_path_factory.mktemp("byte_bpe_so"))


@pytest.fixture(scope="module")
def fuzz():
    return BR.fuzz_texts(1234, FUZZ_N)


# ---- the algorithm ------------------------------------------------------------------------------------------------------------------------------
def test_vocabulary_is_as_the_tests_assume(tok):
    vocab, merges = BR.trained()
    assert len(merges) == BR.N_MERGES and (tok.cls_id, tok.pad_id, tok.sep_id, tok.unk_id) == (BR.CLS, BR.PAD, BR.SEP, BR.UNK)
    assert all(u in vocab for u in _byte_to_unicode().values()) and "<mask>" in vocab
    assert any(len(m[0] + m[1]) >= 4 for m in merges), "merges of merges exist"


def test_whitespace_table_of_the_issue_is_what_regex_says():
    for text, want in BR.WHITESPACE_CASES.items():
        assert regex.findall(RobertaBpeTokenizer.PAT, text) == want, repr(text)


def test_host_algorithm_equals_the_host_tokeniser_on_fixed_cases(tok, algo):
    bad = []
    for text in BR.FIXED_CASES:
        for ml in MAX_LENGTHS:
            got, st = algo.encode(text, ml)
            want = tok.encode(text, ml)
            if st != 0 or got != want:
                bad.append((text, ml, st, got, want))
    assert not bad, bad[:3]
    # the cases say what they are meant to say
    assert tok.encode("I'll")[1:-1] == tok.encode("I")[1:-1] + tok.encode("'ll")[1:-1]
    assert tok.encode("I'LL")[1:-1] == tok.encode("I")[1:-1] + tok.encode("'")[1:-1] + tok.encode("LL")[1:-1]
    assert regex.findall(tok.PAT, "1234567890 42nd") == ["1234567890", " 42", "nd"], "a run of digits is one pre-token"
    assert any(len(tok.encode(t, 512)) > 16 for t in BR.FIXED_CASES) and all(len(algo.encode(t, 3)[0]) <= 3 for t in BR.FIXED_CASES)


def test_pre_token_length_limit(tok, algo):
    """128 bytes stay on the device route, 129 report MQ_TOK_NEEDS_HOST (at every max_length: the pre-token is the text's first)"""
    assert [len(t.encode()) for t in regex.findall(tok.PAT, BR.LONG_OK)][0] == 128
    assert [len(t.encode()) for t in regex.findall(tok.PAT, BR.LONG_HOST)][0] == 129
    for ml in MAX_LENGTHS:
        got, st = algo.encode(BR.LONG_OK, ml)
        assert st == 0 and got == tok.encode(BR.LONG_OK, ml)
        assert algo.encode(BR.LONG_HOST, ml) == ([], BR.NEEDS_HOST)
    # a leading space counts: " " + 128 letters is a pre-token of 129 bytes
    assert algo.encode("x " + "a" * 128, 512) == ([], BR.NEEDS_HOST)
    # beyond the kept ids an over-long pre-token no longer matters: the first ids are the host's
    got, st = algo.encode("fox dog " + "a" * 300, 4)
    assert st == 0 and got == tok.encode("fox dog " + "a" * 300, 4)
    # out of the table / malformed
    assert algo.encode("a \U00030000 b", 512) == ([], BR.NEEDS_HOST) and algo.encode("a \U0010ffff", 512) == ([], BR.NEEDS_HOST)


def test_host_algorithm_equals_the_host_tokeniser_on_the_fuzz(tok, algo, fuzz):
    assert len(fuzz) >= 5000
    routed, bad = 0, []
    for i, text in enumerate(fuzz):
        if not _in_scope(tok, text):
            continue
        for ml in (MAX_LENGTHS if i % 8 == 0 else (512, 16)):
            got, st = algo.encode(text, ml)
            if st != 0:
                routed += ml == 512
                continue
            if got != tok.encode(text, ml):
                bad.append((text, ml, got, tok.encode(text, ml)))
    share = routed / len(fuzz)
    print(f"byte-level BPE fuzz: {routed} of {len(fuzz)} texts ({100 * share:.3f} %) came back NEEDS_HOST at max_length 512 (cap {100 * HOST_SHARE_CAP:.0f} %)")
    assert not bad, bad[:3]
    assert share <= HOST_SHARE_CAP
    scripts = {"cjk": "\u6771", "cyrillic": "\u0431", "arabic": "\u0627", "emoji": "\U0001f600", "marks": "\u0301"}
    for name, ch in scripts.items():
        assert sum(ch in t for t in fuzz) >= 20, f"the fuzz has too few {name} texts"


def _in_scope(tok, text):
    from marqo_amd.engine.gpu_tokenizers import byte_bpe_in_scope
    return byte_bpe_in_scope(tok, text)


def test_against_transformers(tok_dir, tok, algo, fuzz):
    """the third-party definition over the same files: a few hundred fuzz texts and the fixed cases"""
    hf = BR.hf_tokenizer(tok_dir)
    texts = [t for t in BR.FIXED_CASES + [BR.LONG_OK] + fuzz[:400] if _in_scope(tok, t)]
    assert len(texts) >= 400
    bad = []
    for text in texts:
        for ml in (512, 16):
            want = hf(text, truncation=True, max_length=ml)["input_ids"]
            got, st = algo.encode(text, ml)
            if st != 0 or got != want or tok.encode(text, ml) != want:
                bad.append((text, ml, st, got, want))
    assert not bad, bad[:3]


# ---- the table builder ------------------------------------------------------------------------------------------------------------------------------
def _tok_from(tmp_path, name, vocab, merges):
    d = tmp_path / name
    d.mkdir()
    (d / "vocab.json").write_text(json.dumps(vocab), encoding="utf-8")
    (d / "merges.txt").write_text("#version: 0.2\n" + "\n".join(" ".join(m) for m in merges) + "\n", encoding="utf-8")
    return RobertaBpeTokenizer(str(d))


def test_table_builder_refusals(tmp_path):
    from marqo_amd.engine.gpu_tokenizers import build_byte_bpe_table
    vocab, merges = BR.trained()
    t = build_byte_bpe_table(_tok_from(tmp_path, "ok", vocab, merges))
    assert t["byte_id"].shape == (256,) and t["byte_id"].dtype == np.uint16 and int((t["slots"]["key"] != 0xffffffff).sum()) == len(set(merges))
    big = dict(vocab)
    big.update({f"filler{i}": len(vocab) + i for i in range(70000 - len(vocab))})
    assert len(big) == 70000
    with pytest.raises(ValueError, match="at most 65535"):
        build_byte_bpe_table(_tok_from(tmp_path, "big", big, merges))
    b2u = _byte_to_unicode()
    unused = next(b for b in range(256) if not any(b2u[b] in m[0] + m[1] for m in merges))
    with pytest.raises(ValueError, match=f"byte 0x{unused:02x}"):
        build_byte_bpe_table(_tok_from(tmp_path, "nobyte", {k: v for k, v in vocab.items() if k != b2u[unused]}, merges))
    result = "".join(merges[-1])
    with pytest.raises(ValueError, match="is not in vocab.json"):
        build_byte_bpe_table(_tok_from(tmp_path, "noresult", {k: v for k, v in vocab.items() if k != result}, merges))


def test_scope(tok):
    from marqo_amd.engine.gpu_tokenizers import byte_bpe_in_scope
    for text in ("a <s> b", "x</s>y", "fill the <mask> in", "<pad>", "<unk>"):
        assert not byte_bpe_in_scope(tok, text), text
    for text in ("< s >", "a < b > c", "<S>", "</ s>", "plain", ""):
        assert byte_bpe_in_scope(tok, text), text
    assert not byte_bpe_in_scope(tok, "lone \ud800 surrogate")


def test_unicode_table_of_the_gpt2_kind():
    from marqo_amd.engine import gpu_tokenizers as GT
    tab = GT.build_unicode_table("gpt2", False)
    flags = (tab & np.uint64(0xff)).astype(np.int64)
    host = np.nonzero(flags & GT.U_HOST)[0]
    assert host.min() == 0xD800 and host.max() == 0xDFFF and host.size == 0x800, "only the surrogates go to the host"
    for ch, want in ((" ", GT.U_WS), ("\u00a0", GT.U_WS), ("\u3000", GT.U_WS), ("\x1c", 0), ("\x85", GT.U_WS), ("a", GT.U_LETTER),
                     ("\u00df", GT.U_LETTER), ("\u6771", GT.U_LETTER), ("7", GT.U_NUMBER), ("\u00bd", GT.U_NUMBER), ("\u0663", GT.U_NUMBER), ("!", 0),
                     ("\u0301", 0), ("\u200b", 0), ("\x00", 0)):
        assert int(flags[ord(ch)]) == want, repr(ch)
        assert bool(regex.match(r"\s", ch)) == (want == GT.U_WS)


# ---- the loaders ------------------------------------------------------------------------------------------------------------------------------------
class _Captured(Exception):
    pass


@pytest.fixture(scope="module")
def ce_dir(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("roberta_ce"))
    BR.write_cross_encoder_dir(d, seed=0)
    return d


def test_cross_encoder_loader_takes_a_byte_bpe_roberta(ce_dir, monkeypatch, tmp_path):
    seen = {}

    def init(self, arch, sd, device, tokenizer, model_max_length=512, family=ER.BERT):
        seen.update(arch=arch, tokenizer=tokenizer, model_max_length=model_max_length, family=family)
        raise _Captured()
    monkeypatch.setattr(ER.CrossEncoderTower, "__init__", init)
    with pytest.raises(_Captured):
        ER.CrossEncoderTower.from_dir(ce_dir, "cuda:0")
    a = seen["arch"]
    assert seen["family"] is ER.XLMR and isinstance(seen["tokenizer"], RobertaBpeTokenizer)
    assert (a.pos_offset, a.type_vocab, a.max_pos, a.width) == (2, 1, BR.XR.USABLE, 128) and a.vocab == seen["tokenizer"].vocab_size
    # the same files under model_type xlm-roberta
    seen.clear()
    xl = str(tmp_path / "xl")
    shutil.copytree(ce_dir, xl)
    cfg = json.load(open(os.path.join(xl, "config.json")))
    cfg["model_type"] = "xlm-roberta"
    json.dump(cfg, open(os.path.join(xl, "config.json"), "w"))
    with pytest.raises(_Captured):
        ER.CrossEncoderTower.from_dir(xl, "cuda:0")
    assert seen["family"] is ER.XLMR and isinstance(seen["tokenizer"], RobertaBpeTokenizer)
    # add_prefix_space: refused before the constructor, in the words the older refusals use
    seen.clear()
    ps = str(tmp_path / "prefix")
    shutil.copytree(ce_dir, ps)
    BR.write_tokenizer_files(ps, add_prefix_space=True)
    with pytest.raises(ValueError, match=r"byte-level BPE tokeniser \(vocab.json \+ merges.txt\) is not served as a cross-encoder: .*add_prefix_space"):
        ER.CrossEncoderTower.from_dir(ps, "cuda:0")
    nov = str(tmp_path / "novocab")
    shutil.copytree(ce_dir, nov)
    os.remove(os.path.join(nov, "vocab.json"))
    with pytest.raises(ValueError, match="byte-level BPE tokeniser.*is not served as a cross-encoder: vocab.json or merges.txt is not there"):
        ER.CrossEncoderTower.from_dir(nov, "cuda:0")
    assert not seen, "a refused directory reached the constructor"


def test_hf_loader_takes_a_byte_bpe_roberta(tmp_path, monkeypatch):
    from marqo_amd.engine import towers
    from marqo_amd.s2_inference.errors import InvalidModelPropertiesError
    from marqo_amd.s2_inference.hugging_face_model import HuggingFaceModel
    d = str(tmp_path / "enc")
    BR.write_encoder_dir(d, seed=0)
    seen = {}

    def init(self, arch, sd, device, pooling="mean", precision="bf16"):
        seen.update(arch=arch, sd=sd, pooling=pooling)
        raise _Captured()
    monkeypatch.setattr(towers.BertTower, "__init__", init)
    props = {"type": "hf", "name": d, "dimensions": 128, "tokens": 32}
    m = HuggingFaceModel(model_properties=props, device="cuda:0")
    with pytest.raises(_Captured):
        m._load_necessary_components()
    assert isinstance(m._tokenizer, RobertaBpeTokenizer) and seen["arch"].pos_offset == 2 and seen["arch"].vocab == m._tokenizer.vocab_size
    assert "embeddings.word_embeddings.weight" in seen["sd"] and seen["pooling"] == "mean"
    seen.clear()
    ps = str(tmp_path / "prefix")
    shutil.copytree(d, ps)
    BR.write_tokenizer_files(ps, add_prefix_space=True)
    m = HuggingFaceModel(model_properties=dict(props, name=ps), device="cuda:0")
    with pytest.raises(InvalidModelPropertiesError, match="add_prefix_space"):
        m._load_necessary_components()
    assert not seen

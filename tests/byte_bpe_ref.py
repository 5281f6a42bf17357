"""Fixtures and oracles of the GPT-2 / RoBERTa byte-level BPE tests (tests/test_byte_bpe_host.py, tests/test_byte_bpe_gpu.py).  A plain helper
module: nothing here calls the library.

VOCABULARY.  A byte-level BPE of N_MERGES merges trained here (train_byte_level_bpe, the trainer tests/test_tokenizers.py uses for the host
tokeniser's own test) over a small corpus with multi-byte scripts; every one of the 256 byte symbols is in it by construction.

HOST ALGORITHM.  `HostAlgorithm` compiles marqo_amd/csrc/tokenize_byte_bpe_host.cpp with g++ (the functions of csrc/tokenize_algo.h the kernels
instantiate) and feeds it the numpy tables of engine/gpu_tokenizers.py.

MODELS.  transformers' own RobertaModel / RobertaForSequenceClassification (num_labels = 1) in fp32 on the CPU at the sizes of
tests/rerank_xlmr_ref.py (width 128, 2 layers, 2 heads, FFN 256, 64 usable positions) under the same weight recipe, saved with save_pretrained
next to the trained vocab.json + merges.txt.
"""
import collections
import ctypes as C
import functools
import json
import os
import subprocess

import numpy as np
import torch

from tests import rerank_xlmr_ref as XR
from tests.test_gpu_tokenizers import _unicode_texts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_SRC = os.path.join(ROOT, "marqo_amd", "csrc", "tokenize_byte_bpe_host.cpp")
N_MERGES = 150
CLS, PAD, SEP, UNK = 0, 1, 2, 3
NEEDS_HOST = 1

WORDS = ("the quick brown fox jumps over lazy dog search engine vector index query document ranking tensor model token merge "
         "river mountain winter summer paper stone light water green silver market street number letter").split()
CORPUS = [" ".join(WORDS)] * 12 + [
    "The quick brown fox jumps over the lazy dog. It's 42 degrees, isn't it?",
    "I'll search the index; we've ranked 1000 documents, they're sorted and he'd said so.",
    "Vector search engines rank documents by the similarity of their tensors: 3.14159 != 2.71828!",
    "naïve café über straße Ærøskøbing façade smörgåsbord",
    "東京都は日本の首都です。中文汉字也在这里。",
    "Привет, мир! Это тест токенизатора на кириллице.",
    "مرحبا بكم في هذا النص العربي ١٢٣",
    "한국어 안녕하세요 서울 대학교",
    "emoji 😀😂🎉🔥 and marks é ñ ö",
    "tabs\tand\nnew lines  and   runs of   spaces ",
] * 4


def train_byte_level_bpe(corpus, n_merges):
    """a small GPT-2-style byte-level BPE (vocab.json + merges.txt contents) trained on `corpus`"""
    import regex
    from marqo_amd.engine.tokenizers import RobertaBpeTokenizer, _byte_to_unicode
    b2u = _byte_to_unicode()
    words = collections.Counter()
    for line in corpus:
        for tok in regex.findall(RobertaBpeTokenizer.PAT, line):
            words[tuple(b2u[b] for b in tok.encode("utf-8"))] += 1
    merges = []
    for _ in range(n_merges):
        pairs = collections.Counter()
        for w, c in words.items():
            for a, b in zip(w[:-1], w[1:]):
                pairs[(a, b)] += c
        if not pairs:
            break
        best = max(sorted(pairs), key=lambda p: pairs[p])
        merges.append(best)
        new = collections.Counter()
        for w, c in words.items():
            out, i = [], 0
            while i < len(w):
                if i + 1 < len(w) and (w[i], w[i + 1]) == best:
                    out.append(w[i] + w[i + 1])
                    i += 2
                else:
                    out.append(w[i])
                    i += 1
            new[tuple(out)] += c
        words = new
    toks = ["<s>", "<pad>", "</s>", "<unk>"] + sorted(set(b2u.values())) + ["".join(m) for m in merges] + ["<mask>"]
    seen, vocab = set(), {}
    for t in toks:
        if t not in seen:
            seen.add(t)
            vocab[t] = len(vocab)
    return vocab, merges


@functools.lru_cache(maxsize=1)
def trained():
    """(vocab, merges) of the tests' vocabulary"""
    return train_byte_level_bpe(CORPUS + [t for t in _unicode_texts(41, 200) if "\x00" not in t], N_MERGES)


def write_tokenizer_files(directory, model_max_length=512, add_prefix_space=None):
    """vocab.json + merges.txt + tokenizer_config.json of the trained vocabulary -> (vocab, merges)"""
    d = str(directory)
    os.makedirs(d, exist_ok=True)
    vocab, merges = trained()
    with open(os.path.join(d, "vocab.json"), "w", encoding="utf-8") as f:
        json.dump(vocab, f, ensure_ascii=False)
    with open(os.path.join(d, "merges.txt"), "w", encoding="utf-8") as f:
        f.write("#version: 0.2\n" + "\n".join(" ".join(m) for m in merges) + "\n")
    cfg = dict(model_max_length=model_max_length, tokenizer_class="RobertaTokenizer", bos_token="<s>", eos_token="</s>", sep_token="</s>",
               cls_token="<s>", unk_token="<unk>", pad_token="<pad>", mask_token="<mask>")
    if add_prefix_space is not None:
        cfg["add_prefix_space"] = add_prefix_space
    with open(os.path.join(d, "tokenizer_config.json"), "w") as f:
        json.dump(cfg, f)
    return vocab, merges


def hf_tokenizer(directory):
    """transformers' own RobertaTokenizer over the trained files"""
    from transformers import RobertaTokenizer
    d = str(directory)
    return RobertaTokenizer(os.path.join(d, "vocab.json"), os.path.join(d, "merges.txt"))


# ---- texts ----------------------------------------------------------------------------------------------------------------------------------------
WHITESPACE_CASES = {          # the issue's table: input -> pre-tokens (checked with `regex` in the host test)
    "a  b": ["a", " ", " b"],
    "a \n b ": ["a", " \n", " b", " "],
    "  x": [" ", " x"],
    "x \t": ["x", " \t"],
    "a\u00a0\u00a0b": ["a", "\u00a0", "\u00a0", "b"],
}
LONG_OK = "a" * 128 + " fox"                   # a pre-token of exactly 128 bytes: stays on the device route
LONG_HOST = "a" * 129 + " fox"                 # 129 bytes: MQ_TOK_NEEDS_HOST
FIXED_CASES = list(WHITESPACE_CASES) + [
    "I'll", "I'LL", "don't", "x's'", "we've they're he'd I'm 'twas 'sam", " 's", "!'s", "''ll", "it'S", "a'",
    "1234567890 42nd 3.14159 \u0661\u0662\u0663 \uff12\uff10\uff12\uff14 x\u00b2\u00b3 \u00bd", "abc123def!!!456ghi", "a1!b2?c3",
    "$100.00 (approx.) #tag @user 50%",
    "\u00a0word", "\u2003word", "\u3000word", "a\u00a0word", "a \u2003word", "a\u3000 word", "a \u00a0 \u3000  word", "a\t\u3000",
    " ", "   ", " \t\n ", "\n", "\u00a0\u2003\u3000", "",
    LONG_OK, "\u00e9" * 64 + " x", "x " + "!" * 127, " " + "z" * 127,
    "\u6771\u4eac\u90fd\u306f\u65e5\u672c\u306e\u9996\u90fd\u3067\u3059\u3002", "\u041f\u0440\u0438\u0432\u0435\u0442, \u043c\u0438\u0440! \u042d\u0442\u043e \u0442\u0435\u0441\u0442.",
    "\u0645\u0631\u062d\u0628\u0627 \u0628\u0643\u0645 \u0641\u064a \u0647\u0630\u0627 \u0627\u0644\u0646\u0635", "\U0001f600\U0001f602\U0001f389\U0001f525\U0001f44d\U0001f3fd\u2764\ufe0f\U0001f1ef\U0001f1f5",
    "e\u0301 n\u0303o\u0308 \u0301x a\u0323\u0327", "\ud55c\uad6d\uc5b4 \uc548\ub155\ud558\uc138\uc694", "\u0939\u093f\u0928\u094d\u0926\u0940 \u092d\u093e\u0937\u093e",
    "The quick brown fox jumps over the lazy dog.", "  leading and trailing  ", "tabs\tand\nnewlines\r\n",
    "< s > <notmask> a<b", "UPPER lower MiXeD", "\x00a\x07b\x7f", "a\ufffdb\u200b\u00adc\ufeff", "\x1c\x1d x\x85y\u2028z",
]


def fuzz_texts(seed, n):
    """the seeded multi-script texts of tests/test_gpu_tokenizers.py (words of one to eight characters from seventeen scripts, joined by spaces,
    punctuation, apostrophes, nothing): a pre-token of more than 128 bytes needs six or more 3-byte words glued by the empty separator"""
    return _unicode_texts(seed, n)


# ---- the host build of the product algorithm ----------------------------------------------------------------------------------------------------------
class _HostVocab(C.Structure):
    _fields_ = [("slots", C.c_void_p), ("byte_id", C.c_void_p), ("unicode", C.c_void_p), ("n_slots", C.c_uint32), ("cls_id", C.c_int32),
                ("sep_id", C.c_int32), ("pad_id", C.c_int32)]


class HostAlgorithm:
    """mq_host_byte_bpe over the numpy tables of a RobertaBpeTokenizer"""

    def __init__(self, tok, build_dir):
        from marqo_amd.engine.gpu_tokenizers import build_byte_bpe_table, build_unicode_table
        so = os.path.join(str(build_dir), "libbytebpe.so")
        subprocess.run(["g++", "-O2", "-fPIC", "-std=c++17", "-Wall", "-Werror", "-shared", "-o", so, HOST_SRC], check=True)
        self.lib = C.CDLL(so)
        self.lib.mq_host_byte_bpe.restype = C.c_int
        self.lib.mq_host_byte_bpe.argtypes = [C.POINTER(_HostVocab), C.c_char_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        t = build_byte_bpe_table(tok)
        self._keep = (np.ascontiguousarray(t["slots"]), np.ascontiguousarray(t["byte_id"]), np.ascontiguousarray(build_unicode_table("gpt2", False)))
        self.vocab = _HostVocab(slots=self._keep[0].ctypes.data, byte_id=self._keep[1].ctypes.data, unicode=self._keep[2].ctypes.data,
                                n_slots=t["n_slots"], cls_id=t["cls_id"], sep_id=t["sep_id"], pad_id=t["pad_id"])
        self.pad_id = t["pad_id"]

    def encode(self, text, max_length):
        """-> (ids without the padding, status); the row is checked to be padded with <pad> up to ld = max_length + 3 and not beyond"""
        data = text.encode("utf-8")
        ld = max_length + 3
        row = np.full(ld + 4, -7, dtype=np.int32)
        st = np.full(1, -1, dtype=np.int32)
        n = self.lib.mq_host_byte_bpe(C.byref(self.vocab), data, len(data), max_length, row.ctypes.data, ld, st.ctypes.data)
        assert (row[ld:] == -7).all(), "a word beyond the row changed"
        if int(st[0]) != 0:
            assert n == 0
            return [], int(st[0])
        assert 2 <= n <= max_length and (row[n:ld] == self.pad_id).all(), (text, n, row)
        return row[:n].tolist(), 0


# ---- tiny checkpoints ---------------------------------------------------------------------------------------------------------------------------------
def config(vocab, num_labels=1):
    from transformers import RobertaConfig
    s = XR.SHAPE
    return RobertaConfig(vocab_size=vocab, hidden_size=s["W"], num_hidden_layers=s["layers"], num_attention_heads=s["heads"],
                         intermediate_size=s["mlp"], max_position_embeddings=s["max_pos"], type_vocab_size=1, pad_token_id=s["pad"],
                         bos_token_id=0, eos_token_id=2, layer_norm_eps=1e-5, hidden_act="gelu", num_labels=num_labels)


def write_cross_encoder_dir(directory, seed=0, model_max_length=512, add_prefix_space=None):
    """a local RobertaForSequenceClassification directory (model_type roberta; save_pretrained + the trained tokeniser files) -> the model"""
    from transformers import RobertaForSequenceClassification
    vocab, _ = write_tokenizer_files(directory, model_max_length, add_prefix_space)
    model = RobertaForSequenceClassification(config(len(vocab))).eval()
    missing, unexpected = model.load_state_dict(XR.state_dict(len(vocab), seed), strict=False)
    assert not unexpected and all("position_ids" in k or "token_type_ids" in k for k in missing), (missing, unexpected)
    model.save_pretrained(str(directory), safe_serialization=True)
    return model


def write_encoder_dir(directory, seed=0, add_prefix_space=None):
    """a local RobertaModel directory (no pooling layer: a sentence-transformers RoBERTa encoder) with the same encoder weights -> the model"""
    from transformers import RobertaModel
    vocab, _ = write_tokenizer_files(directory, 512, add_prefix_space)
    model = RobertaModel(config(len(vocab)), add_pooling_layer=False).eval()
    sd = {k[len("roberta."):]: v for k, v in XR.state_dict(len(vocab), seed).items() if k.startswith("roberta.")}
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and all("position_ids" in k or "token_type_ids" in k for k in missing), (missing, unexpected)
    model.save_pretrained(str(directory), safe_serialization=True)
    return model


def mean_pooled(model, rows):
    """the fp32 encoder on unpadded id lists -> mean over the tokens, L2-normalised, float64 [n, W]"""
    n, S = len(rows), max(len(r) for r in rows)
    ids = torch.full((n, S), PAD, dtype=torch.int64)
    mask = torch.zeros((n, S), dtype=torch.int64)
    for i, r in enumerate(rows):
        ids[i, :len(r)] = torch.tensor(r, dtype=torch.int64)
        mask[i, :len(r)] = 1
    with torch.no_grad():
        h = model(input_ids=ids, attention_mask=mask).last_hidden_state.double()
    m = mask.double()[:, :, None]
    e = (h * m).sum(1) / m.sum(1)
    return (e / e.norm(dim=-1, keepdim=True)).numpy()


def text_of(k, seed):
    g = np.random.default_rng(seed)
    return " ".join(WORDS[int(i)] for i in g.integers(0, len(WORDS), k))

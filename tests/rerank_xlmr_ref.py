"""Oracle and fixtures of the XLM-RoBERTa cross-encoder tests (tests/test_rerank_xlmr_host.py, tests/test_rerank_xlmr_gpu.py).  A plain helper
module: nothing here calls the library.

ORACLE.  transformers' own XLMRobertaForSequenceClassification (num_labels = 1) in fp32 on the CPU, built from a tiny config (width 128, 2 layers,
2 heads of 64, FFN 256, max_position_embeddings = 66: 64 usable positions at pad_token_id = 1) and written with save_pretrained, so the weight
names in the directory are the ones transformers gives them.  Its weights are engine.synthetic.cross_encoder_state_dict's under RoBERTa's names
(the recipe tests/rerank_ref.py uses for the BERT head: peaky attention, tanh neither linear nor saturated, classifier weights 8 / sqrt(W), so
logits of unrelated pairs spread), which is what lets the BERT test's logit bound carry over.

VOCABULARY.  The SentencePiece unigram model of tests/test_gpu_tokenizers.py's `sp_model` fixture, trained by the same call on the same corpus.

PAIR IDS.  The fast tokenizer's pair call (truncation="longest_first") where `tokenizers` can convert the fixture's SentencePiece model
(`fast_tokenizer` returns None where it cannot); otherwise `pair_ids_rule`, a NumPy statement of LongestFirst with B = max_length - 4 over the
slow tokeniser's pieces.  `PAIR_ORACLE` says which of the two ran.
"""
import json
import os

import numpy as np
import torch

from tests.test_gpu_tokenizers import _unicode_texts
from tests.test_tokenizers import CORPUS, SENTENCES

SHAPE = dict(W=128, layers=2, heads=2, mlp=256, max_pos=66, pad=1)
USABLE = SHAPE["max_pos"] - SHAPE["pad"] - 1          # 64
CLS, PAD, SEP = 0, 1, 2                               # <s> <pad> </s>: the fairseq layout
PAIR_ORACLE = None                                    # "fast tokenizer" | "numpy rule": set by pair_oracle()


# ---- vocabulary ---------------------------------------------------------------------------------------------------------------------------
def train_sentencepiece(directory):
    """-> directory/sentencepiece.bpe.model: the call of tests/test_gpu_tokenizers.py::sp_model"""
    import sentencepiece as spm
    d = str(directory)
    os.makedirs(d, exist_ok=True)
    corpus = [" ".join(CORPUS)] * 20 + SENTENCES[:6] * 5 + _unicode_texts(41, 600)
    with open(os.path.join(d, "c.txt"), "w", encoding="utf-8") as f:
        f.write("\n".join(t.replace("\n", " ").replace("\x00", "") for t in corpus))
    spm.SentencePieceTrainer.train(input=os.path.join(d, "c.txt"), model_prefix=os.path.join(d, "sentencepiece.bpe"), vocab_size=600,
                                   model_type="unigram", character_coverage=0.98, hard_vocab_limit=False, minloglevel=2)
    os.remove(os.path.join(d, "c.txt"))
    return os.path.join(d, "sentencepiece.bpe.model")


def one_piece_words(tok):
    """the ASCII words of CORPUS that the tokeniser keeps as ONE piece: a text of k of them has exactly k pieces"""
    words = sorted({w for w in CORPUS if w.isascii() and w.isalpha()})
    return [w for w in words if len(tok.encode(w)) == 3]


def text_of(words, k, seed):
    g = np.random.default_rng(seed)
    return " ".join(words[int(i)] for i in g.integers(0, len(words), k))


def sentences(words, n_words, seed):
    """n_words one-piece words with a full stop after every fifth (more pieces: the stop is its own)"""
    g = np.random.default_rng(seed)
    out = [words[int(g.integers(0, len(words)))] + ("." if k % 5 == 4 or k == n_words - 1 else "") for k in range(n_words)]
    return " ".join(out)


# ---- checkpoint directory ---------------------------------------------------------------------------------------------------------------------
def roberta_names(sd):
    """engine.synthetic.cross_encoder_state_dict (BertForSequenceClassification names) -> XLMRobertaForSequenceClassification names: the pooler
    becomes classifier.dense, the classifier classifier.out_proj, and one token-type row is kept"""
    out = {}
    for k, v in sd.items():
        if k.startswith("bert.pooler.dense."):
            out["classifier.dense." + k.rsplit(".", 1)[1]] = v
        elif k.startswith("classifier."):
            out["classifier.out_proj." + k.rsplit(".", 1)[1]] = v
        elif k == "bert.embeddings.token_type_embeddings.weight":
            out["roberta.embeddings.token_type_embeddings.weight"] = v[:1].clone()
        else:
            out["roberta." + k[len("bert."):]] = v
    return out


def config(vocab, num_labels=1):
    from transformers import XLMRobertaConfig
    s = SHAPE
    return XLMRobertaConfig(vocab_size=vocab, hidden_size=s["W"], num_hidden_layers=s["layers"], num_attention_heads=s["heads"],
                            intermediate_size=s["mlp"], max_position_embeddings=s["max_pos"], type_vocab_size=1, pad_token_id=s["pad"],
                            bos_token_id=0, eos_token_id=2, layer_norm_eps=1e-5, hidden_act="gelu", num_labels=num_labels)


def state_dict(vocab, seed=0):
    from marqo_amd.engine import synthetic
    s = SHAPE
    return roberta_names(synthetic.cross_encoder_state_dict(s["W"], s["layers"], s["heads"], s["mlp"], vocab=vocab, seed=seed, max_pos=s["max_pos"]))


def write_dir(directory, seed=0, model_max_length=512, stray_pooler=False):
    """a local XLMRobertaForSequenceClassification directory (save_pretrained + the SentencePiece model + tokenizer_config.json) -> the model.
    stray_pooler: the weights file also carries roberta.pooler.dense.*, as checkpoints converted from an encoder with a pooling layer do;
    transformers builds the model with add_pooling_layer=False and does not read them."""
    from transformers import XLMRobertaForSequenceClassification
    from marqo_amd.engine.tokenizers import XlmRobertaTokenizer
    d = str(directory)
    train_sentencepiece(d)
    vocab = XlmRobertaTokenizer(d).vocab_size
    model = XLMRobertaForSequenceClassification(config(vocab)).eval()
    missing, unexpected = model.load_state_dict(state_dict(vocab, seed), strict=False)
    assert not unexpected and all("position_ids" in k or "token_type_ids" in k for k in missing), (missing, unexpected)
    model.save_pretrained(d, safe_serialization=True)
    if stray_pooler:
        from safetensors.torch import load_file, save_file
        g = torch.Generator().manual_seed(seed + 31)
        W = SHAPE["W"]
        sd = load_file(os.path.join(d, "model.safetensors"))
        sd["roberta.pooler.dense.weight"] = torch.randn(W, W, generator=g) / W ** 0.5
        sd["roberta.pooler.dense.bias"] = torch.randn(W, generator=g)
        save_file(sd, os.path.join(d, "model.safetensors"), metadata={"format": "pt"})
    with open(os.path.join(d, "tokenizer_config.json"), "w") as f:
        json.dump(dict(model_max_length=model_max_length, tokenizer_class="XLMRobertaTokenizer", bos_token="<s>", eos_token="</s>", sep_token="</s>",
                       cls_token="<s>", unk_token="<unk>", pad_token="<pad>", mask_token="<mask>"), f)
    return model


def load_model(directory):
    from transformers import XLMRobertaForSequenceClassification
    return XLMRobertaForSequenceClassification.from_pretrained(str(directory), torch_dtype=torch.float32).eval()


# ---- pair ids ----------------------------------------------------------------------------------------------------------------------------------
def fast_tokenizer(directory):
    """XLMRobertaTokenizerFast over the directory's SentencePiece model, or None where `tokenizers` cannot convert it"""
    try:
        from transformers import XLMRobertaTokenizerFast
        tok = XLMRobertaTokenizerFast.from_pretrained(str(directory))
        tok(["a"], ["b"], truncation="longest_first", max_length=8)
        return tok
    except Exception:  # noqa: BLE001  (no converter, no protobuf, ...: the rule below stands in)
        return None


def longest_first(la, lb, max_length):
    """the `tokenizers` library's LongestFirst on a pair with FOUR specials, written out on its own: B = max_length - 4"""
    B = max_length - 4
    assert B >= 1
    if la + lb <= B:
        return la, lb
    swap = la > lb                                  # n1 = the shorter; on a tie the first text
    n1, n2 = (lb, la) if swap else (la, lb)
    n2 = n1 if n1 > B else max(n1, B - n1)
    if n1 + n2 > B:
        n1 = B // 2
        n2 = B - n1
    return (n2, n1) if swap else (n1, n2)


def pair_ids_rule(tok, query, docs, max_length):
    """<s> q[:a] </s> </s> d[:b] </s> over the slow tokeniser's pieces (XlmRobertaTokenizer.encode = <s> pieces </s>)"""
    q = tok.encode(query)[1:-1]
    out = []
    for d in docs:
        p = tok.encode(d)[1:-1]
        a, b = longest_first(len(q), len(p), max_length)
        out.append([CLS, *q[:a], SEP, SEP, *p[:b], SEP])
    return out


def pair_oracle(directory, tok):
    """-> f(query, docs, max_length) = list of id lists; sets PAIR_ORACLE to the name of what runs"""
    global PAIR_ORACLE
    fast = fast_tokenizer(directory)
    if fast is not None:
        PAIR_ORACLE = "fast tokenizer"
        return lambda query, docs, max_length: fast([query] * len(docs), list(docs), truncation="longest_first", max_length=max_length)["input_ids"]
    PAIR_ORACLE = "numpy rule"
    return lambda query, docs, max_length: pair_ids_rule(tok, query, docs, max_length)


def hf_forward(model, seqs):
    """the fp32 model on unpadded id lists, right-padded with <pad> and masked as the tokenizer's padding=True does -> (logits float64 [n],
    final <s> rows float64 [n, W])"""
    n, S = len(seqs), max(len(s) for s in seqs)
    ids = torch.full((n, S), PAD, dtype=torch.int64)
    mask = torch.zeros((n, S), dtype=torch.int64)
    for i, s in enumerate(seqs):
        ids[i, :len(s)] = torch.tensor(s, dtype=torch.int64)
        mask[i, :len(s)] = 1
    with torch.no_grad():
        out = model(input_ids=ids, attention_mask=mask, output_hidden_states=True)
    return out.logits[:, 0].double().numpy(), out.hidden_states[-1][:, 0].double().numpy()


# ---- a canned search result -----------------------------------------------------------------------------------------------------------------------
CANNED_SEED = 18         # chosen on the CPU: the oracle's logits decide every hit's best chunk and the order of the hits by more than 0.53


def canned_search(words, seed=None):
    """(query, hits): four hits with a one-chunk `title` and a `body` of six capitalised five-word sentences (three chunks of two sentences)"""
    seed = CANNED_SEED if seed is None else seed
    query = sentences(words, 5, 5000 + seed)
    hits = [{"_id": f"doc{i}", "title": sentences(words, 5 + i, 6000 + 10 * seed + i).capitalize(),
             "body": " ".join(sentences(words, 5, 7000 + 100 * seed + 10 * i + j).capitalize() for j in range(6)), "_score": 0.5 + 0.01 * i}
            for i in range(4)]
    return query, hits

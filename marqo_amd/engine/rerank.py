"""Cross-encoder scoring for text reranking: (query, passage) pairs through the BERT tower and a one-logit head (csrc/rerank.hip).

The reference scores pairs with sentence-transformers' `CrossEncoder` (s2_inference/reranking/model_utils.py load_sbert_cross_encoder_model),
i.e. a Hugging Face `*ForSequenceClassification` with num_labels = 1 behind the fast tokenizer's pair call (`truncation="longest_first"`).
Two families are served (`_Family`): BERT (WordPiece, [CLS] a [SEP] b [SEP], two type rows, pooler + classifier) and XLM-RoBERTa /
RoBERTa with a SentencePiece model or with GPT-2's byte-level BPE (<s> a </s> </s> b </s>, one type row, position ids from padding_idx + 1,
classifier.dense + classifier.out_proj).
The texts are tokenised once on the GPU (engine/gpu_tokenizers.py), paired, truncated and packed there (mq_pair_plan_n / mq_pack_pairs |
mq_pack_pairs_xlmr), and every batch is ONE mq_score_pairs_bert | mq_score_pairs_xlmr call.
A third family runs on the ModernBERT tower (ModernBertCrossEncoderTower: `ModernBertForSequenceClassification`, [CLS] a [SEP] b [SEP], mean or CLS
pooling, dense -> GELU -> LayerNorm -> classifier; one mq_score_pairs_modernbert call per batch).  Its texts are tokenised once on the HOST, by the
`tokenizers` library from the checkpoint's tokenizer.json; pairing, truncation and packing are the same GPU calls.  A fourth runs on the DeBERTa tower
(DebertaCrossEncoderTower: `DebertaV2ForSequenceClassification`, [CLS] a [SEP] b [SEP], disentangled attention, ContextPooler head; one
mq_score_pairs_deberta call per batch), tokenised on the host in the same way.  What the towers share — the length cap, the longest-first order, the
batch loop — is `_PairScorer.score`.  A fifth is a decoder: the Qwen3 rerankers (QwenRerankerTower: `Qwen3ForCausalLM` judged by yes / no or its one-logit
`Qwen3ForSequenceClassification` conversion, the model card's chat template, tokenised on the host; one mq_score_qwen_pairs call per batch in which the
system prompt, the instruction and the query — the same for every document under the causal mask — are computed once).  A sixth is Gemma-2B
(GemmaRerankerTower: BAAI/bge-reranker-v2-gemma, `GemmaForCausalLM` judged by the logit of `Yes`, or its one-logit `GemmaForSequenceClassification`
conversion; FlagEmbedding's piecewise-tokenised input, on the host; one mq_score_gemma_pairs call per batch with `[bos] A: query` computed once).
`load_cross_encoder_tower` picks the class from a directory's config.json.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import json
import os
import threading
import unicodedata
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from marqo_amd import _lib as L
from marqo_amd.engine import archs, checkpoint
from marqo_amd.engine.deberta import DebertaTower
from marqo_amd.engine.modernbert import ModernBertTower
from marqo_amd.engine.qwen import QwenTower
from marqo_amd.engine.tokenizers import HfJsonTokenizer, RobertaBpeTokenizer, WordPieceTokenizer, XlmRobertaTokenizer
from marqo_amd.engine.tower_weights import gemma_causal_state_dict, modernbert_head_tensors
from marqo_amd.engine.towers import BertTower, _PackedTextTower, _check_precision, _large_call, _need, request_stream

Tensor = torch.Tensor


@dataclasses.dataclass(frozen=True)
class _Family:
    """what differs between the cross-encoder families: everything else of CrossEncoderTower is shared"""
    name: str
    prefix: str           # of the encoder's weights
    dense: str            # head: tanh(Linear) on the final first row ...
    out: str              # ... and the one-logit Linear on it
    specials: int         # special tokens of a packed pair
    typed: bool           # the pack kernel writes token-type ids and the scoring call looks the type row up per token


BERT = _Family("bert", "bert.", "bert.pooler.dense", "classifier", specials=3, typed=True)
# RobertaClassificationHead: classifier.dense -> tanh -> classifier.out_proj on the final <s> row; the encoder has no pooler
XLMR = _Family("xlm-roberta", "roberta.", "classifier.dense", "classifier.out_proj", specials=4, typed=False)


def pair_lengths(la, lb, max_length: int, specials: int = 3):
    """Pieces (a, b) that the `tokenizers` library's LongestFirst truncation keeps of a pair with la and lb pieces when the sequence
    [CLS] a [SEP] b [SEP] (`specials` = 3; <s> a </s> </s> b </s>: 4) may hold max_length tokens (ints or integer arrays; both texts keep
    their prefix).  B = max_length - specials:
    nothing is cut when la + lb <= B.  Otherwise, with s the shorter and l the longer text (on a tie the SECOND text counts as the
    longer), l' = s when s > B, else max(s, B - s); when s + l' is still above B, s = B // 2 and l' = B - s; the longer text keeps l'.
    This is NOT the slow tokenizers' loop that removes one token at a time from the longer text."""
    if max_length < specials + 1:
        raise ValueError(f"max_length={max_length} must be at least {specials + 1}")
    scalar = np.ndim(la) == 0 and np.ndim(lb) == 0
    la, lb = np.broadcast_arrays(np.asarray(la, dtype=np.int64), np.asarray(lb, dtype=np.int64))
    B = max_length - specials
    swap = la > lb
    s = np.where(swap, lb, la)
    l = np.where(s > B, s, np.maximum(s, B - s))
    both = s + l > B
    s = np.where(both, B // 2, s)
    l = np.where(both, B - B // 2, l)
    fits = la + lb <= B
    a = np.where(fits, la, np.where(swap, l, s))
    b = np.where(fits, lb, np.where(swap, s, l))
    return (int(a), int(b)) if scalar else (a, b)


def _tokenizer_settings(directory: str, default_max: int = 512) -> Tuple[bool, int]:
    """(do_lower_case, model_max_length) of a checkpoint's tokenizer_config.json (BERT's defaults when absent; XLM-R's model_max_length
    defaults to 512 as well; ModernBERT's to what its caller passes)"""
    lower, max_len = True, default_max
    p = os.path.join(directory, "tokenizer_config.json")
    if os.path.isfile(p):
        try:
            with open(p) as f:
                j = json.load(f)
            lower = bool(j.get("do_lower_case", True))
            m = j.get("model_max_length", default_max)
            if isinstance(m, (int, float)) and 4 <= m < 1 << 20:    # (transformers writes 1e30 for "no limit")
                max_len = int(m)
        except (OSError, ValueError):
            pass
    return lower, max_len


def _byte_bpe_refusal(directory: str) -> Optional[str]:
    """why a directory's GPT-2 / RoBERTa byte-level BPE files (vocab.json + merges.txt) cannot be served, or None"""
    if not (os.path.isfile(os.path.join(directory, "vocab.json")) and os.path.isfile(os.path.join(directory, "merges.txt"))):
        return "vocab.json or merges.txt is not there"
    try:
        with open(os.path.join(directory, "vocab.json"), encoding="utf-8") as f:
            vocab = json.load(f)
    except (OSError, ValueError) as e:
        return f"vocab.json cannot be read ({e})"
    gone = [t for t in ("<s>", "<pad>", "</s>", "<unk>") if not isinstance(vocab, dict) or t not in vocab]
    if gone:
        return f"vocab.json has no {' / '.join(gone)} token"
    p = os.path.join(directory, "tokenizer_config.json")
    if os.path.isfile(p):
        try:
            with open(p) as f:
                if json.load(f).get("add_prefix_space"):
                    return "its tokenizer_config.json sets add_prefix_space, which the tokeniser here does not implement"
        except (OSError, ValueError, AttributeError):
            pass
    return None


def head_tensors(sd: Dict[str, Tensor], family: _Family, W: int) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """(dense weight [W, W], dense bias [W], out weight [1, W], out bias [1]) of a checkpoint's scoring head under the family's names"""
    return (_need(sd, family.dense + ".weight", (W, W)), _need(sd, family.dense + ".bias", (W,)),
            _need(sd, family.out + ".weight", (1, W)), _need(sd, family.out + ".bias", (1,)))


class _PairScorer:
    """score() of the cross-encoder towers: ONE query against n documents.  The tower supplies
      pair_specials                      special tokens of a packed pair
      pair_id_rows                       rows of the packed id buffer: 1, or 2 when the pack call also writes token-type ids
      tokenizer.cls_id / .sep_id         the two ids the pack call inserts
      model_max_length                   the longest pair the checkpoint takes
      _tokenize_query(query)             -> (ids int32 [1, >= len] on the device: CLS pieces SEP, its length [1]) at the query's FULL length
      _tokenize(texts, cap)              -> (ids int32 [n, cap] on the device: CLS pieces SEP pad, lengths int64 [n]), rows cut to cap tokens
      _pack_chunk(pack, d_ids, rows, stream)                        the pack call of one batch (pack: the arguments the pack entry points share)
      _score_chunk(d_ids, d_cu, cu, logits, scores, rows, m)        the scoring call of one batch of m pairs / `rows` tokens
    and _chunks / _to_device / _stream of the text towers; batches are sized by ROWS (_chunks), whatever the pairs' lengths are."""

    def score(self, query: str, docs: Sequence[str], max_length: int = 512) -> Tuple[np.ndarray, np.ndarray]:
        """-> (logits, sigmoid(logits)) fp32 [len(docs)] on the host, in the order of `docs`.  Texts are stripped as CrossEncoder strips
        them; the pair is cut to min(max_length, the tokenizer's model_max_length) tokens by `pair_lengths`.  An empty text contributes no
        piece, as in the fast tokenizer's pair call: the pair keeps all of its special tokens."""
        if not isinstance(query, str) or not all(isinstance(d, str) for d in docs):
            raise TypeError("a cross-encoder scores (str, str) pairs")
        n = len(docs)
        if n == 0:
            return np.zeros(0, np.float32), np.zeros(0, np.float32)
        specials = int(self.pair_specials)
        cap = int(min(max_length, self.model_max_length))
        if cap < specials + 1:
            raise ValueError(f"max_length={max_length} must be at least {specials + 1}")
        query, docs = query.strip(), [d.strip() for d in docs]
        lib, dev, tok = self.lib, self.device, self.tokenizer
        with request_stream(dev), torch.cuda.device(dev):
            # the query once (its full length: which text is the longer decides who loses a piece), the documents once.  A document cut
            # to cap - 2 pieces is still longer than B = cap - specials, and still at least as long as any query of <= cap - 2 pieces; for
            # a longer query the documents are read up to the query's length, which keeps every comparison of pair_lengths exact.
            d_q, qlen = self._tokenize_query(query)
            la = int(qlen[0]) - 2
            ld = cap if la <= cap - 2 else la + 2
            d_docs, dlen = self._tokenize(docs, ld)
            a, b = pair_lengths(la, dlen - 2, cap, specials)
            total = (a + b + specials).astype(np.int64)
            order = np.argsort(-total, kind="stable")          # longest first: a batch holds sequences of similar length
            inv = np.empty(n, dtype=np.int64)
            inv[order] = np.arange(n)
            sorted_total = total[order]
            d_order = self._to_device(torch.from_numpy(order))
            d_docs = d_docs.index_select(0, d_order)            # (row gather: memory movement, as torch is used throughout the engine)
            d_dlen = self._to_device(torch.from_numpy(dlen[order].astype(np.int32)))
            d_query = d_q[0, 1:1 + max(la, 0)].contiguous()
            logits = torch.empty(n, dtype=torch.float32, device=dev)
            scores = torch.empty(n, dtype=torch.float32, device=dev)
            stream = self._stream()
            with _large_call(dev, int(sorted_total.sum())):
                for s0, s1 in self._chunks(sorted_total):
                    m = s1 - s0
                    cu_np = np.zeros(m + 1, dtype=np.int32)
                    np.cumsum(sorted_total[s0:s1], out=cu_np[1:])
                    rows = int(cu_np[-1])
                    cu = torch.from_numpy(cu_np)
                    d_cu = self._to_device(cu)
                    plan = torch.empty(3, m, dtype=torch.int32, device=dev)
                    d_ids = torch.empty(int(self.pair_id_rows), rows, dtype=torch.int32, device=dev)
                    L.check(lib.mq_pair_plan_n(la, d_dlen[s0:s1].data_ptr(), m, ld, cap, specials, plan[0].data_ptr(), plan[1].data_ptr(),
                                               plan[2].data_ptr(), stream), "mq_pair_plan_n")
                    pack = (d_query.data_ptr() if la > 0 else None, la, d_docs[s0:s1].data_ptr(), ld, plan[0].data_ptr(), plan[1].data_ptr(),
                            d_cu.data_ptr(), m, tok.cls_id, tok.sep_id, d_ids[0].data_ptr())
                    self._pack_chunk(pack, d_ids, rows, stream)
                    self._score_chunk(d_ids, d_cu, cu, logits[s0:s1], scores[s0:s1], rows, m)
            out = torch.stack((logits, scores)).cpu().numpy()
        return np.ascontiguousarray(out[0][inv]), np.ascontiguousarray(out[1][inv])


class CrossEncoderTower(_PairScorer, BertTower):
    """`BertForSequenceClassification` / `XLMRobertaForSequenceClassification` (num_labels = 1): `bert.*` | `roberta.*` = the encoder (prepared
    exactly as for the embedding towers: engine/tower_weights.py; XLM-R's position table is handed over from row padding_idx + 1 on),
    `bert.pooler.dense.*` + `classifier.*` | `classifier.dense.*` + `classifier.out_proj.*` = the head (a `roberta.pooler.*` is not read: the
    model is built with add_pooling_layer=False).  score() returns the raw logits and their sigmoid."""

    def __init__(self, arch: archs.BertArch, sd: Dict[str, Tensor], device: str, tokenizer, model_max_length: int = 512,
                 family: _Family = BERT):
        if arch.glu or arch.rope_theta is not None or arch.rel_buckets:
            raise ValueError("cross-encoders run on plain BERT encoders (model_type 'bert', 'xlm-roberta' or 'roberta')")
        if bool(arch.pos_offset) != (family is XLMR):
            raise ValueError(f"a {family.name} cross-encoder cannot have position ids that start at {arch.pos_offset}")
        if arch.type_vocab < 1:
            raise ValueError(f"type_vocab_size={arch.type_vocab}: a cross-encoder's embedding needs a token-type row")
        W = arch.width
        if W % 64 != 0 or W > 2048:
            raise ValueError(f"the scoring head needs a hidden size that is a multiple of 64, at most 2048 (got {W})")
        pooler_w, pooler_b, cls_w, cls_b = head_tensors(sd, family, W)
        enc = {k[len(family.prefix):]: v for k, v in sd.items() if k.startswith(family.prefix)}
        super().__init__(arch, enc, device, pooling="cls", precision="bf16")
        h = self._h
        self.family = family
        self.head = L.ScoreHeadWeights(pooler_w=h.bf16(pooler_w), pooler_b=h.f32(pooler_b), cls_w=h.f32(cls_w.reshape(W)),
                                       cls_b=float(cls_b.detach().float().reshape(-1)[0]), type_vocab=int(arch.type_vocab))
        if _need(sd, family.prefix + "embeddings.token_type_embeddings.weight").shape != (arch.type_vocab, W):
            raise ValueError(f"token_type_embeddings must be [{arch.type_vocab}, {W}]")
        self.tokenizer = tokenizer
        self.model_max_length = int(min(model_max_length, arch.max_pos))     # (max_pos counts the usable positions: archs.BertArch)
        from marqo_amd.engine.gpu_tokenizers import DeviceByteBpeTokenizer, DeviceSentencePieceTokenizer, DeviceWordPieceTokenizer
        device_cls = DeviceWordPieceTokenizer if family is BERT else \
            DeviceByteBpeTokenizer if isinstance(tokenizer, RobertaBpeTokenizer) else DeviceSentencePieceTokenizer
        self.device_tokenizer = device_cls(tokenizer, str(self.device))
        self.tune_residual_default()      # the same load-time policy as the embedding towers, on the encoder's [CLS] rows
        self.release_unused_folded()

    @classmethod
    def from_dir(cls, directory: str, device: str) -> "CrossEncoderTower":
        """a local Hugging Face directory: config.json, model.safetensors | pytorch_model.bin, vocab.txt | sentencepiece.bpe.model |
        vocab.json + merges.txt, tokenizer_config.json"""
        cfg, sd = checkpoint.load_hf_dir(directory)
        mtype = cfg.get("model_type", "bert")
        if mtype == "modernbert":       # its own tower and head (below)
            return ModernBertCrossEncoderTower._from_loaded(directory, cfg, sd, device)
        byte_bpe = False
        if mtype == "bert":
            family = BERT
        elif mtype in ("xlm-roberta", "roberta"):
            family = XLMR
            if not os.path.isfile(os.path.join(directory, "sentencepiece.bpe.model")):
                if mtype == "roberta" or os.path.isfile(os.path.join(directory, "merges.txt")):
                    byte_bpe = True
                    why = _byte_bpe_refusal(directory)
                    if why:
                        raise ValueError(f"{directory}: model_type={mtype!r} with a byte-level BPE tokeniser (vocab.json + merges.txt) is not served as "
                                         f"a cross-encoder: {why}")
                else:
                    raise ValueError(f"{directory}: model_type={mtype!r} needs the checkpoint's sentencepiece.bpe.model, which is not there")
        elif mtype == "nomic_bert":
            raise ValueError(f"{directory}: model_type='nomic_bert' (NomicBERT) is not served as a cross-encoder")
        else:
            raise ValueError(f"{directory}: model_type={mtype!r} is not served as a cross-encoder (only 'bert', 'xlm-roberta' and 'roberta')")
        labels = cfg.get("num_labels", len(cfg["id2label"]) if isinstance(cfg.get("id2label"), dict) else 2)
        if int(labels) != 1:
            raise ValueError(f"{directory}: num_labels={labels} is not served as a cross-encoder (only one-logit heads)")
        try:
            arch = archs.bert_arch_from_hf_config(cfg)
        except KeyError as e:
            raise ValueError(f"{directory}: {e}") from e
        if isinstance(arch, archs.JinaBertArch):
            raise ValueError(f"{directory}: position_embedding_type='alibi' (JinaBERT) is not served as a cross-encoder")
        arch = dataclasses.replace(arch, type_vocab=int(cfg.get("type_vocab_size", 2 if family is BERT else 1)))
        lower, max_len = _tokenizer_settings(directory)
        if family is BERT:
            tokenizer = WordPieceTokenizer(directory, do_lower_case=lower)
        else:
            tokenizer = RobertaBpeTokenizer(directory) if byte_bpe else XlmRobertaTokenizer(directory)
        return cls(arch, sd, device, tokenizer, model_max_length=max_len, family=family)

    # ---- scoring -------------------------------------------------------------------------------------------------------------------
    def _tokenize(self, texts: Sequence[str], cap: int) -> Tuple[Tensor, np.ndarray]:
        d_ids, lens = self.device_tokenizer.encode_device(list(texts), cap)
        return d_ids.contiguous(), lens.numpy().astype(np.int64)

    def _tokenize_query(self, query: str) -> Tuple[Tensor, np.ndarray]:
        """the query's row at its full length.  A WordPiece text has at most one piece per character.  SentencePiece adds the dummy prefix
        and normalises by NFKC, which can expand a character: a row that fills 4 pieces per character is tokenised again on the host."""
        if self.family is BERT:
            return self._tokenize([query], max(len(query) + 2, 4))
        if isinstance(self.tokenizer, RobertaBpeTokenizer):     # byte-level BPE: at most one id per byte
            return self._tokenize([query], len(query.encode("utf-8", "surrogatepass")) + 2)
        cap = 4 * len(query) + 4
        d_q, qlen = self._tokenize([query], cap)
        if int(qlen[0]) >= cap:
            row = np.asarray(self.tokenizer.encode(query), dtype=np.int32)
            return self._to_device(torch.from_numpy(row[None, :])), np.asarray([row.size], dtype=np.int64)
        return d_q, qlen

    # ---- what _PairScorer.score asks of this tower ------------------------------------------------------------------------------------
    @property
    def pair_specials(self) -> int:
        return self.family.specials

    @property
    def pair_id_rows(self) -> int:
        return 2 if self.family.typed else 1

    def _pack_chunk(self, pack: tuple, d_ids: Tensor, rows: int, stream: int) -> None:
        if self.family.typed:
            L.check(self.lib.mq_pack_pairs(*pack, d_ids[1].data_ptr(), rows, stream), "mq_pack_pairs")
        else:
            L.check(self.lib.mq_pack_pairs_xlmr(*pack, rows, stream), "mq_pack_pairs_xlmr")

    def _score_chunk(self, d_ids: Tensor, d_cu: Tensor, cu: Tensor, logits: Tensor, scores: Tensor, rows: int, m: int) -> None:
        ws = self._workspace(self.lib.mq_score_pairs_workspace_bytes(C.byref(self.cfg), rows, m))
        self.score_packed(d_ids[0], d_ids[1] if self.family.typed else None, d_cu, cu, logits, scores, None, ws)

    def score_packed(self, d_ids: Tensor, d_type_ids: Optional[Tensor], d_cu: Tensor, cu: Tensor, logits: Tensor, scores: Optional[Tensor],
                     cls_rows: Optional[Tensor], ws: Tensor) -> None:
        """one mq_score_pairs_bert | mq_score_pairs_xlmr call on this thread's current stream: packed ids / type ids int32 [rows] (type ids:
        BERT only, None for XLM-R), cu_seqlens on the device and the host, logits / scores fp32 [nseq] (scores may be None), cls_rows fp32
        [nseq, W] or None"""
        if (d_type_ids is not None) != self.family.typed:
            raise ValueError(f"a {self.family.name} cross-encoder takes {'token-type ids' if self.family.typed else 'no token-type ids'}")
        if not self.family.typed:
            L.check(self.lib.mq_score_pairs_xlmr(C.byref(self.cfg), C.byref(self.w), C.byref(self.head), d_ids.data_ptr(), d_cu.data_ptr(),
                                                 cu.data_ptr(), int(cu.numel()) - 1, logits.data_ptr(), L.ptr(scores), L.ptr(cls_rows),
                                                 ws.data_ptr(), ws.numel(), self._stream()), "mq_score_pairs_xlmr")
            return
        L.check(self.lib.mq_score_pairs_bert(C.byref(self.cfg), C.byref(self.w), C.byref(self.head), d_ids.data_ptr(), d_type_ids.data_ptr(),
                                             d_cu.data_ptr(), cu.data_ptr(), int(cu.numel()) - 1, logits.data_ptr(), L.ptr(scores),
                                             L.ptr(cls_rows), ws.data_ptr(), ws.numel(), self._stream()), "mq_score_pairs_bert")


def _special_spellings(directory: str, **defaults) -> Dict[str, str]:
    """cls / sep / pad spellings of a checkpoint (special_tokens_map.json, then tokenizer_config.json), else the family's"""
    out = dict(defaults)
    for name in ("special_tokens_map.json", "tokenizer_config.json"):
        try:
            with open(os.path.join(directory, name)) as f:
                j = json.load(f)
        except (OSError, ValueError):
            continue
        for k in out:
            v = j.get(k + "_token") if isinstance(j, dict) else None
            if isinstance(v, dict):       # AddedToken serialisation
                v = v.get("content")
            if isinstance(v, str) and v:
                out[k] = v
    return out


class ModernBertCrossEncoderTower(_PairScorer, ModernBertTower):
    """`ModernBertForSequenceClassification` (num_labels = 1): `model.*` = the encoder (engine/tower_weights.py::modernbert_state_dict, as for the
    embedding tower), pooled as the config's `classifier_pooling` says, `head.dense` -> GELU -> `head.norm` -> `classifier` = the head
    (mq_score_head_ln_weights).  Pairs are [CLS] a [SEP] b [SEP]; a pair may be as long as the encoder serves (8192 tokens at most).  score() returns
    the raw logits and their sigmoid."""
    pair_specials = 3
    pair_id_rows = 2        # mq_pack_pairs also writes token-type ids: a scratch row nobody reads

    def __init__(self, arch: archs.ModernBertArch, sd: Dict[str, Tensor], device: str, tokenizer, model_max_length: int = 8192, pooling: str = "cls",
                 classifier_bias: bool = False, norm_bias: bool = False):
        W = arch.width
        dense_w, dense_b, norm_g, norm_b, cls_w, cls_b = modernbert_head_tensors(sd, W, classifier_bias, norm_bias)
        super().__init__(arch, sd, device, pooling=pooling, precision="bf16")
        h = self._h
        self.head = L.ScoreHeadLnWeights(dense_w=h.bf16(dense_w), dense_b=h.f32(dense_b) if dense_b is not None else None, norm_g=h.f32(norm_g),
                                         norm_b=h.f32(norm_b) if norm_b is not None else None, cls_w=h.f32(cls_w.reshape(W)),
                                         cls_b=float(cls_b.reshape(-1)[0]), ln_eps=float(arch.ln_eps))
        self.tokenizer = tokenizer
        self.model_max_length = int(min(model_max_length, arch.max_pos, 8192))

    @classmethod
    def from_dir(cls, directory: str, device: str) -> "ModernBertCrossEncoderTower":
        """a local Hugging Face directory: config.json, model.safetensors | pytorch_model.bin, tokenizer.json, tokenizer_config.json"""
        cfg, sd = checkpoint.load_hf_dir(directory)
        if cfg.get("model_type") != "modernbert":
            raise ValueError(f"{directory}: model_type={cfg.get('model_type')!r} is not a ModernBERT checkpoint")
        return cls._from_loaded(directory, cfg, sd, device)

    @classmethod
    def _from_loaded(cls, directory: str, cfg: dict, sd: Dict[str, Tensor], device: str) -> "ModernBertCrossEncoderTower":
        labels = cfg.get("num_labels", len(cfg["id2label"]) if isinstance(cfg.get("id2label"), dict) else 2)
        if int(labels) != 1:
            raise ValueError(f"{directory}: num_labels={labels} is not served as a cross-encoder (only one-logit heads)")
        act = cfg.get("classifier_activation", "gelu")
        if act != "gelu":
            raise ValueError(f"{directory}: classifier_activation={act!r} is not served (the head's dense layer runs the erf GELU only)")
        pooling = cfg.get("classifier_pooling", "cls")
        if pooling not in ("cls", "mean"):
            raise ValueError(f"{directory}: classifier_pooling={pooling!r} must be 'cls' or 'mean'")
        try:
            arch = archs.modernbert_arch_from_hf_config(cfg)      # 64-wide heads only, no biases in the encoder, the default rope type
        except KeyError as e:
            raise ValueError(f"{directory}: {e.args[0] if e.args else e}") from e
        if not os.path.isfile(os.path.join(directory, "tokenizer.json")):
            raise ValueError(f"{directory}: a ModernBERT cross-encoder needs the checkpoint's tokenizer.json, which is not there")
        tokenizer = HfJsonTokenizer(directory, **_special_spellings(directory, cls="[CLS]", sep="[SEP]", pad="[PAD]"))
        _, max_len = _tokenizer_settings(directory, default_max=arch.max_pos)
        return cls(arch, sd, device, tokenizer, model_max_length=max_len, pooling=pooling, classifier_bias=bool(cfg.get("classifier_bias", False)),
                   norm_bias=bool(cfg.get("norm_bias", False)))

    # ---- what _PairScorer.score asks of this tower ------------------------------------------------------------------------------------
    def _tokenize(self, texts: Sequence[str], cap: int) -> Tuple[Tensor, np.ndarray]:
        """each text ONCE, alone, through the file's own post-processor: rows [CLS] pieces [SEP] pad of exactly `cap` columns (the layout
        mq_pair_plan_n / mq_pack_pairs read: lengths count the two specials, pieces start at column 1)"""
        ids, lens = hf_rows(self.tokenizer, texts, cap)
        return self._to_device(torch.from_numpy(ids)), lens

    def _tokenize_query(self, query: str) -> Tuple[Tensor, np.ndarray]:
        return self._tokenize([query], None)

    def _pack_chunk(self, pack: tuple, d_ids: Tensor, rows: int, stream: int) -> None:
        L.check(self.lib.mq_pack_pairs(*pack, d_ids[1].data_ptr(), rows, stream), "mq_pack_pairs")

    def _score_chunk(self, d_ids: Tensor, d_cu: Tensor, cu: Tensor, logits: Tensor, scores: Tensor, rows: int, m: int) -> None:
        ws = self._workspace(self.lib.mq_score_pairs_modernbert_workspace_bytes(C.byref(self.cfg), rows, m))
        self.score_packed(d_ids[0], d_cu, cu, logits, scores, None, ws)

    def score_packed(self, d_ids: Tensor, d_cu: Tensor, cu: Tensor, logits: Tensor, scores: Optional[Tensor], pooled: Optional[Tensor],
                     ws: Tensor) -> None:
        """one mq_score_pairs_modernbert call on this thread's current stream: packed ids int32 [rows], cu_seqlens on the device and the host,
        logits / scores fp32 [nseq] (scores may be None), pooled fp32 [nseq, W] or None"""
        L.check(self.lib.mq_score_pairs_modernbert(C.byref(self.cfg), C.byref(self.w), C.byref(self.head), d_ids.data_ptr(), d_cu.data_ptr(),
                                                   cu.data_ptr(), int(cu.numel()) - 1, logits.data_ptr(), L.ptr(scores), L.ptr(pooled),
                                                   ws.data_ptr(), ws.numel(), self._stream()), "mq_score_pairs_modernbert")


class DebertaCrossEncoderTower(_PairScorer, DebertaTower):
    """`DebertaV2ForSequenceClassification` (num_labels = 1; the mxbai-rerank-*-v1 and cross-encoder/*-deberta-v3-* checkpoints): `deberta.*` = the encoder
    (engine/tower_weights.py::deberta_state_dict), `pooler.dense` -> GELU -> `classifier` on the final [CLS] row = the head (mq_score_head_gelu).  Pairs
    are [CLS] a [SEP] b [SEP]; token-type ids are not read (type_vocab_size 0).  score() returns the raw logits and their sigmoid."""
    pair_specials = 3
    pair_id_rows = 2        # mq_pack_pairs also writes token-type ids: a scratch row nobody reads

    def __init__(self, arch: archs.DebertaArch, sd: Dict[str, Tensor], device: str, tokenizer, model_max_length: int = 512, precision: str = "bf16"):
        super().__init__(arch, sd, device, pooling="cls", precision=precision, max_len=int(min(model_max_length, 8192)))
        h, t, W = self._h, self.tensors, arch.width
        self.head = L.ScoreHeadWeights(pooler_w=h.bf16(t["pooler.weight"]), pooler_b=h.f32(t["pooler.bias"]), cls_w=h.f32(t["classifier.weight"].reshape(W)),
                                       cls_b=float(t["classifier.bias"].reshape(-1)[0]), type_vocab=1)
        self.tokenizer = tokenizer
        self.model_max_length = int(self.arch.max_pos)      # min(the tokenizer's, 8192): the index table is built for it

    @classmethod
    def from_dir(cls, directory: str, device: str, precision: str = "bf16") -> "DebertaCrossEncoderTower":
        """a local Hugging Face directory: config.json, model.safetensors | pytorch_model.bin, tokenizer.json, tokenizer_config.json"""
        cfg, sd = checkpoint.load_hf_dir(directory)
        return cls._from_loaded(directory, cfg, sd, device, precision)

    @classmethod
    def _from_loaded(cls, directory: str, cfg: dict, sd: Dict[str, Tensor], device: str, precision: str = "bf16") -> "DebertaCrossEncoderTower":
        if precision != "bf16":
            raise ValueError(f"{directory}: enginePrecision={precision!r} is not served for DeBERTa cross-encoders (bf16 operands only)")
        try:
            arch = archs.deberta_arch_from_hf_config(cfg)
        except KeyError as e:
            raise ValueError(f"{directory}: config.json has no {e.args[0] if e.args else e}") from e
        except ValueError as e:
            raise ValueError(f"{directory}: {e}") from e
        labels = cfg.get("num_labels", len(cfg["id2label"]) if isinstance(cfg.get("id2label"), dict) else 2)
        if int(labels) != 1:
            raise ValueError(f"{directory}: num_labels={labels} is not served as a cross-encoder (only one-logit heads)")
        if not os.path.isfile(os.path.join(directory, "tokenizer.json")):
            only_spm = " (spm.model alone is not read: export the fast tokenizer)" if os.path.isfile(os.path.join(directory, "spm.model")) else ""
            raise ValueError(f"{directory}: a DeBERTa cross-encoder needs the checkpoint's tokenizer.json, which is not there{only_spm}")
        tokenizer = HfJsonTokenizer(directory, **_special_spellings(directory, cls="[CLS]", sep="[SEP]", pad="[PAD]"))
        _, max_len = _tokenizer_settings(directory, default_max=512)
        return cls(arch, sd, device, tokenizer, model_max_length=max_len, precision=precision)

    # ---- what _PairScorer.score asks of this tower ------------------------------------------------------------------------------------
    def _tokenize(self, texts: Sequence[str], cap: int) -> Tuple[Tensor, np.ndarray]:
        ids, lens = hf_rows(self.tokenizer, texts, cap)
        return self._to_device(torch.from_numpy(ids)), lens

    def _tokenize_query(self, query: str) -> Tuple[Tensor, np.ndarray]:
        return self._tokenize([query], None)

    def _pack_chunk(self, pack: tuple, d_ids: Tensor, rows: int, stream: int) -> None:
        L.check(self.lib.mq_pack_pairs(*pack, d_ids[1].data_ptr(), rows, stream), "mq_pack_pairs")

    def _score_chunk(self, d_ids: Tensor, d_cu: Tensor, cu: Tensor, logits: Tensor, scores: Tensor, rows: int, m: int) -> None:
        ws = self._workspace(self.lib.mq_score_pairs_deberta_workspace_bytes(C.byref(self.cfg), rows, m))
        self.score_packed(d_ids[0], d_cu, cu, logits, scores, None, ws)

    def score_packed(self, d_ids: Tensor, d_cu: Tensor, cu: Tensor, logits: Tensor, scores: Optional[Tensor], pooled: Optional[Tensor],
                     ws: Tensor) -> None:
        """one mq_score_pairs_deberta call on this thread's current stream: packed ids int32 [rows], cu_seqlens on the device and the host, logits /
        scores fp32 [nseq] (scores may be None), pooled fp32 [nseq, W] or None"""
        L.check(self.lib.mq_score_pairs_deberta(C.byref(self.cfg), C.byref(self.w), C.byref(self.head), d_ids.data_ptr(), d_cu.data_ptr(),
                                                cu.data_ptr(), int(cu.numel()) - 1, logits.data_ptr(), L.ptr(scores), L.ptr(pooled),
                                                ws.data_ptr(), ws.numel(), self._stream()), "mq_score_pairs_deberta")


class _PrefixPairScorer(_PairScorer):
    """what the decoder rerankers (QwenRerankerTower, GemmaRerankerTower) share behind their own templates: token rows [shared | segment_1 | ... |
    segment_n] -> one `pairs_entry` call (mq_score_qwen_pairs' contract) per batch of segments.  The tower supplies cfg / w / score_w, arch.max_pos and
    max_rows_per_call."""
    pairs_entry = "mq_score_qwen_pairs"

    def score_rows(self, shared: np.ndarray, segs: Sequence[np.ndarray]) -> Tuple[np.ndarray, np.ndarray]:
        """token rows -> (logits, scores): batches of segments, longest first, each behind its own copy of the shared rows (the prefix is recomputed per
        batch); a batch holds at most max_rows_per_call rows (one segment at least)"""
        n, P, dev = len(segs), int(shared.size), self.device
        lens = np.asarray([s.size for s in segs], dtype=np.int64)
        if n == 0 or int(lens.min()) < 1 or P + int(lens.max()) > self.arch.max_pos:
            raise ValueError(f"segments must hold 1 .. max_pos - prefix = {self.arch.max_pos - P} tokens")
        order = np.argsort(-lens, kind="stable")
        inv = np.empty(n, dtype=np.int64)
        inv[order] = np.arange(n)
        limit = max(int(self.max_rows_per_call) - P, int(lens.max()))
        with request_stream(dev), torch.cuda.device(dev):
            logits = torch.empty(n, dtype=torch.float32, device=dev)
            scores = torch.empty(n, dtype=torch.float32, device=dev)
            with _large_call(dev, int(lens.sum()) + P):
                a = 0
                while a < n:
                    b, rows = a + 1, int(lens[order[a]])
                    while b < n and rows + int(lens[order[b]]) <= limit:
                        rows += int(lens[order[b]])
                        b += 1
                    cu = torch.zeros(b - a + 2, dtype=torch.int32)
                    cu[1] = P
                    cu[2:] = torch.from_numpy(P + np.cumsum(lens[order[a:b]])).to(torch.int32)
                    packed = torch.from_numpy(np.concatenate([shared] + [segs[i] for i in order[a:b]]).astype(np.int32))
                    d_ids, d_cu = self._to_device(packed), self._to_device(cu)
                    ws = self._workspace(getattr(self.lib, self.pairs_entry + "_workspace_bytes")(C.byref(self.cfg), P + rows, b - a))
                    self.score_packed(d_ids, d_cu, cu, P, logits[a:b], scores[a:b], ws)
                    a = b
            out = torch.stack((logits, scores)).cpu().numpy()
        return np.ascontiguousarray(out[0][inv]), np.ascontiguousarray(out[1][inv])

    def score_packed(self, d_ids: Tensor, d_cu: Tensor, cu: Tensor, prefix_len: int, logits: Tensor, scores: Optional[Tensor], ws: Tensor) -> None:
        """one mq_score_qwen_pairs | mq_score_gemma_pairs call (`pairs_entry`) on this thread's current stream: packed ids int32 [prefix_len + segment rows], cu_seqlens int32 [nseq + 2] =
        {0, prefix_len, ...} on the device and the host, logits / scores fp32 [nseq] (scores may be None)"""
        L.check(getattr(self.lib, self.pairs_entry)(C.byref(self.cfg), C.byref(self.w), self.score_w, d_ids.data_ptr(), d_cu.data_ptr(), cu.data_ptr(),
                                             int(cu.numel()) - 2, int(prefix_len), logits.data_ptr(), L.ptr(scores), ws.data_ptr(), ws.numel(),
                                             self._stream()), self.pairs_entry)


# ---- Qwen3 rerankers: a decoder judged by one logit, the part every pair of a search shares computed once -------------------------------------------------
# The template, restated from the model card of Qwen/Qwen3-Reranker-0.6B (no real checkpoint has been run here: README.md)
QWEN_RERANK_PREFIX = ('<|im_start|>system\nJudge whether the Document meets the requirements based on the Query and the Instruct provided. '
                      'Note that the answer can only be "yes" or "no".<|im_end|>\n<|im_start|>user\n')
QWEN_RERANK_SUFFIX = "<|im_end|>\n<|im_start|>assistant\n<think>\n\n</think>\n\n"
QWEN_RERANK_INSTRUCTION = "Given a web search query, retrieve relevant passages that answer the query"


def qwen_rerank_head(instruction: str, query: str) -> str:
    """the body of the template up to and including `<Document>:` — with the prefix, the part every document of a search shares"""
    return f"<Instruct>: {instruction}\n<Query>: {query}\n<Document>:"


def qwen_split_is_safe(doc: str) -> bool:
    """the cheap test of a document's text: may ids(head + " " + doc) be formed as ids(head) + ids(" " + doc)?  The Qwen pre-tokeniser starts a new
    piece at that space whatever follows it, and BPE merges stay inside a piece; the NFC normaliser runs in front of it and is the one step that looks
    across characters.  A starter (canonical combining class 0, not a mark) behind the space leaves the space alone under NFC; a leading combining mark
    attaches to it, and that case is not argued here: the call is scored unshared."""
    return not doc or (unicodedata.combining(doc[0]) == 0 and not unicodedata.category(doc[0]).startswith("M"))


def qwen_rerank_rows(tk, prefix_ids: Sequence[int], suffix_ids: Sequence[int], head: str, docs: Sequence[str], budget: int,
                     normalizer_ok: bool = True) -> Tuple[np.ndarray, list]:
    """One query's call as token rows -> (shared int32 [P], segments: list of int32 arrays).  The reference forms every pair on its own:
    prefix + ids(head + " " + doc)[:budget] + suffix.  Shared form (P > 0): shared = prefix + ids(head), segment i = ids(" " + doc_i)[:budget -
    len(ids(head))] + suffix, the same ids in the same order.  It is taken only when the tokeniser's normaliser is none or NFC (`normalizer_ok`), every
    document passes qwen_split_is_safe, the head's ids do not change when text follows the head (probed on this call's head), and the head leaves room
    for at least one document token under the cap.  Otherwise P = 0 and every segment is a whole pair."""
    enc = lambda s: tk.encode(s, add_special_tokens=False).ids
    head_ids = enc(head)
    shared_ok = (normalizer_ok and len(head_ids) < budget and all(qwen_split_is_safe(d) for d in docs)
                 and enc(head + " a")[:len(head_ids)] == head_ids and enc(head + " a")[len(head_ids):] == enc(" a"))
    if shared_ok:
        room = budget - len(head_ids)
        rows = tk.encode_batch([" " + d for d in docs], add_special_tokens=False)
        return (np.asarray(list(prefix_ids) + head_ids, dtype=np.int32),
                [np.asarray(e.ids[:room] + list(suffix_ids), dtype=np.int32) for e in rows])
    rows = tk.encode_batch([head + " " + d for d in docs], add_special_tokens=False)
    return np.zeros(0, dtype=np.int32), [np.asarray(list(prefix_ids) + e.ids[:budget] + list(suffix_ids), dtype=np.int32) for e in rows]


def qwen_score_row(cfg: dict, sd: Dict[str, Tensor], tk, W: int, where: str) -> Tensor:
    """the one fp32 weight row [W] whose dot product with the final hidden state of a pair's last token is the logit.  Qwen3ForCausalLM (the published
    form): lm_head[yes] - lm_head[no], formed here in fp32 (lm_head.weight, else the tied embed_tokens.weight), so that sigmoid(logit) is the model
    card's softmax over (no, yes); Qwen3ForSequenceClassification with one label (the one-logit conversions): score.weight."""
    arch_names = cfg.get("architectures") or []
    if "Qwen3ForSequenceClassification" in arch_names:
        labels = cfg.get("num_labels", len(cfg["id2label"]) if isinstance(cfg.get("id2label"), dict) else 2)
        if int(labels) != 1:
            raise ValueError(f"{where}: num_labels={labels} is not served as a Qwen3 reranker (only one-logit heads)")
        return _need(sd, "score.weight", (1, W)).detach().to(torch.float32).reshape(W)
    if "Qwen3ForCausalLM" in arch_names:
        ids = {t: tk.token_to_id(t) for t in ("yes", "no")}
        gone = [t for t, i in ids.items() if i is None]
        if gone:
            raise ValueError(f"{where}: tokenizer.json has no {' / '.join(repr(t) for t in gone)} token, which the yes / no judgement reads")
        name = next((k for k in ("lm_head.weight", "model.embed_tokens.weight", "embed_tokens.weight") if k in sd), None)
        if name is None:
            raise ValueError(f"{where}: neither lm_head.weight nor embed_tokens.weight is in the checkpoint")
        head = _need(sd, name, (int(cfg["vocab_size"]), W)).detach()
        return head[ids["yes"]].to(torch.float32) - head[ids["no"]].to(torch.float32)
    raise ValueError(f"{where}: architectures={arch_names} is not served as a Qwen3 reranker (Qwen3ForCausalLM or Qwen3ForSequenceClassification)")


class QwenRerankerTower(_PrefixPairScorer, QwenTower):
    """`Qwen3ForCausalLM` read as a yes / no judge (Qwen/Qwen3-Reranker-0.6B) or `Qwen3ForSequenceClassification` with one label: the decoder of
    engine/qwen.py, the final norm on every pair's last token, one fp32 dot product (qwen_score_row).  One query against n documents is ONE
    mq_score_qwen_pairs call per batch of documents over the rows [shared | segment_1 | ... | segment_n] (qwen_rerank_rows): the system prompt, the
    instruction and the query are computed once per batch, not once per document.  score() is this class's own: a pair here is one templated string cut
    from the right, not two texts under LongestFirst, so _PairScorer's pairing and packing calls have nothing to do; its contract (logits and sigmoid in
    the order of `docs`) is kept."""

    def __init__(self, arch: archs.QwenArch, sd: Dict[str, Tensor], device: str, tokenizer, score_row: Tensor, model_max_length: int = 8192,
                 instruction: str = QWEN_RERANK_INSTRUCTION):
        if not arch.qk_norm:
            raise ValueError("Qwen2-based rerankers are not served (the Qwen3 form only)")
        QwenTower.__init__(self, arch, sd, device, pooling="last", precision="bf16")
        if tuple(score_row.shape) != (arch.width,):
            raise ValueError(f"the score row must be [{arch.width}], got {tuple(score_row.shape)}")
        self.score_w = self._h.f32(score_row)           # (a device pointer; the holder keeps the tensor)
        self.tokenizer = tokenizer
        tokenizer.no_truncation()
        tokenizer.no_padding()
        self.instruction = instruction
        self.model_max_length = int(min(model_max_length, arch.max_pos, 8192))
        self.prefix_ids = tokenizer.encode(QWEN_RERANK_PREFIX, add_special_tokens=False).ids
        self.suffix_ids = tokenizer.encode(QWEN_RERANK_SUFFIX, add_special_tokens=False).ids
        norm = json.loads(tokenizer.to_str()).get("normalizer")
        self.normalizer_ok = norm is None or norm.get("type") == "NFC"
        self._lock = threading.Lock()
        self.last_prefix_len = None      # of the latest score(): 0 = it ran unshared

    @classmethod
    def from_dir(cls, directory: str, device: str) -> "QwenRerankerTower":
        """a local Hugging Face directory: config.json, model.safetensors | pytorch_model.bin, tokenizer.json, tokenizer_config.json"""
        cfg, sd = checkpoint.load_hf_dir(directory)
        return cls._from_loaded(directory, cfg, sd, device)

    @classmethod
    def _from_loaded(cls, directory: str, cfg: dict, sd: Dict[str, Tensor], device: str) -> "QwenRerankerTower":
        mtype = cfg.get("model_type")
        if mtype == "qwen2":
            raise ValueError(f"{directory}: model_type='qwen2' is not served as a reranker (Qwen2-based rerankers such as mxbai-rerank-v2 are out of scope)")
        if mtype != "qwen3":
            raise ValueError(f"{directory}: model_type={mtype!r} is not a Qwen3 reranker")
        try:
            arch = archs.qwen_arch_from_hf_config(cfg)      # (refuses widths above 2048 — the 4B / 8B sizes —, other head widths, rope scaling ...)
        except KeyError as e:
            raise ValueError(f"{directory}: {e.args[0] if e.args else e}") from e
        if not os.path.isfile(os.path.join(directory, "tokenizer.json")):
            raise ValueError(f"{directory}: a Qwen3 reranker needs the checkpoint's tokenizer.json, which is not there")
        from tokenizers import Tokenizer
        tk = Tokenizer.from_file(os.path.join(directory, "tokenizer.json"))
        row = qwen_score_row(cfg, sd, tk, arch.width, directory)
        _, max_len = _tokenizer_settings(directory, default_max=8192)
        return cls(arch, sd, device, tk, row, model_max_length=max_len)

    # ---- scoring ----------------------------------------------------------------------------------------------------------------------------
    def rows_for(self, query: str, docs: Sequence[str], max_length: int = 512, instruction: Optional[str] = None) -> Tuple[np.ndarray, list]:
        """(shared ids, segments) of one call (qwen_rerank_rows): the host half of score(), no GPU work"""
        cap = int(min(max_length, self.model_max_length))
        budget = cap - len(self.prefix_ids) - len(self.suffix_ids)
        if budget < 1:
            raise ValueError(f"max_length={max_length} leaves no room behind the template's {len(self.prefix_ids) + len(self.suffix_ids)} tokens")
        head = qwen_rerank_head(self.instruction if instruction is None else instruction, query)
        with self._lock:
            return qwen_rerank_rows(self.tokenizer, self.prefix_ids, self.suffix_ids, head, docs, budget, self.normalizer_ok)

    def score(self, query: str, docs: Sequence[str], max_length: int = 512, instruction: Optional[str] = None) -> Tuple[np.ndarray, np.ndarray]:
        """-> (logits, sigmoid(logits)) fp32 [len(docs)] on the host, in the order of `docs`.  Texts are taken as they are (the model card strips
        nothing); the templated body is cut to min(max_length, model_max_length) - len(prefix) - len(suffix) tokens from the right."""
        if not isinstance(query, str) or not all(isinstance(d, str) for d in docs):
            raise TypeError("a cross-encoder scores (str, str) pairs")
        if len(docs) == 0:
            return np.zeros(0, np.float32), np.zeros(0, np.float32)
        shared, segs = self.rows_for(query, docs, max_length, instruction)
        self.last_prefix_len = int(shared.size)
        return self.score_rows(shared, segs)


# ---- Gemma rerankers: Gemma-2B judged by the logit of `Yes`, `[bos] A: query` computed once per batch ------------------------------------------------------
# The input format, restated from memory of FlagEmbedding's FlagLLMReranker (the package is not installed here and no real checkpoint has been run:
# README.md).  The reference tokenises the query, the passage, the separator and the prompt SEPARATELY and concatenates ids, so the shared part is the
# same token row for every hit by construction: no test of the text is needed.
GEMMA_RERANK_PROMPT = ("Given a query A and a passage B, determine whether the passage contains an answer to the query by providing a prediction of "
                       "either 'Yes' or 'No'.")


def gemma_rerank_rows(tk, bos_id: int, query: str, docs: Sequence[str], prompt: str, max_length: int, share: bool = True) -> Tuple[np.ndarray, list]:
    """One query's call as token rows -> (shared int32 [P], segments: list of int32 arrays).  Per pair the reference forms
        [bos] + ids("A: " + query)[:max_length * 3 // 4] + ids("\\n") + ids("B: " + passage)[:room] + ids("\\n") + ids(prompt)
    with room = max_length - len([bos] + query ids) - len(ids("\\n")), at least 0: the passage is cut from the right so that shared + "\\n" + passage fits
    max_length; the second separator and the prompt ride on top of the cap.  Every piece is tokenised on its own, without specials.  share: shared =
    [bos] + query ids (P >= 1 always), segment = the rest; not share: P = 0 and every segment is the whole pair (the same ids in the same order)."""
    enc = lambda s: tk.encode(s, add_special_tokens=False).ids
    q_ids = [int(bos_id)] + enc("A: " + query)[:max_length * 3 // 4]
    sep, tail = enc("\n"), enc(prompt)
    room = max(max_length - len(q_ids) - len(sep), 0)
    rows = tk.encode_batch(["B: " + d for d in docs], add_special_tokens=False)
    segs = [sep + e.ids[:room] + sep + tail for e in rows]
    if share:
        return np.asarray(q_ids, dtype=np.int32), [np.asarray(s, dtype=np.int32) for s in segs]
    return np.zeros(0, dtype=np.int32), [np.asarray(q_ids + s, dtype=np.int32) for s in segs]


def gemma_score_row(cfg: dict, sd: Dict[str, Tensor], tk, W: int, where: str) -> Tensor:
    """the one fp32 weight row [W] whose dot product with the final hidden state of a pair's last token is the logit.  GemmaForCausalLM (the published
    form): lm_head.weight[yes], else — Gemma ties them — embed_tokens.weight[yes], UNSCALED (the sqrt(width) belongs to the input side only); yes = the
    first id of "Yes" encoded without specials.  GemmaForSequenceClassification with one label: score.weight."""
    arch_names = cfg.get("architectures") or []
    if "GemmaForSequenceClassification" in arch_names:
        labels = cfg.get("num_labels", len(cfg["id2label"]) if isinstance(cfg.get("id2label"), dict) else 2)
        if int(labels) != 1:
            raise ValueError(f"{where}: num_labels={labels} is not served as a Gemma reranker (only one-logit heads)")
        return _need(sd, "score.weight", (1, W)).detach().to(torch.float32).reshape(W)
    if "GemmaForCausalLM" in arch_names:
        try:
            ids = tk.encode("Yes", add_special_tokens=False).ids
        except Exception:       # (a vocabulary without the piece and without an unknown token raises)
            ids = []
        if not ids:
            raise ValueError(f"{where}: tokenizer.json gives no token for 'Yes', which the judgement reads")
        name = next((k for k in ("lm_head.weight", "model.embed_tokens.weight", "embed_tokens.weight") if k in sd), None)
        if name is None:
            raise ValueError(f"{where}: neither lm_head.weight nor embed_tokens.weight is in the checkpoint")
        return _need(sd, name, (int(cfg["vocab_size"]), W)).detach()[int(ids[0])].to(torch.float32)
    raise ValueError(f"{where}: architectures={arch_names} is not served as a Gemma reranker (GemmaForCausalLM or GemmaForSequenceClassification)")


class GemmaRerankerTower(_PrefixPairScorer, _PackedTextTower):
    """`GemmaForCausalLM` read as a judge (BAAI/bge-reranker-v2-gemma: the score is the logit of `Yes` at the last token) or
    `GemmaForSequenceClassification` with one label: the Gemma decoder (csrc/gemma_causal.hip; 256-wide heads, causal and prefix-sharing attention of
    csrc/attention_gqa256_causal.hip), the final norm on every pair's last token, one fp32 dot product (gemma_score_row).  One query against n documents
    is ONE mq_score_gemma_pairs call per batch of documents over the rows [shared | segment_1 | ... | segment_n] (gemma_rerank_rows): `[bos] A: query` is
    computed once per batch, not once per document.  Batching, the longest-first order and max_rows_per_call are _PrefixPairScorer.score_rows'.
    `instruction` is the prompt behind the passage; score(..., instruction=...) replaces it for one call.  Not an embedder: encode_ids refuses."""
    family = "gemma_causal"
    pairs_entry = "mq_score_gemma_pairs"

    def __init__(self, arch: archs.GemmaCausalArch, sd: Dict[str, Tensor], device: str, tokenizer, score_row: Tensor, bos_id: int,
                 model_max_length: int = 8192, instruction: str = GEMMA_RERANK_PROMPT, precision: str = "bf16"):
        _PackedTextTower.__init__(self, device)
        _check_precision(precision, ("bf16",), f"the Gemma reranker runs on bf16 operands only (fp8 is out of scope), got precision {precision!r}")
        if arch.head_dim != 256:
            raise ValueError(f"the Gemma reranker runs 256-wide attention heads only (head_dim {arch.head_dim})")
        if arch.heads < 1 or arch.kv_heads < 1 or arch.heads % arch.kv_heads:
            raise ValueError(f"heads {arch.heads} must be a multiple of kv_heads {arch.kv_heads}")
        if arch.width > 2048 or arch.width % 64:
            raise ValueError(f"the Gemma reranker runs widths that are multiples of 64 up to 2048 (width {arch.width}: the 7B size is not served)")
        if tuple(score_row.shape) != (arch.width,):
            raise ValueError(f"the score row must be [{arch.width}], got {tuple(score_row.shape)}")
        if not 0 <= int(bos_id) < arch.vocab:
            raise ValueError(f"bos id {bos_id} outside the vocabulary of {arch.vocab}")
        self.precision, self.arch, self.pooling = precision, arch, "last"
        self._fp8 = None
        h, W = self._h, arch.width
        t = gemma_causal_state_dict(arch, sd)
        self._layers = (L.GemmaCausalLayer * arch.layers)()
        for l in range(arch.layers):
            p = f"layers.{l}."
            self._layers[l] = L.GemmaCausalLayer(
                input_norm_g=h.f32(t[p + "input_layernorm.weight"]), qkv_w=h.bf16(t[p + "self_attn.qkv.weight"]),
                out_w=h.bf16(t[p + "self_attn.o_proj.weight"]), post_norm_g=h.f32(t[p + "post_attention_layernorm.weight"]),
                ug_w=h.bf16(t[p + "mlp.up_gate.weight"]), down_w=h.bf16(t[p + "mlp.down_proj.weight"]))
        self.w = L.GemmaCausalWeights(tok_emb=h.f32(t["embed_tokens.weight"]), final_norm_g=h.f32(t["norm.weight"]), zeros=h.f32(torch.zeros(W)),
                                      d_inv_freq=h.f32(arch.inv_freq()), layers=self._layers)
        self.cfg = L.GemmaCausalCfg(width=W, layers=arch.layers, q_heads=arch.heads, kv_heads=arch.kv_heads, head_dim=arch.head_dim, mlp_dim=arch.mlp_dim,
                                    vocab=arch.vocab, max_pos=arch.max_pos, rms_eps=arch.rms_eps, attn_scale=arch.attn_scale)
        self.score_w = h.f32(score_row)                 # (a device pointer; the holder keeps the tensor)
        self.tokenizer = tokenizer
        tokenizer.no_truncation()
        tokenizer.no_padding()
        self.bos_id = int(bos_id)
        self.instruction = instruction
        self.model_max_length = int(min(model_max_length, arch.max_pos, 8192))
        self._lock = threading.Lock()
        self.last_prefix_len = None      # of the latest score(): 0 = it ran unshared

    def encode_ids(self, ids: Tensor, attention_mask: Tensor, normalize: bool = True) -> Tensor:
        raise ValueError("the Gemma tower is served as a reranker only (Gemma as an embedder is out of scope)")

    @classmethod
    def from_dir(cls, directory: str, device: str) -> "GemmaRerankerTower":
        """a local Hugging Face directory: config.json, model.safetensors | pytorch_model.bin, tokenizer.json, tokenizer_config.json"""
        cfg, sd = checkpoint.load_hf_dir(directory)
        return cls._from_loaded(directory, cfg, sd, device)

    @classmethod
    def _from_loaded(cls, directory: str, cfg: dict, sd: Dict[str, Tensor], device: str) -> "GemmaRerankerTower":
        try:
            arch = archs.gemma_causal_arch_from_hf_config(cfg)    # (refuses gemma2 / gemma3, the 7B, other head widths, rope scaling ... by key)
        except KeyError as e:
            raise ValueError(f"{directory}: config.json has no {e.args[0] if e.args else e}") from e
        except ValueError as e:
            raise ValueError(f"{directory}: {e}") from e
        if not os.path.isfile(os.path.join(directory, "tokenizer.json")):
            raise ValueError(f"{directory}: a Gemma reranker needs the checkpoint's tokenizer.json, which is not there (GPU tokenisation and "
                             f"tokenizer.model alone are not served for this family)")
        from tokenizers import Tokenizer
        tk = Tokenizer.from_file(os.path.join(directory, "tokenizer.json"))
        row = gemma_score_row(cfg, sd, tk, arch.width, directory)
        bos = tk.token_to_id(_special_spellings(directory, bos="<bos>")["bos"])
        if bos is None:
            bos = cfg.get("bos_token_id")
        if bos is None:
            raise ValueError(f"{directory}: neither the tokenizer's bos token nor config.json's bos_token_id names the first token of a pair")
        _, max_len = _tokenizer_settings(directory, default_max=8192)
        return cls(arch, sd, device, tk, row, int(bos), model_max_length=max_len)

    # ---- scoring ----------------------------------------------------------------------------------------------------------------------------
    def rows_for(self, query: str, docs: Sequence[str], max_length: int = 512, instruction: Optional[str] = None) -> Tuple[np.ndarray, list]:
        """(shared ids, segments) of one call (gemma_rerank_rows): the host half of score(), no GPU work.  The reference puts the second separator and
        the prompt on top of max_length; a pair that would then pass the positions the tower serves is refused (a query that alone reaches the cap keeps
        its 3/4 cut and runs SHARED like any other: the passage is then cut to nothing)."""
        cap = int(min(max_length, self.model_max_length))
        if cap < 4:
            raise ValueError(f"max_length={max_length} must be at least 4")
        with self._lock:
            shared, segs = gemma_rerank_rows(self.tokenizer, self.bos_id, query, docs, self.instruction if instruction is None else instruction, cap)
        longest = int(shared.size) + max(int(s.size) for s in segs)
        if longest > self.arch.max_pos:
            raise ValueError(f"a pair of {longest} tokens (max_length={cap} + the separator and the prompt) exceeds the {self.arch.max_pos} positions served")
        return shared, segs

    def score(self, query: str, docs: Sequence[str], max_length: int = 512, instruction: Optional[str] = None) -> Tuple[np.ndarray, np.ndarray]:
        """-> (logits, sigmoid(logits)) fp32 [len(docs)] on the host, in the order of `docs`.  Texts are taken as they are."""
        if not isinstance(query, str) or not all(isinstance(d, str) for d in docs):
            raise TypeError("a cross-encoder scores (str, str) pairs")
        if len(docs) == 0:
            return np.zeros(0, np.float32), np.zeros(0, np.float32)
        shared, segs = self.rows_for(query, docs, max_length, instruction)
        self.last_prefix_len = int(shared.size)
        return self.score_rows(shared, segs)


def load_cross_encoder_tower(directory: str, device: str):
    """the cross-encoder tower of a local Hugging Face directory, by its config.json: model_type "deberta-v2" -> DebertaCrossEncoderTower.from_dir,
    "deberta" (v1) is refused here by name, "qwen3" -> QwenRerankerTower.from_dir, "gemma" -> GemmaRerankerTower.from_dir ("gemma2", "gemma3" and
    "gemma3_text" are refused there by name), everything else -> CrossEncoderTower.from_dir (which picks among BERT, XLM-RoBERTa / RoBERTa and ModernBERT
    and refuses the rest, "qwen3" and "gemma" included when it is called directly)"""
    mtype = None
    try:
        with open(os.path.join(directory, "config.json")) as f:
            mtype = json.load(f).get("model_type")
    except (OSError, ValueError, AttributeError):
        pass                                 # (the loader below reports a missing or broken config.json in its own words)
    if mtype in ("deberta-v2", "deberta"):   # ("deberta": deberta_arch_from_hf_config refuses it, naming model_type)
        return DebertaCrossEncoderTower.from_dir(directory, device)
    if mtype == "qwen3":
        return QwenRerankerTower.from_dir(directory, device)
    if mtype in ("gemma", "gemma2", "gemma3", "gemma3_text"):   # (the later families: gemma_causal_arch_from_hf_config refuses them, naming model_type)
        return GemmaRerankerTower.from_dir(directory, device)
    return CrossEncoderTower.from_dir(directory, device)


def hf_rows(tokenizer: HfJsonTokenizer, texts: Sequence[str], cap: Optional[int]) -> Tuple[np.ndarray, np.ndarray]:
    """texts -> (ids int32 [n, cap], lengths int64 [n]): every text encoded alone by the `tokenizers` library, cut to `cap` tokens with both specials
    kept, right-padded to exactly `cap` columns (cap None: no cut, padded to the longest row)"""
    enc = tokenizer(list(texts), max_length=cap)
    got, lens = enc["input_ids"], enc["attention_mask"].sum(axis=1).astype(np.int64)
    width = int(cap) if cap else max(int(got.shape[1]), 2)
    ids = np.full((len(texts), width), tokenizer.pad_id, dtype=np.int32)
    ids[:, :got.shape[1]] = got[:, :width]
    return ids, lens

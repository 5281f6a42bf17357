"""Qwen3 rerankers on the host (no GPU): the float64 restatement of prefix attention against the grouped-query reference on the concatenated sequence, the
project's float64 pair score against transformers' own Qwen3ForCausalLM / Qwen3ForSequenceClassification, the split tokenisation of the shared part
against the `tokenizers` library on one string, the fallback rule, the loader's routing and refusals, and the new entry points' argument checks.

Bars: prefix restatement 1e-12 (both sides float64, the same sums in another order); pair score 1e-6 in float64, as the other families pin theirs.
Measured (printed as QWENRR_* lines): prefix restatement 2.2e-16; pair score TINY3 lm 1.1e-7 / cls 1.1e-7, TINY64 lm 2.1e-7 / cls 4.2e-8 (transformers
forms the rotary cos / sin in fp32 even in a float64 model, the project's reference forms them in float64: that is the whole difference)."""
import ctypes as C
import json
import os
import random

import numpy as np
import pytest
import torch

from marqo_amd import _lib as L
from marqo_amd.engine import archs
from tests import attention_ref as AR
from tests import qwen_ref as Q
from tests import qwen_rerank_ref as QR

TINY = {"TINY3": Q.TINY3, "TINY64": Q.TINY64}


# ---- prefix attention in float64 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hs", ((4, 2, 128), (7, 1, 64)))
@pytest.mark.parametrize("P", (0, 1, 63, 65))
def test_prefix_restatement_equals_the_reference_on_the_concatenated_sequence(hs, P):
    lens = [1, 17, 65]
    qkv = Q.make_gqa_qkv("randn", [P + sum(lens)], *hs, seed=P + hs[0])
    out, absout = QR.prefix_reference(qkv, P, lens, *hs)
    assert not out[:P].any() and not absout[:P].any()
    r0, worst = P, 0.0
    for ln in lens:
        cat = torch.cat([qkv[:P], qkv[r0:r0 + ln]])
        ref, refabs = Q.gqa_reference(cat, [P + ln], *hs, AR.MASK_CAUSAL)
        worst = max(worst, float((out[r0:r0 + ln] - ref[P:]).abs().max()), float((absout[r0:r0 + ln] - refabs[P:]).abs().max()))
        r0 += ln
    print(f"QWENRR_PREFIX_REF heads={hs} P={P}: max |restatement - reference| = {worst:.2e} (bar 1e-12)")
    assert worst < 1e-12


# ---- the pair score against transformers -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tuple(TINY))
@pytest.mark.parametrize("kind", ("lm", "cls"))
def test_pair_score_equals_transformers(name, kind):
    cfg = TINY[name]
    model = QR.hf_reranker(cfg, kind, seed=5)
    arch = archs.qwen_arch_from_hf_config(cfg)
    yes, no = 17, 230
    seqs = Q.random_seqs([1, 17, 70], cfg["vocab_size"], seed=4)
    ref = QR.hf_pair_logits(model, kind, seqs, yes, no)
    row = QR.score_row(model, kind, yes, no)
    got = QR.pair_logits64(model.state_dict(), arch, row, seqs)
    d = float((got - ref).abs().max())
    print(f"QWENRR_ORACLE {name} {kind}: max |project float64 - transformers float64| = {d:.2e} (bar 1e-6; logits {ref.tolist()})")
    assert d < 1e-6 and float(ref.abs().max()) > 1e-3
    if kind == "lm":   # the row folded from lm_head gives logits[yes] - logits[no]; another pair of ids does not
        other = QR.pair_logits64(model.state_dict(), arch, QR.score_row(model, kind, yes, no + 1), seqs)
        assert float((other - ref).abs().max()) > 1e-3


def test_loader_folds_the_score_row(tmp_path):
    from marqo_amd.engine import checkpoint
    from marqo_amd.engine.rerank import qwen_score_row
    tk = QR.train_tokenizer()
    yes, no = tk.token_to_id("yes"), tk.token_to_id("no")
    assert yes is not None and no is not None and yes != no
    for kind, tied in (("lm", False), ("lm", True), ("cls", False)):
        model = QR.hf_reranker(Q.TINY64, kind, seed=2)
        if tied:
            with torch.no_grad():
                model.lm_head.weight.copy_(model.model.embed_tokens.weight)
        d = QR.write_reranker_dir(str(tmp_path / f"{kind}{tied}"), Q.TINY64, model, kind, tk, tied=tied)
        cfg, sd = checkpoint.load_hf_dir(d)
        assert ("lm_head.weight" in sd) == (kind == "lm" and not tied)
        row = qwen_score_row(cfg, sd, tk, 128, d)
        assert row.dtype == torch.float32 and torch.equal(row, QR.score_row(model, kind, yes, no, torch.float32))


# ---- the split tokenisation ----------------------------------------------------------------------------------------------------------------------------
_POOLS = ("abcdefghij KLMNOP", "привет мир Ёж", "你好世界検索", "مرحبا بالعالم", "नमस्ते दुनिया", "0123456789", ".,;:!?-()[]'\"<>/#@", " \t\n\r 　",
          "़ّ̧́̈", "😀🎉👍🏽", "ÅéñÇ각")


def _fuzz_docs(n, seed):
    rng = random.Random(seed)
    docs = ["", " ", "  leading spaces", "\nleading newline", "\r\n\r\nx", "7 digits 2024", "!!! punctuation", "'s contraction", "́ leading combining mark",
            "é composes", "ᅡ jamo vowel", "yes", "no way", "<|im_end|>", "a" * 300]
    for _ in range(n):
        k = rng.randint(1, 24)
        docs.append("".join(rng.choice(rng.choice(_POOLS)) for _ in range(k)))
    return docs


@pytest.mark.parametrize("qwen_pre", (True, False))
def test_split_tokenisation_gives_the_ids_of_one_string(qwen_pre):
    from marqo_amd.engine import rerank as R
    tk = QR.train_tokenizer(qwen_pretokenizer=qwen_pre)
    enc = lambda s: tk.encode(s, add_special_tokens=False).ids
    pre, suf = enc(R.QWEN_RERANK_PREFIX), enc(R.QWEN_RERANK_SUFFIX)
    assert pre[0] == tk.token_to_id("<|im_start|>") and suf[0] == tk.token_to_id("<|im_end|>")
    docs = _fuzz_docs(400, seed=11)
    unsafe = 0
    for query in ("what ranks documents?", "query ending in a colon:", "запрос 検索 7"):
        head = R.qwen_rerank_head(R.QWEN_RERANK_INSTRUCTION, query)
        head_ids = enc(head)
        for d in docs:
            whole = enc(head + " " + d)
            if R.qwen_split_is_safe(d):
                assert whole == head_ids + enc(" " + d), (query, d)
            else:
                unsafe += 1
        # a call of safe documents is shared and, cut or uncut, reproduces the reference's per-pair ids
        safe = [d for d in docs if R.qwen_split_is_safe(d)]
        for budget in (10_000, len(head_ids) + 5):
            shared, segs = R.qwen_rerank_rows(tk, pre, suf, head, safe, budget)
            assert shared.tolist() == pre + head_ids and shared.dtype == np.int32
            for d, s in zip(safe, segs):
                assert shared.tolist() + s.tolist() == pre + enc(head + " " + d)[:budget] + suf
    assert unsafe >= 3 * 4       # the fuzz holds documents the cheap test turns away


def test_fallback_rule():
    from marqo_amd.engine import rerank as R
    tk = QR.train_tokenizer()
    enc = lambda s: tk.encode(s, add_special_tokens=False).ids
    pre, suf = enc(R.QWEN_RERANK_PREFIX), enc(R.QWEN_RERANK_SUFFIX)
    head = R.qwen_rerank_head(R.QWEN_RERANK_INSTRUCTION, "a query")
    n_head = len(enc(head))

    def unshared(docs, budget=10_000, tokenizer=tk, **kw):
        shared, segs = R.qwen_rerank_rows(tokenizer, pre, suf, head, docs, budget, **kw)
        e = lambda s: tokenizer.encode(s, add_special_tokens=False).ids
        assert [shared.tolist() + s.tolist() for s in segs] == [pre + e(head + " " + d)[:budget] + suf for d in docs]      # shared or not: the pair's ids
        return shared.size == 0

    assert not R.qwen_split_is_safe("́x") and not R.qwen_split_is_safe("़") and R.qwen_split_is_safe("") and R.qwen_split_is_safe(" x")
    assert unshared(["plain", "́ leading combining mark"])          # one unsafe document: the whole call
    assert unshared(["plain"], budget=n_head) and unshared(["plain"], budget=n_head - 3)      # the shared part alone reaches the cap
    assert not unshared(["plain"], budget=n_head + 1)
    assert unshared(["plain"], normalizer_ok=False)                      # a normaliser other than NFC (the tower sets this from tokenizer.json)
    # a tokeniser whose pieces reach across the space behind `<Document>:` (no pre-tokeniser: BPE merges run over the whole string)
    from tokenizers import Tokenizer, models, trainers
    from tests.modernbert_ref import CORPUS
    glue = Tokenizer(models.BPE(unk_token=None))
    glue.train_from_iterator([f"<Document>: {line}" for line in CORPUS] * 4, trainers.BpeTrainer(vocab_size=400, show_progress=False))   # ("<Document>: " becomes one token)
    g = lambda s: glue.encode(s, add_special_tokens=False).ids
    assert g(head + " a")[:len(g(head))] != g(head) or g(head + " a")[len(g(head)):] != g(" a")
    assert unshared(["plain", "another document"], tokenizer=glue)


# ---- loader ---------------------------------------------------------------------------------------------------------------------------------------------
def _capture(monkeypatch):
    from marqo_amd.engine import rerank as R
    seen = {}

    def init(self, arch, sd, device, tokenizer, score_row, model_max_length=8192, instruction=R.QWEN_RERANK_INSTRUCTION):
        seen.update(arch=arch, sd=sd, device=device, tokenizer=tokenizer, score_row=score_row, model_max_length=model_max_length)
        self.model_max_length = min(model_max_length, arch.max_pos, 8192)
    monkeypatch.setattr(R.QwenRerankerTower, "__init__", init)
    return seen


def test_loader_routes_qwen3_directories(tmp_path, monkeypatch):
    from marqo_amd.engine import rerank as R
    seen = _capture(monkeypatch)
    tk = QR.train_tokenizer()
    cfg = Q.config_dict(Q.TINY3, max_position_embeddings=4096)
    model = QR.hf_reranker(cfg, "lm", seed=1)
    d = QR.write_reranker_dir(str(tmp_path / "lm"), cfg, model, "lm", tk, model_max_length=2048)
    tower = R.load_cross_encoder_tower(d, "cuda:0")
    assert isinstance(tower, R.QwenRerankerTower) and tower.model_max_length == 2048
    assert torch.equal(seen["score_row"], QR.score_row(model, "lm", tk.token_to_id("yes"), tk.token_to_id("no"), torch.float32))
    assert seen["arch"] == archs.qwen_arch_from_hf_config(cfg) and "model.embed_tokens.weight" in seen["sd"]
    model = QR.hf_reranker(cfg, "cls", seed=1)
    d = QR.write_reranker_dir(str(tmp_path / "cls"), cfg, model, "cls", tk)
    assert isinstance(R.load_cross_encoder_tower(d, "cuda:0"), R.QwenRerankerTower)
    assert torch.equal(seen["score_row"].double(), model.score.weight[0].detach()) and seen["model_max_length"] == 8192
    # the BERT-family loader itself keeps refusing the family
    with pytest.raises(ValueError, match="model_type='qwen3' is not served as a cross-encoder"):
        R.CrossEncoderTower.from_dir(d, "cuda:0")


def test_loader_refusals(tmp_path, monkeypatch):
    from marqo_amd.engine import rerank as R
    from marqo_amd.s2_inference.errors import RerankerError
    from marqo_amd.s2_inference.reranking.cross_encoders import load_cross_encoder_model
    _capture(monkeypatch)
    tk = QR.train_tokenizer()
    lm, cls = QR.hf_reranker(Q.TINY64, "lm"), QR.hf_reranker(Q.TINY64, "cls")

    def refused(tag, match, kind="lm", edit=None, tokenizer=tk, drop=()):
        d = QR.write_reranker_dir(str(tmp_path / tag), Q.TINY64, lm if kind == "lm" else cls, kind, tokenizer)
        with open(os.path.join(d, "config.json")) as f:
            cfg = json.load(f)
        cfg.update(edit or {})
        with open(os.path.join(d, "config.json"), "w") as f:
            json.dump(cfg, f)
        for name in drop:
            os.remove(os.path.join(d, name))
        with pytest.raises(ValueError, match=match):
            R.load_cross_encoder_tower(d, "cuda:0")
        return d

    refused("labels", "num_labels=3 is not served as a Qwen3 reranker", kind="cls", edit={"num_labels": 3, "id2label": {"0": "a", "1": "b", "2": "c"}})
    refused("arch", r"architectures=\['Qwen3Model'\] is not served as a Qwen3 reranker", edit={"architectures": ["Qwen3Model"]})
    refused("wide", "hidden_size=2560 unsupported", edit={"hidden_size": 2560})
    refused("rope", "rope_scaling", edit={"rope_scaling": {"type": "yarn", "factor": 4.0}})
    refused("hd", "head_dim=96 unsupported", edit={"head_dim": 96})
    refused("swa", "use_sliding_window=true unsupported", edit={"use_sliding_window": True})
    refused("notok", "needs the checkpoint's tokenizer.json", drop=("tokenizer.json",))
    plain = Q.train_tokenizer(append_eos=False)           # no "yes" / "no" token
    refused("yesno", "tokenizer.json has no 'yes' / 'no' token", tokenizer=plain)
    # Qwen2: not routed to the new tower; the BERT-family loader refuses it as before
    d = QR.write_reranker_dir(str(tmp_path / "qwen2"), Q.TINY64, lm, "lm", tk)
    with open(os.path.join(d, "config.json"), "w") as f:
        json.dump(dict(Q.TINY2, architectures=["Qwen2ForCausalLM"]), f)
    with pytest.raises(ValueError, match="model_type='qwen2' is not served as a cross-encoder"):
        R.load_cross_encoder_tower(d, "cuda:0")
    with pytest.raises(ValueError, match="Qwen2-based rerankers"):
        R.QwenRerankerTower.from_dir(d, "cuda:0")
    # through the reranker's loader every one of them is a RerankerError
    d = refused("wide2", "hidden_size=2560 unsupported", edit={"hidden_size": 2560})
    with pytest.raises(RerankerError, match="hidden_size=2560 unsupported"):
        load_cross_encoder_model(d, "cuda:0")


def test_instruction_reaches_the_tower():
    from marqo_amd.s2_inference.reranking.cross_encoders import EngineCrossEncoder, ReRankerText

    class Tower:
        instruction = "default"

        def score(self, query, docs, max_length, **kw):
            self.seen = (query, list(docs), max_length, kw)
            return np.zeros(len(docs), np.float32), np.full(len(docs), 0.5, np.float32)

    model = EngineCrossEncoder.__new__(EngineCrossEncoder)
    model.tower, model.max_length = Tower(), 512
    rr = ReRankerText("x", "cuda:0", instruction="find the recipe")
    rr.model = model
    rr.rerank("q", {"hits": [{"_id": "a", "body": "text"}]})
    assert model.tower.seen == ("q", ["text"], 512, {"instruction": "find the recipe"})
    ReRankerText("x", "cuda:0").__dict__.update(model=model)
    model.predict([["q", "t"]])
    assert model.tower.seen[3] == {}
    del Tower.instruction
    with pytest.raises(ValueError, match="takes no instruction"):
        model.predict([["q", "t"]], instruction="i")


# ---- the C ABI without a GPU ---------------------------------------------------------------------------------------------------------------------------
def test_entry_points_judge_their_arguments_before_any_launch():
    text = L.HEADER_PATH.read_text()
    names = ("mq_attention_gqa_prefix", "mq_qk_norm_rope_at", "mq_score_dot", "mq_score_qwen_pairs", "mq_score_qwen_pairs_workspace_bytes")
    for name in names:
        assert name in text and name in L.EXPORTED_SYMBOLS
    assert "#define MQ_ABI_VERSION 15" in text and L.ABI_VERSION == 15
    assert [C.sizeof(s) for s in (L.QwenLayer, L.QwenWeights, L.QwenCfg)] == [72, 40, 40]
    lib = L.load()
    assert lib.mq_abi_version() == 15
    ops = L.load_torch_ops()
    assert hasattr(ops, "mq_attention_gqa_prefix") and hasattr(ops, "mq_qk_norm_rope_at")
    with pytest.raises(NotImplementedError):       # GPU only: no CPU kernel to fall back to
        ops.mq_attention_gqa_prefix(torch.zeros(4, 512, dtype=torch.bfloat16), torch.zeros(2, dtype=torch.int32), 1, 3, 4, 2, 64,
                                    torch.zeros(4, 256, dtype=torch.bfloat16))
    fake = C.c_void_p(4096)

    def refused(rc, what):
        assert rc == -1 and what in lib.mq_last_error(), lib.mq_last_error()
    att = lambda P=10, mx=20, Qh=4, KV=2, hd=64, cu=fake, qkv=fake, nseq=1: lib.mq_attention_gqa_prefix(qkv, fake, cu, nseq, P, mx, Qh, KV, hd, None)
    refused(att(qkv=None), b"mq_attention_gqa_prefix: null pointer")
    refused(att(hd=96), b"mq_attention_gqa_prefix: head_dim 96 unsupported")
    refused(att(Qh=6, KV=4), b"mq_attention_gqa_prefix: q_heads 6 must be a multiple of kv_heads 4")
    refused(att(cu=None), b"mq_attention_gqa_prefix: need cu_seqlens")
    refused(att(P=-1), b"mq_attention_gqa_prefix: prefix_len -1 unsupported")
    refused(att(mx=0), b"mq_attention_gqa_prefix: max sequence length 0 unsupported")
    refused(att(P=8000, mx=193), b"mq_attention_gqa_prefix: prefix_len 8000 + max segment length 193 exceeds 8192")
    assert att(nseq=0) == 0
    rope = lambda hd=64, off=0, qg=fake, kg=fake, cu=fake, fl=0, nseq=1: lib.mq_qk_norm_rope_at(fake, cu, nseq, fl, 4, 2, hd, qg, kg, 1e-6, fake, off, None)
    refused(rope(hd=96), b"mq_qk_norm_rope_at: head_dim 96 unsupported")
    refused(rope(kg=None), b"mq_qk_norm_rope_at: q and k norm weights come together")
    refused(rope(cu=None), b"mq_qk_norm_rope_at: need fixed_len or cu_seqlens")
    refused(rope(off=-1), b"mq_qk_norm_rope_at: offset -1 outside [0, 8192]")
    refused(rope(off=8193), b"mq_qk_norm_rope_at: offset 8193 outside [0, 8192]")
    assert rope(nseq=0) == 0
    refused(lib.mq_qk_norm_rope(fake, fake, 1, 0, 4, 2, 96, fake, fake, 1e-6, fake, None), b"mq_qk_norm_rope: head_dim 96 unsupported")    # (its own name, as before)
    refused(lib.mq_score_dot(fake, fake, 1, 4096, fake, None, None), b"mq_score_dot: W=4096")
    refused(lib.mq_score_dot(fake, None, 1, 128, fake, None, None), b"mq_score_dot: null pointer")
    assert lib.mq_score_dot(fake, fake, 0, 128, fake, None, None) == 0
    # the tower
    mk = lambda **kw: L.QwenCfg(**dict(dict(width=128, layers=1, q_heads=2, kv_heads=1, head_dim=64, mlp_dim=192, vocab=10, max_pos=64, pool=L.MQ_POOL_LAST,
                                            rms_eps=1e-6), **kw))
    layer = (L.QwenLayer * 1)(L.QwenLayer(input_norm_g=4096, qkv_w=4096, out_w=4096, post_norm_g=4096, ug_w=4096, down_w=4096))
    w = L.QwenWeights(tok_emb=4096, final_norm_g=4096, zeros=4096, d_inv_freq=4096, layers=layer)
    cu = lambda *v: (C.c_int32 * len(v))(*v)
    run = lambda cfg=None, wts=w, row=fake, h=cu(0, 10, 30), nseq=1, P=10, ws=fake, nbytes=0, logits=fake: lib.mq_score_qwen_pairs(
        C.byref(cfg or mk()), C.byref(wts), row, fake, fake, h, nseq, P, logits, None, ws, nbytes, None)
    refused(run(cfg=mk(width=4096)), b"mq_encode_qwen: width 4096 > 2048")
    refused(run(cfg=mk(head_dim=96)), b"head_dim 96 unsupported")
    refused(run(row=None), b"mq_score_qwen_pairs: null pointer")
    refused(run(wts=L.QwenWeights(tok_emb=4096, final_norm_g=4096, zeros=4096, d_inv_freq=4096, layers=(L.QwenLayer * 1)(L.QwenLayer()))),
            b"mq_score_qwen_pairs: layer 0 has null weights")
    refused(run(P=-1), b"mq_score_qwen_pairs: prefix_len -1 outside [0, max_pos=64)")
    refused(run(P=64), b"mq_score_qwen_pairs: prefix_len 64 outside")
    refused(run(h=cu(0, 9, 30)), b"mq_score_qwen_pairs: cu_seqlens must begin {0, prefix_len=10}")
    refused(run(h=cu(1, 10, 30)), b"mq_score_qwen_pairs: cu_seqlens must begin")
    refused(run(h=cu(0, 10, 10)), b"mq_score_qwen_pairs: sequence lengths must be in [1, max_pos=64]")
    refused(run(h=cu(0, 10, 70)), b"mq_score_qwen_pairs: prefix_len 10 + the longest segment 60 exceeds max_pos=64")
    refused(run(h=cu(0, 0, 0), P=0), b"mq_score_qwen_pairs: sequence lengths must be in [1, max_pos=64]")
    refused(run(ws=None), b"mq_score_qwen_pairs: null input / workspace")
    need = lib.mq_score_qwen_pairs_workspace_bytes(C.byref(mk()), 30, 1)
    assert need > lib.mq_qwen_workspace_bytes(C.byref(mk()), 30, 1) > 0 and lib.mq_score_qwen_pairs_workspace_bytes(C.byref(mk()), 0, 1) == 0
    assert run(nbytes=need - 1) == -3 and b"mq_score_qwen_pairs: workspace" in lib.mq_last_error()
    assert run(nseq=0) == 0

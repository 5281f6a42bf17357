"""Gemma rerankers on the host (no GPU): the float64 restatement of prefix attention at 256-wide heads against the grouped-query reference on the
concatenated sequence, the wrong-key inputs of the GPU test (two faulty references leave the budget, the tile-order model of the kernel stays inside it),
arch parsing and every refusal by key, the input rows against a plain-Python restatement, the score-row fold, the loader's routing, the ctypes layouts
and the C entry points' argument checks.

Bars: prefix restatement 1e-12 (both sides float64, the same sums in another order); tile-order model 1.0 x budget; a faulty reference more than
2 x 1.25 + 1 budgets from the true one (then no output lies within 1.25 of both), budget = 2**-8 (P|V| + |out|) (tests/attention_ref.py).
Measured (GEMMARR_* lines): restatement 0.0 (the same bits); model 0.79 (P = 65) / 0.83 (P = 130) x budget; the reference that admits the first future
key 256 x, the one that drops the last prefix key 4.0e4 / 3.8e4 x."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from marqo_amd import _lib as L
from marqo_amd.engine import archs
from tests import attention_ref as AR
from tests import gemma_ref as G
from tests import gemma_rerank_ref as GR
from tests import qwen_ref as Q
from tests.test_attention_gpu import MARGIN

REAL = dict(model_type="gemma", hidden_size=2048, num_attention_heads=8, num_key_value_heads=1, num_hidden_layers=18, intermediate_size=16384,
            vocab_size=256000, head_dim=256, max_position_embeddings=8192, rms_norm_eps=1e-6, hidden_activation="gelu_pytorch_tanh", rope_theta=10000.0)


# ---- attention references -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hs", ((8, 1), (3, 1)))
@pytest.mark.parametrize("P", (0, 1, 65))
def test_prefix_restatement_equals_the_reference_on_the_concatenated_sequence(hs, P):
    lens = [1, 17, 65]
    qkv = Q.make_gqa_qkv("randn", [P + sum(lens)], *hs, GR.HD, seed=P + hs[0])
    out, absout = GR.prefix_reference(qkv, P, lens, *hs)
    assert not out[:P].any() and not absout[:P].any()
    r0, worst = P, 0.0
    for ln in lens:
        cat = torch.cat([qkv[:P], qkv[r0:r0 + ln]])
        ref, refabs = Q.gqa_reference(cat, [P + ln], *hs, GR.HD, AR.MASK_CAUSAL)
        worst = max(worst, float((out[r0:r0 + ln] - ref[P:]).abs().max()), float((absout[r0:r0 + ln] - refabs[P:]).abs().max()))
        r0 += ln
    print(f"GEMMARR_PREFIX_REF heads={hs} P={P}: max |restatement - reference| = {worst:.2e} (bar 1e-12)")
    assert worst < 1e-12


@pytest.mark.parametrize("P", (65, 130))
def test_wrong_key_inputs_tell_the_references_apart(P):
    """the inputs of test_gemma_rerank_gpu.py::test_one_wrong_key_is_visible: the kernel's tile-order model within 1.0 x budget of the true reference,
    either faulty reference more than 1.25 x budget away from the TRUE one on the query it is wrong for (so a kernel inside the bar of the one is outside
    the bar of the other by more than the bar)"""
    hs, lens, seg, t = (8, 1), [20, 70, 20], 1, 37
    qkv = GR.loud_key_inputs(P, lens, *hs, seg, t, seed=P)
    out, absout = GR.prefix_reference(qkv, P, lens, *hs)
    model = GR.emulate_prefix(qkv, P, lens, *hs)
    r = AR.worst_ratio(model[P:], out[P:], absout[P:])
    row = P + sum(lens[:seg]) + t
    print(f"GEMMARR_MODEL P={P}: tile-order model / budget = {r:.4f} (bar 1.0)")
    assert r <= 1.0
    for kind in ("future", "drop_prefix"):
        bad, badabs = GR.prefix_reference(qkv, P, lens, *hs, fault=(kind, seg, t))
        far = AR.worst_ratio(out[row:row + 1, :GR.HD], bad[row:row + 1, :GR.HD], badabs[row:row + 1, :GR.HD])
        print(f"GEMMARR_MODEL P={P} {kind}: true reference / faulty reference's budget = {far:.1f} (must exceed {2 * MARGIN + 1})")
        assert far > 2 * MARGIN + 1       # |true - faulty| > (2 x 1.25 + 1) budgets: within 1.25 of the one is beyond 1.25 of the other
        other = torch.ones(out.shape[0], dtype=torch.bool)
        other[row] = False
        assert torch.equal(bad[other], out[other])


# ---- arch parsing ---------------------------------------------------------------------------------------------------------------------------------------
def test_arch_of_the_checkpoint():
    a = archs.gemma_causal_arch_from_hf_config(REAL)
    assert (a.width, a.layers, a.heads, a.kv_heads, a.head_dim, a.mlp_dim, a.vocab, a.max_pos) == (2048, 18, 8, 1, 256, 16384, 256000, 8192)
    assert a.rope_theta == 10000.0 and a.attn_scale == 1 / 16 and not a.qk_norm and not a.qkv_bias
    assert archs.gemma_causal_arch_from_hf_config(dict(REAL, rope_theta=None, rope_parameters={"rope_type": "default", "rope_theta": 5e4})).rope_theta == 5e4
    # hidden_activation wins over the legacy hidden_act when the file has both (what transformers 4.39+ wrote); hidden_act alone may say the tanh form
    assert archs.gemma_causal_arch_from_hf_config(dict(REAL, hidden_act="gelu")) == a
    assert archs.gemma_causal_arch_from_hf_config(dict(REAL, hidden_activation=None, hidden_act="gelu_pytorch_tanh")) == a
    tiny = archs.gemma_causal_arch_from_hf_config(GR.TINY81)
    assert (tiny.width, tiny.heads * tiny.head_dim) == (256, 2048)


@pytest.mark.parametrize("edit, match", (
    (dict(model_type="gemma2"), "model_type=gemma2 is not served"),
    (dict(model_type="gemma3"), "model_type=gemma3 is not served"),
    (dict(model_type="gemma3_text"), "model_type=gemma3_text is not served"),
    (dict(hidden_size=3072), "hidden_size=3072 unsupported"),
    (dict(head_dim=128), "head_dim=128 unsupported"),
    (dict(rope_scaling={"type": "linear", "factor": 2.0}), "rope_scaling="),
    (dict(rope_parameters={"rope_type": "yarn", "factor": 4.0}), "rope_parameters.rope_type=yarn"),
    (dict(attention_bias=True), "attention_bias=true"),
    (dict(hidden_activation="relu"), "hidden_activation=relu unsupported"),
    (dict(hidden_activation=None, hidden_act="gelu"), "hidden_act=gelu is ambiguous"),
    (dict(hidden_activation=None, hidden_act="silu"), "hidden_act=silu unsupported"),
    (dict(max_position_embeddings=16384), "max_position_embeddings=16384"),
    (dict(attn_logit_softcapping=50.0), "attn_logit_softcapping=50.0"),
    (dict(num_key_value_heads=3), "num_attention_heads=8 must be a multiple of num_key_value_heads=3"),
))
def test_arch_refusals_name_the_key(edit, match):
    with pytest.raises(ValueError, match=match):
        archs.gemma_causal_arch_from_hf_config(dict(REAL, **edit))


def test_the_installed_transformers_reads_hidden_act_alone():
    """why hidden_act='gelu' without hidden_activation is refused and not mapped: the installed transformers runs the erf form for it"""
    import transformers
    from transformers.activations import GELUActivation
    kw = {k: v for k, v in GR.TINY21.items() if k not in ("model_type", "hidden_activation")}
    mlp = transformers.GemmaForCausalLM(transformers.GemmaConfig(**dict(kw, hidden_act="gelu"))).model.layers[0].mlp
    assert isinstance(mlp.act_fn, GELUActivation)
    x = torch.linspace(-4, 4, 33, dtype=torch.float64)
    tanh = transformers.GemmaForCausalLM(transformers.GemmaConfig(**kw)).model.layers[0].mlp.act_fn
    assert float((tanh(x) - G.gelu_tanh(x)).abs().max()) < 1e-12 and float((mlp.act_fn(x) - G.gelu_tanh(x)).abs().max()) > 1e-4


# ---- input rows -------------------------------------------------------------------------------------------------------------------------------------------
def test_rows_against_the_plain_restatement():
    from marqo_amd.engine import rerank as R
    assert R.GEMMA_RERANK_PROMPT == GR.PROMPT
    tk = G.train_tokenizer()
    bos = tk.token_to_id(G.BOS)
    enc = lambda s: list(tk.encode(s, add_special_tokens=False).ids)
    docs = ["a short passage", "", "the cat sat on the mat " * 30, "B: looks like a field", "\nnewline first", "Yes"]
    query = "what ranks documents?"
    for prompt in (GR.PROMPT, "answer Yes or No"):
        for cap in (512, 64, 40, 12):
            q, whole = GR.plain_rows(tk, bos, query, docs, prompt, cap)
            shared, segs = R.gemma_rerank_rows(tk, bos, query, docs, prompt, cap)
            assert shared.dtype == np.int32 and shared.tolist() == q and shared[0] == bos          # the same shared ids for every document
            assert [shared.tolist() + s.tolist() for s in segs] == whole
            none, un = R.gemma_rerank_rows(tk, bos, query, docs, prompt, cap, share=False)
            assert none.size == 0 and [s.tolist() for s in un] == whole                        # shared + segment = the unshared builder's row
            sep, tail = enc("\n"), enc(prompt)
            for d, s in zip(docs, segs):
                body = s.tolist()[len(sep):len(s) - len(sep) - len(tail)]
                assert s.tolist()[:len(sep)] == sep and s.tolist()[len(s) - len(tail):] == tail
                assert body == enc("B: " + d)[:max(cap - len(q) - len(sep), 0)]                # cut from the right, to what the cap leaves
                assert len(q) + len(sep) + len(body) <= max(cap, len(q) + len(sep))
    # an empty passage keeps "B: " and both separators
    _, segs = R.gemma_rerank_rows(tk, bos, query, [""], GR.PROMPT, 512)
    assert segs[0].tolist() == enc("\n") + enc("B: ") + enc("\n") + enc(GR.PROMPT)
    # the query is cut at 3/4 of the cap; one that alone reaches the cap runs SHARED, its passage cut to nothing
    long_q = "why " * 200
    for cap in (40, 41):
        shared, segs = R.gemma_rerank_rows(tk, bos, long_q, ["doc one", "doc two"], GR.PROMPT, cap)
        assert shared.size == 1 + cap * 3 // 4 and shared.tolist()[1:] == enc("A: " + long_q)[:cap * 3 // 4]
    shared, segs = R.gemma_rerank_rows(tk, bos, long_q, ["doc one", "doc two"], GR.PROMPT, 4)
    assert shared.size == 4 and all(s.tolist() == enc("\n") + enc("\n") + enc(GR.PROMPT) for s in segs)


# ---- loader ---------------------------------------------------------------------------------------------------------------------------------------------
def test_loader_folds_the_score_row(tmp_path):
    from marqo_amd.engine import checkpoint
    from marqo_amd.engine.rerank import gemma_score_row
    tk = G.train_tokenizer()
    yes = tk.encode("Yes", add_special_tokens=False).ids[0]
    for kind, tied in (("lm", False), ("lm", True), ("cls", False)):
        model = GR.hf_reranker(GR.TINY21, kind, seed=2)
        if tied:
            with torch.no_grad():
                model.lm_head.weight.copy_(model.model.embed_tokens.weight)
        d = GR.write_reranker_dir(str(tmp_path / f"{kind}{tied}"), GR.TINY21, model, kind, tk, tied=tied)
        cfg, sd = checkpoint.load_hf_dir(d)
        assert ("lm_head.weight" in sd) == (kind == "lm" and not tied)
        row = gemma_score_row(cfg, sd, tk, 256, d)
        assert row.dtype == torch.float32 and torch.equal(row, GR.score_row(model, kind, yes, torch.float32))      # (tied: the UNSCALED table's row)


def test_state_dict_folds_norms_and_the_token_scale():
    from marqo_amd.engine.tower_weights import gemma_causal_state_dict
    model = GR.hf_reranker(GR.TINY21, "lm", seed=4).float()
    arch = archs.gemma_causal_arch_from_hf_config(GR.TINY21)
    sd = model.state_dict()
    t = gemma_causal_state_dict(arch, sd)
    assert torch.equal(t["norm.weight"], 1.0 + sd["model.norm.weight"])
    assert torch.equal(t["layers.1.post_attention_layernorm.weight"], 1.0 + sd["model.layers.1.post_attention_layernorm.weight"])
    assert torch.equal(t["embed_tokens.weight"], sd["model.embed_tokens.weight"] * torch.tensor(16.0))
    assert t["layers.0.self_attn.qkv.weight"].shape == ((2 + 2) * 256, 256) and t["layers.0.mlp.up_gate.weight"].shape == (1024, 256)
    assert torch.equal(t["layers.0.mlp.up_gate.weight"][:512], sd["model.layers.0.mlp.up_proj.weight"])
    with pytest.raises(ValueError, match="bias-free"):
        gemma_causal_state_dict(arch, dict(sd, **{"model.layers.0.self_attn.q_proj.bias": torch.zeros(512)}))


def _capture(monkeypatch):
    from marqo_amd.engine import rerank as R
    seen = {}

    def init(self, arch, sd, device, tokenizer, score_row, bos_id, model_max_length=8192, instruction=R.GEMMA_RERANK_PROMPT, precision="bf16"):
        seen.update(arch=arch, sd=sd, device=device, tokenizer=tokenizer, score_row=score_row, bos_id=bos_id, model_max_length=model_max_length)
        self.model_max_length = min(model_max_length, arch.max_pos, 8192)
    monkeypatch.setattr(R.GemmaRerankerTower, "__init__", init)
    return seen


def test_loader_routes_gemma_directories(tmp_path, monkeypatch):
    from marqo_amd.engine import rerank as R
    seen = _capture(monkeypatch)
    tk = G.train_tokenizer()
    yes = tk.encode("Yes", add_special_tokens=False).ids[0]
    cfg = Q.config_dict(GR.TINY81, max_position_embeddings=4096)
    model = GR.hf_reranker(cfg, "lm", seed=1)
    d = GR.write_reranker_dir(str(tmp_path / "lm"), cfg, model, "lm", tk, model_max_length=2048)
    tower = R.load_cross_encoder_tower(d, "cuda:0")
    assert isinstance(tower, R.GemmaRerankerTower) and tower.model_max_length == 2048 and seen["bos_id"] == tk.token_to_id(G.BOS) == 2
    assert torch.equal(seen["score_row"], GR.score_row(model, "lm", yes, torch.float32))
    assert seen["arch"] == archs.gemma_causal_arch_from_hf_config(cfg) and "model.embed_tokens.weight" in seen["sd"]
    model = GR.hf_reranker(cfg, "cls", seed=1)
    d = GR.write_reranker_dir(str(tmp_path / "cls"), cfg, model, "cls", tk)
    assert isinstance(R.load_cross_encoder_tower(d, "cuda:0"), R.GemmaRerankerTower)
    assert torch.equal(seen["score_row"].double(), model.score.weight[0].detach()) and seen["model_max_length"] == 8192
    # the BERT-family loader itself keeps refusing the family
    with pytest.raises(ValueError, match="model_type='gemma' is not served as a cross-encoder"):
        R.CrossEncoderTower.from_dir(d, "cuda:0")


def test_loader_refusals(tmp_path, monkeypatch):
    from marqo_amd.engine import rerank as R
    from marqo_amd.s2_inference.errors import RerankerError
    from marqo_amd.s2_inference.reranking.cross_encoders import load_cross_encoder_model
    _capture(monkeypatch)
    tk = G.train_tokenizer()
    lm, cls = GR.hf_reranker(GR.TINY21, "lm"), GR.hf_reranker(GR.TINY21, "cls")

    def refused(tag, match, kind="lm", edit=None, tokenizer=tk, drop=()):
        d = GR.write_reranker_dir(str(tmp_path / tag), GR.TINY21, lm if kind == "lm" else cls, kind, tokenizer)
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

    refused("gemma2", "model_type=gemma2 is not served as a reranker", edit={"model_type": "gemma2"})
    refused("wide", "hidden_size=3072 unsupported", edit={"hidden_size": 3072})
    refused("hd", "head_dim=128 unsupported", edit={"head_dim": 128})
    refused("rope", "rope_scaling", edit={"rope_scaling": {"type": "linear", "factor": 2.0}})
    refused("labels", "num_labels=2 is not served as a Gemma reranker", kind="cls", edit={"num_labels": 2, "id2label": {"0": "a", "1": "b"}})
    refused("arch", r"architectures=\['GemmaModel'\] is not served as a Gemma reranker", edit={"architectures": ["GemmaModel"]})
    refused("notok", "needs the checkpoint's tokenizer.json", drop=("tokenizer.json",))
    # a tokeniser that has no piece for "Yes": a word-level vocabulary without an unknown token
    from tokenizers import Tokenizer, models
    refused("noyes", "gives no token for 'Yes'", tokenizer=Tokenizer(models.WordLevel({"<bos>": 0, "a": 1}, unk_token=None)))
    # through the reranker's loader every one of them is a RerankerError
    d = refused("wide2", "hidden_size=3072 unsupported", edit={"hidden_size": 3072})
    with pytest.raises(RerankerError, match="hidden_size=3072 unsupported"):
        load_cross_encoder_model(d, "cuda:0")


# ---- the C ABI without a GPU ---------------------------------------------------------------------------------------------------------------------------
def test_entry_points_judge_their_arguments_before_any_launch():
    text = L.HEADER_PATH.read_text()
    names = ("mq_attention_gqa256_causal", "mq_attention_gqa256_prefix", "mq_score_gemma_pairs", "mq_score_gemma_pairs_workspace_bytes")
    for name in names:
        assert name in text and name in L.EXPORTED_SYMBOLS
    assert "#define MQ_ABI_VERSION 15" in text and L.ABI_VERSION == 15
    assert [C.sizeof(s) for s in (L.GemmaCausalLayer, L.GemmaCausalWeights, L.GemmaCausalCfg)] == [48, 40, 40]      # the static_assert of csrc/gemma_causal.hip
    lib = L.load()
    assert lib.mq_abi_version() == 15
    ops = L.load_torch_ops()
    assert hasattr(ops, "mq_attention_gqa256_prefix")
    with pytest.raises(NotImplementedError):       # GPU only: no CPU kernel to fall back to
        ops.mq_attention_gqa256_prefix(torch.zeros(4, 1024, dtype=torch.bfloat16), torch.zeros(2, dtype=torch.int32), 1, 3, 2, 1, 256, 1 / 16,
                                       torch.zeros(4, 512, dtype=torch.bfloat16))
    fake = C.c_void_p(4096)

    def refused(rc, what):
        assert rc == -1 and what in lib.mq_last_error(), lib.mq_last_error()
    pre = lambda P=10, mx=20, Qh=8, KV=1, hd=256, cu=fake, qkv=fake, nseq=1, sc=1 / 16: lib.mq_attention_gqa256_prefix(qkv, fake, cu, nseq, P, mx, Qh, KV, hd, sc, None)
    refused(pre(qkv=None), b"mq_attention_gqa256_prefix: null pointer")
    refused(pre(hd=128), b"mq_attention_gqa256_prefix: head_dim 128 unsupported")
    refused(pre(Qh=6, KV=4), b"mq_attention_gqa256_prefix: q_heads 6 must be a multiple of kv_heads 4")
    refused(pre(sc=0.0), b"mq_attention_gqa256_prefix: softmax scale")
    refused(pre(cu=None), b"mq_attention_gqa256_prefix: need cu_seqlens")
    refused(pre(P=-1), b"mq_attention_gqa256_prefix: prefix_len -1 unsupported")
    refused(pre(mx=0), b"mq_attention_gqa256_prefix: max sequence length 0 unsupported")
    refused(pre(P=8000, mx=193), b"mq_attention_gqa256_prefix: prefix_len 8000 + max segment length 193 exceeds 8192")
    assert pre(nseq=0) == 0
    cau = lambda fl=0, mx=20, Qh=8, KV=1, hd=256, cu=fake, out=fake, nseq=1, sc=1 / 16: lib.mq_attention_gqa256_causal(fake, out, cu, nseq, fl, mx, Qh, KV, hd, sc, None)
    refused(cau(out=None), b"mq_attention_gqa256_causal: null pointer")
    refused(cau(hd=128), b"mq_attention_gqa256_causal: head_dim 128 unsupported")
    refused(cau(Qh=3, KV=2), b"mq_attention_gqa256_causal: q_heads 3 must be a multiple of kv_heads 2")
    refused(cau(sc=-1.0), b"mq_attention_gqa256_causal: softmax scale")
    refused(cau(cu=None), b"mq_attention_gqa256_causal: need fixed_len or cu_seqlens")
    refused(cau(mx=8193), b"mq_attention_gqa256_causal: max sequence length 8193 unsupported")
    assert cau(nseq=0) == 0
    # the tower
    mk = lambda **kw: L.GemmaCausalCfg(**dict(dict(width=128, layers=1, q_heads=2, kv_heads=1, head_dim=256, mlp_dim=192, vocab=10, max_pos=64, rms_eps=1e-6,
                                                   attn_scale=1 / 16), **kw))
    layer = (L.GemmaCausalLayer * 1)(L.GemmaCausalLayer(input_norm_g=4096, qkv_w=4096, out_w=4096, post_norm_g=4096, ug_w=4096, down_w=4096))
    w = L.GemmaCausalWeights(tok_emb=4096, final_norm_g=4096, zeros=4096, d_inv_freq=4096, layers=layer)
    cu = lambda *v: (C.c_int32 * len(v))(*v)
    run = lambda cfg=None, wts=w, row=fake, h=cu(0, 10, 30), nseq=1, P=10, ws=fake, nbytes=0, logits=fake: lib.mq_score_gemma_pairs(
        C.byref(cfg or mk()), C.byref(wts), row, fake, fake, h, nseq, P, logits, None, ws, nbytes, None)
    refused(run(cfg=mk(width=4096)), b"mq_score_gemma_pairs: width 4096 > 2048")
    refused(run(cfg=mk(head_dim=128)), b"mq_score_gemma_pairs: head_dim 128 unsupported (256)")
    refused(run(cfg=mk(max_pos=8193)), b"mq_score_gemma_pairs: max_pos 8193 outside [1, 8192]")
    refused(run(cfg=mk(attn_scale=0.0)), b"mq_score_gemma_pairs: attn_scale")
    refused(run(row=None), b"mq_score_gemma_pairs: null pointer")
    refused(run(wts=L.GemmaCausalWeights(tok_emb=4096, final_norm_g=4096, zeros=4096, d_inv_freq=4096, layers=(L.GemmaCausalLayer * 1)(L.GemmaCausalLayer()))),
            b"mq_score_gemma_pairs: layer 0 has null weights")
    refused(run(P=-1), b"mq_score_gemma_pairs: prefix_len -1 outside [0, max_pos=64)")
    refused(run(P=64), b"mq_score_gemma_pairs: prefix_len 64 outside")
    refused(run(h=cu(0, 9, 30)), b"mq_score_gemma_pairs: cu_seqlens must begin {0, prefix_len=10}")
    refused(run(h=cu(0, 10, 10)), b"mq_score_gemma_pairs: sequence lengths must be in [1, max_pos=64]")
    refused(run(h=cu(0, 10, 70)), b"mq_score_gemma_pairs: prefix_len 10 + the longest segment 60 exceeds max_pos=64")
    refused(run(h=cu(0, 0, 0), P=0), b"mq_score_gemma_pairs: sequence lengths must be in [1, max_pos=64]")
    refused(run(ws=None), b"mq_score_gemma_pairs: null input / workspace")
    need = lib.mq_score_gemma_pairs_workspace_bytes(C.byref(mk()), 30, 1)
    assert need > 0 and lib.mq_score_gemma_pairs_workspace_bytes(C.byref(mk()), 0, 1) == 0
    assert run(nbytes=need - 1) == -3 and b"mq_score_gemma_pairs: workspace" in lib.mq_last_error()
    assert run(nseq=0) == 0

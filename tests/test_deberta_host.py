"""DeBERTa on the host: the index table against transformers' own function, the float64 restatement of the tower (tests/deberta_ref.py::exact) against
transformers' DebertaV2ForSequenceClassification in float64, the folding of the position tables, the parser's refusals, the dispatch of
EngineCrossEncoder, and the mutants of the float64 bf16 model against the stream bar of the GPU test.

Bars:
  `exact` logits against float64 transformers: 1e-6 of max(1, |logit|) on every tiny and both batches.  The one known cause of a difference is that
  transformers forms sqrt(3 head_dim) in fp32 (6.5e-9 measured when the restatement was first written down); the loader's position tables are stored
  in fp32 (6e-8 relative).  Measured here: worst 9.3e-9 of max(1, |logit|) (DEBERTA_EXACT lines).
  Mutants: each must leave MARGIN = 4.0 (the stream bar of tests/test_deberta_gpu.py: max |mutant - exact| / |model - exact| per row) on at least one
  tiny, in the final stream or in the logits.  A mutant that stayed inside the bar on every tiny would be listed in NOT_DETECTABLE with an assertion that
  keeps it so; none is (DEBERTA_MUTANT lines: the smallest worst-view ratio of any mutant on any tiny is rel_not_normed's 51).
"""
import json
import os

import pytest
import torch

from marqo_amd.engine import archs
from tests import deberta_ref as D

MARGIN = 4.0
NOT_DETECTABLE = ()


# ---- the index table ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S, max_rel, T", ((4, 16, 300), (8, 64, 300), (256, 512, 1100)))
def test_idx_table_is_transformers_bucket_clamped(S, max_rel, T):
    arch = archs.DebertaArch(span=S, max_rel=max_rel)
    reach = T - 1
    t = arch.idx_table(reach)
    assert t.dtype == torch.int32 and tuple(t.shape) == (2 * reach + 1,)
    assert torch.equal(D.pair_index(t, T, reach), D.transformers_idx(T, S, max_rel))
    assert bool((t[1:] >= t[:-1]).all()), "the table must be non-decreasing in query - key"
    assert int(t[0]) == 0 and int(t[-1]) == 2 * S - 1, "both clamp ends are reached"
    assert int((t == 0).sum()) > 1 and int((t == 2 * S - 1).sum()) > 1, "the clamp is active at both ends"
    assert int(t[reach]) == S
    # a shorter table is the middle of a longer one: the kernel indexes it from its centre
    assert torch.equal(arch.idx_table(40), t[reach - 40:reach + 41])


# ---- exact against transformers ---------------------------------------------------------------------------------------------------------------------------
def _hf64_logits(b, seqs):
    import copy
    m = copy.deepcopy(b["hf"]).double().eval()
    with torch.no_grad():
        return torch.stack([m(input_ids=s[None], attention_mask=torch.ones_like(s[None])).logits[0, 0] for s in seqs])


@pytest.mark.parametrize("name", tuple(D.TINIES))
def test_exact_is_transformers_in_float64(name):
    b = D.build(name)
    for bi, seqs in enumerate(b["batches"]):
        lens = [len(s) for s in seqs]
        ref = _hf64_logits(b, seqs)
        ex = D.exact(b["arch"], b["tensors"], torch.cat(seqs), lens)
        err = float(((ex.logits - ref).abs() / ref.abs().clamp(min=1.0)).max())
        print(f"DEBERTA_EXACT {name} batch={bi}: worst |exact - transformers| / max(1, |logit|) = {err:.2e}; logits {[round(float(v), 3) for v in ref]}")
        assert err <= 1e-6
        assert float(ref.abs().max()) > 0.5, "the tiny's logits must be of working size"


@pytest.mark.parametrize("name", ("S8_SHARE", "S8_SPLIT"))
def test_position_tables_are_the_projections_of_the_normalised_rel_embeddings(name):
    b = D.build(name)
    arch, att0 = b["arch"], b["hf"].deberta.encoder.layer[0].attention.self
    enc = b["hf"].deberta.encoder
    with torch.no_grad():
        rel = enc.get_rel_embedding().double()
        assert tuple(rel.shape) == (2 * arch.span, arch.width)
        kproj, qproj = (att0.key_proj, att0.query_proj) if arch.share_att_key else (att0.pos_key_proj, att0.pos_query_proj)
        for got, proj in ((b["tensors"]["layer.0.pos_key"], kproj), (b["tensors"]["layer.0.pos_query"], qproj)):
            ref = torch.nn.functional.linear(rel, proj.weight.double(), proj.bias.double()).reshape(2 * arch.span, arch.heads, 64).transpose(0, 1)
            assert tuple(got.shape) == (arch.heads, 2 * arch.span, 64) and got.dtype == torch.float32
            assert float((got.double() - ref).abs().max()) <= 1e-6 * float(ref.abs().max())
    if not arch.share_att_key:      # and the two settings read different matrices
        other = torch.nn.functional.linear(rel, att0.key_proj.weight.double(), att0.key_proj.bias.double()).reshape(2 * arch.span, arch.heads, 64).transpose(0, 1)
        assert float((b["tensors"]["layer.0.pos_key"].double() - other).abs().max()) > 0.1
    fused = b["tensors"]["layer.0.attn.qkv.weight"]
    assert torch.equal(fused, torch.cat([att0.query_proj.weight, att0.key_proj.weight, att0.value_proj.weight]).detach())


# ---- the parser ---------------------------------------------------------------------------------------------------------------------------------------------
_REFUSALS = (
    (dict(model_type="deberta"), "model_type"), (dict(relative_attention=False), "relative_attention"), (dict(pos_att_type=["c2p"]), "pos_att_type"),
    (dict(pos_att_type=["c2p", "p2c", "p2p"]), "pos_att_type"), (dict(position_biased_input=True), "position_biased_input"),
    (dict(conv_kernel_size=3), "conv_kernel_size"), (dict(norm_rel_ebd="none"), "norm_rel_ebd"), (dict(type_vocab_size=2), "type_vocab_size"),
    (dict(embedding_size=64), "embedding_size"), (dict(pooler_hidden_size=64), "pooler_hidden_size"), (dict(pooler_hidden_act="tanh"), "pooler_hidden_act"),
    (dict(hidden_act="relu"), "hidden_act"), (dict(num_attention_heads=4), "num_attention_heads"), (dict(hidden_size=2112, num_attention_heads=33), "hidden_size"),
    (dict(position_buckets=2048), "position_buckets"), (dict(position_buckets=0), "position_buckets"), (dict(position_buckets=-1), "position_buckets"),
)


@pytest.mark.parametrize("over, key", _REFUSALS, ids=[f"{k}-{i}" for i, (_, k) in enumerate(_REFUSALS)])
def test_parser_refuses_by_the_name_of_the_key(over, key):
    with pytest.raises(ValueError, match=key):
        archs.deberta_arch_from_hf_config(dict(D.TINIES["S8_SHARE"], **over))


def test_parser_reads_the_served_shape():
    a = archs.deberta_arch_from_hf_config(dict(D.TINIES["S8_SPLIT"], pos_att_type="p2c|c2p"))
    assert (a.width, a.heads, a.span, a.max_rel, a.share_att_key, a.ln_eps) == (128, 2, 8, 64, False, 1e-7)
    assert archs.deberta_arch_from_hf_config(dict(D.TINIES["S8_SHARE"], max_relative_positions=40)).max_rel == 40
    with pytest.raises(KeyError):       # the BERT-family parser keeps refusing the family
        archs.bert_arch_from_hf_config(D.TINIES["S8_SHARE"])


@pytest.fixture(scope="module")
def ckpt(tmp_path_factory):
    d = tmp_path_factory.mktemp("deberta_host") / "reranker"
    D.write_dir(d, "S8_SHARE", seed=4)
    return str(d)


def _variant(ckpt, tmp_path, **over):
    import shutil
    d = tmp_path / "variant"
    shutil.copytree(ckpt, d)
    with open(d / "config.json") as f:
        cfg = json.load(f)
    cfg.update(over)
    with open(d / "config.json", "w") as f:
        json.dump(cfg, f)
    return str(d)


def test_loader_refusals(ckpt, tmp_path):
    from marqo_amd.engine.rerank import CrossEncoderTower, DebertaCrossEncoderTower, load_cross_encoder_tower
    three = _variant(ckpt, tmp_path, num_labels=3, id2label={"0": "a", "1": "b", "2": "c"})
    with pytest.raises(ValueError, match="num_labels=3"):
        DebertaCrossEncoderTower.from_dir(three, "cpu")
    with pytest.raises(ValueError, match="enginePrecision"):
        DebertaCrossEncoderTower.from_dir(ckpt, "cpu", precision="fp8")
    with pytest.raises(ValueError, match="model_type"):
        load_cross_encoder_tower(_variant(ckpt, tmp_path / "v1", model_type="deberta"), "cpu")
    nojson = _variant(ckpt, tmp_path / "spm")
    os.remove(os.path.join(nojson, "tokenizer.json"))
    open(os.path.join(nojson, "spm.model"), "wb").close()
    with pytest.raises(ValueError, match="tokenizer.json"):
        DebertaCrossEncoderTower.from_dir(nojson, "cpu")
    with pytest.raises(ValueError, match="not served as a cross-encoder"):      # the BERT-tower loader still refuses the directory
        CrossEncoderTower.from_dir(ckpt, "cpu")


def test_engine_cross_encoder_dispatches_by_model_type(ckpt, monkeypatch):
    from marqo_amd.engine import rerank as ER
    from marqo_amd.s2_inference.errors import RerankerError
    from marqo_amd.s2_inference.reranking import cross_encoders as CE
    seen = []

    class _Stub:
        model_max_length = 77

    monkeypatch.setattr(ER.DebertaCrossEncoderTower, "from_dir", classmethod(lambda cls, d, dev, *a, **k: seen.append(("deberta", d, dev)) or _Stub()))
    monkeypatch.setattr(ER.CrossEncoderTower, "from_dir", classmethod(lambda cls, d, dev, *a, **k: seen.append(("bert", d, dev)) or _Stub()))
    m = CE.EngineCrossEncoder(ckpt, "cuda:0", max_length=512)
    assert seen == [("deberta", ckpt, "cuda:0")] and m.max_length == 77
    other = os.path.join(os.path.dirname(ckpt), "other")
    os.makedirs(other, exist_ok=True)
    with open(os.path.join(other, "config.json"), "w") as f:
        json.dump({"model_type": "bert"}, f)
    CE.EngineCrossEncoder(other, "cuda:0")
    assert seen[-1] == ("bert", other, "cuda:0")
    monkeypatch.undo()
    # a refusal of the parser surfaces as a RerankerError that names the key
    bad = os.path.join(os.path.dirname(ckpt), "bad")
    os.makedirs(bad, exist_ok=True)
    with open(os.path.join(ckpt, "config.json")) as f:
        cfg = json.load(f)
    import shutil
    for fn in os.listdir(ckpt):
        shutil.copy(os.path.join(ckpt, fn), os.path.join(bad, fn))
    with open(os.path.join(bad, "config.json"), "w") as f:
        json.dump(dict(cfg, conv_kernel_size=3), f)
    with pytest.raises(RerankerError, match="conv_kernel_size"):
        CE.load_cross_encoder_model(bad, "cpu")


# ---- the mutants of the model -------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def passes():
    out = {}
    for name in D.TINIES:
        b = D.build(name)
        seqs = b["batches"][0]
        lens, ids = [len(s) for s in seqs], torch.cat(seqs)
        out[name] = (b, ids, lens, D.exact(b["arch"], b["tensors"], ids, lens), D.model(b["arch"], b["tensors"], ids, lens))
    return out


def test_the_model_is_near_exact_and_not_equal(passes):
    for name, (b, ids, lens, ex, mo) in passes.items():
        rel = float((mo.final - ex.final).norm() / ex.final.norm())
        assert 1e-4 < rel < 3e-2, (name, rel)


@pytest.mark.parametrize("mut", D.MUTANTS)
def test_every_mutant_leaves_the_stream_bar_on_some_tiny(passes, mut):
    worst = {}
    for name, (b, ids, lens, ex, mo) in passes.items():
        mm = D.model(b["arch"], b["tensors"], ids, lens, mut=mut, sd=b["sd"])
        worst[name] = max(D.row_ratio(mm.final, ex.final, mo.final)["ratio"], D.scalar_ratio(mm.logits, ex.logits, mo.logits))
    print(f"DEBERTA_MUTANT {mut}: " + " ".join(f"{k}={v:.1f}" for k, v in worst.items()))
    if mut in NOT_DETECTABLE:
        assert max(worst.values()) <= MARGIN, f"{mut} has become detectable: take it off NOT_DETECTABLE"
    else:
        assert max(worst.values()) > MARGIN, (mut, worst)

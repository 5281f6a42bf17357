"""Jina v3 without a GPU: the float64 restatement of csrc/jina_v3.hip (tests/jina_v3_ref.py::exact) against transformers' JinaEmbeddingsV3Model in
float64 — the base block, and the LoRA delta against the same model with W + scale B A merged into its nn.Linear / nn.Embedding weights — the config
parser, the adapter directory parser with every refusal, the loader branch, the argument checks of the C ABI.

Bars: 1e-6 of max(1, |value|) on every element of the last hidden state (tests/test_nomic_bert_host.py's pin), on the lengths 1, 7 and 70 in ONE padded
batch with its attention mask (the padded positions are not compared: the engine never runs them).

Measured (JINA3_EXACT lines): base 1.8e-8; merged adapters, worst of the five tasks 2.1e-7."""
import ctypes as C
import json
import os

import pytest
import torch

from marqo_amd import _lib as L
from marqo_amd.engine import archs
from marqo_amd.engine import jina_v3 as J
from tests import jina_v3_ref as N
from tests.test_patch_attn_gpu import MARGIN


def _padded(seqs):
    S = max(len(s) for s in seqs)
    ids = torch.ones(len(seqs), S, dtype=torch.int64)
    mask = torch.zeros(len(seqs), S, dtype=torch.int64)
    for i, s in enumerate(seqs):
        ids[i, :len(s)], mask[i, :len(s)] = s, 1
    return ids, mask


def _worst(ex, ref, seqs, tag):
    worst, r0 = 0.0, 0
    for i, s in enumerate(seqs):
        got, want = ex.final[r0:r0 + len(s)], ref[i, :len(s)]
        err = float(((got - want).abs() / want.abs().clamp(min=1.0)).max())
        print(f"JINA3_EXACT {tag} len={len(s)}: worst |exact - transformers| / max(1, |value|) = {err:.2e}")
        worst = max(worst, err)
        r0 += len(s)
    return worst


# ---- the config ---------------------------------------------------------------------------------------------------------------------------------------
def test_bert_arch_from_hf_config_returns_a_jina_v3_arch():
    b = N.build()
    a = b["arch"]
    assert isinstance(a, archs.JinaV3Arch) and (a.width, a.layers, a.heads, a.head_dim, a.mlp_dim, a.vocab) == (128, 2, 2, 64, 192, 384)
    assert a.rope_theta == 20000.0 and a.max_pos == 2048 and a.type_vocab == 1 and a.ln_eps == 1e-5
    full = archs.resolve_jina_v3(dict(model_type="jina_embeddings_v3", hidden_size=1024, num_attention_heads=16, num_hidden_layers=24,
                                      intermediate_size=4096, vocab_size=250002, max_position_embeddings=8194))
    assert full == archs.JinaV3Arch() and full.max_pos == 8192
    assert archs.resolve_jina_v3(dict(b["cfg"], rope_parameters={"rope_theta": 5000.0, "rope_type": "default"})).rope_theta == 5000.0
    assert archs.resolve_jina_v3(dict(b["cfg"], max_position_embeddings=40000)).max_pos == 8192


@pytest.mark.parametrize("over, what", [
    (dict(hidden_act="relu"), "hidden_act=relu unsupported"),
    (dict(rope_parameters={"rope_type": "dynamic", "rope_theta": 20000.0, "factor": 2.0}), "rope_parameters.rope_type=dynamic unsupported"),
    (dict(num_attention_heads=4), "64-wide heads only"),
    (dict(hidden_size=2112, num_attention_heads=33), "hidden_size=2112 unsupported"),
    (dict(intermediate_size=100), "intermediate_size=100 must be a multiple of 64"),
    (dict(max_position_embeddings=2), "leaves no position"),
])
def test_the_config_refuses_by_key(over, what):
    with pytest.raises(KeyError, match=what):
        archs.bert_arch_from_hf_config(dict(N.build()["cfg"], **over))


def test_the_original_repositorys_custom_code_naming_is_refused():
    cfg = dict(model_type="xlm-roberta", vocab_size=250002, hidden_size=1024, num_hidden_layers=24, num_attention_heads=16, intermediate_size=4096,
               max_position_embeddings=8194, lora_adaptations=list(N.TASKS), position_embedding_type="rotary")
    with pytest.raises(KeyError, match="lora_adaptations is the original jina-embeddings-v3 repository's custom-code naming"):
        archs.bert_arch_from_hf_config(cfg)
    cfg.pop("lora_adaptations")
    cfg["position_embedding_type"] = "absolute"
    assert isinstance(archs.bert_arch_from_hf_config(cfg), archs.BertArch)      # (a plain XLM-RoBERTa keeps its path)


# ---- exact against transformers -----------------------------------------------------------------------------------------------------------------------
def test_exact_is_transformers_in_float64():
    b = N.build()
    seqs = N.random_seqs(N.PIN_LENS, b["cfg"]["vocab_size"], seed=5)
    ids, mask = _padded(seqs)
    with torch.no_grad():
        ref = N.merged_model(b["model"], None)(input_ids=ids, attention_mask=mask).last_hidden_state
    assert ref.dtype == torch.float64
    ex = N.exact(b["arch"], b["tensors"], None, torch.cat(seqs), N.PIN_LENS, None)
    assert float(ex.final.abs().max()) > 1.0           # (working magnitudes: the comparison is not between two zeros)
    assert _worst(ex, ref, seqs, "base") <= 1e-6
    # ... and a LoraSet whose every sequence has no adapter is the base model, exactly
    none = N.exact(b["arch"], b["tensors"], b["lora"].t, torch.cat(seqs), N.PIN_LENS, [-1, -1, -1])
    assert torch.equal(none.final, ex.final)


@pytest.mark.parametrize("task", N.TASKS)
def test_the_lora_delta_is_the_merged_model_in_float64(task):
    b = N.build()
    seqs = N.random_seqs(N.PIN_LENS, b["cfg"]["vocab_size"], seed=6)
    ids, mask = _padded(seqs)
    with torch.no_grad():
        ref = N.merged_model(b["model"], b["adapters"][task])(input_ids=ids, attention_mask=mask).last_hidden_state
        base = N.merged_model(b["model"], None)(input_ids=ids, attention_mask=mask).last_hidden_state
    t = b["lora"].task_id(task)
    ex = N.exact(b["arch"], b["tensors"], b["lora"].t, torch.cat(seqs), N.PIN_LENS, [t, t, t])
    assert _worst(ex, ref, seqs, task) <= 1e-6
    assert float((ref - base)[0, 0].abs().max()) > 0.1          # (the adapter moves the model: the comparison above is not the base model's)


def test_a_mixed_batch_is_each_sequence_under_its_own_task():
    b = N.build()
    seqs = N.random_seqs(N.PIN_LENS, b["cfg"]["vocab_size"], seed=7)
    tasks = [2, -1, 0]
    mixed = N.exact(b["arch"], b["tensors"], b["lora"].t, torch.cat(seqs), N.PIN_LENS, tasks)
    r0 = 0
    for s, t in zip(seqs, tasks):
        alone = N.exact(b["arch"], b["tensors"], b["lora"].t, s, [len(s)], [t])
        assert torch.allclose(mixed.final[r0:r0 + len(s)], alone.final, rtol=0, atol=1e-12)
        r0 += len(s)


def test_the_rounding_model_is_near_exact_and_its_second_history_inside_the_bar():
    b = N.build()
    seqs = N.random_seqs([1, 7, 70], b["cfg"]["vocab_size"], seed=8)
    args = (b["arch"], b["tensors"], b["lora"].t, torch.cat(seqs), [1, 7, 70], [1, -1, 4])
    ex, mo, h1 = N.exact(*args), N.model(*args), N.model(*args, hist=1)
    r = N.row_ratio(h1.final, ex.final, mo.final)["ratio"]
    print(f"JINA3_HIST stream={r:.2f}")
    assert r <= MARGIN and float((mo.final - ex.final).abs().max()) < 0.2


# ---- adapters -----------------------------------------------------------------------------------------------------------------------------------------
def test_adapter_directories_parse_into_the_stacked_layouts(tmp_path):
    b = N.build()
    arch, ads = b["arch"], b["adapters"]
    for task in N.TASKS[:2]:
        N.write_adapter_dir(str(tmp_path / task), ads[task], prefix="roberta." if task == N.TASKS[1] else "")
    (tmp_path / "not_an_adapter").mkdir()
    dirs = J.find_adapter_dirs(str(tmp_path))
    assert list(dirs) == sorted(N.TASKS[:2])
    ls = J.load_adapters(arch, dirs)
    assert ls.names == sorted(N.TASKS[:2]) and ls.rank == 4 and ls.t["scale"].tolist() == [2.0, 2.0]
    i = ls.task_id(N.TASKS[0])
    src = ads[N.TASKS[0]]["tensors"]
    W = arch.width
    assert torch.equal(ls.t["layer.1.qkv_a"][i, 4:8], src["base_model.model.layers.1.self_attn.k_proj.lora_A.weight"])
    assert torch.equal(ls.t["layer.1.qkv_b"][i, 2 * W:], src["base_model.model.layers.1.self_attn.v_proj.lora_B.weight"])
    assert torch.equal(ls.t["layer.0.fc2_a"][i], src["base_model.model.layers.0.mlp.fc2.lora_A.weight"])
    assert torch.equal(ls.t["emb_a"][i], src["base_model.model.embeddings.word_embeddings.lora_embedding_A"].t())
    assert ls.task_id(None) == -1
    with pytest.raises(ValueError, match="unknown LoRA task 'summarise'"):
        ls.task_id("summarise")
    # rsLoRA's scale, a rank that is no multiple of 4 (zero-padded), an adapter of two modules only (the others carry zeros)
    g = torch.Generator().manual_seed(1)
    small = dict(r=6, alpha=12.0, tensors={"base_model.model.layers.0.mlp.fc1.lora_A.weight": torch.randn(6, W, generator=g),
                                           "base_model.model.layers.0.mlp.fc1.lora_B.weight": torch.randn(192, 6, generator=g)})
    d = N.write_adapter_dir(str(tmp_path / "x" / "small"), small, use_rslora=True, target_modules=["fc1"])
    one = J.load_adapters(arch, {"small": d})
    assert one.rank == 8 and abs(float(one.t["scale"][0]) - 12.0 / 6 ** 0.5) < 1e-6 and "emb_a" not in one.t
    assert torch.equal(one.t["layer.0.fc1_a"][0, :6], small["tensors"]["base_model.model.layers.0.mlp.fc1.lora_A.weight"])
    assert float(one.t["layer.0.fc1_a"][0, 6:].abs().max()) == 0.0 and float(one.t["layer.1.qkv_b"].abs().max()) == 0.0


def _broken(ad, **tensors):
    t = dict(ad["tensors"])
    for k, v in tensors.items():
        if v is None:
            t.pop(k)
        else:
            t[k] = v
    return dict(ad, tensors=t)


def test_every_adapter_refusal_says_why(tmp_path):
    b = N.build()
    arch, ad = b["arch"], b["adapters"][N.TASKS[0]]
    qa = "base_model.model.layers.0.self_attn.q_proj.lora_A.weight"
    cases = [
        (ad, dict(target_modules=["q_proj", "LayerNorm"]), r"target_modules \['LayerNorm'\] are outside the six Linears"),
        (ad, dict(bias="all"), "bias='all' is not served"),
        (ad, dict(use_dora=True), "DoRA adapters are not served"),
        (dict(ad, r=32), {}, "rank r=32 is above 16"),
        (ad, dict(rank_pattern={"fc1": 8}), "ranks that differ across modules"),
        (_broken(ad, **{qa: torch.zeros(8, 128)}), {}, "has rank 8 where adapter_config.json says r=4"),
        (_broken(ad, **{qa: None}), {}, "q_proj has lora_B without its other half"),
        (_broken(ad, **{"base_model.model.layers.0.self_attn.q_proj.lora_magnitude_vector": torch.zeros(128)}), {}, "is unexpected"),
        (_broken(ad, **{"base_model.model.layers.5.mlp.fc1.lora_A.weight": torch.zeros(4, 128)}), {}, "names layer 5 of a 2-layer model"),
        (ad, dict(peft_type="IA3"), "peft_type=IA3 is not served"),
    ]
    for i, (adapter, over, what) in enumerate(cases):
        d = N.write_adapter_dir(str(tmp_path / f"case{i}"), adapter, **over)
        with pytest.raises(ValueError, match=what):
            J.read_adapter("t", d, arch)


# ---- the loader ---------------------------------------------------------------------------------------------------------------------------------------
class _Captured(Exception):
    pass


def _capture(monkeypatch):
    seen = {}

    def init(self, arch, sd, device, pooling="mean", precision="bf16", adapters=None, default_task=None):
        seen.update(arch=arch, sd=sd, pooling=pooling, precision=precision, adapters=adapters, default_task=default_task)
        if default_task is not None and (adapters is None or default_task not in adapters.names):     # (the constructor's own first check)
            raise ValueError(f"unknown LoRA task {default_task!r}: this checkpoint has {adapters.names if adapters else 'no adapters'}")
        raise _Captured()
    monkeypatch.setattr(J.JinaV3Tower, "__init__", init)
    return seen


def _model(props):
    from marqo_amd.s2_inference.hugging_face_model import HuggingFaceModel
    return HuggingFaceModel(model_properties=props, device="cuda:0")


@pytest.fixture(scope="module")
def ckpts(tmp_path_factory):
    b, tk = N.build(), N.train_tokenizer()
    root = tmp_path_factory.mktemp("jina3")
    out = {}
    for name in ("bare", "full"):
        d = str(root / name)
        b["model"].save_pretrained(d)
        N.write_tokenizer(d, tk)
        out[name] = d
    for task in N.TASKS:
        N.write_adapter_dir(os.path.join(out["full"], task), b["adapters"][task])
    out["extra"] = N.write_adapter_dir(str(root / "extra"), b["adapters"][N.TASKS[2]])
    out["dora"] = N.write_adapter_dir(str(root / "dora"), b["adapters"][N.TASKS[2]], use_dora=True)
    os.makedirs(os.path.join(out["full"], "1_Pooling"))
    with open(os.path.join(out["full"], "1_Pooling", "config.json"), "w") as f:
        json.dump({"word_embedding_dimension": 128, "pooling_mode_cls_token": True, "pooling_mode_mean_tokens": False}, f)
    return out


def test_hf_loader_takes_a_jina_v3_directory(ckpts, monkeypatch):
    from marqo_amd.engine.tokenizers import HfJsonTokenizer
    from marqo_amd.s2_inference.errors import InvalidModelPropertiesError
    seen = _capture(monkeypatch)
    b = N.build()
    with open(os.path.join(ckpts["bare"], "config.json")) as f:
        assert json.load(f)["model_type"] == "jina_embeddings_v3"
    for d, extra, pool, names, task, tokens, cap in (
            (ckpts["bare"], {}, "mean", None, None, 128, 128),
            (ckpts["bare"], {"trustRemoteCode": True, "loraAdapters": {"sep": ckpts["extra"]}, "loraTask": "sep"}, "mean", ["sep"], "sep", 9000, 2048),
            (ckpts["full"], {"loraTask": "retrieval.query"}, "cls", sorted(N.TASKS), "retrieval.query", 16, 16),
            (ckpts["full"], {"poolingMethod": "mean"}, "mean", sorted(N.TASKS), None, 128, 128)):
        m = _model(dict({"type": "hf", "name": d, "dimensions": 128, "tokens": tokens}, **extra))
        with pytest.raises(_Captured):
            m._load_necessary_components()
        assert isinstance(seen["arch"], archs.JinaV3Arch) and seen["arch"].rope_theta == 20000.0 and seen["pooling"] == pool
        assert (seen["adapters"].names if seen["adapters"] else None) == names and seen["default_task"] == task
        assert isinstance(m._tokenizer, HfJsonTokenizer) and m._tokenizer.pad_id == 1 and m.model_properties.tokens == cap
        t = J.jina_v3_state_dict(seen["arch"], seen["sd"])
        assert all(torch.equal(t[k], b["tensors"][k]) for k in b["tensors"])
        tok = m._tokenizer(["hello world"], max_length=16)["input_ids"][0]
        assert int(tok[0]) == 0 and int(tok[-1]) == 2          # <s> ... </s>
    ok = {"type": "hf", "name": ckpts["full"], "dimensions": 128}
    for over, what in ((dict(enginePrecision="fp8"), "'enginePrecision': 'fp8' is not available for Jina v3 encoders"),
                       (dict(poolingMethod="last"), "Original error pooling_method must be 'mean' or 'cls'"),
                       (dict(dimensions=64), "'dimensions'=64 but the encoder width is 128"),
                       (dict(loraTask="summarise"), "unknown LoRA task 'summarise'"),
                       (dict(loraAdapters={"d": ckpts["dora"]}), "DoRA adapters are not served"),
                       (dict(loraAdapters=["x"]), "'loraAdapters' must map task names to adapter directories")):
        with pytest.raises(InvalidModelPropertiesError, match=what):
            _model(dict(ok, **over))._load_necessary_components()
    with pytest.raises(InvalidModelPropertiesError, match="unknown LoRA task 'retrieval.query'.*no adapters"):
        _model({"type": "hf", "name": ckpts["bare"], "dimensions": 128, "loraTask": "retrieval.query"})._load_necessary_components()


def test_registry_is_unchanged():
    from marqo_amd.s2_inference import s2_inference as S
    mp = S.load_model_properties()
    assert len(mp["models"]) == 204 and not any("jina-embeddings-v3" in n.lower() for n in mp["models"])


# ---- the C ABI without a GPU --------------------------------------------------------------------------------------------------------------------------
def test_struct_sizes_header_and_argument_checks():
    assert [C.sizeof(s) for s in (L.JinaV3Layer, L.JinaV3Weights, L.JinaV3Cfg, L.JinaV3LoraLayer, L.JinaV3Lora)] == [96, 48, 40, 64, 40]
    text = L.HEADER_PATH.read_text()
    for name in ("mq_lora_down", "mq_lora_up", "mq_lora_gather", "mq_encode_jina_v3", "mq_jina_v3_workspace_bytes"):
        assert name in text and name in L.EXPORTED_SYMBOLS
    assert "#define MQ_ABI_VERSION 15" in text and "lora" in L.NO_SCRATCH_UNITS
    head = (L.CSRC_DIR / "lora.hip").read_text().split("#include")[0]
    assert "no scratch" in head and "VGPRs" in head and "SGPRs" in head
    lib = L.load()
    fake = C.c_void_p(4096)
    seq = (C.c_int32 * 2)(0, 1)

    def refused(rc, what):
        assert rc == -1 and what in lib.mq_last_error(), lib.mq_last_error()
    down = lambda R=12, K=128, tasks=2, h=seq, lda=None: lib.mq_lora_down(fake, K if lda is None else lda, fake, fake, fake, h, fake, 2, 0, 10, tasks, R, K,
                                                                         fake, None)
    refused(down(R=68), b"mq_lora_down: R 68 must be a multiple of 4 in [4, 64]")
    refused(down(R=6), b"mq_lora_down: R 6 must be")
    refused(down(K=100), b"mq_lora_down: K 100 must be a multiple of 64")
    refused(down(lda=64), b"mq_lora_down: lda 64")
    refused(down(tasks=1), b"mq_lora_down: task id 1 of sequence 1 is not below tasks 1")
    refused(down(h=None), b"mq_lora_down: null task list")
    up = lambda R=12, r=4, nb=3, N=384, ldc=384, mode=0, act=0, tasks=2: lib.mq_lora_up(fake, R, fake, r, nb, fake, seq, fake, 2, 0, 10, tasks, fake, ldc, N,
                                                                                      mode, act, None)
    refused(up(r=20, R=60), b"mq_lora_up: rank 20")
    refused(up(R=16), b"mq_lora_up: R 16 is not nblocks 3 x rank 4")
    refused(up(N=386), b"mq_lora_up: N 386")
    refused(up(ldc=380), b"mq_lora_up: ldc 380")
    refused(up(mode=3), b"mq_lora_up: bad mode 3")
    refused(up(mode=0, act=1), b"mq_lora_up: act 1")
    refused(up(tasks=1), b"mq_lora_up: task id 1 of sequence 1 is not below tasks 1")
    refused(lib.mq_lora_gather(fake, fake, fake, fake, seq, fake, 2, 0, 10, 1, 4, 100, fake, None), b"mq_lora_gather: task id 1")
    none = (C.c_int32 * 2)(-1, -1)     # no sequence has an adapter: nothing to launch (accumulate), no device is touched
    assert lib.mq_lora_down(fake, 128, fake, fake, fake, none, fake, 2, 0, 10, 2, 12, 128, fake, None) == 0
    assert lib.mq_lora_up(fake, 12, fake, 4, 3, fake, none, fake, 2, 0, 10, 2, fake, 384, 384, L.MQ_LORA_ACCUM, 0, None) == 0
    # the tower
    mk = lambda **kw: L.JinaV3Cfg(**dict(dict(width=128, layers=1, heads=2, head_dim=64, mlp_dim=256, vocab=10, max_pos=64, pool=L.MQ_POOL_MEAN, ln_eps=1e-5), **kw))
    enc = lambda cfg, w, lora, h_task, nseq=0, cu=None, ws=0: lib.mq_encode_jina_v3(C.byref(cfg), C.byref(w), lora, fake, fake, cu, fake, h_task, nseq, fake, 1,
                                                                                    fake, ws, None)
    for kw, what in ((dict(head_dim=128, heads=1), b"head_dim 128 unsupported"), (dict(width=2112, heads=33), b"width 2112"),
                     (dict(mlp_dim=100), b"mlp_dim 100"), (dict(max_pos=9000), b"max_pos 9000"), (dict(pool=L.MQ_POOL_LAST), b"bad pooling 2")):
        refused(enc(mk(**kw), L.JinaV3Weights(), None, None), b"mq_encode_jina_v3: " + what)
    cfg = mk()
    layers = (L.JinaV3Layer * 1)(L.JinaV3Layer(*([4096] * 12)))
    w = L.JinaV3Weights(tok_emb=4096, type0=4096, emb_ln_g=4096, emb_ln_b=4096, d_inv_freq=4096, layers=layers)
    refused(enc(cfg, L.JinaV3Weights(), None, None), b"mq_encode_jina_v3: null weight pointer")
    holed = (L.JinaV3Layer * 1)(L.JinaV3Layer(*([4096] * 11)))
    refused(enc(cfg, L.JinaV3Weights(tok_emb=4096, type0=4096, emb_ln_g=4096, emb_ln_b=4096, d_inv_freq=4096, layers=holed), None, None),
            b"layer 0 has null weights")
    assert enc(cfg, w, None, None) == 0      # nseq 0: nothing to do
    ll = (L.JinaV3LoraLayer * 1)(L.JinaV3LoraLayer(*([4096] * 8)))
    lora = lambda **kw: C.byref(L.JinaV3Lora(**dict(dict(tasks=2, rank=4, d_scale=4096, emb_a=4096, emb_b=4096, layers=ll), **kw)))
    refused(enc(cfg, w, lora(rank=5), seq), b"lora rank 5 must be 4, 8, 12 or 16")
    refused(enc(cfg, w, lora(rank=20), seq), b"lora rank 20")
    refused(enc(cfg, w, lora(emb_b=None), seq), b"needs both emb_a and emb_b")
    refused(enc(cfg, w, lora(layers=(L.JinaV3LoraLayer * 1)(L.JinaV3LoraLayer(*([4096] * 7)))), seq), b"lora layer 0 has null adapter tensors")
    refused(enc(cfg, w, lora(), None), b"needs the task list")
    cu = (C.c_int32 * 3)(0, 5, 12)
    refused(enc(cfg, w, lora(tasks=1), seq, 2, cu, 1 << 30), b"mq_encode_jina_v3: task id 1 of sequence 1 is not below tasks 1")
    need = lib.mq_jina_v3_workspace_bytes(C.byref(cfg), 12, 2)
    assert need >= 12 * (128 * 8 + 384 * 2 + 48 * 4) and lib.mq_jina_v3_workspace_bytes(None, 12, 2) == 0
    assert enc(cfg, w, lora(), seq, 2, cu, need - 1) == -3 and b"mq_encode_jina_v3: workspace" in lib.mq_last_error()      # MQ_ERR_WORKSPACE
    assert lib.mq_abi_version() == L.ABI_VERSION == 15

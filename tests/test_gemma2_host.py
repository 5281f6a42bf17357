"""Gemma2 on the host (no GPU): config parsing on the shapes of Gemma-2-2B and -9B (written from memory of the public configs), every refusal by its key —
the arch's and the `hf` loader's —, and the tiny float64 transformers Gemma2Models that tests/test_gemma2_gpu.py takes as its reference: TINY (width 128)
and WIDE (2112: the row kernels above 2048 run), 4 layers (sliding, full, sliding, full), heads (4, 2) of 256, window 8, cap 4.  With the cap removed,
and with the window at 512, transformers' own model moves the pooled rows by more than 10 x COS_TOL: a tower that ignored either would fail."""
import pytest
import torch

from marqo_amd.engine import archs
from tests import gemma_ref as G
from tests import qwen_ref as Q

COS_TOL = 3e-4   # tests/test_modernbert_gpu.py's bar, which the GPU test imports
TINY = dict(model_type="gemma2", vocab_size=300, hidden_size=128, num_hidden_layers=4, num_attention_heads=4, num_key_value_heads=2, head_dim=256,
            intermediate_size=256, max_position_embeddings=512, rms_norm_eps=1e-6, hidden_activation="gelu_pytorch_tanh", query_pre_attn_scalar=64,
            sliding_window=8, attn_logit_softcapping=4.0, final_logit_softcapping=30.0, rope_theta=10000.0, pad_token_id=0, eos_token_id=1, bos_token_id=2)
CONFIGS, LENS = {"TINY": TINY, "WIDE": dict(TINY, hidden_size=2112)}, [1, 9, 40, 70]
GEMMA2_9B = dict(TINY, vocab_size=256000, max_position_embeddings=8192, attn_logit_softcapping=50.0, sliding_window=4096, query_pre_attn_scalar=256,
                 hidden_size=3584, num_hidden_layers=42, num_attention_heads=16, num_key_value_heads=8, intermediate_size=14336)
GEMMA2_2B = dict(GEMMA2_9B, hidden_size=2304, num_hidden_layers=26, num_attention_heads=8, num_key_value_heads=4, intermediate_size=9216)


def hf_model(cfg, seed=1, **edit):
    # gemma_ref.randomize's weights at gain 1.5; the token table, which the model scales by sqrt(width), kept at TINY's size (the blocks matter as much)
    import transformers
    kw = {k: v for k, v in {**cfg, **edit}.items() if k != "model_type"}
    model = transformers.Gemma2Model(transformers.Gemma2Config(**kw, attn_implementation="eager")).double().eval()
    G.randomize(model, seed, 1.5)
    with torch.no_grad():
        model.embed_tokens.weight.mul_((128 / model.config.hidden_size) ** 0.5)
    return model


def pooled_rows(model, seqs, pooling):
    with torch.no_grad():
        hid = [model(input_ids=s[None]).last_hidden_state[0].double() for s in seqs]
    return torch.stack([h[-1] if pooling == "last" else h.mean(0) for h in hid])


def cos_err(out, ref):
    return 1 - (out.double().cpu() * ref).sum(-1) / (out.double().cpu().norm(dim=-1) * ref.norm(dim=-1))


@pytest.mark.parametrize("cfg,shape", ((GEMMA2_2B, (2304, 26, 8, 4, 9216)), (GEMMA2_9B, (3584, 42, 16, 8, 14336))))
def test_the_real_shapes_parse(cfg, shape):
    a = archs.gemma2_arch_from_hf_config(cfg)
    assert (a.width, a.layers, a.heads, a.kv_heads, a.mlp_dim) == shape and (a.head_dim, a.max_pos, a.softcap, a.window, a.attn_scale) == (256, 8192, 50.0, 4096, 1 / 16)
    assert a.sliding == tuple(i % 2 == 0 for i in range(a.layers))     # transformers' default: the first layer slides
    assert not any(archs.gemma2_arch_from_hf_config(dict(cfg, layer_types=["full_attention"] * a.layers)).sliding)
    with pytest.raises(KeyError, match="model_type=gemma2 is not a BERT-family encoder"):
        archs.bert_arch_from_hf_config(cfg)


@pytest.mark.parametrize("edit,key", (
    (dict(head_dim=128), "head_dim=128"), (dict(hidden_size=4608), "hidden_size=4608"), (dict(hidden_size=2300), "hidden_size=2300"),
    (dict(attn_logit_softcapping=None), "attn_logit_softcapping=None"), (dict(attn_logit_softcapping=65.0), "attn_logit_softcapping=65.0"),
    (dict(rope_scaling={"type": "linear", "factor": 2.0}), "rope_scaling="), (dict(hidden_activation="gelu"), "hidden_activation=gelu")))
def test_config_refusals_name_the_key(edit, key):
    with pytest.raises(KeyError, match=key):
        archs.gemma2_arch_from_hf_config(dict(GEMMA2_9B, **edit))


@pytest.mark.parametrize("props,edit,msg", (
    (dict(enginePrecision="fp8"), {}, "'enginePrecision': 'fp8' is not available for Gemma2 encoders .*gated tanh-GELU"),
    (dict(poolingMethod="cls"), {}, "pooling_method 'cls' is not available for Gemma2"),
    (dict(weightPrecision="e4m3"), {}, "'weightPrecision': 'e4m3' is available for Mistral / Llama checkpoints only"),
    ({}, dict(attn_logit_softcapping=None), "attn_logit_softcapping=None unsupported(?!.*BERT-family)")))
def test_the_hf_loader_refuses_by_name(tmp_path, props, edit, msg):
    from marqo_amd.s2_inference.errors import InvalidModelPropertiesError
    from marqo_amd.s2_inference.hugging_face_model import HuggingFaceModel
    d = Q.write_checkpoint_dir(str(tmp_path / "g2"), dict(TINY, **edit), {"model.x": torch.zeros(1)}, Q.train_tokenizer())
    with pytest.raises(InvalidModelPropertiesError, match=msg):
        HuggingFaceModel(model_properties={"type": "hf", "name": d, "dimensions": 128, **props}, device="cuda:0")._load_necessary_components()


@pytest.mark.parametrize("name", tuple(CONFIGS))
def test_the_cap_and_the_window_matter_to_the_test_models(name):
    seqs = G.random_seqs(LENS, 300, seed=3)
    for pooling in ("last", "mean"):
        ref = pooled_rows(hf_model(CONFIGS[name]), seqs, pooling)
        for edit in (dict(attn_logit_softcapping=None), dict(sliding_window=512)):
            moved = float(cos_err(pooled_rows(hf_model(CONFIGS[name], **edit), seqs, pooling), ref).max())
            print(f"GEMMA2_COND {name} {pooling} {edit}: {moved:.2e} (needs > {10 * COS_TOL:.0e})")
            assert moved > 10 * COS_TOL, (name, pooling, edit, moved)

"""The mixture-of-experts NomicBERT on the host: which config.json files select it, every refusal by the name of its key, the single-key files that stay
refused with the text they had, and the state-dict transform (per-expert slices, the w2 transpose, a routed block recognised from its tensors)."""
import pytest
import torch

from marqo_amd.engine import archs, tower_weights as TW
from tests import nomic_bert_ref as N
from tests import nomic_moe_ref as M


def test_both_keys_select_the_moe_arch():
    a = archs.bert_arch_from_hf_config(M.hub_config())
    assert isinstance(a, archs.NomicMoeArch)
    assert (a.width, a.heads, a.layers, a.mlp_dim, a.experts, a.top_k, a.rope_theta, a.type_vocab, a.ln_eps) == (128, 2, 4, 192, 4, 2, 10000.0, 1, 1e-5)
    assert archs.bert_arch_from_hf_config(M.hub_config(n_positions=32768)).max_pos == 8192


@pytest.mark.parametrize("over,what", (
    (dict(moe_top_k=3), "moe_top_k=3"), (dict(moe_top_k=0), "moe_top_k=0"), (dict(num_experts=2, moe_top_k=2, n_inner=100), "n_inner=100"),
    (dict(num_experts=17), "num_experts=17"), (dict(moe_normalize_expert_weights=1.0), "moe_normalize_expert_weights=1.0"),
    (dict(expert_choice_router=True), "expert_choice_router=True"), (dict(activation_function="swiglu"), "activation_function=swiglu"),
    (dict(prenorm=True), "prenorm=True"), (dict(use_rms_norm=True), "use_rms_norm=True"), (dict(rotary_scaling_factor=2), "rotary_scaling_factor=2"),
    (dict(rotary_emb_fraction=0.5), "rotary_emb_fraction=0.5"), (dict(n_head=4), "n_embd=128 / n_head=4"),
    (dict(n_embd=2112, n_head=33), "n_embd=2112 unsupported"), (dict(mlp_fc1_bias=False), "mlp_fc1_bias=False"),
))
def test_moe_config_refuses_by_key(over, what):
    with pytest.raises(KeyError, match=what.replace("(", "\\(")):
        archs.bert_arch_from_hf_config(M.hub_config(**over))


@pytest.mark.parametrize("cfg", (N.hub_config, N.native_config))
@pytest.mark.parametrize("over,what", (
    (dict(moe_every_n_layers=2), "moe_every_n_layers=2 unsupported (mixture-of-experts NomicBERT, nomic-embed-text-v2-moe, is not served)"),
    (dict(num_experts=8), "num_experts=8 unsupported (mixture-of-experts NomicBERT, nomic-embed-text-v2-moe, is not served)"),
))
def test_one_key_alone_keeps_its_refusal(cfg, over, what):
    with pytest.raises(KeyError) as e:
        archs.bert_arch_from_hf_config(cfg(**over))
    assert e.value.args[0] == what


@pytest.mark.parametrize("over,what", ((dict(activation_function="gelu"), "activation_function=gelu"), (dict(mlp_fc1_bias=True), "mlp_fc1_bias=True")))
def test_a_dense_gelu_or_biased_config_stays_refused(over, what):
    with pytest.raises(KeyError, match=what):
        archs.bert_arch_from_hf_config(N.hub_config(**over))


def test_state_dict_transform_slices_and_transposes_bit_exactly():
    b = M.build()
    arch, sd, t = b["arch"], b["sd"], b["tensors"]
    E, F, W = arch.experts, arch.mlp_dim, arch.width
    for l in range(arch.layers):
        src, p = f"encoder.layers.{l}.", f"layer.{l}."
        routed = src + "mlp.router.layer.weight" in sd
        assert routed == (l in (1, 3)) and routed == (p + "moe.w1" in t) and routed != (p + "mlp.fc1.weight" in t)
        if routed:
            assert t[p + "moe.router.weight"].dtype == torch.float32 and torch.equal(t[p + "moe.router.weight"], sd[src + "mlp.router.layer.weight"])
            for e in range(E):
                assert torch.equal(t[p + "moe.w1"][e], sd[src + "mlp.experts.mlp.w1"][e * F:(e + 1) * F])
                assert torch.equal(t[p + "moe.w2t"][e], sd[src + "mlp.experts.mlp.w2"][e * F:(e + 1) * F].T)
            assert t[p + "moe.w2t"].shape == (E, W, F) and t[p + "moe.w2t"].is_contiguous() and torch.equal(t[p + "moe.bias"], sd[src + "mlp.experts.bias"])


def test_a_block_is_routed_by_its_tensors_not_its_index():
    b = M.build()
    sd = dict(b["sd"])
    for name in ("router.layer.weight", "experts.mlp.w1", "experts.mlp.w2", "experts.bias"):         # block 0 takes block 1's routed MLP, block 1 block 0's dense one
        sd["encoder.layers.0.mlp." + name] = sd.pop("encoder.layers.1.mlp." + name)
    for name in ("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias"):
        sd["encoder.layers.1.mlp." + name] = sd.pop("encoder.layers.0.mlp." + name)
    t = TW.nomic_moe_state_dict(b["arch"], sd)
    assert "layer.0.moe.w1" in t and "layer.1.mlp.fc1.weight" in t and "layer.1.moe.w1" not in t
    del sd["encoder.layers.2.mlp.fc1.weight"]
    with pytest.raises(ValueError, match="block 2 has neither"):
        TW.nomic_moe_state_dict(b["arch"], sd)

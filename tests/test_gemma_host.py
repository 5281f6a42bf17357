"""EmbeddingGemma on the host (no GPU): the project's fp32 oracle of the tower against transformers' Gemma3TextModel (eager attention, fp32,
use_bidirectional_attention, random weights from tiny configs), the band mask against the mask transformers builds, the config parser and its refusals,
a tile-order arithmetic model of csrc/attention_gqa256.hip whose deliberate faults leave the rounding budget of tests/attention_ref.py, and the tanh-GELU
product's budget, which the erf form fails.

Tolerance of the oracle comparison: both sides are fp32 torch on the CPU computing the same graph; they differ by the association order of fp32 sums only.
Measured on right-padded batches of lengths [1, 17, 70] at the real rows: 7.2e-7 on each of TINY, TINY_SLIDING and TINY_FULL.
ORACLE_ATOL = 3e-5 is that of tests/test_qwen_host.py.

The arithmetic model at 256-deep dot products: the budget u (P|V| + |out|), u = 2**-8, has no term that grows with the head width — the Q.K sums are fp32
accumulations of exact bf16 x bf16 products, 256 x 2**-24 relative at worst, five orders below u — and the model stays within 1.0 x on every input of the
GPU test (measured worst 0.98), so no term is missing and the margin is not widened."""
import pytest
import torch

from marqo_amd.engine import archs
from tests import attention_ref as AR
from tests import gemma_ref as G

ORACLE_ATOL = 3e-5

# ---- the inputs of tests/test_attention_gqa256_gpu.py: (q_heads, kv_heads), half_window, packed lengths -------------------------------------------------
HEADS = [(3, 1), (2, 2), (4, 2)]            # the checkpoint's; no K/V head shared; the K/V head index matters
WINDOWS = [0, 1, 16, 64, 256]
PACKS = [[1], [15, 16, 17], [63, 64, 65], [129, 1, 33], [127, 128, 129]]   # [63, 64, 65]: around the 64-query slice; [127 .. 129]: around one LDS piece


def gpu_cases():
    """every (heads, half_window, lens) the GPU test runs.  The checkpoint's head shape takes every window on every pack; the other two a subset.  Around
    hw and 2 hw + 1 (where the band first stops covering the sequence), and one length of about 600 at hw 64 and 256, where whole tiles fall outside a
    block's band and the skip path runs."""
    out = [((3, 1), hw, lens) for hw in WINDOWS for lens in PACKS]
    out += [(hs, hw, lens) for hs in HEADS[1:] for hw in (0, 16, 256) for lens in ([15, 16, 17], [129, 1, 33])]
    for hw in WINDOWS[1:]:
        out.append(((3, 1), hw, [max(hw - 1, 1), hw, hw + 1]))
        out.append(((3, 1), hw, [2 * hw, 2 * hw + 1, 2 * hw + 2]))
    out.append(((4, 2), 16, [32, 33, 34]))
    out += [((3, 1), 64, [600]), ((4, 2), 64, [600]), ((3, 1), 256, [601]), ((2, 2), 256, [601])]
    return out


# (heads, half_window, lens): a subset that shows every fault — two rounds of work items and several pieces ((3, 1) at 600 tokens), a shared and an
# unshared K/V head, a band of one key
MUTANT_SHAPES = [((3, 1), 16, [129, 1, 33]), ((4, 2), 1, [63, 64, 65]), ((3, 1), 64, [600]), ((2, 2), 0, [129, 1, 33]), ((4, 2), 256, [601])]


# ---- the fp32 oracle against transformers ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def models():
    return {k: G.hf_model(cfg, seed=i + 1) for i, (k, cfg) in enumerate(G.TINIES.items())}


@pytest.mark.parametrize("name", tuple(G.TINIES))
def test_oracle_equals_transformers(models, name):
    cfg, model = G.TINIES[name], models[name]
    arch = archs.bert_arch_from_hf_config(cfg)
    assert isinstance(arch, archs.GemmaArch) and arch.half_window == 4 and arch.head_dim == 256
    assert arch.sliding == tuple(t == "sliding_attention" for t in model.config.layer_types)
    assert model.config.sliding_window == 5        # transformers: 8 // 2 + 1, exclusive
    seqs = G.random_seqs([1, 17, 70], cfg["vocab_size"], seed=2)
    ids, mask = G.pad_batch(seqs)
    with torch.no_grad():
        ref = model(input_ids=ids, attention_mask=mask).last_hidden_state
    sd = G.state_dict_of(model)
    got = G.oracle_hidden(sd, arch, ids, mask)
    d = max(float((got[i, :len(s)] - ref[i, :len(s)]).abs().max()) for i, s in enumerate(seqs))
    print(f"GEMMA_ORACLE {name}: max |oracle - transformers| = {d:.3e} (bar {ORACLE_ATOL:.0e})")
    assert d < ORACLE_ATOL
    # the packed form (what the tower runs) gives the padded form's real rows: padded keys are masked
    for i, h in enumerate(G.oracle_hidden_packed(sd, arch, seqs)):
        assert float((h - got[i, :len(seqs[i])]).abs().max()) < ORACLE_ATOL
    # a window off by one, a dropped q_norm and the erf form of GELU are far outside the bar
    import dataclasses
    if any(arch.sliding):
        for hw in (3, 5):
            wrong = G.oracle_hidden(sd, dataclasses.replace(arch, half_window=hw), ids, mask)
            assert float((wrong[2, :70] - ref[2, :70]).abs().max()) > 100 * ORACLE_ATOL
    zeros = {k: torch.zeros_like(v) if k.endswith("q_norm.weight") else v for k, v in sd.items()}
    assert float((G.oracle_hidden(zeros, arch, ids, mask)[2, :70] - ref[2, :70]).abs().max()) > 100 * ORACLE_ATOL


@pytest.mark.parametrize("sw", (4, 5, 512))
def test_band_mask_is_the_mask_transformers_builds(sw):
    """a file on disk says sliding_window = sw; Gemma3TextConfig makes it sw // 2 + 1 and the sliding layers mask |i - j| < that: half_window = sw // 2"""
    from transformers.models.gemma3.modeling_gemma3 import _bidirectional_window_overlay, create_sliding_window_causal_mask
    cfg = G.config_dict(G.TINY, sliding_window=sw, max_position_embeddings=2048)
    arch = archs.gemma_arch_from_hf_config(cfg)
    assert arch.half_window == sw // 2
    config = G.hf_config(cfg)
    assert config.sliding_window == sw // 2 + 1
    S = 2 * sw + 9
    m = create_sliding_window_causal_mask(config=config, inputs_embeds=torch.zeros(1, S, cfg["hidden_size"]), attention_mask=torch.ones(1, S, dtype=torch.long),
                                          past_key_values=None, position_ids=torch.arange(S)[None],
                                          or_mask_function=_bidirectional_window_overlay(config.sliding_window))
    assert m is not None and m.shape[-2:] == (S, S)
    seen = m[0, 0] if m.dtype == torch.bool else m[0, 0] == 0
    assert bool((seen == G.band_allowed(S, arch.half_window)).all())
    assert not bool((seen == G.band_allowed(S, arch.half_window + 1)).all()) and not bool((seen == G.band_allowed(S, arch.half_window - 1)).all())


# ---- the config parser -------------------------------------------------------------------------------------------------------------------------------
def test_arch_parser_reads_both_spellings():
    a = archs.gemma_arch_from_hf_config(G.TINY)
    assert (a.theta_global, a.theta_local) == (1000000.0, 10000.0) and a.sliding == (True, True, False) and a.attn_scale == 256 ** -0.5
    new = G.config_dict(G.TINY, rope_theta=None, rope_local_base_freq=None, sliding_window_pattern=None,
                        layer_types=["sliding_attention", "full_attention", "sliding_attention"],
                        rope_parameters={"full_attention": {"rope_type": "default", "rope_theta": 500000.0},
                                         "sliding_attention": {"rope_type": "default", "rope_theta": 20000.0}})
    b = archs.gemma_arch_from_hf_config(new)
    assert (b.theta_global, b.theta_local) == (500000.0, 20000.0) and b.sliding == (True, False, True)
    c = archs.gemma_arch_from_hf_config(G.config_dict(G.TINY, num_hidden_layers=12, sliding_window_pattern=None))     # pattern 6 when absent
    assert c.sliding == tuple((i + 1) % 6 != 0 for i in range(12))
    real = archs.gemma_arch_from_hf_config(G.config_dict(G.TINY, sliding_window=512, hidden_size=768, num_attention_heads=3, num_hidden_layers=24,
                                                         sliding_window_pattern=6, intermediate_size=1152, max_position_embeddings=2048))
    assert real.half_window == 256 and real.sliding.count(False) == 4 and real.max_pos == 2048
    assert isinstance(archs.bert_arch_from_hf_config(G.TINY), archs.GemmaArch)


@pytest.mark.parametrize("over, what", [
    (dict(use_bidirectional_attention=False), "use_bidirectional_attention=False"), (dict(use_bidirectional_attention=None), "use_bidirectional_attention=None"),
    (dict(attn_logit_softcapping=50.0), "attn_logit_softcapping=50.0"), (dict(rope_scaling={"rope_type": "linear", "factor": 8.0}), "rope_scaling="),
    (dict(rope_parameters={"full_attention": {"rope_type": "yarn", "rope_theta": 1e6}}), "rope_type=yarn"),
    (dict(rope_parameters={"full_attention": {"rope_type": "default", "factor": 8.0}}), "rope_parameters[full_attention]"),
    (dict(head_dim=128), "head_dim=128"), (dict(hidden_activation="gelu"), "hidden_activation=gelu"),
    (dict(max_position_embeddings=32768), "max_position_embeddings=32768"), (dict(hidden_size=2560), "hidden_size=2560")])
def test_arch_parser_refuses_by_key(over, what):
    with pytest.raises(KeyError, match=what.replace("[", r"\[").replace("]", r"\]")):
        archs.bert_arch_from_hf_config(G.config_dict(G.TINY, **over))


def test_state_dict_folds_the_plus_one_and_fuses():
    from marqo_amd.engine.tower_weights import gemma_state_dict
    model = G.hf_model(G.TINY, seed=5)
    arch = archs.gemma_arch_from_hf_config(G.TINY)
    sd = G.state_dict_of(model, prefix="model.")
    t = gemma_state_dict(arch, sd)
    assert torch.equal(t["norm.weight"], 1.0 + sd["model.norm.weight"]) and torch.equal(t["layers.1.self_attn.k_norm.weight"], 1.0 + sd["model.layers.1.self_attn.k_norm.weight"])
    assert torch.equal(t["layers.0.mlp.up_gate.weight"], torch.cat([sd["model.layers.0.mlp.up_proj.weight"], sd["model.layers.0.mlp.gate_proj.weight"]]))
    assert t["layers.2.self_attn.qkv.weight"].shape == (4 * 256, 128)
    with pytest.raises(KeyError, match="q_norm"):
        gemma_state_dict(arch, {k: v for k, v in sd.items() if "layers.1.self_attn.q_norm" not in k})


# ---- the arithmetic model of the kernel and its faults -----------------------------------------------------------------------------------------------
def test_arithmetic_model_stays_inside_the_budget_on_every_gpu_input():
    worst = 0.0
    for hs, hw, lens in gpu_cases():
        for fam in ("readout", "peaked"):
            qkv = G.make_band_qkv(fam, lens, *hs, seed=sum(lens) + hs[0])
            out, absout = G.band_gqa_reference(qkv, lens, *hs, G.HD, hw)
            r = AR.worst_ratio(G.emulate_band(qkv, lens, *hs, G.HD, hw), out, absout)
            print(f"GQA256_MODEL heads={hs} hw={hw} lens={lens} family={fam} ratio={r:.4f}")
            worst = max(worst, r)
            assert r <= 1.0, (hs, hw, lens, fam, r)
    print(f"GQA256_MODEL worst {worst:.4f}")


@pytest.fixture(scope="module")
def mutant_cases():
    out = {}
    for i, (hs, hw, lens) in enumerate(MUTANT_SHAPES):
        qkv = G.make_band_qkv("readout", lens, *hs, seed=3 + i)
        out[i] = (qkv, *G.band_gqa_reference(qkv, lens, *hs, G.HD, hw))
    return out


@pytest.mark.parametrize("mutant", G.BAND_MUTANTS)
def test_every_fault_leaves_the_budget(mutant_cases, mutant):
    """each fault is far outside the margin the GPU test allows (1.25) on at least one of the shapes"""
    worst = 0.0
    for i, (hs, hw, lens) in enumerate(MUTANT_SHAPES):
        qkv, out, absout = mutant_cases[i]
        r = AR.worst_ratio(G.emulate_band(qkv, lens, *hs, G.HD, hw, mutant=mutant), out, absout)
        print(f"GQA256_MUTANT {mutant} heads={hs} hw={hw} lens={lens} ratio={r:.1f}")
        worst = max(worst, r)
    assert worst > 50.0


def test_reference_equals_attention_ref_without_a_band():
    """hw = 0 is qwen_ref.gqa_reference unmasked (the scale of both is 1 / sqrt(256)); a band that covers the sequence is no band"""
    from tests import qwen_ref as Q
    for hs, lens in (((3, 1), [129, 1, 33]), ((4, 2), [15, 16, 17])):
        qkv = G.make_band_qkv("randn", lens, *hs, seed=9)
        out, absout = G.band_gqa_reference(qkv, lens, *hs, G.HD, 0)
        o2, a2 = Q.gqa_reference(qkv, lens, *hs, G.HD, AR.MASK_NONE)
        assert float((out - o2).abs().max()) < 1e-12 and float((absout - a2).abs().max()) < 1e-12
        o3, _ = G.band_gqa_reference(qkv, lens, *hs, G.HD, max(lens) - 1)
        assert float((out - o3).abs().max()) < 1e-12


# ---- the tanh-GELU product ----------------------------------------------------------------------------------------------------------------------------
def test_the_erf_form_fails_the_tanh_budget():
    """on the GPU test's input, up * gelu_tanh(gate) computed in fp32 and rounded to bf16 stays inside glu_tanh_budget; the erf form (MQ_ACT_GELU's) leaves it
    by a wide factor: the two differ by several percent of their value for gate in [-4, -2], against a budget of half a bf16 ulp (0.2 - 0.4 percent)"""
    buf = G.glu_tanh_input()
    ref, gate = G.glu_tanh_reference(buf)
    bud = G.glu_tanh_budget(ref, gate)
    F = buf.shape[1] // 2
    up, g32 = buf[:, :F].float(), buf[:, F:].float()
    # the kernel's form, x / (1 + exp(-2u)) in fp32: relatively accurate in the negative tail, where 0.5 x (1 + tanh(u)) cancels
    u = torch.tensor(0.7978845608028654) * (g32 * (1.0 + torch.tensor(0.044715) * (g32 * g32)))
    tanh_form = (up * (g32 / (1.0 + torch.exp(-2.0 * u)))).to(torch.bfloat16).double()
    erf_form = (up * torch.nn.functional.gelu(g32)).to(torch.bfloat16).double()
    ok = bud > 0
    r_tanh = float(((tanh_form - ref).abs()[ok] / bud[ok]).max())
    r_erf = float(((erf_form - ref).abs()[ok] / bud[ok]).max())
    print(f"GEMMA_GLU host: tanh form {r_tanh:.3f} x budget, erf form {r_erf:.1f} x budget")
    assert r_tanh <= 1.25 and r_erf > 10.0

"""The LanguageBind restatement (tests/languagebind_ref.py) without a GPU: with `add_time_attn` off it is transformers' CLIP on the same weights,
and the temporal attention by strided indexing (the kernel's walk) is the one by explicit rearrange (the reference's formulation)."""
import pytest
import torch

from tests import languagebind_ref as LBR

TOL = 2e-5      # absolute, the bound of tests/test_oracle_golden.py


def _ids(n, seed=0):
    """[n, 77] rows SOT, random ids, EOT, padded with the EOT id (the reference's tokenizer pads with its EOS)"""
    g = torch.Generator().manual_seed(seed)
    ids = torch.full((n, LBR.CTX), LBR.VOCAB - 1, dtype=torch.int64)
    for i in range(n):
        ln = 2 + (i * 19) % (LBR.CTX - 3)
        ids[i, 0] = LBR.VOCAB - 2
        ids[i, 1:1 + ln] = torch.randint(0, LBR.VOCAB - 2, (ln,), generator=g)
    return ids


@pytest.mark.parametrize("act", ["gelu", "quick_gelu"])
def test_restatement_without_time_attention_is_transformers_clip(act):
    """transformers' CLIP classes load these keys as they are: `vision_model.pre_layrnorm` is their spelling too (position_ids is a buffer they
    derive)"""
    import transformers
    cfg = LBR.config(LBR.SMALL, add_time_attn=False, hidden_act=act)
    sd = LBR.synthetic_state_dict(cfg, seed=3)
    v, t = cfg["vision_config"], cfg["text_config"]
    keep = lambda c: {k: c[k] for k in ("hidden_size", "num_hidden_layers", "num_attention_heads", "intermediate_size", "hidden_act", "layer_norm_eps")}
    vm = transformers.CLIPVisionModelWithProjection(transformers.CLIPVisionConfig(
        image_size=v["image_size"], patch_size=v["patch_size"], projection_dim=cfg["projection_dim"], **keep(v))).eval()
    tm = transformers.CLIPTextModelWithProjection(transformers.CLIPTextConfig(
        vocab_size=t["vocab_size"], max_position_embeddings=t["max_position_embeddings"], projection_dim=cfg["projection_dim"],
        bos_token_id=t["bos_token_id"], eos_token_id=t["eos_token_id"], pad_token_id=t["pad_token_id"], **keep(t))).eval()
    for m, prefixes in ((vm, ("vision_model.", "visual_projection.")), (tm, ("text_model.", "text_projection."))):
        res = m.load_state_dict({k: x for k, x in sd.items() if k.startswith(prefixes)}, strict=False)
        assert not res.unexpected_keys and all(k.endswith("position_ids") for k in res.missing_keys), res
    px = torch.randn(3, 3, v["image_size"], v["image_size"], generator=torch.Generator().manual_seed(1))
    ids = _ids(5)
    with torch.no_grad():
        want_v, want_t = vm(pixel_values=px).image_embeds, tm(input_ids=ids).text_embeds
    got_v, got_t = LBR.image_forward(sd, cfg, px), LBR.text_forward(sd, cfg, ids)
    ev, et = float((got_v - want_v).abs().max()), float((got_t - want_t).abs().max())
    print(f"LANGUAGEBIND_REF act={act} vision={ev:.2e} text={et:.2e}")
    assert ev <= TOL and et <= TOL, (ev, et)


@pytest.mark.parametrize("B,T,N,heads", [(1, 1, 1, 2), (2, 3, 5, 2), (1, 8, 7, 2), (3, 16, 2, 1)])
def test_strided_temporal_attention_is_the_rearranged_one(B, T, N, heads):
    g = torch.Generator().manual_seed(B * 100 + T * 10 + N)
    qkv = torch.randn(B * T * N, 3 * heads * 64, generator=g).to(torch.bfloat16)
    a, aa = LBR.temporal_attention_rearranged(qkv, B, T, N, heads)
    b, ba = LBR.temporal_attention_strided(qkv, B, T, N, heads)
    assert a.dtype == torch.float64 and float((a - b).abs().max()) <= 1e-14 and float((aa - ba).abs().max()) <= 1e-14


def test_temporal_sub_block_is_the_explicit_rearrange_form():
    """the layer with `add_time_attn` = the CLIP block applied to x + (temporal attention of LN(x + temb) over the frames), written out with
    strided indexing per (clip, token) in float64"""
    T, b = 3, 2
    cfg = LBR.config(LBR.SMALL, T=T, add_time_attn=True)
    sd = LBR.synthetic_state_dict(cfg, seed=5)
    c = cfg["vision_config"]
    W, N = c["hidden_size"], 5
    p = "vision_model.encoder.layers.0."
    dt = torch.float64
    x = torch.randn(b * T, N, W, dtype=dt, generator=torch.Generator().manual_seed(2))
    got = LBR.encoder_layer(x, sd, p, c, dt, T=T, temporal=True)
    y = x.clone().reshape(b, T, N, W)
    y = y + sd[p + "temporal_embedding"].to(dt)[0][None, :, None, :]
    upd = torch.zeros_like(y)
    for bi in range(b):
        for n in range(N):
            seq = LBR._ln(y[bi, :, n, :][None], sd, p + "temporal_layer_norm1", c["layer_norm_eps"], dt)
            upd[bi, :, n, :] = LBR.attention(seq, sd, p + "temporal_attn.", c["num_attention_heads"], dt)[0]
    want = LBR.encoder_layer((y + upd).reshape(b * T, N, W), sd, p, c, dt, T=T, temporal=False)
    assert float((got - want).abs().max()) <= 1e-12


def test_frame_order_moves_the_restatement():
    """temporal embeddings of ordinary size make the clip embedding depend on the frame order (what tests/test_languagebind_gpu.py asks of the
    tower); without them and without temporal attention it would be the mean of per-frame embeddings"""
    cfg = LBR.config(LBR.SMALL, T=8)
    sd = LBR.synthetic_state_dict(cfg, seed=0)
    clip = LBR.make_clip(1, 8, cfg["vision_config"]["image_size"])
    a = LBR.embed(LBR.video_forward(sd, cfg, clip), sd, "video", True)
    r = LBR.embed(LBR.video_forward(sd, cfg, clip.flip(2)), sd, "video", True)
    assert float(1 - (a * r).sum()) > 1e-3      # (the bf16 tower bound: the GPU test asks the tower to move by more than its own noise)

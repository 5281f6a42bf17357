"""Reference and rounding model of the two LanguageBind towers of engine/languagebind.py — LanguageBindVideoTower and LanguageBindAudioTower — for
tests/test_languagebind_tower_ref_host.py and tests/test_languagebind_passes_gpu.py.  A plain helper module: nothing here calls the library, and
everything runs on the device of its input.  The CLIP blocks are tests/encoder_ref.py's (pre-LN, fp32 stream), the front end is the one of
tests/tower_ref.py's image tower; what this module adds is the temporal sub-block in front of every block, the per-layer orchestration, the
rectangular grid of the audio part and the two tails.

    exact(ops, clip) / audio_exact(ops, px)                       round nothing -> Pass
    model(ops, clip, mut=, hist=, rounds=) / audio_model(...)     the same code, rounding where the towers store bf16 / fp32
Pass.x0 is the float64 token stream [(b t) n, W] behind the front end, Pass.temporal[l] / Pass.blocks[l] the stream after layer l's temporal sub-block /
after its CLIP block, Pass.cls_ln the class rows after post_layernorm [(b t), W], Pass.proj the per-frame projections [(b t), D], Pass.pooled[0 / 1] the
rows of a clip without / with L2.  The audio Pass has no temporal streams and its pooled rows are the projections.

Operands (ops / audio_ops) are what the towers' loader stores: the patch weight, the blocks' matrices (encoder_ref.blocks_from_sd on
hf_clip.clip_state_dict's names), the temporal q | k | v and out_proj matrices (engine.languagebind.temporal_weights) and visual_projection rounded to
bf16; class token, positions, every bias and LayerNorm weight and the temporal embeddings in fp32.  `rounded=False` keeps the checkpoint's fp32 matrices:
the form in which `exact` is pinned to the restatements of tests/languagebind_ref.py and tests/audio_ref.py.

Where `model` rounds — written down from engine/languagebind.py (_forward of either tower), engine/vit_tokens.py (_patchify_f32, _tokens), csrc/temporal.hip
(temporal_embed_ln_kernel, temporal_attention_kernel, patchify_clip_kernel) and csrc/towers.hip (mq_vit_assemble, the pre-LN block on residual_stream = 2):
    front end       pixel = bf16(fp32 pixel), once (mq_patchify_clip / mq_patchify_rect; the zero padding to Kp multiplies zero columns and is left out)
                    patch = fp32(pixel-row @ bf16(conv)^T)        x = fp32(LN_pre(fp32(class | patch + pos)))                    (mq_vit_assemble)
    temporal        x = fp32(x + temb[t]) — T == 1: no add at all, the stream keeps its bits (mq_temporal_embed_ln hands the kernel no table)
                    xn = bf16(LN_t x)      qkv = bf16(xn @ Wqkv^T + b)      probabilities fp32, NEVER rounded to bf16 (there is no MFMA operand to feed)
                    att = bf16(P V / l)    x = fp32(x + att @ Wo^T + b)     (MQ_EPI_BIAS | MQ_EPI_RESIDUAL | MQ_EPI_OUT_F32, in place on the stream)
    CLIP block      encoder_ref.model under PRE_F32, one block per call (video) or all blocks in one call (audio): residual_stream = 2 forces the fp32
                    stream, nothing is folded; GELU or QuickGELU per vision_config.hidden_act
    tail            cls_ln = bf16(LN_post(class rows))      proj = fp32(cls_ln @ bf16(visual_projection)^T)
                    video: pooled = fp32(mean over the T frames of proj) (mq_avg_tokens)       audio: pooled = proj
                    L2: fp32(pooled / |pooled|)
hist = 1 is a second rounding history of the same stores: every GEMM (patch, temporal q | k | v and out_proj, the blocks', the projection) sums fp32
partial products of 64-wide k chunks in reverse order (encoder_ref._mm, Form.hist).

`mut` is ONE deliberate defect of the orchestration (MUTANTS; APPLIES says at which shapes a defect exists at all).
"""
import math
from dataclasses import dataclass, field, replace
from typing import Dict, List, Optional

import torch

from tests import audio_ref as AR
from tests import encoder_ref as E
from tests import languagebind_ref as LBR
from tests.encoder_ref import ZeroYardstick, row_ratio      # noqa: F401

Tensor = torch.Tensor
F64 = torch.float64

MUTANTS = {
    # video
    "drop_out_bias_last": "the last layer's temporal out_proj runs without its bias",
    "ln_before_add": "the temporal LayerNorm reads the stream from before the embedding add (the stream itself still takes the add)",
    "temb_roll": "the last layer's temporal embedding rolled by one frame: frame t takes temb[t - 1]",
    "temb_layer0_in_1": "layer 1 adds layer 0's temporal embedding",
    "temb_at_T1": "the temporal embedding is added for a single frame as well",
    "regroup_bt_n": "temporal attention over the N tokens of a frame ((b t) n) instead of over the T frames of a token ((b n) t)",
    "eps_x10": "eps times ten in the temporal LayerNorm",
    "stale_xn_row": "row 0 of the temporal LayerNorm's output keeps layer 0's value in layer 1",
    "post_ln_after_mean": "post_layernorm applied to the frame mean of the class rows instead of to every class row",
    "mean_over_N": "the frame mean walks N rows per clip instead of T: clip i averages the N projection rows from row i N on (wrapped at the end)",
    # audio
    "pos_transposed": "positions read for the transposed grid: patch (py, px) takes the row of (px, py) in a grid_w x grid_h table",
}
AUDIO_MUTANTS = ("pos_transposed",)
# defects the ratio bar cannot see on any asserted view (tests/test_languagebind_tower_ref_host.py measures every entry of MUTANTS): behind pre_layrnorm
# and the O(1) temporal embeddings every stream row has a variance of order one, so eps = 1e-4 instead of 1e-5 moves rstd by about 5e-5 of itself — a
# fortieth of the half ulp (2 ** -9) the bf16 store of the same LayerNorm's output carries.  Measured 1.3 .. 1.9 against a second history's 1.0 .. 1.6.
INVISIBLE = ("eps_x10",)


def applies(mut: str, T: int, layers: int = 2) -> bool:
    """whether the defect exists at this shape: the embedding defects need the add (T > 1) — the single-frame one its absence —, the frame-mean ones
    more than one frame, the cross-layer ones a second layer"""
    if mut == "temb_at_T1":
        return T == 1
    if mut in ("ln_before_add", "temb_roll", "temb_layer0_in_1", "post_ln_after_mean"):
        return T > 1 and (layers > 1 or mut != "temb_layer0_in_1")
    if mut == "stale_xn_row":
        return layers > 1
    return True


@dataclass
class Pass:
    x0: Tensor
    temporal: List[Tensor]
    blocks: List[Tensor]
    cls_ln: Tensor
    proj: Tensor
    pooled: Dict[int, Tensor]


def views(p: Pass) -> Dict[str, Tensor]:
    """the views tests/test_languagebind_passes_gpu.py asserts, by name.  The audio tower runs all its blocks in one call: only the stream behind the last
    one can be seen from outside"""
    out = {"x0": p.x0}
    for l, x in enumerate(p.blocks):
        if p.temporal:
            out[f"temporal{l}"] = p.temporal[l]
        if p.temporal or l == len(p.blocks) - 1:
            out[f"block{l}"] = x
    out["cls_ln"] = p.cls_ln
    out["pooled/l2=0"], out["pooled/l2=1"] = p.pooled[0], p.pooled[1]
    return out


# ---- operands ----------------------------------------------------------------------------------------------------------------------------------------
def _arch(cfg):
    from marqo_amd.engine import archs
    return archs.languagebind_arch_from_hf_config(cfg)


def ops(cfg: dict, sd: Dict[str, Tensor], rounded: bool = True, device="cpu") -> dict:
    """the vision side of a video or audio part as its tower stores it, float64 on `device`"""
    from marqo_amd.engine.hf_clip import clip_state_dict
    from marqo_amd.engine.languagebind import temporal_weights
    a = _arch(cfg)
    v, W, P = "vision_model.", a.width, a.patch_size
    w = E._w16 if rounded else E._f32
    blocks = E.blocks_from_sd("clip", clip_state_dict(sd, v, a.layers), "transformer.", a.layers)
    if not rounded:
        for b in blocks:
            for n in ("qkv", "out", "fc1", "fc2"):
                b[n + "_w"] = b[n + "_w32"]
    o = dict(arch=a, patch_w=w(sd[v + "embeddings.patch_embedding.weight"].reshape(W, 3 * P * P)), cls=E._f32(sd[v + "embeddings.class_embedding"]),
             pos=E._f32(sd[v + "embeddings.position_embedding.weight"]), pre_g=E._f32(sd[v + "pre_layrnorm.weight"]), pre_b=E._f32(sd[v + "pre_layrnorm.bias"]),
             post_g=E._f32(sd[v + "post_layernorm.weight"]), post_b=E._f32(sd[v + "post_layernorm.bias"]), proj_w=w(sd["visual_projection.weight"]),
             blocks=E.blocks_to(blocks, device), temporal=[])
    assert o["pos"].shape[0] == a.tokens
    if a.add_time_attn:
        for i in range(a.layers):
            t = temporal_weights(sd, a, i)
            o["temporal"].append({k: (w(t[k]) if k in ("qkv_w", "out_w") else E._f32(t[k])).to(device) for k in t})
    return {k: (t.to(device) if isinstance(t, Tensor) else t) for k, t in o.items()}


def _cfg(a) -> E.Cfg:
    return E.Cfg(W=a.width, heads=a.heads, F=a.mlp_dim, layers=a.layers, act="quick" if a.quick_gelu else "gelu", eps=a.ln_eps)


def _form(rounds: bool, hist: int) -> Optional[E.Form]:
    return replace(E.PRE_F32, hist=hist if rounds else 0, rounds=rounds)


# ---- the pieces ----------------------------------------------------------------------------------------------------------------------------------------
def _front(o, R, pics: Tensor, gh: int, gw: int, hist: int, pos_transposed: bool = False) -> Tensor:
    """pics float64 [m, 3, H, Wd] -> the stream [m (gh gw + 1), W]: im2col rows in (py, px) order, columns (c, ky, kx)"""
    a = o["arch"]
    W, P, m = a.width, a.patch_size, pics.shape[0]
    px = R.b(pics)[:, :, :gh * P, :gw * P]
    rows = px.reshape(m, 3, gh, P, gw, P).permute(0, 2, 4, 1, 3, 5).reshape(m * gh * gw, 3 * P * P)
    patch = R.f(E._mm(rows, o["patch_w"], hist)).reshape(m, gh * gw, W)
    pos = o["pos"]
    if pos_transposed:
        py, qx = torch.arange(gh, device=pos.device)[:, None], torch.arange(gw, device=pos.device)[None, :]
        pos = torch.cat([pos[:1], pos[1 + (qx * gh + py).reshape(-1)]], 0)
    tok = torch.cat([o["cls"].expand(m, 1, W), patch], 1)
    return R.f(E._ln(R.f(tok + pos), o["pre_g"], o["pre_b"], a.ln_eps)).reshape(m * (gh * gw + 1), W)


def _temporal_attention(qkv: Tensor, b: int, T: int, N: int, H: int, regroup: bool = False) -> Tensor:
    """softmax(q k^T / sqrt(hd)) v over the T rows (b T + t) N + n of every (b, n, head); the probabilities are not rounded.  `regroup`: over the N
    rows of every (b, t, head) instead"""
    W = qkv.shape[1] // 3
    hd = W // H
    if regroup:
        x = qkv.reshape(b * T, N, 3, H, hd).permute(0, 2, 3, 1, 4)            # f 3 h n d
        back = lambda y: y.permute(0, 2, 1, 3).reshape(b * T * N, W)          # f h n d -> (f n) (h d)
    else:
        x = qkv.reshape(b, T, N, 3, H, hd).permute(0, 2, 3, 4, 1, 5)          # b n 3 h t d
        back = lambda y: y.permute(0, 3, 1, 2, 4).reshape(b * T * N, W)       # b n h t d -> (b t n) (h d)
    q, k, v = x.unbind(-4)
    return back(torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(hd), dim=-1) @ v)


def _temporal(o, R, x: Tensor, l: int, b: int, T: int, N: int, hist: int, mut: Optional[str], stale: dict) -> Tensor:
    a, layers = o["arch"], o["arch"].layers
    t = o["temporal"][l]
    last = l == layers - 1
    before = x
    if T != 1 or mut == "temb_at_T1":
        temb = t["temb"]
        if mut == "temb_roll" and last:
            temb = torch.roll(temb, 1, 0)
        if mut == "temb_layer0_in_1" and l == 1:
            temb = o["temporal"][0]["temb"]
        frame = (torch.arange(x.shape[0], device=x.device) // N) % T
        x = R.f(x + temb[frame])
    eps = a.ln_eps * (10.0 if mut == "eps_x10" else 1.0)
    xn = R.b(E._ln(before if mut == "ln_before_add" else x, t["ln_g"], t["ln_b"], eps))
    if mut == "stale_xn_row":
        if l == 0:
            stale["xn0"] = xn[0].clone()
        elif l == 1:
            xn = xn.clone()
            xn[0] = stale["xn0"]
    qkv = R.b(E._linear(xn, t["qkv_w"], t["qkv_b"], hist))
    att = R.b(_temporal_attention(qkv, b, T, N, a.heads, regroup=mut == "regroup_bt_n"))
    out_b = None if (mut == "drop_out_bias_last" and last) else t["out_b"]
    return R.f(x + E._linear(att, t["out_w"], out_b, hist))


def _l2(R, rows: Tensor) -> Tensor:
    return R.f(rows / rows.norm(dim=-1, keepdim=True))


# ---- the video tower -------------------------------------------------------------------------------------------------------------------------------
def _video(o, clip: Tensor, rounds: bool, mut: Optional[str], hist: int) -> Pass:
    assert mut is None or mut in MUTANTS
    a = o["arch"]
    form = _form(rounds, hist)
    R = E._Round(form)
    hist = form.hist
    b, ch, T, S, _ = clip.shape
    assert T == a.num_frames and ch == 3 and S == a.image_size
    W, N, D, G = a.width, a.tokens, a.out_dim, a.grid
    frames = b * T
    pics = clip.to(F64).permute(0, 2, 1, 3, 4).reshape(frames, 3, S, S)          # b c t h w -> (b t) c h w
    x0 = _front(o, R, pics, G, G, hist)
    cfg, lens = _cfg(a), [N] * frames
    x, temporal, blocks, stale = x0, [], [], {}
    for l in range(a.layers):
        x = _temporal(o, R, x, l, b, T, N, hist, mut, stale)
        temporal.append(x)
        x = E._run(cfg, [o["blocks"][l]], x, lens, form, 1)[-1]                  # one block per mq_encoder_forward call
        blocks.append(x)
    cls = x.reshape(frames, N, W)[:, 0]
    if mut == "post_ln_after_mean":
        cls_ln = R.b(E._ln(cls.reshape(b, T, W).mean(1), o["post_g"], o["post_b"], a.ln_eps))
        proj = R.f(E._mm(cls_ln, o["proj_w"], hist))
        pooled = proj
    else:
        cls_ln = R.b(E._ln(cls, o["post_g"], o["post_b"], a.ln_eps))
        proj = R.f(E._mm(cls_ln, o["proj_w"], hist))
        if mut == "mean_over_N":
            idx = (torch.arange(b, device=proj.device)[:, None] * N + torch.arange(N, device=proj.device)[None, :]) % frames
            pooled = R.f(proj[idx].mean(1))
        else:
            pooled = R.f(proj.reshape(b, T, D).mean(1))
    return Pass(x0, temporal, blocks, cls_ln, proj, {0: pooled, 1: _l2(R, pooled)})


def exact(o, clip: Tensor) -> Pass:
    return _video(o, clip, False, None, 0)


def model(o, clip: Tensor, mut: Optional[str] = None, hist: int = 0, rounds: bool = True) -> Pass:
    return _video(o, clip, rounds, mut, hist)


# ---- the audio tower -------------------------------------------------------------------------------------------------------------------------------
def _audio(o, px: Tensor, rounds: bool, mut: Optional[str], hist: int) -> Pass:
    assert mut is None or mut in AUDIO_MUTANTS
    a = o["arch"]
    form = _form(rounds, hist)
    R = E._Round(form)
    hist = form.hist
    b = px.shape[0]
    assert tuple(px.shape[1:]) == (3, a.num_mel_bins, a.target_length)
    W, N = a.width, a.tokens
    x0 = _front(o, R, px.to(F64), a.grid_h, a.grid_w, hist, pos_transposed=mut == "pos_transposed")
    blocks = E._run(_cfg(a), o["blocks"], x0, [N] * b, form, a.layers)          # all blocks in one mq_encoder_forward call
    cls_ln = R.b(E._ln(blocks[-1].reshape(b, N, W)[:, 0], o["post_g"], o["post_b"], a.ln_eps))
    proj = R.f(E._mm(cls_ln, o["proj_w"], hist))
    return Pass(x0, [], blocks, cls_ln, proj, {0: proj, 1: _l2(R, proj)})


def audio_exact(o, px: Tensor) -> Pass:
    return _audio(o, px, False, None, 0)


def audio_model(o, px: Tensor, mut: Optional[str] = None, hist: int = 0, rounds: bool = True) -> Pass:
    return _audio(o, px, rounds, mut, hist)


# ---- the cases both test files run -----------------------------------------------------------------------------------------------------------------
P14 = dict(LBR.SMALL, S=28, P=14)                 # 5 tokens as SMALL; K = 3 * 14 * 14 = 588 < Kp = 640: the im2col rows end in zero padding
AUDIO_SQUARE = dict(AR.SMALL, bins=16, L=16)      # a 2 x 2 grid at patch 8: the square control of the 2 x 5 grid


@dataclass
class VCase:
    id: str
    T: int
    B: int
    shape: dict = field(default_factory=lambda: LBR.SMALL)
    act: str = "gelu"
    split: int = 0          # > 0: max_items_per_call of the test's tower instance (the batch runs in several calls)

    def cfg(self) -> dict:
        return LBR.config(self.shape, T=self.T, hidden_act=self.act)

    def sd(self) -> Dict[str, Tensor]:
        return LBR.synthetic_state_dict(self.cfg(), seed=self.T)

    def clip(self) -> Tensor:
        return LBR.make_clip(self.B, self.T, self.shape["S"], seed=self.B)


@dataclass
class ACase:
    id: str
    B: int
    shape: dict = field(default_factory=lambda: AR.SMALL)

    def cfg(self) -> dict:
        return AR.config(self.shape)

    def sd(self) -> Dict[str, Tensor]:
        return AR.synthetic_state_dict(self.cfg(), seed=3)

    def px(self) -> Tensor:
        return AR.make_spectrograms(self.B, self.shape["bins"], self.shape["L"], seed=1)


def video_cases(max_frames: int = 16) -> List[VCase]:
    """the smallest shapes at which each thing can go wrong; `max_frames`: engine.languagebind.MAX_FRAMES"""
    C = VCase
    return [C("T1-B2[no-add-branch]", 1, 2), C("T2-B1", 2, 1), C("T3-B3[clips-interleave]", 3, 3), C("T8-B1", 8, 1),
            C(f"T{max_frames}-B2[MAX_FRAMES]", max_frames, 2), C("T3-B2-quick_gelu", 3, 2, act="quick_gelu"), C("T2-B2-P14[Kp>3PP]", 2, 2, shape=P14),
            C("T3-B3-split2[max_items_per_call=2]", 3, 3, split=2)]


def audio_cases() -> List[ACase]:
    C = ACase
    return [C("grid2x5-b1", 1), C("grid2x5-b3", 3), C("grid2x2-b2[square-control]", 2, shape=AUDIO_SQUARE)]

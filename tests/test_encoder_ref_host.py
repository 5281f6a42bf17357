"""tests/encoder_ref.py on the CPU: what tests/test_encoder_forms_gpu.py rests on.

1. The exact reference is the oracle's arithmetic: on tiny pre-LN CLIP, post-LN BERT and EVA02 encoders `exact` agrees with oracle/towers.py (fp32) to
   fp32 round-off — every row for CLIP and BERT; for EVA the oracle only hands out the class-token rows behind its final LayerNorm.
2. The yardstick is usable on every input the GPU file runs: the model's distance from `exact` is strictly positive in every row, the model measures
   1.0 against itself, and two models with rounding histories of the same size (folded / un-folded LayerNorms on the bf16 stream, the gated product in
   or behind the GEMM) stay within MARGIN of each other's yardstick: the bar admits every correct form.  (An fp32-stream and a bf16-stream form do NOT
   share a yardstick — the bf16 stream rounds x itself, 2^-9 of a channel of size 6 against 2^-9 of a block's output — which is why every GPU case is
   measured against the model of its own form; the ratio between the two is printed for the record.)
3. The bar sees the defects this suite is there for: each is injected into `model` and leaves the bar by at least 10 x, or breaks the bit comparison.
4. The e4m3 forms (tests/test_encoder_fp8_forms_gpu.py): the six static scales of every case lie a factor of two apart; with every store switched off a form's
   dataflow IS the exact reference on the dequantised weights, and the e4m3 stores are the larger part of its yardstick; the yardstick is positive in every
   row; a second rounding history of the same form (fp32 GEMM sums over reversed 64-wide k chunks) stays within MARGIN of the first on every case — the
   condition under which the bar is fair to a correct kernel; and each hand-off defect of the fp8 orchestration leaves the bar on every case it applies to."""
import dataclasses
import math

import pytest
import torch

from oracle import towers as O
from tests import encoder_ref as E
from tests.test_patch_attn_gpu import MARGIN

SMALL_M = 80        # the default of the small_m knob (csrc/knobs.hip); the GPU file reads the running value from the getter


def _round_matrices(sd):
    return {k: (v.to(torch.bfloat16).float() if v.dim() >= 2 else v.float()) for k, v in sd.items()}


def _pin(name, got, want):
    scale = max(1.0, float(want.abs().max()))
    err = float((got - want.double()).abs().max())
    print(f"ORACLE_PIN {name}: max |exact - oracle| = {err:.3e} (scale {scale:.2f}, bound {2e-6 * scale:.3e})")
    assert err <= 2e-6 * scale      # the oracle is fp32: 6e-8 per operation, a few dozen dependent operations over two blocks


def test_exact_is_the_oracle_clip_pre_ln():
    W, H, F, layers, B, T = 128, 2, 256, 2, 3, 12
    sd = _round_matrices(E.make_sd("clip", layers, W, F, 1))
    x0 = E.make_input(B * T, W, 2, False)
    for causal, quick in ((False, False), (True, True)):
        cfg = E.Cfg(W=W, heads=H, F=F, layers=layers, act="quick" if quick else "gelu", mask=1 if causal else 0)
        mask = torch.full((T, T), float("-inf")).triu(1) if causal else None
        want = O._clip_resblocks(x0.reshape(B, T, W), sd, "t.", layers, H, quick, cfg.eps, mask).reshape(B * T, W)
        got = E.exact(cfg, E.blocks_from_sd("clip", sd, "t.", layers), x0, [T] * B)[-1]
        _pin(f"clip causal={causal} quick={quick}", got, want)


def test_exact_is_the_oracle_bert_post_ln():
    ocfg = O.BertConfig(vocab=50, max_pos=16, width=128, layers=2, heads=2, mlp_dim=256)
    sd = _round_matrices(O.synthetic_bert_state_dict(ocfg, seed=3))
    lens = [11, 7]
    ids = torch.randint(0, 50, (2, 11), generator=torch.Generator().manual_seed(4))
    am = torch.tensor([[1] * ln + [0] * (11 - ln) for ln in lens])
    valid = am.bool().reshape(-1)
    x0 = O.bert_forward(sd, dataclasses.replace(ocfg, layers=0), ids, am).reshape(-1, 128)[valid]
    want = O.bert_forward(sd, ocfg, ids, am).reshape(-1, 128)[valid]
    cfg = E.Cfg(W=128, heads=2, F=256, layers=2, post_ln=True, eps=ocfg.ln_eps)
    got = E.exact(cfg, E.blocks_from_sd("bert", sd, "", 2), x0, lens)[-1]
    _pin("bert", got, want)


def test_exact_is_the_oracle_eva():
    ocfg = O.EvaVitConfig(image_size=32, patch_size=8, width=128, layers=2, heads=2, mlp_dim=256, out_dim=128)
    sd = O.synthetic_eva_state_dict(ocfg, seed=5)
    t = "visual.trunk."
    sd[t + "head.weight"], sd[t + "head.bias"] = torch.eye(128), torch.zeros(128)      # the oracle's output becomes norm(x)[:, 0]
    sd = _round_matrices(sd)
    B, T = 3, ocfg.tokens
    px = torch.randn(B, 3, 32, 32, generator=torch.Generator().manual_seed(6))
    x0 = torch.nn.functional.conv2d(px, sd[t + "patch_embed.proj.weight"], sd[t + "patch_embed.proj.bias"], stride=8).reshape(B, 128, -1).permute(0, 2, 1)
    x0 = (torch.cat([sd[t + "cls_token"].expand(B, 1, 128), x0], 1) + sd[t + "pos_embed"]).reshape(B * T, 128)
    want = O.eva_vit_forward(sd, ocfg, px, normalize=False)
    sin, cos = O.eva_rope(ocfg)
    cfg = E.Cfg(W=128, heads=2, F=256, layers=2, act="silu", glu=2, eps=ocfg.ln_eps, rope_table=torch.stack([cos, sin], 1), rope_prefix=1)
    x = E.exact(cfg, E.blocks_from_sd("eva", sd, t, 2), x0, [T] * B)[-1]
    got = E._ln(x[::T], sd[t + "norm.weight"].double(), sd[t + "norm.bias"].double(), ocfg.ln_eps)
    _pin("eva (class-token rows behind the final LayerNorm)", got, want)


_ref_cache = {}


def _reference(case, layers=None):
    key = (case.id, layers)
    if key not in _ref_cache:
        _ref_cache[key] = E.reference(case, "cpu", layers)
    return _ref_cache[key]


@pytest.mark.parametrize("case", E.cases(SMALL_M), ids=lambda c: c.id)
def test_yardstick_is_positive_on_every_gpu_input(case):
    for layers in sorted({1, case.layers}):
        ex, mo = _reference(case, layers)
        y = (mo - ex).norm(dim=1)
        r = E.row_ratio(mo, ex, mo)         # raises ZeroYardstick if a row of the model is exact
        print(f"YARDSTICK case={case.id} layers={layers}: row error of the model min {float(y.min()):.3e} median {float(y.median()):.3e} max {float(y.max()):.3e}")
        assert float(y.min()) > 0 and r["ratio"] == 1.0 and torch.isfinite(mo).all()


def test_zero_yardstick_is_an_error_not_a_division():
    ex = torch.randn(4, 8, dtype=torch.float64)
    mo = ex + 1e-3
    mo[2] = ex[2]
    with pytest.raises(E.ZeroYardstick):
        E.row_ratio(ex, ex, mo)


def _by_id(prefix):
    return next(c for c in E.cases(SMALL_M) if c.id.startswith(prefix))


@pytest.mark.parametrize("prefix,forms", [
    ("pre_ln-bf16-gelu-packed217", (E.PRE_BF16, E.PRE_BF16_FOLD)),
    ("post_ln-f32-gelu-packed217", (E.POST_F32, E.POST_SMALL)),
])
def test_forms_of_one_rounding_size_stay_within_margin_of_each_other(prefix, forms):
    case = _by_id(prefix)
    cfg, blocks, x0 = case.cfg(), E.blocks_from_sd(case.kind, case.sd(), "t.", case.layers), case.x0()
    ex = E.exact(cfg, blocks, x0, case.lens)[-1]
    mo = [E.model(cfg, blocks, x0, case.lens, f)[-1] for f in forms]
    for i, a in enumerate(forms):
        for j, b in enumerate(forms):
            if i != j:
                r = E.row_ratio(mo[i], ex, mo[j])
                print(f"FORM_PAIR {a.name} against the yardstick of {b.name}: worst row ratio {r['ratio']:.3f} (row {r['row']})")
                assert r["ratio"] <= MARGIN


def test_streams_of_different_width_do_not_share_a_yardstick():
    case = _by_id("pre_ln-f32-gelu-packed217")
    cfg, blocks, x0 = case.cfg(), E.blocks_from_sd(case.kind, case.sd(), "t.", case.layers), case.x0()
    ex = E.exact(cfg, blocks, x0, case.lens)[-1]
    f32, b16 = (E.model(cfg, blocks, x0, case.lens, f)[-1] for f in (E.PRE_F32, E.PRE_BF16))
    r = E.row_ratio(b16, ex, f32)
    print(f"FORM_PAIR pre_ln/bf16 against the yardstick of pre_ln/f32: worst row ratio {r['ratio']:.2f} — not one rounding size, not asserted against MARGIN")
    assert r["ratio"] > 1.0 and E.row_ratio(f32, ex, b16)["ratio"] < 1.0
    # the EVA forms behind the 24-unit outlier channel: the folded GEMM multiplies the raw channel by bf16(g W), the un-folded one the normalised channel
    # by bf16(W) — measured 4.3 between the two on the CPU, so they are not held to each other here; on the GPU each is held to its own model
    case = _by_id("eva-bf16-glu2-subln-fixed5x50[fold_ok")
    cfg, blocks, x0 = case.cfg(), E.blocks_from_sd(case.kind, case.sd(), "t.", case.layers), case.x0()
    ex = E.exact(cfg, blocks, x0, case.lens)[-1]
    a, b = (E.model(cfg, blocks, x0, case.lens, f)[-1] for f in (E.EVA_BF16_FOLD_EPI, E.Form("eva/bf16+glu_epi", stream="bf16", glu_epi=True)))
    print(f"FORM_PAIR eva folded / un-folded on the bf16 stream: {E.row_ratio(a, ex, b)['ratio']:.2f} and {E.row_ratio(b, ex, a)['ratio']:.2f} — not asserted")


# ---- mutations: each leaves the bar by >= 10 x ----------------------------------------------------------------------------------------------

MUTATIONS = [
    # (name, case id prefix, mutation)
    ("one row's residual is dropped", "pre_ln-bf16-gelu-packed217[grouped", dict(kind="drop_residual", row=100)),
    ("one row's residual is dropped (post-LN)", "post_ln-f32-gelu-packed217", dict(kind="drop_residual", row=100)),
    # (one row's stale statistics rescale that row's q, k and v: the row itself shows it where its own v carries its attention output — the one-row
    # sequence, the first row of a causal sequence — the other rows of a long sequence hold 1 / len of it)
    ("block 2 reads block 1's (mean, rstd) in one row", "pre_ln-bf16-quick-packed217[fold_ok,ln_fold=2", dict(kind="stale_stats", row=0)),
    ("block 2 reads block 1's (mean, rstd) in one row (causal, first row of a sequence)", "pre_ln-bf16-gelu-causal-packed217[fold_ok,ln_fold=1",
     dict(kind="stale_stats", row=18)),
    ("block 2 reads block 1's (mean, rstd) in one row (un-folded)", "pre_ln-f32-gelu-packed217", dict(kind="stale_stats", row=0)),
    ("the fc1 output of the previous block is left in one row of qf", "pre_ln-f32-gelu-packed217", dict(kind="stale_fc1", row=216)),
    ("the fc1 output of the previous block is left in one row of qf (post-LN bf16 stream)", "post_ln_bf16-gelu-packed217", dict(kind="stale_fc1", row=0)),
    ("a sequence boundary is off by one row", "pre_ln-f32-gelu-packed217", dict(kind="seq_boundary")),
    ("a sequence boundary is off by one row (causal, fixed length)", "pre_ln-f32-quick-causal-fixed5x50", dict(kind="seq_boundary")),
    ("the gated hidden is read with stride F instead of 2F", "post_ln-f32-rope-glu1-bias-packed217", dict(kind="glu_stride")),
    ("the gated hidden is read with stride F instead of 2F (EVA)", "eva-f32-glu1-rope1-nosubln", dict(kind="glu_stride")),
    ("the LN2 output of a selected row is taken from its neighbour", "rows-pre_ln-f32-packed217", dict(kind="ln2_neighbour", row=4)),
    ("the LN2 output of a selected row is taken from its neighbour (post-LN)", "rows-post_ln-f32-packed217", dict(kind="ln2_neighbour", row=4)),
]


@pytest.mark.parametrize("name,prefix,mut", MUTATIONS, ids=[m[0] for m in MUTATIONS])
def test_mutation_leaves_the_bar(name, prefix, mut):
    case = _by_id(prefix)
    ex, mo = _reference(case)
    cfg, blocks, x0 = case.cfg(), E.blocks_from_sd(case.kind, case.sd(), "t.", case.layers), case.x0()
    sel = case.sel_rows()
    sel_t = torch.tensor(sel) if sel is not None else None
    bad = E.model(cfg, blocks, x0, case.lens, case.form, None, sel_t, mut)[-1]
    rows = sel_t if sel is not None else None          # a row selection is measured on the selected rows, as the GPU test does
    r = E.row_ratio(bad, ex, mo, rows)
    print(f"MUTATION {name} [{case.form.name}]: worst row ratio {r['ratio']:.1f} = {r['ratio'] / MARGIN:.1f} x the bar (row {r['row']}, l2 {r['l2']:.1f}, linf {r['linf']:.1f})")
    assert r["ratio"] >= 10.0 * MARGIN
    # ... and in one row only where the defect is one row's: the yardstick does not smear it
    if "row" in mut and mut["kind"] != "ln2_neighbour":
        others = torch.tensor([i for i in range(case.rows) if i != mut["row"]])
        if mut["kind"] in ("drop_residual",) and case.layers - 1 > 0:
            assert E.row_ratio(bad, ex, mo, others)["ratio"] <= MARGIN      # the last block's defect stays in its row


@pytest.mark.parametrize("prefix", ["rows-pre_ln-f32-packed217", "rows-post_ln_bf16-packed217"])
def test_mutation_scatter_over_the_other_rows_breaks_the_bit_comparison(prefix):
    case = _by_id(prefix)
    cfg, blocks, x0 = case.cfg(), E.blocks_from_sd(case.kind, case.sd(), "t.", case.layers), case.x0()
    sel = torch.tensor(case.sel_rows())
    keep = torch.ones(case.rows, dtype=torch.bool)
    keep[sel] = False
    before = E.model(cfg, blocks, x0, case.lens, case.form, case.layers - 1)[-1]
    good = E.model(cfg, blocks, x0, case.lens, case.form, None, sel)[-1]
    bad = E.model(cfg, blocks, x0, case.lens, case.form, None, sel, dict(kind="scatter_all"))[-1]
    if not (case.post_ln and case.form.stream == "bf16"):     # (post-LN bf16 stream: the model's stream between blocks is the bf16 rows, a layers - 1 call ends in an fp32 LayerNorm)
        assert torch.equal(good[keep], before[keep])
    n_bad = int((bad[keep] != good[keep]).any(dim=1).sum())
    print(f"MUTATION the non-selected rows are overwritten by the scatter [{case.form.name}]: {n_bad} of {int(keep.sum())} other rows differ in bits")
    assert n_bad > 0 and not torch.equal(bad[keep], good[keep])


# ---- the e4m3 forms ---------------------------------------------------------------------------------------------------------------------------

F8 = E.f8_cases()
_f8_cache = {}


def _f8(case, layers=None, **form_changes):
    """(setup, exact stream, model stream of the case's form with `form_changes`) after `layers` blocks, as the GPU test measures that call"""
    n = case.layers if layers is None else layers
    key = (case.id, n)
    if key not in _f8_cache:
        s = E.f8_setup(case, "cpu", n)
        _f8_cache[key] = (s, E.exact(s["cfg"], s["blocks"], s["x0"], case.lens, n)[-1])
    s, ex = _f8_cache[key]
    return s, ex, _f8_model(case, s, n, **form_changes)


def _f8_sel(case, n):
    sel = case.sel_rows()
    return torch.tensor(sel) if (sel is not None and not case.post_ln and n == case.layers) else None


def _f8_model(case, s, n, mut=None, **form_changes):
    form = dataclasses.replace(s["form"], **form_changes)
    return E.model(s["cfg"], s["blocks"], s["x0"], case.lens, form, n, _f8_sel(case, n), mut)[-1]


@pytest.mark.parametrize("case", F8, ids=lambda c: c.id)
def test_f8_scales_lie_a_factor_of_two_apart(case):
    s = E.f8_setup(case)
    v = sorted(s["scales"].flatten().tolist())
    gaps = [b / a for a, b in zip(v, v[1:])]
    print(f"F8_SCALES case={case.id}: max|tensor| = {[round(x * 448 * case.scale_div, 2) for x in s['scales'].flatten().tolist()]}, smallest ratio of two scales {min(gaps):.2f}")
    assert len(v) == 2 * case.layers and min(v) > 0 and min(gaps) >= 2.0
    ex = {k: m for k, m in s["amax_exact"].items()}
    assert all(abs(float(s["scales"][l, k]) * case.scale_div * 448.0 - ex[(l, k)]) <= 1e-6 * ex[(l, k)] for l in range(case.layers) for k in (0, 1))


@pytest.mark.parametrize("case", F8, ids=lambda c: c.id)
def test_f8_rounding_switched_off_is_the_exact_reference(case):
    for n in (1, case.layers):
        s, ex, off = _f8(case, n, rounds=False, fold=False)
        if _f8_sel(case, n) is None:
            assert torch.equal(off, ex)
        else:
            sel = _f8_sel(case, n)
            assert torch.equal(off[sel], ex[sel])
        if n == case.layers:        # the e4m3 stores are what the yardstick of these forms is made of: without them the model lies closer to exact
            mo, no8 = _f8_model(case, s, n), _f8_model(case, s, n, e4m3=False)
            rows = _f8_sel(case, n)
            y, y0 = (mo - ex).norm(dim=1), (no8 - ex).norm(dim=1)
            if rows is not None:
                y, y0 = y[rows], y0[rows]
            print(f"F8_SHARE case={case.id}: median row error with / without the e4m3 stores {float(y.median()):.3e} / {float(y0.median()):.3e}")
            assert float(y0.median()) < float(y.median())


@pytest.mark.parametrize("case", F8, ids=lambda c: c.id)
def test_f8_yardstick_is_positive_on_every_gpu_input(case):
    for n in (1, case.layers):
        s, ex, mo = _f8(case, n)
        rows = _f8_sel(case, n)
        r = E.row_ratio(mo, ex, mo, rows)
        y = (mo - ex).norm(dim=1)
        y = y if rows is None else y[rows]
        print(f"YARDSTICK case={case.id} layers={n}: row error of the model min {float(y.min()):.3e} median {float(y.median()):.3e} max {float(y.max()):.3e}")
        assert float(y.min()) > 0 and r["ratio"] == 1.0 and torch.isfinite(mo).all()


@pytest.mark.parametrize("case", F8, ids=lambda c: c.id)
def test_f8_second_rounding_history_stays_within_margin(case):
    for n in (1, case.layers):
        s, ex, mo = _f8(case, n)
        m2 = _f8_model(case, s, n, hist=1)
        rows = _f8_sel(case, n)
        a, b = E.row_ratio(m2, ex, mo, rows), E.row_ratio(mo, ex, m2, rows)
        n_diff = int((m2 != mo).any(dim=1).sum())
        print(f"F8_HISTORY case={case.id} layers={n}: second history against the first {a['ratio']:.3f} (row {a['row']}), first against second {b['ratio']:.3f}; "
              f"{n_diff} rows differ")
        assert max(a["ratio"], b["ratio"]) <= MARGIN


_SAT = "[scales/4:saturating]"
_plain = lambda c: _SAT not in c.id                                          # noqa: E731
F8_MUTATIONS = [
    # (name, kind, the cases it applies to)
    ("s_attn and s_mlp swapped", "swap_scales", _plain),
    ("the scales of layer l - 1 used", "prev_layer_scales", _plain),
    ("row_scale of the neighbouring row", "row_scale_neighbour", _plain),
    ("row_scale of LN1 re-used for LN2", "row_scale_ln1_for_ln2", _plain),
    ("rowquant skipped at the post-LN transition", "skip_rowquant", lambda c: c.post_ln and c.form.first8 > 0),
    ("e4m3 stores truncated instead of rounded to nearest", "e4m3_truncate", _plain),
    ("no saturation", "no_saturation", lambda c: _SAT in c.id),
    ("the selected body gathers attention rows at 2 * Wa bytes", "gather_2wa", lambda c: c.sel is not None and not c.post_ln),
]
_F8_MUT_PAIRS = [(name, kind, c) for name, kind, ok in F8_MUTATIONS for c in F8 if ok(c)]


@pytest.mark.parametrize("name,kind,case", _F8_MUT_PAIRS, ids=[f"{k}-{c.id}" for _, k, c in _F8_MUT_PAIRS])
def test_f8_mutation_leaves_the_bar(name, kind, case):
    """in one of the two calls the GPU test measures: all blocks (the selected rows of a row selection), or the first block alone"""
    worst = []
    for n in (case.layers, 1):
        s, ex, mo = _f8(case, n)
        bad = _f8_model(case, s, n, mut=dict(kind=kind))
        worst.append(E.row_ratio(bad, ex, mo, _f8_sel(case, n))["ratio"])
    print(f"F8_MUTATION {name} [{case.form.name}] case={case.id}: worst row ratio {worst[0]:.1f} after all blocks, {worst[1]:.1f} after the first alone = "
          f"{max(worst) / MARGIN:.1f} x the bar")
    assert max(worst) > MARGIN


def test_f8_quantize_rows_is_the_kernels_rule():
    """the host stand-in for the engine's weight quantiser: scale = max|row| / 448 (1 for a zero row), codes within half an e4m3 step"""
    from tests.gemm_fp8_ref import decode
    w = (torch.randn(40, 128, generator=torch.Generator().manual_seed(3)) * torch.rand(40, 1, generator=torch.Generator().manual_seed(4))).to(torch.bfloat16)
    w[7] = 0
    codes, sc = E.quantize_rows(w.double())
    assert float(sc[7]) == 1.0 and torch.equal(sc[torch.arange(40) != 7], (w.float().abs().amax(1) / 448.0)[torch.arange(40) != 7])
    err = (decode(codes) * sc.double()[:, None] - w.double()).abs().amax(1)
    assert bool((err <= w.double().abs().amax(1) * 2.0 ** -4 / 1.75 + 1e-12).all())       # half a step of the top binade: 2^-4 of 256 / 448 of the maximum

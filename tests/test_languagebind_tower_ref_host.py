"""tests/languagebind_tower_ref.py on the host (no GPU): what its float64 passes are pinned to, and what the bar of tests/test_languagebind_passes_gpu.py can see.

1. `exact` on the checkpoint's own fp32 weights (ops(rounded=False)) gives the pooled rows of tests/languagebind_ref.py's video_forward and of
   tests/audio_ref.py's audio_forward in float64, on every case of the GPU file.  The two differ in evaluation order only (the restatement regroups
   `(b t) n d <-> (b n) t d` and projects the frame mean, `exact` walks the rows at their stride and averages the projections; torch's conv2d against
   an im2col product).  Measured max |a - b| / max |b| over the cases: video 3.7e-16 .. 1.0e-15, audio 5.4e-16 .. 1.1e-15; asserted PIN_RTOL = 1e-13,
   a hundred times that and nine orders of magnitude under the bf16 effects the passes measure.
2. `model` with every store switched off equals `exact` bit for bit, and with the stores on no row of any asserted view has a zero yardstick.  At T = 1
   the temporal embedding is no part of the pass: another table gives the same bits.
3. model(hist = 1) against model(hist = 0): every asserted view stays inside MARGIN (tests/test_patch_attn_gpu.py).  Printed as LB_HIST.
4. One deliberate defect at a time (languagebind_tower_ref.MUTANTS) measured with the same row_ratio against the same bar, printed as
   LB_MUTANT name=... view=... ratio=..., and for each the pooled 1 - cos of the defective model against `exact`: what the old bar of 1e-3
   (tests/test_languagebind_gpu.py COS_TOL) had to go by.  Each must leave the bar on a view the GPU file asserts, or be named in
   languagebind_tower_ref.INVISIBLE — and then stay under the bar here, so that the list cannot grow stale.

Measured (LB_HIST, worst view per case, bar 4.0): video 1.00 .. 1.65 (T = 16, B = 2, the stream after the last block), audio 1.00 .. 1.19.
Measured (LB_MUTANT: worst asserted view, its ratio; pooled 1 - cos, UNDER = the old 1e-3 bar lets the defect through):
  T8-B1   drop_out_bias_last temporal1 17.3, 4.7e-4 UNDER   ln_before_add temporal0 179, 2.1e-2   temb_roll temporal1 155, 3.9e-3   temb_layer0_in_1 temporal1 153, 1.1e-2
          regroup_bt_n temporal0 732, 2.1e-1   stale_xn_row temporal1 98, 1.5e-2   post_ln_after_mean pooled/l2=0 44, 1.0e-4 UNDER   mean_over_N pooled/l2=0 101, 2.3e-2
  T3-B3   drop_out_bias_last block1 23.4, 1.4e-3   ln_before_add temporal0 246, 4.5e-2   temb_roll temporal1 111, 3.9e-3   temb_layer0_in_1 temporal1 135, 2.7e-2
          regroup_bt_n temporal0 596, 3.5e-1   stale_xn_row temporal1 197, 7.5e-2   post_ln_after_mean pooled/l2=0 35, 1.0e-4 UNDER   mean_over_N pooled/l2=0 169, 7.4e-2
  T1-B2   drop_out_bias_last block1 13.8, 7.7e-4 UNDER   temb_at_T1 temporal0 283, 2.0e-1   regroup_bt_n temporal0 476, 4.8e-1   stale_xn_row temporal1 225, 1.5e-1
          mean_over_N pooled/l2=1 68, 2.5e-2
  audio   pos_transposed x0 900 (2 x 5 grid, b = 3), 2.0e-1;  x0 703 (2 x 2 grid), 2.1e-2
  INVISIBLE   eps_x10 1.33 / 1.91 / 1.72 (T1-B2 / T3-B3 / T8-B1), pooled 1 - cos 2e-6 .. 6e-6: the reason is at languagebind_tower_ref.INVISIBLE
Four (defect, case) pairs that the row bar sees by factors of 14 to 44 lie under the old pooled bar: the bias drop at T = 8 and at T = 1, and post_layernorm
behind the frame mean at both shapes.  (The issue's 4.8e-4 and 1.35e-3 for the bias drop are float64 against float64; here the defective pass also rounds.)
"""
import functools

import pytest
import torch

from tests import audio_ref as AR
from tests import languagebind_ref as LBR
from tests import languagebind_tower_ref as T
from tests.test_patch_attn_gpu import MARGIN

PIN_RTOL = 1e-13
COS_TOL = 1e-3          # tests/test_languagebind_gpu.py, tests/test_audio_gpu.py
VCASES, ACASES = T.video_cases(), T.audio_cases()
MUT_VCASES = [c for c in VCASES if c.id.split("[")[0] in ("T8-B1", "T3-B3", "T1-B2")]
MUT_ACASES = [c for c in ACASES if c.B > 1]


def test_max_frames_is_the_engines():
    from marqo_amd.engine.languagebind import MAX_FRAMES
    assert MAX_FRAMES == 16 and any(c.T == MAX_FRAMES for c in VCASES)


@functools.lru_cache(maxsize=None)
def _ref(kind, idx):
    """(case, ops, input, exact, model) of a case, computed once"""
    case = (VCASES if kind == "v" else ACASES)[idx]
    o = T.ops(case.cfg(), case.sd())
    x = case.clip() if kind == "v" else case.px()
    ex, mo = (T.exact(o, x), T.model(o, x)) if kind == "v" else (T.audio_exact(o, x), T.audio_model(o, x))
    return case, o, x, ex, mo


def _all():
    return [("v", i) for i in range(len(VCASES))] + [("a", i) for i in range(len(ACASES))]


def _id(k):
    return f"{k[0]}-{(VCASES if k[0] == 'v' else ACASES)[k[1]].id}"


def _cos_err(a, b):
    return float((1 - (a * b).sum(-1) / (a.norm(dim=-1) * b.norm(dim=-1))).max())


# ---- 1. exact is the restatement ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", _all(), ids=_id)
def test_exact_is_pinned_to_the_restatement(key):
    kind, idx = key
    case = (VCASES if kind == "v" else ACASES)[idx]
    cfg, sd = case.cfg(), case.sd()
    o = T.ops(cfg, sd, rounded=False)
    if kind == "v":
        got = T.exact(o, case.clip()).pooled[0]
        want = LBR.video_forward(sd, cfg, case.clip(), dtype=torch.float64)
    else:
        got = T.audio_exact(o, case.px()).pooled[0]
        want = AR.audio_forward(sd, cfg, case.px(), dtype=torch.float64)
    err = float((got - want).abs().max() / want.abs().max())
    print(f"LB_PIN case={case.id} max|exact - restatement| / max|restatement| = {err:.2e}")
    assert got.shape == want.shape and got.dtype == torch.float64 and err <= PIN_RTOL, err
    unit = LBR.embed(want, sd, "video" if kind == "v" else "audio", True)
    assert _cos_err(T.exact(o, case.clip()).pooled[1] if kind == "v" else T.audio_exact(o, case.px()).pooled[1], unit) <= 1e-14


# ---- 2. no store, no difference; stores on: no zero yardstick ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", _all(), ids=_id)
def test_model_without_stores_is_exact_and_no_yardstick_is_zero(key):
    case, o, x, ex, mo = _ref(*key)
    off = T.model(o, x, rounds=False) if key[0] == "v" else T.audio_model(o, x, rounds=False)
    for (name, a), (_, b) in zip(T.views(off).items(), T.views(ex).items()):
        assert torch.equal(a, b), f"{name}: the model with every store switched off is not the exact pass"
    assert torch.equal(off.proj, ex.proj)
    for name, e in T.views(ex).items():
        T.row_ratio(T.views(mo)[name], e, T.views(mo)[name])       # raises ZeroYardstick if a row of the model is exact
    T.row_ratio(mo.proj, ex.proj, mo.proj)
    if key[0] == "v" and case.T == 1:      # the no-add branch: the temporal embedding is not part of the pass at all
        o2 = dict(o, temporal=[dict(t, temb=t["temb"] + 1.0) for t in o["temporal"]])
        assert torch.equal(T.model(o2, x).pooled[0], mo.pooled[0])


# ---- 3. the second rounding history ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", _all(), ids=_id)
def test_second_history_stays_inside_the_bar(key):
    case, o, x, ex, mo = _ref(*key)
    h1 = T.model(o, x, hist=1) if key[0] == "v" else T.audio_model(o, x, hist=1)
    rs = {name: T.row_ratio(T.views(h1)[name], e, T.views(mo)[name])["ratio"] for name, e in T.views(ex).items()}
    print(f"LB_HIST case={case.id} worst={max(rs.values()):.3f} " + " ".join(f"{k}={v:.3f}" for k, v in rs.items()))
    assert max(rs.values()) <= MARGIN, rs
    assert any(not torch.equal(T.views(h1)[n], T.views(mo)[n]) for n in rs), "hist = 1 is no second history: it rounds as hist = 0 does"


# ---- 4. the defects ------------------------------------------------------------------------------------------------------------------------------------------
def _mutant_pairs():
    out = []
    for name in T.MUTANTS:
        if name in T.AUDIO_MUTANTS:
            out += [(name, ("a", ACASES.index(c))) for c in MUT_ACASES]
        else:
            out += [(name, ("v", VCASES.index(c))) for c in MUT_VCASES if T.applies(name, c.T)]
    return out


def test_every_mutant_is_measured_somewhere():
    assert {m for m, _ in _mutant_pairs()} == set(T.MUTANTS) and set(T.INVISIBLE) <= set(T.MUTANTS)


@pytest.mark.parametrize("name,key", _mutant_pairs(), ids=[f"{m}-{_id(k)}" for m, k in _mutant_pairs()])
def test_mutants_leave_the_bar(name, key):
    case, o, x, ex, mo = _ref(*key)
    bad = T.model(o, x, mut=name) if key[0] == "v" else T.audio_model(o, x, mut=name)
    rs = {}
    for view, e in T.views(ex).items():
        b = T.views(bad)[view]
        if b.shape != e.shape:      # (post_layernorm behind the frame mean leaves b rows where the tower leaves b T: nothing to compare row by row)
            continue
        rs[view] = T.row_ratio(b, e, T.views(mo)[view])["ratio"]
        print(f"LB_MUTANT name={name} case={case.id} view={view} ratio={rs[view]:.2f}")
    worst = max(rs, key=rs.get)
    cos = _cos_err(bad.pooled[1], ex.pooled[1])
    print(f"LB_MUTANT name={name} case={case.id} worst_view={worst} ratio={rs[worst]:.2f} pooled_1-cos={cos:.2e} "
          f"({'UNDER' if cos <= COS_TOL else 'over'} the pooled bar of {COS_TOL:g}) :: {T.MUTANTS[name]}")
    if name in T.INVISIBLE:
        assert rs[worst] <= MARGIN, f"{name} is listed as invisible and measures {rs[worst]:.2f} on {worst}"
        return
    assert rs[worst] > MARGIN, f"{name}: the bar cannot see this defect on any asserted view (worst {rs[worst]:.2f} on {worst})"


def test_the_issue_defect_passes_the_old_bar_and_not_the_new():
    """the last layer's temporal out_proj bias dropped at T = 8, B = 1: under the pooled cosine bar, over the row bar on the very stream it is added to"""
    case, o, x, ex, mo = _ref("v", next(i for i, c in enumerate(VCASES) if c.id == "T8-B1"))
    bad = T.model(o, x, mut="drop_out_bias_last")
    assert _cos_err(bad.pooled[1], ex.pooled[1]) <= COS_TOL
    last = f"temporal{o['arch'].layers - 1}"
    assert T.row_ratio(T.views(bad)[last], T.views(ex)[last], T.views(mo)[last])["ratio"] > MARGIN

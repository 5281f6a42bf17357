"""tests/packed_text_ref.py on the CPU: what tests/test_packed_text_forms_gpu.py rests on.

1. `exact` is the oracles' arithmetic.  modernbert_ref / qwen_ref / gemma_ref.oracle_hidden_packed (fp32; each pinned to transformers by its own host
   test) and `exact` agree to fp32 round-off in every call the GPU file measures against — every case and batch, all blocks and the first block alone
   (the arch cut as modernbert_ref.first_layers cuts it) — in every row behind the final norm and in the pooled rows of the family's poolings, with and
   without L2.  The bound, in units of 2**-23 times the row's norm, is  blocks * (32 + longest sequence) + 8:  per block two norms, four GEMMs, a softmax
   and a gated activation of the fp32 oracle, each a few roundings relative to the row (32 for all of them); the oracle's fp32 product position *
   inv_freq is off by up to position * 2**-24 rad, which turns q and k by as much — together position * 2**-23 of the logits' operands; 8 for the final
   norm.  It is a worst case (every frequency's angle error at its limit and of one sign) and is far from reached; at 1e-5 .. 8e-5 of a row it still
   lies 14 times and more below the rounding model's yardstick (2.), which is what it has to separate `exact` from.  A pooled row is held to the same
   multiple of the norms of the rows that enter it (their mean for mean pooling); behind L2 to twice that over the pooled row's norm.  Measured:
   PACKED_ORACLE lines, all blocks: worst row 6.22 of the 491 allowed (qwen-TINY2, the 127 / 128 / 129 batch), pooled rows 4.36; the first block alone:
   3.47 and 2.90 of 105 .. 169.
2. The claim the GPU bar rests on: a second rounding history of `model` (every GEMM summed in fp32 over reversed 64-wide k chunks) stays within MARGIN of
   the first on every case, batch, call (all blocks / the first alone) and view (the stream, the pooled rows with and without L2).  Measured:
   PACKED_HISTORY lines, worst 1.71 (qwen-TINY3, the 127 / 128 / 129 batch, all blocks); the yardstick itself is 1.1e-3 .. 4.8e-3 of a row's norm after
   all blocks, 4.5e-4 .. 3.2e-3 after the first.
3. Every mutant of packed_text_ref.MUTANTS against the plain `model`, measured as the GPU file measures a kernel: each leaves the bar by at least
   2 x MARGIN on at least one case.  Measured (PACKED_MUTANT lines; worst ratio over the cases it applies to):
       local_gets_global 80    global_gets_local 383    window_plus1 320    window_minus1 293    pattern_shift 560    layer0_attn_norm 86
       next_norm_same_block 73    no_embed_scale 2275    no_qkv_bias 619    last_row_minus1 2140 (the pooled rows alone)    stale_row 207
   NOT detectable: eps_x10.  Every norm's eps times ten measures 1.45 .. 2.39 over the 40 calls (worst: modernbert-F128, the 63 / 64 / 65 batch), inside
   the bar of 4 everywhere: the rows' mean squares are of order 1 against an eps of 1e-5 / 1e-6, so the defect itself is far below the yardstick — what
   is measured is that the small shift re-draws the bf16 roundings, which makes the mutant one more rounding history (compare 2.).  Asserted to stay
   inside the bar, so that this paragraph cannot go stale.
4. No case raises ZeroYardstick: the model differs from `exact` in every row of every view."""
import dataclasses

import pytest
import torch

from tests import packed_text_ref as P
from tests.test_patch_attn_gpu import MARGIN

CASES = P.cases()
EPS32 = 2.0 ** -23
NOT_DETECTABLE = ("eps_x10",)

_refs = {}


def _ids(case, lens):
    return torch.cat(P.seqs_of(case, lens))


def _ref(case, bname, lens, layers):
    """(exact, model) of one call, computed once and never changed"""
    key = (case.id, bname, layers)
    if key not in _refs:
        b = P.build(case)
        ids = _ids(case, lens)
        _refs[key] = (P.exact(case.family, b["arch"], b["tensors"], ids, lens, layers), P.model(case.family, b["arch"], b["tensors"], ids, lens, layers))
    return _refs[key]


def _views(case, p):
    """every tensor the GPU file measures of one call: the stream as the workspace holds it under each pooling, and the pooled rows"""
    out = {}
    for pool in P.POOLS[case.family]:
        out["stream/" + ("pre_norm" if pool == "last" else "final")] = P.views(p, pool)
        for l2 in (0, 1):
            out[f"pooled/{pool}/l2={l2}"] = p.pooled[(pool, l2)]
    return out


def _worst(case, got, ex, mo):
    """(ratio, view, row) of the worst row over every view"""
    g, e, m = _views(case, got), _views(case, ex), _views(case, mo)
    best = (0.0, "", -1)
    for name in g:
        r = P.row_ratio(g[name], e[name], m[name])      # raises ZeroYardstick where a row of the model is exact
        if r["ratio"] > best[0]:
            best = (r["ratio"], name, r["row"])
    return best


def _calls(case):
    arch = P.build(case)["arch"]
    for bname, lens in case.batches():
        for layers in (arch.layers, 1):
            yield bname, lens, layers


def _cut(arch, layers):
    """the model cut behind its first `layers` blocks (the final norm follows), as modernbert_ref.first_layers cuts it"""
    kw = dict(layers=layers)
    if hasattr(arch, "sliding"):
        kw["sliding"] = tuple(arch.sliding[:layers])
    return dataclasses.replace(arch, **kw)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_exact_is_the_fp32_oracle(case):
    """every call the GPU file measures against: both batches, all blocks and the first block alone; every row behind the final norm, and the pooled rows
    of the family's poolings with and without L2 (formed here in float64 from the oracle's rows)"""
    b = P.build(case)
    arch, ref = b["arch"], P._ref_module(case.family)
    for bname, lens, layers in _calls(case):
        seqs = P.seqs_of(case, lens)
        if case.family == "gemma":
            hidden = ref.oracle_hidden_packed(b["sd"], _cut(arch, layers), seqs)
        else:
            hidden = ref.oracle_hidden_packed(b["tensors"], _cut(arch, layers), seqs, kernel_glu=True)
        hidden = [h.double() for h in hidden]
        want = torch.cat(hidden)
        ex = _ref(case, bname, lens, layers)[0]
        mult = layers * (32 + max(lens)) + 8
        err = (ex.final - want).norm(dim=1) / want.norm(dim=1) / EPS32
        worst_pooled = 0.0
        for pool in P.POOLS[case.family]:
            rows = torch.stack([h.mean(0) if pool == "mean" else h[0] if pool == "cls" else h[-1] for h in hidden])
            # the rows that enter the pooled row carry errors of up to mult * 2^-23 of their norms: so does their mean, against the mean of those norms
            scale = torch.stack([h.norm(dim=1).mean() if pool == "mean" else h[0].norm() if pool == "cls" else h[-1].norm() for h in hidden])
            e0 = (ex.pooled[(pool, 0)] - rows).norm(dim=1) / scale / EPS32
            # L2: |n(v + e) - n(v)| <= 2 |e| / |v| for the unit rows n(.)
            e1 = (ex.pooled[(pool, 1)] - rows / rows.norm(dim=1, keepdim=True)).norm(dim=1) / (2.0 * scale / rows.norm(dim=1)) / EPS32
            worst_pooled = max(worst_pooled, float(e0.max()), float(e1.max()))
        print(f"PACKED_ORACLE case={case.id} batch={bname} layers={layers}: worst row |exact - oracle| / |row| = {float(err.max()):.2f} x 2^-23 (row {int(err.argmax())}), "
              f"pooled rows {worst_pooled:.2f}; bound {mult}")
        assert float(err.max()) <= mult and worst_pooled <= mult


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_second_rounding_history_stays_within_margin(case):
    b = P.build(case)
    for bname, lens, layers in _calls(case):
        ex, mo = _ref(case, bname, lens, layers)
        m2 = P.model(case.family, b["arch"], b["tensors"], _ids(case, lens), lens, layers, hist=1)
        a, c = _worst(case, m2, ex, mo), _worst(case, mo, ex, m2)
        y = (P.views(mo, "mean") - P.views(ex, "mean")).norm(dim=1) / P.views(ex, "mean").norm(dim=1)
        print(f"PACKED_HISTORY case={case.id} batch={bname} layers={layers}: second against first {a[0]:.3f} ({a[1]} row {a[2]}), first against second {c[0]:.3f}; "
              f"yardstick per row, relative: min {float(y.min()):.2e} median {float(y.median()):.2e} max {float(y.max()):.2e}")
        assert _worst(case, mo, ex, mo)[0] == 1.0 and max(a[0], c[0]) <= MARGIN


@pytest.mark.parametrize("mut", P.MUTANTS)
def test_mutant_against_the_plain_model(mut):
    """measured in every call the GPU file makes: both batches, all blocks and the first block alone (stale_row: all blocks), every view"""
    worst, moved = {}, 0.0
    for case in CASES:
        b = P.build(case)
        if not P.applies(mut, case, b["arch"]):
            continue
        for bname, lens, layers in _calls(case):
            if mut == "stale_row" and layers < 2:
                continue
            ex, mo = _ref(case, bname, lens, layers)
            bad = P.model(case.family, b["arch"], b["tensors"], _ids(case, lens), lens, layers, mut=mut)
            r = _worst(case, bad, ex, mo)
            # how far the defect itself moves a row, in yardsticks
            moved = max(moved, float(((P.views(bad, "mean") - P.views(mo, "mean")).norm(dim=1) / (P.views(mo, "mean") - P.views(ex, "mean")).norm(dim=1)).max()))
            print(f"PACKED_MUTANT {mut} case={case.id} batch={bname} layers={layers}: ratio {r[0]:.3f} ({r[1]} row {r[2]})")
            worst[case.id] = max(worst.get(case.id, 0.0), r[0])
    assert worst, "the mutant applies to no case"
    top = max(worst.values())
    print(f"PACKED_MUTANT {mut}: worst ratio over {len(worst)} cases {top:.3f} = {top / MARGIN:.2f} x the bar; the defect moves a stream row by up to {moved:.3f} yardsticks")
    if mut in NOT_DETECTABLE:
        assert top <= MARGIN, "the module docstring lists this mutant as not detectable: it now leaves the bar — move it to the detected ones"
    else:
        assert top >= 2.0 * MARGIN

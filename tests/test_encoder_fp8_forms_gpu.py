"""The e4m3 block dataflows of csrc/towers.hip (encoder_forward_impl: block_fp8, the MLP-only e4m3 block inside block_pre_ln, the e4m3 body of
last_block_selected) through the C ABI, every row of the token stream held to the float64 reference and the e4m3 rounding model of tests/encoder_ref.py.
The kernels underneath have their own parity tests; this file is about the hand-offs between them: the per-row scales one launch writes and the next
GEMM reads, the static scales' slots, the bf16 -> e4m3 transition, and what a row selection and a recording call switch off.

Engine, guards and the measure are tests/test_encoder_forms_gpu.py's (_Engine, _measure, GUARD_ROWS, SENTINEL, MARGIN): the weights are quantised by the
engine's own _Fp8State and read back, the static activation scales are max |exact tensor| / 448 of the float64 reference — never a recording run's — on a
checkpoint whose six scales lie a factor of two or more apart (tests/test_encoder_ref_host.py asserts it), so that a scale from another slot is far off.

Every case (E.f8_cases(): 3 blocks, W 128, two 64-wide heads, F 256, 217 packed / 5 x 50 fixed rows):
  - the worst row of max(l2, linf) of |got - exact| / |model - exact| <= MARGIN after all blocks and after the first block alone, printed as ENCODER_RATIO;
  - the stream between 64 guard rows, the workspace exactly mq_encoder_workspace_bytes long with an untouched sentinel tail (_Engine.run);
  - the same call twice, the second on a workspace of other garbage: the same bits;
  - mq_encoder_forward_rows on a pre-LN e4m3 form: the selected rows within the bar, every other row the bits of a `layers - 1` call;
    with d_fp8_act_amax set, and on a post-LN e4m3 form: the bits of mq_encoder_forward (select_last is off);
  - one case with every scale divided by 4: a share of the values saturates, the model clamps at +-448, the stream stays finite and within the bar.
Recording calls (d_fp8_act_amax): the stream has the bits of the call without recording; amax[l, k] of every e4m3 tensor is the exact reference's maximum
within MARGIN x |model's maximum - exact maximum|; entries of bf16 blocks keep the sentinel they were filled with, the MLP-only block writes [l, 1] alone;
a second recording call accumulates the maximum.

Measured on an MI355X (worst ENCODER_RATIO per form over its cases, all blocks / first block alone; bar 4.0):
  f8/pre_ln/f32 1.47 / 1.31 (scales / 4, saturating: 1.02 / 1.02)     f8/pre_ln/bf16 2.92 / 2.49     f8/pre_ln/bf16+fold|split1 2.69 / 2.36
  f8/pre_ln/bf16+fold|split2+mlp1 1.63 / 1.04     f8/post_ln 1.73 / 1.53     f8/post_ln|split1 1.90 / 1.72
Selected rows (mq_encoder_forward_rows, 10 of 217 rows): 1.07 for f8/pre_ln/f32, 2.16 for f8/pre_ln/bf16; the other 207 rows equal the 2-block stream bit
for bit in both.  Recorded maxima: worst ratio 2.54 (amax[1, 0] of the fp32-stream case), the others 0.15 .. 1.53.
On the CPU (tests/test_encoder_ref_host.py) the second rounding history stays within 2.07 of the first over all cases, and the mutations leave the bar by
at least: scales swapped 6.4 x, scales of layer l - 1 7.8 x, neighbour's row scale 13.5 x, LN1's row scale for LN2 2.5 x, truncation 1.1 x, the 2 * Wa gather
2.6 x; a skipped rowquant and a non-saturating store give NaN.

Found by this file: no defect in towers.hip — every hand-off listed above does what its comment says.  What the first run did find was an input of this
file's own: with the rows' strong channel RAISED by up to 30 the bf16 stream held values of 32 .. 64 there, one bf16 step of which (0.25) outweighs the rest
of a row's error; the split1 case measured 4.71 in the max-norm in that channel (1.42 in the 2-norm) — two roundings of one value falling to different
sides, not a rounding the model lacks.  The channel is now lowered instead (E.make_input), which keeps it below 32 as in the bf16 cases; the bar stayed.
"""
import pytest
import torch

from tests import encoder_ref as E
from tests.knobs import tuned
from tests.test_encoder_forms_gpu import DEV, MARGIN, _Engine, _measure

pytestmark = pytest.mark.gpu

CASES = E.f8_cases()
_IDS = [c.id for c in CASES]
_BY_ID = {c.id: i for i, c in enumerate(CASES)}
AMAX_SENTINEL = -1.0        # (the accumulators take an integer atomic maximum of non-negative floats: any write replaces a negative fill)


def _case(idx) -> E.Case:
    return E.f8_cases()[idx]


def _bits(t):
    return t.contiguous().view(torch.uint8)


def _check_readback(case):
    """the codes and scales read back from the engine are those of the weights the reference holds: within half an e4m3 step of the top binade per row"""
    from tests.gemm_fp8_ref import decode
    base = E.blocks_to(E.blocks_from_sd(case.kind, case.sd(), "t.", case.layers), DEV)
    for l, b in enumerate(base):
        for name in E.F8_NAMES:
            codes, ws = case.q8[l][name]
            w = b[name + "_w"]
            assert codes.shape == w.shape and ws.shape == (w.shape[0],)
            err = (decode(codes) * ws.double()[:, None] - w).abs().amax(1)
            assert bool((err <= w.abs().amax(1) * 2.0 ** -4 / 1.75 * 1.001 + 1e-30).all()), f"block {l} {name}: the engine's e4m3 weights are not the checkpoint's"


@pytest.mark.parametrize("idx", range(len(_IDS)), ids=_IDS)
def test_encoder_fp8_form_against_float64(idx):
    case = _case(idx)
    sel_rows = case.sel_rows()
    selected = sel_rows is not None and len(sel_rows) * 2 <= case.rows and not case.post_ln      # (post-LN e4m3: select_last is off)
    with tuned(**case.knobs):
        eng = _Engine(case)
        _check_readback(case)
        sel = torch.tensor(sel_rows, dtype=torch.int32, device=DEV) if sel_rows is not None else None
        got, _ = eng.run(case.layers, sel)
        again, _ = eng.run(case.layers, sel, ws_fill=0x3C)
        first, _ = eng.run(1)
        before, _ = eng.run(case.layers - 1) if selected else (None, None)
        full, _ = eng.run(case.layers) if (sel is not None and not selected) else (None, None)
    assert torch.equal(_bits(got), _bits(again)), "the same call twice: other bits"
    worst = []
    if selected:
        idx_t = torch.tensor(sel_rows, device=DEV)
        worst.append(_measure(case, got, case.layers, idx_t))
        keep = torch.ones(case.rows, dtype=torch.bool, device=DEV)
        keep[idx_t] = False
        n_diff = int((_bits(got[keep]) != _bits(before[keep])).any(dim=1).sum())
        print(f"ENCODER_OTHER_ROWS case={case.id}: {n_diff} of {int(keep.sum())} non-selected rows differ from the stream of a {case.layers - 1}-block call")
    else:
        worst.append(_measure(case, got, case.layers))
    worst.append(_measure(case, first, 1))
    assert max(worst) <= MARGIN
    if selected:
        assert n_diff == 0, "rows outside the selection are not the stream of the block before"
    if full is not None:
        assert torch.equal(_bits(got), _bits(full)), "a row selection on a post-LN e4m3 form: not the stream of mq_encoder_forward"


def _amax(case):
    return torch.full((case.layers, 2), AMAX_SENTINEL, dtype=torch.float32, device=DEV)


def test_row_selection_while_recording_runs_every_row():
    """d_fp8_act_amax set: select_last is off, the maxima see every row — the stream and the maxima of mq_encoder_forward with the same pointer"""
    case = _case(_BY_ID["f8-rows-pre_ln-f32-packed217[select_last,f8]"])
    with tuned(**case.knobs):
        eng = _Engine(case)
        sel = torch.tensor(case.sel_rows(), dtype=torch.int32, device=DEV)
        m_sel, m_full = _amax(case), _amax(case)
        got, _ = eng.run(case.layers, sel, amax=m_sel)
        full, _ = eng.run(case.layers, None, amax=m_full)
        pooled, _ = eng.run(case.layers, sel)
    assert torch.equal(_bits(got), _bits(full)) and torch.equal(m_sel, m_full) and bool((m_sel > 0).all())
    n = int((_bits(pooled) != _bits(full)).any(dim=1).sum())
    print(f"ENCODER_RECORDING_SELECTION case={case.id}: without recording {n} rows differ from the full call (the rows the selection leaves out)")
    assert n > 0


_CALIBRATED = ["f8-pre_ln-f32-gelu-packed217[block_fp8,first8=0]", "f8-pre_ln-bf16-gelu-fixed5x50[first8=2,fp8_mlp_extra=1,ln_fold=2,rs_finalize=1]",
               "f8-post_ln-gelu-fixed5x50[first8=1,residual_stream=1:post16=0]"]


@pytest.mark.parametrize("cid", _CALIBRATED)
def test_recording_call(cid):
    case = _case(_BY_ID[cid])
    form = case.form
    with tuned(**case.knobs):
        eng = _Engine(case)
        plain, _ = eng.run(case.layers)
        amax = _amax(case)
        got, _ = eng.run(case.layers, amax=amax)
        first = amax.clone()
        mult = torch.tensor([2.0, 0.5], device=DEV).expand_as(first)        # a larger maximum from an earlier call stays, a smaller one is raised
        preset = torch.where(first > 0, first * mult, first)
        amax.copy_(preset)
        eng.run(case.layers, amax=amax)
    assert torch.equal(_bits(got), _bits(plain)), "a recording call changes the stream"
    s = E.f8_setup(case, DEV)
    rec: dict = {}
    E.model(s["cfg"], s["blocks"], s["x0"], case.lens, s["form"], rec=rec)
    for l in range(case.layers):
        for k in (0, 1):
            written = l >= form.first8 or (k == 1 and l >= form.first8 - form.mlp_extra)
            v = float(first[l, k])
            if not written:
                assert v == AMAX_SENTINEL and float(amax[l, k]) == AMAX_SENTINEL, f"amax[{l}, {k}] of a bf16 tensor was written"
                continue
            ex, mo = s["amax_exact"][(l, k)], rec[(l, k)]
            if mo == ex:
                raise E.ZeroYardstick(f"amax[{l}, {k}]: the model's maximum equals the exact one")
            ratio = abs(v - ex) / abs(mo - ex)
            print(f"ENCODER_AMAX case={case.id} amax[{l}, {k}] = {v:.6g} exact {ex:.6g} model {mo:.6g} ratio {ratio:.3f}")
            assert ratio <= MARGIN
            assert float(amax[l, k]) == max(v, float(preset[l, k])), f"amax[{l}, {k}]: the second recording call did not accumulate a maximum"

"""The block dataflows of csrc/towers.hip (encoder_forward_impl) through the C ABI — mq_encoder_workspace_bytes, mq_encoder_forward,
mq_encoder_forward_rows — with every row of the token stream held to the float64 reference of tests/encoder_ref.py.

Every case: weights from the engine's own loaders (_clip_blocks / _bert_blocks / _eva_blocks, folded tensors included) on a seeded checkpoint,
knobs through tests.knobs.tuned, and
  - the worst row of  max(|got - exact|_2 / |model - exact|_2, |got - exact|_inf / |model - exact|_inf)  <= MARGIN (tests/test_patch_attn_gpu.py),
    `model` being the rounding model of the form the case means to reach, after all blocks AND after the first block alone; printed as
    ENCODER_RATIO form=... case=... ratio=...;
  - the stream lies between 64 guard rows of a sentinel on either side, the workspace is exactly mq_encoder_workspace_bytes long with a sentinel
    region behind it: both come back untouched;
  - the same call made twice (the second on a workspace filled with other garbage) gives the same bits;
  - the launches per kernel family (mq_profile_collect: LayerNorm / statistics / cast, attention, gather / rotary / gate) are those the form implies,
    where the form implies a count (Case.launches; derivation below);
  - mq_encoder_forward_rows with a selection that halves the rows: the selected rows (first, middle and last row of every sequence) are within the
    bar of `exact`, every other row equals, bit for bit, the stream a `layers - 1` call leaves.

Which launch counts tell forms apart (LayerNorm family, attention family, gather family; 2 blocks):
  pre-LN, LayerNorm kernels 4 / 2 / 0; LayerNorms inside the skinny GEMMs (rows <= small_m) 0 / 2 / 0; folded with in-launch statistics (rs_finalize = 1) 1 / 2 / 0;
  post-LN fp32 5 (cast + 4 LayerNorms) / 2 / 0, rows <= 32: 2 (cast + the last LayerNorm); rotary + gate +2 gathers per block; a row selection +3 gathers.
  NOT told apart by anything observable: ln_fold 0 / 1 / 2 with rs_finalize = 0 (each 4 launches of the LayerNorm family: LayerNorms, statistics passes
  or finalise launches), block_post_ln against block_post_ln_bf16 (5 / 2 / 0 both), the EVA sub-LayerNorm fold against its kernels (printed, not asserted),
  the panel GEMM against the tiled GEMM (one GEMM launch each; the attention + out-projection launch is seen: 1 LayerNorm-family launch instead of 2).

The e4m3 forms — block_fp8, the MLP-only e4m3 block and the e4m3 body of last_block_selected — are held to their own rounding model in
tests/test_encoder_fp8_forms_gpu.py, which runs them through this file's _Engine.

Not covered here:
  - the fixed-pitch selected body (sel_strided_ok) and the `stats0` hand-in: encoder_forward_impl takes both from the image tower only
    (mq_encode_image_*); tests/test_tower_passes_gpu.py reads the stream and the stats0 region of those calls from the tower's workspace and holds
    them to the float64 reference of tests/tower_ref.py.

Measured on an MI355X (worst ENCODER_RATIO per form over its cases, all blocks / first block alone; bar 4.0):
  pre_ln/f32 1.55 / 1.75     pre_ln/bf16 1.61 / 1.29     pre_ln/bf16+fold 2.52 / 1.10 (the 768-wide one-workgroup-per-image case 1.54)
  post_ln/f32 1.87 / 2.00    post_ln_small 1.53 / 1.10   post_ln_bf16 2.34 / 1.90
  eva/f32 1.43 / 1.21        eva/bf16+fold+glu_epi 1.33 / 1.01     eva/bf16+fold+glu_epi+subln_fold 1.21 / 1.03
  (the folded sub-LayerNorms measured 4.05 against the model of the un-folded ones, in the 24-unit outlier channel: the fold multiplies bf16(g W) with
  the un-normalised rows, a rounding the un-folded model does not make — it went into the model as Form.sub_fold, the margin stayed)
(encoder_ref no longer folds fc1 in a row-selected last block, as last_block_selected does not: no case of this file selects rows on a folded form, so the
references of its cases, and with them the figures here, are the same numbers as before)
Selected rows (mq_encoder_forward_rows, 10 of 217 rows): 1.26 / 1.02 / 1.51 / 2.34 for pre_ln/f32, pre_ln/bf16, post_ln/f32, post_ln_bf16; the other 207
rows equal the 1-block stream bit for bit in all four.

Found by this file: on the post-LN bf16 stream the blocks before the last keep the stream in `h` (bf16) and never wrote d_x, so after a row-selected
call all 207 non-selected rows still held the CALLER'S INPUT, not the previous block's output.  block_post_ln_bf16 now lets the LayerNorm in front of
a selected last block write its fp32 rows to d_x as well (the kernel a call of one block fewer ends in: the same bits)."""
import ctypes as C

import pytest
import torch

from marqo_amd import _lib as L
from tests import encoder_ref as E
from tests import knobs
from tests.knobs import tuned
from tests.test_patch_attn_gpu import MARGIN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD_ROWS = 64
SENTINEL = 0xA5

_IDS = [c.id for c in E.cases(80)]       # (the ids do not depend on the knob; the row counts of two cases do, and are read at run time)
_ACT = {"gelu": L.MQ_ACT_GELU, "quick": L.MQ_ACT_QUICKGELU, "relu": L.MQ_ACT_RELU, "silu": L.MQ_ACT_SILU}


def _stream():
    return torch.cuda.current_stream().cuda_stream


class _Engine:
    """the loaders' tensors and the mq_encoder_cfg of one case"""

    def __init__(self, case: E.Case):
        from marqo_amd.engine import tower_weights as TW, towers
        self.case = case
        self.holder = TW._Holder(torch.device(DEV))
        sd, W, F, H, n = case.sd(), case.W, case.F, case.heads, case.layers
        if case.kind == "clip":
            self.blocks = TW._clip_blocks(self.holder, sd, "t.", n, W, F, H)
        elif case.kind in ("bert", "new_model"):
            self.blocks = TW._bert_blocks(self.holder, sd, "t.", n, W, F, H, new_model=case.kind == "new_model")
        else:
            was = TW.EVA_GLU_EPILOGUE       # mlp_glu = 2: (up, gate) rows interleaved 16 by 16; 1: (up | gate)
            TW.EVA_GLU_EPILOGUE = case.glu == 2
            try:
                self.blocks = TW._eva_blocks(self.holder, sd, "t.", n, W, F, H)
            finally:
                TW.EVA_GLU_EPILOGUE = was
        ref = case.cfg()
        cfg = towers._encoder_cfg(W, n, H, F, case.act == "quick", case.post_ln, case.mask, case.eps())
        cfg.act, cfg.residual_stream, cfg.mlp_glu = _ACT[case.act], case.stream, case.glu
        self.keep = []
        if ref.inv_freq is not None:
            self.keep.append(ref.inv_freq.to(DEV).contiguous())
            cfg.d_rope_inv_freq = self.keep[-1].data_ptr()
        if ref.rope_table is not None:
            self.keep.append(ref.rope_table.to(DEV).contiguous())
            cfg.d_rope_table, cfg.rope_prefix = self.keep[-1].data_ptr(), ref.rope_prefix
        if ref.rel_bias is not None:        # the kernel adds the table to the UNSCALED scores: the bias times sqrt(head width) (include/marqo_hip.h)
            self.keep.append((ref.rel_bias * (W // H) ** 0.5).float().to(DEV).contiguous())
            cfg.d_rel_bias, cfg.rel_span = self.keep[-1].data_ptr(), max(case.lens)
        if case.kind == "eva" and case.sub_ln:
            cfg.mlp_ln_dim = F
        self.f8 = None
        if case.form.first8 is not None:
            # the e4m3 forms (tests/test_encoder_fp8_forms_gpu.py): the engine's own class quantises the weights; the reference takes the codes and scales it
            # wrote (Case.q8); the static activation scales come from the float64 reference (E.f8_setup), never from a recording run
            n0 = len(self.holder.tensors)
            self.f8 = towers._Fp8State(L.load(), self.holder, self.blocks, n, W, F, torch.device(DEV))
            torch.cuda.synchronize()
            t = self.holder.tensors[n0:]
            assert len(t) == 8 * n
            case.q8 = [{name: (t[(i * 4 + j) * 2], t[(i * 4 + j) * 2 + 1]) for j, name in enumerate(E.F8_NAMES)} for i in range(n)]
            self.f8.scale.copy_(E.f8_setup(case, DEV)["scales"])
            self.f8.attach(cfg, calibrating=False)
            cfg.fp8_first_layer, cfg.fp8_mlp_extra = case.form.first8, case.form.mlp_extra
        self.cfg = cfg
        self.bf16_io = case.stream == 1 and not case.post_ln      # the caller of a pre-LN bf16-stream encoder hands bf16 rows in and gets bf16 rows back
        fixed = len(set(case.lens)) == 1
        self.fixed_len = case.lens[0] if fixed else 0
        from tests import attention_ref as A
        self.cu = None if fixed else A.cu_seqlens(case.lens, DEV)
        self.x0 = case.x0().to(DEV)

    def run(self, layers, sel=None, ws_fill=SENTINEL, profile=False, amax=None):
        """one call on a fresh guarded stream and workspace -> (stream [rows, W] in its stored type, launches per family or None).  `amax`: the fp32
        [layers, 2] accumulator of a recording call of an e4m3 form (d_fp8_act_amax)"""
        lib, case = L.load(), self.case
        if self.f8 is not None:
            self.cfg.d_fp8_act_amax = amax.data_ptr() if amax is not None else None
        rows, W = case.rows, case.W
        dt = torch.bfloat16 if self.bf16_io else torch.float32
        rb = W * (2 if self.bf16_io else 4)
        buf = torch.full(((rows + 2 * GUARD_ROWS) * rb,), SENTINEL, dtype=torch.uint8, device=DEV)
        x = buf[GUARD_ROWS * rb:(GUARD_ROWS + rows) * rb].view(dt).view(rows, W)
        x.copy_(self.x0.to(dt))
        self.cfg.layers = layers
        need = lib.mq_encoder_workspace_bytes(C.byref(self.cfg), rows, len(case.lens))
        assert need > 0
        ws = torch.full((need + 4096,), ws_fill, dtype=torch.uint8, device=DEV)
        assert x.data_ptr() % 256 == 0 and ws.data_ptr() % 256 == 0
        cu = self.cu.data_ptr() if self.cu is not None else None
        torch.cuda.synchronize()
        if profile:
            L.check(lib.mq_profile_collect(None, None, None), "mq_profile_collect")
            L.check(lib.mq_profile_enable(1), "mq_profile_enable")
        try:
            if sel is None:
                rc = lib.mq_encoder_forward(C.byref(self.cfg), self.blocks, x.data_ptr(), rows, cu, len(case.lens), self.fixed_len, max(case.lens), ws.data_ptr(), need,
                                            _stream())
            else:
                rc = lib.mq_encoder_forward_rows(C.byref(self.cfg), self.blocks, x.data_ptr(), rows, cu, len(case.lens), self.fixed_len, max(case.lens), sel.data_ptr(),
                                                 sel.numel(), ws.data_ptr(), need, _stream())
            L.check(rc, "mq_encoder_forward")
            torch.cuda.synchronize()
            launches = None
            if profile:
                n = (C.c_int64 * L.MQ_PROF_FAMILIES)()
                L.check(lib.mq_profile_collect(None, n, None), "mq_profile_collect")
                launches = list(n)
        finally:
            if profile:
                lib.mq_profile_enable(0)
        g = GUARD_ROWS * rb
        assert bool((buf[:g] == SENTINEL).all()) and bool((buf[g + rows * rb:] == SENTINEL).all()), "a guard row of the stream was written"
        assert bool((ws[need:] == ws_fill).all()), "the workspace was written past mq_encoder_workspace_bytes"
        return x.clone(), launches


_engines = {}


def _case(idx) -> E.Case:
    return E.cases(knobs.get("small_m"))[idx]


def _measure(case, got, layers, rows=None):
    ex, mo = E.reference(case, DEV, layers)
    assert bool(torch.isfinite(got.double()).all())
    r = E.row_ratio(got.double(), ex, mo, rows)
    print(f"ENCODER_RATIO form={case.form.name} case={case.id} layers={layers} ratio={r['ratio']:.3f} (row {r['row']} col {r['col']}: l2 {r['l2']:.3f} linf {r['linf']:.3f})")
    return r["ratio"]


@pytest.mark.parametrize("idx", range(len(_IDS)), ids=_IDS)
def test_encoder_form_against_float64(idx):
    case = _case(idx)
    sel_rows = case.sel_rows()
    with tuned(**case.knobs):
        eng = _Engine(case)
        sel = torch.tensor(sel_rows, dtype=torch.int32, device=DEV) if sel_rows is not None else None
        got, launches = eng.run(case.layers, sel, profile=True)
        again, _ = eng.run(case.layers, sel, ws_fill=0x3C)
        first, _ = eng.run(1) if case.layers > 1 else (None, None)
        before, _ = eng.run(case.layers - 1) if (sel is not None and case.layers > 1) else (None, None)
    assert torch.equal(got.view(torch.uint8), again.view(torch.uint8)), "the same call twice: other bits"
    print(f"ENCODER_LAUNCHES case={case.id} gemm={launches[0]} layernorm={launches[1]} attention={launches[2]} gather={launches[3]}")
    selected = sel_rows is not None and len(sel_rows) * 2 <= case.rows
    worst = []
    if selected:
        idx_t = torch.tensor(sel_rows, device=DEV)
        worst.append(_measure(case, got, case.layers, idx_t))
        keep = torch.ones(case.rows, dtype=torch.bool, device=DEV)
        keep[idx_t] = False
        n_diff = int((got[keep].view(torch.uint8) != before[keep].view(torch.uint8)).any(dim=1).sum())
        print(f"ENCODER_OTHER_ROWS case={case.id}: {n_diff} of {int(keep.sum())} non-selected rows differ from the stream of a {case.layers - 1}-block call")
    else:
        worst.append(_measure(case, got, case.layers))
    if first is not None:
        worst.append(_measure(case, first, 1))
    for want, have, fam in zip(case.launches or (), launches[1:4], ("layernorm", "attention", "gather")):
        if want is not None:
            assert have == want, f"{fam} family: {have} launches, the form implies {want}"
    assert max(worst) <= MARGIN
    if selected:
        assert n_diff == 0, "rows outside the selection are not the stream of the block before"

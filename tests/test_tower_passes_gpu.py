"""The whole passes of the three original towers through the C ABI — mq_encode_image_u8 / _f32, mq_encode_clip_text, mq_encode_bert (csrc/towers.hip) —
with d_out and every row of the token stream held to the float64 reference of tests/tower_ref.py.  Under test is the host orchestration: patchify ->
conv GEMM -> assembly (with and without the stats0 hand-in), the pooled last block at a fixed pitch or through an index vector, the four image heads,
mq_embed_tokens with cls_pos, mq_last_rows or the caller's rows, the biased SigLIP projection, BERT's embedding LayerNorm, pooling and the three heads,
and the plan arithmetic of vit_plan / text_plan.  The kernels have their own files.

cfg and weights come from VitTower / ClipTextTower / BertTower / MclipTextTower / HfClipTextTower on the seeded checkpoints of tower_ref's cases; the calls
are made here on a workspace of exactly mq_*_workspace_bytes, knobs through tests.knobs.tuned.

Every case, normalize 0 and 1:
  - the worst row of max(|got - exact|_2 / |model - exact|_2, |got - exact|_inf / |model - exact|_inf) <= MARGIN (tests/test_patch_attn_gpu.py) on d_out,
    on the stream after all blocks and after the first block alone; a row-selected last block: the selected rows against `exact` after all blocks, every
    other row against `exact` after layers - 1 blocks; no row skipped.  Printed as TOWER_RATIO tower=... case=... n=... view=... ratio=...
  - layout, before any ratio is measured: the plan restated here gives the library's *_workspace_bytes, and library kernels redo the head from the slice and must
    give d_out bit for bit — BERT without projection: mq_pool; BERT with a head: mq_pool + the bf16 cast + mq_gemm_bf16 (+ mq_l2_normalize); CLIP text with the
    LayerNorm + tiled head (81 sequences, SigLIP's proj_b): mq_layernorm_ex + mq_gemm_bf16; the image tower's tiled class-token head (n = 100, 321):
    mq_cls_rows + mq_layernorm_ex by row index + mq_gemm_bf16.  A failure says "the workspace layout changed; no parity was measured".
  - the launches per kernel family (mq_profile_collect) are those the branch the case names implies (_expect_vit / _expect_text / _expect_bert: the derivation is
    in their docstrings; row limits from mq_tune_get): the LayerNorm family tells the skinny prologue from the LayerNorm + tiled head, the pooled block on 20 /
    100 / 321 rows, post_ln_small; the gather family tells sel_strided_ok from the index vector and a row-selected last block from a full one;
  - d_out between guard rows and a sentinel region behind the workspace come back untouched;
  - the same call on a workspace of 0xFF bytes (NaN as bf16 and fp32) and of 0x3C bytes gives the same finite bits in stream and d_out;
  - a workspace one byte short: MQ_ERR_WORKSPACE, d_out and workspace keep their fill;
  - stats0 cases: the region at off_stats0 holds (mean, rstd) of the assembled bf16 rows (read by a layers = 0 call of the same case: the assembly's bits do
    not depend on the hand-in, tests/test_vit_step_fusions_gpu.py) within the budget of tests/rowops_ref.py at tests/test_rowops_gpu.py's margin, and the
    LayerNorm-family launch count is one below the same call with assemble_stats = 0: the statistics pass was not launched;
  - u8 and f32 pixel input: each entry point with all of the above (both normalize settings, both fills, the short workspace), each within the bar of its own reference;
  - a permuted batch of images returns the permuted rows bit for bit (small_m = 0: every GEMM on the tiled family).

The image cases' batch sizes come from mq_tune_get("small_m") / ("small_m_grouped") at run time (tower_ref.vit_cases); the ids are those of the defaults.

Measured on an MI355X (worst TOWER_RATIO per tower over its cases: stream after all blocks / after the first block alone / d_out; bar 4.0):
  image 2.18 / 1.66 / 1.81 (f32 pixel input 2.18; the assembled rows of a no-block call 1.004); MAP with the final projection 1.40 / 1.13 / 1.51; EVA 1.42 / 1.25 / 1.30
  clip_text 1.90 / 1.33 / 1.74      bert 2.14 / 2.58 / 2.10; rotary + gated MLP 1.49 / 1.52 / 1.14; MPNet's relative bias 1.62 / 2.74 / 1.46
  stats0 against the float64 statistics of the assembled bf16 rows, in units of rowops_ref's budget (bar 1.25): mean <= 0.008, rstd <= 0.23; the LayerNorm
  family has one launch fewer with the hand-in (2 against 3 at 340 rows, 4 against 5 at T = 5) in all five cases meant to reach it.
  Every implied launch count was met on the first run; every head redo gave d_out bit for bit.
One rounding went into the model, the margin stayed: after a ONE-block BERT call with CLS pooling the 213 non-selected rows are the embedding LayerNorm's own
fp32 output; against a model that rounds a float64 LayerNorm once they measured 7.57 (fp32 mean / variance / rsqrt of the kernel are a few ulps, the yardstick
was half an ulp).  tower_ref's BERT front end now does that LayerNorm in fp32 arithmetic, as embed_tokens_kernel does: 2.58.

Found by this file: nothing in the library.  What a defect of the orchestration would measure is in tests/test_tower_ref_host.py (TOWER_MUTANT: 37 .. 4621
against this bar of 4.0; a neighbour's stats0 is the one listed defect the ratio bar cannot see, and the stats0 check above sees it by four orders of magnitude).
"""
import ctypes as C
import os
import types

import pytest
import torch

from marqo_amd import _lib as L
from tests import attention_ref as A
from tests import encoder_ref as E
from tests import knobs
from tests import rowops_ref as R
from tests import tower_ref as T
from tests.knobs import tuned
from tests.test_patch_attn_gpu import MARGIN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD_ROWS = 8
SENTINEL = 0xA5
MQ_ERR_WORKSPACE = -3
LAYOUT = "the workspace layout changed; no parity was measured"

VCASES, TCASES, BCASES = T.vit_cases(), T.text_cases(), T.bert_cases()       # (ids only: the image cases' batch sizes are read again at run time, from the knobs)
_towers = {}
LN_ROWS = 32        # rows up to which the skinny GEMM takes a LayerNorm into its prologue (gemm_small.hip SM_LN_MAX_MT * 16 = towers.hip SMALL_LN_ROWS)


def _vcase(idx):
    return T.vit_cases(knobs.get("small_m"), knobs.get("small_m_grouped"))[idx]


def _expect_vit(case, ka, ln_fold, pool_strided):
    """(LayerNorm family, gather family) launches the branch the case names implies for a 2-block call without L2; None: not derived.
    Class-token towers: rows <= 32 every LayerNorm rides in a skinny GEMM's prologue; up to small_m 4 LayerNorm launches; beyond, block 0 has 2 (folded:
    the fc1 statistics' launch, and the QKV statistics pass unless stats0 is handed in), the row-selected block 1 has LN1 / the QKV statistics (1) and LN2 on
    the pooled rows (a launch past 32 pooled rows), the head's LayerNorm is a launch past 32 images.  Gathers: the assembly, + 3 mq_move_rows with an index vector."""
    a, n = case.arch, case.n
    rows, sm, smg = n * a.tokens, ka["small_m"], ka["small_m_grouped"]
    if a.eva:       # (the assembly + one mq_rope_table per block; the gate's product rides in the GEMM's epilogue or in mq_glu_ln, a LayerNorm-family launch)
        return None, 1 + a.layers
    if a.pool != "cls":
        return None, 1
    head = 0 if n <= min(LN_ROWS, sm) else 1
    if rows <= min(LN_ROWS, sm):
        return 0, 1
    if rows <= sm:
        return 4 + head, 1
    fold = case.stream == 1 and ln_fold and rows > max(sm, smg)
    handed = fold and case.stats0 and case.knobs.get("assemble_stats", 1)
    ln = ((1 if handed else 2) if fold else 2) + 1 + (0 if n <= min(LN_ROWS, sm) else 1) + head
    strided = pool_strided and n <= max(sm, smg)
    return ln, 1 + (0 if strided else 3)


def _expect_text(case, nseq, rows, ka, ln_fold):
    """pre-LN text tower, 2 blocks: rows <= small_m: 4 LayerNorms; beyond: 2 + LN1 + LN2 on the pooled rows (a launch past 32) in the row-selected block;
    the head's LayerNorm is a launch with proj_b or past 32 sequences.  Gathers: the embedding, + 3 mq_move_rows when the last block is row-selected."""
    sm, smg = ka["small_m"], ka["small_m_grouped"]
    head = 1 if (case.siglip or nseq > min(LN_ROWS, sm)) else 0
    if case.stream == 1 and ln_fold and rows > max(sm, smg):
        return None, 4, head
    if rows <= min(LN_ROWS, sm):
        return 0 + head, 1, head
    if rows <= sm:
        return 4 + head, 1, head
    return 3 + (0 if nseq <= min(LN_ROWS, sm) else 1) + head, 4, head


def _expect_bert(case, pool, rows, nseq, ka):
    """post-LN, 2 blocks: the cast + 4 LayerNorms (rows <= 32: the cast + the last LayerNorm), + the head's cast; gathers: the embedding, + 3 when CLS pooling
    selects the last block's rows.  Rotary / gated encoders: not derived."""
    if case.kind == "rope":     # (block_post_ln whatever the rows: the cast + 4 LayerNorms; the embedding + mq_rope and mq_glu in either block; no row selection)
        return 5, 1 + 2 * case.arch.layers
    ln = (2 if rows <= min(LN_ROWS, ka["small_m"]) else 5) + (1 if case.head else 0)
    sel = pool == "cls" and T.selects_last(rows, nseq, ka["small_m"])
    return ln, 1 + (3 if sel else 0)


def _assert_launches(what, case, counts, ln, gather):
    print(f"TOWER_LAUNCHES tower={what} case={case.id} gemm={counts[0]} layernorm={counts[1]} attention={counts[2]} gather={counts[3]} pool={counts[4]} (implied: layernorm {ln}, gather {gather})")
    if ln is not None:
        assert counts[1] == ln, f"LayerNorm family: {counts[1]} launches, the branch the case names implies {ln}"
    if gather is not None:
        assert counts[3] == gather, f"gather family: {counts[3]} launches, the branch the case names implies {gather}"


def _s():
    return torch.cuda.current_stream().cuda_stream


def _al(v):
    return (v + 255) // 256 * 256


def _build(key, make):
    """the engine's tower of a case, built on the fp32 stream without the load-time calibration runs (the calls below set residual_stream themselves)"""
    if key not in _towers:
        was = os.environ.get("MARQO_AMD_RESIDUAL_STREAM")
        os.environ["MARQO_AMD_RESIDUAL_STREAM"] = "fp32"
        try:
            _towers[key] = make()
        finally:
            if was is None:
                del os.environ["MARQO_AMD_RESIDUAL_STREAM"]
            else:
                os.environ["MARQO_AMD_RESIDUAL_STREAM"] = was
    return _towers[key]


def _knob_args():
    return dict(small_m=knobs.get("small_m"), small_m_grouped=knobs.get("small_m_grouped"))


class _Buffers:
    """a guarded d_out [n, D] and a workspace of exactly `need` bytes with a sentinel region behind it"""

    def __init__(self, n, D, need, fill):
        self.n, self.D, self.need, self.fill = n, D, need, fill
        self.rb = D * 4
        self.buf = torch.full(((n + 2 * GUARD_ROWS) * self.rb,), SENTINEL, dtype=torch.uint8, device=DEV)
        self.out = self.buf[GUARD_ROWS * self.rb:(GUARD_ROWS + n) * self.rb].view(torch.float32).view(n, D)
        self.ws = torch.full((need + 4096,), fill, dtype=torch.uint8, device=DEV)
        assert self.ws.data_ptr() % 256 == 0 and self.out.data_ptr() % 16 == 0

    def check(self, short):
        g = GUARD_ROWS * self.rb
        assert bool((self.buf[:g] == SENTINEL).all()) and bool((self.buf[g + self.n * self.rb:] == SENTINEL).all()), "a guard row of d_out was written"
        assert bool((self.ws[self.need:] == self.fill).all()), "the workspace was written past *_workspace_bytes"
        if short:
            assert bool((self.buf == SENTINEL).all()) and bool((self.ws == self.fill).all()), "a refused call wrote to d_out or to the workspace"

    def stream(self, rows, W, bf16):
        if bf16:
            return self.ws[:rows * W * 2].view(torch.bfloat16).view(rows, W)
        return self.ws[:rows * W * 4].view(torch.float32).view(rows, W)


def _line(tower, case, n, view, r, worst):
    print(f"TOWER_RATIO tower={tower} case={case.id} n={n} view={view} ratio={r['ratio']:.3f} (row {r['row']} col {r['col']}: l2 {r['l2']:.3f} linf {r['linf']:.3f})")
    key = view.split("/")[0]
    worst[key] = max(worst.get(key, 0.0), r["ratio"])


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _profiled(lib, call):
    L.check(lib.mq_profile_collect(None, None, None), "mq_profile_collect")
    L.check(lib.mq_profile_enable(1), "mq_profile_enable")
    try:
        call()
        torch.cuda.synchronize()
        n = (C.c_int64 * L.MQ_PROF_FAMILIES)()
        L.check(lib.mq_profile_collect(None, n, None), "mq_profile_collect")
        return list(n)
    finally:
        lib.mq_profile_enable(0)


# ---- the image tower -----------------------------------------------------------------------------------------------------------------------

class _Vit:
    def __init__(self, case):
        from marqo_amd.engine.towers import VitTower
        self.case, self.lib, a = case, L.load(), case.arch
        self.tower = _build(("v", case.id), lambda: VitTower(a, case.sd(), DEV))
        if case.proj_b and not self.tower.w.proj_b:
            self.tower.w.proj_b = self.tower._h.f32(case.proj_bias())
        if case.map_proj and not self.tower.w.proj_w:
            self.tower.w.proj_w = self.tower._h.bf16(case.map_proj_w())
        self.T, self.W, self.D = a.tokens, a.width, case.out_dim
        self.rows = case.n * self.T
        self.u8 = case.images().to(DEV).contiguous()
        from oracle import towers as O
        self.f32 = O.preprocess_u8_exact_size(case.images()).to(DEV).contiguous()

    def cfg(self, layers):
        cfg = L.VitCfg.from_buffer_copy(self.tower.cfg)
        cfg.enc.layers, cfg.enc.residual_stream, cfg.out_dim = layers, self.case.stream, self.D
        return cfg

    def redo_head(self, b, normalize):
        """the tiled class-token head again from the slice: mq_cls_rows + mq_layernorm_ex by row index + mq_gemm_bf16 (+ mq_l2_normalize) must give d_out"""
        lib, w, n, W, D, a = self.lib, self.tower.w, self.case.n, self.W, self.D, self.case.arch
        idx = torch.empty(n, dtype=torch.int32, device=DEV)
        L.check(lib.mq_cls_rows(idx.data_ptr(), n, self.T, _s()), "mq_cls_rows")
        c16 = torch.empty(n, W, dtype=torch.bfloat16, device=DEV)
        again = torch.empty(n, D, dtype=torch.float32, device=DEV)
        L.check(lib.mq_layernorm_ex(b.ws.data_ptr(), 1 if self.case.stream == 1 else 0, idx.data_ptr(), w.ln_post_g, w.ln_post_b, c16.data_ptr(), None, n, W, a.ln_eps, _s()),
                "mq_layernorm_ex")
        L.check(lib.mq_gemm_bf16(c16.data_ptr(), W, w.proj_w, W, w.proj_b, None, again.data_ptr(), D, n, D, W, L.MQ_EPI_OUT_F32 | (L.MQ_EPI_BIAS if w.proj_b else 0), _s()),
                "mq_gemm_bf16")
        if normalize:
            L.check(lib.mq_l2_normalize(again.data_ptr(), again.data_ptr(), n, D, _s()), "mq_l2_normalize")
        torch.cuda.synchronize()
        if not _same_bits(again, b.out):
            pytest.fail(f"mq_layernorm_ex + mq_gemm_bf16 on the class-token rows of the first slice do not reproduce d_out of mq_encode_image: {LAYOUT}")

    def plan(self, cfg, n):
        """vit_plan restated -> (off_stats0, total)"""
        a, W, T = self.case.arch, self.W, self.T
        rows, npt = n * T, (a.image_size // a.patch_size) ** 2
        Kp = (3 * a.patch_size ** 2 + 63) // 64 * 64
        off = _al(rows * W * 4)
        off = _al(off) + n * 4
        off = _al(off) + n * W * 2
        off_stats0 = _al(off)
        off = off_stats0 + rows * 8
        mapped = a.pool in ("map", "query")
        if mapped:
            for b in (n * W * 4, n * W * 2, n * cfg.map_mlp_dim * 2):
                off = _al(off) + b
        off_enc = _al(off)
        enc = self.lib.mq_encoder_workspace_bytes(C.byref(cfg.enc), rows, n)
        if mapped:
            enc = max(enc, _al(_al(rows * W * 2) + rows * 2 * W * 2))
        patches = _al(_al(n * npt * Kp * 2) + n * npt * W * 4)
        return off_stats0, off_enc + max(enc, patches)

    def run(self, layers, normalize, kind="u8", fill=0xFF, short=0, px=None):
        cfg, n = self.cfg(layers), self.case.n
        need = self.lib.mq_vit_workspace_bytes(C.byref(cfg), n)
        self.off_stats0, total = self.plan(cfg, n)
        if total != need:
            pytest.fail(f"vit_plan restated gives {total} bytes, mq_vit_workspace_bytes {need}: {LAYOUT}")
        b = _Buffers(n, self.D, need, fill)
        px = px if px is not None else (self.u8 if kind == "u8" else self.f32)
        fn = self.lib.mq_encode_image_u8 if kind == "u8" else self.lib.mq_encode_image_f32
        torch.cuda.synchronize()
        rc = fn(C.byref(cfg), C.byref(self.tower.w), px.data_ptr(), n, b.out.data_ptr(), normalize, b.ws.data_ptr(), need - short, _s())
        torch.cuda.synchronize()
        b.check(short)
        return rc, b


@pytest.mark.parametrize("idx", range(len(VCASES)), ids=[c.id for c in VCASES])
def test_image_pass_against_float64(idx):
    case = _vcase(idx)
    ka = _knob_args()
    worst = {}
    with tuned(**case.knobs):
        v = _Vit(case)
        bf16 = case.stream == 1
        layers = case.arch.layers
        ln, gather = _expect_vit(case, ka, knobs.get("ln_fold"), knobs.get("pool_strided"))
        _assert_launches("image", case, _profiled(v.lib, lambda: v.run(layers, 0)), ln, gather)
        tiled_head = case.arch.pool == "cls" and not case.arch.eva and case.n > min(LN_ROWS, ka["small_m"])     # (held by the launch count above)
        assert tiled_head == (case.head == "tiled"), "the case's batch does not take the head its id names"
        for nl, kind in ((layers, "u8"), (layers, "f32"), (1, "u8")):
            name = f"mq_encode_image_{kind}"
            ref = T.vit_reference(case, DEV, nl, kind, images=v.f32 if kind == "f32" else None, ln_fold=knobs.get("ln_fold"), **ka)
            for normalize in (0, 1):
                rc, b = v.run(nl, normalize, kind)
                L.check(rc, name)
                if tiled_head:
                    v.redo_head(b, normalize)
                x, out = b.stream(v.rows, v.W, bf16).clone(), b.out.clone()
                rc2, b2 = v.run(nl, normalize, kind, fill=0x3C)
                L.check(rc2, name)
                assert _same_bits(x, b2.stream(v.rows, v.W, bf16)) and _same_bits(out, b2.out), "the same call on a workspace of 0xFF and of 0x3C bytes: other bits"
                assert bool(torch.isfinite(x.float()).all()) and bool(torch.isfinite(out).all())
                rc3, _ = v.run(nl, normalize, kind, short=1)
                assert rc3 == MQ_ERR_WORKSPACE, f"a workspace one byte short: rc {rc3}"
                tag = ("stream" if nl == layers else "first") if kind == "u8" else "f32in"
                _line("image", case, case.n, f"{tag}/stream/l2={normalize}" if kind == "f32" else f"{tag}/l2={normalize}",
                      E.row_ratio(x.double(), ref.ex_stream, ref.mo_stream), worst)
                _line("image", case, case.n, f"{'f32in' if kind == 'f32' else 'out'}/out/layers={nl}/l2={normalize}", E.row_ratio(out, ref.ex.out[normalize], ref.mo.out[normalize]),
                      worst)
        if case.stats0 or "assemble_stats" in case.knobs:
            # the assembled rows (a call of no blocks), then the full call's stats0 region against their float64 statistics
            rc, b0 = v.run(0, 0)
            L.check(rc, "mq_encode_image_u8")
            x0 = b0.stream(v.rows, v.W, True).clone()
            r0 = T.vit_reference(case, DEV, 0, "u8", **ka)
            _line("image", case, case.n, "x0", E.row_ratio(x0.double(), r0.ex.x0, r0.mo.x0), worst)
            lib = v.lib
            holder = {}
            counts = _profiled(lib, lambda: holder.update(r=v.run(layers, 0)))
            with tuned(assemble_stats=0):
                counts_off = _profiled(lib, lambda: v.run(layers, 0))
            print(f"TOWER_STATS_PASS case={case.id} layernorm-family {counts[1]} (assemble_stats=0: {counts_off[1]})")
            if case.stats0:
                assert counts[1] == counts_off[1] - 1, "the stats0 hand-in was meant to be reached: the statistics pass was launched all the same"
                st = holder["r"][1].ws[v.off_stats0:v.off_stats0 + v.rows * 8].view(torch.float32).view(v.rows, 2)
                mu, rstd, c, rho = R.stats_budget(x0, case.arch.ln_eps)
                rm, rr = R.ratio(st[:, 0], mu, c), R.ratio(st[:, 1], rstd, rho * rstd)
                print(f"TOWER_STATS0 case={case.id} mean={rm:.4f} rstd={rr:.4f}")
                from tests.test_rowops_gpu import MARGIN as ROW_MARGIN
                assert rm <= ROW_MARGIN and rr <= ROW_MARGIN
            else:
                assert counts[1] == counts_off[1], "assemble_stats = 0 and the hand-in was taken all the same"
    print(f"TOWER_WORST tower=image case={case.id}: " + " ".join(f"{k} {x:.3f}" for k, x in worst.items()))
    assert max(worst.values()) <= MARGIN, worst


def test_image_batch_permutation_is_bitwise():
    case = _vcase(next(i for i, c in enumerate(VCASES) if "f32[select_last" in c.id))
    with tuned(small_m=0, small_m_grouped=0):
        v = _Vit(case)
        perm = torch.randperm(case.n, generator=torch.Generator().manual_seed(5)).to(DEV)
        rc, b = v.run(case.arch.layers, 1)
        L.check(rc, "mq_encode_image_u8")
        rc, bp = v.run(case.arch.layers, 1, px=v.u8[perm].contiguous())
        L.check(rc, "mq_encode_image_u8")
    assert _same_bits(b.out[perm], bp.out), "a permuted batch of images does not return the permuted rows bit for bit"


# ---- the packed text towers ------------------------------------------------------------------------------------------------------------------

class _Packed:
    def __init__(self, tower, ids, lens, D):
        self.lib, self.tower, self.lens = L.load(), tower, list(lens)
        self.W, self.D = tower.arch.width, D
        self.rows, self.nseq = sum(lens), len(lens)
        self.d_ids = ids.to(torch.int32).to(DEV).contiguous()
        self.cu_h = A.cu_seqlens(lens)
        self.d_cu = self.cu_h.to(DEV)

    def plan(self, cfg):
        off = _al(self.rows * self.W * 4)
        off = _al(off + self.nseq * 4)
        off = _al(off + self.nseq * self.W * 4)
        return off + self.lib.mq_encoder_workspace_bytes(C.byref(cfg.enc), self.rows, self.nseq)


class _Text(_Packed):
    def __init__(self, case):
        from marqo_amd.engine.towers import ClipTextTower
        tower = _build(("t", case.siglip, case.seed), lambda: ClipTextTower(case.arch, case.sd(), DEV))
        super().__init__(tower, case.ids(), case.lens, case.arch.out_dim)
        self.case = case
        pr = case.pool_rows()
        self.d_pool = pr.to(torch.int32).to(DEV) if pr is not None else None

    def run(self, layers, normalize, fill=0xFF, short=0):
        cfg = L.ClipTextCfg.from_buffer_copy(self.tower.cfg)
        cfg.enc.layers, cfg.enc.residual_stream, cfg.cls_pos = layers, self.case.stream, self.case.cls_pos
        self.cfg_used = cfg
        need = self.lib.mq_clip_text_workspace_bytes(C.byref(cfg), self.rows, self.nseq)
        if self.plan(cfg) != need:
            pytest.fail(f"text_plan restated gives {self.plan(cfg)} bytes, mq_clip_text_workspace_bytes {need}: {LAYOUT}")
        b = _Buffers(self.nseq, self.D, need, fill)
        torch.cuda.synchronize()
        rc = self.lib.mq_encode_clip_text(C.byref(cfg), C.byref(self.tower.w), self.d_ids.data_ptr(), self.d_cu.data_ptr(), self.cu_h.data_ptr(), self.nseq,
                                          self.d_pool.data_ptr() if self.d_pool is not None else None, b.out.data_ptr(), normalize, b.ws.data_ptr(), need - short, _s())
        torch.cuda.synchronize()
        b.check(short)
        return rc, b

    def redo_head(self, b, normalize):
        """mq_layernorm_ex on the pooled rows of the slice + mq_gemm_bf16 (+ L2): the library's own head, from the bytes this test reads as the stream"""
        lib, w, cfg, W, D, n = self.lib, self.tower.w, self.cfg_used, self.W, self.D, self.nseq
        idx = self.d_pool
        if idx is None:
            idx = torch.empty(n, dtype=torch.int32, device=DEV)
            L.check(lib.mq_last_rows(self.d_cu.data_ptr(), idx.data_ptr(), n, _s()), "mq_last_rows")
        pooled = torch.empty(n, W, dtype=torch.bfloat16, device=DEV)
        again = torch.zeros(n, D, dtype=torch.float32, device=DEV)
        L.check(lib.mq_layernorm_ex(b.ws.data_ptr(), 1 if self.case.stream == 1 else 0, idx.data_ptr(), w.ln_final_g, w.ln_final_b, pooled.data_ptr(), None, n, W,
                                    cfg.enc.ln_eps, _s()), "mq_layernorm_ex")
        if w.proj_b:
            flags = L.MQ_EPI_BIAS | L.MQ_EPI_RESIDUAL | L.MQ_EPI_OUT_F32
            L.check(lib.mq_gemm_bf16(pooled.data_ptr(), W, w.proj_w, W, w.proj_b, again.data_ptr(), again.data_ptr(), D, n, D, W, flags, _s()), "mq_gemm_bf16")
        else:
            L.check(lib.mq_gemm_bf16(pooled.data_ptr(), W, w.proj_w, W, None, None, again.data_ptr(), D, n, D, W, L.MQ_EPI_OUT_F32, _s()), "mq_gemm_bf16")
        if normalize:
            L.check(lib.mq_l2_normalize(again.data_ptr(), again.data_ptr(), n, D, _s()), "mq_l2_normalize")
        torch.cuda.synchronize()
        if not _same_bits(again, b.out):
            pytest.fail(f"mq_layernorm_ex + mq_gemm_bf16 on the first slice of the workspace do not reproduce d_out of mq_encode_clip_text: {LAYOUT}")


@pytest.mark.parametrize("case", TCASES, ids=lambda c: c.id)
def test_clip_text_pass_against_float64(case):
    ka = _knob_args()
    t = _Text(case)
    worst = {}
    bf16 = case.stream == 1
    layers = case.arch.layers
    ln, gather, head_ln = _expect_text(case, t.nseq, t.rows, ka, knobs.get("ln_fold"))
    _assert_launches("clip_text", case, _profiled(t.lib, lambda: t.run(layers, 0)), ln, gather)
    tiled_head = bool(head_ln)      # (proj_b, or past the skinny kernel's fused-LayerNorm rows: mq_layernorm_ex + tiled GEMM — held by the launch count above)
    for nl in (layers, 1):
        ref = T.text_reference(case, DEV, nl, ln_fold=knobs.get("ln_fold"), **ka)
        for normalize in (0, 1):
            rc, b = t.run(nl, normalize)
            L.check(rc, "mq_encode_clip_text")
            if tiled_head:
                t.redo_head(b, normalize)
            x, out = b.stream(t.rows, t.W, bf16).clone(), b.out.clone()
            rc2, b2 = t.run(nl, normalize, fill=0x3C)
            L.check(rc2, "mq_encode_clip_text")
            assert _same_bits(x, b2.stream(t.rows, t.W, bf16)) and _same_bits(out, b2.out), "the same call on a workspace of 0xFF and of 0x3C bytes: other bits"
            assert bool(torch.isfinite(x.float()).all()) and bool(torch.isfinite(out).all())
            rc3, _ = t.run(nl, normalize, short=1)
            assert rc3 == MQ_ERR_WORKSPACE, f"a workspace one byte short: rc {rc3}"
            tag = "stream" if nl == layers else "first"
            _line("clip_text", case, t.nseq, f"{tag}/l2={normalize}", E.row_ratio(x.double(), ref.ex_stream, ref.mo_stream), worst)
            _line("clip_text", case, t.nseq, f"out/layers={nl}/l2={normalize}", E.row_ratio(out, ref.ex.out[normalize], ref.mo.out[normalize]), worst)
    print(f"TOWER_WORST tower=clip_text case={case.id}: " + " ".join(f"{k} {x:.3f}" for k, x in worst.items()))
    assert max(worst.values()) <= MARGIN, worst


class _Bert(_Packed):
    def __init__(self, case):
        from marqo_amd.engine.towers import BertTower, HfClipTextTower, MclipTextTower
        a, head = case.arch, case.head_tensors()

        def make():
            sd = case.enc_sd()
            if head is None:
                return BertTower(a, sd, DEV)
            if "w2" not in head:
                full = {"transformer." + k: v for k, v in sd.items()}
                full["LinearTransformation.weight"], full["LinearTransformation.bias"] = head["w1"], head["b1"]
                return MclipTextTower(a, T.D_, full, DEV)
            full = {"text.transformer." + k: v for k, v in sd.items()}
            full["text.proj.0.weight"], full["text.proj.2.weight"] = head["w1"], head["w2"]
            return HfClipTextTower(types.SimpleNamespace(bert=a, out_dim=T.D_, proj_hidden=head["w1"].shape[0], ctx=a.max_pos, pad_id=1), full, DEV)

        tower = _build(("b", case.kind, case.head, case.seed), make)
        super().__init__(tower, case.ids(), case.lens, T.D_ if head is not None else a.width)
        self.case = case

    def run(self, layers, pool, normalize, fill=0xFF, short=0):
        cfg = L.BertCfg.from_buffer_copy(self.tower.cfg)
        cfg.enc.layers, cfg.enc.residual_stream = layers, self.case.stream
        cfg.pool = L.MQ_POOL_MEAN if pool == "mean" else L.MQ_POOL_CLS
        w = type(self.tower.w).from_buffer_copy(self.tower.w)
        if not self.case.type_emb:
            w.type_emb = None
        need = self.lib.mq_bert_workspace_bytes(C.byref(cfg), self.rows, self.nseq)
        if self.plan(cfg) != need:
            pytest.fail(f"text_plan restated gives {self.plan(cfg)} bytes, mq_bert_workspace_bytes {need}: {LAYOUT}")
        b = _Buffers(self.nseq, self.D, need, fill)
        torch.cuda.synchronize()
        rc = self.lib.mq_encode_bert(C.byref(cfg), C.byref(w), self.d_ids.data_ptr(), self.d_cu.data_ptr(), self.cu_h.data_ptr(), self.nseq, b.out.data_ptr(),
                                     normalize, b.ws.data_ptr(), need - short, _s())
        torch.cuda.synchronize()
        b.check(short)
        if rc == 0 and not short and self.case.head is None:
            again = torch.empty(self.nseq, self.W, dtype=torch.float32, device=DEV)
            L.check(self.lib.mq_pool(b.ws.data_ptr(), self.d_cu.data_ptr(), self.nseq, again.data_ptr(), self.W, cfg.pool, normalize, _s()), "mq_pool")
            torch.cuda.synchronize()
            if not _same_bits(again, b.out):
                pytest.fail(f"mq_pool on the first slice of the workspace does not reproduce d_out of mq_encode_bert: {LAYOUT}")
        elif rc == 0 and not short:
            self.redo_head(b, cfg, w, normalize)
        return rc, b

    def redo_head(self, b, cfg, w, normalize):
        """the projection head again from the slice: mq_pool, the bf16 cast (round to nearest even, as mq_cast_bf16 stores) and mq_gemm_bf16 must give d_out"""
        lib, n, W, D = self.lib, self.nseq, self.W, self.D
        pooled = torch.empty(n, W, dtype=torch.float32, device=DEV)
        L.check(lib.mq_pool(b.ws.data_ptr(), self.d_cu.data_ptr(), n, pooled.data_ptr(), W, cfg.pool, 0, _s()), "mq_pool")
        torch.cuda.synchronize()
        pb = pooled.to(torch.bfloat16).contiguous()
        again = torch.empty(n, D, dtype=torch.float32, device=DEV)
        if not w.proj2_w:
            L.check(lib.mq_gemm_bf16(pb.data_ptr(), W, w.proj1_w, W, w.proj1_b, None, again.data_ptr(), D, n, D, W, L.MQ_EPI_BIAS | L.MQ_EPI_OUT_F32, _s()), "mq_gemm_bf16")
        else:
            Hp = cfg.proj_hidden
            h1 = torch.empty(n, Hp, dtype=torch.bfloat16, device=DEV)
            L.check(lib.mq_gemm_bf16(pb.data_ptr(), W, w.proj1_w, W, w.proj1_b, None, h1.data_ptr(), Hp, n, Hp, W, L.MQ_EPI_BIAS | L.MQ_EPI_GELU, _s()), "mq_gemm_bf16")
            L.check(lib.mq_gemm_bf16(h1.data_ptr(), Hp, w.proj2_w, Hp, None, None, again.data_ptr(), D, n, D, Hp, L.MQ_EPI_OUT_F32, _s()), "mq_gemm_bf16")
        if normalize:
            L.check(lib.mq_l2_normalize(again.data_ptr(), again.data_ptr(), n, D, _s()), "mq_l2_normalize")
        torch.cuda.synchronize()
        if not _same_bits(again, b.out):
            pytest.fail(f"mq_pool + cast + mq_gemm_bf16 on the first slice of the workspace do not reproduce d_out of mq_encode_bert: {LAYOUT}")


@pytest.mark.parametrize("case", BCASES, ids=lambda c: c.id)
def test_bert_pass_against_float64(case):
    ka = _knob_args()
    t = _Bert(case)
    worst = {}
    layers = case.arch.layers
    for pool in ("mean", "cls"):
        ln, gather = _expect_bert(case, pool, t.rows, t.nseq, ka)
        _assert_launches("bert", case, _profiled(t.lib, lambda: t.run(layers, pool, 0)), ln, gather)
        for nl in (layers, 1):
            ref = T.bert_reference(case, pool, DEV, nl, small_m=ka["small_m"])
            for normalize in (0, 1):
                rc, b = t.run(nl, pool, normalize)
                L.check(rc, "mq_encode_bert")
                x, out = b.stream(t.rows, t.W, False).clone(), b.out.clone()
                rc2, b2 = t.run(nl, pool, normalize, fill=0x3C)
                L.check(rc2, "mq_encode_bert")
                assert _same_bits(x, b2.stream(t.rows, t.W, False)) and _same_bits(out, b2.out), "the same call on a workspace of 0xFF and of 0x3C bytes: other bits"
                assert bool(torch.isfinite(x).all()) and bool(torch.isfinite(out).all())
                rc3, _ = t.run(nl, pool, normalize, short=1)
                assert rc3 == MQ_ERR_WORKSPACE, f"a workspace one byte short: rc {rc3}"
                tag = "stream" if nl == layers else "first"
                _line("bert", case, t.nseq, f"{tag}/{pool}/l2={normalize}", E.row_ratio(x.double(), ref.ex_stream, ref.mo_stream), worst)
                _line("bert", case, t.nseq, f"out/{pool}/layers={nl}/l2={normalize}", E.row_ratio(out, ref.ex.out[normalize], ref.mo.out[normalize]), worst)
    print(f"TOWER_WORST tower=bert case={case.id}: " + " ".join(f"{k} {x:.3f}" for k, x in worst.items()))
    assert max(worst.values()) <= MARGIN, worst

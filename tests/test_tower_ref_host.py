"""tests/tower_ref.py on the CPU: is the reference the towers' formula, is the bar usable, and what would a defect of the orchestration measure.

1. tower_ref's `exact` passes against the fp32 restatements of oracle/towers.py — vit_forward (class token; the CLIPA avg form without ln_pre),
   siglip_vit_forward (MAP; with the final projection: the oracle's pooled row times the matrix), coca_vit_forward (QUERY), eva_vit_forward, clip_text_forward, siglip_text_forward, hf_encode (BERT and MPNet, mean / cls), new_model_encode (rotary + gated MLP), mclip_text_forward (one Linear)
   and hf_clip_text_forward (the MLP head; with CLS pooling the oracle's encoder row through the same head) — on the cases' checkpoints with the matrices rounded to bf16 (what the loaders store, and what `exact` reads):
   max |exact - oracle| <= 1e-4 max |oracle|, fp32 agreement for passes of a few thousand fp32 operations per element.  The oracle pools CLIP text at
   argmax(id): TCase.ids() ends every sequence in the largest id.  Not pinned (no oracle restatement takes them): the caller's pool rows in the middle of
   the sequences, cls_pos on a plain causal tower, proj_b on the class-token image head (pinned as oracle + bias), a BERT without type table (pinned with
   a zero table).
2. model(hist = 1) against model(hist = 0) on every case: x0, the stream after all blocks and the output rows with and without L2 stay within MARGIN
   (tests/test_patch_attn_gpu.py) of each other's yardstick, and no row raises ZeroYardstick.  Printed as TOWER_HIST.
3. One deliberate defect at a time through the model (tower_ref.MUTANTS), printed as TOWER_MUTANT ... ratio= (the worst view of stream and output rows);
   each must leave the bar, or is named in tower_ref.INVISIBLE and shown to be seen by another check.

Measured (TOWER_HIST, worst over the cases and views, bar 4.0):  image 1.91   clip_text 1.41   bert 1.74
Measured (TOWER_MUTANT, worst view, bar 4.0):
  image   class token in the last row 441   position behind ln_pre 131   mean / std of two channels swapped 60   patch as (y, x, c) 556
          head LayerNorm on row i T + 1: 444 (n = 20), 814 (n = 3)   pooled last block on row i T + 1: 155   L2 in front of the projection 248
          proj_b dropped 167   MAP without its residual 920   AVG with the class token 37   QUERY with the tower's heads 111
  text    pooled at len - 2: 782   cls_pos ignored 559   proj_b dropped 65   L2 in front of the projection 573
  bert    mean over max_len 1689   type row 0 not added 4621   CLS pooling on the last row 1235   the MLP head's GELU dropped 417
Invisible to this bar: stats0 of the neighbouring row, 2.2 — behind ln_pre every row has all but the same (mean, rstd).  Held instead by the check the GPU file
makes on the stats0 region itself: the neighbour's statistics lie 64536 budgets of tests/rowops_ref.py from the row's own (asserted here).  Every norm's eps
times ten is invisible as in tests/test_packed_text_ref_host.py.
"""
import pytest
import torch

from oracle import towers as O
from tests import encoder_ref as E
from tests import tower_ref as T
from tests.test_patch_attn_gpu import MARGIN

_TABLES = ("positional_embedding", "pos_embed", "token_embedding", "word_embeddings", "position_embeddings", "token_type", "query", "latent",
           "class_embedding", "cls_emb")


def _rounded(sd):
    """the checkpoint with every weight MATRIX rounded to bf16 (tables and vectors stay fp32, as the loaders keep them)"""
    return {k: (v.float().to(torch.bfloat16).float() if v.dim() >= 2 and not any(t in k for t in _TABLES) else v) for k, v in sd.items()}


def _close(a, b, what):
    a, b = a.double(), b.double()
    err, ref = float((a - b).abs().max()), float(b.abs().max())
    print(f"TOWER_PIN {what}: max |exact - oracle| = {err:.2e} (max |oracle| {ref:.2e})")
    assert err <= 1e-4 * ref, what


VCASES, TCASES, BCASES = T.vit_cases(), T.text_cases(), T.bert_cases()
_PIN_V = [c for c in VCASES if c.n <= 3 and c.stream == 2]


@pytest.mark.parametrize("case", _PIN_V, ids=lambda c: c.id)
def test_vit_exact_is_the_oracle(case):
    a = case.arch
    sd = _rounded(case.sd())
    ops = T.vit_ops(a, sd, case.proj_bias(), case.map_proj_w())
    img = case.images()
    px = O.preprocess_u8_exact_size(img)
    for normalize in (0, 1):
        if a.eva:
            ref = O.eva_vit_forward(sd, O.EvaVitConfig(a.image_size, a.patch_size, a.width, a.layers, a.heads, a.mlp_dim, a.out_dim, ln_eps=a.ln_eps), px, bool(normalize))
        elif a.pool == "map":
            ref = O.siglip_vit_forward(sd, O.SiglipVitConfig(a.image_size, a.patch_size, a.width, a.layers, a.heads, a.mlp_dim, a.ln_eps), px,
                                       bool(normalize) and not case.map_proj)
            if case.map_proj:       # the oracle's pooled row through the final projection (bf16-rounded, as the loader stores a matrix)
                ref = ref @ case.map_proj_w().to(torch.bfloat16).float().t()
                ref = O.l2_normalize_clip(ref) if normalize else ref
        elif a.pool == "query":
            cfg = O.CocaVitConfig(a.image_size, a.patch_size, a.width, a.layers, a.heads, a.mlp_dim, a.out_dim, pool_heads=a.pool_heads, n_queries=3)
            ref = O.coca_vit_forward(sd, cfg, px, bool(normalize))
        else:
            cfg = O.VitConfig(a.image_size, a.patch_size, a.width, a.layers, a.heads, a.mlp_dim, a.out_dim, a.quick_gelu, a.ln_eps, a.ln_pre, a.pool)
            ref = O.vit_forward(sd, cfg, px, False)
            if case.proj_b:
                ref = ref + case.proj_bias()
            ref = O.l2_normalize_clip(ref) if normalize else ref
        _close(T.vit_exact(ops, img).out[normalize], ref, f"{case.id} l2={normalize} u8")
        _close(T.vit_exact(ops, px, "f32").out[normalize], ref, f"{case.id} l2={normalize} f32")


@pytest.mark.parametrize("case", [c for c in TCASES if c.pool == "last" and not c.cls_pos and len(c.lens) <= 6], ids=lambda c: c.id)
def test_text_exact_is_the_oracle(case):
    a = case.arch
    sd = _rounded(case.sd())
    ops = T.text_ops(a, sd)
    ids = case.ids()
    for normalize in (0, 1):
        got = T.text_exact(ops, ids, case.lens).out[normalize]
        r0 = 0
        for i, ln in enumerate(case.lens):
            row = ids[r0:r0 + ln][None]
            if case.siglip:
                ref = O.siglip_text_forward(sd, O.SiglipTextConfig(a.vocab, a.ctx, a.width, a.layers, a.heads, a.mlp_dim, a.out_dim, a.ln_eps), row, bool(normalize))
            else:
                ref = O.clip_text_forward(sd, O.ClipTextConfig(a.vocab, a.ctx, a.width, a.layers, a.heads, a.mlp_dim, a.out_dim), row, bool(normalize))
            _close(got[i:i + 1], ref, f"{case.id} seq {i} l2={normalize}")
            r0 += ln


@pytest.mark.parametrize("case", BCASES, ids=lambda c: c.id)
def test_bert_exact_is_the_oracle(case):
    a = case.arch
    sd = _rounded(case.enc_sd())
    if not case.type_emb:
        sd["embeddings.token_type_embeddings.weight"] = torch.zeros_like(sd["embeddings.token_type_embeddings.weight"])
    head = case.head_tensors()
    if head is not None:
        head = {k: (v.to(torch.bfloat16).float() if (v is not None and v.dim() == 2) else v) for k, v in head.items()}
    ops = T.bert_ops(a, sd, head, True)
    ids = case.ids()
    for pool in ("mean", "cls"):
        cfg = O.BertConfig(a.vocab, a.max_pos, a.width, a.layers, a.heads, a.mlp_dim, a.ln_eps, pool, a.pos_offset)
        for normalize in (0, 1):
            got = T.bert_exact(ops, ids, case.lens, pool).out[normalize]
            r0 = 0
            for i, ln in enumerate(case.lens):
                row, mask = ids[r0:r0 + ln][None], torch.ones(1, ln, dtype=torch.int64)
                if case.kind == "rope":
                    ref = O.new_model_encode(sd, O.NewModelConfig(a.vocab, a.max_pos, a.width, a.layers, a.heads, a.mlp_dim, a.ln_eps, 10000.0, None, pool), row, mask,
                                             bool(normalize))
                elif head is None:
                    ref = O.hf_encode(sd, cfg, row, mask, bool(normalize))
                elif pool == "cls":     # the oracle's head restatements pool the mean: the CLS row of its encoder through the same head
                    last = O.bert_forward(sd, cfg, row, mask)[:, 0]
                    ref = (torch.nn.functional.linear(torch.nn.functional.gelu(torch.nn.functional.linear(last, head["w1"])), head["w2"]) if "w2" in head
                           else torch.nn.functional.linear(last, head["w1"], head["b1"]))
                    ref = O.l2_normalize_clip(ref) if normalize else ref
                elif "w2" in head:
                    full = {"text.transformer." + k: v for k, v in sd.items()}
                    full["text.proj.0.weight"], full["text.proj.2.weight"] = head["w1"], head["w2"]
                    ref = O.hf_clip_text_forward(full, cfg, row, 1, bool(normalize))
                else:
                    full = {"transformer." + k: v for k, v in sd.items()}
                    full["LinearTransformation.weight"], full["LinearTransformation.bias"] = head["w1"], head["b1"]
                    ref = O.mclip_text_forward(full, cfg, row, mask, bool(normalize))
                _close(got[i:i + 1], ref, f"{case.id} {pool} seq {i} l2={normalize}")
                r0 += ln


def _ratios(got: T.Ref, ref: T.Ref, stream_got=None):
    """worst row ratio per view of `got`'s model against `ref`'s yardstick (|ref.mo - ref.ex|)"""
    out = {}
    out["stream"] = E.row_ratio(got.mo_stream if stream_got is None else stream_got, ref.ex_stream, ref.mo_stream)["ratio"]
    for nz in (0, 1):
        out[f"out/l2={nz}"] = E.row_ratio(got.mo.out[nz], ref.ex.out[nz], ref.mo.out[nz])["ratio"]
    return out


def _refs(case, **kw):
    if isinstance(case, T.VCase):
        return [("u8", T.vit_reference(case, **kw))]
    if isinstance(case, T.TCase):
        return [("last" if case.pool == "last" else "middle", T.text_reference(case, **kw))]
    return [(p, T.bert_reference(case, p, **kw)) for p in ("mean", "cls")]


_worst_hist = {}


@pytest.mark.parametrize("case", VCASES + TCASES + BCASES, ids=lambda c: f"{type(c).__name__[0]}-{c.id}")
def test_second_history_stays_inside_the_bar(case):
    fam = type(case).__name__[0]
    for (name, r0), (_, r1) in zip(_refs(case), _refs(case, hist=1)):
        rs = _ratios(r1, r0)
        if fam == "V":      # the front end has a GEMM of its own
            rs["x0"] = E.row_ratio(r1.mo.x0, r0.ex.x0, r0.mo.x0)["ratio"]
        else:
            E.row_ratio(r0.mo.x0, r0.ex.x0, r0.mo.x0)      # (raises ZeroYardstick if a row of the front end is exact)
        print(f"TOWER_HIST tower={fam} case={case.id} view={name} " + " ".join(f"{k}={v:.3f}" for k, v in rs.items()))
        _worst_hist[fam] = max(_worst_hist.get(fam, 0.0), *rs.values())
        assert max(rs.values()) <= MARGIN, rs
    print(f"TOWER_HIST_WORST {_worst_hist}")


def _by_id(cases, frag):
    return next(c for c in cases if frag in c.id)


_MUT_CASES = [
    ("vit", "cls_last_row", "bf16-fold2[stats0"), ("vit", "pos_behind_ln_pre", "bf16-fold2[stats0"), ("vit", "swap_mean_std_channels", "bf16-fold2[stats0"),
    ("vit", "patch_yxc", "bf16-fold2[stats0"), ("vit", "head_row_plus1", "bf16-fold2[stats0"), ("vit", "pooled_block_row_plus1", "bf16-fold2[stats0"),
    ("vit", "stats0_neighbour", "bf16-fold2[stats0"), ("vit", "l2_before_proj", "bf16-fold2[stats0"), ("vit", "head_row_plus1", "cls-n3-f32[skinny]"),
    ("vit", "drop_proj_b", "cls-n3-f32-proj_b"), ("vit", "map_no_residual", "map-n3-f32"), ("vit", "avg_with_cls", "avg-n3-f32"),
    ("vit", "query_tower_heads", "query-n3-f32"),
    ("text", "pool_len_minus2", "causal-6len-f32[mq_last_rows"), ("text", "cls_pos_ignored", "cls_pos76"), ("text", "drop_proj_b", "siglip-proj_b-mask_none-f32"),
    ("text", "l2_before_proj", "causal-6len-f32[mq_last_rows"),
    ("bert", "mean_over_max_len", "packed217-f32[out_dim=0"), ("bert", "no_type_row0", "packed217-f32[out_dim=0"), ("bert", "cls_reads_last_row", "packed217-f32[out_dim=0"),
    ("bert", "head_no_gelu", "packed217-mlp64-head"),
]


@pytest.mark.parametrize("fam,kind,frag", _MUT_CASES, ids=[f"{f}-{k}-{g}" for f, k, g in _MUT_CASES])
def test_mutants_leave_the_bar(fam, kind, frag):
    assert kind in T.MUTANTS[fam]
    case = _by_id(dict(vit=VCASES, text=TCASES, bert=BCASES)[fam], frag)
    worst = 0.0
    for (name, good), (_, bad) in zip(_refs(case), _refs(case, mut=dict(kind=kind))):
        if fam == "bert" and kind == "cls_reads_last_row" and name != "cls":
            continue
        if fam == "bert" and kind == "mean_over_max_len" and name != "mean":
            continue
        rs = _ratios(bad, good)
        worst = max(worst, *rs.values())
        print(f"TOWER_MUTANT tower={fam} defect={kind} case={case.id} view={name} ratio={max(rs.values()):.1f} (" + " ".join(f"{k}={v:.1f}" for k, v in rs.items()) + ")")
    if kind in T.INVISIBLE:
        # the ratio bar does not see it; the check the GPU file makes on stats0 itself does: the neighbour's statistics against the row's own, in units of
        # the budget of tests/rowops_ref.py (what tests/test_rowops_gpu.py allows mq_row_stats)
        from tests import rowops_ref as R
        x0 = _refs(case)[0][1].mo.x0
        mu, rstd, c, rho = R.stats_budget(x0, case.arch.ln_eps)
        far = max(R.ratio(torch.roll(mu, -1), mu, c), R.ratio(torch.roll(rstd, -1), rstd, rho * rstd))
        print(f"TOWER_MUTANT tower={fam} defect={kind}: invisible to the ratio bar ({worst:.2f}); against the statistics' own budget {far:.0f}")
        assert worst <= MARGIN and far > 10 * MARGIN
        return
    assert worst > MARGIN, f"{kind}: the bar cannot see this defect (worst ratio {worst:.2f})"

"""The whole passes of LanguageBindVideoTower and LanguageBindAudioTower (engine/languagebind.py) with every row of the token stream held to the float64
reference of tests/languagebind_tower_ref.py.  Under test is the Python orchestration: mq_patchify_clip / mq_patchify_rect -> conv GEMM -> mq_vit_assemble,
per layer mq_temporal_embed_ln -> QKV GEMM -> mq_temporal_attention -> out-projection with the fp32 residual, in place on the stream between one-block
mq_encoder_forward calls, then mq_cls_rows -> mq_layernorm -> projection -> mq_avg_tokens -> mq_l2_normalize; for audio the rectangular grid and its
positions.  The kernels have their own files (tests/test_languagebind_gpu.py, tests/test_audio_gpu.py), which also keep the pooled cosine bar.

The engine is not touched: a subclass of each tower made here overrides `_tokens` and `_encoder` to clone the stream behind the front end and in front of
and behind every mq_encoder_forward call — for video the stream after every temporal sub-block and after every CLIP block.  Before any ratio is measured:
  - the capturing subclass returns the bits of the plain tower (else "no parity was measured");
  - one more call of the plain tower's own `_tokens` on im2col rows made here (mq_patchify_clip / `_patchify_f32`) gives the captured front-end stream;
  - the tail redone here from the captured last stream with library kernels (mq_cls_rows + mq_layernorm — whose bf16 rows are the `cls_ln` view —,
    mq_gemm_bf16, mq_avg_tokens, mq_l2_normalize) gives the tower's output, bit for bit.

Every case (languagebind_tower_ref.video_cases / audio_cases), normalize on and off:
  - the worst row of max(|got - exact|_2 / |model - exact|_2, |got - exact|_inf / |model - exact|_inf) <= MARGIN (tests/test_patch_attn_gpu.py) on the
    front end, the stream after every temporal sub-block and every block (audio: after all blocks, one call), the post_layernorm class rows and the pooled
    rows; no row skipped.  Printed as LB_RATIO tower=... case=... view=... ratio=... (row, col, l2, linf) and one LB_WORST line per case;
  - finite outputs; the same call twice: the same bits; normalize=False rows point where the unit rows point (1 - cos <= 1e-6); unit rows have norm 1;
  - the split case runs a batch of 3 clips with max_items_per_call = 2 set on the test's tower instance: every captured stream and the pooled rows
    equal the unsplit call's bit for bit.

Measured on an MI355X (worst LB_RATIO per view over the cases, both normalize settings; bar 4.0):
  video   front end 2.67 (T = 2, B = 1; 1.52 .. 2.67 over the cases)   after a temporal sub-block 1.40   after a block 1.58 (both T = 16, B = 2, layer 1)
          post_layernorm class rows 1.53   pooled rows 1.46 without / 1.50 with L2 (T = 3, B = 3)
  audio   front end 1.95   after all blocks 1.25   post_layernorm class rows 1.11   pooled rows 1.16 / 1.15
  LB_WORST per case (largest view): T1-B2 2.10   T2-B1 2.67   T3-B3 1.91   T8-B1 1.52   T16-B2 2.43   T3-B2-quick_gelu 1.91   T2-B2-P14 2.18   T3-B3-split2 1.91
                                    grid2x5-b1 1.95   grid2x5-b3 1.95   grid2x2-b2 1.95 — in every case the front end's view
  The front end is the largest view everywhere: mq_vit_assemble's LayerNorm is fp32 arithmetic (sums, rsqrt, affine: a few ulps) against a yardstick
  of one fp32 rounding of a float64 LayerNorm (half an ulp).  It stays inside the bar, so the model keeps the single rounding; behind the first bf16
  store the views measure 1.0 .. 1.6.  No rounding had to be added to `model`; every parity check in front of the ratios held on the first run.
Found by this file: nothing in the library.

What a defect of the orchestration would measure against this bar is in tests/test_languagebind_tower_ref_host.py (LB_MUTANT).
"""
import functools

import pytest
import torch

from marqo_amd import _lib as L
from tests import encoder_ref as E
from tests import languagebind_tower_ref as T
from tests.test_patch_attn_gpu import MARGIN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NO_PARITY = "no parity was measured"


def _max_frames():
    from marqo_amd.engine.languagebind import MAX_FRAMES
    return MAX_FRAMES


VCASES, ACASES = T.video_cases(), T.audio_cases()       # (ids; the MAX_FRAMES case is checked against the engine's constant below)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _cos_err(a, b):
    a, b = a.double(), b.double()
    return float((1 - (a * b).sum(-1) / (a.norm(dim=-1) * b.norm(dim=-1))).max())


def _capturing(base):
    class Capturing(base):
        """one record per `_forward` call: the stream behind the front end, in front of and behind every mq_encoder_forward call"""
        calls = None

        def _tokens(self, patches, frames):
            x = super()._tokens(patches, frames)
            if self.calls is not None:
                self.calls.append(dict(x0=x.clone(), before=[], after=[]))
            return x

        def _encoder(self, x, frames, ws, first=0):
            if self.calls is not None:
                self.calls[-1]["before"].append(x.clone())
            super()._encoder(x, frames, ws, first=first)
            if self.calls is not None:
                self.calls[-1]["after"].append(x.clone())

    return Capturing


@functools.lru_cache(maxsize=None)
def _setup(kind, idx):
    """(case, plain tower, capturing tower, input on the device, exact Pass, model Pass): built and computed once per case, never changed"""
    from marqo_amd.engine import archs
    from marqo_amd.engine.languagebind import LanguageBindAudioTower, LanguageBindVideoTower
    case = (VCASES if kind == "v" else ACASES)[idx]
    cfg, sd = case.cfg(), case.sd()
    arch = archs.languagebind_arch_from_hf_config(cfg)
    base = LanguageBindVideoTower if kind == "v" else LanguageBindAudioTower
    plain, cap = base(arch, sd, DEV), _capturing(base)(arch, sd, DEV)
    o = T.ops(cfg, sd, device=DEV)
    x = (case.clip() if kind == "v" else case.px()).to(DEV)
    ex, mo = (T.exact(o, x), T.model(o, x)) if kind == "v" else (T.audio_exact(o, x), T.audio_model(o, x))
    return case, plain, cap, x, ex, mo


def _encode(tower, kind, x, normalize):
    out = tower.encode_clips(x, normalize=normalize) if kind == "v" else tower.encode_spectrograms(x, normalize=normalize)
    torch.cuda.synchronize()
    return out


def _captured(cap, kind, x, normalize):
    cap.calls = []
    try:
        out = _encode(cap, kind, x, normalize)
    finally:
        calls, cap.calls = cap.calls, None
    return out, calls


def _s():
    return torch.cuda.current_stream(DEV).cuda_stream


def _front_end_again(tower, kind, x):
    """one more call of the tower's own `_tokens`, on im2col rows made here from the items of ONE call"""
    lib, a = tower.lib, tower.arch
    with torch.cuda.device(DEV):
        if kind == "v":
            b, frames = x.shape[0], x.shape[0] * a.num_frames
            patches = torch.empty(frames * a.grid ** 2, tower.Kp, dtype=torch.bfloat16, device=DEV)
            L.check(lib.mq_patchify_clip(x.data_ptr(), patches.data_ptr(), b, a.num_frames, a.image_size, a.patch_size, tower.Kp, _s()), "mq_patchify_clip")
        else:
            frames = x.shape[0]
            patches = tower._patchify_f32(x)
        x0 = tower._tokens(patches, frames)
        torch.cuda.synchronize()
    return x0


def _tail_again(tower, kind, stream, items, normalize):
    """the tail from the captured last stream of ONE call with library kernels -> (cls_ln bf16 [frames, W], out fp32 [items, D])"""
    lib, a, s = tower.lib, tower.arch, _s()
    W, N, D = a.width, a.tokens, a.out_dim
    T_ = a.num_frames if kind == "v" else 1
    frames = items * T_
    assert stream.shape == (frames * N, W)
    with torch.cuda.device(DEV):
        idx = torch.empty(frames, dtype=torch.int32, device=DEV)
        cls_ln = torch.empty(frames, W, dtype=torch.bfloat16, device=DEV)
        proj = torch.empty(frames, D, dtype=torch.float32, device=DEV)
        out = torch.empty(items, D, dtype=torch.float32, device=DEV)
        L.check(lib.mq_cls_rows(idx.data_ptr(), frames, N, s), "mq_cls_rows")
        L.check(lib.mq_layernorm(stream.data_ptr(), idx.data_ptr(), tower._post[0], tower._post[1], cls_ln.data_ptr(), None, frames, W, a.ln_eps, s), "mq_layernorm")
        L.check(lib.mq_gemm_bf16(cls_ln.data_ptr(), W, tower._proj, W, None, None, proj.data_ptr(), D, frames, D, W, L.MQ_EPI_OUT_F32, s), "mq_gemm_bf16")
        if kind == "v":
            L.check(lib.mq_avg_tokens(proj.data_ptr(), 0, out.data_ptr(), items, T_, 0, D, s), "mq_avg_tokens")
        else:
            out.copy_(proj)
        if normalize:
            L.check(lib.mq_l2_normalize(out.data_ptr(), out.data_ptr(), items, D, s), "mq_l2_normalize")
        torch.cuda.synchronize()
    return cls_ln, out


def _joined(calls, kind, layers):
    """{view: the captured rows of all calls, one after the other}"""
    cat = lambda ts: torch.cat(ts, 0)
    got = {"x0": cat([c["x0"] for c in calls])}
    if kind == "v":
        for c in calls:
            assert len(c["before"]) == len(c["after"]) == layers, "one mq_encoder_forward call per layer was expected"
        for l in range(layers):
            got[f"temporal{l}"] = cat([c["before"][l] for c in calls])
            got[f"block{l}"] = cat([c["after"][l] for c in calls])
    else:
        for c in calls:
            assert len(c["before"]) == len(c["after"]) == 1, "one mq_encoder_forward call over all blocks was expected"
            assert _same_bits(c["before"][0], c["x0"]), "the audio tower's encoder call does not start from the front end's stream"
        got[f"block{layers - 1}"] = cat([c["after"][0] for c in calls])
    return got


def _run_case(kind, idx):
    case, plain, cap, x, ex, mo = _setup(kind, idx)
    a = plain.arch
    tower_name, layers = ("video" if kind == "v" else "audio"), a.layers
    items_per_frame = a.num_frames if kind == "v" else 1
    split = getattr(case, "split", 0)
    worst, outs = {}, {}
    vex, vmo = T.views(ex), T.views(mo)
    for normalize in (True, False):
        want = _encode(plain, kind, x, normalize)
        cap.max_items_per_call = split or plain.max_items_per_call
        got, calls = _captured(cap, kind, x, normalize)
        if not _same_bits(got, want):
            pytest.fail(f"the capturing subclass does not return the plain tower's bits (normalize={normalize}): {NO_PARITY}")
        assert _same_bits(_encode(plain, kind, x, normalize), want), "the same call twice: other bits"
        assert tuple(got.shape) == (case.B, a.out_dim) and bool(torch.isfinite(got).all())
        per_call = [c["x0"].shape[0] // (a.tokens * items_per_frame) for c in calls]
        assert sum(per_call) == case.B and (per_call == [2, 1] if split else len(calls) == 1), per_call
        view = _joined(calls, kind, layers)
        assert all(bool(torch.isfinite(t).all()) for t in view.values())
        # the front end once more, and the tail from the captured last stream: the captured tensors are what the tower computed its output from
        cls_parts, i0 = [], 0
        for c, n in zip(calls, per_call):
            if not _same_bits(_front_end_again(plain, kind, x[i0:i0 + n].contiguous()), c["x0"]):
                pytest.fail(f"one more call of the tower's own _tokens does not give the captured front-end stream: {NO_PARITY}")
            cls_ln, again = _tail_again(plain, kind, c["after"][-1], n, normalize)
            if not _same_bits(again, got[i0:i0 + n]):
                pytest.fail(f"the tail redone from the captured last stream does not give the tower's output (normalize={normalize}): {NO_PARITY}")
            cls_parts.append(cls_ln)
            i0 += n
        view["cls_ln"] = torch.cat(cls_parts, 0)
        view[f"pooled/l2={int(normalize)}"] = got
        if split:       # the same batch in one call: every stream and the pooled rows bit for bit
            cap.max_items_per_call = plain.max_items_per_call
            whole_out, whole_calls = _captured(cap, kind, x, normalize)
            assert len(whole_calls) == 1
            whole = _joined(whole_calls, kind, layers)
            for name, t in whole.items():
                assert _same_bits(t, view[name]), f"{name}: a batch split over {len(calls)} calls differs from the unsplit call"
            assert _same_bits(whole_out, got), "pooled rows: a batch split over several calls differs from the unsplit call"
        assert set(view) | {"pooled/l2=0", "pooled/l2=1"} == set(vex), (sorted(view), sorted(vex))
        for name, t in view.items():
            r = E.row_ratio(t, vex[name], vmo[name])
            print(f"LB_RATIO tower={tower_name} case={case.id} normalize={int(normalize)} view={name} ratio={r['ratio']:.3f} "
                  f"(row {r['row']} col {r['col']}: l2 {r['l2']:.3f} linf {r['linf']:.3f})")
            worst[name] = max(worst.get(name, 0.0), r["ratio"])
        outs[normalize] = got
    assert float((outs[True].norm(dim=-1) - 1).abs().max()) <= 1e-5
    assert _cos_err(outs[False], outs[True]) <= 1e-6, "normalize=False rows do not keep the direction of the unit rows"
    print(f"LB_WORST tower={tower_name} case={case.id}: " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= MARGIN, worst


def test_the_max_frames_case_is_at_the_engines_constant():
    assert any(c.T == _max_frames() for c in VCASES) and T.video_cases(_max_frames())[4].T == _max_frames()


@pytest.mark.parametrize("idx", range(len(VCASES)), ids=[c.id for c in VCASES])
def test_video_pass_against_float64(idx):
    _run_case("v", idx)


@pytest.mark.parametrize("idx", range(len(ACASES)), ids=[c.id for c in ACASES])
def test_audio_pass_against_float64(idx):
    _run_case("a", idx)

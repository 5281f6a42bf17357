"""The two host-side walks of the convolutional towers — cnx_forward (csrc/convnext.hip) and rn_forward (csrc/resnet.hip) — through the C ABI
(mq_convnext_workspace_bytes / mq_encode_convnext_u8 / _f32, mq_resnet_workspace_bytes / mq_encode_resnet_u8 / _f32) with a caller-owned workspace and
normalize = 0, every output row held to the float64 reference of tests/convtower_ref.py.

Weights: the engine's own towers (ConvNextTower, ResNetTower: the load-time folds and paddings) on seeded checkpoints; the reference builds its operands
from the same checkpoint with the same fold functions (tests/test_convtower_ref_host.py pins it to the fp32 restatements).  Every case:
  - the worst row of  max(|got - exact|_2 / |model - exact|_2, |got - exact|_inf / |model - exact|_inf)  <= MARGIN (tests/test_patch_attn_gpu.py) on the
    output rows and on the last stage's per-pixel stream, for n = 1 and n = 3; printed as CONVTOWER_RATIO tower=... case=... n=... what=... ratio=...;
  - the workspace is exactly mq_*_workspace_bytes long, filled with 0xFF bytes (NaN as bf16 and as fp32: anything read before it is written reaches the
    output), between two 64 KiB guard regions of another sentinel that must come back untouched.
Where the stream is read: ConvNeXt keeps it in the first region of its plan for the whole walk — [n H3 H3, C3] bf16 at workspace offset 0; the plan's
arithmetic is restated here and must reproduce mq_convnext_workspace_bytes.  ResNet's workspace is five equal buffers, the stream starts in the first and
changes places with the second once per stage (the downsample branch of every stage's first block): an even number of times, so it ends at offset 0 too, and
the attention pool behind it writes the other four.
Per tower also: one batch that moves the late GEMMs out of the skinny family (convtower_ref.CNX_BIG_N / RN_BIG_N, from the row limits of
tests/test_small_m_gpu.py); u8 and f32 input; a permuted batch returns the permuted rows bit for bit (tiled GEMMs pinned); workspace_bytes - 1 is refused with
nothing written.

Measured on an MI355X (worst CONVTOWER_RATIO over the cases, output rows / last-stage stream rows; bar 4.0):
  ConvNeXt  n = 1, 3 over the seven cases 1.50 / 1.57     n = 321 (tiled last stage and head) 1.62 / 2.27     f32 input 1.27 / 1.26
  ResNet    n = 1, 3 over the twelve cases 1.53 / 1.49   n = 81 (tiled stage-4 downsample and k | v) 1.20 / 2.06    f32 input 1.05 / 1.23
            (the width-16 cases 1.00 .. 1.04 / 1.00 .. 1.14)
No value anywhere was non-finite: with the workspace filled with NaN bytes, no padded channel and no buffer is read before the walk has written it.

Found while this file was written: rn_forward decided whether a block has the downsample branch by comparing its PADDED input width with its output width.
At width 16 pad64(16) = 64 = 4 x 16, so layer1.0 was run as an identity block: its downsample convolution was skipped and the zero-padded stem output was
added in its place.  No served checkpoint has that width (64, 80, 96, 128: pad64(w) < 4 w), and the full-size tests run only those.  The reference carries
the old rule as the mutation ds_by_padded_width: 126 .. 222 yardsticks on the width-16 cases (tests/test_convtower_ref_host.py).  The walk now takes the first
block of every stage, as the module and the loader do.
"""
import ctypes as C

import pytest
import torch

from marqo_amd import _lib as L
from tests import convtower_ref as T
from tests.convtower_ref import MARGIN, row_ratio

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64 * 1024
SENTINEL, WS_FILL, OUT_FILL = 0xA5, 0xFF, 0x5A

_CNX = {c[0]: c for c in T.convnext_cases()}
_RN = {c[0]: c for c in T.resnet_cases()}
_towers = {}


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def _align(x, a=256):
    return (x + a - 1) // a * a


def _tower(kind, cid):
    """(arch, the engine's tower, the reference's operands on the device); one tower at a time"""
    key = (kind, cid)
    if key not in _towers:
        _towers.clear()
        torch.cuda.empty_cache()
        from marqo_amd.engine import towers
        if kind == "convnext":
            _, arch, b2, seed, stem = _CNX[cid]
            sd = T.convnext_sd(arch, b2, seed, stem)
            _towers[key] = (arch, seed, towers.ConvNextTower(arch, sd, DEV), T.ops_to(T.convnext_operands(arch, sd), DEV))
        else:
            _, arch, seed = _RN[cid]
            sd = T.resnet_sd(arch, seed)
            _towers[key] = (arch, seed, towers.ResNetTower(arch, sd, DEV), T.ops_to(T.resnet_operands(arch, sd), DEV))
    return _towers[key]


def _entry(kind, what):
    lib = L.load()
    return getattr(lib, f"mq_encode_{kind}_{what}"), getattr(lib, f"mq_{kind}_workspace_bytes")


def _call(kind, tw, pixels, short=0):
    """one call on a fresh guarded workspace of exactly workspace_bytes - short bytes -> (rc, out [n, E] fp32, the workspace bytes, need)"""
    what = "u8" if pixels.dtype == torch.uint8 else "f32"
    encode, ws_bytes = _entry(kind, what)
    n = pixels.shape[0]
    need = ws_bytes(C.byref(tw.cfg), n)
    assert need > 0
    buf = torch.full((GUARD + need + GUARD,), SENTINEL, dtype=torch.uint8, device=DEV)
    ws = buf[GUARD:GUARD + need]
    ws.fill_(WS_FILL)
    assert ws.data_ptr() % 256 == 0
    out = torch.full((n * tw.cfg.out_dim * 4,), OUT_FILL, dtype=torch.uint8, device=DEV)
    pixels = pixels.contiguous()
    torch.cuda.synchronize()
    rc = encode(C.byref(tw.cfg), C.byref(tw.w), pixels.data_ptr(), n, out.data_ptr(), 0, ws.data_ptr(), need - short, _stream())
    torch.cuda.synchronize()
    assert bool((buf[:GUARD] == SENTINEL).all()), "the guard region in front of the workspace was written"
    assert bool((buf[GUARD + need:] == SENTINEL).all()), "the guard region behind the workspace was written"
    return rc, out.view(torch.float32).view(n, tw.cfg.out_dim), ws, need


def _convnext_plan_bytes(arch, n):
    """cnx_plan restated: the stream x is the FIRST region (offset 0); every region is rounded up to 256 bytes"""
    rows0, E = n * (arch.image_size // 4) ** 2, arch.out_dim
    stream = rows0 * arch.dims[0] * 2
    regions = [stream, stream, max(4 * stream, rows0 * 64 * 2), (arch.dims[0] // 64) * rows0 * 8, rows0 * 8, n * arch.dims[3] * 2, n * 2 * E * 2]
    return sum(_align(r) for r in regions), stream


def _last_stream(kind, arch, ws, need, n):
    if kind == "convnext":
        total, first = _convnext_plan_bytes(arch, n)
        assert total == need, "mq_convnext_workspace_bytes is not the plan this file reads the stream by"
        H3, C3 = arch.image_size // 32, arch.dims[3]
    else:
        assert need % 5 == 0 and (need // 5) % 256 == 0
        first = need // 5
        H3, C3 = arch.image_size // 32, 32 * arch.width
    rows = n * H3 * H3
    assert rows * C3 * 2 <= first
    return ws[:rows * C3 * 2].view(torch.bfloat16).view(rows, C3).clone()


def _reference(kind, arch, ops, px):
    if kind == "convnext":
        return T.convnext_exact(arch, ops, px), T.convnext_model(arch, ops, px)
    return T.resnet_exact(arch, ops, px), T.resnet_model(arch, ops, px)


def _measure(kind, cid, tw_tuple, u8, what="u8"):
    arch, seed, tw, ops = tw_tuple
    n = u8.shape[0]
    px = T.normalise(u8)
    rc, out, ws, need = _call(kind, tw, u8 if what == "u8" else px)
    L.check(rc, f"mq_encode_{kind}_{what}")
    stream = _last_stream(kind, arch, ws, need, n)
    ex, mo = _reference(kind, arch, ops, px)
    worst = []
    for name, got, e, m in (("output", out, ex[0], mo[0]), ("stream", stream, ex[1], mo[1])):
        finite = bool(torch.isfinite(got.double()).all())
        r = row_ratio(got.double(), e, m)
        print(f"CONVTOWER_RATIO tower={kind} case={cid} n={n} input={what} what={name} ratio={r['ratio']:.3f} (row {r['row']} col {r['col']}: l2 {r['l2']:.3f} "
              f"linf {r['linf']:.3f}){'' if finite else ' NON-FINITE'}")
        worst.append(r["ratio"])
    return max(worst), out


def _images(arch, seed, n):
    return T.images(n, arch.image_size, seed).to(DEV)


@pytest.mark.parametrize("cid", list(_CNX))
def test_convnext_walk_against_float64(cid):
    t = _tower("convnext", cid)
    worst = [_measure("convnext", cid, t, _images(t[0], t[1], n))[0] for n in (1, 3)]
    assert max(worst) <= MARGIN


@pytest.mark.parametrize("cid", list(_RN))
def test_resnet_walk_against_float64(cid):
    t = _tower("resnet", cid)
    worst = [_measure("resnet", cid, t, _images(t[0], t[1], n))[0] for n in (1, 3)]
    assert max(worst) <= MARGIN


def test_convnext_batch_past_the_skinny_gemms():
    cid = T.convnext_cases()[0][0]
    t = _tower("convnext", cid)
    assert T.CNX_BIG_N * (t[0].image_size // 32) ** 2 > T.GROUPED_ROWS      # the last stage's and the head's GEMMs: tiled
    assert _measure("convnext", cid, t, _images(t[0], t[1], T.CNX_BIG_N))[0] <= MARGIN


def test_resnet_batch_past_the_skinny_gemms():
    cid = T.resnet_cases()[0][0]
    t = _tower("resnet", cid)
    assert T.RN_BIG_N * (t[0].image_size // 32) ** 2 > T.GROUPED_ROWS and T.RN_BIG_N > T.SKINNY_ROWS
    assert _measure("resnet", cid, t, _images(t[0], t[1], T.RN_BIG_N))[0] <= MARGIN


@pytest.mark.parametrize("kind,cid", [("convnext", T.convnext_cases()[3][0]), ("resnet", T.resnet_cases()[5][0])])
def test_f32_input_against_float64(kind, cid):
    t = _tower(kind, cid)
    u8 = _images(t[0], t[1], 3)
    assert _measure(kind, cid, t, u8, what="f32")[0] <= MARGIN


@pytest.mark.parametrize("kind,cid", [("convnext", T.convnext_cases()[4][0]), ("resnet", T.resnet_cases()[10][0])])
def test_permuted_batch_returns_the_permuted_rows(kind, cid, tiled_gemm_only):
    t = _tower(kind, cid)
    u8 = _images(t[0], t[1], 3)
    perm = [2, 0, 1]
    rc, a, _, _ = _call(kind, t[2], u8)
    L.check(rc, kind)
    rc, b, _, _ = _call(kind, t[2], u8[perm])
    L.check(rc, kind)
    assert bool(torch.isfinite(a).all())
    assert torch.equal(a[perm].view(torch.int32), b.view(torch.int32))
    rc, one, _, _ = _call(kind, t[2], u8[1:2])
    L.check(rc, kind)
    assert torch.equal(one[0].view(torch.int32), a[1].view(torch.int32))


@pytest.mark.parametrize("kind,cid", [("convnext", T.convnext_cases()[1][0]), ("resnet", T.resnet_cases()[2][0])])
def test_a_workspace_one_byte_short_is_refused_with_nothing_written(kind, cid):
    t = _tower(kind, cid)
    u8 = _images(t[0], t[1], 3)
    rc, out, ws, need = _call(kind, t[2], u8, short=1)
    assert rc != 0
    assert bool((ws == WS_FILL).all()), "a refused call wrote to the workspace"
    assert bool((out.view(torch.uint8) == OUT_FILL).all()), "a refused call wrote to the output"
    rc, out, _, _ = _call(kind, t[2], u8)           # exactly workspace_bytes: works
    L.check(rc, kind)
    assert bool(torch.isfinite(out).all())

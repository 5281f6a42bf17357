"""The building blocks of csrc/embed.hip, one by one at the C ABI, against a float64 torch statement of the same operation: the rotary steps
(NewModel rotate_half, EVA02 table), the gated MLP with and without its LayerNorm (modes 0-3), the pooling heads (map, mean / CLS, avg), the
token / patch front ends and the row gathers.  Bounds are elementwise: bit equality where the kernel's fp32 arithmetic is the reference's, else about
one bf16 ulp of the operands' magnitude.  In-place kernels start from sentinel-filled buffers, and everything outside their documented output
(V columns, gate halves, prefix rows, neighbouring rows) must come back bit for bit."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from marqo_amd import _lib as L
from marqo_amd.engine import archs
from marqo_amd.engine.archs import OPENAI_DATASET_MEAN, OPENAI_DATASET_STD

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT16 = 0x7FA5          # a bf16 NaN: a kernel that reads it spreads NaN, one that writes over it changes its bits
ULP = 2.0 ** -8          # one bf16 ulp, relative


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def _sync_check(rc, what):
    L.check(rc, what)
    torch.cuda.synchronize(DEV)


def _bits(t):
    return t.view({torch.bfloat16: torch.int16, torch.float32: torch.int32, torch.uint8: torch.uint8}[t.dtype])


def _sent_bf16(*shape):
    return torch.full(shape, SENT16, dtype=torch.int16, device=DEV).view(torch.bfloat16)


def _sent_f32(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def _within(out, ref, tol, what):
    err = (out.double() - ref).abs()
    bad = ~(err <= tol)
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())} of {bad.numel()} elements out of bound; worst excess "
                                 f"{float((err - tol)[bad].max()) if bool(bad.any()) else 0.0:.3e} at {tuple(bad.nonzero()[0].tolist())}")


def _cu(lens):
    cu = [0]
    for n in lens:
        cu.append(cu[-1] + n)
    return torch.tensor(cu, dtype=torch.int32, device=DEV)


def _positions(lens):
    return torch.cat([torch.arange(n) for n in lens]).to(DEV)


# ---- mq_rope: NewModel rotary (rotate_half) on Q and K --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("heads,lens,ragged", [
    (2, [7, 7, 7], False), (12, [64, 64], False), (16, [33, 33], False),
    (2, [1, 5, 1, 40], True), (12, [1, 300, 17, 1], True), (16, [5, 1, 64], True),
    (16, [8192], True),                          # one sequence at NewModel's max_pos (stella_en_400M_v5)
])
def test_rope_matches_rotate_half(heads, lens, ragged):
    lib = L.load()
    hd = 64
    Wa, rows, half = heads * hd, sum(lens), hd // 2
    inv = archs.STELLA_EN_400M.rope_inv_freq().to(DEV)            # [32] fp32, head width 64
    assert inv.numel() == half
    g = torch.Generator().manual_seed(heads * 1000 + rows)
    buf = _sent_bf16(rows + 2, 3 * Wa)
    buf[:rows] = torch.randn(rows, 3 * Wa, generator=g).to(torch.bfloat16).to(DEV)
    before = buf.clone()
    if ragged:
        cu = _cu(lens)
        _sync_check(lib.mq_rope(buf.data_ptr(), cu.data_ptr(), len(lens), 0, Wa, heads, inv.data_ptr(), _stream()), "mq_rope")
    else:
        _sync_check(lib.mq_rope(buf.data_ptr(), None, len(lens), lens[0], Wa, heads, inv.data_ptr(), _stream()), "mq_rope")
    # the angle exactly as oracle/towers.py::new_model_forward builds it (fp32 position * fp32 inv_freq); its cos / sin in fp64
    ang = _positions(lens).to(torch.float32)[:, None] * inv[None, :]
    cs, sn = ang.double().cos()[:, None, :], ang.double().sin()[:, None, :]
    x = before[:rows, :2 * Wa].double().view(rows, 2 * heads, hd)
    x1, x2 = x[..., :half], x[..., half:]
    out = buf[:rows, :2 * Wa].view(rows, 2 * heads, hd)
    tol = ULP * (x1.abs() + x2.abs()) + 1e-6                      # against the operands: y itself may cancel
    _within(out[..., :half], x1 * cs - x2 * sn, tol, "rope first half")
    _within(out[..., half:], x2 * cs + x1 * sn, tol, "rope second half")
    assert torch.equal(_bits(buf[:rows, 2 * Wa:]), _bits(before[:rows, 2 * Wa:])), "V columns changed"
    assert torch.equal(_bits(buf[rows:]), _bits(before[rows:])), "rows past the last sequence changed"


# ---- mq_rope_table: EVA02 2-D rotary from a (cos | sin) table on interleaved pairs ----------------------------------------------------------------
@pytest.mark.parametrize("name", ["EVA02-B-16", "EVA02-L-14", "EVA02-L-14-336", "random"])
@pytest.mark.parametrize("prefix", [0, 1])
def test_rope_table_matches_interleaved_rotation(name, prefix):
    lib = L.load()
    arch = archs.OPEN_CLIP_ARCHS["EVA02-B-16" if name == "random" else name][0]
    table = arch.rope_table().to(DEV)                              # [patches, 2, hs]
    g = torch.Generator().manual_seed(prefix * 7 + len(name))
    if name == "random":   # the real table repeats every value across a pair: only independent values tell cos[2i] from cos[2i + 1]
        table = (2 * torch.rand(table.shape, generator=g) - 1).to(DEV)
    P, _, hs = table.shape
    heads, Wa = arch.heads, arch.width
    assert hs * heads == Wa
    T, n = P + prefix, 3 if arch.width < 1024 else 2
    rows = n * T
    buf = _sent_bf16(rows + 1, 3 * Wa)
    buf[:rows] = torch.randn(rows, 3 * Wa, generator=g).to(torch.bfloat16).to(DEV)
    before = buf.clone()
    _sync_check(lib.mq_rope_table(buf.data_ptr(), rows, T, prefix, Wa, heads, table.data_ptr(), _stream()), "mq_rope_table")
    t = torch.arange(rows, device=DEV) % T
    rot = t >= prefix
    tab = table.double()[(t - prefix)[rot]]                        # [rotated rows, 2, hs]
    cs, sn = tab[:, 0][:, None, :], tab[:, 1][:, None, :]
    x = before[:rows, :2 * Wa][rot].double().view(-1, 2 * heads, hs)
    xe, xo = x[..., 0::2], x[..., 1::2]
    a_e, b_e = xe * cs[..., 0::2], xo * sn[..., 0::2]
    a_o, b_o = xo * cs[..., 1::2], xe * sn[..., 1::2]
    out = buf[:rows, :2 * Wa][rot].view(-1, 2 * heads, hs)
    _within(out[..., 0::2], a_e - b_e, ULP * (a_e.abs() + b_e.abs()) + 1e-6, "rope_table even elements")
    _within(out[..., 1::2], a_o + b_o, ULP * (a_o.abs() + b_o.abs()) + 1e-6, "rope_table odd elements")
    assert torch.equal(_bits(buf[:rows][~rot]), _bits(before[:rows][~rot])), "prefix rows changed"
    assert torch.equal(_bits(buf[:rows, 2 * Wa:]), _bits(before[:rows, 2 * Wa:])), "V columns changed"
    assert torch.equal(_bits(buf[rows:]), _bits(before[rows:])), "the row past the last sequence changed"


# ---- mq_glu / mq_glu_ln: the gated MLP's product, with and without the LayerNorm behind it ------------------------------------------------------
ACTS = {L.MQ_ACT_SILU: F.silu, L.MQ_ACT_GELU: F.gelu, L.MQ_ACT_QUICKGELU: lambda x: x * torch.sigmoid(1.702 * x)}
# absolute error of the kernel's activation itself: gelu_erf is a clamped minimax polynomial with |error| <= 7e-5 (csrc/common.h); silu and
# quick_gelu are exact up to fp32 rounding (covered by the 2^-16 term of the bound)
ACT_ABS_ERR = {L.MQ_ACT_SILU: 0.0, L.MQ_ACT_GELU: 7e-5, L.MQ_ACT_QUICKGELU: 0.0}
GLU_F = [(64, 64), (1024, 1024), (1032, 1032), (2048, 2048), (2752, 2730), (3072, 3072), (4096, 4096)]   # every CH of glu_ln_kernel


def _glu_case(kind, F_, Ft, act, rows, seed):
    """-> (buffer before, buffer after, up, gate, g, b) for one call; kind: 'glu' / 'glu_il' (mq_glu) or LayerNorm mode 0-3 (mq_glu_ln)"""
    lib = L.load()
    il = kind in ("glu_il", 1, 3)
    gen = torch.Generator().manual_seed(seed)
    up = 1.0 + 0.5 * torch.randn(rows, F_, generator=gen)          # a nonzero mean: the LayerNorm's statistics must come from the right columns
    up[:, Ft:] = 0.0                                               # the zero padding of a width-Ft model: its products are exactly 0
    up = up.to(torch.bfloat16).to(DEV)
    gate = (2.0 * torch.randn(rows, F_, generator=gen)).to(torch.bfloat16).to(DEV)
    buf = _sent_bf16(rows + 2, 2 * F_)
    if il:   # (up, gate) interleaved 16 by 16 (MQ_EPI_GLU's layout)
        buf[:rows] = torch.stack([up.view(rows, -1, 16), gate.view(rows, -1, 16)], 2).reshape(rows, 2 * F_)
    elif kind == 2:   # the product is already there; the other half is never read
        buf[:rows, :F_] = up
    else:
        buf[:rows, :F_], buf[:rows, F_:] = up, gate
    g = (1.0 + 0.2 * torch.randn(F_, generator=gen))
    b = 0.2 * torch.randn(F_, generator=gen)
    g[Ft:], b[Ft:] = 0.0, 0.0
    g, b = g.to(DEV), b.to(DEV)
    before = buf.clone()
    if kind == "glu" or kind == "glu_il":
        _sync_check(lib.mq_glu(buf.data_ptr(), rows, F_, act, 1 if il else 0, _stream()), "mq_glu")
    else:
        gp, bp = (None, None) if kind == 3 else (g.data_ptr(), b.data_ptr())
        _sync_check(lib.mq_glu_ln(buf.data_ptr(), rows, F_, Ft, act, gp, bp, 1e-6, kind, _stream()), "mq_glu_ln")
    return before, buf, up, gate, g, b


def _check_glu(kind, F_, Ft, act, rows, seed):
    before, buf, up, gate, g, b = _glu_case(kind, F_, Ft, act, rows, seed)
    out = buf[:rows, :F_]
    u = up.double()
    prod = u if kind == 2 else u * ACTS[act](gate.double())
    if kind in ("glu", "glu_il", 3):
        tol = ULP * prod.abs() + u.abs() * (ACT_ABS_ERR[act] + 2.0 ** -16 * (1 + gate.double().abs()))
        _within(out, prod, tol, f"glu product ({kind}, act {act})")
    else:
        v = prod[:, :Ft]
        mean = v.mean(1, keepdim=True)
        nrm = (prod - mean) / torch.sqrt(v.var(1, unbiased=False, keepdim=True) + 1e-6)
        ng, bb = nrm * g.double(), b.double()
        _within(out[:, :Ft], (ng + bb)[:, :Ft], (ULP * (ng.abs() + bb.abs()) + 2.0 ** -12 * g.double().abs())[:, :Ft],
                f"glu_ln mode {kind} (act {act})")
        assert bool((out[:, Ft:] == 0).all()), "the zero padding of a width-Ft row did not stay 0"
    # outside [:rows, :F] nothing moves: the gate half / the interleaved source tail / the unread half, and the neighbouring rows
    assert torch.equal(_bits(buf[:rows, F_:]), _bits(before[:rows, F_:])), "columns F.. changed"
    assert torch.equal(_bits(buf[rows:]), _bits(before[rows:])), "rows past the call changed"


@pytest.mark.parametrize("kind,F_,Ft", [(k, f, ft) for k in ("glu", "glu_il", 0, 1, 2, 3) for f, ft in GLU_F
                                         if f % 16 == 0 or k in ("glu", 0, 2)])   # the interleaved layouts need F % 16 == 0 (tests/test_abi.py)
def test_glu_and_glu_ln_match_fp64(kind, F_, Ft):
    if kind in ("glu", "glu_il", 3) and Ft != F_:
        Ft = F_                                                     # no LayerNorm: no statistics width
    for i, act in enumerate(ACTS):
        _check_glu(kind, F_, Ft, act, 7 if i % 2 == 0 else 13, seed=F_ * 10 + i)    # row counts not divisible by 4


def test_glu_grid_stride_wraps():
    """12 800 x 4096: 6.5 M 8-column chunks, more than the 16384 x 256 threads of the capped grid"""
    _check_glu("glu", 4096, 4096, L.MQ_ACT_SILU, 12800, seed=5)


# ---- mq_map_pool: one learned query per head (SigLIP map head, CoCa attentional pooler) -------------------------------------------------------
def _map_pool(hd, heads, T, spread, n=2, seed=0):
    lib = L.load()
    W = hd * heads
    gen = torch.Generator().manual_seed(seed)
    kv = torch.randn(n * T, 2 * W, generator=gen).to(torch.bfloat16).to(DEV)
    q = (spread / hd ** 0.5 * torch.randn(W, generator=gen)).to(DEV)
    out = _sent_bf16(n + 1, W)
    _sync_check(lib.mq_map_pool(kv.data_ptr(), q.data_ptr(), out.data_ptr(), n, T, W, heads, _stream()), "mq_map_pool")
    k = kv[:, :W].double().view(n, T, heads, hd)
    v = kv[:, W:].double().view(n, T, heads, hd)
    s = torch.einsum("nthd,hd->nht", k, q.double().view(heads, hd))
    p = torch.softmax(s, -1)
    ref = torch.einsum("nht,nthd->nhd", p, v).reshape(n, W)
    tol = ULP * torch.einsum("nht,nthd->nhd", p, v.abs()).reshape(n, W) + 1e-6
    _within(out[:n], ref, tol, f"map_pool hd {hd} T {T}")
    assert torch.equal(_bits(out[n:]), torch.full((1, W), SENT16, dtype=torch.int16, device=DEV)), "the row past the call changed"
    return s


@pytest.mark.parametrize("T", [1, 63, 64, 65, 196, 729, 4096])
@pytest.mark.parametrize("hd,heads", [(64, 12), (72, 16), (128, 16)])   # 72: lanes 64-71 take the second output column (SO400M)
def test_map_pool_matches_softmax(hd, heads, T):
    _map_pool(hd, heads, T, spread=2.0, seed=T + hd)


def test_map_pool_wide_score_spread():
    s = _map_pool(72, 16, 196, spread=15.0, seed=3)
    assert float(s.max()) > 25 and float(s.min()) < -25          # the max subtraction is exercised


# ---- mq_pool: masked mean / CLS pooling (+ L2) over packed sequences ---------------------------------------------------------------------
@pytest.mark.parametrize("W", [384, 768, 1000, 2048])
@pytest.mark.parametrize("pool", [L.MQ_POOL_MEAN, L.MQ_POOL_CLS])
@pytest.mark.parametrize("normalize", [0, 1])
def test_pool_matches_fp64(W, pool, normalize):
    lib = L.load()
    lens = [1, 7, 1, 300, 4, 33]
    zero = (2, 4)                                                  # an all-zero sequence of 1 row and one of 4 rows
    nseq, rows = len(lens), sum(lens)
    gen = torch.Generator().manual_seed(W + pool * 3 + normalize)
    x = (0.3 + torch.randn(rows, W, generator=gen)).to(DEV)
    cu = _cu(lens)
    for i in zero:
        x[cu[i]:cu[i + 1]] = 0.0
    out = _sent_f32(nseq + 1, W)
    _sync_check(lib.mq_pool(x.data_ptr(), cu.data_ptr(), nseq, out.data_ptr(), W, pool, normalize, _stream()), "mq_pool")
    assert not bool(out[:nseq].isnan().any()), "NaN in the pooled rows (an all-zero row must normalise to zeros: the 1e-12 clamp)"
    for i, n in enumerate(lens):
        seg = x[cu[i]:cu[i + 1]].double()
        m = seg[:1] if pool == L.MQ_POOL_CLS else seg
        ref = m.mean(0)
        mag = m.abs().mean(0)
        ln = m.shape[0]
        den = max(float(ref.norm()), 1e-12) if normalize else 1.0
        ref = ref / den
        tol = 2 * (ln * 2.0 ** -24 + 2.0 ** -20) * mag / den + 2.0 ** -20 * ref.abs()
        if pool == L.MQ_POOL_CLS and not normalize:
            assert torch.equal(_bits(out[i]), _bits(x[cu[i]])), "CLS pooling is a copy"
        _within(out[i], ref, tol, f"pool seq {i} (len {n})")
        if i in zero:
            assert bool((out[i] == 0).all())
    assert bool(out[nseq:].isnan().all()), "the row past the call changed"


# ---- mq_embed_tokens: token (+ position, + type) embedding (+ LayerNorm) ------------------------------------------------------------------------
EMBED_W = [256, 384, 768, 1024, 1152, 2048]   # CH 1, 2, 3, 4, 6 (masked tail: 288 of 384 lanes), 8


def _embed(W, ids, lens, *, pos=False, type0=False, ln=False, out_f32=True, out_bf16=False, last_pos=0, vocab=1000, seed=0):
    lib = L.load()
    gen = torch.Generator().manual_seed(seed)
    rows = sum(lens)
    tok = torch.randn(vocab, W, generator=gen).to(DEV)
    pt = (0.1 * torch.randn(600, W, generator=gen)).to(DEV) if pos else None
    ty = (0.1 * torch.randn(W, generator=gen)).to(DEV) if type0 else None
    g = (1 + 0.2 * torch.randn(W, generator=gen)).to(DEV) if ln else None
    b = (0.2 * torch.randn(W, generator=gen)).to(DEV) if ln else None
    cu = _cu(lens)
    x = _sent_f32(rows + 2, W) if out_f32 else None
    xb = _sent_bf16(rows + 2, W) if out_bf16 else None
    ptr = lambda t: None if t is None else t.data_ptr()
    _sync_check(lib.mq_embed_tokens(ids.data_ptr(), cu.data_ptr(), len(lens), tok.data_ptr(), ptr(pt), ptr(ty), ptr(g), ptr(b), ptr(x), ptr(xb),
                                    W, vocab, 1e-12, last_pos, _stream()), "mq_embed_tokens")
    # the sum in the kernel's fp32 order: token, + position, + type
    s = tok[ids.long().clamp(0, vocab - 1)]
    if pos:
        t = _positions(lens)
        if last_pos:
            t[cu[1:].long() - 1] = last_pos
        s = s + pt[t]
    if ty is not None:
        s = s + ty
    return s, g, b, x, xb, rows


@pytest.mark.parametrize("W", EMBED_W)
@pytest.mark.parametrize("variant", ["plain", "clip", "coca", "bert", "both"])
def test_embed_tokens_matches_fp64(W, variant):
    lens = [1, 5, 512, 3]                                          # 512 rows: the 4 waves of the workgroup wrap 128 times
    opts = {"plain": dict(), "clip": dict(pos=True, out_f32=False, out_bf16=True), "coca": dict(pos=True, out_bf16=True, last_pos=76),
            "bert": dict(pos=True, type0=True, ln=True), "both": dict(pos=True, ln=True, out_bf16=True)}[variant]
    gen = torch.Generator().manual_seed(W)
    ids = torch.randint(0, 1000, (sum(lens),), generator=gen, dtype=torch.int32).to(DEV)
    s, g, b, x, xb, rows = _embed(W, ids, lens, seed=W, **opts)
    if g is None:   # no LayerNorm: the same fp32 additions, then round-to-nearest-even to bf16
        if x is not None:
            assert torch.equal(_bits(x[:rows]), _bits(s)), "fp32 rows differ"
        if xb is not None:
            assert torch.equal(_bits(xb[:rows]), _bits(s.to(torch.bfloat16))), "bf16 rows differ"
    else:
        sd = s.double()
        nrm = (sd - sd.mean(1, keepdim=True)) / torch.sqrt(sd.var(1, unbiased=False, keepdim=True) + 1e-12)
        ng, bb, gg = nrm * g.double(), b.double(), g.double().abs()
        if x is not None:
            _within(x[:rows], ng + bb, 2.0 ** -16 * (ng.abs() + bb.abs() + gg), "embed LayerNorm fp32")
        if xb is not None:
            _within(xb[:rows], ng + bb, ULP * (ng.abs() + bb.abs()) + 2.0 ** -12 * gg, "embed LayerNorm bf16")
    if x is not None:
        assert bool(x[rows:].isnan().all()), "fp32 rows past the call changed"
    if xb is not None:
        assert bool((_bits(xb[rows:]) == SENT16).all()), "bf16 rows past the call changed"


def test_embed_tokens_clamps_out_of_range_ids():
    """ids < 0 read row 0 and ids >= vocab read row vocab - 1: the only guard against an out-of-bounds table read"""
    vocab = 1000
    ids = torch.tensor([-7, -1, 0, 999, 1000, 1005, 2 ** 31 - 1, -(2 ** 31), 17], dtype=torch.int32, device=DEV)
    s, _, _, x, _, rows = _embed(768, ids, [4, 5], vocab=vocab, seed=1)
    want = torch.tensor([0, 0, 0, 999, 999, 999, 999, 0, 17])
    assert torch.equal(ids.long().clamp(0, vocab - 1).cpu(), want)
    assert torch.equal(_bits(x[:rows]), _bits(s))


# ---- mq_vit_assemble: class token + patches + positions (+ ln_pre) -----------------------------------------------------------------------------
@pytest.mark.parametrize("W", EMBED_W)
def test_vit_assemble_matches_fp64(W):
    lib = L.load()
    n, npch, eps = 2, 49, 1e-5
    gen = torch.Generator().manual_seed(W)
    for cls in (True, False):
        T = npch + (1 if cls else 0)
        po = torch.randn(n * npch, W, generator=gen).to(DEV)
        ct = torch.randn(W, generator=gen).to(DEV)
        pos = (0.5 * torch.randn(T, W, generator=gen)).to(DEV)
        g, b = (1 + 0.2 * torch.randn(W, generator=gen)).to(DEV), (0.2 * torch.randn(W, generator=gen)).to(DEV)
        src = po.view(n, npch, W)
        if cls:
            src = torch.cat([ct.expand(n, 1, W), src], 1)
        s = (src + pos).reshape(n * T, W)                           # the kernel's single fp32 addition
        for ln in (False, True):
            for x_bf16 in (0, 1):
                x = _sent_bf16(n * T + 1, W) if x_bf16 else _sent_f32(n * T + 1, W)
                _sync_check(lib.mq_vit_assemble(po.data_ptr(), ct.data_ptr() if cls else None, pos.data_ptr(), g.data_ptr() if ln else None,
                                                b.data_ptr() if ln else None, x.data_ptr(), n, T, W, eps, x_bf16, _stream()), "mq_vit_assemble")
                what = f"vit_assemble cls={cls} ln={ln} bf16={x_bf16}"
                if not ln:
                    assert torch.equal(_bits(x[:n * T]), _bits(s.to(x.dtype))), what
                else:
                    sd = s.double()
                    nrm = (sd - sd.mean(1, keepdim=True)) / torch.sqrt(sd.var(1, unbiased=False, keepdim=True) + eps)
                    ng, bb, gg = nrm * g.double(), b.double(), g.double().abs()
                    tol = ULP * (ng.abs() + bb.abs()) + 2.0 ** -12 * gg if x_bf16 else 2.0 ** -16 * (ng.abs() + bb.abs() + gg)
                    _within(x[:n * T], ng + bb, tol, what)
                tail = _bits(x[n * T:])
                assert bool((tail == SENT16).all() if x_bf16 else x[n * T:].isnan().all()), f"{what}: the row past the call changed"


# ---- mq_patchify: image -> bf16 im2col rows (ToTensor + Normalize fused for uint8) ------------------------------------------------------------
def _patchify(lib, src_ptr, is_u8, n, S, P, Kp, mean, std):
    G = S // P
    out = _sent_bf16(n * G * G + 1, Kp)
    m, sd = (C.c_float * 3)(*mean), (C.c_float * 3)(*std)           # host pointers
    _sync_check(lib.mq_patchify(src_ptr, is_u8, out.data_ptr(), n, S, P, Kp, C.addressof(m), C.addressof(sd), _stream()), "mq_patchify")
    return out


@pytest.mark.parametrize("P,S,Kp", [(4, 256, 64), (14, 224, 640), (14, 336, 640), (16, 224, 768), (16, 384, 768), (32, 224, 3072)])
@pytest.mark.parametrize("u8", [True, False])
def test_patchify_matches_torch_bit_for_bit(P, S, Kp, u8):
    lib = L.load()
    n, G, K = 2, S // P, 3 * P * P
    gen = torch.Generator().manual_seed(P * S)
    if u8:
        img = torch.randint(0, 256, (n, S, S, 3), generator=gen, dtype=torch.uint8)
        # torch's fp32 (b / 255 - mean) / std with true divisions (full-size divisors: a scalar divisor is turned into a reciprocal multiply)
        t = img.permute(0, 3, 1, 2).float()
        mean = torch.tensor(OPENAI_DATASET_MEAN, dtype=torch.float32).view(1, 3, 1, 1)
        std = torch.tensor(OPENAI_DATASET_STD, dtype=torch.float32).view(1, 3, 1, 1)
        t = (t / torch.full_like(t, 255.0) - mean) / std.expand_as(t).contiguous()
        dev = img.to(DEV)
        out = _patchify(lib, dev.data_ptr(), 1, n, S, P, Kp, OPENAI_DATASET_MEAN, OPENAI_DATASET_STD)
        # the same pixels one byte into a larger buffer: not 8-byte aligned, so the generic kernel runs (P % 8 == 0 otherwise takes u8x8)
        raw = torch.zeros(img.numel() + 16, dtype=torch.uint8, device=DEV)
        raw[1:1 + img.numel()] = dev.view(-1)
        out_generic = _patchify(lib, raw.data_ptr() + 1, 1, n, S, P, Kp, OPENAI_DATASET_MEAN, OPENAI_DATASET_STD)
        assert torch.equal(_bits(out), _bits(out_generic)), "the uint8 fast path and the generic kernel disagree"
    else:
        t = torch.randn(n, 3, S, S, generator=gen)
        dev = t.to(DEV)
        out = _patchify(lib, dev.data_ptr(), 0, n, S, P, Kp, (0.0,) * 3, (1.0,) * 3)
    ref = t.reshape(n, 3, G, P, G, P).permute(0, 2, 4, 1, 3, 5).reshape(n * G * G, K).to(torch.bfloat16).to(DEV)
    assert torch.equal(_bits(out[:n * G * G, :K]), _bits(ref)), "patch columns differ from torch"
    assert bool((_bits(out[:n * G * G, K:]) == 0).all()), "columns >= 3 P^2 are not exactly 0"
    assert bool((_bits(out[n * G * G:]) == SENT16).all()), "the row past the call changed"


# ---- mq_avg_tokens, mq_move_rows, mq_cls_rows / mq_last_rows --------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [768, 1152])
@pytest.mark.parametrize("x_bf16", [0, 1])
@pytest.mark.parametrize("T,first", [(50, 1), (50, 0), (2, 1), (1, 0)])
def test_avg_tokens_matches_fp64(W, x_bf16, T, first):
    lib = L.load()
    n = 3
    gen = torch.Generator().manual_seed(W + T + first)
    x = torch.randn(n * T, W, generator=gen).to(torch.bfloat16 if x_bf16 else torch.float32).to(DEV)
    out = _sent_f32(n + 1, W)
    _sync_check(lib.mq_avg_tokens(x.data_ptr(), x_bf16, out.data_ptr(), n, T, first, W, _stream()), "mq_avg_tokens")
    seg = x.double().view(n, T, W)[:, first:]
    if T - first == 1:
        assert torch.equal(_bits(out[:n]), _bits(x.float().view(n, T, W)[:, first])), "the mean of one row is that row"
    L_ = T - first
    _within(out[:n], seg.mean(1), 2 * (L_ * 2.0 ** -24 + 2.0 ** -22) * seg.abs().mean(1), "avg_tokens")
    assert bool(out[n:].isnan().all())


@pytest.mark.parametrize("n,row_bytes", [(0, 1536), (37, 16), (300, 1536), (3000, 16384)])   # 3000 x 1024 chunks wraps the 8192-workgroup grid
def test_move_rows_gather_and_scatter(n, row_bytes):
    lib = L.load()
    S = max(2 * n, 8)
    gen = torch.Generator().manual_seed(n + row_bytes)
    sparse = torch.randint(0, 256, (S, row_bytes), generator=gen, dtype=torch.uint8).to(DEV)
    idx = torch.randint(0, S, (max(n, 1),), generator=gen, dtype=torch.int32)
    if n > 1:
        idx[1] = idx[0]                                             # repeated indices are fine for a gather
    idx = idx.to(DEV)
    dense = torch.full((n + 1, row_bytes), 0xA5, dtype=torch.uint8, device=DEV)
    _sync_check(lib.mq_move_rows(sparse.data_ptr(), idx.data_ptr(), dense.data_ptr(), n, row_bytes, 0, _stream()), "mq_move_rows gather")
    assert torch.equal(dense[:n], sparse[idx[:n].long()])
    assert bool((dense[n:] == 0xA5).all()), "gather wrote past its n rows"
    # scatter: distinct destinations into a sentinel-filled buffer; every row not named stays as it was
    perm = torch.randperm(S, generator=gen)[:n].to(torch.int32).to(DEV) if n else torch.zeros(1, dtype=torch.int32, device=DEV)
    src = torch.randint(0, 256, (max(n, 1), row_bytes), generator=gen, dtype=torch.uint8).to(DEV)
    dst = torch.full((S, row_bytes), 0x5A, dtype=torch.uint8, device=DEV)
    _sync_check(lib.mq_move_rows(dst.data_ptr(), perm.data_ptr(), src.data_ptr(), n, row_bytes, 1, _stream()), "mq_move_rows scatter")
    named = torch.zeros(S, dtype=torch.bool, device=DEV)
    named[perm[:n].long()] = True
    assert torch.equal(dst[perm[:n].long()], src[:n])
    assert bool((dst[~named] == 0x5A).all()), "scatter touched rows it was not given"


def test_cls_and_last_rows():
    lib = L.load()
    lens = [1, 5, 1, 300, 2]
    cu = _cu(lens)
    rows = torch.full((len(lens) + 1,), -5, dtype=torch.int32, device=DEV)
    _sync_check(lib.mq_last_rows(cu.data_ptr(), rows.data_ptr(), len(lens), _stream()), "mq_last_rows")
    assert rows.tolist() == [0, 5, 6, 306, 308, -5]
    n, T = 600, 577                                                 # more than one 256-thread block
    cls = torch.full((n + 1,), -5, dtype=torch.int32, device=DEV)
    _sync_check(lib.mq_cls_rows(cls.data_ptr(), n, T, _stream()), "mq_cls_rows")
    assert cls.tolist() == [i * T for i in range(n)] + [-5]

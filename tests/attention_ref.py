"""Reference, rounding budget, arithmetic model and input families for the tests of csrc/attention.hip
(tests/test_attention_ref_host.py, tests/test_attention_gpu.py, tests/test_kernels_gpu.py).  A plain helper module: nothing here calls
the library.

Conventions (those of the kernel): `qkv` is bf16 [rows, 3 * W], W = heads * hs, the columns are [q | k | v] and head h owns columns
h * hs .. h * hs + hs - 1 of each third; the sequences are packed one after the other, `lens` holds their lengths (a length of 0 is an
empty sequence); the softmax scale is 1 / sqrt(hs) with hs the head STRIDE (the 80 / 88 / 104-wide heads padded to 96 / 112 are
rescaled by the loader, tests/test_pad_heads.py)."""
import math

import torch

MASK_NONE, MASK_CAUSAL, MASK_CAUSAL_CLS = 0, 1, 2
U = 2.0 ** -8            # unit roundoff of bf16 (8 significant bits, round to nearest even)
KEEP_P_ROWS = 200        # reference() returns the probabilities themselves for sequences up to this long

FAMILIES = ("randn", "peaked", "readout", "ramp_up", "ramp_down", "padded_heads")
MUTANTS = ("dup_last", "causal_plus1", "causal_minus_self", "cls_drop", "cls_len1", "skip_tile", "l_no_alpha", "o_no_alpha", "l_from_bf16")


def allowed(ln, mask, device="cpu"):
    """[query, key] boolean: which keys a query sees.  MASK_CAUSAL_CLS (include/marqo_hip.h): causal, and row len-1 (the appended class
    token) does not see key len-1 — unless len == 1, where the row would otherwise see nothing."""
    q = torch.arange(ln, device=device)[:, None]
    k = torch.arange(ln, device=device)[None, :]
    ok = torch.ones(ln, ln, dtype=torch.bool, device=device) if mask == MASK_NONE else (k <= q)
    if mask == MASK_CAUSAL_CLS and ln > 1:
        ok = ok.clone()
        ok[ln - 1, ln - 1] = False
    return ok


def _heads_of(blk, heads, hs):
    """[B, ln, W] -> [B, heads, ln, hs]"""
    B, ln, _ = blk.shape
    return blk.reshape(B, ln, heads, hs).transpose(1, 2)


def reference(qkv_bf16, lens, heads, hs, mask, bias=None, keep_p=False):
    """float64 attention on the device of `qkv_bf16`: returns (out, absout, P) with out = P V and absout = P |V|, both float64 [rows, W];
    P is a list with one [heads, len, len] tensor per sequence when keep_p is set and every sequence has at most KEEP_P_ROWS rows, else None.
    `bias` is the relative-position bias itself (NOT premultiplied by sqrt(hs)): [heads, 2 * span - 1], entry (h, d + span - 1) is added to
    the scaled score of key - query == d."""
    W = heads * hs
    dev = qkv_bf16.device
    rows = qkv_bf16.shape[0]
    assert qkv_bf16.dtype == torch.bfloat16 and qkv_bf16.shape[1] == 3 * W and rows == sum(lens)
    out = torch.zeros(rows, W, dtype=torch.float64, device=dev)
    absout = torch.zeros(rows, W, dtype=torch.float64, device=dev)
    keep_p = keep_p and max(lens, default=0) <= KEEP_P_ROWS
    P = [] if keep_p else None
    fixed = len(lens) > 1 and len(set(lens)) == 1 and lens[0] > 0
    groups = [(0, len(lens), lens[0])] if fixed else None
    if groups is None:
        groups, r0 = [], 0
        for ln in lens:
            groups.append((r0, 1, ln))
            r0 += ln
    for r0, B, ln in groups:
        if ln == 0:
            if keep_p:
                P.append(torch.zeros(heads, 0, 0, dtype=torch.float64, device=dev))
            continue
        blk = qkv_bf16[r0:r0 + B * ln].double().reshape(B, ln, 3 * W)
        q, k, v = (_heads_of(t, heads, hs) for t in blk.split(W, dim=2))
        s = q @ k.transpose(2, 3) / math.sqrt(hs)
        if bias is not None:
            span = (bias.shape[1] + 1) // 2
            pos = torch.arange(ln, device=dev)
            s = s + bias.double()[:, (pos[None, :] - pos[:, None]) + span - 1][None]
        s = s.masked_fill(~allowed(ln, mask, dev), float("-inf"))
        p = torch.softmax(s, dim=-1)
        out[r0:r0 + B * ln] = (p @ v).transpose(1, 2).reshape(B * ln, W)
        absout[r0:r0 + B * ln] = (p @ v.abs()).transpose(1, 2).reshape(B * ln, W)
        if keep_p:
            P.extend(p[b] for b in range(B))
    return out, absout, P


def budget(out, absout, out_fp8=False):
    """Elementwise bound on |kernel - reference|, derived from the kernel's arithmetic, not tuned:  u * (P|V| + |out|),  u = 2**-8.

    - bf16 has 8 significant bits: rounding to nearest changes a value by at most u = 2**-8 of its magnitude.
    - The kernel rounds every unnormalised probability p_k to bf16 before the P.V product (the MFMA's B operand): each term p_k * v_k of the sum is
      off by at most u * p_k * |v_k|.  The normaliser l is the fp32 sum of the UNROUNDED probabilities, so after the division by l the error is at
      most u * sum_k P_k |v_k| = u * (P|V|).
    - The normalised value is then rounded to bf16 once more for the store: at most u * |out|.
    - Everything else is fp32 and two orders of magnitude smaller (2**-24 per operation against 2**-8): the Q.K accumulation of exact bf16 x bf16
      products, v_exp_f32, the alpha rescale of the running sums, the reciprocal of l.  The callers allow a factor for these (1.0 for the arithmetic
      model below, 1.25 for the kernel).
    - The fp8 output is converted from the fp32 value directly: no bf16 store rounding, the budget before the e4m3 rounding is u * (P|V|) alone."""
    return U * absout if out_fp8 else U * (absout + out.abs())


def ratio_to_budget(got, out, absout, out_fp8=False):
    """elementwise |got - out| / budget (0 where both are 0, inf where the error is non-zero against a zero budget or not finite)"""
    err = (got.double() - out).abs()
    b = budget(out, absout, out_fp8)
    r = torch.where(b > 0, err / b, torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
    return torch.where(torch.isfinite(err), r, torch.full_like(err, float("inf")))


def worst_ratio(got, out, absout, out_fp8=False):
    r = ratio_to_budget(got, out, absout, out_fp8)
    return float(r.max()) if r.numel() else 0.0


def worst_coords(got, out, absout, lens, heads, hs):
    """where the worst ratio sits, in the kernel's coordinates: (ratio, sequence, head, query, query block, column)"""
    r = ratio_to_budget(got, out, absout)
    i = int(r.argmax())
    row, col = divmod(i, r.shape[1])
    seq, r0 = 0, 0
    for seq, ln in enumerate(lens):
        if row < r0 + ln:
            break
        r0 += ln
    return dict(ratio=float(r.flatten()[i]), seq=seq, len=lens[seq], head=col // hs, query=row - r0, qblk=(row - r0) // 16, col=col % hs,
                got=float(got.flatten()[i]), ref=float(out.flatten()[i]))


def emulate(qkv_bf16, lens, heads, hs, mask, mutant=None):
    """torch-CPU model of the kernel's arithmetic, per (sequence, head), every query in parallel:
    fp32 raw scores; 64-key tiles with a running max m (from -1e30) and a running sum l; p = exp2(s * c - m * c) with c = log2(e) / sqrt(hs);
    the probabilities are rounded to bf16 for the P.V product but summed unrounded; the fp32 accumulators are rescaled by alpha = exp2((m_old - m) * c);
    the result is o * (1 / l), stored as bf16.  Keys past the sequence in the ragged last tile are copies of key len-1 (the kernel's staging clamps) with
    a score of -inf.  (A tile a causal query block never reaches is skipped by the kernel; here it is all -inf: p = 0, alpha = 1 — the same numbers.)

    `mutant` switches ONE deliberate fault on (MUTANTS), for the host test that shows the budget can see them:
      dup_last           key `len` is admitted in the ragged tile: key len-1 counted twice (an off-by-one in `key < len`)
      causal_plus1       causal admits key q + 1
      causal_minus_self  causal excludes key q
      cls_drop           MASK_CAUSAL_CLS without the class row's self-exclusion
      cls_len1           the self-exclusion applied at len == 1 too
      skip_tile          key tile 5 (keys 320..383) is skipped in sequences of more than 640 keys
      l_no_alpha         the running sum is not rescaled when the max moves
      o_no_alpha         the accumulators are not rescaled when the max moves
      l_from_bf16        the normaliser is summed from the bf16-rounded probabilities"""
    assert mutant is None or mutant in MUTANTS
    W = heads * hs
    x = qkv_bf16.cpu()
    rows = x.shape[0]
    out = torch.zeros(rows, W, dtype=torch.bfloat16)
    c = torch.tensor(1.44269504088896340736 / math.sqrt(hs), dtype=torch.float32)
    NEG = float("-inf")
    r0 = 0
    for ln in lens:
        if ln == 0:
            continue
        blk = x[r0:r0 + ln].float().reshape(1, ln, 3 * W)
        q, k, v = (_heads_of(t, heads, hs)[0] for t in blk.split(W, dim=2))     # [heads, ln, hs]
        nkt = (ln + 63) // 64
        kp = nkt * 64
        kidx = torch.arange(kp).clamp(max=ln - 1)
        k, v = k[:, kidx], v[:, kidx]
        key = torch.arange(kp)[None, :]
        qi = torch.arange(ln)[:, None]
        valid = key < (ln + 1 if mutant == "dup_last" else ln)
        if mask != MASK_NONE:
            lim = qi + 1 if mutant == "causal_plus1" else qi
            valid = valid & ((key < lim) if mutant == "causal_minus_self" else (key <= lim))
        else:
            valid = valid.expand(ln, kp)
        if mask == MASK_CAUSAL_CLS and mutant != "cls_drop" and (ln > 1 or mutant == "cls_len1"):
            valid = valid & ~((qi == ln - 1) & (key == ln - 1))
        s = (q @ k.transpose(1, 2)).masked_fill(~valid[None], NEG)            # raw fp32 scores [heads, ln, kp]
        m = torch.full((heads, ln, 1), -1e30, dtype=torch.float32)
        l = torch.zeros(heads, ln, 1, dtype=torch.float32)
        o = torch.zeros(heads, ln, hs, dtype=torch.float32)
        for kt in range(nkt):
            if mutant == "skip_tile" and ln > 640 and kt == 5:
                continue
            st = s[:, :, kt * 64:kt * 64 + 64]
            m_new = torch.maximum(m, st.max(dim=-1, keepdim=True).values)
            p = torch.exp2(st * c - m_new * c)
            pb = p.to(torch.bfloat16).float()
            alpha = torch.exp2((m - m_new) * c)
            l = (l if mutant == "l_no_alpha" else l * alpha) + (pb if mutant == "l_from_bf16" else p).sum(-1, keepdim=True)
            o = (o if mutant == "o_no_alpha" else o * alpha) + pb @ v[:, kt * 64:kt * 64 + 64]
            m = m_new
        res = (o * (1.0 / l)).to(torch.bfloat16)
        out[r0:r0 + ln] = res.transpose(0, 1).reshape(ln, W)
        r0 += ln
    return out


# ---- input families: all built as bf16, so the reference sees exactly what the kernel sees -----------------------------------------------

REAL_DIMS = {96: (80,), 112: (88, 104)}     # the head widths a padded stride carries (ViT-H / g / bigG)


def readout_v(lens, heads, hs, reserve_last=False):
    """V of the `readout` family, fp32 [rows, heads, hs]: the row of key j of sequence s is one-hot at column (j + s) % n; keys of the second and later
    wraps (j >= n) carry 0.5 at column (j + s + j // n) % n as well, so that keys which share a column differ in their second one.  n = hs — or, with
    reserve_last, hs - 1 for every key but the LAST of a sequence, which alone owns column hs - 1 (the class row of MASK_CAUSAL_CLS must then read
    exactly 0.0 there)."""
    rows = sum(lens)
    v = torch.zeros(rows, heads, hs)
    n = hs - 1 if reserve_last else hs
    r0 = 0
    for s, ln in enumerate(lens):
        j = torch.arange(ln)
        v[r0 + j, :, (j + s) % n] = 1.0
        w = j[j >= n]
        v[r0 + w, :, (w + s + w // n) % n] += 0.5
        if reserve_last and ln > 0:
            v[r0 + ln - 1] = 0.0
            v[r0 + ln - 1, :, hs - 1] = 1.0
        r0 += ln
    return v


def make_qkv(family, lens, heads, hs, seed=0, device="cpu", real=None, reserve_last=False):
    """bf16 [sum(lens), 3 * heads * hs] of one family (module docstring of tests/test_attention_gpu.py); built on the CPU from `seed`, so the host and
    the GPU tests see the same numbers."""
    assert family in FAMILIES
    g = torch.Generator().manual_seed(seed)
    rows, W = sum(lens), heads * hs
    q = torch.randn(rows, heads, hs, generator=g)
    k = torch.randn(rows, heads, hs, generator=g)
    v = torch.randn(rows, heads, hs, generator=g)
    if family == "peaked":
        # sharp softmax rows, and keys whose values span four decades: the budget follows P|V|, so large and small keys are each checked at their own scale
        q = q * 4.0
        v = v * 10.0 ** (torch.rand(rows, heads, 1, generator=g) * 4.0 - 2.0)
    elif family == "readout":
        v = readout_v(lens, heads, hs, reserve_last)
    elif family in ("ramp_up", "ramp_down"):
        # constant q, k proportional to the key index (tile index and index inside the tile in two dims, both exact in bf16): the scaled score moves by
        # a * log2(e) / sqrt(hs) log2 units per 64-key tile, a = 64 / 32 / 16 by head -> 11.5 / 5.8 / 2.9 (hs 64), 8.2 / 4.1 / 2.0 (hs 128).  ramp_up moves
        # the running max in every tile (and past ~11 tiles at a = 64 the early tiles' share is below fp32's range: exactly 0); ramp_down has its max at
        # key 0, so every later tile takes the no-rescale path
        sign = 1.0 if family == "ramp_up" else -1.0
        q = torch.zeros(rows, heads, hs)
        a = 64.0 / 2.0 ** (torch.arange(heads) % 3)
        q[:, :, 0] = a
        q[:, :, 1] = a
        pos = torch.cat([torch.arange(ln) for ln in lens]) if rows else torch.zeros(0, dtype=torch.long)
        k[:, :, 0] = (sign * (pos // 64).float())[:, None]
        k[:, :, 1] = (sign * (pos % 64).float() / 64.0)[:, None]
    elif family == "padded_heads":
        real = real if real is not None else REAL_DIMS[hs][0]
    if real is not None and real < hs:       # the pad columns of q, k and v are zero, as the loader leaves them
        q[:, :, real:] = 0
        k[:, :, real:] = 0
        v[:, :, real:] = 0
    qkv = torch.cat([q.reshape(rows, W), k.reshape(rows, W), v.reshape(rows, W)], dim=1).to(torch.bfloat16)
    return qkv.to(device)


def cu_seqlens(lens, device="cpu"):
    cu = [0]
    for ln in lens:
        cu.append(cu[-1] + ln)
    return torch.tensor(cu, dtype=torch.int32, device=device)

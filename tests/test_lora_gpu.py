"""csrc/lora.hip on the device: mq_lora_down and mq_lora_up in each mode (through torch.ops.marqo_hip.mq_lora_* and, for the refusals and the leading
dimension, the C ABI) against their float64 statement (tests/jina_v3_ref.py::lora_down_ref / lora_up_ref), per element:

    |kernel - reference| <= 1.25 x budget

with the budgets derived there from the operand roundings (down: (K + 1) 2^-24 |scale| sum |x a| — the products of bf16 values are exact in fp32, the
adds are not; up: r 2^-24 sum |T b|, plus the fp32 add, the GELU polynomial's contract and the bf16 store where the mode has them); the 1.25 is
tests/test_attention_gpu.py's allowance (MARGIN), not a fitted number.

Shapes: K in {64, 1024} x R in {4, 12, 64} x tasks in {1, 2, 5} for the down half; (r, column blocks, N) in (4, 1, 4 / 192 / 1028), (4, 3, 192),
(12, 1, 4 / 1028), (16, 4, 192), (16, 1, 1028) for the up half in all four forms.  Rows: the packed lengths (1, 63, 65, 3) — task changes inside a
16-row tile (row 1), on a tile edge (row 64), one row past the 128-row workgroup (row 129); 132 rows, no multiple of 128 — and (40, 24, 64, 7, 2), 137
rows; one sequence of every pack has task -1; and fixed_len 33 x 4.  Rows without adapter: T and the written delta are +0.0 bit for bit, an
accumulate / in-place target keeps its bits, the GELU form gives the bits of the pure activation pass.  Every output sits between guard rows and (up)
in front of four guard columns (ldc = N + 4).

Measured on an MI355X (LORA_RATIO lines), worst |kernel - reference| / budget: down 0.022 (its budget is a worst-case bound linear in K: 0.022 at K = 64,
0.0015 at K = 1024); up accumulate 0.84, write 0.76, in place 1.00, in place + GELU 0.99 (the last two are the bf16 store's half ulp)."""
import pytest
import torch

from marqo_amd import _lib as L
from tests import jina_v3_ref as N
from tests.test_attention_gpu import MARGIN

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 8
PACKS = {"a": (1, 63, 65, 3), "b": (40, 24, 64, 7, 2)}
SENT = 1234.5


@pytest.fixture(scope="module")
def ops():
    return L.load_torch_ops()


def _tasks_of(lens, tasks, shift=0):
    """one task per sequence, cycling through the adapters, the second sequence without one"""
    return [-1 if i == 1 else (i + shift) % tasks for i in range(len(lens))]


def _seqs(lens, seq_task, fixed=False):
    h = torch.tensor(seq_task, dtype=torch.int32)
    cu = None if fixed else torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32, device=DEV)
    row_task = h.to(DEV).long()[N.seq_of_rows(lens, DEV)]
    return h.to(DEV), h, cu, (lens[0] if fixed else 0), row_task


def _operands(rows, K, R, tasks, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, K, generator=g).to(torch.bfloat16).to(DEV)
    A = (torch.randn(tasks, R, K, generator=g) / K ** 0.5).to(torch.bfloat16).to(DEV)
    scale = (0.5 + torch.rand(tasks, generator=g) * 2).to(DEV)
    return x, A, scale


def _ratio(got, ref, budget):
    """worst |got - ref| / budget; where the budget is 0 the values must be equal"""
    err = (got.double() - ref).abs()
    assert bool((err[budget == 0] == 0).all()), "a value with no rounding in its derivation differs"
    return float((err / budget.clamp(min=1e-300))[budget > 0].max()) if bool((budget > 0).any()) else 0.0


# ---- down -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tasks", (1, 2, 5))
@pytest.mark.parametrize("R", (4, 12, 64))
@pytest.mark.parametrize("K", (64, 1024))
def test_down_within_the_rounding_budget(ops, K, R, tasks):
    for name, lens, fixed in (("a", PACKS["a"], False), ("b", PACKS["b"], False), ("fixed33", (33,) * 4, True)):
        rows = sum(lens)
        d_task, h_task, cu, fl, row_task = _seqs(lens, _tasks_of(lens, tasks), fixed)
        x, A, scale = _operands(rows, K, R, tasks, seed=K + R + tasks)
        T = ops.mq_lora_down(x, A, scale, d_task, h_task, cu, fl)
        torch.cuda.synchronize()
        ref, budget = N.lora_down_ref(x, A, scale, row_task)
        r = _ratio(T, ref, budget)
        print(f"LORA_RATIO down K={K} R={R} tasks={tasks} rows={name}: {r:.4f}")
        assert r <= MARGIN
        off = row_task < 0
        assert bool(off.any()) and bool((T[off].view(torch.int32) == 0).all())          # rows without adapter: +0.0, bit for bit
        assert float(T[~off].abs().min()) > 0


def test_down_reads_lda_and_writes_only_its_rows():
    lib = L.load()
    lens, K, R, tasks, lda = PACKS["a"], 64, 12, 2, 96
    rows = sum(lens)
    d_task, h_task, cu, _, row_task = _seqs(lens, _tasks_of(lens, tasks))
    x, A, scale = _operands(rows, K, R, tasks, seed=3)
    wide = torch.full((rows, lda), float("nan"), dtype=torch.bfloat16, device=DEV)
    wide[:, :K] = x
    buf = torch.full((rows + 2 * GUARD, R), SENT, dtype=torch.float32, device=DEV)
    L.check(lib.mq_lora_down(wide.data_ptr(), lda, A.data_ptr(), scale.data_ptr(), d_task.data_ptr(), h_task.data_ptr(), cu.data_ptr(), len(lens), 0, rows,
                             tasks, R, K, buf[GUARD:].data_ptr(), torch.cuda.current_stream().cuda_stream), "mq_lora_down")
    torch.cuda.synchronize()
    assert bool((buf[:GUARD] == SENT).all()) and bool((buf[GUARD + rows:] == SENT).all())
    ref, budget = N.lora_down_ref(x, A, scale, row_task)
    assert _ratio(buf[GUARD:GUARD + rows], ref, budget) <= MARGIN


def test_one_wrong_task_shows(ops):
    """two adapters that differ in ONE column of A: rows of task 0 and rows of task 1 are each checked against their own adapter, and the other
    adapter's product is shown to leave the bar on the same rows"""
    lens, K, R = PACKS["a"], 1024, 12
    rows = sum(lens)
    seq_task = [0, 1, 0, 1]
    d_task, h_task, cu, fl, row_task = _seqs(lens, seq_task)
    x, A, scale = _operands(rows, K, R, 2, seed=9)
    scale[:] = 1.0
    A[0, :, 517] = 0.5
    A[1] = A[0]
    A[1, :, 517] = -0.5
    x[:, 517] = 4.0
    T = ops.mq_lora_down(x, A, scale, d_task, h_task, cu, fl)
    torch.cuda.synchronize()
    ref, budget = N.lora_down_ref(x, A, scale, row_task)
    swapped, _ = N.lora_down_ref(x, A, scale, 1 - row_task)
    for t in (0, 1):
        sel = row_task == t
        assert _ratio(T[sel], ref[sel], budget[sel]) <= MARGIN
        assert float(((swapped[sel] - ref[sel]).abs() / budget[sel]).min()) > 100 * MARGIN


# ---- up -------------------------------------------------------------------------------------------------------------------------------------------------
UP_SHAPES = [(4, 1, 4), (4, 1, 192), (4, 1, 1028), (4, 3, 192), (12, 1, 4), (12, 1, 1028), (16, 4, 192), (16, 1, 1028)]
FORMS = {"accumulate": (L.MQ_LORA_ACCUM, 0), "write": (L.MQ_LORA_WRITE, 0), "inplace": (L.MQ_LORA_INPLACE, 0), "inplace_gelu": (L.MQ_LORA_INPLACE, L.MQ_ACT_GELU)}


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("r, nblocks, Ncols", UP_SHAPES)
def test_up_within_the_rounding_budget(ops, r, nblocks, Ncols, form):
    mode, act = FORMS[form]
    R = r * nblocks
    for tasks, (name, lens, fixed) in zip((1, 2, 5), (("a", PACKS["a"], False), ("b", PACKS["b"], False), ("fixed33", (33,) * 4, True))):
        rows, ldc = sum(lens), Ncols + 4
        d_task, h_task, cu, fl, row_task = _seqs(lens, _tasks_of(lens, tasks, shift=1), fixed)
        g = torch.Generator().manual_seed(r + nblocks + Ncols + tasks)
        T = torch.randn(rows, R, generator=g).to(DEV)
        B = torch.randn(tasks, Ncols, r, generator=g).to(torch.bfloat16).to(DEV)
        dt = torch.bfloat16 if mode == L.MQ_LORA_INPLACE else torch.float32
        out0 = (torch.randn(rows, Ncols, generator=g) * 2).to(dt).to(DEV)
        buf = torch.full((rows + 2 * GUARD, ldc), SENT, dtype=dt, device=DEV)
        buf[GUARD:GUARD + rows, :Ncols] = out0
        ops.mq_lora_up(T, B, nblocks, d_task, h_task, cu, fl, buf[GUARD:GUARD + rows], mode, act)
        torch.cuda.synchronize()
        assert bool((buf[:GUARD] == SENT).all()) and bool((buf[GUARD + rows:] == SENT).all()) and bool((buf[:, Ncols:] == SENT).all())
        got = buf[GUARD:GUARD + rows, :Ncols]
        ref, budget = N.lora_up_ref(T, B, row_task, nblocks, out0, {L.MQ_LORA_ACCUM: "accumulate", L.MQ_LORA_WRITE: "write"}.get(mode, "inplace"), bool(act))
        ratio = _ratio(got, ref, budget)
        print(f"LORA_RATIO up {form} r={r} blocks={nblocks} N={Ncols} tasks={tasks} rows={name}: {ratio:.4f}")
        assert ratio <= MARGIN
        off = row_task < 0
        assert bool(off.any())
        if form == "write":
            assert bool((got[off].view(torch.int32) == 0).all())                          # +0.0, bit for bit
        elif form == "inplace_gelu":   # the bits of the pure activation pass: the same call with no adapter anywhere
            alone = out0.clone()
            none = torch.full_like(h_task, -1)
            ops.mq_lora_up(T, B, nblocks, none.to(DEV), none, cu, fl, alone, mode, act)
            torch.cuda.synchronize()
            assert torch.equal(got[off].view(torch.int16), alone[off].view(torch.int16))
            assert not torch.equal(alone.view(torch.int16), out0.view(torch.int16))
        else:
            assert torch.equal(got[off].view(torch.int16 if dt == torch.bfloat16 else torch.int32), out0[off].view(torch.int16 if dt == torch.bfloat16 else torch.int32))
        assert not torch.equal(got[~off].float(), out0[~off].float())


def test_down_then_up_is_the_stacked_qkv_delta(ops):
    """the two halves chained as the tower chains them: q | k | v adapters stacked on one input, each column block reading its own r columns of T"""
    lens, K, r, tasks = PACKS["b"], 128, 4, 5
    rows, Ncols = sum(lens), 3 * K
    d_task, h_task, cu, fl, row_task = _seqs(lens, _tasks_of(lens, tasks))
    x, A, scale = _operands(rows, K, 3 * r, tasks, seed=21)
    B = torch.randn(tasks, Ncols, r, generator=torch.Generator().manual_seed(22)).to(torch.bfloat16).to(DEV)
    T = ops.mq_lora_down(x, A, scale, d_task, h_task, cu, fl)
    out = torch.full((rows, Ncols), SENT, dtype=torch.float32, device=DEV)
    ops.mq_lora_up(T, B, 3, d_task, h_task, cu, fl, out, L.MQ_LORA_WRITE, 0)
    torch.cuda.synchronize()
    t = row_task.clamp(min=0)
    want = torch.zeros(rows, Ncols, dtype=torch.float64, device=DEV)
    for b in range(3):      # scale (x A_b^T) B_b^T, block by block
        Tb = torch.einsum("mk,mrk->mr", x.double(), A.double()[t][:, b * r:(b + 1) * r]) * scale.double()[t][:, None]
        want[:, b * K:(b + 1) * K] = torch.einsum("mr,mnr->mn", Tb, B.double()[t][:, b * K:(b + 1) * K])
    want *= (row_task >= 0)[:, None]
    mag = want.abs().max()
    assert float((out.double() - want).abs().max()) <= 1e-5 * float(mag) and float(mag) > 0.1


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    lib = L.load()
    lens, K, R, tasks = PACKS["a"], 64, 12, 2
    rows = sum(lens)
    d_task, h_task, cu, _, _ = _seqs(lens, [0, 1, 0, -1])
    x, A, scale = _operands(rows, 128, 64, tasks, seed=1)
    T = torch.full((rows, 80), SENT, dtype=torch.float32, device=DEV)
    s = torch.cuda.current_stream().cuda_stream
    bad_task = torch.tensor([0, 2, 0, -1], dtype=torch.int32)

    def down(R=R, K=K, h=h_task):
        return lib.mq_lora_down(x.data_ptr(), 128, A.data_ptr(), scale.data_ptr(), d_task.data_ptr(), h.data_ptr(), cu.data_ptr(), len(lens), 0, rows, tasks, R,
                                K, T.data_ptr(), s)

    def up(R=R, r=4, nb=3, h=h_task, mode=L.MQ_LORA_WRITE):
        return lib.mq_lora_up(T.data_ptr(), R, A.data_ptr(), r, nb, d_task.data_ptr(), h.data_ptr(), cu.data_ptr(), len(lens), 0, rows, tasks, x.data_ptr(), 128,
                              12, mode, 0, s)
    for call, what in ((lambda: down(R=68), b"R 68"), (lambda: down(K=96), b"K 96 must be a multiple of 64"),
                       (lambda: down(h=bad_task), b"task id 2 of sequence 1 is not below tasks 2"), (lambda: up(R=68, r=17, nb=4), b"rank 17"),
                       (lambda: up(h=bad_task), b"task id 2 of sequence 1"), (lambda: up(mode=7), b"bad mode 7")):
        rc = call()
        torch.cuda.synchronize()
        assert rc == -1 and what in lib.mq_last_error(), lib.mq_last_error()
    assert bool((T == SENT).all()) and bool(torch.isfinite(x.float()).all())

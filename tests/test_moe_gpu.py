"""The routed-MLP kernels of csrc/moe.hip on the GPU, per element against the float64 statements of tests/nomic_moe_ref.py: |got - ref| <= MARGIN x budget
(MARGIN = 1.25, tests/test_attention_gpu.py; the budgets are derived in the reference's docstrings, never from the kernels' output).  Route: indices on
every decided row (and on ties: the lower index), weights within budget.  Grouped MLP through mq_moe_mlp under forced routings: segments of 0, 1, BM - 1,
BM, BM + 1 rows, everything to one expert, the first and last expert empty, both tile heights, (W, F) = (64, 64) and (768, 192), k = 1 and 2, Y between
guard rows, the index maps inverse and ordered.  One wrong expert shows; a token's bits do not depend on the batch; mq_moe_combine_ln.
Measured on an MI355X (MOE_RATIO lines, worst |got - ref| / budget): route weights 0.001 (26 tied rows at E = 8, none undecided); grouped MLP 0.40
(bm 128, W 64) / 0.19 (bm 128, W 768) / 0.40 (bm 32, W 64) / 0.16 (bm 32, W 768); the wrong expert: own 0.32, the other 73; combine 0.18 / 0.13."""
import pytest
import torch

from marqo_amd import _lib as L
from tests import nomic_moe_ref as M
from tests.test_attention_gpu import MARGIN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16


_gen = lambda seed: torch.Generator().manual_seed(seed)
_ratio = lambda got, ref, budget: float(((got.double().cpu() - ref.cpu()).abs() / budget.cpu()).max())


@pytest.mark.parametrize("E,k,W", ((2, 1, 64), (8, 2, 768), (16, 2, 128)))
def test_route_against_float64(E, k, W):
    ops = L.load_torch_ops()
    g = _gen(E)
    x, Wr = torch.randn(137, W, generator=g), torch.randn(E, W, generator=g) * (4.0 / W ** 0.5)
    if E == 8:
        Wr[5] = Wr[2]           # a tie in every row: the lower index must win wherever the pair is at the cut
    r = M.route_ref(x, Wr, k)
    tie = r["gap"] == 0
    decided = r["gap"] > 2 * r["bound"]
    assert int((~decided & ~tie).sum()) <= 137 // 100, "the seed leaves more than 1 % of the rows under the deciding gap"
    assert E != 8 or int(tie.sum()) >= 5, "the duplicated router row never sits at the cut"
    top_e, top_w = ops.mq_moe_route(x.to(DEV), Wr.to(DEV), k)
    torch.cuda.synchronize()
    ok = decided | tie
    assert torch.equal(top_e.cpu().long()[ok], r["top_e"][ok]), "a decided row (or a tie, lower index first) chose another expert"
    ratio = _ratio(top_w[ok], r["top_w"][ok], r["w_budget"][ok])
    print(f"MOE_RATIO route E={E} k={k} W={W}: weights {ratio:.3f}, ties {int(tie.sum())}, undecided {int((~ok).sum())}")
    assert ratio <= MARGIN


def _forced(sizes, k, seed):
    """top_e [rows, k] whose flat entries give expert e exactly sizes[e] entries (shuffled), rows = sum(sizes) / k"""
    flat = torch.cat([torch.full((n,), e, dtype=torch.int32) for e, n in enumerate(sizes)])
    return flat[torch.randperm(flat.numel(), generator=_gen(seed))].reshape(-1, k).contiguous()


def _mlp(h, top_e, top_w, w1, w2t, bm):
    """one guarded mq_moe_mlp call -> (Y [rows, k, W] looked up through row_slot, row_slot, slot_row, expert_off), the index invariants asserted"""
    ops = L.load_torch_ops()
    rows, k = top_e.shape
    W = h.shape[1]
    buf = torch.full((rows * k + 2, W), float("nan"), dtype=torch.float32, device=DEV)
    row_slot, slot_row, off = ops.mq_moe_mlp(h.to(DEV), top_e.to(DEV), top_w.to(DEV), w1.to(DEV), w2t.to(DEV), bm, buf[1:-1])
    torch.cuda.synchronize()
    assert bool(buf[0].isnan().all()) and bool(buf[-1].isnan().all()), "a guard row of Y was written"
    assert bool(torch.isfinite(buf[1:-1]).all()), "a slot of Y was not written"
    row_slot, slot_row, off = row_slot.cpu().long(), slot_row.cpu().long(), off.cpu().long()
    n = rows * k
    assert torch.equal(torch.sort(row_slot.flatten()).values, torch.arange(n)) and torch.equal(slot_row[row_slot.flatten()], torch.arange(n) // k)
    E = w1.shape[0]
    assert torch.equal(off, torch.cat([torch.zeros(1, dtype=torch.long), torch.bincount(top_e.flatten().long(), minlength=E).cumsum(0)]))
    by_slot = top_e.flatten().long()[row_slot.flatten().argsort()]          # the expert of every slot: expert-major ...
    assert torch.equal(by_slot, torch.repeat_interleave(torch.arange(E), off[1:] - off[:-1]))
    for e in range(E):                                                      # ... and ascending rows inside an expert
        seg = slot_row[off[e]:off[e + 1]]
        assert bool((seg[1:] >= seg[:-1]).all())
    return buf[1:-1][row_slot.to(DEV)], row_slot


@pytest.mark.parametrize("W,F", ((64, 64), (768, 192)))
@pytest.mark.parametrize("bm", (32, 128))
@pytest.mark.parametrize("k", (1, 2))
def test_grouped_mlp_under_forced_routings(bm, W, F, k):
    E = 7
    g = _gen(bm + W + k)
    w1 = (torch.randn(E, F, W, generator=g) * (0.6 / W ** 0.5)).to(BF)
    w2t = (torch.randn(E, W, F, generator=g) * (0.6 / F ** 0.5)).to(BF)
    worst = 0.0
    for name, sizes in (("edges", [0, 1, bm - 1, bm, bm + 1, 2 * bm + 3, 0]), ("one expert", [0, 0, 0, 2 * bm + 2, 0, 0, 0])):
        assert sum(sizes) % 2 == 0
        top_e = _forced(sizes, k, bm)
        rows = top_e.shape[0]
        h, top_w = torch.randn(rows, W, generator=g).to(BF), torch.rand(rows, k, generator=g) + 0.1
        ref, budget = M.moe_mlp_ref(h.float(), top_e, top_w, w1.float(), w2t.float())
        Y, _ = _mlp(h, top_e, top_w, w1, w2t, bm)
        ratio = _ratio(Y, ref, budget)
        print(f"MOE_RATIO mlp bm={bm} W={W} F={F} k={k} {name} rows={rows}: {ratio:.3f}")
        worst = max(worst, ratio)
    assert worst <= MARGIN


def test_one_wrong_expert_shows():
    W, F, E = 64, 64, 4
    g = _gen(5)
    w1 = (torch.randn(1, F, W, generator=g) * (0.6 / W ** 0.5)).to(BF).repeat(E, 1, 1)
    w1[2, :, 7] = (w1[2, :, 7].float() + 0.5).to(BF)           # experts 1 and 2 differ in one column of W1
    w2t = (torch.randn(1, W, F, generator=g) * (0.6 / F ** 0.5)).to(BF).repeat(E, 1, 1)
    top_e = torch.tensor([[1], [2]] * 20, dtype=torch.int32)
    h, top_w = torch.randn(40, W, generator=g), torch.ones(40, 1)
    h[:, 7] = torch.where(h[:, 7] >= 0, 2.0, -2.0)            # (a row with h[7] near 0 could not tell the two experts apart: every pre-activation moves by 1)
    h = h.to(BF)
    Y, _ = _mlp(h, top_e, top_w, w1, w2t, 32)
    ref, budget = M.moe_mlp_ref(h.float(), top_e, top_w, w1.float(), w2t.float())
    other, _ = M.moe_mlp_ref(h.float(), 3 - top_e, top_w, w1.float(), w2t.float())
    own = ((Y.double().cpu() - ref).abs() / budget).amax((1, 2))
    swapped = ((Y.double().cpu() - other).abs() / budget).amax((1, 2))
    print(f"MOE_RATIO wrong expert: own {float(own.max()):.3f} other {float(swapped.min()):.1f}")
    assert float(own.max()) <= MARGIN < float(swapped.min())


def test_a_tokens_bits_do_not_depend_on_the_batch():
    W, F, E, k = 128, 192, 4, 2
    g = _gen(9)
    w1, w2t = (torch.randn(E, F, W, generator=g) * 0.05).to(BF), (torch.randn(E, W, F, generator=g) * 0.05).to(BF)
    h, top_w = torch.randn(205, W, generator=g).to(BF), torch.rand(205, k, generator=g)
    top_e = torch.stack([torch.randperm(E, generator=g)[:k] for _ in range(205)]).to(torch.int32)
    alone, _ = _mlp(h[:5], top_e[:5], top_w[:5], w1, w2t, 0)
    for bm in (0, 32, 128):         # 0: the host's choice (the tall tile at 205 rows, the short one at 5)
        full, _ = _mlp(h, top_e, top_w, w1, w2t, bm)
        assert torch.equal(full[:5].view(torch.int32), alone.view(torch.int32)), f"bm={bm}"


@pytest.mark.parametrize("W", (64, 768))
def test_combine_ln_against_float64(W):
    from tests.rowops_ref import reference_ln
    lib = L.load()
    rows, k, eps = 37, 2, 1e-5
    g = _gen(W)
    x, Y, bias = torch.randn(rows, W, generator=g), torch.randn(rows * k, W, generator=g), torch.randn(W, generator=g)
    gam, bet = 1 + 0.1 * torch.randn(W, generator=g), 0.1 * torch.randn(W, generator=g)
    row_slot = torch.randperm(rows * k, generator=g).to(torch.int32).reshape(rows, k)
    row_slot[0] = torch.tensor([10, 11])            # a row whose two slots are neighbours of one expert's segment
    summed = ((x + Y[row_slot[:, 0].long()]) + Y[row_slot[:, 1].long()]) + bias          # the kernel's fp32 order
    ref, budget = reference_ln(summed, gam, bet, eps)
    dx, dh = x.to(DEV), torch.empty(rows, W, dtype=BF, device=DEV)
    d = [t.to(DEV) for t in (Y, row_slot, bias, gam, bet)]
    L.check(lib.mq_moe_combine_ln(dx.data_ptr(), d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr(), dh.data_ptr(), rows, W,
                                  k, eps, torch.cuda.current_stream().cuda_stream), "mq_moe_combine_ln")
    torch.cuda.synchronize()
    ratio = _ratio(dx, ref, budget)
    print(f"MOE_RATIO combine_ln W={W}: {ratio:.3f}")
    assert ratio <= MARGIN
    assert torch.equal(dh, dx.to(BF))

"""The whole passes of the three packed-token text towers through the C ABI — mq_<family>_workspace_bytes and mq_encode_<family> for modernbert
(csrc/modernbert.hip), qwen (csrc/qwen.hip) and gemma (csrc/gemma.hip) — with every row of the token stream held to the float64 reference of
tests/packed_text_ref.py.  What is under test is the host orchestration of those three files: which buffer each step reads and writes, the epilogue
flags, the inv_freq and half_window of each layer kind, the in-place final norm, Gemma's add_norm chain with its `last` switch, ModernBERT's layer 0
on the embedding's h, and the Plan workspace arithmetic.  The kernels have their own files.

cfg and weights come from ModernBertTower / QwenTower / GemmaTower on the seeded tiny checkpoints of packed_text_ref.cases(); the calls are made here,
as _PackedTextTower.encode_ids makes them, on a workspace of exactly mq_<family>_workspace_bytes.

Seeing the stream.  All three plans take the fp32 stream as the first slice of the workspace (off_x is the first ws.take: offset 0, rows * W floats), so
it is read from there after the call.  Every call checks that assumption before any parity is measured: mq_pool on that slice (mean / cls), or
mq_last_rows + mq_rmsnorm by row index + mq_l2_normalize (Qwen, last-token pooling: the slice then holds the stream in FRONT of the final norm), must
reproduce d_out bit for bit.  A failure there says that the workspace layout has changed, not that a tower is wrong.

Every case (a checkpoint x a batch: lengths 1, 17, 70, 129, or three lengths on the attention kernels' query-slice edges), every pooling, L2 on and off:
  - the worst row of  max(|got - exact|_2 / |model - exact|_2, |got - exact|_inf / |model - exact|_inf)  <= MARGIN (tests/test_patch_attn_gpu.py) for the
    stream after all blocks AND after the first block alone (cfg.layers = 1; Gemma: `last` in block 0), and for the pooled rows; no row is skipped;
    printed as PACKED_RATIO family=... case=... layers=... ratio=... (row, col, l2, linf);
  - the workspace is exactly as long as the library asks, with a 4 KiB sentinel region behind it, d_out lies between guard rows: both come back untouched;
  - the same call twice — the workspace filled with 0xA5, then with 0x3C — gives the same bits in the stream and in d_out: a slice read before it is
    written shows here;
  - the same call with a workspace one byte short is refused with MQ_ERR_WORKSPACE, d_out and the workspace keep their fill — for every case, batch,
    pooling, L2 setting and both block counts, so on either side of the plan's max(qkv width, 2 F);
  - Qwen: the pooled last rows of a batch of prefixes (1, 16, 17, 64, 65, 128, 129 tokens) of one sequence are the reference's rows len - 1 of that
    sequence — causality gives this without any knowledge of the workspace.

Measured on an MI355X (worst PACKED_RATIO per family over its cases: all blocks / first block alone / pooled; bar 4.0):
  modernbert 2.22 / 1.64 / 1.68      qwen 1.79 / 1.68 / 1.25      gemma 1.87 / 1.75 / 1.28
  Qwen's causal prefixes 1.02 / 1.24 / 1.29 (TINY3 / TINY2 / TINY64); the 129-token sequence alone 0.97 / 0.95 / 1.42.
No kernel needed a rounding the model lacks: packed_text_ref.model is the one written down from the three files' stores, the margin is the project's.

Found by this file: nothing.  What a defect of the orchestration would measure is in tests/test_packed_text_ref_host.py (PACKED_MUTANT: ratios of
73 .. 2275 against this bar of 4.0; every norm's eps times ten is the one defect listed there that this bar cannot see).
"""
import ctypes as C

import pytest
import torch

from marqo_amd import _lib as L
from tests import attention_ref as A
from tests import packed_text_ref as P
from tests.test_patch_attn_gpu import MARGIN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD_ROWS = 8
SENTINEL = 0xA5
MQ_ERR_WORKSPACE = -3
_POOL = dict(mean=L.MQ_POOL_MEAN, cls=L.MQ_POOL_CLS, last=L.MQ_POOL_LAST)

CASES = P.cases()
_PAIRS = [(c, b) for c in CASES for b in c.batches()]
_towers = {}


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _tower(case):
    """the engine's tower of the case: its cfg and weights are what the calls below hand to the library"""
    if case.id not in _towers:
        from marqo_amd.engine.gemma import GemmaTower
        from marqo_amd.engine.modernbert import ModernBertTower
        from marqo_amd.engine.qwen import QwenTower
        b = P.build(case)
        cls = dict(modernbert=ModernBertTower, qwen=QwenTower, gemma=GemmaTower)[case.family]
        _towers[case.id] = cls(b["arch"], b["sd"], DEV, pooling=P.POOLS[case.family][0])
    return _towers[case.id]


class _Call:
    """one mq_encode_<family> call on a fresh guarded d_out and a workspace of exactly the length the library asks for"""

    def __init__(self, case, lens, ids):
        self.case, self.lens, self.tower = case, list(lens), _tower(case)
        self.lib = L.load()
        self.ws_bytes = getattr(self.lib, f"mq_{case.family}_workspace_bytes")
        self.encode = getattr(self.lib, f"mq_encode_{case.family}")
        self.W = self.tower.arch.width
        self.rows, self.nseq = sum(lens), len(lens)
        self.d_ids = ids.to(torch.int32).to(DEV).contiguous()
        self.cu_h = A.cu_seqlens(lens)
        self.d_cu = self.cu_h.to(DEV)

    def run(self, layers, pool, normalize, ws_fill=SENTINEL, short=0):
        """-> (rc, stream slice [rows, W] fp32 (a copy), d_out [nseq, W] (a copy), the live workspace)"""
        cfg, W = type(self.tower.cfg).from_buffer_copy(self.tower.cfg), self.W      # (a copy: the cached tower keeps its own layers and pooling)
        cfg.layers, cfg.pool = layers, _POOL[pool]
        need = self.ws_bytes(C.byref(cfg), self.rows, self.nseq)
        assert need >= self.rows * W * 4
        ws = torch.full((need + 4096,), ws_fill, dtype=torch.uint8, device=DEV)
        rb = W * 4
        buf = torch.full(((self.nseq + 2 * GUARD_ROWS) * rb,), SENTINEL, dtype=torch.uint8, device=DEV)
        out = buf[GUARD_ROWS * rb:(GUARD_ROWS + self.nseq) * rb].view(torch.float32).view(self.nseq, W)
        assert ws.data_ptr() % 256 == 0 and out.data_ptr() % 16 == 0
        torch.cuda.synchronize()
        rc = self.encode(C.byref(cfg), C.byref(self.tower.w), self.d_ids.data_ptr(), self.d_cu.data_ptr(), self.cu_h.data_ptr(), self.nseq, out.data_ptr(),
                         normalize, ws.data_ptr(), need - short, _stream())
        torch.cuda.synchronize()
        g = GUARD_ROWS * rb
        assert bool((buf[:g] == SENTINEL).all()) and bool((buf[g + self.nseq * rb:] == SENTINEL).all()), "a guard row of d_out was written"
        assert bool((ws[need:] == ws_fill).all()), f"the workspace was written past mq_{self.case.family}_workspace_bytes"
        if short:
            assert bool((buf == SENTINEL).all()) and bool((ws == ws_fill).all()), "a refused call wrote to d_out or to the workspace"
            return rc, None, None, ws
        self.x_live = ws[:self.rows * rb].view(torch.float32).view(self.rows, W)
        return rc, self.x_live.clone(), out.clone(), ws

    def check_layout(self, pool, normalize, out):
        """the stream is the workspace's first slice: pooling it here must give d_out bit for bit"""
        lib, W, t = self.lib, self.W, self.tower
        again = torch.empty(self.nseq, W, dtype=torch.float32, device=DEV)
        if pool == "last":
            idx = torch.empty(self.nseq, dtype=torch.int32, device=DEV)
            L.check(lib.mq_last_rows(self.d_cu.data_ptr(), idx.data_ptr(), self.nseq, _stream()), "mq_last_rows")
            L.check(lib.mq_rmsnorm(self.x_live.data_ptr(), idx.data_ptr(), t.w.final_norm_g, None, again.data_ptr(), self.nseq, W, t.cfg.rms_eps, _stream()), "mq_rmsnorm")
            if normalize:
                L.check(lib.mq_l2_normalize(again.data_ptr(), again.data_ptr(), self.nseq, W, _stream()), "mq_l2_normalize")
        else:
            L.check(lib.mq_pool(self.x_live.data_ptr(), self.d_cu.data_ptr(), self.nseq, again.data_ptr(), W, _POOL[pool], normalize, _stream()), "mq_pool")
        torch.cuda.synchronize()
        if not torch.equal(again.view(torch.int32), out.view(torch.int32)):
            pytest.fail(f"the workspace layout of mq_encode_{self.case.family} has changed: pooling the first rows * W floats of the workspace does not reproduce "
                        f"d_out (pool={pool}, normalize={normalize}) — this test reads the stream from there; no parity was measured")


def _line(case, bname, layers, view, r):
    print(f"PACKED_RATIO family={case.family} case={case.id} batch={bname} layers={layers} view={view} ratio={r['ratio']:.3f} "
          f"(row {r['row']} col {r['col']}: l2 {r['l2']:.3f} linf {r['linf']:.3f})")
    return r["ratio"]


@pytest.mark.parametrize("case,batch", _PAIRS, ids=[f"{c.id}-{b[0]}" for c, b in _PAIRS])
def test_packed_tower_against_float64(case, batch):
    bname, lens = batch
    b = P.build(case)
    arch = b["arch"]
    ids = torch.cat(P.seqs_of(case, lens))
    call = _Call(case, lens, ids)
    worst = {}
    for layers in (arch.layers, 1):
        ex = P.exact(case.family, arch, b["tensors"], ids.to(DEV), lens, layers)
        mo = P.model(case.family, arch, b["tensors"], ids.to(DEV), lens, layers)
        for pool in P.POOLS[case.family]:
            for normalize in (0, 1):
                rc, x, out, _ = call.run(layers, pool, normalize)
                L.check(rc, f"mq_encode_{case.family}")
                call.check_layout(pool, normalize, out)
                rc2, x2, out2, _ = call.run(layers, pool, normalize, ws_fill=0x3C)
                L.check(rc2, f"mq_encode_{case.family}")
                assert torch.equal(x.view(torch.int32), x2.view(torch.int32)) and torch.equal(out.view(torch.int32), out2.view(torch.int32)), \
                    "the same call twice (the workspace filled with 0xA5, then 0x3C): other bits"
                assert bool(torch.isfinite(x).all()) and bool(torch.isfinite(out).all())
                rc3, _, _, _ = call.run(layers, pool, normalize, short=1)      # (run() asserts that d_out and the workspace keep their fill)
                assert rc3 == MQ_ERR_WORKSPACE, f"a workspace one byte short: rc {rc3}, not MQ_ERR_WORKSPACE"
                view = "pre_norm" if pool == "last" else "final"
                rs = _line(case, bname, layers, f"stream/{view}/{pool}/l2={normalize}", P.row_ratio(x, P.views(ex, pool), P.views(mo, pool)))
                rp = _line(case, bname, layers, f"pooled/{pool}/l2={normalize}", P.row_ratio(out, ex.pooled[(pool, normalize)], mo.pooled[(pool, normalize)]))
                key = "all" if layers == arch.layers else "first"
                worst[key] = max(worst.get(key, 0.0), rs)
                worst["pooled"] = max(worst.get("pooled", 0.0), rp)
    print(f"PACKED_WORST family={case.family} case={case.id} batch={bname}: all blocks {worst['all']:.3f} first block {worst['first']:.3f} pooled {worst['pooled']:.3f}")
    assert max(worst.values()) <= MARGIN, worst


@pytest.mark.parametrize("case", [c for c in CASES if c.family == "qwen"], ids=lambda c: c.id)
def test_qwen_causal_prefixes(case):
    """row len - 1 of a causal tower depends on the first len tokens only: the last-token rows of a batch of prefixes are rows of ONE long sequence"""
    b = P.build(case)
    arch = b["arch"]
    long = P.seqs_of(case, [129], seed=11)[0]
    cuts = [1, 16, 17, 64, 65, 128, 129]
    ex = P.exact("qwen", arch, b["tensors"], long.to(DEV), [129])
    mo = P.model("qwen", arch, b["tensors"], long.to(DEV), [129])
    at = torch.tensor(cuts, device=DEV) - 1
    rc, _, one, _ = _Call(case, [129], long).run(arch.layers, "last", 0)
    L.check(rc, "mq_encode_qwen")
    r1 = P.row_ratio(one, ex.final[128:129], mo.final[128:129])
    rc, _, out, _ = _Call(case, cuts, torch.cat([long[:n] for n in cuts])).run(arch.layers, "last", 0)
    L.check(rc, "mq_encode_qwen")
    r = P.row_ratio(out, ex.final[at], mo.final[at])
    print(f"PACKED_RATIO family=qwen case={case.id} batch=prefixes layers={arch.layers} view=pooled/last/l2=0 ratio={r['ratio']:.3f} "
          f"(prefix {cuts[r['row']]} col {r['col']}: l2 {r['l2']:.3f} linf {r['linf']:.3f}); the 129-token sequence alone {r1['ratio']:.3f}")
    assert max(r["ratio"], r1["ratio"]) <= MARGIN

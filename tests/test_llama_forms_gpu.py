"""The whole pass of the Mistral / Llama tower through the C ABI — mq_llama_workspace_bytes and mq_encode_llama (csrc/llama.hip) — with every row of the
token stream held to the float64 reference of tests/llama_ref.py (stream_exact / stream_model: the qwen form of tests/packed_text_ref.py with the
window), as tests/test_packed_text_forms_gpu.py holds the three sibling towers, with its call scaffold and its bar.  What is under test is the host
orchestration: which buffer each step reads and writes, the epilogue flags, the `windowed` switch, the wide row kernels in their places, the in-place
final norm, the last-row gather, and the Plan workspace arithmetic.

Seeing the stream.  mq_encode_llama's plan takes the fp32 stream as the first slice of the workspace (off_x is the first ws.take), so it is read from
there after the call, and every call checks that before any parity is measured: mq_pool_wide on that slice (mean), or mq_last_rows + mq_rmsnorm_wide by
row index + mq_l2_normalize (last: the slice then holds the stream in FRONT of the final norm) must reproduce d_out bit for bit.

The four tinies of tests/llama_ref.py (M128: window 48; M2560: window 200 through the wide row kernels; M4096: no window; L128: a Llama), one packed call
of lengths 1, 17, 70, 129, 300, both poolings, L2 on and off:
  - the worst row of  max(|got - exact|_2 / |model - exact|_2, |got - exact|_inf / |model - exact|_inf)  <= MARGIN = 4.0 for the stream after all
    blocks AND after the first block alone (cfg.layers = 1), and for the pooled rows; printed as LLAMA_STREAM lines;
  - the workspace is exactly as long as the library asks, with a sentinel region behind it, d_out lies between guard rows: both come back untouched;
  - the same call twice — the workspace filled with 0xA5, then with 0x3C — gives the same bits in the stream and in d_out;
  - the same call with a workspace one byte short is refused with MQ_ERR_WORKSPACE, d_out and the workspace keep their fill;
  - a batch of lengths 17 and 40 on M128 (no sequence reaches the window of 48: the causal kernel) is held to the same bar."""
import pytest
import torch

from marqo_amd import _lib as L
from tests import llama_ref as LR
from tests import packed_text_ref as P
from tests import qwen_ref as Q
from tests import test_packed_text_forms_gpu as F
from tests.test_patch_attn_gpu import MARGIN

pytestmark = pytest.mark.gpu
DEV = F.DEV
POOLS = ("last", "mean")


class _Case:
    family = "llama"

    def __init__(self, name):
        self.id = "llama-" + name


def _call(name, lens, ids):
    """test_packed_text_forms_gpu's call scaffold on the LlamaTower of the tiny; the layout check runs the wide entry points"""
    from marqo_amd.engine.llama import LlamaTower
    case = _Case(name)
    if case.id not in F._towers:
        b = LR.stream_build(name)
        F._towers[case.id] = LlamaTower(b["arch"], b["sd"], DEV, pooling="last")
    return _Call(case, lens, ids)


class _Call(F._Call):
    def check_layout(self, pool, normalize, out):
        lib, W, t = self.lib, self.W, self.tower
        again = torch.empty(self.nseq, W, dtype=torch.float32, device=DEV)
        if pool == "last":
            idx = torch.empty(self.nseq, dtype=torch.int32, device=DEV)
            L.check(lib.mq_last_rows(self.d_cu.data_ptr(), idx.data_ptr(), self.nseq, F._stream()), "mq_last_rows")
            L.check(lib.mq_rmsnorm_wide(self.x_live.data_ptr(), idx.data_ptr(), t.w.final_norm_g, None, again.data_ptr(), self.nseq, W, t.cfg.rms_eps, F._stream()),
                    "mq_rmsnorm_wide")
            if normalize:
                L.check(lib.mq_l2_normalize(again.data_ptr(), again.data_ptr(), self.nseq, W, F._stream()), "mq_l2_normalize")
        else:
            L.check(lib.mq_pool_wide(self.x_live.data_ptr(), self.d_cu.data_ptr(), self.nseq, again.data_ptr(), W, normalize, F._stream()), "mq_pool_wide")
        torch.cuda.synchronize()
        if not torch.equal(again.view(torch.int32), out.view(torch.int32)):
            pytest.fail(f"the workspace layout of mq_encode_llama has changed: pooling the first rows * W floats of the workspace does not reproduce d_out "
                        f"(pool={pool}, normalize={normalize}) — this test reads the stream from there; no parity was measured")


def _line(name, lens, layers, view, r):
    print(f"LLAMA_STREAM tiny={name} lens={list(lens)} layers={layers} view={view} ratio={r['ratio']:.3f} (row {r['row']} col {r['col']}: l2 {r['l2']:.3f} "
          f"linf {r['linf']:.3f})")
    return r["ratio"]


def _held(name, lens, seed):
    b = LR.stream_build(name)
    arch = b["arch"]
    ids = torch.cat(Q.random_seqs(list(lens), arch.vocab, seed=seed))
    call = _call(name, lens, ids)
    worst = {}
    for layers in (arch.layers, 1):
        ex = LR.stream_exact(arch, b["tensors"], ids.to(DEV), lens, layers)
        mo = LR.stream_model(arch, b["tensors"], ids.to(DEV), lens, layers)
        for pool in POOLS:
            for normalize in (0, 1):
                rc, x, out, _ = call.run(layers, pool, normalize)
                L.check(rc, "mq_encode_llama")
                call.check_layout(pool, normalize, out)
                rc2, x2, out2, _ = call.run(layers, pool, normalize, ws_fill=0x3C)
                L.check(rc2, "mq_encode_llama")
                assert torch.equal(x.view(torch.int32), x2.view(torch.int32)) and torch.equal(out.view(torch.int32), out2.view(torch.int32)), \
                    "the same call twice (the workspace filled with 0xA5, then 0x3C): other bits"
                assert bool(torch.isfinite(x).all()) and bool(torch.isfinite(out).all())
                rc3, _, _, _ = call.run(layers, pool, normalize, short=1)      # (run() asserts that d_out and the workspace keep their fill)
                assert rc3 == F.MQ_ERR_WORKSPACE, f"a workspace one byte short: rc {rc3}, not MQ_ERR_WORKSPACE"
                view = "pre_norm" if pool == "last" else "final"
                rs = _line(name, lens, layers, f"stream/{view}/{pool}/l2={normalize}", P.row_ratio(x, P.views(ex, pool), P.views(mo, pool)))
                rp = _line(name, lens, layers, f"pooled/{pool}/l2={normalize}", P.row_ratio(out, ex.pooled[(pool, normalize)], mo.pooled[(pool, normalize)]))
                key = "all" if layers == arch.layers else "first"
                worst[key] = max(worst.get(key, 0.0), rs)
                worst["pooled"] = max(worst.get("pooled", 0.0), rp)
    print(f"LLAMA_STREAM_WORST tiny={name} lens={list(lens)}: all blocks {worst['all']:.3f} first block {worst['first']:.3f} pooled {worst['pooled']:.3f} (bar {MARGIN})")
    assert max(worst.values()) <= MARGIN, worst


@pytest.mark.parametrize("name", tuple(LR.TINIES))
def test_llama_tower_stream_against_float64(name):
    _held(name, LR.LENGTHS, seed=5)


def test_a_call_no_sequence_of_which_reaches_the_window():
    _held("M128", (17, 40), seed=6)

"""The host scaffold of the packed-token text towers (no GPU): the argument checks that run in front of the first launch of mq_encode_modernbert /
mq_encode_qwen / mq_encode_gemma (and the sequence-length checks of mq_encode_bert / mq_encode_clip_text), their workspace sizes against the layouts the
units' comments state, and the Python-side validation of (ids, attention_mask).

Every call here that carries a fake device pointer is refused before any launch; the only calls that return MQ_OK have nseq = 0.  A sufficient workspace is
never passed together with fake pointers."""
import ctypes as C

import numpy as np
import pytest
import torch

from marqo_amd import _lib as L

FAKE = 4096
MQ_ERR_INVALID, MQ_ERR_WORKSPACE = -1, -3
MAX_POS = 64


def _all_set(struct, **over):
    """a ctypes struct with every pointer field at a fake non-null address"""
    s = struct()
    for name, tp in struct._fields_:
        if tp is C.c_void_p:
            setattr(s, name, FAKE)
    for k, v in over.items():
        setattr(s, k, v)
    return s


class _Family:
    def __init__(self, name, cfg_t, layer_t, weights_t, cfgs):
        self.name, self.cfg_t, self.layer_t, self.weights_t, self.cfgs = name, cfg_t, layer_t, weights_t, cfgs
        self.encode_name = f"mq_encode_{name}"

    def cfg(self, i=0, **over):
        return self.cfg_t(**dict(self.cfgs[i], **over))

    def weights(self, layer_over=None, **over):
        layers = (self.layer_t * 1)(_all_set(self.layer_t, **(layer_over or {})))
        w = _all_set(self.weights_t, **over)
        w.layers = layers
        w._keep = layers
        return w

    def encode(self, lib, cfg, w, d_ids, cu, nseq, ws=FAKE, ws_bytes=0):
        h_cu = None if cu is None else np.asarray(cu, dtype=np.int32)
        rc = getattr(lib, self.encode_name)(None if cfg is None else C.byref(cfg), C.byref(w), d_ids, FAKE, None if h_cu is None else h_cu.ctypes.data,
                                            nseq, FAKE, 1, ws, ws_bytes, None)
        return rc, lib.mq_last_error()

    def workspace_bytes(self, lib, cfg, rows, nseq):
        return getattr(lib, f"mq_{self.name}_workspace_bytes")(None if cfg is None else C.byref(cfg), rows, nseq)


# two cfgs per family: [0] the QKV width is the widest row of the shared buffer, [1] 2 * mlp_dim is
FAMILIES = {
    "modernbert": _Family("modernbert", L.ModernBertCfg, L.ModernBertLayer, L.ModernBertWeights, (
        dict(width=128, layers=1, heads=2, mlp_dim=64, vocab=10, max_pos=MAX_POS, half_window=4, pool=L.MQ_POOL_MEAN, ln_eps=1e-5),
        dict(width=64, layers=1, heads=1, mlp_dim=256, vocab=10, max_pos=MAX_POS, half_window=4, pool=L.MQ_POOL_CLS, ln_eps=1e-5))),
    "qwen": _Family("qwen", L.QwenCfg, L.QwenLayer, L.QwenWeights, (
        dict(width=128, layers=1, q_heads=4, kv_heads=2, head_dim=128, mlp_dim=64, vocab=10, max_pos=MAX_POS, pool=L.MQ_POOL_LAST, rms_eps=1e-6),
        dict(width=192, layers=1, q_heads=2, kv_heads=1, head_dim=64, mlp_dim=384, vocab=10, max_pos=MAX_POS, pool=L.MQ_POOL_MEAN, rms_eps=1e-6))),
    "gemma": _Family("gemma", L.GemmaCfg, L.GemmaLayer, L.GemmaWeights, (
        dict(width=128, layers=1, q_heads=2, kv_heads=1, head_dim=256, mlp_dim=64, vocab=10, max_pos=MAX_POS, half_window=4, pool=L.MQ_POOL_MEAN,
             rms_eps=1e-6, attn_scale=0.0625),
        dict(width=192, layers=1, q_heads=1, kv_heads=1, head_dim=256, mlp_dim=512, vocab=10, max_pos=MAX_POS, half_window=4, pool=L.MQ_POOL_CLS,
             rms_eps=1e-6, attn_scale=0.0625))),
}


# ---- the three towers: refusals in front of the first launch ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tuple(FAMILIES))
def test_entry_point_refusals(name):
    lib, f = L.load(), FAMILIES[name]
    cfg, w = f.cfg(), f.weights()
    me = f.encode_name.encode()

    def refused(got, what):
        rc, msg = got
        assert rc == MQ_ERR_INVALID and msg.startswith(me + b": ") and what in msg, (rc, msg)

    refused(f.encode(lib, None, w, FAKE, [0, 3], 1), b"null cfg")
    refused(f.encode(lib, cfg, f.weights(tok_emb=None), FAKE, [0, 3], 1), b"null weight pointer")
    refused(f.encode(lib, cfg, f.weights(layer_over=dict(qkv_w=None)), FAKE, [0, 3], 1), b"layer 0 has null weights")
    refused(f.encode(lib, cfg, w, None, [0, 3], 1), b"null input / workspace")
    refused(f.encode(lib, cfg, w, FAKE, [0, 3], 1, ws=None), b"null input / workspace")
    refused(f.encode(lib, cfg, w, FAKE, None, 1), b"null input / workspace")
    refused(f.encode(lib, cfg, w, FAKE, [1, 3], 1), b"cu_seqlens[0] must be 0")
    lengths = b"sequence lengths must be in [1, max_pos=%d]" % MAX_POS
    refused(f.encode(lib, cfg, w, FAKE, [0, 3, 3, 5], 3), lengths)             # a zero-length sequence in the middle
    refused(f.encode(lib, cfg, w, FAKE, [0, 5, 3], 2), lengths)                # a negative one
    refused(f.encode(lib, cfg, w, FAKE, [0, MAX_POS + 1], 1), lengths)
    refused(f.encode(lib, cfg, w, FAKE, [0, 2, 2 + MAX_POS + 1, 70], 3), lengths)
    # the weight checks come first, also for an empty batch; with sound weights an empty batch is nothing to do
    refused(f.encode(lib, cfg, f.weights(tok_emb=None), None, None, 0, ws=None), b"null weight pointer")
    assert f.encode(lib, cfg, w, None, None, 0, ws=None)[0] == L.MQ_OK


@pytest.mark.parametrize("name", tuple(FAMILIES))
def test_a_length_of_max_pos_passes_and_meets_the_workspace_check(name):
    lib, f = L.load(), FAMILIES[name]
    cfg, w = f.cfg(), f.weights()
    for cu in ([0, MAX_POS], [0, 1, 1 + MAX_POS, 3 + MAX_POS]):
        nseq = len(cu) - 1
        need = f.workspace_bytes(lib, cfg, cu[-1], nseq)
        assert need > 0
        rc, msg = f.encode(lib, cfg, w, FAKE, cu, nseq, ws_bytes=need - 1)
        assert rc == MQ_ERR_WORKSPACE and msg == b"%s: workspace %d < required %d" % (f.encode_name.encode(), need - 1, need), (rc, msg)


# ---- workspace sizes: the 256-aligned slices each unit's comment lists -----------------------------------------------------------------------------------
def _total(slices):
    off = 0
    for nbytes in slices:
        off = -(-off // 256) * 256 + nbytes      # align, then take
    return -(-off // 256) * 256


def _slices(name, c, rows, nseq):
    W, F = c["width"], c["mlp_dim"]
    if name == "modernbert":
        big = max(3 * W, 2 * F)
        return [rows * W * 4, rows * W * 2, rows * W * 2, rows * big * 2]
    aw, qkvw = c["q_heads"] * c["head_dim"], (c["q_heads"] + 2 * c["kv_heads"]) * c["head_dim"]
    big = max(qkvw, 2 * F)
    if name == "qwen":
        return [rows * W * 4, rows * W * 2, rows * aw * 2, rows * big * 2, nseq * 4]
    return [rows * W * 4, rows * W * 2, rows * aw * 2, rows * W * 2, rows * big * 2]


@pytest.mark.parametrize("name", tuple(FAMILIES))
def test_workspace_bytes_restated(name):
    lib, f = L.load(), FAMILIES[name]
    wins = []
    for i, c in enumerate(f.cfgs):
        qkvw = 3 * c["width"] if name == "modernbert" else (c["q_heads"] + 2 * c["kv_heads"]) * c["head_dim"]
        wins.append(qkvw > 2 * c["mlp_dim"])
        cfg = f.cfg(i)
        for rows in (1, 67, 4097):
            for nseq in (1, 3):
                assert f.workspace_bytes(lib, cfg, rows, nseq) == _total(_slices(name, c, rows, nseq)), (i, rows, nseq)
        assert f.workspace_bytes(lib, cfg, 0, 1) == 0 and f.workspace_bytes(lib, cfg, 5, 0) == 0 and f.workspace_bytes(lib, cfg, -1, -1) == 0
    assert wins == [True, False]
    assert f.workspace_bytes(lib, None, 5, 1) == 0


# ---- BERT and CLIP text: the same length walk ----------------------------------------------------------------------------------------------------------------
def test_bert_length_refusals():
    lib = L.load()
    cfg = L.BertCfg(enc=L.EncoderCfg(width=128, layers=2, heads=2, mlp_dim=256, act=1, post_ln=1, mask=0, ln_eps=1e-5), vocab=100, max_pos=MAX_POS, pool=1)
    w = L.BertWeights(word_emb=FAKE, pos_emb=FAKE, type_emb=FAKE, emb_ln_g=FAKE, emb_ln_b=FAKE)

    def call(cu, ws_bytes=0):
        h_cu = np.asarray(cu, dtype=np.int32)
        rc = lib.mq_encode_bert(C.byref(cfg), C.byref(w), FAKE, FAKE, h_cu.ctypes.data, len(cu) - 1, FAKE, 1, FAKE, ws_bytes, None)
        return rc, lib.mq_last_error()

    lengths = b"mq_encode_bert: sequence lengths must be in [1, max_pos=%d]" % MAX_POS
    assert call([1, 3]) == (MQ_ERR_INVALID, b"mq_encode_bert: cu_seqlens[0] must be 0")
    for cu in ([0, 3, 3, 5], [0, MAX_POS + 1], [0, 2, 2 + MAX_POS + 1]):
        assert call(cu) == (MQ_ERR_INVALID, lengths), cu
    need = lib.mq_bert_workspace_bytes(C.byref(cfg), MAX_POS + 2, 2)
    assert need > 0
    assert call([0, 2, 2 + MAX_POS], need - 1) == (MQ_ERR_WORKSPACE, b"mq_encode_bert: workspace %d < required %d" % (need - 1, need))


@pytest.mark.parametrize("cls_pos", (0, 3))
def test_clip_text_length_refusals(cls_pos):
    """a tower that adds its own [CLS] row (cls_pos > 0) takes ctx + 1 rows per sequence; the message names ctx either way"""
    lib = L.load()
    ctx = 16
    cfg = L.ClipTextCfg(enc=L.EncoderCfg(width=128, layers=2, heads=2, mlp_dim=256, act=2, post_ln=0, mask=1, ln_eps=1e-5), vocab=100, ctx=ctx, out_dim=64,
                        cls_pos=cls_pos)
    w = L.ClipTextWeights(tok_emb=FAKE, pos=FAKE, ln_final_g=FAKE, ln_final_b=FAKE, proj_w=FAKE)

    def call(cu, ws_bytes=0):
        h_cu = np.asarray(cu, dtype=np.int32)
        rc = lib.mq_encode_clip_text(C.byref(cfg), C.byref(w), FAKE, FAKE, h_cu.ctypes.data, len(cu) - 1, None, FAKE, 1, FAKE, ws_bytes, None)
        return rc, lib.mq_last_error()

    bound = ctx + (1 if cls_pos else 0)
    lengths = b"mq_encode_clip_text: sequence lengths must be in [1, ctx=%d]" % ctx
    assert call([1, 3]) == (MQ_ERR_INVALID, b"mq_encode_clip_text: cu_seqlens[0] must be 0")
    for cu in ([0, 3, 3, 5], [0, bound + 1], [0, 2, 2 + bound + 1]):
        assert call(cu) == (MQ_ERR_INVALID, lengths), cu
    need = lib.mq_clip_text_workspace_bytes(C.byref(cfg), bound + 2, 2)
    assert need > 0
    assert call([0, 2, 2 + bound], need - 1) == (MQ_ERR_WORKSPACE, b"mq_encode_clip_text: workspace %d < required %d" % (need - 1, need))


# ---- the Python side: (ids, attention_mask) -> host ids and lengths ----------------------------------------------------------------------------------------
def _mask(lengths, S):
    return (np.arange(S)[None, :] < np.asarray(lengths)[:, None]).astype(np.int64)


BAD_INPUTS = (
    ("shapes", np.zeros((2, 3), np.int64), np.ones((2, 4), np.int64), r"ids and attention_mask must both be \[n, S\]"),
    ("1-D", np.zeros(3, np.int64), np.ones(3, np.int64), r"ids and attention_mask must both be \[n, S\]"),
    ("empty row", np.zeros((2, 3), np.int64), np.asarray([[1, 1, 0], [0, 0, 0]]), "every sequence needs at least one unmasked token"),
    ("hole", np.zeros((2, 3), np.int64), np.asarray([[1, 1, 0], [1, 0, 1]]), r"attention_mask must be right-padded \(a prefix of ones per row\)"),
    ("left-padded", np.zeros((2, 3), np.int64), np.asarray([[1, 1, 1], [0, 1, 1]]), r"attention_mask must be right-padded \(a prefix of ones per row\)"),
    ("too long", np.zeros((2, 9), np.int64), _mask([2, 9], 9), "sequence longer than max_position_embeddings=8"),
)


def test_ids_and_lengths():
    from marqo_amd.engine.towers import _ids_and_lengths
    for what, ids, mask, msg in BAD_INPUTS:
        with pytest.raises(ValueError, match=msg):
            _ids_and_lengths(torch.from_numpy(ids), torch.from_numpy(mask), 8)
    with pytest.raises(ValueError, match="left-padded input is not served"):
        _ids_and_lengths(np.zeros((1, 3), np.int64), np.asarray([[0, 1, 1]]), 8)
    ids = np.arange(3 * 70, dtype=np.int64).reshape(3, 70)
    ids_h, lengths = _ids_and_lengths(torch.from_numpy(ids).to(torch.int32), torch.from_numpy(_mask([1, 17, 70], 70)), 70)
    assert ids_h.dtype == np.int64 and np.array_equal(ids_h, ids) and lengths.tolist() == [1, 17, 70]
    ids_h, lengths = _ids_and_lengths(np.zeros((0, 4), np.int64), np.zeros((0, 4), np.int64), 8)       # an empty batch is no error
    assert ids_h.shape == (0, 4) and lengths.size == 0


def _towers():
    from marqo_amd.engine.gemma import GemmaTower
    from marqo_amd.engine.modernbert import ModernBertTower
    from marqo_amd.engine.qwen import QwenTower
    from marqo_amd.engine.towers import BertTower
    return BertTower, ModernBertTower, QwenTower, GemmaTower


@pytest.mark.parametrize("i", range(4))
def test_every_tower_refuses_bad_input_before_it_touches_the_device(i):
    """encode_ids of an instance that has no device, no library and no weights: the refusal is raised in front of all of them"""
    cls = _towers()[i]
    tower = object.__new__(cls)
    tower.arch = type("Arch", (), {"max_pos": 8})()
    for what, ids, mask, msg in BAD_INPUTS:
        with pytest.raises(ValueError, match=msg):
            tower.encode_ids(torch.from_numpy(ids), torch.from_numpy(mask))

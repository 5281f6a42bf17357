"""The C-ABI shared library loads WITHOUT a GPU and exports every entry point include/marqo_hip.h declares; the ctypes
binding covers the same set; POD struct layouts match the header (no compute is launched here)."""
import ctypes as C
import os
import re

from marqo_amd import _lib as L

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "marqo_hip.h")


def _declared():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(mq_[a-z0-9_]+)\s*\(", src)))


def test_header_symbols_are_exported_and_bound():
    names = _declared()
    assert len(names) >= 25
    lib = L.load()
    raw = C.CDLL(str(L.LIB_PATH))
    for n in names:
        assert hasattr(raw, n), f"libmarqo_hip.so does not export {n}"
        assert n in L.EXPORTED_SYMBOLS, f"ctypes binding is missing {n}"
    assert set(L.EXPORTED_SYMBOLS) <= set(names), set(L.EXPORTED_SYMBOLS) - set(names)
    assert lib.mq_abi_version() == L.ABI_VERSION == 15 and lib.mq_build_arch() == b"gfx950"


def test_struct_layouts_match_header():
    assert C.sizeof(L.BlockWeights) == 36 * 8           # ABI 10: + attn_ln_g / _b, mlp_ln_g / _b (the EVA02 blocks' sub-LayerNorms); ABI 12: + their folded out / fc2 tensors
    # ... + d_rel_bias, rel_span, residual_stream (ABI 5: reserved0), fp8_mlp_extra, rope_prefix (ABI 6: reserved1) + ABI 10: d_rope_table, mlp_ln_dim, reserved2
    ENC = 8 * 4 + 4 * 4 + 3 * 8 + 8 + 2 * 4 + 2 * 4 + 8 + 2 * 4
    assert C.sizeof(L.EncoderCfg) == ENC
    assert C.sizeof(L.VitCfg) == ENC + 3 * 4 + 6 * 4 + 4 * 4 + 4  # + tail padding to 8
    assert C.sizeof(L.VitWeights) == 11 * 8 and C.sizeof(L.MapHead) == 11 * 8
    assert C.sizeof(L.ClipTextCfg) == ENC + 4 * 4 and C.sizeof(L.ClipTextWeights) == 7 * 8
    assert C.sizeof(L.BertCfg) == ENC + 5 * 4 + 4 and C.sizeof(L.BertWeights) == 9 * 8   # + proj_hidden, out_dim / proj1_w, proj1_b, proj2_w
    assert C.sizeof(L.QueueCfg) == 10 * 4 and C.sizeof(L.QueueStats) == 9 * 8   # ABI 14: the native request queue


def test_argument_errors_are_reported_without_a_gpu():
    lib = L.load()
    assert lib.mq_gemm_bf16(None, 0, None, 0, None, None, None, 0, 1, 4, 64, 0, None) == -1
    assert b"null operand" in lib.mq_last_error()
    cfg = L.EncoderCfg(width=100, layers=1, heads=1, mlp_dim=64, act=1, post_ln=0, mask=0, ln_eps=1e-5)
    assert lib.mq_encoder_forward(C.byref(cfg), None, None, 0, None, 0, 0, 0, None, 0, None) == -1
    assert b"multiple of 64" in lib.mq_last_error()
    assert lib.mq_encoder_workspace_bytes(C.byref(L.EncoderCfg(width=768, layers=12, heads=12, mlp_dim=3072, act=1)), 100, 2) > 0
    assert lib.mq_chunk_grid_count(3, 3, 0) == 10 and lib.mq_chunk_grid_count(3, 3, 1) == 14 and lib.mq_chunk_grid_count(0, 3, 0) == 0
    assert lib.mq_resample_ksize(640, 224) == 13 and lib.mq_resample_ksize(80, 224) == 5
    # ABI 14, the native request queue: arguments are judged before any device is asked for
    h = C.c_void_p()
    assert lib.mq_queue_create(None, None, None, C.byref(h)) == -1 and b"null pointer" in lib.mq_last_error() and not h
    qc = L.QueueCfg(kind=L.QUEUE_BERT, device=0, max_seqs=0, max_rows=512, normalize=1, depth=2, window_us=0, graphs=0)
    bc, bw = L.BertCfg(), L.BertWeights()
    assert lib.mq_queue_create(C.byref(qc), C.cast(C.byref(bc), C.c_void_p), C.cast(C.byref(bw), C.c_void_p), C.byref(h)) == -1 and not h
    assert b"max_seqs" in lib.mq_last_error()
    assert lib.mq_queue_encode(None, None, None, 1, None) == -1 and b"null queue" in lib.mq_last_error()
    assert lib.mq_queue_get_stats(None, None) == -1 and lib.mq_queue_destroy(None) == 0
    # the tiled GEMM entry points: every shape / layout refusal returns -1 before any launch or device query and names the entry point and the
    # bad quantity (fake: a non-null operand address, never dereferenced)
    fake = 256
    gemms = {   # name -> (call(M, N, K, lda), K step, leading dimension of a bad layout)
        "mq_gemm_bf16": (lambda M, N, K, ld: lib.mq_gemm_bf16(fake, ld, fake, K, fake, None, fake, N, M, N, K, 1, None), 64, 4),
        "mq_gemm_bf16_ln": (lambda M, N, K, ld: lib.mq_gemm_bf16_ln(fake, ld, fake, K, fake, fake, fake, fake, N, M, N, K, 1, None), 64, 4),
        "mq_gemm_bf16_rs": (lambda M, N, K, ld: lib.mq_gemm_bf16_rs(fake, ld, fake, K, fake, fake, fake, N, M, N, K, 9, fake, None), 64, 4),
        "mq_gemm_bf16_lnrs": (lambda M, N, K, ld: lib.mq_gemm_bf16_lnrs(fake, ld, fake, K, fake, fake, fake, fake, fake, N, M, N, K, 9, fake, None),
                              64, 4),
        "mq_gemm_bf16_rsf": (lambda M, N, K, ld: lib.mq_gemm_bf16_rsf(fake, ld, fake, K, fake, fake, fake, N, M, N, K, 9, fake, fake, 1e-5, None,
                                                                     None, 0, None, 0, None), 64, 4),
        "mq_gemm_fp8": (lambda M, N, K, ld: lib.mq_gemm_fp8(fake, ld, fake, K, fake, 1, fake, fake, None, fake, N, None, None, M, N, K, 1, None), 128, 8),
    }
    for name, (call, bk, bad_ld) in gemms.items():
        for args, what in (((0, 64, bk, bk), b"M=0"),                       # bad shape
                           ((1, 64, bk + 32, bk + 32), b"K=%d" % (bk + 32)),  # K not a multiple of the k-step
                           ((1, 66, bk, bk), b"N=66"),                      # N not a multiple of 4
                           ((1, 64, bk, bad_ld), b"leading dims"),          # rows that are not 16-byte aligned
                           ((1 << 30, 64, bk, bk), b"shape too large")):    # beyond the kernels' 32-bit row indices
            assert call(*args) == -1, (name, args)
            err = lib.mq_last_error()
            assert err.startswith(name.encode() + b": ") and what in err, (name, args, err)


def test_product_never_imports_the_oracle():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for dp, _, files in os.walk(os.path.join(root, "marqo_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                src = open(os.path.join(dp, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M), os.path.join(dp, f)
                assert "liboracle" not in src


def test_host_gather_checked_bounds_and_copies():
    """mq_host_gather_checked: the destination's capacity is validated before any byte moves; within bounds it is mq_host_gather"""
    import ctypes as C
    import numpy as np
    from marqo_amd import _lib as L
    lib = L.load()
    srcs_np = [np.arange(n, dtype=np.uint8) for n in (1000, 0, 5_000_000, 777)]
    offs = np.asarray([0, 1024, 1024, 5_001_200], dtype=np.int64)
    nbytes = np.asarray([a.nbytes for a in srcs_np], dtype=np.int64)
    dst = np.zeros(5_002_000, dtype=np.uint8)
    srcs = (C.c_void_p * 4)(*[a.ctypes.data for a in srcs_np])
    L.check(lib.mq_host_gather_checked(srcs, nbytes.ctypes.data, offs.ctypes.data, 4, dst.ctypes.data, dst.nbytes, 4))
    for a, o in zip(srcs_np, offs):
        assert np.array_equal(dst[o:o + a.nbytes], a)
    rc = lib.mq_host_gather_checked(srcs, nbytes.ctypes.data, offs.ctypes.data, 4, dst.ctypes.data, 5_001_900, 4)   # the last item would overrun
    assert rc != 0 and b"leaves" in lib.mq_last_error()


def test_building_block_argument_errors_are_reported_without_a_gpu():
    """csrc/embed.hip's entry points judge their shapes before any launch: each refusal returns -1 and names the problem"""
    lib = L.load()
    fake = 256   # a non-null operand address: never dereferenced, the argument check fails first

    def refused(rc, msg):
        assert rc == -1
        assert msg in lib.mq_last_error(), lib.mq_last_error()

    refused(lib.mq_rope(fake, None, 1, 4, 72, 1, fake, None), b"head width 72 must be a multiple of 16")
    refused(lib.mq_rope(fake, None, 1, 4, 480, 12, fake, None), b"head width 40 must be a multiple of 16")
    refused(lib.mq_glu_ln(fake, 4, 64, 65, L.MQ_ACT_SILU, fake, fake, 1e-6, 0, None), b"Ft=65 unsupported")
    refused(lib.mq_glu_ln(fake, 4, 64, 64, L.MQ_ACT_SILU, fake, fake, 1e-6, 4, None), b"glu_ln: mode 4")
    refused(lib.mq_glu_ln(fake, 4, 4104, 4104, L.MQ_ACT_SILU, fake, fake, 1e-6, 0, None), b"F=4104")
    refused(lib.mq_glu_ln(fake, 4, 1032, 1032, L.MQ_ACT_SILU, fake, fake, 1e-6, 1, None), b"glu_ln: mode 1 / F=1032")
    refused(lib.mq_glu_ln(fake, 4, 64, 64, L.MQ_ACT_SILU, None, None, 1e-6, 0, None), b"glu_ln: F=64")   # LayerNorm modes need g and b
    refused(lib.mq_glu(fake, 4, 1032, L.MQ_ACT_SILU, 1, None), b"F=1032 must be a multiple of 8 (16 interleaved)")
    refused(lib.mq_glu(fake, 4, 4608, L.MQ_ACT_SILU, 1, None), b"F=4608 > 4096")
    refused(lib.mq_map_pool(fake, fake, fake, 1, 16, 136, 1, None), b"head dim 136 unsupported")
    refused(lib.mq_map_pool(fake, fake, fake, 1, 4097, 768, 12, None), b"4097 tokens unsupported")
    refused(lib.mq_map_pool(fake, fake, fake, 1, 16, 768, 7, None), b"map_pool: W=768 heads=7")
    refused(lib.mq_pool(fake, fake, 1, fake, 2056, L.MQ_POOL_MEAN, 1, None), b"pool: W=2056 unsupported")
    refused(lib.mq_move_rows(fake, fake, fake, 1, 24, 0, None), b"row_bytes=24 must be a multiple of 16")
    refused(lib.mq_rope_table(fake, 10, 3, 1, 768, 12, fake, None), b"rows (10) a multiple of the sequence length 3")
    refused(lib.mq_rope_table(fake, 9, 3, 1, 768, 12, None, None), b"rope_table:")   # no table
    refused(lib.mq_vit_assemble(fake, fake, fake, None, None, fake, 1, 50, 2052, 1e-6, 0, None), b"vit_assemble: W=2052 unsupported")
    refused(lib.mq_embed_tokens(fake, fake, 1, fake, None, None, None, None, fake, None, 770, 100, 1e-12, 0, None),
            b"embed_tokens: W=770 unsupported")
    refused(lib.mq_avg_tokens(fake, 0, fake, 1, 50, 50, 768, None), b"avg_tokens: bad shape W=768 T=50 first=50")

"""engine/vit_tokens.py on the GPU: the shared front end and encoder step of the token-level towers (DinoTower, OwlTower, LanguageBindVideoTower)
issue exactly the five library calls written out here — mq_patchify, mq_gemm_bf16 (fp32 out), mq_vit_assemble, mq_encoder_workspace_bytes,
mq_encoder_forward — on the tower's own weight tensors: the token streams are bit-identical.  The numerics of those calls are held against
the references by the towers' own tests; this file holds the launch sequence they rely on, in the three forms it is used in."""
import ctypes as C

import pytest
import torch

from marqo_amd import _lib as L
from marqo_amd.engine import archs, synthetic, towers
from marqo_amd.engine.vit_tokens import VitTokenTower

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
W, HEADS, MLP, LAYERS = 128, 2, 256, 3
MEAN, STD = archs.OPENAI_DATASET_MEAN, archs.OPENAI_DATASET_STD


class _Tower(VitTokenTower):
    def __init__(self, arch, sd, pre, enc_layers):
        super().__init__(DEV, arch, "bf16", enc_layers)
        self.mean, self.std = (C.c_float * 3)(*MEAN), (C.c_float * 3)(*STD)
        self._load_vit(sd, "visual.conv1.weight", sd["visual.class_embedding"], sd["visual.positional_embedding"],
                       (sd["visual.ln_pre.weight"], sd["visual.ln_pre.bias"]) if pre else None, sd, "visual.transformer.")


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def _front_end_by_hand(t, u8):
    """today's front end on the tower's weights -> the fp32 token stream [m T, W]"""
    lib, a, m, s = L.load(), t.arch, u8.shape[0], _stream()
    S, P = a.image_size, a.patch_size
    G, K = S // P, 3 * P * P
    T, Kp = G * G + 1, (K + 63) // 64 * 64
    patches = torch.empty(m * G * G, Kp, dtype=torch.bfloat16, device=DEV)
    patch_out = torch.empty(m * G * G, W, dtype=torch.float32, device=DEV)
    x = torch.empty(m * T, W, dtype=torch.float32, device=DEV)
    mean, std = (C.c_float * 3)(*MEAN), (C.c_float * 3)(*STD)
    L.check(lib.mq_patchify(u8.data_ptr(), 1, patches.data_ptr(), m, S, P, Kp, C.addressof(mean), C.addressof(std), s), "mq_patchify")
    L.check(lib.mq_gemm_bf16(patches.data_ptr(), Kp, t._patch_w, Kp, None, None, patch_out.data_ptr(), W, m * G * G, W, Kp, L.MQ_EPI_OUT_F32, s),
            "mq_gemm_bf16")
    L.check(lib.mq_vit_assemble(patch_out.data_ptr(), t._cls, t._pos, t._pre[0], t._pre[1], x.data_ptr(), m, T, W, a.ln_eps, 0, s), "mq_vit_assemble")
    return x


def _encoder_by_hand(t, x, m, layers, firsts):
    """mq_encoder_forward over `layers` blocks from each of `firsts`, one workspace for all of them; x in place"""
    lib, a, s = L.load(), t.arch, _stream()
    T = a.tokens
    enc = towers._encoder_cfg(W, layers, HEADS, MLP, False, False, L.MQ_MASK_NONE, a.ln_eps)
    enc.residual_stream = 2
    ws = torch.empty(lib.mq_encoder_workspace_bytes(C.byref(enc), m * T, m) + 256, dtype=torch.uint8, device=DEV)
    for first in firsts:
        L.check(lib.mq_encoder_forward(C.byref(enc), C.byref(t._blocks[first]), x.data_ptr(), m * T, None, m, T, T, ws.data_ptr(), ws.numel(), s),
                "mq_encoder_forward")
    return x


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == torch.float32 and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("m", [1, 3])
@pytest.mark.parametrize("pre", [True, False])
@pytest.mark.parametrize("S,P", [(32, 16), (28, 14)])       # 5 tokens each; K = 768 = Kp, K = 588 < Kp = 640
def test_base_class_issues_the_launch_sequence_written_out_here(S, P, pre, m):
    arch = archs.VitArch(S, P, W, LAYERS, HEADS, MLP, 64)
    sd = synthetic.random_open_clip_state_dict(vision=arch, seed=S + m)
    u8 = torch.randint(0, 256, (m, S, S, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(7 * S + m)).to(DEV)
    by_layers = {}
    with torch.cuda.device(DEV):
        for enc_layers, firsts in ((3, (0,)), (2, (0,)), (1, (0, 1, 2))):      # every block at once; DinoTower's form; LanguageBindVideoTower's form
            t = _Tower(arch, sd, pre, enc_layers)
            assert t.Kp == (3 * P * P + 63) // 64 * 64 and t.Kp % 64 == 0 and (t.Kp > 3 * P * P) == (P == 14)
            assert t.grid == S // P and arch.tokens == 5 and t.max_items_per_call == towers.MAX_ROWS_PER_CALL // 5
            assert t.enc.layers == enc_layers and t.enc.residual_stream == 2
            want = _front_end_by_hand(t, u8)
            patches = t._patchify(u8)
            assert patches.shape == (m * t.grid ** 2, t.Kp) and patches.dtype == torch.bfloat16
            x = t._tokens(patches, m)
            torch.cuda.synchronize(DEV)
            assert _same_bits(x, want), f"front end, {enc_layers} blocks per call"
            assert not _same_bits(x, _front_end_by_hand(_Tower(arch, sd, not pre, enc_layers), u8)), "the pre-LayerNorm changes nothing: the test cannot see it"
            want = _encoder_by_hand(t, want, m, enc_layers, firsts)
            ws = t._encoder_workspace(m)
            for first in firsts:
                t._encoder(x, m, ws, first=first)
            torch.cuda.synchronize(DEV)
            assert _same_bits(x, want), f"encoder, {enc_layers} blocks per call from {firsts}"
            assert bool(torch.isfinite(x).all())
            by_layers[enc_layers] = x
    assert not _same_bits(by_layers[2], by_layers[3]), "the third block changes nothing: the test cannot see the layer count"
    # one block per call, three calls = three blocks in one call: the blocks are the same kernels on the same rows either way
    assert _same_bits(by_layers[1], by_layers[3]), "finding: mq_encoder_forward block by block differs from one call over all blocks"

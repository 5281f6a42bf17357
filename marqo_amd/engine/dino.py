"""DINO ViT attention boxes: the model behind the 'dino-v1' / 'dino-v2' image patch methods (s2_inference/processing/image.py).

The reference runs a facebookresearch/dino ViT-S/16 and reads `get_last_selfattention` (processing/DINO_utils.py:85-123,
vision_transformer.py:221-228): every block but the last in full, then of the last block only norm1 -> qkv -> softmax(q k^T / 8), of which
the class token's row over the patch keys is kept.  Here that is

    mq_patchify -> mq_gemm_bf16 (conv as GEMM) -> mq_vit_assemble (class token + positions; the conv bias rides on the patch positions)
    -> mq_encoder_forward over the first L - 1 blocks (fp32 residual stream) -> mq_layernorm (norm1 of block L - 1) -> mq_gemm_bf16 (+ bias: qkv)
    -> mq_attention_cls_probs -> mq_attn_boxes

The last block's out-projection, MLP and V are never computed.  The residual stream stays in fp32 whatever MARQO_AMD_RESIDUAL_STREAM says: the boxes
hang on a threshold between two uint8 levels of the map, and this tower is one call per indexed image, not the throughput path.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Tuple

import torch

from marqo_amd import _lib as L
from marqo_amd.engine.archs import DINO_MEAN, DINO_STD, VitArch, dino_arch
from marqo_amd.engine.towers import _need, _TIMM_KEYS
from marqo_amd.engine.vit_tokens import VitTokenTower

Tensor = torch.Tensor
MODE_MEAN, MODE_PER_HEAD = 0, 1     # mq_attn_boxes: 'abs' (dino-v1) / 'pos' (dino-v2) of the reference's _process_attention


class DinoTower(VitTokenTower):
    """facebookresearch/dino state dict (`cls_token`, `pos_embed`, `patch_embed.proj.*`, `blocks.N.*`, `norm`) -> class-token attention maps and
    their boxes.  `DinoTower(arch, sd, device)` or `DinoTower(arch, None, device, synthetic=seed)`; bf16 operands only."""

    def __init__(self, arch: VitArch, sd: Optional[Dict[str, Tensor]], device: str, precision: str = "bf16", synthetic: Optional[int] = None):
        super().__init__(device, arch, precision, arch.layers - 1)
        if sd is None:
            if synthetic is None:
                raise ValueError("DinoTower needs a state dict or a synthetic= seed")
            from marqo_amd.engine.synthetic import random_dino_state_dict
            sd = random_dino_state_dict(arch, seed=int(synthetic))
        W = arch.width
        if self.grid > 32:
            raise ValueError(f"DinoTower: image {arch.image_size} / patch {arch.patch_size} must give a grid of at most 32 x 32 patches")
        pos = _need(sd, "pos_embed", (1, arch.tokens, W)).detach().to(torch.float32)[0].clone()
        pos[1:] += _need(sd, "patch_embed.proj.bias", (W,)).detach().to(torch.float32)
        _need(sd, "norm.weight", (W,))     # (part of the checkpoint's contract; the attention maps are read in front of it)
        self._load_vit(sd, "patch_embed.proj.weight", _need(sd, "cls_token", (1, 1, W)).reshape(W), pos, None, sd, "", _TIMM_KEYS)
        self.mean, self.std = (C.c_float * 3)(*DINO_MEAN), (C.c_float * 3)(*DINO_STD)
        self.max_boxes = ((self.grid + 1) // 2) ** 2       # isolated cells on every other row and column: no map has more components

    # ---- one call of m images: uint8 [m, S, S, 3] on the device -> fp32 [m, heads, T - 1] -------------------------------------------------------
    def _probs_call(self, u8: Tensor, out: Tensor) -> None:
        lib, a, s = self.lib, self.arch, self._stream()
        m, W, T = u8.shape[0], a.width, a.tokens
        rows, dev = m * T, self.device
        x = self._tokens(self._patchify(u8), m)
        if self.enc.layers > 0:
            self._encoder(x, m, self._encoder_workspace(m))
        # The last block's norm1 and QKV run as mq_layernorm + mq_gemm_bf16, not as the encoder's LN-folded QKV GEMM: that fold takes its row statistics
        # from the bf16 residual stream, and this tower keeps the stream in fp32 (the maps are thresholded between two uint8 levels).  The buffers
        # below are allocated per call: one call per indexed image, off the throughput path.  (_clip_blocks prepares the folded qkv / fc1 tensors for
        # every block, the last one's unused: one code path for loading blocks, at the price of ~2 MB of device memory for ViT-S.)
        last = self._blocks[a.layers - 1]
        hn = torch.empty(rows, W, dtype=torch.bfloat16, device=dev)
        qkv = torch.empty(rows, 3 * W, dtype=torch.bfloat16, device=dev)
        L.check(lib.mq_layernorm(x.data_ptr(), None, last.ln1_g, last.ln1_b, hn.data_ptr(), None, rows, W, a.ln_eps, s), "mq_layernorm")
        L.check(lib.mq_gemm_bf16(hn.data_ptr(), W, last.qkv_w, W, last.qkv_b, None, qkv.data_ptr(), 3 * W, rows, 3 * W, W, L.MQ_EPI_BIAS, s),
                "mq_gemm_bf16")
        L.check(lib.mq_attention_cls_probs(qkv.data_ptr(), out.data_ptr(), m, T, W, a.heads, s), "mq_attention_cls_probs")

    def probs(self, images_u8: Tensor) -> Tensor:
        """uint8 [n, S, S, 3] (HWC RGB) -> fp32 [n, heads, G * G] on the device: the class token's attention over the patch keys in the last block"""
        u8 = self._check_u8(images_u8)
        n, a = u8.shape[0], self.arch
        with torch.cuda.device(self.device):
            out = torch.empty(n, a.heads, a.tokens - 1, dtype=torch.float32, device=self.device)
            for i in range(0, n, self.max_items_per_call):
                self._probs_call(u8[i:i + self.max_items_per_call], out[i:i + self.max_items_per_call])
        return out

    def boxes_from_probs(self, probs: Tensor, mode: int) -> Tuple[Tensor, Tensor]:
        """fp32 [n, heads, G * G] on the device -> (int32 [n, maps, max_boxes, 4] boxes (x1, y1, x2, y2) in PIXELS of the S x S input, int32 [n, maps] counts)"""
        if mode not in (MODE_MEAN, MODE_PER_HEAD):
            raise ValueError(f"mode must be {MODE_MEAN} (mean over heads) or {MODE_PER_HEAD} (per head), got {mode!r}")
        n, a = probs.shape[0], self.arch
        maps = 1 if mode == MODE_MEAN else a.heads
        with torch.cuda.device(self.device):
            boxes = torch.zeros(n, maps, self.max_boxes, 4, dtype=torch.int32, device=self.device)
            counts = torch.zeros(n, maps, dtype=torch.int32, device=self.device)
            L.check(self.lib.mq_attn_boxes(probs.data_ptr(), n, a.heads, self.grid, mode, boxes.data_ptr(), counts.data_ptr(), self.max_boxes,
                                           self._stream()), "mq_attn_boxes")
            boxes *= a.patch_size      # nearest upsampling by the patch size: grid cells -> pixels
        return boxes, counts

    def boxes(self, images_u8: Tensor, mode: int) -> Tuple[Tensor, Tensor]:
        """uint8 [n, S, S, 3] -> (boxes, counts) as boxes_from_probs; one launch sequence for the n images"""
        return self.boxes_from_probs(self.probs(images_u8), mode)


def load_dino(path: str, device: str, name: str = "vit_small", patch_size: int = 16) -> DinoTower:
    """a facebookresearch/dino checkpoint file (dino_deitsmall16_pretrain.pth, ...) -> DinoTower"""
    from marqo_amd.engine.checkpoint import load_state_dict
    return DinoTower(dino_arch(name, patch_size), load_state_dict(path), device)

"""The ViT towers that keep every token (engine/dino.py, engine/owl.py, engine/languagebind.py): what they load and launch alike.

    im2col rows (mq_patchify, or the tower's own kernel) -> mq_gemm_bf16 (conv as GEMM) -> mq_vit_assemble (class token + positions [+ pre-LayerNorm])
    -> mq_encoder_forward over a run of blocks, on the fp32 residual stream whatever MARQO_AMD_RESIDUAL_STREAM says; bf16 operands only"""
import ctypes as C
from typing import Optional, Tuple

import torch

from marqo_amd import _lib as L
from marqo_amd.engine.hf_clip import clip_state_dict
from marqo_amd.engine.towers import MAX_ROWS_PER_CALL, _ImageTowerBase, _check_precision, _clip_blocks, _encoder_cfg, _need, _OPEN_CLIP_KEYS, patch_embed_weight

Tensor = torch.Tensor


class VitTokenTower(_ImageTowerBase):
    """`enc_layers`: the blocks one mq_encoder_forward call runs; `frames`: images per item of a call (the frames of a clip)"""

    def __init__(self, device: str, arch, precision: str, enc_layers: int, frames: int = 1):
        super().__init__(device)
        W, P, S, name = arch.width, arch.patch_size, arch.image_size, type(self).__name__
        H, Wd = getattr(arch, "image_hw", (S, S))       # (a picture that is not square: the LanguageBind audio part's mel bins x frames)
        _check_precision(precision, ("bf16",), f"{name} runs on bf16 operands only, got precision {precision!r}")
        if arch.heads * 64 != W or W > 2048 or arch.layers < 1 or H % P or Wd % P or arch.tokens > 8192:
            raise ValueError(f"{name} runs 64-wide attention heads, widths up to 2048, a whole grid of at most 8191 patches and at least one block "
                             f"(width {W} with {arch.heads} heads, image {S if H == Wd else f'{H} x {Wd}'} / patch {P}, {arch.layers} blocks)")
        self.precision, self.arch, self.grid, self.grid_hw = precision, arch, S // P, (H // P, Wd // P)
        self.enc = _encoder_cfg(W, enc_layers, arch.heads, arch.mlp_dim, arch.quick_gelu, False, L.MQ_MASK_NONE, arch.ln_eps)
        self.enc.residual_stream = 2
        self.max_items_per_call = max(1, MAX_ROWS_PER_CALL // (frames * arch.tokens))

    def _load_vit(self, sd, patch_key: str, cls: Tensor, pos: Tensor, pre: Optional[Tuple[Tensor, Tensor]], block_sd, block_prefix: str, block_keys=_OPEN_CLIP_KEYS):
        """sd[patch_key]: the conv weight; cls [W]; pos [T, W]; pre: (weight, bias) of the LayerNorm behind the positions or None; block_*: for _clip_blocks"""
        a, h = self.arch, self._h
        patch_w = patch_embed_weight(sd, patch_key, a.width, a.patch_size)
        self.Kp = patch_w.shape[1]
        self._patch_w, self._cls, self._pos = h.bf16(patch_w), h.f32(cls), h.f32(pos)
        self._pre = (h.f32(pre[0]), h.f32(pre[1])) if pre else (None, None)
        self._blocks = _clip_blocks(h, block_sd, block_prefix, a.layers, a.width, a.mlp_dim, a.heads, keys=block_keys)

    def _load_hf_vit(self, sd, v: str, pre: str) -> None:
        """transformers' CLIPVisionModel names under `v`; `pre`: the LayerNorm behind the positions as the checkpoint spells it; keeps `_post`"""
        W = self.arch.width
        ln = lambda k: (_need(sd, v + k + ".weight", (W,)), _need(sd, v + k + ".bias", (W,)))
        self._load_vit(sd, v + "embeddings.patch_embedding.weight", _need(sd, v + "embeddings.class_embedding", (W,)),
                       _need(sd, v + "embeddings.position_embedding.weight", (self.arch.tokens, W)), ln(pre), clip_state_dict(sd, v, self.arch.layers), "transformer.")
        self._post = tuple(self._h.f32(t) for t in ln("post_layernorm"))

    # ---- one call of `frames` images ------------------------------------------------------------------------------------------------------------
    def _patchify(self, u8: Tensor) -> Tensor:
        """uint8 [m, S, S, 3] on the device -> bf16 im2col rows [m G G, Kp], normalised with the tower's `mean` / `std`"""
        a, m = self.arch, u8.shape[0]
        if self.grid_hw != (self.grid, self.grid):
            raise ValueError(f"{type(self).__name__}: mq_patchify takes square uint8 images, this tower's grid is {self.grid_hw[0]} x {self.grid_hw[1]}")
        patches = torch.empty(m * self.grid ** 2, self.Kp, dtype=torch.bfloat16, device=self.device)
        L.check(self.lib.mq_patchify(u8.data_ptr(), 1, patches.data_ptr(), m, a.image_size, a.patch_size, self.Kp, C.addressof(self.mean), C.addressof(self.std),
                                     self._stream()), "mq_patchify")
        return patches

    def _patchify_f32(self, px: Tensor) -> Tensor:
        """preprocessed fp32 [m, 3, H, Wd] on the device (contiguous; H x Wd the tower's picture, square or not) -> bf16 im2col rows [m Gh Gw, Kp]"""
        a, m, (gh, gw) = self.arch, px.shape[0], self.grid_hw
        patches = torch.empty(m * gh * gw, self.Kp, dtype=torch.bfloat16, device=self.device)
        L.check(self.lib.mq_patchify_rect(px.data_ptr(), patches.data_ptr(), m, gh * a.patch_size, gw * a.patch_size, a.patch_size, self.Kp, self._stream()),
                "mq_patchify_rect")
        return patches

    def _tokens(self, patches: Tensor, frames: int) -> Tensor:
        """bf16 im2col rows [frames G G, Kp] -> the fp32 token stream [frames T, W].  The GEMM's output is scratch of this method: once the
        caller has dropped `patches` too, both are back in the allocator before the encoder's workspace is asked for"""
        lib, s, W, T, n = self.lib, self._stream(), self.arch.width, self.arch.tokens, patches.shape[0]
        patch_out, x = (torch.empty(r, W, dtype=torch.float32, device=self.device) for r in (n, frames * T))
        L.check(lib.mq_gemm_bf16(patches.data_ptr(), self.Kp, self._patch_w, self.Kp, None, None, patch_out.data_ptr(), W, n, W, self.Kp, L.MQ_EPI_OUT_F32, s),
                "mq_gemm_bf16")
        L.check(lib.mq_vit_assemble(patch_out.data_ptr(), self._cls, self._pos, *self._pre, x.data_ptr(), frames, T, W, self.arch.ln_eps, 0, s), "mq_vit_assemble")
        return x

    def _encoder_workspace(self, frames: int) -> Tensor:
        return self._workspace(self.lib.mq_encoder_workspace_bytes(C.byref(self.enc), frames * self.arch.tokens, frames))

    def _encoder(self, x: Tensor, frames: int, ws: Tensor, first: int = 0) -> None:
        """blocks first .. first + enc_layers - 1 on the stream x, in place"""
        T = self.arch.tokens
        L.check(self.lib.mq_encoder_forward(C.byref(self.enc), C.byref(self._blocks[first]), x.data_ptr(), frames * T, None, frames, T, T,
                                            ws.data_ptr(), ws.numel(), self._stream()), "mq_encoder_forward")

"""OWL-ViT open-vocabulary detection: the model behind the image reranker (s2_inference/reranking/cross_encoders.py ReRankerOwl).

The reference runs transformers' `OwlViTForObjectDetection` one image at a time (model_utils.py:305-366): the processor squashes the 240 x 240
working image to S x S (Pillow bicubic), the CLIP ViT with `pre_layernorm` keeps every token, the class token is merged into the patch tokens,
a class head scores every patch against the query's text embedding and a box head predicts one box per patch.  Here every image of a search goes
through as few launch sequences as the row cap allows:

    mq_resize_u8 (Pillow-identical bicubic) -> mq_patchify -> mq_gemm_bf16 (conv as GEMM) -> mq_vit_assemble (class token + positions + pre_layernorm)
    -> mq_encoder_forward on ALL rows (fp32 residual stream) -> mq_owl_merge_ln (post_layernorm, x class token, layer_norm: one pass)
    -> class head: mq_gemm_bf16 (dense0 + bias, fp32 out) -> mq_owl_class_head (normalised dot with the query, learned shift, ELU scale, max, sigmoid)
    -> box head:   mq_gemm_bf16 (dense0 + bias + GELU) -> mq_gemm_bf16 (dense1 + bias + GELU) -> mq_owl_box_head (dense2, grid bias, sigmoid,
                   corner format, target size)
    -> mq_owl_topk (one workgroup per image): only k rows per image go back to the host.

The query runs through the CLIP text machinery with 16 positions, packed up to its EOT (under the causal mask nothing behind the EOT reaches the
pooled row).  The residual stream of the image encoder stays in fp32 whatever MARQO_AMD_RESIDUAL_STREAM says: every patch row is an output here,
not one pooled row, and this is one call per search, not the throughput path.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from marqo_amd import _lib as L
from marqo_amd.engine import archs, checkpoint
from marqo_amd.engine.archs import OPENAI_DATASET_MEAN, OPENAI_DATASET_STD, OwlArch
from marqo_amd.engine.hf_clip import clip_text_state_dict, load_tokenizer
from marqo_amd.engine.tokenizers import ClipBpeTokenizer
from marqo_amd.engine.towers import ClipTextTower, _need, request_stream
from marqo_amd.engine.vit_tokens import VitTokenTower

Tensor = torch.Tensor
MAX_QUERIES = 8        # mq_owl_class_head


def box_bias(grid: int) -> Tensor:
    """OwlViTForObjectDetection.compute_box_bias for a grid x grid map, the torch ops in their order -> fp32 [grid * grid, 4]"""
    c = torch.arange(1, grid + 1, dtype=torch.float32)
    xx, yy = torch.meshgrid(c, c, indexing="xy")
    xy = torch.stack((xx, yy), dim=-1)
    xy[..., 0] /= grid
    xy[..., 1] /= grid
    xy = torch.clip(xy.view(-1, 2), 0.0, 1.0)
    coord = torch.log(xy + 1e-4) - torch.log1p(-xy + 1e-4)
    size = torch.full_like(coord, 1.0)
    size[..., 0] /= grid
    size[..., 1] /= grid
    return torch.cat([coord, torch.log(size + 1e-4) - torch.log1p(-size + 1e-4)], dim=-1).contiguous()


class OwlTower(VitTokenTower):
    """`OwlViTForObjectDetection` state dict (`owlvit.vision_model.*`, `owlvit.text_model.*`, `owlvit.text_projection`, `class_head.*`,
    `box_head.*`, `layer_norm.*`) -> per-patch scores and boxes, and the k best per image.  bf16 operands only."""

    def __init__(self, arch: OwlArch, sd: Dict[str, Tensor], device: str, tokenizer: ClipBpeTokenizer, precision: str = "bf16"):
        super().__init__(device, arch, precision, arch.layers)
        self.tokenizer = tokenizer
        W, Dq = arch.width, arch.query_dim
        if arch.text_heads * 64 != arch.text_width or Dq > 2048 or Dq % 4 or Dq != arch.text_width:
            raise ValueError(f"OwlTower runs 64-wide attention heads and a query dimension up to 2048 that is a multiple of 4 and equals the text "
                             f"width (text width {arch.text_width} with {arch.text_heads} heads, query {Dq})")
        if tokenizer.eot_id >= arch.vocab:
            raise ValueError(f"the tokenizer's EOT id {tokenizer.eot_id} is outside the model's vocabulary of {arch.vocab}")
        self.patches = self.grid ** 2
        h = self._h
        f32 = lambda k, shape=None: _need(sd, k, shape).detach().to(torch.float32)
        self._load_hf_vit(sd, "owlvit.vision_model.", "pre_layernorm")
        self._merge = (h.f32(f32("layer_norm.weight", (W,))), h.f32(f32("layer_norm.bias", (W,))))
        # heads
        self._cls0 = (h.bf16(f32("class_head.dense0.weight", (Dq, W))), h.f32(f32("class_head.dense0.bias", (Dq,))))
        self._shift_w, self._shift_b = h.f32(f32("class_head.logit_shift.weight", (1, W)).reshape(W)), float(f32("class_head.logit_shift.bias", (1,))[0])
        self._scale_w, self._scale_b = h.f32(f32("class_head.logit_scale.weight", (1, W)).reshape(W)), float(f32("class_head.logit_scale.bias", (1,))[0])
        self._box0 = (h.bf16(f32("box_head.dense0.weight", (W, W))), h.f32(f32("box_head.dense0.bias", (W,))))
        self._box1 = (h.bf16(f32("box_head.dense1.weight", (W, W))), h.f32(f32("box_head.dense1.bias", (W,))))
        self._box2 = (h.f32(f32("box_head.dense2.weight", (4, W))), h.f32(f32("box_head.dense2.bias", (4,))))
        self._box_bias = h.f32(box_bias(self.grid))
        self.mean, self.std = (C.c_float * 3)(*OPENAI_DATASET_MEAN), (C.c_float * 3)(*OPENAI_DATASET_STD)
        # the query side: the CLIP text tower on 16 positions
        self.text = ClipTextTower(arch.text(), clip_text_state_dict(sd, "owlvit.text_model.", "owlvit.text_projection.weight", arch.text()), str(self.device))
        self.text.release_unused_folded()

    @classmethod
    def from_dir(cls, directory: str, device: str, name: Optional[str] = None) -> "OwlTower":
        """a local Hugging Face OWL-ViT directory: config.json (model_type owlvit), model.safetensors | pytorch_model.bin, vocab.json, merges.txt.
        `name`: the checkpoint's published name, whose table entry fills what config.json leaves out"""
        cfg, sd = checkpoint.load_hf_dir(directory)
        try:
            arch = archs.owl_arch_from_hf_config(cfg, archs.OWL_ARCHS.get(name) if name else None)
        except KeyError as e:
            raise ValueError(f"{directory}: {e.args[0] if e.args else e}") from e
        return cls(arch, sd, device, load_tokenizer(directory, arch.ctx))

    # ---- the query --------------------------------------------------------------------------------------------------------------------------
    def query_ids(self, queries: Sequence[str]) -> np.ndarray:
        """-> int64 [Q, ctx]: SOT ids EOT, zero-padded.  The reference's processor pads to the model's 16 positions and does NOT truncate, so a
        longer query fails there in the position embedding; here it is refused by name."""
        a, tok = self.arch, self.tokenizer
        out = np.zeros((len(queries), a.ctx), dtype=np.int64)
        for i, q in enumerate(queries):
            if not isinstance(q, str):
                raise TypeError(f"an OWL-ViT query is a string, found {type(q).__name__}")
            ids = [tok.sot_id] + tok.encode(q) + [tok.eot_id]
            if len(ids) > a.ctx:
                raise ValueError(f"the query has {len(ids)} tokens with its start and end tokens; OWL-ViT takes at most {a.ctx} and the reference's "
                                 f"processor does not truncate: {q[:80]!r}")
            out[i, :len(ids)] = ids
        return out

    def embed_queries(self, queries: Sequence[str]) -> Tensor:
        """-> fp32 [Q, Dq] on the device: text_projection(pooled EOT row) / its norm = the `query_embeds` the class head receives"""
        ids = self.query_ids(queries)
        return self.text.encode_ids(torch.from_numpy(ids), normalize=True).to(self.device, non_blocking=True).contiguous()

    # ---- the images ----------------------------------------------------------------------------------------------------------------------------
    def resize(self, u8: Tensor) -> Tensor:
        """uint8 [m, h, w, 3] on the device -> uint8 [m, S, S, 3]: PIL.Image.resize((S, S), BICUBIC) of every image"""
        m, hh, ww = u8.shape[0], u8.shape[1], u8.shape[2]
        S = self.arch.image_size
        if (hh, ww) == (S, S):
            return u8
        off = (np.arange(m, dtype=np.int64) * (hh * ww * 3))
        hs, ws_ = np.full(m, hh, dtype=np.int32), np.full(m, ww, dtype=np.int32)
        out = torch.empty(m, S, S, 3, dtype=torch.uint8, device=self.device)
        need = self.lib.mq_resize_workspace_bytes(hs.ctypes.data, ws_.ctypes.data, m, S, S)
        scratch = torch.empty(int(need) + 256, dtype=torch.uint8, device=self.device)
        L.check(self.lib.mq_resize_u8(u8.data_ptr(), off.ctypes.data, hs.ctypes.data, ws_.ctypes.data, m, S, S, out.data_ptr(), scratch.data_ptr(),
                                      scratch.numel(), self._stream()), "mq_resize_u8")
        return out

    def features(self, u8: Tensor) -> Tuple[Tensor, Tensor]:
        """uint8 [m, S, S, 3] on the device -> feats (bf16, fp32) [m P, W]: encoder, post_layernorm, class-token merge, layer_norm"""
        lib, a, s, dev = self.lib, self.arch, self._stream(), self.device
        m, W, T, P = u8.shape[0], a.width, a.tokens, self.patches
        x = self._tokens(self._patchify(u8), m)
        self._encoder(x, m, self._encoder_workspace(m))
        fb = torch.empty(m * P, W, dtype=torch.bfloat16, device=dev)
        ff = torch.empty(m * P, W, dtype=torch.float32, device=dev)
        L.check(lib.mq_owl_merge_ln(x.data_ptr(), self._post[0], self._post[1], self._merge[0], self._merge[1], fb.data_ptr(), ff.data_ptr(), m, T, W,
                                    a.ln_eps, s), "mq_owl_merge_ln")
        return fb, ff

    def heads(self, fb: Tensor, ff: Tensor, queries: Tensor, query_mask: Optional[Tensor], m: int, target_size: Tuple[float, float], score: Tensor,
              logit: Tensor, label: Tensor, boxes: Tensor) -> None:
        """feats of m images -> score / logit fp32 [m, P], label int32 [m, P], boxes fp32 [m, P, 4] (x0, y0, x1, y1) in target_size = (w, h)"""
        lib, a, s, dev = self.lib, self.arch, self._stream(), self.device
        W, Dq, P = a.width, a.query_dim, self.patches
        rows = m * P
        e = torch.empty(rows, Dq, dtype=torch.float32, device=dev)
        L.check(lib.mq_gemm_bf16(fb.data_ptr(), W, self._cls0[0], W, self._cls0[1], None, e.data_ptr(), Dq, rows, Dq, W,
                                 L.MQ_EPI_BIAS | L.MQ_EPI_OUT_F32, s), "mq_gemm_bf16")
        L.check(lib.mq_owl_class_head(e.data_ptr(), ff.data_ptr(), queries.data_ptr(), L.ptr(query_mask), 0, self._shift_w, self._shift_b,
                                      self._scale_w, self._scale_b, score.data_ptr(), logit.data_ptr(), label.data_ptr(), m, P, W, Dq,
                                      queries.shape[0], s), "mq_owl_class_head")
        h0 = torch.empty(rows, W, dtype=torch.bfloat16, device=dev)
        h1 = torch.empty(rows, W, dtype=torch.bfloat16, device=dev)
        L.check(lib.mq_gemm_bf16(fb.data_ptr(), W, self._box0[0], W, self._box0[1], None, h0.data_ptr(), W, rows, W, W,
                                 L.MQ_EPI_BIAS | L.MQ_EPI_GELU, s), "mq_gemm_bf16")
        L.check(lib.mq_gemm_bf16(h0.data_ptr(), W, self._box1[0], W, self._box1[1], None, h1.data_ptr(), W, rows, W, W,
                                 L.MQ_EPI_BIAS | L.MQ_EPI_GELU, s), "mq_gemm_bf16")
        L.check(lib.mq_owl_box_head(h1.data_ptr(), self._box2[0], self._box2[1], self._box_bias, boxes.data_ptr(), m, P, W, float(target_size[0]),
                                    float(target_size[1]), s), "mq_owl_box_head")

    def _check_images(self, images_u8) -> Tensor:
        if not isinstance(images_u8, torch.Tensor):
            images_u8 = torch.from_numpy(np.ascontiguousarray(images_u8))
        if images_u8.dtype != torch.uint8 or images_u8.ndim != 4 or images_u8.shape[3] != 3 or min(images_u8.shape[1:3]) < 1:
            raise ValueError(f"expected uint8 [n, h, w, 3], got {images_u8.dtype} {tuple(images_u8.shape)}")
        if images_u8.device.type == "cpu":
            images_u8 = images_u8.pin_memory()
        return images_u8.to(self.device, non_blocking=True).contiguous()

    def detect_all(self, queries, images_u8, target_size: Tuple[float, float]) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
        """queries: one string or up to 8 (an empty string is a padded query: masked out, as the reference masks all-zero id rows);
        images_u8: uint8 [n, h, w, 3] (HWC RGB, host or device) at the reranker's working size; target_size = (w, h) the boxes are scaled to
        -> on the device: score fp32 [n, P] = sigmoid(max over the queries of the logits), logit fp32 [n, P], label int32 [n, P], boxes fp32 [n, P, 4]"""
        queries = [queries] if isinstance(queries, str) else list(queries)
        if not 1 <= len(queries) <= MAX_QUERIES:
            raise ValueError(f"between 1 and {MAX_QUERIES} queries per call, got {len(queries)}")
        dev, P = self.device, self.patches
        with request_stream(dev, device_output=True), torch.cuda.device(dev):
            u8 = self._check_images(images_u8)
            n = u8.shape[0]
            live = [q != "" for q in queries]
            emb = torch.zeros(len(queries), self.arch.query_dim, dtype=torch.float32, device=dev)
            if any(live):
                got = self.embed_queries([q for q, ok in zip(queries, live) if ok])
                emb[torch.as_tensor([i for i, ok in enumerate(live) if ok], dtype=torch.int64).to(dev)] = got      # (row scatter: memory movement)
            mask = None if all(live) else torch.tensor([int(ok) for ok in live], dtype=torch.int32).to(dev)
            score = torch.empty(n, P, dtype=torch.float32, device=dev)
            logit = torch.empty(n, P, dtype=torch.float32, device=dev)
            label = torch.empty(n, P, dtype=torch.int32, device=dev)
            boxes = torch.empty(n, P, 4, dtype=torch.float32, device=dev)
            for i in range(0, n, self.max_items_per_call):
                j = min(n, i + self.max_items_per_call)
                fb, ff = self.features(self.resize(u8[i:j]))
                self.heads(fb, ff, emb, mask, j - i, target_size, score[i:j], logit[i:j], label[i:j], boxes[i:j])
        return score, logit, label, boxes

    def topk(self, score: Tensor, boxes: Tensor, k: int) -> Tuple[Tensor, Tensor, Tensor]:
        """score fp32 [n, P], boxes fp32 [n, P, 4] on the device -> the min(k, P) best per image, descending, ties to the lower patch:
        (scores [n, k], boxes [n, k, 4], patch int32 [n, k]) on the device"""
        if k < 1:
            raise ValueError(f"k={k} must be at least 1")
        n, P = score.shape
        k = min(int(k), P)
        with torch.cuda.device(self.device):
            ts = torch.empty(n, k, dtype=torch.float32, device=self.device)
            tb = torch.empty(n, k, 4, dtype=torch.float32, device=self.device)
            tp = torch.empty(n, k, dtype=torch.int32, device=self.device)
            L.check(self.lib.mq_owl_topk(score.data_ptr(), boxes.data_ptr(), n, P, k, ts.data_ptr(), tb.data_ptr(), tp.data_ptr(), self._stream()),
                    "mq_owl_topk")
        return ts, tb, tp

    def detect(self, query, images_u8, k: int = 1, target_size: Tuple[float, float] = (240, 240)) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """the k best boxes of every image for `query` -> host arrays scores fp32 [n, k], boxes fp32 [n, k, 4], patch int32 [n, k]
        (k = min(k, patches per image))"""
        if k < 1:
            raise ValueError(f"k={k} must be at least 1")
        score, _, _, boxes = self.detect_all(query, images_u8, target_size)
        if score.shape[0] == 0:
            k = min(int(k), self.patches)
            return np.zeros((0, k), np.float32), np.zeros((0, k, 4), np.float32), np.zeros((0, k), np.int32)
        ts, tb, tp = self.topk(score, boxes, k)
        return ts.cpu().numpy(), tb.cpu().numpy(), tp.cpu().numpy()

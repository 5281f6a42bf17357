/*
 * marqo_hip.h — C ABI of libmarqo_hip.so, the MI355X (gfx950) engine underneath
 * Marqo's s2_inference.vectorise() hot path.
 *
 * The reference (marqo-ai/marqo @ v2.13.0) has NO FFI for this path: its "plugin"
 * interface is Python duck-typing through the loader map
 * (src/marqo/s2_inference/model_registry.py:2133-2145) and the arithmetic lives in
 * un-vendored wheels (open_clip_torch 2.24.0 / transformers 4.41.2).  This header is
 * therefore the boundary the reference WOULD bind (via ctypes) to
 * replace, one for one:
 *
 *   mq_encode_image_*   <- OPEN_CLIP.encode_image -> open_clip model.encode_image
 *                          src/marqo/core/inference/embedding_models/open_clip_model.py:249-266
 *                          (+ the preprocess transform src/marqo/s2_inference/clip_utils.py:48-67
 *                             when raw uint8 pixels are handed over)
 *   mq_encode_clip_text <- OPEN_CLIP.encode_text -> open_clip model.encode_text
 *                          .../open_clip_model.py:268-286
 *   mq_encode_bert      <- HuggingFaceModel.encode -> AutoModel forward + pooling + F.normalize
 *                          .../hugging_face_model.py:172-214
 *   mq_chunk_grid_u8    <- PatchifySimple / chunk_image  src/marqo/s2_inference/processing/image.py:46-151
 *
 * Conventions
 *   - every pointer named d_* is a DEVICE pointer (HBM) owned by the caller (the Python
 *     host allocates through PyTorch-ROCm; the library never allocates device memory —
 *     the one exception is mq_queue_create, ABI 14, which sizes its own staging once);
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); every entry
 *     point only ENQUEUES work on it and returns; results are valid after the caller
 *     synchronises that stream;
 *   - no torch types, no C++ types: plain pointers, ints and POD structs;
 *   - return value: 0 = MQ_OK, negative = error; mq_last_error() gives the text
 *     (thread-local).
 *   - bf16 = the 16 high bits of an IEEE fp32 (round-to-nearest-even when produced here).
 */
#ifndef MARQO_HIP_H
#define MARQO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MQ_OK 0
#define MQ_ERR_INVALID (-1)   /* bad argument / unsupported shape */
#define MQ_ERR_HIP (-2)       /* a HIP runtime call or launch failed */
#define MQ_ERR_WORKSPACE (-3) /* caller's workspace too small */
#define MQ_ERR_UNSUPPORTED (-4) /* ABI 11: the device is not the one this library is built for (mq_check_device) */

#define MQ_ABI_VERSION 15

/* ---- activation / mask / pooling selectors ---------------------------------------- */
#define MQ_ACT_NONE 0
#define MQ_ACT_GELU 1      /* erf GELU (open_clip nn.GELU, HF "gelu") */
#define MQ_ACT_QUICKGELU 2 /* x * sigmoid(1.702 x) (OpenAI / *-quickgelu weights) */
#define MQ_ACT_SILU 3      /* x * sigmoid(x): the gate of the SwiGLU MLP (EVA02 towers; gated MLPs only) */
#define MQ_ACT_RELU 4      /* max(0, x) (the M2M100 / NLLB encoder behind the NLLB-CLIP text towers): plain pre-LN bf16 encoders only — no fp8, no gated MLP */

#define MQ_MASK_NONE 0   /* ViT: full attention inside a sequence */
#define MQ_MASK_CAUSAL 1 /* CLIP text tower */
#define MQ_MASK_CAUSAL_CLS 2 /* ABI 11 — CoCa text tower (open_clip TextTransformer embed_cls): causal, and the LAST row of a sequence — the appended class
                              * token — does not attend its own key.  open_clip 2.24.0 build_cls_mask pads the key axis of the class row's mask on the LEFT
                              * (F.pad(cls_mask, (1, 0, S, 0), value=True)): the class row sees key 0 and key j + 1 wherever text[j] != pad — i.e. the text, the
                              * FIRST pad position, and itself only when the text fills all S positions.  The caller packs [text, one pad row, class row]
                              * (text shorter than S) or [text, class row, class row] (full text: the twin stands for "itself"). */
/* key-padding masks (BERT) are expressed by packing: only real tokens are rows. */

#define MQ_PREC_BF16 0
#define MQ_PREC_FP8 1

#define MQ_POOL_MEAN 0 /* hugging_face_model.py:205-209 */
#define MQ_POOL_CLS 1  /* hugging_face_model.py:211-214 */

#define MQ_VIT_POOL_CLS 0 /* open_clip VisionTransformer: class token */
#define MQ_VIT_POOL_MAP 1 /* timm SigLIP ViT: attention-pool ('map') head */
#define MQ_VIT_POOL_AVG 2 /* open_clip VisionTransformer pool_type 'avg' with final_ln_after_pool (CLIPA): mean of the patch tokens -> ln_post -> proj;
                           * ln_pre_g / ln_pre_b may be NULL (no_ln_pre) */
#define MQ_VIT_POOL_QUERY 3 /* open_clip VisionTransformer with an AttentionalPooler behind it (CoCa, model_registry.py:344-370): class token and ln_pre as
                             * in CLIP; every token runs every block; k | v = ln_k(x) @ kv_w^T + kv_b of width pool_dim, ONE query row (query 0 of the
                             * learned queries, projected at load) -> out-projection -> ln_post -> proj.  mq_map_head carries the pooler (fc1 / fc2 NULL) */

/* GEMM epilogue flags for mq_gemm_bf16 */
#define MQ_EPI_BIAS 1      /* + bias[n] (fp32) */
#define MQ_EPI_GELU 2      /* erf GELU after bias */
#define MQ_EPI_QUICKGELU 4 /* quick GELU after bias */
#define MQ_EPI_RESIDUAL 8  /* + residual[m,n] (fp32, leading dim ldc) */
#define MQ_EPI_OUT_F32 16  /* write fp32 instead of bf16 */
#define MQ_EPI_OUT_FP8 32  /* (mq_gemm_fp8 only) write e4m3 codes = value / out_scale, saturating at +-448 */

/* ---- transformer encoder description ---------------------------------------------- */

/* One residual block.  Linear weights are bf16, row-major [out_features, in_features]
 * (PyTorch nn.Linear layout); biases and LayerNorm parameters are fp32. */
typedef struct mq_block_weights {
    const float* ln1_g; const float* ln1_b;   /* [W]  pre-LN: before attention; post-LN: after attention */
    const void*  qkv_w; const float* qkv_b;   /* [3W, W], [3W]  rows: q | k | v */
    const void*  out_w; const float* out_b;   /* [W, W], [W] */
    const float* ln2_g; const float* ln2_b;   /* [W] */
    const void*  fc1_w; const float* fc1_b;   /* [F, W], [F] */
    const void*  fc2_w; const float* fc2_b;   /* [W, F], [W] */
    /* fp8 path (precision == MQ_PREC_FP8, else ignored / NULL): e4m3 codes in the same [out, in] layout and the
     * per-output-channel fp32 scales written by mq_quantize_weights_fp8 */
    const void*  qkv_w8; const float* qkv_ws; /* [3W, W], [3W] */
    const void*  out_w8; const float* out_ws; /* [W, W],  [W]  */
    const void*  fc1_w8; const float* fc1_ws; /* [F, W],  [F]  */
    const void*  fc2_w8; const float* fc2_ws; /* [W, F],  [W]  */
    /* LayerNorm folding (pre-LN bf16 encoders; all six NULL = off): the LayerNorm in front of the QKV / fc1 GEMM folded into
     * that GEMM, LN(x) @ W^T = rstd * (x @ (g*W)^T - mean * colsum(g*W)) + (b + W @ beta):
     * *_wf = bf16(g[k] * W[n,k]) [out, in], *_sf = fp32 sum_k of those bf16 values [out], *_bf = fp32 b + W @ beta [out]. */
    const void*  qkv_wf; const float* qkv_sf; const float* qkv_bf;
    const void*  fc1_wf; const float* fc1_sf; const float* fc1_bf;
    /* sub-LayerNorms of the EVA02 blocks (timm eva.py; ABI 10; NULL = none): attn_ln over the attention output [attn_width], in front of the
     * out-projection (`scale_attn_inner`); mlp_ln over the gated hidden row up * silu(gate) [F] in front of fc2 (`scale_mlp`; mean and variance
     * over the first mq_encoder_cfg.mlp_ln_dim columns — the checkpoint's hidden width — when F is that width zero-padded to a multiple of 64). */
    const float* attn_ln_g; const float* attn_ln_b;
    const float* mlp_ln_g;  const float* mlp_ln_b;
    /* ABI 12 — the sub-LayerNorms folded into the GEMMs behind them (bf16 stream, tiled GEMM family; all six NULL = the LayerNorm kernels run):
     * out_wf = bf16(attn_ln_g[k] * out_w[n,k]) [W, attn_width], out_sf its row sums, out_bf = out_b + out_w @ attn_ln_b;
     * fc2_wf = bf16(mlp_ln_g[k] * fc2_w[n,k]) [W, F], fc2_sf, fc2_bf likewise.  The rows' (mean, rstd) come from the launch that wrote them: the
     * attention kernel's per-head sums (mq_attention_stats), the gated epilogue's per-slot sums (mq_gemm_bf16_lnrs with MQ_EPI_GLU). */
    const void*  out_wf; const float* out_sf; const float* out_bf;
    const void*  fc2_wf; const float* fc2_sf; const float* fc2_bf;
} mq_block_weights;

typedef struct mq_encoder_cfg {
    int32_t width;      /* W, multiple of 64 */
    int32_t layers;
    int32_t heads;      /* attention runs 64-, 96-, 112- or 128-wide heads: heads * that == attn_width (or width) */
    int32_t mlp_dim;    /* F, multiple of 64 */
    int32_t act;        /* MQ_ACT_* */
    int32_t post_ln;    /* 0: pre-LN (CLIP); 1: post-LN (BERT) */
    int32_t mask;       /* MQ_MASK_* */
    float   ln_eps;
    int32_t precision;  /* MQ_PREC_BF16 (0) or MQ_PREC_FP8 (width and mlp_dim multiples of 128) */
    int32_t attn_width; /* 0 = width.  heads * {64, 96, 112, 128} when the checkpoint's heads are narrower and were zero-padded at load
                         * (QKV weights [3*attn_width, W], out-projection [W, attn_width]) */
    int32_t fp8_first_layer; /* MQ_PREC_FP8: blocks [0, fp8_first_layer) run their GEMMs on bf16 operands, blocks from here on on e4m3.
                              * Quantisation noise injected in EARLY blocks is amplified by every later one (measured: the first 12 of
                              * ViT-L/14's 24 blocks cost 2-7x the cosine error of the last 12), so the loaders pick the smallest value
                              * that keeps the calibrated error inside the budget (engine/towers.py::tune_fp8); 0 = every block fp8 */
    int32_t mlp_glu;         /* 1: gated MLP: fc1_w is [2F, W] = (up | gate) rows, hidden = up * act(gate), fc2 takes the F-wide product.  2 (ABI 11, pre-LN
                              * blocks with MQ_ACT_SILU): the same with fc1_w / fc1_b (and the folded copies) interleaved 16 rows at a time as MQ_EPI_GLU
                              * takes them — the product is formed in the GEMM's epilogue.  bf16 path only:
                              * post-LN = the "NewModel" encoders (stella_en_400M_v5, gte-*-en-v1.5); pre-LN = the EVA02 vision blocks (SwiGLU:
                              * act = MQ_ACT_SILU, up = fc1_x, gate = fc1_g, optional mlp_ln). */
    /* fp8 path: static per-tensor activation scales, device fp32 [layers][2] = (attention output, MLP hidden), and the
     * calibration accumulator of the same shape (NULL = frozen scales; non-NULL = fold max|value| of this pass into it) */
    const float* d_fp8_act_scale;
    float*       d_fp8_act_amax;
    /* rotary position embedding (NULL: none — learned absolute positions are added by the embedding kernel instead): device fp32
     * [head_dim / 2] inverse frequencies (theta scaling, NTK factor etc. are folded in by the loader).  Applied to the Q and K columns
     * of the QKV buffer in place, HF "rotate_half" convention: (x1, x2) = (x[d], x[d + hd/2]) -> (x1 cos - x2 sin, x2 cos + x1 sin),
     * angle = position_in_sequence * inv_freq[d].  bf16 path only. */
    const float* d_rope_inv_freq;
    /* relative-position attention bias (NULL: none).  MPNet (sentence-transformers all-mpnet-base-*, transformers MPNetModel: one T5-style
     * bucketed bias table shared by every layer, added to the attention scores before the softmax): device fp32
     * [heads][2 * rel_span - 1], entry (h, d + rel_span - 1) = bias(h, key - query == d) * sqrt(head_dim) (i.e. divided by the softmax
     * scale, which the kernel applies to the sum), rel_span >= the longest sequence run.  bf16 path, 64-wide heads, unmasked attention. */
    const float* d_rel_bias;
    int32_t      rel_span;
    int32_t      residual_stream; /* 0 = the process default (mq_tune("residual_bf16") / MQ_RESIDUAL_BF16 for pre-LN bf16 encoders, fp32 unless set),
                                   * 1 = bf16 residual stream, 2 = fp32.  Pre-LN encoders (bf16, and e4m3 towers whose policy asks for it): x is
                                   * kept in bf16 between blocks (half the bytes of every residual epilogue and LayerNorm).  Post-LN bf16 encoders
                                   * (BERT family): the normalised bf16 rows are the residual, updated in place; the last LayerNorm writes the fp32
                                   * rows that are pooled.  The loaders decide 1 / 2 per MODEL at load on a fixed seeded batch
                                   * (engine/towers.py::tune_residual_stream / tune_fp8: bf16 only where it stays within a 1 - cos budget of the
                                   * fp32 stream).  (Took the slot of the former reserved0.) */
    int32_t      fp8_mlp_extra;   /* MQ_PREC_FP8, pre-LN encoders: the `fp8_mlp_extra` blocks in FRONT of fp8_first_layer run only their MLP half on e4m3
                                   * (LayerNorm 2 -> e4m3 rows, fc1 + activation -> e4m3, fc2 + residual) and keep LayerNorm 1 / QKV / attention /
                                   * out-projection on bf16 operands: two thirds of a block's GEMM FLOPs for the rounding noise of two of its four
                                   * GEMMs.  0 = none (every block is all-bf16 or all-e4m3).  Must be <= fp8_first_layer.  (ABI 6) */
    int32_t      rope_prefix;     /* d_rope_table: rows at the head of every sequence that are NOT rotated (1 = the class token) */
    /* 2-D rotary position embedding of the EVA02 vision towers (timm RotaryEmbeddingCat; NULL: none; ABI 10): device fp32
     * [T - rope_prefix][2][head_dim] = (cos row | sin row) per rotated position, the same for every head.  Applied to the Q and K columns of the QKV
     * buffer in place, INTERLEAVED pairs: (y[2i], y[2i+1]) = (x[2i] cos[2i] - x[2i+1] sin[2i], x[2i+1] cos[2i+1] + x[2i] sin[2i+1]).  Fixed-length
     * sequences (images), pre-LN bf16 path only. */
    const float* d_rope_table;
    int32_t      mlp_ln_dim;      /* mq_block_weights.mlp_ln_*: the un-padded hidden width the statistics run over (0 = mlp_dim) */
    int32_t      reserved2;
} mq_encoder_cfg;

/* ---- towers ------------------------------------------------------------------------ */

/* timm AttentionPoolLatent, the 'map' pooling head of the SigLIP ViTs (open_clip TimmModel, pool = "map"): one learned query
 * attends over all tokens, then x = x + mlp(norm(x)) */
typedef struct mq_map_head {
    const float* q;                            /* fp32 [W]: Linear_q(latent), computed once at load, times 1/sqrt(W / heads) */
    const void*  kv_w;   const float* kv_b;    /* bf16 [2W, W], fp32 [2W]  (keys | values) */
    const void*  proj_w; const float* proj_b;  /* bf16 [W, W], fp32 [W] */
    const float* ln_g;   const float* ln_b;    /* fp32 [W] */
    const void*  fc1_w;  const float* fc1_b;   /* bf16 [F, W], fp32 [F] */
    const void*  fc2_w;  const float* fc2_b;   /* bf16 [W, F], fp32 [W] */
} mq_map_head;

typedef struct mq_vit_weights {
    const void*  patch_w;      /* bf16 [W, Kp]  conv1 weight flattened (c, ky, kx), K zero-padded to Kp = ceil64(3*P*P) */
    const float* cls;          /* [W]   class embedding (MQ_VIT_POOL_MAP: NULL, there is no class token) */
    const float* pos;          /* [T, W] positional embedding, T = 1 + (S/P)^2 (MQ_VIT_POOL_MAP: T = (S/P)^2, patch bias added in) */
    const float* ln_pre_g; const float* ln_pre_b;   /* NULL: no pre-LayerNorm (MQ_VIT_POOL_MAP; CLIPA; the EVA02 towers) */
    const mq_block_weights* blocks;  /* host array, `layers` entries */
    const float* ln_post_g; const float* ln_post_b; /* CLIP: on the class token; MQ_VIT_POOL_MAP: the trunk's final norm, all tokens */
    const void*  proj_w;       /* bf16 [D, W]  (= visual.proj transposed); MQ_VIT_POOL_MAP: NULL (D == W, no projection) */
    const mq_map_head* map;    /* MQ_VIT_POOL_MAP only, else NULL */
    const float* proj_b;       /* fp32 [D] or NULL: bias of the projection (MQ_VIT_POOL_CLS; the timm EVA02 towers project through their classifier
                                * head, a Linear WITH bias; ABI 10) */
} mq_vit_weights;

typedef struct mq_vit_cfg {
    mq_encoder_cfg enc;
    int32_t image_size;  /* S: 224 */
    int32_t patch_size;  /* P: 32 / 14 / 16 */
    int32_t out_dim;     /* D */
    float mean[3];       /* preprocessing normalisation (clip_utils.py:32-33 by default) */
    float std[3];
    int32_t pool;        /* MQ_VIT_POOL_CLS (0): open_clip VisionTransformer — class token, ln_pre, ln_post(class token) @ proj;
                          * MQ_VIT_POOL_MAP (1): timm SigLIP ViT — no class token, no ln_pre, norm(all tokens) -> attention-pool head */
    int32_t map_mlp_dim; /* F of the attention-pool head's MLP (MQ_VIT_POOL_MAP) */
    int32_t pool_dim;    /* MQ_VIT_POOL_QUERY: width Dp of the attentional pooler (keys, values, output; <= enc.width); else 0 */
    int32_t pool_heads;  /* MQ_VIT_POOL_QUERY: its heads (Dp / pool_heads = 64 / 96 / 128 ...) */
} mq_vit_cfg;

typedef struct mq_clip_text_weights {
    const float* tok_emb;      /* fp32 [V, W] token embedding */
    const float* pos;          /* fp32 [ctx, W] */
    const mq_block_weights* blocks;
    const float* ln_final_g; const float* ln_final_b;
    const void*  proj_w;       /* bf16 [D, W] (= text_projection transposed) */
    const float* proj_b;       /* fp32 [D] or NULL (SigLIP text towers: text_projection is a Linear with bias) */
} mq_clip_text_weights;

typedef struct mq_clip_text_cfg {
    mq_encoder_cfg enc;
    int32_t vocab;
    int32_t ctx;      /* 77 */
    int32_t out_dim;
    int32_t cls_pos;  /* > 0 (CoCa text towers, open_clip TextTransformer embed_cls): the LAST row of every sequence is the appended class
                       * embedding — it takes position `cls_pos` (= the text context length) instead of its index; sequences may then hold
                       * ctx + 1 rows (MQ_MASK_CAUSAL_CLS: a full-length text carries the class row twice); 0 = off */
} mq_clip_text_cfg;

typedef struct mq_bert_weights {
    const float* word_emb;   /* fp32 [V, W] */
    const float* pos_emb;    /* fp32 [P, W] */
    const float* type_emb;   /* fp32 [2, W] (mq_encode_bert uses row 0: token_type_ids are all zero; mq_score_pairs_bert looks the row up per token) */
    const float* emb_ln_g; const float* emb_ln_b;
    const mq_block_weights* blocks;
    /* optional projection head on the pooled row (NULL: none) — open_clip's HFTextEncoder with proj "mlp" (the text tower of
     * open_clip/xlm-roberta-base-ViT-B-32 and xlm-roberta-large-ViT-H-14): Linear(W, proj_hidden) -> GELU -> Linear(proj_hidden, out_dim),
     * both without bias in open_clip (proj1_b: fp32 [proj_hidden], zeros then).  bf16 row-major [out_features, in_features].
     * proj2_w == NULL with proj1_w set: ONE biased Linear(W, out_dim) instead (multilingual_clip's `LinearTransformation`, the M-CLIP text
     * encoders of the reference's multilingual_clip loader: clip_utils.py:521-565); mq_bert_cfg.proj_hidden is 0 then. */
    const void*  proj1_w;
    const float* proj1_b;
    const void*  proj2_w;
} mq_bert_weights;

typedef struct mq_bert_cfg {
    mq_encoder_cfg enc;
    int32_t vocab;
    int32_t max_pos;
    int32_t pool;     /* MQ_POOL_* */
    int32_t proj_hidden; /* hidden width of the MLP head (multiple of 64), 0 for the single-Linear head / no head */
    int32_t out_dim;     /* 0: no projection head, d_out is [nseq, W]; else d_out is [nseq, out_dim] */
} mq_bert_cfg;

/* ---- library info ------------------------------------------------------------------ */
int         mq_abi_version(void);
const char* mq_last_error(void);
/* name of the code object arch this library was built for ("gfx950") */
const char* mq_build_arch(void);
/* ABI 11 — MQ_OK when `device` (-1 = the current one) is what the kernels are laid out for: gfx950 with 256 CUs (one whole MI355X, 8 XCDs).  The
 * persistent GEMM grids, the XCD-aware tile order and the in-kernel tail are sized for exactly that; a DPX / CPX partition or another part is
 * refused (MQ_ERR_UNSUPPORTED) by every tiled GEMM launch and, earlier, by the Python loaders at load(). */
int mq_check_device(int device);

/* Host-side staging helper (no GPU work): copy n host buffers to h_dst + h_dst_off[i] with up to `threads` copy threads, in one call
 * (the Python loaders pack a request's decoded images into one pinned buffer this way: one GIL release per request). */
int mq_host_gather(const void* const* h_src, const int64_t* h_bytes, const int64_t* h_dst_off, int64_t n, void* h_dst, int32_t threads);
/* the same with the destination's capacity in bytes: an item that would leave [0, dst_bytes) is refused (MQ_ERR_INVALID) before any copy */
int mq_host_gather_checked(const void* const* h_src, const int64_t* h_bytes, const int64_t* h_dst_off, int64_t n, void* h_dst,
                           int64_t dst_bytes, int32_t threads);

/* ---- workspace sizing (bytes of device scratch the caller must provide) ------------- */
/* rows = total token rows in the call (images: n*T; text: sum of sequence lengths);
 * nseq = number of sequences. */
size_t mq_encoder_workspace_bytes(const mq_encoder_cfg* cfg, int64_t rows, int64_t nseq);
size_t mq_vit_workspace_bytes(const mq_vit_cfg* cfg, int64_t n_images);
size_t mq_clip_text_workspace_bytes(const mq_clip_text_cfg* cfg, int64_t rows, int64_t nseq);
size_t mq_bert_workspace_bytes(const mq_bert_cfg* cfg, int64_t rows, int64_t nseq);

/* ---- hot-path entry points ----------------------------------------------------------- */

/* Image tower on raw pixels already at model resolution.
 * d_pixels: uint8 [n, S, S, 3] (HWC, RGB).  ToTensor (/255) + Normalize(mean,std) are fused
 * into the patch gather.  d_out: fp32 [n, D]; L2-normalised when normalize != 0. */
int mq_encode_image_u8(const mq_vit_cfg* cfg, const mq_vit_weights* w,
                       const uint8_t* d_pixels, int64_t n, float* d_out, int normalize,
                       void* d_workspace, size_t workspace_bytes, void* stream);

/* Image tower on already-preprocessed tensors (what the reference's `.preprocess`
 * returns, add_docs.py:130-134): d_pixels fp32 [n, 3, S, S] (CHW, normalised). */
int mq_encode_image_f32(const mq_vit_cfg* cfg, const mq_vit_weights* w,
                        const float* d_pixels, int64_t n, float* d_out, int normalize,
                        void* d_workspace, size_t workspace_bytes, void* stream);

/* CLIP text tower.  Sequences are PACKED: d_ids int32 [rows] holds the tokens of sequence
 * s at [cu_seqlens[s], cu_seqlens[s+1]) where each sequence is SOT ... EOT (the tokens after
 * EOT never influence the pooled EOT row under the causal mask, so they are not run).
 * d_cu_seqlens: int32 [nseq+1] on device; h_cu_seqlens: the same array on the host.
 * The pooled row is the LAST row of each sequence (the EOT token = argmax id,
 * open_clip text pooling).  To reproduce the reference's padded 77-token execution
 * exactly, pass every sequence with its full 77 ids and d_pool_rows = argmax rows. */
int mq_encode_clip_text(const mq_clip_text_cfg* cfg, const mq_clip_text_weights* w,
                        const int32_t* d_ids, const int32_t* d_cu_seqlens,
                        const int32_t* h_cu_seqlens, int64_t nseq,
                        const int32_t* d_pool_rows, /* int32 [nseq] absolute row to pool, or NULL = last row */
                        float* d_out, int normalize,
                        void* d_workspace, size_t workspace_bytes, void* stream);

/* BERT-family text tower + pooling (+ L2).  Packed like mq_encode_clip_text: only the
 * attention_mask==1 tokens of each sequence are rows (results are identical to the
 * reference's pad-to-longest execution because padded keys are masked out and padded rows
 * are excluded from the pool: hugging_face_model.py:205-209). */
int mq_encode_bert(const mq_bert_cfg* cfg, const mq_bert_weights* w,
                   const int32_t* d_ids, const int32_t* d_cu_seqlens,
                   const int32_t* h_cu_seqlens, int64_t nseq,
                   float* d_out, int normalize,
                   void* d_workspace, size_t workspace_bytes, void* stream);

/* ---- image preprocessing on device (K10 / K11) ----------------------------------------- */
/* All images are uint8 HWC RGB, dense (row stride = w*3), image i at d_src + h_src_off[i] with
 * size h_heights[i] x h_widths[i] (host arrays: the planning — Pillow's coefficient tables — is host
 * work, the pixel passes are device work).  Results are bit-identical to Pillow's
 * Image.resize(..., BICUBIC) (antialiased two-pass 8-bit resampler), which is what the reference's
 * transforms run on the CPU. */

/* CLIP transform up to uint8  (clip_utils.py:61-63: Resize(S, BICUBIC) -> CenterCrop(S)):
 * d_out uint8 [n, S, S, 3].  Feed it to mq_encode_image_u8 (which fuses ToTensor + Normalize) or to
 * mq_to_tensor_normalize. */
size_t mq_clip_resize_workspace_bytes(const int32_t* h_heights, const int32_t* h_widths, int64_t n, int32_t S);
int mq_clip_resize_crop_u8(const uint8_t* d_src, const int64_t* h_src_off, const int32_t* h_heights,
                           const int32_t* h_widths, int64_t n, int32_t S, uint8_t* d_out,
                           void* d_workspace, size_t workspace_bytes, void* stream);

/* Plain PIL.Image.resize((out_w, out_h), BICUBIC) of every image (no aspect preservation, no crop): the
 * chunker's working image (processing/image.py:143).  d_out uint8 [n, out_h, out_w, 3]. */
size_t mq_resize_workspace_bytes(const int32_t* h_heights, const int32_t* h_widths, int64_t n, int32_t out_h, int32_t out_w);
int mq_resize_u8(const uint8_t* d_src, const int64_t* h_src_off, const int32_t* h_heights, const int32_t* h_widths,
                 int64_t n, int32_t out_h, int32_t out_w, uint8_t* d_out, void* d_workspace, size_t workspace_bytes,
                 void* stream);

/* The same with the resampling filter chosen: filter = 2 (PIL.Image.BILINEAR) or 3 (PIL.Image.BICUBIC).  CLIPA checkpoints are
 * preprocessed with a BILINEAR squash to S x S (open_clip's _apcfg(), which the reference selects for
 * image_preprocessor = "CLIPA": core/inference/embedding_models/open_clip_model.py:87-97). */
size_t mq_resize_filter_workspace_bytes(const int32_t* h_heights, const int32_t* h_widths, int64_t n, int32_t out_h, int32_t out_w,
                                        int32_t filter);
int mq_resize_filter_u8(const uint8_t* d_src, const int64_t* h_src_off, const int32_t* h_heights, const int32_t* h_widths,
                        int64_t n, int32_t out_h, int32_t out_w, int32_t filter, uint8_t* d_out, void* d_workspace,
                        size_t workspace_bytes, void* stream);

/* Grid chunker (PatchifySimple, processing/image.py:120-151; 'simple' / 'overlap' patch methods):
 * every image is resized to 240x240 (no aspect preservation), cut into the whole image + the
 * generate_boxes(hn, wn, overlap) grid (image_utils.py:165-202), and every crop is put through the CLIP
 * transform above.  d_out uint8 [n * count, S, S, 3] with count = mq_chunk_grid_count(hn, wn, overlap);
 * h_boxes (host, may be NULL) float [n * count, 4] = (x1, y1, x2, y2) in ORIGINAL pixel coordinates
 * (rescale_box, image_utils.py:141-163). */
int    mq_chunk_grid_count(int32_t hn, int32_t wn, int32_t overlap);
size_t mq_chunk_grid_workspace_bytes(const int32_t* h_heights, const int32_t* h_widths, int64_t n,
                                     int32_t hn, int32_t wn, int32_t overlap, int32_t S);
int mq_chunk_grid_u8(const uint8_t* d_src, const int64_t* h_src_off, const int32_t* h_heights,
                     const int32_t* h_widths, int64_t n, int32_t hn, int32_t wn, int32_t overlap, int32_t S,
                     uint8_t* d_out, float* h_boxes, void* d_workspace, size_t workspace_bytes, void* stream);

/* Resize by the source image's MODE, as Pillow itself resizes it.  The reference's transform calls PIL's Image.resize on whatever mode
 * the decoder produced and converts to RGB only afterwards (src/marqo/s2_inference/clip_utils.py:61-64; open_clip image_transform,
 * open_clip_model.py:84-97), and Image.resize is mode dependent:
 *   MQ_IMG_RGB      uint8 [h, w, 3]: the given filter (2 = Image.BILINEAR, 3 = Image.BICUBIC) — what mq_clip_resize_crop_u8 /
 *                   mq_resize_filter_u8 do; also right for "L" images replicated to RGB by the caller (the filter is per band);
 *   MQ_IMG_NEAREST  uint8 [h, w, 3] converted from a palette ("P") or bilevel ("1") image: Pillow forces NEAREST for these modes
 *                   (nearest sampling commutes with the palette lookup, so the caller converts first);
 *   MQ_IMG_RGBA     uint8 [h, w, 4] (RGBA; LA expanded to RGBA by the caller), images 4-byte aligned: premultiply by alpha, resample
 *                   all four bands, un-premultiply (Pillow's "RGBa" round trip), alpha dropped = the transform's .convert("RGB").
 *                   An image that needs no resize at all passes its colour bytes through untouched, as in the reference.
 * crop != 0: Resize(out_h) on the shorter side + CenterCrop(out_h) (the CLIP transform; out_w == out_h); crop == 0: plain
 * Image.resize((out_w, out_h)).  d_out uint8 [n, out_h, out_w, 3] in every mode; bit-identical to Pillow. */
#define MQ_IMG_RGB 0
#define MQ_IMG_NEAREST 1
#define MQ_IMG_RGBA 2
size_t mq_resize_mode_workspace_bytes(const int32_t* h_heights, const int32_t* h_widths, int64_t n, int32_t out_h, int32_t out_w,
                                      int32_t filter, int32_t crop, int32_t mode);
int mq_resize_mode_u8(const uint8_t* d_src, const int64_t* h_src_off, const int32_t* h_heights, const int32_t* h_widths, int64_t n,
                      int32_t out_h, int32_t out_w, int32_t filter, int32_t crop, int32_t mode, uint8_t* d_out,
                      void* d_workspace, size_t workspace_bytes, void* stream);

/* Decoded Pillow images hold 4 bytes per pixel (R, G, B, pad: Imaging "RGB" storage); the loaders stage those bytes as they are (a
 * zero-copy view through Pillow's Arrow export instead of PIL's 4 -> 3 byte repack on the host, which is what Image.tobytes /
 * np.asarray — and torchvision's ToTensor in the reference, clip_utils.py:65 — spend their time on) and repack on the device.
 * d_staging: one buffer holding the pixel bytes and, at jobs_off (multiple of 8), n records {int64 src_off, int64 dst_off, int64 npix}
 * (byte offsets into d_staging / d_rgb, both multiples of 256).  d_rgb receives packed RGB. */
int mq_unpack_rgbx(const uint8_t* d_staging, int64_t jobs_off, int64_t n, int64_t max_npix, uint8_t* d_rgb, void* stream);

/* ToTensor + Normalize (clip_utils.py:65-66): uint8 [n, S, S, 3] -> fp32 [n, 3, S, S]; this is the
 * tensor the reference's `.preprocess` hands to add_docs.py:130-134. mean/std: host float[3]. */
int mq_to_tensor_normalize(const uint8_t* d_u8, float* d_out, int64_t n, int32_t S,
                           const float* mean, const float* std, void* stream);

/* Pillow's fixed-point bicubic coefficient table of one axis (host only; exported for parity tests):
 * for output positions [first, first+count) of an in_size -> out_size resize, h_bounds int32
 * [count, 2] = (first source index, tap count), h_kk int32 [count, ksize] 22-bit fixed-point weights,
 * ksize = mq_resample_ksize(in_size, out_size). */
int mq_resample_ksize(int32_t in_size, int32_t out_size);
int mq_resample_coeffs(int32_t in_size, int32_t out_size, int32_t first, int32_t count,
                       int32_t* h_bounds, int32_t* h_kk);

/* ---- building blocks (exported for parity tests and for callers that compose) -------- */

/* fp8 (OCP e4m3) GEMM, K13:  out[M,N] = epilogue( (A8[M,K] @ W8[N,K]^T) * a_scale * w_scale[n] ).
 * A8, W8: e4m3 codes, row-major (lda, ldw in bytes, multiples of 16); K % 128 == 0.  d_a_scale: fp32 [M] when
 * a_scale_per_row != 0 (written by mq_layernorm_fp8), else one device scalar (static per-tensor scale).
 * d_w_scale fp32 [N] per output channel (mq_quantize_weights_fp8).  flags: one of
 *   OUT_F32 | BIAS (bf16 out) | BIAS|GELU|OUT_FP8 | BIAS|QUICKGELU|OUT_FP8 | BIAS|RESIDUAL|OUT_F32.
 * With OUT_FP8 the result is divided by *d_out_scale (device scalar) before conversion and, when d_amax != NULL,
 * max|value| is atomically folded into *d_amax (calibration of the static scale). */
int mq_gemm_fp8(const void* d_A8, int64_t lda, const void* d_W8, int64_t ldw, const float* d_a_scale,
                int a_scale_per_row, const float* d_w_scale, const float* d_bias, const float* d_residual,
                void* d_out, int64_t ldc, const float* d_out_scale, float* d_amax,
                int64_t M, int64_t N, int64_t K, int flags, void* stream);

/* W bf16 [N,K] -> e4m3 codes [N,K] + per-row scale[N] = absmax / 448 (done once at model load). */
int mq_quantize_weights_fp8(const void* d_W_bf16, int64_t ldw, void* d_W8, int64_t ld8, float* d_scale,
                            int64_t N, int64_t K, void* stream);

/* LayerNorm with e4m3 output and a dynamic per-row scale: q[r,:] = LN(x[r,:]) / s[r], s[r] = max|LN(x[r,:])| / 448. */
int mq_layernorm_fp8(const float* d_x, const float* d_g, const float* d_b, void* d_out_fp8, float* d_row_scale,
                     float* d_out_f32 /* optional fp32 copy of LN(x) (post-LN models), may be NULL */,
                     int64_t rows, int32_t W, float eps, void* stream);

/* the same with the input rows in bf16 (x_bf16 != 0: the bf16 residual stream of an fp8 tower; d_out_f32 must then be NULL) */
int mq_layernorm_fp8_ex(const void* d_x, int x_bf16, const float* d_g, const float* d_b, void* d_out_fp8, float* d_row_scale,
                        float* d_out_f32, int64_t rows, int32_t W, float eps, void* stream);

/* Per-row e4m3 quantisation without normalisation: q[r,:] = x[r,:] / s[r], s[r] = max|x[r,:]| / 448 (the GEMM operand of the
 * first block of a post-LN fp8 encoder). */
int mq_rowquant_fp8(const float* d_x, void* d_out_fp8, float* d_row_scale, int64_t rows, int32_t W, void* stream);

/* out[M,N] = epilogue(A[M,K] @ W[N,K]^T).  A, W bf16 row-major (lda, ldw in elements);
 * K % 64 == 0, N % 4 == 0.  bias fp32 [N]; residual fp32 [M, ldc]; out bf16 or fp32 [M, ldc]
 * (residual may alias out when MQ_EPI_OUT_F32). */
int mq_gemm_bf16(const void* d_A, int64_t lda, const void* d_W, int64_t ldw,
                 const float* d_bias, const float* d_residual, void* d_out, int64_t ldc,
                 int64_t M, int64_t N, int64_t K, int flags, void* stream);

/* The search path (tensor_search.py:1876-1911 -> vectorise() with ONE query; s2_inference.py:135-146 with a one-item batch): GEMMs of
 * M <= 80 rows (a query text; one ViT-B/32 image = 50 tokens).  Column-sliced skinny kernels (csrc/gemm_small.hip): one workgroup per 16 output columns, its 4 waves split K, so the
 * weight matrix is streamed once by the whole chip.  mq_gemm_bf16 routes such calls here by itself (mq_tune("small_m", rows), 0 = off);
 * the entry points are public for tests and for callers that hold a normalisation to fuse.
 *   mq_gemm_small_bf16:    flags as mq_gemm_bf16 (BIAS | RESIDUAL without OUT_F32 = bf16 residual in / out); K % 32 == 0, N % 4 == 0.
 *   mq_ln_gemm_small_bf16: out = act(LayerNorm(x) @ W^T + bias), the LayerNorm computed in the kernel's prologue (x fp32 [M, ldx], or the
 *                          bf16 residual stream when x_bf16 != 0); M <= 32, K <= 1280; flags BIAS [| GELU | QUICKGELU]; bf16 out.
 *                          d_ln_out (may be NULL; fp32 [M, K]; must not alias d_x) receives the normalised rows — what a post-LN
 *                          encoder (BERT) carries on as its residual. */
int mq_gemm_small_bf16(const void* d_A, int64_t lda, const void* d_W, int64_t ldw, const float* d_bias, const void* d_residual,
                       void* d_out, int64_t ldc, int64_t M, int64_t N, int64_t K, int flags, void* stream);
int mq_ln_gemm_small_bf16(const void* d_x, int64_t ldx, int x_bf16, const float* d_ln_g, const float* d_ln_b, float eps, const void* d_W,
                          int64_t ldw, const float* d_bias, void* d_out, int64_t ldc, int64_t M, int64_t N, int64_t K, int flags,
                          float* d_ln_out, void* stream);

/* The LayerNorm of a pre-LN block folded into the GEMM behind it (csrc/gemm_epilogue.h; the towers' QKV / fc1 GEMMs on the bf16 residual stream):
 *   mq_row_stats:    d_stats fp32 [rows][2] = (mean, rstd) of every bf16 row of d_x [rows, W] (W % 8 == 0, W <= 2048) — ONE read pass, 8 bytes written
 *                    per row; the LayerNorm launch it replaces read AND wrote the whole stream.
 *   mq_gemm_bf16_ln: out bf16 [M, N] = act( LN(A) @ W0^T + b0 ) computed as act( rstd * (A @ d_W^T - mean * d_colsum) + d_bias ) with
 *                    d_W = bf16(gamma * W0) [N, K], d_bias = b0 + W0 @ beta, d_colsum[n] = sum_k d_W[n, k], d_rowstats from mq_row_stats;
 *                    d_A: the UN-normalised bf16 rows (K = the normalised width).  flags: MQ_EPI_BIAS [| MQ_EPI_GELU | MQ_EPI_QUICKGELU].
 * Replaces what open_clip's ResidualAttentionBlock computes as ln_1 -> attn.in_proj / ln_2 -> mlp.c_fc
 * (reached from /root/reference/src/marqo/core/inference/embedding_models/open_clip_model.py:249-266).
 *   mq_gemm_bf16_rs + mq_row_stats_finalize: when the rows were just written by a residual GEMM of the bf16 stream, that GEMM can leave
 *                    per-row partial sums behind (d_partials fp32 [ceil(N/64)][M][2], SLOT-major since ABI 12: (sum, sum of squares) of the bf16 values it stored per
 *                    64-column slot) and the statistics pass shrinks to a finalise over those partials — same d_stats layout as mq_row_stats.
 *                    flags of mq_gemm_bf16_rs: MQ_EPI_BIAS | MQ_EPI_RESIDUAL (bf16 in / out, in place). */
#define MQ_EPI_ROW_STATS 64
#define MQ_EPI_LN_APPLY 128
/* ABI 11 — MQ_EPI_GLU (mq_gemm_bf16 / mq_gemm_bf16_ln with MQ_EPI_BIAS): the gated MLP's product in the (up | gate) GEMM's epilogue.  d_W's N = 2 F rows
 * come INTERLEAVED 16 at a time — rows 32 j .. 32 j + 15 = up units 16 j .. 16 j + 15, rows 32 j + 16 .. 32 j + 31 = the same units' gate rows — so one lane
 * holds up AND gate of the same hidden units; out bf16 [M, F] at row stride ldc: out[m, u] = (up + b_up) * silu(gate + b_gate).  N % 32 == 0. */
#define MQ_EPI_GLU 256
/* MQ_EPI_RELU (mq_gemm_bf16 with MQ_EPI_BIAS [| MQ_EPI_RESIDUAL], bf16 out): max(0, .) as the last step, after the residual add (the ResNet
 * towers' conv + BN + ReLU and conv3 + BN + identity + ReLU).  These combinations always run on the tiled GEMMs, whatever the row count.
 * MQ_EPI_BIAS | MQ_EPI_RELU is also an epilogue of mq_gemm_bf16_ln (LayerNorm folded in) and of the skinny kernels (mq_gemm_small_bf16,
 * mq_ln_gemm_small_bf16): the fc1 of an MQ_ACT_RELU encoder block, whatever its row count. */
#define MQ_EPI_RELU 512
int mq_gemm_bf16_rs(const void* d_A, int64_t lda, const void* d_W, int64_t ldw, const float* d_bias, const void* d_residual, void* d_out, int64_t ldc,
                    int64_t M, int64_t N, int64_t K, int flags, float* d_partials, void* stream);
int mq_row_stats_finalize(const float* d_partials, int32_t nslots, float* d_stats, int64_t rows, int32_t W, float eps, void* stream);
/* ABI 12 — LN_APPLY and ROW_STATS in one launch (csrc/gemm_bf16.hip; the EVA02 sub-LayerNorms, timm eva.py EvaAttention.norm / SwiGLU.norm, reached from
 * /root/reference/src/marqo/core/inference/embedding_models/open_clip_model.py:249-266): out = [residual +] LN(A) @ W0^T + b0 with d_W / d_bias / d_colsum
 * folded as for mq_gemm_bf16_ln, d_rowstats = (mean, rstd) of A's rows, and d_partials = (sum, sum of squares) per row and 64-column slot of what the
 * launch stores.  flags: MQ_EPI_BIAS | MQ_EPI_RESIDUAL (bf16 residual read-modify-write; d_partials [ceil(N/64)][M][2]) or MQ_EPI_BIAS | MQ_EPI_GLU
 * (d_residual NULL; out [M, N/2]; a slot = 64 GEMM columns = 32 hidden units: d_partials [ceil(N/64)][M][2] of the rounded products).
 * mq_attention_stats = mq_attention that also writes (sum, sum of squares) of every output row's rounded values per head: d_row_part [heads][rows][2] (slot-major; rows = the call's token rows). */
int mq_gemm_bf16_lnrs(const void* d_A, int64_t lda, const void* d_W, int64_t ldw, const float* d_bias, const float* d_colsum, const float* d_rowstats,
                      const void* d_residual, void* d_out, int64_t ldc, int64_t M, int64_t N, int64_t K, int flags, float* d_partials, void* stream);
int mq_attention_stats(const void* d_qkv, void* d_out, const int32_t* d_cu_seqlens, int64_t nseq, int32_t fixed_len, int32_t max_len, int32_t W,
                       int32_t heads, int32_t mask, float* d_row_part, int64_t rows, void* stream);
/* ABI 13 — attention + out-projection + residual + the LayerNorm statistics behind it in ONE launch (csrc/attn_proj.hip), for the short fixed-length
 * sequences of the ViT-B/32 image tower (the x = x + out_proj(attention(qkv)) half of open_clip's residual attention block, reached from
 * /root/reference/src/marqo/core/inference/embedding_models/open_clip_model.py:249-266): one workgroup per sequence keeps the attention output in LDS as
 * the GEMM's A operand, streams the weight, adds bias and residual in place and — holding complete rows — writes their (mean, rstd).
 *   d_qkv bf16 [rows, 3 W] (q | k | v, head-major), d_w bf16 [W, W] row-major, d_bias fp32 [W], d_x bf16 [rows, W] updated in place, d_rowstats fp32
 *   [rows][2] = (mean, rstd) with the LayerNorm's eps, as mq_row_stats_finalize leaves them (NULL: not written); rows = nseq * fixed_len, no mask.
 * The rows of d_x carry the same bits as mq_attention + mq_gemm_bf16(MQ_EPI_BIAS | MQ_EPI_RESIDUAL) would leave (same operations, same order), and the
 * statistics the bits of mq_gemm_bf16_rs + mq_row_stats_finalize (same per-lane chains, lane folds and slot order).  mq_attention_proj_ok: 1 for the shapes it takes
 * (1..64 tokens, W = 768, 12 heads), which is what the towers ask before planning a block around it (mq_tune("attn_proj", 0) turns that off).
 * d_pf_a / d_pf_b (may be NULL): weight ranges of the GEMMs behind the launch, touched one dword per 128-byte line so that they sit in the Infinity
 * Cache when those GEMMs start (what mq_gemm_bf16_rsf's d_pf_* are to the finalise this launch replaces). */
int mq_attention_proj_ok(int64_t nseq, int32_t fixed_len, int32_t W, int32_t heads);
int mq_attention_proj(const void* d_qkv, const void* d_w, const float* d_bias, void* d_x, float* d_rowstats, int64_t nseq, int32_t fixed_len, int32_t W,
                      int32_t heads, float eps, const void* d_pf_a, size_t pf_a_bytes, const void* d_pf_b, size_t pf_b_bytes, void* stream);
/* ABI 13 — mq_gemm_bf16_ln for fixed-length sequences of <= 64 rows, one workgroup per sequence (csrc/panel_gemm.hip: the QKV and fc1 GEMMs of the ViT-B/32
 * image tower at chip-filling batches; same reference call site as mq_attention_proj): the sequence's rows are staged once in LDS as the MFMA token operand
 * and the weight streams through per-wave rings in passes of 768 output columns.  Operands as mq_gemm_bf16_ln (d_W / d_bias / d_colsum folded, d_rowstats =
 * (mean, rstd) per row), K = 768, N a multiple of 768, rows = nseq * fixed_len; flags MQ_EPI_BIAS [| MQ_EPI_GELU | MQ_EPI_QUICKGELU]; d_out bf16 [rows, ldc].
 * Output bits = mq_gemm_bf16_ln's (same k order, same epilogue order).  Measured 17-30 % slower than the tiled kernel at the tower's shapes (3.5 / 4.7 MB of
 * weight per CU and image; profiles/r06za_panel_gemm_ab.txt): an opt-in — mq_encoder_forward takes it only under mq_tune("panel_gemm", n) / MQ_PANEL_GEMM=n,
 * from n sequences up when they fill the chip's 256 CUs in whole rounds to >= 3/4 (default 0 = never). */
int mq_panel_gemm_ln_ok(int64_t nseq, int32_t fixed_len, int64_t N, int64_t K);
int mq_panel_gemm_ln(const void* d_x, const void* d_W, const float* d_bias, const float* d_colsum, const float* d_rowstats, void* d_out, int64_t ldc,
                     int64_t nseq, int32_t fixed_len, int64_t N, int64_t K, int flags, void* stream);
/* ABI 11 — mq_gemm_bf16_rsf = mq_gemm_bf16_rs + the finalise, in ONE launch: on return (stream order) d_stats holds (mean, rstd) of every row of d_out,
 * bit for bit what mq_row_stats_finalize would have written (same slot order, same expression).  The last wave to arrive at a row band's counter sums
 * the band's partials inside the GEMM's own launch (csrc/gemm_epilogue.h, GemmLn::band_ctr); d_band_ctr: mq_gemm_band_counters(M) 32-bit counters, all
 * zero on entry, all zero again when the launch has finished (NULL: the finalise runs as a second launch, as before ABI 11).  d_pf_a / d_pf_b
 * (nullable): weight ranges of the GEMMs behind this one, touched one dword per 128-byte line on the way out (the prefetch the finalise launch carried). */
int64_t mq_gemm_band_counters(int64_t M);
int mq_gemm_bf16_rsf(const void* d_A, int64_t lda, const void* d_W, int64_t ldw, const float* d_bias, const void* d_residual, void* d_out, int64_t ldc,
                     int64_t M, int64_t N, int64_t K, int flags, float* d_partials, float* d_stats, float eps, uint32_t* d_band_ctr,
                     const void* d_pf_a, size_t pf_a_bytes, const void* d_pf_b, size_t pf_b_bytes, void* stream);
int mq_row_stats(const void* d_x_bf16, float* d_stats, int64_t rows, int32_t W, float eps, void* stream);
int mq_gemm_bf16_ln(const void* d_A, int64_t lda, const void* d_W, int64_t ldw, const float* d_bias, const float* d_colsum, const float* d_rowstats,
                    void* d_out, int64_t ldc, int64_t M, int64_t N, int64_t K, int flags, void* stream);

/* y = LayerNorm(x) * g + b over the last dim.  x fp32 [rows, W] gathered through an optional
 * row index (d_row_idx int32 [rows], NULL = identity).  Writes bf16 (d_out_bf16) and/or fp32
 * (d_out_f32); either may be NULL. */
int mq_layernorm(const float* d_x, const int32_t* d_row_idx, const float* d_g, const float* d_b,
                 void* d_out_bf16, float* d_out_f32, int64_t rows, int32_t W, float eps, void* stream);
/* the same with the input rows in bf16 (x_bf16 != 0): the LayerNorm of the towers' bf16 residual-stream form (mq_tune("residual_bf16", 1)) */
int mq_layernorm_ex(const void* d_x, int x_bf16, const int32_t* d_row_idx, const float* d_g, const float* d_b,
                    void* d_out_bf16, float* d_out_f32, int64_t rows, int32_t W, float eps, void* stream);

/* Multi-head attention over packed sequences.  d_qkv bf16 [rows, 3W] (q | k | v, head h at
 * columns h*hd .. h*hd+hd-1 of each third, hd = W / heads in {64, 96, 112, 128}; softmax scale 1/sqrt(hd)).
 * d_out bf16 [rows, W].  Either pass fixed_len > 0 (all sequences have that length, nseq = rows / fixed_len)
 * or d_cu_seqlens int32 [nseq+1] with max_len = the longest sequence (<= 8192; sequences beyond 640 keys at
 * hd = 64 / 320 keys at wider heads stream their K / V through the LDS in pieces). */
int mq_attention(const void* d_qkv, void* d_out, const int32_t* d_cu_seqlens, int64_t nseq,
                 int32_t fixed_len, int32_t max_len, int32_t W, int32_t heads, int32_t mask,
                 void* stream);

/* mq_attention (unmasked, bf16 out, 64-wide heads) with an additive relative-position bias on the scores: d_rel_bias as described at
 * mq_encoder_cfg.d_rel_bias. */
int mq_attention_bias(const void* d_qkv, void* d_out, const int32_t* d_cu_seqlens, int64_t nseq, int32_t fixed_len,
                      int32_t max_len, int32_t W, int32_t heads, const float* d_rel_bias, int32_t rel_span, void* stream);

/* mq_attention with an optional e4m3 output (out_fp8 != 0: d_out holds codes = value / *d_out_scale; max|value| is
 * folded into *d_amax when it is non-NULL). */
int mq_attention_ex(const void* d_qkv, void* d_out, const int32_t* d_cu_seqlens, int64_t nseq,
                    int32_t fixed_len, int32_t max_len, int32_t W, int32_t heads, int32_t mask,
                    int32_t out_fp8, const float* d_out_scale, float* d_amax, void* stream);

/* One full encoder stack, in place on the fp32 residual stream d_x [rows, W]. */
int mq_encoder_forward(const mq_encoder_cfg* cfg, const mq_block_weights* blocks,
                       float* d_x, int64_t rows, const int32_t* d_cu_seqlens, int64_t nseq,
                       int32_t fixed_len, int32_t max_len,
                       void* d_workspace, size_t workspace_bytes, void* stream);

/* mq_encoder_forward when only the rows listed in d_out_rows (int32 [n_out_rows], absolute row numbers) are read
 * afterwards — class-token / EOT / CLS pooling.  Every row still feeds the last block's keys and values, but its
 * out-projection, MLP and LayerNorms run on the listed rows only; those rows come out bit-identical to
 * mq_encoder_forward, every other row of d_x is unspecified on return.  The towers use this internally. */
int mq_encoder_forward_rows(const mq_encoder_cfg* cfg, const mq_block_weights* blocks,
                            float* d_x, int64_t rows, const int32_t* d_cu_seqlens, int64_t nseq,
                            int32_t fixed_len, int32_t max_len,
                            const int32_t* d_out_rows, int64_t n_out_rows,
                            void* d_workspace, size_t workspace_bytes, void* stream);

/* rows of x: out[r,:] = x[r,:] / ||x[r,:]||_2   (in place allowed) */
int mq_l2_normalize(const float* d_x, float* d_out, int64_t rows, int32_t D, void* stream);

/* The front / back ends of the towers and their gated-MLP and rotary steps (csrc/embed.hip).  Every tower reaches them internally; they are
 * exported for parity tests.  W % 4 == 0 and W <= 2048 wherever a row width W appears, unless stated otherwise.
 *   mq_patchify:     d_out bf16 [n (S/P)^2, Kp], row (img, py, px), column c P^2 + ky P + kx = pixel (py P + ky, px P + kx) channel c of d_in, which
 *                    is uint8 HWC [n, S, S, 3] (is_u8 != 0: (b / 255 - mean[c]) / std[c] in fp32) or normalised fp32 CHW [n, 3, S, S]; columns
 *                    >= 3 P^2 are 0.  mean / std are HOST pointers to 3 floats (read at the call; ignored for fp32 input).  Kp % 8 == 0.
 *   mq_vit_assemble: d_x [n T, W] = (class token d_cls at t = 0 | row b (T - 1) + t - 1 of d_patch_out) + d_pos[t], then LayerNorm(g, b) when g
 *                    is not NULL; d_cls NULL: no class token, row b T + t of d_patch_out.  fp32 inputs; d_x fp32, or bf16 when x_bf16 != 0.
 *   mq_embed_tokens: per sequence i of d_cu [nseq + 1], row r = tok[clamp(ids[r], 0, vocab - 1)] (+ pos[t]) (+ type0) (LayerNorm(g, b) when g is
 *                    not NULL) -> d_x fp32 and / or d_xb bf16 [rows, W] (either may be NULL); t = r - d_cu[i], except the last row of a
 *                    sequence takes pos[last_pos] when last_pos > 0 (CoCa's appended class embedding).
 *   mq_pool:         d_out fp32 [nseq, W] = the mean over each sequence's rows (MQ_POOL_MEAN) or its first row (MQ_POOL_CLS) of d_x fp32, then
 *                    x / max(||x||, 1e-12) when normalize != 0.
 *   mq_map_pool:     one learned query per head: d_out bf16 [n, W], head h = softmax(q_h . k_t) . v_t over the T rows of each image in d_kv bf16
 *                    [n T, 2 W] = (K | V); d_q fp32 [W] already scaled.  hd = W / heads a multiple of 8, <= 128; 1 <= T <= 4096.
 *   mq_avg_tokens:   d_out fp32 [n, W] = mean of rows [first, T) of each image of d_x (fp32, or bf16 when x_bf16 != 0).
 *   mq_move_rows:    gather (scatter == 0) d_dense[i] = d_sparse[d_idx[i]] or scatter (scatter != 0) d_sparse[d_idx[i]] = d_dense[i], rows of
 *                    row_bytes bytes (a multiple of 16); rows of d_sparse not named in d_idx are not touched.
 *   mq_last_rows / mq_cls_rows: d_rows int32 = d_cu[i + 1] - 1 per sequence / i T per image.
 *   mq_rope:         rotary embedding (rotate_half form, angle float(t) * inv_freq[i] with t the row's position in its sequence) on the Q and K
 *                    thirds of d_qkv bf16 [rows, 3 Wa], in place; V is not touched.  Sequences from d_cu, or fixed_len rows each when d_cu is
 *                    NULL.  Head width Wa / heads a multiple of 16; d_inv_freq fp32 [head width / 2].
 *   mq_rope_table:   rotary embedding from a table (the interleaved pairs of the EVA02 towers) on the Q and K thirds of d_qkv bf16 [rows, 3 Wa],
 *                    in place; d_table fp32 [T - prefix][2][hs] = (cos | sin); the first `prefix` rows of every T-row sequence and V are not touched.
 *                    rows % T == 0, hs = Wa / heads a multiple of 8.
 *   mq_glu:          d_buf bf16 [rows, 2F] = (up | gate) -> d_buf[:, :F] = up * act(gate), in place (row stride 2F).  interleaved != 0: up and gate
 *                    alternate 16 columns at a time (MQ_EPI_GLU's layout) and the product is written compactly to the first F columns;
 *                    F % 8 == 0 (F % 16 == 0 and F <= 4096 interleaved).
 *   mq_glu_ln:       d_buf bf16 [rows, 2F] -> d_buf[:, :F] = LayerNorm(product) g + b, statistics over the first Ft columns (the rest is the zero
 *                    padding of a width Ft model).  mode 0: (up | gate) halves; 1: interleaved as mq_glu; 2: the product is already in the first F
 *                    columns; 3: interleaved, the product only (no LayerNorm, g / b may be NULL).  F % 8 == 0, F <= 4096, Ft <= F, F % 16 == 0
 *                    in modes 1 and 3. */
int mq_patchify(const void* d_in, int32_t is_u8, void* d_out, int64_t n, int32_t S, int32_t P, int32_t Kp, const float* mean, const float* std,
                void* stream);
int mq_vit_assemble(const float* d_patch_out, const float* d_cls, const float* d_pos, const float* d_g, const float* d_b, void* d_x, int64_t n,
                    int32_t T, int32_t W, float eps, int32_t x_bf16, void* stream);
int mq_embed_tokens(const int32_t* d_ids, const int32_t* d_cu, int64_t nseq, const float* d_tok, const float* d_pos, const float* d_type0,
                    const float* d_g, const float* d_b, float* d_x, void* d_xb, int32_t W, int32_t vocab, float eps, int32_t last_pos, void* stream);
int mq_pool(const float* d_x, const int32_t* d_cu, int64_t nseq, float* d_out, int32_t W, int32_t pool, int32_t normalize, void* stream);
int mq_map_pool(const void* d_kv, const float* d_q, void* d_out, int64_t n, int32_t T, int32_t W, int32_t heads, void* stream);
int mq_avg_tokens(const void* d_x, int32_t x_bf16, float* d_out, int64_t n, int32_t T, int32_t first, int32_t W, void* stream);
int mq_move_rows(void* d_sparse, const int32_t* d_idx, void* d_dense, int64_t n, int64_t row_bytes, int32_t scatter, void* stream);
int mq_last_rows(const int32_t* d_cu, int32_t* d_rows, int64_t nseq, void* stream);
int mq_cls_rows(int32_t* d_rows, int64_t n, int32_t T, void* stream);
int mq_rope(void* d_qkv, const int32_t* d_cu, int64_t nseq, int32_t fixed_len, int32_t Wa, int32_t heads, const float* d_inv_freq, void* stream);
int mq_rope_table(void* d_qkv, int64_t rows, int32_t T, int32_t prefix, int32_t Wa, int32_t heads, const float* d_table, void* stream);
int mq_glu(void* d_buf, int64_t rows, int32_t F, int32_t act, int32_t interleaved, void* stream);
int mq_glu_ln(void* d_buf, int64_t rows, int32_t F, int32_t Ft, int32_t act, const float* d_g, const float* d_b, float eps, int32_t mode,
              void* stream);

/* ---- ConvNeXt image towers (csrc/convnext.hip) ------------------------------------------------------------------------------------------------
 * The open_clip convnext_* CLIP image towers (model_registry.py:274-339 in the reference; open_clip TimmModel over a timm ConvNeXt with timm_pool "",
 * i.e. timm's own head: global average pool -> LayerNorm, then open_clip's projection head).  Activations are NHWC bf16 rows [pixels, C]: the 1x1
 * convolutions (stem patches, downsample 2x2 patches, fc1 / fc2) are mq_gemm_bf16* calls, the LayerNorm of a block is folded into its fc1 GEMM
 * (statistics from the depthwise kernel's slot partials), gamma (layer scale) into its fc2 GEMM.  Every pointer below is a device pointer. */
#define MQ_CONVNEXT_HEAD_LINEAR 0   /* visual.head.proj: Linear(C3, out_dim) without bias */
#define MQ_CONVNEXT_HEAD_MLP 1      /* visual.head.mlp: Linear(C3, 2 out_dim) + bias -> GELU -> Linear(2 out_dim, out_dim) [+ bias] */

typedef struct mq_convnext_cfg {
    int32_t image_size;   /* S: multiple of 32 (224 / 256 / 320) */
    int32_t depths[4];    /* blocks per stage */
    int32_t dims[4];      /* channels per stage, multiples of 64; <= 3072 (stages 0-2: <= 2048) */
    float   ln_eps;       /* every LayerNorm of trunk and head */
    int32_t head;         /* MQ_CONVNEXT_HEAD_* */
    int32_t out_dim;      /* embedding width E */
    float   mean[3];      /* preprocessing normalisation of the u8 entry point */
    float   std[3];
} mq_convnext_cfg;

/* one block: x = x + gamma * fc2(GELU(fc1(LN(dwconv7x7(x))))) */
typedef struct mq_convnext_block_weights {
    const float* dw_w;    /* fp32 [49, C]: conv_dw.weight [C, 1, 7, 7] transposed to (ky * 7 + kx, c) */
    const float* dw_b;    /* fp32 [C] */
    const void*  fc1_w;   /* bf16 [4C, C] = bf16(norm.weight[k] * mlp.fc1.weight[n, k]) */
    const float* fc1_b;   /* fp32 [4C] = fc1.bias + fc1.weight @ norm.bias */
    const float* fc1_s;   /* fp32 [4C] = sum_k of the bf16 fc1_w row (the colsum of mq_gemm_bf16_ln) */
    const void*  fc2_w;   /* bf16 [C, 4C] = bf16(gamma[n] * mlp.fc2.weight[n, k]) */
    const float* fc2_b;   /* fp32 [C] = gamma * fc2.bias */
} mq_convnext_block_weights;

typedef struct mq_convnext_weights {
    const void*  stem_w;                      /* bf16 [C0, 64]: stem.0.weight [C0, 3, 4, 4] flattened (c, ky, kx), zero-padded from 48 to 64 columns */
    const float* stem_b;                      /* [C0] */
    const float* stem_ln_g; const float* stem_ln_b;   /* stem.1 */
    const float* ds_ln_g[4]; const float* ds_ln_b[4]; /* stages.i.downsample.0 (index 0 unused) */
    const void*  ds_w[4];                     /* bf16 [C_i, 4 C_{i-1}]: stages.i.downsample.1.weight [C_i, C_{i-1}, 2, 2] permuted to (ky, kx, c) columns */
    const float* ds_b[4];                     /* [C_i] */
    const mq_convnext_block_weights* blocks;  /* host array, sum(depths) entries, stage by stage */
    const float* head_ln_g; const float* head_ln_b;   /* head.norm */
    const void*  proj_w;   /* linear: bf16 [E, C3]; mlp: bf16 [2E, C3] (head.mlp.fc1) */
    const float* proj_b;   /* mlp: fp32 [2E]; linear: NULL */
    const void*  proj2_w;  /* mlp: bf16 [E, 2E] (head.mlp.fc2); linear: NULL */
    const float* proj2_b;  /* mlp: fp32 [E] or NULL */
} mq_convnext_weights;

/* workspace of one call of n images (0 for an unsupported cfg) */
size_t mq_convnext_workspace_bytes(const mq_convnext_cfg* cfg, int64_t n_images);
/* the whole tower in one call, with the contract of mq_encode_image_u8 / _f32: d_pixels uint8 [n, S, S, 3] (HWC RGB; ToTensor + Normalize with
 * cfg->mean / std fused into the stem's patch gather) or fp32 [n, 3, S, S] (normalised); d_out fp32 [n, E], L2-normalised when normalize != 0. */
int mq_encode_convnext_u8(const mq_convnext_cfg* cfg, const mq_convnext_weights* w, const uint8_t* d_pixels, int64_t n, float* d_out, int normalize,
                          void* d_workspace, size_t workspace_bytes, void* stream);
int mq_encode_convnext_f32(const mq_convnext_cfg* cfg, const mq_convnext_weights* w, const float* d_pixels, int64_t n, float* d_out, int normalize,
                           void* d_workspace, size_t workspace_bytes, void* stream);
/* building blocks (exported for parity tests):
 *   mq_convnext_dwconv:     d_y bf16 [n, H, W, C] = depthwise 7x7 (zero padding 3) of d_x bf16 [n, H, W, C] + d_b, taps d_w fp32 [49, C]; d_partials fp32
 *                           [C / 64][n H W][2] = (sum, sum of squares) of the stored bf16 values per pixel and 64-channel slot (mq_row_stats_finalize
 *                           turns them into (mean, rstd)).  C % 64 == 0; d_y must not alias d_x.
 *   mq_convnext_downsample: d_out bf16 [n (H/2) (W/2), 4 C], column (ky * 2 + kx) * C + c = LayerNorm(pixel (2 oy + ky, 2 ox + kx))[c] * g[c] + b[c],
 *                           (mean, rstd) per input pixel from d_stats fp32 [n H W][2] (mq_row_stats).  H, W even, C % 8 == 0.
 *   mq_convnext_pool_ln:    per image, LayerNorm over C of the mean of its HW rows of d_x bf16 [n, HW, C], in fp32; written as bf16 and / or fp32
 *                           [n, C] (either output may be NULL).  C % 8 == 0, C <= 3072. */
int mq_convnext_dwconv(const void* d_x, const float* d_w, const float* d_b, void* d_y, float* d_partials, int64_t n, int32_t H, int32_t W, int32_t C,
                       void* stream);
int mq_convnext_downsample(const void* d_x, const float* d_stats, const float* d_g, const float* d_b, void* d_out, int64_t n, int32_t H, int32_t W,
                           int32_t C, void* stream);
int mq_convnext_pool_ln(const void* d_x, const float* d_g, const float* d_b, void* d_out_bf16, float* d_out_f32, int64_t n, int32_t HW, int32_t C,
                        float eps, void* stream);

/* ---- ResNet image towers (csrc/resnet.hip) --------------------------------------------------------------------------------------------------
 * OpenAI CLIP's / open_clip's ModifiedResNet (RN50, RN101, RN50x4, RN50x16, RN50x64; model_registry.py:16-140 in the reference).  Activations are
 * NHWC bf16 rows [pixels, C]; every BatchNorm is folded into the convolution in front of it (weights and a bias).  Channel counts that are not a
 * multiple of 64 (the stem output w and the planes of stages 1-2 when w = 80 / 96) are zero-padded to one: pad64(c) columns, whose weights and
 * biases are 0, so that those columns stay 0 through the ReLUs.  The stem's inner width w / 2 is not padded.  Every pointer is a device pointer. */
typedef struct mq_resnet_cfg {
    int32_t image_size;   /* S: multiple of 32 */
    int32_t layers[4];    /* Bottleneck blocks per stage */
    int32_t width;        /* w: stem output width; stage i has planes w << i and 4 (w << i) output channels; w % 16 == 0 */
    int32_t heads;        /* attention-pool heads = 32 w / 64 */
    int32_t out_dim;      /* embedding width E (attnpool.c_proj) */
    float   mean[3];      /* preprocessing normalisation of the u8 entry point */
    float   std[3];
} mq_resnet_cfg;

/* one Bottleneck block; P = pad64(planes), I = the padded input width, O = 4 planes.  3x3 weights: bf16 [Cout, Kp], column (ky * 3 + kx) * Cin + c,
 * Kp = 9 Cin rounded up to a multiple of 64, zero past 9 Cin. */
typedef struct mq_resnet_block_weights {
    const void* conv1_w; const float* conv1_b;   /* bf16 [P, I], fp32 [P]: conv1 * bn1 */
    const void* conv2_w; const float* conv2_b;   /* bf16 [P, Kp(P)], fp32 [P]: conv2 (3x3) * bn2 */
    const void* conv3_w; const float* conv3_b;   /* bf16 [O, P], fp32 [O]: conv3 * bn3 */
    const void* ds_w;    const float* ds_b;      /* bf16 [O, I], fp32 [O]: downsample.0 * downsample.1; NULL when the block has none */
} mq_resnet_block_weights;

typedef struct mq_resnet_weights {
    const void*  stem_w[3];   /* conv1 (3x3 / 2, Cin 3): bf16 [w/2, 64], column (ky * 3 + kx) * 3 + c, zero past 27; conv2: [w/2, Kp(w/2)]; conv3: [pad64(w), Kp(w/2)] */
    const float* stem_b[3];   /* the folded bn1..bn3 biases: [w/2], [w/2], [pad64(w)] */
    const mq_resnet_block_weights* blocks;   /* host array, sum(layers) entries, stage by stage */
    const float* pos;         /* fp32 [T, C]: attnpool.positional_embedding, T = (S/32)^2 + 1, C = 32 w */
    const void*  q_w; const float* q_b;      /* bf16 [C, C], fp32 [C]: q_proj scaled by 1/8 (= 64^-0.5) */
    const void*  kv_w; const float* kv_b;    /* bf16 [2C, C], fp32 [2C]: k_proj rows, then v_proj rows */
    const void*  c_w; const float* c_b;      /* bf16 [E, C], fp32 [E]: c_proj */
} mq_resnet_weights;

/* workspace of one call of n images (0 for an unsupported cfg) */
size_t mq_resnet_workspace_bytes(const mq_resnet_cfg* cfg, int64_t n_images);
/* the whole tower in one call, with the contract of mq_encode_convnext_u8 / _f32: d_pixels uint8 [n, S, S, 3] (HWC RGB, normalised with cfg->mean /
 * std in the stem gather) or fp32 [n, 3, S, S] (normalised); d_out fp32 [n, E], L2-normalised when normalize != 0. */
int mq_encode_resnet_u8(const mq_resnet_cfg* cfg, const mq_resnet_weights* w, const uint8_t* d_pixels, int64_t n, float* d_out, int normalize,
                        void* d_workspace, size_t workspace_bytes, void* stream);
int mq_encode_resnet_f32(const mq_resnet_cfg* cfg, const mq_resnet_weights* w, const float* d_pixels, int64_t n, float* d_out, int normalize,
                         void* d_workspace, size_t workspace_bytes, void* stream);
/* building blocks (exported for parity tests):
 *   mq_resnet_conv3x3:         d_y bf16 [n H W, ldy] columns 0..Cout-1 = [ReLU](3x3 convolution, stride 1, zero padding 1, of d_x bf16 [n, H, W, Cin] with d_w
 *                              (layout above) + d_b fp32 [Cout]); columns Cout..ldy-1 untouched.  Cin % 8 == 0, Cout % 4 == 0, both <= 4096; relu 0 / 1;
 *                              n H W < 2^30; d_y must not alias d_x.  An implicit GEMM with 64-bit activation addresses: no 2^31-byte limit on d_x / d_y.
 *   mq_resnet_stem_gather:     d_out bf16 [n (S/2)^2, 64], column (ky * 3 + kx) * 3 + c = the normalised pixel (2 oy + ky - 1, 2 ox + kx - 1) of channel
 *                              c (0 outside the image and past column 26); is_u8: d_pixels uint8 [n, S, S, 3] with mean / std (host arrays), else fp32
 *                              [n, 3, S, S] (mean / std ignored).  S even.
 *   mq_resnet_avgpool2:        d_out bf16 [n (H/2) (W/2), C] = mean of each 2x2 window of d_x bf16 [n, H, W, C].  H, W even, C % 8 == 0.
 *   mq_resnet_attnpool_tokens: d_tokens bf16 [n, HW + 1, C]: row 0 = mean of the HW rows of d_x bf16 [n, HW, C] + d_pos[0], row 1 + p = row p + d_pos[1 + p]
 *                              (d_pos fp32 [HW + 1, C]).  C % 8 == 0, HW + 1 <= 256.
 *   mq_resnet_attnpool_attend: d_out bf16 [n, C], heads of 64: softmax(q . k^T) v per image and head, with d_q bf16 [n, C] (already scaled) and d_kv bf16
 *                              [n, T, 2C] (k columns, then v columns).  C % 64 == 0, T <= 256. */
int mq_resnet_conv3x3(const void* d_x, const void* d_w, const float* d_b, void* d_y, int64_t ldy, int64_t n, int32_t H, int32_t W, int32_t Cin,
                      int32_t Cout, int32_t relu, void* stream);
int mq_resnet_stem_gather(const void* d_pixels, int32_t is_u8, void* d_out, int64_t n, int32_t S, const float* mean, const float* std, void* stream);
int mq_resnet_avgpool2(const void* d_x, void* d_out, int64_t n, int32_t H, int32_t W, int32_t C, void* stream);
int mq_resnet_attnpool_tokens(const void* d_x, const float* d_pos, void* d_tokens, int64_t n, int32_t HW, int32_t C, void* stream);
int mq_resnet_attnpool_attend(const void* d_q, const void* d_kv, void* d_out, int64_t n, int32_t T, int32_t C, void* stream);

/* ---- attention-based image patching (csrc/patch_attn.hip) ---------------------------------------------------------------------------------
 * The 'dino-v1' / 'dino-v2' patch methods of the reference (s2_inference/processing/image.py:102-108, DINO_utils.py): where the class token of a
 * DINO ViT looks in the last block, and boxes around the bright regions of those maps.  Both are building blocks of engine/dino.py.
 *   mq_attention_cls_probs: d_qkv bf16 [nseq T, 3W] in mq_attention's layout, 64-wide heads (W == heads * 64), every sequence T rows long with the
 *                           class token in row 0.  d_probs fp32 [nseq, heads, T - 1] = softmax(q_0 . k_j / 8) over ALL T keys j, entries j = 1 .. T - 1
 *                           written (the class key counts in the denominator and is left out of the output).  fp32 arithmetic on exact bf16 products;
 *                           V is never read.  2 <= T <= 8192.
 *   mq_attn_boxes:          d_probs fp32 [n, heads, G G], one row-major G x G map per (image, head), G <= 32.  mode 0: one map per image, the mean over
 *                           the heads of |p|; mode 1: one map per head, negatives zeroed (maps = 1 in mode 0, heads in mode 1).  Per map: x / max(x) * 255 in float32,
 *                           truncated to uint8; Otsu's threshold over the 256-bin histogram as OpenCV's getThreshVal_Otsu computes it (double precision,
 *                           classes lighter than FLT_EPSILON skipped, first strict maximum); foreground = value > threshold; 8-connected foreground
 *                           components, of which those are reported that touch the 4-connected background joined to the frame (cv2.findContours with
 *                           RETR_EXTERNAL: a blob inside another blob's hole is not).  d_boxes int32 [n, maps, max_boxes, 4] = (x, y, x + w, y + h) in
 *                           grid cells, in the raster order of each component's first cell; d_counts int32 [n, maps] = components found (only the first
 *                           max_boxes are written; ceil(G / 2)^2 always suffice).  max_boxes >= 1.  A map whose maximum is 0 (all zero, or in mode 1 nothing
 *                           positive) has no defined rescale in the reference (0 / 0 cast to uint8); here every cell becomes level 0, the
 *                           threshold is 0 and the map reports no box (count 0). */
int mq_attention_cls_probs(const void* d_qkv, float* d_probs, int64_t nseq, int32_t T, int32_t W, int32_t heads, void* stream);
int mq_attn_boxes(const float* d_probs, int64_t n, int32_t heads, int32_t G, int32_t mode, int32_t* d_boxes, int32_t* d_counts, int32_t max_boxes,
                  void* stream);

/* ---- text tokenisation on device (K14) ------------------------------------------------------------------- */
/* The reference tokenises on the host with third-party code (open_clip SimpleTokenizer at
 * src/marqo/core/inference/embedding_models/open_clip_model.py:277, transformers BertTokenizer at
 * .../hugging_face_model.py:179-185).  These entry points run the same published algorithms (one GPU thread per text for the
 * splitting, one per word for the vocabulary work) on any UTF-8 text.  Character handling is table-driven (d_unicode: one 64-bit
 * entry per code point below 0x30000 — flags drop / whitespace / isolate / needs-host / letter / number / Hangul plus the
 * lower-cased, accent-stripped output code points — built on the host from Python's unicodedata / str.lower / regex, so it agrees
 * with the host tokenisers by construction).  Texts whose treatment depends on context the table cannot express (a flagged code
 * point, a code point >= 0x30000, a word longer than the per-thread scratch) come back with d_status[i] = 1, d_lens[i] = 0 and
 * are tokenised by the host tokeniser; every other text gets ids identical to the host ones.
 * Texts are UTF-8 bytes packed back to back: text i = d_text[d_offsets[i] .. d_offsets[i+1]).
 * The hash tables are built once per vocabulary by the host (marqo_amd/engine/gpu_tokenizers.py); layouts: tokenize_algo.h. */
typedef struct mq_wordpiece_vocab {
    const void*    d_slots;   /* mq_wp_entry[n_slots]: {u64 fnv1a hash, i32 id (-1 empty), u32 (pool_off << 8 | cont << 7 | len)} */
    const uint8_t* d_pool;    /* piece bytes (without the "##" prefix) */
    uint32_t n_slots;         /* power of two */
    int32_t unk_id, cls_id, sep_id, pad_id;
    int32_t lower;            /* do_lower_case (informational: the behaviour is in d_unicode) */
    int32_t max_word_chars;   /* 100 */
    const uint64_t* d_unicode;  /* [0x30000] character table for this vocabulary's basic tokenisation (tokenize_algo.h) */
} mq_wordpiece_vocab;

typedef struct mq_clip_bpe_vocab {
    const void*     d_slots;        /* mq_bpe_entry[n_slots]: {u32 key = a << 16 | b (0xffffffff empty), u32 rank, u32 merged id, u32 pad} */
    const uint16_t* d_byte_id;      /* [256] id of the one-byte symbol */
    const uint16_t* d_byte_end_id;  /* [256] id of the word-final one-byte symbol (unit + "</w>") */
    uint32_t n_slots;               /* power of two */
    int32_t sot_id, eot_id;
    int32_t lower;
    const uint64_t* d_unicode;      /* [0x30000] character table: lower-casing + the \s / \p{L} / \p{N} classes of the pre-tokeniser regex */
} mq_clip_bpe_vocab;

/* Scratch of one tokenisation call (spans, counts, per-byte piece slots): total_bytes = d_offsets[n], cap_tokens = max_length
 * (WordPiece) or ctx (CLIP). */
size_t mq_tokenize_workspace_bytes(int64_t n, int64_t total_bytes, int32_t cap_tokens);

/* BERT WordPiece: d_ids int32 [n, ld] rows = [CLS] pieces... [SEP] then pad_id (truncated to max_length like
 * truncation=True, max_length=...), d_lens[i] = tokens in row i including CLS / SEP. */
int mq_tokenize_wordpiece(const mq_wordpiece_vocab* v, const uint8_t* d_text, const int64_t* d_offsets, int64_t n,
                          int64_t total_bytes, int32_t max_length, int32_t* d_ids, int64_t ld, int32_t* d_lens,
                          int32_t* d_status, void* d_workspace, size_t workspace_bytes, void* stream);

/* CLIP byte-level BPE: d_ids int32 [n, ctx] rows = SOT ids... EOT, zero padded; over-long texts are cut to ctx with EOT in
 * the last position (open_clip tokenize).  d_lens[i] = SOT..EOT length (what mq_encode_clip_text packs to). */
int mq_tokenize_clip_bpe(const mq_clip_bpe_vocab* v, const uint8_t* d_text, const int64_t* d_offsets, int64_t n,
                         int64_t total_bytes, int32_t ctx, int32_t* d_ids, int32_t* d_lens, int32_t* d_status,
                         void* d_workspace, size_t workspace_bytes, void* stream);

/* GPT-2 / RoBERTa byte-level BPE (vocab.json + merges.txt; transformers RobertaTokenizer without add_prefix_space): no normalisation, the
 * pre-token pattern 's 't 're 've 'm 'll 'd |  ?\p{L}+ |  ?\p{N}+ |  ?[^\s\p{L}\p{N}]+ | \s+(?!\S) | \s+ over the raw text (classes from
 * d_unicode), byte symbols without a word-final variant, merges lowest rank first.  d_ids int32 [n, ld] rows = <s> ids... </s> then pad_id,
 * the first max_length - 2 ids kept; d_lens[i] = tokens in row i including <s> / </s>.  A pre-token of more than 128 bytes sends its text to
 * the host (d_status[i] = 1).  The caller guarantees that every merge's parts and result are vocabulary ids (< 65536) and routes texts that
 * spell a special token to the host.  Workspace: mq_tokenize_workspace_bytes(n, total_bytes, max_length).  (Added without an ABI bump:
 * new symbols only.) */
typedef struct mq_byte_bpe_vocab {
    const void*     d_slots;    /* mq_bpe_entry[n_slots], as mq_clip_bpe_vocab */
    const uint16_t* d_byte_id;  /* [256] id of the one-character string a byte maps to */
    const uint64_t* d_unicode;  /* [0x30000] character table: the \s / \p{L} / \p{N} classes only */
    uint32_t n_slots;           /* power of two */
    int32_t cls_id, sep_id, pad_id;
} mq_byte_bpe_vocab;

int mq_tokenize_byte_bpe(const mq_byte_bpe_vocab* v, const uint8_t* d_text, const int64_t* d_offsets, int64_t n,
                         int64_t total_bytes, int32_t max_length, int32_t* d_ids, int64_t ld, int32_t* d_lens,
                         int32_t* d_status, void* d_workspace, size_t workspace_bytes, void* stream);

/* SentencePiece unigram (XLM-RoBERTa checkpoints of the multilingual-e5 family; T5-style vocabularies of the SigLIP towers): the model's
 * own normaliser as a per-code-point map + whitespace rules, then the unigram Viterbi search (tokenize_algo.h).  Rows are
 * [prefix_id] ids + id_offset ... suffix_id pad_id..., truncated to max_length; <unk> is written as unk_out. */
typedef struct mq_sentencepiece_vocab {
    const void*     d_slots;      /* mq_sp_entry[n_slots]: every piece and every proper prefix of a piece */
    const uint8_t*  d_pool;       /* piece bytes */
    const float*    d_score;      /* [vocab] */
    const uint32_t* d_nmap;       /* [0x30000] (npool offset << 8) | normalised bytes; 0xff = needs host */
    const uint8_t*  d_npool;
    const uint8_t*  d_ccc;        /* [0x30000] canonical combining classes */
    uint32_t n_slots;             /* power of two */
    int32_t unk_id;
    float   unk_score;            /* min piece score - 10 */
    int32_t add_dummy_prefix, remove_extra_ws, max_piece_bytes;
    int32_t prefix_id, suffix_id, pad_id, id_offset, unk_out;
} mq_sentencepiece_vocab;

size_t mq_tokenize_sentencepiece_workspace_bytes(int64_t n, int64_t total_bytes, int32_t max_length);
int mq_tokenize_sentencepiece(const mq_sentencepiece_vocab* v, const uint8_t* d_text, const int64_t* d_offsets, int64_t n,
                              int64_t total_bytes, int32_t max_length, int32_t* d_ids, int64_t ld, int32_t* d_lens,
                              int32_t* d_status, void* d_workspace, size_t workspace_bytes, void* stream);

/* SentencePiece BPE (the NLLB vocabulary of the NLLB-CLIP text towers): the same vocabulary struct and normalisation stage as the unigram entry,
 * then SentencePiece's BPE encode per whitespace word (one thread per word): start from the characters, repeatedly merge the adjacent pair whose
 * concatenation is a piece with the highest score (leftmost on ties) until none is; a symbol that is no piece is <unk> (consecutive ones joined into one).  The caller guarantees
 * that no piece carries U+2581 behind its first character (merges then never cross a word).  unk_score is unused.  Rows as above.
 * Workspace: mq_tokenize_workspace_bytes(n, total_bytes, max_length). */
int mq_tokenize_sentencepiece_bpe(const mq_sentencepiece_vocab* v, const uint8_t* d_text, const int64_t* d_offsets, int64_t n,
                                  int64_t total_bytes, int32_t max_length, int32_t* d_ids, int64_t ld, int32_t* d_lens,
                                  int32_t* d_status, void* d_workspace, size_t workspace_bytes, void* stream);

/* padded id rows -> the packed layout of the text towers: d_packed[cu[s] + j] = d_padded[s * ld + j], j < cu[s+1] - cu[s] */
int mq_pack_ids(const int32_t* d_padded, int64_t ld, const int32_t* d_cu_seqlens, int64_t nseq, int32_t* d_packed,
                void* stream);

/* Weighted combination of sub-embeddings (multimodal-combination fields and weighted multi-term queries):
 *   out[g,:] = mean over the group's terms t of ( d_weights[t] * d_emb[d_rows[t], :] ),  t in [d_cu_terms[g], d_cu_terms[g+1])
 * replacing the host numpy of  src/marqo/core/inference/tensor_fields_container.py:346-365  (mode MQ_COMBINE_NORMALIZE:
 * divide by the L2 norm unconditionally, a zero vector gives NaN like numpy) and
 * src/marqo/tensor_search/tensor_search.py:1954-1963  (mode MQ_COMBINE_NORMALIZE_IF_NONZERO).  Accumulation is fp64 like
 * the reference; d_emb fp32 [*, ld]; d_rows int32 [terms] (NULL = term t reads row t); d_out fp32 [n_groups, D]. */
#define MQ_COMBINE_RAW 0
#define MQ_COMBINE_NORMALIZE 1
#define MQ_COMBINE_NORMALIZE_IF_NONZERO 2
int mq_weighted_combine(const float* d_emb, int64_t ld, const int32_t* d_rows, const float* d_weights,
                        const int32_t* d_cu_terms, int64_t n_groups, int32_t D, int32_t mode, float* d_out,
                        void* stream);

/* ---- native request queue: cross-request batching of the request threads' small calls (ABI 14) -----------------------------------------------------
 * The reference runs up to 8 indexing + 8 search request threads (src/marqo/api/configs.py:27-28), each calling vectorise() with one query
 * (src/marqo/tensor_search/tensor_search.py, the query vectorisation) or the few chunks of one document field
 * (src/marqo/core/inference/tensor_fields_container.py:179-223).  A queue merges what concurrent callers hand over into ONE
 * mq_encode_clip_text / mq_encode_bert call per group on worker threads of its own — no interpreter lock anywhere between a caller's hand-over and
 * its wake-up (the Python-level coalescer, marqo_amd/s2_inference/coalesce.py, pays that lock on every hand-off; csrc/queue.hip).
 *   - a request = nseq sequences, PACKED host token ids (h_ids int32 [sum of h_lens], sequence s at its running offset) + h_lens int32 [nseq];
 *     mq_queue_encode blocks until the request's rows are in h_out (fp32 [nseq, out_dim]); any number of threads may call it on one queue;
 *   - "natural" batching: a lone caller's request runs at once; requests that arrive while a merged call executes form the next group (up to
 *     max_seqs sequences / max_rows token rows per tower call).  depth = worker threads = merged calls in flight (each with its own HIP stream, device
 *     scratch and pinned staging, all allocated in mq_queue_create and nowhere else); window_us = how long a group that is not full is held back for
 *     company WHILE another merged call is executing (0 = never);
 *   - tower_cfg / tower_weights: mq_clip_text_cfg + mq_clip_text_weights (MQ_QUEUE_CLIP_TEXT) or mq_bert_cfg + mq_bert_weights (MQ_QUEUE_BERT); the queue
 *     keeps the POINTERS (a tower whose policy fields change after load — fp8 calibration, residual stream — is seen as it is at each call): both
 *     structs and everything they point to must outlive the queue;
 *   - a request is validated on its caller's thread (lengths within the tower's context, ids inside the embedding table): a bad request fails alone,
 *     before it can join a group.  If a merged call itself fails every request of that group gets its status and text;
 *   - embeddings are those of the merged call: rows of a batch are independent in these towers, so a request's rows do not depend on its company
 *     as long as lone and merged call take the same kernel family (the small-row families end at 320 token rows). */
#define MQ_QUEUE_CLIP_TEXT 0
#define MQ_QUEUE_BERT 1
#define MQ_QUEUE_IMAGE_F32 2 /* an image tower (mq_vit_cfg + mq_vit_weights) on preprocessed images: a request = n DEVICE pointers to fp32 [3, S, S] tensors
                              * (what the reference's `.preprocess` returns, add_docs.py:130-134) anywhere in HBM; the worker gathers a group's images into
                              * one batch (device-to-device) and runs ONE mq_encode_image_f32.  max_rows = max_seqs (an image is one "row" here).  The
                              * images must be complete when mq_queue_encode_images is entered (the workers' streams are not ordered behind any other) */
typedef struct mq_queue mq_queue;   /* opaque */
typedef struct mq_queue_cfg {
    int32_t kind;        /* MQ_QUEUE_* */
    int32_t device;      /* HIP device ordinal the tower's weights live on */
    int32_t max_seqs;    /* sequences per merged tower call (and per request) */
    int32_t max_rows;    /* token rows per merged tower call (and per request): >= the tower's context length */
    int32_t normalize;   /* != 0: L2-normalised rows */
    int32_t depth;       /* worker threads (lanes) = merged calls in flight: 1..4.  EQUAL lanes cost heavy load its large groups (measured: depth 1 > 4 > 3 > 2,
                          * profiles/r08d_queue_depth_window_sweep.txt: a small-row tower call is host-launch-bound whatever its size); the loaders use 2 with
                          * helper_seqs = 4 — the second lane only works under light load */
    int32_t window_us;   /* see above; 0 = a group never waits */
    int32_t graphs;      /* != 0: a group of ONE sequence (the search path's lone query) replays a hipGraph of its token count, captured at the second
                          * call of that count on a worker (~100 dependent small launches: 0.45 ms enqueued one by one, 0.3 ms as a graph) */
    int32_t helper_seqs; /* > 0 (with depth > 1): the lanes beyond the first are HELPERS — they take what is waiting only while that is at most this many
                          * sequences AND the group the first lane is executing is that small too.  Light load (two or three request threads: never more than
                          * one request waiting, nothing to merge) then runs its calls side by side instead of one behind the other; under heavy load the first
                          * lane's groups are large, the helpers sleep and it forms them alone.  0 = every lane takes whatever waits */
    int32_t reserved;
} mq_queue_cfg;
typedef struct mq_queue_stats {
    uint64_t requests;            /* served (mq_queue_encode calls that reached a worker) */
    uint64_t calls;               /* tower calls */
    uint64_t merged_calls;        /* ... of more than one request */
    uint64_t failed_calls;
    uint64_t sequences, rows;     /* totals over all calls */
    uint64_t max_call_sequences;  /* the largest group so far */
    uint64_t graphs;              /* single-sequence launch sequences captured */
    uint64_t graph_replays;       /* tower calls that were one hipGraphLaunch */
} mq_queue_stats;
int mq_queue_create(const mq_queue_cfg* cfg, const void* tower_cfg, const void* tower_weights, mq_queue** out);
int mq_queue_encode(mq_queue* q, const int32_t* h_ids, const int32_t* h_lens, int64_t nseq, float* h_out);
int mq_queue_encode_images(mq_queue* q, const float* const* d_images, int64_t n, float* h_out);   /* MQ_QUEUE_IMAGE_F32: d_images = HOST array of n device pointers */
int mq_queue_get_stats(mq_queue* q, mq_queue_stats* out);
/* serves what is still pending, joins the workers, frees the staging; no mq_queue_encode may be entered after this starts */
int mq_queue_destroy(mq_queue* q);


/* Run-time selection of a kernel variant (benchmark A/B and parity tests of every variant in one process).  TEST / BENCH ONLY: the
 * knobs are relaxed atomics (csrc/knobs.h; one table row each in csrc/knobs.hip) that the launch code of every request thread reads — a new
 * value takes effect from the next launch that reads it, so set them while no request is in flight if one call must run under one setting;
 * the loaders never touch them.  key (environment variable the initial value comes from, built-in default): values
 *   "gemm_mt" (MQ_GEMM_MT, 0): 0 = auto, else GEMM tile height in 32-row units (the bf16 and the fp8 tiles)
 *   "gemm_cgroup" (MQ_GEMM_CGROUP, 8): column tiles per L2 group, 0 = row-major walk
 *   "gemm_nh" (MQ_GEMM_NH, 0): 0 = the default tile plan, 1 = the (32 MT) x 128 tiles only, 3 = the 8-wave 256 x 256 tile on every row wherever
 *       N >= 256, 4 = the eager row-split plan.  Setting it also sets the fp8 GEMM's big-tile switch (no key of its own; MQ_GEMM_FP8_NH, 0:
 *       0 = plan, 1 = never, 3 = always) to the same value, 4 as 0
 *   "gemm_tail" (MQ_GEMM_TAIL, 0): 1 = the big tile's in-kernel split-K tail for a ragged last row of tiles
 *   "gemm_wd" (MQ_GEMM_WD, 0): csrc/gemm_wd.hip, the W-operand-from-global main loop: 0 = off, 2 / 3 = on with that many LDS stages of A,
 *       6 / 7 = the same with both k-halves' W loads issued together
 *   "rs_finalize" (MQ_GEMM_RS_FIN, 0): 1 = mq_gemm_bf16_rsf finalises the row statistics inside the GEMM's launch
 *   "row_select" (MQ_ROW_SELECT, 1): 0 = the towers run their last block on every row instead of the pooled rows only
 *   "ln_fold" (MQ_LN_FOLD, 2): 0 = LayerNorm kernels, 1 = folded into the QKV GEMM, 2 = and into fc1; needs the folded weights
 *   "subln_fold" (MQ_SUBLN_FOLD, 1; ABI 12): 0 = the EVA02 sub-LayerNorms run as LayerNorm passes instead of inside the out-projection / fc2 GEMMs
 *   "attn_proj" (MQ_ATTN_PROJ, 128; ABI 13): fewest fixed-length sequences from which a ViT-B/32-shaped block runs mq_attention_proj instead of
 *       attention + out-projection + finalise, 0 = never
 *   "panel_gemm" (MQ_PANEL_GEMM, 0; ABI 13): fewest fixed-length sequences from which the folded QKV / fc1 GEMMs of a 768-wide tower run as
 *       mq_panel_gemm_ln, 0 = never
 *   "residual_bf16" (MQ_RESIDUAL_BF16, 0): 1 = pre-LN bf16 towers without a policy of their own keep the residual stream in bf16
 *   "pool_strided" (MQ_POOL_STRIDED, 1): 0 = the ViT class-token rows of the pooled last block and the head go through an index vector, two
 *       gathers and a scatter instead of being read and updated where they lie
 *   "assemble_stats" (MQ_ASSEMBLE_STATS, 1): 0 = a row-statistics pass over x behind the ViT token assembly instead of the (mean, rstd) the
 *       assembly leaves itself
 *   "small_m" (MQ_SMALL_M, 80), "small_m_grouped" (MQ_SMALL_M_GROUPED, 320): row limits of the skinny GEMM kernels, 0 = never
 *   "ln_prefetch" (MQ_LN_PREFETCH, 1): 0 = the towers' LayerNorms do not prefetch the weights of the GEMMs behind them
 *   "ln_rows" (MQ_LN_ROWS, 2): 1 = one row per wave in the generic LayerNorm at any row count, 2 = two from 8192 rows
 *   "ln_bf16_wide" (MQ_LN_BF16_WIDE, 1): 0 = bf16 rows take the generic LayerNorm, 1 = the 16-byte form above small_m rows, 4 = that form with
 *       four rows per wave from 16384 rows
 *   "xcd_band" (MQ_XCD_BAND, 1): 0 = the row-wise kernels do not follow the GEMMs' XCD banding
 *   "attn_waves" (no variable, 0): 0 = auto, 4 / 8 wave64s per attention workgroup
 *   "gemm_addr_limit_mb" (no variable, 0): bytes / 2^20 one launch may address per operand, 0 = the 4 GiB of a 32-bit buffer offset: taller
 *       matrices go in row chunks
 * An unknown key is MQ_ERR_INVALID ("unknown key"). */
int mq_tune(const char* key, int value);
/* ABI 15: the current value of a knob (what mq_tune stored, or the value at load); "gemm_addr_limit_mb" reads 0 at the 4 GiB default */
int mq_tune_get(const char* key, int* value);

/* ---- per-kernel timing (bench.py roofline) ------------------------------------------- */
/* When enabled, every launch of a kernel family is bracketed by hipEvents on its stream.
 * mq_profile_collect synchronises, sums the elapsed time per family and resets.
 * family ids: 0 gemm, 1 layernorm, 2 attention, 3 embed/gather, 4 pool/head, 5 preprocess */
#define MQ_PROF_FAMILIES 6
int mq_profile_enable(int on);
int mq_profile_collect(double* ms_per_family /* [MQ_PROF_FAMILIES] */,
                       int64_t* launches_per_family /* [MQ_PROF_FAMILIES] */,
                       double* gemm_flops /* total 2*M*N*K over gemm launches */);

/* ---- measurement support (bench.py `roofline.peak_sustained_measured`; not on the product path) ---------------------------- */
/* A register-resident v_mfma_f32_16x16x32_bf16 burn (no LDS, no memory; 256 CUs x 4 SIMDs x 2 waves, pseudo-random operand bits) of
 * about target_ms on `stream`; waits for it.  *tflops = the dense bf16 rate this chip sustains at the clock it holds under full MFMA
 * load, *shader_mhz = that clock (s_memtime ticks / wall time).  d_scratch: >= 32 KiB of device memory.  No reference counterpart. */
int mq_probe_mfma_peak(double target_ms, void* d_scratch, int64_t scratch_bytes, double* tflops, double* shader_mhz, void* stream);

/* ---- text reranking: cross-encoder scoring on the BERT tower (csrc/rerank.hip) --------------------------------------------------------------
 * s2_inference/reranking/rerank.py rerank_search_results -> cross_encoders.py ReRankerText -> sentence-transformers CrossEncoder.predict in the
 * reference: a BertForSequenceClassification (encoder, pooler = tanh(Linear) on the [CLS] row, one-logit classifier) over (query, chunk) pairs.
 * Additions to ABI 14: nothing above changes.  Every pointer is a device pointer unless its name starts with h_.
 *
 *   mq_pair_plan:   per pair i of ONE query of la = Lq pieces and document i of lb = clamp(d_doc_len[i] - 2, 0, ld - 2) pieces, the lengths kept
 *                   by the `tokenizers` library's LongestFirst truncation (the fast tokenizers' truncation="longest_first"; NOT the slow
 *                   tokenizers' one-token-at-a-time loop) to B = max_length - 3 pieces: both when la + lb <= B; else with s = min, l = max
 *                   (a tie counts the SECOND text as the longer): l' = s when s > B, else max(s, B - s); when s + l' > B: s = B / 2,
 *                   l' = B - s; the longer text keeps l'.  d_keep_a / d_keep_b int32 [n]; d_total int32 [n] = a + b + 3.  max_length >= 4.
 *   mq_pair_plan_n: the same rule for a pair sequence with `specials` special tokens (0 .. 8): B = max_length - specials, d_total = a + b +
 *                   specials, max_length >= specials + 1.  mq_pair_plan is mq_pair_plan_n with specials = 3; XLM-RoBERTa's
 *                   <s> a </s> </s> b </s> has 4.
 *   mq_pack_pairs:  d_ids / d_type_ids int32 [rows]: sequence i at [d_cu[i], d_cu[i + 1]) = [CLS] q[:a] [SEP] (type 0) d_i[:b] [SEP] (type 1);
 *                   d_query int32 [Lq] holds the query's pieces only, d_docs int32 [n, ld] rows [CLS] pieces [SEP] pad (mq_tokenize_wordpiece's
 *                   layout: the pieces start at column 1).  d_cu int32 [n + 1] is the exclusive scan of d_total (the caller's: it needs the
 *                   host copy for the tower anyway).  Both texts keep their prefix.  Nothing at or beyond row `rows` is written.
 *   mq_pack_pairs_xlmr: d_ids int32 [rows]: sequence i at [d_cu[i], d_cu[i + 1]) = cls_id q[:a] sep_id sep_id d_i[:b] sep_id (XLM-RoBERTa's
 *                   <s> a </s> </s> b </s>; no type ids: the family has one type row).  d_query int32 [Lq] holds the query's pieces only, d_docs
 *                   int32 [n, ld] rows <s> pieces </s> <pad> (mq_tokenize_sentencepiece's layout: the pieces start at column 1); d_keep_a /
 *                   d_keep_b / d_cu from mq_pair_plan_n with specials = 4.  Both texts keep their prefix.  Nothing at or beyond row `rows` is
 *                   written.
 *   mq_embed_tokens_typed: mq_embed_tokens with a type id per row: + d_type_emb[clamp(d_type_ids[r], 0, type_vocab - 1)] where mq_embed_tokens
 *                   adds row 0 — same order of the additions (token, position, type), so all-zero type ids give mq_embed_tokens' bits.
 *   mq_score_head:  d_h fp32 [n, W] (the final [CLS] rows) -> y = tanh(pooler_w bf16(h) + pooler_b) (mq_gemm_bf16: bf16 operands, fp32
 *                   accumulation; tanhf in fp32), z = cls_w . y + cls_b -> d_logits fp32 [n]; d_scores (NULL ok) = 1 / (1 + exp(-z)).
 *                   W % 64 == 0, W <= 2048.  Scratch: mq_score_head_workspace_bytes(n, W).
 *   mq_score_pairs_bert: typed embedding -> the encoder with mq_encode_bert's MQ_POOL_CLS row selection -> the [CLS] rows (d_cls_rows fp32
 *                   [nseq, W], NULL ok: bit-identical to mq_encode_bert(pool = CLS, normalize = 0) when the type rows agree) -> mq_score_head.
 *                   bf16 encoders only (MQ_PREC_FP8 is refused).  Scratch: mq_score_pairs_workspace_bytes(cfg, rows, nseq).
 *   mq_score_pairs_xlmr: mq_score_pairs_bert for an encoder with ONE type row and a position offset (XLMRobertaForSequenceClassification): no
 *                   type ids; the embedding is mq_encode_bert's own (mq_embed_tokens: token + position + type row 0), so token t of a sequence
 *                   takes row t of mq_bert_weights.pos_emb.  As for mq_encode_bert, the host hands that table over from row padding_idx + 1
 *                   on: the position ids of a packed pair run offset, offset + 1, ... over the whole pair, which is transformers'
 *                   create_position_ids_from_input_ids on an unpadded row.  The head is RoBERTa's classification head under the names of
 *                   mq_score_head_weights: pooler_w / pooler_b = classifier.dense, cls_w / cls_b = classifier.out_proj.  d_cls_rows are
 *                   bit-identical to mq_encode_bert(pool = CLS, normalize = 0).  Same refusals and scratch as mq_score_pairs_bert. */
typedef struct mq_score_head_weights {
    const void*  pooler_w;   /* bf16 [W, W]: bert.pooler.dense.weight (RoBERTa heads: classifier.dense.weight) */
    const float* pooler_b;   /* fp32 [W] */
    const float* cls_w;      /* fp32 [W]: classifier.weight (num_labels = 1; RoBERTa heads: classifier.out_proj.weight) */
    float        cls_b;      /* classifier.bias (classifier.out_proj.bias) */
    int32_t      type_vocab; /* rows of mq_bert_weights.type_emb (config.json type_vocab_size) */
} mq_score_head_weights;

int mq_pair_plan(int32_t Lq, const int32_t* d_doc_len, int64_t n, int32_t ld, int32_t max_length, int32_t* d_keep_a, int32_t* d_keep_b,
                 int32_t* d_total, void* stream);
int mq_pair_plan_n(int32_t Lq, const int32_t* d_doc_len, int64_t n, int32_t ld, int32_t max_length, int32_t specials, int32_t* d_keep_a,
                   int32_t* d_keep_b, int32_t* d_total, void* stream);
int mq_pack_pairs(const int32_t* d_query, int32_t Lq, const int32_t* d_docs, int32_t ld, const int32_t* d_keep_a, const int32_t* d_keep_b,
                  const int32_t* d_cu, int64_t n, int32_t cls_id, int32_t sep_id, int32_t* d_ids, int32_t* d_type_ids, int64_t rows,
                  void* stream);
int mq_pack_pairs_xlmr(const int32_t* d_query, int32_t Lq, const int32_t* d_docs, int32_t ld, const int32_t* d_keep_a, const int32_t* d_keep_b,
                       const int32_t* d_cu, int64_t n, int32_t cls_id, int32_t sep_id, int32_t* d_ids, int64_t rows, void* stream);
int mq_embed_tokens_typed(const int32_t* d_ids, const int32_t* d_type_ids, const int32_t* d_cu, int64_t nseq, const float* d_tok,
                          const float* d_pos, const float* d_type_emb, int32_t type_vocab, const float* d_g, const float* d_b, float* d_x,
                          void* d_xb, int32_t W, int32_t vocab, float eps, int32_t last_pos, void* stream);
size_t mq_score_head_workspace_bytes(int64_t n, int32_t W);
int mq_score_head(const float* d_h, int64_t n, int32_t W, const mq_score_head_weights* head, float* d_logits, float* d_scores,
                  void* d_workspace, size_t workspace_bytes, void* stream);
size_t mq_score_pairs_workspace_bytes(const mq_bert_cfg* cfg, int64_t rows, int64_t nseq);
int mq_score_pairs_bert(const mq_bert_cfg* cfg, const mq_bert_weights* w, const mq_score_head_weights* head, const int32_t* d_ids,
                        const int32_t* d_type_ids, const int32_t* d_cu_seqlens, const int32_t* h_cu_seqlens, int64_t nseq, float* d_logits,
                        float* d_scores, float* d_cls_rows, void* d_workspace, size_t workspace_bytes, void* stream);
int mq_score_pairs_xlmr(const mq_bert_cfg* cfg, const mq_bert_weights* w, const mq_score_head_weights* head, const int32_t* d_ids,
                        const int32_t* d_cu_seqlens, const int32_t* h_cu_seqlens, int64_t nseq, float* d_logits, float* d_scores,
                        float* d_cls_rows, void* d_workspace, size_t workspace_bytes, void* stream);

/* ---- image reranking: the OWL-ViT detection heads (csrc/owl_head.hip; engine/owl.py) ----------------------------------------------------------
 * s2_inference/reranking/rerank.py rerank_search_results -> cross_encoders.py ReRankerOwl -> transformers' OwlViTForObjectDetection in the
 * reference.  The image encoder is the CLIP ViT of the towers (all T rows of every image kept); these entry points are what follows it, as
 * modeling_owlvit.py computes it (image_text_embedder, OwlViTClassPredictionHead, OwlViTBoxPredictionHead, box_predictor); the W x W linears in
 * between are mq_gemm_bf16 calls.  Additions to ABI 14: nothing above changes.  P = T - 1 patches per image, P <= 8191; no scratch is needed.
 *
 *   mq_owl_merge_ln:   d_x fp32 [n T, W], class token in row 0 of every image.  c = LayerNorm(x_0; post_g, post_b), p_j = LayerNorm(x_j; post_g,
 *                      post_b), feats[img P + j - 1] = LayerNorm(p_j * c; ln_g, ln_b) for j = 1 .. T - 1, written as bf16 (d_feats_bf16) and / or
 *                      fp32 (d_feats_f32) [n P, W]; one eps for the three.  W % 4 == 0, W <= 2048, T >= 2.
 *   mq_owl_class_head: d_embeds fp32 [n P, Dq] = class_head.dense0(feats); d_queries fp32 [Q, Dq] shared by every image (per_image == 0) or
 *                      [n, Q, Dq] (per_image != 0) = the model's query_embeds; d_query_mask int32 of the same leading shape (NULL: all valid).
 *                      Per row: z_q = (e / (|e| + 1e-6)) . (t_q / (|t_q| + 1e-6)); shift = feats . shift_w + shift_b; scale = ELU(feats . scale_w +
 *                      scale_b) + 1; logit_q = (z_q + shift) scale, -FLT_MAX where the mask is 0.  d_logits fp32 [n P] = max_q, d_labels int32 =
 *                      the first q that attains it, d_scores = 1 / (1 + exp(-max)).  1 <= Q <= 8.
 *   mq_owl_box_head:   d_hidden bf16 [n P, W] = gelu(box_head.dense1(gelu(box_head.dense0(feats)))), the GELU epilogue's output; d_w2 fp32 [4, W], d_b2 fp32 [4] = dense2;
 *                      d_box_bias fp32 [P, 4] = compute_box_bias of the grid.  (cx, cy, w, h) = sigmoid(hidden w2^T + b2 + box_bias[patch]) ->
 *                      d_boxes fp32 [n P, 4] = (cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2) x (target_w, target_h, target_w, target_h);
 *                      d_boxes 16-byte aligned.
 *   mq_owl_topk:       per image the k highest of d_scores fp32 [n, P] in descending order, ties to the lower patch, NaN last: d_top_scores fp32
 *                      [n, k], d_top_boxes fp32 [n, k, 4] (rows of d_boxes [n, P, 4]; both 16-byte aligned), d_top_patch int32 [n, k].
 *                      1 <= k <= P (callers clamp k = min(num_highlights, P)).  One workgroup per image. */
int mq_owl_merge_ln(const float* d_x, const float* d_post_g, const float* d_post_b, const float* d_ln_g, const float* d_ln_b, void* d_feats_bf16,
                    float* d_feats_f32, int64_t n, int32_t T, int32_t W, float eps, void* stream);
int mq_owl_class_head(const float* d_embeds, const float* d_feats, const float* d_queries, const int32_t* d_query_mask, int32_t per_image,
                      const float* d_shift_w, float shift_b, const float* d_scale_w, float scale_b, float* d_scores, float* d_logits,
                      int32_t* d_labels, int64_t n, int32_t P, int32_t W, int32_t Dq, int32_t Q, void* stream);
int mq_owl_box_head(const void* d_hidden, const float* d_w2, const float* d_b2, const float* d_box_bias, float* d_boxes, int64_t n, int32_t P,
                    int32_t W, float target_w, float target_h, void* stream);
int mq_owl_topk(const float* d_scores, const float* d_boxes, int64_t n, int32_t P, int32_t k, float* d_top_scores, float* d_top_boxes,
                int32_t* d_top_patch, void* stream);

/* ---- LanguageBind video tower: the temporal sub-block and the clip-layout front end (csrc/temporal.hip; engine/languagebind.py) ---------------
 * s2_inference/languagebind/video/modeling_video.py:209-231 in the reference: in front of every CLIP block, a per-frame temporal embedding is
 * added into the residual stream, a temporal LayerNorm follows, a second attention attends ACROSS the T frames at each spatial token, and a residual
 * add closes the sub-block.  The activation keeps the frame-major order of the spatial blocks throughout: row r = (b T + t) N + n (clip b, frame t,
 * token n); the reference's `(b t) n d <-> (b n) t d` transposes are never materialised.  The QKV / out-projection GEMMs are mq_gemm_bf16 calls.
 * Additions to ABI 14: nothing above changes.  No scratch is needed.
 *
 *   mq_temporal_embed_ln:  d_x fp32 [B T N, W], in place: x[r, :] += d_temb[t, :] (d_temb fp32 [T, W]; one fp32 add per element; skipped when
 *                          T == 1, as the reference skips it), then d_out_bf16 [B T N, W] = LayerNorm(x[r]; g, b) of the updated row.  One pass over
 *                          the row.  W % 4 == 0, W <= 2048.
 *   mq_temporal_attention: d_qkv bf16 [B T N, 3W] in mq_attention's column layout (q | k | v, head h owns columns 64 h .. 64 h + 63 of each third),
 *                          d_out bf16 [B T N, W] in the same row order.  For every (b, n, head): out = softmax(q k^T / 8) v, unmasked, over the T
 *                          rows {(b T + t) N + n}.  Scores, softmax and the P V sums are fp32 (the probabilities are not rounded); every q / k / v
 *                          element is read once.  W == 64 heads and 1 <= T <= 16, anything else is MQ_ERR_INVALID and launches nothing.  Both
 *                          pointers 16-byte aligned.
 *   mq_patchify_clip:      d_in fp32 [B, 3, T, S, S] (the `pixel_values` layout `b c t h w`) -> d_out bf16 [B T (S/P)^2, Kp]: the rows mq_patchify
 *                          (is_u8 == 0) writes for the B T frames in (b t) order, bit for bit.  Kp % 8 == 0, Kp >= 3 P^2. */
int mq_temporal_embed_ln(float* d_x, const float* d_temb, const float* d_g, const float* d_b, void* d_out_bf16, int64_t B, int32_t T, int32_t N,
                         int32_t W, float eps, void* stream);
int mq_temporal_attention(const void* d_qkv, void* d_out, int64_t B, int32_t T, int32_t N, int32_t W, int32_t heads, void* stream);
int mq_patchify_clip(const float* d_in, void* d_out, int64_t B, int32_t T, int32_t S, int32_t P, int32_t Kp, void* stream);

/* ---- LanguageBind audio part: Kaldi fbank, the three-crop picture, im2col rows of a non-square picture (csrc/audio.hip; engine/audio.py,
 * engine/languagebind.py) -----------------------------------------------------------------------------------------------------------------------
 * s2_inference/languagebind/audio/processing_audio.py in the reference: torchaudio.compliance.kaldi.fbank (sample_frequency 16000, frame_length 25,
 * frame_shift 10, window_type "hanning", dither 0, use_energy False, htk_compat True, everything else at torchaudio's default), three crops of the
 * log-mel rows stacked into a [3, num_mel_bins, target_length] picture, (x - audio_mean) / (2 audio_std); modeling_audio.py:767-811: a CLIP ViT
 * over image_size = [num_mel_bins, target_length].  Additions to ABI 14: nothing above changes.  Every entry point judges its arguments before any
 * launch (MQ_ERR_INVALID, the message names the entry point and the bad value), runs on `stream` and allocates nothing.
 *
 *   mq_fbank:         d_wave fp32 [n_mean] -> d_mel fp32 [m, bins], m = 1 + (n - 400) / 160 (integer division; the samples behind the last whole
 *                     frame are dropped).  The mean of all n_mean samples is subtracted first (the reference's `audio_data -= audio_data.mean()`
 *                     over the whole tensor), and frames are cut from the first n of them: for a [channels, n] waveform n_mean = channels n and
 *                     channel 0 is framed, as Kaldi does; for a 1-D one n_mean = n.  Per frame: subtract the frame's mean; x[i] -= 0.97 x[i - 1]
 *                     with x[-1] := x[0]; times the symmetric Hann window 0.5 - 0.5 cos(2 pi i / 399); zero-padded to 512; power spectrum of bins
 *                     0..255 (the Nyquist bin carries no weight); `bins` triangular filters, linear in mel(f) = 1127 ln(1 + f / 700) from 20 Hz to
 *                     8 kHz; log(max(e, FLT_EPSILON)).  fp32 in and out, fp64 between (the FFT and the filter sums included).  d_ws:
 *                     MQ_FBANK_WS_BYTES of device scratch, 8-byte aligned (the partial sums of the mean).  Served: sample_rate == 16000,
 *                     1 <= bins <= 128, n >= 400; anything else is refused.
 *   mq_mel_fusion:    d_mel fp32 [m, bins] -> d_px fp32 [3, bins, L]: px[c, f, t] = (mel[(start_c + t) mod m, f] - mean) / (2 std), the division
 *                     IEEE.  start 0, 0, 0 on m <= L rows is the reference's mel.repeat(...)[:L]; three starts with start + L <= m are its three
 *                     crops.  0 <= start_c < m, std > 0, 1 <= bins <= 128.
 *   mq_patchify_rect: d_in fp32 [n, 3, H, Wd] -> d_out bf16 [n (H/P)(Wd/P), Kp], rows in (img, py, px) order, columns as mq_patchify writes them
 *                     (c P^2 + ky P + kx, zero from 3 P^2 on); for H == Wd bit for bit what mq_patchify (is_u8 == 0) writes.  H % P == 0,
 *                     Wd % P == 0, Kp % 8 == 0, Kp >= 3 P^2, d_out 16-byte aligned. */
#define MQ_FBANK_WS_BYTES 2048
int mq_fbank(const float* d_wave, int64_t n, int64_t n_mean, int32_t sample_rate, int32_t bins, float* d_mel, void* d_ws, void* stream);
int mq_mel_fusion(const float* d_mel, int64_t m, int32_t bins, int64_t start0, int64_t start1, int64_t start2, float mean, float std, float* d_px,
                  int32_t L, void* stream);
int mq_patchify_rect(const float* d_in, void* d_out, int64_t n, int32_t H, int32_t Wd, int32_t P, int32_t Kp, void* stream);

/* ---- LanguageBind front ends for media as a decoder hands it over: raw video frames and any-rate audio (csrc/video.hip, csrc/audio.hip;
 * engine/video.py, engine/audio.py) -------------------------------------------------------------------------------------------------------------
 * s2_inference/languagebind/video/processing_video.py:20-93 in the reference: np.linspace frame pick, x / 255, NormalizeVideo, pytorchvideo's
 * ShortSideScale, torchvision's CenterCropVideo, a horizontal flip; audio/processing_audio.py:47-49: torchaudio.functional.resample at its defaults.
 * Additions to ABI 14: nothing above changes.  Both entry points judge their arguments before any launch (MQ_ERR_INVALID, the message names the entry
 * point and the bad value), run on `stream` and allocate nothing.  Nothing here decodes a file.
 *
 *   mq_video_preprocess: d_frames uint8 [T_in, H, W, 3] (decoded frames, RGB last) -> d_out fp32 [3, T, S, S], one clip of the `b c t h w` tensor
 *                        mq_patchify_clip reads.  Output frame t is source frame d_pick[t] (int32 [T] on the device; a value outside [0, T_in) is
 *                        clamped into it).  out[c, t, y, x] is pixel (top + y, left + x') of that frame scaled to new_h x new_w, x' = x, or S - 1 - x
 *                        with flip == 1: the bilinear taps of torch.nn.functional.interpolate(size = (new_h, new_w), mode = "bilinear",
 *                        align_corners = False), no antialiasing — source coordinate (dst + 0.5) (in / out) - 0.5 clamped at 0, upper neighbour
 *                        clamped at in - 1 —, each tap first (u8 / 255 - h_mean[c]) / h_std[c] with both divisions IEEE, blended along x, then
 *                        along y.  Coordinates are fp64, taps and blend fp32; with new_h == H and new_w == W the output is the normalised input bit
 *                        for bit.  h_mean, h_std: HOST float[3], std > 0.  The integers new_h, new_w, top, left are the caller's
 *                        (engine/video.py states the reference's rules).  Served: 1 <= H, W <= 16384, 1 <= T_in < 2^31, 1 <= T <= 4096,
 *                        1 <= S <= 4096, S <= new_h, new_w <= 16384, 0 <= top <= new_h - S, 0 <= left <= new_w - S.
 *   mq_resample:         d_wave fp32 [channels, len] -> d_out fp32 [channels, ceil(n len / o)], every channel on its own.  o = orig / gcd,
 *                        n = new / gcd (coprime, o != n).  d_taps fp64 [n, K = 2 width + o] on the device, 8-byte aligned: the polyphase table of
 *                        the windowed-sinc filter (engine/audio.py builds it in fp64).  With x_pad = `width` zeros, the channel, zeros:
 *                        out[f n + p] = sum_k taps[p][k] x_pad[f o + k], summed in fp64 in ascending k, stored as fp32.  Served: K <= 12288,
 *                        n K <= MQ_RESAMPLE_MAX_TAPS, 1 <= channels <= 65535, 1 <= len < 2^36. */
#define MQ_RESAMPLE_MAX_TAPS (1 << 21)
int mq_video_preprocess(const uint8_t* d_frames, int64_t T_in, int32_t H, int32_t W, const int32_t* d_pick, int32_t T, int32_t S, int32_t new_h,
                        int32_t new_w, int32_t top, int32_t left, const float* h_mean, const float* h_std, int32_t flip, float* d_out, void* stream);
int mq_resample(const float* d_wave, int64_t channels, int64_t len, const double* d_taps, int32_t o, int32_t n, int32_t width, float* d_out,
                void* stream);

/* ---- ModernBERT text encoders: sliding-window attention and the tower (csrc/attention_window.hip, csrc/modernbert.hip; engine/modernbert.py) ------
 * transformers' ModernBertModel (model_type "modernbert": gte-modernbert-base, modernbert-embed-base, granite-embedding-*-r2 ...): pre-LN blocks
 * without any bias, rotary positions, a gated-GELU MLP, and two layers in three attending only a band of keys.
 * Additions to ABI 15: nothing above changes; the structs below are new.  Every entry point judges its arguments before any launch
 * (MQ_ERR_INVALID, the message names the entry point and the bad value), runs on `stream` and allocates nothing.
 *
 *   mq_attention_window: mq_attention (bf16, 64-wide heads, no causal mask, no bias; packed or fixed-length sequences up to 8192 rows) where query i
 *                   attends the keys j of its own sequence with |i - j| <= half_window — inclusive on both sides, as transformers' ModernBERT
 *                   builds its sliding mask with half_window = local_attention / 2.  A band kernel: one workgroup per (sequence, head, 64-query slice)
 *                   stages only the 64-key tiles the slice can reach, and a 16-query block visits only the tiles that cut its band (masked per key at the
 *                   band's edges, unmasked inside).  half_window >= 0; half_window >= max_len - 1 is full attention and runs mq_attention's kernel.
 *   mq_encode_modernbert: token embedding -> LayerNorm -> `layers` blocks  x += Wo(attn(rope(Wqkv(attn_norm(x))))) ; x += mlp.Wo(gelu(input) * gate) with
 *                   (input | gate) = mlp.Wi(mlp_norm(x))  -> final_norm over all rows -> mean / CLS pooling (+ L2), on packed sequences like
 *                   mq_encode_bert.  fp32 residual stream, bf16 GEMM operands.  Layer 0 has no attn_norm (attn_norm_g NULL: the embedding
 *                   LayerNorm's output feeds Wqkv and is the residual).  A layer with sliding != 0 rotates with d_inv_freq_local and runs
 *                   mq_attention_window(half_window); the others rotate with d_inv_freq_global and run mq_attention.  d_out fp32 [nseq, width]. */
typedef struct mq_modernbert_layer {
    const float* attn_norm_g;   /* fp32 [W], NULL: no LayerNorm in front of Wqkv (layer 0) */
    const void*  qkv_w;         /* bf16 [3W, W]  attn.Wqkv, rows q | k | v */
    const void*  out_w;         /* bf16 [W, W]   attn.Wo */
    const float* mlp_norm_g;    /* fp32 [W] */
    const void*  wi_w;          /* bf16 [2F, W]  mlp.Wi with its halves SWAPPED to mq_glu's (up | gate) order: rows 0 .. F-1 = the checkpoint's `gate`
                                 * half (rows F .. 2F-1 of mlp.Wi, the plain multiplier), rows F .. 2F-1 = its `input` half (the one GELU is applied to) */
    const void*  wo_w;          /* bf16 [W, F]   mlp.Wo */
    int32_t      sliding;       /* 0: full attention, global rotary base; 1: band of half_window, local rotary base */
    int32_t      reserved;
} mq_modernbert_layer;

typedef struct mq_modernbert_weights {
    const float* tok_emb;       /* fp32 [vocab, W] */
    const float* emb_ln_g;      /* fp32 [W] */
    const float* final_ln_g;    /* fp32 [W] */
    const float* zeros;         /* fp32 [W] of zeros: the bias of the bias-free LayerNorms and residual GEMMs */
    const float* d_inv_freq_global; /* fp32 [32]: theta_global ^ -(2 i / 64) */
    const float* d_inv_freq_local;  /* fp32 [32]: theta_local ^ -(2 i / 64) */
    const mq_modernbert_layer* layers;  /* host array, `layers` entries */
} mq_modernbert_weights;

typedef struct mq_modernbert_cfg {
    int32_t width;       /* W = heads * 64 */
    int32_t layers;
    int32_t heads;
    int32_t mlp_dim;     /* F, multiple of 64 */
    int32_t vocab;
    int32_t max_pos;     /* longest sequence served (<= 8192) */
    int32_t half_window; /* local_attention / 2 */
    int32_t pool;        /* MQ_POOL_* */
    float   ln_eps;
    int32_t reserved;
} mq_modernbert_cfg;

int mq_attention_window(const void* d_qkv, void* d_out, const int32_t* d_cu_seqlens, int64_t nseq, int32_t fixed_len, int32_t max_len, int32_t W,
                        int32_t heads, int32_t half_window, void* stream);
size_t mq_modernbert_workspace_bytes(const mq_modernbert_cfg* cfg, int64_t rows, int64_t nseq);
int mq_encode_modernbert(const mq_modernbert_cfg* cfg, const mq_modernbert_weights* w, const int32_t* d_ids, const int32_t* d_cu_seqlens,
                         const int32_t* h_cu_seqlens, int64_t nseq, float* d_out, int normalize, void* d_workspace, size_t workspace_bytes, void* stream);

/* ---- text reranking on the ModernBERT tower (csrc/rerank.hip; engine/rerank.py ModernBertCrossEncoderTower) --------------------------------
 * transformers' ModernBertForSequenceClassification with num_labels = 1 (gte-reranker-modernbert-base, reranker-ModernBERT-*-gooaq-bce, the
 * cross-encoder/ms-marco-ModernBERT-* shape): the encoder of mq_encode_modernbert, mean or CLS pooling of the final-normed rows, and a head that is
 * NOT mq_score_head's: dense -> erf GELU -> LayerNorm -> one-logit classifier (dropout does nothing at inference).  Pairs are planned and packed by
 * mq_pair_plan_n / mq_pack_pairs with specials = 3 ([CLS] q [SEP] d [SEP]; the type ids mq_pack_pairs writes are not read).  Additions to ABI 15:
 * nothing above changes.  Both entry
 * points judge their arguments before any launch (MQ_ERR_INVALID, the message names the entry point and the bad value), run on `stream` and
 * allocate nothing.
 *
 *   mq_score_head_ln: d_h fp32 [n, W] (the pooled rows) -> a = gelu(dense_w bf16(h) + dense_b) (mq_gemm_bf16: bf16 operands, fp32 accumulation and
 *                   output, the erf GELU of MQ_EPI_GELU in its epilogue; a head without dense_b adds a bias of zeros from the scratch), then one
 *                   wave64 per pair: mu and rstd = rsqrt(mean((a - mu)^2) + ln_eps) in two passes over the row held in registers, and
 *                   z = sum_j ((a_j - mu) rstd norm_g[j] + norm_b[j]) cls_w[j] + cls_b -> d_logits fp32 [n]; d_scores (NULL ok) = 1 / (1 + exp(-z)).
 *                   The normalised row is never written.  W % 64 == 0, W <= 2048, n >= 1.  Scratch: mq_score_head_ln_workspace_bytes(n, W).
 *   mq_score_pairs_modernbert: mq_encode_modernbert(cfg, w, ..., normalize = 0) into a scratch slot (d_pooled fp32 [nseq, W], NULL ok, receives a
 *                   copy: bit-identical to that entry point on the same ids, because it IS that entry point) -> mq_score_head_ln.  The encoder's
 *                   refusals (cfg, weights, sequence lengths) are mq_encode_modernbert's.  Scratch:
 *                   mq_score_pairs_modernbert_workspace_bytes(cfg, rows, nseq). */
typedef struct mq_score_head_ln_weights {
    const void*  dense_w;    /* bf16 [W, W]: head.dense.weight */
    const float* dense_b;    /* fp32 [W]: head.dense.bias, NULL when the config has classifier_bias = false */
    const float* norm_g;     /* fp32 [W]: head.norm.weight */
    const float* norm_b;     /* fp32 [W]: head.norm.bias, NULL when the config has norm_bias = false */
    const float* cls_w;      /* fp32 [W]: classifier.weight (num_labels = 1) */
    float        cls_b;      /* classifier.bias */
    float        ln_eps;     /* norm_eps */
} mq_score_head_ln_weights;

size_t mq_score_head_ln_workspace_bytes(int64_t n, int32_t W);
int mq_score_head_ln(const float* d_h, int64_t n, int32_t W, const mq_score_head_ln_weights* head, float* d_logits, float* d_scores,
                     void* d_workspace, size_t workspace_bytes, void* stream);
size_t mq_score_pairs_modernbert_workspace_bytes(const mq_modernbert_cfg* cfg, int64_t rows, int64_t nseq);
int mq_score_pairs_modernbert(const mq_modernbert_cfg* cfg, const mq_modernbert_weights* w, const mq_score_head_ln_weights* head,
                              const int32_t* d_ids, const int32_t* d_cu_seqlens, const int32_t* h_cu_seqlens, int64_t nseq, float* d_logits,
                              float* d_scores, float* d_pooled, void* d_workspace, size_t workspace_bytes, void* stream);

/* ---- Qwen3 / Qwen2 text embedders: grouped-query causal attention and the tower (csrc/attention_gqa.hip, csrc/qwen.hip; engine/qwen.py) --------------
 * transformers' Qwen3Model / Qwen2Model (model_type "qwen3" / "qwen2": Qwen3-Embedding-0.6B, gte-Qwen2-1.5B-instruct, Qwen2-0.5B fine-tunes): pre-norm
 * decoder blocks with RMSNorm, fewer K/V heads than query heads, rotary positions, a gated-SiLU MLP, a causal mask and last-token (or mean) pooling.
 * Additions to ABI 15: nothing above changes; the selector, structs and entry points below are new.  Every entry point judges its arguments before any
 * launch (MQ_ERR_INVALID, the message names the entry point and the bad value), runs on `stream` and allocates nothing.
 *
 *   mq_attention_gqa: d_qkv bf16 [rows, (q_heads + 2 kv_heads) head_dim] = (q | k | v), head h of each part at columns h head_dim ..; d_out bf16
 *                   [rows, q_heads head_dim].  q_heads % kv_heads == 0; query head h reads K/V head h / (q_heads / kv_heads) (transformers' repeat_kv).
 *                   head_dim 64 or 128, softmax scale 1/sqrt(head_dim); mask MQ_MASK_NONE or MQ_MASK_CAUSAL; sequences packed or fixed-length as for
 *                   mq_attention, max_len <= 8192.  One workgroup per (sequence, K/V head, 128-query slice) stages that head's K and V once for every
 *                   query head that reads it; under the causal mask a slice stages, and a 16-query block visits, only the keys it can see.
 *   mq_rmsnorm:     y = x * rsqrt(mean(x^2) + eps) * g over the last dim, fp32 statistics; x fp32 [rows, W] gathered through an optional row index as
 *                   for mq_layernorm; writes bf16 and / or fp32 (d_out_f32 may be d_x when there is no row index).  W % 4 == 0, W <= 2048.
 *   mq_qk_norm_rope: in place on the q and k parts of the layout above (V is not touched): per head, RMSNorm over head_dim with d_q_g / d_k_g (fp32
 *                   [head_dim]; both NULL: no norm), then rotary positions in rotate_half form, angle = float(t) * d_inv_freq[i] with t the row's position
 *                   in its sequence, exactly as mq_rope forms it.  fp32 from the bf16 input to the one rounding of the bf16 output.  head_dim 64, 128 or 256.
 *   mq_encode_qwen: token gather -> `layers` blocks  x += Wo(attn(qk_norm_rope(Wqkv(rmsnorm(x))))) ; x += Wdown(up * silu(gate)) with
 *                   (up | gate) = Wug(rmsnorm(x))  -> final RMSNorm -> pooling (+ L2), on packed sequences like mq_encode_bert; fp32 residual stream,
 *                   bf16 GEMM operands.  MQ_POOL_LAST: the last row of every sequence, normalised alone; MQ_POOL_MEAN: every row is normalised, then
 *                   mq_pool.  width <= 2048 (a multiple of 64), head_dim 64 or 128, mlp_dim % 64 == 0, max_pos <= 8192.  d_out fp32 [nseq, width]. */
#define MQ_POOL_LAST 2 /* mq_encode_qwen only: the last token of every sequence (mq_pool itself takes MQ_POOL_MEAN / MQ_POOL_CLS) */

typedef struct mq_qwen_layer {
    const float* input_norm_g;  /* fp32 [W]  input_layernorm */
    const void*  qkv_w;         /* bf16 [(Q + 2 KV) hd, W]  rows: q_proj | k_proj | v_proj */
    const float* qkv_b;         /* fp32 [(Q + 2 KV) hd] (Qwen2) or NULL (Qwen3) */
    const float* q_norm_g;      /* fp32 [hd] (Qwen3) or NULL */
    const float* k_norm_g;      /* fp32 [hd] (Qwen3) or NULL */
    const void*  out_w;         /* bf16 [W, Q hd]  o_proj */
    const float* post_norm_g;   /* fp32 [W]  post_attention_layernorm */
    const void*  ug_w;          /* bf16 [2F, W]  rows: up_proj | gate_proj (mq_glu's order) */
    const void*  down_w;        /* bf16 [W, F]  down_proj */
} mq_qwen_layer;

typedef struct mq_qwen_weights {
    const float* tok_emb;       /* fp32 [vocab, W] */
    const float* final_norm_g;  /* fp32 [W] */
    const float* zeros;         /* fp32 [W] of zeros: the bias of the residual GEMMs */
    const float* d_inv_freq;    /* fp32 [hd / 2]: rope_theta ^ -(2 i / hd) */
    const mq_qwen_layer* layers;  /* host array, `layers` entries */
} mq_qwen_weights;

typedef struct mq_qwen_cfg {
    int32_t width;       /* W, multiple of 64, <= 2048 */
    int32_t layers;
    int32_t q_heads;     /* Q */
    int32_t kv_heads;    /* KV, divides Q */
    int32_t head_dim;    /* hd: 64 or 128; Q hd need not be W */
    int32_t mlp_dim;     /* F, multiple of 64 */
    int32_t vocab;
    int32_t max_pos;     /* longest sequence served (<= 8192) */
    int32_t pool;        /* MQ_POOL_LAST or MQ_POOL_MEAN */
    float   rms_eps;
} mq_qwen_cfg;

int mq_attention_gqa(const void* d_qkv, void* d_out, const int32_t* d_cu_seqlens, int64_t nseq, int32_t fixed_len, int32_t max_len, int32_t q_heads,
                     int32_t kv_heads, int32_t head_dim, int32_t mask, void* stream);
int mq_rmsnorm(const float* d_x, const int32_t* d_row_idx, const float* d_g, void* d_out_bf16, float* d_out_f32, int64_t rows, int32_t W, float eps,
               void* stream);
int mq_qk_norm_rope(void* d_qkv, const int32_t* d_cu, int64_t nseq, int32_t fixed_len, int32_t q_heads, int32_t kv_heads, int32_t head_dim,
                    const float* d_q_g, const float* d_k_g, float eps, const float* d_inv_freq, void* stream);
size_t mq_qwen_workspace_bytes(const mq_qwen_cfg* cfg, int64_t rows, int64_t nseq);
int mq_encode_qwen(const mq_qwen_cfg* cfg, const mq_qwen_weights* w, const int32_t* d_ids, const int32_t* d_cu_seqlens, const int32_t* h_cu_seqlens,
                   int64_t nseq, float* d_out, int normalize, void* d_workspace, size_t workspace_bytes, void* stream);

/* ---- Qwen3 rerankers: prefix-sharing causal attention and the pair-scoring tower (csrc/attention_gqa.hip, csrc/qwen.hip, csrc/rerank.hip;
 * engine/rerank.py QwenRerankerTower) -------------------------------------------------------------------------------------------------------------------
 * transformers' Qwen3ForCausalLM used as a yes / no judge (Qwen/Qwen3-Reranker-0.6B) or Qwen3ForSequenceClassification with one label: one query against
 * n documents.  Under the causal mask everything in front of the document (system prompt, instruction, query) is the same for every hit, so it is
 * computed once: P + sum(d_i) rows instead of n P + sum(d_i).  Additions to ABI 15: nothing above changes; the entry points below are new.  Each judges
 * its arguments before any launch, runs on `stream` and allocates nothing.
 *
 *   mq_attention_gqa_prefix: mq_attention_gqa's layout.  Rows [0, prefix_len) of d_qkv are the shared prefix, the nseq segments follow: d_cu_seqlens
 *                   int32 [nseq + 1] with d_cu_seqlens[0] = prefix_len, max_len = the longest SEGMENT, prefix_len + max_len <= 8192.  The query at local
 *                   position t of a segment sees the prefix_len prefix keys and its own segment's keys 0 .. t, nothing of other segments.  Only the
 *                   segments' rows of d_out are written (the prefix rows' own attention is mq_attention_gqa on one fixed-length causal sequence).
 *                   prefix_len need not be a multiple of 64.  With prefix_len = 0 the result is bit-identical to mq_attention_gqa with MQ_MASK_CAUSAL.
 *   mq_qk_norm_rope_at: mq_qk_norm_rope with a position offset in [0, 8192]: row t of a sequence rotates at position offset + t.  offset 0 is
 *                   bit-identical to mq_qk_norm_rope.
 *   mq_score_dot:   d_logits[i] = d_h[i] . d_w  (fp32 [n, W] rows, one fp32 [W] row, fp32 accumulation), d_scores (may be NULL) = sigmoid.  W <= 2048.
 *   mq_score_qwen_pairs: mq_encode_qwen's tower over packed rows [prefix | seg_1 | ... | seg_n].  The prefix is sequence 0 of the batch:
 *                   d_cu_seqlens / h_cu_seqlens int32 [nseq + 2] = {0, prefix_len, prefix_len + d_1, ...}; prefix_len may be 0 (every segment is then a
 *                   whole sequence: the unshared path).  The rotary step runs on the prefix at offset 0 and on the segments at offset prefix_len;
 *                   attention is mq_attention_gqa (causal) on the prefix and mq_attention_gqa_prefix on the segments; the final RMSNorm runs on every
 *                   segment's last row only; d_logits fp32 [nseq] = that row . d_score_w (fp32 [width]), d_scores (may be NULL) its sigmoid.
 *                   prefix_len + the longest segment <= cfg->max_pos.  cfg->pool is not read beyond mq_encode_qwen's check of it. */
int mq_attention_gqa_prefix(const void* d_qkv, void* d_out, const int32_t* d_cu_seqlens, int64_t nseq, int32_t prefix_len, int32_t max_len,
                            int32_t q_heads, int32_t kv_heads, int32_t head_dim, void* stream);
int mq_qk_norm_rope_at(void* d_qkv, const int32_t* d_cu, int64_t nseq, int32_t fixed_len, int32_t q_heads, int32_t kv_heads, int32_t head_dim,
                       const float* d_q_g, const float* d_k_g, float eps, const float* d_inv_freq, int32_t offset, void* stream);
int mq_score_dot(const float* d_h, const float* d_w, int64_t n, int32_t W, float* d_logits, float* d_scores, void* stream);
size_t mq_score_qwen_pairs_workspace_bytes(const mq_qwen_cfg* cfg, int64_t rows, int64_t nseq);
int mq_score_qwen_pairs(const mq_qwen_cfg* cfg, const mq_qwen_weights* w, const float* d_score_w, const int32_t* d_ids, const int32_t* d_cu_seqlens,
                        const int32_t* h_cu_seqlens, int64_t nseq, int32_t prefix_len, float* d_logits, float* d_scores, void* d_workspace,
                        size_t workspace_bytes, void* stream);

/* ---- EmbeddingGemma text embedders: 256-wide-head grouped-query band attention and the tower (csrc/attention_gqa256.hip, csrc/gemma.hip;
 * engine/gemma.py) ------------------------------------------------------------------------------------------------------------------------------------
 * transformers' Gemma3TextModel with use_bidirectional_attention (model_type "gemma3_text": google/embeddinggemma-300m and its fine-tunes): blocks with
 * four RMSNorms (one in front of and one behind each sub-layer), 256-wide heads with fewer K/V heads than query heads, per-head q / k RMSNorm, rotary
 * positions with one base per layer kind, a gated tanh-GELU MLP, no causal mask, and `sliding` layers that attend only the keys within half_window
 * positions.  Additions to ABI 15: nothing above changes but mq_qk_norm_rope, which now also takes head_dim 256; the structs and entry points below are
 * new.  Every entry point judges its arguments before any launch (MQ_ERR_INVALID, the message names the entry point and the bad value), runs on
 * `stream` and allocates nothing.
 *
 *   mq_attention_gqa_band: mq_attention_gqa's layout — d_qkv bf16 [rows, (q_heads + 2 kv_heads) head_dim] = (q | k | v), d_out bf16 [rows, q_heads
 *                   head_dim], query head h reads K/V head h / (q_heads / kv_heads), sequences packed or fixed-length, max_len <= 8192 — at head_dim 256,
 *                   unmasked and bidirectional.  half_window == 0: every key of the sequence; half_window = hw > 0: query i sees keys j with
 *                   |i - j| <= hw.  `scale` is the softmax scale (> 0; Gemma: query_pre_attn_scalar ** -0.5).  One workgroup of 8 waves per (sequence,
 *                   K/V head, 64-query slice) stages the 64-key tiles the slice's band reaches, two tiles (128 KiB of LDS) at a time, once per round
 *                   for every query head that reads them; a 16-query block visits only the tiles that cut its own band.  Compiler report (gfx950):
 *                   213 VGPRs, 68 SGPRs, no scratch, no static LDS.
 *   mq_rmsnorm_add_norm: d_x fp32 [rows, W] += rmsnorm(d_o bf16 [rows, W]; d_g_post), then — when d_g_next and d_h are given (together or not at all) —
 *                   d_h bf16 [rows, W] = rmsnorm(d_x; d_g_next).  fp32 statistics, mq_rmsnorm's order of operations.  W % 4 == 0, W <= 2048.
 *   mq_glu_tanh:    mq_glu's (up | gate) layout, in place: buf[:, :F] = up * gelu_tanh(gate), gelu_tanh(x) = x / (1 + exp(-2 sqrt(2 / pi) (x + 0.044715
 *                   x^3))) (transformers' gelu_pytorch_tanh; not the erf form of MQ_ACT_GELU).  F % 8 == 0.
 *   mq_encode_gemma: token gather * sqrt(width) -> `layers` blocks  x += norm(Wo(attn(qk_norm_rope(Wqkv(norm(x)))))) ; x += norm(Wdown(up *
 *                   gelu_tanh(gate))) with (up | gate) = Wug(norm(x))  -> final RMSNorm -> mq_pool (MQ_POOL_MEAN or MQ_POOL_CLS) (+ L2), on packed
 *                   sequences like mq_encode_bert; fp32 residual stream, bf16 GEMM operands.  Every norm weight is the checkpoint's 1 + w.  width <= 2048
 *                   (a multiple of 64), head_dim 256, mlp_dim % 64 == 0, max_pos <= 8192.  d_out fp32 [nseq, width]. */
typedef struct mq_gemma_layer {
    const float* input_norm_g;      /* fp32 [W]  1 + input_layernorm */
    const void*  qkv_w;             /* bf16 [(Q + 2 KV) hd, W]  rows: q_proj | k_proj | v_proj */
    const float* q_norm_g;          /* fp32 [hd]  1 + q_norm */
    const float* k_norm_g;          /* fp32 [hd]  1 + k_norm */
    const void*  out_w;             /* bf16 [W, Q hd]  o_proj */
    const float* post_attn_norm_g;  /* fp32 [W]  1 + post_attention_layernorm */
    const float* pre_ffn_norm_g;    /* fp32 [W]  1 + pre_feedforward_layernorm */
    const void*  ug_w;              /* bf16 [2F, W]  rows: up_proj | gate_proj (mq_glu's order) */
    const void*  down_w;            /* bf16 [W, F]  down_proj */
    const float* post_ffn_norm_g;   /* fp32 [W]  1 + post_feedforward_layernorm */
    int32_t sliding;                /* 1: sliding_attention (cfg.half_window, d_inv_freq_local); 0: full_attention (d_inv_freq_global) */
    int32_t reserved;
} mq_gemma_layer;

typedef struct mq_gemma_weights {
    const float* tok_emb;            /* fp32 [vocab, W] */
    const float* final_norm_g;       /* fp32 [W]  1 + norm */
    const float* d_inv_freq_global;  /* fp32 [hd / 2]: rope_theta ^ -(2 i / hd) */
    const float* d_inv_freq_local;   /* fp32 [hd / 2]: rope_local_base_freq ^ -(2 i / hd) */
    const mq_gemma_layer* layers;    /* host array, `layers` entries */
} mq_gemma_weights;

typedef struct mq_gemma_cfg {
    int32_t width;        /* W, multiple of 64, <= 2048 */
    int32_t layers;
    int32_t q_heads;      /* Q */
    int32_t kv_heads;     /* KV, divides Q */
    int32_t head_dim;     /* hd: 256; Q hd need not be W */
    int32_t mlp_dim;      /* F, multiple of 64 */
    int32_t vocab;
    int32_t max_pos;      /* longest sequence served (<= 8192) */
    int32_t half_window;  /* of the sliding layers: config sliding_window / 2 */
    int32_t pool;         /* MQ_POOL_MEAN or MQ_POOL_CLS */
    float   rms_eps;
    float   attn_scale;   /* query_pre_attn_scalar ^ -0.5 */
} mq_gemma_cfg;

int mq_attention_gqa_band(const void* d_qkv, void* d_out, const int32_t* d_cu_seqlens, int64_t nseq, int32_t fixed_len, int32_t max_len, int32_t q_heads,
                          int32_t kv_heads, int32_t head_dim, int32_t half_window, float scale, void* stream);
int mq_rmsnorm_add_norm(float* d_x, const void* d_o, const float* d_g_post, const float* d_g_next, void* d_h, int64_t rows, int32_t W, float eps,
                        void* stream);
int mq_glu_tanh(void* d_buf, int64_t rows, int32_t F, void* stream);
size_t mq_gemma_workspace_bytes(const mq_gemma_cfg* cfg, int64_t rows, int64_t nseq);
int mq_encode_gemma(const mq_gemma_cfg* cfg, const mq_gemma_weights* w, const int32_t* d_ids, const int32_t* d_cu_seqlens, const int32_t* h_cu_seqlens,
                    int64_t nseq, float* d_out, int normalize, void* d_workspace, size_t workspace_bytes, void* stream);

/* ---- T5 encoder text embedders: clamped relative-bias attention and the tower (csrc/attention_relbias.hip, csrc/t5.hip; engine/t5.py) -----------------
 * transformers' T5EncoderModel (model_type "t5": sentence-t5, gtr-t5, flan-t5 / T5 v1.1 encoder fine-tunes): pre-norm blocks with RMSNorms (T5LayerNorm),
 * bias-free Linears, an inner attention width heads * d_kv that need not be d_model, NO softmax scale, one relative-position bias table (block 0's)
 * shared by every block, a ReLU or a gated gelu_new MLP, no position table.  Additions to ABI 15: nothing above changes; the structs and entry points
 * below are new.  Every entry point judges its arguments before any launch (MQ_ERR_INVALID, the message names the entry point and the bad value), runs on
 * `stream` and allocates nothing.
 *
 *   mq_attention_relbias: d_qkv bf16 [rows, 3 inner] = (q | k | v), inner = heads head_dim, head h at columns h head_dim .. of each third; d_out bf16
 *                   [rows, inner]; head_dim 64 or 128; sequences packed or fixed-length as mq_attention, max_len <= 8192.  Unmasked, bidirectional:
 *                   scores[q, k] = scale (q . k) + d_rel_bias[h][clamp(k - q, -D, D) + D], D = max_distance in [1, 1024], d_rel_bias fp32 [heads][2 D + 1]
 *                   used as it is (nothing is pre-divided by the scale); scale > 0 is the caller's (T5: 1.0).  One workgroup of 4 waves per (sequence,
 *                   head, 64-query slice); the head's table lies in LDS behind the K / V image (576 keys at head_dim 64, 256 at 128; longer sequences
 *                   stream through in pieces).  Compiler report (gfx950): csrc/attention_relbias.hip's header.
 *   mq_encode_t5:   token gather -> `layers` blocks  x += Wo(attn(Wqkv(norm(x)))) ; x += Wo_ff(relu(Wi(norm(x))))  or, gated,  x += Wo_ff(up *
 *                   gelu_new(gate)) with (up | gate) = Wi'(norm(x))  -> final RMSNorm -> mq_pool (MQ_POOL_MEAN or MQ_POOL_CLS) (+ L2), on packed
 *                   sequences like mq_encode_bert; fp32 residual stream, bf16 GEMM operands.  width (d_model) a multiple of 64, <= 2048; head_dim (d_kv)
 *                   64 or 128; heads * head_dim <= 4096; mlp_dim (d_ff) % 64 == 0; max_pos <= 8192; max_distance in [1, 1024].  d_out fp32 [nseq, width]. */
typedef struct mq_t5_layer {
    const float* attn_norm_g;   /* fp32 [W]  layer.0.layer_norm */
    const void*  qkv_w;         /* bf16 [3 A, W]  rows: q | k | v, A = heads * head_dim */
    const void*  out_w;         /* bf16 [W, A]  SelfAttention.o */
    const float* ff_norm_g;     /* fp32 [W]  layer.1.layer_norm */
    const void*  wi_w;          /* bf16 [F, W] wi (relu), or [2F, W] rows: wi_1 | wi_0 = up | gate (mq_glu_tanh's order) */
    const void*  wo_w;          /* bf16 [W, F]  DenseReluDense.wo */
} mq_t5_layer;

typedef struct mq_t5_weights {
    const float* tok_emb;       /* fp32 [vocab, W]  shared.weight */
    const float* final_norm_g;  /* fp32 [W]  final_layer_norm */
    const float* zeros;         /* fp32 [max(W, F)] of zeros: the bias of the residual and ReLU GEMM epilogues */
    const float* d_rel_bias;    /* fp32 [heads][2 max_distance + 1]: block 0's relative_attention_bias by clamped key - query */
    const mq_t5_layer* layers;  /* host array, `layers` entries */
} mq_t5_weights;

typedef struct mq_t5_cfg {
    int32_t width;         /* W = d_model, multiple of 64, <= 2048 */
    int32_t layers;
    int32_t heads;
    int32_t head_dim;      /* d_kv: 64 or 128; heads * head_dim (<= 4096) need not be W */
    int32_t mlp_dim;       /* F = d_ff, multiple of 64 */
    int32_t vocab;
    int32_t max_pos;       /* longest sequence served (<= 8192) */
    int32_t pool;          /* MQ_POOL_MEAN or MQ_POOL_CLS */
    int32_t max_distance;  /* D = relative_attention_max_distance, 1 .. 1024 */
    int32_t gated;         /* 0: relu MLP; 1: gated gelu_new (T5 v1.1) */
    float   rms_eps;       /* layer_norm_epsilon */
    int32_t reserved;
} mq_t5_cfg;

int mq_attention_relbias(const void* d_qkv, void* d_out, const int32_t* d_cu_seqlens, int64_t nseq, int32_t fixed_len, int32_t max_len, int32_t heads,
                         int32_t head_dim, const float* d_rel_bias, int32_t max_distance, float scale, void* stream);
size_t mq_t5_workspace_bytes(const mq_t5_cfg* cfg, int64_t rows, int64_t nseq);
int mq_encode_t5(const mq_t5_cfg* cfg, const mq_t5_weights* w, const int32_t* d_ids, const int32_t* d_cu_seqlens, const int32_t* h_cu_seqlens,
                 int64_t nseq, float* d_out, int normalize, void* d_workspace, size_t workspace_bytes, void* stream);

/* ---- JinaBERT text embedders: ALiBi attention and the tower (csrc/attention_alibi.hip, csrc/jina_bert.hip; engine/jina_bert.py) ------------------------
 * jina-embeddings-v2-small-en / -base-en, their fine-tunes and MosaicBERT-style ALiBi encoders with the same block (config.json: model_type "bert" with
 * position_embedding_type "alibi"): post-LN blocks, Linears with biases, a bias-free gated erf-GELU MLP (GEGLU), no position table, a score bias of
 * -slope_h |key - query|.  The block semantics restate the published architecture; they are not pinned to a run of the original modelling code.
 * Additions to ABI 15: nothing above changes; the structs and entry points below are new.  Every entry point judges its arguments before any launch
 * (MQ_ERR_INVALID, the message names the entry point and the bad value), runs on `stream` and allocates nothing.
 *
 *   mq_attention_alibi: d_qkv bf16 [rows, 3 inner] = (q | k | v), inner = heads head_dim, head h at columns h head_dim .. of each third; d_out bf16
 *                   [rows, inner]; head_dim 64; sequences packed or fixed-length as mq_attention, max_len <= 8192.  Unmasked, bidirectional, every key
 *                   of the sequence contributes: scores[q, k] = fmaf(q . k, scale, -d_slopes[h] |k - q|) in fp32, d_slopes fp32 [heads] the caller's
 *                   (the kernel knows nothing about how slopes are derived); scale > 0 is the caller's.  One workgroup of 4 waves per (sequence, head,
 *                   64-query slice); the bias is formed in registers, the K / V image has the whole LDS (640 keys; longer sequences stream through in
 *                   pieces).  Compiler report (gfx950): csrc/attention_alibi.hip's header.
 *   mq_encode_jina_bert: token gather + type row 0 + LayerNorm -> `layers` blocks  x = LN(Wo(attn(Wqkv(x))) + x) ; x = LN(Wwo(up * gelu(gate)) + x) with
 *                   (up | gate) = Wg'(x)  -> mq_pool (MQ_POOL_MEAN or MQ_POOL_CLS) (+ L2), on packed sequences like mq_encode_bert; fp32 residual
 *                   stream, bf16 GEMM operands; softmax scale 1 / sqrt(head_dim).  width a multiple of 64, <= 2048; head_dim 64; heads * 64 == width;
 *                   mlp_dim % 64 == 0; max_pos <= 8192.  d_out fp32 [nseq, width]. */
typedef struct mq_jina_bert_layer {
    const void*  qkv_w;         /* bf16 [3 W, W]  rows: query | key | value */
    const float* qkv_b;         /* fp32 [3 W] */
    const void*  out_w;         /* bf16 [W, W]  attention.output.dense */
    const float* out_b;         /* fp32 [W] */
    const float* attn_ln_g;     /* fp32 [W]  attention.output.LayerNorm */
    const float* attn_ln_b;
    const void*  wg_w;          /* bf16 [2F, W]  rows: up | gate = mlp.gated_layers rows [F:] | [:F] (mq_glu's order), no bias */
    const void*  wo_w;          /* bf16 [W, F]  mlp.wo */
    const float* wo_b;          /* fp32 [W] */
    const float* mlp_ln_g;      /* fp32 [W]  mlp.layernorm */
    const float* mlp_ln_b;
} mq_jina_bert_layer;

typedef struct mq_jina_bert_weights {
    const float* tok_emb;       /* fp32 [vocab, W]  embeddings.word_embeddings */
    const float* type0;         /* fp32 [W]  row 0 of embeddings.token_type_embeddings */
    const float* emb_ln_g;      /* fp32 [W]  embeddings.LayerNorm */
    const float* emb_ln_b;
    const float* d_slopes;      /* fp32 [heads]: the ALiBi slope of every head */
    const mq_jina_bert_layer* layers;  /* host array, `layers` entries */
} mq_jina_bert_weights;

typedef struct mq_jina_bert_cfg {
    int32_t width;         /* W, multiple of 64, <= 2048 */
    int32_t layers;
    int32_t heads;         /* heads * 64 == W */
    int32_t head_dim;      /* 64 */
    int32_t mlp_dim;       /* F = intermediate_size, multiple of 64 */
    int32_t vocab;
    int32_t max_pos;       /* longest sequence served (<= 8192) */
    int32_t pool;          /* MQ_POOL_MEAN or MQ_POOL_CLS */
    float   ln_eps;        /* layer_norm_eps */
    int32_t reserved;
} mq_jina_bert_cfg;

int mq_attention_alibi(const void* d_qkv, void* d_out, const int32_t* d_cu_seqlens, int64_t nseq, int32_t fixed_len, int32_t max_len, int32_t heads,
                       int32_t head_dim, const float* d_slopes, float scale, void* stream);
size_t mq_jina_bert_workspace_bytes(const mq_jina_bert_cfg* cfg, int64_t rows, int64_t nseq);
int mq_encode_jina_bert(const mq_jina_bert_cfg* cfg, const mq_jina_bert_weights* w, const int32_t* d_ids, const int32_t* d_cu_seqlens,
                        const int32_t* h_cu_seqlens, int64_t nseq, float* d_out, int normalize, void* d_workspace, size_t workspace_bytes, void* stream);

/* ---- DeBERTa-v2 / -v3 rerankers: disentangled attention, the tower and the scoring call (csrc/attention_disentangled.hip, csrc/deberta.hip,
 * csrc/rerank.hip; engine/deberta.py, engine/rerank.py) ---------------------------------------------------------------------------------------------------
 * transformers' DebertaV2ForSequenceClassification with one label as the mxbai-rerank-*-v1 and cross-encoder/*-deberta-v3-* checkpoints configure it
 * (config.json: model_type "deberta-v2", relative_attention, pos_att_type c2p | p2c, position_biased_input false, type_vocab_size 0, norm_rel_ebd
 * "layer_norm", no convolution): post-LN BERT blocks with biases and an erf-GELU MLP, no position table, and
 *   scores[q, k] = scale (Q_q . K_k + Q_q . Kr[idx(q - k)] + K_k . Qr[idx(q - k)]),  scale = 1 / sqrt(3 head_dim).
 * Additions to ABI 15: nothing above changes; the structs and entry points below are new.  Every entry point judges its arguments before any launch
 * (MQ_ERR_INVALID, the message names the entry point and the bad value), runs on `stream` and allocates nothing.
 *
 *   mq_attention_disentangled: d_qkv bf16 [.., 3 inner] = (q | k | v), inner = heads head_dim, head h at columns h head_dim .. of each third; d_out bf16
 *                   [.., inner]; head_dim 64; sequences packed (d_cu_seqlens int32 [nseq + 1] holds ABSOLUTE row offsets into d_qkv / d_out: its first
 *                   entry need not be 0, so a batch can run in groups behind a moved pointer) or fixed_len > 0; max_len <= 8192.  rows = the call's token
 *                   rows (d_cu_seqlens[nseq] - d_cu_seqlens[0], or nseq fixed_len).  d_pos_key / d_pos_query bf16 [heads][2 span][64] = Kr / Qr, span in
 *                   [1, 1024].  d_idx int32 [2 reach + 1]: entry d + reach = idx(d) in [0, 2 span - 1], the bucket of query - key == d, non-decreasing in
 *                   d, built by the caller on the host (the kernel forms no logarithm); max_len > reach + 1 is refused.  [win_lo, win_hi] = [idx(-(max_len
 *                   - 1)), idx(max_len - 1)]: the buckets the call can touch.  The position scores pass through the workspace as fp32 strips
 *                   [rows][heads][2][win rounded up to 16] (mq_attention_disentangled_workspace_bytes; MQ_ERR_WORKSPACE when short); no [T, T] tensor
 *                   exists in global memory.  nseq <= 0: MQ_OK, nothing is written.  Compiler report (gfx950): csrc/attention_disentangled.hip's header.
 *   mq_encode_deberta: token gather + LayerNorm -> `layers` blocks  x = LN(Wo(attn(Wqkv(x))) + x) ; x = LN(W2(gelu(W1(x))) + x)  -> mq_pool (MQ_POOL_CLS or
 *                   MQ_POOL_MEAN) (+ L2), on packed sequences like mq_encode_bert; fp32 residual stream, bf16 GEMM operands.  width a multiple of 64, <=
 *                   2048; head_dim 64; heads * 64 == width; mlp_dim % 64 == 0; max_pos <= min(8192, reach + 1).  The attention runs over groups of whole
 *                   sequences whose strips stay under 256 MiB (or one sequence's, when that alone is larger).  d_out fp32 [nseq, width].
 *   mq_score_head_gelu: mq_score_head with the erf GELU in place of tanh (ContextPooler: pooler.dense -> GELU -> classifier); the same weights struct
 *                   (type_vocab is not read) and scratch (mq_score_head_workspace_bytes).
 *   mq_score_pairs_deberta: mq_encode_deberta(cfg, w, ..., normalize = 0) with cfg->pool == MQ_POOL_CLS into a scratch slot (d_pooled fp32 [nseq, W],
 *                   NULL ok, receives a copy) -> mq_score_head_gelu.  d_logits fp32 [nseq]; d_scores (NULL ok) = sigmoid.  Scratch:
 *                   mq_score_pairs_deberta_workspace_bytes(cfg, rows, nseq). */
typedef struct mq_deberta_layer {
    const void*  qkv_w;         /* bf16 [3 W, W]  rows: query_proj | key_proj | value_proj */
    const float* qkv_b;         /* fp32 [3 W] */
    const void*  out_w;         /* bf16 [W, W]  attention.output.dense */
    const float* out_b;         /* fp32 [W] */
    const float* attn_ln_g;     /* fp32 [W]  attention.output.LayerNorm */
    const float* attn_ln_b;
    const void*  fc1_w;         /* bf16 [F, W]  intermediate.dense */
    const float* fc1_b;         /* fp32 [F] */
    const void*  fc2_w;         /* bf16 [W, F]  output.dense */
    const float* fc2_b;         /* fp32 [W] */
    const float* mlp_ln_g;      /* fp32 [W]  output.LayerNorm */
    const float* mlp_ln_b;
    const void*  pos_key;       /* bf16 [heads][2 span][64]  Kr = key_proj | pos_key_proj of LayerNorm(rel_embeddings), split into heads */
    const void*  pos_query;     /* bf16 [heads][2 span][64]  Qr = query_proj | pos_query_proj of the same rows */
} mq_deberta_layer;

typedef struct mq_deberta_weights {
    const float* tok_emb;       /* fp32 [vocab, W]  embeddings.word_embeddings */
    const float* emb_ln_g;      /* fp32 [W]  embeddings.LayerNorm */
    const float* emb_ln_b;
    const int32_t* d_idx;       /* device int32 [2 reach + 1]: entry d + reach = the bucket of query - key == d */
    const int32_t* h_idx;       /* the same table on the host */
    const mq_deberta_layer* layers;  /* host array, `layers` entries */
} mq_deberta_weights;

typedef struct mq_deberta_cfg {
    int32_t width;         /* W, multiple of 64, <= 2048 */
    int32_t layers;
    int32_t heads;         /* heads * 64 == W */
    int32_t head_dim;      /* 64 */
    int32_t mlp_dim;       /* F = intermediate_size, multiple of 64 */
    int32_t vocab;
    int32_t max_pos;       /* longest sequence served (<= 8192, <= reach + 1) */
    int32_t pool;          /* MQ_POOL_MEAN or MQ_POOL_CLS */
    int32_t span;          /* S = position_buckets: the position tables have 2 S rows */
    int32_t reach;         /* the index table covers |query - key| <= reach */
    float   ln_eps;        /* layer_norm_eps */
    int32_t reserved;
} mq_deberta_cfg;

size_t mq_attention_disentangled_workspace_bytes(int64_t rows, int32_t heads, int32_t win_lo, int32_t win_hi);
int mq_attention_disentangled(const void* d_qkv, void* d_out, const int32_t* d_cu_seqlens, int64_t nseq, int64_t rows, int32_t fixed_len, int32_t max_len,
                              int32_t heads, int32_t head_dim, const void* d_pos_key, const void* d_pos_query, const int32_t* d_idx, int32_t reach,
                              int32_t span, int32_t win_lo, int32_t win_hi, float scale, void* d_workspace, size_t workspace_bytes, void* stream);
size_t mq_deberta_workspace_bytes(const mq_deberta_cfg* cfg, int64_t rows, int64_t nseq);
int mq_encode_deberta(const mq_deberta_cfg* cfg, const mq_deberta_weights* w, const int32_t* d_ids, const int32_t* d_cu_seqlens,
                      const int32_t* h_cu_seqlens, int64_t nseq, float* d_out, int normalize, void* d_workspace, size_t workspace_bytes, void* stream);
int mq_score_head_gelu(const float* d_h, int64_t n, int32_t W, const mq_score_head_weights* head, float* d_logits, float* d_scores, void* d_workspace,
                       size_t workspace_bytes, void* stream);
size_t mq_score_pairs_deberta_workspace_bytes(const mq_deberta_cfg* cfg, int64_t rows, int64_t nseq);
int mq_score_pairs_deberta(const mq_deberta_cfg* cfg, const mq_deberta_weights* w, const mq_score_head_weights* head, const int32_t* d_ids,
                           const int32_t* d_cu_seqlens, const int32_t* h_cu_seqlens, int64_t nseq, float* d_logits, float* d_scores, float* d_pooled,
                           void* d_workspace, size_t workspace_bytes, void* stream);

/* ---- NomicBERT text embedders: sliced full attention and the tower (csrc/attention_full.hip, csrc/nomic_bert.hip; engine/nomic_bert.py) ----------------
 * nomic-embed-text-v1 / -v1.5 / -v1-unsupervised, their fine-tunes and snowflake-arctic-embed-m-long (config.json: model_type "nomic_bert"): post-LN
 * blocks with biased LayerNorms, bias-free Linears, a gated-SiLU MLP, full-width rotate-half rotary positions, a token-type row, no position table, plain
 * bidirectional softmax attention over up to 8192 tokens.  The block semantics are pinned to transformers' NomicBertModel in float64.
 * Additions to ABI 15: nothing above changes; the structs and entry points below are new.  Every entry point judges its arguments before any launch
 * (MQ_ERR_INVALID, the message names the entry point and the bad value), runs on `stream` and allocates nothing.
 *
 *   mq_attention_full: d_qkv bf16 [rows, 3 inner] = (q | k | v), inner = heads head_dim, head h at columns h head_dim .. of each third; d_out bf16
 *                   [rows, inner]; head_dim 64; sequences packed or fixed-length as mq_attention, max_len <= 8192.  Unmasked, bidirectional, every key
 *                   of the sequence contributes: out = softmax(scale (q . k)) V, scale > 0 the caller's.  The function mq_attention computes at
 *                   MQ_MASK_NONE, with the work split over (sequence, head, 64-query slice) instead of (sequence, head): one workgroup of 4 waves per
 *                   slice, the K / V image has the whole LDS (640 keys; longer sequences stream through in pieces).  Compiler report (gfx950):
 *                   csrc/attention_full.hip's header.
 *   mq_encode_nomic_bert: token gather + type row 0 + LayerNorm -> `layers` blocks  x = LN(Wo(attn(rope(Wqkv(x)))) + x) ; x = LN(Wdown(up * silu(gate)) + x)
 *                   with (up | gate) = Wug(x)  -> mq_pool (MQ_POOL_MEAN or MQ_POOL_CLS) (+ L2), on packed sequences like mq_encode_bert; fp32 residual
 *                   stream, bf16 GEMM operands; softmax scale 1 / sqrt(head_dim); rotary angle = position in the sequence * d_inv_freq[i], rotate_half
 *                   form over the whole head (mq_rope).  width a multiple of 64, <= 2048; head_dim 64; heads * 64 == width; mlp_dim % 64 == 0;
 *                   max_pos <= 8192.  d_out fp32 [nseq, width]. */
typedef struct mq_nomic_bert_layer {
    const void*  qkv_w;         /* bf16 [3 W, W]  rows: q | k | v, no bias */
    const void*  out_w;         /* bf16 [W, W]  self_attn.o_proj, no bias */
    const float* attn_ln_g;     /* fp32 [W]  post_attention_layernorm */
    const float* attn_ln_b;
    const void*  ug_w;          /* bf16 [2F, W]  rows: up_proj | gate_proj (mq_glu's order), no bias */
    const void*  down_w;        /* bf16 [W, F]  mlp.down_proj, no bias */
    const float* mlp_ln_g;      /* fp32 [W]  post_mlp_layernorm */
    const float* mlp_ln_b;
} mq_nomic_bert_layer;

typedef struct mq_nomic_bert_weights {
    const float* tok_emb;       /* fp32 [vocab, W]  embeddings.word_embeddings */
    const float* type0;         /* fp32 [W]  row 0 of embeddings.token_type_embeddings */
    const float* emb_ln_g;      /* fp32 [W]  embeddings.LayerNorm */
    const float* emb_ln_b;
    const float* zeros;         /* fp32 [W] of 0: the bias operand of the residual epilogues (no Linear has a bias) */
    const float* d_inv_freq;    /* fp32 [32]: rope_theta ^ -(2 i / 64) */
    const mq_nomic_bert_layer* layers;  /* host array, `layers` entries */
} mq_nomic_bert_weights;

typedef struct mq_nomic_bert_cfg {
    int32_t width;         /* W, multiple of 64, <= 2048 */
    int32_t layers;
    int32_t heads;         /* heads * 64 == W */
    int32_t head_dim;      /* 64 */
    int32_t mlp_dim;       /* F = intermediate_size, multiple of 64 */
    int32_t vocab;
    int32_t max_pos;       /* longest sequence served (<= 8192) */
    int32_t pool;          /* MQ_POOL_MEAN or MQ_POOL_CLS */
    float   ln_eps;        /* layer_norm_eps */
    int32_t reserved;
} mq_nomic_bert_cfg;

int mq_attention_full(const void* d_qkv, void* d_out, const int32_t* d_cu_seqlens, int64_t nseq, int32_t fixed_len, int32_t max_len, int32_t heads,
                      int32_t head_dim, float scale, void* stream);
size_t mq_nomic_bert_workspace_bytes(const mq_nomic_bert_cfg* cfg, int64_t rows, int64_t nseq);
int mq_encode_nomic_bert(const mq_nomic_bert_cfg* cfg, const mq_nomic_bert_weights* w, const int32_t* d_ids, const int32_t* d_cu_seqlens,
                         const int32_t* h_cu_seqlens, int64_t nseq, float* d_out, int normalize, void* d_workspace, size_t workspace_bytes, void* stream);

/* ---- Jina v3 text embedders: per-sequence task LoRA adapters and the tower (csrc/lora.hip, csrc/jina_v3.hip; engine/jina_v3.py) -----------------------
 * jina-embeddings-v3 (config.json: model_type "jina_embeddings_v3", transformers' JinaEmbeddingsV3Model): the NomicBERT block with biases on all four
 * Linears and a plain fc1 -> erf-GELU -> fc2 MLP, plus one low-rank adapter per task on every Linear and on the token table.  Adapters are NOT merged into
 * the weights: the base GEMM runs once for all rows and a row of sequence s with task t = task[s] gets  y += scale_t (x A_t^T) B_t^T  on top, so one batch
 * may hold sequences of different tasks and sequences without adapter (task[s] < 0: the row's delta is not computed, its bits are what the base model
 * leaves).  Additions to ABI 15: nothing above changes; the structs and entry points below are new.  Every entry point judges its arguments before any
 * launch (MQ_ERR_INVALID, the message names the entry point and the bad value), runs on `stream` and allocates nothing.
 *
 * The sequence arguments of the three LoRA entry points: d_seq_task int32 [nseq] on the device and h_seq_task, its host copy (the host copy is judged — an
 * id >= tasks is refused — and decides whether anything is launched; the kernels read the device copy and treat ids outside [0, tasks) as "no adapter");
 * sequences packed (d_cu_seqlens int32 [nseq + 1], cu[0] == 0, cu[nseq] == rows) or fixed_len > 0 rows each (rows == nseq fixed_len, d_cu_seqlens NULL ok).
 *
 *   mq_lora_down:   d_T fp32 [rows, R] = scale_t (x A_t^T): d_x bf16 [rows, K] with leading dimension lda, d_A bf16 [tasks][R][K], d_scale fp32 [tasks].
 *                   R a multiple of 4 in [4, 64] (a rank that is none is padded with zero rows at load), K % 64 == 0, lda % 8 == 0.  Rows without adapter
 *                   get T = 0.  When NO sequence has an adapter nothing is launched and d_T is not written.
 *   mq_lora_up:     delta[m, n] = sum_j T[m, (n / (N / nblocks)) r + j] B_t[n, j]: d_T fp32 [rows, R], R = nblocks r; d_B bf16 [tasks][N][r]; r in
 *                   {4, 8, 12, 16}; N % 4 == 0, N % nblocks == 0, (N / nblocks) % 4 == 0 (q | k | v stacked: nblocks = 3); ldc % 4 == 0.  mode:
 *                   MQ_LORA_ACCUM d_out fp32 [rows, ldc] += delta ; MQ_LORA_WRITE d_out fp32 = delta (0 for rows without adapter) ; MQ_LORA_INPLACE d_out
 *                   bf16 [rows, ldc] = act(d_out + delta) with act 0 or MQ_ACT_GELU (the erf GELU of MQ_EPI_GELU).  Rows without adapter: not touched
 *                   (ACCUM; INPLACE with act 0), act(d_out) (INPLACE with MQ_ACT_GELU).  When no sequence has an adapter only MQ_LORA_WRITE and the GELU
 *                   form launch.
 *   mq_lora_gather: d_T fp32 [rows, r] = scale_t A_emb_t[id[m], :]: d_ids int32 [rows], d_A_emb fp32 [tasks][vocab][r] (PEFT's lora_embedding_A,
 *                   transposed).  The embedding adapter's up half is mq_lora_up in MQ_LORA_ACCUM (B_emb in bf16).
 *   mq_encode_jina_v3: token gather + type row 0 (+ embedding adapter) -> LayerNorm -> `layers` blocks  x = LN(Wo(attn(rope(Wqkv(x)))) + x) ;
 *                   x = LN(W2(gelu(W1(x))) + x), every Linear with its bias and, with `lora`, its per-row correction -> mq_pool (MQ_POOL_MEAN or
 *                   MQ_POOL_CLS) (+ L2), on packed sequences like mq_encode_nomic_bert.  lora NULL: the base model, d_seq_task / h_seq_task are not read
 *                   and no LoRA kernel is launched.  lora != NULL: the task lists are required; with every task negative only fc1's activation pass
 *                   (mq_lora_up, MQ_LORA_INPLACE + MQ_ACT_GELU) is launched, so that a sequence without adapter gets the same bits in any batch.  Where
 *                   the corrections sit: csrc/jina_v3.hip's header.  Limits: mq_encode_nomic_bert's.  Compiler report: csrc/lora.hip's header. */
#define MQ_LORA_ACCUM 0
#define MQ_LORA_WRITE 1
#define MQ_LORA_INPLACE 2

typedef struct mq_jina_v3_layer {
    const void*  qkv_w;         /* bf16 [3 W, W]  rows: q | k | v */
    const float* qkv_b;         /* fp32 [3 W] */
    const void*  out_w;         /* bf16 [W, W]  self_attn.o_proj */
    const float* out_b;         /* fp32 [W] */
    const float* attn_ln_g;     /* fp32 [W]  post_attention_layernorm */
    const float* attn_ln_b;
    const void*  fc1_w;         /* bf16 [F, W]  mlp.fc1 */
    const float* fc1_b;         /* fp32 [F] */
    const void*  fc2_w;         /* bf16 [W, F]  mlp.fc2 */
    const float* fc2_b;         /* fp32 [W] */
    const float* mlp_ln_g;      /* fp32 [W]  post_mlp_layernorm */
    const float* mlp_ln_b;
} mq_jina_v3_layer;

typedef struct mq_jina_v3_weights {
    const float* tok_emb;       /* fp32 [vocab, W]  embeddings.word_embeddings */
    const float* type0;         /* fp32 [W]  row 0 of embeddings.token_type_embeddings */
    const float* emb_ln_g;      /* fp32 [W]  embeddings.LayerNorm */
    const float* emb_ln_b;
    const float* d_inv_freq;    /* fp32 [32]: rope_theta ^ -(2 i / 64) */
    const mq_jina_v3_layer* layers;  /* host array, `layers` entries */
} mq_jina_v3_weights;

typedef struct mq_jina_v3_lora_layer {      /* every tensor [tasks] x ..., bf16; a Linear that a task does not adapt carries zeros for it */
    const void* qkv_a;          /* [tasks][3 r][W]  rows: A_q | A_k | A_v */
    const void* qkv_b;          /* [tasks][3 W][r]  rows: B_q | B_k | B_v */
    const void* out_a;          /* [tasks][r][W] */
    const void* out_b;          /* [tasks][W][r] */
    const void* fc1_a;          /* [tasks][r][W] */
    const void* fc1_b;          /* [tasks][F][r] */
    const void* fc2_a;          /* [tasks][r][F] */
    const void* fc2_b;          /* [tasks][W][r] */
} mq_jina_v3_lora_layer;

typedef struct mq_jina_v3_lora {
    int32_t tasks;              /* adapters, 1 .. 1024 */
    int32_t rank;               /* r: 4, 8, 12 or 16 (zero-padded at load) */
    const float* d_scale;       /* fp32 [tasks]: lora_alpha / r, or lora_alpha / sqrt(r) (rsLoRA) */
    const float* emb_a;         /* fp32 [tasks][vocab][r], or NULL with emb_b: no embedding adapter */
    const void*  emb_b;         /* bf16 [tasks][W][r] */
    const mq_jina_v3_lora_layer* layers;  /* host array, `layers` entries */
} mq_jina_v3_lora;

typedef struct mq_jina_v3_cfg {
    int32_t width;         /* W, multiple of 64, <= 2048 */
    int32_t layers;
    int32_t heads;         /* heads * 64 == W */
    int32_t head_dim;      /* 64 */
    int32_t mlp_dim;       /* F = intermediate_size, multiple of 64 */
    int32_t vocab;
    int32_t max_pos;       /* longest sequence served (<= 8192) */
    int32_t pool;          /* MQ_POOL_MEAN or MQ_POOL_CLS */
    float   ln_eps;        /* layer_norm_eps */
    int32_t reserved;
} mq_jina_v3_cfg;

int mq_lora_down(const void* d_x, int64_t lda, const void* d_A, const float* d_scale, const int32_t* d_seq_task, const int32_t* h_seq_task,
                 const int32_t* d_cu_seqlens, int64_t nseq, int32_t fixed_len, int64_t rows, int32_t tasks, int32_t R, int32_t K, float* d_T, void* stream);
int mq_lora_up(const float* d_T, int32_t R, const void* d_B, int32_t r, int32_t nblocks, const int32_t* d_seq_task, const int32_t* h_seq_task,
               const int32_t* d_cu_seqlens, int64_t nseq, int32_t fixed_len, int64_t rows, int32_t tasks, void* d_out, int64_t ldc, int32_t N, int32_t mode,
               int32_t act, void* stream);
int mq_lora_gather(const int32_t* d_ids, const float* d_A_emb, const float* d_scale, const int32_t* d_seq_task, const int32_t* h_seq_task,
                   const int32_t* d_cu_seqlens, int64_t nseq, int32_t fixed_len, int64_t rows, int32_t tasks, int32_t r, int32_t vocab, float* d_T,
                   void* stream);
size_t mq_jina_v3_workspace_bytes(const mq_jina_v3_cfg* cfg, int64_t rows, int64_t nseq);
int mq_encode_jina_v3(const mq_jina_v3_cfg* cfg, const mq_jina_v3_weights* w, const mq_jina_v3_lora* lora, const int32_t* d_ids, const int32_t* d_cu_seqlens,
                      const int32_t* h_cu_seqlens, const int32_t* d_seq_task, const int32_t* h_seq_task, int64_t nseq, float* d_out, int normalize,
                      void* d_workspace, size_t workspace_bytes, void* stream);

/* ---- Gemma rerankers: causal and prefix-sharing grouped-query attention at 256-wide heads, and the pair-scoring tower
 * (csrc/attention_gqa256_causal.hip, csrc/gemma_causal.hip; engine/rerank.py GemmaRerankerTower) ----------------------------------------------------------
 * transformers' GemmaForCausalLM (model_type "gemma": BAAI/bge-reranker-v2-gemma = Gemma-2B, 18 blocks, width 2048, 8 query heads over ONE K/V head of
 * width 256) read as a judge whose score is the logit of `Yes` at the last token, or GemmaForSequenceClassification with one label: pre-norm blocks with
 * two RMSNorms (weights applied as 1 + w), rotary positions, no q / k norm, no soft-capping, no sliding window, a gated tanh-GELU MLP, the token table
 * scaled by sqrt(width), a causal mask.  One query against n documents: `[bos] A: query` is the same token row for every hit and is computed once.
 * Additions to ABI 15: nothing above changes; the structs and entry points below are new.  Each judges its arguments before any launch (MQ_ERR_INVALID,
 * the message names the entry point and the bad value), runs on `stream` and allocates nothing.
 *
 *   mq_attention_gqa256_causal: mq_attention_gqa_band's layout at head_dim 256 under the causal mask: query i of a sequence sees keys 0 .. i of that
 *                   sequence.  Sequences packed (d_cu_seqlens int32 [nseq + 1], max_len = the longest) or fixed_len > 0.  `scale` is the softmax scale.
 *   mq_attention_gqa256_prefix: mq_attention_gqa_prefix's conventions at head_dim 256, with the softmax scale as an argument: rows [0, prefix_len) of
 *                   d_qkv are the shared prefix, d_cu_seqlens int32 [nseq + 1] with d_cu_seqlens[0] = prefix_len are the segments, max_len = the longest
 *                   SEGMENT, prefix_len + max_len <= 8192; the query at local position t of a segment sees the prefix_len prefix keys and its own
 *                   segment's keys 0 .. t.  Only the segments' rows of d_out are written.  prefix_len need not be a multiple of 64; prefix_len = 0 gives
 *                   the bits of mq_attention_gqa256_causal on the same packed batch (it is the same kernel).  One workgroup of 8 waves per (sequence,
 *                   K/V head, slice of max(1, 8 / G) 16-query blocks) stages the K/V head's tiles once for all G query heads, two 64-key tiles (128 KiB
 *                   of LDS) at a time, and only the prefix's tiles and the own tiles up to the slice's last query.
 *   mq_score_gemma_pairs: mq_score_qwen_pairs' contract on the Gemma blocks: packed rows [prefix | seg_1 | ... | seg_n], d_cu_seqlens / h_cu_seqlens
 *                   int32 [nseq + 2] = {0, prefix_len, prefix_len + d_1, ...}; prefix_len may be 0 (the unshared path).  Per block
 *                   x += Wo(attn(rope(Wqkv(norm(x))))) ; x += Wdown(up * gelu_tanh(gate)) with (up | gate) = Wug(norm(x)); the rotary step runs on the
 *                   prefix at offset 0 and on the segments at offset prefix_len; attention is mq_attention_gqa256_causal on the prefix and
 *                   mq_attention_gqa256_prefix on the segments at cfg->attn_scale; the final RMSNorm runs on every segment's last row only; d_logits fp32
 *                   [nseq] = that row . d_score_w (fp32 [width]), d_scores (may be NULL) its sigmoid.  width <= 2048 (a multiple of 64), head_dim 256,
 *                   mlp_dim % 64 == 0, max_pos <= 8192, prefix_len + the longest segment <= cfg->max_pos. */
typedef struct mq_gemma_causal_layer {
    const float* input_norm_g;  /* fp32 [W]  1 + input_layernorm */
    const void*  qkv_w;         /* bf16 [(Q + 2 KV) hd, W]  rows: q_proj | k_proj | v_proj */
    const void*  out_w;         /* bf16 [W, Q hd]  o_proj */
    const float* post_norm_g;   /* fp32 [W]  1 + post_attention_layernorm */
    const void*  ug_w;          /* bf16 [2F, W]  rows: up_proj | gate_proj (mq_glu's order) */
    const void*  down_w;        /* bf16 [W, F]  down_proj */
} mq_gemma_causal_layer;

typedef struct mq_gemma_causal_weights {
    const float* tok_emb;       /* fp32 [vocab, W]  embed_tokens * sqrtf(W): the fp32 product mq_encode_gemma forms per row, formed once at load */
    const float* final_norm_g;  /* fp32 [W]  1 + norm */
    const float* zeros;         /* fp32 [W] zeros (the bias slot of the residual GEMMs) */
    const float* d_inv_freq;    /* fp32 [hd / 2]: rope_theta ^ -(2 i / hd) */
    const mq_gemma_causal_layer* layers;  /* host array, `layers` entries */
} mq_gemma_causal_weights;

typedef struct mq_gemma_causal_cfg {
    int32_t width;       /* W, multiple of 64, <= 2048 */
    int32_t layers;
    int32_t q_heads;     /* Q */
    int32_t kv_heads;    /* KV, divides Q */
    int32_t head_dim;    /* hd: 256; Q hd need not be W */
    int32_t mlp_dim;     /* F, multiple of 64 */
    int32_t vocab;
    int32_t max_pos;     /* longest pair served (<= 8192) */
    float   rms_eps;
    float   attn_scale;  /* head_dim ^ -0.5 */
} mq_gemma_causal_cfg;

int mq_attention_gqa256_causal(const void* d_qkv, void* d_out, const int32_t* d_cu_seqlens, int64_t nseq, int32_t fixed_len, int32_t max_len,
                               int32_t q_heads, int32_t kv_heads, int32_t head_dim, float scale, void* stream);
int mq_attention_gqa256_prefix(const void* d_qkv, void* d_out, const int32_t* d_cu_seqlens, int64_t nseq, int32_t prefix_len, int32_t max_len,
                               int32_t q_heads, int32_t kv_heads, int32_t head_dim, float scale, void* stream);
size_t mq_score_gemma_pairs_workspace_bytes(const mq_gemma_causal_cfg* cfg, int64_t rows, int64_t nseq);
int mq_score_gemma_pairs(const mq_gemma_causal_cfg* cfg, const mq_gemma_causal_weights* w, const float* d_score_w, const int32_t* d_ids,
                         const int32_t* d_cu_seqlens, const int32_t* h_cu_seqlens, int64_t nseq, int32_t prefix_len, float* d_logits, float* d_scores,
                         void* d_workspace, size_t workspace_bytes, void* stream);

/* ---- Mistral / Llama text embedders: causal sliding-window grouped-query attention, row kernels up to 4096 wide and the tower
 * (csrc/attention_gqa.hip, csrc/llama.hip; engine/llama.py) -------------------------------------------------------------------------------------------------
 * transformers' MistralModel / LlamaModel (model_type "mistral" / "llama": e5-mistral-7b-instruct, SFR-Embedding-Mistral, Linq-Embed-Mistral, Llama-2-shaped
 * fine-tunes): mq_encode_qwen's block without q / k norm and without a QKV bias, up to 4096 wide, with Mistral's sliding window.  Additions to ABI 15:
 * nothing above changes (mq_rmsnorm, mq_embed_tokens, mq_pool, mq_encode_qwen keep their 2048 bound and their refusals); the struct and entry points
 * below are new.  Each judges its arguments before any launch (MQ_ERR_INVALID, the message names the entry point and the bad value), runs on `stream` and
 * allocates nothing.
 *
 *   mq_attention_gqa_window: mq_attention_gqa's layout and sequence arguments; the query at position i of a sequence sees the keys j of that sequence
 *                   with i - window < j <= i (transformers' sliding_window_causal_mask_function).  window >= 1; a window of at least the longest
 *                   sequence gives the bits of mq_attention_gqa with MQ_MASK_CAUSAL.  A 128-query slice stages only the key tiles its band cuts and a
 *                   16-query block visits only its own: the cost of a long sequence is O(T window).
 *   mq_rmsnorm_wide: mq_rmsnorm's contract (row gather, bf16 and / or fp32 output, in place on the fp32 rows) for W % 64 == 0, W <= 4096.  W <= 2048:
 *                   mq_rmsnorm itself (the same bits).
 *   mq_embed_tokens_wide: d_x fp32 [rows, W] = tok[clamp(id)] over packed sequences: the gather of mq_embed_tokens without positions, types or
 *                   LayerNorm, W % 64 == 0, W <= 4096.  W <= 2048: mq_embed_tokens itself.
 *   mq_pool_wide:   mq_pool's MQ_POOL_MEAN (+ L2 as F.normalize forms it) for W % 64 == 0, W <= 4096.  W <= 2048: mq_pool itself.  (The last-token
 *                   tail is mq_last_rows, mq_rmsnorm_wide through the row index and mq_l2_normalize, which has no width bound.)
 *   mq_encode_llama: mq_encode_qwen's tower on mq_qwen_weights whose layers carry no qkv_b / q_norm_g / k_norm_g (all three must be NULL), through the
 *                   wide row kernels.  cfg->window > 0 and smaller than the longest sequence of the call: every layer attends through
 *                   mq_attention_gqa_window; otherwise through mq_attention_gqa (causal).  width <= 4096 (a multiple of 64), head_dim 64 or 128,
 *                   mlp_dim % 64 == 0, max_pos <= 8192.  d_out fp32 [nseq, width]. */
typedef struct mq_llama_cfg {
    int32_t width;       /* W, multiple of 64, <= 4096 */
    int32_t layers;
    int32_t q_heads;     /* Q */
    int32_t kv_heads;    /* KV, divides Q */
    int32_t head_dim;    /* hd: 64 or 128; Q hd need not be W */
    int32_t mlp_dim;     /* F, multiple of 64 */
    int32_t vocab;
    int32_t max_pos;     /* longest sequence served (<= 8192) */
    int32_t pool;        /* MQ_POOL_LAST or MQ_POOL_MEAN */
    int32_t window;      /* sliding_window (>= 1), or 0: none */
    float   rms_eps;
    int32_t reserved0;   /* 0 */
} mq_llama_cfg;

int mq_attention_gqa_window(const void* d_qkv, void* d_out, const int32_t* d_cu_seqlens, int64_t nseq, int32_t fixed_len, int32_t max_len,
                            int32_t q_heads, int32_t kv_heads, int32_t head_dim, int32_t window, void* stream);
int mq_rmsnorm_wide(const float* d_x, const int32_t* d_row_idx, const float* d_g, void* d_out_bf16, float* d_out_f32, int64_t rows, int32_t W, float eps,
                    void* stream);
int mq_embed_tokens_wide(const int32_t* d_ids, const int32_t* d_cu, int64_t nseq, const float* tok, float* d_x, int32_t W, int32_t vocab, void* stream);
int mq_pool_wide(const float* d_x, const int32_t* d_cu, int64_t nseq, float* d_out, int32_t W, int32_t normalize, void* stream);
size_t mq_llama_workspace_bytes(const mq_llama_cfg* cfg, int64_t rows, int64_t nseq);
int mq_encode_llama(const mq_llama_cfg* cfg, const mq_qwen_weights* w, const int32_t* d_ids, const int32_t* d_cu_seqlens, const int32_t* h_cu_seqlens,
                    int64_t nseq, float* d_out, int normalize, void* d_workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MARQO_HIP_H */

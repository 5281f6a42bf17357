// Host scaffold of the entry points that take packed token sequences (ids [rows] + cu_seqlens): the workspace bump helper, the sequence-length walk, the
// checks in front of the first launch and the cfg checks the decoder-style towers share.  Host code only: no kernel lives here.
// Users: modernbert.hip, qwen.hip, llama.hip, gemma.hip (all of it), towers.hip (mq_encode_bert, mq_encode_clip_text) and rerank.hip (score_pairs).
#pragma once
#include "common.h"

constexpr size_t WS_ALIGN = 256;

// bump allocator over the caller's workspace: take() returns the (256-B aligned) OFFSET of a slice, end() the aligned total
struct Off {
    size_t off = 0;
    size_t take(size_t bytes) {
        off = align_up(off, WS_ALIGN);
        const size_t o = off;
        off += bytes;
        return o;
    }
    size_t end() const { return align_up(off, WS_ALIGN); }
};

// longest sequence of a packed batch (-1 when any length is below 1) and its row count; the caller has checked h_cu[0] == 0
static inline int max_seq_len(const int32_t* h_cu, int64_t nseq, int64_t* rows_out) {
    int mx = 0;
    for (int64_t i = 0; i < nseq; ++i) {
        const int l = h_cu[i + 1] - h_cu[i];
        if (l < 1) return -1;
        if (l > mx) mx = l;
    }
    *rows_out = h_cu[nseq] - h_cu[0];
    return mx;
}

// what a packed-token entry point checks once its weights are judged and nseq > 0: the inputs, cu_seqlens[0], every length in [1, max_pos] -> maxl, rows
static inline int packed_begin(const char* what, const void* d_ids, const int32_t* d_cu_seqlens, const int32_t* h_cu_seqlens, int64_t nseq, int max_pos,
                               const void* d_workspace, int* maxl, int64_t* rows) {
    MQ_CHECK_ARG(d_ids && d_cu_seqlens && h_cu_seqlens && d_workspace, "%s: null input / workspace", what);
    MQ_CHECK_ARG(h_cu_seqlens[0] == 0, "%s: cu_seqlens[0] must be 0", what);
    *maxl = max_seq_len(h_cu_seqlens, nseq, rows);
    MQ_CHECK_ARG(*maxl >= 1 && *maxl <= max_pos, "%s: sequence lengths must be in [1, max_pos=%d]", what, max_pos);
    return MQ_OK;
}

// ... and, with the plan of those rows in hand, the last refusal in front of the first launch
static inline int packed_workspace(const char* what, size_t workspace_bytes, size_t required) {
    if (workspace_bytes < required) {
        mq_set_error("%s: workspace %zu < required %zu", what, workspace_bytes, required);
        return MQ_ERR_WORKSPACE;
    }
    return MQ_OK;
}

// cfg checks of the grouped-query towers (Qwen, Gemma), in front of their own width bound
static inline int check_gqa_shape(const char* what, int q_heads, int kv_heads, int width) {
    MQ_CHECK_ARG(q_heads >= 1 && kv_heads >= 1 && q_heads % kv_heads == 0, "%s: q_heads %d must be a multiple of kv_heads %d", what, q_heads, kv_heads);
    MQ_CHECK_ARG(width >= 64 && width % 64 == 0, "%s: width %d must be a multiple of 64", what, width);
    return MQ_OK;
}

// ... and of all three towers, behind it
static inline int check_tower_sizes(const char* what, int mlp_dim, int layers, int vocab, int max_pos) {
    MQ_CHECK_ARG(mlp_dim >= 64 && mlp_dim % 64 == 0, "%s: mlp_dim %d must be a multiple of 64", what, mlp_dim);
    MQ_CHECK_ARG(layers >= 1 && vocab >= 1, "%s: layers %d / vocab %d", what, layers, vocab);
    MQ_CHECK_ARG(max_pos >= 1 && max_pos <= 8192, "%s: max_pos %d outside [1, 8192]", what, max_pos);
    return MQ_OK;
}

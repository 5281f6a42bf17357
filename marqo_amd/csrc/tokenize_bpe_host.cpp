// Host build of the SentencePiece-BPE functions of tokenize_algo.h (the ones tokenize.hip instantiates on the GPU), for CPU-side pinning against
// the `sentencepiece` wheel (tests/test_nllb_host.py compiles this file with g++; it is not part of libmarqo_hip.so).  One text per call, the three
// phases in sequence with element stride 1 where the kernels stride their LDS scratch by the lane.
#include <stddef.h>
#include <stdint.h>
#include <vector>

#include "tokenize_algo.h"

extern "C" {

struct mq_host_sp_vocab {
    const void* slots; const uint8_t* pool; const float* score; const uint32_t* nmap; const uint8_t* npool; const uint8_t* ccc;
    uint32_t n_slots; int32_t unk_id; float unk_score; int32_t add_dummy_prefix, remove_extra_ws, max_piece_bytes;
    int32_t prefix_id, suffix_id, pad_id, id_offset, unk_out;
};

// row [ld] <- one text; returns the row length, *status = MQ_TOK_OK / MQ_TOK_NEEDS_HOST
int mq_host_sentencepiece_bpe(const mq_host_sp_vocab* v, const uint8_t* text, int nbytes, int max_length, int32_t* row, int ld, int32_t* status) {
    mq_sp_table T;
    T.slots = (const mq_sp_entry*)v->slots; T.pool = v->pool; T.score = v->score; T.nmap = v->nmap; T.npool = v->npool; T.ccc = v->ccc;
    T.mask = v->n_slots - 1; T.unk_id = v->unk_id; T.unk_score = v->unk_score; T.add_dummy_prefix = v->add_dummy_prefix;
    T.remove_extra_ws = v->remove_extra_ws; T.max_piece_bytes = v->max_piece_bytes;
    const mq_sp_frame F{v->prefix_id, v->suffix_id, v->pad_id, v->id_offset, v->unk_out};
    const int cap = max_length;
    const size_t ncap = (size_t)mq_norm_capacity(nbytes), wcap = (size_t)cap;
    std::vector<uint8_t> norm(ncap);
    std::vector<uint64_t> spans(wcap);
    std::vector<int16_t> counts(wcap);
    std::vector<int32_t> pieces(ncap);
    int st = MQ_TOK_OK;
    int nw = mq_spb_split(T, text, nbytes, cap, spans.data(), norm.data(), &st);
    if (nw > cap) nw = cap;
    uint8_t word[MQ_SPB_MAX_WORD], slen[MQ_SPB_MAX_WORD];
    float pair[MQ_SPB_MAX_WORD];
    for (int j = 0; j < nw && st == MQ_TOK_OK; ++j) {
        const int c = mq_spb_word(T, norm.data(), spans[j], pieces.data() + mq_span_start(spans[j]), word, slen, pair, 1);
        if (c < 0) st = MQ_TOK_NEEDS_HOST;
        counts[j] = (int16_t)(c < 0 ? 0 : c);
    }
    *status = st;
    const int len = mq_spb_gather(T, F, spans.data(), counts.data(), pieces.data(), st == MQ_TOK_OK ? nw : 0, max_length, row, ld);
    return st == MQ_TOK_OK ? len : 0;
}

}  // extern "C"

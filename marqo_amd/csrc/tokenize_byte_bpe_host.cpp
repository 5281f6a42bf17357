// Host build of the GPT-2 / RoBERTa byte-level BPE functions of tokenize_algo.h (the ones tokenize.hip instantiates on the GPU), for CPU-side pinning
// against engine/tokenizers.py::RobertaBpeTokenizer and transformers.RobertaTokenizer (tests/test_byte_bpe_host.py compiles this file with g++; it is
// not part of libmarqo_hip.so).  One text per call, the three phases in sequence with element stride 1 where the kernels stride their LDS scratch by
// the lane.
#include <stddef.h>
#include <stdint.h>
#include <vector>

#include "tokenize_algo.h"

extern "C" {

struct mq_host_byte_bpe_vocab {
    const void* slots; const uint16_t* byte_id; const uint64_t* unicode;
    uint32_t n_slots; int32_t cls_id, sep_id, pad_id;
};

// row [ld] <- one text; returns the row length, *status = MQ_TOK_OK / MQ_TOK_NEEDS_HOST
int mq_host_byte_bpe(const mq_host_byte_bpe_vocab* v, const uint8_t* text, int nbytes, int max_length, int32_t* row, int ld, int32_t* status) {
    mq_bpe_table T;
    T.slots = (const mq_bpe_entry*)v->slots; T.byte_id = v->byte_id; T.byte_end_id = v->byte_id; T.mask = v->n_slots - 1;
    T.sot_id = v->cls_id; T.eot_id = v->sep_id; T.lower = 0;
    const mq_bbpe_frame F{v->cls_id, v->sep_id, v->pad_id};
    const mq_uni_table U{v->unicode};
    const int cap = max_length > 2 ? max_length - 2 : 1;
    std::vector<uint64_t> spans((size_t)cap);
    std::vector<int16_t> counts((size_t)cap);
    std::vector<uint16_t> syms((size_t)nbytes + 1);
    int st = MQ_TOK_OK;
    const int nw = mq_bbpe_split(U, text, nbytes, cap, spans.data(), &st);
    uint16_t sym[MQ_BPE_MAX_SYMS];
    for (int j = 0; j < nw; ++j) counts[j] = (int16_t)mq_bbpe_merge_span(T, text, spans[j], syms.data() + mq_span_start(spans[j]), sym, 1);
    *status = st;
    const int len = mq_bbpe_gather(F, spans.data(), counts.data(), syms.data(), st == MQ_TOK_OK ? nw : 0, max_length, row, ld);
    return st == MQ_TOK_OK ? len : 0;
}

}  // extern "C"

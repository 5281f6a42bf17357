// Run-time knobs (A/B benchmarking and the parity tests of every code path in one process): the one definition of every knob, one table row per
// knob, mq_tune / mq_tune_get.  Host code only, no kernel.  TEST / BENCH ONLY (the loaders never touch them): relaxed atomics (knobs.h) that the
// launch code of every request thread reads — a change takes effect from the next launch that reads it, so set them while no request is in flight
// if one call must run under one setting.  A new knob is one variable and one row here, an extern in knobs.h and a line in include/marqo_hip.h.
#include <stdlib.h>
#include <string.h>
#include "common.h"
#include "knobs.h"

GemmTune g_tune;
std::atomic<uint64_t> mq_gemm_addr_limit{0xffffffffull};
mq_knob mq_tower_row_select, mq_tower_ln_fold, mq_tower_subln_fold, mq_tower_attn_proj, mq_tower_panel_gemm, mq_tower_residual_bf16,
    mq_tower_pool_strided, mq_tower_assemble_stats;
mq_knob mq_gemm_small_max_rows, mq_gemm_small_group_rows;
mq_knob mq_ln_prefetch, mq_ln_rows_per_wave, mq_ln_bf16_wide;
mq_knob mq_xcd_band;
mq_knob mq_attention_waves;

namespace {

// key of mq_tune / mq_tune_get (null: none); env: the value at load (null: always def); var null: gemm_addr_limit_mb, kept in mq_gemm_addr_limit as bytes
struct Knob { const char* key; const char* env; int def; mq_knob* var; };
const Knob g_knobs[] = {
    {"gemm_mt", "MQ_GEMM_MT", 0, &g_tune.mt},                    // 0 = auto (choose_mt), else the tile height in 32-row units (bf16 and fp8 tiles)
    {"gemm_cgroup", "MQ_GEMM_CGROUP", 8, &g_tune.cgroup},        // column tiles per L2 group of the tile walk, 0 = row-major walk
    {"gemm_nh", "MQ_GEMM_NH", 0, &g_tune.nh},                    // 0 = default plan, 1 = (32*MT) x 128 tiles only, 3 = the big 256 x 256 tile on every row wherever N >= 256, 4 = the eager row-split plan
    {nullptr, "MQ_GEMM_FP8_NH", 0, &g_tune.fp8_big},             // the fp8 GEMM's big tile (plan_fp8_big): 0 = plan, 1 = never, 3 = always; follows mq_tune("gemm_nh")
    {"gemm_tail", "MQ_GEMM_TAIL", 0, &g_tune.tail},              // 1 = the big tile's in-kernel split-K tail for a ragged last row of tiles (gemm_sched.h: why it is off)
    {"gemm_wd", "MQ_GEMM_WD", 0, &g_tune.wd},                    // the W-direct main loop (gemm_wd.hip) on the narrow tiles: 0 = off, 2 / 3 = on with that many LDS stages of A, 6 / 7 = the same with both k-halves' W loads issued together
    {"rs_finalize", "MQ_GEMM_RS_FIN", 0, &g_tune.rs_fin},        // 1 = mq_gemm_bf16_rsf finalises the row statistics inside the GEMM's launch, 0 = a row_stats_finalize_kernel launch behind it
    {"row_select", "MQ_ROW_SELECT", 1, &mq_tower_row_select},    // 0 = the towers run their last block on every row instead of the pooled rows only
    {"ln_fold", "MQ_LN_FOLD", 2, &mq_tower_ln_fold},             // 0 = LayerNorm kernels, 1 = folded into the GEMMs with statistics from a read pass, 2 = statistics from the residual GEMMs' partial sums
    {"subln_fold", "MQ_SUBLN_FOLD", 1, &mq_tower_subln_fold},    // 0 = the EVA02 sub-LayerNorms run as LayerNorm passes instead of inside the out-projection / fc2 GEMMs
    {"attn_proj", "MQ_ATTN_PROJ", 128, &mq_tower_attn_proj},     // fewest fixed-length sequences from which a ViT-B/32-shaped block runs attention + out-projection + residual + statistics as ONE launch (attn_proj.hip); 0 = never
    {"panel_gemm", "MQ_PANEL_GEMM", 0, &mq_tower_panel_gemm},    // fewest fixed-length sequences from which the folded QKV / fc1 GEMMs of a 768-wide tower run one workgroup per sequence (panel_gemm.hip); 0 = never
    {"residual_bf16", "MQ_RESIDUAL_BF16", 0, &mq_tower_residual_bf16},        // 1 = pre-LN bf16 towers without a policy of their own keep the residual stream in bf16
    {"pool_strided", "MQ_POOL_STRIDED", 1, &mq_tower_pool_strided},           // 0 = the ViT class-token rows go through an index vector, two gathers and a scatter instead of being used where they lie
    {"assemble_stats", "MQ_ASSEMBLE_STATS", 1, &mq_tower_assemble_stats},     // 0 = a row_stats pass over x behind the ViT token assembly instead of the statistics the assembly leaves itself
    {"small_m", "MQ_SMALL_M", 80, &mq_gemm_small_max_rows},                   // rows up to which the towers take the skinny GEMM path, 0 = never
    {"small_m_grouped", "MQ_SMALL_M_GROUPED", 320, &mq_gemm_small_group_rows},  // rows up to which a plain GEMM call takes the skinny kernel in row groups of <= 80, 0 = no grouping
    {"ln_prefetch", "MQ_LN_PREFETCH", 1, &mq_ln_prefetch},       // 0 = the towers' LayerNorms do not prefetch the weights of the GEMMs behind them; 2 / 3 = 64 / 32 bytes per touch instead of 128
    {"ln_rows", "MQ_LN_ROWS", 2, &mq_ln_rows_per_wave},          // 1 = one row per wave in the generic LayerNorm at any row count, 2 = two from 8192 rows
    {"ln_bf16_wide", "MQ_LN_BF16_WIDE", 1, &mq_ln_bf16_wide},    // 0 = bf16 rows take the generic LayerNorm, 1 = the 16-byte form above small_m rows, 4 = that form with four rows per wave from 16384 rows
    {"xcd_band", "MQ_XCD_BAND", 1, &mq_xcd_band},                // 0 = the row-wise kernels do not follow the GEMMs' XCD banding
    {"attn_waves", nullptr, 0, &mq_attention_waves},             // 0 = auto, 4 / 8 wave64s per attention workgroup, 5 = five waves for 65..80-token sequences (else auto)
    {"gemm_addr_limit_mb", nullptr, 0, nullptr},                 // bytes / 2^20 one launch may address per operand, 0 = the 4 GiB - 1 of a 32-bit buffer offset: taller matrices go in row chunks
};

const bool g_knobs_from_env = [] {
    for (const Knob& k : g_knobs) {
        const char* v = k.env ? getenv(k.env) : nullptr;
        if (k.var) *k.var = v ? atoi(v) : k.def;
    }
    return true;
}();

const Knob* find_knob(const char* who, const char* key) {
    for (const Knob& k : g_knobs)
        if (key && k.key && !strcmp(k.key, key)) return &k;
    mq_set_error("%s: unknown key %s", who, key ? key : "(null)");
    return nullptr;
}

}  // namespace

extern "C" int mq_tune(const char* key, int value) {
    const Knob* k = find_knob("mq_tune", key);
    if (!k) return MQ_ERR_INVALID;
    if (k->var) *k->var = value;
    else mq_gemm_addr_limit = value > 0 ? ((uint64_t)value << 20) - 1 : 0xffffffffull;
    if (k->var == &g_tune.nh) g_tune.fp8_big = value == 4 ? 0 : value;
    return MQ_OK;
}

extern "C" int mq_tune_get(const char* key, int* value) {
    const Knob* k = find_knob("mq_tune_get", key);
    if (!k) return MQ_ERR_INVALID;
    MQ_CHECK_ARG(value, "mq_tune_get: null value");
    const uint64_t lim = mq_gemm_addr_limit;
    *value = k->var ? (int)*k->var : lim == 0xffffffffull ? 0 : (int)((lim + 1) >> 20);
    return MQ_OK;
}

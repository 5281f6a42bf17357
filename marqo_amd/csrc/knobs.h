// The library's run-time knobs (mq_tune / mq_tune_get, test and bench only): defined, tabled and initialised from the environment in knobs.hip.
// Relaxed atomics: request threads read them in their launch code while a test thread may set them.
#pragma once
#include <atomic>
#include <stdint.h>

typedef std::atomic<int> mq_knob;

// the tiled GEMMs' schedule (gemm_sched.h); mt and cgroup steer the bf16 and the fp8 tiles alike
struct GemmTune { mq_knob mt, cgroup, nh, fp8_big, tail, wd, rs_fin; };
extern GemmTune g_tune;
extern std::atomic<uint64_t> mq_gemm_addr_limit;   // bytes one launch may address per operand (4 GiB - 1; tests lower it)

extern mq_knob mq_tower_row_select, mq_tower_ln_fold, mq_tower_subln_fold, mq_tower_attn_proj, mq_tower_panel_gemm, mq_tower_residual_bf16,
    mq_tower_pool_strided, mq_tower_assemble_stats;                                  // read in towers.hip
extern mq_knob mq_gemm_small_max_rows, mq_gemm_small_group_rows;                     // gemm_small.hip, rowops.hip
extern mq_knob mq_ln_prefetch, mq_ln_rows_per_wave, mq_ln_bf16_wide;                 // rowops.hip, embed.hip, attn_proj.hip
extern mq_knob mq_xcd_band;                                                          // the row-wise kernels' launches (common.h, xcd_banded_block)
extern mq_knob mq_attention_waves;                                                   // attention.hip

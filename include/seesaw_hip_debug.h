/* seesaw_hip_debug.h -- lab-bench entry points of libseesaw_hip_debug.so.
 *
 * NOT part of the product ABI.  The product library (libseesaw_hip.so, include/seesaw_hip.h) is compiled without
 * -DSSW_DEBUG_HOOKS: its kernel-selection switches are constants and none of the symbols below exist in it.  The lab
 * build compiles the same sources with -DSSW_DEBUG_HOOKS and adds csrc/debug_hooks.hip and csrc/gemm_pw4.hip; tests and
 * tools that compare kernel variants, feed single kernels with chosen operands or read intermediate state load that
 * library instead (seesaw_amd._lib.debug_hooks()).  The switches are process-global and not thread-safe: one test at a
 * time.  Nothing here has a counterpart in the reference.
 */
#ifndef SEESAW_HIP_DEBUG_H
#define SEESAW_HIP_DEBUG_H

#include "seesaw_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* tuning hook (tools/sweep_scan.py): pick the scan kernel's schedule variant for dim=512
 * (0 u4, 1 u4+nt, 2 u8, 3 u8+nt, 4 u2+nt; -1 = default) and cap its resident blocks per CU
 * (0 = no cap, -1 = default).  Indexes under 65 536 rows run a latency-shaped kernel (8 rows in flight per wave, query
 * through LDS) unless a variant is named; -2 = the default streaming variant at every size.  All produce identical bits.
 * The f16 index's scan reads the same switches: at dim=512 0 u4, 1 u8+nt, 4 u2+nt, other = default u4+nt. */
ssw_status ssw_tune_scan(int32_t variant, int32_t blocks_per_cu);

/* The widest chunk of ssw_index_scan_batch / ssw_index_topk_batch: 1 (every query through the single-query scan), 2, 4,
 * 8 or 16; any other value = the product's (16 for f32 rows, 8 for f16 rows).  All widths write identical bits.  blocks_per_cu: four-wave blocks per CU of the multi-query
 * kernel (1 .. 8; any other value = the product's, 2).  tools/perf_topk_batch.py sweeps both. */
ssw_status ssw_tune_scan_batch(int32_t max_width, int32_t blocks_per_cu);

/* ssw_index_topk on an index of <= 8192 images / 65536 rows and <= 8192 excluded ids runs as three launches (query staged
 * through a kernel argument; scan; per-image max + exclusion + selection in one workgroup) with the ids and the result in
 * pinned memory the device maps -- no copies, no stream wait (flag bit 0).  From 2^24 values on and k <= 2048 the selection's threshold comes from a
 * 1-in-16 sample instead of two full histogram passes (flag bit 1; exact all the same: a sample that leaves fewer than k
 * candidates raises the overflow word and the deep path runs).  Default 3; tests switch the forms off to compare. */
ssw_status ssw_tune_topk(int32_t flags);

/* The pruned top-k (seesaw_hip.h, ssw_index_prune_stats): enable 0 = every top-k scans in full (what
 * SSW_TOPK_FULL_SCAN does), min_rows >= 0 = the smallest index that is pruned, for f32 and f16 rows alike,
 * reserve_bytes = the free device memory a shadow must leave (< 0 = the defaults: 2^22 rows for f32 and for f16 rows,
 * 4 GiB).  Applies to the next top-k of every index; a shadow refused for memory is retried only after its rows
 * change. */
ssw_status ssw_tune_prune(int32_t enable, int64_t min_rows, int64_t reserve_bytes);

/* The launch shape of the shadow scan (k_q8_bounds): four-wave blocks per CU (1 .. 8) and 16-byte loads a lane keeps in
 * flight per group (4, 8 or 16: 4, 8 or 16 KiB a wave); any other value = the product's (1 block, 8 loads).  Every
 * shape writes bounds that satisfy the same certificate; the summation order of a row's products differs with the
 * loads a group.  tools/sweep_prune.py times them. */
ssw_status ssw_tune_prune_scan(int32_t blocks_per_cu, int32_t group_loads);

/* The pre-scan's intermediate state, for tests/test_prune_certificate_gpu.py.  The three hooks run the product's
 * kernels through the launch functions of the pruned top-k on the index's own buffers; all out pointers are HOST
 * memory; the index must be one the next top-k would prune (ssw_tune_prune, dim 256 / 512 / 1024, own rows).
 * shadow: builds the int8 shadow if it is missing or stale (the product's ensure_shadow -> k_q8_build; SSW_ERR_NOMEM
 *   when it is refused for memory) and copies out the codes [n_rows, dim] int8, s_r and a_r [n_rows] of the rows
 *   [first_row, first_row + n_rows); an output that is NULL is skipped.
 * bounds: k_q8_query + k_q8_bounds for a host query (finite, as for ssw_index_topk): out_lb [n] = every row's lower
 *   bound, *out_Q = the state's Q, *out_unbounded = its "the query cannot be bounded" word.  The bounds stay in the
 *   score buffer, marked partial with the query kept, exactly as after the product's shadow scan: every reader of
 *   the buffer (ssw_index_topk without a query, gather, ...) first completes it with the full scan of that query.
 * survivors: k_survivors + k_prune_publish over the bounds of the last ssw_debug_prune_bounds (SSW_ERR_INVALID when a
 *   reader has completed the buffer since) against the caller's threshold, standing in for what the threshold
 *   selection leaves: k keys of that value, a count of sel_count keys and the overflow word sel_overflow.  cap <= 2^18
 *   is the list's capacity.  *out_published = what the host would read (survivors, or -1 = fall back to the full scan),
 *   *out_collected = the device's survivor counter (it passes cap when more rows qualify; 0 when nothing was
 *   collected), out_rows [cap] receives the first *out_published rows of the list (unordered). */
ssw_status ssw_debug_prune_shadow(ssw_index *idx, int64_t first_row, int64_t n_rows, int8_t *out_codes, float *out_scale,
                                  float *out_err);
ssw_status ssw_debug_prune_bounds(ssw_index *idx, const float *q_host, float *out_lb, float *out_Q,
                                  int32_t *out_unbounded);
ssw_status ssw_debug_prune_survivors(ssw_index *idx, float threshold, int32_t k, int32_t sel_count, int32_t sel_overflow,
                                     int64_t cap, int32_t *out_published, int64_t *out_collected, int64_t *out_rows);

/* The packed 6-bit shadow that single queries on a large f32 or f16 index scan instead of the int8 one (csrc/prune.hip,
 * "6-bit shadow"; tests/test_prune6_gpu.py, tests/test_prune6_f16_gpu.py).  None of these changes what the hooks above
 * do: they keep building and driving the int8 shadow, and ssw_tune_prune's min_rows keeps governing the int8 path only.
 * ssw_tune_prune6: enable 0 = every index takes the int8 path at every size (A/B in one process); min_rows >= 0 = the
 *   smallest index, of either dtype, whose single queries scan the 6-bit shadow, < 0 = the product's constants again.
 *   Dim 768: the 6-bit hooks (ssw_debug_prune6_shadow / _bounds / _survivors / _scan_shape, the _mq ones below and
 *   ssw_debug_prune_maxima with six != 0) admit a dim-768 index, which has the 6-bit shadow alone and is governed by
 *   ssw_tune_prune6 and ssw_tune_prune6_batch only, never by ssw_tune_prune's min_rows; the int8 hooks above keep
 *   refusing it ("the index is not pruned", "dim=768 has no shadow scan").
 * ssw_tune_prune6_scan: the launch shape of k_q6_bounds: four-wave blocks per CU (1 .. 8) and 16-row tiles a wave
 *   requests at a time (1, 2 or 4, as far as tiles x dim <= 1024); any other value = the product's (1 block; 2 / 1 / 1 / 1
 *   tiles at dim 256 / 512 / 768 / 1024).  ssw_debug_prune6_scan_shape: the blocks and tiles of the next launch.
 * ssw_debug_prune6_shadow: builds the 6-bit shadow if it is missing or stale (the product's ensure_shadow ->
 *   k_q6_build or k_q6_build_h16) and copies out, for the rows [first_row, first_row + n_rows): the codes [n_rows, dim]
 *   unpacked to int8 in natural element order (by the placement function the kernels use), s6_r and a6_r.  NULL
 *   outputs are skipped.
 * ssw_debug_prune6_bounds: k_q6_query + k_q6_bounds through the product's launch functions for one host query
 *   (non-finite allowed: it is flagged).  out_I [n] = the exact integer sums of 4 c with 256 d_hi + d_lo (int64),
 *   out_lb [n], out_Qe [4] = Q, e, t2 and the "cannot be bounded" word as floats, out_codes [2, dim] = the query's hi
 *   and lo plane in natural element order.  Any output may be NULL.  The handle is left as after the product's
 *   shadow scan: partial, the query kept. */
ssw_status ssw_tune_prune6(int32_t enable, int64_t min_rows);
ssw_status ssw_tune_prune6_scan(int32_t blocks_per_cu, int32_t tiles);
ssw_status ssw_debug_prune6_scan_shape(ssw_index *idx, int32_t *out_blocks, int32_t *out_tiles);
ssw_status ssw_debug_prune6_shadow(ssw_index *idx, int64_t first_row, int64_t n_rows, int8_t *out_codes, float *out_scale,
                                   float *out_err);
ssw_status ssw_debug_prune6_bounds(ssw_index *idx, const float *q_host, int64_t *out_I, float *out_lb, float *out_Qe,
                                   int8_t *out_codes);
/* The survivor passes' pre-test on the bounds alone (csrc/prune.hip, survivor_pass; tests/test_prune_tail_gpu.py).
 * ssw_debug_prune_maxima: builds the int8 (six = 0) or the 6-bit (six != 0) shadow if it is missing or stale and copies
 *   out what k_shadow_max left for it: out2 [2] = the largest finite a_r and the largest finite s_r.
 * ssw_debug_prune6_survivors: k_survivors_mq with the 6-bit code norm + k_prune_publish_mq over the bounds of the last
 *   ssw_debug_prune6_bounds; arguments and outputs as ssw_debug_prune_survivors. */
ssw_status ssw_debug_prune_maxima(ssw_index *idx, int32_t six, float *out2);
ssw_status ssw_debug_prune6_survivors(ssw_index *idx, float threshold, int32_t k, int32_t sel_count, int32_t sel_overflow,
                                      int64_t cap, int32_t *out_published, int64_t *out_collected, int64_t *out_rows);

/* The packed 5-bit shadow that single queries on a large f32 index of dim 512 or 1024 without an image map scan instead
 * of the 6-bit one, with the threshold raised to the k-th exact score of a thousand candidates (csrc/prune.hip, "5-bit
 * shadow"; tests/test_prune5_gpu.py).  None of these changes what the hooks above do.
 * ssw_tune_prune5: enable 0 = no index takes the 5-bit path (A/B in one process); min_rows >= 0 = the smallest index whose
 *   single queries scan the 5-bit shadow, < 0 = the product's constant again (25 M rows).  ssw_tune_prune(0, ..) still
 *   switches every pruned path off.
 * ssw_tune_prune5_scan: the launch shape of k_q5_bounds: four-wave blocks per CU (1 .. 8) and 16-row tiles a wave
 *   requests at a time (1 or 2 at dim 512, 1 at dim 1024); any other value = the product's (1 block; 2 / 1 tiles at dim
 *   512 / 1024).  ssw_debug_prune5_scan_shape: the blocks and tiles of the next launch.
 * ssw_debug_prune5_shadow: builds the 5-bit shadow if it is missing or stale (the product's ensure_shadow -> k_q5_build)
 *   and copies out, for the rows [first_row, first_row + n_rows): the codes [n_rows, dim] unpacked to int8 in natural
 *   element order (by q5_fields, the placement function the builder uses), s5_r and a5_r.  NULL outputs are skipped.
 * ssw_debug_prune5_bounds: k_q6_query + k_q5_bounds through the product's launch functions for one host query; outputs
 *   as ssw_debug_prune6_bounds, out_I [n] = the exact integer sums of 8 c with 256 d_hi + d_lo.
 * ssw_debug_prune5_survivors: k_survivors_mq with the 5-bit code norm + k_prune_publish_mq over the bounds of the last
 *   ssw_debug_prune5_bounds, against a threshold written by hand (the product raises the selection's k-th key to the
 *   exact threshold first); arguments and outputs as ssw_debug_prune_survivors. */
ssw_status ssw_tune_prune5(int32_t enable, int64_t min_rows);
/* The two-stage 4 + 1-bit shadow (csrc/prune.hip; tests/test_prune41_gpu.py).
 * ssw_tune_prune41: enable 0 = no index takes the two-stage path; min_rows >= 0 = the smallest index whose single queries
 *   take it, < 0 = the product's constant again; coarse_cap in [0, 2^23] = the first-stage survivors above which the
 *   refine walks every row instead of the list (dense), any other value = 2^23.
 * ssw_tune_prune41_scan / ssw_debug_prune41_scan_shape: the launch shape of k_q4_bounds, as ssw_tune_prune5_scan.
 * ssw_debug_prune41_shadow: builds the shadow if it is missing or stale and copies out, for rows [first_row, first_row +
 *   n_rows): the nibbles h [n_rows, dim] in natural element order (by q4_nibble, the builder's placement function), the
 *   fine plane's words [n_rows, dim / 32], s5, a5 and a4.  NULL outputs are skipped.
 * ssw_debug_prune41_stage1: k_q41_query + k_q4_bounds for one host query: out_H [n], out_lb4 [n], out_Qe [4] as
 *   ssw_debug_prune6_bounds, out_sumD [2] = the sums of the hi and lo code planes.
 * ssw_debug_prune41_survivors1: k_survivors_q4 over those bounds against a threshold written by hand, with `blocks`
 *   blocks (0 = the product's grid): *out_count = the counter, out_rows [min(count, rows_cap)] the list.
 * ssw_debug_prune41_refine: k_q41_refine over the list `rows` [m] given by hand (repeats allowed), against a threshold
 *   written by hand; with m above the coarse cap the kernel walks every row instead and the outputs are per row.
 *   out_lb5 / out_B: per entry (per row when dense); *out_survivors and out_surv_rows [min(survivors, SURV_CAP)]. */
ssw_status ssw_tune_prune41(int32_t enable, int64_t min_rows, int64_t coarse_cap);
ssw_status ssw_tune_prune41_scan(int32_t blocks_per_cu, int32_t tiles);
ssw_status ssw_debug_prune41_scan_shape(ssw_index *idx, int32_t *out_blocks, int32_t *out_tiles);
ssw_status ssw_debug_prune41_shadow(ssw_index *idx, int64_t first_row, int64_t n_rows, uint8_t *out_h, uint32_t *out_fine,
                                    float *out_s5, float *out_a5, float *out_a4);
ssw_status ssw_debug_prune41_stage1(ssw_index *idx, const float *q_host, int32_t *out_H, float *out_lb4, float *out_Qe,
                                    int32_t *out_sumD);
ssw_status ssw_debug_prune41_survivors1(ssw_index *idx, float threshold, int32_t k, int32_t blocks, int64_t rows_cap,
                                        int64_t *out_count, uint32_t *out_rows);
ssw_status ssw_debug_prune41_refine(ssw_index *idx, const uint32_t *rows, int64_t m, float threshold, int32_t k,
                                    float *out_lb5, int32_t *out_B, int64_t *out_survivors, int64_t *out_surv_rows);
ssw_status ssw_tune_prune5_scan(int32_t blocks_per_cu, int32_t tiles);
ssw_status ssw_debug_prune5_scan_shape(ssw_index *idx, int32_t *out_blocks, int32_t *out_tiles);
ssw_status ssw_debug_prune5_shadow(ssw_index *idx, int64_t first_row, int64_t n_rows, int8_t *out_codes, float *out_scale,
                                   float *out_err);
ssw_status ssw_debug_prune5_bounds(ssw_index *idx, const float *q_host, int64_t *out_I, float *out_lb, float *out_Qe,
                                   int8_t *out_codes);
ssw_status ssw_debug_prune5_survivors(ssw_index *idx, float threshold, int32_t k, int32_t sel_count, int32_t sel_overflow,
                                      int64_t cap, int32_t *out_published, int64_t *out_collected, int64_t *out_rows);

/* The pruned batch (seesaw_hip.h, ssw_index_topk_batch_pruned).
 * ssw_tune_prune_scan_mq: the launch shape of its shadow scan (k_q8_bounds_mq): four-wave blocks per CU (1 .. 8) and
 *   16-row tiles a wave requests at a time (1, 2 or 4, as far as two register sets of them fit: tiles x dim <= 1024);
 *   any other value = the product's (1 block; 2 tiles at dim 256 and 512, 1 at dim 1024).  ssw_tune_prune's min_rows
 *   and reserve apply to the pruned batch as well.
 * ssw_debug_prune_scan_mq_shape: the blocks and tiles the next launch over this index would use (a wave's request is
 *   16 x tiles rows; a launch has 4 x blocks waves).
 * ssw_debug_prune_bounds_mq: k_q8_query_mq + k_q8_bounds_mq for nq <= 16 host queries (non-finite ones allowed: they are
 *   flagged) on the index's own buffers, with the kernel's debug flag on when an integer output is asked for.
 *   out_I_hi / out_I_lo [nq, n] = the exact int32 sums of a row's codes with the query's two code planes, out_lb [nq, n],
 *   out_Qe [nq, 4] = Q, e, t2 and the "cannot be bounded" word (0 / 1) as floats, out_codes [nq, 2, dim] = the hi and
 *   the lo plane in natural element order.  Any output may be NULL.  The handle is left as after the product's shadow
 *   scan of the chunk: partial, the last query kept.
 * ssw_debug_prune_survivors_mq: k_survivors_mq for one slot of the chunk of nq queries the last ssw_debug_prune_bounds_mq
 *   bounded, then k_prune_publish_mq; arguments and outputs as ssw_debug_prune_survivors. */
ssw_status ssw_tune_prune_scan_mq(int32_t blocks_per_cu, int32_t tiles);
ssw_status ssw_debug_prune_scan_mq_shape(ssw_index *idx, int32_t *out_blocks, int32_t *out_tiles);
ssw_status ssw_debug_prune_bounds_mq(ssw_index *idx, const float *q_host, int32_t nq, int32_t *out_I_hi, int32_t *out_I_lo,
                                     float *out_lb, float *out_Qe, int8_t *out_codes);
ssw_status ssw_debug_prune_survivors_mq(ssw_index *idx, int32_t nq, int32_t slot, float threshold, int32_t k,
                                        int32_t sel_count, int32_t sel_overflow, int64_t cap, int32_t *out_published,
                                        int64_t *out_collected, int64_t *out_rows);

/* The pruned batch's chunk on the packed 6-bit shadow (csrc/prune.hip, "a chunk of up to 16 queries on the 6-bit
 * shadow"; tests/test_prune6_batch_gpu.py): what a pruned batch runs on an index that ssw_tune_prune6 and
 * ssw_tune_prune6_batch make six-eligible, instead of the int8 chunk above.  The hooks above keep driving the int8 chunk; a chunk's state words,
 * planes and slabs belong to whichever pair of hooks bounded it last.
 * ssw_tune_prune6_batch: min_rows >= 0 = the smallest index, of either dtype, whose pruned batches scan the 6-bit
 *   shadow, provided its single queries do (ssw_tune_prune6: the batch never goes below the single call); < 0 = the
 *   product's two constants again (25 M rows).  ssw_tune_prune6's own min_rows does not move the batch: with it
 *   alone a pruned batch on a small index keeps building and scanning the int8 shadow.
 * ssw_tune_prune6_scan_mq: the launch shape of k_q6_bounds_mq: four-wave blocks per CU (1 .. 8) and 16-row tiles a wave
 *   requests at a time (1, 2 or 4, as far as tiles x dim <= 1024); any other value = the product's (1 block; 4 / 2 / 1 / 1
 *   tiles at dim 256 / 512 / 768 / 1024).  ssw_debug_prune6_scan_mq_shape: the blocks and tiles of the next launch.
 * ssw_debug_prune6_bounds_mq: k_q6_query_mq + k_q6_bounds_mq through the product's launch functions for nq <= 16 host
 *   queries (non-finite ones allowed: they are flagged) on the index's own buffers; builds the 6-bit shadow if it is
 *   missing or stale.  out_I [nq, n] = the exact integer sums of 4 c with 256 d_hi + d_lo (int64), out_lb [nq, n],
 *   out_Qe [nq, 4] = Q, e, t2 and the "cannot be bounded" word as floats, out_codes [nq, 2, dim] = the hi and the lo
 *   plane, put back into natural element order by q6_slot.  Any output may be NULL.  The handle is left as after the
 *   product's shadow scan of the chunk: partial, the last query kept.
 * ssw_debug_prune6_survivors_mq: k_survivors_mq with the 6-bit code norm for one slot of the chunk the last
 *   ssw_debug_prune6_bounds_mq bounded, then k_prune_publish_mq; arguments and outputs as ssw_debug_prune_survivors. */
ssw_status ssw_tune_prune6_batch(int64_t min_rows);
ssw_status ssw_tune_prune6_scan_mq(int32_t blocks_per_cu, int32_t tiles);
ssw_status ssw_debug_prune6_scan_mq_shape(ssw_index *idx, int32_t *out_blocks, int32_t *out_tiles);
ssw_status ssw_debug_prune6_bounds_mq(ssw_index *idx, const float *q_host, int32_t nq, int64_t *out_I, float *out_lb,
                                      float *out_Qe, int8_t *out_codes);
ssw_status ssw_debug_prune6_survivors_mq(ssw_index *idx, int32_t nq, int32_t slot, float threshold, int32_t k,
                                         int32_t sel_count, int32_t sel_overflow, int64_t cap, int32_t *out_published,
                                         int64_t *out_collected, int64_t *out_rows);

/* The pruned batch that stays on the device (seesaw_hip.h, ssw_index_topk_batch_dev_pruned; csrc/rescore_dev.hip).
 * ssw_tune_surv_cap: the survivors a slot of that entry may have and still be certified (and the final survivors of a
 *   single query on the two-stage 4 + 1-bit shadow, ssw_tune_prune41), 1 .. 2^18; any other value =
 *   the product's 2^18.  Governs that entry and the hook below only.
 * ssw_debug_rescore_survivors: k_rescore_survivors alone, through the product's launch function, on the index's own
 *   chunk buffers (dim 256 / 512 / 1024; no shadow is needed).  nq <= 16 host queries [nq, dim]; slot j's state words
 *   are set to counts[j] survivors, "selection failed" = fail_bits[j] & 1, "unboundable" = (fail_bits[j] >> 1) & 1;
 *   its list is the next min(counts[j], cap) entries of rows_host (the lists lie end to end; rows in [0, n), repeats
 *   allowed), cap being ssw_tune_surv_cap's.  Every slab is filled with the f32 of bits 0x7FC0BEEF first;
 *   out_slabs_host [nq, n] receives the slabs after the launch and *out_waves the waves a slot had in it.  The
 *   handle's score buffer is left as after ssw_index_scan of the last query. */
ssw_status ssw_tune_surv_cap(int64_t cap);
ssw_status ssw_debug_rescore_survivors(ssw_index *idx, const float *q_host, int32_t nq, const int64_t *rows_host,
                                       const int64_t *counts, const int32_t *fail_bits, float *out_slabs_host,
                                       int32_t *out_waves);

/* Kernel A/B harness for the towers' bf16 GEMM (C[M,N] = A[M,K] W[N,K]^T + epilogue `epi`, see
 * csrc/gemm_bf16.hip): runs `variant` on seeded operands, reports ms per launch over `iters`
 * launches and the max |difference| to variant 0.  Not part of the reference's interface. */
ssw_status ssw_debug_gemm(int32_t M, int32_t N, int32_t K, int32_t epi, int32_t variant, int32_t iters,
                          float *out_ms, float *out_maxdiff);
/* Selects the GEMM variant the towers use (0 register-staged, 2 LDS-DMA ring with 4 waves per tile,
 * 14 the same with 8 waves per tile, 7 256-row pipelined, 9 the 8-wave 256 x 256 tile, 20-23 the persistent
 * four-wave kernel of csrc/gemm_pw4.hip with its column tile chosen / 256 / 192 / 128). */
ssw_status ssw_tune_gemm(int32_t variant);
/* Diagnostics of csrc/gemm_pw4.hip for tools/perf_gemm.py: mode 0 the kernel, 1 cycle stamps (out6 = cycles in the
 * mid-step wait + barrier, cycles in K-steps, K-steps, waves, s_memtime and s_memrealtime ticks per kernel; read and reset), 2-4 ablations (no LDS-DMA / no MFMA /
 * no fragment reads inside the loop: wrong results, timing only). */
ssw_status ssw_debug_gemm_pw4_mode(int32_t mode, uint64_t *out6_or_null);
/* mode 1's per-workgroup record of the last launch: [1024][4] = start, end (100-MHz ticks), HW_ID, XCC_ID; then mode 5's
 * [20] = cycles per interleave group (16), wait + barrier, sub-stages (summed over waves; read and reset) */
ssw_status ssw_debug_gemm_pw4_wg(uint64_t *out4116);

/* ONE product of the towers' bf16 GEMM on the caller's operands, everything it writes returned (tests/test_gemm_gpu.py
 * compares every shipped epilogue with a torch f32 matmul + the same epilogue).  All pointers are HOST memory; bf16
 * values travel as uint16 bit patterns.  epi (csrc/gemm_bf16.hip, enum Epilogue):
 *   0 C = A W^T                       -> C f32          4 LayerNorm folded (GemmLn): rstd (A W'^T - mean c1) + c2 -> C bf16
 *   1 + bias                          -> C bf16         5 the same + quick-GELU                                   -> C bf16
 *   2 + bias, quick-GELU              -> C bf16         6 + bias + residual -> C f32, xcopy = bf16(C), stats_out
 *   3 + bias + residual (f32)         -> C f32          7 xcopy += A W^T + bias in place (bf16 stream), stats_out
 * A [M,K], W [N,K] (K-contiguous, nn.Linear's layout), bias / c2 [N], residual [M,N] f32, xcopy [M,N] bf16,
 * stats_in [M][np_in][2] partial (sum, sum of squares) of the un-normalised f32 rows, c1 [N], stats_out [M][N/128][2].
 * variant: the kernel (ssw_tune_gemm's numbers; -1 = the library's default choice).
 * Three more forms take another meaning of `variant`: 8 = the split-K product (launch_gemm_splitk_f32; variant = splits);
 * 9 = epilogue 6 behind a split-K product (launch_gemm_splitk_stats: the text tower's fc2; variant = splits); 10 = epilogue 6
 * with the residual rows at a stride (GemmLn::res_ld: the pooled last layer's out-projection; variant = S, residual holds
 * M * S rows and row m * S is added to row m). */
ssw_status ssw_debug_gemm_run(int32_t epi, int32_t variant, int32_t M, int32_t N, int32_t K, const uint16_t *A_bf16,
                              const uint16_t *W_bf16, const float *bias_or_c2, const float *residual_or_null,
                              uint16_t *xcopy_inout_or_null, const float *stats_in_or_null, int32_t np_in,
                              const float *c1_or_null, float inv_dim, float eps, void *C_out_or_null,
                              float *stats_out_or_null);

/* The image tower's fused attention + out-projection launch (csrc/attn_out.hip) on the caller's operands.  qkv
 * [B*S, 3*768] bf16 (q | k | v), Wo [768,768] bf16 as nn.Linear holds it (packed here), bo [768]; bf16 stream
 * (res_in NULL): xcopy [B*S,768] bf16 is read, added to and returned; f32 stream: res_in -> res_out [B*S,768] f32 and
 * xcopy returns the bf16 copy.  stats_out [B*S][2][2]: partial (sum, sum of squares) of the new row's column halves. */
ssw_status ssw_debug_attn_out_run(int32_t B, int32_t S, const uint16_t *qkv_bf16, const uint16_t *Wo_bf16, const float *bo,
                                  uint16_t *xcopy_inout, const float *res_in_or_null, float *res_out_or_null,
                                  float *stats_out, float scale);
/* s_memtime stamps of the last launch of that kernel under SSW_AO_STAMPS=1: out[wg * 32 + slot], slots 0..4 = start, after
 * attention, after the product, after the stores, end; 8 + 2p / 9 + 2p = head pair p staged / computed */
ssw_status ssw_debug_attn_out_stamps(uint64_t *out, int32_t n_words);

/* ONE launch of one of the towers' attention kernels (csrc/clip.hip) on the caller's operands, with the launch shape
 * run_tower gives it (tests/test_attention_gpu.py holds each to an f64 softmax).  form: 0 attention_mfma<4>,
 * 1 attention_mfma<4, 2>, 2 attention_mfma<5>, 3 attention_rows64, 4 launch_attention_long (its own choice of
 * instance), 5 attn_pooled_rows (out is [B, D]: row 0 of every sequence; non-causal only).  qkv [qkv_rows_alloc, 3 D]
 * bf16 (q | k | v; rows_alloc >= B S), out [out_rows_alloc, D] bf16: both buffers travel whole, up and -- after the one
 * launch on the default stream -- down, so the rows past B S (past B for form 5) are guards the caller fills and reads
 * back.  SSW_ERR_UNSUPPORTED, with nothing launched and out untouched: S < 1, S > 64 (forms 0, 1, 3, 5), S > 80
 * (form 2), S > 272 (form 4), D != 64 H, causal with form 5. */
ssw_status ssw_debug_attention_run(int32_t form, int32_t B, int32_t S, int32_t D, int32_t H, int32_t causal, float scale,
                                   const uint16_t *qkv_bf16, int64_t qkv_rows_alloc, uint16_t *out_bf16_inout,
                                   int64_t out_rows_alloc);
/* The text tower's fused attention + out-projection of a short query (skinny_attn_out<1> for B L <= 16 rows, <2> for
 * 17 .. 32; more is SSW_ERR_UNSUPPORTED): qkv [B L, 1536] bf16, Wo [512, 512] bf16 as nn.Linear holds it, bias [512],
 * residual [B L, 512] f32, out [B L, 512] f32 is uploaded, written by the one launch and returned.  On the device 32
 * rows of 0xFF bytes follow the qkv, residual and out rows: a read past the rows shows as NaN in the output, a write
 * past them is SSW_ERR_NUMERIC. */
ssw_status ssw_debug_skinny_attn_out_run(int32_t B, int32_t L, int32_t causal, float scale, const uint16_t *qkv_bf16,
                                         const uint16_t *Wo_bf16, const float *bias, const float *residual,
                                         float *out_f32_inout);

/* Keep the residual rows behind transformer layer `layer` of tower `tower` (0 image, 1 text; layer -1 = off) of the
 * handle's next forward passes, as f32 [rows][hidden]; ssw_clip_debug_tap_read waits for the stream and returns them
 * (tests/test_clip_gpu.py compares every layer with transformers' output_hidden_states). */
ssw_status ssw_clip_debug_tap(ssw_clip *clip, int32_t tower, int32_t layer);
ssw_status ssw_clip_debug_tap_read(ssw_clip *clip, float *out_host_or_null, int64_t cap_floats, int64_t *out_rows,
                                   int32_t *out_dim);

/* The device-side tile pyramid (csrc/tiler.hip) seen from outside, through the product's planner, job table and
 * kernels (tests/test_device_tiling_gpu.py).  resize: one image [src_h, src_w, 3] uint8 -> the level [dst_h, dst_w, 3]
 * (any size from 1 x 1 on: no tile is cut) back on the host, rows tight.  multiscale_tiles: the arguments of
 * ssw_clip_embed_multiscale_u8 without `normalize`; returns the uint8 tiles [n, tile, tile, 3] the gather would read
 * instead of their vectors. */
ssw_status ssw_debug_resize_u8(ssw_clip *clip, const uint8_t *src_hwc_host, int32_t src_w, int32_t src_h, int32_t dst_w,
                               int32_t dst_h, uint8_t *out_hwc_host);
ssw_status ssw_debug_clip_multiscale_tiles(ssw_clip *clip, const uint8_t *images_hwc_concat_host, int32_t n_images,
                                           const int64_t *image_offsets, const int32_t *image_hw,
                                           const int32_t *level_first, const int32_t *level_wh, uint8_t *out_tiles_host,
                                           int64_t out_cap_tiles, int64_t *out_n_tiles);

/* The f64 loss of the engine's last evaluation (ssw_fb_lossgrad, ssw_fb_lossgrad2, ssw_fb_lossgrad2_dev), which those
 * entries round to f32 on the way out.  The fit drivers compare the f64 value (L-BFGS stops on |loss - prev_loss| <
 * 1e-9), so a restatement of the driver around the engine's own evaluation needs it (tests/test_fit_driver_gpu.py).
 * Host code only: reads the word the evaluation left, launches nothing.  After a fit it holds that fit's last word. */
ssw_status ssw_debug_fb_last_loss(const ssw_fb *fb, double *out);

#ifdef __cplusplus
}
#endif
#endif /* SEESAW_HIP_DEBUG_H */

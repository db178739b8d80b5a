// index_prune.hip -- the certified pre-scan of the index's top-k: when it applies, the int8, the packed 6-bit, the packed
// 5-bit and the two-stage 4 + 1-bit shadow of the rows, and the steps of one pruned query and of one pruned chunk of a batch (kernels: prune.hip).  The handle:
// index_handle.h.
#include <algorithm>

#include "index_handle.h"

using namespace ssw;

// ---- the certified pre-scan (prune.hip) -------------------------------------------------------
// Top-k with a query on an index of at least MIN_ROWS rows scans a shadow instead of the rows and rescores the
// survivors exactly; the score buffer then holds exact scores for the survivors and lower bounds elsewhere
// (scores_partial) until a consumer that reads all of it materialises the full scan of the kept query; the second-stage
// readers make exact the rows they read (rescore_rows) and leave it partial.
constexpr int64_t NO_SHADOW = INT64_MAX;  // the int8 shadow at dim 768: no such shadow (q8_dim_supported)
// The rows from which a call is pruned on a shadow: [ShadowKind][single call, batch][dim 256 / 512 / 1024, dim 768]
// [f32, f16 rows].  The two row formats are measured separately and need not stay equal.
constexpr int64_t MIN_ROWS[2][2][2][2] = {
    // ---- SHADOW_Q8 ----
    {{// single call
      {(int64_t)1 << 22,  // above the feedback loop's 1.56 M rows, below a rank's 12.5 M
       // f16 rows: the full scan reads half the bytes, yet the pruned call is ahead from the smallest size of the
       // measured sweep on (2^22 rows: 0.49 against 0.72 ms a call, profiles/prune_f16_sweep.txt), so the value is the
       // f32 one
       (int64_t)1 << 22},
      {NO_SHADOW, NO_SHADOW}},
     {// the pruned batch (ssw_index_topk_batch_pruned) against the plain batch at 16 queries: its own entries, chosen by
      // its own sweep ("Pruned batch"), the single call's value for either row format
      {(int64_t)1 << 22, (int64_t)1 << 22},
      {NO_SHADOW, NO_SHADOW}}},
    // ---- SHADOW_Q6 ----
    {{// Single queries on an f32 index of at least this many rows scan the packed 6-bit shadow (392 instead of 520 bytes
      // a row at dim 512, more survivors) and never need the int8 one.  The value follows from tools/perf_prune.py
      // --three-way ("6-bit shadow"): the smallest size from which the 6-bit call beats the int8
      // call, there and at every larger size, by more than both spreads.
      // Measured with the survivor pass that reads the bounds alone (profiles/prune_tail_sweep.txt): 2^23 (0.719 against
      // 0.816 ms a call, spreads 0.043 together; at 2^22 the gap of 0.032 ms is inside the spreads' 0.042).  The ~22 000
      // survivors of the 6-bit bounds no longer cost 0.3 ms, which was what kept the int8 call ahead below 2^25 rows.
      {(int64_t)1 << 23,
       // f16 rows (the shadow is built from the widened rows by k_q6_build_h16, the same bytes a row): its own entry
       // under the same rule, from the same tool with --dtype float16 (the same file): 2^24 rows is the smallest
       // measured size from which the 6-bit call is ahead by more than both spreads, there and above (1.239 against
       // 1.409 ms a call, spreads 0.155; 6.75 against 8.10 at 100 M).  At 2^23 and 12.5 M rows the 6-bit call is ahead by
       // 0.06 and 0.12 ms, but both forms' spreads were 0.2-0.3 ms in that run, so the rule does not admit them.
       (int64_t)1 << 24},
      // A dim-768 index has the 6-bit shadow alone (584 bytes a row against 3072 of f32 and 1536 of f16 rows; the int8
      // scan's lanes-per-row map has no C = 3, prune.hip), so the alternative of a pruned call there is the
      // full-precision path: the full scan for a single query, the plain batch for a batch.  Entries of their own,
      // under the rule above and governed by ssw_tune_prune6 / ssw_tune_prune6_batch alone -- never by ssw_tune_prune's
      // min_rows, which is the int8 shadow's.
      // Single call, tools/perf_prune.py --dim 768 (profiles/prune6_dim768_sweep.txt; full scan and 6-bit call
      // alternating in one process, 2 + 20 rounds, 2^20 .. 2^25, 12.5 M, 25 M and 50 M rows): the 6-bit call is ahead by
      // more than both spreads at EVERY measured size, so each entry is the smallest size of the sweep, 2^20 rows.
      // f32: 0.208 against 0.524 ms a call at 2^20 rows (spreads 0.026 together), 4.903 against 22.655 at 50 M.  f16:
      // 0.203 against 0.320 at 2^20 (spreads 0.023), 4.896 against 12.871 at 50 M.  Nothing below 2^20 rows was measured.
      {(int64_t)1 << 20, (int64_t)1 << 20}},
     {// The pruned batch on an index of at least this many rows bounds its chunks on the 6-bit shadow instead of the
      // int8 one ("Pruned batch on the 6-bit shadow"); below it, and never below the single call's
      // entries (prune6_eligible), the int8 shadow as before.  Entries of their own under the rule above, from
      // tools/perf_prune_batch.py --shadow both (profiles/prune6_batch_ab.txt; the plain, the int8 and the 6-bit batch
      // alternating in one process): 25 M rows is the smallest measured size from which the 6-bit batch is ahead of the
      // int8 batch by more than both spreads, there and above, at nq = 16 and nq = 4 (f32: 0.330 against 0.366 ms a
      // query at nq = 16, spreads 0.015 together; 0.864 against 1.030 at 100 M).  At 2^24 rows and nq = 16 it is ahead
      // by 0.018 (f32) and 0.017 ms (f16) with spreads of 0.021 and 0.019 together -- the two ranges do not overlap, but
      // the rule does not admit it; at 2^23 f32 rows it is ahead by 0.008 with spreads of 0.003, which a size above
      // that fails does not carry.
      {25000000, 25000000},
      // Dim 768, tools/perf_prune_batch.py --dim 768 --nq 16 4 (profiles/prune6_dim768_batch.txt; the plain batch was
      // a loop of full scans when this was measured; against the multi-query kernel the dim has now:
      // profiles/batch_dims_ab.txt): ahead at every size, at nq = 16 and nq = 4.
      // f32, 2^20 rows: 0.115 against 0.562 ms a query at nq = 16 (spreads 0.008), 0.144 against 0.651 at nq = 4
      // (0.019); 50 M rows: 0.651 against 24.837 and 1.615 against 28.876.  f16, 2^20 rows: 0.110 against 0.336 (0.005)
      // and 0.138 against 0.385 (0.008).
      {(int64_t)1 << 20, (int64_t)1 << 20}}}};
// ---- SHADOW_Q5 ----
// Single queries on an f32 index of dim 512 or 1024 without an image map and of at least this many rows scan the packed
// 5-bit shadow (328 instead of 392 bytes a row at dim 512) and raise the threshold to the k-th exact score of a
// thousand candidates (prune.hip, "5-bit shadow"); such an index builds no 6-bit shadow for single queries.  One entry,
// under the rule of the 6-bit single call above, from tools/perf_prune.py --three-way with its fourth column, over 25 M,
// 2^25, 50 M and 100 M rows; never below 25 M rows: tests/test_prune6_gpu.py pins 2^24 f32 rows to the 6-bit shadow's
// bytes.  Measured (profiles/prune5_four_way_sweep.txt, host wall ms a call, 6-bit / 5-bit, medians of 20): 1.697 /
// 1.539 at 25 M (spreads 0.071 together), 2.350 / 1.905 at 2^25, 3.408 / 2.972 at 50 M, 6.335 / 5.377 at 100 M (0.165):
// ahead by more than both spreads at every size of the sweep, so the entry is its smallest.
constexpr int64_t MIN_ROWS_Q5 = 25000000;
// ---- SHADOW_Q41 ----
// The calls that take the 5-bit shadow scan the two-stage 4 + 1-bit shadow instead on an index of at least this many rows
// (264 instead of 328 bytes a row read by the scan at dim 512, a refine pass over the first stage's survivors; prune.hip,
// "two-stage 4 + 1-bit shadow"), and such an index builds no packed 5-bit shadow.  One entry under the rule above
// MIN_ROWS_Q5, against the 5-bit call, over the same sizes; never below 25 M rows.
// Measured (profiles/prune41_sweep.txt, tools/perf_prune.py --two-stage, host wall ms a call, 5-bit / two-stage, medians of
// 20, spreads together in brackets): 1.563 / 1.435 at 25 M (0.067), 2.090 / 1.934 at 2^25 (0.157), 2.825 / 2.701 at 50 M
// (0.250), 5.890 / 4.946 at 100 M (0.224).  The two-stage call is ahead at every size, but at 2^25 and 50 M rows by no more
// than the spreads, so the rule admits 100 M rows alone (profiles/prune41_*_kernel_stats.txt, 10^8 rows: the scan saves
// 0.74 ms a launch and the two passes over the first stage's 1.5 M survivors cost 0.23 ms more than k_survivors_mq).  A second
// run of the sweep (the same file): 1.553 / 1.447 (0.065), 2.078 / 1.953 (0.133), 2.779 / 2.647 (0.071), 5.435 / 4.950
// (0.113) -- 2^25 rows inside the spreads again, 50 M outside them this time; a size has to clear in both.
constexpr int64_t MIN_ROWS_Q41 = 100000000;
constexpr int64_t PRUNE_RESERVE = (int64_t)4 << 30;   // free device memory the shadow must leave
static SSW_TUNABLE bool g_prune = true;               // ssw_tune_prune
static SSW_TUNABLE bool g_prune6 = true;              // ssw_tune_prune6
static SSW_TUNABLE bool g_prune5 = true;              // ssw_tune_prune5
static SSW_TUNABLE int64_t g_prune5_min_rows = -1;     // >= 0: this many rows instead of MIN_ROWS_Q5
static SSW_TUNABLE bool g_prune41 = true;             // ssw_tune_prune41
static SSW_TUNABLE int64_t g_prune41_min_rows = -1;    // >= 0: this many rows instead of MIN_ROWS_Q41
static SSW_TUNABLE int64_t g_coarse_cap = COARSE_CAP;  // first-stage survivors the refine walks as a list; more: dense
static SSW_TUNABLE int64_t g_prune6_min_rows = -1;     // >= 0: this many rows for both dtypes instead
static SSW_TUNABLE int64_t g_prune_min_rows = -1;      // >= 0: this many rows for both dtypes instead
static SSW_TUNABLE int64_t g_prune6_batch_min_rows = -1;  // ssw_tune_prune6_batch: >= 0: the batch's, for both dtypes
static SSW_TUNABLE int64_t g_prune_reserve = PRUNE_RESERVE;
static SSW_TUNABLE int64_t g_surv_cap_dev = SURV_CAP;  // ssw_tune_surv_cap: of ssw_index_topk_batch_dev_pruned, and of the
                                                       // two-stage single call's final survivors (scan_for_topk)

// what differs between the shadows where they are made: the dims, the sizes of the codes and of the two constant
// arrays, what the shadow holds beside them, the builder (into the shadow's buffers), the constant whose maximum the
// survivor pass pre-tests with, and whether a single query on it needs its own state words and operand (state6, planes6)
struct ShadowDesc {
    bool (*dim_ok)(int32_t dim);
    size_t (*code_bytes)(int64_t n, int32_t dim);
    int64_t (*const_rows)(int64_t n);
    size_t (*extra_bytes)(int64_t n, int32_t dim);  // NULL: codes, scale and err are all of it
    ssw_status (*build)(const void *X, int32_t dtype, int64_t n, int32_t dim, const Shadow &s, hipStream_t stream);
    float *Shadow::*width_err;                      // a_r of the bounds the survivor pass reads first (launch_shadow_max)
    bool query_operand;
};
// the two-stage shadow beside its coarse plane, s5 and a5: a4 and H (a word a row each) and the fine plane
static size_t q41_extra_bytes(int64_t n, int32_t dim) {
    return (size_t)packed_padded_rows(n) * (sizeof(float) + sizeof(int32_t)) + q41_fine_bytes(n, dim);
}
// ... and the buffers of a call on it: the first stage's list, its state words, the query's D
static size_t q41_call_bytes(int32_t dim) {
    return (size_t)COARSE_CAP * sizeof(uint32_t) + Q41_STATE_WORDS * sizeof(unsigned) + (size_t)dim * sizeof(int32_t);
}
#define SSW_PLAIN_BUILD(launch)                                                                                  \
    [](const void *X, int32_t dtype, int64_t n, int32_t dim, const Shadow &s, hipStream_t stream) -> ssw_status { \
        return launch(X, dtype, n, dim, s.codes, s.scale, s.err, stream);                                        \
    }
static const ShadowDesc SHADOW[4] = {
    {q8_dim_supported, [](int64_t n, int32_t dim) { return (size_t)n * dim; }, [](int64_t n) { return n; }, nullptr,
     SSW_PLAIN_BUILD(launch_q8_build), &Shadow::err, false},
    {q6_dim_supported, q6_code_bytes, packed_padded_rows, nullptr, SSW_PLAIN_BUILD(launch_q6_build), &Shadow::err, true},
    // (the 6-bit query's words and operand)
    {q5_dim_supported, q5_code_bytes, packed_padded_rows, nullptr, SSW_PLAIN_BUILD(launch_q5_build), &Shadow::err, true},
    // codes: the coarse plane; the first stage's width is a4's, the refine reads a5 and s5 of the rows it bounds
    {q5_dim_supported, q41_coarse_bytes, packed_padded_rows, q41_extra_bytes,
     [](const void *X, int32_t dtype, int64_t n, int32_t dim, const Shadow &s, hipStream_t stream) -> ssw_status {
         return launch_q41_build(X, dtype, n, dim, s.codes, s.fine, s.scale, s.err, s.err4, stream);
     },
     &Shadow::err4, true},
};
#undef SSW_PLAIN_BUILD

// of launch_survivors_mq (the two-stage shadow's own passes: prune41_stage1, prune41_refine)
static int code_bits(ShadowKind kind) { return kind == SHADOW_Q8 ? 8 : kind == SHADOW_Q6 ? 6 : 5; }

static bool prune_forced_off() {
    static const bool v = getenv("SSW_TOPK_FULL_SCAN") != nullptr;  // A/B: every top-k runs the full f32 scan
    return v;
}

// MIN_ROWS' entry for the index, or the lab build's value in its place: ssw_tune_prune's min_rows is the int8 shadow's,
// for the single call and the batch; ssw_tune_prune6's is the 6-bit single call's alone (lowering it leaves the batch
// on the int8 shadow, or at dim 768, which has none, on the plain batch) and ssw_tune_prune6_batch's the 6-bit batch's
static int64_t prune_min_rows(const ssw_index *idx, ShadowKind kind, bool batch) {
    if (kind == SHADOW_Q5) return g_prune5_min_rows >= 0 ? g_prune5_min_rows : MIN_ROWS_Q5;  // ssw_tune_prune5's alone
    if (kind == SHADOW_Q41) return g_prune41_min_rows >= 0 ? g_prune41_min_rows : MIN_ROWS_Q41;  // ssw_tune_prune41's alone
    const int64_t lab = kind == SHADOW_Q8 ? g_prune_min_rows : batch ? g_prune6_batch_min_rows : g_prune6_min_rows;
    return lab >= 0 ? lab : MIN_ROWS[kind][batch][idx->dim == 768][idx->dtype == SSW_DTYPE_F16];
}

static bool prune_eligible_on(const ssw_index *idx, ShadowKind kind, bool batch) {
    return g_prune && (kind != SHADOW_Q6 || g_prune6) && (kind != SHADOW_Q5 || g_prune5) && (kind != SHADOW_Q41 || g_prune41) &&
           !prune_forced_off() &&
           idx->owns_X && !idx->rows_escaped && idx->n >= prune_min_rows(idx, kind, batch) && idx->n_images > 0 &&
           SHADOW[kind].dim_ok(idx->dim);
}
// the 5-bit shadow: single queries on f32 rows of an index that has no image map at the time of the call (its exact
// threshold reads rows out of the selection's keys); an index with a map keeps the 6-bit or int8 path
bool ssw::prune5_eligible(const ssw_index *idx) {
    return prune_eligible_on(idx, SHADOW_Q5, false) && idx->dtype == SSW_DTYPE_F32 && !idx->has_map;
}
// the two-stage shadow: the calls and indexes of the 5-bit shadow (its own switch and row count)
bool ssw::prune41_eligible(const ssw_index *idx) {
    return prune_eligible_on(idx, SHADOW_Q41, false) && idx->dtype == SSW_DTYPE_F32 && !idx->has_map;
}
int64_t ssw::prune41_coarse_cap() { return g_coarse_cap; }
bool ssw::prune_eligible(const ssw_index *idx) { return prune_eligible_on(idx, SHADOW_Q8, false); }
bool ssw::prune_batch_eligible(const ssw_index *idx) { return prune_eligible_on(idx, SHADOW_Q8, true); }
bool ssw::prune6_eligible(const ssw_index *idx) { return prune_eligible_on(idx, SHADOW_Q6, false); }
static bool prune6_batch_eligible(const ssw_index *idx) {
    return prune6_eligible(idx) && idx->n >= prune_min_rows(idx, SHADOW_Q6, true);
}

// the rows are about to change: the buffer keeps the scores of the rows it was computed from, the shadow goes stale
ssw_status ssw::rows_changing(ssw_index *idx) {
    SSW_TRY(ensure_full_scores(idx));
    for (Shadow &s : idx->prune.sh) s.stale = true, s.refused = false;
    return SSW_OK;
}

// the buffers of one pruned call, whichever shadow it scans
static ssw_status ensure_call_buffers(ssw_index *idx) {
    PruneState &p = idx->prune;
    // each under its own test: a call that failed part-way is completed by the next one
    if (!p.state) SSW_HIP_TRY(hipMalloc((void **)&p.state, 4 * sizeof(unsigned)));
    if (!p.surv_rows) SSW_HIP_TRY(hipMalloc((void **)&p.surv_rows, (size_t)SURV_CAP * sizeof(int64_t)));
    if (!p.surv_scores) SSW_HIP_TRY(hipMalloc((void **)&p.surv_scores, (size_t)SURV_CAP * sizeof(float)));
    if (!p.q_last) SSW_HIP_TRY(hipMalloc((void **)&p.q_last, (size_t)idx->dim * sizeof(float)));
    if (!p.host) {
        SSW_HIP_TRY(hipHostMalloc((void **)&p.host, 16, hipHostMallocMapped | hipHostMallocCoherent));
        memset(p.host, 0, 16);
    }
    if (!p.ev) SSW_HIP_TRY(hipEventCreateWithFlags(&p.ev, hipEventDisableTiming));
    return SSW_OK;
}

// does a shadow of `bytes` leave the reserve free, beside the buffers of a call?
static ssw_status shadow_fits(const ssw_index *idx, size_t bytes, bool *fits) {
    size_t free_b = 0, total_b = 0;
    SSW_HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    const size_t need = bytes + (size_t)SURV_CAP * 12 + ((size_t)idx->dim + 64) * sizeof(float);
    *fits = free_b >= need && free_b - need >= (size_t)g_prune_reserve;
    return SSW_OK;
}

// The shadow `kind` of the rows for the pruned scan: (re)built when stale, if the device keeps PRUNE_RESERVE free beside
// it.  A refusal for memory holds until the rows change.
ssw_status ssw::ensure_shadow(ssw_index *idx, ShadowKind kind, bool *ready) {
    PruneState &p = idx->prune;
    Shadow &s = p.sh[kind];
    const ShadowDesc &desc = SHADOW[kind];
    *ready = false;
    if (s.codes && !s.stale) {
        *ready = true;
        return SSW_OK;
    }
    if (s.refused) return SSW_OK;
    if (!s.codes) {
        const size_t codes = desc.code_bytes(idx->n, idx->dim), consts = (size_t)desc.const_rows(idx->n) * sizeof(float);
        const bool two = desc.extra_bytes != nullptr;  // the two-stage shadow: its planes, and the buffers of a call on it
        const size_t extra = two ? desc.extra_bytes(idx->n, idx->dim) + (p.coarse_rows ? 0 : q41_call_bytes(idx->dim)) : 0;
        bool fits = false;
        SSW_TRY(shadow_fits(idx, codes + 2 * consts + extra, &fits));
        if (!fits) {
            s.refused = true;
            return SSW_OK;
        }
        bool got = hipMalloc((void **)&s.codes, codes) == hipSuccess && hipMalloc((void **)&s.scale, consts) == hipSuccess &&
                   hipMalloc((void **)&s.err, consts) == hipSuccess;
        if (got && two)
            got = hipMalloc((void **)&s.err4, consts) == hipSuccess && hipMalloc((void **)&s.H, consts) == hipSuccess &&
                  hipMalloc((void **)&s.fine, q41_fine_bytes(idx->n, idx->dim)) == hipSuccess &&
                  (p.cstate || hipMalloc((void **)&p.cstate, Q41_STATE_WORDS * sizeof(unsigned)) == hipSuccess) &&
                  (p.coarse_rows || hipMalloc((void **)&p.coarse_rows, (size_t)COARSE_CAP * sizeof(uint32_t)) == hipSuccess) &&
                  (p.D41 || hipMalloc((void **)&p.D41, (size_t)idx->dim * sizeof(int32_t)) == hipSuccess);
        if (!got) {  // (a call buffer that was had stays for the next attempt: each is under its own test)
            (void)hipGetLastError();
            s.free();
            s.refused = true;
            return SSW_OK;
        }
    }
    // each buffer under its own test: a call that failed part-way is completed by the next one
    SSW_TRY(ensure_call_buffers(idx));
    if (desc.query_operand && !p.state6) SSW_HIP_TRY(hipMalloc((void **)&p.state6, (size_t)Q8_MQ_WORDS * sizeof(unsigned)));
    if (desc.query_operand && !p.planes6) {
        SSW_HIP_TRY(hipMalloc((void **)&p.planes6, q6_plane_bytes(idx->dim)));
        // columns 2 .. 15 of the query operand stay zero for good: k_q6_query writes columns 0 and 1 only
        SSW_HIP_TRY(hipMemsetAsync(p.planes6, 0, q6_plane_bytes(idx->dim), idx->stream));
    }
    if (!s.max) SSW_HIP_TRY(hipMalloc((void **)&s.max, SHADOW_MAX_WORDS * sizeof(unsigned)));
    SSW_TRY(desc.build(idx->X, idx->dtype, idx->n, idx->dim, s, idx->stream));
    SSW_TRY(launch_shadow_max(s.*desc.width_err, s.scale, idx->n, s.max, idx->device, idx->stream));
    s.stale = false;
    *ready = true;
    return SSW_OK;
}

// The two steps of the pre-scan that the lab hooks (ssw_debug_prune_*, ssw_debug_prune6_*) drive as well; the shadow
// `kind` is ready.  Lower bounds of the scores of q_dev into the buffer, which is partial from here on: a consumer
// rescans q_last.  dbg_I: of the 6-bit scan (lab hook only).
ssw_status ssw::prune_bounds(ssw_index *idx, ShadowKind kind, const float *q_dev, int64_t *dbg_I) {
    PruneState &p = idx->prune;
    const Shadow &s = p.sh[kind];
    if (kind == SHADOW_Q41) {  // the first stage: lb4 into the buffer, H beside the shadow (dbg_I: not this scan's)
        SSW_TRY(launch_q41_query(q_dev, idx->dim, p.state6, p.planes6, p.q_last, p.D41, p.cstate, idx->stream));
        SSW_TRY(launch_q4_bounds(s.codes, s.scale, s.err4, p.planes6, p.state6, idx->scores, s.H, idx->n, idx->dim, idx->device,
                                 idx->stream));
    } else if (kind == SHADOW_Q5) {
        SSW_TRY(launch_q6_query(q_dev, idx->dim, p.state6, p.planes6, p.q_last, idx->stream));
        SSW_TRY(launch_q5_bounds(s.codes, s.scale, s.err, p.planes6, p.state6, idx->scores, idx->n, idx->dim, dbg_I,
                                 idx->device, idx->stream));
    } else if (kind == SHADOW_Q6) {
        SSW_TRY(launch_q6_query(q_dev, idx->dim, p.state6, p.planes6, p.q_last, idx->stream));
        SSW_TRY(launch_q6_bounds(s.codes, s.scale, s.err, p.planes6, p.state6, idx->scores, idx->n, idx->dim, dbg_I,
                                 idx->device, idx->stream));
    } else {
        SSW_TRY(launch_q8_query(q_dev, idx->dim, p.q_last, p.state, idx->stream));
        SSW_TRY(launch_q8_bounds(s.codes, s.scale, s.err, p.q_last, p.state, idx->scores, idx->n, idx->dim, idx->device,
                                 idx->stream));
    }
    idx->scores_partial = true;
    return SSW_OK;
}

// The rows that may still reach the k-th key of the last selection, at most cap of them -> *out_m = their published
// count, -1 = run the full scan.  One host wait: a sleep on sleep_ev_or_null first, then a spin.  The bounds in the
// buffer are the shadow `kind`'s: the 6-bit query is a chunk of one slot (width (***) of prune.hip).
ssw_status ssw::prune_survivors(ssw_index *idx, ShadowKind kind, int32_t k, int64_t cap, hipEvent_t sleep_ev_or_null,
                                int32_t *out_m) {
    PruneState &p = idx->prune;
    const Shadow &s = p.sh[kind];
    const unsigned seq = next_seq(p.seq);
    int32_t *host_dev = nullptr;
    SSW_HIP_TRY(hipHostGetDevicePointer((void **)&host_dev, p.host, 0));
    if (kind == SHADOW_Q41) {
        // both stages on the device, no wait between them: the first stage's survivors, then their 5-bit bounds
        SSW_TRY(prune41_stage1(idx, k, 0));
        SSW_TRY(prune41_refine(idx, k, nullptr, cap, nullptr, nullptr));
        SSW_TRY(launch_prune_publish_q41(p.state6, p.cstate, cap, host_dev, seq, idx->stream));
    } else if (kind != SHADOW_Q8) {
        SSW_TRY(launch_survivors_mq(idx->scores, s.err, s.scale, s.max, idx->n, idx->dim, code_bits(kind), idx->ws.out_keys,
                                    idx->ws.out_count, k, p.state6, p.surv_rows, cap, idx->device, idx->stream));
        SSW_TRY(launch_prune_publish_mq(p.state6, 1, cap, host_dev, seq, idx->stream));
    } else {
        SSW_TRY(launch_survivors(idx->scores, s.err, s.max, idx->n, idx->ws.out_keys, idx->ws.out_count, k, p.state, p.surv_rows,
                                 cap, host_dev, seq, idx->device, idx->stream));
    }
    if (sleep_ev_or_null) SSW_HIP_TRY(hipEventSynchronize(sleep_ev_or_null));
    SSW_TRY(wait_host_seq(idx->stream, reinterpret_cast<const unsigned *>(p.host), seq));
    *out_m = __atomic_load_n(p.host + 1, __ATOMIC_ACQUIRE);
    if (kind == SHADOW_Q41) {
        p.coarse_last = __atomic_load_n(p.host + 2, __ATOMIC_ACQUIRE);
        p.dense_refines += __atomic_load_n(p.host + 3, __ATOMIC_ACQUIRE) != 0 ? 1 : 0;
        ++p.two_stage_calls;
    }
    return SSW_OK;
}

// The two device steps of the two-stage shadow's survivors, which the lab hooks drive one at a time as well; lb4 of the
// kept query is in the buffer and H beside the shadow (prune_bounds).  Stage 1: the rows whose coarse upper bound reaches
// the k-th key, into the 32-bit list.  blocks: 0 = the pass's own grid (lab hook: one block walks many stages).
ssw_status ssw::prune41_stage1(ssw_index *idx, int32_t k, int blocks) {
    PruneState &p = idx->prune;
    const Shadow &s = p.sh[SHADOW_Q41];
    return launch_survivors_q4(idx->scores, s.err4, s.scale, s.max, idx->n, idx->dim, idx->ws.out_keys, idx->ws.out_count, k,
                               p.state6, p.cstate, p.coarse_rows, COARSE_CAP, blocks, idx->device, idx->stream);
}
// Refine: the 5-bit bound of the listed rows (the first stage's list, or the lab hook's), or of every row when the list
// holds more than the coarse cap; its survivors into surv_rows, counted in state6[0]
ssw_status ssw::prune41_refine(ssw_index *idx, int32_t k, const uint32_t *list_or_null, int64_t cap, float *dbg_lb5,
                               int32_t *dbg_B) {
    PruneState &p = idx->prune;
    const Shadow &s = p.sh[SHADOW_Q41];
    return launch_q41_refine(s.H, s.fine, s.scale, s.err, p.D41, idx->ws.out_keys, k, p.state6, p.cstate,
                             list_or_null ? list_or_null : p.coarse_rows, std::min(g_coarse_cap, COARSE_CAP), idx->n, idx->dim,
                             p.surv_rows, cap, dbg_lb5, dbg_B, idx->device, idx->stream);
}

// The exact threshold of the 5-bit path, between the threshold selection of kc keys and the survivor pass, all on the
// device: the keys' rows, their exact scores for the kept query, and the k-th key raised to the k-th of those scores
// (prune.hip, "the exact threshold").  The survivor list and its scores are free until the survivor pass.
ssw_status ssw::prune_exact_threshold(ssw_index *idx, int32_t k, int32_t kc) {
    PruneState &p = idx->prune;
    SSW_TRY(launch_candidate_rows(idx->ws.out_keys, idx->ws.out_count, kc, idx->n, p.surv_rows, idx->stream));
    SSW_TRY(launch_score_rows(idx->X, idx->dtype, p.q_last, p.surv_rows, kc, idx->dim, p.surv_scores, idx->stream));
    return launch_exact_threshold(idx->ws.out_keys, idx->ws.out_count, p.surv_scores, k, kc, idx->stream);
}

// The score buffer for the selection of the top-k of query q_dev (exclusions installed): the full f32 scan, or on a
// large index the certified pre-scan -- shadow scan (lower bounds), threshold selection over them that publishes
// nothing, survivors, exact rescoring of the survivors.  One host wait for the survivor count; any failure of the
// certificate (fewer than k keys or an overflow in the threshold selection, more survivors than SURV_CAP, a query
// that cannot be bounded) runs the full scan instead.  The profiling events bracket the whole replacement.
// The shadow is the 6-bit one where prune6_eligible says so (only that one is built then), else the int8 one; a 6-bit
// shadow refused for memory leaves the int8 path, if an int8 shadow exists or fits.  A dim-768 index is never
// prune_eligible (no int8 shadow at that dim): it reaches the 6-bit shadow or the full scan.
// *out_candidates: the pruned path succeeded on an index without an image map, and the candidates of the final top-k
// are in the selection's workspace (launch_scatter_candidates): the caller's selection, the next thing on the stream,
// runs over them alone (do_select, from_candidates).  Nothing of it is kept in the handle.
// The 5-bit shadow comes first where prune5_eligible says so (and then no 6-bit shadow is built for single queries; a
// refusal for memory falls through to the 6-bit and then the int8 shadow).  Its bounds are twice as wide, so its
// threshold selection runs for kc = min(SSW_MAX_TOPK, max(1024, 4 k)) keys and prune_exact_threshold raises the k-th key
// to the k-th exact score of those candidates before the survivor pass, on the device; everything after is the same.
// Ahead of it, where prune41_eligible says so, comes the two-stage form of the same codes (and then no packed 5-bit shadow
// is built; a refusal for memory falls through to it): the scan bounds every row on the 4-bit plane, the selection and
// the exact threshold run as for the 5-bit shadow, and prune_survivors enqueues both survivor stages (prune41_stage1,
// prune41_refine) ahead of the one host wait; what it publishes are the rows that survive the 5-bit bound.
ssw_status ssw::scan_for_topk(ssw_index *idx, const float *q_dev, int32_t k, bool *out_candidates) {
    *out_candidates = false;
    bool ready = false;
    ShadowKind kind = SHADOW_Q41;
    const bool k_ok = k >= 1 && k <= SSW_MAX_TOPK && (idx->ws.xchg.msg_out == nullptr || k <= idx->ws.xchg.k_max);
    const int32_t kc = std::min<int32_t>(SSW_MAX_TOPK, std::max<int32_t>(1024, 4 * std::min<int32_t>(k, SSW_MAX_TOPK)));
    if (k_ok && prune41_eligible(idx)) SSW_TRY(ensure_shadow(idx, kind, &ready));
    if (k_ok && !ready && prune5_eligible(idx)) {
        kind = SHADOW_Q5;
        SSW_TRY(ensure_shadow(idx, kind, &ready));
    }
    if (k_ok && !ready && prune6_eligible(idx)) {
        kind = SHADOW_Q6;
        SSW_TRY(ensure_shadow(idx, kind, &ready));
    }
    if (k_ok && !ready && prune_eligible(idx)) {
        kind = SHADOW_Q8;
        SSW_TRY(ensure_shadow(idx, kind, &ready));
    }
    if (!ready) return do_scan(idx, q_dev);
    SSW_TRY(ensure_ws(idx));
    return profiled(idx, [&]() -> ssw_status {
        PruneState &p = idx->prune;
        SSW_TRY(prune_bounds(idx, kind, q_dev, nullptr));
        SSW_HIP_TRY(hipEventRecord(p.ev, idx->stream));
        // threshold: the ordinary selection over the lower bounds, with the exclusions, without a message or host result
        const bool exact_t = kind == SHADOW_Q5 || kind == SHADOW_Q41;  // the wide bounds: kc keys, the exact threshold
        SSW_TRY(do_select(idx, idx->scores, exact_t ? kc : k, SelectDest{nullptr, 0u, false}, idx->stream));
        // (ahead of the host wait; the survivor pass reads the selection's keys and count, not these words)
        if (!idx->has_map) SSW_TRY(select_reset_state(idx->ws, idx->stream));
        if (exact_t) SSW_TRY(prune_exact_threshold(idx, k, kc));
        int32_t m = -1;
        // (the two-stage path's final survivors are held to ssw_tune_surv_cap's value in the lab build: SURV_CAP unless set)
        const int64_t cap = kind == SHADOW_Q41 ? std::min<int64_t>(SURV_CAP, g_surv_cap_dev) : SURV_CAP;
        SSW_TRY(prune_survivors(idx, kind, k, cap, p.ev, &m));  // sleep through the shadow scan, spin on the rest
        p.last = m;
        ++p.queries;
        if (m < 0) {
            ++p.fallbacks;
            idx->scores_partial = false;
            return launch_index_scan(idx, p.q_last, idx->stream);
        }
        SSW_TRY(launch_score_rows(idx->X, idx->dtype, p.q_last, p.surv_rows, m, idx->dim, p.surv_scores, idx->stream));
        if (idx->has_map) return launch_scatter_scores(p.surv_rows, p.surv_scores, m, idx->scores, idx->stream);
        *out_candidates = m > 0;
        return launch_scatter_candidates(idx->ws, p.surv_rows, p.surv_scores, m, k, idx->scores, idx->stream);
    });
}

// "make dst[rows] exact for query q_dev": the scan's bits of the m listed rows (any rows of the index, repeats allowed)
// into vals_dev and from there into dst, the handle's buffer or a slab of a chunk.  What a second-stage reader of a
// partial buffer runs on the rows it is about to read, instead of the full scan; an exact value over a lower bound or
// over itself changes nothing for anybody else.
ssw_status ssw::rescore_rows(ssw_index *idx, const float *q_dev, const int64_t *rows_dev, float *vals_dev, int64_t m,
                             float *dst, hipStream_t stream) {
    SSW_TRY(launch_score_rows(idx->X, idx->dtype, q_dev, rows_dev, m, idx->dim, vals_dev, stream));
    SSW_TRY(launch_scatter_scores(rows_dev, vals_dev, m, dst, stream));
    idx->prune.rescored_rows += m;
    return SSW_OK;
}

// ---- the pruned batch: ONE pass over the int8 or the 6-bit shadow bounds a chunk of up to 16 queries (prune.hip,
// "Pruned batch") ----
static_assert(BATCH_MAX_WIDTH == Q8_MQ_WIDTH, "a chunk of the pruned batch uses the batch's slabs");

// the state of a chunk of w queries; the survivor lists may only be had for fewer slots: *out_w
ssw_status ssw::ensure_prune_batch(ssw_index *idx, int w, int *out_w) {
    PruneBatchState &pb = idx->prune_batch;
    if (!pb.mq) {
        SSW_HIP_TRY(hipMalloc((void **)&pb.mq, (size_t)Q8_MQ_WIDTH * Q8_MQ_WORDS * sizeof(unsigned)));
        SSW_HIP_TRY(hipMemsetAsync(pb.mq, 0, (size_t)Q8_MQ_WIDTH * Q8_MQ_WORDS * sizeof(unsigned), idx->stream));
        SSW_HIP_TRY(hipMalloc((void **)&pb.planes, q8_mq_plane_bytes(idx->dim)));
        SSW_HIP_TRY(hipHostMalloc((void **)&pb.host, (1 + Q8_MQ_WIDTH) * sizeof(int32_t),
                                  hipHostMallocMapped | hipHostMallocCoherent));
        memset(pb.host, 0, (1 + Q8_MQ_WIDTH) * sizeof(int32_t));
    }
    while (pb.slots < w) {  // grow; on failure keep halving the width
        SSW_HIP_TRY(hipStreamSynchronize(idx->stream));
        (void)hipFree(pb.surv_rows);
        (void)hipFree(pb.surv_scores);
        pb.surv_rows = nullptr;
        pb.surv_scores = nullptr;
        pb.slots = 0;
        if (hipMalloc((void **)&pb.surv_rows, (size_t)w * SURV_CAP * sizeof(int64_t)) == hipSuccess &&
            hipMalloc((void **)&pb.surv_scores, (size_t)w * SURV_CAP * sizeof(float)) == hipSuccess) {
            pb.slots = w;
        } else {
            (void)hipGetLastError();
            (void)hipFree(pb.surv_rows);
            pb.surv_rows = nullptr;
            pb.surv_scores = nullptr;
            if (w == 1) {
                set_error("topk_batch_pruned: no memory for one survivor list");
                return SSW_ERR_NOMEM;
            }
            w >>= 1;
        }
    }
    *out_w = w;
    return SSW_OK;
}

// The shadow that bounds the chunks of a pruned batch, made ready: the single call's rule (scan_for_topk).  The 6-bit one
// where prune6_eligible says so and the index has the batch's rows for it (only that one is built then); else, and
// where the 6-bit shadow is refused for memory, the int8 one under prune_batch_eligible.  prune_batch.kind remembers
// the choice for the steps below.  *ready false: the batch is the plain one -- at dim 768, which has no int8 fallback,
// whenever the index is below the batch's 6-bit constant or the 6-bit shadow was refused.
ssw_status ssw::prune_batch_shadow(ssw_index *idx, bool *ready) {
    *ready = false;
    ShadowKind kind = SHADOW_Q6;
    if (prune6_batch_eligible(idx)) SSW_TRY(ensure_shadow(idx, kind, ready));
    if (!*ready && prune_batch_eligible(idx)) {
        kind = SHADOW_Q8;
        SSW_TRY(ensure_shadow(idx, kind, ready));
    }
    if (*ready) idx->prune_batch.kind = kind;
    return SSW_OK;
}

// The two device steps of a chunk that the lab hooks drive as well; the shadow prune_batch.kind names and the chunk's
// buffers are ready and the w queries are in batch.qb_dev.  Lower bounds of query j into slab j; the handle's buffer
// (the last query's slab) is partial from here on and q_last is the last query.  dbg_hi / dbg_lo: of the int8 chunk,
// dbg_I: of the 6-bit chunk (lab hooks only).
ssw_status ssw::prune_bounds_mq(ssw_index *idx, int w, int32_t *dbg_hi, int32_t *dbg_lo, int64_t *dbg_I) {
    PruneState &p = idx->prune;
    PruneBatchState &pb = idx->prune_batch;
    const Shadow &s = p.sh[pb.kind];
    if (pb.kind == SHADOW_Q6) {
        SSW_TRY(launch_q6_query_mq(idx->batch.qb_dev, idx->dim, w, pb.mq, pb.planes, p.q_last, idx->stream));
        SSW_TRY(launch_q6_bounds_mq(s.codes, s.scale, s.err, pb.planes, pb.mq, w, idx->batch.side, slab_stride(idx),
                                    idx->scores, idx->n, idx->dim, dbg_I, idx->device, idx->stream));
    } else {
        SSW_TRY(launch_q8_query_mq(idx->batch.qb_dev, idx->dim, w, pb.mq, pb.planes, p.q_last, idx->stream));
        SSW_TRY(launch_q8_bounds_mq(s.codes, s.scale, s.err, pb.planes, pb.mq, w, idx->batch.side, slab_stride(idx),
                                    idx->scores, idx->n, idx->dim, dbg_hi, dbg_lo, idx->device, idx->stream));
    }
    idx->scores_partial = true;
    return SSW_OK;
}

// the survivors of slot j against the keys the last selection left, into the slot's list (no publish)
ssw_status ssw::prune_survivors_slot(ssw_index *idx, int w, int j, int32_t k, int64_t cap) {
    PruneBatchState &pb = idx->prune_batch;
    const Shadow &s = idx->prune.sh[pb.kind];
    return launch_survivors_mq(chunk_slab(idx, w, j), s.err, s.scale, s.max, idx->n, idx->dim, code_bits(pb.kind),
                               idx->ws.out_keys, idx->ws.out_count, k, pb.mq + j * Q8_MQ_WORDS, pb.surv_rows + (int64_t)j * SURV_CAP, cap, idx->device,
                               idx->stream);
}

// every slot's count (or -1) of the chunk -> out_m[w]; ONE host wait: a sleep on sleep_ev_or_null first, then a spin
ssw_status ssw::prune_publish_mq(ssw_index *idx, int w, int64_t cap, hipEvent_t sleep_ev_or_null, int32_t *out_m) {
    PruneBatchState &pb = idx->prune_batch;
    const unsigned seq = next_seq(pb.seq);
    int32_t *host_dev = nullptr;
    SSW_HIP_TRY(hipHostGetDevicePointer((void **)&host_dev, pb.host, 0));
    SSW_TRY(launch_prune_publish_mq(pb.mq, w, cap, host_dev, seq, idx->stream));
    if (sleep_ev_or_null) SSW_HIP_TRY(hipEventSynchronize(sleep_ev_or_null));
    SSW_TRY(wait_host_seq(idx->stream, reinterpret_cast<const unsigned *>(pb.host), seq));
    for (int j = 0; j < w; ++j) out_m[j] = __atomic_load_n(pb.host + 1 + j, __ATOMIC_ACQUIRE);
    return SSW_OK;
}

// ---- the chunk that never waits (ssw_index_topk_batch_dev_pruned, index_batch.hip) ------------------------------------
int64_t ssw::batch_dev_surv_cap() { return g_surv_cap_dev; }

// exact scores of the survivors of every certified slot of the chunk of w, straight into the slabs: ONE launch, sized
// without a count from the device (rescore_dev.hip); the lab hook drives it as well
ssw_status ssw::rescore_survivors_chunk(ssw_index *idx, int w, int64_t cap) {
    PruneBatchState &pb = idx->prune_batch;
    return launch_rescore_survivors(idx->X, idx->dtype, idx->batch.qb_dev, pb.mq, pb.surv_rows, SURV_CAP, cap, w,
                                    idx->batch.side, slab_stride(idx), idx->scores, idx->n, idx->dim, idx->device,
                                    idx->stream);
}

extern "C" {

ssw_status ssw_index_prune_batch_dev_read(ssw_index *idx, int32_t *out32, int32_t *out_w) {
    SSW_REQUIRE(idx != nullptr && out32 != nullptr && out_w != nullptr, "NULL argument");
    const PruneBatchState &pb = idx->prune_batch;
    *out_w = 0;
    if (pb.dev_w <= 0 || !pb.mq) return SSW_OK;
    DeviceGuard guard(idx->device);
    unsigned mq[Q8_MQ_WIDTH * Q8_MQ_WORDS];
    SSW_HIP_TRY(hipMemcpyAsync(mq, pb.mq, sizeof(mq), hipMemcpyDeviceToHost, idx->stream));
    SSW_HIP_TRY(hipStreamSynchronize(idx->stream));
    for (int j = 0; j < pb.dev_w; ++j) {
        const unsigned *st = mq + j * Q8_MQ_WORDS;
        out32[2 * j] = (int32_t)st[0];
        out32[2 * j + 1] = (st[5] != 0u ? 1 : 0) | (st[2] != 0u ? 2 : 0) | ((int64_t)st[0] > pb.dev_cap ? 4 : 0);
    }
    *out_w = pb.dev_w;
    return SSW_OK;
}

ssw_status ssw_index_prune_stats(ssw_index *idx, int64_t *out6) {
    SSW_REQUIRE(idx != nullptr && out6 != nullptr, "NULL argument");
    const PruneState &p = idx->prune;
    // the state of the shadow single queries use: the 6-bit one where it applies and was not refused
    // (a dim-768 index has no other: there a refusal is the 6-bit shadow's)
    const Shadow &q8 = p.sh[SHADOW_Q8], &q6 = p.sh[SHADOW_Q6], &q5 = p.sh[SHADOW_Q5], &q41 = p.sh[SHADOW_Q41];
    const bool six = prune6_eligible(idx) && (!q6.refused || !q8_dim_supported(idx->dim));
    const bool five = prune5_eligible(idx) && !q5.refused;  // ... and before it the 5-bit one, on the same terms
    const bool two = prune41_eligible(idx) && !q41.refused;  // ... and before that the two-stage one
    const Shadow &s = two ? q41 : five ? q5 : six ? q6 : q8;
    out6[0] = s.codes ? (s.stale ? 2 : 1) : (s.refused ? 3 : 0);
    out6[1] = prune_eligible(idx) || six || five || two ? 1 : 0;
    out6[2] = p.last;
    out6[3] = p.queries;
    out6[4] = p.fallbacks;
    out6[5] = (q8.codes ? idx->n * (idx->dim + 8) : 0) + (q6.codes ? packed_padded_rows(idx->n) * (idx->dim * 3 / 4 + 8) : 0) +
              (q5.codes ? packed_padded_rows(idx->n) * (idx->dim * 5 / 8 + 8) : 0) +
              (q41.codes ? packed_padded_rows(idx->n) * (idx->dim * 5 / 8 + 16) : 0);  // both planes, s5, a5, a4, H
    return SSW_OK;
}

ssw_status ssw_index_prune_coarse_stats(ssw_index *idx, int64_t *out3) {
    SSW_REQUIRE(idx != nullptr && out3 != nullptr, "NULL argument");
    out3[0] = idx->prune.coarse_last;
    out3[1] = idx->prune.dense_refines;
    out3[2] = idx->prune.two_stage_calls;
    return SSW_OK;
}

ssw_status ssw_index_prune_completions(ssw_index *idx, int64_t *out2) {
    SSW_REQUIRE(idx != nullptr && out2 != nullptr, "NULL argument");
    out2[0] = idx->prune.completions;
    out2[1] = idx->prune.rescored_rows;
    return SSW_OK;
}

#ifdef SSW_DEBUG_HOOKS
ssw_status ssw_tune_prune(int32_t enable, int64_t min_rows, int64_t reserve_bytes) {
    g_prune = enable != 0;
    g_prune_min_rows = min_rows < 0 ? -1 : min_rows;  // < 0: MIN_ROWS' entries again
    g_prune_reserve = reserve_bytes < 0 ? PRUNE_RESERVE : reserve_bytes;
    return SSW_OK;
}

ssw_status ssw_tune_surv_cap(int64_t cap) {
    g_surv_cap_dev = cap >= 1 && cap <= SURV_CAP ? cap : SURV_CAP;
    return SSW_OK;
}

ssw_status ssw_tune_prune_scan(int32_t blocks_per_cu, int32_t group_loads) {
    tune_q8_bounds(blocks_per_cu, group_loads);
    return SSW_OK;
}

ssw_status ssw_tune_prune6(int32_t enable, int64_t min_rows) {
    g_prune6 = enable != 0;
    g_prune6_min_rows = min_rows < 0 ? -1 : min_rows;  // < 0: MIN_ROWS' entries again
    return SSW_OK;
}

ssw_status ssw_tune_prune5(int32_t enable, int64_t min_rows) {
    g_prune5 = enable != 0;
    g_prune5_min_rows = min_rows < 0 ? -1 : min_rows;  // < 0: MIN_ROWS_Q5 again
    return SSW_OK;
}

ssw_status ssw_tune_prune41(int32_t enable, int64_t min_rows, int64_t coarse_cap) {
    g_prune41 = enable != 0;
    g_prune41_min_rows = min_rows < 0 ? -1 : min_rows;  // < 0: MIN_ROWS_Q41 again
    g_coarse_cap = coarse_cap >= 0 && coarse_cap <= COARSE_CAP ? coarse_cap : COARSE_CAP;
    return SSW_OK;
}

ssw_status ssw_tune_prune41_scan(int32_t blocks_per_cu, int32_t tiles) {
    tune_tile_scan(SCAN_Q4, blocks_per_cu, tiles);
    return SSW_OK;
}

ssw_status ssw_tune_prune5_scan(int32_t blocks_per_cu, int32_t tiles) {
    tune_tile_scan(SCAN_Q5, blocks_per_cu, tiles);
    return SSW_OK;
}

ssw_status ssw_tune_prune6_batch(int64_t min_rows) {
    g_prune6_batch_min_rows = min_rows < 0 ? -1 : min_rows;  // < 0: MIN_ROWS' entries again
    return SSW_OK;
}

ssw_status ssw_tune_prune6_scan(int32_t blocks_per_cu, int32_t tiles) {
    tune_tile_scan(SCAN_Q6, blocks_per_cu, tiles);
    return SSW_OK;
}

ssw_status ssw_tune_prune_scan_mq(int32_t blocks_per_cu, int32_t tiles) {
    tune_tile_scan(SCAN_Q8_MQ, blocks_per_cu, tiles);
    return SSW_OK;
}

ssw_status ssw_tune_prune6_scan_mq(int32_t blocks_per_cu, int32_t tiles) {
    tune_tile_scan(SCAN_Q6_MQ, blocks_per_cu, tiles);
    return SSW_OK;
}
#endif

}  // extern "C"

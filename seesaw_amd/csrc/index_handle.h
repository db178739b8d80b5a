// index_handle.h -- the resident index's handle and the host helpers shared by the sources of its C-ABI: capi_index.hip,
// index_topk.hip, index_prune.hip, index_batch.hip and, in the lab build, debug_hooks.hip.
#pragma once
#include "ssw_common.h"

constexpr int BATCH_MAX_WIDTH = 16;                 // queries of one chunk of a batch (index_batch.hip)
constexpr int64_t SURV_CAP = (int64_t)1 << 18;      // survivors rescored at most; more: the full scan
constexpr int64_t SMALL_EXCL_CAP = 8192;            // the small form (index_topk.hip): excluded ids in its pinned block
constexpr int64_t SMALL_ROWS = 65536;               // and the small scan kernel's range (scan.hip)

// a shadow of the rows for the certified pre-scan of the top-k (prune.hip): the int8 one, and the packed 6-bit one that
// single queries scan instead on an index of enough rows, and the packed 5-bit one that single queries on a still larger
// f32 index without an image map scan instead of that (index_prune.hip, MIN_ROWS, MIN_ROWS_Q5).  Each is built lazily by
// the first top-k with a query that wants it after the rows last changed
// SHADOW_Q41: the 5-bit codes as a 4-bit plane every row is scanned on and a 1-bit plane read for the survivors of that
// scan alone (prune.hip, "two-stage 4 + 1-bit shadow"); where it applies (MIN_ROWS_Q41) no packed 5-bit shadow is built
enum ShadowKind { SHADOW_Q8, SHADOW_Q6, SHADOW_Q5, SHADOW_Q41 };
struct Shadow {
    unsigned char *codes = nullptr;               // int8: [n, dim] codes; 6-bit: q6_code_bytes(n, dim), tiles of 16 rows;
                                                  // 5-bit: q5_code_bytes(n, dim), tiles of 16 rows
    float *scale = nullptr, *err = nullptr;       // s_r, a_r: [n]; 6-bit, 5-bit: [packed_padded_rows(n)]
    unsigned *max = nullptr;                      // [SHADOW_MAX_WORDS] the largest finite a_r, s_r (launch_shadow_max);
                                                  // SHADOW_Q41: of a4_r, s5_r (the first stage's width)
    // SHADOW_Q41 only: codes is the coarse plane (q41_coarse_bytes), scale / err are s5 / a5, and beside them
    float *err4 = nullptr;                        // a4_r [packed_padded_rows(n)]
    int32_t *H = nullptr;                         // [packed_padded_rows(n)] the last first-stage scan's integer sums
    unsigned *fine = nullptr;                     // the fine plane (q41_fine_bytes)
    bool stale = true;                            // the rows changed since the shadow was built
    bool refused = false;                         // too little free memory at the last attempt (until the rows change)
    void free() {
        for (void *p : {(void *)codes, (void *)scale, (void *)err, (void *)err4, (void *)H, (void *)fine}) (void)hipFree(p);
        codes = nullptr;
        scale = err = err4 = nullptr;
        H = nullptr;
        fine = nullptr;
        stale = true;
    }
};

// the shadows and the buffers of one pruned call
struct PruneState {
    Shadow sh[4];                                  // by ShadowKind
    unsigned *state = nullptr;                     // [4] device words (ssw_common.h, launch_q8_query)
    int64_t *surv_rows = nullptr;                  // [SURV_CAP]
    float *surv_scores = nullptr;                  // [SURV_CAP]
    int32_t *host = nullptr;                       // pinned, mapped: [seq, survivors or -1]
    unsigned seq = 0;
    hipEvent_t ev = nullptr;                       // after the shadow scan: the host sleeps on it, then spins
    float *q_last = nullptr;                       // [dim] the query of the last pruned scan
    int64_t last = 0, queries = 0, fallbacks = 0;
    // ssw_index_prune_completions: full scans that completed a partial buffer or slab, rows rescored on demand instead
    int64_t completions = 0, rescored_rows = 0;
    // a single query on the 6-bit or the 5-bit shadow
    unsigned *state6 = nullptr;                    // [Q8_MQ_WORDS] the query's words, a slot's of the chunk
    int8_t *planes6 = nullptr;                     // q6_plane_bytes(dim): the query's operand
    // a single query on the two-stage shadow, beside those
    unsigned *cstate = nullptr;                    // [Q41_STATE_WORDS] the first stage's counter, the dense flag
    uint32_t *coarse_rows = nullptr;               // [COARSE_CAP] the first stage's survivors
    int32_t *D41 = nullptr;                        // [dim] the query's 256 d_hi + d_lo in natural order
    int64_t coarse_last = 0, dense_refines = 0, two_stage_calls = 0;  // ssw_index_prune_coarse_stats
    void free_shadow() {
        for (Shadow &s : sh) s.free();
    }
    void release() {
        for (Shadow &s : sh) {
            s.free();
            (void)hipFree(s.max);
        }
        for (void *p : {(void *)state, (void *)surv_rows, (void *)surv_scores, (void *)q_last, (void *)state6, (void *)planes6,
                        (void *)cstate, (void *)coarse_rows, (void *)D41})
            (void)hipFree(p);
        if (host) (void)hipHostFree(host);
        if (ev) (void)hipEventDestroy(ev);
    }
};

// pruned batch (ssw_index_topk_batch_pruned): the per-query state, query codes and survivor lists of one chunk of up to
// Q8_MQ_WIDTH queries; allocated by the first pruned batch
struct PruneBatchState {
    unsigned *mq = nullptr;        // [Q8_MQ_WIDTH][Q8_MQ_WORDS] (ssw_common.h)
    int8_t *planes = nullptr;      // q8_mq_plane_bytes(dim)
    int64_t *surv_rows = nullptr;  // [slots][SURV_CAP]
    float *surv_scores = nullptr;  // [slots][SURV_CAP]
    int slots = 0;
    // the shadow that bounds the chunk (prune_batch_shadow): the packed 6-bit one, else the int8 one.  The state words,
    // the planes and the slabs hold one chunk at a time, so only one shadow ever serves them
    ShadowKind kind = SHADOW_Q8;
    int32_t *host = nullptr;       // pinned, mapped: [seq, survivors or -1 of each slot]
    unsigned seq = 0;
    // the last chunk of ssw_index_topk_batch_dev_pruned, for ssw_index_prune_batch_dev_read: its width (0: the words
    // above are not such a chunk's) and the cap its slots were held to
    int dev_w = 0;
    int64_t dev_cap = 0;
    void release() {
        for (void *p : {(void *)mq, (void *)planes, (void *)surv_rows, (void *)surv_scores}) (void)hipFree(p);
        if (host) (void)hipHostFree(host);
    }
};

// batched scan (ssw_index_scan_batch / ssw_index_topk_batch): the queries of one chunk, and the score slabs of all but
// its last query (that one's slab is `scores`); allocated by the first batched call
struct BatchState {
    float *qb_dev = nullptr;  // [BATCH_MAX_WIDTH, dim]
    ssw::PinnedStage qb_stage;
    float *side = nullptr;    // [side_slabs, slab_stride]
    int side_slabs = 0;
    // second stage of a chunk (ssw_index_topk_batch_avg): [BATCH_MAX_WIDTH, SSW_MAX_TOPK] each
    float *avg_score = nullptr;
    int64_t *avg_row = nullptr;
    void release() {
        (void)hipFree(qb_dev);
        (void)hipFree(side);
        (void)hipFree(avg_score);
        (void)hipFree(avg_row);
        qb_stage.release();
    }
};

// ssw_index_stage2_pair_batch: one pinned host block and its device mirror, [inputs | outputs] of one call; allocated
// by the first call, grown by a larger one
struct PairStage {
    unsigned char *host = nullptr, *dev = nullptr;
    size_t cap = 0;
    void release() {
        if (host) (void)hipHostFree(host);
        (void)hipFree(dev);
        host = dev = nullptr;
        cap = 0;
    }
};

struct ssw_index {
    int device = 0;
    int64_t n = 0;
    int32_t dim = 0;
    int64_t n_images = 0;
    bool has_map = false;
    int32_t dtype = SSW_DTYPE_F32;
    float *X = nullptr;  // SSW_DTYPE_F16: binary16 rows in the lane-interleaved layout (ssw_common.h)
    bool owns_X = false;
    // a view (ssw_index_create_view): X is the parent's matrix and row j of the view is its row row_src[j].  Only the
    // scan (launch_index_scan) and the entries that translate staged view rows to parent rows on the host (stage_rows
    // with matrix_rows in capi_index.hip; index_view_rows in feedback.hip) read X of a view; every other reader of X
    // refuses it (refuse_view).  The parent counts its live views and is not destroyed before them
    ssw_index *parent = nullptr;
    int32_t *row_src = nullptr;         // [n] device
    std::vector<int32_t> row_src_host;  // its host mirror
    int64_t live_views = 0;
    // f16 upload / download: bounded device staging of natural-order rows (f32 or binary16)
    void *xfer = nullptr;
    size_t xfer_bytes = 0;
    float *scores = nullptr;      // [n]
    float *q_dev = nullptr;       // [dim] device copy of a host query
    ssw::PinnedStage q_stage;
    int64_t *row_start = nullptr;  // [n_images + 1] when has_map
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    ssw::SelectWorkspace ws;
    bool ws_ready = false;
    // the batched exchange target (ssw_index_set_exchange_target_batch): msg_out is slot 0 of [xchg_batch_slots, msg_len];
    // state of its own beside ws.xchg, written only by ssw_index_topk_batch_dev / ssw_index_topk_slot_deep_dev
    ssw::FinalExchange xchg_batch;
    int32_t xchg_batch_slots = 0;
    // gather staging
    int64_t *gather_idx = nullptr;
    float *gather_out = nullptr;
    int64_t gather_cap = 0;
    ssw::PinnedStage rows_stage;
    void *res_host = nullptr;  // pinned result mirror
    // small index (one scan launch + one selection launch, no copies, no stream wait): pinned, device-visible block
    // [query dim f32][excluded ids SMALL_EXCL_CAP i64][packed result], and the sequence number the host spins on
    unsigned char *small_host = nullptr;
    unsigned small_seq = 0;
    unsigned res_pending_seq = 0;  // != 0: the selection in flight publishes into res_host under this sequence number
    unsigned small_pending_seq = 0;  // the same for the small form, into small_host
    // batched graph round (index_enqueue_topk_slot): BATCH_MAX_WIDTH pinned, device-visible blocks, one a slot of a chunk,
    // [excluded ids SMALL_EXCL_CAP i64][packed result]; each slot's selection publishes into its own block
    unsigned char *slot_host = nullptr;
    float *q2_dev = nullptr;  // second query vector (score_rows)
    ssw::PinnedStage q2_stage;
    // tile geometry + staging of the avg_score aggregation (rescore.hip)
    std::vector<int64_t> row_start_host;  // host mirror of row_start
    int64_t max_image_tiles = -1;  // the most rows of one image; -1: not computed since the map was set
    float *tile_boxes = nullptr;   // [n, 4] x1, y1, x2, y2
    int32_t *tile_zoom = nullptr;  // [n]
    int64_t *rs_pos = nullptr, *rs_off = nullptr, *rs_row = nullptr;  // [rs_cap]
    float *rs_score = nullptr;     // [rs_cap]
    float *rs_minus = nullptr;     // [rs_minus_cap]
    int64_t rs_cap = 0, rs_minus_cap = 0;
    PruneState prune;           // never for a borrowed matrix or once ssw_index_device_ptrs handed out the rows
    bool rows_escaped = false;  // the row pointer was handed out: never a shadow
    // scores hold exact values for the survivors only: ensure_full_scores materialises, a second-stage reader makes the
    // rows it reads exact (rescore_rows) and leaves the buffer partial
    bool scores_partial = false;
    BatchState batch;
    PruneBatchState prune_batch;
    PairStage pair;
    // profiling of the scan kernel
    bool profiling = false;
    std::vector<hipEvent_t> ev;  // pairs
    int ev_used = 0;
};

// the second stage of a batch (ssw_index_topk_batch_avg): the aggregation code and the host outputs [nq, k]
struct AvgStage {
    int32_t aug;
    float *out_scores;
    int64_t *out_rows;
};

#pragma GCC visibility push(hidden)  // shared between the library's own sources, not exported from it
namespace ssw {

inline ssw_status ensure_ws(ssw_index *idx) {
    if (idx->ws_ready) return SSW_OK;
    SSW_TRY(select_alloc(idx->ws, idx->n, idx->n_images, idx->has_map));
    idx->ws_ready = true;
    return SSW_OK;
}

inline unsigned next_seq(unsigned &counter) {  // sequence numbers are never 0 ("nothing in flight")
    if (++counter == 0) ++counter;
    return counter;
}

// one pair of profiling events around `work`, the scan or whatever replaces it; none when fewer than two are left
template <class F>
static ssw_status profiled(ssw_index *idx, F work) {
    const bool prof = idx->profiling && idx->ev_used + 2 <= (int)idx->ev.size();
    if (prof) SSW_HIP_TRY(hipEventRecord(idx->ev[idx->ev_used], idx->stream));
    SSW_TRY(work());
    if (prof) {
        SSW_HIP_TRY(hipEventRecord(idx->ev[idx->ev_used + 1], idx->stream));
        idx->ev_used += 2;
    }
    return SSW_OK;
}

// capi_index.hip
ssw_status check_query(const ssw_index *idx, const float *q_host);
ssw_status check_excluded(const ssw_index *idx, const int64_t *ids, int64_t first, int64_t last);
ssw_status check_aug_code(int32_t aug_larger);
ssw_status check_avg_args(const ssw_index *idx, int32_t aug_larger, const char *who);
ssw_status launch_index_scan(ssw_index *idx, const float *q_dev, hipStream_t stream);
ssw_status do_scan(ssw_index *idx, const float *q_dev);
ssw_status ensure_full_scores(ssw_index *idx, hipStream_t stream);
inline ssw_status ensure_full_scores(ssw_index *idx) { return ensure_full_scores(idx, idx->stream); }

// index_topk.hip
ssw_status stage_query(ssw_index *idx, const float *q_host);
ssw_status do_select(ssw_index *idx, const float *scores, int32_t k, SelectDest dest, hipStream_t stream,
                     bool from_candidates = false);
ssw_status do_select_deep(ssw_index *idx, const float *scores, int32_t k, SelectDest dest, hipStream_t stream);
ssw_status install_excluded(ssw_index *idx, const int64_t *excluded_images, int64_t n_excluded, hipStream_t stream);
ssw_status topk_enqueue(ssw_index *idx, const float *q_host, const float *scores, hipStream_t stream,
                        const int64_t *excluded_images, int64_t n_excluded, int32_t k);
ssw_status topk_collect(ssw_index *idx, const float *scores, hipStream_t stream, int32_t k, int64_t *out_images,
                        float *out_scores, int64_t *out_best_rows, int32_t *out_count);
ssw_status wait_host_seq(hipStream_t stream, const unsigned *flag, unsigned seq);

// index_prune.hip
bool prune_eligible(const ssw_index *idx);
bool prune_batch_eligible(const ssw_index *idx);
bool prune6_eligible(const ssw_index *idx);
bool prune5_eligible(const ssw_index *idx);
bool prune41_eligible(const ssw_index *idx);
int64_t prune41_coarse_cap();
ssw_status prune41_stage1(ssw_index *idx, int32_t k, int blocks);
ssw_status prune41_refine(ssw_index *idx, int32_t k, const uint32_t *list_or_null, int64_t cap, float *dbg_lb5, int32_t *dbg_B);
ssw_status prune_exact_threshold(ssw_index *idx, int32_t k, int32_t kc);
ssw_status ensure_shadow(ssw_index *idx, ShadowKind kind, bool *ready);
ssw_status rows_changing(ssw_index *idx);
ssw_status prune_bounds(ssw_index *idx, ShadowKind kind, const float *q_dev, int64_t *dbg_I);
ssw_status prune_survivors(ssw_index *idx, ShadowKind kind, int32_t k, int64_t cap, hipEvent_t sleep_ev_or_null,
                           int32_t *out_m);
ssw_status scan_for_topk(ssw_index *idx, const float *q_dev, int32_t k, bool *out_candidates);
ssw_status ensure_prune_batch(ssw_index *idx, int w, int *out_w);
ssw_status prune_batch_shadow(ssw_index *idx, bool *ready);
ssw_status prune_bounds_mq(ssw_index *idx, int w, int32_t *dbg_hi, int32_t *dbg_lo, int64_t *dbg_I = nullptr);
ssw_status prune_survivors_slot(ssw_index *idx, int w, int j, int32_t k, int64_t cap);
ssw_status prune_publish_mq(ssw_index *idx, int w, int64_t cap, hipEvent_t sleep_ev_or_null, int32_t *out_m);
ssw_status rescore_rows(ssw_index *idx, const float *q_dev, const int64_t *rows_dev, float *vals_dev, int64_t m, float *dst,
                        hipStream_t stream);
int64_t batch_dev_surv_cap();
ssw_status rescore_survivors_chunk(ssw_index *idx, int w, int64_t cap);

// index_batch.hip
int64_t slab_stride(const ssw_index *idx);
float *chunk_slab(ssw_index *idx, int w, int j);
ssw_status batch_buffers(ssw_index *idx, int w, bool with_queries, int *out_w);

}  // namespace ssw
#pragma GCC visibility pop

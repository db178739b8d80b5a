// index_batch.hip -- several queries in one pass over the index's rows (scan.hip: batch_scores_kernel; over the member
// rows of a view: view_batch_kernel, through the ssw_index_view_* entries): the batched scan
// and the batched top-k, plain, pruned and two-stage, on one driver.  The handle: index_handle.h.  A batch is cut into chunks of the widest kernel form the shape and the side buffer allow, the remainder into
// narrower ones and at last single queries.  A chunk's last query scores into the handle's own buffer, the others into
// the side slabs; the selection then runs slab by slab through the single-query path (topk_enqueue / topk_collect).
#include <algorithm>
#include <cmath>
#include <cstring>

#include "index_handle.h"

using namespace ssw;

int64_t ssw::slab_stride(const ssw_index *idx) { return (idx->n + 64 + 63) & ~(int64_t)63; }  // slabs stay 256-byte aligned

// slab j of a chunk of w queries: where the scan, the pruned chunk's steps and the lab hooks put query j's scores
float *ssw::chunk_slab(ssw_index *idx, int w, int j) {
    return j + 1 < w ? idx->batch.side + (int64_t)j * slab_stride(idx) : idx->scores;
}

// the chunk's buffers for a width of w: the width they could be grown to.  The query block is allocated from a width
// of 2 on, with_queries: at any width (the pruned batch's chunk of one query reads it there); it may be missing after.
ssw_status ssw::batch_buffers(ssw_index *idx, int w, bool with_queries, int *out_w) {
    BatchState &bt = idx->batch;
    if ((w >= 2 || with_queries) && !bt.qb_dev) {
        if (hipMalloc((void **)&bt.qb_dev, (size_t)BATCH_MAX_WIDTH * idx->dim * sizeof(float)) != hipSuccess) {
            (void)hipGetLastError();
            bt.qb_dev = nullptr;
            w = 1;
        }
    }
    while (w >= 2 && bt.side_slabs < w - 1) {  // grow; on failure keep halving the width
        SSW_HIP_TRY(hipStreamSynchronize(idx->stream));
        (void)hipFree(bt.side);
        bt.side = nullptr;
        bt.side_slabs = 0;
        if (hipMalloc((void **)&bt.side, (size_t)(w - 1) * slab_stride(idx) * sizeof(float)) == hipSuccess) {
            bt.side_slabs = w - 1;
        } else {
            (void)hipGetLastError();
            bt.side = nullptr;
            w >>= 1;
        }
    }
    *out_w = w < 1 ? 1 : w;
    return SSW_OK;
}

// the chunk width to use for nq queries: limited by the shape, by nq and by what the side buffer could be grown to
static ssw_status batch_width(ssw_index *idx, int32_t nq, int *out_w) {
    int w = idx->parent ? scan_view_batch_max_width(idx->n, idx->dim, idx->dtype)
                        : scan_batch_max_width(idx->n, idx->dim, idx->dtype);
    if (w > BATCH_MAX_WIDTH) w = BATCH_MAX_WIDTH;
    while (w > nq) w >>= 1;
    return batch_buffers(idx, w, false, out_w);
}

// queries [w, dim] (host), w >= 2 -> one launch that fills chunk_slab(w, j) with the scores of query j; on a view (only
// the ssw_index_view_* entries come here with one) over its member rows in the parent's matrix
static ssw_status do_scan_chunk(ssw_index *idx, const float *q_host, int w) {
    BatchState &bt = idx->batch;
    float *slab[BATCH_MAX_WIDTH];
    for (int j = 0; j < w; ++j) slab[j] = chunk_slab(idx, w, j);
    SSW_TRY(bt.qb_stage.push(bt.qb_dev, q_host, (size_t)w * idx->dim * sizeof(float), idx->stream));
    idx->scores_partial = false;
    return profiled(idx, [&] {
        if (idx->parent)
            return launch_scan_view_batch(idx->X, idx->dtype, bt.qb_dev, idx->row_src, slab, w, idx->n, idx->dim, idx->device,
                                          idx->stream);
        return launch_scan_batch(idx->X, idx->dtype, bt.qb_dev, slab, w, idx->n, idx->dim, idx->device, idx->stream);
    });
}

static ssw_status check_query_batch(const ssw_index *idx, const float *q_host, int32_t nq) {
    for (int32_t b = 0; b < nq; ++b) {
        for (int i = 0; i < idx->dim; ++i) {
            if (!std::isfinite(q_host[(size_t)b * idx->dim + i])) {
                set_error("query %d of the batch has a non-finite component at %d", b, i);
                return SSW_ERR_NUMERIC;
            }
        }
    }
    return SSW_OK;
}

// The batched entries come in two sets.  The plain ones refuse a view (refuse_view), as every entry that walks the matrix
// by row number does; the ssw_index_view_* ones take a view and nothing else.  `view`: the call is one of the latter,
// named `who`.  Behind the gate one driver serves both: batch_width and do_scan_chunk pick the view's kernels by the
// handle, the single scans go through launch_index_scan, and the rest works on the handle's own buffers.
static ssw_status view_gate(const ssw_index *idx, bool view, const char *who) {
    if (!view) return refuse_view(idx, who);
    SSW_REQUIRE(idx == nullptr || idx->parent != nullptr,
                "%s: the index is not a view (ssw_index_create_view); the entry without `view_` takes it", who);
    return SSW_OK;
}

static ssw_status scan_batch_run(ssw_index *idx, const float *q_host, int32_t nq, float *out_scores_host, bool view) {
    SSW_TRY(view_gate(idx, view, view ? "ssw_index_view_scan_batch" : "ssw_index_scan_batch"));
    SSW_REQUIRE(nq >= 1, "nq=%d < 1", nq);
    SSW_REQUIRE(idx != nullptr && q_host != nullptr, "NULL argument");
    SSW_TRY(check_query_batch(idx, q_host, nq));
    if (nq == 1) return ssw_index_scan(idx, q_host, out_scores_host);
    DeviceGuard guard(idx->device);
    int W = 1;
    SSW_TRY(batch_width(idx, nq, &W));
    const size_t dim = (size_t)idx->dim, row_bytes = (size_t)idx->n * sizeof(float);
    for (int32_t b = 0; b < nq;) {
        int w = W;
        while (w > nq - b) w >>= 1;
        if (w >= 2) {
            SSW_TRY(do_scan_chunk(idx, q_host + b * dim, w));
        } else {
            w = 1;
            SSW_TRY(idx->q_stage.push(idx->q_dev, q_host + b * dim, dim * sizeof(float), idx->stream));
            SSW_TRY(do_scan(idx, idx->q_dev));
        }
        if (out_scores_host && idx->n > 0) {
            for (int j = 0; j < w; ++j)
                SSW_HIP_TRY(hipMemcpyAsync(out_scores_host + (size_t)(b + j) * idx->n, chunk_slab(idx, w, j), row_bytes,
                                           hipMemcpyDeviceToHost, idx->stream));
        }
        b += w;
    }
    SSW_HIP_TRY(hipStreamSynchronize(idx->stream));
    return SSW_OK;
}

extern "C" ssw_status ssw_index_scan_batch(ssw_index *idx, const float *q_host, int32_t nq, float *out_scores_host) {
    return scan_batch_run(idx, q_host, nq, out_scores_host, false);
}

extern "C" ssw_status ssw_index_view_scan_batch(ssw_index *idx, const float *q_host, int32_t nq, float *out_scores_host) {
    return scan_batch_run(idx, q_host, nq, out_scores_host, true);
}

// ---- the second stage of a batch (ssw_index_topk_batch_avg) -----------------------------------------------------------
// the most rows of one image of the index (the aggregation sizes its LDS by it): computed once per image map
static int64_t max_image_tiles(ssw_index *idx) {
    if (idx->max_image_tiles < 0) {
        int64_t m = 0;
        for (size_t p = 0; p + 1 < idx->row_start_host.size(); ++p)
            m = std::max(m, idx->row_start_host[p + 1] - idx->row_start_host[p]);
        idx->max_image_tiles = m;
    }
    return idx->max_image_tiles;
}

static ssw_status ensure_avg_buffers(ssw_index *idx) {
    BatchState &bt = idx->batch;
    const size_t slots = (size_t)BATCH_MAX_WIDTH * SSW_MAX_TOPK;
    if (!bt.avg_row) SSW_HIP_TRY(hipMalloc((void **)&bt.avg_row, slots * sizeof(int64_t)));
    if (!bt.avg_score) SSW_HIP_TRY(hipMalloc((void **)&bt.avg_score, slots * sizeof(float)));
    return SSW_OK;
}

// `partial_q`: `scores` is a pruned buffer or slab of that query (device), exact on its survivors only.  The tiles of the
// result's images are made exact first -- listed by k_candidate_tiles_keys into `rows`, scored by gather through `vals`
// (both [SURV_CAP]: survivor lists whose own rescoring is already on the stream) -- or, where k slots of max_tiles
// entries exceed the lists, the whole of `scores` by the full scan of the query.  *completed says which.
static ssw_status exact_tiles_of_result(ssw_index *idx, const float *partial_q, float *scores, int32_t k, int64_t *rows,
                                        float *vals, bool *completed) {
    const int64_t entries = (int64_t)k * idx->max_image_tiles;
    *completed = entries > SURV_CAP || !rows || !vals;
    if (*completed) {
        ++idx->prune.completions;
        return launch_scan(idx->X, idx->dtype, partial_q, scores, idx->n, idx->dim, idx->device, idx->stream);
    }
    SSW_TRY(launch_candidate_tiles_keys(idx->row_start, idx->n_images, idx->ws.out_keys, idx->ws.out_count, k,
                                        (int32_t)idx->max_image_tiles, rows, idx->stream));
    return rescore_rows(idx, partial_q, rows, vals, entries, scores, idx->stream);
}

// the aggregation of the images the selection that has just run on the stream left in the handle's result buffers,
// over the tile scores in `scores`, into row j of the chunk's device arrays
static ssw_status enqueue_avg_of_result(ssw_index *idx, const float *scores, int32_t k, int32_t aug, int j) {
    BatchState &bt = idx->batch;
    return launch_avg_score_keys(idx->tile_boxes, idx->tile_zoom, scores, idx->row_start, idx->n_images, idx->ws.out_keys,
                                 idx->ws.out_count, k, (int32_t)idx->max_image_tiles, aug, bt.avg_score + (size_t)j * k,
                                 bt.avg_row + (size_t)j * k, idx->stream);
}

// rows [0, w) of the chunk's device arrays -> the caller's rows [b, b + w): one copy each and ONE host wait
static ssw_status collect_avg(ssw_index *idx, const AvgStage *avg, int32_t b, int w, int32_t k) {
    BatchState &bt = idx->batch;
    const size_t o = (size_t)b * k, m = (size_t)w * k;
    SSW_HIP_TRY(hipMemcpyAsync(avg->out_scores + o, bt.avg_score, m * sizeof(float), hipMemcpyDeviceToHost, idx->stream));
    SSW_HIP_TRY(hipMemcpyAsync(avg->out_rows + o, bt.avg_row, m * sizeof(int64_t), hipMemcpyDeviceToHost, idx->stream));
    SSW_HIP_TRY(hipStreamSynchronize(idx->stream));
    return SSW_OK;
}

// ---- the batched top-k: one driver ----------------------------------------------------------------------------------
// the exclusion lists of a batch: query b excludes images[offsets[b] .. offsets[b + 1]); no offsets: nobody excludes
struct BatchExcluded {
    const int64_t *images, *offsets;
    const int64_t *of(int32_t b, int64_t *n_ex) const {
        *n_ex = offsets ? offsets[b + 1] - offsets[b] : 0;
        return *n_ex > 0 ? images + offsets[b] : nullptr;
    }
};

static ssw_status check_excluded_offsets(const ssw_index *idx, const BatchExcluded &ex, int32_t nq) {
    if (!ex.offsets) return SSW_OK;
    SSW_REQUIRE(ex.offsets[0] >= 0, "excluded_offsets[0]=%lld < 0", (long long)ex.offsets[0]);
    for (int32_t b = 0; b < nq; ++b)
        SSW_REQUIRE(ex.offsets[b] <= ex.offsets[b + 1], "excluded_offsets decrease at query %d", b);
    SSW_REQUIRE(ex.offsets[nq] == ex.offsets[0] || ex.images != nullptr, "excluded_images is NULL");
    return check_excluded(idx, ex.images, ex.offsets[0], ex.offsets[nq]);
}

// The scores of a pruned chunk: ONE pass over the shadow prune_batch_shadow chose bounds its w queries [b, b + w), already
// in batch.qb_dev (prune.hip, "Pruned batch"); per query a threshold selection and the survivors, one publish and ONE host wait for
// the chunk, then exact rescoring of each query's survivors, or its full scan where the certificate failed.
// m[j]: the survivors of slot j, -1 where its slab holds the full scan.
static ssw_status prune_scan_chunk(ssw_index *idx, const BatchExcluded &excl, int32_t b, int w, int32_t k, int32_t *m) {
    PruneState &p = idx->prune;
    PruneBatchState &pb = idx->prune_batch;
    pb.dev_w = 0;  // the state words are this chunk's from here on
    SSW_TRY(prune_bounds_mq(idx, w, nullptr, nullptr));
    SSW_HIP_TRY(hipEventRecord(p.ev, idx->stream));
    for (int j = 0; j < w; ++j) {  // threshold and survivors of each query, in stream order
        int64_t n_ex = 0;
        const int64_t *ex = excl.of(b + j, &n_ex);
        SSW_TRY(install_excluded(idx, ex, n_ex, idx->stream));
        SSW_TRY(do_select(idx, chunk_slab(idx, w, j), k, SelectDest{nullptr, 0u, false}, idx->stream));
        SSW_TRY(prune_survivors_slot(idx, w, j, k, SURV_CAP));
    }
    SSW_TRY(prune_publish_mq(idx, w, SURV_CAP, p.ev, m));  // sleep through the shadow scan, spin on the rest
    for (int j = 0; j < w; ++j) {
        const float *qj = idx->batch.qb_dev + (size_t)j * idx->dim;
        float *slab = chunk_slab(idx, w, j);
        ++p.queries;
        if (m[j] < 0) {
            ++p.fallbacks;
            SSW_TRY(launch_scan(idx->X, idx->dtype, qj, slab, idx->n, idx->dim, idx->device, idx->stream));
        } else {
            const int64_t *rows = pb.surv_rows + (int64_t)j * SURV_CAP;
            float *vals = pb.surv_scores + (int64_t)j * SURV_CAP;
            SSW_TRY(launch_score_rows(idx->X, idx->dtype, qj, rows, m[j], idx->dim, vals, idx->stream));
            SSW_TRY(launch_scatter_scores(rows, vals, m[j], slab, idx->stream));
        }
    }
    p.last = m[w - 1];
    idx->scores_partial = m[w - 1] >= 0;  // the handle's buffer is the last query's slab
    return SSW_OK;
}

// The four batched top-k entries and the two of a view (`view`: view_gate; never `pruned`, a view holds no shadow).
// `pruned`: a chunk's slabs get their scores from the certified pre-scan (if the index
// is not eligible or its shadow is refused: from the plain scan, and the prune counters stay as they are).  With `avg`,
// every query's selection is followed by the aggregation over its own slab; a pruned slab is exact on its survivors
// only, so the tiles of the selected images are rescored into it first (exact_tiles_of_result).
static ssw_status topk_batch_run(ssw_index *idx, const float *q_host, int32_t nq, const int64_t *excluded_images,
                                 const int64_t *excluded_offsets, int32_t k, int64_t *out_images, float *out_scores,
                                 int64_t *out_best_rows, int32_t *out_counts, const AvgStage *avg, bool pruned,
                                 bool view = false) {
    SSW_TRY(view_gate(idx, view, view ? (avg ? "ssw_index_view_topk_batch_avg" : "ssw_index_view_topk_batch")
                                 : avg ? (pruned ? "ssw_index_topk_batch_avg_pruned" : "ssw_index_topk_batch_avg")
                                       : (pruned ? "ssw_index_topk_batch_pruned" : "ssw_index_topk_batch")));
    SSW_REQUIRE(nq >= 1, "nq=%d < 1", nq);
    SSW_REQUIRE(idx != nullptr && q_host != nullptr && out_counts != nullptr, "NULL argument");
    SSW_REQUIRE(k >= 1 && k <= SSW_MAX_TOPK, "k=%d outside [1, %d]", k, SSW_MAX_TOPK);
    const BatchExcluded excl{excluded_images, excluded_offsets};
    SSW_TRY(check_excluded_offsets(idx, excl, nq));
    SSW_TRY(check_query_batch(idx, q_host, nq));
    for (int32_t b = 0; b < nq; ++b) out_counts[b] = 0;
    DeviceGuard guard(idx->device);
    int W = 1;
    if (avg && nq == 1) pruned = false;  // the single call below prunes by itself, on whichever shadow applies
    if (pruned) {
        bool ready = false;
        if (idx->ws.xchg.msg_out == nullptr) SSW_TRY(prune_batch_shadow(idx, &ready));
        if (ready) SSW_TRY(batch_buffers(idx, std::min<int32_t>(nq, Q8_MQ_WIDTH), true, &W));
        pruned = ready && idx->batch.qb_dev;
    }
    if (pruned) {
        // (a partial buffer is not completed first: every chunk overwrites it and the kept query together)
        SSW_TRY(ensure_ws(idx));
        SSW_TRY(ensure_prune_batch(idx, W, &W));
    } else if (nq == 1) {  // the single call itself, pruning included
        int64_t n_ex = 0;
        const int64_t *ex = excl.of(0, &n_ex);
        SSW_TRY(ssw_index_topk(idx, q_host, ex, n_ex, k, out_images, out_scores, out_best_rows, out_counts));
        if (!avg || idx->n_images == 0) return SSW_OK;
        SSW_TRY(ensure_avg_buffers(idx));
        if (idx->scores_partial) {  // a pruned top-k left exact scores for its survivors only
            bool completed = false;
            SSW_TRY(exact_tiles_of_result(idx, idx->prune.q_last, idx->scores, k, idx->prune.surv_rows,
                                          idx->prune.surv_scores, &completed));
            if (completed) idx->scores_partial = false;
        }
        SSW_TRY(enqueue_avg_of_result(idx, idx->scores, k, avg->aug, 0));
        return collect_avg(idx, avg, 0, 1, k);
    } else {
        SSW_TRY(ensure_full_scores(idx));
        if (avg) SSW_TRY(ensure_avg_buffers(idx));
        SSW_TRY(batch_width(idx, nq, &W));
    }
    if (pruned && avg) SSW_TRY(ensure_avg_buffers(idx));
    const size_t dim = (size_t)idx->dim;
    int32_t surv[Q8_MQ_WIDTH];  // of a pruned chunk's slots, -1: the slab holds the full scan
    for (int32_t b = 0; b < nq;) {
        const float *q = q_host + b * dim;
        int w = W;
        if (pruned) w = std::min<int32_t>(W, nq - b);  // the shadow scan takes any width,
        else while (w > nq - b) w >>= 1;               // the row scan powers of two
        if (pruned) {
            SSW_TRY(idx->batch.qb_stage.push(idx->batch.qb_dev, q, (size_t)w * dim * sizeof(float), idx->stream));
            SSW_TRY(profiled(idx, [&] { return prune_scan_chunk(idx, excl, b, w, k, surv); }));
        } else if (w >= 2) {
            SSW_TRY(do_scan_chunk(idx, q, w));
        } else {  // one query: the full single-query scan (never the pre-scan) into the handle's buffer
            w = 1;
            SSW_TRY(stage_query(idx, q));
            SSW_TRY(do_scan(idx, idx->q_dev));
        }
        for (int j = 0; j < w; ++j) {
            int64_t n_ex = 0;
            const int64_t *ex = excl.of(b + j, &n_ex);
            const size_t o = (size_t)(b + j) * k;
            float *slab = chunk_slab(idx, w, j);
            SSW_TRY(topk_enqueue(idx, nullptr, slab, idx->stream, ex, n_ex, k));
            SSW_TRY(topk_collect(idx, slab, idx->stream, k, out_images ? out_images + o : nullptr,
                                 out_scores ? out_scores + o : nullptr, out_best_rows ? out_best_rows + o : nullptr,
                                 out_counts + b + j));
            // after the collect: after a deep rerun too, and before the next query's selection takes the result buffers
            if (avg && pruned && surv[j] >= 0) {
                PruneBatchState &pb = idx->prune_batch;
                bool completed = false;
                SSW_TRY(exact_tiles_of_result(idx, idx->batch.qb_dev + (size_t)j * dim, slab, k,
                                              pb.surv_rows + (int64_t)j * SURV_CAP, pb.surv_scores + (int64_t)j * SURV_CAP,
                                              &completed));
                if (completed && slab == idx->scores) idx->scores_partial = false;
            }
            if (avg) SSW_TRY(enqueue_avg_of_result(idx, slab, k, avg->aug, j));
        }
        if (avg) SSW_TRY(collect_avg(idx, avg, b, w, k));  // (before the next chunk's scan takes the slabs)
        b += w;
    }
    return SSW_OK;
}

extern "C" {

ssw_status ssw_index_topk_batch(ssw_index *idx, const float *q_host, int32_t nq, const int64_t *excluded_images,
                                const int64_t *excluded_offsets, int32_t k, int64_t *out_images, float *out_scores,
                                int64_t *out_best_rows, int32_t *out_counts) {
    return topk_batch_run(idx, q_host, nq, excluded_images, excluded_offsets, k, out_images, out_scores, out_best_rows,
                          out_counts, nullptr, false);
}

ssw_status ssw_index_topk_batch_pruned(ssw_index *idx, const float *q_host, int32_t nq, const int64_t *excluded_images,
                                       const int64_t *excluded_offsets, int32_t k, int64_t *out_images,
                                       float *out_scores, int64_t *out_best_rows, int32_t *out_counts) {
    return topk_batch_run(idx, q_host, nq, excluded_images, excluded_offsets, k, out_images, out_scores, out_best_rows,
                          out_counts, nullptr, true);
}

ssw_status ssw_index_view_topk_batch(ssw_index *idx, const float *q_host, int32_t nq, const int64_t *excluded_images,
                                     const int64_t *excluded_offsets, int32_t k, int64_t *out_images, float *out_scores,
                                     int64_t *out_best_rows, int32_t *out_counts) {
    return topk_batch_run(idx, q_host, nq, excluded_images, excluded_offsets, k, out_images, out_scores, out_best_rows,
                          out_counts, nullptr, false, true);
}

}  // extern "C"

// ---- the batched top-k that stays on the device: every query's message into a slot of the batch exchange target ------
// what a call that writes slots [first, first + n) of the batch target must hold, checked before anything is enqueued
static ssw_status check_batch_target(const ssw_index *idx, int32_t k, int32_t first, int32_t n, const char *who) {
    SSW_REQUIRE(k >= 1 && k <= SSW_MAX_TOPK, "k=%d outside [1, %d]", k, SSW_MAX_TOPK);
    SSW_REQUIRE(idx->xchg_batch.msg_out != nullptr, "%s: no batch exchange target attached", who);
    SSW_REQUIRE(k <= idx->xchg_batch.k_max, "%s: k=%d exceeds the batch exchange target's k_max=%d", who, k,
                idx->xchg_batch.k_max);
    SSW_REQUIRE(first >= 0 && (int64_t)first + n <= idx->xchg_batch_slots, "%s: slots [%d, %lld) outside the target's %d",
                who, first, (long long)first + n, idx->xchg_batch_slots);
    return SSW_OK;
}

// the batch target narrowed to one slot: what the selection's last kernel takes as its message
static FinalExchange batch_slot(const ssw_index *idx, int32_t slot) {
    FinalExchange x = idx->xchg_batch;
    x.msg_out += (int64_t)slot * x.msg_len;
    return x;
}

// an index without images still takes part in the exchange: its slots say "0 keys"
static ssw_status empty_slots(ssw_index *idx, int32_t first, int32_t n) {
    for (int32_t s = first; s < first + n; ++s)
        SSW_HIP_TRY(hipMemsetAsync(batch_slot(idx, s).msg_out + (idx->xchg_batch.msg_len - 1), 0, sizeof(uint64_t),
                                   idx->stream));
    return SSW_OK;
}

// The chunk of w queries [b, b + w) of ssw_index_topk_batch_dev_pruned, already in batch.qb_dev: prune_scan_chunk without
// its host wait.  The bounds of all w queries from one pass over the chosen shadow; per slot the threshold selection (no
// message, no host result) and the survivors; ONE launch scores every certified slot's survivors into its slab
// (rescore_dev.hip).  Nothing is published: which slots failed their certificate stays on the device, where
// launch_mark_uncertified tells the slot's message after the selection.
static ssw_status prune_scan_chunk_dev(ssw_index *idx, const BatchExcluded &excl, int32_t b, int w, int32_t k, int64_t cap) {
    PruneBatchState &pb = idx->prune_batch;
    pb.dev_w = w;
    pb.dev_cap = cap;
    SSW_TRY(prune_bounds_mq(idx, w, nullptr, nullptr));
    const FinalExchange none;  // (not ws.xchg either: a single target may be attached beside the batch target)
    for (int j = 0; j < w; ++j) {
        int64_t n_ex = 0;
        const int64_t *ex = excl.of(b + j, &n_ex);
        SSW_TRY(install_excluded(idx, ex, n_ex, idx->stream));
        SelectDest quiet;
        quiet.message = false;
        quiet.target = &none;
        SSW_TRY(do_select(idx, chunk_slab(idx, w, j), k, quiet, idx->stream));
        SSW_TRY(prune_survivors_slot(idx, w, j, k, cap));
    }
    SSW_TRY(rescore_survivors_chunk(idx, w, cap));
    idx->prune.queries += w;  // (last_survivors and fallbacks: the host does not know them)
    return SSW_OK;
}

// The two batched top-k entries that stay on the device.  `pruned`: a chunk's slabs get their scores from the certified
// pre-scan without a host wait (if the index is not eligible or its shadow is refused: from the plain scan, and the
// call is ssw_index_topk_batch_dev).
static ssw_status topk_batch_dev_run(ssw_index *idx, const float *q_host, int32_t nq, const int64_t *excluded_images,
                                     const int64_t *excluded_offsets, int32_t k, int32_t first_slot, bool pruned) {
    // a view has no exchange target to write into, so the batch that stays on the device has no view form
    SSW_TRY(refuse_view(idx, pruned ? "ssw_index_topk_batch_dev_pruned" : "ssw_index_topk_batch_dev"));
    SSW_REQUIRE(nq >= 1, "nq=%d < 1", nq);
    SSW_REQUIRE(idx != nullptr && q_host != nullptr, "NULL argument");
    SSW_TRY(check_batch_target(idx, k, first_slot, nq, "topk_batch_dev"));
    const BatchExcluded excl{excluded_images, excluded_offsets};
    SSW_TRY(check_excluded_offsets(idx, excl, nq));
    SSW_TRY(check_query_batch(idx, q_host, nq));
    DeviceGuard guard(idx->device);
    if (idx->n_images == 0) return empty_slots(idx, first_slot, nq);
    int W = 1;
    if (pruned) {
        bool ready = false;
        idx->prune_batch.dev_w = 0;  // until a chunk of this call says otherwise
        SSW_TRY(prune_batch_shadow(idx, &ready));
        if (ready) SSW_TRY(batch_buffers(idx, std::min<int32_t>(nq, Q8_MQ_WIDTH), true, &W));
        pruned = ready && idx->batch.qb_dev;
    }
    if (pruned) {
        // (a partial buffer is not completed first: every chunk overwrites it and the kept query together)
        SSW_TRY(ensure_ws(idx));
        SSW_TRY(ensure_prune_batch(idx, W, &W));
    } else {
        SSW_TRY(ensure_full_scores(idx));
        SSW_TRY(ensure_ws(idx));
        SSW_TRY(batch_width(idx, nq, &W));
    }
    const int64_t cap = batch_dev_surv_cap();
    const size_t dim = (size_t)idx->dim;
    for (int32_t b = 0; b < nq;) {
        const float *q = q_host + b * dim;
        int w = W;
        if (pruned) w = std::min<int32_t>(W, nq - b);  // the shadow scan takes any width,
        else while (w > nq - b) w >>= 1;               // the row scan powers of two
        if (pruned) {
            SSW_TRY(idx->batch.qb_stage.push(idx->batch.qb_dev, q, (size_t)w * dim * sizeof(float), idx->stream));
            SSW_TRY(profiled(idx, [&] { return prune_scan_chunk_dev(idx, excl, b, w, k, cap); }));
        } else if (w >= 2) {
            SSW_TRY(do_scan_chunk(idx, q, w));
        } else {  // one query: the full single-query scan (never the pre-scan) into the handle's buffer
            w = 1;
            SSW_TRY(stage_query(idx, q));
            SSW_TRY(do_scan(idx, idx->q_dev));
        }
        for (int j = 0; j < w; ++j) {  // the ordinary selection on each slab; its last kernel writes the slot
            int64_t n_ex = 0;
            const int64_t *ex = excl.of(b + j, &n_ex);
            SSW_TRY(install_excluded(idx, ex, n_ex, idx->stream));
            const FinalExchange slot = batch_slot(idx, first_slot + b + j);
            SelectDest dest;
            dest.target = &slot;
            SSW_TRY(do_select(idx, chunk_slab(idx, w, j), k, dest, idx->stream));
            if (pruned)  // a slot that failed its certificate selected among bounds: bit 33 of its last word says so
                SSW_TRY(launch_mark_uncertified(idx->prune_batch.mq + j * Q8_MQ_WORDS, cap,
                                                slot.msg_out + (slot.msg_len - 1), idx->stream));
        }
        b += w;
    }
    return SSW_OK;
}

extern "C" ssw_status ssw_index_topk_batch_dev(ssw_index *idx, const float *q_host, int32_t nq,
                                               const int64_t *excluded_images, const int64_t *excluded_offsets,
                                               int32_t k, int32_t first_slot) {
    return topk_batch_dev_run(idx, q_host, nq, excluded_images, excluded_offsets, k, first_slot, false);
}

extern "C" ssw_status ssw_index_topk_batch_dev_pruned(ssw_index *idx, const float *q_host, int32_t nq,
                                                      const int64_t *excluded_images, const int64_t *excluded_offsets,
                                                      int32_t k, int32_t first_slot) {
    return topk_batch_dev_run(idx, q_host, nq, excluded_images, excluded_offsets, k, first_slot, true);
}

extern "C" ssw_status ssw_index_topk_slot_deep_dev(ssw_index *idx, const float *q_host, const int64_t *excluded_images,
                                                   int64_t n_excluded, int32_t k, int32_t slot) {
    SSW_TRY(refuse_view(idx, "ssw_index_topk_slot_deep_dev"));
    SSW_REQUIRE(idx != nullptr && q_host != nullptr, "NULL argument");
    SSW_REQUIRE(n_excluded == 0 || excluded_images != nullptr, "excluded_images is NULL");
    SSW_TRY(check_batch_target(idx, k, slot, 1, "topk_slot_deep_dev"));
    SSW_TRY(check_excluded(idx, excluded_images, 0, n_excluded));
    SSW_TRY(check_query(idx, q_host));
    DeviceGuard guard(idx->device);
    if (idx->n_images == 0) return empty_slots(idx, slot, 1);
    SSW_TRY(ensure_ws(idx));
    SSW_TRY(stage_query(idx, q_host));
    SSW_TRY(do_scan(idx, idx->q_dev));  // the slab of the flagged query is gone: the same bits again
    SSW_TRY(install_excluded(idx, excluded_images, n_excluded, idx->stream));
    if (idx->has_map)
        SSW_TRY(launch_image_max(idx->scores, idx->row_start, idx->n_images, idx->ws.img_score, idx->ws.img_best,
                                 idx->stream));
    const FinalExchange target = batch_slot(idx, slot);
    SelectDest dest;
    dest.target = &target;
    return do_select_deep(idx, idx->scores, k, dest, idx->stream);
}

// The second stage of a sharded batch on this handle (k_avg_score_owner, rescore.hip): the group's merged candidates are
// aggregated where their tiles live, from the index rows alone.  It reads no score buffer, result buffer or prune state
// and writes none, so it follows the plain and the pruned first stage alike and never completes a buffer.
extern "C" ssw_status ssw_index_stage2_avg_batch_dev(ssw_index *idx, const float *q_host, int32_t nq,
                                                     const uint64_t *dev_keys, const int32_t *dev_counts, int32_t k_max,
                                                     int32_t k, int32_t aug_larger, int64_t image_offset,
                                                     int64_t row_offset, uint64_t *dev_out) {
    SSW_TRY(refuse_view(idx, "ssw_index_stage2_avg_batch_dev"));  // k_avg_score_owner scores tiles from the matrix by row
    SSW_REQUIRE(nq >= 1, "nq=%d < 1", nq);
    SSW_REQUIRE(k >= 1 && k <= k_max && k_max <= SSW_MAX_TOPK, "k=%d outside [1, k_max=%d], k_max at most %d", k, k_max,
                SSW_MAX_TOPK);
    SSW_TRY(check_aug_code(aug_larger));
    SSW_REQUIRE(idx && q_host && dev_keys && dev_counts && dev_out, "NULL argument");
    SSW_TRY(check_avg_args(idx, aug_larger, "stage2_avg_batch_dev"));
    if (idx->dim != 256 && idx->dim != 512 && idx->dim != 768 && idx->dim != 1024) {
        set_error("stage2_avg_batch_dev: dim=%d unsupported", idx->dim);
        return SSW_ERR_UNSUPPORTED;
    }
    const int64_t max_tiles = max_image_tiles(idx);
    SSW_REQUIRE(max_tiles <= SSW_RESCORE_MAX_TILES,
                "the index has an image with %lld tiles, more than the %d the kernel keeps in LDS", (long long)max_tiles,
                SSW_RESCORE_MAX_TILES);
    SSW_TRY(check_query_batch(idx, q_host, nq));
    DeviceGuard guard(idx->device);
    int W = 1;
    SSW_TRY(batch_buffers(idx, 1, true, &W));  // the query block alone
    if (!idx->batch.qb_dev) {
        set_error("stage2_avg_batch_dev: no device memory for the query block");
        return SSW_ERR_NOMEM;
    }
    const size_t dim = (size_t)idx->dim;
    for (int32_t b = 0; b < nq; b += BATCH_MAX_WIDTH) {  // the block holds BATCH_MAX_WIDTH queries
        const int32_t w = std::min<int32_t>(BATCH_MAX_WIDTH, nq - b);
        SSW_TRY(idx->batch.qb_stage.push(idx->batch.qb_dev, q_host + b * dim, (size_t)w * dim * sizeof(float), idx->stream));
        AvgOwnerArgs a;
        a.qb = idx->batch.qb_dev;
        a.boxes = idx->tile_boxes;
        a.zoom = idx->tile_zoom;
        a.row_start = idx->row_start;
        a.n_images = idx->n_images;
        a.keys = dev_keys + (size_t)b * k_max;
        a.counts = dev_counts + b;
        a.nq = w, a.k_max = k_max, a.k = k, a.max_tiles = (int32_t)max_tiles, a.aug = aug_larger;
        a.image_offset = image_offset, a.row_offset = row_offset;
        a.out = dev_out + (size_t)b * 2 * k_max;
        SSW_TRY(launch_avg_score_owner(idx->X, idx->dtype, idx->dim, a, idx->stream));
    }
    return SSW_OK;
}

// The second stage of a batch of two-vector queries on this handle (k_pair_score, rescore.hip): host data in, host data
// out, ONE copy up, ONE launch, ONE copy down, ONE host wait.  Like the entry above it reads the rows, the image map and
// (avg) the tile meta and nothing else.
extern "C" ssw_status ssw_index_stage2_pair_batch(ssw_index *idx, const float *q_host, const float *q2_host, int32_t nq,
                                                  const int64_t *image_positions_host, const int32_t *counts_host,
                                                  int32_t k, int32_t agg, int32_t aug_larger, float *out_scores,
                                                  int64_t *out_best_rows) {
    SSW_REQUIRE(idx != nullptr, "idx is NULL");
    SSW_TRY(refuse_view(idx, "ssw_index_stage2_pair_batch"));  // k_pair_score scores tiles from the matrix by row
    SSW_REQUIRE(nq >= 1 && nq <= 65535, "nq=%d outside [1, 65535]", nq);
    SSW_REQUIRE(k >= 1 && k <= SSW_MAX_TOPK, "k=%d outside [1, %d]", k, SSW_MAX_TOPK);
    SSW_REQUIRE(agg == SSW_AGG_PLAIN || agg == SSW_AGG_AVG, "agg=%d is not 0 (plain_score) or 1 (avg_score)", agg);
    SSW_REQUIRE(q_host && q2_host && image_positions_host && counts_host && out_scores && out_best_rows, "NULL argument");
    SSW_REQUIRE(idx->has_map, "stage2_pair_batch needs ssw_index_set_row2image first");
    if (agg == SSW_AGG_AVG) {
        SSW_TRY(check_aug_code(aug_larger));
        if (!idx->tile_boxes || !idx->tile_zoom) {
            set_error("stage2_pair_batch: the avg_score aggregation needs ssw_index_set_tile_meta first");
            return SSW_ERR_UNSUPPORTED;
        }
    }
    if (idx->dim != 256 && idx->dim != 512 && idx->dim != 768 && idx->dim != 1024) {
        set_error("stage2_pair_batch: dim=%d unsupported", idx->dim);
        return SSW_ERR_UNSUPPORTED;
    }
    const int64_t max_tiles = max_image_tiles(idx);
    if (max_tiles > SSW_RESCORE_MAX_TILES) {
        set_error("stage2_pair_batch: the index has an image with %lld tiles, more than the %d the kernel takes",
                  (long long)max_tiles, SSW_RESCORE_MAX_TILES);
        return SSW_ERR_UNSUPPORTED;
    }
    for (int32_t b = 0; b < nq; ++b) {
        SSW_REQUIRE(counts_host[b] >= 0 && counts_host[b] <= k, "counts[%d]=%d outside [0, k=%d]", b, counts_host[b], k);
        for (int32_t c = 0; c < counts_host[b]; ++c) {
            const int64_t p = image_positions_host[(size_t)b * k + c];
            SSW_REQUIRE(p >= 0 && p < idx->n_images, "image position %lld (query %d, slot %d) outside [0, %lld)",
                        (long long)p, b, c, (long long)idx->n_images);
        }
    }
    SSW_TRY(check_query_batch(idx, q_host, nq));
    SSW_TRY(check_query_batch(idx, q2_host, nq));
    DeviceGuard guard(idx->device);
    // the block: [positions i64 nq k | q f32 nq dim | q2 f32 nq dim | counts i32 nq] [rows i64 nq k | scores f32 nq k],
    // the query blocks (read as float4) and the outputs on 16-byte boundaries
    const size_t slots = (size_t)nq * k, qbytes = (size_t)nq * idx->dim * sizeof(float);
    const size_t off_q = (slots * 8 + 15) & ~(size_t)15, off_q2 = off_q + qbytes, off_cnt = off_q2 + qbytes;
    const size_t in_bytes = (off_cnt + (size_t)nq * 4 + 15) & ~(size_t)15;
    const size_t off_score = in_bytes + slots * 8, total = off_score + slots * 4;
    PairStage &ps = idx->pair;
    hipStream_t s = idx->stream;
    if (total > ps.cap) {
        SSW_HIP_TRY(hipStreamSynchronize(s));
        ps.release();
        size_t cap = (size_t)1 << 16;
        while (cap < total) cap <<= 1;
        if (hipHostMalloc((void **)&ps.host, cap) != hipSuccess || hipMalloc((void **)&ps.dev, cap) != hipSuccess) {
            (void)hipGetLastError();
            ps.release();
            set_error("stage2_pair_batch: no memory for the %zu-byte staging blocks", cap);
            return SSW_ERR_NOMEM;
        }
        ps.cap = cap;
    }
    memcpy(ps.host, image_positions_host, slots * 8);
    memcpy(ps.host + off_q, q_host, qbytes);
    memcpy(ps.host + off_q2, q2_host, qbytes);
    memcpy(ps.host + off_cnt, counts_host, (size_t)nq * 4);
    SSW_HIP_TRY(hipMemcpyAsync(ps.dev, ps.host, in_bytes, hipMemcpyHostToDevice, s));
    PairScoreArgs a;
    a.qb = reinterpret_cast<const float *>(ps.dev + off_q);
    a.q2b = reinterpret_cast<const float *>(ps.dev + off_q2);
    a.boxes = idx->tile_boxes;
    a.zoom = idx->tile_zoom;
    a.row_start = idx->row_start;
    a.n_images = idx->n_images;
    a.pos = reinterpret_cast<const int64_t *>(ps.dev);
    a.counts = reinterpret_cast<const int32_t *>(ps.dev + off_cnt);
    a.nq = nq, a.k = k, a.max_tiles = (int32_t)max_tiles, a.aug = agg == SSW_AGG_AVG ? aug_larger : 0;
    a.avg = agg == SSW_AGG_AVG;
    a.out_row = reinterpret_cast<int64_t *>(ps.dev + in_bytes);
    a.out_score = reinterpret_cast<float *>(ps.dev + off_score);
    SSW_TRY(launch_pair_score(idx->X, idx->dtype, idx->dim, a, s));
    SSW_HIP_TRY(hipMemcpyAsync(ps.host + in_bytes, ps.dev + in_bytes, total - in_bytes, hipMemcpyDeviceToHost, s));
    SSW_HIP_TRY(hipStreamSynchronize(s));
    const int64_t *rows = reinterpret_cast<const int64_t *>(ps.host + in_bytes);
    const float *scores = reinterpret_cast<const float *>(ps.host + off_score);
    for (int32_t b = 0; b < nq; ++b) {  // slots at or past the count stay the caller's
        const size_t o = (size_t)b * k, m = (size_t)counts_host[b];
        memcpy(out_scores + o, scores + o, m * 4);
        memcpy(out_best_rows + o, rows + o, m * 8);
    }
    return SSW_OK;
}

// the two-stage entries: the first stage plain or, `pruned`, from the certified pre-scan
static ssw_status topk_batch_avg(ssw_index *idx, const float *q_host, int32_t nq, const int64_t *excluded_images,
                                 const int64_t *excluded_offsets, int32_t k, int32_t aug_larger, int64_t *out_images,
                                 float *out_scores, int64_t *out_best_rows, float *out_avg_scores, int64_t *out_avg_rows,
                                 int32_t *out_counts, bool pruned, bool view = false) {
    SSW_TRY(view_gate(idx, view, view ? "ssw_index_view_topk_batch_avg"
                                      : pruned ? "ssw_index_topk_batch_avg_pruned" : "ssw_index_topk_batch_avg"));
    SSW_REQUIRE(nq >= 1, "nq=%d < 1", nq);
    SSW_REQUIRE(idx && q_host && out_counts && out_avg_scores && out_avg_rows, "NULL argument");
    SSW_TRY(check_avg_args(idx, aug_larger, "topk_batch_avg"));
    const int64_t max_tiles = max_image_tiles(idx);
    SSW_REQUIRE(max_tiles <= SSW_RESCORE_MAX_TILES,
                "the index has an image with %lld tiles, more than the %d the kernel keeps in LDS", (long long)max_tiles,
                SSW_RESCORE_MAX_TILES);
    const AvgStage avg{aug_larger, out_avg_scores, out_avg_rows};
    return topk_batch_run(idx, q_host, nq, excluded_images, excluded_offsets, k, out_images, out_scores, out_best_rows,
                          out_counts, &avg, pruned, view);
}

extern "C" {

ssw_status ssw_index_topk_batch_avg(ssw_index *idx, const float *q_host, int32_t nq, const int64_t *excluded_images,
                                    const int64_t *excluded_offsets, int32_t k, int32_t aug_larger, int64_t *out_images,
                                    float *out_scores, int64_t *out_best_rows, float *out_avg_scores,
                                    int64_t *out_avg_rows, int32_t *out_counts) {
    return topk_batch_avg(idx, q_host, nq, excluded_images, excluded_offsets, k, aug_larger, out_images, out_scores,
                          out_best_rows, out_avg_scores, out_avg_rows, out_counts, false);
}

ssw_status ssw_index_topk_batch_avg_pruned(ssw_index *idx, const float *q_host, int32_t nq, const int64_t *excluded_images,
                                           const int64_t *excluded_offsets, int32_t k, int32_t aug_larger,
                                           int64_t *out_images, float *out_scores, int64_t *out_best_rows,
                                           float *out_avg_scores, int64_t *out_avg_rows, int32_t *out_counts) {
    return topk_batch_avg(idx, q_host, nq, excluded_images, excluded_offsets, k, aug_larger, out_images, out_scores,
                          out_best_rows, out_avg_scores, out_avg_rows, out_counts, true);
}

ssw_status ssw_index_view_topk_batch_avg(ssw_index *idx, const float *q_host, int32_t nq, const int64_t *excluded_images,
                                         const int64_t *excluded_offsets, int32_t k, int32_t aug_larger,
                                         int64_t *out_images, float *out_scores, int64_t *out_best_rows,
                                         float *out_avg_scores, int64_t *out_avg_rows, int32_t *out_counts) {
    return topk_batch_avg(idx, q_host, nq, excluded_images, excluded_offsets, k, aug_larger, out_images, out_scores,
                          out_best_rows, out_avg_scores, out_avg_rows, out_counts, false, true);
}

}  // extern "C"

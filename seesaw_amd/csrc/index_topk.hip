// index_topk.hip -- the index's top-k selection (see include/seesaw_hip.h): the small and the general form behind one
// enqueue / collect pair, and the entries built on it.  The handle: index_handle.h.
#include <algorithm>
#include <chrono>

#include "index_handle.h"

using namespace ssw;

// a host query reaches q_dev through the kernel-argument segment of a one-wave kernel (dim <= 768): a launch is a
// third of what the 2-KB copy and its event cost on the host
constexpr int Q_ARG_FLOATS = 768;
struct QArg {
    float v[Q_ARG_FLOATS];
};
__global__ void k_stage_query(QArg q, float *__restrict__ dst, int dim) {
    for (int i = threadIdx.x; i < dim; i += 256) dst[i] = q.v[i];
}
ssw_status ssw::stage_query(ssw_index *idx, const float *q_host) {
    if (idx->dim > Q_ARG_FLOATS)
        return idx->q_stage.push(idx->q_dev, q_host, (size_t)idx->dim * sizeof(float), idx->stream);
    QArg q;
    memcpy(q.v, q_host, (size_t)idx->dim * sizeof(float));
    hipLaunchKernelGGL(k_stage_query, dim3(1), dim3(256), 0, idx->stream, q, idx->q_dev, idx->dim);
    SSW_HIP_TRY(hipGetLastError());
    return SSW_OK;
}

// the selection over the row scores in `scores`: per-image maxima first when the index has an image map.
// from_candidates: scan_for_topk, just before on this stream, left the candidates of this very selection in the
// workspace (an index without a map), so only the last kernel runs.
ssw_status ssw::do_select(ssw_index *idx, const float *scores, int32_t k, SelectDest dest, hipStream_t stream,
                          bool from_candidates) {
    SSW_TRY(ensure_ws(idx));
    if (from_candidates) return launch_select_candidates(idx->ws, k, dest, stream);
    if (idx->has_map) {
        SSW_TRY(launch_image_max(scores, idx->row_start, idx->n_images, idx->ws.img_score, idx->ws.img_best, stream));
        return launch_select_topk(idx->ws, idx->ws.img_score, idx->n_images, idx->ws.img_best, k, dest, idx->device, stream);
    }
    return launch_select_topk(idx->ws, scores, idx->n, nullptr, k, dest, idx->device, stream);
}

// the deep path over what the last do_select of `scores` left (the per-image maxima are still in the workspace)
ssw_status ssw::do_select_deep(ssw_index *idx, const float *scores, int32_t k, SelectDest dest, hipStream_t stream) {
    const float *values = idx->has_map ? idx->ws.img_score : scores;
    const uint32_t *best = idx->has_map ? idx->ws.img_best : nullptr;
    return launch_select_topk_deep(idx->ws, values, idx->n_images, best, k, dest, idx->device, stream);
}

ssw_status ssw::install_excluded(ssw_index *idx, const int64_t *excluded_images, int64_t n_excluded, hipStream_t stream) {
    SSW_TRY(check_excluded(idx, excluded_images, 0, n_excluded));
    SSW_TRY(ensure_ws(idx));
    return select_set_excluded(idx->ws, idx->n_images, excluded_images, n_excluded, stream);
}

// one pinned block receives the packed result [count, overflow, k, seq][keys k][best k]: written by the selection
// itself (select_to_host), else one async copy + one synchronisation
static ssw_status ensure_res_host(ssw_index *idx) {
    const size_t cap = 16 + (size_t)SSW_MAX_TOPK * 12;
    if (!idx->res_host) {
        SSW_HIP_TRY(hipHostMalloc((void **)&idx->res_host, cap, hipHostMallocMapped | hipHostMallocCoherent));
        memset(idx->res_host, 0, cap);
    }
    return SSW_OK;
}

ssw_status ssw::wait_host_seq(hipStream_t stream, const unsigned *flag, unsigned seq) {
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned it = 0;; ++it) {
        if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) == seq) return SSW_OK;
        if ((it & 1023u) == 1023u && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(5)) break;
    }
    SSW_HIP_TRY(hipStreamSynchronize(stream));  // a long scan ahead of the selection: sleep in the runtime instead
    if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) != seq) {
        set_error("topk: the selection kernel finished without publishing its result");
        return SSW_ERR_HIP;
    }
    return SSW_OK;
}

// ---- top-k of row scores that are resident on the device -> host: ONE path, in an enqueue and a collect half ----------
// An index of a few thousand images (an LVIS-category subset: 1 109 images x 13 tiles) spends its round in fixed
// costs, not in the scan: three copies, five launches and a stream wait were ~95 us around ~10 us of kernels.  Its form
// is three launches and no copy: the query goes to q_dev through a kernel argument, the scan runs on every CU, and ONE
// kernel takes the per-image maximum, strikes out the excluded ids (read from pinned memory the device maps), selects
// and writes the packed result into the same pinned block, releasing a sequence word the host spins on.
static SSW_TUNABLE bool g_small_path = true;  // ssw_tune_topk

static bool small_path_ok(const ssw_index *idx, int64_t n_excluded) {
    return g_small_path && idx->n_images >= 1 && idx->n_images <= SELECT_SMALL_IMAGES && idx->n <= SMALL_ROWS &&
           n_excluded <= SMALL_EXCL_CAP;
}

// the small form's enqueue: [stage the query, scan,] exclusion list into the pinned block, ONE selection launch that
// publishes the packed result under a fresh sequence number (idx->small_pending_seq)
static ssw_status small_enqueue(ssw_index *idx, const float *q_host, const float *scores, hipStream_t stream,
                                const int64_t *excluded_images, int64_t n_excluded, int32_t k) {
    const size_t q_bytes = (size_t)idx->dim * sizeof(float), ex_bytes = (size_t)SMALL_EXCL_CAP * sizeof(int64_t);
    const size_t res_bytes = 16 + (size_t)SSW_MAX_TOPK * 12;
    if (!idx->small_host) {
        SSW_HIP_TRY(hipHostMalloc((void **)&idx->small_host, q_bytes + ex_bytes + res_bytes,
                                  hipHostMallocMapped | hipHostMallocCoherent));
        memset(idx->small_host, 0, q_bytes + ex_bytes + res_bytes);
    }
    unsigned char *dev_view = nullptr;
    SSW_HIP_TRY(hipHostGetDevicePointer((void **)&dev_view, idx->small_host, 0));
    SSW_TRY(check_excluded(idx, excluded_images, 0, n_excluded));
    SSW_TRY(ensure_ws(idx));
    if (idx->ws.excl_dirty)  // a list installed by ssw_index_set_excluded does not apply to this call
        SSW_TRY(select_set_excluded(idx->ws, idx->n_images, nullptr, 0, stream));
    if (q_host) {
        if (idx->dim <= Q_ARG_FLOATS) {  // through a kernel argument into q_dev: 451 workgroups then read it out of L2
            SSW_TRY(stage_query(idx, q_host));
            SSW_TRY(do_scan(idx, idx->q_dev));
        } else {  // (a wider query stays in the mapped block: every workgroup reads it over the host link)
            memcpy(idx->small_host, q_host, q_bytes);
            SSW_TRY(do_scan(idx, reinterpret_cast<const float *>(dev_view)));
        }
    }
    if (n_excluded > 0) memcpy(idx->small_host + q_bytes, excluded_images, (size_t)n_excluded * sizeof(int64_t));
    const unsigned seq = next_seq(idx->small_seq);
    SSW_TRY(launch_select_small(idx->ws, scores, idx->has_map ? idx->row_start : nullptr, idx->n_images,
                                reinterpret_cast<const int64_t *>(dev_view + q_bytes), n_excluded, k,
                                dev_view + q_bytes + ex_bytes, seq, stream));
    idx->small_pending_seq = seq;
    return SSW_OK;
}

// the general form's selection (deep: the rerun after an overflow): its last kernel writes the packed result into the
// pinned mirror and releases a fresh sequence word the host spins on (no device-to-host copy, no stream wait)
static ssw_status select_to_host(ssw_index *idx, const float *scores, hipStream_t stream, int32_t k, bool deep,
                                 bool from_candidates = false) {
    SSW_TRY(ensure_ws(idx));
    SSW_TRY(ensure_res_host(idx));
    SelectDest dest;
    SSW_HIP_TRY(hipHostGetDevicePointer((void **)&dest.host_packed, idx->res_host, 0));
    dest.seq = idx->res_pending_seq = next_seq(idx->small_seq);
    idx->small_pending_seq = 0;  // this selection is the one in flight: topk_collect reads res_host
    const ssw_status st = deep ? do_select_deep(idx, scores, k, dest, stream)
                                : do_select(idx, scores, k, dest, stream, from_candidates);
    if (st != SSW_OK) idx->res_pending_seq = 0;  // nothing was launched that would publish
    return st;
}

// Enqueue half.  q_host = NULL: the top-k of the row scores in `scores`, which are complete (the handle's buffer after
// ensure_full_scores, or a slab of a batch).  With a query, which is scanned into the handle's buffer on the handle's
// stream, those are `scores` and `stream`: the query is staged and scanned first -- after the exclusions are
// installed, a pruned scan selects its threshold with them.
ssw_status ssw::topk_enqueue(ssw_index *idx, const float *q_host, const float *scores, hipStream_t stream,
                               const int64_t *excluded_images, int64_t n_excluded, int32_t k) {
    SSW_REQUIRE(!q_host || (scores == idx->scores && stream == idx->stream), "topk: a query scans into the handle's buffer");
    if (small_path_ok(idx, n_excluded)) return small_enqueue(idx, q_host, scores, stream, excluded_images, n_excluded, k);
    if (q_host) SSW_TRY(stage_query(idx, q_host));
    if (idx->n_images > 0) SSW_TRY(install_excluded(idx, excluded_images, n_excluded, stream));
    bool candidates = false;
    if (q_host) SSW_TRY(scan_for_topk(idx, idx->q_dev, k, &candidates));
    if (idx->n_images == 0) return SSW_OK;
    return select_to_host(idx, scores, stream, k, false, candidates);
}

// the packed block [count, overflow, k, seq][keys k][best k] -> the caller's arrays
static void decode_packed(const unsigned char *block, int32_t k, int64_t *out_images, float *out_scores,
                          int64_t *out_best_rows, int32_t *out_count) {
    const uint64_t *keys = reinterpret_cast<const uint64_t *>(block + 16);
    const uint32_t *best = reinterpret_cast<const uint32_t *>(block + 16 + (size_t)k * sizeof(uint64_t));
    const int32_t count = std::min(*reinterpret_cast<const int32_t *>(block), k);
    for (int32_t i = 0; i < count; ++i) {
        const uint64_t key = keys[i];
        if (out_images) out_images[i] = (int64_t)(0xffffffffu - (uint32_t)(key & 0xffffffffull));
        if (out_scores) out_scores[i] = ord_to_f32((uint32_t)(key >> 32));
        if (out_best_rows) out_best_rows[i] = (int64_t)best[i];
    }
    *out_count = count;
}

// the result of the last general selection into res_host: published there by the selection itself, else copied
static ssw_status fetch_results(ssw_index *idx, hipStream_t stream, int32_t k, bool *overflow) {
    SSW_TRY(ensure_res_host(idx));
    if (idx->res_pending_seq != 0) {
        const unsigned seq = idx->res_pending_seq;
        idx->res_pending_seq = 0;
        SSW_TRY(wait_host_seq(stream, reinterpret_cast<const unsigned *>(idx->res_host) + 3, seq));
    } else {
        SSW_HIP_TRY(hipMemcpyAsync(idx->res_host, idx->ws.packed, 16 + (size_t)k * 12, hipMemcpyDeviceToHost, stream));
        SSW_HIP_TRY(hipStreamSynchronize(stream));
    }
    const int32_t *hdr = reinterpret_cast<const int32_t *>(idx->res_host);
    *overflow = hdr[1] != 0;
    if (hdr[2] != k) {
        set_error("topk_fetch: k=%d does not match the k=%d of the selection that produced the result", k, hdr[2]);
        return SSW_ERR_INVALID;
    }
    return SSW_OK;
}

// The general form's result over `scores`: the wait (a spin on the sequence word; without a selection in flight the
// result of the last ssw_index_topk_dev / _select_deep_dev, copied), the deep rerun when the fast selection
// overflowed, the decode.
static ssw_status fetch_topk(ssw_index *idx, const float *scores, hipStream_t stream, int32_t k, int64_t *out_images,
                             float *out_scores, int64_t *out_best_rows, int32_t *out_count) {
    SSW_REQUIRE(k >= 1 && k <= SSW_MAX_TOPK, "k=%d outside [1, %d]", k, SSW_MAX_TOPK);
    *out_count = 0;
    if (idx->n_images == 0) return SSW_OK;
    SSW_TRY(ensure_ws(idx));
    bool overflow = false;
    SSW_TRY(fetch_results(idx, stream, k, &overflow));
    if (overflow) {  // massive exact ties: rerun the selection on the deep path (over the per-image maxima the fast
                     // selection left in the workspace; `scores` itself is read only by an index without an image map)
        SSW_TRY(select_to_host(idx, scores, stream, k, true));
        SSW_TRY(fetch_results(idx, stream, k, &overflow));
    }
    decode_packed(static_cast<const unsigned char *>(idx->res_host), k, out_images, out_scores, out_best_rows, out_count);
    return SSW_OK;
}

// Collect half of topk_enqueue
ssw_status ssw::topk_collect(ssw_index *idx, const float *scores, hipStream_t stream, int32_t k, int64_t *out_images,
                               float *out_scores, int64_t *out_best_rows, int32_t *out_count) {
    *out_count = 0;
    if (idx->small_pending_seq == 0) return fetch_topk(idx, scores, stream, k, out_images, out_scores, out_best_rows, out_count);
    const unsigned seq = idx->small_pending_seq;
    idx->small_pending_seq = 0;
    const unsigned char *res = idx->small_host + (size_t)idx->dim * sizeof(float) + (size_t)SMALL_EXCL_CAP * sizeof(int64_t);
    SSW_TRY(wait_host_seq(stream, reinterpret_cast<const unsigned *>(res) + 3, seq));
    decode_packed(res, k, out_images, out_scores, out_best_rows, out_count);
    return SSW_OK;
}

// ---- the two halves for callers that put more work on the stream in between or ahead (ssw_labelprop_round:
// propagation -> scores -> this selection, ONE wait), on a stream of theirs
namespace ssw {
ssw_status index_enqueue_topk_resident(ssw_index *idx, hipStream_t on_stream, const int64_t *excluded_images, int64_t n_excluded,
                                       int32_t k) {
    SSW_REQUIRE(idx != nullptr, "NULL argument");
    SSW_REQUIRE(k >= 1 && k <= SSW_MAX_TOPK, "k=%d outside [1, %d]", k, SSW_MAX_TOPK);
    SSW_REQUIRE(n_excluded == 0 || excluded_images != nullptr, "excluded_images is NULL");
    SSW_TRY(ensure_full_scores(idx, on_stream));
    return topk_enqueue(idx, nullptr, idx->scores, on_stream, excluded_images, n_excluded, k);
}

ssw_status index_collect_topk(ssw_index *idx, hipStream_t on_stream, int32_t k, int64_t *out_images, float *out_scores,
                              int64_t *out_best_rows, int32_t *out_count) {
    SSW_REQUIRE(idx != nullptr && out_count != nullptr, "NULL argument");
    return topk_collect(idx, idx->scores, on_stream, k, out_images, out_scores, out_best_rows, out_count);
}

// ---- the same two halves once per slot of a chunk (ssw_labelprop_round_batch): the selections of a chunk's slots are
// enqueued back to back on one stream, each over its own score slab, and each publishes into its own pinned block
// under its own sequence word, so the host waits once for the chunk -- on the word of the slot enqueued last
constexpr size_t SLOT_EXCL_BYTES = (size_t)SMALL_EXCL_CAP * sizeof(int64_t);
constexpr size_t SLOT_BYTES = SLOT_EXCL_BYTES + 16 + (size_t)SSW_MAX_TOPK * 12;

ssw_status index_round_slabs(ssw_index *idx, int w, int *out_w, float **slabs) {
    SSW_REQUIRE(idx != nullptr && out_w != nullptr && slabs != nullptr && w >= 1, "NULL argument");
    if (w > BATCH_MAX_WIDTH) w = BATCH_MAX_WIDTH;
    SSW_TRY(batch_buffers(idx, w, false, &w));
    for (int j = 0; j < w; ++j) slabs[j] = chunk_slab(idx, w, j);
    *out_w = w;
    return SSW_OK;
}

ssw_status index_enqueue_topk_slot(ssw_index *idx, hipStream_t on_stream, int slot, const float *slab,
                                   const int64_t *excluded_images, int64_t n_excluded, int32_t k, unsigned *out_seq) {
    SSW_REQUIRE(idx != nullptr && out_seq != nullptr && slot >= 0 && slot < BATCH_MAX_WIDTH, "bad slot");
    SSW_REQUIRE(k >= 1 && k <= SSW_MAX_TOPK, "k=%d outside [1, %d]", k, SSW_MAX_TOPK);
    SSW_REQUIRE(n_excluded == 0 || excluded_images != nullptr, "excluded_images is NULL");
    *out_seq = 0;
    if (idx->n_images == 0) return SSW_OK;
    if (!idx->slot_host) {
        SSW_HIP_TRY(hipHostMalloc((void **)&idx->slot_host, (size_t)BATCH_MAX_WIDTH * SLOT_BYTES,
                                  hipHostMallocMapped | hipHostMallocCoherent));
        memset(idx->slot_host, 0, (size_t)BATCH_MAX_WIDTH * SLOT_BYTES);
    }
    unsigned char *block = idx->slot_host + (size_t)slot * SLOT_BYTES, *dev_view = nullptr;
    SSW_HIP_TRY(hipHostGetDevicePointer((void **)&dev_view, block, 0));
    SSW_TRY(check_excluded(idx, excluded_images, 0, n_excluded));
    SSW_TRY(ensure_ws(idx));
    const unsigned seq = next_seq(idx->small_seq);
    if (small_path_ok(idx, n_excluded)) {  // the form the single call takes on this index: one launch, ids read in place
        if (idx->ws.excl_dirty) SSW_TRY(select_set_excluded(idx->ws, idx->n_images, nullptr, 0, on_stream));
        if (n_excluded > 0) memcpy(block, excluded_images, (size_t)n_excluded * sizeof(int64_t));
        SSW_TRY(launch_select_small(idx->ws, slab, idx->has_map ? idx->row_start : nullptr, idx->n_images,
                                    reinterpret_cast<const int64_t *>(dev_view), n_excluded, k, dev_view + SLOT_EXCL_BYTES,
                                    seq, on_stream));
    } else {
        SSW_TRY(install_excluded(idx, excluded_images, n_excluded, on_stream));
        SelectDest dest;
        dest.host_packed = dev_view + SLOT_EXCL_BYTES;
        dest.seq = seq;
        SSW_TRY(do_select(idx, slab, k, dest, on_stream));
    }
    *out_seq = seq;
    return SSW_OK;
}

// the chunk's one wait: on the word of the slot whose selection was enqueued last
ssw_status index_wait_topk_slot(ssw_index *idx, hipStream_t on_stream, int slot, unsigned seq) {
    SSW_REQUIRE(idx != nullptr && idx->slot_host != nullptr && slot >= 0 && slot < BATCH_MAX_WIDTH && seq != 0, "bad slot");
    const unsigned char *res = idx->slot_host + (size_t)slot * SLOT_BYTES + SLOT_EXCL_BYTES;
    return wait_host_seq(on_stream, reinterpret_cast<const unsigned *>(res) + 3, seq);
}

// Collect half.  *reran: the fast selection had reported overflow (massive ties) and the slot was selected again on the
// deep path, from its slab -- the per-image maxima in the workspace are a later slot's by now -- behind one more wait.
// The excluded set is installed again for it: a later slot's is in the workspace as well.
ssw_status index_collect_topk_slot(ssw_index *idx, hipStream_t on_stream, int slot, unsigned seq, const float *slab,
                                   const int64_t *excluded_images, int64_t n_excluded, int32_t k, int64_t *out_images,
                                   float *out_scores, int64_t *out_best_rows, int32_t *out_count, bool *reran) {
    SSW_REQUIRE(idx != nullptr && out_count != nullptr && slot >= 0 && slot < BATCH_MAX_WIDTH, "bad slot");
    *out_count = 0;
    if (reran) *reran = false;
    if (idx->n_images == 0 || seq == 0) return SSW_OK;
    unsigned char *res = idx->slot_host + (size_t)slot * SLOT_BYTES + SLOT_EXCL_BYTES;
    SSW_TRY(wait_host_seq(on_stream, reinterpret_cast<const unsigned *>(res) + 3, seq));
    const int32_t *hdr = reinterpret_cast<const int32_t *>(res);
    if (!small_path_ok(idx, n_excluded) && hdr[1] != 0) {
        unsigned char *dev_view = nullptr;
        SSW_HIP_TRY(hipHostGetDevicePointer((void **)&dev_view, res, 0));
        SSW_TRY(install_excluded(idx, excluded_images, n_excluded, on_stream));
        if (idx->has_map)
            SSW_TRY(launch_image_max(slab, idx->row_start, idx->n_images, idx->ws.img_score, idx->ws.img_best, on_stream));
        SelectDest dest;
        dest.host_packed = dev_view;
        dest.seq = next_seq(idx->small_seq);
        SSW_TRY(do_select_deep(idx, slab, k, dest, on_stream));
        SSW_TRY(wait_host_seq(on_stream, reinterpret_cast<const unsigned *>(res) + 3, dest.seq));
        if (reran) *reran = true;
    }
    if (hdr[2] != k) {
        set_error("topk slot %d: k=%d does not match the k=%d of the selection that produced the result", slot, k, hdr[2]);
        return SSW_ERR_INVALID;
    }
    decode_packed(res, k, out_images, out_scores, out_best_rows, out_count);
    return SSW_OK;
}

int index_device(const ssw_index *idx) { return idx ? idx->device : -1; }
int32_t index_dtype(const ssw_index *idx) { return idx ? idx->dtype : SSW_DTYPE_F32; }
const void *index_matrix(const ssw_index *idx, int64_t *n_rows, int32_t *dim) {
    if (n_rows) *n_rows = idx->parent ? idx->parent->n : idx->n;  // a view's matrix is its parent's (index_view_rows)
    if (dim) *dim = idx->dim;
    return idx->X;
}
}  // namespace ssw

extern "C" {

ssw_status ssw_index_set_excluded(ssw_index *idx, const int64_t *excluded_images, int64_t n_excluded) {
    SSW_REQUIRE(idx != nullptr, "idx is NULL");
    SSW_REQUIRE(n_excluded == 0 || excluded_images != nullptr, "excluded_images is NULL");
    DeviceGuard guard(idx->device);
    return install_excluded(idx, excluded_images, n_excluded, idx->stream);
}

ssw_status ssw_index_topk_dev(ssw_index *idx, const float *q_dev, int32_t k) {
    SSW_REQUIRE(idx != nullptr, "idx is NULL");
    DeviceGuard guard(idx->device);
    bool candidates = false;
    if (q_dev) SSW_TRY(scan_for_topk(idx, q_dev, k, &candidates));
    else SSW_TRY(ensure_full_scores(idx));
    if (idx->n_images == 0) {  // an empty shard still takes part in the exchange: its message says "0 keys"
        if (idx->ws.xchg.msg_out)
            SSW_HIP_TRY(hipMemsetAsync(idx->ws.xchg.msg_out + (idx->ws.xchg.msg_len - 1), 0, sizeof(uint64_t), idx->stream));
        return SSW_OK;
    }
    return do_select(idx, idx->scores, k, SelectDest(), idx->stream, candidates);
}

// The fast selection keeps at most 8192 candidates; when more images than that share the 24-bit score prefix
// of the k-th score (duplicated vectors, mass ties) it raises the overflow word next to the count
// (ssw_index_result_ptrs: count[1]).  The host-fetching entry points rerun the deep path by themselves;
// callers of the device-resident form read the flag (e.g. after their exchange step) and call this.
ssw_status ssw_index_select_deep_dev(ssw_index *idx, int32_t k) {
    SSW_REQUIRE(idx != nullptr, "idx is NULL");
    SSW_REQUIRE(k >= 1 && k <= SSW_MAX_TOPK, "k=%d outside [1, %d]", k, SSW_MAX_TOPK);
    if (idx->n_images == 0) return SSW_OK;
    DeviceGuard guard(idx->device);
    SSW_TRY(ensure_ws(idx));
    if (idx->scores_partial) {  // the per-image values of the last selection came from a pruned buffer
        SSW_TRY(ensure_full_scores(idx));
        if (idx->has_map)
            SSW_TRY(launch_image_max(idx->scores, idx->row_start, idx->n_images, idx->ws.img_score, idx->ws.img_best,
                                     idx->stream));
    }
    return do_select_deep(idx, idx->scores, k, SelectDest(), idx->stream);
}

ssw_status ssw_index_result_ptrs(ssw_index *idx, void **dev_keys, void **dev_count,
                                 void **dev_best_rows) {
    SSW_REQUIRE(idx != nullptr, "idx is NULL");
    DeviceGuard guard(idx->device);
    SSW_TRY(ensure_ws(idx));
    if (dev_keys) *dev_keys = idx->ws.out_keys;
    if (dev_count) *dev_count = idx->ws.out_count;
    if (dev_best_rows) *dev_best_rows = idx->ws.out_best;
    return SSW_OK;
}

ssw_status ssw_index_topk_fetch(ssw_index *idx, int32_t k, int64_t *out_images, float *out_scores,
                                int64_t *out_best_rows, int32_t *out_count) {
    SSW_REQUIRE(idx != nullptr && out_count != nullptr, "NULL argument");
    DeviceGuard guard(idx->device);
    return fetch_topk(idx, idx->scores, idx->stream, k, out_images, out_scores, out_best_rows, out_count);
}

ssw_status ssw_index_topk(ssw_index *idx, const float *q_host, const int64_t *excluded_images,
                          int64_t n_excluded, int32_t k, int64_t *out_images, float *out_scores,
                          int64_t *out_best_rows, int32_t *out_count) {
    SSW_REQUIRE(idx != nullptr && out_count != nullptr, "NULL argument");
    SSW_REQUIRE(k >= 1 && k <= SSW_MAX_TOPK, "k=%d outside [1, %d]", k, SSW_MAX_TOPK);
    SSW_REQUIRE(n_excluded == 0 || excluded_images != nullptr, "excluded_images is NULL");
    *out_count = 0;
    DeviceGuard guard(idx->device);
    if (q_host) SSW_TRY(check_query(idx, q_host));
    else SSW_TRY(ensure_full_scores(idx));
    SSW_TRY(topk_enqueue(idx, q_host, idx->scores, idx->stream, excluded_images, n_excluded, k));
    return topk_collect(idx, idx->scores, idx->stream, k, out_images, out_scores, out_best_rows, out_count);
}

#ifdef SSW_DEBUG_HOOKS
ssw_status ssw_tune_topk(int32_t flags) {
    g_small_path = (flags & 1) != 0;
    tune_select((flags & 2) != 0);
    return SSW_OK;
}
#endif

}  // extern "C"

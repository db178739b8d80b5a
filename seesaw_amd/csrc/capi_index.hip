// capi_index.hip -- C-ABI of the resident vector index (see include/seesaw_hip.h).
#include <algorithm>
#include <cmath>
#include <chrono>
#include <vector>

#include "ssw_common.h"

namespace ssw {

static thread_local std::string g_last_error;

void set_error(const char *fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
}

int num_cus(int device) {
    static int cache[16] = {0};
    const int slot = device & 15;
    if (cache[slot] == 0) {
        int v = 0;
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess ||
            v <= 0)
            v = 256;
        cache[slot] = v;
    }
    return cache[slot];
}

ssw_status PinnedStage::push(void *dev_dst, const void *src, size_t bytes, hipStream_t stream) {
    if (bytes == 0) return SSW_OK;
    if (pending) {  // the previous copy out of this buffer must have been consumed
        SSW_HIP_TRY(hipEventSynchronize(ev));
        pending = false;
    }
    if (bytes > cap) {
        if (host) (void)hipHostFree(host);
        host = nullptr;
        cap = 0;
        size_t c = 4096;
        while (c < bytes) c <<= 1;
        SSW_HIP_TRY(hipHostMalloc(&host, c, hipHostMallocDefault));
        cap = c;
    }
    if (!ev) SSW_HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    memcpy(host, src, bytes);
    SSW_HIP_TRY(hipMemcpyAsync(dev_dst, host, bytes, hipMemcpyHostToDevice, stream));
    SSW_HIP_TRY(hipEventRecord(ev, stream));
    pending = true;
    return SSW_OK;
}

void PinnedStage::release() {
    if (pending && ev) (void)hipEventSynchronize(ev);
    if (host) (void)hipHostFree(host);
    if (ev) (void)hipEventDestroy(ev);
    host = nullptr;
    ev = nullptr;
    cap = 0;
    pending = false;
}

}  // namespace ssw

using namespace ssw;

// certified int8 pre-scan of the top-k (prune.hip): the shadow of the rows, built lazily by the first top-k with a query
// after the rows last changed, and the buffers of one pruned call
struct PruneState {
    int8_t *q8 = nullptr;                          // [n, dim] codes
    float *q8_scale = nullptr, *q8_err = nullptr;  // [n] s_r, a_r
    bool stale = true;                             // the rows changed since the shadow was built
    bool refused = false;                          // too little free memory at the last attempt (until the rows change)
    unsigned *state = nullptr;                     // [4] device words (ssw_common.h, launch_q8_query)
    int64_t *surv_rows = nullptr;                  // [SURV_CAP]
    float *surv_scores = nullptr;                  // [SURV_CAP]
    int32_t *host = nullptr;                       // pinned, mapped: [seq, survivors or -1]
    unsigned seq = 0;
    hipEvent_t ev = nullptr;                       // after the shadow scan: the host sleeps on it, then spins
    float *q_last = nullptr;                       // [dim] the query of the last pruned scan
    int64_t last = 0, queries = 0, fallbacks = 0;
    void free_shadow() {
        for (void *p : {(void *)q8, (void *)q8_scale, (void *)q8_err}) (void)hipFree(p);
        q8 = nullptr;
        q8_scale = q8_err = nullptr;
        stale = true;
    }
    void release() {
        free_shadow();
        for (void *p : {(void *)state, (void *)surv_rows, (void *)surv_scores, (void *)q_last}) (void)hipFree(p);
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
    int32_t *host = nullptr;       // pinned, mapped: [seq, survivors or -1 of each slot]
    unsigned seq = 0;
    void release() {
        for (void *p : {(void *)mq, (void *)planes, (void *)surv_rows, (void *)surv_scores}) (void)hipFree(p);
        if (host) (void)hipHostFree(host);
    }
};

// batched scan (ssw_index_scan_batch / ssw_index_topk_batch): the queries of one chunk, and the score slabs of all but
// its last query (that one's slab is `scores`); allocated by the first batched call
struct BatchState {
    float *qb_dev = nullptr;  // [BATCH_MAX_WIDTH, dim]
    PinnedStage qb_stage;
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

struct ssw_index {
    int device = 0;
    int64_t n = 0;
    int32_t dim = 0;
    int64_t n_images = 0;
    bool has_map = false;
    int32_t dtype = SSW_DTYPE_F32;
    float *X = nullptr;  // SSW_DTYPE_F16: binary16 rows in the lane-interleaved layout (ssw_common.h)
    bool owns_X = false;
    // f16 upload / download: bounded device staging of natural-order rows (f32 or binary16)
    void *xfer = nullptr;
    size_t xfer_bytes = 0;
    float *scores = nullptr;      // [n]
    float *q_dev = nullptr;       // [dim] device copy of a host query
    PinnedStage q_stage;
    int64_t *row_start = nullptr;  // [n_images + 1] when has_map
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    SelectWorkspace ws;
    bool ws_ready = false;
    // gather staging
    int64_t *gather_idx = nullptr;
    float *gather_out = nullptr;
    int64_t gather_cap = 0;
    PinnedStage rows_stage;
    void *res_host = nullptr;  // pinned result mirror
    // small index (one scan launch + one selection launch, no copies, no stream wait): pinned, device-visible block
    // [query dim f32][excluded ids SMALL_EXCL_CAP i64][packed result], and the sequence number the host spins on
    unsigned char *small_host = nullptr;
    unsigned small_seq = 0;
    unsigned res_pending_seq = 0;  // != 0: the selection in flight publishes into res_host under this sequence number
    unsigned small_pending_seq = 0;  // the same for the small form, into small_host
    float *q2_dev = nullptr;  // second query vector (score_rows)
    PinnedStage q2_stage;
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
    bool scores_partial = false;  // scores hold exact values for the survivors only (ensure_full_scores materialises)
    BatchState batch;
    PruneBatchState prune_batch;
    // profiling of the scan kernel
    bool profiling = false;
    std::vector<hipEvent_t> ev;  // pairs
    int ev_used = 0;
};

static ssw_status ensure_ws(ssw_index *idx) {
    if (idx->ws_ready) return SSW_OK;
    SSW_TRY(select_alloc(idx->ws, idx->n, idx->n_images, idx->has_map));
    idx->ws_ready = true;
    return SSW_OK;
}

static unsigned next_seq(unsigned &counter) {  // sequence numbers are never 0 ("nothing in flight")
    if (++counter == 0) ++counter;
    return counter;
}

static ssw_status check_row_range(const ssw_index *idx, int64_t first_row, int64_t n) {
    SSW_REQUIRE(first_row >= 0 && n >= 0 && first_row + n <= idx->n,
                "rows [%lld, %lld) outside the index of %lld rows", (long long)first_row,
                (long long)(first_row + n), (long long)idx->n);
    return SSW_OK;
}

static ssw_status check_excluded(const ssw_index *idx, const int64_t *ids, int64_t first, int64_t last) {
    for (int64_t i = first; i < last; ++i)
        SSW_REQUIRE(ids[i] >= 0 && ids[i] < idx->n_images, "excluded image %lld outside [0, %lld)", (long long)ids[i],
                    (long long)idx->n_images);
    return SSW_OK;
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

static ssw_status check_query(const ssw_index *idx, const float *q_host) {
    for (int i = 0; i < idx->dim; ++i) {
        if (!std::isfinite(q_host[i])) {
            // the reference asserts on NaN query vectors (seesaw/loops/loop_base.py:47)
            set_error("query vector has a non-finite component at %d", i);
            return SSW_ERR_NUMERIC;
        }
    }
    return SSW_OK;
}

// a host query reaches q_dev through the kernel-argument segment of a one-wave kernel (dim <= 768): a launch is a
// third of what the 2-KB copy and its event cost on the host
constexpr int Q_ARG_FLOATS = 768;
struct QArg {
    float v[Q_ARG_FLOATS];
};
__global__ void k_stage_query(QArg q, float *__restrict__ dst, int dim) {
    for (int i = threadIdx.x; i < dim; i += 256) dst[i] = q.v[i];
}
static ssw_status stage_query(ssw_index *idx, const float *q_host) {
    if (idx->dim > Q_ARG_FLOATS)
        return idx->q_stage.push(idx->q_dev, q_host, (size_t)idx->dim * sizeof(float), idx->stream);
    QArg q;
    memcpy(q.v, q_host, (size_t)idx->dim * sizeof(float));
    hipLaunchKernelGGL(k_stage_query, dim3(1), dim3(256), 0, idx->stream, q, idx->q_dev, idx->dim);
    SSW_HIP_TRY(hipGetLastError());
    return SSW_OK;
}

static ssw_status launch_index_scan(ssw_index *idx, const float *q_dev, hipStream_t stream) {
    return launch_scan(idx->X, idx->dtype, q_dev, idx->scores, idx->n, idx->dim, idx->device, stream);
}

static ssw_status do_scan(ssw_index *idx, const float *q_dev) {
    idx->scores_partial = false;
    return profiled(idx, [&] { return launch_index_scan(idx, q_dev, idx->stream); });
}

// the selection over the row scores in `scores`: per-image maxima first when the index has an image map
static ssw_status do_select(ssw_index *idx, const float *scores, int32_t k, SelectDest dest, hipStream_t stream) {
    SSW_TRY(ensure_ws(idx));
    if (idx->has_map) {
        SSW_TRY(launch_image_max(scores, idx->row_start, idx->n_images, idx->ws.img_score, idx->ws.img_best, stream));
        return launch_select_topk(idx->ws, idx->ws.img_score, idx->n_images, idx->ws.img_best, k, dest, idx->device, stream);
    }
    return launch_select_topk(idx->ws, scores, idx->n, nullptr, k, dest, idx->device, stream);
}

// the deep path over what the last do_select of `scores` left (the per-image maxima are still in the workspace)
static ssw_status do_select_deep(ssw_index *idx, const float *scores, int32_t k, SelectDest dest, hipStream_t stream) {
    const float *values = idx->has_map ? idx->ws.img_score : scores;
    const uint32_t *best = idx->has_map ? idx->ws.img_best : nullptr;
    return launch_select_topk_deep(idx->ws, values, idx->n_images, best, k, dest, idx->device, stream);
}

// ---- the certified pre-scan (prune.hip) -------------------------------------------------------
// Top-k with a query on an index of at least PRUNE_MIN_ROWS f32 rows, or PRUNE_MIN_ROWS_F16 f16 rows, scans the int8
// shadow instead of the rows and rescores the survivors exactly; the score buffer then holds exact scores for the
// survivors and lower bounds elsewhere (scores_partial) until a consumer that reads it materialises the full scan of
// the kept query.
constexpr int64_t PRUNE_MIN_ROWS = (int64_t)1 << 22;  // above the feedback loop's 1.56 M rows, below a rank's 12.5 M
// f16 rows: the full scan reads half the bytes, yet the pruned call is ahead from the smallest size of the measured
// sweep on (2^22 rows: 0.49 against 0.72 ms a call, profiles/prune_f16_sweep.txt), so the value is the f32 one.  Its
// own constant: the two row formats are measured separately and need not stay equal.
constexpr int64_t PRUNE_MIN_ROWS_F16 = (int64_t)1 << 22;
// the pruned batch (ssw_index_topk_batch_pruned) against the plain batch at 16 queries: its own constant, chosen by its
// own sweep ("Pruned batch")
constexpr int64_t PRUNE_BATCH_MIN_ROWS = PRUNE_MIN_ROWS;
constexpr int64_t PRUNE_RESERVE = (int64_t)4 << 30;   // free device memory the shadow must leave
constexpr int64_t SURV_CAP = (int64_t)1 << 18;        // survivors rescored at most; more: the full scan
static SSW_TUNABLE bool g_prune = true;               // ssw_tune_prune
static SSW_TUNABLE int64_t g_prune_min_rows = -1;      // >= 0: this many rows for both dtypes instead
static SSW_TUNABLE int64_t g_prune_reserve = PRUNE_RESERVE;

static bool prune_forced_off() {
    static const bool v = getenv("SSW_TOPK_FULL_SCAN") != nullptr;  // A/B: every top-k runs the full f32 scan
    return v;
}

static int64_t prune_min_rows(const ssw_index *idx) {
    if (g_prune_min_rows >= 0) return g_prune_min_rows;
    return idx->dtype == SSW_DTYPE_F16 ? PRUNE_MIN_ROWS_F16 : PRUNE_MIN_ROWS;
}

static bool prune_eligible_from(const ssw_index *idx, int64_t min_rows) {
    return g_prune && !prune_forced_off() && idx->owns_X && !idx->rows_escaped && idx->n >= min_rows &&
           idx->n_images > 0 && q8_dim_supported(idx->dim);
}
static bool prune_eligible(const ssw_index *idx) { return prune_eligible_from(idx, prune_min_rows(idx)); }
static bool prune_batch_eligible(const ssw_index *idx) {
    return prune_eligible_from(idx, g_prune_min_rows >= 0 ? g_prune_min_rows : PRUNE_BATCH_MIN_ROWS);
}

static ssw_status ensure_full_scores(ssw_index *idx, hipStream_t stream) {
    if (!idx->scores_partial) return SSW_OK;
    idx->scores_partial = false;
    return launch_index_scan(idx, idx->prune.q_last, stream);
}
static ssw_status ensure_full_scores(ssw_index *idx) { return ensure_full_scores(idx, idx->stream); }

// the rows are about to change: the buffer keeps the scores of the rows it was computed from, the shadow goes stale
static ssw_status rows_changing(ssw_index *idx) {
    SSW_TRY(ensure_full_scores(idx));
    idx->prune.stale = true;
    idx->prune.refused = false;
    return SSW_OK;
}

// the candidates' tiles laid end to end: off[c] = first tile of candidate c, their total and the most of one image
static ssw_status candidate_geometry(const ssw_index *idx, const int64_t *image_positions, int32_t m,
                                     std::vector<int64_t> &off, int64_t *total, int64_t *max_tiles) {
    off.resize((size_t)m);
    *total = *max_tiles = 0;
    for (int32_t c = 0; c < m; ++c) {
        const int64_t p = image_positions[c];
        SSW_REQUIRE(p >= 0 && p < idx->n_images, "image position %lld outside [0, %lld)", (long long)p,
                    (long long)idx->n_images);
        const int64_t t = idx->row_start_host[(size_t)p + 1] - idx->row_start_host[(size_t)p];
        off[(size_t)c] = *total;
        *total += t;
        *max_tiles = std::max(*max_tiles, t);
    }
    return SSW_OK;
}

static ssw_status install_excluded(ssw_index *idx, const int64_t *excluded_images, int64_t n_excluded, hipStream_t stream) {
    SSW_TRY(check_excluded(idx, excluded_images, 0, n_excluded));
    SSW_TRY(ensure_ws(idx));
    return select_set_excluded(idx->ws, idx->n_images, excluded_images, n_excluded, stream);
}

static ssw_status scan_for_topk(ssw_index *idx, const float *q_dev, int32_t k);

extern "C" {

int32_t ssw_abi_version(void) { return SSW_ABI_VERSION; }
const char *ssw_last_error(void) { return g_last_error.c_str(); }

ssw_status ssw_device_count(int32_t *out_count) {
    SSW_REQUIRE(out_count != nullptr, "out_count is NULL");
    int c = 0;
    SSW_HIP_TRY(hipGetDeviceCount(&c));
    *out_count = c;
    return SSW_OK;
}

ssw_status ssw_device_info(int32_t device, char *name, int32_t name_cap, int32_t *out_cus,
                           int64_t *out_hbm_bytes) {
    hipDeviceProp_t p;
    SSW_HIP_TRY(hipGetDeviceProperties(&p, device));
    if (name && name_cap > 0) {
        snprintf(name, (size_t)name_cap, "%s (%s)", p.name, p.gcnArchName);
    }
    if (out_cus) *out_cus = p.multiProcessorCount;
    if (out_hbm_bytes) *out_hbm_bytes = (int64_t)p.totalGlobalMem;
    return SSW_OK;
}

ssw_status ssw_index_create(int32_t device, int64_t n_rows, int32_t dim,
                            const float *dev_vectors_or_null, ssw_index **out) {
    return ssw_index_create_typed(device, n_rows, dim, SSW_DTYPE_F32, dev_vectors_or_null, out);
}

ssw_status ssw_index_create_typed(int32_t device, int64_t n_rows, int32_t dim, int32_t dtype,
                                  const void *dev_vectors_or_null, ssw_index **out) {
    SSW_REQUIRE(out != nullptr, "out is NULL");
    *out = nullptr;
    SSW_REQUIRE(n_rows >= 0, "n_rows=%lld < 0", (long long)n_rows);
    if (dtype != SSW_DTYPE_F32 && dtype != SSW_DTYPE_F16) {
        set_error("index: dtype=%d unsupported (SSW_DTYPE_F32 = 0, SSW_DTYPE_F16 = 1)", dtype);
        return SSW_ERR_UNSUPPORTED;
    }
    if (dtype == SSW_DTYPE_F16 && dev_vectors_or_null) {
        set_error("index: an f16 index keeps its rows in a private layout and cannot borrow a device matrix");
        return SSW_ERR_UNSUPPORTED;
    }
    if (dim <= 0 || dim % 256 != 0 || dim > 1024) {
        set_error("index: dim=%d unsupported (need a multiple of 256, <= 1024)", dim);
        return SSW_ERR_UNSUPPORTED;
    }
    if (n_rows >= (int64_t)0x7fff0000) {
        set_error("index: %lld rows exceed the 2^31 row limit of one shard", (long long)n_rows);
        return SSW_ERR_UNSUPPORTED;
    }
    SSW_REQUIRE(((uintptr_t)dev_vectors_or_null & 15) == 0, "device matrix is not 16-byte aligned");
    DeviceGuard guard(device);
    if (!guard.ok) {
        set_error("hipSetDevice(%d) failed", device);
        return SSW_ERR_HIP;
    }
    ssw_index *idx = new (std::nothrow) ssw_index();
    if (!idx) return SSW_ERR_NOMEM;
    idx->device = device;
    idx->n = n_rows;
    idx->dim = dim;
    idx->dtype = dtype;
    idx->n_images = n_rows;
    ssw_status st = SSW_OK;
    auto fail = [&](ssw_status s) {
        ssw_index_destroy(idx);
        return s;
    };
    if (hipStreamCreateWithFlags(&idx->own_stream, hipStreamNonBlocking) != hipSuccess) {
        set_error("hipStreamCreate failed");
        return fail(SSW_ERR_HIP);
    }
    idx->stream = idx->own_stream;
    const size_t row_bytes = (size_t)dim * sizeof(float);
    const size_t elem_bytes = dtype == SSW_DTYPE_F16 ? 2 : 4;
    if (dev_vectors_or_null) {
        idx->X = const_cast<float *>(static_cast<const float *>(dev_vectors_or_null));
    } else {
        hipError_t e = hipMalloc((void **)&idx->X, (size_t)(n_rows > 0 ? n_rows : 1) * dim * elem_bytes);
        if (e != hipSuccess) {
            set_error("hipMalloc of %.2f GB for the index failed: %s",
                      (double)n_rows * dim * elem_bytes / 1e9, hipGetErrorString(e));
            idx->X = nullptr;
            return fail(SSW_ERR_NOMEM);
        }
        idx->owns_X = true;
    }
    if (hipMalloc((void **)&idx->scores, (size_t)(n_rows + 64) * sizeof(float)) != hipSuccess ||
        hipMalloc((void **)&idx->q_dev, row_bytes) != hipSuccess) {
        set_error("hipMalloc of the score buffer failed");
        return fail(SSW_ERR_NOMEM);
    }
    (void)st;
    *out = idx;
    return SSW_OK;
}

ssw_status ssw_index_destroy(ssw_index *idx) {
    if (!idx) return SSW_OK;
    DeviceGuard guard(idx->device);
    if (idx->own_stream) (void)hipStreamSynchronize(idx->own_stream);
    for (hipEvent_t e : idx->ev) (void)hipEventDestroy(e);
    if (idx->ws_ready) select_free(idx->ws);
    idx->prune.release();
    idx->batch.release();
    idx->prune_batch.release();
    if (idx->owns_X) (void)hipFree(idx->X);
    (void)hipFree(idx->xfer);
    (void)hipFree(idx->scores);
    (void)hipFree(idx->q_dev);
    idx->q_stage.release();
    (void)hipFree(idx->tile_boxes);
    (void)hipFree(idx->tile_zoom);
    (void)hipFree(idx->rs_pos);
    (void)hipFree(idx->rs_off);
    (void)hipFree(idx->rs_row);
    (void)hipFree(idx->rs_score);
    (void)hipFree(idx->rs_minus);
    (void)hipFree(idx->row_start);
    (void)hipFree(idx->gather_idx);
    (void)hipFree(idx->gather_out);
    (void)hipFree(idx->q2_dev);
    idx->rows_stage.release();
    if (idx->res_host) (void)hipHostFree(idx->res_host);
    if (idx->small_host) (void)hipHostFree(idx->small_host);
    idx->q2_stage.release();
    if (idx->own_stream) (void)hipStreamDestroy(idx->own_stream);
    delete idx;
    return SSW_OK;
}

ssw_status ssw_index_set_stream(ssw_index *idx, void *hip_stream) {
    SSW_REQUIRE(idx != nullptr, "idx is NULL");
    DeviceGuard guard(idx->device);
    SSW_HIP_TRY(hipStreamSynchronize(idx->stream));
    idx->stream = hip_stream ? (hipStream_t)hip_stream : idx->own_stream;
    return SSW_OK;
}

ssw_status ssw_index_sync(ssw_index *idx) {
    SSW_REQUIRE(idx != nullptr, "idx is NULL");
    DeviceGuard guard(idx->device);
    SSW_HIP_TRY(hipStreamSynchronize(idx->stream));
    return SSW_OK;
}

ssw_status ssw_index_shape(const ssw_index *idx, int64_t *n_rows, int32_t *dim, int64_t *n_images) {
    SSW_REQUIRE(idx != nullptr, "idx is NULL");
    if (n_rows) *n_rows = idx->n;
    if (dim) *dim = idx->dim;
    if (n_images) *n_images = idx->n_images;
    return SSW_OK;
}

ssw_status ssw_index_dtype(const ssw_index *idx, int32_t *out) {
    SSW_REQUIRE(idx != nullptr && out != nullptr, "NULL argument");
    *out = idx->dtype;
    return SSW_OK;
}

ssw_status ssw_index_device_ptrs(ssw_index *idx, void **dev_vectors, void **dev_scores) {
    SSW_REQUIRE(idx != nullptr, "idx is NULL");
    DeviceGuard guard(idx->device);
    SSW_TRY(ensure_full_scores(idx));
    if (dev_vectors) {  // the caller may write the rows through it: no shadow from now on
        idx->rows_escaped = true;
        SSW_HIP_TRY(hipStreamSynchronize(idx->stream));
        idx->prune.free_shadow();
        *dev_vectors = idx->X;
    }
    if (dev_scores) *dev_scores = idx->scores;
    return SSW_OK;
}

// f16 index: host rows go through a bounded device staging buffer (never an n x dim x 4 temporary)
constexpr size_t XFER_BYTES = (size_t)32 << 20;

static ssw_status ensure_xfer(ssw_index *idx) {
    if (idx->xfer) return SSW_OK;
    if (hipMalloc(&idx->xfer, XFER_BYTES) != hipSuccess) {
        idx->xfer = nullptr;
        set_error("hipMalloc of the %zu-byte f16 staging buffer failed", XFER_BYTES);
        return SSW_ERR_NOMEM;
    }
    idx->xfer_bytes = XFER_BYTES;
    return SSW_OK;
}

// natural-order host rows (f32, or binary16 when src_h16) -> rows [first_row, first_row + n) of an f16 index
static ssw_status upload_h16(ssw_index *idx, const void *host_rows, bool src_h16, int64_t first_row, int64_t n) {
    SSW_TRY(ensure_xfer(idx));
    const size_t row_bytes = (size_t)idx->dim * (src_h16 ? 2 : 4);
    const int64_t chunk = (int64_t)(idx->xfer_bytes / row_bytes);
    const unsigned char *src = static_cast<const unsigned char *>(host_rows);
    for (int64_t r = 0; r < n; r += chunk) {
        const int64_t m = std::min(chunk, n - r);
        // stream order: the copy into the staging buffer waits for the previous chunk's conversion
        SSW_HIP_TRY(hipMemcpyAsync(idx->xfer, src + (size_t)r * row_bytes, (size_t)m * row_bytes, hipMemcpyHostToDevice,
                                   idx->stream));
        SSW_TRY(launch_rows_to_h16(src_h16 ? nullptr : static_cast<const float *>(idx->xfer),
                                   src_h16 ? static_cast<const uint16_t *>(idx->xfer) : nullptr, m, idx->dim,
                                   reinterpret_cast<uint16_t *>(idx->X) + (first_row + r) * idx->dim, idx->stream));
    }
    SSW_HIP_TRY(hipStreamSynchronize(idx->stream));
    return SSW_OK;
}

ssw_status ssw_index_upload(ssw_index *idx, const float *host_rows, int64_t first_row, int64_t n) {
    SSW_REQUIRE(idx != nullptr && host_rows != nullptr, "NULL argument");
    SSW_TRY(check_row_range(idx, first_row, n));
    DeviceGuard guard(idx->device);
    SSW_TRY(rows_changing(idx));
    if (idx->dtype == SSW_DTYPE_F16) return upload_h16(idx, host_rows, false, first_row, n);
    SSW_HIP_TRY(hipMemcpyAsync(idx->X + first_row * idx->dim, host_rows,
                               (size_t)n * idx->dim * sizeof(float), hipMemcpyHostToDevice,
                               idx->stream));
    SSW_HIP_TRY(hipStreamSynchronize(idx->stream));
    return SSW_OK;
}

ssw_status ssw_index_upload_f16(ssw_index *idx, const uint16_t *rows_f16, int64_t first_row, int64_t n) {
    SSW_REQUIRE(idx != nullptr && rows_f16 != nullptr, "NULL argument");
    if (idx->dtype != SSW_DTYPE_F16) {
        set_error("ssw_index_upload_f16: the index holds f32 rows (use ssw_index_upload)");
        return SSW_ERR_UNSUPPORTED;
    }
    SSW_TRY(check_row_range(idx, first_row, n));
    DeviceGuard guard(idx->device);
    SSW_TRY(rows_changing(idx));
    return upload_h16(idx, rows_f16, true, first_row, n);
}

ssw_status ssw_index_download(ssw_index *idx, float *host_rows, int64_t first_row, int64_t n) {
    SSW_REQUIRE(idx != nullptr && host_rows != nullptr, "NULL argument");
    SSW_TRY(check_row_range(idx, first_row, n));
    DeviceGuard guard(idx->device);
    if (idx->dtype == SSW_DTYPE_F16) {  // widened, natural element order, through the staging buffer
        SSW_TRY(ensure_xfer(idx));
        const size_t row_bytes = (size_t)idx->dim * sizeof(float);
        const int64_t chunk = (int64_t)(idx->xfer_bytes / row_bytes);
        for (int64_t r = 0; r < n; r += chunk) {
            const int64_t m = std::min(chunk, n - r);
            SSW_TRY(launch_gather_rows(idx->X, idx->dtype, nullptr, first_row + r, m, idx->dim,
                                       static_cast<float *>(idx->xfer), idx->stream));
            SSW_HIP_TRY(hipMemcpyAsync(host_rows + (size_t)r * idx->dim, idx->xfer, (size_t)m * row_bytes,
                                       hipMemcpyDeviceToHost, idx->stream));
        }
        SSW_HIP_TRY(hipStreamSynchronize(idx->stream));
        return SSW_OK;
    }
    SSW_HIP_TRY(hipMemcpyAsync(host_rows, idx->X + first_row * idx->dim,
                               (size_t)n * idx->dim * sizeof(float), hipMemcpyDeviceToHost,
                               idx->stream));
    SSW_HIP_TRY(hipStreamSynchronize(idx->stream));
    return SSW_OK;
}

ssw_status ssw_index_fill_random(ssw_index *idx, uint64_t seed, int64_t global_first_row) {
    SSW_REQUIRE(idx != nullptr, "idx is NULL");
    DeviceGuard guard(idx->device);
    SSW_TRY(rows_changing(idx));
    SSW_TRY(launch_fill_random(idx->X, idx->dtype, idx->n, idx->dim, seed, global_first_row, idx->stream));
    SSW_HIP_TRY(hipStreamSynchronize(idx->stream));
    return SSW_OK;
}

ssw_status ssw_index_set_row2image(ssw_index *idx, const int32_t *row2image_host, int64_t n_images) {
    SSW_REQUIRE(idx != nullptr, "idx is NULL");
    DeviceGuard guard(idx->device);
    SSW_HIP_TRY(hipStreamSynchronize(idx->stream));
    if (idx->ws_ready) {
        select_free(idx->ws);
        idx->ws_ready = false;
    }
    (void)hipFree(idx->row_start);
    idx->row_start = nullptr;
    idx->row_start_host.clear();
    idx->max_image_tiles = -1;
    if (row2image_host == nullptr) {
        idx->has_map = false;
        idx->n_images = idx->n;
        return SSW_OK;
    }
    SSW_REQUIRE(n_images >= 0 && n_images <= idx->n, "n_images=%lld outside [0, n_rows]",
                (long long)n_images);
    std::vector<int64_t> start((size_t)n_images + 1, 0);
    int32_t prev = 0;
    for (int64_t r = 0; r < idx->n; ++r) {
        const int32_t m = row2image_host[r];
        if (m < prev || m >= n_images) {
            set_error("row2image[%lld]=%d is not non-decreasing within [0, %lld)", (long long)r, m,
                      (long long)n_images);
            return SSW_ERR_INVALID;
        }
        prev = m;
        start[(size_t)m + 1]++;
    }
    for (int64_t m = 0; m < n_images; ++m) {
        if (start[(size_t)m + 1] == 0) {
            set_error("image position %lld has no rows", (long long)m);
            return SSW_ERR_INVALID;
        }
        start[(size_t)m + 1] += start[(size_t)m];
    }
    SSW_HIP_TRY(hipMalloc((void **)&idx->row_start, ((size_t)n_images + 1) * sizeof(int64_t)));
    SSW_HIP_TRY(hipMemcpy(idx->row_start, start.data(), ((size_t)n_images + 1) * sizeof(int64_t),
                          hipMemcpyHostToDevice));
    idx->row_start_host = std::move(start);
    idx->has_map = true;
    idx->n_images = n_images;
    return SSW_OK;
}

ssw_status ssw_index_set_tile_meta(ssw_index *idx, const float *boxes_host, const int32_t *zoom_host) {
    SSW_REQUIRE(idx != nullptr && boxes_host != nullptr && zoom_host != nullptr, "NULL argument");
    DeviceGuard guard(idx->device);
    for (int64_t r = 0; r < idx->n; ++r)
        SSW_REQUIRE(zoom_host[r] >= 0 && zoom_host[r] <= SSW_RESCORE_MAX_ZOOM, "zoom_level[%lld]=%d outside [0, %d]",
                    (long long)r, zoom_host[r], SSW_RESCORE_MAX_ZOOM);
    SSW_HIP_TRY(hipStreamSynchronize(idx->stream));
    if (!idx->tile_boxes) SSW_HIP_TRY(hipMalloc((void **)&idx->tile_boxes, (size_t)std::max<int64_t>(idx->n, 1) * 16));
    if (!idx->tile_zoom) SSW_HIP_TRY(hipMalloc((void **)&idx->tile_zoom, (size_t)std::max<int64_t>(idx->n, 1) * 4));
    SSW_HIP_TRY(hipMemcpy(idx->tile_boxes, boxes_host, (size_t)idx->n * 16, hipMemcpyHostToDevice));
    SSW_HIP_TRY(hipMemcpy(idx->tile_zoom, zoom_host, (size_t)idx->n * 4, hipMemcpyHostToDevice));
    return SSW_OK;
}

ssw_status ssw_index_rescore_avg(ssw_index *idx, const int64_t *image_positions, int32_t m, int32_t aug_larger,
                                 const float *minus_scores_or_null, float *out_scores, int64_t *out_best_rows) {
    SSW_REQUIRE(idx != nullptr, "idx is NULL");
    if (m <= 0) return SSW_OK;
    SSW_REQUIRE(image_positions && out_scores && out_best_rows, "NULL argument");
    SSW_REQUIRE(aug_larger >= 0 && (aug_larger & 3) <= 2 && aug_larger <= 6,
                "aug_larger=%d is not 0 (all), 1 (greater) or 2 (adjacent), optionally + 4 (aug_weight = cont_weighted)", aug_larger);
    SSW_REQUIRE(idx->has_map && idx->tile_boxes && idx->tile_zoom,
                "rescore_avg needs ssw_index_set_row2image and ssw_index_set_tile_meta first");
    DeviceGuard guard(idx->device);
    SSW_TRY(ensure_full_scores(idx));
    std::vector<int64_t> off;
    int64_t total = 0, max_tiles = 0;
    SSW_TRY(candidate_geometry(idx, image_positions, m, off, &total, &max_tiles));
    SSW_REQUIRE(max_tiles <= SSW_RESCORE_MAX_TILES, "an image with %lld tiles exceeds the %d the kernel keeps in LDS",
                (long long)max_tiles, SSW_RESCORE_MAX_TILES);
    hipStream_t s = idx->stream;
    if (m > idx->rs_cap) {
        SSW_HIP_TRY(hipStreamSynchronize(s));
        for (void *q : {(void *)idx->rs_pos, (void *)idx->rs_off, (void *)idx->rs_row, (void *)idx->rs_score}) (void)hipFree(q);
        idx->rs_pos = idx->rs_off = idx->rs_row = nullptr;
        idx->rs_score = nullptr;
        idx->rs_cap = 0;
        int64_t cap = 256;
        while (cap < m) cap <<= 1;
        SSW_HIP_TRY(hipMalloc((void **)&idx->rs_pos, (size_t)cap * 8));
        SSW_HIP_TRY(hipMalloc((void **)&idx->rs_off, (size_t)cap * 8));
        SSW_HIP_TRY(hipMalloc((void **)&idx->rs_row, (size_t)cap * 8));
        SSW_HIP_TRY(hipMalloc((void **)&idx->rs_score, (size_t)cap * 4));
        idx->rs_cap = cap;
    }
    if (minus_scores_or_null && total > idx->rs_minus_cap) {
        SSW_HIP_TRY(hipStreamSynchronize(s));
        (void)hipFree(idx->rs_minus);
        idx->rs_minus = nullptr;
        idx->rs_minus_cap = 0;
        int64_t cap = 4096;
        while (cap < total) cap <<= 1;
        SSW_HIP_TRY(hipMalloc((void **)&idx->rs_minus, (size_t)cap * 4));
        idx->rs_minus_cap = cap;
    }
    // inputs are a few hundred bytes: plain synchronous copies from the caller's buffers (ordered before the launch)
    SSW_HIP_TRY(hipMemcpyAsync(idx->rs_pos, image_positions, (size_t)m * 8, hipMemcpyHostToDevice, s));
    SSW_HIP_TRY(hipMemcpyAsync(idx->rs_off, off.data(), (size_t)m * 8, hipMemcpyHostToDevice, s));
    if (minus_scores_or_null)
        SSW_HIP_TRY(hipMemcpyAsync(idx->rs_minus, minus_scores_or_null, (size_t)total * 4, hipMemcpyHostToDevice, s));
    SSW_HIP_TRY(hipStreamSynchronize(s));  // `off` is a local; pageable sources are staged by now
    SSW_TRY(launch_avg_score(idx->tile_boxes, idx->tile_zoom, idx->scores, minus_scores_or_null ? idx->rs_minus : nullptr,
                             idx->row_start, idx->rs_pos, idx->rs_off, m, (int32_t)max_tiles, aug_larger,
                             idx->rs_score, idx->rs_row, s));
    SSW_HIP_TRY(hipMemcpyAsync(out_scores, idx->rs_score, (size_t)m * 4, hipMemcpyDeviceToHost, s));
    SSW_HIP_TRY(hipMemcpyAsync(out_best_rows, idx->rs_row, (size_t)m * 8, hipMemcpyDeviceToHost, s));
    SSW_HIP_TRY(hipStreamSynchronize(s));
    return SSW_OK;
}

ssw_status ssw_index_rescore_avg_f64(ssw_index *idx, const double *dev_scores, const int64_t *image_positions, int32_t m,
                                     int32_t aug_larger, double *out_scores, int64_t *out_best_rows) {
    SSW_REQUIRE(idx != nullptr, "idx is NULL");
    if (m <= 0) return SSW_OK;
    SSW_REQUIRE(dev_scores && image_positions && out_scores && out_best_rows, "NULL argument");
    SSW_REQUIRE(aug_larger >= 0 && (aug_larger & 3) <= 2 && aug_larger <= 6,
                "aug_larger=%d is not 0 (all), 1 (greater) or 2 (adjacent), optionally + 4 (aug_weight = cont_weighted)", aug_larger);
    SSW_REQUIRE(idx->has_map && idx->tile_boxes && idx->tile_zoom,
                "rescore_avg needs ssw_index_set_row2image and ssw_index_set_tile_meta first");
    DeviceGuard guard(idx->device);
    std::vector<int64_t> off;
    int64_t total = 0, max_tiles = 0;
    SSW_TRY(candidate_geometry(idx, image_positions, m, off, &total, &max_tiles));
    hipStream_t s = idx->stream;
    int64_t *d_pos = nullptr, *d_off = nullptr, *d_row = nullptr;
    double *d_score = nullptr;
    auto release = [&]() {
        for (void *q : {(void *)d_pos, (void *)d_off, (void *)d_row, (void *)d_score}) (void)hipFree(q);
    };
    // (a few hundred bytes per call and one call per round of a graph loop: plain allocations keep this entry
    //  independent of the f32 path's cached buffers)
    if (hipMalloc((void **)&d_pos, (size_t)m * 8) != hipSuccess || hipMalloc((void **)&d_off, (size_t)m * 8) != hipSuccess ||
        hipMalloc((void **)&d_row, (size_t)m * 8) != hipSuccess || hipMalloc((void **)&d_score, (size_t)m * 8) != hipSuccess) {
        release();
        set_error("rescore_avg_f64: allocation failed");
        return SSW_ERR_NOMEM;
    }
    ssw_status rc = SSW_OK;
    hipError_t e = hipMemcpyAsync(d_pos, image_positions, (size_t)m * 8, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d_off, off.data(), (size_t)m * 8, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e == hipSuccess)
        rc = launch_avg_score_f64(idx->tile_boxes, idx->tile_zoom, dev_scores, idx->row_start, d_pos, d_off, m,
                                  (int32_t)max_tiles, aug_larger, d_score, d_row, s);
    if (e == hipSuccess && rc == SSW_OK) e = hipMemcpyAsync(out_scores, d_score, (size_t)m * 8, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && rc == SSW_OK) e = hipMemcpyAsync(out_best_rows, d_row, (size_t)m * 8, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    else (void)hipStreamSynchronize(s);
    release();
    if (rc != SSW_OK) return rc;
    if (e != hipSuccess) {
        set_error("rescore_avg_f64: %s", hipGetErrorString(e));
        return SSW_ERR_HIP;
    }
    return SSW_OK;
}

ssw_status ssw_index_scan_dev(ssw_index *idx, const float *q_dev) {
    SSW_REQUIRE(idx != nullptr && q_dev != nullptr, "NULL argument");
    DeviceGuard guard(idx->device);
    return do_scan(idx, q_dev);
}

ssw_status ssw_index_scan(ssw_index *idx, const float *q_host, float *out_scores_host_or_null) {
    SSW_REQUIRE(idx != nullptr && q_host != nullptr, "NULL argument");
    SSW_TRY(check_query(idx, q_host));
    DeviceGuard guard(idx->device);
    SSW_TRY(idx->q_stage.push(idx->q_dev, q_host, (size_t)idx->dim * sizeof(float), idx->stream));
    SSW_TRY(do_scan(idx, idx->q_dev));
    if (out_scores_host_or_null && idx->n > 0) {
        SSW_HIP_TRY(hipMemcpyAsync(out_scores_host_or_null, idx->scores,
                                   (size_t)idx->n * sizeof(float), hipMemcpyDeviceToHost,
                                   idx->stream));
    }
    SSW_HIP_TRY(hipStreamSynchronize(idx->stream));
    return SSW_OK;
}

ssw_status ssw_index_load_scores(ssw_index *idx, const float *scores_host) {
    SSW_REQUIRE(idx != nullptr && (idx->n == 0 || scores_host != nullptr), "NULL argument");
    DeviceGuard guard(idx->device);
    idx->scores_partial = false;  // the whole buffer is overwritten
    if (idx->n > 0) {
        SSW_HIP_TRY(hipMemcpyAsync(idx->scores, scores_host, (size_t)idx->n * sizeof(float),
                                   hipMemcpyHostToDevice, idx->stream));
        SSW_HIP_TRY(hipStreamSynchronize(idx->stream));
    }
    return SSW_OK;
}

ssw_status ssw_index_set_excluded(ssw_index *idx, const int64_t *excluded_images, int64_t n_excluded) {
    SSW_REQUIRE(idx != nullptr, "idx is NULL");
    SSW_REQUIRE(n_excluded == 0 || excluded_images != nullptr, "excluded_images is NULL");
    DeviceGuard guard(idx->device);
    return install_excluded(idx, excluded_images, n_excluded, idx->stream);
}

ssw_status ssw_index_topk_dev(ssw_index *idx, const float *q_dev, int32_t k) {
    SSW_REQUIRE(idx != nullptr, "idx is NULL");
    DeviceGuard guard(idx->device);
    if (q_dev) SSW_TRY(scan_for_topk(idx, q_dev, k));
    else SSW_TRY(ensure_full_scores(idx));
    if (idx->n_images == 0) {  // an empty shard still takes part in the exchange: its message says "0 keys"
        if (idx->ws.xchg.msg_out)
            SSW_HIP_TRY(hipMemsetAsync(idx->ws.xchg.msg_out + (idx->ws.xchg.msg_len - 1), 0, sizeof(uint64_t), idx->stream));
        return SSW_OK;
    }
    return do_select(idx, idx->scores, k, SelectDest(), idx->stream);
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

static ssw_status wait_host_seq(hipStream_t stream, const unsigned *flag, unsigned seq) {
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

// shadow of the rows for the pruned scan: (re)built when stale, if the device keeps PRUNE_RESERVE free beside it
static ssw_status ensure_shadow(ssw_index *idx, bool *ready) {
    PruneState &p = idx->prune;
    *ready = false;
    if (p.q8 && !p.stale) {
        *ready = true;
        return SSW_OK;
    }
    if (p.refused) return SSW_OK;
    if (!p.q8) {
        const size_t codes = (size_t)idx->n * idx->dim, consts = (size_t)idx->n * sizeof(float);
        size_t free_b = 0, total_b = 0;
        SSW_HIP_TRY(hipMemGetInfo(&free_b, &total_b));
        const size_t need = codes + 2 * consts + (size_t)SURV_CAP * 12 + ((size_t)idx->dim + 64) * sizeof(float);
        if (free_b < need || free_b - need < (size_t)g_prune_reserve) {
            p.refused = true;
            return SSW_OK;
        }
        if (hipMalloc((void **)&p.q8, codes) != hipSuccess || hipMalloc((void **)&p.q8_scale, consts) != hipSuccess ||
            hipMalloc((void **)&p.q8_err, consts) != hipSuccess) {
            (void)hipGetLastError();
            p.free_shadow();
            p.refused = true;
            return SSW_OK;
        }
    }
    if (!p.state) {
        SSW_HIP_TRY(hipMalloc((void **)&p.state, 4 * sizeof(unsigned)));
        SSW_HIP_TRY(hipMalloc((void **)&p.surv_rows, (size_t)SURV_CAP * sizeof(int64_t)));
        SSW_HIP_TRY(hipMalloc((void **)&p.surv_scores, (size_t)SURV_CAP * sizeof(float)));
        SSW_HIP_TRY(hipMalloc((void **)&p.q_last, (size_t)idx->dim * sizeof(float)));
        SSW_HIP_TRY(hipHostMalloc((void **)&p.host, 16, hipHostMallocMapped | hipHostMallocCoherent));
        memset(p.host, 0, 16);
        SSW_HIP_TRY(hipEventCreateWithFlags(&p.ev, hipEventDisableTiming));
    }
    SSW_TRY(launch_q8_build(idx->X, idx->dtype, idx->n, idx->dim, p.q8, p.q8_scale, p.q8_err, idx->stream));
    p.stale = false;
    *ready = true;
    return SSW_OK;
}

// The two steps of the pre-scan that the lab hooks (ssw_debug_prune_*) drive as well; the shadow is ready.
// Lower bounds of the scores of q_dev into the buffer, which is partial from here on: a consumer rescans q_last.
static ssw_status prune_bounds(ssw_index *idx, const float *q_dev) {
    PruneState &p = idx->prune;
    SSW_TRY(launch_q8_query(q_dev, idx->dim, p.q_last, p.state, idx->stream));
    SSW_TRY(launch_q8_bounds(p.q8, p.q8_scale, p.q8_err, p.q_last, p.state, idx->scores, idx->n, idx->dim, idx->device,
                             idx->stream));
    idx->scores_partial = true;
    return SSW_OK;
}

// The rows that may still reach the k-th key of the last selection, at most cap of them -> *out_m = their published
// count, -1 = run the full scan.  One host wait: a sleep on sleep_ev_or_null first, then a spin.
static ssw_status prune_survivors(ssw_index *idx, int32_t k, int64_t cap, hipEvent_t sleep_ev_or_null, int32_t *out_m) {
    PruneState &p = idx->prune;
    const unsigned seq = next_seq(p.seq);
    int32_t *host_dev = nullptr;
    SSW_HIP_TRY(hipHostGetDevicePointer((void **)&host_dev, p.host, 0));
    SSW_TRY(launch_survivors(idx->scores, p.q8_err, idx->n, idx->ws.out_keys, idx->ws.out_count, k, p.state, p.surv_rows, cap,
                             host_dev, seq, idx->device, idx->stream));
    if (sleep_ev_or_null) SSW_HIP_TRY(hipEventSynchronize(sleep_ev_or_null));
    SSW_TRY(wait_host_seq(idx->stream, reinterpret_cast<const unsigned *>(p.host), seq));
    *out_m = __atomic_load_n(p.host + 1, __ATOMIC_ACQUIRE);
    return SSW_OK;
}

// The score buffer for the selection of the top-k of query q_dev (exclusions installed): the full f32 scan, or on a
// large index the certified pre-scan -- shadow scan (lower bounds), threshold selection over them that publishes
// nothing, survivors, exact rescoring of the survivors.  One host wait for the survivor count; any failure of the
// certificate (fewer than k keys or an overflow in the threshold selection, more survivors than SURV_CAP, a query
// that cannot be bounded) runs the full scan instead.  The profiling events bracket the whole replacement.
static ssw_status scan_for_topk(ssw_index *idx, const float *q_dev, int32_t k) {
    bool ready = false;
    const bool k_ok = k >= 1 && k <= SSW_MAX_TOPK && (idx->ws.xchg.msg_out == nullptr || k <= idx->ws.xchg.k_max);
    if (k_ok && prune_eligible(idx)) SSW_TRY(ensure_shadow(idx, &ready));
    if (!ready) return do_scan(idx, q_dev);
    SSW_TRY(ensure_ws(idx));
    return profiled(idx, [&]() -> ssw_status {
        PruneState &p = idx->prune;
        SSW_TRY(prune_bounds(idx, q_dev));
        SSW_HIP_TRY(hipEventRecord(p.ev, idx->stream));
        // threshold: the ordinary selection over the lower bounds, with the exclusions, without a message or host result
        SSW_TRY(do_select(idx, idx->scores, k, SelectDest{nullptr, 0u, false}, idx->stream));
        int32_t m = -1;
        SSW_TRY(prune_survivors(idx, k, SURV_CAP, p.ev, &m));  // sleep through the shadow scan, spin on the rest
        p.last = m;
        ++p.queries;
        if (m < 0) {
            ++p.fallbacks;
            idx->scores_partial = false;
            return launch_index_scan(idx, p.q_last, idx->stream);
        }
        SSW_TRY(launch_score_rows(idx->X, idx->dtype, p.q_last, p.surv_rows, m, idx->dim, p.surv_scores, idx->stream));
        return launch_scatter_scores(p.surv_rows, p.surv_scores, m, idx->scores, idx->stream);
    });
}

ssw_status ssw_index_prune_stats(ssw_index *idx, int64_t *out6) {
    SSW_REQUIRE(idx != nullptr && out6 != nullptr, "NULL argument");
    const PruneState &p = idx->prune;
    out6[0] = p.q8 ? (p.stale ? 2 : 1) : (p.refused ? 3 : 0);
    out6[1] = prune_eligible(idx) ? 1 : 0;
    out6[2] = p.last;
    out6[3] = p.queries;
    out6[4] = p.fallbacks;
    out6[5] = p.q8 ? idx->n * (idx->dim + 8) : 0;
    return SSW_OK;
}

// ---- top-k of row scores that are resident on the device -> host: ONE path, in an enqueue and a collect half ----------
// An index of a few thousand images (an LVIS-category subset: 1 109 images x 13 tiles) spends its round in fixed
// costs, not in the scan: three copies, five launches and a stream wait were ~95 us around ~10 us of kernels.  Its form
// is three launches and no copy: the query goes to q_dev through a kernel argument, the scan runs on every CU, and ONE
// kernel takes the per-image maximum, strikes out the excluded ids (read from pinned memory the device maps), selects
// and writes the packed result into the same pinned block, releasing a sequence word the host spins on.
constexpr int64_t SMALL_EXCL_CAP = 8192;
constexpr int64_t SMALL_ROWS = 65536;  // the small scan kernel's range (scan.hip)

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
static ssw_status select_to_host(ssw_index *idx, const float *scores, hipStream_t stream, int32_t k, bool deep) {
    SSW_TRY(ensure_ws(idx));
    SSW_TRY(ensure_res_host(idx));
    SelectDest dest;
    SSW_HIP_TRY(hipHostGetDevicePointer((void **)&dest.host_packed, idx->res_host, 0));
    dest.seq = idx->res_pending_seq = next_seq(idx->small_seq);
    idx->small_pending_seq = 0;  // this selection is the one in flight: topk_collect reads res_host
    const ssw_status st = deep ? do_select_deep(idx, scores, k, dest, stream) : do_select(idx, scores, k, dest, stream);
    if (st != SSW_OK) idx->res_pending_seq = 0;  // nothing was launched that would publish
    return st;
}

// Enqueue half.  q_host = NULL: the top-k of the row scores in `scores`, which are complete (the handle's buffer after
// ensure_full_scores, or a slab of a batch).  With a query, which is scanned into the handle's buffer on the handle's
// stream, those are `scores` and `stream`: the query is staged and scanned first -- after the exclusions are
// installed, a pruned scan selects its threshold with them.
static ssw_status topk_enqueue(ssw_index *idx, const float *q_host, const float *scores, hipStream_t stream,
                               const int64_t *excluded_images, int64_t n_excluded, int32_t k) {
    SSW_REQUIRE(!q_host || (scores == idx->scores && stream == idx->stream), "topk: a query scans into the handle's buffer");
    if (small_path_ok(idx, n_excluded)) return small_enqueue(idx, q_host, scores, stream, excluded_images, n_excluded, k);
    if (q_host) SSW_TRY(stage_query(idx, q_host));
    if (idx->n_images > 0) SSW_TRY(install_excluded(idx, excluded_images, n_excluded, stream));
    if (q_host) SSW_TRY(scan_for_topk(idx, idx->q_dev, k));
    if (idx->n_images == 0) return SSW_OK;
    return select_to_host(idx, scores, stream, k, false);
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
static ssw_status topk_collect(ssw_index *idx, const float *scores, hipStream_t stream, int32_t k, int64_t *out_images,
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

ssw_status ssw_index_topk_fetch(ssw_index *idx, int32_t k, int64_t *out_images, float *out_scores,
                                int64_t *out_best_rows, int32_t *out_count) {
    SSW_REQUIRE(idx != nullptr && out_count != nullptr, "NULL argument");
    DeviceGuard guard(idx->device);
    return fetch_topk(idx, idx->scores, idx->stream, k, out_images, out_scores, out_best_rows, out_count);
}

// ---- the two halves for callers that put more work on the stream in between or ahead (ssw_labelprop_round:
// propagation -> scores -> this selection, ONE wait), on a stream of theirs
extern "C++" {
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

int index_device(const ssw_index *idx) { return idx ? idx->device : -1; }
int32_t index_dtype(const ssw_index *idx) { return idx ? idx->dtype : SSW_DTYPE_F32; }
const void *index_matrix(const ssw_index *idx, int64_t *n_rows, int32_t *dim) {
    if (n_rows) *n_rows = idx->n;
    if (dim) *dim = idx->dim;
    return idx->X;
}
}  // namespace ssw
}  // extern "C++"

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

// ---- several queries in one pass over the rows (scan.hip: batch_scores_kernel) --------------------------------------
// A batch is cut into chunks of the widest kernel form the shape and the side buffer allow, the remainder into
// narrower ones and at last single queries.  A chunk's last query scores into the handle's own buffer, the others into
// the side slabs; the selection then runs slab by slab through the single-query path (topk_enqueue / topk_collect).
constexpr int BATCH_MAX_WIDTH = 16;

static int64_t slab_stride(const ssw_index *idx) { return (idx->n + 64 + 63) & ~(int64_t)63; }  // slabs stay 256-byte aligned

// the chunk's buffers for a width of w: the width they could be grown to
static ssw_status batch_buffers(ssw_index *idx, int w, int *out_w) {
    BatchState &bt = idx->batch;
    if (w >= 2 && !bt.qb_dev) {
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
    int w = scan_batch_max_width(idx->n, idx->dim, idx->dtype);
    if (w > BATCH_MAX_WIDTH) w = BATCH_MAX_WIDTH;
    while (w > nq) w >>= 1;
    return batch_buffers(idx, w, out_w);
}

// queries [w, dim] (host) -> one launch that fills slab[j] = scores of query j; slab[w - 1] is the handle's buffer
static ssw_status do_scan_chunk(ssw_index *idx, const float *q_host, int w, float **slab) {
    BatchState &bt = idx->batch;
    for (int j = 0; j + 1 < w; ++j) slab[j] = bt.side + (int64_t)j * slab_stride(idx);
    slab[w - 1] = idx->scores;
    SSW_TRY(bt.qb_stage.push(bt.qb_dev, q_host, (size_t)w * idx->dim * sizeof(float), idx->stream));
    idx->scores_partial = false;
    return profiled(idx, [&] {
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

ssw_status ssw_index_scan_batch(ssw_index *idx, const float *q_host, int32_t nq, float *out_scores_host) {
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
        float *slab[BATCH_MAX_WIDTH];
        if (w >= 2) {
            SSW_TRY(do_scan_chunk(idx, q_host + b * dim, w, slab));
        } else {
            w = 1;
            slab[0] = idx->scores;
            SSW_TRY(idx->q_stage.push(idx->q_dev, q_host + b * dim, dim * sizeof(float), idx->stream));
            SSW_TRY(do_scan(idx, idx->q_dev));
        }
        if (out_scores_host && idx->n > 0) {
            for (int j = 0; j < w; ++j)
                SSW_HIP_TRY(hipMemcpyAsync(out_scores_host + (size_t)(b + j) * idx->n, slab[j], row_bytes,
                                           hipMemcpyDeviceToHost, idx->stream));
        }
        b += w;
    }
    SSW_HIP_TRY(hipStreamSynchronize(idx->stream));
    return SSW_OK;
}

// the second stage of a batch (ssw_index_topk_batch_avg): the aggregation code and the host outputs [nq, k]
struct AvgStage {
    int32_t aug;
    float *out_scores;
    int64_t *out_rows;
};

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

// ssw_index_topk_batch; with `avg`, every query's selection is followed by the aggregation over its own slab
static ssw_status topk_batch_run(ssw_index *idx, const float *q_host, int32_t nq, const int64_t *excluded_images,
                                 const int64_t *excluded_offsets, int32_t k, int64_t *out_images, float *out_scores,
                                 int64_t *out_best_rows, int32_t *out_counts, const AvgStage *avg) {
    SSW_REQUIRE(nq >= 1, "nq=%d < 1", nq);
    SSW_REQUIRE(idx != nullptr && q_host != nullptr && out_counts != nullptr, "NULL argument");
    SSW_REQUIRE(k >= 1 && k <= SSW_MAX_TOPK, "k=%d outside [1, %d]", k, SSW_MAX_TOPK);
    if (excluded_offsets) {
        SSW_REQUIRE(excluded_offsets[0] >= 0, "excluded_offsets[0]=%lld < 0", (long long)excluded_offsets[0]);
        for (int32_t b = 0; b < nq; ++b)
            SSW_REQUIRE(excluded_offsets[b] <= excluded_offsets[b + 1], "excluded_offsets decrease at query %d", b);
        SSW_REQUIRE(excluded_offsets[nq] == excluded_offsets[0] || excluded_images != nullptr, "excluded_images is NULL");
        SSW_TRY(check_excluded(idx, excluded_images, excluded_offsets[0], excluded_offsets[nq]));
    }
    SSW_TRY(check_query_batch(idx, q_host, nq));
    for (int32_t b = 0; b < nq; ++b) out_counts[b] = 0;
    auto excl = [&](int32_t b, int64_t *n_ex) -> const int64_t * {
        *n_ex = excluded_offsets ? excluded_offsets[b + 1] - excluded_offsets[b] : 0;
        return *n_ex > 0 ? excluded_images + excluded_offsets[b] : nullptr;
    };
    if (nq == 1) {  // the single call itself, pruning included
        int64_t n_ex = 0;
        const int64_t *ex = excl(0, &n_ex);
        SSW_TRY(ssw_index_topk(idx, q_host, ex, n_ex, k, out_images, out_scores, out_best_rows, out_counts));
        if (!avg || idx->n_images == 0) return SSW_OK;
        DeviceGuard guard(idx->device);
        SSW_TRY(ensure_full_scores(idx));  // a pruned top-k left exact scores for its survivors only
        SSW_TRY(ensure_avg_buffers(idx));
        SSW_TRY(enqueue_avg_of_result(idx, idx->scores, k, avg->aug, 0));
        return collect_avg(idx, avg, 0, 1, k);
    }
    DeviceGuard guard(idx->device);
    SSW_TRY(ensure_full_scores(idx));
    if (avg) SSW_TRY(ensure_avg_buffers(idx));
    int W = 1;
    SSW_TRY(batch_width(idx, nq, &W));
    const size_t dim = (size_t)idx->dim;
    for (int32_t b = 0; b < nq;) {
        int w = W;
        while (w > nq - b) w >>= 1;
        float *slab[BATCH_MAX_WIDTH];
        if (w >= 2) {
            SSW_TRY(do_scan_chunk(idx, q_host + b * dim, w, slab));
        } else {  // one query: the full single-query scan (never the pre-scan) into the handle's buffer
            w = 1;
            slab[0] = idx->scores;
            SSW_TRY(stage_query(idx, q_host + b * dim));
            SSW_TRY(do_scan(idx, idx->q_dev));
        }
        for (int j = 0; j < w; ++j) {
            int64_t n_ex = 0;
            const int64_t *ex = excl(b + j, &n_ex);
            const size_t o = (size_t)(b + j) * k;
            SSW_TRY(topk_enqueue(idx, nullptr, slab[j], idx->stream, ex, n_ex, k));
            SSW_TRY(topk_collect(idx, slab[j], idx->stream, k, out_images ? out_images + o : nullptr,
                                 out_scores ? out_scores + o : nullptr, out_best_rows ? out_best_rows + o : nullptr,
                                 out_counts + b + j));
            // after the collect: after a deep rerun too, and before the next query's selection takes the result buffers
            if (avg) SSW_TRY(enqueue_avg_of_result(idx, slab[j], k, avg->aug, j));
        }
        if (avg) SSW_TRY(collect_avg(idx, avg, b, w, k));  // (before the next chunk's scan takes the slabs)
        b += w;
    }
    return SSW_OK;
}

ssw_status ssw_index_topk_batch(ssw_index *idx, const float *q_host, int32_t nq, const int64_t *excluded_images,
                                const int64_t *excluded_offsets, int32_t k, int64_t *out_images, float *out_scores,
                                int64_t *out_best_rows, int32_t *out_counts) {
    return topk_batch_run(idx, q_host, nq, excluded_images, excluded_offsets, k, out_images, out_scores, out_best_rows,
                          out_counts, nullptr);
}

ssw_status ssw_index_topk_batch_avg(ssw_index *idx, const float *q_host, int32_t nq, const int64_t *excluded_images,
                                    const int64_t *excluded_offsets, int32_t k, int32_t aug_larger, int64_t *out_images,
                                    float *out_scores, int64_t *out_best_rows, float *out_avg_scores,
                                    int64_t *out_avg_rows, int32_t *out_counts) {
    SSW_REQUIRE(nq >= 1, "nq=%d < 1", nq);
    SSW_REQUIRE(idx != nullptr && q_host != nullptr && out_counts != nullptr && out_avg_scores != nullptr &&
                    out_avg_rows != nullptr,
                "NULL argument");
    SSW_REQUIRE(aug_larger >= 0 && (aug_larger & 3) <= 2 && aug_larger <= 6,
                "aug_larger=%d is not 0 (all), 1 (greater) or 2 (adjacent), optionally + 4 (aug_weight = cont_weighted)", aug_larger);
    SSW_REQUIRE(idx->has_map && idx->tile_boxes && idx->tile_zoom,
                "topk_batch_avg needs ssw_index_set_row2image and ssw_index_set_tile_meta first");
    const int64_t max_tiles = max_image_tiles(idx);
    SSW_REQUIRE(max_tiles <= SSW_RESCORE_MAX_TILES,
                "the index has an image with %lld tiles, more than the %d the kernel keeps in LDS", (long long)max_tiles,
                SSW_RESCORE_MAX_TILES);
    const AvgStage avg{aug_larger, out_avg_scores, out_avg_rows};
    return topk_batch_run(idx, q_host, nq, excluded_images, excluded_offsets, k, out_images, out_scores, out_best_rows,
                          out_counts, &avg);
}

// ---- the pruned batch: ONE pass over the int8 shadow bounds a chunk of up to 16 queries (prune.hip, "Pruned batch") ----
static_assert(BATCH_MAX_WIDTH == Q8_MQ_WIDTH, "a chunk of the pruned batch uses the batch's slabs");

// the state of a chunk of w queries; the survivor lists may only be had for fewer slots: *out_w
static ssw_status ensure_prune_batch(ssw_index *idx, int w, int *out_w) {
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

// slab j of a chunk of w queries, exactly as do_scan_chunk places them
static float *chunk_slab(ssw_index *idx, int w, int j) {
    return j + 1 < w ? idx->batch.side + (int64_t)j * slab_stride(idx) : idx->scores;
}

// The two device steps of a chunk that the lab hook drives as well; the shadow and the chunk's buffers are ready and
// the w queries are in batch.qb_dev.  Lower bounds of query j into slab j; the handle's buffer (the last query's slab)
// is partial from here on and q_last is the last query.
static ssw_status prune_bounds_mq(ssw_index *idx, int w, int32_t *dbg_hi, int32_t *dbg_lo) {
    PruneState &p = idx->prune;
    PruneBatchState &pb = idx->prune_batch;
    SSW_TRY(launch_q8_query_mq(idx->batch.qb_dev, idx->dim, w, pb.mq, pb.planes, p.q_last, idx->stream));
    SSW_TRY(launch_q8_bounds_mq(p.q8, p.q8_scale, p.q8_err, pb.planes, pb.mq, w, idx->batch.side, slab_stride(idx),
                                idx->scores, idx->n, idx->dim, dbg_hi, dbg_lo, idx->device, idx->stream));
    idx->scores_partial = true;
    return SSW_OK;
}

// the survivors of slot j against the keys the last selection left, into the slot's list (no publish)
static ssw_status prune_survivors_slot(ssw_index *idx, int w, int j, int32_t k, int64_t cap) {
    PruneState &p = idx->prune;
    PruneBatchState &pb = idx->prune_batch;
    return launch_survivors_mq(chunk_slab(idx, w, j), p.q8_err, p.q8_scale, idx->n, idx->dim, idx->ws.out_keys,
                               idx->ws.out_count, k, pb.mq + j * Q8_MQ_WORDS, pb.surv_rows + (int64_t)j * SURV_CAP, cap,
                               idx->device, idx->stream);
}

// every slot's count (or -1) of the chunk -> out_m[w]; ONE host wait: a sleep on sleep_ev_or_null first, then a spin
static ssw_status prune_publish_mq(ssw_index *idx, int w, int64_t cap, hipEvent_t sleep_ev_or_null, int32_t *out_m) {
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

ssw_status ssw_index_topk_batch_pruned(ssw_index *idx, const float *q_host, int32_t nq, const int64_t *excluded_images,
                                       const int64_t *excluded_offsets, int32_t k, int64_t *out_images,
                                       float *out_scores, int64_t *out_best_rows, int32_t *out_counts) {
    SSW_REQUIRE(nq >= 1, "nq=%d < 1", nq);
    SSW_REQUIRE(idx != nullptr && q_host != nullptr && out_counts != nullptr, "NULL argument");
    SSW_REQUIRE(k >= 1 && k <= SSW_MAX_TOPK, "k=%d outside [1, %d]", k, SSW_MAX_TOPK);
    bool ready = false;
    int W = 1;
    {
        DeviceGuard guard(idx->device);
        if (prune_batch_eligible(idx) && idx->ws.xchg.msg_out == nullptr) SSW_TRY(ensure_shadow(idx, &ready));
        if (ready && !idx->batch.qb_dev &&
            hipMalloc((void **)&idx->batch.qb_dev, (size_t)BATCH_MAX_WIDTH * idx->dim * sizeof(float)) != hipSuccess) {
            (void)hipGetLastError();
            idx->batch.qb_dev = nullptr;
            ready = false;
        }
    }
    if (!ready)  // not eligible, or the shadow is refused: the plain batch, which leaves the counters alone
        return ssw_index_topk_batch(idx, q_host, nq, excluded_images, excluded_offsets, k, out_images, out_scores,
                                    out_best_rows, out_counts);
    if (excluded_offsets) {
        SSW_REQUIRE(excluded_offsets[0] >= 0, "excluded_offsets[0]=%lld < 0", (long long)excluded_offsets[0]);
        for (int32_t b = 0; b < nq; ++b)
            SSW_REQUIRE(excluded_offsets[b] <= excluded_offsets[b + 1], "excluded_offsets decrease at query %d", b);
        SSW_REQUIRE(excluded_offsets[nq] == excluded_offsets[0] || excluded_images != nullptr, "excluded_images is NULL");
        SSW_TRY(check_excluded(idx, excluded_images, excluded_offsets[0], excluded_offsets[nq]));
    }
    SSW_TRY(check_query_batch(idx, q_host, nq));
    for (int32_t b = 0; b < nq; ++b) out_counts[b] = 0;
    auto excl = [&](int32_t b, int64_t *n_ex) -> const int64_t * {
        *n_ex = excluded_offsets ? excluded_offsets[b + 1] - excluded_offsets[b] : 0;
        return *n_ex > 0 ? excluded_images + excluded_offsets[b] : nullptr;
    };
    DeviceGuard guard(idx->device);
    // (a partial buffer is not completed first: every chunk overwrites it and the kept query together)
    SSW_TRY(ensure_ws(idx));
    SSW_TRY(batch_buffers(idx, std::min<int32_t>(nq, Q8_MQ_WIDTH), &W));
    SSW_TRY(ensure_prune_batch(idx, W, &W));
    PruneState &p = idx->prune;
    PruneBatchState &pb = idx->prune_batch;
    BatchState &bt = idx->batch;
    const size_t dim = (size_t)idx->dim;
    for (int32_t b = 0; b < nq;) {
        const int w = std::min<int32_t>(W, nq - b);
        int32_t m[Q8_MQ_WIDTH];
        SSW_TRY(bt.qb_stage.push(bt.qb_dev, q_host + b * dim, (size_t)w * dim * sizeof(float), idx->stream));
        SSW_TRY(profiled(idx, [&]() -> ssw_status {
            SSW_TRY(prune_bounds_mq(idx, w, nullptr, nullptr));
            SSW_HIP_TRY(hipEventRecord(p.ev, idx->stream));
            for (int j = 0; j < w; ++j) {  // threshold and survivors of each query, in stream order
                int64_t n_ex = 0;
                const int64_t *ex = excl(b + j, &n_ex);
                SSW_TRY(install_excluded(idx, ex, n_ex, idx->stream));
                SSW_TRY(do_select(idx, chunk_slab(idx, w, j), k, SelectDest{nullptr, 0u, false}, idx->stream));
                SSW_TRY(prune_survivors_slot(idx, w, j, k, SURV_CAP));
            }
            SSW_TRY(prune_publish_mq(idx, w, SURV_CAP, p.ev, m));  // sleep through the shadow scan, spin on the rest
            for (int j = 0; j < w; ++j) {
                const float *qj = bt.qb_dev + (size_t)j * dim;
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
        }));
        for (int j = 0; j < w; ++j) {
            int64_t n_ex = 0;
            const int64_t *ex = excl(b + j, &n_ex);
            const size_t o = (size_t)(b + j) * k;
            float *slab = chunk_slab(idx, w, j);
            SSW_TRY(topk_enqueue(idx, nullptr, slab, idx->stream, ex, n_ex, k));
            SSW_TRY(topk_collect(idx, slab, idx->stream, k, out_images ? out_images + o : nullptr,
                                 out_scores ? out_scores + o : nullptr, out_best_rows ? out_best_rows + o : nullptr,
                                 out_counts + b + j));
        }
        b += w;
    }
    return SSW_OK;
}

static ssw_status stage_rows(ssw_index *idx, const int64_t *rows_host, int64_t n) {
    for (int64_t i = 0; i < n; ++i) {
        SSW_REQUIRE(rows_host[i] >= 0 && rows_host[i] < idx->n, "row %lld outside [0, %lld)",
                    (long long)rows_host[i], (long long)idx->n);
    }
    if (n > idx->gather_cap) {
        SSW_HIP_TRY(hipStreamSynchronize(idx->stream));
        (void)hipFree(idx->gather_idx);
        (void)hipFree(idx->gather_out);
        idx->gather_idx = nullptr;
        idx->gather_out = nullptr;
        idx->gather_cap = 0;
        int64_t cap = 4096;
        while (cap < n) cap <<= 1;
        SSW_HIP_TRY(hipMalloc((void **)&idx->gather_idx, (size_t)cap * sizeof(int64_t)));
        SSW_HIP_TRY(hipMalloc((void **)&idx->gather_out, (size_t)cap * sizeof(float)));
        idx->gather_cap = cap;
    }
    return idx->rows_stage.push(idx->gather_idx, rows_host, (size_t)n * sizeof(int64_t), idx->stream);
}

ssw_status ssw_index_score_rows(ssw_index *idx, const float *q_host, const int64_t *rows_host,
                                int64_t n, float *out_scores_host) {
    SSW_REQUIRE(idx != nullptr, "idx is NULL");
    if (n <= 0) return SSW_OK;
    SSW_REQUIRE(q_host && rows_host && out_scores_host, "NULL argument");
    SSW_TRY(check_query(idx, q_host));
    DeviceGuard guard(idx->device);
    SSW_TRY(stage_rows(idx, rows_host, n));
    if (!idx->q2_dev) SSW_HIP_TRY(hipMalloc((void **)&idx->q2_dev, (size_t)idx->dim * sizeof(float)));
    SSW_TRY(idx->q2_stage.push(idx->q2_dev, q_host, (size_t)idx->dim * sizeof(float), idx->stream));
    SSW_TRY(launch_score_rows(idx->X, idx->dtype, idx->q2_dev, idx->gather_idx, n, idx->dim, idx->gather_out,
                              idx->stream));
    SSW_HIP_TRY(hipMemcpyAsync(out_scores_host, idx->gather_out, (size_t)n * sizeof(float),
                               hipMemcpyDeviceToHost, idx->stream));
    SSW_HIP_TRY(hipStreamSynchronize(idx->stream));
    return SSW_OK;
}

ssw_status ssw_index_gather_scores(ssw_index *idx, const int64_t *rows_host, int64_t n,
                                   float *out_scores_host) {
    SSW_REQUIRE(idx != nullptr, "idx is NULL");
    if (n <= 0) return SSW_OK;
    SSW_REQUIRE(rows_host != nullptr && out_scores_host != nullptr, "NULL argument");
    DeviceGuard guard(idx->device);
    SSW_TRY(ensure_full_scores(idx));
    SSW_TRY(stage_rows(idx, rows_host, n));
    SSW_TRY(launch_gather_f32(idx->scores, idx->gather_idx, n, idx->gather_out, idx->stream));
    SSW_HIP_TRY(hipMemcpyAsync(out_scores_host, idx->gather_out, (size_t)n * sizeof(float),
                               hipMemcpyDeviceToHost, idx->stream));
    SSW_HIP_TRY(hipStreamSynchronize(idx->stream));
    return SSW_OK;
}

// the vectors of arbitrary rows (`index.vectors[rows]`: what the fitting loops read of the labelled tiles,
// multi_reg.py:204, loops/util.py:6,11) out of the resident matrix -- for callers that do not hold a host copy of it
// (a rank of the row-sharded index serves its own rows this way)
ssw_status ssw_index_gather_rows(ssw_index *idx, const int64_t *rows_host, int64_t n, float *out_host) {
    SSW_REQUIRE(idx != nullptr, "idx is NULL");
    if (n <= 0) return SSW_OK;
    SSW_REQUIRE(rows_host != nullptr && out_host != nullptr, "NULL argument");
    for (int64_t i = 0; i < n; ++i)
        SSW_REQUIRE(rows_host[i] >= 0 && rows_host[i] < idx->n, "row %lld outside [0, %lld)", (long long)rows_host[i],
                    (long long)idx->n);
    DeviceGuard guard(idx->device);
    SSW_TRY(stage_rows(idx, rows_host, n));
    float *buf = nullptr;
    SSW_HIP_TRY(hipMalloc((void **)&buf, (size_t)n * idx->dim * sizeof(float)));
    // f16 rows come back widened, in natural element order
    const ssw_status st = launch_gather_rows(idx->X, idx->dtype, idx->gather_idx, 0, n, idx->dim, buf, idx->stream);
    if (st != SSW_OK) {
        (void)hipFree(buf);
        return st;
    }
    hipError_t e =
        hipMemcpyAsync(out_host, buf, (size_t)n * idx->dim * sizeof(float), hipMemcpyDeviceToHost, idx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(idx->stream);
    (void)hipFree(buf);
    if (e != hipSuccess) {
        set_error("ssw_index_gather_rows: %s", hipGetErrorString(e));
        return SSW_ERR_HIP;
    }
    return SSW_OK;
}

ssw_status ssw_topk_merge_dev(int32_t device, void *hip_stream, const uint64_t *dev_keys_in,
                              int32_t n_lists, int32_t list_stride, const int32_t *dev_counts,
                              int32_t k, uint64_t *dev_keys_out, int32_t *dev_count_out) {
    SSW_REQUIRE(dev_keys_in && dev_counts && dev_keys_out && dev_count_out, "NULL argument");
    DeviceGuard guard(device);
    return launch_merge_topk(dev_keys_in, n_lists, list_stride, dev_counts, k, dev_keys_out,
                             dev_count_out, (hipStream_t)hip_stream);
}

// the sharded exchange without elementwise kernels around the collective: the selection's last kernel also writes
// this rank's message (globalised keys, optional best rows, count | overflow << 32) into dev_msg
ssw_status ssw_index_set_exchange_target(ssw_index *idx, uint64_t *dev_msg_or_null, int32_t k_max, int32_t with_best,
                                         int64_t image_offset, int64_t row_offset) {
    SSW_REQUIRE(idx != nullptr, "idx is NULL");
    FinalExchange x;
    if (dev_msg_or_null) {
        SSW_REQUIRE(k_max >= 1 && k_max <= SSW_MAX_TOPK && image_offset >= 0, "bad message geometry");
        x.msg_out = dev_msg_or_null;
        x.image_offset = (uint64_t)image_offset;
        x.row_offset = row_offset;
        x.k_max = k_max;
        x.with_best = with_best ? 1 : 0;
        x.msg_len = (with_best ? 2 : 1) * k_max + 1;
    }
    idx->ws.xchg = x;
    return SSW_OK;
}

ssw_status ssw_topk_merge_msgs_dev(int32_t device, void *hip_stream, const uint64_t *dev_msgs, int32_t world,
                                   int32_t k_max, int32_t with_best, int32_t k, uint64_t *dev_keys_out,
                                   int32_t *dev_count_out, int64_t *dev_flags_or_null, int64_t *dev_flags_seen_or_null) {
    SSW_REQUIRE(dev_msgs && dev_keys_out && dev_count_out, "NULL argument");
    DeviceGuard guard(device);
    return launch_merge_msgs(dev_msgs, world, k_max, with_best, k, dev_keys_out, dev_count_out,
                             reinterpret_cast<long long *>(dev_flags_or_null),
                             reinterpret_cast<long long *>(dev_flags_seen_or_null), (hipStream_t)hip_stream);
}

#ifdef SSW_DEBUG_HOOKS
ssw_status ssw_tune_topk(int32_t flags) {
    g_small_path = (flags & 1) != 0;
    tune_select((flags & 2) != 0);
    return SSW_OK;
}

ssw_status ssw_tune_scan(int32_t variant, int32_t blocks_per_cu) {
    tune_scan(variant, blocks_per_cu);
    return SSW_OK;
}

ssw_status ssw_tune_scan_batch(int32_t max_width, int32_t blocks_per_cu) {
    tune_scan_batch(max_width, blocks_per_cu);
    return SSW_OK;
}

ssw_status ssw_tune_prune(int32_t enable, int64_t min_rows, int64_t reserve_bytes) {
    g_prune = enable != 0;
    g_prune_min_rows = min_rows < 0 ? -1 : min_rows;  // < 0: PRUNE_MIN_ROWS / PRUNE_MIN_ROWS_F16 again
    g_prune_reserve = reserve_bytes < 0 ? PRUNE_RESERVE : reserve_bytes;
    return SSW_OK;
}

ssw_status ssw_tune_prune_scan(int32_t blocks_per_cu, int32_t group_loads) {
    tune_q8_bounds(blocks_per_cu, group_loads);
    return SSW_OK;
}

// ---- the pre-scan's intermediate state (tests/test_prune_certificate_gpu.py) ----------------------------------------
// Each hook drives the product's kernels through the steps scan_for_topk is made of, on the index's own buffers.
ssw_status ssw_debug_prune_shadow(ssw_index *idx, int64_t first_row, int64_t n_rows, int8_t *out_codes, float *out_scale,
                                  float *out_err) {
    SSW_REQUIRE(idx != nullptr, "idx is NULL");
    SSW_REQUIRE(first_row >= 0 && n_rows >= 0 && first_row + n_rows <= idx->n, "rows [%lld, +%lld) outside [0, %lld)",
                (long long)first_row, (long long)n_rows, (long long)idx->n);
    SSW_REQUIRE(prune_eligible(idx), "the index is not pruned (ssw_tune_prune, dim, borrowed or escaped rows)");
    DeviceGuard guard(idx->device);
    bool ready = false;
    SSW_TRY(ensure_shadow(idx, &ready));
    if (!ready) {
        set_error("prune_shadow: the shadow was refused for memory");
        return SSW_ERR_NOMEM;
    }
    if (n_rows > 0 && out_codes)
        SSW_HIP_TRY(hipMemcpyAsync(out_codes, idx->prune.q8 + first_row * idx->dim, (size_t)n_rows * idx->dim,
                                   hipMemcpyDeviceToHost, idx->stream));
    if (n_rows > 0 && out_scale)
        SSW_HIP_TRY(hipMemcpyAsync(out_scale, idx->prune.q8_scale + first_row, (size_t)n_rows * sizeof(float),
                                   hipMemcpyDeviceToHost, idx->stream));
    if (n_rows > 0 && out_err)
        SSW_HIP_TRY(hipMemcpyAsync(out_err, idx->prune.q8_err + first_row, (size_t)n_rows * sizeof(float),
                                   hipMemcpyDeviceToHost, idx->stream));
    SSW_HIP_TRY(hipStreamSynchronize(idx->stream));
    return SSW_OK;
}

ssw_status ssw_debug_prune_bounds(ssw_index *idx, const float *q_host, float *out_lb, float *out_Q,
                                  int32_t *out_unbounded) {
    SSW_REQUIRE(idx != nullptr && q_host != nullptr && out_lb != nullptr && out_Q != nullptr && out_unbounded != nullptr,
                "NULL argument");
    SSW_TRY(check_query(idx, q_host));
    SSW_REQUIRE(prune_eligible(idx), "the index is not pruned (ssw_tune_prune, dim, borrowed or escaped rows)");
    DeviceGuard guard(idx->device);
    bool ready = false;
    SSW_TRY(ensure_shadow(idx, &ready));
    if (!ready) {
        set_error("prune_bounds: the shadow was refused for memory");
        return SSW_ERR_NOMEM;
    }
    SSW_TRY(idx->q_stage.push(idx->q_dev, q_host, (size_t)idx->dim * sizeof(float), idx->stream));
    SSW_TRY(prune_bounds(idx, idx->q_dev));  // as in scan_for_topk: every reader completes the buffer with the scan of q_last
    unsigned state[4] = {0u, 0u, 0u, 0u};
    SSW_HIP_TRY(hipMemcpyAsync(state, idx->prune.state, sizeof(state), hipMemcpyDeviceToHost, idx->stream));
    SSW_HIP_TRY(hipMemcpyAsync(out_lb, idx->scores, (size_t)idx->n * sizeof(float), hipMemcpyDeviceToHost, idx->stream));
    SSW_HIP_TRY(hipStreamSynchronize(idx->stream));
    memcpy(out_Q, &state[1], sizeof(float));
    *out_unbounded = (int32_t)state[2];
    return SSW_OK;
}

ssw_status ssw_debug_prune_survivors(ssw_index *idx, float threshold, int32_t k, int32_t sel_count, int32_t sel_overflow,
                                     int64_t cap, int32_t *out_published, int64_t *out_collected, int64_t *out_rows) {
    SSW_REQUIRE(idx != nullptr && out_published != nullptr && out_collected != nullptr, "NULL argument");
    SSW_REQUIRE(k >= 1 && k <= SSW_MAX_TOPK, "k=%d outside [1, %d]", k, SSW_MAX_TOPK);
    SSW_REQUIRE(cap >= 0 && cap <= SURV_CAP, "cap=%lld outside [0, %lld]", (long long)cap, (long long)SURV_CAP);
    SSW_REQUIRE(cap == 0 || out_rows != nullptr, "out_rows is NULL");
    SSW_REQUIRE(idx->scores_partial && idx->prune.q8 && !idx->prune.stale, "no bounds in the buffer: ssw_debug_prune_bounds first");
    DeviceGuard guard(idx->device);
    SSW_TRY(ensure_ws(idx));
    // what the threshold selection leaves behind: k keys (only the k-th is read) and [count, overflow]
    std::vector<uint64_t> keys((size_t)k, (uint64_t)f32_to_ord(threshold) << 32);
    const int32_t count[2] = {sel_count, sel_overflow};
    SSW_HIP_TRY(hipMemcpyAsync(idx->ws.out_keys, keys.data(), keys.size() * sizeof(uint64_t), hipMemcpyHostToDevice,
                               idx->stream));
    SSW_HIP_TRY(hipMemcpyAsync(idx->ws.out_count, count, sizeof(count), hipMemcpyHostToDevice, idx->stream));
    SSW_HIP_TRY(hipMemsetAsync(idx->prune.state, 0, sizeof(unsigned), idx->stream));  // the counter k_q8_query resets
    SSW_HIP_TRY(hipStreamSynchronize(idx->stream));  // keys and count are pageable host memory
    int32_t m = -1;
    SSW_TRY(prune_survivors(idx, k, cap, nullptr, &m));
    unsigned collected = 0u;
    SSW_HIP_TRY(hipMemcpyAsync(&collected, idx->prune.state, sizeof(unsigned), hipMemcpyDeviceToHost, idx->stream));
    if (m > 0)
        SSW_HIP_TRY(hipMemcpyAsync(out_rows, idx->prune.surv_rows, (size_t)m * sizeof(int64_t), hipMemcpyDeviceToHost,
                                   idx->stream));
    SSW_HIP_TRY(hipStreamSynchronize(idx->stream));
    *out_published = m;
    *out_collected = (int64_t)collected;
    return SSW_OK;
}
ssw_status ssw_tune_prune_scan_mq(int32_t blocks_per_cu, int32_t tiles) {
    tune_q8_bounds_mq(blocks_per_cu, tiles);
    return SSW_OK;
}

ssw_status ssw_debug_prune_scan_mq_shape(ssw_index *idx, int32_t *out_blocks, int32_t *out_tiles) {
    SSW_REQUIRE(idx != nullptr && out_blocks != nullptr && out_tiles != nullptr, "NULL argument");
    SSW_REQUIRE(q8_dim_supported(idx->dim), "dim=%d has no shadow scan", idx->dim);
    int blocks = 0, tiles = 0;
    q8_bounds_mq_shape(idx->dim, idx->device, idx->n, &blocks, &tiles);
    *out_blocks = blocks;
    *out_tiles = tiles;
    return SSW_OK;
}

// the chunk's buffers for nq queries staged from the host, for the two hooks below
static ssw_status debug_chunk_ready(ssw_index *idx, int32_t nq) {
    SSW_REQUIRE(prune_batch_eligible(idx), "the index is not pruned (ssw_tune_prune, dim, borrowed or escaped rows)");
    bool ready = false;
    SSW_TRY(ensure_shadow(idx, &ready));
    if (!ready) {
        set_error("prune_bounds_mq: the shadow was refused for memory");
        return SSW_ERR_NOMEM;
    }
    SSW_TRY(ensure_ws(idx));
    if (!idx->batch.qb_dev)
        SSW_HIP_TRY(hipMalloc((void **)&idx->batch.qb_dev, (size_t)BATCH_MAX_WIDTH * idx->dim * sizeof(float)));
    int w = 0;
    SSW_TRY(batch_buffers(idx, nq, &w));
    if (w == nq) SSW_TRY(ensure_prune_batch(idx, nq, &w));
    if (w != nq) {
        set_error("prune_bounds_mq: no memory for a chunk of %d queries", nq);
        return SSW_ERR_NOMEM;
    }
    return SSW_OK;
}

ssw_status ssw_debug_prune_bounds_mq(ssw_index *idx, const float *q_host, int32_t nq, int32_t *out_I_hi, int32_t *out_I_lo,
                                     float *out_lb, float *out_Qe, int8_t *out_codes) {
    SSW_REQUIRE(idx != nullptr && q_host != nullptr, "NULL argument");
    SSW_REQUIRE(nq >= 1 && nq <= Q8_MQ_WIDTH, "nq=%d outside [1, %d]", nq, Q8_MQ_WIDTH);
    DeviceGuard guard(idx->device);
    SSW_TRY(debug_chunk_ready(idx, nq));
    PruneBatchState &pb = idx->prune_batch;
    const size_t dim = (size_t)idx->dim, cells = (size_t)nq * idx->n;
    int32_t *dbg = nullptr;
    if (out_I_hi || out_I_lo) SSW_HIP_TRY(hipMalloc((void **)&dbg, 2 * cells * sizeof(int32_t)));
    std::vector<unsigned> mq((size_t)Q8_MQ_WIDTH * Q8_MQ_WORDS);
    std::vector<int8_t> planes(q8_mq_plane_bytes(idx->dim));
    auto run = [&]() -> ssw_status {
        SSW_TRY(idx->batch.qb_stage.push(idx->batch.qb_dev, q_host, (size_t)nq * dim * sizeof(float), idx->stream));
        SSW_TRY(prune_bounds_mq(idx, nq, dbg, dbg ? dbg + cells : nullptr));
        if (out_I_hi) SSW_HIP_TRY(hipMemcpyAsync(out_I_hi, dbg, cells * sizeof(int32_t), hipMemcpyDeviceToHost, idx->stream));
        if (out_I_lo)
            SSW_HIP_TRY(hipMemcpyAsync(out_I_lo, dbg + cells, cells * sizeof(int32_t), hipMemcpyDeviceToHost, idx->stream));
        if (out_lb)
            for (int j = 0; j < nq; ++j)
                SSW_HIP_TRY(hipMemcpyAsync(out_lb + (size_t)j * idx->n, chunk_slab(idx, nq, j), (size_t)idx->n * sizeof(float),
                                           hipMemcpyDeviceToHost, idx->stream));
        SSW_HIP_TRY(hipMemcpyAsync(mq.data(), pb.mq, mq.size() * sizeof(unsigned), hipMemcpyDeviceToHost, idx->stream));
        SSW_HIP_TRY(hipMemcpyAsync(planes.data(), pb.planes, planes.size(), hipMemcpyDeviceToHost, idx->stream));
        SSW_HIP_TRY(hipStreamSynchronize(idx->stream));
        return SSW_OK;
    };
    const ssw_status st = run();
    if (st != SSW_OK) (void)hipStreamSynchronize(idx->stream);
    (void)hipFree(dbg);
    SSW_TRY(st);
    for (int j = 0; j < nq; ++j) {
        const unsigned *w = mq.data() + (size_t)j * Q8_MQ_WORDS;
        if (out_Qe) {
            memcpy(out_Qe + 4 * j, &w[1], 4);      // Q
            memcpy(out_Qe + 4 * j + 1, &w[3], 4);  // e
            memcpy(out_Qe + 4 * j + 2, &w[4], 4);  // t2
            out_Qe[4 * j + 3] = (float)w[2];       // 1 = the query cannot be bounded
        }
        if (out_codes)  // the planes' fragment order (prune.hip) back to natural element order
            for (int pl = 0; pl < 2; ++pl)
                for (size_t i = 0; i < dim; ++i)
                    out_codes[((size_t)j * 2 + pl) * dim + i] =
                        planes[(((i >> 6) * 2 + pl) * 64 + ((i & 63) >> 4) * 16 + j) * 16 + (i & 15)];
    }
    return SSW_OK;
}

ssw_status ssw_debug_prune_survivors_mq(ssw_index *idx, int32_t nq, int32_t slot, float threshold, int32_t k,
                                        int32_t sel_count, int32_t sel_overflow, int64_t cap, int32_t *out_published,
                                        int64_t *out_collected, int64_t *out_rows) {
    SSW_REQUIRE(idx != nullptr && out_published != nullptr && out_collected != nullptr, "NULL argument");
    SSW_REQUIRE(nq >= 1 && nq <= Q8_MQ_WIDTH && slot >= 0 && slot < nq, "slot=%d outside the chunk of %d", slot, nq);
    SSW_REQUIRE(k >= 1 && k <= SSW_MAX_TOPK, "k=%d outside [1, %d]", k, SSW_MAX_TOPK);
    SSW_REQUIRE(cap >= 0 && cap <= SURV_CAP, "cap=%lld outside [0, %lld]", (long long)cap, (long long)SURV_CAP);
    SSW_REQUIRE(cap == 0 || out_rows != nullptr, "out_rows is NULL");
    PruneBatchState &pb = idx->prune_batch;
    SSW_REQUIRE(idx->scores_partial && idx->prune.q8 && !idx->prune.stale && pb.slots >= nq && idx->batch.side_slabs >= nq - 1,
                "no bounds of such a chunk in the buffers: ssw_debug_prune_bounds_mq first");
    DeviceGuard guard(idx->device);
    SSW_TRY(ensure_ws(idx));
    std::vector<uint64_t> keys((size_t)k, (uint64_t)f32_to_ord(threshold) << 32);
    const int32_t count[2] = {sel_count, sel_overflow};
    unsigned *st = pb.mq + slot * Q8_MQ_WORDS;
    SSW_HIP_TRY(hipMemcpyAsync(idx->ws.out_keys, keys.data(), keys.size() * sizeof(uint64_t), hipMemcpyHostToDevice,
                               idx->stream));
    SSW_HIP_TRY(hipMemcpyAsync(idx->ws.out_count, count, sizeof(count), hipMemcpyHostToDevice, idx->stream));
    SSW_HIP_TRY(hipMemsetAsync(st, 0, sizeof(unsigned), idx->stream));      // the counter and the "selection failed"
    SSW_HIP_TRY(hipMemsetAsync(st + 5, 0, sizeof(unsigned), idx->stream));  // word k_q8_query_mq resets
    SSW_HIP_TRY(hipStreamSynchronize(idx->stream));  // keys and count are pageable host memory
    SSW_TRY(prune_survivors_slot(idx, nq, slot, k, cap));
    int32_t m[Q8_MQ_WIDTH];
    SSW_TRY(prune_publish_mq(idx, nq, cap, nullptr, m));
    unsigned collected = 0u;
    SSW_HIP_TRY(hipMemcpyAsync(&collected, st, sizeof(unsigned), hipMemcpyDeviceToHost, idx->stream));
    if (m[slot] > 0)
        SSW_HIP_TRY(hipMemcpyAsync(out_rows, pb.surv_rows + (int64_t)slot * SURV_CAP, (size_t)m[slot] * sizeof(int64_t),
                                   hipMemcpyDeviceToHost, idx->stream));
    SSW_HIP_TRY(hipStreamSynchronize(idx->stream));
    *out_published = m[slot];
    *out_collected = (int64_t)collected;
    return SSW_OK;
}
#endif

ssw_status ssw_index_profile(ssw_index *idx, int32_t enable) {
    SSW_REQUIRE(idx != nullptr, "idx is NULL");
    DeviceGuard guard(idx->device);
    SSW_HIP_TRY(hipStreamSynchronize(idx->stream));
    if (enable && idx->ev.empty()) {
        idx->ev.resize(2 * 4096);
        for (auto &e : idx->ev) SSW_HIP_TRY(hipEventCreate(&e));
    }
    idx->profiling = enable != 0;
    idx->ev_used = 0;
    return SSW_OK;
}

ssw_status ssw_index_profile_read(ssw_index *idx, float *out_ms, int32_t cap, int32_t *out_n) {
    SSW_REQUIRE(idx != nullptr && out_n != nullptr, "NULL argument");
    DeviceGuard guard(idx->device);
    SSW_HIP_TRY(hipStreamSynchronize(idx->stream));
    const int pairs = idx->ev_used / 2;
    int n = 0;
    for (int i = 0; i < pairs && n < cap; ++i) {
        float ms = 0.f;
        SSW_HIP_TRY(hipEventElapsedTime(&ms, idx->ev[2 * i], idx->ev[2 * i + 1]));
        out_ms[n++] = ms;
    }
    *out_n = n;
    idx->ev_used = 0;
    return SSW_OK;
}

}  // extern "C"

// capi_index.hip -- C-ABI of the resident vector index (see include/seesaw_hip.h): the handle, its rows, the scan, row
// gathers, rescoring.  Its top-k: index_topk.hip, index_prune.hip, index_batch.hip; the handle itself: index_handle.h.
#include <algorithm>
#include <cmath>
#include <vector>

#include "index_handle.h"

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

static ssw_status check_row_range(const ssw_index *idx, int64_t first_row, int64_t n) {
    SSW_REQUIRE(first_row >= 0 && n >= 0 && first_row + n <= idx->n,
                "rows [%lld, %lld) outside the index of %lld rows", (long long)first_row,
                (long long)(first_row + n), (long long)idx->n);
    return SSW_OK;
}

ssw_status ssw::check_excluded(const ssw_index *idx, const int64_t *ids, int64_t first, int64_t last) {
    for (int64_t i = first; i < last; ++i)
        SSW_REQUIRE(ids[i] >= 0 && ids[i] < idx->n_images, "excluded image %lld outside [0, %lld)", (long long)ids[i],
                    (long long)idx->n_images);
    return SSW_OK;
}

ssw_status ssw::check_query(const ssw_index *idx, const float *q_host) {
    for (int i = 0; i < idx->dim; ++i) {
        if (!std::isfinite(q_host[i])) {
            // the reference asserts on NaN query vectors (seesaw/loops/loop_base.py:47)
            set_error("query vector has a non-finite component at %d", i);
            return SSW_ERR_NUMERIC;
        }
    }
    return SSW_OK;
}

ssw_status ssw::launch_index_scan(ssw_index *idx, const float *q_dev, hipStream_t stream) {
    if (idx->parent)  // a view: its member rows in place, out of the parent's matrix
        return launch_scan_view(idx->X, idx->dtype, q_dev, idx->row_src, idx->scores, idx->n, idx->dim, idx->device, stream);
    return launch_scan(idx->X, idx->dtype, q_dev, idx->scores, idx->n, idx->dim, idx->device, stream);
}

ssw_status ssw::refuse_view(const ssw_index *idx, const char *who) {
    if (!idx || !idx->parent) return SSW_OK;
    set_error("%s: the index is a view of another index's rows and has no matrix of its own; call it on the parent or on a "
              "copied subset", who);
    return SSW_ERR_UNSUPPORTED;
}

const int32_t *ssw::index_view_rows(const ssw_index *idx) { return idx && idx->parent ? idx->row_src_host.data() : nullptr; }

ssw_status ssw::do_scan(ssw_index *idx, const float *q_dev) {
    idx->scores_partial = false;
    return profiled(idx, [&] { return launch_index_scan(idx, q_dev, idx->stream); });
}

ssw_status ssw::ensure_full_scores(ssw_index *idx, hipStream_t stream) {
    if (!idx->scores_partial) return SSW_OK;
    idx->scores_partial = false;
    ++idx->prune.completions;
    return launch_index_scan(idx, idx->prune.q_last, stream);
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

// the arguments of an avg_score aggregation over the index's tiles; `who` names the entry in the message
ssw_status ssw::check_aug_code(int32_t aug_larger) {
    SSW_REQUIRE(aug_larger >= 0 && (aug_larger & 3) <= 2 && aug_larger <= 6,
                "aug_larger=%d is not 0 (all), 1 (greater) or 2 (adjacent), optionally + 4 (aug_weight = cont_weighted)", aug_larger);
    return SSW_OK;
}

ssw_status ssw::check_avg_args(const ssw_index *idx, int32_t aug_larger, const char *who) {
    SSW_TRY(check_aug_code(aug_larger));
    SSW_REQUIRE(idx->has_map && idx->tile_boxes && idx->tile_zoom,
                "%s needs ssw_index_set_row2image and ssw_index_set_tile_meta first", who);
    return SSW_OK;
}

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
    *out = idx;
    return SSW_OK;
}

ssw_status ssw_index_destroy(ssw_index *idx) {
    if (!idx) return SSW_OK;
    SSW_REQUIRE(idx->live_views == 0, "ssw_index_destroy: %lld views still read this index's rows; destroy them first",
                (long long)idx->live_views);
    DeviceGuard guard(idx->device);
    if (idx->own_stream) (void)hipStreamSynchronize(idx->own_stream);
    if (idx->parent) {
        if (idx->stream != idx->own_stream) (void)hipStreamSynchronize(idx->stream);  // its scans read the parent's rows
        --idx->parent->live_views;
    }
    (void)hipFree(idx->row_src);
    for (hipEvent_t e : idx->ev) (void)hipEventDestroy(e);
    if (idx->ws_ready) select_free(idx->ws);
    idx->prune.release();
    idx->batch.release();
    idx->prune_batch.release();
    idx->pair.release();
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
    if (idx->slot_host) (void)hipHostFree(idx->slot_host);
    idx->q2_stage.release();
    if (idx->own_stream) (void)hipStreamDestroy(idx->own_stream);
    delete idx;
    return SSW_OK;
}

ssw_status ssw_index_create_view(ssw_index *parent, const int64_t *image_positions, int64_t m, ssw_index **out) {
    SSW_REQUIRE(out != nullptr, "out is NULL");
    *out = nullptr;
    SSW_REQUIRE(parent != nullptr && image_positions != nullptr, "NULL argument");
    if (parent->parent) {
        set_error("ssw_index_create_view: the index is itself a view; take the view from its parent");
        return SSW_ERR_UNSUPPORTED;
    }
    SSW_REQUIRE(m >= 1, "ssw_index_create_view: m=%lld < 1", (long long)m);
    // the members' rows, in the parent's row order, and the view's own image map: all on the host, before any device call
    std::vector<int32_t> src;
    std::vector<int64_t> start;
    if (parent->has_map) start.push_back(0);
    for (int64_t i = 0; i < m; ++i) {
        const int64_t p = image_positions[i];
        SSW_REQUIRE(p >= 0 && p < parent->n_images, "ssw_index_create_view: position %lld outside [0, %lld)", (long long)p,
                    (long long)parent->n_images);
        SSW_REQUIRE(i == 0 || p > image_positions[i - 1], "ssw_index_create_view: positions must be strictly ascending (entry %lld)",
                    (long long)i);
        const int64_t r0 = parent->has_map ? parent->row_start_host[(size_t)p] : p;
        const int64_t r1 = parent->has_map ? parent->row_start_host[(size_t)p + 1] : p + 1;
        for (int64_t r = r0; r < r1; ++r) src.push_back((int32_t)r);  // (a shard has fewer than 2^31 rows)
        if (parent->has_map) start.push_back((int64_t)src.size());
    }
    const int64_t n = (int64_t)src.size();
    DeviceGuard guard(parent->device);
    if (!guard.ok) {
        set_error("hipSetDevice(%d) failed", parent->device);
        return SSW_ERR_HIP;
    }
    ssw_index *idx = new (std::nothrow) ssw_index();
    if (!idx) return SSW_ERR_NOMEM;
    idx->device = parent->device;
    idx->n = n;
    idx->dim = parent->dim;
    idx->dtype = parent->dtype;
    idx->n_images = m;
    idx->X = parent->X;  // borrowed: owns_X stays false, so the view is never pruned and builds no shadow
    auto fail = [&](ssw_status s) {
        ssw_index_destroy(idx);  // (not yet counted by the parent)
        return s;
    };
    if (hipStreamCreateWithFlags(&idx->own_stream, hipStreamNonBlocking) != hipSuccess) {
        set_error("hipStreamCreate failed");
        return fail(SSW_ERR_HIP);
    }
    idx->stream = idx->own_stream;
    if (hipMalloc((void **)&idx->row_src, (size_t)n * sizeof(int32_t)) != hipSuccess ||
        hipMalloc((void **)&idx->scores, (size_t)(n + 64) * sizeof(float)) != hipSuccess ||
        hipMalloc((void **)&idx->q_dev, (size_t)idx->dim * sizeof(float)) != hipSuccess ||
        (parent->has_map && hipMalloc((void **)&idx->row_start, ((size_t)m + 1) * sizeof(int64_t)) != hipSuccess)) {
        set_error("hipMalloc of the view's row table and score buffer failed");
        return fail(SSW_ERR_NOMEM);
    }
    if (hipMemcpy(idx->row_src, src.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess ||
        (parent->has_map && hipMemcpy(idx->row_start, start.data(), ((size_t)m + 1) * sizeof(int64_t),
                                      hipMemcpyHostToDevice) != hipSuccess)) {
        set_error("ssw_index_create_view: copying the row table failed");
        return fail(SSW_ERR_HIP);
    }
    idx->row_src_host = std::move(src);
    idx->row_start_host = std::move(start);
    idx->has_map = parent->has_map;
    idx->parent = parent;
    ++parent->live_views;
    *out = idx;
    return SSW_OK;
}

ssw_status ssw_index_view_rows(const ssw_index *view, int64_t *out_parent_rows_host) {
    SSW_REQUIRE(view != nullptr && out_parent_rows_host != nullptr, "NULL argument");
    SSW_REQUIRE(view->parent != nullptr, "ssw_index_view_rows: the index is not a view");
    for (size_t j = 0; j < view->row_src_host.size(); ++j) out_parent_rows_host[j] = view->row_src_host[j];
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
    if (dev_vectors && idx->parent) {  // a view has no rows of its own to hand out
        *dev_vectors = nullptr;
    } else if (dev_vectors) {  // the caller may write the rows through it: no shadow from now on
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
    SSW_TRY(refuse_view(idx, "ssw_index_upload"));
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
    SSW_TRY(refuse_view(idx, "ssw_index_upload_f16"));
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
    SSW_TRY(refuse_view(idx, "ssw_index_download"));
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

// the coarse index's rows out of a multiscale index (coarse.hip): every refusal is decided on the host, from the handle's
// host mirror of the image map and the caller's mask, before anything is enqueued
ssw_status ssw_index_coarse_mean(ssw_index *src, const uint8_t *keep_host, const int64_t *images_host, int64_t m,
                                 ssw_index *dst) {
    SSW_REQUIRE(src != nullptr && dst != nullptr && keep_host != nullptr && (m == 0 || images_host != nullptr), "NULL argument");
    if (!src->has_map) {
        set_error("ssw_index_coarse_mean: the source index has no image map (ssw_index_set_row2image)");
        return SSW_ERR_UNSUPPORTED;
    }
    SSW_TRY(refuse_view(dst, "ssw_index_coarse_mean (dst)"));
    SSW_REQUIRE(dst != src && dst != src->parent, "ssw_index_coarse_mean: dst holds the rows src reads");
    SSW_REQUIRE(m >= 0 && dst->n == m && dst->dim == src->dim,
                "ssw_index_coarse_mean: dst is [%lld, %d], need [%lld, %d] (one row a listed image, the source's dim)",
                (long long)dst->n, dst->dim, (long long)m, src->dim);
    SSW_REQUIRE(dst->device == src->device, "ssw_index_coarse_mean: dst is on device %d, src on device %d", dst->device,
                src->device);
    for (int64_t i = 0; i < m; ++i) {
        const int64_t p = images_host[i];
        SSW_REQUIRE(p >= 0 && p < src->n_images, "ssw_index_coarse_mean: image position %lld outside [0, %lld)", (long long)p,
                    (long long)src->n_images);
        SSW_REQUIRE(i == 0 || p > images_host[i - 1], "ssw_index_coarse_mean: positions must be strictly ascending (entry %lld)",
                    (long long)i);
        int64_t r = src->row_start_host[(size_t)p];
        const int64_t r1 = src->row_start_host[(size_t)p + 1];
        while (r < r1 && keep_host[r] == 0) ++r;
        SSW_REQUIRE(r < r1, "ssw_index_coarse_mean: image position %lld has no kept row", (long long)p);
    }
    if (m == 0) return SSW_OK;
    DeviceGuard guard(src->device);
    SSW_TRY(rows_changing(dst));
    if (dst->stream != src->stream) SSW_HIP_TRY(hipStreamSynchronize(dst->stream));  // whatever still reads dst's rows
    hipStream_t s = src->stream;
    // staged for this call alone: the mask (a byte a source row) and the listed positions
    unsigned char *d_keep = nullptr;
    int64_t *d_images = nullptr;
    if (hipMalloc((void **)&d_keep, (size_t)std::max<int64_t>(src->n, 1)) != hipSuccess ||
        hipMalloc((void **)&d_images, (size_t)m * sizeof(int64_t)) != hipSuccess) {
        (void)hipFree(d_keep);
        set_error("ssw_index_coarse_mean: hipMalloc of the %lld mask bytes and %lld positions failed", (long long)src->n,
                  (long long)m);
        return SSW_ERR_NOMEM;
    }
    ssw_status rc = SSW_OK;
    hipError_t e = hipMemcpyAsync(d_keep, keep_host, (size_t)src->n, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d_images, images_host, (size_t)m * sizeof(int64_t), hipMemcpyHostToDevice, s);
    if (e == hipSuccess)  // (ssw_index_profile(src): one event pair around the kernel)
        rc = profiled(src, [&] {
            return launch_coarse_mean(src->X, src->dtype, src->parent ? src->row_src : nullptr, d_keep, src->row_start,
                                      d_images, m, src->dim, dst->X, dst->dtype, src->device, s);
        });
    const hipError_t e2 = hipStreamSynchronize(s);  // the staging is freed below; dst's stream finds the rows written
    if (e == hipSuccess) e = e2;
    (void)hipFree(d_keep);
    (void)hipFree(d_images);
    if (rc != SSW_OK) return rc;
    if (e != hipSuccess) {
        set_error("ssw_index_coarse_mean: %s", hipGetErrorString(e));
        return SSW_ERR_HIP;
    }
    return SSW_OK;
}

ssw_status ssw_index_fill_random(ssw_index *idx, uint64_t seed, int64_t global_first_row) {
    SSW_REQUIRE(idx != nullptr, "idx is NULL");
    SSW_TRY(refuse_view(idx, "ssw_index_fill_random"));
    DeviceGuard guard(idx->device);
    SSW_TRY(rows_changing(idx));
    SSW_TRY(launch_fill_random(idx->X, idx->dtype, idx->n, idx->dim, seed, global_first_row, idx->stream));
    SSW_HIP_TRY(hipStreamSynchronize(idx->stream));
    return SSW_OK;
}

ssw_status ssw_index_set_row2image(ssw_index *idx, const int32_t *row2image_host, int64_t n_images) {
    SSW_REQUIRE(idx != nullptr, "idx is NULL");
    SSW_TRY(refuse_view(idx, "ssw_index_set_row2image"));  // (its image map is its members': ssw_index_create_view)
    // a view's members are rows of the images the parent's map named when the view was made
    SSW_REQUIRE(idx->live_views == 0, "ssw_index_set_row2image: %lld views were made from this index's image map; destroy them first",
                (long long)idx->live_views);
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
    SSW_TRY(check_avg_args(idx, aug_larger, "rescore_avg"));
    DeviceGuard guard(idx->device);
    std::vector<int64_t> off;
    int64_t total = 0, max_tiles = 0;
    SSW_TRY(candidate_geometry(idx, image_positions, m, off, &total, &max_tiles));
    SSW_REQUIRE(max_tiles <= SSW_RESCORE_MAX_TILES, "an image with %lld tiles exceeds the %d the kernel keeps in LDS",
                (long long)max_tiles, SSW_RESCORE_MAX_TILES);
    // after a pruned top-k the kernel reads exact scores on the candidates' tiles and nowhere else: up to SURV_CAP of
    // them are rescored by gather with the kept query and the buffer stays partial; more take the full scan
    PruneState &pr = idx->prune;
    const bool on_demand = idx->scores_partial && total <= SURV_CAP && pr.surv_rows && pr.surv_scores;
    if (!on_demand) SSW_TRY(ensure_full_scores(idx));
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
    if (on_demand) {  // (the survivor lists are free: their own rescoring ran before the wait above)
        SSW_TRY(launch_candidate_tiles(idx->row_start, idx->rs_pos, idx->rs_off, m, pr.surv_rows, s));
        SSW_TRY(rescore_rows(idx, pr.q_last, pr.surv_rows, pr.surv_scores, total, idx->scores, s));
    }
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
    SSW_TRY(check_avg_args(idx, aug_larger, "rescore_avg"));
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

// matrix_rows: the staged rows index the matrix (score_rows, gather_rows), so a view stages its rows' parent rows
static ssw_status stage_rows(ssw_index *idx, const int64_t *rows_host, int64_t n, bool matrix_rows = false) {
    for (int64_t i = 0; i < n; ++i) {
        SSW_REQUIRE(rows_host[i] >= 0 && rows_host[i] < idx->n, "row %lld outside [0, %lld)",
                    (long long)rows_host[i], (long long)idx->n);
    }
    std::vector<int64_t> parent_rows;
    if (matrix_rows && idx->parent) {
        parent_rows.resize((size_t)n);
        for (int64_t i = 0; i < n; ++i) parent_rows[(size_t)i] = idx->row_src_host[(size_t)rows_host[i]];
        rows_host = parent_rows.data();  // (push copies it into the pinned block before it returns)
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
    SSW_TRY(stage_rows(idx, rows_host, n, true));
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
    if (idx->scores_partial && n <= SURV_CAP) {
        // after a pruned top-k: the requested rows scored with the kept query, the scan's bits; the buffer stays partial
        // (never a view, which is not pruned; its rows would be translated all the same)
        SSW_TRY(stage_rows(idx, rows_host, n, true));
        SSW_TRY(launch_score_rows(idx->X, idx->dtype, idx->prune.q_last, idx->gather_idx, n, idx->dim, idx->gather_out,
                                  idx->stream));
        idx->prune.rescored_rows += n;
    } else {
        SSW_TRY(ensure_full_scores(idx));
        SSW_TRY(stage_rows(idx, rows_host, n));
        SSW_TRY(launch_gather_f32(idx->scores, idx->gather_idx, n, idx->gather_out, idx->stream));
    }
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
    DeviceGuard guard(idx->device);
    SSW_TRY(stage_rows(idx, rows_host, n, true));
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
    SSW_TRY(refuse_view(idx, "ssw_index_set_exchange_target"));
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

// the target of the batched form (ssw_index_topk_batch_dev): n_slots messages, beside the single target
ssw_status ssw_index_set_exchange_target_batch(ssw_index *idx, uint64_t *dev_msgs_or_null, int32_t n_slots, int32_t k_max,
                                               int32_t with_best, int64_t image_offset, int64_t row_offset) {
    SSW_REQUIRE(idx != nullptr, "idx is NULL");
    SSW_TRY(refuse_view(idx, "ssw_index_set_exchange_target_batch"));
    FinalExchange x;
    if (dev_msgs_or_null) {
        SSW_REQUIRE(n_slots >= 1, "n_slots=%d < 1", n_slots);
        SSW_REQUIRE(k_max >= 1 && k_max <= SSW_MAX_TOPK && image_offset >= 0, "bad message geometry");
        x.msg_out = dev_msgs_or_null;
        x.image_offset = (uint64_t)image_offset;
        x.row_offset = row_offset;
        x.k_max = k_max;
        x.with_best = with_best ? 1 : 0;
        x.msg_len = (with_best ? 2 : 1) * k_max + 1;
    }
    idx->xchg_batch = x;
    idx->xchg_batch_slots = dev_msgs_or_null ? n_slots : 0;
    return SSW_OK;
}

ssw_status ssw_topk_merge_msgs_batch_dev(int32_t device, void *hip_stream, const uint64_t *dev_msgs, int32_t world,
                                         int64_t rank_stride, int32_t nq, int32_t k_max, int32_t with_best, int32_t k,
                                         uint64_t *dev_keys_out, int32_t *dev_counts_out, int64_t *dev_flags_or_null,
                                         int64_t *dev_flags_seen_or_null) {
    SSW_REQUIRE(dev_msgs && dev_keys_out && dev_counts_out, "NULL argument");
    DeviceGuard guard(device);
    return launch_merge_msgs_batch(dev_msgs, world, rank_stride, nq, k_max, with_best, k, dev_keys_out, dev_counts_out,
                                   reinterpret_cast<long long *>(dev_flags_or_null),
                                   reinterpret_cast<long long *>(dev_flags_seen_or_null), (hipStream_t)hip_stream);
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
ssw_status ssw_tune_scan(int32_t variant, int32_t blocks_per_cu) {
    tune_scan(variant, blocks_per_cu);
    return SSW_OK;
}

ssw_status ssw_tune_scan_batch(int32_t max_width, int32_t blocks_per_cu) {
    tune_scan_batch(max_width, blocks_per_cu);
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

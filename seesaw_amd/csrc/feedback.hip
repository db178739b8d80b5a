// feedback.hip -- online relevance-feedback update: fused loss + gradient kernels and the
// L-BFGS (strong Wolfe) driver that turns labelled tile vectors into the next query vector
// (gfx950 / MI355X).  This file holds the engine's C entry points; the map of the rest is below.
//
// Replaces, for the two linear scorers the feedback loops fit every round:
//   LogisticRegressionPT / LogisticRegModule     seesaw/logistic_regression.py:68-124,270-421
//       mean_i BCEWithLogits(x_i.w + b, y_i; weight_i, pos_weight) + (lambda/n) R(w),
//       R = (|w|-1)^2 + |w/|w| - q/|q||^2   (vector regulariser, :304-330)
//   RegModule ("seesaw" / MultiReg)              seesaw/loops/multi_reg.py:24-134
//       sum_i sw_i item_i + l_norm (cosh(log w.w) - 1) + l_data w'(X'LX)w + l_query (1 - w^.q^)/2,
//       item = BCE (balanced re-weighting :90-105) | pairwise hinge (:106-112, rank_loss.py:63-95)
//              | pairwise logistic (:113-119, rank_loss.py:34-61)
//   MultiRegModule (the multi_reg_neg loop's two-output scorer)   seesaw/loops/multi_reg_module.py:40-165
//       two logits a row from the L2-normalised rows of W [2, dim]; vertical BCE pair + horizontal CE on the labelled
//       rows + l_norm sum_c (cosh(log |W_c|) - 1) + l_query sum_c (1 - w^_c.q^)/2, all f32
//   torch.optim.LBFGS(line_search_fn="strong_wolfe") closure loop   seesaw/basic_trainer.py:11-69
//
// The reference evaluates the closure through Python autograd (with anomaly detection on)
// up to 1.25 x max_iter times per refine; the math per evaluation is two skinny GEMVs
// (n x 512, n = labelled tile vectors, up to ~10^4 with pseudo-labels) plus O(n^2) pairwise
// terms.  Two drivers over the same arithmetic (bit-identical fits, tests/test_feedback_gpu.py):
//   * n <= 1024 rows (every feedback session): k_fb_fit_wg -- the whole optimizer.step(closure), i.e. L-BFGS
//     direction updates, strong-Wolfe line search and all closure evaluations, in ONE launch of one workgroup;
//     k_fb_fit_wg_batch (ssw_fb_fit_batch) is that workgroup once per session of a group that refines in lock step,
//     S fits in one launch and one host wait: the call site it replaces S times is the LBFGS of
//     seesaw/loops/multi_reg.py:156 stepped by seesaw/basic_trainer.py:59-63 (opt.step(closure)), which the
//     reference runs once per session and spreads over Ray actors;
//   * larger sets (PseudoLR's 10 000 pseudo-labelled rows) and the rank objective: the host walks the same
//     state machine and launches one evaluation at a time = 3-4 small kernels on rows that already sit in HBM:
//       fb_logits   z = Xc w (+ b)                        wave per row, coalesced 16-B loads
//       fb_pairwise per-item pairwise loss + dL/dz        one workgroup, z and targets in LDS
//       fb_elem     per-item BCE loss + dL/dz             elementwise
//       fb_grad     partial g = Xc' r per 32-row slab     thread per column, coalesced
//       fb_final    fixed-order reduction of the partials + regulariser terms -> [loss, grad]
// The two-output objective has three forms.  ssw_fb_fit2 / ssw_fb_lossgrad2 (the default, its bits kept): the host
// drives, and per evaluation the data part runs on the device (k_fb2_logits_elem, k_fb_grad twice, k_fb2_reduce) and the
// O(dim) part -- F.normalize, its chain rule, the two regularisers -- on the host.  Opt-in, ssw_fb_lossgrad2_dev /
// ssw_fb_fit2_batch: the O(dim) part on the device too (fb2_norm_body / fb2_tail_body of fb_math.h, in the host
// tail's operation order; only logf / coshf / sinhf are the device library's), under two drivers that return
// bit-identical fits (tests/test_fit2_device_gpu.py):
//   * n <= 1024 rows: k_fb_fit2_wg -- the whole step(closure) in one launch, fit_driver_step<16> around new evaluation
//     phases; k_fb_fit2_wg_batch is that workgroup once per engine, S sessions' fits in one launch and one host wait;
//   * larger sets, or SSW_FB_HOST_DRIVER: lbfgs_host over fb_eval2_dev -- one copy of W, k_fb2_norm, k_fb2_logits_elem,
//     k_fb_grad twice, k_fb2_final_dev and one wait per evaluation, no host arithmetic.
// Bound: issue / launch latency, not HBM -- nothing here is GEMM-shaped enough for MFMA.  Compiled with
// -ffp-contract=off (Makefile), like the four files below: the host driver and the device driver must round alike,
// and the expressions that are meant to be fused say fmaf.
//
// The engine's sources:
//   fb_math.h            the arithmetic both drivers share, and nothing else -- the bit-identity contract
//   fb_handle.h          struct ssw_fb, FitWgArgs, Evaluator, the host functions that cross the files below
//   feedback_eval.hip    data-preparation and per-evaluation kernels; fb_reserve, fb_center, fb_prepare, fb_eval, fb_eval2,
//                        fb_eval2_dev
//   feedback_fit_wg.hip  k_fb_fit_wg / k_fb_fit_wg_batch, their LDS map, phases and driver step, and their host side;
//                        k_fb_fit2_wg / k_fb_fit2_wg_batch on the same driver step
//   feedback_lbfgs.hip   the host L-BFGS: strong_wolfe, lbfgs_host
//   feedback.hip         the C entry points (ssw_fb_*, ssw_rank_pairwise): no kernel, no device code
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <string>
#include <vector>

#include "fb_handle.h"

using namespace ssw;

extern "C" {

ssw_status ssw_fb_destroy(ssw_fb *fb) {
    if (!fb) return SSW_OK;
    DeviceGuard guard(fb->device);
    if (fb->stream) (void)hipStreamSynchronize(fb->stream);
    fb->th_stage.release();
    fb->drawn_stage.release();
    (void)hipFree(fb->th);
    (void)hipFree(fb->drawn);
    fb->rows_stage.release();
    fb->y_stage.release();
    fb->q_stage.release();
    fb->coef_stage.release();
    (void)hipFree(fb->X);
    (void)hipFree(fb->mu);
    (void)hipFree(fb->y);
    (void)hipFree(fb->coef);
    (void)hipFree(fb->z);
    (void)hipFree(fb->item);
    (void)hipFree(fb->r);
    (void)hipFree(fb->rows);
    (void)hipFree(fb->partial);
    (void)hipFree(fb->gsum);
    (void)hipFree(fb->rankg);
    for (float *p2 : {fb->y2, fb->sw2, fb->z2, fb->r2, fb->itemv, fb->itemh, fb->partial2, fb->nw2, fb->w2}) (void)hipFree(p2);
    if (fb->out2_host) (void)hipHostFree(fb->out2_host);
    (void)hipFree(fb->colsum);
    (void)hipFree(fb->w);
    (void)hipFree(fb->qhat);
    (void)hipFree(fb->xlx);
    (void)hipFree(fb->out);
    (void)hipFree(fb->loss_dev);
    (void)hipFree(fb->hist);
    fb->batch_tab_stage.release();
    fb->batch_w_stage.release();
    (void)hipFree(fb->batch_tab);
    (void)hipFree(fb->batch_w);
    if (fb->batch_ev) (void)hipEventDestroy(fb->batch_ev);
    if (fb->loss_host) (void)hipHostFree(fb->loss_host);
    if (fb->out_host) (void)hipHostFree(fb->out_host);
    if (fb->w_host) (void)hipHostFree(fb->w_host);
    if (fb->flag_host) (void)hipHostFree(fb->flag_host);
    if (fb->stream) (void)hipStreamDestroy(fb->stream);
    delete fb;
    return SSW_OK;
}

ssw_status ssw_fb_create(int32_t device, int32_t dim, ssw_fb **out) {
    SSW_REQUIRE(out != nullptr, "out is NULL");
    *out = nullptr;
    if (dim <= 0 || dim % 4 != 0 || dim > 1024) {
        set_error("feedback: dim=%d unsupported (multiple of 4, <= 1024)", dim);
        return SSW_ERR_UNSUPPORTED;
    }
    DeviceGuard guard(device);
    if (!guard.ok) {
        set_error("hipSetDevice(%d) failed", device);
        return SSW_ERR_HIP;
    }
    ssw_fb *fb = new (std::nothrow) ssw_fb();
    if (!fb) return SSW_ERR_NOMEM;
    fb->device = device;
    fb->dim = dim;
    const size_t outn = (size_t)(1 + 2 * dim + 8);  // [loss, gradient (dim + 1, or 2 dim for the two-output objective), parts]
    if (hipStreamCreateWithFlags(&fb->stream, hipStreamNonBlocking) != hipSuccess ||
        hipMalloc((void **)&fb->mu, (size_t)dim * sizeof(float)) != hipSuccess ||
        hipMalloc((void **)&fb->w, (size_t)(dim + 1) * sizeof(float)) != hipSuccess ||
        hipMalloc((void **)&fb->qhat, (size_t)dim * sizeof(float)) != hipSuccess ||
        hipMalloc((void **)&fb->xlx, (size_t)dim * dim * sizeof(float)) != hipSuccess ||
        hipMalloc((void **)&fb->out, outn * sizeof(float)) != hipSuccess ||
        hipMalloc((void **)&fb->loss_dev, sizeof(double)) != hipSuccess ||
        hipMalloc((void **)&fb->hist, (size_t)2 * FIT_HISTORY * 1024 * sizeof(float)) != hipSuccess ||
        hipHostMalloc((void **)&fb->loss_host, sizeof(double), hipHostMallocMapped) != hipSuccess ||
        hipHostMalloc((void **)&fb->out_host, outn * sizeof(float), hipHostMallocMapped) != hipSuccess ||
        hipHostMalloc((void **)&fb->flag_host, 128, hipHostMallocMapped) != hipSuccess ||
        hipHostMalloc((void **)&fb->w_host, (size_t)(2 * dim + 1) * sizeof(float), hipHostMallocDefault) != hipSuccess) {
        set_error("feedback: allocation failed");
        ssw_fb_destroy(fb);
        return SSW_ERR_NOMEM;
    }
    // hipHostMalloc does not zero: a stale completion word equal to the first sequence number would end the
    // first wait before the kernel has written anything
    memset(fb->flag_host, 0, 128);
    memset(fb->out_host, 0, outn * sizeof(float));
    memset(fb->loss_host, 0, sizeof(double));
    if (hipHostGetDevicePointer((void **)&fb->out_host_dev, fb->out_host, 0) != hipSuccess ||
        hipHostGetDevicePointer((void **)&fb->loss_host_dev, fb->loss_host, 0) != hipSuccess ||
        hipHostGetDevicePointer((void **)&fb->flag_host_dev, fb->flag_host, 0) != hipSuccess) {
        set_error("feedback: pinned host memory is not mapped into the device address space");
        ssw_fb_destroy(fb);
        return SSW_ERR_HIP;
    }
    *out = fb;
    return SSW_OK;
}

ssw_status ssw_fb_set_data(ssw_fb *fb, const float *X_host, int64_t n, int32_t center) {
    SSW_REQUIRE(fb != nullptr && n >= 0 && (n == 0 || X_host != nullptr), "bad argument");
    DeviceGuard guard(fb->device);
    SSW_TRY(fb_reserve(fb, n));
    fb->n = n;
    fb->has_targets2 = false;
    fb->targets_on_device = false;  // a new row set: the pseudo-sample's device-made targets (if any) went with the old one
    if (n > 0)
        SSW_HIP_TRY(hipMemcpyAsync(fb->X, X_host, (size_t)n * fb->dim * sizeof(float), hipMemcpyHostToDevice, fb->stream));
    SSW_TRY(fb_center(fb, center));
    SSW_HIP_TRY(hipStreamSynchronize(fb->stream));
    return SSW_OK;
}

static ssw_status fb_set_data_gathered(ssw_fb *fb, const void *dev_matrix, int32_t dtype, int64_t n_matrix_rows,
                                       const int64_t *rows_host, int64_t n, int32_t center) {
    SSW_REQUIRE(fb != nullptr && dev_matrix != nullptr && n >= 0 && (n == 0 || rows_host != nullptr), "bad argument");
    for (int64_t i = 0; i < n; ++i)
        SSW_REQUIRE(rows_host[i] >= 0 && rows_host[i] < n_matrix_rows, "row %lld outside [0, %lld)",
                    (long long)rows_host[i], (long long)n_matrix_rows);
    DeviceGuard guard(fb->device);
    SSW_TRY(fb_reserve(fb, n));
    fb->n = n;
    fb->has_targets2 = false;
    fb->targets_on_device = false;
    if (n > 0) {
        SSW_TRY(fb->rows_stage.push(fb->rows, rows_host, (size_t)n * sizeof(int64_t), fb->stream));
        SSW_TRY(launch_gather_rows(dev_matrix, dtype, fb->rows, 0, n, fb->dim, fb->X, fb->stream));
    }
    SSW_TRY(fb_center(fb, center));
    return SSW_OK;  // no wait: every consumer (the fit, lossgrad, get_mean, scores) is ordered behind this on the stream
}

ssw_status ssw_fb_set_data_from_device(ssw_fb *fb, const float *dev_matrix, int64_t n_matrix_rows,
                                       const int64_t *rows_host, int64_t n, int32_t center) {
    return fb_set_data_gathered(fb, dev_matrix, SSW_DTYPE_F32, n_matrix_rows, rows_host, n, center);
}

// the matrix, its row count and element type out of an index handle whose dim must be the engine's
static ssw_status fb_index_matrix(const ssw_fb *fb, const ssw_index *index, const void **X, int64_t *n_rows,
                                  int32_t *dtype) {
    SSW_REQUIRE(fb != nullptr && index != nullptr, "NULL argument");
    int32_t dim = 0;
    *X = index_matrix(index, n_rows, &dim);
    *dtype = index_dtype(index);
    SSW_REQUIRE(dim == fb->dim, "the index has dim %d, the feedback engine %d", dim, fb->dim);
    return SSW_OK;
}

ssw_status ssw_fb_set_data_from_index(ssw_fb *fb, const ssw_index *index, const int64_t *rows_host, int64_t n,
                                      int32_t center) {
    const void *X = nullptr;
    int64_t n_rows = 0;
    int32_t dtype = SSW_DTYPE_F32;
    SSW_TRY(fb_index_matrix(fb, index, &X, &n_rows, &dtype));
    if (const int32_t *parent_row = index_view_rows(index)) {  // a view: its rows' places in the parent's matrix
        SSW_REQUIRE(n >= 0 && (n == 0 || rows_host != nullptr), "bad argument");
        int64_t n_view = 0;
        SSW_TRY(ssw_index_shape(index, &n_view, nullptr, nullptr));
        std::vector<int64_t> rows((size_t)n);
        for (int64_t i = 0; i < n; ++i) {
            SSW_REQUIRE(rows_host[i] >= 0 && rows_host[i] < n_view, "row %lld outside [0, %lld)", (long long)rows_host[i],
                        (long long)n_view);
            rows[(size_t)i] = parent_row[rows_host[i]];
        }
        return fb_set_data_gathered(fb, X, dtype, n_rows, rows.data(), n, center);  // (staged before it returns)
    }
    return fb_set_data_gathered(fb, X, dtype, n_rows, rows_host, n, center);
}

static ssw_status fb_set_pseudo_sample(ssw_fb *fb, const void *dev_matrix, int32_t dtype, int64_t n_matrix_rows,
                                       const double *dev_scores, const int64_t *labelled_rows_sorted,
                                       const float *labelled_y, int64_t n_lab, const int64_t *drawn, int64_t n_drawn,
                                       float real_weight, int32_t center) {
    SSW_REQUIRE(fb != nullptr && dev_matrix != nullptr && dev_scores != nullptr && n_lab >= 0 && n_drawn >= 0, "bad argument");
    SSW_REQUIRE((n_lab == 0 || (labelled_rows_sorted && labelled_y)) && (n_drawn == 0 || drawn), "bad argument");
    const int64_t n = n_lab + n_drawn, n_unl = n_matrix_rows - n_lab;
    for (int64_t j = 0; j < n_lab; ++j) {
        SSW_REQUIRE(labelled_rows_sorted[j] >= 0 && labelled_rows_sorted[j] < n_matrix_rows &&
                    (j == 0 || labelled_rows_sorted[j] > labelled_rows_sorted[j - 1]), "labelled rows must ascend inside [0, %lld)",
                    (long long)n_matrix_rows);
        SSW_REQUIRE(std::isfinite(labelled_y[j]), "target %lld is not finite", (long long)j);
    }
    for (int64_t i = 0; i < n_drawn; ++i)
        SSW_REQUIRE(drawn[i] >= 0 && drawn[i] < n_unl, "draw %lld outside the %lld unlabelled rows", (long long)drawn[i], (long long)n_unl);
    DeviceGuard guard(fb->device);
    SSW_TRY(fb_reserve(fb, n));
    if (n_lab + 1 > fb->th_cap) {
        SSW_HIP_TRY(hipStreamSynchronize(fb->stream));
        (void)hipFree(fb->th);
        fb->th = nullptr;
        int64_t cap = 1024;
        while (cap < n_lab + 1) cap <<= 1;
        SSW_HIP_TRY(hipMalloc((void **)&fb->th, (size_t)cap * sizeof(int64_t)));
        fb->th_cap = cap;
    }
    if (n_drawn + 1 > fb->drawn_cap) {
        SSW_HIP_TRY(hipStreamSynchronize(fb->stream));
        (void)hipFree(fb->drawn);
        fb->drawn = nullptr;
        int64_t cap = 16384;
        while (cap < n_drawn + 1) cap <<= 1;
        SSW_HIP_TRY(hipMalloc((void **)&fb->drawn, (size_t)cap * sizeof(int64_t)));
        fb->drawn_cap = cap;
    }
    fb->n = n;
    fb->has_targets2 = false;
    fb->targets_on_device = true;
    // host copies for the objective's set-up: the logistic objective reads the weights only
    fb->y_host.assign((size_t)n, 0.f);
    fb->sw_host.assign((size_t)n, 1.f);
    std::vector<int64_t> th((size_t)std::max<int64_t>(n_lab, 1));
    for (int64_t j = 0; j < n_lab; ++j) {
        fb->y_host[(size_t)j] = labelled_y[j];
        fb->sw_host[(size_t)j] = real_weight;
        th[(size_t)j] = labelled_rows_sorted[j] - j;
    }
    if (n > 0) {
        // labelled part: row ids and targets as ssw_fb_set_data_from_device / ssw_fb_set_targets upload them
        if (n_lab > 0) {
            SSW_TRY(fb->rows_stage.push(fb->rows, labelled_rows_sorted, (size_t)n_lab * sizeof(int64_t), fb->stream));
            SSW_TRY(fb->y_stage.push(fb->y, fb->y_host.data(), (size_t)n_lab * sizeof(float), fb->stream));
            SSW_TRY(fb->th_stage.push(fb->th, th.data(), (size_t)n_lab * sizeof(int64_t), fb->stream));
        }
        if (n_drawn > 0) {
            SSW_TRY(fb->drawn_stage.push(fb->drawn, drawn, (size_t)n_drawn * sizeof(int64_t), fb->stream));
            launch_fb_pseudo_rows(fb, n_lab, n_drawn, dev_scores, n_matrix_rows);
        }
        SSW_TRY(launch_gather_rows(dev_matrix, dtype, fb->rows, 0, n, fb->dim, fb->X, fb->stream));
    }
    SSW_TRY(fb_center(fb, center));
    return SSW_OK;  // no wait: the fit is ordered behind this on the stream
}

ssw_status ssw_fb_set_pseudo_sample(ssw_fb *fb, const float *dev_matrix, int64_t n_matrix_rows, const double *dev_scores,
                                    const int64_t *labelled_rows_sorted, const float *labelled_y, int64_t n_lab,
                                    const int64_t *drawn, int64_t n_drawn, float real_weight, int32_t center) {
    return fb_set_pseudo_sample(fb, dev_matrix, SSW_DTYPE_F32, n_matrix_rows, dev_scores, labelled_rows_sorted, labelled_y,
                                n_lab, drawn, n_drawn, real_weight, center);
}

ssw_status ssw_fb_set_pseudo_sample_from_index(ssw_fb *fb, const ssw_index *index, const double *dev_scores,
                                               const int64_t *labelled_rows_sorted, const float *labelled_y,
                                               int64_t n_lab, const int64_t *drawn, int64_t n_drawn, float real_weight,
                                               int32_t center) {
    const void *X = nullptr;
    int64_t n_rows = 0;
    int32_t dtype = SSW_DTYPE_F32;
    SSW_TRY(refuse_view(index, "ssw_fb_set_pseudo_sample_from_index"));  // its rows are drawn on the device, by row number
    SSW_TRY(fb_index_matrix(fb, index, &X, &n_rows, &dtype));
    return fb_set_pseudo_sample(fb, X, dtype, n_rows, dev_scores, labelled_rows_sorted, labelled_y, n_lab, drawn, n_drawn,
                                real_weight, center);
}

ssw_status ssw_fb_set_targets(ssw_fb *fb, const float *y_host, const float *sample_weight_or_null) {
    SSW_REQUIRE(fb != nullptr && (fb->n == 0 || y_host != nullptr), "bad argument");
    DeviceGuard guard(fb->device);
    const int64_t n = fb->n;
    fb->targets_on_device = false;
    fb->y_host.assign(y_host, y_host + n);
    if (sample_weight_or_null)
        fb->sw_host.assign(sample_weight_or_null, sample_weight_or_null + n);
    else
        fb->sw_host.clear();
    for (int64_t i = 0; i < n; ++i)
        SSW_REQUIRE(std::isfinite(y_host[i]), "target %lld is not finite", (long long)i);
    if (n > 0) {
        SSW_TRY(fb->y_stage.push(fb->y, fb->y_host.data(), (size_t)n * sizeof(float), fb->stream));
    }
    return SSW_OK;
}

ssw_status ssw_fb_set_query(ssw_fb *fb, const float *q_host) {
    SSW_REQUIRE(fb != nullptr && q_host != nullptr, "bad argument");
    DeviceGuard guard(fb->device);
    double nn = 0;
    for (int i = 0; i < fb->dim; ++i) nn += (double)q_host[i] * q_host[i];
    SSW_REQUIRE(nn > 0 && std::isfinite(nn), "query vector has zero or non-finite norm");
    const double inv = 1.0 / std::fmax(std::sqrt(nn), 1e-12);
    std::vector<float> qh((size_t)fb->dim);
    for (int i = 0; i < fb->dim; ++i) qh[(size_t)i] = (float)(q_host[i] * inv);  // F.normalize
    if (fb->has_q && fb->qhat_host.size() == qh.size() && memcmp(fb->qhat_host.data(), qh.data(), qh.size() * sizeof(float)) == 0)
        return SSW_OK;  // a session hands over the same text vector every round: already installed
    SSW_TRY(fb->q_stage.push(fb->qhat, qh.data(), (size_t)fb->dim * sizeof(float), fb->stream));
    fb->qhat_host = qh;
    fb->has_q = true;
    return SSW_OK;
}

ssw_status ssw_fb_set_xlx(ssw_fb *fb, const float *xlx_host) {
    SSW_REQUIRE(fb != nullptr && xlx_host != nullptr, "bad argument");
    DeviceGuard guard(fb->device);
    SSW_HIP_TRY(hipMemcpy(fb->xlx, xlx_host, (size_t)fb->dim * fb->dim * sizeof(float), hipMemcpyHostToDevice));
    fb->has_xlx = true;
    return SSW_OK;
}

ssw_status ssw_fb_get_mean(ssw_fb *fb, float *out_mu_host) {
    SSW_REQUIRE(fb != nullptr && out_mu_host != nullptr, "bad argument");
    DeviceGuard guard(fb->device);
    SSW_HIP_TRY(hipMemcpyAsync(out_mu_host, fb->mu, (size_t)fb->dim * sizeof(float), hipMemcpyDeviceToHost, fb->stream));
    SSW_HIP_TRY(hipStreamSynchronize(fb->stream));  // behind the centring kernels of set_data on the same stream
    return SSW_OK;
}

ssw_status ssw_fb_lossgrad(ssw_fb *fb, const ssw_fb_objective *obj, const float *w_host, float *out_loss,
                           float *out_grad, float *out_parts4_or_null) {
    SSW_REQUIRE(fb && obj && w_host && out_loss && out_grad, "NULL argument");
    DeviceGuard guard(fb->device);
    const int P = fb_fit_params(fb, obj);
    FbObjDev dev;
    float pw = 1.f;
    bool pa = false;
    SSW_TRY(fb_prepare(fb, obj, &dev, &pw, &pa));
    memcpy(fb->w_host, w_host, (size_t)P * sizeof(float));
    if (P == fb->dim) fb->w_host[fb->dim] = 0.f;
    SSW_TRY(fb_eval(fb, obj, dev, pw, pa, fb->dim + 1));
    *out_loss = (float)fb->loss_host[0];
    memcpy(out_grad, fb->out_host + 1, (size_t)P * sizeof(float));
    if (out_parts4_or_null) memcpy(out_parts4_or_null, fb->out_host + 1 + fb->dim + 1, 4 * sizeof(float));
    return SSW_OK;
}

ssw_status ssw_fb_scores(ssw_fb *fb, const float *w_host, int32_t has_bias, float *out_logits) {
    SSW_REQUIRE(fb && w_host && (fb->n == 0 || out_logits), "NULL argument");
    DeviceGuard guard(fb->device);
    if (fb->n == 0) return SSW_OK;
    memcpy(fb->w_host, w_host, (size_t)(fb->dim + (has_bias ? 1 : 0)) * sizeof(float));
    SSW_HIP_TRY(hipMemcpyAsync(fb->w, fb->w_host, (size_t)(fb->dim + 1) * sizeof(float), hipMemcpyHostToDevice, fb->stream));
    launch_fb_logits(fb, has_bias);
    SSW_HIP_TRY(hipMemcpyAsync(out_logits, fb->z, (size_t)fb->n * sizeof(float), hipMemcpyDeviceToHost, fb->stream));
    SSW_HIP_TRY(hipStreamSynchronize(fb->stream));
    return SSW_OK;
}

// The host-driven fit behind ssw_fb_fit and ssw_fb_fit2: lbfgs_host from the caller's `P` weights (E.P >= P parameters
// go to the device, the rest start at 0), the divergence check, the bookkeeping and the outputs
static ssw_status fb_fit_host(Evaluator &E, int P, int zero_slot, float *w_inout, int32_t max_iter, float lr,
                              int32_t *out_iters, int32_t *out_evals, float *out_final_loss) {
    std::vector<float> x((size_t)E.P, 0.f);
    for (int i = 0; i < P; ++i) {
        SSW_REQUIRE(std::isfinite(w_inout[i]), "initial weight %d is not finite", i);
        x[(size_t)i] = w_inout[i];
    }
    int n_iter = 0;
    double loss = 0;
    SSW_TRY(lbfgs_host(E, x, zero_slot, max_iter, lr, &n_iter, &loss));
    for (int i = 0; i < P; ++i) {
        if (!std::isfinite(x[(size_t)i])) {
            set_error("feedback: weights diverged");
            return SSW_ERR_NUMERIC;
        }
        w_inout[i] = x[(size_t)i];
    }
    E.fb->last_iters = n_iter;
    if (out_iters) *out_iters = n_iter;
    if (out_evals) *out_evals = E.fb->last_evals;
    if (out_final_loss) *out_final_loss = (float)loss;
    return SSW_OK;
}

ssw_status ssw_fb_fit(ssw_fb *fb, const ssw_fb_objective *obj, float *w_inout, int32_t max_iter, float lr,
                      int32_t *out_iters, int32_t *out_evals, float *out_final_loss) {
    SSW_REQUIRE(fb && obj && w_inout, "NULL argument");
    SSW_REQUIRE(max_iter >= 1, "max_iter < 1");
    DeviceGuard guard(fb->device);
    const int P = fb_fit_params(fb, obj);
    Evaluator E;
    E.fb = fb;
    E.o = obj;
    E.P = fb->dim + 1;  // the device always sees dim+1 parameters; slot dim is the (maybe unused) bias
    const auto t_fit0 = std::chrono::steady_clock::now();
    SSW_TRY(fb_prepare(fb, obj, &E.dev, &E.pw, &E.pairwise_active));
    const double prep_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_fit0).count();
    g_fit_eval_s = 0;
    fb->last_evals = 0;
    fb->last_fit_on_device = false;
    // ---- the whole step(closure) in one launch (k_fb_fit_wg) when the labelled set fits one workgroup's reach
    if (fb_fit_wg_eligible(fb, obj)) {
        for (int i = 0; i < P; ++i) SSW_REQUIRE(std::isfinite(w_inout[i]), "initial weight %d is not finite", i);
        FitWgArgs a;
        fb_fit_wg_fill(fb, obj, E.dev, E.pw, E.pairwise_active, max_iter, lr, &a);
        FbW w0v;
        memset(&w0v, 0, sizeof(w0v));
        if (fb->dim + 1 <= FB_ARG_FLOATS) {
            memcpy(w0v.v, w_inout, (size_t)P * sizeof(float));
        } else {
            memcpy(fb->w_host, w_inout, (size_t)P * sizeof(float));
            if (P == fb->dim) fb->w_host[fb->dim] = 0.f;
            SSW_HIP_TRY(hipMemcpyAsync(fb->w, fb->w_host, (size_t)(fb->dim + 1) * sizeof(float), hipMemcpyHostToDevice, fb->stream));
            a.w0_or_null = fb->w;
        }
        SSW_TRY(fb_fit_wg_launch(fb, a, w0v));
        if (!fb_fit_wg_spin(fb, fb->seqno)) SSW_HIP_TRY(hipStreamSynchronize(fb->stream));
        SSW_TRY(fb_fit_wg_collect(fb, P, w_inout, out_iters, out_evals, out_final_loss));
        const int *counts = reinterpret_cast<const int *>(fb->flag_host) + 4;
        if (getenv("SSW_FB_TIMING"))
            fprintf(stderr, "fit (one launch): n=%lld iters=%d evals=%d total %.1f us, prepare %.1f; kernel %.1f us = logits %.1f + "
                    "labels %.1f + gradient %.1f + final %.1f + driver %.1f (%.0f MHz)\n", (long long)fb->n, counts[0], counts[1],
                    1e6 * std::chrono::duration<double>(std::chrono::steady_clock::now() - t_fit0).count(), 1e6 * prep_s,
                    counts[7] * 0.01, counts[3] * 0.01, counts[4] * 0.01, counts[5] * 0.01, counts[6] * 0.01,
                    (counts[7] - counts[3] - counts[4] - counts[5] - counts[6]) * 0.01,
                    counts[7] > 0 ? 16.0 * counts[8] / (counts[7] * 0.01) : 0.0);
        if (getenv("SSW_FB_TIMING"))
            fprintf(stderr, "   of the driver: two-loop recursion %.1f us\n", counts[10] * 0.01);
        if (getenv("SSW_FB_TIMING") && counts[11])
            fprintf(stderr, "   one pass (SSW_FIT_STAMPS build), cycles per evaluation: %.0f, %.0f, %.0f\n",
                    16.0 * counts[11] / counts[1], 16.0 * counts[12] / counts[1], 16.0 * counts[13] / counts[1]);
        return SSW_OK;
    }
    SSW_TRY(fb_fit_host(E, P, P == fb->dim ? fb->dim : -1, w_inout, max_iter, lr, out_iters, out_evals, out_final_loss));
    if (getenv("SSW_FB_TIMING"))
        fprintf(stderr, "fit: n=%lld iters=%d evals=%d total %.1f us, prepare %.1f, evaluations %.1f\n", (long long)fb->n,
                fb->last_iters, fb->last_evals,
                1e6 * std::chrono::duration<double>(std::chrono::steady_clock::now() - t_fit0).count(), 1e6 * prep_s,
                1e6 * g_fit_eval_s);
    return SSW_OK;
}

// ---- S sessions' fits in one launch (k_fb_fit_wg_batch) ----------------------------------------
ssw_status ssw_fb_fit_batch(ssw_fb *const *fbs, const ssw_fb_objective *objs, int32_t nfit, float *W_inout,
                            const int32_t *max_iter, const float *lr, int32_t *out_iters, int32_t *out_evals,
                            float *out_final_loss, int32_t *out_status) {
    // ---- refusals, before anything is queued
    SSW_REQUIRE(nfit >= 1, "nfit < 1");
    SSW_REQUIRE(fbs && objs && W_inout && max_iter && lr && out_status, "NULL argument");
    for (int s = 0; s < nfit; ++s) {
        SSW_REQUIRE(fbs[s] != nullptr, "slot %d: NULL handle", s);
        for (int t = 0; t < s; ++t) SSW_REQUIRE(fbs[t] != fbs[s], "slots %d and %d share one handle", t, s);
        SSW_REQUIRE(fbs[s]->device == fbs[0]->device, "slot %d: device %d, slot 0 is on device %d", s, fbs[s]->device,
                    fbs[0]->device);
        SSW_REQUIRE(fbs[s]->dim == fbs[0]->dim, "slot %d: dim %d, slot 0 has dim %d", s, fbs[s]->dim, fbs[0]->dim);
        SSW_REQUIRE(max_iter[s] >= 1, "slot %d: max_iter < 1", s);
    }
    const int dim = fbs[0]->dim, Pd = dim + 1;
    for (int s = 0; s < nfit; ++s) {
        const int P = fb_fit_params(fbs[s], &objs[s]);
        for (int i = 0; i < P; ++i)
            SSW_REQUIRE(std::isfinite(W_inout[(size_t)s * Pd + i]), "slot %d: initial weight %d is not finite", s, i);
    }
    DeviceGuard guard(fbs[0]->device);
    std::vector<int> slots;  // the slots one workgroup each serves; the others go through ssw_fb_fit afterwards
    for (int s = 0; s < nfit; ++s) {
        fbs[s]->batch_error.clear();
        out_status[s] = SSW_OK;
        if (fb_fit_wg_eligible(fbs[s], &objs[s])) slots.push_back(s);
    }
    // One slot's result, formed by `fit` on a copy of the slot's row: the copy goes back on SSW_OK; SSW_ERR_NUMERIC is
    // the slot's own (its row stays as it came, the others are not concerned); any other status ends the call
    std::vector<float> row((size_t)Pd);
    auto fit_slot = [&](int s, auto &&fit) -> ssw_status {
        float *Ws = &W_inout[(size_t)s * Pd];
        memcpy(row.data(), Ws, (size_t)Pd * sizeof(float));
        const ssw_status st = fit(row.data(), out_iters ? &out_iters[s] : nullptr, out_evals ? &out_evals[s] : nullptr,
                                  out_final_loss ? &out_final_loss[s] : nullptr);
        if (st == SSW_OK) {
            memcpy(Ws, row.data(), (size_t)Pd * sizeof(float));
        } else if (st == SSW_ERR_NUMERIC) {
            out_status[s] = st;
            fbs[s]->batch_error = ssw_last_error();
        } else {
            return st;
        }
        return SSW_OK;
    };
    const int nwg = (int)slots.size();
    if (nwg > 0) {
        ssw_fb *lead = fbs[slots[0]];  // its stream takes the launch, its tables the arguments
        // every engine queues its own uploads (fb_prepare: the coefficients; before it the rows, targets and query of
        // its set_* calls) on its own stream, without a wait
        std::vector<FbObjDev> dev((size_t)nwg);
        std::vector<float> pw((size_t)nwg);
        std::vector<char> active((size_t)nwg);
        for (int b = 0; b < nwg; ++b) {
            ssw_fb *fb = fbs[slots[b]];
            bool pa = false;
            SSW_TRY(fb_prepare(fb, &objs[slots[b]], &dev[b], &pw[b], &pa));
            active[b] = pa;
            fb->last_evals = 0;
            fb->last_fit_on_device = false;
        }
        SSW_TRY(fb_batch_reserve(lead, nwg));
        std::vector<FitWgArgs> tab((size_t)nwg);
        std::vector<float> w0((size_t)nwg * Pd, 0.f);
        for (int b = 0; b < nwg; ++b) {
            const int s = slots[b];
            fb_fit_wg_fill(fbs[s], &objs[s], dev[b], pw[b], active[b] != 0, max_iter[s], lr[s], &tab[b]);
            tab[b].w0_or_null = lead->batch_w + (size_t)b * Pd;
            memcpy(&w0[(size_t)b * Pd], &W_inout[(size_t)s * Pd], (size_t)tab[b].P * sizeof(float));
        }
        SSW_TRY(lead->batch_tab_stage.push(lead->batch_tab, tab.data(), tab.size() * sizeof(FitWgArgs), lead->stream));
        SSW_TRY(lead->batch_w_stage.push(lead->batch_w, w0.data(), w0.size() * sizeof(float), lead->stream));
        for (int b = 1; b < nwg; ++b) {  // the launch is ordered behind every slot's uploads
            ssw_fb *fb = fbs[slots[b]];
            if (!fb->batch_ev) SSW_HIP_TRY(hipEventCreateWithFlags(&fb->batch_ev, hipEventDisableTiming));
            SSW_HIP_TRY(hipEventRecord(fb->batch_ev, fb->stream));
            SSW_HIP_TRY(hipStreamWaitEvent(lead->stream, fb->batch_ev, 0));
        }
        SSW_TRY(fb_fit_wg_launch_batch(lead, tab.data(), nwg));
        for (int b = 0; b < nwg; ++b) {
            if (!fb_fit_wg_spin(fbs[slots[b]], tab[b].seqno)) {
                SSW_HIP_TRY(hipStreamSynchronize(lead->stream));  // every workgroup has published
                break;
            }
        }
        for (int b = 0; b < nwg; ++b) {
            const int s = slots[b];
            SSW_TRY(fit_slot(s, [&](float *w, int32_t *iters, int32_t *evals, float *final_loss) {
                return fb_fit_wg_collect(fbs[s], tab[b].P, w, iters, evals, final_loss);
            }));
        }
    }
    // ---- the slots the single call drives from the host: through it, one after another
    size_t next_wg = 0;
    for (int s = 0; s < nfit; ++s) {
        if (next_wg < slots.size() && slots[next_wg] == s) {
            ++next_wg;
            continue;
        }
        SSW_TRY(fit_slot(s, [&](float *w, int32_t *iters, int32_t *evals, float *final_loss) {
            return ssw_fb_fit(fbs[s], &objs[s], w, max_iter[s], lr[s], iters, evals, final_loss);
        }));
    }
    return SSW_OK;
}

const char *ssw_fb_batch_error(const ssw_fb *fb) { return fb ? fb->batch_error.c_str() : ""; }

// ---- MultiRegModule (multi_reg_neg loop): two-output objective -------------------------------
ssw_status ssw_fb_set_targets2(ssw_fb *fb, const float *y2_host, const float *sample_weight_or_null) {
    SSW_REQUIRE(fb != nullptr && (fb->n == 0 || y2_host != nullptr), "bad argument");
    DeviceGuard guard(fb->device);
    SSW_REQUIRE(2 * fb->dim <= 1024, "feedback: the two-output objective takes dim <= 512, got %d", fb->dim);
    SSW_TRY(fb2_reserve(fb));
    const int64_t n = fb->n, plane = fb->cap2;
    std::vector<float> buf((size_t)3 * n);
    for (int64_t i = 0; i < n; ++i) {
        SSW_REQUIRE(std::isfinite(y2_host[2 * i]) && std::isfinite(y2_host[2 * i + 1]), "target %lld is not finite", (long long)i);
        buf[(size_t)i] = y2_host[2 * i];
        buf[(size_t)(n + i)] = y2_host[2 * i + 1];
        buf[(size_t)(2 * n + i)] = sample_weight_or_null ? sample_weight_or_null[i] : 1.f;
        SSW_REQUIRE(std::isfinite(buf[(size_t)(2 * n + i)]), "sample weight %lld is not finite", (long long)i);
    }
    if (n > 0) {
        SSW_HIP_TRY(hipMemcpyAsync(fb->y2, buf.data(), (size_t)n * sizeof(float), hipMemcpyHostToDevice, fb->stream));
        SSW_HIP_TRY(hipMemcpyAsync(fb->y2 + plane, buf.data() + n, (size_t)n * sizeof(float), hipMemcpyHostToDevice, fb->stream));
        SSW_HIP_TRY(hipMemcpyAsync(fb->sw2, buf.data() + 2 * n, (size_t)n * sizeof(float), hipMemcpyHostToDevice, fb->stream));
        SSW_HIP_TRY(hipStreamSynchronize(fb->stream));
    }
    fb->has_targets2 = true;
    return SSW_OK;
}

ssw_status ssw_fb_lossgrad2(ssw_fb *fb, const float *W_host, float reg_norm_lambda, float reg_query_lambda,
                            float *out_loss, float *out_grad, float *out_parts5_or_null) {
    SSW_REQUIRE(fb && W_host && out_loss && out_grad, "NULL argument");
    DeviceGuard guard(fb->device);
    SSW_REQUIRE(2 * fb->dim <= 1024, "feedback: the two-output objective takes dim <= 512, got %d", fb->dim);
    memcpy(fb->w_host, W_host, (size_t)2 * fb->dim * sizeof(float));
    SSW_TRY(fb_eval2(fb, reg_norm_lambda, reg_query_lambda, out_parts5_or_null));
    *out_loss = (float)fb->loss_host[0];
    memcpy(out_grad, fb->out_host + 1, (size_t)2 * fb->dim * sizeof(float));
    return SSW_OK;
}

ssw_status ssw_fb_fit2(ssw_fb *fb, float *W_inout, float reg_norm_lambda, float reg_query_lambda, int32_t max_iter,
                       float lr, int32_t *out_iters, int32_t *out_evals, float *out_final_loss) {
    SSW_REQUIRE(fb && W_inout, "NULL argument");
    SSW_REQUIRE(max_iter >= 1, "max_iter < 1");
    DeviceGuard guard(fb->device);
    SSW_REQUIRE(2 * fb->dim <= 1024, "feedback: the two-output objective takes dim <= 512, got %d", fb->dim);
    Evaluator E;
    E.fb = fb;
    E.o = nullptr;
    E.P = 2 * fb->dim;
    E.two = true;
    E.l_norm2 = reg_norm_lambda;
    E.l_query2 = reg_query_lambda;
    E.pw = 1.f;
    E.pairwise_active = false;
    memset(&E.dev, 0, sizeof(E.dev));
    fb->last_evals = 0;
    fb->last_fit_on_device = false;
    return fb_fit_host(E, E.P, -1, W_inout, max_iter, lr, out_iters, out_evals, out_final_loss);
}

// ---- the two-output objective evaluated and fitted entirely on the device (opt-in) ---------------
ssw_status ssw_fb_lossgrad2_dev(ssw_fb *fb, const float *W_host, float reg_norm_lambda, float reg_query_lambda,
                                float *out_loss, float *out_grad, float *out_parts5_or_null) {
    SSW_REQUIRE(fb && W_host && out_loss && out_grad, "NULL argument");
    DeviceGuard guard(fb->device);
    SSW_REQUIRE(2 * fb->dim <= 1024, "feedback: the two-output objective takes dim <= 512, got %d", fb->dim);
    memcpy(fb->w_host, W_host, (size_t)2 * fb->dim * sizeof(float));
    SSW_TRY(fb_eval2_dev(fb, reg_norm_lambda, reg_query_lambda, out_parts5_or_null));
    *out_loss = (float)fb->loss_host[0];
    memcpy(out_grad, fb->out_host + 1, (size_t)2 * fb->dim * sizeof(float));
    return SSW_OK;
}

// the host-driven fit over the device evaluation: the driver k_fb_fit2_wg is pinned on, and the path of the sets
// one workgroup does not reach
static ssw_status fb_fit2_host_dev(ssw_fb *fb, float *W_inout, float l_norm, float l_query, int32_t max_iter, float lr,
                                   int32_t *out_iters, int32_t *out_evals, float *out_final_loss) {
    Evaluator E;
    E.fb = fb;
    E.o = nullptr;
    E.P = 2 * fb->dim;
    E.two = true;
    E.two_dev = true;
    E.l_norm2 = l_norm;
    E.l_query2 = l_query;
    E.pw = 1.f;
    E.pairwise_active = false;
    memset(&E.dev, 0, sizeof(E.dev));
    fb->last_evals = 0;
    fb->last_fit_on_device = false;
    return fb_fit_host(E, E.P, -1, W_inout, max_iter, lr, out_iters, out_evals, out_final_loss);
}

ssw_status ssw_fb_fit2_batch(ssw_fb *const *fbs, int32_t nfit, float *W_inout, const float *reg_norm_lambda,
                             const float *reg_query_lambda, const int32_t *max_iter, const float *lr, int32_t *out_iters,
                             int32_t *out_evals, float *out_final_loss, int32_t *out_status) {
    // ---- refusals, before anything is queued
    SSW_REQUIRE(nfit >= 1, "nfit < 1");
    SSW_REQUIRE(fbs && W_inout && reg_norm_lambda && reg_query_lambda && max_iter && lr && out_status, "NULL argument");
    for (int s = 0; s < nfit; ++s) {
        SSW_REQUIRE(fbs[s] != nullptr, "slot %d: NULL handle", s);
        for (int t = 0; t < s; ++t) SSW_REQUIRE(fbs[t] != fbs[s], "slots %d and %d share one handle", t, s);
        SSW_REQUIRE(fbs[s]->device == fbs[0]->device, "slot %d: device %d, slot 0 is on device %d", s, fbs[s]->device,
                    fbs[0]->device);
        SSW_REQUIRE(fbs[s]->dim == fbs[0]->dim, "slot %d: dim %d, slot 0 has dim %d", s, fbs[s]->dim, fbs[0]->dim);
        SSW_REQUIRE(max_iter[s] >= 1, "slot %d: max_iter < 1", s);
    }
    const int dim = fbs[0]->dim, P = 2 * dim;
    SSW_REQUIRE(P <= 1024, "feedback: the two-output objective takes dim <= 512, got %d", dim);
    for (int s = 0; s < nfit; ++s) {
        const ssw_fb *fb = fbs[s];
        SSW_REQUIRE(fb->n == 0 || (fb->has_targets2 && fb->cap2 >= fb->cap),
                    "slot %d: ssw_fb_set_targets2 has not been called for these rows", s);
        SSW_REQUIRE(fb->has_q, "slot %d: the two-output objective needs ssw_fb_set_query first", s);
        for (int i = 0; i < P; ++i)
            SSW_REQUIRE(std::isfinite(W_inout[(size_t)s * P + i]), "slot %d: initial weight %d is not finite", s, i);
    }
    DeviceGuard guard(fbs[0]->device);
    std::vector<int> slots;  // the slots one workgroup each serves; the others are driven from the host afterwards
    for (int s = 0; s < nfit; ++s) {
        fbs[s]->batch_error.clear();
        out_status[s] = SSW_OK;
        if (fb_fit2_wg_eligible(fbs[s])) slots.push_back(s);
    }
    // one slot's result, formed on a copy of the slot's row (as in ssw_fb_fit_batch)
    std::vector<float> row((size_t)P);
    auto fit_slot = [&](int s, auto &&fit) -> ssw_status {
        float *Ws = &W_inout[(size_t)s * P];
        memcpy(row.data(), Ws, (size_t)P * sizeof(float));
        const ssw_status st = fit(row.data(), out_iters ? &out_iters[s] : nullptr, out_evals ? &out_evals[s] : nullptr,
                                  out_final_loss ? &out_final_loss[s] : nullptr);
        if (st == SSW_OK) {
            memcpy(Ws, row.data(), (size_t)P * sizeof(float));
        } else if (st == SSW_ERR_NUMERIC) {
            out_status[s] = st;
            fbs[s]->batch_error = ssw_last_error();
        } else {
            return st;
        }
        return SSW_OK;
    };
    const int nwg = (int)slots.size();
    if (nwg > 0) {
        ssw_fb *lead = fbs[slots[0]];  // its stream takes the launch, its tables the arguments and start vectors
        const int wrow = 2 * (dim + 1);  // the start-vector table's rows are dim + 1 wide: a slot's 2 dim floats take two
        SSW_TRY(fb_batch_reserve(lead, 2 * nwg));
        std::vector<FitWgArgs> tab((size_t)nwg);
        std::vector<float> w0((size_t)nwg * wrow, 0.f);
        for (int b = 0; b < nwg; ++b) {
            const int s = slots[b];
            fbs[s]->last_evals = 0;
            fbs[s]->last_fit_on_device = false;
            fb_fit2_wg_fill(fbs[s], reg_norm_lambda[s], reg_query_lambda[s], max_iter[s], lr[s],
                            lead->batch_w + (size_t)b * wrow, &tab[b]);
            memcpy(&w0[(size_t)b * wrow], &W_inout[(size_t)s * P], (size_t)P * sizeof(float));
        }
        if (nwg > 1) SSW_TRY(lead->batch_tab_stage.push(lead->batch_tab, tab.data(), tab.size() * sizeof(FitWgArgs), lead->stream));
        SSW_TRY(lead->batch_w_stage.push(lead->batch_w, w0.data(), w0.size() * sizeof(float), lead->stream));
        for (int b = 1; b < nwg; ++b) {  // the launch is ordered behind every slot's uploads
            ssw_fb *fb = fbs[slots[b]];
            if (!fb->batch_ev) SSW_HIP_TRY(hipEventCreateWithFlags(&fb->batch_ev, hipEventDisableTiming));
            SSW_HIP_TRY(hipEventRecord(fb->batch_ev, fb->stream));
            SSW_HIP_TRY(hipStreamWaitEvent(lead->stream, fb->batch_ev, 0));
        }
        SSW_TRY(fb_fit2_wg_launch(lead, tab.data(), nwg));
        for (int b = 0; b < nwg; ++b) {
            if (!fb_fit_wg_spin(fbs[slots[b]], tab[b].seqno)) {
                SSW_HIP_TRY(hipStreamSynchronize(lead->stream));  // every workgroup has published
                break;
            }
        }
        for (int b = 0; b < nwg; ++b) {
            const int s = slots[b];
            SSW_TRY(fit_slot(s, [&](float *w, int32_t *iters, int32_t *evals, float *final_loss) {
                return fb_fit_wg_collect(fbs[s], P, w, iters, evals, final_loss);
            }));
        }
    }
    // ---- the slots driven from the host, one evaluation at a time on the device: one after another
    size_t next_wg = 0;
    for (int s = 0; s < nfit; ++s) {
        if (next_wg < slots.size() && slots[next_wg] == s) {
            ++next_wg;
            continue;
        }
        SSW_TRY(fit_slot(s, [&](float *w, int32_t *iters, int32_t *evals, float *final_loss) {
            return fb_fit2_host_dev(fbs[s], w, reg_norm_lambda[s], reg_query_lambda[s], max_iter[s], lr[s], iters, evals,
                                    final_loss);
        }));
    }
    return SSW_OK;
}

ssw_status ssw_fb_reset(ssw_fb *fb) {
    SSW_REQUIRE(fb != nullptr, "NULL argument");
    DeviceGuard guard(fb->device);
    SSW_HIP_TRY(hipStreamSynchronize(fb->stream));
    fb->n = 0;
    fb->has_q = fb->has_xlx = false;
    fb->has_targets2 = false;
    fb->targets_on_device = false;
    fb->y_host.clear();
    fb->sw_host.clear();
    fb->last_iters = fb->last_evals = 0;
    fb->last_fit_on_device = false;
    return SSW_OK;
}

ssw_status ssw_fb_last_fit_on_device(const ssw_fb *fb, int32_t *out) {
    SSW_REQUIRE(fb && out, "NULL argument");
    *out = fb->last_fit_on_device ? 1 : 0;
    return SSW_OK;
}

// The pairwise losses evaluated directly on given scores: the kernel the fit uses (k_fb_pairwise, feedback_eval.hip),
// without a data matrix in front of it.  The reference's functions normalise nothing (rank_loss.py:34-95); RegModule
// divides column j by max_inversions_j and multiplies by sample_weight_j (multi_reg.py:106-121):
// coef_j is that per-item factor times max_inversions_j, i.e. coef = max_inversions reproduces the raw column
// sums / gradient of rank_loss.py and coef = sample_weight what RegModule optimises.
ssw_status ssw_rank_pairwise(int32_t device, int32_t logistic, const float *target_host, const float *scores_host,
                             const float *coef_host_or_null, int32_t n, float margin, double *out_item_loss,
                             float *out_grad) {
    SSW_REQUIRE(n >= 0 && n <= FB_MAX_PAIRWISE, "rank_pairwise: n = %d outside [0, %d]", n, FB_MAX_PAIRWISE);
    if (n == 0) return SSW_OK;
    SSW_REQUIRE(target_host && scores_host && out_item_loss && out_grad, "NULL argument");
    DeviceGuard guard(device);
    float *buf = nullptr;  // z | y | coef | r   then f64 item losses
    double *item = nullptr;
    SSW_HIP_TRY(hipMalloc((void **)&buf, (size_t)4 * n * sizeof(float)));
    if (hipMalloc((void **)&item, (size_t)n * sizeof(double)) != hipSuccess) {
        (void)hipFree(buf);
        set_error("rank_pairwise: out of device memory");
        return SSW_ERR_HIP;
    }
    std::vector<float> ones;
    if (!coef_host_or_null) ones.assign((size_t)n, 1.f);
    ssw_status st = SSW_OK;
    auto run = [&]() -> ssw_status {
        SSW_HIP_TRY(hipMemcpy(buf, scores_host, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
        SSW_HIP_TRY(hipMemcpy(buf + n, target_host, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
        SSW_HIP_TRY(hipMemcpy(buf + 2 * n, coef_host_or_null ? coef_host_or_null : ones.data(), (size_t)n * sizeof(float),
                              hipMemcpyHostToDevice));
        launch_fb_pairwise(logistic, buf, buf + n, buf + 2 * n, margin, n, item, buf + 3 * n, 0);
        SSW_HIP_TRY(hipGetLastError());
        SSW_HIP_TRY(hipMemcpy(out_grad, buf + 3 * n, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
        SSW_HIP_TRY(hipMemcpy(out_item_loss, item, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
        return SSW_OK;
    };
    st = run();
    (void)hipFree(buf);
    (void)hipFree(item);
    return st;
}

}  // extern "C"

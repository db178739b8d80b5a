// fb_math.h -- the arithmetic the feedback engine's two fit drivers share.
//
// THE CONTRACT.  The one-launch fit (k_fb_fit_wg / k_fb_fit_wg_batch, feedback_fit_wg.hip) and the host-driven fit
// (the per-evaluation kernels of feedback_eval.hip under the L-BFGS of feedback_lbfgs.hip) return bit-identical fits
// (tests/test_feedback_gpu.py, tools/fuzz_fit_drivers.py).  They do because every value both of them form comes from
// ONE body, and those bodies are this file:
//   label terms      softplus_neg, sigmoidd, bce_item, bce_lw, bce_dz; fb_pairwise_body
//                    (k_fb_elem, k_fb_logits_arg, k_fb_pairwise  |  fit_eval_labels, fit_eval_onepass)
//   slab sums        slab_column_sum                (k_fb_final, k_fb2_reduce; fit_eval_grad adds in the same order)
//   wave reductions  wave_sum_d / wave_sum_f / wave_max_d on the device and wave_sum_host, which restates their
//                    network for the host's dot products (vdot of feedback_lbfgs.hip  |  fit_driver_step)
//   last step        FbFinalLds + fb_final_body     (k_fb_final  |  fit_eval_final)
//   line search      cubic_interpolate_dev          (strong_wolfe  |  fit_driver_step)
//   two outputs      fb2_row_terms, fb2_item_tree, fb2_norm_body, fb2_tail_body + Fb2Lds
//                    (k_fb2_logits_elem, k_fb2_reduce, k_fb2_norm, k_fb2_final_dev  |  fit2_eval_*)
// and the plain data those take (FbW, FbObjDev, the slab and argument-segment sizes).  A change here changes both
// drivers at once; an expression of this kind written a second time somewhere else breaks the contract.  Every
// translation unit that includes this file is compiled with -ffp-contract=off (Makefile, NOCONTRACT): the host and the
// device must round alike, and the expressions that are meant to be fused say fmaf.
//
// Only __device__ __forceinline__, __host__ __device__ inline, constexpr and plain structs: no kernel and no
// out-of-line device function, so each including source inlines its own copy and nothing links across code objects.
#pragma once
#include <cmath>

#include "ssw_common.h"

#pragma GCC visibility push(hidden)  // shared between the library's own sources, not exported from it
namespace ssw {

constexpr int FB_SLAB = 32;          // rows per fb_grad workgroup
constexpr int FB_MAX_PAIRWISE = 4096;  // items the one-workgroup pairwise kernel takes

// Parameters of one closure evaluation, passed BY VALUE in the kernel-argument segment: the driver
// changes them every evaluation, and a separate 2-KB host-to-device copy per evaluation costs more
// than the kernels it feeds.  (dim <= 768; larger dims take the device buffer.)
constexpr int FB_ARG_FLOATS = 772;
struct FbW {
    float v[FB_ARG_FLOATS];
};

struct FbObjDev {
    int kind;          // 0 logreg, 1 multireg
    int has_bias;
    int reg_kind;      // logreg: 0 none, 1 vector, 2 norm (target 0), 3 norm1 (target 1)
    float scale;       // multiplies the data loss and its gradient (1/n for logreg, 1 for multireg)
    float reg_weight;  // logreg: lambda / n
    float l_norm, l_data, l_query;  // multireg
    int exact;         // diagnostic (env SSW_FB_EXACT_LOSS): exact f64 loss values instead of torch's mixed f32/f64 rounding
};

// The reference's label losses are evaluated in f64 (its targets are float64, so torch
// promotes: logistic_regression.py:393, multi_reg.py:170) while logits and gradients stay
// f32.  L-BFGS stops on |loss - prev_loss| < 1e-9, which an f32 loss cannot resolve, so the
// per-item losses are f64 here too; dL/dz is rounded to f32 like torch's.
__device__ __forceinline__ double softplus_neg(double z) {  // log(1 + exp(-z)), stable
    return log1p(exp(-fabs(z))) + fmax(-z, 0.0);
}
__device__ __forceinline__ double sigmoidd(double z) { return 1.0 / (1.0 + exp(-z)); }
// One BCE-with-logits item the way torch forms it with f32 logits and f64 targets
// (binary_cross_entropy_with_logits: log_sigmoid(input) is an f32 tensor, multiplied IN PLACE by the f64
// log_weight -- so the product is rounded to f32 again -- and only then subtracted from the f64
// (1 - target) * input).  The values differ from the exact ones by ~1e-8 per item; L-BFGS's last line search
// and its |loss - prev_loss| < 1e-9 stop sit on exactly that noise, so the rounding is reproduced here.
__device__ __forceinline__ double bce_item(double z, double y, double lw, bool exact) {
    if (exact) return (1.0 - y) * z + lw * softplus_neg(z);  // diagnostic mode (SSW_FB_EXACT_LOSS)
    const float log_sig = (float)(-softplus_neg(z));
    const float weighted = (float)((double)log_sig * lw);
    return (1.0 - y) * z - (double)weighted;
}

__device__ __forceinline__ double bce_lw(float pw, double y) { return 1.0 + ((double)pw - 1.0) * y; }  // the item's log-weight
// d loss / d logit of one BCE item, rounded to f32 like torch's (one body for every site that forms it)
__device__ __forceinline__ float bce_dz(double z, double y, double c, double lw) {
    return (float)(c * ((1.0 - y) - lw * sigmoidd(-z)));
}

// pairwise losses over all ordered pairs (i, j), t_ij = sign(y_i - y_j), s_ij = z_i - z_j:
//   hinge    : max(0, m - t_ij s_ij) - m [t_ij == 0]        (rank_loss.py:63-95)
//   logistic : t_ij^2 log(1 + exp(-t_ij s_ij))              (rank_loss.py:34-61)
// item_j = coef_j / max_inv_j * sum_i loss_ij, max_inv_j = #{i : t_ij != 0};
// r_k = d(sum_j item_j)/dz_k.  One workgroup; z, y, c = coef/max_inv in LDS.
template <int LOGISTIC>
__device__ __forceinline__ void fb_pairwise_body(const float *__restrict__ z, const float *__restrict__ y,
                                                 const float *__restrict__ coef, float margin, int n,
                                                 double *__restrict__ item_loss, float *__restrict__ r,
                                                 float *sh /* LDS, 3 n floats */) {
    float *sz = sh, *sy = sh + n, *sc = sh + 2 * n;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        sz[i] = z[i];
        sy[i] = y[i];
    }
    __syncthreads();
    for (int j = threadIdx.x; j < n; j += blockDim.x) {
        int cnt = 0;
        const float yj = sy[j];
        for (int i = 0; i < n; ++i) cnt += (sy[i] != yj);
        sc[j] = cnt > 0 ? coef[j] / (float)cnt : 0.f;
    }
    __syncthreads();
    for (int k = threadIdx.x; k < n; k += blockDim.x) {
        const float zk = sz[k], yk = sy[k], ck = sc[k];
        double loss_k = 0.0;  // column sum over i of loss_ik
        double rk = 0.0;
        for (int i = 0; i < n; ++i) {
            const float d = sy[i] - yk;
            if (d == 0.f) continue;
            const double t = d > 0.f ? 1.0 : -1.0;  // t_ik
            const double s = (double)(sz[i] - zk);  // s_ik (f32 difference, as torch forms it)
            // pair (i, k): contributes to item_k (column k) with weight ck; z_k enters with -1
            // pair (k, i): t_ki = -t, s_ki = -s, contributes to item_i with weight sc[i]; z_k enters with +1
            if (LOGISTIC) {
                const double u = -t * s;  // -t_ik s_ik  (== -t_ki s_ki)
                loss_k += log(1.0 + exp(u));  // the reference's unguarded form (rank_loss.py:48)
                const double sg = sigmoidd(u);  // d/du log(1+exp(u))
                // d loss_ik / d z_k = sg * (-t) * (-1) = t sg ;  d loss_ki / d z_k = sg * (t)(+1)... see below
                rk += ck * (t * sg) + sc[i] * (t * sg);
            } else {
                const double h = (double)margin - t * s;
                if (h >= 0.0) {  // torch's clamp(min=0) passes the gradient at the kink
                    loss_k += h;
                    // loss_ik = m - t (z_i - z_k): d/dz_k = +t ; loss_ki = m - (-t)(z_k - z_i) = m + t z_k - t z_i: d/dz_k = +t
                    rk += ck * t + sc[i] * t;
                }
            }
        }
        item_loss[k] = (double)ck * loss_k;
        r[k] = (float)rk;
    }
}

// sum of a column over the slab partials, in slab order, with the loads of 32 slabs in flight at a time: the plain
// loop issued them a few at a time (322 slabs at 10 000 rows = ~80 trips to L2, 80 of the 113 us a closure evaluation
// cost there); the additions and their order are unchanged
__device__ __forceinline__ float slab_column_sum(const float *__restrict__ col, int nslabs, int dim) {
    float g = 0.f;
    for (int s0 = 0; s0 < nslabs; s0 += 32) {
        float v[32];
#pragma unroll
        for (int u = 0; u < 32; ++u) v[u] = col[(int64_t)min(s0 + u, nslabs - 1) * dim];
#pragma unroll
        for (int u = 0; u < 32; ++u)
            if (s0 + u < nslabs) g += v[u];
    }
    return g;
}

// ---- reductions inside one full wave: row_shr 1, 2, 4, 8 (lane l takes lane l - s of its 16-lane row, rows'
// first s lanes take 0), the four row totals (lanes 15, 31, 47, 63) added in ascending order
template <int CTRL>
__device__ __forceinline__ double dpp_take_d(double v) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xf, 0xf, false);
    hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double readlane_d(double v, int l) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), l), hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double wave_sum_d(double v) {
    v += dpp_take_d<0x111>(v);
    v += dpp_take_d<0x112>(v);
    v += dpp_take_d<0x114>(v);
    v += dpp_take_d<0x118>(v);
    return ((readlane_d(v, 15) + readlane_d(v, 31)) + readlane_d(v, 47)) + readlane_d(v, 63);
}
template <int CTRL>
__device__ __forceinline__ float dpp_take_f(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false));
}
__device__ __forceinline__ float wave_sum_f(float v) {  // the same network in f32
    v += dpp_take_f<0x111>(v);
    v += dpp_take_f<0x112>(v);
    v += dpp_take_f<0x114>(v);
    v += dpp_take_f<0x118>(v);
    const float r0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 15));
    const float r1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 31));
    const float r2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 47));
    const float r3 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
    return ((r0 + r1) + r2) + r3;
}
__device__ __forceinline__ double wave_max_d(double v) {  // v >= 0
    v = fmax(v, dpp_take_d<0x111>(v));
    v = fmax(v, dpp_take_d<0x112>(v));
    v = fmax(v, dpp_take_d<0x114>(v));
    v = fmax(v, dpp_take_d<0x118>(v));
    return fmax(fmax(readlane_d(v, 15), readlane_d(v, 31)), fmax(readlane_d(v, 47), readlane_d(v, 63)));
}
// The host twin of wave_sum_d (T = double) and wave_sum_f (T = float): sums in the association k_fb_fit_wg's driving
// wave uses (element i in lane i % 64, each lane adding its elements in ascending order; then inside every 16-lane
// row lane l takes lane l - s for s = 1, 2, 4, 8; then the four row totals in ascending order), so that the
// host-driven and the single-launch fit agree bit for bit.  (torch's own dot is a BLAS call with an unspecified order.)
template <class T>
inline T wave_sum_host(const T *p, size_t n) {
    T b[64], nb[64];
    for (size_t l = 0; l < 64; ++l) {
        T s = 0;
        for (size_t i = l; i < n; i += 64) s += p[i];
        b[l] = s;
    }
    for (size_t s = 1; s <= 8; s <<= 1) {
        for (size_t l = 0; l < 64; ++l) nb[l] = b[l] + ((l & 15) >= s ? b[l - s] : T(0));
        for (size_t l = 0; l < 64; ++l) b[l] = nb[l];
    }
    return ((b[15] + b[31]) + b[47]) + b[63];
}

struct FbFinalLds {
    double *red;   // [64]  wave partials of the four-way sum
    double *red2;  // [16]  wave partials of the single sums
    float *sw_;    // [1024] parameters
};

// the body of the last evaluation step, shared by k_fb_final (one launch per evaluation, host-driven fit) and
// k_fb_fit_wg (whole fit in one launch): `g` = this column's data gradient summed over the slabs in slab order,
// `wc` = this column's parameter.  `out` / `out_loss` may point to LDS.
__device__ __forceinline__ void fb_final_body(float g, const float wc, const double *__restrict__ item_loss,
                                              const float *__restrict__ r, int64_t n, int dim,
                                              const float *__restrict__ qhat, const float *__restrict__ xlx,
                                              const FbObjDev &obj, float *out, double *out_loss, const FbFinalLds &L) {
    double *red = L.red, *red2 = L.red2;
    float *sw_ = L.sw_;
    const int c = threadIdx.x;
    const bool act = c < dim;
    if (act) sw_[c] = wc;
    g *= obj.scale;
    // block reductions: |w|^2, w.qhat, data loss, sum r.  Inside each wave the DPP network of wave_sum_d (no LDS
    // traffic), then the 16 wave totals added in ascending order by every thread; four sums share one barrier.
    // (The first version walked an LDS tree with six barriers and 48 ds_bpermute per sum: 5 of the 6 us this
    // step took.)
    const int lane = c & 63, wave = c >> 6;
    auto block_sum = [&](double v) -> double {
        const double wsum = wave_sum_d(v);
        if (lane == 0) red2[wave] = wsum;
        __syncthreads();
        double o = 0.0;
#pragma unroll
        for (int w = 0; w < 16; ++w) o += red2[w];
        __syncthreads();
        return o;
    };
    // Waves without a column (c >= dim) or without an item have zeros to sum: their wave totals are +0.0 without the DPP
    // network, and only the waves that use a total add the 16 wave totals up (every thread did, for all four: 64 f64
    // additions a thread, four waves deep on every SIMD, ~2000 cycles of this step).  The additions that remain are
    // the same, in the same order.
    const bool has_cols = wave * 64 < dim, has_items = (int64_t)wave * 64 < n || n > 1024;
    double ls = 0.0, rs = 0.0;
    if (n <= 1024) {  // one item a thread at most
        if (c < n) {
            ls += item_loss[c];
            rs += (double)r[c];
        }
    } else {
        for (int64_t i0 = c; i0 < n; i0 += 8 * 1024) {  // eight of this thread's items in flight; same order of additions
            double li[8];
            float ri[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int64_t i = i0 + (int64_t)u * 1024;
                li[u] = item_loss[i < n ? i : c];
                ri[u] = r[i < n ? i : c];
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                if (i0 + (int64_t)u * 1024 < n) {
                    ls += li[u];
                    rs += (double)ri[u];
                }
            }
        }
    }
    double ww, wq, data_loss, rsum;
    {
        const double v0 = act ? (double)wc * wc : 0.0, v1 = act && qhat ? (double)wc * qhat[c] : 0.0;
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
        if (has_cols) {
            s0 = wave_sum_d(v0);
            s1 = wave_sum_d(v1);
        }
        if (has_items) {
            s2 = wave_sum_d(ls);
            s3 = wave_sum_d(rs);
        }
        if (lane == 0) {
            red[4 * wave + 0] = s0;
            red[4 * wave + 1] = s1;
            red[4 * wave + 2] = s2;
            red[4 * wave + 3] = s3;
        }
        __syncthreads();
        double t0 = 1.0, t1 = 0.0, t2 = 0.0, t3 = 0.0;  // a wave without columns uses none of them (ww = 1 keeps its arithmetic finite)
        if (has_cols) {
            t0 = 0.0;
#pragma unroll
            for (int w = 0; w < 16; ++w) {
                t0 += red[4 * w + 0];
                t1 += red[4 * w + 1];
            }
        }
        if (wave == 0) {
#pragma unroll
            for (int w = 0; w < 16; ++w) {
                t2 += red[4 * w + 2];
                t3 += red[4 * w + 3];
            }
        }
        ww = t0;
        wq = t1;
        data_loss = t2 * obj.scale;
        rsum = t3 * obj.scale;
    }
    const double norm = sqrt(ww);
    const double nclamp = norm > 1e-12 ? norm : 1e-12;  // F.normalize eps
    // From here on the scalar terms of the loss are formed by thread 0 only and waves that own no column leave
    // once the last barrier is behind them: with all 16 waves walking the whole body its ~800 instructions, four
    // waves deep on every SIMD, were most of this step's time.
    float greg = 0.f;
    if (obj.kind == 0) {
        double d2 = 0.0;
        if (obj.reg_kind == 1) {
            // (|w| - 1)^2 + |w^ - q^|^2 ; |w^ - q^|^2 = w^.w^ - 2 w^.q^ + q^.q^  (q^ unit)
            const double what_c = wc / nclamp;
            d2 = block_sum(act ? (what_c - qhat[c]) * (what_c - qhat[c]) : 0.0);
        }
        if (wave != 0 && wave * 64 >= dim) return;
        double reg_loss = 0.0;
        if (obj.reg_kind == 1) {
            const double what_c = wc / nclamp;
            const double whq = wq / nclamp;
            reg_loss = (norm - 1.0) * (norm - 1.0) + d2;
            if (act) {
                const double diff = what_c - qhat[c];
                // J'(diff), J = (I - w^ w^')/|w| ; w^.diff = w^.w^ - w^.q^
                const double wd = ww / (nclamp * nclamp) - whq;
                greg = (float)(2.0 * (norm - 1.0) * (wc / nclamp) + 2.0 / nclamp * (diff - what_c * wd));
            }
        } else if (obj.reg_kind == 2 || obj.reg_kind == 3) {
            const double target = obj.reg_kind == 3 ? 1.0 : 0.0;
            reg_loss = (norm - target) * (norm - target);
            if (act) greg = (float)(2.0 * (norm - target) * (wc / nclamp));
        }
        reg_loss *= obj.reg_weight;
        greg *= obj.reg_weight;
        if (act) out[1 + c] = g + greg;
        if (c == 0) {
            out[0] = (float)(data_loss + reg_loss);
            *out_loss = data_loss + reg_loss;
            out[1 + dim] = obj.has_bias ? (float)rsum : 0.f;
            float *parts = out + 1 + dim + 1;
            parts[0] = 0.f;
            parts[1] = 0.f;
            parts[2] = 0.f;
            parts[3] = (float)data_loss;
        }
    } else {
        // data: l w'Mw ; d/dw = l (M + M') w
        double mw = 0.0, mtw = 0.0, p_data = 0.0;
        if (obj.l_data != 0.f) {
            if (act && xlx) {
                for (int k = 0; k < dim; ++k) {
                    mw += (double)xlx[(int64_t)c * dim + k] * sw_[k];
                    mtw += (double)xlx[(int64_t)k * dim + c] * sw_[k];
                }
            }
            p_data = obj.l_data * block_sum(act ? (double)wc * mw : 0.0);
        }
        if (wave != 0 && wave * 64 >= dim) return;
        // query: l (1 - w^.q^)/2 ; d/dw = -l/2 (q^ - (w^.q^) w^)/|w|
        const double whq = wq / nclamp;
        if (act) {
            const double what_c = wc / nclamp;
            // norm: l (cosh(log s) - 1), s = w.w ; d/dw = l (1 - 1/s^2) w
            greg = (float)(obj.l_norm * (1.0 - 1.0 / (ww * ww)) * wc + obj.l_data * (mw + mtw) -
                           obj.l_query * 0.5 * ((qhat ? qhat[c] : 0.f) - whq * what_c) / nclamp);
            out[1 + c] = g + greg;
        }
        if (c == 0) {
            // The three regulariser VALUES are rounded the way the reference's f32 tensors round them
            // (multi_reg.py:125-129): the label loss is f64 there (float64 targets promote) but these terms are
            // f32, and cosh(log s) - 1 near s = 1 moves in steps of 2^-23 -- times l_norm = 100 that is a 1.2e-5
            // staircase in the total loss.  torch's L-BFGS stops / accepts line-search points on that staircase
            // (|loss - prev_loss| < 1e-9, Armijo), so an exact f64 value here walks a different path and ends up to
            // 7e-4 (rank scores) away from the reference's fit -- measured on tests/golden/multireg.npz c4.
            // Gradients stay analytic (autograd's f32 sinh(log s)/s * 2w equals l (1 - 1/s^2) w to rounding).
            const double p_norm = obj.exact ? obj.l_norm * (0.5 * (ww + 1.0 / ww) - 1.0)
                                            : (double)(obj.l_norm * (coshf(logf((float)ww)) - 1.f));
            if (!obj.exact) p_data = (double)(float)p_data;
            const double p_query =
                obj.exact ? obj.l_query * (1.0 - whq) * 0.5 : (double)(obj.l_query * ((1.f - (float)whq) / 2.f));
            const double reg_loss = p_norm + p_data + p_query;
            out[0] = (float)(data_loss + reg_loss);
            *out_loss = data_loss + reg_loss;
            out[1 + dim] = obj.has_bias ? (float)rsum : 0.f;
            float *parts = out + 1 + dim + 1;
            parts[0] = (float)p_norm;
            parts[1] = (float)p_data;
            parts[2] = (float)p_query;
            parts[3] = (float)data_loss;
        }
    }
}

// ---- the two-output objective, one closure evaluation of MultiRegModule._step entirely on the device
// (seesaw/loops/multi_reg_module.py:64-128).  Two drivers take it: the host-driven device evaluation (k_fb2_norm,
// k_fb2_logits_elem, k_fb_grad, k_fb2_final_dev of feedback_eval.hip) and the one-launch fit (k_fb_fit2_wg,
// feedback_fit_wg.hip).  The data part is fb2_row_terms per row, k_fb_grad's slab chains and fb2_item_tree; the
// O(dim) part is fb2_norm_body before the logits and fb2_tail_body after the gradient.  The O(dim) part keeps the
// operation order of fb_eval2's host tail (sums over k sequential in f32, the total ((labels + loss_norm) + lq0) + lq1),
// so it differs from ssw_fb_fit2 only where the device library's logf / coshf / sinhf differ from the host's.
struct Fb2Lds {     // all in LDS
    float *W;       // [2 dim] the raw weights of this evaluation
    float *nw;      // [2 dim] rows of W over max(|row|, 1e-12)  (F.normalize)
    float *g;       // [2 dim] d labels / d nw: the slab sums of both gradient planes
    float *qh;      // [dim]   unit query
    float *sc;      // [8]     |W_0|, |W_1|, nw_0.q, nw_1.q, nw_0.G_0, nw_1.G_1
    float *rv, *rh; // [1024]  fb2_item_tree's scratch
};

// One row's label terms from its two logits (a: target, b: confusion class), all f32 as in the reference: the
// vertical BCE pair, the horizontal CE where the row carries a label, d loss / d logit, times the sample weight
__device__ __forceinline__ void fb2_row_terms(float a, float b, float y0, float y1, float s, float *r0, float *r1,
                                              float *item_v, float *item_h) {
    // binary_cross_entropy_with_logits: (1 - y) z - log_sigmoid(z), log_sigmoid(z) = min(z, 0) - log1p(exp(-|z|))
    const float ls0 = fminf(a, 0.f) - log1pf(expf(-fabsf(a))), ls1 = fminf(b, 0.f) - log1pf(expf(-fabsf(b)));
    const float vert = ((1.f - y0) * a - ls0) + ((1.f - y1) * b - ls1);
    const float sg0 = 1.f / (1.f + expf(-a)), sg1 = 1.f / (1.f + expf(-b));
    float g0 = sg0 - y0, g1 = sg1 - y1, hor = 0.f;
    const float near = y0 + y1;
    if (near > 0.f) {  // cross_entropy with probability targets on the rows that carry any label
        const float m = fmaxf(a, b);
        const float lse = m + logf(expf(a - m) + expf(b - m));
        hor = -(y0 * (a - lse) + y1 * (b - lse));
        g0 += near * expf(a - lse) - y0;
        g1 += near * expf(b - lse) - y1;
    }
    *r0 = s * g0;
    *r1 = s * g1;
    *item_v = s * vert;
    *item_h = s * hor;
}

// sums of the per-row vertical / horizontal losses: thread t brings its own rows' sums (rows t, t + 1024, ...), a
// 1024-wide LDS tree adds them.  Afterwards rv[0] / rh[0] hold the totals (a barrier has passed).
__device__ __forceinline__ void fb2_item_tree(float v, float h, float *rv, float *rh) {
    const int t = threadIdx.x;
    rv[t] = v;
    rh[t] = h;
    __syncthreads();
    for (int off = 512; off >= 1; off >>= 1) {
        if (t < off) {
            rv[t] += rv[t + off];
            rh[t] += rh[t + off];
        }
        __syncthreads();
    }
}

// sum of dim terms in k order, f32: term4(j) returns terms 4 j .. 4 j + 3.  The terms of 32 k are formed (their LDS loads
// in flight together) before the sequential additions take them, instead of an LDS round trip per element; measured
// 4 % of a one-launch fit at 390 rows (2.26 -> 2.16 ms).  The additions and their order are the plain loop's.
template <class Term4>
__device__ __forceinline__ float fb2_seq_sum(int dim, Term4 term4) {
    const int q = dim / 4;
    float s = 0.f;
    for (int j0 = 0; j0 < q; j0 += 8) {
        float4 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = term4(min(j0 + u, q - 1));
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (j0 + u < q) {
                s += v[u].x;
                s += v[u].y;
                s += v[u].z;
                s += v[u].w;
            }
    }
    return s;
}
__device__ __forceinline__ float4 fb2_ld4(const float *p, int j) { return reinterpret_cast<const float4 *>(p)[j]; }

// row norms and normalised rows of L.W into L.sc[0..1] / L.nw.  One thread per row walks the sum of squares in k
// order (thread 0 and thread 64: two waves, side by side).  Ends behind a barrier only for the thread's own nw[t].
// (Every Fb2Lds array is 16-byte aligned and dim is a multiple of 4.)
__device__ __forceinline__ void fb2_norm_body(const Fb2Lds &L, int dim) {
    const int t = threadIdx.x;
    if (t == 0 || t == 64) {
        const int c = t >> 6;
        const float *w = L.W + c * dim;
        const float ss = fb2_seq_sum(dim, [&](int j) {
            const float4 a = fb2_ld4(w, j);
            return make_float4(a.x * a.x, a.y * a.y, a.z * a.z, a.w * a.w);
        });
        L.sc[c] = sqrtf(ss);
    }
    __syncthreads();
    if (t < 2 * dim) L.nw[t] = L.W[t] / fmaxf(L.sc[t / dim], 1e-12f);  // F.normalize's eps
}

// The regularisers and the chain rule through the normalisation, from L.nw, L.sc[0..1], L.g, L.qh and the label
// sums: out[0] = (float) total, out[1 .. 1 + 2 dim) = d total / d W, *out_loss = total; parts5 (or null) =
// loss_norm, loss_queryreg, loss_queryreg2, vertical, horizontal.  The values are formed as f32 the way the
// reference's tensors are (see the comment on the one-output regularisers in fb_final_body).  L.nw / L.g / L.sc[0..1]
// must be visible to the workgroup on entry.
__device__ __forceinline__ void fb2_tail_body(const Fb2Lds &L, int dim, float l_norm, float l_query, float vsum,
                                              float hsum, float *out, double *out_loss, float *parts5) {
    const int t = threadIdx.x;
    if (t < 256 && (t & 63) == 0) {  // four sequential sums over k, a wave each
        const int c = (t >> 6) & 1;
        const float *nw = L.nw + c * dim, *g = L.g + c * dim;
        const float hq = 0.5f * l_query;
        float s;
        if (t < 128) {
            s = fb2_seq_sum(dim, [&](int j) {
                const float4 a = fb2_ld4(nw, j), b = fb2_ld4(L.qh, j);
                return make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w);
            });
        } else {
            s = fb2_seq_sum(dim, [&](int j) {
                const float4 a = fb2_ld4(nw, j), b = fb2_ld4(L.qh, j), c4 = fb2_ld4(g, j);
                return make_float4(a.x * (c4.x - hq * b.x), a.y * (c4.y - hq * b.y), a.z * (c4.z - hq * b.z),
                                   a.w * (c4.w - hq * b.w));
            });
        }
        L.sc[2 + (t >> 6)] = s;
    }
    __syncthreads();
    if (t < 2 * dim) {
        // G = d total / d nw_c ; d nw / d W = (I - nw nw') / |W|
        const int c = t / dim, k = t - c * dim;
        const float nrm = L.sc[c], dotg = L.sc[4 + c];
        const float lg = logf(nrm);
        const float den = fmaxf(nrm, 1e-12f);
        const float radial = l_norm * sinhf(lg) / den;  // d [l_norm (cosh(log |W|) - 1)] / d|W|, times d|W|/dW = nw
        const float G = L.g[t] - 0.5f * l_query * L.qh[k];
        out[1 + t] = (G - L.nw[t] * dotg) / den + radial * L.nw[t];
    }
    if (t == 0) {
        float loss_norm = 0.f, lq[2];
        for (int c = 0; c < 2; ++c) {
            loss_norm += coshf(logf(L.sc[c])) - 1.f;
            lq[c] = l_query * ((1.f - L.sc[2 + c]) / 2.f);
        }
        loss_norm *= l_norm;
        const float labels = vsum + hsum;
        const float total = ((labels + loss_norm) + lq[0]) + lq[1];
        out[0] = total;
        *out_loss = (double)total;
        if (parts5) {
            parts5[0] = loss_norm; parts5[1] = lq[0]; parts5[2] = lq[1]; parts5[3] = vsum; parts5[4] = hsum;
        }
    }
}

// minFunc's polyinterp restricted to two points with derivatives (torch.optim.lbfgs._cubic_interpolate)
__host__ __device__ inline double cubic_interpolate_dev(double x1, double f1, double g1, double x2, double f2, double g2,
                                                        bool has_bounds, double lo, double hi) {
    double xmin = lo, xmax = hi;
    if (!has_bounds) {
        xmin = x1 <= x2 ? x1 : x2;
        xmax = x1 <= x2 ? x2 : x1;
    }
    const double d1 = g1 + g2 - 3.0 * (f1 - f2) / (x1 - x2);
    const double d2sq = d1 * d1 - g1 * g2;
    if (d2sq >= 0) {
        const double d2 = sqrt(d2sq);
        double mp;
        if (x1 <= x2)
            mp = x2 - (x2 - x1) * ((g2 + d2 - d1) / (g2 - g1 + 2 * d2));
        else
            mp = x1 - (x1 - x2) * ((g1 + d2 - d1) / (g1 - g2 + 2 * d2));
        return fmin(fmax(mp, xmin), xmax);
    }
    return (xmin + xmax) / 2.0;
}

}  // namespace ssw
#pragma GCC visibility pop

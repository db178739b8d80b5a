// feedback_eval.hip -- the feedback engine's data preparation and one closure evaluation at a time: the kernels the
// host-driven fit (feedback_lbfgs.hip), ssw_fb_lossgrad / ssw_fb_lossgrad2 and ssw_fb_scores launch, the device buffers
// behind them and the objective's set-up (gfx950 / MI355X).  The engine's overview is in feedback.hip; the label terms,
// the slab sums and the last step's body are fb_math.h's, shared with the one-launch fit.  Compiled with
// -ffp-contract=off (Makefile).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <vector>

#include "fb_handle.h"

namespace ssw {
namespace {

// ---- data preparation ---------------------------------------------------------------
// column means in f64 (fixed order), then subtract: StandardScaler(with_std=False) /
// `X - X.mean(axis=0)` (logistic_regression.py:353-355, multi_reg.py:168-169).  Three small launches: per-column sums
// of 256-row blocks, the block sums added in block order, the subtraction over all elements.  (One thread walking a
// whole column took 3.7 ms on PseudoLR's 10 000 rows.)
constexpr int FB_CENTER_ROWS = 256;
__global__ void k_fb_colsum_blocks(const float *__restrict__ X, int64_t n, int dim, double *__restrict__ partial) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= dim) return;
    const int64_t r0 = (int64_t)blockIdx.y * FB_CENTER_ROWS, r1 = min(r0 + FB_CENTER_ROWS, n);
    double s = 0.0;
    for (int64_t i0 = r0; i0 < r1; i0 += 32) {  // 32 rows in flight; the additions stay in row order
        float v[32];
#pragma unroll
        for (int u = 0; u < 32; ++u) v[u] = X[min(i0 + u, r1 - 1) * dim + c];
#pragma unroll
        for (int u = 0; u < 32; ++u)
            if (i0 + u < r1) s += (double)v[u];
    }
    partial[(int64_t)blockIdx.y * dim + c] = s;
}
__global__ void k_fb_colmean(const double *__restrict__ partial, int nblk, int64_t n, int dim, float *__restrict__ mu) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= dim) return;
    double s = 0.0;
    for (int b = 0; b < nblk; ++b) s += partial[(int64_t)b * dim + c];
    mu[c] = (float)(s / (double)n);
}
__global__ void k_fb_subtract_mean(float *__restrict__ X, int64_t n, int dim, const float *__restrict__ mu) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= dim) return;
    const float m = mu[c];
    const int64_t r0 = (int64_t)blockIdx.y * FB_CENTER_ROWS, r1 = min(r0 + FB_CENTER_ROWS, n);
    for (int64_t i0 = r0; i0 < r1; i0 += 32) {
        float v[32];
#pragma unroll
        for (int u = 0; u < 32; ++u) v[u] = X[min(i0 + u, r1 - 1) * dim + c];
#pragma unroll
        for (int u = 0; u < 32; ++u)
            if (i0 + u < r1) X[(i0 + u) * dim + c] = v[u] - m;
    }
}

// PseudoLR's sample on the device (ssw_fb_set_pseudo_sample): thread i takes the p-th unlabelled row for p = drawn[i] --
// p + #{j : th[j] <= p} with th[j] = labelled[j] - j, found by bisection (== np.nonzero(~is_labeled)[0][p]) -- and that row's
// propagated score as its target; rows / y / row ids land behind the n_lab labelled entries
__global__ void k_fb_pseudo_rows(const int64_t *__restrict__ th, int n_lab, const int64_t *__restrict__ drawn, int64_t n_drawn,
                                 const double *__restrict__ scores, int64_t n_scores, int64_t *__restrict__ rows_out,
                                 float *__restrict__ y_out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_drawn) return;
    const int64_t p = drawn[i];
    int lo = 0, hi = n_lab;  // first j with th[j] > p
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (th[mid] <= p) lo = mid + 1;
        else hi = mid;
    }
    int64_t pick = p + lo;
    if (pick >= n_scores) pick = n_scores - 1;  // (the host checked p < #unlabelled: cannot happen)
    rows_out[n_lab + i] = pick;
    y_out[n_lab + i] = (float)scores[pick];
}

// ---- per-evaluation kernels -----------------------------------------------------------
// z_i = <x_i, w> + b ; one wave per row
__global__ __launch_bounds__(256) void k_fb_logits(const float *__restrict__ X,
                                                   const float *__restrict__ w, int64_t n, int dim,
                                                   int has_bias, float *__restrict__ z) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    const float4 *x4 = reinterpret_cast<const float4 *>(X + row * dim);
    const float4 *w4 = reinterpret_cast<const float4 *>(w);
    float a = 0.f;
    for (int c = lane; c < dim / 4; c += 64) {
        const float4 xv = x4[c], wv = w4[c];
        a = fmaf(xv.x, wv.x, a);
        a = fmaf(xv.y, wv.y, a);
        a = fmaf(xv.z, wv.z, a);
        a = fmaf(xv.w, wv.w, a);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) a += __shfl_xor(a, off, 64);
    if (lane == 0) z[row] = a + (has_bias ? w[dim] : 0.f);
}

// elementwise BCE-with-logits with pos_weight pw and per-item coefficient c_i:
//   l = c [ (1-y) z + (1 + (pw-1) y) softplus(-z) ],  dl/dz = c [ (1-y) - (1 + (pw-1) y) sigmoid(-z) ]
__global__ void k_fb_elem(const float *__restrict__ z, const float *__restrict__ y,
                          const float *__restrict__ coef, float pw, int64_t n,
                          double *__restrict__ item_loss, float *__restrict__ r, int exact) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double zi = z[i], yi = y[i], ci = coef[i];
    const double lw = bce_lw(pw, yi);
    item_loss[i] = ci * bce_item(zi, yi, lw, exact != 0);
    r[i] = bce_dz(zi, yi, ci, lw);
}

// k_fb_logits with the parameters in the argument segment and, when `elem` is set, k_fb_elem folded in
// (same expressions, same order: the results are bit-identical to the two-kernel form)
__global__ __launch_bounds__(256) void k_fb_logits_arg(const float *__restrict__ X, FbW wv, int64_t n, int dim,
                                                       int has_bias, float *__restrict__ z, int elem,
                                                       const float *__restrict__ y, const float *__restrict__ coef,
                                                       float pw, double *__restrict__ item_loss,
                                                       float *__restrict__ r) {
    // a wave takes FOUR rows: their loads are in flight together and lanes 0-3 each finish one row's label term (the
    // f64 exp / log1p chain was one lane per wave: a quarter of the waves, the same latency each).  Per row the
    // arithmetic is unchanged: the lane's fma chain over its columns, the xor butterfly 32 ... 1.
    const int lane = threadIdx.x & 63;
    const int64_t row0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 4;
    if (row0 >= n) return;
    const float4 *w4 = reinterpret_cast<const float4 *>(wv.v);
    const float4 *x4[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) x4[u] = reinterpret_cast<const float4 *>(X + (row0 + u < n ? row0 + u : row0) * dim);
    float a[4] = {0.f, 0.f, 0.f, 0.f};
    for (int c = lane; c < dim / 4; c += 64) {
        float4 xv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) xv[u] = x4[u][c];
        const float4 wq = w4[c];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            a[u] = fmaf(xv[u].x, wq.x, a[u]);
            a[u] = fmaf(xv[u].y, wq.y, a[u]);
            a[u] = fmaf(xv[u].z, wq.z, a[u]);
            a[u] = fmaf(xv[u].w, wq.w, a[u]);
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
        for (int u = 0; u < 4; ++u) a[u] += __shfl_xor(a[u], off, 64);
    }
    const float mine = lane == 0 ? a[0] : lane == 1 ? a[1] : lane == 2 ? a[2] : a[3];
    const int64_t row = row0 + lane;
    if (lane < 4 && row < n) {
        const float zf = mine + (has_bias ? wv.v[dim] : 0.f);
        z[row] = zf;
        if (elem) {
            const double zi = zf, yi = y[row], ci = coef[row];
            const double lw = bce_lw(pw, yi);
            item_loss[row] = ci * bce_item(zi, yi, lw, elem == 2);
            r[row] = bce_dz(zi, yi, ci, lw);
        }
    }
}

// fb_pairwise_body (fb_math.h) as one workgroup of its own
template <int LOGISTIC>
__global__ __launch_bounds__(1024) void k_fb_pairwise(const float *__restrict__ z,
                                                      const float *__restrict__ y,
                                                      const float *__restrict__ coef, float margin,
                                                      int n, double *__restrict__ item_loss,
                                                      float *__restrict__ r) {
    extern __shared__ float sh[];
    fb_pairwise_body<LOGISTIC>(z, y, coef, margin, n, item_loss, r, sh);
}

// RankingRegModule (logistic_regression.py:16-65): per-item "loss" |g_i| / total_pairs and the pseudo-gradient
// g_i / total_pairs that _CheapPairwiseRankingLoss.backward hands to autograd (rank_loss.py:164-187), g = the
// quick zero-margin gradient of rank.hip
__global__ void k_fb_rank_items(const float *__restrict__ g, float factor, int64_t n, double *__restrict__ item_loss,
                                float *__restrict__ r) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float v = g[i] * factor;  // f32, as torch forms grads * factor
    item_loss[i] = (double)fabsf(v);
    r[i] = v;
}

// partial gradient of one slab of rows: thread c owns column c
__global__ void k_fb_grad(const float *__restrict__ X, const float *__restrict__ r, int64_t n,
                          int dim, float *__restrict__ partial /* [nslabs, dim] */) {
    const int c = threadIdx.x + blockIdx.y * blockDim.x;
    if (c >= dim) return;
    const int64_t r0 = (int64_t)blockIdx.x * FB_SLAB;
    const int cnt = (int)(min(r0 + FB_SLAB, n) - r0);
    // all of the slab's loads are issued before the (ordered, dependent) fma chain consumes them: the chain
    // itself is 32 steps, waiting for one row at a time made it 32 memory latencies
    float xv[FB_SLAB], rv[FB_SLAB];
#pragma unroll
    for (int i = 0; i < FB_SLAB; ++i) {
        const int64_t row = r0 + (i < cnt ? i : 0);
        xv[i] = X[row * dim + c];
        rv[i] = r[row];
    }
    float g = 0.f;
#pragma unroll
    for (int i = 0; i < FB_SLAB; ++i)
        if (i < cnt) g = fmaf(rv[i], xv[i], g);
    partial[(int64_t)blockIdx.x * dim + c] = g;
}

// ---- two linear outputs: MultiRegModule (seesaw/loops/multi_reg_module.py:40-165), the scorer of the multi_reg_neg
// loop.  Row i has logits z_ic = <x_i, W_c / |W_c|>, c = 0 (target) / 1 (confusion class), f32 targets y_ic and a
// sample weight s_i.  loss_labels = sum_i s_i [ bce(z_i0, y_i0) + bce(z_i1, y_i1) ]          ("vertical")
//                                 + sum_{i : y_i0 + y_i1 > 0} s_i * -(sum_c y_ic log_softmax(z_i)_c)  ("horizontal")
// Everything is f32 in the reference (targets are cast with .astype('float32'), multi_reg_neg.py:73), so it is here.
// z, y, r are stored as two planes of `plane` floats so the single-output gradient kernel serves both outputs.
__global__ __launch_bounds__(256) void k_fb2_logits_elem(const float *__restrict__ X, const float *__restrict__ nw /* [2, dim] */,
                                                         int64_t n, int dim, int64_t plane, const float *__restrict__ y2,
                                                         const float *__restrict__ sw, float *__restrict__ z2,
                                                         float *__restrict__ r2, float *__restrict__ item_v,
                                                         float *__restrict__ item_h) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    const float4 *x4 = reinterpret_cast<const float4 *>(X + row * dim);
    const float4 *w0 = reinterpret_cast<const float4 *>(nw), *w1 = reinterpret_cast<const float4 *>(nw + dim);
    float a = 0.f, b = 0.f;
    for (int c = lane; c < dim / 4; c += 64) {
        const float4 xv = x4[c], p = w0[c], q = w1[c];
        a = fmaf(xv.x, p.x, a); a = fmaf(xv.y, p.y, a); a = fmaf(xv.z, p.z, a); a = fmaf(xv.w, p.w, a);
        b = fmaf(xv.x, q.x, b); b = fmaf(xv.y, q.y, b); b = fmaf(xv.z, q.z, b); b = fmaf(xv.w, q.w, b);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        a += __shfl_xor(a, off, 64);
        b += __shfl_xor(b, off, 64);
    }
    if (lane != 0) return;
    float r0, r1, iv, ih;
    fb2_row_terms(a, b, y2[row], y2[plane + row], sw[row], &r0, &r1, &iv, &ih);
    z2[row] = a;
    z2[plane + row] = b;
    r2[row] = r0;
    r2[plane + row] = r1;
    item_v[row] = iv;
    item_h[row] = ih;
}

// The slab sums (slab_column_sum, fb_math.h) ahead of k_fb_final, over several workgroups, for sets of thousands of
// rows: one workgroup adding 322 slab partials of 512 columns reads 660 KB through one CU (23 us of a 48-us closure
// evaluation at 10 000 rows).  Here a workgroup takes 64 columns; its four thread groups fetch a quarter of a 128-slab
// chunk each into LDS (32 loads in flight per thread), then one thread per column adds the chunk in slab order -- the
// additions k_fb_final's own loop makes, in its order; k_fb_final then finds one "slab" per column.
__global__ __launch_bounds__(256) void k_fb_slabsum(const float *__restrict__ partial, int nslabs, int dim,
                                                    float *__restrict__ gsum) {
    __shared__ float buf[128][64];
    const int t = threadIdx.x, col = t & 63, part = t >> 6;
    const int c = blockIdx.x * 64 + col;
    const int cc = c < dim ? c : dim - 1;
    float g = 0.f;
    for (int s0 = 0; s0 < nslabs; s0 += 128) {
        float v[32];
#pragma unroll
        for (int u = 0; u < 32; ++u) v[u] = partial[(int64_t)min(s0 + part * 32 + u, nslabs - 1) * dim + cc];
#pragma unroll
        for (int u = 0; u < 32; ++u) buf[part * 32 + u][col] = v[u];
        __syncthreads();
        if (part == 0) {
            const int cnt = min(128, nslabs - s0);
            for (int i = 0; i < cnt; ++i) g += buf[i][col];
        }
        __syncthreads();
    }
    if (part == 0 && c < dim) gsum[c] = g;
}

// out[0] = sum item_v, out[1] = sum item_h, out[2 + c*dim + k] = sum over slabs of partial_c[slab][k]; then the flag
__global__ __launch_bounds__(1024) void k_fb2_reduce(const float *__restrict__ partial /* [2][nslabs_cap][dim] */,
                                                     int64_t partial_plane, int nslabs, const float *__restrict__ item_v,
                                                     const float *__restrict__ item_h, int64_t n, int dim,
                                                     float *__restrict__ out, unsigned *__restrict__ done_flag,
                                                     unsigned seqno) {
    __shared__ float rv[1024], rh[1024];
    const int t = threadIdx.x;
    if (t < 2 * dim) {
        const float *pp = partial + (t / dim) * partial_plane + (t % dim);
        float g = 0.f;
        g = slab_column_sum(pp, nslabs, dim);
        out[2 + t] = g;
    }
    float v = 0.f, h = 0.f;
    for (int64_t i = t; i < n; i += 1024) {
        v += item_v[i];
        h += item_h[i];
    }
    fb2_item_tree(v, h, rv, rh);
    if (t == 0) {
        out[0] = rv[0];
        out[1] = rh[0];
    }
    __threadfence_system();
    __syncthreads();
    if (t == 0) __hip_atomic_store(done_flag, seqno, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// ---- the two-output evaluation with its O(dim) part on the device too (fb_eval2_dev): k_fb2_norm in front of
// k_fb2_logits_elem / k_fb_grad, k_fb2_final_dev in place of k_fb2_reduce and fb_eval2's host tail.  The bodies are
// fb_math.h's (fb2_norm_body, fb2_item_tree, fb2_tail_body), the ones k_fb_fit2_wg runs.
// wn [2 dim + 2]: raw weights in, then |W_0|, |W_1| out; nw [2 dim] out
__global__ __launch_bounds__(1024) void k_fb2_norm(float *__restrict__ wn, int dim, float *__restrict__ nw) {
    __shared__ __align__(16) float sW[1024], snw[1024], ssc[8];
    const int t = threadIdx.x;
    if (t < 2 * dim) sW[t] = wn[t];
    __syncthreads();
    const Fb2Lds L{sW, snw, nullptr, nullptr, ssc, nullptr, nullptr};
    fb2_norm_body(L, dim);
    if (t < 2 * dim) nw[t] = snw[t];
    if (t < 2) wn[2 * dim + t] = ssc[t];
}

// out[0] = (float) loss, out[1 .. 1 + 2 dim) = d loss / d W, out[1 + 2 dim ..) = parts5, *out_loss; then the flag
__global__ __launch_bounds__(1024) void k_fb2_final_dev(const float *__restrict__ partial /* [2][nslabs_cap][dim] */,
                                                        int64_t partial_plane, int nslabs, const float *__restrict__ item_v,
                                                        const float *__restrict__ item_h, int64_t n, int dim,
                                                        const float *__restrict__ wn, const float *__restrict__ nw,
                                                        const float *__restrict__ qhat, float l_norm, float l_query,
                                                        float *__restrict__ out, double *__restrict__ out_loss,
                                                        unsigned *__restrict__ done_flag, unsigned seqno) {
    __shared__ __align__(16) float snw[1024], sg[1024], sqh[512], ssc[8], rv[1024], rh[1024];
    const int t = threadIdx.x;
    if (t < 2 * dim) {
        snw[t] = nw[t];
        sg[t] = slab_column_sum(partial + (t / dim) * partial_plane + (t % dim), nslabs, dim);
    }
    if (t < dim) sqh[t] = qhat[t];
    if (t < 2) ssc[t] = wn[2 * dim + t];
    float v = 0.f, h = 0.f;
    for (int64_t i = t; i < n; i += 1024) {
        v += item_v[i];
        h += item_h[i];
    }
    fb2_item_tree(v, h, rv, rh);
    const Fb2Lds L{nullptr, snw, sg, sqh, ssc, rv, rh};  // the tail reads the normalised rows and their norms only
    fb2_tail_body(L, dim, l_norm, l_query, rv[0], rh[0], out, out_loss, out + 1 + 2 * dim);
    __threadfence_system();
    __syncthreads();
    if (t == 0) __hip_atomic_store(done_flag, seqno, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// one workgroup of 1024 threads (column c = thread c, dim <= 1024): reduce partials in slab order, add the
// regulariser terms (fb_final_body, the body fit_eval_final of the one-launch fit runs too), emit out[0] = loss,
// out[1 .. 1+P) = gradient, out[1+P ..] = parts
__global__ __launch_bounds__(1024) void k_fb_final(const float *__restrict__ partial, int nslabs,
                                                   const double *__restrict__ item_loss,
                                                   const float *__restrict__ r, int64_t n, int dim,
                                                   const float *__restrict__ w_or_null, FbW wv,
                                                   const float *__restrict__ qhat,
                                                   const float *__restrict__ xlx, FbObjDev obj,
                                                   float *__restrict__ out, double *__restrict__ out_loss,
                                                   unsigned *__restrict__ done_flag, unsigned seqno) {
    __shared__ double red[64], red2[16];
    __shared__ float sw_[1024];
    const int c = threadIdx.x;
    const bool act = c < dim;
    const float wc = act ? (w_or_null ? w_or_null[c] : wv.v[c < FB_ARG_FLOATS ? c : 0]) : 0.f;
    // data gradient
    float g = 0.f;
    if (act)
        g = slab_column_sum(partial + c, nslabs, dim);
    FbFinalLds L{red, red2, sw_};
    fb_final_body(g, wc, item_loss, r, n, dim, qhat, xlx, obj, out, out_loss, L);
    // completion signal for the host's spin-wait (cheaper than waking up from hipStreamSynchronize, which costs
    // ~10 us per closure evaluation): every thread's result stores are released to the system, then one flag word
    if (done_flag) {
        __threadfence_system();
        __syncthreads();
        if (c == 0) {
            __hip_atomic_store(done_flag, seqno, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

}  // namespace

// ---- launchers of the kernels the C entry points use directly ----------------------------------
void launch_fb_logits(ssw_fb *fb, int has_bias) {
    hipLaunchKernelGGL(k_fb_logits, dim3((unsigned)((fb->n + 3) / 4)), dim3(256), 0, fb->stream, fb->X, fb->w, fb->n,
                       fb->dim, has_bias, fb->z);
}

void launch_fb_pairwise(int logistic, const float *z, const float *y, const float *coef, float margin, int n,
                        double *item_loss, float *r, hipStream_t stream) {
    const size_t lds = (size_t)3 * n * sizeof(float);
    if (logistic)
        hipLaunchKernelGGL(k_fb_pairwise<1>, dim3(1), dim3(1024), lds, stream, z, y, coef, margin, n, item_loss, r);
    else
        hipLaunchKernelGGL(k_fb_pairwise<0>, dim3(1), dim3(1024), lds, stream, z, y, coef, margin, n, item_loss, r);
}

void launch_fb_pseudo_rows(ssw_fb *fb, int64_t n_lab, int64_t n_drawn, const double *dev_scores, int64_t n_scores) {
    hipLaunchKernelGGL(k_fb_pseudo_rows, dim3((unsigned)((n_drawn + 255) / 256)), dim3(256), 0, fb->stream, fb->th, (int)n_lab,
                       fb->drawn, n_drawn, dev_scores, n_scores, fb->rows, fb->y);
}

// ---- device buffers, centring, the objective's set-up -------------------------------------------
ssw_status fb_reserve(ssw_fb *fb, int64_t n) {
    if (n <= fb->cap) return SSW_OK;
    SSW_HIP_TRY(hipStreamSynchronize(fb->stream));
    for (void **p : {(void **)&fb->X, (void **)&fb->y, (void **)&fb->coef, (void **)&fb->z, (void **)&fb->item, (void **)&fb->r,
                     (void **)&fb->rows, (void **)&fb->partial, (void **)&fb->rankg, (void **)&fb->colsum}) {
        (void)hipFree(*p);
        *p = nullptr;
    }
    fb->cap = 0;
    int64_t cap = 256;
    while (cap < n) cap <<= 1;
    const int64_t nslabs = (cap + FB_SLAB - 1) / FB_SLAB;
    SSW_HIP_TRY(hipMalloc((void **)&fb->X, (size_t)cap * fb->dim * sizeof(float)));
    SSW_HIP_TRY(hipMalloc((void **)&fb->y, (size_t)cap * sizeof(float)));
    SSW_HIP_TRY(hipMalloc((void **)&fb->coef, (size_t)cap * sizeof(float)));
    SSW_HIP_TRY(hipMalloc((void **)&fb->z, (size_t)cap * sizeof(float)));
    SSW_HIP_TRY(hipMalloc((void **)&fb->item, (size_t)cap * sizeof(double)));
    SSW_HIP_TRY(hipMalloc((void **)&fb->r, (size_t)cap * sizeof(float)));
    SSW_HIP_TRY(hipMalloc((void **)&fb->rows, (size_t)cap * sizeof(int64_t)));
    SSW_HIP_TRY(hipMalloc((void **)&fb->partial, (size_t)nslabs * fb->dim * sizeof(float)));
    SSW_HIP_TRY(hipMalloc((void **)&fb->rankg, (size_t)cap * sizeof(float)));
    SSW_HIP_TRY(hipMalloc((void **)&fb->colsum, (size_t)((cap + FB_CENTER_ROWS - 1) / FB_CENTER_ROWS) * fb->dim * sizeof(double)));
    fb->cap = cap;
    return SSW_OK;
}

ssw_status fb_center(ssw_fb *fb, int center) {
    if (center && fb->n > 0) {
        const int nblk = (int)((fb->n + FB_CENTER_ROWS - 1) / FB_CENTER_ROWS);
        const dim3 grid((fb->dim + 63) / 64, nblk);
        hipLaunchKernelGGL(k_fb_colsum_blocks, grid, dim3(64), 0, fb->stream, fb->X, fb->n, fb->dim, fb->colsum);
        hipLaunchKernelGGL(k_fb_colmean, dim3((fb->dim + 63) / 64), dim3(64), 0, fb->stream, fb->colsum, nblk, fb->n,
                           fb->dim, fb->mu);
        hipLaunchKernelGGL(k_fb_subtract_mean, grid, dim3(64), 0, fb->stream, fb->X, fb->n, fb->dim, fb->mu);
        SSW_HIP_TRY(hipGetLastError());
    } else {
        SSW_HIP_TRY(hipMemsetAsync(fb->mu, 0, (size_t)fb->dim * sizeof(float), fb->stream));
    }
    return SSW_OK;
}

// effective per-item coefficients + pos_weight + data-loss scale for an objective
ssw_status fb_prepare(ssw_fb *fb, const ssw_fb_objective *o, FbObjDev *dev, float *pw_out, bool *pairwise_active) {
    const int64_t n = fb->n;
    std::vector<float> coef((size_t)n);
    *pairwise_active = false;
    memset(dev, 0, sizeof(*dev));
    dev->kind = o->kind;
    dev->exact = getenv("SSW_FB_EXACT_LOSS") != nullptr;
    if (fb->targets_on_device && o->kind != SSW_FB_LOGREG) {
        set_error("feedback: targets set by ssw_fb_set_pseudo_sample serve the logistic objective only");
        return SSW_ERR_INVALID;
    }
    if (o->kind == SSW_FB_LOGREG) {
        // mean over items of weight_i * bce(.; pos_weight)   (logistic_regression.py:98-105)
        for (int64_t i = 0; i < n; ++i) coef[(size_t)i] = fb->sw_host.empty() ? 1.f : fb->sw_host[(size_t)i];
        *pw_out = o->pos_weight;
        dev->has_bias = o->fit_intercept ? 1 : 0;
        dev->reg_kind = o->reg_kind;
        dev->scale = n > 0 ? 1.f / (float)n : 0.f;
        dev->reg_weight = o->reg_weight;
        if (o->reg_kind == 1 && !fb->has_q) {
            set_error("feedback: vector regulariser needs ssw_fb_set_query first");
            return SSW_ERR_INVALID;
        }
    } else if (o->kind == SSW_FB_MULTIREG) {
        dev->scale = 1.f;
        dev->l_norm = o->reg_norm_lambda;
        dev->l_data = o->reg_data_lambda;
        dev->l_query = o->reg_query_lambda;
        if (!fb->has_q) {
            set_error("feedback: multireg needs ssw_fb_set_query first");
            return SSW_ERR_INVALID;
        }
        if (o->reg_data_lambda != 0.f && !fb->has_xlx) {
            set_error("feedback: reg_data_lambda != 0 needs ssw_fb_set_xlx first");
            return SSW_ERR_INVALID;
        }
        // sample_weight bookkeeping of RegModule._step (multi_reg.py:85-105), in f32 like torch
        float orig_sum = 0.f, pos_total = 0.f;
        for (int64_t i = 0; i < n; ++i) {
            const float s = fb->sw_host.empty() ? 1.f : fb->sw_host[(size_t)i];
            coef[(size_t)i] = s;
            orig_sum += s;
            if (fb->y_host[(size_t)i] == 1.f) pos_total += s;
        }
        const float neg_total = orig_sum - pos_total;
        *pw_out = 1.f;
        if (o->loss_type == SSW_FB_LOSS_CE) {
            const float positive_weight = o->pos_weight < 0.f ? (neg_total + 1.f) / (pos_total + 1.f) : o->pos_weight;
            float new_sum = 0.f;
            for (int64_t i = 0; i < n; ++i) {
                if (fb->y_host[(size_t)i] == 1.f) coef[(size_t)i] *= positive_weight;
                new_sum += coef[(size_t)i];
            }
            const float f = n > 0 ? orig_sum / new_sum : 0.f;
            for (int64_t i = 0; i < n; ++i) coef[(size_t)i] *= f;
        } else {
            *pairwise_active = (pos_total > 0.f && neg_total > 0.f);
            if (n > FB_MAX_PAIRWISE) {
                set_error("feedback: pairwise losses take at most %d items, got %lld", FB_MAX_PAIRWISE, (long long)n);
                return SSW_ERR_UNSUPPORTED;
            }
        }
    } else if (o->kind == SSW_FB_RANKREG) {
        // sum_i |g_i| / total_pairs + (lambda / n) R(w): RankRegressionPT.fit (logistic_regression.py:216-255)
        dev->kind = SSW_FB_LOGREG;  // the regulariser terms are LogisticRegressionPT's
        dev->reg_kind = o->reg_kind;
        dev->scale = 1.f;
        dev->reg_weight = o->reg_weight;
        if (o->reg_kind == 1 && !fb->has_q) {
            set_error("feedback: vector regulariser needs ssw_fb_set_query first");
            return SSW_ERR_INVALID;
        }
        if (n > SSW_RANK_MAX_ITEMS) {
            set_error("feedback: the rank objective takes at most %d items, got %lld", SSW_RANK_MAX_ITEMS, (long long)n);
            return SSW_ERR_UNSUPPORTED;
        }
        // total_pairs = n^2 - sum over distinct targets of (class size)^2 (rank_loss.py:152)
        std::vector<float> ys(fb->y_host.begin(), fb->y_host.begin() + n);
        std::sort(ys.begin(), ys.end());
        double total = (double)n * (double)n;
        for (int64_t i = 0; i < n;) {
            int64_t j = i;
            while (j < n && ys[(size_t)j] == ys[(size_t)i]) ++j;
            total -= (double)(j - i) * (double)(j - i);
            i = j;
        }
        fb->rank_factor = total > 0 ? (float)(1.0 / total) : 0.f;
        *pw_out = 1.f;
        return SSW_OK;  // no per-item coefficients
    } else {
        set_error("feedback: unknown objective kind %d", o->kind);
        return SSW_ERR_INVALID;
    }
    // through pinned staging (coef is a local), without a wait: the evaluations are stream-ordered behind the copy
    if (n > 0) SSW_TRY(fb->coef_stage.push(fb->coef, coef.data(), (size_t)n * sizeof(float), fb->stream));
    return SSW_OK;
}

// one closure evaluation at the parameters in fb->w_host; results land in fb->out_host
ssw_status fb_eval(ssw_fb *fb, const ssw_fb_objective *o, const FbObjDev &dev, float pw, bool pairwise_active, int P) {
    hipStream_t s = fb->stream;
    const int64_t n = fb->n;
    const int dim = fb->dim;
    const bool by_arg = dim + 1 <= FB_ARG_FLOATS;
    FbW wv;
    if (by_arg) {
        memcpy(wv.v, fb->w_host, (size_t)P * sizeof(float));
        for (int i = P; i < FB_ARG_FLOATS; ++i) wv.v[i] = 0.f;
    } else {
        SSW_HIP_TRY(hipMemcpyAsync(fb->w, fb->w_host, (size_t)P * sizeof(float), hipMemcpyHostToDevice, s));
    }
    int nslabs = 0;
    if (n > 0) {
        const bool rankreg = o->kind == SSW_FB_RANKREG;
        const bool pairwise = rankreg || (o->kind == SSW_FB_MULTIREG && o->loss_type != SSW_FB_LOSS_CE);
        nslabs = (int)((n + FB_SLAB - 1) / FB_SLAB);
        if (by_arg)
            hipLaunchKernelGGL(k_fb_logits_arg, dim3((unsigned)((n + 15) / 16)), dim3(256), 0, s, fb->X, wv, n, dim,
                               dev.has_bias, fb->z, pairwise ? 0 : (dev.exact ? 2 : 1), fb->y, fb->coef, pw, fb->item, fb->r);
        else
            launch_fb_logits(fb, dev.has_bias);
        if (!pairwise) {
            if (!by_arg)
                hipLaunchKernelGGL(k_fb_elem, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, fb->z, fb->y, fb->coef,
                                   pw, n, fb->item, fb->r, dev.exact);
        } else if (rankreg) {
            // z is ready: net position changes by counting (rank.hip), then |g| / total_pairs and g / total_pairs
            SSW_TRY(launch_rank_quick(fb->y, fb->z, (int)n, fb->rankg, nullptr, nullptr, s));
            hipLaunchKernelGGL(k_fb_rank_items, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, fb->rankg,
                               fb->rank_factor, n, fb->item, fb->r);
        } else if (pairwise_active) {
            launch_fb_pairwise(o->loss_type == SSW_FB_LOSS_PAIRWISE_LOGISTIC, fb->z, fb->y, fb->coef, o->margin, (int)n,
                               fb->item, fb->r, s);
        } else {  // only one class labelled so far: the label loss is identically 0 (multi_reg.py:107)
            SSW_HIP_TRY(hipMemsetAsync(fb->item, 0, (size_t)n * sizeof(double), s));
            SSW_HIP_TRY(hipMemsetAsync(fb->r, 0, (size_t)n * sizeof(float), s));
        }
        // (folding this into the logits kernel, one 32-row slab per workgroup, was measured: fewer, longer
        // workgroups cost more than the launch they save -- 48 vs 36 us per evaluation)
        const int tx = dim < 256 ? dim : 256;
        hipLaunchKernelGGL(k_fb_grad, dim3((unsigned)nslabs, (unsigned)((dim + tx - 1) / tx)), dim3(tx), 0, s, fb->X,
                           fb->r, n, dim, fb->partial);
    }
    const float *final_partial = fb->partial;
    int final_slabs = nslabs;
    if (nslabs >= 64 && !getenv("SSW_FB_NO_SLABSUM")) {  // thousands of rows: the slab sums on several CUs first (same additions, same order; the variable is the tests' A/B switch)
        if (!fb->gsum) SSW_HIP_TRY(hipMalloc((void **)&fb->gsum, 1024 * sizeof(float)));
        hipLaunchKernelGGL(k_fb_slabsum, dim3((unsigned)((dim + 63) / 64)), dim3(256), 0, s, fb->partial, nslabs, dim, fb->gsum);
        final_partial = fb->gsum;
        final_slabs = 1;
    }
    // the last kernel writes loss + gradient straight into the pinned host mirror (mapped into the
    // device's address space): no device-to-host copies are queued behind it
    hipLaunchKernelGGL(k_fb_final, dim3(1), dim3(1024), 0, s, final_partial, final_slabs, fb->item, fb->r, n, dim,
                       by_arg ? (const float *)nullptr : (const float *)fb->w, wv,
                       fb->has_q ? fb->qhat : (const float *)nullptr, fb->has_xlx ? fb->xlx : (const float *)nullptr,
                       dev, fb->out_host_dev, fb->loss_host_dev, fb->flag_host_dev, ++fb->seqno);
    SSW_HIP_TRY(hipGetLastError());
    {   // spin on the completion word (the results are in host memory when it flips); the stream wait is the fallback
        const unsigned want = fb->seqno;
        bool seen = false;
        if (!getenv("SSW_FB_NO_SPIN")) {
            const auto t0 = std::chrono::steady_clock::now();
            for (unsigned it = 0;; ++it) {
                if (__atomic_load_n(fb->flag_host, __ATOMIC_ACQUIRE) == want) {
                    seen = true;
                    break;
                }
                if ((it & 1023u) == 1023u &&
                    std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2))
                    break;  // long evaluation (thousands of rows): sleep in the runtime instead
            }
        }
        if (!seen) SSW_HIP_TRY(hipStreamSynchronize(s));
    }
    fb->last_evals++;
    return SSW_OK;
}

// ---- two-output objective: device buffers, one closure evaluation ----------------------------
ssw_status fb2_reserve(ssw_fb *fb) {
    if (fb->cap2 >= fb->cap && fb->cap2 > 0) return SSW_OK;
    SSW_HIP_TRY(hipStreamSynchronize(fb->stream));
    for (float **p : {&fb->y2, &fb->sw2, &fb->z2, &fb->r2, &fb->itemv, &fb->itemh, &fb->partial2}) {
        (void)hipFree(*p);
        *p = nullptr;
    }
    fb->cap2 = 0;
    const int64_t cap = fb->cap > 0 ? fb->cap : 256;
    const int64_t nslabs = (cap + FB_SLAB - 1) / FB_SLAB;
    SSW_HIP_TRY(hipMalloc((void **)&fb->y2, (size_t)2 * cap * sizeof(float)));
    SSW_HIP_TRY(hipMalloc((void **)&fb->sw2, (size_t)cap * sizeof(float)));
    SSW_HIP_TRY(hipMalloc((void **)&fb->z2, (size_t)2 * cap * sizeof(float)));
    SSW_HIP_TRY(hipMalloc((void **)&fb->r2, (size_t)2 * cap * sizeof(float)));
    SSW_HIP_TRY(hipMalloc((void **)&fb->itemv, (size_t)cap * sizeof(float)));
    SSW_HIP_TRY(hipMalloc((void **)&fb->itemh, (size_t)cap * sizeof(float)));
    SSW_HIP_TRY(hipMalloc((void **)&fb->partial2, (size_t)2 * nslabs * fb->dim * sizeof(float)));
    if (!fb->nw2) SSW_HIP_TRY(hipMalloc((void **)&fb->nw2, (size_t)2 * fb->dim * sizeof(float)));
    if (!fb->out2_host) {
        SSW_HIP_TRY(hipHostMalloc((void **)&fb->out2_host, (size_t)(2 + 2 * fb->dim) * sizeof(float), hipHostMallocMapped));
        memset(fb->out2_host, 0, (size_t)(2 + 2 * fb->dim) * sizeof(float));
        SSW_HIP_TRY(hipHostGetDevicePointer((void **)&fb->out2_host_dev, fb->out2_host, 0));
    }
    fb->cap2 = cap;
    return SSW_OK;
}

// the device copies of the raw and the normalised weights (fb_eval2_dev, the one-launch fit's start vector)
ssw_status fb2_dev_reserve(ssw_fb *fb) {
    if (!fb->w2) SSW_HIP_TRY(hipMalloc((void **)&fb->w2, (size_t)(2 * fb->dim + 2) * sizeof(float)));
    if (!fb->nw2) SSW_HIP_TRY(hipMalloc((void **)&fb->nw2, (size_t)2 * fb->dim * sizeof(float)));
    return SSW_OK;
}

// One evaluation of MultiRegModule._step (multi_reg_module.py:64-128) at the raw weights W = fb->w_host [2, dim]:
// the data part (logits, per-row losses, X' r per output) on the device; the O(dim) part -- F.normalize and its
// chain rule, the norm and query regularisers -- here, in f32 like the reference's tensors.
// Results: fb->loss_host[0] = total loss, fb->out_host[1 .. 1 + 2 dim) = d loss / d W.  parts5 (optional):
// loss_norm, loss_queryreg, loss_queryreg2, vertical, horizontal.
ssw_status fb_eval2(ssw_fb *fb, float l_norm, float l_query, float *parts5) {
    hipStream_t s = fb->stream;
    const int64_t n = fb->n;
    const int dim = fb->dim;
    const float *W = fb->w_host;
    float nrm[2], nw[2][1024];
    for (int c = 0; c < 2; ++c) {
        float ss = 0.f;
        for (int k = 0; k < dim; ++k) ss += W[c * dim + k] * W[c * dim + k];
        nrm[c] = std::sqrt(ss);
        const float den = std::fmax(nrm[c], 1e-12f);  // F.normalize's eps
        for (int k = 0; k < dim; ++k) nw[c][k] = W[c * dim + k] / den;
    }
    float vsum = 0.f, hsum = 0.f;
    const float *g = nullptr;  // [2, dim] d labels / d (normalised weights)
    std::vector<float> gz;
    if (n > 0) {
        SSW_REQUIRE(fb->has_targets2 && fb->cap2 >= fb->cap, "feedback: ssw_fb_set_targets2 has not been called for these rows");
        const int64_t plane = fb->cap2;
        const int nslabs = (int)((n + FB_SLAB - 1) / FB_SLAB);
        const int64_t pplane = ((fb->cap2 + FB_SLAB - 1) / FB_SLAB) * dim;
        SSW_HIP_TRY(hipMemcpyAsync(fb->nw2, &nw[0][0], (size_t)dim * sizeof(float), hipMemcpyHostToDevice, s));
        SSW_HIP_TRY(hipMemcpyAsync(fb->nw2 + dim, &nw[1][0], (size_t)dim * sizeof(float), hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_fb2_logits_elem, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, fb->X, fb->nw2, n, dim, plane,
                           fb->y2, fb->sw2, fb->z2, fb->r2, fb->itemv, fb->itemh);
        const int tx = dim < 256 ? dim : 256;
        for (int c = 0; c < 2; ++c)
            hipLaunchKernelGGL(k_fb_grad, dim3((unsigned)nslabs, (unsigned)((dim + tx - 1) / tx)), dim3(tx), 0, s, fb->X,
                               fb->r2 + c * plane, n, dim, fb->partial2 + c * pplane);
        hipLaunchKernelGGL(k_fb2_reduce, dim3(1), dim3(1024), 0, s, fb->partial2, pplane, nslabs, fb->itemv, fb->itemh, n,
                           dim, fb->out2_host_dev, fb->flag_host_dev, ++fb->seqno);
        SSW_HIP_TRY(hipGetLastError());
        const unsigned want = fb->seqno;
        bool seen = false;
        const auto t0 = std::chrono::steady_clock::now();
        for (unsigned it = 0;; ++it) {
            if (__atomic_load_n(fb->flag_host, __ATOMIC_ACQUIRE) == want) {
                seen = true;
                break;
            }
            if ((it & 1023u) == 1023u && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) break;
        }
        if (!seen) SSW_HIP_TRY(hipStreamSynchronize(s));
        vsum = fb->out2_host[0];
        hsum = fb->out2_host[1];
        g = fb->out2_host + 2;
    } else {
        gz.assign((size_t)2 * dim, 0.f);
        g = gz.data();
    }
    SSW_REQUIRE(fb->has_q, "feedback: the two-output objective needs ssw_fb_set_query first");
    const std::vector<float> &qh = fb->qhat_host;
    // regularisers (multi_reg_module.py:112-117), f32
    float loss_norm = 0.f, lq[2];
    float *grad = fb->out_host + 1;
    for (int c = 0; c < 2; ++c) {
        const float lg = std::log(nrm[c]);
        loss_norm += std::cosh(lg) - 1.f;
        float nq = 0.f;
        for (int k = 0; k < dim; ++k) nq += nw[c][k] * qh[(size_t)k];
        lq[c] = l_query * ((1.f - nq) / 2.f);
        // G = d total / d nw_c ; d nw / d W = (I - nw nw') / |W|
        float dotg = 0.f;
        for (int k = 0; k < dim; ++k) dotg += nw[c][k] * (g[c * dim + k] - 0.5f * l_query * qh[(size_t)k]);
        const float den = std::fmax(nrm[c], 1e-12f);
        const float radial = l_norm * std::sinh(lg) / den;  // d [l_norm (cosh(log |W|) - 1)] / d|W|, times d|W|/dW = nw
        for (int k = 0; k < dim; ++k) {
            const float G = g[c * dim + k] - 0.5f * l_query * qh[(size_t)k];
            grad[c * dim + k] = (G - nw[c][k] * dotg) / den + radial * nw[c][k];
        }
    }
    loss_norm *= l_norm;
    const float labels = vsum + hsum;
    const float total = ((labels + loss_norm) + lq[0]) + lq[1];
    fb->loss_host[0] = (double)total;
    if (parts5) {
        parts5[0] = loss_norm; parts5[1] = lq[0]; parts5[2] = lq[1]; parts5[3] = vsum; parts5[4] = hsum;
    }
    fb->last_evals++;
    return SSW_OK;
}

// fb_eval2 with nothing left on the host: one copy of the raw weights, the launches below, one wait.  Results as
// fb_eval2 leaves them (fb->loss_host[0], fb->out_host[1 .. 1 + 2 dim)); parts5 optional.  A set of 0 rows is
// regulariser-only: k_fb2_norm and k_fb2_final_dev alone.
ssw_status fb_eval2_dev(ssw_fb *fb, float l_norm, float l_query, float *parts5) {
    hipStream_t s = fb->stream;
    const int64_t n = fb->n;
    const int dim = fb->dim;
    SSW_REQUIRE(fb->has_q, "feedback: the two-output objective needs ssw_fb_set_query first");
    SSW_REQUIRE(n == 0 || (fb->has_targets2 && fb->cap2 >= fb->cap),
                "feedback: ssw_fb_set_targets2 has not been called for these rows");
    SSW_TRY(fb2_dev_reserve(fb));
    SSW_HIP_TRY(hipMemcpyAsync(fb->w2, fb->w_host, (size_t)2 * dim * sizeof(float), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_fb2_norm, dim3(1), dim3(1024), 0, s, fb->w2, dim, fb->nw2);
    const int nslabs = (int)((n + FB_SLAB - 1) / FB_SLAB);
    const int64_t plane = fb->cap2, pplane = ((fb->cap2 + FB_SLAB - 1) / FB_SLAB) * dim;
    if (n > 0) {
        hipLaunchKernelGGL(k_fb2_logits_elem, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, fb->X, fb->nw2, n, dim, plane,
                           fb->y2, fb->sw2, fb->z2, fb->r2, fb->itemv, fb->itemh);
        const int tx = dim < 256 ? dim : 256;
        for (int c = 0; c < 2; ++c)
            hipLaunchKernelGGL(k_fb_grad, dim3((unsigned)nslabs, (unsigned)((dim + tx - 1) / tx)), dim3(tx), 0, s, fb->X,
                               fb->r2 + c * plane, n, dim, fb->partial2 + c * pplane);
    }
    hipLaunchKernelGGL(k_fb2_final_dev, dim3(1), dim3(1024), 0, s, n > 0 ? fb->partial2 : (const float *)nullptr, pplane, nslabs,
                       fb->itemv, fb->itemh, n, dim, fb->w2, fb->nw2, fb->qhat, l_norm, l_query, fb->out_host_dev,
                       fb->loss_host_dev, fb->flag_host_dev, ++fb->seqno);
    SSW_HIP_TRY(hipGetLastError());
    if (!fb_fit_wg_spin(fb, fb->seqno)) SSW_HIP_TRY(hipStreamSynchronize(s));
    if (parts5) memcpy(parts5, fb->out_host + 1 + 2 * dim, 5 * sizeof(float));
    fb->last_evals++;
    return SSW_OK;
}

}  // namespace ssw

// feedback_fit_wg.hip -- the feedback engine's whole fit in one launch: k_fb_fit_wg, k_fb_fit_wg_batch and their host
// side (gfx950 / MI355X).  The engine's overview is in feedback.hip.  Every value an evaluation or the driver forms
// that the host-driven fit forms too comes from fb_math.h; what is written out here is how one workgroup schedules
// it.  Compiled with -ffp-contract=off (Makefile).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>

#include "fb_handle.h"

namespace ssw {
namespace {

// ---- the whole fit in one launch --------------------------------------------------------------
// k_fb_fit_wg: torch.optim.LBFGS(strong_wolfe).step(closure) -- direction update, line search and every closure
// evaluation -- inside ONE workgroup, for labelled sets of up to FIT_WG_MAX_ROWS rows (a feedback session has
// tens to hundreds).  The host-driven form (lbfgs_host, feedback_lbfgs.hip) pays three launches and a
// host <-> device round trip per closure evaluation, ~27 us each and 80 % of a fit.  Here:
//   * all 16 waves evaluate the closure: logits (a wave per row, eight rows in flight), label loss, gradient
//     (column per thread, the two thread halves take alternate 32-row slabs), regulariser terms -- the bodies of
//     the per-evaluation kernels, with z / r / item losses / targets / the query in LDS so that no phase waits
//     for a global store to become visible; the only global traffic is two passes over the rows, which sit in L2;
//   * wave 0 alone drives: the L-BFGS vectors live in LDS (element k in lane k % 64), reductions are DPP networks
//     inside the wave -- no barrier and no memory round trip in the two-loop recursion; the history is the one
//     structure too large for LDS (100 x 2 x 513 floats) and is prefetched from global one entry ahead.
// The driver is the host loop of lbfgs_host (torch.optim.LBFGS.step + _strong_wolfe) unrolled into a state machine
// around ONE evaluation site: ST_INIT (first closure call), ST_BRACKET (an evaluation of the bracketing phase),
// ST_ZOOM (an evaluation of the zoom phase); ST_NEW_ITER, ST_ZOOM_HEAD, ST_LS_END need no evaluation.
// The arithmetic is the host driver's, operation for operation (wave_sum_host restates the reduction network),
// so both drivers return bit-identical fits, which tests/test_feedback_gpu.py asserts.
constexpr int FIT_ROUND_SLABS = 8;  // slabs whose partial gradients are staged in LDS at a time

struct FitDriver {  // the L-BFGS / line-search scalars of k_fb_fit_wg's driving wave
    double loss, prev_loss, t, H_diag, gtd;
    double f0, d_norm, t_prev, f_prev, gtd_prev, gtd_new;
    double br0, br1, brf0, brf1, brg0, brg1;
    int st, status, n_iter, current_evals, evals, m, head;
    int nbr, low, ls_iter, ls_evals, done, insuf, first_ls_eval;
};

// ---- LDS map of k_fb_fit_wg (the launch sizes the allocation with fit_wg_lds_bytes)
__host__ __device__ inline size_t fit_wg_vec_stride(int dim) { return dim + 1 <= 9 * 64 ? 9 * 64 : 16 * 64; }  // FIT_EPL * 64
constexpr int FIT_OP_ROWS = 16, FIT_OP_BUFS = 3, FIT_OP_DIM = 512;  // fit_eval_onepass: units of rows staged in LDS
__host__ __device__ inline size_t fit_wg_stage_floats(int dim, bool onepass) {
    const size_t a = (size_t)FIT_ROUND_SLABS * dim, b = (size_t)3 * FIT_WG_MAX_ROWS;
    const size_t c = onepass ? (size_t)FIT_OP_BUFS * FIT_OP_ROWS * FIT_OP_DIM : 0;
    return a > b ? (a > c ? a : c) : (b > c ? b : c);
}
constexpr size_t FIT_LDS_DOUBLES = 64 + 16 + 2 * FIT_HISTORY + 2 + 2 + 32 + 8 + FIT_WG_MAX_ROWS + 32 /* FitWgArgs */;
__host__ __device__ inline size_t fit_wg_lds_bytes(int dim, bool onepass) {
    const size_t floats = 1024 /*sw*/ + 1040 /*gout*/ + 4 * FIT_WG_MAX_ROWS /*z r y coef*/ + 1024 /*qhat*/ +
                          7 * fit_wg_vec_stride(dim) + fit_wg_stage_floats(dim, onepass);
    return FIT_LDS_DOUBLES * sizeof(double) + floats * sizeof(float);
}
// pointers read back from the LDS copy of the arguments are generic to the compiler (flat loads, 64-bit address
// arithmetic per access); the phases cast them back to what they are
typedef const float __attribute__((address_space(1))) *fit_gcptr;
typedef float __attribute__((address_space(1))) *fit_gptr;
typedef float fit_v4f __attribute__((ext_vector_type(4)));
typedef const fit_v4f __attribute__((address_space(1))) *fit_g4ptr;

struct FitLds {
    double *red;        // [64]  wave partials of the four-way block sum (fb_final_body)
    double *red2;       // [16]
    double *ro, *al;    // [FIT_HISTORY] 1 / y.s of the history entries; the two-loop recursion's alphas
    double *loss_slot;  // [2]  loss of the last evaluation (f64)
    double *ctl;        // [2]  ctl[0] != 0: the driver has finished
    FitDriver *drv;     // [32 doubles]
    unsigned long long *tk;  // [8] diagnostic timers (100 MHz ticks)
    double *item;       // [FIT_WG_MAX_ROWS] per-item label losses
    FitWgArgs *args;    // [32 doubles] the kernel arguments, for the phases compiled as functions
    float *sw_;         // [1024] parameters of the evaluation
    float *gout;        // [1 + dim + 1 + 4] loss, gradient, parts (the layout k_fb_final emits)
    float *zl, *rl, *yl, *cl;  // [FIT_WG_MAX_ROWS] logits, d loss / d logit, targets, per-item coefficients
    float *qh;          // [dim] unit query
    float *vx, *vd, *vg, *vpg, *vgp, *vb0, *vb1;  // L-BFGS vectors, [FIT_EPL * 64] each, zero beyond element dim
    float *stage;       // pairwise staging [3 n] / partial gradients [FIT_ROUND_SLABS, dim] / fit_eval_onepass's row units
};
__device__ __forceinline__ FitLds fit_lds_map(double *base, int dim) {
    static_assert(sizeof(FitDriver) <= 32 * sizeof(double), "FitDriver outgrew its LDS slot");
    static_assert(sizeof(FitWgArgs) <= 32 * sizeof(double), "FitWgArgs outgrew its LDS slot");
    FitLds S;
    S.red = base;
    S.red2 = S.red + 64;
    S.ro = S.red2 + 16;
    S.al = S.ro + FIT_HISTORY;
    S.loss_slot = S.al + FIT_HISTORY;
    S.ctl = S.loss_slot + 2;
    S.drv = reinterpret_cast<FitDriver *>(S.ctl + 2);
    S.tk = reinterpret_cast<unsigned long long *>(S.ctl + 2 + 32);
    S.item = S.ctl + 2 + 32 + 8;
    S.args = reinterpret_cast<FitWgArgs *>(S.item + FIT_WG_MAX_ROWS);
    S.sw_ = reinterpret_cast<float *>(base + FIT_LDS_DOUBLES);
    S.gout = S.sw_ + 1024;
    S.zl = S.gout + 1040;
    S.rl = S.zl + FIT_WG_MAX_ROWS;
    S.yl = S.rl + FIT_WG_MAX_ROWS;
    S.cl = S.yl + FIT_WG_MAX_ROWS;
    S.qh = S.cl + FIT_WG_MAX_ROWS;
    const int VS = (int)fit_wg_vec_stride(dim);
    S.vx = S.qh + 1024;
    S.vd = S.vx + VS;
    S.vg = S.vd + VS;
    S.vpg = S.vg + VS;
    S.vgp = S.vpg + VS;
    S.vb0 = S.vgp + VS;
    S.vb1 = S.vb0 + VS;
    S.stage = S.vb1 + VS;
    return S;
}

// The phases of one closure evaluation and the driver step are separate (not inlined) functions: each gets the
// whole 128-register budget of a 1024-thread workgroup.  Inlined into one body the kernel spilled 130+ registers
// into scratch inside its hot loops, and every phase ran 3-5x slower than its memory traffic allows.

// z = X w (+ b): a wave per row, eight rows in flight
__device__ __noinline__ void fit_eval_logits(double *base, int dim_) {
    const FitLds S = fit_lds_map(base, dim_);
    const FitWgArgs &a = *S.args;
    const int c = threadIdx.x, lane = c & 63, wave = c >> 6;
    const int n = a.n, dim = a.dim;
    float *sw_ = S.sw_, *zl = S.zl;
    for (int row0 = wave; row0 < n; row0 += 128) {
        float acc[8];
        fit_g4ptr x4[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int row = row0 + 16 * u;
            x4[u] = (fit_g4ptr)(a.X + (int64_t)(row < n ? row : row0) * dim);
            acc[u] = 0.f;
        }
        const float4 *w4 = reinterpret_cast<const float4 *>(sw_);
        for (int k = lane; k < dim / 4; k += 64) {  // the eight rows' loads are issued together
            // (both column steps of a 512-wide row in one trip -- sixteen loads in flight per lane -- was measured:
            //  logits 7.3 -> 10.4 us per evaluation at 390 rows; eight it stays)
            fit_v4f xv[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) xv[u] = x4[u][k];
            const float4 wq = w4[k];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                float s_ = acc[u];
                s_ = fmaf(xv[u].x, wq.x, s_);
                s_ = fmaf(xv[u].y, wq.y, s_);
                s_ = fmaf(xv[u].z, wq.z, s_);
                s_ = fmaf(xv[u].w, wq.w, s_);
                acc[u] = s_;
            }
        }
        // the xor butterfly of k_fb_logits (a += shfl_xor(a, off), off = 32 ... 1) for eight rows at once: at
        // off = 32, 16, 8 each lane keeps half of its rows and hands the other half to its partner, so a step
        // moves 4, 2, 1 values instead of 8, 8, 8 -- the sums formed are the butterfly's (a + b = b + a), bit for bit
        float b4[4], b2[2], b1;
        {
            const bool hi = (lane & 32) != 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float keep = hi ? acc[j + 4] : acc[j], send = hi ? acc[j] : acc[j + 4];
                b4[j] = keep + __shfl_xor(send, 32, 64);
            }
        }
        {
            const bool hi = (lane & 16) != 0;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const float keep = hi ? b4[j + 2] : b4[j], send = hi ? b4[j] : b4[j + 2];
                b2[j] = keep + __shfl_xor(send, 16, 64);
            }
        }
        {
            const bool hi = (lane & 8) != 0;
            const float keep = hi ? b2[1] : b2[0], send = hi ? b2[0] : b2[1];
            b1 = keep + __shfl_xor(send, 8, 64);
        }
        b1 += __shfl_xor(b1, 4, 64);
        b1 += __shfl_xor(b1, 2, 64);
        b1 += __shfl_xor(b1, 1, 64);
        {
            const int u = ((lane >> 5) & 1) * 4 + ((lane >> 4) & 1) * 2 + ((lane >> 3) & 1);
            const int row = row0 + 16 * u;
            if ((lane & 7) == 0 && row < n) zl[row] = b1 + (a.obj.has_bias ? sw_[dim] : 0.f);
        }
    }
}

// per-item label losses and d loss / d logit
__device__ __noinline__ void fit_eval_labels(double *base, int dim_) {
    const FitLds S = fit_lds_map(base, dim_);
    const FitWgArgs &a = *S.args;
    const int c = threadIdx.x;
    const int n = a.n;
    float *zl = S.zl, *yl = S.yl, *cl = S.cl, *rl = S.rl, *stage = S.stage;
    double *item = S.item;
    if (a.label_mode == 0) {
        for (int i = c; i < n; i += 1024) {
            const double zi = zl[i], yi = yl[i], ci = cl[i];
            const double lw = bce_lw(a.pw, yi);
            item[i] = ci * bce_item(zi, yi, lw, a.obj.exact != 0);
            rl[i] = bce_dz(zi, yi, ci, lw);
        }
    } else if (a.label_mode == 1) {
        fb_pairwise_body<0>(zl, yl, cl, a.margin, n, item, rl, stage);
    } else if (a.label_mode == 2) {
        fb_pairwise_body<1>(zl, yl, cl, a.margin, n, item, rl, stage);
    } else {
        for (int i = c; i < n; i += 1024) {
            item[i] = 0.0;
            rl[i] = 0.f;
        }
    }
}

// g = X' r: slabs of FB_SLAB rows, an ordered fma chain inside each (k_fb_grad), the slab sums added in slab
// order (k_fb_final); returns column threadIdx.x's sum
__device__ __noinline__ float fit_eval_grad(double *base, int dim_) {
    const FitLds S = fit_lds_map(base, dim_);
    const FitWgArgs &a = *S.args;
    const int c = threadIdx.x;
    const int n = a.n, dim = a.dim;
    float *rl = S.rl, *stage = S.stage;
    float gcol = 0.f;
    {
        // a thread takes four adjacent columns (16-byte loads); thread group grp = c / (dim / 4) takes slab s0 + grp
        // of every round of FIT_ROUND_SLABS slabs; a slab's chain runs in two halves of 16 rows in flight
        const int dq = dim / 4;
        const int groups = min(FIT_ROUND_SLABS, 1024 / dq);
        const int grp = c / dq, cq = c - grp * dq;
        const int nslabs = (n + FB_SLAB - 1) / FB_SLAB;
        for (int s0 = 0; s0 < nslabs; s0 += groups) {
            const int sl = s0 + grp;
            if (grp < groups && sl < nslabs) {
                const int r0 = sl * FB_SLAB;
                const int cnt = min(r0 + FB_SLAB, n) - r0;
                float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
                // quarters of 8 rows on two register sets: the next quarter's loads are in flight while this one's
                // chain runs (it was two halves of 16, the second requested only after the first had been consumed)
                static_assert(FB_SLAB == 32, "four quarters of eight rows");
                fit_v4f xq[2][8];
#pragma unroll
                for (int i = 0; i < 8; ++i) xq[0][i] = *(fit_g4ptr)(a.X + (int64_t)(r0 + (i < cnt ? i : 0)) * dim + 4 * cq);
#pragma unroll
                for (int qd = 0; qd < 4; ++qd) {
                    const int h = qd * 8;
                    if (qd + 1 < 4) {
#pragma unroll
                        for (int i = 0; i < 8; ++i)
                            xq[(qd + 1) & 1][i] =
                                *(fit_g4ptr)(a.X + (int64_t)(r0 + (h + 8 + i < cnt ? h + 8 + i : 0)) * dim + 4 * cq);
                    }
#pragma unroll
                    for (int i = 0; i < 8; ++i)
                        if (h + i < cnt) {
                            const float ri = rl[r0 + h + i];
                            const fit_v4f xv = xq[qd & 1][i];
                            p.x = fmaf(ri, xv.x, p.x);
                            p.y = fmaf(ri, xv.y, p.y);
                            p.z = fmaf(ri, xv.z, p.z);
                            p.w = fmaf(ri, xv.w, p.w);
                        }
                }
                *reinterpret_cast<float4 *>(stage + (size_t)grp * dim + 4 * cq) = p;
            }
            __syncthreads();
            if (c < dim)
                for (int j = 0; j < groups && s0 + j < nslabs; ++j) gcol += stage[(size_t)j * dim + c];
            __syncthreads();
        }
    }
    return gcol;
}

// The three phases above in ONE pass over the rows (elementwise BCE, dim = 512): the rows are what an evaluation
// costs -- a CU pulls them from L2 at ~110 GB/s, and the logits and the gradient each walked them once.  Here a
// unit of 16 rows is loaded once, by the waves that take its logits (lane k the float4s k and k + 64 of a row --
// fit_eval_logits' assignment, so the fma chain and the butterfly's additions are the same), and copied to LDS on
// the way for the gradient chain, which needs it two barriers later.  The waves have roles:
//     stage s :  waves 4-11  loads of unit s + 2 issued; logits of unit s (two rows a wave), its rows to LDS
//                wave 12     d loss / d logit of unit s - 1 (one f64 exp + divide chain for its 16 rows; on the
//                            logit waves it was 16 wave-wide chains a stage and three times the rows' time)
//                waves 0-3   gradient chain of unit s - 2 from LDS, two columns a thread
// Three row units of 32 KB rotate through LDS.  Every sum keeps its order: a row's logit is the lane chain + xor
// butterfly (v_permlane32/16_swap and row_ror DPP adds form the butterfly's sums without its six LDS round trips);
// a column's slab sum is the fma chain over the slab's rows in row order (a thread keeps it across the slab's two
// units); the slab sums are added in slab order.  The per-item loss values (exp + log1p) are not on the gradient's
// path and are taken after the last unit for all rows at once.  Returns column threadIdx.x's gradient sum.
// Measured (390 rows, tools/perf_fit.py): 15.3 us an evaluation for what took 7.3 + 1.4 + 9.5 = 18.2; a stage is
// ~1260 cycles whatever is taken out of it (no row loads, no f64 chain, no butterfly: 33-35 k cycles a pass each
// time): each role is a latency chain of 800-1000 cycles -- exp + divide in f64, LDS round trips, the wait for the
// rows -- and the barrier adds ~250, i.e. 78 cycles a row against the two passes' 112 and the rows' own 45.
__device__ __forceinline__ float fit_xor_butterfly(float a) {  // a += shfl_xor(a, off), off = 32 ... 1: the same additions
    {
        const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(a), __float_as_uint(a), false, false);
        a = __uint_as_float(r[0]) + __uint_as_float(r[1]);
    }
    {
        const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(a), __float_as_uint(a), false, false);
        a = __uint_as_float(r[0]) + __uint_as_float(r[1]);
    }
    a += dpp_take_f<0x128>(a);  // row_ror 8, 4, 2, 1: the values repeat with that period by then, so a rotation is the xor
    a += dpp_take_f<0x124>(a);
    a += dpp_take_f<0x122>(a);
    a += dpp_take_f<0x121>(a);
    return a;
}

#ifndef SSW_FIT_STAMPS
#define SSW_FIT_STAMPS 0  // diagnostic builds: 1 busy cycles per evaluation of a logit wave, the d loss / d logit wave and a gradient wave; 2 an idle wave's entry -> last stage -> return
#endif
__device__ __noinline__ float fit_eval_onepass(double *base, int dim_) {
    long long t_entry = 0;
    if (SSW_FIT_STAMPS == 2) t_entry = clock64();
    const FitLds S = fit_lds_map(base, dim_);
    const FitWgArgs &a = *S.args;
    const int c = threadIdx.x, lane = c & 63, wave = c >> 6;
    const int n = a.n;
    constexpr int D = FIT_OP_DIM, D4 = FIT_OP_DIM / 4;
    static_assert(FIT_OP_ROWS == 16 && FIT_OP_BUFS == 3 && FB_SLAB == 2 * FIT_OP_ROWS, "roles and rotation below");
    float *rows = S.stage;  // [FIT_OP_BUFS][FIT_OP_ROWS][D]
    float *zl = S.zl, *rl = S.rl, *yl = S.yl, *cl = S.cl;
    // (Spreading the roles over the SIMDs by their VALU cost -- the f64 wave alone with one logit wave -- measured
    // slower: 429 against 397 us of data phases per fit at 390 rows.)
    const bool gwave = wave < 4, zwave = wave >= 4 && wave < 12, rwave = wave == 12;
    const int zslot = wave - 4;
    const int gi = c;  // a gradient thread takes columns 2 gi, 2 gi + 1
    const int zrow = 2 * zslot;  // a logit wave's first row inside the unit
    const int H = (n + FIT_OP_ROWS - 1) / FIT_OP_ROWS;
    const fit_g4ptr X4 = (fit_g4ptr)a.X;
    long long busy = 0;
    float g0 = 0.f, g1 = 0.f;
    // A loop per role, H + 2 barriers each.  (One loop with the roles as branches made the compiler wait for every
    // load in flight before it issued the next unit's: the row loads must stay two stages ahead.)
    if (zwave) {
        // The row loads and their waits are written out (inline asm): left to the compiler, the wait-count pass drained
        // every load in flight at the loop header -- once per three stages no load was in flight, and the rows' stream
        // is what bounds a stage.  Four loads a stage, in order; a stage consumes the set issued two stages earlier,
        // i.e. it waits until at most eight newer loads are outstanding.
#ifndef SSW_FIT_PF
#define SSW_FIT_PF 2  // units of rows in flight ahead of the one a stage consumes
#endif
        constexpr int PF = SSW_FIT_PF, NS = PF + 1;
        fit_v4f xl[NS][2], xh[NS][2];
        auto load = [&](int s, fit_v4f(&lo)[2], fit_v4f(&hi)[2]) {  // s beyond the last unit: the last unit again, unused
            s = s < H ? s : H - 1;
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                int row = FIT_OP_ROWS * s + zrow + u;
                row = row < n ? row : n - 1;
                const fit_g4ptr src = X4 + (int64_t)row * D4 + lane;
                asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(lo[u]) : "v"(src) : "memory");
                asm volatile("global_load_dwordx4 %0, %1, off offset:1024" : "=v"(hi[u]) : "v"(src) : "memory");
            }
        };
#pragma unroll
        for (int q = 0; q < PF; ++q) load(q, xl[q], xh[q]);
        // The rows do not depend on the point of the evaluation: the first units are on their way while wave 0 still
        // drives (the caller enters here without waiting for it).  Behind this barrier sw_ and ctl are published.
        __syncthreads();
        if (S.ctl[0] != 0.0) {  // the driver has finished: nothing to evaluate
#pragma unroll
            for (int q = 0; q < PF; ++q)
                asm volatile("s_waitcnt vmcnt(0)" : "+v"(xl[q][0]), "+v"(xh[q][0]), "+v"(xl[q][1]), "+v"(xh[q][1])::"memory");
            return 0.f;
        }
        const float4 wa = reinterpret_cast<const float4 *>(S.sw_)[lane], wb = reinterpret_cast<const float4 *>(S.sw_)[lane + 64];
        const float bias = a.obj.has_bias ? S.sw_[D] : 0.f;
        for (int s0 = 0; s0 < H; s0 += NS) {
#pragma unroll
            for (int j = 0; j < NS; ++j) {
                const int s = s0 + j;
                if (s >= H) break;
                long long tb = 0;
                if (SSW_FIT_STAMPS == 1) tb = clock64();
                load(s + PF, xl[(j + PF) % NS], xh[(j + PF) % NS]);
                static_assert(PF == 2 || PF == 3, "the wait below names the count");
                if (PF == 2)
                    asm volatile("s_waitcnt vmcnt(8)" : "+v"(xl[j][0]), "+v"(xh[j][0]), "+v"(xl[j][1]), "+v"(xh[j][1])::"memory");
                else
                    asm volatile("s_waitcnt vmcnt(12)" : "+v"(xl[j][0]), "+v"(xh[j][0]), "+v"(xl[j][1]), "+v"(xh[j][1])::"memory");
                float acc[2];
                float *buf = rows + (size_t)(s % 3) * FIT_OP_ROWS * D;
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const fit_v4f x0 = xl[j][u], x1 = xh[j][u];
                    float t = 0.f;
                    t = fmaf(x0.x, wa.x, t);
                    t = fmaf(x0.y, wa.y, t);
                    t = fmaf(x0.z, wa.z, t);
                    t = fmaf(x0.w, wa.w, t);
                    t = fmaf(x1.x, wb.x, t);
                    t = fmaf(x1.y, wb.y, t);
                    t = fmaf(x1.z, wb.z, t);
                    t = fmaf(x1.w, wb.w, t);
                    acc[u] = t;
                    float *dst = buf + (size_t)(zrow + u) * D;
                    *reinterpret_cast<fit_v4f *>(dst + 4 * lane) = x0;
                    *reinterpret_cast<fit_v4f *>(dst + 256 + 4 * lane) = x1;
                }
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const float z = fit_xor_butterfly(acc[u]) + bias;
                    const int row = FIT_OP_ROWS * s + zrow + u;
                    if (lane == 0 && row < n) zl[row] = z;
                }
                if (SSW_FIT_STAMPS == 1) busy += clock64() - tb;
                __syncthreads();
            }
        }
        // the loads still in flight land in registers the compiler would otherwise hand out again
#pragma unroll
        for (int q = 0; q < NS; ++q)
            asm volatile("s_waitcnt vmcnt(0)" : "+v"(xl[q][0]), "+v"(xh[q][0]), "+v"(xl[q][1]), "+v"(xh[q][1])::"memory");
        __syncthreads();
        __syncthreads();
    } else if (rwave) {
        __syncthreads();
        if (S.ctl[0] != 0.0) return 0.f;
        for (int s = 0; s < H + 2; ++s) {
            long long tb = 0;
            if (SSW_FIT_STAMPS == 1) tb = clock64();
            const int row = FIT_OP_ROWS * (s - 1) + lane;
            if (s >= 1 && s - 1 < H && lane < FIT_OP_ROWS && row < n) {
                const double yi = yl[row], ci = cl[row];
                rl[row] = bce_dz((double)zl[row], yi, ci, bce_lw(a.pw, yi));
            }
            if (SSW_FIT_STAMPS == 1) busy += clock64() - tb;
            __syncthreads();
        }
    } else if (gwave) {
        __syncthreads();
        if (S.ctl[0] != 0.0) return 0.f;
        float p0 = 0.f, p1 = 0.f;
        for (int s = 0; s < H + 2; ++s) {
            long long tb = 0;
            if (SSW_FIT_STAMPS == 1) tb = clock64();
            if (s >= 2) {
                const int u = s - 2, r0 = FIT_OP_ROWS * u;
                const float *src = rows + (size_t)(u % 3) * FIT_OP_ROWS * D + 2 * gi;
                if (r0 + FIT_OP_ROWS <= n) {
                    float rr[FIT_OP_ROWS];  // the unit's sixteen rows in flight together: one LDS latency, not two
                    float2 xv[FIT_OP_ROWS];
#pragma unroll
                    for (int q = 0; q < FIT_OP_ROWS / 4; ++q) {
                        const float4 t = *reinterpret_cast<const float4 *>(rl + r0 + 4 * q);
                        rr[4 * q + 0] = t.x;
                        rr[4 * q + 1] = t.y;
                        rr[4 * q + 2] = t.z;
                        rr[4 * q + 3] = t.w;
                    }
#pragma unroll
                    for (int i = 0; i < FIT_OP_ROWS; ++i) xv[i] = *reinterpret_cast<const float2 *>(src + (size_t)i * D);
#pragma unroll
                    for (int i = 0; i < FIT_OP_ROWS; ++i) {
                        p0 = fmaf(rr[i], xv[i].x, p0);
                        p1 = fmaf(rr[i], xv[i].y, p1);
                    }
                } else {
                    for (int i = 0; r0 + i < n; ++i) {
                        const float2 xv = *reinterpret_cast<const float2 *>(src + (size_t)i * D);
                        const float ri = rl[r0 + i];
                        p0 = fmaf(ri, xv.x, p0);
                        p1 = fmaf(ri, xv.y, p1);
                    }
                }
                if ((u & 1) || u == H - 1) {  // the slab is complete
                    g0 += p0;
                    g1 += p1;
                    p0 = 0.f;
                    p1 = 0.f;
                }
            }
            if (SSW_FIT_STAMPS == 1) busy += clock64() - tb;
            __syncthreads();
        }
    } else {
        __syncthreads();
        if (S.ctl[0] != 0.0) return 0.f;
        for (int s = 0; s < H + 2; ++s) __syncthreads();
    }
    long long t_loop = 0;
    if (SSW_FIT_STAMPS == 2) t_loop = clock64();
    if (SSW_FIT_STAMPS == 1 && lane == 0) {
        if (wave == 4) S.tk[4] += (unsigned long long)busy;
        if (wave == 12) S.tk[6] += (unsigned long long)busy;
        if (wave == 0) S.tk[7] += (unsigned long long)busy;
    }
    // columns back to their threads (thread c: column c)
    if (gwave) *reinterpret_cast<float2 *>(rows + 2 * gi) = make_float2(g0, g1);
    // the loss values of all rows (exp + log1p: ~1700 cycles a chain -- as a wave's job inside the stages it was the
    // longest of them and cost 130 us a fit; here all rows' chains run side by side once, ~1 us)
    for (int i = c; i < n; i += 1024) {
        const double zi = zl[i], yi = yl[i], ci = cl[i];
        S.item[i] = ci * bce_item(zi, yi, bce_lw(a.pw, yi), a.obj.exact != 0);
    }
    __syncthreads();
    if (SSW_FIT_STAMPS == 2 && c == 1023) {  // an idle wave's view: entry -> loop end -> return
        S.tk[4] += (unsigned long long)(t_loop - t_entry);
        S.tk[6] += (unsigned long long)(clock64() - t_loop);
    }
    return c < D ? rows[c] : 0.f;
}

// the last step of an evaluation: k_fb_final's body on the LDS copies
__device__ __noinline__ void fit_eval_final(double *base, int dim_, float gcol) {
    const FitLds S = fit_lds_map(base, dim_);
    const FitWgArgs &a = *S.args;
    const int c = threadIdx.x;
    const FbFinalLds L{S.red, S.red2, S.sw_};
    fb_final_body(gcol, c < a.dim ? S.sw_[c] : 0.f, S.item, S.rl, a.n, a.dim, a.qhat ? S.qh : (const float *)nullptr, a.xlx,
                  a.obj, S.gout, S.loss_slot, L);
}

// One step of the driver (wave 0): consumes the evaluation in gout / loss_slot, advances the L-BFGS / line-search
// state machine up to the next point that needs an evaluation, and publishes that point in sw_ (or ctl[0] = 1).
// FIT_EPL: vector elements per lane (9 covers dim + 1 <= 576, 16 covers 1024).
template <int FIT_EPL>
__device__ __noinline__ void fit_driver_step(double *base, int dim_) {
    const FitLds S = fit_lds_map(base, dim_);
    const FitWgArgs &a = *S.args;
    const int lane = threadIdx.x & 63;
    const int dim = a.dim, Pd = dim + 1;
    double *ro = S.ro, *al = S.al, *loss_slot = S.loss_slot, *ctl = S.ctl;
    float *sw_ = S.sw_, *gout = S.gout;
    float *vx = S.vx, *vd = S.vd, *vg = S.vg, *vpg = S.vpg, *vgp = S.vgp, *vb0 = S.vb0, *vb1 = S.vb1;
    enum { ST_INIT, ST_BRACKET, ST_ZOOM, ST_NEW_ITER, ST_ZOOM_HEAD, ST_LS_END };
    FitDriver D = *S.drv;  // a register copy for the duration of the step (LDS round trips between dependent scalar
                           // operations were most of a step's time); written back on the way out
    int &st = D.st, &status = D.status, &n_iter = D.n_iter, &current_evals = D.current_evals, &evals = D.evals;
    int &m = D.m, &head = D.head;  // history ring: logical entry i sits in slot (head + i) % FIT_HISTORY
    int &nbr = D.nbr, &low = D.low, &ls_iter = D.ls_iter, &ls_evals = D.ls_evals;
    int &done = D.done, &insuf = D.insuf, &first_ls_eval = D.first_ls_eval;
    double &loss = D.loss, &prev_loss = D.prev_loss, &t = D.t, &H_diag = D.H_diag, &gtd = D.gtd;
    double &f0 = D.f0, &d_norm = D.d_norm, &t_prev = D.t_prev, &f_prev = D.f_prev, &gtd_prev = D.gtd_prev;
    double &gtd_new = D.gtd_new;
    double &br0 = D.br0, &br1 = D.br1, &brf0 = D.brf0, &brf1 = D.brf1, &brg0 = D.brg0, &brg1 = D.brg1;  // bracket ends: t, f, g.d
    const double tol_grad = 1e-7, tol_change = 1e-9, c1 = 1e-4, c2 = 0.9;
    const int max_ls = 25;
    const int max_eval = a.max_iter * 5 / 4;
    // vector helpers: element k of a vector lives in lane k % 64.  The L-BFGS vectors are FIT_EPL * 64 long and zero
    // beyond element dim, so the loops are unrolled without bounds checks (the LDS reads overlap); `g_new` is the one
    // operand with live data behind element dim (the loss parts): it is masked when copied and only ever multiplied
    // with a padded vector otherwise.
    // dot products are f32 throughout, like torch's (a BLAS sdot there; here: per-lane products added in ascending
    // order, then wave_sum_f's network) -- one wave owns the whole recursion, so every instruction saved is latency
    auto vdot = [&](const float *u, const float *v) -> double {
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < FIT_EPL; ++j) s += u[lane + 64 * j] * v[lane + 64 * j];
        return (double)wave_sum_f(s);
    };
    auto vabsmax = [&](const float *u) -> double {
        double mx = 0.0;
#pragma unroll
        for (int j = 0; j < FIT_EPL; ++j) mx = fmax(mx, (double)fabsf(u[lane + 64 * j]));
        return wave_max_d(mx);
    };
    auto vcopy = [&](float *dst, const float *src) {
        float v[FIT_EPL];
#pragma unroll
        for (int j = 0; j < FIT_EPL; ++j) v[j] = src[lane + 64 * j];
#pragma unroll
        for (int j = 0; j < FIT_EPL; ++j) dst[lane + 64 * j] = lane + 64 * j < Pd ? v[j] : 0.f;
    };
    const float *g_new = gout + 1;  // the gradient of the last evaluation (element dim is forced to 0 without intercept)

    evals++;
    if (a.P == dim && lane == 0) gout[1 + dim] = 0.f;  // no intercept: that slot is not a parameter
    const double f_new = loss_slot[0];
    bool finished = false;
    if (!isfinite(f_new)) {
        status = 1;
        finished = true;
    } else if (st == ST_INIT) {
        loss = f_new;
        vcopy(vg, g_new);
        current_evals = 1;
        prev_loss = loss;
        if (vabsmax(vg) <= tol_grad) finished = true;
        st = ST_NEW_ITER;
    } else if (st == ST_BRACKET) {
        if (first_ls_eval) {
            ls_evals = 1;
            first_ls_eval = 0;
        } else {
            ls_evals++;
            ls_iter++;
        }
        gtd_new = vdot(g_new, vd);
        bool next_eval = false;
        if (ls_iter < max_ls) {
            if (f_new > (f0 + c1 * t * gtd) || (ls_iter > 1 && f_new >= f_prev)) {
                br0 = t_prev; br1 = t; brf0 = f_prev; brf1 = f_new;
                vcopy(vb0, vgp); vcopy(vb1, g_new); brg0 = gtd_prev; brg1 = gtd_new; nbr = 2;
            } else if (fabs(gtd_new) <= -c2 * gtd) {
                br0 = t; brf0 = f_new; vcopy(vb0, g_new); nbr = 1;
                done = 1;
            } else if (gtd_new >= 0) {
                br0 = t_prev; br1 = t; brf0 = f_prev; brf1 = f_new;
                vcopy(vb0, vgp); vcopy(vb1, g_new); brg0 = gtd_prev; brg1 = gtd_new; nbr = 2;
            } else {
                const double min_step = t + 0.01 * (t - t_prev), max_step = t * 10;
                const double tmp = t;
                t = cubic_interpolate_dev(t_prev, f_prev, gtd_prev, t, f_new, gtd_new, true, min_step, max_step);
                t_prev = tmp; f_prev = f_new; vcopy(vgp, g_new); gtd_prev = gtd_new;
                next_eval = true;
            }
        } else {  // max_ls interpolations without a bracket: [0, t]
            br0 = 0; br1 = t; brf0 = f0; brf1 = f_new; vcopy(vb0, vg); vcopy(vb1, g_new); nbr = 2;
            brg0 = gtd; brg1 = gtd_new;
        }
        if (!next_eval) {
            insuf = 0;
            low = 0;
            if (nbr == 2) low = brf0 <= brf1 ? 0 : 1;
            st = ST_ZOOM_HEAD;
        }
    } else {  // ST_ZOOM
        ls_evals++;
        gtd_new = vdot(g_new, vd);
        ls_iter++;
        const double brf_low = low == 0 ? brf0 : brf1;
        if (f_new > (f0 + c1 * t * gtd) || f_new >= brf_low) {
            if (low == 0) { br1 = t; brf1 = f_new; vcopy(vb1, g_new); brg1 = gtd_new; }
            else          { br0 = t; brf0 = f_new; vcopy(vb0, g_new); brg0 = gtd_new; }
            low = brf0 <= brf1 ? 0 : 1;
        } else {
            if (fabs(gtd_new) <= -c2 * gtd) {
                done = 1;
            } else {
                const double br_high = low == 0 ? br1 : br0, br_low = low == 0 ? br0 : br1;
                if (gtd_new * (br_high - br_low) >= 0) {
                    if (low == 0) { br1 = br0; brf1 = brf0; vcopy(vb1, vb0); brg1 = brg0; }
                    else          { br0 = br1; brf0 = brf1; vcopy(vb0, vb1); brg0 = brg1; }
                }
            }
            if (low == 0) { br0 = t; brf0 = f_new; vcopy(vb0, g_new); brg0 = gtd_new; }
            else          { br1 = t; brf1 = f_new; vcopy(vb1, g_new); brg1 = gtd_new; }
        }
        st = ST_ZOOM_HEAD;
    }

    while (!finished && st != ST_BRACKET && st != ST_ZOOM) {
        if (st == ST_ZOOM_HEAD) {
            if (done || ls_iter >= max_ls || fabs(br1 - br0) * d_norm < tol_change) {
                st = ST_LS_END;
                continue;
            }
            t = cubic_interpolate_dev(br0, brf0, brg0, br1, brf1, brg1, false, 0, 0);
            const double bmax = fmax(br0, br1), bmin = fmin(br0, br1);
            const double eps = 0.1 * (bmax - bmin);
            if (fmin(bmax - t, t - bmin) < eps) {
                if (insuf || t >= bmax || t <= bmin) {
                    t = (fabs(t - bmax) < fabs(t - bmin)) ? bmax - eps : bmin + eps;
                    insuf = 0;
                } else {
                    insuf = 1;
                }
            } else {
                insuf = 0;
            }
            st = ST_ZOOM;
        } else if (st == ST_LS_END) {
            // accepted point: the bracket's low end
            loss = low == 0 ? brf0 : brf1;
            vcopy(vg, low == 0 ? vb0 : vb1);
            t = low == 0 ? br0 : br1;
            double dm = 0.0;  // max_i |d_i t| in f64, as the host forms it
            for (int k = lane; k < Pd; k += 64) {
                vx[k] += (float)t * vd[k];
                dm = fmax(dm, fabs((double)vd[k] * t));
            }
            dm = wave_max_d(dm);
            const bool opt_cond = vabsmax(vg) <= tol_grad;
            current_evals += ls_evals;
            if (n_iter == a.max_iter || current_evals >= max_eval || opt_cond || dm <= tol_change ||
                fabs(loss - prev_loss) < tol_change) {
                finished = true;
                break;
            }
            st = ST_NEW_ITER;
        } else {  // ST_NEW_ITER: the optimality test of the initial point / previous iteration has passed
            if (n_iter >= a.max_iter) {
                finished = true;
                break;
            }
            n_iter++;
            if (n_iter == 1) {
                for (int k = lane; k < Pd; k += 64) vd[k] = -vg[k];
                H_diag = 1.0;
            } else {
                const unsigned long long t2l = wall_clock64();
                // y = g - prev_g, s = d t
                float yv[FIT_EPL], sv[FIT_EPL];
                float pys = 0.f, pyy = 0.f;
#pragma unroll
                for (int j = 0; j < FIT_EPL; ++j) {
                    const int k = lane + 64 * j;
                    yv[j] = vg[k] - vpg[k];  // the vectors are zero beyond element dim
                    sv[j] = vd[k] * (float)t;
                    pys += yv[j] * sv[j];
                    pyy += yv[j] * yv[j];
                }
                const double ys = (double)wave_sum_f(pys);
                if (ys > 1e-10) {
                    if (m == FIT_HISTORY) {
                        head = (head + 1) % FIT_HISTORY;
                        m--;
                    }
                    const int slot = (head + m) % FIT_HISTORY;
#pragma unroll
                    for (int j = 0; j < FIT_EPL; ++j) {
                        ((fit_gptr)a.hist_dirs + (size_t)slot * 1024 + lane)[64 * j] = yv[j];
                        ((fit_gptr)a.hist_stps + (size_t)slot * 1024 + lane)[64 * j] = sv[j];
                    }
                    if (lane == 0) ro[slot] = 1.0 / ys;
                    m++;
                    H_diag = ys / (double)wave_sum_f(pyy);
                }
                // two-loop recursion, q in registers.  A step is ~60 instructions of one wave (~300 cycles) and needs
                // one history entry (2 x 513 floats in L2, ~800 cycles away): four register sets, entries loaded three
                // steps ahead, the trip unrolled by four so the sets rotate without copies.
                const fit_gcptr hst = (fit_gcptr)a.hist_stps + lane, hdr = (fit_gcptr)a.hist_dirs + lane;
                float q[FIT_EPL], sb[4][FIT_EPL], db[4][FIT_EPL];
#pragma unroll
                for (int j = 0; j < FIT_EPL; ++j) {
                    q[j] = -vg[lane + 64 * j];
#pragma unroll
                    for (int u = 0; u < 4; ++u) sb[u][j] = db[u][j] = 0.f;
                }
                auto load_entry = [&](int i, float *s_out, float *d_out) {
                    const int slot = (head + i) % FIT_HISTORY;
                    const fit_gcptr ps = hst + (size_t)slot * 1024, pd = hdr + (size_t)slot * 1024;
#pragma unroll
                    for (int j = 0; j < FIT_EPL; ++j) {
                        s_out[j] = ps[64 * j];
                        d_out[j] = pd[64 * j];
                    }
                };
                auto first_loop_step = [&](int i, const float *cs, const float *cd) {
                    const double roi = ro[(head + i) % FIT_HISTORY];  // read before the reduction, not after it
                    float p = 0.f;
#pragma unroll
                    for (int j = 0; j < FIT_EPL; ++j) p += cs[j] * q[j];
                    const double ali = (double)wave_sum_f(p) * roi;
                    if (lane == 0) al[i] = ali;
#pragma unroll
                    for (int j = 0; j < FIT_EPL; ++j) q[j] -= (float)ali * cd[j];
                };
#pragma unroll
                for (int u = 0; u < 3; ++u)
                    if (u < m) load_entry(m - 1 - u, sb[u], db[u]);
                for (int k0 = 0; k0 < m; k0 += 4) {
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int k = k0 + u;  // step k works on entry m - 1 - k
                        if (k < m) {
                            if (k + 3 < m) load_entry(m - 1 - (k + 3), sb[(u + 3) & 3], db[(u + 3) & 3]);
                            first_loop_step(m - 1 - k, sb[u], db[u]);
                        }
                    }
                }
#pragma unroll
                for (int j = 0; j < FIT_EPL; ++j) q[j] = q[j] * (float)H_diag;  // q is now d
                auto second_loop_step = [&](int i, const float *cs, const float *cd) {
                    const double roi = ro[(head + i) % FIT_HISTORY], ali = al[i];
                    float p = 0.f;
#pragma unroll
                    for (int j = 0; j < FIT_EPL; ++j) p += cd[j] * q[j];
                    const double be = (double)wave_sum_f(p) * roi;
                    const float cf = (float)(ali - be);
#pragma unroll
                    for (int j = 0; j < FIT_EPL; ++j) q[j] += cf * cs[j];
                };
#pragma unroll
                for (int u = 0; u < 3; ++u)
                    if (u < m) load_entry(u, sb[u], db[u]);
                for (int k0 = 0; k0 < m; k0 += 4) {
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int k = k0 + u;
                        if (k < m) {
                            if (k + 3 < m) load_entry(k + 3, sb[(u + 3) & 3], db[(u + 3) & 3]);
                            second_loop_step(k, sb[u], db[u]);
                        }
                    }
                }
#pragma unroll
                for (int j = 0; j < FIT_EPL; ++j) {
                    vd[lane + 64 * j] = q[j];
                }
                if (lane == 0) S.tk[5] += wall_clock64() - t2l;
            }
            vcopy(vpg, vg);
            prev_loss = loss;
            if (n_iter == 1) {
                double pa = 0.0;
                for (int k = lane; k < Pd; k += 64) pa += (double)fabsf(vg[k]);
                const double gs = wave_sum_d(pa);
                t = fmin(1.0, 1.0 / gs) * (double)a.lr;
            } else {
                t = (double)a.lr;
            }
            gtd = vdot(vg, vd);
            if (gtd > -tol_change) {
                finished = true;
                break;
            }
            // line-search set-up
            f0 = loss;
            d_norm = vabsmax(vd);
            t_prev = 0; f_prev = f0; gtd_prev = gtd;
            vcopy(vgp, vg);
            done = 0;
            ls_iter = 0;
            nbr = 0;
            first_ls_eval = 1;
            st = ST_BRACKET;
        }
    }
    if (finished) {
        if (lane == 0) ctl[0] = 1.0;
    } else {
#pragma unroll
        for (int j = 0; j < FIT_EPL; ++j) sw_[lane + 64 * j] = vx[lane + 64 * j] + (float)t * vd[lane + 64 * j];
    }
    if (lane == 0) *S.drv = D;
}

// The body both fit kernels run, from the LDS set-up to the publish by wave 0.  Nothing in it (nor in fit_eval_*,
// fit_driver_step, fb_final_body) reads blockIdx / gridDim or a global scratch word: a workgroup touches its LDS and
// the buffers its FitWgArgs name, so any number of them run side by side.  ARG_W: the start vector may sit in the
// argument segment (`w0v`, the single launch); without it `w0_or_null` is set.
template <int FIT_EPL, bool ARG_W>
__device__ __forceinline__ void fit_wg_body(double *fit_lds, const FitWgArgs &a_in, const FbW *w0v) {
    const int c = threadIdx.x, lane = c & 63, wave = c >> 6;
    const int dim = a_in.dim, n = a_in.n, Pd = dim + 1;
    const FitLds S = fit_lds_map(fit_lds, dim);
    const int VS = (int)fit_wg_vec_stride(dim);
    if (c == 0) {
        *S.args = a_in;
        FitDriver z0;
        memset(&z0, 0, sizeof(z0));
        z0.H_diag = 1.0;  // st = ST_INIT = 0
        *S.drv = z0;
        S.ctl[0] = 0.0;
        for (int i = 0; i < 8; ++i) S.tk[i] = 0;
    }
    for (int i = c; i < n; i += 1024) {
        S.yl[i] = a_in.y[i];
        S.cl[i] = a_in.coef[i];
    }
    if (c < dim) S.qh[c] = a_in.qhat ? a_in.qhat[c] : 0.f;
    for (int k = c; k < 1040; k += 1024) S.gout[k] = 0.f;  // the driver reads it FIT_EPL * 64 wide
    for (int k = c; k < VS; k += 1024) {
        float x0 = 0.f;
        if (k < a_in.P) {
            if constexpr (ARG_W) x0 = a_in.w0_or_null ? a_in.w0_or_null[k] : w0v->v[k < FB_ARG_FLOATS ? k : 0];
            else x0 = a_in.w0_or_null[k];
        }
        S.vx[k] = x0;
        S.vd[k] = 0.f;
        S.vg[k] = 0.f;
        S.vpg[k] = 0.f;
        S.vgp[k] = 0.f;
        S.vb0[k] = 0.f;
        S.vb1[k] = 0.f;
        if (k < 1024) S.sw_[k] = x0 + (float)0.0 * 0.f;  // the first closure call: f(x + 0 d)
    }
    // The set-up is published before any phase runs: fit_eval_onepass reads n and X out of S.args on entry, ahead of
    // its own first barrier (the early row loads).  Without this barrier a wave with no set-up work of its own could
    // get there before thread 0 had stored the arguments and take the previous workgroup's -- rows of an engine
    // that may have been destroyed since (an illegal access, seen once in a batch of 261 slots).
    __syncthreads();
    const unsigned long long t_kernel0 = wall_clock64();
    const long long c_kernel0 = clock64();
    for (;;) {
        unsigned long long tq0 = wall_clock64();
        float gcol;
        if (a_in.onepass) {
            // the barrier that publishes sw_ / ctl is inside: the logit waves request their first rows ahead of it
            gcol = fit_eval_onepass(fit_lds, dim);
            if (S.ctl[0] != 0.0) break;
            __syncthreads();
            if (c == 0) { const unsigned long long q = wall_clock64(); S.tk[0] += q - tq0; tq0 = q; }
        } else {
            __syncthreads();  // sw_ and ctl are published
            if (S.ctl[0] != 0.0) break;
            tq0 = wall_clock64();
            fit_eval_logits(fit_lds, dim);
            __syncthreads();
            if (c == 0) { const unsigned long long q = wall_clock64(); S.tk[0] += q - tq0; tq0 = q; }
            fit_eval_labels(fit_lds, dim);
            __syncthreads();
            if (c == 0) { const unsigned long long q = wall_clock64(); S.tk[1] += q - tq0; tq0 = q; }
            gcol = fit_eval_grad(fit_lds, dim);
            if (c == 0) { const unsigned long long q = wall_clock64(); S.tk[2] += q - tq0; tq0 = q; }
        }
        fit_eval_final(fit_lds, dim, gcol);
        __syncthreads();
        if (c == 0) { const unsigned long long q = wall_clock64(); S.tk[3] += q - tq0; tq0 = q; }
        if (wave == 0) fit_driver_step<FIT_EPL>(fit_lds, dim);
    }
    // every wave is here; wave 0 publishes the result
    if (wave == 0) {
        const FitDriver &D = *S.drv;
        for (int k = lane; k < Pd; k += 64) a_in.out_w[k] = S.vx[k];
        if (lane == 0) {
            a_in.out_counts[0] = D.n_iter;
            a_in.out_counts[1] = D.evals;
            a_in.out_counts[2] = D.status;
            for (int i = 0; i < 4; ++i) a_in.out_counts[3 + i] = (int)S.tk[i];
            a_in.out_counts[7] = (int)(wall_clock64() - t_kernel0);
            a_in.out_counts[8] = (int)((clock64() - c_kernel0) >> 4);
            a_in.out_counts[9] = 0;
            a_in.out_counts[10] = (int)S.tk[5];
            a_in.out_counts[11] = (int)(S.tk[4] >> 4);
            a_in.out_counts[12] = (int)(S.tk[6] >> 4);
            a_in.out_counts[13] = (int)(S.tk[7] >> 4);
            *a_in.out_loss = D.loss;
        }
        __threadfence_system();
        if (lane == 0) __hip_atomic_store(a_in.done_flag, a_in.seqno, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

template <int FIT_EPL>
__global__ __launch_bounds__(1024) void k_fb_fit_wg(FitWgArgs a_in, FbW w0v) {
    extern __shared__ double fit_lds[];
    fit_wg_body<FIT_EPL, true>(fit_lds, a_in, &w0v);
}

// k_fb_fit_wg_batch: S independent fits side by side -- the LBFGS of multi_reg.py:156, stepped at
// basic_trainer.py:59-63, taken S times, once per session of a lock-step group -- in one launch and one host wait.  Block b is k_fb_fit_wg for entry b of `table`: its own engine's rows, targets,
// coefficients, history and mapped result words with that engine's sequence number, so it publishes exactly as the
// single launch does and no two blocks share a byte.  The start vector comes through w0_or_null (a row of a device
// table of [nfit][dim + 1] floats).  n, P, label_mode, onepass, max_iter and lr are block-uniform loads: one launch
// mixes objectives and set sizes.  The LDS allocation is the largest any slot needs (`stage` is the last region: a
// larger allocation moves nothing); at 160 KB that is one workgroup a compute unit, further slots queue.
template <int FIT_EPL>
__global__ __launch_bounds__(1024) void k_fb_fit_wg_batch(const FitWgArgs *__restrict__ table) {
    extern __shared__ double fit_lds[];
    const FitWgArgs a_in = table[blockIdx.x];
    fit_wg_body<FIT_EPL, false>(fit_lds, a_in, nullptr);
}

// ---- the two-output objective's whole fit in one launch ------------------------------------------
// k_fb_fit2_wg / k_fb_fit2_wg_batch: k_fb_fit_wg for MultiRegModule's objective (multi_reg_module.py:64-128; the
// LBFGS of multi_reg_module.py:142 stepped at basic_trainer.py:59-63).  The driver is fit_driver_step<16> as it
// stands: 16 x 64 = 1024 vector elements hold the 2 dim <= 1024 parameters exactly, the driver sees them as
// "dim + 1 parameters with intercept" (a.dim = 2 dim2 - 1, a.P = 2 dim2), so no slot is zeroed -- lbfgs_host with
// E.P = 2 dim and zero_slot = -1 on the other side.  Only the evaluation phases are new; what they compute is
// fb_math.h's (fb2_norm_body, fb2_row_terms, fb2_item_tree, fb2_tail_body) in the order of the per-evaluation
// kernels: k_fb2_logits_elem's lane chains and butterfly, k_fb_grad's slab chains, k_fb2_reduce's slab and item sums.
//
// LDS map: FitLds at the 1024 stride (fit_lds_map(base, FIT2_MAP_DIM)), whose regions serve as
//     sw_  raw weights of the evaluation [2 dim2]        gout  loss + gradient [1 + 2 dim2]
//     zl / rl  d loss / d logit, planes 0 / 1            yl / cl  targets, planes 0 / 1
//     item  the per-row vertical [0, 1024) and horizontal [1024, 2048) losses as floats       qh  unit query
// and behind them, in `stage`:
//     sample weights [1024] | normalised weights [1024] | label gradient [1024] | scalars [16] |
//     slab partials [FIT_ROUND_SLABS][2][dim2] (after the gradient: the item tree's 2 x 1024 floats)
constexpr int FIT2_MAP_DIM = 1023;  // any dim of the 16 x 64 vector stride
constexpr size_t FIT2_STAGE_FLOATS = 3 * 1024 + 16 + (size_t)FIT_ROUND_SLABS * 1024;
constexpr size_t FIT2_LDS_BYTES = FIT_LDS_DOUBLES * sizeof(double) +
                                  (1024 + 1040 + 4 * FIT_WG_MAX_ROWS + 1024 + 7 * 1024 + FIT2_STAGE_FLOATS) * sizeof(float);
static_assert(FIT2_LDS_BYTES <= 160 * 1024, "k_fb_fit2_wg's LDS map outgrew the 160 KB attribute");
static_assert(FIT_ROUND_SLABS * 1024 >= 2 * 1024, "the item tree borrows the slab partials' region");
static_assert(FIT_WG_MAX_ROWS == 1024, "one row a thread in the item sums; two float planes in FitLds::item");

struct Fit2Lds {
    float *sw;     // [FIT_WG_MAX_ROWS] sample weights
    float *nw;     // [1024] normalised weights
    float *glab;   // [1024] d labels / d nw
    float *sc;     // [16]
    float *part;   // [FIT_ROUND_SLABS][2][dim2]
    float *iv, *ih;  // [FIT_WG_MAX_ROWS] per-row losses
};
__device__ __forceinline__ Fit2Lds fit2_lds_map(const FitLds &S) {
    Fit2Lds T;
    T.sw = S.stage;
    T.nw = T.sw + 1024;
    T.glab = T.nw + 1024;
    T.sc = T.glab + 1024;
    T.part = T.sc + 16;
    T.iv = reinterpret_cast<float *>(S.item);
    T.ih = T.iv + FIT_WG_MAX_ROWS;
    return T;
}
__device__ __forceinline__ Fb2Lds fit2_math_lds(const FitLds &S, const Fit2Lds &T) {
    return Fb2Lds{S.sw_, T.nw, T.glab, S.qh, T.sc, T.part, T.part + 1024};
}

__device__ __noinline__ void fit2_eval_norm(double *base) {
    const FitLds S = fit_lds_map(base, FIT2_MAP_DIM);
    const Fit2Lds T = fit2_lds_map(S);
    fb2_norm_body(fit2_math_lds(S, T), S.args->dim2);
}

// two logits a row from both normalised weight rows (a wave takes four rows at a time, their loads in flight
// together; per row k_fb2_logits_elem's lane chains and xor butterfly), then lanes 0-3 one row's label terms each
__device__ __noinline__ void fit2_eval_logits_labels(double *base) {
    const FitLds S = fit_lds_map(base, FIT2_MAP_DIM);
    const Fit2Lds T = fit2_lds_map(S);
    const FitWgArgs &a = *S.args;
    const int c = threadIdx.x, lane = c & 63, wave = c >> 6;
    const int n = a.n, dim = a.dim2;
    const float4 *w0 = reinterpret_cast<const float4 *>(T.nw), *w1 = reinterpret_cast<const float4 *>(T.nw + dim);
    for (int row0 = wave * 4; row0 < n; row0 += 64) {
        fit_g4ptr x4[4];
        float pa[4], pb[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            x4[u] = (fit_g4ptr)(a.X + (int64_t)(row0 + u < n ? row0 + u : row0) * dim);
            pa[u] = 0.f;
            pb[u] = 0.f;
        }
        for (int k = lane; k < dim / 4; k += 64) {
            fit_v4f xv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) xv[u] = x4[u][k];
            const float4 p = w0[k], q = w1[k];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                float s_ = pa[u], t_ = pb[u];
                s_ = fmaf(xv[u].x, p.x, s_); s_ = fmaf(xv[u].y, p.y, s_); s_ = fmaf(xv[u].z, p.z, s_); s_ = fmaf(xv[u].w, p.w, s_);
                t_ = fmaf(xv[u].x, q.x, t_); t_ = fmaf(xv[u].y, q.y, t_); t_ = fmaf(xv[u].z, q.z, t_); t_ = fmaf(xv[u].w, q.w, t_);
                pa[u] = s_;
                pb[u] = t_;
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                pa[u] += __shfl_xor(pa[u], off, 64);
                pb[u] += __shfl_xor(pb[u], off, 64);
            }
        }
        const float za = lane == 0 ? pa[0] : lane == 1 ? pa[1] : lane == 2 ? pa[2] : pa[3];
        const float zb = lane == 0 ? pb[0] : lane == 1 ? pb[1] : lane == 2 ? pb[2] : pb[3];
        const int row = row0 + lane;
        if (lane < 4 && row < n)
            fb2_row_terms(za, zb, S.yl[row], S.cl[row], T.sw[row], &S.zl[row], &S.rl[row], &T.iv[row], &T.ih[row]);
    }
}

// both gradient planes in one pass over the rows: fit_eval_grad's schedule (four adjacent columns a thread, thread
// group grp the slab s0 + grp of a round, quarters of eight rows on two register sets) with two chains a column --
// k_fb_grad's ordered chain per plane and slab, the slab sums added in slab order (k_fb2_reduce).  Leaves T.glab.
__device__ __noinline__ void fit2_eval_grad(double *base) {
    const FitLds S = fit_lds_map(base, FIT2_MAP_DIM);
    const Fit2Lds T = fit2_lds_map(S);
    const FitWgArgs &a = *S.args;
    const int c = threadIdx.x;
    const int n = a.n, dim = a.dim2;
    const float *r0l = S.zl, *r1l = S.rl;
    float *part = T.part;
    float gcol = 0.f;
    const int dq = dim / 4;
    const int groups = min(FIT_ROUND_SLABS, 1024 / dq);
    const int grp = c / dq, cq = c - grp * dq;
    const int nslabs = (n + FB_SLAB - 1) / FB_SLAB;
    const int pc = c < 2 * dim ? c / dim : 0, kc = c - pc * dim;  // this thread's plane and column in the slab sums
    for (int s0 = 0; s0 < nslabs; s0 += groups) {
        const int sl = s0 + grp;
        if (grp < groups && sl < nslabs) {
            const int r0 = sl * FB_SLAB;
            const int cnt = min(r0 + FB_SLAB, n) - r0;
            float4 p = make_float4(0.f, 0.f, 0.f, 0.f), q = make_float4(0.f, 0.f, 0.f, 0.f);
            static_assert(FB_SLAB == 32, "four quarters of eight rows");
            fit_v4f xq[2][8];
#pragma unroll
            for (int i = 0; i < 8; ++i) xq[0][i] = *(fit_g4ptr)(a.X + (int64_t)(r0 + (i < cnt ? i : 0)) * dim + 4 * cq);
#pragma unroll
            for (int qd = 0; qd < 4; ++qd) {
                const int h = qd * 8;
                if (qd + 1 < 4) {
#pragma unroll
                    for (int i = 0; i < 8; ++i)
                        xq[(qd + 1) & 1][i] =
                            *(fit_g4ptr)(a.X + (int64_t)(r0 + (h + 8 + i < cnt ? h + 8 + i : 0)) * dim + 4 * cq);
                }
#pragma unroll
                for (int i = 0; i < 8; ++i)
                    if (h + i < cnt) {
                        const float ri = r0l[r0 + h + i], si = r1l[r0 + h + i];
                        const fit_v4f xv = xq[qd & 1][i];
                        p.x = fmaf(ri, xv.x, p.x); p.y = fmaf(ri, xv.y, p.y); p.z = fmaf(ri, xv.z, p.z); p.w = fmaf(ri, xv.w, p.w);
                        q.x = fmaf(si, xv.x, q.x); q.y = fmaf(si, xv.y, q.y); q.z = fmaf(si, xv.z, q.z); q.w = fmaf(si, xv.w, q.w);
                    }
            }
            *reinterpret_cast<float4 *>(part + (size_t)(2 * grp) * dim + 4 * cq) = p;
            *reinterpret_cast<float4 *>(part + (size_t)(2 * grp + 1) * dim + 4 * cq) = q;
        }
        __syncthreads();
        if (c < 2 * dim)
            for (int j = 0; j < groups && s0 + j < nslabs; ++j) gcol += part[(size_t)(2 * j + pc) * dim + kc];
        __syncthreads();
    }
    if (c < 2 * dim) T.glab[c] = gcol;
}

// the item sums and the O(dim) tail into gout / loss_slot
__device__ __noinline__ void fit2_eval_final(double *base) {
    const FitLds S = fit_lds_map(base, FIT2_MAP_DIM);
    const Fit2Lds T = fit2_lds_map(S);
    const FitWgArgs &a = *S.args;
    const int c = threadIdx.x;
    const Fb2Lds L = fit2_math_lds(S, T);
    float v = 0.f, h = 0.f;
    if (c < a.n) {  // k_fb2_reduce's `for (i = t; i < n; i += 1024)` at n <= 1024
        v += T.iv[c];
        h += T.ih[c];
    }
    fb2_item_tree(v, h, L.rv, L.rh);
    fb2_tail_body(L, a.dim2, a.obj.l_norm, a.obj.l_query, L.rv[0], L.rh[0], S.gout, S.loss_slot, nullptr);
}

__device__ __forceinline__ void fit2_wg_body(double *fit_lds, const FitWgArgs &a_in) {
    const int c = threadIdx.x, lane = c & 63, wave = c >> 6;
    const int dim = a_in.dim2, n = a_in.n, P = 2 * dim;
    const FitLds S = fit_lds_map(fit_lds, FIT2_MAP_DIM);
    const Fit2Lds T = fit2_lds_map(S);
    if (c == 0) {
        *S.args = a_in;
        FitDriver z0;
        memset(&z0, 0, sizeof(z0));
        z0.H_diag = 1.0;  // st = ST_INIT = 0
        *S.drv = z0;
        S.ctl[0] = 0.0;
        for (int i = 0; i < 8; ++i) S.tk[i] = 0;
    }
    for (int i = c; i < n; i += 1024) {
        S.yl[i] = a_in.y[i];
        S.cl[i] = a_in.y[(size_t)a_in.plane2 + i];
        T.sw[i] = a_in.coef[i];
    }
    if (c < dim) S.qh[c] = a_in.qhat[c];
    for (int k = c; k < 1040; k += 1024) S.gout[k] = 0.f;  // the driver reads it 16 x 64 wide
    {
        const float x0 = c < P ? a_in.w0_or_null[c] : 0.f;
        S.vx[c] = x0;
        S.vd[c] = 0.f;
        S.vg[c] = 0.f;
        S.vpg[c] = 0.f;
        S.vgp[c] = 0.f;
        S.vb0[c] = 0.f;
        S.vb1[c] = 0.f;
        S.sw_[c] = x0 + (float)0.0 * 0.f;  // the first closure call: f(x + 0 d)
    }
    const unsigned long long t_kernel0 = wall_clock64();
    for (;;) {
        __syncthreads();  // the set-up, or the driver's sw_ and ctl, are published
        if (S.ctl[0] != 0.0) break;
        fit2_eval_norm(fit_lds);
        __syncthreads();
        if (n > 0) {
            fit2_eval_logits_labels(fit_lds);
            __syncthreads();
        }
        fit2_eval_grad(fit_lds);  // no slab at n = 0: the label gradient is 0
        __syncthreads();
        fit2_eval_final(fit_lds);
        __syncthreads();
        if (wave == 0) fit_driver_step<16>(fit_lds, FIT2_MAP_DIM);
    }
    if (wave == 0) {  // every wave is here; wave 0 publishes as fit_wg_body does
        const FitDriver &D = *S.drv;
        for (int k = lane; k < P; k += 64) a_in.out_w[k] = S.vx[k];
        if (lane == 0) {
            a_in.out_counts[0] = D.n_iter;
            a_in.out_counts[1] = D.evals;
            a_in.out_counts[2] = D.status;
            for (int i = 3; i < 14; ++i) a_in.out_counts[i] = 0;
            a_in.out_counts[7] = (int)(wall_clock64() - t_kernel0);
            *a_in.out_loss = D.loss;
        }
        __threadfence_system();
        if (lane == 0) __hip_atomic_store(a_in.done_flag, a_in.seqno, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

__global__ __launch_bounds__(1024) void k_fb_fit2_wg(FitWgArgs a_in) {
    extern __shared__ double fit_lds[];
    fit2_wg_body(fit_lds, a_in);
}
// one workgroup per table entry, each on its own engine's buffers and completion word (cf. k_fb_fit_wg_batch)
__global__ __launch_bounds__(1024) void k_fb_fit2_wg_batch(const FitWgArgs *__restrict__ table) {
    extern __shared__ double fit_lds[];
    const FitWgArgs a_in = table[blockIdx.x];
    fit2_wg_body(fit_lds, a_in);
}

// the 160 KB dynamic-LDS attribute of the fit kernel `kern` (batch: k_fb_fit_wg_batch), once per (device, kernel)
ssw_status fb_fit_wg_attr(const void *kern, int device, int dim, bool batch) {
    static bool attr_done[64][4] = {};
    const int dslot = device >= 0 && device < 64 ? device : -1, kslot = (dim + 1 <= 9 * 64 ? 0 : 1) + (batch ? 2 : 0);
    if (dslot < 0 || !attr_done[dslot][kslot]) {
        SSW_HIP_TRY(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        if (dslot >= 0) attr_done[dslot][kslot] = true;
    }
    return SSW_OK;
}

}  // namespace

// ---- the one-launch fit's host side, shared by ssw_fb_fit and ssw_fb_fit_batch ----------------------------------
// a labelled set one workgroup reaches; every other fit is driven from the host, one evaluation at a time
bool fb_fit_wg_eligible(const ssw_fb *fb, const ssw_fb_objective *obj) {
    return fb->n <= FIT_WG_MAX_ROWS && fb->dim + 1 <= 1024 && obj->kind != SSW_FB_RANKREG && !getenv("SSW_FB_HOST_DRIVER");
}

// the arguments of one fit workgroup after fb_prepare (`dev`, `pw`, `pairwise_active` are its outputs); takes the
// engine's next sequence number.  w0_or_null is the caller's.
void fb_fit_wg_fill(ssw_fb *fb, const ssw_fb_objective *obj, const FbObjDev &dev, float pw, bool pairwise_active,
                    int max_iter, float lr, FitWgArgs *out) {
    FitWgArgs a;
    memset(&a, 0, sizeof(a));
    a.X = fb->X; a.y = fb->y; a.coef = fb->coef;
    a.qhat = fb->has_q ? fb->qhat : nullptr;
    a.xlx = fb->has_xlx ? fb->xlx : nullptr;
    a.hist_dirs = fb->hist;
    a.hist_stps = fb->hist + (size_t)FIT_HISTORY * 1024;
    a.out_w = fb->out_host_dev + 1;
    a.out_loss = fb->loss_host_dev;
    a.out_counts = reinterpret_cast<int *>(fb->flag_host_dev) + 4;
    a.done_flag = fb->flag_host_dev;
    a.seqno = ++fb->seqno;
    a.n = (int)fb->n; a.dim = fb->dim; a.P = fb_fit_params(fb, obj);
    const bool pairwise = obj->kind == SSW_FB_MULTIREG && obj->loss_type != SSW_FB_LOSS_CE;
    a.label_mode = !pairwise ? 0 : !pairwise_active ? 3 : obj->loss_type == SSW_FB_LOSS_PAIRWISE_LOGISTIC ? 2 : 1;
    a.pw = pw; a.margin = obj->margin; a.max_iter = max_iter; a.lr = lr; a.obj = dev;
    a.onepass = a.label_mode == 0 && fb->dim == FIT_OP_DIM && fb->n >= 1 && !getenv("SSW_FB_TWO_PASS");  // the variable is the tests' A/B switch
    *out = a;
}

// k_fb_fit_wg for `a` on the engine's stream; the start vector is `w0v` unless a.w0_or_null is set
ssw_status fb_fit_wg_launch(ssw_fb *fb, const FitWgArgs &a, const FbW &w0v) {
    const size_t lds = fit_wg_lds_bytes(fb->dim, a.onepass != 0);
    auto kern = fb->dim + 1 <= 9 * 64 ? k_fb_fit_wg<9> : k_fb_fit_wg<16>;
    SSW_TRY(fb_fit_wg_attr(reinterpret_cast<const void *>(kern), fb->device, fb->dim, false));
    hipLaunchKernelGGL(kern, dim3(1), dim3(1024), lds, fb->stream, a, w0v);
    SSW_HIP_TRY(hipGetLastError());
    return SSW_OK;
}

// k_fb_fit_wg_batch on the lead engine's stream: block b is entry b of lead->batch_tab, whose host copy is `tab`
ssw_status fb_fit_wg_launch_batch(ssw_fb *lead, const FitWgArgs *tab, int nwg) {
    const int dim = lead->dim;
    size_t lds = 0;
    for (int b = 0; b < nwg; ++b) lds = std::max(lds, fit_wg_lds_bytes(dim, tab[b].onepass != 0));
    auto kern = dim + 1 <= 9 * 64 ? k_fb_fit_wg_batch<9> : k_fb_fit_wg_batch<16>;
    SSW_TRY(fb_fit_wg_attr(reinterpret_cast<const void *>(kern), lead->device, dim, true));
    hipLaunchKernelGGL(kern, dim3(nwg), dim3(1024), lds, lead->stream, (const FitWgArgs *)lead->batch_tab);
    SSW_HIP_TRY(hipGetLastError());
    return SSW_OK;
}

// bounded spin on the engine's completion word; false = not seen (the caller synchronises the launch stream)
bool fb_fit_wg_spin(const ssw_fb *fb, unsigned want) {
    if (getenv("SSW_FB_NO_SPIN")) return false;
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned it = 0;; ++it) {
        if (__atomic_load_n(fb->flag_host, __ATOMIC_ACQUIRE) == want) return true;
        if ((it & 1023u) == 1023u && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) return false;
    }
}

// what a finished fit workgroup left in the engine's mapped words: bookkeeping, the divergence checks, the weights
ssw_status fb_fit_wg_collect(ssw_fb *fb, int P, float *w_inout, int32_t *out_iters, int32_t *out_evals,
                             float *out_final_loss) {
    const int *counts = reinterpret_cast<const int *>(fb->flag_host) + 4;
    fb->last_iters = counts[0];
    fb->last_evals = counts[1];
    fb->last_fit_on_device = true;
    if (counts[2] != 0) {
        set_error("feedback: loss diverged -- regression training failed with a nan");
        return SSW_ERR_NUMERIC;  // logistic_regression.py:398-401
    }
    for (int i = 0; i < P; ++i) {
        if (!std::isfinite(fb->out_host[1 + i])) {
            set_error("feedback: weights diverged");
            return SSW_ERR_NUMERIC;
        }
        w_inout[i] = fb->out_host[1 + i];
    }
    if (out_iters) *out_iters = counts[0];
    if (out_evals) *out_evals = counts[1];
    if (out_final_loss) *out_final_loss = (float)fb->loss_host[0];
    return SSW_OK;
}

// ---- S sessions' fits in one launch (k_fb_fit_wg_batch): the lead engine's argument and start-vector tables
ssw_status fb_batch_reserve(ssw_fb *fb, int nfit) {
    if (nfit <= fb->batch_cap) return SSW_OK;
    SSW_HIP_TRY(hipStreamSynchronize(fb->stream));
    (void)hipFree(fb->batch_tab);
    (void)hipFree(fb->batch_w);
    fb->batch_tab = nullptr;
    fb->batch_w = nullptr;
    fb->batch_cap = 0;
    int cap = 16;
    while (cap < nfit) cap <<= 1;
    SSW_HIP_TRY(hipMalloc((void **)&fb->batch_tab, (size_t)cap * sizeof(FitWgArgs)));
    SSW_HIP_TRY(hipMalloc((void **)&fb->batch_w, (size_t)cap * (fb->dim + 1) * sizeof(float)));
    fb->batch_cap = cap;
    return SSW_OK;
}

// ---- the two-output fit's host side (ssw_fb_fit2_batch) ------------------------------------------
bool fb_fit2_wg_eligible(const ssw_fb *fb) {
    return fb->n <= FIT_WG_MAX_ROWS && 2 * fb->dim <= 1024 && !getenv("SSW_FB_HOST_DRIVER");
}

// the arguments of one k_fb_fit2_wg workgroup; takes the engine's next sequence number.  w0_dev: [2 dim] on the device
void fb_fit2_wg_fill(ssw_fb *fb, float l_norm, float l_query, int max_iter, float lr, const float *w0_dev, FitWgArgs *out) {
    FitWgArgs a;
    memset(&a, 0, sizeof(a));
    a.X = fb->X; a.y = fb->y2; a.coef = fb->sw2;
    a.qhat = fb->qhat;
    a.w0_or_null = w0_dev;
    a.hist_dirs = fb->hist;
    a.hist_stps = fb->hist + (size_t)FIT_HISTORY * 1024;
    a.out_w = fb->out_host_dev + 1;
    a.out_loss = fb->loss_host_dev;
    a.out_counts = reinterpret_cast<int *>(fb->flag_host_dev) + 4;
    a.done_flag = fb->flag_host_dev;
    a.seqno = ++fb->seqno;
    a.n = (int)fb->n; a.dim2 = fb->dim; a.plane2 = (int)fb->cap2;
    a.dim = 2 * fb->dim - 1; a.P = 2 * fb->dim;  // the driver step's view: 2 dim parameters, none unused
    a.max_iter = max_iter; a.lr = lr;
    a.obj.l_norm = l_norm; a.obj.l_query = l_query;
    *out = a;
}

ssw_status fb_fit2_wg_launch(ssw_fb *lead, const FitWgArgs *tab_host, int nwg) {
    static bool attr_done[64][2] = {};
    const bool batch = nwg > 1;
    const void *kern = batch ? reinterpret_cast<const void *>(k_fb_fit2_wg_batch) : reinterpret_cast<const void *>(k_fb_fit2_wg);
    const int dslot = lead->device >= 0 && lead->device < 64 ? lead->device : -1;
    if (dslot < 0 || !attr_done[dslot][batch]) {
        SSW_HIP_TRY(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        if (dslot >= 0) attr_done[dslot][batch] = true;
    }
    if (batch)
        hipLaunchKernelGGL(k_fb_fit2_wg_batch, dim3(nwg), dim3(1024), FIT2_LDS_BYTES, lead->stream, (const FitWgArgs *)lead->batch_tab);
    else
        hipLaunchKernelGGL(k_fb_fit2_wg, dim3(1), dim3(1024), FIT2_LDS_BYTES, lead->stream, tab_host[0]);
    SSW_HIP_TRY(hipGetLastError());
    return SSW_OK;
}

}  // namespace ssw

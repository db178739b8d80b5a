// prune.hip -- certified int8 pre-scan for the exact top-k of a large f32 index (gfx950 / MI355X)
//
// The f32 scan (scan.hip) streams dim*4 bytes a row and is HBM-bound.  An exact top-k needs the exact score of only a
// few rows: the ones that can still reach the k-th image.  This file keeps an int8 SHADOW of every row (dim bytes, plus
// a scale s_r and an error constant a_r) and scans it instead.  For a query q with ||q|| <= Q the shadow score
// s~_r = s_r * sum_i c_ri q_i satisfies
//
//     | S_r - s~_r | <= a_r * Q + PAD_ABS                                                                    (*)
//
// where S_r is the BITS the f32 scan computes for row r (any summation order of dim products: the bound is the
// standard gamma_dim one, DESIGN.md section 4 derives it).  k_q8_bounds writes lb_r = s~_r - a_r Q - pad, rounded down,
// into the score buffer.  The caller (capi_index.hip, scan_for_topk) selects the k-th image over those lower bounds
// (threshold T <= the exact k-th image score), keeps the rows whose upper bound reaches T (k_survivors), rescores them
// with the f32 scan's own arithmetic (score_rows_kernel) and scatters the exact scores back (k_scatter_scores).  The
// normal selection over that buffer then returns the bits of a full scan.
//
// Shadow layout: natural row order, natural element order, one signed byte per element (c = rint(x / s), |c| <= 127,
// s = max|x| / 127).  A 16-byte load of lane l covers bytes 16 (l % L) .. +15 of one row, L = dim / 16 lanes a row:
// at dim 512 one wave-instruction reads two rows (1 KiB).  Rows that cannot be bounded (a non-finite element, a scale
// outside [2^-60, 2^60] / 127) get c = 0, s = 0 and a = +inf: their upper bound is +inf, so they are always rescored.
#include <algorithm>
#include <cmath>

#include "ssw_common.h"

namespace ssw {

namespace {

constexpr int Q8_GROUP_LOADS = 8;      // 16-byte loads a lane keeps in flight per group (8 KiB a wave)
constexpr double PAD_ABS = 0x1p-100;   // covers underflow of both computations (dim + 16 roundings at 2^-126 each)
constexpr double SAFETY = 1.0 + 0x1p-10;  // explicit factor on every a_r (covers the double-precision sums and sqrt)
constexpr float MAX_ABS = 0x1p60f, MIN_ABS = 0x1p-60f;  // a row's max |x| outside this range is not bounded
constexpr float MAX_QNORM = 0x1p40f;  // ... nor a query above this norm (|S| < 2^104 keeps every partial sum finite),
                                      // nor the zero query (k_q8_query)

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) v += __shfl_xor(v, off, 64);
    return v;
}

template <int C>
__device__ __forceinline__ void q8_build_row(const float *__restrict__ X, int64_t r, int lane, int8_t *__restrict__ codes,
                                             float *__restrict__ scale, float *__restrict__ err) {
    constexpr int dim = 256 * C;
    const float4 *src = reinterpret_cast<const float4 *>(X + r * dim) + lane * C;
    float x[4 * C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float4 v = src[c];
        x[4 * c] = v.x;
        x[4 * c + 1] = v.y;
        x[4 * c + 2] = v.z;
        x[4 * c + 3] = v.w;
    }
    float m = 0.0f;
    bool finite = true;
#pragma unroll
    for (int i = 0; i < 4 * C; ++i) {
        finite = finite && isfinite(x[i]);
        m = fmaxf(m, fabsf(x[i]));
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    const bool ok = __all(finite) && (m == 0.0f || (m >= MIN_ABS && m <= MAX_ABS));
    const float s = (ok && m > 0.0f) ? m / 127.0f : 0.0f;
    double e2 = 0.0, x2 = 0.0, c2 = 0.0;
    unsigned packed[C];
#pragma unroll
    for (int c = 0; c < C; ++c) packed[c] = 0u;
#pragma unroll
    for (int i = 0; i < 4 * C; ++i) {
        float q = s > 0.0f ? rintf(x[i] / s) : 0.0f;
        q = fminf(fmaxf(q, -127.0f), 127.0f);
        const int ci = (int)q;
        packed[i >> 2] |= ((unsigned)ci & 0xffu) << (8 * (i & 3));
        // x~_i = s * c_i is exact in double; so is its difference to x_i
        const double d = (double)x[i] - (double)s * (double)ci;
        e2 += d * d;
        if (ok) x2 += (double)x[i] * (double)x[i];
        c2 += (double)ci * (double)ci;
    }
    unsigned *dst = reinterpret_cast<unsigned *>(codes + r * dim) + lane * C;
#pragma unroll
    for (int c = 0; c < C; ++c) dst[c] = packed[c];
    e2 = wave_sum_d(e2);
    x2 = wave_sum_d(x2);
    c2 = wave_sum_d(c2);
    if (lane == 0) {
        // gamma_dim = dim u / (1 - dim u), u = 2^-24: any summation of dim products in f32 (both scans)
        const double g = (double)dim * 0x1p-24 / (1.0 - (double)dim * 0x1p-24);
        const double a = SAFETY * (sqrt(e2) + g * sqrt(x2) + g * (double)s * sqrt(c2));
        scale[r] = s;
        err[r] = ok ? __double2float_ru(a) : INFINITY;
    }
}

// one wave per row (grid-strided: the grid stays far below 2^32 threads); lane l converts the 4C elements
// 4C*l .. 4C*l + 4C - 1 (natural order, C = dim / 256)
template <int C>
__global__ __launch_bounds__(256) void k_q8_build(const float *__restrict__ X, int64_t n, int8_t *__restrict__ codes,
                                                  float *__restrict__ scale, float *__restrict__ err) {
    const int lane = threadIdx.x & 63;
    for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < n; r += (int64_t)gridDim.x * 4)
        q8_build_row<C>(X, r, lane, codes, scale, err);
}

// ||q|| rounded up (Q), the validity of the query for the bound, the survivor counter reset, and the query copied into
// the index's own buffer (the score buffer's materialisation rescans with it).  One block of 256 threads.
// state: [0] survivors, [1] the query's Q as float bits, [2] 1 = the query cannot be bounded
__global__ __launch_bounds__(256) void k_q8_query(const float *__restrict__ q, int dim, float *__restrict__ q_keep,
                                                  unsigned *__restrict__ state) {
    __shared__ double part[4];
    double s = 0.0;
    bool finite = true;
    for (int i = threadIdx.x; i < dim; i += 256) {
        const float v = q[i];
        q_keep[i] = v;
        finite = finite && isfinite(v);
        s += (double)v * (double)v;
    }
    s = wave_sum_d(s);
    const bool all_finite = __syncthreads_and(finite);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        const double t = part[0] + part[1] + part[2] + part[3];
        const float Q = __double2float_ru(sqrt(t) * (1.0 + 0x1p-40));
        // the zero query bounds nothing (every score is +-0 or NaN) and a * Q = inf * 0 would make the lower bound of an
        // unbounded row NaN: as the k-th key that is a threshold no upper bound is below, so every row would survive
        const bool bad = !all_finite || !(Q <= MAX_QNORM) || Q == 0.0f;
        state[0] = 0u;
        state[1] = __float_as_uint(Q);
        state[2] = bad ? 1u : 0u;
    }
}

// the shadow scan: lb_r into scores[r] for every row.  C = dim / 256; L = 16 C lanes a row, 4 / C rows per
// wave-instruction; a wave walks groups of Q8_GROUP_LOADS wave-instructions (double-buffered), grid-strided.
template <int C>
__global__ __launch_bounds__(256) void k_q8_bounds(const int8_t *__restrict__ codes, const float *__restrict__ scale,
                                                   const float *__restrict__ err, const float *__restrict__ q,
                                                   const unsigned *__restrict__ state, float *__restrict__ scores,
                                                   int64_t n) {
    constexpr int L = 16 * C, RPL = 4 / C, U = Q8_GROUP_LOADS, G = U * RPL;  // G rows a group
    const int lane = threadIdx.x & 63;
    const int seg = lane / L, j = lane % L;
    const int64_t gwave = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t nwaves = (int64_t)gridDim.x * 4;
    const int64_t ngroups = (n + G - 1) / G;
    if (gwave >= ngroups) return;
    const int64_t last = n - 1;
    const double Qd = (double)__uint_as_float(state[1]);
    float qv[16];
#pragma unroll
    for (int t = 0; t < 16; t += 4) {
        const float4 v = reinterpret_cast<const float4 *>(q)[(16 * j + t) >> 2];
        qv[t] = v.x;
        qv[t + 1] = v.y;
        qv[t + 2] = v.z;
        qv[t + 3] = v.w;
    }
    u32x4 cur[U], nxt[U];
    auto load = [&](u32x4(&dst)[U], int64_t g) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t row = min(g * G + u * RPL + seg, last);
            dst[u] = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(codes + row * (256 * C)) + j);
        }
    };
    load(cur, gwave);
    for (int64_t g = gwave; g < ngroups; g += nwaves) {
        const int64_t gn = g + nwaves < ngroups ? g + nwaves : g;  // no next group: re-touch own rows
        load(nxt, gn);
        // this group's per-row constants: lane i < G holds row g*G + i
        const int64_t my_row = g * G + lane;
        float s_r = 0.0f, a_r = 0.0f;
        if (lane < G && my_row < n) {
            s_r = scale[my_row];
            a_r = err[my_row];
        }
        float acc[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const unsigned w[4] = {cur[u].x, cur[u].y, cur[u].z, cur[u].w};
            float a = 0.0f;
#pragma unroll
            for (int t = 0; t < 16; ++t) a = fmaf((float)(int)(int8_t)(w[t >> 2] >> (8 * (t & 3))), qv[t], a);
#pragma unroll
            for (int off = 1; off < L; off <<= 1) a += __shfl_xor(a, off, 64);
            acc[u] = a;
        }
        // lane i < G takes row i of the group: load u = i / RPL, segment i % RPL
        float mine = 0.0f;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const float v = __shfl(acc[u], (lane % RPL) * L, 64);
            mine = (lane / RPL == u) ? v : mine;
        }
        if (lane < G && my_row < n) {
            // s * A and a * Q are exact in double; the subtraction's rounding is covered by the relative pad
            double lb = (double)s_r * (double)mine - (double)a_r * Qd;
            lb -= fabs(lb) * 0x1p-50 + PAD_ABS;
            scores[my_row] = __double2float_rd(lb);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) cur[u] = nxt[u];
    }
}

// the rows whose upper bound reaches T = the k-th key of the threshold selection over the lower bounds.
// ub_r <= lb_r + 2 a_r Q + pads, so a row with lb + 2 a Q + pads < T is proven below the exact k-th image score.
// Nothing is collected when the selection returned fewer than k keys or overflowed, or the query cannot be bounded:
// the survivor count is then left at 0 and prune_publish reports the fallback.
__global__ __launch_bounds__(256) void k_survivors(const float *__restrict__ lb, const float *__restrict__ err,
                                                   int64_t n, const uint64_t *__restrict__ keys,
                                                   const int32_t *__restrict__ sel_count, int32_t k,
                                                   unsigned *__restrict__ state, int64_t *__restrict__ rows,
                                                   int64_t cap) {
    if (sel_count[0] < k || sel_count[1] != 0 || state[2] != 0u) return;
    const float T = ord_to_f32((uint32_t)(keys[k - 1] >> 32));
    const double Qd = (double)__uint_as_float(state[1]);
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t base = (int64_t)blockIdx.x * 256 + (threadIdx.x & ~63u); base < n; base += stride) {  // wave-uniform
        const int64_t r = base + lane;
        bool keep = false;
        if (r < n) {
            const double l = (double)lb[r], w = (double)err[r] * Qd;
            const double ub = l + 2.0 * w + (fabs(l) + w) * 0x1p-20 + 2.0 * PAD_ABS;
            keep = !(ub < (double)T);  // NaN survives
        }
        const uint64_t ballot = __ballot(keep);
        if (ballot == 0ull) continue;
        unsigned slot0 = 0u;
        if (lane == __builtin_ctzll(ballot)) slot0 = atomicAdd(&state[0], (unsigned)__popcll(ballot));
        slot0 = __shfl(slot0, __builtin_ctzll(ballot), 64);
        if (keep) {
            const int64_t at = (int64_t)slot0 + __popcll(ballot & ((1ull << lane) - 1ull));
            if (at < cap) rows[at] = r;
        }
    }
}

// the host's answer: survivors (0 .. cap) or -1 = fall back to the full scan; released into pinned memory under seq
__global__ void k_prune_publish(const int32_t *__restrict__ sel_count, int32_t k, const unsigned *__restrict__ state,
                                int64_t cap, int32_t *__restrict__ host_block, unsigned seq) {
    if (threadIdx.x != 0) return;
    const bool fall = sel_count[0] < k || sel_count[1] != 0 || state[2] != 0u || (int64_t)state[0] > cap;
    host_block[1] = fall ? -1 : (int32_t)state[0];
    __threadfence_system();
    __hip_atomic_store(reinterpret_cast<unsigned *>(host_block), seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

__global__ __launch_bounds__(256) void k_scatter_scores(const int64_t *__restrict__ rows, const float *__restrict__ v,
                                                        int64_t m, float *__restrict__ scores) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < m) scores[rows[i]] = v[i];
}

}  // namespace

bool q8_dim_supported(int32_t dim) { return dim == 256 || dim == 512 || dim == 1024; }

ssw_status launch_q8_build(const float *X, int64_t n, int32_t dim, int8_t *codes, float *scale, float *err,
                           hipStream_t stream) {
    if (n <= 0) return SSW_OK;
    const dim3 grid((unsigned)std::min<int64_t>((n + 3) / 4, (int64_t)1 << 20)), block(256);
    switch (dim) {
        case 256: hipLaunchKernelGGL(k_q8_build<1>, grid, block, 0, stream, X, n, codes, scale, err); break;
        case 512: hipLaunchKernelGGL(k_q8_build<2>, grid, block, 0, stream, X, n, codes, scale, err); break;
        case 1024: hipLaunchKernelGGL(k_q8_build<4>, grid, block, 0, stream, X, n, codes, scale, err); break;
        default:
            set_error("q8_build: dim=%d unsupported", dim);
            return SSW_ERR_UNSUPPORTED;
    }
    SSW_HIP_TRY(hipGetLastError());
    return SSW_OK;
}

ssw_status launch_q8_query(const float *q_dev, int32_t dim, float *q_keep, unsigned *state, hipStream_t stream) {
    hipLaunchKernelGGL(k_q8_query, dim3(1), dim3(256), 0, stream, q_dev, (int)dim, q_keep, state);
    SSW_HIP_TRY(hipGetLastError());
    return SSW_OK;
}

ssw_status launch_q8_bounds(const int8_t *codes, const float *scale, const float *err, const float *q_dev,
                            const unsigned *state, float *scores, int64_t n, int32_t dim, int device,
                            hipStream_t stream) {
    if (n <= 0) return SSW_OK;
    const int C = dim / 256;
    const int64_t rows_per_group = (int64_t)Q8_GROUP_LOADS * (4 / C);
    const int64_t need = ((n + rows_per_group - 1) / rows_per_group + 3) / 4;
    int64_t grid = (int64_t)num_cus(device) * 2;  // two 4-wave blocks per CU
    if (grid > need) grid = need;
    if (grid < 1) grid = 1;
    switch (dim) {
        case 256:
            hipLaunchKernelGGL(k_q8_bounds<1>, dim3((unsigned)grid), dim3(256), 0, stream, codes, scale, err, q_dev, state,
                               scores, n);
            break;
        case 512:
            hipLaunchKernelGGL(k_q8_bounds<2>, dim3((unsigned)grid), dim3(256), 0, stream, codes, scale, err, q_dev, state,
                               scores, n);
            break;
        case 1024:
            hipLaunchKernelGGL(k_q8_bounds<4>, dim3((unsigned)grid), dim3(256), 0, stream, codes, scale, err, q_dev, state,
                               scores, n);
            break;
        default:
            set_error("q8_bounds: dim=%d unsupported", dim);
            return SSW_ERR_UNSUPPORTED;
    }
    SSW_HIP_TRY(hipGetLastError());
    return SSW_OK;
}

ssw_status launch_survivors(const float *lb, const float *err, int64_t n, const uint64_t *keys, const int32_t *sel_count,
                            int32_t k, unsigned *state, int64_t *rows, int64_t cap, int32_t *host_block, unsigned seq,
                            int device, hipStream_t stream) {
    int64_t grid = (int64_t)num_cus(device) * 4;
    const int64_t need = (n + 255) / 256;
    if (grid > need) grid = need;
    if (grid < 1) grid = 1;
    hipLaunchKernelGGL(k_survivors, dim3((unsigned)grid), dim3(256), 0, stream, lb, err, n, keys, sel_count, k, state,
                       rows, cap);
    hipLaunchKernelGGL(k_prune_publish, dim3(1), dim3(64), 0, stream, sel_count, k, state, cap, host_block, seq);
    SSW_HIP_TRY(hipGetLastError());
    return SSW_OK;
}

ssw_status launch_scatter_scores(const int64_t *rows, const float *v, int64_t m, float *scores, hipStream_t stream) {
    if (m <= 0) return SSW_OK;
    hipLaunchKernelGGL(k_scatter_scores, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, stream, rows, v, m, scores);
    SSW_HIP_TRY(hipGetLastError());
    return SSW_OK;
}

}  // namespace ssw

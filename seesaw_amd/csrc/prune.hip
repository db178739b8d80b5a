// prune.hip -- certified int8 pre-scan for the exact top-k of a large f32 or f16 index (gfx950 / MI355X)
//
// The f32 scan (scan.hip) streams dim*4 bytes a row and is HBM-bound.  An exact top-k needs the exact score of only a
// few rows: the ones that can still reach the k-th image.  This file keeps an int8 SHADOW of every row (dim bytes, plus
// a scale s_r and an error constant a_r) and scans it instead.  For a query q with ||q|| <= Q the shadow score
// s~_r = s_r * sum_i c_ri q_i satisfies
//
//     | S_r - s~_r | <= a_r * Q + PAD_ABS                                                                    (*)
//
// where S_r is the BITS the f32 scan computes for row r (any summation order of dim products: the bound is the
// standard gamma_dim one, DESIGN.md section 4 derives it).  For an f16 index the rows x are the widened binary16 rows:
// widening is exact and the f16 scan returns the f32 scan's bits on them, so the same statement holds unchanged.
// k_q8_bounds writes lb_r = s~_r - a_r Q - pad, rounded down, into the score buffer.  The caller (capi_index.hip, scan_for_topk) selects the k-th image over those lower bounds
// (threshold T <= the exact k-th image score), keeps the rows whose upper bound reaches T (k_survivors), rescores them
// with the f32 scan's own arithmetic (score_rows_kernel) and scatters the exact scores back (k_scatter_scores).  The
// normal selection over that buffer then returns the bits of a full scan (on an index without an image map it runs over
// the survivors at or above T alone: select.hip, k_scatter_candidates).
//
// Shadow layout: natural row order, natural element order, one signed byte per element (c = rint(x / s), |c| <= 127,
// s = max|x| / 127).  A 16-byte load of lane l covers bytes 16 (l % L) .. +15 of one row, L = dim / 16 lanes a row:
// at dim 512 one wave-instruction reads two rows (1 KiB).  Rows that cannot be bounded (a non-finite element, a scale
// outside [2^-60, 2^60] / 127) get c = 0, s = 0 and a = +inf: their upper bound is +inf, so they are always rescored.
#include <algorithm>
#include <cmath>
#include <type_traits>

#include "ssw_common.h"

namespace ssw {

namespace {

constexpr int Q8_GROUP_LOADS = 8;      // 16-byte loads a lane keeps in flight per group (8 KiB a wave)
constexpr int Q8_BLOCKS_PER_CU = 1;    // four-wave blocks of the shadow scan per CU (one wave a SIMD)
// tuning hooks (ssw_tune_prune_scan, lab build only): group loads 4 / 8 / 16, blocks per CU 1 .. 8
SSW_TUNABLE int g_q8_group_loads = Q8_GROUP_LOADS;
SSW_TUNABLE int g_q8_blocks_per_cu = Q8_BLOCKS_PER_CU;
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

// The part of a row's conversion both builders share: the lane's 4C elements x (any fixed assignment of the row's
// elements to lanes and slots) -> their codes, slot i in byte i % 4 of packed[i / 4], and the row's s_r and a_r, which
// lane 0 writes.  The codes and s_r do not depend on the assignment; a_r's double sums are taken in its order.
// LEVELS: the largest |code|, 127 for the int8 shadow, 31 for the packed 6-bit one (k_q6_build).
// s_out / ok_out (k_q41_build only, else NULL): the row's s_r and whether the row can be bounded, in every lane.
template <int C, int LEVELS = 127>
__device__ __forceinline__ void q8_quantise_row(const float (&x)[4 * C], int64_t r, int lane, unsigned (&packed)[C],
                                                float *__restrict__ scale, float *__restrict__ err,
                                                float *s_out = nullptr, bool *ok_out = nullptr) {
    constexpr int dim = 256 * C;
    constexpr float LV = (float)LEVELS;
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
    const float s = (ok && m > 0.0f) ? m / LV : 0.0f;
    if (s_out) *s_out = s;
    if (ok_out) *ok_out = ok;
    double e2 = 0.0, x2 = 0.0, c2 = 0.0;
#pragma unroll
    for (int c = 0; c < C; ++c) packed[c] = 0u;
#pragma unroll
    for (int i = 0; i < 4 * C; ++i) {
        float q = s > 0.0f ? rintf(x[i] / s) : 0.0f;
        q = fminf(fmaxf(q, -LV), LV);
        const int ci = (int)q;
        packed[i >> 2] |= ((unsigned)ci & 0xffu) << (8 * (i & 3));
        // x~_i = s * c_i is exact in double; so is its difference to x_i
        const double d = (double)x[i] - (double)s * (double)ci;
        e2 += d * d;
        if (ok) x2 += (double)x[i] * (double)x[i];
        c2 += (double)ci * (double)ci;
    }
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

// f32 rows: lane l converts the 4C elements 4C*l .. 4C*l + 4C - 1 (natural order, C = dim / 256)
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
    unsigned packed[C];
    q8_quantise_row<C>(x, r, lane, packed, scale, err);
    unsigned *dst = reinterpret_cast<unsigned *>(codes + r * dim) + lane * C;
#pragma unroll
    for (int c = 0; c < C; ++c) dst[c] = packed[c];
}

// binary16 rows in the f16 index's lane-interleaved layout (ssw_common.h): lane l reads its 8C contiguous bytes at
// l * 8C of the row (one 16-byte load at dim 512, two at dim 1024, 8 bytes at dim 256, three 8-byte loads at dim 768,
// which only the 6-bit builder instantiates) and widens them, exactly; chunk c
// of them, x[4c .. 4c + 3], is the natural elements 256c + 4l .. + 3.
template <int C>
__device__ __forceinline__ void load_row_h16(const uint16_t *__restrict__ X, int64_t r, int lane, float (&x)[4 * C]) {
    constexpr int dim = 256 * C;
    const u32x2 *src = reinterpret_cast<const u32x2 *>(X + r * dim) + lane * C;
    u32x2 w[C];
    if constexpr (C % 2 != 0) {
        // a lane's 8C bytes are only 8-byte aligned (24 at dim 768): one 8-byte load a chunk, as H16Rows::load (scan.hip)
#pragma unroll
        for (int c = 0; c < C; ++c) w[c] = src[c];
    } else {
#pragma unroll
        for (int c = 0; c < C; c += 2) {
            const u32x4 v = *reinterpret_cast<const u32x4 *>(src + c);
            w[c] = u32x2{v.x, v.y};
            w[c + 1] = u32x2{v.z, v.w};
        }
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float4 v = widen_h16x4(w[c]);
        x[4 * c] = v.x;
        x[4 * c + 1] = v.y;
        x[4 * c + 2] = v.z;
        x[4 * c + 3] = v.w;
    }
}

// binary16 rows: the four codes of chunk c are the 4 bytes at 256c + 4l of the row's code line: a wave writes 256
// contiguous bytes a chunk, and the shadow is in natural element order as for f32 rows.
template <int C>
__device__ __forceinline__ void q8_build_row_h16(const uint16_t *__restrict__ X, int64_t r, int lane,
                                                 int8_t *__restrict__ codes, float *__restrict__ scale,
                                                 float *__restrict__ err) {
    constexpr int dim = 256 * C;
    float x[4 * C];
    load_row_h16<C>(X, r, lane, x);
    unsigned packed[C];
    q8_quantise_row<C>(x, r, lane, packed, scale, err);
    unsigned *dst = reinterpret_cast<unsigned *>(codes + r * dim) + lane;
#pragma unroll
    for (int c = 0; c < C; ++c) dst[64 * c] = packed[c];
}

// one wave per row (grid-strided: the grid stays far below 2^32 threads)
template <int C>
__global__ __launch_bounds__(256) void k_q8_build(const float *__restrict__ X, int64_t n, int8_t *__restrict__ codes,
                                                  float *__restrict__ scale, float *__restrict__ err) {
    const int lane = threadIdx.x & 63;
    for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < n; r += (int64_t)gridDim.x * 4)
        q8_build_row<C>(X, r, lane, codes, scale, err);
}

template <int C>
__global__ __launch_bounds__(256) void k_q8_build_h16(const uint16_t *__restrict__ X, int64_t n,
                                                      int8_t *__restrict__ codes, float *__restrict__ scale,
                                                      float *__restrict__ err) {
    const int lane = threadIdx.x & 63;
    for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < n; r += (int64_t)gridDim.x * 4)
        q8_build_row_h16<C>(X, r, lane, codes, scale, err);
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

// v of the lane whose index differs by the DPP control: quad_perm [1,0,3,2] (lane ^ 1), quad_perm [2,3,0,1] (lane ^ 2),
// row_half_mirror (lane ^ 7) and row_ror:8 (lane ^ 8).  One VALU instruction each, where __shfl_xor goes through the LDS
// crossbar (ds_bpermute_b32) and needs an address register.
constexpr int DPP_XOR1 = 0xB1, DPP_XOR2 = 0x4E, DPP_XOR7 = 0x141, DPP_XOR8 = 0x128;
template <int CTRL>
__device__ __forceinline__ float dpp(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, true));
}

// v of lane ^ (1 << BIT) (lane ^ 7 for BIT 2: see q8_group_reduce)
template <int BIT>
__device__ __forceinline__ float q8_partner(float v) {
    if constexpr (BIT == 0) return dpp<DPP_XOR1>(v);
    else if constexpr (BIT == 1) return dpp<DPP_XOR2>(v);
    else if constexpr (BIT == 2) return dpp<DPP_XOR7>(v);
    else if constexpr (BIT == 3) return dpp<DPP_XOR8>(v);
    else return __shfl_xor(v, 1 << BIT, 64);
}

// one transposing step over lane bit BIT: the H pairs (acc[i], acc[i + H]) become acc[i] = own + partner's of the half
// the lane's bit selects, so H values are left; then the steps below it
template <int BIT, int H>
__device__ __forceinline__ void q8_fold(float *acc, int j) {
    const bool upper = (j >> BIT) & 1;
#pragma unroll
    for (int i = 0; i < H; ++i) {
        const float keep = upper ? acc[i + H] : acc[i];
        const float send = upper ? acc[i] : acc[i + H];
        acc[i] = keep + q8_partner<BIT>(send);
    }
    if constexpr (H > 1) q8_fold<BIT - 1, H / 2>(acc, j);
}

// Sums the U accumulators of a group over the L lanes of a row together: log2 U transposing steps from lane bit
// log2 U - 1 down to bit 0 (U - 1 exchanges in all), then one value over the remaining lane bits: lane j of a row's L
// lanes ends with the whole sum of load j % U.  Bit 2's partner is lane ^ 7, not lane ^ 4 (DPP has no xor 4): both lanes
// of that pair still hold all values of the bits below, which are folded afterwards, so every lane is still counted once.
template <int U, int L>
__device__ __forceinline__ float q8_group_reduce(float (&acc)[U], int j) {
    static_assert(U == 4 || U == 8 || U == 16, "loads a group");
    constexpr int TOP = U == 4 ? 1 : U == 8 ? 2 : 3;
    q8_fold<TOP, U / 2>(acc, j);
    float v = acc[0];
    // lanes now differ in what they hold by their bits below log2 U: from here on plain xor partners only
    if constexpr (U <= 4 && L > 4) v += __shfl_xor(v, 4, 64);
    if constexpr (U <= 8 && L > 8) v += dpp<DPP_XOR8>(v);
#pragma unroll
    for (int off = 16; off < L; off <<= 1) v += __shfl_xor(v, off, 64);
    return v;
}

typedef float f32x2 __attribute__((ext_vector_type(2)));

// the shadow scan: lb_r into scores[r] for every row.  C = dim / 256; L = 16 C lanes a row, RPL = 4 / C rows per
// wave-instruction (1 KiB at every dim); a wave walks the full groups of U wave-instructions, grid-strided.  Two
// register sets (a, b) take turns: while one group is multiplied the next group's codes AND its rows' constants are in
// flight, so the only waits inside the loop are counted ones for the group that was requested an iteration earlier.
// Lane j < U of row segment `seg` owns row j * RPL + seg of its group: it loads that row's s_r and a_r and writes its
// bound.  The loop has one exit and no branch around a request: a path with fewer loads outstanding would make the
// compiler's wait counts conservative on every path.  The last n % G rows are one clamped group of their own, after
// the loop, for one wave.
template <int C, int U>
__global__ __launch_bounds__(256) void k_q8_bounds(const int8_t *__restrict__ codes, const float *__restrict__ scale,
                                                   const float *__restrict__ err, const float *__restrict__ q,
                                                   const unsigned *__restrict__ state, float *__restrict__ scores,
                                                   int64_t n) {
    constexpr int L = 16 * C, RPL = 4 / C, G = U * RPL;  // G rows a group
    constexpr unsigned LOAD_BYTES = 1024;               // RPL rows of 256 C bytes
    const int lane = threadIdx.x & 63;
    const int seg = lane / L, j = lane % L;
    const int64_t gwave = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t nwaves = (int64_t)gridDim.x * 4;
    const int64_t nfull = n / G;       // groups of G rows
    const int ragged = (int)(n % G);   // rows of the group after them
    const double Qd = (double)__uint_as_float(state[1]);
    f32x2 qv[8];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const float4 v = reinterpret_cast<const float4 *>(q)[4 * j + t];
        qv[2 * t] = f32x2{v.x, v.y};
        qv[2 * t + 1] = f32x2{v.z, v.w};
    }
    const unsigned lane_byte = (unsigned)(seg * 256 * C + 16 * j);  // of this lane's 16 codes in a wave-instruction
    const int mine = (j % U) * RPL + seg;                           // the group row this lane holds the constants of
    struct Set {
        u32x4 c[U];
        float s, a;
    };
    // all requests of a full group: U code loads and the two constants (every lane loads them: lanes j >= U those of
    // lane j % U, the same cache line)
    auto load = [&](Set &d, int64_t g) {
        const int8_t *base = codes + g * (int64_t)(G * 256 * C);  // wave-uniform
#pragma unroll
        for (int u = 0; u < U; ++u)
            d.c[u] = __builtin_nontemporal_load(
                reinterpret_cast<const u32x4 *>(base + (lane_byte + (unsigned)u * LOAD_BYTES)));
        d.s = (scale + g * G)[mine];
        d.a = (err + g * G)[mine];
        // left alone the scheduler sinks these requests into the multiplies that follow, to reuse the registers of
        // the set being consumed: the next group would be requested half a group late
        __builtin_amdgcn_sched_barrier(0);
    };
    // the bounds of the first `rows` rows of group g from a set that has arrived
    auto bounds = [&](const Set &d, int64_t g, int rows) {
        float acc[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const unsigned w[4] = {d.c[u].x, d.c[u].y, d.c[u].z, d.c[u].w};
            f32x2 a2 = {0.0f, 0.0f};  // even and odd elements: the order of the dim products is free
#pragma unroll
            for (int t = 0; t < 16; t += 2) {
                const f32x2 c2 = {(float)(int)(int8_t)(w[t >> 2] >> (8 * (t & 3))),
                                  (float)(int)(int8_t)(w[t >> 2] >> (8 * ((t + 1) & 3)))};
                a2 = __builtin_elementwise_fma(c2, qv[t >> 1], a2);
            }
            acc[u] = a2.x + a2.y;
        }
        const float A = q8_group_reduce<U, L>(acc, j);
        if (j < U && mine < rows) {
            // s * A and a * Q are exact in double; the subtraction's rounding is covered by the relative pad
            double lb = (double)d.s * (double)A - (double)d.a * Qd;
            lb -= fabs(lb) * 0x1p-50 + PAD_ABS;
            (scores + g * G)[mine] = __double2float_rd(lb);
        }
    };
    if (gwave < nfull) {
        Set a, b;
        int64_t g = gwave;
        load(a, g);
        for (;;) {
            // a wave without a next group requests its last one once more (cache hits) and writes nothing for it
            const int64_t g1 = g + nwaves < nfull ? g + nwaves : g;
            load(b, g1);
            bounds(a, g, G);
            const int64_t g2 = g1 + nwaves < nfull ? g1 + nwaves : g1;
            load(a, g2);
            bounds(b, g1, g1 != g ? G : 0);
            if (g2 == g1) break;
            g = g2;
        }
    }
    if (ragged != 0 && gwave == nfull % nwaves) {
        Set t;
        const int8_t *base = codes + nfull * (int64_t)(G * 256 * C);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const unsigned row = (unsigned)min(u * RPL + seg, ragged - 1);  // nothing beyond row n - 1
            t.c[u] = *reinterpret_cast<const u32x4 *>(base + (row * (unsigned)(256 * C) + 16u * (unsigned)j));
        }
        t.s = (scale + nfull * G)[min(mine, ragged - 1)];
        t.a = (err + nfull * G)[min(mine, ragged - 1)];
        bounds(t, nfull, ragged);
    }
}

// ---- the shadow's maxima: what lets the survivor pass read the bounds alone ---------------------------------------------
// mx[0] = the largest finite a_r, mx[1] = the largest finite s_r of the shadow, as float bits (non-negative floats order as
// their bit patterns, so atomicMax on unsigned is a float maximum); the caller zeroes both words first.  Rows with
// a = +inf are left out: their lb is -inf, which the survivor pass keeps by a clause of its own.
__global__ __launch_bounds__(256) void k_shadow_max(const float *__restrict__ err, const float *__restrict__ scale, int64_t n,
                                                    unsigned *__restrict__ mx) {
    float a = 0.0f, s = 0.0f;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float e = err[i], c = scale[i];
        if (isfinite(e)) a = fmaxf(a, e);
        if (isfinite(c)) s = fmaxf(s, c);
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        a = fmaxf(a, __shfl_xor(a, off, 64));
        s = fmaxf(s, __shfl_xor(s, off, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        if (a > 0.0f) atomicMax(&mx[0], __float_as_uint(a));
        if (s > 0.0f) atomicMax(&mx[1], __float_as_uint(s));
    }
}

// the upper bound of a row from its lower bound l and the width w of its bound: ub_r <= l + 2 w + pads
__device__ __forceinline__ double surv_ub(double l, double w) {
    return l + 2.0 * w + (fabs(l) + w) * 0x1p-20 + 2.0 * PAD_ABS;
}

constexpr double WMAX_INFLATE = 1.0 + 0x1p-30;  // on w_max: a different fma contraction of the two ub's cannot matter
constexpr int SURV_UNROLL = 4;                  // 16-byte loads of lb a lane keeps in flight
constexpr int SURV_STAGE = 1024;                // survivors a block collects in LDS before it takes its place in the list
// FLUSH (survivor_pass): a block adds at most 4 waves x SURV_UNROLL steps x 256 rows between two looks at its stage, and
// the last n % 4 rows after the last look
constexpr int SURV_FLUSH_STAGE = SURV_STAGE + 4 * SURV_UNROLL * 256 + 4;

// The survivor pass of both kernels below: the rows with !(ub < T), their number added to *counter and the first cap of
// them listed in rows (any order).  MQ: the width is e wA + s wS ((**) / (***)), else e wA.
// Two steps.  A lane takes four consecutive rows and first loads their lb ONLY; with w_max >= every bounded row's w
// (from the shadow's maxima) surv_ub(l, w_max) >= surv_ub(l, w): the expression is monotone in w >= 0 under round to
// nearest.  So a row with ub_max < T and lb > -inf cannot pass the test and its constants are never read; lb = -inf
// (an unboundable row: a = +inf is not in the maxima) and a NaN bound stay candidates.  (The lb > -inf clause is
// redundant: surv_ub's (|l| + w) 2^-20 term is +inf at l = -inf, so ub_max is the NaN of -inf + inf there whatever
// w_max is, and !(NaN < T) holds.  It stays as a second line of defence should the ub expression ever change.)  A lane
// with a candidate loads its four rows' constants and applies the test itself, unchanged.
// The list: one atomicAdd with return on the one global counter per wave-step that found a survivor was most of the
// pass once the 6-bit shadow left ~22 000 survivors (that many dependent atomics on one address).  A block now collects
// its survivors in LDS (an LDS atomic a wave-step) and takes its place in the list once, at the end; a wave-step that
// no longer fits the stage goes to the global counter directly, as before, and so does every wave-step of the block
// after it (once a claim has failed the stage is closed).  Count and set are the same; only the order of the list,
// which was the atomics' already, differs.
// FLUSH (the first stage of the two-stage path, millions of survivors: a closed stage would leave most of the pass to
// atomics on the one global counter): the block looks at its stage before every round of SURV_UNROLL steps, all waves
// together, and once more than SURV_STAGE rows are staged it claims their place in the list with ONE global atomic,
// writes them out and starts the stage again.  The stage has room for a whole round beyond that mark, so no claim fails
// and nothing goes to the global counter directly.  Rows are 32-bit (Row = uint32_t), the list's type.
template <bool MQ, bool FLUSH = false, class Row = int64_t>
__device__ __forceinline__ void survivor_pass(const float *__restrict__ lb, const float *__restrict__ err,
                                              const float *__restrict__ scale, int64_t n, float T, double wA, double wS,
                                              double w_max, unsigned *__restrict__ counter, Row *__restrict__ rows,
                                              int64_t cap) {
    const int lane = threadIdx.x & 63;
    const uint64_t below = (1ull << lane) - 1ull;
    const int64_t stride = (int64_t)gridDim.x * 1024;
    const double Td = (double)T;
    __shared__ Row stage[FLUSH ? SURV_FLUSH_STAGE : SURV_STAGE];
    __shared__ unsigned staged, first_failed, stage_base;
    if (threadIdx.x == 0) staged = 0u, first_failed = 0xffffffffu;
    __syncthreads();
    // the lane's rows r0 .. r0 + nv - 1 with the bounds l (nv = 4, 0 for a lane without rows, or the last n % 4 rows);
    // called by whole waves
    auto step = [&](int64_t r0, const float (&l4)[4], int nv) {
        bool cand = false;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const double l = (double)l4[t];
            cand = cand || (t < nv && (!(surv_ub(l, w_max) < Td) || !(l4[t] > -INFINITY)));
        }
        if (__ballot(cand) == 0ull) return;
        float e4[4] = {0.0f, 0.0f, 0.0f, 0.0f}, s4[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (cand) {
            if (nv == 4) {
                const float4 ev = *reinterpret_cast<const float4 *>(err + r0);
                e4[0] = ev.x, e4[1] = ev.y, e4[2] = ev.z, e4[3] = ev.w;
                if constexpr (MQ) {
                    const float4 sv = *reinterpret_cast<const float4 *>(scale + r0);
                    s4[0] = sv.x, s4[1] = sv.y, s4[2] = sv.z, s4[3] = sv.w;
                }
            } else {
                for (int t = 0; t < nv; ++t) {
                    e4[t] = err[r0 + t];
                    if constexpr (MQ) s4[t] = scale[r0 + t];
                }
            }
        }
        bool keep[4];
        uint64_t ballot[4];
        unsigned total = 0u;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const double l = (double)l4[t];
            double w = (double)e4[t] * wA;
            if constexpr (MQ) w = (double)e4[t] * wA + (double)s4[t] * wS;
            keep[t] = cand && t < nv && !(surv_ub(l, w) < Td);  // NaN survives
            ballot[t] = __ballot(keep[t]);
            total += (unsigned)__popcll(ballot[t]);
        }
        if (total == 0u) return;
        // a place in the block's stage.  A claim is never undone: the first one that does not fit leaves `staged` above
        // SURV_STAGE, so every later claim fails too, and the claims that hold are exactly those below the smallest
        // failed slot, contiguous from 0 (claims only ever advance `staged`)
        unsigned slot = 0u;
        int direct = 0;
        if (lane == 0) {
            slot = atomicAdd(&staged, total);
            if constexpr (!FLUSH) {
                if (slot + total > (unsigned)SURV_STAGE) {
                    atomicMin(&first_failed, slot);
                    slot = atomicAdd(counter, total);
                    direct = 1;
                }
            }
        }
        slot = __shfl(slot, 0, 64);
        direct = __shfl(direct, 0, 64);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int64_t at = (int64_t)slot + __popcll(ballot[t] & below);
            if (keep[t]) {
                if (!direct) stage[at] = (Row)(r0 + t);
                else if (at < cap) rows[at] = (Row)(r0 + t);
            }
            slot += (unsigned)__popcll(ballot[t]);
        }
    };
    // the whole groups of four rows: a wave takes 256 rows a step, SURV_UNROLL steps a stride apart at a time, their loads
    // requested together (wave-uniform loop; no scalar path beside the loads, which would make the waits conservative)
    const int64_t n4 = n & ~(int64_t)3;
    // the staged rows into the list behind one claim on the global counter (whole block; FLUSH: the stage starts again)
    auto flush = [&](unsigned count) {
        if (threadIdx.x == 0) stage_base = atomicAdd(counter, count);
        __syncthreads();
        for (unsigned i = threadIdx.x; i < count; i += 256) {
            const int64_t at = (int64_t)stage_base + i;
            if (at < cap) rows[at] = stage[i];
        }
        if constexpr (FLUSH) {
            __syncthreads();
            if (threadIdx.x == 0) staged = 0u;
            __syncthreads();
        }
    };
    // FLUSH: the loop is the block's (wave 0's base decides), so that every wave reaches the barriers; a wave past the
    // rows has r0 >= n4 throughout and does nothing
    for (int64_t base0 = (int64_t)blockIdx.x * 1024 + (threadIdx.x & ~63u) * 4;
         base0 - (FLUSH ? (int64_t)((threadIdx.x & ~63u) * 4) : 0) < n4; base0 += SURV_UNROLL * stride) {
        if constexpr (FLUSH) {
            __syncthreads();
            const unsigned have = staged;  // (block-uniform: read between two barriers)
            __syncthreads();
            if (have > (unsigned)SURV_STAGE) flush(have);
        }
        float4 lv[SURV_UNROLL];
#pragma unroll
        for (int u = 0; u < SURV_UNROLL; ++u) {
            const int64_t r0 = base0 + u * stride + 4 * lane;
            lv[u] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (r0 < n4) lv[u] = *reinterpret_cast<const float4 *>(lb + r0);
        }
#pragma unroll
        for (int u = 0; u < SURV_UNROLL; ++u) {
            const int64_t r0 = base0 + u * stride + 4 * lane;
            const float l4[4] = {lv[u].x, lv[u].y, lv[u].z, lv[u].w};
            step(r0, l4, r0 < n4 ? 4 : 0);
        }
    }
    // the last n % 4 rows: lane 0 of the first wave
    if (n4 < n && blockIdx.x == 0 && threadIdx.x < 64) {
        float l4[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        const int nv = lane == 0 ? (int)(n - n4) : 0;
        for (int t = 0; t < nv; ++t) l4[t] = lb[n4 + t];
        step(n4, l4, nv);
    }
    // the block's staged survivors into the list, behind one claim on the global counter
    __syncthreads();
    const unsigned mine = min(staged, first_failed);  // <= SURV_STAGE: where the first claim that did not fit began
    if (mine == 0u) return;
    flush(mine);
}

// the rows whose upper bound reaches T = the k-th key of the threshold selection over the lower bounds.
// ub_r <= lb_r + 2 a_r Q + pads, so a row with lb + 2 a Q + pads < T is proven below the exact k-th image score.
// Nothing is collected when the selection returned fewer than k keys or overflowed, or the query cannot be bounded:
// the survivor count is then left at 0 and prune_publish reports the fallback.  mx: the shadow's maxima (k_shadow_max).
__global__ __launch_bounds__(256) void k_survivors(const float *__restrict__ lb, const float *__restrict__ err,
                                                   const unsigned *__restrict__ mx, int64_t n,
                                                   const uint64_t *__restrict__ keys,
                                                   const int32_t *__restrict__ sel_count, int32_t k,
                                                   unsigned *__restrict__ state, int64_t *__restrict__ rows,
                                                   int64_t cap) {
    if (sel_count[0] < k || sel_count[1] != 0 || state[2] != 0u) return;
    const float T = ord_to_f32((uint32_t)(keys[k - 1] >> 32));
    const double Qd = (double)__uint_as_float(state[1]);
    const double w_max = (double)__uint_as_float(mx[0]) * Qd * WMAX_INFLATE;
    survivor_pass<false>(lb, err, nullptr, n, T, Qd, 0.0, w_max, &state[0], rows, cap);
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

// ---- the pre-scan of a chunk of up to 16 queries on the int8 matrix core ("Pruned batch") -----
// The queries are quantised to two int8 planes, q ~ t2 (256 d_hi + d_lo) with t2 = max|q| / 127 / 256, and one
// v_mfma_i32_16x16x64_i8 forms 16 rows x 16 queries x 64 elements of sum_i c_i d_i, exactly.  With e >= ||q - t2 (256
// d_hi + d_lo)|| and ||c|| <= 127 sqrt(dim)
//
//     | S_r - s_r t2 (256 I_hi + I_lo) | <= a_r Q + s_r 127 sqrt(dim) e =: w                                  (**)
//
// Per-query state, MQ_WORDS words a slot: [0] survivors, [1] Q, [2] 1 = the query cannot be bounded, [3] e, [4] t2,
// [5] 1 = the slot's threshold selection failed (k_survivors_mq).
// Query planes: the fragment of k-step ks (64 elements), plane p (0 hi, 1 lo) and lane l is the u32x4 at
// (ks * 2 + p) * 64 + l: bytes j = 0 .. 15 are the codes of query l & 15 at elements 64 ks + 16 (l >> 4) + j.  The
// rows' fragments take the same elements: lane l loads the 16 bytes at 64 ks + 16 (l >> 4) of row l & 15 of its tile,
// so the four lanes of a row read 64 contiguous bytes per load instruction and two adjacent k-steps a whole line.
// Whatever element of K the matrix core pairs byte j of lane group l >> 4 with, it pairs the same one of A and B:
// the sum over all of them does not depend on it.
constexpr int MQ_WIDTH = 16, MQ_WORDS = 8;
constexpr double MQ_INFLATE = 1.0 + 0x1p-40;  // on w: the double roundings of w and of s t2 I (a few 2^-53 (|lb| + w))
constexpr int MQ_BLOCKS_PER_CU = 1;
constexpr int mq_default_tiles(int C) { return C == 4 ? 1 : 2; }  // 16-row tiles of one request: 8 / 16 / 16 KiB a wave

typedef int i32x4 __attribute__((ext_vector_type(4)));

// 127 sqrt(dim), rounded up
__host__ __device__ constexpr double mq_code_norm(int dim) { return dim == 256 ? 2032.0 : dim == 512 ? 2873.6819588 : 4064.0; }

// A slot's constants of (**) and its kin from its state words: the factor on the integer sum (t2 times the shadow's
// `factor`, a power of two: exact) and the two factors of the width w = a_r wQ + s_r wE, with the shadow's code norm.
// The scans (tile_scan) and the survivor pass (k_survivors_mq) form the same w from them.
struct SlotBound {
    double t2q, wQ, wE;
};
__device__ __forceinline__ SlotBound slot_bound(const unsigned *st, double factor, double code_norm) {
    return {(double)__uint_as_float(st[4]) * factor, (double)__uint_as_float(st[1]) * MQ_INFLATE,
            (double)__uint_as_float(st[3]) * code_norm * MQ_INFLATE};
}

// THE certificate of the matrix-core scans: the lower bound of row r's score from its exact integer sum I and its
// constants s_r, a_r, lb = s t2q I - (a wQ + s wE) in double, padded downwards by its own rounding (relative) and by
// underflow (PAD_ABS), and rounded down to float.  Every tile scan's epilogue is this function.  (k_q8_bounds forms
// s A - a Q from a float sum A, another expression: it keeps its own.)
__device__ __forceinline__ float certified_lb(double I, float s, float a, const SlotBound &b) {
    const double sd = (double)s;
    const double wv = (double)a * b.wQ + sd * b.wE;
    double lb = sd * b.t2q * I - wv;
    lb -= fabs(lb) * 0x1p-50 + PAD_ABS;
    return __double2float_rd(lb);
}

// One query into its two code planes and its state words, by one block of 256 threads.  code_at(i, p) is where the
// code of element i in plane p (0 hi, 1 lo) goes: the caller's operand layout.
template <class CodeAt>
__device__ __forceinline__ void mq_quantise_query(const float *__restrict__ q, int dim, float *__restrict__ q_keep,
                                                  unsigned *__restrict__ st, CodeAt code_at) {
    __shared__ double part[4], part_e[4];
    __shared__ float part_m[4];
    double s = 0.0;
    float m = 0.0f;
    bool finite = true;
    for (int i = threadIdx.x; i < dim; i += 256) {
        const float v = q[i];
        if (q_keep) q_keep[i] = v;
        finite = finite && isfinite(v);
        m = fmaxf(m, fabsf(v));
        s += (double)v * (double)v;
    }
    s = wave_sum_d(s);
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    const bool all_finite = __syncthreads_and(finite);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s, part_m[threadIdx.x >> 6] = m;
    __syncthreads();
    m = fmaxf(fmaxf(part_m[0], part_m[1]), fmaxf(part_m[2], part_m[3]));
    const double tot = part[0] + part[1] + part[2] + part[3];
    const float Q = __double2float_ru(sqrt(tot) * (1.0 + 0x1p-40));  // k_q8_query's Q
    const bool bad = !all_finite || !(Q <= MAX_QNORM) || Q == 0.0f || !(m >= MIN_ABS && m <= MAX_ABS);
    const float t = m / 127.0f, t2 = t * 0x1p-8f;
    double e2 = 0.0;
    for (int i = threadIdx.x; i < dim; i += 256) {
        int hi = 0, lo = 0;
        if (!bad) {
            const double v = (double)q[i];
            const double dh = rint(v / (double)t);
            const double r1 = v - (double)t * dh;  // exact
            const double dl = fmin(fmax(rint(r1 / (double)t2), -127.0), 127.0);
            const double r2 = r1 - (double)t2 * dl;
            e2 = __dadd_rn(e2, __dmul_rn(r2, r2));  // not contracted: the numpy twin adds the rounded square
            hi = (int)dh, lo = (int)dl;
        }
        *code_at(i, 0) = (int8_t)hi;
        *code_at(i, 1) = (int8_t)lo;
    }
    e2 = wave_sum_d(e2);
    if ((threadIdx.x & 63) == 0) part_e[threadIdx.x >> 6] = e2;
    __syncthreads();
    if (threadIdx.x == 0) {
        const double te = part_e[0] + part_e[1] + part_e[2] + part_e[3];
        st[0] = 0u;
        st[1] = __float_as_uint(Q);
        st[2] = bad ? 1u : 0u;
        st[3] = __float_as_uint(__double2float_ru(sqrt(te) * SAFETY));
        st[4] = __float_as_uint(t2);
        st[5] = 0u;
    }
}

// One block a slot.  Slots >= w get zero codes and nothing else.
__global__ __launch_bounds__(256) void k_q8_query_mq(const float *__restrict__ qb, int dim, int w, unsigned *__restrict__ mq,
                                                     int8_t *__restrict__ planes, float *__restrict__ q_last) {
    const int b = blockIdx.x;
    auto code_at = [&](int i, int p) -> int8_t * {
        const int ks = i >> 6, g = (i & 63) >> 4, j = i & 15;
        return planes + ((size_t)((ks * 2 + p) * 64 + g * 16 + b) * 16 + j);
    };
    if (b >= w) {
        for (int i = threadIdx.x; i < dim; i += 256) *code_at(i, 0) = 0, *code_at(i, 1) = 0;
        return;
    }
    mq_quantise_query(qb + (size_t)b * dim, dim, b == w - 1 ? q_last : nullptr, mq + b * MQ_WORDS, code_at);
}

// One v_mfma_i32_16x16x64_i8 per query plane of a k-step: the row operand a with the PLANES operands of the k-step
template <int PLANES>
__device__ __forceinline__ void mq_products(i32x4 a, const i32x4 (&q)[PLANES], i32x4 (&acc)[PLANES]) {
#pragma unroll
    for (int p = 0; p < PLANES; ++p) acc[p] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, q[p], acc[p], 0, 0, 0);
}

// Codes policy of tile_scan (below): the int8 shadow's rows, (**).  A tile is 16 consecutive rows in row-major order;
// lane l loads the 16 bytes at 64 ks + 16 (l >> 4) of row l & 15 for every k-step ks, which are the MFMA's row operand
// as they are (no unpack).  The buffers are NOT padded to whole tiles: the group after the last full one is loaded row
// by row, every row index clamped to the last row (nothing beyond row n - 1 is read), codes and constants alike.
template <int C>
struct Q8Rows {
    static_assert(C == 1 || C == 2 || C == 4, "dims 256, 512 and 1024");
    static constexpr int dim = 256 * C, KS = dim / 64;
    static constexpr int NL = KS;           // 16-byte words a lane holds of a tile
    static constexpr bool PADDED = false;   // the ragged group goes through load_clamped
    static constexpr double FACTOR = 1.0;   // on t2: the sums are of c
    static constexpr double CODE_NORM = mq_code_norm(dim);
    typedef int8_t Elem;
    // tile t of a full group whose first tile is tile0: every tile of it exists
    __device__ static __forceinline__ int64_t tile(int64_t tile0, int t, int64_t) { return tile0 + t; }
    __device__ static __forceinline__ void load_tile(u32x4 (&c)[NL], const int8_t *__restrict__ codes, int64_t tile0, int t,
                                                     int64_t, int lane) {
        const int8_t *base = codes + tile0 * (int64_t)(16 * dim);                     // wave-uniform
        const unsigned lane_byte = (unsigned)((lane & 15) * dim + 16 * (lane >> 4));  // of the lane's 16 codes of k-step 0
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
            c[ks] = __builtin_nontemporal_load(
                reinterpret_cast<const u32x4 *>(base + (lane_byte + (unsigned)(t * 16 * dim + ks * 64))));
    }
    // tile t of the ragged group of `ragged` rows, whose first tile is tile0 (plain loads, as they have always been: at
    // most one group a launch; the full groups' loads above are the non-temporal ones)
    __device__ static __forceinline__ void load_clamped(u32x4 (&c)[NL], float (&s)[4], float (&a)[4],
                                                        const int8_t *__restrict__ codes, const float *__restrict__ scale,
                                                        const float *__restrict__ err, int64_t tile0, int t, int ragged,
                                                        int lane) {
        const int col = lane & 15, quad = lane >> 4;
        const int8_t *base = codes + tile0 * (int64_t)(16 * dim);
        const unsigned row = (unsigned)min(t * 16 + col, ragged - 1);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
            c[ks] = *reinterpret_cast<const u32x4 *>(base + (row * (unsigned)dim + (unsigned)(ks * 64 + 16 * quad)));
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = min(t * 16 + 4 * quad + i, ragged - 1);
            s[i] = (scale + tile0 * 16)[r];
            a[i] = (err + tile0 * 16)[r];
        }
    }
    template <int PLANES>
    __device__ static __forceinline__ void products(const u32x4 (&c)[NL], const i32x4 (&q)[KS][PLANES], i32x4 (&acc)[PLANES]) {
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) mq_products(__builtin_bit_cast(i32x4, c[ks]), q[ks], acc);
    }
};

// k_survivors for one slot of a chunk: the width is w of (**), from the slot's state and the row's scale beside its
// err; the list and the counter are the slot's.  A failed selection or a flagged query collects nothing and leaves
// word [5] / [2] for k_prune_publish_mq.
__global__ __launch_bounds__(256) void k_survivors_mq(const float *__restrict__ lb, const float *__restrict__ err,
                                                      const float *__restrict__ scale, const unsigned *__restrict__ mx,
                                                      int64_t n, double code_norm, const uint64_t *__restrict__ keys,
                                                      const int32_t *__restrict__ sel_count, int32_t k,
                                                      unsigned *__restrict__ st, int64_t *__restrict__ rows,
                                                      int64_t cap) {
    if (sel_count[0] < k || sel_count[1] != 0) {
        if (threadIdx.x == 0) st[5] = 1u;  // every block writes the same word
        return;
    }
    if (st[2] != 0u) return;
    const float T = ord_to_f32((uint32_t)(keys[k - 1] >> 32));
    const SlotBound b = slot_bound(st, 1.0, code_norm);  // (its factor on the sums is not used here)
    const double w_max = ((double)__uint_as_float(mx[0]) * b.wQ + (double)__uint_as_float(mx[1]) * b.wE) * WMAX_INFLATE;
    survivor_pass<true>(lb, err, scale, n, T, b.wQ, b.wE, w_max, &st[0], rows, cap);
}

// every slot's answer in one launch: host_block[1 + j] = survivors or -1, j < w, released under host_block[0] = seq
__global__ void k_prune_publish_mq(const unsigned *__restrict__ mq, int w, int64_t cap, int32_t *__restrict__ host_block,
                                   unsigned seq) {
    if (threadIdx.x != 0) return;
    for (int j = 0; j < w; ++j) {
        const unsigned *st = mq + j * MQ_WORDS;
        const bool fall = st[5] != 0u || st[2] != 0u || (int64_t)st[0] > cap;
        host_block[1 + j] = fall ? -1 : (int32_t)st[0];
    }
    __threadfence_system();
    __hip_atomic_store(reinterpret_cast<unsigned *>(host_block), seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

__global__ __launch_bounds__(256) void k_scatter_scores(const int64_t *__restrict__ rows, const float *__restrict__ v,
                                                        int64_t m, float *__restrict__ scores) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < m) scores[rows[i]] = v[i];
}


// ---- the packed 6-bit shadow of the rows and its scan on the int8 matrix core ("6-bit shadow") -----
// The rows x are the f32 rows, or the widened binary16 rows of an f16 index (as for the int8 shadow: the head of this
// file).  Codes c = rint(x / s6), |c| <= 31, s6 = max|x| / 31; a6 is the int8 shadow's a_r with these codes.  The query
// is the chunk's (k_q8_query_mq: two int8 planes, residual norm e), so with ||c|| <= 31 sqrt(dim)
//
//     | S_r - (s6_r / 4) t2 I_r | <= a6_r Q + s6_r 31 sqrt(dim) e =: w,   I_r = sum_i 4 c_ri (256 d_hi,i + d_lo,i)   (***)
//
// Layout (q6_slot, q6_word_offset in ssw_common.h: the ONE placement function, shared with the lab hook and mirrored by
// the tests' numpy twin): tiles of 16 consecutive rows; the lane of row r and element i is 16 ((i % 64) / 16) + r % 16,
// which owns 3 dim / 64 words of the tile; k-step u = i / 64 takes its words 3u .. 3u + 2, slot j = i % 16: slots 0 ..
// 11 are the upper six bits of those twelve bytes, slot 12 + b is spread over the low two bits of byte b of the three
// words (code bits 5:4, 3:2, 1:0).  Word wi of lane l is the four bytes at (wi / 4) * 1024 + 16 l + 4 (wi % 4) of the
// tile: every wave load instruction reads 1 KiB contiguous.  The state words are a slot's of the chunk (MQ_WORDS).
// Query operand: k-step u, lane l: the u32x4 at u * 64 + l holds the hi plane's codes of elements 64 u + 16 (l >> 4) + j
// in column 0 (l & 15 == 0), the lo plane's in column 1, zeros elsewhere (written once, when the buffer is made).
constexpr int Q6_BLOCKS_PER_CU = 1;
// 16-row tiles of one request of a wave: 6 KiB at dim 256 and 512, 12 KiB (one tile) at dim 1024.  From the traced sweep
// of blocks a CU x tiles at 10^8 rows (docs/EXPERIMENTS.md, "The 6-bit scan's launch shape"): at dim 256 two tiles take
// 3.63 ms a launch where the four of the 12-KiB rule took 4.13, at dim 512 one tile 6.17 where two took 6.25; a second
// or fourth block a CU is level with one at dim 256 and behind it at dim 512 and 1024.  Dim 768 (C = 3, 9 KiB a tile) takes
// one tile, the only count scan_tiles admits there; its launch shape has not been swept.
constexpr int q6_default_tiles(int C) { return C == 1 ? 2 : 1; }

// 31 sqrt(dim), rounded up
__host__ __device__ constexpr double q6_code_norm(int dim) {
    return dim == 256 ? 496.0 : dim == 512 ? 701.4499270 : dim == 768 ? 859.0972006 : 992.0;
}

// The tile assembly both builders share: cl is the wave's LDS line with the codes of row r in natural element order,
// one byte each; lane l assembles words l, l + 64, .. of the row's 12 dim / 64 and stores each at its place in the tile.
template <int C>
__device__ __forceinline__ void q6_store_row(const int8_t *cl, int64_t r, int lane, unsigned char *__restrict__ codes) {
    constexpr int dim = 256 * C, KS = dim / 64, WPL = 3 * KS;  // words a lane of the tile owns
    constexpr size_t TILE_BYTES = (size_t)16 * dim * 3 / 4;
    unsigned char *tile = codes + (size_t)(r >> 4) * TILE_BYTES;
    for (int w = lane; w < 4 * WPL; w += 64) {
        const int g = w / WPL, wi = w % WPL, u = wi / 3, part = wi % 3;
        unsigned word = 0u;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int main_c = cl[q6_element(u, g, 4 * part + b)], low_c = cl[q6_element(u, g, 12 + b)];
            word |= ((((unsigned)main_c & 0x3fu) << 2) | (((unsigned)low_c >> (4 - 2 * part)) & 3u)) << (8 * b);
        }
        *reinterpret_cast<unsigned *>(tile + q6_word_offset(16 * g + (int)(r & 15), wi)) = word;
    }
}

// one wave per row (grid-strided).  The row's codes in natural order go through the wave's own LDS line (lane l holds
// the elements 4C l .. + 4C - 1: words l C .. + C - 1 of the line), then q6_store_row.
template <int C>
__global__ __launch_bounds__(256) void k_q6_build(const float *__restrict__ X, int64_t n, unsigned char *__restrict__ codes,
                                                  float *__restrict__ scale, float *__restrict__ err) {
    constexpr int dim = 256 * C;
    __shared__ unsigned line[4][64 * C];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int8_t *cl = reinterpret_cast<const int8_t *>(line[wave]);
    for (int64_t r = (int64_t)blockIdx.x * 4 + wave; r < n; r += (int64_t)gridDim.x * 4) {
        const float4 *src = reinterpret_cast<const float4 *>(X + r * dim) + lane * C;
        float x[4 * C];
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float4 v = src[c];
            x[4 * c] = v.x, x[4 * c + 1] = v.y, x[4 * c + 2] = v.z, x[4 * c + 3] = v.w;
        }
        unsigned packed[C];
        q8_quantise_row<C, 31>(x, r, lane, packed, scale, err);
        __builtin_amdgcn_wave_barrier();  // the previous row's reads of the line are issued (LDS is in order per wave)
#pragma unroll
        for (int c = 0; c < C; ++c) line[wave][lane * C + c] = packed[c];
        __builtin_amdgcn_wave_barrier();
        q6_store_row<C>(cl, r, lane, codes);
    }
}

// The same from binary16 rows in the f16 index's layout (load_row_h16): chunk c of lane l is the natural elements
// 256c + 4l .. + 3, so its word of codes is word 64c + l of the line (a wave's store of a chunk is 256 contiguous bytes,
// no bank is hit twice).  The codes and s6_r are those of k_q6_build on the widened rows; a6_r's double sums are taken
// over another assignment of elements to lanes.
template <int C>
__global__ __launch_bounds__(256) void k_q6_build_h16(const uint16_t *__restrict__ X, int64_t n,
                                                      unsigned char *__restrict__ codes, float *__restrict__ scale,
                                                      float *__restrict__ err) {
    __shared__ unsigned line[4][64 * C];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int8_t *cl = reinterpret_cast<const int8_t *>(line[wave]);
    for (int64_t r = (int64_t)blockIdx.x * 4 + wave; r < n; r += (int64_t)gridDim.x * 4) {
        float x[4 * C];
        load_row_h16<C>(X, r, lane, x);
        unsigned packed[C];
        q8_quantise_row<C, 31>(x, r, lane, packed, scale, err);
        __builtin_amdgcn_wave_barrier();  // as in k_q6_build
#pragma unroll
        for (int c = 0; c < C; ++c) line[wave][64 * c + lane] = packed[c];
        __builtin_amdgcn_wave_barrier();
        q6_store_row<C>(cl, r, lane, codes);
    }
}

// the query's planes in the operand layout above, its state words and its copy into the index's own buffer
__global__ __launch_bounds__(256) void k_q6_query(const float *__restrict__ q, int dim, unsigned *__restrict__ st,
                                                  int8_t *__restrict__ planes, float *__restrict__ q_keep) {
    mq_quantise_query(q, dim, q_keep, st, [&](int i, int p) -> int8_t * {
        int u, g, j;
        q6_slot(i, &u, &g, &j);
        return planes + ((size_t)(u * 64 + g * 16 + p) * 16 + j);
    });
}

template <int CTRL>
__device__ __forceinline__ int dpp_i(int v) {
    return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, true);
}

// What the two packed shadows share as Codes policies of tile_scan: NL contiguous 1-KiB wave loads a tile (word l of
// lane `lane` is the u32x4 at l * 64 + lane of the tile), code and constant buffers padded to whole tiles, so the
// ragged group is loaded as a full one with a tile past the last one read as the last one again.
template <int NL_>
struct PackedTiles {
    static constexpr int NL = NL_;  // 16-byte words a lane holds of a tile
    static constexpr bool PADDED = true;
    typedef u32x4 Elem;
    // tile t of a group whose first tile is tile0; none beyond last_tile is read (wave-uniform)
    __device__ static __forceinline__ int64_t tile(int64_t tile0, int t, int64_t last_tile) {
        return tile0 + t < last_tile ? tile0 + t : last_tile;
    }
    __device__ static __forceinline__ void load_tile(u32x4 (&c)[NL], const u32x4 *__restrict__ codes, int64_t tile0, int t,
                                                     int64_t last_tile, int lane) {
        const u32x4 *base = codes + tile(tile0, t, last_tile) * (int64_t)(NL * 64) + lane;
#pragma unroll
        for (int l = 0; l < NL; ++l) c[l] = __builtin_nontemporal_load(base + l * 64);
    }
    // the lane's words, a dword each
    __device__ static __forceinline__ void words(const u32x4 (&c)[NL], unsigned (&w)[4 * NL]) {
#pragma unroll
        for (int l = 0; l < NL; ++l) w[4 * l] = c[l].x, w[4 * l + 1] = c[l].y, w[4 * l + 2] = c[l].z, w[4 * l + 3] = c[l].w;
    }
};

// Codes policy of tile_scan: the packed 6-bit shadow, (***): three words a k-step.
// Unpack, per 16 codes = one k-step of a lane (ISA of k_q6_bounds<2, 2>: 3 v_and_b32 with 0xfcfcfcfc for the three
// operand words 4c, and for the fourth 3 v_and_b32 with 0x03030303, 3 v_lshlrev_b32 and 1 v_or3_b32): 10 VALU
// instructions, no sign extension.  Then one v_mfma_i32_16x16x64_i8 a query plane.
template <int C>
struct Q6Tiles : PackedTiles<3 * C> {
    static constexpr int dim = 256 * C, KS = dim / 64, NL = 3 * C;
    static constexpr double FACTOR = 0.25;  // on t2, exact: the sums are of 4 c
    static constexpr double CODE_NORM = q6_code_norm(dim);
    template <int PLANES>
    __device__ static __forceinline__ void products(const u32x4 (&c)[NL], const i32x4 (&q)[KS][PLANES], i32x4 (&acc)[PLANES]) {
        unsigned w[4 * NL];
        PackedTiles<NL>::words(c, w);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const unsigned w0 = w[3 * ks], w1 = w[3 * ks + 1], w2 = w[3 * ks + 2];
            const i32x4 a = {(int)(w0 & 0xfcfcfcfcu), (int)(w1 & 0xfcfcfcfcu), (int)(w2 & 0xfcfcfcfcu),
                             (int)(((w0 & 0x03030303u) << 6) | ((w1 & 0x03030303u) << 4) | ((w2 & 0x03030303u) << 2))};
            mq_products(a, q[ks], acc);
        }
    }
};

// ---- a chunk of up to 16 queries on the 6-bit shadow ("Pruned batch on the 6-bit shadow") ---------
// k_q6_bounds multiplies 14 of the 16 query columns by zeros; here every column is a query of the chunk, (***) holds per
// slot, and the pass costs the same code loads and the same unpack with two MFMAs a k-step instead of one.
// Query operand: with (u, g, j) = q6_slot(i) the code of element i, plane p (0 hi, 1 lo) of query b is byte
// (((u * 2 + p) * 64 + 16 g + b) * 16 + j): the operand of k-step u and plane p is the u32x4 at (u * 2 + p) * 64 + l of
// lane l, column l & 15 the query, its elements those the row operand of k_q6_bounds holds in lane group l >> 4.  The
// buffer is the int8 chunk's (q8_mq_plane_bytes): one shadow serves a chunk.
// One block a slot.  Slots >= w get zero codes and nothing else.
__global__ __launch_bounds__(256) void k_q6_query_mq(const float *__restrict__ qb, int dim, int w, unsigned *__restrict__ mq,
                                                     int8_t *__restrict__ planes, float *__restrict__ q_last) {
    const int b = blockIdx.x;
    auto code_at = [&](int i, int p) -> int8_t * {
        int u, g, j;
        q6_slot(i, &u, &g, &j);
        return planes + ((size_t)((u * 2 + p) * 64 + 16 * g + b) * 16 + j);
    };
    if (b >= w) {
        for (int i = threadIdx.x; i < dim; i += 256) *code_at(i, 0) = 0, *code_at(i, 1) = 0;
        return;
    }
    mq_quantise_query(qb + (size_t)b * dim, dim, b == w - 1 ? q_last : nullptr, mq + b * MQ_WORDS, code_at);
}

constexpr int Q6MQ_BLOCKS_PER_CU = 1;
// 12 KiB a wave at every dim, the request k_q6_bounds had when this was set; one tile at dim 512 is behind two at nq = 16
// (profiles/q6_shape_batch_thresholds.txt); dim 768 (C = 3): one tile, 9 KiB
constexpr int q6mq_default_tiles(int C) { return 4 / C; }

// ---- the packed 5-bit shadow of f32 rows and its scan ("5-bit shadow") ------------------------------
// Codes c = rint(x / s5), |c| <= 15, s5 = max|x| / 15; a5 is the int8 shadow's a_r with these codes.  The query is
// k_q6_query's (planes and state words unchanged), so with ||c|| <= 15 sqrt(dim)
//
//     | S_r - (s5_r / 8) t2 I_r | <= a5_r Q + s5_r 15 sqrt(dim) e =: w,   I_r = sum_i 8 c_ri (256 d_hi,i + d_lo,i)   (****)
//
// |8 c| <= 120 fits int8 and a plane's sum stays below 2^31 at dim 1024 (120 * 127 * 1024).  w is twice the 6-bit
// shadow's, which the threshold over the lower bounds alone does not survive: the caller raises it to the k-th exact
// score of a thousand candidates before the survivor pass (k_exact_threshold below).
// Layout (q5_fields in ssw_common.h): the 6-bit shadow's tiles, lanes, k-steps and slots; a lane owns 5 dim / 128 words of
// the tile, the pair of k-steps 2 p, 2 p + 1 its words 5 p .. 5 p + 4; word wi of lane l is at q6_word_offset(l, wi): every
// wave load instruction reads 1 KiB contiguous, five of them a tile at dim 512, ten at dim 1024.  Dims 256 and 768 have
// 2.5 and 7.5 such loads and no 5-bit shadow.
// 10 KiB a request of a wave at both dims.  Swept at 10^8 x 512 rows (profiles/prune5_shape_sweep.txt, host wall ms of a
// whole call, medians of 12 with the shapes alternating): one block a CU 5.510 with one tile and 5.498 with two -- level,
// the ranges overlap -- two blocks a CU 5.656 and 5.664, behind both.  Dim 1024 has the one shape (scan_tiles).
constexpr int Q5_BLOCKS_PER_CU = 1;
constexpr int q5_default_tiles(int C) { return C == 2 ? 2 : 1; }

// 15 sqrt(dim), rounded up
__host__ __device__ constexpr double q5_code_norm(int dim) { return dim == 512 ? 339.4112550 : 480.0; }

// one wave per row (grid-strided).  The row's codes in natural order go through the wave's LDS line as in k_q6_build;
// then every lane ORs the fields of its 4C codes (q5_fields) into the row's 4 * WPL packed words in LDS, word g * WPL + wi
// being word wi of the lane of group g, and the words go to their places in the tile.
template <int C>
__global__ __launch_bounds__(256) void k_q5_build(const float *__restrict__ X, int64_t n, unsigned char *__restrict__ codes,
                                                  float *__restrict__ scale, float *__restrict__ err) {
    constexpr int dim = 256 * C, KS = dim / 64, WPL = 5 * KS / 2;  // words a lane of the tile owns
    constexpr size_t TILE_BYTES = (size_t)16 * dim * 5 / 8;
    __shared__ unsigned packed_row[4][4 * WPL];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t r = (int64_t)blockIdx.x * 4 + wave; r < n; r += (int64_t)gridDim.x * 4) {
        const float4 *src = reinterpret_cast<const float4 *>(X + r * dim) + lane * C;
        float x[4 * C];
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float4 v = src[c];
            x[4 * c] = v.x, x[4 * c + 1] = v.y, x[4 * c + 2] = v.z, x[4 * c + 3] = v.w;
        }
        unsigned packed[C];
        q8_quantise_row<C, 15>(x, r, lane, packed, scale, err);
        __builtin_amdgcn_wave_barrier();  // the previous row's reads of the words are issued (LDS is in order per wave)
        for (int w = lane; w < 4 * WPL; w += 64) packed_row[wave][w] = 0u;
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int t = 0; t < 4 * C; ++t) {
            const unsigned c5 = (packed[t >> 2] >> (8 * (t & 3))) & 0x1fu;  // the code of element 4C lane + t, five bits
            int u, g, j;
            q6_slot(4 * C * lane + t, &u, &g, &j);
            Q5Field f[3];
            const int nf = q5_fields(u, j, f);
#pragma unroll
            for (int i = 0; i < 3; ++i)  // (unrolled: the fields stay in registers)
                if (i < nf)
                    atomicOr(&packed_row[wave][g * WPL + f[i].word],
                             ((c5 >> f[i].from) & ((1u << f[i].bits) - 1u)) << (8 * f[i].byte + f[i].lo));
        }
        __builtin_amdgcn_wave_barrier();
        unsigned char *tile = codes + (size_t)(r >> 4) * TILE_BYTES;
        for (int w = lane; w < 4 * WPL; w += 64)
            *reinterpret_cast<unsigned *>(tile + q6_word_offset(16 * (w / WPL) + (int)(r & 15), w % WPL)) = packed_row[wave][w];
    }
}

// Codes policy of tile_scan: the packed 5-bit shadow, (****): five words a pair of k-steps, NL = 5 C / 2 loads a tile.
// Unpack, per five words = 32 codes = two k-steps of a lane: five v_and_b32 with 0xf8f8f8f8 give 20 operand bytes 8 c;
// the three spill words x0, x1, x2 are put together from the low bits (the map at q5_fields), no sign extension.  Two
// MFMAs a pair and query plane: {m0, m1, m2, x0} with the query operand of k-step 2 p, {m3, m4, x1, x2} with that of
// 2 p + 1.
template <int C>
struct Q5Tiles : PackedTiles<5 * C / 2> {
    static_assert(C == 2 || C == 4, "dims 512 and 1024");
    static constexpr int dim = 256 * C, KS = dim / 64, NL = 5 * C / 2;
    static constexpr double FACTOR = 0.125;  // on t2, exact: the sums are of 8 c
    static constexpr double CODE_NORM = q5_code_norm(dim);
    template <int PLANES>
    __device__ static __forceinline__ void products(const u32x4 (&c)[NL], const i32x4 (&q)[KS][PLANES], i32x4 (&acc)[PLANES]) {
        unsigned w[4 * NL];
        PackedTiles<NL>::words(c, w);
#pragma unroll
        for (int p = 0; p < KS / 2; ++p) {
            const unsigned w0 = w[5 * p], w1 = w[5 * p + 1], w2 = w[5 * p + 2], w3 = w[5 * p + 3], w4 = w[5 * p + 4];
            const unsigned x0 = ((w0 & 0x07070707u) << 5) | ((w1 & 0x03030303u) << 3);
            const unsigned x1 = ((w2 & 0x07070707u) << 5) | ((w3 & 0x03030303u) << 3);
            const unsigned x2 = ((w4 & 0x07070707u) << 5) | ((w1 & 0x04040404u) << 2) | ((w3 & 0x04040404u) << 1);
            const i32x4 a0 = {(int)(w0 & 0xf8f8f8f8u), (int)(w1 & 0xf8f8f8f8u), (int)(w2 & 0xf8f8f8f8u), (int)x0};
            const i32x4 a1 = {(int)(w3 & 0xf8f8f8f8u), (int)(w4 & 0xf8f8f8f8u), (int)x1, (int)x2};
            mq_products(a0, q[2 * p], acc);
            mq_products(a1, q[2 * p + 1], acc);
        }
    }
};

// ---- the tile scan: one skeleton for the four shadow scans on the int8 matrix core ---------------------------------------
// Where the lab hooks' DEBUG instances put a row's integer sums: I_r as int64, or the two plane sums as int32
struct DebugSum {
    int64_t *__restrict__ I;
    __device__ __forceinline__ void put(int64_t at, int, int, double sum) const { I[at] = (int64_t)sum; }
};
struct DebugPlanes {
    int32_t *__restrict__ hi, *__restrict__ lo;
    __device__ __forceinline__ void put(int64_t at, int h, int l, double) const { hi[at] = h, lo[at] = l; }
};

// Out policy: ONE query (k_q6_bounds, k_q5_bounds).  The operand (k_q6_query) has one plane: the hi codes in column 0,
// the lo codes in column 1 and zeros elsewhere, so 14 of the 16 result columns are products with zeros.  Result lane l
// holds rows 4 (l >> 4) .. + 3 of the tile for column l & 15; the lanes of column 0 fetch column 1's sum with one DPP
// move each, do the double epilogue and store into scores.  Debug: I_r goes to dbg.I[r].
struct OneQuery {
    static constexpr int PLANES = 1;
    static constexpr bool ONE_TEST = true;  // four lanes of a wave store: one test around everything (tile_scan)
    static constexpr bool STORE_H = false;  // (OneQueryH below)
    __device__ __forceinline__ double adjust(double I) const { return I; }
    const unsigned *state;                  // the kernel's arguments: the query's state words (a slot's, MQ_WORDS),
    float *scores;
    DebugSum dbg;
    __device__ __forceinline__ const unsigned *st(int) const { return state; }
    __device__ __forceinline__ float *dst(int) const { return scores; }
    __device__ __forceinline__ bool stores(int col) const { return col == 0; }
    __device__ __forceinline__ int64_t dbg_at(int, int64_t r) const { return r; }
    // the two plane sums of the lane's row i
    __device__ __forceinline__ void sums(const i32x4 (&acc)[1], int i, int *hi, int *lo) const {
        *hi = acc[0][i];
        *lo = dpp_i<DPP_XOR1>(acc[0][i]);  // column 1's sum, for the lanes of column 0
    }
};

// Out policy: a CHUNK of w <= 16 queries (k_q8_bounds_mq, k_q6_bounds_mq).  The operand has two planes a k-step (hi, lo:
// k_q8_query_mq, k_q6_query_mq) and every result column is a query: lane l holds query l & 15 and rows 4 (l >> 4) .. + 3
// of the tile in two accumulators and stores into its slot's slab (query j's is slab j: side + j * stride for
// j + 1 < w, the last one `own`); the lanes of a slot >= w store nothing.  Debug: the sums of query j's row r go to
// element j * n + r of the arrays of Debug.
template <class Debug>
struct Chunk {
    static constexpr int PLANES = 2;
    static constexpr bool ONE_TEST = false;  // most lanes store: every store on its own test
    static constexpr bool STORE_H = false;
    __device__ __forceinline__ double adjust(double I) const { return I; }
    const unsigned *mq;                      // the kernel's arguments
    int w;
    float *side;
    int64_t stride;
    float *own;
    int64_t n;
    Debug dbg;
    __device__ __forceinline__ const unsigned *st(int col) const { return mq + (col < w ? col : 0) * MQ_WORDS; }
    __device__ __forceinline__ float *dst(int col) const { return col + 1 < w ? side + (int64_t)col * stride : own; }
    __device__ __forceinline__ bool stores(int col) const { return col < w; }
    __device__ __forceinline__ int64_t dbg_at(int col, int64_t r) const { return (int64_t)col * n + r; }
    __device__ __forceinline__ void sums(const i32x4 (&acc)[2], int i, int *hi, int *lo) const {
        *hi = acc[0][i];
        *lo = acc[1][i];
    }
};

// THE scan of a shadow on the matrix core: lb of every row, for the query or queries of `out`.  C = dim / 256; a wave
// takes groups of T tiles of 16 consecutive rows, grid-strided.  Two register sets (a, b) take turns as in k_q8_bounds:
// while one group is multiplied the next group's codes AND its rows' constants are in flight, so the only waits inside
// the loop are counted ones for the group that was requested an iteration earlier.  The loop has one exit and no branch
// around a request: a path with fewer loads outstanding would make the compiler's wait counts conservative on every
// path.  The last n % (16 T) rows are one clamped group of their own, after the loop, for one wave: nothing is stored
// for a row >= n.  Result map of the 16x16 product: lane l holds column l & 15 and rows 4 (l >> 4) .. + 3 of the tile, so
// it loads those rows' s and a with one 16-byte load each and writes its four bounds with one 16-byte store.
// Codes: the shadow's layout and unpack (Q8Rows, Q6Tiles, Q5Tiles; Q4Tiles further down); Out: what the 16 columns are
// (OneQuery, Chunk; OneQueryH further down: Out::adjust turns the integer sum into the bound's, Out::STORE_H keeps it).
// DEBUG (lab hooks only): the integer sums go to out.dbg as well.
template <template <int> class CodesOf, class Out, int C, int T, bool DEBUG>
__device__ __forceinline__ void tile_scan(const typename CodesOf<C>::Elem *__restrict__ codes, const float *__restrict__ scale,
                                          const float *__restrict__ err, const u32x4 *__restrict__ planes, int64_t n,
                                          const Out out) {
    typedef CodesOf<C> Codes;
    constexpr int KS = Codes::KS, NL = Codes::NL, P = Out::PLANES, G = 16 * T;
    const int lane = threadIdx.x & 63;
    const int col = lane & 15, quad = lane >> 4;
    const int64_t gwave = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t nwaves = (int64_t)gridDim.x * 4;
    const int64_t nfull = n / G;      // groups of G rows
    const int ragged = (int)(n % G);  // rows of the group after them
    // the query operand: plane p of k-step ks is the u32x4 at (ks * P + p) * 64 + lane
    i32x4 q[KS][P];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
        for (int p = 0; p < P; ++p) q[ks][p] = __builtin_bit_cast(i32x4, planes[(ks * P + p) * 64 + lane]);
    const bool each = Out::ONE_TEST || out.stores(col);  // (see the stores)
    float *__restrict__ dst = out.dst(col);
    const SlotBound sb = slot_bound(out.st(col), Codes::FACTOR, Codes::CODE_NORM);
    struct Set {
        u32x4 c[T][NL];
        float s[T][4], a[T][4];
    };
    // all requests of a group.  tile0: its first tile; last_tile: a padded shadow reads none beyond it.  Every code load
    // is non-temporal (Codes::load_tile), with the builtin called without a condition: with
    // `nt ? __builtin_nontemporal_load(p) : *p` the two arms were merged into one load before the constant got in, the
    // hint was lost (no `nt` on any global_load_dwordx4 of the kernel) and the scan ran at the default policy's HBM rate.
    auto load = [&](Set &d, int64_t tile0, int64_t last_tile) {
#pragma unroll
        for (int t = 0; t < T; ++t) Codes::load_tile(d.c[t], codes, tile0, t, last_tile, lane);
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const int64_t tile = Codes::tile(tile0, t, last_tile);
            const float4 sv = *reinterpret_cast<const float4 *>(scale + tile * 16 + 4 * quad);
            const float4 av = *reinterpret_cast<const float4 *>(err + tile * 16 + 4 * quad);
            d.s[t][0] = sv.x, d.s[t][1] = sv.y, d.s[t][2] = sv.z, d.s[t][3] = sv.w;
            d.a[t][0] = av.x, d.a[t][1] = av.y, d.a[t][2] = av.z, d.a[t][3] = av.w;
        }
        // left alone the scheduler sinks these requests into the products that follow, to reuse the registers of the
        // set being consumed: the next group would be requested half a group late
        __builtin_amdgcn_sched_barrier(0);
    };
    // the bounds of the first `rows` rows of group g from a set that has arrived (rows == G: whole stores)
    auto bounds = [&](const Set &d, int64_t g, int rows) {
#pragma unroll
        for (int t = 0; t < T; ++t) {
            i32x4 acc[P];
#pragma unroll
            for (int p = 0; p < P; ++p) acc[p] = i32x4{0, 0, 0, 0};
            Codes::products(d.c[t], q, acc);
            float lb[4];
            int hi[4], lo[4];
            double I[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                out.sums(acc, i, &hi[i], &lo[i]);
                I[i] = (double)hi[i] * 256.0 + (double)lo[i];  // exact: |I| < 2^39 at dim 1024
                lb[i] = certified_lb(out.adjust(I[i]), d.s[t][i], d.a[t][i], sb);
            }
            const int r0 = t * 16 + 4 * quad;  // of the lane's four rows in the group
            // Out::ONE_TEST: one test of the lane stands around all its stores; else each store has it beside the row's
            if (!Out::ONE_TEST || out.stores(col)) {
                if (rows == G) {
                    if (each) *reinterpret_cast<float4 *>(dst + g * G + r0) = make_float4(lb[0], lb[1], lb[2], lb[3]);
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (each && r0 + i < rows) (dst + g * G)[r0 + i] = lb[i];
                }
                if constexpr (Out::STORE_H) {  // the lane's four H beside its four bounds (the array is padded to whole tiles)
                    const i32x4 h4 = {hi[0] * 256 + lo[0], hi[1] * 256 + lo[1], hi[2] * 256 + lo[2], hi[3] * 256 + lo[3]};
                    if (rows == G || r0 < rows) *reinterpret_cast<i32x4 *>(out.H + g * G + r0) = h4;
                }
                if constexpr (DEBUG) {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (each && r0 + i < rows) out.dbg.put(out.dbg_at(col, g * G + r0 + i), hi[i], lo[i], I[i]);
                }
            }
        }
    };
    if (gwave < nfull) {
        const int64_t last = nfull * T - 1;
        Set a, b;
        int64_t g = gwave;
        load(a, g * T, last);
        for (;;) {
            // a wave without a next group requests its last one once more (cache hits) and writes nothing for it
            const int64_t g1 = g + nwaves < nfull ? g + nwaves : g;
            load(b, g1 * T, last);
            bounds(a, g, G);
            const int64_t g2 = g1 + nwaves < nfull ? g1 + nwaves : g1;
            load(a, g2 * T, last);
            bounds(b, g1, g1 != g ? G : 0);
            if (g2 == g1) break;
            g = g2;
        }
    }
    if (ragged != 0 && gwave == nfull % nwaves) {
        Set t;
        if constexpr (Codes::PADDED) {
            load(t, nfull * T, (n - 1) >> 4);
        } else {
#pragma unroll
            for (int tt = 0; tt < T; ++tt)
                Codes::load_clamped(t.c[tt], t.s[tt], t.a[tt], codes, scale, err, nfull * T, tt, ragged, lane);
        }
        bounds(t, nfull, ragged);
    }
}

// The four kernels: a shadow's Codes and the Out of one query or of a chunk.  dbg_*: lab hooks only (DEBUG), else NULL.
// lb of every row for every query of the chunk into the slot's slab, on the int8 shadow
template <int C, int T, bool DEBUG>
__global__ __launch_bounds__(256) void k_q8_bounds_mq(const int8_t *__restrict__ codes, const float *__restrict__ scale,
                                                      const float *__restrict__ err, const u32x4 *__restrict__ planes,
                                                      const unsigned *__restrict__ mq, int w, float *__restrict__ side,
                                                      int64_t stride, float *__restrict__ own, int64_t n,
                                                      int32_t *__restrict__ dbg_hi, int32_t *__restrict__ dbg_lo) {
    tile_scan<Q8Rows, Chunk<DebugPlanes>, C, T, DEBUG>(codes, scale, err, planes, n,
                                                       {mq, w, side, stride, own, n, {dbg_hi, dbg_lo}});
}

// lb of every row into scores[r], on the packed 6-bit shadow
template <int C, int T, bool DEBUG>
__global__ __launch_bounds__(256) void k_q6_bounds(const u32x4 *__restrict__ codes, const float *__restrict__ scale,
                                                   const float *__restrict__ err, const u32x4 *__restrict__ planes,
                                                   const unsigned *__restrict__ st, float *__restrict__ scores, int64_t n,
                                                   int64_t *__restrict__ dbg_I) {
    tile_scan<Q6Tiles, OneQuery, C, T, DEBUG>(codes, scale, err, planes, n, {st, scores, {dbg_I}});
}

// lb of every row for every query of the chunk into the slot's slab, on the packed 6-bit shadow
template <int C, int T, bool DEBUG>
__global__ __launch_bounds__(256) void k_q6_bounds_mq(const u32x4 *__restrict__ codes, const float *__restrict__ scale,
                                                      const float *__restrict__ err, const u32x4 *__restrict__ planes,
                                                      const unsigned *__restrict__ mq, int w, float *__restrict__ side,
                                                      int64_t stride, float *__restrict__ own, int64_t n,
                                                      int64_t *__restrict__ dbg_I) {
    tile_scan<Q6Tiles, Chunk<DebugSum>, C, T, DEBUG>(codes, scale, err, planes, n,
                                                     {mq, w, side, stride, own, n, {dbg_I}});
}

// lb of every row into scores[r], on the packed 5-bit shadow
template <int C, int T, bool DEBUG>
__global__ __launch_bounds__(256) void k_q5_bounds(const u32x4 *__restrict__ codes, const float *__restrict__ scale,
                                                   const float *__restrict__ err, const u32x4 *__restrict__ planes,
                                                   const unsigned *__restrict__ st, float *__restrict__ scores, int64_t n,
                                                   int64_t *__restrict__ dbg_I) {
    tile_scan<Q5Tiles, OneQuery, C, T, DEBUG>(codes, scale, err, planes, n, {st, scores, {dbg_I}});
}

// ---- the two-stage 4 + 1-bit shadow of f32 rows ("Two-stage 4 + 1-bit shadow") ----------------------
// Codes, s5 and a5 are q8_quantise_row<C, 15>'s, the 5-bit shadow's.  Write u = c + 16 in [1, 31], h = u >> 1 in [0, 15],
// b = u & 1, so c = 2 h + b - 16.  With D_i = 256 d_hi,i + d_lo,i and the query state of k_q6_query:
//
// COARSE bound (first stage, every row, the 4-bit plane alone):
//     x = s5 (2 h - 15.5) + r4,     a4_r >= ||r4|| (+ a5's rounding terms; summed in double with SAFETY as a5 is)
//     | S_r - (s5_r / 2) t2 J_r | <= a4_r Q + s5_r 15.5 sqrt(dim) e =: w4
//     J_r = sum_i (4 h_ri - 31) D_i = 4 H_r - 31 sum D,     H_r = sum_i h_ri D_i = 256 H_hi + H_lo
// The operand bytes are the nibbles h themselves (0 .. 15); |H| <= 15 * 1024 * 32639 < 2^31 is one int32 a row, which the
// scan keeps; J is formed exactly in double and goes through certified_lb with FACTOR 0.5 and the code norm 15.5 sqrt(dim).
// Zero rows, rows with a non-finite element and unboundable queries keep the builders' conventions (a = +inf, lb = -inf;
// the flagged query takes the full scan).
//
// FINE bound (second stage, the first stage's survivors only): B_r = sum_i b_ri D_i (|B| < 2^25) and
//     I_r = sum_i 8 c_ri D_i = 8 (2 H_r + B_r - 16 sum D)
// is k_q5_bounds' integer sum, exactly, so certified_lb(I_r, s5_r, a5_r, slot_bound(st, 0.125, q5_code_norm(dim))) is that
// kernel's lower bound bit for bit, and everything downstream of it is the 5-bit path's.
// Layout: q4_nibble (ssw_common.h) for the coarse plane, a tile of 16 rows = NL = 2 C wave loads of 1 KiB; the fine plane
// row-major, dim / 32 words a row.
constexpr int Q4_BLOCKS_PER_CU = 1;
constexpr int q4_default_tiles(int C) { return C == 2 ? 2 : 1; }  // 8 KiB a request of a wave at both dims

// 15.5 sqrt(dim), rounded up
__host__ __device__ constexpr double q4_code_norm(int dim) { return dim == 512 ? 350.7249635 : 496.0; }

// one wave per row (grid-strided), as k_q5_build: the codes and s5, a5 from q8_quantise_row<C, 15> with that kernel's
// assignment of elements to lanes (bit-identical constants); a4 from the same sums with 2 h - 15.5 in the code's place;
// every lane ORs its nibbles (q4_nibble) and its fifth bits into the row's words in LDS, which go to their places.
template <int C>
__global__ __launch_bounds__(256) void k_q41_build(const float *__restrict__ X, int64_t n, unsigned char *__restrict__ coarse,
                                                   unsigned *__restrict__ fine, float *__restrict__ scale,
                                                   float *__restrict__ err, float *__restrict__ err4) {
    constexpr int dim = 256 * C, KS = dim / 64, WPL = 2 * KS, FW = dim / 32;  // words a lane owns; fine words a row
    constexpr size_t TILE_BYTES = (size_t)16 * dim / 2;
    __shared__ unsigned packed_row[4][4 * WPL + FW];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t r = (int64_t)blockIdx.x * 4 + wave; r < n; r += (int64_t)gridDim.x * 4) {
        const float4 *src = reinterpret_cast<const float4 *>(X + r * dim) + lane * C;
        float x[4 * C];
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float4 v = src[c];
            x[4 * c] = v.x, x[4 * c + 1] = v.y, x[4 * c + 2] = v.z, x[4 * c + 3] = v.w;
        }
        unsigned packed[C];
        float s = 0.0f;
        bool ok = false;
        q8_quantise_row<C, 15>(x, r, lane, packed, scale, err, &s, &ok);
        __builtin_amdgcn_wave_barrier();  // the previous row's reads of the words are issued (LDS is in order per wave)
        for (int w = lane; w < 4 * WPL + FW; w += 64) packed_row[wave][w] = 0u;
        __builtin_amdgcn_wave_barrier();
        double e2 = 0.0, x2 = 0.0, c2 = 0.0;
#pragma unroll
        for (int t = 0; t < 4 * C; ++t) {
            const int ci = (int)(int8_t)(packed[t >> 2] >> (8 * (t & 3)));
            const unsigned uu = (unsigned)(ci + 16), h = uu >> 1, b = uu & 1u;
            const int i = 4 * C * lane + t;
            int u, g, j, word, byte, shift;
            q6_slot(i, &u, &g, &j);
            q4_nibble(u, j, &word, &byte, &shift);
            atomicOr(&packed_row[wave][g * WPL + word], h << (8 * byte + shift));
            atomicOr(&packed_row[wave][4 * WPL + (i >> 5)], b << (i & 31));
            const double mid = 2.0 * (double)h - 15.5;  // s * mid is exact in double; so is its difference to x
            const double d = (double)x[t] - (double)s * mid;
            e2 += d * d;
            if (ok) x2 += (double)x[t] * (double)x[t];
            c2 += mid * mid;
        }
        e2 = wave_sum_d(e2);
        x2 = wave_sum_d(x2);
        c2 = wave_sum_d(c2);
        if (lane == 0) {
            const double g = (double)dim * 0x1p-24 / (1.0 - (double)dim * 0x1p-24);
            const double a = SAFETY * (sqrt(e2) + g * sqrt(x2) + g * (double)s * sqrt(c2));
            err4[r] = ok ? __double2float_ru(a) : INFINITY;
        }
        __builtin_amdgcn_wave_barrier();
        unsigned char *tile = coarse + (size_t)(r >> 4) * TILE_BYTES;
        for (int w = lane; w < 4 * WPL; w += 64)
            *reinterpret_cast<unsigned *>(tile + q6_word_offset(16 * (w / WPL) + (int)(r & 15), w % WPL)) = packed_row[wave][w];
        if (lane < FW) fine[r * FW + lane] = packed_row[wave][4 * WPL + lane];
    }
}

// k_q6_query, then: the sums of the two code planes as integers into st[6], st[7], D in natural order, and the first
// stage's counter and dense flag reset
__global__ __launch_bounds__(256) void k_q41_query(const float *__restrict__ q, int dim, unsigned *__restrict__ st,
                                                   int8_t *__restrict__ planes, float *__restrict__ q_keep,
                                                   int32_t *__restrict__ D, unsigned *__restrict__ cstate) {
    auto code_at = [&](int i, int p) -> int8_t * {
        int u, g, j;
        q6_slot(i, &u, &g, &j);
        return planes + ((size_t)(u * 64 + g * 16 + p) * 16 + j);
    };
    mq_quantise_query(q, dim, q_keep, st, code_at);
    __syncthreads();  // (each thread reads back the codes it wrote itself: the same i)
    __shared__ int sums[2][4];
    int sh = 0, sl = 0;
    for (int i = threadIdx.x; i < dim; i += 256) {
        const int hi = *code_at(i, 0), lo = *code_at(i, 1);
        D[i] = 256 * hi + lo;
        sh += hi, sl += lo;
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) sh += __shfl_xor(sh, off, 64), sl += __shfl_xor(sl, off, 64);
    if ((threadIdx.x & 63) == 0) sums[0][threadIdx.x >> 6] = sh, sums[1][threadIdx.x >> 6] = sl;
    __syncthreads();
    if (threadIdx.x == 0) {
        st[6] = (unsigned)(sums[0][0] + sums[0][1] + sums[0][2] + sums[0][3]);
        st[7] = (unsigned)(sums[1][0] + sums[1][1] + sums[1][2] + sums[1][3]);
        for (int i = 0; i < Q41_STATE_WORDS; ++i) cstate[i] = 0u;
    }
}

// Codes policy of tile_scan: the coarse plane.  Unpack, per two words = 16 nibbles = one k-step of a lane: two v_and_b32
// with 0x0f0f0f0f and two shift-and-mask give the four operand words; no sign, no offset (the epilogue has it).
template <int C>
struct Q4Tiles : PackedTiles<2 * C> {
    static_assert(C == 2 || C == 4, "dims 512 and 1024");
    static constexpr int dim = 256 * C, KS = dim / 64, NL = 2 * C;
    static constexpr double FACTOR = 0.5;  // on t2, exact: the sums are of 4 h - 31
    static constexpr double CODE_NORM = q4_code_norm(dim);
    template <int PLANES>
    __device__ static __forceinline__ void products(const u32x4 (&c)[NL], const i32x4 (&q)[KS][PLANES], i32x4 (&acc)[PLANES]) {
        unsigned w[4 * NL];
        PackedTiles<NL>::words(c, w);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const unsigned w0 = w[2 * ks], w1 = w[2 * ks + 1];
            const i32x4 a = {(int)(w0 & 0x0f0f0f0fu), (int)((w0 >> 4) & 0x0f0f0f0fu), (int)(w1 & 0x0f0f0f0fu),
                             (int)((w1 >> 4) & 0x0f0f0f0fu)};
            mq_products(a, q[ks], acc);
        }
    }
};

// Out policy: OneQuery on the coarse plane.  The integer sum of a row is H; the bound takes J = 4 H - 31 sum D (`off`,
// exact in double), and the lane stores its four H beside its four bounds with one 16-byte store.
struct OneQueryH : OneQuery {
    static constexpr bool STORE_H = true;
    int32_t *H;
    double off;
    __device__ __forceinline__ double adjust(double I) const { return 4.0 * I - off; }
};

// lb4 of every row into scores[r] and H_r into H[r], on the coarse plane
template <int C, int T, bool DEBUG>
__global__ __launch_bounds__(256) void k_q4_bounds(const u32x4 *__restrict__ codes, const float *__restrict__ scale,
                                                   const float *__restrict__ err4, const u32x4 *__restrict__ planes,
                                                   const unsigned *__restrict__ st, float *__restrict__ scores,
                                                   int32_t *__restrict__ H, int64_t n) {
    const double off = 31.0 * ((double)(int)st[6] * 256.0 + (double)(int)st[7]);
    tile_scan<Q4Tiles, OneQueryH, C, T, DEBUG>(codes, scale, err4, planes, n, OneQueryH{{st, scores, {nullptr}}, H, off});
}

// the first stage's survivors: k_survivors_mq's pass over the coarse bounds with the coarse width, into the 32-bit list
// behind cstate[0], a block's stage flushed and used again (survivor_pass, FLUSH)
__global__ __launch_bounds__(256) void k_survivors_q4(const float *__restrict__ lb, const float *__restrict__ err4,
                                                      const float *__restrict__ scale, const unsigned *__restrict__ mx,
                                                      int64_t n, double code_norm, const uint64_t *__restrict__ keys,
                                                      const int32_t *__restrict__ sel_count, int32_t k,
                                                      unsigned *__restrict__ st, unsigned *__restrict__ cstate,
                                                      uint32_t *__restrict__ rows, int64_t cap) {
    if (sel_count[0] < k || sel_count[1] != 0) {
        if (threadIdx.x == 0) st[5] = 1u;  // every block writes the same word
        return;
    }
    if (st[2] != 0u) return;
    const float T = ord_to_f32((uint32_t)(keys[k - 1] >> 32));
    const SlotBound b = slot_bound(st, 1.0, code_norm);
    const double w_max = ((double)__uint_as_float(mx[0]) * b.wQ + (double)__uint_as_float(mx[1]) * b.wE) * WMAX_INFLATE;
    survivor_pass<true, true, uint32_t>(lb, err4, scale, n, T, b.wQ, b.wE, w_max, &cstate[0], rows, cap);
}

constexpr int REFINE_UNROLL = 4;  // rows a group of lanes has in flight

// The second stage.  A group of LPR = dim / 32 lanes takes a row: lane j of the group holds D of the row's fine word j in
// 32 registers for the whole launch, so a row costs one 4-byte load a lane, 32 multiply-adds and a reduction over the
// group.  The rows are the first stage's list -- or, when it holds more than coarse_cap, every row of the index (dense:
// lb5 is a bound of any row, so the test below alone decides).  Survivors: survivor_pass' own test with the 5-bit width,
// collected in a block's stage as there (a claim that does not fit goes to the global counter).  The grid does not depend
// on the count, which is read here.  DEBUG (lab hook): lb5 and B per entry.
template <int C, bool DEBUG>
__global__ __launch_bounds__(256) void k_q41_refine(const int32_t *__restrict__ H, const unsigned *__restrict__ fine,
                                                    const float *__restrict__ scale, const float *__restrict__ err,
                                                    const int32_t *__restrict__ D, const uint64_t *__restrict__ keys,
                                                    int32_t k, unsigned *__restrict__ st, unsigned *__restrict__ cstate,
                                                    const uint32_t *__restrict__ list, int64_t coarse_cap, int64_t n,
                                                    int64_t *__restrict__ rows, int64_t cap, float *__restrict__ dbg_lb5,
                                                    int32_t *__restrict__ dbg_B) {
    constexpr int dim = 256 * C, LPR = dim / 32, RPW = 64 / LPR;  // lanes a row, rows a wave-step
    if (st[5] != 0u || st[2] != 0u) return;  // the selection failed or the query cannot be bounded: the full scan
    const int64_t found = (int64_t)cstate[0];
    const bool dense = found > coarse_cap;
    const int64_t m = dense ? n : found;
    if (blockIdx.x == 0 && threadIdx.x == 0) cstate[1] = dense ? 1u : 0u;
    const int lane = threadIdx.x & 63, j = lane % LPR, sub = lane / LPR;
    int Dj[32];
#pragma unroll
    for (int t = 0; t < 32; ++t) Dj[t] = D[32 * j + t];
    const double Td = (double)ord_to_f32((uint32_t)(keys[k - 1] >> 32));
    const SlotBound sb = slot_bound(st, 0.125, q5_code_norm(dim));  // k_q5_bounds' and, for the width, k_survivors_mq's
    const double sumD = (double)(int)st[6] * 256.0 + (double)(int)st[7];
    __shared__ int64_t stage[SURV_STAGE];
    __shared__ unsigned staged, first_failed, stage_base;
    if (threadIdx.x == 0) staged = 0u, first_failed = 0xffffffffu;
    __syncthreads();
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * 4;
    constexpr int STEP = RPW * REFINE_UNROLL;  // entries a wave takes at a time
    for (int64_t e0 = wave * STEP; e0 < m; e0 += nwaves * STEP) {
        int64_t r[REFINE_UNROLL];
        bool have[REFINE_UNROLL];
#pragma unroll
        for (int v = 0; v < REFINE_UNROLL; ++v) {
            const int64_t e = e0 + v * RPW + sub;
            have[v] = e < m;
            r[v] = !have[v] ? 0 : dense ? e : (int64_t)list[e];
            if (r[v] >= n) r[v] = 0, have[v] = false;  // (never beyond the rows, whatever the list holds)
        }
        unsigned fw[REFINE_UNROLL];
        int h[REFINE_UNROLL];
        float s[REFINE_UNROLL], a[REFINE_UNROLL];
#pragma unroll
        for (int v = 0; v < REFINE_UNROLL; ++v) {
            fw[v] = fine[r[v] * LPR + j];
            h[v] = H[r[v]];
            s[v] = scale[r[v]];
            a[v] = err[r[v]];
        }
#pragma unroll
        for (int v = 0; v < REFINE_UNROLL; ++v) {
            int B = 0;
#pragma unroll
            for (int t = 0; t < 32; ++t) B += (int)((fw[v] >> t) & 1u) * Dj[t];
#pragma unroll
            for (int off = 1; off < LPR; off <<= 1) B += __shfl_xor(B, off, 64);
            const double I = 8.0 * (2.0 * (double)h[v] + (double)B - 16.0 * sumD);  // exact: |I| < 2^39
            const float lb5 = certified_lb(I, s[v], a[v], sb);
            const double l = (double)lb5, w = (double)a[v] * sb.wQ + (double)s[v] * sb.wE;
            const bool keep = have[v] && j == 0 && (!(surv_ub(l, w) < Td) || !(lb5 > -INFINITY));
            if constexpr (DEBUG) {
                const int64_t e = e0 + v * RPW + sub;
                if (e < m && j == 0) dbg_lb5[e] = lb5, dbg_B[e] = B;
            }
            const uint64_t ballot = __ballot(keep);
            if (ballot == 0ull) continue;
            const unsigned total = (unsigned)__popcll(ballot);
            unsigned slot = 0u;
            int direct = 0;
            if (lane == 0) {
                slot = atomicAdd(&staged, total);
                if (slot + total > (unsigned)SURV_STAGE) {
                    atomicMin(&first_failed, slot);
                    slot = atomicAdd(&st[0], total);
                    direct = 1;
                }
            }
            slot = __shfl(slot, 0, 64);
            direct = __shfl(direct, 0, 64);
            const int64_t at = (int64_t)slot + __popcll(ballot & ((1ull << lane) - 1ull));
            if (keep) {
                if (!direct) stage[at] = r[v];
                else if (at < cap) rows[at] = r[v];
            }
        }
    }
    __syncthreads();
    const unsigned mine = min(staged, first_failed);
    if (mine == 0u) return;
    if (threadIdx.x == 0) stage_base = atomicAdd(&st[0], mine);
    __syncthreads();
    for (unsigned i = threadIdx.x; i < mine; i += 256) {
        const int64_t at = (int64_t)stage_base + i;
        if (at < cap) rows[at] = stage[i];
    }
}

// k_prune_publish_mq for the one slot, with the first stage's count and the dense flag for the host's counters
__global__ void k_prune_publish_q41(const unsigned *__restrict__ st, const unsigned *__restrict__ cstate, int64_t cap,
                                    int32_t *__restrict__ host_block, unsigned seq) {
    if (threadIdx.x != 0) return;
    const bool fall = st[5] != 0u || st[2] != 0u || (int64_t)st[0] > cap;
    host_block[1] = fall ? -1 : (int32_t)st[0];
    host_block[2] = (int32_t)min(cstate[0], 0x7fffffffu);
    host_block[3] = (int32_t)cstate[1];
    __threadfence_system();
    __hip_atomic_store(reinterpret_cast<unsigned *>(host_block), seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// ---- the exact threshold of the 5-bit path ---------------------------------------------------------------------------
// The threshold selection over the lower bounds ran for kc = min(SSW_MAX_TOPK, max(1024, 4 k)) keys instead of k.  Their
// rows are scored exactly and T_x = the k-th largest of those scores: k distinct rows, none excluded, score at least
// T_x, so the k-th best score of the index is >= T_x and a row with ub < max(T_lb, T_x) cannot be among the k best.
__global__ __launch_bounds__(256) void k_candidate_rows(const uint64_t *__restrict__ keys, const int32_t *__restrict__ sel_count,
                                                        int32_t kc, int64_t n, int64_t *__restrict__ rows_out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= kc) return;
    // a selection that overflowed leaves no keys to trust: row 0 throughout (k_exact_threshold leaves it alone)
    const int count = sel_count[1] != 0 ? 0 : max(0, min(sel_count[0], kc));
    // composite_key's low word (select.hip): 0xffffffff - row
    const uint64_t key = i < count ? keys[i] : count > 0 ? keys[0] : 0xffffffffull;
    const int64_t row = (int64_t)(0xffffffffu - (uint32_t)key);
    rows_out[i] = row < n ? row : 0;  // (never beyond the rows, whatever the keys hold)
}

constexpr int TX_THREADS = 1024, TX_KEYS = SSW_MAX_TOPK;
static_assert((TX_KEYS & (TX_KEYS - 1)) == 0 && TX_KEYS >= TX_THREADS, "a power of two");

// One block.  The ordinal keys of the candidates' exact scores (0 for a NaN score and beyond the count: below every
// score's key, -inf's included) are sorted descending in LDS (bitonic over P = the power of two >= kc keys); T_x's key
// is the k-th, if it is a score's.
__global__ __launch_bounds__(TX_THREADS) void k_exact_threshold(uint64_t *__restrict__ keys,
                                                                const int32_t *__restrict__ sel_count,
                                                                const float *__restrict__ vals, int32_t k, int32_t kc,
                                                                int32_t P) {
    __shared__ uint32_t ord[TX_KEYS];
    if (sel_count[0] < k || sel_count[1] != 0) return;  // the selection failed: the caller falls back
    const int count = min(sel_count[0], kc);  // >= k >= 1 here
    for (int i = threadIdx.x; i < P; i += TX_THREADS) {
        const float v = i < count ? vals[i] : NAN;
        ord[i] = v != v ? 0u : f32_to_ord(v);
    }
    __syncthreads();
    for (int size = 2; size <= P; size <<= 1)
        for (int j = size >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < P; i += TX_THREADS) {
                const int partner = i ^ j;
                if (partner > i) {
                    const uint32_t a = ord[i], b = ord[partner];
                    const bool descending = (i & size) == 0;
                    if (descending ? a < b : a > b) ord[i] = b, ord[partner] = a;
                }
            }
            __syncthreads();
        }
    if (threadIdx.x == 0) {
        const uint32_t tx = ord[k - 1];  // 0: fewer than k scores that are not NaN, T_x = -inf
        const uint64_t key = keys[k - 1];
        if (tx > (uint32_t)(key >> 32)) keys[k - 1] = ((uint64_t)tx << 32) | (key & 0xffffffffull);
    }
}
}  // namespace

bool q8_dim_supported(int32_t dim) { return dim == 256 || dim == 512 || dim == 1024; }
// the packed 6-bit shadow also takes dim 768 (C = 3): its matrix-core scans work in k-steps of 64 elements, where
// k_q8_bounds' lanes-per-row map needs 4 % C == 0
bool q6_dim_supported(int32_t dim) { return q8_dim_supported(dim) || dim == 768; }

// ---- run-time shapes -> template instances ----------------------------------------------------------------------------
template <int N>
using Int = std::integral_constant<int, N>;

// f(Int<C>) for C = dim / 256 of a supported dim; C3: the kernel has a C = 3 instance (the 6-bit shadow's do)
template <bool C3, class F>
static void dispatch_dim(int C, F f) {
    if (C == 1) return f(Int<1>{});
    if (C == 2) return f(Int<2>{});
    if constexpr (C3)
        if (C == 3) return f(Int<3>{});
    f(Int<4>{});
}

// The launch shape of the five tile scans on the matrix core, by TileScan (ssw_tune_prune_scan_mq, ssw_tune_prune6_scan,
// ssw_tune_prune6_scan_mq, ssw_tune_prune5_scan, ssw_tune_prune41_scan; lab build only): four-wave blocks per CU, and 16-row tiles of one request (0: the scan's
// default for C)
struct ScanTune {
    int blocks_per_cu;
    int tiles;
};
constexpr int SCAN_BLOCKS_PER_CU[5] = {MQ_BLOCKS_PER_CU, Q6_BLOCKS_PER_CU, Q6MQ_BLOCKS_PER_CU, Q5_BLOCKS_PER_CU, Q4_BLOCKS_PER_CU};
static SSW_TUNABLE ScanTune g_scan_tune[5] = {{SCAN_BLOCKS_PER_CU[0], 0}, {SCAN_BLOCKS_PER_CU[1], 0}, {SCAN_BLOCKS_PER_CU[2], 0},
                                              {SCAN_BLOCKS_PER_CU[3], 0}, {SCAN_BLOCKS_PER_CU[4], 0}};
constexpr int scan_default_tiles(TileScan scan, int C) {
    return scan == SCAN_Q8_MQ ? mq_default_tiles(C)
           : scan == SCAN_Q6  ? q6_default_tiles(C)
           : scan == SCAN_Q5  ? q5_default_tiles(C)
           : scan == SCAN_Q4  ? q4_default_tiles(C)
                              : q6mq_default_tiles(C);
}

static int scan_tiles(const ScanTune &tune, int default_tiles, int C) {
    int t = tune.tiles > 0 ? tune.tiles : default_tiles;
    // two register sets of more than 16 KiB (int8 codes) or 12 KiB (6-bit codes) a wave do not fit beside the query operand
    while (t * C > 4) t >>= 1;
    return t;
}

void scan_shape(TileScan scan, int32_t dim, int device, int64_t n, int *out_blocks, int *out_tiles) {
    const int T = scan_tiles(g_scan_tune[scan], scan_default_tiles(scan, dim / 256), dim / 256);
    const int64_t need = ((n + 16 * T - 1) / (16 * T) + 3) / 4;
    int64_t grid = (int64_t)num_cus(device) * g_scan_tune[scan].blocks_per_cu;
    if (grid > need) grid = need;
    if (grid < 1) grid = 1;
    *out_blocks = (int)grid;
    *out_tiles = T;
}

#ifdef SSW_DEBUG_HOOKS
void tune_tile_scan(TileScan scan, int blocks_per_cu, int tiles) {
    g_scan_tune[scan].blocks_per_cu = blocks_per_cu >= 1 && blocks_per_cu <= 8 ? blocks_per_cu : SCAN_BLOCKS_PER_CU[scan];
    g_scan_tune[scan].tiles = tiles == 1 || tiles == 2 || tiles == 4 ? tiles : 0;
}
#endif

// the C = dim / 256 a tile scan has instances of: its shadow's dims
constexpr bool scan_has_dim(TileScan scan, int C) {
    return scan == SCAN_Q8_MQ ? C != 3 : scan == SCAN_Q5 || scan == SCAN_Q4 ? C == 2 || C == 4 : true;
}

// f(Int<C>, Int<T>, DEBUG) for the instance of tile scan S that scan_shape's T and the caller's debug output ask for.
// The product has one instance per C of scan_has_dim, at the scan's default T and without DEBUG; the lab build has
// every T with T * C <= 4 (scan_tiles), each with and without DEBUG (SCAN_Q4: without).  (A C without instances: the caller has refused it.)
template <TileScan S, class F>
static void dispatch_scan(int C, int T, bool debug, F f) {
    auto at = [&](auto c) {
        if constexpr (scan_has_dim(S, c.value)) {
#ifdef SSW_DEBUG_HOOKS
            // (k_q4_bounds keeps its integer sums for the refine in every launch: it has no DEBUG instance)
            auto with_debug = [&](auto t) {
                if constexpr (S == SCAN_Q4) f(c, t, std::false_type{});
                else debug ? f(c, t, std::true_type{}) : f(c, t, std::false_type{});
            };
            if constexpr (c.value == 1)
                if (T == 4) return with_debug(Int<4>{});
            if constexpr (c.value <= 2)
                if (T == 2) return with_debug(Int<2>{});
            with_debug(Int<1>{});
#else
            (void)T, (void)debug;
            f(c, Int<scan_default_tiles(S, c.value)>{}, std::false_type{});
#endif
        }
    };
    C == 1 ? at(Int<1>{}) : C == 2 ? at(Int<2>{}) : C == 3 ? at(Int<3>{}) : at(Int<4>{});
}

// What the four launchers of the tile scans share: grid and T from scan_shape, then launch(grid, Int<C>, Int<T>, DEBUG)
// for the instance (the launcher has checked dim and n > 0)
template <TileScan S, class Launch>
static ssw_status launch_tile_scan(int32_t dim, int device, int64_t n, bool debug, Launch launch) {
    int grid = 1, T = 1;
    scan_shape(S, dim, device, n, &grid, &T);
    dispatch_scan<S>(dim / 256, T, debug, [&](auto c, auto t, auto d) { launch(dim3((unsigned)grid), c, t, d); });
    SSW_HIP_TRY(hipGetLastError());
    return SSW_OK;
}
static const u32x4 *as_u32x4(const void *p) { return static_cast<const u32x4 *>(p); }

ssw_status launch_q8_build(const void *X, int32_t dtype, int64_t n, int32_t dim, unsigned char *codes, float *scale,
                           float *err, hipStream_t stream) {
    if (n <= 0) return SSW_OK;
    if (!q8_dim_supported(dim) || (dtype != SSW_DTYPE_F32 && dtype != SSW_DTYPE_F16)) {
        set_error("q8_build: dim=%d, dtype=%d unsupported", dim, dtype);
        return SSW_ERR_UNSUPPORTED;
    }
    const dim3 grid((unsigned)std::min<int64_t>((n + 3) / 4, (int64_t)1 << 20)), block(256);
    int8_t *c8 = reinterpret_cast<int8_t *>(codes);
    dispatch_dim<false>(dim / 256, [&](auto c) {
        if (dtype == SSW_DTYPE_F16)
            hipLaunchKernelGGL(k_q8_build_h16<c.value>, grid, block, 0, stream, static_cast<const uint16_t *>(X), n, c8, scale, err);
        else
            hipLaunchKernelGGL(k_q8_build<c.value>, grid, block, 0, stream, static_cast<const float *>(X), n, c8, scale, err);
    });
    SSW_HIP_TRY(hipGetLastError());
    return SSW_OK;
}

ssw_status launch_q8_query(const float *q_dev, int32_t dim, float *q_keep, unsigned *state, hipStream_t stream) {
    hipLaunchKernelGGL(k_q8_query, dim3(1), dim3(256), 0, stream, q_dev, (int)dim, q_keep, state);
    SSW_HIP_TRY(hipGetLastError());
    return SSW_OK;
}

ssw_status launch_q8_bounds(const unsigned char *codes, const float *scale, const float *err, const float *q_dev,
                            const unsigned *state, float *scores, int64_t n, int32_t dim, int device,
                            hipStream_t stream) {
    if (n <= 0) return SSW_OK;
    if (!q8_dim_supported(dim)) {
        set_error("q8_bounds: dim=%d unsupported", dim);
        return SSW_ERR_UNSUPPORTED;
    }
    const int C = dim / 256;
    const int64_t rows_per_group = (int64_t)g_q8_group_loads * (4 / C);
    const int64_t need = ((n + rows_per_group - 1) / rows_per_group + 3) / 4;
    int64_t grid = (int64_t)num_cus(device) * g_q8_blocks_per_cu;  // four-wave blocks
    if (grid > need) grid = need;
    if (grid < 1) grid = 1;
    const int8_t *cd = reinterpret_cast<const int8_t *>(codes);
    dispatch_dim<false>(C, [&](auto c) {
        auto launch = [&](auto u) {
            hipLaunchKernelGGL((k_q8_bounds<c.value, u.value>), dim3((unsigned)grid), dim3(256), 0, stream, cd, scale, err,
                               q_dev, state, scores, n);
        };
#ifdef SSW_DEBUG_HOOKS
        if (g_q8_group_loads == 4) return launch(Int<4>{});
        if (g_q8_group_loads == 16) return launch(Int<16>{});
#endif
        launch(Int<Q8_GROUP_LOADS>{});
    });
    SSW_HIP_TRY(hipGetLastError());
    return SSW_OK;
}

#ifdef SSW_DEBUG_HOOKS
void tune_q8_bounds(int blocks_per_cu, int group_loads) {
    g_q8_blocks_per_cu = blocks_per_cu >= 1 && blocks_per_cu <= 8 ? blocks_per_cu : Q8_BLOCKS_PER_CU;
    g_q8_group_loads = group_loads == 4 || group_loads == 16 ? group_loads : Q8_GROUP_LOADS;
}
#endif

// the maxima of a shadow's finite constants into mx[0] (a) and mx[1] (s): after every build of the shadow, on its stream
ssw_status launch_shadow_max(const float *err, const float *scale, int64_t n, unsigned *mx, int device, hipStream_t stream) {
    SSW_HIP_TRY(hipMemsetAsync(mx, 0, SHADOW_MAX_WORDS * sizeof(unsigned), stream));
    if (n <= 0) return SSW_OK;
    int64_t grid = (int64_t)num_cus(device) * 8;
    const int64_t need = (n + 255) / 256;
    if (grid > need) grid = need;
    hipLaunchKernelGGL(k_shadow_max, dim3((unsigned)grid), dim3(256), 0, stream, err, scale, n, mx);
    SSW_HIP_TRY(hipGetLastError());
    return SSW_OK;
}

// the blocks of a survivor pass over n bounds
static dim3 survivor_grid(int device, int64_t n) {
    int64_t grid = (int64_t)num_cus(device) * 4;
    const int64_t need = (n + 1023) / 1024;  // four rows a lane
    if (grid > need) grid = need;
    if (grid < 1) grid = 1;
    return dim3((unsigned)grid);
}

ssw_status launch_survivors(const float *lb, const float *err, const unsigned *mx, int64_t n, const uint64_t *keys,
                            const int32_t *sel_count, int32_t k, unsigned *state, int64_t *rows, int64_t cap, int32_t *host_block, unsigned seq,
                            int device, hipStream_t stream) {
    hipLaunchKernelGGL(k_survivors, survivor_grid(device, n), dim3(256), 0, stream, lb, err, mx, n, keys, sel_count, k,
                       state, rows, cap);
    hipLaunchKernelGGL(k_prune_publish, dim3(1), dim3(64), 0, stream, sel_count, k, state, cap, host_block, seq);
    SSW_HIP_TRY(hipGetLastError());
    return SSW_OK;
}

size_t q8_mq_plane_bytes(int32_t dim) { return (size_t)(dim / 64) * 2 * 64 * 16; }

ssw_status launch_q8_query_mq(const float *qb_dev, int32_t dim, int32_t w, unsigned *mq, int8_t *planes, float *q_last,
                              hipStream_t stream) {
    hipLaunchKernelGGL(k_q8_query_mq, dim3(MQ_WIDTH), dim3(256), 0, stream, qb_dev, (int)dim, (int)w, mq, planes, q_last);
    SSW_HIP_TRY(hipGetLastError());
    return SSW_OK;
}

ssw_status launch_q8_bounds_mq(const unsigned char *codes, const float *scale, const float *err, const int8_t *planes,
                               const unsigned *mq, int32_t w, float *side, int64_t stride, float *own, int64_t n,
                               int32_t dim, int32_t *dbg_hi, int32_t *dbg_lo, int device, hipStream_t stream) {
    if (n <= 0) return SSW_OK;
    if (!q8_dim_supported(dim) || w < 1 || w > MQ_WIDTH) {
        set_error("q8_bounds_mq: dim=%d, w=%d unsupported", dim, w);
        return SSW_ERR_UNSUPPORTED;
    }
    return launch_tile_scan<SCAN_Q8_MQ>(dim, device, n, dbg_hi != nullptr, [&](dim3 grid, auto c, auto t, auto d) {
        hipLaunchKernelGGL((k_q8_bounds_mq<c.value, t.value, d.value>), grid, dim3(256), 0, stream,
                           reinterpret_cast<const int8_t *>(codes), scale, err, as_u32x4(planes), mq, (int)w, side, stride, own,
                           n, dbg_hi, dbg_lo);
    });
}

// code_bits: the bounds, err, scale and mx are the int8 (8: width (**)), the 6-bit (6: (***)) or the 5-bit shadow's (5: (****))
ssw_status launch_survivors_mq(const float *lb, const float *err, const float *scale, const unsigned *mx, int64_t n, int32_t dim,
                               int code_bits, const uint64_t *keys, const int32_t *sel_count, int32_t k, unsigned *slot_state,
                               int64_t *rows, int64_t cap, int device, hipStream_t stream) {
    const double code_norm = code_bits == 8 ? mq_code_norm(dim) : code_bits == 6 ? q6_code_norm(dim) : q5_code_norm(dim);
    hipLaunchKernelGGL(k_survivors_mq, survivor_grid(device, n), dim3(256), 0, stream, lb, err, scale, mx, n, code_norm, keys,
                       sel_count, k, slot_state, rows, cap);
    SSW_HIP_TRY(hipGetLastError());
    return SSW_OK;
}

ssw_status launch_prune_publish_mq(const unsigned *mq, int32_t w, int64_t cap, int32_t *host_block, unsigned seq,
                                   hipStream_t stream) {
    hipLaunchKernelGGL(k_prune_publish_mq, dim3(1), dim3(64), 0, stream, mq, (int)w, cap, host_block, seq);
    SSW_HIP_TRY(hipGetLastError());
    return SSW_OK;
}

// ---- the packed 6-bit shadow ----------------------------------------------------------------------------------------
int64_t packed_padded_rows(int64_t n) { return (n + 15) / 16 * 16; }
size_t q6_code_bytes(int64_t n, int32_t dim) { return (size_t)packed_padded_rows(n) * (size_t)dim * 3 / 4; }
size_t q6_plane_bytes(int32_t dim) { return (size_t)(dim / 64) * 64 * 16; }

// zeros for the rows past n of a packed shadow's last tile, ahead of its builder: code_bytes of codes in tiles of
// tile_bytes, packed_padded_rows floats of scale and err
static ssw_status zero_last_tile(unsigned char *codes, size_t code_bytes, size_t tile_bytes, float *scale, float *err, int64_t n,
                                 hipStream_t stream) {
    const int64_t np = packed_padded_rows(n);
    if (np == n) return SSW_OK;
    SSW_HIP_TRY(hipMemsetAsync(codes + code_bytes - tile_bytes, 0, tile_bytes, stream));
    SSW_HIP_TRY(hipMemsetAsync(scale + np - 16, 0, 16 * sizeof(float), stream));
    SSW_HIP_TRY(hipMemsetAsync(err + np - 16, 0, 16 * sizeof(float), stream));
    return SSW_OK;
}

// codes / scale / err: q6_code_bytes and packed_padded_rows floats each; the rows past n of the last tile get zeros
ssw_status launch_q6_build(const void *X, int32_t dtype, int64_t n, int32_t dim, unsigned char *codes, float *scale,
                           float *err, hipStream_t stream) {
    if (n <= 0) return SSW_OK;
    if (!q6_dim_supported(dim) || (dtype != SSW_DTYPE_F32 && dtype != SSW_DTYPE_F16)) {
        set_error("q6_build: dim=%d, dtype=%d unsupported", dim, dtype);
        return SSW_ERR_UNSUPPORTED;
    }
    SSW_TRY(zero_last_tile(codes, q6_code_bytes(n, dim), (size_t)16 * dim * 3 / 4, scale, err, n, stream));
    const dim3 grid((unsigned)std::min<int64_t>((n + 3) / 4, (int64_t)1 << 20)), block(256);
    dispatch_dim<true>(dim / 256, [&](auto c) {
        if (dtype == SSW_DTYPE_F16)
            hipLaunchKernelGGL(k_q6_build_h16<c.value>, grid, block, 0, stream, static_cast<const uint16_t *>(X), n, codes, scale, err);
        else
            hipLaunchKernelGGL(k_q6_build<c.value>, grid, block, 0, stream, static_cast<const float *>(X), n, codes, scale, err);
    });
    SSW_HIP_TRY(hipGetLastError());
    return SSW_OK;
}

// st: Q8_MQ_WORDS words (a slot's of the chunk); planes: q6_plane_bytes(dim), zeroed when they were allocated
ssw_status launch_q6_query(const float *q_dev, int32_t dim, unsigned *st, int8_t *planes, float *q_keep,
                           hipStream_t stream) {
    hipLaunchKernelGGL(k_q6_query, dim3(1), dim3(256), 0, stream, q_dev, (int)dim, st, planes, q_keep);
    SSW_HIP_TRY(hipGetLastError());
    return SSW_OK;
}

ssw_status launch_q6_bounds(const unsigned char *codes, const float *scale, const float *err, const int8_t *planes,
                            const unsigned *st, float *scores, int64_t n, int32_t dim, int64_t *dbg_I, int device,
                            hipStream_t stream) {
    if (n <= 0) return SSW_OK;
    if (!q6_dim_supported(dim)) {
        set_error("q6_bounds: dim=%d unsupported", dim);
        return SSW_ERR_UNSUPPORTED;
    }
    return launch_tile_scan<SCAN_Q6>(dim, device, n, dbg_I != nullptr, [&](dim3 grid, auto c, auto t, auto d) {
        hipLaunchKernelGGL((k_q6_bounds<c.value, t.value, d.value>), grid, dim3(256), 0, stream, as_u32x4(codes), scale, err,
                           as_u32x4(planes), st, scores, n, dbg_I);
    });
}

// ---- a chunk of up to 16 queries on the 6-bit shadow ------------------------------------------------------------------
// planes: q8_mq_plane_bytes(dim), the int8 chunk's buffer
ssw_status launch_q6_query_mq(const float *qb_dev, int32_t dim, int32_t w, unsigned *mq, int8_t *planes, float *q_last,
                              hipStream_t stream) {
    hipLaunchKernelGGL(k_q6_query_mq, dim3(MQ_WIDTH), dim3(256), 0, stream, qb_dev, (int)dim, (int)w, mq, planes, q_last);
    SSW_HIP_TRY(hipGetLastError());
    return SSW_OK;
}

ssw_status launch_q6_bounds_mq(const unsigned char *codes, const float *scale, const float *err, const int8_t *planes,
                               const unsigned *mq, int32_t w, float *side, int64_t stride, float *own, int64_t n,
                               int32_t dim, int64_t *dbg_I, int device, hipStream_t stream) {
    if (n <= 0) return SSW_OK;
    if (!q6_dim_supported(dim) || w < 1 || w > MQ_WIDTH) {
        set_error("q6_bounds_mq: dim=%d, w=%d unsupported", dim, w);
        return SSW_ERR_UNSUPPORTED;
    }
    return launch_tile_scan<SCAN_Q6_MQ>(dim, device, n, dbg_I != nullptr, [&](dim3 grid, auto c, auto t, auto d) {
        hipLaunchKernelGGL((k_q6_bounds_mq<c.value, t.value, d.value>), grid, dim3(256), 0, stream, as_u32x4(codes), scale, err,
                           as_u32x4(planes), mq, (int)w, side, stride, own, n, dbg_I);
    });
}

// ---- the packed 5-bit shadow ----------------------------------------------------------------------------------------
bool q5_dim_supported(int32_t dim) { return dim == 512 || dim == 1024; }
size_t q5_code_bytes(int64_t n, int32_t dim) { return (size_t)packed_padded_rows(n) * (size_t)dim * 5 / 8; }

// codes / scale / err: q5_code_bytes and packed_padded_rows floats each; the rows past n of the last tile get zeros
ssw_status launch_q5_build(const void *X, int32_t dtype, int64_t n, int32_t dim, unsigned char *codes, float *scale,
                           float *err, hipStream_t stream) {
    if (n <= 0) return SSW_OK;
    if (!q5_dim_supported(dim) || dtype != SSW_DTYPE_F32) {
        set_error("q5_build: dim=%d, dtype=%d unsupported", dim, dtype);
        return SSW_ERR_UNSUPPORTED;
    }
    SSW_TRY(zero_last_tile(codes, q5_code_bytes(n, dim), (size_t)16 * dim * 5 / 8, scale, err, n, stream));
    const dim3 grid((unsigned)std::min<int64_t>((n + 3) / 4, (int64_t)1 << 20)), block(256);
    const float *Xf = static_cast<const float *>(X);
    if (dim == 512) hipLaunchKernelGGL(k_q5_build<2>, grid, block, 0, stream, Xf, n, codes, scale, err);
    else hipLaunchKernelGGL(k_q5_build<4>, grid, block, 0, stream, Xf, n, codes, scale, err);
    SSW_HIP_TRY(hipGetLastError());
    return SSW_OK;
}

ssw_status launch_q5_bounds(const unsigned char *codes, const float *scale, const float *err, const int8_t *planes,
                            const unsigned *st, float *scores, int64_t n, int32_t dim, int64_t *dbg_I, int device,
                            hipStream_t stream) {
    if (n <= 0) return SSW_OK;
    if (!q5_dim_supported(dim)) {
        set_error("q5_bounds: dim=%d unsupported", dim);
        return SSW_ERR_UNSUPPORTED;
    }
    return launch_tile_scan<SCAN_Q5>(dim, device, n, dbg_I != nullptr, [&](dim3 grid, auto c, auto t, auto d) {
        hipLaunchKernelGGL((k_q5_bounds<c.value, t.value, d.value>), grid, dim3(256), 0, stream, as_u32x4(codes), scale, err,
                           as_u32x4(planes), st, scores, n, dbg_I);
    });
}

// ---- the two-stage 4 + 1-bit shadow ---------------------------------------------------------------------------------
size_t q41_coarse_bytes(int64_t n, int32_t dim) { return (size_t)packed_padded_rows(n) * (size_t)dim / 2; }
size_t q41_fine_bytes(int64_t n, int32_t dim) { return (size_t)packed_padded_rows(n) * (size_t)dim / 8; }

ssw_status launch_q41_build(const void *X, int32_t dtype, int64_t n, int32_t dim, unsigned char *coarse, unsigned *fine,
                            float *scale, float *err, float *err4, hipStream_t stream) {
    if (n <= 0) return SSW_OK;
    if (!q5_dim_supported(dim) || dtype != SSW_DTYPE_F32) {
        set_error("q41_build: dim=%d, dtype=%d unsupported", dim, dtype);
        return SSW_ERR_UNSUPPORTED;
    }
    SSW_TRY(zero_last_tile(coarse, q41_coarse_bytes(n, dim), (size_t)16 * dim / 2, scale, err, n, stream));
    const int64_t np = packed_padded_rows(n);
    if (np != n) {
        SSW_HIP_TRY(hipMemsetAsync(err4 + np - 16, 0, 16 * sizeof(float), stream));
        SSW_HIP_TRY(hipMemsetAsync(fine + (np - 16) * (dim / 32), 0, (size_t)16 * dim / 8, stream));
    }
    const dim3 grid((unsigned)std::min<int64_t>((n + 3) / 4, (int64_t)1 << 20)), block(256);
    const float *Xf = static_cast<const float *>(X);
    if (dim == 512) hipLaunchKernelGGL(k_q41_build<2>, grid, block, 0, stream, Xf, n, coarse, fine, scale, err, err4);
    else hipLaunchKernelGGL(k_q41_build<4>, grid, block, 0, stream, Xf, n, coarse, fine, scale, err, err4);
    SSW_HIP_TRY(hipGetLastError());
    return SSW_OK;
}

ssw_status launch_q41_query(const float *q_dev, int32_t dim, unsigned *st, int8_t *planes, float *q_keep, int32_t *D,
                            unsigned *cstate, hipStream_t stream) {
    hipLaunchKernelGGL(k_q41_query, dim3(1), dim3(256), 0, stream, q_dev, (int)dim, st, planes, q_keep, D, cstate);
    SSW_HIP_TRY(hipGetLastError());
    return SSW_OK;
}

ssw_status launch_q4_bounds(const unsigned char *coarse, const float *scale, const float *err4, const int8_t *planes,
                            const unsigned *st, float *scores, int32_t *H, int64_t n, int32_t dim, int device,
                            hipStream_t stream) {
    if (n <= 0) return SSW_OK;
    if (!q5_dim_supported(dim)) {
        set_error("q4_bounds: dim=%d unsupported", dim);
        return SSW_ERR_UNSUPPORTED;
    }
    return launch_tile_scan<SCAN_Q4>(dim, device, n, false, [&](dim3 grid, auto c, auto t, auto d) {
        hipLaunchKernelGGL((k_q4_bounds<c.value, t.value, d.value>), grid, dim3(256), 0, stream, as_u32x4(coarse), scale, err4,
                           as_u32x4(planes), st, scores, H, n);
    });
}

ssw_status launch_survivors_q4(const float *lb4, const float *err4, const float *scale, const unsigned *mx, int64_t n,
                               int32_t dim, const uint64_t *keys, const int32_t *sel_count, int32_t k, unsigned *st,
                               unsigned *cstate, uint32_t *rows32, int64_t list_cap, int blocks, int device,
                               hipStream_t stream) {
    const dim3 grid = blocks > 0 ? dim3((unsigned)blocks) : survivor_grid(device, n);
    hipLaunchKernelGGL(k_survivors_q4, grid, dim3(256), 0, stream, lb4, err4, scale, mx, n, q4_code_norm(dim), keys, sel_count, k,
                       st, cstate, rows32, list_cap);
    SSW_HIP_TRY(hipGetLastError());
    return SSW_OK;
}

ssw_status launch_q41_refine(const int32_t *H, const unsigned *fine, const float *scale, const float *err, const int32_t *D,
                             const uint64_t *keys, int32_t k, unsigned *st, unsigned *cstate, const uint32_t *rows32,
                             int64_t coarse_cap, int64_t n, int32_t dim, int64_t *rows, int64_t cap, float *dbg_lb5,
                             int32_t *dbg_B, int device, hipStream_t stream) {
    if (n <= 0) return SSW_OK;
    if (!q5_dim_supported(dim)) {
        set_error("q41_refine: dim=%d unsupported", dim);
        return SSW_ERR_UNSUPPORTED;
    }
    // without the count: enough waves to hide the gathers' latency, no more blocks than a dense pass has steps
    const int64_t step = (int64_t)4 * (64 / (dim / 32)) * REFINE_UNROLL;  // rows a block takes at a time
    int64_t grid = (int64_t)num_cus(device) * 8;
    if (grid > (n + step - 1) / step) grid = (n + step - 1) / step;
    auto launch = [&](auto c, auto d) {
        hipLaunchKernelGGL((k_q41_refine<c.value, d.value>), dim3((unsigned)grid), dim3(256), 0, stream, H, fine, scale, err, D,
                           keys, k, st, cstate, rows32, coarse_cap, n, rows, cap, dbg_lb5, dbg_B);
    };
    auto with_dim = [&](auto d) { dim == 512 ? launch(Int<2>{}, d) : launch(Int<4>{}, d); };
#ifdef SSW_DEBUG_HOOKS
    if (dbg_lb5 != nullptr) with_dim(std::true_type{});
    else
#endif
        with_dim(std::false_type{});
    SSW_HIP_TRY(hipGetLastError());
    return SSW_OK;
}

ssw_status launch_prune_publish_q41(const unsigned *st, const unsigned *cstate, int64_t cap, int32_t *host_block,
                                    unsigned seq, hipStream_t stream) {
    hipLaunchKernelGGL(k_prune_publish_q41, dim3(1), dim3(64), 0, stream, st, cstate, cap, host_block, seq);
    SSW_HIP_TRY(hipGetLastError());
    return SSW_OK;
}

ssw_status launch_candidate_rows(const uint64_t *keys, const int32_t *sel_count, int32_t kc, int64_t n, int64_t *rows_out,
                                 hipStream_t stream) {
    hipLaunchKernelGGL(k_candidate_rows, dim3((unsigned)((kc + 255) / 256)), dim3(256), 0, stream, keys, sel_count, kc, n, rows_out);
    SSW_HIP_TRY(hipGetLastError());
    return SSW_OK;
}

ssw_status launch_exact_threshold(uint64_t *keys, const int32_t *sel_count, const float *vals, int32_t k, int32_t kc,
                                  hipStream_t stream) {
    if (k < 1 || kc < k || kc > TX_KEYS) {
        set_error("exact_threshold: k=%d, kc=%d outside [1, %d]", k, kc, TX_KEYS);
        return SSW_ERR_INVALID;
    }
    int P = TX_THREADS;
    while (P < kc) P <<= 1;
    hipLaunchKernelGGL(k_exact_threshold, dim3(1), dim3(TX_THREADS), 0, stream, keys, sel_count, vals, k, kc, P);
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

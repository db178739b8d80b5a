// index_mc.hip -- large-batch top-k on the matrix cores (ssw_index_topk_batch_mc; gfx950 / MI355X)
//
// The batched scan (index_batch.hip) reads the rows once per chunk of 16 queries and multiplies on the vector ALUs.  Here
// a GROUP of up to 1024 queries is scored in ONE pass over the rows, in place, on v_mfma_f32_16x16x32_f16, and every
// query's answer is the bits of ssw_index_topk.  The recipe is the k-NN builder's (knn.hip) turned rectangular and
// index-stationary:
//
//   1. stats        maxabs and an upper bound of the largest row norm, once per index (kept in the handle beside the
//                   shadows and stale where they are); scale = 2^e with scale * maxabs in [128, 256).
//   2. queries      Qh = fp16(scale_q Q) for the group (scale_q a power of two from the group's maxabs), norms on the device.
//   3. candidates   a workgroup owns a STRIP of R consecutive rows (128 at dim <= 512, 64 above): it reads them once from
//                   HBM -- f32 or f16 rows, widened, scaled, rounded to fp16 -- and writes all of K into LDS in the
//                   swizzled fragment layout of knn.hip (a 64-element K-slice of the strip is one operand image).  Then
//                   it walks the group's query tiles (128 queries): K-slices of Qh stream from L2 into a two-stage ring
//                   by LDS-DMA, the accumulators are compared with each query's threshold and the survivors appended
//                   (score, row) to that query's buffer, one atomic a survivor.  No copy of the index is made.
//   4. levels       strips are dealt to levels in a seeded random order: the first level holds MC_CAP rows (a buffer
//                   takes all of them), later ones grow by a constant ratio <= MC_CAP / (2 M); between levels one
//                   workgroup a query keeps the best M and raises the threshold to the M-th score, so a level appends
//                   ~ M x ratio <= MC_CAP / 2 entries a query whatever the data looks like.
//   5. finish       one workgroup a query rescores its <= M candidates with the scan's lane arithmetic (rescore_rows.h),
//                   sorts by (score desc, row asc), keeps the first row of each image, strikes out excluded images,
//                   takes k and certifies the list.
//   6. fallback     uncertified or overflowed queries go once through ssw_index_topk_batch with their own exclusions.
//
// Certificate.  A row outside the list has fp16-path score <= b (the final threshold, unscaled), so its scan score is
// <= b + E; the query is proven when score(k-th accepted) - E > b (strictly: a tie with an outside row is never decided
// here), or when no threshold was ever raised (the list holds every row).
// E: write a = scale x, c = scale_q q (exact: powers of two).  Components of |v| >= 2^-14 round to fp16 within 2^-11 |v|;
// smaller ones may be flushed by the matrix core, an error <= 2^-14.  With da, dc the operand errors
//   sum |ah ch - a c| <= sum |a||dc| + |c||da| + |da||dc|
//                    <= (2^-10 + 2^-22) |a||c| + 2^-14 (1 + 2^-11) sqrt(D) (|a| + |c|) + D 2^-28.
// fp16 products are exact in f32; the f32 accumulation of D <= 1024 terms (truncating adds assumed, knn.hip) adds
// <= D 2^-23 |ah||ch| <= 2^-13 (1 + 2^-10) |a||c|.  The scan score itself is within 15 roundings, < 2^-20 |x||q|, of the
// real product (2 C <= 8 fma, one add, six butterfly adds).  Divided by scale scale_q, with 1 / scale <= maxabs_x / 128,
// 1 / scale_q <= maxabs_q / 128 and sqrt(D) <= 32:
//   E <= (2^-10 + 2^-13 + 2^-20 + 3 2^-22) |x||q|                                  = 1.1003e-3 |x||q|
//        + 2^-16 (1 + 2^-11) (|x| maxabs_q + |q| maxabs_x)                         = 1.527e-5 (...)
//        + 2^-32 maxabs_x maxabs_q                                                 = 2.4e-10 maxabs_x maxabs_q.
// f16 rows scale exactly, so da is the flushed tail alone and the first line is 2^-11 + 2^-13 + 2^-20 = 6.113e-4.
// The kernel uses 1.2e-3 (f16 rows: 6.5e-4), 1.6e-5 and 1e-9 with |x| <= maxnorm and |q| rounded up: 6 % and more of
// margin for its own f32 evaluation.  Largest elements outside [2^-40, 2^40] are not bounded at all (plain batch).
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <vector>

#include "index_handle.h"
#include "rescore_rows.h"

using namespace ssw;

namespace {

typedef _Float16 f16;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(4))) _Float16 f16x4;

constexpr int MC_GROUP = 1024;      // queries of one pass over the rows
constexpr int MC_CAP = 4096;        // entries of a query's buffer: 32 MiB for a group
constexpr int MC_MAX_K = 128;       // M = 4 k <= 512
constexpr int MC_QT = 128;          // queries of a tile
constexpr int MC_BK = 64;           // elements of a K-slice: 128 bytes a row
constexpr int MC_STAGE = MC_QT * 128;   // one K-slice of a query tile
constexpr int MC_RING = 2 * MC_STAGE;   // the ring sits at LDS offset 0, the strip behind it
constexpr int64_t MC_MAX_LAUNCH = (int64_t)1 << 22;  // strips of one launch: 2^22 x 512 work-items < 2^32
constexpr float MC_MIN_ABS = 9.094947e-13f, MC_MAX_ABS = 1.0995116e12f;  // 2^-40, 2^40

// ---- 1. stats ---------------------------------------------------------------------------------------------------------
// maxima[0] = the largest |element| (+inf if any is NaN), maxima[1] = an upper bound of the largest norm; f16 rows are
// read group by group in storage order (neither figure depends on the order)
template <bool H16>
__global__ __launch_bounds__(256) void k_mc_stats(const void *__restrict__ Xv, int64_t n, int D,
                                                  unsigned *__restrict__ maxima) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), waves = (int64_t)gridDim.x * 4;
    float mx_all = 0.f, nr_all = 0.f;
    for (int64_t r = wave; r < n; r += waves) {
        float ss = 0.f, mx = 0.f;
        for (int g = lane; g < D / 4; g += 64) {
            float4 v;
            if constexpr (H16) v = widen_h16x4(reinterpret_cast<const u32x2 *>(Xv)[r * (D / 4) + g]);
            else v = reinterpret_cast<const float4 *>(Xv)[r * (D / 4) + g];
            const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                ss = fmaf(e[i], e[i], ss);
                mx = e[i] != e[i] ? INFINITY : fmaxf(mx, fabsf(e[i]));
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            ss += __shfl_xor(ss, off, 64);
            mx = fmaxf(mx, __shfl_xor(mx, off, 64));
        }
        mx_all = fmaxf(mx_all, mx);
        nr_all = fmaxf(nr_all, sqrtf(ss) * 1.0001f);  // f32 sum of squares: ~3e-5 relative
    }
    if (lane == 0) {
        atomicMax(&maxima[0], __float_as_uint(mx_all));  // non-negative floats order like their bits
        atomicMax(&maxima[1], __float_as_uint(nr_all));
    }
}

__global__ void k_mc_clear(unsigned *__restrict__ words, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) words[i] = 0u;
}

// ---- 2. queries -------------------------------------------------------------------------------------------------------
// one wave a padded query: Qh row, norm (rounded up), and the query's state reset; queries from nq on are zero rows
// whose threshold +inf keeps them out of every buffer
__global__ __launch_bounds__(256) void k_mc_prep(const float *__restrict__ Qf, int nq, int qp, int D, float scale_q,
                                                 f16 *__restrict__ Qh, float *__restrict__ qnorm, float *__restrict__ thr,
                                                 unsigned *__restrict__ cnt, unsigned *__restrict__ kept,
                                                 unsigned *__restrict__ ovf, unsigned long long *__restrict__ appended) {
    const int lane = threadIdx.x & 63;
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (blockIdx.x == 0 && threadIdx.x == 0) *appended = 0ull;
    if (q >= qp) return;
    float ss = 0.f;
    for (int c = lane * 4; c < D; c += 256) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (q < nq) v = *reinterpret_cast<const float4 *>(Qf + (int64_t)q * D + c);
        ss = fmaf(v.x, v.x, fmaf(v.y, v.y, fmaf(v.z, v.z, fmaf(v.w, v.w, ss))));
        f16x4 o;
        o[0] = (f16)(v.x * scale_q), o[1] = (f16)(v.y * scale_q), o[2] = (f16)(v.z * scale_q), o[3] = (f16)(v.w * scale_q);
        *reinterpret_cast<f16x4 *>(Qh + (int64_t)q * D + c) = o;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) ss += __shfl_xor(ss, off, 64);
    if (lane == 0) {
        qnorm[q] = sqrtf(ss) * 1.0001f;
        thr[q] = q < nq ? -INFINITY : INFINITY;
        cnt[q] = 0u, kept[q] = 0u, ovf[q] = 0u;
    }
}

// ---- 3. candidates: the strip stays in LDS, the queries stream past it --------------------------------------------------
// LDS: [ring: 2 stages x (128 queries x 128 B)] [strip: D / 64 K-slices x (R rows x 128 B)].  Both kinds of image are
// knn.hip's: row r at r * 128, its 16-byte chunk c at position c ^ ((r >> 1) & 7).  Eight waves, WM x WN: a wave
// multiplies NI x 16 queries with 32 rows of the strip.  The queries are the operand whose index a lane keeps across the
// four accumulator registers (k_knn_gemm_filter<false>'s rows), so one threshold serves a register quad:
//   acc[i][j][r] = S~[query T * 128 + wm * NI * 16 + i * 16 + fr][row row0 + wn * 32 + j * 16 + fq * 4 + r].
template <int D, int R, bool H16>
__global__ __launch_bounds__(512) void k_mc_candidates(const void *__restrict__ Xv, int64_t n, float scale,
                                                       const int32_t *__restrict__ strips, const f16 *__restrict__ Qh,
                                                       int q_tiles, const float *__restrict__ thr,
                                                       unsigned *__restrict__ cnt, uint64_t *__restrict__ buf) {
    extern __shared__ __attribute__((aligned(1024))) unsigned char smem[];
    constexpr int NK = D / MC_BK, SLICE = R * 128, CH = D / 8;
    constexpr int WN = R / 32, WM = 8 / WN, NI = MC_QT / WM / 16;
    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int64_t row0 = (int64_t)strips[blockIdx.x] * R;
    unsigned char *strip = smem + MC_RING;

    // the strip, through registers: eight natural elements a step -> one 16-byte chunk of its K-slice
#pragma unroll 4
    for (int idx = t; idx < R * CH; idx += 512) {
        const int row = idx / CH, ch = idx % CH;
        const int64_t g = row0 + row;
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;  // rows past the index: zeros, never appended
        if (g < n) {
            if constexpr (H16) {
                const uint16_t *x = reinterpret_cast<const uint16_t *>(Xv) + g * D;
                a = widen_h16x4(*reinterpret_cast<const u32x2 *>(x + h16_group_pos(ch * 8, D / 256)));
                b = widen_h16x4(*reinterpret_cast<const u32x2 *>(x + h16_group_pos(ch * 8 + 4, D / 256)));
            } else {
                const float4 *x = reinterpret_cast<const float4 *>(reinterpret_cast<const float *>(Xv) + g * D + ch * 8);
                a = x[0], b = x[1];
            }
        }
        f16x8 o;
        o[0] = (f16)(a.x * scale), o[1] = (f16)(a.y * scale), o[2] = (f16)(a.z * scale), o[3] = (f16)(a.w * scale);
        o[4] = (f16)(b.x * scale), o[5] = (f16)(b.y * scale), o[6] = (f16)(b.z * scale), o[7] = (f16)(b.w * scale);
        *reinterpret_cast<f16x8 *>(strip + (ch >> 3) * SLICE + row * 128 + (((ch & 7) ^ ((row >> 1) & 7)) << 4)) = o;
    }
    __syncthreads();

    // the ring: a stage is 16 pieces of 8 queries x 128 B, two a wave (knn.hip's a_src)
    const f16 *q_src[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int row = (wave * 2 + i) * 8 + (lane >> 3);
        const int chunk = (lane & 7) ^ ((row >> 1) & 7);
        q_src[i] = Qh + (int64_t)row * D + chunk * 8;
    }
    const unsigned lds0 = (unsigned)(size_t)((__attribute__((address_space(3))) unsigned char *)smem);
    const unsigned q_dst = lds0 + wave * 2048;
#define MC_ISSUE(T, kt, slot)                                                                               \
    {                                                                                                       \
        _Pragma("unroll") for (int i = 0; i < 2; ++i)                                                       \
            glds16(q_src[i] + (int64_t)(T) * MC_QT * D + (kt) * MC_BK, q_dst + (slot) * MC_STAGE + i * 1024); \
    }
    const int fr = lane & 15, fq = lane >> 4;
    const int frag0 = fr * 128 + ((fq ^ (fr >> 1)) << 4);
    const int wm = wave / WN, wn = wave % WN;
    const int a_frag = wm * (NI * 2048) + frag0, b_frag = wn * 4096 + frag0;
    asm volatile("" ::"s"(cnt), "s"(buf), "s"(thr));  // scalar loads done before the loop (gemm_bf16.hip)
    MC_ISSUE(0, 0, 0)
    int slot = 0;
    for (int T = 0; T < q_tiles; ++T) {
        float trow[NI];
#pragma unroll
        for (int i = 0; i < NI; ++i) trow[i] = thr[T * MC_QT + wm * (NI * 16) + i * 16 + fr];
        f32x4 acc[NI][2];
#pragma unroll
        for (int i = 0; i < NI; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
        for (int kt = 0; kt < NK; ++kt) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            // the ring never drains between tiles: the next tile's first slice is requested while this tile's last
            // slice multiplies and its epilogue runs
            if (kt + 1 < NK) {
                MC_ISSUE(T, kt + 1, slot ^ 1)
            } else if (T + 1 < q_tiles) {
                MC_ISSUE(T + 1, 0, slot ^ 1)
            }
            const unsigned char *sa = smem + slot * MC_STAGE;
            const unsigned char *sb = strip + kt * SLICE;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                f16x8 a[NI], b[2];
#pragma unroll
                for (int i = 0; i < NI; ++i)
                    a[i] = *reinterpret_cast<const f16x8 *>(sa + ((a_frag + i * 2048) ^ (ks * 64)));
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    b[j] = *reinterpret_cast<const f16x8 *>(sb + ((b_frag + j * 2048) ^ (ks * 64)));
#pragma unroll
                for (int i = 0; i < NI; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(b[j], a[i], acc[i][j], 0, 0, 0);
            }
            asm volatile("" ::: "memory");
            slot ^= 1;
        }
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const float tr = trow[i];
            const int q = T * MC_QT + wm * (NI * 16) + i * 16 + fr;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const f32x4 v = acc[i][j];
                if (fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3])) > tr) {
                    const int64_t row = row0 + wn * 32 + j * 16 + fq * 4;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        if (v[r] > tr && row + r < n) {
                            const unsigned pos = atomicAdd(&cnt[q], 1u);
                            if (pos < (unsigned)MC_CAP)
                                buf[(int64_t)q * MC_CAP + pos] =
                                    ((uint64_t)f32_to_ord(v[r]) << 32) | (uint64_t)(0xFFFFFFFFu - (unsigned)(row + r));
                        }
                    }
                }
            }
        }
    }
#undef MC_ISSUE
}

// descending bitonic sort of P (a power of two >= 64) keys in LDS by 256 threads (k_knn_compact's network)
__device__ __forceinline__ void mc_sort_desc(uint64_t *keys, int P) {
    for (int size = 2; size <= P; size <<= 1) {
        for (int stride = size >> 1; stride >= 1; stride >>= 1) {
            for (int i = threadIdx.x; i < P / 2; i += 256) {
                const int lo = 2 * i - (i & (stride - 1));  // index with bit `stride` clear
                const int hi = lo + stride;
                const bool desc = (lo & size) == 0;
                const uint64_t a = keys[lo], b = keys[hi];
                if ((a < b) == desc) {
                    keys[lo] = b;
                    keys[hi] = a;
                }
            }
            __syncthreads();
        }
    }
}

// ---- 4. between levels: keep the best M of a query's entries, raise its threshold ----------------------------------------
__global__ __launch_bounds__(256) void k_mc_compact(uint64_t *__restrict__ buf, unsigned *__restrict__ cnt,
                                                    unsigned *__restrict__ kept, float *__restrict__ thr,
                                                    unsigned *__restrict__ ovf, unsigned long long *__restrict__ appended,
                                                    int M) {
    __shared__ uint64_t keys[MC_CAP];
    const int q = blockIdx.x;
    unsigned c = cnt[q];
    __syncthreads();  // everybody has read the count before thread 0 rewrites it
    if (threadIdx.x == 0) atomicAdd(appended, (unsigned long long)(c - kept[q]));
    if (c > (unsigned)MC_CAP) {  // entries were dropped: the query cannot be certified any more
        if (threadIdx.x == 0) ovf[q] = 1u;
        c = MC_CAP;
    }
    if (c > 1) {
        int P = 64;
        while (P < (int)c) P <<= 1;
        uint64_t *qb = buf + (int64_t)q * MC_CAP;
        for (int i = threadIdx.x; i < P; i += 256) keys[i] = i < (int)c ? qb[i] : 0ull;
        __syncthreads();
        mc_sort_desc(keys, P);
        const int keep = (int)c < M ? (int)c : M;
        for (int i = threadIdx.x; i < keep; i += 256) qb[i] = keys[i];
    }
    if (threadIdx.x == 0) {
        const unsigned keep = c < (unsigned)M ? c : (unsigned)M;
        cnt[q] = keep, kept[q] = keep;
        if (c >= (unsigned)M) thr[q] = ord_to_f32((uint32_t)(keys[M - 1] >> 32));  // (M >= 64 > 1: the keys are sorted)
    }
}

// ---- 5. finish ----------------------------------------------------------------------------------------------------------
struct McFinishArgs {
    const float *Qf, *qnorm, *thr;
    const unsigned *cnt, *ovf;
    const uint64_t *buf;
    const int64_t *row_start;  // NULL: image = row
    int64_t n_images;
    const int64_t *ex_off, *ex_ids;  // ids ascending within a query's list
    int M, k;
    float inv_scale, inv_scale_q, eps_rel, maxnorm, maxabs_x, maxabs_q;
    int64_t *out_images, *out_rows;
    float *out_scores;
    int32_t *out_counts, *out_flags;  // flag 0: proven, 1: not certified, 2: its buffer overflowed
    float *out_bE;                    // [nq][2] b and E as evaluated below; NULL in the product (the lab hook's view)
};

template <class Rw, int C>
__global__ __launch_bounds__(256) void k_mc_finish(const typename Rw::T *__restrict__ X, McFinishArgs a) {
    constexpr int PMAX = 4 * MC_MAX_K;
    __shared__ uint64_t keys[PMAX];
    __shared__ int64_t img[PMAX];
    __shared__ unsigned char ok[PMAX];
    __shared__ int bad;
    const int q = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int c = min((int)a.cnt[q], a.M);
    int P = 64;
    while (P < c) P <<= 1;
    if (t == 0) bad = 0;
    for (int i = t; i < P; i += 256) keys[i] = 0ull;  // below every key of a finite score
    __syncthreads();
    // exact scores, the scan's bits: one wave a candidate
    const rows::Frag<C> qf = rows::load_query<C>(a.Qf + (int64_t)q * (C * 256), lane);
    for (int e = wave; e < c; e += 4) {
        const uint32_t row = 0xFFFFFFFFu - (uint32_t)a.buf[(int64_t)q * MC_CAP + e];
        const rows::Frag<C> x = Rw::template load<C>(X, (int64_t)row, lane);
        const float v = rows::wave_sum(rows::lane_partial<C>(x, qf));
        if (lane == 0) {
            if (!(fabsf(v) <= FLT_MAX)) bad = 1;  // an overflowed product: the plain batch decides
            keys[e] = ((uint64_t)f32_to_ord(v) << 32) | (uint64_t)(0xFFFFFFFFu - row);
        }
    }
    __syncthreads();
    mc_sort_desc(keys, P);  // (score desc, row asc)
    const int64_t ex0 = a.ex_off[q], ex1 = a.ex_off[q + 1];
    for (int i = t; i < c; i += 256) {
        const int64_t row = (int64_t)(0xFFFFFFFFu - (uint32_t)keys[i]);
        int64_t im = row;
        if (a.row_start) {  // the last image whose first row is at or before `row`
            int64_t lo = 0, hi = a.n_images;
            while (hi - lo > 1) {
                const int64_t mid = lo + ((hi - lo) >> 1);
                if (a.row_start[mid] <= row) lo = mid;
                else hi = mid;
            }
            im = lo;
        }
        int64_t lo = ex0, hi = ex1;  // the first listed id >= im
        while (lo < hi) {
            const int64_t mid = lo + ((hi - lo) >> 1);
            if (a.ex_ids[mid] < im) lo = mid + 1;
            else hi = mid;
        }
        img[i] = im;
        ok[i] = !(lo < ex1 && a.ex_ids[lo] == im);
    }
    __syncthreads();
    if (a.row_start) {  // an image's first occurrence is its best row, the lowest on ties; the later ones go
        for (int i = t; i < c; i += 256) {
            const int64_t im = img[i];
            bool dup = false;
            for (int j = 0; j < i; ++j) dup |= img[j] == im;
            if (dup) ok[i] = 0;
        }
        __syncthreads();
    }
    if (t == 0) {
        int rank = 0;
        float s_k = -INFINITY;
        for (int i = 0; i < c && rank < a.k; ++i) {
            if (!ok[i]) continue;
            s_k = ord_to_f32((uint32_t)(keys[i] >> 32));
            const int64_t o = (int64_t)q * a.k + rank;
            a.out_images[o] = img[i];
            a.out_rows[o] = (int64_t)(0xFFFFFFFFu - (uint32_t)keys[i]);
            a.out_scores[o] = s_k;
            ++rank;
        }
        const float thr = a.thr[q], qn = a.qnorm[q];
        const float b = thr * a.inv_scale * a.inv_scale_q;
        const float E = a.eps_rel * qn * a.maxnorm + 1.6e-5f * (a.maxnorm * a.maxabs_q + qn * a.maxabs_x) +
                        1e-9f * a.maxabs_x * a.maxabs_q;
        const bool all_rows = thr == -INFINITY;  // never M entries: every row of the index is in the list
        const bool proven = !bad && (all_rows || (rank == a.k && s_k - E > b));
        a.out_counts[q] = rank;
        a.out_flags[q] = a.ovf[q] ? 2 : (proven ? 0 : 1);
        if (a.out_bE) a.out_bE[2 * q] = b, a.out_bE[2 * q + 1] = E;
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------
inline uint64_t splitmix64(uint64_t &s) {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

int strip_rows(int32_t dim) { return dim <= 512 ? 128 : 64; }

// maxabs and maxnorm of the rows: one pass and one wait, once per state of the rows
ssw_status rows_stats(ssw_index *idx) {
    PruneState &p = idx->prune;
    McState &mc = idx->mc;
    if (!idx->owns_X || idx->rows_escaped) p.rows_stats_stale = true;  // somebody else may write the rows
    if (!p.rows_stats_stale) return SSW_OK;
    if (!mc.maxima) SSW_HIP_TRY(hipMalloc((void **)&mc.maxima, 2 * sizeof(unsigned)));
    float mx[2] = {0.f, 0.f};
    if (idx->n > 0) {
        hipLaunchKernelGGL(k_mc_clear, dim3(1), dim3(64), 0, idx->stream, mc.maxima, 2);
        const dim3 grid((unsigned)std::min<int64_t>((idx->n + 3) / 4, 4096));
        if (idx->dtype == SSW_DTYPE_F16)
            hipLaunchKernelGGL(k_mc_stats<true>, grid, dim3(256), 0, idx->stream, idx->X, idx->n, (int)idx->dim, mc.maxima);
        else
            hipLaunchKernelGGL(k_mc_stats<false>, grid, dim3(256), 0, idx->stream, idx->X, idx->n, (int)idx->dim, mc.maxima);
        SSW_HIP_TRY(hipGetLastError());
        SSW_HIP_TRY(hipMemcpyAsync(mx, mc.maxima, sizeof(mx), hipMemcpyDeviceToHost, idx->stream));
        SSW_HIP_TRY(hipStreamSynchronize(idx->stream));
    }
    p.rows_maxabs = mx[0], p.rows_maxnorm = mx[1];
    p.rows_stats_stale = false;
    return SSW_OK;
}

float pow2_scale(float maxabs) {  // scale * maxabs in [128, 256)
    int e2 = 0;
    (void)std::frexp(maxabs, &e2);  // maxabs in [2^(e2-1), 2^e2)
    return std::ldexp(1.0f, 8 - e2);
}

// the layout of a group's device state and of its result block
struct McLayout {
    size_t qh, qnorm, thr, cnt, kept, ovf, buf, grp_bytes;
    size_t appended, images, rows, scores, counts, flags, res_bytes;
    McLayout(int qp, int nq, int k, int dim) {
        size_t o = 0;
        auto take = [&](size_t bytes) {
            const size_t at = o;
            o += (bytes + 255) & ~(size_t)255;
            return at;
        };
        qh = take((size_t)qp * dim * 2), qnorm = take((size_t)qp * 4), thr = take((size_t)qp * 4);
        cnt = take((size_t)qp * 4), kept = take((size_t)qp * 4), ovf = take((size_t)qp * 4);
        buf = take((size_t)qp * MC_CAP * 8), grp_bytes = o;
        o = 0;
        appended = take(8), images = take((size_t)nq * k * 8), rows = take((size_t)nq * k * 8);
        scores = take((size_t)nq * k * 4), counts = take((size_t)nq * 4), flags = take((size_t)nq * 4), res_bytes = o;
    }
};

ssw_status mc_nomem(ssw_index *idx, const char *what) {
    (void)hipGetLastError();
    idx->mc.release();  // the next call starts over; the handle stays usable
    set_error("ssw_index_topk_batch_mc: no memory for %s", what);
    return SSW_ERR_NOMEM;
}

// the group workspace for qp padded queries of k results, the upload block of in_bytes and the strip order
ssw_status mc_workspace(ssw_index *idx, int qp, int k, size_t in_bytes, int64_t strips) {
    McState &mc = idx->mc;
    if (qp > mc.q_cap || k > mc.k_cap) {
        const int q_cap = std::max(qp, mc.q_cap), k_cap = std::max(k, mc.k_cap);
        const McLayout cap(q_cap, q_cap, k_cap, idx->dim);
        SSW_HIP_TRY(hipStreamSynchronize(idx->stream));
        (void)hipFree(mc.grp), (void)hipFree(mc.res_dev);
        if (mc.res_host) (void)hipHostFree(mc.res_host);
        mc.grp = mc.res_dev = mc.res_host = nullptr;
        mc.q_cap = mc.k_cap = 0;
        if (hipMalloc((void **)&mc.grp, cap.grp_bytes) != hipSuccess || hipMalloc((void **)&mc.res_dev, cap.res_bytes) != hipSuccess ||
            hipHostMalloc((void **)&mc.res_host, cap.res_bytes, hipHostMallocDefault) != hipSuccess)
            return mc_nomem(idx, "the group's buffers");
        mc.q_cap = q_cap, mc.k_cap = k_cap;
    }
    if (in_bytes > mc.in_cap) {
        SSW_HIP_TRY(hipStreamSynchronize(idx->stream));
        (void)hipFree(mc.in_dev);
        mc.in_dev = nullptr, mc.in_cap = 0;
        size_t cap = (size_t)1 << 16;
        while (cap < in_bytes) cap <<= 1;
        if (hipMalloc((void **)&mc.in_dev, cap) != hipSuccess) return mc_nomem(idx, "the query block");
        mc.in_cap = cap;
    }
    if (mc.perm_strips != strips) {  // Fisher-Yates over the strip ids, a fixed seed: the same order every call
        SSW_HIP_TRY(hipStreamSynchronize(idx->stream));
        (void)hipFree(mc.perm);
        mc.perm = nullptr, mc.perm_strips = 0;
        if (hipMalloc((void **)&mc.perm, (size_t)strips * 4) != hipSuccess) return mc_nomem(idx, "the strip order");
        std::vector<int32_t> perm((size_t)strips);
        for (int64_t i = 0; i < strips; ++i) perm[(size_t)i] = (int32_t)i;
        uint64_t st = 0x5EE5A3D1ull ^ (uint64_t)strips;
        for (int64_t i = strips - 1; i > 0; --i) std::swap(perm[(size_t)i], perm[(size_t)(splitmix64(st) % (uint64_t)(i + 1))]);
        SSW_HIP_TRY(hipMemcpy(mc.perm, perm.data(), (size_t)strips * 4, hipMemcpyHostToDevice));
        mc.perm_strips = strips;
    }
    return SSW_OK;
}

// level boundaries in strips: the first level holds MC_CAP rows, then a constant ratio <= MC_CAP / (2 M) up to all
std::vector<int64_t> level_bounds(int64_t strips, int R, int M) {
    std::vector<int64_t> bounds;
    const int64_t b0 = std::min<int64_t>(strips, MC_CAP / R);
    bounds.push_back(b0);
    if (strips > b0) {
        const double span = (double)strips / (double)b0;
        const int levels = std::max(1, (int)std::ceil(std::log(span) / std::log((double)MC_CAP / (2.0 * M)) - 1e-9));
        const double ratio = std::pow(span, 1.0 / levels);
        for (int l = 1; l < levels; ++l)
            bounds.push_back(std::min(strips, std::max(bounds.back(), (int64_t)std::llround((double)b0 * std::pow(ratio, l)))));
        bounds.push_back(strips);
    }
    return bounds;
}

template <int D, int R, bool H16>
ssw_status launch_candidates_t(const ssw_index *idx, float scale, const int32_t *strips, int64_t count, const f16 *Qh,
                               int q_tiles, const float *thr, unsigned *cnt, uint64_t *buf) {
    constexpr int lds = MC_RING + R * D * 2;
    SSW_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k_mc_candidates<D, R, H16>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    for (int64_t s0 = 0; s0 < count; s0 += MC_MAX_LAUNCH) {
        const unsigned g = (unsigned)std::min<int64_t>(MC_MAX_LAUNCH, count - s0);
        hipLaunchKernelGGL((k_mc_candidates<D, R, H16>), dim3(g), dim3(512), lds, idx->stream, (const void *)idx->X, idx->n,
                           scale, strips + s0, Qh, q_tiles, thr, cnt, buf);
    }
    return SSW_OK;
}

ssw_status launch_candidates(const ssw_index *idx, float scale, const int32_t *strips, int64_t count, const f16 *Qh,
                             int q_tiles, const float *thr, unsigned *cnt, uint64_t *buf) {
    const bool h = idx->dtype == SSW_DTYPE_F16;
#define MC_CASE(D, R)                                                                                       \
    case D:                                                                                                 \
        return h ? launch_candidates_t<D, R, true>(idx, scale, strips, count, Qh, q_tiles, thr, cnt, buf)   \
                 : launch_candidates_t<D, R, false>(idx, scale, strips, count, Qh, q_tiles, thr, cnt, buf);
    switch (idx->dim) {
        MC_CASE(256, 128)
        MC_CASE(512, 128)
        MC_CASE(768, 64)
        MC_CASE(1024, 64)
    }
#undef MC_CASE
    return SSW_ERR_UNSUPPORTED;
}

void launch_finish(const ssw_index *idx, int nq, const McFinishArgs &a) {
    const dim3 grid((unsigned)nq), block(256);
#define MC_CASE(C)                                                                                                  \
    case C * 256:                                                                                                   \
        if (idx->dtype == SSW_DTYPE_F16)                                                                            \
            hipLaunchKernelGGL((k_mc_finish<rows::H16Rows, C>), grid, block, 0, idx->stream,                        \
                               reinterpret_cast<const uint16_t *>(idx->X), a);                                      \
        else                                                                                                        \
            hipLaunchKernelGGL((k_mc_finish<rows::F32Rows, C>), grid, block, 0, idx->stream,                        \
                               reinterpret_cast<const float *>(idx->X), a);                                         \
        break;
    switch (idx->dim) {
        MC_CASE(1)
        MC_CASE(2)
        MC_CASE(3)
        MC_CASE(4)
    }
#undef MC_CASE
}

// What the lab build's hook (ssw_debug_mc_candidates, at the foot of this file) reads out of a group's device state; the
// product passes none.  Every pointer is host memory and may be NULL.  mode 1: the state behind the first level's
// candidate launch, before any compaction (`stride` = MC_CAP entries a query), and run_group returns there; mode 0: the
// state the finish saw (`stride` = M entries a query).
struct McProbe {
    int mode = 0;
    float *meta = nullptr;       // [6] scale, scale_q, maxabs_x, maxnorm, maxabs_q, M
    int64_t *levels = nullptr;   // [levels_cap] the level bounds in strips
    int32_t levels_cap = 0, *n_levels = nullptr, *perm = nullptr;  // perm [strips]
    float *thr = nullptr;        // [nq]
    uint32_t *cnt = nullptr;     // [nq] as the device holds it: above MC_CAP after an overflowing launch (mode 1)
    float *scores = nullptr;     // [nq, stride] fp16-path scores of the first min(cnt, stride) entries
    int64_t *rows = nullptr;     // [nq, stride] their rows
    int32_t *flags = nullptr;    // [nq] mode 0
    float *bE = nullptr;         // [nq, 2] mode 0: b and E as k_mc_finish evaluated them
    float *bE_dev = nullptr;     // the device words behind bE (the hook's)
};

// a group's thresholds, counts and buffer entries, unpacked for the probe (after the stream has been waited for)
ssw_status probe_read(const McProbe &pr, int nq, int stride, const float *thr, const unsigned *cnt, const uint64_t *buf) {
    if (pr.thr) SSW_HIP_TRY(hipMemcpy(pr.thr, thr, (size_t)nq * 4, hipMemcpyDeviceToHost));
    std::vector<uint32_t> c((size_t)nq);
    SSW_HIP_TRY(hipMemcpy(c.data(), cnt, (size_t)nq * 4, hipMemcpyDeviceToHost));
    if (pr.cnt) std::copy(c.begin(), c.end(), pr.cnt);
    if (!pr.scores && !pr.rows) return SSW_OK;
    std::vector<uint64_t> keys((size_t)nq * stride);
    SSW_HIP_TRY(hipMemcpy2D(keys.data(), (size_t)stride * 8, buf, (size_t)MC_CAP * 8, (size_t)stride * 8, (size_t)nq,
                            hipMemcpyDeviceToHost));
    for (int q = 0; q < nq; ++q)
        for (uint32_t e = 0; e < std::min<uint32_t>(c[(size_t)q], (uint32_t)stride); ++e) {
            const uint64_t key = keys[(size_t)q * stride + e];
            if (pr.scores) pr.scores[(size_t)q * stride + e] = ord_to_f32((uint32_t)(key >> 32));
            if (pr.rows) pr.rows[(size_t)q * stride + e] = (int64_t)(0xFFFFFFFFu - (uint32_t)key);
        }
    return SSW_OK;
}

// one group of nq <= MC_GROUP queries [q0, q0 + nq) of the call: everything up to its results in the caller's arrays;
// failed: the call's queries that the plain batch has to answer
ssw_status run_group(ssw_index *idx, const float *q_host, int32_t q0, int32_t nq, const int64_t *ex_images,
                     const int64_t *ex_offsets, int32_t k, int M, float scale, int64_t *out_images, float *out_scores,
                     int64_t *out_best_rows, int32_t *out_counts, std::vector<int32_t> &failed,
                     const McProbe *probe = nullptr) {
    McState &mc = idx->mc;
    const int D = idx->dim, R = strip_rows(D);
    const float *Q = q_host + (size_t)q0 * D;
    float maxabs_q = 0.f;
    for (size_t i = 0; i < (size_t)nq * D; ++i) maxabs_q = std::max(maxabs_q, std::fabs(Q[i]));
    if (!(maxabs_q >= MC_MIN_ABS && maxabs_q <= MC_MAX_ABS)) {  // no bound at this magnitude (zero queries too)
        for (int32_t b = 0; b < nq; ++b) failed.push_back(q0 + b);
        mc.stats[3] += nq;
        return SSW_OK;
    }
    const float scale_q = pow2_scale(maxabs_q);
    // the upload: [queries | exclusion offsets from 0 | each query's ids ascending]
    const size_t q_bytes = (size_t)nq * D * sizeof(float);
    const int64_t ex_total = ex_offsets ? ex_offsets[q0 + nq] - ex_offsets[q0] : 0;
    const size_t in_bytes = q_bytes + ((size_t)nq + 1 + (size_t)ex_total) * 8;
    std::vector<unsigned char> in(in_bytes);
    memcpy(in.data(), Q, q_bytes);
    int64_t *off = reinterpret_cast<int64_t *>(in.data() + q_bytes), *ids = off + nq + 1;
    for (int32_t b = 0; b <= nq; ++b) off[b] = ex_offsets ? ex_offsets[q0 + b] - ex_offsets[q0] : 0;
    for (int32_t b = 0; b < nq && ex_total > 0; ++b) {
        std::copy(ex_images + ex_offsets[q0 + b], ex_images + ex_offsets[q0 + b + 1], ids + off[b]);
        std::sort(ids + off[b], ids + off[b + 1]);
    }
    const int qp = (nq + MC_QT - 1) / MC_QT * MC_QT;
    const int64_t strips = (idx->n + R - 1) / R;
    SSW_TRY(mc_workspace(idx, qp, k, in_bytes, strips));
    SSW_TRY(mc.in_stage.push(mc.in_dev, in.data(), in_bytes, idx->stream));
    const McLayout L(qp, nq, k, D);
    hipStream_t s = idx->stream;
    f16 *Qh = reinterpret_cast<f16 *>(mc.grp + L.qh);
    float *qnorm = reinterpret_cast<float *>(mc.grp + L.qnorm), *thr = reinterpret_cast<float *>(mc.grp + L.thr);
    unsigned *cnt = reinterpret_cast<unsigned *>(mc.grp + L.cnt), *kept = reinterpret_cast<unsigned *>(mc.grp + L.kept);
    unsigned *ovf = reinterpret_cast<unsigned *>(mc.grp + L.ovf);
    uint64_t *buf = reinterpret_cast<uint64_t *>(mc.grp + L.buf);
    unsigned long long *appended = reinterpret_cast<unsigned long long *>(mc.res_dev + L.appended);
    const float *Qf = reinterpret_cast<const float *>(mc.in_dev);
    hipLaunchKernelGGL(k_mc_prep, dim3(qp / 4), dim3(256), 0, s, Qf, (int)nq, qp, D, scale_q, Qh, qnorm, thr, cnt, kept, ovf,
                       appended);
    const std::vector<int64_t> bounds = level_bounds(strips, R, M);
    if (probe) {
        const float meta[6] = {scale, scale_q, idx->prune.rows_maxabs, idx->prune.rows_maxnorm, maxabs_q, (float)M};
        if (probe->meta) std::copy(meta, meta + 6, probe->meta);
        if (probe->n_levels) *probe->n_levels = (int32_t)bounds.size();
        for (size_t l = 0; probe->levels && l < bounds.size() && l < (size_t)probe->levels_cap; ++l) probe->levels[l] = bounds[l];
        if (probe->perm) SSW_HIP_TRY(hipMemcpy(probe->perm, mc.perm, (size_t)strips * 4, hipMemcpyDeviceToHost));
    }
    int64_t s0 = 0;
    for (const int64_t s1 : bounds) {
        if (s1 <= s0) continue;
        SSW_TRY(launch_candidates(idx, scale, mc.perm + s0, s1 - s0, Qh, qp / MC_QT, thr, cnt, buf));
        if (probe && probe->mode == 1) {  // the candidate kernel's raw output
            SSW_HIP_TRY(hipGetLastError());
            SSW_HIP_TRY(hipStreamSynchronize(s));
            return probe_read(*probe, nq, MC_CAP, thr, cnt, buf);
        }
        hipLaunchKernelGGL(k_mc_compact, dim3(nq), dim3(256), 0, s, buf, cnt, kept, thr, ovf, appended, M);
        s0 = s1;
    }
    McFinishArgs a;
    a.Qf = Qf, a.qnorm = qnorm, a.thr = thr, a.cnt = cnt, a.ovf = ovf, a.buf = buf;
    a.row_start = idx->has_map ? idx->row_start : nullptr;
    a.n_images = idx->n_images;
    a.ex_off = reinterpret_cast<const int64_t *>(mc.in_dev + q_bytes), a.ex_ids = a.ex_off + nq + 1;
    a.M = M, a.k = k;
    a.inv_scale = 1.0f / scale, a.inv_scale_q = 1.0f / scale_q;
    a.eps_rel = idx->dtype == SSW_DTYPE_F16 ? 6.5e-4f : 1.2e-3f;
    a.maxnorm = idx->prune.rows_maxnorm, a.maxabs_x = idx->prune.rows_maxabs, a.maxabs_q = maxabs_q;
    a.out_images = reinterpret_cast<int64_t *>(mc.res_dev + L.images), a.out_rows = reinterpret_cast<int64_t *>(mc.res_dev + L.rows);
    a.out_scores = reinterpret_cast<float *>(mc.res_dev + L.scores);
    a.out_counts = reinterpret_cast<int32_t *>(mc.res_dev + L.counts), a.out_flags = reinterpret_cast<int32_t *>(mc.res_dev + L.flags);
    a.out_bE = probe ? probe->bE_dev : nullptr;
    launch_finish(idx, nq, a);
    SSW_HIP_TRY(hipGetLastError());
    SSW_HIP_TRY(hipMemcpyAsync(mc.res_host, mc.res_dev, L.res_bytes, hipMemcpyDeviceToHost, s));
    SSW_HIP_TRY(hipStreamSynchronize(s));  // the group's one wait
    if (probe) {
        SSW_TRY(probe_read(*probe, nq, M, thr, cnt, buf));
        if (probe->flags) memcpy(probe->flags, mc.res_host + L.flags, (size_t)nq * 4);
        if (probe->bE && probe->bE_dev) SSW_HIP_TRY(hipMemcpy(probe->bE, probe->bE_dev, (size_t)nq * 8, hipMemcpyDeviceToHost));
    }
    mc.stats[6] += strips;
    mc.stats[7] += (int64_t) * reinterpret_cast<const unsigned long long *>(mc.res_host + L.appended);
    const int64_t *r_img = reinterpret_cast<const int64_t *>(mc.res_host + L.images);
    const int64_t *r_row = reinterpret_cast<const int64_t *>(mc.res_host + L.rows);
    const float *r_sc = reinterpret_cast<const float *>(mc.res_host + L.scores);
    const int32_t *r_cnt = reinterpret_cast<const int32_t *>(mc.res_host + L.counts);
    const int32_t *r_flag = reinterpret_cast<const int32_t *>(mc.res_host + L.flags);
    for (int32_t b = 0; b < nq; ++b) {
        if (r_flag[b] != 0) {
            ++mc.stats[r_flag[b] == 2 ? 4 : 3];
            failed.push_back(q0 + b);
            continue;
        }
        ++mc.stats[2];
        const size_t o = (size_t)(q0 + b) * k, g = (size_t)b * k, m = (size_t)r_cnt[b];
        out_counts[q0 + b] = r_cnt[b];
        if (out_images) memcpy(out_images + o, r_img + g, m * 8);
        if (out_best_rows) memcpy(out_best_rows + o, r_row + g, m * 8);
        if (out_scores) memcpy(out_scores + o, r_sc + g, m * 4);
    }
    return SSW_OK;
}

// the state a pruned call leaves: the last query kept, the score buffer for the first reader to complete
ssw_status leave_last_query(ssw_index *idx, const float *q_host, int32_t nq) {
    const size_t D = (size_t)idx->dim;
    PruneState &p = idx->prune;
    if (!p.q_last) SSW_HIP_TRY(hipMalloc((void **)&p.q_last, D * sizeof(float)));
    SSW_TRY(idx->q_stage.push(p.q_last, q_host + (size_t)(nq - 1) * D, D * sizeof(float), idx->stream));
    idx->scores_partial = true;
    return SSW_OK;
}

}  // namespace

extern "C" ssw_status ssw_index_topk_batch_mc(ssw_index *idx, const float *q_host, int32_t nq, const int64_t *excluded_images,
                                              const int64_t *excluded_offsets, int32_t k, int64_t *out_images,
                                              float *out_scores, int64_t *out_best_rows, int32_t *out_counts) {
    const char *who = "ssw_index_topk_batch_mc";
    SSW_TRY(refuse_view(idx, who));
    SSW_TRY(refuse_dims128(idx, who));  // the strips and the finish read whole 256-element chunks
    SSW_REQUIRE(idx != nullptr && q_host != nullptr && out_counts != nullptr, "NULL argument");
    if (idx->dim != 256 && idx->dim != 512 && idx->dim != 768 && idx->dim != 1024) {
        set_error("%s: dim=%d unsupported", who, idx->dim);
        return SSW_ERR_UNSUPPORTED;
    }
    if (nq < 1 || nq > 65535) {
        set_error("%s: nq=%d outside [1, 65535]", who, nq);
        return SSW_ERR_UNSUPPORTED;
    }
    SSW_REQUIRE(k >= 1 && k <= SSW_MAX_TOPK, "k=%d outside [1, %d]", k, SSW_MAX_TOPK);
    SSW_TRY(check_excluded_lists(idx, excluded_images, excluded_offsets, nq));
    SSW_TRY(check_query_batch(idx, q_host, nq));
    McState &mc = idx->mc;
    DeviceGuard guard(idx->device);
    if (k <= MC_MAX_K) SSW_TRY(rows_stats(idx));
    const float maxabs = idx->prune.rows_maxabs;
    if (k <= MC_MAX_K && (!(maxabs > 0.f) || !std::isfinite(maxabs))) {
        set_error("%s: the index holds no finite non-zero vector, or a NaN", who);
        return SSW_ERR_NUMERIC;
    }
    ++mc.stats[0];
    mc.stats[1] += nq;
    if (k > MC_MAX_K || maxabs < MC_MIN_ABS || maxabs > MC_MAX_ABS) {  // no list of 4 k candidates / no bound: the plain batch
        if (k > MC_MAX_K) ++mc.stats[5];
        else mc.stats[3] += nq;
        return ssw_index_topk_batch(idx, q_host, nq, excluded_images, excluded_offsets, k, out_images, out_scores,
                                    out_best_rows, out_counts);
    }
    int M = 64;
    while (M < 4 * k) M <<= 1;
    const float scale = pow2_scale(maxabs);
    std::vector<int32_t> failed;
    for (int32_t b = 0; b < nq; ++b) out_counts[b] = 0;
    for (int32_t q0 = 0; q0 < nq; q0 += MC_GROUP)
        SSW_TRY(run_group(idx, q_host, q0, std::min<int32_t>(MC_GROUP, nq - q0), excluded_images, excluded_offsets, k, M, scale,
                          out_images, out_scores, out_best_rows, out_counts, failed));
    const size_t D = (size_t)idx->dim;
    if (!failed.empty()) {  // ONE plain batch for all of them, each with its own exclusions
        const size_t nf = failed.size();
        std::vector<float> Qf(nf * D), sc(nf * k);
        std::vector<int64_t> off(nf + 1, 0), ids, im(nf * k), rw(nf * k);
        std::vector<int32_t> cn(nf, 0);
        for (size_t f = 0; f < nf; ++f) {
            const int32_t b = failed[f];
            memcpy(&Qf[f * D], q_host + (size_t)b * D, D * sizeof(float));
            if (excluded_offsets) ids.insert(ids.end(), excluded_images + excluded_offsets[b], excluded_images + excluded_offsets[b + 1]);
            off[f + 1] = (int64_t)ids.size();
        }
        SSW_TRY(ssw_index_topk_batch(idx, Qf.data(), (int32_t)nf, ids.empty() ? nullptr : ids.data(), off.data(), k, im.data(),
                                     sc.data(), rw.data(), cn.data()));
        for (size_t f = 0; f < nf; ++f) {
            const size_t o = (size_t)failed[f] * k, m = (size_t)cn[f];
            out_counts[failed[f]] = cn[f];
            if (out_images) memcpy(out_images + o, &im[f * k], m * 8);
            if (out_best_rows) memcpy(out_best_rows + o, &rw[f * k], m * 8);
            if (out_scores) memcpy(out_scores + o, &sc[f * k], m * 4);
        }
    }
    return leave_last_query(idx, q_host, nq);
}

extern "C" ssw_status ssw_index_topk_batch_mc_stats(ssw_index *idx, int64_t *out8) {
    SSW_REQUIRE(idx != nullptr && out8 != nullptr, "NULL argument");
    for (int i = 0; i < 8; ++i) out8[i] = idx->mc.stats[i];
    return SSW_OK;
}

#ifdef SSW_DEBUG_HOOKS
// include/seesaw_hip_debug.h: one group through run_group with a probe
extern "C" ssw_status ssw_debug_mc_candidates(ssw_index *idx, const float *q_host, int32_t nq, int32_t k, int32_t mode,
                                              float *out_meta, int64_t *out_levels, int32_t levels_cap, int32_t *out_n_levels,
                                              int32_t *out_perm, float *out_thr, uint32_t *out_cnt, float *out_scores,
                                              int64_t *out_rows, int32_t *out_flags, float *out_bE) {
    const char *who = "ssw_debug_mc_candidates";
    SSW_TRY(refuse_view(idx, who));
    SSW_TRY(refuse_dims128(idx, who));
    SSW_REQUIRE(idx != nullptr && q_host != nullptr, "NULL argument");
    if (idx->dim != 256 && idx->dim != 512 && idx->dim != 768 && idx->dim != 1024) {
        set_error("%s: dim=%d unsupported", who, idx->dim);
        return SSW_ERR_UNSUPPORTED;
    }
    if (nq < 1 || nq > MC_GROUP || k < 1 || k > MC_MAX_K || (mode != 0 && mode != 1)) {
        set_error("%s: nq=%d outside [1, %d], k=%d outside [1, %d] or mode=%d not 0 or 1", who, nq, MC_GROUP, k, MC_MAX_K, mode);
        return SSW_ERR_UNSUPPORTED;
    }
    SSW_TRY(check_query_batch(idx, q_host, nq));
    McState &mc = idx->mc;
    DeviceGuard guard(idx->device);
    SSW_TRY(rows_stats(idx));
    const float maxabs = idx->prune.rows_maxabs;
    float maxabs_q = 0.f;
    for (size_t i = 0; i < (size_t)nq * idx->dim; ++i) maxabs_q = std::max(maxabs_q, std::fabs(q_host[i]));
    if (!(maxabs >= MC_MIN_ABS && maxabs <= MC_MAX_ABS && maxabs_q >= MC_MIN_ABS && maxabs_q <= MC_MAX_ABS)) {
        set_error("%s: no bound at this magnitude of the rows or the queries (the product takes the plain batch)", who);
        return SSW_ERR_UNSUPPORTED;
    }
    int M = 64;
    while (M < 4 * k) M <<= 1;
    McProbe pr;
    pr.mode = mode, pr.meta = out_meta, pr.levels = out_levels, pr.levels_cap = levels_cap, pr.n_levels = out_n_levels;
    pr.perm = out_perm, pr.thr = out_thr, pr.cnt = out_cnt, pr.scores = out_scores, pr.rows = out_rows;
    pr.flags = out_flags, pr.bE = out_bE;
    if (mode == 0) SSW_HIP_TRY(hipMalloc((void **)&pr.bE_dev, (size_t)nq * 8));
    int64_t stats[8];
    std::copy(mc.stats, mc.stats + 8, stats);  // the counters are the product calls' alone
    std::vector<int32_t> failed, counts((size_t)nq, 0);
    ssw_status st = run_group(idx, q_host, 0, nq, nullptr, nullptr, k, M, pow2_scale(maxabs), nullptr, nullptr, nullptr,
                              counts.data(), failed, &pr);
    std::copy(stats, stats + 8, mc.stats);
    (void)hipFree(pr.bE_dev);
    if (st != SSW_OK) return st;
    return leave_last_query(idx, q_host, nq);
}
#endif

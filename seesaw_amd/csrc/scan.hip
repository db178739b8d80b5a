// scan.hip -- brute-force cosine scan: scores[i] = <X[i,:], q>  (gfx950 / MI355X)
//
// Replaces `scores = vectors @ vector.reshape(-1)` of the reference
// (seesaw/indices/multiscale/multiscale_index.py:171, :285, :345;
//  seesaw/indices/coarse/coarse_index.py:38, :73).
//
// Roofline: HBM-bound.  Algorithmic traffic = dim*4 bytes per row read once
// (2048 B at dim=512) + 4 B per row of score written.  No reuse -> no LDS staging:
// rows go straight from HBM to VGPRs with 16-byte loads, a wave reading one whole
// row (2 KiB at dim=512) with `dim/256` fully coalesced 1-KiB wave-instructions.
//
// Work decomposition (64-wide wavefronts):
//   * one wave owns a BATCH of 64 consecutive rows (128 KiB contiguous at dim=512) and
//     walks it in GROUPS of U rows (U = 2 at dim=512); the loads of group g+1 are
//     issued before group g is reduced (register double buffer).  Loads are non-temporal
//     (`global_load_dwordx4 ... nt`): the index is read once per query and must not churn
//     L2 / Infinity Cache.  One 4-wave workgroup per CU turned out to be the fastest
//     residency (see the schedule note below).
//   * lane l accumulates, for one row, two fmaf chains over the elements it loaded
//     (float4 v[c] = X[row, 256*c + 4*l .. +3], c < dim/256):
//         a0 = fma(v[c].x, q.x, a0); a1 = fma(v[c].y, q.y, a1);
//         a0 = fma(v[c].z, q.z, a0); a1 = fma(v[c].w, q.w, a1);     (c ascending)
//     both starting from +0.0f; the lane partial is p = a0 + a1.  (The two chains
//     are what v_pk_fma_f32 computes on a register pair.)
//   * the 64 lane partials of a row are summed by the xor-butterfly
//         v <- v + v[lane ^ off],   off = 1, 2, 4, 8, 16, 32
//     (f32 add is commutative, so every lane ends with the same bits).  For the
//     first log2(U) offsets the U rows of a group are reduced TOGETHER by a
//     transpose-reduce (each exchange halves the number of live registers and leaves
//     lane l with row l % U), which is value-identical to the butterfly; the
//     remaining offsets are plain butterfly steps.  U + 5 - log2(U) exchanges per U
//     rows instead of 6 per row.
//   * lane l = U*g + j then owns the finished score of row j of group g; after the
//     64/U groups of a batch lane l holds the score of row l and the wave stores its
//     64 scores with one coalesced 256-B write.
//   oracle/ssw_oracle.c::ssw_oracle_scores_kernel_order restates exactly this order,
//   which makes the scores BIT-EXACT against the CPU oracle, not merely close.
//
// The f16 index (SSW_DTYPE_F16) runs the same kernels with another row format (H16Rows below): binary16 rows in the
// lane-interleaved layout of ssw_common.h (h16_group_pos), where lane l's 4*C elements are 8*C contiguous bytes -- one
// 16-byte load per lane per row at dim 512.  A fragment stays packed while it is in flight and is widened exactly
// (v_cvt_f32_f16; the code object keeps f16 denormals) into the float4s the f32 kernel would have loaded for the
// widened row right before dot_frag, so the scores are the BITS of the f32 scan over X.astype(float16).astype(float32).
// A row is dim*2 bytes, so a group takes twice the rows of the f32 schedule: the same bytes in flight per wave.
//
// Grid: persistent, (#CUs x resident blocks per CU) blocks of 256 threads; waves
// stride over the batches.
#include <cstdlib>

#include "ssw_common.h"

namespace ssw {

namespace {

template <int C>
struct RowFrag {
    float4 v[C];
};

// ---- row formats: how a lane's part of a row is stored and loaded, and how it becomes the RowFrag dot_frag reads.
// NT: non-temporal loads (`global_load_dwordx4 ... nt`): the index is streamed once per query
// and is far larger than L2 / Infinity Cache, so it should not displace anything.

// f32 rows in natural order: chunk c of lane l is the float4 at element 256*c + 4*l, used as loaded
struct F32Rows {
    typedef float T;
    template <int C>
    using Frag = RowFrag<C>;

    template <int C, bool NT>
    static __device__ __forceinline__ RowFrag<C> load(const float *__restrict__ X, int row, int lane) {
        RowFrag<C> r;
        const float4 *p = reinterpret_cast<const float4 *>(X) + (int64_t)row * (C * 64) + lane;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            if (NT) {
                const f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(p + c * 64));
                r.v[c] = make_float4(v.x, v.y, v.z, v.w);
            } else {
                r.v[c] = p[c * 64];
            }
        }
        return r;
    }
    template <int C>
    static __device__ __forceinline__ const RowFrag<C> &widen(const RowFrag<C> &f) { return f; }
    // the 4 elements from natural element e of a row
    static __device__ __forceinline__ float4 group4(const float *row, int e, int dim) {
        return reinterpret_cast<const float4 *>(row)[e >> 2];
    }
};

// binary16 rows in the f16 index's lane-interleaved layout: lane l's 4*C elements are its 8*C contiguous bytes
template <int C>
struct HalfFrag {
    u32x2 w[C];  // chunk c = elements 256*c + 4*l .. +3
};

struct H16Rows {
    typedef uint16_t T;
    template <int C>
    using Frag = HalfFrag<C>;

    template <int C, bool NT>
    static __device__ __forceinline__ HalfFrag<C> load(const uint16_t *__restrict__ X, int row, int lane) {
        HalfFrag<C> r;
        const unsigned char *p = reinterpret_cast<const unsigned char *>(X) + (int64_t)row * (C * 512) + lane * (C * 8);
        if constexpr (C % 2 == 0) {  // 16-byte aligned: one dwordx4 per two chunks (dim 512: one per lane per row)
            const u32x4 *p4 = reinterpret_cast<const u32x4 *>(p);
#pragma unroll
            for (int i = 0; i < C / 2; ++i) {
                u32x4 v;
                if constexpr (NT) v = __builtin_nontemporal_load(p4 + i);
                else v = p4[i];
                r.w[2 * i] = u32x2{v.x, v.y};
                r.w[2 * i + 1] = u32x2{v.z, v.w};
            }
        } else {
            const u32x2 *p2 = reinterpret_cast<const u32x2 *>(p);
#pragma unroll
            for (int c = 0; c < C; ++c) {
                if constexpr (NT) r.w[c] = __builtin_nontemporal_load(p2 + c);
                else r.w[c] = p2[c];
            }
        }
        return r;
    }
    template <int C>
    static __device__ __forceinline__ RowFrag<C> widen(const HalfFrag<C> &f) {
        RowFrag<C> r;
#pragma unroll
        for (int c = 0; c < C; ++c) r.v[c] = widen_h16x4(f.w[c]);
        return r;
    }
    static __device__ __forceinline__ float4 group4(const uint16_t *row, int e, int dim) {
        return widen_h16x4(*reinterpret_cast<const u32x2 *>(row + h16_group_pos(e, dim >> 8)));
    }
};

typedef float f32x2 __attribute__((ext_vector_type(2)));

// the two fmaf chains (a0 over .x/.z, a1 over .y/.w) as packed math on register pairs
template <int C>
__device__ __forceinline__ float dot_frag(const RowFrag<C> &x, const RowFrag<C> &q) {
    f32x2 a = {0.0f, 0.0f};
#pragma unroll
    for (int c = 0; c < C; ++c) {
        a = __builtin_elementwise_fma(f32x2{x.v[c].x, x.v[c].y}, f32x2{q.v[c].x, q.v[c].y}, a);
        a = __builtin_elementwise_fma(f32x2{x.v[c].z, x.v[c].w}, f32x2{q.v[c].z, q.v[c].w}, a);
    }
    return a.x + a.y;
}

// all-ones where the lane has bit `off` set, as a plain lane value the optimiser cannot turn back into a lane mask
__device__ __forceinline__ unsigned lane_bit_mask(int lane, int off) {
    unsigned m = (lane & off) ? 0xffffffffu : 0u;
    asm volatile("" : "+v"(m));
    return m;
}
// m all-ones: b, m zero: a (one v_bfi_b32)
__device__ __forceinline__ float pick(unsigned m, float a, float b) {
    return __uint_as_float((__float_as_uint(b) & m) | (__float_as_uint(a) & ~m));
}

// U lane-partial registers (acc[j] = row j of the group) -> every lane l holds the
// complete sum of row (l % U): transpose-reduce over offsets 1..U/2, then butterfly
// over offsets U..32.  Canonical offset order 1,2,4,8,16,32 for every U.
// BITSEL: the keep / send choice as bit selects on a per-lane mask instead of selects on a lane mask in SGPRs.  Same
// values.  The multi-query kernel's 8- and 16-register sets need it: the optimiser merged their select trees into chains
// over 2^k combined lane masks, which no longer fit the SGPRs and were spilled into VGPR lanes (v_readlane + s_nop per
// select: 80 a group at 8 registers).
template <int U, bool BITSEL = false>
__device__ __forceinline__ float group_reduce(float (&acc)[U], int lane) {
#pragma unroll
    for (int off = 1; off < U; off <<= 1) {
        // register distance of the pair merged at this offset == off
        const bool upper = (lane & off) != 0;
        const unsigned m = BITSEL ? lane_bit_mask(lane, off) : 0u;
#pragma unroll
        for (int i = 0; i < U; i += 2 * off) {
            const float keep = BITSEL ? pick(m, acc[i], acc[i + off]) : (upper ? acc[i + off] : acc[i]);
            const float send = BITSEL ? pick(m, acc[i + off], acc[i]) : (upper ? acc[i] : acc[i + off]);
            acc[i] = keep + __shfl_xor(send, off, 64);
        }
    }
    float v = acc[0];
#pragma unroll
    for (int off = U; off < 64; off <<= 1) v = v + __shfl_xor(v, off, 64);
    return v;
}

template <class R, int C, int U>
struct Group {
    typename R::template Frag<C> r[U];
};

template <class R, int C, int U, bool NT>
__device__ __forceinline__ void load_group(Group<R, C, U> &g, const typename R::T *__restrict__ X,
                                           int first_row, int last, int lane) {
#pragma unroll
    for (int u = 0; u < U; ++u) g.r[u] = R::template load<C, NT>(X, min(first_row + u, last), lane);
}

template <class R, int C, int U, bool NT>
__global__ __launch_bounds__(256) void scan_scores_kernel(const typename R::T *__restrict__ X,
                                                         const float *__restrict__ q,
                                                         float *__restrict__ scores, int n) {
    constexpr int GPB = 64 / U;  // groups per batch
    const int lane = threadIdx.x & 63;
    // wave index through readfirstlane: keeps every row/address computation on the SALU
    // (rows are 32-bit: n < 2^31 - 2^16 is checked by the launcher)
    const int gwave = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int nwaves = gridDim.x * 4;
    const int nbatches = (n + 63) >> 6;
    const int last = n - 1;
    if (gwave >= nbatches) return;

    RowFrag<C> qf;
#pragma unroll
    for (int c = 0; c < C; ++c) qf.v[c] = reinterpret_cast<const float4 *>(q)[c * 64 + lane];

    const int my_group = lane / U;
    Group<R, C, U> cur, nxt;
    load_group<R, C, U, NT>(cur, X, gwave << 6, last, lane);
    for (int b = gwave; b < nbatches; b += nwaves) {
        const int row0 = b << 6;
        const int nb = b + nwaves;
        const int next0 = (nb < nbatches ? nb : b) << 6;  // no next batch: re-touch own rows
        float out = 0.0f;
#pragma unroll 2
        for (int g = 0; g < GPB; ++g) {
            // request group g+1 (or the first group of this wave's next batch) ...
            const int nrow = (g + 1 < GPB) ? row0 + (g + 1) * U : next0;
            load_group<R, C, U, NT>(nxt, X, nrow, last, lane);
            // ... then finish group g
            float acc[U];
#pragma unroll
            for (int u = 0; u < U; ++u) acc[u] = dot_frag<C>(R::widen(cur.r[u]), qf);
            const float v = group_reduce<U>(acc, lane);
            out = (my_group == g) ? v : out;
            cur = nxt;
        }
        if (row0 + lane < n) scores[row0 + lane] = out;
    }
}

// Multi-query form of the streaming kernel: the rows are walked exactly as above (persistent grid, 64-row batches,
// groups of U rows, non-temporal 16-byte loads, register double buffer), but a lane holds the fragments of B queries
// and forms B lane partials per row, so one pass over the rows in HBM scores B queries.  Per query the two fma chains
// of dot_frag and the offset order 1, 2, 4, 8, 16, 32 of the lane sum are the single-query kernel's: slab b receives
// the BITS scan_scores_kernel writes for query b.
//   * the V = U*B (row, query) partials of a group are ONE register set for group_reduce (item u + U*b): V - 1
//     exchanges of the transpose-reduce and log2(64 / V) butterfly steps leave lane l with the finished score of row
//     l % U for query (l / U) % B -- 10 exchanges per two rows at U = 2, B = 4 where four butterflies take 24.
//   * every value exists 64 / V times; lane l keeps, into register t, the value of group s*B + t for s = l / V.  After
//     the 64 / U groups of a batch lane l = s*V + b*U + u holds rows s*V + t*U + u (t < B) of query b: a B x B
//     transpose between register index and lane bits (B/2 * log2(B) exchanges per 64 rows) gives lane l row l of
//     every query, and the wave stores one coalesced 256-byte line per slab.
// (The name carries no "scan": tests/test_index_f16_cpu.py pins the kernels so named to the three single-query ones;
//  tests/test_topk_batch_cpu.py asserts for this kernel what that test asserts for them.)
template <int B>
struct ScoreSlabs {
    float *p[B];
};

template <class R, int C, int U, int B, bool NT>
__global__ __launch_bounds__(256) void batch_scores_kernel(const typename R::T *__restrict__ X,
                                                               const float *__restrict__ q,  // [B, 256*C]
                                                               ScoreSlabs<B> out, int n) {
    constexpr int V = U * B;
    static_assert(V <= 64 && (B & (B - 1)) == 0 && (U & (U - 1)) == 0, "U*B (row, query) partials share one wave-wide reduce");
    constexpr int GPB = 64 / U;  // groups per batch
    constexpr int T = B <= 4 ? B : 4;  // groups unrolled per trip
    const int lane = threadIdx.x & 63;
    const int gwave = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int nwaves = gridDim.x * 4;
    const int nbatches = (n + 63) >> 6;
    const int last = n - 1;
    if (gwave >= nbatches) return;

    RowFrag<C> qf[B];
#pragma unroll
    for (int b = 0; b < B; ++b) {
#pragma unroll
        for (int c = 0; c < C; ++c) qf[b].v[c] = reinterpret_cast<const float4 *>(q)[(b * C + c) * 64 + lane];
    }

    const int my_run = lane / V;
    Group<R, C, U> cur, nxt;
    load_group<R, C, U, NT>(cur, X, gwave << 6, last, lane);
    for (int bt = gwave; bt < nbatches; bt += nwaves) {
        const int row0 = bt << 6;
        const int nb = bt + nwaves;
        const int next0 = (nb < nbatches ? nb : bt) << 6;  // no next batch: re-touch own rows
        float o[B];
#pragma unroll
        for (int t = 0; t < B; ++t) o[t] = 0.0f;
        // T groups are unrolled inside a rolled loop, so that a group's value goes to a register chosen at compile time
        // (T = B up to 4; a runtime slot costs B selects and B live lane masks a group, which at 16 partials spilled
        // SGPRs into VGPR lanes).  All B groups unrolled is 64 KiB of code at B = 8, more than the instruction cache.
        // The scheduling barriers keep a group's arithmetic behind the request for the next group and ahead of the one
        // after: without them the two groups' fma chains were interleaved and every trip waited for vmcnt(0).
#pragma unroll 1
        for (int s = 0; s < GPB / T; ++s) {
#pragma unroll
            for (int t = 0; t < T; ++t) {
                const int g = s * T + t;
                const int nrow = (g + 1 < GPB) ? row0 + (g + 1) * U : next0;
                load_group<R, C, U, NT>(nxt, X, nrow, last, lane);
                __builtin_amdgcn_sched_barrier(0);
                float acc[V];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const RowFrag<C> x = R::widen(cur.r[u]);
#pragma unroll
                    for (int b = 0; b < B; ++b) acc[b * U + u] = dot_frag<C>(x, qf[b]);
                }
                const float v = group_reduce<V, true>(acc, lane);
                const bool mine = my_run == s / (B / T);
#pragma unroll
                for (int j = 0; j < B / T; ++j) {
                    const bool here = (B == T) || (s % (B / T)) == j;  // wave-uniform
                    unsigned m = (mine && here) ? 0xffffffffu : 0u;
                    asm volatile("" : "+v"(m));
                    o[t + T * j] = pick(m, o[t + T * j], v);
                }
                cur = nxt;
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        // register t <-> query bits of the lane
#pragma unroll
        for (int off = 1; off < B; off <<= 1) {
            const unsigned m = lane_bit_mask(lane, U * off);  // (my_q & off) != 0
#pragma unroll
            for (int i = 0; i < B; ++i) {
                if ((i & off) != 0) continue;
                const float got = __shfl_xor(pick(m, o[i + off], o[i]), U * off, 64);
                o[i] = pick(m, o[i], got);
                o[i + off] = pick(m, got, o[i + off]);
            }
        }
        if (row0 + lane < n) {
#pragma unroll
            for (int b = 0; b < B; ++b) out.p[b][row0 + lane] = o[b];
        }
    }
}

// Small index (fewer rows than the streaming kernel needs to fill the chip: an LVIS-subset index has 14 417): the
// streaming kernel gives each wave 64 rows, fetched two at a time -- 32 dependent round trips to HBM, and only
// rows / 256 workgroups.  A CU streams ~10 B per clock from HBM (MICROARCH guide), so 29 MB on 57 or 113 CUs is 10+ us
// however the loads are scheduled; the bytes have to be spread over every CU.  Here a wave takes U rows per step (all in
// flight at once), four waves a workgroup: 32 rows per workgroup, 451 workgroups for the LVIS subset.  The query comes
// through LDS (one wave's read per workgroup, from L2).  Same dot_frag / group_reduce order: identical bits.  Plain
// loads: an index this size stays in the Infinity Cache between rounds.
template <class R, int C, int U>
__global__ __launch_bounds__(256) void scan_small_kernel(const typename R::T *__restrict__ X, const float *__restrict__ q,
                                                         float *__restrict__ scores, int n, int steps) {
    __shared__ float4 ql[C * 64];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int last = n - 1;
    const int row_base = (blockIdx.x * 4 + wave) * U * steps;
    Group<R, C, U> cur, nxt;
    load_group<R, C, U, false>(cur, X, row_base, last, lane);
    for (int i = threadIdx.x; i < C * 64; i += 256) ql[i] = reinterpret_cast<const float4 *>(q)[i];
    __syncthreads();
    RowFrag<C> qf;
#pragma unroll
    for (int c = 0; c < C; ++c) qf.v[c] = ql[c * 64 + lane];
    for (int g = 0; g < steps; ++g) {
        const int row0 = row_base + g * U;
        if (row0 >= n) break;
        if (g + 1 < steps) load_group<R, C, U, false>(nxt, X, row0 + U, last, lane);
        float acc[U];
#pragma unroll
        for (int u = 0; u < U; ++u) acc[u] = dot_frag<C>(R::widen(cur.r[u]), qf);
        const float v = group_reduce<U>(acc, lane);
        if (lane < U && row0 + lane < n) scores[row0 + lane] = v;
        cur = nxt;
    }
}

// ---- the scan of a VIEW (ssw_index_create_view): scores[j] = <X[row_src[j], :], q> over the parent's matrix -----------
// Row j of the view is row row_src[j] of X.  The wave reads the 64 (small form: U * steps) source rows of its batch with
// one coalesced load, lane l holding the source of row row0 + l, and takes the U sources of a group out of that register
// with wave-uniform lane reads (v_readlane_b32), so a row's address is formed on the SALU exactly as in the unmapped
// kernels.  Lanes past the view's last row clamp to it, as load_group does with `last`.  dot_frag / group_reduce<U> and
// the group order are the unmapped kernels': a view's score is the BITS the parent's scan gives the same row.
// (The names carry neither "scan" nor "score_rows": tests/test_index_f16_cpu.py pins the kernels so named.)
template <class R, int C, int U, bool NT>
__device__ __forceinline__ void load_view_group(Group<R, C, U> &g, const typename R::T *__restrict__ X, int src,
                                                int first_lane, int lane) {
#pragma unroll
    for (int u = 0; u < U; ++u) g.r[u] = R::template load<C, NT>(X, __builtin_amdgcn_readlane(src, first_lane + u), lane);
}

// streaming form: scan_scores_kernel's schedule (persistent grid, 64-row batches, groups of U, register double buffer,
// non-temporal loads); the sources of the wave's next batch are requested when a batch starts, a batch ahead of their use
template <class R, int C, int U, bool NT>
__global__ __launch_bounds__(256) void view_scores_kernel(const typename R::T *__restrict__ X,
                                                         const float *__restrict__ q,
                                                         const int32_t *__restrict__ row_src,
                                                         float *__restrict__ scores, int n) {
    constexpr int GPB = 64 / U;  // groups per batch
    const int lane = threadIdx.x & 63;
    const int gwave = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int nwaves = gridDim.x * 4;
    const int nbatches = (n + 63) >> 6;
    const int last = n - 1;
    if (gwave >= nbatches) return;

    RowFrag<C> qf;
#pragma unroll
    for (int c = 0; c < C; ++c) qf.v[c] = reinterpret_cast<const float4 *>(q)[c * 64 + lane];

    const int my_group = lane / U;
    int src = row_src[min((gwave << 6) + lane, last)];
    Group<R, C, U> cur, nxt;
    load_view_group<R, C, U, NT>(cur, X, src, 0, lane);
    for (int b = gwave; b < nbatches; b += nwaves) {
        const int row0 = b << 6;
        const int nb = b + nwaves;
        const int next0 = (nb < nbatches ? nb : b) << 6;  // no next batch: re-touch own rows
        const int src_next = row_src[min(next0 + lane, last)];
        float out = 0.0f;
#pragma unroll 2
        for (int g = 0; g < GPB; ++g) {
            // request group g+1 (or the first group of this wave's next batch) ...
            const bool more = g + 1 < GPB;
            load_view_group<R, C, U, NT>(nxt, X, more ? src : src_next, more ? (g + 1) * U : 0, lane);
            // ... then finish group g
            float acc[U];
#pragma unroll
            for (int u = 0; u < U; ++u) acc[u] = dot_frag<C>(R::widen(cur.r[u]), qf);
            const float v = group_reduce<U>(acc, lane);
            out = (my_group == g) ? v : out;
            cur = nxt;
        }
        if (row0 + lane < n) scores[row0 + lane] = out;
        src = src_next;
    }
}

// small form: scan_small_kernel's shape (U rows in flight per wave per step, the query through LDS, plain loads); the
// launcher keeps U * steps <= 64, so one register holds the sources of all the wave's rows
template <class R, int C, int U>
__global__ __launch_bounds__(256) void view_small_kernel(const typename R::T *__restrict__ X, const float *__restrict__ q,
                                                        const int32_t *__restrict__ row_src, float *__restrict__ scores,
                                                        int n, int steps) {
    __shared__ float4 ql[C * 64];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int last = n - 1;
    const int row_base = (blockIdx.x * 4 + wave) * U * steps;
    const int src = row_src[min(row_base + lane, last)];
    for (int i = threadIdx.x; i < C * 64; i += 256) ql[i] = reinterpret_cast<const float4 *>(q)[i];
    Group<R, C, U> cur, nxt;
    load_view_group<R, C, U, false>(cur, X, src, 0, lane);
    __syncthreads();
    RowFrag<C> qf;
#pragma unroll
    for (int c = 0; c < C; ++c) qf.v[c] = ql[c * 64 + lane];
    for (int g = 0; g < steps; ++g) {
        const int row0 = row_base + g * U;
        if (row0 >= n) break;
        if (g + 1 < steps) load_view_group<R, C, U, false>(nxt, X, src, (g + 1) * U, lane);
        float acc[U];
#pragma unroll
        for (int u = 0; u < U; ++u) acc[u] = dot_frag<C>(R::widen(cur.r[u]), qf);
        const float v = group_reduce<U>(acc, lane);
        if (lane < U && row0 + lane < n) scores[row0 + lane] = v;
        cur = nxt;
    }
}

// multi-query form: slab b, row j = <X[row_src[j], :], Q[b, :]>.  batch_scores_kernel's schedule and arithmetic line for
// line (persistent grid, 64-row batches, groups of U rows, nt loads, register double buffer, T groups unrolled between
// scheduling barriers, dot_frag, group_reduce<V, true>, the B x B register / lane transpose, one 256-byte store a slab);
// only the rows come as in view_scores_kernel: one coalesced row_src load per 64-row batch, requested a batch ahead,
// lanes past the view's last row clamped to it, a group's U sources taken out by load_view_group.  Slab b holds the bits
// view_scores_kernel writes for query b.  It is a kernel of its own, not an instance of a body shared with
// batch_scores_kernel: behind a shared inlined body that kernel's instances no longer compiled to what they compile to
// alone ("Batched scan of a view").  A change to either loop belongs in both.  Two more live
// registers than batch_scores_kernel (src, src_next): scan_view_batch_max_width.
template <class R, int C, int U, int B, bool NT>
__global__ __launch_bounds__(256) void view_batch_kernel(const typename R::T *__restrict__ X,
                                                        const float *__restrict__ q,  // [B, 256*C]
                                                        const int32_t *__restrict__ row_src, ScoreSlabs<B> out, int n) {
    constexpr int V = U * B;
    static_assert(V <= 64 && (B & (B - 1)) == 0 && (U & (U - 1)) == 0, "U*B (row, query) partials share one wave-wide reduce");
    constexpr int GPB = 64 / U;  // groups per batch
    constexpr int T = B <= 4 ? B : 4;  // groups unrolled per trip
    const int lane = threadIdx.x & 63;
    const int gwave = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int nwaves = gridDim.x * 4;
    const int nbatches = (n + 63) >> 6;
    const int last = n - 1;
    if (gwave >= nbatches) return;

    RowFrag<C> qf[B];
#pragma unroll
    for (int b = 0; b < B; ++b) {
#pragma unroll
        for (int c = 0; c < C; ++c) qf[b].v[c] = reinterpret_cast<const float4 *>(q)[(b * C + c) * 64 + lane];
    }

    const int my_run = lane / V;
    int src = row_src[min((gwave << 6) + lane, last)];
    Group<R, C, U> cur, nxt;
    load_view_group<R, C, U, NT>(cur, X, src, 0, lane);
    for (int bt = gwave; bt < nbatches; bt += nwaves) {
        const int row0 = bt << 6;
        const int nb = bt + nwaves;
        const int next0 = (nb < nbatches ? nb : bt) << 6;  // no next batch: re-touch own rows
        const int src_next = row_src[min(next0 + lane, last)];
        float o[B];
#pragma unroll
        for (int t = 0; t < B; ++t) o[t] = 0.0f;
#pragma unroll 1
        for (int s = 0; s < GPB / T; ++s) {
#pragma unroll
            for (int t = 0; t < T; ++t) {
                const int g = s * T + t;
                const bool more = g + 1 < GPB;
                load_view_group<R, C, U, NT>(nxt, X, more ? src : src_next, more ? (g + 1) * U : 0, lane);
                __builtin_amdgcn_sched_barrier(0);
                float acc[V];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const RowFrag<C> x = R::widen(cur.r[u]);
#pragma unroll
                    for (int b = 0; b < B; ++b) acc[b * U + u] = dot_frag<C>(x, qf[b]);
                }
                const float v = group_reduce<V, true>(acc, lane);
                const bool mine = my_run == s / (B / T);
#pragma unroll
                for (int j = 0; j < B / T; ++j) {
                    const bool here = (B == T) || (s % (B / T)) == j;  // wave-uniform
                    unsigned m = (mine && here) ? 0xffffffffu : 0u;
                    asm volatile("" : "+v"(m));
                    o[t + T * j] = pick(m, o[t + T * j], v);
                }
                cur = nxt;
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        // register t <-> query bits of the lane
#pragma unroll
        for (int off = 1; off < B; off <<= 1) {
            const unsigned m = lane_bit_mask(lane, U * off);  // (my_q & off) != 0
#pragma unroll
            for (int i = 0; i < B; ++i) {
                if ((i & off) != 0) continue;
                const float got = __shfl_xor(pick(m, o[i + off], o[i]), U * off, 64);
                o[i] = pick(m, o[i], got);
                o[i + off] = pick(m, got, o[i + off]);
            }
        }
        if (row0 + lane < n) {
#pragma unroll
            for (int b = 0; b < B; ++b) out.p[b][row0 + lane] = o[b];
        }
        src = src_next;
    }
}

// scores of an explicit list of rows, same summation order as the full scan (one wave per
// row, plain butterfly) -- stage-2 rescoring against a second vector
// (multiscale_index.py:347-349).
template <class R, int C>
__global__ __launch_bounds__(256) void score_rows_kernel(const typename R::T *__restrict__ X,
                                                        const float *__restrict__ q,
                                                        const int64_t *__restrict__ rows, int64_t n,
                                                        float *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= n) return;
    RowFrag<C> qf;
#pragma unroll
    for (int c = 0; c < C; ++c) qf.v[c] = reinterpret_cast<const float4 *>(q)[c * 64 + lane];
    const RowFrag<C> x = R::widen(R::template load<C, false>(X, (int)rows[w], lane));
    float v = dot_frag<C>(x, qf);
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) v = v + __shfl_xor(v, off, 64);
    if (lane == 0) out[w] = v;
}

// k-NN graph build, last stage (knn.hip): one wave per row re-scores its <= M candidate columns in
// the scan's summation order (so the scores are the bits a brute-force scan of that row returns),
// orders them by (score desc, row id asc) with a 64-lane bitonic network and certifies the row:
// every column outside the list has fp16-path score <= b, hence exact score <= b + E.
template <int C>
__global__ __launch_bounds__(256) void knn_rescore_kernel(const float *__restrict__ X, const int32_t *__restrict__ perm,
                                                         int r0, int rows, const uint64_t *__restrict__ buf, int cap,
                                                         const unsigned *__restrict__ cnt,
                                                         const unsigned char *__restrict__ overflow, int M,
                                                         const float *__restrict__ norms, float inv_scale2,
                                                         float maxnorm, int k1, int32_t *__restrict__ out_dst,
                                                         float *__restrict__ out_score,
                                                         unsigned char *__restrict__ out_cert) {
    const int lane = threadIdx.x & 63;
    const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= rows) return;
    const int orig_i = perm[r0 + w];
    const int c = min((int)cnt[w], M);
    const uint64_t key = lane < c ? buf[(int64_t)w * cap + lane] : 0ull;
    const int orig_c = lane < c ? perm[0xFFFFFFFFu - (uint32_t)key] : -1;
    const float approx = ord_to_f32((uint32_t)(key >> 32));  // fp16-path score (scaled)
    const RowFrag<C> xi = F32Rows::load<C, false>(X, orig_i, lane);
    float mine = -INFINITY;
    for (int t = 0; t < c; ++t) {
        const int j = __shfl(orig_c, t, 64);
        const RowFrag<C> xj = F32Rows::load<C, false>(X, j, lane);
        float v = dot_frag<C>(xj, xi);
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) v = v + __shfl_xor(v, off, 64);
        if (lane == t) mine = v;
    }
    uint32_t hi = lane < c ? f32_to_ord(mine) : 0u, lo = lane < c ? 0xFFFFFFFFu - (uint32_t)orig_c : 0u;
#pragma unroll
    for (int size = 2; size <= 64; size <<= 1) {
#pragma unroll
        for (int stride = size >> 1; stride >= 1; stride >>= 1) {
            const uint32_t ohi = __shfl_xor(hi, stride, 64), olo = __shfl_xor(lo, stride, 64);
            const bool desc = (lane & size) == 0, lower = (lane & stride) == 0;
            const bool other_gt = ohi > hi || (ohi == hi && olo > lo);
            if ((lower == desc) == other_gt) {  // keep the larger key on the descending side's lower lane
                hi = ohi;
                lo = olo;
            }
        }
    }
    const bool have = (hi | lo) != 0u;
    const float score = have ? ord_to_f32(hi) : -INFINITY;
    if (lane < k1) {
        out_dst[(int64_t)orig_i * k1 + lane] = have ? (int32_t)(0xFFFFFFFFu - lo) : -1;
        out_score[(int64_t)orig_i * k1 + lane] = score;
    }
    const float s_k1 = __shfl(score, k1 - 1, 64);
    const float b = __shfl(approx, M - 1, 64) * inv_scale2;  // meaningful when c == M
    if (lane == 0) {
        const float E = 1.2e-3f * norms[orig_i] * maxnorm + 2.5e-5f * maxnorm * maxnorm;
        const bool cert = !overflow[w] && (c < M || (s_k1 - E > b));
        out_cert[orig_i] = cert ? 1 : 0;
    }
}

// Schedule (measured on MI355X, interleaved A/B in one process, tools/sweep_scan.py):
// non-temporal loads are worth +4...7 %, and with them FEWER resident waves stream faster --
// at 100 M rows u2+nt with one block per CU reads 6.70 TB/s, u4 (default policy, 8 waves/SIMD)
// 6.17 TB/s; 1 M rows: 6.66 vs 5.65 TB/s.  All variants produce identical bits.
constexpr int64_t SCAN_SMALL_ROWS = 65536;  // below: the streaming kernel has under one 4-wave workgroup per CU
SSW_TUNABLE bool g_scan_small = true;       // tuning hook (ssw_tune_scan variant -2: streaming kernel at every size)
SSW_TUNABLE int g_scan_variant = -1;        // tuning hook (ssw_tune_scan): -1 = default (u2 + nt; f16: u4 + nt)
SSW_TUNABLE int g_scan_blocks_per_cu = -1;  // -1 = default (1 per CU for dim 512), 0 = as many as fit

template <class R, int C, int U, bool NT>
ssw_status launch_scan_t(const void *Xv, const float *q, float *scores, int64_t n, int device,
                         hipStream_t stream) {
    const typename R::T *X = static_cast<const typename R::T *>(Xv);
    static int max_blocks_per_cu[16] = {0};
    int dev_slot = device & 15;
    if (max_blocks_per_cu[dev_slot] == 0) {
        int nb = 0;
        SSW_HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, scan_scores_kernel<R, C, U, NT>,
                                                                 256, 0));
        if (nb < 1) nb = 1;
        if (nb > 8) nb = 8;
        max_blocks_per_cu[dev_slot] = nb;
    }
    int blocks_per_cu[16];
    blocks_per_cu[dev_slot] = max_blocks_per_cu[dev_slot];
    const int cap = g_scan_blocks_per_cu < 0 ? (C == 2 ? 1 : 2) : g_scan_blocks_per_cu;
    if (cap >= 1 && cap < blocks_per_cu[dev_slot]) blocks_per_cu[dev_slot] = cap;
    if (n >= (int64_t)0x7fff0000) {
        set_error("scan: n=%lld rows exceeds the 2^31 row limit of one index shard", (long long)n);
        return SSW_ERR_UNSUPPORTED;
    }
    if (n < SCAN_SMALL_ROWS && g_scan_small) {
        constexpr int SU = C <= 2 ? 8 : 4;
        const int64_t per_step = 4 * SU;  // rows a workgroup takes per step
        const int steps = (int)((n + 4096 * per_step - 1) / (4096 * per_step));  // 1 below 131 072 rows
        const int64_t sgrid = (n + per_step * steps - 1) / (per_step * steps);
        hipLaunchKernelGGL((scan_small_kernel<R, C, SU>), dim3((unsigned)sgrid), dim3(256), 0, stream, X, q, scores,
                           (int)n, steps);
        SSW_HIP_TRY(hipGetLastError());
        return SSW_OK;
    }
    const int64_t nbatches = (n + 63) >> 6;
    int64_t grid = (int64_t)num_cus(device) * blocks_per_cu[dev_slot];
    const int64_t need = (nbatches + 3) / 4;
    if (grid > need) grid = need;
    if (grid < 1) grid = 1;
    hipLaunchKernelGGL((scan_scores_kernel<R, C, U, NT>), dim3((unsigned)grid), dim3(256), 0, stream, X,
                       q, scores, (int)n);
    SSW_HIP_TRY(hipGetLastError());
    return SSW_OK;
}

// Batch widths are compile-time: 2, 4, 8 and 16.  The widest one the product uses is, per row format, the width with
// the lowest measured time per query (docs/EXPERIMENTS.md): 16 for f32 rows, 8 for f16 rows, with
// two four-wave blocks per CU (the second block hides what one wave's exchange chain leaves idle).
constexpr int SCAN_BATCH_MAX_F32 = 16, SCAN_BATCH_MAX_F16 = 8;
constexpr int SCAN_BATCH_BLOCKS_PER_CU = 2;
// The same per dim: the product's width (`f32`, `f16`) and the widest instance launch_scan_batch has (`*_built`, what a
// wider request of the lab hook is clamped to).  Off dim 512 the instances are those whose code object uses no scratch
// (profiles/batch_dims_resource_usage.txt): a lane holds B * C float4 of queries, so four chunks end at a width of 8,
// and three chunks take 16 only past 256 registers (copies in AGPRs, one block a CU resident).  The product's width is
// the one with the lowest time per query in profiles/batch_dims_sweep.txt, ahead of the next narrower one by more than
// the run-to-run spread at 2^20, 12.5 M and (dim 768) 50 M rows ("Batched scan at dims 256 / 768
// / 1024"): at 12.5 M rows and two blocks a CU, ms a query at 16 against 8 -- dim 256 0.277 / 0.300 (f32) and 0.257 /
// 0.275 (f16), dim 768 f32 0.694 / 0.766; dim 768 f16 is slower at 16 (0.742 / 0.507).
struct ScanBatchWidths {
    int32_t dim;
    int f32, f16, f32_built, f16_built;
};
constexpr ScanBatchWidths SCAN_BATCH_WIDTHS[] = {
    {256, 16, 16, 16, 16},
    {512, SCAN_BATCH_MAX_F32, SCAN_BATCH_MAX_F16, 16, 16},
    {768, 16, 8, 16, 16},
    {1024, 8, 8, 8, 8},
};
constexpr const ScanBatchWidths *scan_batch_widths(int32_t dim) {
    for (const ScanBatchWidths &w : SCAN_BATCH_WIDTHS)
        if (w.dim == dim) return &w;
    return nullptr;
}
SSW_TUNABLE int g_scan_batch_max = -1;  // tuning hook (ssw_tune_scan_batch): -1 = the product's widths
SSW_TUNABLE int g_scan_batch_blocks_per_cu = SCAN_BATCH_BLOCKS_PER_CU;  // the same hook: four-wave blocks per CU

// row_src: the rows are a view's (view_batch_kernel), n its rows; NULL: the matrix's own (batch_scores_kernel)
template <class R, int C, int U, int B>
ssw_status launch_scan_batch_t(const void *Xv, const float *qb, const int32_t *row_src, float *const *slabs, int64_t n,
                               int device, hipStream_t stream) {
    const typename R::T *X = static_cast<const typename R::T *>(Xv);
    ScoreSlabs<B> out;
    for (int b = 0; b < B; ++b) out.p[b] = slabs[b];
    const int per_cu = g_scan_batch_blocks_per_cu;
    const int64_t nbatches = (n + 63) >> 6;
    int64_t grid = (int64_t)num_cus(device) * per_cu;
    const int64_t need = (nbatches + 3) / 4;
    if (grid > need) grid = need;
    if (grid < 1) grid = 1;
    if (row_src)
        hipLaunchKernelGGL((view_batch_kernel<R, C, U, B, true>), dim3((unsigned)grid), dim3(256), 0, stream, X, qb,
                           row_src, out, (int)n);
    else
        hipLaunchKernelGGL((batch_scores_kernel<R, C, U, B, true>), dim3((unsigned)grid), dim3(256), 0, stream, X, qb,
                           out, (int)n);
    SSW_HIP_TRY(hipGetLastError());
    return SSW_OK;
}

template <class R>
ssw_status launch_score_rows_t(const void *Xv, const float *q_dev, const int64_t *rows_dev, int64_t n, int32_t dim,
                               float *out, hipStream_t stream) {
    const typename R::T *X = static_cast<const typename R::T *>(Xv);
    const dim3 grid((unsigned)((n + 3) / 4)), block(256);
    switch (dim) {
        case 256: hipLaunchKernelGGL((score_rows_kernel<R, 1>), grid, block, 0, stream, X, q_dev, rows_dev, n, out); break;
        case 512: hipLaunchKernelGGL((score_rows_kernel<R, 2>), grid, block, 0, stream, X, q_dev, rows_dev, n, out); break;
        case 768: hipLaunchKernelGGL((score_rows_kernel<R, 3>), grid, block, 0, stream, X, q_dev, rows_dev, n, out); break;
        case 1024: hipLaunchKernelGGL((score_rows_kernel<R, 4>), grid, block, 0, stream, X, q_dev, rows_dev, n, out); break;
        default:
            set_error("score_rows: dim=%d unsupported", dim);
            return SSW_ERR_UNSUPPORTED;
    }
    SSW_HIP_TRY(hipGetLastError());
    return SSW_OK;
}

}  // namespace

// Variants differ in schedule only (rows per group, load policy); numerics are identical.  A binary16 row is half the
// bytes of an f32 row, so the f16 schedule takes twice the rows per group (one 4-wave block per CU at dim 512 for both).
ssw_status launch_scan(const void *X, int32_t dtype, const float *q_dev, float *scores, int64_t n, int32_t dim,
                       int device, hipStream_t stream) {
    if (n <= 0) return SSW_OK;
    if (dtype == SSW_DTYPE_F16) {
        switch (dim) {
            case 256: return launch_scan_t<H16Rows, 1, 16, true>(X, q_dev, scores, n, device, stream);
            case 512:
                switch (g_scan_variant) {
                    case 0: return launch_scan_t<H16Rows, 2, 4, false>(X, q_dev, scores, n, device, stream);
                    case 1: return launch_scan_t<H16Rows, 2, 8, true>(X, q_dev, scores, n, device, stream);
                    case 4: return launch_scan_t<H16Rows, 2, 2, true>(X, q_dev, scores, n, device, stream);
                    default: return launch_scan_t<H16Rows, 2, 4, true>(X, q_dev, scores, n, device, stream);
                }
            case 768: return launch_scan_t<H16Rows, 3, 4, true>(X, q_dev, scores, n, device, stream);
            case 1024: return launch_scan_t<H16Rows, 4, 4, true>(X, q_dev, scores, n, device, stream);
        }
    } else {
        switch (dim) {
            case 256: return launch_scan_t<F32Rows, 1, 8, true>(X, q_dev, scores, n, device, stream);
            case 512:
                switch (g_scan_variant) {
                    case 0: return launch_scan_t<F32Rows, 2, 4, false>(X, q_dev, scores, n, device, stream);
                    case 2: return launch_scan_t<F32Rows, 2, 8, false>(X, q_dev, scores, n, device, stream);
                    case 3: return launch_scan_t<F32Rows, 2, 8, true>(X, q_dev, scores, n, device, stream);
                    case 4: return launch_scan_t<F32Rows, 2, 2, true>(X, q_dev, scores, n, device, stream);
                    case 1: return launch_scan_t<F32Rows, 2, 4, true>(X, q_dev, scores, n, device, stream);
                    default: return launch_scan_t<F32Rows, 2, 2, true>(X, q_dev, scores, n, device, stream);
                }
            case 768: return launch_scan_t<F32Rows, 3, 2, true>(X, q_dev, scores, n, device, stream);
            case 1024: return launch_scan_t<F32Rows, 4, 2, true>(X, q_dev, scores, n, device, stream);
        }
    }
    set_error("scan: dim=%d unsupported (need a multiple of 256, <= 1024)", dim);
    return SSW_ERR_UNSUPPORTED;
}

namespace {
// the view's scan in the default schedule of launch_scan_t: small form up to SCAN_SMALL_ROWS rows (inclusive: the
// range of the small top-k form, index_handle.h SMALL_ROWS), the persistent streaming form above
template <class R, int C, int U>
ssw_status launch_view_t(const void *Xv, const float *q, const int32_t *row_src, float *scores, int64_t n, int device,
                         hipStream_t stream) {
    const typename R::T *X = static_cast<const typename R::T *>(Xv);
    if (n <= SCAN_SMALL_ROWS) {
        constexpr int SU = C <= 2 ? 8 : 4;
        const int64_t per_step = 4 * SU;  // rows a workgroup takes per step
        const int steps = (int)((n + 4096 * per_step - 1) / (4096 * per_step));
        static_assert(SU * ((SCAN_SMALL_ROWS + 4096 * 4 * SU - 1) / (4096 * 4 * SU)) <= 64,
                      "one register holds the sources of a wave's rows");
        const int64_t sgrid = (n + per_step * steps - 1) / (per_step * steps);
        hipLaunchKernelGGL((view_small_kernel<R, C, SU>), dim3((unsigned)sgrid), dim3(256), 0, stream, X, q, row_src,
                           scores, (int)n, steps);
        SSW_HIP_TRY(hipGetLastError());
        return SSW_OK;
    }
    const int64_t nbatches = (n + 63) >> 6;
    int64_t grid = (int64_t)num_cus(device) * (C == 2 ? 1 : 2);  // launch_scan_t's residency
    const int64_t need = (nbatches + 3) / 4;
    if (grid > need) grid = need;
    hipLaunchKernelGGL((view_scores_kernel<R, C, U, true>), dim3((unsigned)grid), dim3(256), 0, stream, X, q, row_src,
                       scores, (int)n);
    SSW_HIP_TRY(hipGetLastError());
    return SSW_OK;
}
}  // namespace

// scores[j] = <X[row_src[j], :], q> for j < n_view: the bits launch_scan gives row row_src[j].  row_src [n_view] i32
// (device), every entry a row of X; the rows per group are launch_scan's defaults.
ssw_status launch_scan_view(const void *X, int32_t dtype, const float *q_dev, const int32_t *row_src, float *scores,
                            int64_t n_view, int32_t dim, int device, hipStream_t stream) {
    if (n_view <= 0) return SSW_OK;
    if (n_view >= (int64_t)0x7fff0000) {
        set_error("scan: a view of %lld rows exceeds the 2^31 row limit of one index shard", (long long)n_view);
        return SSW_ERR_UNSUPPORTED;
    }
    if (dtype == SSW_DTYPE_F16) {
        switch (dim) {
            case 256: return launch_view_t<H16Rows, 1, 16>(X, q_dev, row_src, scores, n_view, device, stream);
            case 512: return launch_view_t<H16Rows, 2, 4>(X, q_dev, row_src, scores, n_view, device, stream);
            case 768: return launch_view_t<H16Rows, 3, 4>(X, q_dev, row_src, scores, n_view, device, stream);
            case 1024: return launch_view_t<H16Rows, 4, 4>(X, q_dev, row_src, scores, n_view, device, stream);
        }
    } else {
        switch (dim) {
            case 256: return launch_view_t<F32Rows, 1, 8>(X, q_dev, row_src, scores, n_view, device, stream);
            case 512: return launch_view_t<F32Rows, 2, 2>(X, q_dev, row_src, scores, n_view, device, stream);
            case 768: return launch_view_t<F32Rows, 3, 2>(X, q_dev, row_src, scores, n_view, device, stream);
            case 1024: return launch_view_t<F32Rows, 4, 2>(X, q_dev, row_src, scores, n_view, device, stream);
        }
    }
    set_error("scan: dim=%d unsupported (need a multiple of 256, <= 1024)", dim);
    return SSW_ERR_UNSUPPORTED;
}

// The widest batch launch_scan_batch takes for this shape: the multi-query kernel serves every dim of the width table
// from the streaming kernel's range on; 1 = every query goes through launch_scan.  A width asked for through the lab
// hook is clamped to the widest instance of the shape, so that a chunk is never refused in the middle of a batch.
int scan_batch_max_width(int64_t n, int32_t dim, int32_t dtype) {
    const ScanBatchWidths *w = scan_batch_widths(dim);
    if (w == nullptr || n < SCAN_SMALL_ROWS || n >= (int64_t)0x7fff0000) return 1;
    const bool h16 = dtype == SSW_DTYPE_F16;
    const int built = h16 ? w->f16_built : w->f32_built;
    if (g_scan_batch_max > 0) return g_scan_batch_max < built ? g_scan_batch_max : built;
    return h16 ? w->f16 : w->f32;
}

// The same for a view of n rows.  A width whose view_batch_kernel instance used scratch would be narrowed here; none
// does: every instance holds two registers more than batch_scores_kernel's and stays at its occupancy, the 16-wide ones
// at dim 768 and f16 dim 512 past 256 registers as theirs are (profiles/view_batch_resource_usage.txt), so the widths
// are the matrix's own.
int scan_view_batch_max_width(int64_t n, int32_t dim, int32_t dtype) { return scan_batch_max_width(n, dim, dtype); }

namespace {
// the instance of a width nb the callers below have checked: over the matrix's own rows (row_src NULL) or a view's
ssw_status scan_batch_dispatch(const void *X, int32_t dtype, const float *qb_dev, const int32_t *row_src,
                               float *const *slabs, int32_t nb, int64_t n, int32_t dim, int device, hipStream_t stream) {
    const bool h16 = dtype == SSW_DTYPE_F16;
    // <row format, chunks, rows a group, width>.  Rows a group: launch_scan's value at the dim, halved where U * B would
    // pass the 64 partials of one reduce (dim 256) or the registers ask for it.
#define SSW_BATCH_ARGS (X, qb_dev, row_src, slabs, n, device, stream)
    switch (dim) {
        case 256:
            switch (nb) {
                case 2:
                    return h16 ? launch_scan_batch_t<H16Rows, 1, 16, 2> SSW_BATCH_ARGS
                               : launch_scan_batch_t<F32Rows, 1, 8, 2> SSW_BATCH_ARGS;
                case 4:
                    return h16 ? launch_scan_batch_t<H16Rows, 1, 16, 4> SSW_BATCH_ARGS
                               : launch_scan_batch_t<F32Rows, 1, 8, 4> SSW_BATCH_ARGS;
                case 8:
                    return h16 ? launch_scan_batch_t<H16Rows, 1, 8, 8> SSW_BATCH_ARGS
                               : launch_scan_batch_t<F32Rows, 1, 8, 8> SSW_BATCH_ARGS;
                case 16:
                    return h16 ? launch_scan_batch_t<H16Rows, 1, 4, 16> SSW_BATCH_ARGS
                               : launch_scan_batch_t<F32Rows, 1, 4, 16> SSW_BATCH_ARGS;
            }
            break;
        case 512:
            switch (nb) {
                case 2:
                    return h16 ? launch_scan_batch_t<H16Rows, 2, 4, 2> SSW_BATCH_ARGS
                               : launch_scan_batch_t<F32Rows, 2, 2, 2> SSW_BATCH_ARGS;
                case 4:
                    return h16 ? launch_scan_batch_t<H16Rows, 2, 4, 4> SSW_BATCH_ARGS
                               : launch_scan_batch_t<F32Rows, 2, 2, 4> SSW_BATCH_ARGS;
                case 8:
                    return h16 ? launch_scan_batch_t<H16Rows, 2, 4, 8> SSW_BATCH_ARGS
                               : launch_scan_batch_t<F32Rows, 2, 2, 8> SSW_BATCH_ARGS;
                case 16:
                    return h16 ? launch_scan_batch_t<H16Rows, 2, 4, 16> SSW_BATCH_ARGS
                               : launch_scan_batch_t<F32Rows, 2, 2, 16> SSW_BATCH_ARGS;
            }
            break;
        case 768:
            switch (nb) {
                case 2:
                    return h16 ? launch_scan_batch_t<H16Rows, 3, 4, 2> SSW_BATCH_ARGS
                               : launch_scan_batch_t<F32Rows, 3, 2, 2> SSW_BATCH_ARGS;
                case 4:
                    return h16 ? launch_scan_batch_t<H16Rows, 3, 4, 4> SSW_BATCH_ARGS
                               : launch_scan_batch_t<F32Rows, 3, 2, 4> SSW_BATCH_ARGS;
                case 8:
                    return h16 ? launch_scan_batch_t<H16Rows, 3, 4, 8> SSW_BATCH_ARGS
                               : launch_scan_batch_t<F32Rows, 3, 2, 8> SSW_BATCH_ARGS;
                case 16:  // 48 float4 of queries a lane: no scratch, but past 256 registers (one block a CU at most)
                    return h16 ? launch_scan_batch_t<H16Rows, 3, 2, 16> SSW_BATCH_ARGS
                               : launch_scan_batch_t<F32Rows, 3, 1, 16> SSW_BATCH_ARGS;
            }
            break;
        case 1024:
            switch (nb) {
                case 2:
                    return h16 ? launch_scan_batch_t<H16Rows, 4, 4, 2> SSW_BATCH_ARGS
                               : launch_scan_batch_t<F32Rows, 4, 2, 2> SSW_BATCH_ARGS;
                case 4:
                    return h16 ? launch_scan_batch_t<H16Rows, 4, 4, 4> SSW_BATCH_ARGS
                               : launch_scan_batch_t<F32Rows, 4, 2, 4> SSW_BATCH_ARGS;
                case 8:  // 32 float4 of queries a lane: half launch_scan's rows a group keeps two blocks a CU
                    return h16 ? launch_scan_batch_t<H16Rows, 4, 2, 8> SSW_BATCH_ARGS
                               : launch_scan_batch_t<F32Rows, 4, 1, 8> SSW_BATCH_ARGS;
            }
            break;
    }
#undef SSW_BATCH_ARGS
    set_error("scan_batch: width %d has no kernel in this build", nb);
    return SSW_ERR_UNSUPPORTED;
}
}  // namespace

// slabs[b][i] = <X[i,:], qb[b,:]> for b < nb (a power of two, 2 <= nb <= scan_batch_max_width): the bits of launch_scan
// per query
ssw_status launch_scan_batch(const void *X, int32_t dtype, const float *qb_dev, float *const *slabs, int32_t nb,
                             int64_t n, int32_t dim, int device, hipStream_t stream) {
    if (n <= 0) return SSW_OK;
    if (nb < 2 || nb > scan_batch_max_width(n, dim, dtype)) {
        set_error("scan_batch: a batch of %d queries over %lld rows of dim %d has no kernel", nb, (long long)n, dim);
        return SSW_ERR_UNSUPPORTED;
    }
    return scan_batch_dispatch(X, dtype, qb_dev, nullptr, slabs, nb, n, dim, device, stream);
}

// slabs[b][j] = <X[row_src[j],:], qb[b,:]> for j < n_view, b < nb (a power of two, 2 <= nb <= scan_view_batch_max_width):
// the bits of launch_scan_view per query.  row_src [n_view] i32 (device), every entry a row of X
ssw_status launch_scan_view_batch(const void *X, int32_t dtype, const float *qb_dev, const int32_t *row_src,
                                  float *const *slabs, int32_t nb, int64_t n_view, int32_t dim, int device,
                                  hipStream_t stream) {
    if (n_view <= 0) return SSW_OK;
    if (row_src == nullptr || nb < 2 || nb > scan_view_batch_max_width(n_view, dim, dtype)) {
        set_error("scan_view_batch: a batch of %d queries over a view of %lld rows of dim %d has no kernel", nb,
                  (long long)n_view, dim);
        return SSW_ERR_UNSUPPORTED;
    }
    return scan_batch_dispatch(X, dtype, qb_dev, row_src, slabs, nb, n_view, dim, device, stream);
}

ssw_status launch_score_rows(const void *X, int32_t dtype, const float *q_dev, const int64_t *rows_dev, int64_t n,
                             int32_t dim, float *out, hipStream_t stream) {
    if (n <= 0) return SSW_OK;
    if (dtype == SSW_DTYPE_F16) return launch_score_rows_t<H16Rows>(X, q_dev, rows_dev, n, dim, out, stream);
    return launch_score_rows_t<F32Rows>(X, q_dev, rows_dev, n, dim, out, stream);
}

ssw_status launch_knn_rescore(const float *X, int32_t dim, const int32_t *perm, int r0, int rows, const uint64_t *buf,
                              int cap, const unsigned *cnt, const unsigned char *overflow, int M, const float *norms,
                              float scale, float maxnorm, int k1, int32_t *out_dst, float *out_score,
                              unsigned char *out_cert, hipStream_t stream) {
    if (rows <= 0) return SSW_OK;
    const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
    const float inv_scale2 = 1.0f / (scale * scale);
#define SSW_KNN_RESCORE(C)                                                                                          \
    hipLaunchKernelGGL(knn_rescore_kernel<C>, grid, block, 0, stream, X, perm, r0, rows, buf, cap, cnt, overflow, M, \
                       norms, inv_scale2, maxnorm, k1, out_dst, out_score, out_cert)
    switch (dim) {
        case 256: SSW_KNN_RESCORE(1); break;
        case 512: SSW_KNN_RESCORE(2); break;
        case 768: SSW_KNN_RESCORE(3); break;
        case 1024: SSW_KNN_RESCORE(4); break;
        default:
            set_error("knn_rescore: dim=%d unsupported", dim);
            return SSW_ERR_UNSUPPORTED;
    }
#undef SSW_KNN_RESCORE
    SSW_HIP_TRY(hipGetLastError());
    return SSW_OK;
}

// ---- moving rows between natural-order f32 and the index (upload, download, gather) --------------------------------
namespace {
// one thread per 4-element group of a row (8 bytes of binary16, one float4)
template <bool FROM_F32>
__global__ __launch_bounds__(256) void k_rows_to_h16(const float *__restrict__ src_f32,
                                                     const uint16_t *__restrict__ src_h16, int64_t n, int dim,
                                                     uint16_t *__restrict__ dst) {
    const int groups = dim >> 2;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n * groups) return;
    const int64_t r = t / groups;
    const int e = (int)(t - r * groups) << 2;
    u32x2 w;
    if constexpr (FROM_F32) w = round_h16x4(reinterpret_cast<const float4 *>(src_f32 + r * dim)[e >> 2]);
    else w = reinterpret_cast<const u32x2 *>(src_h16 + r * dim)[e >> 2];
    *reinterpret_cast<u32x2 *>(dst + r * dim + h16_group_pos(e, dim >> 8)) = w;
}

// one 128-thread block per row, one thread per 4-element group
template <class R>
__global__ void k_gather_rows(const typename R::T *__restrict__ X, const int64_t *__restrict__ rows, int64_t first_row,
                              int dim, float *__restrict__ out) {
    const int64_t i = blockIdx.x;
    const typename R::T *src = X + (rows ? rows[i] : first_row + i) * dim;
    float4 *dst = reinterpret_cast<float4 *>(out + i * dim);
    for (int c = threadIdx.x; c < dim / 4; c += blockDim.x) dst[c] = R::group4(src, 4 * c, dim);
}
}  // namespace

ssw_status launch_rows_to_h16(const float *src_f32, const uint16_t *src_h16, int64_t n, int32_t dim, uint16_t *dst,
                              hipStream_t stream) {
    if (n <= 0) return SSW_OK;
    if (dim <= 0 || dim % 256 != 0 || dim > 1024) {
        set_error("rows_to_h16: dim=%d unsupported", dim);
        return SSW_ERR_UNSUPPORTED;
    }
    const int64_t blocks = (n * (dim / 4) + 255) / 256;
    if (src_f32)
        hipLaunchKernelGGL(k_rows_to_h16<true>, dim3((unsigned)blocks), dim3(256), 0, stream, src_f32, nullptr, n, (int)dim, dst);
    else
        hipLaunchKernelGGL(k_rows_to_h16<false>, dim3((unsigned)blocks), dim3(256), 0, stream, nullptr, src_h16, n, (int)dim, dst);
    SSW_HIP_TRY(hipGetLastError());
    return SSW_OK;
}

ssw_status launch_gather_rows(const void *X, int32_t dtype, const int64_t *rows_or_null, int64_t first_row, int64_t n,
                              int32_t dim, float *out, hipStream_t stream) {
    if (n <= 0) return SSW_OK;
    if (dtype == SSW_DTYPE_F16)
        hipLaunchKernelGGL(k_gather_rows<H16Rows>, dim3((unsigned)n), dim3(128), 0, stream,
                           static_cast<const uint16_t *>(X), rows_or_null, first_row, (int)dim, out);
    else
        hipLaunchKernelGGL(k_gather_rows<F32Rows>, dim3((unsigned)n), dim3(128), 0, stream,
                           static_cast<const float *>(X), rows_or_null, first_row, (int)dim, out);
    SSW_HIP_TRY(hipGetLastError());
    return SSW_OK;
}

#ifdef SSW_DEBUG_HOOKS
void tune_scan(int variant, int blocks_per_cu) {
    g_scan_small = variant == -1;  // an explicit variant (or -2) means the streaming kernel at every size
    if (variant < -1) variant = -1;
    g_scan_variant = variant;
    g_scan_blocks_per_cu = blocks_per_cu;
}
void tune_scan_batch(int max_width, int blocks_per_cu) {
    g_scan_batch_max = (max_width == 1 || max_width == 2 || max_width == 4 || max_width == 8 || max_width == 16)
                           ? max_width : -1;
    g_scan_batch_blocks_per_cu = (blocks_per_cu >= 1 && blocks_per_cu <= 8) ? blocks_per_cu : SCAN_BATCH_BLOCKS_PER_CU;
}
#endif

}  // namespace ssw

// lknn.hip -- L-KNN active search: the two-step look-ahead score of every node in one pass (gfx950 / MI355X).
//
// Replaces _top_sum as _opt_expected_utility_helper_lknn2 calls it
// (seesaw/research/active_search/efficient_nonmyopic_search.py:94-205; model: seesaw/loops/LKNN_model.py:76-281):
//   for every node i:  E_y(i) = sum of the K largest scores among all OTHER unlabelled nodes, had i been labelled y
//   (labelling i changes only the scores of i's D neighbours: (num_j + y) / (den_j + 1));
//   value(i) = s_i (1 + E_1(i)) + (1 - s_i) E_0(i);   next node = nanargmax(value).
// The reference materialises, for every node, the K + D globally best scores plus its D neighbours' new scores --
// an N x (K + 2D) f64 matrix, twice -- and argsorts every row (seconds at 10^5 nodes, O(N (K+2D)) memory).
//
// Here nothing is materialised.  The K + D globally best (id, score) pairs are shared by all rows and already
// sorted; a row only (a) strikes out of that list itself and those of its neighbours that are in it (each node's
// rank in the list is a 4-byte gather), and (b) merges what is left with its D neighbours' new scores, sorted in
// registers -- a two-pointer merge that stops after K picks.  One thread per row, O(K + D log D) work, no LDS
// beyond the shared list, D random 20-byte gathers per row: bound by those gathers (lines out of L2 / Infinity
// Cache), nowhere near HBM.
//
// Bit-exactness: the K picked values come out in descending order, exactly the row numpy sums, and the sum is
// formed in numpy's pairwise order for a contiguous row of K <= 128 doubles (8 running sums over the elements
// 0..8 floor(K/8), combined ((0+1)+(2+3))+((4+5)+(6+7)), then the tail one by one; plain left-to-right below
// 8 elements).  Divisions and the final combination are single IEEE operations, as numpy's elementwise ops.
#include <algorithm>
#include <cmath>
#include <vector>

#include "ssw_common.h"

// Compiled with -ffp-contract=off (csrc/Makefile): results of this file are compared bit for bit with numpy /
// scipy / torch, so every product and sum must round on its own (hipcc would contract a * b + c into an fma).

namespace ssw {
namespace {

constexpr int LK_THREADS = 256;
constexpr int LK_MAX_D = 32;      // neighbours per node held in registers
constexpr int LK_MAX_LIST = 192;  // K + D entries of the shared list (3 x 64-bit strike-out mask)

// numpy's pairwise summation of a contiguous row of n <= 128 doubles (np.add.reduce over the last axis), fed in order:
// n < 8: res = 0.; res += a[i].  Otherwise r[j] = a[j] (j < 8); r[j] += a[i + j] over i = 8, 16, ... < n - n % 8;
// res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)); then res += a[i] for the n % 8 tail elements.
struct RowSum {
    double r[8];
    double res;
    int n, i, body;
    bool combined;
    __device__ void init(int count) {
        n = count;
        i = 0;
        body = count < 8 ? 0 : count - (count % 8);
        res = 0.0;
        combined = false;
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] = 0.0;
    }
    __device__ void add(double v) {
        if (n < 8) {
            res = __dadd_rn(res, v);  // res = 0.; res += a[i]
        } else if (i < 8) {
#pragma unroll
            for (int q = 0; q < 8; ++q)
                if (q == i) r[q] = v;
        } else if (i < body) {
            const int j = i & 7;
#pragma unroll
            for (int q = 0; q < 8; ++q)
                if (q == j) r[q] = __dadd_rn(r[q], v);
        } else {
            if (!combined) {
                res = __dadd_rn(__dadd_rn(__dadd_rn(r[0], r[1]), __dadd_rn(r[2], r[3])),
                                __dadd_rn(__dadd_rn(r[4], r[5]), __dadd_rn(r[6], r[7])));
                combined = true;
            }
            res = __dadd_rn(res, v);
        }
        ++i;
    }
    __device__ double result() {
        if (n >= 8 && !combined)
            res = __dadd_rn(__dadd_rn(__dadd_rn(r[0], r[1]), __dadd_rn(r[2], r[3])),
                            __dadd_rn(__dadd_rn(r[4], r[5]), __dadd_rn(r[6], r[7])));
        return res;
    }
};

// Every kernel body below is a __device__ function: the single kernels hand it their arguments, the *_batch kernels (at
// the end of the namespace) the fields of their slot's descriptor -- one body, the same bits.  blockIdx.x / threadIdx.x
// mean the same in both; the slot of a batch kernel is blockIdx.y.
__device__ __forceinline__ void lk_mark_body(int32_t *__restrict__ rank_in_list, const int32_t *__restrict__ list_ids, int L) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < L) rank_in_list[list_ids[j]] = j;
}

__device__ __forceinline__ void lk_unmark_body(int32_t *__restrict__ rank_in_list, const int32_t *__restrict__ list_ids, int L) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < L) rank_in_list[list_ids[j]] = -1;
}

__global__ void k_lknn_mark(int32_t *__restrict__ rank_in_list, const int32_t *__restrict__ list_ids, int L) {
    lk_mark_body(rank_in_list, list_ids, L);
}

__global__ void k_lknn_unmark(int32_t *__restrict__ rank_in_list, const int32_t *__restrict__ list_ids, int L) {
    lk_unmark_body(rank_in_list, list_ids, L);
}

// numer: numerators + gamma (-inf for labelled nodes); denom: denominators + 1
// lscore: the workgroup's [LK_MAX_LIST] doubles of LDS
__device__ __forceinline__ void lk_top_sum_body(double *lscore, int64_t n, int D, int K, int L,
                                                const int32_t *__restrict__ nbr /* [n, D] ascending */,
                                                const double *__restrict__ numer, const double *__restrict__ denom,
                                                const int32_t *__restrict__ list_ids /* [L] score desc */,
                                                const int32_t *__restrict__ rank_in_list, double *__restrict__ out) {
    for (int j = threadIdx.x; j < L; j += LK_THREADS) {
        const int id = list_ids[j];
        lscore[j] = numer[id] / denom[id];
    }
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * LK_THREADS + threadIdx.x;
    if (i >= n) return;
    unsigned long long gone[3] = {0ull, 0ull, 0ull};  // list entries struck out for this row
    auto strike = [&](int rk) {
        if (rk >= 0) gone[rk >> 6] |= 1ull << (rk & 63);
    };
    strike(rank_in_list[i]);
    double s1[LK_MAX_D], s0[LK_MAX_D];
    for (int d = 0; d < LK_MAX_D; ++d) {
        if (d < D) {
            const int j = nbr[i * D + d];
            strike(rank_in_list[j]);
            const double nd = __dadd_rn(denom[j], 1.0);
            const double nj = numer[j];
            const bool self = j == (int)i;
            s0[d] = self ? -INFINITY : __ddiv_rn(nj, nd);
            s1[d] = self ? -INFINITY : __ddiv_rn(__dadd_rn(nj, 1.0), nd);
        } else {
            s0[d] = s1[d] = -INFINITY;
        }
    }
    // the neighbours' new scores in descending order (insertion sort in registers; D <= 32)
    auto sort_desc = [&](double *a) {
        for (int p = 1; p < LK_MAX_D; ++p) {
            if (p >= D) break;
            const double v = a[p];
            int q = p - 1;
            while (q >= 0 && a[q] < v) {
                a[q + 1] = a[q];
                --q;
            }
            a[q + 1] = v;
        }
    };
    sort_desc(s0);
    sort_desc(s1);
    auto top_sum = [&](const double *nb) -> double {
        RowSum acc;
        acc.init(K);
        int a = 0, b = 0;
        for (int picked = 0; picked < K; ++picked) {
            while (a < L && ((gone[a >> 6] >> (a & 63)) & 1ull)) ++a;
            const double va = a < L ? lscore[a] : -INFINITY;
            const double vb = b < D ? nb[b] : -INFINITY;
            if (va >= vb) {
                acc.add(va);
                ++a;
            } else {
                acc.add(vb);
                ++b;
            }
        }
        return acc.result();
    };
    const double e1 = top_sum(s1), e0 = top_sum(s0);
    const double s = __ddiv_rn(numer[i], denom[i]);
    // scores * (1 + expected1) + (1 - scores) * expected0, one rounding per operation as numpy evaluates it
    out[i] = __dadd_rn(__dmul_rn(s, __dadd_rn(1.0, e1)), __dmul_rn(__dadd_rn(1.0, -s), e0));
}

__global__ __launch_bounds__(LK_THREADS) void k_lknn_top_sum(int64_t n, int D, int K, int L,
                                                             const int32_t *__restrict__ nbr /* [n, D] ascending */,
                                                             const double *__restrict__ numer,
                                                             const double *__restrict__ denom,
                                                             const int32_t *__restrict__ list_ids /* [L] score desc */,
                                                             const int32_t *__restrict__ rank_in_list,
                                                             double *__restrict__ out) {
    __shared__ double lscore[LK_MAX_LIST];
    lk_top_sum_body(lscore, n, D, K, L, nbr, numer, denom, list_ids, rank_in_list, out);
}

// np.nanargmax: the first index of the largest non-NaN value
// sv / si: the workgroup's [LK_THREADS] entries of LDS each
__device__ __forceinline__ void lk_argmax_body(double *sv, long long *si, const double *__restrict__ v, int64_t n,
                                               double *__restrict__ best_v, long long *__restrict__ best_i) {
    double bv = -INFINITY;
    long long bi = -1;
    for (int64_t i = (int64_t)blockIdx.x * LK_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * LK_THREADS) {
        const double x = v[i];
        if (x != x) continue;
        if (bi < 0 || x > bv) {
            bv = x;
            bi = i;
        }
    }
    sv[threadIdx.x] = bv;
    si[threadIdx.x] = bi;
    __syncthreads();
    for (int s = LK_THREADS / 2; s >= 1; s >>= 1) {
        if (threadIdx.x < s) {
            const double ov = sv[threadIdx.x + s];
            const long long oi = si[threadIdx.x + s];
            const bool take = oi >= 0 && (si[threadIdx.x] < 0 || ov > sv[threadIdx.x] ||
                                          (ov == sv[threadIdx.x] && oi < si[threadIdx.x]));
            if (take) {
                sv[threadIdx.x] = ov;
                si[threadIdx.x] = oi;
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        best_v[blockIdx.x] = sv[0];
        best_i[blockIdx.x] = si[0];
    }
}

__global__ __launch_bounds__(LK_THREADS) void k_lknn_argmax(const double *__restrict__ v, int64_t n,
                                                            double *__restrict__ best_v, long long *__restrict__ best_i) {
    __shared__ double sv[LK_THREADS];
    __shared__ long long si[LK_THREADS];
    lk_argmax_body(sv, si, v, n, best_v, best_i);
}

// ---- the device-resident model (ssw_lknn_state_init .. ssw_lknn_step) ------------------------------------------------
// The state of LKNNModel (numerators, denominators, gamma: f64 [n]; seen: u8 [n]) stays in HBM.  A planning step forms
// numer = numerators + gamma (-inf at seen nodes), denom = denominators + 1 and score = numer / denom in ONE pass over it
// (25 n bytes read, the 16 n bytes of numer / denom written for k_lknn_top_sum) and selects, in the same pass, the exact
// L = K + D best unseen nodes under the total order (score descending, node id ascending).
//
// The selection is a hierarchy of comparisons on whole keys -- nothing is binned by value (the prior is 0.1 +- 1e-6: every
// key shares its sign, exponent and leading mantissa bits, so a histogram of the high bits would put all nodes into one
// bin).  A workgroup keeps its best 256 candidates sorted in the lower half of a 512-entry LDS array (LkTop); candidates
// come 256 at a time, one a thread; those that beat the L-th best so far are appended to the upper half, and when the
// next 256 might not fit a bitonic sort orders all 512 and empties the upper half (sort and truncate).  Candidates that
// do not beat the L-th best cannot be in the result, so dropping them changes nothing; how many sorts a workgroup runs
// depends on the order the scores arrive in, between one and -- scores rising along the slice -- one per 256 candidates.
//   k_lknn_select: a workgroup reduces its slice of LK_SLICE rows to its own best L;
//   k_lknn_merge:  a workgroup reduces up to LK_FAN such lists to one, the same way; levels repeat until one list is
//                  left, which the last level writes as node ids (and scores) in order.
// A key is unique (the id breaks every tie), so the result is the same for any slice length, fan-in or grid, and for
// any order in which the LDS atomic hands out places in the upper half.
constexpr int LK_SLICE = 2048;  // rows of one workgroup of k_lknn_select
constexpr int LK_FAN = 32;      // lists one workgroup of k_lknn_merge reduces
constexpr int LK_SORT = 2 * LK_THREADS;
constexpr unsigned LK_EMPTY = 0xffffffffu;  // id of an empty entry (key 0): after every node
static_assert(LK_MAX_LIST <= LK_THREADS, "a workgroup's list is the sorted lower half");

// ascending unsigned order == ascending order of the doubles (-0 and +0 compare equal in numpy: one key)
__device__ inline unsigned long long score_key(double s) {
    if (s == 0.0) s = 0.0;
    const unsigned long long u = (unsigned long long)__double_as_longlong(s);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

__device__ inline bool lk_before(unsigned long long ka, unsigned ia, unsigned long long kb, unsigned ib) {
    return ka > kb || (ka == kb && ia < ib);
}

// a workgroup's best candidates: k / id [0, 256) sorted best first (empty entries last), [256, 256 + fill) appended since
struct LkTop {
    unsigned long long k[LK_SORT];
    unsigned id[LK_SORT];
    int fill;
};

__device__ inline void lk_clear_upper(LkTop &s) {
    s.k[LK_THREADS + threadIdx.x] = 0ull, s.id[LK_THREADS + threadIdx.x] = LK_EMPTY;
    if (threadIdx.x == 0) s.fill = 0;
    __syncthreads();
}

__device__ inline void lk_init(LkTop &s) {
    s.k[threadIdx.x] = 0ull, s.id[threadIdx.x] = LK_EMPTY;
    lk_clear_upper(s);
}

// the bitonic sort of all LK_SORT entries, best first, then the upper half emptied.  Whole workgroup.
__device__ inline void lk_flush(LkTop &s) {
    const int t = threadIdx.x;
    __syncthreads();  // the appends
    for (int size = 2; size <= LK_SORT; size <<= 1)
        for (int stride = size >> 1; stride >= 1; stride >>= 1) {
            const int lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
            const unsigned long long ka = s.k[lo], kb = s.k[hi];
            const unsigned ia = s.id[lo], ib = s.id[hi];
            const bool in_order = (lo & size) == 0;  // this run is to come out best first, the next one reversed
            if (in_order ? lk_before(kb, ib, ka, ia) : lk_before(ka, ia, kb, ib)) {
                s.k[lo] = kb, s.id[lo] = ib;
                s.k[hi] = ka, s.id[hi] = ia;
            }
            __syncthreads();
        }
    lk_clear_upper(s);
}

// every thread of the workgroup offers one candidate (id LK_EMPTY: none).  fill: the thread's copy of s.fill, the same
// in all threads.  The L-th best so far (an empty entry while there are fewer) is read from the lower half, which only
// lk_flush changes; the barrier inside the count separates that from this call's appends.
__device__ inline void lk_offer(LkTop &s, int L, unsigned long long key, unsigned id, int &fill) {
    const bool beats = id != LK_EMPTY && lk_before(key, id, s.k[L - 1], s.id[L - 1]);
    const int count = __syncthreads_count(beats);
    if (count == 0) return;
    if (fill + count > LK_THREADS) {
        lk_flush(s);
        fill = 0;
    }
    if (beats) {
        const int at = LK_THREADS + atomicAdd(&s.fill, 1);
        s.k[at] = key, s.id[at] = id;
    }
    fill += count;
}

__device__ __forceinline__ void lk_select_body(LkTop &top, int64_t n, int L, const double *__restrict__ numerators,
                                               const double *__restrict__ denominators, const double *__restrict__ gamma,
                                               const unsigned char *__restrict__ seen, double *__restrict__ numer,
                                               double *__restrict__ denom, unsigned long long *__restrict__ out_keys,
                                               unsigned *__restrict__ out_ids) {
    const int t = threadIdx.x;
    lk_init(top);
    int fill = 0;
    const int64_t first = (int64_t)blockIdx.x * LK_SLICE;
    const int64_t last = first + LK_SLICE < n ? first + LK_SLICE : n;
    for (int64_t c = first; c < last; c += LK_THREADS) {
        const int64_t i = c + t;
        unsigned long long key = 0ull;
        unsigned id = LK_EMPTY;
        if (i < last) {
            const bool gone = seen[i] != 0;
            const double nu = gone ? -INFINITY : __dadd_rn(numerators[i], gamma[i]);
            const double de = __dadd_rn(denominators[i], 1.0);
            numer[i] = nu;
            denom[i] = de;
            if (!gone) key = score_key(__ddiv_rn(nu, de)), id = (unsigned)i;
        }
        lk_offer(top, L, key, id, fill);
    }
    lk_flush(top);
    if (t < L) {
        out_keys[(size_t)blockIdx.x * LK_MAX_LIST + t] = top.k[t];
        out_ids[(size_t)blockIdx.x * LK_MAX_LIST + t] = top.id[t];
    }
}

__global__ __launch_bounds__(LK_THREADS) void k_lknn_select(int64_t n, int L, const double *__restrict__ numerators,
                                                            const double *__restrict__ denominators,
                                                            const double *__restrict__ gamma,
                                                            const unsigned char *__restrict__ seen,
                                                            double *__restrict__ numer, double *__restrict__ denom,
                                                            unsigned long long *__restrict__ out_keys,
                                                            unsigned *__restrict__ out_ids) {
    __shared__ LkTop top;
    lk_select_body(top, n, L, numerators, denominators, gamma, seen, numer, denom, out_keys, out_ids);
}

// final_ids != NULL (the last level, one workgroup): the list as node ids, with numer / denom of each as its score
__device__ __forceinline__ void lk_merge_body(LkTop &top, int n_lists, int L, const unsigned long long *__restrict__ in_keys,
                                              const unsigned *__restrict__ in_ids, unsigned long long *__restrict__ out_keys,
                                              unsigned *__restrict__ out_ids, int32_t *__restrict__ final_ids,
                                              double *__restrict__ final_scores, const double *__restrict__ numer,
                                              const double *__restrict__ denom) {
    const int t = threadIdx.x;
    lk_init(top);
    int fill = 0;
    const int first = blockIdx.x * LK_FAN;
    const int lists = first + LK_FAN < n_lists ? LK_FAN : n_lists - first;
    const int entries = lists * L;  // of this workgroup's lists, list after list
    for (int c = 0; c < entries; c += LK_THREADS) {
        const int e = c + t;
        unsigned long long key = 0ull;
        unsigned id = LK_EMPTY;
        if (e < entries) {
            const size_t at = (size_t)(first + e / L) * LK_MAX_LIST + e % L;
            key = in_keys[at], id = in_ids[at];
        }
        lk_offer(top, L, key, id, fill);
    }
    lk_flush(top);
    if (t >= L) return;
    if (final_ids) {
        const unsigned id = top.id[t];
        final_ids[t] = (int32_t)id;
        final_scores[t] = id == LK_EMPTY ? -INFINITY : __ddiv_rn(numer[id], denom[id]);
    } else {
        out_keys[(size_t)blockIdx.x * LK_MAX_LIST + t] = top.k[t];
        out_ids[(size_t)blockIdx.x * LK_MAX_LIST + t] = top.id[t];
    }
}

__global__ __launch_bounds__(LK_THREADS) void k_lknn_merge(int n_lists, int L, const unsigned long long *__restrict__ in_keys,
                                                           const unsigned *__restrict__ in_ids,
                                                           unsigned long long *__restrict__ out_keys,
                                                           unsigned *__restrict__ out_ids, int32_t *__restrict__ final_ids,
                                                           double *__restrict__ final_scores,
                                                           const double *__restrict__ numer,
                                                           const double *__restrict__ denom) {
    __shared__ LkTop top;
    lk_merge_body(top, n_lists, L, in_keys, in_ids, out_keys, out_ids, final_ids, final_scores, numer, denom);
}

// the one-step branch: value = score, -inf at seen nodes (k_lknn_argmax then is np.nanargmax)
__device__ __forceinline__ void lk_score_body(int64_t n, const double *__restrict__ numerators,
                                              const double *__restrict__ denominators, const double *__restrict__ gamma,
                                              const unsigned char *__restrict__ seen, double *__restrict__ value) {
    const int64_t i = (int64_t)blockIdx.x * LK_THREADS + threadIdx.x;
    if (i >= n) return;
    const double nu = seen[i] ? -INFINITY : __dadd_rn(numerators[i], gamma[i]);
    value[i] = __ddiv_rn(nu, __dadd_rn(denominators[i], 1.0));
}

__global__ __launch_bounds__(LK_THREADS) void k_lknn_score(int64_t n, const double *__restrict__ numerators,
                                                           const double *__restrict__ denominators,
                                                           const double *__restrict__ gamma,
                                                           const unsigned char *__restrict__ seen, double *__restrict__ value) {
    lk_score_body(n, numerators, denominators, gamma, seen, value);
}

// predict_proba of a few nodes: (numerators + gamma) / (denominators + 1), seen or not
__global__ void k_lknn_gather_score(int m, const int32_t *__restrict__ ids, const double *__restrict__ numerators,
                                    const double *__restrict__ denominators, const double *__restrict__ gamma,
                                    double *__restrict__ out) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= m) return;
    const int id = ids[t];
    out[t] = __ddiv_rn(__dadd_rn(numerators[id], gamma[id]), __dadd_rn(denominators[id], 1.0));
}

// condition_ for m answers in order, one workgroup of LK_MAX_D lanes: lane d owns neighbour d of the answered node.  A
// neighbour listed twice in a row counts once (numpy's `numerators[neighbors] = num + y`); rows are ascending.
__global__ __launch_bounds__(LK_MAX_D) void k_lknn_condition(int m, int D, const int32_t *__restrict__ pairs /* [m] (id, y) */,
                                                             const int32_t *__restrict__ nbr, double *__restrict__ numerators,
                                                             double *__restrict__ denominators,
                                                             unsigned char *__restrict__ seen) {
    const int d = threadIdx.x;
    for (int t = 0; t < m; ++t) {
        const int64_t id = pairs[2 * t];
        const double y = (double)pairs[2 * t + 1];
        if (d < D) {
            const int j = nbr[id * D + d];
            if (d == 0 || nbr[id * D + d - 1] != j) {
                numerators[j] = __dadd_rn(numerators[j], y);
                denominators[j] = __dadd_rn(denominators[j], 1.0);
            }
        }
        if (d == 0) seen[id] = 1;
        __syncthreads();  // the next answer may touch the same neighbours
    }
}

// ---- several handles' steps in one pass (ssw_lknn_step_batch, ssw_lknn_top_remaining_batch) --------------------------
// One descriptor a slot, in a device table; every kernel of the pass is launched once with the slot on blockIdx.y and
// runs the single kernel's body on the slot's own buffers.  The table holds the lookahead-2 slots first: the selection,
// mark, look-ahead and unmark kernels cover those, k_lknn_score_batch the lookahead-1 slots behind them, the block
// argmax and the finish all of them.
struct LkSlot {
    const double *numerators, *denominators, *gamma;
    const unsigned char *seen;
    const int32_t *nbr;
    double *numer, *denom, *value;
    int32_t *rank_in_list, *list_ids;
    double *list_scores;
    unsigned long long *keys_a, *keys_b;
    unsigned *ids_a, *ids_b;
    double *blk_v;
    long long *blk_i;
    int32_t K, L;        // L: entries of the slot's list (K + D of a step, min(k, unseen) of a top_remaining)
    int32_t slot;        // the caller's slot: where the results go in the result block
    int32_t want_list;   // the finish copies list_ids (1) and list_scores too (2) into the result block
};

// the result block of a pass (device and pinned host copy alike), for `cap` slots: the picks, then the lists
struct LkBest {
    double value;
    long long index;
};
__host__ __device__ inline size_t lk_res_ids(int cap) { return (size_t)cap * sizeof(LkBest); }
__host__ __device__ inline size_t lk_res_scores(int cap) { return lk_res_ids(cap) + (size_t)cap * LK_MAX_LIST * 4; }
__host__ __device__ inline size_t lk_res_bytes(int cap) { return lk_res_scores(cap) + (size_t)cap * LK_MAX_LIST * 8; }

__global__ __launch_bounds__(LK_THREADS) void k_lknn_select_batch(const LkSlot *__restrict__ tab, int64_t n) {
    __shared__ LkTop top;
    const LkSlot &d = tab[blockIdx.y];
    lk_select_body(top, n, d.L, d.numerators, d.denominators, d.gamma, d.seen, d.numer, d.denom, d.keys_a, d.ids_a);
}

// from_a: this level reads the slot's keys_a / ids_a and writes the others; last: it writes list_ids / list_scores
__global__ __launch_bounds__(LK_THREADS) void k_lknn_merge_batch(const LkSlot *__restrict__ tab, int n_lists, int from_a,
                                                                 int last) {
    __shared__ LkTop top;
    const LkSlot &d = tab[blockIdx.y];
    lk_merge_body(top, n_lists, d.L, from_a ? d.keys_a : d.keys_b, from_a ? d.ids_a : d.ids_b, from_a ? d.keys_b : d.keys_a,
                  from_a ? d.ids_b : d.ids_a, last ? d.list_ids : (int32_t *)nullptr, d.list_scores, d.numer, d.denom);
}

__global__ void k_lknn_mark_batch(const LkSlot *__restrict__ tab) {
    const LkSlot &d = tab[blockIdx.y];
    lk_mark_body(d.rank_in_list, d.list_ids, d.L);
}

__global__ void k_lknn_unmark_batch(const LkSlot *__restrict__ tab) {
    const LkSlot &d = tab[blockIdx.y];
    lk_unmark_body(d.rank_in_list, d.list_ids, d.L);
}

__global__ __launch_bounds__(LK_THREADS) void k_lknn_top_sum_batch(const LkSlot *__restrict__ tab, int64_t n, int D) {
    __shared__ double lscore[LK_MAX_LIST];
    const LkSlot &d = tab[blockIdx.y];
    lk_top_sum_body(lscore, n, D, d.K, d.L, d.nbr, d.numer, d.denom, d.list_ids, d.rank_in_list, d.value);
}

// tab: the first lookahead-1 slot's descriptor
__global__ __launch_bounds__(LK_THREADS) void k_lknn_score_batch(const LkSlot *__restrict__ tab, int64_t n) {
    const LkSlot &d = tab[blockIdx.y];
    lk_score_body(n, d.numerators, d.denominators, d.gamma, d.seen, d.value);
}

__global__ __launch_bounds__(LK_THREADS) void k_lknn_argmax_batch(const LkSlot *__restrict__ tab, int64_t n) {
    __shared__ double sv[LK_THREADS];
    __shared__ long long si[LK_THREADS];
    const LkSlot &d = tab[blockIdx.y];
    lk_argmax_body(sv, si, d.value, n, d.blk_v, d.blk_i);
}

// the lists of a slot into the result block: ids (want_list >= 1) and scores (want_list == 2).  L <= LK_THREADS.
__device__ inline void lk_collect(const LkSlot &d, unsigned char *__restrict__ res, int cap) {
    const int t = threadIdx.x;
    if (t >= d.L || d.want_list == 0) return;
    ((int32_t *)(res + lk_res_ids(cap)))[(size_t)d.slot * LK_MAX_LIST + t] = d.list_ids[t];
    if (d.want_list == 2) ((double *)(res + lk_res_scores(cap)))[(size_t)d.slot * LK_MAX_LIST + t] = d.list_scores[t];
}

// One workgroup a slot: the n_blocks partial results of k_lknn_argmax_batch reduced by the rule the single call's host
// loop applies to them -- the largest value, the lowest index among equal values; a partial without a candidate (index
// -1) never wins; none at all gives (0.0, -1).  (value descending, index ascending) is a total order of the partials, so
// the winner is the same element whatever the order of the reduction.
__global__ __launch_bounds__(LK_THREADS) void k_lknn_finish_batch(const LkSlot *__restrict__ tab, int n_blocks,
                                                                  unsigned char *__restrict__ res, int cap) {
    __shared__ double sv[LK_THREADS];
    __shared__ long long si[LK_THREADS];
    const LkSlot &d = tab[blockIdx.y];
    const int t = threadIdx.x;
    double bv = 0.0;
    long long bi = -1;
    for (int b = t; b < n_blocks; b += LK_THREADS) {
        const long long oi = d.blk_i[b];
        const double ov = d.blk_v[b];
        if (oi < 0) continue;
        if (bi < 0 || ov > bv || (ov == bv && oi < bi)) bv = ov, bi = oi;
    }
    sv[t] = bv;
    si[t] = bi;
    __syncthreads();
    for (int s = LK_THREADS / 2; s >= 1; s >>= 1) {
        if (t < s) {
            const double ov = sv[t + s];
            const long long oi = si[t + s];
            if (oi >= 0 && (si[t] < 0 || ov > sv[t] || (ov == sv[t] && oi < si[t]))) sv[t] = ov, si[t] = oi;
        }
        __syncthreads();
    }
    if (t == 0) {
        LkBest *best = (LkBest *)res;
        best[d.slot].value = si[0] < 0 ? 0.0 : sv[0];
        best[d.slot].index = si[0];
    }
    lk_collect(d, res, cap);
}

// top_remaining: nothing but the lists to bring home
__global__ __launch_bounds__(LK_THREADS) void k_lknn_collect_batch(const LkSlot *__restrict__ tab, unsigned char *__restrict__ res,
                                                                   int cap) {
    lk_collect(tab[blockIdx.y], res, cap);
}

}  // namespace
}  // namespace ssw

using namespace ssw;

struct ssw_lknn {
    int device = 0;
    int64_t n = 0;
    int D = 0;
    int32_t *nbr = nullptr;           // [n, D] ascending per row
    double *numer = nullptr, *denom = nullptr, *value = nullptr;  // [n]
    int32_t *rank_in_list = nullptr;  // [n], -1 outside the shared list
    int32_t *list_ids = nullptr;      // [LK_MAX_LIST]
    double *blk_v = nullptr;
    long long *blk_i = nullptr;
    int argmax_blocks = 0;
    hipStream_t stream = nullptr;
    // the device-resident model (ssw_lknn_state_init): its own buffers, numer / denom above stay the staging of a step
    bool has_state = false;
    double *numerators = nullptr, *denominators = nullptr, *gamma = nullptr;  // [n]
    unsigned char *seen = nullptr;                                            // [n]
    std::vector<unsigned char> seen_host;  // the marks once more, for the refusals of ssw_lknn_condition
    int64_t n_seen = 0;
    int n_slices = 0;                      // workgroups of k_lknn_select
    unsigned long long *keys_a = nullptr, *keys_b = nullptr;  // [n_slices] / [ceil(n_slices / LK_FAN)] lists of LK_MAX_LIST
    unsigned *ids_a = nullptr, *ids_b = nullptr;
    double *list_scores = nullptr;         // [LK_MAX_LIST]
    int32_t *small_ids = nullptr;          // [LK_MAX_ANSWERS, 2]: the answers of a condition call, the ids of a predict call
    double *small_out = nullptr;           // [LK_MAX_ANSWERS]
    PinnedStage small_stage;
    unsigned char *pinned = nullptr;       // block results, list ids and list scores of a step
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};  // around the selection and the look-ahead (ssw_lknn_step_times)
    bool timing = false;
    int timed = 0;                         // of the last call: 1 = the selection was timed, 2 = the look-ahead too
    int64_t info[4] = {0, 0, 0, 0};        // of the last step: launches, host waits, bytes up, bytes down
    // ssw_lknn_step_batch / ssw_lknn_top_remaining_batch: the handle of a call's first slot lends the descriptor table
    // and the result block (device + pinned host copy), batch_cap slots each, grown on demand; every slot's handle has
    // the event the pass waits on and keeps the message of its own status
    LkSlot *batch_tab = nullptr;
    unsigned char *batch_res = nullptr, *batch_pinned = nullptr;
    int batch_cap = 0;
    PinnedStage batch_stage;
    hipEvent_t batch_ev = nullptr;
    std::string batch_error;
};

static constexpr int LK_MAX_ANSWERS = 4096;  // answers of one ssw_lknn_condition, nodes of one ssw_lknn_predict

extern "C" {

ssw_status ssw_lknn_destroy(ssw_lknn *h) {
    if (!h) return SSW_OK;
    DeviceGuard guard(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    for (void *p : {(void *)h->nbr, (void *)h->numer, (void *)h->denom, (void *)h->value, (void *)h->rank_in_list,
                    (void *)h->list_ids, (void *)h->blk_v, (void *)h->blk_i, (void *)h->numerators, (void *)h->denominators,
                    (void *)h->gamma, (void *)h->seen, (void *)h->keys_a, (void *)h->keys_b, (void *)h->ids_a, (void *)h->ids_b,
                    (void *)h->list_scores, (void *)h->small_ids, (void *)h->small_out})
        (void)hipFree(p);
    h->small_stage.release();
    if (h->pinned) (void)hipHostFree(h->pinned);
    (void)hipFree(h->batch_tab);
    (void)hipFree(h->batch_res);
    h->batch_stage.release();
    if (h->batch_pinned) (void)hipHostFree(h->batch_pinned);
    if (h->batch_ev) (void)hipEventDestroy(h->batch_ev);
    for (hipEvent_t e : h->ev)
        if (e) (void)hipEventDestroy(e);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
    return SSW_OK;
}

ssw_status ssw_lknn_create(int32_t device, int64_t n, int32_t D, const int32_t *neighbors_sorted_host, ssw_lknn **out) {
    SSW_REQUIRE(out != nullptr, "out is NULL");
    *out = nullptr;
    SSW_REQUIRE(n > 0 && D >= 1 && D <= LK_MAX_D && neighbors_sorted_host, "lknn: n=%lld, D=%d (1..%d)", (long long)n, D, LK_MAX_D);
    SSW_REQUIRE(n < (int64_t)0x7fffffff, "lknn: node ids are 32-bit");
    for (int64_t i = 0; i < n; ++i)
        for (int d = 0; d < D; ++d) {
            const int32_t j = neighbors_sorted_host[i * D + d];
            SSW_REQUIRE(j >= 0 && j < n, "lknn: neighbour %d of node %lld out of range", j, (long long)i);
            SSW_REQUIRE(d == 0 || neighbors_sorted_host[i * D + d - 1] <= j, "lknn: neighbours of node %lld are not sorted", (long long)i);
        }
    DeviceGuard guard(device);
    ssw_lknn *h = new (std::nothrow) ssw_lknn();
    if (!h) return SSW_ERR_NOMEM;
    h->device = device;
    h->n = n;
    h->D = D;
    h->argmax_blocks = (int)std::min<int64_t>(1024, (n + LK_THREADS - 1) / LK_THREADS);
    bool ok = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) == hipSuccess &&
              hipMalloc((void **)&h->nbr, (size_t)n * D * 4) == hipSuccess &&
              hipMalloc((void **)&h->numer, (size_t)n * 8) == hipSuccess &&
              hipMalloc((void **)&h->denom, (size_t)n * 8) == hipSuccess &&
              hipMalloc((void **)&h->value, (size_t)n * 8) == hipSuccess &&
              hipMalloc((void **)&h->rank_in_list, (size_t)n * 4) == hipSuccess &&
              hipMalloc((void **)&h->list_ids, LK_MAX_LIST * 4) == hipSuccess &&
              hipMalloc((void **)&h->blk_v, (size_t)h->argmax_blocks * 8) == hipSuccess &&
              hipMalloc((void **)&h->blk_i, (size_t)h->argmax_blocks * 8) == hipSuccess &&
              hipMemcpy(h->nbr, neighbors_sorted_host, (size_t)n * D * 4, hipMemcpyHostToDevice) == hipSuccess &&
              hipMemset(h->rank_in_list, 0xff, (size_t)n * 4) == hipSuccess;
    if (!ok) {
        ssw_lknn_destroy(h);
        set_error("lknn: allocation / upload failed");
        return SSW_ERR_NOMEM;
    }
    *out = h;
    return SSW_OK;
}

ssw_status ssw_lknn_top_sum(ssw_lknn *h, const double *numer_host, const double *denom_host, const int32_t *top_ids_desc,
                            int32_t K, double *out_values_or_null, int64_t *out_best_idx, double *out_best_value) {
    SSW_REQUIRE(h && numer_host && denom_host && top_ids_desc, "NULL argument");
    const int L = K + h->D;
    SSW_REQUIRE(K >= 1 && K <= 128, "lknn: K=%d outside [1, 128] (the row sum follows numpy's order for one 128-element block)", K);
    SSW_REQUIRE(L <= LK_MAX_LIST && L <= h->n, "lknn: K + D = %d exceeds %d or the node count", L, LK_MAX_LIST);
    for (int j = 0; j < L; ++j)
        SSW_REQUIRE(top_ids_desc[j] >= 0 && top_ids_desc[j] < h->n, "lknn: list id %d out of range", top_ids_desc[j]);
    DeviceGuard guard(h->device);
    hipStream_t s = h->stream;
    const int64_t n = h->n;
    SSW_HIP_TRY(hipMemcpyAsync(h->numer, numer_host, (size_t)n * 8, hipMemcpyHostToDevice, s));
    SSW_HIP_TRY(hipMemcpyAsync(h->denom, denom_host, (size_t)n * 8, hipMemcpyHostToDevice, s));
    SSW_HIP_TRY(hipMemcpyAsync(h->list_ids, top_ids_desc, (size_t)L * 4, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_lknn_mark, dim3(1), dim3(LK_THREADS), 0, s, h->rank_in_list, h->list_ids, L);
    hipLaunchKernelGGL(k_lknn_top_sum, dim3((unsigned)((n + LK_THREADS - 1) / LK_THREADS)), dim3(LK_THREADS), 0, s, n, h->D,
                       (int)K, L, h->nbr, h->numer, h->denom, h->list_ids, h->rank_in_list, h->value);
    hipLaunchKernelGGL(k_lknn_unmark, dim3(1), dim3(LK_THREADS), 0, s, h->rank_in_list, h->list_ids, L);
    hipLaunchKernelGGL(k_lknn_argmax, dim3(h->argmax_blocks), dim3(LK_THREADS), 0, s, h->value, n, h->blk_v, h->blk_i);
    SSW_HIP_TRY(hipGetLastError());
    std::vector<double> bv((size_t)h->argmax_blocks);
    std::vector<long long> bi((size_t)h->argmax_blocks);
    SSW_HIP_TRY(hipMemcpyAsync(bv.data(), h->blk_v, bv.size() * 8, hipMemcpyDeviceToHost, s));
    SSW_HIP_TRY(hipMemcpyAsync(bi.data(), h->blk_i, bi.size() * 8, hipMemcpyDeviceToHost, s));
    if (out_values_or_null) SSW_HIP_TRY(hipMemcpyAsync(out_values_or_null, h->value, (size_t)n * 8, hipMemcpyDeviceToHost, s));
    SSW_HIP_TRY(hipStreamSynchronize(s));
    long long best = -1;
    double bval = 0.0;
    for (size_t b = 0; b < bv.size(); ++b) {
        if (bi[b] < 0) continue;
        if (best < 0 || bv[b] > bval || (bv[b] == bval && bi[b] < best)) {
            best = bi[b];
            bval = bv[b];
        }
    }
    if (out_best_idx) *out_best_idx = best;
    if (out_best_value) *out_best_value = bval;
    return SSW_OK;
}

}  // extern "C"

// ---- the device-resident model ---------------------------------------------------------------------------------------
namespace {

ssw_status check_gamma(const ssw_lknn *h, const double *gamma_host) {
    for (int64_t i = 0; i < h->n; ++i)
        SSW_REQUIRE(std::isfinite(gamma_host[i]), "lknn: gamma of node %lld is not finite", (long long)i);
    return SSW_OK;
}

void free_state(ssw_lknn *h) {
    for (void **p : {(void **)&h->numerators, (void **)&h->denominators, (void **)&h->gamma, (void **)&h->seen, (void **)&h->keys_a,
                     (void **)&h->keys_b, (void **)&h->ids_a, (void **)&h->ids_b, (void **)&h->list_scores, (void **)&h->small_ids,
                     (void **)&h->small_out}) {
        (void)hipFree(*p);
        *p = nullptr;
    }
    if (h->pinned) (void)hipHostFree(h->pinned);
    h->pinned = nullptr;
    h->has_state = false;
}

// the places of a step's small results in the pinned block
size_t pinned_blk_i(const ssw_lknn *h) { return (size_t)h->argmax_blocks * 8; }
size_t pinned_list_ids(const ssw_lknn *h) { return (size_t)h->argmax_blocks * 16; }
size_t pinned_list_scores(const ssw_lknn *h) { return pinned_list_ids(h) + LK_MAX_LIST * 4; }
size_t pinned_bytes(const ssw_lknn *h) { return pinned_list_scores(h) + LK_MAX_LIST * 8; }

// the state pass and the merge levels: afterwards numer / denom hold the step's operands and list_ids / list_scores the
// L best unseen nodes, best first.  L <= the number of unseen nodes (the callers check).  Enqueue only.
ssw_status enqueue_select(ssw_lknn *h, int L) {
    hipStream_t s = h->stream;
    hipLaunchKernelGGL(k_lknn_select, dim3((unsigned)h->n_slices), dim3(LK_THREADS), 0, s, h->n, L, h->numerators, h->denominators,
                       h->gamma, h->seen, h->numer, h->denom, h->keys_a, h->ids_a);
    ++h->info[0];
    int lists = h->n_slices;
    bool from_a = true;
    do {
        const int out = (lists + LK_FAN - 1) / LK_FAN;
        const bool last = out == 1;
        hipLaunchKernelGGL(k_lknn_merge, dim3((unsigned)out), dim3(LK_THREADS), 0, s, lists, L, from_a ? h->keys_a : h->keys_b,
                           from_a ? h->ids_a : h->ids_b, from_a ? h->keys_b : h->keys_a, from_a ? h->ids_b : h->ids_a,
                           last ? h->list_ids : (int32_t *)nullptr, h->list_scores, h->numer, h->denom);
        ++h->info[0];
        lists = out;
        from_a = !from_a;
    } while (lists > 1);
    SSW_HIP_TRY(hipGetLastError());
    return SSW_OK;
}

ssw_status copy_down(ssw_lknn *h, void *dst, const void *src, size_t bytes) {
    SSW_HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, h->stream));
    h->info[3] += (int64_t)bytes;
    return SSW_OK;
}

ssw_status wait(ssw_lknn *h) {
    SSW_HIP_TRY(hipStreamSynchronize(h->stream));
    ++h->info[1];
    return SSW_OK;
}

// what a step refuses for this handle, decided on the host (ssw_lknn_step and a slot of ssw_lknn_step_batch alike)
ssw_status check_step(const ssw_lknn *h, int32_t K, int32_t lookahead) {
    SSW_REQUIRE(lookahead == 1 || lookahead == 2, "lknn: lookahead=%d (1 or 2)", lookahead);
    const int64_t unseen = h->n - h->n_seen;
    const int L = K + h->D;
    if (lookahead == 2) {
        SSW_REQUIRE(K >= 1 && K <= 128, "lknn: K=%d outside [1, 128] (the row sum follows numpy's order for one 128-element block)", K);
        SSW_REQUIRE(L <= LK_MAX_LIST, "lknn: K + D = %d exceeds %d", L, LK_MAX_LIST);
        SSW_REQUIRE(L <= unseen, "lknn: K + D = %d exceeds the %lld unseen nodes", L, (long long)unseen);
    } else {
        SSW_REQUIRE(unseen >= 1, "lknn: no unseen node is left");
    }
    return SSW_OK;
}

ssw_status check_top_remaining(int32_t k) {
    SSW_REQUIRE(k >= 1 && k <= LK_MAX_LIST, "lknn: top_remaining k=%d outside [1, %d]", k, LK_MAX_LIST);
    return SSW_OK;
}

}  // namespace

extern "C" {

ssw_status ssw_lknn_state_init(ssw_lknn *h, const double *gamma_host) {
    SSW_REQUIRE(h && gamma_host, "NULL argument");
    SSW_TRY(check_gamma(h, gamma_host));
    DeviceGuard guard(h->device);
    const int64_t n = h->n;
    if (!h->has_state) {
        h->n_slices = (int)((n + LK_SLICE - 1) / LK_SLICE);
        const size_t lists_b = (size_t)(h->n_slices + LK_FAN - 1) / LK_FAN;
        bool ok = hipMalloc((void **)&h->numerators, (size_t)n * 8) == hipSuccess &&
                  hipMalloc((void **)&h->denominators, (size_t)n * 8) == hipSuccess &&
                  hipMalloc((void **)&h->gamma, (size_t)n * 8) == hipSuccess &&
                  hipMalloc((void **)&h->seen, (size_t)n) == hipSuccess &&
                  hipMalloc((void **)&h->keys_a, (size_t)h->n_slices * LK_MAX_LIST * 8) == hipSuccess &&
                  hipMalloc((void **)&h->ids_a, (size_t)h->n_slices * LK_MAX_LIST * 4) == hipSuccess &&
                  hipMalloc((void **)&h->keys_b, lists_b * LK_MAX_LIST * 8) == hipSuccess &&
                  hipMalloc((void **)&h->ids_b, lists_b * LK_MAX_LIST * 4) == hipSuccess &&
                  hipMalloc((void **)&h->list_scores, LK_MAX_LIST * 8) == hipSuccess &&
                  hipMalloc((void **)&h->small_ids, LK_MAX_ANSWERS * 8) == hipSuccess &&
                  hipMalloc((void **)&h->small_out, LK_MAX_ANSWERS * 8) == hipSuccess &&
                  hipHostMalloc((void **)&h->pinned, pinned_bytes(h), hipHostMallocDefault) == hipSuccess;
        for (hipEvent_t &e : h->ev)
            if (ok && !e) ok = hipEventCreate(&e) == hipSuccess;
        if (!ok) {
            free_state(h);
            set_error("lknn: allocation of the resident state failed");
            return SSW_ERR_NOMEM;
        }
        h->has_state = true;
    }
    hipStream_t s = h->stream;
    SSW_HIP_TRY(hipMemsetAsync(h->numerators, 0, (size_t)n * 8, s));
    SSW_HIP_TRY(hipMemsetAsync(h->denominators, 0, (size_t)n * 8, s));
    SSW_HIP_TRY(hipMemsetAsync(h->seen, 0, (size_t)n, s));
    SSW_HIP_TRY(hipMemcpyAsync(h->gamma, gamma_host, (size_t)n * 8, hipMemcpyHostToDevice, s));
    SSW_HIP_TRY(hipStreamSynchronize(s));  // gamma_host is the caller's again
    h->seen_host.assign((size_t)n, 0);
    h->n_seen = 0;
    return SSW_OK;
}

ssw_status ssw_lknn_set_gamma(ssw_lknn *h, const double *gamma_host) {
    SSW_REQUIRE(h && gamma_host, "NULL argument");
    SSW_REQUIRE(h->has_state, "lknn: no resident state (ssw_lknn_state_init)");
    SSW_TRY(check_gamma(h, gamma_host));
    DeviceGuard guard(h->device);
    SSW_HIP_TRY(hipMemcpyAsync(h->gamma, gamma_host, (size_t)h->n * 8, hipMemcpyHostToDevice, h->stream));
    SSW_HIP_TRY(hipStreamSynchronize(h->stream));
    return SSW_OK;
}

ssw_status ssw_lknn_condition(ssw_lknn *h, const int64_t *ids, const int32_t *ys, int32_t m) {
    SSW_REQUIRE(h && (m == 0 || (ids && ys)), "NULL argument");
    SSW_REQUIRE(h->has_state, "lknn: no resident state (ssw_lknn_state_init)");
    SSW_REQUIRE(m >= 0 && m <= LK_MAX_ANSWERS, "lknn: %d answers in one call (at most %d)", m, LK_MAX_ANSWERS);
    if (m == 0) return SSW_OK;
    // every refusal comes before the first change: a node of this call carries the mark 2 until all have passed
    int bad = -1;
    const char *why = nullptr;
    for (int t = 0; t < m && bad < 0; ++t) {
        if (ids[t] < 0 || ids[t] >= h->n) bad = t, why = "is outside the graph";
        else if (ys[t] != 0 && ys[t] != 1) bad = t, why = "has a label that is neither 0 nor 1";
        else if (h->seen_host[(size_t)ids[t]] == 1) bad = t, why = "has been answered before";
        else if (h->seen_host[(size_t)ids[t]] == 2) bad = t, why = "is repeated in the call";
        else h->seen_host[(size_t)ids[t]] = 2;
    }
    for (int t = 0; t < (bad < 0 ? m : bad); ++t) h->seen_host[(size_t)ids[t]] = bad < 0 ? 1 : 0;
    SSW_REQUIRE(bad < 0, "lknn: answer %d (node %lld) %s", bad, (long long)ids[bad], why);
    h->n_seen += m;
    std::vector<int32_t> pairs((size_t)m * 2);
    for (int t = 0; t < m; ++t) pairs[2 * t] = (int32_t)ids[t], pairs[2 * t + 1] = ys[t];
    DeviceGuard guard(h->device);
    SSW_TRY(h->small_stage.push(h->small_ids, pairs.data(), pairs.size() * 4, h->stream));
    hipLaunchKernelGGL(k_lknn_condition, dim3(1), dim3(LK_MAX_D), 0, h->stream, (int)m, h->D, h->small_ids, h->nbr, h->numerators,
                       h->denominators, h->seen);
    SSW_HIP_TRY(hipGetLastError());
    return SSW_OK;
}

ssw_status ssw_lknn_step(ssw_lknn *h, int32_t K, int32_t lookahead, int64_t *out_best_idx, double *out_best_value,
                         double *out_values_or_null, int32_t *out_list_or_null) {
    SSW_REQUIRE(h, "NULL argument");
    SSW_REQUIRE(h->has_state, "lknn: no resident state (ssw_lknn_state_init)");
    SSW_TRY(check_step(h, K, lookahead));
    const int64_t n = h->n;
    const int L = K + h->D;
    DeviceGuard guard(h->device);
    hipStream_t s = h->stream;
    h->info[0] = h->info[1] = h->info[2] = h->info[3] = 0;
    h->timed = 0;
    const unsigned row_blocks = (unsigned)((n + LK_THREADS - 1) / LK_THREADS);
    if (lookahead == 2) {
        if (h->timing) SSW_HIP_TRY(hipEventRecord(h->ev[0], s));
        SSW_TRY(enqueue_select(h, L));
        if (h->timing) SSW_HIP_TRY(hipEventRecord(h->ev[1], s));
        hipLaunchKernelGGL(k_lknn_mark, dim3(1), dim3(LK_THREADS), 0, s, h->rank_in_list, h->list_ids, L);
        if (h->timing) SSW_HIP_TRY(hipEventRecord(h->ev[2], s));
        hipLaunchKernelGGL(k_lknn_top_sum, dim3(row_blocks), dim3(LK_THREADS), 0, s, n, h->D, (int)K, L, h->nbr, h->numer, h->denom,
                           h->list_ids, h->rank_in_list, h->value);
        if (h->timing) SSW_HIP_TRY(hipEventRecord(h->ev[3], s));
        hipLaunchKernelGGL(k_lknn_unmark, dim3(1), dim3(LK_THREADS), 0, s, h->rank_in_list, h->list_ids, L);
        h->info[0] += 3;
        h->timed = h->timing ? 3 : 0;
    } else {
        hipLaunchKernelGGL(k_lknn_score, dim3(row_blocks), dim3(LK_THREADS), 0, s, n, h->numerators, h->denominators, h->gamma,
                           h->seen, h->value);
        ++h->info[0];
    }
    hipLaunchKernelGGL(k_lknn_argmax, dim3(h->argmax_blocks), dim3(LK_THREADS), 0, s, h->value, n, h->blk_v, h->blk_i);
    ++h->info[0];
    SSW_HIP_TRY(hipGetLastError());
    const double *bv = (const double *)h->pinned;
    const long long *bi = (const long long *)(h->pinned + pinned_blk_i(h));
    SSW_TRY(copy_down(h, h->pinned, h->blk_v, (size_t)h->argmax_blocks * 8));
    SSW_TRY(copy_down(h, h->pinned + pinned_blk_i(h), h->blk_i, (size_t)h->argmax_blocks * 8));
    if (out_list_or_null && lookahead == 2) SSW_TRY(copy_down(h, h->pinned + pinned_list_ids(h), h->list_ids, (size_t)L * 4));
    if (out_values_or_null) SSW_TRY(copy_down(h, out_values_or_null, h->value, (size_t)n * 8));
    SSW_TRY(wait(h));
    if (out_list_or_null && lookahead == 2) memcpy(out_list_or_null, h->pinned + pinned_list_ids(h), (size_t)L * 4);
    long long best = -1;
    double bval = 0.0;
    for (int b = 0; b < h->argmax_blocks; ++b) {
        if (bi[b] < 0) continue;
        if (best < 0 || bv[b] > bval || (bv[b] == bval && bi[b] < best)) {
            best = bi[b];
            bval = bv[b];
        }
    }
    if (out_best_idx) *out_best_idx = best;
    if (out_best_value) *out_best_value = bval;
    return SSW_OK;
}

ssw_status ssw_lknn_top_remaining(ssw_lknn *h, int32_t k, int32_t *out_ids, double *out_scores, int32_t *out_count) {
    SSW_REQUIRE(h && out_ids && out_scores && out_count, "NULL argument");
    SSW_REQUIRE(h->has_state, "lknn: no resident state (ssw_lknn_state_init)");
    SSW_TRY(check_top_remaining(k));
    const int64_t unseen = h->n - h->n_seen;
    const int L = (int)std::min<int64_t>(k, unseen);
    h->info[0] = h->info[1] = h->info[2] = h->info[3] = 0;
    h->timed = 0;
    *out_count = L;
    if (L == 0) return SSW_OK;
    DeviceGuard guard(h->device);
    if (h->timing) SSW_HIP_TRY(hipEventRecord(h->ev[0], h->stream));
    SSW_TRY(enqueue_select(h, L));
    if (h->timing) SSW_HIP_TRY(hipEventRecord(h->ev[1], h->stream));
    h->timed = h->timing ? 1 : 0;
    SSW_TRY(copy_down(h, h->pinned + pinned_list_ids(h), h->list_ids, (size_t)L * 4));
    SSW_TRY(copy_down(h, h->pinned + pinned_list_scores(h), h->list_scores, (size_t)L * 8));
    SSW_TRY(wait(h));
    memcpy(out_ids, h->pinned + pinned_list_ids(h), (size_t)L * 4);
    memcpy(out_scores, h->pinned + pinned_list_scores(h), (size_t)L * 8);
    return SSW_OK;
}

ssw_status ssw_lknn_predict(ssw_lknn *h, const int64_t *ids, int32_t m, double *out_scores) {
    SSW_REQUIRE(h && (m == 0 || (ids && out_scores)), "NULL argument");
    SSW_REQUIRE(h->has_state, "lknn: no resident state (ssw_lknn_state_init)");
    SSW_REQUIRE(m >= 0 && m <= LK_MAX_ANSWERS, "lknn: %d nodes in one call (at most %d)", m, LK_MAX_ANSWERS);
    if (m == 0) return SSW_OK;
    std::vector<int32_t> ids32((size_t)m);
    for (int t = 0; t < m; ++t) {
        SSW_REQUIRE(ids[t] >= 0 && ids[t] < h->n, "lknn: node %lld is outside the graph", (long long)ids[t]);
        ids32[t] = (int32_t)ids[t];
    }
    DeviceGuard guard(h->device);
    SSW_TRY(h->small_stage.push(h->small_ids, ids32.data(), ids32.size() * 4, h->stream));
    hipLaunchKernelGGL(k_lknn_gather_score, dim3((unsigned)((m + LK_THREADS - 1) / LK_THREADS)), dim3(LK_THREADS), 0, h->stream, (int)m,
                       h->small_ids, h->numerators, h->denominators, h->gamma, h->small_out);
    SSW_HIP_TRY(hipGetLastError());
    SSW_HIP_TRY(hipMemcpyAsync(out_scores, h->small_out, (size_t)m * 8, hipMemcpyDeviceToHost, h->stream));
    SSW_HIP_TRY(hipStreamSynchronize(h->stream));
    return SSW_OK;
}

ssw_status ssw_lknn_state_fetch(ssw_lknn *h, double *numerators, double *denominators, double *gamma, uint8_t *seen_u8) {
    SSW_REQUIRE(h, "NULL argument");
    SSW_REQUIRE(h->has_state, "lknn: no resident state (ssw_lknn_state_init)");
    DeviceGuard guard(h->device);
    hipStream_t s = h->stream;
    const size_t n = (size_t)h->n;
    if (numerators) SSW_HIP_TRY(hipMemcpyAsync(numerators, h->numerators, n * 8, hipMemcpyDeviceToHost, s));
    if (denominators) SSW_HIP_TRY(hipMemcpyAsync(denominators, h->denominators, n * 8, hipMemcpyDeviceToHost, s));
    if (gamma) SSW_HIP_TRY(hipMemcpyAsync(gamma, h->gamma, n * 8, hipMemcpyDeviceToHost, s));
    if (seen_u8) SSW_HIP_TRY(hipMemcpyAsync(seen_u8, h->seen, n, hipMemcpyDeviceToHost, s));
    SSW_HIP_TRY(hipStreamSynchronize(s));
    return SSW_OK;
}

ssw_status ssw_lknn_step_info(ssw_lknn *h, int64_t *out4) {
    SSW_REQUIRE(h && out4, "NULL argument");
    for (int j = 0; j < 4; ++j) out4[j] = h->info[j];
    return SSW_OK;
}

ssw_status ssw_lknn_step_times(ssw_lknn *h, int32_t enable, double *out_ms2_or_null) {
    SSW_REQUIRE(h, "NULL argument");
    SSW_REQUIRE(h->has_state, "lknn: no resident state (ssw_lknn_state_init)");
    if (out_ms2_or_null) {
        out_ms2_or_null[0] = out_ms2_or_null[1] = -1.0;
        float ms = 0.f;
        if (h->timed & 1) {
            SSW_HIP_TRY(hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));
            out_ms2_or_null[0] = ms;
        }
        if (h->timed & 2) {
            SSW_HIP_TRY(hipEventElapsedTime(&ms, h->ev[2], h->ev[3]));
            out_ms2_or_null[1] = ms;
        }
    }
    h->timing = enable != 0;
    return SSW_OK;
}

}  // extern "C"

// ---- several handles' steps in one pass ---------------------------------------------------------------------------------
namespace {

constexpr int LK_MAX_BATCH = SSW_LKNN_MAX_BATCH;

// the whole-call refusals of both batched entries; nothing is read through a handle before every handle is known non-NULL
ssw_status check_batch(ssw_lknn *const *hs, int32_t n_slots, bool arrays) {
    SSW_REQUIRE(n_slots >= 1 && n_slots <= LK_MAX_BATCH, "lknn batch: n_slots=%d outside [1, %d]", n_slots, LK_MAX_BATCH);
    SSW_REQUIRE(hs != nullptr && arrays, "NULL argument");
    for (int j = 0; j < n_slots; ++j) SSW_REQUIRE(hs[j] != nullptr, "lknn batch: handle %d is NULL", j);
    for (int j = 0; j < n_slots; ++j) {
        for (int i = 0; i < j; ++i) SSW_REQUIRE(hs[i] != hs[j], "lknn batch: handle %d repeats handle %d", j, i);
        SSW_REQUIRE(hs[j]->has_state, "lknn batch: handle %d has no resident state (ssw_lknn_state_init)", j);
        SSW_REQUIRE(hs[j]->device == hs[0]->device && hs[j]->n == hs[0]->n && hs[j]->D == hs[0]->D,
                    "lknn batch: handle %d (device %d, n=%lld, D=%d) differs from handle 0 (device %d, n=%lld, D=%d)", j,
                    hs[j]->device, (long long)hs[j]->n, hs[j]->D, hs[0]->device, (long long)hs[0]->n, hs[0]->D);
    }
    return SSW_OK;
}

void refuse_slot(ssw_lknn *h, ssw_status rc, int32_t *out_status) {
    *out_status = rc;
    const char *msg = ssw_last_error();
    h->batch_error = msg ? msg : "";
}

LkSlot describe(ssw_lknn *h, int slot, int K, int L, int want_list) {
    LkSlot d;
    d.numerators = h->numerators, d.denominators = h->denominators, d.gamma = h->gamma, d.seen = h->seen, d.nbr = h->nbr;
    d.numer = h->numer, d.denom = h->denom, d.value = h->value;
    d.rank_in_list = h->rank_in_list, d.list_ids = h->list_ids, d.list_scores = h->list_scores;
    d.keys_a = h->keys_a, d.keys_b = h->keys_b, d.ids_a = h->ids_a, d.ids_b = h->ids_b;
    d.blk_v = h->blk_v, d.blk_i = h->blk_i;
    d.K = K, d.L = L, d.slot = slot, d.want_list = want_list;
    return d;
}

// the first handle's table and result block for n_slots slots; the table goes up; the pass waits for every other
// handle's stream (answers enqueued there must be seen)
ssw_status begin_pass(ssw_lknn *const *hs, int32_t n_slots, const std::vector<LkSlot> &tab) {
    ssw_lknn *h0 = hs[0];
    if (n_slots > h0->batch_cap) {  // nothing of an earlier pass is in flight: every pass ends with a wait
        (void)hipFree(h0->batch_tab);
        (void)hipFree(h0->batch_res);
        if (h0->batch_pinned) (void)hipHostFree(h0->batch_pinned);
        h0->batch_tab = nullptr, h0->batch_res = nullptr, h0->batch_pinned = nullptr, h0->batch_cap = 0;
        int cap = 16;
        while (cap < n_slots) cap <<= 1;
        SSW_HIP_TRY(hipMalloc((void **)&h0->batch_tab, (size_t)cap * sizeof(LkSlot)));
        SSW_HIP_TRY(hipMalloc((void **)&h0->batch_res, lk_res_bytes(cap)));
        SSW_HIP_TRY(hipHostMalloc((void **)&h0->batch_pinned, lk_res_bytes(cap), hipHostMallocDefault));
        h0->batch_cap = cap;
    }
    for (int j = 1; j < n_slots; ++j) {
        if (!hs[j]->batch_ev) SSW_HIP_TRY(hipEventCreateWithFlags(&hs[j]->batch_ev, hipEventDisableTiming));
        SSW_HIP_TRY(hipEventRecord(hs[j]->batch_ev, hs[j]->stream));
        SSW_HIP_TRY(hipStreamWaitEvent(h0->stream, hs[j]->batch_ev, 0));
    }
    h0->info[0] = h0->info[1] = h0->info[2] = h0->info[3] = 0;
    h0->timed = 0;
    SSW_TRY(h0->batch_stage.push(h0->batch_tab, tab.data(), tab.size() * sizeof(LkSlot), h0->stream));
    h0->info[2] += (int64_t)(tab.size() * sizeof(LkSlot));
    return SSW_OK;
}

// the state pass and the merge levels of the table's first n2 slots (enqueue_select, slot on blockIdx.y)
ssw_status enqueue_select_batch(ssw_lknn *h0, int n2) {
    hipStream_t s = h0->stream;
    hipLaunchKernelGGL(k_lknn_select_batch, dim3((unsigned)h0->n_slices, (unsigned)n2), dim3(LK_THREADS), 0, s, h0->batch_tab, h0->n);
    ++h0->info[0];
    int lists = h0->n_slices;
    bool from_a = true;
    do {
        const int out = (lists + LK_FAN - 1) / LK_FAN;
        hipLaunchKernelGGL(k_lknn_merge_batch, dim3((unsigned)out, (unsigned)n2), dim3(LK_THREADS), 0, s, h0->batch_tab, lists,
                           from_a ? 1 : 0, out == 1 ? 1 : 0);
        ++h0->info[0];
        lists = out;
        from_a = !from_a;
    } while (lists > 1);
    SSW_HIP_TRY(hipGetLastError());
    return SSW_OK;
}

}  // namespace

extern "C" {

ssw_status ssw_lknn_step_batch(ssw_lknn *const *hs, int32_t n_slots, const int32_t *K, const int32_t *lookahead,
                               int64_t *out_best_idx, double *out_best_value, double *const *out_values_or_null,
                               int32_t *out_lists_or_null, int32_t *out_status, int64_t *out_stats4_or_null) {
    SSW_TRY(check_batch(hs, n_slots, K && lookahead && out_best_idx && out_best_value && out_status));
    ssw_lknn *h0 = hs[0];
    const int64_t n = h0->n;
    // per slot, on the host: refused, or a descriptor -- the lookahead-2 slots first
    std::vector<LkSlot> tab, ones;
    for (int j = 0; j < n_slots; ++j) {
        hs[j]->batch_error.clear();
        out_status[j] = SSW_OK;
        out_best_idx[j] = -1, out_best_value[j] = 0.0;
        const ssw_status rc = check_step(hs[j], K[j], lookahead[j]);
        if (rc != SSW_OK) {
            refuse_slot(hs[j], rc, &out_status[j]);
            continue;
        }
        if (lookahead[j] == 2) tab.push_back(describe(hs[j], j, K[j], K[j] + hs[j]->D, out_lists_or_null ? 1 : 0));
        else ones.push_back(describe(hs[j], j, K[j], 0, 0));
    }
    const int n2 = (int)tab.size(), n1 = (int)ones.size(), active = n2 + n1;
    tab.insert(tab.end(), ones.begin(), ones.end());
    if (out_stats4_or_null) out_stats4_or_null[0] = out_stats4_or_null[1] = out_stats4_or_null[2] = out_stats4_or_null[3] = 0;
    if (active == 0) return SSW_OK;
    DeviceGuard guard(h0->device);
    SSW_TRY(begin_pass(hs, n_slots, tab));
    hipStream_t s = h0->stream;
    const unsigned row_blocks = (unsigned)((n + LK_THREADS - 1) / LK_THREADS);
    if (n2) {
        if (h0->timing) SSW_HIP_TRY(hipEventRecord(h0->ev[0], s));
        SSW_TRY(enqueue_select_batch(h0, n2));
        if (h0->timing) SSW_HIP_TRY(hipEventRecord(h0->ev[1], s));
        hipLaunchKernelGGL(k_lknn_mark_batch, dim3(1, (unsigned)n2), dim3(LK_THREADS), 0, s, h0->batch_tab);
        if (h0->timing) SSW_HIP_TRY(hipEventRecord(h0->ev[2], s));
        hipLaunchKernelGGL(k_lknn_top_sum_batch, dim3(row_blocks, (unsigned)n2), dim3(LK_THREADS), 0, s, h0->batch_tab, n, h0->D);
        if (h0->timing) SSW_HIP_TRY(hipEventRecord(h0->ev[3], s));
        hipLaunchKernelGGL(k_lknn_unmark_batch, dim3(1, (unsigned)n2), dim3(LK_THREADS), 0, s, h0->batch_tab);
        h0->info[0] += 3;
        h0->timed = h0->timing ? 3 : 0;
    }
    if (n1) {
        hipLaunchKernelGGL(k_lknn_score_batch, dim3(row_blocks, (unsigned)n1), dim3(LK_THREADS), 0, s, h0->batch_tab + n2, n);
        ++h0->info[0];
    }
    hipLaunchKernelGGL(k_lknn_argmax_batch, dim3((unsigned)h0->argmax_blocks, (unsigned)active), dim3(LK_THREADS), 0, s, h0->batch_tab, n);
    hipLaunchKernelGGL(k_lknn_finish_batch, dim3(1, (unsigned)active), dim3(LK_THREADS), 0, s, h0->batch_tab, h0->argmax_blocks,
                       h0->batch_res, h0->batch_cap);
    h0->info[0] += 2;
    SSW_HIP_TRY(hipGetLastError());
    const int cap = h0->batch_cap;
    SSW_TRY(copy_down(h0, h0->batch_pinned, h0->batch_res, (size_t)n_slots * sizeof(LkBest)));
    if (out_lists_or_null && n2)
        SSW_TRY(copy_down(h0, h0->batch_pinned + lk_res_ids(cap), h0->batch_res + lk_res_ids(cap), (size_t)n_slots * LK_MAX_LIST * 4));
    if (out_values_or_null)
        for (const LkSlot &d : tab)
            if (out_values_or_null[d.slot]) SSW_TRY(copy_down(h0, out_values_or_null[d.slot], d.value, (size_t)n * 8));
    SSW_TRY(wait(h0));
    const LkBest *best = (const LkBest *)h0->batch_pinned;
    const int32_t *lists = (const int32_t *)(h0->batch_pinned + lk_res_ids(cap));
    for (const LkSlot &d : tab) {
        out_best_idx[d.slot] = best[d.slot].index;
        out_best_value[d.slot] = best[d.slot].value;
        if (out_lists_or_null && d.L) memcpy(out_lists_or_null + (size_t)d.slot * LK_MAX_LIST, lists + (size_t)d.slot * LK_MAX_LIST, (size_t)d.L * 4);
        ssw_lknn *h = hs[d.slot];
        if (h != h0) {
            for (int q = 0; q < 4; ++q) h->info[q] = h0->info[q];
            h->timed = 0;
        }
    }
    if (out_stats4_or_null)
        for (int q = 0; q < 4; ++q) out_stats4_or_null[q] = h0->info[q];
    return SSW_OK;
}

ssw_status ssw_lknn_top_remaining_batch(ssw_lknn *const *hs, int32_t n_slots, const int32_t *k, int32_t *out_ids,
                                        double *out_scores, int32_t *out_counts, int32_t *out_status) {
    SSW_TRY(check_batch(hs, n_slots, k && out_ids && out_scores && out_counts && out_status));
    ssw_lknn *h0 = hs[0];
    std::vector<LkSlot> tab;
    for (int j = 0; j < n_slots; ++j) {
        hs[j]->batch_error.clear();
        out_status[j] = SSW_OK;
        out_counts[j] = 0;
        const ssw_status rc = check_top_remaining(k[j]);
        if (rc != SSW_OK) {
            refuse_slot(hs[j], rc, &out_status[j]);
            continue;
        }
        const int L = (int)std::min<int64_t>(k[j], hs[j]->n - hs[j]->n_seen);
        out_counts[j] = L;
        if (L == 0) {  // as the single call: nothing to do, and that is what its info says
            hs[j]->info[0] = hs[j]->info[1] = hs[j]->info[2] = hs[j]->info[3] = 0;
            hs[j]->timed = 0;
            continue;
        }
        tab.push_back(describe(hs[j], j, 0, L, 2));
    }
    const int active = (int)tab.size();
    if (active == 0) return SSW_OK;
    DeviceGuard guard(h0->device);
    SSW_TRY(begin_pass(hs, n_slots, tab));
    hipStream_t s = h0->stream;
    if (h0->timing) SSW_HIP_TRY(hipEventRecord(h0->ev[0], s));
    SSW_TRY(enqueue_select_batch(h0, active));
    if (h0->timing) SSW_HIP_TRY(hipEventRecord(h0->ev[1], s));
    h0->timed = h0->timing ? 1 : 0;
    hipLaunchKernelGGL(k_lknn_collect_batch, dim3(1, (unsigned)active), dim3(LK_THREADS), 0, s, h0->batch_tab, h0->batch_res, h0->batch_cap);
    ++h0->info[0];
    SSW_HIP_TRY(hipGetLastError());
    const int cap = h0->batch_cap;
    SSW_TRY(copy_down(h0, h0->batch_pinned + lk_res_ids(cap), h0->batch_res + lk_res_ids(cap), (size_t)n_slots * LK_MAX_LIST * 4));
    SSW_TRY(copy_down(h0, h0->batch_pinned + lk_res_scores(cap), h0->batch_res + lk_res_scores(cap), (size_t)n_slots * LK_MAX_LIST * 8));
    SSW_TRY(wait(h0));
    const int32_t *ids = (const int32_t *)(h0->batch_pinned + lk_res_ids(cap));
    const double *scores = (const double *)(h0->batch_pinned + lk_res_scores(cap));
    for (const LkSlot &d : tab) {
        memcpy(out_ids + (size_t)d.slot * LK_MAX_LIST, ids + (size_t)d.slot * LK_MAX_LIST, (size_t)d.L * 4);
        memcpy(out_scores + (size_t)d.slot * LK_MAX_LIST, scores + (size_t)d.slot * LK_MAX_LIST, (size_t)d.L * 8);
        ssw_lknn *h = hs[d.slot];
        if (h != h0) {
            for (int q = 0; q < 4; ++q) h->info[q] = h0->info[q];
            h->timed = 0;
        }
    }
    return SSW_OK;
}

const char *ssw_lknn_batch_error(const ssw_lknn *h) { return h ? h->batch_error.c_str() : ""; }

}  // extern "C"

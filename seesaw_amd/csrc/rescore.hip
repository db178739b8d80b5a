// rescore.hip -- second stage of the multiscale lookup: the `avg_score` aggregation of the candidate
// images' tile scores (gfx950 / MI355X).
//
// Replaces score_frame2 + box_join as rescore_candidates drives them
// (seesaw/indices/multiscale/multiscale_index.py:112-150, 379-403; seesaw/box_utils.py:336-372):
//   for every candidate image, all tile pairs (i, j) with IoU > 0 are joined, filtered by aug_larger
//   ('all' | 'greater': zoom_j >= zoom_i | 'adjacent': zoom_j == zoom_i), and tile i's score becomes the mean,
//   over the zoom levels z present among its partners, of the score of the level-z partner overlapping it most
//   (pandas idxmax: the first maximum).  The image is represented by its first tile with the highest
//   aggregated score.
// The reference does this with a pandas self-join + two groupbys per image (milliseconds per image, ~50
// images per query).  Here: one workgroup per candidate image, boxes / zoom levels / scores of its tiles in
// LDS, one thread per tile i walking the T partners once per zoom level.  Latency-bound (T ~ 13 .. 60 tiles,
// a few hundred IoUs per tile); what it removes is the host loop and the PCIe round trip of the tile scores:
// the scores are read from the buffer the scan left in HBM.
//
// Arithmetic is the reference's, op for op, so results are bit-identical to it given identical tile scores:
//   IoU in f32 exactly as torchvision's _box_inter_union forms it on float32 boxes
//     (area = (x2-x1)*(y2-y1); wh = max(min(rb) - max(lt), 0); inter = w*h; union = (a_i + a_j) - inter),
//   the mean as pandas' float32 group_mean: Kahan-compensated f32 sum in ascending zoom level, f32 division; a NaN
//   score is skipped (and its level not counted), the compensation restarts at 0 after an infinite score.
// aug_weight = 'cont_weighted' (bit 2 of `aug`): softmax-of-containment weights over all partners instead (f32 like
// scipy.special.softmax on float32 input; the weighted sum runs in partner order, numpy's dot in BLAS order: 1e-6).
// Explicitly rounded intrinsics keep the compiler from contracting w*h into the union's subtraction.
#include "rescore_rows.h"

// Compiled with -ffp-contract=off (csrc/Makefile): results of this file are compared bit for bit with numpy /
// scipy / torch, so every product and sum must round on its own (hipcc would contract a * b + c into an fma).
// The row scoring k_avg_score_owner takes from rescore_rows.h asks for its fmas explicitly, so the flag leaves it alone.

namespace ssw {
namespace {

constexpr int RS_THREADS = 256;

__device__ __forceinline__ float iou_f32(const float4 a, float area_a, const float4 b, float area_b) {
    const float w = fmaxf(__fsub_rn(fminf(a.z, b.z), fmaxf(a.x, b.x)), 0.f);
    const float h = fmaxf(__fsub_rn(fminf(a.w, b.w), fmaxf(a.y, b.y)), 0.f);
    const float inter = __fmul_rn(w, h);
    const float uni = __fsub_rn(__fadd_rn(area_a, area_b), inter);
    return __fdiv_rn(inter, uni);
}

// The LDS of ONE image's aggregation: boxes, scores, aggregated scores, areas and zoom levels of its T tiles, and the
// mask of the zoom levels present.  avg_score_lds_bytes sizes the dynamic part.
template <typename ST>
struct AvgLds {
    float4 *sbox;     // [T]
    ST *sscore;       // [T]  (8-byte types first: the base is 16-byte aligned)
    ST *sagg;         // [T]
    float *sarea;     // [T]
    int *szoom;       // [T]
    unsigned *levels;
};

template <typename ST>
__device__ __forceinline__ AvgLds<ST> avg_lds(const int T) {
    extern __shared__ float4 sh4[];
    __shared__ unsigned level_mask;
    AvgLds<ST> l;
    l.sbox = sh4;
    l.sscore = reinterpret_cast<ST *>(l.sbox + T);
    l.sagg = l.sscore + T;
    l.sarea = reinterpret_cast<float *>(l.sagg + T);
    l.szoom = reinterpret_cast<int *>(l.sarea + T);
    l.levels = &level_mask;
    return l;
}

// First half, "fill LDS": the boxes, areas and zoom levels of the image's tiles (rows [r0, r0 + T)) and the level mask;
// with SCORES also tile i's score, scores[r0 + i] minus minus_or_null[i] (optional, one per tile of this image).  A kernel
// that computes the scores itself (k_avg_score_owner) stores them into sscore before it calls the second half.
template <typename ST, bool SCORES>
__device__ __forceinline__ void avg_score_fill(const AvgLds<ST> &l, const float4 *__restrict__ boxes,
                                               const int32_t *__restrict__ zoom, const ST *__restrict__ scores,
                                               const ST *__restrict__ minus_or_null, const int64_t r0, const int T) {
    if (threadIdx.x == 0) *l.levels = 0u;
    __syncthreads();
    for (int i = threadIdx.x; i < T; i += RS_THREADS) {
        const float4 b = boxes[r0 + i];
        l.sbox[i] = b;
        l.sarea[i] = __fmul_rn(__fsub_rn(b.z, b.x), __fsub_rn(b.w, b.y));
        if constexpr (SCORES) {
            ST s = scores[r0 + i];
            if (minus_or_null) s = s - minus_or_null[i];
            l.sscore[i] = s;
        }
        const int z = zoom[r0 + i];
        l.szoom[i] = z;
        atomicOr(l.levels, 1u << z);
    }
}

// Second half, "aggregate from LDS": the aggregation of ONE image by one workgroup over what the first half (and the
// scores' writer) left in LDS -- it opens with the barrier that makes them visible.  Thread 0 ends with
// out(aggregated score or NaN, the image's first tile with that score).  Every entry kernel below runs it, so the
// arithmetic exists once.
// ST = the dtype of the score column: float for the scan's scores (pandas' float32 group mean), double for the graph
// loops, which hand rescore_candidates the label-propagation output as float64 (graph_based.py:100-108; pandas' float64
// group mean is the same Kahan sum in f64).  IoUs are f32 either way (the boxes are).
template <typename ST, class Out>
__device__ __forceinline__ void avg_score_from_lds(const AvgLds<ST> &l, const int T, int aug, Out out) {
    const float4 *sbox = l.sbox;
    const ST *sscore = l.sscore;
    ST *sagg = l.sagg;
    const float *sarea = l.sarea;
    const int *szoom = l.szoom;
    __syncthreads();
    const unsigned levels = *l.levels;
    const bool cont_weighted = (aug & 4) != 0;
    aug &= 3;
    for (int i = threadIdx.x; i < T && cont_weighted; i += RS_THREADS) {
        // aug_weight = 'cont_weighted' (multiscale_index.py:133-145): over ALL joined partners j (IoU > 0, level
        // filter), weights = softmax(containment_ij), containment = inter / area_i (box_utils.py:347-349, f32);
        // score_i = weights . score_j.  scipy.special.softmax: exp(x - max) / sum(exp(x - max)), f32 on f32 input.
        const float4 bi = sbox[i];
        const float ai = sarea[i];
        const int zi = szoom[i];
        float cmax = -1.f;
        for (int j = 0; j < T; ++j) {
            const int z = szoom[j];
            if ((aug == 1 && z < zi) || (aug == 2 && z != zi)) continue;
            const float4 bj = sbox[j];
            const float w = fmaxf(__fsub_rn(fminf(bi.z, bj.z), fmaxf(bi.x, bj.x)), 0.f);
            const float h = fmaxf(__fsub_rn(fminf(bi.w, bj.w), fmaxf(bi.y, bj.y)), 0.f);
            const float inter = __fmul_rn(w, h);
            const float v = __fdiv_rn(inter, __fsub_rn(__fadd_rn(ai, sarea[j]), inter));
            if (!(v > 0.f)) continue;
            cmax = fmaxf(cmax, __fdiv_rn(inter, ai));
        }
        if (cmax < 0.f) {  // no partner at all (not even itself: a degenerate box)
            sagg[i] = (ST)__builtin_nanf("");
            continue;
        }
        float esum = 0.f;
        for (int pass = 0; pass < 2; ++pass) {
            ST acc = 0;
            for (int j = 0; j < T; ++j) {
                const int z = szoom[j];
                if ((aug == 1 && z < zi) || (aug == 2 && z != zi)) continue;
                const float4 bj = sbox[j];
                const float w = fmaxf(__fsub_rn(fminf(bi.z, bj.z), fmaxf(bi.x, bj.x)), 0.f);
                const float h = fmaxf(__fsub_rn(fminf(bi.w, bj.w), fmaxf(bi.y, bj.y)), 0.f);
                const float inter = __fmul_rn(w, h);
                const float v = __fdiv_rn(inter, __fsub_rn(__fadd_rn(ai, sarea[j]), inter));
                if (!(v > 0.f)) continue;
                const float e = expf(__fsub_rn(__fdiv_rn(inter, ai), cmax));
                if (pass == 0)
                    esum = __fadd_rn(esum, e);
                else
                    acc = acc + (ST)__fdiv_rn(e, esum) * sscore[j];
            }
            if (pass == 1) sagg[i] = acc;
        }
    }
    for (int i = threadIdx.x; i < T && !cont_weighted; i += RS_THREADS) {
        const float4 bi = sbox[i];
        const float ai = sarea[i];
        const int zi = szoom[i];
        ST sum = 0, comp = 0;  // Kahan pair
        int groups = 0;
        for (unsigned m = levels; m != 0u; m &= m - 1u) {
            const int z = __ffs(m) - 1;  // ascending zoom level
            if (aug == 1 && z < zi) continue;
            if (aug == 2 && z != zi) continue;
            float best = 0.f;  // only IoU > 0 joins
            int bj = -1;
            for (int j = 0; j < T; ++j) {
                if (szoom[j] != z) continue;
                const float v = iou_f32(bi, ai, sbox[j], sarea[j]);
                if (v > best) {  // strict: the first maximum wins, NaN never does
                    best = v;
                    bj = j;
                }
            }
            const ST x = bj >= 0 ? sscore[bj] : (ST)__builtin_nanf("");
            if (x == x) {  // pandas' group mean skips a NaN score (and so does not count its level)
                const ST y = x - comp;  // (this file is compiled without fma contraction)
                const ST t = sum + y;
                comp = (t - sum) - y;
                if (comp != comp) comp = 0;  // an infinite score: pandas restarts the compensation, the sum stays infinite
                sum = t;
                ++groups;
            }
        }
        sagg[i] = groups > 0 ? sum / (ST)groups : (ST)__builtin_nanf("");
    }
    __syncthreads();
    if (threadIdx.x == 0) {  // first tile with the highest aggregated score (NaN skipped, as pandas' max does)
        int bi = -1;
        ST bv = 0;
        for (int i = 0; i < T; ++i) {
            const ST v = sagg[i];
            if (v != v) continue;
            if (bi < 0 || v > bv) {
                bv = v;
                bi = i;
            }
        }
        out(bi >= 0 ? bv : (ST)__builtin_nanf(""), bi >= 0 ? bi : 0);
    }
}

// both halves over a score column: writes out_score[c] / out_row[c]
template <typename ST>
__device__ __forceinline__ void avg_score_of_image(const float4 *__restrict__ boxes, const int32_t *__restrict__ zoom,
                                                   const ST *__restrict__ scores, const ST *__restrict__ minus_or_null,
                                                   const int64_t r0, const int T, int aug, const int c,
                                                   ST *__restrict__ out_score, int64_t *__restrict__ out_row) {
    const AvgLds<ST> l = avg_lds<ST>(T);
    avg_score_fill<ST, true>(l, boxes, zoom, scores, minus_or_null, r0, T);
    avg_score_from_lds<ST>(l, T, aug, [&](ST score, int tile) {
        out_score[c] = score;
        out_row[c] = r0 + tile;
    });
}

// boxes: x1, y1, x2, y2 per row.  cand_pos[c] = image position; its rows are [row_start[p], row_start[p+1]).
// minus (optional) holds one value per candidate row, in candidate order (cand_off[c] = first), subtracted from
// the resident score (the vector2 form of MultiscaleIndex.query).
template <typename ST>
__global__ __launch_bounds__(RS_THREADS) void k_avg_score(const float4 *__restrict__ boxes,
                                                          const int32_t *__restrict__ zoom,
                                                          const ST *__restrict__ scores,
                                                          const ST *__restrict__ minus_or_null,
                                                          const int64_t *__restrict__ row_start,
                                                          const int64_t *__restrict__ cand_pos,
                                                          const int64_t *__restrict__ cand_off, int aug,
                                                          ST *__restrict__ out_score,
                                                          int64_t *__restrict__ out_row) {
    const int c = blockIdx.x;
    const int64_t p = cand_pos[c];
    const int64_t r0 = row_start[p];
    const int T = (int)(row_start[p + 1] - r0);
    avg_score_of_image<ST>(boxes, zoom, scores, minus_or_null ? minus_or_null + cand_off[c] : nullptr, r0, T, aug, c,
                           out_score, out_row);
}

// The candidates are the result slots of the selection that has just run on the stream (select.hip: keys [count] =
// (orderable(score) << 32) | (0xFFFFFFFF - image position), descending): one workgroup per slot, launched for k slots;
// a slot the selection did not fill writes nothing.  `scores` is the score slab the selection ranked -- of a batch,
// the slab of this query -- so no candidate list travels to the host and back between the two stages.
__global__ __launch_bounds__(RS_THREADS) void k_avg_score_keys(const float4 *__restrict__ boxes,
                                                               const int32_t *__restrict__ zoom,
                                                               const float *__restrict__ scores,
                                                               const int64_t *__restrict__ row_start, int64_t n_images,
                                                               const uint64_t *__restrict__ keys,
                                                               const int32_t *__restrict__ count, int aug,
                                                               float *__restrict__ out_score,
                                                               int64_t *__restrict__ out_row) {
    const int c = blockIdx.x;
    if (c >= count[0]) return;
    const int64_t p = (int64_t)(0xffffffffu - (uint32_t)(keys[c] & 0xffffffffull));
    if (p >= n_images) return;  // (never a key of this index: the LDS is sized for its images only)
    const int64_t r0 = row_start[p];
    const int T = (int)(row_start[p + 1] - r0);
    avg_score_of_image<float>(boxes, zoom, scores, nullptr, r0, T, aug, c, out_score, out_row);
}

// The second stage of a sharded batch on the rank that OWNS the image ("Sharded batch: second
// stage").  grid (k, nq): workgroup (c, b) takes merged key c of query b (keys [nq, k_max] / counts [nq] as the batched
// merge wrote them; the low word holds 0xFFFFFFFF - the GLOBAL image position).  This handle's images are the positions
// [image_offset, image_offset + n_images).  An image of another rank, or a slot past the count, stores two zero words and
// touches nothing else.  An owned one needs no score buffer: wave w scores tiles w, w + 4, ... straight from the index
// rows into sscore, two rows in flight -- the scan's bits (rescore_rows.h) -- and the aggregation above does the rest.
// out [nq, 2, k_max]: [b, 0, c] = 1 << 32 | the f32 bits of the aggregated score (the owned bit is apart because the
// score may be NaN), [b, 1, c] = row_offset + the best tile's row.
template <class R, int C>
__global__ __launch_bounds__(RS_THREADS) void k_avg_score_owner(
    const typename R::T *__restrict__ X, const float *__restrict__ qb, const float4 *__restrict__ boxes,
    const int32_t *__restrict__ zoom, const int64_t *__restrict__ row_start, int64_t n_images,
    const uint64_t *__restrict__ keys, const int32_t *__restrict__ counts, int k_max, int aug, int64_t image_offset,
    int64_t row_offset, unsigned long long *__restrict__ out) {
    const int c = blockIdx.x, b = blockIdx.y;
    unsigned long long *o = out + (size_t)b * 2 * k_max;
    int64_t p = -1;
    if (c < counts[b])
        p = (int64_t)(0xffffffffu - (uint32_t)(keys[(size_t)b * k_max + c] & 0xffffffffull)) - image_offset;
    if (p < 0 || p >= n_images) {  // not owned: before any row, box or row_start access
        if (threadIdx.x == 0) o[c] = o[k_max + c] = 0ull;
        return;
    }
    const int64_t r0 = row_start[p];
    const int T = (int)(row_start[p + 1] - r0);
    const AvgLds<float> l = avg_lds<float>(T);
    avg_score_fill<float, false>(l, boxes, zoom, nullptr, nullptr, r0, T);
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const rows::Frag<C> qf = rows::load_query<C>(qb + (size_t)b * (C * 256), lane);
    for (int i = w; i < T; i += 2 * (RS_THREADS / 64)) {
        const int i1 = i + RS_THREADS / 64;
        const bool two = i1 < T;
        const rows::Frag<C> x0 = R::template load<C>(X, r0 + i, lane);
        const rows::Frag<C> x1 = R::template load<C>(X, r0 + (two ? i1 : i), lane);
        const float v0 = rows::wave_sum(rows::lane_partial<C>(x0, qf));
        const float v1 = rows::wave_sum(rows::lane_partial<C>(x1, qf));
        if (lane == 0) {
            l.sscore[i] = v0;
            if (two) l.sscore[i1] = v1;
        }
    }
    avg_score_from_lds<float>(l, T, aug, [&](float score, int tile) {
        o[c] = (1ull << 32) | (unsigned long long)__float_as_uint(score);
        o[k_max + c] = (unsigned long long)(row_offset + r0 + tile);
    });
}

// The second stage of a batch of TWO-VECTOR queries (the `vector2` form of MultiscaleIndex.query; DESIGN.md section 4,
// "Batched two-vector query").  grid (k, nq): workgroup (c, b) takes candidate image pos[b * k + c] of query b; a slot
// at or past counts[b] writes nothing and touches no row, box or row_start.  Like the owner kernel it needs no score
// buffer: wave w scores tiles w, w + 4, ... straight from the index rows, two rows in flight, each row loaded ONCE for
// both fragments -- v the scan's bits for qb[b], v2 launch_score_rows' bits for q2b[b] -- and keeps d = v - v2, one f32
// subtraction (numpy's gather_scores(rows) - score_rows(vector2, rows)).
//   AVG:   d goes to sscore and the shared aggregation does the rest: launch_avg_score with the minus form on a handle
//          whose resident scores are qb[b]'s.
//   plain: the first tile attaining the maximum of the non-NaN d (np.lexsort((arange, -s, dbidx)) in
//          rescore_candidates' plain branch); an image whose every d is NaN gives its first row and that row's d.
//          No dynamic LDS, no box and no zoom level is read.
// out_score / out_row [nq, k].
template <class R, int C, bool AVG>
__global__ __launch_bounds__(RS_THREADS) void k_pair_score(
    const typename R::T *__restrict__ X, const float *__restrict__ qb, const float *__restrict__ q2b,
    const float4 *__restrict__ boxes, const int32_t *__restrict__ zoom, const int64_t *__restrict__ row_start,
    int64_t n_images, const int64_t *__restrict__ pos, const int32_t *__restrict__ counts, int k, int aug,
    float *__restrict__ out_score, int64_t *__restrict__ out_row) {
    constexpr int WAVES = RS_THREADS / 64;
    const int c = blockIdx.x, b = blockIdx.y;
    if (c >= counts[b]) return;
    const size_t slot = (size_t)b * k + c;
    const int64_t p = pos[slot];
    if (p < 0 || p >= n_images) return;  // (the host refused such a list: the LDS is sized for this index's images only)
    const int64_t r0 = row_start[p];
    const int T = (int)(row_start[p + 1] - r0);
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const rows::Frag<C> qf = rows::load_query<C>(qb + (size_t)b * (C * 256), lane);
    const rows::Frag<C> q2f = rows::load_query<C>(q2b + (size_t)b * (C * 256), lane);
    AvgLds<float> l = {};
    if constexpr (AVG) {
        l = avg_lds<float>(T);
        avg_score_fill<float, false>(l, boxes, zoom, nullptr, nullptr, r0, T);
    }
    // plain: this wave's first maximum among its tiles (ascending), every lane the same; wave 0 also keeps tile 0's d
    float bv = 0.f, d_first = 0.f;
    int bi = -1;
    for (int i = w; i < T; i += 2 * WAVES) {
        const int i1 = i + WAVES;
        const bool two = i1 < T;
        const rows::Frag<C> x0 = R::template load<C>(X, r0 + i, lane);
        const rows::Frag<C> x1 = R::template load<C>(X, r0 + (two ? i1 : i), lane);
        const float d0 = __fsub_rn(rows::wave_sum(rows::lane_partial<C>(x0, qf)), rows::wave_sum(rows::lane_partial<C>(x0, q2f)));
        const float d1 = __fsub_rn(rows::wave_sum(rows::lane_partial<C>(x1, qf)), rows::wave_sum(rows::lane_partial<C>(x1, q2f)));
        if constexpr (AVG) {
            if (lane == 0) {
                l.sscore[i] = d0;
                if (two) l.sscore[i1] = d1;
            }
        } else {
            if (i == 0) d_first = d0;
            if (d0 == d0 && (bi < 0 || d0 > bv)) bv = d0, bi = i;
            if (two && d1 == d1 && (bi < 0 || d1 > bv)) bv = d1, bi = i1;
        }
    }
    if constexpr (AVG) {
        avg_score_from_lds<float>(l, T, aug, [&](float score, int tile) {
            out_score[slot] = score;
            out_row[slot] = r0 + tile;
        });
    } else {
        __shared__ float wave_v[WAVES + 1];  // [WAVES]: tile 0's d
        __shared__ int wave_i[WAVES];
        if (lane == 0) {
            wave_v[w] = bv;
            wave_i[w] = bi;
            if (w == 0) wave_v[WAVES] = d_first;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            float v = 0.f;
            int t = -1;
            for (int j = 0; j < WAVES; ++j) {  // the highest d; among equals the lowest tile
                const int tj = wave_i[j];
                if (tj < 0) continue;
                const float vj = wave_v[j];
                if (t < 0 || vj > v || (vj == v && tj < t)) v = vj, t = tj;
            }
            out_score[slot] = t >= 0 ? v : wave_v[WAVES];
            out_row[slot] = r0 + (t >= 0 ? t : 0);
        }
    }
}

// The rows the aggregation above is about to read, as a list the gather scoring can take: candidate c's tiles at
// rows_out[cand_off[c] ..).  One workgroup a candidate.
__global__ __launch_bounds__(RS_THREADS) void k_candidate_tiles(const int64_t *__restrict__ row_start,
                                                                const int64_t *__restrict__ cand_pos,
                                                                const int64_t *__restrict__ cand_off,
                                                                int64_t *__restrict__ rows_out) {
    const int c = blockIdx.x;
    const int64_t p = cand_pos[c];
    const int64_t r0 = row_start[p];
    const int T = (int)(row_start[p + 1] - r0);
    int64_t *out = rows_out + cand_off[c];
    for (int i = threadIdx.x; i < T; i += RS_THREADS) out[i] = r0 + i;
}

// The same for the result slots k_avg_score_keys reads, decoded as there: slot c's tiles at rows_out[c * max_tiles ..),
// padded to max_tiles entries with the image's first row; a slot the selection did not fill (or a key of no image of
// this index) lists row 0 throughout.  Every entry is a row of the index, so the list can be scored as it stands.
__global__ __launch_bounds__(RS_THREADS) void k_candidate_tiles_keys(const int64_t *__restrict__ row_start,
                                                                     int64_t n_images,
                                                                     const uint64_t *__restrict__ keys,
                                                                     const int32_t *__restrict__ count, int max_tiles,
                                                                     int64_t *__restrict__ rows_out) {
    const int c = blockIdx.x;
    int64_t r0 = 0;
    int T = 0;
    if (c < count[0]) {
        const int64_t p = (int64_t)(0xffffffffu - (uint32_t)(keys[c] & 0xffffffffull));
        if (p < n_images) {
            r0 = row_start[p];
            T = (int)(row_start[p + 1] - r0);
        }
    }
    int64_t *out = rows_out + (int64_t)c * max_tiles;
    for (int i = threadIdx.x; i < max_tiles; i += RS_THREADS) out[i] = i < T ? r0 + i : r0;
}

}  // namespace

size_t avg_score_lds_bytes(int max_tiles, size_t score_bytes) {
    return (size_t)max_tiles * (sizeof(float4) + 2 * score_bytes + sizeof(float) + sizeof(int));
}

// the dynamic LDS of a launch of `kernel` for images of up to max_tiles tiles; the kernel's limit is raised when that and
// its static LDS (the 4-byte level mask) together exceed 64 KB: 2048 tiles of f32 scores are 65 536 + 4 bytes
static ssw_status avg_score_lds(const void *kernel, int32_t max_tiles, size_t score_bytes, size_t *out_lds) {
    if (max_tiles > SSW_RESCORE_MAX_TILES) {
        set_error("avg_score: an image with %d tiles exceeds the %d the kernel keeps in LDS", max_tiles,
                  SSW_RESCORE_MAX_TILES);
        return SSW_ERR_UNSUPPORTED;
    }
    *out_lds = avg_score_lds_bytes(max_tiles, score_bytes);
    if (*out_lds + sizeof(unsigned) > (size_t)64 * 1024) {  // 2048 tiles: 64 KB + 4 B (f32 scores), 80 KB + 4 B (f64)
        // per device and cheap: set on every such launch instead of caching a process-wide flag
        SSW_HIP_TRY(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024));
    }
    return SSW_OK;
}

template <typename ST>
static ssw_status launch_avg_score_t(const float *boxes, const int32_t *zoom, const ST *scores, const ST *minus_or_null,
                                     const int64_t *row_start, const int64_t *cand_pos, const int64_t *cand_off, int32_t m,
                                     int32_t max_tiles, int32_t aug, ST *out_score, int64_t *out_row, hipStream_t stream) {
    if (m <= 0) return SSW_OK;
    size_t lds = 0;
    SSW_TRY(avg_score_lds(reinterpret_cast<const void *>(k_avg_score<ST>), max_tiles, sizeof(ST), &lds));
    hipLaunchKernelGGL(k_avg_score<ST>, dim3((unsigned)m), dim3(RS_THREADS), lds, stream,
                       reinterpret_cast<const float4 *>(boxes), zoom, scores, minus_or_null, row_start, cand_pos,
                       cand_off, (int)aug, out_score, out_row);
    SSW_HIP_TRY(hipGetLastError());
    return SSW_OK;
}

ssw_status launch_avg_score_keys(const float *boxes, const int32_t *zoom, const float *scores, const int64_t *row_start,
                                 int64_t n_images, const uint64_t *keys, const int32_t *count, int32_t k,
                                 int32_t max_tiles, int32_t aug, float *out_score, int64_t *out_row, hipStream_t stream) {
    if (k <= 0) return SSW_OK;
    size_t lds = 0;
    SSW_TRY(avg_score_lds(reinterpret_cast<const void *>(k_avg_score_keys), max_tiles, sizeof(float), &lds));
    hipLaunchKernelGGL(k_avg_score_keys, dim3((unsigned)k), dim3(RS_THREADS), lds, stream,
                       reinterpret_cast<const float4 *>(boxes), zoom, scores, row_start, n_images, keys, count, (int)aug,
                       out_score, out_row);
    SSW_HIP_TRY(hipGetLastError());
    return SSW_OK;
}

template <class R, int C>
static ssw_status launch_avg_score_owner_t(const void *X, const AvgOwnerArgs &a, hipStream_t stream) {
    size_t lds = 0;
    SSW_TRY(avg_score_lds(reinterpret_cast<const void *>(k_avg_score_owner<R, C>), a.max_tiles, sizeof(float), &lds));
    hipLaunchKernelGGL((k_avg_score_owner<R, C>), dim3((unsigned)a.k, (unsigned)a.nq), dim3(RS_THREADS), lds, stream,
                       static_cast<const typename R::T *>(X), a.qb, reinterpret_cast<const float4 *>(a.boxes), a.zoom,
                       a.row_start, a.n_images, a.keys, a.counts, (int)a.k_max, (int)a.aug, a.image_offset, a.row_offset,
                       reinterpret_cast<unsigned long long *>(a.out));
    SSW_HIP_TRY(hipGetLastError());
    return SSW_OK;
}

ssw_status launch_avg_score_owner(const void *X, int32_t dtype, int32_t dim, const AvgOwnerArgs &a, hipStream_t stream) {
    if (a.nq <= 0 || a.k <= 0) return SSW_OK;
    const bool h16 = dtype == SSW_DTYPE_F16;
#define SSW_AVG_OWNER(C) \
    return h16 ? launch_avg_score_owner_t<rows::H16Rows, C>(X, a, stream) : launch_avg_score_owner_t<rows::F32Rows, C>(X, a, stream)
    switch (dim) {
        case 256: SSW_AVG_OWNER(1);
        case 512: SSW_AVG_OWNER(2);
        case 768: SSW_AVG_OWNER(3);
        case 1024: SSW_AVG_OWNER(4);
    }
#undef SSW_AVG_OWNER
    set_error("avg_score_owner: dim=%d unsupported", dim);
    return SSW_ERR_UNSUPPORTED;
}

template <class R, int C, bool AVG>
static ssw_status launch_pair_score_t(const void *X, const PairScoreArgs &a, hipStream_t stream) {
    size_t lds = 0;
    if constexpr (AVG)
        SSW_TRY(avg_score_lds(reinterpret_cast<const void *>(k_pair_score<R, C, true>), a.max_tiles, sizeof(float), &lds));
    hipLaunchKernelGGL((k_pair_score<R, C, AVG>), dim3((unsigned)a.k, (unsigned)a.nq), dim3(RS_THREADS), lds, stream,
                       static_cast<const typename R::T *>(X), a.qb, a.q2b, reinterpret_cast<const float4 *>(a.boxes), a.zoom,
                       a.row_start, a.n_images, a.pos, a.counts, (int)a.k, (int)a.aug, a.out_score, a.out_row);
    SSW_HIP_TRY(hipGetLastError());
    return SSW_OK;
}

ssw_status launch_pair_score(const void *X, int32_t dtype, int32_t dim, const PairScoreArgs &a, hipStream_t stream) {
    if (a.nq <= 0 || a.k <= 0) return SSW_OK;
    if (a.max_tiles > SSW_RESCORE_MAX_TILES) {  // both aggregations: the entry's one limit
        set_error("pair_score: an image with %d tiles exceeds the %d the kernel takes", a.max_tiles, SSW_RESCORE_MAX_TILES);
        return SSW_ERR_UNSUPPORTED;
    }
    const bool h16 = dtype == SSW_DTYPE_F16;
#define SSW_PAIR_SCORE(C)                                                                          \
    return h16 ? (a.avg ? launch_pair_score_t<rows::H16Rows, C, true>(X, a, stream)                \
                        : launch_pair_score_t<rows::H16Rows, C, false>(X, a, stream))              \
               : (a.avg ? launch_pair_score_t<rows::F32Rows, C, true>(X, a, stream)                \
                        : launch_pair_score_t<rows::F32Rows, C, false>(X, a, stream))
    switch (dim) {
        case 256: SSW_PAIR_SCORE(1);
        case 512: SSW_PAIR_SCORE(2);
        case 768: SSW_PAIR_SCORE(3);
        case 1024: SSW_PAIR_SCORE(4);
    }
#undef SSW_PAIR_SCORE
    set_error("pair_score: dim=%d unsupported", dim);
    return SSW_ERR_UNSUPPORTED;
}

ssw_status launch_candidate_tiles(const int64_t *row_start, const int64_t *cand_pos, const int64_t *cand_off, int32_t m,
                                  int64_t *rows_out, hipStream_t stream) {
    if (m <= 0) return SSW_OK;
    hipLaunchKernelGGL(k_candidate_tiles, dim3((unsigned)m), dim3(RS_THREADS), 0, stream, row_start, cand_pos, cand_off,
                       rows_out);
    SSW_HIP_TRY(hipGetLastError());
    return SSW_OK;
}

ssw_status launch_candidate_tiles_keys(const int64_t *row_start, int64_t n_images, const uint64_t *keys,
                                       const int32_t *count, int32_t k, int32_t max_tiles, int64_t *rows_out,
                                       hipStream_t stream) {
    if (k <= 0 || max_tiles <= 0) return SSW_OK;
    hipLaunchKernelGGL(k_candidate_tiles_keys, dim3((unsigned)k), dim3(RS_THREADS), 0, stream, row_start, n_images, keys,
                       count, (int)max_tiles, rows_out);
    SSW_HIP_TRY(hipGetLastError());
    return SSW_OK;
}

ssw_status launch_avg_score(const float *boxes, const int32_t *zoom, const float *scores, const float *minus_or_null,
                            const int64_t *row_start, const int64_t *cand_pos, const int64_t *cand_off, int32_t m,
                            int32_t max_tiles, int32_t aug, float *out_score, int64_t *out_row, hipStream_t stream) {
    return launch_avg_score_t<float>(boxes, zoom, scores, minus_or_null, row_start, cand_pos, cand_off, m, max_tiles, aug,
                                     out_score, out_row, stream);
}

ssw_status launch_avg_score_f64(const float *boxes, const int32_t *zoom, const double *scores,
                                const int64_t *row_start, const int64_t *cand_pos, const int64_t *cand_off, int32_t m,
                                int32_t max_tiles, int32_t aug, double *out_score, int64_t *out_row, hipStream_t stream) {
    return launch_avg_score_t<double>(boxes, zoom, scores, (const double *)nullptr, row_start, cand_pos, cand_off, m,
                                      max_tiles, aug, out_score, out_row, stream);
}

}  // namespace ssw

// Device-side tile pyramid: Pillow's 8-bit bilinear resample (the reference's `rescale`, multiscale_tools.py:10-14, run
// once per pyramid level, :16-49) as two launches per call -- one for the horizontal passes of every level of every
// image, one for the vertical passes -- driven by a job table, into levels the patch gather of clip.hip reads in place.
//
// The arithmetic is Pillow's (Resample.c: precompute_coeffs, normalize_coeffs_8bpc, ImagingResampleHorizontal_8bpc /
// Vertical_8bpc), integer from the coefficients on, so a level equals PIL.Image.resize(..., BILINEAR) byte for byte:
//   scale = in / out, fs = max(scale, 1), support = fs, ksize = 2 ceil(support) + 1
//   output x: center = (x + 0.5) scale, first = max(0, (int)(center - support + 0.5)),
//             n = min(in, (int)(center + support + 0.5)) - first
//   w_j = max(0, 1 - |(j + first - center + 0.5) / fs|) in double, divided by their sum; k_j = (int)(0.5 + w_j 2^22)
//   out = clip(0, 255, (2^21 + sum_j px_j k_j) >> 22) per channel; the sum stays below 2^31 (255 * (2^22 + ksize))
// The horizontal pass runs first (if the width changes) to uint8, the vertical pass (if the height changes) on its
// result.  Coefficients are made on the host, in double, once per distinct (in, out) pair of a call.
//
// Storage: RGB interleaved uint8; every level's base and row pitch are multiples of 8 bytes (the aligned gather's
// 8-byte loads); the horizontal pass's intermediate rows live in the same arena.
#include <algorithm>
#include <cmath>
#include <map>

#include "tiler.h"

namespace ssw {
namespace {

constexpr int PRECISION_BITS = 22;
constexpr int TILER_BLOCK = 256;  // output pixels (threads) a block

inline int64_t align8(int64_t v) { return (v + 7) & ~(int64_t)7; }

// One thread = one output pixel (three channels) of one job; a block finds its job by its first block.
__global__ __launch_bounds__(TILER_BLOCK) void tiler_resample(uint8_t *__restrict__ arena, const TilerJob *__restrict__ jobs,
                                                               int n_jobs, const int32_t *__restrict__ coefs) {
    int lo = 0, hi = n_jobs - 1;
    while (lo < hi) {  // the last job whose first block is <= this one
        const int mid = (lo + hi + 1) >> 1;
        if (jobs[mid].first_block <= (int)blockIdx.x) lo = mid;
        else hi = mid - 1;
    }
    const TilerJob j = jobs[lo];
    const int64_t p = (int64_t)((int)blockIdx.x - j.first_block) * TILER_BLOCK + threadIdx.x;
    if (p >= (int64_t)j.dst_w * j.dst_h) return;
    const int y = (int)(p / j.dst_w), x = (int)(p % j.dst_w);
    const uint8_t *src = arena + j.src;
    uint8_t *dst = arena + j.dst + (int64_t)y * j.dst_pitch + (int64_t)x * 3;
    if (j.kind == TILER_COPY) {
        const uint8_t *s = src + (int64_t)y * j.src_pitch + (int64_t)x * 3;
        dst[0] = s[0]; dst[1] = s[1]; dst[2] = s[2];
        return;
    }
    const bool horizontal = j.kind == TILER_HORIZONTAL;
    const int o = horizontal ? x : y;                        // the output index along the pass's axis
    const int n_out = horizontal ? j.dst_w : j.dst_h;
    const int32_t *bounds = coefs + j.coef + 2 * (int64_t)o;
    const int first = bounds[0], n = bounds[1];
    const int32_t *k = coefs + j.coef + 2 * (int64_t)n_out + (int64_t)o * j.ksize;
    const uint8_t *s = horizontal ? src + (int64_t)y * j.src_pitch + (int64_t)first * 3
                                  : src + (int64_t)first * j.src_pitch + (int64_t)x * 3;
    const int64_t step = horizontal ? 3 : j.src_pitch;
    int a0 = 1 << (PRECISION_BITS - 1), a1 = a0, a2 = a0;
    for (int t = 0; t < n; ++t) {
        const int w = k[t];
        a0 += (int)s[0] * w;
        a1 += (int)s[1] * w;
        a2 += (int)s[2] * w;
        s += step;
    }
    dst[0] = (uint8_t)min(max(a0 >> PRECISION_BITS, 0), 255);
    dst[1] = (uint8_t)min(max(a1 >> PRECISION_BITS, 0), 255);
    dst[2] = (uint8_t)min(max(a2 >> PRECISION_BITS, 0), 255);
}

// Pillow's precompute_coeffs + normalize_coeffs_8bpc for the bilinear filter, appended to `table` as [out][2] bounds and
// [out][ksize] weights.  Every (first, n) it writes satisfies 0 <= first, 0 <= n <= ksize, first + n <= in: the
// kernel's reads stay inside the source row / column.
void append_coefficients(int in, int out, std::vector<int32_t> &table, int *ksize_out) {
#pragma clang fp contract(off)
    const double scale = (double)in / (double)out;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = 1.0 * filterscale;
    const int ksize = (int)ceil(support) * 2 + 1;
    const double ss = 1.0 / filterscale;
    const size_t at = table.size();
    table.resize(at + (size_t)out * (2 + ksize), 0);
    int32_t *bounds = table.data() + at, *kk = bounds + 2 * (size_t)out;
    std::vector<double> k(ksize);
    for (int xx = 0; xx < out; ++xx) {
        const double center = 0.0 + (xx + 0.5) * scale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in) xmax = in;
        xmax -= xmin;
        if (xmax < 0) xmax = 0;
        if (xmax > ksize) xmax = ksize;
        double ww = 0.0;
        for (int x = 0; x < xmax; ++x) {
            double a = (x + xmin - center + 0.5) * ss;
            if (a < 0.0) a = -a;
            const double w = a < 1.0 ? 1.0 - a : 0.0;
            k[x] = w;
            ww += w;
        }
        for (int x = 0; x < xmax; ++x) {
            if (ww != 0.0) k[x] /= ww;
            kk[(size_t)xx * ksize + x] = (int32_t)(0.5 + k[x] * (double)(1 << PRECISION_BITS));  // bilinear: never negative
        }
        bounds[2 * xx] = xmin;
        bounds[2 * xx + 1] = xmax;
    }
    *ksize_out = ksize;
}

}  // namespace

ssw_status tiler_plan(int tile, int min_side, int32_t n_images, const int64_t *image_offsets, const int32_t *image_hw,
                      const int32_t *level_first, const int32_t *level_wh, TilerPlan *plan) {
    SSW_REQUIRE(n_images > 0 && image_offsets && image_hw && level_first && level_wh && plan, "multiscale: bad argument");
    SSW_REQUIRE(image_offsets[0] == 0 && level_first[0] == 0, "multiscale: image_offsets[0] = %lld and level_first[0] = %d must be 0",
                (long long)image_offsets[0], level_first[0]);
    for (int i = 0; i < n_images; ++i) {
        const int h = image_hw[2 * i], w = image_hw[2 * i + 1];
        SSW_REQUIRE(h >= 1 && h <= TILER_MAX_SIDE, "multiscale: image %d: source height %d outside [1, %d]", i, h, TILER_MAX_SIDE);
        SSW_REQUIRE(w >= 1 && w <= TILER_MAX_SIDE, "multiscale: image %d: source width %d outside [1, %d]", i, w, TILER_MAX_SIDE);
        const int64_t bytes = image_offsets[i + 1] - image_offsets[i];
        SSW_REQUIRE(bytes >= (int64_t)h * w * 3, "multiscale: image %d: %lld bytes between its offsets, %d x %d x 3 needs %lld", i,
                    (long long)bytes, h, w, (long long)h * w * 3);
        SSW_REQUIRE(level_first[i + 1] > level_first[i], "multiscale: image %d: level_first %d .. %d names no level", i,
                    level_first[i], level_first[i + 1]);
        for (int l = level_first[i]; l < level_first[i + 1]; ++l) {
            const int lw = level_wh[2 * l], lh = level_wh[2 * l + 1];
            SSW_REQUIRE(lw >= min_side && lh >= min_side, "multiscale: image %d: level %d is %d x %d, a side below the tile size %d",
                        i, l - level_first[i], lw, lh, min_side);
            SSW_REQUIRE(lw <= TILER_MAX_SIDE && lh <= TILER_MAX_SIDE, "multiscale: image %d: level %d is %d x %d, a side above %d", i,
                        l - level_first[i], lw, lh, TILER_MAX_SIDE);
        }
    }
    *plan = TilerPlan();
    plan->src_bytes = image_offsets[n_images];
    int64_t cursor = align8(plan->src_bytes);
    auto take = [&](int64_t bytes) {
        const int64_t at = cursor;
        cursor = align8(cursor + bytes);
        return at;
    };
    std::map<std::pair<int, int>, std::pair<int32_t, int32_t>> coef_of;  // (in, out) -> (offset, ksize)
    auto coefficients = [&](int in, int out, TilerJob &j) {
        auto it = coef_of.find({in, out});
        if (it == coef_of.end()) {
            int ksize = 0;
            const int32_t at = (int32_t)plan->coefs.size();
            append_coefficients(in, out, plan->coefs, &ksize);
            it = coef_of.emplace(std::make_pair(in, out), std::make_pair(at, (int32_t)ksize)).first;
        }
        j.coef = it->second.first;
        j.ksize = it->second.second;
    };
    auto add_job = [&](int launch, TilerJob j) {
        j.first_block = plan->blocks[launch];
        plan->blocks[launch] += (int32_t)(((int64_t)j.dst_w * j.dst_h + TILER_BLOCK - 1) / TILER_BLOCK);
        plan->jobs[launch].push_back(j);
    };
    const int64_t budget = TILER_ARENA_MAX_BYTES;
    // What the call needs so far, tables included: checked level by level, so that the host-side tables -- and the int32
    // offsets into the coefficient table -- are bounded by the budget too, not only the arena they are copied into.
    auto need = [&](int64_t more_tiles) {
        return cursor + 32 + (int64_t)(plan->jobs[0].size() + plan->jobs[1].size()) * (int64_t)sizeof(TilerJob) +
               (int64_t)plan->coefs.size() * (int64_t)sizeof(int32_t) +
               ((int64_t)plan->tiles.size() + more_tiles) * (int64_t)sizeof(TileDesc);
    };
    SSW_REQUIRE(need(0) <= budget, "multiscale: the sources alone are %lld bytes, the arena's budget is %lld: hand over fewer "
                "images a call", (long long)plan->src_bytes, (long long)budget);
    for (int i = 0; i < n_images; ++i) {
        const int h = image_hw[2 * i], w = image_hw[2 * i + 1];
        const int64_t src = image_offsets[i];
        const int32_t src_pitch = w * 3;
        for (int l = level_first[i]; l < level_first[i + 1]; ++l) {
            const int lw = level_wh[2 * l], lh = level_wh[2 * l + 1];
            const int32_t pitch = (int32_t)align8((int64_t)lw * 3);
            const bool in_place = lw == w && lh == h && src % 8 == 0 && src_pitch % 8 == 0;  // the level is the source itself
            const int64_t base = in_place ? src : take((int64_t)lh * pitch);
            const int32_t level_pitch = in_place ? src_pitch : pitch;
            if (!in_place) {
                TilerJob j{};
                j.src = src; j.src_pitch = src_pitch; j.src_w = w; j.src_h = h;
                j.dst = base; j.dst_pitch = pitch; j.dst_w = lw; j.dst_h = lh;
                if (lw == w && lh == h) {  // the source's own size, but not on the gather's alignment: a copy, as Pillow makes one
                    j.kind = TILER_COPY;
                    add_job(0, j);
                } else if (lh == h) {
                    j.kind = TILER_HORIZONTAL;
                    coefficients(w, lw, j);
                    add_job(0, j);
                } else if (lw == w) {
                    j.kind = TILER_VERTICAL;
                    coefficients(h, lh, j);
                    add_job(1, j);
                } else {
                    TilerJob hz = j;  // source rows -> [h][lw], then down the columns
                    hz.kind = TILER_HORIZONTAL;
                    hz.dst = take((int64_t)h * pitch);
                    hz.dst_h = h;
                    coefficients(w, lw, hz);
                    add_job(0, hz);
                    j.kind = TILER_VERTICAL;
                    j.src = hz.dst; j.src_pitch = pitch; j.src_w = lw;
                    coefficients(h, lh, j);
                    add_job(1, j);
                }
            }
            const int half = tile / 2;
            int64_t level_tiles = 0;
            for (int si = 0; si < 2; ++si)
                for (int sj = 0; sj < 2; ++sj)
                    level_tiles += (int64_t)(std::max(lh - sj * half, 0) / tile) * (std::max(lw - si * half, 0) / tile);
            SSW_REQUIRE(need(level_tiles) <= budget, "multiscale: sources, levels and tables up to image %d need %lld bytes, the "
                        "arena's budget is %lld: hand over fewer images a call", i, (long long)need(level_tiles), (long long)budget);
            plan->level_base.push_back(base);
            plan->level_pitch.push_back(level_pitch);
            for (int si = 0; si < 2; ++si)
                for (int sj = 0; sj < 2; ++sj) {
                    const int sx = si * half, sy = sj * half;
                    const int nh = std::max(lh - sy, 0) / tile, nw = std::max(lw - sx, 0) / tile;
                    for (int r = 0; r < nh; ++r)
                        for (int q = 0; q < nw; ++q)
                            plan->tiles.push_back(TileDesc{base, level_pitch, sx + q * tile, sy + r * tile, 0});
                }
        }
    }
    plan->jobs_off[0] = take((int64_t)plan->jobs[0].size() * sizeof(TilerJob));
    plan->jobs_off[1] = take((int64_t)plan->jobs[1].size() * sizeof(TilerJob));
    plan->coefs_off = take((int64_t)plan->coefs.size() * sizeof(int32_t));
    plan->tiles_off = take((int64_t)plan->tiles.size() * sizeof(TileDesc));
    plan->arena_bytes = cursor;
    return SSW_OK;  // (cursor <= need(0) <= budget: the tables were counted with 8 bytes of alignment slack each)
}

ssw_status tiler_run(hipStream_t s, uint8_t *arena, const uint8_t *images_host, const TilerPlan &plan) {
    SSW_HIP_TRY(hipMemcpyAsync(arena, images_host, (size_t)plan.src_bytes, hipMemcpyHostToDevice, s));
    for (int l = 0; l < 2; ++l)
        if (!plan.jobs[l].empty())
            SSW_HIP_TRY(hipMemcpyAsync(arena + plan.jobs_off[l], plan.jobs[l].data(), plan.jobs[l].size() * sizeof(TilerJob),
                                       hipMemcpyHostToDevice, s));
    if (!plan.coefs.empty())
        SSW_HIP_TRY(hipMemcpyAsync(arena + plan.coefs_off, plan.coefs.data(), plan.coefs.size() * sizeof(int32_t),
                                   hipMemcpyHostToDevice, s));
    if (!plan.tiles.empty())
        SSW_HIP_TRY(hipMemcpyAsync(arena + plan.tiles_off, plan.tiles.data(), plan.tiles.size() * sizeof(TileDesc),
                                   hipMemcpyHostToDevice, s));
    for (int l = 0; l < 2; ++l)  // every horizontal pass (and copy) of the call, then every vertical pass
        if (plan.blocks[l] > 0)
            hipLaunchKernelGGL(tiler_resample, dim3(plan.blocks[l]), dim3(TILER_BLOCK), 0, s, arena,
                               reinterpret_cast<const TilerJob *>(arena + plan.jobs_off[l]), (int)plan.jobs[l].size(),
                               reinterpret_cast<const int32_t *>(arena + plan.coefs_off));
    SSW_HIP_TRY(hipGetLastError());
    return SSW_OK;
}

}  // namespace ssw

// coarse.hip -- the coarse index's rows out of a resident multiscale index (ssw_index_coarse_mean): per listed image the
// mean of its KEPT rows, normalised.  Replaces infer_coarse_embedding of the reference
// (seesaw/indices/coarse/preprocessor.py:11-19): lev1 = rows with zoom_level == max_zoom_level,
// lev1.groupby("dbidx").vectors.mean(), res / np.maximum(np.linalg.norm(res, axis=1, keepdims=True), 1e-6).
//
// Arithmetic of one image, whose kept rows are r_1 < ... < r_c (keep[r] != 0 inside [row_start[i], row_start[i + 1])):
//   s[e]    = x[r_1][e] + x[r_2][e] + ... + x[r_c][e]    in double, in ascending row order (binary16 rows widened exactly)
//   mean[e] = s[e] / c                                   in double
//   nrm     = sqrt(sum_e mean[e]^2)                      in double (per lane over its elements, then a wave butterfly)
//   out[e]  = (float)(mean[e] / max(nrm, 1e-6))          one rounding; a binary16 destination rounds that f32 once more
// One WAVE per image: lane l holds the dim / 64 elements the scan's lane l works on (256 c + 4 l + j: one float4 a chunk
// of an f32 row, the lane's 8 C contiguous bytes of a binary16 row) as double accumulators, walks the image's rows 64
// mask bytes at a time (one byte a lane, __ballot makes the kept set wave-uniform) and loads kept rows only.  No atomics,
// no partial sums across waves: an image's output depends on its own kept rows and on nothing else -- not on the grid,
// the other images of the call or the CU count.  Purely HBM-bound: kept rows x row bytes + n mask bytes read (a row is
// read once: non-temporal loads, as in the scans), m x dim x 4 (or 2) written.
#include <algorithm>

#include "ssw_common.h"

namespace ssw {

namespace {

constexpr int COARSE_BLOCK = 256;       // 4 waves, an image each
constexpr int COARSE_BLOCKS_PER_CU = 8; // 32 waves a CU: a wave has one or two row loads in flight, occupancy hides the rest

// lane `lane`'s part of row `row` as 4 C floats, chunk c = natural elements 256 c + 4 lane .. + 3
template <int C, bool H16>
__device__ __forceinline__ void load_part(const void *__restrict__ X, int64_t row, int lane, float4 (&v)[C]) {
    if constexpr (H16) {
        const u32x2 *p = reinterpret_cast<const u32x2 *>(static_cast<const unsigned char *>(X) + row * (C * 512) + lane * (C * 8));
        if constexpr (C % 2 == 0) {  // 16-byte aligned: one dwordx4 per two chunks
            const u32x4 *p4 = reinterpret_cast<const u32x4 *>(p);
#pragma unroll
            for (int i = 0; i < C / 2; ++i) {
                const u32x4 w = __builtin_nontemporal_load(p4 + i);
                v[2 * i] = widen_h16x4(u32x2{w.x, w.y});
                v[2 * i + 1] = widen_h16x4(u32x2{w.z, w.w});
            }
        } else {
#pragma unroll
            for (int c = 0; c < C; ++c) v[c] = widen_h16x4(__builtin_nontemporal_load(p + c));
        }
    } else {
        const f32x4 *p = reinterpret_cast<const f32x4 *>(static_cast<const float *>(X) + row * (C * 256)) + lane;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const f32x4 w = __builtin_nontemporal_load(p + c * 64);
            v[c] = make_float4(w.x, w.y, w.z, w.w);
        }
    }
}

template <int C>
__device__ __forceinline__ void add_part(double (&acc)[4 * C], const float4 (&v)[C]) {
#pragma unroll
    for (int c = 0; c < C; ++c) {
        acc[4 * c] += (double)v[c].x;
        acc[4 * c + 1] += (double)v[c].y;
        acc[4 * c + 2] += (double)v[c].z;
        acc[4 * c + 3] += (double)v[c].w;
    }
}

// row_src: the source is a view, keep / row_start are in ITS numbering and row j is the matrix's row row_src[j]
// out_h16: the destination is a binary16 matrix in the index layout, else f32 rows in natural order
template <int C, bool H16>
__global__ __launch_bounds__(COARSE_BLOCK) void k_coarse_mean(const void *__restrict__ X, const int32_t *__restrict__ row_src,
                                                              const unsigned char *__restrict__ keep,
                                                              const int64_t *__restrict__ row_start,
                                                              const int64_t *__restrict__ images, int64_t m,
                                                              void *__restrict__ out, int out_h16) {
    const int lane = threadIdx.x & 63;
    const int64_t waves = (int64_t)gridDim.x * (COARSE_BLOCK / 64);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // (tells the compiler it is wave-uniform)
    for (int64_t i = (int64_t)blockIdx.x * (COARSE_BLOCK / 64) + wave; i < m; i += waves) {
        const int64_t img = images[i];
        const int64_t r0 = row_start[img], r1 = row_start[img + 1];
        double acc[4 * C];
#pragma unroll
        for (int e = 0; e < 4 * C; ++e) acc[e] = 0.0;
        int64_t count = 0;
        for (int64_t base = r0; base < r1; base += 64) {
            const int64_t r = base + lane;
            unsigned long long kept = __ballot(r < r1 && __builtin_nontemporal_load(keep + r) != 0);
            count += __popcll(kept);
            while (kept) {  // ascending rows, two loads in flight; the sum takes them in row order
                const int j0 = __ffsll(kept) - 1;
                kept &= kept - 1;
                const bool two = kept != 0;
                const int j1 = two ? __ffsll(kept) - 1 : j0;
                if (two) kept &= kept - 1;
                int64_t ra = base + j0, rb = base + j1;
                if (row_src) ra = row_src[ra], rb = row_src[rb];
                float4 a[C], b[C];
                load_part<C, H16>(X, ra, lane, a);
                load_part<C, H16>(X, rb, lane, b);
                add_part<C>(acc, a);
                if (two) add_part<C>(acc, b);
            }
        }
        const double c = (double)count;  // >= 1: the entry refuses an image without a kept row on the host
        double ss = 0.0;
#pragma unroll
        for (int e = 0; e < 4 * C; ++e) {
            acc[e] = acc[e] / c;
            ss += acc[e] * acc[e];
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) ss += __shfl_xor(ss, off);  // every lane ends with the same bits
        const double d = fmax(sqrt(ss), 1e-6);
#pragma unroll
        for (int ch = 0; ch < C; ++ch) {
            const float4 o = make_float4((float)(acc[4 * ch] / d), (float)(acc[4 * ch + 1] / d), (float)(acc[4 * ch + 2] / d),
                                         (float)(acc[4 * ch + 3] / d));
            if (out_h16)
                reinterpret_cast<u32x2 *>(static_cast<unsigned char *>(out) + i * (C * 512) + lane * (C * 8))[ch] = round_h16x4(o);
            else
                reinterpret_cast<float4 *>(static_cast<float *>(out) + i * (C * 256))[ch * 64 + lane] = o;
        }
    }
}

template <int C>
void launch_c(bool h16, unsigned blocks, hipStream_t stream, const void *X, const int32_t *row_src, const unsigned char *keep,
              const int64_t *row_start, const int64_t *images, int64_t m, void *out, int out_h16) {
    if (h16)
        hipLaunchKernelGGL((k_coarse_mean<C, true>), dim3(blocks), dim3(COARSE_BLOCK), 0, stream, X, row_src, keep, row_start,
                           images, m, out, out_h16);
    else
        hipLaunchKernelGGL((k_coarse_mean<C, false>), dim3(blocks), dim3(COARSE_BLOCK), 0, stream, X, row_src, keep, row_start,
                           images, m, out, out_h16);
}

}  // namespace

ssw_status launch_coarse_mean(const void *X, int32_t src_dtype, const int32_t *row_src_or_null, const unsigned char *keep,
                              const int64_t *row_start, const int64_t *images, int64_t m, int32_t dim, void *out,
                              int32_t dst_dtype, int device, hipStream_t stream) {
    if (m <= 0) return SSW_OK;
    if (dim <= 0 || dim % 256 != 0 || dim > 1024) {
        set_error("coarse_mean: dim=%d unsupported (need a multiple of 256, <= 1024)", dim);
        return SSW_ERR_UNSUPPORTED;
    }
    const int64_t want = (m + COARSE_BLOCK / 64 - 1) / (COARSE_BLOCK / 64);
    const unsigned blocks = (unsigned)std::min<int64_t>(want, (int64_t)num_cus(device) * COARSE_BLOCKS_PER_CU);
    const bool h16 = src_dtype == SSW_DTYPE_F16;
    const int out_h16 = dst_dtype == SSW_DTYPE_F16 ? 1 : 0;
    switch (dim / 256) {
        case 1: launch_c<1>(h16, blocks, stream, X, row_src_or_null, keep, row_start, images, m, out, out_h16); break;
        case 2: launch_c<2>(h16, blocks, stream, X, row_src_or_null, keep, row_start, images, m, out, out_h16); break;
        case 3: launch_c<3>(h16, blocks, stream, X, row_src_or_null, keep, row_start, images, m, out, out_h16); break;
        default: launch_c<4>(h16, blocks, stream, X, row_src_or_null, keep, row_start, images, m, out, out_h16); break;
    }
    SSW_HIP_TRY(hipGetLastError());
    return SSW_OK;
}

}  // namespace ssw

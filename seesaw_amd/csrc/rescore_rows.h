// rescore_rows.h -- the exact score of ONE index row by ONE wave, shared by the kernels that rescore rows outside the scan:
// k_rescore_survivors (rescore_dev.hip) and k_avg_score_owner (rescore.hip).  The score is the BITS of scan.hip's
// kernels, whose summation order is restated here once (scan.hip itself stays as measured): lane l holds the float4 at
// element 256 c + 4 l of chunk c < C = dim / 256; two packed fma chains, over .x/.y and then .z/.w, c ascending, from
// +0; the lane partial is a.x + a.y; the 64 partials are summed by the butterfly v + shfl_xor(v, off), off = 1, 2, 4, 8,
// 16, 32.  An f16 row (ssw_common.h: lane l's 4 C elements are the 8 C bytes at l * 8 C) is widened exactly first.
// The fma is explicit (__builtin_elementwise_fma), so a translation unit compiled with -ffp-contract=off gets the same
// bits as one compiled without.
#pragma once
#include "ssw_common.h"

namespace ssw {
namespace rows {

typedef float f32x2 __attribute__((ext_vector_type(2)));

template <int C>
struct Frag {
    float4 v[C];
};

struct F32Rows {
    typedef float T;
    template <int C>
    static __device__ __forceinline__ Frag<C> load(const float *__restrict__ X, int64_t row, int lane) {
        Frag<C> r;
        const float4 *p = reinterpret_cast<const float4 *>(X) + row * (C * 64) + lane;
#pragma unroll
        for (int c = 0; c < C; ++c) r.v[c] = p[c * 64];
        return r;
    }
};

struct H16Rows {
    typedef uint16_t T;
    template <int C>
    static __device__ __forceinline__ Frag<C> load(const uint16_t *__restrict__ X, int64_t row, int lane) {
        Frag<C> r;
        const unsigned char *p = reinterpret_cast<const unsigned char *>(X) + row * (C * 512) + lane * (C * 8);
        if constexpr (C % 2 == 0) {  // 16-byte aligned: one dwordx4 per two chunks
            const u32x4 *p4 = reinterpret_cast<const u32x4 *>(p);
#pragma unroll
            for (int i = 0; i < C / 2; ++i) {
                const u32x4 w = p4[i];
                r.v[2 * i] = widen_h16x4(u32x2{w.x, w.y});
                r.v[2 * i + 1] = widen_h16x4(u32x2{w.z, w.w});
            }
        } else {
            const u32x2 *p2 = reinterpret_cast<const u32x2 *>(p);
#pragma unroll
            for (int c = 0; c < C; ++c) r.v[c] = widen_h16x4(p2[c]);
        }
        return r;
    }
};

// a query's fragment: lane l's float4 of every chunk of the f32 query at q
template <int C>
__device__ __forceinline__ Frag<C> load_query(const float *__restrict__ q, int lane) {
    Frag<C> r;
#pragma unroll
    for (int c = 0; c < C; ++c) r.v[c] = reinterpret_cast<const float4 *>(q)[c * 64 + lane];
    return r;
}

// the lane partial: scan.hip's dot_frag
template <int C>
__device__ __forceinline__ float lane_partial(const Frag<C> &x, const Frag<C> &q) {
    f32x2 a = {0.0f, 0.0f};
#pragma unroll
    for (int c = 0; c < C; ++c) {
        a = __builtin_elementwise_fma(f32x2{x.v[c].x, x.v[c].y}, f32x2{q.v[c].x, q.v[c].y}, a);
        a = __builtin_elementwise_fma(f32x2{x.v[c].z, x.v[c].w}, f32x2{q.v[c].z, q.v[c].w}, a);
    }
    return a.x + a.y;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) v = v + __shfl_xor(v, off, 64);
    return v;
}

}  // namespace rows
}  // namespace ssw

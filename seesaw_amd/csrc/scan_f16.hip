// scan_f16.hip -- the scan kernels of the f16 index (SSW_DTYPE_F16): scores[i] = <widen(X[i,:]), q>  (gfx950 / MI355X)
//
// The f16 index stores each element as IEEE binary16 (round to nearest even, subnormals kept) in a lane-interleaved
// row layout (ssw_common.h, h16_group_pos): lane l of a wave owns the elements {256c + 4l .. +3} exactly as in the f32
// scan (scan.hip), and those 4*C elements are 8*C contiguous bytes -- one 16-byte `global_load_dwordx4 ... nt` per lane
// per row at dim 512.  Rows stay dim*2 contiguous bytes.  Each fragment is widened with v_cvt_f32_f16 (exact; the code
// object keeps f16 denormals: .amdhsa_float_denorm_mode_16_64 3) into the float4s the f32 kernel would have loaded for
// the widened row, and dot_frag / group_reduce below are the f32 scan's, statement for statement: the same products and
// sums in the same order, so the scores are the BITS of the f32 scan over X.astype(float16).astype(float32) and the
// f32 oracle (oracle/ssw_oracle.c::ssw_oracle_scores_kernel_order) checks them unchanged.
//
// Roofline: HBM-bound, dim*2 bytes per row read once (1 KiB at dim 512) + 4 B of score.  Same schedule as the f32
// scan (persistent grid, one 4-wave block per CU at dim 512, register double buffer) with twice the rows per group:
// the same bytes in flight per wave.
#include "ssw_common.h"

namespace ssw {

namespace {

// ---- the f32 scan's lane arithmetic (scan.hip), kept identical: the bit-exactness argument rests on it
template <int C>
struct RowFrag {
    float4 v[C];
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

// U lane-partial registers (acc[j] = row j of the group) -> every lane l holds the
// complete sum of row (l % U): transpose-reduce over offsets 1..U/2, then butterfly
// over offsets U..32.  Canonical offset order 1,2,4,8,16,32 for every U.
template <int U>
__device__ __forceinline__ float group_reduce(float (&acc)[U], int lane) {
#pragma unroll
    for (int off = 1; off < U; off <<= 1) {
        // register distance of the pair merged at this offset == off
        const bool upper = (lane & off) != 0;
#pragma unroll
        for (int i = 0; i < U; i += 2 * off) {
            const float keep = upper ? acc[i + off] : acc[i];
            const float send = upper ? acc[i] : acc[i + off];
            acc[i] = keep + __shfl_xor(send, off, 64);
        }
    }
    float v = acc[0];
#pragma unroll
    for (int off = U; off < 64; off <<= 1) v = v + __shfl_xor(v, off, 64);
    return v;
}

// ---- binary16 rows in the f16 index's lane-interleaved layout (ssw_common.h): lane l's 4*C elements are its 8*C
// contiguous bytes of the row.  A fragment is loaded raw (it stays packed until it is used, so the register double
// buffer keeps its loads in flight) and widened to the float4s of the f32 layout right before dot_frag.
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 h16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

template <int C>
struct HalfFrag {
    u32x2 w[C];  // chunk c = elements 256*c + 4*l .. +3
};

template <int C, bool NT>
__device__ __forceinline__ HalfFrag<C> load_row_h16(const uint16_t *__restrict__ X, int row, int lane) {
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

// v_cvt_f32_f16 is exact (f16 denormals are kept: .amdhsa_float_denorm_mode_16_64 of the code object)
__device__ __forceinline__ float4 widen4(u32x2 w) {
    const f32x4 f = __builtin_convertvector(__builtin_bit_cast(h16x4, w), f32x4);
    return make_float4(f.x, f.y, f.z, f.w);
}

template <int C>
__device__ __forceinline__ RowFrag<C> widen(const HalfFrag<C> &f) {
    RowFrag<C> r;
#pragma unroll
    for (int c = 0; c < C; ++c) r.v[c] = widen4(f.w[c]);
    return r;
}

template <int C, int U>
struct Group {
    HalfFrag<C> r[U];
};

template <int C, int U, bool NT>
__device__ __forceinline__ void load_group(Group<C, U> &g, const uint16_t *__restrict__ X, int first_row, int last,
                                           int lane) {
#pragma unroll
    for (int u = 0; u < U; ++u) g.r[u] = load_row_h16<C, NT>(X, min(first_row + u, last), lane);
}

// f16 index: the f32 streaming kernel's walk over half-size rows (twice the rows per group at the same bytes in flight
// per wave)
template <int C, int U, bool NT>
__global__ __launch_bounds__(256) void scan_h16_kernel(const uint16_t *__restrict__ X, const float *__restrict__ q,
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
    Group<C, U> cur, nxt;
    load_group<C, U, NT>(cur, X, gwave << 6, last, lane);
    for (int b = gwave; b < nbatches; b += nwaves) {
        const int row0 = b << 6;
        const int nb = b + nwaves;
        const int next0 = (nb < nbatches ? nb : b) << 6;  // no next batch: re-touch own rows
        float out = 0.0f;
#pragma unroll 2
        for (int g = 0; g < GPB; ++g) {
            // request group g+1 (or the first group of this wave's next batch) ...
            const int nrow = (g + 1 < GPB) ? row0 + (g + 1) * U : next0;
            load_group<C, U, NT>(nxt, X, nrow, last, lane);
            // ... then finish group g
            float acc[U];
#pragma unroll
            for (int u = 0; u < U; ++u) acc[u] = dot_frag<C>(widen<C>(cur.r[u]), qf);
            const float v = group_reduce<U>(acc, lane);
            out = (my_group == g) ? v : out;
            cur = nxt;
        }
        if (row0 + lane < n) scores[row0 + lane] = out;
    }
}

// small index (under SCAN_SMALL_ROWS): scan.hip's latency-shaped kernel, U rows per wave all in flight at once
template <int C, int U>
__global__ __launch_bounds__(256) void scan_small_h16_kernel(const uint16_t *__restrict__ X, const float *__restrict__ q,
                                                             float *__restrict__ scores, int n, int steps) {
    __shared__ float4 ql[C * 64];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int last = n - 1;
    const int row_base = (blockIdx.x * 4 + wave) * U * steps;
    Group<C, U> cur, nxt;
    load_group<C, U, false>(cur, X, row_base, last, lane);
    for (int i = threadIdx.x; i < C * 64; i += 256) ql[i] = reinterpret_cast<const float4 *>(q)[i];
    __syncthreads();
    RowFrag<C> qf;
#pragma unroll
    for (int c = 0; c < C; ++c) qf.v[c] = ql[c * 64 + lane];
    for (int g = 0; g < steps; ++g) {
        const int row0 = row_base + g * U;
        if (row0 >= n) break;
        if (g + 1 < steps) load_group<C, U, false>(nxt, X, row0 + U, last, lane);
        float acc[U];
#pragma unroll
        for (int u = 0; u < U; ++u) acc[u] = dot_frag<C>(widen<C>(cur.r[u]), qf);
        const float v = group_reduce<U>(acc, lane);
        if (lane < U && row0 + lane < n) scores[row0 + lane] = v;
        cur = nxt;
    }
}

// scores of an explicit list of rows, same summation order as the full scan (one wave per
// row, plain butterfly) -- stage-2 rescoring against a second vector
// (multiscale_index.py:347-349).
template <int C>
__global__ __launch_bounds__(256) void score_rows_h16_kernel(const uint16_t *__restrict__ X, const float *__restrict__ q,
                                                            const int64_t *__restrict__ rows, int64_t n,
                                                            float *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= n) return;
    RowFrag<C> qf;
#pragma unroll
    for (int c = 0; c < C; ++c) qf.v[c] = reinterpret_cast<const float4 *>(q)[c * 64 + lane];
    const RowFrag<C> x = widen<C>(load_row_h16<C, false>(X, (int)rows[w], lane));
    float v = dot_frag<C>(x, qf);
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) v = v + __shfl_xor(v, off, 64);
    if (lane == 0) out[w] = v;
}


// ---- launch
constexpr int64_t SCAN_SMALL_ROWS = 65536;  // as scan.hip: below, the latency-shaped kernel
SSW_TUNABLE bool g_scan_small = true;       // tuning hooks (ssw_tune_scan drives both element types)
SSW_TUNABLE int g_scan_variant = -1;
SSW_TUNABLE int g_scan_blocks_per_cu = -1;

template <int C, int U, bool NT>
ssw_status launch_scan_t(const uint16_t *X, const float *q, float *scores, int64_t n, int device,
                         hipStream_t stream) {
    static int max_blocks_per_cu[16] = {0};
    int dev_slot = device & 15;
    if (max_blocks_per_cu[dev_slot] == 0) {
        int nb = 0;
        SSW_HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, scan_h16_kernel<C, U, NT>,
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
        hipLaunchKernelGGL((scan_small_h16_kernel<C, SU>), dim3((unsigned)sgrid), dim3(256), 0, stream, X, q, scores, (int)n,
                           steps);
        SSW_HIP_TRY(hipGetLastError());
        return SSW_OK;
    }
    const int64_t nbatches = (n + 63) >> 6;
    int64_t grid = (int64_t)num_cus(device) * blocks_per_cu[dev_slot];
    const int64_t need = (nbatches + 3) / 4;
    if (grid > need) grid = need;
    if (grid < 1) grid = 1;
    hipLaunchKernelGGL((scan_h16_kernel<C, U, NT>), dim3((unsigned)grid), dim3(256), 0, stream, X,
                       q, scores, (int)n);
    SSW_HIP_TRY(hipGetLastError());
    return SSW_OK;
}

}  // namespace

// f16 index: a row is half the bytes, so a group is twice the rows of the f32 schedule (the same bytes in flight per
// wave); one 4-wave block per CU at dim 512 as for f32.  Variants (ssw_tune_scan, dim 512): 1 = u8 + nt, 4 = u2 + nt,
// 0 = u4 plain loads.
ssw_status launch_scan_h16(const uint16_t *X, const float *q_dev, float *scores, int64_t n, int32_t dim,
                           int device, hipStream_t stream) {
    if (n <= 0) return SSW_OK;
    switch (dim) {
        case 256: return launch_scan_t<1, 16, true>(X, q_dev, scores, n, device, stream);
        case 512: {
            switch (g_scan_variant) {
                case 0: return launch_scan_t<2, 4, false>(X, q_dev, scores, n, device, stream);
                case 1: return launch_scan_t<2, 8, true>(X, q_dev, scores, n, device, stream);
                case 4: return launch_scan_t<2, 2, true>(X, q_dev, scores, n, device, stream);
                default: return launch_scan_t<2, 4, true>(X, q_dev, scores, n, device, stream);
            }
        }
        case 768: return launch_scan_t<3, 4, true>(X, q_dev, scores, n, device, stream);
        case 1024: return launch_scan_t<4, 4, true>(X, q_dev, scores, n, device, stream);
        default:
            set_error("scan: dim=%d unsupported (need a multiple of 256, <= 1024)", dim);
            return SSW_ERR_UNSUPPORTED;
    }
}

ssw_status launch_score_rows_h16(const uint16_t *X, const float *q_dev, const int64_t *rows_dev, int64_t n,
                                 int32_t dim, float *out, hipStream_t stream) {
    if (n <= 0) return SSW_OK;
    const dim3 grid((unsigned)((n + 3) / 4)), block(256);
    switch (dim) {
        case 256: hipLaunchKernelGGL(score_rows_h16_kernel<1>, grid, block, 0, stream, X, q_dev, rows_dev, n, out); break;
        case 512: hipLaunchKernelGGL(score_rows_h16_kernel<2>, grid, block, 0, stream, X, q_dev, rows_dev, n, out); break;
        case 768: hipLaunchKernelGGL(score_rows_h16_kernel<3>, grid, block, 0, stream, X, q_dev, rows_dev, n, out); break;
        case 1024: hipLaunchKernelGGL(score_rows_h16_kernel<4>, grid, block, 0, stream, X, q_dev, rows_dev, n, out); break;
        default:
            set_error("score_rows: dim=%d unsupported", dim);
            return SSW_ERR_UNSUPPORTED;
    }
    SSW_HIP_TRY(hipGetLastError());
    return SSW_OK;
}

// ---- conversions between natural-order rows and the f16 layout (upload, download, gather) --------------------------
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
    if constexpr (FROM_F32) {
        const float4 v = reinterpret_cast<const float4 *>(src_f32 + r * dim)[e >> 2];
        // v_cvt_f16_f32: round to nearest even, subnormals kept, overflow to +-inf (numpy's astype(float16))
        const h16x4 h = __builtin_convertvector((f32x4{v.x, v.y, v.z, v.w}), h16x4);
        w = __builtin_bit_cast(u32x2, h);
    } else {
        w = reinterpret_cast<const u32x2 *>(src_h16 + r * dim)[e >> 2];
    }
    *reinterpret_cast<u32x2 *>(dst + r * dim + h16_group_pos(e, dim >> 8)) = w;
}

__global__ __launch_bounds__(256) void k_rows_from_h16(const uint16_t *__restrict__ X, const int64_t *__restrict__ rows,
                                                       int64_t first_row, int64_t n, int dim, float *__restrict__ out) {
    const int groups = dim >> 2;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n * groups) return;
    const int64_t i = t / groups;
    const int e = (int)(t - i * groups) << 2;
    const int64_t r = rows ? rows[i] : first_row + i;
    const u32x2 w = *reinterpret_cast<const u32x2 *>(X + r * dim + h16_group_pos(e, dim >> 8));
    reinterpret_cast<float4 *>(out + i * dim)[e >> 2] = widen4(w);
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

ssw_status launch_rows_from_h16(const uint16_t *X, const int64_t *rows_dev, int64_t first_row, int64_t n, int32_t dim,
                                float *out, hipStream_t stream) {
    if (n <= 0) return SSW_OK;
    if (dim <= 0 || dim % 256 != 0 || dim > 1024) {
        set_error("rows_from_h16: dim=%d unsupported", dim);
        return SSW_ERR_UNSUPPORTED;
    }
    const int64_t blocks = (n * (dim / 4) + 255) / 256;
    hipLaunchKernelGGL(k_rows_from_h16, dim3((unsigned)blocks), dim3(256), 0, stream, X, rows_dev, first_row, n, (int)dim, out);
    SSW_HIP_TRY(hipGetLastError());
    return SSW_OK;
}

#ifdef SSW_DEBUG_HOOKS
void tune_scan_h16(int variant, int blocks_per_cu) {
    g_scan_small = variant == -1;
    if (variant < -1) variant = -1;
    g_scan_variant = variant;
    g_scan_blocks_per_cu = blocks_per_cu;
}
#endif

}  // namespace ssw

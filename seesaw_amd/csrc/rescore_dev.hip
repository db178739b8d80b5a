// rescore_dev.hip -- exact rescoring of a pruned chunk's survivors, sized on the device ("Pruned
// sharded batch").  The host-waiting chunk (index_batch.hip, prune_scan_chunk) reads every slot's survivor count back and
// sizes one score_rows_kernel and one scatter launch per slot by it.  Here ONE launch serves the chunk and no count
// leaves the device: the grid depends on the device alone, gridDim.y is the chunk's width, and slot j's waves read their
// own state words (prune.hip: [0] survivors, [2] unboundable, [5] selection failed), grid-stride over the slot's
// survivor list and store each exact score straight into the slot's slab.  A slot whose certificate failed is left as it
// is -- lower bounds -- and k_mark_uncertified says so in the slot's exchange message.
//
// The score is the BITS of scan.hip's kernels: the row loads and the summation order are rescore_rows.h's.
#include "rescore_rows.h"

namespace ssw {

namespace {

using namespace rows;

constexpr int RESCORE_BLOCKS_PER_CU = 1;  // four-wave blocks per CU and slot; a chunk of 16 slots is 16 of them a CU
constexpr int RESCORE_IN_FLIGHT = 2;      // rows a wave has requested before it reduces the first

// grid (blocks, w): slot j = blockIdx.y.  mq: the chunk's state words, read only.  lists: slot j's rows at
// lists + j * list_stride, the first st[0] <= cap of them written by k_survivors_mq.  Slab j of w is side + j * stride,
// the last one `own` (index_batch.hip, chunk_slab).
template <class R, int C>
__global__ __launch_bounds__(256) void k_rescore_survivors(const typename R::T *__restrict__ X, const float *__restrict__ qb,
                                                          const unsigned *__restrict__ mq,
                                                          const int64_t *__restrict__ lists, int64_t list_stride,
                                                          int64_t cap, float *__restrict__ side, int64_t stride,
                                                          float *__restrict__ own, int64_t n) {
    const int j = blockIdx.y, w = gridDim.y;
    const unsigned *st = mq + j * Q8_MQ_WORDS;
    const int64_t m = (int64_t)st[0];
    if ((st[5] | st[2]) != 0u || m > cap) return;  // not certified: the slab keeps its bounds
    const int lane = threadIdx.x & 63;
    const int64_t gwave = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t nwaves = (int64_t)gridDim.x * 4;
    if (gwave >= m) return;
    const int64_t *rows = lists + (int64_t)j * list_stride;
    float *slab = j + 1 < w ? side + (int64_t)j * stride : own;
    const Frag<C> qf = load_query<C>(qb + (int64_t)j * (C * 256), lane);
    for (int64_t i = gwave; i < m; i += RESCORE_IN_FLIGHT * nwaves) {
        const int64_t i1 = i + nwaves;
        const bool two = i1 < m;
        const int64_t r0 = rows[i], r1 = rows[two ? i1 : i];  // wave-uniform
        // (a list holds rows of the index; anything else is skipped, never dereferenced)
        const bool ok0 = (uint64_t)r0 < (uint64_t)n, ok1 = two && (uint64_t)r1 < (uint64_t)n;
        const Frag<C> x0 = R::template load<C>(X, ok0 ? r0 : 0, lane);
        const Frag<C> x1 = R::template load<C>(X, ok1 ? r1 : 0, lane);
        const float v0 = wave_sum(lane_partial<C>(x0, qf));
        const float v1 = wave_sum(lane_partial<C>(x1, qf));
        if (lane == 0) {
            if (ok0) slab[r0] = v0;
            if (ok1) slab[r1] = v1;
        }
    }
}

// the last word of a slot's exchange message (count | flags << 32, written by the selection that has just run on the
// stream) gets bit 33 when the slot's certificate failed: "this rank's scores for this query are bounds"
__global__ void k_mark_uncertified(const unsigned *__restrict__ st, int64_t cap, unsigned long long *__restrict__ word) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if ((st[5] | st[2]) != 0u || (int64_t)st[0] > cap) *word = *word | (2ull << 32);
}

int rescore_blocks(int device, int64_t cap) {
    int64_t grid = (int64_t)num_cus(device) * RESCORE_BLOCKS_PER_CU;
    const int64_t need = (cap + 4 * RESCORE_IN_FLIGHT - 1) / (4 * RESCORE_IN_FLIGHT);  // what the loop needs at cap
    if (grid > need) grid = need;
    return (int)(grid < 1 ? 1 : grid);
}

template <class R>
ssw_status launch_t(const void *Xv, const float *qb, const unsigned *mq, const int64_t *lists, int64_t list_stride,
                    int64_t cap, int32_t w, float *side, int64_t stride, float *own, int64_t n, int32_t dim, int device,
                    hipStream_t stream) {
    const typename R::T *X = static_cast<const typename R::T *>(Xv);
    const dim3 grid((unsigned)rescore_blocks(device, cap), (unsigned)w), block(256);
#define SSW_RESCORE_DEV(C)                                                                                        \
    hipLaunchKernelGGL((k_rescore_survivors<R, C>), grid, block, 0, stream, X, qb, mq, lists, list_stride, cap, side, \
                       stride, own, n)
    switch (dim) {
        case 256: SSW_RESCORE_DEV(1); break;
        case 512: SSW_RESCORE_DEV(2); break;
        case 768: SSW_RESCORE_DEV(3); break;
        case 1024: SSW_RESCORE_DEV(4); break;
        default:
            set_error("rescore_survivors: dim=%d unsupported", dim);
            return SSW_ERR_UNSUPPORTED;
    }
#undef SSW_RESCORE_DEV
    SSW_HIP_TRY(hipGetLastError());
    return SSW_OK;
}

}  // namespace

int rescore_survivors_waves(int device, int64_t cap) { return rescore_blocks(device, cap) * 4; }

ssw_status launch_rescore_survivors(const void *X, int32_t dtype, const float *qb_dev, const unsigned *mq,
                                    const int64_t *lists, int64_t list_stride, int64_t cap, int32_t w, float *side,
                                    int64_t stride, float *own, int64_t n, int32_t dim, int device, hipStream_t stream) {
    if (n <= 0 || w <= 0) return SSW_OK;
    if (w > Q8_MQ_WIDTH || cap < 1 || cap > list_stride || n >= (int64_t)0x7fff0000 || (w > 1 && side == nullptr)) {
        set_error("rescore_survivors: w=%d, cap=%lld of %lld, n=%lld", w, (long long)cap, (long long)list_stride,
                  (long long)n);
        return SSW_ERR_INVALID;
    }
    if (dtype == SSW_DTYPE_F16)
        return launch_t<H16Rows>(X, qb_dev, mq, lists, list_stride, cap, w, side, stride, own, n, dim, device, stream);
    return launch_t<F32Rows>(X, qb_dev, mq, lists, list_stride, cap, w, side, stride, own, n, dim, device, stream);
}

ssw_status launch_mark_uncertified(const unsigned *slot_state, int64_t cap, uint64_t *msg_last_word, hipStream_t stream) {
    hipLaunchKernelGGL(k_mark_uncertified, dim3(1), dim3(1), 0, stream, slot_state, cap,
                       reinterpret_cast<unsigned long long *>(msg_last_word));
    SSW_HIP_TRY(hipGetLastError());
    return SSW_OK;
}

}  // namespace ssw

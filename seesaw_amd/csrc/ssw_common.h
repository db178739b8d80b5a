// Shared host-side helpers for libseesaw_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/seesaw_hip.h"
#ifdef SSW_DEBUG_HOOKS
#include "../../include/seesaw_hip_debug.h"
#endif

// Kernel-selection switches are file-scope constants in the product library; only the lab build (-DSSW_DEBUG_HOOKS ->
// libseesaw_hip_debug.so, entry points in include/seesaw_hip_debug.h) can change them.
#ifdef SSW_DEBUG_HOOKS
#define SSW_TUNABLE
#else
#define SSW_TUNABLE const
#endif

namespace ssw {

void set_error(const char *fmt, ...);

#define SSW_HIP_TRY(expr)                                                                   \
    do {                                                                                    \
        hipError_t _e = (expr);                                                             \
        if (_e != hipSuccess) {                                                             \
            ssw::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, \
                           __LINE__);                                                       \
            return (_e == hipErrorOutOfMemory) ? SSW_ERR_NOMEM : SSW_ERR_HIP;               \
        }                                                                                   \
    } while (0)

#define SSW_REQUIRE(cond, ...)           \
    do {                                 \
        if (!(cond)) {                   \
            ssw::set_error(__VA_ARGS__); \
            return SSW_ERR_INVALID;      \
        }                                \
    } while (0)

#define SSW_TRY(expr)                   \
    do {                                \
        ssw_status _s = (expr);         \
        if (_s != SSW_OK) return _s;    \
    } while (0)

// Orderable key of an f32: ascending unsigned order == ascending float order
// (-inf lowest; used with -inf for excluded images).
__host__ __device__ inline uint32_t f32_to_ord(float f) {
    uint32_t u;
#if defined(__HIP_DEVICE_COMPILE__)
    u = __float_as_uint(f);
#else
    memcpy(&u, &f, 4);
#endif
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__host__ __device__ inline float ord_to_f32(uint32_t o) {
    uint32_t u = (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o;
#if defined(__HIP_DEVICE_COMPILE__)
    return __uint_as_float(u);
#else
    float f;
    memcpy(&f, &u, 4);
    return f;
#endif
}

// One LDS-DMA wave-instruction: 64 lanes x 16 B from per-lane global addresses to the LDS bytes
// [lds_dst, lds_dst + 1024) in lane order (lds_dst is wave-uniform).  Issued from inline asm so that the
// compiler's wait-count bookkeeping is not disturbed: for the builtin form it degrades every later
// s_waitcnt lgkmcnt / vmcnt to (0), which serialises fragment reads and MFMAs.  The vmcnt accounting for
// these loads is done by hand at the call sites (gemm_bf16.hip, knn.hip).
__device__ __forceinline__ void glds16(const void *gsrc, unsigned lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(gsrc), "s"(lds_dst)
                 : "memory");
}

// the same with the address split into a wave-uniform base (SGPR pair) and a 32-bit per-lane byte offset
__device__ __forceinline__ void glds16s(unsigned voff, const void *sbase, unsigned lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(voff), "s"(sbase), "s"(lds_dst)
                 : "memory");
}

struct DeviceGuard {
    int prev = -1;
    bool ok = false;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        ok = (hipSetDevice(dev) == hipSuccess);
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

int num_cus(int device);

// Pinned host staging for small host->device inputs (query vectors, id lists): the
// caller's buffer is copied into pinned memory on the CPU, so the async H2D copy never
// reads memory the caller may free, and no stream synchronisation is needed.
struct PinnedStage {
    void *host = nullptr;
    size_t cap = 0;
    hipEvent_t ev = nullptr;
    bool pending = false;
    ssw_status push(void *dev_dst, const void *src, size_t bytes, hipStream_t stream);
    void release();
};

// ---- launchers implemented in the kernel translation units -----------------

// index_topk.hip: the two halves of ssw_index_topk(q = NULL) on a stream of the caller's (ssw_labelprop_round), which
// has made sure that the handle's own stream is idle (ssw_index_sync) and holds a DeviceGuard on the index's device
// (neither half sets the device itself)
ssw_status index_enqueue_topk_resident(ssw_index *idx, hipStream_t on_stream, const int64_t *excluded_images, int64_t n_excluded,
                                       int32_t k);
ssw_status index_collect_topk(ssw_index *idx, hipStream_t on_stream, int32_t k, int64_t *out_images, float *out_scores,
                              int64_t *out_best_rows, int32_t *out_count);
// ... and once per slot of a chunk (ssw_labelprop_round_batch).  index_round_slabs: the score slabs of a chunk of up to
// w (<= 16) slots -- *out_w is the width the side buffer could be grown to, slabs[j] slot j's slab; the last one is the
// handle's own score buffer.  index_enqueue_topk_slot: install_excluded + the ordinary selection over `slab`, which
// publishes into the slot's own pinned block under *out_seq.  index_collect_topk_slot: the wait on that word, the deep
// rerun from the slab when the fast selection overflowed (*reran), the decode.
ssw_status index_round_slabs(ssw_index *idx, int w, int *out_w, float **slabs);
ssw_status index_enqueue_topk_slot(ssw_index *idx, hipStream_t on_stream, int slot, const float *slab,
                                   const int64_t *excluded_images, int64_t n_excluded, int32_t k, unsigned *out_seq);
ssw_status index_wait_topk_slot(ssw_index *idx, hipStream_t on_stream, int slot, unsigned seq);  // the wait alone
ssw_status index_collect_topk_slot(ssw_index *idx, hipStream_t on_stream, int slot, unsigned seq, const float *slab,
                                   const int64_t *excluded_images, int64_t n_excluded, int32_t k, int64_t *out_images,
                                   float *out_scores, int64_t *out_best_rows, int32_t *out_count, bool *reran);
int index_device(const ssw_index *idx);
// element type of the resident matrix (SSW_DTYPE_*), its device pointer and shape, for the entries that read it through
// a handle without index_handle.h (feedback gathers; k-NN and X'LX refuse an f16 matrix)
int32_t index_dtype(const ssw_index *idx);
const void *index_matrix(const ssw_index *idx, int64_t *n_rows, int32_t *dim);
// A view (ssw_index_create_view) reads its rows out of its parent's matrix through a row table.  refuse_view: the one
// refusal of every entry that would read or write the matrix with the view's own row numbers (SSW_ERR_UNSUPPORTED, the
// message names `who` and says "view").  index_view_rows: the parent row of each view row (host, [n]), NULL for an
// index that is not a view; index_matrix then reports the PARENT's row count.
ssw_status refuse_view(const ssw_index *idx, const char *who);
const int32_t *index_view_rows(const ssw_index *idx);

// ---- the f16 index's row layout ---------------------------------------------------------------------------------
// A row of dim = 256*C binary16 elements is stored LANE-INTERLEAVED: the 4*C elements scan lane l works on
// (256*c + 4*l + j, c < C, j < 4, the f32 scan's lane/element map) are the 8*C contiguous bytes at l*8*C, chunk c at
// byte 8*c inside them.  A row stays dim*2 contiguous bytes; at dim 512 a lane reads its part with one 16-byte load.
// Position (in elements) of the 4-element group that starts at natural element e (e % 4 == 0) of a row:
__host__ __device__ inline int h16_group_pos(int e, int C) { return ((e & 255) >> 2) * 4 * C + (e >> 8) * 4; }
// A 4-element group of binary16 is one u32x2.  Widening is exact (v_cvt_f32_f16; the code objects keep f16 denormals,
// .amdhsa_float_denorm_mode_16_64 3); rounding is to nearest even with subnormals kept and overflow to +-inf
// (v_cvt_f16_f32: numpy's astype(float16)).
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 h16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 widen_h16x4(u32x2 w) {
    const f32x4 f = __builtin_convertvector(__builtin_bit_cast(h16x4, w), f32x4);
    return make_float4(f.x, f.y, f.z, f.w);
}
__device__ __forceinline__ u32x2 round_h16x4(float4 v) {
    return __builtin_bit_cast(u32x2, __builtin_convertvector((f32x4{v.x, v.y, v.z, v.w}), h16x4));
}

// scan.hip: scores[i] = dot(X[i,:], q) in the fixed kernel order (see scan.hip), over an index matrix of element type
// dtype (SSW_DTYPE_F32, or SSW_DTYPE_F16 in the layout above: the bits of the f32 kernels on the widened rows)
ssw_status launch_scan(const void *X, int32_t dtype, const float *q_dev, float *scores, int64_t n, int32_t dim,
                       int device, hipStream_t stream);
ssw_status launch_score_rows(const void *X, int32_t dtype, const float *q_dev, const int64_t *rows_dev, int64_t n,
                             int32_t dim, float *out, hipStream_t stream);
// the scan of a view (ssw_index_create_view): scores[j] = dot(X[row_src[j],:], q), the bits launch_scan gives that row
ssw_status launch_scan_view(const void *X, int32_t dtype, const float *q_dev, const int32_t *row_src, float *scores,
                            int64_t n_view, int32_t dim, int device, hipStream_t stream);
// the multi-query form: slabs[b][i] = dot(X[i,:], qb_dev[b,:]) for b < nb in ONE pass over the rows, per query the bits
// of launch_scan.  nb = 2, 4, 8 or 16, at most scan_batch_max_width(n, dim, dtype) (1 = this shape has no batched kernel)
int scan_batch_max_width(int64_t n, int32_t dim, int32_t dtype);
ssw_status launch_scan_batch(const void *X, int32_t dtype, const float *qb_dev, float *const *slabs, int32_t nb,
                             int64_t n, int32_t dim, int device, hipStream_t stream);
// the multi-query form over a view's rows: slabs[b][j] = dot(X[row_src[j],:], qb_dev[b,:]) for j < n_view, per query the
// bits of launch_scan_view.  nb at most scan_view_batch_max_width(n_view, dim, dtype): scan_batch_max_width, narrowed
// where the view instance of a width is not built
int scan_view_batch_max_width(int64_t n_view, int32_t dim, int32_t dtype);
ssw_status launch_scan_view_batch(const void *X, int32_t dtype, const float *qb_dev, const int32_t *row_src,
                                  float *const *slabs, int32_t nb, int64_t n_view, int32_t dim, int device,
                                  hipStream_t stream);
// prune.hip: the int8 shadow of an index (rows of element type dtype: f32, or binary16 in the layout above, taken as
// their widened values) and the certified pre-scan of the exact top-k (see prune.hip).
// query state words: [0] survivors, [1] Q = ||q|| rounded up (f32 bits), [2] 1 = the query cannot be bounded
bool q8_dim_supported(int32_t dim);
// the dims of the packed 6-bit shadow's builders and scans: those of the int8 shadow and 768, which has no int8 shadow
bool q6_dim_supported(int32_t dim);
ssw_status launch_q8_build(const void *X, int32_t dtype, int64_t n, int32_t dim, unsigned char *codes, float *scale,
                           float *err, hipStream_t stream);
ssw_status launch_q8_query(const float *q_dev, int32_t dim, float *q_keep, unsigned *state, hipStream_t stream);
ssw_status launch_q8_bounds(const unsigned char *codes, const float *scale, const float *err, const float *q_dev,
                            const unsigned *state, float *scores, int64_t n, int32_t dim, int device, hipStream_t stream);
// mx[0], mx[1] = the largest finite a_r and s_r of a shadow (float bits): what the survivor passes pre-test lb with
constexpr int SHADOW_MAX_WORDS = 2;
ssw_status launch_shadow_max(const float *err, const float *scale, int64_t n, unsigned *mx, int device, hipStream_t stream);
// rows with upper bound >= the k-th key of the last selection -> rows[0, cap), then host_block[1] = survivors or -1
// (fall back to the full scan) and host_block[0] = seq, released to the host
ssw_status launch_survivors(const float *lb, const float *err, const unsigned *mx, int64_t n, const uint64_t *keys,
                            const int32_t *sel_count, int32_t k, unsigned *state, int64_t *rows, int64_t cap, int32_t *host_block, unsigned seq,
                            int device, hipStream_t stream);
ssw_status launch_scatter_scores(const int64_t *rows, const float *v, int64_t m, float *scores, hipStream_t stream);
// the same for a chunk of w <= 16 queries, bounded together by one pass on the int8 matrix core (prune.hip, "Pruned
// batch").  mq: Q8_MQ_WORDS words a slot ([0] survivors, [1] Q, [2] unboundable, [3] e, [4] t2, [5] selection failed);
// planes: q8_mq_plane_bytes(dim) bytes of query codes; slab j of the bounds is side + j * stride, the last one `own`.
constexpr int Q8_MQ_WIDTH = 16, Q8_MQ_WORDS = 8;
size_t q8_mq_plane_bytes(int32_t dim);
ssw_status launch_q8_query_mq(const float *qb_dev, int32_t dim, int32_t w, unsigned *mq, int8_t *planes, float *q_last,
                              hipStream_t stream);
ssw_status launch_q8_bounds_mq(const unsigned char *codes, const float *scale, const float *err, const int8_t *planes,
                               const unsigned *mq, int32_t w, float *side, int64_t stride, float *own, int64_t n,
                               int32_t dim, int32_t *dbg_hi, int32_t *dbg_lo, int device, hipStream_t stream);
// code_bits: lb, err, scale and mx are the int8 shadow's (8), the 6-bit shadow's (6: launch_q6_bounds, launch_q6_bounds_mq) or
// the 5-bit shadow's (5: launch_q5_bounds, with the k-th key of `keys` raised by launch_exact_threshold)
ssw_status launch_survivors_mq(const float *lb, const float *err, const float *scale, const unsigned *mx, int64_t n, int32_t dim,
                               int code_bits, const uint64_t *keys, const int32_t *sel_count, int32_t k, unsigned *slot_state,
                               int64_t *rows, int64_t cap, int device, hipStream_t stream);
ssw_status launch_prune_publish_mq(const unsigned *mq, int32_t w, int64_t cap, int32_t *host_block, unsigned seq,
                                   hipStream_t stream);
// rescore_dev.hip: the exact scores (launch_scan's bits) of every certified slot's survivors in ONE launch sized by the
// device alone: slot j < w reads mq + j * Q8_MQ_WORDS and, unless it failed ([5] | [2] | [0] > cap), scores the first
// [0] rows of lists + j * list_stride for query qb_dev + j * dim straight into its slab (side + j * stride, the last
// one `own`).  rescore_survivors_waves: the waves a slot gets in that launch.  mark_uncertified: one thread ORs bit 33
// into a message's last word if the slot failed.
ssw_status launch_rescore_survivors(const void *X, int32_t dtype, const float *qb_dev, const unsigned *mq,
                                    const int64_t *lists, int64_t list_stride, int64_t cap, int32_t w, float *side,
                                    int64_t stride, float *own, int64_t n, int32_t dim, int device, hipStream_t stream);
int rescore_survivors_waves(int device, int64_t cap);
ssw_status launch_mark_uncertified(const unsigned *slot_state, int64_t cap, uint64_t *msg_last_word, hipStream_t stream);
// the tile scans on the int8 matrix core: launch_q8_bounds_mq, launch_q6_bounds, launch_q6_bounds_mq, launch_q5_bounds; scan_shape:
// blocks and 16-row tiles per request of the launch the scan's launcher would make
enum TileScan { SCAN_Q8_MQ, SCAN_Q6, SCAN_Q6_MQ, SCAN_Q5, SCAN_Q4 };  // SCAN_Q5: launch_q5_bounds, SCAN_Q4: launch_q4_bounds (below)
void scan_shape(TileScan scan, int32_t dim, int device, int64_t n, int *out_blocks, int *out_tiles);
// the packed 6-bit shadow of f32 or f16 rows (prune.hip, "6-bit shadow"): tiles of 16 rows, 3 dim / 4 bytes a row, buffers
// padded to whole tiles.  q6_slot / q6_element / q6_word_offset are the ONE placement of an element's code: k-step u, lane
// group g (the lane of row r is 16 g + r % 16) and slot j of the lane's 16 codes of that k-step; slot j < 12 is the upper
// six bits of byte j % 4 of the lane's word 3 u + j / 4, slot 12 + b the low two bits of byte b of words 3 u .. 3 u + 2
// (code bits 5:4, 3:2, 1:0); word wi of lane l sits at q6_word_offset(l, wi) in the tile.
__host__ __device__ inline void q6_slot(int i, int *u, int *g, int *j) { *u = i >> 6, *g = (i & 63) >> 4, *j = i & 15; }
__host__ __device__ inline int q6_element(int u, int g, int j) { return 64 * u + 16 * g + j; }
__host__ __device__ inline size_t q6_word_offset(int lane, int wi) {
    return (size_t)(wi >> 2) * 1024 + (size_t)lane * 16 + (size_t)(wi & 3) * 4;
}
int64_t packed_padded_rows(int64_t n);  // of both packed shadows: n rounded up to whole tiles
size_t q6_code_bytes(int64_t n, int32_t dim);
size_t q6_plane_bytes(int32_t dim);
// X: f32 rows in natural order, or binary16 rows in the f16 index's lane-interleaved layout (dtype: SSW_DTYPE_*)
ssw_status launch_q6_build(const void *X, int32_t dtype, int64_t n, int32_t dim, unsigned char *codes, float *scale,
                           float *err, hipStream_t stream);
ssw_status launch_q6_query(const float *q_dev, int32_t dim, unsigned *st, int8_t *planes, float *q_keep,
                           hipStream_t stream);
// dbg_I (lab hook only, else NULL): [n] the exact integer sums
ssw_status launch_q6_bounds(const unsigned char *codes, const float *scale, const float *err, const int8_t *planes,
                            const unsigned *st, float *scores, int64_t n, int32_t dim, int64_t *dbg_I, int device,
                            hipStream_t stream);
// the chunk of w <= 16 queries on the 6-bit shadow (prune.hip): mq and planes are the int8 chunk's buffers
// (q8_mq_plane_bytes), the slabs launch_q8_bounds_mq's; dbg_I (lab hook only, else NULL): [w, n] the exact integer sums
ssw_status launch_q6_query_mq(const float *qb_dev, int32_t dim, int32_t w, unsigned *mq, int8_t *planes, float *q_last,
                              hipStream_t stream);
ssw_status launch_q6_bounds_mq(const unsigned char *codes, const float *scale, const float *err, const int8_t *planes,
                               const unsigned *mq, int32_t w, float *side, int64_t stride, float *own, int64_t n,
                               int32_t dim, int64_t *dbg_I, int device, hipStream_t stream);
// the packed 5-bit shadow of f32 rows at dim 512 and 1024 (prune.hip, "5-bit shadow"): tiles of 16 rows, 5 dim / 8 bytes a
// row, buffers padded to whole tiles.  Lanes, k-steps and slots are the 6-bit shadow's (q6_slot / q6_element: the lane
// of row r and element i is 16 g + r % 16), and so is the place of a lane's word in the tile (q6_word_offset).  Two
// k-steps u = 2 p, 2 p + 1 share the lane's five words 5 p .. 5 p + 4 (w0 .. w4): the upper five bits of their 20 bytes
// are 20 codes, the low three bits hold the other 12.  q5_fields is the ONE placement of a code's bits, shared by the
// builder and the lab hook and mirrored by the tests' numpy twin; k_q5_bounds' unpack is its inverse:
//   k-step 2 p:     slots 0 .. 11 = bits 7:3 of w0, w1, w2;  slot 12 + b = (w0 & 7) << 2 | (w1 & 3) of byte b
//   k-step 2 p + 1: slots 0 .. 7 = bits 7:3 of w3, w4;  slot 8 + b = (w2 & 7) << 2 | (w3 & 3);
//                   slot 12 + b = (w4 & 7) << 2 | (w1 >> 2 & 1) << 1 | (w3 >> 2 & 1)
// A field: code bits [from, from + bits) sit at bits [lo, lo + bits) of byte `byte` of the lane's word `word`.
struct Q5Field {
    int word, byte, lo, bits, from;
};
__host__ __device__ inline int q5_fields(int u, int j, Q5Field (&f)[3]) {
    const int w = 5 * (u >> 1), b = j & 3;
    if ((u & 1) == 0) {
        if (j < 12) return f[0] = Q5Field{w + (j >> 2), b, 3, 5, 0}, 1;
        return f[0] = Q5Field{w, b, 0, 3, 2}, f[1] = Q5Field{w + 1, b, 0, 2, 0}, 2;
    }
    if (j < 8) return f[0] = Q5Field{w + 3 + (j >> 2), b, 3, 5, 0}, 1;
    if (j < 12) return f[0] = Q5Field{w + 2, b, 0, 3, 2}, f[1] = Q5Field{w + 3, b, 0, 2, 0}, 2;
    return f[0] = Q5Field{w + 4, b, 0, 3, 2}, f[1] = Q5Field{w + 1, b, 2, 1, 1}, f[2] = Q5Field{w + 3, b, 2, 1, 0}, 3;
}
bool q5_dim_supported(int32_t dim);
size_t q5_code_bytes(int64_t n, int32_t dim);
// X: f32 rows in natural order (dtype must be SSW_DTYPE_F32)
ssw_status launch_q5_build(const void *X, int32_t dtype, int64_t n, int32_t dim, unsigned char *codes, float *scale,
                           float *err, hipStream_t stream);
// the query's operand and state words are the 6-bit scan's (launch_q6_query); dbg_I (lab hook only, else NULL): [n] the
// exact integer sums of 8 c with 256 d_hi + d_lo
ssw_status launch_q5_bounds(const unsigned char *codes, const float *scale, const float *err, const int8_t *planes,
                            const unsigned *st, float *scores, int64_t n, int32_t dim, int64_t *dbg_I, int device,
                            hipStream_t stream);
// The exact threshold of the 5-bit path (prune.hip, "exact threshold").  keys / sel_count: what a threshold selection of
// kc >= k keys over the lower bounds left (an index without an image map: the low word of a key names its row).
// candidate_rows: rows_out[i] = the row of key i for i < the number of keys, of key 0 (row 0 without keys) beyond, kc
// entries below n, for launch_score_rows.  exact_threshold: with vals[i] the exact scores of those rows, T_x = the k-th largest
// of the first min(count, kc) that are not NaN (-inf if fewer than k are left) and keys[k - 1]'s score word becomes
// max(T_lb, T_x) in the key domain.  Nothing is changed when the selection failed (fewer than k keys or an overflow).
ssw_status launch_candidate_rows(const uint64_t *keys, const int32_t *sel_count, int32_t kc, int64_t n, int64_t *rows_out,
                                 hipStream_t stream);
ssw_status launch_exact_threshold(uint64_t *keys, const int32_t *sel_count, const float *vals, int32_t k, int32_t kc,
                                  hipStream_t stream);
// The two-plane 5-bit shadow of f32 rows at dim 512 and 1024 (prune.hip, "two-stage 4 + 1-bit shadow").  The codes c, s5
// and a5 are the 5-bit shadow's; with u = c + 16 the COARSE plane holds h = u >> 1 (a nibble) of every element in tiles of
// 16 rows, dim / 2 bytes a row, and the FINE plane b = u & 1 row-major, dim / 8 bytes a row (bit i & 31 of the row's word
// i >> 5 is b of natural element i).  Lanes, k-steps and slots of the coarse plane are the 6-bit shadow's (q6_slot), and
// so is the place of a lane's word in the tile (q6_word_offset); a lane owns two words a k-step.  q4_nibble is the ONE
// placement of a nibble, shared by the builder and the lab hook and mirrored by the tests' numpy twin: slot j of k-step u
// sits at bits [shift, shift + 4) of byte `byte` of the lane's word `word`, so that w & 0x0f0f0f0f and (w >> 4) &
// 0x0f0f0f0f of the two words are the matrix core's four operand words of the k-step.
__host__ __device__ inline void q4_nibble(int u, int j, int *word, int *byte, int *shift) {
    *word = 2 * u + (j >> 3), *byte = j & 3, *shift = 4 * ((j >> 2) & 1);
}
constexpr int64_t COARSE_CAP = (int64_t)1 << 23;  // rows of the first stage's survivor list; more: the dense refine
constexpr int Q41_STATE_WORDS = 4;                // [0] first-stage survivors, [1] 1 = the last refine was dense
size_t q41_coarse_bytes(int64_t n, int32_t dim);
size_t q41_fine_bytes(int64_t n, int32_t dim);
// coarse / fine: the two planes; scale, err, err4: s5, a5 and a4 >= ||x - s5 (2 h - 15.5)|| (+ the rounding terms of a5),
// packed_padded_rows floats each; the rows past n of the last tile get zeros
ssw_status launch_q41_build(const void *X, int32_t dtype, int64_t n, int32_t dim, unsigned char *coarse, unsigned *fine,
                            float *scale, float *err, float *err4, hipStream_t stream);
// launch_q6_query, and beside it: the sums of the two code planes into st[6], st[7] (int32), D_i = 256 d_hi,i + d_lo,i in
// natural order into D [dim], and cstate's Q41_STATE_WORDS words zeroed
ssw_status launch_q41_query(const float *q_dev, int32_t dim, unsigned *st, int8_t *planes, float *q_keep, int32_t *D,
                            unsigned *cstate, hipStream_t stream);
// the first stage: lb4 of every row into scores and H_r = sum_i h_ri D_i into H [packed_padded_rows]
ssw_status launch_q4_bounds(const unsigned char *coarse, const float *scale, const float *err4, const int8_t *planes,
                            const unsigned *st, float *scores, int32_t *H, int64_t n, int32_t dim, int device,
                            hipStream_t stream);
// its survivors against the k-th key of `keys` (raised by launch_exact_threshold): the first `list_cap` into rows32 (any
// order), their number into cstate[0]; a failed selection sets st[5].  No host wait.  blocks: 0 = the pass's own grid
ssw_status launch_survivors_q4(const float *lb4, const float *err4, const float *scale, const unsigned *mx, int64_t n,
                               int32_t dim, const uint64_t *keys, const int32_t *sel_count, int32_t k, unsigned *st,
                               unsigned *cstate, uint32_t *rows32, int64_t list_cap, int blocks, int device,
                               hipStream_t stream);
// the second stage: for the listed rows -- or, with cstate[0] > coarse_cap, for every row (dense) -- the 5-bit scan's own
// lower bound lb5 from H, the fine plane, s5 and a5, and the survivors of k_survivors_mq's test with the 5-bit width into
// rows (cap) and st[0].  dbg_lb5 / dbg_B (lab hook only, else NULL): per list entry (per row when dense)
ssw_status launch_q41_refine(const int32_t *H, const unsigned *fine, const float *scale, const float *err, const int32_t *D,
                             const uint64_t *keys, int32_t k, unsigned *st, unsigned *cstate, const uint32_t *rows32,
                             int64_t coarse_cap, int64_t n, int32_t dim, int64_t *rows, int64_t cap, float *dbg_lb5,
                             int32_t *dbg_B, int device, hipStream_t stream);
// launch_prune_publish_mq for one slot, with the first stage's count and the dense flag in host_block[2], [3]
ssw_status launch_prune_publish_q41(const unsigned *st, const unsigned *cstate, int64_t cap, int32_t *host_block,
                                    unsigned seq, hipStream_t stream);
// rows between natural order and the index.  to_h16: n rows of natural-order f32 (src_f32) or binary16 (src_h16, the
// other NULL) -> rows [0, n) of dst in the f16 layout, rounded to nearest even.  gather: rows (rows_or_null[i], or
// first_row + i when it is NULL) of an index matrix of element type dtype -> n natural-order f32 rows of out.
ssw_status launch_rows_to_h16(const float *src_f32, const uint16_t *src_h16, int64_t n, int32_t dim, uint16_t *dst,
                              hipStream_t stream);
ssw_status launch_gather_rows(const void *X, int32_t dtype, const int64_t *rows_or_null, int64_t first_row, int64_t n,
                              int32_t dim, float *out, hipStream_t stream);
// coarse.hip: out row i (i < m) = the normalised mean of the KEPT rows of image images[i] -- the rows r of
// [row_start[images[i]], row_start[images[i] + 1]) with keep[r] != 0, at least one -- summed in double in ascending row
// order, / count, / max(its double norm, 1e-6), rounded once to f32 (see coarse.hip).  X: f32 rows in natural order, or
// binary16 rows in the f16 index's layout (src_dtype); row_src_or_null: X is read through a view's row table and keep /
// row_start are in the view's numbering.  out: [m, dim] f32, or binary16 in the index layout (dst_dtype).  keep [rows],
// row_start and images [m] are device pointers.  An image's row depends on its own kept rows alone.
ssw_status launch_coarse_mean(const void *X, int32_t src_dtype, const int32_t *row_src_or_null, const unsigned char *keep,
                              const int64_t *row_start, const int64_t *images, int64_t m, int32_t dim, void *out,
                              int32_t dst_dtype, int device, hipStream_t stream);
#ifdef SSW_DEBUG_HOOKS
void tune_scan(int variant, int blocks_per_cu);
void tune_scan_batch(int max_width, int blocks_per_cu);
void tune_q8_bounds(int blocks_per_cu, int group_loads);
void tune_tile_scan(TileScan scan, int blocks_per_cu, int tiles);
#endif
// knn.hip's last stage (lives in scan.hip to share the scan's summation order)
ssw_status launch_knn_rescore(const float *X, int32_t dim, const int32_t *perm, int r0, int rows, const uint64_t *buf,
                              int cap, const unsigned *cnt, const unsigned char *overflow, int M, const float *norms,
                              float scale, float maxnorm, int k1, int32_t *out_dst, float *out_score,
                              unsigned char *out_cert, hipStream_t stream);
// gemm_bf16.hip: C[M,N] = A[M,K] W[N,K]^T (bf16 in, f32 accumulate) with fused epilogue
// epi: 0 f32 | 1 +bias -> bf16 | 2 +bias, quick-GELU -> bf16 | 3 +bias +residual -> f32
ssw_status launch_gemm_bf16_nt(int epi, hipStream_t stream, const void *A, const void *W, const float *bias,
                               const float *residual, void *C, int M, int N, int K);
#ifdef SSW_DEBUG_HOOKS
void tune_gemm(int variant);
#endif
// LayerNorm folded into a product (tile path of the CLIP towers; gemm_bf16.hip explains the algebra):
//   epi 4 / 5 (consumer):  C = rstd * (A W'^T - mean * c1) + c2 [quick-GELU] -> bf16, with A = bf16(x), W' = gamma (.) W,
//                          c2 passed as `bias`, the rows' statistics as np_in partial (sum, sum of squares) pairs
//   epi 6 (producer):      C = A W^T + bias + residual -> f32, plus its bf16 copy and the partial statistics of the
//                          128-column tile, for the next consumer
struct GemmLn {
    const float *stats_in = nullptr;  // [M][np_in][2]
    int np_in = 0;
    float inv_dim = 0.f, eps = 0.f;   // 1 / (row length of the normalised vector), LayerNorm epsilon
    const float *c1 = nullptr;        // [N]
    __bf16 *xcopy = nullptr;          // producer: [M][N] bf16 copy of the f32 output
    float *stats_out = nullptr;       // producer: [M][N / 128][2]
    int64_t res_ld = 0;               // producer (f32 rows): elements between consecutive residual rows, 0 = N (round 5: the
                                      // pooled last layer adds row b S of the stack to row b of the product)
    int xcd_contig = 0;               // 128 x 128 kernel: XCD x takes a CONTIGUOUS run of row tiles instead of x, x + 8, ...
                                      // (round 6 experiment: the rows of an image then sit in one XCD's L2 for the attention launch)
};
ssw_status launch_gemm_bf16_ln(int epi, hipStream_t stream, const void *A, const void *W, const float *bias,
                               const float *residual, void *C, int M, int N, int K, const GemmLn &ln);
// out[M][N] (f32) = A W^T + bias [+ residual] for a product of few tiles: K split over `splits` workgroups, partial
// products ([splits][M][N] f32 in `partials`) added in ascending order by a second launch
ssw_status launch_gemm_splitk_f32(hipStream_t stream, const void *A, const void *W, const float *bias, const float *residual,
                                  float *out, float *partials, int M, int N, int K, int splits);
// producer epilogue 6 (f32 row + bf16 copy + per-128-column statistics) behind a split-K product of few tiles;
// splitk_choice: how many ways such a product is worth splitting (1 = not at all)
int splitk_choice(int M, int N, int K, int cus);
ssw_status launch_gemm_splitk_stats(hipStream_t stream, const void *A, const void *W, const float *bias, const float *residual,
                                    float *out, float *partials, int M, int N, int K, int splits, const GemmLn &ln);
ssw_status launch_gemm_splitk_partials(hipStream_t stream, const void *A, const void *W, float *partials, int M, int N, int K,
                                       int splits);
// attn_out.hip: attention + out-projection (+ residual, + LayerNorm partial sums) of a ViT-B/32 layer, a workgroup per image
bool attn_outproj_supports(int S, int D, int H);
ssw_status pack_attn_outproj_weight(hipStream_t stream, const void *Wo_768x768, void *out_same_size);
// affinity_row_tiles > 0 (round 6 experiment): the qkv rows were produced by the 128-row tile kernel with
// GemmLn::xcd_contig over that many row tiles; the workgroup of image i is then launched on the XCD that produced its rows
ssw_status launch_attn_outproj(hipStream_t stream, const void *qkv, const void *Wo, const float *bo, void *xcopy,
                               const float *res_in, float *res_out, float *stats_out, int B, int S, int D, int H,
                               float scale, int affinity_row_tiles = 0);
#ifdef SSW_DEBUG_HOOKS
ssw_status read_ao_stamps(uint64_t *out, int n_words);
int gemm_variant();
// gemm_pw4.hip: the persistent four-wave kernel (256 x bn tiles, bn = 256 / 192 / 128, 0 = choose); N % 128, K % 128
bool gemm_pw4_supports(int M, int N, int K);
void gemm_pw4_set_mode(int mode);  // diagnostics of tools/perf_gemm.py (0 = the kernel)
ssw_status gemm_pw4_read_diag(unsigned long long out[6], bool reset);
ssw_status gemm_pw4_read_wg(unsigned long long *out);
ssw_status launch_gemm_pw4(int epi, hipStream_t stream, const void *A, const void *W, const float *bias,
                           const float *residual, void *C, int M, int N, int K, int bn);
#endif
// rng.hip: synthetic unit-norm rows (SSW_DTYPE_F16: the same values rounded to binary16, in the f16 index's layout)
ssw_status launch_fill_random(void *X, int32_t dtype, int64_t n, int32_t dim, uint64_t seed, int64_t first_row,
                              hipStream_t stream);

// side outputs / inputs of the selection's last kernel for the row-sharded exchange (select.hip, k_final)
struct FinalExchange {
    uint64_t *msg_out = nullptr;   // selection: this rank's message
    uint64_t image_offset = 0;     // subtracted from the keys (globalises the image position in the low word)
    int64_t row_offset = 0;        // added to the best rows
    int32_t k_max = 0, with_best = 0, msg_len = 0;
    int32_t from_msgs = 0;         // merge: the input lists are messages
    long long *flags_out = nullptr, *flags_seen = nullptr;
    // merge of a chunk of queries (launch_merge_msgs_batch): workgroup b merges query b's messages, which start
    // b * msg_len words into every rank's block; its keys go to row b of [nq, k_max], its count to word b, its flags to
    // row b of [nq, n_lists].  The single merge is the grid of one workgroup.
    // few images (<= the sort's capacity): the selection is this one kernel over all of them
    const float *values_all = nullptr;
    int64_t m_all = 0;
    const uint32_t *excl = nullptr;
    // ... which can also take the per-image maximum (values_all = row scores, row_start set; fills img_score / img_best),
    // the excluded ids as a list (device-visible pinned memory) and write the packed result into pinned host memory,
    // ending with the release of host_seq into its header word 3 (the host spins on it)
    const int64_t *row_start = nullptr;
    float *img_score = nullptr;
    uint32_t *img_best = nullptr;
    const int64_t *excl_ids = nullptr;
    int64_t n_excl = 0;
    unsigned host_seq = 0;
    int32_t sampled = 0;  // the threshold came from a sample: too few candidates is a failure, reported as overflow
};

// select.hip: exact top-k of per-image best scores.
struct SelectWorkspace {
    FinalExchange xchg;             // set by ssw_index_set_exchange_target
    // all device pointers
    uint32_t *hist1 = nullptr;      // [4096]
    uint32_t *hist2 = nullptr;      // [4096]
    uint32_t *state = nullptr;      // [16] see select.hip
    uint64_t *cand = nullptr;       // [SELECT_CAND_CAP]
    uint64_t *out_keys = nullptr;   // [SSW_MAX_TOPK]
    int32_t *out_count = nullptr;   // [1]
    uint32_t *out_best = nullptr;   // [SSW_MAX_TOPK]
    unsigned char *packed = nullptr;  // [16 + 12 k] host mirror layout: header, keys[k], best[k]
    float *img_score = nullptr;     // [n_images]   (only when row2image is set)
    uint32_t *img_best = nullptr;   // [n_images]
    uint32_t *excl_bits = nullptr;  // [(n_images+31)/32]
    int64_t *excl_ids = nullptr;    // device copy of the installed excluded-id list
    PinnedStage excl_stage;
    int64_t excl_ids_cap = 0;
    int64_t n_excluded_distinct = 0;  // distinct excluded images currently installed
    bool excl_dirty = false;          // bitmap currently has bits set
    std::vector<int64_t> excl_installed;  // the installed set, sorted: a new list costs its difference from this one
};

// where the last kernel of one selection leaves its result
struct SelectDest {
    unsigned char *host_packed = nullptr;  // pinned host block (device view) instead of ws.packed ...
    unsigned seq = 0;                      // ... whose header word 3 receives seq, released to the host
    bool message = true;                   // write the message of ws.xchg too, when a target is attached
    const FinalExchange *target = nullptr; // ... or the message of this target instead (a slot of the batch target)
};

#ifdef SSW_DEBUG_HOOKS
void tune_select(bool sampled);
#endif
ssw_status select_alloc(SelectWorkspace &ws, int64_t n_rows, int64_t n_images, bool has_map);
void select_free(SelectWorkspace &ws);
// install the excluded set (host ids) into ws.excl_bits; counts distinct ids.
ssw_status select_set_excluded(SelectWorkspace &ws, int64_t n_images, const int64_t *ids_host,
                               int64_t n, hipStream_t stream);
// per-image max over contiguous row ranges (row_start [n_images+1]).
ssw_status launch_image_max(const float *scores, const int64_t *row_start, int64_t n_images,
                            float *img_score, uint32_t *img_best, hipStream_t stream);
// top-k over values[m] (f32), skipping ids whose excl bit is set. Results in ws.out_* and where dest says.
ssw_status launch_select_topk(SelectWorkspace &ws, const float *values, int64_t m,
                              const uint32_t *best_rows_or_null, int32_t k, SelectDest dest, int device,
                              hipStream_t stream);
// small index (n_images <= SELECT_SMALL_IMAGES): per-image max, exclusion by id list, selection and the packed result
// into pinned host memory in ONE launch; the host waits for header word 3 == seq (see FinalExchange)
constexpr int64_t SELECT_SMALL_IMAGES = 8192;
ssw_status launch_select_small(SelectWorkspace &ws, const float *row_scores, const int64_t *row_start_or_null,
                               int64_t n_images, const int64_t *excl_ids_mapped, int64_t n_excl, int32_t k,
                               unsigned char *packed_mapped, unsigned seq, hipStream_t stream);
// the fast path flags (out_count[1]) a 24-bit prefix bin with more candidates than the final
// sort can take (massive exact ties); the caller then reruns the selection on the deep path.
// The final top-k of a pruned scan on an index without an image map, from its survivors (index_prune.hip): the state
// words zeroed; survivor i's exact score v[i] into scores[rows[i]] and, at or above the k-th key still in ws.out_keys and
// not excluded, its key into ws.cand; then the selection over that list alone (k_final, with dest as launch_select_topk).
ssw_status select_reset_state(SelectWorkspace &ws, hipStream_t stream);
ssw_status launch_scatter_candidates(SelectWorkspace &ws, const int64_t *rows, const float *v, int64_t m, int32_t k,
                                     float *scores, hipStream_t stream);
ssw_status launch_select_candidates(SelectWorkspace &ws, int32_t k, SelectDest dest, hipStream_t stream);
ssw_status launch_select_topk_deep(SelectWorkspace &ws, const float *values, int64_t m,
                                   const uint32_t *best_rows_or_null, int32_t k, SelectDest dest, int device,
                                   hipStream_t stream);
ssw_status launch_merge_topk(const uint64_t *keys_in, int32_t n_lists, int32_t list_stride,
                             const int32_t *counts, int32_t k, uint64_t *keys_out,
                             int32_t *count_out, hipStream_t stream);
ssw_status launch_merge_msgs(const uint64_t *msgs, int32_t world, int32_t k_max, int32_t with_best, int32_t k,
                             uint64_t *keys_out, int32_t *count_out, long long *flags_out, long long *flags_seen,
                             hipStream_t stream);
// the merge of nq queries in one launch: rank r's message for query b starts at msgs + r * rank_stride + b * msg_len;
// keys_out [nq, k_max], counts_out [nq], flags_out [nq, world]
ssw_status launch_merge_msgs_batch(const uint64_t *msgs, int32_t world, int64_t rank_stride, int32_t nq, int32_t k_max,
                                   int32_t with_best, int32_t k, uint64_t *keys_out, int32_t *counts_out,
                                   long long *flags_out, long long *flags_seen, hipStream_t stream);
ssw_status launch_gather_f32(const float *src, const int64_t *idx_dev, int64_t n, float *dst,
                             hipStream_t stream);

constexpr int SSW_RANK_MAX_ITEMS = 65536;    // rank.hip: items of one counting launch (O(n^2) compares)

// rank.hip: quick zero-margin pairwise gradient on device-resident targets / scores (feedback engine)
ssw_status launch_rank_quick(const float *target_dev, const float *scores_dev, int n, float *grad_dev,
                             float *maxrev_dev_or_null, unsigned long long *total_dev_or_null, hipStream_t stream);

// rescore.hip: avg_score aggregation of candidate images' tiles (score_frame2 / box_join).
constexpr int SSW_RESCORE_MAX_TILES = 2048;  // tiles of one image held in LDS (32 B each with f32 scores, 40 B with f64)
constexpr int SSW_RESCORE_MAX_ZOOM = 31;     // zoom levels index a 32-bit presence mask
ssw_status launch_avg_score(const float *boxes, const int32_t *zoom, const float *scores, const float *minus_or_null,
                            const int64_t *row_start, const int64_t *cand_pos, const int64_t *cand_off, int32_t m,
                            int32_t max_tiles, int32_t aug, float *out_score, int64_t *out_row, hipStream_t stream);
// the same aggregation for the result slots of the selection that has just run on `stream` (keys / count as in
// SelectWorkspace): k workgroups, slot c < count writes out_score[c] / out_row[c]; max_tiles = the most tiles of any
// image of the index
ssw_status launch_avg_score_keys(const float *boxes, const int32_t *zoom, const float *scores, const int64_t *row_start,
                                 int64_t n_images, const uint64_t *keys, const int32_t *count, int32_t k,
                                 int32_t max_tiles, int32_t aug, float *out_score, int64_t *out_row, hipStream_t stream);
// the same aggregation on the owners of a sharded batch's merged candidates (k_avg_score_owner): grid (k, nq); workgroup
// (c, b) decodes the GLOBAL image position of keys[b * k_max + c] (c < counts[b]), and if this index holds it -- the
// positions [image_offset, image_offset + n_images) -- scores the image's tiles for query qb + b * dim straight from the
// rows X (launch_scan's bits) and aggregates them.  out [nq, 2, k_max] u64: [b, 0, c] = 1 << 32 | f32 bits of the score,
// [b, 1, c] = row_offset + the best tile's row; both 0 where the image is not this index's.  Every c < k is written.
struct AvgOwnerArgs {
    const float *qb;  // [nq, dim] device
    const float *boxes;
    const int32_t *zoom;
    const int64_t *row_start;
    int64_t n_images;
    const uint64_t *keys;
    const int32_t *counts;
    int32_t nq, k_max, k, max_tiles, aug;
    int64_t image_offset, row_offset;
    uint64_t *out;
};
ssw_status launch_avg_score_owner(const void *X, int32_t dtype, int32_t dim, const AvgOwnerArgs &args, hipStream_t stream);
// the second stage of a batch of two-vector queries (k_pair_score): grid (k, nq); workgroup (c, b), c < counts[b], scores
// the tiles of image pos[b * k + c] straight from the rows X for qb + b * dim and for q2b + b * dim, takes the
// difference and aggregates it -- avg: as launch_avg_score with the minus form (aug: its code), plain: the first tile
// with the highest non-NaN difference.  out_score / out_row [nq, k]; slots at or past counts[b] are not written.
// boxes / zoom may be NULL for plain.  max_tiles = the most tiles of any image of the index.
struct PairScoreArgs {
    const float *qb, *q2b;  // [nq, dim] device
    const float *boxes;
    const int32_t *zoom;
    const int64_t *row_start;
    int64_t n_images;
    const int64_t *pos;     // [nq, k] device
    const int32_t *counts;  // [nq] device
    int32_t nq, k, max_tiles, aug;
    bool avg;
    float *out_score;
    int64_t *out_row;
};
ssw_status launch_pair_score(const void *X, int32_t dtype, int32_t dim, const PairScoreArgs &args, hipStream_t stream);
// the rows those two launches read, as row lists for launch_score_rows: candidate c's tiles at rows_out[cand_off[c] ..)
// (the candidates' tile total entries); slot c's at rows_out[c * max_tiles ..), padded with rows of the index to
// k * max_tiles entries in all
ssw_status launch_candidate_tiles(const int64_t *row_start, const int64_t *cand_pos, const int64_t *cand_off, int32_t m,
                                  int64_t *rows_out, hipStream_t stream);
ssw_status launch_candidate_tiles_keys(const int64_t *row_start, int64_t n_images, const uint64_t *keys,
                                       const int32_t *count, int32_t k, int32_t max_tiles, int64_t *rows_out,
                                       hipStream_t stream);
// the same aggregation over float64 scores that live on the device (label-propagation output)
ssw_status launch_avg_score_f64(const float *boxes, const int32_t *zoom, const double *scores,
                                const int64_t *row_start, const int64_t *cand_pos, const int64_t *cand_off, int32_t m,
                                int32_t max_tiles, int32_t aug, double *out_score, int64_t *out_row, hipStream_t stream);

}  // namespace ssw

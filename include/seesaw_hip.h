/*
 * seesaw_hip.h -- C-ABI of libseesaw_hip.so, the MI355X (gfx950) hot path behind
 * seesaw's Python API surface.
 *
 * The reference (orm011/seesaw) has no FFI: its boundary is a duck-typed Python
 * interface whose numeric work is delegated to numpy / scipy / torch-CPU.  Every
 * entry point below replaces one of those numeric call sites; the reference
 * file:line each one stands in for is cited next to it (paths relative to the
 * reference root).  The Python mirror of the reference interface that binds
 * these symbols lives in seesaw_amd/ (see INTEGRATION.md for the ctypes stub a
 * reference maintainer would add).
 *
 * Conventions
 *   - plain pointers and sizes only; no torch / numpy types cross this boundary;
 *   - every function returns ssw_status: 0 = OK, <0 = error, and the failing
 *     thread can read a message with ssw_last_error();
 *   - "host" pointers are ordinary process memory, "dev" pointers are HIP device
 *     memory on the handle's device (e.g. torch.Tensor.data_ptr());
 *   - a handle is bound to one device and one HIP stream and is NOT thread-safe:
 *     the same serial-per-session model the reference uses
 *     (seesaw/web/web_session_actor.py:13-16);
 *   - functions with a host-side result synchronise the handle's stream before
 *     returning; the *_dev / *_async forms only enqueue work.
 */
#ifndef SEESAW_HIP_H
#define SEESAW_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int32_t ssw_status;
#define SSW_OK 0
#define SSW_ERR_INVALID (-1)     /* bad argument                                  */
#define SSW_ERR_HIP (-2)         /* a HIP runtime call failed                     */
#define SSW_ERR_NOMEM (-3)       /* device or host allocation failed              */
#define SSW_ERR_UNSUPPORTED (-4) /* shape / size outside what the kernels support */
#define SSW_ERR_NUMERIC (-5)     /* NaN / bound violation the reference asserts on */

#define SSW_ABI_VERSION 1
#define SSW_MAX_TOPK 4096        /* largest k ssw_index_topk accepts               */

int32_t ssw_abi_version(void);
const char *ssw_last_error(void);
ssw_status ssw_device_count(int32_t *out_count);
/* name / CU count / HBM bytes of a device, for bench reports. name_cap >= 64. */
ssw_status ssw_device_info(int32_t device, char *name, int32_t name_cap, int32_t *out_cus,
                           int64_t *out_hbm_bytes);

/* ------------------------------------------------------------------------- */
/* Vector index: resident [N, d] f32 matrix + brute-force cosine scan + top-k */
/* replaces: vectors @ q ; np.argsort(-scores)                                */
/*   seesaw/indices/multiscale/multiscale_index.py:170-175 (_get_top_exact)   */
/*   seesaw/indices/multiscale/multiscale_index.py:177-199 (_get_top_dbidxs)  */
/*   seesaw/indices/coarse/coarse_index.py:57-96 (CoarseIndex.query)          */
/*   seesaw/vector_index.py:44-60 (VectorIndex.query)                         */
/* ------------------------------------------------------------------------- */
typedef struct ssw_index ssw_index;

/* dev_vectors_or_null: borrow an existing device matrix (row-major, 16-byte
 * aligned, must outlive the handle); NULL -> the handle allocates n_rows*dim*4
 * bytes itself.  dim must be a multiple of 256 and <= 1024 (CLIP: 512). */
ssw_status ssw_index_create(int32_t device, int64_t n_rows, int32_t dim,
                            const float *dev_vectors_or_null, ssw_index **out);
/* Element type of the resident matrix.  SSW_DTYPE_F16 stores every element as IEEE binary16, rounded to nearest
 * even (subnormals kept, overflow to +-inf: numpy's astype(float16)), in a private lane-interleaved row layout
 * (dim * 2 bytes a row).  Every operation on an f16 index returns the bits the same operation returns on an f32 index
 * of the widened rows: the query stays f32, products and sums are f32 in the f32 scan's order.  A large f16 index
 * prunes its single-query top-k like an f32 index (ssw_index_prune_stats: the int8 shadow is built from the widened
 * rows, from 2^22 rows on, as for f32 rows).  Entries that read the matrix as f32 through the handle and have no f16
 * form (ssw_knn_build, ssw_xlx) return SSW_ERR_UNSUPPORTED; ssw_index_device_ptrs hands out the private layout. */
#define SSW_DTYPE_F32 0
#define SSW_DTYPE_F16 1
/* ssw_index_create with an element type.  SSW_DTYPE_F32 is ssw_index_create; SSW_DTYPE_F16 allocates
 * n_rows*dim*2 bytes and cannot borrow a device matrix (dev_vectors_or_null != NULL -> SSW_ERR_UNSUPPORTED). */
ssw_status ssw_index_create_typed(int32_t device, int64_t n_rows, int32_t dim, int32_t dtype,
                                  const void *dev_vectors_or_null, ssw_index **out);
ssw_status ssw_index_dtype(const ssw_index *idx, int32_t *out);
ssw_status ssw_index_destroy(ssw_index *idx);

/* A zero-copy VIEW of a resident index: a handle over the rows of m member images that scans them IN PLACE, out of the
 * parent's matrix (AccessMethod.subset(BitMap) of the reference, seesaw/seesaw_session.py:216-225, without the host
 * gather and the second upload a copied subset index costs).  image_positions [m] (host): parent image positions --
 * row positions for a parent without an image map -- strictly ascending, inside the parent, m >= 1; anything else is
 * SSW_ERR_INVALID, decided on the host before any device call, as are a NULL parent, NULL positions and a NULL out.
 * The view is an ordinary ssw_index of n_rows = the members' rows (in the parent's order) and n_images = m, with the
 * parent's dim, dtype and device; it owns a row table (4 bytes a row), a score buffer, streams, a selection workspace,
 * staging and -- when the parent has an image map -- the image map of its members, and takes its own tile meta
 * (ssw_index_set_tile_meta).  Rows, image positions and results are the VIEW's: what a copied subset index of
 * X[member rows] returns, bit for bit (the scan runs the parent's lane arithmetic on the member rows).  It reads the
 * parent's current rows: an ssw_index_upload into the parent shows in the view's next scan.  A view is never pruned
 * and builds no shadow.
 * Work on a view: shape, dtype, set_stream, sync, scan, scan_dev, load_scores, topk (small and general form),
 * set_excluded, topk_dev, select_deep_dev, result_ptrs, topk_fetch, gather_scores, set_tile_meta, rescore_avg,
 * rescore_avg_f64, profile, profile_read, prune_stats / prune_completions ("not pruned"), ssw_labelprop_scores_to_index,
 * ssw_labelprop_round, and the batched entries of its own, ssw_index_view_scan_batch / _view_topk_batch /
 * _view_topk_batch_avg; ssw_index_device_ptrs hands out the view's score buffer and a NULL row pointer;
 * ssw_index_score_rows, ssw_index_gather_rows and ssw_fb_set_data_from_index take VIEW rows and translate them;
 * ssw_index_coarse_mean reads a view as its SOURCE through the row table (and refuses one as its destination).
 * Refused on a view with SSW_ERR_UNSUPPORTED (the message says "view") before anything is touched: upload, upload_f16,
 * download, fill_random, set_row2image, every *_batch* entry without `view_` in its name, topk_slot_deep_dev, stage2_avg_batch_dev, both exchange
 * target setters, ssw_knn_build, ssw_xlx, ssw_fb_set_pseudo_sample_from_index, and a view of a view.
 * Lifetime: the parent counts its live views; ssw_index_destroy(parent) with live views is SSW_ERR_INVALID and leaves
 * the parent intact.  Destroy the views first.  A view's members are the rows the parent's image map gave those images
 * when the view was made, so ssw_index_set_row2image(parent) with live views is SSW_ERR_INVALID too; the parent's ROWS
 * may change under a view (ssw_index_upload).
 * ssw_index_view_rows: the parent row of every view row, out_parent_rows_host [n_rows] (SSW_ERR_INVALID if the handle
 * is not a view). */
ssw_status ssw_index_create_view(ssw_index *parent, const int64_t *image_positions, int64_t m, ssw_index **out);
ssw_status ssw_index_view_rows(const ssw_index *view, int64_t *out_parent_rows_host);
/* run all of this handle's work on an existing hipStream_t (e.g. torch's current
 * stream) instead of the handle's own (non-blocking) stream.  NULL restores the own stream; to name the
 * default stream -- whose handle IS NULL, e.g. torch.cuda.current_stream().cuda_stream == 0 -- pass
 * hipStreamLegacy ((hipStream_t)1). */
ssw_status ssw_index_set_stream(ssw_index *idx, void *hip_stream);
ssw_status ssw_index_sync(ssw_index *idx);
ssw_status ssw_index_shape(const ssw_index *idx, int64_t *n_rows, int32_t *dim, int64_t *n_images);
/* device pointers of the resident matrix and of the score buffer ([n_rows] f32,
 * valid after the last scan).  After a pruned top-k (ssw_index_prune_stats) this first completes the score buffer with
 * the full scan of that query.  Handing out dev_vectors ends the index's int8 shadow for good: the caller may write
 * the rows through it. */
ssw_status ssw_index_device_ptrs(ssw_index *idx, void **dev_vectors, void **dev_scores);

/* copy rows [first_row, first_row+n) from host memory into the index (an f16 index rounds them on the device,
 * through a bounded staging buffer). */
ssw_status ssw_index_upload(ssw_index *idx, const float *host_rows, int64_t first_row, int64_t n);
/* the same from rows that are already binary16 (natural element order); f16 index only, else SSW_ERR_UNSUPPORTED. */
ssw_status ssw_index_upload_f16(ssw_index *idx, const uint16_t *rows_f16, int64_t first_row, int64_t n);
/* copy rows back as f32 (tests / subset(); an f16 index widens them). */
ssw_status ssw_index_download(ssw_index *idx, float *host_rows, int64_t first_row, int64_t n);
/* fill the whole index on the device with the counter-based synthetic generator
 * (unit-norm rows; bit-identical to oracle.synth_rows(seed, global_first_row+i)). */
ssw_status ssw_index_fill_random(ssw_index *idx, uint64_t seed, int64_t global_first_row);

/* The coarse (one vector per image) rows out of a resident multiscale index, on the device: infer_coarse_embedding of
 * the reference (seesaw/indices/coarse/preprocessor.py:11-19: the rows with zoom_level == max_zoom_level,
 * groupby("dbidx").vectors.mean(), / np.maximum(norm, 1e-6)), the one way it builds a CoarseIndex (from_fine_grained,
 * preprocessor.py:22-52).  keep_host [src n_rows]: != 0 marks a kept row; images_host [m]: positions in src's image map,
 * strictly ascending.  Row i of dst becomes, for image images_host[i] with kept rows r_1 < ... < r_c:
 *   s = x[r_1] + ... + x[r_c] in double in ascending row order (binary16 rows widened exactly), mean = s / c,
 *   dst[i] = (float)(mean / max(||mean||, 1e-6)), norm and divisions in double, ONE rounding to f32 (an f16 dst rounds
 *   that f32 to binary16, nearest even).
 * An image's row depends on its own kept rows alone: not on m, on the other listed images or on the device.
 * src: needs an image map (else SSW_ERR_UNSUPPORTED); f32, f16 or a view (keep_host and images_host are then in the
 * VIEW's numbering).  dst: an index of n_rows == m and src's dim on src's device, of either dtype, not a view
 * (SSW_ERR_UNSUPPORTED, the message says "view"), not src and not src's parent.  The work is enqueued on src's stream
 * and the call returns when it is done; dst's rows then count as changed exactly as after ssw_index_upload (its shadows
 * are stale, its score buffer is completed first and is not partial).
 * SSW_ERR_INVALID, like every refusal decided on the host before anything is enqueued: positions not strictly ascending
 * or outside the map, a listed image without a kept row, dst of another shape or device, a NULL pointer.
 * Device memory: n_rows mask bytes and 8 m bytes of positions for the duration of the call, nothing afterwards.
 * ssw_index_profile(src) records one event pair around the kernel. */
ssw_status ssw_index_coarse_mean(ssw_index *src, const uint8_t *keep_host, const int64_t *images_host, int64_t m,
                                 ssw_index *dst);

/* row -> image map (vector_meta.dbidx of the reference, multiscale_index.py:192):
 * host array [n_rows] int32, non-decreasing, values are *positions* 0..n_images-1 of
 * the distinct images in ascending dbidx order.  NULL -> identity (one vector per
 * image, CoarseIndex). */
ssw_status ssw_index_set_row2image(ssw_index *idx, const int32_t *row2image_host, int64_t n_images);

/* scores = vectors @ q   (index.score(): multiscale_index.py:284-285, coarse_index.py:37-38).
 * Leaves the scores resident on the device; out_host may be NULL. */
ssw_status ssw_index_scan(ssw_index *idx, const float *q_host, float *out_scores_host_or_null);
/* same, q already on the device, nothing copied back, no synchronisation. */
ssw_status ssw_index_scan_dev(ssw_index *idx, const float *q_dev);

/* replace the resident per-row scores with caller-supplied ones ([n_rows] f32, -inf = skip the
 * row); a following ssw_index_topk(q_host = NULL) then ranks images by them.  Used to rank by
 * label-propagation scores (KnnProp2.next_batch, seesaw/loops/graph_based.py:88-109). */
ssw_status ssw_index_load_scores(ssw_index *idx, const float *scores_host);

/* Top-k distinct images by their best-scoring row, skipping excluded images:
 * _get_top_exact + _get_top_dbidxs (multiscale_index.py:170-199).  Order: score
 * descending, ties by ascending image position.  q_host==NULL reuses the resident
 * scores of the previous scan.  excluded = image positions (any order, may repeat).
 * Outputs (host, capacity k): image position, its max score, the row that attains it
 * (lowest row on ties).  *out_count = min(k, #non-excluded images). */
ssw_status ssw_index_topk(ssw_index *idx, const float *q_host, const int64_t *excluded_images,
                          int64_t n_excluded, int32_t k, int64_t *out_images, float *out_scores,
                          int64_t *out_best_rows, int32_t *out_count);
/* Several queries in ONE pass over the rows.  The scan is bound by HBM: a row that sits in registers for one query
 * scores a second, a fourth, a sixteenth one for almost no extra traffic.  From 65 536 rows on (f32 and f16 rows,
 * every dim) a batch is cut into chunks of the width with the lowest measured time per query for the shape -- f32 / f16
 * rows: 16 / 16 queries at dim 256, 16 / 8 at dims 512 and 768, 8 / 8 at dim 1024 --, the remainder into chunks of 8,
 * 4 and 2 and at last a single query, and every chunk is one launch of the multi-query scan kernel; smaller indexes
 * are served by one single-query scan launch per query.  Either way query b's scores are the BITS ssw_index_scan
 * returns for q[b].  Any nq >= 1; nq == 1 IS the single-query call.
 *
 * ssw_index_scan_batch: scores[b, :] = vectors @ q[b].  q_host [nq, dim], out_scores_host [nq, n_rows] (may be NULL:
 * nothing is copied back).  Afterwards the resident scores are those of the LAST query, as after ssw_index_scan(q[nq-1]).
 *
 * ssw_index_topk_batch: ssw_index_topk for nq queries.  Query b's excluded images are
 * excluded_images[excluded_offsets[b] .. excluded_offsets[b+1]) (excluded_offsets [nq + 1]; NULL: no exclusions).
 * Outputs are [nq, k] row-major (row b filled up to out_counts[b]); out_counts [nq].  Query b's row is exactly what
 * ssw_index_topk(idx, q[b], its excluded list, k) returns -- images, best rows, score bits and count, the mass-tie
 * case through the deep selection included.  One selection and one host wait per query.
 * State afterwards: that of ssw_index_topk with the last query and its excluded list after a full scan -- the resident
 * scores, the installed excluded set and the device result buffers are the last query's, so ssw_index_topk(q = NULL),
 * ssw_index_gather_scores, ssw_index_rescore_avg and ssw_index_result_ptrs refer to it.
 * Pruning (ssw_index_prune_stats): a batch of nq >= 2 always runs the full-precision scan; it never reads or builds
 * the int8 shadow and leaves the prune counters alone.  It first completes a partial score buffer: right after a pruned
 * single top-k that is one full scan of the previous query (31 ms at 100 M rows) before the batch starts.
 * Measured on one MI355X ("Batched scan"; k = 100): one launch costs 1.04-1.07 x a single-query
 * scan at 2 queries, 1.08-1.17 x at 4, 1.14-1.20 x (f32) at 8 and 1.57-1.68 x (f32) at 16.  Per query, against single
 * calls that scan in full (below 2^22 rows, or a borrowed matrix), topk_batch takes
 * 0.52-0.62 x at nq = 2, 0.27-0.40 x at 4, 0.15-0.32 x at 8 and, f32, 0.10-0.17 x at 16 (the f16 figures were taken
 * against the f16 full scan at every size).  Where the single call is PRUNED (measured for f32, >= 2^22 rows) the
 * crossover is nq = 4: the batch is slower at nq = 2 (16.3 against 8.4 ms per query at 100 M rows), equal at 4 (8.46
 * against 8.42; 1.17 against 1.19 at 12.5 M), faster from 8 on (4.6, and 3.2 at 16, against 8.4; 0.67 and 0.49 against
 * 1.20).  Callers choose; nothing dispatches silently.
 * Memory: the scores of a chunk's last query go to the handle's own buffer, the others to a side buffer of at most
 * 15 x n_rows x 4 bytes (7 x for f16 rows) allocated by the first batched call and sized by the widest chunk it
 * needed; if it cannot be allocated the call falls back to narrower chunks and in the end to one query at a time -- it
 * does not fail.
 * Errors, both before anything is enqueued: a non-finite component in any query is SSW_ERR_NUMERIC (the message
 * names the query and the component); nq < 1, a NULL pointer, decreasing offsets or an excluded id out of range are
 * SSW_ERR_INVALID.  ssw_index_profile records one event pair per scan launch, batched or not. */
ssw_status ssw_index_scan_batch(ssw_index *idx, const float *q_host, int32_t nq, float *out_scores_host);
ssw_status ssw_index_topk_batch(ssw_index *idx, const float *q_host, int32_t nq, const int64_t *excluded_images,
                                const int64_t *excluded_offsets, int32_t k, int64_t *out_images, float *out_scores,
                                int64_t *out_best_rows, int32_t *out_counts);

/* ssw_index_topk_batch with the certified int8 pre-scan (ssw_index_prune_stats) shared by a chunk of up to 16 queries:
 * arguments, results, errors and the deep-selection case exactly as ssw_index_topk_batch; every query's row is the
 * bits of ssw_index_topk for it.  On an index the single call would prune (own rows, dim 256 / 512 / 1024, at least
 * 2^22 rows, the shadow not refused for memory) a chunk is ONE pass over the int8 shadow on the int8 matrix core
 * (v_mfma_i32_16x16x64_i8: the queries are quantised to two int8 planes, the integer sums are exact) that writes a
 * certified lower bound of every row for every query; per query a threshold selection, the survivors and their exact
 * rescoring follow, with ONE host wait per chunk, and then the ordinary selection.  A query that cannot be bounded (zero,
 * norm above 2^40, largest element outside [2^-60, 2^60]), one with more than 2^18 survivors or fewer than k keys runs
 * the full scan by itself.  Any other index takes ssw_index_topk_batch itself and leaves the prune counters alone.
 * On an index of at least 25 M rows, f32 or f16, whose single queries scan the packed 6-bit shadow (that shadow not
 * refused for memory) the chunk's pass runs over that shadow instead, 3 dim / 4 + 8 bytes a row, and no int8 shadow is
 * built: one shadow serves both kinds of call.  The same holds for ssw_index_topk_batch_avg_pruned and
 * ssw_index_topk_batch_dev_pruned.  Which shadow certifies never changes what is returned.
 * A dim-768 index has the packed 6-bit shadow only (584 bytes a row; there is no int8 shadow at that dim): its pruned
 * batches scan it from 2^20 rows on (ssw_index_prune_stats) and are ssw_index_topk_batch itself below that count or
 * when the shadow is refused for memory.
 * State afterwards: that of a pruned ssw_index_topk of the last query with its excluded list (the resident scores are
 * completed by the first reader).  ssw_index_prune_stats counts every query of a pruned batch in [3] and every one that
 * fell back in [4]; [2] is the last query's.  ssw_index_profile records one event pair per chunk.
 * Memory: the side buffer of ssw_index_topk_batch at up to 15 slabs (f16 rows too) and 16 survivor lists of 3 MiB; a
 * failed allocation narrows the chunk.  Opt-in: nothing dispatches to it silently. */
ssw_status ssw_index_topk_batch_pruned(ssw_index *idx, const float *q_host, int32_t nq, const int64_t *excluded_images,
                                       const int64_t *excluded_offsets, int32_t k, int64_t *out_images,
                                       float *out_scores, int64_t *out_best_rows, int32_t *out_counts);

/* device-resident form used by bench.py and the sharded index: q_dev [dim] f32;
 * the excluded set is whatever the last ssw_index_set_excluded installed; results
 * stay on the device in the handle's result buffers (ssw_index_result_ptrs).
 * Enqueues only. */
ssw_status ssw_index_set_excluded(ssw_index *idx, const int64_t *excluded_images, int64_t n_excluded);
ssw_status ssw_index_topk_dev(ssw_index *idx, const float *q_dev, int32_t k);
/* device result buffers of the last topk: keys [SSW_MAX_TOPK] u64 =
 * (orderable(score) << 32) | (0xFFFFFFFF - image), sorted descending; count [2] i32 = {number of keys,
 * overflow flag}; best_rows [SSW_MAX_TOPK] u32.  overflow != 0: more than 8192 images share the 24-bit score
 * prefix of the k-th score (duplicated vectors) and the keys are NOT the exact top-k -- rerun with
 * ssw_index_select_deep_dev (ssw_index_topk / ssw_index_topk_fetch do that by themselves). */
ssw_status ssw_index_result_ptrs(ssw_index *idx, void **dev_keys, void **dev_count,
                                 void **dev_best_rows);
/* exact selection over the resident scores for the mass-tie case (host-synchronised radix descent over the
 * full 64-bit composite key); leaves keys / count / best_rows in the same buffers, overflow cleared.
 * No reference counterpart: np.argsort sorts all N keys (multiscale_index.py:171-172). */
ssw_status ssw_index_select_deep_dev(ssw_index *idx, int32_t k);
/* read the last device-side result back (synchronises). */
ssw_status ssw_index_topk_fetch(ssw_index *idx, int32_t k, int64_t *out_images, float *out_scores,
                                int64_t *out_best_rows, int32_t *out_count);

/* scores of arbitrary rows from the resident score buffer (stage-2 rescoring of
 * the candidate images' tiles, multiscale_index.py:341-345). */
ssw_status ssw_index_gather_scores(ssw_index *idx, const int64_t *rows_host, int64_t n,
                                   float *out_scores_host);

/* the vectors of arbitrary rows, [n, dim] f32 (`index.vectors[rows]`: the labelled tiles the fitting loops read,
 * seesaw/loops/multi_reg.py:204, loops/util.py:6,11), out of the resident matrix. */
ssw_status ssw_index_gather_rows(ssw_index *idx, const int64_t *rows_host, int64_t n, float *out_host);

/* scores of arbitrary rows against another vector, in the scan's summation order
 * (`vectors[ilocs] @ vector2`, multiscale_index.py:347-349). */
ssw_status ssw_index_score_rows(ssw_index *idx, const float *q_host, const int64_t *rows_host,
                                int64_t n, float *out_scores_host);

/* ------------------------------------------------------------------------- */
/* Second stage of the multiscale lookup: `avg_score` aggregation on the device */
/* replaces: score_frame2 (both aug_weight modes) + box_join as driven by        */
/*           rescore_candidates   seesaw/indices/multiscale/multiscale_index.py */
/*           :112-150, 379-403;   seesaw/box_utils.py:336-372                   */
/* ------------------------------------------------------------------------- */
/* tile geometry of every row: boxes [n_rows, 4] f32 = x1, y1, x2, y2 (vector_meta's columns, original-image
 * pixels) and zoom_level [n_rows] i32 in [0, 31]. */
ssw_status ssw_index_set_tile_meta(ssw_index *idx, const float *boxes_host, const int32_t *zoom_host);
/* for each of m candidate images (positions as returned by ssw_index_topk): tile i's score := mean over zoom
 * levels of the score of the best-overlapping (IoU > 0, first maximum) tile of that level, levels restricted by
 * aug_larger (0 'all', 1 'greater': partner level >= own, 2 'adjacent': partner level == own); the image is
 * represented by its first tile with the highest aggregated score.  Tile scores are the ones the last scan left
 * on the device, minus minus_scores (optional; one value per candidate tile, candidates in the given order, tiles
 * in row order: the `vector2` form, multiscale_index.py:347-349).  IoU in f32 as torchvision forms it, mean as
 * pandas' float32 group mean (Kahan sum): bit-identical to the reference on identical tile scores.
 * aug_larger + 4 selects aug_weight = 'cont_weighted' (multiscale_index.py:133-145): tile i's score := softmax over
 * ALL its joined partners of the containment inter / area_i, dotted with the partners' scores (f32; 1e-6 of the
 * reference, whose dot runs in BLAS order). */
ssw_status ssw_index_rescore_avg(ssw_index *idx, const int64_t *image_positions, int32_t m, int32_t aug_larger,
                                 const float *minus_scores_or_null, float *out_scores, int64_t *out_best_rows);
/* the same aggregation over float64 tile scores that live on the device, one per index row (the output of
 * ssw_labelprop_run_resident: ssw_labelprop_device_scores) -- what the graph loops' own rescoring does with the
 * propagated scores (`fullmeta.assign(score=scores[rows])` then rescore_candidates, seesaw/loops/graph_based.py:100-108):
 * mean = pandas' float64 group mean (Kahan sum in f64), IoU in f32 as above. */
ssw_status ssw_index_rescore_avg_f64(ssw_index *idx, const double *dev_scores, const int64_t *image_positions, int32_t m,
                                     int32_t aug_larger, double *out_scores, int64_t *out_best_rows);

/* Both stages of the multiscale lookup for nq queries: ssw_index_topk_batch, and for every query the aggregation of
 * ssw_index_rescore_avg over the images it selected, read from the query's OWN score slab while the chunk is alive (a
 * batch leaves only its last query's scores resident, so the single entry cannot follow it).
 * First stage: arguments, results, errors, chunking, the side buffer and the state afterwards are exactly those of
 * ssw_index_topk_batch -- the full-precision scan for nq >= 2; nq == 1 IS ssw_index_topk, pruning included, after
 * which the tiles of the selected images are rescored exactly into the partial score buffer (as in
 * ssw_index_topk_batch_avg_pruned below; the buffer stays partial).
 * Second stage: after query b's selection has been collected (so after a deep rerun too) one launch of one workgroup
 * per result slot takes its candidates from the handle's device result buffers (ssw_index_result_ptrs) and the tile
 * scores from slab b, on the same stream, before the next query's selection overwrites those buffers; no candidate
 * list travels to the host and back.  A chunk's results come back in one copy per array and ONE host wait.
 * out_avg_scores / out_avg_rows [nq, k]: entry [b, i], i < out_counts[b], belongs to out_images[b, i] and holds the
 * bits ssw_index_rescore_avg returns for that image when q[b]'s scores are resident (no minus form); entries from
 * out_counts[b] on are unspecified.  aug_larger: that entry's codes, 0 / 1 / 2, optionally + 4.
 * Errors, before anything is enqueued: no row map or tile meta, a bad aug_larger or an image of more than 2048 tiles
 * ANYWHERE in the index are SSW_ERR_INVALID -- index-wide, because the candidates are not known to the host at launch
 * (ssw_index_rescore_avg checks the images it is given only).
 * Memory: the first call adds two device arrays of 16 x SSW_MAX_TOPK entries (f32 + i64: 768 KiB). */
ssw_status ssw_index_topk_batch_avg(ssw_index *idx, const float *q_host, int32_t nq, const int64_t *excluded_images,
                                    const int64_t *excluded_offsets, int32_t k, int32_t aug_larger, int64_t *out_images,
                                    float *out_scores, int64_t *out_best_rows, float *out_avg_scores,
                                    int64_t *out_avg_rows, int32_t *out_counts);
/* ssw_index_topk_batch_avg with the first stage of ssw_index_topk_batch_pruned: arguments, results, errors and the
 * state afterwards as there, every output the bits of ssw_index_topk_batch_avg.  A pruned slab is exact on the query's
 * survivors only, and the aggregation reads the tiles of the k selected images and nothing else: after query b's
 * selection has been collected, one launch lists those tiles from the device result buffers (one workgroup a slot,
 * k x T entries, T = the most tiles of any image, short images padded with their first row), the rows are scored
 * exactly with q[b] by gather and scattered into slab b, then the aggregation runs as above.  A slot whose first stage
 * fell back holds the full scan already; where k x T exceeds 2^18 the slab is completed by the full scan of q[b]
 * (counted in ssw_index_prune_completions [0]).  nq == 1 is ssw_index_topk followed by the same steps on the handle's
 * buffer.  An index that is not pruned, or whose int8 shadow is refused, takes ssw_index_topk_batch_avg itself and
 * leaves every prune counter alone.  Opt-in: nothing dispatches to it silently. */
ssw_status ssw_index_topk_batch_avg_pruned(ssw_index *idx, const float *q_host, int32_t nq, const int64_t *excluded_images,
                                           const int64_t *excluded_offsets, int32_t k, int32_t aug_larger,
                                           int64_t *out_images, float *out_scores, int64_t *out_best_rows,
                                           float *out_avg_scores, int64_t *out_avg_rows, int32_t *out_counts);

/* The batched scan, top-k and two-stage top-k of a VIEW (ssw_index_create_view): ssw_index_scan_batch,
 * ssw_index_topk_batch and ssw_index_topk_batch_avg over the member rows, read in place out of the parent's matrix
 * ONCE per chunk of queries (the multi-query scan with the view's row table, 4 more bytes a row a chunk).  Signatures,
 * validation, per-query exclusion lists, chunk widths, the deep rerun on mass ties, out_counts, the side buffer and the
 * errors are those of the plain entries; a view of fewer than 65 536 rows is served by one single-query scan of the
 * view per query.  Query b's outputs are the bits of the view's ssw_index_scan / ssw_index_topk (/ ssw_index_rescore_avg
 * over the view's own tile meta) for q[b], which are those of a copied subset index of the member rows.  There is no
 * pruned form: a view holds no shadow.  State afterwards: that of ssw_index_topk on the view with the last query --
 * its resident scores are the last query's and are not partial.  The side slabs and the query block belong to the view
 * handle and go with it in ssw_index_destroy; the parent is read only, and sees nothing of the call.
 * Each entry takes a view only: any other handle is SSW_ERR_INVALID (the message names the entry), as are NULL
 * arguments, before anything is touched.  The plain entries keep refusing a view. */
ssw_status ssw_index_view_scan_batch(ssw_index *view, const float *q_host, int32_t nq, float *out_scores_host);
ssw_status ssw_index_view_topk_batch(ssw_index *view, const float *q_host, int32_t nq, const int64_t *excluded_images,
                                     const int64_t *excluded_offsets, int32_t k, int64_t *out_images, float *out_scores,
                                     int64_t *out_best_rows, int32_t *out_counts);
ssw_status ssw_index_view_topk_batch_avg(ssw_index *view, const float *q_host, int32_t nq, const int64_t *excluded_images,
                                         const int64_t *excluded_offsets, int32_t k, int32_t aug_larger,
                                         int64_t *out_images, float *out_scores, int64_t *out_best_rows,
                                         float *out_avg_scores, int64_t *out_avg_rows, int32_t *out_counts);

/* The SECOND STAGE of a batch of TWO-VECTOR queries (`query(vector=, vector2=)`, seesaw/indices/multiscale/
 * multiscale_index.py:341-352: `scores = vectors[ilocs] @ vector`, `scores -= vectors[ilocs] @ vector2`, then
 * rescore_candidates), for nq queries in ONE launch (k_pair_score, csrc/rescore.hip; DESIGN.md section 4, "Batched
 * two-vector query").  image_positions_host [nq, k] / counts_host [nq]: query b's candidates are its first counts_host[b]
 * entries (positions as ssw_index_topk_batch returns them, any order).  For query b and slot c < counts_host[b] the tiles
 * of that image are scored straight from the index rows, each row read once: v = the bits of ssw_index_scan(q_host[b]),
 * v2 = the bits of ssw_index_score_rows(q2_host[b]), d = v - v2 in f32, and aggregated:
 *   agg = SSW_AGG_AVG:   as ssw_index_rescore_avg aggregates the resident scores of q_host[b] with minus_scores = v2
 *                        (aug_larger: its codes, 0 / 1 / 2, optionally + 4);
 *   agg = SSW_AGG_PLAIN: the image's first tile with the highest non-NaN d (rescore_candidates' plain_score branch); an
 *                        image whose every d is NaN gives its first row, score NaN.  aug_larger is ignored.
 * out_scores / out_best_rows [nq, k]: entry [b, c] for c < counts_host[b]; entries from counts_host[b] on are LEFT AS
 * THEY WERE.  Host data in, host data out: one copy up (both query blocks, the positions, the counts), one launch, one
 * copy down, one host wait, on the handle's stream; the staging blocks are allocated by the first call and grown by a
 * larger one (ssw_index_destroy frees them).
 * Refused on the host before anything is enqueued: a view (SSW_ERR_UNSUPPORTED, the message says "view"); agg =
 * SSW_AGG_AVG on an index without tile meta, dim other than 256 / 512 / 768 / 1024, an image of more than 2048 tiles
 * anywhere in the index (SSW_ERR_UNSUPPORTED); nq outside [1, 65535], k outside [1, SSW_MAX_TOPK], a bad agg or
 * aug_larger, no image map, a count outside [0, k], a listed position outside the index, NULL arguments
 * (SSW_ERR_INVALID); a non-finite component in either query block (SSW_ERR_NUMERIC).
 * State afterwards is the state before, as for ssw_index_stage2_avg_batch_dev: the score buffer (partial or complete,
 * with its kept query), the result buffers, the installed exclusion set and the counters of ssw_index_prune_stats /
 * ssw_index_prune_completions stay as they were, so it follows a plain and a pruned first stage alike and never causes
 * a completing full scan. */
#define SSW_AGG_PLAIN 0
#define SSW_AGG_AVG 1
ssw_status ssw_index_stage2_pair_batch(ssw_index *idx, const float *q_host, const float *q2_host, int32_t nq,
                                       const int64_t *image_positions_host, const int32_t *counts_host, int32_t k,
                                       int32_t agg, int32_t aug_larger, float *out_scores, int64_t *out_best_rows);

/* merge several sorted key lists (e.g. the all-gathered per-shard top-k of a
 * row-sharded index; keys as in ssw_index_result_ptrs but with GLOBAL image ids
 * added by the caller via id_offsets) into the global top-k.  All pointers device. */
ssw_status ssw_topk_merge_dev(int32_t device, void *hip_stream, const uint64_t *dev_keys_in,
                              int32_t n_lists, int32_t list_stride, const int32_t *dev_counts,
                              int32_t k, uint64_t *dev_keys_out, int32_t *dev_count_out);

/* The sharded query as ONE device pipeline: scan -> select -> all-gather -> merge, with no elementwise kernels around
 * the collective.  ssw_index_set_exchange_target makes the selection's last kernel also write this rank's MESSAGE into
 * dev_msg [msg_len = (with_best ? 2 : 1) * k_max + 1 words]: keys - image_offset (the low word then holds
 * 0xFFFFFFFF - global image position) at [0, k), best rows + row_offset at [k_max, k_max + k) when with_best, and
 * count | overflow << 32 in the last word (NULL detaches).  ssw_topk_merge_msgs_dev merges `world` gathered messages:
 * a list's count is the low half of its last word; the overflow flags go to dev_flags [world] (i64) and are OR-ed into
 * dev_flags_seen [1].  No reference counterpart. */
ssw_status ssw_index_set_exchange_target(ssw_index *idx, uint64_t *dev_msg_or_null, int32_t k_max, int32_t with_best,
                                         int64_t image_offset, int64_t row_offset);
ssw_status ssw_topk_merge_msgs_dev(int32_t device, void *hip_stream, const uint64_t *dev_msgs, int32_t world,
                                   int32_t k_max, int32_t with_best, int32_t k, uint64_t *dev_keys_out,
                                   int32_t *dev_count_out, int64_t *dev_flags_or_null, int64_t *dev_flags_seen_or_null);

/* The sharded query for a CHUNK of queries: every rank reads its rows once per chunk and the exchange is one
 * all-gather and one merge launch per chunk.  Opt-in and beside everything above: ssw_index_topk_dev, the
 * ssw_index_topk_batch entries and the single exchange target keep their results, state and launch sequence.
 *
 * ssw_index_set_exchange_target_batch: dev_msgs [n_slots, msg_len] u64, msg_len = (with_best ? 2 : 1) * k_max + 1, every
 * slot a message in the format of ssw_index_set_exchange_target (NULL detaches).  State of its own: the single target,
 * if attached, is neither moved nor written by the batched entries, and they never write this one.  n_slots < 1 or
 * k_max outside [1, SSW_MAX_TOPK] is SSW_ERR_INVALID.
 *
 * ssw_index_topk_batch_dev: queries and exclusion lists as ssw_index_topk_batch, validated the same way before anything
 * is enqueued (SSW_ERR_NUMERIC / SSW_ERR_INVALID); also SSW_ERR_INVALID, before anything is enqueued: no batch target
 * attached, k > k_max, first_slot < 0, first_slot + nq > n_slots.  ENQUEUES ONLY: it waits for the device only where a
 * buffer has to grow or a staging block is reused (the side buffer, a long exclusion delta, the query block).  Chunking
 * and the side buffer are ssw_index_topk_batch's; the scan is always the full-precision one (no shadow is built or read,
 * the prune counters stay; a partial score buffer is completed first).  For query b the call installs its exclusion set
 * and runs the ordinary selection on its slab -- the one-launch, the histogram or the sampled form -- whose last kernel
 * writes message slot first_slot + b.  An overflowed fast selection (mass ties, a sampled threshold that left too few
 * candidates) is NOT repaired here: the overflow bit travels in the slot's last word, as in the single path.  An index
 * without images writes "0 keys" into its slots.
 * State afterwards: that of ssw_index_topk_dev(q[nq-1]) with the last query's exclusion set installed (resident scores,
 * result buffers, installed set).  ssw_index_profile records one event pair per scan launch.
 * Measured with tools/perf_sharded_batch.py ("Sharded batch").
 *
 * ssw_index_topk_slot_deep_dev: the repair of ONE flagged query: a single-query full scan of q_host (the slabs of the
 * chunk are gone by the time the flags are read; the batched scan returns the bits of the single scan, so the result
 * is the one the slab would have given), its exclusion list installed, the deep selection, the message into `slot` of
 * the batch target.  Synchronises inside, like ssw_index_select_deep_dev.  Same refusals as above.
 *
 * ssw_topk_merge_msgs_batch_dev: ssw_topk_merge_msgs_dev for nq queries in ONE launch (one workgroup per query).  Rank
 * r's message for query b starts at word r * rank_stride + b * msg_len -- the layout one all-gather of nq * msg_len
 * words per rank leaves, with rank_stride = nq * msg_len.  dev_keys_out [nq, k_max], dev_counts_out [nq], dev_flags
 * [nq, world] (i64), dev_flags_seen [1] (OR-ed, atomically).  Row b holds the bits ssw_topk_merge_msgs_dev produces
 * from query b's `world` messages.  Limits: those of the single merge (world * k <= 8192, k <= k_max), nq >= 1,
 * rank_stride >= nq * msg_len. */
ssw_status ssw_index_set_exchange_target_batch(ssw_index *idx, uint64_t *dev_msgs_or_null, int32_t n_slots, int32_t k_max,
                                               int32_t with_best, int64_t image_offset, int64_t row_offset);
ssw_status ssw_index_topk_batch_dev(ssw_index *idx, const float *q_host, int32_t nq, const int64_t *excluded_images,
                                    const int64_t *excluded_offsets, int32_t k, int32_t first_slot);
ssw_status ssw_index_topk_slot_deep_dev(ssw_index *idx, const float *q_host, const int64_t *excluded_images,
                                        int64_t n_excluded, int32_t k, int32_t slot);

/* ssw_index_topk_batch_dev with the certified int8 pre-scan of ssw_index_topk_batch_pruned, and still ENQUEUE ONLY: no
 * survivor count is published and nothing waits for the device.  Arguments, refusals and the empty index are
 * ssw_index_topk_batch_dev's.  On an index the pruned batch does not serve (fewer than 2^22 rows, dim other than 256 /
 * 512 / 768 / 1024, a dim-768 index of fewer than 2^20 rows -- its own count --, borrowed or escaped rows, a shadow
 * refused for memory) the call IS ssw_index_topk_batch_dev.  Otherwise,
 * per chunk of up to 16 queries (any width): one pass over the shadow bounds the chunk; per query the threshold
 * selection and the survivor list; ONE launch (k_rescore_survivors, csrc/rescore_dev.hip), sized by the device alone,
 * scores every certified slot's survivors -- the full scan's bits -- straight into its slab; per query the ordinary
 * selection writes message slot first_slot + b.  A slot whose certificate failed (threshold selection short of k keys or
 * overflowed, unboundable query, more than 2^18 survivors) is NOT repaired here: its selection ran over bounds and BIT
 * 33 (value 2 in the upper half) of its message's last word says so, beside the overflow bit 32.  The merge reports
 * either as a non-zero flag of that (query, rank), and ssw_index_topk_slot_deep_dev repairs either exactly.
 * State afterwards: that of ssw_index_topk_batch_dev, except that the score buffer is partial with the last query kept
 * (every reader completes or rescores it by the rules of the pruned top-k), and ssw_index_prune_stats counts every
 * query in [3]; [2] and [4] stay, the host does not know them.
 * ssw_index_prune_batch_dev_read: what the device decided for the LAST chunk of the last such call: waits for the
 * stream, then out32 [2 * 16]: for slot j < *out_w, out32[2 j] = the raw survivor count (it passes the cap when more
 * rows qualify) and out32[2 j + 1] = the reasons it failed: 1 threshold selection, 2 unboundable query, 4 over the cap;
 * 0 = certified.  *out_w = 0 when the last call took the plain scan or a host-waiting pruned batch ran since. */
ssw_status ssw_index_topk_batch_dev_pruned(ssw_index *idx, const float *q_host, int32_t nq, const int64_t *excluded_images,
                                           const int64_t *excluded_offsets, int32_t k, int32_t first_slot);
ssw_status ssw_index_prune_batch_dev_read(ssw_index *idx, int32_t *out32, int32_t *out_w);
ssw_status ssw_topk_merge_msgs_batch_dev(int32_t device, void *hip_stream, const uint64_t *dev_msgs, int32_t world,
                                         int64_t rank_stride, int32_t nq, int32_t k_max, int32_t with_best, int32_t k,
                                         uint64_t *dev_keys_out, int32_t *dev_counts_out, int64_t *dev_flags_or_null,
                                         int64_t *dev_flags_seen_or_null);

/* The SECOND STAGE of the sharded chunk, for the avg_score aggregation (rescore_candidates, multiscale_index.py:379-403):
 * every merged candidate is aggregated on the rank that holds its tiles, in ONE launch for the group's nq queries
 * (k_avg_score_owner, csrc/rescore.hip; DESIGN.md section 4, "Sharded batch: second stage").  dev_keys [nq, k_max] and
 * dev_counts [nq] are what ssw_topk_merge_msgs_batch_dev wrote: the low word of a key holds 0xFFFFFFFF - the GLOBAL
 * image position.  This handle's images are the positions [image_offset, image_offset + n_images) and its rows start at
 * row_offset of the whole index.  For query b and slot c < k: if c < dev_counts[b] and the image is this handle's, its
 * tiles are scored for q_host[b] straight from the index rows -- the bits of ssw_index_scan -- and aggregated as
 * ssw_index_rescore_avg aggregates them (aug_larger: its codes, 0 / 1 / 2, optionally + 4);
 *   dev_out[b][0][c] = 1 << 32 | the f32 bits of the aggregated score (the owned bit is apart: the score may be NaN),
 *   dev_out[b][1][c] = row_offset + the image's first tile with that score (i64);
 * otherwise both words are 0.  dev_out is [nq, 2, k_max] u64; every c < k is written, c >= k is left as it was.  Over
 * all ranks every (b, c < dev_counts[b]) has exactly one owner.
 * ENQUEUES ONLY, on the handle's stream: it waits for the device only where a staging block is reused (the query block,
 * which holds 16 queries; a longer batch is served in parts).  Refused before anything is enqueued: NULL arguments,
 * nq < 1, k outside [1, k_max], k_max > SSW_MAX_TOPK, a bad aug_larger, no image map or tile meta, an image of more than
 * 2048 tiles anywhere in the index (SSW_ERR_INVALID); a non-finite query (SSW_ERR_NUMERIC); dim other than 256 / 512 /
 * 768 / 1024 (SSW_ERR_UNSUPPORTED).
 * State afterwards is the state before: the kernel reads the rows, the tile meta and the image map and nothing else,
 * so the score buffer (partial or complete, with its kept query), the result buffers, the installed exclusion set and
 * the counters of ssw_index_prune_stats / ssw_index_prune_completions stay as they were -- it follows the plain and the
 * pruned first stage alike and never causes a completing full scan. */
ssw_status ssw_index_stage2_avg_batch_dev(ssw_index *idx, const float *q_host, int32_t nq, const uint64_t *dev_keys,
                                          const int32_t *dev_counts, int32_t k_max, int32_t k, int32_t aug_larger,
                                          int64_t image_offset, int64_t row_offset, uint64_t *dev_out);

/* The collective itself (`ssw_topk_allgather(ssw_comm *, ...)`): RCCL bound at run time (dlopen; the
 * copy torch mapped, if any).  ssw_comm_unique_id on one rank -> 128 bytes handed to every rank by the caller's own
 * means -> ssw_comm_create on every rank (collective).  ssw_topk_allgather enqueues ncclAllGather of msg_len u64 words
 * per rank on hip_stream; dev_recv [world * msg_len] is in rank order. */
typedef struct ssw_comm ssw_comm;
ssw_status ssw_comm_unique_id(void *out_id128);
ssw_status ssw_comm_create(int32_t device, const void *unique_id128, int32_t rank, int32_t world, ssw_comm **out);
ssw_status ssw_comm_destroy(ssw_comm *comm);
ssw_status ssw_topk_allgather(ssw_comm *comm, void *hip_stream, const uint64_t *dev_send, uint64_t *dev_recv,
                              int32_t msg_len);

/* per-launch device time of the dominant (scan) kernel, measured with HIP events
 * on the handle's stream.  enable=1 starts recording one event pair per scan
 * launch (up to 4096 launches); ssw_index_profile_read synchronises and returns
 * the durations in milliseconds. */
ssw_status ssw_index_profile(ssw_index *idx, int32_t enable);
ssw_status ssw_index_profile_read(ssw_index *idx, float *out_ms, int32_t cap, int32_t *out_n);

/* Pruned top-k.  ssw_index_topk / ssw_index_topk_dev with a query, on an index of at least 2^22 rows (f32 or f16) that
 * owns its matrix (dim 256, 512 or 1024), scan an int8 shadow of the rows -- of the widened rows for f16 -- (dim + 8
 * bytes a row, built on the first such call
 * after the rows last changed, only if 4 GiB of device memory stay free beside it) for certified lower and upper bounds
 * of every score, and rescore exactly only the rows whose upper bound reaches the k-th image's lower bound.  The result
 * is the bits of the full scan; the call waits once on the host for the survivor count.  Whenever the certificate
 * fails the full scan runs instead.  The score buffer then holds exact scores for the survivors only; every entry that
 * reads all of it (topk with q = NULL, select_deep_dev, device_ptrs, the labelprop top-k) first completes it with the
 * full scan of the kept query, and upload / fill_random do so before they change the rows.  The second-stage readers
 * make exact what they read and leave it partial: rescore_avg scores the candidates' tiles with the kept query by
 * gather and scatters them into the buffer, gather_scores scores the requested rows straight into its output -- both
 * the full scan's bits; above 2^18 rows in one call either completes the buffer instead.
 * An index that borrows a device matrix and an index whose row pointer ssw_index_device_ptrs has handed out never get
 * a shadow.  An f16 index with its shadow holds dim * 3 + 8 bytes a row.  The environment variable SSW_TOPK_FULL_SCAN
 * (read once) forces the full scan everywhere, for both element types.
 * Dim 768 (CLIP ViT-L/14): such an index is pruned on the packed 6-bit shadow alone -- 3 dim / 4 + 8 = 584 bytes a row in
 * tiles of 16 rows, (n + 15) / 16 * 16 * 584 bytes in all, against 3072 (f32) or 1536 (f16) bytes of a row -- from 2^20
 * rows on, f32 or f16, single queries and pruned batches alike (the smallest size measured; the pruned call is ahead of
 * the full scan at every one); it never gets an int8 shadow, and below that count, or when the shadow is refused for
 * memory, every call is the full-precision one.  [0] and [5] then report that shadow.
 * From 25 M rows on, single queries on an f32 index of dim 512 or 1024 that has no image map at the time of the call
 * scan a packed 5-bit shadow instead of the 6-bit one -- 5 dim / 8 + 8 = 328 bytes a row at dim 512, (n + 15) / 16 * 16
 * rows of it -- and raise the threshold to the k-th exact score of max(1024, 4 k) candidates before the survivors are
 * listed; such an index builds no 6-bit shadow for single queries (a pruned batch still builds its own), [0] reports
 * the 5-bit shadow and [5] includes its bytes.  Refused for memory, it leaves the 6-bit and then the int8 path.
 * The same calls scan the two-stage form of those 5-bit codes instead where the library's constant for it admits the
 * index ("Two-stage 4 + 1-bit shadow"): a 4-bit plane every row is scanned on and a 1-bit plane read
 * only for the rows that scan leaves, 5 dim / 8 + 16 bytes a row in all; such an index builds no packed 5-bit shadow, [0]
 * reports the two-stage shadow and [5] includes its bytes; refused for memory, it leaves the 5-bit path.
 * out6: [0] shadow 0 none / 1 current / 2 stale / 3 refused (memory), [1] 1 = the next top-k with a query is pruned,
 * [2] survivors of the last pruned call (-1 = it fell back), [3] pruned calls, [4] fallbacks, [5] shadow bytes. */
ssw_status ssw_index_prune_stats(ssw_index *idx, int64_t *out6);
/* the two-stage shadow's own counters: out3 [0] rows the first stage left in the last such call, [1] calls so far whose
 * second stage walked every row because the first left more than its list admits (dense), [2] two-stage calls so far. */
ssw_status ssw_index_prune_coarse_stats(ssw_index *idx, int64_t *out3);
/* what the readers of a partial score buffer or slab cost: out2 [0] full scans launched to complete one (by a reader of
 * the whole buffer, by a second-stage call over more than 2^18 rows, before the rows change), [1] rows scored by gather
 * instead -- the candidates' tile total of ssw_index_rescore_avg, the rows of ssw_index_gather_scores, the k x T list
 * entries of the two-stage batch. */
ssw_status ssw_index_prune_completions(ssw_index *idx, int64_t *out2);

/* ------------------------------------------------------------------------- */
/* k-NN-graph label propagation                                               */
/* replaces: LabelPropagation.fit_transform  seesaw/label_propagation.py:45-79 */
/*           (scipy csr_matvec sweeps, <= 300 per refine: knn_methods.py:186)  */
/* ------------------------------------------------------------------------- */
typedef struct ssw_lp ssw_lp;

/* W: n x n CSR with sorted column indices (get_weight_matrix, knn_graph.py:31-104);
 * host arrays indptr [n+1] i64, indices [nnz] i32, data [nnz] f64.
 * weight_sum = W.sum(0) [n] f64, or NULL to have it computed in scipy's order. */
ssw_status ssw_labelprop_create(int32_t device, int64_t n, const int64_t *indptr_host,
                                const int32_t *indices_host, const double *data_host,
                                const double *weight_sum_host_or_null, ssw_lp **out);
ssw_status ssw_labelprop_destroy(ssw_lp *lp);
/* one fit_transform: prior = reg_values (NULL only with reg_lambda == 0), start = the
 * start iterate (labels are clamped into it first), label ids/values, epsilon, max_iter.
 * out_f [n] f64 = what the reference returns: the iterate that entered the converging
 * sweep, or the last sweep's output without convergence.  *out_sweeps = sweeps run.
 * SSW_ERR_NUMERIC if a sweep leaves [min(0,prior.min()), max(1,prior.max())] -- the
 * reference's assert (label_propagation.py:36-40). */
ssw_status ssw_labelprop_run(ssw_lp *lp, const double *prior_host_or_null, const double *start_host,
                             const int64_t *label_ids, const double *label_vals, int64_t n_labels,
                             double reg_lambda, double eps, int32_t max_iter, double *out_f_host,
                             int32_t *out_sweeps, int32_t *out_converged);

/* A graph laid out in a LOCALITY ORDER (label_propagation.py:30-43 is unchanged arithmetic): node `old`
 * sits at position new_of_old[old]; row r of the CSR passed to create is the row of the node at position r, its columns
 * relabelled to positions but kept in ascending ORIGINAL column id -- scipy's summation order, which the sweep follows
 * entry by entry, so results stay bit-identical -- and weight_sum in position order.  Neighbours then sit near each other
 * in the iterate and the sweep's gathers hit cache.  Every entry point keeps taking and returning original ids.
 * ssw_labelprop_set_permutation must directly follow ssw_labelprop_create; ssw_labelprop_create_ordered does both and
 * skips the column-blocked copy. */
ssw_status ssw_labelprop_set_permutation(ssw_lp *lp, const int32_t *new_of_old_host);
ssw_status ssw_labelprop_create_ordered(int32_t device, int64_t n, const int64_t *indptr_host, const int32_t *indices_host,
                                        const double *data_host, const double *weight_sum_host,
                                        const int32_t *new_of_old_host, ssw_lp **out);

/* Device-resident chaining for the ranking loop (KnnProp2: the same prior is reg_values and start iterate
 * of every call, and the result only feeds a top-k): install the prior once, propagate without moving the
 * [n] f64 vectors over PCIe, hand the scores to the index's score buffer as f32 (labelled nodes at -inf
 * when mask_labeled != 0) for ssw_index_topk(q = NULL), and fetch the f64 result only when asked for. */
ssw_status ssw_labelprop_set_prior(ssw_lp *lp, const double *prior_host);
ssw_status ssw_labelprop_run_resident(ssw_lp *lp, const int64_t *label_ids, const double *label_vals,
                                      int64_t n_labels, double reg_lambda, double eps, int32_t max_iter,
                                      int32_t *out_sweeps, int32_t *out_converged);
/* Consecutive ssw_labelprop_run_resident calls of a ranking loop (knn_methods.py:176-199: every update() restarts from
 * the same prior with a few more labels) are INCREMENTAL: the handle keeps the previous call's iterates and, per sweep,
 * the block maxima of the convergence test; a call recomputes the rows within k hops of a changed label for sweep k and
 * nothing else -- same per-row arithmetic and order as the full sweeps, so values, sweep count and the returned iterate
 * are bit-identical to a from-scratch run (label_propagation.py:45-79), at a cost independent of n.  Falls back to full
 * sweeps when the change reaches n / 8 rows, when parameters change, or when more sweeps are needed than were kept (7).
 * out8: [0] 1 = the last propagation was an incremental update (0 = full sweeps, 2 = an incremental pass over the kept
 * iterates that did not converge within them, continued by full sweeps from there), [1] sweeps as the reference counts
 * them, [2] kernel launches, [3] host synchronisations, [4] rows recomputed over all sweeps, [5] iterates kept for the
 * next call, [6] nanoseconds of host time from entry until everything was enqueued, [7] nanoseconds waited for the device
 * (incremental runs).  Environment SSW_LP_NO_INCREMENTAL=1: every call runs the full sweeps (A/B, tests). */
ssw_status ssw_labelprop_last_run_info(ssw_lp *lp, int64_t *out8);
/* "nothing to propagate yet": the installed prior itself becomes the resident result (unchanged values) and the given
 * nodes are marked labelled, so that the first rounds of a graph loop -- BaseLabelPropagationRanker.update skips the
 * propagation until a negative label exists and serves the prior (research/knn_methods.py:62-75) -- go through the
 * same device path as the later ones. */
ssw_status ssw_labelprop_prior_as_result(ssw_lp *lp, const int64_t *label_ids, int64_t n_labels);
ssw_status ssw_labelprop_fetch(ssw_lp *lp, double *out_f_host);
/* out[i] = result[rows[i]] for m nodes (host arrays): the pseudo-labels makeXy takes from the propagated scores
 * (seesaw/loops/util.py:19, `lr.current_scores()[~is_labeled][randsel]`) -- 8 m bytes back instead of 8 n. */
ssw_status ssw_labelprop_gather(ssw_lp *lp, const int64_t *rows_host, int64_t m, double *out_host);
ssw_status ssw_labelprop_scores_to_index(ssw_lp *lp, ssw_index *index, int32_t mask_labeled);
/* One feedback round of a graph loop in ONE call -- KnnProp2.refine + next_batch (seesaw/loops/graph_based.py:73-121;
 * LabelPropagationRanker2.update, seesaw/research/knn_methods.py:176-199):
 *   propagate != 0: ssw_labelprop_run_resident(label_ids, label_vals, ...);  == 0: ssw_labelprop_prior_as_result(label_ids)
 *   then ssw_labelprop_scores_to_index(mask_labeled) and ssw_index_topk(index, q = NULL, excluded_images, n_excluded, k, out_*)
 * with the results of the three calls.  When the propagation is an incremental update (every round of a session after the
 * first that propagates) the whole round is enqueued on one stream -- the scores kernel takes the converged iterate's
 * number from the device-side control block -- and the host waits ONCE, on the selection's sequence word in pinned memory
 * (ssw_labelprop_last_run_info: [3] = 1).  info[0] = 3 for propagate == 0. */
ssw_status ssw_labelprop_round(ssw_lp *lp, ssw_index *index, int32_t propagate, const int64_t *label_ids,
                               const double *label_vals, int64_t n_labels, double reg_lambda, double eps, int32_t max_iter,
                               int32_t mask_labeled, const int64_t *excluded_images, int64_t n_excluded, int32_t k,
                               int64_t *out_images, float *out_scores, int64_t *out_best_rows, int32_t *out_count,
                               int32_t *out_sweeps, int32_t *out_converged);
/* ssw_labelprop_round for n_slots graph handles over ONE index in one call: the lock-step round of several graph loops
 * (SessionGroup.refine -> KnnProp2.refine_batch).  lps [n_slots]: distinct handles on the index's device, each with a
 * prior installed and n == the index's rows.  Per slot j: propagate[j], its labels label_ids / label_vals
 * [label_offsets[j], label_offsets[j + 1]) of the packed arrays, reg_lambda[j], eps[j], max_iter[j], and its excluded
 * images packed with offsets as in ssw_index_topk_batch (excluded_offsets NULL: nobody excludes).  mask_labeled and k
 * hold for the whole call.  Outputs [n_slots, k] row-major (row j filled up to out_counts[j]), out_counts / out_sweeps /
 * out_converged / out_status [n_slots] (images, scores, best rows, sweeps and converged may be NULL).
 * Contract: for every slot the outputs are the bits ssw_labelprop_round(lps[j], index, slot j's arguments) returns,
 * and the handle is left as that call leaves it -- iterates, kept levels and block maxima, installed labels, result,
 * sweeps hint and ssw_labelprop_last_run_info [0], [1], [4], [5] -- so a later single or batched call on any of the
 * handles continues from there, incrementally.  A slot's failure (e.g. SSW_ERR_NUMERIC when its values left the bounds)
 * is out_status[j] with the message in ssw_labelprop_batch_error(lps[j]); the other slots are not affected and the call
 * returns SSW_OK.
 * Routing, decided on the host before anything is enqueued for the slot:
 *   incremental slots (propagate, valid tracked state, unchanged reg_lambda / eps / max_iter, unique ids, a non-empty
 *     change of at most n / 8 labels, SSW_LP_NO_INCREMENTAL unset) take the BATCHED PASS: one device table of per-slot
 *     descriptors, the pass's kernels launched once for the chunk with the slot on blockIdx.y -- 3 + 3 x (the deepest kept
 *     level) launches whatever the number of slots -- the last of which writes slot j's f32 scores into slab j of the
 *     index's batch slabs and leaves the slot's control block in the slot's pinned memory;
 *   prior slots (propagate == 0) enqueue ssw_labelprop_prior_as_result's work without a wait and join the batched scores
 *     and selection with iterate 0; unchanged slots (the same labels) join with the kept result;
 *   everything else (a first full propagation, other parameters, duplicate ids, too large a change, max_iter == 0) runs
 *     the single round inside the call, one slot after another.  A batched FIRST propagation is out of scope.
 * The selections of a chunk's slots follow back to back, each over its slab into its own pinned block under its own
 * sequence word, and the host waits ONCE a chunk.  After that wait: a slot whose fast selection overflowed (mass ties) is
 * selected again on the deep path from its slab; an incremental slot whose frontier overflowed or that needs more sweeps
 * than were kept is finished by the single path's continuation (full sweeps) and gets its own scores and selection.
 * More than 16 slots: several chunks in the one call.
 * Streams: the call runs on lps[0]'s stream; it first waits for the index (ssw_index_sync) and every other handle's
 * stream, and returns with everything complete.  The index's score buffer holds some slot's scores afterwards and is
 * complete (no resident query describes it).
 * Errors before any device work, leaving every handle and the index untouched (SSW_ERR_INVALID): NULL or duplicate
 * handles, a device or row-count mismatch, a handle without a prior, k outside [1, SSW_MAX_TOPK], a label id or an
 * excluded image out of range in any slot, decreasing offsets.  A view index: SSW_ERR_UNSUPPORTED ("view").
 * out_stats4 (may be NULL): [0] slots that took the batched pass, [1] kernel launches of that pass up to and including
 * the scores kernel (selections excluded), [2] host waits of the call, [3] slots finished on the single path or by the
 * continuation.  ssw_labelprop_last_run_info of a batched slot: [2] = the launches of its chunk's pass, [3] = 1 (the
 * chunk's wait), [6] / [7] = nanoseconds of the CALL from entry until the chunk was enqueued / waited for the chunk. */
ssw_status ssw_labelprop_round_batch(ssw_lp *const *lps, int32_t n_slots, ssw_index *index, const int32_t *propagate,
                                     const int64_t *label_ids, const double *label_vals, const int64_t *label_offsets,
                                     const double *reg_lambda, const double *eps, const int32_t *max_iter,
                                     int32_t mask_labeled, const int64_t *excluded_images, const int64_t *excluded_offsets,
                                     int32_t k, int64_t *out_images, float *out_scores, int64_t *out_best_rows,
                                     int32_t *out_counts, int32_t *out_sweeps, int32_t *out_converged, int32_t *out_status,
                                     int64_t *out_stats4);
const char *ssw_labelprop_batch_error(const ssw_lp *lp);
/* device address of the [n] f64 result of the last propagation (valid until the next run on this handle). */
ssw_status ssw_labelprop_device_scores(ssw_lp *lp, const double **out_dev_scores);

/* The symmetric k-NN weight matrix on the device: get_weight_matrix(symmetric=True) (seesaw/knn_graph.py:31-104) from
 * the directed edge list src / dst [n_edges] i32 and w [n_edges] f64 = kfun(distance) (formed by the caller on the host:
 * exp() rounds as numpy's) -> CSR with sorted indices, W_ij = (sum over the directions present) / (their number), the
 * diagonal stored as 0.  Bit-identical to the reference's arrays (one commutative addition, one division per entry).
 * SSW_ERR_UNSUPPORTED: a vertex with more than 4096 incident edges, or a vertex pair with more than two edges (repeated
 * edges: the host path then decides the sum order).  ssw_wm_fetch copies indptr [n + 1] i64, indices [nnz] i32, data [nnz]
 * f64 to the host. */
typedef struct ssw_wm ssw_wm;
ssw_status ssw_wm_build_symmetric(int32_t device, int64_t n, int64_t n_edges, const int32_t *src_host,
                                  const int32_t *dst_host, const double *w_host, ssw_wm **out, int64_t *out_nnz);
ssw_status ssw_wm_fetch(ssw_wm *m, int64_t *indptr_host, int32_t *indices_host, double *data_host);
ssw_status ssw_wm_destroy(ssw_wm *m);

/* Exact k-NN graph over the resident matrix (rows as vertices, cosine / dot similarity):
 * replaces compute_exact_knn, seesaw/knn_graph.py:170-191 (`1 - X @ X.T`, argsort, first k+1).
 * out_dst / out_score are [n_rows, k+1]: per row the k+1 best rows INCLUDING the row itself,
 * ordered by (score descending, row id ascending); scores are the bits ssw_index_scan would
 * return for that row as the query (distance = 1 - score).  out_certified [n_rows]: 1 when the
 * row's list is proven exact; rows with 0 must be recomputed with ssw_index_topk (rare: the
 * fp16 candidate pass could not separate the k+1-th neighbour from the rest).  `seed` fixes the
 * random column order of the candidate pass; results do not depend on it.  1 <= k <= 31. */
ssw_status ssw_knn_build(ssw_index *index, int32_t k, uint64_t seed, int32_t *out_dst_host,
                         float *out_score_host, uint8_t *out_certified_host);

/* K6: out [dim, dim] f64 = X' L X for the resident matrix X of `index` and the CSR matrix L held
 * by `laplacian` (an ssw_lp created from the graph Laplacian, already divided by its trace):
 * replaces `X_vectors.T @ (L @ X_vectors)`, seesaw/loops/graph_based.py:45-49. */
ssw_status ssw_xlx(ssw_index *index, ssw_lp *laplacian, double *out_host);

/* ------------------------------------------------------------------------- */
/* Online relevance-feedback update: fused loss+gradient on the GPU, L-BFGS    */
/* (strong Wolfe) driver on the host.                                          */
/* replaces: LogisticRegressionPT.fit      seesaw/logistic_regression.py:350-406 */
/*           RegModule.fit (MultiReg)      seesaw/loops/multi_reg.py:139-162    */
/*           BasicTrainer.fit / torch.optim.LBFGS closure loop                  */
/*                                         seesaw/basic_trainer.py:11-69        */
/*           ref_pairwise_rank_loss / ref_pairwise_logistic_loss               */
/*                                         seesaw/rank_loss.py:34-95            */
/* ------------------------------------------------------------------------- */
typedef struct ssw_fb ssw_fb;

enum { SSW_FB_LOGREG = 0, SSW_FB_MULTIREG = 1, SSW_FB_RANKREG = 2 };
enum { SSW_FB_LOSS_CE = 0, SSW_FB_LOSS_PAIRWISE_HINGE = 1, SSW_FB_LOSS_PAIRWISE_LOGISTIC = 2 };
enum { SSW_FB_REG_NONE = 0, SSW_FB_REG_VECTOR = 1, SSW_FB_REG_NORM = 2, SSW_FB_REG_NORM1 = 3 };

typedef struct ssw_fb_objective {
    int32_t kind;          /* SSW_FB_LOGREG | SSW_FB_MULTIREG | SSW_FB_RANKREG (RankRegressionPT:  */
                           /* cheap pairwise rank loss + reg_kind / reg_weight as LOGREG)      */
    int32_t loss_type;     /* MULTIREG: label_loss_type (multi_reg.py:34-35)                   */
    int32_t fit_intercept; /* LOGREG: extra bias parameter after the dim weights               */
    int32_t reg_kind;      /* LOGREG: regulariser (logistic_regression.py:304-330)             */
    float pos_weight;      /* LOGREG: BCE pos_weight; MULTIREG ce_loss: < 0 means 'balanced'   */
    float reg_weight;      /* LOGREG: reg_lambda / n_examples (:366)                           */
    float margin;          /* MULTIREG: rank_loss_margin                                       */
    float reg_norm_lambda; /* MULTIREG                                                         */
    float reg_data_lambda; /* MULTIREG (needs ssw_fb_set_xlx when != 0)                        */
    float reg_query_lambda;/* MULTIREG                                                         */
} ssw_fb_objective;

/* Two linear outputs sharing the rows: MultiRegModule, the scorer of the multi_reg_neg loop
 * (seesaw/loops/multi_reg_module.py:40-165, loops/multi_reg_neg.py:26-109).  W [2, dim] raw weights (row 0 the target
 * query, row 1 the confusion class); logits use the L2-normalised rows.  loss = sum_i s_i [bce(z_i0, y_i0) +
 * bce(z_i1, y_i1)] + sum_{i: y_i0 + y_i1 > 0} s_i CE(z_i, y_i) + reg_norm_lambda sum_c (cosh(log |W_c|) - 1)
 * + reg_query_lambda sum_c (1 - <W_c / |W_c|, q^>) / 2, all f32 as in the reference.  Rows come from
 * ssw_fb_set_data[_from_device] (centred), the query from ssw_fb_set_query; y2 is [n, 2] row-major.
 * ssw_fb_fit2 = one torch.optim.LBFGS(strong_wolfe).step from W_inout (BasicTrainer.fit, max_epochs = 1).
 * out_parts5: loss_norm, loss_queryreg, loss_queryreg2, vertical, horizontal.  dim <= 512. */
ssw_status ssw_fb_set_targets2(ssw_fb *fb, const float *y2_host, const float *sample_weight_or_null);
ssw_status ssw_fb_lossgrad2(ssw_fb *fb, const float *W_host, float reg_norm_lambda, float reg_query_lambda,
                            float *out_loss, float *out_grad, float *out_parts5_or_null);
ssw_status ssw_fb_fit2(ssw_fb *fb, float *W_inout, float reg_norm_lambda, float reg_query_lambda, int32_t max_iter,
                       float lr, int32_t *out_iters, int32_t *out_evals, float *out_final_loss);
/* ssw_fb_lossgrad2 with the whole evaluation on the device (opt-in): replaces one call of MultiRegModule._step
 * (seesaw/loops/multi_reg_module.py:64-128) including F.normalize, its chain rule and the two regularisers, which
 * ssw_fb_lossgrad2 forms on the host.  Same outputs; the operation order is ssw_fb_lossgrad2's, the values differ from
 * it only where the device library's logf / coshf / sinhf differ from the host's. */
ssw_status ssw_fb_lossgrad2_dev(ssw_fb *fb, const float *W_host, float reg_norm_lambda, float reg_query_lambda,
                                float *out_loss, float *out_grad, float *out_parts5_or_null);
/* ssw_fb_fit2 over that device evaluation for nfit engines at once (opt-in; nfit = 1 is the single fit): the call
 * site it replaces nfit times is the LBFGS of seesaw/loops/multi_reg_module.py:142 stepped at basic_trainer.py:59-63
 * (opt.step(closure)), once per multi_reg_neg session of a group that refines in lock step.  Slot s fits fbs[s] from
 * row s of W_inout ([nfit][2 dim]) with reg_norm_lambda[s], reg_query_lambda[s], max_iter[s], lr[s].  Every slot of
 * 0 to 1024 rows gets one workgroup of ONE launch (k_fb_fit2_wg_batch; 0 rows: the regularisers alone); a larger set,
 * or env SSW_FB_HOST_DRIVER, is driven from the host afterwards, one device evaluation and one wait at a time.  Both
 * drivers walk the same path bit for bit (weights, iterations, evaluations, loss); ssw_fb_last_fit_on_device tells per
 * handle.  Stream and event ordering between the engines, the per-slot SSW_ERR_NUMERIC (row untouched, message in
 * ssw_fb_batch_error, the call returns SSW_OK) and the optional outputs are ssw_fb_fit_batch's.
 * Refused before anything is queued (SSW_ERR_INVALID): nfit < 1, a NULL or repeated handle, handles of different
 * device or dim, 2 dim > 1024, max_iter < 1, a non-finite start weight, a slot with rows but without
 * ssw_fb_set_targets2, a slot without ssw_fb_set_query. */
ssw_status ssw_fb_fit2_batch(ssw_fb *const *fbs, int32_t nfit, float *W_inout, const float *reg_norm_lambda,
                             const float *reg_query_lambda, const int32_t *max_iter, const float *lr,
                             int32_t *out_iters, int32_t *out_evals, float *out_final_loss, int32_t *out_status);

ssw_status ssw_fb_create(int32_t device, int32_t dim, ssw_fb **out);
ssw_status ssw_fb_destroy(ssw_fb *fb);
/* labelled vectors X [n, dim] f32 from the host; center != 0 subtracts the column means
 * (StandardScaler(with_std=False) / X - X.mean(0)). */
ssw_status ssw_fb_set_data(ssw_fb *fb, const float *X_host, int64_t n, int32_t center);
/* PseudoLR's training set assembled on the device -- makeXy (seesaw/loops/util.py:4-23) + the weights of
 * seesaw/loops/pseudo_lr.py:42-44: rows = [the labelled rows, then for every p in `drawn` the p-th unlabelled row
 * (np.nonzero(~is_labeled)[0][p])], targets = [their labels, then the propagated scores of the drawn rows (f64 -> f32)],
 * sample weights = [real_weight ..., 1 ...]; the vectors are gathered out of the resident matrix and centred as in
 * ssw_fb_set_data.  dev_scores: ssw_labelprop_device_scores of the propagation that has just run; `drawn`: the prefix of
 * np.random.permutation(#unlabelled) (ssw_np_permutation_prefix[_dev]).  Replaces the three host passes and four copies
 * of the same construction through ssw_labelprop_gather + ssw_fb_set_data_from_device + ssw_fb_set_targets; the targets
 * exist on the device only, so the set serves the logistic objective (SSW_FB_LOGREG), which reads no target on the host. */
ssw_status ssw_fb_set_pseudo_sample(ssw_fb *fb, const float *dev_matrix, int64_t n_matrix_rows, const double *dev_scores,
                                    const int64_t *labelled_rows_sorted, const float *labelled_y, int64_t n_lab,
                                    const int64_t *drawn, int64_t n_drawn, float real_weight, int32_t center);
/* same, but the rows are gathered on the device out of a resident matrix (e.g. the index:
 * ssw_index_device_ptrs) -- `index.vectors[matchdf.index.values]`, multi_reg.py:204. */
ssw_status ssw_fb_set_data_from_device(ssw_fb *fb, const float *dev_matrix, int64_t n_matrix_rows,
                                       const int64_t *rows_host, int64_t n, int32_t center);
/* the two entries above with the rows gathered out of an index handle's matrix of either element type (an f16
 * index's rows are widened to f32): the same data as the raw-pointer forms on an f32 index of the widened rows. */
ssw_status ssw_fb_set_data_from_index(ssw_fb *fb, const ssw_index *index, const int64_t *rows_host, int64_t n,
                                      int32_t center);
ssw_status ssw_fb_set_pseudo_sample_from_index(ssw_fb *fb, const ssw_index *index, const double *dev_scores,
                                               const int64_t *labelled_rows_sorted, const float *labelled_y,
                                               int64_t n_lab, const int64_t *drawn, int64_t n_drawn, float real_weight,
                                               int32_t center);
/* targets y [n] f32 and optional per-item sample weights [n] f32. */
ssw_status ssw_fb_set_targets(ssw_fb *fb, const float *y_host, const float *sample_weight_or_null);
/* regulariser vector / query vector (normalised inside, F.normalize) and X'LX [dim, dim]. */
ssw_status ssw_fb_set_query(ssw_fb *fb, const float *q_host);
ssw_status ssw_fb_set_xlx(ssw_fb *fb, const float *xlx_host);
/* column means removed by the last set_data (the scaler's mean_). */
ssw_status ssw_fb_get_mean(ssw_fb *fb, float *out_mu_host);
/* one closure evaluation: loss and d loss / d params at w ([dim] or [dim+1] with intercept).
 * out_parts4 (MULTIREG) = loss_norm, loss_datareg, loss_queryreg, loss_labels. */
ssw_status ssw_fb_lossgrad(ssw_fb *fb, const ssw_fb_objective *obj, const float *w_host,
                           float *out_loss, float *out_grad, float *out_parts4_or_null);
/* logits X w (+ b) of the installed rows. */
ssw_status ssw_fb_scores(ssw_fb *fb, const float *w_host, int32_t has_bias, float *out_logits);
/* one optimizer.step(closure) of LBFGS(max_iter, lr, line_search_fn='strong_wolfe') starting
 * from w_inout; returns the fitted parameters in place.  SSW_ERR_NUMERIC on NaN/Inf loss
 * (the reference raises ValueError, logistic_regression.py:398-401). */
ssw_status ssw_fb_fit(ssw_fb *fb, const ssw_fb_objective *obj, float *w_inout, int32_t max_iter,
                      float lr, int32_t *out_iters, int32_t *out_evals, float *out_final_loss);
/* *out = 1 when the last ssw_fb_fit ran as ONE kernel launch (direction updates, line search and all closure
 * evaluations inside one workgroup: labelled sets of up to 1024 rows, every objective except SSW_FB_RANKREG),
 * 0 when the host drove one evaluation at a time (larger sets; or env SSW_FB_HOST_DRIVER).  Both walk the same
 * path bit for bit. */
ssw_status ssw_fb_last_fit_on_device(const ssw_fb *fb, int32_t *out);
/* ssw_fb_fit for nfit engines at once: the call site it replaces nfit times is the LBFGS of multi_reg.py:156 stepped
 * at basic_trainer.py:59-63 (opt.step(closure)), taken once per session of a group that refines in lock step.  Slot s fits objs[s] on
 * fbs[s] from row s of W_inout ([nfit][dim + 1]; a slot without intercept uses the first dim entries) with max_iter[s]
 * and lr[s], and ends with the bits ssw_fb_fit returns for the same inputs: weights, iterations, evaluations, loss.
 * Every slot that ssw_fb_fit would run as one launch gets one workgroup of ONE launch (k_fb_fit_wg_batch, grid = those
 * slots), on its own engine's buffers and completion word; one launch may mix objectives and set sizes, and more slots
 * than compute units queue.  Each engine's pending uploads stay on its own stream: the launch, on the first such
 * slot's stream, waits for an event recorded on every other slot's.  The host then waits for every slot's completion
 * word as ssw_fb_fit waits for one.  The slots ssw_fb_fit drives from the host (more than 1024 rows, SSW_FB_RANKREG,
 * env SSW_FB_HOST_DRIVER) go through ssw_fb_fit afterwards, one by one; ssw_fb_last_fit_on_device tells per handle.
 * Refused before anything is queued (SSW_ERR_INVALID): nfit < 1, a NULL or repeated handle, handles of different
 * device or dim, max_iter < 1, a non-finite start weight.
 * A slot whose loss or weights diverged gets SSW_ERR_NUMERIC in out_status, keeps its row of W_inout as it came, and
 * ssw_fb_batch_error(fbs[s]) is the message ssw_fb_fit would have left ("" for a slot that is SSW_OK); the other
 * slots are not concerned and the call returns SSW_OK.  out_iters, out_evals, out_final_loss ([nfit]) may be NULL. */
ssw_status ssw_fb_fit_batch(ssw_fb *const *fbs, const ssw_fb_objective *objs, int32_t nfit, float *W_inout,
                            const int32_t *max_iter, const float *lr, int32_t *out_iters, int32_t *out_evals,
                            float *out_final_loss, int32_t *out_status);
const char *ssw_fb_batch_error(const ssw_fb *fb);
/* forget the installed rows, targets, query and X'LX (the allocations stay): lets one engine serve the scorers the
 * loops build anew every refine (LogisticRegressionPT(...) per round, loops/pseudo_lr.py:33, log_reg.py:22) without
 * an allocate / free cycle per round. */
ssw_status ssw_fb_reset(ssw_fb *fb);

/* Host-only.  The first k entries of numpy's legacy `np.random.permutation(n)` drawn from the MT19937 state
 * (key[624], pos) of `np.random.get_state()`, which is advanced exactly as numpy's own call advances it (write it back
 * with `np.random.set_state`).  replaces `np.random.permutation(unl.shape[0])[:sample_size]`, seesaw/loops/util.py:13
 * (makeXy: PseudoLR's draw of pseudo-labelled rows) -- same sample, 15 ms -> 5 ms at 1.56 M rows. */
ssw_status ssw_np_permutation_prefix(uint32_t *mt_key624, int32_t *mt_pos, int64_t n, int64_t k,
                                     int64_t *out_prefix);
/* The same draw (same values, same stream position afterwards) with the walk through the swaps on GPU `device`: the host
 * makes the n - 1 draws into pinned memory, the device links the steps by target with one atomic exchange each and traces
 * the k wanted positions independently (~6 short list walks each) -- 2.4 ms -> 0.7 ms for 10 000 of 1.56 M.  device < 0,
 * n < 2^18 or k > n / 16: the host-only form above. */
ssw_status ssw_np_permutation_prefix_dev(int32_t device, uint32_t *mt_key624, int32_t *mt_pos, int64_t n, int64_t k,
                                         int64_t *out_prefix);

/* The pairwise rank losses on given scores (no data matrix): per-item column sums and d(sum)/d scores.
 * replaces ref_pairwise_rank_loss / ref_pairwise_logistic_loss(aggregate='sum') and
 * ref_pairwise_rank_loss_gradient, seesaw/rank_loss.py:34-106, and the per-item normalisation of
 * RegModule._step, seesaw/loops/multi_reg.py:106-121: out_item_loss[j] = coef_j / max_inversions_j *
 * sum_i loss_ij (coef NULL = all ones; coef = max_inversions gives the raw sums), out_grad = d sum_j / d scores. */
ssw_status ssw_rank_pairwise(int32_t device, int32_t logistic, const float *target_host, const float *scores_host,
                             const float *coef_host_or_null, int32_t n, float margin, double *out_item_loss,
                             float *out_grad);

/* The sort-based rank functions as counting kernels (exact integers, ties as the reference's stable sorts):
 * quick_pairwise_gradient_zero_margin(target, scores, return_max_inversions=True) -> gradient [n] (= 2 x net
 * position change between the (target, score) order and the (score, -target) order), max_reversals [n],
 * total_pairs; seesaw/rank_loss.py:109-161.  _CheapPairwiseRankingLoss (:164-187) is |gradient| / total_pairs. */
ssw_status ssw_rank_quick_gradient(int32_t device, const float *target_host, const float *scores_host, int32_t n,
                                   float *out_grad, float *out_max_reversals_or_null, int64_t *out_total_pairs_or_null);
/* compute_inversions(labs, scores), seesaw/pairwise_rank_loss.py:24-43: in descending score order (ties by index) a
 * positive counts the negatives before it, a negative the positives after it. */
ssw_status ssw_rank_inversions(int32_t device, const uint8_t *labels_host, const float *scores_host, int32_t n,
                               int64_t *out_inversions);

/* ------------------------------------------------------------------------- */
/* L-KNN active search: two-step look-ahead value of every node                 */
/* replaces: _top_sum / _opt_expected_utility_helper_lknn2                      */
/*           seesaw/research/active_search/efficient_nonmyopic_search.py:94-205 */
/*           (model state: seesaw/loops/LKNN_model.py:76-281)                   */
/* ------------------------------------------------------------------------- */
typedef struct ssw_lknn ssw_lknn;
/* neighbors_sorted: [n, D] i32, every row ascending (np.sort(matrix.indices.reshape(-1, D))), D <= 32. */
ssw_status ssw_lknn_create(int32_t device, int64_t n, int32_t D, const int32_t *neighbors_sorted_host, ssw_lknn **out);
ssw_status ssw_lknn_destroy(ssw_lknn *h);
/* numer = numerators + gamma with -inf at labelled nodes, denom = denominators + 1 (both [n] f64);
 * top_ids_desc = the K + D nodes of highest numer/denom, best first.  value[i] = s_i (1 + E1_i) + (1 - s_i) E0_i with
 * E_y = sum of the K best scores among the other nodes after labelling i with y (only i's neighbours change).
 * Returns np.nanargmax(value) and its value; out_values (optional) receives all n values.  K <= 128. */
ssw_status ssw_lknn_top_sum(ssw_lknn *h, const double *numer_host, const double *denom_host, const int32_t *top_ids_desc,
                            int32_t K, double *out_values_or_null, int64_t *out_best_idx, double *out_best_value);

/* The device-resident model: LKNNModel's state (numerators, denominators, gamma: f64 [n]; which nodes are seen) kept on
 * the handle, in buffers of its own -- ssw_lknn_top_sum keeps working on the same handle and does not touch them.
 *
 * Order.  Wherever nodes are ranked here the order is total: score descending, node id ascending, seen nodes left out,
 * score = (numerators + gamma) / (denominators + 1) with one rounding per operation.  Whenever the K + D + 1 highest
 * unseen scores are pairwise distinct, every result below equals LKNNModel's bit for bit.  Under exact ties the host
 * model's order comes from np.argpartition and is unspecified; this one is the order just defined, whatever the launch
 * shape.
 *
 * state_init: numerators = denominators = 0, no node seen, gamma installed (finite values; one 8 n-byte upload).
 * set_gamma:  LKNNModel.with_gamma -- replaces gamma, keeps counts and seen marks (one 8 n-byte upload). */
ssw_status ssw_lknn_state_init(ssw_lknn *h, const double *gamma_host);
ssw_status ssw_lknn_set_gamma(ssw_lknn *h, const double *gamma_host);
/* LKNNModel.condition_ for m <= 4096 answers, applied in order: every distinct neighbour j of ids[t] (the handle's table)
 * gets numerators[j] += ys[t], denominators[j] += 1, then ids[t] is marked seen.  Checked on the host before anything
 * is enqueued: ids in range, ys 0 or 1, no id seen already, none twice in the call -- otherwise SSW_ERR_INVALID and the
 * state is as before.  Enqueue only: the host waits for nothing but an earlier call's staging copy still in flight. */
ssw_status ssw_lknn_condition(ssw_lknn *h, const int64_t *ids, const int32_t *ys, int32_t m);
/* One planning step, one host wait, nothing of size n copied to the device.
 * lookahead 2: numer = numerators + gamma (-inf at seen nodes), denom = denominators + 1, the L = K + D best unseen
 *   nodes selected in the same pass over the state, then ssw_lknn_top_sum's kernels on them: np.nanargmax(value) and
 *   its value; out_values (optional) [n] all values, out_list (optional) [K + D] the selected nodes, best first.
 *   1 <= K <= 128, K + D <= 192, K + D <= the number of unseen nodes: otherwise SSW_ERR_INVALID before any launch.
 * lookahead 1 (K ignored): the first index of the largest score among the unseen nodes, and that score; out_values
 *   (optional) the scores, -inf at seen nodes; out_list is not written. */
ssw_status ssw_lknn_step(ssw_lknn *h, int32_t K, int32_t lookahead, int64_t *out_best_idx, double *out_best_value,
                         double *out_values_or_null, int32_t *out_list_or_null);
/* the k <= 192 best unseen nodes, best first, with their scores; *out_count = min(k, unseen nodes).  One host wait. */
ssw_status ssw_lknn_top_remaining(ssw_lknn *h, int32_t k, int32_t *out_ids, double *out_scores, int32_t *out_count);
/* predict_proba: the score of m <= 4096 nodes, seen or not */
ssw_status ssw_lknn_predict(ssw_lknn *h, const int64_t *ids, int32_t m, double *out_scores);
/* the state copied back ([n] each; any pointer may be NULL): tests and debugging */
ssw_status ssw_lknn_state_fetch(ssw_lknn *h, double *numerators, double *denominators, double *gamma, uint8_t *seen_u8);
/* of the last ssw_lknn_step or ssw_lknn_top_remaining: [0] kernel launches, [1] host waits, [2] bytes copied host ->
 * device, [3] bytes copied device -> host */
ssw_status ssw_lknn_step_info(ssw_lknn *h, int64_t *out4);
/* out_ms2 (optional): device-event times in ms of the last step's [0] selection (state pass + merge levels) and [1]
 * look-ahead kernel, -1 where that step was not timed; then steps from now on are timed (enable != 0) or not. */
ssw_status ssw_lknn_step_times(ssw_lknn *h, int32_t enable, double *out_ms2_or_null);

/* Several handles' planning steps in ONE pass of kernels with ONE host wait -- S sessions that plan together share the
 * launches and the wait (ssw_lknn_step alone: 3-8 launches and a wait each).  hs: n_slots <= SSW_LKNN_MAX_BATCH distinct
 * handles with resident state, of one device, one n and one D; K, lookahead: [n_slots].
 * Contract: slot j returns the bits ssw_lknn_step(hs[j], K[j], lookahead[j], ...) returns -- out_best_idx[j],
 * out_best_value[j], out_values[j] ([n], NaN pattern included; the array or any entry may be NULL) and, of a lookahead-2
 * slot, the first K[j] + D entries of row j of out_lists ([n_slots][192]; may be NULL; the rest of a row is not written)
 * -- and like it leaves the model state (numerators, denominators, gamma, seen) untouched.
 * Per-slot refusals: whatever ssw_lknn_step would refuse for that handle (lookahead not 1 or 2, K outside [1, 128], K + D
 * above 192 or above the slot's unseen nodes, no unseen node left) is out_status[j] (SSW_ERR_INVALID) with that call's
 * message in ssw_lknn_batch_error(hs[j]), decided on the host before anything is enqueued for the slot; its outputs are
 * index -1, value 0.  The other slots run and the call returns SSW_OK; a slot that is SSW_OK has "" as its batch error.
 * The pass: one device table of per-slot descriptors (the slot's own state and staging buffers, K, L -- no new O(n)
 * allocation), every kernel launched once with the slot on blockIdx.y and running the single kernel's body: for the
 * lookahead-2 slots the state pass with the selection, the merge levels, mark, look-ahead, unmark; for the lookahead-1
 * slots the score kernel; for all the block argmax and a finish kernel, one workgroup a slot, that reduces the block
 * results on the device by the host loop's rule (largest non-NaN value, lowest index among equals: a total order, so the
 * reduction order does not matter).  The number of launches does not depend on n_slots (1.56 M nodes: 3 + 3 + 2, one
 * more with lookahead-1 slots present); 16 bytes a slot come back, plus the lists and value vectors asked for.
 * Streams: the pass runs on hs[0]'s stream after waiting on an event recorded on every other handle's stream -- answers
 * enqueued with ssw_lknn_condition are seen -- and the call returns with everything complete.  The descriptor table and
 * the pinned result block belong to hs[0], grow on demand and are freed with it.
 * Whole-call refusals (SSW_ERR_INVALID, nothing enqueued, every handle untouched): n_slots outside
 * [1, SSW_LKNN_MAX_BATCH], NULL arrays, a NULL or repeated handle, a handle without resident state, handles of
 * different device, n or D.
 * out_stats4 (may be NULL): [0] kernel launches, [1] host waits (1; 0 when every slot was refused), [2] bytes copied host
 * -> device (the table), [3] bytes copied device -> host.  ssw_lknn_step_info of hs[0] and of every slot that ran
 * reports the same four; with timing enabled on hs[0], ssw_lknn_step_times(hs[0], ...) reports the pass's selection and
 * look-ahead phases (all slots together).
 *
 * ssw_lknn_top_remaining_batch: slot j returns the bits of ssw_lknn_top_remaining(hs[j], k[j], ...) in row j of out_ids /
 * out_scores ([n_slots][192] each) with out_counts[j] = min(k[j], unseen nodes) entries; a slot without an unseen node
 * has count 0 and enqueues nothing; k[j] outside [1, 192] is that slot's refusal.  Same pass (state pass, merge levels,
 * one kernel that gathers the lists), same streams, same whole-call refusals, one host wait. */
#define SSW_LKNN_MAX_BATCH 256
ssw_status ssw_lknn_step_batch(ssw_lknn *const *hs, int32_t n_slots, const int32_t *K, const int32_t *lookahead,
                               int64_t *out_best_idx, double *out_best_value, double *const *out_values_or_null,
                               int32_t *out_lists_or_null, int32_t *out_status, int64_t *out_stats4_or_null);
ssw_status ssw_lknn_top_remaining_batch(ssw_lknn *const *hs, int32_t n_slots, const int32_t *k, int32_t *out_ids,
                                        double *out_scores, int32_t *out_counts, int32_t *out_status);
const char *ssw_lknn_batch_error(const ssw_lknn *h);

/* ------------------------------------------------------------------------- */
/* CLIP ViT-B/32 image / text towers (bf16 MFMA forward)                       */
/* replaces: transformers.CLIPModel.get_text_features                          */
/*               seesaw/models/embeddings.py:441-455 (HGWrapper.from_string)   */
/*           get_image_features + F.normalize                                  */
/*               seesaw/models/model.py:50-57 (HGFaceWrapper.forward),         */
/*               seesaw/indices/multiscale/multiscale_tools.py:187-202          */
/* ------------------------------------------------------------------------- */
typedef struct ssw_clip ssw_clip;

/* weight_blob: 72-byte header ("SSWCLIP1", then int32 v_hidden, v_layers, v_heads, v_mlp,
 * image, patch, t_hidden, t_layers, t_heads, t_mlp, t_max_positions, vocab, eos_token_id,
 * projection_dim, float layer_norm_eps, int32 reserved) followed by the f32 tensors of a
 * transformers.CLIPModel state_dict in the order seesaw_amd/models/clip.py::pack_clip_weights
 * writes them.  GEMM weights are converted to bf16 on the device.
 * Served: head dim 64, hidden / MLP sizes multiples of 128 and hidden <= 1024, an image tower of at most 272 tokens
 * ((image / patch)^2 + 1; any patch size that divides the image: ViT-B/32, ViT-B/16, ViT-L/14 at 224 pixels), a text
 * tower of at most 80 positions.  Anything else is SSW_ERR_UNSUPPORTED, decided before any device call. */
ssw_status ssw_clip_create(int32_t device, const void *weight_blob, size_t bytes, ssw_clip **out);
ssw_status ssw_clip_destroy(ssw_clip *clip);
/* pixel_values [b, 3, image, image] f32 (already CLIP-normalised) -> [b, projection_dim] f32;
 * normalize != 0 L2-normalises every row (HGFaceWrapper). */
ssw_status ssw_clip_embed_image(ssw_clip *clip, const float *nchw_host, int32_t b, int32_t normalize,
                                float *out_host);
/* same with device pointers, enqueued on hip_stream (NULL: the handle's stream), no sync.  At most 1024 images a call,
 * fewer for an image tower above 80 tokens: as many as make 1024 * 80 token rows (ViT-B/16: 415, ViT-L/14: 318). */
ssw_status ssw_clip_embed_image_dev(ssw_clip *clip, void *hip_stream, const float *nchw_dev, int32_t b,
                                    int32_t normalize, float *out_dev);
/* tiles [b, image, image, 3] uint8 (HWC, as cut by the multiscale tiler): batch_tx's
 * `x / 255 -> (x - mean) / std` (seesaw/indices/multiscale/multiscale_tools.py:167-183) is fused into
 * the patch gather, then the same forward pass as ssw_clip_embed_image.  Replaces batch_tx +
 * InferenceActor.__call__ (multiscale_tools.py:187-202). */
ssw_status ssw_clip_embed_tiles_u8(ssw_clip *clip, const uint8_t *tiles_hwc_host, int32_t b, int32_t normalize,
                                   float *out_host);
/* Decoded images -> the vectors of their multiscale tiles, pyramid and tiling on the device (csrc/tiler.hip).  Replaces,
 * for a batch of images, pyramid + rescale + strided_tiling + generate_multiscale_tiling
 * (seesaw/indices/multiscale/multiscale_tools.py:16-117), batch_tx (:167-183) and InferenceActor.__call__ (:187-202).
 *   images_hwc_concat_host: the images' RGB bytes, [h, w, 3] uint8 each, rows tight; image i starts at byte
 *     image_offsets[i] (image_offsets[0] = 0, image_offsets[n_images] = the buffer's size; starts that are multiples of
 *     8 save a device copy for a level of the source's own size).  image_hw[i] = {height, width}, each in 1 .. 16384.
 *   level_wh[level_first[i] .. level_first[i + 1]) = {width, height} of image i's pyramid levels, in the order their tiles
 *     are wanted.  The CALLER names them (seesaw_amd ... multiscale_tools.multiscale_plan: np.geomspace and math.floor
 *     are Python's); every side is at least the tower's image size, the tile size.
 * A level is PIL.Image.resize(size, BILINEAR) of the source, byte for byte (Pillow's 8-bit resample is integer
 * arithmetic: 22-bit fixed-point coefficients, horizontal pass to uint8, then vertical pass); a level of the source's
 * own size is the source.  Tiles per level: for i in (0, 1), for j in (0, 1), the row-major (h' / tile) x (w' / tile) grid
 * of the level shifted by x = i tile / 2, y = j tile / 2.  The tiles are never materialised: the patch gather reads them
 * in place, with batch_tx's arithmetic as in ssw_clip_embed_tiles_u8, and a tile's vector is the one that entry gives
 * for the same bytes.  out_vectors_host [out_cap_tiles, projection_dim] f32 receives the vectors in tile order, image
 * after image; *out_n_tiles their count (also set when out_cap_tiles is too small).
 * Refused with SSW_ERR_INVALID before any device call, the message naming the value: a level side below the tile size,
 * a source or level side outside 1 .. 16384, out_cap_tiles below the count (the message holds the count), offsets that
 * do not hold their image, and a call whose sources, levels, intermediate rows and tables exceed
 * SSW_CLIP_TILER_ARENA_BYTES (hand over fewer images).  The handle stays usable. */
#define SSW_CLIP_TILER_ARENA_BYTES ((int64_t)1 << 30)
ssw_status ssw_clip_embed_multiscale_u8(ssw_clip *clip, const uint8_t *images_hwc_concat_host, int32_t n_images,
                                        const int64_t *image_offsets, const int32_t *image_hw, const int32_t *level_first,
                                        const int32_t *level_wh, int32_t normalize, float *out_vectors_host,
                                        int64_t out_cap_tiles, int64_t *out_n_tiles);
/* input_ids [b, seq_len] int32 (BOS ... EOS [pad]); the feature is taken at the first EOS. */
ssw_status ssw_clip_embed_text(ssw_clip *clip, const int32_t *ids_host, int32_t b, int32_t seq_len,
                               int32_t normalize, float *out_host);
ssw_status ssw_clip_sync(ssw_clip *clip);

/* Per-handle options of the towers' tile path (csrc/clip.hip, run_tower); a handle starts from the environment
 * (SSW_CLIP_BF16_STREAM=1 sets option 0, SSW_CLIP_UNFUSED_ATTN=1 option 3).  Waits for the handle's stream first.
 *   SSW_CLIP_OPT_IMAGE_ROWS_BF16 (0): residual rows of the image tower in bf16 instead of the default f32 rows (SURVEY 8
 *       a-12's arithmetic) -- the precision / throughput choice of an ingest job: 6 % more tiles per second for 4x the score
 *       error (1.5e-3 against 4e-4 on a unit query, tests/test_clip_gpu.py retrieval test); both forms meet the parity bar,
 *       also at ViT-L/14's 24 layers (max |delta| of a unit vector's component 1.6e-3 against 4.0e-4 with f32 rows);
 *   SSW_CLIP_OPT_TEXT_ROWS_BF16 (1): residual rows of the text tower's batched path in bf16 (default f32);
 *   SSW_CLIP_OPT_FULL_LAST_LAYER (4): the image tower's last layer over every row (as the reference's model runs it)
 *       instead of for the pooled rows only -- the embedding reads the first row of an image and nothing else, so the
 *       default runs the last attention for row 0's query only (all keys and values), and the out-projection, fc1 and
 *       fc2 on those B rows.  The vectors differ from the full layer's by 2e-5 ... 5e-5 on unit vectors (measured at
 *       200 tiles; test bar 1e-4, the tower itself is 4e-4 from transformers' f32 model): row 0's attention output and
 *       residual row are the full layer's bit for bit, but the products on B rows select other tile kernels and split
 *       K over workgroups, so sums are taken in another order and a bf16 hidden value may round the other way;
 *   SSW_CLIP_OPT_ATTN_DIRECT (2), SSW_CLIP_OPT_ATTN_OUT_UNFUSED (3): earlier kernel forms of the image tower's attention
 *       (fragments straight from memory; attention and out-projection as two launches) kept for A/B measurements;
 *   SSW_CLIP_OPT_ATTN_LONG (6): attention_long, the kernel of sequences above 80 tokens (ViT-B/16: 197, ViT-L/14: 257), for
 *       shorter sequences too.  Like option 2 it acts only where attention is a launch of its own (the text tower's tile
 *       path; the image tower with option 3 or at widths the fused launch does not serve).  Same arithmetic, same bits:
 *       kept for that comparison (tests/test_clip_variants_gpu.py).  Number 5 stays unknown to ssw_clip_set_option.
 * Not part of the reference's interface (its precision choice is `.half()` on the whole model, embeddings.py:433-435). */
#define SSW_CLIP_OPT_IMAGE_ROWS_BF16 0
#define SSW_CLIP_OPT_TEXT_ROWS_BF16 1
#define SSW_CLIP_OPT_ATTN_DIRECT 2
#define SSW_CLIP_OPT_ATTN_OUT_UNFUSED 3
#define SSW_CLIP_OPT_FULL_LAST_LAYER 4
#define SSW_CLIP_OPT_ATTN_LONG 6
ssw_status ssw_clip_set_option(ssw_clip *clip, int32_t option, int32_t value);

#ifdef __cplusplus
}
#endif
#endif /* SEESAW_HIP_H */

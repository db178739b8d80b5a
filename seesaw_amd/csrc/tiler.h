// Device-side tile pyramid (tiler.hip): the plan of one call -- job table, coefficient table, tile descriptors, arena
// layout -- made on the host without a device call, and the two resample launches that carry it out.  DESIGN.md
// section 4, "Device-side tile pyramid".
#pragma once

#include "ssw_common.h"

namespace ssw {

// What one call's sources, levels, intermediate rows and tables may take of the device (the arena, owned by the
// ssw_clip handle, grows up to this).  A 640 x 480 image with its two levels takes 3.1 MiB, a 3000 x 2000 one with its
// four levels 64 MiB (fifteen a call), an 8192 x 8192 one with its six 719 MiB; a call that needs more is refused and the
// caller splits it
// (seesaw_amd/models/clip.py::TILER_ARENA_BYTES is the same number).
constexpr int64_t TILER_ARENA_MAX_BYTES = SSW_CLIP_TILER_ARENA_BYTES;
constexpr int TILER_MAX_SIDE = 16384;  // of a source or a level

enum : int32_t { TILER_HORIZONTAL = 0, TILER_VERTICAL = 1, TILER_COPY = 2 };

// One pass of one level.  Offsets are bytes from the arena's base; rows are RGB interleaved uint8.
struct TilerJob {
    int64_t src, dst;
    int32_t src_pitch, dst_pitch;
    int32_t src_w, src_h;
    int32_t dst_w, dst_h;
    int32_t coef, ksize;  // the job's coefficient block in the int32 table: [out][2] = (first, n), then [out][ksize] weights
    int32_t first_block;  // of this job inside its launch (256 output pixels a block)
    int32_t kind;
};

// Where a tile sits: rows y0 .. y0 + tile of a level, from pixel x0 on.
struct TileDesc {
    int64_t base;
    int32_t pitch, x0, y0, pad;
};

struct TilerPlan {
    std::vector<TilerJob> jobs[2];  // [0]: horizontal passes and copies (first launch), [1]: vertical passes (second)
    int32_t blocks[2] = {0, 0};
    std::vector<int32_t> coefs;
    std::vector<TileDesc> tiles;           // tile order: image, level, shift, row-major grid
    std::vector<int64_t> level_base;       // per level of the call
    std::vector<int32_t> level_pitch;
    int64_t src_bytes = 0;                 // the concatenated sources, at offset 0 of the arena
    int64_t jobs_off[2] = {0, 0}, coefs_off = 0, tiles_off = 0;  // the tables, behind the levels
    int64_t arena_bytes = 0;
};

// Host only, no device call: checks every size (SSW_ERR_INVALID with the offending value in the message) and lays the
// call out.  min_side = the smallest level side allowed (the tower's tile size; 1 for the lab's single resize).
ssw_status tiler_plan(int tile, int min_side, int32_t n_images, const int64_t *image_offsets, const int32_t *image_hw,
                      const int32_t *level_first, const int32_t *level_wh, TilerPlan *plan);

// Uploads the sources and the tables into `arena` (>= plan.arena_bytes) and runs the two resample launches on `s`.  The host
// buffers are pageable: the caller keeps them and the plan alive until the stream has been synchronised.
ssw_status tiler_run(hipStream_t s, uint8_t *arena, const uint8_t *images_host, const TilerPlan &plan);

}  // namespace ssw

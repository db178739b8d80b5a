"""CPU: multiscale_plan -- the tiling's metadata and the pyramid's level sizes without touching a pixel -- against
generate_multiscale_tiling / pyramid, which cut the pixels.  The device-side pyramid (ClipModel.embed_multiscale_u8) is
told its level sizes by the plan and its vectors are joined to the plan's rows, so the two must not drift: equal
columns, dtypes and float32 bits."""
import numpy as np
import PIL.Image
import pytest

from oracle import seesaw_oracle as orc
from seesaw_amd.indices.multiscale import multiscale_tools as mt

SIZES = list(orc.TILING_SIZES) + [(449, 448), (225, 224), (224, 300), (3000, 2001)]  # (width, height)


@pytest.mark.parametrize("min_tile_size", [224, 112])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_plan_equals_the_tiling_without_its_pixels(size, min_tile_size):
    (w, h) = size
    im = PIL.Image.fromarray(np.zeros((h, w, 3), np.uint8))
    ref = mt.generate_multiscale_tiling(im, tile_size=224, factor=0.5, min_tile_size=min_tile_size).drop(columns="tile")
    levels, meta = mt.multiscale_plan((w, h), tile_size=224, factor=0.5, min_tile_size=min_tile_size)
    assert list(meta.columns) == list(ref.columns)
    assert meta.shape == ref.shape
    assert [str(t) for t in meta.dtypes] == [str(t) for t in ref.dtypes]
    for c in ("x1", "y1", "x2", "y2", "scale_factor"):
        assert meta[c].dtype == np.float32
        assert np.array_equal(meta[c].to_numpy().view(np.uint32), ref[c].to_numpy().view(np.uint32)), c
    for c in ("zoom_level", "patch_id", "max_zoom_level"):
        assert meta[c].dtype == np.int16
        assert np.array_equal(meta[c].to_numpy(), ref[c].to_numpy()), c
    # the level sizes are the sizes of the Pillow images the pyramid makes, for the levels the tiler keeps, in its order
    pdf = mt.pyramid(im, factor=0.5, abs_min=224)
    kept = pdf[(224 / pdf.scale_factor >= min_tile_size) | (pdf.index == 0)]
    assert [(int(a), int(b)) for a, b in zip(levels.w, levels.h)] == [i.size for i in kept.image]
    assert levels.scale_factor.tolist() == kept.scale_factor.tolist()
    assert levels.zoom_level.tolist() == kept.zoom_level.tolist()
    # and the plan's tile count per level is what the strided grid of that size holds
    half = 112
    per_level = [sum(max(lh - sy, 0) // 224 * (max(lw - sx, 0) // 224) for sx in (0, half) for sy in (0, half))
                 for lw, lh in zip(levels.w, levels.h)]
    assert meta.groupby("zoom_level", sort=False).size().tolist() == per_level

"""GPU: the device-side tile pyramid (csrc/tiler.hip, ssw_clip_embed_multiscale_u8).  Pillow's
8-bit bilinear resample is integer arithmetic, so every comparison here is exact: levels against PIL.Image.resize byte
for byte, tiles against the reference tiler's CRCs (tests/golden/tiling.npz, which test_multiscale_tools_cpu.py holds
the host tiler to), vectors against embed_tiles_u8 of the host-made tiles as uint32 bits, the written index against
the host path's.  Towers are small random-init ones (hidden 256, two layers): the tower is not what is tested."""
import ctypes
import io
import os
import zlib

import numpy as np
import PIL.Image
import pytest

import _tiler_helpers as th

pytestmark = pytest.mark.gpu
_MODELS = {}


def _model(patch):
    """a small tower of patch size 32 (aligned gather, 50 tokens) or 14 (scalar gather, 257 tokens), built once"""
    if patch not in _MODELS:
        import transformers
        from seesaw_amd.models.clip import ClipModel
        cfg = transformers.CLIPConfig(
            text_config=dict(hidden_size=128, num_attention_heads=2, intermediate_size=128, num_hidden_layers=2, vocab_size=1000,
                             bos_token_id=998, eos_token_id=999, pad_token_id=0, max_position_embeddings=77,
                             hidden_act="quick_gelu"),
            vision_config=dict(hidden_size=256, num_attention_heads=4, intermediate_size=512, num_hidden_layers=2,
                               image_size=224, patch_size=patch, hidden_act="quick_gelu"),
            projection_dim=512)
        _MODELS[patch] = ClipModel.random_init(seed=77 + patch, config=cfg)
    return _MODELS[patch]


def _plan(size, min_tile_size=224):
    from seesaw_amd.indices.multiscale.multiscale_tools import multiscale_plan
    return multiscale_plan(size, tile_size=224, factor=0.5, min_tile_size=min_tile_size)


def _level_sizes(plan):
    return list(zip(plan[0].w.tolist(), plan[0].h.tolist()))


def _host_tiles(a, min_tile_size=224):
    from seesaw_amd.indices.multiscale.multiscale_tools import generate_multiscale_tiling
    d = generate_multiscale_tiling(PIL.Image.fromarray(a), tile_size=224, factor=0.5, min_tile_size=min_tile_size)
    return np.stack(d.tile.values)


# ---- resize ----------------------------------------------------------------------------------------------------------
RESIZE_PAIRS = [((640, 480), (597, 448)), ((640, 480), (298, 224)),
                ((3000, 2001), (335, 224)),   # a 19-tap window
                ((1024, 231), (512, 224)),    # one axis halves, the other is clamped
                ((100, 80), (280, 224)),      # upscale
                ((225, 224), (224, 224)),     # horizontal pass only
                ((224, 300), (224, 224)),     # vertical pass only
                ((224, 224), (224, 224)),     # no pass: the level is the source
                ((225, 224), (225, 224)),     # no pass, rows of 675 bytes: copied onto the 8-byte pitch
                ((641, 480), (299, 224))]     # rows of 897 bytes (597 x 3 = 1791 above is no multiple of 8 either)


@pytest.mark.parametrize("src,dst", RESIZE_PAIRS, ids=lambda s: f"{s[0]}x{s[1]}")
def test_resize_equals_pillow_byte_for_byte(src, dst):
    from seesaw_amd import _lib
    a = np.random.default_rng(src[0] * 7 + dst[0]).integers(0, 256, (src[1], src[0], 3), dtype=np.uint8)
    ref = np.asarray(PIL.Image.fromarray(a).resize(dst, resample=PIL.Image.BILINEAR))
    model = _model(32)
    with _lib.debug_hooks():
        got = th.device_resize(_lib, model, a, dst[0], dst[1])
    assert got.shape == ref.shape
    if not np.array_equal(got, ref):
        assert np.array_equal(th.resize(a, dst[0], dst[1]), ref), "the numpy twin itself differs from Pillow"
        pytest.fail(f"{src} -> {dst}: {int((got != ref).sum())} bytes differ from Pillow; " + th.which_pass_differs(a, got, *dst))


# ---- tiles against the reference tiler ---------------------------------------------------------------------------------
def _fixture_cases(min_tile_size):
    from oracle import seesaw_oracle as orc
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "tiling.npz"))
    cases = []
    for i, (w, h) in enumerate(orc.TILING_SIZES):
        tag = f"im{i}" if min_tile_size == 224 else f"im{i}_min112"
        if f"{tag}_tile_crc" in g.files:
            cases.append((orc.tiling_image(w, h, seed=100 + i), _plan((w, h), min_tile_size), g[f"{tag}_tile_crc"]))
    assert cases
    return cases


def _crcs(tiles):
    return np.array([zlib.crc32(t.tobytes()) for t in tiles], dtype=np.uint32)


@pytest.mark.parametrize("patch", [32, 14])
@pytest.mark.parametrize("min_tile_size", [224, 112])
def test_tiles_equal_the_reference_tilers(min_tile_size, patch):
    """count, order and bytes of the tiles the gather reads, one image a call and all images in one call"""
    from seesaw_amd import _lib
    cases = _fixture_cases(min_tile_size)
    model = _model(patch)
    with _lib.debug_hooks():
        for k, (a, plan, crc) in enumerate(cases):
            tiles = th.device_tiles(_lib, model, [a], [_level_sizes(plan)])
            assert tiles.shape[0] == len(crc) == len(plan[1]), (k, tiles.shape, len(crc))
            assert np.array_equal(_crcs(tiles), crc), (k, np.nonzero(_crcs(tiles) != crc)[0][:8])
        tiles = th.device_tiles(_lib, model, [c[0] for c in cases], [_level_sizes(c[1]) for c in cases])
    want = np.concatenate([c[2] for c in cases])
    assert tiles.shape[0] == len(want)
    assert np.array_equal(_crcs(tiles), want), np.nonzero(_crcs(tiles) != want)[0][:8]


# ---- vectors ---------------------------------------------------------------------------------------------------------
MIXED = [(640, 480), (224, 224), (225, 900), (100, 80), (500, 375)]  # 13 + 1 + ... tiles


def _images(sizes, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for (w, h) in sizes]


@pytest.mark.parametrize("patch", [32, 14])
@pytest.mark.parametrize("min_tile_size", [224, 112])
def test_vectors_equal_those_of_the_host_made_tiles(min_tile_size, patch):
    model = _model(patch)
    images = _images(MIXED, seed=11)
    plans = [_plan((a.shape[1], a.shape[0]), min_tile_size) for a in images]
    host = np.concatenate([_host_tiles(a, min_tile_size) for a in images])
    if min_tile_size == 224:
        assert len(plans[0][1]) == 13 and len(plans[1][1]) == 1
    want = model.embed_tiles_u8(host, normalize=True)
    got = model.embed_multiscale_u8(images, plans, normalize=True)
    assert got.shape == want.shape == (sum(len(p[1]) for p in plans), model.projection_dim)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), np.nonzero((got != want).any(axis=1))[0][:8]
    raw = model.embed_multiscale_u8(images[:2], plans[:2], normalize=False)
    assert np.array_equal(raw.view(np.uint32), model.embed_tiles_u8(host[:len(raw)], normalize=False).view(np.uint32))


def test_a_chunk_boundary_inside_an_image():
    """257 tokens: a device chunk is 318 tiles; four 94-tile images make 376, so the third image straddles the boundary"""
    from oracle import seesaw_oracle as orc
    model = _model(14)
    a = orc.tiling_image(1344, 896, seed=106)
    plan = _plan((1344, 896))
    assert len(plan[1]) == 94
    host = _host_tiles(a)
    want = model.embed_tiles_u8(np.concatenate([host] * 4), normalize=True)
    got = model.embed_multiscale_u8([a] * 4, [plan] * 4, normalize=True)
    assert got.shape == (376, model.projection_dim)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), np.nonzero((got != want).any(axis=1))[0][:8]


def test_a_list_is_split_under_the_arena_budget():
    """the wrapper hands over as many images a call as the budget admits; the vectors do not depend on the split"""
    model = _model(32)
    images = _images([(640, 480), (300, 260), (500, 375)], seed=3)
    plans = [_plan((a.shape[1], a.shape[0])) for a in images]
    want = model.embed_multiscale_u8(images, plans)
    need = [model.tiler_bytes(a.shape, _level_sizes(p)) for a, p in zip(images, plans)]
    saved = type(model).TILER_ARENA_BYTES
    calls, one_call = [], model._embed_multiscale_call
    model.TILER_ARENA_BYTES = need[0] + need[1]  # -> two calls: images 0 and 1, then image 2
    model._embed_multiscale_call = lambda arrays, sizes, normalize: (calls.append(len(arrays)), one_call(arrays, sizes, normalize))[1]
    try:
        got = model.embed_multiscale_u8(images, plans)
    finally:
        del model.TILER_ARENA_BYTES, model._embed_multiscale_call
    assert type(model).TILER_ARENA_BYTES == saved and calls == [2, 1]
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


# ---- pipeline --------------------------------------------------------------------------------------------------------
def test_create_multiscale_index_writes_the_same_index_either_way(tmp_path):
    import pandas as pd
    from seesaw_amd.indices.multiscale.multiscale_tools import create_multiscale_index, read_vector_parquet
    model = _model(32)
    rows = []
    for dbidx, a in enumerate(_images([(640, 480), (224, 224), (500, 375), (300, 260), (225, 900), (100, 80)], seed=21)):
        buf = io.BytesIO()
        PIL.Image.fromarray(a).save(buf, format="PNG")
        rows.append({"dbidx": dbidx, "file_path": f"img{dbidx}.png", "bytes": buf.getvalue()})
    rows.insert(3, {"dbidx": 6, "file_path": "broken.png", "bytes": b"this is no image"})
    frame = pd.DataFrame(rows)
    read = {}
    for device_tiling in (False, True):
        root = tmp_path / ("device" if device_tiling else "host")
        with pytest.warns(UserWarning, match="error parsing binary broken.png"):
            path = create_multiscale_index(image_rows=frame, dataset_path=str(root), index_name="ix", model=model,
                                           model_path=None, min_tile_size=112, device_tiling=device_tiling)
        read[device_tiling] = read_vector_parquet(f"{path}/vectors.sorted.cached")
    (meta_h, vec_h), (meta_d, vec_d) = read[False], read[True]
    assert 6 not in meta_h.dbidx.values and sorted(set(meta_h.dbidx)) == list(range(6))
    pd.testing.assert_frame_equal(meta_d, meta_h, check_exact=True)
    assert [str(t) for t in meta_d.dtypes] == [str(t) for t in meta_h.dtypes]
    assert vec_d.shape == vec_h.shape and np.array_equal(vec_d.view(np.uint32), vec_h.view(np.uint32))


# ---- refusals --------------------------------------------------------------------------------------------------------
def _good_call_still_works(model):
    a = _images([(300, 260)], seed=5)[0]
    got = model.embed_multiscale_u8([a], [_plan((300, 260))])
    assert np.array_equal(got.view(np.uint32), model.embed_tiles_u8(_host_tiles(a)).view(np.uint32))


def test_refusals_leave_the_handle_usable():
    from seesaw_amd import _lib
    model = _model(32)
    a = _images([(300, 260)], seed=6)[0]
    with pytest.raises(_lib.SeesawHipError) as e:
        model.embed_multiscale_u8([a], [[(223, 224)]])
    assert e.value.status == _lib.SSW_ERR_INVALID and "223 x 224" in str(e.value)
    _good_call_still_works(model)
    with pytest.raises(_lib.SeesawHipError) as e:
        model.embed_multiscale_u8([np.zeros((0, 300, 3), np.uint8)], [[(224, 224)]])
    assert e.value.status == _lib.SSW_ERR_INVALID and "height 0" in str(e.value)
    _good_call_still_works(model)
    # out_cap_tiles one short: 640 x 480 makes 13 tiles
    c = _images([(640, 480)], seed=7)[0]
    buf, offsets, hw, first, wh = th.pack_call([c], [_level_sizes(_plan((640, 480)))])
    out = np.zeros((13, model.projection_dim), np.float32)
    n = ctypes.c_int64(0)
    p = lambda x: ctypes.c_void_p(x.ctypes.data)  # noqa: E731
    with pytest.raises(_lib.SeesawHipError) as e:
        _lib.call("ssw_clip_embed_multiscale_u8", model._h, p(buf), 1, p(offsets), p(hw), p(first), p(wh), 1, p(out), 12,
                  ctypes.byref(n))
    assert e.value.status == _lib.SSW_ERR_INVALID and "13 tiles" in str(e.value) and n.value == 13
    assert not out.any()
    _good_call_still_works(model)
    _lib.call("ssw_clip_embed_multiscale_u8", model._h, p(buf), 1, p(offsets), p(hw), p(first), p(wh), 1, p(out), 13,
              ctypes.byref(n))
    assert n.value == 13 and np.array_equal(out.view(np.uint32), model.embed_tiles_u8(_host_tiles(c)).view(np.uint32))
    for bad in (c.astype(np.float32), c[:, :, 0], c.tolist()):
        with pytest.raises(ValueError, match="uint8"):
            model.embed_multiscale_u8([bad], [_plan((640, 480))])
    _good_call_still_works(model)


def test_a_call_over_the_arena_budget_is_refused_before_the_device():
    from seesaw_amd import _lib
    model = _model(32)
    big = np.zeros((4096, 6144, 3), np.uint8)  # 72 MiB; a 16384 x 16384 level is 768 MiB, its intermediate rows 192 more
    with pytest.raises(_lib.SeesawHipError) as e:
        model.embed_multiscale_u8([big], [[(16384, 16384)]])
    assert e.value.status == _lib.SSW_ERR_INVALID and str(1 << 30) in str(e.value)
    _good_call_still_works(model)

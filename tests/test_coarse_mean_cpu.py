"""The coarse index out of a multiscale index (ssw_index_coarse_mean, seesaw_amd.indices.coarse.preprocessor), the part
that needs no GPU: the ABI entry is declared and bound, the reference's import path resolves, the host selection of the
kept rows and of the images that have one, and the float64 oracle the GPU tests compare with, on a case worked by hand."""
import ctypes

import numpy as np
import pandas as pd
import pytest

from _coarse_helpers import coarse_oracle, make_index, reference_f32, ulp_distance_f16, ulp_distance_f32, unit_rows


def test_entry_is_declared_in_the_header_and_bound():
    from seesaw_amd import _lib
    assert "ssw_index_coarse_mean" in _lib.declared_symbols()
    restype, argtypes = _lib._SIGNATURES["ssw_index_coarse_mean"]
    assert restype is _lib.c_i32 and len(argtypes) == 5 and argtypes[3] is _lib.c_i64
    text = open(_lib.HEADER_PATH).read()
    assert "seesaw/indices/coarse/preprocessor.py" in text  # the reference call site it stands in for
    assert "ssw_index_coarse_mean" not in _lib.declared_symbols(_lib.DEBUG_HEADER_PATH)


def test_null_arguments_are_refused_on_the_host():
    from seesaw_amd import _lib
    lib = _lib.load()
    one = np.zeros(1, dtype=np.int64)
    assert lib.ssw_index_coarse_mean(None, None, None, 0, None) == _lib.SSW_ERR_INVALID
    assert lib.ssw_index_coarse_mean(None, ctypes.c_void_p(one.ctypes.data), ctypes.c_void_p(one.ctypes.data), 1,
                                     None) == _lib.SSW_ERR_INVALID
    assert "NULL" in _lib.last_error()


def test_reference_import_path_resolves_through_the_alias():
    import seesaw.indices.coarse.preprocessor as ref_name
    import seesaw_amd.indices.coarse.preprocessor as own
    assert ref_name is own
    assert callable(ref_name.from_fine_grained) and callable(ref_name.infer_coarse_embedding)
    from seesaw.indices.coarse.preprocessor import from_fine_grained  # noqa: F401
    from seesaw_amd.indices.multiscale.multiscale_index import MultiscaleIndex
    assert callable(MultiscaleIndex.coarse_index)


def test_host_selection_keeps_max_zoom_rows_and_drops_images_without_one():
    from seesaw_amd.device_index import kept_images
    from seesaw_amd.indices.coarse.preprocessor import coarse_keep, coarse_selection
    # image 11: rows at levels 0, 1, 1 of max 1 -> two kept; image 20: levels 0, 1 of max 2 -> none (as after a
    # min_zoom_level filter); image 35: its one row at level 0 of max 0 -> kept
    meta = pd.DataFrame({"dbidx": [11, 11, 11, 20, 20, 35], "zoom_level": [0, 1, 1, 0, 1, 0],
                         "max_zoom_level": [1, 1, 1, 2, 2, 0]})
    keep = coarse_keep(meta)
    assert keep.dtype == np.uint8 and keep.tolist() == [0, 1, 1, 0, 0, 1]
    # the column decides, not the largest level present: image 20's rows reach level 1 only
    assert keep.tolist() != (meta.zoom_level == meta.groupby("dbidx").zoom_level.transform("max")).astype(int).tolist()
    positions, dbidx = coarse_selection(meta.dbidx.values, keep)
    assert positions.tolist() == [0, 2] and dbidx.tolist() == [11, 35]
    assert kept_images(np.array([0, 3, 5, 6]), keep).tolist() == [0, 2]
    assert kept_images(np.array([0, 3, 5, 6]), np.zeros(6)).tolist() == []
    assert kept_images(np.array([0, 1, 2, 3, 4, 5, 6]), keep).tolist() == [1, 2, 5]
    with pytest.raises(ValueError):
        kept_images(np.array([0, 3, 5, 6]), keep[:5])
    with pytest.raises(ValueError, match="max_zoom_level"):
        coarse_keep(meta.drop(columns="max_zoom_level"))


def test_oracle_on_three_images_worked_by_hand():
    X = np.zeros((6, 4), dtype=np.float32)
    X[0] = [9, 9, 9, 9]        # image 0: not kept
    X[1] = [3, 0, 0, 0]        # image 0: kept
    X[2] = [0, 4, 0, 0]        # image 0: kept      -> mean (1.5, 2, 0, 0), norm 2.5 -> (0.6, 0.8, 0, 0)
    X[3] = [0, 0, 2, 0]        # image 1: its one row -> (0, 0, 1, 0)
    X[4] = [1e-8, 0, 0, 0]     # image 2: kept       -> mean (5e-9, 0, 0, -5e-9), norm 7.07e-9 < 1e-6 -> mean / 1e-6
    X[5] = [0, 0, 0, -1e-8]    # image 2: kept
    row_start, keep = np.array([0, 3, 4, 6]), np.array([0, 1, 1, 1, 1, 1])
    out = coarse_oracle(X, row_start, keep, [0, 1, 2])
    assert out.dtype == np.float32 and out.shape == (3, 4)
    assert np.array_equal(out[0], np.array([0.6, 0.8, 0, 0], dtype=np.float32))
    assert np.array_equal(out[1], np.array([0, 0, 1, 0], dtype=np.float32))
    h = np.float64(np.float32(1e-8)) / 2 / 1e-6
    assert np.array_equal(out[2], np.array([h, 0, 0, -h]).astype(np.float32))
    assert np.array_equal(coarse_oracle(X, row_start, keep, [2]), out[2:])  # a row depends on its own image alone
    ref, counts = reference_f32(X, row_start, keep, [0, 1, 2])
    assert counts.tolist() == [2, 1, 2] and ulp_distance_f32(ref[:2], out[:2]).max() <= 1
    with pytest.raises(AssertionError):
        coarse_oracle(X, row_start, np.array([0, 0, 0, 1, 1, 1]), [0])


def test_ulp_distances_and_generator():
    one = np.float32(1)
    up = np.nextafter(one, np.float32(2))
    assert ulp_distance_f32([one, -one, 0.0], [up, -up, -0.0]).tolist() == [1, 1, 0]
    assert ulp_distance_f32([np.float32(1e-45)], [np.float32(-1e-45)]).tolist() == [2]
    assert ulp_distance_f16([np.float16(1)], [np.nextafter(np.float16(1), np.float16(2))]).tolist() == [1]
    g = make_index(3, 40, 256, absent=(4, 9))
    n = g["X"].shape[0]
    assert g["meta"].shape[0] == n == g["row_start"][-1] and g["tiles"].min() == 1 and g["tiles"].max() == 70
    assert np.allclose(np.linalg.norm(g["X"], axis=1), 1, atol=1e-6)
    assert sorted(set(range(40)) - set(g["images"].tolist())) == [4, 9]
    from seesaw_amd.indices.coarse.preprocessor import coarse_keep, coarse_selection
    assert np.array_equal(coarse_keep(g["meta"]), g["keep"])
    assert np.array_equal(coarse_selection(g["meta"].dbidx.values, g["keep"])[0], g["images"])
    # the premise of the f32 bound: every mean of generated rows has norm >= 1/2
    rows = unit_rows(np.random.default_rng(0), 500, 512)
    assert np.linalg.norm(rows.astype(np.float64).mean(axis=0)) >= 0.5
    assert np.linalg.norm(rows[:2].astype(np.float64).mean(axis=0)) >= 0.5

"""Zero-copy subset views (ssw_index_create_view), the part that needs no GPU: the host arithmetic that maps a view's
rows to its parent's, the refusals decided before any device call, and where the view's scan kernels live."""
import ctypes
import os
import re

import numpy as np
import pytest

from seesaw_amd import _lib
from seesaw_amd.device_index import view_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def by_ranges(row_start, positions):
    rows = np.concatenate([np.arange(row_start[p], row_start[p + 1]) for p in positions]).astype(np.int64)
    counts = [row_start[p + 1] - row_start[p] for p in positions]
    return rows, np.concatenate(([0], np.cumsum(counts))).astype(np.int64)


@pytest.mark.parametrize("positions", [
    [0], [6], [0, 6], [2], [1, 2, 3], [0, 1, 2, 3, 4, 5, 6], [0, 2, 4, 6], [1, 3, 5], [5, 6]])
def test_view_rows_equals_concatenated_ranges(positions):
    """images of 1 and of many rows, the first and the last image, single-image runs and runs of several images"""
    counts = [3, 1, 1, 13, 1, 7, 2]  # images 1, 2 and 4 hold one row
    row_start = np.concatenate(([0], np.cumsum(counts))).astype(np.int64)
    rows, start = view_rows(row_start, positions)
    o_rows, o_start = by_ranges(row_start, positions)
    assert rows.dtype == np.int64 and start.dtype == np.int64
    assert np.array_equal(rows, o_rows) and np.array_equal(start, o_start)


def test_view_rows_random_against_ranges():
    rng = np.random.default_rng(3)
    counts = rng.integers(1, 14, size=500)
    row_start = np.concatenate(([0], np.cumsum(counts))).astype(np.int64)
    for frac in (0.01, 0.3, 0.99):
        positions = np.nonzero(rng.random(500) < frac)[0]
        rows, start = view_rows(row_start, positions)
        o_rows, o_start = by_ranges(row_start, positions)
        assert np.array_equal(rows, o_rows) and np.array_equal(start, o_start)
    # an index without an image map: row_start is the identity and the positions are rows
    rows, start = view_rows(np.arange(12), [0, 4, 10])  # 11 rows
    assert rows.tolist() == [0, 4, 10] and start.tolist() == [0, 1, 2, 3]


@pytest.mark.parametrize("positions", [[], [3, 3], [4, 2], [-1, 2], [0, 7]])
def test_view_rows_refuses_bad_positions(positions):
    with pytest.raises(ValueError):
        view_rows(np.arange(8), positions)


def test_create_view_null_arguments_are_invalid_without_a_gpu():
    lib = _lib.load()
    out = ctypes.c_void_p()
    pos = np.array([0, 1], dtype=np.int64)
    assert lib.ssw_index_create_view(None, ctypes.c_void_p(pos.ctypes.data), 2, ctypes.byref(out)) == _lib.SSW_ERR_INVALID
    assert not out.value
    # (NULL positions are refused before the parent is looked at: any non-NULL value stands for it here)
    fake_parent = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(8)))
    assert lib.ssw_index_create_view(None, None, 2, ctypes.byref(out)) == _lib.SSW_ERR_INVALID
    assert lib.ssw_index_create_view(fake_parent, None, 2, ctypes.byref(out)) == _lib.SSW_ERR_INVALID
    assert lib.ssw_index_create_view(fake_parent, ctypes.c_void_p(pos.ctypes.data), 2, None) == _lib.SSW_ERR_INVALID
    assert lib.ssw_index_view_rows(None, None) == _lib.SSW_ERR_INVALID
    assert lib.ssw_abi_version() == 1  # additive: the ABI version stays


def test_abi_lists_the_view_entries():
    declared = _lib.declared_symbols()
    for name in ("ssw_index_create_view", "ssw_index_view_rows"):
        assert name in declared and name in _lib._SIGNATURES, name


def test_view_kernels_are_row_format_templates_in_scan_hip():
    """the view's scan runs the parent scan's lane arithmetic: its two kernels are instances of the `class R, ...`
    row-format template in scan.hip, reduce with dot_frag / group_reduce<U>, and launch_scan_view names both forms"""
    scan = open(os.path.join(ROOT, "seesaw_amd", "csrc", "scan.hip")).read()
    kernels = dict((name, params) for params, name in re.findall(
        r"template <([^>]*)>\s*__global__(?:\s+__launch_bounds__\(\d+\))?\s+void\s+(\w+)\s*\(", scan))
    for name in ("view_scores_kernel", "view_small_kernel"):
        assert name in kernels and kernels[name].startswith("class R,"), (name, kernels.get(name))
        body = scan[scan.index("void %s(" % name):]
        body = body[:body.index("\n}\n")]
        assert "dot_frag<C>(R::widen(" in body and "group_reduce<U>(acc, lane)" in body, name
        assert "__builtin_amdgcn_readlane" not in body and "load_view_group<R, C, U" in body, name
    assert "__builtin_amdgcn_readlane(src, first_lane + u)" in scan
    launcher = scan[scan.index("ssw_status launch_view_t("):scan.index("ssw_status launch_scan_view(")]
    assert "view_small_kernel<R, C, SU>" in launcher and "view_scores_kernel<R, C, U, true>" in launcher
    assert "n <= SCAN_SMALL_ROWS" in launcher
    for fmt in ("F32Rows", "H16Rows"):
        for c in (1, 2, 3, 4):
            assert re.search(r"launch_view_t<%s, %d, \d+>" % (fmt, c), scan), (fmt, c)
    capi = open(os.path.join(ROOT, "seesaw_amd", "csrc", "capi_index.hip")).read()
    assert "launch_scan_view(idx->X, idx->dtype, q_dev, idx->row_src" in capi

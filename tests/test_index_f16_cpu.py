"""CPU: the float16 index's C-ABI entries are declared, exported and bound; the dtype option is parsed and bad values
are refused before any device is touched; SyntheticDataset keeps its cached index per vector dtype."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ssw_index_create_typed", "ssw_index_dtype", "ssw_index_upload_f16", "ssw_fb_set_data_from_index",
       "ssw_fb_set_pseudo_sample_from_index")


@pytest.fixture(scope="module")
def lib():
    from seesaw_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "seesaw_amd", "csrc"), "-j", "4"], check=True)
    return _lib


def test_new_symbols_in_header_library_and_ctypes_table(lib):
    declared = set(lib.declared_symbols())
    nm = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (ssw_[a-z0-9_]+)", nm))
    for name in NEW:
        assert name in declared and name in exported and name in lib._SIGNATURES, name
    text = open(lib.HEADER_PATH).read()
    assert re.search(r"#define SSW_DTYPE_F32 0\b", text) and re.search(r"#define SSW_DTYPE_F16 1\b", text)
    assert (lib.SSW_DTYPE_F32, lib.SSW_DTYPE_F16) == (0, 1)


def test_create_typed_refuses_bad_dtype_and_borrowed_f16_without_a_device(lib):
    h = lib.load()
    out = ctypes.c_void_p()
    assert h.ssw_index_create_typed(0, 10, 512, 7, None, ctypes.byref(out)) == lib.SSW_ERR_UNSUPPORTED
    assert "dtype=7" in lib.last_error() and not out.value
    fake = ctypes.c_void_p(1 << 20)  # never dereferenced: the refusal comes first
    assert h.ssw_index_create_typed(0, 10, 512, lib.SSW_DTYPE_F16, fake, ctypes.byref(out)) == lib.SSW_ERR_UNSUPPORTED
    assert "borrow" in lib.last_error() and not out.value
    assert h.ssw_index_create_typed(0, 10, 500, lib.SSW_DTYPE_F16, None, ctypes.byref(out)) == lib.SSW_ERR_UNSUPPORTED
    assert "dim=500" in lib.last_error()


@pytest.mark.parametrize("spec,want", [(np.float32, np.float32), ("float32", np.float32), ("float16", np.float16),
                                       (np.float16, np.float16), ("f2", np.float16), (np.dtype("<f4"), np.float32)])
def test_vector_dtype_parsed(spec, want):
    from seesaw_amd.device_index import vector_dtype
    assert vector_dtype(spec) == np.dtype(want)


@pytest.mark.parametrize("spec", ["bfloat16", "int8", np.float64, "float", None, "half-ish"])
def test_vector_dtype_rejected(spec):
    from seesaw_amd.device_index import vector_dtype
    with pytest.raises(ValueError):
        vector_dtype(spec)


def test_round_vectors_is_numpy_rounding():
    from seesaw_amd.device_index import round_vectors
    X = np.array([[1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 2.0 ** -25, 3 * 2.0 ** -25, 7e4, 65519.0]], np.float32)
    r = round_vectors(X, "float16")
    assert r.dtype == np.float32
    assert r.tolist() == [[1.0, 1 + 2.0 ** -9, 0.0, 2.0 ** -23, np.inf, 65504.0]]
    assert round_vectors(X, "float32") is not None and np.array_equal(round_vectors(X, np.float32), X)


class _FakeDev:
    """stands in for DeviceIndex: records what the index asked for"""
    made = []

    def __init__(self, vectors, dtype):
        self.vectors, self.dtype = vectors, np.dtype(dtype)

    @classmethod
    def from_numpy(cls, vectors, row2image=None, device=0, dtype=np.float32, **_):
        d = cls(np.array(vectors), dtype)
        cls.made.append(d)
        return d

    def set_tile_meta(self, *a):
        pass


def test_synthetic_load_index_caches_by_dtype(monkeypatch):
    from seesaw_amd import synthetic
    from seesaw_amd.indices.multiscale import multiscale_index
    monkeypatch.setattr(multiscale_index, "DeviceIndex", _FakeDev)
    _FakeDev.made.clear()
    ds = synthetic.make_dataset("f16cache", n_images=40, tiles_per_image=3, seed=2)
    a = ds.load_index(options={"vector_dtype": "float32"})
    b = ds.load_index(options={"vector_dtype": "float16"})
    assert a is not b and a._dev.dtype == np.float32 and b._dev.dtype == np.float16
    assert ds.load_index(options={"vector_dtype": "float16"}) is b
    assert ds.load_index(options={"vector_dtype": "float32"}) is a
    assert ds.load_index() is a and ds.load_index(options={"use_vec_index": True}) is a
    assert len(_FakeDev.made) == 2
    # the f16 index's host rows are the widened rounded rows; the f32 index's are the dataset's own
    assert np.array_equal(b.vectors, ds.vectors.astype(np.float16).astype(np.float32))
    assert np.array_equal(a.vectors, ds.vectors)
    with pytest.raises(ValueError):
        ds.load_index(options={"vector_dtype": "int8"})


def test_f16_and_f32_scans_share_one_lane_arithmetic():
    """the f16 scan's bit-exactness rests on running the f32 scan's RowFrag / dot_frag / group_reduce on widened rows:
    each is defined once under csrc, and every scan kernel of either element type is an instance of one template
    parameterised by the row format"""
    csrc = os.path.join(ROOT, "seesaw_amd", "csrc")
    text = {f: open(os.path.join(csrc, f)).read() for f in os.listdir(csrc) if f.endswith((".hip", ".h"))}
    for pattern in (r"struct RowFrag\s*\{", r"float dot_frag\s*\(", r"float group_reduce\s*\("):
        assert sum(len(re.findall(pattern, t)) for t in text.values()) == 1, pattern
    kernels = re.findall(r"(?:template <([^>]*)>\s*)?__global__(?:\s+__launch_bounds__\(\d+\))?\s+void\s+(\w+)\s*\(",
                         "".join(text.values()))
    kernels = [(params, name) for params, name in kernels if re.search("scan|score_rows", name)]
    assert sorted(name for _, name in kernels) == ["scan_scores_kernel", "scan_small_kernel", "score_rows_kernel"]
    assert all(params.startswith("class R,") for params, _ in kernels), kernels
    scan = text["scan.hip"]
    for fmt in ("F32Rows", "H16Rows"):
        assert re.search(r"launch_scan_t<%s, \d, \d+, (true|false)>" % fmt, scan), fmt
        assert "launch_score_rows_t<%s>" % fmt in scan, fmt

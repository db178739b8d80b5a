"""The coarse index out of a resident multiscale index on the GPU: ssw_index_coarse_mean / DeviceIndex.coarse_mean /
MultiscaleIndex.coarse_index / from_fine_grained.

The oracle is tests/_coarse_helpers.coarse_oracle, the kernel's arithmetic in numpy float64 with one rounding to f32.
Everything before that rounding is float64 on both sides and only the order of the norm's dim-term sum is free (a
relative difference of at most dim * 2^-53), so a result may differ from the oracle only where the exact value sits
that close to a rounding boundary: every element is held to ONE f32 ulp, none is exempted.  An f16 destination rounds
the f32 once more: it is compared with the oracle rounded to binary16 and may be a neighbouring binary16 value."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest

from _coarse_helpers import (coarse_oracle, make_index, reference_f32, ulp_distance_f16, ulp_distance_f32, unit_rows)

pytestmark = pytest.mark.gpu

F16, F32 = np.float16, np.float32
DIMS = (256, 512, 768, 1024)
N_IMAGES = 300
ABSENT = (17, 123)  # images without a row at their max_zoom_level


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def held(X, dtype):
    """the f32 rows an index of that dtype holds"""
    return np.asarray(X).astype(np.float16).astype(np.float32) if dtype == F16 else X


@functools.lru_cache(maxsize=None)
def case(dim):
    """~300 images of 1..70 tiles, ~4 k rows"""
    return make_index(1000 + dim, N_IMAGES, dim, absent=ABSENT)


@functools.lru_cache(maxsize=None)
def want(dim, src):
    g = case(dim)
    return coarse_oracle(held(g["X"], src), g["row_start"], g["keep"], g["images"])


@functools.lru_cache(maxsize=None)
def got(dim, src, dst):
    """the full call (images=None) on the generated index, downloaded"""
    from seesaw_amd.device_index import DeviceIndex
    g = case(dim)
    idx = DeviceIndex.from_numpy(g["X"], row2image=g["row2image"], dtype=src)
    try:
        out = idx.coarse_mean(g["keep"], dtype=dst)
        try:
            assert (out.n_rows, out.dim, out.n_images, out.dtype) == (len(g["images"]), dim, len(g["images"]), np.dtype(dst))
            assert not out.is_view and out._row_start is None
            rows = out.download()
        finally:
            out.close()
    finally:
        idx.close()
    rows.setflags(write=False)
    return rows


def assert_matches(rows, oracle_rows, dst, what):
    """the parity bound of this file"""
    assert rows.shape == oracle_rows.shape and np.isfinite(rows).all()
    if np.dtype(dst) == F16:
        assert np.array_equal(rows, rows.astype(F16).astype(F32))  # (the download widens binary16 values)
        d = ulp_distance_f16(rows.astype(F16), oracle_rows.astype(F16))
    else:
        d = ulp_distance_f32(rows, oracle_rows)
    print(f"{what}: max ulp distance {int(d.max())}, elements off by one {int((d == 1).sum())} of {d.size}")
    assert d.max() <= 1, what


@pytest.mark.parametrize("dst", [F32, F16], ids=["to_f32", "to_f16"])
@pytest.mark.parametrize("src", [F32, F16], ids=["f32", "f16"])
@pytest.mark.parametrize("dim", DIMS)
def test_parity_with_the_float64_oracle(dim, src, dst):
    g = case(dim)
    assert 3000 <= g["X"].shape[0] <= 6000 and len(g["images"]) == N_IMAGES - len(ABSENT)
    rows = got(dim, src, dst)
    assert_matches(rows, want(dim, src), dst, f"dim {dim} {np.dtype(src)} -> {np.dtype(dst)}")
    if np.dtype(dst) == F32:  # unit rows (the rounding of 3 dim operations off at the most)
        assert np.abs(np.linalg.norm(rows.astype(np.float64), axis=1) - 1).max() < 1e-6


class Edges:
    """260 images whose kept sets sit on the kernel's segment edges (a wave walks an image 64 rows at a time and loads
    kept rows two at a time): kept counts 1, 2, 3, 65 and all of 70 and of 130, a kept row that is first / last in its
    image, kept rows on both sides of the 64-row step, in image 0 and in the last image of the source"""

    def __init__(self, dim, seed=5):
        rng = np.random.default_rng(seed)
        special = [3, 1, 5, 4, 6, 70, 130, 70, 66]
        tiles = np.array(special + rng.integers(1, 7, size=260 - len(special) - 1).tolist() + [2], dtype=np.int64)
        self.row_start = np.concatenate(([0], np.cumsum(tiles))).astype(np.int64)
        self.n_images, self.n = tiles.shape[0], int(self.row_start[-1])
        keep = np.zeros(self.n, dtype=np.uint8)
        for i in range(self.n_images):
            t = int(tiles[i])
            keep[self.row_start[i] + rng.permutation(t)[:int(rng.integers(1, t + 1))]] = 1
        self.kept = {}

        def put(i, local):
            keep[self.row_start[i]:self.row_start[i + 1]] = 0
            keep[self.row_start[i] + np.asarray(local)] = 1
            self.kept[i] = len(local)

        put(0, [0])                                       # image 0: one kept row, the first of the source
        put(1, [0])                                       # a one-tile image
        put(2, [4])                                       # one kept row, the last of its image
        put(3, [0, 3])                                    # two: first and last
        put(4, [1, 2, 4])                                 # three
        put(5, [j for j in range(70) if j not in (10, 30, 31, 50, 69)])  # 65 of 70, rows 63 and 64 among them
        put(6, list(range(130)))                          # every row, three 64-row steps
        put(7, list(range(70)))                           # every row
        put(8, [63, 64, 65])                              # both sides of the step, and the last row
        put(self.n_images - 1, [1])                       # the last image: the last row of the source
        self.keep = keep
        self.row2image = np.repeat(np.arange(self.n_images, dtype=np.int32), tiles)
        self.X = unit_rows(rng, self.n, dim)


@pytest.mark.parametrize("dim,src", [(512, F32), (768, F16), (1024, F32), (256, F16)])
def test_segment_edges(dim, src):
    from seesaw_amd.device_index import DeviceIndex
    e = Edges(dim)
    assert [e.kept[i] for i in (0, 1, 2, 3, 4, 5, 6, 7, 8)] == [1, 1, 1, 2, 3, 65, 130, 70, 3]
    W = held(e.X, src)
    every = np.arange(e.n_images, dtype=np.int64)
    oracle_rows = coarse_oracle(W, e.row_start, e.keep, every)
    idx = DeviceIndex.from_numpy(e.X, row2image=e.row2image, dtype=src)
    try:
        def run(images):
            out = idx.coarse_mean(e.keep, images=images)
            try:
                return out.download()
            finally:
                out.close()

        full = run(None)
        assert_matches(full, oracle_rows, F32, f"edges dim {dim} {np.dtype(src)}")
        # exactly one kept row: that row, normalised
        for i, local in ((0, 0), (1, 0), (2, 4), (e.n_images - 1, 1)):
            row = W[e.row_start[i] + local].astype(np.float64)
            assert ulp_distance_f32(full[i], (row / np.linalg.norm(row)).astype(F32)).max() <= 1
        # m = 1, 5, 257: the same rows, bit for bit, whatever else the call lists
        for images in ([0], [e.n_images - 1], [0, 5, 6, 8, e.n_images - 1], list(range(3, 260))):
            part = run(np.array(images))
            assert len(images) in (1, 5, 257) and part.shape == (len(images), dim)
            assert np.array_equal(bits(part), bits(full[images]))
    finally:
        idx.close()


def test_degenerate_norms():
    from seesaw_amd.device_index import DeviceIndex
    dim = 512
    rng = np.random.default_rng(8)
    v = unit_rows(rng, 1, dim)[0]
    tiny = (unit_rows(rng, 2, dim, direction=v.astype(np.float64)).astype(np.float64) * 1e-8).astype(F32)
    X = np.concatenate([np.zeros((3, dim), F32), np.stack([v, -v]), tiny, unit_rows(rng, 2, dim)])
    row2image = np.array([0, 0, 0, 1, 1, 2, 2, 3, 3], dtype=np.int32)
    row_start = np.array([0, 3, 5, 7, 9])
    keep = np.ones(9, dtype=np.uint8)
    idx = DeviceIndex.from_numpy(X, row2image=row2image)
    try:
        out = idx.coarse_mean(keep)
        try:
            rows = out.download()
        finally:
            out.close()
    finally:
        idx.close()
    assert np.isfinite(rows).all()
    assert not rows[0].any() and not rows[1].any()  # all kept rows zero; v and -v: a zero row, not NaN
    mean = tiny.astype(np.float64).sum(axis=0) / 2
    assert np.linalg.norm(mean) < 1e-6  # under the floor: mean / 1e-6
    assert ulp_distance_f32(rows[2], (mean / 1e-6).astype(F32)).max() <= 1 and rows[2].any()
    assert_matches(rows, coarse_oracle(X, row_start, keep, np.arange(4)), F32, "degenerate norms")


@pytest.mark.parametrize("src,dst", [(F32, F32), (F16, F16)], ids=["f32", "f16"])
def test_a_row_depends_on_its_own_image_alone(src, dst):
    from seesaw_amd.device_index import DeviceIndex
    dim = 512
    g = case(dim)
    full = got(dim, src, dst)
    idx = DeviceIndex.from_numpy(g["X"], row2image=g["row2image"], dtype=src)
    try:
        again = idx.coarse_mean(g["keep"], dtype=dst)
        try:
            assert again.download().tobytes() == full.tobytes()  # the full call twice: equal bytes
        finally:
            again.close()
        for j in (0, 1, 57, 150, len(g["images"]) - 1):  # (image 1 has 70 tiles)
            one = idx.coarse_mean(g["keep"], images=[int(g["images"][j])], dtype=dst)
            try:
                assert np.array_equal(bits(one.download()[0]), bits(full[j])), j
            finally:
                one.close()
    finally:
        idx.close()


@pytest.mark.parametrize("src", [F32, F16], ids=["f32", "f16"])
def test_view_source_equals_the_parent_call(src):
    from seesaw_amd.device_index import DeviceIndex
    dim = 768
    g = case(dim)
    full = got(dim, src, F32)
    members = np.arange(0, N_IMAGES, 3, dtype=np.int64)
    idx = DeviceIndex.from_numpy(g["X"], row2image=g["row2image"], dtype=src)
    try:
        v = idx.view(members)
        try:
            keep_v = g["keep"][v.parent_rows]
            out = v.coarse_mean(keep_v)  # keep and the default images in the VIEW's numbering
            try:
                rows = out.download()
            finally:
                out.close()
        finally:
            v.close()
    finally:
        idx.close()
    with_row = members[np.isin(members, g["images"])]
    assert 0 < with_row.shape[0] < members.shape[0]  # image 123 is a member without a kept row
    assert np.array_equal(bits(rows), bits(full[np.searchsorted(g["images"], with_row)]))


def _multiscale(g, dtype="float32"):
    from seesaw_amd.indices.multiscale.multiscale_index import MultiscaleIndex
    return MultiscaleIndex(embedding=None, vectors=g["X"], vector_meta=g["meta"], vector_dtype=dtype)


def test_subset_view_multiscale_index_gives_an_owning_coarse_index_of_the_subset():
    from seesaw_amd.bitmap import BitMap
    dim = 512
    g = case(dim)
    ms = _multiscale(g)
    whole = ms.coarse_index()
    all_dbidx = np.unique(g["meta"].dbidx.values)
    sub = ms.subset_view(BitMap(all_dbidx[::3]))
    assert sub._dev.is_view
    part = sub.coarse_index()
    assert not part._dev.is_view and part._dev.parent is None and len(part) < len(sub)
    pos = np.searchsorted(whole._dbidx, part._dbidx)
    assert np.array_equal(whole._dbidx[pos], part._dbidx)
    assert np.array_equal(part._dbidx, np.intersect1d(all_dbidx[::3], whole._dbidx))
    assert np.array_equal(bits(part.vectors), bits(whole.vectors[pos]))
    assert np.array_equal(bits(part._dev.download()), bits(part.vectors))
    assert np.array_equal(bits(whole.vectors), bits(got(dim, F32, F32)))
    q = g["X"][11]
    a = part.query(topk=10, vector=q)
    b = whole.subset(BitMap(part._dbidx)).query(topk=10, vector=q)
    assert np.array_equal(a["dbidxs"], b["dbidxs"])
    # vector_dtype defaults to the source's
    half = _multiscale(g, "float16").coarse_index()
    assert half.vector_dtype == np.dtype(F16) and half._dev.dtype == np.dtype(F16)
    assert np.array_equal(bits(half.vectors), bits(got(dim, F16, F16)))


def test_refusals_are_host_checks_with_status_and_message():
    from seesaw_amd import _lib
    from seesaw_amd.device_index import DeviceIndex
    lib = _lib.load()
    dim = 256
    g = case(dim)
    keep, images = g["keep"], g["images"]
    src = DeviceIndex.from_numpy(g["X"], row2image=g["row2image"])
    before = unit_rows(np.random.default_rng(2), 4, dim)
    dst = DeviceIndex.from_numpy(before)
    nomap = DeviceIndex.from_numpy(g["X"][:100])
    wrong_dim = DeviceIndex(4, 512)
    view = dst.view([0, 1, 2, 3])
    try:
        def call(s, k, im, d):
            im = np.ascontiguousarray(im, dtype=np.int64)
            return lib.ssw_index_coarse_mean(s._h, _p(np.ascontiguousarray(k, dtype=np.uint8)), _p(im), im.shape[0], d._h)

        four = images[:4]
        INVALID, UNSUPPORTED = _lib.SSW_ERR_INVALID, _lib.SSW_ERR_UNSUPPORTED
        for name, args, status, word in (
                ("unsorted", (src, keep, four[[0, 2, 1, 3]], dst), INVALID, "ascending"),
                ("repeated", (src, keep, four[[0, 1, 1, 3]], dst), INVALID, "ascending"),
                ("past the map", (src, keep, [0, 1, 2, N_IMAGES], dst), INVALID, "outside"),
                ("negative", (src, keep, [-1, 1, 2, 3], dst), INVALID, "outside"),
                ("no kept row", (src, keep, [0, 1, ABSENT[0], 200], dst), INVALID, "no kept row"),
                ("dst of another n", (src, keep, images[:5], dst), INVALID, "need [5, 256]"),
                ("dst of another dim", (src, keep, four, wrong_dim), INVALID, "need [4, 256]"),
                ("a view as dst", (src, keep, four, view), UNSUPPORTED, "view"),
                ("src without a map", (nomap, np.ones(100), [0, 1, 2, 3], dst), UNSUPPORTED, "image map"),
                ("dst is src", (src, keep, four, src), INVALID, "rows src reads")):
            assert call(*args) == status and word in _lib.last_error(), (name, _lib.last_error())
        assert np.array_equal(bits(dst.download()), bits(before))  # nothing was written
        # the Python layer raises with the library's status
        with pytest.raises(_lib.SeesawHipError) as err:
            src.coarse_mean(keep, images=[3, 2])
        assert err.value.status == _lib.SSW_ERR_INVALID
        with pytest.raises(_lib.SeesawHipError) as err:
            nomap.coarse_mean(np.ones(100), images=[0, 1])
        assert err.value.status == _lib.SSW_ERR_UNSUPPORTED
        with pytest.raises(ValueError):
            src.coarse_mean(keep[:-1])
        # and the handles still work
        ok = src.coarse_mean(keep, images=four)
        try:
            assert np.array_equal(bits(ok.download()), bits(got(dim, F32, F32)[:4]))
        finally:
            ok.close()
    finally:
        view.close()
        for h in (src, dst, nomap, wrong_dim):
            h.close()


@pytest.mark.parametrize("dst_dtype", [F32, F16], ids=["f32", "f16"])
def test_destination_that_already_answered_a_topk(dst_dtype):
    """dst's rows count as changed, as after ssw_index_upload: the next top-k reads the new rows"""
    from seesaw_amd import _lib
    from seesaw_amd.device_index import DeviceIndex
    dim = 512
    g = case(dim)
    m = len(g["images"])
    rng = np.random.default_rng(4)
    q = unit_rows(rng, 1, dim)[0]
    src = DeviceIndex.from_numpy(g["X"], row2image=g["row2image"])
    dst = DeviceIndex.from_numpy(unit_rows(rng, m, dim, noise=2.0), dtype=dst_dtype)
    try:
        old = dst.topk(q, 10)
        _lib.call("ssw_index_coarse_mean", src._h, _p(g["keep"]), _p(g["images"]), m, dst._h)
        rows = dst.download()
        assert np.array_equal(bits(rows), bits(got(dim, F32, dst_dtype)))
        new = dst.topk(q, 10)
        fresh = DeviceIndex.from_numpy(rows, dtype=dst_dtype)
        try:
            ref = fresh.topk(q, 10)
        finally:
            fresh.close()
        assert np.array_equal(new[0], ref[0]) and np.array_equal(bits(new[1]), bits(ref[1])) and np.array_equal(new[2], ref[2])
        assert not np.array_equal(new[0], old[0])
    finally:
        dst.close()
        src.close()


def test_end_to_end_from_fine_grained(tmp_path):
    from seesaw_amd.indices.coarse.coarse_index import CoarseIndex
    from seesaw_amd.indices.coarse.preprocessor import from_fine_grained
    from seesaw_amd.indices.multiscale.multiscale_index import MultiscaleIndex
    from seesaw_amd.indices.multiscale.multiscale_tools import write_vector_parquet
    dim = 512
    g = case(dim)
    fine = tmp_path / "indices" / "multiscale"
    os.makedirs(fine)
    info = {"constructor": "seesaw.indices.multiscale.multiscale_index.MultiscaleIndex", "model": "synthetic:random-init",
            "dataset": str(tmp_path)}
    json.dump(info, open(fine / "info.json", "w"))
    write_vector_parquet(g["meta"].assign(vectors=list(g["X"])), str(fine / "vectors.sorted.cached"))
    out_path = str(tmp_path / "indices" / "coarse")
    assert from_fine_grained(str(fine), out_path) == os.path.realpath(out_path)
    assert sorted(os.listdir(tmp_path / "indices")) == ["coarse", "multiscale"]  # no .tmp.coarse left behind
    out_info = json.load(open(f"{out_path}/info.json"))
    assert out_info == {"constructor": "seesaw.indices.coarse.coarse_index.CoarseIndex", "model": info["model"],
                        "dataset": info["dataset"]}
    vectors = np.load(f"{out_path}/vectors.npy")
    assert vectors.dtype == F32 and vectors.shape == (len(g["images"]), dim)
    assert_matches(vectors, want(dim, F32), F32, "vectors.npy")
    with pytest.raises(FileExistsError):
        from_fine_grained(str(fine), out_path)
    loaded = CoarseIndex.from_path(out_path)
    expect_dbidx = np.unique(g["meta"].dbidx.values)[g["images"]]
    assert np.array_equal(loaded._dbidx, expect_dbidx) and np.all(np.diff(loaded._dbidx) > 0)
    assert list(loaded.vector_meta.columns) == ["dbidx"]
    ms = MultiscaleIndex.from_path(str(fine))
    assert "max_zoom_level" in ms.vector_meta
    direct = ms.coarse_index()
    assert direct.embedding is ms.embedding
    assert np.array_equal(direct._dbidx, expect_dbidx)
    assert np.array_equal(bits(direct.vectors), bits(vectors)) and np.array_equal(bits(direct._dev.download()), bits(vectors))
    q = g["X"][g["row_start"][40]]
    a, b = direct.query(topk=10, vector=q), loaded.query(topk=10, vector=q)
    assert a["dbidxs"].shape == (10,) and np.array_equal(a["dbidxs"], b["dbidxs"])


@pytest.mark.parametrize("dim", DIMS)
def test_distance_from_the_reference_f32_arithmetic(dim):
    """against infer_coarse_embedding as the reference runs it, in f32: every component within 4 (c + 4) 2^-24, c the
    image's kept rows.  The sequential f32 sum of c unit-bounded terms is off by at most (c - 1) 2^-24 after the
    division; normalising by a norm >= 1/2 at most doubles that; the rest covers the division and the final rounding.
    Observed on an MI355X: see DESIGN.md section 5."""
    g = case(dim)
    ref, counts = reference_f32(g["X"], g["row_start"], g["keep"], g["images"])
    rows = got(dim, F32, F32)
    bound = 4.0 * (counts + 4) * 2.0 ** -24
    diff = np.abs(rows.astype(np.float64) - ref.astype(np.float64))
    ratio = diff.max(axis=1) / bound
    print(f"dim {dim}: max |device - f32 reference| = {diff.max():.3e}, largest share of the bound {ratio.max():.4f} "
          f"(image of c = {int(counts[ratio.argmax()])}), c up to {int(counts.max())}")
    assert (diff <= bound[:, None]).all()

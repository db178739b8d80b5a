"""GPU: both stages of the multiscale lookup for a batch (ssw_index_topk_batch_avg, csrc/rescore.hip:
k_avg_score_keys).  The first stage is `topk_batch`'s bytes; every candidate's aggregated score and best tile are the
BITS `topk(Q[b])` followed by `rescore_avg` returns on a second handle over the same rows, and for 'level_max' the bits
of the numpy oracle fed the batch's own tile scores; `MultiscaleIndex.query_batch` equals the loop of `query` entry by
entry.  Every comparison is exact.

Index A is the smallest shape at which every path is reached: 9 000 images (more than the one-launch selection's
8 192, so the histogram selection writes the keys), tile counts cycling over 1, 5 and 21 (a three-level pyramid of
overlapping f32 boxes), one image of a single zero-area box (no partner at all: NaN), one of 300 tiles (more than the
kernel's 256 threads: its strided loops run twice), ~81 000 rows (the multi-query scan kernel's range).  Index B is
the golden pyramid of tests/golden/multiscale_query.npz: per-query scan launches and the one-launch selection."""
import os

import numpy as np
import pandas as pd
import pytest

from _prune_helpers import same

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
NQS = (1, 2, 3, 16, 19)  # 19 is cut as 16 + 2 + 1
K = 50
AUGS = ("all", "greater", "adjacent")
WEIGHTS = ("level_max", "cont_weighted")
N_IMAGES_A, NAN_IMAGE, BIG_IMAGE = 9000, 3000, 4001
ZOOMS = (1, 2, 4)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def pyramid(w, h, levels):
    """level l: a 2^l x 2^l grid of tiles 1.5 cells wide, so neighbours overlap -> (boxes f32 [T, 4], zoom [T])"""
    boxes, zoom = [], []
    for l in range(levels):
        g = 1 << l
        sw, sh = (w, h) if g == 1 else (w / g * 1.5, h / g * 1.5)
        for iy in range(g):
            for ix in range(g):
                x1 = 0.0 if g == 1 else ix * (w - sw) / (g - 1)
                y1 = 0.0 if g == 1 else iy * (h - sh) / (g - 1)
                boxes.append((x1, y1, x1 + sw, y1 + sh))
                zoom.append(ZOOMS[l])
    return np.asarray(boxes, dtype=np.float32), np.asarray(zoom, dtype=np.int32)


def geometry_a():
    rng = np.random.default_rng(11)
    boxes, zoom, counts = [], [], []
    for i in range(N_IMAGES_A):
        w, h = 200 + 37.3 * (i % 11), 150 + 29.7 * (i % 7)
        if i == NAN_IMAGE:
            b, z = np.array([[10, 10, 10, 50]], dtype=np.float32), np.array([ZOOMS[0]], dtype=np.int32)
        elif i == BIG_IMAGE:  # the whole image, then 99 and 200 random boxes
            x1, y1 = rng.uniform(0, 0.8 * w, 299), rng.uniform(0, 0.8 * h, 299)
            rnd = np.stack([x1, y1, x1 + rng.uniform(0.1, 0.3, 299) * w, y1 + rng.uniform(0.1, 0.3, 299) * h], axis=1)
            b = np.concatenate([[[0, 0, w, h]], rnd]).astype(np.float32)
            z = np.repeat(ZOOMS, (1, 99, 200)).astype(np.int32)
        else:
            b, z = pyramid(w, h, 1 + i % 3)  # 1, 5, 21 tiles
        boxes.append(b)
        zoom.append(z)
        counts.append(b.shape[0])
    counts = np.asarray(counts)
    assert counts[BIG_IMAGE] == 300 and counts[NAN_IMAGE] == 1 and set(counts[:3]) == {1, 5, 21}
    return np.concatenate(boxes), np.concatenate(zoom), np.repeat(np.arange(N_IMAGES_A), counts).astype(np.int32)


def queries(oracle, nq, first=0):
    return np.stack([oracle.synth_query(first + i) * np.float32(1.0 + 0.1 * i) for i in range(nq)])


class Case:
    """the rows and tile geometry of one index, two handles over them (`a` runs the batch, `b` the single calls), and
    the single-call results, computed once per exclusion list"""

    def __init__(self, name, X, row2image, boxes, zoom, Q):
        self.name, self.X, self.row2image, self.boxes, self.zoom, self.Q = name, X, row2image, boxes, zoom, Q
        self.n_images = int(row2image[-1]) + 1
        self.row_start = np.concatenate(([0], np.cumsum(np.bincount(row2image))))
        self.a, self.b = self.handle(X), self.handle(X)
        self._single = {}

    def handle(self, X, dtype=np.float32):
        from seesaw_amd.device_index import DeviceIndex
        idx = DeviceIndex.from_numpy(X, row2image=self.row2image, dtype=dtype)
        idx.set_tile_meta(self.boxes, self.zoom)
        return idx

    def single(self, b, aug, weight, excluded=None, tag="none"):
        """(images, scores, rows, avg_scores, avg_rows) of query b by topk + rescore_avg on handle `b`"""
        if (b, tag) not in self._single:
            top = self.b.topk(self.Q[b], K, excluded=excluded)
            self._single[(b, tag)] = {(g, w): top + self.b.rescore_avg(top[0], g, aug_weight=w)
                                      for g in AUGS for w in WEIGHTS}
        return self._single[(b, tag)][(aug, weight)]

    def close(self):
        self.a.close()
        self.b.close()


@pytest.fixture(scope="module")
def case_a(oracle):
    boxes, zoom, row2image = geometry_a()
    assert row2image.shape[0] >= 65536
    c = Case("A", oracle.synth_rows(19, 0, row2image.shape[0], 512), row2image, boxes, zoom, queries(oracle, max(NQS)))
    yield c
    c.close()


def golden_pyramid(oracle):
    g = np.load(os.path.join(GOLDEN, "multiscale_query.npz"))
    m = g["pyr_meta"]
    meta = pd.DataFrame({"dbidx": m[:, 0].astype(np.int64), "zoom_level": m[:, 1].astype(np.int16),
                         "x1": m[:, 2].astype(np.float32), "y1": m[:, 3].astype(np.float32),
                         "x2": m[:, 4].astype(np.float32), "y2": m[:, 5].astype(np.float32)})
    return meta, oracle.synth_rows(int(g["pyr_seed"]), 0, meta.shape[0], 512)


@pytest.fixture(scope="module")
def case_b(oracle):
    meta, X = golden_pyramid(oracle)
    row2image = np.unique(meta.dbidx.values, return_inverse=True)[1].astype(np.int32)
    assert row2image[-1] + 1 <= 8192 and X.shape[0] <= 65536 and row2image[-1] + 1 > K
    c = Case("B", X, row2image, meta[["x1", "y1", "x2", "y2"]].values.astype(np.float32),
             meta.zoom_level.values.astype(np.int32), queries(oracle, max(NQS), first=100))
    yield c
    c.close()


@pytest.fixture(params=["A", "B"])
def case(request):
    return request.getfixturevalue("case_" + request.param.lower())


@pytest.mark.parametrize("nq", NQS)
def test_batch_is_topk_batch_then_rescore_avg_per_query(case, nq):
    Q = case.Q[:nq]
    first = case.a.topk_batch(Q, K)
    for aug in AUGS:
        for weight in WEIGHTS:
            got = case.a.topk_batch_avg(Q, K, aug, aug_weight=weight)
            assert len(got) == nq
            for b in range(nq):
                same(first[b], got[b][:3])
                same(case.single(b, aug, weight), got[b])
                assert got[b][0].shape[0] == K


@pytest.mark.parametrize("aug", AUGS)
def test_level_max_is_the_oracle_on_the_batchs_own_tile_scores(case, oracle, aug):
    tile_scores = case.a.scores_batch(case.Q)
    memo = {}

    def expect(b, p):
        if (b, p) not in memo:
            r0, r1 = case.row_start[p], case.row_start[p + 1]
            if case.name == "A" and p == NAN_IMAGE:  # no partner at all: NaN, represented by its first tile
                memo[(b, p)] = (r0, np.float32(np.nan))
            else:
                j, sc, _ = oracle.avg_score_image(case.boxes[r0:r1], case.zoom[r0:r1], tile_scores[b, r0:r1], aug)
                memo[(b, p)] = (r0 + j, np.float32(sc))
        return memo[(b, p)]

    for nq in NQS:
        for b, (imgs, _, _, avg_scores, avg_rows) in enumerate(case.a.topk_batch_avg(case.Q[:nq], K, aug)):
            ref = [expect(b, int(p)) for p in imgs]
            assert avg_rows.tolist() == [r for r, _ in ref], (nq, b)
            assert np.array_equal(bits(avg_scores), bits([s for _, s in ref])), (nq, b)


def test_per_query_excluded_lists(case):
    """none, 100 images, all but 3: count < k, and the slots beyond it are never read"""
    keep = np.array([NAN_IMAGE, BIG_IMAGE, 17] if case.name == "A" else [3, 17, 40])
    lists = {"none": None, "hundred": (np.arange(100) * 2 + 1).tolist(), "but3": np.setdiff1d(np.arange(case.n_images), keep)}
    tags = [("none", "hundred", "but3")[(b + 1) % 3] for b in range(max(NQS))]  # query 0 excludes 100 images
    for nq in (3, 19):
        excluded = [lists[t] for t in tags[:nq]]
        first = case.a.topk_batch(case.Q[:nq], K, excluded=excluded)
        for aug, weight in (("all", "level_max"), ("greater", "cont_weighted"), ("adjacent", "level_max")):
            got = case.a.topk_batch_avg(case.Q[:nq], K, aug, excluded=excluded, aug_weight=weight)
            for b in range(nq):
                same(first[b], got[b][:3])
                same(case.single(b, aug, weight, lists[tags[b]], tags[b]), got[b])
                assert got[b][0].shape[0] == (3 if tags[b] == "but3" else K)
            if case.name == "A":
                imgs, _, _, avg_scores, avg_rows = got[1]  # all but 3
                assert sorted(imgs.tolist()) == sorted(keep.tolist())
                at = imgs.tolist().index(NAN_IMAGE)
                assert np.isnan(avg_scores[at]) and avg_rows[at] == case.row_start[NAN_IMAGE]


def test_mass_ties_take_the_deep_selection_inside_the_batch(case_a, oracle):
    """every row the same vector: all 9 000 images tie, the fast selection overflows and the deep path runs for
    every query of the batch, before its second stage"""
    X = np.broadcast_to(oracle.synth_rows(1, 0, 1, 512), case_a.X.shape)
    idx = case_a.handle(X)
    try:
        for nq in (1, 3):
            got = idx.topk_batch_avg(case_a.Q[:nq], K, "all")
            for b in range(nq):
                top = idx.topk(case_a.Q[b], K)
                assert top[0].tolist() == list(range(K))  # ties go to the lowest position
                same(top + idx.rescore_avg(top[0], "all"), got[b])
    finally:
        idx.close()


def test_f16_rows_equal_the_f32_index_of_the_widened_rows(case_a):
    half = case_a.handle(case_a.X, dtype=np.float16)
    wide = case_a.handle(case_a.X.astype(np.float16).astype(np.float32))
    try:
        for aug, weight in (("all", "level_max"), ("greater", "cont_weighted")):
            got = half.topk_batch_avg(case_a.Q, K, aug, aug_weight=weight)
            ref = wide.topk_batch_avg(case_a.Q, K, aug, aug_weight=weight)
            for g, r in zip(got, ref):
                same(r, g)
    finally:
        half.close()
        wide.close()


@pytest.mark.parametrize("nq", NQS)
def test_state_afterwards_is_the_last_querys(case, nq):
    excluded = [list(range(i, 290, 7)) for i in range(nq)]
    res = case.a.topk_batch_avg(case.Q[:nq], K, "greater", excluded=excluded)
    last = case.b.topk(case.Q[nq - 1], K, excluded=excluded[-1])
    same(last, res[-1][:3])
    same(last, case.a.topk(None, K, excluded=excluded[-1]))
    probe = np.arange(0, case.X.shape[0], 97)
    assert np.array_equal(bits(case.a.gather_scores(probe)), bits(case.b.scores(case.Q[nq - 1])[probe]))
    same(case.b.rescore_avg(last[0], "greater"), case.a.rescore_avg(last[0], "greater"))


def test_errors_come_before_anything_runs(case_b):
    from seesaw_amd import _lib
    from seesaw_amd.device_index import DeviceIndex
    a, Q = case_b.a, case_b.Q[:3]
    before = a.topk(Q[0], K)
    avg_scores, avg_rows, counts = np.empty(3 * K, np.float32), np.empty(3 * K, np.int64), np.zeros(3, np.int32)
    with pytest.raises(_lib.SeesawHipError) as e:  # aug_larger = 3 is no code
        _lib.call("ssw_index_topk_batch_avg", a._h, Q.ctypes.data, 3, None, None, K, 3, None, None, None,
                  avg_scores.ctypes.data, avg_rows.ctypes.data, counts.ctypes.data)
    assert e.value.status == _lib.SSW_ERR_INVALID and "aug_larger=3" in str(e.value)
    bare = DeviceIndex.from_numpy(case_b.X, row2image=case_b.row2image)  # no tile meta
    try:
        with pytest.raises(_lib.SeesawHipError) as e:
            bare.topk_batch_avg(Q, K, "all")
        assert e.value.status == _lib.SSW_ERR_INVALID and "set_tile_meta" in str(e.value)
    finally:
        bare.close()
    same(before, a.topk(None, K))


# ---- MultiscaleIndex.query_batch against the loop of query -------------------------------------------------------------
def same_entries(got, ref):
    assert len(got) == len(ref)
    for g, r in zip(got, ref):
        assert np.array_equal(g["dbidxs"], r["dbidxs"]) and g["dbidxs"].dtype == r["dbidxs"].dtype
        if isinstance(r["activations"], list):
            assert g["activations"] == r["activations"] == []
            continue
        ga, ra = np.asarray(g["activations"].records()), np.asarray(r["activations"].records())
        assert ga.shape == ra.shape and np.array_equal(ga.view(np.uint64), ra.view(np.uint64))  # (NaN scores too)


@pytest.fixture(scope="module")
def multiscale_a(case_a):
    from seesaw_amd.indices.multiscale.multiscale_index import MultiscaleIndex
    b = case_a.boxes
    meta = pd.DataFrame({"dbidx": case_a.row2image.astype(np.int64) * 3 + 1, "zoom_level": case_a.zoom.astype(np.int16),
                         "x1": b[:, 0], "y1": b[:, 1], "x2": b[:, 2], "y2": b[:, 3]})
    index = MultiscaleIndex(embedding=None, vectors=case_a.X, vector_meta=meta)
    yield index
    index._dev.close()


@pytest.fixture(scope="module")
def multiscale_b(oracle):
    from seesaw_amd.indices.multiscale.multiscale_index import MultiscaleIndex
    meta, X = golden_pyramid(oracle)
    index = MultiscaleIndex(embedding=None, vectors=X, vector_meta=meta)
    yield index
    index._dev.close()


@pytest.mark.parametrize("which", ["A", "B"])
def test_query_batch_is_the_loop_of_query(request, which, case_a, case_b):
    from seesaw_amd.bitmap import BitMap
    from seesaw_amd.indices.interface import AccessMethod
    index = request.getfixturevalue("multiscale_" + which.lower())
    Q = (case_a if which == "A" else case_b).Q
    ids = index._dbidx
    keep = ids[[NAN_IMAGE, BIG_IMAGE, 17]] if which == "A" else ids[[3, 17, 40]]
    pool = [None, BitMap(ids[:100].tolist()), BitMap(ids.tolist()), BitMap(np.setdiff1d(ids, keep).tolist()), BitMap()]
    vectors = [q for q in Q[:7]]
    excludes = [pool[i % len(pool)] for i in range(7)]  # entry 2 covers the index, entry 3 leaves 3 images
    settings = [dict(agg_method="plain_score", aug_larger="all")]
    settings += [dict(agg_method="avg_score", aug_larger=g, aug_weight=w) for g in AUGS for w in WEIGHTS]
    for kw in settings:
        kw = dict(kw, topk=10, shortlist_size=50, rescore_method=None)
        got = index.query_batch(vectors=vectors, excludes=excludes, **kw)
        assert np.array_equal(index._resident_q, Q[6])
        ref = AccessMethod.query_batch(index, vectors=vectors, excludes=excludes, **kw)
        same_entries(got, ref)
        assert got[2]["dbidxs"].shape[0] == 0 and got[3]["dbidxs"].shape[0] == 3 and got[0]["dbidxs"].shape[0] == 10
        same_entries(index.query_batch(vectors=vectors, **kw), AccessMethod.query_batch(index, vectors=vectors, **kw))
    # `vector2` keeps going through the loop
    kw = dict(topk=10, shortlist_size=50, agg_method="avg_score", aug_larger="greater", rescore_method=None,
              vector2=Q[9])
    same_entries(index.query_batch(vectors=vectors[:2], **kw), [index.query(vector=v, exclude=None, **kw) for v in vectors[:2]])


@pytest.mark.parametrize("agg_method", ["plain_score", "avg_score"])
def test_sixteen_queries_are_one_scan_launch(multiscale_a, case_a, agg_method):
    dev = multiscale_a._dev
    dev.profile(True)
    try:
        got = multiscale_a.query_batch(vectors=[q for q in case_a.Q[:16]], topk=10, shortlist_size=50,
                                       agg_method=agg_method, aug_larger="greater", rescore_method=None)
        launches = dev.profile_read().shape[0]
    finally:
        dev.profile(False)
    assert len(got) == 16 and launches == 1, launches

"""GPU: the second stage of a batch of two-vector queries (ssw_index_stage2_pair_batch; csrc/rescore.hip, k_pair_score)
through `DeviceIndex.stage2_pair` on ONE handle, against the same computation composed from the single entries on a SECOND
handle over the same rows: `scores(q)` (resident), `score_rows(q2, rows)`, and then
  avg:   `rescore_avg(positions, aug, minus, aug_weight)` -- the device runs the same aggregation on the same differences,
         so the comparison is on bit patterns (NaN aggregates included) and there is no tolerance to choose;
  plain: numpy on `scores(q) - score_rows(q2, rows)`: the first tile with the highest non-NaN difference, an image of
         NaN differences alone gives its first row and NaN (what np.lexsort((arange, -s, dbidx)) picks in
         rescore_candidates).  Scores are compared on bit patterns except that any NaN equals any NaN.

Layouts as tests/test_stage2_owner_gpu.py: `_rescore_helpers.Layout()` at dim 256, the 1 / 3 / 4 / 5 / 8 / 13-tile layout at
dims 512, 768 and 1024; f32 and f16 rows."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _rescore_helpers import AUGS, DIM, Layout  # noqa: E402
from test_stage2_owner_gpu import SmallLayout  # noqa: E402

pytestmark = pytest.mark.gpu

NQ_MAX = 16
K = 20
WEIGHTS = ("level_max", "cont_weighted")
FILL_SCORE, FILL_ROW = np.float32(-12345.5), np.int64(-77)
Q2_ZERO, Q2_SAME = 4, 5  # queries whose second vector is 0 / the first vector


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_scores(got, want):
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got[~nan]), bits(want[~nan]))


def plain_per_image(d, row_start):
    """numpy: per image (the highest non-NaN d or NaN, the row of its first tile with it or the image's first row)"""
    n = row_start.shape[0] - 1
    score, row = np.empty(n, dtype=np.float32), np.empty(n, dtype=np.int64)
    for p in range(n):
        seg = d[row_start[p]:row_start[p + 1]]
        if np.isnan(seg).all():
            score[p], row[p] = np.nan, row_start[p]
        else:
            i = int(np.nanargmax(seg))  # the first maximum
            score[p], row[p] = seg[i], row_start[p] + i
    return score, row


class Pair:
    """`dut` runs the entry, `ref` composes the expectation; NQ_MAX query pairs; per query what every image should give"""

    def __init__(self, oracle, layout, dim, dtype):
        from seesaw_amd.device_index import DeviceIndex
        self.lay, self.dim, self.dtype = layout, dim, dtype
        X = oracle.synth_rows(4242 + dim, 0, layout.n_rows, dim)
        self.Q = np.stack([oracle.synth_query(900 + b, dim) for b in range(NQ_MAX)])
        self.Q2 = np.stack([oracle.synth_query(1900 + b, dim) for b in range(NQ_MAX)])
        if isinstance(layout, Layout):  # column 0 carries the planted scores; queries 0 .. 3 = c * e_0 read them back
            planted = layout.scores(np.float32)
            X[:, 0] = np.clip(planted, -60000.0, 60000.0) if dtype == "float16" else planted
            for b, c in enumerate((1.0, 2.0, 0.5, -1.0)):
                self.Q[b] = Layout.query(c)
            self.Q2[0], self.Q2[1] = Layout.query(0.25), Layout.query(-1.0)
        self.Q2[Q2_ZERO] = 0.0
        self.Q2[Q2_SAME] = self.Q[Q2_SAME]
        self.X = X
        self.dut, self.ref = (self.make(DeviceIndex) for _ in range(2))
        self.positions = np.arange(layout.n_images, dtype=np.int64)
        self.all_rows = np.arange(layout.n_rows, dtype=np.int64)
        self.d, self.plain, self.avg = [], [], {}
        for b in range(NQ_MAX):  # computed once, shared by every test below
            v = self.ref.scores(self.Q[b])  # (and resident on `ref`)
            v2 = self.ref.score_rows(self.Q2[b], self.all_rows)
            with np.errstate(invalid="ignore"):
                self.d.append(v - v2)
            self.plain.append(plain_per_image(self.d[b], layout.row_start))
            for aug in AUGS:
                for wgt in WEIGHTS:
                    self.avg[b, aug, wgt] = self.ref.rescore_avg(self.positions, aug, v2, aug_weight=wgt)

    def make(self, DeviceIndex):
        idx = DeviceIndex.from_numpy(self.X, row2image=self.lay.row2image, device=0, dtype=self.dtype)
        idx.set_tile_meta(self.lay.boxes, self.lay.zoom)
        return idx

    def want(self, b, agg, aug, wgt):
        return self.plain[b] if agg == "plain_score" else self.avg[b, aug, wgt]

    def lists(self, nq, seed):
        """per query its own UNSORTED list: every image once, shuffled, then repeats; counts cycle through K, 0 and 7"""
        rng = np.random.default_rng(seed)
        n = self.lay.n_images
        assert n <= K
        pos = np.stack([np.concatenate([rng.permutation(n), rng.integers(0, n, K - n)]) for _ in range(nq)]).astype(np.int64)
        counts = np.array([(K, 0, 7)[b % 3] for b in range(nq)], dtype=np.int32)
        return pos, counts

    def check(self, queries, agg, aug="all", wgt="level_max", seed=0):
        queries = list(queries)
        nq = len(queries)
        pos, counts = self.lists(nq, seed)
        scores, rows = np.full((nq, K), FILL_SCORE), np.full((nq, K), FILL_ROW)
        got = self.dut.stage2_pair(self.Q[queries], self.Q2[queries], pos, counts, agg, aug_larger=aug, aug_weight=wgt,
                                   out=(scores, rows))
        assert got[0] is scores and got[1] is rows
        for j, b in enumerate(queries):
            m = int(counts[j])
            ws, wr = self.want(b, agg, aug, wgt)
            assert np.array_equal(rows[j, :m], wr[pos[j, :m]]), (agg, aug, wgt, nq, j, b)
            if agg == "plain_score":
                assert same_scores(scores[j, :m], ws[pos[j, :m]]), (agg, nq, j, b)
            else:
                assert np.array_equal(bits(scores[j, :m]), bits(ws[pos[j, :m]])), (agg, aug, wgt, nq, j, b)
            # a slot at or past the count is left untouched
            assert (bits(scores[j, m:]) == bits(FILL_SCORE.reshape(1))[0]).all() and (rows[j, m:] == FILL_ROW).all()

    def close(self):
        self.dut.close()
        self.ref.close()


@pytest.fixture(scope="module", params=[("edges", 256, "float32"), ("edges", 256, "float16"),
                                        ("small", 512, "float32"), ("small", 512, "float16"),
                                        ("small", 768, "float32"), ("small", 768, "float16"),
                                        ("small", 1024, "float32"), ("small", 1024, "float16")],
                ids=lambda p: "-".join(str(v) for v in p))
def pair(request, oracle):
    which, dim, dtype = request.param
    s = Pair(oracle, Layout() if which == "edges" else SmallLayout(), dim, dtype)
    yield s
    s.close()


QUERIES = {1: [7], 3: [6, 0, 9], 16: list(range(16)), 19: list(range(16)) + [2, 1, 0]}


@pytest.mark.parametrize("nq", [1, 3, 16, 19])
def test_avg_is_rescore_avg_with_the_minus_form(pair, nq):
    """every aug_larger and both aug_weights; counts 0, 7 and K; unsorted positions; the all-NaN image is in every list"""
    case = 0
    for aug in AUGS:
        for wgt in WEIGHTS:
            pair.check(QUERIES[nq], "avg_score", aug, wgt, seed=100 * nq + case)
            case += 1


@pytest.mark.parametrize("nq", [1, 3, 16, 19])
def test_plain_is_the_first_tile_with_the_highest_difference(pair, nq):
    pair.check(QUERIES[nq], "plain_score", seed=31 * nq)


def test_zero_and_equal_second_vectors(pair):
    """q2 = 0: the differences are the scan's scores; q2 = q: exact zeros, so every image ties on its first row"""
    lay = pair.lay
    assert np.array_equal(bits(pair.d[Q2_ZERO]), bits(pair.ref.scores(pair.Q[Q2_ZERO])))
    assert (bits(pair.d[Q2_SAME]) == 0).all()  # +0.0
    assert np.array_equal(pair.plain[Q2_SAME][1], lay.row_start[:-1]) and (bits(pair.plain[Q2_SAME][0]) == 0).all()
    for agg in ("plain_score", "avg_score"):
        pair.check([Q2_ZERO, Q2_SAME, Q2_ZERO], agg, "greater", "level_max", seed=11)
    # q2 = 0, plain: the per-image maximum and its tile are the first stage's own
    pos, sc, best = pair.ref.topk(pair.Q[Q2_ZERO], lay.n_images)
    assert np.array_equal(best, pair.plain[Q2_ZERO][1][pos]) and same_scores(sc, pair.plain[Q2_ZERO][0][pos])


def test_the_all_zero_area_image_aggregates_to_nan(pair):
    p = pair.lay.all_nan_position
    for b in (0, 7):
        s, r = pair.avg[b, "all", "level_max"]
        assert np.isnan(s[p]) and r[p] == pair.lay.row_start[p]
    pos = np.full((2, 3), p, dtype=np.int64)
    s, r = pair.dut.stage2_pair(pair.Q[[0, 7]], pair.Q2[[0, 7]], pos, [3, 1], "avg_score", aug_larger="all")
    assert np.isnan(s[0]).all() and np.isnan(s[1, 0]) and (r[0] == pair.lay.row_start[p]).all()


def test_the_handle_is_left_as_it_was(pair):
    idx = pair.dut
    idx.topk(pair.Q[5], 5, excluded=[1])
    before = (idx.gather_scores(pair.all_rows), idx.topk(None, 5), idx.prune_stats(completions=True))
    pair.check(range(16), "avg_score", "all", "level_max", seed=1)
    pair.check([3, 2, 1], "plain_score", seed=2)
    after = (idx.gather_scores(pair.all_rows), idx.topk(None, 5), idx.prune_stats(completions=True))
    assert np.array_equal(bits(before[0]), bits(after[0]))
    assert all(np.array_equal(a, b) for a, b in zip(before[1], after[1]))
    assert before[2] == after[2]
    assert np.array_equal(bits(after[0]), bits(pair.ref.scores(pair.Q[5])))  # (and those were query 5's)


# ---- differences that are NaN: inf - inf -----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float16"])
def test_nan_differences(dtype):
    """rows x * e_0 against q = 1e35 e_0 and q2 = 2e35 e_0: x = +-60000 overflows both products to the same infinity, so
    d = NaN; x = 1, 0.5, -2 gives the finite d = -x 1e35.  Image 0: all NaN; image 1: mixed, the best finite tile third;
    image 2: mixed with a NaN first; image 3: finite; image 4: one NaN tile."""
    from seesaw_amd.device_index import DeviceIndex
    xs = [[60000, -60000, 60000, 60000, -60000], [60000, 1, -2, 0.5, -2, -60000, 1, 60000, -2], [-60000, 0.5, 0.5, 60000],
          [1, 0.5, -2, -2, 1, 0.5], [60000]]
    counts = [len(x) for x in xs]
    row_start = np.concatenate(([0], np.cumsum(counts))).astype(np.int64)
    X = np.zeros((int(row_start[-1]), DIM), dtype=np.float32)
    X[:, 0] = np.concatenate(xs)
    r2i = np.repeat(np.arange(len(xs)), counts).astype(np.int32)
    rng = np.random.default_rng(3)
    boxes = np.tile(np.float32([0, 0, 64, 64]), (X.shape[0], 1)) + 16 * rng.integers(0, 3, (X.shape[0], 1)).astype(np.float32)
    zoom = rng.integers(0, 2, X.shape[0]).astype(np.int32)
    q, q2 = Layout.query(1e35), Layout.query(2e35)
    with np.errstate(over="ignore", invalid="ignore"):
        d = (X[:, 0] * np.float32(1e35)).astype(np.float32) - (X[:, 0] * np.float32(2e35)).astype(np.float32)
    assert np.isnan(d[:5]).all() and np.isnan(d[5]) and not np.isnan(d[6:9]).any()
    want_s, want_r = plain_per_image(d, row_start)
    assert np.isnan(want_s[0]) and want_r[0] == 0 and want_r[1] == row_start[1] + 2 and want_r[2] == row_start[2] + 1
    dut, ref = (DeviceIndex.from_numpy(X, row2image=r2i, device=0, dtype=dtype) for _ in range(2))
    try:
        for h in (dut, ref):
            h.set_tile_meta(boxes, zoom)
        pos = np.array([[4, 2, 0, 1, 3], [0, 1, 2, 3, 4]], dtype=np.int64)
        Q, Q2 = np.stack([q, q]), np.stack([q2, q2])
        s, r = dut.stage2_pair(Q, Q2, pos, [5, 5], "plain_score")
        for b in range(2):
            assert np.array_equal(r[b], want_r[pos[b]]) and same_scores(s[b], want_s[pos[b]])
        with np.errstate(over="ignore", invalid="ignore"):
            assert same_scores(ref.scores(q) - ref.score_rows(q2, np.arange(X.shape[0])), d)  # (the composition is that d)
        v2 = ref.score_rows(q2, np.arange(X.shape[0]))
        for aug in AUGS:
            ws, wr = ref.rescore_avg(np.arange(len(xs)), aug, v2)
            s, r = dut.stage2_pair(Q, Q2, pos, [5, 5], "avg_score", aug_larger=aug)
            for b in range(2):
                assert np.array_equal(r[b], wr[pos[b]]) and np.array_equal(bits(s[b]), bits(ws[pos[b]])), aug
    finally:
        dut.close()
        ref.close()


# ---- refusals: all decided on the host ---------------------------------------------------------------------------------
def raw_call(idx, Q, Q2, nq, pos, counts, k, agg=1, aug=0):
    from seesaw_amd import _lib
    s, r = np.zeros(max(1, nq * k), dtype=np.float32), np.zeros(max(1, nq * k), dtype=np.int64)
    p = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    _lib.call("ssw_index_stage2_pair_batch", idx._h, p(Q), p(Q2), nq, p(pos), p(counts), k, agg, aug, p(s), p(r))


def test_refusals(pair, oracle):
    from seesaw_amd import _lib
    from seesaw_amd.device_index import DeviceIndex
    Q, Q2 = np.ascontiguousarray(pair.Q[:2]), np.ascontiguousarray(pair.Q2[:2])
    pos, counts = np.zeros((2, 4), dtype=np.int64), np.array([4, 4], dtype=np.int32)

    def refused(status, fn, word=None):
        with pytest.raises(_lib.SeesawHipError) as e:
            fn()
        assert e.value.status == status, str(e.value)
        assert word is None or word in str(e.value)

    view = pair.dut.view([0, 1])
    try:
        for agg in ("plain_score", "avg_score"):
            refused(_lib.SSW_ERR_UNSUPPORTED, lambda: view.stage2_pair(Q, Q2, pos, counts, agg), "view")
    finally:
        view.close()
    n = 40  # (the small layout has 42 rows)
    bare = DeviceIndex.from_numpy(pair.X[:n], row2image=(np.arange(n) // 4).astype(np.int32), device=0, dtype=pair.dtype)
    try:
        refused(_lib.SSW_ERR_UNSUPPORTED, lambda: bare.stage2_pair(Q, Q2, pos, counts, "avg_score"), "set_tile_meta")
        s, r = bare.stage2_pair(Q, Q2, pos, counts, "plain_score")  # plain needs no tile meta
        with np.errstate(invalid="ignore"):
            d = bare.scores(Q[1]) - bare.score_rows(Q2[1], np.arange(n))
        ws, wr = plain_per_image(d, np.arange(0, n + 1, 4))
        assert (r[1] == wr[0]).all() and same_scores(s[1], np.repeat(ws[:1], 4))
    finally:
        bare.close()
    for bad in (-1, pair.lay.n_images):
        p2 = pos.copy()
        p2[1, 3] = bad
        refused(_lib.SSW_ERR_INVALID, lambda: pair.dut.stage2_pair(Q, Q2, p2, counts, "plain_score"), "position")
        pair.dut.stage2_pair(Q, Q2, p2, [4, 3], "plain_score")  # (a slot past the count is not read)
    refused(_lib.SSW_ERR_INVALID, lambda: raw_call(pair.dut, Q, Q2, 2, pos, counts, 0))
    big = np.zeros((2, _lib.SSW_MAX_TOPK + 1), dtype=np.int64)
    refused(_lib.SSW_ERR_INVALID, lambda: raw_call(pair.dut, Q, Q2, 2, big, counts, _lib.SSW_MAX_TOPK + 1))
    refused(_lib.SSW_ERR_INVALID, lambda: raw_call(pair.dut, Q, Q2, 0, pos, counts, 4))
    refused(_lib.SSW_ERR_INVALID, lambda: raw_call(pair.dut, Q, Q2, 2, pos, np.array([4, 5], dtype=np.int32), 4))
    refused(_lib.SSW_ERR_INVALID, lambda: raw_call(pair.dut, Q, Q2, 2, pos, counts, 4, agg=2))
    refused(_lib.SSW_ERR_INVALID, lambda: raw_call(pair.dut, Q, Q2, 2, pos, counts, 4, agg=1, aug=3))
    Qbad = Q.copy()
    Qbad[1, 3] = np.inf
    refused(_lib.SSW_ERR_NUMERIC, lambda: pair.dut.stage2_pair(Qbad, Q2, pos, counts, "plain_score"))
    refused(_lib.SSW_ERR_NUMERIC, lambda: pair.dut.stage2_pair(Q, Qbad, pos, counts, "avg_score"))


def test_an_image_of_too_many_tiles_is_refused(oracle):
    from seesaw_amd import _lib
    from seesaw_amd.device_index import DeviceIndex
    n = DeviceIndex.RESCORE_MAX_TILES + 1 + 3
    r2i = np.concatenate([np.zeros(3), np.ones(n - 3)]).astype(np.int32)
    idx = DeviceIndex.from_numpy(oracle.synth_rows(5, 0, n, DIM), row2image=r2i, device=0)
    try:
        idx.set_tile_meta(np.tile(np.float32([0, 0, 32, 32]), (n, 1)), np.zeros(n, dtype=np.int32))
        Q = np.stack([oracle.synth_query(1, DIM)])
        for agg in ("plain_score", "avg_score"):  # even for a list that names the small image alone
            with pytest.raises(_lib.SeesawHipError) as e:
                idx.stage2_pair(Q, Q, np.zeros((1, 1), dtype=np.int64), [1], agg)
            assert e.value.status == _lib.SSW_ERR_UNSUPPORTED and "tiles" in str(e.value)
    finally:
        idx.close()

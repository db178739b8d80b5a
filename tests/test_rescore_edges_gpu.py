"""GPU: the three entries of csrc/rescore.hip -- k_avg_score<float> (rescore_avg), k_avg_score<double> (rescore_avg_f64),
k_avg_score_keys (topk_batch_avg) -- on the edge layouts of tests/_rescore_helpers.py: 1 .. 2048 tiles per image (more
tiles than the 256 threads; 2048 tiles are the LDS ceiling: 64 KiB of dynamic LDS for f32 scores, 80 KiB for f64), zoom
levels up to 31, exactly tied IoUs / scores / aggregates, a zero-area box, NaN and infinite scores, an image whose
aggregates are all NaN.  Bit for bit against the numpy oracle and the reference's own results
(tests/golden/avg_score_edges.npz) for 'level_max'; within the derived bound (2P + 8) * 2**-24 * A of the float64 oracle
for 'cont_weighted'.  The golden leaves the all-NaN image out (the reference raises on it): the oracle covers it.

Finite scores enter through the scan exactly (row i is s_i * e_0, the query c * e_0); NaN / inf through load_scores."""
import os

import numpy as np
import pytest

import _rescore_helpers as H

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "avg_score_edges.npz")
DTYPES = {"f32": np.float32, "f64": np.float64}


def bits(a):
    a = np.asarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same_bits(a, b):
    """equal bit for bit, any NaN equal to any NaN"""
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


@pytest.fixture(scope="module")
def g():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def lay():
    return H.Layout()


@pytest.fixture(scope="module")
def idx(lay):
    from seesaw_amd.device_index import DeviceIndex
    index = DeviceIndex.from_numpy(lay.vectors(), row2image=lay.row2image)
    index.set_tile_meta(lay.boxes, lay.zoom)
    yield index
    index.close()


@pytest.fixture(scope="module")
def ref(lay, oracle):
    """(aug, dtype name, scores name[, 'cw']) -> the oracle's per-image (rows in the index, scores[, P, A, aggregates]),
    computed once"""
    cache = {}

    def get(aug, dt, sc, weight="level_max"):
        key = (aug, dt, sc, weight)
        if key not in cache:
            s = lay.scores(DTYPES[dt], loaded=sc != "fin")
            if sc == "ldm":
                s = s - lay.minus()
            per_image = [oracle.avg_score_image(lay.boxes[lay.rows(p)], lay.zoom[lay.rows(p)], s[lay.rows(p)], aug,
                                                dtype=DTYPES[dt], aug_weight=weight) for p in range(lay.n_images)]
            rows = lay.row_start[:-1] + np.asarray([r[0] for r in per_image], dtype=np.int64)
            cache[key] = (rows, np.asarray([r[1] for r in per_image]), per_image)
        return cache[key]
    return get


def check_level_max(lay, g, ref, got_scores, got_rows, aug, dt, sc):
    tag = f"lm_{aug}_{dt}_{sc}"
    want_rows, want_scores, _ = ref(aug, dt, sc)
    assert np.array_equal(got_rows, want_rows), (tag, got_rows - lay.row_start[:-1], want_rows - lay.row_start[:-1])
    assert same_bits(got_scores, want_scores.astype(DTYPES[dt])), (tag, got_scores, want_scores)
    keep = np.arange(lay.n_images) != lay.all_nan_position  # the golden holds every other image
    assert np.array_equal(got_rows[keep] - lay.row_start[:-1][keep], g[f"row_{tag}"]), tag
    assert same_bits(got_scores[keep], g[f"score_{tag}"]), tag
    a = lay.all_nan_position
    assert np.isnan(got_scores[a]) and got_rows[a] == lay.row_start[a], (tag, got_scores[a], got_rows[a])


@pytest.mark.parametrize("aug", H.AUGS)
def test_rescore_avg_level_max_equals_oracle_and_reference(lay, g, ref, idx, aug):
    """k_avg_score<float> over ALL images (2048 tiles: exactly 64 KiB of dynamic LDS): the scan's finite scores, loaded
    scores with NaN / +inf / -inf, and those minus a vector on every image"""
    pos = np.arange(lay.n_images, dtype=np.int64)
    idx.scan(lay.query(1.0))
    assert same_bits(idx.gather_scores(np.arange(lay.n_rows)), lay.scores(np.float32))  # the scores entered exactly
    check_level_max(lay, g, ref, *idx.rescore_avg(pos, aug), aug, "f32", "fin")
    idx.load_scores(lay.scores(np.float32, loaded=True))
    check_level_max(lay, g, ref, *idx.rescore_avg(pos, aug), aug, "f32", "ld")
    check_level_max(lay, g, ref, *idx.rescore_avg(pos, aug, minus_scores=lay.minus()), aug, "f32", "ldm")
    # candidates in another order, some of them twice: one workgroup each, the same answers
    order = np.asarray([12, 0, 9, 12, 7, 13, 1], dtype=np.int64)
    sc, rows = idx.rescore_avg(order, aug)
    want_rows, want_scores, _ = ref(aug, "f32", "ld")
    assert np.array_equal(rows, want_rows[order]) and same_bits(sc, want_scores[order].astype(np.float32))


@pytest.mark.parametrize("aug", H.AUGS)
def test_rescore_avg_f64_level_max_equals_oracle_and_reference(lay, g, ref, idx, aug):
    """k_avg_score<double> over a float64 score tensor on the device; 2048 tiles take 80 KiB of LDS (the raised limit)"""
    import torch
    pos = np.arange(lay.n_images, dtype=np.int64)
    for sc in ("fin", "ld"):
        dev = torch.from_numpy(lay.scores(np.float64, loaded=sc == "ld")).cuda()
        got_scores, got_rows = idx.rescore_avg_f64(dev.data_ptr(), pos, aug)
        check_level_max(lay, g, ref, got_scores, got_rows, aug, "f64", sc)


@pytest.mark.parametrize("aug", H.AUGS)
def test_topk_batch_avg_equals_rescore_avg_per_query(lay, g, ref, idx, aug):
    """k_avg_score_keys: 3 queries c * e_0, c in {1, 2, 0.5} (the scores scale exactly), k = the number of images and more:
    avg_*[i] is what rescore_avg returns for images[i] under that query's scores -- the 2048-tile image included -- and
    for c = 1 what the oracle and the reference return"""
    cs = [1.0, 2.0, 0.5]
    Q = np.stack([lay.query(c) for c in cs])
    for k in (lay.n_images, lay.n_images + 6):
        res = idx.topk_batch_avg(Q, k, aug)
        assert len(res) == 3
        for c, (images, scores, rows, avg_scores, avg_rows) in zip(cs, res):
            assert sorted(images.tolist()) == list(range(lay.n_images)), (k, c, images)
            idx.scan(lay.query(c))
            want_scores, want_rows = idx.rescore_avg(images, aug)
            assert np.array_equal(avg_rows, want_rows) and same_bits(avg_scores, want_scores), (aug, k, c)
            if c == 1.0:
                by_image = np.argsort(images)
                check_level_max(lay, g, ref, avg_scores[by_image], avg_rows[by_image], aug, "f32", "fin")


def check_cont_weighted(lay, ref, got_scores, got_rows, aug, dt):
    _, _, per_image = ref(aug, dt, "fin", "cont_weighted")
    worst = 0.0
    for p, (best, _, agg, P, A) in enumerate(per_image):
        bound = H.cont_weighted_bound(P, A)
        r = int(got_rows[p] - lay.row_start[p])
        assert 0 <= r < lay.tile_counts[p]
        if p == lay.all_nan_position:
            assert np.isnan(got_scores[p]) and r == 0
            continue
        # the best row is the reference's unless the two aggregates lie within the sum of their bounds
        assert r == best or abs(agg[r] - agg[best]) <= bound[r] + bound[best], (aug, dt, p, r, best)
        err = abs(float(got_scores[p]) - agg[r])
        print(f"cont_weighted {aug} {dt} T={lay.tile_counts[p]}: |got - ref64| = {err:.3e}, bound = {bound[r]:.3e}, "
              f"P = {P[r]}, ratio = {err / bound[r]:.3f}")
        assert err <= bound[r], (aug, dt, p, err, bound[r])
        worst = max(worst, err / bound[r])
    print(f"cont_weighted {aug} {dt}: largest ratio to the bound = {worst:.3f}")


@pytest.mark.parametrize("aug", H.AUGS)
def test_cont_weighted_f32_and_f64_within_the_derived_bound(lay, ref, idx, aug):
    """|got - ref64| <= (2P + 8) * 2**-24 * A for the winning tile of every image (P partners, A = sum_j w_j |s_j|, both
    from the oracle): every f32 weight carries expf, one division and the P-term sum, the weighted sum P more roundings.
    The test prints every ratio to the bound before it asserts (docs/EXPERIMENTS.md keeps the record)."""
    import torch
    pos = np.arange(lay.n_images, dtype=np.int64)
    idx.scan(lay.query(1.0))
    check_cont_weighted(lay, ref, *idx.rescore_avg(pos, aug, aug_weight="cont_weighted"), aug, "f32")
    dev = torch.from_numpy(lay.scores(np.float64)).cuda()
    check_cont_weighted(lay, ref, *idx.rescore_avg_f64(dev.data_ptr(), pos, aug, aug_weight="cont_weighted"), aug, "f64")
    res = idx.topk_batch_avg(lay.query(1.0), lay.n_images, aug, aug_weight="cont_weighted")[0]
    by_image = np.argsort(res[0])
    want = idx.rescore_avg(pos, aug, aug_weight="cont_weighted")
    assert np.array_equal(res[4][by_image], want[1]) and same_bits(res[3][by_image], want[0])


def test_an_image_of_2049_tiles_is_refused_and_the_handle_lives_on(oracle):
    """one tile more than the kernel keeps in LDS: a status from all three entries, no launch; the other image of the same
    index is still answered"""
    import torch
    from seesaw_amd import _lib
    from seesaw_amd.device_index import DeviceIndex
    lay = H.Layout(tile_counts=[2049, 65], seed=H.SEED + 2, all_nan_image=False)
    index = DeviceIndex.from_numpy(lay.vectors(), row2image=lay.row2image)
    try:
        index.set_tile_meta(lay.boxes, lay.zoom)
        dev = torch.from_numpy(lay.scores(np.float64)).cuda()
        index.scan(lay.query(1.0))
        for call in (lambda: index.rescore_avg(np.asarray([0, 1]), "all"),
                     lambda: index.rescore_avg_f64(dev.data_ptr(), np.asarray([1, 0]), "all"),
                     lambda: index.topk_batch_avg(lay.query(1.0), 2, "all")):
            with pytest.raises(_lib.SeesawHipError) as e:
                call()
            assert e.value.status in (_lib.SSW_ERR_INVALID, _lib.SSW_ERR_UNSUPPORTED) and "2049" in str(e.value)
        r = lay.rows(1)
        for aug in H.AUGS:
            best, score, _ = oracle.avg_score_image(lay.boxes[r], lay.zoom[r], lay.scores(np.float32)[r], aug)
            got_scores, got_rows = index.rescore_avg(np.asarray([1]), aug)
            assert got_rows[0] == r.start + best and same_bits(got_scores[0], score), aug
            best64, score64, _ = oracle.avg_score_image(lay.boxes[r], lay.zoom[r], lay.scores(np.float64)[r], aug,
                                                        dtype=np.float64)
            got_scores, got_rows = index.rescore_avg_f64(dev.data_ptr(), np.asarray([1]), aug)
            assert got_rows[0] == r.start + best64 and same_bits(got_scores[0], score64), aug
        images, _, _ = index.topk(lay.query(1.0), 2)
        assert sorted(images.tolist()) == [0, 1]
    finally:
        index.close()


@pytest.mark.parametrize("bad", [32, -1])
def test_set_tile_meta_refuses_a_zoom_level_outside_the_mask(bad):
    from seesaw_amd import _lib
    from seesaw_amd.device_index import DeviceIndex
    lay = H.Layout(tile_counts=[12], all_nan_image=False)
    index = DeviceIndex.from_numpy(lay.vectors(), row2image=lay.row2image)
    try:
        zoom = lay.zoom.copy()
        zoom[4] = bad
        with pytest.raises(_lib.SeesawHipError) as e:
            index.set_tile_meta(lay.boxes, zoom)
        assert e.value.status == _lib.SSW_ERR_INVALID
        zoom[4] = 31
        index.set_tile_meta(lay.boxes, zoom)  # the edge itself is accepted
    finally:
        index.close()

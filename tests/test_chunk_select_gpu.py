"""GPU: chunk selection (DeviceIndex.chunk_select; select.hip k_chunk_*) -- every slot of a chunk selected by one set of
launches -- against plain numpy on the device's own score slabs, against the same call with the setting off, byte for
byte, and against its own counters (chunk_select_stats), which say which branch ran.

Shapes: the batched scan serves one query at a time below 65 536 rows, so `topk_batch` forms a chunk only from there
on.  The small form (at most 8192 images) is therefore reached through `views_topk_batch` (views of 1 ... 8192 images
in the slots of one chunk) and through the 8192 x 8 index of `test_slot_counts`; the general form through `topk_batch`
on indexes of at least 65 536 rows -- with an image map 8193 and 40 000 images of enough tiles, without one (row =
image) the smallest such index, 65 537 rows.  8193 and 40 000 images WITHOUT a map are below that: they are views of
a parent without a map, in the slots of one `views_topk_batch` chunk (`test_general_form_without_a_map`)."""
import numpy as np
import pytest

from tests._chunk_select_helpers import DIM, STATS, _index, _on_off, _reference, _same  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dtype", ["float32", "float16"])
@pytest.mark.parametrize("tiles", [(1, 1), (1, 5)])
@pytest.mark.parametrize("k", [1, 64, 65])
def test_small_form_views(k, tiles, dtype):
    """views of 1, 64, 65, 1025 and 8192 images in the slots of ONE chunk, every slot its own exclusions: none, the
    slot's own top three, all but five images (count < k), a random set; k = 64 on the view of one image: count < k"""
    from seesaw_amd.device_index import DeviceIndex
    rng = np.random.default_rng(k * 10 + tiles[1])
    parent, row_start = _index(rng, 12001, tiles, True, dtype)
    sizes = [1, 64, 65, 1025, 8192, 1025, 64, 8192]
    positions = [np.sort(rng.choice(12001, size=m, replace=False)) for m in sizes[:5]]
    positions += [positions[3], positions[1], positions[4]]
    views = [parent.view(p) for p in positions[:5]]
    views += [views[3], views[1], views[4]]
    Q = rng.standard_normal((len(views), DIM)).astype(np.float32)
    slabs, starts = [], []
    for s, v in enumerate(views):
        slabs.append(v.view_scores_batch(Q[s:s + 1])[0])
        starts.append(np.concatenate(([0], np.cumsum(np.diff(row_start)[positions[s]]))))
    excluded = [[] for _ in views]
    excluded[5] = _reference(slabs[5], starts[5], [], 3)[0].tolist()
    excluded[6] = list(range(5, 64))
    excluded[7] = rng.choice(8192, size=700, replace=False).tolist() + [3, 3]
    off, on, d = _on_off(parent, lambda: DeviceIndex.views_topk_batch(views, Q, k, excluded=excluded))
    for s in range(len(views)):
        want = _reference(slabs[s], starts[s], excluded[s], k)
        _same([on[s]], [want], ("reference", s))
    _same(on, off, "setting off")
    assert d == dict(chunks=1, slots=len(views), second_level=0, per_slot=0, deep_reruns=0, launches=1), d
    assert on[0][0].shape[0] == 1 and on[6][0].shape[0] == min(k, 5)
    for v in views[:5]:
        v.close()
    parent.close()


GENERAL = [(8193, (7, 10), True), (40000, (1, 5), True), (65537, (1, 1), False)]


@pytest.mark.parametrize("dtype", ["float32", "float16"])
@pytest.mark.parametrize("n_images,tiles,has_map", GENERAL)
def test_general_form(n_images, tiles, has_map, dtype):
    """four slots of one chunk: no exclusions, the slot's own top three, a random hundred, and 4040 ids -- above the
    4096 - k the chunk form takes, so that slot alone goes to the per-slot selection.  (A set that leaves fewer than k
    images of more than 8192 is above that cap by its size: it takes the same route; the small form has the case.)"""
    rng = np.random.default_rng(n_images)
    idx, row_start = _index(rng, n_images, tiles, has_map, dtype)
    assert idx.n_rows >= 65536  # (below, the batch scores one query at a time and forms no chunk)
    k = 64
    Q = rng.standard_normal((4, DIM)).astype(np.float32)
    slabs = idx.scores_batch(Q)
    excluded = [[], _reference(slabs[1], row_start, [], 3)[0].tolist(), rng.choice(n_images, size=100, replace=False).tolist(),
                rng.choice(n_images, size=4040, replace=False).tolist()]
    off, on, d = _on_off(idx, lambda: idx.topk_batch(Q, k, excluded=excluded))
    for s in range(4):
        _same([on[s]], [_reference(slabs[s], row_start, excluded[s], k)], ("reference", s))
    _same(on, off, "setting off")
    assert d == dict(chunks=1, slots=3, second_level=d["second_level"], per_slot=1, deep_reruns=0, launches=4), d
    idx.close()


@pytest.mark.parametrize("dtype", ["float32", "float16"])
def test_general_form_without_a_map(dtype):
    """8193 and 40 000 images without an image map (row = image: the slab itself is read, as 16-byte loads with one
    value and none left over): views of a parent without a map, twice each in ONE `views_topk_batch` chunk, with no
    exclusions, the slot's own top three, a random hundred, and 4040 ids (above 4096 - k: the per-slot selection)"""
    from seesaw_amd.device_index import DeviceIndex
    rng = np.random.default_rng(17)
    parent, _ = _index(rng, 45001, (1, 1), False, dtype)
    positions = [np.sort(rng.choice(45001, size=m, replace=False)) for m in (8193, 40000)]
    small, large = (parent.view(p) for p in positions)
    views = [small, large, small, large]
    k = 64
    Q = rng.standard_normal((4, DIM)).astype(np.float32)
    slabs = [v.view_scores_batch(Q[s:s + 1])[0] for s, v in enumerate(views)]
    starts = [np.arange(v.n_rows + 1) for v in views]
    excluded = [[], _reference(slabs[1], starts[1], [], 3)[0].tolist(), rng.choice(8193, size=100, replace=False).tolist(),
                rng.choice(40000, size=4040, replace=False).tolist()]
    off, on, d = _on_off(parent, lambda: DeviceIndex.views_topk_batch(views, Q, k, excluded=excluded))
    for s in range(4):
        _same([on[s]], [_reference(slabs[s], starts[s], excluded[s], k)], ("reference", s))
    _same(on, off, "setting off")
    assert d == dict(chunks=1, slots=3, second_level=d["second_level"], per_slot=1, deep_reruns=0, launches=4), d
    small.close()
    large.close()
    parent.close()


@pytest.mark.parametrize("dtype", ["float32", "float16"])
def test_second_level(dtype):
    """rows = 0.9375 e0 + small noise, queried with e0: every score lies in [0.875, 1), one bin of the top 12 key bits
    (sign, exponent, three mantissa bits), so the first level leaves everything and the second must run"""
    rng = np.random.default_rng(5)
    n_images = 8193
    counts = rng.integers(7, 11, n_images)
    X = (rng.standard_normal((int(counts.sum()), DIM)) * 1e-3).astype(np.float32)
    X[:, 0] += 0.9375
    q = np.zeros(DIM, dtype=np.float32)
    q[0] = 1.0
    exact = X.astype(np.float16).astype(np.float64)[:, 0] if dtype == "float16" else X.astype(np.float64)[:, 0]
    assert exact.min() > 0.88 and exact.max() < 0.995, "the band does not hold"
    idx, row_start = _index(np.random.default_rng(5), n_images, (7, 10), True, dtype, X=X)
    Q = np.stack([q, q])
    slabs = idx.scores_batch(Q)
    excluded = [[], _reference(slabs[1], row_start, [], 5)[0].tolist()]
    off, on, d = _on_off(idx, lambda: idx.topk_batch(Q, 50, excluded=excluded))
    for s in range(2):
        _same([on[s]], [_reference(slabs[s], row_start, excluded[s], 50)], ("reference", s))
    _same(on, off, "setting off")
    assert d == dict(chunks=1, slots=2, second_level=2, per_slot=0, deep_reruns=0, launches=4), d
    idx.close()


def test_mass_ties_rerun_deep():
    """9000 copies of one long row, queried with it: more than 8192 images tie at the top of slot 0, whose final kernel
    reports overflow; slot 1 (another query: the copies tie far below its top) does not"""
    rng = np.random.default_rng(9)
    n = 66001
    X = rng.standard_normal((n, DIM)).astype(np.float32)
    X[:9000] = 3.0 * X[0]
    idx, row_start = _index(rng, n, (1, 1), False, "float32", X=X)
    Q = np.stack([X[0], -X[0]])
    slabs = idx.scores_batch(Q)
    off, on, d = _on_off(idx, lambda: idx.topk_batch(Q, 40, excluded=[[2, 7], [1]]))
    for s, ex in enumerate(([2, 7], [1])):
        _same([on[s]], [_reference(slabs[s], row_start, ex, 40)], ("reference", s))
    _same(on, off, "setting off")
    assert (d["chunks"], d["slots"], d["per_slot"], d["deep_reruns"]) == (1, 2, 0, 1), d
    idx.close()


@pytest.mark.parametrize("n_images,tiles", [(8192, (8, 8)), (8193, (8, 8))])
def test_slot_counts(n_images, tiles):
    """1 query: the single call's route, counters unchanged; 2 and 16: one chunk, and the launches of a chunk of 16 are
    those of a chunk of 2; 17: a chunk of 16 and the single call.  8192 x 8 is the small form, 8193 x 8 the general."""
    rng = np.random.default_rng(n_images)
    idx, row_start = _index(rng, n_images, tiles, True, "float32")
    Q = rng.standard_normal((17, DIM)).astype(np.float32)
    slabs = np.concatenate([idx.scores_batch(Q[:16]), idx.scores_batch(Q[16:])])
    excluded = [rng.choice(n_images, size=s, replace=False).tolist() for s in range(17)]
    launches = {}
    for nq, chunks in ((1, 0), (2, 1), (16, 1), (17, 1)):
        off, on, d = _on_off(idx, lambda: idx.topk_batch(Q[:nq], 65, excluded=excluded[:nq]))
        for s in range(nq):
            _same([on[s]], [_reference(slabs[s], row_start, excluded[s], 65)], ("reference", nq, s))
        _same(on, off, ("setting off", nq))
        assert (d["chunks"], d["slots"], d["per_slot"]) == (chunks, nq - nq % 2 if chunks else 0, 0), (nq, d)
        launches[nq] = d["launches"]
    assert launches[16] == launches[2] == (1 if n_images <= 8192 else 4), launches
    idx.close()


def test_views_of_two_forms_and_second_stage():
    """a view of 1 109 and one of 9 000 images in one `views_topk_batch` call: two forms in one chunk, four launches in
    all; then the second stage behind the chunk's selections -- `views_topk_batch_avg` on the same two views, and
    `topk_batch_avg` on the parent (the general form) -- against the setting-off call"""
    from seesaw_amd.device_index import DeviceIndex
    rng = np.random.default_rng(11)
    parent, row_start = _index(rng, 12001, (7, 10), True, "float32")
    n = parent.n_rows
    boxes = rng.uniform(0, 200, (n, 4)).astype(np.float32)
    boxes[:, 2:] += boxes[:, :2]
    zoom = rng.integers(0, 3, n)
    parent.set_tile_meta(boxes, zoom)
    positions = [np.sort(rng.choice(12001, size=m, replace=False)) for m in (1109, 9000)]
    views = [parent.view(p) for p in positions]
    for v, p in zip(views, positions):
        rows = np.concatenate([np.arange(row_start[i], row_start[i + 1]) for i in p])
        v.set_tile_meta(boxes[rows], zoom[rows])
    Q = rng.standard_normal((2, DIM)).astype(np.float32)
    excluded = [[4, 9], rng.choice(9000, size=50, replace=False).tolist()]
    off, on, d = _on_off(parent, lambda: DeviceIndex.views_topk_batch(views, Q, 64, excluded=excluded))
    for s, (v, p) in enumerate(zip(views, positions)):
        start = np.concatenate(([0], np.cumsum(np.diff(row_start)[p])))
        _same([on[s]], [_reference(v.view_scores_batch(Q[s:s + 1])[0], start, excluded[s], 64)], ("reference", s))
    _same(on, off, "setting off")
    assert d == dict(chunks=1, slots=2, second_level=d["second_level"], per_slot=0, deep_reruns=0, launches=4), d
    off, on, d = _on_off(parent, lambda: DeviceIndex.views_topk_batch_avg(views, Q, 64, "greater", excluded=excluded))
    _same(on, off, "views avg, setting off")
    assert (d["chunks"], d["slots"]) == (1, 2), d
    off, on, d = _on_off(parent, lambda: parent.topk_batch_avg(Q, 64, "greater", excluded=excluded))
    _same(on, off, "avg, setting off")
    assert (d["chunks"], d["slots"], d["launches"]) == (1, 2, 4), d
    for v in views:
        v.close()
    parent.close()


def test_graph_round_batch():
    """S = 4 sessions, ten scripted rounds (the twins of test_labelprop_round_batch_gpu): `round_batch` with the setting
    on against `round` per handle, byte for byte -- the twins compare every slot of every round"""
    from tests.test_labelprop_round_batch_gpu import _Twins, _add
    rng = np.random.default_rng(21)
    tw = _Twins(rng, 9000, 9, 0.03, False, S=4)
    tw.idx_a.chunk_select = True
    for rnd in range(10):
        for j in range(4):
            _add(rng, tw.labels[j], tw.n, int(rng.integers(1, 14)), positive_only=(j == 0 and rnd < 4))
        tw.round(rng, rnd)
    d = tw.idx_a.chunk_select_stats()
    # (9000 images: the general form, four launches a chunk; random priors: no slot is refused or ties en masse)
    assert d["chunks"] >= 3 and d["slots"] >= 2 * d["chunks"] and d["launches"] == 4 * d["chunks"], d
    assert d["per_slot"] == 0 and d["deep_reruns"] == 0, d
    tw.close()

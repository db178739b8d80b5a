"""GPU: the second stage of a pruned query rescoring the candidates' tiles instead of completing the score buffer
(ssw_index_rescore_avg and ssw_index_gather_scores on a partial buffer, ssw_index_topk_batch_avg_pruned,
ssw_index_prune_completions; csrc/rescore.hip: k_candidate_tiles, k_candidate_tiles_keys), on the lab build.

Every comparison is exact (`same`, bits for floats) and the reference side is always a second handle over the same rows,
asked while the pruning is switched off (the switch is process-wide, so a test asks the reference first).  The index is
index A of tests/test_query_batch_gpu.py: 9 000 images of 1 / 5 / 21 tiles, one of 300 tiles, one zero-area NaN image,
~81 000 rows of dim 512 -- the smallest shape that reaches the histogram selection, the multi-slot chunk and a strided
aggregation; ssw_tune_prune(1, 1, -1) makes it prune-eligible, ssw_tune_prune6(1, 1) moves the single query onto the
6-bit shadow.

`completions` counts full scans that completed a partial buffer or slab, `rescored_rows` the rows scored on demand
instead; the tests hold them to the exact figures the design gives (the candidates' tile total, the rows of a gather,
k x 300 list entries a query of a batch)."""
import numpy as np
import pandas as pd
import pytest

from _prune_batch_helpers import flagged_queries
from _prune_helpers import same
from test_query_batch_gpu import AUGS, BIG_IMAGE, K, N_IMAGES_A, NAN_IMAGE, WEIGHTS, Case, bits, geometry_a, queries, same_entries

pytestmark = pytest.mark.gpu

SURV_CAP = 1 << 18  # csrc/index_handle.h
MAX_TILES_A = 300   # the 300-tile image: the list of a batch's query has K x 300 entries


def prune(on, min_rows=1, six=False):
    """the process-wide switches of the lab build: pruning off; on from `min_rows` rows (int8 shadow); six: single
    queries on the 6-bit shadow"""
    from seesaw_amd import _lib
    _lib.call("ssw_tune_prune", 1 if on else 0, int(min_rows), -1)
    _lib.call("ssw_tune_prune6", 1, 1 if six else -1)


def restore():
    from seesaw_amd import _lib
    _lib.call("ssw_tune_prune", 1, -1, -1)
    _lib.call("ssw_tune_prune6", 1, -1)


def stats(idx):
    return idx.prune_stats(completions=True)


@pytest.fixture(scope="module")
def data_a(oracle):
    """the arrays of index A (host only: the handles are made inside each test, on the lab build)"""
    boxes, zoom, row2image = geometry_a()
    return dict(X=oracle.synth_rows(19, 0, row2image.shape[0], 512), row2image=row2image, boxes=boxes, zoom=zoom,
                Q=queries(oracle, 19))


def case_of(d, X=None):
    """handles `a` (asked with the pruning on) and `b` (the reference, asked with it off) over index A's geometry"""
    return Case("A", d["X"] if X is None else X, d["row2image"], d["boxes"], d["zoom"], d["Q"])


def tiles_of(c, pos):
    return int((c.row_start[np.asarray(pos) + 1] - c.row_start[np.asarray(pos)]).sum())


@pytest.mark.parametrize("dtype", [np.float32, np.float16])
@pytest.mark.parametrize("shadow", ["int8", "six"])
def test_single_call_rescores_the_candidates_tiles_only(lab_build, data_a, shadow, dtype):
    """`gather_scores(all rows)`: index A has fewer rows than the 2^18 a gather scores on demand, so "all rows" are
    asked four times over in one call (every row, 4 x 81 000 entries > 2^18) -- the size from which a gather completes
    the buffer."""
    c = case_of(data_a)
    a, b = (c.a, c.b) if dtype == np.float32 else (c.handle(c.X, dtype), c.handle(c.X, dtype))
    try:
        n, q = c.X.shape[0], c.Q[3]
        rng = np.random.default_rng(5)
        others = np.setdiff1d(rng.choice(N_IMAGES_A, 230, replace=False), [NAN_IMAGE, BIG_IMAGE])[:198]
        arbitrary = rng.permutation(np.concatenate([others, [NAN_IMAGE, BIG_IMAGE]]))  # mostly images without a survivor
        assert arbitrary.shape[0] == 200
        probe = rng.choice(n, 5000, replace=False)
        prune(False)
        ref_top = b.topk(q, K)
        lists = [np.sort(ref_top[0]), arbitrary]
        minus = [rng.standard_normal(tiles_of(c, pos)).astype(np.float32) for pos in lists]
        ref = {(i, g, w, m): b.rescore_avg(pos, g, minus[i] if m else None, aug_weight=w)
               for i, pos in enumerate(lists) for g in AUGS for w in WEIGHTS for m in (False, True)}
        full = b.scores(q)
        ref_again = b.topk(None, K)

        prune(True, six=shadow == "six")
        top = a.topk(q, K)
        same(ref_top, top)
        st = stats(a)
        # the shadow the call scanned: 3 dim / 4 + 8 bytes a row of the 6-bit one (tiles of 16 rows), dim + 8 of the int8 one
        shadow_bytes = (n + 15) // 16 * 16 * (512 * 3 // 4 + 8) if shadow == "six" else n * (512 + 8)
        assert st["shadow"] == "current" and st["shadow_bytes"] == shadow_bytes, st
        assert K <= st["last_survivors"] < n and st["queries"] == 1 and st["fallbacks"] == 0, st
        assert st["completions"] == 0 and st["rescored_rows"] == 0, st
        rescored = 0
        for (i, g, w, m), want in ref.items():
            same(want, a.rescore_avg(lists[i], g, minus[i] if m else None, aug_weight=w))
            rescored += tiles_of(c, lists[i])
            now = stats(a)
            assert now["completions"] == 0 and now["rescored_rows"] == rescored, (i, g, w, m, now)
        assert np.array_equal(bits(a.gather_scores(probe)), bits(full[probe]))
        now = stats(a)
        assert now["completions"] == 0 and now["rescored_rows"] == rescored + 5000, now
        every = np.arange(4 * n) % n
        assert every.shape[0] > SURV_CAP
        assert np.array_equal(bits(a.gather_scores(every)), bits(full[every]))
        now = stats(a)
        assert now["completions"] == 1 and now["rescored_rows"] == rescored + 5000, now
        same(ref_again, a.topk(None, K))
        assert stats(a)["completions"] == 1 and stats(a)["queries"] == 1
    finally:
        restore()
        a.close()  # (closing a handle twice is harmless)
        b.close()
        c.close()


def test_more_tiles_than_the_cap_complete_the_buffer(lab_build):
    """2^18 + 4096 rows, four tiles an image (the geometry of test_rescore_avg_after_a_pruned_topk): the tile total
    of all images is above 2^18, so `rescore_avg` over all of them takes the full scan, once"""
    from seesaw_amd.device_index import DeviceIndex
    n = SURV_CAP + 4096
    idx, other = DeviceIndex.synthetic(n, 512, seed=4), DeviceIndex.synthetic(n, 512, seed=4)
    try:
        boxes = np.tile(np.array([[0, 0, 1, 1], [0, 0, .5, .5], [.5, 0, 1, .5], [0, .5, .5, 1]], np.float32), (n // 4, 1))
        for h in (idx, other):
            h.set_row2image((np.arange(n, dtype=np.int64) // 4).astype(np.int32))
            h.set_tile_meta(boxes, np.tile(np.array([0, 1, 1, 1], np.int32), n // 4))
        q = queries_unit(8)
        pos = np.arange(idx.n_images)
        prune(False)
        top = other.topk(q, 100)
        ref = other.rescore_avg(pos, "greater")
        prune(True)
        same(top, idx.topk(q, 100))
        before = stats(idx)
        assert before["last_survivors"] >= 100 and before["completions"] == 0, before
        same(ref, idx.rescore_avg(pos, "greater"))
        now = stats(idx)
        assert now["completions"] == 1 and now["rescored_rows"] == before["rescored_rows"], now
        same(ref, idx.rescore_avg(pos, "greater"))  # complete now: nothing more to do
        assert stats(idx) == now
    finally:
        restore()
        idx.close()
        other.close()


def queries_unit(seed, dim=512):
    q = np.random.default_rng(seed).standard_normal(dim).astype(np.float32)
    return (q / np.linalg.norm(q)).astype(np.float32)


def check_batch(a, b, Q, settings, excluded=None, fallbacks=0):
    """topk_batch_avg(prune=True) on `a` against the plain call on `b` asked with the pruning off, for every setting;
    the counters move by exactly what the design says"""
    prune(False)
    want = {s: b.topk_batch_avg(Q, K, s[0], excluded=excluded, aug_weight=s[1]) for s in settings}
    prune(True)
    nq = Q.shape[0]
    for s in settings:
        before = stats(a)
        got = a.topk_batch_avg(Q, K, s[0], excluded=excluded, aug_weight=s[1], prune=True)
        now = stats(a)
        assert len(got) == nq
        for g, r in zip(got, want[s]):
            same(r, g)
        assert now["queries"] - before["queries"] == nq, (s, before, now)
        assert now["completions"] == before["completions"], (s, before, now)
        fell = now["fallbacks"] - before["fallbacks"]
        assert fallbacks is None or fell == fallbacks, (s, before, now)
        # every query that kept its pruned slab lists K slots of 300 entries (padded); nq = 1 is the single call
        assert now["rescored_rows"] - before["rescored_rows"] == (nq - fell) * K * MAX_TILES_A, (s, before, now)


def test_pruned_batch_equals_the_plain_batch(lab_build, data_a):
    c = case_of(data_a)
    try:
        every = [(g, w) for g in AUGS for w in WEIGHTS]
        for nq in (1, 2, 16, 19):
            check_batch(c.a, c.b, c.Q[:nq], every if nq == 16 else [("greater", "level_max")])
        # queries that cannot be bounded among ordinary ones: they alone fall back, their second stage on the full scan
        Q = c.Q[:7].copy()
        Q[1] = 0.0
        Q[4] = flagged_queries(512)[3]  # every element 2^37
        check_batch(c.a, c.b, Q, [("all", "level_max"), ("greater", "cont_weighted")], fallbacks=2)
        # per-query exclusion lists; one leaves 3 images, fewer than k: that query's threshold selection fails
        keep = np.array([NAN_IMAGE, BIG_IMAGE, 17])
        lists = [None, (np.arange(100) * 2 + 1).tolist(), np.setdiff1d(np.arange(N_IMAGES_A), keep), list(range(0, 290, 7)), None]
        check_batch(c.a, c.b, c.Q[:5], [("all", "level_max"), ("adjacent", "cont_weighted")], excluded=lists, fallbacks=1)
        prune(True)
        got = c.a.topk_batch_avg(c.Q[:5], K, "all", excluded=lists, prune=True)[2]
        assert sorted(got[0].tolist()) == sorted(keep.tolist())
        at = got[0].tolist().index(NAN_IMAGE)
        assert np.isnan(got[3][at]) and got[4][at] == c.row_start[NAN_IMAGE]
    finally:
        restore()
        c.close()


def test_mass_ties_rerun_deep_inside_a_pruned_chunk(lab_build, data_a, oracle):
    """every row the same vector (test_mass_ties_take_the_deep_selection_inside_the_batch): the fast selection overflows
    and the deep path runs for every query of the pruned chunk, before its second stage.  Whether a slot keeps its
    pruned slab or takes the full scan is the certificate's business (an overflowed threshold selection fails it), so
    the fallbacks are counted, not prescribed"""
    X = np.broadcast_to(oracle.synth_rows(1, 0, 1, 512), data_a["X"].shape)
    c = case_of(data_a, X)
    try:
        for nq in (1, 3):
            check_batch(c.a, c.b, c.Q[:nq], [("all", "level_max")], fallbacks=None)
        prune(True)
        assert c.a.topk_batch_avg(c.Q[:3], K, "all", prune=True)[1][0].tolist() == list(range(K))
    finally:
        restore()
        c.close()


def test_a_list_longer_than_the_cap_completes_the_slab(lab_build, data_a):
    """k = 1000 slots of 300 entries are more than the 2^18 a survivor list holds: every pruned slab, and the handle's
    buffer after the single call, is completed by the full scan of its query instead"""
    c = case_of(data_a)
    try:
        k = 1000
        assert k * MAX_TILES_A > SURV_CAP
        for nq in (1, 3):
            prune(False)
            want = c.b.topk_batch_avg(c.Q[:nq], k, "greater")
            again = c.b.topk(None, k)
            prune(True)
            before = stats(c.a)
            got = c.a.topk_batch_avg(c.Q[:nq], k, "greater", prune=True)
            now = stats(c.a)
            for r, g in zip(want, got):
                same(r, g)
                assert g[0].shape[0] == k
            assert now["queries"] - before["queries"] == nq and now["fallbacks"] == before["fallbacks"], (before, now)
            assert now["completions"] - before["completions"] == nq, (before, now)
            assert now["rescored_rows"] == before["rescored_rows"], (before, now)
            same(again, c.a.topk(None, k))  # the last slab is the handle's buffer, complete by now
            assert stats(c.a)["completions"] == now["completions"]
    finally:
        restore()
        c.close()


def test_pruned_batch_over_f16_rows(lab_build, data_a):
    c = case_of(data_a)
    a, b = c.handle(c.X, np.float16), c.handle(c.X, np.float16)
    try:
        check_batch(a, b, c.Q[:16], [("greater", "cont_weighted")])
    finally:
        restore()
        a.close()
        b.close()
        c.close()


def test_state_after_the_pruned_two_stage_batch(lab_build, data_a):
    c = case_of(data_a)
    try:
        a, b, Q = c.a, c.b, c.Q
        ex = [list(range(i, 290, 7)) for i in range(19)]
        probe = np.arange(0, c.X.shape[0], 97)
        prune(False)
        last = b.topk(Q[18], K, excluded=ex[-1])
        again = b.topk(None, K, excluded=ex[-1])
        gathered = b.scores(Q[18])[probe]
        rescored = b.rescore_avg(last[0], "greater")
        plain = b.topk_batch_avg(Q[:5], K, "greater")
        single = b.topk(Q[2], K)
        prune(True)
        got = a.topk_batch_avg(Q, K, "greater", excluded=ex, prune=True)
        same(last, got[-1][:3])
        st = stats(a)
        assert st["last_survivors"] >= K and st["queries"] == 19 and st["fallbacks"] == 0 and st["completions"] == 0, st
        # the handle's buffer is the last query's slab, still partial: the second-stage readers rescore, topk(None) completes
        assert np.array_equal(bits(a.gather_scores(probe)), bits(gathered))
        same(rescored, a.rescore_avg(last[0], "greater"))
        assert stats(a)["completions"] == 0
        same(again, a.topk(None, K, excluded=ex[-1]))
        assert stats(a)["completions"] == 1
        a.topk_batch_avg(Q, K, "greater", excluded=ex, prune=True)
        for r, g in zip(plain, a.topk_batch_avg(Q[:5], K, "greater")):  # a plain batch after it: unaffected
            same(r, g)
        assert stats(a)["queries"] == 38 and stats(a)["completions"] == 2  # (the plain batch completes first, as ever)
        a.topk_batch_avg(Q, K, "greater", excluded=ex, prune=True)
        same(single, a.topk(Q[2], K))  # a pruned single call after it
        assert stats(a)["queries"] == 58 and stats(a)["last_survivors"] >= K and stats(a)["completions"] == 2
    finally:
        restore()
        c.close()


def test_an_index_that_is_not_pruned_takes_the_plain_batch(lab_build, data_a):
    c = case_of(data_a)
    try:
        prune(False)
        want = c.b.topk_batch_avg(c.Q[:5], K, "greater")
        prune(True, min_rows=c.X.shape[0] + 1)
        before = stats(c.a)
        assert not before["eligible"]
        for nq in (1, 5):
            for r, g in zip(want, c.a.topk_batch_avg(c.Q[:nq], K, "greater", prune=True)):
                same(r, g)
        assert stats(c.a) == before and before["queries"] == before["completions"] == before["rescored_rows"] == 0
    finally:
        restore()
        c.close()


def test_multiscale_query_batch_pruned_is_the_loop_of_query(lab_build, data_a):
    from seesaw_amd.bitmap import BitMap
    from seesaw_amd.indices.interface import AccessMethod
    from seesaw_amd.indices.multiscale.multiscale_index import MultiscaleIndex
    bx = data_a["boxes"]
    meta = pd.DataFrame({"dbidx": data_a["row2image"].astype(np.int64) * 3 + 1, "zoom_level": data_a["zoom"].astype(np.int16),
                         "x1": bx[:, 0], "y1": bx[:, 1], "x2": bx[:, 2], "y2": bx[:, 3]})
    index = MultiscaleIndex(embedding=None, vectors=data_a["X"], vector_meta=meta)
    try:
        Q, ids, dev = data_a["Q"], index._dbidx, index._dev
        keep = ids[[NAN_IMAGE, BIG_IMAGE, 17]]
        pool = [None, BitMap(ids[:100].tolist()), BitMap(ids.tolist()), BitMap(np.setdiff1d(ids, keep).tolist()), BitMap()]
        vectors = [q for q in Q[:7]]
        excludes = [pool[i % len(pool)] for i in range(7)]  # entry 2 covers the index, entry 3 leaves 3 images
        settings = [dict(agg_method="plain_score", aug_larger="all")]
        settings += [dict(agg_method="avg_score", aug_larger=g, aug_weight=w) for g in AUGS for w in WEIGHTS]
        settings = [dict(kw, topk=10, shortlist_size=50, rescore_method=None) for kw in settings]
        v2 = dict(topk=10, shortlist_size=50, agg_method="avg_score", aug_larger="greater", rescore_method=None, vector2=Q[9])
        prune(False)
        full = [AccessMethod.query_batch(index, vectors=vectors, excludes=excludes, **kw) for kw in settings]
        full_v2 = [index.query(vector=v, exclude=None, **v2) for v in vectors[:2]]
        prune(True)
        assert dev.prune_stats()["eligible"]
        for kw, ref in zip(settings, full):
            before = stats(dev)
            got = index.query_batch(vectors=vectors, excludes=excludes, prune=True, **kw)
            assert np.array_equal(index._resident_q, Q[6])
            same_entries(got, ref)
            assert got[2]["dbidxs"].shape[0] == 0 and got[3]["dbidxs"].shape[0] == 3 and got[0]["dbidxs"].shape[0] == 10
            now = stats(dev)
            assert now["queries"] - before["queries"] == 6 and now["completions"] == before["completions"], (kw, before, now)
            same_entries(AccessMethod.query_batch(index, vectors=vectors, excludes=excludes, **kw), ref)  # the pruned loop
        # the principal query, eight times over: the second stage never completes the buffer
        kw = dict(topk=10, shortlist_size=50, agg_method="avg_score", aug_larger="greater", rescore_method=None)
        prune(False)
        ref = [index.query(vector=Q[i], exclude=None, **kw) for i in range(8)]
        prune(True)
        dev.topk(Q[0], K)  # (whatever the loop above left: a partial buffer from here on)
        before = stats(dev)
        same_entries([index.query(vector=Q[i], exclude=None, **kw) for i in range(8)], ref)
        now = stats(dev)
        assert now["completions"] == before["completions"] and now["queries"] - before["queries"] == 8, (before, now)
        assert now["fallbacks"] == before["fallbacks"] and now["rescored_rows"] > before["rescored_rows"], (before, now)
        # `vector2` keeps going through the loop, and `prune` does not reach `query`
        same_entries(index.query_batch(vectors=vectors[:2], prune=True, **v2), full_v2)
    finally:
        restore()
        index._dev.close()

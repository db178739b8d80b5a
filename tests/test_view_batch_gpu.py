"""GPU: the batched entries of a subset view (DeviceIndex.view_scores_batch / view_topk_batch / view_topk_batch_avg,
ssw_index_view_*) and the query_batch / SessionGroup layers above them.

Every comparison is against code that existed before these entries: `parent.scores(q)[rows]`, the loop of `view.topk`,
and `topk_batch` / `topk_batch_avg` of the COPIED subset `Parent.copy_of(positions)`.  Bits of scores, positions and
best rows are equal, with no tolerance.

Parent: 20 000 images of 1-7 tiles (about 80 000 rows), seeded, rows from `hard_rows` (tests/test_subset_view_gpu.py).
Member lists: (a) exactly 65 536 rows -- the shortest prefix of at least that many rows less ONE image of the excess
tiles (no prefix of the seeded parent totals exactly 65 536; the list keeps the image map): the single view scan is
the small form there and the batch the streaming form; (b) a prefix of rows % 64 == 1 above 66 000 rows: a ragged last
batch; (c) the last image in, one image in eight out: every run short, the tail clamp reads real rows.  (d) fewer
batches than waves holds at these sizes and is asserted from the device's CU count."""
import numpy as np
import pytest

from test_subset_view_gpu import F16, F32, MAX_TOPK, SMALL_ROWS, Parent, bits, hard_rows, prefix_with_rows_mod, same_query, \
    same_result

pytestmark = pytest.mark.gpu

PAIRS = [(dim, dt) for dim in (256, 512, 768, 1024) for dt in (F32, F16)]
PAIR_IDS = ["%d-%s" % (dim, np.dtype(dt).name) for dim, dt in PAIRS]
ALL_LISTS = [(256, F32), (512, F16)]  # the pairs that run member lists (a) and (c) beside (b)
NQS = (2, 3, 16, 17, 23)  # chunks of 16, 8, 4, 2 and 1 all run (23 = 16 + 4 + 2 + 1 at width 16, 8 + 8 + 4 + 2 + 1 at 8)
BLOCKS_PER_CU = 2  # scan.hip: SCAN_BATCH_BLOCKS_PER_CU


@pytest.fixture(scope="module")
def parents(oracle):
    made = {}

    def get(dim, dtype):
        key = (dim, np.dtype(dtype).name)
        if key not in made:
            made[key] = Parent(oracle, 20000, 1, 7, dim, dtype, seed=33)
        return made[key]

    yield get
    for p in made.values():
        p.close()


def exactly_small_rows(par):
    """(a): exactly SMALL_ROWS rows, with the image map"""
    every = np.arange(par.n_images)
    n_pref = int(np.searchsorted(par.row_start, SMALL_ROWS, side="left"))  # the shortest prefix of >= SMALL_ROWS rows
    excess = int(par.row_start[n_pref]) - SMALL_ROWS
    if excess == 0:
        return every[:n_pref]
    drop = np.nonzero(par.counts[:n_pref] == excess)[0]
    assert drop.size, excess
    return np.delete(every[:n_pref], drop[drop.size // 2])


def member_lists(par, all_lists):
    every = np.arange(par.n_images)
    lists = {"b": prefix_with_rows_mod(par.counts, every, 1, 66001)}
    if all_lists:
        lists["a"] = exactly_small_rows(par)
        lists["c"] = np.concatenate((every[:-1][np.arange(par.n_images - 1) % 8 != 3], [par.n_images - 1]))
    return lists


def queries(oracle, dim, nq, seed=0):
    scale = np.linspace(0.6, 1.9, nq, dtype=np.float32)
    return np.stack([oracle.synth_query(seed + 11 * b, dim) * scale[b] for b in range(nq)])


def exclusions(m, nq, seed):
    """per query: some None, some short, one a third of the images"""
    rng = np.random.default_rng(seed)
    ex = [None if b % 3 == 0 else rng.choice(m, size=5 + 20 * b, replace=False).tolist() for b in range(nq)]
    ex[1] = rng.choice(m, size=m // 3, replace=False).tolist()
    return ex


def waves_of_the_grid():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count * BLOCKS_PER_CU * 4


@pytest.mark.parametrize("dim,dtype", PAIRS, ids=PAIR_IDS)
def test_widths_scores_and_topk_bit_exact(oracle, parents, dim, dtype):
    par = parents(dim, dtype)
    assert 75000 < par.n < 85000
    Q = queries(oracle, dim, max(NQS))
    parent_scores = [par.dev.scores(q) for q in Q]  # the reference, once
    for name, pos in member_lists(par, (dim, dtype) in ALL_LISTS).items():
        rows, _ = par.rows_of(pos)
        n, m = rows.shape[0], len(pos)
        if name == "a":
            assert n == SMALL_ROWS
        elif name == "b":
            assert n > 66000 and n % 64 == 1
        else:
            assert n > SMALL_ROWS and pos[-1] == par.n_images - 1
        assert (n + 63) // 64 < waves_of_the_grid()  # (d)
        ref = [s[rows] for s in parent_scores]
        ex = exclusions(m, max(NQS), seed=dim)
        pick = np.random.default_rng(n).integers(0, n, 2000)
        v, c = par.dev.view(pos), par.copy_of(pos)
        try:
            assert np.array_equal(v.parent_rows, rows)
            loop = {k: [v.topk(Q[b], k, excluded=ex[b]) for b in range(max(NQS))] for k in (1, 50, MAX_TOPK)}
            for nq in NQS:
                S = v.view_scores_batch(Q[:nq])
                assert S.shape == (nq, n) and S.dtype == np.float32
                for b in range(nq):
                    assert np.array_equal(bits(S[b]), bits(ref[b])), (name, nq, b)
                assert np.array_equal(bits(v.gather_scores(pick)), bits(ref[nq - 1][pick])), (name, nq)  # the last query's
                for k in (1, 50, MAX_TOPK):
                    got = v.view_topk_batch(Q[:nq], k, excluded=ex[:nq])
                    copied = c.topk_batch(Q[:nq], k, excluded=ex[:nq])
                    assert len(got) == len(copied) == nq
                    for b in range(nq):
                        assert got[b][0].shape[0] == min(k, m - len(ex[b] or []))
                        same_result(got[b], loop[k][b])
                        same_result(got[b], copied[b])
                    # the view is left as after the last query's topk: its resident scores are that query's, whole
                    assert np.array_equal(bits(v.gather_scores(pick)), bits(ref[nq - 1][pick])), (name, nq, k)
                    same_result(v.topk(None, k, excluded=ex[nq - 1]), loop[k][nq - 1])
            got = v.view_topk_batch(Q[:5], 50)  # excluded=None: nobody excludes
            for b in range(5):
                same_result(got[b], v.topk(Q[b], 50))
        finally:
            v.close()
            c.close()


def test_mass_ties_take_the_deep_path_inside_a_chunk(oracle):
    """the construction of test_topk_mass_ties_take_the_deep_path (streaming size, with an image map): duplicated rows,
    more than 8192 images share the k-th score, the fast selection overflows and the deep rerun answers -- here for
    each query of a chunk of 2 and for the single query after it, while later slabs wait"""
    from seesaw_amd.device_index import DeviceIndex, view_rows
    n_parent = 150000
    base = oracle.synth_rows(1, 0, 1, 512)[0]
    counts = np.arange(n_parent * 2 // 3) % 3 + 1
    row_start = np.concatenate(([0], np.cumsum(counts))).astype(np.int64)
    r2i = np.repeat(np.arange(counts.shape[0]), counts).astype(np.int32)
    X = np.repeat(base[None, :] * np.float32(0.5), int(row_start[-1]), axis=0)
    pos = np.arange(0, row_start.shape[0] - 1, 2)
    rows, start = view_rows(row_start, pos)
    m = pos.shape[0]
    assert m > 8192 and rows.shape[0] > SMALL_ROWS
    marked = rows[(np.arange(20) * (rows.shape[0] // 20) + 8)]
    X[marked] = base[None, :] * np.linspace(0.6, 0.9, 20, dtype=np.float32)[:, None]
    compact = np.repeat(np.arange(m), np.diff(start)).astype(np.int32)
    Q = np.stack([base, oracle.synth_query(4, 512), base * np.float32(-1.5)])  # every query ties on the duplicated rows
    ex = [None, list(range(0, 60, 3)), None]
    parent = DeviceIndex.from_numpy(X, row2image=r2i)
    v, c = parent.view(pos), DeviceIndex.from_numpy(X[rows], row2image=compact)
    try:
        for k in (21, 100, MAX_TOPK):
            loop = [v.topk(Q[b], k, excluded=ex[b]) for b in range(3)]
            got = v.view_topk_batch(Q, k, excluded=ex)
            copied = c.topk_batch(Q, k, excluded=ex)
            for b in range(3):
                assert got[b][0].shape[0] == k
                same_result(got[b], loop[b])
                same_result(got[b], copied[b])
        ref = oracle.scores_kernel_order(X[rows], Q[0])
        same_result(v.view_topk_batch(Q, 100)[0], oracle.topk_images_tiebreak(ref, compact, m, [], 100))
    finally:
        v.close()
        c.close()
        parent.close()


@pytest.mark.parametrize("aug_larger", ["all", "greater"])
def test_two_stage_batch_equals_the_copied_subset(oracle, parents, aug_larger):
    par = parents(512, F16)
    pos = member_lists(par, False)["b"]
    rows, _ = par.rows_of(pos)
    rng = np.random.default_rng(8)
    boxes = rng.uniform(0, 100, (par.n, 4)).astype(np.float32)
    boxes[:, 2:] += boxes[:, :2]
    zoom = rng.integers(0, 3, par.n).astype(np.int32)
    Q = queries(oracle, 512, 5, seed=3)
    ex = exclusions(len(pos), 5, seed=2)
    v, c = par.dev.view(pos), par.copy_of(pos)
    try:
        for d in (v, c):
            d.set_tile_meta(boxes[rows], zoom[rows])  # the view's own tile meta, by view row
        for weight in ("level_max", "cont_weighted"):
            got = v.view_topk_batch_avg(Q, 60, aug_larger, excluded=ex, aug_weight=weight)
            copied = c.topk_batch_avg(Q, 60, aug_larger, excluded=ex, aug_weight=weight)
            for b in range(5):
                same_result(got[b][:3], copied[b][:3])
                same_result(got[b][:3], v.topk(Q[b], 60, excluded=ex[b]))
                assert np.array_equal(bits(got[b][3]), bits(copied[b][3])) and np.array_equal(got[b][4], copied[b][4])
                # and the single second stage on the view, while that query's scores are resident
                order = np.argsort(got[b][0])
                s1, r1 = v.rescore_avg(got[b][0][order], aug_larger, aug_weight=weight)
                assert np.array_equal(bits(s1), bits(got[b][3][order])) and np.array_equal(r1, got[b][4][order])
    finally:
        v.close()
        c.close()


def test_the_parents_uploads_show_in_the_next_batch(oracle):
    import ctypes
    from seesaw_amd import _lib
    par = Parent(oracle, 20000, 1, 7, 256, F32, seed=61)
    pos = member_lists(par, False)["b"]
    rows, start = par.rows_of(pos)
    Q = queries(oracle, 256, 3, seed=5)
    v = par.dev.view(pos)
    try:
        first = v.view_topk_batch(Q, 50)
        for b in range(3):
            same_result(first[b], v.topk(Q[b], 50))
        i = int(first[0][0][0])  # the best image of the first query: new rows for it change that result
        img = int(pos[i])
        r0, r1 = int(par.row_start[img]), int(par.row_start[img + 1])
        fresh = hard_rows(oracle, r1 - r0, 256, seed=99) * np.float32(0.01)
        _lib.call("ssw_index_upload", par.dev._h, ctypes.c_void_p(fresh.ctypes.data), r0, r1 - r0)
        X2 = par.X.copy()
        X2[r0:r1] = fresh
        second = v.view_topk_batch(Q, 50)
        S = v.view_scores_batch(Q)
        for b in range(3):
            same_result(second[b], v.topk(Q[b], 50))
            assert np.array_equal(bits(S[b]), bits(oracle.scores_kernel_order(X2[rows], Q[b])))
        assert int(second[0][0][0]) != i
    finally:
        v.close()
        par.close()


def test_a_small_view_returns_the_loops_results(oracle, parents):
    par = parents(512, F16)
    rng = np.random.default_rng(4)
    pos = np.nonzero(rng.random(par.n_images) < 0.4)[0]
    rows, _ = par.rows_of(pos)
    assert rows.shape[0] < SMALL_ROWS and len(pos) > 5000
    Q = queries(oracle, 512, 5, seed=9)
    ex = exclusions(len(pos), 5, seed=6)
    v, c = par.dev.view(pos), par.copy_of(pos)
    try:
        S = v.view_scores_batch(Q)
        for b in range(5):
            assert np.array_equal(bits(S[b]), bits(par.dev.scores(Q[b])[rows]))
        for k in (1, 50, MAX_TOPK):
            got, copied = v.view_topk_batch(Q, k, excluded=ex), c.topk_batch(Q, k, excluded=ex)
            for b in range(5):
                same_result(got[b], v.topk(Q[b], k, excluded=ex[b]))
                same_result(got[b], copied[b])
        one = v.view_topk_batch(Q[:1], 50, excluded=ex[:1])  # nq == 1 is the single call
        same_result(one[0], v.topk(Q[0], 50, excluded=ex[0]))
    finally:
        v.close()
        c.close()


def test_refusals(oracle, parents):
    from seesaw_amd import _lib
    par = parents(256, F32)
    pos = member_lists(par, False)["b"]
    Q = queries(oracle, 256, 2, seed=1)
    v = par.dev.view(pos)
    rng = np.random.default_rng(1)
    boxes = rng.uniform(0, 100, (v.n_rows, 4)).astype(np.float32)
    v.set_tile_meta(boxes, rng.integers(0, 3, v.n_rows).astype(np.int32))
    try:
        before = v.topk(Q[0], 40, excluded=[1, 5])
        # the new entries take a view only
        for name, fn in (("ssw_index_view_scan_batch", lambda d: d.view_scores_batch(Q)),
                         ("ssw_index_view_topk_batch", lambda d: d.view_topk_batch(Q, 5)),
                         ("ssw_index_view_topk_batch_avg", lambda d: d.view_topk_batch_avg(Q, 5, "all"))):
            with pytest.raises(_lib.SeesawHipError) as e:
                fn(par.dev)
            assert e.value.status == _lib.SSW_ERR_INVALID and (name + ":") in str(e.value) and "not a view" in str(e.value)
            fn(v)  # and do take one
        # the old entries keep refusing one
        for name, fn in (("ssw_index_scan_batch:", lambda: v.scores_batch(Q)),
                         ("ssw_index_topk_batch:", lambda: v.topk_batch(Q, 5)),
                         ("ssw_index_topk_batch_pruned:", lambda: v.topk_batch(Q, 5, prune=True)),
                         ("ssw_index_topk_batch_avg:", lambda: v.topk_batch_avg(Q, 5, "all")),
                         ("ssw_index_topk_batch_avg_pruned:", lambda: v.topk_batch_avg(Q, 5, "all", prune=True)),
                         ("ssw_index_topk_batch_dev:", lambda: v.topk_batch_dev(Q, 5)),
                         ("ssw_index_stage2_pair_batch:", lambda: v.stage2_pair(Q, Q, np.zeros((2, 5), np.int64),
                                                                                 np.zeros(2, np.int32), "plain_score"))):
            with pytest.raises(_lib.SeesawHipError) as e:
                fn()
            assert e.value.status == _lib.SSW_ERR_UNSUPPORTED and "view" in str(e.value) and name in str(e.value)
        # argument errors are the plain entries'
        with pytest.raises(_lib.SeesawHipError) as e:
            v.view_topk_batch(Q, MAX_TOPK + 1)
        assert e.value.status == _lib.SSW_ERR_INVALID
        with pytest.raises(_lib.SeesawHipError) as e:
            v.view_topk_batch(Q, 5, excluded=[[0], [v.n_images]])
        assert e.value.status == _lib.SSW_ERR_INVALID
        bad = Q.copy()
        bad[1, 7] = np.nan
        with pytest.raises(_lib.SeesawHipError) as e:
            v.view_topk_batch(bad, 5)
        assert e.value.status == _lib.SSW_ERR_NUMERIC
        same_result(v.topk(Q[0], 40, excluded=[1, 5]), before)
    finally:
        v.close()


# ---- the index layer ---------------------------------------------------------------------------------------------------
def counted(obj, name, calls):
    """wrap the bound method `name` on the instance: every call is appended to `calls`"""
    inner = getattr(obj, name)

    def wrapper(*args, **kwargs):
        calls.append(name)
        return inner(*args, **kwargs)

    setattr(obj, name, wrapper)


@pytest.fixture(scope="module")
def dataset():
    from seesaw_amd.synthetic import make_dataset
    return make_dataset("views", n_images=120, tiles_per_image=13, positive_frac=0.1, seed=5)


@pytest.mark.parametrize("vector_dtype", ["float32", "float16"])
def test_multiscale_query_batch_on_a_view_is_one_batched_call(dataset, vector_dtype):
    from seesaw_amd.bitmap import BitMap
    from seesaw_amd.indices.multiscale.multiscale_index import MultiscaleIndex
    from test_subset_view_gpu import members_of
    ds = dataset
    full = MultiscaleIndex(embedding=ds.embedding, vectors=ds.vectors, vector_meta=ds.vector_meta, vector_dtype=vector_dtype)
    ids = members_of(ds)
    sub, view = full.subset(BitMap(ids)), full.subset_view(BitMap(ids))
    assert view._dev.is_view and not sub._dev.is_view
    vecs = [ds.embedding.from_string(string="a c%d" % i).reshape(-1) for i in (1, 2, 0, 1, 3)]
    excludes = [None, BitMap(ids[3:9]), BitMap(ids[::2]), None, BitMap(ids)]  # the last covers the index: through `query`
    try:
        for kw, method in ((dict(agg_method="plain_score", aug_larger="greater"), "view_topk_batch"),
                           (dict(agg_method="avg_score", aug_larger="greater"), "view_topk_batch_avg"),
                           (dict(agg_method="avg_score", aug_larger="all"), "view_topk_batch_avg")):
            for prune in (False, True):  # consumed: the plain view batch
                calls = []
                for name in ("view_topk_batch", "view_topk_batch_avg", "topk", "topk_batch", "topk_batch_avg"):
                    counted(view._dev, name, calls)
                got = view.query_batch(topk=5, vectors=vecs, excludes=excludes, shortlist_size=25, prune=prune, **kw)
                for name in ("view_topk_batch", "view_topk_batch_avg", "topk", "topk_batch", "topk_batch_avg"):
                    delattr(view._dev, name)
                assert calls == [method], (kw, calls)  # ONE batched call, no call of the single top-k
                want = sub.query_batch(topk=5, vectors=vecs, excludes=excludes, shortlist_size=25, **kw)
                for a, b, v, e in zip(got, want, vecs, excludes):
                    same_query(a, b)
                    same_query(a, view.query(vector=v, topk=5, shortlist_size=25, exclude=e, **kw))
        # two-vector entries keep the loop on a view: no stage2_pair takes one
        kw = dict(agg_method="avg_score", aug_larger="greater")
        calls = []
        counted(view._dev, "topk", calls)
        got = view.query_batch(topk=5, vectors=vecs[:2], vectors2=[vecs[2], None], shortlist_size=25, **kw)
        delattr(view._dev, "topk")
        assert calls == ["topk", "topk"]
        for a, b in zip(got, sub.query_batch(topk=5, vectors=vecs[:2], vectors2=[vecs[2], None], shortlist_size=25, **kw)):
            same_query(a, b)
    finally:
        for idx in (view, sub):
            idx._dev.close()
        full._dev.close()


def test_coarse_query_batch_on_a_view_is_one_batched_call(oracle):
    import pandas as pd
    from seesaw_amd.bitmap import BitMap
    from seesaw_amd.indices.coarse.coarse_index import CoarseIndex
    from seesaw_amd.synthetic import SyntheticEmbedding
    n = 160000  # the view of 40 % of it scans in the streaming form
    X = oracle.synth_rows(12, 0, n, 256)
    meta = pd.DataFrame({"dbidx": np.arange(n) * 2 + 1})
    full = CoarseIndex(embedding=SyntheticEmbedding({}, 256), vectors=X, vector_meta=meta)
    ids = (np.nonzero(np.random.default_rng(4).random(n) < 0.45)[0] * 2 + 1).tolist()
    sub, view = full.subset(BitMap(ids)), full.subset_view(BitMap(ids))
    assert view._dev.is_view and view._dev.n_rows > SMALL_ROWS
    vecs = [oracle.synth_query(s, 256) for s in (1, 2, 3)] + [None]  # the last: random order, through `query`
    excludes = [None, BitMap(ids[5:40]), BitMap(ids[::3]), BitMap(ids[:-7])]
    try:
        calls = []
        for name in ("view_topk_batch", "topk", "topk_batch"):
            counted(view._dev, name, calls)
        got = view.query_batch(topk=7, vectors=vecs, excludes=excludes, prune=True)
        for name in ("view_topk_batch", "topk", "topk_batch"):
            delattr(view._dev, name)
        assert calls == ["view_topk_batch"], calls
        want = sub.query_batch(topk=7, vectors=vecs, excludes=excludes)
        for a, b in list(zip(got, want))[:3]:
            assert a["nextstartk"] == b["nextstartk"]
            same_query(a, b)
        assert len(got[3]["dbidxs"]) == 7 and set(got[3]["dbidxs"].tolist()) <= set(ids[-7:])
    finally:
        for d in (view, sub):
            d._dev.close()
        full._dev.close()


# ---- the session layer -------------------------------------------------------------------------------------------------
def test_a_session_group_on_a_view_index_batches_its_round(oracle):
    """four multi_reg sessions on ONE subset_view index, the small synthetic dataset of tests/test_session_group_gpu.py:
    SessionGroup.next() shows what the four sessions show on their own, and reaches the view's batched entry once a
    round"""
    from seesaw_amd.basic_types import IndexSpec, SessionParams
    from seesaw_amd.bitmap import BitMap
    from seesaw_amd.seesaw_session import Session, SessionGroup
    from seesaw_amd.synthetic import GlobalDataManager, make_dataset
    from test_session_group_gpu import MULTI_REG, SESSIONS, _label, _snapshot
    ds = make_dataset("grp", n_images=200, tiles_per_image=13, n_categories=3, positive_frac=0.08, seed=21, knn_k=10)
    gdm = GlobalDataManager().add(ds)
    full = ds.load_index("multiscale", options={"use_vec_index": False})
    members = BitMap(sorted(set(range(200)) - set(range(3, 200, 5))))  # 160 of the 200 images
    specs = SESSIONS[:4]
    assert all(s[0] == "multi_reg" for s in specs)

    def run(grouped):
        view = full.subset_view(members)
        assert view._dev.is_view
        calls = []
        for name in ("view_topk_batch", "view_topk_batch_avg", "topk"):
            counted(view._dev, name, calls)
        sessions = []
        for _, _, text, _, policy in specs:
            p = SessionParams(index_spec=IndexSpec(d_name="grp", i_name="multiscale", c_name=None), interactive="multi_reg",
                              interactive_options=MULTI_REG, batch_size=3, shortlist_size=50, agg_method="avg_score",
                              aug_larger="greater", start_policy=policy, index_options={"use_vec_index": False})
            s = Session(gdm, ds, view, p)
            s.set_text(text)
            sessions.append(s)
        group = SessionGroup(sessions)
        trace, per_round = [], []
        for _ in range(3):
            del calls[:]
            if grouped:
                assert group.query_groups() == [(0, 1, 2, 3)]
                group.next()
            else:
                for s in sessions:
                    s.next()
            per_round.append(list(calls))
            for s, spec in zip(sessions, specs):
                _label(s, spec[3], ds)
            if grouped:
                group.refine()
            else:
                for s in sessions:
                    s.refine()
            trace.append([_snapshot(s) for s in sessions])
        view._dev.close()
        return trace, per_round

    try:
        alone, alone_calls = run(False)
        together, group_calls = run(True)
    finally:
        full._dev.close()
    assert alone_calls == [["topk"] * 4] * 3
    assert group_calls == [["view_topk_batch_avg"]] * 3  # once a round, and no single top-k beside it
    for r in range(3):
        for i in range(4):
            a, t = alone[r][i], together[r][i]
            assert np.array_equal(a["dbidxs"], t["dbidxs"]) and len(a["dbidxs"]) == 3, (r, i)
            assert a["activations"] == t["activations"], (r, i)
            assert np.array_equal(a["returned"], t["returned"]), (r, i)
            assert a["started"] == t["started"], (r, i)
            assert np.array_equal(a["curr_vec"], t["curr_vec"]), (r, i)

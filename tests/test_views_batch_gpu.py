"""GPU: top-k across views of one parent in one call (DeviceIndex.views_topk_batch*, ssw_index_views_topk_batch*) and the
query_batch_views / SessionGroup.view_groups layers above it.  Reference: a float64 dot product of the stored row values
(float16: the widened binary16 values).  Tolerance, from the reference alone: |got - ref| <= dim * 2^-24 * sum_d |x_d q_d|,
the bound of an f32 sum of `dim` products in any order.  The float64 distinct-image top-k must come back exactly; the
cases are seeded so that every gap between ranks 1 .. k+1 of the reference exceeds twice the slot's largest bound, which
`Case` asserts before anything is launched.  Every slot also equals, byte for byte, `view.topk` (+ `rescore_avg`).
The small form's workgroup takes 4 * U * steps rows, U = 8 up to dim 512 and 4 above; steps is 1 at these sizes and 3
for the small-form slots of case (c) together."""
import ctypes

import numpy as np
import pytest

from test_subset_view_gpu import F16, F32, bits, held

pytestmark = pytest.mark.gpu
K = 6


def members_with_rows(counts, target, first=0):
    pos, total = [], 0
    for p in range(first, len(counts)):
        if total + counts[p] <= target:
            pos.append(p)
            total += counts[p]
    assert total == target, (target, total)
    return np.array(pos)


class Case:
    """a parent, member lists, the slots (list, query seed, excluded images) of one call and their float64 reference"""

    def __init__(self, oracle, counts, dim, dtype, seed, lists, slots):
        self.dim, self.dtype, self.lists, self.slots = dim, dtype, lists, slots
        self.counts = np.asarray(counts)
        self.row_start = np.concatenate(([0], np.cumsum(self.counts))).astype(np.int64)
        n = int(self.row_start[-1])
        self.X = oracle.synth_rows(seed, 0, n, dim)
        self.W = held(self.X, dtype).astype(np.float64)
        rng = np.random.default_rng(seed)
        self.boxes = rng.uniform(0, 100, (n, 4)).astype(np.float32)
        self.boxes[:, 2:] += self.boxes[:, :2]
        self.zoom = rng.integers(0, 3, n).astype(np.int32)
        self.Q = np.stack([oracle.synth_query(qs, dim) * np.float32(0.7 + 0.1 * (qs % 7)) for _, qs, _ in slots])
        from seesaw_amd.device_index import view_rows
        self.ref = []  # per slot: (row scores f64, row bounds, expected images, their best rows)
        for s, (name, _, ex) in enumerate(slots):
            rows, start = view_rows(self.row_start, lists[name])
            q = self.Q[s].astype(np.float64)
            sc = self.W[rows] @ q
            bound = dim * 2.0 ** -24 * (np.abs(self.W[rows]) @ np.abs(q))
            best = np.array([a + int(np.argmax(sc[a:b])) for a, b in zip(start[:-1], start[1:])])
            img = sc[best].copy()
            img[list(ex or [])] = -np.inf
            order = np.argsort(-img, kind="stable")[:K + 1]
            order = order[np.isfinite(img[order])]
            assert np.all(-np.diff(img[order]) > 2 * bound.max()), (name, s, "reseed: a gap within twice the bound")
            for p in order[:K]:  # and the best tile of a returned image leads its other tiles by as much
                tiles = np.sort(sc[start[p]:start[p + 1]])
                assert tiles.size == 1 or tiles[-1] - tiles[-2] > 2 * bound.max(), (name, s, "reseed: tiles tie")
            self.ref.append((sc, bound, order[:K], best[order[:K]]))

    def open(self):
        from seesaw_amd.device_index import DeviceIndex, view_rows
        r2i = np.repeat(np.arange(len(self.counts)), self.counts).astype(np.int32)
        self.parent = DeviceIndex.from_numpy(self.X, row2image=r2i, dtype=self.dtype)
        self.views = {}
        for name, pos in self.lists.items():
            v = self.parent.view(pos)
            rows, _ = view_rows(self.row_start, pos)
            v.set_tile_meta(self.boxes[rows], self.zoom[rows])
            self.views[name] = v
        return self

    def close(self):
        [v.close() for v in list(self.views.values()) + [self.parent]]

    def check(self, sel=None):
        """one plain and one two-stage call over slots `sel` (all): reference, then the loop of single calls"""
        from seesaw_amd.device_index import DeviceIndex
        sel = list(range(len(self.slots))) if sel is None else sel
        views, ex = [self.views[self.slots[s][0]] for s in sel], [self.slots[s][2] for s in sel]
        got = DeviceIndex.views_topk_batch(views, self.Q[sel], K, excluded=ex)
        avg = DeviceIndex.views_topk_batch_avg(views, self.Q[sel], K, "greater", excluded=ex)
        last = {id(v): j for j, v in enumerate(views)}
        for j, s in enumerate(sel):
            sc, bound, want_img, want_row = self.ref[s]
            imgs, scs, rows = got[j]
            assert np.array_equal(imgs, want_img) and np.array_equal(rows, want_row), (s, self.slots[s][0])
            assert np.all(np.abs(scs.astype(np.float64) - sc[rows]) <= bound[rows]), s
            if last[id(views[j])] == j:  # the view's last slot: its whole slab is resident
                slab = views[j].gather_scores(np.arange(views[j].n_rows)).astype(np.float64)
                assert np.all(np.abs(slab - sc) <= bound), s
        for j, s in enumerate(sel):  # byte for byte the single calls (after the slabs above: they overwrite them)
            one = views[j].topk(self.Q[s], K, excluded=ex[j])
            order = np.argsort(one[0])
            sa, ra = views[j].rescore_avg(one[0][order], "greater")
            for r in (got[j], avg[j][:3]):
                assert all(np.array_equal(a, b) for a, b in zip(r, one)) and np.array_equal(bits(r[1]), bits(one[1])), s
            assert np.array_equal(bits(avg[j][3][order]), bits(sa)) and np.array_equal(avg[j][4][order], ra), s


def open_check_close(case):
    case.open()
    try:
        case.check()
    finally:
        case.close()


# query-seed shifts for which every slot's reference holds the gaps `Case` asserts (found on the CPU, fixed here)
EDGE_SHIFT = {(256, "float32"): 10, (256, "float16"): 17, (512, "float32"): 3, (512, "float16"): 3,
              (768, "float32"): 38, (768, "float16"): 38, (1024, "float32"): 24, (1024, "float16"): 24}


def edge_case(oracle, dim, dtype, shift=None):
    """(a): 300 images of 1-13 tiles; sixteen slots on the kernel's edges"""
    shift = EDGE_SHIFT[(dim, np.dtype(dtype).name)] if shift is None else shift
    counts = np.random.default_rng(5).integers(1, 14, 300)
    counts[::3] = 1
    E = 4 * (8 if dim <= 512 else 4)  # rows a workgroup of the small form takes at steps = 1
    sizes = sorted({1, 63, 64, 65, E - 1, E, E + 1, 2 * E - 1, 2 * E + 1})
    lists = {"r%d" % r: members_with_rows(counts, r, first=r % 50) for r in sizes}
    lists.update(whole=np.arange(300), left=np.arange(0, 180), right=np.arange(120, 300))
    names = list(lists)
    slots = [(nm, shift + 5 * i, None if i % 2 else [0]) for i, nm in enumerate(names)]  # (excluding image 0 of each view)
    slots[names.index("r1")] = ("r1", shift, None)  # its one image stays
    slots += [("left", shift + 71, [2, 5, 9]), ("whole", shift + 72, list(range(0, 300, 7))), ("r65", shift + 73, None),
              ("right", shift + 74, [1]), ("r64", shift + 75, [3]), ("r1", shift + 76, None)]
    return Case(oracle, counts, dim, dtype, 100 + dim, lists, slots[:16])


@pytest.mark.parametrize("dtype", [F32, F16], ids=["f32", "f16"])
@pytest.mark.parametrize("dim", [256, 512, 768, 1024])
def test_edge_shapes(oracle, dim, dtype):
    case = edge_case(oracle, dim, dtype)
    assert len(case.slots) == 16 and sum(s[0] == "left" for s in case.slots) == 2
    open_check_close(case)


@pytest.fixture(scope="module")
def case512(oracle):
    case = edge_case(oracle, 512, F32).open()
    yield case
    case.close()


@pytest.mark.parametrize("ns", [1, 2, 16, 17, 33])
def test_slot_counts(case512, ns):
    case512.check([(7 * i) % 16 for i in range(ns)])


def stream_case(oracle, n_view, dtype, shift=21):
    """(c): 70 000 rows of dim 256, an image a row; a view on either side of the form threshold with a 100-row view"""
    lists = {"big": np.arange(2000, 2000 + n_view), "small": np.arange(500, 600)}
    slots = [("big", shift, None), ("small", shift + 1, [3]), ("big", shift + 2, list(range(0, 60000, 11)))]
    return Case(oracle, np.ones(70000, dtype=np.int64), 256, dtype, 9, lists, slots)


@pytest.mark.parametrize("dtype", [F32, F16], ids=["f32", "f16"])
@pytest.mark.parametrize("n_view", [65535, 65536, 65537])
def test_streaming_form_shares_a_call(oracle, n_view, dtype):
    open_check_close(stream_case(oracle, n_view, dtype))


def test_refusals_launch_nothing(oracle, case512):
    from seesaw_amd import _lib
    from seesaw_amd.device_index import DeviceIndex
    other = DeviceIndex.from_numpy(case512.X[:400], row2image=np.arange(400, dtype=np.int32) // 2)
    stranger = other.view(np.arange(50))
    a, b = case512.views["left"], case512.views["r64"]
    lib, Q, p = _lib.load(), np.ascontiguousarray(case512.Q[:2]), lambda x: ctypes.c_void_p(x.ctypes.data)

    def refused(handles, k, ex_ids, word):
        outs = [np.full((2, 8), 77, dtype=t) for t in (np.int64, np.float32, np.int64)] + [np.full(2, 77, np.int32)]
        offs, ids = np.array([0, 0, len(ex_ids)], dtype=np.int64), np.array(ex_ids + [0], dtype=np.int64)
        arr = (ctypes.c_void_p * 2)(*[h._h for h in handles])
        st = lib.ssw_index_views_topk_batch(arr, p(Q), 2, p(ids), p(offs), k, p(outs[0]), p(outs[1]), p(outs[2]), p(outs[3]))
        assert st == _lib.SSW_ERR_INVALID and word in _lib.last_error(), (st, _lib.last_error())
        assert all(np.all(o == 77) for o in outs)

    try:
        refused([a, case512.parent], 5, [], "ssw_index_views_topk_batch: views[1] is not a view")
        refused([a, stranger], 5, [], "ssw_index_views_topk_batch: views[1] is a view of another parent")
        refused([a, b], 0, [], "k=0")
        refused([a, b], 5, [b.n_images], "excluded image")  # in range for `a`, one past the end for `b`, whose slot it is
    finally:
        stranger.close()
        other.close()


def test_session_group_merges_views_of_one_parent(monkeypatch):
    """four sessions on three subset_views, two on one view: MIN_VIEW_GROUP = 2 shows what they show driven alone"""
    from seesaw_amd.basic_types import IndexSpec, SessionParams
    from seesaw_amd.bitmap import BitMap
    from seesaw_amd.device_index import DeviceIndex
    from seesaw_amd.seesaw_session import Session, SessionGroup
    from seesaw_amd.synthetic import GlobalDataManager, make_dataset
    from test_session_group_gpu import MULTI_REG, SESSIONS, _label, _snapshot
    ds = make_dataset("grp", n_images=200, tiles_per_image=13, n_categories=3, positive_frac=0.08, seed=21, knn_k=10)
    gdm = GlobalDataManager().add(ds)
    full = ds.load_index("multiscale", options={"use_vec_index": False})
    members = [BitMap(sorted(set(range(200)) - set(range(r, 200, 5)))) for r in (3, 1, 2)]
    calls, real = [], DeviceIndex.views_topk_batch_avg
    monkeypatch.setattr(DeviceIndex, "views_topk_batch_avg",
                        staticmethod(lambda *a, **k: calls.append(len(a[0])) or real(*a, **k)))

    Merging = type("Merging", (SessionGroup,), {"MIN_VIEW_GROUP": 2})
    def rounds(grouped):
        views = [full.subset_view(m) for m in members]
        sessions = []
        for (_, _, text, _, policy), view in zip(SESSIONS[:4], views + views[:1]):
            sp = SessionParams(index_spec=IndexSpec(d_name="grp", i_name="multiscale", c_name=None), interactive="multi_reg",
                               interactive_options=MULTI_REG, batch_size=3, shortlist_size=50, agg_method="avg_score",
                               aug_larger="greater", start_policy=policy, index_options={"use_vec_index": False})
            sessions.append(Session(gdm, ds, view, sp))
            sessions[-1].set_text(text)
        group, trace = Merging(sessions), []
        for _ in range(3):
            # query_groups(): as without the feature, keyed on the index object
            assert group.query_groups() == [(0, 3), (1,), (2,)] and group.view_groups() == [(0, 1, 2, 3)]
            group.next() if grouped else [s.next() for s in sessions]
            for s, spec in zip(sessions, SESSIONS):
                _label(s, spec[3], ds)
            group.refine() if grouped else [s.refine() for s in sessions]
            trace.append([_snapshot(s) for s in sessions])
        for v in views:
            v._dev.close()
        return trace

    try:
        alone = rounds(False)
        together = rounds(True)
    finally:
        full._dev.close()
    assert calls == [4, 4, 4]
    for r, (a, t) in ((r, at) for r in range(3) for at in zip(alone[r], together[r])):
        assert len(a["dbidxs"]) == 3 and a["activations"] == t["activations"] and a["started"] == t["started"], r
        assert all(np.array_equal(a[key], t[key]) for key in ("dbidxs", "returned", "curr_vec")), r

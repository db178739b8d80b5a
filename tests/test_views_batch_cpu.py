"""CPU: SessionGroup.view_groups() on stubs; DeviceIndex.views_topk_batch*'s argument checks (raised before the library)"""
import types

import numpy as np
import pytest


def _session(loop_cls, index, *, started=True, agg_method="avg_score", two_vectors=False):
    params = types.SimpleNamespace(batch_size=3, shortlist_size=50, agg_method=agg_method, aug_larger="greater")
    loop = object.__new__(loop_cls)
    loop.params, loop.started = params, started
    loop.q = types.SimpleNamespace(index=index, returned=set())
    loop.curr_qvec, loop.curr_vec = np.ones(4, np.float32), np.full(4, 2.0, np.float32)
    if two_vectors:
        loop.confusion_vec, loop.options = np.ones(4, np.float32), {"discount_neg": True}
    return types.SimpleNamespace(loop=loop, params=params, q=loop.q)


def test_view_groups_on_stub_sessions():
    from seesaw_amd.loops.multi_reg import MultiReg
    from seesaw_amd.loops.multi_reg_neg import MultiRegNeg
    from seesaw_amd.seesaw_session import SessionGroup
    Idx = type("Idx", (), {"query_batch_views": staticmethod(lambda *a, **k: None)})
    p1, p2 = object(), object()

    def view_index(parent):
        ix = Idx()
        ix._dev = types.SimpleNamespace(is_view=parent is not None, parent=parent)
        return ix

    a, b, c, d, other, whole = [view_index(p) for p in (p1, p1, p1, p1, p2, None)]
    sessions = [
        _session(MultiReg, a),                          # 0
        _session(MultiReg, b),                          # 1: another view of the same parent: with 0
        _session(MultiReg, a, started=False),           # 2: the same view as 0: one query group with it
        _session(MultiReg, other),                      # 3: a view of another parent
        _session(MultiReg, c, agg_method="plain_score"),  # 4: another agg_method
        _session(MultiRegNeg, c, two_vectors=True),     # 5: asks with a second vector: today's route
        _session(MultiReg, whole),                      # 6: not a view
        _session(MultiReg, c),                          # 7: in 5's query group, which keeps its route whole
        _session(MultiReg, d),                          # 8: with 0, 1, 2
    ]
    g = SessionGroup(sessions)
    assert g.query_groups() == [(0, 2), (1,), (3,), (4,), (5, 7), (6,), (8,)]  # keyed on the index object, as before
    assert g.view_groups() == [(0, 1, 2, 8), (3,), (4,)]
    assert SessionGroup.MIN_VIEW_GROUP is None  # not ahead when measured: next() keeps the route of query_groups()
    served = []
    Merging = type("Merging", (SessionGroup,), {"MIN_VIEW_GROUP": 4, "_next_views": lambda self, g, out: served.append(g)})

    def next_of(cls, members, **kw):  # (the stubs cannot answer a query: only the merged route is looked at)
        del served[:]
        grp = cls([sessions[i] for i in members], **kw)
        merged = grp.view_groups()
        grp.view_groups, grp.query_groups = (lambda: merged), (lambda: [])
        grp.next()
        return list(served)

    assert next_of(Merging, range(9)) == [(0, 1, 2, 8)]
    assert next_of(Merging, (0, 1, 2)) == []              # below MIN_VIEW_GROUP
    assert next_of(Merging, range(9), prune=True) == []   # prune keeps today's route
    assert next_of(SessionGroup, range(9)) == []          # None: never


def test_wrapper_argument_checks_need_no_device():
    from seesaw_amd.device_index import DeviceIndex

    def stub(parent, is_view=True, dim=512):
        v = object.__new__(DeviceIndex)
        v._h, v.dim, v.is_view, v.parent = None, dim, is_view, parent  # (`_h` None: close() has nothing to destroy)
        return v

    p1, p2 = stub(None, False), stub(None, False)
    a, b, c = stub(p1), stub(p1), stub(p2)
    Q = np.zeros((2, 512), np.float32)
    for fn, extra in ((DeviceIndex.views_topk_batch, ()), (DeviceIndex.views_topk_batch_avg, ("greater",))):
        for views, q, ex, word in (([], Q, None, "at least one"), ([a, p1], Q, None, r"views\[1\] is not a view"),
                                   ([a, c], Q, None, "another parent"), ([a, b], Q[:1], None, "one query a slot"),
                                   ([a, b], np.zeros((2, 256), np.float32), None, "queries must be"),
                                   ([a, b], Q, [None], "1 lists for 2")):
            with pytest.raises(ValueError, match=word):
                fn(views, q, 5, *extra, excluded=ex)

"""CPU: the batched fit's interface (header, ctypes table), RegModule's stage / engine call / finish split against the
engine calls the one-piece `fit` made, and SessionGroup's grouping rules on stub sessions.  No GPU compute."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fit_batch_is_declared_and_bound_with_its_signature():
    from seesaw_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    m = re.search(r"ssw_status\s+ssw_fb_fit_batch\s*\((.*?)\)\s*;", text, re.S)
    assert m, "ssw_fb_fit_batch is not declared in include/seesaw_hip.h"
    params = [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]
    assert params == ["ssw_fb *const *fbs", "const ssw_fb_objective *objs", "int32_t nfit", "float *W_inout",
                      "const int32_t *max_iter", "const float *lr", "int32_t *out_iters", "int32_t *out_evals",
                      "float *out_final_loss", "int32_t *out_status"]
    restype, argtypes = _lib._SIGNATURES["ssw_fb_fit_batch"]
    i32p, f32p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_float)
    assert restype is ctypes.c_int32
    assert argtypes == [ctypes.POINTER(ctypes.c_void_p), ctypes.c_void_p, ctypes.c_int32, f32p, i32p, f32p, i32p, i32p,
                        f32p, i32p]
    assert "ssw_fb_fit_batch" in _lib.declared_symbols()
    from seesaw_amd.feedback import FeedbackEngine
    assert isinstance(FeedbackEngine.__dict__["fit_batch"], staticmethod)


class _StubEngine:
    """records every call RegModule makes; `fit` answers with a fixed vector"""

    def __init__(self, dim, answer=None):
        self.dim, self.device, self.calls, self.answer = dim, 0, [], answer

    def _rec(self, name, *args, **kw):
        self.calls.append((name, args, kw))

    def set_xlx(self, m):
        self._rec("set_xlx", m)

    def set_query(self, q):
        self._rec("set_query", q)

    def set_data(self, X, center):
        self._rec("set_data", X, center=center)

    def set_data_from_index(self, index, rows, center):
        self._rec("set_data_from_index", index, rows, center=center)

    def set_targets(self, y, sample_weight=None):
        self._rec("set_targets", y, sample_weight)

    def fit(self, obj, w0, max_iter, lr=1.0):
        self._rec("fit", obj, w0, max_iter=max_iter, lr=lr)
        if isinstance(self.answer, Exception):
            raise self.answer
        return self.answer, {"n_iter": 3, "func_evals": 4, "loss": 0.25, "on_device": True}


def _module(engine, dim=8):
    from seesaw_amd.loops.multi_reg import RegModule
    q = np.arange(1, dim + 1, dtype=np.float32)
    return RegModule(dim=dim, xlx_matrix=None, qvec=q, label_loss_type="ce_loss", reg_data_lambda=0.0,
                     reg_norm_lambda=100.0, reg_query_lambda=1.0, use_qvec_norm=None, rank_loss_margin=0.2,
                     pos_weight="balanced", max_iter=17, lr=0.5, engine=engine)


def _same(a, b):
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return a is not None and b is not None and np.asarray(a).dtype == np.asarray(b).dtype and np.array_equal(a, b)
    if isinstance(a, ctypes.Structure):
        return bytes(a) == bytes(b)
    return a == b


def _assert_calls(got, want):
    assert [c[0] for c in got] == [c[0] for c in want]
    for (name, ga, gk), (_, wa, wk) in zip(got, want):
        assert len(ga) == len(wa) and sorted(gk) == sorted(wk), name
        assert all(_same(x, y) for x, y in zip(ga, wa)), (name, ga, wa)
        assert all(_same(gk[k], wk[k]) for k in wk), (name, gk, wk)


@pytest.mark.parametrize("case", ["host_rows", "index_rows", "unsorted_images", "no_rows"])
def test_fit_from_its_parts_makes_the_engine_calls_of_the_one_piece_fit(case):
    """the calls below are listed from RegModule.fit as it stood in one piece: set_data (or set_data_from_index,
    centred) then set_targets(y as f64, 1 / tiles of the image), or for an empty set set_data(zeros [0, dim], no
    centring) and set_targets(zeros(0)); then fit(objective, weight, max_iter=, lr=)"""
    dim = 8
    rng = np.random.default_rng(1)
    answer = rng.standard_normal(dim).astype(np.float32)
    dbidx = {"unsorted_images": np.array([4, 2, 4, 9, 2, 4]), "no_rows": np.zeros(0, np.int64)}.get(
        case, np.array([2, 2, 4, 4, 4, 9]))
    n = dbidx.shape[0]
    X = rng.standard_normal((n, dim)).astype(np.float32)
    y = (np.arange(n) % 2).astype("float")
    rows, index = np.arange(n) * 3, object()
    counts = {int(d): int((dbidx == d).sum()) for d in dbidx}
    weight = np.array([1.0 / counts[int(d)] for d in dbidx], dtype=np.float64)
    eng = _StubEngine(dim, answer)
    m = _module(eng, dim)
    w0 = m.weight.copy()
    set_up = list(eng.calls)
    assert [c[0] for c in set_up] == ["set_query"]
    if case == "no_rows":
        want = [("set_data", (np.zeros((0, dim), np.float32),), {"center": False}), ("set_targets", (np.zeros(0), None), {})]
    elif case == "index_rows":
        want = [("set_data_from_index", (index, rows), {"center": True}), ("set_targets", (y.astype(np.float64), weight), {})]
    else:
        want = [("set_data", (X,), {"center": True}), ("set_targets", (y.astype(np.float64), weight), {})]
    want.append(("fit", (m._objective(), w0), {"max_iter": 17, "lr": 0.5}))
    args = (None, y, dbidx, index, rows) if case == "index_rows" else (X, y, dbidx)
    # the parts, by hand
    m._stage(*args)
    w, info = eng.fit(m._objective(), m.weight, max_iter=m.max_iter, lr=m.lr)
    out = m._finish(w, info)
    _assert_calls(eng.calls[len(set_up):], want)
    assert out == [{"k": "total_loss", "loss": 0.25}] and m.weight is answer and m.info_ == info
    # and `fit`, which is the three in a row
    eng2 = _StubEngine(dim, answer)
    m2 = _module(eng2, dim)
    assert m2.fit(*args) == out
    _assert_calls(eng2.calls[len(set_up):], want)
    assert m2.weight is answer and np.array_equal(m2.get_coeff(), m.get_coeff())


def test_a_fit_that_raised_surfaces_through_finish_with_fit_s_text():
    from seesaw_amd import _lib
    err = _lib.SeesawHipError(_lib.SSW_ERR_NUMERIC, "feedback: loss diverged -- regression training failed with a nan")
    m = _module(_StubEngine(8, err))
    before = m.weight.copy()
    with pytest.raises(AssertionError) as single:
        m.fit(np.ones((2, 8), np.float32), np.array([1.0, 0.0]), np.array([1, 2]))
    with pytest.raises(AssertionError) as parts:
        m._finish(err, None)
    assert str(single.value) == str(parts.value) == f"regression training failed: {err}"
    assert np.array_equal(m.weight, before) and m.info_ is None


def test_refine_batch_sets_every_vector_before_a_failed_slot_raises(monkeypatch):
    """one engine call for all loops; the loop whose fit diverged raises `fit`'s AssertionError after the others have
    their vectors, and keeps its own"""
    from seesaw_amd import _lib
    from seesaw_amd.feedback import FeedbackEngine
    from seesaw_amd.loops.multi_reg import MultiReg, RegModule
    dim = 8
    err = _lib.SeesawHipError(_lib.SSW_ERR_NUMERIC, "feedback: weights diverged")
    answers = [np.full(dim, 2.0, np.float32), err, np.arange(1, dim + 1, dtype=np.float32)]
    info = {"n_iter": 1, "func_evals": 2, "loss": 0.5, "on_device": True}
    calls = []

    def fake_fit_batch(engines, objs, w0s, max_iters, lrs):
        calls.append((list(engines), list(max_iters), list(lrs)))
        assert all(e.calls[-1][0] == "set_targets" for e in engines)  # every loop staged before the one call
        return [a if isinstance(a, Exception) else (a, dict(info)) for a in answers]

    monkeypatch.setattr(FeedbackEngine, "fit_batch", staticmethod(fake_fit_batch))
    loops = []
    for i in range(3):
        loop = object.__new__(MultiReg)
        loop._engine = _StubEngine(dim)
        loop.curr_vec = np.full(dim, -1.0, np.float32)
        loop._fit_args = lambda: (np.ones((2, dim), np.float32), np.array([1.0, 0.0]), np.array([3, 4]), None, None)
        loop._model = lambda loop=loop: _module(loop._engine, dim)
        loops.append(loop)
    with pytest.raises(AssertionError) as ei:
        MultiReg.refine_batch(loops)
    assert str(ei.value) == f"regression training failed: {err}"
    assert len(calls) == 1 and calls[0][0] == [l._engine for l in loops] and calls[0][1] == [17] * 3
    assert np.allclose(loops[0].curr_vec, 1 / np.sqrt(dim)) and np.array_equal(loops[1].curr_vec, np.full(dim, -1.0))
    assert np.array_equal(loops[2].curr_vec, (answers[2] / np.linalg.norm(answers[2])).astype(np.float32))
    assert isinstance(RegModule.__dict__["fit_batch"], staticmethod)
    MultiReg.refine_batch([])  # nothing to do, nothing called
    assert len(calls) == 1


# ---- SessionGroup's grouping, on stubs ------------------------------------------------------------------------
def _stub_session(loop_cls, index, *, started, batch_size=3, shortlist_size=50, agg_method="plain_score",
                  aug_larger="greater", dim=512, device=0):
    params = types.SimpleNamespace(batch_size=batch_size, shortlist_size=shortlist_size, agg_method=agg_method,
                                   aug_larger=aug_larger)
    loop = object.__new__(loop_cls)
    loop.params, loop.started = params, started
    loop.q = types.SimpleNamespace(index=index, returned=set())
    loop.curr_qvec = np.ones(4, np.float32)
    loop.curr_vec = np.full(4, 2.0, np.float32)
    loop._engine = types.SimpleNamespace(dim=dim, device=device)
    return types.SimpleNamespace(loop=loop, params=params, q=loop.q)


def test_session_group_grouping_rules():
    from seesaw_amd.loops.graph_based import KnnProp2
    from seesaw_amd.loops.multi_reg import MultiReg
    from seesaw_amd.loops.multi_reg_neg import MultiRegNeg
    from seesaw_amd.loops.point_based import Plain
    from seesaw_amd.loops.random_results import RandomResults
    from seesaw_amd.seesaw_session import SessionGroup
    a, b = object(), object()
    sessions = [
        _stub_session(MultiReg, a, started=True),                       # 0
        _stub_session(Plain, a, started=False),                         # 1: same query batch as 0
        _stub_session(KnnProp2, a, started=True),                       # 2: its own next_batch
        _stub_session(KnnProp2, a, started=False),                      # 3: start policy not fired: the text vector
        _stub_session(MultiReg, b, started=True),                       # 4: another index object
        _stub_session(MultiReg, a, started=True, batch_size=5),         # 5: another batch size
        _stub_session(MultiReg, a, started=False, agg_method="avg_score"),  # 6
        _stub_session(MultiReg, a, started=True, agg_method="avg_score"),   # 7: with 6
        _stub_session(RandomResults, a, started=False),                 # 8: never asks the index with a vector
        _stub_session(MultiRegNeg, a, started=True),                    # 9: a PointBased loop with its own next_batch
        _stub_session(MultiReg, b, started=True, shortlist_size=40),    # 10
        _stub_session(MultiReg, a, started=True, aug_larger="all"),     # 11
        _stub_session(MultiReg, a, started=True, dim=256),              # 12: with 0 in the query, not in the fit
    ]
    g = SessionGroup(sessions)
    assert g.query_groups() == [(0, 1, 3, 12), (2,), (4,), (5,), (6, 7), (8,), (9,), (10,), (11,)]
    vec = SessionGroup.batch_vector
    assert vec(sessions[0].loop) is sessions[0].loop.curr_vec       # started PointBased: the refined vector
    assert vec(sessions[1].loop) is sessions[1].loop.curr_qvec      # not started: the text vector
    assert vec(sessions[3].loop) is sessions[3].loop.curr_qvec
    assert vec(sessions[2].loop) is None and vec(sessions[8].loop) is None and vec(sessions[9].loop) is None
    batched, alone = g.fit_groups()
    # started MultiReg loops refine together, per (dim, device); every other loop on its own
    assert batched == [(0, 4, 5, 7, 10, 11), (12,)]
    assert alone == [1, 2, 3, 6, 8, 9]
    assert SessionGroup(sessions, prune=True).prune is True and g.prune is False


def test_session_group_hands_single_sessions_to_their_own_calls():
    """groups of one go through Session.next() / Session.refine() themselves"""
    from seesaw_amd.loops.graph_based import KnnProp2
    from seesaw_amd.seesaw_session import SessionGroup
    log = []
    s = _stub_session(KnnProp2, object(), started=True)
    s.next = lambda: log.append("next") or [7]
    s.refine = lambda: log.append("refine")
    g = SessionGroup([s])
    assert g.next() == [[7]]
    g.refine()
    assert log == ["next", "refine"]

"""CPU: the batched L-KNN step's interface (header, exported symbols, ctypes table), its whole-call refusals -- decided
before the device is touched -- and SessionGroup's grouping of the active-search loops on stub sessions.  No GPU compute."""
import ctypes
import re
import subprocess
import types

import numpy as np

INVALID = -1  # SSW_ERR_INVALID


def test_the_three_symbols_are_declared_exported_and_bound():
    from seesaw_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    want = {
        "ssw_lknn_step_batch": ["ssw_lknn *const *hs", "int32_t n_slots", "const int32_t *K", "const int32_t *lookahead",
                                "int64_t *out_best_idx", "double *out_best_value", "double *const *out_values_or_null",
                                "int32_t *out_lists_or_null", "int32_t *out_status", "int64_t *out_stats4_or_null"],
        "ssw_lknn_top_remaining_batch": ["ssw_lknn *const *hs", "int32_t n_slots", "const int32_t *k", "int32_t *out_ids",
                                         "double *out_scores", "int32_t *out_counts", "int32_t *out_status"],
    }
    for name, params in want.items():
        m = re.search(r"ssw_status\s+%s\s*\((.*?)\)\s*;" % name, text, re.S)
        assert m, f"{name} is not declared in include/seesaw_hip.h"
        assert [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")] == params
        restype, argtypes = _lib._SIGNATURES[name]
        assert restype is ctypes.c_int32 and len(argtypes) == len(params)
        for p, t in zip(params, argtypes):
            if "*const *" in p:
                assert t == ctypes.POINTER(ctypes.c_void_p), p
            elif "*" in p:
                assert t is ctypes.c_void_p, p
            else:
                assert t is ctypes.c_int32, p
    assert re.search(r"const char\s*\*\s*ssw_lknn_batch_error\s*\(\s*const ssw_lknn \*h\s*\)\s*;", text)
    assert _lib._SIGNATURES["ssw_lknn_batch_error"] == (ctypes.c_char_p, [ctypes.c_void_p])
    assert re.search(r"#define\s+SSW_LKNN_MAX_BATCH\s+256\b", text)
    names = {"ssw_lknn_step_batch", "ssw_lknn_top_remaining_batch", "ssw_lknn_batch_error"}
    assert names <= set(_lib.declared_symbols())
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert names <= {line.split()[-1] for line in exported.splitlines() if line.strip()}
    lib = _lib.load()
    for name in names:
        assert getattr(lib, name) is not None
    from seesaw_amd.loops.active_search import ActiveSearch, LKNNSearch
    from seesaw_amd.loops.LKNN_model import DeviceLKNNModel
    assert isinstance(DeviceLKNNModel.__dict__["step_batch"], staticmethod)
    assert isinstance(DeviceLKNNModel.__dict__["top_k_remaining_batch"], staticmethod)
    assert isinstance(ActiveSearch.__dict__["next_batch_group"], classmethod)
    assert isinstance(LKNNSearch.__dict__["next_batch_group"], classmethod)
    assert DeviceLKNNModel.MAX_BATCH == 256


def _step_batch(lib, hs, n_slots, *, K=True, lookahead=True, best_i=True, best_v=True, status=True):
    S = max(1, abs(n_slots))
    keep = [np.zeros(S, dtype=np.int64) for _ in range(5)]  # the arrays outlive the call
    ptr = lambda a, on: ctypes.c_void_p(a.ctypes.data) if on else None
    return lib.ssw_lknn_step_batch(hs, n_slots, ptr(keep[0].view(np.int32), K), ptr(keep[1].view(np.int32), lookahead),
                                   ptr(keep[2], best_i), ptr(keep[3].view(np.float64), best_v), None, None,
                                   ptr(keep[4].view(np.int32), status), None)


def _top_remaining_batch(lib, hs, n_slots, *, k=True, ids=True, scores=True, counts=True, status=True):
    S = max(1, abs(n_slots))
    keep = [np.zeros(S, dtype=np.int32), np.zeros((S, 192), dtype=np.int32), np.zeros((S, 192), dtype=np.float64),
            np.zeros(S, dtype=np.int32), np.zeros(S, dtype=np.int32)]
    on = (k, ids, scores, counts, status)
    return lib.ssw_lknn_top_remaining_batch(hs, n_slots, *[ctypes.c_void_p(a.ctypes.data) if o else None for a, o in zip(keep, on)])


def test_whole_call_refusals_come_before_the_device_is_touched():
    """n_slots outside [1, 256], a NULL handle array, a NULL handle in it: SSW_ERR_INVALID with a message, decided on the
    arguments alone (no handle exists here, so nothing could have been enqueued)"""
    from seesaw_amd import _lib
    lib = _lib.load()
    nulls = (ctypes.c_void_p * 3)(None, None, None)
    for call in (_step_batch, _top_remaining_batch):
        for n_slots in (0, -1, 257):
            assert call(lib, nulls, n_slots) == INVALID
            assert b"n_slots" in lib.ssw_last_error()
        assert call(lib, None, 2) == INVALID
        assert b"NULL" in lib.ssw_last_error()
        assert call(lib, nulls, 3) == INVALID
        assert b"handle 0 is NULL" in lib.ssw_last_error()
        assert call(lib, nulls, 3, status=False) == INVALID   # a NULL array is refused before any handle is looked at
        assert b"NULL argument" in lib.ssw_last_error()
    assert _step_batch(lib, nulls, 3, K=False) == INVALID and b"NULL argument" in lib.ssw_last_error()
    assert _top_remaining_batch(lib, nulls, 3, ids=False) == INVALID and b"NULL argument" in lib.ssw_last_error()
    assert lib.ssw_lknn_batch_error(None) == b""


def test_the_model_layer_raises_the_whole_call_refusal():
    import pytest
    from seesaw_amd import _lib
    from seesaw_amd.loops.LKNN_model import DeviceLKNNModel
    with pytest.raises(_lib.SeesawHipError) as err:
        DeviceLKNNModel.step_batch([], [], [])
    assert err.value.status == INVALID and "n_slots" in str(err.value)
    with pytest.raises(_lib.SeesawHipError) as err:
        DeviceLKNNModel.top_k_remaining_batch([], [])
    assert err.value.status == INVALID and "n_slots" in str(err.value)


# ---- the loop layer on stubs: what runs on the host around the one call ------------------------------------------------
def _planner(returned, *, reward_horizon=10, adjust_horizon=False, max_steps=100):
    import pandas as pd
    from seesaw_amd.loops.active_search import ActiveSearch
    loop = object.__new__(ActiveSearch)
    loop.params = types.SimpleNamespace(interactive_options=dict(reward_horizon=reward_horizon, adjust_horizon=adjust_horizon,
                                                                 max_steps=max_steps, pruning_on=False, implementation="vectorized"))
    index = types.SimpleNamespace(vector_meta=pd.DataFrame({"dbidx": np.arange(100, 200)}))
    loop.q = types.SimpleNamespace(index=index, returned=set(returned))
    loop.prob_model = types.SimpleNamespace(device_resident=True)
    loop.pruned_fractions = []
    return loop


def test_next_batch_group_works_out_every_horizon_first_and_serves_the_others_when_a_slot_fails(monkeypatch, capsys):
    import pytest
    from seesaw_amd import _lib
    from seesaw_amd.loops import active_search
    from seesaw_amd.loops.active_search import ActiveSearch
    from seesaw_amd.research.active_search.common import Result
    asked = []

    def search(models, horizons, lookaheads, return_errors=False):
        asked.append((list(horizons), list(lookaheads), return_errors))
        return answers

    monkeypatch.setattr(active_search, "efficient_nonmyopic_search_batch", search)
    # the third member has used its max_steps up: its own next_batch would assert, so nothing is asked for anybody
    loops = [_planner([]), _planner([1, 2]), _planner(range(12), adjust_horizon=True, max_steps=12)]
    with pytest.raises(AssertionError, match="horizon"):
        ActiveSearch.next_batch_group(loops)
    assert asked == [] and all(l.pruned_fractions == [] for l in loops) and loops[1].q.returned == {1, 2}
    # horizons per loop: 10; 5; max_steps - shown = 1, the one-step branch
    loops = [_planner([]), _planner([1], reward_horizon=5), _planner(range(11), adjust_horizon=True, max_steps=12)]
    answers = [Result(value=1.5, index=7, pruned_fraction=0.0), Result(value=0.5, index=3, pruned_fraction=0.0),
               Result(value=0.25, index=99, pruned_fraction=0.0)]
    out = ActiveSearch.next_batch_group(loops)
    assert asked == [([10, 5, 1], [2, 2, 1], True)]
    assert [o["dbidxs"].tolist() for o in out] == [[107], [103], [199]] and all(o["activations"] is None for o in out)
    assert loops[0].q.returned == {107} and loops[1].q.returned == {1, 103} and 199 in loops[2].q.returned
    assert all(l.pruned_fractions == [0.0] for l in loops)
    assert capsys.readouterr().out.splitlines() == ["res.index=7, res.value=1.5", "res.index=3, res.value=0.5",
                                                    "res.index=99, res.value=0.25"]
    # a refused slot: the others are served as their own next_batch serves them, then the first error is raised
    loops = [_planner([]), _planner([]), _planner([])]
    answers = [Result(value=1.5, index=7, pruned_fraction=0.0), _lib.SeesawHipError(-1, "lknn: K + D = 19 exceeds the 18 unseen nodes"),
               Result(value=0.25, index=9, pruned_fraction=0.0)]
    with pytest.raises(_lib.SeesawHipError, match="unseen"):
        ActiveSearch.next_batch_group(loops)
    assert loops[0].q.returned == {107} and loops[1].q.returned == set() and loops[2].q.returned == {109}
    assert [l.pruned_fractions for l in loops] == [[0.0], [], [0.0]]


def test_search_batch_asserts_per_member_before_the_call(monkeypatch):
    import pytest
    from seesaw_amd.research.active_search.efficient_nonmyopic_search import efficient_nonmyopic_search_batch
    calls = []

    class Model:
        device_resident = True

        @staticmethod
        def step_batch(models, Ks, lookaheads):
            calls.append((list(Ks), list(lookaheads)))
            return [(4, 2.5), ValueError("refused")][:len(models)]

    for horizons, lookaheads in [([5, 0], [2, 1]), ([5, 1], [2, 2]), ([5, 5], [2, 3])]:
        with pytest.raises(AssertionError):
            efficient_nonmyopic_search_batch([Model(), Model()], horizons, lookaheads)
    with pytest.raises(AssertionError, match="device-resident"):
        efficient_nonmyopic_search_batch([Model(), object()], [5, 5], [2, 2])
    assert calls == []
    res = efficient_nonmyopic_search_batch([Model()], [5], [2])
    assert calls == [([4], [2])] and (res[0].index, res[0].value, res[0].pruned_fraction) == (4, 2.5, 0.0)
    with pytest.raises(ValueError, match="refused"):
        efficient_nonmyopic_search_batch([Model(), Model()], [5, 1], [2, 1])
    res = efficient_nonmyopic_search_batch([Model(), Model()], [5, 1], [2, 1], return_errors=True)
    assert res[0].index == 4 and isinstance(res[1], ValueError)


# ---- SessionGroup.planning_groups on stubs ----------------------------------------------------------------------------
def _model(n=3000, degree=10, device=0):
    from seesaw_amd.loops.LKNN_model import DeviceLKNNModel
    return DeviceLKNNModel(dataset=None, owner=None, n=n, degree=degree, device=device)  # no handle: nothing is called


def _session(loop_cls, model, *, started=True, log=None, name=None):
    params = types.SimpleNamespace(batch_size=1, shortlist_size=50, agg_method="plain_score", aug_larger="greater")
    loop = object.__new__(loop_cls)
    loop.params, loop.started, loop.prob_model = params, started, model
    loop.q = types.SimpleNamespace(index=types.SimpleNamespace(), returned=set())
    loop.curr_qvec = np.ones(4, np.float32)
    s = types.SimpleNamespace(loop=loop, params=params, q=loop.q, timing=[], acc_indices=[], acc_activations=[])
    if log is not None:
        s._log = lambda msg: log.append((name, msg))
        s.next = lambda: log.append((name, "own next")) or name
    return s


def test_planning_groups_on_stub_loops():
    from seesaw_amd.loops.active_search import ActiveSearch, LKNNSearch
    from seesaw_amd.loops.point_based import Plain
    from seesaw_amd.seesaw_session import SessionGroup

    class OwnSearch(ActiveSearch):
        pass

    class OwnGate(LKNNSearch):
        def next_batch_external(self):
            pass

    host = types.SimpleNamespace(device=0, n=3000, degree=10)  # stands for the host LKNNModel: not a DeviceLKNNModel
    g = SessionGroup([_session(ActiveSearch, host), _session(LKNNSearch, host), _session(Plain, None)])
    assert g.planning_groups() == []
    sessions = [
        _session(LKNNSearch, _model()),                  # 0
        _session(ActiveSearch, _model()),                # 1
        _session(LKNNSearch, _model()),                  # 2: with 0
        _session(ActiveSearch, _model(n=5000)),          # 3: another node count: a group of one
        _session(OwnSearch, _model()),                   # 4: a subclass answers on its own
        _session(OwnGate, _model()),                     # 5
        _session(ActiveSearch, _model(), started=False), # 6: start policy not fired
        _session(ActiveSearch, host),                    # 7: the host model
        _session(ActiveSearch, _model()),                # 8: with 1
        _session(LKNNSearch, _model(degree=5)),          # 9: another degree
        _session(LKNNSearch, _model(device=1)),          # 10: another device
        _session(Plain, None),                           # 11
        _session(LKNNSearch, _model()),                  # 12: with 0 and 2
    ]
    g = SessionGroup(sessions)
    queries = g.query_groups()
    assert g.planning_groups() == [(0, 2, 12), (1, 8), (3,), (9,), (10,)]
    assert g.query_groups() == queries and all((i,) in queries for i in (0, 1, 2, 3, 8, 9, 10, 12))


def test_next_routes_a_group_from_its_minimum_size_on(monkeypatch):
    from seesaw_amd.loops.active_search import ActiveSearch, LKNNSearch
    from seesaw_amd.seesaw_session import SessionGroup
    log, calls = [], []

    def group_call(cls, loops):
        calls.append((cls.__name__, list(loops)))
        return [{"dbidxs": np.array([10 + len(calls)]), "activations": None} for _ in loops]

    monkeypatch.setattr(ActiveSearch, "next_batch_group", classmethod(group_call))
    monkeypatch.setattr(LKNNSearch, "next_batch_group", classmethod(group_call))
    sessions = [_session(LKNNSearch, _model(), log=log, name=0), _session(ActiveSearch, _model(), log=log, name=1),
                _session(LKNNSearch, _model(), log=log, name=2), _session(ActiveSearch, _model(), log=log, name=3),
                _session(LKNNSearch, _model(), log=log, name=4)]
    # the routing constants as committed decide nothing here: switched off, every session answers on its own
    monkeypatch.setattr(SessionGroup, "MIN_LKNN_GROUP", None)
    monkeypatch.setattr(SessionGroup, "MIN_ACTIVE_SEARCH_GROUP", None)
    g = SessionGroup(sessions)
    assert g.next() == [0, 1, 2, 3, 4] and calls == []
    assert [e for e in log if e[1] == "own next"] == [(i, "own next") for i in range(5)]
    # lknn from 3 members on, active_search from 3: the three lknn sessions share one call, the two others do not
    log.clear()
    monkeypatch.setattr(SessionGroup, "MIN_LKNN_GROUP", 3)
    monkeypatch.setattr(SessionGroup, "MIN_ACTIVE_SEARCH_GROUP", 3)
    out = g.next()
    assert calls == [("LKNNSearch", [sessions[0].loop, sessions[2].loop, sessions[4].loop])]
    assert log == [(0, "next.start"), (2, "next.start"), (4, "next.start"), (0, "next.end"), (2, "next.end"), (4, "next.end"),
                   (1, "own next"), (3, "own next")]
    assert [int(out[i][0]) for i in (0, 2, 4)] == [11, 11, 11] and (out[1], out[3]) == (1, 3)
    for i in (0, 2, 4):
        s = sessions[i]
        assert len(s.timing) == 1 and s.timing[0] == sessions[0].timing[0]       # the shared call's time for each member
        assert [a.tolist() for a in s.acc_indices] == [[11]] and s.acc_activations == [None]
    assert sessions[1].timing == [] and sessions[1].acc_indices == []
    # a minimum of 1 still leaves a single loop to its own next(): a group has at least two members
    log.clear(), calls.clear()
    monkeypatch.setattr(SessionGroup, "MIN_ACTIVE_SEARCH_GROUP", 1)
    monkeypatch.setattr(SessionGroup, "MIN_LKNN_GROUP", None)
    g2 = SessionGroup(sessions[:2])
    g2.next()
    assert calls == [] and [e for e in log if e[1] == "own next"] == [(0, "own next"), (1, "own next")]

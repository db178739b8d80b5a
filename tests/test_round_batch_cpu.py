"""CPU: the batched graph round's interface (header, ctypes table), the offset packing of round_batch's arguments, and
SessionGroup's grouping of graph loops on stub sessions.  No GPU compute."""
import ctypes
import re
import types

import numpy as np
import pytest


def test_round_batch_is_declared_and_bound_with_its_signature():
    from seesaw_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    m = re.search(r"ssw_status\s+ssw_labelprop_round_batch\s*\((.*?)\)\s*;", text, re.S)
    assert m, "ssw_labelprop_round_batch is not declared in include/seesaw_hip.h"
    params = [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]
    assert params == ["ssw_lp *const *lps", "int32_t n_slots", "ssw_index *index", "const int32_t *propagate",
                      "const int64_t *label_ids", "const double *label_vals", "const int64_t *label_offsets",
                      "const double *reg_lambda", "const double *eps", "const int32_t *max_iter", "int32_t mask_labeled",
                      "const int64_t *excluded_images", "const int64_t *excluded_offsets", "int32_t k", "int64_t *out_images",
                      "float *out_scores", "int64_t *out_best_rows", "int32_t *out_counts", "int32_t *out_sweeps",
                      "int32_t *out_converged", "int32_t *out_status", "int64_t *out_stats4"]
    restype, argtypes = _lib._SIGNATURES["ssw_labelprop_round_batch"]
    assert restype is ctypes.c_int32 and len(argtypes) == len(params)
    for p, t in zip(params, argtypes):
        if p.startswith("int32_t ") and "*" not in p:
            assert t is ctypes.c_int32, p
        elif p == "ssw_lp *const *lps":
            assert t == ctypes.POINTER(ctypes.c_void_p), p
        else:
            assert t is ctypes.c_void_p, p
    assert re.search(r"const char\s*\*\s*ssw_labelprop_batch_error\s*\(\s*const ssw_lp \*lp\s*\)\s*;", text)
    assert _lib._SIGNATURES["ssw_labelprop_batch_error"] == (ctypes.c_char_p, [ctypes.c_void_p])
    declared = _lib.declared_symbols()
    assert "ssw_labelprop_round_batch" in declared and "ssw_labelprop_batch_error" in declared
    from seesaw_amd.label_propagation import LabelPropagation
    from seesaw_amd.loops.graph_based import KnnProp2
    from seesaw_amd.research.knn_methods import LabelPropagationRanker2
    assert isinstance(LabelPropagation.__dict__["round_batch"], staticmethod)
    assert isinstance(LabelPropagationRanker2.__dict__["update_and_select_batch"], staticmethod)
    assert isinstance(KnnProp2.__dict__["refine_batch"], classmethod)


def test_round_batch_packs_per_slot_lists_with_offsets():
    from seesaw_amd.label_propagation import LabelPropagation
    ids = [[5, 9, 2], [], np.array([7], dtype=np.int32), [1, 1]]
    vals = [[1.0, 0.0, 1.0], [], [0.5], [0.0, 1.0]]
    excluded = [None, [3, 4], np.zeros(0, dtype=np.int64), [8]]
    p_ids, p_vals, off, p_ex, ex_off = LabelPropagation.pack_round_batch(ids, vals, excluded)
    assert p_ids.dtype == np.int64 and p_vals.dtype == np.float64 and p_ex.dtype == np.int64
    assert off.dtype == np.int64 and ex_off.dtype == np.int64
    assert all(a.flags.c_contiguous for a in (p_ids, p_vals, off, p_ex, ex_off))
    assert off.tolist() == [0, 3, 3, 4, 6] and ex_off.tolist() == [0, 0, 2, 2, 3]
    assert p_ids.tolist() == [5, 9, 2, 7, 1, 1]          # each slot's ids in the order given (the library sorts them)
    assert p_vals.tolist() == [1.0, 0.0, 1.0, 0.5, 0.0, 1.0]
    assert p_ex.tolist() == [3, 4, 8]
    for j in range(4):                                   # slot j owns [off[j], off[j + 1]) of the packed arrays
        assert p_ids[off[j]:off[j + 1]].tolist() == list(np.asarray(ids[j], dtype=np.int64))
        want = [] if excluded[j] is None else list(np.asarray(excluded[j], dtype=np.int64))
        assert p_ex[ex_off[j]:ex_off[j + 1]].tolist() == want
    # nothing labelled and nobody excluded anywhere: empty arrays of the right types, offsets all zero
    p_ids, p_vals, off, p_ex, ex_off = LabelPropagation.pack_round_batch([[], []], [[], []], [None, None])
    assert p_ids.shape == p_vals.shape == p_ex.shape == (0,) and p_ids.dtype == np.int64 and p_vals.dtype == np.float64
    assert off.tolist() == [0, 0, 0] and ex_off.tolist() == [0, 0, 0]
    with pytest.raises(AssertionError):
        LabelPropagation.pack_round_batch([[1, 2]], [[1.0]], [None])       # ids and values of a slot must pair up
    with pytest.raises(AssertionError):
        LabelPropagation.pack_round_batch([[1]], [[1.0]], [None, None])    # one entry a slot in every list


# ---- SessionGroup's grouping of graph loops, on stubs -----------------------------------------------------------------
def _index(view=False, dev=True, batch=True):
    ix = types.SimpleNamespace(_dev=types.SimpleNamespace(is_view=view) if dev else None)
    if batch:
        ix.topk_after_update_batch = lambda *a, **k: []
    return ix


def _session(loop_cls, index, *, started=True, shortlist_size=50, fuse=True, log=None, name=None):
    params = types.SimpleNamespace(batch_size=3, shortlist_size=shortlist_size, agg_method="plain_score", aug_larger="greater")
    loop = object.__new__(loop_cls)
    loop.params, loop.started = params, started
    loop.q = types.SimpleNamespace(index=index, returned=set())
    loop.curr_qvec = np.ones(4, np.float32)
    loop.state = types.SimpleNamespace(knn_model=types.SimpleNamespace(can_fuse_round=lambda: fuse))
    loop._engine = types.SimpleNamespace(dim=512, device=0)
    s = types.SimpleNamespace(loop=loop, params=params, q=loop.q)
    if log is not None:
        s._log = lambda msg: log.append((name, msg))
        s.refine = lambda: log.append((name, "own refine"))
    return s


def test_propagation_groups_on_stub_loops(monkeypatch):
    from seesaw_amd.loops.graph_based import KnnProp2
    from seesaw_amd.loops.multi_reg import MultiReg
    from seesaw_amd.loops.point_based import Plain
    from seesaw_amd.seesaw_session import SessionGroup

    class OwnRefine(KnnProp2):
        def refine(self, change=None):
            pass

    class OwnGate(KnnProp2):
        def refine_external(self, change=None):
            pass

    monkeypatch.delenv("SSW_NO_FUSED_ROUND", raising=False)
    a, b, view, host = _index(), _index(), _index(view=True), _index(dev=False)
    sessions = [
        _session(KnnProp2, a),                          # 0
        _session(Plain, a),                             # 1: not a graph loop
        _session(KnnProp2, a),                          # 2: with 0
        _session(OwnRefine, a),                         # 3: a subclass with its own refine stays alone
        _session(OwnGate, a),                           # 4: ... or its own start gate
        _session(KnnProp2, a, started=False),           # 5: start policy not fired
        _session(KnnProp2, a, shortlist_size=40),       # 6: another shortlist: a group of one
        _session(KnnProp2, b),                          # 7: another index object
        _session(KnnProp2, view),                       # 8: a view index stays alone
        _session(KnnProp2, host),                       # 9: rows not on the device
        _session(KnnProp2, a, fuse=False),              # 10: the model cannot fuse the round
        _session(KnnProp2, b),                          # 11: with 7
        _session(MultiReg, a),                          # 12
        _session(KnnProp2, _index(batch=False)),        # 13: an index without the batched entry
    ]
    g = SessionGroup(sessions)
    assert g.propagation_groups() == [(0, 2), (6,), (7, 11)]
    # the other groupings do not see any of this: as far as fit_groups goes a started graph loop refines alone, and
    # neither it nor query_groups changes with the switch that empties the propagation groups
    fits, queries = g.fit_groups(), g.query_groups()
    assert fits == ([(12,)], [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 13])
    assert all((i,) in queries for i in (0, 2, 3, 4, 6, 7, 8, 9, 10, 11, 13))  # a started graph loop answers on its own
    monkeypatch.setenv("SSW_NO_FUSED_ROUND", "1")
    assert g.propagation_groups() == []
    assert (g.fit_groups(), g.query_groups()) == (fits, queries)
    assert SessionGroup.MIN_PROPAGATION_GROUP >= 2


def test_refine_batches_groups_of_two_and_leaves_single_loops_alone(monkeypatch):
    from seesaw_amd.loops.graph_based import KnnProp2
    from seesaw_amd.seesaw_session import SessionGroup
    monkeypatch.delenv("SSW_NO_FUSED_ROUND", raising=False)
    monkeypatch.setattr(SessionGroup, "MIN_PROPAGATION_GROUP", 2)
    log, batches = [], []
    monkeypatch.setattr(KnnProp2, "refine_batch", classmethod(lambda cls, loops: batches.append(list(loops))))
    a, b = _index(), _index()
    sessions = [_session(KnnProp2, a, log=log, name=0), _session(KnnProp2, b, log=log, name=1),
                _session(KnnProp2, a, log=log, name=2), _session(KnnProp2, a, started=False, log=log, name=3)]
    sessions[3].loop._start_condition = lambda: False
    g = SessionGroup(sessions)
    assert g.propagation_groups() == [(0, 2), (1,)]
    g.refine()
    assert batches == [[sessions[0].loop, sessions[2].loop]]
    # the batch's members get the session's log entries around the one call; the group of one and the loop that has not
    # started go through their own refine(), in session order
    assert log == [(0, "refine.start"), (2, "refine.start"), (0, "refine.end"), (2, "refine.end"), (1, "own refine"),
                   (3, "own refine")]
    # the start gate of refine_external is applied to graph loops too: a loop whose condition fires joins this very round
    log.clear(), batches.clear()
    sessions[3].loop._start_condition = lambda: True
    g.refine()
    assert sessions[3].loop.started is True
    assert batches == [[sessions[0].loop, sessions[2].loop, sessions[3].loop]]
    assert (1, "own refine") in log and (3, "own refine") not in log
    # a larger minimum size leaves smaller groups to their own refine()
    log.clear(), batches.clear()
    monkeypatch.setattr(SessionGroup, "MIN_PROPAGATION_GROUP", 4)
    g.refine()
    assert batches == [] and [e for e in log if e[1] == "own refine"] == [(i, "own refine") for i in range(4)]

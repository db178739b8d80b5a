"""CPU: the host side of the batched two-vector query -- the plain finishing helper against rescore_candidates, the
`vectors2` keyword of the default / coarse `query_batch`, SessionGroup's grouping of started multi_reg_neg loops on stubs,
and the entry's declaration (include/seesaw_hip.h) and binding (seesaw_amd/_lib.py)."""
import re
import types

import numpy as np
import pandas as pd
import pytest


# ---- plain_pair_result against rescore_candidates' plain_score branch -------------------------------------------------
def _frames(rng, n_images, special):
    """candidate frames in ascending dbidx order with f32 tile scores drawn from a handful of values (ties within and
    across images), NaN and -inf mixed in; `special`: also an all-NaN image, an all -inf one and a single-tile one"""
    counts = rng.integers(1, 9, n_images)
    if special:
        counts[1] = 1
    dbidx = np.sort(rng.choice(1000, n_images, replace=False))
    row_dbidx = np.repeat(dbidx, counts)
    n = int(counts.sum())
    score = rng.choice(np.float32([-2.0, -0.5, 0.0, 0.25, 0.25, 1.5, 3.0]), n).astype(np.float32)
    score[rng.random(n) < 0.15] = np.nan
    score[rng.random(n) < 0.10] = -np.inf
    row_start = np.concatenate(([0], np.cumsum(counts)))
    if special:
        score[row_start[0]:row_start[1]] = np.nan
        score[row_start[2]:row_start[3]] = -np.inf
    box = rng.integers(0, 500, (n, 4)).astype(np.float32)
    meta = pd.DataFrame({"dbidx": row_dbidx, "zoom_level": rng.integers(0, 3, n).astype(np.int16), "x1": box[:, 0],
                         "y1": box[:, 1], "x2": box[:, 2], "y2": box[:, 3]})
    return meta, score, row_start


def _per_image(score, row_start):
    """what the device stage hands over: per image the highest non-NaN score (NaN: none) and its first tile's row"""
    s, r = [], []
    for a, b in zip(row_start[:-1], row_start[1:]):
        seg = score[a:b]
        if np.isnan(seg).all():
            s.append(np.float32(np.nan)), r.append(a)
        else:
            i = int(np.nanargmax(seg))
            s.append(seg[i]), r.append(a + i)
    return np.asarray(s, dtype=np.float32), np.asarray(r, dtype=np.int64)


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("topk", [1, 4, 50])
def test_plain_helper_is_the_plain_branch_of_rescore_candidates(seed, topk):
    from seesaw_amd.indices.multiscale.multiscale_index import plain_pair_result, rescore_candidates
    rng = np.random.default_rng(seed)
    # an index of 3 x the candidates: the candidates are every third image, so index rows and fullmeta rows differ
    meta_all, score_all, row_start_all = _frames(rng, 36, special=False)
    positions = np.arange(1, 36, 3)
    rows = np.concatenate([np.arange(row_start_all[p], row_start_all[p + 1]) for p in positions])
    score = score_all[rows].copy()
    tiles = row_start_all[positions + 1] - row_start_all[positions]
    cand_start = np.concatenate(([0], np.cumsum(tiles)))
    if seed % 2:  # the special images among the candidates
        score[cand_start[0]:cand_start[1]] = np.nan
        score[cand_start[2]:cand_start[3]] = -np.inf
    fullmeta = meta_all.iloc[rows].assign(score=score)
    want = rescore_candidates(fullmeta, topk, agg_method="plain_score")
    s, r = _per_image(score, cand_start)
    index_rows = rows[r]  # rows of the index, as the device returns them
    got = plain_pair_result(meta_all, row_start_all, positions, s, index_rows, topk)
    assert np.array_equal(got["dbidxs"], want["dbidxs"]) and got["dbidxs"].dtype == want["dbidxs"].dtype
    assert len(got["activations"]) == len(want["activations"]) == min(topk, positions.shape[0])
    for fg, fw in zip(got["activations"], want["activations"]):
        pd.testing.assert_frame_equal(fg, fw, check_exact=True)
        assert fg.score.dtype == np.float32


# ---- query_batch(vectors2=...) on the default and the coarse index -----------------------------------------------------
def test_default_query_batch_loops_query_with_the_right_keywords():
    from seesaw_amd.indices.interface import AccessMethod

    class Recorder(AccessMethod):
        def __init__(self):
            self.calls = []

        def query(self, **kw):
            self.calls.append(kw)
            return len(self.calls)

    idx = Recorder()
    v, w = [np.ones(4), np.zeros(4), None], [np.full(4, 2.0), None, np.full(4, 3.0)]
    ex = [None, {1, 2}, None]
    assert idx.query_batch(topk=5, vectors=v, excludes=ex, vectors2=w, shortlist_size=9, agg_method="avg_score") == [1, 2, 3]
    assert [sorted(c) for c in idx.calls] == [
        ["agg_method", "exclude", "shortlist_size", "topk", "vector", "vector2"],
        ["agg_method", "exclude", "shortlist_size", "topk", "vector"],  # None: the keyword is not passed at all
        ["agg_method", "exclude", "shortlist_size", "topk", "vector", "vector2"]]
    assert idx.calls[0]["vector2"] is w[0] and idx.calls[2]["vector2"] is w[2] and idx.calls[2]["vector"] is None
    assert idx.calls[1]["exclude"] is ex[1] and all(c["topk"] == 5 and c["shortlist_size"] == 9 for c in idx.calls)
    idx.calls.clear()
    idx.query_batch(topk=5, vectors=v[:2], vector2=w[0])  # the single keyword keeps its meaning: every entry
    assert all(c["vector2"] is w[0] for c in idx.calls) and len(idx.calls) == 2
    idx.calls.clear()
    idx.query_batch(topk=5, vectors=v[:2], vectors2=None)
    assert all("vector2" not in c for c in idx.calls)
    with pytest.raises(ValueError):
        idx.query_batch(topk=5, vectors=v, vectors2=w[:2])


def test_coarse_index_drops_vectors2():
    """its `query` ignores `vector2`; on a view `query_batch` is the loop of `query`, which shows what it passes on"""
    from seesaw_amd.indices.coarse.coarse_index import CoarseIndex
    calls = []
    stub = types.SimpleNamespace(_dev=types.SimpleNamespace(is_view=True),
                                 query=lambda **kw: calls.append(kw) or {"dbidxs": np.zeros(0, dtype=int)})
    v = [np.ones(4), np.zeros(4)]
    out = CoarseIndex.query_batch(stub, topk=3, vectors=v, vectors2=[np.ones(4), None], shortlist_size=7)
    assert len(out) == 2 and [sorted(c) for c in calls] == [["exclude", "shortlist_size", "topk", "vector"]] * 2


# ---- SessionGroup's grouping with started multi_reg_neg loops, on stubs ------------------------------------------------
def _stub_session(loop_cls, index, *, started, confusion=None, discount_neg=True, constructed=True, **params):
    p = types.SimpleNamespace(**dict(dict(batch_size=3, shortlist_size=50, agg_method="plain_score", aug_larger="greater"),
                                     **params))
    loop = object.__new__(loop_cls)
    loop.params, loop.started = p, started
    loop.q = types.SimpleNamespace(index=index, returned=set())
    loop.curr_qvec = np.ones(4, np.float32)
    loop.curr_vec = np.full(4, 2.0, np.float32)
    loop._engine = types.SimpleNamespace(dim=4, device=0)
    if constructed:
        loop.options = dict(discount_neg=discount_neg)
        loop.confusion_vec = confusion
    return types.SimpleNamespace(loop=loop, params=p, q=loop.q)


def test_started_multi_reg_neg_loops_join_the_query_group():
    from seesaw_amd.loops.multi_reg import MultiReg
    from seesaw_amd.loops.multi_reg_neg import MultiRegNeg
    from seesaw_amd.loops.point_based import Plain
    from seesaw_amd.seesaw_session import SessionGroup

    class Own(MultiRegNeg):
        def next_batch(self):
            return None

    class OwnExternal(MultiRegNeg):
        def next_batch_external(self):
            return None

    a = types.SimpleNamespace(vectors=np.zeros((2, 4), dtype=np.float32))
    b = types.SimpleNamespace(vectors=np.zeros((2, 4), dtype=np.float32))
    conf = np.full(4, 7.0, np.float32)
    sessions = [
        _stub_session(MultiReg, a, started=True),                                 # 0
        _stub_session(MultiRegNeg, a, started=True, confusion=conf),              # 1: with 0, vector2 = confusion_vec
        _stub_session(MultiRegNeg, a, started=True, confusion=conf, discount_neg=False),  # 2: with 0, vector2 = zeros
        _stub_session(MultiRegNeg, a, started=False, confusion=conf),             # 3: not started: the text vector alone
        _stub_session(Own, a, started=True, confusion=conf),                      # 4: its own next_batch
        _stub_session(OwnExternal, a, started=True, confusion=conf),              # 5: its own next_batch_external
        _stub_session(MultiRegNeg, b, started=True, confusion=conf),              # 6: another index object
        _stub_session(MultiRegNeg, a, started=True, confusion=conf, agg_method="avg_score"),  # 7: other parameters
        _stub_session(Plain, a, started=True),                                    # 8: with 0
        _stub_session(MultiRegNeg, a, started=True, confusion=None),              # 9: with 0; no confusion vector yet
        _stub_session(MultiRegNeg, a, started=True, constructed=False),           # 10: made without its constructor
    ]
    g = SessionGroup(sessions)
    assert g.query_groups() == [(0, 1, 2, 3, 8, 9), (4,), (5,), (6,), (7,), (10,)]
    vec, vec2 = SessionGroup.batch_vector, SessionGroup.batch_vector2
    for i in (1, 2, 6, 7, 9):
        assert vec(sessions[i].loop) is sessions[i].loop.curr_vec
    assert vec(sessions[3].loop) is sessions[3].loop.curr_qvec
    assert vec(sessions[4].loop) is None and vec(sessions[5].loop) is None and vec(sessions[10].loop) is None
    assert vec2(sessions[1].loop) is conf and vec2(sessions[6].loop) is conf
    assert np.array_equal(vec2(sessions[2].loop), np.zeros(4)) and vec2(sessions[2].loop).shape == (4,)
    for i in (0, 3, 4, 5, 8, 9, 10):
        assert vec2(sessions[i].loop) is None, i
    # fit_groups does not look at any of this
    assert g.fit_groups() == ([(0,)], [1, 2, 3, 4, 5, 6, 7, 8, 9, 10])


def test_group_next_hands_both_vector_lists_to_query_batch():
    from seesaw_amd.loops.multi_reg_neg import MultiRegNeg
    from seesaw_amd.loops.point_based import Plain
    from seesaw_amd.seesaw_session import SessionGroup
    seen = {}

    def query_batch(**kw):
        seen.update(kw)
        return [{"dbidxs": np.array([10 * i + 1, 10 * i + 2]), "activations": None} for i in range(len(kw["vectors"]))]

    index = types.SimpleNamespace(vectors=np.zeros((2, 4), dtype=np.float32), query_batch=query_batch)
    conf = np.full(4, 7.0, np.float32)
    sessions = [_stub_session(Plain, index, started=True), _stub_session(MultiRegNeg, index, started=True, confusion=conf),
                _stub_session(MultiRegNeg, index, started=True, confusion=conf, discount_neg=False)]
    for s in sessions:
        s._log, s.timing, s.acc_indices, s.acc_activations = (lambda msg: None), [], [], []
        s.loop.q.returned = types.SimpleNamespace(update=lambda ids, s=s: s.acc_indices.append(("returned", list(ids))))
    out = SessionGroup(sessions).next()
    assert [o.tolist() for o in out] == [[1, 2], [11, 12], [21, 22]]
    assert seen["vectors2"][0] is None and seen["vectors2"][1] is conf and np.array_equal(seen["vectors2"][2], np.zeros(4))
    assert all(v is s.loop.curr_vec for v, s in zip(seen["vectors"], sessions)) and seen["topk"] == 3
    # a group without two-vector loops calls query_batch as before: no `vectors2` keyword at all
    seen.clear()
    plain = [sessions[0], _stub_session(Plain, index, started=False)]
    plain[1]._log, plain[1].timing, plain[1].acc_indices, plain[1].acc_activations = (lambda msg: None), [], [], []
    plain[1].loop.q.returned = types.SimpleNamespace(update=lambda ids: None)
    SessionGroup(plain).next()
    assert "vectors2" not in seen and len(seen["vectors"]) == 2


# ---- the entry's declaration and binding ---------------------------------------------------------------------------------
def test_header_and_ctypes_table_list_the_entry():
    from seesaw_amd import _lib
    name = "ssw_index_stage2_pair_batch"
    assert name in _lib.declared_symbols() and name in _lib._SIGNATURES
    text = open(_lib.HEADER_PATH).read()
    decl = re.search(r"ssw_status " + name + r"\((.*?)\);", text, re.S).group(1)
    args = [a.strip() for a in decl.split(",")]
    assert len(args) == 11 == len(_lib._SIGNATURES[name][1])
    assert [a.split()[-1].lstrip("*") for a in args] == ["idx", "q_host", "q2_host", "nq", "image_positions_host",
                                                         "counts_host", "k", "agg", "aug_larger", "out_scores", "out_best_rows"]
    comment = text[:text.index("ssw_status " + name)]
    comment = comment[comment.rindex("/*"):]
    assert "multiscale_index.py:341-352" in comment and "vector2" in comment and "view" in comment
    assert re.search(r"#define SSW_AGG_PLAIN 0\b", text) and re.search(r"#define SSW_AGG_AVG 1\b", text)
    from seesaw_amd.device_index import DeviceIndex
    assert (DeviceIndex.AGG_PLAIN, DeviceIndex.AGG_AVG) == (0, 1)
    lib = _lib.load()
    assert hasattr(lib, name)

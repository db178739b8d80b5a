"""CPU: the crafted cases of test_chunk_select_edges_gpu.py have the structure that file relies on.  `plan` -- the chunk
form's documented rule restated in numpy (tests/_chunk_select_helpers.py) -- is run on every case's scores, so the
counters the GPU file expects (second_level, deep_reruns, per_slot) follow from the inputs and the rule, not from the
code under test; and `_reference` alone returns the ids each construction implies."""
import numpy as np
import pytest

from tests import _chunk_select_helpers as H


def _ids(c, mapped=False):
    v = c.values()
    if mapped:
        rows, row_start = H.map_rows(v)
        ids, scores, best_rows = H._reference(rows, row_start, c.excluded, c.k)
        counts = np.diff(row_start)[ids]
        assert np.array_equal(best_rows, row_start[ids] + counts // 2), "the lowest row of the repeated maximum"
        assert np.array_equal(scores.view(np.uint32), v[ids].view(np.uint32))
        return ids
    return H._reference(v, np.arange(v.shape[0] + 1), c.excluded, c.k)[0]


def test_key_restatement():
    """ord_key is monotone over the floats the cases use, and the two bins are its top 12 and next 12 bits"""
    s = np.array([-np.inf, -2.0, -1.0, -1e-40, 0.0, 1e-45, 1e-40, 0.875, np.nextafter(np.float32(1), np.float32(0)), 1.0, 2.0],
                 dtype=np.float32)
    key = H.ord_key(s).astype(np.int64)
    assert (np.diff(key) > 0).all() and key[0] == 0x007fffff and key[4] == 0x80000000
    assert H.bin1(s)[9] == H.B_ONE and H.bin2(s)[9] == 0 and H.bin1(s)[8] == H.B_ONE - 1 and H.bin2(s)[8] == 0xfff
    assert (H.key_value(H.bin1(s[5:]), H.bin2(s[5:]), H.ord_key(s[5:]) & 0xff).view(np.uint32) == s[5:].view(np.uint32)).all()
    assert H.fillers(H.POOL).max() < 0.125 and np.unique(H.fillers(H.POOL)).shape[0] == H.POOL
    assert (H.fillers(H.POOL).astype(np.float16).astype(np.float32) == H.fillers(H.POOL)).all()


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("mapped", [False, True])
def test_tight_rank(half, mapped):
    for c in H.tight_rank_cases(half, n=8200 if mapped else None):
        v, p = c.values(), H.plan(c.values(), c.excluded, c.k)
        if half:
            assert (v.astype(np.float16).astype(np.float32) == v).all(), c
        ex = np.asarray(c.excluded)
        rest = np.setdiff1d(np.arange(c.n), ex)
        assert ex.shape[0] == c.facts["n_excl"] == np.unique(ex).shape[0] and v[ex].min() > v[rest].max(), c
        assert p["kk"] == c.k + c.facts["n_excl"] and H.route(c.n, c.excluded, c.k) == "general", c
        order = H.best_ids(v, p["kk"] + 1)
        last, following = v[order[-2]], v[order[-1]]
        assert H.bin1(last) == p["b1"] and last > following, c
        if c.facts["edge"] == "first":  # rank kk - 1 is the last key of the bin above
            assert H.bin1(v[order[-3]]) == p["b1"] + 1 and H.ord_key(v[order[-3]]) & 0xfffff == 0 and H.bin1(following) == p["b1"], c
        elif c.facts["edge"]:  # rank kk is the last key of its bin, the bin's edge; rank kk + 1 the first of the next one
            assert p["at_or_above1"] == p["kk"] and H.ord_key(last) & 0xfffff == 0 and H.bin1(following) == p["b1"] - 1, c
        else:
            assert p["at_or_above1"] > p["kk"] and H.bin1(following) == p["b1"], c
        assert np.array_equal(_ids(c, mapped), c.facts["want"]), c


def test_exclusion_cap():
    cases = H.excl_cap_cases()
    assert sorted((c.k, len(set(c.excluded)), len(c.excluded)) for c in cases) == [
        (64, 4032, 4032), (64, 4032, 4082), (64, 4033, 4033), (4095, 1, 1), (4095, 1, 51), (4095, 2, 2), (4096, 0, 0), (4096, 1, 1)]
    for c in cases:
        assert H.route(c.n, c.excluded, c.k) == c.facts["form"], c
        assert H.predict([c.slot()])["per_slot"] == (c.facts["form"] == "per_slot"), c
        ids = _ids(c)
        first = len(set(c.excluded))
        assert np.array_equal(ids, H.best_ids(c.values(), first + c.k)[first:]), c  # the excluded are the best ones


@pytest.mark.parametrize("half", [False, True])
def test_level2_threshold(half):
    for c in H.level2_cases(half):
        p = H.plan(*c.slot())
        assert p["b1"] == H.B_ONE and p["at_or_above1"] == c.facts["total"] and p["level2"] == (c.facts["total"] == 1025), c
        assert not p["overflow"] and len(c.excluded) in (0, 10), c
        assert (H.bin1(c.values()[c.excluded]) == H.B_ONE).all(), c
        assert np.array_equal(_ids(c), [i for i in H.best_ids(c.values(), 74) if i not in set(c.excluded)][:64]), c


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("mapped", [False, True])
def test_final_capacity(half, mapped):
    cases = H.final_cap_cases(half, n=8201 if mapped else None)
    assert [c.facts["total"] for c in cases] == [8192] * 3 + [8193] * 3 + [None]
    for c in cases:
        v, p = c.values(), H.plan(*c.slot())
        if c.facts["total"] is None:
            assert not p["level2"] and not p["overflow"], c
            continue
        group = np.nonzero(v == np.float32(1.0))[0]
        assert p["level2"] and p["b1"] == H.B_ONE and p["b2"] == 0 and p["total2"] == c.facts["total"], c
        assert p["overflow"] == (c.facts["total"] == 8193) and c.n > 8192, c
        assert c.excluded == group[:len(c.excluded)].tolist() and len(c.excluded) in (0, 5), c
        higher = c.facts["total"] - group.shape[0]
        assert higher in (0, 100) and (v > 1.0).sum() == higher, c
        ids = _ids(c, mapped)
        assert np.array_equal(ids[higher:], group[len(c.excluded):][:c.k - higher]) and (v[ids[:higher]] > 1.0).all(), c


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("mapped", [False, True])
def test_ties_across_the_cut(half, mapped):
    cases = H.tie_cases(half, n=8200 if mapped else None)
    assert [(c.facts["higher"], c.facts["level2"]) for c in cases] == [(34, False), (34, True), (40, False), (40, True)]
    for c in cases:
        v, p, higher = c.values(), H.plan(*c.slot()), c.facts["higher"]
        group = np.nonzero(v == c.facts["tie"])[0]
        left = np.setdiff1d(group, c.excluded)
        assert group.shape[0] == 40 and c.excluded == group[::3].tolist() and left.shape[0] == 26, c
        assert (v > c.facts["tie"]).sum() == higher and higher < c.k < higher + 40, "the group straddles raw rank k"
        if higher == 34:
            assert c.k - higher == 30, "30 of the group above the cut"
        else:
            assert 0 < c.k - higher < left.shape[0], "the group straddles rank k among the images that count"
        # (behind 34 higher scores rank k + n_excl = 78 lies past the group's 74: the pick takes the lower scores beside
        # the group where there are any, else a bin of the fillers)
        assert (p["b1"] == H.B_ONE) == (higher == 40 or c.facts["level2"]) and p["level2"] == c.facts["level2"] and not p["overflow"], c
        ids = _ids(c, mapped)
        taken = min(26, c.k - higher)
        assert np.array_equal(ids, c.facts["want"]) and np.array_equal(ids[higher:higher + taken], left[:taken]), c
        assert (v[ids[higher + taken:]] < c.facts["tie"]).all(), c


def test_key_edges_tails_and_small_form():
    negative, zero, subnormal, powers = H.key_edge_cases()
    assert negative.values().max() < 0 and negative.n == 8193
    v = zero.values()
    ids = _ids(zero)
    assert (v > 0).sum() == 40 and (v == 0).sum() == 1 and not np.signbit(v[v == 0]).any() and v[ids[40]] == 0 and v[ids[49]] < 0
    v = subnormal.values()
    tiny = np.float32(np.finfo(np.float32).tiny)
    assert ((v > 0) & (v < tiny)).sum() == 8165 and np.unique(v).shape[0] == v.shape[0] and (v[_ids(subnormal)] < tiny).sum() == 20
    v = powers.values()
    assert all((v == np.float32(2.0) ** -j).sum() >= 1 and (H.ord_key(v) == H.ord_key(np.float32(2.0) ** -j) - 1).sum() == 1
               for j in range(7))
    for c in (negative, zero, subnormal, powers):
        assert H.route(c.n, c.excluded, c.k) == "general" and c.k == 50, c
    for c in H.tail_cases():
        order = H.best_ids(c.values(), 64)
        assert c.n in (8193, 8194, 8195, 8196) and (order[0], order[63], order[62]) == (c.n - 1, c.n - 2, c.n - 3), c
        assert np.array_equal(_ids(c), order)
    small = H.small_cases()
    assert [H.route(c.n, c.excluded, c.k) for c in small] == ["small"] * 3
    assert [(c.n, len(c.excluded), len(set(c.excluded))) for c in small] == [(64, 64, 64), (8192, 8192, 8189), (1000, 0, 0)]
    assert [_ids(c).shape[0] for c in small] == [c.facts["count"] for c in small] == [0, 3, 64]
    assert H.predict([c.slot() for c in small]) == dict(chunks=1, slots=3, second_level=0, per_slot=0, deep_reruns=0, launches=1)


def test_sequence_kinds():
    calls = H.sequence_calls()
    assert [len(cases) for _, cases in calls] == [2, 2, 2, 2, 16, 3, 2]
    for what, cases in calls:
        assert len(set(c.k for c in cases)) == 1, what
        for c in cases:
            p, kind = H.plan(*c.slot()), c.facts["kind"]
            assert H.route(c.n, c.excluded, c.k) == ("per_slot" if kind == "per_slot" else "general"), c
            if kind != "per_slot":
                assert (p["level2"], p["overflow"]) == dict(plain=(False, False), level2=(True, False), overflow=(True, True))[kind], c
    d = H.predict([c.slot() for c in calls[5][1]])
    assert d == dict(chunks=1, slots=2, second_level=2, per_slot=1, deep_reruns=1, launches=4), d


def test_fewer_than_k_finite():
    """-inf is a key of its own, below every finite score: the 30 finite images come first, then the 20 lowest-numbered
    masked ones; every image lies at or above the picked 24-bit prefix, so the slot reruns deep"""
    c = H.masked_case()
    v, p = c.values(), H.plan(*c.slot())
    assert np.isfinite(v).sum() == 30 and c.n == 8200 and H.route(c.n, c.excluded, c.k) == "general"
    assert (H.ord_key(v[c.facts["labelled"]]) == 0x007fffff).all() and H.ord_key(v[c.facts["free"]]).min() > 0x80000000
    assert (p["b1"], p["b2"], p["level2"], p["total2"], p["overflow"]) == (0x007, 0xfff, True, 8200, True)
    ids = _ids(c)
    free = c.facts["free"]
    assert np.array_equal(ids[:30], free[np.argsort(-v[free].astype(np.float64), kind="stable")])
    assert np.array_equal(ids[30:], c.facts["labelled"][:20])

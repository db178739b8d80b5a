"""GPU: chunk selection (select.hip k_chunk_*) at its rank, tie and capacity edges, on crafted score slabs
(tests/_chunk_select_helpers.py; test_chunk_select_edges_cpu.py holds the cases to the structure relied on here).
Every slot of every call is held to three things: the call with the setting on equals plain numpy (`_reference`, on the
slab the device returned, which must be the crafted values bit for bit), it equals the call with the setting off byte
for byte, and the change of `chunk_select_stats` is what `predict` -- the documented rule on the scores, not the
library -- says: which slots took the second level, which overflowed into the deep rerun, which went per-slot.

Without an image map a case is a view of one parent of at most 45 001 rows (`_run_views`), with one a column of an index
of 8200 or 8201 images of 1, 8, 9, 16 and 17 rows (`_run_mapped`: `topk_batch` forms chunks from 65 536 rows on)."""
import numpy as np
import pytest

from tests import _chunk_select_helpers as H
from tests._chunk_select_helpers import DIM, _on_off, _reference, _same

pytestmark = pytest.mark.gpu

DTYPES = ["float32", "float16"]


def _unit(column, sign=1.0):
    q = np.zeros(DIM, dtype=np.float32)
    q[column] = sign
    return q


def _check(cases, slabs, starts, off, on, d):
    per_image = []
    for s, c in enumerate(cases):
        want = _reference(slabs[s], starts[s], c.excluded, c.k)
        _same([on[s]], [want], ("reference", c.name))
        if "want" in c.facts:
            assert np.array_equal(on[s][0], c.facts["want"]), c
        if "count" in c.facts:
            assert on[s][0].shape[0] == c.facts["count"], c
        per_image.append(np.maximum.reduceat(slabs[s], starts[s][:-1]))
    _same(on, off, "setting off")
    want = H.predict([(v, c.excluded, c.k) for v, c in zip(per_image, cases)])
    assert d == want, (d, want, cases)


def _run_views(calls, dtype, rounds=1):
    """every call (cases of one k) as one `views_topk_batch` on views of ONE parent without a map: the parent holds
    the fillers' upper half, every distinct block, the fillers' lower half; a case's view is its block between as many
    fillers of either half as it asks for"""
    from seesaw_amd.device_index import DeviceIndex
    cases = [c for call in calls for c in call]
    ahead, behind = max(c.ahead() for c in cases), max(c.behind() for c in cases)
    fill = H.fillers(H.POOL)
    blocks, at, n = {}, {}, ahead
    for c in cases:
        if id(c.top) not in blocks:
            blocks[id(c.top)], at[id(c.top)] = c.top, n
            n += c.top.shape[0]
    column = np.concatenate([fill[:ahead]] + list(blocks.values()) + [fill[H.POOL // 2:H.POOL // 2 + behind]])
    assert column.shape[0] <= 45001
    X = np.zeros((column.shape[0], DIM), dtype=np.float32)
    X[:, 0] = column
    parent = DeviceIndex.from_numpy(X, dtype=dtype)
    views = {}

    def view(c):
        key = (id(c.top), c.n)
        if key not in views:
            views[key] = parent.view(np.concatenate((np.arange(c.ahead()), at[id(c.top)] + np.arange(c.top.shape[0]),
                                                     n + np.arange(c.behind()))))
        return views[key]

    for rnd in range(rounds):
        for call in calls:
            vs, k = [view(c) for c in call], call[0].k
            assert all(c.k == k for c in call)
            Q = np.stack([_unit(0, c.sign) for c in call])
            slabs = [v.view_scores_batch(Q[s:s + 1])[0] for s, v in enumerate(vs)]
            for c, slab in zip(call, slabs):
                assert slab.tobytes() == c.values().tobytes(), ("the slab is not the crafted one", c)
            excluded = [c.excluded for c in call]
            off, on, d = _on_off(parent, lambda: DeviceIndex.views_topk_batch(vs, Q, k, excluded=excluded))
            _check(call, slabs, [np.arange(c.n + 1) for c in call], off, on, d)
    for v in views.values():
        v.close()
    parent.close()


def _run_mapped(calls, dtype):
    """every call as one `topk_batch` on ONE index with an image map: case j is column j, queried with e_j"""
    from seesaw_amd.device_index import DeviceIndex
    n_images = calls[0][0].n
    # the row scan takes chunks of 2, 4, 8 or 16 queries: a call is filled up to ONE chunk with plain slots of its own
    # (a hundred distinct scores above the fillers, no exclusions), which are checked and counted like every other slot
    calls = [call + [H.Case(f"padding {s}", H.ladder(100 + s, H.B_LADDER), n_images, call[0].k)
                     for s in range((1 << (len(call) - 1).bit_length()) - len(call))] for call in calls]
    cases = [c for call in calls for c in call]
    assert all(c.n == n_images and c.sign == 1.0 for c in cases) and len(cases) <= DIM
    columns, row_start = [], None
    for c in cases:
        rows, row_start = H.map_rows(c.values())
        columns.append(rows)
    X = np.zeros((columns[0].shape[0], DIM), dtype=np.float32)
    for j, rows in enumerate(columns):
        X[:, j] = rows
    idx = DeviceIndex.from_numpy(X, row2image=np.repeat(np.arange(n_images, dtype=np.int32), np.diff(row_start)), dtype=dtype)
    assert idx.n_rows >= 65536  # (below, the batch scores one query at a time and forms no chunk)
    column = {id(c): j for j, c in enumerate(cases)}
    for call in calls:
        k = call[0].k
        assert all(c.k == k for c in call) and len(call) in (2, 4, 8, 16)
        Q = np.stack([_unit(column[id(c)]) for c in call])
        slabs = idx.scores_batch(Q)
        for s, c in enumerate(call):
            assert slabs[s].tobytes() == columns[column[id(c)]].tobytes(), ("the slab is not the crafted one", c)
        excluded = [c.excluded for c in call]
        off, on, d = _on_off(idx, lambda: idx.topk_batch(Q, k, excluded=excluded))
        _check(call, slabs, [row_start] * len(call), off, on, d)
    idx.close()


def _by_k(cases):
    return [[c for c in cases if c.k == k] for k in sorted(set(c.k for c in cases))]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mapped", [False, True])
def test_tight_rank(mapped, dtype):
    """excluded = exactly the best n_excl images (1, 100, 4096 - k; k = 1, 64, 65): the k-th survivor has overall rank
    k + n_excl, the rank the pick takes -- mid-bin, and with that rank the last or the first key of its bin"""
    cases = H.tight_rank_cases(dtype == "float16", n=8200 if mapped else None)
    (_run_mapped if mapped else _run_views)(_by_k(cases), dtype)


def test_exclusion_cap():
    """4096 - k distinct ids stay in the chunk form, one more goes per-slot, duplicates do not count: k = 64, 4095, 4096"""
    _run_views(_by_k(H.excl_cap_cases()), "float32")


@pytest.mark.parametrize("dtype", DTYPES)
def test_level2_threshold(dtype):
    """1024 keys at or above the picked bin: level 1 only; 1025: the second level; each also with 10 excluded in the bin"""
    _run_views([H.level2_cases(dtype == "float16")], dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mapped", [False, True])
def test_final_capacity(mapped, dtype):
    """8192 candidates fill the final sort and must not rerun, 8193 must -- one tie group alone, behind 100 higher
    scores, and with its 5 lowest-numbered members excluded; with a map the images tie on their maxima and the rerun
    recomputes them; the last slot of the chunk does not overflow and is unaffected"""
    cases = H.final_cap_cases(dtype == "float16", n=8201 if mapped else None)
    (_run_mapped if mapped else _run_views)([cases], dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mapped", [False, True])
def test_ties_across_the_cut(mapped, dtype):
    """a group of 40 equal scores straddles rank 64 (behind 34 and behind 40 higher scores) with every third member
    excluded: it comes out by ascending image,
    with level 1 only and inside a level-2 bin; with a map the maximum is repeated inside every image, last in its last
    row, and `rows` is the lowest row (images of 1, 8, 9, 16 and 17 rows: the `r += 8` loop's clamp)"""
    cases = H.tie_cases(dtype == "float16", n=8200 if mapped else None)
    (_run_mapped if mapped else _run_views)([cases], dtype)


def test_key_edges():
    """k = 50: all scores negative; the cut below +0.0; subnormals among normals; 2^-j and the float under it"""
    _run_views([H.key_edge_cases()], "float32")


def test_tails():
    """8193, 8194, 8195 and 8196 images in one chunk: the 16-byte loads' leftovers hold the best and the 64th image"""
    _run_views([H.tail_cases()], "float32")


def test_one_handle_many_chunks():
    """one view in every slot, twice over: plain, second level, overflow and deep rerun, plain, 16 slots (the workspace
    grows), one slot past the exclusion cap, plain -- what a kernel leaves behind shows in the call after it"""
    _run_views([cases for _, cases in H.sequence_calls()], "float32", rounds=2)


def test_small_form_nothing_left():
    """one chunk: all 64 images excluded (count 0), all but three of 8192 excluded by 8192 shuffled ids, none excluded"""
    _run_views([H.small_cases()], "float32")


def test_fewer_than_k_finite():
    """the graph round (LabelPropagation.round_batch, the twins of test_graph_round_batch) on 8200 images of one tile:
    session 0 has labelled all but 30 nodes, positively, so the prior ranks and `mask_labeled` leaves 30 finite scores;
    k = 50 takes them and then the 20 lowest-numbered masked images -- -inf is a real key that ties by image id.
    Equal to the per-handle `round` (the twins compare), to numpy on fetch() with the labelled nodes at -inf, and the
    counters to `predict` on those scores -- which says whether the slot reruns deep.  Session 1 is a plain slot."""
    from tests.test_labelprop_round_batch_gpu import _Twins
    rng = np.random.default_rng(23)
    tw = _Twins(rng, H.MASKED_N, 1, 0.03, False, S=2)
    tw.idx_a.chunk_select = True
    labelled, free = H.masked_labels()
    tw.labels[0] = {int(i): 1.0 for i in labelled}
    tw.labels[1] = {int(i): 1.0 for i in free[:5]}
    before = tw.idx_a.chunk_select_stats()
    stats, (prop, ids, vals, exs), got = tw.round(rng, "masked")
    after = tw.idx_a.chunk_select_stats()
    assert prop == [False, False] and stats[3] == 0, (prop, stats)
    slots = []
    for j in range(2):
        scores = tw.a[j].fetch().astype(np.float32)
        scores[ids[j]] = -np.inf
        _same([got[j]], [_reference(scores, np.arange(tw.n + 1), exs[j], 50)], ("numpy on fetch()", j))
        slots.append((scores, exs[j].tolist(), 50))
    images, scores, _ = got[0]
    left = np.setdiff1d(free, exs[0])
    assert images.shape[0] == 50 and np.isfinite(scores).sum() == left.shape[0] and np.isneginf(scores[left.shape[0]:]).all()
    assert np.array_equal(np.sort(images[:left.shape[0]]), left)
    assert np.array_equal(images[left.shape[0]:], np.setdiff1d(labelled, exs[0])[:50 - left.shape[0]])
    d, want = {key: after[key] - before[key] for key in H.STATS}, H.predict(slots)
    assert d == want and H.plan(*slots[0])["overflow"] == bool(want["deep_reruns"]), (d, want)
    tw.close()

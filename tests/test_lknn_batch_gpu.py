"""GPU: several device-resident L-KNN models planning in one call (DeviceLKNNModel.step_batch / top_k_remaining_batch:
ssw_lknn_step_batch / ssw_lknn_top_remaining_batch) against the single calls on the same models, bit for bit, and against
the numpy restatement of tests/_lknn_device_helpers.py; per-slot and whole-call refusals; the order after enqueued answers;
the launch count's independence of the number of slots; and both loops behind SessionGroup against sessions driven alone.

Priors are jittered as the device model's own tests jitter them: 0.1 +- 1e-6."""
import numpy as np
import pytest

from _lknn_device_helpers import Restatement, regular_graph, same_bits

pytestmark = pytest.mark.gpu
INVALID = -1  # SSW_ERR_INVALID


def _prior(n, seed):
    return np.random.default_rng(seed).normal(loc=0.1, scale=1e-6, size=n)


def _model(n, W, gamma):
    from seesaw_amd.loops.LKNN_model import DeviceLKNNModel
    from seesaw_amd.research.active_search.common import Dataset
    return DeviceLKNNModel.from_dataset(Dataset.from_vectors(np.zeros((n, 1))), weight_matrix=W, gamma=gamma)


def _pair(n, D, seed, self_loop_at=None, graph=None):
    """a device model and its restatement on a graph of their own (or on `graph`), prior seeded by `seed`"""
    nbr, W = graph if graph is not None else regular_graph(n, D, seed=seed, self_loop_at=self_loop_at)
    gamma = _prior(n, 1000 + seed)
    return _model(n, W, gamma), Restatement(nbr, gamma)


def _answer(dev, twin, answers, sync=True):
    for i, y in answers:
        twin.condition(int(i), int(y))
    dev.condition_many_([(int(i), int(y)) for i, y in answers])
    if sync:
        dev.state()


def _states(models):
    return [m.state() for m in models]


def _same_states(before, after):
    return all(np.array_equal(b[k], a[k]) if k != "gamma" else same_bits(b[k], a[k]) for b, a in zip(before, after) for k in b)


def _same_entry(a, b):
    """two results of step(..., return_values=True, return_list=True)"""
    return (a[0], a[1]) == (b[0], b[1]) and same_bits(a[2], b[2]) and \
        ((a[3] is None and b[3] is None) or np.array_equal(a[3], b[3]))


def _single(models, Ks, lookaheads):
    return [m.step(K, a, return_values=True, return_list=True) for m, K, a in zip(models, Ks, lookaheads)]


def _batch(models, Ks, lookaheads):
    from seesaw_amd.loops.LKNN_model import DeviceLKNNModel
    return DeviceLKNNModel.step_batch(models, Ks, lookaheads, return_values=True, return_list=True)


def _close(models):
    for m in models:
        m.close()


# ---- 1. single against batch against the restatement ------------------------------------------------------------------
@pytest.fixture(scope="module")
def five():
    """5 models at n = 8193 (four slices and one row), D = 10, in different states: fresh; the three best nodes answered; 23
    answers; node 0 its own neighbour; and one more with answers for the lookahead-1 slot.  K = 1, 4, 8, 128."""
    n, D = 8193, 10
    pairs = [_pair(n, D, seed=s, self_loop_at=0 if s == 3 else None) for s in range(5)]
    _answer(*pairs[1], [(i, t % 2) for t, i in enumerate(pairs[1][1].select(3))])
    rng = np.random.default_rng(5)
    _answer(*pairs[2], [(i, int(rng.random() < 0.3)) for i in rng.choice(n, 23, replace=False)])
    _answer(*pairs[4], [(i, 1) for i in pairs[4][1].select(2)])
    models, twins = [p[0] for p in pairs], [p[1] for p in pairs]
    Ks, lookaheads = [1, 4, 8, 128, 7], [2, 2, 2, 2, 1]
    before = _states(models)
    first = _single(models, Ks, lookaheads)
    together = _batch(models, Ks, lookaheads)
    again = _single(models, Ks, lookaheads)
    out = dict(models=models, twins=twins, Ks=Ks, lookaheads=lookaheads, first=first, together=together, again=again,
               unchanged=_same_states(before, _states(models)))
    yield out
    _close(models)


def test_five_models_in_different_states_single_batch_single(five):
    for j, (a, t, b) in enumerate(zip(five["first"], five["together"], five["again"])):
        assert not isinstance(t, Exception), (j, t)
        assert _same_entry(a, t) and _same_entry(t, b), j
        assert (t[3] is None) == (five["lookaheads"][j] == 1)
    assert five["unchanged"]
    assert len({e[0] for e in five["together"]}) > 1   # the slots did plan on states of their own


@pytest.mark.parametrize("slot", range(5))
def test_five_models_equal_their_restatement(five, oracle, slot):
    twin, K, got = five["twins"][slot], five["Ks"][slot], five["together"][slot]
    if five["lookaheads"][slot] == 1:
        pick, value = twin.step1()
        assert (got[0], got[1]) == (pick, value) and same_bits(got[2], twin.operands()[2]) and got[3] is None
        return
    pick, value, values, top = twin.step(K, oracle)
    assert np.array_equal(got[3], top) and same_bits(got[2], values) and (got[0], got[1]) == (pick, value)


@pytest.fixture(scope="module")
def three_large():
    """S = 3 at n = 67 585 (33 slices and one row: two merge levels), D = 10, K = 8; one graph, three states"""
    n, D, K = 67585, 10, 8
    graph = regular_graph(n, D, seed=67)
    pairs = [_pair(n, D, seed=70 + s, graph=graph) for s in range(3)]
    _answer(*pairs[1], [(i, t % 2) for t, i in enumerate(pairs[1][1].select(3))])
    rng = np.random.default_rng(6)
    _answer(*pairs[2], [(i, int(rng.random() < 0.3)) for i in rng.choice(n, 23, replace=False)])
    models, twins = [p[0] for p in pairs], [p[1] for p in pairs]
    before = _states(models)
    first = _single(models, [K] * 3, [2] * 3)
    together = _batch(models, [K] * 3, [2] * 3)
    again = _single(models, [K] * 3, [2] * 3)
    yield dict(twins=twins, K=K, first=first, together=together, again=again, unchanged=_same_states(before, _states(models)))
    _close(models)


def test_three_models_over_two_merge_levels_single_batch_single(three_large):
    for j, (a, t, b) in enumerate(zip(three_large["first"], three_large["together"], three_large["again"])):
        assert not isinstance(t, Exception), (j, t)
        assert _same_entry(a, t) and _same_entry(t, b), j
    assert three_large["unchanged"]


@pytest.mark.parametrize("slot", range(3))
def test_three_models_over_two_merge_levels_equal_their_restatement(three_large, oracle, slot):
    got = three_large["together"][slot]
    pick, value, values, top = three_large["twins"][slot].step(three_large["K"], oracle)
    assert np.array_equal(got[3], top) and same_bits(got[2], values) and (got[0], got[1]) == (pick, value)


# ---- 2. shape edges ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [8, 128])
@pytest.mark.parametrize("D", [1, 32])
def test_shape_edges_with_exactly_enough_and_one_too_few_unseen_nodes(oracle, D, K):
    """n = L + 1, 255, 257, 1025 (L = K + D): a fresh slot, a slot with exactly L unseen nodes and a slot with L - 1; the
    last is refused ("unseen") on the host, the others equal their single calls and the restatement, no state changes"""
    from seesaw_amd._lib import SeesawHipError
    L = K + D
    for n in sorted({L + 1, 255, 257, 1025}):
        if n < L + 1:
            continue
        graph = regular_graph(n, D, seed=200 + n, self_loop_at=0)
        pairs = [_pair(n, D, seed=s, graph=graph) for s in range(3)]
        rng = np.random.default_rng(n)
        for (dev, twin), left in zip(pairs[1:], (L, L - 1)):
            _answer(dev, twin, [(i, t % 2) for t, i in enumerate(rng.choice(n, n - left, replace=False))])
        models = [p[0] for p in pairs]
        before = _states(models)
        single = _single(models[:2], [K, K], [2, 2])
        with pytest.raises(SeesawHipError) as err:
            models[2].step(K, 2)
        got = _batch(models, [K] * 3, [2] * 3)
        assert isinstance(got[2], SeesawHipError) and got[2].status == INVALID and "unseen" in str(got[2]), (n, got[2])
        assert str(got[2]) == str(err.value)
        for j in range(2):
            assert _same_entry(single[j], got[j]), (n, j)
            pick, value, values, top = pairs[j][1].step(K, oracle)
            assert np.array_equal(got[j][3], top) and same_bits(got[j][2], values) and (got[j][0], got[j][1]) == (pick, value), (n, j)
        assert _same_states(before, _states(models)), n
        _close(models)


def test_one_slot_and_more_slots_than_a_chunk_of_sixteen_or_thirty_two():
    """S = 1 equals step; S = 17 and S = 33 equal the loop of single calls (mixed K and lookahead, a refused slot inside)"""
    from seesaw_amd._lib import SeesawHipError
    n, D = 257, 10
    graph = regular_graph(n, D, seed=9)
    pairs = [_pair(n, D, seed=s, graph=graph) for s in range(33)]
    for s, (dev, twin) in enumerate(pairs):
        rng = np.random.default_rng(s)
        _answer(dev, twin, [(i, int(rng.random() < 0.4)) for i in rng.choice(n, s % 7, replace=False)])
    models = [p[0] for p in pairs]
    Ks = [1 + (5 * s) % 128 for s in range(33)]
    lookaheads = [1 if s % 5 == 4 else 2 for s in range(33)]
    lookaheads[11] = 3  # refused
    single = []
    for m, K, a in zip(models, Ks, lookaheads):
        try:
            single.append(m.step(K, a, return_values=True, return_list=True))
        except SeesawHipError as e:
            single.append(e)
    assert isinstance(single[11], SeesawHipError)
    for S in (1, 17, 33):
        got = _batch(models[:S], Ks[:S], lookaheads[:S])
        for j in range(S):
            if isinstance(single[j], Exception):
                assert isinstance(got[j], SeesawHipError) and str(got[j]) == str(single[j]) and got[j].status == INVALID, (S, j)
            else:
                assert _same_entry(single[j], got[j]), (S, j)
    _close(models)


# ---- 3. ties ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tied", [2, 4])
def test_a_slot_with_exact_ties_beside_two_tie_free_slots(oracle, tied):
    """the tied slot is that of the device model's own tie test: `tied` nodes share gamma inside the list, `tied` more
    straddle its last place"""
    n, D, K = 1025, 10, 8
    L = K + D
    nbr, W = regular_graph(n, D, seed=7)
    gamma = _prior(n, 3)
    order = np.argsort(-gamma)
    inside, across = order[3:3 + tied], order[L - tied // 2:L + tied // 2]
    gamma[inside] = gamma[inside[0]]
    gamma[across] = gamma[across[0]]
    tied_pair = (_model(n, W, gamma), Restatement(nbr, gamma))
    assert not tied_pair[1].top_distinct(L)
    pairs = [_pair(n, D, seed=31), tied_pair, _pair(n, D, seed=32)]
    assert pairs[0][1].top_distinct(L) and pairs[2][1].top_distinct(L)
    got = _batch([p[0] for p in pairs], [K] * 3, [2] * 3)
    for j, (_, twin) in enumerate(pairs):
        pick, value, values, top = twin.step(K, oracle)
        assert np.array_equal(got[j][3], top), j
        assert same_bits(got[j][2], values) and (got[j][0], got[j][1]) == (pick, value), j
    _close([p[0] for p in pairs])


# ---- 4. ordering ------------------------------------------------------------------------------------------------------
def test_answers_enqueued_on_every_model_are_seen_by_the_batch(oracle):
    """condition_many_ is enqueue-only, each model on its own stream: the batch that follows at once plans on the state
    after the answers"""
    n, D, K = 1025, 10, 4
    graph = regular_graph(n, D, seed=41)
    pairs = [_pair(n, D, seed=40 + s, graph=graph) for s in range(4)]
    models = [p[0] for p in pairs]
    for s, (dev, twin) in enumerate(pairs):
        rng = np.random.default_rng(s)
        best = [int(i) for i in twin.select(3)]
        more = [int(i) for i in rng.choice(np.setdiff1d(np.arange(n), best), 200, replace=False)]
        _answer(dev, twin, [(i, t % 2) for t, i in enumerate(best + more)], sync=False)
    got = _batch(models, [K] * 4, [2, 2, 1, 2])
    for j, (_, twin) in enumerate(pairs):
        if j == 2:
            assert (got[j][0], got[j][1]) == twin.step1() and same_bits(got[j][2], twin.operands()[2])
            continue
        pick, value, values, top = twin.step(K, oracle)
        assert np.array_equal(got[j][3], top) and same_bits(got[j][2], values) and (got[j][0], got[j][1]) == (pick, value), j
    _close(models)


# ---- 5. top_k_remaining_batch -------------------------------------------------------------------------------------------
def test_top_k_remaining_batch_equals_top_k_remaining():
    from seesaw_amd.loops.LKNN_model import DeviceLKNNModel
    n, D = 257, 10
    graph = regular_graph(n, D, seed=51)
    pairs = [_pair(n, D, seed=50 + s, graph=graph) for s in range(6)]
    models = [p[0] for p in pairs]
    rng = np.random.default_rng(5)
    _answer(*pairs[1], [(i, t % 2) for t, i in enumerate(pairs[1][1].select(3))])
    _answer(*pairs[2], [(i, t % 2) for t, i in enumerate(rng.choice(n, n - 100, replace=False))])   # 100 unseen, k = 150
    _answer(*pairs[3], [(i, t % 2) for t, i in enumerate(rng.permutation(n))])                      # every node answered
    ks = [1, 192, 150, 5, 193, 0]
    before = _states(models)
    single = [m.top_k_remaining(k) for m, k in zip(models[:4], ks)]
    got = DeviceLKNNModel.top_k_remaining_batch(models, ks)
    for j in range(4):
        assert got[j][0].dtype == single[j][0].dtype and np.array_equal(got[j][0], single[j][0]), j
        assert same_bits(got[j][1], single[j][1]), j
        assert np.array_equal(got[j][0], pairs[j][1].select(ks[j])), j
    assert [len(got[j][0]) for j in range(4)] == [1, 192, 100, 0]
    for j in (4, 5):   # what top_k_remaining raises for such a k
        with pytest.raises(ValueError) as err:
            models[j].top_k_remaining(ks[j])
        assert isinstance(got[j], ValueError) and str(got[j]) == str(err.value)
    assert _same_states(before, _states(models))
    # every slot with nothing to list: no launch, no wait, counts 0
    got = DeviceLKNNModel.top_k_remaining_batch([models[3]], [7])
    assert len(got[0][0]) == 0 and models[3].step_info()["launches"] == 0
    _close(models)


def test_top_remaining_slot_refusal_in_the_library():
    """k outside [1, 192] at the C entry: that slot's status and batch error, the other slot served"""
    import ctypes
    from seesaw_amd import _lib
    n, D = 255, 10
    graph = regular_graph(n, D, seed=52)
    (a, ta), (b, _) = _pair(n, D, seed=1, graph=graph), _pair(n, D, seed=2, graph=graph)
    hs = (ctypes.c_void_p * 2)(a._h, b._h)
    ks = np.array([3, 193], dtype=np.int32)
    ids, scores = np.zeros((2, 192), dtype=np.int32), np.zeros((2, 192))
    counts, status = np.zeros(2, dtype=np.int32), np.zeros(2, dtype=np.int32)
    _lib.call("ssw_lknn_top_remaining_batch", hs, 2, *(ctypes.c_void_p(x.ctypes.data) for x in (ks, ids, scores, counts, status)))
    assert status.tolist() == [0, INVALID] and counts.tolist() == [3, 0]
    assert np.array_equal(ids[0, :3], ta.select(3))
    lib = _lib.load()
    assert lib.ssw_lknn_batch_error(a._h) == b"" and b"k=193" in lib.ssw_lknn_batch_error(b._h)
    _close([a, b])


# ---- 6. stats ---------------------------------------------------------------------------------------------------------
def test_launches_do_not_depend_on_the_number_of_slots_and_the_host_waits_once():
    from seesaw_amd.loops.LKNN_model import DeviceLKNNModel
    n, D, K = 8193, 10, 4
    graph = regular_graph(n, D, seed=61)
    models = [_pair(n, D, seed=s, graph=graph)[0] for s in range(16)]
    models[0].step(K, 2)
    alone = models[0].step_info()
    stats = {}
    for S in (2, 16):
        got = DeviceLKNNModel.step_batch(models[:S], [K] * S, [2] * S)
        assert not any(isinstance(e, Exception) for e in got)
        stats[S] = dict(DeviceLKNNModel.last_batch_stats)
        assert stats[S]["host_waits"] == 1 and stats[S]["bytes_to_host"] == 16 * S, stats[S]
        assert stats[S]["bytes_to_device"] > 0
        for m in models[:S]:
            assert m.step_info() == stats[S]
    assert stats[2]["launches"] == stats[16]["launches"]
    # the pass is the single step's kernels and one finish kernel: select, one merge level, mark, look-ahead, unmark, argmax
    assert stats[2]["launches"] == alone["launches"] + 1 == 7
    with_ones = DeviceLKNNModel.step_batch(models[:4], [K] * 4, [2, 1, 2, 1])
    assert not any(isinstance(e, Exception) for e in with_ones)
    assert DeviceLKNNModel.last_batch_stats["launches"] == 8 and DeviceLKNNModel.last_batch_stats["host_waits"] == 1
    DeviceLKNNModel.top_k_remaining_batch(models[:2], [1, 1])
    a = models[0].step_info()
    DeviceLKNNModel.top_k_remaining_batch(models, [1] * 16)
    assert models[0].step_info()["launches"] == a["launches"] == 3 and models[0].step_info()["host_waits"] == 1
    _close(models)


# ---- 7. call-level refusals ---------------------------------------------------------------------------------------------
def test_a_repeated_handle_or_another_node_count_refuses_the_call_and_touches_nothing():
    from seesaw_amd._lib import SeesawHipError
    from seesaw_amd.loops.LKNN_model import DeviceLKNNModel
    K = 4
    a, _ = _pair(1025, 10, seed=71)
    b, _ = _pair(1025, 10, seed=72)
    c, _ = _pair(257, 10, seed=73)      # another n
    d, _ = _pair(1025, 5, seed=74)      # another degree
    models = [a, b, c, d]
    before, first = _states(models), _single(models, [K] * 4, [2] * 4)
    for group, word in [([a, b, a], "repeats"), ([a, c], "differs"), ([a, b, d], "differs")]:
        with pytest.raises(SeesawHipError) as err:
            DeviceLKNNModel.step_batch(group, [K] * len(group), [2] * len(group))
        assert err.value.status == INVALID and word in str(err.value), str(err.value)
        with pytest.raises(SeesawHipError) as err:
            DeviceLKNNModel.top_k_remaining_batch(group, [1] * len(group))
        assert err.value.status == INVALID and word in str(err.value), str(err.value)
    again = _single(models, [K] * 4, [2] * 4)
    assert all(_same_entry(x, y) for x, y in zip(first, again)) and _same_states(before, _states(models))
    _close(models)


# ---- 8. the loops behind SessionGroup -----------------------------------------------------------------------------------
ROUNDS = 12
LP = dict(matrix_options=dict(knn_path="nndescent60", symmetric=False, self_edges=False, normalized_weights=False, knn_k=10,
                              edist=0.05),
          normalize_scores=False, sigmoid_before_propagate=True, calib_a=10.0, calib_b=-0.4, prior_weight=1.0)
ACTIVE = dict(gamma=dict(mode="clip", calibration="sigmoid", a=10.0, b=-0.2), reward_horizon=10, adjust_horizon=False,
              max_steps=100, pruning_on=False, implementation="vectorized", model_on_device=True, **LP)
LKNN = dict(gamma=0.1, use_clip_as_gamma=False, model_on_device=True, **LP)
# (options, text, the category the simulated user accepts).  The dataset of the device model's own loop test has the two
# categories c0 and c1: the members search one or the other and so get different answers; the second active_search
# member's horizon runs 10, 10, 10, 9, ..., 1 -- its last round is the one-step branch beside lookahead-2 members -- and
# the third plans with another reward_horizon
MEMBERS = {
    "lknn": [(LKNN, "a c1", "c1"), (LKNN, "a c0", "c0"), (dict(LKNN, gamma=0.2), "a c1", "c0"), (LKNN, "a c0", "c1")],
    "active_search": [(ACTIVE, "a c1", "c1"), (dict(ACTIVE, adjust_horizon=True, max_steps=12), "a c0", "c0"),
                      (dict(ACTIVE, reward_horizon=5), "a c1", "c1"), (ACTIVE, "a c0", "c1")],
}


@pytest.fixture(scope="module")
def lvis():
    from seesaw_amd.synthetic import GlobalDataManager, make_dataset
    ds = make_dataset("lvis", n_images=1500, tiles_per_image=1, n_categories=2, positive_frac=0.03, seed=4, knn_k=10, signal=0.5)
    return GlobalDataManager().add(ds), ds


def _sessions(gdm, loop):
    from seesaw_amd.basic_types import IndexSpec, SessionParams
    from seesaw_amd.seesaw_session import make_session
    out = []
    for options, text, _ in MEMBERS[loop]:
        p = SessionParams(index_spec=IndexSpec(d_name="lvis", i_name="coarse"), interactive=loop, interactive_options=dict(options),
                          batch_size=1, shortlist_size=50, agg_method="plain_score", aug_larger="greater",
                          start_policy="from_start", index_options={"use_vec_index": False})
        s = make_session(gdm, p)["session"]
        s.set_text(text)
        out.append(s)
    return out


def _label(session, category, ds):
    from seesaw_amd.basic_types import BenchParams
    from seesaw_amd.seesaw_bench import _group_boxes, fill_imdata
    b = BenchParams(name="lvis", ground_truth_category=category, qstr=f"a {category}", n_batches=ROUNDS)
    boxes = ds.box_data.assign(description=ds.box_data.category)
    boxes = boxes[boxes.category == category]
    groups = _group_boxes(boxes)
    session.update_last_batch([fill_imdata(im, boxes, b, _groups=groups) for im in session.last_batch()])


def _drive(gdm, ds, loop, group_cls):
    sessions = _sessions(gdm, loop)
    group = group_cls(sessions) if group_cls is not None else None
    for r in range(ROUNDS):
        if group is not None:
            shown = group.next()
            assert all(np.array_equal(a, s.acc_indices[-1]) for a, s in zip(shown, sessions))
        else:
            for s in sessions:
                s.next()
        for s, (_, _, category) in zip(sessions, MEMBERS[loop]):
            _label(s, category, ds)
        if r + 1 < ROUNDS:
            for s in sessions:
                s.refine()
    out = [dict(acc_indices=[np.asarray(a).tolist() for a in s.acc_indices], returned=np.array(s.q.returned).tolist(),
                pruned_fractions=list(getattr(s.loop, "pruned_fractions", [])), n_timing=len(s.timing),
                log=[e[1:] for e in s._log_raw]) for s in sessions]
    for s in sessions:
        s.loop.prob_model.close()
    return out


@pytest.mark.parametrize("loop", ["lknn", "active_search"])
def test_sessions_planning_together_equal_sessions_driven_alone(lvis, loop, monkeypatch):
    from seesaw_amd.loops.active_search import ActiveSearch, LKNNSearch
    from seesaw_amd.seesaw_session import SessionGroup
    gdm, ds = lvis

    class Routed(SessionGroup):  # (the product's minimum is a measured break-even or None, not a rule of correctness)
        MIN_LKNN_GROUP = 2
        MIN_ACTIVE_SEARCH_GROUP = 2

    cls = LKNNSearch if loop == "lknn" else ActiveSearch
    calls = []
    own = cls.next_batch_group.__func__
    monkeypatch.setattr(cls, "next_batch_group", classmethod(lambda c, loops: (calls.append(len(loops)), own(c, loops))[1]))
    alone = _drive(gdm, ds, loop, None)
    assert calls == []
    together = _drive(gdm, ds, loop, Routed)
    assert calls == [4] * ROUNDS
    for i, (a, t) in enumerate(zip(alone, together)):
        assert a["acc_indices"] == t["acc_indices"] and len(a["acc_indices"]) == ROUNDS, (loop, i)
        assert a["returned"] == t["returned"] and len(set(a["returned"])) == ROUNDS, (loop, i)
        assert a["pruned_fractions"] == t["pruned_fractions"], (loop, i)
        assert a["n_timing"] == t["n_timing"] == ROUNDS and a["log"] == t["log"], (loop, i)
    if loop == "active_search":
        assert all(len(t["pruned_fractions"]) == ROUNDS for t in together)
    assert len({tuple(map(tuple, t["acc_indices"])) for t in together}) > 1   # the members went their own ways

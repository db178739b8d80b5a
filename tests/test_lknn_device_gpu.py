"""GPU: the device-resident L-KNN model (DeviceLKNNModel: ssw_lknn_state_init / condition / step / top_remaining) against
the host LKNNModel and against the numpy restatement of tests/_lknn_device_helpers.py: the reference's planning session,
the edges of the selection (sizes around a wave, a workgroup and a workgroup's slice; exactly L unseen nodes; seen nodes
at the top; exact ties, where the order is (score descending, id ascending)), the one-step branch and top_remaining, the
refusals of condition, and both loops behind the session API with model_on_device on and off."""
import ctypes
import os

import numpy as np
import pytest

from _lknn_device_helpers import Restatement, regular_graph, same_bits
from test_lknn_cpu import session_graph

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
INVALID = -1  # SSW_ERR_INVALID


def _models(N, W, gamma, host=True):
    from seesaw_amd.loops.LKNN_model import DeviceLKNNModel, LKNNModel
    from seesaw_amd.research.active_search.common import Dataset
    dev = DeviceLKNNModel.from_dataset(Dataset.from_vectors(np.zeros((N, 1))), weight_matrix=W, gamma=gamma)
    ref = LKNNModel.from_dataset(Dataset.from_vectors(np.zeros((N, 1))), weight_matrix=W, gamma=gamma.copy()) if host else None
    return dev, ref


def _state_equals(dev, numerators, denominators, gamma, seen_ids):
    st = dev.state()
    seen = np.zeros(dev.n, dtype=bool)
    seen[np.asarray(list(seen_ids), dtype=np.int64)] = True
    return (np.array_equal(st["numerators"], numerators) and np.array_equal(st["denominators"], denominators)
            and same_bits(st["gamma"], gamma) and np.array_equal(st["seen"], seen))


@pytest.mark.parametrize("horizon", [2, 9, 20, 101])
def test_planning_session_on_the_device_model_matches_reference(horizon):
    from seesaw_amd.loops.LKNN_model import initial_gamma_array
    from seesaw_amd.research.active_search.efficient_nonmyopic_search import efficient_nonmyopic_search
    g = np.load(os.path.join(GOLDEN, "lknn.npz"))
    N, D, nbr, W, truth = session_graph(g)
    dev, host = _models(N, W, initial_gamma_array(0.1, N))
    for rnd in range(12):
        res = efficient_nonmyopic_search(dev, reward_horizon=horizon, lookahead_limit=2, pruning_on=False,
                                         implementation="vectorized")
        info = dev.step_info()
        assert info["host_waits"] == 1 and info["bytes_to_device"] == 0 and info["bytes_to_host"] < 8 * N, info
        assert int(res.index) == int(g[f"h{horizon}_picks"][rnd]), (horizon, rnd)
        assert res.value == g[f"h{horizon}_values"][rnd], (horizon, rnd, res.value, g[f"h{horizon}_values"][rnd])
        if rnd in (0, 5, 11):
            best, value, vals = dev.top_sum(K=horizon - 1, return_values=True)
            assert (best, value) == (int(res.index), res.value)
            assert same_bits(vals, g[f"h{horizon}_values_r{rnd}"]), (horizon, rnd)
            info = dev.step_info()
            assert info["host_waits"] == 1 and info["bytes_to_device"] == 0, info
        y = int(truth[int(res.index)])
        dev.condition_(int(res.index), y)
        host.condition_(int(res.index), y)
        assert _state_equals(dev, host.numerators, host.denominators, host.gamma, host.dataset.seen_indices), (horizon, rnd)
    assert list(dev.dataset.seen_indices) == list(host.dataset.seen_indices) and dev.dataset.idx2label == host.dataset.idx2label
    dev.close()


def _prior(n, seed):
    return np.random.default_rng(seed).normal(loc=0.1, scale=1e-6, size=n)


def _check_step(dev, twin, K, oracle, where):
    pick, value, values, top = twin.step(K, oracle)
    got_pick, got_value, got_values, got_top = dev.step(K, 2, return_values=True, return_list=True)
    assert np.array_equal(got_top, top), where
    assert same_bits(got_values, values), where
    assert (got_pick, got_value) == (pick, value), where


@pytest.mark.parametrize("K", [1, 8, 128])
@pytest.mark.parametrize("D", [1, 10, 32])
def test_selection_edges_against_the_restatement(oracle, D, K):
    """sizes on either side of a wave (64), a workgroup (256) and a workgroup's slice (2048 rows: 8193 is four slices and
    one row); node 0 is its own neighbour; after the first step the three best nodes are answered, so seen nodes sit at
    the top of the order; n = L + 1 ends with exactly L unseen nodes, n = L with one too few"""
    from seesaw_amd._lib import SeesawHipError
    L = K + D
    for n in sorted({L, L + 1, 255, 256, 257, 1023, 1025, 8193}):
        if n < L:
            continue
        nbr, W = regular_graph(n, D, seed=100 + n, self_loop_at=0)
        gamma = _prior(n, n)
        dev, _ = _models(n, W, gamma, host=False)
        twin = Restatement(nbr, gamma)
        _check_step(dev, twin, K, oracle, (n, "fresh"))
        answers = [int(i) for i in twin.select(3)] if n >= L + 3 else [int(twin.select(1)[0])] if n == L + 1 else []
        if n >= L + 40:
            answers += [int(i) for i in np.random.default_rng(n).choice(np.setdiff1d(np.arange(n), answers), 20, replace=False)]
        for t, i in enumerate(answers):
            twin.condition(i, t % 2)
        dev.condition_many_([(i, t % 2) for t, i in enumerate(answers)])
        assert _state_equals(dev, twin.numerators, twin.denominators, twin.gamma, np.flatnonzero(twin.seen)), n
        if n > L:
            assert n - len(answers) >= L and (n != L + 1 or n - len(answers) == L)
            _check_step(dev, twin, K, oracle, (n, "answered"))
        else:  # one unseen node fewer than the list needs
            dev.condition_(int(twin.select(1)[0]), 1)
            with pytest.raises(SeesawHipError) as err:
                dev.step(K, 2)
            assert err.value.status == INVALID and "unseen" in str(err.value)
        dev.close()


@pytest.mark.parametrize("tied", [2, 4])
def test_exact_ties_inside_the_list_and_across_its_last_place(oracle, tied):
    """`tied` nodes share gamma and counts inside the list, and `tied` more straddle its last place: the list and the values
    are those of the order (score descending, id ascending) -- compared with the lexsort restatement, not the host model"""
    n, D, K = 1025, 10, 8
    L = K + D
    nbr, W = regular_graph(n, D, seed=7)
    gamma = _prior(n, 3)
    order = np.argsort(-gamma)
    inside = order[3:3 + tied]
    across = order[L - tied // 2:L + tied // 2]
    gamma[inside] = gamma[inside[0]]
    gamma[across] = gamma[across[0]]
    dev, _ = _models(n, W, gamma, host=False)
    twin = Restatement(nbr, gamma)
    assert not twin.top_distinct(L)
    top = twin.select(L)
    assert set(inside) <= set(top) and len(set(across) & set(top)) == tied // 2
    assert sorted(set(across) & set(top)) == sorted(across)[:tied // 2]   # the lower ids are the ones inside
    _check_step(dev, twin, K, oracle, "ties")
    ids, scores = dev.top_k_remaining(L + tied)
    assert np.array_equal(ids, twin.select(L + tied)) and same_bits(scores, twin.operands()[2][ids])
    dev.close()


def test_one_step_branch_and_top_remaining_against_the_host_model():
    from seesaw_amd.loops.LKNN_model import initial_gamma_array
    from seesaw_amd.research.active_search.efficient_nonmyopic_search import efficient_nonmyopic_search
    n, D = 2500, 10
    nbr, W = regular_graph(n, D, seed=11)
    dev, host = _models(n, W, initial_gamma_array(0.1, n))
    rng = np.random.default_rng(2)
    answers = [(int(i), int(rng.random() < 0.3)) for i in rng.choice(n, 20, replace=False)]
    dev.condition_many_(answers)
    for i, y in answers:
        host.condition_(i, y)
    a = efficient_nonmyopic_search(dev, reward_horizon=1, lookahead_limit=1, pruning_on=False, implementation="vectorized")
    b = efficient_nonmyopic_search(host, reward_horizon=1, lookahead_limit=1, pruning_on=False, implementation="vectorized")
    assert int(a.index) == int(b.index) and a.value == b.value
    info = dev.step_info()
    assert info["host_waits"] == 1 and info["bytes_to_device"] == 0, info
    for k in (1, 4, 192):
        ids, scores = dev.top_k_remaining(k)
        want_ids, want_scores = host.top_k_remaining(k)
        assert np.array_equal(ids, want_ids) and same_bits(scores, want_scores), k
    assert int(dev.top_k_remaining(1)[0][0]) == int(b.index)
    some = np.array([0, 5, answers[0][0], n - 1])
    assert same_bits(dev.predict_proba(some), host.predict_proba(some))
    dev.close()


def test_condition_refusals_leave_the_state_and_top_sum_leaves_it_too():
    from seesaw_amd import _lib
    from seesaw_amd.loops.LKNN_model import initial_gamma_array
    n, D, K = 1200, 10, 8
    nbr, W = regular_graph(n, D, seed=21)
    gamma = initial_gamma_array(0.1, n)
    dev, _ = _models(n, W, gamma, host=False)
    twin = Restatement(nbr, gamma)
    dev.condition_many_([(5, 1), (9, 0)])
    twin.condition(5, 1)
    twin.condition(9, 0)
    before = dev.state()
    for pairs, word in [([(17, 1), (n, 0)], "outside"), ([(17, 1), (-1, 0)], "outside"), ([(17, 1), (30, 0), (17, 0)], "repeated"),
                        ([(17, 1), (5, 0)], "answered before"), ([(17, 2)], "neither 0 nor 1")]:
        with pytest.raises(_lib.SeesawHipError) as err:
            dev.condition_many_(pairs)
        assert err.value.status == INVALID and word in str(err.value), (pairs, str(err.value))
        after = dev.state()
        assert all(np.array_equal(before[k], after[k]) for k in before), pairs
        assert list(dev.dataset.seen_indices) == [5, 9]
    dev.condition_(17, 1)   # a refused id is not left marked
    twin.condition(17, 1)
    assert _state_equals(dev, twin.numerators, twin.denominators, twin.gamma, [5, 9, 17])
    # ssw_lknn_top_sum on the same handle between two steps: its staging buffers are not the resident state
    first = dev.step(K, 2, return_values=True)
    numer, denom = np.full(n, 0.5), np.full(n, 2.0)
    top = np.arange(K + D, dtype=np.int32)
    best_i, best_v = ctypes.c_int64(-1), ctypes.c_double(0.0)
    _lib.call("ssw_lknn_top_sum", dev._h, ctypes.c_void_p(numer.ctypes.data), ctypes.c_void_p(denom.ctypes.data),
              ctypes.c_void_p(top.ctypes.data), K, None, ctypes.byref(best_i), ctypes.byref(best_v))
    assert best_i.value >= 0
    assert _state_equals(dev, twin.numerators, twin.denominators, twin.gamma, [5, 9, 17])
    second = dev.step(K, 2, return_values=True)
    assert first[:2] == second[:2] and same_bits(first[2], second[2])
    # with_gamma keeps counts and marks
    new_gamma = np.clip(gamma + np.random.default_rng(1).uniform(0.0, 0.5, n), 0.01, 0.99)
    assert dev.with_gamma(new_gamma) is dev
    twin.set_gamma(new_gamma)
    assert _state_equals(dev, twin.numerators, twin.denominators, new_gamma, [5, 9, 17])
    assert np.array_equal(dev.top_k_remaining(30)[0], twin.select(30))
    dev.close()
    with pytest.raises(RuntimeError, match="closed"):
        dev.step(K, 2)


def test_what_the_device_model_cannot_serve_is_refused_before_the_device():
    import scipy.sparse as sp
    from seesaw_amd.loops.LKNN_model import DeviceLKNNModel
    from seesaw_amd.research.active_search.common import Dataset
    n = 50
    ds = Dataset.from_vectors(np.zeros((n, 1)))
    ragged = sp.csr_array(np.triu(np.ones((n, n)), k=1))
    with pytest.raises(ValueError, match="regular"):
        DeviceLKNNModel.from_dataset(ds, ragged, np.full(n, 0.1))
    dense = sp.csr_array(np.ones((n, n)))   # regular, 50 neighbours a node
    with pytest.raises(ValueError, match="degree 1..32"):
        DeviceLKNNModel.from_dataset(ds, dense, np.full(n, 0.1))
    _, W = regular_graph(n, 4, seed=0)
    dev = DeviceLKNNModel.from_dataset(ds, W, np.full(n, 0.1))
    with pytest.raises(NotImplementedError):
        dev.condition(3, 1)
    with pytest.raises(NotImplementedError):
        dev.probability_bound(1)
    dev.close()


def _session(loop, extra, matrix_extra=None, n_batches=12):
    from seesaw_amd.basic_types import BenchParams, IndexSpec, SessionParams
    from seesaw_amd.bitmap import BitMap
    from seesaw_amd.seesaw_bench import benchmark_loop
    from seesaw_amd.seesaw_session import make_session
    from seesaw_amd.synthetic import GlobalDataManager, make_dataset
    ds = make_dataset("lvis", n_images=1500, tiles_per_image=1, n_categories=2, positive_frac=0.03, seed=4, knn_k=10, signal=0.5)
    gdm = GlobalDataManager().add(ds)
    matrix = dict(knn_path="nndescent60", symmetric=False, self_edges=False, normalized_weights=False, knn_k=10, edist=0.05)
    matrix.update(matrix_extra or {})
    lp = dict(matrix_options=matrix, normalize_scores=False, sigmoid_before_propagate=True, calib_a=10.0, calib_b=-0.4, prior_weight=1.0)
    if loop == "lknn":
        opts = dict(gamma=0.1, use_clip_as_gamma=False, **lp)
    else:
        opts = dict(gamma=dict(mode="clip", calibration="sigmoid", a=10.0, b=-0.2), reward_horizon=10, adjust_horizon=False,
                    max_steps=100, pruning_on=False, implementation="vectorized", **lp)
    opts.update(extra)
    p = SessionParams(index_spec=IndexSpec(d_name="lvis", i_name="coarse"), interactive=loop, interactive_options=opts,
                      batch_size=1, shortlist_size=50, agg_method="plain_score", aug_larger="greater",
                      start_policy="from_start", index_options={"use_vec_index": False})
    b = BenchParams(name=loop, ground_truth_category="c1", qstr="a c1", n_batches=n_batches, max_results=10 ** 6)
    ret = make_session(gdm, p, b=b)
    boxes, _ = ds.load_ground_truth()
    out = benchmark_loop(session=ret["session"], box_data=boxes, subset=BitMap(ds.file_meta.index.values), b=b, p=p)
    return out, [int(a[0]) for a in ret["session"].acc_indices]


@pytest.mark.parametrize("loop,extra", [("lknn", {}), ("active_search", {}),
                                        ("active_search", dict(adjust_horizon=True, max_steps=12))])
def test_loops_show_the_same_images_with_the_model_on_the_device(loop, extra):
    """12 batches of one image; with adjust_horizon the horizon runs 10, 10, 10, 9, ..., 1: the last round is the one-step
    branch"""
    off_out, off = _session(loop, dict(extra))
    on_out, on = _session(loop, dict(extra, model_on_device=True))
    assert on_out["nseen"] == off_out["nseen"] == 12 and len(set(on)) == 12
    assert on == off


@pytest.mark.parametrize("extra,matrix_extra,word", [(dict(implementation="loop"), None, "vectorized"),
                                                     (dict(pruning_on=True), None, "pruning_on"),
                                                     (dict(reward_horizon=130), None, "reward_horizon"),
                                                     ({}, dict(symmetric=True), "regular")])
def test_loop_options_the_device_model_cannot_serve_raise_at_construction(extra, matrix_extra, word):
    with pytest.raises(ValueError, match=word):
        _session("active_search", dict(extra, model_on_device=True), matrix_extra=matrix_extra)

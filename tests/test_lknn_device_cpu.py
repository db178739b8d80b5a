"""CPU: the yardstick of the device-resident L-KNN model (tests/_lknn_device_helpers.py: a numpy state machine, the
selection by lexsort, the look-ahead by the oracle) reproduces the reference's planning session (tests/golden/lknn.npz:
N = 3000, D = 10, horizons 2, 9, 20, 101, 12 rounds each) -- picks and values every round, the value vectors at rounds
0, 5 and 11 bit for bit -- and the L + 1 highest remaining scores are distinct at every round, which is the condition
under which the device model must equal the host model."""
import os

import numpy as np
import pytest

from _lknn_device_helpers import Restatement, lookahead_with_list, regular_graph, same_bits
from test_lknn_cpu import session_graph

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def jittered_prior(n):
    """the prior of the reference's session (LKNN_model.py:70-73), restated"""
    return np.random.default_rng(seed=0).normal(loc=0.1, scale=1e-6, size=n)


@pytest.mark.parametrize("horizon", [2, 9, 20, 101])
def test_restatement_reproduces_the_reference_session(oracle, horizon):
    g = np.load(os.path.join(GOLDEN, "lknn.npz"))
    N, D, nbr, _, truth = session_graph(g)
    model = Restatement(nbr, jittered_prior(N))
    K = horizon - 1
    for rnd in range(12):
        assert model.top_distinct(K + D), (horizon, rnd)
        pick, value, values, top = model.step(K, oracle)
        assert pick == int(g[f"h{horizon}_picks"][rnd]), (horizon, rnd)
        assert value == g[f"h{horizon}_values"][rnd], (horizon, rnd)
        if rnd in (0, 5, 11):
            assert same_bits(values, g[f"h{horizon}_values_r{rnd}"]), (horizon, rnd)
            if horizon in (2, 20):  # the look-ahead with the list handed in (used under ties) is the oracle's
                numer, denom, _ = model.operands()
                assert same_bits(lookahead_with_list(numer, denom, model.nbr, K, top), values), (horizon, rnd)
        model.condition(pick, int(truth[pick]))


def test_selection_order_under_ties_and_seen_nodes():
    nbr, _ = regular_graph(40, 3, seed=1)
    gamma = np.full(40, 0.25)
    gamma[[7, 3, 30]] = 0.5
    gamma[12] = 0.75
    model = Restatement(nbr, gamma)
    assert model.select(5).tolist() == [12, 3, 7, 30, 0]   # equal scores: the lower id first
    assert not model.top_distinct(3) and model.top_distinct(1)
    model.seen[12] = model.seen[3] = True
    assert model.select(3).tolist() == [7, 30, 0]
    assert model.step1() == (7, 0.5)

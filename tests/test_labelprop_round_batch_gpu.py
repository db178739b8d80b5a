"""GPU: the batched graph round (ssw_labelprop_round_batch through LabelPropagation.round_batch) against the single
rounds (LabelPropagation.round) on twin handles: S sessions' propagation, scores and selection in one call must return,
slot by slot and round by round, the bits of S single calls and leave every handle in the state its own call leaves."""
import contextlib
import io

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

K = 50


def _session_graph(rng, n, deg, weight_hi):
    """a symmetric k-NN-like graph whose weights decide how many sweeps a propagation needs"""
    rows = np.repeat(np.arange(n), deg)
    cols = rng.integers(0, n, n * deg)
    A = sp.coo_array((rng.uniform(0.02, weight_hi, n * deg), (rows, cols)), shape=(n, n)).tocsr()
    W = (A + A.T).tocsr()
    W.setdiag(0)
    W.eliminate_zeros()
    W.sum_duplicates()
    W.sort_indices()
    return W


def _quiet():
    return contextlib.redirect_stdout(io.StringIO())


class _Twins:
    """S twin pairs over two indexes of the same rows: set A is driven by round_batch on index A, set B by round, one
    handle after another, on index B"""

    def __init__(self, rng, n_images, tiles, weight_hi, ordered, S, lambdas=None, const_prior_slot=None, const_prior=0.5):
        from seesaw_amd.device_index import DeviceIndex
        from seesaw_amd.label_propagation import LabelPropagation
        self.n_images, self.tiles, self.n, self.S = n_images, tiles, n_images * tiles, S
        n = self.n
        self.W = _session_graph(rng, n, 5, weight_hi)
        X = rng.standard_normal((n, 256)).astype(np.float32)
        row2image = np.repeat(np.arange(n_images, dtype=np.int32), tiles)
        self.order = rng.permutation(n).astype(np.int32) if ordered else None
        self.idx_a = DeviceIndex.from_numpy(X, row2image=row2image)
        self.idx_b = DeviceIndex.from_numpy(X, row2image=row2image)
        self.lambdas = list(lambdas) if lambdas is not None else [1.0] * S
        self.priors, self.a, self.b = [], [], []
        for j in range(S):
            prior = np.full(n, const_prior) if const_prior_slot in (j, "all") else rng.uniform(0.05, 0.95, n)
            self.priors.append(prior)
            for side in (self.a, self.b):
                lp = LabelPropagation(self.W, reg_lambda=self.lambdas[j], max_iter=300, node_order=self.order)
                lp.collect_run_info = True
                lp.set_prior(prior)
                side.append(lp)
        self.labels = [dict() for _ in range(S)]
        self.excluded = [[] for _ in range(S)]

    def args(self, rng):
        """the per-slot arguments of one round from the label dicts: (propagate, ids, vals, excluded)"""
        prop, ids, vals, exs = [], [], [], []
        for j in range(self.S):
            self.excluded[j] = sorted(set(self.excluded[j]) | set(int(v) for v in rng.choice(self.n_images, size=3, replace=False)))
            i = np.array(sorted(self.labels[j]), dtype=np.int64)
            v = np.array([self.labels[j][int(x)] for x in i], dtype=np.float64)
            p = bool((v == 0).any())
            prop.append(p)
            ids.append(i)
            vals.append(v if p else np.zeros(i.shape[0]))  # (update_and_select hands zeros over while the prior ranks)
            exs.append(np.asarray(self.excluded[j], dtype=np.int64))
        return prop, ids, vals, exs

    def compare(self, got, want, lp_a, lp_b, propagate, where):
        assert not isinstance(got, Exception), (where, got)
        assert got[0].shape == want[0].shape, (where, "count")
        assert np.array_equal(got[0], want[0]), (where, "images")
        assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), (where, "scores")
        assert np.array_equal(got[2], want[2]), (where, "rows")
        if propagate:
            assert (lp_a.last_sweeps, lp_a.last_converged) == (lp_b.last_sweeps, lp_b.last_converged), where
        assert np.array_equal(lp_a.fetch().view(np.uint64), lp_b.fetch().view(np.uint64)), (where, "fetch")
        assert (lp_a.last_mode, lp_a.last_rows_recomputed, lp_a.last_kept_levels) == \
            (lp_b.last_mode, lp_b.last_rows_recomputed, lp_b.last_kept_levels), (where, "run info")

    def round(self, rng, where, a_slots=None):
        """one round: round_batch on set A (on `a_slots` of it; the other A handles take their own `round`), round on every
        B handle; everything compared.  -> (stats of the batched call, the per-slot arguments, A's results)"""
        from seesaw_amd.label_propagation import LabelPropagation
        prop, ids, vals, exs = self.args(rng)
        slots = list(range(self.S)) if a_slots is None else list(a_slots)
        with _quiet():
            outs = LabelPropagation.round_batch([self.a[j] for j in slots], self.idx_a, propagate=[prop[j] for j in slots],
                                                label_ids=[ids[j] for j in slots], label_values=[vals[j] for j in slots],
                                                mask_labeled=True, excluded=[exs[j] for j in slots], k=K)
            got = dict(zip(slots, outs))
            for j in range(self.S):
                if j not in got:
                    got[j] = self.a[j].round(self.idx_a, propagate=prop[j], label_ids=ids[j], label_values=vals[j],
                                             mask_labeled=True, excluded=exs[j], k=K)
            want = [self.b[j].round(self.idx_b, propagate=prop[j], label_ids=ids[j], label_values=vals[j], mask_labeled=True,
                                    excluded=exs[j], k=K) for j in range(self.S)]
        for j in range(self.S):
            self.compare(got[j], want[j], self.a[j], self.b[j], prop[j], (where, j))
        return LabelPropagation.last_batch_stats, (prop, ids, vals, exs), got

    def close(self):
        for lp in self.a + self.b:
            lp.close()
        self.idx_a.close()
        self.idx_b.close()


def _add(rng, labels, n, count, positive_only=False):
    for v in rng.choice(n, size=count, replace=False):
        labels[int(v)] = 1.0 if positive_only else float(rng.integers(0, 2))


@pytest.mark.parametrize("n_images,tiles,weight_hi,ordered", [(900, 5, 0.03, False), (9000, 9, 0.03, False), (9000, 9, 0.25, False),
                                                              (8000, 10, 0.04, True)])
def test_round_batch_equals_the_single_rounds(oracle, n_images, tiles, weight_hi, ordered):
    """Five sessions, ten rounds, one round_batch a round against five rounds on the twins.  The label streams are
    scripted so that one call mixes the states a slot can be in: slot 0 has only positive labels until round 4 (the
    prior ranks: propagate=False), slot 1 adds n // 6 labels in round 6 (more than the frontier holds / the change the
    tracked run takes), slot 2 changes nothing in round 5, slot 3 loses a label in round 5 and has one flipped in round
    7, slot 4 runs with reg_lambda = 2.  (900, 5): the selection's small form; (9000, 9): the general form, where slot
    3's prior is the constant 0.5 -- nearly every image ties at 0.5f and the fast selection overflows; weight_hi = 0.25:
    runs of five or six sweeps whose incremental passes do not end in the batch -- the slots are finished by the
    continuation's full sweeps (the continuation FROM kept iterates has a test of its own below); (8000, 10): a node
    order.
    Waits: a call whose propagating slots were all batched and converged waits once -- plus once for a slot that had to
    be selected again on the deep path, which only the constant-prior shape has; there the 50th score of that slot
    being exactly 0.5f means over 8 900 images share its key, so the rerun is certain, and otherwise it may or may not
    happen (scores within 256 ulp of 0.5f share the selection's 24-bit bin)."""
    rng = np.random.default_rng(n_images + tiles)
    light = weight_hi <= 0.05
    ties_slot = 3 if (n_images, weight_hi) == (9000, 0.03) else None
    tw = _Twins(rng, n_images, tiles, weight_hi, ordered, S=5, lambdas=[1.0, 1.0, 1.0, 1.0, 2.0], const_prior_slot=ties_slot)
    n = tw.n
    batched_calls = 0
    for rnd in range(10):
        for j in range(5):
            lab = tw.labels[j]
            if j == 0:
                _add(rng, lab, n, int(rng.integers(1, 14)), positive_only=rnd < 4)
            elif j == 1 and rnd == 6:
                _add(rng, lab, n, n // 6)
            elif j == 2 and rnd == 5:
                pass
            elif j == 3 and rnd == 5 and lab:
                lab.pop(sorted(lab)[1])
            elif j == 3 and rnd == 7 and lab:
                key = sorted(lab)[0]
                lab[key] = 1.0 - lab[key]
            else:
                _add(rng, lab, n, int(rng.integers(1, 14)))
        stats, (prop, ids, vals, exs), got = tw.round(rng, rnd)
        kept = [lp.last_kept_levels for lp, p in zip(tw.a, prop) if p]
        modes = [lp.last_mode for lp in tw.a]
        print(f"round {rnd}: stats {stats} modes {modes} kept {kept}")
        if stats[0] >= 2:
            batched_calls += 1
        propagating = sum(prop)
        # every propagating slot was batched and converged: none went the single way or through the continuation, and
        # the batched ones are the incremental updates (mode 1; a slot whose labels did not change is mode 1 without a pass)
        if stats[3] == 0 and propagating > 0 and all(m == 1 for m, p in zip(modes, prop) if p):
            if ties_slot is None:
                assert stats[2] == 1, (rnd, stats)
            else:
                sc = got[ties_slot][1]
                assert 1 <= stats[2] <= 2, (rnd, stats)
                if sc.shape[0] == K and sc[K - 1] == np.float32(0.5):
                    assert stats[2] == 2, (rnd, stats)
            assert stats[1] <= 3 + 3 * max(kept), (rnd, stats, kept)
        if (n_images, tiles) == (900, 5) and prop[4]:  # one slot against the CPU oracle's bits
            ref, sweeps, conv = oracle.label_propagation(tw.W, label_ids=ids[4], label_values=vals[4], reg_lambda=2.0,
                                                         reg_values=tw.priors[4], start_value=tw.priors[4], max_iter=300)
            assert (tw.a[4].last_sweeps, tw.a[4].last_converged) == (sweeps, conv), rnd
            assert np.array_equal(tw.a[4].fetch().view(np.uint64), ref.view(np.uint64)), rnd
    if light:
        assert batched_calls >= 3, batched_calls
    tw.close()


def test_round_batch_chunks_and_continues():
    """On the 4 500-row graph: S = 1 equals round; S = 17 -- two chunks inside the one call -- equals 17 single rounds,
    three rounds each.  After a batched round, a single round on one handle and a round_batch on the rest continue
    incrementally (last_mode == 1) with the twins' bits: the batched call left every handle where its own round does."""
    for S in (1, 17):
        rng = np.random.default_rng(40 + S)
        tw = _Twins(rng, 900, 5, 0.03, False, S=S)
        for rnd in range(3):
            for lab in tw.labels:
                _add(rng, lab, tw.n, int(rng.integers(2, 10)))
                if rnd == 0:
                    lab[int(rng.integers(0, tw.n))] = 0.0  # every session propagates from the first round on
            stats, (prop, *_), _ = tw.round(rng, (S, rnd))
            assert all(prop)
            if rnd > 0:
                assert stats[0] == S and stats[3] == 0, (S, rnd, stats)
                assert stats[2] == (S + 15) // 16, (S, rnd, stats)  # one wait a chunk
        if S == 17:
            for lab in tw.labels:
                _add(rng, lab, tw.n, 3)
            stats, _, _ = tw.round(rng, "mixed", a_slots=range(1, S))
            assert stats[0] == S - 1, stats
            assert [lp.last_mode for lp in tw.a] == [1] * S
        tw.close()


def test_round_batch_continues_from_the_kept_levels():
    """The continuation with iterates to keep.  On a random prior the sweeps a run needs are set by the prior's own
    smoothing, so a few changed labels rarely need more sweeps than were kept; here the prior is 0 everywhere.  A first
    propagation whose labels are all 0 moves nothing and converges in its first sweep, so ONE level is kept; labels of
    1 in the next round need a second sweep.  The batched pass brings iterates 0 .. 1 up to date and reports "not
    converged", and the slot is finished by the single path's continuation from iterate 1 (run kind 2) -- with the
    twins' bits, twice in one call, beside a slot that converges."""
    rng = np.random.default_rng(99)
    tw = _Twins(rng, 9000, 9, 0.03, False, S=3, const_prior_slot="all", const_prior=0.0)
    n = tw.n
    for lab in tw.labels:  # the prior is 0 everywhere and so are the labels: nothing moves, sweep 1 converges
        _add(rng, lab, n, 6, positive_only=True)
        for key in lab:
            lab[key] = 0.0
    tw.round(rng, "first")
    assert [lp.last_kept_levels for lp in tw.a] == [1, 1, 1]
    for j in (0, 1):  # a label of 1 moves its neighbours by w / (column sum + lambda) >= 0.02 / 1.6 in the first sweep: 1.5e-4 squared
        _add(rng, tw.labels[j], n, 4, positive_only=True)
    tw.labels[2][int(rng.integers(0, n))] = 0.0
    stats, _, _ = tw.round(rng, "second")
    assert [lp.last_mode for lp in tw.a] == [2, 2, 1], [lp.last_mode for lp in tw.a]
    assert stats[0] == 3 and stats[3] == 2, stats
    tw.round(rng, "third")  # ... and the handles go on from there
    tw.close()


def test_round_batch_refusals():
    """Every refusal is decided before any device work: the call raises, no handle's resident result changes, and a
    correct call right afterwards returns the twins' bits."""
    from seesaw_amd import _lib
    from seesaw_amd.device_index import DeviceIndex
    from seesaw_amd.label_propagation import LabelPropagation
    rng = np.random.default_rng(7)
    tw = _Twins(rng, 900, 5, 0.03, False, S=4)
    n, n_images = tw.n, tw.n_images
    for rnd in range(2):
        for lab in tw.labels:
            _add(rng, lab, n, 5)
            lab[int(rng.integers(0, n))] = 0.0
        tw.round(rng, rnd)
    before = [lp.fetch() for lp in tw.a]
    for lab in tw.labels:
        _add(rng, lab, n, 4)
    prop, ids, vals, exs = tw.args(rng)

    def call(lps=None, index=None, k=K, ids_=None, exs_=None):
        with _quiet():
            return LabelPropagation.round_batch(lps or tw.a, index or tw.idx_a, propagate=prop, label_ids=ids_ or ids,
                                                label_values=vals, mask_labeled=True, excluded=exs_ or exs, k=k)

    other = DeviceIndex.from_numpy(rng.standard_normal((n - 5, 256)).astype(np.float32),
                                   row2image=np.repeat(np.arange(n_images - 1, dtype=np.int32), 5))
    view = tw.idx_a.view(np.arange(n_images, dtype=np.int64))
    bad_ids = [a.copy() for a in ids]
    bad_ids[2][-1] = n
    bad_ids[2].sort()
    bad_exs = [a.copy() for a in exs]
    bad_exs[3][-1] = n_images
    refusals = [("the same handle twice", dict(lps=[tw.a[0], tw.a[1], tw.a[0], tw.a[3]])),
                ("an index with another n", dict(index=other)),
                ("k = 0", dict(k=0)),
                ("a label id equal to n in slot 2", dict(ids_=bad_ids)),
                ("an excluded image equal to n_images in slot 3", dict(exs_=bad_exs))]
    for what, kw in refusals:
        with pytest.raises(_lib.SeesawHipError) as err:
            call(**kw)
        assert err.value.status == _lib.SSW_ERR_INVALID, (what, err.value)
    with pytest.raises(_lib.SeesawHipError) as err:
        call(index=view)
    assert err.value.status == _lib.SSW_ERR_UNSUPPORTED and "view" in str(err.value)
    for lp, f in zip(tw.a, before):
        assert np.array_equal(lp.fetch().view(np.uint64), f.view(np.uint64))
    # the correct call: set B takes its single rounds on the same arguments
    got = call()
    with _quiet():
        want = [tw.b[j].round(tw.idx_b, propagate=prop[j], label_ids=ids[j], label_values=vals[j], mask_labeled=True,
                              excluded=exs[j], k=K) for j in range(4)]
    for j in range(4):
        tw.compare(got[j], want[j], tw.a[j], tw.b[j], prop[j], ("after the refusals", j))
    view.close()
    other.close()
    tw.close()

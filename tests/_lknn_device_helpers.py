"""A numpy restatement of the device-resident L-KNN model, written from its definition and not from the product code
(seesaw_amd/loops/LKNN_model.py, seesaw_amd/csrc/lknn.hip): a state machine over (numerators, denominators, gamma,
seen), the selection as np.lexsort((ids, -score))[:L] -- the total order (score descending, node id ascending) -- and
the look-ahead by oracle.lknn_top_sum.

The oracle picks its own K + D best nodes with an argsort, which is the same list whenever the L + 1 highest remaining
scores are pairwise distinct (`top_distinct`).  Under exact ties the list decides the values, so there the look-ahead is
`lookahead_with_list`, the same row-by-row definition with the list handed in; tests/test_lknn_device_cpu.py holds it to
the oracle, bit for bit, on the reference's session."""
import numpy as np
import scipy.sparse as sp


def regular_graph(n, degree, seed, self_loop_at=None):
    """[n, degree] distinct neighbours a node, rows unsorted as a CSR would hold them, and that CSR"""
    rng = np.random.default_rng(seed)
    nbr = np.stack([rng.choice(n, degree, replace=False) for _ in range(n)]).astype(np.int32)
    if self_loop_at is not None and self_loop_at not in nbr[self_loop_at]:
        nbr[self_loop_at, 0] = self_loop_at
    W = sp.csr_array((np.ones(n * degree), nbr.reshape(-1), np.arange(0, n * degree + 1, degree)), shape=(n, n))
    return nbr, W


def lookahead_with_list(numer, denom, nbr_sorted, K, top):
    """value of every node given the list `top` (best first) of the K + D best remaining nodes: the pool of node i is the
    list without i and without i's neighbours, plus the neighbours (not i) at their scores had i been labelled y; E_y =
    the sum of its K largest, added largest first; value = s (1 + E_1) + (1 - s) E_0"""
    n, D = nbr_sorted.shape
    scores = numer / denom
    top = np.asarray(top, dtype=np.int64)
    top_scores = scores[top]
    after = {0: numer / (denom + 1), 1: (numer + 1) / (denom + 1)}
    out = np.empty(n)
    for i in range(n):
        row = nbr_sorted[i]
        kept = top_scores[~(np.isin(top, row) | (top == i))]
        e = {}
        for y in (0, 1):
            mine = after[y][row[row != i]]
            pool = np.sort(np.concatenate([kept, mine]))[::-1]
            if pool.shape[0] < K:
                pool = np.concatenate([pool, np.full(K - pool.shape[0], -np.inf)])
            e[y] = np.ascontiguousarray(pool[:K]).reshape(1, -1).sum(axis=1)[0]
        with np.errstate(invalid="ignore"):
            out[i] = scores[i] * (1 + e[1]) + (1 - scores[i]) * e[0]
    return out


class Restatement:
    def __init__(self, nbr, gamma):
        self.nbr = np.sort(np.asarray(nbr), axis=1)
        self.n, self.D = self.nbr.shape
        self.numerators, self.denominators = np.zeros(self.n), np.zeros(self.n)
        self.gamma = np.array(gamma, dtype=np.float64)
        self.seen = np.zeros(self.n, dtype=bool)

    def set_gamma(self, gamma):
        self.gamma = np.array(gamma, dtype=np.float64)

    def condition(self, idx, y):
        assert not self.seen[idx] and y in (0, 1)
        js = np.unique(self.nbr[idx])
        self.numerators[js] += y
        self.denominators[js] += 1
        self.seen[idx] = True

    def operands(self):
        numer = self.numerators + self.gamma
        numer[self.seen] = -np.inf
        denom = self.denominators + 1
        return numer, denom, numer / denom

    def select(self, L):
        """the L best unseen nodes, (score descending, id ascending)"""
        _, _, score = self.operands()
        ids = np.flatnonzero(~self.seen)
        return ids[np.lexsort((ids, -score[ids]))[:L]]

    def top_distinct(self, L):
        """are the L + 1 highest remaining scores pairwise distinct (the parity precondition)?"""
        _, _, score = self.operands()
        best = score[self.select(L + 1)]
        return np.unique(best).shape[0] == best.shape[0]

    def step(self, K, oracle):
        """-> (pick, value, all values, the list): lookahead 2"""
        numer, denom, _ = self.operands()
        L = K + self.D
        top = self.select(L)
        assert top.shape[0] == L, "fewer unseen nodes than K + D"
        if self.top_distinct(L):
            values = oracle.lknn_top_sum(numer, denom, self.nbr, K)
        else:
            values = lookahead_with_list(numer, denom, self.nbr, K, top)
        pick = int(np.nanargmax(values))
        return pick, float(values[pick]), values, top

    def step1(self):
        """-> (pick, score): lookahead 1, the first index of the largest remaining score"""
        _, _, score = self.operands()
        pick = int(np.nanargmax(score))
        return pick, float(score[pick])


def same_bits(a, b):
    """equal NaN pattern and equal bits elsewhere"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return np.array_equal(a[ok].view(np.uint64), b[ok].view(np.uint64))

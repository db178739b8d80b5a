"""GPU: the streaming shape of the shadow scan (csrc/prune.hip, k_q8_bounds) and the four-rows-a-lane k_survivors at the
row counts where their loops end: the scan prefetches a group's codes TOGETHER with its rows' constants s_r / a_r one
iteration ahead into one of two register sets, the last n % G rows are a clamped group of their own, a wave without a
next group requests its last one again and must write nothing for it.  The shapes of
tests/test_prune_certificate_gpu.py (2^16 + 1 rows and up) do not reach the small ends, and its synthetic rows all have
norm 1: a row that picked up a neighbour's constants would hardly show.

Row counts, per dim (G = 32 / 16 / 8 rows a group at dim 256 / 512 / 1024; W = waves of a full launch = 4 x CUs):
1, G - 1, G, G + 1 (fewer groups than one block's waves), W G - 1, W G, W G + 1 (every wave one group, then the ragged
group alone / one wave a second group), W G + (W / 2) G + 3 (half the waves two groups: the second register set ends the
loop), 2 W G + G + 1 and 3 W G + 5 (two to four groups a wave: both sets take turns, either one is last; 98 309 rows
at dim 256, below the survivor capacity of 2^18 that "keep all rows" needs).

Rows: Gaussian directions scaled by 2^e with e drawn from -20 .. 20 per row, so neighbouring rows have s_r and a_r
that differ by orders of magnitude; an unboundable row (one +inf element: s = 0, a = +inf) as the last row and as the
first row of the last group.

Checked for every row (the statement of tests/test_prune_certificate_gpu.py): lb < S and
S - lb <= 2 a Q (1 + 2^-19) + |lb| 2^-19 + 2^-98 with S from the f32 scan (pruning off) and a, Q from the lab build's
hooks; lb = -inf where a = +inf.  ssw_debug_prune_survivors equals the numpy survivor set at thresholds that keep none,
one, a few and all of the boundable rows.  Pruned top-k = full top-k, with the three-launch top-k of small indexes
switched off (ssw_tune_topk(2)): it never prunes.  The lab build's other launch shapes
(ssw_tune_prune_scan: 2 / 3 blocks a CU, 4 / 16 loads a group) pass the same per-row check."""
import numpy as np
import pytest

from _prune_helpers import both, hook_bounds, hook_shadow, hook_survivors, mode, same

pytestmark = pytest.mark.gpu

DIMS = (256, 512, 1024)
PAD_ABS = 2.0 ** -100


def f64(a):
    return np.asarray(a, dtype=np.float64)


def full_launch_waves():
    import torch
    return 4 * torch.cuda.get_device_properties(0).multi_processor_count  # one four-wave block a CU


def row_counts(dim, loads=8, blocks=1):
    G = loads * 1024 // dim
    W = full_launch_waves() * blocks
    return [1, G - 1, G, G + 1, W * G - 1, W * G, W * G + 1, W * G + (W // 2) * G + 3, 2 * W * G + G + 1,
            3 * W * G + 5]


def make_rows(n, dim, G, seed):
    """[n, dim] f32: directions x 2^e, e in -20 .. 20 per row; +inf in the last row and in the first row of the last group"""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, dim)).astype(np.float32) / np.float32(np.sqrt(dim))
    X *= np.exp2(rng.integers(-20, 21, n)).astype(np.float32)[:, None]
    X[n - 1, dim // 3] = np.inf
    first_of_last_group = ((n - 1) // G) * G
    X[first_of_last_group, 5] = np.inf
    return np.ascontiguousarray(X)


def the_queries(dim):
    rng = np.random.default_rng(77)
    q = rng.standard_normal(dim).astype(np.float32)
    return [(q / np.linalg.norm(q)).astype(np.float32), (rng.standard_normal(dim) * 37.5).astype(np.float32)]


def check_rows(lab, idx, X, q, G):
    """the per-row statement; -> (S, lb, a, Q)"""
    n = X.shape[0]
    mode(lab, True, 1)
    _, s, a = hook_shadow(idx, codes=False)
    unb = ~np.all(np.isfinite(X), axis=1)
    assert np.array_equal(np.isinf(a), unb) and np.all(s[unb] == 0)
    assert unb[n - 1] and unb[((n - 1) // G) * G]
    mode(lab, False)
    S = idx.scores(q)
    mode(lab, True, 1)
    lb, Q, bad = hook_bounds(idx, q)
    assert bad == 0
    norm = float(np.sqrt(np.sum(f64(q) ** 2)))
    assert norm <= float(Q) <= norm * (1 + 2.0 ** -20)
    fin = ~unb
    assert np.all(lb[unb] == -np.inf), np.nonzero(unb & ~(lb == -np.inf))[0][:8]
    Sd, lbd, aq = f64(S[fin]), f64(lb[fin]), f64(a[fin]) * float(Q)
    rows = np.nonzero(fin)[0]
    assert np.all(np.isfinite(Sd)) and np.all(np.isfinite(lbd)), rows[~np.isfinite(lbd)][:8]
    assert np.all(lbd < Sd), (n, rows[~(lbd < Sd)][:8])
    slack = 2 * aq * (1 + 2.0 ** -19) + np.abs(lbd) * 2.0 ** -19 + 2.0 ** -98
    wide = ~(Sd - lbd <= slack)
    assert not wide.any(), (n, rows[wide][:8], float(((Sd - lbd) / slack).max()))
    return S, lb, a, Q


def survivor_reference(lb, a, Q):
    """k_survivors' upper bound in float64, term by term (NaN where a = +inf: such a row always survives)"""
    l, w = f64(lb), f64(a) * float(Q)
    with np.errstate(invalid="ignore"):
        return l + 2.0 * w + (np.abs(l) + w) * 2.0 ** -20 + 2.0 * PAD_ABS


def thresholds(ub):
    """f32 thresholds between two neighbouring upper bounds that lie clearly apart (the device may contract the formula's
    products and sums, one float64 rounding of difference), keeping none, one, a few and all of the finite ones"""
    u = np.sort(ub[np.isfinite(ub)])[::-1]
    out = []
    if u.size == 0:
        return [np.float32(0)]

    def between(hi, lo):
        t = np.float32((hi + lo) / 2)
        return t if lo < float(t) < hi and (hi - lo) > 1e-6 * max(abs(hi), abs(lo)) else None

    out.append(np.float32(2) * np.float32(abs(u[0])) + np.float32(1))  # keeps none
    for keep in (1, 5, 37):
        if u.size > keep:
            t = between(u[keep - 1], u[keep])
            if t is not None:
                out.append(t)
    out.append(np.float32(-2) * np.float32(np.abs(u).max()) - np.float32(1))  # keeps all
    return out


@pytest.mark.parametrize("dim", DIMS)
def test_bounds_survivors_and_topk_at_the_loop_ends(lab_build, dim):
    from seesaw_amd import _lib
    from seesaw_amd.device_index import DeviceIndex
    G = 8 * 1024 // dim
    try:
        _lib.call("ssw_tune_topk", 2)
        for n in row_counts(dim):
            X = make_rows(n, dim, G, seed=n)
            idx = DeviceIndex.from_numpy(X)
            try:
                mode(lab_build, True, 1)
                for qi, q in enumerate(the_queries(dim)):
                    S, lb, a, Q = check_rows(lab_build, idx, X, q, G)
                    ub = survivor_reference(lb, a, Q)
                    for T in thresholds(ub):
                        expect = np.nonzero(~(ub < float(T)))[0]
                        pub, got, rows = hook_survivors(idx, T, 1)
                        msg = (dim, n, qi, float(T), pub, got, expect.shape[0])
                        assert pub == got == expect.shape[0], msg
                        assert np.array_equal(np.sort(rows), expect), msg
                    for k in sorted({1, min(n, 10), min(n, 100)}):
                        full, pruned, st = both(lab_build, idx, lambda: idx.topk(q, k), min_rows=1)
                        same(full, pruned)
                        assert len(pruned[0]) == k and st[0] == 1 and st[2] >= k, (dim, n, k, st)
            finally:
                idx.close()
    finally:
        mode(lab_build, True)
        _lib.call("ssw_tune_topk", 3)
        _lib.call("ssw_tune_prune_scan", -1, -1)


@pytest.mark.parametrize("blocks,loads", [(2, 8), (3, 8), (1, 4), (1, 16)])
@pytest.mark.parametrize("dim", DIMS)
def test_other_launch_shapes_keep_the_certificate(lab_build, dim, blocks, loads):
    from seesaw_amd import _lib
    from seesaw_amd.device_index import DeviceIndex
    G = loads * 1024 // dim
    try:
        _lib.call("ssw_tune_topk", 2)
        _lib.call("ssw_tune_prune_scan", blocks, loads)
        counts = row_counts(dim, loads, blocks)
        for n in (counts[1], counts[3], counts[6], counts[7], counts[9]):
            X = make_rows(n, dim, G, seed=n + 1)
            idx = DeviceIndex.from_numpy(X)
            try:
                mode(lab_build, True, 1)
                q = the_queries(dim)[0]
                check_rows(lab_build, idx, X, q, G)
                k = min(n, 100)
                full, pruned, st = both(lab_build, idx, lambda: idx.topk(q, k), min_rows=1)
                same(full, pruned)
                assert st[0] == 1 and st[2] >= k, (dim, n, blocks, loads, st)
            finally:
                idx.close()
    finally:
        mode(lab_build, True)
        _lib.call("ssw_tune_topk", 3)
        _lib.call("ssw_tune_prune_scan", -1, -1)

"""CPU twin of the pruned top-k's tail (csrc/prune.hip survivor_pass, csrc/select.hip k_scatter_candidates; DESIGN.md
section 4, "The tail"), on the adversarial rows of tests/_prune_helpers.py beside rows whose norms span 2^40.

  a. the two-step survivor test: a row the pre-test on lb alone rules out (ub with w_max < T and lb > -inf) is never a
     row the test on its own width keeps, for the int8 pair (w = a Q) and the `_mq` pair (w = a wQ + s wE) of both
     shadows, at every threshold; omitting s_max from w_max does lose a survivor here, dropping the lb = -inf clause
     cannot (the ub expression is NaN at lb = -inf whatever the width);
  b. the candidate rule: the k largest composite keys among the survivors at or above the threshold are the k largest
     over all rows, in the oracle's key order (score descending, image position ascending), with NaN scores of either
     sign, signed zeros, mass ties and exclusions."""
import numpy as np
import pytest

from _prune6_helpers import lower_bound6, shadow6, width6
from _prune_batch_helpers import lower_bound, quantise_query, upper_bound, width
from _prune_helpers import adversarial_rows, shadow

DIM = 512
WMAX_INFLATE = 1 + 2.0 ** -30


def rows_and_query():
    rng = np.random.default_rng(0)
    A = adversarial_rows(rng, DIM)
    G = (rng.standard_normal((600, DIM)) / np.sqrt(DIM)).astype(np.float32)
    G *= np.exp2((np.arange(600) * 7) % 41 - 20).astype(np.float32)[:, None]
    X = np.concatenate([A[:30], G, A[30:]])
    q = rng.standard_normal(DIM).astype(np.float32)
    return X, (q / np.linalg.norm(q)).astype(np.float32)


def finite_max(v):
    v = np.asarray(v, dtype=np.float32)
    return np.float64(v[np.isfinite(v)].max())


def pre_test(lb, w_max, T, clause=True):
    """the rows the first step cannot rule out"""
    l = np.asarray(lb, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        cand = ~(upper_bound(l, np.float64(w_max) * WMAX_INFLATE) < np.float64(T))
    return cand | ~(l > -np.inf) if clause else cand


def own_test(lb, w, T):
    with np.errstate(invalid="ignore", over="ignore"):
        return ~(upper_bound(lb, w) < np.float64(T))


def cases():
    """(name, lb, w, w_max, w_max without s_max, w_max over the non-finite entries too)"""
    X, q = rows_and_query()
    qq = quantise_query(q)
    out = []
    c, s, a = shadow(X)
    lb, w, _, _ = lower_bound(c, s, a, qq)
    one = lambda av, sv: float(width(np.array([sv]), np.array([av]), qq, DIM)[0])
    out.append(("mq", lb, w, one(finite_max(a), finite_max(s)), one(finite_max(a), 0.0), one(np.max(a), np.max(s))))
    Q = np.float64(qq["Q"])
    out.append(("int8", lb, a.astype(np.float64) * Q, finite_max(a) * Q, finite_max(a) * Q, np.float64(np.max(a)) * Q))
    c6, s6, a6 = shadow6(X)
    lb6, w6, _ = lower_bound6(c6, s6, a6, qq)
    one6 = lambda av, sv: float(width6(np.array([sv]), np.array([av]), qq, DIM)[0])
    out.append(("q6", lb6, w6, one6(finite_max(a6), finite_max(s6)), one6(finite_max(a6), 0.0),
                one6(np.max(a6), np.max(s6))))
    return out


def thresholds(lb, w):
    with np.errstate(invalid="ignore", over="ignore"):
        ub = upper_bound(lb, w)
    fin = np.sort(ub[np.isfinite(ub)])
    mids = [np.float32(v) for v in fin[:: max(1, fin.size // 40)]]
    mids.append(np.float32(ub[np.argmax(np.where(np.isfinite(w), w, 0))]))  # beside the ub of the widest bounded row
    out = [np.float32(-np.inf), np.float32(np.inf), np.float32(0)] + mids
    out += [np.nextafter(t, np.float32(np.inf)) for t in mids] + [np.nextafter(t, np.float32(-np.inf)) for t in mids]
    return out


@pytest.mark.parametrize("case", cases(), ids=lambda c: c[0])
def test_pre_test_never_rules_out_a_survivor(case):
    name, lb, w, w_max, w_no_s, w_all = case
    assert np.isinf(w).sum() >= 13 and np.all(lb[np.isinf(w)] == -np.inf)  # the unboundable rows: a = +inf, lb = -inf
    assert np.isfinite(w_max) and w_max >= w[np.isfinite(w)].max()
    lost_without_clause = lost_without_s = 0
    for T in thresholds(lb, w):
        keep = own_test(lb, w, T)
        cand = pre_test(lb, w_max, T)
        assert not (keep & ~cand).any(), (name, float(T), np.nonzero(keep & ~cand)[0][:8])
        lost_without_clause += int((keep & ~pre_test(lb, w_max, T, clause=False)).sum())
        lost_without_s += int((keep & ~pre_test(lb, w_no_s, T)).sum())
    # the lb = -inf clause is belt and braces: the ub expression's own (|l| + w) 2^-20 term is +inf at l = -inf, so
    # ub_max is the NaN of -inf + inf there for every w_max and the first clause keeps the row already
    assert lost_without_clause == 0
    # omitting s_max makes w_max smaller than some row's w in the forms that have the term
    assert (lost_without_s > 0) == (name != "int8"), (name, lost_without_s)
    # the maxima over non-finite entries too: w_max = +inf, every row is a candidate at every threshold
    assert np.isinf(w_all) and pre_test(lb, w_all, np.float32(np.inf)).all()


def ord32(v):
    u = np.asarray(v, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint64)


def keys(v):
    return (ord32(v) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - np.arange(len(v), dtype=np.uint64))


def topk_keys(key, keep, k):
    c = np.nonzero(keep)[0]
    return c[np.argsort(key[c])[::-1][:k]]


def candidate_topk(E, lb, surv, excluded, k, rule="ordinal"):
    """the threshold selection over lb, then the k largest keys among the listed survivors"""
    n = len(E)
    keep = np.ones(n, bool)
    keep[excluded] = False
    th = topk_keys(keys(lb), keep, k)
    if th.size < k:
        return None  # the call falls back
    T = lb[th[-1]]
    at = (ord32(E) >= ord32(np.float32(T))) | np.isnan(E)
    if rule == "float":
        with np.errstate(invalid="ignore"):
            at = E >= T
    listed = surv & at & (keep if rule != "no exclusion" else True)
    return topk_keys(keys(E), listed, k)


def scored_rows():
    """exact scores E with ties, signed zeros and NaNs of both signs, lower bounds lb <= E (-inf where E is NaN: an
    unboundable row), and the survivor set of the widths w"""
    rng = np.random.default_rng(3)
    n = 5000
    E = rng.standard_normal(n).astype(np.float32)
    E[rng.integers(0, n, 400)] = E[7]            # a mass tie high up
    E[[11, 12]] = [0.0, -0.0]
    w = (rng.random(n) * 0.3 + 1e-3).astype(np.float64)
    lb = (E.astype(np.float64) - w * rng.random(n)).astype(np.float32)
    lb = np.minimum(lb, np.nextafter(E, np.float32(-np.inf)))
    nan_pos, nan_neg = [5, 4000], [9, 77]
    E[nan_pos] = np.float32(np.nan)
    E[nan_neg] = np.array([0xFFC00000, 0xFFC00000], np.uint32).view(np.float32)
    lb[nan_pos + nan_neg] = -np.inf
    w[nan_pos + nan_neg] = np.inf
    return E, lb, w


@pytest.mark.parametrize("k", [1, 100, 1024])
def test_candidate_rule_equals_the_full_selection(oracle, k):
    E, lb, w = scored_rows()
    n = len(E)
    full_order = np.argsort(keys(E))[::-1]
    for excluded in (np.zeros(0, np.int64), np.concatenate([full_order[:40:2], full_order[k:k + 300:3]]),
                     np.arange(k - 1, n)):  # the last leaves k - 1 images: the fallback
        keep = np.ones(n, bool)
        keep[excluded] = False
        want = topk_keys(keys(E), keep, k)
        th = topk_keys(keys(lb), keep, k)
        if th.size < k:
            assert candidate_topk(E, lb, np.ones(n, bool), excluded, k) is None
            continue
        surv = own_test(lb, w, lb[th[-1]])
        got = candidate_topk(E, lb, surv, excluded, k)
        assert np.array_equal(got, want), (k, excluded.size)
        # the oracle's key order on the same scores (its C restatement takes no NaN: those rows lead or trail by sign)
        fin = ~np.isnan(E)
        o_img, o_s, _ = oracle.topk_images_tiebreak(np.where(fin, E, np.float32(-np.inf)), None, n,
                                                    np.concatenate([excluded, np.nonzero(~fin)[0]]), k)
        lead = [i for i in (5, 4000) if keep[i]]  # sign-clear NaNs, by position
        lead = lead[:k]
        assert np.array_equal(got[:len(lead)], lead)
        m = min(k - len(lead), len(o_img))
        assert np.array_equal(got[len(lead):len(lead) + m], o_img[:m]), (k, excluded.size)
        # mutations: a float comparison drops the leading NaNs; skipping the exclusion check lists excluded images
        if lead:
            assert not np.array_equal(candidate_topk(E, lb, surv, excluded, k, rule="float"), want)
        if excluded.size and k > 1:
            assert not np.array_equal(candidate_topk(E, lb, surv, excluded, k, rule="no exclusion"), want)


def test_sign_set_nan_is_listed_when_nothing_else_is_left(oracle):
    """one unboundable row whose score is a NaN with the sign bit set: T = -inf, and the row is the top-1"""
    E = np.array([0xFFC00000], np.uint32).view(np.float32)
    lb = np.array([-np.inf], np.float32)
    got = candidate_topk(E, lb, np.ones(1, bool), np.zeros(0, np.int64), 1)
    assert np.array_equal(got, [0])

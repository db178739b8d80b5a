"""The feedback engine's objectives held to a float64 restatement (tests/_fb_ref.py, pinned by
tests/test_feedback_ref_cpu.py) at saturated logits, on the kink of the hinge and at the shapes where a path changes
-- through the public entry points only: FeedbackEngine.lossgrad / lossgrad2 / lossgrad2_dev / fit / fit2_dev and
rank_loss.pairwise_sums.  The suite's other feedback tests either use logits in [-1, 1] (where a naive
log(1 + exp(-z)) is right too) or compare two drivers that inline the same bodies of csrc/fb_math.h.

INPUT FAMILIES (tests/_fb_ref.py; their conditions are asserted in tests/test_feedback_ref_cpu.py)
  exact      rows a_i e_0, a_i multiples of 1/8, w = e_0, center=False: z_i = a_i exactly; hinge margin 0.25 with pairs
             on, an eighth inside and an eighth outside the kink.  Every sum is a small dyadic number, so the device's
             item sums and r must equal the f64 values BIT FOR BIT.
  saturated  unit rows with a planted component along w, |w| = 90 (a third of the logits beyond 30, 5 % beyond 80) or 30;
             38 for the pairwise logistic loss (|z_i - z_j| <= 80, where the reference's f32 log(1 + exp) is finite);
             rows scaled to |z| <= 80 for the two-output form, whose logits use the normalised weights.  Targets 0, 1 and
             soft, sample weights in [0.5, 3].
  mild       the same shapes at |z| <= 1: the control.

BOUNDS.  u = 2^-24.  Every bound is computed per case from the reference's values alone; the reference sees the f32
inputs the device sees (rows after the f32 centring, f32 targets, weights and parameters).
  logit      |z32_i - z_i| <= ez_i = (dim + 1) u (sum_k |x_ik w_k| + |b|): dim fma steps and the bias, any order.
  BCE item   c_i [(1 - y) z - f32(f32(-softplus(-z)) lw)] in f64 (torch's two roundings, bce_item): d item / dz =
             c ((1 - y) - lw sigmoid(-z)), within c max(1, lw) in absolute value, so
             e_item_i = c_i (max(1, lw_i) ez_i + 2 u lw_i softplus_i).
  dl/dz      r_i = f32(c ((1 - y) - lw sigmoid(-z))), sigmoid' <= 1/4:  e_r_i = c_i lw_i / 4 ez_i + u |r_i|.
  loss       scale sum_i e_item_i + 2 u |data loss| (the f32 scale 1/n, the f32 part) + the regularisers' own rounding
             (f64 for the logistic ones; for multireg the f32 values torch forms: l_norm (cosh(L) (2 |L| + 8) u + 2 u)
             with L = log w.w, 2 u |p_data|, 4 u l_query) + u |loss| for the f32 output.
  gradient   column k is a chain of min(n, 32) fma steps inside a slab and one addition per slab, m = min(n, 32) +
             ceil(n / 32) + 4 steps with the scale and the regulariser's addition:
             e_g_k = scale (sum_i |x_ik| e_r_i + gamma_m sum_i |r_i x_ik|) + 2 u |greg_k| + 2 u |g_k|, gamma_m = m u / (1 - m u);
             the intercept's entry is an f64 sum: scale sum_i e_r_i + 2 u |g_b|.
  multireg   BCE with lw = 1 and the re-weighted coefficients, which the host forms in f32 from three sequential sums
             over the items: relative (3 n + 6) u on every c_i, added to e_item and e_r.
  pairwise   s_ij is an f32 difference of two f32 logits: |s32 - s| <= d_ij = ez_i + ez_j + u |s_ij|.  The logistic loss
             has slope <= 1 and curvature <= 1/4 in s; the hinge has slope 1 and switches where |margin - t s| <= d_ij,
             such a pair counting with its whole contribution (tests/_fb_ref.py, pairwise).  The f32 coefficient
             coef_j / max_inv_j adds u to every term.
  two-output f32 throughout.  Rows of W over their norm: relative e_nw = (dim / 2 + 4) u (a sequential sum of dim squares
             under a root, a division); logits ez_ic = ((dim + 1) u + e_nw) sum_k |x_ik nw_ck|.  Per row: the BCE pair has
             slope <= 1 in each logit and about eight roundings of terms of magnitude |(1 - y) z| + |min(z, 0)| +
             softplus; the horizontal CE slope <= y_0 + y_1 and twelve roundings of y_c (|z_c| + |lse|); expf / log1pf /
             logf of the device library within 4 u.  The item sums are a sequential sum per thread and a 1024-wide tree:
             gamma with ceil(n / 1024) + 10 steps.  The gradient planes as above; the chain rule through the
             normalisation and the regularisers term by term (_two_output_bounds).

OBSERVED / BOUND, the largest ratio per family over all its cases, the fits' reported losses included (MI355X; the
module prints the table when it ends, and every comparison prints its own figures before it asserts):
  logreg saturated             0.20  loss, n = 2 dim 16 vector          logreg mild               0.13  gradient
  multireg ce saturated        0.58  p_norm, n = 2048 dim 1024          multireg ce mild          0.12  parts
  multireg hinge saturated     0.52  label loss, n = 4095               multireg pairwise mild    0.12  gradient
  multireg logistic saturated  0.37  label loss, n = 1025               multireg exact            0.10  label loss, soft
  pairwise_sums hinge          0.64  r, n = 1025                        pairwise_sums logistic    0.32  item sums, n = 4096
  two-output saturated         0.10  parts, n = 1 dim 4                 two-output mild           0.10  parts
No family is below 0.01, so no derivation was tightened.  Inside a family the worst-case constants show: at n in the
thousands the ratios of the loss and the gradient drop to 1e-3 .. 1e-4 (the bound adds every row's worst logit error
with one sign, the device's errors cancel), and the fits' reported losses sit at 1e-4 .. 0.2 of the loss bound.
NOT TESTED, being the reference's own behaviour: above |z_i - z_j| ~ 88 its f32 pairwise log(1 + exp(.)) returns inf,
the device's f64 form (fb_pairwise_body) stays finite up to ~709; the logistic family stays below 80.

WHICH EVALUATION `fit` REPORTS.  lbfgs_host (feedback_lbfgs.hip) returns `loss` = br_f[low] of the last strong-Wolfe
search, the closure value at x + t d for the accepted t -- and then sets x += t d with the same expression, so
out_final_loss (info["loss"]) is the evaluation AT THE RETURNED WEIGHTS (at the start weights when no iteration
ran); fit_wg_body (feedback_fit_wg.hip) publishes the same D.loss.  It is held here to the f64 loss at the returned
weights, within the loss bound formed there.
"""
import math
import os

import numpy as np
import pytest

import _fb_ref as R

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
RATIOS = {}
LOSS_CODE = {"ce_loss": 0, "pairwise_rank_loss": 1, "pairwise_logistic_loss": 2}
REG_CODE = {"none": 0, "vector": 1, "norm": 2, "norm1": 3}


@pytest.fixture(scope="module", autouse=True)
def _report_ratios():
    yield
    print("\nobserved / bound, largest per family:")
    for fam in sorted(RATIOS):
        print(f"  {fam:34s} {RATIOS[fam][0]:.3g}   ({RATIOS[fam][1]})")


def _hold(family, what, got, ref, bound):
    """|got - ref| <= bound element by element; prints the figures first and records the largest ratio"""
    got, ref, bound = (np.asarray(a, np.float64).reshape(-1) for a in (got, ref, bound))
    assert got.shape == ref.shape == bound.shape, (what, got.shape, ref.shape, bound.shape)
    assert np.isfinite(got).all(), (what, "not finite")
    err = np.abs(got - ref)
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    k = int(ratio.argmax())
    print(f"  {family} {what}: worst error / bound {ratio[k]:.3g} (error {err[k]:.3g}, bound {bound[k]:.3g}, "
          f"reference {ref[k]:.6g}, entry {k})")
    if ratio[k] > RATIOS.get(family, (0.0, ""))[0] and np.isfinite(ratio[k]):
        RATIOS[family] = (float(ratio[k]), what)
    assert (err <= bound).all(), (family, what, k, got[k], ref[k], err[k], bound[k])


def ez_of(dim):
    return lambda absxw: (dim + 1) * U * absxw


def _gamma(m):
    return m * U / (1.0 - m * U)


# ---- bounds of the one-output objectives ---------------------------------------------------------------
def _one_output_bounds(ref, Xc, dim, has_bias, multireg_kw=None):
    """-> (e_loss, e_data, e_grad [dim (+1)], e_parts [4] or None) from the reference's values (module docstring)"""
    Xc = np.asarray(Xc, np.float64)
    n = Xc.shape[0]
    scale = ref["scale"]
    ez = ez_of(dim)(ref["absxw"])
    c = np.abs(ref["coef"])
    if "pair" in ref:
        p = ref["pair"]
        e_item = p["e_item"] + 2 * U * np.abs(ref["item"])
        e_r = p["e_r"] + U * p["abs_r"] + U * np.abs(ref["r"])
    elif "sp" in ref:
        lw = ref["lw"]
        e_item = c * (np.maximum(1.0, lw) * ez + 2 * U * lw * ref["sp"])
        e_r = c * lw / 4.0 * ez + U * np.abs(ref["r"])
        if multireg_kw is not None:   # the f32 re-weighting on the host
            e_item = e_item + (3 * n + 6) * U * np.abs(ref["item"])
            e_r = e_r + (3 * n + 6) * U * np.abs(ref["r"])
    else:                             # label loss off
        e_item, e_r = np.zeros(n), np.zeros(n)
    data = scale * ref["item"].sum()
    e_data = scale * e_item.sum() + 2 * U * abs(data) + n * 2.0 ** -52 * scale * np.abs(ref["item"]).sum()
    m = min(n, 32) + (n + 31) // 32 + 4
    g_data = scale * (Xc.T @ ref["r"])
    e_grad = scale * (np.abs(Xc).T @ e_r + _gamma(m) * (np.abs(Xc).T @ np.abs(ref["r"]))) + 2 * U * np.abs(ref["greg"]) \
        + 2 * U * np.abs(g_data) + 2 * U * np.abs(ref["grad"][:dim])
    if has_bias:
        e_grad = np.concatenate([e_grad, [scale * e_r.sum() + 2 * U * abs(ref["grad"][dim])]])
    e_parts = None
    if multireg_kw is None:
        e_reg = 1e-14 * (abs(ref["reg_loss"]) + 1.0)
    else:
        L = math.log(ref["ww"])
        p_norm, p_data, p_query, _ = ref["parts"]
        e_norm = multireg_kw["l_norm"] * (math.cosh(L) * (2 * abs(L) + 8) * U + 2 * U)
        e_pd, e_pq = 2 * U * abs(p_data), 4 * U * multireg_kw["l_query"]
        e_reg = e_norm + e_pd + e_pq
        e_parts = np.array([e_norm + U * abs(p_norm), e_pd + U * abs(p_data), e_pq + U * abs(p_query), e_data + U * abs(data)])
    e_loss = e_data + e_reg + U * abs(ref["loss"])
    return e_loss, e_data + U * abs(data), e_grad, e_parts


def _logreg_engine(f):
    from seesaw_amd import _lib
    from seesaw_amd.feedback import FeedbackEngine
    eng = FeedbackEngine(f["dim"])
    eng.set_data(f["X"], center=f["center"])
    eng.set_targets(f["y"], f["sw"])
    eng.set_query(f["q"])
    obj = _lib.FbObjective(kind=_lib.SSW_FB_LOGREG, loss_type=0, fit_intercept=f["icpt"], reg_kind=REG_CODE[f["reg"]],
                           pos_weight=f["pos_weight"], reg_weight=f["reg_weight"], margin=0, reg_norm_lambda=0,
                           reg_data_lambda=0, reg_query_lambda=0)
    return eng, obj


def _multireg_engine(f):
    from seesaw_amd import _lib
    from seesaw_amd.feedback import FeedbackEngine
    eng = FeedbackEngine(f["dim"])
    eng.set_data(f["X"], center=f["center"])
    eng.set_targets(f["y"], f["sw"])
    eng.set_query(f["q"])
    if f["xlx"] is not None:
        eng.set_xlx(f["xlx"])
    kw = f["kw"]
    obj = _lib.FbObjective(kind=_lib.SSW_FB_MULTIREG, loss_type=LOSS_CODE[kw["loss_type"]], fit_intercept=0, reg_kind=0,
                           pos_weight=kw["pos_weight"], reg_weight=0.0, margin=kw["margin"],
                           reg_norm_lambda=kw["l_norm"], reg_data_lambda=kw["l_data"], reg_query_lambda=kw["l_query"])
    return eng, obj


def _hold_logreg(family, f, eng, obj):
    loss, grad, parts = eng.lossgrad(obj, f["w"])
    ref = f["ref"]
    e_loss, e_data, e_grad, _ = _one_output_bounds(ref, f["Xc"], f["dim"], bool(f["icpt"]))
    tag = f"n={f['n']} dim={f['dim']} {f['reg']} intercept={f['icpt']} pw={f['pos_weight']:.3g}"
    _hold(family, f"loss [{tag}]", loss, ref["loss"], e_loss)
    _hold(family, f"data part [{tag}]", parts[3], ref["data_loss"], e_data)
    assert parts[0] == parts[1] == parts[2] == 0.0
    _hold(family, f"gradient [{tag}]", grad, ref["grad"], e_grad)


def _hold_multireg(family, f, eng, obj):
    loss, grad, parts = eng.lossgrad(obj, f["w"])
    ref = f["ref"]
    e_loss, _, e_grad, e_parts = _one_output_bounds(ref, f["Xc"], f["dim"], False, f["kw"])
    tag = f"n={f['n']} dim={f['dim']} {f['kw']['loss_type']} pw={f['kw']['pos_weight']:.3g}"
    _hold(family, f"loss [{tag}]", loss, ref["loss"], e_loss)
    _hold(family, f"parts [{tag}]", parts, ref["parts"], e_parts)
    _hold(family, f"gradient [{tag}]", grad, ref["grad"], e_grad)


# ---- logistic regression -------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(R.LOGREG_CASES)), ids=lambda k: "n%d-dim%d-%s-b%d" % R.LOGREG_CASES[k][:4])
def test_logreg_saturated(k):
    """loss, data part and every gradient entry (the intercept's included) at logits spanning +-90, every n and dim
    of the table, every regulariser kind with and without the intercept, pos_weight 0.2 / 1 / 7 / balanced"""
    f = R.logreg_case(k, R.SPAN_SAT)
    eng, obj = _logreg_engine(f)
    _hold_logreg("logreg saturated", f, eng, obj)
    eng.close()


@pytest.mark.parametrize("k", range(0, len(R.LOGREG_CASES), 2), ids=lambda k: "n%d-dim%d-%s-b%d" % R.LOGREG_CASES[k][:4])
def test_logreg_span_30(k):
    f = R.logreg_case(k, R.SPAN_MID)
    eng, obj = _logreg_engine(f)
    _hold_logreg("logreg saturated", f, eng, obj)
    eng.close()


@pytest.mark.parametrize("k", range(len(R.LOGREG_CASES)), ids=lambda k: "n%d-dim%d-%s-b%d" % R.LOGREG_CASES[k][:4])
def test_logreg_mild_control(k):
    f = R.logreg_case(k, R.SPAN_MILD)
    eng, obj = _logreg_engine(f)
    _hold_logreg("logreg mild", f, eng, obj)
    eng.close()


# ---- RegModule, BCE labels -----------------------------------------------------------------------------
_CE_IDS = lambda k: "n%d-dim%d" % R.MULTIREG_CE_CASES[k][:2]  # noqa: E731


@pytest.mark.parametrize("k", range(len(R.MULTIREG_CE_CASES)), ids=_CE_IDS)
def test_multireg_ce_saturated(k):
    """the balanced re-weighting (its y == 1 test against soft targets), the BCE items and the three regularisers"""
    f = R.multireg_ce_case(k, R.SPAN_SAT)
    eng, obj = _multireg_engine(f)
    _hold_multireg("multireg ce saturated", f, eng, obj)
    eng.close()


@pytest.mark.parametrize("k", range(len(R.MULTIREG_CE_CASES)), ids=_CE_IDS)
def test_multireg_ce_mild_control(k):
    f = R.multireg_ce_case(k, R.SPAN_MILD)
    eng, obj = _multireg_engine(f)
    _hold_multireg("multireg ce mild", f, eng, obj)
    eng.close()


# ---- RegModule, pairwise labels ------------------------------------------------------------------------
_PAIR_IDS = lambda k: "n%d-dim%d-%s" % R.MULTIREG_PAIR_CASES[k][:3]  # noqa: E731


@pytest.mark.parametrize("k", range(len(R.MULTIREG_PAIR_CASES)), ids=_PAIR_IDS)
def test_multireg_pairwise_saturated(k):
    """hinge at logits spanning +-90, logistic at +-38, 2 items to FB_MAX_PAIRWISE"""
    f = R.multireg_pair_case(k, ez_of=ez_of(R.MULTIREG_PAIR_CASES[k][1]))
    eng, obj = _multireg_engine(f)
    fam = "multireg hinge saturated" if f["kw"]["loss_type"] == "pairwise_rank_loss" else "multireg logistic saturated"
    _hold_multireg(fam, f, eng, obj)
    eng.close()


@pytest.mark.parametrize("k", [0, 1, 2, 6, 7, 8], ids=_PAIR_IDS)
def test_multireg_pairwise_mild_control(k):
    f = R.multireg_pair_case(k, ez_of=ez_of(R.MULTIREG_PAIR_CASES[k][1]), mild=True)
    eng, obj = _multireg_engine(f)
    _hold_multireg("multireg pairwise mild", f, eng, obj)
    eng.close()


def test_pairwise_refuses_more_than_its_limit_by_name():
    from seesaw_amd import _lib, rank_loss
    f = R.multireg_case(4097, 4, 7, R.SPAN_MILD, False, "pairwise_rank_loss")
    eng, obj = _multireg_engine(f)
    with pytest.raises(_lib.SeesawHipError, match="4096"):
        eng.lossgrad(obj, f["w"])
    with pytest.raises(_lib.SeesawHipError, match="4096"):
        eng.fit(obj, f["w"], 3)
    eng.close()
    with pytest.raises(_lib.SeesawHipError, match="4096"):
        rank_loss.pairwise_sums(f["y"], scores=f["Xc"][:, 0], margin=0.2)


@pytest.mark.parametrize("logistic", [False, True], ids=["hinge", "logistic"])
@pytest.mark.parametrize("n", [2, 3, 1024, 1025, 4095, 4096])
def test_pairwise_sums_on_given_scores(n, logistic):
    """rank_loss.pairwise_sums (the kernel the fit evaluates, without a data matrix in front of it): item sums and r
    on f32 scores spanning +-90 (hinge) / +-38 (logistic), weighted coefficients"""
    from seesaw_amd import rank_loss
    rng = np.random.default_rng(n)
    span = R.SPAN_PAIR_LOGISTIC if logistic else R.SPAN_SAT
    z = (span * R.planted_fraction(n)).astype(np.float32)
    y, sw = R.labels_mixed(n, n + 1)
    coef = (sw * rng.uniform(0.5, 2.0, n)).astype(np.float32)
    margin = R.f32(0.2)
    item, r = rank_loss.pairwise_sums(y, scores=z, margin=margin, logistic=logistic, coef=coef)
    ref = R.pairwise(y, z, coef, margin, logistic, ez=np.zeros(n))
    fam = "pairwise_sums logistic" if logistic else "pairwise_sums hinge"
    _hold(fam, f"item sums [n={n}]", item, ref["item"], ref["e_item"] + 2 * U * np.abs(ref["item"]))
    _hold(fam, f"r [n={n}]", r, ref["r"], ref["e_r"] + U * ref["abs_r"] + U * np.abs(ref["r"]))


# ---- the exact family: bit for bit -------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["kink", "soft", "one_pos", "equal"])
def test_hinge_on_the_kink_bit_for_bit(kind):
    """pairs with margin - t s == 0 exactly: torch's clamp(min=0) passes the gradient there, so must h >= 0.  All
    values are small dyadic numbers: the device's item sums and r equal the f64 ones bit for bit.  `equal` has no
    pair at all (max_inv = 0: coefficient 0, not 0 / 0), `one_pos` a single positive, `soft` targets in (0, 1)."""
    from seesaw_amd import rank_loss
    f = R.family_exact(kind)
    y, a = f["y"], f["a"]
    cnt = rank_loss.max_inversions(y)
    coef = (cnt * f["sw"]).astype(np.float32)
    item, r = rank_loss.pairwise_sums(y, scores=a, margin=f["margin"], logistic=False, coef=coef)
    ref = R.pairwise(y, a, coef, f["margin"], logistic=False)
    print(f"  exact {kind}: {ref['kinks']} ordered pairs on the kink; item sums {item.sum()} vs {ref['item'].sum()}")
    assert np.array_equal(item, ref["item"]), (kind, item, ref["item"])
    assert np.array_equal(r.astype(np.float64), ref["r"]), (kind, r, ref["r"])
    # the logistic loss on the same items, to its bound (s is exact here)
    item, r = rank_loss.pairwise_sums(y, scores=a, logistic=True, coef=coef)
    ref = R.pairwise(y, a, coef, 0.0, logistic=True, ez=np.zeros(a.shape[0]))
    assert np.isfinite(item).all() and np.isfinite(r).all()
    _hold("pairwise_sums logistic", f"item sums [exact {kind}]", item, ref["item"], ref["e_item"] + 2 * U * np.abs(ref["item"]) + 1e-300)
    _hold("pairwise_sums logistic", f"r [exact {kind}]", r, ref["r"], ref["e_r"] + U * ref["abs_r"] + U * np.abs(ref["r"]) + 1e-300)


@pytest.mark.parametrize("kind", ["kink", "one_pos", "equal", "soft", "soft_no_positive"])
def test_exact_family_through_the_engine(kind):
    """the same items as rows a_i e_0 under w = e_0 (|w| = 1: the norm regulariser and its gradient vanish):
    parts[3] and the gradient are exact sums -- bit for bit where coef / max_inv is exact (kink, one_pos), to the
    bound otherwise.  One labelled class (`equal`) or no target equal to 1 (`soft_no_positive`) switches the label
    loss off: exactly 0, as multi_reg.py:107 has it."""
    from seesaw_amd import _lib
    from seesaw_amd.feedback import FeedbackEngine
    f = R.family_exact("soft" if kind == "soft_no_positive" else kind)
    y = f["y"].copy()
    if kind == "soft_no_positive":
        y[y == 1.0] = 0.5
    n = y.shape[0]
    X = np.zeros((n, 4), np.float32)
    X[:, 0] = f["a"]
    w = np.array([1, 0, 0, 0], np.float32)
    eng = FeedbackEngine(4)
    eng.set_data(X, center=False)
    eng.set_targets(y, f["sw"])
    eng.set_query(w)
    for lt in ("pairwise_rank_loss", "pairwise_logistic_loss"):
        obj = _lib.FbObjective(kind=_lib.SSW_FB_MULTIREG, loss_type=LOSS_CODE[lt], fit_intercept=0, reg_kind=0, pos_weight=-1.0,
                               reg_weight=0.0, margin=f["margin"], reg_norm_lambda=100.0, reg_data_lambda=0.0,
                               reg_query_lambda=0.0)
        loss, grad, parts = eng.lossgrad(obj, w)
        ref = R.multireg(w, X, y, f["sw"], w, None, loss_type=lt, margin=f["margin"], l_norm=100.0, ez_of=lambda a: 0 * a)
        print(f"  exact {kind} {lt}: label loss {parts[3]} vs {ref['parts'][3]}, gradient {grad[0]} vs {ref['grad'][0]}")
        assert ref["active"] == (kind in ("kink", "one_pos", "soft"))
        assert parts[0] == 0.0 and parts[1] == 0.0 and parts[2] == 0.0 and not grad[1:].any()
        if not ref["active"]:
            assert loss == 0.0 and parts[3] == 0.0 and grad[0] == 0.0
        elif lt == "pairwise_rank_loss" and kind in ("kink", "one_pos"):
            assert float(parts[3]) == ref["parts"][3] and float(loss) == ref["loss"] and float(grad[0]) == ref["grad"][0]
        else:
            e_loss, _, e_grad, e_parts = _one_output_bounds(ref, X, 4, False, dict(l_norm=100.0, l_query=0.0))
            _hold("multireg exact", f"label loss [{kind} {lt}]", parts[3], ref["parts"][3], e_parts[3])
            _hold("multireg exact", f"gradient [{kind} {lt}]", grad, ref["grad"], e_grad + 1e-300)
    eng.close()


# ---- the two-output objective --------------------------------------------------------------------------
def _two_output_bounds(f, ref):
    """-> (e_loss, e_parts [5], e_grad [2, dim]); the construction of the module docstring, term by term"""
    Xc, ys, dim, l_norm, l_query = np.asarray(f["Xc"], np.float64), np.asarray(f["ys"], np.float64), f["dim"], f["l_norm"], f["l_query"]
    n = Xc.shape[0]
    aX = np.abs(Xc)
    q = np.asarray(f["qhat"], np.float64)
    e_nw = (dim / 2 + 4) * U                                          # relative, rows of W over their norm
    e_den = (dim / 2 + 2) * U                                         # relative, the norm itself
    z, s, near, sp, lse = ref["z"], ref["s"], ref["near"], ref["sp"], ref["lse"]
    lab = near > 0
    ez = ((dim + 1) * U + e_nw) * ref["absxw"]                        # [n, 2]
    sg, sm = R.sigmoid(z), np.exp(z - lse[:, None])
    # per-row losses
    mag_v = (np.abs((1.0 - ys) * z) + np.abs(np.minimum(z, 0.0)) + sp).sum(axis=1)
    e_vert = ez.sum(axis=1) + 8 * U * mag_v
    mag_h = np.where(lab, (ys * (np.abs(z) + np.abs(lse)[:, None])).sum(axis=1), 0.0)
    e_hor = np.where(lab, near * ez.sum(axis=1) + 12 * U * mag_h, 0.0)
    e_iv = s * (e_vert + 2 * U * np.abs(ref["vert"]))
    e_ih = s * (e_hor + 2 * U * np.abs(ref["hor"]))
    g_items = _gamma((n + 1023) // 1024 + 10)
    vsum, hsum = ref["parts"][3], ref["parts"][4]
    e_vsum = e_iv.sum() + g_items * float(s @ np.abs(ref["vert"])) + U * abs(vsum)
    e_hsum = e_ih.sum() + g_items * float(s @ np.abs(ref["hor"])) + U * abs(hsum)
    # d loss / d logit
    nr = np.where(lab, near, 0.0)[:, None]
    e_r = s[:, None] * (0.25 * ez + nr / 4.0 * ez.sum(axis=1)[:, None] + 8 * U * (sg + ys)
                        + nr * sm * (4 * U * (np.abs(z) + np.abs(lse)[:, None]) + 8 * U) + 4 * U * (nr * sm + ys)) \
        + 2 * U * np.abs(ref["r"])
    m = min(n, 32) + (n + 31) // 32 + 2
    g = ref["g"]                                                      # [2, dim]
    e_g = (aX.T @ e_r).T + _gamma(m) * (aX.T @ np.abs(ref["r"])).T    # [2, dim]
    hq = 0.5 * l_query * np.abs(q)[None, :]
    e_G = e_g + 2 * U * (np.abs(g) + hq)
    nw, G, dotg, nrm, radial = ref["nw"], ref["G"], ref["dotg"], ref["nrm"], ref["radial"]
    anw = np.abs(nw)
    mag_dot = (anw * (np.abs(g) + hq)).sum(axis=1)
    e_dotg = (anw * e_G).sum(axis=1) + ((dim + 2) * U + e_nw) * mag_dot
    den = np.maximum(nrm, R.EPS_NORMALIZE)
    lg = np.log(nrm)
    e_lg = e_den + 4 * U * np.abs(lg) + U
    e_sinh = np.cosh(lg) * e_lg + 4 * U * np.abs(np.sinh(lg))
    e_radial = l_norm * (e_sinh / den + np.abs(np.sinh(lg)) / den * (e_den + 2 * U))
    proj = anw * np.abs(dotg)[:, None]
    e_grad = (e_G + anw * e_dotg[:, None] + (e_nw + 2 * U) * proj + 2 * U * (np.abs(G) + proj)) / den[:, None] \
        + (e_den + 2 * U) * (np.abs(G) + proj) / den[:, None] + e_radial[:, None] * anw \
        + (e_nw + 2 * U) * np.abs(radial)[:, None] * anw + U * np.abs(ref["grad"])
    # regularisers
    e_norm = l_norm * float((np.abs(np.sinh(lg)) * e_lg + 4 * U * np.cosh(lg) + U).sum()) + U * abs(ref["parts"][0])
    nq_mag = (anw * np.abs(q)[None, :]).sum(axis=1)
    e_lq = l_query / 2.0 * ((dim + 1) * U + e_nw) * nq_mag + 3 * U * l_query * (1.0 + nq_mag) / 2.0
    e_parts = np.array([e_norm, e_lq[0], e_lq[1], e_vsum, e_hsum])
    e_loss = e_parts.sum() + 4 * U * np.abs(ref["parts"]).sum()
    return e_loss, e_parts, e_grad


def _two_engine(f):
    from seesaw_amd.feedback import FeedbackEngine
    eng = FeedbackEngine(f["dim"])
    eng.set_data(f["X"], center=False)
    eng.set_targets2(f["ys"], f["sw"])
    eng.set_query(f["q"])
    return eng


def _hold_two(family, f, eng):
    ref = f["ref"]
    e_loss, e_parts, e_grad = _two_output_bounds(f, ref)
    for name in ("lossgrad2", "lossgrad2_dev"):
        loss, grad, parts = getattr(eng, name)(f["W"], f["l_norm"], f["l_query"])
        tag = f"{name} n={f['n']} dim={f['dim']}"
        _hold(family, f"loss [{tag}]", loss, ref["loss"], e_loss)
        _hold(family, f"parts [{tag}]", parts, ref["parts"], e_parts)
        _hold(family, f"gradient [{tag}]", grad, ref["grad"], e_grad)


_TWO_IDS = lambda k: "n%d-dim%d" % R.TWO_OUTPUT_CASES[k]  # noqa: E731


@pytest.mark.parametrize("k", range(len(R.TWO_OUTPUT_CASES)), ids=_TWO_IDS)
def test_two_output_saturated(k):
    """both evaluations (host tail and all-device) at logits spanning +-80: loss, the five parts, every gradient entry"""
    f = R.two_output_case(k, R.SPAN_TWO)
    eng = _two_engine(f)
    _hold_two("two-output saturated", f, eng)
    eng.close()


@pytest.mark.parametrize("k", range(len(R.TWO_OUTPUT_CASES)), ids=_TWO_IDS)
def test_two_output_mild_control(k):
    f = R.two_output_case(k, R.SPAN_MILD)
    eng = _two_engine(f)
    _hold_two("two-output mild", f, eng)
    eng.close()


def test_two_output_refuses_dim_516_by_name():
    from seesaw_amd import _lib
    from seesaw_amd.feedback import FeedbackEngine
    eng = FeedbackEngine(516)
    eng.set_data(np.zeros((3, 516), np.float32), center=False)
    eng.set_query(np.ones(516, np.float32))
    with pytest.raises(_lib.SeesawHipError, match="dim <= 512"):
        eng.set_targets2(np.zeros((3, 2), np.float32), None)
    for name in ("lossgrad2", "lossgrad2_dev"):
        with pytest.raises(_lib.SeesawHipError, match="dim <= 512"):
            getattr(eng, name)(np.ones((2, 516), np.float32), 1.0, 1.0)
    with pytest.raises(_lib.SeesawHipError, match="dim <= 512"):
        eng.fit2_dev(np.ones((2, 516), np.float32), 1.0, 1.0, 3)
    eng.close()


# ---- the fits from saturated starts -------------------------------------------------------------------------
def _fit_both_drivers(fit):
    """the one-launch fit and the host-driven one (SSW_FB_HOST_DRIVER) of the same call"""
    assert "SSW_FB_HOST_DRIVER" not in os.environ
    w_dev, info_dev = fit()
    os.environ["SSW_FB_HOST_DRIVER"] = "1"
    try:
        w_host, info_host = fit()
    finally:
        del os.environ["SSW_FB_HOST_DRIVER"]
    assert info_dev.pop("on_device") is True and info_host.pop("on_device") is False
    return (w_dev, info_dev), (w_host, info_host)


def _hold_fit(family, tag, fit, n, loss_at, bound_at, w0):
    """both drivers bit for bit where the one-launch fit serves (n <= 1024); the reported loss against the f64 loss at
    the returned weights (module docstring); the f64 loss not above the f64 loss at the start"""
    if n <= 1024:
        (w, info), (wh, ih) = _fit_both_drivers(fit)
        assert info == ih, (tag, info, ih)
        assert np.array_equal(w.view(np.uint32), wh.view(np.uint32)), (tag, np.abs(w - wh).max())
    else:
        w, info = fit()
        assert info.pop("on_device") is False
    assert np.isfinite(w).all() and info["func_evals"] >= 1
    ref_end, ref_start = loss_at(w), loss_at(w0)
    print(f"  {family} fit [{tag}]: {info}, f64 loss {ref_start['loss']:.9g} -> {ref_end['loss']:.9g}")
    _hold(family, f"reported loss [{tag}]", info["loss"], ref_end["loss"], bound_at(ref_end))
    assert ref_end["loss"] <= ref_start["loss"], (tag, ref_end["loss"], ref_start["loss"])
    return info


@pytest.mark.parametrize("k", [0, 1, 2, 3, 4, 5, 6, 13], ids=lambda k: "n%d-dim%d-%s-b%d" % R.LOGREG_CASES[k][:4])
def test_logreg_fit_from_a_saturated_start(k):
    f = R.logreg_case(k, R.SPAN_SAT)
    eng, obj = _logreg_engine(f)
    info = _hold_fit("logreg saturated", f"n={f['n']} dim={f['dim']} {f['reg']}", lambda: eng.fit(obj, f["w"], 15), f["n"],
                     lambda w: R.logreg_at(f, w),
                     lambda ref: _one_output_bounds(ref, f["Xc"], f["dim"], bool(f["icpt"]))[0], f["w"])
    assert info["n_iter"] >= 1 or f["n"] == 1   # one saturated row with y = 1: the gradient is below tolerance_grad
    eng.close()


@pytest.mark.parametrize("k", [0, 2, 4, 5, 6, 7], ids=_CE_IDS)
def test_multireg_ce_fit_from_a_saturated_start(k):
    f = R.multireg_ce_case(k, R.SPAN_SAT)
    eng, obj = _multireg_engine(f)
    _hold_fit("multireg ce saturated", f"ce n={f['n']} dim={f['dim']}", lambda: eng.fit(obj, f["w"], 15), f["n"],
              lambda w: R.multireg_at(f, w),
              lambda ref: _one_output_bounds(ref, f["Xc"], f["dim"], False, f["kw"])[0], f["w"])
    eng.close()


@pytest.mark.parametrize("k", [1, 2, 3, 7, 8], ids=_PAIR_IDS)
def test_multireg_pairwise_fit_from_a_saturated_start(k):
    f = R.multireg_pair_case(k, ez_of=ez_of(R.MULTIREG_PAIR_CASES[k][1]))
    eng, obj = _multireg_engine(f)
    fam = "multireg hinge saturated" if f["kw"]["loss_type"] == "pairwise_rank_loss" else "multireg logistic saturated"
    _hold_fit(fam, f"{f['kw']['loss_type']} n={f['n']} dim={f['dim']}", lambda: eng.fit(obj, f["w"], 10),
              f["n"], lambda w: R.multireg_at(f, w),
              lambda ref: _one_output_bounds(ref, f["Xc"], f["dim"], False, f["kw"])[0], f["w"])
    eng.close()


@pytest.mark.parametrize("k", range(len(R.TWO_OUTPUT_CASES)), ids=_TWO_IDS)
def test_two_output_fit_from_a_saturated_start(k):
    f = R.two_output_case(k, R.SPAN_TWO)
    eng = _two_engine(f)
    _hold_fit("two-output saturated", f"n={f['n']} dim={f['dim']}",
              lambda: eng.fit2_dev(f["W"], f["l_norm"], f["l_query"], 12), f["n"],
              lambda W: R.two_output_at(f, W), lambda ref: _two_output_bounds(f, ref)[0], f["W"])
    eng.close()

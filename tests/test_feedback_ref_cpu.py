"""Pins tests/_fb_ref.py -- the numpy float64 restatement tests/test_feedback_f64_gpu.py judges the feedback engine
by -- before anything is judged by it:

  * against oracle/feedback_oracle.py (logreg_loss, multireg_loss, multiregneg_loss) evaluated in float64 with
    autograd, on mild seeded inputs, every objective and every regulariser kind: loss and gradient to 1e-12 relative.
    The oracle casts a few tensors with `.float()` and builds `torch.tensor([pos_weight])`; for this comparison
    `.float()` is made to return float64 and the pos_weights are f32-exact, so the oracle is float64 throughout;
  * its analytic gradient against a central finite difference of its own float64 loss on the smooth objectives, the
    saturated family included;
  * the conditions the GPU input families must satisfy, from the reference alone, on exactly the GPU cases."""
import numpy as np
import pytest

import _fb_ref as R

REL = 1e-12


@pytest.fixture()
def f64_oracle(monkeypatch):
    import torch
    from oracle import feedback_oracle as fo
    monkeypatch.setattr(torch.Tensor, "float", torch.Tensor.double)
    return fo, torch


def _mild(n, dim, seed, intercept=False):
    f = R.family_logits(n, dim, seed, R.SPAN_MILD, center=True, intercept=intercept)
    f["qhat"] = R.qhat_f32(f["q"])
    return f


def _close(a, b, what):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    err = np.abs(a - b).max()
    assert err <= REL * max(1.0, np.abs(b).max()), (what, err, np.abs(b).max())


@pytest.mark.parametrize("reg_kind", ["none", "vector", "norm", "norm1"])
@pytest.mark.parametrize("intercept", [0, 1])
@pytest.mark.parametrize("pos_weight", [0.25, 1.0, 7.0])
def test_logreg_is_the_oracle_in_f64(f64_oracle, reg_kind, intercept, pos_weight):
    fo, torch = f64_oracle
    n, dim = 57, 24
    f = _mild(n, dim, 11 + intercept, bool(intercept))
    w = torch.tensor(f["w"][:dim].astype(np.float64), requires_grad=True)
    b = torch.tensor(f["w"][dim:].astype(np.float64), requires_grad=True) if intercept else None
    loss = fo.logreg_loss(w, b, torch.from_numpy(f["Xc"].astype(np.float64)), torch.from_numpy(f["y"].astype(np.float64)),
                          torch.from_numpy(f["sw"].astype(np.float64)).reshape(-1, 1), pos_weight, 0.7 / n,
                          torch.from_numpy(f["qhat"].astype(np.float64)), reg_kind=reg_kind)
    loss.backward()
    ref = R.logreg(f["w"][:dim], f["w"][dim] if intercept else None, f["Xc"], f["y"], f["sw"], pos_weight, 0.7 / n,
                   f["qhat"], reg_kind)
    _close(ref["loss"], loss.item(), "loss")
    g = w.grad.numpy() if not intercept else np.concatenate([w.grad.numpy(), b.grad.numpy()])
    _close(ref["grad"], g, "grad")


@pytest.mark.parametrize("loss_type", ["ce_loss", "pairwise_rank_loss", "pairwise_logistic_loss"])
@pytest.mark.parametrize("pos_weight", [-1.0, 0.25, 7.0])
def test_multireg_is_the_oracle_in_f64(f64_oracle, loss_type, pos_weight):
    fo, torch = f64_oracle
    n, dim = 61, 20
    f = _mild(n, dim, 23)
    rng = np.random.default_rng(5)
    A = rng.standard_normal((dim, dim)) * 0.1
    xlx = (A @ A.T + 0.05 * rng.standard_normal((dim, dim))).astype(np.float32)  # not symmetric: (M + M') w matters
    kw = dict(loss_type=loss_type, margin=0.2, l_norm=100.0, l_data=0.5, l_query=3.0)
    w = torch.tensor(f["w"].astype(np.float64), requires_grad=True)
    loss, parts = fo.multireg_loss(w, torch.from_numpy(f["Xc"].astype(np.float64)),
                                   torch.from_numpy(f["y"].astype(np.float64)),
                                   torch.from_numpy(f["sw"].astype(np.float64)),
                                   torch.from_numpy(f["qhat"].astype(np.float64)),
                                   torch.from_numpy(xlx.astype(np.float64)),
                                   pos_weight="balanced" if pos_weight < 0 else pos_weight, **kw)
    loss.backward()
    ref = R.multireg(f["w"], f["Xc"], f["y"], f["sw"], f["qhat"], xlx, pos_weight=pos_weight, **kw)
    _close(ref["loss"], loss.item(), "loss")
    _close(ref["parts"], [float(p.detach()) for p in parts], "parts")
    _close(ref["grad"], w.grad.numpy(), "grad")
    assert ref["active"] and ref["parts"][3] > 0


def test_multireg_pairwise_is_off_until_both_classes_are_labelled(f64_oracle):
    """one labelled class: the oracle's label loss is identically 0 (multi_reg.py:107); so is the restatement's"""
    fo, torch = f64_oracle
    f = _mild(9, 8, 3)
    for y in (np.ones(9), np.zeros(9), np.full(9, 0.5)):
        for lt in ("pairwise_rank_loss", "pairwise_logistic_loss"):
            ref = R.multireg(f["w"], f["Xc"], y, f["sw"], f["qhat"], None, loss_type=lt, l_norm=1.0, l_query=1.0)
            w = torch.tensor(f["w"].astype(np.float64), requires_grad=True)
            loss, parts = fo.multireg_loss(w, torch.from_numpy(f["Xc"].astype(np.float64)), torch.from_numpy(y),
                                           torch.from_numpy(f["sw"].astype(np.float64)),
                                           torch.from_numpy(f["qhat"].astype(np.float64)),
                                           torch.zeros(8, 8, dtype=torch.float64), loss_type=lt, margin=0.2, l_norm=1.0,
                                           l_data=0.0, l_query=1.0)
            loss.backward()
            assert not ref["active"] and ref["parts"][3] == 0.0 and float(parts[3].detach()) == 0.0
            _close(ref["loss"], loss.item(), "loss")
            _close(ref["grad"], w.grad.numpy(), "grad")


@pytest.mark.parametrize("n,dim", [(1, 4), (40, 12)])
def test_multiregneg_is_the_oracle_in_f64(f64_oracle, n, dim):
    fo, torch = f64_oracle
    f = R.family_two_output(n, dim, 31, R.SPAN_MILD)
    qhat = R.qhat_f32(f["q"])
    W = torch.tensor(f["W"].astype(np.float64), requires_grad=True)
    loss, parts = fo.multiregneg_loss(W, torch.from_numpy(f["Xc"].astype(np.float64)),
                                      torch.from_numpy(f["ys"].astype(np.float64)),
                                      torch.from_numpy(f["sw"].astype(np.float64)),
                                      torch.from_numpy(qhat.astype(np.float64)), l_norm=10.0, l_query=3.0)
    loss.backward()
    ref = R.multiregneg(f["W"], f["Xc"], f["ys"], f["sw"], qhat, l_norm=10.0, l_query=3.0)
    _close(ref["loss"], loss.item(), "loss")
    _close(ref["parts"], [float(p.detach()) for p in parts], "parts")
    _close(ref["grad"], W.grad.numpy(), "grad")


# ---- analytic gradient against finite differences of the restatement's own loss ---------------------------
def _fd_check(fn, x, what, n_dirs=6, h=1e-6):
    """central differences along random unit directions and the first / last coordinate; the loss is smooth and f64,
    so the difference quotient is good to h^2 |f'''| + 2^-52 |f| / h"""
    x = np.asarray(x, np.float64)
    rng = np.random.default_rng(0)
    base = fn(x)
    g = np.asarray(base["grad"], np.float64).reshape(-1)
    dirs = [rng.standard_normal(x.size) for _ in range(n_dirs)]
    dirs += [np.eye(1, x.size, 0).reshape(-1), np.eye(1, x.size, x.size - 1).reshape(-1)]
    scale = max(1.0, np.abs(x).max())
    for d in dirs:
        d = (d / np.linalg.norm(d)).reshape(x.shape)
        step = h * scale
        fd = (fn(x + step * d)["loss"] - fn(x - step * d)["loss"]) / (2 * step)
        an = float(g @ d.reshape(-1))
        tol = 1e-6 * max(1.0, abs(an)) + 4 * 2.0 ** -52 * abs(base["loss"]) / step
        assert abs(fd - an) <= tol, (what, fd, an, tol)


@pytest.mark.parametrize("span", [R.SPAN_MILD, R.SPAN_MID, R.SPAN_SAT])
@pytest.mark.parametrize("reg_kind,intercept", [("none", 1), ("vector", 0), ("norm", 1), ("norm1", 0)])
def test_logreg_gradient_is_the_finite_difference(span, reg_kind, intercept):
    n, dim = 97, 16
    f = R.family_logits(n, dim, 41, span, center=True, intercept=bool(intercept))
    qhat = R.qhat_f32(f["q"])
    fn = lambda p: R.logreg(p[:dim], p[dim] if intercept else None, f["Xc"], f["y"], f["sw"], 7.0, 1.0 / n, qhat, reg_kind)
    _fd_check(fn, f["w"], (span, reg_kind))


@pytest.mark.parametrize("span", [R.SPAN_MILD, R.SPAN_PAIR_LOGISTIC, R.SPAN_SAT])
@pytest.mark.parametrize("loss_type", ["ce_loss", "pairwise_logistic_loss"])
def test_multireg_gradient_is_the_finite_difference(span, loss_type):
    n, dim = 83, 12
    f = R.family_logits(n, dim, 43, span, center=True)
    qhat = R.qhat_f32(f["q"])
    rng = np.random.default_rng(6)
    xlx = (0.1 * rng.standard_normal((dim, dim))).astype(np.float32)
    fn = lambda p: R.multireg(p, f["Xc"], f["y"], f["sw"], qhat, xlx, loss_type=loss_type, l_norm=0.01, l_data=0.25,
                              l_query=3.0)
    _fd_check(fn, f["w"], (span, loss_type))


@pytest.mark.parametrize("span", [R.SPAN_MILD, R.SPAN_TWO])
def test_multiregneg_gradient_is_the_finite_difference(span):
    f = R.family_two_output(77, 12, 47, span)
    qhat = R.qhat_f32(f["q"])
    fn = lambda P: R.multiregneg(P.reshape(2, -1), f["Xc"], f["ys"], f["sw"], qhat, l_norm=2.0, l_query=3.0)
    _fd_check(fn, f["W"].astype(np.float64), span)


def test_hinge_gradient_is_the_finite_difference_away_from_the_kinks():
    """piecewise linear: exact wherever no pair sits within the step of its kink"""
    f = R.family_logits(40, 8, 53, R.SPAN_SAT, center=True)
    qhat = R.qhat_f32(f["q"])
    fn = lambda p: R.multireg(p, f["Xc"], f["y"], f["sw"], qhat, None, loss_type="pairwise_rank_loss", margin=0.2,
                              l_norm=0.01, l_query=3.0)
    assert fn(f["w"].astype(np.float64))["pair"]["kinks"] == 0
    _fd_check(fn, f["w"], "hinge", h=1e-9)


# ---- the conditions the GPU input families must satisfy -----------------------------------------------------
def _saturated(z):
    z = np.abs(np.asarray(z)).reshape(-1)
    return (z >= 30).mean(), (z >= 80).mean()


def test_saturated_one_output_families_are_saturated():
    """at least a third of the logits with |z| >= 30 and 5 % with |z| >= 80, every reference loss finite -- on every
    logistic and BCE-multireg case the GPU module runs; the mild control stays within |z| <= 1.1"""
    for k, case in enumerate(R.LOGREG_CASES):
        ref = R.logreg_case(k, R.SPAN_SAT)["ref"]
        a, b = _saturated(ref["z"])
        assert a >= 1 / 3 and b >= 0.05, (case, a, b)
        assert np.isfinite(ref["loss"]) and np.isfinite(ref["grad"]).all()
        assert np.abs(R.logreg_case(k, R.SPAN_MILD)["ref"]["z"]).max() <= 1.1, case
    for k, case in enumerate(R.MULTIREG_CE_CASES):
        ref = R.multireg_ce_case(k, R.SPAN_SAT)["ref"]
        a, b = _saturated(ref["z"])
        assert a >= 1 / 3 and b >= 0.05, (case, a, b)
        assert np.isfinite(ref["loss"]) and np.isfinite(ref["grad"]).all()
        assert np.abs(R.multireg_ce_case(k, R.SPAN_MILD)["ref"]["z"]).max() <= 1.1, case


def test_pairwise_families_stay_where_the_reference_is_finite():
    """pairwise logistic: max |z_i - z_j| <= 80, so the reference's own f32 log(1 + exp(.)) stays finite; the hinge
    family is the saturated one; every loss finite and the label loss on"""
    for k, (n, dim, lt, center) in enumerate(R.MULTIREG_PAIR_CASES):
        ref = R.multireg_pair_case(k)["ref"]
        assert ref["active"] and np.isfinite(ref["loss"]) and np.isfinite(ref["grad"]).all()
        spread = ref["z"].max() - ref["z"].min()
        if lt == "pairwise_logistic_loss":
            assert spread <= 80.0, (n, dim, spread)
            assert np.isfinite(np.log(np.float32(1) + np.exp(np.float32(spread))))
        else:
            a, b = _saturated(ref["z"])
            assert a >= 1 / 3 and (b >= 0.05 or n < 10), (n, dim, a, b)


def test_two_output_family_is_saturated_in_f32_range():
    """the f32 form: |z| <= 80 (one part in 10^6 of slack for the rows' quantisation), a third of the logits with
    |z| >= 30 and 5 % within a tenth of the top"""
    for k, case in enumerate(R.TWO_OUTPUT_CASES):
        ref = R.two_output_case(k, R.SPAN_TWO)["ref"]
        z = np.abs(ref["z"]).reshape(-1)
        assert z.max() <= R.SPAN_TWO * (1 + 1e-6)
        assert (z >= 30).mean() >= 1 / 3 and (z >= 0.9 * R.SPAN_TWO).mean() >= 0.05, case
        assert np.isfinite(ref["loss"]) and np.isfinite(ref["grad"]).all()


@pytest.mark.parametrize("kind", ["kink", "soft", "one_pos", "equal"])
def test_exact_family_is_exact_and_sits_on_the_kink(kind):
    """z = a exactly (multiples of 1/8); pairs with margin - t s == 0 exactly exist, and pairs an eighth inside and
    outside; every sum of the hinge is a small dyadic number, so f64 and f32 hold it exactly"""
    f = R.family_exact(kind)
    a, y = f["a"].astype(np.float64), f["y"].astype(np.float64)
    assert np.array_equal(a * 8, np.round(a * 8))
    cnt = np.array([(y != v).sum() for v in y], dtype=np.float64)
    ref = R.pairwise(y, a, cnt * f["sw"], f["margin"], logistic=False)
    t = np.sign(y[:, None] - y[None, :])
    h = f["margin"] - t * (a[:, None] - a[None, :])
    if kind == "equal":
        assert ref["kinks"] == 0 and not ref["item"].any() and not ref["r"].any() and not cnt.any()
        return
    assert ref["kinks"] > 0
    assert ((t != 0) & (h == 0.125)).any() and ((t != 0) & (h < 0)).any()
    if kind != "one_pos":
        assert ((t != 0) & (h == -0.125)).any()
    assert np.array_equal(ref["c"], f["sw"].astype(np.float64))           # coef / max_inv is exact
    assert np.array_equal(ref["item"], ref["item"].astype(np.float32))    # one rounding changes nothing
    assert np.array_equal(ref["r"], ref["r"].astype(np.float32))
    # a strict h > 0 would lose exactly the kink pairs' gradient
    strict = np.where((t != 0) & (h > 0), -t, 0.0)
    r_strict = -ref["c"] * strict.sum(axis=0) + strict @ ref["c"]
    assert not np.array_equal(r_strict, ref["r"])

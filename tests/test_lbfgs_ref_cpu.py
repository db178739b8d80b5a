"""CPU: the restatement of the feedback fit's driver (tests/_lbfgs_ref.py) is anchored to torch.optim.LBFGS, its
wave-form dot to an exact rational sum, and every input of tests/test_fit_driver_gpu.py is shown to reach the branch
it is named for -- by the restatement alone, over tests/_fb_ref.py's f64 objectives, before a GPU is asked to.

RESTATEMENT AGAINST TORCH.  Both run the same closure: f32 parameters, the objectives of oracle/feedback_oracle.py
evaluated in f64, the gradient rounded to f32 by autograd.  The restatement uses torch.dot (`plain_dot`) and, like the
installed torch, max_ls = max_eval - current_evals (`ls_budget=True`; the project's drivers keep max_ls = 25, and
the same fits run with that too and must not change, i.e. the cap binds in neither form).  n_iter and func_evals must
be EQUAL.  The weights agree to rounding only: torch keeps 1 / y.s, H_diag and the alphas as f32 tensors, the
restatement (as feedback_lbfgs.hip documents) as f64 scalars.  Measured on this project's CPU runner, largest
|w_restatement - w_torch| over the five fits: 5.96e-8 (multireg ce, |w| ~ 1; the three logistic fits: 7.5e-9, 1.9e-9,
0); asserted: four times that, 2.4e-7 (the margin covers BLAS's thread-dependent order in torch.dot).  Every fit
prints its own figure.  The fits converge (6 to 16 iterations, ended by |dloss|, g.d or the gradient) and stay clear
of max_eval: a fit that is cut off while it still moves -- the pairwise hinge needs 39 iterations here -- follows
either side's rounding onto another path, which says nothing about the restatement.
"""
from fractions import Fraction

import numpy as np
import pytest

import _fb_ref as R
import _fit_driver_cases as C
import _lbfgs_ref as L

F32 = np.float32
L_NORM, MR_ITERS = 10.0, 40
TORCH_TOL = 2.4e-7   # four times the measured 5.96e-8 (module docstring)


# ---- the restatement against torch's own optimiser --------------------------------------------------------------
def _anchor_inputs(n, dim, seed):
    import torch
    X, d = R.planted_rows(n, dim, seed)
    Xc = torch.from_numpy(R.center_f32(X)).double()
    y, sw = R.labels_mixed(n, seed + 1)
    q = R._unit(d + 0.3 * np.random.default_rng(seed + 2).standard_normal(dim) / np.sqrt(dim)).astype(F32)
    return Xc, torch.from_numpy(y).double(), torch.from_numpy(sw).double(), torch.from_numpy(R.qhat_f32(q)).double(), q


def _anchor_closures():
    """(name, loss(w f64 tensor) -> f64 scalar tensor, w0 f32, max_iter)"""
    import torch
    from oracle import feedback_oracle as O
    out = []
    for name, n, dim, reg, icpt, lam in (("logreg vector + intercept", 40, 16, "vector", 1, 1.0),
                                         ("logreg norm", 33, 64, "norm", 0, 10.0),
                                         ("logreg norm1 + intercept", 64, 32, "norm1", 1, 3.0)):
        Xc, y, sw, qh, q = _anchor_inputs(n, dim, 500 + n)

        def loss(w, Xc=Xc, y=y, sw=sw, qh=qh, dim=dim, reg=reg, icpt=icpt, lam=lam, n=n):
            return O.logreg_loss(w[:dim], w[dim:] if icpt else None, Xc, y, sw.reshape(-1, 1), 2.0, lam / n, qh, reg_kind=reg)
        out.append((name, loss, np.concatenate([q, np.zeros(icpt, F32)]).astype(F32), 20))
    for name, n, dim, lt, l_query in (("multireg ce", 48, 16, "ce_loss", 1.0),
                                      ("multireg logistic", 30, 16, "pairwise_logistic_loss", 1.0)):
        l_norm = L_NORM
        Xc, y, sw, qh, q = _anchor_inputs(n, dim, 600 + n)
        y = (y > 0.5).double()
        M = torch.zeros(dim, dim, dtype=torch.float64)

        def loss(w, Xc=Xc, y=y, sw=sw, qh=qh, M=M, lt=lt, l_query=l_query, l_norm=l_norm):
            return O.multireg_loss(w, Xc, y, sw, qh, M, loss_type=lt, margin=0.2, l_norm=l_norm, l_data=0.0, l_query=l_query)[0]
        # (multireg_loss casts the sample weights to f32 and back: both sides run the same function)
        out.append((name, loss, R.qhat_f32(q), MR_ITERS))
    return out


def test_restatement_equals_torch_lbfgs_in_iterations_and_evaluations():
    """five short, well-conditioned fits.  Measured largest |w_restatement - w_torch|: 5.96e-8; asserted: 2.4e-7 (four
    times that; module docstring)"""
    import torch
    worst = 0.0
    for name, loss_of, w0, max_iter in _anchor_closures():
        w = torch.tensor(w0, requires_grad=True)
        opt = torch.optim.LBFGS([w], max_iter=max_iter, lr=1.0, line_search_fn="strong_wolfe")

        def closure():
            opt.zero_grad()
            loss = loss_of(w.double())
            loss.backward()
            return loss
        opt.step(closure)
        state = opt.state[w]

        def ev(wn):
            wt = torch.tensor(np.asarray(wn, F32), requires_grad=True)
            loss = loss_of(wt.double())
            loss.backward()
            return float(loss.detach()), wt.grad.numpy().copy()
        x, n_iter, evals, loss, tr = L.lbfgs(ev, w0, max_iter, 1.0, dot=L.plain_dot, abs_sum64=L.plain_abs_sum64, ls_budget=True)
        diff = float(np.abs(x - w.detach().numpy()).max())
        worst = max(worst, diff)
        print(f"  {name}: torch n_iter {state['n_iter']} func_evals {state['func_evals']}, restatement {n_iter} {evals} "
              f"({tr.exit}), max |dw| {diff:.3g}")
        assert (n_iter, evals) == (state["n_iter"], state["func_evals"]), name
        assert 5 <= n_iter < max_iter and evals < max_iter * 5 // 4, (name, "not a fit, or cut off")
        assert diff <= TORCH_TOL, (name, diff)
        # the project's max_ls = 25 takes the same path: neither cap binds on these fits
        x25, it25, ev25, loss25, tr25 = L.lbfgs(ev, w0, max_iter, 1.0, dot=L.plain_dot, abs_sum64=L.plain_abs_sum64)
        assert (it25, ev25, loss25) == (n_iter, evals, loss) and np.array_equal(x25.view(np.uint32), x.view(np.uint32)), name
    print(f"  largest |w_restatement - w_torch|: {worst:.3g} (asserted {TORCH_TOL:.3g})")


def test_cubic_interpolate_equals_torchs():
    from torch.optim.lbfgs import _cubic_interpolate
    import torch
    rng = np.random.default_rng(3)
    for _ in range(200):
        x1, x2 = rng.uniform(0, 3, 2)
        f1, f2, g1, g2 = rng.standard_normal(4)
        bounds = None if rng.uniform() < 0.5 else (min(x1, x2) + 0.1, max(x1, x2) * 3)
        ref = _cubic_interpolate(x1, torch.tensor(f1), torch.tensor(g1), x2, torch.tensor(f2), torch.tensor(g2), bounds)
        assert L.cubic_interpolate(x1, f1, g1, x2, f2, g2, bounds) == float(ref)


# ---- the wave-form dot --------------------------------------------------------------------------------
def _wave_sum_literal(p):
    """the network documented above wave_sum_host (seesaw_amd/csrc/fb_math.h), written out lane by lane in f32"""
    p = [F32(v) for v in p]
    b = []
    for lane in range(64):
        s = F32(0)
        for i in range(lane, len(p), 64):
            s = F32(s + p[i])
        b.append(s)
    for s_ in (1, 2, 4, 8):
        b = [F32(b[lane] + (b[lane - s_] if (lane & 15) >= s_ else F32(0))) for lane in range(64)]
    return F32(F32(F32(b[15] + b[31]) + b[47]) + b[63])


@pytest.mark.parametrize("n", [1, 63, 64, 65, 513, 576, 1024, 1025])
def test_wave_dot_against_an_exact_rational_sum(n):
    """|wave sum - exact sum of the f32 products| <= gamma_k sum |p_i|, k = ceil(n / 64) + 6: an element passes at most
    ceil(n / 64) - 1 additions inside its lane (the first is 0 + p, exact), four in the row network and three across
    the rows, each rounding once (u = 2^-24, gamma_k = k u / (1 - k u))"""
    rng = np.random.default_rng(n)
    a = (rng.standard_normal(n) * np.exp(rng.uniform(-8, 8, n))).astype(F32)
    b = rng.standard_normal(n).astype(F32)
    p = a * b                                              # the f32 products both drivers form
    got = L.wave_dot(a, b)
    exact = sum(Fraction(float(v)) for v in p)
    k = (n + 63) // 64 + 6
    u = Fraction(1, 2 ** 24)
    bound = k * u / (1 - k * u) * sum(abs(Fraction(float(v))) for v in p)
    assert abs(Fraction(got) - exact) <= bound, (n, got, float(exact), float(bound))
    assert np.array_equal(np.asarray(L.wave_sum(p)).view(np.uint32), np.asarray(_wave_sum_literal(p)).view(np.uint32))


def test_wave_dot_keeps_the_documented_order_where_it_matters():
    """2^27 in lane 0, 1 behind it in the same lane (element 64), -2^27 in lane 1, 1 in lane 2: the lane sum 2^27 + 1
    rounds the 1 away (ulp 16) before the network cancels the large terms, so the documented order gives 1 where the
    exact sum -- and a sum in element order -- is 2"""
    p = np.zeros(65, F32)
    p[0], p[1], p[2], p[64] = 2.0 ** 27, -2.0 ** 27, 1.0, 1.0
    assert float(np.sum(p.astype(np.float64))) == 2.0
    seq = F32(0)
    for v in p:
        seq = F32(seq + v)
    assert float(seq) == 2.0
    assert float(L.wave_sum(p)) == 1.0 and float(_wave_sum_literal(p)) == 1.0
    assert L.wave_dot(p, np.ones(65, F32)) == 1.0
    # the f64 form (the first step's sum of |g|) keeps both: 2^27 + 1 is exact there
    assert float(L.wave_sum(np.abs(p).astype(np.float64), np.float64)) == 2.0 ** 28 + 2.0


# ---- the inputs reach what they are for ---------------------------------------------------------------------
def _run(c, **kw):
    return L.lbfgs(C.cpu_eval(c), C.start_vector(c), c["max_iter"], c["lr"], zero_slot=C.zero_slot(c), **kw)


@pytest.fixture(scope="module")
def wrap_runs():
    return {c["name"]: (c, _run(c)) for c in C.wrap_cases()}


@pytest.mark.parametrize("k", range(4), ids=lambda k: ("logreg-dim512", "logreg-dim768", "ce-dim512", "two-output")[k])
def test_history_wrap_inputs_turn_the_history(wrap_runs, k):
    c, (x, n_iter, evals, loss, tr) = list(wrap_runs.values())[k]
    print(f"  {c['name']}: n_iter {n_iter} func_evals {evals} loss {loss:.9g} {tr.counters()}")
    assert n_iter >= 110 and tr.evictions >= 10 and tr.history_len == L.HISTORY, (c["name"], n_iter, tr.evictions)
    assert evals <= c["max_iter"] * 5 // 4, (c["name"], evals)
    assert np.isfinite(x).all()


def test_a_shorter_history_changes_the_fit(wrap_runs):
    """what a ring of the wrong length does (FIT_HISTORY = 50 in fb_handle.h, or a lost entry): the restatement with
    history 50 leaves the path of the one with 100 at the 51st update, so a comparison of weights cannot miss it"""
    c, (x, n_iter, evals, loss, tr) = wrap_runs["wrap-logreg-n384-dim512"]
    x50, it50, ev50, loss50, tr50 = _run(c, history=50)
    assert tr50.evictions > 0 and not np.array_equal(x50.view(np.uint32), x.view(np.uint32))
    assert (it50, ev50) != (n_iter, evals) or loss50 != loss


@pytest.mark.parametrize("k", range(len(C.LINE_CASES)), ids=lambda k: C.LINE_CASES[k][0])
def test_line_search_inputs_reach_their_branches(k):
    c = C.line_cases()[k]
    assert 17 <= c["n"] <= 64
    x, n_iter, evals, loss, tr = _run(c)
    print(f"  {c['name']}: n_iter {n_iter} func_evals {evals} loss {loss:.9g} {tr.counters()}")
    assert not C.reached(tr, c["want"]), (c["name"], C.reached(tr, c["want"]), tr.counters())
    assert np.isfinite(x).all() and np.isfinite(loss)


def test_the_line_cases_cover_every_branch_the_driver_has():
    """every required branch, and the five best-effort ones, is wanted by at least one case"""
    wanted = {w for _, _, _, _, _, kw in C.LINE_CASES for w in kw["want"]}
    required = {"bracket_armijo", "bracket_wolfe", "bracket_gtd_pos", "extrapolations", "high_replaced", "low_replaced",
                "swapped", "insuf_set", "forced_steps", "exit:max_iter", "exit:max_eval", "exit:dloss", "exit:initial_opt"}
    best_effort = {"max_ls_exhausted", "skipped_updates", "zoom_width", "exit:gtd", "exit:dm"}
    assert not (required | best_effort) - wanted, (required | best_effort) - wanted
    by_lr = lambda lo, hi: {w for _, _, _, _, _, kw in C.LINE_CASES if lo <= kw["lr"] <= hi for w in kw["want"]}  # noqa: E731
    assert "extrapolations" in by_lr(1e-3, 1e-3)
    assert {"high_replaced", "low_replaced", "swapped"} <= by_lr(10.0, 100.0)


def test_big_and_short_cases_are_what_they_are_named():
    c = C.big_case()
    x, n_iter, evals, loss, tr = _run(c)
    assert c["n"] > 1024 and n_iter >= 5 and not C.reached(tr, c["want"])
    for obj in ("logreg", "ce", "two"):
        s = C.short_case(obj, 40, 512, 9)
        xs, it_s, ev_s, loss_s, tr_s = _run(s)
        assert 1 <= it_s <= 12 and tr_s.evictions == 0 and np.isfinite(xs).all()

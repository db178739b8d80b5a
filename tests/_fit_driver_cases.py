"""The inputs tests/test_fit_driver_gpu.py drives the feedback fit's two drivers with, and the CPU evaluations
tests/test_lbfgs_ref_cpu.py runs the restatement (tests/_lbfgs_ref.py) over to show that every case reaches the
branches it is named for before a GPU is asked to.  (A helper module, not a conftest.)

A case is a dict: the objective ("logreg", "ce", "hinge", "logistic" -- the last three are RegModule's label losses --
or "two" for the two-output fit), the rows as the engine receives them (center=False, multiples of 2^-20), targets,
sample weights, the query, the start vector, max_iter and lr, and `want`: the trace counters that must be non-zero
(`exit` names the outer exit).  Everything is seeded and built from numpy alone.
"""
from __future__ import annotations

import numpy as np

import _fb_ref as R

F32 = np.float32
REG_CODE = {"none": 0, "vector": 1, "norm": 2, "norm1": 3}
LOSS_TYPE = {"ce": "ce_loss", "hinge": "pairwise_rank_loss", "logistic": "pairwise_logistic_loss"}


def _finish(c):
    c["n"], c["dim"] = c["X"].shape
    c["qhat"] = R.qhat_f32(c["q"])
    if c["objective"] == "logreg":
        c["P"] = c["dim"] + c["icpt"]
        c["reg_weight"] = R.f32(c["reg_lambda"] / c["n"])
        c["pos_weight"] = R.f32(c["pos_weight"])
    elif c["objective"] == "two":
        c["P"] = 2 * c["dim"]
    else:
        c["P"] = c["dim"]
        c["kw"] = dict(loss_type=LOSS_TYPE[c["objective"]], margin=R.f32(c.get("margin", 0.2)), l_norm=R.f32(c["l_norm"]),
                       l_data=R.f32(0.0), l_query=R.f32(c["l_query"]), pos_weight=R.f32(c.get("pos_weight", -1.0)))
    c["w0"] = np.asarray(c["w0"], F32).reshape(-1)
    assert c["w0"].shape[0] == c["P"]
    return c


# ---- the history wrap: fits of more than 110 iterations ------------------------------------------------------
def _spread_rows(n, dim, seed):
    """rows whose column scales spread over e^-6 .. 1, labels drawn from a planted logistic model"""
    rng = np.random.default_rng(seed)
    scales = np.exp(np.linspace(-6.0, 0.0, dim))
    X = R.quantise(rng.standard_normal((n, dim)) * scales[None, :])
    w_true = rng.standard_normal(dim) / scales / np.sqrt(dim) * 2.0
    y = (rng.uniform(size=n) < R.sigmoid(X.astype(np.float64) @ w_true)).astype(F32)
    q = R._unit(np.random.default_rng(seed + 1).standard_normal(dim)).astype(F32)
    return X, y, q


def wrap_logreg(n, dim):
    X, y, q = _spread_rows(n, dim, 5)
    return _finish(dict(name=f"wrap-logreg-n{n}-dim{dim}", objective="logreg", X=X, y=y, sw=np.ones(n, F32), q=q, icpt=1,
                        reg="norm", reg_lambda=1e-6, pos_weight=1.0, w0=np.zeros(dim + 1, F32), max_iter=200, lr=1.0,
                        want=("evictions",)))


def wrap_ce(n, dim):
    X, y, q = _spread_rows(n, dim, 5)
    return _finish(dict(name=f"wrap-ce-n{n}-dim{dim}", objective="ce", X=X, y=y, sw=np.ones(n, F32), q=q, l_norm=0.01,
                        l_query=0.0, pos_weight=1.0, w0=R.qhat_f32(q), max_iter=200, lr=1.0, want=("evictions",)))


def wrap_two(n, dim, row_norm=1000.0):
    """The two-output loss is an f32 total, and an f32 loss stalls L-BFGS long before 100 updates unless every
    iteration's decrease stays above 2^-24 of the loss: separable rows of norm ~1000, so that the loss falls by
    orders of magnitude for as long as the direction improves (the logits use the normalised weights)."""
    rng = np.random.default_rng(5)
    X = R.quantise(rng.standard_normal((n, dim)) * row_norm / np.sqrt(dim))
    y = (rng.uniform(size=n) < 0.5).astype(F32)
    ys = np.stack([y, 1.0 - y], axis=1).astype(F32)
    q = R._unit(rng.standard_normal(dim)).astype(F32)
    qh = R.qhat_f32(q)
    W0 = (np.stack([qh, -qh]) + 0.1 * rng.standard_normal((2, dim)) / np.sqrt(dim)).astype(F32)
    return _finish(dict(name=f"wrap-two-n{n}-dim{dim}", objective="two", X=X, ys=ys, sw=np.ones(n, F32), q=q, l_norm=1e-3,
                        l_query=0.0, w0=W0.reshape(-1), max_iter=200, lr=1.0, want=("evictions",)))


def big_case(n=1100, dim=64):
    """above the one-launch fit's 1024 rows: the host driver alone, held to the restatement"""
    X, d = R.planted_rows(n, dim, 77)
    y, sw = R.labels_mixed(n, 78)
    q = R._unit(d + 0.3 * np.random.default_rng(79).standard_normal(dim) / np.sqrt(dim)).astype(F32)
    return _finish(dict(name=f"big-logreg-n{n}-dim{dim}", objective="logreg", X=X, y=y, sw=sw, q=q, icpt=1, reg="vector",
                        reg_lambda=1.0, pos_weight=2.0, w0=np.concatenate([q, [0.0]]), max_iter=20, lr=1.0,
                        want=("bracket_wolfe",)))


# row counts: the smallest multiple of 64 at which the CPU check (tests/test_lbfgs_ref_cpu.py) reaches 110 iterations is
# 320 at dim 512 (118) and 512 at dim 768 (129); the engine rounds an evaluation differently and the GPU run must get
# there on its own path, so the next size up is used (164 and 171 iterations on the CPU)
def wrap_cases():
    return [wrap_logreg(384, 512), wrap_logreg(576, 768), wrap_ce(512, 512), wrap_two(320, 512)]


def short_case(objective, n, dim, seed, max_iter=8):
    """a short fit of the same kind, for the slots around the long one in a batch"""
    if objective == "two":
        c = wrap_two(n, dim, row_norm=4.0)
        c.update(name=f"short-two-n{n}", max_iter=max_iter, want=())
        return c
    rng = np.random.default_rng(seed)
    X = R.quantise(R._unit(rng.standard_normal((n, dim))))
    y = (np.arange(n) % 2).astype(F32)
    q = R._unit(rng.standard_normal(dim)).astype(F32)
    if objective == "logreg":
        return _finish(dict(name=f"short-logreg-n{n}", objective="logreg", X=X, y=y, sw=np.ones(n, F32), q=q, icpt=1,
                            reg="vector", reg_lambda=1.0, pos_weight=1.0, w0=np.concatenate([q, [0.0]]),
                            max_iter=max_iter, lr=1.0, want=()))
    return _finish(dict(name=f"short-{objective}-n{n}", objective=objective, X=X, y=y, sw=np.ones(n, F32), q=q, l_norm=100.0,
                        l_query=1.0, w0=R.qhat_f32(q), max_iter=max_iter, lr=1.0, want=()))


# ---- line-search cases: small fits, found by a seeded search over `line_case`'s arguments ------------------------
def line_case(name, objective, n, dim, seed, *, scale, lr, max_iter, w0_scale, want, reg="none", icpt=0, reg_lambda=0.0,
              l_norm=100.0, l_query=1.0, margin=0.2, labels="random", sw_scale=1.0, w0=None):
    rng = np.random.default_rng(seed)
    X = R.quantise(rng.standard_normal((n, dim)) * scale / np.sqrt(dim))
    if labels == "random":
        y = (rng.uniform(size=n) < 0.5).astype(F32)
        y[0], y[1] = 1.0, 0.0
    elif labels == "ties":           # few distinct rows and soft targets that repeat: the hinge sits on its kinks
        X = X[rng.integers(0, 4, n)]
        y = (rng.integers(0, 3, n) / 2.0).astype(F32)
        y[0], y[1] = 1.0, 0.0
    elif labels == "equal":          # every target the same: the label loss has no gradient
        y = np.ones(n, F32)
    elif labels == "linear":
        # degenerate on purpose: positive rows, targets of 2 and a start with every logit saturated, so that the BCE
        # (1 - y) z + softplus(-z) ~ -z falls linearly along every descent direction and no step, however long,
        # brackets a minimum or flattens the slope -- the way to max_ls extrapolations
        X = np.abs(X)
        y = np.full(n, 2.0, F32)
    else:
        raise ValueError(labels)
    q = R._unit(rng.standard_normal(dim)).astype(F32)
    sw = (sw_scale * rng.uniform(0.5, 2.0, n)).astype(F32)
    P = dim + icpt if objective == "logreg" else dim
    if w0 is not None:
        pass
    elif objective != "logreg":
        w0 = w0_scale * R.qhat_f32(q)
    elif labels != "linear":
        w0 = w0_scale * rng.standard_normal(P) / np.sqrt(dim)
    else:
        w0 = w0_scale * np.ones(P) / np.sqrt(dim)
    c = dict(name=name, objective=objective, X=X, y=y, sw=sw, q=q, w0=w0, max_iter=max_iter, lr=lr, want=tuple(want))
    if objective == "logreg":
        c.update(icpt=icpt, reg=reg, reg_lambda=reg_lambda, pos_weight=1.0)
    else:
        c.update(l_norm=l_norm, l_query=l_query, margin=margin)
    return _finish(c)


def _e0(dim):
    e = np.zeros(dim, F32)
    e[0] = 1.0
    return e


# (name, objective, n, dim, seed, keywords): `want` holds for the restatement over tests/_fb_ref.py's f64 objectives
# and survived four runs with the loss perturbed by 1e-7 and the gradient by 1e-6 (relative) when it was chosen, so
# that the engine's own rounding of an evaluation does not take a case off its branch.
LINE_CASES = [
    ("armijo-zoom-lr10", "logreg", 22, 4, 413813,
     dict(scale=100.0, lr=10.0, max_iter=1, w0_scale=1e-3, labels="ties", reg="norm", icpt=1, reg_lambda=0.0,
          want=("bracket_armijo", "insuf_set", "forced_steps", "high_replaced", "low_replaced", "exit:max_iter"))),
    ("swap-lr100", "hinge", 22, 64, 980421,
     dict(scale=100.0, lr=100.0, max_iter=25, w0_scale=1e-3, l_norm=100.0, l_query=10.0, margin=0.0,
          want=("bracket_armijo", "bracket_wolfe", "extrapolations", "forced_steps", "high_replaced", "swapped",
                "exit:max_eval"))),
    ("gtdpos-lr10", "logistic", 54, 4, 430655,
     dict(scale=0.1, lr=10.0, max_iter=25, w0_scale=10.0, labels="ties", l_norm=100.0, l_query=1.0, margin=0.0,
          want=("bracket_armijo", "bracket_wolfe", "bracket_gtd_pos", "extrapolations", "insuf_set", "high_replaced",
                "low_replaced", "low_to_high", "exit:max_eval"))),
    ("extrapolate-lr1e-3", "hinge", 45, 4, 35754,
     dict(scale=100.0, lr=1e-3, max_iter=3, w0_scale=10.0, l_norm=1.0, l_query=0.0, margin=1.0,
          want=("bracket_gtd_pos", "extrapolations", "low_replaced", "exit:max_eval"))),
    ("extrapolate-wolfe-lr1e-3", "logreg", 22, 64, 984544,
     dict(scale=10.0, lr=1e-3, max_iter=1, w0_scale=10.0, labels="equal", reg="vector", icpt=0, reg_lambda=100.0,
          want=("bracket_wolfe", "extrapolations", "exit:max_iter"))),
    ("zoom-max-ls", "hinge", 27, 16, 324026,
     dict(scale=1.0, lr=10.0, max_iter=25, w0_scale=1.0, labels="ties", l_norm=100.0, l_query=10.0, margin=0.2,
          want=("bracket_armijo", "insuf_set", "forced_steps", "high_replaced", "low_replaced", "zoom_max_ls",
                "exit:max_eval"))),
    ("width-dm", "hinge", 24, 4, 368665,
     dict(scale=1.0, lr=1.0, max_iter=12, w0_scale=1e-3, labels="ties", l_norm=1.0, l_query=10.0, margin=0.0,
          want=("bracket_armijo", "bracket_wolfe", "high_replaced", "zoom_width", "exit:dm"))),
    ("gtd", "logreg", 64, 16, 612014,
     dict(scale=1.0, lr=1.0, max_iter=25, w0_scale=1e-3, reg="vector", icpt=0, reg_lambda=100.0,
          want=("bracket_wolfe", "extrapolations", "exit:gtd"))),
    ("opt-cond", "logreg", 53, 64, 711744,
     dict(scale=10.0, lr=1.0, max_iter=25, w0_scale=0.0, reg="none", icpt=1, reg_lambda=0.0,
          want=("bracket_wolfe", "exit:opt_cond"))),
    ("dloss", "logreg", 59, 4, 720976,
     dict(scale=1.0, lr=1.0, max_iter=25, w0_scale=0.0, reg="norm", icpt=1, reg_lambda=100.0, sw_scale=1e-3,
          want=("bracket_wolfe", "exit:dloss"))),
    # (not held to the perturbation: its gradient is the same bits at every point, which is what skips the update)
    ("max-ls-exhausted", "logreg", 17, 16, 3,
     dict(scale=10.0, lr=1e-3, max_iter=24, w0_scale=10.0, labels="linear", reg="none", icpt=0,
          want=("max_ls_exhausted", "extrapolations", "skipped_updates"))),
    # every target equal (no label gradient), no query term, |w0| = 1 exactly: the gradient is zero in every format
    ("initial-opt", "hinge", 17, 16, 11,
     dict(scale=1.0, lr=1.0, max_iter=5, w0_scale=1.0, labels="equal", l_norm=100.0, l_query=0.0, w0=_e0(16),
          want=("exit:initial_opt",))),
]


def line_cases():
    return [line_case(name, obj, n, dim, seed, **kw) for name, obj, n, dim, seed, kw in LINE_CASES]


def reached(trace, want):
    """the entries of `want` the trace does not show"""
    return [w for w in want if not (trace.exit == w[5:] if w.startswith("exit:") else getattr(trace, w) > 0)]


# ---- the CPU evaluation: tests/_fb_ref.py's f64 objectives, the gradient rounded to f32 ----------------------------
def driver_len(c):
    """the length of the vectors the drivers carry: a one-output fit always has the bias slot"""
    return c["P"] if c["objective"] == "two" else c["dim"] + 1


def zero_slot(c):
    return c["dim"] if (c["objective"] != "two" and c["P"] == c["dim"]) else -1


def start_vector(c):
    x0 = np.zeros(driver_len(c), F32)
    x0[:c["P"]] = c["w0"]
    return x0


def cpu_eval(c):
    dim = c["dim"]
    if c["objective"] == "logreg":
        def ev(w):
            o = R.logreg(w[:dim], w[dim] if c["icpt"] else None, c["X"], c["y"], c["sw"], c["pos_weight"], c["reg_weight"],
                         c["qhat"], c["reg"])
            g = o["grad"] if c["icpt"] else np.concatenate([o["grad"], [0.0]])
            return float(o["loss"]), g.astype(F32)
    elif c["objective"] == "two":
        def ev(w):
            o = R.multiregneg(w.reshape(2, dim), c["X"], c["ys"], c["sw"], c["qhat"], l_norm=R.f32(c["l_norm"]),
                              l_query=R.f32(c["l_query"]))
            return float(o["loss"]), o["grad"].reshape(-1).astype(F32)
    else:
        def ev(w):
            o = R.multireg(w[:dim], c["X"], c["y"], c["sw"], c["qhat"], None, **c["kw"])
            return float(o["loss"]), np.concatenate([o["grad"], [0.0]]).astype(F32)
    return ev

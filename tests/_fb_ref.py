"""A plain numpy float64 restatement of the three objectives the feedback engine evaluates, and the seeded input
families the tests judge the engine on.  (A helper module, not a conftest.)

No torch in the arithmetic and no early rounding: every function takes the values the device receives (the f32
rows, targets, weights and parameters, widened to f64 exactly) and returns the loss, its parts, the analytic
gradient and the per-item intermediates the error bounds of tests/test_feedback_f64_gpu.py are formed from.
Stable forms throughout: softplus(-z) = logaddexp(0, -z), sigmoid(z) = exp(-logaddexp(0, -z)); the pairwise sums run
in row blocks so that 4096 items stay within memory.  tests/test_feedback_ref_cpu.py pins this file against
oracle/feedback_oracle.py (f64 autograd) and against finite differences of its own loss before anything is judged
by it.

    logreg       mean_i weight_i BCE-with-logits(z_i, y_i; pos_weight) + (lambda / n) R(w),  R = none | vector | norm |
                 norm1, optional intercept                       (seesaw/logistic_regression.py:68-124, 304-330)
    multireg     sum_i sw_i item_i + l_norm (cosh(log w.w) - 1) + l_data w'Mw + l_query (1 - w^.q^)/2, item = BCE under
                 the balanced re-weighting | pairwise hinge | pairwise logistic, the pairwise items carrying
                 coef_j / max_inv_j                              (seesaw/loops/multi_reg.py:85-129, rank_loss.py:34-95)
    multiregneg  two logits a row from the normalised rows of W: vertical BCE pair + horizontal CE on the labelled rows
                 + the norm and query regularisers, with the chain rule through F.normalize
                                                                 (seesaw/loops/multi_reg_module.py:64-128)
"""
from __future__ import annotations

import numpy as np

F64 = np.float64
EPS_NORMALIZE = 1e-12  # F.normalize's eps


def _f64(a):
    return np.asarray(a, dtype=F64)


def softplus_neg(z):
    """log(1 + exp(-z))"""
    return np.logaddexp(0.0, -z)


def sigmoid(z):
    return np.exp(-np.logaddexp(0.0, -z))


def center_f32(X):
    """the rows as the engine holds them after set_data(center=True): the f64 column mean rounded to f32, one f32
    subtraction per element.  (Exact whatever the order of the column sums when the rows are multiples of 2^-20, as
    every family below makes them: the f64 sums are then exact.)"""
    X = np.asarray(X, dtype=np.float32)
    mu = (X.astype(F64).sum(axis=0) / X.shape[0]).astype(np.float32)
    return X - mu[None, :]


# ---- logistic regression ------------------------------------------------------------------------------
def logreg(w, b, Xc, y, sample_weight, pos_weight, reg_weight, qhat=None, reg_kind="none"):
    """w [dim], b scalar or None, Xc [n, dim], y [n] in [0, 1], sample_weight [n] or None.  reg_weight = lambda / n."""
    w, Xc, y = _f64(w).reshape(-1), _f64(Xc), _f64(y).reshape(-1)
    n, dim = Xc.shape
    c = np.ones(n) if sample_weight is None else _f64(sample_weight).reshape(-1)
    bias = 0.0 if b is None else float(b)
    z = Xc @ w + bias
    lw = 1.0 + (float(pos_weight) - 1.0) * y
    sp = softplus_neg(z)
    bce = (1.0 - y) * z + lw * sp
    item = c * bce
    r = c * ((1.0 - y) - lw * sigmoid(-z))  # d item / d z
    data_loss = item.sum() / n if n else 0.0
    grad_w = (Xc.T @ r) / n if n else np.zeros(dim)
    grad_b = r.sum() / n if n else 0.0
    norm = float(np.sqrt(w @ w))
    nc = max(norm, EPS_NORMALIZE)
    what = w / nc
    reg, greg = 0.0, np.zeros(dim)
    if reg_kind == "vector":
        q = _f64(qhat).reshape(-1)
        diff = what - q
        reg = (norm - 1.0) ** 2 + diff @ diff
        greg = 2.0 * (norm - 1.0) * what + 2.0 * (diff - what * (what @ diff)) / nc
    elif reg_kind in ("norm", "norm1"):
        target = 1.0 if reg_kind == "norm1" else 0.0
        reg = (norm - target) ** 2
        greg = 2.0 * (norm - target) * what
    elif reg_kind != "none":
        raise ValueError(reg_kind)
    rw = float(reg_weight)
    grad = grad_w + rw * greg
    if b is not None:
        grad = np.concatenate([grad, [grad_b]])
    return {"loss": data_loss + rw * reg, "data_loss": data_loss, "reg_loss": rw * reg, "grad": grad, "z": z, "lw": lw,
            "sp": sp, "coef": c, "item": item, "r": r, "greg": rw * greg, "scale": 1.0 / max(n, 1),
            "absxw": np.abs(Xc) @ np.abs(w) + abs(bias)}


# ---- pairwise sums -------------------------------------------------------------------------------------
def pairwise(y, z, coef, margin, logistic, ez=None, block=256):
    """Over all ordered pairs (i, j): t_ij = sign(y_i - y_j), s_ij = z_i - z_j;
        hinge    loss_ij = max(0, margin - t_ij s_ij) - margin [t_ij == 0]   (0 where t_ij == 0, margin >= 0)
        logistic loss_ij = t_ij^2 log(1 + exp(-t_ij s_ij))
    item_j = coef_j / max_inv_j sum_i loss_ij with max_inv_j = #{i : t_ij != 0} (an item nobody differs from
    carries 0, where the reference's 0 / 0 is nan); r = d (sum_j item_j) / d z, the hinge passing its gradient on the
    kink (h >= 0) as torch's clamp(min=0) does.

    Also returned, for the bounds: `abs_s` [n] = sum_i |s_ij| over the pairs of column j; `kinks` = the number of
    ordered pairs with margin - t s == 0 exactly; and, given `ez` [n] (how far each z may be from the value the device
    holds), `e_item` / `e_r`: how far item and r can move under perturbations of s_ij of up to
    d_ij = ez_i + ez_j + 2^-24 |s_ij| (the device forms s as an f32 difference) -- a pair whose hinge argument lies within
    d_ij of the kink may switch, and counts with its whole contribution."""
    y, z, coef = _f64(y).reshape(-1), _f64(z).reshape(-1), _f64(coef).reshape(-1)
    n = z.shape[0]
    u = 2.0 ** -24
    ez = np.zeros(n) if ez is None else _f64(ez).reshape(-1)
    cnt = np.array([(y != yj).sum() for yj in y], dtype=F64) if n <= 64 else _count_different(y)
    c = np.where(cnt > 0, coef / np.where(cnt > 0, cnt, 1.0), 0.0)
    colloss, colD, rowD = np.zeros(n), np.zeros(n), np.zeros(n)
    abs_s, e_col, e_colD, e_rowD = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n)
    kinks = 0
    for i0 in range(0, n, block):
        i1 = min(i0 + block, n)
        t = np.sign(y[i0:i1, None] - y[None, :])            # [block, n]
        s = z[i0:i1, None] - z[None, :]
        on = t != 0
        d = (ez[i0:i1, None] + ez[None, :] + u * np.abs(s)) * on
        if logistic:
            a = -t * s
            loss = np.where(on, np.logaddexp(0.0, a), 0.0)
            D = np.where(on, -t * sigmoid(a), 0.0)          # d loss_ij / d s_ij
            eloss = d                                       # |d loss / d s| <= 1
            eD = d * 0.25                                   # |d^2 loss / d s^2| <= 1/4
        else:
            h = margin - t * s
            act = on & (h >= 0.0)
            kinks += int((on & (h == 0.0)).sum())
            loss = np.where(act, h, 0.0)
            D = np.where(act, -t, 0.0)
            near = on & (np.abs(h) <= d)                    # may be on the other side on the device
            eloss = np.where(act | near, d, 0.0)
            eD = near.astype(F64)
        colloss += loss.sum(axis=0)
        colD += D.sum(axis=0)
        rowD[i0:i1] = D @ c
        abs_s += (np.abs(s) * on).sum(axis=0)
        e_col += eloss.sum(axis=0)
        e_colD += eD.sum(axis=0)
        e_rowD[i0:i1] = eD @ np.abs(c)
    item = c * colloss
    r = -c * colD + rowD
    return {"item": item, "r": r, "c": c, "cnt": cnt, "abs_s": abs_s, "kinks": kinks, "colloss": colloss,
            "e_item": np.abs(c) * e_col, "e_r": np.abs(c) * e_colD + e_rowD,
            "abs_r": np.abs(c) * cnt + _weighted_count(y, np.abs(c), cnt)}


def _count_different(y):
    _, inv, counts = np.unique(y, return_inverse=True, return_counts=True)
    return (y.shape[0] - counts[inv]).astype(F64)


def _weighted_count(y, c, cnt):
    """sum of c_i over the items i that differ from j: an upper bound of the second half of |r_j|'s terms"""
    vals, inv = np.unique(y, return_inverse=True)
    per = np.zeros(vals.shape[0])
    np.add.at(per, inv, c)
    return c.sum() - per[inv]


# ---- RegModule -----------------------------------------------------------------------------------------
def multireg_coef(y, sample_weight, loss_type, pos_weight=-1.0):
    """the per-item coefficients of RegModule._step's sample-weight bookkeeping (multi_reg.py:85-105) and whether the
    label loss is on at all: BCE re-weights the items with y == 1 and renormalises to the original total; the
    pairwise forms keep the weights and are off until both a positive (y == 1) and anything else are labelled"""
    y, sw = _f64(y).reshape(-1), _f64(sample_weight).reshape(-1).copy()
    orig = sw.sum()
    pos_total = sw[y == 1.0].sum()
    neg_total = orig - pos_total
    if loss_type == "ce_loss":
        pw = (neg_total + 1.0) / (pos_total + 1.0) if pos_weight < 0 else float(pos_weight)
        sw[y == 1.0] *= pw
        sw *= orig / sw.sum()
        return sw, True
    return sw, bool(pos_total > 0 and neg_total > 0)


def multireg(w, Xc, y, sample_weight, qhat, xlx, *, loss_type, margin=0.2, l_norm=100.0, l_data=0.0, l_query=0.0,
             pos_weight=-1.0, ez_of=None):
    """`ez_of(absxw)` (optional) turns sum_k |x_ik w_k| into the logit error the pairwise bounds start from"""
    w, Xc, y = _f64(w).reshape(-1), _f64(Xc), _f64(y).reshape(-1)
    n, dim = Xc.shape
    q = _f64(qhat).reshape(-1)
    coef, active = multireg_coef(y, sample_weight, loss_type, pos_weight)
    z = Xc @ w
    absxw = np.abs(Xc) @ np.abs(w)
    extra = {}
    if loss_type == "ce_loss":
        sp = softplus_neg(z)
        item = coef * ((1.0 - y) * z + sp)
        r = coef * ((1.0 - y) - sigmoid(-z))
        extra = {"sp": sp, "lw": np.ones(n)}
    elif active:
        pw_ = pairwise(y, z, coef, margin, loss_type == "pairwise_logistic_loss",
                       ez=None if ez_of is None else ez_of(absxw))
        item, r = pw_["item"], pw_["r"]
        extra = {"pair": pw_}
    else:
        item, r = np.zeros(n), np.zeros(n)
    ww = float(w @ w)
    norm = np.sqrt(ww)
    nc = max(norm, EPS_NORMALIZE)
    what = w / nc
    whq = float(what @ q)
    p_norm = l_norm * (np.cosh(np.log(ww)) - 1.0)
    M = None if xlx is None else _f64(xlx)
    p_data = l_data * float(w @ (M @ w)) if (M is not None and l_data != 0.0) else 0.0
    p_query = l_query * (1.0 - whq) / 2.0
    g_norm = l_norm * np.sinh(np.log(ww)) / ww * 2.0 * w
    g_data = l_data * ((M + M.T) @ w) if (M is not None and l_data != 0.0) else np.zeros(dim)
    g_query = -0.5 * l_query * (q - whq * what) / nc
    labels = float(item.sum())
    g_lab = Xc.T @ r
    out = {"loss": labels + p_data + p_norm + p_query, "parts": np.array([p_norm, p_data, p_query, labels]),
           "grad": g_lab + g_norm + g_data + g_query, "greg": g_norm + g_data + g_query, "z": z, "coef": coef,
           "item": item, "r": r, "absxw": absxw, "active": active, "ww": ww, "scale": 1.0}
    out.update(extra)
    return out


# ---- MultiRegModule ------------------------------------------------------------------------------------
def multiregneg(W, Xc, ys, sample_weight, qhat, *, l_norm, l_query):
    """W [2, dim] raw weights, ys [n, 2] (target, confusion class), sample_weight [n]"""
    W, Xc, ys = _f64(W), _f64(Xc), _f64(ys)
    n, dim = Xc.shape
    s = np.ones(n) if sample_weight is None else _f64(sample_weight).reshape(-1)
    q = _f64(qhat).reshape(-1)
    nrm = np.sqrt((W * W).sum(axis=1))
    den = np.maximum(nrm, EPS_NORMALIZE)
    nw = W / den[:, None]
    z = Xc @ nw.T                                            # [n, 2]
    sp = softplus_neg(z)
    vert = ((1.0 - ys) * z + sp).sum(axis=1)
    near = ys.sum(axis=1)
    lab = near > 0
    lse = np.logaddexp(z[:, 0], z[:, 1])
    logsm = z - lse[:, None]
    hor = np.where(lab, -(ys * logsm).sum(axis=1), 0.0)
    dz = sigmoid(z) - ys
    dz = dz + np.where(lab[:, None], near[:, None] * np.exp(logsm) - ys, 0.0)
    r = s[:, None] * dz                                      # [n, 2]
    vsum, hsum = float(s @ vert), float(s @ hor)
    g = Xc.T @ r                                             # [dim, 2] d labels / d nw
    nq = nw @ q
    lq = l_query * (1.0 - nq) / 2.0
    lg = np.log(nrm)
    loss_norm = l_norm * float((np.cosh(lg) - 1.0).sum())
    G = g.T - 0.5 * l_query * q[None, :]                     # [2, dim] d total / d nw
    dotg = (nw * G).sum(axis=1)
    radial = l_norm * np.sinh(lg) / den
    grad = (G - nw * dotg[:, None]) / den[:, None] + radial[:, None] * nw
    return {"loss": vsum + hsum + loss_norm + lq[0] + lq[1], "parts": np.array([loss_norm, lq[0], lq[1], vsum, hsum]),
            "grad": grad, "z": z, "nw": nw, "nrm": nrm, "r": r, "g": g.T, "G": G, "dotg": dotg, "radial": radial,
            "vert": vert, "hor": hor, "sp": sp, "lse": lse, "near": near, "s": s,
            "absxw": np.abs(Xc) @ np.abs(nw).T}


# ---- input families ------------------------------------------------------------------------------------
Q20 = 2.0 ** 20


def quantise(X):
    """to multiples of 2^-20: column sums of such rows are exact in f64, so the centred rows do not depend on the
    order the device adds them in"""
    return (np.round(np.asarray(X, F64) * Q20) / Q20).astype(np.float32)


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def planted_fraction(n, phase=0):
    """signed a_i in [-1, 1], the row's component along the weight direction: every tenth row |a| in [0.9, 1]
    ("hi"), every third |a| in [0.36, 0.9] ("mid"), the rest |a| < 0.3 -- deterministic in i, so that the fractions
    hold at n = 1, 2, 3 too"""
    rng = np.random.default_rng(1000 + n + 7919 * phase)
    i = np.arange(n) + phase
    hi, mid = (i % 10) == 0, (i % 3) == 1
    mag = np.where(hi, rng.uniform(0.9, 1.0, n), np.where(mid, rng.uniform(0.36, 0.9, n), rng.uniform(0.0, 0.3, n)))
    return mag * np.where(rng.uniform(size=n) < 0.5, -1.0, 1.0)


def planted_rows(n, dim, seed, phase=0):
    """golden-like unit rows x_i = a_i d + sqrt(1 - a_i^2) p_i, d a random unit direction, p_i unit and orthogonal to
    d; quantised.  -> (X f32 [n, dim], d f64 [dim])"""
    rng = np.random.default_rng(seed)
    d = _unit(rng.standard_normal(dim))
    a = planted_fraction(n, phase)
    P = rng.standard_normal((n, dim))
    P -= (P @ d)[:, None] * d[None, :]
    P = _unit(P)
    return quantise(a[:, None] * d[None, :] + np.sqrt(1.0 - a * a)[:, None] * P), d


def labels_mixed(n, seed):
    """targets 0, 1 and soft (a third each, at least one 1 and one 0 from n = 2 on), sample weights in [0.5, 3]; f32"""
    rng = np.random.default_rng(seed)
    kind = np.arange(n) % 3
    y = np.where(kind == 0, 1.0, np.where(kind == 1, 0.0, rng.uniform(0.05, 0.95, n)))
    perm = rng.permutation(n) if n > 2 else np.arange(n)
    return y[perm].astype(np.float32), rng.uniform(0.5, 3.0, n).astype(np.float32)


def family_logits(n, dim, seed, span, center, intercept=False):
    """one-output inputs whose logits span +-`span`: planted rows and w = span d (span 1: the mild control).
    -> dict X (as handed to set_data), Xc (as the engine then holds it), w f32 [dim (+1)], y, sw, q"""
    X, d = planted_rows(n, dim, seed)
    Xc = center_f32(X) if center else X
    rng = np.random.default_rng(seed + 1)
    w = (span * d + 0.02 * span * rng.standard_normal(dim) / np.sqrt(dim)).astype(np.float32)
    if intercept:
        w = np.concatenate([w, [np.float32(0.03 * span)]]).astype(np.float32)
    y, sw = labels_mixed(n, seed + 2)
    q = _unit(d + 0.3 * rng.standard_normal(dim) / np.sqrt(dim)).astype(np.float32)
    return {"X": X, "Xc": Xc, "w": w, "y": y, "sw": sw, "q": q, "center": center}


def qhat_f32(q):
    """the unit query as ssw_fb_set_query installs it: f64 norm, each element rounded to f32"""
    q = np.asarray(q, np.float32)
    nn = float((q.astype(F64) ** 2).sum())
    return (q.astype(F64) * (1.0 / max(np.sqrt(nn), EPS_NORMALIZE))).astype(np.float32)


def family_two_output(n, dim, seed, span):
    """two-output inputs: rows span (a_i d0 + b_i d1) + noise, d0 and d1 orthonormal, W rows along d0 / d1 (the logits use W's normalised
    rows, so it is the rows that are scaled), then one common factor so that max |z| = span exactly enough.
    -> dict X = Xc (center=False), W f32 [2, dim], ys f32 [n, 2], sw, q"""
    rng = np.random.default_rng(seed)
    D = _unit(rng.standard_normal((2, dim)))
    D[1] = _unit(D[1] - (D[1] @ D[0]) * D[0])   # orthonormal: each logit follows its own planted component
    a, b = planted_fraction(n, 0), planted_fraction(n, 1)
    noise = _unit(rng.standard_normal((n, dim)))
    X = span * (a[:, None] * D[0][None, :] + b[:, None] * D[1][None, :]) + min(1.0, span) * 0.5 * noise
    W = (D * np.array([[1.3], [0.8]]) + 0.02 * rng.standard_normal((2, dim)) / np.sqrt(dim)).astype(np.float32)
    nw = W.astype(F64) / np.linalg.norm(W.astype(F64), axis=1, keepdims=True)
    X = quantise(X * (span / np.abs(X @ nw.T).max()))
    k = np.arange(n) % 5   # rows without a label, with one, with the other, with both soft, with a hard pair
    y0 = np.where(k == 1, 1.0, np.where(k == 3, rng.uniform(0.1, 0.9, n), np.where(k == 4, 1.0, 0.0)))
    y1 = np.where(k == 2, 1.0, np.where(k == 3, rng.uniform(0.1, 0.9, n), 0.0))
    ys = np.stack([y0, y1], axis=1).astype(np.float32)
    sw = rng.uniform(0.5, 3.0, n).astype(np.float32)
    q = _unit(D[0] + 0.3 * rng.standard_normal(dim) / np.sqrt(dim)).astype(np.float32)
    return {"X": X, "Xc": X, "W": W, "ys": ys, "sw": sw, "q": q}


def family_exact(kind="kink"):
    """The exact family: rows a_i e_0 with a_i a multiple of 1/8, w = e_0, center=False, so z_i = a_i exactly; hinge
    margin 0.25.  16 items, 8 labelled 1 and 8 labelled 0 (max_inv = 8 everywhere: coef / max_inv is exact), with
    pairs on the kink (a_pos - a_neg = 0.25), just inside (0.125) and just outside (0.375) among them.
    kind: "kink" as described; "equal" all labels 1; "one_pos" 33 items with a single 1 (max_inv 32 and 1); "soft"
    labels that are multiples of 1/8 in (0, 1) with one 1.
    -> dict a f32 [n], y f32 [n], sw f32 [n] (multiples of 1/4), margin"""
    neg = np.array([0.0, 0.125, 0.25, 0.5, -0.375, 1.0, 0.75, -1.0])
    pos = np.array([0.25, 0.375, 0.625, 0.875, 0.0, 1.25, 0.5, -0.75])
    if kind in ("kink", "equal"):
        a = np.concatenate([pos, neg])
        y = np.concatenate([np.ones(8), np.zeros(8) if kind == "kink" else np.ones(8)])
    elif kind == "one_pos":
        a = np.concatenate([[0.25], np.tile(neg, 4)])
        y = np.concatenate([[1.0], np.zeros(32)])
    elif kind == "soft":
        a = np.concatenate([pos, neg])
        y = np.concatenate([[1.0], (np.arange(15) % 7 + 1) / 8.0])
    else:
        raise ValueError(kind)
    n = a.shape[0]
    sw = (1.0 + (np.arange(n) % 4)) / 4.0 * 2.0
    return {"a": a.astype(np.float32), "y": y.astype(np.float32), "sw": sw.astype(np.float32), "margin": 0.25}


# ---- the cases of tests/test_feedback_f64_gpu.py (tests/test_feedback_ref_cpu.py asserts the families' conditions
# on exactly these inputs, from the reference alone) -----------------------------------------------------------
SPAN_SAT, SPAN_MID, SPAN_MILD = 90.0, 30.0, 1.0
SPAN_PAIR_LOGISTIC = 38.0   # |z_i - z_j| <= 80: the reference's own f32 log(1 + exp(.)) stays finite
SPAN_TWO = 80.0             # the two-output form is f32 throughout

# (n, dim, regulariser, intercept, pos_weight (-1: balanced, n_neg / n_pos as LogisticRegressionPT forms it), center)
LOGREG_CASES = [
    (1, 4, "none", 0, 1.0, False), (2, 16, "vector", 1, 0.2, False), (31, 64, "norm", 0, 7.0, True),
    (32, 192, "norm1", 1, -1.0, False), (33, 512, "vector", 0, 1.0, True), (1023, 768, "none", 1, 7.0, True),
    (1024, 772, "norm", 1, 0.2, False), (1025, 776, "norm1", 0, -1.0, True), (2047, 1020, "vector", 1, 7.0, False),
    (2048, 1024, "norm1", 1, 1.0, True), (8192, 16, "norm", 1, 1.0, False), (8193, 512, "vector", 1, 0.2, True),
    (9217, 64, "none", 0, 7.0, True), (33, 1020, "norm1", 1, 0.2, False),   # the last: the one-launch fit's widest driver
]
# (n, dim, pos_weight (-1: balanced over the sample weights), l_data, l_query, center)
MULTIREG_CE_CASES = [
    (1, 4, -1.0, 0.5, 1.0, False), (2, 16, 0.2, 0.0, 0.0, False), (31, 64, -1.0, 0.25, 10.0, True),
    (32, 192, 7.0, 0.0, 1.0, False), (33, 512, -1.0, 0.0, 10.0, True), (1023, 768, 1.0, 0.0, 1.0, True),
    (1024, 772, -1.0, 0.0, 0.0, False), (1025, 776, 0.2, 0.0, 1.0, True), (2047, 1020, -1.0, 0.0, 10.0, False),
    (2048, 1024, 7.0, 0.0, 1.0, True), (8192, 16, -1.0, 0.5, 1.0, False), (8193, 512, 1.0, 0.0, 0.0, True),
    (9217, 64, -1.0, 0.0, 10.0, True),
]
# (n, dim, loss_type, center)
MULTIREG_PAIR_CASES = [(n, dim, lt, center) for lt in ("pairwise_rank_loss", "pairwise_logistic_loss")
                       for n, dim, center in ((2, 4, False), (3, 16, False), (1024, 64, True), (1025, 192, False),
                                              (4095, 16, True), (4096, 4, False))]
# (n, dim)
TWO_OUTPUT_CASES = [(1, 4), (33, 256), (1024, 512), (1025, 4), (1025, 512)]
MULTIREG_L_NORM = {SPAN_SAT: 0.01, SPAN_MID: 0.01, SPAN_PAIR_LOGISTIC: 0.01, SPAN_MILD: 100.0}


def logreg_pos_weight(pw, y):
    if pw >= 0:
        return float(pw)
    return max(int((y == 0).sum()), 1) / max(int((y == 1).sum()), 1)


def f32(v):
    """the value a float parameter has once it has crossed the C interface"""
    return float(np.float32(v))


def logreg_case(k, span):
    """inputs of LOGREG_CASES[k] at logit span `span`, with the reference evaluated at them under "ref" """
    n, dim, reg, icpt, pw, center = LOGREG_CASES[k]
    f = family_logits(n, dim, 100 + k, span, center and n > 1, bool(icpt))
    f.update(n=n, dim=dim, reg=reg, icpt=icpt, qhat=qhat_f32(f["q"]), reg_weight=f32(1.0 / n),
             pos_weight=f32(logreg_pos_weight(pw, f["y"])))
    f["ref"] = logreg_at(f, f["w"])
    return f


def logreg_at(f, w):
    dim = f["dim"]
    return logreg(w[:dim], w[dim] if f["icpt"] else None, f["Xc"], f["y"], f["sw"], f["pos_weight"], f["reg_weight"],
                  f["qhat"], f["reg"])


def multireg_case(n, dim, seed, span, center, loss_type, pos_weight=-1.0, l_data=0.0, l_query=0.0, ez_of=None):
    f = family_logits(n, dim, seed, span, center and n > 1)
    xlx = None
    if l_data:
        rng = np.random.default_rng(seed + 9)
        A, K = rng.standard_normal((dim, dim)), rng.standard_normal((dim, dim))
        # positive semi-definite (the objective stays bounded below) plus an antisymmetric part: w'Mw does not see
        # it, M w and M'w do, and (M + M') w must not
        xlx = ((0.2 * A @ A.T + 0.1 * (K - K.T)) / dim).astype(np.float32)
    f.update(n=n, dim=dim, qhat=qhat_f32(f["q"]), xlx=xlx, ez_of=ez_of,
             kw=dict(loss_type=loss_type, margin=f32(0.2), l_norm=f32(MULTIREG_L_NORM[span]), l_data=f32(l_data),
                     l_query=f32(l_query), pos_weight=f32(pos_weight)))
    f["ref"] = multireg_at(f, f["w"])
    return f


def multireg_at(f, w):
    return multireg(w, f["Xc"], f["y"], f["sw"], f["qhat"], f["xlx"], ez_of=f["ez_of"], **f["kw"])


def multireg_ce_case(k, span, ez_of=None):
    n, dim, pw, l_data, l_query, center = MULTIREG_CE_CASES[k]
    return multireg_case(n, dim, 200 + k, span, center, "ce_loss", pw, l_data, l_query, ez_of)


def multireg_pair_case(k, ez_of=None, mild=False):
    n, dim, lt, center = MULTIREG_PAIR_CASES[k]
    span = SPAN_MILD if mild else (SPAN_PAIR_LOGISTIC if lt == "pairwise_logistic_loss" else SPAN_SAT)
    return multireg_case(n, dim, 300 + k, span, center, lt, l_query=1.0, ez_of=ez_of)


def two_output_case(k, span):
    n, dim = TWO_OUTPUT_CASES[k]
    f = family_two_output(n, dim, 400 + k, span)
    f.update(n=n, dim=dim, qhat=qhat_f32(f["q"]), l_norm=f32(0.5), l_query=f32(3.0))
    f["ref"] = two_output_at(f, f["W"])
    return f


def two_output_at(f, W):
    return multiregneg(W, f["Xc"], f["ys"], f["sw"], f["qhat"], l_norm=f["l_norm"], l_query=f["l_query"])

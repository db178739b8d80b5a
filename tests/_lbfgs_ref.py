"""A numpy restatement of the feedback fit's driver -- torch.optim.LBFGS.step with the strong-Wolfe line search -- that
keeps a trace of the branches it takes.  (A helper module, not a conftest.)

Written from torch/optim/lbfgs.py (LBFGS.step, _strong_wolfe, _cubic_interpolate) with the numeric conventions the
header of seesaw_amd/csrc/feedback_lbfgs.hip documents, and from nothing else of the project's:
  * vectors are f32, scalars (loss, step, g.d, 1 / y.s, H_diag, the alphas) are f64 python floats;
  * a trial point is x + f32(t) * d, one f32 multiplication and one f32 addition (no contraction);
  * the first step's sum of |g| is taken in f64;
  * max_eval = max_iter * 5 // 4, max_ls = 25 (the installed torch passes max_eval - current_evals for max_ls instead:
    `ls_budget=True` restates that, for the comparison with torch itself);
  * `zero_slot`: a parameter slot the objective does not use (the bias of a fit without an intercept), whose gradient
    entry is held at zero wherever the driver keeps a gradient.

The dot product is a parameter.  `wave_dot` restates the association documented above wave_sum_host
(seesaw_amd/csrc/fb_math.h): element i sits in lane i % 64, a lane adds its f32 products in ascending order, then
inside every 16-lane row lane l takes lane l - s for s = 1, 2, 4, 8, then the four row totals (lanes 15, 31, 47, 63)
are added in ascending order.  `plain_dot` is torch.dot, to stand beside torch on the CPU.

The history is a python list with pop(0): no ring, no slots, no prefetch.  That is the point of it.

    lbfgs(evalfn, x0, max_iter, lr, ...) -> (x f32, n_iter, func_evals, loss f64, Trace)
    evalfn(w f32 [P]) -> (loss as a python float (f64), gradient f32 [P])
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np

F32 = np.float32
HISTORY = 100
TOL_GRAD, TOL_CHANGE, C1, C2, MAX_LS = 1e-7, 1e-9, 1e-4, 0.9, 25


@dataclass
class Trace:
    evictions: int = 0          # history entries dropped at the front (the 101st accepted update on)
    skipped_updates: int = 0    # y.s <= 1e-10: the pair is not stored
    updates: int = 0            # pairs stored
    bracket_armijo: int = 0     # bracketing ended by (a) Armijo violated or no decrease
    bracket_wolfe: int = 0      # (b) strong Wolfe satisfied
    bracket_gtd_pos: int = 0    # (c) g_new.d >= 0
    extrapolations: int = 0     # bracketing went on to a longer step
    max_ls_exhausted: int = 0   # max_ls extrapolations without a bracket: [0, t]
    zoom_evals: int = 0
    insuf_set: int = 0          # the insufficient-progress flag was raised
    forced_steps: int = 0       # the trial point was moved 0.1 of the bracket away from an end
    high_replaced: int = 0      # the new point became the bracket's high end
    low_replaced: int = 0       # the new point became the bracket's low end
    swapped: int = 0            # low and high changed places after the high end was replaced
    low_to_high: int = 0        # the old low end became the high end before the new point took its place
    zoom_done: int = 0          # zoom ended by strong Wolfe
    zoom_width: int = 0         # ... by |bracket| * max|d| < 1e-9
    zoom_max_ls: int = 0        # ... by max_ls evaluations
    exit: str = ""              # initial_opt | max_iter | max_eval | opt_cond | dm | dloss | gtd
    history_len: int = 0        # entries held at the end
    max_ls_iter: int = 0        # the largest ls_iter any line search reached
    min_ls_budget: int = field(default=10 ** 9)  # the smallest max_eval - current_evals a line search started with

    def counters(self):
        return {k: v for k, v in self.__dict__.items() if v not in (0, "", 10 ** 9)}


# ---- sums and dots -------------------------------------------------------------------------------------
def wave_sum(p, dtype=F32):
    """sum of p in the association of wave_sum_host<dtype>; every addition is one numpy addition in `dtype`"""
    p = np.asarray(p, dtype=dtype).reshape(-1)
    n = p.shape[0]
    rows = max((n + 63) // 64, 1)
    if rows * 64 != n:
        p = np.concatenate([p, np.zeros(rows * 64 - n, dtype)])
    p = p.reshape(rows, 64)
    b = np.zeros(64, dtype)
    for r in range(rows):           # a lane adds its elements in ascending order (the zeros behind the end change nothing)
        b = b + p[r]
    b = b.reshape(4, 16)
    for s in (1, 2, 4, 8):          # lane l takes lane l - s of its row; the row's first s lanes take 0
        b = b + np.concatenate([np.zeros((4, s), dtype), b[:, :-s]], axis=1)
    return dtype(dtype(dtype(b[0, 15] + b[1, 15]) + b[2, 15]) + b[3, 15])


def wave_dot(a, b):
    """f32 products, wave_sum in f32, widened"""
    return float(wave_sum(np.asarray(a, F32) * np.asarray(b, F32), F32))


def wave_abs_sum64(g):
    return float(wave_sum(np.abs(np.asarray(g, F32)).astype(np.float64), np.float64))


def plain_dot(a, b):
    import torch
    return float(torch.dot(torch.from_numpy(np.ascontiguousarray(a, F32)), torch.from_numpy(np.ascontiguousarray(b, F32))))


def plain_abs_sum64(g):
    return float(np.abs(np.asarray(g, F32)).astype(np.float64).sum())


def _absmax(v):
    return float(np.abs(v).max()) if v.shape[0] else 0.0


def _div(a, b):
    """a / b as IEEE does it (python raises on a zero divisor)"""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


# ---- the line search -----------------------------------------------------------------------------------
def _strong_wolfe(obj, t, d, f, g, gtd, dot, tr, max_ls):
    d_norm = _absmax(d)
    f_new, g_new = obj(t)
    ls_evals = 1
    gtd_new = dot(g_new, d)
    t_prev, f_prev, g_prev, gtd_prev = 0.0, f, g, gtd
    done = False
    ls_iter = 0
    bracket = None
    while ls_iter < max_ls:
        if f_new > (f + C1 * t * gtd) or (ls_iter > 1 and f_new >= f_prev):
            bracket, bracket_f, bracket_g, bracket_gtd = [t_prev, t], [f_prev, f_new], [g_prev, g_new], [gtd_prev, gtd_new]
            tr.bracket_armijo += 1
            break
        if abs(gtd_new) <= -C2 * gtd:
            bracket, bracket_f, bracket_g, bracket_gtd = [t], [f_new], [g_new], [gtd_new]
            done = True
            tr.bracket_wolfe += 1
            break
        if gtd_new >= 0:
            bracket, bracket_f, bracket_g, bracket_gtd = [t_prev, t], [f_prev, f_new], [g_prev, g_new], [gtd_prev, gtd_new]
            tr.bracket_gtd_pos += 1
            break
        min_step, max_step = t + 0.01 * (t - t_prev), t * 10
        tmp = t
        t = cubic_interpolate(t_prev, f_prev, gtd_prev, t, f_new, gtd_new, (min_step, max_step))
        tr.extrapolations += 1
        t_prev, f_prev, g_prev, gtd_prev = tmp, f_new, g_new, gtd_new
        f_new, g_new = obj(t)
        ls_evals += 1
        gtd_new = dot(g_new, d)
        ls_iter += 1
    exhausted = ls_iter == max_ls
    if exhausted:
        bracket, bracket_f, bracket_g, bracket_gtd = [0.0, t], [f, f_new], [g, g_new], [gtd, gtd_new]
        tr.max_ls_exhausted += 1
    insuf = False
    low, high = (0, 1) if bracket_f[0] <= bracket_f[-1] else (1, 0)
    while not done:
        if ls_iter >= max_ls:
            if not exhausted:
                tr.zoom_max_ls += 1
            break
        if abs(bracket[1] - bracket[0]) * d_norm < TOL_CHANGE:
            tr.zoom_width += 1
            break
        t = cubic_interpolate(bracket[0], bracket_f[0], bracket_gtd[0], bracket[1], bracket_f[1], bracket_gtd[1], None)
        bmax, bmin = max(bracket), min(bracket)
        eps = 0.1 * (bmax - bmin)
        if min(bmax - t, t - bmin) < eps:
            if insuf or t >= bmax or t <= bmin:
                t = bmax - eps if abs(t - bmax) < abs(t - bmin) else bmin + eps
                insuf = False
                tr.forced_steps += 1
            else:
                insuf = True
                tr.insuf_set += 1
        else:
            insuf = False
        f_new, g_new = obj(t)
        ls_evals += 1
        tr.zoom_evals += 1
        gtd_new = dot(g_new, d)
        ls_iter += 1
        if f_new > (f + C1 * t * gtd) or f_new >= bracket_f[low]:
            bracket[high], bracket_f[high], bracket_g[high], bracket_gtd[high] = t, f_new, g_new, gtd_new
            tr.high_replaced += 1
            new_low = 0 if bracket_f[0] <= bracket_f[1] else 1
            if new_low != low:
                tr.swapped += 1
            low, high = new_low, 1 - new_low
        else:
            if abs(gtd_new) <= -C2 * gtd:
                done = True
                tr.zoom_done += 1
            elif gtd_new * (bracket[high] - bracket[low]) >= 0:
                bracket[high], bracket_f[high], bracket_g[high], bracket_gtd[high] = \
                    bracket[low], bracket_f[low], bracket_g[low], bracket_gtd[low]
                tr.low_to_high += 1
            bracket[low], bracket_f[low], bracket_g[low], bracket_gtd[low] = t, f_new, g_new, gtd_new
            tr.low_replaced += 1
    tr.max_ls_iter = max(tr.max_ls_iter, ls_iter)
    return bracket_f[low], bracket_g[low], bracket[low], ls_evals


def cubic_interpolate(x1, f1, g1, x2, f2, g2, bounds=None):
    """torch.optim.lbfgs._cubic_interpolate on python floats, with IEEE divisions: 0 / 0 and x / 0 give nan / inf as
    in C, and the clamp treats a nan as fmin / fmax do (the other operand wins)"""
    if bounds is not None:
        xmin, xmax = bounds
    else:
        xmin, xmax = (x1, x2) if x1 <= x2 else (x2, x1)
    with np.errstate(all="ignore"):
        d1 = g1 + g2 - _div(3.0 * (f1 - f2), x1 - x2)
        d2sq = d1 * d1 - g1 * g2
        if d2sq >= 0:
            d2 = math.sqrt(d2sq)
            if x1 <= x2:
                mp = x2 - (x2 - x1) * _div(g2 + d2 - d1, g2 - g1 + 2.0 * d2)
            else:
                mp = x1 - (x1 - x2) * _div(g1 + d2 - d1, g1 - g2 + 2.0 * d2)
            return float(np.fmin(np.fmax(mp, xmin), xmax))
    return (xmin + xmax) / 2.0


# ---- the driver ----------------------------------------------------------------------------------------
def lbfgs(evalfn, x0, max_iter, lr, *, dot=wave_dot, abs_sum64=wave_abs_sum64, zero_slot=-1, history=HISTORY,
          max_ls=MAX_LS, ls_budget=False):
    """one LBFGS(max_iter, lr, line_search_fn="strong_wolfe").step(closure) from x0"""
    tr = Trace()
    x = np.array(x0, dtype=F32).reshape(-1)
    lr32 = float(F32(lr))                      # the step length crosses the C interface as a float
    max_eval = max_iter * 5 // 4
    evals = [0]

    def call(w):
        loss, g = evalfn(w)
        evals[0] += 1
        loss = float(loss)
        if not math.isfinite(loss):
            raise FloatingPointError(f"loss diverged ({loss})")
        g = np.array(g, dtype=F32).reshape(-1)
        assert g.shape == x.shape
        return loss, g

    def held(g):
        if zero_slot >= 0:
            g = g.copy()
            g[zero_slot] = F32(0)
        return g

    loss, g = call(x + F32(0.0) * np.zeros_like(x))
    g = held(g)
    current_evals, n_iter = 1, 0
    t, H_diag = 0.0, 1.0
    d = np.zeros_like(x)
    old_dirs, old_stps, ro = [], [], []
    prev_g = None
    if _absmax(g) <= TOL_GRAD:
        tr.exit = "initial_opt"
        return x, 0, evals[0], loss, tr
    tr.exit = "max_iter"                        # the loop condition's own exit
    while n_iter < max_iter:
        n_iter += 1
        if n_iter == 1:
            d = -g
            H_diag = 1.0
        else:
            y = g - prev_g
            s = d * F32(t)
            ys = dot(y, s)
            if ys > 1e-10:
                if len(old_dirs) == history:
                    old_dirs.pop(0)
                    old_stps.pop(0)
                    ro.pop(0)
                    tr.evictions += 1
                old_dirs.append(y)
                old_stps.append(s)
                ro.append(1.0 / ys)
                tr.updates += 1
                H_diag = _div(ys, dot(y, y))
            else:
                tr.skipped_updates += 1
            m = len(old_dirs)
            al = [0.0] * m
            q = -g
            for i in range(m - 1, -1, -1):
                al[i] = dot(old_stps[i], q) * ro[i]
                q = q - F32(al[i]) * old_dirs[i]
            d = q * F32(H_diag)
            for i in range(m):
                be = dot(old_dirs[i], d) * ro[i]
                d = d + F32(al[i] - be) * old_stps[i]
        prev_g = g.copy()
        prev_loss = loss
        if n_iter == 1:
            t = min(1.0, _div(1.0, abs_sum64(g))) * lr32
        else:
            t = lr32
        gtd = dot(g, d)
        if gtd > -TOL_CHANGE:
            tr.exit = "gtd"
            break
        budget = max_eval - current_evals
        tr.min_ls_budget = min(tr.min_ls_budget, budget)
        x_ls, d_ls = x, d
        f_new, g_new, t, ls_evals = _strong_wolfe(lambda tt: call(x_ls + F32(tt) * d_ls), t, d, loss, g, gtd, dot, tr,
                                                  budget if ls_budget else max_ls)
        loss, g = f_new, held(g_new)
        x = x + F32(t) * d
        opt_cond = _absmax(g) <= TOL_GRAD
        current_evals += ls_evals
        if n_iter == max_iter:
            tr.exit = "max_iter"
            break
        if current_evals >= max_eval:
            tr.exit = "max_eval"
            break
        if opt_cond:
            tr.exit = "opt_cond"
            break
        if float(np.abs(d.astype(np.float64) * t).max()) <= TOL_CHANGE:
            tr.exit = "dm"
            break
        if abs(loss - prev_loss) < TOL_CHANGE:
            tr.exit = "dloss"
            break
    tr.history_len = len(old_dirs)
    return x, n_iter, evals[0], loss, tr

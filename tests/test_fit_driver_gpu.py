"""The feedback fit's two L-BFGS drivers -- lbfgs_host (csrc/feedback_lbfgs.hip) and the six-state machine
fit_driver_step walks inside k_fb_fit_wg / k_fb_fit_wg_batch / k_fb_fit2_wg / k_fb_fit2_wg_batch
(csrc/feedback_fit_wg.hip) -- held to a third statement of the algorithm that shares nothing with them:
tests/_lbfgs_ref.py, written from torch/optim/lbfgs.py, with a python list for the history (no ring) and a trace of
the branches it takes.  tests/test_lbfgs_ref_cpu.py anchors that restatement to torch.optim.LBFGS itself, its dot to an
exact rational sum, and shows on the CPU that every input below reaches the branch it is named for.

For every case THREE runs must agree bit for bit in the weights and be equal in n_iter, func_evals and the loss:
  * the restatement over the engine's own evaluation (FeedbackEngine.lossgrad + ssw_debug_fb_last_loss, the f64 loss
    the drivers compare; lossgrad2_dev for the two-output objective, whose loss is an f32 total),
  * the host driver (SSW_FB_HOST_DRIVER),
  * the one-launch driver,
and the restatement's trace -- now over the engine's evaluation, not the CPU's -- must show the case's counters.  That is
an assertion, not a skip.  The bit equality of the two drivers alone (tests/test_feedback_gpu.py) cannot see an error
in what they share: cubic_interpolate_dev and wave_sum_host (csrc/fb_math.h) serve both.

HISTORY WRAP.  The device keeps the history as a ring in global memory (head, m, slot (head + i) % FIT_HISTORY), ro[]
by slot and al[] by logical entry, four register sets prefetching three entries ahead; all of it changes behaviour at
the 101st accepted update, and no other test gets there.  Four fits of 110+ iterations with 10+ evictions: the
logistic objective with an intercept at dim 512 (nine elements a lane) and dim 768 (sixteen), RegModule's BCE at dim
512, the two-output fit (P = 1024, fit_driver_step<16>).  Once more as the middle slot of fit_batch / fit2_batch
between short fits, and a second batch on the same engines with the long fit moved to slot 0: every slot the bits of
its single fit both times, so neither a ring nor ro[] of the previous call leaks.

LINE SEARCH.  tests/_fit_driver_cases.py, LINE_CASES: fits of 17-64 rows found by a seeded search, each named for
the counters it must show (`want`).  Across them: the three bracket exits, extrapolation (lr 1e-3), the zoom's
high-end and low-end replacement, the low/high swap and the old-low-to-high move (lr 10-100), the insufficient-progress
flag and the forced step, the zoom ended by max_ls; the outer exits by max_iter, max_eval (max_iter 3, eight
evaluations in the first line search), |dloss|, the optimality test after a step and the initial one.
Best effort, all five REACHED: max_ls exhausted and the skipped update (targets of 2 on positive rows: a loss that
falls linearly for ever), zoom ended by width, g.d > -1e-9, max |d t| <= 1e-9.  None is left unreached.

LARGER SETS.  One fit of 1100 rows: host-driven only, restatement against host driver.

WHAT FAILS WHEN THE DRIVER IS WRONG (reasoned and tried on the CPU, never with a wrong kernel on a GPU): with
FIT_HISTORY = 50 both drivers drop an entry at the 51st update where the restatement keeps 100 --
test_a_shorter_history_changes_the_fit shows the weights, iterations and loss all move; indexing ro[] by the logical
entry in second_loop_step reads another entry's 1 / y.s as soon as head != 0, i.e. from the first eviction on, and
changes be, d and every later bit of the one-launch fit while the host driver and the restatement stay together.  A
CPU build of lbfgs_host around a stub objective was compared with the restatement bit for bit (weights, counts, f64
loss) on fits of 9 to 164 iterations with up to 63 evictions while this file was written.
"""
import ctypes
import os

import numpy as np
import pytest

import _fit_driver_cases as C
import _lbfgs_ref as L

pytestmark = pytest.mark.gpu
F32 = np.float32
LOSS_CODE = {"ce": 0, "hinge": 1, "logistic": 2}


# ---- engines and the three runs -----------------------------------------------------------------------
def _engine(c):
    """-> (engine, objective or None); handles are created under the lab build and closed by the test"""
    from seesaw_amd import _lib
    from seesaw_amd.feedback import FeedbackEngine
    eng = FeedbackEngine(c["dim"])
    eng.set_data(c["X"], center=False)
    eng.set_query(c["q"])
    if c["objective"] == "two":
        eng.set_targets2(c["ys"], c["sw"])
        return eng, None
    eng.set_targets(c["y"], c["sw"])
    if c["objective"] == "logreg":
        obj = _lib.FbObjective(kind=_lib.SSW_FB_LOGREG, loss_type=0, fit_intercept=c["icpt"], reg_kind=C.REG_CODE[c["reg"]],
                               pos_weight=c["pos_weight"], reg_weight=c["reg_weight"], margin=0, reg_norm_lambda=0,
                               reg_data_lambda=0, reg_query_lambda=0)
    else:
        kw = c["kw"]
        obj = _lib.FbObjective(kind=_lib.SSW_FB_MULTIREG, loss_type=LOSS_CODE[c["objective"]], fit_intercept=0, reg_kind=0,
                               pos_weight=kw["pos_weight"], reg_weight=0.0, margin=kw["margin"], reg_norm_lambda=kw["l_norm"],
                               reg_data_lambda=kw["l_data"], reg_query_lambda=kw["l_query"])
    return eng, obj


def _engine_eval(c, eng, obj):
    """the restatement's callback: one evaluation by the engine itself, the loss as the drivers see it"""
    from seesaw_amd import _lib
    dim, P = c["dim"], c["P"]
    if c["objective"] == "two":
        ln, lq = F32(c["l_norm"]), F32(c["l_query"])

        def ev(w):
            loss, grad, _ = eng.lossgrad2_dev(w.reshape(2, dim), ln, lq)
            return loss, grad.reshape(-1)          # an f32 total widened: exact
        return ev

    def ev(w):
        _, grad, _ = eng.lossgrad(obj, w[:P])
        loss = ctypes.c_double(0.0)
        _lib.call("ssw_debug_fb_last_loss", eng._h, ctypes.byref(loss))
        g = np.zeros(dim + 1, F32)
        g[:P] = grad
        return loss.value, g
    return ev


def _fit(c, eng, obj):
    if c["objective"] == "two":
        W, info = eng.fit2_dev(c["w0"].reshape(2, c["dim"]), F32(c["l_norm"]), F32(c["l_query"]), c["max_iter"], c["lr"])
        return W.reshape(-1), info
    return eng.fit(obj, c["w0"], c["max_iter"], c["lr"])


def _host_fit(c, eng, obj):
    assert "SSW_FB_HOST_DRIVER" not in os.environ
    os.environ["SSW_FB_HOST_DRIVER"] = "1"
    try:
        w, info = _fit(c, eng, obj)
    finally:
        del os.environ["SSW_FB_HOST_DRIVER"]
    assert info.pop("on_device") is False
    return w, info


def _restate(c, eng, obj):
    x, n_iter, evals, loss, tr = L.lbfgs(_engine_eval(c, eng, obj), C.start_vector(c), c["max_iter"], c["lr"],
                                         zero_slot=C.zero_slot(c))
    return x[:c["P"]], {"n_iter": n_iter, "func_evals": evals, "loss": float(F32(loss))}, tr


def _same(tag, a, b):
    (wa, ia), (wb, ib) = a, b
    assert ia == ib, (tag, ia, ib)
    assert wa.shape == wb.shape and np.array_equal(wa.view(np.uint32), wb.view(np.uint32)), \
        (tag, int((wa.view(np.uint32) != wb.view(np.uint32)).sum()), float(np.abs(wa - wb).max()))


def _three_runs(c, eng, obj, one_launch=True):
    """restatement == host driver == one-launch driver; returns (weights, info, trace)"""
    w_ref, info_ref, tr = _restate(c, eng, obj)
    print(f"  {c['name']}: {info_ref} {tr.counters()}")
    w_host, info_host = _host_fit(c, eng, obj)
    _same(f"{c['name']}: restatement vs host driver", (w_ref, info_ref), (w_host, info_host))
    if one_launch:
        w_dev, info_dev = _fit(c, eng, obj)
        assert info_dev.pop("on_device") is True
        _same(f"{c['name']}: restatement vs one-launch driver", (w_ref, info_ref), (w_dev, info_dev))
    assert np.isfinite(w_ref).all()
    return w_ref, info_ref, tr


# ---- history wrap -------------------------------------------------------------------------------------
WRAP_IDS = ("logreg-dim512", "logreg-dim768", "ce-dim512", "two-output")


@pytest.fixture(scope="module")
def wrap_cases():
    return C.wrap_cases()


@pytest.mark.parametrize("k", range(4), ids=lambda k: WRAP_IDS[k])
def test_history_wrap(lab_build, wrap_cases, k):
    c = wrap_cases[k]
    eng, obj = _engine(c)
    try:
        w, info, tr = _three_runs(c, eng, obj)
        assert info["n_iter"] >= 110 and tr.evictions >= 10, (c["name"], info, tr.counters())
        assert info["func_evals"] <= c["max_iter"] * 5 // 4
    finally:
        eng.close()


def _batch(kind, cases, engines, objs):
    from seesaw_amd.feedback import FeedbackEngine
    if kind == "two":
        dim = cases[0]["dim"]
        return FeedbackEngine.fit2_batch(engines, [c["w0"].reshape(2, dim) for c in cases], [F32(c["l_norm"]) for c in cases],
                                         [F32(c["l_query"]) for c in cases], [c["max_iter"] for c in cases],
                                         [c["lr"] for c in cases])
    return FeedbackEngine.fit_batch(engines, objs, [c["w0"] for c in cases], [c["max_iter"] for c in cases],
                                    [c["lr"] for c in cases])


@pytest.mark.parametrize("kind", ["logreg", "two"])
def test_history_wrap_as_one_slot_of_a_batch(lab_build, wrap_cases, kind):
    """short | long | short in one launch, then long | short | short on the same engines: every slot the bits of its
    single fit, and of the restatement for the long one"""
    long_case = wrap_cases[0] if kind == "logreg" else wrap_cases[3]
    cases = [C.short_case(kind, 40, 512, 21), long_case, C.short_case(kind, 33, 512, 22)]
    pairs = [_engine(c) for c in cases]
    try:
        engines, objs = [p[0] for p in pairs], [p[1] for p in pairs]
        w_ref, info_ref, tr = _restate(long_case, engines[1], objs[1])
        assert info_ref["n_iter"] >= 110 and tr.evictions >= 10, (info_ref, tr.counters())
        single = []
        for c, (eng, obj) in zip(cases, pairs):
            w, info = _fit(c, eng, obj)
            assert info.pop("on_device") is True
            single.append((w.reshape(-1), info))
        _same("long fit: restatement vs single one-launch fit", (w_ref, info_ref), single[1])
        for order in ((0, 1, 2), (1, 2, 0), (0, 1, 2)):
            res = _batch(kind, [cases[i] for i in order], [engines[i] for i in order], [objs[i] for i in order])
            for slot, i in enumerate(order):
                assert not isinstance(res[slot], Exception), res[slot]
                w, info = res[slot]
                assert info.pop("on_device") is True
                _same(f"{kind} batch order {order} slot {slot}", single[i], (w.reshape(-1), info))
    finally:
        for eng, _ in pairs:
            eng.close()


# ---- line search --------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(C.LINE_CASES)), ids=lambda k: C.LINE_CASES[k][0])
def test_line_search_branches(lab_build, k):
    c = C.line_cases()[k]
    eng, obj = _engine(c)
    try:
        w, info, tr = _three_runs(c, eng, obj)
        assert not C.reached(tr, c["want"]), (c["name"], C.reached(tr, c["want"]), tr.counters())
    finally:
        eng.close()


# ---- above the one-launch fit's reach -----------------------------------------------------------------------
def test_host_driver_alone_above_1024_rows(lab_build):
    c = C.big_case()
    eng, obj = _engine(c)
    try:
        w, info, tr = _three_runs(c, eng, obj, one_launch=False)
        w_plain, info_plain = _fit(c, eng, obj)          # without the switch the same set is host-driven too
        assert info_plain.pop("on_device") is False
        _same("plain fit above 1024 rows", (w, info), (w_plain, info_plain))
        assert info["n_iter"] >= 5 and not C.reached(tr, c["want"])
    finally:
        eng.close()

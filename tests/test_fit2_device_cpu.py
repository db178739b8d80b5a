"""CPU: the interface of the two-output device fit (header, ctypes table), SessionGroup's grouping of the multi_reg_neg
loops that opted in, the option's default, the batched refine's order of work on stubs, and a numpy restatement of the
O(dim) tail the device evaluation runs (f32, numpy's log / cosh / sinh) against the reference's captured loss and
gradient -- the tolerance tests/test_fit2_device_gpu.py holds the device to is one the arithmetic itself meets.
No GPU compute."""
import ctypes
import os
import re
import types

import numpy as np

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
TOL = 1e-4


def test_the_new_entry_points_are_declared_and_bound_with_their_signatures():
    from seesaw_amd import _lib
    from seesaw_amd.feedback import FeedbackEngine
    text = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    m = re.search(r"ssw_status\s+ssw_fb_fit2_batch\s*\((.*?)\)\s*;", text, re.S)
    assert m, "ssw_fb_fit2_batch is not declared in include/seesaw_hip.h"
    params = [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]
    assert params == ["ssw_fb *const *fbs", "int32_t nfit", "float *W_inout", "const float *reg_norm_lambda",
                      "const float *reg_query_lambda", "const int32_t *max_iter", "const float *lr", "int32_t *out_iters",
                      "int32_t *out_evals", "float *out_final_loss", "int32_t *out_status"]
    i32p, f32p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_float)
    restype, argtypes = _lib._SIGNATURES["ssw_fb_fit2_batch"]
    assert restype is ctypes.c_int32
    assert argtypes == [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int32, f32p, f32p, f32p, i32p, f32p, i32p, i32p, f32p, i32p]
    assert _lib._SIGNATURES["ssw_fb_lossgrad2_dev"] == _lib._SIGNATURES["ssw_fb_lossgrad2"]
    assert {"ssw_fb_fit2_batch", "ssw_fb_lossgrad2_dev"} <= set(_lib.declared_symbols())
    assert isinstance(FeedbackEngine.__dict__["fit2_batch"], staticmethod)


def _stub_session(loop_cls, *, started, dim=512, device=0, **attrs):
    params = types.SimpleNamespace(batch_size=3, shortlist_size=50, agg_method="plain_score", aug_larger="greater")
    loop = object.__new__(loop_cls)
    loop.params, loop.started = params, started
    loop.q = types.SimpleNamespace(index=object(), returned=set())
    loop._engine = types.SimpleNamespace(dim=dim, device=device)
    for k, v in attrs.items():
        setattr(loop, k, v)
    return types.SimpleNamespace(loop=loop, params=params, q=loop.q)


def test_fit_groups_puts_exactly_the_opted_in_loops_together():
    from seesaw_amd.loops.multi_reg import MultiReg
    from seesaw_amd.loops.multi_reg_neg import MultiRegNeg
    from seesaw_amd.loops.point_based import Plain
    from seesaw_amd.seesaw_session import SessionGroup

    class OwnRefine(MultiRegNeg):
        def refine(self, change=None):
            pass

    sessions = [
        _stub_session(MultiRegNeg, started=True, fit_on_device=True),             # 0
        _stub_session(MultiReg, started=True),                                    # 1: a launch of its own kind
        _stub_session(MultiRegNeg, started=True, fit_on_device=False),            # 2: did not opt in
        _stub_session(MultiRegNeg, started=True),                                 # 3: built before the option existed
        _stub_session(MultiRegNeg, started=True, fit_on_device=True),             # 4: with 0
        _stub_session(MultiRegNeg, started=False, fit_on_device=True),            # 5: start policy has not fired
        _stub_session(MultiRegNeg, started=True, fit_on_device=True, dim=256),    # 6: another dim
        _stub_session(MultiRegNeg, started=True, fit_on_device=True, device=1),   # 7: another device
        _stub_session(OwnRefine, started=True, fit_on_device=True),               # 8: a subclass with its own refine
        _stub_session(Plain, started=True),                                       # 9
        _stub_session(MultiReg, started=True),                                    # 10: with 1
        _stub_session(MultiRegNeg, started=True, fit_on_device=True),             # 11: with 0 and 4
    ]
    batched, alone = SessionGroup(sessions).fit_groups()
    assert batched == [(0, 4, 11), (1, 10), (6,), (7,)]
    assert alone == [2, 3, 5, 8, 9]


class _StubEngine:
    def __init__(self, dim, log, name):
        self.dim, self.device, self.log, self.name = dim, 0, log, name

    def set_query(self, q):
        self.log.append((self.name, "set_query"))

    def set_data(self, X, center):
        self.log.append((self.name, "set_data"))

    def set_targets2(self, y2, sample_weight=None):
        self.log.append((self.name, "set_targets2"))


def _loop(name, log, options, dim=8):
    """a MultiRegNeg on stubs: three labelled vectors of two images"""
    import pandas as pd
    from seesaw_amd.loops.multi_reg_neg import MultiRegNeg
    matchdf = pd.DataFrame({"dbidx": [4, 4, 9], "ys": [1.0, 0.0, 0.0]}, index=[0, 1, 2])
    box_df = pd.DataFrame({"marked_accepted": [1], "description": ["x"]})
    vectors = np.arange(3 * dim, dtype=np.float32).reshape(3, dim) / (3 * dim)
    index = types.SimpleNamespace(vectors=vectors)
    q = types.SimpleNamespace(index=index, getXy=lambda target_description=None: matchdf,
                              label_db=types.SimpleNamespace(get_box_df=lambda return_description: box_df))
    params = types.SimpleNamespace(interactive_options=options, start_policy="from_start")
    import seesaw_amd.loops.multi_reg_neg as mod
    saved = mod.FeedbackEngine
    mod.FeedbackEngine = lambda dim, device=0: _StubEngine(dim, log, name)
    try:
        loop = MultiRegNeg(None, q, params)
    finally:
        mod.FeedbackEngine = saved
    loop.curr_qvec = np.ones(dim, np.float32)
    return loop


OPTS = dict(reg_norm_lambda=100.0, reg_query_lambda=10.0, reg_data_lambda=0.0, verbose=False, max_iter=100, lr=1.0,
            matrix_options=None, discount_neg=True)


def test_multi_reg_neg_reads_the_option_and_an_absent_one_is_todays_path(monkeypatch):
    from seesaw_amd.feedback import FeedbackEngine
    log = []
    assert _loop("a", log, dict(OPTS)).fit_on_device is False
    assert _loop("a", log, dict(OPTS, fit_on_device=False)).fit_on_device is False
    assert _loop("a", log, dict(OPTS, fit_on_device=True)).fit_on_device is True
    # the module takes the loop's choice, and each choice its own engine call
    calls = []
    for name, dev in (("fit2", False), ("fit2_dev", True)):
        def fake(self, W0, l_norm, l_query, max_iter, lr=1.0, _name=name, _dev=dev):
            calls.append(_name)
            return np.asarray(W0) * 2, {"n_iter": 1, "func_evals": 2, "loss": 0.5, "on_device": _dev}
        monkeypatch.setattr(_StubEngine, name, fake, raising=False)
    for opt, want in ((dict(OPTS), "fit2"), (dict(OPTS, fit_on_device=True), "fit2_dev")):
        loop = _loop("a", log, opt)
        assert loop._model().fit_on_device is loop.fit_on_device
        loop.refine()
        assert calls[-1] == want and loop.curr_vec is not None and loop.confusion_vec is not None
    assert hasattr(FeedbackEngine, "fit2_dev") and hasattr(FeedbackEngine, "lossgrad2_dev")


def test_refine_batch_stages_loop_by_loop_and_sets_every_vector_before_a_failed_slot_raises(monkeypatch):
    import torch
    from seesaw_amd import _lib
    from seesaw_amd.feedback import FeedbackEngine
    from seesaw_amd.loops.multi_reg_neg import MultiRegNeg
    import pytest
    log = []
    loops = [_loop(n, log, dict(OPTS, fit_on_device=True)) for n in "abc"]
    del log[:]
    seen = {}

    def fake_fit2_batch(engines, W0s, l_norms, l_queries, max_iters, lrs):
        log.append(("batch", [e.name for e in engines]))
        seen["W0s"] = [np.array(w) for w in W0s]
        out = [(np.asarray(w) + 1, {"n_iter": 1, "func_evals": 2, "loss": 0.5, "on_device": True}) for w in W0s]
        out[1] = _lib.SeesawHipError(_lib.SSW_ERR_NUMERIC, "feedback: loss diverged")
        return out

    monkeypatch.setattr(FeedbackEngine, "fit2_batch", staticmethod(fake_fit2_batch))
    torch.manual_seed(3)
    with pytest.raises(AssertionError, match="regression training failed"):
        MultiRegNeg.refine_batch(loops)
    # every loop staged on its own engine, in loop order, before the one engine call
    assert log == [("a", "set_query"), ("a", "set_data"), ("a", "set_targets2"), ("b", "set_query"), ("b", "set_data"),
                   ("b", "set_targets2"), ("c", "set_query"), ("c", "set_data"), ("c", "set_targets2"),
                   ("batch", ["a", "b", "c"])]
    assert loops[0].curr_vec is not None and loops[2].confusion_vec is not None and loops[1].confusion_vec is None
    # the start weights are the ones the loops' own refine() calls would have drawn, in that order
    torch.manual_seed(3)
    from seesaw_amd.loops.multi_reg_module import _dataloader_draws, _linear_init
    for w in seen["W0s"]:
        assert np.array_equal(w, _linear_init(8))
        _dataloader_draws(3)
    MultiRegNeg.refine_batch([])  # nothing to do, nothing called
    assert log[-1] == ("batch", ["a", "b", "c"])


def _tail_numpy(W, g, qh, l_norm, l_query, vsum, hsum):
    """fb2_norm_body + fb2_tail_body of seesaw_amd/csrc/fb_math.h in numpy f32: sums over k sequential, the total
    ((labels + loss_norm) + lq0) + lq1"""
    f = np.float32
    dim = W.shape[1]
    grad, loss_norm, lq = np.zeros_like(W), f(0), []
    for c in range(2):
        ss = f(0)
        for k in range(dim):
            ss = f(ss + f(W[c, k] * W[c, k]))
        nrm = np.sqrt(ss, dtype=np.float32)
        den = max(nrm, f(1e-12))
        nw = (W[c] / den).astype(np.float32)
        nq, dotg = f(0), f(0)
        G = (g[c] - f(f(0.5) * f(l_query)) * qh).astype(np.float32)
        for k in range(dim):
            nq = f(nq + f(nw[k] * qh[k]))
            dotg = f(dotg + f(nw[k] * G[k]))
        lg = np.log(nrm, dtype=np.float32)
        loss_norm = f(loss_norm + f(np.cosh(lg, dtype=np.float32) - f(1)))
        lq.append(f(f(l_query) * f(f(f(1) - nq) / f(2))))
        radial = f(f(f(l_norm) * np.sinh(lg, dtype=np.float32)) / den)
        grad[c] = ((G - nw * dotg) / den + radial * nw).astype(np.float32)
    loss_norm = f(loss_norm * f(l_norm))
    total = f(f(f(f(vsum + hsum) + loss_norm) + lq[0]) + lq[1])
    return total, grad, np.array([loss_norm, lq[0], lq[1], vsum, hsum], np.float32)


def test_numpy_restatement_of_the_tail_meets_the_device_tests_tolerance():
    g = np.load(os.path.join(GOLDEN, "multiregneg.npz"))
    f = np.float32
    for c in range(int(g["n_cases"])):
        X, ys, W = g[f"c{c}_X"], g[f"c{c}_ys"].astype(np.float32), g[f"c{c}_w0"].astype(np.float32)
        _, inv, cnt = np.unique(g[f"c{c}_img"], return_inverse=True, return_counts=True)
        s = (1.0 / cnt[inv]).astype(np.float32)
        Xc = (X - X.astype(np.float64).mean(axis=0).astype(np.float32)).astype(np.float32)
        q = g[f"c{c}_q"].astype(np.float64)
        qh = (q / max(np.sqrt((q * q).sum()), 1e-12)).astype(np.float32)
        nw = (W / np.maximum(np.linalg.norm(W, axis=1, keepdims=True), f(1e-12))).astype(np.float32)
        z = (Xc @ nw.T).astype(np.float32)
        # the data part (fb2_row_terms): vertical BCE pair, horizontal CE where the row carries a label
        ls = np.minimum(z, 0) - np.log1p(np.exp(-np.abs(z)))
        vert = ((1 - ys) * z - ls).sum(axis=1)
        r = 1 / (1 + np.exp(-z)) - ys
        near = ys.sum(axis=1)
        m = z.max(axis=1, keepdims=True)
        lse = m + np.log(np.exp(z - m).sum(axis=1, keepdims=True))
        hor = np.where(near > 0, -(ys * (z - lse)).sum(axis=1), 0)
        r = r + np.where(near[:, None] > 0, near[:, None] * np.exp(z - lse) - ys, 0)
        vsum, hsum = f((s * vert).sum(dtype=np.float32)), f((s * hor).sum(dtype=np.float32))
        glab = ((s[:, None] * r).astype(np.float32).T @ Xc).astype(np.float32)
        loss, grad, parts = _tail_numpy(W, glab, qh, float(g[f"c{c}_l_norm"]), float(g[f"c{c}_l_query"]), vsum, hsum)
        l0, g0, p0 = float(g[f"c{c}_loss0"]), g[f"c{c}_grad0"], g[f"c{c}_parts0"]
        print(f"case {c}: loss {loss!r} vs {l0!r}; gradient diff {np.abs(grad - g0).max():.2e}; parts {parts} vs {p0}")
        assert abs(float(loss) - l0) <= TOL * max(1.0, abs(l0)), (c, loss, l0)
        assert np.abs(grad - g0).max() <= TOL * max(1.0, np.abs(g0).max()), (c, np.abs(grad - g0).max())
        assert np.allclose(parts, p0, rtol=1e-4, atol=1e-5), (c, parts, p0)

"""GPU: the batched fit (ssw_fb_fit_batch / k_fb_fit_wg_batch through FeedbackEngine.fit_batch) against the single
`fit` on fresh engines with the same inputs -- the path the reference goldens pin (tests/test_feedback_gpu.py).
The fits of a batch are independent and each lives in one workgroup, so the bar is equality: weights by
np.array_equal, `n_iter`, `func_evals` and `loss` by ==."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CE, HINGE, PLOGISTIC, LOGREG, ALLNEG = "ce", "hinge", "plogistic", "logreg", "allneg"


def _objective(kind, n):
    from seesaw_amd import _lib
    if kind == LOGREG:
        return _lib.FbObjective(kind=_lib.SSW_FB_LOGREG, loss_type=0, fit_intercept=1, reg_kind=_lib.SSW_FB_REG_VECTOR,
                                pos_weight=1.5, reg_weight=1.0 / max(n, 1), margin=0, reg_norm_lambda=0,
                                reg_data_lambda=0, reg_query_lambda=0)
    code = {CE: _lib.SSW_FB_LOSS_CE, HINGE: _lib.SSW_FB_LOSS_PAIRWISE_HINGE, ALLNEG: _lib.SSW_FB_LOSS_PAIRWISE_HINGE,
            PLOGISTIC: _lib.SSW_FB_LOSS_PAIRWISE_LOGISTIC}[kind]
    return _lib.FbObjective(kind=_lib.SSW_FB_MULTIREG, loss_type=code, fit_intercept=0, reg_kind=0, pos_weight=-1.0,
                            reg_weight=0.0, margin=0.2, reg_norm_lambda=100.0, reg_data_lambda=0.0, reg_query_lambda=10.0)


def _slot(dim, n, kind, seed, max_iter=40, lr=1.0):
    """the inputs of one fit: rows, targets, weights, query, objective, start vector"""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, dim)).astype(np.float32)
    if n:
        X /= np.linalg.norm(X, axis=1, keepdims=True)
    q = rng.standard_normal(dim).astype(np.float32)
    if kind == LOGREG:  # soft targets, as PseudoLR's
        y = rng.uniform(0, 1, n)
        y[: n // 2] = rng.uniform(size=n // 2) > 0.6
    elif kind == ALLNEG:
        y = np.zeros(n)
    else:
        y = (rng.uniform(size=n) > 0.6).astype(np.float64)
        if n >= 2:
            y[0], y[1] = 1.0, 0.0  # a positive and a negative: the pairwise losses are active
    w0 = (q / np.linalg.norm(q)).astype(np.float32)
    if kind == LOGREG:
        w0 = np.concatenate([w0 * 0.05, [0.1]]).astype(np.float32)
    return dict(dim=dim, n=n, kind=kind, X=X, y=y, sw=rng.uniform(0.5, 1.5, n) if n else None, q=q,
                obj=_objective(kind, n), w0=w0, max_iter=max_iter, lr=lr)


def _stage(eng, s):
    eng.set_query(s["q"])
    eng.set_data(s["X"], center=s["n"] > 1)
    eng.set_targets(s["y"], s["sw"])


def _single(s):
    """the single fit on a fresh engine: (w, info), or the SeesawHipError it raised"""
    from seesaw_amd import _lib
    from seesaw_amd.feedback import FeedbackEngine
    eng = FeedbackEngine(s["dim"])
    try:
        _stage(eng, s)
        return eng.fit(s["obj"], s["w0"], s["max_iter"], s["lr"])
    except _lib.SeesawHipError as e:
        return e
    finally:
        eng.close()


def _engines(slots):
    from seesaw_amd.feedback import FeedbackEngine
    engines = [FeedbackEngine(s["dim"]) for s in slots]
    for e, s in zip(engines, slots):
        _stage(e, s)
    return engines


def _batch(engines, slots):
    from seesaw_amd.feedback import FeedbackEngine
    return FeedbackEngine.fit_batch(engines, [s["obj"] for s in slots], [s["w0"] for s in slots],
                                    [s["max_iter"] for s in slots], [s["lr"] for s in slots])


def _assert_equal(got, want, slots, on_device=None):
    assert len(got) == len(want) == len(slots)
    for i, (g, w, s) in enumerate(zip(got, want, slots)):
        tag = (i, s["kind"], s["dim"], s["n"])
        assert not isinstance(w, Exception), (tag, w)
        assert not isinstance(g, Exception), (tag, g)
        (gw, gi), (ww, wi) = g, w
        assert gw.dtype == np.float32 and gw.shape == ww.shape, tag
        assert np.array_equal(gw.view(np.uint32), ww.view(np.uint32)), (tag, np.abs(gw - ww).max())
        assert gi["n_iter"] == wi["n_iter"] and gi["func_evals"] == wi["func_evals"] and gi["loss"] == wi["loss"], \
            (tag, gi, wi)
        assert sorted(gi) == sorted(wi), tag
        assert gi["on_device"] is (wi["on_device"] if on_device is None else on_device[i]), (tag, gi)


def _close(engines):
    for e in engines:
        e.close()


def test_one_launch_mixing_objectives_and_set_sizes():
    """n = 0 (regularisers only), 1, 15 / 16 / 17 (around the one-pass unit of 16 rows), 390 and the cap, under the
    multireg CE, pairwise hinge (margin 0.2), pairwise logistic and intercept-logistic objectives, plus all-negative
    pairwise slots (label_mode 3): one launch, every slot its single fit"""
    slots, seed = [], 0
    for n in (0, 1, 15, 16, 17, 390, 1024):
        for kind in (CE, LOGREG):
            slots.append(_slot(512, n, kind, seed := seed + 1))
    for n in (15, 17, 390, 1024):
        slots.append(_slot(512, n, HINGE, seed := seed + 1))
    for n in (16, 390):
        slots.append(_slot(512, n, PLOGISTIC, seed := seed + 1))
    for n in (17, 390):
        slots.append(_slot(512, n, ALLNEG, seed := seed + 1))
    want = [_single(s) for s in slots]
    engines = _engines(slots)
    _assert_equal(_batch(engines, slots), want, slots, on_device=[True] * len(slots))
    assert sum(w[1]["func_evals"] for w in want) > 5 * len(slots)
    _close(engines)


def test_a_slot_beyond_the_row_cap_runs_through_the_single_path():
    slots = [_slot(512, 390, CE, 101), _slot(512, 1025, LOGREG, 102, max_iter=12), _slot(512, 17, HINGE, 103)]
    want = [_single(s) for s in slots]
    assert [w[1]["on_device"] for w in want] == [True, False, True]
    engines = _engines(slots)
    _assert_equal(_batch(engines, slots), want, slots, on_device=[True, False, True])
    _close(engines)


@pytest.mark.parametrize("dim", [256, 768])
def test_other_dims(dim):
    """dim 256: nine elements a lane in the driver, the two-pass evaluation; dim 768: sixteen"""
    slots = [_slot(dim, n, kind, 200 + dim + i) for i, (n, kind) in enumerate(
        [(0, CE), (1, LOGREG), (16, CE), (70, PLOGISTIC), (90, HINGE), (390, CE), (390, LOGREG), (33, ALLNEG)])]
    want = [_single(s) for s in slots]
    engines = _engines(slots)
    _assert_equal(_batch(engines, slots), want, slots, on_device=[True] * len(slots))
    _close(engines)


def test_more_slots_than_compute_units():
    """at 160 KB of LDS a compute unit holds one fit workgroup: the slots beyond the CU count queue"""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    slots = [_slot(512, 5, CE if i % 3 else LOGREG, 1000 + i, max_iter=20) for i in range(cus + 5)]
    want = [_single(s) for s in slots]
    engines = _engines(slots)
    _assert_equal(_batch(engines, slots), want, slots, on_device=[True] * len(slots))
    _close(engines)


def test_a_diverging_slot_leaves_its_row_and_its_neighbours_alone():
    from seesaw_amd import _lib
    from seesaw_amd.feedback import FeedbackEngine
    slots = [_slot(512, 33, CE, 301), _slot(512, 40, CE, 302), _slot(512, 17, LOGREG, 303)]
    slots[1]["X"][7, 3] = np.nan
    want = [_single(s) for s in slots]
    assert isinstance(want[1], _lib.SeesawHipError) and want[1].status == _lib.SSW_ERR_NUMERIC
    engines = _engines(slots)
    got = _batch(engines, slots)
    assert isinstance(got[1], _lib.SeesawHipError) and got[1].status == _lib.SSW_ERR_NUMERIC
    assert str(got[1]) == str(want[1])
    _assert_equal([got[0], got[2]], [want[0], want[2]], [slots[0], slots[2]])
    # at the C interface: SSW_ERR_NUMERIC for that slot alone, its row of W untouched, the call itself SSW_OK
    W = np.zeros((3, 513), np.float32)
    for i, s in enumerate(slots):
        W[i, : s["w0"].shape[0]] = s["w0"]
    W[1, 512] = 7.25  # not a parameter of that slot: stays as well
    before = W.copy()
    _, _, _, status = FeedbackEngine._fit_batch_raw(engines, [s["obj"] for s in slots], W, [s["max_iter"] for s in slots],
                                                     [s["lr"] for s in slots])
    assert status.tolist() == [_lib.SSW_OK, _lib.SSW_ERR_NUMERIC, _lib.SSW_OK]
    assert np.array_equal(W[1].view(np.uint32), before[1].view(np.uint32))
    assert np.array_equal(W[0, :512].view(np.uint32), want[0][0].view(np.uint32))
    assert np.array_equal(W[2].view(np.uint32), want[2][0].view(np.uint32))
    _close(engines)


def test_a_second_batch_on_the_same_engines_without_a_reset():
    """sequence numbers and completion words carry over: the same engines, another order (another engine leads the
    launch), new start vectors, one engine with new data"""
    slots = [_slot(512, n, kind, 400 + i) for i, (n, kind) in enumerate([(390, CE), (16, LOGREG), (17, HINGE), (0, CE)])]
    engines = _engines(slots)
    _assert_equal(_batch(engines, slots), [_single(s) for s in slots], slots)
    order = [2, 0, 3, 1]
    slots2 = [dict(slots[i], w0=(slots[i]["w0"] * 0.5).astype(np.float32), max_iter=25) for i in order]
    slots2[1] = dict(_slot(512, 45, CE, 450), max_iter=25)
    engines2 = [engines[i] for i in order]
    _stage(engines2[1], slots2[1])
    _assert_equal(_batch(engines2, slots2), [_single(s) for s in slots2], slots2)
    w, info = engines[1].fit(slots[1]["obj"], slots[1]["w0"], slots[1]["max_iter"])  # and the single call after a batch
    _assert_equal([(w, info)], [_single(slots[1])], [slots[1]])
    _close(engines)


def test_refusals_launch_nothing_and_the_engines_still_fit():
    from seesaw_amd import _lib
    from seesaw_amd.feedback import FeedbackEngine
    slots = [_slot(512, 20, CE, 501), _slot(512, 31, LOGREG, 502)]
    engines = _engines(slots)
    other = _slot(256, 20, CE, 503)
    eng256 = _engines([other])[0]
    with pytest.raises(_lib.SeesawHipError, match="dim") as ei:
        _batch(engines + [eng256], slots + [other])
    assert ei.value.status == _lib.SSW_ERR_INVALID
    with pytest.raises(_lib.SeesawHipError, match="share one handle"):
        _batch([engines[0], engines[1], engines[0]], [slots[0], slots[1], slots[0]])
    with pytest.raises(_lib.SeesawHipError, match="nfit"):
        FeedbackEngine.fit_batch([], [], [], [], [])
    bad = dict(slots[1], w0=slots[1]["w0"].copy())
    bad["w0"][100] = np.inf
    with pytest.raises(_lib.SeesawHipError, match="not finite"):
        _batch(engines, [slots[0], bad])
    with pytest.raises(_lib.SeesawHipError, match="max_iter"):
        _batch(engines, [slots[0], dict(slots[1], max_iter=0)])
    # a refused call took no sequence number and left no launch behind: the single and the batched fit go on as before
    want = [_single(s) for s in slots]
    _assert_equal([e.fit(s["obj"], s["w0"], s["max_iter"]) for e, s in zip(engines, slots)], want, slots)
    _assert_equal(_batch(engines, slots), want, slots)
    _close(engines + [eng256])

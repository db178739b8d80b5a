"""GPU: the two-output (multi_reg_neg) objective evaluated and fitted entirely on the device -- ssw_fb_lossgrad2_dev,
ssw_fb_fit2_batch (k_fb_fit2_wg / k_fb_fit2_wg_batch), MultiRegModule(fit_on_device=True), MultiRegNeg.refine_batch
and SessionGroup -- against the reference's captures (tests/golden/multiregneg.npz), against the host-driven fit over
the same device evaluation (bit for bit), and batched against single (bit for bit)."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
TOL = 1e-4  # the tolerance tests/test_multiregneg_gpu.py holds the host tail to


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(GOLDEN, "multiregneg.npz"))


def _module(g, c):
    import pandas as pd
    from seesaw_amd.loops.multi_reg_module import MultiRegModule
    m = MultiRegModule(qvec=g[f"c{c}_q"], reg_norm_lambda=float(g[f"c{c}_l_norm"]), reg_query_lambda=float(g[f"c{c}_l_query"]),
                       max_iter=100, lr=1.0, weight0=g[f"c{c}_w0"], fit_on_device=True)
    matchdf = pd.DataFrame({"dbidx": g[f"c{c}_img"]})
    return m, matchdf


# ---- test 1: the device evaluation against the reference --------------------------------------------------------
def test_device_evaluation_at_w0_and_along_the_reference_trajectory(g):
    for c in range(int(g["n_cases"])):
        m, matchdf = _module(g, c)
        m._install(g[f"c{c}_X"], g[f"c{c}_ys"], matchdf)
        loss, grad, parts = m.lossgrad(g[f"c{c}_w0"])
        l0, g0, p0 = float(g[f"c{c}_loss0"]), g[f"c{c}_grad0"], g[f"c{c}_parts0"]
        print(f"case {c}: loss {loss!r} vs {l0!r}; gradient diff {np.abs(grad - g0).max():.2e}; parts {parts} vs {p0}")
        assert abs(loss - l0) <= TOL * max(1.0, abs(l0)), (c, loss, l0)
        assert np.abs(grad - g0).max() <= TOL * max(1.0, np.abs(g0).max()), (c, np.abs(grad - g0).max())
        assert np.allclose(parts, p0, rtol=1e-4, atol=1e-5), (c, parts, p0)
        TW, TL, TG = g[f"c{c}_traj_w"], g[f"c{c}_traj_loss"], g[f"c{c}_traj_grad"]
        worst_l = worst_g = 0.0
        for t in range(TW.shape[0]):
            loss, grad, _ = m.lossgrad(TW[t].reshape(2, -1))
            worst_l = max(worst_l, abs(loss - TL[t]) / max(1.0, abs(TL[t])))
            worst_g = max(worst_g, np.abs(grad.reshape(-1) - TG[t]).max() / max(1.0, np.abs(TG[t]).max()))
        print(f"case {c}: {TW.shape[0]} closure evaluations, worst relative loss diff {worst_l:.2e}, gradient {worst_g:.2e}")
        assert worst_l <= TOL and worst_g <= TOL, (c, worst_l, worst_g)


# ---- synthetic labelled sets ------------------------------------------------------------------------------------
def _slot(dim, n, seed, labels="mixed", weights="images", max_iter=100, lr=1.0, l_norm=100.0, l_query=10.0):
    rng = np.random.default_rng(seed)
    centre = rng.standard_normal(dim)
    X = (rng.standard_normal((n, dim)) + 0.5 * centre).astype(np.float32)
    X /= np.maximum(np.linalg.norm(X, axis=1, keepdims=True), 1e-12)
    q = (centre + 0.3 * rng.standard_normal(dim)).astype(np.float32)
    y0 = (X @ (centre / np.linalg.norm(centre)) > np.median(X @ centre / np.linalg.norm(centre)) if n else np.zeros(0, bool))
    y1 = (~y0) & (rng.random(n) < 0.4)
    if labels == "none":  # no row carries a label: the horizontal term is never taken
        y0, y1 = np.zeros(n, bool), np.zeros(n, bool)
    elif labels == "all":  # every row carries one
        y1 = ~y0
    ys = np.stack([y0, y1], axis=1).astype(np.float32)
    if weights == "images":  # 1 / (vectors of the same image), images of one to four vectors
        img = np.sort(rng.integers(0, max(1, n // 2), n))
        _, inv, cnt = np.unique(img, return_inverse=True, return_counts=True)
        sw = (1.0 / cnt[inv]).astype(np.float32)
    else:  # anything but uniform
        sw = rng.uniform(0.05, 3.0, n).astype(np.float32)
    w0 = (rng.uniform(-1, 1, (2, dim)) / np.sqrt(dim)).astype(np.float32)  # nn.Linear's range
    return dict(dim=dim, n=n, X=X, ys=ys, sw=sw, q=q, w0=w0, max_iter=max_iter, lr=lr, l_norm=l_norm, l_query=l_query)


def _stage(eng, s):
    eng.set_data(s["X"], center=s["n"] > 0)
    if s["n"] > 0:  # a set of 0 rows needs no targets: the regularisers alone
        eng.set_targets2(s["ys"], s["sw"])
    eng.set_query(s["q"])


def _fit(eng, s):
    return eng.fit2_dev(s["w0"], s["l_norm"], s["l_query"], max_iter=s["max_iter"], lr=s["lr"])


def _fit_both_drivers(eng, s):
    """(W, info) of the one-launch fit (k_fb_fit2_wg) and of the host-driven fit over the device evaluation"""
    assert "SSW_FB_HOST_DRIVER" not in os.environ
    dev = _fit(eng, s)
    os.environ["SSW_FB_HOST_DRIVER"] = "1"
    try:
        host = _fit(eng, s)
    finally:
        del os.environ["SSW_FB_HOST_DRIVER"]
    return dev, host


def _assert_same_fit(a, b, tag):
    (Wa, ia), (Wb, ib) = a, b
    assert np.array_equal(Wa.view(np.uint32), Wb.view(np.uint32)), (tag, np.abs(Wa - Wb).max(), ia, ib)
    assert ia["n_iter"] == ib["n_iter"] and ia["func_evals"] == ib["func_evals"], (tag, ia, ib)
    assert np.array_equal(np.float32(ia["loss"]).view(np.uint32), np.float32(ib["loss"]).view(np.uint32)), (tag, ia, ib)


# ---- test 2: the two drivers agree bit for bit -------------------------------------------------------------------
def test_one_launch_fit_is_the_host_driven_fit_on_the_golden_cases(g):
    from seesaw_amd.feedback import FeedbackEngine
    for c in range(int(g["n_cases"])):
        X = g[f"c{c}_X"]
        _, inv, cnt = np.unique(g[f"c{c}_img"], return_inverse=True, return_counts=True)
        s = dict(dim=X.shape[1], n=X.shape[0], X=X, ys=g[f"c{c}_ys"], sw=(1.0 / cnt[inv]), q=g[f"c{c}_q"], w0=g[f"c{c}_w0"],
                 max_iter=100, lr=1.0, l_norm=float(g[f"c{c}_l_norm"]), l_query=float(g[f"c{c}_l_query"]))
        eng = FeedbackEngine(s["dim"])
        _stage(eng, s)
        dev, host = _fit_both_drivers(eng, s)
        print(f"golden case {c}: n={s['n']} dim={s['dim']} {dev[1]}")
        assert dev[1]["on_device"] is True and host[1]["on_device"] is False
        assert dev[1]["n_iter"] >= 2 and dev[1]["func_evals"] > dev[1]["n_iter"]
        _assert_same_fit(dev, host, c)
        eng.close()


EDGES = [(512, n, "mixed", "images", 100) for n in (0, 1, 31, 32, 33, 255, 256, 257, 1024)] + [
    (256, 0, "mixed", "images", 100), (256, 33, "mixed", "images", 100), (256, 257, "all", "random", 100),
    (512, 100, "none", "images", 100), (512, 100, "all", "images", 100), (512, 97, "mixed", "random", 100),
    (512, 65, "mixed", "images", 1), (256, 1024, "mixed", "random", 1)]


@pytest.mark.parametrize("dim,n,labels,weights,max_iter", EDGES)
def test_one_launch_fit_is_the_host_driven_fit_at_the_edges(dim, n, labels, weights, max_iter):
    from seesaw_amd.feedback import FeedbackEngine
    s = _slot(dim, n, 1000 + n + dim, labels=labels, weights=weights, max_iter=max_iter)
    if labels == "none":
        assert not (s["ys"].sum(axis=1) > 0).any()
    if labels == "all":
        assert (s["ys"].sum(axis=1) > 0).all()
    eng = FeedbackEngine(dim)
    _stage(eng, s)
    dev, host = _fit_both_drivers(eng, s)
    print(f"dim={dim} n={n} {labels} {weights} max_iter={max_iter}: {dev[1]}")
    assert dev[1]["on_device"] is True and host[1]["on_device"] is False
    assert dev[1]["n_iter"] >= 1 and (max_iter > 1 or dev[1]["n_iter"] == 1)
    assert np.isfinite(dev[0]).all() and not np.array_equal(dev[0], s["w0"])
    _assert_same_fit(dev, host, (dim, n, labels, weights, max_iter))
    # and the fit went downhill on the objective the device evaluation states
    l0, _, _ = eng.lossgrad2_dev(s["w0"], s["l_norm"], s["l_query"])
    l1, _, _ = eng.lossgrad2_dev(dev[0], s["l_norm"], s["l_query"])
    assert l1 < l0, (l0, l1)
    eng.close()


def test_a_set_beyond_one_workgroup_takes_the_host_driven_device_evaluation():
    from seesaw_amd.feedback import FeedbackEngine
    s = _slot(512, 1025, 77, max_iter=30)
    eng = FeedbackEngine(512)
    _stage(eng, s)
    W, info = _fit(eng, s)
    assert info["on_device"] is False and info["n_iter"] >= 2 and np.isfinite(W).all()
    l0, _, _ = eng.lossgrad2_dev(s["w0"], s["l_norm"], s["l_query"])
    l1, _, _ = eng.lossgrad2_dev(W, s["l_norm"], s["l_query"])
    assert l1 < l0
    eng.close()


# ---- test 3: the end point against the reference ---------------------------------------------------------------
def test_device_fit_reaches_the_reference_end_point(g):
    """test_fit_reaches_the_reference_end_point's criterion (tests/test_multiregneg_gpu.py) on the device fit.
    Measured on an MI355X: see the figures this test prints; the criterion's numbers are that test's."""
    for c in range(int(g["n_cases"])):
        m, matchdf = _module(g, c)
        X = g[f"c{c}_X"]
        m.fit(X, g[f"c{c}_ys"], matchdf)
        assert m.info_["on_device"] is True
        loss, _, _ = m.lossgrad()
        ref_final = float(g[f"c{c}_traj_loss"][-1])
        Xc = X - X.mean(axis=0)
        nrm = lambda W: W / np.linalg.norm(W, axis=1, keepdims=True)  # noqa: E731
        ref = g[f"c{c}_weight_seeds"]
        spread = max(np.abs(Xc @ (nrm(ref[0]) - nrm(r)).T).max() for r in ref)
        d = min(np.abs(Xc @ (nrm(m.weight) - nrm(r)).T).max() for r in ref)
        print(f"multiregneg case {c} (device fit): loss {loss:.6f} vs reference {ref_final:.6f}; rank-score distance to the "
              f"nearest reference seed {d:.2e} (its own seeds {spread:.2e} apart); {m.info_}")
        assert loss <= ref_final * (1 + 2e-6) + 1e-6, (c, loss, ref_final)
        assert d <= max(5e-4, 2 * spread), (c, d, spread)
        assert np.abs(m.get_coeff() - nrm(m.weight)[0]).max() <= 1e-6


# ---- test 4: the batch equals the single fits --------------------------------------------------------------------
def _engines(slots):
    from seesaw_amd.feedback import FeedbackEngine
    engines = [FeedbackEngine(s["dim"]) for s in slots]
    for e, s in zip(engines, slots):
        _stage(e, s)
    return engines


def _single(s):
    from seesaw_amd import _lib
    (e,) = _engines([s])
    try:
        return _fit(e, s)
    except _lib.SeesawHipError as err:
        return err
    finally:
        e.close()


def _batch(engines, slots):
    from seesaw_amd.feedback import FeedbackEngine
    return FeedbackEngine.fit2_batch(engines, [s["w0"] for s in slots], [s["l_norm"] for s in slots],
                                     [s["l_query"] for s in slots], [s["max_iter"] for s in slots], [s["lr"] for s in slots])


@pytest.mark.parametrize("nfit", [1, 2, 5])
def test_every_slot_of_a_batch_is_its_single_fit(nfit):
    shapes = [(1024, "mixed", "images", 60, 1.0, 100.0, 10.0), (0, "mixed", "images", 100, 1.0, 50.0, 5.0),
              (33, "all", "random", 100, 0.5, 100.0, 10.0), (257, "none", "images", 7, 1.0, 10.0, 20.0),
              (100, "mixed", "random", 100, 1.0, 100.0, 0.0)][:nfit]
    slots = [_slot(512, n, 2000 + i, labels=lb, weights=wt, max_iter=mi, lr=lr, l_norm=ln, l_query=lq)
             for i, (n, lb, wt, mi, lr, ln, lq) in enumerate(shapes)]
    want = [_single(s) for s in slots]
    engines = _engines(slots)
    got = _batch(engines, slots)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a[1]["on_device"] is True and b[1]["on_device"] is True
        _assert_same_fit(a, b, (nfit, i))
    # a second batch on the same engines, another engine leading: sequence numbers and completion words carry over
    order = list(reversed(range(nfit)))
    got2 = _batch([engines[i] for i in order], [slots[i] for i in order])
    for i, a in zip(order, got2):
        _assert_same_fit(a, want[i], (nfit, i, "again"))
    for e in engines:
        e.close()


def test_a_slot_beyond_the_row_cap_is_driven_from_the_host_afterwards():
    slots = [_slot(256, 40, 3001), _slot(256, 1025, 3002, max_iter=25), _slot(256, 77, 3003, weights="random")]
    want = [_single(s) for s in slots]
    engines = _engines(slots)
    got = _batch(engines, slots)
    assert [r[1]["on_device"] for r in got] == [True, False, True]
    for i, (a, b) in enumerate(zip(got, want)):
        _assert_same_fit(a, b, i)
    for e in engines:
        e.close()


def test_a_diverging_slot_leaves_its_row_and_its_neighbours_alone():
    """a NaN among a slot's rows makes its first loss NaN, deterministically: that slot comes back SSW_ERR_NUMERIC"""
    from seesaw_amd import _lib
    slots = [_slot(512, 33, 4001), _slot(512, 40, 4002), _slot(512, 0, 4003)]
    slots[1]["X"][7, 3] = np.nan
    want = [_single(s) for s in slots]
    assert isinstance(want[1], _lib.SeesawHipError) and want[1].status == _lib.SSW_ERR_NUMERIC
    engines = _engines(slots)
    got = _batch(engines, slots)
    assert isinstance(got[1], _lib.SeesawHipError) and got[1].status == _lib.SSW_ERR_NUMERIC
    assert str(got[1]) == str(want[1])
    _assert_same_fit(got[0], want[0], 0)
    _assert_same_fit(got[2], want[2], 2)
    # at the C interface: that slot's row of W stays as it came and the call itself is SSW_OK
    import ctypes
    W = np.stack([s["w0"] for s in slots]).astype(np.float32)
    before = W.copy()
    handles = (ctypes.c_void_p * 3)(*[e._h for e in engines])
    f32 = lambda a: np.asarray(a, np.float32).ctypes.data_as(_lib.c_f32_p)  # noqa: E731
    ln, lq, lr = (np.array([s[k] for s in slots], np.float32) for k in ("l_norm", "l_query", "lr"))
    mi, status = np.array([s["max_iter"] for s in slots], np.int32), np.full(3, 99, np.int32)
    _lib.call("ssw_fb_fit2_batch", handles, 3, W.ctypes.data_as(_lib.c_f32_p), f32(ln), f32(lq), mi.ctypes.data_as(_lib.c_i32_p),
              f32(lr), None, None, None, status.ctypes.data_as(_lib.c_i32_p))
    assert status.tolist() == [_lib.SSW_OK, _lib.SSW_ERR_NUMERIC, _lib.SSW_OK]
    assert np.array_equal(W[1].view(np.uint32), before[1].view(np.uint32))
    assert np.array_equal(W[0].view(np.uint32), want[0][0].view(np.uint32))
    assert np.array_equal(W[2].view(np.uint32), want[2][0].view(np.uint32))
    for e in engines:
        e.close()


def test_refusals_queue_nothing_and_the_engines_still_fit():
    from seesaw_amd import _lib
    from seesaw_amd.feedback import FeedbackEngine
    slots = [_slot(256, 20, 5001), _slot(256, 31, 5002)]
    engines = _engines(slots)
    other = _slot(512, 20, 5003)
    eng512 = _engines([other])[0]
    with pytest.raises(_lib.SeesawHipError, match="dim") as ei:
        _batch(engines + [eng512], slots + [other])
    assert ei.value.status == _lib.SSW_ERR_INVALID
    with pytest.raises(_lib.SeesawHipError, match="share one handle"):
        _batch([engines[0], engines[1], engines[0]], [slots[0], slots[1], slots[0]])
    with pytest.raises(_lib.SeesawHipError, match="nfit"):
        FeedbackEngine.fit2_batch([], [], [], [], [], [])
    bad = dict(slots[1], w0=slots[1]["w0"].copy())
    bad["w0"][1, 100] = np.inf
    with pytest.raises(_lib.SeesawHipError, match="not finite"):
        _batch(engines, [slots[0], bad])
    with pytest.raises(_lib.SeesawHipError, match="max_iter"):
        _batch(engines, [slots[0], dict(slots[1], max_iter=0)])
    big = FeedbackEngine(768)  # 2 dim > 1024
    big.set_data(np.zeros((0, 768), np.float32), center=False)
    big.set_query(np.ones(768, np.float32))
    with pytest.raises(_lib.SeesawHipError, match="dim <= 512"):
        FeedbackEngine.fit2_batch([big], [np.ones((2, 768), np.float32)], [1.0], [1.0], [5], [1.0])
    no_targets, no_query = FeedbackEngine(256), FeedbackEngine(256)
    no_targets.set_data(slots[0]["X"], center=True)
    no_targets.set_query(slots[0]["q"])
    with pytest.raises(_lib.SeesawHipError, match="ssw_fb_set_targets2"):
        _batch([engines[0], no_targets], slots)
    no_query.set_data(slots[0]["X"], center=True)
    no_query.set_targets2(slots[0]["ys"], slots[0]["sw"])
    with pytest.raises(_lib.SeesawHipError, match="ssw_fb_set_query"):
        _batch([engines[0], no_query], slots)
    # a refused call took no sequence number and left no launch behind: the fits go on as before
    want = [_single(s) for s in slots]
    for a, b in zip(_batch(engines, slots), want):
        _assert_same_fit(a, b, "after the refusals")
    for e in engines + [eng512, big, no_targets, no_query]:
        e.close()


# ---- test 5: sessions against the reference ---------------------------------------------------------------------
@pytest.mark.parametrize("name", ["multi_reg_neg", "multi_reg_neg_nodiscount"])
def test_session_sequence_matches_reference_with_the_device_fit(g, name):
    """test_session_sequence_matches_reference (tests/test_multiregneg_gpu.py) with fit_on_device=True: the same
    stable-prefix rule against the reference's own runs"""
    import torch
    import seesaw_amd.seesaw_bench as sb
    from seesaw_amd.basic_types import BenchParams, IndexSpec, SessionParams
    from seesaw_amd.bitmap import BitMap
    from seesaw_amd.loops.multi_reg_neg import MultiRegNeg
    from seesaw_amd.seesaw_session import make_session
    from seesaw_amd.synthetic import GlobalDataManager, make_dataset
    gb = np.load(os.path.join(GOLDEN, "bench_loop.npz"))
    spec = json.loads(str(gb["datasets"]))["A"]
    ds = make_dataset("lvis", knn_k=0, **spec["make"])
    ds.embedding.noise = spec["noise"]
    gdm = GlobalDataManager().add(ds)
    opts = dict(reg_norm_lambda=100.0, reg_query_lambda=10.0, reg_data_lambda=0.0, verbose=False, max_iter=100, lr=1.0,
                matrix_options=None, discount_neg=(name == "multi_reg_neg"), fit_on_device=True)
    p = SessionParams(index_spec=IndexSpec(d_name="lvis", i_name="multiscale", c_name=None), interactive="multi_reg_neg",
                      interactive_options=opts, shortlist_size=50, agg_method="plain_score", aug_larger="greater",
                      batch_size=1, start_policy="after_first_batch", index_options={"use_vec_index": False})
    b = BenchParams(name=name, ground_truth_category="c1", qstr="a c1", n_batches=25, max_results=10,
                    provide_textual_feedback=True)
    old = dict(sb.objnet_dict)
    sb.objnet_dict.update(json.loads(str(g["confusion"])))
    try:
        np.random.seed(0)
        torch.manual_seed(0)
        ret = make_session(gdm, p, b=b)
        assert isinstance(ret["session"].loop, MultiRegNeg) and ret["session"].loop.fit_on_device is True
        boxes, _ = ds.load_ground_truth()
        out = sb.benchmark_loop(session=ret["session"], box_data=boxes, subset=BitMap(ds.file_meta.index.values), b=b, p=p)
    finally:
        sb.objnet_dict.clear()
        sb.objnet_dict.update(old)
    shown = np.concatenate([np.asarray(a, dtype=np.int64).reshape(-1) for a in ret["session"].acc_indices])
    ref = g[f"{name}_shown"]
    seqs = [ref] + [g[f"{name}_shown_seed{s}"] for s in g["session_seeds"][1:]]
    stable = 0
    while stable < min(len(x) for x in seqs) and all(x[stable] == ref[stable] for x in seqs):
        stable += 1
    same = 0
    while same < min(len(shown), len(ref)) and shown[same] == ref[same]:
        same += 1
    print(f"{name} (device fit): reference reproduces itself over {stable} of {len(ref)} rounds; ours equals it over {same}")
    assert np.array_equal(shown[:stable], ref[:stable]), (shown.tolist(), ref.tolist())
    if stable == len(ref):
        assert out["nfound"] == int(g[f"{name}_nfound"]) and out["nseen"] == int(g[f"{name}_nseen"])


# ---- test 6: SessionGroup ---------------------------------------------------------------------------------------
ROUNDS = 5
NEG = dict(reg_norm_lambda=100.0, reg_query_lambda=10.0, reg_data_lambda=0.0, verbose=False, max_iter=100, lr=1.0,
           matrix_options=None, discount_neg=True)
MULTI_REG = dict(label_loss_type="ce_loss", rank_loss_margin=0.2, use_qvec_norm=None, reg_data_lambda=0.0,
                 reg_norm_lambda=100.0, reg_query_lambda=0.0, verbose=False, max_iter=200, pos_weight="balanced",
                 lr=1.0, matrix_options=None)
# (loop, options, text, the category the simulated user labels, start policy).  The loops that draw from torch's global
# generator (every multi_reg_neg builds an nn.Linear a refine) stand in the order a group refines them: the batch first
GROUP = [("multi_reg_neg", dict(NEG, fit_on_device=True), "a c0", "c0", "after_first_batch"),
         ("multi_reg_neg", dict(NEG, fit_on_device=True, discount_neg=False), "a c1", "c1", "after_first_batch"),
         ("multi_reg_neg", dict(NEG, fit_on_device=True, reg_query_lambda=3.0), "a c2", "c2", "after_first_batch"),
         ("multi_reg_neg", dict(NEG, fit_on_device=True, max_iter=40), "a c0", "c2", "after_first_positive"),
         ("multi_reg_neg", dict(NEG), "a c1", "c1", "after_first_batch"),
         ("multi_reg", MULTI_REG, "a c2", "c2", "after_first_batch")]


@pytest.fixture(scope="module")
def grp():
    from seesaw_amd.synthetic import GlobalDataManager, make_dataset
    ds = make_dataset("grp2", n_images=200, tiles_per_image=13, n_categories=3, positive_frac=0.08, seed=21, knn_k=0)
    return GlobalDataManager().add(ds), ds


def _label(session, category, ds):
    """the simulated user of benchmark_loop: the ground-truth boxes of `category` on the batch just shown"""
    from seesaw_amd.basic_types import BenchParams
    from seesaw_amd.seesaw_bench import _group_boxes, fill_imdata
    b = BenchParams(name="grp2", ground_truth_category=category, qstr=f"a {category}", n_batches=ROUNDS)
    boxes = ds.box_data.assign(description=ds.box_data.category)
    boxes = boxes[boxes.category == category]
    groups = _group_boxes(boxes)
    session.update_last_batch([fill_imdata(im, boxes, b, _groups=groups) for im in session.last_batch()])


def _run_group(gdm, ds, grouped, calls):
    import torch
    from seesaw_amd.basic_types import IndexSpec, SessionParams
    from seesaw_amd.seesaw_session import SessionGroup, make_session
    np.random.seed(5)
    torch.manual_seed(5)
    sessions = []
    for loop, options, text, _, policy in GROUP:
        p = SessionParams(index_spec=IndexSpec(d_name="grp2", i_name="multiscale", c_name=None), interactive=loop,
                          interactive_options=options, batch_size=3, shortlist_size=50, agg_method="plain_score",
                          aug_larger="greater", start_policy=policy, index_options={"use_vec_index": False})
        s = make_session(gdm, p)["session"]
        s.set_text(text)
        sessions.append(s)
    group = SessionGroup(sessions)
    trace = []
    for _ in range(ROUNDS):
        if grouped:
            group.next()
        else:
            for s in sessions:
                s.next()
        for s, spec in zip(sessions, GROUP):
            _label(s, spec[3], ds)
        if grouped:
            group.refine()
            calls.append(group.fit_groups())
        else:
            for s in sessions:
                s.refine()
        u32 = lambda v: None if v is None else np.asarray(v, dtype=np.float32).copy().view(np.uint32)  # noqa: E731
        trace.append([dict(curr_vec=u32(s.loop.curr_vec), confusion_vec=u32(getattr(s.loop, "confusion_vec", None)),
                           acc_indices=np.asarray(s.acc_indices[-1]).copy(), returned=np.array(s.q.returned).copy(),
                           started=s.loop.started, log=[e[1:] for e in s._log_raw]) for s in sessions])
    return trace


def test_session_group_refines_the_opted_in_loops_together(grp):
    gdm, ds = grp
    calls = []
    alone = _run_group(gdm, ds, False, calls)
    together = _run_group(gdm, ds, True, calls)
    for r, (ra, rt) in enumerate(zip(alone, together)):
        for i, (a, t) in enumerate(zip(ra, rt)):
            tag = (r, i, GROUP[i][0])
            assert a["started"] == t["started"], tag
            for k in ("curr_vec", "confusion_vec"):
                assert (a[k] is None) == (t[k] is None), (tag, k)
                if a[k] is not None:
                    assert np.array_equal(a[k], t[k]), (tag, k)
            assert np.array_equal(a["acc_indices"], t["acc_indices"]), tag
            assert np.array_equal(a["returned"], t["returned"]), tag
            assert a["log"] == t["log"], tag
    # exactly the opted-in, started multi_reg_neg loops refined in one batch; the one that did not opt in on its own;
    # the multi_reg loop in a group of its own kind
    late = [rt[3]["started"] for rt in together]  # the after_first_positive session, after each round's refine
    for (batched, on_their_own), started in zip(calls, late):
        assert sorted(batched) == [(0, 1, 2, 3) if started else (0, 1, 2), (5,)], (batched, late)
        assert on_their_own == ([4] if started else [3, 4]), (on_their_own, late)
    # the fits moved both vectors, differently per session
    vecs = [together[-1][i] for i in range(4)]
    assert all(v["confusion_vec"] is not None for v in vecs)
    assert not np.array_equal(vecs[0]["curr_vec"], vecs[1]["curr_vec"])
    assert not np.array_equal(together[0][0]["curr_vec"], together[-1][0]["curr_vec"])

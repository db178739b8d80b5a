"""GPU: SessionGroup with graph loops.  The started knn_prop2 sessions of one index refine through ONE
KnnProp2.refine_batch (one ssw_labelprop_round_batch: the propagations, scores and selections of all of them in one
call); against the same sessions run independently every session keeps, per round, the same dbidxs, activations,
`returned` set, log, timing count, `curr_vec` bits and propagated f64 scores."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROUNDS = 6
MATRIX = dict(knn_path="nndescent60", symmetric=True, self_edges=False, normalized_weights=False, knn_k=10, edist=0.05)
MULTI_REG = dict(label_loss_type="ce_loss", rank_loss_margin=0.2, use_qvec_norm=None, reg_data_lambda=0.0,
                 reg_norm_lambda=100.0, reg_query_lambda=0.0, verbose=False, max_iter=200, pos_weight="balanced",
                 lr=1.0, matrix_options=MATRIX)
KNN_PROP2 = dict(matrix_options=MATRIX, normalize_scores=False, sigmoid_before_propagate=True, calib_a=10.0,
                 calib_b=-0.4, prior_weight=1.0)
# (loop, options, text, category the simulated user labels, start policy).  The fourth graph session searches "c0" while
# its user accepts "c2" only: under after_first_positive it stays on the text vector for its first rounds -- inside the
# query batch, outside the propagation batch -- and joins the other three once it starts
SESSIONS = [("knn_prop2", KNN_PROP2, "a c0", "c0", "from_start"),
            ("knn_prop2", KNN_PROP2, "a c1", "c1", "from_start"),
            ("knn_prop2", KNN_PROP2, "a c2", "c2", "from_start"),
            ("knn_prop2", KNN_PROP2, "a c0", "c2", "after_first_positive"),
            ("multi_reg", MULTI_REG, "a c1", "c1", "after_first_batch"),
            ("plain", None, "a c2", "c2", "after_first_batch")]
KNN = (0, 1, 2, 3)


@pytest.fixture(scope="module")
def grp():
    from seesaw_amd.synthetic import GlobalDataManager, make_dataset
    ds = make_dataset("grp", n_images=200, tiles_per_image=13, n_categories=3, positive_frac=0.08, seed=21, knn_k=10)
    return GlobalDataManager().add(ds), ds


def _make_sessions(gdm, agg_method):
    from seesaw_amd.basic_types import IndexSpec, SessionParams
    from seesaw_amd.seesaw_session import make_session
    out = []
    for loop, options, text, _, policy in SESSIONS:
        p = SessionParams(index_spec=IndexSpec(d_name="grp", i_name="multiscale", c_name=None), interactive=loop,
                          interactive_options=options, batch_size=3, shortlist_size=50, agg_method=agg_method,
                          aug_larger="greater", start_policy=policy, index_options={"use_vec_index": False})
        s = make_session(gdm, p)["session"]
        s.set_text(text)
        out.append(s)
    assert len({id(s.index) for s in out}) == 1  # one shared MultiscaleIndex
    return out


def _label(session, category, ds):
    """the simulated user of benchmark_loop: the ground-truth boxes of `category` on the batch just shown"""
    from seesaw_amd.basic_types import BenchParams
    from seesaw_amd.seesaw_bench import _group_boxes, fill_imdata
    b = BenchParams(name="grp", ground_truth_category=category, qstr=f"a {category}", n_batches=ROUNDS)
    boxes = ds.box_data.assign(description=ds.box_data.category)
    boxes = boxes[boxes.category == category]
    groups = _group_boxes(boxes)
    session.update_last_batch([fill_imdata(im, boxes, b, _groups=groups) for im in session.last_batch()])


def _records(acts):
    if acts is None:
        return None
    if hasattr(acts, "records"):
        return acts.records()
    return [None if a is None else a[["x1", "y1", "x2", "y2", "score"]].to_numpy(dtype=np.float64).tolist() for a in acts]


def _snapshot(s):
    vec = getattr(s.loop, "curr_vec", None)
    model = getattr(s.loop.state, "knn_model", None)
    return dict(dbidxs=np.asarray(s.acc_indices[-1]).copy(), activations=_records(s.acc_activations[-1]),
                returned=np.array(s.q.returned).copy(), started=s.loop.started,
                curr_vec=None if vec is None else np.asarray(vec, dtype=np.float32).copy().view(np.uint32),
                propagated=None if model is None else model.lp.fetch().view(np.uint64),
                log=[e[1:] for e in s._log_raw], n_timing=len(s.timing))


def _run(gdm, ds, agg_method, grouped, calls=()):
    from seesaw_amd.seesaw_session import SessionGroup
    sessions = _make_sessions(gdm, agg_method)
    group = SessionGroup(sessions)
    trace = []
    for _ in range(ROUNDS):
        if grouped:
            query_groups = group.query_groups()
            shown = group.next()
            assert all(np.array_equal(a, s.acc_indices[-1]) for a, s in zip(shown, sessions))
        else:
            for s in sessions:
                s.next()
        for s, spec in zip(sessions, SESSIONS):
            _label(s, spec[3], ds)
        if grouped:
            group.refine()
            # (`started` only ever turns on: these are the groups refine() used)
            calls.append((query_groups, group.fit_groups()[0], group.propagation_groups()))
        else:
            for s in sessions:
                s.refine()
        trace.append([_snapshot(s) for s in sessions])
    return trace


@pytest.mark.parametrize("agg_method", ["plain_score", "avg_score"])
def test_group_rounds_with_graph_loops_equal_independent_sessions(grp, agg_method, monkeypatch):
    from seesaw_amd.loops.graph_based import KnnProp2
    from seesaw_amd.seesaw_session import SessionGroup
    gdm, ds = grp
    calls, batches = [], []
    monkeypatch.setattr(SessionGroup, "MIN_PROPAGATION_GROUP", 2)  # (the product's minimum is a measured break-even, not a rule of correctness)
    alone = _run(gdm, ds, agg_method, grouped=False)
    own = KnnProp2.refine_batch.__func__
    monkeypatch.setattr(KnnProp2, "refine_batch", classmethod(lambda cls, loops: (batches.append(len(loops)), own(cls, loops))[1]))
    together = _run(gdm, ds, agg_method, grouped=True, calls=calls)
    for r, (ra, rt) in enumerate(zip(alone, together)):
        for i, (a, t) in enumerate(zip(ra, rt)):
            tag = (agg_method, r, i, SESSIONS[i][0])
            assert np.array_equal(a["dbidxs"], t["dbidxs"]), tag
            assert len(a["dbidxs"]) == 3, tag
            assert a["activations"] == t["activations"], tag
            assert np.array_equal(a["returned"], t["returned"]), tag
            assert a["started"] == t["started"], tag
            assert (a["curr_vec"] is None) == (t["curr_vec"] is None), tag
            if a["curr_vec"] is not None:
                assert np.array_equal(a["curr_vec"], t["curr_vec"]), tag
            assert (a["propagated"] is None) == (t["propagated"] is None) == (i not in KNN), tag
            if i in KNN:
                assert np.array_equal(a["propagated"], t["propagated"]), tag
            assert a["log"] == t["log"] and a["n_timing"] == t["n_timing"] == r + 1, tag
    late = [rt[3]["started"] for rt in together]  # the after_first_positive graph session, after each round's refine
    assert late[0] is False and late[-1] is True, late
    for (queries, fits, props), started, n_batched in zip(calls, late, batches):
        # the started graph sessions of the round refine in one batch; the late one joins once it starts
        assert props == ([(0, 1, 2, 3)] if started else [(0, 1, 2)]), (props, late)
        assert n_batched == (4 if started else 3), (batches, late)
        assert fits == [(4,)], fits  # as without the feature: the one multi_reg loop, a group of its own
    assert len(batches) == ROUNDS
    # query_groups() as without the feature: a started graph loop answers on its own; until the late one starts it asks
    # with its text vector, together with the multi_reg and the plain session
    started_before = [False] + late[:-1]
    for (queries, _, _), started in zip(calls, started_before):
        if started:
            assert queries == [(0,), (1,), (2,), (3,), (4, 5)], queries
        else:
            assert queries == [(0,), (1,), (2,), (3, 4, 5)], queries
    # the graph sessions propagated: their scores left the prior, each its own way
    last = together[-1]
    assert not np.array_equal(last[0]["propagated"], last[2]["propagated"])
    assert not np.array_equal(together[0][0]["propagated"], last[0]["propagated"])

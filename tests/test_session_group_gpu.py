"""GPU: SessionGroup (one query_batch and one batched fit for the sessions of a lock-step round) against the same
sessions run independently: per round and per session the same dbidxs, activations, `returned` set and `curr_vec`
bits."""
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
# (loop, options, text, category the simulated user labels, start policy).  The fourth session searches "c0" while its
# user accepts "c2" only: its batches are negative until an image of both turns up, so under after_first_positive it
# stays on the text vector -- out of the fit batch, inside the query batch -- for its first rounds
SESSIONS = [("multi_reg", MULTI_REG, "a c0", "c0", "after_first_batch"),
            ("multi_reg", MULTI_REG, "a c1", "c1", "after_first_batch"),
            ("multi_reg", MULTI_REG, "a c2", "c2", "after_first_batch"),
            ("multi_reg", MULTI_REG, "a c0", "c2", "after_first_positive"),
            ("plain", None, "a c1", "c1", "after_first_batch"),
            ("knn_prop2", KNN_PROP2, "a c2", "c2", "from_start")]


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
    """a batch's activations as plain numbers: [(x1, y1, x2, y2, score), ...] per image"""
    if acts is None:
        return None
    if hasattr(acts, "records"):
        return acts.records()
    return [None if a is None else a[["x1", "y1", "x2", "y2", "score"]].to_numpy(dtype=np.float64).tolist() for a in acts]


def _snapshot(s):
    vec = getattr(s.loop, "curr_vec", None)
    return dict(dbidxs=np.asarray(s.acc_indices[-1]).copy(), activations=_records(s.acc_activations[-1]),
                returned=np.array(s.q.returned).copy(), started=s.loop.started,
                curr_vec=None if vec is None else np.asarray(vec, dtype=np.float32).copy().view(np.uint32),
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
            calls.append((query_groups, group.fit_groups()[0]))  # `started` only ever turns on: the groups refine() used
        else:
            for s in sessions:
                s.refine()
        trace.append([_snapshot(s) for s in sessions])
    return trace


@pytest.mark.parametrize("agg_method", ["plain_score", "avg_score"])
def test_group_rounds_equal_independent_sessions(grp, agg_method):
    gdm, ds = grp
    calls = []
    alone = _run(gdm, ds, agg_method, grouped=False)
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
            assert a["log"] == t["log"] and a["n_timing"] == t["n_timing"] == r + 1, tag
    # the work was shared: the five point-based sessions asked in one query_batch every round (knn_prop2, started
    # from the first round, on its own), and the started multi_reg loops refined in one batch
    assert all(q == [(0, 1, 2, 3, 4), (5,)] for q, _ in calls), calls
    late = [rt[3]["started"] for rt in together]  # the after_first_positive session, after each round's refine
    assert late[0] is False and late[-1] is True, late  # it dropped out of a fit batch, and joined one
    for (_, fits), started in zip(calls, late):
        assert fits == [(0, 1, 2, 3)] if started else fits == [(0, 1, 2)], (fits, late)
    # feedback moved the three vectors away from their text vectors, differently
    vecs = [together[-1][i]["curr_vec"] for i in range(3)]
    assert not np.array_equal(vecs[0], vecs[1]) and not np.array_equal(vecs[1], vecs[2])
    assert not np.array_equal(together[0][0]["curr_vec"], together[-1][0]["curr_vec"])

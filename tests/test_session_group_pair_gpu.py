"""GPU: SessionGroup.next() with started `multi_reg_neg` loops in the group's query_batch (`vectors2`: the two-vector
query batched, one `ssw_index_stage2_pair_batch` launch a round) against the same sessions run one by one: per round and
per session every field tests/test_session_group_gpu.py snapshots, plus `confusion_vec`.  The dataset is the shape of
`grp2` in tests/test_fit2_device_gpu.py."""
import numpy as np
import pytest

from test_session_group_gpu import _snapshot

pytestmark = pytest.mark.gpu

ROUNDS = 4
NEG = dict(reg_norm_lambda=100.0, reg_query_lambda=10.0, reg_data_lambda=0.0, verbose=False, max_iter=100, lr=1.0,
           matrix_options=None, discount_neg=True)
MULTI_REG = dict(label_loss_type="ce_loss", rank_loss_margin=0.2, use_qvec_norm=None, reg_data_lambda=0.0,
                 reg_norm_lambda=100.0, reg_query_lambda=0.0, verbose=False, max_iter=200, pos_weight="balanced",
                 lr=1.0, matrix_options=None)
# (loop, options, text, the category the simulated user labels).  The loops that draw from torch's global generator stand
# in the order a group refines them: the opted-in batch first
GROUP = [("multi_reg_neg", dict(NEG, fit_on_device=True), "a c0", "c0"),
         ("multi_reg_neg", dict(NEG, fit_on_device=True, discount_neg=False), "a c1", "c1"),
         ("multi_reg_neg", dict(NEG), "a c2", "c2"),
         ("multi_reg_neg", dict(NEG, discount_neg=False), "a c0", "c2"),
         ("multi_reg", MULTI_REG, "a c2", "c2"),
         ("plain", None, "a c1", "c1")]
NAME = "grp2pair"


@pytest.fixture(scope="module")
def grp():
    from seesaw_amd.synthetic import GlobalDataManager, make_dataset
    ds = make_dataset(NAME, n_images=200, tiles_per_image=13, n_categories=3, positive_frac=0.08, seed=21, knn_k=0)
    return GlobalDataManager().add(ds), ds


def _label(session, category, ds):
    """the simulated user of benchmark_loop: the ground-truth boxes of `category` on the batch just shown"""
    from seesaw_amd.basic_types import BenchParams
    from seesaw_amd.seesaw_bench import _group_boxes, fill_imdata
    b = BenchParams(name=NAME, ground_truth_category=category, qstr=f"a {category}", n_batches=ROUNDS)
    boxes = ds.box_data.assign(description=ds.box_data.category)
    boxes = boxes[boxes.category == category]
    groups = _group_boxes(boxes)
    session.update_last_batch([fill_imdata(im, boxes, b, _groups=groups) for im in session.last_batch()])


def _make_sessions(gdm, agg_method):
    import torch
    from seesaw_amd.basic_types import IndexSpec, SessionParams
    from seesaw_amd.seesaw_session import make_session
    np.random.seed(5)
    torch.manual_seed(5)
    sessions = []
    for loop, options, text, _ in GROUP:
        p = SessionParams(index_spec=IndexSpec(d_name=NAME, i_name="multiscale", c_name=None), interactive=loop,
                          interactive_options=options, batch_size=3, shortlist_size=50, agg_method=agg_method,
                          aug_larger="greater", start_policy="after_first_batch", index_options={"use_vec_index": False})
        s = make_session(gdm, p)["session"]
        s.set_text(text)
        sessions.append(s)
    assert len({id(s.index) for s in sessions}) == 1  # one shared MultiscaleIndex
    return sessions


def _run(gdm, ds, agg_method, grouped, monkeypatch):
    from seesaw_amd import _lib
    from seesaw_amd.seesaw_session import SessionGroup
    sessions = _make_sessions(gdm, agg_method)
    group = SessionGroup(sessions)
    calls, call = [], _lib.call

    def counting(name, *args):
        calls.append(name)
        return call(name, *args)

    monkeypatch.setattr(_lib, "call", counting)
    trace, groups = [], []
    try:
        for _ in range(ROUNDS):
            if grouped:
                groups.append(group.query_groups())
                shown = group.next()
                assert all(np.array_equal(a, s.acc_indices[-1]) for a, s in zip(shown, sessions))
            else:
                for s in sessions:
                    s.next()
            for s, spec in zip(sessions, GROUP):
                _label(s, spec[3], ds)
            if grouped:
                group.refine()
            else:
                for s in sessions:
                    s.refine()
            u32 = lambda v: None if v is None else np.asarray(v, dtype=np.float32).copy().view(np.uint32)  # noqa: E731
            trace.append([dict(_snapshot(s), confusion_vec=u32(getattr(s.loop, "confusion_vec", None))) for s in sessions])
    finally:
        monkeypatch.setattr(_lib, "call", call)
    return trace, groups, calls


@pytest.mark.parametrize("agg_method", ["plain_score", "avg_score"])
def test_group_rounds_equal_sessions_one_by_one(grp, agg_method, monkeypatch):
    gdm, ds = grp
    alone, _, calls_alone = _run(gdm, ds, agg_method, False, monkeypatch)
    together, groups, calls = _run(gdm, ds, agg_method, True, monkeypatch)
    for r, (ra, rt) in enumerate(zip(alone, together)):
        for i, (a, t) in enumerate(zip(ra, rt)):
            tag = (agg_method, r, i, GROUP[i][0])
            assert np.array_equal(a["dbidxs"], t["dbidxs"]) and len(a["dbidxs"]) == 3, tag
            assert a["activations"] == t["activations"], tag
            assert np.array_equal(a["returned"], t["returned"]), tag
            assert a["started"] == t["started"], tag
            for k in ("curr_vec", "confusion_vec"):
                assert (a[k] is None) == (t[k] is None), (tag, k)
                if a[k] is not None:
                    assert np.array_equal(a[k], t[k]), (tag, k)
            assert a["log"] == t["log"] and a["n_timing"] == t["n_timing"] == r + 1, tag
    # every round all six asked in ONE query_batch: the started multi_reg_neg loops with the point-based ones
    assert all(g == [(0, 1, 2, 3, 4, 5)] for g in groups), groups
    assert all(t["started"] for t in together[0])
    assert all(together[-1][i]["confusion_vec"] is not None for i in range(4))
    # from the second round on the four two-vector queries are one launch a round, and no per-query second stage is left
    assert calls.count("ssw_index_stage2_pair_batch") == ROUNDS - 1 and "ssw_index_stage2_pair_batch" not in calls_alone
    assert "ssw_index_score_rows" in calls_alone
    assert not [c for c in calls if c in ("ssw_index_score_rows", "ssw_index_gather_scores", "ssw_index_rescore_avg")], calls
    assert not np.array_equal(together[0][0]["curr_vec"], together[-1][0]["curr_vec"])


def test_a_subclass_with_its_own_next_batch_stays_alone(grp):
    from seesaw_amd.loops.multi_reg_neg import MultiRegNeg
    from seesaw_amd.seesaw_session import SessionGroup

    class Own(MultiRegNeg):
        def next_batch(self):
            return MultiRegNeg.next_batch(self)

    gdm, ds = grp
    sessions = _make_sessions(gdm, "plain_score")
    for s in sessions:
        s.loop.started = True
    group = SessionGroup(sessions)
    assert group.query_groups() == [(0, 1, 2, 3, 4, 5)]
    dim = sessions[0].index.vectors.shape[1]
    assert SessionGroup.batch_vector2(sessions[0].loop) is None  # discount_neg, no confusion vector yet: one vector
    assert np.array_equal(SessionGroup.batch_vector2(sessions[1].loop), np.zeros(dim))
    assert SessionGroup.batch_vector2(sessions[4].loop) is None and SessionGroup.batch_vector2(sessions[5].loop) is None
    sessions[1].loop.__class__ = Own
    assert group.query_groups() == [(0, 2, 3, 4, 5), (1,)]
    assert SessionGroup.batch_vector(sessions[1].loop) is None and SessionGroup.batch_vector2(sessions[1].loop) is None
    shown = group.next()  # the group of five through query_batch, the subclass through its own next()
    assert all(len(a) == 3 for a in shown)

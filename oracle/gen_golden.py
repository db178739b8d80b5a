#!/usr/bin/env python3
"""Generate tests/golden/*.npz by running the REFERENCE itself (imported from
/root/reference through oracle/_ref_import.py) on seeded synthetic inputs.

Run in the build container only:   python oracle/gen_golden.py [family ...]
The fixtures are data (inputs or the seeds that regenerate them, plus the reference's
outputs); no reference source travels.  Large inputs are regenerated from seeds with the
bit-exact synthetic generator (oracle.seesaw_oracle.synth_rows), so the fixtures stay small.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import _ref_import as R  # noqa: E402
from oracle import seesaw_oracle as orc  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
OUT_DIR = GOLDEN  # --check redirects the writes to a scratch directory


def save(name, **arrays):
    os.makedirs(OUT_DIR, exist_ok=True)
    path = os.path.join(OUT_DIR, name + ".npz")
    np.savez_compressed(path, **arrays)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


def compare_npz(path_a, path_b, b_may_be_a_slice=False):
    """-> list of differences between two .npz files, array by array: keys, dtype, shape and raw bytes
    (the zip container itself carries timestamps, so files are compared by content).  b_may_be_a_slice: arrays that only the
    committed file (a) holds are not a difference (a family regenerated in part: SSW_C5_QUICK)."""
    a, b = np.load(path_a), np.load(path_b)
    diffs = [f"key only in {os.path.basename(p)}: {k}" for p, ks in ((path_a, set() if b_may_be_a_slice else set(a.files) - set(b.files)),
                                                                      (path_b, set(b.files) - set(a.files))) for k in sorted(ks)]
    for k in sorted(set(a.files) & set(b.files)):
        x, y = a[k], b[k]
        if x.dtype != y.dtype or x.shape != y.shape:
            diffs.append(f"{k}: {x.dtype}{x.shape} vs {y.dtype}{y.shape}")
        elif x.tobytes() != y.tobytes():
            if x.dtype.kind == "f":
                diffs.append(f"{k}: values differ, max |delta| = {np.nanmax(np.abs(x.astype(np.float64) - y.astype(np.float64))):.3e}")
            else:
                diffs.append(f"{k}: values differ")
    return diffs


def synth_vector_meta(n_images, tiles_per_image, dbidx_of_position, rng):
    """vector_meta as the reference's MultiscaleIndex holds it (multiscale_index.py:257-259):
    one row per tile: dbidx, zoom_level, x1, y1, x2, y2; rows sorted by dbidx."""
    import pandas as pd
    rows = []
    for pos in range(n_images):
        t = tiles_per_image[pos]
        for j in range(t):
            zoom = 0 if j < max(1, t - 1) else 1
            x1 = float(rng.integers(0, 400))
            y1 = float(rng.integers(0, 300))
            side = 224.0 * (1 + zoom)
            rows.append((int(dbidx_of_position[pos]), zoom, x1, y1, x1 + side, y1 + side))
    df = pd.DataFrame(rows, columns=["dbidx", "zoom_level", "x1", "y1", "x2", "y2"])
    df = df.assign(zoom_level=df.zoom_level.astype("int16"),
                   **{c: df[c].astype("float32") for c in ["x1", "y1", "x2", "y2"]})
    return df


def synth_pyramid_meta(n_images, dbidx_of_position, rng):
    """tiles of a 3-level pyramid in original-image pixels, like the reference's tiler output
    (multiscale_tools.py:96-117): level z has square tiles of side 224 * 2**z at half-tile stride, the last level
    is clipped to the image; image sizes vary, rows sorted by dbidx."""
    import pandas as pd
    rows = []
    sizes = [(640, 480), (500, 375), (1024, 768), (448, 448), (224, 224), (800, 300)]
    for pos in range(n_images):
        w, h = sizes[int(rng.integers(0, len(sizes)))]
        for zoom in range(3):
            side = 224.0 * (2 ** zoom)
            if zoom > 0 and side / 2 >= max(w, h):
                break
            stride = side / 2
            xs = np.arange(0, max(w - side, 0) + 1e-6, stride) if w > side else np.array([0.0])
            ys = np.arange(0, max(h - side, 0) + 1e-6, stride) if h > side else np.array([0.0])
            for y1 in ys:
                for x1 in xs:
                    rows.append((int(dbidx_of_position[pos]), zoom, x1, y1, min(x1 + side, w), min(y1 + side, h)))
    df = pd.DataFrame(rows, columns=["dbidx", "zoom_level", "x1", "y1", "x2", "y2"])
    return df.assign(zoom_level=df.zoom_level.astype("int16"),
                     **{c: df[c].astype("float32") for c in ["x1", "y1", "x2", "y2"]})


# ------------------------------------------------------------------------------------
def gen_scan_topk():
    """(i) _query_prelim(force_exact=True) and CoarseIndex.query on seeded vectors."""
    import pandas as pd
    msi = R.ref("seesaw.indices.multiscale.multiscale_index")
    coarse = R.ref("seesaw.indices.coarse.coarse_index")
    pr = sys.modules["pyroaring"]

    # known-answer pin the reference itself carries (multiscale_index.py:182-187)
    msi.test_distinct_topk_positions()

    cases = []
    for case_id, (n_images, tmax, k, n_excl, seed) in enumerate(
            [(1539, 13, 50, 40, 101), (400, 1, 100, 0, 102), (997, 30, 50, 300, 103), (64, 5, 200, 10, 104)]):
        rng = np.random.default_rng(seed)
        tiles = np.full(n_images, tmax) if tmax in (1, 13) else rng.integers(1, tmax + 1, n_images)
        dbidx_of_position = np.arange(n_images) * 3 + 5  # non-trivial dbidx values
        meta = synth_vector_meta(n_images, tiles, dbidx_of_position, rng)
        n = meta.shape[0]
        X = orc.synth_rows(seed, 0, n, 512)
        q = orc.synth_query(seed)
        excl_pos = rng.choice(n_images, size=n_excl, replace=False) if n_excl else np.zeros(0, np.int64)
        exclude = pr.BitMap(dbidx_of_position[excl_pos])
        index = msi.MultiscaleIndex(embedding=None, vectors=X, vector_meta=meta, vec_index=None)
        df = index._query_prelim(vector=q, topk_dbidx=k, exclude_dbidx=exclude, force_exact=True)
        scores_full = index.score(q)
        cases.append(dict(seed=seed, n_images=n_images, tiles=tiles, k=k, excl_pos=excl_pos,
                          dbidx=df["dbidx"].values.astype(np.int64),
                          max_score=df["max_score"].values.astype(np.float32),
                          scores_head=scores_full[:256].astype(np.float32)))
    out = {}
    for i, c in enumerate(cases):
        for key, v in c.items():
            out[f"c{i}_{key}"] = np.asarray(v)
    out["n_cases"] = np.asarray(len(cases))

    # CoarseIndex.query (coarse_index.py:57-96)
    n = 3000
    Xc = orc.synth_rows(201, 0, n, 512)
    qc = orc.synth_query(201)
    dbidx = np.arange(n) * 2 + 1
    cmeta = pd.DataFrame({"dbidx": dbidx})
    cidx = coarse.CoarseIndex(embedding=None, vectors=Xc, vector_meta=cmeta)
    excl = pr.BitMap(dbidx[np.random.default_rng(5).choice(n, 200, replace=False)])
    res = cidx.query(topk=100, vector=qc, exclude=excl)
    out["coarse_seed"] = np.asarray(201)
    out["coarse_n"] = np.asarray(n)
    out["coarse_excl"] = np.array(sorted(excl), dtype=np.int64)
    out["coarse_dbidxs"] = np.asarray(res["dbidxs"], dtype=np.int64)
    out["coarse_nextstartk"] = np.asarray(res["nextstartk"])
    out["coarse_scores"] = np.array([a.score.values[0] for a in res["activations"]], dtype=np.float32)
    save("scan_topk", **out)


# ------------------------------------------------------------------------------------
def gen_multiscale_query():
    """(ii) MultiscaleIndex.query(agg_method='plain_score') -- multiscale_index.py:314-403."""
    msi = R.ref("seesaw.indices.multiscale.multiscale_index")
    pr = sys.modules["pyroaring"]
    seed, n_images = 301, 800
    rng = np.random.default_rng(seed)
    tiles = rng.integers(1, 20, n_images)
    dbidx_of_position = np.arange(n_images) * 7 + 2
    meta = synth_vector_meta(n_images, tiles, dbidx_of_position, rng)
    X = orc.synth_rows(seed, 0, meta.shape[0], 512)
    q = orc.synth_query(seed)
    index = msi.MultiscaleIndex(embedding=None, vectors=X, vector_meta=meta, vec_index=None)
    out = dict(seed=np.asarray(seed), n_images=np.asarray(n_images), tiles=tiles,
               meta=meta[["dbidx", "zoom_level", "x1", "y1", "x2", "y2"]].values.astype(np.float64))
    returned = pr.BitMap()
    for rnd in range(4):
        res = index.query(vector=q, topk=5, shortlist_size=50, exclude=returned, force_exact=True,
                          agg_method="plain_score", aug_larger="all",
                          rescore_method=lambda vecs: vecs @ q.reshape(-1, 1))
        out[f"r{rnd}_dbidxs"] = np.asarray(res["dbidxs"], dtype=np.int64)
        acts = np.stack([a[["x1", "y1", "x2", "y2", "dbidx", "score"]].values[0].astype(np.float64)
                         for a in res["activations"]])
        out[f"r{rnd}_activations"] = acts
        returned.update(res["dbidxs"])
    # vector2 form (multiscale_index.py:347-349)
    q2 = orc.synth_query(seed + 1)
    res = index.query(vector=q, vector2=q2, topk=5, shortlist_size=50, exclude=pr.BitMap(), force_exact=True,
                      agg_method="plain_score", aug_larger="all", rescore_method=None)
    out["v2_dbidxs"] = np.asarray(res["dbidxs"], dtype=np.int64)
    out["v2_scores"] = np.array([a.score.values[0] for a in res["activations"]], dtype=np.float64)

    # agg_method='avg_score' (score_frame2 / box_join, multiscale_index.py:112-150, box_utils.py:336-372): the
    # aggregation scripts/configs/std_bench.yaml uses.  A second index with a real 3-level tile pyramid (tiles of
    # neighbouring zoom levels overlap), all three aug_larger modes, plus the vector2 form.  The candidate tiles'
    # scores as the reference formed them are captured too, so the CPU oracle can be pinned on identical inputs.
    pseed, pn = 311, 300
    prng = np.random.default_rng(pseed)
    pmeta = synth_pyramid_meta(pn, np.arange(pn) * 3 + 1, prng)
    PX = orc.synth_rows(pseed, 0, pmeta.shape[0], 512)
    pq = orc.synth_query(pseed)
    pindex = msi.MultiscaleIndex(embedding=None, vectors=PX, vector_meta=pmeta, vec_index=None)
    out["pyr_seed"], out["pyr_n_images"] = np.asarray(pseed), np.asarray(pn)
    out["pyr_meta"] = pmeta[["dbidx", "zoom_level", "x1", "y1", "x2", "y2"]].values.astype(np.float64)
    orig_rescore = msi.rescore_candidates
    for aug in ["all", "greater", "adjacent"]:
        seen = {}

        def recording(fullmeta, topk, _o=orig_rescore, **kw):
            seen["rows"] = fullmeta.index.values.astype(np.int64).copy()
            seen["scores"] = fullmeta.score.values.astype(np.float32).copy()
            return _o(fullmeta, topk, **kw)

        msi.rescore_candidates = recording
        try:
            res = pindex.query(vector=pq, topk=10, shortlist_size=50, exclude=pr.BitMap(pmeta.dbidx.values[:40]),
                               force_exact=True, agg_method="avg_score", aug_larger=aug, rescore_method=None)
        finally:
            msi.rescore_candidates = orig_rescore
        out[f"avg_{aug}_dbidxs"] = np.asarray(res["dbidxs"], dtype=np.int64)
        out[f"avg_{aug}_activations"] = np.stack([a[["x1", "y1", "x2", "y2", "dbidx", "score"]].values[0].astype(np.float64)
                                                  for a in res["activations"]])
        out[f"avg_{aug}_cand_rows"], out[f"avg_{aug}_cand_scores"] = seen["rows"], seen["scores"]
    pq2 = orc.synth_query(pseed + 1)
    res = pindex.query(vector=pq, vector2=pq2, topk=10, shortlist_size=50, exclude=pr.BitMap(), force_exact=True,
                       agg_method="avg_score", aug_larger="greater", rescore_method=None)
    out["avg_v2_dbidxs"] = np.asarray(res["dbidxs"], dtype=np.int64)
    out["avg_v2_activations"] = np.stack([a[["x1", "y1", "x2", "y2", "dbidx", "score"]].values[0].astype(np.float64)
                                          for a in res["activations"]])
    save("multiscale_query", **out)


# ------------------------------------------------------------------------------------
def gen_labelprop():
    """(iii) compute_exact_knn -> get_weight_matrix -> LabelPropagation.fit_transform
    (knn_graph.py:31-104,170-191; label_propagation.py:6-79; knn_methods.py:97-199)."""
    kg = R.ref("seesaw.knn_graph")
    lp = R.ref("seesaw.label_propagation")
    km = R.ref("seesaw.research.knn_methods")
    seed, n, k = 401, 1500, 10
    X = orc.synth_rows(seed, 0, n, 512)
    # clustered data so the graph is not trivial: mix rows with 20 centres
    rng = np.random.default_rng(seed)
    centres = orc.synth_rows(seed + 1, 0, 20, 512)
    assign = rng.integers(0, 20, n)
    X = X + 1.5 * centres[assign]
    X = (X / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float32)
    df = kg.compute_exact_knn(X, n_neighbors=k)
    graph = kg.KNNGraph(df).restrict_k(k=k)
    out = dict(seed=np.asarray(seed), n=np.asarray(n), k=np.asarray(k), X=X.astype(np.float32),
               src=df.src_vertex.values, dst=df.dst_vertex.values, dist=df.distance.values,
               rank=df.dst_rank.values, restricted_rows=np.asarray(graph.knn_df.shape[0]))
    for name, edist, symmetric in [("e05", 0.05, True), ("e10", 0.1, True), ("asym", 0.05, False)]:
        W = kg.get_weight_matrix(graph.knn_df, kfun=kg.rbf_kernel(edist), self_edges=False,
                                 normalized=False, symmetric=symmetric)
        out[f"{name}_indptr"] = W.indptr.astype(np.int64)
        out[f"{name}_indices"] = W.indices.astype(np.int64)
        out[f"{name}_data"] = W.data.astype(np.float64)
    # Laplacian and xlx (graph_based.py:45-49)
    L = kg.get_weight_matrix(graph.knn_df, kfun=kg.rbf_kernel(0.05), self_edges=False, normalized=False,
                             symmetric=True, laplacian=True)
    Ln = L / L.diagonal().sum()
    xlx = X.T @ (Ln @ X)
    out["lap_indptr"], out["lap_indices"], out["lap_data"] = L.indptr.astype(np.int64), L.indices.astype(np.int64), L.data
    out["xlx"] = np.asarray(xlx, dtype=np.float64)

    W = kg.get_weight_matrix(graph.knn_df, kfun=kg.rbf_kernel(0.05), self_edges=False, normalized=False,
                             symmetric=True)
    q = centres[3]
    base_scores = X @ q
    n_runs = 0
    for lam in [0.0, 1.0, 3.0]:
        for n_lab in [0, 6, 40]:
            counter = {"n": 0}
            model = lp.LabelPropagation(W, reg_lambda=lam, max_iter=300)
            orig_step = model._step

            def counting_step(*a, _o=orig_step, **kw):
                counter["n"] += 1
                return _o(*a, **kw)

            model._step = counting_step
            prior = km.sigmoid(10.0 * (base_scores + (-0.2))).astype(np.float64)
            lab_ids = rng.choice(n, n_lab, replace=False) if n_lab else np.zeros(0, np.int64)
            lab_vals = (assign[lab_ids] == 3).astype(np.float64)
            reg = prior if lam > 0 else None
            start = prior.copy()
            res = model.fit_transform(label_ids=lab_ids, label_values=lab_vals, reg_values=reg,
                                      start_value=start)
            out[f"run{n_runs}_lam"] = np.asarray(lam)
            out[f"run{n_runs}_ids"] = lab_ids.astype(np.int64)
            out[f"run{n_runs}_vals"] = lab_vals
            out[f"run{n_runs}_start"] = start
            out[f"run{n_runs}_out"] = np.asarray(res, dtype=np.float64)
            out[f"run{n_runs}_steps"] = np.asarray(counter["n"])
            n_runs += 1
    out["n_runs"] = np.asarray(n_runs)

    # LabelPropagationRanker2 driver: set_base_scores / update / top_k (knn_methods.py:97-199)
    ranker = km.LabelPropagationRanker2(weight_matrix=W, normalize_scores=False, sigmoid_before_propagate=True,
                                        calib_a=10.0, calib_b=-0.2, prior_weight=1.0)
    ranker.set_base_scores(base_scores)
    ids0, sc0 = ranker.top_k(k=20)
    out["rk_base_scores"] = base_scores.astype(np.float32)
    out["rk_top0_ids"], out["rk_top0_scores"] = ids0, sc0
    upd_ids = np.concatenate([ids0[:5], rng.choice(n, 5, replace=False)])
    upd_labels = (assign[upd_ids] == 3).astype(np.float64)
    upd_labels[-1] = 0.0  # make sure there is a negative so propagation runs
    ranker.update(upd_ids, upd_labels)
    ids1, sc1 = ranker.top_k(k=20)
    out["rk_upd_ids"], out["rk_upd_labels"] = upd_ids.astype(np.int64), upd_labels
    out["rk_top1_ids"], out["rk_top1_scores"] = ids1, sc1
    out["rk_scores1"] = np.asarray(ranker.current_scores(), dtype=np.float64)
    out["assign"] = assign
    save("labelprop", **out)


# ------------------------------------------------------------------------------------
def gen_rank_loss():
    """(v) the reference's known-answer table (seesaw/test_rank_loss.py:9-234) re-evaluated by
    the reference's own functions, plus seeded random cases (rank_loss.py:3-187)."""
    import torch
    rl = R.ref("seesaw.rank_loss")
    trl = R.ref("seesaw.test_rank_loss")
    tests = trl.TEST_CASES if hasattr(trl, "TEST_CASES") else None
    cases = []
    if tests is None:
        # locate the table whatever it is called
        for name in dir(trl):
            v = getattr(trl, name)
            if isinstance(v, (list, tuple)) and len(v) > 5 and isinstance(v[0], dict):
                tests = v
                break
    assert tests is not None, "rank-loss known-answer table not found"
    out = {}
    for i, case in enumerate(tests):
        target = torch.as_tensor(case["target"]).float()
        scores = torch.as_tensor(case["scores"]).float()
        margin = float(case.get("margin", 0.0))
        out[f"t{i}_target"], out[f"t{i}_scores"], out[f"t{i}_margin"] = target.numpy(), scores.numpy(), np.asarray(margin)
        out[f"t{i}_inversions"] = rl.ref_signed_inversions(target, scores=scores, margin=margin).numpy()
        out[f"t{i}_loss"] = rl.ref_pairwise_rank_loss(target, scores=scores, margin=margin).numpy()
        out[f"t{i}_grad"] = rl.ref_pairwise_rank_loss_gradient(target, scores=scores, margin=margin).numpy()
        for key in case:
            if key not in ("target", "scores", "margin"):
                try:
                    out[f"t{i}_expected_{key}"] = np.asarray(torch.as_tensor(case[key]).numpy(), dtype=np.float64)
                except Exception:
                    pass
    out["n_table"] = np.asarray(len(tests))
    rng = np.random.default_rng(7)
    for i in range(6):
        n = int(rng.integers(2, 60))
        target = torch.from_numpy(rng.integers(0, 3 if i % 2 else 2, n).astype(np.float32))
        scores = torch.from_numpy(np.round(rng.standard_normal(n), 1 if i < 3 else 5).astype(np.float32))
        margin = float([0.0, 0.2, 1.0][i % 3])
        out[f"r{i}_target"], out[f"r{i}_scores"], out[f"r{i}_margin"] = target.numpy(), scores.numpy(), np.asarray(margin)
        ls, mx = rl.ref_pairwise_rank_loss(target, scores=scores, margin=margin, aggregate="sum",
                                           return_max_inversions=True)
        out[f"r{i}_hinge_sum"], out[f"r{i}_max_inv"] = ls.numpy(), mx.numpy()
        ll, _ = rl.ref_pairwise_logistic_loss(target, scores=scores, aggregate="sum", return_max_inversions=True)
        out[f"r{i}_logistic_sum"] = ll.numpy()
        out[f"r{i}_hinge_grad"] = rl.ref_pairwise_rank_loss_gradient(target, scores=scores, margin=margin).numpy()
        g, maxrev, total = rl.quick_pairwise_gradient_zero_margin(target, scores=scores, return_max_inversions=True)
        out[f"r{i}_quick_grad"], out[f"r{i}_quick_maxrev"], out[f"r{i}_quick_total"] = g.numpy(), maxrev.numpy(), np.asarray(total)
        out[f"r{i}_cheap_loss"] = rl.cheap_pairwise_rank_loss(target, scores=scores).numpy()
    out["n_random"] = np.asarray(6)

    # ---- the rest of the rank-loss code: compute_inversions, RankAndLoss (pairwise_rank_loss.py:24-135) and
    # RankRegressionPT.fit over RankingRegModule / cheap_pairwise_rank_loss (logistic_regression.py:16-65,126-267)
    prl = R.ref("seesaw.pairwise_rank_loss")
    lr = R.ref("seesaw.logistic_regression")
    for i in range(4):
        n = [7, 40, 200, 1000][i]
        labs = rng.integers(0, 2, n).astype(np.float64)
        scores = rng.standard_normal(n).astype(np.float32)
        out[f"inv{i}_labs"], out[f"inv{i}_scores"] = labs, scores
        out[f"inv{i}_inversions"] = np.asarray(prl.compute_inversions(labs, scores), dtype=np.int64)
    k = 0
    for (n, n_pos, margin) in [(30, 5, 0.0), (200, 40, 0.05), (200, 3, 0.2), (64, 63, 0.1), (50, 0, 0.1)]:
        X, y, q = _labelled_set(900 + k, n, max(n_pos, 1), q_noise=3.0)  # a poor w: inversions exist
        if n_pos == 0:
            y[:] = 0.0
        w = torch.from_numpy(q).clone().requires_grad_(True)
        loss = prl.RankAndLoss.apply(w, torch.from_numpy(X), torch.from_numpy(y).float(), torch.tensor(margin))
        if loss.requires_grad:
            loss.backward()
            grad = w.grad.numpy().copy()
        else:
            grad = np.zeros(512, np.float32)
        out[f"ral{k}_set"] = np.asarray([900 + k, n, max(n_pos, 1)])  # oracle.labelled_set(seed, n, n_pos, q_noise=3.0)
        out[f"ral{k}_y"] = y
        out[f"ral{k}_margin"], out[f"ral{k}_loss"], out[f"ral{k}_grad"] = np.asarray(margin), np.asarray(loss.item()), grad
        k += 1
    out["n_ral"] = np.asarray(k)
    # VecState (the old_seesaw loop's online update: one SGD step per call, dummy forward)
    X, y, q = _labelled_set(950, 120, 15)
    vs = prl.VecState(q.copy(), margin=0.1, opt_class=torch.optim.SGD, opt_params={"lr": 0.01}, renormalize=True)
    import contextlib
    import io
    for step in range(3):
        with contextlib.redirect_stdout(io.StringIO()):
            vs.update(X, y)
        out[f"vs_w{step}"] = vs.get_vec().copy()
    out["vs_set"] = np.asarray([950, 120, 15])
    # RankRegressionPT
    kk = 0
    for (n, n_pos, lam) in [(80, 12, 1.0), (300, 40, 10.0)]:
        X, y, q = _labelled_set(970 + kk, n, n_pos, q_noise=2.0)
        captured = {}
        orig_init = lr.RankingRegModule.__init__

        def patched(self, *a, _o=orig_init, **kw):
            _o(self, *a, **kw)
            captured["w0"] = self.linear.weight.detach().clone().numpy()
            captured["traj"] = _Trajectory(self, self.linear.weight)
            torch.manual_seed(0)

        lr.RankingRegModule.__init__ = patched
        try:
            torch.manual_seed(2000 + kk)
            model = lr.RankRegressionPT(scale="centered", reg_lambda=lam, regularizer_vector=q, max_iter=60, lr=1.0)
            model.fit(X, y.reshape(-1, 1).astype(np.float32))
        finally:
            lr.RankingRegModule.__init__ = orig_init
        tw, tl, tg = captured["traj"].arrays()
        out[f"rr{kk}_set"], out[f"rr{kk}_lam"] = np.asarray([970 + kk, n, n_pos]), np.asarray(lam)  # q_noise=2.0
        out[f"rr{kk}_w0"], out[f"rr{kk}_coeff"] = captured["w0"], model.get_coeff()
        out[f"rr{kk}_traj_w"], out[f"rr{kk}_traj_loss"], out[f"rr{kk}_traj_grad"] = tw, tl, tg
        kk += 1
    out["n_rr"] = np.asarray(kk)
    save("rank_loss", **out)


# ------------------------------------------------------------------------------------
_labelled_set = orc.labelled_set


class _Trajectory:
    """Records every (w, loss, grad) the reference's L-BFGS closure evaluates (basic_trainer.py:24-57):
    `training_step` is wrapped to note the parameter and the loss it returns, a tensor hook on the
    parameter notes the gradient of the one backward() that follows."""

    def __init__(self, module, param):
        self.w, self.loss, self.grad = [], [], []
        orig = module.training_step

        def step(batch, batch_idx, _o=orig):
            ret = _o(batch, batch_idx)
            self.w.append(param.detach().clone().numpy().reshape(-1))
            self.loss.append(float(ret["loss"].detach().item()))
            return ret

        module.training_step = step
        param.register_hook(lambda g: self.grad.append(g.detach().clone().numpy().reshape(-1)))

    def arrays(self):
        assert len(self.w) == len(self.loss) == len(self.grad), (len(self.w), len(self.loss), len(self.grad))
        return (np.stack(self.w).astype(np.float32), np.asarray(self.loss, dtype=np.float64),
                np.stack(self.grad).astype(np.float32))


FIT_SEEDS = (0, 1, 2)  # torch seeds: the reference's DataLoader shuffles the rows, so a fit depends on the seed


def gen_logreg():
    """(iv-a) LogisticRegressionPT.fit -> get_coeff (logistic_regression.py:270-421), seeded before every
    fit; the whole closure trajectory of the first seed and the coefficients of all FIT_SEEDS are kept."""
    import torch
    lr = R.ref("seesaw.logistic_regression")
    out = {}
    i = 0
    for (n, n_pos, lam, cw, with_weights) in [(40, 6, 1.0, "balanced", False), (300, 30, 3.3, "balanced", False),
                                              (120, 10, 10.0, 1.0, True), (13, 1, 1.0, "balanced", False)]:
        X, y, q = _labelled_set(500 + i, n, n_pos)
        sw = None
        if with_weights:
            sw = np.ones((n, 1))
            sw[: n // 3] = 4.0
        orig_init = lr.LogisticRegModule.__init__
        coeffs = []
        for seed in FIT_SEEDS:
            captured = {}

            # fit() draws twice from torch's generator: nn.Linear's initial weights (inside the module's
            # __init__) and then the DataLoader shuffle.  w0 is the same for every seed of a case (it is
            # handed to the HIP path as the start point); `seed` governs the shuffle only.
            def patched(self, *a, _o=orig_init, _seed=seed, **kw):
                _o(self, *a, **kw)
                captured["w0"] = self.linear.weight.detach().clone().numpy()
                captured["traj"] = _Trajectory(self, self.linear.weight)
                torch.manual_seed(_seed)

            lr.LogisticRegModule.__init__ = patched
            try:
                torch.manual_seed(1000 + i)
                model = lr.LogisticRegressionPT(class_weights=cw, scale="centered", reg_lambda=lam,
                                                regularizer_vector=q, fit_intercept=False, max_iter=200, lr=1.0)
                model.fit(X, y.reshape(-1, 1), sw)
            finally:
                lr.LogisticRegModule.__init__ = orig_init
            coeffs.append(model.get_coeff().reshape(-1).copy())
            if seed == FIT_SEEDS[0]:
                first, first_captured = model, captured
        tw, tl, tg = first_captured["traj"].arrays()
        out[f"c{i}_X"], out[f"c{i}_y"], out[f"c{i}_q"] = X, y, q
        out[f"c{i}_lam"] = np.asarray(lam)
        out[f"c{i}_cw"] = np.asarray(-1.0 if cw == "balanced" else cw)
        out[f"c{i}_sw"] = np.zeros(0) if sw is None else sw.reshape(-1)
        out[f"c{i}_w0"] = first_captured["w0"]
        out[f"c{i}_coeff"] = first.get_coeff()
        out[f"c{i}_coeff_seeds"] = np.stack(coeffs)
        out[f"c{i}_traj_w"], out[f"c{i}_traj_loss"], out[f"c{i}_traj_grad"] = tw, tl, tg
        out[f"c{i}_losses"] = np.array([l["loss"] for l in first.losses_], dtype=np.float64)
        out[f"c{i}_proba"] = first.predict_proba(X).reshape(-1)
        i += 1
    out["n_cases"] = np.asarray(i)
    out["fit_seeds"] = np.asarray(FIT_SEEDS)
    save("logreg", **out)


def gen_multireg():
    """(iv-b) RegModule.fit -> get_coeff for the three label losses (loops/multi_reg.py:24-200); torch is
    seeded immediately before every fit (the DataLoader shuffle is the only random draw), the closure
    trajectory of the first seed and the coefficients of all FIT_SEEDS are kept."""
    import pandas as pd
    import torch
    mr = R.ref("seesaw.loops.multi_reg")
    g = np.load(os.path.join(GOLDEN, "labelprop.npz"))
    xlx = torch.from_numpy(g["xlx"]).float()
    out = {"xlx": g["xlx"].astype(np.float32)}
    i = 0
    configs = [(lt, n, n_pos, dl, ql, 0.8) for lt in ["ce_loss", "pairwise_rank_loss", "pairwise_logistic_loss"]
               for (n, n_pos, dl, ql) in [(60, 8, 0.0, 0.0), (150, 20, 1000.0, 10.0)]]
    # a poor text query (mostly noise): inversions exist at w0, so the pairwise losses have work to do
    configs += [(lt, 100, 12, 0.0, 1.0, 3.0) for lt in ["pairwise_rank_loss", "pairwise_logistic_loss", "ce_loss"]]
    for (loss_type, n, n_pos, data_lam, query_lam, q_noise) in configs:
        if True:
            X, y, q = _labelled_set(700 + i, n, n_pos, q_noise=q_noise)
            # tiles grouped into images of 1..5 vectors
            rng = np.random.default_rng(i)
            img = np.sort(rng.integers(0, max(2, n // 3), n))
            matchdf = pd.DataFrame({"dbidx": img, "ys": y, "max_iou": y * 0.5})

            def make():
                return mr.RegModule(dim=512, xlx_matrix=xlx, qvec=torch.from_numpy(q).float(),
                                    label_loss_type=loss_type, rank_loss_margin=0.2,
                                    reg_data_lambda=data_lam, reg_norm_lambda=100.0, use_qvec_norm=None,
                                    reg_query_lambda=query_lam, verbose=False, max_iter=200,
                                    pos_weight="balanced", lr=1.0)

            coeffs = []
            for seed in FIT_SEEDS:
                model = make()
                traj = _Trajectory(model, model.weight)
                torch.manual_seed(seed)
                losses = model.fit(X, y, matchdf)
                coeffs.append(model.get_coeff().copy())
                if seed == FIT_SEEDS[0]:
                    first, first_traj, first_losses = model, traj, losses
            tw, tl, tg = first_traj.arrays()
            out[f"c{i}_X"], out[f"c{i}_y"], out[f"c{i}_q"], out[f"c{i}_img"] = X, y, q, img
            out[f"c{i}_loss_type"] = np.asarray(loss_type)
            out[f"c{i}_data_lam"], out[f"c{i}_query_lam"] = np.asarray(data_lam), np.asarray(query_lam)
            out[f"c{i}_coeff"] = first.get_coeff()
            out[f"c{i}_coeff_seeds"] = np.stack(coeffs)
            out[f"c{i}_raw_weight"] = first.weight.detach().numpy()
            out[f"c{i}_traj_w"], out[f"c{i}_traj_loss"], out[f"c{i}_traj_grad"] = tw, tl, tg
            out[f"c{i}_losses"] = np.array([l["loss"] for l in first_losses], dtype=np.float64)
            # one loss/gradient evaluation at w0 = normalised q with the rows in storage order
            m0 = make()
            vw = 1.0 / pd.Series(img).map(pd.Series(img).value_counts()).values
            Xc = X - X.mean(axis=0).reshape(1, -1)
            ret = m0._step((torch.from_numpy(Xc), torch.from_numpy(y), torch.from_numpy(vw)))
            ret["loss"].backward()
            out[f"c{i}_loss0"] = np.asarray(ret["loss"].item())
            out[f"c{i}_grad0"] = m0.weight.grad.numpy().copy()
            out[f"c{i}_parts0"] = np.array([ret[k].item() for k in ["loss_norm", "loss_datareg", "loss_queryreg", "loss_labels"]])
            i += 1
    out["n_cases"] = np.asarray(i)
    out["fit_seeds"] = np.asarray(FIT_SEEDS)
    save("multireg", **out)


BENCH_LOOP_DATASETS = {
    # A: weak signal, mediocre text query -- hits and misses alternate, the point-based updates matter
    "A": dict(make=dict(n_images=400, tiles_per_image=13, n_categories=3, positive_frac=0.04, seed=21, signal=0.17),
              noise=1.0),
    # B: the positives of a category form a tight cluster in the k-NN graph (cosine ~0.6 between them) but the
    # text query is nearly orthogonal to it: propagating the first labels over the graph is what finds the rest
    "B": dict(make=dict(n_images=400, tiles_per_image=13, n_categories=3, positive_frac=0.04, seed=22, signal=0.55),
              noise=6.0),
    # C: one vector per image behind the reference's CoarseIndex -- the only index its LogReg2 loop supports
    # (loops/log_reg.py:21 unpacks CoarseQuery.getXy's pair)
    "C": dict(make=dict(n_images=3000, tiles_per_image=1, n_categories=3, positive_frac=0.02, seed=23, signal=0.2),
              noise=3.5),
    # D: one vector per image WITH a k-NN graph: what the active-search loops plan over (loops/active_search.py takes
    # vector_meta.dbidx.iloc[vector id], i.e. a coarse index); clustered positives as in B
    "D": dict(make=dict(n_images=600, tiles_per_image=1, n_categories=3, positive_frac=0.04, seed=24, signal=0.5),
              noise=3.0, graph=True),
}
BENCH_LOOP_SEEDS = (0, 1, 2, 3, 4)  # torch seeds per fitting variant: how far does the reference reproduce itself?
BENCH_LOOP_KNN_POOL = 11  # neighbours in the stored graph; the loops keep dst_rank < knn_k = 10 of them


def gen_bench_loop():
    """(vii) the reference's own Session + benchmark_loop (seesaw_session.py, seesaw_bench.py:278-355)
    over its own MultiscaleIndex and loops, on synthetic LVIS-shape datasets (seesaw_amd.synthetic supplies
    data only: vectors, tile boxes, ground truth).  The k-NN graph is the reference's compute_exact_knn
    (knn_graph.py:170-191) and the weight matrices its get_weight_matrix; Ray-backed caches are bypassed by
    handing the loops the matrices directly.  Captured: the dbidx returned in every round, nfound / nseen.
    Runs on the CPU only."""
    import contextlib
    import io
    import json
    import torch
    from seesaw_amd.synthetic import make_dataset
    msi = R.ref("seesaw.indices.multiscale.multiscale_index")
    coarse = R.ref("seesaw.indices.coarse.coarse_index")
    sess = R.ref("seesaw.seesaw_session")
    bench = R.ref("seesaw.seesaw_bench")
    bt = R.ref("seesaw.basic_types")
    kg = R.ref("seesaw.knn_graph")
    mreg = R.ref("seesaw.loops.multi_reg")
    gb = R.ref("seesaw.loops.graph_based")
    pr = sys.modules["pyroaring"]

    class FakeDataset:
        def __init__(self, d):
            self.d = d
            self.file_meta = d.file_meta
            self.paths = d.paths

        def load_ground_truth(self):
            return self.d.load_ground_truth()

        def get_urls(self, idxbatch):
            return self.d.get_urls(idxbatch)

    matrix = dict(knn_path="nndescent60", symmetric=True, self_edges=False, normalized_weights=False, knn_k=10, edist=0.05)
    lp_opts = dict(matrix_options=matrix, normalize_scores=False, sigmoid_before_propagate=True, calib_a=10.0,
                   calib_b=-0.4, prior_weight=1.0)
    logreg_opts = dict(class_weights=1.0, scale="centered", reg_lambda=1.0, max_iter=200.0, lr=1, fit_intercept=False)
    # name -> (dataset, interactive, options)
    variants = {
        "plain": ("A", "plain", None),
        "rocchio_update": ("A", "rocchio_update", dict(rocchio_alpha=1.0, rocchio_beta=0.5, rocchio_gamma=0.25, verbose=False)),
        "multi_reg": ("A", "multi_reg", dict(label_loss_type="ce_loss", rank_loss_margin=0.2, use_qvec_norm=None,
                                             reg_data_lambda=0.0, reg_norm_lambda=100.0, reg_query_lambda=0.0,
                                             verbose=False, max_iter=200, pos_weight="balanced", lr=1.0,
                                             matrix_options=matrix)),
        "multi_reg_data": ("A", "multi_reg", dict(label_loss_type="pairwise_rank_loss", rank_loss_margin=0.2,
                                                  use_qvec_norm=None, reg_data_lambda=1000.0, reg_norm_lambda=100.0,
                                                  reg_query_lambda=10.0, verbose=False, max_iter=100,
                                                  pos_weight="balanced", lr=1.0, matrix_options=matrix)),
        "plain_c": ("C", "plain", None),
        "log_reg2_c": ("C", "log_reg2", logreg_opts),
        "knn_prop2": ("A", "knn_prop2", lp_opts),
        "plain_b": ("B", "plain", None),
        "knn_prop2_b": ("B", "knn_prop2", lp_opts),
        "pseudo_lr_b": ("B", "pseudo_lr", dict(switch_over=True, real_sample_weight=1.0, sample_size=2000,
                                               log_reg_params=logreg_opts, label_prop_params=lp_opts)),
        # the aggregation of the reference's standard bench config (scripts/configs/std_bench.yaml:23-24) inside
        # whole sessions (batch size 1: the reference's reversal check takes `batch in accepted`, which only a
        # one-element batch survives, seesaw_session.py:118-130) and the graph loop's own rescoring branch
        "plain_avg": ("A", "plain", None),
        "knn_prop2_b_avg": ("B", "knn_prop2", lp_opts),
        # row f-4 end to end: the L-KNN model as a ranker, and the two-step look-ahead planner
        "lknn_d": ("D", "lknn", dict(gamma=0.1, use_clip_as_gamma=False, **lp_opts)),
        "active_search_d": ("D", "active_search",
                            dict(gamma=dict(mode="clip", calibration="sigmoid", a=10.0, b=-0.2), reward_horizon=5,
                                 adjust_horizon=True, max_steps=25, pruning_on=False, implementation="vectorized",
                                 **{**lp_opts, "matrix_options": {**matrix, "symmetric": False}})),
    }
    session_overrides = {"plain_avg": dict(agg_method="avg_score", aug_larger="all", batch_size=1),
                         "knn_prop2_b_avg": dict(agg_method="avg_score", aug_larger="greater", batch_size=1)}
    out = {"names": np.array(list(variants)), "datasets": np.asarray(json.dumps(BENCH_LOOP_DATASETS)),
           "seeds": np.asarray(BENCH_LOOP_SEEDS),
           "knn_pool": np.asarray(BENCH_LOOP_KNN_POOL),
           "variant_dataset": np.array([v[0] for v in variants.values()]),
           "variant_interactive": np.array([v[1] for v in variants.values()]),
           "session_overrides": np.asarray(json.dumps(session_overrides))}
    built = {}
    W_directed = {}
    for key, spec in BENCH_LOOP_DATASETS.items():
        ds = make_dataset("lvis", knn_k=0, **spec["make"])
        ds.embedding.noise = spec["noise"]
        if spec["make"]["tiles_per_image"] == 1 and not spec.get("graph"):  # coarse: no graph-based loop runs on it
            built[key] = (ds, None, None)
            continue
        knn_df = kg.KNNGraph(kg.compute_exact_knn(ds.vectors, n_neighbors=BENCH_LOOP_KNN_POOL)).restrict_k(k=10).knn_df
        W = kg.get_weight_matrix(knn_df, kfun=kg.rbf_kernel(0.05), self_edges=False, normalized=False, symmetric=True)
        # the directed form (every vertex exactly its 9 nearest neighbours: a regular graph, which the look-ahead
        # planner's vectorised implementation requires -- efficient_nonmyopic_search.py:178)
        W_directed[key] = kg.get_weight_matrix(knn_df, kfun=kg.rbf_kernel(0.05), self_edges=False, normalized=False,
                                               symmetric=False)
        L = kg.get_weight_matrix(knn_df, kfun=kg.rbf_kernel(0.05), self_edges=False, normalized=False, symmetric=True,
                                 laplacian=True)
        xlx = np.asarray(ds.vectors.T @ ((L / L.diagonal().sum()) @ ds.vectors))
        built[key] = (ds, W, xlx)
        out[f"ds{key}_knn_rows"] = np.asarray(knn_df.shape[0])

    current = {}

    def fake_wm(idx, options, xlx_matrix=False):
        if xlx_matrix:
            return current["xlx"]
        return current["W"] if options.get("symmetric", True) else W_directed[current["key"]]

    mreg.get_weight_matrix_from_index = fake_wm
    gb.get_weight_matrix_from_index = fake_wm
    for name, (key, interactive, opts) in variants.items():
        ds, current["W"], current["xlx"] = built[key]
        current["key"] = key
        boxes, _ = ds.load_ground_truth()
        is_coarse = BENCH_LOOP_DATASETS[key]["make"]["tiles_per_image"] == 1
        if is_coarse:
            index = coarse.CoarseIndex(embedding=ds.embedding, vectors=ds.vectors, vector_meta=ds.vector_meta)
        else:
            index = msi.MultiscaleIndex(embedding=ds.embedding, vectors=ds.vectors, vector_meta=ds.vector_meta, vec_index=None)
        over = dict(agg_method="plain_score", aug_larger="greater", batch_size=1)
        over.update(session_overrides.get(name, {}))
        p = bt.SessionParams(index_spec=bt.IndexSpec(d_name="lvis", i_name="coarse" if is_coarse else "multiscale", c_name=None),
                             interactive=interactive, interactive_options=opts, shortlist_size=50, **over,
                             # the reference's KnnProp2 never sets curr_qvec, and its start-policy check reads
                             # the multiscale form of getXy (loop_base.py:82-83): both only run from_start
                             start_policy="from_start" if (interactive == "knn_prop2" or is_coarse) else "after_first_batch",
                             index_options={"use_vec_index": False})
        b = bt.BenchParams(name=name, ground_truth_category="c1", qstr="a c1", n_batches=25, max_results=10)
        # loops that fit with L-BFGS draw from torch's generator (nn.Linear start weights, DataLoader shuffle):
        # they are run under three torch seeds so the fixture records how far the reference reproduces ITSELF
        fits = interactive in ("multi_reg", "log_reg2", "pseudo_lr")
        for seed in (BENCH_LOOP_SEEDS if fits else BENCH_LOOP_SEEDS[:1]):
            np.random.seed(0)
            torch.manual_seed(seed)
            captured = []
            orig_fit = mreg.RegModule.fit
            if name == "multi_reg" and seed == BENCH_LOOP_SEEDS[0]:
                # the fits of the session itself, round by round: labelled rows, targets and the coefficients
                # the reference arrived at (pins the HIP fit on the inputs real rounds produce)
                def recording_fit(self, X, y, matchdf, _o=orig_fit):
                    traj = _Trajectory(self, self.weight)
                    ret = _o(self, X, y, matchdf)
                    captured.append(dict(rows=matchdf.index.values.astype(np.int64), y=np.asarray(y, np.float64),
                                         img=matchdf.dbidx.values.astype(np.int64), coeff=self.get_coeff().copy(),
                                         q=self.qvec.numpy().copy(), traj=traj.arrays()))
                    return ret

                mreg.RegModule.fit = recording_fit
            try:
                with contextlib.redirect_stdout(io.StringIO()):
                    session = sess.Session(None, FakeDataset(ds), index, p)
                    res = bench.benchmark_loop(session=session, subset=pr.BitMap(ds.file_meta.index.values),
                                               box_data=boxes, b=b, p=p)
            finally:
                mreg.RegModule.fit = orig_fit
            for r, cap in enumerate(captured[:8]):
                for k in ("rows", "y", "img", "coeff", "q"):
                    out[f"{name}_fit{r}_{k}"] = cap[k]
                if r < 4:  # the closure trajectories are the bulk of the bytes: the first four rounds carry them
                    out[f"{name}_fit{r}_traj_w"], out[f"{name}_fit{r}_traj_loss"], out[f"{name}_fit{r}_traj_grad"] = cap["traj"]
            if captured:
                out[f"{name}_n_fits"] = np.asarray(min(len(captured), 8))
            shown = np.concatenate([np.asarray(a, dtype=np.int64).reshape(-1) for a in session.acc_indices])
            suffix = "" if seed == BENCH_LOOP_SEEDS[0] else f"_seed{seed}"
            out[f"{name}_shown{suffix}"] = shown
            out[f"{name}_nfound{suffix}"] = np.asarray(res["nfound"])
            out[f"{name}_nseen{suffix}"] = np.asarray(res["nseen"])
            print(name, seed, res["nfound"], res["nseen"], shown[:14])
    assert not np.array_equal(out["knn_prop2_b_shown"], out["plain_b_shown"]), "label propagation left no trace"
    save("bench_loop", **out)


def gen_lknn():
    """(f-4) L-KNN active search: the reference's ring-graph known answers (loops/LKNN_model_test.py:7-45) and the
    vectorised two-step look-ahead (_top_sum / efficient_nonmyopic_search 'vectorized') over a planning session on
    a random 10-regular graph: the node chosen and its value every round, the full value vector at some rounds."""
    import contextlib
    import io
    import scipy.sparse as sp
    lm = R.ref("seesaw.loops.LKNN_model")
    ens = R.ref("seesaw.research.active_search.efficient_nonmyopic_search")
    common = R.ref("seesaw.research.active_search.common")
    out = {}
    # ring graph of the reference's own test (loops/LKNN_model_test.py:7-45; the test file passes gamma as a bare
    # float, which LKNNModel.from_dataset no longer accepts -- same graph, gamma = 0.5 per node): its stated answers
    mat = np.zeros((5, 5))
    for i in range(5):
        mat[i, (i + 1) % 5] = 1
    model = lm.LKNNModel.from_dataset(common.Dataset.from_vectors(np.random.default_rng(0).random((5, 10))),
                                      weight_matrix=sp.csr_array(mat + mat.T), gamma=np.full(5, 0.5))
    assert np.isclose(model.predict_proba(np.arange(5)), 0.5).all()
    assert 0.75 <= model.probability_bound(1) and 2.5 / 3 <= model.probability_bound(2)
    out["ring_probs"] = model.predict_proba(np.arange(5))
    out["ring_cond1_ids"], out["ring_cond1"] = model.condition(2, 1).top_k_remaining(top_k=4)
    out["ring_cond0_ids"], out["ring_cond0"] = model.condition(2, 0).top_k_remaining(top_k=4)
    out["ring_bounds"] = np.array([model.probability_bound(1), model.probability_bound(2)])
    # planning session on a random regular graph
    N, D, seed = 3000, 10, 77
    rng = np.random.default_rng(seed)
    nbr = np.stack([rng.choice(N, D, replace=False) for _ in range(N)]).astype(np.int32)
    W = sp.csr_array((np.ones(N * D), nbr.reshape(-1), np.arange(0, N * D + 1, D)), shape=(N, N))
    truth = (rng.random(N) < 0.08).astype(np.int64)
    out["graph_seed"], out["N"], out["D"] = np.asarray(seed), np.asarray(N), np.asarray(D)
    out["truth"] = truth
    r = 0
    for horizon in (2, 9, 20, 101):
        gamma = lm.initial_gamma_array(0.1, N)
        model = lm.LKNNModel.from_dataset(common.Dataset.from_vectors(np.zeros((N, 1))), weight_matrix=W, gamma=gamma)
        picks, values = [], []
        for rnd in range(12):
            with contextlib.redirect_stdout(io.StringIO()):
                res = ens.efficient_nonmyopic_search(model, reward_horizon=horizon, lookahead_limit=2, pruning_on=False,
                                                     implementation="vectorized")
            picks.append(int(res.index))
            values.append(float(res.value))
            if rnd in (0, 5, 11):  # the whole value vector, straight from _top_sum
                numer = model.numerators + model.gamma
                denom = model.denominators + 1
                numer[np.array(model.dataset.seen_indices, dtype=np.int64)] = -np.inf
                with np.errstate(invalid="ignore"):
                    full = ens._top_sum(numerators=numer, denominators=denom, scores=numer / denom,
                                        neighbor_ids_sorted=np.sort(nbr), N=N, K=horizon - 1, D=D)
                out[f"h{horizon}_values_r{rnd}"] = full
            model.condition_(int(res.index), int(truth[int(res.index)]))
        out[f"h{horizon}_picks"], out[f"h{horizon}_values"] = np.asarray(picks), np.asarray(values)
        r += 1
    out["horizons"] = np.asarray([2, 9, 20, 101])
    save("lknn", **out)


def gen_multiregneg():
    """(viii) the multi_reg_neg loop: MultiRegModule.fit (loops/multi_reg_module.py:40-165) on seeded rows -- start
    weights (nn.Linear's draw), the closure trajectory of the first shuffle seed, the fitted weights of all FIT_SEEDS,
    one evaluation with the rows in storage order -- and whole sessions of the loop (loops/multi_reg_neg.py) under the
    simulated user's textual feedback (seesaw_bench.py:246-258, confusion class registered for the synthetic category)."""
    import contextlib
    import io
    import json
    import pandas as pd
    import torch
    from seesaw_amd.synthetic import make_dataset
    mrm = R.ref("seesaw.loops.multi_reg_module")
    out = {}
    i = 0
    # (n, n_pos, n_conf, conf_overlap, l_norm, l_query, q_noise)
    configs = [(60, 8, 6, 0, 100.0, 10.0, 0.8), (150, 20, 15, 3, 100.0, 1.0, 0.8), (100, 12, 0, 0, 100.0, 10.0, 3.0),
               (40, 5, 8, 2, 10.0, 0.0, 0.8)]
    for (n, n_pos, n_conf, overlap, l_norm, l_query, q_noise) in configs:
        X, y, q = _labelled_set(900 + i, n, n_pos, q_noise=q_noise)
        rng = np.random.default_rng(50 + i)
        img = np.sort(rng.integers(0, max(2, n // 3), n))
        yconf = np.zeros(n)
        neg = np.flatnonzero(y == 0)
        pos = np.flatnonzero(y == 1)
        yconf[rng.choice(neg, size=n_conf - overlap, replace=False)] = 1.0
        if overlap:
            yconf[rng.choice(pos, size=overlap, replace=False)] = 1.0  # a vector overlapping boxes of both classes
        ys = np.stack([y, yconf], axis=1).astype("float32")
        matchdf = pd.DataFrame({"dbidx": img, "ys": y, "max_iou": y * 0.5})

        def make():
            torch.manual_seed(3000 + i)  # nn.Linear's start weights: the same for every shuffle seed of a case
            return mrm.MultiRegModule(qvec=torch.from_numpy(q).float(), reg_norm_lambda=l_norm, reg_query_lambda=l_query,
                                      verbose=False, max_iter=100, lr=1.0)

        weights = []
        for seed in FIT_SEEDS:
            model = make()
            w0 = model.weight.detach().clone().numpy()
            traj = _Trajectory(model, model.linear.weight)
            torch.manual_seed(seed)
            losses = model.fit(X, ys, matchdf)
            weights.append(model.weight.detach().clone().numpy())
            if seed == FIT_SEEDS[0]:
                first, first_traj, first_w0 = model, traj, w0
        tw, tl, tg = first_traj.arrays()
        out[f"c{i}_X"], out[f"c{i}_ys"], out[f"c{i}_q"], out[f"c{i}_img"] = X, ys, q, img
        out[f"c{i}_l_norm"], out[f"c{i}_l_query"] = np.asarray(l_norm), np.asarray(l_query)
        out[f"c{i}_w0"] = first_w0
        out[f"c{i}_weight_seeds"] = np.stack(weights)
        out[f"c{i}_coeff"] = first.get_coeff()
        out[f"c{i}_traj_w"], out[f"c{i}_traj_loss"], out[f"c{i}_traj_grad"] = tw, tl, tg
        m0 = make()
        vw = 1.0 / pd.Series(img).map(pd.Series(img).value_counts()).values
        Xc = X - X.mean(axis=0).reshape(1, -1)
        ret = m0._step((torch.from_numpy(Xc), torch.from_numpy(ys), torch.from_numpy(vw)))
        ret["loss"].backward()
        out[f"c{i}_loss0"] = np.asarray(ret["loss"].item())
        out[f"c{i}_grad0"] = m0.weight.grad.numpy().copy()
        out[f"c{i}_parts0"] = np.array([ret[k].item() for k in ["loss_norm", "loss_queryreg", "loss_queryreg2", "vertical_loss",
                                                                "horizontal_loss"]])
        print("multiregneg case", i, "evals", tw.shape[0], "loss", tl[0], "->", tl[-1])
        i += 1
    out["n_cases"] = np.asarray(i)
    out["fit_seeds"] = np.asarray(FIT_SEEDS)

    # ---- whole sessions ------------------------------------------------------------------
    msi = R.ref("seesaw.indices.multiscale.multiscale_index")
    sess = R.ref("seesaw.seesaw_session")
    bench = R.ref("seesaw.seesaw_bench")
    bt = R.ref("seesaw.basic_types")
    mrn = R.ref("seesaw.loops.multi_reg_neg")
    pr = sys.modules["pyroaring"]

    class FakeDataset:
        def __init__(self, d):
            self.d = d
            self.file_meta = d.file_meta
            self.paths = d.paths

        def load_ground_truth(self):
            return self.d.load_ground_truth()

        def get_urls(self, idxbatch):
            return self.d.get_urls(idxbatch)

    spec = BENCH_LOOP_DATASETS["A"]
    ds = make_dataset("lvis", knn_k=0, **spec["make"])
    ds.embedding.noise = spec["noise"]
    boxes, _ = ds.load_ground_truth()
    mrn.get_weight_matrix_from_index = lambda idx, options, xlx_matrix=False: np.zeros((512, 512), np.float32)  # unused by the module
    bench.objnet_dict["c1"] = "c2"  # the synthetic dataset's confusion pair (the reference's table is ObjectNet's)
    out["confusion"] = np.asarray(json.dumps({"c1": "c2"}))
    matrix = dict(knn_path="nndescent60", symmetric=True, self_edges=False, normalized_weights=False, knn_k=10, edist=0.05)
    variants = {"multi_reg_neg": dict(discount_neg=True), "multi_reg_neg_nodiscount": dict(discount_neg=False)}
    out["names"] = np.array(list(variants))
    for name, extra in variants.items():
        opts = dict(reg_norm_lambda=100.0, reg_query_lambda=10.0, reg_data_lambda=0.0, verbose=False, max_iter=100, lr=1.0,
                    matrix_options=matrix, **extra)
        for seed in BENCH_LOOP_SEEDS[:3]:
            index = msi.MultiscaleIndex(embedding=ds.embedding, vectors=ds.vectors, vector_meta=ds.vector_meta, vec_index=None)
            p = bt.SessionParams(index_spec=bt.IndexSpec(d_name="lvis", i_name="multiscale", c_name=None),
                                 interactive="multi_reg_neg", interactive_options=opts, shortlist_size=50,
                                 agg_method="plain_score", aug_larger="greater", batch_size=1,
                                 start_policy="after_first_batch", index_options={"use_vec_index": False})
            b = bt.BenchParams(name=name, ground_truth_category="c1", qstr="a c1", n_batches=25, max_results=10,
                               provide_textual_feedback=True)
            np.random.seed(0)
            torch.manual_seed(seed)
            with contextlib.redirect_stdout(io.StringIO()):
                session = sess.Session(None, FakeDataset(ds), index, p)
                res = bench.benchmark_loop(session=session, subset=pr.BitMap(ds.file_meta.index.values), box_data=boxes,
                                           b=b, p=p)
            shown = np.concatenate([np.asarray(a, dtype=np.int64).reshape(-1) for a in session.acc_indices])
            suffix = "" if seed == BENCH_LOOP_SEEDS[0] else f"_seed{seed}"
            out[f"{name}_shown{suffix}"] = shown
            out[f"{name}_nfound{suffix}"] = np.asarray(res["nfound"])
            out[f"{name}_nseen{suffix}"] = np.asarray(res["nseen"])
            print(name, seed, res["nfound"], res["nseen"], shown[:16])
    out["session_seeds"] = np.asarray(BENCH_LOOP_SEEDS[:3])
    save("multiregneg", **out)


def gen_contweighted():
    """(ii-b) MultiscaleIndex.query(agg_method='avg_score', aug_weight='cont_weighted') -- score_frame2's softmax-of-
    containment branch (multiscale_index.py:133-145) on the 3-level tile pyramid of the multiscale_query family; per
    aug_larger mode the returned images / activations, every candidate image's aggregated best score, and the
    candidate tiles' scores as the reference formed them."""
    msi = R.ref("seesaw.indices.multiscale.multiscale_index")
    pr = sys.modules["pyroaring"]
    pseed, pn = 311, 300
    prng = np.random.default_rng(pseed)
    pmeta = synth_pyramid_meta(pn, np.arange(pn) * 3 + 1, prng)
    PX = orc.synth_rows(pseed, 0, pmeta.shape[0], 512)
    pq = orc.synth_query(pseed)
    pindex = msi.MultiscaleIndex(embedding=None, vectors=PX, vector_meta=pmeta, vec_index=None)
    out = {"pyr_seed": np.asarray(pseed), "pyr_n_images": np.asarray(pn),
           "pyr_meta": pmeta[["dbidx", "zoom_level", "x1", "y1", "x2", "y2"]].values.astype(np.float64)}
    orig_rescore, orig_frame = msi.rescore_candidates, msi.score_frame2
    for aug in ["all", "greater", "adjacent"]:
        seen = {"img": [], "score": []}

        def recording(fullmeta, topk, _o=orig_rescore, **kw):
            seen["rows"] = fullmeta.index.values.astype(np.int64).copy()
            seen["scores"] = fullmeta.score.values.astype(np.float32).copy()
            return _o(fullmeta, topk, **kw)

        def frame(meta_df, _o=orig_frame, **kw):
            tup = _o(meta_df, **kw)
            seen["img"].append(int(meta_df.dbidx.iloc[0]))
            seen["score"].append(float(tup.score.iloc[0]))
            return tup

        msi.rescore_candidates, msi.score_frame2 = recording, frame
        try:
            res = pindex.query(vector=pq, topk=10, shortlist_size=50, exclude=pr.BitMap(pmeta.dbidx.values[:40]),
                               force_exact=True, agg_method="avg_score", aug_larger=aug, aug_weight="cont_weighted",
                               rescore_method=None)
        finally:
            msi.rescore_candidates, msi.score_frame2 = orig_rescore, orig_frame
        out[f"cw_{aug}_dbidxs"] = np.asarray(res["dbidxs"], dtype=np.int64)
        out[f"cw_{aug}_activations"] = np.stack([a[["x1", "y1", "x2", "y2", "dbidx", "score"]].values[0].astype(np.float64)
                                                 for a in res["activations"]])
        out[f"cw_{aug}_cand_rows"], out[f"cw_{aug}_cand_scores"] = seen["rows"], seen["scores"]
        out[f"cw_{aug}_frame_dbidx"] = np.asarray(seen["img"], dtype=np.int64)
        out[f"cw_{aug}_frame_score"] = np.asarray(seen["score"], dtype=np.float64)
    save("contweighted", **out)


def gen_c5_sequence():
    """(vii-b) BASELINE config C5 at its stated small size: the reference's own Session + benchmark_loop over the
    LVIS-shape synthetic dataset bench.py uses (1 109 images x 13 tiles = 14 417 vectors, mediocre text query), 30 rounds,
    batch 1, shortlist 50, for plain / knn_prop2 / multi_reg (ce_loss) / pseudo_lr; the k-NN graph is the reference's
    compute_exact_knn.  Captured: the image returned in every round (fitting loops under three torch seeds).  Takes a
    few minutes (a dense 14 417 x 14 417 distance matrix and ~90 L-BFGS fits): `--check` covers it only when asked for
    by name or with SSW_GOLDEN_ALL=1."""
    import contextlib
    import io
    import torch
    from seesaw_amd.synthetic import make_dataset
    msi = R.ref("seesaw.indices.multiscale.multiscale_index")
    sess = R.ref("seesaw.seesaw_session")
    bench = R.ref("seesaw.seesaw_bench")
    bt = R.ref("seesaw.basic_types")
    kg = R.ref("seesaw.knn_graph")
    mreg = R.ref("seesaw.loops.multi_reg")
    gb = R.ref("seesaw.loops.graph_based")
    pr = sys.modules["pyroaring"]

    class FakeDataset:
        def __init__(self, d):
            self.d = d
            self.file_meta = d.file_meta
            self.paths = d.paths

        def load_ground_truth(self):
            return self.d.load_ground_truth()

        def get_urls(self, idxbatch):
            return self.d.get_urls(idxbatch)

    make = dict(n_images=1109, tiles_per_image=13, n_categories=2, positive_frac=0.05, seed=11)
    ds = make_dataset("lvis", knn_k=0, **make)
    ds.embedding.noise = 1.2
    boxes, _ = ds.load_ground_truth()
    knn_df = kg.KNNGraph(kg.compute_exact_knn(ds.vectors, n_neighbors=11)).restrict_k(k=10).knn_df
    W = kg.get_weight_matrix(knn_df, kfun=kg.rbf_kernel(0.05), self_edges=False, normalized=False, symmetric=True)
    L = kg.get_weight_matrix(knn_df, kfun=kg.rbf_kernel(0.05), self_edges=False, normalized=False, symmetric=True, laplacian=True)
    xlx = np.asarray(ds.vectors.T @ ((L / L.diagonal().sum()) @ ds.vectors))
    fake_wm = lambda idx, options, xlx_matrix=False: xlx if xlx_matrix else W
    mreg.get_weight_matrix_from_index = fake_wm
    gb.get_weight_matrix_from_index = fake_wm
    matrix = dict(knn_path="nndescent60", symmetric=True, self_edges=False, normalized_weights=False, knn_k=10, edist=0.05)
    lp_opts = dict(matrix_options=matrix, normalize_scores=False, sigmoid_before_propagate=True, calib_a=10.0,
                   calib_b=-0.4, prior_weight=1.0)
    logreg_opts = dict(class_weights=1.0, scale="centered", reg_lambda=1.0, max_iter=200.0, lr=1, fit_intercept=False)
    variants = {
        "plain": None,
        "knn_prop2": lp_opts,
        "multi_reg": dict(label_loss_type="ce_loss", rank_loss_margin=0.2, use_qvec_norm=None, reg_data_lambda=0.0,
                          reg_norm_lambda=100.0, reg_query_lambda=0.0, verbose=False, max_iter=200,
                          pos_weight="balanced", lr=1.0, matrix_options=matrix),
        "pseudo_lr": dict(switch_over=True, real_sample_weight=1.0, sample_size=10000, log_reg_params=logreg_opts,
                          label_prop_params=lp_opts),
    }
    import json
    out = {"make": np.asarray(json.dumps(make)), "noise": np.asarray(1.2), "names": np.array(list(variants)),
           "seeds": np.asarray(BENCH_LOOP_SEEDS[:3]), "knn_rows": np.asarray(knn_df.shape[0])}
    quick = bool(os.environ.get("SSW_C5_QUICK"))  # the first torch seed of the fitting loops only: 4 sessions instead of 8
    for name, opts in variants.items():
        fits = name in ("multi_reg", "pseudo_lr")
        for seed in (BENCH_LOOP_SEEDS[:3] if (fits and not quick) else BENCH_LOOP_SEEDS[:1]):
            index = msi.MultiscaleIndex(embedding=ds.embedding, vectors=ds.vectors, vector_meta=ds.vector_meta, vec_index=None)
            p = bt.SessionParams(index_spec=bt.IndexSpec(d_name="lvis", i_name="multiscale", c_name=None), interactive=name,
                                 interactive_options=opts, shortlist_size=50, agg_method="plain_score", aug_larger="greater",
                                 batch_size=1, start_policy="from_start" if name == "knn_prop2" else "after_first_batch",
                                 index_options={"use_vec_index": False})
            b = bt.BenchParams(name=name, ground_truth_category="c1", qstr="a c1", n_batches=30, max_results=10 ** 6)
            np.random.seed(0)
            torch.manual_seed(seed)
            with contextlib.redirect_stdout(io.StringIO()):
                session = sess.Session(None, FakeDataset(ds), index, p)
                res = bench.benchmark_loop(session=session, subset=pr.BitMap(ds.file_meta.index.values), box_data=boxes, b=b, p=p)
            shown = np.concatenate([np.asarray(a, dtype=np.int64).reshape(-1) for a in session.acc_indices])
            suffix = "" if seed == BENCH_LOOP_SEEDS[0] else f"_seed{seed}"
            out[f"{name}_shown{suffix}"] = shown
            out[f"{name}_nfound{suffix}"] = np.asarray(res["nfound"])
            print(name, seed, res["nfound"], res["nseen"], shown[:12])
    save("c5_sequence", **out)


def gen_multireg_det():
    """(iv-c) the RegModule fits of the `multireg` family and the `multi_reg` session of `bench_loop` once more with the
    reference's DataLoader shuffle switched off (rows in storage order): ONE deterministic end point per case, no torch
    seed involved -- what the non-reproducing cases are held to.  The only change to the reference is
    the `shuffle` flag its fit passes to torch's DataLoader."""
    import contextlib
    import io
    import json
    import pandas as pd
    import torch
    from seesaw_amd.synthetic import make_dataset
    mr = R.ref("seesaw.loops.multi_reg")
    g = np.load(os.path.join(GOLDEN, "labelprop.npz"))
    xlx = torch.from_numpy(g["xlx"]).float()
    orig_dl = mr.DataLoader
    mr.DataLoader = lambda ds, batch_size, shuffle=True: orig_dl(ds, batch_size=batch_size, shuffle=False)
    out = {}
    try:
        i = 0
        configs = [(lt, n, n_pos, dl, ql, 0.8) for lt in ["ce_loss", "pairwise_rank_loss", "pairwise_logistic_loss"]
                   for (n, n_pos, dl, ql) in [(60, 8, 0.0, 0.0), (150, 20, 1000.0, 10.0)]]
        configs += [(lt, 100, 12, 0.0, 1.0, 3.0) for lt in ["pairwise_rank_loss", "pairwise_logistic_loss", "ce_loss"]]
        for (loss_type, n, n_pos, data_lam, query_lam, q_noise) in configs:
            X, y, q = _labelled_set(700 + i, n, n_pos, q_noise=q_noise)
            rng = np.random.default_rng(i)
            img = np.sort(rng.integers(0, max(2, n // 3), n))
            matchdf = pd.DataFrame({"dbidx": img, "ys": y, "max_iou": y * 0.5})
            model = mr.RegModule(dim=512, xlx_matrix=xlx, qvec=torch.from_numpy(q).float(), label_loss_type=loss_type,
                                 rank_loss_margin=0.2, reg_data_lambda=data_lam, reg_norm_lambda=100.0, use_qvec_norm=None,
                                 reg_query_lambda=query_lam, verbose=False, max_iter=200, pos_weight="balanced", lr=1.0)
            traj = _Trajectory(model, model.weight)
            model.fit(X, y, matchdf)
            out[f"c{i}_coeff"] = model.get_coeff().copy()
            out[f"c{i}_final_loss"] = np.asarray(traj.arrays()[1][-1])
            out[f"c{i}_evals"] = np.asarray(len(traj.loss))
            i += 1
        out["n_cases"] = np.asarray(i)
        # the multi_reg session of bench_loop (dataset A), shuffle off
        msi = R.ref("seesaw.indices.multiscale.multiscale_index")
        sess = R.ref("seesaw.seesaw_session")
        bench = R.ref("seesaw.seesaw_bench")
        bt = R.ref("seesaw.basic_types")
        pr = sys.modules["pyroaring"]

        class FakeDataset:
            def __init__(self, d):
                self.d = d
                self.file_meta = d.file_meta
                self.paths = d.paths

            def load_ground_truth(self):
                return self.d.load_ground_truth()

            def get_urls(self, idxbatch):
                return self.d.get_urls(idxbatch)

        spec = BENCH_LOOP_DATASETS["A"]
        ds = make_dataset("lvis", knn_k=0, **spec["make"])
        ds.embedding.noise = spec["noise"]
        boxes, _ = ds.load_ground_truth()
        matrix = dict(knn_path="nndescent60", symmetric=True, self_edges=False, normalized_weights=False, knn_k=10, edist=0.05)
        opts = dict(label_loss_type="ce_loss", rank_loss_margin=0.2, use_qvec_norm=None, reg_data_lambda=0.0,
                    reg_norm_lambda=100.0, reg_query_lambda=0.0, verbose=False, max_iter=200, pos_weight="balanced", lr=1.0,
                    matrix_options=matrix)
        mr.get_weight_matrix_from_index = lambda idx, options, xlx_matrix=False: np.zeros((512, 512), np.float32)  # unused: reg_data_lambda = 0
        index = msi.MultiscaleIndex(embedding=ds.embedding, vectors=ds.vectors, vector_meta=ds.vector_meta, vec_index=None)
        p = bt.SessionParams(index_spec=bt.IndexSpec(d_name="lvis", i_name="multiscale", c_name=None), interactive="multi_reg",
                             interactive_options=opts, shortlist_size=50, agg_method="plain_score", aug_larger="greater",
                             batch_size=1, start_policy="after_first_batch", index_options={"use_vec_index": False})
        b = bt.BenchParams(name="multi_reg", ground_truth_category="c1", qstr="a c1", n_batches=25, max_results=10)
        np.random.seed(0)
        torch.manual_seed(0)
        with contextlib.redirect_stdout(io.StringIO()):
            session = sess.Session(None, FakeDataset(ds), index, p)
            res = bench.benchmark_loop(session=session, subset=pr.BitMap(ds.file_meta.index.values), box_data=boxes, b=b, p=p)
        out["multi_reg_shown"] = np.concatenate([np.asarray(a, dtype=np.int64).reshape(-1) for a in session.acc_indices])
        out["multi_reg_nfound"] = np.asarray(res["nfound"])
        print("multi_reg session, shuffle off:", res["nfound"], res["nseen"], out["multi_reg_shown"])
    finally:
        mr.DataLoader = orig_dl
    save("multireg_det", **out)


TILING_SIZES, tiling_image = orc.TILING_SIZES, orc.tiling_image


def gen_sliding():
    """VERDICT r3 "What's missing" #4: SlidingWindow / gen_strided_blocks (seesaw/models/embeddings.py:252-281, 344-378)
    on seeded tensors with a stand-in kernel (per-window channel means and a corner pixel): the window order, the output
    layout [1, C, len(iis), len(jjs)] and the index lists."""
    import torch
    emb = R.ref("seesaw.models.embeddings")

    class Kernel(torch.nn.Module):
        def forward(self, x):
            return torch.cat([x.mean(dim=(2, 3)), x[:, :, 0, 0], x[:, :, -1, -1]], dim=1)  # [n, 9]

    out = {}
    rng = np.random.default_rng(31)
    for tag, (h, w, ks, st) in {"a": (448, 560, 224, 112), "b": (224, 224, 224, 112), "c": (300, 500, 224, 112), "d": (20, 33, 8, 3)}.items():
        x = rng.standard_normal((1, 3, h, w)).astype(np.float32)
        batch, iis, jjs = emb.gen_strided_blocks(torch.from_numpy(x), ks, st, flatten=True)
        v = emb.SlidingWindow(Kernel(), kernel_size=ks, stride=st, center=True)(torch.from_numpy(x))
        out[f"{tag}_shape"] = np.array([h, w, ks, st], dtype=np.int32)
        out[f"{tag}_iis"], out[f"{tag}_jjs"] = np.array(iis, dtype=np.int32), np.array(jjs, dtype=np.int32)
        out[f"{tag}_batch_shape"] = np.array(batch.shape, dtype=np.int32)
        out[f"{tag}_out"] = v.numpy()
    save("sliding", **out)


class _TileFrame:
    """what batch_tx touches of its DataFrame argument -- `.tile.values` (a ray TensorArray: `to_numpy()`) and
    `.assign(tile=...)` -- around the stand-in TensorArray of _ref_import (ray's pandas extension type is not in this
    image; the arithmetic between the two calls is the reference's own)"""

    class _Col:
        def __init__(self, values):
            self.values = values

    def __init__(self, tiles):
        ta = sys.modules["ray.data.extensions"].TensorArray
        self.tile = self._Col(tiles if isinstance(tiles, ta) else ta(tiles))

    def assign(self, tile):
        return _TileFrame(tile)


def gen_tiling():
    """VERDICT r3 #4 (row f-3): the reference's tiler and tile normalisation on seeded images --
    generate_multiscale_tiling (seesaw/indices/multiscale/multiscale_tools.py:96-117: pyramid :16-48, strided_tiling
    :80-94) and batch_tx (:167-183).  Per image: every tile's box, zoom level, scale factor, patch id, a CRC of its
    pixels and a CRC of its normalised f32 CHW tensor; for the first image the normalised tensor of two tiles in full."""
    import zlib
    import pandas as pd
    import PIL.Image
    mt = R.ref("seesaw.indices.multiscale.multiscale_tools")
    out = {"sizes": np.array(TILING_SIZES, dtype=np.int32)}
    for i, (w, h) in enumerate(TILING_SIZES):
        arr = tiling_image(w, h, seed=100 + i)
        for mts, tag in ((224, f"im{i}"),) + (((112, f"im{i}_min112"),) if i in (0, 6) else ()):
            df = mt.generate_multiscale_tiling(PIL.Image.fromarray(arr), factor=0.5, tile_size=224, min_tile_size=mts)
            tiles = np.stack([np.asarray(t) for t in df.tile.values])
            assert tiles.dtype == np.uint8 and tiles.shape[1:] == (224, 224, 3)
            norm = np.stack(mt.batch_tx(_TileFrame(tiles)).tile.values.to_numpy())
            assert norm.dtype == np.float32 and norm.shape[1:] == (3, 224, 224)
            out[f"{tag}_boxes"] = df[["x1", "y1", "x2", "y2"]].to_numpy(dtype=np.float32)
            out[f"{tag}_zoom_level"] = df.zoom_level.to_numpy(dtype=np.int16)
            out[f"{tag}_max_zoom_level"] = df.max_zoom_level.to_numpy(dtype=np.int16)
            out[f"{tag}_scale_factor"] = df.scale_factor.to_numpy(dtype=np.float32)
            out[f"{tag}_patch_id"] = df.patch_id.to_numpy(dtype=np.int16)
            out[f"{tag}_tile_crc"] = np.array([zlib.crc32(t.tobytes()) for t in tiles], dtype=np.uint32)
            out[f"{tag}_norm_crc"] = np.array([zlib.crc32(np.ascontiguousarray(t).tobytes()) for t in norm], dtype=np.uint32)
            if i == 0 and mts == 224:
                out["im0_norm_tiles_0_12"] = norm[[0, 12]]
    save("tiling", **out)


def gen_avg_score_edges():
    """(ii-c) score_frame2 (multiscale_index.py:112-150) itself, one image at a time, on the seeded edge layouts of
    tests/_rescore_helpers.py: images of 1 .. 2048 tiles (the device kernel has 256 threads and an LDS ceiling of 2048
    tiles), zoom levels up to 31, exactly tied IoUs and scores, a zero-area box, NaN / +inf / -inf scores.  The inputs
    regenerate from the helper's seed; recorded per mode are every image's best row (inside the image) and score, and the
    per-tile aggregates of the images of at most 513 tiles (`agg_*`, concatenated in image order).
    Modes `<weight>_<aug>_<dtype>_<scores>`: weight lm (level_max) | cw (cont_weighted); the three aug_larger modes;
    f32 | f64 score columns; scores fin (finite) | ld (with the NaN / inf plants) | ldm (ld minus the helper's `minus`
    vector, f32 only).  cont_weighted runs on the finite scores only.  The image of zero-area tiles is left out: with
    every aggregate NaN the reference's frame is empty and its caller raises.  The pandas join of the 2048-tile image
    (~1.5 M pairs) runs in seconds here, so every image is recorded from the full layout."""
    import pandas as pd
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    try:
        import _rescore_helpers as H
    finally:
        sys.path.pop(0)
    msi = R.ref("seesaw.indices.multiscale.multiscale_index")
    lay = H.Layout()
    images = [p for p in range(lay.n_images) if p != lay.all_nan_position]
    out = {"seed": np.asarray(H.SEED), "tile_counts": np.asarray([lay.tile_counts[p] for p in images], dtype=np.int64),
           "agg_max_tiles": np.asarray(513)}
    modes = [("lm", aug, dt, sc) for aug in H.AUGS for dt in ("f32", "f64") for sc in ("fin", "ld")]
    modes += [("lm", aug, "f32", "ldm") for aug in H.AUGS]
    modes += [("cw", aug, dt, "fin") for aug in H.AUGS for dt in ("f32", "f64")]
    for weight, aug, dt, sc in modes:
        dtype = np.float32 if dt == "f32" else np.float64
        scores = lay.scores(dtype, loaded=sc != "fin")
        if sc == "ldm":
            scores = scores - lay.minus()
        best_row, best_score, aggs = [], [], []
        for p in images:
            r = lay.rows(p)
            b = lay.boxes[r]
            meta = pd.DataFrame({"dbidx": np.full(b.shape[0], p, dtype=np.int64), "zoom_level": lay.zoom[r].astype(np.int16),
                                 "x1": b[:, 0], "y1": b[:, 1], "x2": b[:, 2], "y2": b[:, 3], "score": scores[r]})
            seen = {}
            orig_assign = pd.DataFrame.assign

            def assign(self, _o=orig_assign, **kw):  # the per-tile aggregates, as score_frame2 attaches them
                if "unadjusted_score" in kw:
                    seen["agg"] = np.asarray(_o(self, **kw).score.values).copy()
                return _o(self, **kw)

            pd.DataFrame.assign = assign
            try:
                tup = msi.score_frame2(meta, agg_method="avg_score", aug_larger=aug,
                                       aug_weight={"lm": "level_max", "cw": "cont_weighted"}[weight])
            finally:
                pd.DataFrame.assign = orig_assign
            assert tup.shape[0] == 1 and seen["agg"].dtype == dtype, (p, tup.shape, seen["agg"].dtype)
            best_row.append(int(tup.index[0]))
            best_score.append(tup.score.iloc[0])
            if b.shape[0] <= 513:
                aggs.append(seen["agg"])
        tag = f"{weight}_{aug}_{dt}_{sc}"
        out[f"row_{tag}"] = np.asarray(best_row, dtype=np.int64)
        out[f"score_{tag}"] = np.asarray(best_score, dtype=dtype)
        out[f"agg_{tag}"] = np.concatenate(aggs).astype(dtype)
        print(tag, best_row)
    save("avg_score_edges", **out)


FAMILIES = {"tiling": gen_tiling, "sliding": gen_sliding, "lknn": gen_lknn, "scan_topk": gen_scan_topk, "multiscale_query": gen_multiscale_query, "labelprop": gen_labelprop,
            "rank_loss": gen_rank_loss, "logreg": gen_logreg, "multireg": gen_multireg, "bench_loop": gen_bench_loop,
            "multiregneg": gen_multiregneg, "contweighted": gen_contweighted, "avg_score_edges": gen_avg_score_edges,
            "c5_sequence": gen_c5_sequence, "multireg_det": gen_multireg_det}
HEAVY = {"c5_sequence"}  # minutes each: regenerated only when named or with SSW_GOLDEN_ALL=1

def main(argv):
    """python oracle/gen_golden.py [--check] [family ...]
    --check: regenerate into a scratch directory and fail on any byte of any array that differs from the
    committed tests/golden/*.npz (run by tests/test_golden_regen_cpu.py where /root/reference exists)."""
    global OUT_DIR
    check = "--check" in argv
    names = [a for a in argv if not a.startswith("--")] or [f for f in FAMILIES
                                                           if f not in HEAVY or os.environ.get("SSW_GOLDEN_ALL")]
    if not check:
        for nm in names:
            print(f"== {nm}")
            FAMILIES[nm]()
        return 0
    import tempfile
    bad = 0
    with tempfile.TemporaryDirectory(prefix="ssw_golden_") as tmp:
        OUT_DIR = tmp
        for nm in names:
            print(f"== {nm}")
            FAMILIES[nm]()
            diffs = compare_npz(os.path.join(GOLDEN, nm + ".npz"), os.path.join(tmp, nm + ".npz"),
                                b_may_be_a_slice=(nm == "c5_sequence" and bool(os.environ.get("SSW_C5_QUICK"))))
            for d in diffs:
                print(f"   DIFF {nm}: {d}")
            print(f"   {nm}: {'reproduced byte for byte' if not diffs else f'{len(diffs)} arrays differ'}")
            bad += bool(diffs)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))

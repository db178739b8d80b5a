"""GPU: every way to the index's top-k on ONE long-lived handle, in sequence -- host top-k pruned and full, a batch with
a mass-tie query in the middle of a chunk, the resident scores afterwards, the device form with an exchange target, the
enqueue / collect halves under the fused label-propagation round, the one-launch form of a small index -- each step
against the same call on a fresh handle with the pruning off (the first also against the kernel-order oracle), and the
profiling pairs each kind of call records.  Every comparison is exact.  One step goes beyond what the code did before
the paths were joined: topk(None) on a small index whose buffer a pruned scan left partial used to select over the lower
bounds; it completes the buffer first now, as the enqueue half under the fused round always did.

The sequence runs at two shapes.  dim 256 / ~40 000 rows: no multi-query kernel serves it (scan.hip:
scan_batch_max_width needs dim 512 and 65 536 rows), so a batch of 5 is five single-query scans.  dim 512 / ~70 000 rows:
the batch of 5 is a chunk of 4 into the side slabs plus a single query, 2 profiling pairs."""
import numpy as np
import pytest
import scipy.sparse as sp

from _prune_helpers import mode, same, stats

pytestmark = pytest.mark.gpu

K = 50


def ragged(n_images, seed):
    counts = np.random.default_rng(seed).integers(1, 4, size=n_images)  # 1-3 rows an image
    return np.repeat(np.arange(n_images), counts).astype(np.int32)


def ring_graph(n):
    """any symmetric graph: the round below makes the prior the result, nothing is propagated over it"""
    i = np.arange(n)
    W = sp.coo_array((np.full(n, 0.05), (i, (i + 1) % n)), shape=(n, n)).tocsr()
    W = (W + W.T).tocsr()
    W.sort_indices()
    return W


def fused_round(lp, idx, ids, excluded, k):
    import contextlib
    import io
    with contextlib.redirect_stdout(io.StringIO()):
        return lp.round(idx, propagate=False, label_ids=ids, label_values=np.ones(ids.shape[0]), mask_labeled=True,
                        excluded=excluded, k=k)


def three_calls(lp, idx, ids, excluded, k):
    lp.prior_as_result(ids)
    lp.scores_to_index(idx, mask_labeled=True)
    return idx.topk(None, k, excluded=excluded)


@pytest.mark.parametrize("dim,n_images,chunked", [(256, 20000, False), (512, 35000, True)])
def test_one_handle_through_every_topk_path(lab_build, oracle, dim, n_images, chunked):
    import torch
    from seesaw_amd import _lib
    from seesaw_amd.device_index import DeviceIndex
    from seesaw_amd.label_propagation import LabelPropagation
    from seesaw_amd.sharded import ShardedTopK

    rng = np.random.default_rng(dim)
    row2image = ragged(n_images, seed=dim)
    n = row2image.shape[0]
    assert n_images > 8192 and (not chunked or n >= 65536)
    X = oracle.synth_rows(11, 0, n, dim)
    base = oracle.synth_rows(1, 0, 1, dim)[0]
    tied = (row2image >= 6000) & (row2image < 18000)  # 12 000 images with one score for the query `base`: deep rerun
    X[tied] = base[None, :] * np.float32(0.5)
    Q = np.stack([oracle.synth_query(20 + i, dim) for i in range(8)])
    Q[2] = base
    excl = [rng.integers(0, n_images, 300).tolist(), None, [5, 5, 9, 17999], list(range(0, 6000, 3)), [7]]

    def fresh():
        return DeviceIndex.from_numpy(X, row2image=row2image)

    def on_fresh(fn, make=fresh):
        """fn(handle) on a fresh handle with the pruning off; the pruning is forced on again afterwards"""
        mode(lab_build, False)
        ref = make()
        try:
            return fn(ref)
        finally:
            ref.close()
            mode(lab_build, True, min_rows=1)

    idx = fresh()
    lp = LabelPropagation(ring_graph(n), reg_lambda=1.0, max_iter=10)
    lp.set_prior(rng.uniform(0.05, 0.95, n))
    n_small, tiles = 1000, 13
    Xs = oracle.synth_rows(12, 0, n_small * tiles, dim)
    small_map = np.repeat(np.arange(n_small, dtype=np.int32), tiles)

    def fresh_small():
        return DeviceIndex.from_numpy(Xs, row2image=small_map)

    small = fresh_small()
    lp_small = LabelPropagation(ring_graph(n_small * tiles), reg_lambda=1.0, max_iter=10)
    lp_small.set_prior(rng.uniform(0.05, 0.95, n_small * tiles))
    dev = torch.device("cuda", 0)
    try:
        mode(lab_build, True, min_rows=1)
        assert stats(idx)[1] == 1

        # host top-k with exclusions, pruned: the oracle's and the full scan's
        got = idx.topk(Q[0], K, excluded=excl[0])
        st = stats(idx)
        assert st[3] == 1 and st[2] >= K, st  # pruned, and the score buffer is partial now
        o = oracle.topk_images_tiebreak(oracle.scores_kernel_order(X, Q[0]), row2image, n_images, excl[0], K)
        same(o, got)
        same(on_fresh(lambda r: r.topk(Q[0], K, excluded=excl[0])), got)

        # a batch on the partial buffer; query 2, inside the first chunk, ties on 12 000 images
        ref = on_fresh(lambda r: [r.topk(Q[i], K, excluded=excl[i]) for i in range(5)])
        assert ref[2][1][0] == ref[2][1][-1]  # the tied score fills the result
        batch = idx.topk_batch(Q[:5], K, excluded=excl)
        for r, g in zip(ref, batch):
            same(r, g)
        assert stats(idx)[3] == 1  # no query of a batch is pruned

        # the resident scores are the last query's, complete
        same(ref[4], idx.topk(None, K, excluded=excl[4]))
        probe = np.arange(0, n, 97)
        full4 = on_fresh(lambda r: r.scores(Q[4]))
        same([full4[probe]], [idx.gather_scores(probe)])

        # the device form with an exchange target: the message of a handle that scans in full
        q_dev = torch.from_numpy(Q[5]).to(dev)
        torch.cuda.synchronize()

        def message(handle):
            x = ShardedTopK(rank=0, world=1, device=dev, image_offset=0, k_max=16, with_best=True)
            torch.cuda.synchronize()
            x.attach(handle)
            handle.set_excluded(excl[3])
            handle.topk_dev(q_dev.data_ptr(), 16)
            handle.sync()
            return x, x.send_buf.cpu().numpy().copy()

        _, want_msg = on_fresh(message)
        before = stats(idx)[3]
        x, msg = message(idx)
        assert stats(idx)[3] == before + 1
        same([want_msg], [msg])
        assert int(msg[-1]) & 0xFFFFFFFF == 16
        with pytest.raises(_lib.SeesawHipError, match="k_max"):
            idx.topk(Q[6], 17)
        same(on_fresh(lambda r: r.topk(Q[6], 16, excluded=excl[0])), idx.topk(Q[6], 16, excluded=excl[0]))
        idx.topk_dev(q_dev.data_ptr(), 16)  # the exclusions of the call before stay installed
        same(on_fresh(lambda r: r.topk(Q[5], 16, excluded=excl[0])), idx.topk_fetch(16))
        _lib.call("ssw_index_set_exchange_target", idx._h, None, 0, 0, 0, 0)
        same(on_fresh(lambda r: r.topk(Q[6], 17)), idx.topk(Q[6], 17))

        # one pair of profiling events per scan, or per whatever replaces it
        idx.profile(True)
        before = stats(idx)[3]
        idx.topk(Q[0], K)
        assert stats(idx)[3] == before + 1
        assert idx.profile_read().shape[0] == 1
        mode(lab_build, False)
        idx.topk(Q[0], K)
        assert idx.profile_read().shape[0] == 1
        mode(lab_build, True, min_rows=1)
        idx.topk_batch(Q[:5], K)
        assert idx.profile_read().shape[0] == (2 if chunked else 5)
        idx.scores(Q[0])
        assert idx.profile_read().shape[0] == 1
        idx.profile(False)

        # a small index pruned (an exclusion list longer than the one-launch form takes sends it through the general
        # form), then topk(None): the partial buffer is completed before the one-launch selection reads it
        long_excl = [3] * 8200 + [10, 20]
        want = on_fresh(lambda r: (r.topk(Q[3], K, excluded=long_excl), r.topk(None, K, excluded=[7])), make=fresh_small)
        got = small.topk(Q[3], K, excluded=long_excl)
        st = stats(small)
        assert st[3] == 1 and st[4] == 0 and st[2] >= K, st  # pruned without a fallback: the buffer holds lower bounds
        same(want[0], got)
        same(want[1], small.topk(None, K, excluded=[7]))

        # the enqueue / collect halves (fused round) between two host calls: the one-launch form of the small index, then
        # the general form (the round takes the row pointer of its index: that handle is never pruned again)
        for handle, prop, n_img, make in ((small, lp_small, n_small, fresh_small), (idx, lp, n_images, fresh)):
            ids = rng.choice(handle.n_rows, 40, replace=False).astype(np.int64)
            ex = np.sort(rng.choice(n_img, 25, replace=False)).astype(np.int64)
            mode(lab_build, False)
            r = make()
            try:
                want = [r.topk(Q[7], K, excluded=[3]), three_calls(prop, r, ids, ex, K), r.topk(Q[1], K)]
            finally:
                r.close()
                mode(lab_build, True, min_rows=1)
            same(want[0], handle.topk(Q[7], K, excluded=[3]))
            same(want[1], fused_round(prop, handle, ids, ex, K))
            same(want[1], handle.topk(None, K, excluded=ex))
            same(want[2], handle.topk(Q[1], K))
        assert stats(idx)[1] == 0
    finally:
        mode(lab_build, True)
        lp.close()
        lp_small.close()
        idx.close()
        small.close()

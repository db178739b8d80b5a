"""GPU: both stages of the sharded batch in one process (ssw_index_topk_batch_dev[_pruned], ssw_topk_merge_msgs_batch_dev,
ssw_index_stage2_avg_batch_dev, seesaw_amd.sharded.combine_stage2_block).  The image pyramid of
tests/golden/multiscale_query.npz is cut at an image boundary into handles A and B, which play rank 0 and rank 1
(image_offset / row_offset set accordingly); their blocks are stacked by hand as one all-gather leaves them.  The
reference is a third handle W over the whole index: `topk(q)` and then `rescore_avg` of the selected images in
ascending position, what the single sharded query computes.  Every (position, score, row) is compared exactly: the
second stage scores its tiles in the scan's summation order and runs the one aggregation."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _prune_helpers import mode  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
K_MAX, K, N_SLOTS, NQ_MAX = 64, 50, 16, 19
NQS = (1, 2, 3, 16, 19)  # 19: a second group of three queries through the 16-slot block


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


class ThreeHandles:
    def __init__(self, oracle, dtype):
        import torch
        from seesaw_amd.device_index import DeviceIndex
        self.torch, self.dev = torch, torch.device("cuda", 0)
        g = np.load(os.path.join(GOLDEN, "multiscale_query.npz"))
        m, seed = g["pyr_meta"], int(g["pyr_seed"])
        r2i = np.unique(m[:, 0], return_inverse=True)[1].astype(np.int64)
        assert (np.diff(r2i) >= 0).all()  # rows sorted by image
        boxes, zoom = m[:, 2:6].astype(np.float32), m[:, 1].astype(np.int32)
        X = oracle.synth_rows(seed, 0, m.shape[0], 512)
        self.n_images = int(r2i[-1]) + 1
        self.img_cut = self.n_images // 2 + 7
        self.row_cut = int(np.searchsorted(r2i, self.img_cut))
        parts = [(0, self.row_cut, 0), (self.row_cut, m.shape[0], self.img_cut), (0, m.shape[0], 0)]
        self.handles = []
        for lo, hi, img0 in parts:
            h = DeviceIndex.from_numpy(X[lo:hi], row2image=(r2i[lo:hi] - img0).astype(np.int32), device=0, dtype=dtype)
            h.set_tile_meta(boxes[lo:hi], zoom[lo:hi])
            h.set_stream(torch.cuda.current_stream(self.dev).cuda_stream)
            self.handles.append(h)
        self.ranks, self.W = self.handles[:2], self.handles[2]
        self.offsets = [(0, 0), (self.img_cut, self.row_cut)]
        self.msg_len = 2 * K_MAX + 1
        self.blocks = [torch.full((N_SLOTS, self.msg_len), -1, dtype=torch.int64, device=self.dev) for _ in range(2)]
        self.stage2 = [torch.full((N_SLOTS, 2, K_MAX), -1, dtype=torch.int64, device=self.dev) for _ in range(2)]
        for r, h in enumerate(self.ranks):
            h.set_exchange_target_batch(self.blocks[r].data_ptr(), N_SLOTS, K_MAX, True, *self.offsets[r])
        self.Q = np.stack([oracle.synth_query(seed + 10 + b) for b in range(NQ_MAX)])
        rng = np.random.default_rng(3)
        self.excluded = [None if b % 3 == 0 else rng.integers(0, self.n_images, 40).tolist() for b in range(NQ_MAX)]

    def reference(self, aug, wgt):
        """W: topk, then rescore_avg of the selected images in ascending position (the scores of q are resident)"""
        out = []
        for b in range(NQ_MAX):
            imgs, _, _ = self.W.topk(self.Q[b], K, excluded=self.excluded[b])
            pos = np.sort(imgs)
            s, r = self.W.rescore_avg(pos, aug, aug_weight=wgt)
            out.append((pos, s, r))
        return out

    def local(self, excluded, r):
        lo = self.offsets[r][0]
        hi = self.img_cut if r == 0 else self.n_images
        return [[] if e is None else [int(i) - lo for i in e if lo <= int(i) < hi] for e in excluded]

    def group(self, Qg, excluded, aug, wgt, prune=False):
        """one group of nq <= N_SLOTS queries: first stage on A and B, one merge, second stage on A and B, the combine
        -> per query (positions ascending, scores, rows)"""
        from seesaw_amd import _lib
        from seesaw_amd.device_index import decode_keys
        from seesaw_amd.sharded import combine_stage2_block
        torch, nq = self.torch, Qg.shape[0]
        for r, h in enumerate(self.ranks):
            h.topk_batch_dev(Qg, K, excluded=self.local(excluded, r), prune=prune)
        gathered = torch.stack([b[:nq] for b in self.blocks]).contiguous()
        keys = torch.zeros((nq, K_MAX), dtype=torch.int64, device=self.dev)
        counts = torch.zeros(nq, dtype=torch.int32, device=self.dev)
        flags = torch.full((nq, 2), -1, dtype=torch.int64, device=self.dev)
        seen = torch.zeros(1, dtype=torch.int64, device=self.dev)
        _lib.call("ssw_topk_merge_msgs_batch_dev", 0, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream),
                  ctypes.c_void_p(gathered.data_ptr()), 2, nq * self.msg_len, nq, K_MAX, 1, K,
                  ctypes.c_void_p(keys.data_ptr()), ctypes.c_void_p(counts.data_ptr()), ctypes.c_void_p(flags.data_ptr()),
                  ctypes.c_void_p(seen.data_ptr()))
        for r, h in enumerate(self.ranks):
            h.stage2_avg_batch_dev(Qg, keys.data_ptr(), counts.data_ptr(), K_MAX, K, aug, self.stage2[r].data_ptr(),
                                   image_offset=self.offsets[r][0], row_offset=self.offsets[r][1], aug_weight=wgt)
        torch.cuda.synchronize()
        assert not flags.cpu().numpy().any()
        counts_h, keys_h = counts.cpu().numpy(), keys.cpu().numpy().view(np.uint64)
        assert counts_h.tolist() == [K] * nq
        block = torch.stack([s[:nq] for s in self.stage2]).cpu().numpy()
        scores, rows = combine_stage2_block(block, counts_h, K_MAX)
        out = []
        for b in range(nq):
            pos, _ = decode_keys(keys_h[b, :K])
            order = np.argsort(pos, kind="stable")
            out.append((pos[order], scores[b, :K][order], rows[b, :K][order]))
        return out

    def batch(self, nq, aug, wgt, prune=False):
        out = []
        for g in range(0, nq, N_SLOTS):
            out += self.group(self.Q[g:min(nq, g + N_SLOTS)], self.excluded[g:min(nq, g + N_SLOTS)], aug, wgt, prune)
        return out

    def close(self):
        for h in self.handles:
            h.close()


def same(got, want, where):
    assert np.array_equal(got[0], want[0]), where
    assert np.array_equal(bits(got[1]), bits(want[1])), where
    assert np.array_equal(got[2], want[2]), where


@pytest.fixture(scope="module", params=["float32", "float16"])
def three(request, oracle):
    t = ThreeHandles(oracle, request.param)
    t.want = t.reference("greater", "level_max")
    yield t
    t.close()


@pytest.mark.parametrize("nq", NQS)
def test_two_ranks_and_the_combine_equal_the_whole_index(three, nq):
    got = three.batch(nq, "greater", "level_max")
    assert len(got) == nq
    for b in range(nq):
        same(got[b], three.want[b], b)
    # both ranks own some of every query's candidates: the cut runs through the shortlist
    assert all(0 < int((three.want[b][0] < three.img_cut).sum()) < K for b in range(nq))


def test_cont_weighted_and_all(three):
    want = three.reference("all", "cont_weighted")
    got = three.batch(3, "all", "cont_weighted")
    for b in range(3):
        same(got[b], want[b], b)


@pytest.mark.parametrize("dtype", ["float32", "float16"])
def test_behind_the_pruned_first_stage(oracle, dtype):
    """the lab build prunes from one row on: the slabs hold bounds outside the survivors, the second stage does not read
    them, and nothing completes a slab"""
    from seesaw_amd import _lib
    with _lib.debug_hooks() as lib:
        try:
            mode(lib, False)
            t = ThreeHandles(oracle, dtype)
            try:
                want = t.reference("greater", "level_max")  # pruning off
                mode(lib, True, 1)
                before = [h.prune_stats(completions=True) for h in t.ranks]
                got = t.batch(NQ_MAX, "greater", "level_max", prune=True)
                after = [h.prune_stats(completions=True) for h in t.ranks]
                for b in range(NQ_MAX):
                    same(got[b], want[b], b)
                for a, z in zip(before, after):
                    assert z["queries"] == a["queries"] + NQ_MAX  # the first stage really was the pruned one
                    assert z["completions"] == a["completions"] and z["rescored_rows"] == a["rescored_rows"]
            finally:
                t.close()
        finally:
            mode(lib, True)

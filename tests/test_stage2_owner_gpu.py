"""GPU: the owner-side second stage of a sharded batch (ssw_index_stage2_avg_batch_dev; csrc/rescore.hip,
k_avg_score_owner) through the product entry on ONE handle.  The expected value of every owned entry is what the same
handle returns for `scores(q_b)` followed by `rescore_avg(positions, aug)`: the kernel scores the tiles itself, in the
scan's summation order, and runs the one aggregation, so the comparison is on bit patterns and there is no tolerance to
choose.  For `level_max` the aggregate is also compared with the oracle's restatement over those scores.

Layouts: `_rescore_helpers.Layout()` at dim 256 (tile counts 1, 2, 63 .. 257 .. 2048: the 256-thread loops and the
64 KiB + 4 B LDS line) and a small one with 1, 3, 4, 5, 8 and 13 tiles (around the four waves and the two rows a wave
keeps in flight) at dims 512, 768 and 1024; f32 and f16 rows drawn by the oracle's generator."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _rescore_helpers import AUGS, LEVEL_SETS, SIDES, Layout  # noqa: E402

pytestmark = pytest.mark.gpu

NQ_MAX = 16
K_MAX, K = 24, 20
FILL = np.uint64(0xA5A5A5A5A5A5A5A5)
OWNED = np.uint64(1) << np.uint64(32)
WEIGHTS = ("level_max", "cont_weighted")
OFFSETS = ((0, 0), (1000, 2 ** 33 + 5))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


class SmallLayout:
    """images of 1, 3, 4, 5, 8 and 13 tiles and one of 8 zero-area tiles; boxes and levels drawn as Layout draws them"""

    def __init__(self, seed=77):
        rng = np.random.default_rng(seed)
        counts = [1, 3, 4, 5, 8, 13, 8]
        self.tile_counts, self.n_images, self.all_nan_position = counts, len(counts), len(counts) - 1
        self.row_start = np.concatenate(([0], np.cumsum(counts))).astype(np.int64)
        self.n_rows = int(self.row_start[-1])
        self.row2image = np.repeat(np.arange(self.n_images), counts).astype(np.int32)
        w, h = rng.choice(SIDES, self.n_rows), rng.choice(SIDES, self.n_rows)
        x1, y1 = 16 * rng.integers(0, (400 - w) // 16 + 1), 16 * rng.integers(0, (624 - h) // 16 + 1)
        self.boxes = np.stack([x1, y1, x1 + w, y1 + h], axis=1).astype(np.float32)
        self.zoom = np.concatenate([np.asarray(LEVEL_SETS[(p + 2) % len(LEVEL_SETS)])[rng.integers(0, 99, T) % len(
            LEVEL_SETS[(p + 2) % len(LEVEL_SETS)])] for p, T in enumerate(counts)]).astype(np.int32)
        a = int(self.row_start[self.all_nan_position])
        self.boxes[a:, 2], self.boxes[a:, 3] = self.boxes[a:, 0], self.boxes[a:, 1]


class Shard:
    """one handle with tile meta, NQ_MAX queries, and per (query, aug, weight) what rescore_avg gives for every image"""

    def __init__(self, oracle, layout, dim, dtype):
        import torch
        from seesaw_amd.device_index import DeviceIndex
        self.torch, self.lay, self.dim = torch, layout, dim
        self.dev = torch.device("cuda", 0)
        X = oracle.synth_rows(4242 + dim, 0, layout.n_rows, dim)
        self.Q = np.stack([oracle.synth_query(900 + b, dim) for b in range(NQ_MAX)])
        if isinstance(layout, Layout):
            # column 0 carries the layout's planted scores (ties, the Kahan triple, the best tile past index 255), which
            # queries 0 .. 3 = c * e_0 read back exactly; the other queries see them among 255 random columns
            planted = layout.scores(np.float32)
            X[:, 0] = np.clip(planted, -60000.0, 60000.0) if dtype == "float16" else planted
            for b, c in enumerate((1.0, 2.0, 0.5, -1.0)):
                self.Q[b] = Layout.query(c)
        self.index = DeviceIndex.from_numpy(X, row2image=layout.row2image, device=0, dtype=dtype)
        self.index.set_tile_meta(layout.boxes, layout.zoom)
        self.index.set_stream(torch.cuda.current_stream(self.dev).cuda_stream)
        self.positions = np.arange(layout.n_images, dtype=np.int64)
        self.tile_scores, self.want = [], {}
        for b in range(NQ_MAX):  # computed once, shared by every test below
            self.tile_scores.append(self.index.scores(self.Q[b]))
            for aug in AUGS:
                for wgt in WEIGHTS:
                    self.want[b, aug, wgt] = self.index.rescore_avg(self.positions, aug, aug_weight=wgt)

    def keys_and_counts(self, nq, image_offset, seed):
        """per slot its own shuffled list: every image of the handle, the images just outside it and one far away,
        then repeats; arbitrary upper words; counts cycle through k, 0 and less than k"""
        rng = np.random.default_rng(seed)
        n = self.lay.n_images
        outside = [image_offset + n, 0xFFFFFFF0] + ([image_offset - 1] if image_offset > 0 else [])
        g = np.zeros((nq, K_MAX), dtype=np.int64)
        for b in range(nq):
            first = rng.permutation(np.concatenate([image_offset + self.positions, outside]))
            rest = image_offset + rng.integers(0, n, K_MAX - first.shape[0])
            g[b] = np.concatenate([first, rest])
        assert n + len(outside) <= K and ((g[:, :K] < image_offset) | (g[:, :K] >= image_offset + n)).any()
        upper = rng.integers(0, 2 ** 32, size=(nq, K_MAX), dtype=np.uint64) << np.uint64(32)
        keys = upper | (np.uint64(0xFFFFFFFF) - g.astype(np.uint64))
        counts = np.array([(K, 0, 7)[b % 3] for b in range(nq)], dtype=np.int32)
        return g, keys, counts

    def run(self, nq, aug, wgt, image_offset, row_offset, seed, k=K, k_max=K_MAX):
        torch = self.torch
        g, keys, counts = self.keys_and_counts(nq, image_offset, seed)
        d_keys = torch.from_numpy(keys.view(np.int64)).to(self.dev)
        d_counts = torch.from_numpy(counts).to(self.dev)
        d_out = torch.from_numpy(np.full((nq, 2, K_MAX), FILL, dtype=np.uint64).view(np.int64)).to(self.dev)
        self.index.stage2_avg_batch_dev(self.Q[:nq], d_keys.data_ptr(), d_counts.data_ptr(), k_max, k, aug, d_out.data_ptr(),
                                        image_offset=image_offset, row_offset=row_offset, aug_weight=wgt)
        torch.cuda.synchronize()
        return g, counts, d_out.cpu().numpy().view(np.uint64)

    def expected(self, nq, aug, wgt, g, counts, image_offset, row_offset, k=K):
        want = np.full((nq, 2, K_MAX), FILL, dtype=np.uint64)
        want[:, :, :k] = 0
        for b in range(nq):
            s, r = self.want[b, aug, wgt]
            for c in range(min(k, int(counts[b]))):
                p = int(g[b, c]) - image_offset
                if 0 <= p < self.lay.n_images:
                    want[b, 0, c] = OWNED | np.uint64(bits(s[p:p + 1])[0])
                    want[b, 1, c] = np.uint64(row_offset + int(r[p]))
        return want

    def close(self):
        self.index.close()


@pytest.fixture(scope="module", params=[("edges", 256, "float32"), ("edges", 256, "float16"),
                                        ("small", 512, "float32"), ("small", 512, "float16"),
                                        ("small", 768, "float32"), ("small", 768, "float16"),
                                        ("small", 1024, "float32"), ("small", 1024, "float16")],
                ids=lambda p: "-".join(str(v) for v in p))
def shard(request, oracle):
    which, dim, dtype = request.param
    s = Shard(oracle, Layout() if which == "edges" else SmallLayout(), dim, dtype)
    yield s
    s.close()


@pytest.mark.parametrize("nq", [1, 3, 16])
def test_the_block_is_rescore_avg_on_the_owned_and_zero_elsewhere(shard, nq):
    """every aug_larger and both aug_weights, the offsets alternating; entries c >= k keep the fill"""
    case = 0
    for aug in AUGS:
        for wgt in WEIGHTS:
            image_offset, row_offset = OFFSETS[(case + nq) % 2]
            g, counts, got = shard.run(nq, aug, wgt, image_offset, row_offset, seed=100 * nq + case)
            want = shard.expected(nq, aug, wgt, g, counts, image_offset, row_offset)
            assert np.array_equal(got, want), (nq, aug, wgt, image_offset, np.argwhere(got != want)[:5])
            assert (got[:, :, K:] == FILL).all()
            case += 1


def test_both_offsets_at_every_width_and_the_all_nan_image(shard):
    for nq in (1, 3, 16):
        for image_offset, row_offset in OFFSETS:
            g, counts, got = shard.run(nq, "greater", "level_max", image_offset, row_offset, seed=7 * nq + image_offset)
            assert np.array_equal(got, shard.expected(nq, "greater", "level_max", g, counts, image_offset, row_offset))
            b = 0  # counts[0] = K: the list holds every image of the handle, the all-NaN one among them
            c = int(np.flatnonzero(g[b, :K] == image_offset + shard.lay.all_nan_position)[0])
            assert got[b, 0, c] >> np.uint64(32) == np.uint64(1)
            assert np.isnan(np.uint32(got[b, 0, c] & np.uint64(0xFFFFFFFF)).view(np.float32))
            assert int(got[b, 1, c]) == row_offset + int(shard.lay.row_start[shard.lay.all_nan_position])


def test_level_max_equals_the_oracle_on_the_scans_scores(shard, oracle):
    lay = shard.lay
    for aug in AUGS:
        s, r = shard.want[0, aug, "level_max"]
        g, counts, got = shard.run(1, aug, "level_max", 0, 0, seed=5)
        for c in range(K):
            p = int(g[0, c])
            if not 0 <= p < lay.n_images:
                continue
            rows = slice(int(lay.row_start[p]), int(lay.row_start[p + 1]))
            best, sc, _ = oracle.avg_score_image(lay.boxes[rows], lay.zoom[rows], shard.tile_scores[0][rows], aug)
            assert np.uint32(got[0, 0, c] & np.uint64(0xFFFFFFFF)) == bits(np.float32(sc).reshape(1))[0], (aug, p)
            assert int(got[0, 1, c]) == rows.start + best, (aug, p)


def test_the_handle_is_left_as_it_was(shard):
    idx = shard.index
    all_rows = np.arange(shard.lay.n_rows, dtype=np.int64)
    idx.topk(shard.Q[5], 5, excluded=[1])
    before = (idx.gather_scores(all_rows), idx.topk(None, 5), idx.prune_stats(completions=True))
    shard.run(16, "all", "level_max", 1000, 7, seed=1)
    shard.run(3, "adjacent", "cont_weighted", 0, 0, seed=2)
    after = (idx.gather_scores(all_rows), idx.topk(None, 5), idx.prune_stats(completions=True))
    assert np.array_equal(bits(before[0]), bits(after[0]))
    assert all(np.array_equal(a, b) for a, b in zip(before[1], after[1]))
    assert before[2] == after[2]
    assert np.array_equal(bits(before[0]), bits(shard.tile_scores[5]))  # (and those were query 5's)


def test_more_queries_than_the_query_block_holds(shard):
    """nq = 19: the entry serves the block of 16 queries in parts"""
    torch, nq = shard.torch, 19
    Q = np.concatenate([shard.Q, shard.Q[:3][::-1]])
    g, keys, counts = shard.keys_and_counts(nq, 0, seed=3)
    d_keys = torch.from_numpy(keys.view(np.int64)).to(shard.dev)
    d_counts = torch.from_numpy(counts).to(shard.dev)
    d_out = torch.from_numpy(np.full((nq, 2, K_MAX), FILL, dtype=np.uint64).view(np.int64)).to(shard.dev)
    shard.index.stage2_avg_batch_dev(Q, d_keys.data_ptr(), d_counts.data_ptr(), K_MAX, K, "all", d_out.data_ptr())
    torch.cuda.synchronize()
    got = d_out.cpu().numpy().view(np.uint64)
    want = shard.expected(16, "all", "level_max", g[:16], counts[:16], 0, 0)
    assert np.array_equal(got[:16], want)
    for b, src in ((16, 2), (17, 1), (18, 0)):
        s, r = shard.want[src, "all", "level_max"]
        for c in range(min(K, int(counts[b]))):
            p = int(g[b, c])
            if 0 <= p < shard.lay.n_images:
                assert got[b, 0, c] == OWNED | np.uint64(bits(s[p:p + 1])[0]) and int(got[b, 1, c]) == int(r[p])
            else:
                assert got[b, 0, c] == 0 and got[b, 1, c] == 0


def test_refusals(shard, oracle):
    from seesaw_amd import _lib
    from seesaw_amd.device_index import DeviceIndex
    with pytest.raises(_lib.SeesawHipError) as e:
        shard.run(3, "all", "level_max", 0, 0, seed=1, k=K_MAX + 1)
    assert e.value.status == _lib.SSW_ERR_INVALID
    Qbad = shard.Q[:2].copy()
    Qbad[1, 3] = np.inf
    words = shard.torch.zeros(2 * 2 * K_MAX, dtype=shard.torch.int64, device=shard.dev)
    with pytest.raises(_lib.SeesawHipError) as e:
        shard.index.stage2_avg_batch_dev(Qbad, words.data_ptr(), words.data_ptr(), K_MAX, K, "all", words.data_ptr())
    assert e.value.status == _lib.SSW_ERR_NUMERIC
    bare = DeviceIndex.from_numpy(oracle.synth_rows(1, 0, 64, shard.dim), row2image=(np.arange(64) // 4).astype(np.int32), device=0)
    try:
        with pytest.raises(_lib.SeesawHipError) as e:
            bare.stage2_avg_batch_dev(shard.Q[:2], words.data_ptr(), words.data_ptr(), K_MAX, K, "all", words.data_ptr())
        assert e.value.status == _lib.SSW_ERR_INVALID and "set_tile_meta" in str(e.value)
    finally:
        bare.close()

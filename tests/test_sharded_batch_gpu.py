"""GPU: the batched top-k over the row-sharded index (ssw_index_set_exchange_target_batch, ssw_index_topk_batch_dev,
ssw_index_topk_slot_deep_dev, ssw_topk_merge_msgs_batch_dev; csrc/index_batch.hip, csrc/select.hip k_final in its grid
form).  One process: two handles over the two halves of one matrix play rank 0 and rank 1 (image_offset / row_offset set
accordingly), their message blocks are stacked by hand into the [world, nq, msg_len] layout one all-gather leaves, and
one merge launch follows.  The reference is always DeviceIndex.topk on a third handle over the whole matrix: images,
score BITS and best rows.  Every comparison is exact: the batched scan returns the bits of the single scan and the
selection is exact, so there is no tolerance to choose."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DIM = 512
HALF = 66_000        # rows per handle: the multi-query scan kernel serves >= 65 536
TILES = 3            # per image -> 22 000 images a handle (> 8192: the histogram selection)
K_MAX = 64
N_SLOTS = 19
NQ_MAX = 19


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def unit_queries(seed, nq, dim):
    rng = np.random.default_rng(seed)
    Q = rng.standard_normal((nq, dim)).astype(np.float32)
    return Q / np.linalg.norm(Q, axis=1, keepdims=True)


class TwoRanks:
    """rank 0 and rank 1 over the halves of one matrix, the reference over all of it; everything on torch's stream"""

    def __init__(self, make, n_half, imgs_half, rows_per_image, dim):
        import torch
        self.torch = torch
        self.dev = torch.device("cuda", 0)
        self.n_half, self.imgs_half, self.dim = n_half, imgs_half, dim
        self.ranks = [make(0), make(1)]
        self.ref = make(None)
        r2i = None if rows_per_image == 1 else (np.arange(n_half) // rows_per_image).astype(np.int32)
        if r2i is not None:
            for h in self.ranks:
                h.set_row2image(r2i)
            self.ref.set_row2image((np.arange(2 * n_half) // rows_per_image).astype(np.int32))
        stream = torch.cuda.current_stream(self.dev).cuda_stream
        for h in self.ranks:
            h.set_stream(stream)
        self.blocks = None

    def attach(self, n_slots, k_max, with_best):
        torch = self.torch
        self.n_slots, self.k_max, self.with_best = n_slots, k_max, with_best
        self.msg_len = (2 if with_best else 1) * k_max + 1
        self.blocks = [torch.full((n_slots, self.msg_len), -1, dtype=torch.int64, device=self.dev) for _ in range(2)]
        for r, h in enumerate(self.ranks):
            h.set_exchange_target_batch(self.blocks[r].data_ptr(), n_slots, k_max, with_best, r * self.imgs_half, r * self.n_half)

    def local_lists(self, excluded, r):
        lo = r * self.imgs_half
        return [[] if e is None else [int(i) - lo for i in e if lo <= int(i) < lo + self.imgs_half] for e in excluded]

    def select(self, Q, k, excluded, first_slot=0):
        for r, h in enumerate(self.ranks):
            h.topk_batch_dev(Q, k, excluded=None if excluded is None else self.local_lists(excluded, r), first_slot=first_slot)

    def merge(self, nq, k, flags_seen=None):
        """stack the two blocks as one all-gather of nq * msg_len words per rank would, merge in ONE launch"""
        torch = self.torch
        from seesaw_amd import _lib
        gathered = torch.stack([b[:nq] for b in self.blocks]).contiguous()  # [2, nq, msg_len]
        keys = torch.zeros((nq, self.k_max), dtype=torch.int64, device=self.dev)
        counts = torch.zeros(nq, dtype=torch.int32, device=self.dev)
        flags = torch.full((nq, 2), -1, dtype=torch.int64, device=self.dev)
        seen = torch.zeros(1, dtype=torch.int64, device=self.dev) if flags_seen is None else flags_seen
        _lib.call("ssw_topk_merge_msgs_batch_dev", 0, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream),
                  ctypes.c_void_p(gathered.data_ptr()), 2, nq * self.msg_len, nq, self.k_max, int(self.with_best), k,
                  ctypes.c_void_p(keys.data_ptr()), ctypes.c_void_p(counts.data_ptr()), ctypes.c_void_p(flags.data_ptr()),
                  ctypes.c_void_p(seen.data_ptr()))
        torch.cuda.synchronize()
        return keys.cpu().numpy().view(np.uint64), counts.cpu().numpy(), flags.cpu().numpy(), gathered.cpu().numpy(), seen

    def check_row(self, keys_row, count, gathered, b, want):
        """row b of a merge against the reference's (images, scores, rows)"""
        from seesaw_amd.device_index import decode_keys
        from seesaw_amd.sharded import unpack_message_block
        imgs, scores = decode_keys(keys_row[:count])
        assert np.array_equal(imgs, want[0]), b
        assert np.array_equal(bits(scores), bits(want[1])), b
        if self.with_best:
            lists = unpack_message_block(gathered, self.k_max, True)
            sent = {int(k_): int(row) for r in range(2) for k_, row in zip(lists[r][b][0], lists[r][b][1])}
            assert [sent[int(k_)] for k_ in keys_row[:count]] == want[2].tolist(), b

    def close(self):
        for h in self.ranks + [self.ref]:
            h.close()


def excluded_lists(ref, Q, n_images, seed):
    """a different list per query: every fourth empty, every fourth + 1 with repeats, the others 200 random images;
    all but the empty ones strike out the query's own five best, so that the exclusion decides the result"""
    rng = np.random.default_rng(seed)
    out = []
    for b in range(Q.shape[0]):
        top = ref.topk(Q[b], 5)[0].tolist()
        if b % 4 == 0:
            out.append(None)
        elif b % 4 == 1:
            out.append(top + top[:2] + [7, 7, n_images - 1, n_images - 1])
        else:
            out.append(top + rng.integers(0, n_images, size=200).tolist())
    return out


@pytest.fixture(scope="module", params=["float32", "float16"])
def big(request):
    """2 x 66 000 rows of dim 512, 3 tiles an image; the reference's top-K_MAX of every query, computed once"""
    from seesaw_amd.device_index import DeviceIndex
    dt = request.param

    def make(r):
        if r is None:
            return DeviceIndex.synthetic(2 * HALF, DIM, seed=11, first_row=0, device=0, dtype=dt)
        return DeviceIndex.synthetic(HALF, DIM, seed=11, first_row=r * HALF, device=0, dtype=dt)
    t = TwoRanks(make, HALF, HALF // TILES, TILES, DIM)
    t.Q = unit_queries(3, NQ_MAX, DIM)
    t.excluded = excluded_lists(t.ref, t.Q, 2 * (HALF // TILES), 4)
    t.want = [t.ref.topk(t.Q[b], K_MAX, excluded=t.excluded[b]) for b in range(NQ_MAX)]
    yield t
    t.close()


@pytest.mark.parametrize("with_best", [True, False])
@pytest.mark.parametrize("k", [10, K_MAX])
def test_batched_select_and_one_merge_equal_the_whole_index(big, k, with_best):
    """nq = 1, 2, 3, 16 and 19 (a remainder chunk and a second chunk) through the multi-query scan kernel and the
    histogram selection; the reference's top-k is the prefix of its top-K_MAX (the order is total)"""
    big.attach(N_SLOTS, K_MAX, with_best)
    for nq in (1, 2, 3, 16, 19):
        big.select(big.Q[:nq], k, big.excluded[:nq])
        keys, counts, flags, gathered, seen = big.merge(nq, k)
        assert counts.tolist() == [k] * nq and not flags.any() and int(seen.item()) == 0
        for b in range(nq):
            big.check_row(keys[b], k, gathered, b, tuple(a[:k] for a in big.want[b]))
    # the halves really are the halves of the reference's matrix
    assert np.array_equal(bits(big.ranks[1].download(5, 2)), bits(big.ref.download(HALF + 5, 2)))


def test_first_slot_fills_one_block_in_two_calls(big):
    big.attach(N_SLOTS, K_MAX, True)
    big.select(big.Q[:8], 10, big.excluded[:8], first_slot=0)
    big.select(big.Q[8:16], 10, big.excluded[8:16], first_slot=8)
    keys, counts, flags, gathered, _ = big.merge(16, 10)
    assert counts.tolist() == [10] * 16 and not flags.any()
    for b in range(16):
        big.check_row(keys[b], 10, gathered, b, tuple(a[:10] for a in big.want[b]))
    assert (big.blocks[0][16:].cpu().numpy() == -1).all()  # the slots nobody asked for were not written


@pytest.mark.parametrize("dim", [512, 256])
def test_below_the_multi_query_kernel(dim):
    """2 x 3000 rows, one tile an image: the one-launch selection and a single-scan launch per query; dim 256 is a dim
    the multi-query kernel never serves"""
    from seesaw_amd.device_index import DeviceIndex
    n = 3000

    def make(r):
        return DeviceIndex.synthetic(2 * n if r is None else n, dim, seed=5, first_row=0 if r is None else r * n, device=0)
    t = TwoRanks(make, n, n, 1, dim)
    try:
        Q = unit_queries(8, 3, dim)
        excluded = excluded_lists(t.ref, Q, 2 * n, 9)
        t.attach(4, 16, True)
        t.ranks[0].profile(True)
        t.select(Q, 10, excluded)
        assert t.ranks[0].profile_read().shape[0] == 3  # one event pair per scan launch: three single scans
        t.ranks[0].profile(False)
        keys, counts, flags, gathered, _ = t.merge(3, 10)
        assert counts.tolist() == [10] * 3 and not flags.any()
        for b in range(3):
            t.check_row(keys[b], 10, gathered, b, t.ref.topk(Q[b], 10, excluded=excluded[b]))
    finally:
        t.close()


def test_mass_ties_are_flagged_and_repaired_by_rescan():
    """rank 1 holds 9000 identical rows, more than the 8192 the final sort takes: every query's flag is set for that rank
    only, flags_seen is raised and stays; after topk_slot_deep_dev and a second merge the result is the reference's,
    which takes its deep path by itself"""
    import torch
    from seesaw_amd.device_index import DeviceIndex
    n, k, nq = 9000, 10, 3
    rng = np.random.default_rng(21)
    A = rng.standard_normal((n, DIM)).astype(np.float32)
    A /= np.linalg.norm(A, axis=1, keepdims=True)
    v = rng.standard_normal(DIM).astype(np.float32)
    v /= np.linalg.norm(v)
    B = np.repeat(v[None, :], n, axis=0)
    X = np.concatenate([A, B])

    def make(r):
        return DeviceIndex.from_numpy(X if r is None else (A, B)[r], device=0)
    t = TwoRanks(make, n, n, 1, DIM)
    try:
        Q = unit_queries(22, nq, DIM)
        Q[0] = v  # the tied rows are this query's best; for the others they rank wherever they fall
        excluded = [None, [3, n + 4, n + 4], [n, 5]]
        t.attach(4, 16, True)
        t.select(Q, k, excluded)
        seen = torch.zeros(1, dtype=torch.int64, device=t.dev)
        keys, counts, flags, gathered, seen = t.merge(nq, k, seen)
        assert flags.tolist() == [[0, 1]] * nq
        assert int(seen.item()) != 0
        for b in range(nq):
            t.ranks[1].topk_slot_deep_dev(Q[b], k, t.local_lists(excluded, 1)[b], b)
        keys, counts, flags, gathered, seen = t.merge(nq, k, seen)
        assert not flags.any() and int(seen.item()) != 0  # the OR over the exchanges stays set
        for b in range(nq):
            t.check_row(keys[b], int(counts[b]), gathered, b, t.ref.topk(Q[b], k, excluded=excluded[b]))
        assert counts.tolist() == [k] * nq
    finally:
        t.close()


# ---- the merge alone ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [1, 2, 8])
@pytest.mark.parametrize("nq", [1, 5])
def test_merge_rows_equal_the_single_merge(world, nq):
    """hand-built messages, one list of count 0, rank_stride > nq * msg_len with poison in the gap (all ones: as a key it
    would win every merge, as a count word it would overrun): row b is what ssw_topk_merge_msgs_dev makes of query b's
    `world` messages"""
    import torch
    from seesaw_amd import _lib
    from seesaw_amd.sharded import pack_message_block
    dev = torch.device("cuda", 0)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(100 * world + nq)
    for with_best, k_max, k in ((True, 16, 10), (False, 16, 16)):
        msg_len = (2 if with_best else 1) * k_max + 1
        lists = []
        for r in range(world):
            row = []
            for b in range(nq):
                c = 0 if (r, b) == (world - 1, nq - 1) else int(rng.integers(1, k_max + 1))
                keys = np.sort(np.unique(rng.integers(1, 2 ** 62, size=c, dtype=np.int64)).astype(np.uint64))[::-1]
                row.append((keys, rng.integers(0, 2 ** 40, size=keys.shape[0], dtype=np.int64), int(rng.integers(0, 2))))
            lists.append(row)
        block = pack_message_block(lists, k_max, with_best)
        stride = nq * msg_len + 37
        padded = np.full((world, stride), np.uint64(0xFFFFFFFFFFFFFFFF), dtype=np.uint64)
        padded[:, :nq * msg_len] = block.reshape(world, -1)
        msgs = torch.from_numpy(padded.view(np.int64)).to(dev)
        keys = torch.zeros((nq, k_max), dtype=torch.int64, device=dev)
        counts = torch.full((nq,), -1, dtype=torch.int32, device=dev)
        flags = torch.full((nq, world), -1, dtype=torch.int64, device=dev)
        seen = torch.zeros(1, dtype=torch.int64, device=dev)
        _lib.call("ssw_topk_merge_msgs_batch_dev", 0, stream, ctypes.c_void_p(msgs.data_ptr()), world, stride, nq, k_max,
                  int(with_best), k, ctypes.c_void_p(keys.data_ptr()), ctypes.c_void_p(counts.data_ptr()),
                  ctypes.c_void_p(flags.data_ptr()), ctypes.c_void_p(seen.data_ptr()))
        any_flag = 0
        for b in range(nq):
            one = torch.from_numpy(np.ascontiguousarray(block[:, b]).view(np.int64)).to(dev)  # [world, msg_len]
            k1 = torch.zeros(k_max, dtype=torch.int64, device=dev)
            c1 = torch.full((1,), -1, dtype=torch.int32, device=dev)
            f1 = torch.full((world,), -1, dtype=torch.int64, device=dev)
            s1 = torch.zeros(1, dtype=torch.int64, device=dev)
            _lib.call("ssw_topk_merge_msgs_dev", 0, stream, ctypes.c_void_p(one.data_ptr()), world, k_max, int(with_best), k,
                      ctypes.c_void_p(k1.data_ptr()), ctypes.c_void_p(c1.data_ptr()), ctypes.c_void_p(f1.data_ptr()),
                      ctypes.c_void_p(s1.data_ptr()))
            torch.cuda.synchronize()
            c = int(c1.item())
            assert int(counts[b].item()) == c == min(k, sum(len(lists[r][b][0]) for r in range(world))), b
            assert torch.equal(keys[b, :c], k1[:c]), b
            assert torch.equal(flags[b], f1) and f1.tolist() == [lists[r][b][2] for r in range(world)], b
            any_flag |= int(s1.item())
        assert int(seen.item()) == any_flag


# ---- refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_slots_alone(big):
    import torch
    from seesaw_amd import _lib
    from seesaw_amd.device_index import DeviceIndex
    big.attach(N_SLOTS, K_MAX, True)
    a = big.ranks[0]
    before = big.blocks[0].clone()

    def refused(status, text, call):
        with pytest.raises(_lib.SeesawHipError) as e:
            call()
        assert e.value.status == status and text in str(e.value), str(e.value)
        torch.cuda.synchronize()
        assert torch.equal(big.blocks[0], before)

    Q = big.Q[:4].copy()
    refused(_lib.SSW_ERR_INVALID, "k_max", lambda: a.topk_batch_dev(Q, K_MAX + 1))
    refused(_lib.SSW_ERR_INVALID, "slots", lambda: a.topk_batch_dev(Q, 10, first_slot=N_SLOTS - 3))
    refused(_lib.SSW_ERR_INVALID, "slots", lambda: a.topk_batch_dev(Q, 10, first_slot=-1))
    refused(_lib.SSW_ERR_INVALID, "slots", lambda: a.topk_slot_deep_dev(Q[0], 10, None, N_SLOTS))
    bad = Q.copy()
    bad[2, 17] = np.nan
    refused(_lib.SSW_ERR_NUMERIC, "query 2", lambda: a.topk_batch_dev(bad, 10))
    ids = np.array([1, 2, 3], dtype=np.int64)
    offsets = np.array([0, 2, 1, 3, 3], dtype=np.int64)
    refused(_lib.SSW_ERR_INVALID, "decrease",
            lambda: _lib.call("ssw_index_topk_batch_dev", a._h, Q.ctypes.data, 4, ids.ctypes.data, offsets.ctypes.data, 10, 0))
    refused(_lib.SSW_ERR_INVALID, "outside", lambda: a.topk_batch_dev(Q, 10, excluded=[[HALF], None, None, None]))
    a.set_exchange_target_batch(0, 0, 0, False)  # detached
    refused(_lib.SSW_ERR_INVALID, "no batch exchange target", lambda: a.topk_batch_dev(Q, 10))
    refused(_lib.SSW_ERR_INVALID, "no batch exchange target", lambda: a.topk_slot_deep_dev(Q[0], 10, None, 0))
    for n_slots, k_max in ((0, 16), (4, 0), (4, _lib.SSW_MAX_TOPK + 1)):
        with pytest.raises(_lib.SeesawHipError) as e:
            a.set_exchange_target_batch(big.blocks[0].data_ptr(), n_slots, k_max, True)
        assert e.value.status == _lib.SSW_ERR_INVALID
    # the merge: world * k beyond the 8192 candidates one workgroup sorts, a stride shorter than the chunk, nq = 0
    dev = big.dev
    k_max = 4096
    msgs = torch.zeros(3 * 2 * (2 * k_max + 1), dtype=torch.int64, device=dev)
    keys = torch.full((2, k_max), -1, dtype=torch.int64, device=dev)
    counts = torch.full((2,), -1, dtype=torch.int32, device=dev)

    def merge(world, stride, nq, k):
        _lib.call("ssw_topk_merge_msgs_batch_dev", 0, None, ctypes.c_void_p(msgs.data_ptr()), world, stride, nq, k_max, 1, k,
                  ctypes.c_void_p(keys.data_ptr()), ctypes.c_void_p(counts.data_ptr()), None, None)
    for args, text in (((3, 2 * (2 * k_max + 1), 2, 4096), "exceed 8192"), ((2, 2 * (2 * k_max + 1) - 1, 2, 10), "stride"),
                       ((2, 2 * (2 * k_max + 1), 0, 10), "nq=0"), ((2, 2 * (2 * k_max + 1), 2, k_max + 1), "k=")):
        with pytest.raises(_lib.SeesawHipError) as e:
            merge(*args)
        assert e.value.status == _lib.SSW_ERR_INVALID and text in str(e.value), str(e.value)
    torch.cuda.synchronize()
    assert (keys == -1).all() and (counts == -1).all()
    # an index without a target of either kind is refused too
    bare = DeviceIndex.synthetic(1000, DIM, seed=1, device=0)
    try:
        with pytest.raises(_lib.SeesawHipError) as e:
            bare.topk_batch_dev(Q, 10)
        assert e.value.status == _lib.SSW_ERR_INVALID and "no batch exchange target" in str(e.value)
    finally:
        bare.close()


# ---- neighbours untouched ----------------------------------------------------------------------------------------------
def test_the_single_target_and_the_handle_state_are_untouched(big):
    """with both targets attached a batched call leaves the single send_buf bit-identical; a following topk_dev +
    exchange_fused gives what it gives on a fresh handle; topk(None, k) ranks the last query; prune_stats is unchanged"""
    import torch
    from seesaw_amd.device_index import DeviceIndex
    from seesaw_amd.sharded import ShardedTopK
    a = big.ranks[0]
    fresh = DeviceIndex.synthetic(HALF, DIM, seed=11, first_row=0, device=0, dtype=big.ref.dtype)
    fresh.set_row2image((np.arange(HALF) // TILES).astype(np.int32))
    fresh.set_stream(torch.cuda.current_stream(big.dev).cuda_stream)
    try:
        k = 10
        xa = ShardedTopK(rank=0, world=1, device=big.dev, image_offset=0, k_max=K_MAX, with_best=True).attach(a)
        xa.attach_batch(a, N_SLOTS)
        xf = ShardedTopK(rank=0, world=1, device=big.dev, image_offset=0, k_max=K_MAX, with_best=True).attach(fresh)
        q0 = torch.from_numpy(big.Q[0]).to(big.dev)
        a.set_excluded(None)
        a.topk_dev(q0.data_ptr(), k)
        torch.cuda.synchronize()
        sent = xa.send_buf.clone()
        stats = a.prune_stats()
        local = big.local_lists(big.excluded[:5], 0)
        a.topk_batch_dev(big.Q[:5], k, excluded=local)
        keys_b, counts_b = xa.exchange_fused_batch(5, k)
        torch.cuda.synchronize()
        assert torch.equal(xa.send_buf, sent)
        assert a.prune_stats() == stats
        assert xa.overflowed_batch() == []
        # world 1: the merged row is the shard's own top-k
        for b in range(5):
            want = fresh.topk(big.Q[b], k, excluded=local[b])
            from seesaw_amd.device_index import decode_keys
            imgs, scores = decode_keys(keys_b[b, :int(counts_b[b].item())].cpu().numpy().view(np.uint64))
            assert np.array_equal(imgs, want[0]) and np.array_equal(bits(scores), bits(want[1]))
            assert np.array_equal(xa.best_rows_of(keys_b[b, :k].cpu().numpy().view(np.uint64), query=b), want[2])
        # the handle is left as after topk_dev of the last query with its list
        want = fresh.topk(big.Q[4], k, excluded=local[4])
        got = a.topk(None, k, excluded=local[4])
        assert all(np.array_equal(x, y) for x, y in zip(got[:1] + got[2:], want[:1] + want[2:]))
        assert np.array_equal(bits(got[1]), bits(want[1]))
        # the single path afterwards: what a fresh handle gives
        for h in (a, fresh):
            h.set_excluded(local[2])
            h.topk_dev(q0.data_ptr(), k)
        ka, ca = xa.exchange_fused(k)
        kf, cf = xf.exchange_fused(k)
        torch.cuda.synchronize()
        assert torch.equal(xa.send_buf, xf.send_buf) and torch.equal(ka[:k], kf[:k]) and int(ca.item()) == int(cf.item()) == k
        a.set_exchange_target_batch(0, 0, 0, False)
        from seesaw_amd import _lib
        _lib.call("ssw_index_set_exchange_target", a._h, None, 0, 0, 0, 0)
    finally:
        fresh.close()


def test_sharded_synthetic_index_topk_batch_equals_the_single_calls():
    """world 1 without a collective: two groups of n_slots = 4 queries and a remainder of one"""
    import torch
    from seesaw_amd.sharded import ShardedSyntheticIndex
    idx = ShardedSyntheticIndex(70_000, DIM, seed=9, rank=0, world=1, local_device=0, k_max=32, force_collective=False,
                                n_slots=4)
    try:
        Q = unit_queries(10, 9, DIM)
        got = idx.topk_batch(Q, 10)
        keys, counts = idx.topk_batch_async(Q[:3], 10)
        torch.cuda.synchronize()
        idx.xchg.assert_no_overflow_seen()
        assert counts.tolist() == [10, 10, 10]
        with pytest.raises(ValueError):
            idx.topk_batch_async(Q[:5], 10)
        assert len(got) == 9
        for b in range(9):
            qd = torch.from_numpy(Q[b]).to(idx.device)
            imgs, scores = idx.topk(qd.data_ptr(), 10)
            assert np.array_equal(got[b][0], imgs) and np.array_equal(bits(got[b][1]), bits(scores)), b
    finally:
        idx.close()

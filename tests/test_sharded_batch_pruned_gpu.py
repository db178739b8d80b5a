"""GPU: the pruned sharded batch (ssw_index_topk_batch_dev_pruned, ssw_index_prune_batch_dev_read; csrc/index_batch.hip,
csrc/rescore_dev.hip), on the lab build with the pruning threshold at one row.  One process: two handles over the halves
of one matrix play rank 0 and rank 1, their message blocks are stacked by hand as one all-gather would leave them and
one merge launch follows (the arrangement of tests/test_sharded_batch_gpu.py).  The reference is always DeviceIndex.topk
on a third handle over the whole matrix with the pruning OFF: images, score BITS and best rows.  Every comparison is
exact: the path is exact, so there is no tolerance to choose.  A (query, rank) whose certificate failed must carry the
flag value 2 and be right after ssw_index_topk_slot_deep_dev and one more merge; the queries beside it must be right
before."""
import ctypes

import numpy as np
import pytest

from _prune_batch_helpers import flagged_queries
from _prune_helpers import mode

pytestmark = pytest.mark.gpu

K_MAX = 64
N_SLOTS = 19
NQ_MAX = 19
NQS = (1, 2, 3, 16, 19)  # one chunk of 16 and a remainder of 3; remainders of 1 and 2
KS = (1, 10, 64)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def unit_queries(seed, nq, dim):
    rng = np.random.default_rng(seed)
    Q = rng.standard_normal((nq, dim)).astype(np.float32)
    return Q / np.linalg.norm(Q, axis=1, keepdims=True)


def unpruned(fn):
    """fn() with the pruning off (the reference), the lab threshold of one row afterwards"""
    mode(None, False)
    try:
        return fn()
    finally:
        mode(None, True, 1)


class TwoRanks:
    """rank 0 and rank 1 over the halves of one matrix, the reference over all of it; everything on torch's stream"""

    def __init__(self, make, n_half, imgs_half, rows_per_image, dim):
        import torch
        self.torch = torch
        self.dev = torch.device("cuda", 0)
        self.n_half, self.imgs_half, self.dim, self.tiles = n_half, imgs_half, dim, rows_per_image
        self.ranks = [make(0), make(1)]
        self.ref = make(None)
        if rows_per_image != 1:
            for h in self.ranks:
                h.set_row2image(self.r2i())
            self.ref.set_row2image((np.arange(2 * n_half) // rows_per_image).astype(np.int32))
        self.stream = torch.cuda.current_stream(self.dev).cuda_stream
        for h in self.ranks:
            h.set_stream(self.stream)
        self.blocks = None

    def r2i(self):
        return (np.arange(self.n_half) // self.tiles).astype(np.int32)

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

    def select(self, Q, k, excluded, first_slot=0, prune=True):
        for r, h in enumerate(self.ranks):
            h.topk_batch_dev(Q, k, excluded=None if excluded is None else self.local_lists(excluded, r), first_slot=first_slot,
                             prune=prune)

    def merge(self, nq, k, first_slot=0):
        """stack the two blocks as one all-gather of nq * msg_len words per rank would, merge in ONE launch"""
        torch = self.torch
        from seesaw_amd import _lib
        gathered = torch.stack([b[first_slot:first_slot + nq] for b in self.blocks]).contiguous()  # [2, nq, msg_len]
        keys = torch.zeros((nq, self.k_max), dtype=torch.int64, device=self.dev)
        counts = torch.zeros(nq, dtype=torch.int32, device=self.dev)
        flags = torch.full((nq, 2), -1, dtype=torch.int64, device=self.dev)
        seen = torch.zeros(1, dtype=torch.int64, device=self.dev)
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
        assert np.array_equal(imgs, want[0]), (b, imgs[:8], want[0][:8])
        assert np.array_equal(bits(scores), bits(want[1])), b
        if self.with_best:
            lists = unpack_message_block(gathered, self.k_max, True)
            sent = {int(k_): int(row) for r in range(2) for k_, row in zip(lists[r][b][0], lists[r][b][1])}
            assert [sent[int(k_)] for k_ in keys_row[:count]] == want[2].tolist(), b

    def available(self, excluded, r):
        """images of rank r each query may still select"""
        return [self.imgs_half - len(set(l)) for l in self.local_lists(excluded, r)]

    def run(self, Q, k, excluded, want, expect_flags, first_slot=0):
        """one pruned call per rank and one merge; the flags must be `expect_flags` [nq, 2] exactly; the unflagged
        queries must be right at once, the flagged ones after their repair and ONE more merge.  -> the device's counts
        of the last chunk, per rank, read before the repair"""
        nq = Q.shape[0]
        excluded = [None] * nq if excluded is None else excluded
        self.select(Q, k, excluded, first_slot)
        keys, counts, flags, gathered, seen = self.merge(nq, k, first_slot)
        read = [h.prune_batch_dev_counts() for h in self.ranks]
        assert flags.tolist() == np.asarray(expect_flags).tolist(), flags.tolist()
        assert int(seen.item()) == int(np.bitwise_or.reduce(np.asarray(expect_flags).reshape(-1)))
        for b in range(nq):
            if not flags[b].any():
                self.check_row(keys[b], int(counts[b]), gathered, b, want[b])
        if flags.any():
            for b, r in zip(*np.nonzero(flags)):
                self.ranks[r].topk_slot_deep_dev(Q[b], k, self.local_lists(excluded, r)[b], first_slot + int(b))
            keys, counts, flags, gathered, _ = self.merge(nq, k, first_slot)
            assert not flags.any()
            for b in range(nq):
                self.check_row(keys[b], int(counts[b]), gathered, b, want[b])
        return read

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
            out.append(top + top[:2] + [min(7, n_images - 1)] * 2 + [n_images - 1, n_images - 1])
        else:
            out.append(top + rng.integers(0, n_images, size=200).tolist())
    return out


def flags_for(t, excluded, k, nq):
    """Gaussian rows at the default cap: a (query, rank) fails its certificate exactly where the rank has fewer than k
    images left to select (the threshold selection then has no k-th key)"""
    excluded = [None] * nq if excluded is None else excluded
    av = [t.available(excluded, r) for r in range(2)]
    return [[2 if av[r][b] < k else 0 for r in range(2)] for b in range(nq)]


@pytest.fixture(scope="module")
def lab():
    """the lab build for the whole module, every index pruned from one row on; the product's switches afterwards"""
    from seesaw_amd import _lib
    with _lib.debug_hooks() as lib:
        try:
            mode(lib, True, 1)
            yield lib
        finally:
            _lib.call("ssw_tune_surv_cap", 0)
            mode(lib, True)


def from_matrix(X, dtype, tiles=1):
    from seesaw_amd.device_index import DeviceIndex
    n = X.shape[0] // 2

    def make(r):
        return DeviceIndex.from_numpy(X if r is None else X[r * n:(r + 1) * n], device=0, dtype=dtype)
    return TwoRanks(make, n, n // tiles, tiles, X.shape[1])


def gaussian(n, dim, seed):
    X = np.random.default_rng(seed).standard_normal((n, dim)).astype(np.float32)
    return X / np.linalg.norm(X, axis=1, keepdims=True)


def prepare(t, seed, k_want=K_MAX):
    """queries, exclusion lists and the reference's answers (pruning off), computed once per arrangement"""
    t.Q = unit_queries(seed, NQ_MAX, t.dim)
    n_images = 2 * t.imgs_half
    t.excluded = unpruned(lambda: excluded_lists(t.ref, t.Q, n_images, seed + 1))
    t.want = unpruned(lambda: [t.ref.topk(t.Q[b], k_want, excluded=t.excluded[b]) for b in range(NQ_MAX)])
    return t


def prefix(want, k):
    return [tuple(a[:k] for a in w) for w in want]  # the order is total: the top-k is the prefix of the top-K_MAX


# ---- results ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["float32", "float16"])
def big(request, lab):
    """2 x 66 000 rows of dim 512, 3 tiles an image: 22 000 images a handle, the histogram selection"""
    from seesaw_amd.device_index import DeviceIndex
    dt, half = request.param, 66_000

    def make(r):
        if r is None:
            return DeviceIndex.synthetic(2 * half, 512, seed=11, first_row=0, device=0, dtype=dt)
        return DeviceIndex.synthetic(half, 512, seed=11, first_row=r * half, device=0, dtype=dt)
    t = prepare(TwoRanks(make, half, half // 3, 3, 512), 3)
    yield t
    t.close()


@pytest.mark.parametrize("with_best", [True, False])
def test_histogram_selection_all_widths_and_k(big, with_best):
    t = big
    t.attach(N_SLOTS, K_MAX, with_best)
    for k in KS:
        for nq in NQS:
            read = t.run(t.Q[:nq], k, t.excluded[:nq], prefix(t.want, k), np.zeros((nq, 2), np.int64))
            for surv, why in read:  # the last chunk of each rank: nobody failed, and k images need k rows at least
                assert surv.shape[0] == (nq - 1) % 16 + 1 and not why.any() and (surv >= k).all(), (k, nq, surv, why)


def test_first_slot_leaves_the_other_slots_alone(big):
    t = big
    t.attach(N_SLOTS, K_MAX, True)
    t.run(t.Q[5:8], 10, t.excluded[5:8], prefix(t.want, 10)[5:8], np.zeros((3, 2), np.int64), first_slot=9)
    for blk in t.blocks:
        b = blk.cpu().numpy()
        assert (b[:9] == -1).all() and (b[12:] == -1).all()
    t.run(t.Q[:9], 10, t.excluded[:9], prefix(t.want, 10)[:9], np.zeros((9, 2), np.int64), first_slot=0)
    keys, counts, flags, gathered, _ = t.merge(3, 10, first_slot=9)  # the earlier call's slots are still what they were
    for b in range(3):
        t.check_row(keys[b], 10, gathered, b, prefix(t.want, 10)[5 + b])


def test_counts_equal_the_host_waiting_batch(big):
    """the survivors the device counted are those ssw_index_topk_batch_pruned publishes for the same chunk: its
    last_survivors is the last slot's"""
    from seesaw_amd.device_index import DeviceIndex
    t = big
    t.attach(N_SLOTS, K_MAX, True)
    fresh = DeviceIndex.synthetic(t.n_half, 512, seed=11, first_row=0, device=0, dtype=t.ref.dtype)
    try:
        fresh.set_row2image(t.r2i())
        for nq in (1, 3, 19):
            local = t.local_lists(t.excluded[:nq], 0)
            before = t.ranks[0].prune_stats()
            t.ranks[0].topk_batch_dev(t.Q[:nq], 10, excluded=local, prune=True)
            surv, why = t.ranks[0].prune_batch_dev_counts()
            after = t.ranks[0].prune_stats()
            assert after["queries"] == before["queries"] + nq
            assert (after["last_survivors"], after["fallbacks"]) == (before["last_survivors"], before["fallbacks"])
            fresh.topk_batch(t.Q[:nq], 10, excluded=local, prune=True)
            assert fresh.prune_stats()["last_survivors"] == int(surv[-1]) and not why.any()
    finally:
        fresh.close()


@pytest.mark.parametrize("dtype", ["float32", "float16"])
@pytest.mark.parametrize("n_half", [1, 17])
def test_tiny_shards(lab, n_half, dtype):
    """1 and 17 rows a handle: a rank that cannot give k images fails its certificate, is flagged and repaired"""
    t = prepare(from_matrix(gaussian(2 * n_half, 512, 40 + n_half), dtype), 41)
    try:
        t.attach(N_SLOTS, K_MAX, True)
        for k in KS:
            for nq in NQS:
                t.run(t.Q[:nq], k, t.excluded[:nq], prefix(t.want, k), flags_for(t, t.excluded[:nq], k, nq))
    finally:
        t.close()


@pytest.mark.parametrize("dtype", ["float32", "float16"])
@pytest.mark.parametrize("dim", [256, 512, 1024])
def test_4099_rows_every_dim(lab, dim, dtype):
    t = prepare(from_matrix(gaussian(2 * 4099, dim, 50 + dim), dtype), 51)
    try:
        t.attach(N_SLOTS, K_MAX, True)
        for k in KS:
            for nq in NQS:
                read = t.run(t.Q[:nq], k, t.excluded[:nq], prefix(t.want, k), np.zeros((nq, 2), np.int64))
                for surv, why in read:
                    assert not why.any() and (surv >= k).all()
    finally:
        t.close()


# ---- every failure reason, repaired ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mid(lab):
    t = prepare(from_matrix(gaussian(2 * 4099, 512, 60), "float32"), 61)
    t.attach(N_SLOTS, K_MAX, True)
    yield t
    t.close()


def test_over_the_cap_is_flagged_and_repaired(mid):
    from seesaw_amd import _lib
    t, k, nq = mid, 10, 3
    # the precondition, read from the device: at the default cap every slot is certified with more than 8 survivors
    t.select(t.Q[:nq], k, t.excluded[:nq])
    for h in t.ranks:
        surv, why = h.prune_batch_dev_counts()
        assert (surv > 8).all() and not why.any(), (surv, why)
    _lib.call("ssw_tune_surv_cap", 8)
    try:
        read = t.run(t.Q[:nq], k, t.excluded[:nq], prefix(t.want, k), np.full((nq, 2), 2, np.int64))
        for surv, why in read:
            assert (surv > 8).all() and (why == 4).all(), (surv, why)
    finally:
        _lib.call("ssw_tune_surv_cap", 0)
    t.run(t.Q[:nq], k, t.excluded[:nq], prefix(t.want, k), np.zeros((nq, 2), np.int64))  # the product's cap again


def test_an_unboundable_query_is_flagged_and_repaired(mid):
    t, k = mid, 10
    Q = t.Q[:3].copy()
    Q[1] = flagged_queries(512)[3]  # finite, norm above 2^40
    assert np.isfinite(Q).all()
    want = prefix(t.want, k)[:3]
    want[1] = unpruned(lambda: t.ref.topk(Q[1], k, excluded=t.excluded[1]))
    read = t.run(Q, k, t.excluded[:3], want, [[0, 0], [2, 2], [0, 0]])
    for surv, why in read:
        assert why.tolist() == [0, 2, 0]


def test_too_few_images_on_one_rank_is_flagged_and_repaired(mid):
    t, k = mid, 10
    excluded = list(t.excluded[:3])
    excluded[2] = list(range(5, t.imgs_half))  # rank 0 keeps images 0 .. 4 for this query, rank 1 all of its own
    want = prefix(t.want, k)[:3]
    want[2] = unpruned(lambda: t.ref.topk(t.Q[2], k, excluded=excluded[2]))
    read = t.run(t.Q[:3], k, excluded, want, [[0, 0], [0, 0], [2, 0]])
    assert read[0][1].tolist() == [0, 0, 1] and read[1][1].tolist() == [0, 0, 0]


def test_mass_ties_need_no_special_case(lab):
    """all rows equal: whichever bit is raised -- the selection's overflow, the failed certificate, both or none -- the
    repaired result is the reference's"""
    n, k, nq = 9000, 10, 3
    v = unit_queries(70, 1, 512)[0]
    t = from_matrix(np.repeat(v[None, :], 2 * n, axis=0), "float32")
    try:
        Q = unit_queries(71, nq, 512)
        Q[0] = v
        excluded = [None, [3, n + 4, n + 4], [n, 5]]
        want = unpruned(lambda: [t.ref.topk(Q[b], k, excluded=excluded[b]) for b in range(nq)])
        t.attach(4, 16, True)
        t.select(Q, k, excluded)
        keys, counts, flags, gathered, _ = t.merge(nq, k)
        assert ((flags >= 0) & (flags <= 3)).all()
        for b, r in zip(*np.nonzero(flags)):
            t.ranks[r].topk_slot_deep_dev(Q[b], k, t.local_lists(excluded, r)[b], int(b))
        keys, counts, flags, gathered, _ = t.merge(nq, k)
        assert not flags.any() and counts.tolist() == [k] * nq
        for b in range(nq):
            t.check_row(keys[b], k, gathered, b, want[b])
    finally:
        t.close()


def test_a_non_finite_query_is_refused_like_the_plain_entry(mid):
    from seesaw_amd import _lib
    t = mid
    bad = t.Q[:4].copy()
    bad[2, 17] = np.nan
    before = t.blocks[0].clone()
    errors = []
    for prune in (False, True):
        with pytest.raises(_lib.SeesawHipError) as e:
            t.ranks[0].topk_batch_dev(bad, 10, prune=prune)
        assert e.value.status == _lib.SSW_ERR_NUMERIC and "query 2" in str(e.value)
        errors.append(str(e.value))
    assert errors[0] == errors[1]
    t.torch.cuda.synchronize()
    assert t.torch.equal(t.blocks[0], before)
    with pytest.raises(_lib.SeesawHipError) as e:
        t.ranks[0].topk_batch_dev(t.Q[:4], 10, first_slot=N_SLOTS - 3, prune=True)
    assert e.value.status == _lib.SSW_ERR_INVALID and "slots" in str(e.value)


# ---- state -----------------------------------------------------------------------------------------------------------
def test_the_handle_reads_as_after_the_plain_entry(lab):
    """after the call topk(None, k), gather_scores and rescore_avg return what they return after topk_batch_dev without
    pruning: the buffer is partial with the last query kept, and the readers' completion rule does the rest"""
    import torch
    from seesaw_amd.device_index import DeviceIndex
    n, tiles, k, nq = 4096, 4, 10, 5
    X = gaussian(n, 512, 80)
    dev = torch.device("cuda", 0)
    boxes = np.tile(np.array([[0, 0, 1, 1], [0, 0, .5, .5], [.5, 0, 1, .5], [0, .5, .5, 1]], np.float32), (n // 4, 1))
    zoom = np.tile(np.array([0, 1, 1, 1], np.int32), n // 4)
    Q = unit_queries(81, nq, 512)
    excluded = [None, [1, 2], None, [7], [3, 3, 900]]
    rows = np.array([0, 5, n - 1, 77, 77], dtype=np.int64)
    pos = np.arange(0, n // tiles, 7)

    def readers(prune):
        out = []
        for reader in range(3):  # a fresh call before each reader: every one meets the state the entry leaves
            h = DeviceIndex.from_numpy(X, row2image=(np.arange(n) // tiles).astype(np.int32), device=0)
            try:
                h.set_tile_meta(boxes, zoom)
                block = torch.full((8, 2 * 16 + 1), -1, dtype=torch.int64, device=dev)
                h.set_exchange_target_batch(block.data_ptr(), 8, 16, True)
                h.topk_batch_dev(Q, k, excluded=excluded, prune=prune)
                if reader == 0:
                    out.append(h.topk(None, k, excluded=excluded[-1]))
                elif reader == 1:
                    out.append((h.gather_scores(rows),))
                else:
                    out.append(h.rescore_avg(pos, "greater"))
                out.append((block.cpu().numpy(),))
                if prune:
                    surv, why = h.prune_batch_dev_counts()
                    assert surv.shape[0] == nq and not why.any()
            finally:
                h.close()
        return out
    plain, pruned = unpruned(lambda: readers(False)), readers(True)
    for a, b in zip(plain, pruned):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            assert x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8))


@pytest.mark.parametrize("why", ["dim 768", "threshold above n"])
def test_an_ineligible_index_takes_the_plain_entry(lab, why):
    import torch
    from seesaw_amd.device_index import DeviceIndex
    dim = 768 if why == "dim 768" else 512
    n, k, nq = 3000, 10, 5
    dev = torch.device("cuda", 0)
    Q = unit_queries(90, nq, dim)
    excluded = [None, [1, 2], None, [7], [3, 3, 900]]
    if why != "dim 768":
        mode(lab, True, n + 1)
    try:
        blocks = []
        for prune in (False, True):
            h = DeviceIndex.synthetic(n, dim, seed=91, device=0)
            try:
                block = torch.full((8, 2 * 16 + 1), -1, dtype=torch.int64, device=dev)
                h.set_exchange_target_batch(block.data_ptr(), 8, 16, True)
                h.topk_batch_dev(Q, k, excluded=excluded, prune=prune)
                h.sync()
                blocks.append(block.cpu().numpy())
                st = h.prune_stats()
                assert st["queries"] == 0 and st["shadow"] == "none"
                assert h.prune_batch_dev_counts()[0].shape[0] == 0
            finally:
                h.close()
        assert np.array_equal(blocks[0], blocks[1]) and (blocks[0][:nq, -1] == k).all()
    finally:
        mode(lab, True, 1)

"""GPU: k_rescore_survivors alone (csrc/rescore_dev.hip), through the lab hook ssw_debug_rescore_survivors: chosen
survivor lists, counts and state words for a chunk of 1, 3 and 16 slots; the slabs come back pre-filled with a sentinel.
Listed rows must hold the BITS of DeviceIndex.scores(q) -- the scan's summation order -- and every other row the
sentinel; a slot whose state says "failed" (either bit, or a count above the cap) must be left untouched while its
neighbours are written.  Every slot has its own query (norms 2^24 apart) and its own list, so a kernel that read a
neighbour's query or list fails every case here.  No tolerance anywhere: the path is exact."""
import ctypes

import numpy as np
import pytest

from _prune_helpers import adversarial_rows

pytestmark = pytest.mark.gpu

N = 4099
SENTINEL = np.uint32(0x7FC0BEEF)
SURV_CAP = 1 << 18


def hook(idx, Q, lists, counts, fail_bits=None):
    """-> (slabs u32 [nq, n], waves a slot); lists[j] holds min(counts[j], cap) rows"""
    from seesaw_amd import _lib
    Q = np.ascontiguousarray(Q, dtype=np.float32)
    nq = Q.shape[0]
    rows = np.ascontiguousarray(np.concatenate([np.asarray(l, dtype=np.int64) for l in lists] + [np.zeros(0, np.int64)]))
    cnt = np.ascontiguousarray(counts, dtype=np.int64)
    bits = np.zeros(nq, dtype=np.int32) if fail_bits is None else np.ascontiguousarray(fail_bits, dtype=np.int32)
    out = np.empty((nq, idx.n_rows), dtype=np.float32)
    waves = ctypes.c_int32(0)
    _lib.call("ssw_debug_rescore_survivors", idx._h, ctypes.c_void_p(Q.ctypes.data), nq, ctypes.c_void_p(rows.ctypes.data),
              ctypes.c_void_p(cnt.ctypes.data), ctypes.c_void_p(bits.ctypes.data), ctypes.c_void_p(out.ctypes.data),
              ctypes.byref(waves))
    return out.view(np.uint32), int(waves.value)


class Setup:
    def __init__(self, dim, dtype):
        from seesaw_amd.device_index import DeviceIndex
        rng = np.random.default_rng(1000 + dim)
        adv = adversarial_rows(rng, dim)
        gauss = rng.standard_normal((N - adv.shape[0], dim)).astype(np.float32) / np.float32(np.sqrt(dim))
        X = np.concatenate([gauss[:2000], adv, gauss[2000:]])  # row 0 and row N - 1 are ordinary rows
        self.idx = DeviceIndex.from_numpy(X, device=0, dtype=dtype)
        Q = rng.standard_normal((16, dim)).astype(np.float32)
        Q /= np.linalg.norm(Q, axis=1, keepdims=True)
        Q *= np.float32(2.0) ** (24 * (np.arange(16) % 3 - 1))[:, None].astype(np.float32)  # norms 2^-24, 1, 2^24
        self.Q = np.ascontiguousarray(Q)
        self.ref = np.stack([self.idx.scores(q) for q in self.Q]).view(np.uint32)  # computed once, never changed
        self.rng = rng

    def expect(self, j, rows):
        want = np.full(N, SENTINEL, dtype=np.uint32)
        rows = np.asarray(rows, dtype=np.int64)
        want[rows] = self.ref[j, rows]
        return want


@pytest.fixture(scope="module", params=[(256, "float32"), (512, "float32"), (1024, "float32"),
                                        (256, "float16"), (512, "float16"), (1024, "float16")],
                ids=lambda p: "%d-%s" % p)
def setup(request):
    from seesaw_amd import _lib
    with _lib.debug_hooks():
        s = Setup(*request.param)
        yield s
        s.idx.close()


def check(s, nq, counts, lists=None, fail_bits=None, written=None, cap=SURV_CAP):
    """list j has the min(counts[j], cap) entries the hook reads for it"""
    lists = [s.rng.permutation(N)[:min(c, cap)] for c in counts] if lists is None else lists
    slabs, waves = hook(s.idx, s.Q[:nq], lists, counts, fail_bits)
    for j in range(nq):
        wrote = written[j] if written is not None else True
        want = s.expect(j, lists[j]) if wrote else np.full(N, SENTINEL, dtype=np.uint32)
        bad = np.flatnonzero(slabs[j] != want)
        assert bad.size == 0, (nq, j, int(counts[j]), bad[:8], slabs[j][bad[:8]], want[bad[:8]])
    return waves


def test_the_reference_is_not_trivial(setup):
    """the sixteen queries' score rows differ from each other and from the sentinel: equality below means something"""
    assert len({setup.ref[j].tobytes() for j in range(16)}) == 16
    assert not (setup.ref == SENTINEL).any()


def test_counts_around_the_waves_of_a_slot(setup):
    """W = waves a slot has in the launch; a wave keeps two rows in flight, W apart: 0, 1, 2, W - 1, W, W + 1, 2 W + 1"""
    s = setup
    W = check(s, 1, [0])
    assert W >= 4 and 2 * W + 1 <= N, W
    edge = [0, 1, 2, W - 1, W, W + 1, 2 * W + 1]
    for c in edge:  # one slot
        check(s, 1, [c])
    for counts in ([0, W, 2 * W + 1], [2, W - 1, W + 1], [1, 2 * W + 1, W]):  # three slots, each its own count
        check(s, 3, counts)
    more = [3, 5, 2 * W, 2 * W + 2, N, 7, 64, 65, 100]  # sixteen slots, sixteen different counts
    check(s, 16, edge + more)


def test_repeats_and_the_ends_of_the_index(setup):
    s = setup
    lists = [[0, N - 1, 5, 5, 0, N - 1, 7], [N - 1], [0, 0, 0]]
    check(s, 3, [len(l) for l in lists], lists=lists)


def test_the_last_legal_index_of_a_list_and_one_past_the_cap(setup):
    """slot 0 lists 2^18 rows (every entry of its list, the last one included); slot 1 claims 2^18 + 1 and is not
    certified: untouched"""
    s = setup
    full = s.rng.integers(0, N, size=SURV_CAP)
    full[-1] = 4098  # only the list's last entry names this row
    full[:-1][full[:-1] == 4098] = 17
    check(s, 2, [SURV_CAP, SURV_CAP + 1], lists=[full, full], written=[True, False])


def test_a_failed_slot_is_left_alone_between_written_neighbours(setup):
    s = setup
    counts = [40, 33, 50, 21, 60]
    check(s, 5, counts, fail_bits=[0, 1, 0, 2, 0], written=[True, False, True, False, True])
    check(s, 3, counts[:3], fail_bits=[3, 0, 1], written=[False, True, False])


def test_a_count_above_the_tuned_cap(setup):
    from seesaw_amd import _lib
    s = setup
    _lib.call("ssw_tune_surv_cap", 8)
    try:
        W = check(s, 3, [8, 9, 3], written=[True, False, True], cap=8)
        assert W == 4  # one four-wave block is all the loop needs at a cap of 8
        check(s, 2, [SURV_CAP, 7], lists=[np.arange(8), np.arange(7)], written=[False, True])
    finally:
        _lib.call("ssw_tune_surv_cap", 0)
    check(s, 1, [9])  # the product's cap again

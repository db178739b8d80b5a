"""Zero-copy subset views of a resident index (ssw_index_create_view / DeviceIndex.view / subset_view) on the GPU.

The reference in every case is the COPIED subset, DeviceIndex.from_numpy(X[rows], row2image=compact, dtype=...), what
`subset()` builds; for scores also oracle.scores_kernel_order(X[rows], q).  Everything is compared bit for bit.

k = m: ssw_index_topk takes k <= SSW_MAX_TOPK = 4096, so a view of more images asks for 4096 there."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F16, F32 = np.float16, np.float32
SMALL_ROWS = 65536
MAX_TOPK = 4096


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def widen(X):
    return np.asarray(X).astype(np.float16).astype(np.float32)


def hard_rows(oracle, n, dim, seed):
    """as in tests/test_index_f16_gpu.py: unit rows scaled to general magnitudes, with elements in the f16 subnormal
    range and exact round-to-nearest-even ties"""
    rng = np.random.default_rng(seed)
    X = oracle.synth_rows(seed, 0, n, dim) * rng.uniform(0.25, 40.0, size=(n, 1)).astype(np.float32)
    m = rng.random(X.shape)
    X[m < 0.05] = (rng.standard_normal(int((m < 0.05).sum())) * 3e-6).astype(np.float32)  # subnormal in f16
    ties = np.array([1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(2 + 2.0 ** -10), 2.0 ** -25, 3 * 2.0 ** -25,
                     -5 * 2.0 ** -25, 2.0 ** -14 + 2.0 ** -25, 0.5 + 2.0 ** -12], dtype=np.float32)
    sel = (m >= 0.05) & (m < 0.08)
    X[sel] = ties[rng.integers(0, ties.shape[0], int(sel.sum()))]
    return np.ascontiguousarray(X, dtype=np.float32)


def held(X, dtype):
    """the f32 rows an index of that dtype holds"""
    return widen(X) if dtype == F16 else X


class Parent:
    """a ragged multiscale parent: images of lo..hi tiles (seeded), its rows, its image map and its DeviceIndex"""

    def __init__(self, oracle, n_images, lo, hi, dim, dtype, seed, with_map=True):
        from seesaw_amd.device_index import DeviceIndex
        rng = np.random.default_rng(seed)
        self.counts = rng.integers(lo, hi + 1, size=n_images)
        self.counts[0] = self.counts[-1] = hi  # the first and the last image are whole pyramids,
        self.counts[7] = 1                      # this one a single tile
        self.n_images, self.dim, self.dtype, self.with_map = n_images, dim, dtype, with_map
        self.row_start = np.concatenate(([0], np.cumsum(self.counts))).astype(np.int64)
        self.n = int(self.row_start[-1])
        self.r2i = np.repeat(np.arange(n_images), self.counts).astype(np.int32)
        self.X = hard_rows(oracle, self.n, dim, seed=seed + dim)
        self.W = held(self.X, dtype)
        self.dev = DeviceIndex.from_numpy(self.X, row2image=self.r2i if with_map else None, dtype=dtype)

    def rows_of(self, positions):
        from seesaw_amd.device_index import view_rows
        rs = self.row_start if self.with_map else np.arange(self.n + 1)
        return view_rows(rs, positions)

    def copy_of(self, positions):
        """the copied subset index of these members: what subset() builds"""
        from seesaw_amd.device_index import DeviceIndex
        rows, start = self.rows_of(positions)
        compact = np.repeat(np.arange(len(positions)), np.diff(start)).astype(np.int32) if self.with_map else None
        return DeviceIndex.from_numpy(self.X[rows], row2image=compact, dtype=self.dtype)

    def close(self):
        self.dev.close()


def prefix_with_rows_mod(counts, candidates, want, at_least=1):
    """the shortest prefix of `candidates` (image positions) of at least `at_least` rows whose row total is `want` mod 64"""
    total = np.cumsum(counts[candidates])
    hit = np.nonzero((total % 64 == want) & (total >= at_least))[0]
    assert hit.size, (want, at_least)
    return candidates[: hit[0] + 1]


def check_scores(oracle, par, positions, q):
    """view.scores == parent.scores[parent_rows] == the copied subset's == the oracle's, and the row table"""
    rows, start = par.rows_of(positions)
    v = par.dev.view(positions)
    c = par.copy_of(positions)
    try:
        assert v.is_view and v.parent is par.dev and v.n_rows == rows.shape[0] and v.n_images == len(positions)
        assert v.dtype == par.dev.dtype and v.dim == par.dim
        assert np.array_equal(v.parent_rows, rows)  # ssw_index_view_rows against the numpy helper
        got = v.scores(q)
        assert np.array_equal(bits(got), bits(par.dev.scores(q)[rows]))
        assert np.array_equal(bits(got), bits(c.scores(q)))
        assert np.array_equal(bits(got), bits(oracle.scores_kernel_order(par.W[rows], q)))
    finally:
        v.close()
        c.close()
    return rows.shape[0]


# ---- the small form --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, F16], ids=["f32", "f16"])
@pytest.mark.parametrize("dim", [256, 512, 768, 1024])
def test_small_form_scores_bit_exact(oracle, dim, dtype):
    par = Parent(oracle, 3000, 1, 13, dim, dtype, seed=21)
    rng = np.random.default_rng(dim)
    q = oracle.synth_query(dim % 7, dim) * np.float32(1.7)
    every = np.arange(par.n_images)
    odd = every[1::2]  # every run of member rows is one image
    members = {
        "random 30 %": np.nonzero(rng.random(par.n_images) < 0.3)[0],
        "first and last": np.array([0, par.n_images - 1]),
        "one single-tile image": np.array([7]),
        "all but one": np.delete(every, 1234),
        "every other": odd,
        "rows % 64 == 0": prefix_with_rows_mod(par.counts, odd, 0, 2000),
        "rows % 64 == 1": prefix_with_rows_mod(par.counts, odd, 1, 2000),
        "rows % 64 == 63": prefix_with_rows_mod(par.counts, every, 63, 2000),
    }
    try:
        seen = {}
        for name, pos in members.items():
            seen[name] = check_scores(oracle, par, pos, q)
            assert seen[name] <= SMALL_ROWS
        assert par.counts[7] == 1 and seen["one single-tile image"] == 1
        assert [seen["rows %% 64 == %d" % r] % 64 for r in (0, 1, 63)] == [0, 1, 63]
        # 1 and 63 are no multiple of any group size U (2 .. 16)
        assert all(seen["rows % 64 == 1"] % u and seen["rows % 64 == 63"] % u for u in (2, 4, 8, 16))
    finally:
        par.close()


# ---- the streaming form ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big_parents(oracle):
    made = {}

    def get(dim, dtype, with_map=True):
        key = (dim, np.dtype(dtype).name, with_map)
        if key not in made:
            made[key] = Parent(oracle, 20000, 1, 7, dim, dtype, seed=33, with_map=with_map)
        return made[key]

    yield get
    for p in made.values():
        p.close()


def streaming_members(par):
    """images taken in order until the view has more than SMALL_ROWS rows, and a longer prefix cut to rows % 64 == 1"""
    every = np.arange(par.n_images)
    over = every[: int(np.searchsorted(par.row_start, SMALL_ROWS + 1, side="left"))]
    cut = prefix_with_rows_mod(par.counts, every, 1, SMALL_ROWS + 1000)
    return over, cut


@pytest.mark.parametrize("dim,dtype", [(256, F32), (512, F16)], ids=["256-f32", "512-f16"])
def test_streaming_form_scores_bit_exact(oracle, big_parents, dim, dtype):
    par = big_parents(dim, dtype)
    assert 75000 < par.n < 85000
    over, cut = streaming_members(par)
    q = oracle.synth_query(5, dim) * np.float32(0.8)
    n_over = check_scores(oracle, par, over, q)
    assert SMALL_ROWS < n_over <= SMALL_ROWS + 7
    n_cut = check_scores(oracle, par, cut, q)
    assert n_cut > SMALL_ROWS and n_cut % 64 == 1
    # members that are not a prefix: every run one image, the last image among them (the tail clamp reads its rows)
    sparse = np.concatenate((np.arange(0, par.n_images - 1, 1)[np.arange(par.n_images - 1) % 8 != 3], [par.n_images - 1]))
    assert check_scores(oracle, par, sparse, q) > SMALL_ROWS


# ---- top-k -----------------------------------------------------------------------------------------------------------
def same_result(a, b):
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2]), (a[0][:5], b[0][:5])
    assert np.array_equal(bits(a[1]), bits(b[1]))


def check_topk(oracle, par, positions, seed):
    import torch
    rows, start = par.rows_of(positions)
    m = len(positions)
    compact = np.repeat(np.arange(m), np.diff(start)).astype(np.int32) if par.with_map else None
    v, c = par.dev.view(positions), par.copy_of(positions)
    rng = np.random.default_rng(seed)
    q = oracle.synth_query(seed, par.dim)
    ref = oracle.scores_kernel_order(par.W[rows], q)
    excluded = rng.choice(m, size=min(m // 3, 700), replace=False).tolist()
    try:
        for k in (1, 50, min(m, MAX_TOPK)):
            for ex in ([], excluded):
                a = v.topk(q, k, excluded=ex)
                same_result(a, c.topk(q, k, excluded=ex))
                same_result(a, oracle.topk_images_tiebreak(ref, compact, m, ex, k))
        # caller-supplied scores
        s = rng.standard_normal(rows.shape[0]).astype(np.float32)
        s[rng.random(rows.shape[0]) < 0.1] = -np.inf
        for d in (v, c):
            d.load_scores(s)
        a = v.topk(None, 50, excluded=excluded)
        same_result(a, c.topk(None, 50, excluded=excluded))
        same_result(a, oracle.topk_images_tiebreak(s, compact, m, excluded, 50))
        # the device-resident form
        q_dev = torch.from_numpy(q).cuda()
        torch.cuda.synchronize()
        got = []
        for d in (v, c):
            d.set_excluded(excluded)
            d.topk_dev(q_dev.data_ptr(), 50)
            got.append(d.topk_fetch(50))
            assert all(p for p in d.result_ptrs())
        same_result(got[0], got[1])
        same_result(got[0], oracle.topk_images_tiebreak(ref, compact, m, excluded, 50))
    finally:
        v.close()
        c.close()


@pytest.mark.parametrize("dtype", [F32, F16], ids=["f32", "f16"])
@pytest.mark.parametrize("with_map", [True, False], ids=["map", "nomap"])
def test_topk_small_views(oracle, dtype, with_map):
    par = Parent(oracle, 3000, 1, 13, 512, dtype, seed=41, with_map=with_map)
    rng = np.random.default_rng(2)
    try:
        n_pos = par.n_images if with_map else par.n
        check_topk(oracle, par, np.nonzero(rng.random(n_pos) < 0.3)[0], seed=3)
        if not with_map:  # more than 8192 images over at most 65 536 rows: the small scan under the general selection
            pos = np.arange(n_pos)[::2]
            assert 8192 < pos.shape[0] <= SMALL_ROWS
            check_topk(oracle, par, pos, seed=4)
    finally:
        par.close()


@pytest.mark.parametrize("dim,dtype", [(256, F32), (512, F16)], ids=["256-f32", "512-f16"])
@pytest.mark.parametrize("with_map", [True, False], ids=["map", "nomap"])
def test_topk_streaming_views(oracle, big_parents, dim, dtype, with_map):
    par = big_parents(dim, dtype, with_map)
    if with_map:
        pos = streaming_members(par)[1]
    else:
        pos = np.arange(par.n)[np.arange(par.n) % 9 != 4]
    assert par.rows_of(pos)[0].shape[0] > SMALL_ROWS
    check_topk(oracle, par, pos, seed=6)


@pytest.mark.parametrize("dtype", [F32, F16], ids=["f32", "f16"])
@pytest.mark.parametrize("with_map", [True, False], ids=["map", "nomap"])
@pytest.mark.parametrize("n_parent", [30000, 150000], ids=["small", "streaming"])
def test_topk_mass_ties_take_the_deep_path(oracle, n_parent, with_map, dtype):
    """duplicated rows: more than 8192 images share the k-th score, the fast selection overflows, select_deep answers
    -- behind the small and behind the streaming scan, and, with an image map (images of 1, 2, 3, 1, ... rows, every other
    image a member), over the view's own row_start: the best row of a tied image is its first row"""
    import torch
    from seesaw_amd.device_index import DeviceIndex, view_rows
    base = oracle.synth_rows(1, 0, 1, 512)[0]
    if with_map:  # two thirds as many images as a map-less parent has rows
        counts = np.arange(n_parent * 2 // 3) % 3 + 1
        row_start = np.concatenate(([0], np.cumsum(counts))).astype(np.int64)
        r2i = np.repeat(np.arange(counts.shape[0]), counts).astype(np.int32)
    else:
        row_start, r2i = np.arange(n_parent + 1, dtype=np.int64), None
    X = np.repeat(base[None, :] * np.float32(0.5), int(row_start[-1]), axis=0)
    n_pos = row_start.shape[0] - 1
    pos = np.arange(0, n_pos, 2)
    rows, start = view_rows(row_start, pos)
    m = pos.shape[0]
    assert m > 8192 and (rows.shape[0] > SMALL_ROWS) == (n_parent == 150000)
    marked = rows[(np.arange(20) * (rows.shape[0] // 20) + 8)]  # 20 member rows that stand out, some not an image's first
    X[marked] = base[None, :] * np.linspace(0.6, 0.9, 20, dtype=np.float32)[:, None]
    compact = np.repeat(np.arange(m), np.diff(start)).astype(np.int32) if with_map else None
    parent = DeviceIndex.from_numpy(X, row2image=r2i, dtype=dtype)
    v, c = parent.view(pos), DeviceIndex.from_numpy(X[rows], row2image=compact, dtype=dtype)
    try:
        assert np.array_equal(v.parent_rows, rows)
        ref = oracle.scores_kernel_order(held(X[rows], dtype), base)
        for k in (10, 21, 100, 4096):
            a = v.topk(base, k)
            same_result(a, c.topk(base, k))
            same_result(a, oracle.topk_images_tiebreak(ref, compact, m, [], k))
        ex = list(range(0, 60, 3))
        a = v.topk(base, 100, excluded=ex)
        same_result(a, c.topk(base, 100, excluded=ex))
        same_result(a, oracle.topk_images_tiebreak(ref, compact, m, ex, 100))
        # the device-resident form raises the overflow word; the deep selection repairs it
        q_dev = torch.from_numpy(base).cuda()
        torch.cuda.synchronize()
        got = []
        for d in (v, c):
            d.set_excluded(None)
            d.topk_dev(q_dev.data_ptr(), 100)
            d.select_deep_dev(100)
            got.append(d.topk_fetch(100))
        same_result(got[0], got[1])
        same_result(got[0], oracle.topk_images_tiebreak(ref, compact, m, [], 100))
    finally:
        v.close()
        c.close()
        parent.close()


# ---- second stage ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, F16], ids=["f32", "f16"])
def test_second_stage_equals_the_copied_subset(oracle, dtype):
    import torch
    par = Parent(oracle, 3000, 1, 13, 512, dtype, seed=51)
    rng = np.random.default_rng(8)
    pos = np.nonzero(rng.random(par.n_images) < 0.3)[0]
    rows, start = par.rows_of(pos)
    n, m = rows.shape[0], pos.shape[0]
    v, c = par.dev.view(pos), par.copy_of(pos)
    try:
        boxes = rng.uniform(0, 100, (par.n, 4)).astype(np.float32)
        boxes[:, 2:] += boxes[:, :2]
        zoom = rng.integers(0, 3, par.n).astype(np.int32)
        q, q2 = oracle.synth_query(3), oracle.synth_query(9) * np.float32(0.4)
        for d in (v, c):
            d.set_tile_meta(boxes[rows], zoom[rows])  # the view's own tile meta, by view row
            d.scan(q)
        pick = rng.integers(0, n, 3000)
        assert np.array_equal(bits(v.gather_scores(pick)), bits(c.gather_scores(pick)))
        assert np.array_equal(bits(v.gather_scores(pick)), bits(oracle.scores_kernel_order(par.W[rows], q)[pick]))
        assert np.array_equal(bits(v.score_rows(q2, pick)), bits(c.score_rows(q2, pick)))
        assert np.array_equal(bits(v.gather_rows(pick)), bits(par.W[rows][pick]))
        assert np.array_equal(bits(v.gather_rows(pick)), bits(c.gather_rows(pick)))
        cand = np.sort(rng.choice(m, 200, replace=False))
        tiles = np.concatenate([np.arange(start[p], start[p + 1]) for p in cand])
        minus = v.score_rows(q2, tiles)
        for aug in ("all", "greater", "adjacent"):
            for mn in (None, minus):
                sa, ra = v.rescore_avg(cand, aug, mn)
                sb, rb = c.rescore_avg(cand, aug, mn)
                assert np.array_equal(bits(sa), bits(sb)) and np.array_equal(ra, rb), aug
        f64 = torch.from_numpy(rng.random(n)).cuda()
        torch.cuda.synchronize()
        for aug in ("all", "greater", "adjacent"):
            sa, ra = v.rescore_avg_f64(f64.data_ptr(), cand, aug)
            sb, rb = c.rescore_avg_f64(f64.data_ptr(), cand, aug)
            assert np.array_equal(sa.view(np.uint64), sb.view(np.uint64)) and np.array_equal(ra, rb), aug
        # the feedback engine gathers a view's rows through the handle
        from seesaw_amd import _lib
        from seesaw_amd.feedback import FeedbackEngine
        means = []
        for d in (v, c):
            e = FeedbackEngine(512)
            e.set_data_from_index(d, pick[:400], center=True)
            mu = np.empty(512, np.float32)
            _lib.call("ssw_fb_get_mean", e._h, ctypes.c_void_p(mu.ctypes.data))
            means.append(mu)
            e.close()
        assert np.array_equal(bits(means[0]), bits(means[1]))
        st = v.prune_stats(completions=True)
        assert st["shadow"] == "none" and not st["eligible"] and st["queries"] == 0 and st["completions"] == 0
        v.profile(True)
        v.scan(q)
        assert v.profile_read().shape[0] == 1
        v.profile(False)
        assert v.device_ptrs()[0] is None and v.device_ptrs()[1]
    finally:
        v.close()
        c.close()
        par.close()


# ---- lifetime and refusals ---------------------------------------------------------------------------------------------
def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def test_lifetime_refusals_and_parent_updates(oracle):
    import scipy.sparse as sp
    from seesaw_amd import _lib
    from seesaw_amd.device_index import DeviceIndex
    from seesaw_amd.feedback import FeedbackEngine
    from seesaw_amd.label_propagation import LabelPropagation
    par = Parent(oracle, 600, 1, 13, 512, F32, seed=61)
    lib = _lib.load()
    pos = np.arange(0, 600, 3)
    rows, start = par.rows_of(pos)
    v = par.dev.view(pos)
    q = oracle.synth_query(2)
    before = v.topk(q, 40, excluded=[1, 5])

    def refused(fn, status=_lib.SSW_ERR_UNSUPPORTED, word="view"):
        try:
            st = fn()
        except _lib.SeesawHipError as e:
            st = e.status
        assert st == status and word in _lib.last_error(), (st, _lib.last_error())

    # the parent cannot go while the view lives, and is intact afterwards
    with pytest.raises(_lib.SeesawHipError) as e:
        par.dev.close()
    assert e.value.status == _lib.SSW_ERR_INVALID and "view" in str(e.value)
    assert np.array_equal(bits(par.dev.scores(q)[rows]), bits(v.scores(q)))
    # nor can its image map change: the view's members are rows of the images that map named
    refused(lambda: par.dev.set_row2image(par.r2i), status=_lib.SSW_ERR_INVALID, word="view")

    one = np.ascontiguousarray(par.X[:1])
    Q = np.stack([q, oracle.synth_query(4)])
    out = ctypes.c_void_p()
    fb = FeedbackEngine(512)
    lap = LabelPropagation(sp.csr_array(sp.identity(v.n_rows, format="csr") / v.n_rows), reg_lambda=0.0, max_iter=0, device=0)
    xlx_out = np.empty((512, 512), np.float64)
    entries = {
        "upload": lambda: lib.ssw_index_upload(v._h, _p(one), 0, 1),
        "upload_f16": lambda: lib.ssw_index_upload_f16(v._h, _p(one.astype(np.float16)), 0, 1),
        "download": lambda: v.download(0, 1),
        "fill_random": lambda: lib.ssw_index_fill_random(v._h, 1, 0),
        "set_row2image": lambda: v.set_row2image(None),
        "scan_batch": lambda: v.scores_batch(Q),
        "topk_batch": lambda: v.topk_batch(Q, 5),
        "topk_batch_pruned": lambda: v.topk_batch(Q, 5, prune=True),
        "topk_batch_avg": lambda: v.topk_batch_avg(Q, 5, "all"),
        "topk_batch_avg_pruned": lambda: v.topk_batch_avg(Q, 5, "all", prune=True),
        "set_exchange_target": lambda: lib.ssw_index_set_exchange_target(v._h, None, 8, 0, 0, 0),
        "set_exchange_target_batch": lambda: v.set_exchange_target_batch(0, 1, 8, False),
        "topk_batch_dev": lambda: v.topk_batch_dev(Q, 5),
        "topk_batch_dev_pruned": lambda: v.topk_batch_dev(Q, 5, prune=True),
        "topk_slot_deep_dev": lambda: v.topk_slot_deep_dev(q, 5, None, 0),
        "stage2_avg_batch_dev": lambda: v.stage2_avg_batch_dev(Q, 0, 0, 8, 5, "all", 0),
        "knn_build": lambda: v.knn(5),
        "xlx": lambda: lib.ssw_xlx(v._h, lap._h, _p(xlx_out)),
        "fb_set_pseudo_sample_from_index": lambda: lib.ssw_fb_set_pseudo_sample_from_index(
            fb._h, v._h, None, None, None, 0, None, 0, 1.0, 0),
        "view of a view": lambda: lib.ssw_index_create_view(v._h, _p(np.array([0, 1], dtype=np.int64)), 2, ctypes.byref(out)),
    }
    for name, fn in entries.items():
        refused(fn)
        same_result(v.topk(q, 40, excluded=[1, 5]), before)  # a refused entry leaves the view as it was
    assert not out.value
    with pytest.raises(_lib.SeesawHipError):
        v.view([0, 1])
    # the message names the entry that was called, the pruned forms included
    for fn, name in ((entries["topk_batch_pruned"], "ssw_index_topk_batch_pruned:"),
                     (entries["topk_batch_avg_pruned"], "ssw_index_topk_batch_avg_pruned:"),
                     (entries["topk_batch_dev_pruned"], "ssw_index_topk_batch_dev_pruned:"),
                     (entries["topk_batch"], "ssw_index_topk_batch:"), (entries["knn_build"], "ssw_knn_build:")):
        refused(fn, word=name)
    fb.close()
    lap.close()

    # bad member lists are refused on the host, before any launch
    for bad in ([3, 2], [2, 2], [0, 600], [-1, 4], []):
        refused(lambda: par.dev.view(bad), status=_lib.SSW_ERR_INVALID, word="")
    same_result(v.topk(q, 40, excluded=[1, 5]), before)

    # the view reads the parent's current rows: new rows for one member image show in its next scan
    img = int(pos[17])
    r0, r1 = int(par.row_start[img]), int(par.row_start[img + 1])
    fresh = hard_rows(oracle, r1 - r0, 512, seed=99)
    _lib.call("ssw_index_upload", par.dev._h, _p(fresh), r0, r1 - r0)
    X2 = par.X.copy()
    X2[r0:r1] = fresh
    got = v.scores(q)
    assert np.array_equal(bits(got), bits(oracle.scores_kernel_order(X2[rows], q)))
    assert not np.array_equal(bits(got[start[17]:start[18]]), bits(oracle.scores_kernel_order(par.X[r0:r1], q)))

    # two views of one parent, each on its own stream, asked alternately
    pos_b = np.arange(1, 600, 2)
    rows_b = par.rows_of(pos_b)[0]
    w = par.dev.view(pos_b)
    r2i_a = np.repeat(np.arange(len(pos)), np.diff(start)).astype(np.int32)
    r2i_b = np.repeat(np.arange(len(pos_b)), par.counts[pos_b]).astype(np.int32)
    ca = DeviceIndex.from_numpy(X2[rows], row2image=r2i_a)
    cb = DeviceIndex.from_numpy(X2[rows_b], row2image=r2i_b)
    for i in range(6):
        qi = oracle.synth_query(20 + i)
        a, b = v.topk(qi, 30, excluded=[i]), w.topk(qi, 30, excluded=[i + 1])
        same_result(a, ca.topk(qi, 30, excluded=[i]))
        same_result(b, cb.topk(qi, 30, excluded=[i + 1]))
    for d in (w, ca, cb, v):
        d.close()
    par.dev.close()  # no view is left: the parent goes
    assert not par.dev._h


# ---- the index layer ---------------------------------------------------------------------------------------------------
def same_query(a, b):
    assert np.array_equal(a["dbidxs"], b["dbidxs"]), (a["dbidxs"], b["dbidxs"])
    fa, fb = a["activations"], b["activations"]
    assert len(fa) == len(fb) == len(a["dbidxs"])
    if isinstance(fa, list):  # the host-side rescore_candidates path: one frame per image
        assert isinstance(fb, list) and all(x.equals(y) for x, y in zip(fa, fb))
        return
    assert fa._scores.dtype == fb._scores.dtype
    assert np.array_equal(fa._scores.view(np.uint8), fb._scores.view(np.uint8))  # (f32 or f64) bit for bit
    assert np.array_equal(fa._boxes, fb._boxes) and np.array_equal(fa._dbidx, fb._dbidx)


@pytest.fixture(scope="module")
def dataset():
    from seesaw_amd.synthetic import make_dataset
    return make_dataset("views", n_images=120, tiles_per_image=13, positive_frac=0.1, seed=5)


def members_of(ds):
    """70 of the 120 images, every positive of category c1 among them"""
    rng = np.random.default_rng(1)
    pos = set(ds.box_data[ds.box_data.category == "c1"].dbidx.tolist())
    rest = [d for d in range(120) if d not in pos]
    return sorted(pos | set(rng.choice(rest, 70 - len(pos), replace=False).tolist()))


@pytest.mark.parametrize("vector_dtype", ["float32", "float16"])
def test_multiscale_subset_view_matches_subset(dataset, vector_dtype):
    from seesaw_amd.bitmap import BitMap
    from seesaw_amd.indices.multiscale.multiscale_index import MultiscaleIndex
    ds = dataset
    full = MultiscaleIndex(embedding=ds.embedding, vectors=ds.vectors, vector_meta=ds.vector_meta, vector_dtype=vector_dtype)
    B = BitMap(members_of(ds))
    sub, view = full.subset(B), full.subset_view(B)
    assert view._dev.is_view and view._dev.parent is full._dev and not sub._dev.is_view
    assert len(view) == len(sub) == 70 and view.vector_meta.equals(sub.vector_meta)
    assert np.array_equal(bits(view.vectors), bits(sub.vectors))
    assert full.subset_view(BitMap(range(120))) is full
    with pytest.raises(NotImplementedError):
        view.subset_view(BitMap(members_of(ds)[:10]))
    q, q2 = ds.embedding.from_string(string="a c1").reshape(-1), ds.embedding.from_string(string="a c2").reshape(-1)
    exclude = BitMap(members_of(ds)[3:9])
    forms = [dict(agg_method="plain_score", aug_larger="greater")]
    forms += [dict(agg_method="avg_score", aug_larger=a) for a in ("all", "greater", "adjacent")]
    for kw in forms:
        for ex in (None, exclude):
            same_query(view.query(vector=q, topk=10, shortlist_size=50, exclude=ex, **kw),
                       sub.query(vector=q, topk=10, shortlist_size=50, exclude=ex, **kw))
        same_query(view.query(vector=q, vector2=q2, topk=10, shortlist_size=50, **kw),
                   sub.query(vector=q, vector2=q2, topk=10, shortlist_size=50, **kw))
    # a view has no batched scan: query_batch is the loop over query
    kw = dict(agg_method="avg_score", aug_larger="greater")
    for a, b in zip(view.query_batch(topk=5, vectors=[q, q2], shortlist_size=25, **kw),
                    sub.query_batch(topk=5, vectors=[q, q2], shortlist_size=25, **kw)):
        same_query(a, b)
    assert np.array_equal(bits(view.score(q)), bits(sub.score(q)))
    s = np.random.default_rng(0).standard_normal(view.vectors.shape[0]).astype(np.float32)
    assert view.topk_from_scores(s, topk_dbidx=20, exclude_dbidx=exclude).equals(
        sub.topk_from_scores(s, topk_dbidx=20, exclude_dbidx=exclude))
    d = members_of(ds)[4]
    assert view.get_data(d).drop(columns="vectors").equals(sub.get_data(d).drop(columns="vectors"))
    assert np.array_equal(np.stack(view.get_data(d).vectors.values), np.stack(sub.get_data(d).vectors.values))
    # getXy of a query object with a few labelled member images: the tiles' labels, and their rows as positions
    from seesaw_amd.basic_types import Box
    ids = members_of(ds)
    frames, positions = [], []
    for idx in (view, sub):
        qq = idx.new_query()
        qq.label_db.put(ids[2], [Box(x1=300, y1=10, x2=400, y2=100, marked_accepted=True)])
        qq.label_db.put(ids[11], [])
        qq.label_db.put(ids[40], [Box(x1=20, y1=250, x2=200, y2=470, marked_accepted=True)])
        frames.append(qq.getXy())
        positions.append(qq.getXy(get_positions=True))
    assert frames[0].equals(frames[1]) and frames[0].shape[0] == 3 * 13 and list(frames[0].columns) == ["dbidx", "ys", "max_iou"]
    assert 0 < frames[0].ys.sum() < 39 and set(frames[0].dbidx.tolist()) == {ids[2], ids[11], ids[40]}
    assert np.array_equal(positions[0][0], positions[1][0]) and np.array_equal(positions[0][1], positions[1][1])
    assert len(positions[0][0]) == int(frames[0].ys.sum()) and len(positions[0][0]) + len(positions[0][1]) == 39
    for idx in (view, sub):
        idx._dev.close()
    full._dev.close()


def test_coarse_subset_view_matches_subset(oracle):
    import pandas as pd
    from seesaw_amd.bitmap import BitMap
    from seesaw_amd.indices.coarse.coarse_index import CoarseIndex
    from seesaw_amd.synthetic import SyntheticEmbedding
    n = 5000
    X = oracle.synth_rows(12, 0, n, 512)
    meta = pd.DataFrame({"dbidx": np.arange(n) * 2 + 1})
    emb = SyntheticEmbedding({}, 512)
    full = CoarseIndex(embedding=emb, vectors=X, vector_meta=meta)
    ids = (np.nonzero(np.random.default_rng(4).random(n) < 0.4)[0] * 2 + 1).tolist()
    B = BitMap(ids)
    sub, view = full.subset(B), full.subset_view(B)
    assert view._dev.is_view and len(view) == len(sub) == len(ids) and view.vector_meta.equals(sub.vector_meta)
    assert full.subset_view(BitMap(meta.dbidx.values.tolist())) is full
    q = oracle.synth_query(1)
    for ex in (None, BitMap(ids[5:40])):
        a, b = view.query(topk=30, vector=q, exclude=ex), sub.query(topk=30, vector=q, exclude=ex)
        assert a["nextstartk"] == b["nextstartk"]
        same_query(a, b)
    for a, b in zip(view.query_batch(topk=7, vectors=[q, oracle.synth_query(2)]),
                    sub.query_batch(topk=7, vectors=[q, oracle.synth_query(2)])):
        same_query(a, b)
    assert np.array_equal(bits(view.score(q)), bits(sub.score(q)))
    # getXy through the stateful query: the labelled images' vectors and labels, and their positions
    from seesaw_amd.basic_types import Box
    got = []
    for idx in (view, sub):
        qq = idx.new_query()
        r = qq.query_stateful(vector=q, batch_size=10)
        assert len(qq.returned) == 10
        for i, d in enumerate(r["dbidxs"]):
            qq.label_db.put(int(d), [Box(x1=0, y1=0, x2=1, y2=1, marked_accepted=True)] if i % 2 == 0 else [])
        got.append((r["dbidxs"], qq.getXy(), qq.getXy(get_positions=True)))
    (da, (Xa, ya), (pa, na)), (db, (Xb, yb), (pb, nb)) = got
    assert np.array_equal(da, db) and Xa.shape == (10, 512) and ya.sum() == 5
    assert np.array_equal(bits(Xa), bits(Xb)) and np.array_equal(ya, yb)
    assert np.array_equal(pa, pb) and np.array_equal(na, nb) and len(pa) == 5 and len(na) == 5
    assert sorted(view._dbidx[np.concatenate([pa, na])].tolist()) == sorted(int(d) for d in da)
    for d in (view, sub):
        d._dev.close()
    full._dev.close()


LOOP_MATRIX = dict(knn_path="exact", symmetric=True, self_edges=False, normalized_weights=False, knn_k=10, edist=0.05)
LOOP_OPTIONS = {
    "multi_reg": dict(label_loss_type="ce_loss", rank_loss_margin=0.2, use_qvec_norm=None, reg_data_lambda=1000.0,
                      reg_norm_lambda=100.0, reg_query_lambda=0.0, verbose=False, max_iter=100, pos_weight="balanced",
                      lr=1.0, matrix_options=LOOP_MATRIX),
    "knn_prop2": dict(matrix_options=LOOP_MATRIX, normalize_scores=False, sigmoid_before_propagate=True, calib_a=10.0,
                      calib_b=-0.4, prior_weight=1.0),
}


@pytest.mark.parametrize("loop", ["multi_reg", "knn_prop2"])
def test_feedback_loop_on_a_view_index_returns_the_subset_sequence(dataset, loop):
    """5 rounds of a fitting loop (labelled rows gathered out of the index, X'LX over its rows) and of a graph loop
    (k-NN graph of its rows, label propagation into its score buffer) on the view index and on the copied subset"""
    import torch
    from seesaw_amd.basic_types import BenchParams, IndexSpec, SessionParams
    from seesaw_amd.bitmap import BitMap
    from seesaw_amd.indices.multiscale.multiscale_index import MultiscaleIndex
    from seesaw_amd.knn_graph import KNNGraph, compute_exact_knn
    from seesaw_amd.seesaw_bench import benchmark_loop
    from seesaw_amd.seesaw_session import Session
    from seesaw_amd.synthetic import GlobalDataManager
    ds = dataset
    full = MultiscaleIndex(embedding=ds.embedding, vectors=ds.vectors, vector_meta=ds.vector_meta)
    ids = members_of(ds)
    B = BitMap(ids)
    p = SessionParams(index_spec=IndexSpec(d_name="views", i_name="multiscale", c_name=None), interactive=loop,
                      interactive_options=LOOP_OPTIONS[loop], batch_size=3, shortlist_size=30, agg_method="avg_score",
                      aug_larger="greater", start_policy="after_first_batch", index_options={"use_vec_index": False})
    b = BenchParams(name=loop, ground_truth_category="c1", qstr="a c1", n_batches=5, max_results=None)
    boxes = ds.box_data[ds.box_data.dbidx.isin(ids)]
    shown = []
    for idx in (full.subset(B), full.subset_view(B)):
        # the graph of the index's own rows, built through the index's device index (a view takes the temporary copy)
        graph = KNNGraph(compute_exact_knn(idx.vectors, n_neighbors=11, device_index=idx._dev))
        idx.knng = {name: graph for name in ("exact", "")}
        np.random.seed(0)
        torch.manual_seed(0)
        session = Session(GlobalDataManager().add(ds), ds, idx, p)
        out = benchmark_loop(session=session, box_data=boxes, subset=B, b=b, p=p)
        assert out["nseen"] >= 12  # (5 batches of 3, unless all 12 positives were found in 4)
        shown.append([im.dbidx for batch in session.get_state().gdata for im in batch])
        del session
        idx._dev.close()
    assert shown[0] == shown[1] and len(shown[0]) >= 12
    full._dev.close()

"""GPU: the tail of the pruned top-k (csrc/prune.hip survivor_pass, csrc/select.hip k_scatter_candidates; DESIGN.md
section 4, "The tail").

Survivor set.  k_survivors / k_survivors_mq pre-test a row on its lower bound alone, with the shadow's largest finite
a_r and s_r in place of the row's, and read the row's constants only when that cannot rule it out.  The set they list
must be exactly the set of the test on the row's own constants: here the numpy statement of that test on the
device's own lb / a / s (float64, the kernel's expression), for the int8 shadow (ssw_debug_prune_survivors), the 6-bit
shadow (ssw_debug_prune6_survivors) and a slot of the pruned batch (ssw_debug_prune_survivors_mq).  Thresholds that
coincide with a row's ub to the last float64 bit are not used: the device may contract the expression's products and
sums (a few float64 ulps), so a threshold is the float32 next to the ub it is chosen beside: about 2^29 float64 ulps away.

Final top-k.  On an index without an image map the pruned call selects among the survivors at or above the threshold
only; every result it can return is compared with the full scan's, byte for byte."""
import ctypes

import numpy as np
import pytest

from _prune6_helpers import hook_bounds6, mode6, width6
from _prune_batch_helpers import hook_bounds_mq, hook_survivors_mq, upper_bound, width
from _prune_helpers import hook_bounds, hook_shadow, hook_survivors, mode, query, same, stats

pytestmark = pytest.mark.gpu

# none is a multiple of a lane's 4 rows, a wave's 256 or a block's 1024; dim 512, and one case each at 256 and 1024
CASES = ((512, (1 << 16) + 1), (512, 100003), (512, (1 << 18) + 37), (256, 100003), (1024, (1 << 16) + 1))
SURV_CAP = 1 << 18
FINAL_CAP = 8192


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def upload(idx, first, B):
    from seesaw_amd import _lib
    B = np.ascontiguousarray(B, dtype=np.float32)
    _lib.call("ssw_index_upload", idx._h, _p(B), int(first), B.shape[0])


def hook_maxima(idx, six):
    from seesaw_amd import _lib
    out = np.zeros(2, np.float32)
    _lib.call("ssw_debug_prune_maxima", idx._h, 1 if six else 0, _p(out))
    return out


def hook_shadow6_consts(idx):
    from seesaw_amd import _lib
    s, a = np.empty(idx.n_rows, np.float32), np.empty(idx.n_rows, np.float32)
    _lib.call("ssw_debug_prune6_shadow", idx._h, 0, idx.n_rows, None, _p(s), _p(a))
    return s, a


def hook_survivors6(idx, threshold, k, cap=SURV_CAP):
    from seesaw_amd import _lib
    rows = np.full(max(int(cap), 1), -1, dtype=np.int64)
    pub, got = ctypes.c_int32(0), ctypes.c_int64(0)
    _lib.call("ssw_debug_prune6_survivors", idx._h, ctypes.c_float(float(threshold)), int(k), int(k), 0, int(cap),
              ctypes.byref(pub), ctypes.byref(got), _p(rows))
    return int(pub.value), int(got.value), rows[:max(int(pub.value), 0)]


def unboundable_block(dim, rng):
    """four rows no shadow bounds: a NaN element, a +inf element, max|x| above 2^60 and below 2^-60"""
    B = (rng.standard_normal((4, dim)) / np.sqrt(dim)).astype(np.float32)
    B[0, 5], B[1, 7] = np.nan, np.inf
    B[2] *= np.float32(2.0 ** 66)
    B[3] *= np.float32(2.0 ** -90)
    return B


def make_index(dim, n, kind):
    """synthetic unit-norm rows; 'span': the first 8192 and the last 2048 rows scaled to norms 2^-20 .. 2^20, so the
    shadow's maxima are ~2^20 times a typical row's constants; unboundable rows at row 0, across the 1024-row edge and
    at row n - 1"""
    from seesaw_amd.device_index import DeviceIndex
    idx = DeviceIndex.synthetic(n, dim, seed=5)
    rng = np.random.default_rng(2)
    if kind == "span":
        for first, m in ((0, 8192), (n - 2048, 2048)):
            X = idx.download(first, m)
            X *= np.exp2((np.arange(m) * 7) % 41 - 20).astype(np.float32)[:, None]
            upload(idx, first, X)
    U = unboundable_block(dim, rng)
    upload(idx, 0, U[:1])
    upload(idx, 1022, U)
    upload(idx, n - 1, U[1:2])
    return idx


def expected(lb, w, T):
    """the kernels' test on a row's own width, float64: the rows with !(ub < T) (a NaN ub survives)"""
    with np.errstate(invalid="ignore", over="ignore"):
        ub = upper_bound(lb, w)
        return ub, np.nonzero(~(ub < np.float64(np.float32(T))))[0]


def beside(u):
    """the float32 neighbours of the float64 value u: the least float32 above it and the greatest below it"""
    u32 = np.float32(u)
    above = u32 if float(u32) > u else np.nextafter(u32, np.float32(np.inf))
    below = u32 if float(u32) < u else np.nextafter(u32, np.float32(-np.inf))
    return above, below


def thresholds_for(lb, w):
    """-inf, +inf, the 100th largest lb, and one float32 above and one below the ub of two bounded rows: a typical one,
    and the widest one (its own width is what a w_max without the s_max term falls short of)"""
    with np.errstate(invalid="ignore", over="ignore"):
        ub = upper_bound(lb, w)
    fin = np.nonzero(np.isfinite(ub))[0]
    chosen = [int(fin[len(fin) // 3]), int(np.argmax(np.where(np.isfinite(ub), w, -1.0)))]
    kth = np.sort(lb[np.isfinite(lb)])[::-1][99]
    Ts = [np.float32(-np.inf), np.float32(np.inf), kth]
    for r in chosen:
        Ts += list(beside(ub[r]))
    return chosen, Ts


def check_set(run, lb, w, n, tag):
    """run(T) -> (published, collected, rows) against the numpy statement, for every threshold"""
    chosen, Ts = thresholds_for(lb, w)
    for T in Ts:
        ub, want = expected(lb, w, T)
        pub, got, rows = run(T)
        msg = (tag, float(T), pub, got, want.size)
        assert got == want.size, msg
        if want.size > SURV_CAP:
            assert pub == -1, msg
            continue
        assert pub == want.size, msg
        assert np.array_equal(np.sort(rows), want), (msg, np.setxor1d(rows, want)[:8])
    # a chosen row is in for the threshold below its ub and out for the one above
    for i, r in enumerate(chosen):
        assert r in expected(lb, w, Ts[4 + 2 * i])[1] and r not in expected(lb, w, Ts[3 + 2 * i])[1]
    # the unboundable rows are in at every threshold but the ones nothing is collected for
    assert np.isin([0, 1022, 1025, n - 1], expected(lb, w, np.float32(np.inf))[1]).all()


@pytest.mark.parametrize("kind", ["unit", "span"])
@pytest.mark.parametrize("dim,n", CASES)
def test_survivor_set_is_the_own_width_test(lab_build, dim, n, kind):
    """int8 shadow, 6-bit shadow and a slot of the pruned batch: maxima = numpy's over the finite device constants;
    survivor set and count = the numpy statement; once more after larger rows made the shadows stale"""
    idx = make_index(dim, n, kind)
    try:
        mode(lab_build, True, 0)
        mode6(True, 0)
        q = query(11, dim)
        Qs = np.stack([query(12, dim), q * np.float32(3), query(13, dim)])
        for stale_round in (0, 1):
            if stale_round:  # rows of norm 2^30 over a lane's worth across a wave edge: both shadows go stale
                X = idx.download(250, 12) * np.float32(2.0 ** 30)
                upload(idx, 250, X)
            # int8 shadow
            lb, Q, bad = hook_bounds(idx, q)
            assert bad == 0
            _, s8, a8 = hook_shadow(idx, codes=False)
            mx = hook_maxima(idx, False)
            assert mx[0] == a8[np.isfinite(a8)].max() and mx[1] == s8[np.isfinite(s8)].max(), (mx, stale_round)
            assert np.isinf(a8).sum() == 6 and np.isfinite(mx).all()
            w = a8.astype(np.float64) * np.float64(Q)
            check_set(lambda T: hook_survivors(idx, T, 100), lb, w, n, ("int8", kind, stale_round))
            # a slot of the pruned batch over the int8 shadow
            got = hook_bounds_mq(idx, Qs, sums=False)
            for slot in (0, 2):
                qq = dict(Q=got["Q"][slot], e=got["e"][slot])
                wm = width(s8, a8, qq, dim)
                check_set(lambda T: hook_survivors_mq(idx, 3, slot, T, 100), got["lb"][slot], wm, n,
                          ("mq", kind, slot, stale_round))
            # 6-bit shadow
            b6 = hook_bounds6(idx, q, sums=False)
            assert not b6["bad"]
            s6, a6 = hook_shadow6_consts(idx)
            mx6 = hook_maxima(idx, True)
            assert mx6[0] == a6[np.isfinite(a6)].max() and mx6[1] == s6[np.isfinite(s6)].max(), (mx6, stale_round)
            w6 = width6(s6, a6, b6, dim)
            check_set(lambda T: hook_survivors6(idx, T, 100), b6["lb"], w6, n, ("q6", kind, stale_round))
            if kind == "span":  # the pre-test passes almost every row here: w_max is far above a typical w
                assert mx[0] > 2.0 ** 15 * np.median(a8[np.isfinite(a8)])
    finally:
        mode(lab_build, True)
        mode6(True)
        idx.close()


def test_survivor_list_past_a_blocks_stage(lab_build):
    """A block collects its survivors in an LDS stage of 1024 rows and hands over to the global counter when a wave-step
    no longer fits.  2^21 + 37 rows are two strides of the launch, so a block takes eight wave-steps; in sixteen blocks
    30 % ... 100 % of the rows are made to survive (a multiple of the query added to them), in claims of ~75 ... 256
    rows: blocks that stay under the stage, blocks that end just under or just over it, and blocks that pass it after
    four wave-steps.  Set and count must be the numpy statement's whichever way the claims of a block's four waves
    interleave (each form is run three times)."""
    import torch
    from seesaw_amd.device_index import DeviceIndex
    n, dim, stage = (1 << 21) + 37, 256, 1024
    idx = DeviceIndex.synthetic(n, dim, seed=6)
    try:
        mode(lab_build, True, 0)
        mode6(True, 0)
        q = query(31, dim)
        rng = np.random.default_rng(9)
        p_hot = np.repeat(0.30 + 0.70 * np.arange(16) / 15.0, 1024)
        for first in (4096, (1 << 20) + 4096):
            X = idx.download(first, 16 * 1024)
            hot = rng.random(16 * 1024) < p_hot
            X[hot] += np.float32(4) * q
            upload(idx, first, X)
        grid = min(4 * torch.cuda.get_device_properties(0).multi_processor_count, (n + 1023) // 1024)

        def per_block(rows):
            return np.bincount((rows // 1024) % grid, minlength=grid)

        T = np.float32(2)

        def check(name, l, w, run):
            _, want = expected(l, w, T)
            counts = per_block(want)
            # the case is what it says: blocks past the stage, blocks that end near it on either side, blocks under it
            assert counts.max() > 2 * stage - 64 and ((counts > stage) & (counts < stage + 256)).any(), counts[counts > 0]
            assert ((counts > stage - 256) & (counts <= stage)).any() and (counts[counts > 0] < stage - 256).any()
            assert want.size <= SURV_CAP
            for _ in range(3):
                pub, collected, rows = run()
                assert pub == collected == want.size, (name, pub, collected, want.size)
                assert np.array_equal(np.sort(rows), want), (name, np.setxor1d(rows, want)[:8])

        # each form's survivors right after its own bounds: the hooks share the handle's score buffer
        lb, Q, bad = hook_bounds(idx, q)
        assert bad == 0
        _, s8, a8 = hook_shadow(idx, codes=False)
        check("int8", lb, a8.astype(np.float64) * np.float64(Q), lambda: hook_survivors(idx, T, 100))
        got = hook_bounds_mq(idx, np.stack([q, query(32, dim)]), sums=False)
        check("mq", got["lb"][0], width(s8, a8, dict(Q=got["Q"][0], e=got["e"][0]), dim),
              lambda: hook_survivors_mq(idx, 2, 0, T, 100))
        b6 = hook_bounds6(idx, q, sums=False)
        s6, a6 = hook_shadow6_consts(idx)
        _, want = expected(b6["lb"], width6(s6, a6, b6, dim), T)
        assert per_block(want).max() > stage
        for _ in range(3):
            pub, collected, rows = hook_survivors6(idx, T, 100)
            assert pub == collected == want.size and np.array_equal(np.sort(rows), want), ("q6", pub, want.size)
    finally:
        mode(lab_build, True)
        mode6(True)
        idx.close()


# ---- the final top-k from the survivor list ---------------------------------------------------------------------------
N_TOPK = 100003


def dev_results(idx, torch, k):
    """(keys [k], count and overflow word, best rows [k]) the last selection left on the device"""
    from seesaw_amd import _lib
    from seesaw_amd.sharded import _DevArray
    keys_ptr, count_ptr, best_ptr = idx.result_ptrs()
    dev = torch.device("cuda", 0)
    torch.cuda.synchronize()
    idx.sync()
    keys = torch.as_tensor(_DevArray(keys_ptr, (_lib.SSW_MAX_TOPK,), "<i8"), device=dev).cpu().numpy()
    count = torch.as_tensor(_DevArray(count_ptr, (2,), "<i4"), device=dev).cpu().numpy()
    best = torch.as_tensor(_DevArray(best_ptr, (_lib.SSW_MAX_TOPK,), "<u4"), device=dev).cpu().numpy()
    c = min(int(count[0]), k)
    return keys[:c].copy(), count.copy(), best[:c].copy()


def score_buffer(idx, torch):
    """a view of the handle's score buffer that does not complete it (taken while the buffer is whole)"""
    from seesaw_amd import _lib
    from seesaw_amd.sharded import _DevArray
    s = ctypes.c_void_p()
    _lib.call("ssw_index_device_ptrs", idx._h, None, ctypes.byref(s))
    return torch.as_tensor(_DevArray(s.value, (idx.n_rows,), "<f4"), device=torch.device("cuda", 0))


def set_shadow(lab_build, six):
    mode(lab_build, True, 0)
    mode6(bool(six), 0)


def host_and_device(lab_build, idx, torch, q, k, ex, six, k_max=1024):
    """one call's every output with the pruning off and on: the host result (decoded from the packed host block), the
    device's keys / count / overflow word / best rows, and the message of an attached ShardedTopK target"""
    from seesaw_amd import _lib
    from seesaw_amd.sharded import ShardedTopK
    dev = torch.device("cuda", 0)
    q_dev = torch.from_numpy(q).to(dev)
    out = []
    for on in (False, True):
        mode(lab_build, on, 0)
        mode6(bool(six) and on, 0)
        host = idx.topk(q, k, excluded=ex)
        st_host = stats(idx).copy()
        x = ShardedTopK(rank=0, world=1, device=dev, image_offset=7, k_max=k_max, with_best=True)
        x.attach(idx, row_offset=11)
        idx.set_excluded(ex)
        idx.topk_dev(q_dev.data_ptr(), k)
        keys, count, best = dev_results(idx, torch, k)
        msg = x.send_buf.cpu().numpy().copy()
        c = int(count[0])
        msg = np.concatenate([msg[:c], msg[k_max:k_max + c], msg[-1:]])  # the words of this call
        _lib.call("ssw_index_set_exchange_target", idx._h, None, 0, 0, 0, 0)
        idx.set_excluded(None)
        out.append((list(host) + [keys, count, best, msg], st_host, stats(idx).copy()))
    set_shadow(lab_build, six)
    (full, _, _), (got, st_h, st_d) = out
    same(full, got)
    return full, st_h, st_d


@pytest.fixture(scope="module")
def base_rows():
    """what the cases below put over rows of the synthetic index: computed once, never changed"""
    rng = np.random.default_rng(8)
    return dict(q=query(21), nan=unboundable_block(512, rng)[:1])


@pytest.mark.parametrize("six", [0, 1])
def test_final_topk_from_the_survivor_list(lab_build, base_rows, six):
    """no image map: k = 1, 100, 1024; exclusions that remove part of the exact top-k and other survivors; duplicated
    rows tied at the k-th score; a NaN score leading; the buffer after the call"""
    import torch
    from seesaw_amd.device_index import DeviceIndex
    idx = DeviceIndex.synthetic(N_TOPK, 512, seed=3)
    try:
        q = base_rows["q"]
        buf = score_buffer(idx, torch)
        mode(lab_build, False)
        S = idx.scores(q)
        order = np.argsort(-S, kind="stable")
        # rows tied at the 100th score: copies of that row below and above it by position, and one far away
        tied = idx.download(int(order[99]), 1)
        for p in (int(order[99]) - 1 if order[99] > 0 else 5, int(order[99]) + 1, 3, N_TOPK - 2):
            upload(idx, p, tied)
        S = idx.scores(q)
        order = np.argsort(-S, kind="stable")
        assert (S == S[order[99]]).sum() >= 4
        set_shadow(lab_build, six)
        for k in (1, 100, 1024):
            full, st_h, st_d = host_and_device(lab_build, idx, torch, q, k, None, six)
            assert len(full[0]) == k and st_h[2] >= k and st_d[2] >= k, (k, st_h, st_d)  # both calls were pruned
            assert full[4][1] == 0
        # the ties break by image position: the lowest positions of the tied rows come first
        full, _, _ = host_and_device(lab_build, idx, torch, q, 100, None, six)
        t = np.nonzero(full[1] == S[order[99]])[0]
        assert t.size >= 1 and np.all(np.diff(full[0][t]) > 0)
        # exclusions: every other image of the exact top-64 and every third of the next 400 (survivors at k = 100)
        ex = np.concatenate([order[:64:2], order[100:500:3]])
        full, st_h, _ = host_and_device(lab_build, idx, torch, q, 100, ex, six)
        assert not np.isin(full[0], ex).any() and st_h[2] >= 100
        # the buffer after a pruned call: the exact score on every survivor, a lower bound below T elsewhere
        set_shadow(lab_build, six)
        got = idx.topk(q, 100)
        idx.sync()
        B = buf.cpu().numpy()
        exact = B.view(np.uint32) == S.view(np.uint32)
        T = got[1][-1]
        assert exact[got[0]].all() and exact.sum() == stats(idx)[2], (int(exact.sum()), stats(idx))
        assert np.all(B[~exact] < S[~exact]) and np.all(B[~exact] < T)
        same(got, idx.topk(None, 100))  # and its readers complete it
        # a NaN score leads: sign-clear NaN keys order above +inf
        upload(idx, 4099, base_rows["nan"])
        mode(lab_build, False)
        assert np.isnan(idx.scores(q)[4099])
        for k in (1, 100):
            full, st_h, _ = host_and_device(lab_build, idx, torch, q, k, None, six)
            assert full[0][0] == 4099 and np.isnan(full[1][0]) and st_h[2] >= k
    finally:
        mode(lab_build, True)
        mode6(True)
        idx.close()


@pytest.mark.parametrize("six", [0, 1])
def test_final_topk_overflow_fallback_and_map(lab_build, base_rows, six):
    """more than FINAL_CAP duplicated rows tied at the top raise the overflow word and the deep rerun equals the full
    scan's; fewer than k images left fall back; an index with an image map keeps its path and its result"""
    import torch
    from seesaw_amd.device_index import DeviceIndex
    idx = DeviceIndex.synthetic(N_TOPK, 512, seed=3)
    try:
        q = base_rows["q"]
        # fewer than k non-excluded images: the threshold selection returns 50 keys, the call falls back
        ex = np.arange(50, N_TOPK)
        full, st_h, st_d = host_and_device(lab_build, idx, torch, q, 100, ex, six)
        assert len(full[0]) == 50 and st_h[2] == -1 and st_d[2] == -1
        # with a map (ragged: 1 .. 5 rows an image)
        sizes = np.random.default_rng(4).integers(1, 6, N_TOPK)
        r2i = np.repeat(np.arange(N_TOPK, dtype=np.int64), sizes)[:N_TOPK].astype(np.int32)
        idx.set_row2image(r2i)
        full, st_h, _ = host_and_device(lab_build, idx, torch, q, 100, r2i[::977][:20], six)
        assert len(full[0]) == 100 and st_h[2] >= 100
        idx.set_row2image(None)
        # FINAL_CAP + 300 copies of the best row, spread over the index
        mode(lab_build, False)
        best = idx.download(int(np.argmax(idx.scores(q))), 1)
        step = N_TOPK // (FINAL_CAP + 300)
        for first in range(0, (FINAL_CAP + 300) * step, 512 * step):
            m = min(512, FINAL_CAP + 300 - first // step)
            X = idx.download(first, (m - 1) * step + 1)
            X[::step] = best
            upload(idx, first, X)
        # identical rows have identical lower bounds: the threshold selection overflows first and the call falls back
        full, st_h, st_d = host_and_device(lab_build, idx, torch, q, 100, None, six)
        assert full[4][1] == 1 and st_d[2] == -1               # the device-resident call reports the overflow
        assert np.array_equal(full[0], np.arange(100) * step)  # the host call reran the deep path: lowest positions
        # the same rows a step of 2^-20 apart in norm: the bounds spread over many 24-bit prefixes, the threshold selection
        # succeeds, and every one of the rows is a survivor at or above T -- more candidates than k_final takes.  Its own
        # test raises the overflow word (the full buffer's selection has no reason to), the host call reruns the deep
        # path by itself and the device-resident caller does (ssw_index_select_deep_dev): both equal the full scan's
        for first in range(0, (FINAL_CAP + 300) * step, 512 * step):
            m = min(512, FINAL_CAP + 300 - first // step)
            X = idx.download(first, (m - 1) * step + 1)
            j = first // step + np.arange(m)
            X[::step] = best * (np.float32(1) + j.astype(np.float32) * np.float32(2.0 ** -20))[:, None]
            upload(idx, first, X)
        mode(lab_build, False)
        full = idx.topk(q, 100)
        q_dev = torch.from_numpy(q).to(torch.device("cuda", 0))
        idx.topk_dev(q_dev.data_ptr(), 100)
        keys_full, count_full, best_full = dev_results(idx, torch, 100)
        assert count_full[1] == 0
        set_shadow(lab_build, six)
        same(full, idx.topk(q, 100))
        assert stats(idx)[2] >= FINAL_CAP + 300
        idx.topk_dev(q_dev.data_ptr(), 100)
        assert dev_results(idx, torch, 100)[1][1] == 1
        idx.select_deep_dev(100)
        keys, count, best_rows = dev_results(idx, torch, 100)
        same([keys_full, count_full, best_full], [keys, count, best_rows])
    finally:
        mode(lab_build, True)
        mode6(True)
        idx.close()

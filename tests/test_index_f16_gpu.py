"""GPU: the opt-in float16 vector index.  Every operation on an f16 index returns the bits the same operation returns
on an f32 index of the widened rows `widen(X) = X.astype(np.float16).astype(np.float32)`; scores are checked against
the kernel-order oracle on the widened rows, selections against an f32 DeviceIndex of them."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F16 = np.float16


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def widen(X):
    return np.asarray(X).astype(np.float16).astype(np.float32)


def hard_rows(oracle, n, dim, seed):
    """unit rows scaled to general magnitudes, with elements in the f16 subnormal range and exact
    round-to-nearest-even ties (halfway between two binary16 neighbours, normal and subnormal)"""
    rng = np.random.default_rng(seed)
    X = oracle.synth_rows(seed, 0, n, dim) * rng.uniform(0.25, 40.0, size=(n, 1)).astype(np.float32)
    m = rng.random(X.shape)
    X[m < 0.05] = (rng.standard_normal(int((m < 0.05).sum())) * 3e-6).astype(np.float32)  # subnormal in f16
    ties = np.array([1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(2 + 2.0 ** -10), 2.0 ** -25, 3 * 2.0 ** -25,
                     -5 * 2.0 ** -25, 2.0 ** -14 + 2.0 ** -25, 0.5 + 2.0 ** -12], dtype=np.float32)
    sel = (m >= 0.05) & (m < 0.08)
    X[sel] = ties[rng.integers(0, ties.shape[0], int(sel.sum()))]
    return np.ascontiguousarray(X, dtype=np.float32)


@pytest.fixture(scope="module")
def DeviceIndex():
    from seesaw_amd.device_index import DeviceIndex
    return DeviceIndex


@pytest.mark.parametrize("n,dim", [(1, 512), (63, 512), (64, 512), (65, 512), (14417, 512), (65535, 512),
                                   (65536, 512), ((1 << 20) + 17, 512), (70000, 256), (70000, 768), (70000, 1024)])
def test_scores_equal_kernel_order_oracle_on_widened_rows(DeviceIndex, oracle, n, dim):
    X = hard_rows(oracle, n, dim, seed=n % 1000 + dim)
    W = widen(X)
    idx = DeviceIndex.from_numpy(X, dtype=F16)
    assert idx.dtype == np.float16
    for qs in range(2):
        q = oracle.synth_query(qs, dim) * np.float32(1.7)
        got = idx.scores(q)
        assert np.array_equal(bits(got), bits(oracle.scores_kernel_order(W, q))), (n, dim, qs)
    idx.close()


def test_device_rounding_equals_numpy_and_raw_upload(DeviceIndex, oracle):
    X = hard_rows(oracle, 5000, 512, seed=4)
    X[0, :8] = [65504.0, 65519.0, 65520.0, 1e6, -7e4, 6e-8, 2.9e-8, -3.0e-8]  # max, below / at overflow, inf, tiny
    a = DeviceIndex.from_numpy(X, dtype=F16, chunk_rows=777)
    b = DeviceIndex.from_numpy(X.astype(np.float16), dtype=F16, chunk_rows=1000)
    da, db = a.download(), b.download()
    assert np.array_equal(bits(da), bits(widen(X)))
    assert np.array_equal(bits(db), bits(widen(X)))
    assert np.isinf(da[0, 2]) and np.isinf(da[0, 4]) and da[0, 1] == 65504.0
    assert np.array_equal(bits(a.download(1234, 321)), bits(widen(X[1234:1555])))
    a.close()
    b.close()


def _pair(DeviceIndex, X, row2image=None):
    return (DeviceIndex.from_numpy(X, row2image=row2image, dtype=F16),
            DeviceIndex.from_numpy(widen(X), row2image=row2image))


def _same_topk(h, f, q, k, excluded=None):
    a = h.topk(q, k, excluded=excluded)
    b = f.topk(q, k, excluded=excluded)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2])
    assert np.array_equal(bits(a[1]), bits(b[1]))
    return a


def test_topk_with_exclusions_and_ragged_images(DeviceIndex, oracle):
    rng = np.random.default_rng(1)
    counts = rng.integers(1, 40, size=5000)
    row2image = np.repeat(np.arange(5000), counts).astype(np.int32)
    X = hard_rows(oracle, row2image.shape[0], 512, seed=9)
    h, f = _pair(DeviceIndex, X, row2image)
    q = oracle.synth_query(4)
    ref = oracle.scores_kernel_order(widen(X), q)
    returned = []
    for rnd in range(4):
        imgs, scores, rows = _same_topk(h, f, q if rnd == 0 else None, 50, returned)
        o = oracle.topk_images_tiebreak(ref, row2image, 5000, returned, 50)
        assert np.array_equal(imgs, o[0]) and np.array_equal(bits(scores), bits(o[1])) and np.array_equal(rows, o[2])
        returned.extend(imgs[:10].tolist())
    h.close()
    f.close()


def test_topk_small_form_fewer_than_k_and_all_excluded(DeviceIndex, oracle):
    X = hard_rows(oracle, 300, 512, seed=2)
    h, f = _pair(DeviceIndex, X)
    q = oracle.synth_query(0)
    imgs, _, _ = _same_topk(h, f, q, 1000)
    assert imgs.shape[0] == 300
    assert _same_topk(h, f, q, 10, range(300))[0].shape[0] == 0
    assert sorted(_same_topk(h, f, q, 10, range(295))[0].tolist()) == [295, 296, 297, 298, 299]
    h.close()
    f.close()


def test_topk_mass_ties_take_the_deep_path(DeviceIndex, oracle):
    base = oracle.synth_rows(1, 0, 1, 512)[0]
    X = np.repeat(base[None, :] * np.float32(0.5), 30000, axis=0)
    pos = np.arange(20) * 1000 + 7
    X[pos] = base[None, :] * np.linspace(0.6, 0.9, 20, dtype=np.float32)[:, None]
    h, f = _pair(DeviceIndex, X)
    for k in (10, 21, 100, 4096):
        _same_topk(h, f, base, k)
    h.close()
    f.close()


def test_score_rows_gather_rows_and_rescore_avg(DeviceIndex, oracle):
    n_images, tiles = 700, 13
    n = n_images * tiles
    X = hard_rows(oracle, n, 512, seed=12)
    r2i = np.repeat(np.arange(n_images), tiles).astype(np.int32)
    h, f = _pair(DeviceIndex, X, r2i)
    rng = np.random.default_rng(5)
    rows = rng.integers(0, n, 3000)
    q = oracle.synth_query(3)
    assert np.array_equal(bits(h.score_rows(q, rows)), bits(f.score_rows(q, rows)))
    assert np.array_equal(bits(h.gather_rows(rows)), bits(widen(X)[rows]))
    boxes = rng.uniform(0, 100, (n, 4)).astype(np.float32)
    boxes[:, 2:] += boxes[:, :2]
    zoom = np.tile(np.array([0] + [1] * 4 + [2] * 8, np.int32), n_images)
    for d in (h, f):
        d.set_tile_meta(boxes, zoom)
        d.scan(q)
    pos = np.arange(0, n_images, 3)
    for aug in ("all", "greater", "adjacent"):
        sa, ra = h.rescore_avg(pos, aug)
        sb, rb = f.rescore_avg(pos, aug)
        assert np.array_equal(bits(sa), bits(sb)) and np.array_equal(ra, rb)
    h.close()
    f.close()


@pytest.mark.parametrize("dim", [256, 512, 768, 1024])
def test_synthetic_is_the_rounded_oracle_rows(DeviceIndex, oracle, dim):
    idx = DeviceIndex.synthetic(4099, dim, seed=11, first_row=5, dtype=F16)
    assert np.array_equal(bits(idx.download()), bits(widen(oracle.synth_rows(11, 5, 4099, dim))))
    idx.close()


def _views(idx, torch):
    from seesaw_amd import _lib
    from seesaw_amd.sharded import _DevArray
    keys_ptr, count_ptr, _ = idx.result_ptrs()
    dev = torch.device("cuda", 0)
    return (torch.as_tensor(_DevArray(keys_ptr, (_lib.SSW_MAX_TOPK,), "<i8"), device=dev),
            torch.as_tensor(_DevArray(count_ptr, (2,), "<i4"), device=dev))


def test_f16_shards_merged_equal_the_whole_index(DeviceIndex, oracle):
    """several f16 shards of one synthetic index on one GPU: local selections packed and merged as ShardedTopK does
    equal the whole f16 index's keys"""
    import torch
    from seesaw_amd.sharded import ShardedTopK
    sizes = [1, 40000, 0, 700, 99999, 13, 30000, 29287]
    offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(int)
    k, seed = 100, 91
    q_dev = torch.from_numpy(oracle.synth_query(6)).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    x = ShardedTopK(rank=0, world=len(sizes), device=torch.device("cuda", 0), image_offset=0, k_max=128)
    x.world = 1
    shards = []
    for r, (n, off) in enumerate(zip(sizes, offsets)):
        idx = DeviceIndex.synthetic(n, 512, seed=seed, first_row=int(off), dtype=F16)
        shards.append(idx)
        idx.set_stream(stream)
        idx.topk_dev(q_dev.data_ptr(), k)
        keys, count = _views(idx, torch)
        if n == 0:
            count = torch.zeros(2, dtype=torch.int32, device=keys.device)
        x.all_buf[r] = x.pack(keys, count, k, image_offset=int(off))
    out_keys, out_count = x.merge_gathered(k)
    torch.cuda.synchronize()
    merged = out_keys[: int(out_count.item())].cpu().numpy().view(np.uint64)
    whole = DeviceIndex.synthetic(int(sum(sizes)), 512, seed=seed, dtype=F16)
    whole.set_stream(stream)
    whole.topk_dev(q_dev.data_ptr(), k)
    wkeys, wcount = _views(whole, torch)
    torch.cuda.synchronize()
    assert np.array_equal(merged, wkeys[: int(wcount[0].item())].cpu().numpy().view(np.uint64))
    for s in shards + [whole]:
        s.restore_own_stream()
        s.close()


def test_feedback_data_and_fits_from_an_f16_index(DeviceIndex, oracle):
    """rows gathered out of an f16 index (ssw_fb_set_data_from_index / _pseudo_sample_from_index) are the rows of the
    f32 index of the widened rows: same column means, same fitted coefficients, bit for bit"""
    import torch
    from seesaw_amd.feedback import FeedbackEngine
    from seesaw_amd.logistic_regression import LogisticRegressionPT
    n = 4000
    X = hard_rows(oracle, n, 512, seed=5) / np.float32(20.0)
    h, f = _pair(DeviceIndex, X)
    rng = np.random.default_rng(3)
    rows = np.arange(0, n, 37)
    ea, eb = FeedbackEngine(512), FeedbackEngine(512)
    ea.set_data_from_index(h, rows, center=True)
    eb.set_data_from_index(f, rows, center=True)
    ma, mb = np.empty(512, np.float32), np.empty(512, np.float32)
    from seesaw_amd import _lib
    _lib.call("ssw_fb_get_mean", ea._h, ctypes.c_void_p(ma.ctypes.data))
    _lib.call("ssw_fb_get_mean", eb._h, ctypes.c_void_p(mb.ctypes.data))
    assert np.array_equal(bits(ma), bits(mb))
    ea.close()
    eb.close()
    y = (rng.uniform(size=rows.shape[0]) > 0.7).astype(np.float64)
    q = oracle.synth_query(8)
    w0 = (rng.standard_normal(512) * 0.04).astype(np.float32)
    kw = dict(class_weights="balanced", scale="centered", reg_lambda=1.0, regularizer_vector=q, fit_intercept=False,
              max_iter=50)
    a, b = LogisticRegressionPT(**kw), LogisticRegressionPT(**kw)
    a.fit(None, y, w0=w0, index=h, rows=rows)
    b.fit(None, y, w0=w0, index=f, rows=rows)
    assert np.array_equal(bits(a.get_coeff()), bits(b.get_coeff()))
    scores = rng.random(n)
    dev_scores = torch.from_numpy(scores).cuda()
    lab = np.sort(rng.choice(n, 37, replace=False))
    y_lab = (rng.random(lab.shape[0]) < 0.4).astype(np.float64)
    drawn = rng.permutation(n - lab.shape[0])[:500].astype(np.int64)
    kw = dict(class_weights=1.0, scale="centered", reg_lambda=1.0, regularizer_vector=None, fit_intercept=False,
              max_iter=60, lr=1.0)
    fits = []
    for d in (h, f):
        torch.manual_seed(0)
        m = LogisticRegressionPT(**kw)
        m.fit(None, None, None, index=d, pseudo=(dev_scores.data_ptr(), lab, y_lab, drawn, 3.0))
        fits.append(m)
    assert np.array_equal(bits(fits[0].get_coeff()), bits(fits[1].get_coeff()))
    assert np.array_equal(bits(fits[0].mu_), bits(fits[1].mu_))
    h.close()
    f.close()


def test_knn_and_xlx_refuse_an_f16_index(DeviceIndex, oracle):
    import scipy.sparse as sp
    from seesaw_amd import _lib
    from seesaw_amd.knn_graph import compute_exact_knn
    from seesaw_amd.label_propagation import LabelPropagation
    X = hard_rows(oracle, 3000, 512, seed=7) / np.float32(20.0)
    h = DeviceIndex.from_numpy(X, dtype=F16)
    before = h.download()
    with pytest.raises(_lib.SeesawHipError) as e:
        h.knn(5)
    assert e.value.status == _lib.SSW_ERR_UNSUPPORTED and "f16" in str(e.value)
    L = sp.identity(3000, format="csr") / 3000.0
    lap = LabelPropagation(sp.csr_array(L), reg_lambda=0.0, max_iter=0, device=0)
    out = np.empty((512, 512), np.float64)
    st = _lib.load().ssw_xlx(h._h, lap._h, ctypes.c_void_p(out.ctypes.data))
    lap.close()
    assert st == _lib.SSW_ERR_UNSUPPORTED and "f16" in _lib.last_error()
    assert np.array_equal(bits(h.download()), bits(before))
    # borrowing a device matrix is refused for f16
    raw = ctypes.c_void_p()
    st = _lib.load().ssw_index_create_typed(0, 10, 512, _lib.SSW_DTYPE_F16, ctypes.c_void_p(h.device_ptrs()[0]),
                                            ctypes.byref(raw))
    assert st == _lib.SSW_ERR_UNSUPPORTED and not raw.value
    # the Python graph build takes the f32 route on the widened rows
    W = widen(X)
    g16 = compute_exact_knn(W, 10, device_index=h)
    g32 = compute_exact_knn(W, 10)
    assert g16.equals(g32)
    h.close()


def test_f16_matrix_takes_half_the_bytes(DeviceIndex):
    import torch
    n, dim = 4 << 20, 512
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info(0)
    idx = DeviceIndex(n, dim, dtype=F16)
    free1, _ = torch.cuda.mem_get_info(0)
    used = free0 - free1
    matrix = n * dim * 2
    assert matrix <= used <= matrix + n * 4 + (64 << 20), used  # + the [n] f32 score buffer and the query
    idx.close()


def test_100m_rows_topk_equals_merged_shards_and_oracle_samples(DeviceIndex, oracle):
    """100 M x 512 f16 (102.4 GB): the top-100 of the whole index equals the merge of 8 shards of 12.5 M rows built and
    freed one at a time; 4096 sampled rows score as the oracle on their rounded synthetic rows"""
    n, seed, k = 100_000_000, 2024, 100
    q = oracle.synth_query(17)
    merged = []
    per = n // 8
    for s in range(8):
        sh = DeviceIndex.synthetic(per, 512, seed=seed, first_row=s * per, dtype=F16)
        imgs, scores, _ = sh.topk(q, k)
        sh.close()
        merged += [(-float(sc), int(i) + s * per, sc) for i, sc in zip(imgs, scores)]
    merged.sort(key=lambda t: (t[0], t[1]))
    idx = DeviceIndex.synthetic(n, 512, seed=seed, dtype=F16)
    imgs, scores, rows = idx.topk(q, k)
    assert np.array_equal(imgs, np.array([t[1] for t in merged[:k]]))
    assert np.array_equal(bits(scores), bits(np.array([t[2] for t in merged[:k]], np.float32)))
    sample = np.sort(np.random.default_rng(0).choice(n, 4096, replace=False))
    W = np.concatenate([widen(oracle.synth_rows(seed, int(r), 1, 512)) for r in sample])
    ref = oracle.scores_kernel_order(W, q)
    assert np.array_equal(bits(idx.score_rows(q, sample)), bits(ref))
    assert np.array_equal(bits(idx.scores(q)[sample]), bits(ref))
    idx.close()


def test_float64_input_rounds_directly_like_numpy(DeviceIndex, oracle):
    """f64 rows are rounded to binary16 in one step (numpy's astype(float16)), not through f32: a value just above an
    f16 tie that f32 would round onto the tie lands on the upper neighbour"""
    X = oracle.synth_rows(3, 0, 300, 512).astype(np.float64)
    X[0, :4] = [1 + 2.0 ** -11 + 2.0 ** -40, -(1 + 2.0 ** -11 + 2.0 ** -40), 2.0 ** -25 + 2.0 ** -60, 0.1]
    idx = DeviceIndex.from_numpy(X, dtype=F16, chunk_rows=128)
    got = idx.download()
    assert np.array_equal(bits(got), bits(X.astype(np.float16).astype(np.float32)))
    assert got[0, 0] == np.float32(1 + 2.0 ** -10) and got[0, 2] == np.float32(2.0 ** -24)
    idx.close()

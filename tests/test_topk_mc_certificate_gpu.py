"""GPU: the certificate of the large-batch top-k on the matrix cores (csrc/index_mc.hip) checked row by row on what the
device wrote.  tests/test_topk_matrix_core_gpu.py compares end results; a row dropped or mis-numbered outside a query's
top 4 k, or an error bound E that is too small, is invisible there.  The lab hook ssw_debug_mc_candidates drives the
product's stages through the product's run_group and returns their state, which is held to float64 / numpy statements
(tests/_mc_helpers.py) and to the oracle's scan bits, never to the code under test:

  a. mapping (mode 1): every query's buffer holds the rows 0 .. n-1 each once, and every fp16-path score is the float64
     product of the binary16 operands within the header's accumulation term D 2^-23 |ah| |ch|;
  b. the bound (mode 1 + E of mode 0): |fp16-path score / (scale scale_q) - scan score| <= E for every (query, row);
  c. the premise (mode 0): every row outside a query's list has scan score <= b + E; every kept entry is >= thr, rows
     distinct and < n.

SSW_MC_CERTIFICATE_PROFILE=<path> writes the largest observed ratios per family, dim and dtype there
(profiles/topk_mc_certificate.txt is such a run)."""
import os

import numpy as np
import pytest

import _mc_helpers as mc

pytestmark = pytest.mark.gpu

DIMS = (256, 1024)  # one per strip height
DTYPES = (np.float32, np.float16)
SHAPES = ((1, 129), (63, 1), (129, 128), (3968, 127), (3968, 129))  # (n, nq): n in {1, 63, 129, 4097 - 129}, nq in {1, 127, 128, 129}
K = 10
RECORD = {}  # (family, dim, dtype) -> [accumulation ratio, bound ratio, proven, uncertified, overflowed]


def f64(a):
    return np.asarray(a, dtype=np.float64)


def scan_scores(oracle, Xs, Q):
    return np.stack([oracle.scores_kernel_order(Xs, q) for q in Q])


def record(family, dim, dtype, acc=0.0, bound=0.0, flags=None):
    r = RECORD.setdefault((family.__name__, dim, np.dtype(dtype).name), [0.0, 0.0, 0, 0, 0])
    r[0], r[1] = max(r[0], float(acc)), max(r[1], float(bound))
    if flags is not None:
        for f in range(3):
            r[2 + f] += int(np.sum(flags == f))


@pytest.fixture(scope="module", autouse=True)
def profile():
    yield
    path = os.environ.get("SSW_MC_CERTIFICATE_PROFILE")
    if not path or not RECORD:
        return
    with open(path, "w") as f:
        f.write("tests/test_topk_mc_certificate_gpu.py on an MI355X: the largest observed figures over the shapes of a family\n"
                "acc   = max |device fp16-path score - float64 product of the binary16 operands| / (D 2^-23 |ah| |ch|)\n"
                "bound = max |device fp16-path score / (scale scale_q) - scan score| / E (E as k_mc_finish evaluated it)\n"
                "both must be <= 1; proven / uncertified / overflowed: the finish's flags over the queries of the family\n\n")
        f.write(f"{'family':<20}{'dim':>6}{'dtype':>9}{'acc':>12}{'bound':>12}{'proven':>8}{'uncert':>8}{'overfl':>8}\n")
        for (name, dim, dt), r in sorted(RECORD.items()):
            f.write(f"{name:<20}{dim:>6}{dt:>9}{r[0]:>12.4g}{r[1]:>12.4g}{r[2]:>8}{r[3]:>8}{r[4]:>8}\n")


def check_meta(h, Xs, Q, k):
    """what the device derived once per call against numpy: exact maxima, powers of two, a norm bound that holds and is
    tight, M"""
    assert h["maxabs_x"] == np.max(np.abs(Xs)) and h["maxabs_q"] == np.max(np.abs(Q))
    assert h["scale"] == mc.pow2_scale(h["maxabs_x"]) and h["scale_q"] == mc.pow2_scale(h["maxabs_q"])
    assert 128 <= h["scale"] * h["maxabs_x"] < 256 and 128 <= h["scale_q"] * h["maxabs_q"] < 256
    true_norm = np.sqrt((f64(Xs) ** 2).sum(1)).max()
    assert true_norm <= h["maxnorm"] <= true_norm * 1.001
    assert h["M"] == max(64, 1 << int(np.ceil(np.log2(4 * k))))


def check_premise(h, S, n):
    """c. for every query: the kept entries and the rows outside the list"""
    for b in range(S.shape[0]):
        rows, sc, thr = h["rows"][b], h["scores"][b], h["thr"][b]
        assert rows.shape[0] == h["cnt"][b] <= h["M"]
        assert np.unique(rows).shape[0] == rows.shape[0] and (rows >= 0).all() and (rows < n).all(), b
        assert (sc >= thr).all(), b
        assert h["b"][b] == np.float32(np.float32(thr / np.float32(h["scale"])) / np.float32(h["scale_q"]))
        outside = np.ones(n, dtype=bool)
        outside[rows] = False
        if thr == -np.inf:  # never raised: the list holds every row
            assert not outside.any(), b
        elif h["flags"][b] != 2:
            assert (f64(S[b][outside]) <= f64(h["b"][b]) + f64(h["E"][b])).all(), (b, f64(S[b][outside]).max(), h["b"][b], h["E"][b])


def cases():
    for family in mc.FAMILIES:
        for dtype in DTYPES:
            if family in mc.F32_ONLY and dtype == np.float16:
                continue
            for dim in DIMS:
                for n, nq in SHAPES:
                    yield pytest.param(family, dtype, dim, n, nq, id=f"{family.__name__}-{np.dtype(dtype).name}-{dim}-{n}-{nq}")


@pytest.mark.parametrize("family,dtype,dim,n,nq", list(cases()))
def test_candidates_row_by_row(lab_build, oracle, family, dtype, dim, n, nq):
    from seesaw_amd.device_index import DeviceIndex
    X, Xs, Q = mc.make(family, n, nq, dim, dtype)
    dev = DeviceIndex.from_numpy(X, dtype=dtype)
    try:
        raw = mc.hook(lab_build, dev, Q, K, 1)
        fin = mc.hook(lab_build, dev, Q, K, 0)
    finally:
        dev.close()
    S = scan_scores(oracle, Xs, Q)
    scale, scale_q, S16, norms = mc.fp16_path(Xs, Q)
    check_meta(raw, Xs, Q, K)
    assert raw["scale"] == scale and raw["scale_q"] == scale_q and fin["scale"] == scale and fin["scale_q"] == scale_q
    assert len(raw["levels"]) == 1 and raw["levels"][0] == -(-n // mc.strip_rows(dim))
    assert sorted(raw["perm"].tolist()) == list(range(raw["levels"][0]))
    # a. the mapping: no padding row, no duplicate, no hole, at a short last strip and a short query tile
    dev16 = np.empty((nq, n), dtype=np.float32)
    for b in range(nq):
        assert raw["cnt"][b] == n, (b, raw["cnt"][b])
        assert np.array_equal(np.sort(raw["rows"][b]), np.arange(n)), b
        dev16[b, raw["rows"][b]] = raw["scores"][b]
    acc = np.abs(f64(dev16) - S16)
    bound = mc.accumulation_bound(norms, dim)
    with np.errstate(invalid="ignore", divide="ignore"):
        acc_ratio = np.where(acc == 0, 0.0, acc / bound).max()
    # b. the bound, with E as the finish evaluated it
    err = np.abs(f64(dev16) / scale / scale_q - f64(S))
    E = f64(fin["E"])[:, None]
    assert (E > 0).all() and np.isfinite(E).all()
    bound_ratio = (err / E).max()
    record(family, dim, dtype, acc_ratio, bound_ratio, fin["flags"])
    print(f"accumulation ratio {acc_ratio:.4g}  bound ratio {bound_ratio:.4g}  flags {np.bincount(fin['flags'], minlength=3)}")
    assert (acc <= bound).all(), acc_ratio
    assert (err <= E).all(), bound_ratio
    # the device's E is the kernel's expression: never below the float64 one by more than its own f32 evaluation
    assert (f64(fin["E"]) >= mc.kernel_E(Xs, Q, dtype) * (1 - 1e-5)).all()
    # c. the premise of the certificate
    assert set(fin["flags"].tolist()) <= {0, 1}
    check_premise(fin, S, n)
    for b in range(nq):  # the kept entries are the raw ones: same (score, row) pairs
        assert np.array_equal(fin["scores"][b], dev16[b, fin["rows"][b]]), b


@pytest.mark.parametrize("family,n,levels", [(mc.gaussian, 65_536, 3), (mc.gaussian, 66_000, 4), (mc.near_duplicates, 66_000, 4),
                                             (mc.spike_2_20, 66_000, 4)])
def test_premise_at_three_levels(lab_build, oracle, family, n, levels):
    """c. with thresholds raised on the way: k = 128 (M = 512, a level ratio <= 4).  65 536 rows = 512 strips = 32 x 4 x 4
    are three levels exactly; 66 000 rows (516 strips, a span of 16.1 > 4^2) are dealt to four"""
    from seesaw_amd.device_index import DeviceIndex
    nq, dim, k = 17, 256, 128
    X, Xs, Q = mc.make(family, n, nq, dim, np.float32)
    dev = DeviceIndex.from_numpy(X)
    try:
        fin = mc.hook(lab_build, dev, Q, k, 0)
    finally:
        dev.close()
    check_meta(fin, Xs, Q, k)
    strips = -(-n // 128)
    assert len(fin["levels"]) == levels and fin["levels"][0] == 32 and fin["levels"][-1] == strips
    assert np.all(np.diff(fin["levels"]) > 0) and np.all(fin["levels"][1:] <= 4.0 * fin["levels"][:-1] + 1)
    assert sorted(fin["perm"].tolist()) == list(range(strips))
    S = scan_scores(oracle, Xs, Q)
    assert set(fin["flags"].tolist()) <= {0, 1} and (fin["thr"] > -np.inf).all() and (fin["cnt"] == 512).all()
    check_premise(fin, S, n)
    # the kept entries' scores are the fp16 path's, at the rows they name
    scale, scale_q, ah, ch = mc.fp16_operands(Xs, Q)
    for b in range(nq):
        a = ah[fin["rows"][b]]
        s16 = a @ ch[b]
        bound = dim * 2.0 ** -23 * np.sqrt((a * a).sum(1)) * np.sqrt((ch[b] * ch[b]).sum())
        assert (np.abs(f64(fin["scores"][b]) - s16) <= bound).all(), b
    record(family, dim, np.float32, flags=fin["flags"])


def test_hook_refusals(lab_build, oracle):
    """the product's refusals, and the magnitudes the product diverts"""
    from seesaw_amd import _lib
    from seesaw_amd.device_index import DeviceIndex
    rng = np.random.default_rng(0)
    dev = DeviceIndex.from_numpy(rng.standard_normal((100, 256)).astype(np.float32))
    Q = rng.standard_normal((3, 256)).astype(np.float32)
    with pytest.raises(_lib.SeesawHipError) as e:
        mc.hook(lab_build, dev, Q, 129, 0)
    assert e.value.status == -4
    with pytest.raises(_lib.SeesawHipError) as e:
        mc.hook(lab_build, dev, Q * np.float32(2.0 ** 41), 10, 0)
    assert e.value.status == -4
    view = dev.view(np.arange(10))
    with pytest.raises(_lib.SeesawHipError, match="view"):
        mc.hook(lab_build, view, Q, 10, 0)
    view.close()
    before = dev.matrix_core_stats()
    mc.hook(lab_build, dev, Q, 10, 0)
    assert dev.matrix_core_stats() == before
    # the handle afterwards: partial, the last query kept, as after the product call
    kept, last = dev.topk(None, 10), dev.topk(Q[-1], 10)
    assert all(np.array_equal(a, b) for a, b in zip(kept, last))
    dev.close()
    d384 = DeviceIndex.from_numpy(rng.standard_normal((64, 384)).astype(np.float32))
    with pytest.raises(_lib.SeesawHipError, match="384"):
        mc.hook(lab_build, d384, rng.standard_normal((2, 384)).astype(np.float32), 10, 0)
    d384.close()


def test_overflowing_level_falls_back(lab_build, oracle):
    """the overflow branch (cnt > MC_CAP, flag 2, `overflowed`): 12 288 rows of dim 256 and k = 10 make two levels, the
    second of 8192 rows.  One query's score rises strip by strip in the order the strips are dealt (read from the hook),
    so every row of the second level beats its threshold and its buffer of 4096 entries drops entries; the query is
    answered by the plain batch.  The other queries do not see that element and are proven."""
    from seesaw_amd.device_index import DeviceIndex
    n, nq, dim, k = 12_288, 17, 256, 10
    rng = np.random.default_rng(4)
    X = rng.standard_normal((n, dim)).astype(np.float32)
    Q = rng.standard_normal((nq, dim)).astype(np.float32)
    dev = DeviceIndex.from_numpy(X)
    h = mc.hook(lab_build, dev, Q, k, 1)
    assert h["levels"].tolist() == [32, 96]
    position = np.empty(96, dtype=np.int64)
    position[h["perm"]] = np.arange(96)  # when strip s is dealt
    X[:, 0] = np.float32(1.0) + np.float32(0.05) * position[np.arange(n) // 128].astype(np.float32)
    Q[:, 0] = 0
    Q[5] = 0
    Q[5, 0] = 1
    dev.close()
    dev = DeviceIndex.from_numpy(X)
    fin = mc.hook(lab_build, dev, Q, k, 0)
    assert fin["flags"][5] == 2 and (np.delete(fin["flags"], 5) == 0).all(), fin["flags"]
    got = dev.topk_batch(Q, k, matrix_core=True)
    st = dev.matrix_core_stats()
    assert st["overflowed"] == 1 and st["proven"] == nq - 1 and st["uncertified"] == 0, st
    for b, (im, sc, rw) in enumerate(got):
        r_im, r_sc, r_rw = dev.topk(Q[b], k)
        s = oracle.scores_kernel_order(X, Q[b])
        order = np.lexsort((np.arange(n), -s.astype(np.float64)))[:k]
        assert np.array_equal(im, r_im) and np.array_equal(rw, r_rw) and np.array_equal(sc.view(np.uint32), r_sc.view(np.uint32)), b
        assert np.array_equal(im, order) and np.array_equal(sc.view(np.uint32), s[order].view(np.uint32)), b
    dev.close()

"""Rows shared by the f16 index's pruned top-k tests (tests/test_prune_f16_cpu.py, tests/test_prune_f16_gpu.py): built as
f32 and meant to be rounded to binary16 -- by `round_vectors(X, np.float16)` on the host, by
`DeviceIndex.from_numpy(X, dtype=np.float16)` on the device.  Never imported by the product."""
import numpy as np

from _prune_helpers import adversarial_rows

N_ROWS = 56       # 49 + 7
N_UNBOUNDED = 20  # after the rounding: 3 non-finite, 16 scaled past 65504 (+-inf), the row with 70000


def f16_adversarial_rows(rng, dim):
    """56 f32 rows.  0-48: adversarial_rows (binary16 turns its f32 subnormals and its `tiny` rows 24-25 into zeros --
    bounded zero rows now -- and the rows scaled by 2^50 and 2^66 into +-inf rows); 49: max |x| = 65504, the largest
    binary16; 50: one element 70000, which rounds to +inf; 51: binary16 subnormals (multiples of 2^-24 up to 2^-15)
    beside normal elements; 52: all binary16 subnormals (max >= 2^-60: bounded, unlike the f32 `tiny` rows); 53: 1e-9
    everywhere, which rounds to the zero row; 54: -0.0 elements; 55: rint ties that survive the rounding (element 0 is
    127 * 2^-7, so s = 2^-7 exactly, the rest (j + 0.5) * 2^-7 with integer j in [-126, 125]: all exact in binary16).
    After the rounding rows 26-28, 33-48 and 50 cannot be bounded."""
    A = adversarial_rows(rng, dim)
    base = A[:8]
    top = base[0].copy()
    top[5] = -65504.0
    over = base[1].copy()
    over[11] = 70000.0
    mixed = base[2].copy()
    mixed[::3] = (rng.integers(-512, 513, (dim + 2) // 3) * 2.0 ** -24).astype(np.float32)
    sub = (rng.integers(-512, 513, dim) * 2.0 ** -24).astype(np.float32)
    sub[0] = np.float32(2.0 ** -15)
    small = np.full(dim, 1e-9, np.float32)
    negzero = base[3].copy()
    negzero[::2] = -0.0
    ties = ((rng.integers(-126, 126, dim) + 0.5) * 2.0 ** -7).astype(np.float32)
    ties[0] = np.float32(127 * 2.0 ** -7)
    X = np.concatenate([A, np.stack([top, over, mixed, sub, small, negzero, ties])])
    assert X.shape == (N_ROWS, dim)
    return np.ascontiguousarray(X, dtype=np.float32)


def unbounded_rows(W):
    """rows k_q8_build_h16 must refuse, from the widened rows themselves"""
    fin = np.all(np.isfinite(W), axis=1)
    m = np.max(np.abs(np.where(np.isfinite(W), W, 0)), axis=1)
    return ~fin | ((m > 0) & ((m < np.float32(2.0 ** -60)) | (m > np.float32(2.0 ** 60))))

"""Test infrastructure of the packed 6-bit shadow of an f16 index (tests/test_prune6_f16_cpu.py,
tests/test_prune6_f16_gpu.py): the rows, built as f32 and meant to be rounded to binary16 by
`DeviceIndex.from_numpy(X, dtype=np.float16)`, and their widened rounding W.  The shadow's twin, the placement and the lab
hooks are the f32 path's (_prune6_helpers): the shadow of an f16 index is the shadow of W.  Never imported by the
product."""
import functools

import numpy as np

from _prune_f16_helpers import N_ROWS, f16_adversarial_rows

# The order the binary16-specific rows take in an index too small for the whole block (n < 56): rows that cannot be
# bounded (50: an element that rounds to +inf, 26: +inf, 33: scaled past 65504, 27: -inf, 41) between rows that can (49:
# max |x| = 65504, 55: rint ties, 52: all binary16 subnormals, 8: one huge element, 0: Gaussian, 53: rounds to the zero
# row, ...), so that every n >= 1 starts with an unbounded row and every n >= 2 holds both kinds.
SMALL_ORDER = (50, 49, 26, 55, 52, 33, 8, 0, 53, 27, 51, 19, 54, 29, 41, 16, 22)


def widen(X):
    """W: the f32 rows an f16 index of X holds (numpy's astype(float16): nearest even, overflow to +-inf)"""
    with np.errstate(over="ignore"):
        return np.asarray(X).astype(np.float16).astype(np.float32)


def small_block(dim, lead=0):
    """the 56 binary16-specific rows in SMALL_ORDER (then the rest), rotated left by `lead`"""
    A = f16_adversarial_rows(np.random.default_rng(0), dim)
    order = list(SMALL_ORDER) + [i for i in range(N_ROWS) if i not in SMALL_ORDER]
    return A[np.roll(order, -lead)]


@functools.lru_cache(maxsize=4)
def _rows(n, dim, seed, lead):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, dim), dtype=np.float32) / np.float32(np.sqrt(dim))
    # elements of about 2^-11 .. 2^7: normal binary16 numbers at every scale (binary16: 2^-14 .. 65504)
    X *= np.exp2(rng.integers(-6, 11, n)).astype(np.float32)[:, None]
    m = N_ROWS
    if n < m:
        X[:] = small_block(dim, lead)[:n]
    else:
        A = f16_adversarial_rows(np.random.default_rng(0), dim)
        X[:m] = A
        if n >= 6 * m:
            at = ((n // 2) // 16) * 16 - m // 2  # straddles a 16-row tile boundary
            X[at:at + m] = A
        if n >= 2 * m:
            X[n - m:] = A[::-1]
    X = np.ascontiguousarray(X)
    W = widen(X)
    X.setflags(write=False)
    W.setflags(write=False)
    return X, W


def f16_rows(n, dim, seed=None, lead=0):
    """(X f32 [n, dim], W = its widened rounding), read-only and cached: Gaussian rows of mixed scale inside binary16's
    range with f16_adversarial_rows over the first rows, across a 16-row tile boundary and, reversed, over the last
    rows; an index of fewer than 56 rows is the first n rows of small_block(dim, lead)"""
    return _rows(int(n), int(dim), int(n if seed is None else seed), int(lead))

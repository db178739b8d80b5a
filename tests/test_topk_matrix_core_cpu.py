"""CPU: the two entries of the large-batch top-k on the matrix cores are declared and bound, and the batch entry takes
exactly ssw_index_topk_batch's arguments; its lab hook is a lab-build symbol alone; and the error bound E of its
certificate, as the header of csrc/index_mc.hip derives it, holds in float64 on the input families of the GPU tests."""
import numpy as np
import pytest

import _mc_helpers as mc
from seesaw_amd import _lib


def test_matrix_core_entries_are_declared_and_bound_like_the_plain_batch():
    declared = _lib.declared_symbols()
    assert {"ssw_index_topk_batch_mc", "ssw_index_topk_batch_mc_stats"} <= set(declared) & set(_lib._SIGNATURES)
    assert _lib._SIGNATURES["ssw_index_topk_batch_mc"] == _lib._SIGNATURES["ssw_index_topk_batch"]


def test_the_hook_is_a_lab_build_symbol():
    hooks = _lib.declared_symbols(_lib.DEBUG_HEADER_PATH)
    assert "ssw_debug_mc_candidates" in hooks and "ssw_debug_mc_candidates" in _lib._DEBUG_SIGNATURES
    assert "ssw_debug_mc_candidates" not in _lib.declared_symbols() and "ssw_debug_mc_candidates" not in _lib._SIGNATURES
    assert len(_lib._DEBUG_SIGNATURES["ssw_debug_mc_candidates"][1]) == 16
    assert [n for n in hooks if n.startswith("ssw_debug_mc_")] == ["ssw_debug_mc_candidates"]  # one hook, not a family


def test_helper_scale_is_the_power_of_two_of_the_header():
    for m in (1.0, 127.9, 128.0, 255.9, 256.0, 2.0 ** -40, 2.0 ** 40, 65504.0, 3e-7):
        s = mc.pow2_scale(m)
        assert np.frexp(s)[0] == 0.5 and 128 <= s * float(np.float32(m)) < 256, m


@pytest.mark.parametrize("dim", [256, 1024])
@pytest.mark.parametrize("family", mc.FAMILIES, ids=lambda f: f.__name__)
def test_derived_bound_holds_in_float64(family, dim):
    """the derivation without a GPU: the float64 product of the binary16 operands, unscaled, lies within the header's E
    of the float64 dot product, per (query, row) and with the row's own norm -- E minus its accumulation (2^-13) and
    scan-rounding (2^-20) shares would do, so the full E has to; and the kernel's constants with the largest row norm
    are nowhere below the derived ones"""
    n, nq = 300, 33
    for dtype in (np.float32, np.float16):
        if family in mc.F32_ONLY and dtype == np.float16:
            continue
        X, Xs, Q = mc.make(family, n, nq, dim, dtype)
        assert Xs.dtype == np.float32 and np.isfinite(Xs).all() and np.max(np.abs(Xs)) > 0
        scale, scale_q, S16, norms = mc.fp16_path(Xs, Q)
        exact = Q.astype(np.float64) @ Xs.astype(np.float64).T
        err = np.abs(S16 / scale / scale_q - exact)
        E = mc.derived_E(Xs, Q, dtype)
        assert (err <= E).all(), (err / E).max()
        assert (mc.kernel_E(Xs, Q, dtype)[:, None] >= E).all()
        # the operands are what the header says: within 2^-11 relative or 2^-14 absolute of the scaled values
        _, _, ah, ch = mc.fp16_operands(Xs, Q)
        a, c = Xs.astype(np.float64) * scale, Q.astype(np.float64) * scale_q
        assert (np.abs(ah - a) <= np.maximum(2.0 ** -11 * np.abs(a), 2.0 ** -14)).all()
        assert (np.abs(ch - c) <= np.maximum(2.0 ** -11 * np.abs(c), 2.0 ** -14)).all()
        assert np.abs(ah).max() < 256 and np.abs(ch).max() < 256

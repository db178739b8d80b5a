"""CPU: the batched two-stage lookup's interface (include/seesaw_hip.h: ssw_index_topk_batch_avg) -- declared, exported
and bound; the argument errors that are detected before the device is touched; which index classes batch on the
device."""
import ctypes
import re
import subprocess

import numpy as np

NEW = "ssw_index_topk_batch_avg"


def test_the_entry_is_declared_exported_and_bound():
    from seesaw_amd import _lib
    lib = _lib.load()
    assert NEW in _lib.declared_symbols()
    assert NEW in _lib._SIGNATURES and len(_lib._SIGNATURES[NEW][1]) == 13
    assert getattr(lib, NEW).restype is ctypes.c_int32
    for path in (_lib.LIB_PATH, _lib.DEBUG_LIB_PATH):
        nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        assert re.search(r" T %s$" % NEW, nm, re.M), path
    assert lib.ssw_abi_version() == 1  # additive: the ABI version stays


def test_null_handle_and_empty_batch_are_invalid():
    from seesaw_amd import _lib
    lib = _lib.load()
    q = np.zeros((2, 512), dtype=np.float32)
    cnt = np.zeros(2, dtype=np.int32)
    sc, rows = np.zeros(20, dtype=np.float32), np.zeros(20, dtype=np.int64)
    qp, cp = ctypes.c_void_p(q.ctypes.data), ctypes.c_void_p(cnt.ctypes.data)
    sp, rp = ctypes.c_void_p(sc.ctypes.data), ctypes.c_void_p(rows.ctypes.data)
    call = lib.ssw_index_topk_batch_avg
    assert call(None, qp, 2, None, None, 10, 0, None, None, None, sp, rp, cp) == _lib.SSW_ERR_INVALID
    assert "NULL" in _lib.last_error()
    assert call(None, qp, 0, None, None, 10, 0, None, None, None, sp, rp, cp) == _lib.SSW_ERR_INVALID
    assert "nq=0" in _lib.last_error()
    assert call(None, qp, -3, None, None, 10, 0, None, None, None, sp, rp, cp) == _lib.SSW_ERR_INVALID
    assert "nq=-3" in _lib.last_error()


def test_which_indexes_batch_on_the_device():
    from seesaw_amd.indices.interface import AccessMethod
    from seesaw_amd.indices.multiscale.multiscale_index import MultiscaleIndex
    from seesaw_amd.indices.multiscale.sharded_index import ShardedMultiscaleIndex
    assert MultiscaleIndex.query_batch is not AccessMethod.query_batch
    assert ShardedMultiscaleIndex.query_batch is AccessMethod.query_batch  # it has no whole-matrix device index

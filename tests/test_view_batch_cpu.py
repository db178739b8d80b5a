"""CPU: the batched entries of a subset view (include/seesaw_hip.h: ssw_index_view_scan_batch, ssw_index_view_topk_batch,
ssw_index_view_topk_batch_avg) -- declared, exported and bound; the argument errors that are detected before the device
is touched; the multi-query view kernel's place among the scan kernels (what tests/test_topk_batch_cpu.py asserts for
batch_scores_kernel) and its launcher; the recorded resource-usage table against the instances the launcher names."""
import ctypes
import os
import re

import numpy as np

NEW = ("ssw_index_view_scan_batch", "ssw_index_view_topk_batch", "ssw_index_view_topk_batch_avg")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = "view_batch_kernel"


def test_symbols_are_declared_exported_and_bound():
    from seesaw_amd import _lib
    declared = _lib.declared_symbols()
    lib = _lib.load()
    for name in NEW:
        assert name in declared, name
        assert name in _lib._SIGNATURES, name
        assert getattr(lib, name).restype is ctypes.c_int32
    # the signatures of the plain counterparts
    for name in NEW:
        assert _lib._SIGNATURES[name] == _lib._SIGNATURES[name.replace("_view_", "_")], name
    assert lib.ssw_abi_version() == 1  # additive: the ABI version stays


def test_null_arguments_and_empty_batches_are_invalid():
    from seesaw_amd import _lib
    lib = _lib.load()
    q = np.zeros((2, 512), dtype=np.float32)
    cnt = np.zeros(2, dtype=np.int32)
    qp, cp = ctypes.c_void_p(q.ctypes.data), ctypes.c_void_p(cnt.ctypes.data)
    calls = {
        "ssw_index_view_scan_batch": lambda h, qq, nq: lib.ssw_index_view_scan_batch(h, qq, nq, None),
        "ssw_index_view_topk_batch": lambda h, qq, nq: lib.ssw_index_view_topk_batch(h, qq, nq, None, None, 10, None, None,
                                                                                     None, cp),
        "ssw_index_view_topk_batch_avg": lambda h, qq, nq: lib.ssw_index_view_topk_batch_avg(
            h, qq, nq, None, None, 10, 0, None, None, None, cp, cp, cp),
    }
    assert sorted(calls) == sorted(NEW)
    for name, fn in calls.items():
        assert fn(None, qp, 2) == _lib.SSW_ERR_INVALID, name
        assert "NULL" in _lib.last_error(), (name, _lib.last_error())
        assert fn(None, None, 2) == _lib.SSW_ERR_INVALID, name
        assert "NULL" in _lib.last_error(), (name, _lib.last_error())
        assert fn(None, qp, 0) == _lib.SSW_ERR_INVALID, name
        assert "nq=0" in _lib.last_error(), (name, _lib.last_error())
        assert fn(None, qp, -3) == _lib.SSW_ERR_INVALID, name
        assert "nq=-3" in _lib.last_error(), (name, _lib.last_error())


def _scan_source():
    return open(os.path.join(ROOT, "seesaw_amd", "csrc", "scan.hip")).read()


def _code(text):
    return re.sub(r"//[^\n]*", "", text)


def _braced(code, start):
    """the text of the brace block that opens at or after `start` of comment-free code"""
    i = code.index("{", start)
    depth = 0
    for j in range(i, len(code)):
        depth += {"{": 1, "}": -1}.get(code[j], 0)
        if depth == 0:
            return code[i:j + 1]
    raise AssertionError("unbalanced braces")


def test_the_view_kernel_is_an_instance_of_the_row_format_template():
    """like batch_scores_kernel (tests/test_topk_batch_cpu.py): one template over the row format, built from the one
    dot_frag / group_reduce, with no arithmetic of its own on scores"""
    scan = _scan_source()
    m = re.search(r"template <([^>]*)>\s*__global__\s+__launch_bounds__\(256\)\s+void\s+%s\s*\(" % KERNEL, scan)
    assert m and m.group(1).startswith("class R,")
    assert not re.search("scan|score_rows", KERNEL)  # tests/test_index_f16_cpu.py pins the kernels so named
    body = _braced(_code(scan[m.end():]), 0)
    assert "dot_frag<C>(" in body and "group_reduce<V, true>(" in body
    assert not re.search(r"fma|\+\s*__shfl|__shfl\w*\([^;]*\)\s*\+", body)
    # the row sources come as in view_scores_kernel: the row table read by lane, a group's sources by load_view_group
    assert "load_view_group<R, C, U, NT>(" in body and "row_src[min(" in body and "load_group<" not in body
    # placed behind the view kernels, outside the span tests/test_topk_batch_cpu.py reads as batch_scores_kernel's body
    assert scan.index("void view_small_kernel") < m.start()
    assert not (scan.index("void batch_scores_kernel") < m.start() < scan.index("// Small index"))
    # one definition of the shared pieces, still
    for pattern in (r"float dot_frag\s*\(", r"float group_reduce\s*\("):
        assert len(re.findall(pattern, scan)) == 1, pattern


def _width_table_dims(scan):
    table = re.search(r"SCAN_BATCH_WIDTHS\[\]\s*=\s*\{(.*?)\n\};", scan, re.S).group(1)
    dims = [int(d) for d in re.findall(r"\{\s*(\d+)\s*,", table)]
    assert dims == [256, 512, 768, 1024]
    return dims


def _dispatched_instances(scan):
    """(row format, chunks, rows a group, width) of every launch the dispatch names"""
    code = _code(scan)
    body = _braced(code, code.index("ssw_status scan_batch_dispatch("))
    return body, {(f, int(c), int(u), int(b)) for f, c, u, b in
                  re.findall(r"launch_scan_batch_t<(\w+), (\d+), (\d+), (\d+)>", body)}


def test_the_launcher_names_both_row_formats_at_every_dim():
    scan = _scan_source()
    code = _code(scan)
    launcher = _braced(code, code.index("ssw_status launch_scan_view_batch("))
    assert re.search(r"scan_batch_dispatch\([^;]*\brow_src\b", launcher)
    assert "scan_view_batch_max_width(n_view, dim, dtype)" in launcher
    _, instances = _dispatched_instances(scan)
    for dim in _width_table_dims(scan):
        for fmt in ("F32Rows", "H16Rows"):
            assert any(f == fmt and c == dim // 256 for f, c, _, _ in instances), (fmt, dim)
    # the instance launcher runs the view kernel where it is given a row table, and the parent's kernel where not
    inst = _braced(code, code.index("ssw_status launch_scan_batch_t("))
    assert re.search(r"if \(row_src\)\s*hipLaunchKernelGGL\(\(%s<R, C, U, B, true>\)" % KERNEL, inst)
    assert "batch_scores_kernel<R, C, U, B, true>" in inst
    # the view's width is the parent form's, from the one function; the header declares both
    width = _braced(code, code.index("int scan_view_batch_max_width("))
    assert "scan_batch_max_width(n, dim, dtype)" in width
    common = open(os.path.join(ROOT, "seesaw_amd", "csrc", "ssw_common.h")).read()
    assert "int scan_view_batch_max_width(" in common and "ssw_status launch_scan_view_batch(" in common


def test_the_driver_is_the_one_driver():
    """the view entries run topk_batch_run and the scan loop: no second driver, and the old entries' refusals stay"""
    src = _code(open(os.path.join(ROOT, "seesaw_amd", "csrc", "index_batch.hip")).read())
    assert len(re.findall(r"static ssw_status topk_batch_run\(", src)) == 1
    assert len(re.findall(r"static ssw_status scan_batch_run\(", src)) == 1
    for name in NEW:
        body = _braced(src, src.index("ssw_status %s(" % name))
        assert re.search(r"return (topk_batch_run|topk_batch_avg|scan_batch_run)\(", body), name
        assert '"%s"' % name in src, name  # the refusal of a non-view handle names the entry
    for old in ("ssw_index_scan_batch", "ssw_index_topk_batch", "ssw_index_topk_batch_pruned", "ssw_index_topk_batch_avg",
                "ssw_index_topk_batch_avg_pruned"):
        assert '"%s"' % old in src, old
    assert "launch_scan_view_batch(" in _braced(src, src.index("static ssw_status do_scan_chunk("))


def test_the_resource_table_lists_every_dispatched_instance_without_scratch():
    scan = _scan_source()
    _, instances = _dispatched_instances(scan)
    rows = {}
    for line in open(os.path.join(ROOT, "profiles", "view_batch_resource_usage.txt")):
        f = line.split()
        if len(f) == 13 and f[0].isdigit():
            rows[(f[1], int(f[2]), int(f[3]), int(f[4]))] = dict(dim=int(f[0]), vgprs=int(f[5]), scratch=int(f[8]))
    assert set(rows) == instances and len(rows) == 30
    for key, r in rows.items():
        assert r["scratch"] == 0 and r["dim"] == 256 * key[1] and r["vgprs"] <= 256, (key, r)

"""CPU: the source of the multi-query scan's dispatch (csrc/scan.hip): instances of the one kernel template for one,
three and four 256-element chunks in both row formats, a width table of powers of two instead of a dim-512 test, and a
perf tool that takes the dim."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def scan_source():
    with open(os.path.join(ROOT, "seesaw_amd", "csrc", "scan.hip")) as f:
        return re.sub(r"//[^\n]*", "", f.read())  # code only


def test_the_kernel_is_dispatched_for_one_three_and_four_chunks():
    scan = scan_source()
    for fmt in ("F32Rows", "H16Rows"):
        for chunks in (1, 3, 4):
            found = re.findall(r"launch_scan_batch_t<%s, %d, (\d+), (\d+)>" % (fmt, chunks), scan)
            assert found, (fmt, chunks)
            for rows, width in found:
                rows, width = int(rows), int(width)
                assert width in (2, 4, 8, 16) and rows in (1, 2, 4, 8, 16) and rows * width <= 64, (fmt, chunks, rows, width)
            assert len({w for _, w in found}) == len(found), (fmt, chunks)  # one instance a width


def test_the_width_function_has_no_dim_512_refusal():
    scan = scan_source()
    m = re.search(r"int scan_batch_max_width\([^)]*\)\s*\{(.*?)\n\}", scan, re.S)
    assert m
    body = m.group(1)
    assert not re.search(r"dim\s*!=\s*512", body) and "512" not in body
    assert "SCAN_SMALL_ROWS" in body  # the small range stays unserved at every dim
    assert re.search(r"constexpr int64_t SCAN_SMALL_ROWS = 65536;", scan)


def test_the_width_table_names_powers_of_two_for_every_dim():
    scan = scan_source()
    m = re.search(r"constexpr ScanBatchWidths SCAN_BATCH_WIDTHS\[\] = \{(.*?)\n\};", scan, re.S)
    assert m
    consts = {name: int(v) for name, v in re.findall(r"(SCAN_BATCH_MAX_F(?:32|16)) = (\d+)", scan)}
    assert consts == {"SCAN_BATCH_MAX_F32": 16, "SCAN_BATCH_MAX_F16": 8}  # dim 512 keeps its widths
    rows = re.findall(r"\{\s*(\d+)\s*,([^{}]*)\}", m.group(1))
    assert [int(d) for d, _ in rows] == [256, 512, 768, 1024]
    for dim, rest in rows:
        vals = [consts[v] if v in consts else int(v) for v in (x.strip() for x in rest.split(","))]
        assert len(vals) == 4 and all(v in (2, 4, 8, 16) for v in vals), (dim, vals)
        f32, f16, f32_built, f16_built = vals
        assert f32 <= f32_built and f16 <= f16_built, (dim, vals)  # the product's width is an instance
        # ... and the widest instance the table names is dispatched
        chunks = int(dim) // 256
        for fmt, built in (("F32Rows", f32_built), ("H16Rows", f16_built)):
            widths = {int(w) for w in re.findall(r"launch_scan_batch_t<%s, %d, \d+, (\d+)>" % (fmt, chunks), scan)}
            assert max(widths) == built and widths == {w for w in (2, 4, 8, 16) if w <= built}, (dim, fmt, widths)


def test_the_perf_tool_takes_the_dim():
    with open(os.path.join(ROOT, "tools", "perf_topk_batch.py")) as f:
        tool = f.read()
    assert '"--dim"' in tool and "default=512" in tool
    assert not re.search(r"synthetic\(n, 512", tool)

"""f16 vs f32 index: scan-kernel bandwidth and vectors/s in ONE process (development aid).

    python tools/perf_scan_f16.py [--rows 50e6] [--big 100e6] [--reps 4] [--sweep]

At --rows both indexes are resident at once and the A/B is interleaved round by round; at --big (100 M x 512: f32
204.8 GB + f16 102.4 GB do not fit together) the f32 index is measured and freed, then the f16 one.  Bytes per row:
dim*4 + 4 (f32), dim*2 + 4 (f16, 1 028 B at dim 512), scores included.  --sweep runs the f16 schedule variants and
blocks-per-CU caps on the lab build (ssw_tune_scan), interleaved, at --rows."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from seesaw_amd.device_index import DeviceIndex

DIM = 512


def kernel_ms(idx, q, n_launch=8):
    idx.scan(q)
    idx.profile(True)
    for _ in range(n_launch):
        idx.scan(q)
    ms = idx.profile_read()
    idx.profile(False)
    return float(np.median(ms))


def report(tag, n, ms, elem_bytes):
    row = DIM * elem_bytes + 4
    print(f"{tag} n={n:>11d}: kernel {np.median(ms):8.3f} ms (min {np.min(ms):.3f}) -> "
          f"{n * row / np.median(ms) / 1e9:6.3f} TB/s, {n / np.median(ms) / 1e6:7.2f} G vectors/s", flush=True)
    return n / np.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=float, default=50e6)
    ap.add_argument("--big", type=float, default=100e6, help="0 = skip the sequential large-size run")
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--sweep", action="store_true")
    a = ap.parse_args()
    q = np.random.default_rng(0).standard_normal(DIM).astype(np.float32)
    q /= np.linalg.norm(q)

    n = int(a.rows)
    f32 = DeviceIndex.synthetic(n, DIM, seed=1)
    f16 = DeviceIndex.synthetic(n, DIM, seed=1, dtype=np.float16)
    res = {"f32": [], "f16": []}
    for _ in range(a.reps):  # interleaved A/B
        res["f32"].append(kernel_ms(f32, q))
        res["f16"].append(kernel_ms(f16, q))
    v32 = report("f32", n, res["f32"], 4)
    v16 = report("f16", n, res["f16"], 2)
    print(f"f16 / f32 vectors/s at {n} rows: {v16 / v32:.3f}x", flush=True)
    f32.close()
    if a.sweep:
        from seesaw_amd import _lib
        f16.close()
        with _lib.debug_hooks():
            f16 = DeviceIndex.synthetic(n, DIM, seed=1, dtype=np.float16)
            names = {0: "u4", 1: "u8nt", 4: "u2nt", -1: "u4nt(dflt)"}
            configs = [(v, b) for v in (-1, 0, 1, 4) for b in (1, 2, 0)]
            sw = {c: [] for c in configs}
            for _ in range(a.reps):
                for c in configs:
                    _lib.call("ssw_tune_scan", c[0], c[1])
                    sw[c].append(kernel_ms(f16, q))
            _lib.call("ssw_tune_scan", -1, -1)
            for c in configs:
                report(f"f16 {names[c[0]]} blocks/CU cap {c[1]}", n, sw[c], 2)
            f16.close()
    else:
        f16.close()

    if a.big > 0:  # sequential: the two do not fit together
        nb = int(a.big)
        out = {}
        for tag, dt, eb in (("f32", np.float32, 4), ("f16", np.float16, 2)):
            idx = DeviceIndex.synthetic(nb, DIM, seed=2024, dtype=dt)
            out[tag] = report(tag, nb, [kernel_ms(idx, q) for _ in range(a.reps)], eb)
            idx.close()
        print(f"f16 / f32 vectors/s at {nb} rows: {out['f16'] / out['f32']:.3f}x", flush=True)


if __name__ == "__main__":
    main()

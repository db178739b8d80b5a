#!/usr/bin/env python3
"""Image bytes -> tile vectors: run_multiscale_extraction_pipeline with the host tiler (Pillow pyramid, numpy tiling,
np.stack, 150 KB a tile over the bus: what the parent commit runs, its boxes made in one step instead of two, which makes
generate_multiscale_tiling no slower than the parent's) against device_tiling=True (the host decodes
and plans; pyramid, tiling and gather on the device: csrc/tiler.hip), in one process on one GPU.

    python tools/perf_ingest.py [--small 512] [--large 64] [--repeats 4] [--large-repeats 3] [--out FILE]
    python tools/perf_ingest.py --device-only --small 128 --large 0      # one pass for a kernel trace

Sets: `--small` images of 640 x 480 (13 tiles each at min_tile_size 224) and `--large` images of 3000 x 2000, JPEG bytes
made from a seed (32 / 8 distinct pictures, repeated).  Tower: the product ViT-B/32 shape, randomly initialised.
Per set, after one untimed pass of each path, `--repeats` alternating blocks (host, device, device, host, ...); a block is
one whole pipeline call, parquet file included.  Per path one JSON line:
  total_s       the block times, their median, and the spread (max - min) / median
  images_s, tiles_s   from the median block
  split_s       medians of: decode (the same bytes decoded apart, PIL open + convert + asarray: common to both paths and
                inside both totals), embed (the model call: upload + forward; for the device path + resample and gather;
                ends in a stream synchronise), write (the parquet file), prep = total - decode - embed - write (host path:
                pyramid + tiling + stack + frames; device path: plan + frames)
  upload_bytes_per_image   counted from the shapes: tiles x 224 x 224 x 3 (host) or h x w x 3 (device; its tables --
                coefficients, jobs, 24 bytes a tile -- are reported apart as table bytes of one 16-image call)
  plan_ms       the device path plans once per image SIZE (multiscale_plan keeps the frames per size): the cost of a plan
                the first time a size is seen and of one served from the cache.  Every image of a set here has one size, so
                `prep` holds one first plan; a dataset of all-different sizes pays the first-time cost per image
and one line `identical`: the two paths' frames and vector bits are equal."""
import argparse
import io
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def picture(w, h, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([xx * 255 // (w - 1), yy * 255 // (h - 1), ((xx // 24 + yy // 24) % 2) * 200], axis=2)
    return np.clip(base + rng.integers(-30, 31, size=(h, w, 3)), 0, 255).astype(np.uint8)


def image_rows(n, w, h, distinct):
    import pandas as pd
    import PIL.Image
    blobs = []
    for s in range(min(distinct, n)):
        buf = io.BytesIO()
        PIL.Image.fromarray(picture(w, h, 1000 + s)).save(buf, format="JPEG", quality=90)
        blobs.append(buf.getvalue())
    return pd.DataFrame({"dbidx": np.arange(n), "file_path": [f"im{i}.jpg" for i in range(n)],
                         "bytes": [blobs[i % len(blobs)] for i in range(n)]})


class Timed:
    """the model with a clock around its two tile entries"""

    def __init__(self, model):
        self.model, self.seconds, self.tiles = model, 0.0, 0
        self.projection_dim = model.projection_dim

    def _timed(self, fn, *a, **k):
        t0 = time.perf_counter()
        out = fn(*a, **k)
        self.seconds += time.perf_counter() - t0
        self.tiles += out.shape[0]
        return out

    def embed_tiles_u8(self, tiles, normalize=True):
        return self._timed(self.model.embed_tiles_u8, tiles, normalize=normalize)

    def embed_multiscale_u8(self, images, plans, normalize=True):
        return self._timed(self.model.embed_multiscale_u8, images, plans, normalize=normalize)


def decode_seconds(rows):
    import PIL.Image
    t0 = time.perf_counter()
    for b in rows.bytes:
        np.asarray(PIL.Image.open(io.BytesIO(b)).convert("RGB"))
    return time.perf_counter() - t0


def one_block(rows, model, device_tiling, tmp):
    from seesaw_amd.indices.multiscale import multiscale_tools as mt
    timed = Timed(model)
    write = [0.0]
    real_write = mt.write_vector_parquet

    def timed_write(df, path):
        t0 = time.perf_counter()
        real_write(df, path)
        write[0] += time.perf_counter() - t0

    mt.write_vector_parquet = timed_write
    try:
        t0 = time.perf_counter()
        df = mt.run_multiscale_extraction_pipeline(rows, timed, os.path.join(tmp, "v"), min_tile_size=224,
                                                   device_tiling=device_tiling)
        total = time.perf_counter() - t0
    finally:
        mt.write_vector_parquet = real_write
    return {"total": total, "embed": timed.seconds, "write": write[0], "tiles": timed.tiles}, df


def table_bytes(w, h, n=16):
    """the device path's tables for one call of n such images, from the shapes (csrc/tiler.hip, tiler_plan)"""
    from seesaw_amd.indices.multiscale.multiscale_tools import multiscale_plan
    levels, meta = multiscale_plan((w, h), 224, 0.5, 224)
    coef = 0
    for lw, lh in zip(levels.w, levels.h):  # one block per distinct (in, out) pair of the call: the n images share them
        coef += 4 * (lw * (2 * -(-w // lw) + 3) if lw != w else 0) + 4 * (lh * (2 * -(-h // lh) + 3) if lh != h else 0)
    return int(coef + n * (len(levels) * 2 * 56 + len(meta) * 24))


def plan_ms(w, h, n=20):
    from seesaw_amd.indices.multiscale import multiscale_tools as mt
    first = mt._multiscale_plan.__wrapped__
    t0 = time.perf_counter()
    for _ in range(n):
        first((w, h), 224, 0.5, 224)
    t1 = time.perf_counter()
    for _ in range(n):
        mt.multiscale_plan((w, h), 224, 0.5, 224)
    return {"first": round(1e3 * (t1 - t0) / n, 3), "cached": round(1e3 * (time.perf_counter() - t1) / n, 3)}


def run_set(tag, rows, w, h, model, repeats, device_only, out):
    paths = ("device",) if device_only else ("host", "device")
    with tempfile.TemporaryDirectory() as tmp:
        frames = {p: one_block(rows, model, p == "device", tmp)[1] for p in paths}  # untimed: warms shapes and allocations
        if not device_only:
            a, b = frames["host"], frames["device"]
            same = a.drop(columns="vectors").equals(b.drop(columns="vectors")) and \
                np.array_equal(np.stack(a.vectors.values).view(np.uint32), np.stack(b.vectors.values).view(np.uint32))
            out({"set": tag, "identical": bool(same), "rows": int(a.shape[0])})
        blocks = {p: [] for p in paths}
        decode = []
        for r in range(repeats):
            decode.append(decode_seconds(rows))
            for p in (paths if r % 2 == 0 else paths[::-1]):
                blocks[p].append(one_block(rows, model, p == "device", tmp)[0])
    n = rows.shape[0]
    dec = float(np.median(decode))
    for p in paths:
        tot = np.array([b["total"] for b in blocks[p]])
        med = float(np.median(tot))
        emb, wr = float(np.median([b["embed"] for b in blocks[p]])), float(np.median([b["write"] for b in blocks[p]]))
        tiles = blocks[p][0]["tiles"]
        per_image = tiles // n * 224 * 224 * 3 if p == "host" else h * w * 3
        line = {"set": tag, "path": p, "images": n, "tiles": tiles, "size": [w, h], "blocks": repeats,
                "total_s": {"blocks": [round(float(t), 3) for t in tot], "median": round(med, 3),
                            "spread": round(float((tot.max() - tot.min()) / med), 3)},
                "images_s": round(n / med, 1), "tiles_s": round(tiles / med, 1),
                "split_s": {"decode": round(dec, 3), "embed": round(emb, 3), "write": round(wr, 3),
                            "prep": round(med - dec - emb - wr, 3)},
                "embed_tiles_s": round(tiles / emb, 1), "upload_bytes_per_image": int(per_image)}
        if p == "device":
            line["table_bytes_per_16_image_call"] = table_bytes(w, h)
            line["plan_ms"] = plan_ms(w, h)
        out(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", type=int, default=512)
    ap.add_argument("--large", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=4)
    ap.add_argument("--large-repeats", type=int, default=3)
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("perf_ingest: no GPU (timings are not taken on a CPU)")
    from seesaw_amd.models.clip import ClipModel
    model = ClipModel.random_init()
    sink = open(args.out, "w") if args.out else None

    def out(line):
        text = json.dumps(line)
        print(text, flush=True)
        if sink:
            sink.write(text + "\n")
            sink.flush()

    try:
        if args.small > 0:
            run_set("640x480", image_rows(args.small, 640, 480, 32), 640, 480, model, args.repeats, args.device_only, out)
        if args.large > 0:
            run_set("3000x2000", image_rows(args.large, 3000, 2000, 8), 3000, 2000, model, args.large_repeats,
                    args.device_only, out)
    finally:
        model.close()
        if sink:
            sink.close()


if __name__ == "__main__":
    main()

"""Image tower forward of ViT-B/32, ViT-B/16 and ViT-L/14 at 200 tiles a call (GPU box), full depth, seeded random-init
weights, no HF forward.

  python tools/perf_clip_variants.py [--models b32,b16,l14] [--tiles 200] [--reps 30] [--text]
Per model: the median of `reps` timed calls (each a device-side forward that ends in a synchronise, after 3 warm-up calls)
with min / max and the interquartile spread, tiles/s, and the fraction of the 2.5 PFLOP/s dense bf16 peak priced at the
model's own FLOP count per tile (the reference model's: every row through every layer, as DESIGN does for ViT-B/32).
--text adds the cost of one text query (B = 1, 9 tokens) through the model's text tower.
--package-root DIR imports seesaw_amd from DIR instead of this tree (the parent commit's build, for the A/B of the B/32 line).
"""
import argparse
import os
import sys
import time

import numpy as np

PEAK_BF16 = 2.5e15

MODELS = {
    # name: (patch, vision hidden, heads, mlp, layers, text hidden, heads, mlp, projection)
    "b32": ("ViT-B/32", 32, 768, 12, 3072, 12, 512, 8, 2048, 512),
    "b16": ("ViT-B/16", 16, 768, 12, 3072, 12, 512, 8, 2048, 512),
    "l14": ("ViT-L/14", 14, 1024, 16, 4096, 24, 768, 12, 3072, 768),
}


def tile_flops(patch, D, M, L, P, image=224):
    """multiply-adds x 2 of one tile through the image tower as the reference's model runs it"""
    T = (image // patch) ** 2 + 1
    layer = 2 * T * (3 * D * D + D * D + 2 * D * M) + 4 * T * T * D
    return 2 * (T - 1) * D * 3 * patch * patch + L * layer + 2 * D * P, T


def config(name):
    import transformers
    _, patch, vh, vn, vm, vl, th, tn, tm, proj = MODELS[name]
    return transformers.CLIPConfig(
        text_config=dict(hidden_size=th, num_attention_heads=tn, intermediate_size=tm),
        vision_config=dict(hidden_size=vh, num_attention_heads=vn, intermediate_size=vm, num_hidden_layers=vl,
                           patch_size=patch),
        projection_dim=proj)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="b32,b16,l14")
    ap.add_argument("--tiles", type=int, default=200)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--text", action="store_true")
    ap.add_argument("--package-root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    sys.path.insert(0, args.package_root)
    import torch
    from seesaw_amd.models.clip import ClipModel
    if not torch.cuda.is_available():
        sys.exit("perf_clip_variants: no GPU (a timing taken elsewhere says nothing)")
    import seesaw_amd
    print(f"# {args.label}seesaw_amd from {os.path.relpath(os.path.dirname(seesaw_amd.__file__))}", flush=True)
    dev = torch.device("cuda", 0)
    B = args.tiles
    for name in args.models.split(","):
        title, patch, vh, vn, vm, vl, th, tn, tm, proj = MODELS[name]
        # ViT-B/32 is transformers' default config: created as every other tool does, which the parent commit can do too
        m = ClipModel.random_init(seed=1234) if name == "b32" else ClipModel.random_init(seed=1234, config=config(name))
        flops, T = tile_flops(patch, vh, vm, vl, proj)
        x = torch.randn(B, 3, 224, 224, device=dev)
        out = torch.empty(B, proj, device=dev)
        s = torch.cuda.current_stream().cuda_stream
        for _ in range(3):
            m.embed_image_dev(x.data_ptr(), B, out.data_ptr(), True, s)
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            m.embed_image_dev(x.data_ptr(), B, out.data_ptr(), True, s)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        ts = np.sort(np.array(ts))
        med, q1, q3 = np.median(ts), ts[len(ts) // 4], ts[(3 * len(ts)) // 4]
        assert torch.isfinite(out).all()
        print(f"{args.label}{title}: {T} tokens, {flops / 1e9:.2f} GFLOP a tile; {B} tiles a call, {args.reps} calls: median "
              f"{med * 1e3:.3f} ms (min {ts[0] * 1e3:.3f}, quartiles {q1 * 1e3:.3f} .. {q3 * 1e3:.3f}, max {ts[-1] * 1e3:.3f}); "
              f"{B / med:.0f} tiles/s; {B * flops / med / PEAK_BF16:.3f} of the dense bf16 peak (call time, model FLOPs)",
              flush=True)
        if args.text:
            ids = np.random.default_rng(1).integers(1, 49000, size=(1, 9)).astype(np.int32)
            ids[0, 0], ids[0, 8] = 49406, 49407
            for _ in range(5):
                m.embed_text(ids)
            tt = np.sort(np.array([_timed(lambda: m.embed_text(ids)) for _ in range(50)]))
            print(f"{args.label}{title}: one text query (1 x 9 tokens, hidden {th}, host call to host result): median "
                  f"{np.median(tt) * 1e3:.3f} ms (min {tt[0] * 1e3:.3f}, max {tt[-1] * 1e3:.3f})", flush=True)
        m.close()
        del x, out


def _timed(f):
    t0 = time.perf_counter()
    f()
    return time.perf_counter() - t0


if __name__ == "__main__":
    main()

"""Full-depth error of the ViT-L/14 (24 layers) and ViT-B/16 image towers against transformers.CLIPModel (f32, CPU), seeded
random-init weights (GPU box), with f32 and with bf16 residual rows -- tools/clip_stream_error.py's measurement for the
towers of tools/perf_clip_variants.py.

  python tools/clip_variants_error.py [--tiles 6]
Prints min cosine and max |delta| of the unit vectors: four lines.  The bar is 0.999 / 5e-3.
"""
import argparse
import os
import sys

import numpy as np
import torch
import transformers

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from seesaw_amd.models.clip import ClipModel  # noqa: E402
from tools.perf_clip_variants import MODELS, config  # noqa: E402


def unit(x):
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


ap = argparse.ArgumentParser()
ap.add_argument("--tiles", type=int, default=6)
args = ap.parse_args()
for name in ("b16", "l14"):
    torch.manual_seed(1234)
    hf = transformers.CLIPModel(config(name)).eval()
    ours = ClipModel.from_hf(hf)
    torch.manual_seed(0)
    x = torch.randn(args.tiles, 3, 224, 224)
    with torch.inference_mode():
        ref = hf.get_image_features(pixel_values=x)
        ref = unit((ref.pooler_output if hasattr(ref, "pooler_output") else ref).numpy())
    for bf16 in (False, True):
        ours.set_rows(image_bf16=bf16)
        got = unit(ours.embed_image(x.numpy(), normalize=False))
        d = np.abs(got - ref)
        print(f"{MODELS[name][0]} ({MODELS[name][5]} layers), {args.tiles} tiles, {'bf16' if bf16 else 'f32'} residual rows: "
              f"cos min {(got * ref).sum(1).min():.6f}  |delta| max {d.max():.2e} rms {np.sqrt((d ** 2).mean()):.2e}", flush=True)
    ours.close()
    del hf

"""GPU: SigLIP towers (transformers.SiglipModel) -- head dim 72 on attention_hd, the class-token-free image tower with
its attention-pooling head (map_pool / map_value), the unmasked text tower pooled at the last position, the tanh GELU,
the MLP width 4304 padded to 4352.

The reference is the seeded transformers model in f64 at 2 layers; the bar is tests/test_clip_variants_gpu.py's: minimum
cosine 0.999 and maximum |delta| 5e-3 on the normalised outputs.  transformers initialises every bias to 0 (or 1e-6) and
every LayerNorm to gamma = 1, beta = 0, which would make the patch bias, the folded query bias, gamma (.) u, the value and
out_proj biases, map_pool's gamma / beta epilogue and the text head's bias multiplications by 1 and additions of 0: _hf
gives every 1-D parameter a seeded value of size 0.1 .. 1 (biases of either sign).  Every image case runs with the
initialised probe (near-uniform pooling) and with the probe and the query rows of in_proj_weight x 32 each, where the
f64 reference's pooling weights are asserted to be concentrated (a wrong mask, maximum or rescaling shows)."""
import numpy as np
import pytest
import test_clip_openclip_gpu as openclip

pytestmark = pytest.mark.gpu
COS_MIN, ABS_MAX = 0.999, 5e-3
VOCAB, PAD = 1000, 1

TOWERS = {  # image, patch, vision hidden / heads / MLP, text hidden / heads / MLP
    "base16": (224, 16, (768, 12, 3072), (768, 12, 3072)),          # 196 tokens; 12 heads: the pad to 16
    "so400m14": (224, 14, (1152, 16, 4304), (1152, 16, 4304)),      # 256 tokens; head dim 72, MLP pad, both towers
    "skinny_t1": (32, 32, (256, 4, 512), (128, 2, 128)),            # one token
    "skinny_t49": (224, 32, (256, 4, 512), (128, 2, 128)),          # no multiple of 16, nor of the strip of 32
    "skinny_t256": (128, 8, (256, 4, 512), (128, 2, 128)),          # no image / patch pair gives 272 tokens: 256 is the most
}
_HF = {}


def _hf(name):
    import torch
    import transformers
    if name not in _HF:
        image, patch, (vh, vn, vm), (th, tn, tm) = TOWERS[name]
        cfg = transformers.SiglipConfig(
            text_config=dict(hidden_size=th, num_attention_heads=tn, intermediate_size=tm, num_hidden_layers=2, vocab_size=VOCAB,
                             max_position_embeddings=64, projection_size=vh, pad_token_id=PAD, bos_token_id=None, eos_token_id=None),
            vision_config=dict(hidden_size=vh, num_attention_heads=vn, intermediate_size=vm, num_hidden_layers=2, image_size=image,
                               patch_size=patch))
        torch.manual_seed(4321)
        hf = transformers.SiglipModel(cfg).eval().double()
        g = torch.Generator().manual_seed(99)
        with torch.no_grad():  # (module docstring: no bias at 0, no LayerNorm at identity)
            for key, p in hf.named_parameters():
                if p.ndim == 1 and not key.startswith("logit_"):
                    sign = torch.randint(0, 2, p.shape, generator=g) * 2 - 1 if key.endswith("bias") else 1
                    p.copy_((0.1 + 0.9 * torch.rand(p.shape, generator=g, dtype=torch.float64)) * sign)
        _HF[name] = hf
    return _HF[name]


def _at_the_bar(got, ref, what):
    ref = ref.pooler_output.numpy()
    got, ref = (x / np.linalg.norm(x, axis=-1, keepdims=True) for x in (got.astype(np.float64), ref))
    cos, err = (got * ref).sum(1), float(np.abs(got - ref).max())
    print(f"{what}: min cosine {cos.min():.6f}, max |delta| {err:.2e}")
    assert np.isfinite(got).all() and cos.min() >= COS_MIN and err <= ABS_MAX, (what, cos, err)


@pytest.mark.parametrize("S", [1, 17, 64, 256, 272])
def test_attention_hd_at_head_dim_72_against_the_f64_softmax(lab_build, S):
    openclip.test_attention_hd_against_the_f64_softmax(lab_build, 72, S)


@pytest.mark.parametrize("probe_scale", [1, 32])
@pytest.mark.parametrize("name", list(TOWERS))
def test_image_tower_vs_hf(name, probe_scale):
    import torch
    from seesaw_amd.models.clip import ClipModel
    hf, image, W = _hf(name), TOWERS[name][0], TOWERS[name][2][0]
    head = hf.vision_model.head
    x = np.random.default_rng(5).standard_normal((3, 3, image, image), dtype=np.float32)
    with torch.inference_mode():
        head.probe.data *= probe_scale
        head.attention.in_proj_weight.data[:W] *= probe_scale
        try:
            ours = ClipModel.from_hf(hf)
            ref = hf.vision_model(pixel_values=torch.from_numpy(x).double())
            weights = head.attention(head.probe.repeat(3, 1, 1), ref.last_hidden_state, ref.last_hidden_state,
                                     need_weights=True, average_attn_weights=False)[1]  # [3, heads, 1, T]
        finally:
            head.probe.data /= probe_scale
            head.attention.in_proj_weight.data[:W] /= probe_scale
    top = float(weights.max(-1).values.median())
    print(f"{name} x {probe_scale}: median over (image, head) of the reference's largest pooling weight {top:.3f}")
    assert probe_scale == 1 or top >= 0.5, ("not peaked", top)
    got = ours.embed_image(x, normalize=True)
    assert got.shape == (3, W) and np.abs(got[0] - got[1]).max() > 1e-3
    _at_the_bar(got, ref, f"{name} probe x {probe_scale}")
    # the device entry: NaN images behind the 3 given, NaN rows behind the 3 written; a tile's vector does not depend on its call
    xd = torch.full((4, 3, image, image), float("nan"), device="cuda")
    xd[:3] = torch.from_numpy(x)
    out = torch.full((4, W), float("nan"), device="cuda")
    ours.embed_image_dev(xd.data_ptr(), 3, out.data_ptr(), True, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    ours.close()
    assert np.array_equal(out[:3].cpu().numpy(), got) and bool(torch.isnan(out[3]).all())


@pytest.mark.parametrize("name", ["base16", "so400m14"])
@pytest.mark.parametrize("n,L", [(4, 64), (1, 9)])
def test_text_tower_vs_hf(name, n, L):
    import torch
    from seesaw_amd.models.clip import ClipModel
    hf = _hf(name)
    ids = np.random.default_rng(6).integers(0, VOCAB, size=(n, L)).astype(np.int32)
    ids[0, L // 2:] = PAD  # padded as SigLIP is trained: the pooled row is the last one given, a pad token here
    ids[-1, 0] = PAD
    with torch.inference_mode():
        ref = hf.get_text_features(input_ids=torch.from_numpy(ids.astype(np.int64)))
    ours = ClipModel.from_hf(hf)
    got = ours.embed_text(ids, normalize=L == 9)  # (the bar normalises both sides: either form must meet it)
    ours.close()
    assert got.shape == (n, TOWERS[name][2][0]) and (L != 9 or np.allclose(np.linalg.norm(got, axis=1), 1, atol=1e-5))
    _at_the_bar(got, ref, f"{name} text {n} x {L}")


def test_refusals_name_the_value_and_the_next_call_is_served():
    import transformers
    from seesaw_amd import _lib
    from seesaw_amd.models.clip import ClipModel
    text = dict(hidden_size=128, num_attention_heads=2, intermediate_size=128, num_hidden_layers=1, vocab_size=64)
    small = dict(intermediate_size=128, num_hidden_layers=1)
    for vision, number in ((dict(hidden_size=128, num_attention_heads=2, image_size=384, patch_size=14, **small), "729"),
                           (dict(hidden_size=384, num_attention_heads=4, image_size=32, patch_size=32, **small), "96")):
        cfg = transformers.SiglipConfig(text_config=dict(text, projection_size=vision["hidden_size"]), vision_config=vision)
        with pytest.raises(_lib.SeesawHipError, match=number):
            ClipModel.random_init(config=cfg)
    cfg = transformers.SiglipConfig(text_config=dict(text, projection_size=128),
                                    vision_config=dict(hidden_size=128, num_attention_heads=2, image_size=32, patch_size=32, **small))
    ours = ClipModel.random_init(config=cfg)
    assert np.isfinite(ours.embed_image(np.ones((1, 3, 32, 32), np.float32))).all()
    ours.close()

"""CPU: the host side of the CLIP variants (ViT-B/32, ViT-B/16, ViT-L/14): the weight blob and its header, the config
that random_init passes through, the padded width of a gathered patch row.  No device call."""
import struct

import numpy as np
import pytest

VARIANTS = {
    # name: (image, patch, vision hidden / heads / mlp, text hidden / heads / mlp, projection)
    "ViT-B/32": (224, 32, 768, 12, 3072, 512, 8, 2048, 512),
    "ViT-B/16": (224, 16, 768, 12, 3072, 512, 8, 2048, 512),
    "ViT-L/14": (224, 14, 1024, 16, 4096, 768, 12, 3072, 768),
}
VOCAB = 600  # (the token table is the bulk of a one-layer model)


def _config(name):
    import transformers
    image, patch, vh, vn, vm, th, tn, tm, proj = VARIANTS[name]
    return transformers.CLIPConfig(
        text_config=dict(hidden_size=th, num_attention_heads=tn, intermediate_size=tm, num_hidden_layers=1,
                         vocab_size=VOCAB, bos_token_id=VOCAB - 2, eos_token_id=VOCAB - 1, pad_token_id=0),
        vision_config=dict(hidden_size=vh, num_attention_heads=vn, intermediate_size=vm, num_hidden_layers=1,
                           image_size=image, patch_size=patch),
        projection_dim=proj)


@pytest.fixture
def no_device(monkeypatch):
    """ssw_clip_create and every other library call recorded, not made"""
    from seesaw_amd import _lib
    calls = []
    monkeypatch.setattr(_lib, "call", lambda name, *args: calls.append((name, args)))
    return calls


@pytest.mark.parametrize("name", list(VARIANTS))
def test_blob_and_header_parse_agree(name, no_device):
    import torch
    import transformers
    from seesaw_amd.models.clip import ClipModel, pack_clip_weights
    image, patch, vh, vn, vm, th, tn, tm, proj = VARIANTS[name]
    cfg = _config(name)
    torch.manual_seed(0)
    hf = transformers.CLIPModel(cfg)
    blob = pack_clip_weights(hf.state_dict(), cfg)
    hdr = struct.unpack("<8s6i7iifi", blob[:72].tobytes())
    assert hdr[0] == b"SSWCLIP1"
    assert hdr[1:7] == (vh, 1, vn, vm, image, patch)
    assert hdr[7:15] == (th, 1, tn, tm, 77, VOCAB, VOCAB - 1, proj)
    # the blob is not padded: the patch weight holds 3 patch^2 columns a row, every tensor of the model is in it once
    # (but CLIP's logit_scale, which no tower reads)
    assert blob.nbytes == 72 + 4 * (sum(p.numel() for p in hf.parameters()) - hf.logit_scale.numel())
    body = blob[72:].view(np.float32)
    w = hf.state_dict()["vision_model.embeddings.patch_embedding.weight"].numpy().reshape(-1)
    assert np.array_equal(body[vh:vh + vh * 3 * patch * patch], w)
    tokens = (image // patch) ** 2 + 1
    assert tokens in (50, 197, 257) and tokens <= 272
    m = ClipModel(blob)
    assert [c[0] for c in no_device] == ["ssw_clip_create"]
    assert (m.image_size, m.patch_size, m.projection_dim) == (image, patch, proj)
    assert (m.vision_hidden, m.text_hidden) == (vh, th)
    assert (m.max_positions, m.vocab_size, m.eos_token_id) == (77, VOCAB, VOCAB - 1)


def test_random_init_passes_the_config_through(no_device):
    from seesaw_amd.models.clip import ClipModel
    m = ClipModel.random_init(seed=3, config=_config("ViT-L/14"))
    assert (m.image_size, m.patch_size, m.projection_dim, m.vision_hidden, m.text_hidden) == (224, 14, 768, 1024, 768)
    name, args = no_device[0]
    assert name == "ssw_clip_create" and args[2].value > 72 + 4 * 1024 * 3 * 14 * 14  # (blob bytes: header + weights)
    assert ClipModel.OPT_ATTN_LONG == 6 and ClipModel.OPT_FULL_LAST_LAYER == 4


def test_option_numbers_match_the_header():
    import re
    from seesaw_amd import _lib
    from seesaw_amd.models.clip import ClipModel
    text = open(_lib.HEADER_PATH).read()
    defines = dict(re.findall(r"#define SSW_CLIP_OPT_([A-Z0-9_]+) (\d+)", text))
    assert {k: int(v) for k, v in defines.items()} == {
        "IMAGE_ROWS_BF16": ClipModel.OPT_IMAGE_ROWS_BF16, "TEXT_ROWS_BF16": ClipModel.OPT_TEXT_ROWS_BF16,
        "ATTN_DIRECT": ClipModel.OPT_ATTN_DIRECT, "ATTN_OUT_UNFUSED": ClipModel.OPT_ATTN_OUT_UNFUSED,
        "FULL_LAST_LAYER": ClipModel.OPT_FULL_LAST_LAYER, "ATTN_LONG": ClipModel.OPT_ATTN_LONG}


@pytest.mark.parametrize("patch,cols", [(14, 640), (16, 768), (32, 3072), (8, 192), (7, 192), (15, 704), (4, 64)])
def test_padded_patch_width(patch, cols):
    from seesaw_amd.models.clip import patch_columns
    assert patch_columns(patch) == cols == -(-3 * patch * patch // 64) * 64
    assert patch_columns(patch) % 64 == 0 and 0 <= patch_columns(patch) - 3 * patch * patch < 64
    if patch % 8 == 0:
        assert patch_columns(patch) == 3 * patch * patch  # the 8-pixel gathers' rows are not padded


def test_load_clip_reads_an_hf_directory_of_another_variant(no_device, tmp_path):
    """load_clip(<directory with config.json + weights>) needs nothing new for a ViT-L/14-shaped model"""
    import torch
    import transformers
    from seesaw_amd.models.embeddings import load_clip
    cfg = _config("ViT-L/14")
    cfg.vision_config.hidden_size, cfg.vision_config.num_attention_heads, cfg.vision_config.intermediate_size = 128, 2, 128
    cfg.text_config.hidden_size, cfg.text_config.num_attention_heads, cfg.text_config.intermediate_size = 128, 2, 128
    torch.manual_seed(0)
    transformers.CLIPModel(cfg).save_pretrained(str(tmp_path / "hf"))
    m = load_clip(str(tmp_path / "hf"))
    assert (m.image_size, m.patch_size, m.projection_dim, m.vision_hidden, m.text_hidden) == (224, 14, 768, 128, 128)
    assert [c[0] for c in no_device] == ["ssw_clip_create"]

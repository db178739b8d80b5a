"""CPU: the host side of the SigLIP towers -- the SSWSIGL1 blob, from_hf's dispatch by model_type, and the tanh GELU
staying out of the SSWCLIP1 header.  No device call."""
import struct

import pytest


@pytest.fixture
def no_device(monkeypatch):
    """ssw_clip_create and every other library call recorded, not made (as tests/test_clip_variants_cpu.py)"""
    from seesaw_amd import _lib
    calls = []
    monkeypatch.setattr(_lib, "call", lambda name, *args: calls.append((name, args)))
    return calls


def _siglip():
    import torch
    import transformers
    cfg = transformers.SiglipConfig(
        text_config=dict(hidden_size=128, num_attention_heads=2, intermediate_size=200, num_hidden_layers=1, vocab_size=300,
                         max_position_embeddings=64, projection_size=256),
        vision_config=dict(hidden_size=256, num_attention_heads=4, intermediate_size=200, num_hidden_layers=1, image_size=64,
                           patch_size=32))
    torch.manual_seed(0)
    return transformers.SiglipModel(cfg).eval()


def test_from_hf_packs_a_siglip_model_into_its_own_blob(no_device):
    from seesaw_amd.models.clip import ClipModel, pack_siglip_weights
    hf = _siglip()
    blob = pack_siglip_weights(hf.state_dict(), hf.config)
    hdr = struct.unpack("<8s6i7iifi2i", blob[:80].tobytes())
    assert hdr[0] == b"SSWSIGL1"
    assert hdr[1:7] == (256, 1, 4, 200, 64, 32) and hdr[7:13] == (128, 1, 2, 200, 64, 300) and hdr[14] == 256
    assert hdr[16:] == (2, 4, 0)  # tanh GELU, the pooling head's heads, the reserved word
    # unpadded (MLP width 200), every parameter once but logit_scale and logit_bias
    assert blob.nbytes == 80 + 4 * (sum(p.numel() for p in hf.parameters()) - hf.logit_scale.numel() - hf.logit_bias.numel())
    m = ClipModel.from_hf(hf)  # model_type "siglip" -> the same packer
    (name, args), = no_device
    assert name == "ssw_clip_create" and args[2].value == blob.nbytes and m.is_siglip
    assert (m.image_size, m.patch_size, m.projection_dim, m.vision_hidden, m.max_positions) == (64, 32, 256, 256, 64)


def test_a_clip_config_with_the_tanh_gelu_is_still_refused():
    import transformers
    from seesaw_amd.models.clip import ACTIVATION_CODES, pack_clip_weights
    cfg = transformers.CLIPConfig(text_config=dict(hidden_act="gelu_pytorch_tanh"), vision_config=dict(hidden_act="gelu_pytorch_tanh"))
    assert ACTIVATION_CODES == {"quick_gelu": 0, "gelu": 1}
    with pytest.raises(ValueError, match="gelu_pytorch_tanh"):
        pack_clip_weights({}, cfg)

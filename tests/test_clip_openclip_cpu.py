"""CPU: the weight blob's activation word (seesaw_amd/models/clip.py::pack_clip_weights) -- 0 for quick_gelu, 1 for gelu,
a quick-GELU blob unchanged to the byte, anything else refused before a device call."""
import hashlib
import struct

import pytest

# sha256 of the blob of ViT-B/32's configuration with one layer a tower, torch.manual_seed(1234), as packed by commit
# 38940e1 ("Pruned batched top-k: bound chunks on the packed 5-bit shadow"), the last one with a reserved zero word
PARENT_SHA256 = "6f70eda87cab1006f477951c2cc910c405d97f1e9e36f468099ee26f7919a79e"


def _model(act_v="quick_gelu", act_t="quick_gelu"):
    import torch
    import transformers
    torch.manual_seed(1234)
    cfg = transformers.CLIPConfig(text_config=dict(num_hidden_layers=1, hidden_act=act_t),
                                  vision_config=dict(num_hidden_layers=1, hidden_act=act_v))
    return transformers.CLIPModel(cfg).eval()


def test_quick_gelu_blob_is_the_parents_and_gelu_differs_in_one_word():
    from seesaw_amd.models.clip import pack_clip_weights
    quick, exact = _model(), _model("gelu", "gelu")
    a = pack_clip_weights(quick.state_dict(), quick.config)
    b = pack_clip_weights(exact.state_dict(), exact.config)
    assert hashlib.sha256(a.tobytes()).hexdigest() == PARENT_SHA256
    assert struct.unpack("<i", a[68:72].tobytes())[0] == 0 and struct.unpack("<i", b[68:72].tobytes())[0] == 1
    assert a[:68].tobytes() == b[:68].tobytes() and a[72:].tobytes() == b[72:].tobytes()  # same seed, same weights


@pytest.mark.parametrize("act_v,act_t", [("gelu", "quick_gelu"), ("quick_gelu", "gelu"), ("relu", "relu")])
def test_mixed_or_unknown_activations_and_header_codes_are_refused(act_v, act_t):
    import numpy as np
    from seesaw_amd.models.clip import ClipModel, pack_clip_weights
    m = _model(act_v, act_t)
    with pytest.raises(ValueError, match="activation|hidden_act"):
        pack_clip_weights(m.state_dict(), m.config)
    header = struct.pack("<8s6i7iifi", b"SSWCLIP1", 768, 1, 12, 3072, 224, 32, 512, 1, 8, 2048, 77, 49408, 2, 512, 1e-5, 2)
    with pytest.raises(ValueError, match="activation code 2"):  # before the library is called
        ClipModel(np.frombuffer(header + bytes(64), dtype=np.uint8))

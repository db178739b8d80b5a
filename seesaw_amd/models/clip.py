"""CLIP (ViT-B/32, ViT-B/16, ViT-L/14) on the GPU: weight packing + ctypes front of the ssw_clip_* entry points.

The reference loads `transformers.CLIPModel.from_pretrained(<local dir>)` and calls
`get_text_features` / `get_image_features` (seesaw/models/embeddings.py:427-455,
seesaw/models/model.py:50-63).  Here the same state_dict is flattened into one blob and the
forward pass runs in libseesaw_hip.so (bf16 MFMA GEMMs, f32 LayerNorm / softmax / residuals).
"""
from __future__ import annotations

import ctypes
import struct

import numpy as np

from .. import _lib

_LAYER_KEYS = ["layer_norm1.weight", "layer_norm1.bias", "self_attn.q_proj.weight", "self_attn.q_proj.bias",
               "self_attn.k_proj.weight", "self_attn.k_proj.bias", "self_attn.v_proj.weight", "self_attn.v_proj.bias",
               "self_attn.out_proj.weight", "self_attn.out_proj.bias", "layer_norm2.weight", "layer_norm2.bias",
               "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias"]


def patch_columns(patch_size: int) -> int:
    """Columns of a gathered patch row on the device: 3 patch^2 padded with zero columns to the next multiple of 64
    (csrc/clip.hip, patch_cols; patch 14: 588 -> 640).  The blob is not padded: ssw_clip_create pads the patch weight."""
    return -(-3 * patch_size * patch_size // 64) * 64


def pack_clip_weights(state_dict, config) -> np.ndarray:
    """transformers.CLIPModel state_dict + CLIPConfig -> the flat blob ssw_clip_create reads."""
    v, t = config.vision_config, config.text_config
    assert v.hidden_act == "quick_gelu" and t.hidden_act == "quick_gelu", "only quick_gelu CLIP variants"
    header = struct.pack("<8s6i7iifi", b"SSWCLIP1", v.hidden_size, v.num_hidden_layers, v.num_attention_heads,
                         v.intermediate_size, v.image_size, v.patch_size, t.hidden_size, t.num_hidden_layers,
                         t.num_attention_heads, t.intermediate_size, t.max_position_embeddings, t.vocab_size,
                         t.eos_token_id, config.projection_dim, float(v.layer_norm_eps), 0)
    assert len(header) == 72

    def get(name):
        x = state_dict[name]
        x = x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)
        return np.ascontiguousarray(x, dtype=np.float32).reshape(-1)

    parts = [get("vision_model.embeddings.class_embedding"), get("vision_model.embeddings.patch_embedding.weight"),
             get("vision_model.embeddings.position_embedding.weight"), get("vision_model.pre_layrnorm.weight"),
             get("vision_model.pre_layrnorm.bias")]
    for i in range(v.num_hidden_layers):
        parts += [get(f"vision_model.encoder.layers.{i}.{k}") for k in _LAYER_KEYS]
    parts += [get("vision_model.post_layernorm.weight"), get("vision_model.post_layernorm.bias"),
              get("visual_projection.weight"), get("text_model.embeddings.token_embedding.weight"),
              get("text_model.embeddings.position_embedding.weight")]
    for i in range(t.num_hidden_layers):
        parts += [get(f"text_model.encoder.layers.{i}.{k}") for k in _LAYER_KEYS]
    parts += [get("text_model.final_layer_norm.weight"), get("text_model.final_layer_norm.bias"),
              get("text_projection.weight")]
    body = np.concatenate(parts)
    blob = np.empty(72 + body.nbytes, dtype=np.uint8)
    blob[:72] = np.frombuffer(header, dtype=np.uint8)
    blob[72:] = body.view(np.uint8)
    return blob


class ClipModel:
    def __init__(self, blob: np.ndarray, device: int = 0):
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        self._h = ctypes.c_void_p()
        hdr = struct.unpack("<8s6i7iifi", blob[:72].tobytes())
        self.image_size, self.patch_size = hdr[5], hdr[6]
        self.vision_hidden, self.text_hidden = hdr[1], hdr[7]
        self.max_positions, self.vocab_size, self.eos_token_id, self.projection_dim = hdr[11], hdr[12], hdr[13], hdr[14]
        _lib.call("ssw_clip_create", int(device), ctypes.c_void_p(blob.ctypes.data), ctypes.c_size_t(blob.nbytes),
                  ctypes.byref(self._h))

    @classmethod
    def from_hf(cls, hf_model, device: int = 0) -> "ClipModel":
        return cls(pack_clip_weights(hf_model.state_dict(), hf_model.config), device=device)

    @classmethod
    def random_init(cls, seed: int = 1234, device: int = 0, config=None) -> "ClipModel":
        """BASELINE.json: 'random-init CLIP weights' -- transformers.CLIPModel(CLIPConfig()) under a seed.
        `config`: a transformers.CLIPConfig of another variant (ViT-B/16, ViT-L/14); default ViT-B/32."""
        import torch
        import transformers
        torch.manual_seed(seed)
        cfg = transformers.CLIPConfig() if config is None else config
        return cls.from_hf(transformers.CLIPModel(cfg).eval(), device=device)

    def close(self):
        if self._h:
            _lib.load().ssw_clip_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def embed_image(self, pixel_values: np.ndarray, normalize: bool = True) -> np.ndarray:
        x = np.ascontiguousarray(pixel_values, dtype=np.float32)
        assert x.ndim == 4 and x.shape[1:] == (3, self.image_size, self.image_size), x.shape
        out = np.empty((x.shape[0], self.projection_dim), dtype=np.float32)
        _lib.call("ssw_clip_embed_image", self._h, ctypes.c_void_p(x.ctypes.data), x.shape[0], int(normalize),
                  ctypes.c_void_p(out.ctypes.data))
        return out

    def embed_tiles_u8(self, tiles: np.ndarray, normalize: bool = True) -> np.ndarray:
        """uint8 HWC tiles [B, S, S, 3] straight from the tiler; batch_tx's normalisation runs on the GPU."""
        x = np.ascontiguousarray(tiles, dtype=np.uint8)
        assert x.ndim == 4 and x.shape[1:] == (self.image_size, self.image_size, 3), x.shape
        out = np.empty((x.shape[0], self.projection_dim), dtype=np.float32)
        _lib.call("ssw_clip_embed_tiles_u8", self._h, ctypes.c_void_p(x.ctypes.data), x.shape[0], int(normalize),
                  ctypes.c_void_p(out.ctypes.data))
        return out

    # What a call's sources, levels, intermediate rows and tables may take of the device (include/seesaw_hip.h,
    # SSW_CLIP_TILER_ARENA_BYTES); embed_multiscale_u8 splits its list so that every call stays under it.
    TILER_ARENA_BYTES = 1 << 30

    def tiler_bytes(self, shape, level_sizes) -> int:
        """An upper bound of what one [h, w, 3] image with these (w', h') levels takes of the arena (csrc/tiler.hip,
        tiler_plan): the source; per level its rows (pitch rounded up to 8 bytes) and the horizontal pass's intermediate
        rows, whether or not that pass runs; the tables -- (2 ceil(in / out) + 3) int32 coefficients an output row or
        column, two 56-byte jobs a level, a 24-byte descriptor a tile."""
        h, w, t = int(shape[0]), int(shape[1]), self.image_size
        total = h * w * 3 + 8
        for (lw, lh) in level_sizes:
            lw, lh = max(int(lw), 1), max(int(lh), 1)
            total += (lh + h) * (-(-lw * 3 // 8) * 8) + 16
            total += 4 * (lw * (2 * -(-w // lw) + 3) + lh * (2 * -(-h // lh) + 3)) + 2 * 56 + 24
            total += 24 * 4 * (lw // t) * (lh // t)
        return total

    def embed_multiscale_u8(self, images, plans, normalize: bool = True) -> np.ndarray:
        """Decoded images -> the vectors of their multiscale tiles, pyramid and tiling on the device
        (ssw_clip_embed_multiscale_u8).  images: list of [h, w, 3] uint8 arrays; plans: per image what
        multiscale_tools.multiscale_plan returned -- (levels, meta), levels with columns w, h -- or just the list of
        (w', h') level sizes.  -> [total tiles, projection_dim] f32 in tile order, image after image: row i belongs to
        row i of the concatenated meta frames."""
        if len(images) != len(plans):
            raise ValueError(f"{len(images)} images, {len(plans)} plans")
        arrays, sizes = [], []
        for i, (im, plan) in enumerate(zip(images, plans)):
            if not isinstance(im, np.ndarray) or im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] != 3:
                raise ValueError(f"image {i}: want a uint8 array [h, w, 3], got "
                                 f"{getattr(im, 'dtype', type(im).__name__)} {getattr(im, 'shape', '')}")
            levels = plan[0] if isinstance(plan, tuple) else plan
            if hasattr(levels, "columns"):
                levels = list(zip(levels["w"].tolist(), levels["h"].tolist()))
            arrays.append(np.ascontiguousarray(im))
            sizes.append([(int(w), int(h)) for (w, h) in levels])
        out, group, used = [], [], 0
        for i in range(len(arrays)):
            need = self.tiler_bytes(arrays[i].shape, sizes[i])
            if group and used + need > self.TILER_ARENA_BYTES:
                out.append(self._embed_multiscale_call([arrays[j] for j in group], [sizes[j] for j in group], normalize))
                group, used = [], 0
            group.append(i)
            used += need
        if group:
            out.append(self._embed_multiscale_call([arrays[j] for j in group], [sizes[j] for j in group], normalize))
        return np.concatenate(out) if out else np.zeros((0, self.projection_dim), np.float32)

    def _embed_multiscale_call(self, arrays, sizes, normalize):
        t, half = self.image_size, self.image_size // 2
        offsets = [0]
        for a in arrays:  # starts on multiples of 8 bytes: a level of the source's own size is then read in place
            offsets.append(-(-(offsets[-1] + a.size) // 8) * 8)
        buf = np.empty(max(offsets[-1], 1), np.uint8)
        for a, o in zip(arrays, offsets):
            buf[o:o + a.size] = a.reshape(-1)
        offsets = np.asarray(offsets, np.int64)
        hw = np.asarray([a.shape[:2] for a in arrays], np.int32).reshape(-1, 2)
        first = np.cumsum([0] + [len(s) for s in sizes]).astype(np.int32)
        wh = np.asarray([s for ls in sizes for s in ls], np.int32).reshape(-1, 2)
        cap = sum(max(h - sy, 0) // t * (max(w - sx, 0) // t) for ls in sizes for (w, h) in ls for sx in (0, half)
                  for sy in (0, half))
        out = np.empty((max(cap, 1), self.projection_dim), np.float32)
        n = ctypes.c_int64(0)
        _lib.call("ssw_clip_embed_multiscale_u8", self._h, ctypes.c_void_p(buf.ctypes.data), len(arrays),
                  ctypes.c_void_p(offsets.ctypes.data), ctypes.c_void_p(hw.ctypes.data), ctypes.c_void_p(first.ctypes.data),
                  ctypes.c_void_p(wh.ctypes.data), int(normalize), ctypes.c_void_p(out.ctypes.data), cap, ctypes.byref(n))
        return out[:n.value]

    def embed_image_dev(self, pixels_ptr: int, b: int, out_ptr: int, normalize: bool = True, stream_ptr: int = 0):
        _lib.call("ssw_clip_embed_image_dev", self._h, ctypes.c_void_p(stream_ptr) if stream_ptr else None,
                  ctypes.c_void_p(pixels_ptr), int(b), int(normalize), ctypes.c_void_p(out_ptr))

    def sync(self):
        _lib.call("ssw_clip_sync", self._h)

    # ssw_clip_set_option (include/seesaw_hip.h): per-handle form of the towers' tile path
    OPT_IMAGE_ROWS_BF16, OPT_TEXT_ROWS_BF16, OPT_ATTN_DIRECT, OPT_ATTN_OUT_UNFUSED, OPT_FULL_LAST_LAYER = 0, 1, 2, 3, 4
    OPT_ATTN_LONG = 6  # the long-sequence attention kernel for towers of <= 80 tokens too (5 is not an option)

    def set_option(self, option: int, value: bool):
        _lib.call("ssw_clip_set_option", self._h, int(option), int(bool(value)))

    def set_rows(self, image_bf16: bool = False, text_bf16: bool = False):
        """residual-row precision of the two towers' tile paths (default: f32 rows in both)"""
        self.set_option(self.OPT_IMAGE_ROWS_BF16, image_bf16)
        self.set_option(self.OPT_TEXT_ROWS_BF16, text_bf16)

    def embed_text(self, input_ids: np.ndarray, normalize: bool = False) -> np.ndarray:
        ids = np.ascontiguousarray(input_ids, dtype=np.int32)
        assert ids.ndim == 2
        out = np.empty((ids.shape[0], self.projection_dim), dtype=np.float32)
        _lib.call("ssw_clip_embed_text", self._h, ctypes.c_void_p(ids.ctypes.data), ids.shape[0], ids.shape[1],
                  int(normalize), ctypes.c_void_p(out.ctypes.data))
        return out

"""GPU: the CLIP towers of OpenCLIP ViT-H/14 and bigG/14 -- attention at head dims 80 / 88 / 104 (attention_hd, form 6
of ssw_debug_attention_run), rows wider than 1024, the exact GELU.

1. The kernel alone against an f64 softmax on the PEAKED input families of tests/test_attention_gpu.py, whose bit
   helpers are imported; its operands, reference and tolerance are written for 64 columns and are restated for HD:
   one-hot / two-hot rows (+-1 keys, query = 8 x its target key, integer V, scale 1/8: the target's logit is HD and the
   reference asserts it holds >= 1 - 2^-20 of the row) must come back BIT FOR BIT; peaked (q, k ~ N(0, 2^2)) and offset
   (+100 on every logit) rows within that file's derived tolerance, u = 2^-8:
       (1 + 2^-6) u (sum_j P_j |v_j| + |ref|)  +  1.01 sum_j P_j (eps_j + N) |v_j| + 288 2^-24 (1 + 2^-7) sum_j P_j |v_j|
       + S 2^-126 max |v|,   eps_j = (HD + 2) 2^-24 scale sum_d |q_d| |k_d| + |x_j| 2^-21 + 2^-22  (a logit is an f32 sum
       of HD exact products; the zero columns that pad it to a k-step add exact zeros),  N = sum_j P_j eps_j + (S + 4) 2^-24,
   with the f32 part asserted to be at most half the bf16 part.  H = 2 with values that differ by head; NaN guard rows
   behind qkv, NaN sentinels in out and its guard rows.
2. Towers against transformers' f32 model at tests/test_clip_variants_gpu.py's bar: seeded random init, 2 layers."""
import numpy as np
import pytest
from test_attention_gpu import OUT_GUARD, QKV_GUARD, SCALE, U, _bits, _finite, _p, _sentinel, _vals

pytestmark = pytest.mark.gpu
B, H = 3, 2
COS_MIN, ABS_MAX = 0.999, 5e-3
VOCAB, BOS, EOS = 1000, 998, 999


def _rows(x):
    """[B, H, S, HD] -> [B S, H HD]"""
    return np.ascontiguousarray(x.transpose(0, 2, 1, 3)).reshape(x.shape[0] * x.shape[2], -1)


def _run(lib, q, k, v, form=6, causal=0):
    """one launch -> (status, written rows as bf16 bits); a refused call must leave `out` as it was"""
    S, D = q.shape[2], q.shape[1] * q.shape[3]
    qkv = np.full((B * S + QKV_GUARD, 3 * D), 0x7FC0, dtype=np.uint16)
    qkv[:B * S] = _bits(np.concatenate([_rows(q), _rows(k), _rows(v)], axis=1))
    out = _sentinel((B * S + OUT_GUARD, D))
    before = out.copy()
    rc = lib.ssw_debug_attention_run(form, B, S, D, q.shape[1], causal, SCALE, _p(qkv), qkv.shape[0], _p(out), out.shape[0])
    assert np.array_equal(out[B * S if rc == 0 else 0:], before[B * S if rc == 0 else 0:]), "guard rows / a refused call wrote"
    assert rc != 0 or _finite(out[:B * S]), "NaN / inf / an unwritten element in the output"
    return rc, out[:B * S]


def _reference(q, k, v):
    """P, ref, tol [B, H, S, .] in f64 (module docstring)"""
    q, k, v = (a.astype(np.float64) for a in (q, k, v))
    S, HD = q.shape[2:]
    x = SCALE * (q @ k.transpose(0, 1, 3, 2))
    x -= x.max(axis=-1, keepdims=True)
    P = np.exp(x) / np.exp(x).sum(axis=-1, keepdims=True)
    ref, apv = P @ v, P @ np.abs(v)
    bf = (1 + 2.0 ** -6) * U * (apv + np.abs(ref))
    eps = (HD + 2) * 2.0 ** -24 * SCALE * (np.abs(q) @ np.abs(k).transpose(0, 1, 3, 2)) - x * 2.0 ** -21 + 2.0 ** -22
    N = (P * eps).sum(axis=-1, keepdims=True) + (S + 4) * 2.0 ** -24
    f32 = 1.01 * ((P * (eps + N)) @ np.abs(v)) + 288 * 2.0 ** -24 * (1 + 2.0 ** -7) * apv + S * 2.0 ** -126 * np.abs(v).max()
    assert (f32 <= 0.5 * bf).all(), ("f32 term above half the bf16 term: wrong inputs", float((f32 / bf).max()))
    return P, ref, bf + f32


@pytest.mark.parametrize("S", [1, 16, 17, 50, 257, 272])
@pytest.mark.parametrize("HD", [80, 88, 104])
def test_attention_hd_against_the_f64_softmax(lab_build, HD, S):
    lib, rng, shape = lab_build, np.random.default_rng(1000 * HD + S), (B, H, S, HD)
    k = rng.choice(np.float32([-1, 1]), shape)
    v = (rng.integers(1, 9, shape) * rng.choice([-1, 1], shape)).astype(np.float32)
    cases = [(k, v, (np.arange(S) + s) % S, None) for s in sorted({0, 1 % S, 17 % S, S - 1})]             # one-hot
    for a, b in ((0, S - 1), (15, 16)):                                                                   # two-hot
        if a < b < S:
            k2, v2 = k.copy(), v.copy()
            k2[:, :, b] = k2[:, :, a]
            v2[:, :, b] = np.where(v2[:, :, a] + v2[:, :, b] == 0, v2[:, :, a], v2[:, :, b])  # no zero in the expected row
            cases.append((k2, v2, np.full(S, a), b))
    for kk, vv, t, b in cases:
        P, _, _ = _reference(8 * kk[:, :, t], kk, vv)
        w = P[..., np.arange(S), t] + (P[..., b] if b is not None else 0)
        assert (w >= 1 - 2.0 ** -20).all() and (b is None or np.array_equal(P[..., t[0]], P[..., b])), "not peaked"
        rc, got = _run(lib, 8 * kk[:, :, t], kk, vv)
        assert rc == 0, lib.ssw_last_error().decode()
        want = vv[:, :, t] if b is None else 0.5 * (vv[:, :, t] + vv[:, :, b:b + 1])
        assert np.array_equal(got, _bits(_rows(want))), ("rows are not V[t(i)] / the pair's mean bit for bit", HD, S, b)
    for offset in (False, True):                                                                          # peaked, offset
        q, kk = (_vals(_bits(2 * rng.standard_normal(shape))) for _ in range(2))
        vv = _vals(_bits(rng.standard_normal(shape)))
        if offset:
            q[..., HD - 1], kk[..., HD - 1] = 16, 50
        _, ref, tol = _reference(q, kk, vv)
        rc, got = _run(lib, q, kk, vv)
        assert rc == 0, lib.ssw_last_error().decode()
        d = np.abs(_vals(got).astype(np.float64) - _rows(ref)) / _rows(tol)
        print(f"HD {HD} S {S} offset {offset}: max |got - ref| / tol = {float(d.max()):.3f}")
        assert (d <= 1).all(), (HD, S, offset, float(d.max()))


def test_form_6_has_no_causal_form_and_the_other_forms_no_head_dim_80(lab_build):
    q = np.ones((B, H, 16, 80), dtype=np.float32)
    assert _run(lab_build, q, q, q, form=6, causal=1)[0] == -4 and lab_build.ssw_last_error()
    assert [_run(lab_build, q, q, q, form=f)[0] for f in range(6)] == [-4] * 6
    assert _run(lab_build, q, q, q)[0] == 0  # and the library serves the next call


TOWERS = {  # vision hidden / heads / MLP, projection, text hidden / heads / MLP, activation
    "hd80_640": ((640, 8, 1280), 512, (512, 8, 2048), "gelu"),            # head dim 80 inside the old width limit; skinny text
    "vit_h14": ((1280, 16, 5120), 1024, (128, 2, 128), "gelu"),           # ViT-H/14's layer
    "vit_h14_quick": ((1280, 16, 5120), 1024, (128, 2, 128), "quick_gelu"),
    "bigg14": ((1664, 16, 8192), 1280, (1280, 20, 5120), "gelu"),         # bigG/14's layers, both towers
}
_CACHE = {}


def _pair(name):
    if name not in _CACHE:
        import torch
        import transformers
        from seesaw_amd.models.clip import ClipModel
        (vh, vn, vm), proj, (th, tn, tm), act = TOWERS[name]
        cfg = transformers.CLIPConfig(
            text_config=dict(hidden_size=th, num_attention_heads=tn, intermediate_size=tm, num_hidden_layers=2, vocab_size=VOCAB,
                             bos_token_id=BOS, eos_token_id=EOS, pad_token_id=0, max_position_embeddings=77, hidden_act=act),
            vision_config=dict(hidden_size=vh, num_attention_heads=vn, intermediate_size=vm, num_hidden_layers=2,
                               image_size=224, patch_size=14, hidden_act=act), projection_dim=proj)
        torch.manual_seed(4321)
        hf = transformers.CLIPModel(cfg).eval()
        _CACHE[name] = (hf, ClipModel.from_hf(hf))
    return _CACHE[name]


def _at_the_bar(got, ref, what):
    ref = (ref.pooler_output if hasattr(ref, "pooler_output") else ref).numpy()
    got, ref = (x / np.linalg.norm(x, axis=-1, keepdims=True) for x in (got, ref))
    cos, err = (got * ref).sum(1), float(np.abs(got - ref).max())
    print(f"{what}: min cosine {cos.min():.6f}, max |delta| {err:.2e}")
    assert np.isfinite(got).all() and cos.min() >= COS_MIN and err <= ABS_MAX, (what, cos, err)


@pytest.mark.parametrize("name", list(TOWERS))
def test_image_tower_vs_hf(name):
    import torch
    hf, ours = _pair(name)
    x = np.random.default_rng(5).standard_normal((3, 3, 224, 224), dtype=np.float32)
    with torch.inference_mode():
        ref = hf.get_image_features(pixel_values=torch.from_numpy(x))
    got = ours.embed_image(x, normalize=True)
    assert got.shape == (3, TOWERS[name][1]) and np.abs(got[0] - got[1]).max() > 1e-3
    _at_the_bar(got, ref, name)


@pytest.mark.parametrize("name", ["hd80_640", "bigg14"])
@pytest.mark.parametrize("n,L", [(4, 77), (1, 9)])
def test_text_tower_vs_hf(name, n, L):
    import torch
    hf, ours = _pair(name)
    ids = np.random.default_rng(6).integers(1, BOS - 1, size=(n, L)).astype(np.int32)
    ids[:, 0], ids[:, L - 1] = BOS, EOS
    with torch.inference_mode():
        ref = hf.get_text_features(input_ids=torch.from_numpy(ids.astype(np.int64)))
    _at_the_bar(ours.embed_text(ids, normalize=False), ref, f"{name} text {n} x {L}")

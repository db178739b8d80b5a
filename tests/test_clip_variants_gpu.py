"""GPU: CLIP image towers beyond ViT-B/32 (attention_long up to 272 tokens, the patch gather for any patch size), and the
text tower at hidden 768, against transformers.CLIPModel (f32, torch-CPU) with seeded random-init weights.

Oracle and bar are tests/test_clip_gpu.py's: on L2-normalised outputs cosine >= 0.999 and
max |delta| <= 5e-3 a component.  Every model is reduced to 2 layers a tower (quick_gelu) and a call holds 2-3 tiles, so
that a test takes seconds; the widths and token counts are the real ones where they select a kernel."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
COS_MIN = 0.999
ABS_MAX = 5e-3
VOCAB, BOS, EOS = 1000, 998, 999  # a small vocabulary: the token table is not what these tests are about


def _config(image, patch, v_hidden, v_heads, v_mlp, t_hidden=128, t_heads=2, t_mlp=128, proj=512, layers=2):
    import transformers
    return transformers.CLIPConfig(
        text_config=dict(hidden_size=t_hidden, num_attention_heads=t_heads, intermediate_size=t_mlp,
                         num_hidden_layers=layers, vocab_size=VOCAB, bos_token_id=BOS, eos_token_id=EOS, pad_token_id=0,
                         max_position_embeddings=77, hidden_act="quick_gelu"),
        vision_config=dict(hidden_size=v_hidden, num_attention_heads=v_heads, intermediate_size=v_mlp,
                           num_hidden_layers=layers, image_size=image, patch_size=patch, hidden_act="quick_gelu"),
        projection_dim=proj)


CONFIGS = {
    # token count -> (image, patch) at vision hidden 256, 4 heads
    "s82": dict(image=126, patch=14, v_hidden=256, v_heads=4, v_mlp=512),    # first S on attention_long, instance 13
    "s197": dict(image=224, patch=16, v_hidden=256, v_heads=4, v_mlp=512),   # tail of 5 rows
    "s257": dict(image=224, patch=14, v_hidden=256, v_heads=4, v_mlp=512),   # tail of 1 row, instance 17
    "b16": dict(image=224, patch=16, v_hidden=768, v_heads=12, v_mlp=3072, proj=512),   # ViT-B/16's widths
    "l14": dict(image=224, patch=14, v_hidden=1024, v_heads=16, v_mlp=4096, proj=768,   # ViT-L/14's widths, both towers
                t_hidden=768, t_heads=12, t_mlp=3072),
}
_CACHE = {}


def _pair(name):
    """(HF model, ours) of a config, built once a session under a fixed seed"""
    if name not in _CACHE:
        import torch
        import transformers
        from seesaw_amd.models.clip import ClipModel
        torch.manual_seed(4321)
        hf = transformers.CLIPModel(_config(**CONFIGS[name])).eval()
        _CACHE[name] = (hf, ClipModel.from_hf(hf))
    return _CACHE[name]


@pytest.fixture(scope="module")
def vit_b32():
    import torch
    import transformers
    from seesaw_amd.models.clip import ClipModel
    torch.manual_seed(1234)
    ours = ClipModel.from_hf(transformers.CLIPModel(transformers.CLIPConfig()).eval())
    yield ours
    ours.close()


def _unit(x):
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


def _hf_image(hf, x):
    import torch
    with torch.inference_mode():
        ref = hf.get_image_features(pixel_values=torch.from_numpy(x))
        ref = ref.pooler_output if hasattr(ref, "pooler_output") else ref
        return _unit(ref.numpy())


def _hf_text(hf, ids):
    import torch
    with torch.inference_mode():
        ref = hf.get_text_features(input_ids=torch.from_numpy(ids.astype(np.int64)))
        return (ref.pooler_output if hasattr(ref, "pooler_output") else ref).numpy()


def _at_the_bar(got, ref, what):
    cos = (got * ref).sum(1)
    err = float(np.abs(got - ref).max())
    print(f"{what}: min cosine {cos.min():.6f}, max |delta| {err:.2e}")
    assert np.isfinite(got).all(), what
    assert cos.min() >= COS_MIN, (what, cos)
    assert err <= ABS_MAX, (what, err)


def _pixels(name, n, seed):
    image = CONFIGS[name]["image"]
    return np.random.default_rng(seed).standard_normal((n, 3, image, image), dtype=np.float32)


@pytest.mark.parametrize("name,tokens", [("s82", 82), ("s197", 197), ("s257", 257), ("b16", 197), ("l14", 257)])
def test_image_tower_vs_hf(name, tokens):
    hf, ours = _pair(name)
    cfg = CONFIGS[name]
    assert (cfg["image"] // cfg["patch"]) ** 2 + 1 == tokens
    x = _pixels(name, 3, seed=tokens)
    got = ours.embed_image(x, normalize=True)
    assert got.shape == (3, cfg.get("proj", 512))
    assert np.abs(np.linalg.norm(got, axis=1) - 1).max() < 1e-5
    _at_the_bar(got, _hf_image(hf, x), name)
    assert np.abs(got[0] - got[1]).max() > 1e-3  # different tiles, different vectors


def test_both_row_precisions_at_vit_l14_widths():
    hf, ours = _pair("l14")
    x = _pixels("l14", 2, seed=7)
    ref = _hf_image(hf, x)
    got = {}
    try:
        for bf16 in (False, True):
            ours.set_rows(image_bf16=bf16)
            got[bf16] = ours.embed_image(x, normalize=True)
    finally:
        ours.set_rows()
    for bf16, g in got.items():
        _at_the_bar(g, ref, f"l14, bf16 rows {bf16}")
    assert np.abs(got[False] - got[True]).max() > 0  # the switch is live


def test_attention_long_gives_the_bits_of_the_existing_attention(vit_b32):
    """the test that pins attention_long's arithmetic: on ViT-B/32, where both serve the sequence, the embeddings are the
    same bytes -- the image tower at S = 50 (attention_rows64 against instance 4, attention as a launch of its own), the
    text tower's batched causal tile path at 16 x 77 tokens (attention_mfma<5> against instance 5)"""
    ours = vit_b32
    x = np.random.default_rng(21).standard_normal((9, 3, 224, 224), dtype=np.float32)
    rng = np.random.default_rng(22)
    ids = rng.integers(0, 49405, size=(16, 77)).astype(np.int32)
    ids[:, 0] = 49406
    for b in range(16):
        ids[b, rng.integers(2, 77) if b else 76] = 49407
    try:
        ours.set_option(ours.OPT_ATTN_OUT_UNFUSED, True)
        a = ours.embed_image(x, normalize=False)
        ta = ours.embed_text(ids, normalize=False)
        ours.set_option(ours.OPT_ATTN_LONG, True)
        b = ours.embed_image(x, normalize=False)
        tb = ours.embed_text(ids, normalize=False)
    finally:
        ours.set_option(ours.OPT_ATTN_LONG, False)
        ours.set_option(ours.OPT_ATTN_OUT_UNFUSED, False)
    assert np.isfinite(a).all() and np.abs(a).max() > 0
    assert a.tobytes() == b.tobytes()
    assert np.isfinite(ta).all() and np.abs(ta).max() > 0
    assert ta.tobytes() == tb.tobytes()


def test_patch14_u8_tiles_equal_host_batch_tx_path():
    """the general patch gather's uint8 form keeps batch_tx's arithmetic: the same bits as normalising on the host"""
    import pandas as pd
    from seesaw_amd.indices.multiscale.multiscale_tools import batch_tx
    _, ours = _pair("s257")
    tiles = np.random.default_rng(4).integers(0, 256, size=(3, 224, 224, 3), dtype=np.uint8)
    host = np.stack(batch_tx(pd.DataFrame({"tile": list(tiles)})).tile.values)
    a = ours.embed_image(host, normalize=True)
    b = ours.embed_tiles_u8(tiles, normalize=True)
    assert np.isfinite(a).all()
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_a_tiles_vector_does_not_depend_on_the_tiles_that_share_its_call():
    _, ours = _pair("s257")
    x = _pixels("s257", 5, seed=31)
    whole = ours.embed_image(x, normalize=True)
    for i in (0, 3, 4):
        alone = ours.embed_image(x[i:i + 1], normalize=True)
        assert alone.tobytes() == whole[i:i + 1].tobytes(), i


def _text_ids(rng, B, L):
    ids = rng.integers(1, BOS - 1, size=(B, L)).astype(np.int32)
    ids[:, 0] = BOS
    ids[:, L - 1] = EOS
    if B > 1 and L > 4:
        ids[B - 1, L - 2] = EOS  # an earlier EOS in the last row: pooled there
    return ids


@pytest.mark.parametrize("B,L", [(5, 8), (5, 77), (1, 9)])
def test_text_tower_at_hidden_768_vs_hf(B, L):
    """ViT-L/14's text tower (hidden 768, 12 heads, MLP 3072, projection 768): no skinny path at that width, so the
    batched calls and the single query all take the causal tile path"""
    hf, ours = _pair("l14")
    ids = _text_ids(np.random.default_rng(100 * B + L), B, L)
    ref = _hf_text(hf, ids)
    got = ours.embed_text(ids, normalize=False)
    assert got.shape == (B, 768)
    _at_the_bar(_unit(got), _unit(ref), f"text 768, {B} x {L}")
    assert np.abs(np.linalg.norm(got, axis=1) / np.linalg.norm(ref, axis=1) - 1).max() < 2e-2
    if B == 1:
        again = ours.embed_text(ids, normalize=False)
        assert got.tobytes() == again.tobytes()


def test_a_577_token_tower_is_refused_and_the_library_goes_on(vit_b32):
    import torch
    import transformers
    from seesaw_amd import _lib
    from seesaw_amd.models.clip import ClipModel, pack_clip_weights
    torch.manual_seed(1)
    cfg = _config(image=336, patch=14, v_hidden=256, v_heads=4, v_mlp=512)
    blob = pack_clip_weights(transformers.CLIPModel(cfg).state_dict(), cfg)
    with pytest.raises(_lib.SeesawHipError) as e:
        ClipModel(blob)
    assert e.value.status == _lib.SSW_ERR_UNSUPPORTED and "272" in str(e.value)
    torch.manual_seed(1234)
    fresh = ClipModel.from_hf(transformers.CLIPModel(transformers.CLIPConfig(
        text_config=dict(num_hidden_layers=1), vision_config=dict(num_hidden_layers=1))).eval())  # ViT-B/32's shapes
    try:
        x = np.random.default_rng(3).standard_normal((2, 3, 224, 224), dtype=np.float32)
        out = fresh.embed_image(x, normalize=True)
        assert out.shape == (2, 512) and np.abs(np.linalg.norm(out, axis=1) - 1).max() < 1e-5
    finally:
        fresh.close()
    assert vit_b32.embed_image(x, normalize=True).shape == (2, 512)  # and so does a handle from before the refusal


def test_create_multiscale_index_round_trip_at_dim_768(tmp_path):
    """image bytes -> tiles -> the ViT-L/14-width towers -> a dim-768 index on disk -> MultiscaleIndex -> a text query from
    the same model: the top hit's score is the dot product of the saved vectors, to f32 rounding of a 768-term sum"""
    import io
    import pandas as pd
    import PIL.Image
    from seesaw_amd.indices.multiscale.multiscale_index import MultiscaleIndex
    from seesaw_amd.indices.multiscale.multiscale_tools import create_multiscale_index, read_vector_parquet
    _, model = _pair("l14")
    rng = np.random.default_rng(9)
    rows = []
    for dbidx, (w, h) in enumerate([(300, 240), (224, 224), (260, 230)]):
        buf = io.BytesIO()
        PIL.Image.fromarray(rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)).save(buf, format="PNG")
        rows.append({"dbidx": dbidx, "file_path": f"img{dbidx}.png", "bytes": buf.getvalue()})
    path = create_multiscale_index(image_rows=pd.DataFrame(rows), dataset_path=str(tmp_path), index_name="l14",
                                   model=model, model_path=None)
    meta, vecs = read_vector_parquet(f"{path}/vectors.sorted.cached")
    assert vecs.dtype == np.float32 and vecs.shape == (meta.shape[0], 768) and meta.shape[0] >= 3
    assert np.abs(np.linalg.norm(vecs, axis=1) - 1).max() < 1e-5
    idx = MultiscaleIndex.from_path(path, use_vec_index=False)
    assert idx.vectors.shape == vecs.shape and len(idx) == 3
    q = _unit(model.embed_text(_text_ids(np.random.default_rng(2), 1, 6), normalize=False)).astype(np.float32)
    res = idx.query(vector=q, topk=1, shortlist_size=3, agg_method="plain_score", aug_larger="greater",
                    rescore_method="plain")
    assert len(res["dbidxs"]) == 1
    got = float(res["activations"][0].score.iloc[0])
    exact = vecs.astype(np.float64) @ q.reshape(-1).astype(np.float64)
    bound = 768 * 2.0 ** -24 * float((np.abs(vecs.astype(np.float64)) @ np.abs(q.reshape(-1).astype(np.float64))).max())
    assert abs(got - exact.max()) <= bound, (got, exact.max(), bound)
    assert int(res["dbidxs"][0]) == int(meta.dbidx.values[int(np.argmax(exact))])

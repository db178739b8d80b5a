"""CPU: the chunk-selection setting's plumbing -- the header, the bindings and the built library agree on its two
symbols, `index_options={"chunk_select": True}` reaches the device index's `chunk_select` through `AccessMethod.load`,
and SessionGroup keeps the setting off unless its constant says otherwise."""
import json
import types

import numpy as np
import pandas as pd
import pytest


def test_symbols_agree():
    from seesaw_amd import _lib
    lib = _lib.load()
    for name in ("ssw_index_set_chunk_select", "ssw_index_chunk_select_stats"):
        assert name in _lib.declared_symbols() and name in _lib._SIGNATURES
        assert getattr(lib, name) is not None


class _Dev:
    """what the index classes and SessionGroup touch of a DeviceIndex"""
    chunk_select, parent, is_view = False, None, False

    @classmethod
    def from_numpy(cls, vectors, **_):
        return cls()

    def set_tile_meta(self, *_):
        pass


@pytest.mark.parametrize("constructor", ["seesaw_amd.indices.coarse.coarse_index.CoarseIndex",
                                         "seesaw_amd.indices.multiscale.multiscale_index.MultiscaleIndex"])
@pytest.mark.parametrize("options,want", [({"chunk_select": True}, True), ({}, False)])
def test_index_options_reach_the_device_index(tmp_path, monkeypatch, constructor, options, want):
    from seesaw_amd.indices import interface
    from seesaw_amd.indices.coarse import coarse_index
    from seesaw_amd.indices.multiscale import multiscale_index
    from seesaw_amd.models import embeddings
    monkeypatch.setattr(coarse_index, "DeviceIndex", _Dev)
    monkeypatch.setattr(multiscale_index, "DeviceIndex", _Dev)
    monkeypatch.setattr(embeddings, "load_embedding", lambda *a, **k: None)
    json.dump({"constructor": constructor, "model": None}, open(tmp_path / "info.json", "w"))
    np.save(tmp_path / "vectors.npy", np.eye(4, 512, dtype=np.float32))
    pd.DataFrame({"dbidx": np.arange(4), "zoom_level": 0, "x1": 0.0, "y1": 0.0, "x2": 1.0, "y2": 1.0}).to_parquet(
        tmp_path / "vector_meta.parquet")
    index = interface.AccessMethod.load(str(tmp_path), options=options)
    assert index._dev.chunk_select is want


@pytest.mark.parametrize("constant,want", [(None, False), (True, True)])
def test_session_group_constant(monkeypatch, constant, want):
    from seesaw_amd.seesaw_session import SessionGroup
    assert SessionGroup.CHUNK_SELECT is None
    monkeypatch.setattr(SessionGroup, "CHUNK_SELECT", constant)
    parent, view = _Dev(), _Dev()
    view.parent = parent
    devs = [view, _Dev(), None]  # a view, a plain index, an index without a whole-matrix device index
    sessions = [types.SimpleNamespace(loop=types.SimpleNamespace(q=types.SimpleNamespace(index=types.SimpleNamespace(_dev=d))))
                for d in devs]
    SessionGroup(sessions)
    assert [d.chunk_select for d in (view, parent, devs[1])] == [want] * 3

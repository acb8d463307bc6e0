"""CPU: the forward-only drivers (ggpm_encoder_infer, ggpm_tree_level_infer) are declared, bound and exported, and their
arenas are a fraction of what the training forward keeps for the backward on the benchmark's batch shapes."""
import ctypes
import os
import re

import pytest

from ggpm_amd import _lib, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["ggpm_encoder_infer_bytes", "ggpm_encoder_infer", "ggpm_tree_level_infer_floats", "ggpm_tree_level_infer",
       "ggpm_decode_steps_infer", "ggpm_decode_steps_infer_async"]

# bench.py CONFIGS[1] / [4]: (hidden, depth, motifs per molecule, motif / attachment vocabulary); 32 molecules
SHAPES = {"configs1": (300, 20, (8, 12)), "configs4": (600, 30, (46, 58))}


def test_new_entry_points_are_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ggpm_hip.h")).read(), flags=re.S)
    lib = _lib.load()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name


def _enc_dims(key, lstm=False):
    from ggpm_amd.fused import EncDims, GATE_DTYPES
    H, depth, motifs = SHAPES[key]
    tree, graph = synth.tensorize(synth.random_batch(1000, 32, motifs=motifs, n_motif_vocab=500, n_attach_vocab=1500))
    return EncDims(H, H, depth, depth, 38, 500, 1500, graph[0].shape[0], graph[1].shape[0], graph[2].shape[1],
                   graph[3].shape[1], tree[0].shape[0], tree[1].shape[0], tree[2].shape[1], tree[3].shape[1],
                   tree[4].shape[1], 32, int(lstm), 0, 0.0, 0, 0, GATE_DTYPES["f32"])


@pytest.mark.parametrize("lstm", [False, True])
@pytest.mark.parametrize("key", sorted(SHAPES))
def test_encoder_infer_arena_is_an_eighth_of_the_saved_arena(key, lstm):
    lib = _lib.load()
    dims = _enc_dims(key, lstm)
    saved = int(lib.ggpm_encoder_saved_bytes(ctypes.byref(dims)))
    infer = int(lib.ggpm_encoder_infer_bytes(ctypes.byref(dims)))
    assert 0 < infer and infer * 8 <= saved, (key, infer, saved)


@pytest.mark.parametrize("lstm", [False, True])
def test_tree_level_infer_arena_drops_the_stashes(lstm):
    """Decoder tree-side levels on the configs[1] batch: diterT = 1 (every shipped configuration) and a deep level."""
    from ggpm_amd.tree_decode import TreeLevelC
    lib = _lib.load()
    tree, _ = synth.tensorize(synth.random_batch(1000, 32, motifs=SHAPES["configs1"][2], n_motif_vocab=500,
                                                 n_attach_vocab=1500))
    for depth in (1, 20):
        L = TreeLevelC()
        L.lstm, L.H, L.He, L.E1, L.n_extra, L.depth, L.n_inst = int(lstm), 300, 300, tree[1].shape[0], 0, depth, \
            tree[0].shape[0]
        saved = int(lib.ggpm_tree_level_saved_floats(ctypes.byref(L)))
        infer = int(lib.ggpm_tree_level_infer_floats(ctypes.byref(L)))
        assert 0 < infer < saved, (depth, infer, saved)
        if depth == 20:
            assert infer * 8 <= saved, (depth, infer, saved)

"""CPU: the two entries of the large-batch top-k on the matrix cores are declared and bound, and the batch entry takes
exactly ssw_index_topk_batch's arguments."""
from seesaw_amd import _lib


def test_matrix_core_entries_are_declared_and_bound_like_the_plain_batch():
    declared = _lib.declared_symbols()
    assert {"ssw_index_topk_batch_mc", "ssw_index_topk_batch_mc_stats"} <= set(declared) & set(_lib._SIGNATURES)
    assert _lib._SIGNATURES["ssw_index_topk_batch_mc"] == _lib._SIGNATURES["ssw_index_topk_batch"]

"""CPU checks of the gallery search's host side: recall_from_topn on hand-written lists, and the C-ABI entry of the select
kernel as hmmc_amd/_lib.py derives it from include/hmmc_hip.h (tests/test_abi.py holds header, exports and ctypes together)."""
import pytest
import torch

from hmmc_amd import _lib
from hmmc_amd import metrics as M


def test_recall_from_topn_on_hand_written_lists():
    # the diagonal target of query q is q; -1 = an empty slot
    lists = torch.tensor([[0, 7, 8, 9, 5, 6],        # at position 0: counts for every K
                          [9, 8, 7, 6, 1, 5],        # at position 4 = K - 1 for K = 5
                          [9, 8, 7, 6, 5, 2],        # at position 5 = K for K = 5: misses R5, counts for R6
                          [9, 8, 7, 6, 5, -1]])      # absent
    assert M.recall_from_topn(lists, ks=(1, 5, 6)) == {"R1": 25.0, "R5": 50.0, "R6": 75.0}
    assert M.recall_from_topn(lists, ks=(4,)) == {"R4": 25.0}
    target = torch.tensor([7, 9, 9, -1], dtype=torch.int32)
    assert M.recall_from_topn(lists, target=target, ks=(1, 2, 6)) == {"R1": 50.0, "R2": 75.0, "R6": 100.0}
    assert M.recall_from_topn(lists.int(), ks=(1,)) == {"R1": 25.0}
    with pytest.raises(ValueError, match="R10"):
        M.recall_from_topn(lists)                    # the default ks reach 10, the lists hold 6
    with pytest.raises(ValueError):
        M.recall_from_topn(lists, ks=(1, 7))


def test_topn_select_signature_follows_the_header():
    # const float*, int, int, long, int, float*, int*, int, int, hmmc_stream_t -> int
    assert _lib.SIGNATURES["hmmc_topn_select"] == ("piilippiip", "i")
    assert _lib.TOPN_MAX == 128
    from hmmc_amd import ops
    assert ops.TOPN_MAX == 128 and callable(ops.topn_select)


def test_default_chunk_meets_the_scorer_dma_conditions():
    from hmmc_amd.search import Gallery
    for P, E in ((16, 512), (32, 512), (16, 32), (32, 1024)):
        nv = Gallery.max_chunk_videos(P, E)
        for n, ok in ((nv, True), (nv + 1, False)):
            assert (n * P * E * 4 + 64 * E * 4 < 2 ** 31 and n * P < 2 ** 31) is ok, (P, E, n)

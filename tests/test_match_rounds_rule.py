"""The round rule of k_mp_rounds against the sequential reference loop, in numpy (no GPU): rounds on lists thinned by the drop rule of k_mp_candidates, with
the early finish, give the claims of the loop that serves one map point after the other -- and the variant that posts only on claimable entries does not.

The lists come from tests/roundgen.py (what k_mp_candidates caches), the sequential loop on them is held equal to the oracle's map search."""
import numpy as np
import pytest

import crowdgen as G
import orc
import roundgen as RG

N_RANDOM = 200
UNSOUND_SEEDS = (0, 28, 31)      # near_scene seeds on which restricted posting gives a wrong claim (nnratio 0.8)


def _obs(s):
    return s["mp"].get("obs_positive")


def _check(s, nn, what):
    lists = RG.lists_of(s, RG.TH)
    seq = RG.sequential(lists, s["init"], _obs(s), nn)
    got, n_rounds, _ = RG.rounds(lists, s["init"], _obs(s), nn)
    assert np.array_equal(got, seq), (what, nn)
    return lists, seq, n_rounds


def test_drop_rule_is_monotone_and_decides_nothing():
    """for every nnratio: a dropped distance is above TH_HIGH, every larger one is dropped too, and as a second-best of the same level it rejects no
    admissible best -- the same answer as no second-best (256, level -1)"""
    for nn in RG.NNRATIOS + (-0.5, 0.5, 1.5, float("nan")):
        gone = [d for d in range(257) if RG.dropped(d, nn)]
        assert all(d > RG.TH_HIGH for d in gone) and gone == list(range(257 - len(gone), 257)), nn
        if nn <= 0:
            assert not gone, nn
        for d in gone:
            for best in range(RG.TH_HIGH + 1):
                assert RG._accept(best, 1, d, 1, nn) and RG._accept(best, 1, 256, -1, nn), (nn, best, d)


def test_sequential_on_lists_is_the_oracle():
    for s, nn in [(RG.near_scene(k), 0.8) for k in range(8)] + [(RG.hand_scene(nn), nn) for nn in RG.NNRATIOS] + [(G.chain_map(77, 48), 0.8)]:
        lists = RG.lists_of(s, RG.TH)
        ref, _ = orc.search_by_projection_map(s["kps"], s["desc"], s["uright"], s["scale"], s["bounds"], s["mp"], RG.TH, nn, s["init"])
        assert np.array_equal(RG.sequential(lists, s["init"], _obs(s), nn), ref), nn


def test_rounds_with_drop_on_random_crowded_scenes():
    """200 crowded scenes whose distances cluster around TH_HIGH and the drop boundary; the scenes do make the rule work: entries are dropped, map points wait"""
    dropped = waited = 0
    for k in range(N_RANDOM):
        nn = RG.NNRATIOS[k % 4] if k % 10 else 0.0
        s = RG.near_scene(k)
        lists, _, n_rounds = _check(s, nn, k)
        dropped += sum(RG.dropped(d, nn) for L in lists for _, d, _ in L)
        waited += n_rounds > 2
    assert dropped > 1000 and waited > N_RANDOM // 2


@pytest.mark.parametrize("nn", RG.NNRATIOS)
def test_rounds_with_drop_on_hand_made_cases(nn):
    s = RG.hand_scene(nn)
    _, seq, _ = _check(s, nn, "hand")
    assert (seq >= 0).sum() > 10


def test_rounds_with_drop_on_a_chain():
    """48 map points with one window: one decision per round without the drop; with it still the sequential claims"""
    s = G.chain_map(77, 48)
    lists, _, _ = _check(s, 0.8, "chain")
    assert RG.rounds(lists, s["init"], _obs(s), 0.8, drop=False)[1] >= 40


def test_restricted_posting_is_unsound():
    """posting only on entries with distance <= TH_HIGH lets a later map point take an earlier one's second-best before that one decides"""
    wrong = 0
    for k in UNSOUND_SEEDS:
        s = RG.near_scene(k)
        lists = RG.lists_of(s, RG.TH)
        seq = RG.sequential(lists, s["init"], _obs(s), 0.8)
        assert np.array_equal(RG.rounds(lists, s["init"], _obs(s), 0.8)[0], seq)
        wrong += not np.array_equal(RG.rounds(lists, s["init"], _obs(s), 0.8, restricted=True)[0], seq)
    assert wrong >= 1

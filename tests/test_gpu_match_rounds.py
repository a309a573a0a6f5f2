"""GPU parity of the local-map search on the scenes of tests/roundgen.py: the drop rule of k_mp_candidates, the dense lists, and k_mp_rounds with its lists in
LDS, with all of them left in the pool (PLF_MATCH_ROUNDS_LDS=0), and with only the middle frame of three left there -- bit-exact against the oracle.
The last-frame search (k_lf_candidates / k_lf_rounds) on descriptors that put many entries above TH_HIGH.

PLF_MATCH_ROUNDS_LDS is read when a matcher is created: the tests set it before they construct theirs."""
import numpy as np
import pytest

import crowdgen as G
import roundgen as RG
from test_gpu_match_crowded import STRIDE, DevFrame, _check_last, _check_map, _dev, _dev_last, _last_calls, _last_refs, _map_call, _need_gpu

pytestmark = pytest.mark.gpu

BUDGETS = [None, "0"]
BUDGET_IDS = ["lists_in_lds", "lists_in_pool"]


def _matcher(monkeypatch, budget, max_batch=1):
    from rgbd_pl_slam_amd import Matcher
    if budget is not None:
        monkeypatch.setenv("PLF_MATCH_ROUNDS_LDS", str(budget))
    return Matcher(max_keypoints=STRIDE, max_mappoints=G.CACHED_MAX_MAPPOINTS, max_batch=max_batch)


@pytest.mark.parametrize("budget", BUDGETS, ids=BUDGET_IDS)
@pytest.mark.parametrize("nn", RG.NNRATIOS)
def test_hand_made_cases(monkeypatch, nn, budget):
    """best at TH_HIGH and TH_HIGH + 1, second-bests on either side of the drop boundary, a map point with nothing kept, a best that rises above TH_HIGH,
    ties, claims without observations, entries set before the call, a window of two walk chunks (roundgen.hand_scene)"""
    _need_gpu()
    s = RG.hand_scene(nn)
    m = _matcher(monkeypatch, budget)
    d = DevFrame(s); dmp = {k: _dev(v) for k, v in s["mp"].items()}
    _check_map(_map_call(m, [d], dmp, [s], RG.TH, nn), [s], s["mp"], RG.TH, nn, "hand")
    m.close()


@pytest.mark.parametrize("budget", BUDGETS, ids=BUDGET_IDS)
def test_crowded_scenes_and_a_chain(monkeypatch, budget):
    """distances around TH_HIGH and the drop boundary under contention, and 48 map points on one window"""
    _need_gpu()
    m = _matcher(monkeypatch, budget)
    for s, nn in [(RG.near_scene(k), RG.NNRATIOS[k % 4]) for k in (0, 28, 31, 5)] + [(RG.near_scene(7, n=300, m=3000), 0.8), (G.chain_map(77, 48), 0.8)]:
        d = DevFrame(s); dmp = {k: _dev(v) for k, v in s["mp"].items()}
        _check_map(_map_call(m, [d], dmp, [s], RG.TH, nn), [s], s["mp"], RG.TH, nn, "near")
    m.close()


def test_only_the_middle_frame_leaves_its_lists_in_the_pool(monkeypatch):
    """three frames against one map, the budget between the entries the outer frames keep and those of the middle one"""
    _need_gpu()
    big = RG.near_scene(3, n=60, m=400)
    mp = big["mp"]
    frames = [G.remap_for_map(G.sparse_frame_for_map(mp, 91, 200), mp), big, G.remap_for_map(G.sparse_frame_for_map(mp, 92, 180), mp)]
    kept = [RG.kept_entries(dict(f, mp=mp), RG.TH, 0.8) for f in frames]
    assert max(kept[0], kept[2]) < kept[1] and kept[0] > 0 and kept[2] > 0
    m = _matcher(monkeypatch, max(kept[0], kept[2]), max_batch=3)
    dframes = [DevFrame(s) for s in frames]; dmp = {k: _dev(v) for k, v in mp.items()}
    for rep in range(2):
        _check_map(_map_call(m, dframes, dmp, frames, RG.TH, 0.8, device_counter_frame=1), frames, mp, RG.TH, 0.8, "mixed")
    m.close()


def test_lastframe_search_with_entries_above_th_high():
    """k_lf_candidates drops every entry above TH_HIGH (k_lf_rounds accepts on the best distance alone)"""
    _need_gpu()
    from rgbd_pl_slam_amd import Matcher
    s = G.crowded_last(35, 96, 600, 4, 0.5, "neither")
    rng = np.random.default_rng(5)
    root = rng.integers(0, 256, 32, dtype=np.uint8)
    base = np.stack([RG._flip(rng, root, int(rng.integers(55, 91))) for _ in range(4)])
    s["desc"], _ = G.alphabet_desc(rng, base, len(s["kps"]))
    s["last"]["mp_desc"], _ = G.alphabet_desc(rng, base, len(s["last"]["mp_desc"]))
    m = Matcher(max_keypoints=max(STRIDE, 600), max_mappoints=G.CACHED_MAX_MAPPOINTS, max_batch=3)
    dlast = _dev_last(s["last"]); d = DevFrame(s)
    poses = [G.lf_pose(mo) for mo in ("backward", "neither", "forward")]
    frames = [s, s, s]
    _check_last(_last_calls(m, [d, d, d], dlast, frames, poses, 15.0, 0, False), frames, _last_refs(frames, s["last"], poses, 15.0, 0), "above")
    m.close()

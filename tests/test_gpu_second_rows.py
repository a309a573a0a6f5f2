"""Every row-per-workgroup (or row-per-wave) kernel of the map stage and the tracking tail with MORE ROWS THAN ITS GRID HOLDS, so that a workgroup takes a
second and a third row and has to work with what the earlier one left in its LDS tables, LDS counters and per-workgroup global scratch: the "goes back to
empty" and "restore zero" statements, the closing barriers and the `continue` paths of the grid-stride loops.  The scenes come from tests/stridegen.py (what
they contain is asserted on the CPU by tests/test_second_row_scenes.py); every output is compared bit for bit with the same plain restatements the
per-kernel tests use, through those tests' own helpers, and the sentinel and guard checks of those helpers hold for the rows past the cap as well."""
import numpy as np
import pytest

import stridegen as S
import test_gpu_covis as C
import test_gpu_culling as K
import test_gpu_localmap as M
import test_gpu_map as P
import test_gpu_normal as N
import test_track_ref as TR
import trackgen as TG
import trigen as XG
from conftest import gpu_available

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _need_gpu():
    if not gpu_available():
        pytest.fail("no GPU visible: the -m gpu tests need a real MI355X")


def _rows_past_the_cap(n_rows, cap):
    assert n_rows >= 2 * cap + 7, (n_rows, cap, "the cap was raised: this test no longer reaches a second row")


# ---------------------------------------------------------------------------------------------------------------- covisibility: k_covis_rows
@pytest.mark.parametrize("mode", ["conn", "votes"])
def test_covis_table_rows_after_an_overflow_into_the_global_counters(mode):
    s = S.covis_table_scene()
    _rows_past_the_cap(len(s["rows"]), S.grid_caps()["covis"])
    if mode == "conn":
        _, h, ref = C._check(s["rows"], s["selfs"], s["obs"], s["n_kf"], s["stride"], C.CONN, s["th"], dense=1, table=s["table"])
    else:
        _, h, ref = C._check(s["rows"], None, s["obs"], s["n_kf"], s["stride"], C.VOTES, 1, kf_bad=s["kf_bad"], dense=1, table=s["table"])
    G = s["G"]
    assert all(e is None for e in ref[G:2 * G]) and all(e is not None for e in ref[:G] + ref[2 * G:])
    # the same rows through the dense counters: the same bits
    if mode == "conn":
        dense = C._run(s["rows"], s["selfs"], s["obs"], s["n_kf"], s["stride"], C.CONN, s["th"]).host()
    else:
        dense = C._run(s["rows"], None, s["obs"], s["n_kf"], s["stride"], C.VOTES, 1, kf_bad=s["kf_bad"]).host()
    C._same(h, dense)


@pytest.mark.parametrize("mode", ["conn", "votes"])
def test_covis_dense_rows_full_empty_one_point_full(mode):
    s = S.covis_dense_scene()
    _rows_past_the_cap(len(s["rows"]), S.grid_caps()["covis"])
    if mode == "conn":
        C._check(s["rows"], s["selfs"], s["obs"], s["n_kf"], s["stride"], C.CONN, s["th"])
    else:
        C._check(s["rows"], None, s["obs"], s["n_kf"], s["stride"], C.VOTES, 1, kf_bad=s["kf_bad"])


@pytest.mark.parametrize("path", ["dense", "table"])
def test_covis_two_consecutive_lists_beyond_the_sort_cap_share_the_global_list(path):
    s = S.covis_long_scene()
    _rows_past_the_cap(len(s["rows"]), S.grid_caps()["covis"])
    kw = dict(dense=1) if path == "table" else {}                    # table: the default table fills, the counts move to the global counters
    _, h, ref = C._check(s["rows"], s["selfs"], s["obs"], s["n_kf"], s["stride"], C.CONN, s["th"], **kw)
    G, cap = s["G"], S.grid_caps()["covis_sort_cap"]
    for b in range(3):
        assert len(ref[b]["conn"]) > len(ref[b + G]["conn"]) > cap and h["n_conn"][b] > h["n_conn"][b + G] > cap
        assert 100 < len(ref[b]["ord"]) < cap


@pytest.mark.parametrize("path", ["dense", "table"])
def test_covis_votes_for_bad_keyframes_only_after_a_large_maximum(path):
    s = S.covis_votes_bad_scene()
    _rows_past_the_cap(len(s["rows"]), S.grid_caps()["covis"])
    kw = dict(dense=1, table=S.COVIS_TABLE) if path == "table" else {}
    _, h, ref = C._check(s["rows"], None, s["obs"], s["n_kf"], s["stride"], C.VOTES, 1, kf_bad=s["kf_bad"], **kw)
    G = s["G"]
    assert (h["max_kf"][G:2 * G] == -1).all() and (h["max_w"][G:2 * G] == 0).all() and (h["max_w"][:G] >= 6).all()


# ---------------------------------------------------------------------------------------------------------------- culling: k_cull_eval
def test_cull_eval_long_skipped_empty_and_mixed_candidates_in_turn():
    s = S.cull_scene()
    _rows_past_the_cap(s["n_cand"], S.grid_caps()["cull"])
    ref, _ = S.cull_reference(s)
    cand = [s["distinct"][d][0] for d in s["which"]]
    flags = [s["distinct"][d][1] for d in s["which"]]
    cmap = K._device_map(s["map"])
    h, _ = K._run(s["map"], cand, flags, False, s["ratio"], s["th_obs"], cmap=cmap)
    K._compare(h, ref, s["n_cand"])
    assert (h["kf_erased"] == K.MARK).all() and (h["point_went_bad"] == K.MARK).all()      # a snapshot erases nothing
    for force in (1, 2, 3):                                          # every point by lane, by lane group, by wave: the same bits
        K._same(h, K._run(s["map"], cand, flags, False, s["ratio"], s["th_obs"], force=force, cmap=cmap)[0])


# ---------------------------------------------------------------------------------------------------------------- local map
def test_local_items_short_and_long_rows_in_turn_share_the_global_table():
    s = S.local_items_scene()
    _rows_past_the_cap(len(s["local"]), S.grid_caps()["local"])
    h, refs = M._items_check(s["local"], s["kf_rows"], s["n_items"], s["item_stride"], s["item_bad"], s["frame_rows"], table=s["table"])
    G = s["G"]
    status = h["status"][:len(s["local"])]
    assert 0 < (status[G:2 * G] == 4).sum() < G and not status[:G].any() and not status[2 * G:3 * G].any()
    lds, _ = M._items_check(s["local"], s["kf_rows"], s["n_items"], s["item_stride"], s["item_bad"], s["frame_rows"])      # every row in the LDS table
    M._same(h, lds)


@pytest.mark.parametrize("dense", [0, 1])
def test_local_keyframes_seeded_with_what_the_waves_last_row_pushed(dense):
    s = S.local_kf_scene()
    _rows_past_the_cap(len(s["seeds"]), S.grid_caps()["local_kf"])
    h, refs = M._kf_check(s["seeds"], s["covis"], s["children"], s["parent"], s["kf_stride"], kf_bad=s["kf_bad"], dense=dense)
    G = s["G"]
    assert sum(len(r) > len(sd) for r, sd in zip(refs[2 * G:3 * G], s["seeds"][2 * G:3 * G])) > G // 4      # the third rows push keyframes of their own


def test_local_visible_empty_and_full_rows_in_turn():
    import torch
    from rgbd_pl_slam_amd import local_visible
    s = S.local_visible_scene()
    n_rows, stride = s["local_item"].shape
    _rows_past_the_cap(n_rows, S.grid_caps()["local"])
    want_iv, want_n, want_vis = S.local_visible_reference(s)
    fs, fi = M._csr(s["frame_rows"])
    iv = torch.full((n_rows * stride + M.GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    iv[:n_rows * stride] = M._dev(s["frustum"]).reshape(-1)
    vis = M._dev(np.concatenate([s["start"], np.full(M.GUARD, M.SENT, np.int32)]))
    n_to = torch.full((n_rows + M.GUARD,), M.SENT, dtype=torch.int32, device="cuda")
    local_visible(M._dev(s["local_item"]), M._dev(s["n_local"]), M._dev(s["seen"]), iv, vis[:s["n_items"]], fs, fi, M._dev(s["item_bad"]), n_to_match=n_to[:n_rows])
    torch.cuda.synchronize()
    iv, vis, n_to = iv.cpu().numpy(), vis.cpu().numpy(), n_to.cpu().numpy()
    assert np.array_equal(n_to[:n_rows], want_n) and (n_to[n_rows:] == M.SENT).all()
    assert np.array_equal(iv[:n_rows * stride].reshape(n_rows, stride), want_iv) and (iv[n_rows * stride:] == 0xA5).all()
    assert np.array_equal(vis[:s["n_items"]], want_vis) and (vis[s["n_items"]:] == M.SENT).all()


# ---------------------------------------------------------------------------------------------------------------- distinctive descriptors: k_map_*
_map_refs = {}


def _map_case(cls):
    """the scene of one size class and the restatement's answer, computed once and left unchanged"""
    if cls not in _map_refs:
        s = S.map_scene(cls)
        _map_refs[cls] = (s, S.map_reference(s))
    return _map_refs[cls]


def _map_check(cls):
    s, (want_md, want_bo, want_bm, _) = _map_case(cls)
    md, bo, bm = P._run(s["start"], s["desc"], s["valid"])
    assert np.array_equal(bo, want_bo), np.flatnonzero(bo != want_bo)[:10]
    assert np.array_equal(bm, want_bm), np.flatnonzero(bm != want_bm)[:10]
    assert np.array_equal(md, want_md)                               # rows without a valid observation stay 0xA5
    return s, want_bo


@pytest.mark.parametrize("cls", ["small", "wave", "block"])
def test_distinctive_descriptors_with_each_class_past_twice_its_grid(cls):
    c = S.grid_caps()
    s, want_bo = _map_check(cls)
    _rows_past_the_cap(s["n"], c["map_" + cls])
    assert (want_bo == -1).sum() >= s["n"] // s["P"] and (want_bo >= 0).sum() > s["n"] // 2


def test_distinctive_descriptors_one_wave_per_point_past_twice_its_grid(monkeypatch):
    """PLF_MAP_NAIVE=1: k_map_wave takes the points of the small class as well; the workgroup class of that schedule would need 2 * 8192 points of more
    than 256 observations, which is left out for its cost"""
    monkeypatch.setenv("PLF_MAP_NAIVE", "1")
    for cls in ("small", "wave"):
        s, _ = _map_check(cls)
        _rows_past_the_cap(s["n"], S.grid_caps()["map_wave"])


# ---------------------------------------------------------------------------------------------------------------- normal and depth: k_mapgeom_wave, k_mapgeom_block
def test_normal_and_depth_with_the_wave_and_workgroup_classes_past_twice_their_grids():
    s = S.normal_scene()
    c = S.grid_caps()
    _rows_past_the_cap(s["nw"], c["map_wave"])
    _rows_past_the_cap(s["nb"], c["mapgeom_block"])
    ref = N._ref(s["m"], s["scale"])
    got = N._run(s["m"], s["scale"])
    N._same(got, ref)
    assert (got[3] == -1).sum() == 3 and (got[3] > 2 * c["mapgeom_chunk"]).sum() >= 10
    untouched = got[3] == -1                                         # sentinels where a point is left alone
    assert (N.R.bits(got[0][untouched]) == N.R.SENTINEL).all() and (N.R.bits(got[1][untouched]) == N.R.SENTINEL).all()


# ---------------------------------------------------------------------------------------------------------------- tracking tail, triangulation
def test_close_points_with_more_frames_than_the_grid():
    """k_track_close_wave.  k_track_close_block is chosen by kp_stride above TRACK_WAVE_KEYS: 2^20 frames of 1025 key points are 38 GB of keys, depths and
    matches, so its second-row path is left to this test -- the body of both kernels is one template."""
    s = S.track_close_scene()
    assert s["n_frames"] >= s["G"] + 64, "the cap was raised: no wave takes a second frame"
    one = TG.ref_close(s["period"], **s["kw"])
    want = S.tile_result(one, s["idx"], ("new_kp", "new_pos", "n_new", "n_walked", "status", "match"))
    got = TG.dev_close(S.tile_batch(s["period"], s["idx"]), **s["kw"])
    TG.assert_close_equal(got, want, "second frames")
    ns = got["new_kp"].shape[1]
    k = np.minimum(want["n_new"], ns)[:, None]
    beyond = np.arange(ns)[None, :] >= k                             # nothing is written beyond min(count, stride)
    assert (got["new_kp"][beyond] == -1).all() and not got["new_pos"][beyond].any()


def test_need_keyframe_with_more_frames_than_the_grid():
    from test_gpu_track import run_need
    s = S.track_need_scene()
    assert s["n_frames"] >= s["G"] + 64
    t, idx = s["period"], s["idx"]
    counts, dec = TR.ref_need(t)
    big = dict(t, depth=t["depth"][idx], match=t["match"][idx], state=t["state"][idx])
    c2, d2 = run_need(big, n=t["n"][idx], n_inliers=t["n_inliers"][idx], item_bad=t["item_bad"], row_id=t["row_id"][idx])
    assert np.array_equal(c2, counts[idx]) and np.array_equal(d2, dec[idx])


def test_triangulation_with_more_jobs_than_the_grid():
    s = S.tri_scene()
    assert s["n_jobs"] >= s["G"] + 64
    one = XG.ref_call(s["period"], new_stride=s["new_stride"])
    want = S.tile_result(one, s["idx"], ("new_i1", "new_i2", "new_pos", "n_new", "status", "reason"))
    got = XG.dev_call(S.tile_jobs(s["period"], s["idx"]), new_stride=s["new_stride"])
    XG.assert_equal(got, want, "second jobs")
    ns = got["new_i1"].shape[1]
    beyond = np.arange(ns)[None, :] >= np.minimum(want["n_new"], ns)[:, None]
    assert (got["new_i1"][beyond] == -1).all() and (got["new_i2"][beyond] == -1).all() and not got["new_pos"][beyond].any()

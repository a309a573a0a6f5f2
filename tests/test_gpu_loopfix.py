"""The loop-correction calls on the device (include/plf.h, "Loop correction") against the definition tests/loopfixref.py -- the reference's literal
sequential loops -- bit for bit (a NaN equals any NaN): the Sim3 pairs and new poses for K = 1, 2 and 65 at three scales with the current keyframe
first, in the middle and last; ownership over rows of 0, 1, 63, 64, 65 and 257 entries, points held by 2, 3 and all rows, null / bad / out-of-range /
already-corrected entries, a second call, the reversed walk; the staged UpdateNormalAndDepth for a point seen from below, at, above and outside its
owner's rank with the reference keyframe in each of those places and 1, 16, 17, 256 and 257 observations; the essential-graph tail; the
bundle-adjustment tail; NaN inputs and empty calls.  The kernels of loopfix_kernels.hip do not cap their grids; the staged mapgeom kernels do, and
run here past the cap of the binning pass and of each size class; the chain runs from plf_sim3_optimize to plf_match_fuse_sim3."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loopfixgen as G  # noqa: E402
import loopfixref as R  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module", autouse=True)
def _leave_no_cached_device_memory():
    yield
    import gc
    import torch
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _check(sc, what=""):
    ref = G.ref_run(sc)
    got = G.gpu_run(sc)
    G.compare(ref, got, what)
    return ref, got


@pytest.mark.parametrize("K,scale,where", [(1, 1.0, 0), (2, 1.07, 0), (2, 0.5, 1), (65, 1.0, 32), (65, 1.07, 64), (65, 0.5, 0)])
def test_pairs_and_poses(K, scale, where):
    """K = 1 is the current keyframe alone (no Tic product); 65 is more keyframes than a wave; `where`: the current keyframe's rank"""
    rng = np.random.default_rng(K)
    n_kf = K + 5
    ranks = rng.permutation(n_kf)[:K]
    sc = G.make_scene(100 + K, n_kf=n_kf, n_points=40, rank_kf=ranks, cur=int(ranks[where]), scale=scale, row_len=[3] * K)
    ref, _ = _check(sc, "K %d" % K)
    assert (ref["corrected"][where] == sc["scw"]).all() and (ref["noncorrected"][:, 7] == 1.0).all()
    assert (ref["corrected"][:, 7] == scale).all() and np.isfinite(ref["tcw_new"]).all()


def test_no_scw_mode_writes_only_the_plain_sim3():
    import torch
    from rgbd_pl_slam_amd import loop_sim3_pairs
    sc = G.make_scene(4, n_kf=70, n_points=0, n_bad=0, n_marked=0)
    slots = np.array(list(range(70)) + [70, -1], np.int32)
    _, ref = R.sim3_pairs(sc["kf_tcw"], sc["kf_ow"], slots, 0, None)
    cor, non = loop_sim3_pairs(torch.from_numpy(sc["kf_tcw"]).cuda(), None, torch.from_numpy(slots).cuda())
    assert cor is None and G.same_bits(ref, non.cpu().numpy()).all() and np.isnan(ref[70:]).all()


SIZES = [0, 1, 63, 64, 65, 257, 30, 12, 5]


def test_rows_of_every_size_and_the_reversed_walk():
    sc = G.make_scene(3, n_kf=9, n_points=260, row_len=SIZES)
    ref, got = _check(sc, "sizes")
    assert len(set(ref["owner_rank"][ref["owner_rank"] >= 0])) >= 6
    rsc = G.reversed_ranks(sc)
    rev, _ = _check(rsc, "reversed")
    K = len(SIZES)
    changed = (ref["owner_rank"] >= 0) & (K - 1 - rev["owner_rank"] != ref["owner_rank"])
    assert changed.any() and (rev["world_pos"][changed] != ref["world_pos"][changed]).any() and (rev["normal"] != ref["normal"]).any()


def test_ownership_directed():
    """five rows that all begin with a null entry, a bad point, an id beyond the map and an already-corrected point; point 10 in every row, 11 in rows 3
    and 4, 12 in rows 1, 2 and 4, 13 only in the last row, 14 only in row 0"""
    n = 40
    sc = G.make_scene(8, n_kf=7, n_points=n, rank_kf=[5, 1, 6, 0, 3], cur=6, rows=[[]] * 5, n_bad=0, n_marked=0)
    sc["point_bad"][[0, 1]] = 1
    sc["corrected_by"][[2, 3]] = sc["cur_kf_id"]
    sc["corrected_ref"][[2, 3]] = 555
    head = [-1, 0, n + 3, 2, 1, -7, 3, 2 ** 31 - 1]
    sc["rows"] = [head + [14, 10, 20], head + [12, 10, 21, 20], head + [10, 12, 22], head + [11, 10, 23, 22], head + [13, 12, 11, 10, 24]]
    ref, got = _check(sc, "directed")
    own = ref["owner_rank"]
    assert [own[p] for p in (10, 11, 12, 13, 14, 20, 21, 22, 23, 24)] == [0, 3, 1, 4, 0, 0, 1, 2, 3, 4]
    assert (own[[0, 1, 2, 3]] == -1).all() and (ref["corrected_ref"][[2, 3]] == 555).all() and (ref["world_pos"][:4] == sc["world_pos"][:4]).all()
    assert (own[[4, 5, 30]] == -1).all()                    # in no row
    # a second call with the same current keyframe moves nothing
    again = dict(sc)
    for k in G.MAP_KEYS:
        again[k] = got[k]
    second = G.gpu_run(again)
    assert (second["owner_rank"] == -1).all() and G.same_bits(second["world_pos"], got["world_pos"]).all()
    assert (second["n_obs_used"] == -1).all() and G.same_bits(second["normal"], got["normal"]).all()


def _staged_scene():
    """ranks 0, 1, 2 are slots 7, 3, 11 of 300 keyframes; slot 20 is outside the list.  Points 0 .. 3 are held by rank 1 alone and seen from all four
    places, with the reference keyframe below, at, above and outside the owner's rank; points 4 .. 8 have 1, 16, 17, 256 and 257 observations"""
    n_kf, n = 300, 12
    lower, owner, higher, outside = 7, 3, 11, 20
    obs = [[lower, owner, higher, outside]] * 4
    for cnt in (1, 16, 17, 256, 257):
        others = [k for k in range(n_kf) if k not in (lower, owner, higher)]
        obs.append(([lower, higher, owner] + others)[:cnt] if cnt > 1 else [lower])
    obs += [[owner], [outside, 5], [higher, lower]]
    sc = G.make_scene(12, n_kf=n_kf, n_points=n, rank_kf=[lower, owner, higher], cur=owner, rows=[[9], list(range(9)) + [10], [0, 4, 11]], obs=obs, n_bad=0,
                      n_marked=0, angle=0.3)
    sc["ref_kf"][:9] = [lower, owner, higher, outside, lower, higher, owner, 100, lower]
    return sc


def test_staged_normal_and_depth():
    import torch
    from rgbd_pl_slam_amd import update_normal_and_depth
    sc = _staged_scene()
    ref, got = _check(sc, "staged")
    assert list(ref["owner_rank"]) == [1] * 9 + [0, 1, 2] and list(ref["n_obs_used"][4:9]) == [1, 16, 17, 256, 257]
    # after the commit a plain call sees every new centre: it must differ on the points whose walk saw a mixture
    d = got["_device"]
    normal, dmin, dmax = d["normal"].clone(), d["min_distance"].clone(), d["max_distance"].clone()
    update_normal_and_depth(world_pos=d["world_pos"], normal=normal, min_distance=dmin, max_distance=dmax, **G.geom_kwargs(d, d["kf_ow"]))
    torch.cuda.synchronize()
    normal, dmax = normal.cpu().numpy(), dmax.cpu().numpy()
    for p in (0, 1, 2, 3, 5, 6, 7, 8):
        assert (normal[p] != ref["normal"][p]).any(), p     # seen from the owner or a higher rank: the walk used an old centre there
    for p in (1, 2, 6):
        assert dmax[p] != ref["max_distance"][p], p         # the reference keyframe at or above the owner's rank
    for p in (0, 3, 4, 8, 10):
        assert dmax[p] == ref["max_distance"][p], p         # ... below it or outside the list: the same centre in both
    assert (normal[4] == ref["normal"][4]).all() and (normal[10] == ref["normal"][10]).all()   # seen only from below the owner / from outside


@pytest.mark.parametrize("sizes", [(42000, 10500, 660), (530000, 0, 0)])
def test_staged_normal_and_depth_past_the_grid_caps(sizes):
    """plf_loop_normal_depth with more owned points than one pass of each grid holds: k_mapgeom_small 2048 x 16, k_mapgeom_wave 2048 x 4, k_mapgeom_block
    512 workgroups; second case: k_mapgeom_bin 2048 x 256 points.  Left-alone (owner_rank -1) and bad points and mixed old / new centres lie all over the
    lists, so also in every workgroup's second pass.  Every point against the vectorised form of the rule, the last points of each class also against the
    literal definition."""
    import stridegen as S
    sc = G.staged_scene(5 + sizes[1], *sizes)
    ref = G.ref_run_staged(sc)
    c = S.grid_caps()
    owned = (sc["owner_rank"] >= 0) & (sc["point_bad"] == 0)
    cnt = np.diff(sc["obs_start"])
    if sizes[1]:
        assert (owned & (cnt <= 16)).sum() > c["map_small"] and (owned & (cnt > 16) & (cnt <= 256)).sum() > c["map_wave"]
        assert (owned & (cnt > 256)).sum() > c["mapgeom_block"]
    else:
        assert sc["n_points"] > 256 * c["map_blocks"]
    assert (~owned).sum() > 100 and (ref["n_obs_used"][~owned] == -1).all() and (ref["n_obs_used"][owned] > 0).all()
    got = G.gpu_run_staged(sc)
    G.compare(ref, got, "staged past the caps")
    # the literal definition on the last owned points of each class
    m = {k: sc[k].copy() for k in ("world_pos", "normal", "min_distance", "max_distance")}
    for k in ("point_bad", "obs_start", "obs_kf", "ref_kf", "ref_level", "scale_factors"):
        m[k] = sc[k]
    ends = np.cumsum(sizes)
    for p in [q for e in ends if e for q in range(e - 6, e) if owned[q]]:
        assert R.update_normal_depth(m, p, G.staged_centres(sc, p)) == got["n_obs_used"][p]
        assert G.same_bits(m["normal"][p], got["normal"][p]).all() and m["max_distance"][p] == got["max_distance"][p] and m["min_distance"][p] == got["min_distance"][p]
    mixed = 0
    for p in np.flatnonzero(owned)[-200:]:
        r = sc["kf_rank"][sc["obs_kf"][sc["obs_start"][p]:sc["obs_start"][p + 1]]]
        mixed += bool(((r >= 0) & (r < sc["owner_rank"][p])).any() and ((r < 0) | (r >= sc["owner_rank"][p])).any())
    assert mixed > 0 or not sizes[1]


def test_essential_graph_tail():
    sc = G.make_scene(3, n_kf=9, n_points=260, row_len=SIZES)
    es = G.essential_scene(sc, 1)
    ref = G.ref_run_essential(es)
    G.compare(ref, G.gpu_run_essential(es), "essential")
    marked = (es["corrected_by"] == es["cur_kf_id"]) & (es["point_bad"] == 0)
    assert (es["id_to_slot"][es["corrected_ref"][marked]] != es["ref_kf"][marked]).any() and (~marked & (es["point_bad"] == 0)).any()
    out = ~marked & ((es["ref_kf"] < 0) | (es["ref_kf"] >= es["n_kf"]))
    assert out.sum() == 3 and (ref["moved"][out] == 0).all() and (ref["moved"][es["point_bad"] == 1] == 0).all()


def test_gba_tail():
    """unflagged chains of depth 5 and 1 under flagged parents, one directly under an origin, two origins, a cycle no origin reaches; all four kinds of
    point (tests/test_loopfix_ref.py asserts the kinds on the same scene)"""
    sc = G.gba_scene(2, **G.GBA_TREE)
    G.compare(G.ref_run_gba(sc), G.gpu_run_gba(sc), "gba")
    flat = G.gba_scene(5, parent=[-1, 0, 0, 0], origins=[0], unflagged=[])       # depth 0: nothing to propagate
    G.compare(G.ref_run_gba(flat), G.gpu_run_gba(flat), "gba flat")
    two = G.gba_scene(6, parent=[-1, 0, 1, 2] + [3] * 300, origins=[0], unflagged=[2, 3] + list(range(4, 304)))   # depth 2 and 300 siblings at depth 3
    G.compare(G.ref_run_gba(two), G.gpu_run_gba(two), "gba wide")
    deep = G.gba_scene(4, **G.deep_tree())                                        # the tree is one chain of 700, a pose chain of depth 40 at its end
    G.compare(G.ref_run_gba(deep), G.gpu_run_gba(deep), "gba chain")


def test_chain_from_sim3_optimize():
    """plf_sim3_optimize -> plf_loop_scw -> plf_loop_sim3_pairs -> plf_loop_correct_points -> plf_loop_new_poses -> plf_loop_normal_depth ->
    plf_loop_commit_poses on one stream, g2oScm and mg2oScw never leaving the device, equal to the definitions' chain (tests/sim3optref.py, then this
    stage's).  The corrected rows are what plf_match_fuse_sim3 takes next, as a host argument (Converter::toCvMat of the row)."""
    import torch
    import sim3optgen as SG
    from rgbd_pl_slam_amd import sim3 as S3, sim3opt as SO, loop_scw
    so = SG.make_scene(93, [dict(n1=70, pairs=50, outliers=0.3, null=3, bad=4)])
    sref = SG.ref_run(so)
    assert sref["status"][0] == 0
    sc = G.make_scene(3, n_kf=9, n_points=260, row_len=SIZES)
    matched = int(sc["rank_kf"][4])
    sc["scw"] = R.row8(R.loop_scw(sref["sim3"][0], sc["kf_tcw"][matched]))
    ref = G.ref_run(sc)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
        keys = [t(np.ascontiguousarray(k).view(np.uint8).reshape(-1)) for k in so["kf_keys"]]
        kfs = S3.Sim3KeyFrames(keys, [t(m) for m in so["kf_mappoints"]], t(so["kf_pose"]), None)
        o = SO.sim3_optimize(kfs, t(so["job_kf1"]), t(so["job_kf2"]), t(so["match12"]), t(np.ascontiguousarray(so["sim3_in"], F32)), t(so["fix_scale"]),
                             t(so["world_pos"]), t(so["point_bad"]), t(so["inv_level_sigma2"]), tuple(float(x) for x in so["cam"][[0, 1, 2, 3, 9]]), th2=so["th2"],
                             scw=False, stream=st.cuda_stream)
        scw = loop_scw(o.sim3[0], t(sc["kf_tcw"]), matched, stream=st.cuda_stream)
        got = G.gpu_run(sc, stream=st.cuda_stream, scw_dev=scw)
    assert G.same_bits(scw.cpu().numpy(), sc["scw"]).all()
    G.compare(ref, got, "chain")
    assert (ref["owner_rank"] >= 0).sum() > 100 and np.isfinite(ref["world_pos"]).all()


def test_chain_from_sim3_optimize_to_fuse_sim3():
    """plf_sim3_optimize -> plf_loop_scw -> calls 1 - 4 -> plf_match_fuse_sim3 with the current keyframe's corrected Scw over the corrected map
    (world_pos, the staged normal and distances), all on one stream; the map stays on the device, the corrected row is read back because Scw is a host
    argument of the matcher.  Against the definitions' chain: tests/sim3optref.py, tests/loopfixref.py, the oracle's Fuse.  The scene puts the corrected
    points onto the map points of a keyframe scene of tests/kfgen.py, so that the fuse finds hundreds of them."""
    import torch
    import orc
    import sim3optgen as SG
    from rgbd_pl_slam_amd import Matcher, sim3 as S3, sim3opt as SO, loop_scw
    so = SG.make_scene(93, [dict(n1=70, pairs=50, outliers=0.3, null=3, bad=4)])
    sref = SG.ref_run(so)
    sc, c, matched = G.fuse_chain_scene(sref["sim3"][0])
    sc["scw"] = R.row8(R.loop_scw(sref["sim3"][0], sc["kf_tcw"][matched]))
    ref = G.ref_run(sc)
    cur_rank = list(sc["rank_kf"]).index(sc["cur_slot"])
    valid = (1 - sc["point_bad"]).astype(np.uint8)
    rpts = dict(xw=ref["world_pos"], normal=ref["normal"], min_dist=ref["min_distance"], max_dist=ref["max_distance"], desc=c["pts"]["desc"], valid=valid)
    eb, en = orc.fuse_sim3(c["kps"], c["desc"], c["scale"], c["bounds"], G.scw_matrix(ref["corrected"][cur_rank]), c["intr"], rpts, 3.0)
    assert en > 200 and len(set(ref["owner_rank"])) >= 3
    st = torch.cuda.Stream()
    m = Matcher(max_keypoints=1024, max_mappoints=1024)
    with torch.cuda.stream(st):
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
        keys = [t(np.ascontiguousarray(k).view(np.uint8).reshape(-1)) for k in so["kf_keys"]]
        kfs = S3.Sim3KeyFrames(keys, [t(x) for x in so["kf_mappoints"]], t(so["kf_pose"]), None)
        o = SO.sim3_optimize(kfs, t(so["job_kf1"]), t(so["job_kf2"]), t(so["match12"]), t(np.ascontiguousarray(so["sim3_in"], F32)), t(so["fix_scale"]),
                             t(so["world_pos"]), t(so["point_bad"]), t(so["inv_level_sigma2"]), tuple(float(x) for x in so["cam"][[0, 1, 2, 3, 9]]), th2=so["th2"],
                             scw=False, stream=st.cuda_stream)
        scw = loop_scw(o.sim3[0], t(sc["kf_tcw"]), matched, stream=st.cuda_stream)
        got = G.gpu_run(sc, stream=st.cuda_stream, scw_dev=scw)
        d = got["_device"]
        Scw = G.scw_matrix(got["corrected"][cur_rank])
        held = [t(np.frombuffer(np.ascontiguousarray(c["kps"]).tobytes(), np.uint8).copy()), t(c["desc"]), t(c["scale"]), t(c["uright"])]   # (the view keeps addresses only)
        kf = Matcher.frame_view(len(c["kps"]), held[0], held[1], held[2], c["bounds"], held[3])
        dp = dict(world_pos=d["world_pos"], normal=d["normal"], min_dist=d["min_distance"], max_dist=d["max_distance"], desc=t(c["pts"]["desc"]), valid=t(valid))
        best = torch.full((len(valid),), -7, dtype=torch.int32, device="cuda")
        cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
        m.FuseSim3(kf, Scw, c["intr"], dp, 3.0, best, cnt, stream=st.cuda_stream)
        st.synchronize()
    G.compare(ref, got, "chain to fuse")
    assert int(cnt[0]) == en and np.array_equal(best.cpu().numpy(), eb)
    m.close()


def test_nan_inputs_propagate():
    sc = G.make_scene(9, n_kf=5, n_points=60, row_len=[20] * 5)
    p = next(q for q in sc["rows"][0] if 0 <= q < 60 and not sc["point_bad"][q] and sc["corrected_by"][q] != sc["cur_kf_id"])
    sc["world_pos"][p, 1] = np.nan
    ref, _ = _check(sc, "NaN point")
    assert np.isnan(ref["world_pos"][p]).all()
    sc = G.make_scene(9, n_kf=5, n_points=60, row_len=[20] * 5)
    sc["scw"][2] = np.nan
    sc["kf_tcw"][1, 5] = np.inf
    ref, _ = _check(sc, "NaN Scw")
    assert np.isnan(ref["world_pos"][ref["owner_rank"] >= 0]).any()


def test_slots_out_of_range_own_nothing():
    sc = G.make_scene(31, n_kf=6, n_points=80, cur=2, rank_kf=[4, 2, 7, 0, -1, 5], row_len=[30] * 6)
    ref, _ = _check(sc, "bad slots")
    assert not set(ref["owner_rank"]) & {2, 4} and np.isnan(ref["corrected"][[2, 4]]).all()


def test_empty_calls():
    _check(G.make_scene(1, n_kf=4, n_points=0, n_bad=0, n_marked=0, row_len=[0] * 4), "no points")
    ref, _ = _check(G.make_scene(2, n_kf=4, n_points=30, rank_kf=[], cur=1, rows=[]), "no ranks")
    assert (ref["owner_rank"] == -1).all()


def test_argument_checks():
    import ctypes as C
    import torch
    from rgbd_pl_slam_amd import _lib as L
    lib = L.loopfix_prototypes(L.lib())
    x = torch.zeros(64, dtype=torch.float64, device="cuda").data_ptr()
    bad = L.PLF_E_BADARG
    assert lib.plf_loop_scw(x, x, 4, 4, x, 0, None) == bad and lib.plf_loop_scw(x, x, 4, -1, x, 0, None) == bad and lib.plf_loop_scw(None, x, 4, 0, x, 0, None) == bad
    assert lib.plf_loop_sim3_pairs(x, x, 4, x, 2, 4, x, x, x, 0, None) == bad and lib.plf_loop_sim3_pairs(x, x, 4, x, 2, 0, x, None, x, 0, None) == bad
    assert lib.plf_loop_sim3_pairs(x, x, 4, x, -1, 0, x, x, x, 0, None) == bad and lib.plf_loop_sim3_pairs(x, x, 4, None, 2, 0, x, x, x, 0, None) == bad
    v = L.LoopView(2, x, x, x, 4, x, 4, x)
    assert lib.plf_loop_correct_points(C.byref(v), x, x, 1, x, x, x, None, 0, None) == bad and lib.plf_loop_correct_points(None, x, x, 1, x, x, x, x, 0, None) == bad
    assert lib.plf_loop_correct_points(C.byref(L.LoopView(2, x, None, x, 4, x, 4, x)), x, x, 1, x, x, x, x, 0, None) == bad
    assert lib.plf_loop_new_poses(None, 2, x, x, 0, None) == bad and lib.plf_loop_commit_poses(x, 2, x, x, None, x, 4, 0, None) == bad
    assert lib.plf_loop_correct_points_by_ref(4, x, x, x, x, 1, None, 3, x, x, 4, x, None, 0, None) == bad
    assert lib.plf_gba_propagate_poses(C.byref(L.GbaView(4, x, x, 1, x, x, x, x, None)), 0, None) == bad
    assert lib.plf_gba_correct_points(4, x, x, x, x, x, x, x, None, 4, x, 0, None) == bad and lib.plf_gba_correct_points(-1, x, x, x, x, x, x, x, x, 4, x, 0, None) == bad
    assert lib.plf_loop_normal_depth(C.byref(L.MapGeomView()), None, x, 2, x, x, x, x, x, 4, x, 0, None) == bad
    assert lib.plf_loop_new_poses(x, 2, x, x, 64, None) == bad

"""plf_sim3_optimize / plf_sim3_keep_inliers on the device against the definition tests/sim3optref.py, bit for bit (a NaN equals any NaN): the
correspondence counts around the `< 10` test, around a round of the workgroup (32 correspondences = 64 edges, one per lane), around two rounds (64)
and beyond the LDS list (1024), both strides, mixed fix_scale, NULL and bad points, absent and out-of-range observations, jobs that cull and
jobs that do not, a start 20 degrees off, NaN inputs, and the chain from plf_sim3_pairs to plf_match_project_sim3."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sim3optgen as G  # noqa: E402
import sim3optref as R  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
SIZES = (0, 9, 10, 11, 31, 32, 33, 63, 64, 65)


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


def _sizes_jobs():
    return [dict(n1=n + 6 + 5 * (i % 4), pairs=n, fix_scale=bool(i & 1), outliers=0.2 if n >= 31 and (i & 2) else 0.0, null=min(i, 2), bad=min(i, 3))
            for i, n in enumerate(SIZES)]


@pytest.mark.parametrize("kp_stride", [64, 300])
def test_correspondence_counts_at_every_edge(kp_stride):
    """kp_stride 64 cuts the key points of the larger jobs (n1 > 64): i runs over [0, min(kf_n, kp_stride))"""
    sc = G.make_scene(31, _sizes_jobs(), kp_stride=kp_stride)
    ref, _ = _check(sc, "sizes %d" % kp_stride)
    n_corr = [len(R.correspondences(sc, j, sc["match12"][j])) for j in range(len(SIZES))]
    if kp_stride == 300:
        assert n_corr == list(SIZES)
    assert [bool(s & R.FEW) for s in ref["status"]] == [n < 10 for n in n_corr]
    its = [c["optimize"] for c in ref["counters"]]
    assert [5, 5] in its and [5, 10] in its and [5] in its


def test_a_job_beyond_the_list_walks_every_key_point():
    """1030 correspondences (the list holds 1024) among 1100 key points, with outliers to cull, beside a short job"""
    sc = G.make_scene(41, [dict(n1=1100, pairs=1030, outliers=0.05, null=3, bad=4), dict(n1=40, pairs=20, fix_scale=True)])
    ref, _ = _check(sc, "beyond the list")
    assert len(R.correspondences(sc, 0, sc["match12"][0])) == 1030 and ref["counters"][0]["optimize"] == [5, 10] and ref["n_inliers"][0] > 900


@pytest.mark.parametrize("n_jobs", [1, 3])
def test_job_counts(n_jobs):
    """a long job, a FEW job and a full one in one call"""
    jobs = [dict(n1=120, pairs=100, outliers=0.3), dict(n1=20, pairs=7), dict(n1=50, pairs=33, fix_scale=True)][:n_jobs]
    ref, _ = _check(G.make_scene(51, jobs), "jobs %d" % n_jobs)
    assert ref["n_inliers"][0] >= 20


def test_points_and_observations_that_do_not_count():
    """bad and NULL points, kf_obs_index entries of -1 and out of range, match12 entries >= kf_n and ids beyond the map: each counts as "none\""""
    sc = G.make_scene(61, [dict(n1=70, pairs=40, null=4, bad=6, noobs=5, outliers=0.1), dict(n1=60, pairs=30, noobs=3, fix_scale=True)], obs_index=True)
    n_before = len(R.correspondences(sc, 0, sc["match12"][0]))
    live = np.nonzero(sc["match12"][0] >= 0)[0]
    sc["match12"][0, live[0]] = sc["kf_n"][1]                       # >= kf_n[kf2]
    sc["match12"][0, live[1]] = 10 ** 6
    sc["kf_obs_index"][1][sc["match12"][0, live[2]]] = sc["kf_n"][1] + 5
    sc["kf_mappoints"][0][live[3]] = len(sc["point_bad"])           # an id beyond the map
    sc["kf_mappoints"][1][sc["match12"][0, live[4]]] = -9
    sc["kf_octave"][0][live[5]] = 99                                # clamped
    sc["kf_keys"][0][live[5], 5] = np.array([99], np.int32).view(F32)[0]
    sc["kf_octave"][0][live[6]] = -3
    sc["kf_keys"][0][live[6], 5] = np.array([-3], np.int32).view(F32)[0]
    assert len(R.correspondences(sc, 0, sc["match12"][0])) <= n_before - 3
    _check(sc, "none")


def test_cull_nothing_cull_some_and_drop_below_ten():
    sc = G.standard_scene()
    ref, _ = _check(sc, "standard")
    its = [c["optimize"] for c in ref["counters"]]
    assert its[0] == [5, 10] and its[1] == [5, 5]                   # a job that culls beside one that does not
    assert ref["status"][4] == R.FEW and (ref["match12"][4] != sc["match12"][4]).any()   # below 10 after the cull: the nulled matches stay nulled
    assert ref["status"][3] == R.FEW and np.array_equal(ref["match12"][3], sc["match12"][3])


def test_start_twenty_degrees_off_rejects_trials():
    sc = G.make_scene(71, [dict(n1=60, pairs=40, off_deg=20.0, off_t=0.3), dict(n1=60, pairs=40, off_deg=20.0, off_t=0.3, fix_scale=True, outliers=0.2)])
    ref, _ = _check(sc, "20 degrees")
    assert sum(c["rejected"] for c in ref["counters"]) > 0


def test_nan_inputs_fault_nowhere_and_leave_the_other_jobs():
    """a NaN / Inf in sim3_in gives NONFINITE.  A NaN map point makes every sum NaN, so every factorisation is refused and every trial rejected: the
    estimate never leaves the start, sim3_out stays FINITE and the definition (as g2o) reports no NONFINITE for it; the device must say the same."""
    jobs = [dict(n1=40, pairs=25), dict(n1=40, pairs=25, fix_scale=True), dict(n1=40, pairs=25, outliers=0.2), dict(n1=30, pairs=20)]
    clean = G.make_scene(81, jobs)
    sc = G.make_scene(81, jobs)
    sc["sim3_in"][0, 4] = np.nan
    i = int(np.nonzero(sc["match12"][1] >= 0)[0][3])
    sc["world_pos"][sc["kf_mappoints"][2][i]] = np.nan              # a point of job 1's keyframe 1
    sc["sim3_in"][3, 12] = np.inf
    ref, got = _check(sc, "nan")
    assert ref["status"][0] & R.NONFINITE and ref["status"][3] & R.NONFINITE and not ref["status"][1] & R.NONFINITE
    assert ref["counters"][1]["rejected"] == ref["counters"][1]["trials"] > 0 and np.isfinite(got["sim3"][1]).all()
    base = G.ref_run(clean)
    assert G.same_doubles(base["sim3"][2], got["sim3"][2]) and np.array_equal(base["match12"][2], got["match12"][2])


def test_bad_slots_do_no_work():
    sc = G.make_scene(91, [dict(n1=30, pairs=20), dict(n1=30, pairs=20), dict(n1=30, pairs=20)])
    sc["job_kf1"][0] = -1
    sc["job_kf2"][2] = len(sc["kf_n"])
    ref, got = _check(sc, "bad slot")
    assert ref["status"].tolist() == [R.BAD_SLOT, 0, R.BAD_SLOT] and np.isnan(got["scw"][0]).all() and np.array_equal(got["match12"][0], sc["match12"][0])


def test_keep_inliers_is_the_elementwise_statement():
    import torch
    from rgbd_pl_slam_amd import sim3_keep_inliers
    rng = np.random.default_rng(3)
    J, S = 3, 300
    match = rng.integers(-1, 50, (J, S)).astype(np.int32)
    inl = (rng.random((J, S)) < 0.6).astype(np.uint8)
    kf_n = np.array([300, 130, 0], np.int32)
    dev = torch.device("cuda", 0)
    for n in (None, kf_n):
        m = torch.from_numpy(match.copy()).to(dev)
        sim3_keep_inliers(m, torch.from_numpy(inl).to(dev), None if n is None else torch.from_numpy(n).to(dev))
        assert np.array_equal(m.cpu().numpy(), R.keep_inliers(match, inl, n))


def test_python_solver_class_optimizes_after_a_hit():
    """Sim3Solver.iterate() to a hit, then .optimize(): keep-inliers and OptimizeSim3 as ComputeSim3 chains them, against the definitions chained"""
    import torch
    import sim3gen
    from rgbd_pl_slam_amd import Sim3KeyFrames, Sim3Solver
    sc = G.make_scene(101, [dict(n1=80, pairs=60, outliers=0.3)])
    sc.update(prob=0.99, min_inliers=20, max_iterations=40, pair_stride=80, max_hits=1, rand3=sim3gen.raw_values(9, (1, 40, 3)))
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    kfs = Sim3KeyFrames([t(np.ascontiguousarray(k).view(np.uint8).reshape(-1)) for k in sc["kf_keys"]], [t(m) for m in sc["kf_mappoints"]], t(sc["kf_pose"]))
    cam = tuple(float(x) for x in sc["cam"][[0, 1, 2, 3, 9]])
    s = Sim3Solver(kfs, 0, 1, t(sc["match12"][0]), t(sc["world_pos"]), t(sc["point_bad"]), t(sc["level_sigma2"]), cam, False)
    s.SetRansacParameters(0.99, 20, 40, rand3=t(sc["rand3"][0]))
    T, _, inl, n = s.iterate(40)
    pr, st, ((count, hits),) = sim3gen.ref_run(sc, [40])
    assert T is not None and hits["n_hits"][0] > 0
    kept = R.keep_inliers(sc["match12"], hits["hit_inlier12"][:, 0])
    ref = R.optimize_sim3(sc, 0, hits["hit_sim3"][0, 0], False, 10.0, kept[0])
    n_in, sim3, scw, match = s.optimize(t(sc["inv_level_sigma2"]))
    assert n_in == ref["n_inliers"] and G.same_doubles(sim3.numpy(), np.array(ref["sim3"])) and np.array_equal(match.numpy(), ref["match"])
    assert G.same_bits(scw.numpy().ravel(), ref["scw"])


def test_chain_pairs_iterate_keep_search_optimize_project():
    """plf_sim3_pairs -> plf_sim3_iterate -> plf_sim3_keep_inliers -> plf_match_sim3 -> plf_sim3_optimize -> plf_match_project_sim3 with the scw_out it wrote:
    the statements of LoopClosing::ComputeSim3 for one candidate, each stage against its own reference (tests/sim3ref.py, the oracle's SearchBySim3,
    tests/sim3optref.py, the oracle's SearchByProjection) chained on the host.  The matches stay on the device from stage to stage; what is copied back is
    only what the matcher calls take as host arguments: the hit's s12 / R12 / t12 and Scw."""
    import torch
    import kfgen
    import orc
    import sim3gen
    from rgbd_pl_slam_amd import Matcher, Sim3KeyFrames, sim3_pairs, sim3_iterate, sim3_keep_inliers, sim3_optimize
    n = 600
    c = kfgen.two_keyframe_scene(5, n, nodes=60, s12=1.0, tz=0.3)
    has1, has2 = c["pts1"]["valid"], c["pts2"]["valid"]
    a1, a2 = np.ascontiguousarray(c["kps1"]["angle"]), np.ascontiguousarray(c["kps2"]["angle"])
    ar = np.arange(n, dtype=np.int32)
    keys = [np.frombuffer(np.ascontiguousarray(c["kps" + s]).tobytes(), F32).reshape(n, 7).copy() for s in "12"]
    pose = np.array([np.concatenate([c["pose" + s]["Rcw"].ravel(), c["pose" + s]["tcw"], c["pose" + s]["Ow"]]) for s in "12"], F32)
    cam = np.array([c["fx"], c["fy"], c["cx"], c["cy"], 0, 0, 0, 0, 0, 40.0], F32)
    sig2 = np.ascontiguousarray(c["sigma2"], F32)
    sc = dict(cam=cam, level_sigma2=sig2, inv_level_sigma2=(F32(1.0) / sig2).astype(F32), kf_n=np.array([n, n], np.int32), kf_pose=pose, kf_keys=keys,
              kf_octave=[np.ascontiguousarray(c["kps" + s]["octave"], np.int32) for s in "12"],
              kf_mappoints=[np.where(has1 != 0, ar, -1).astype(np.int32), np.where(has2 != 0, ar + n, -1).astype(np.int32)], kf_obs_index=None,
              world_pos=np.concatenate([c["pts1"]["xw"], c["pts2"]["xw"]]).astype(F32), point_bad=np.zeros(2 * n, np.uint8), job_kf1=np.array([0], np.int32),
              job_kf2=np.array([1], np.int32), fix_scale=np.array([0], np.uint8), prob=0.99, min_inliers=20, max_iterations=300, pair_stride=n, max_hits=1,
              rand3=sim3gen.raw_values(3, (1, 300, 3)), th2=10.0)
    # ---- the references, stage by stage
    em, _ = orc.search_by_bow_kf(c["desc1"], c["desc2"], a1, a2, has1, has2, c["nodes1"], c["nodes2"], 0.75, 1)
    sc["match12"] = np.ascontiguousarray(em, np.int32).reshape(1, n)
    _, _, ((_, hits),) = sim3gen.ref_run(sc, [300])
    assert hits["n_hits"][0] > 0
    sim3 = hits["hit_sim3"][0, 0]
    kept = R.keep_inliers(sc["match12"], hits["hit_inlier12"][:, 0])[0]

    def masks(match):
        v1 = (has1 != 0) & (match < 0)
        v2 = has2 != 0
        v2[match[match >= 0]] = False
        return v1.astype(np.uint8), v2.astype(np.uint8)

    v1, v2 = masks(kept)
    c2 = dict(c, s12=float(sim3[12]), R12=sim3[:9].reshape(3, 3).copy(), t12=sim3[9:12].copy(), th=7.5, pts1=dict(c["pts1"], valid=v1), pts2=dict(c["pts2"], valid=v2))
    fm, fn = orc.search_by_sim3(c2)
    merged = np.where(fm >= 0, fm, kept).astype(np.int32)
    ro = R.optimize_sim3(sc, 0, sim3, False, 10.0, merged)
    assert fn > 0 and ro["status"] == 0 and ro["n_inliers"] >= 20
    Scw = ro["scw"].reshape(4, 4)
    after = ro["match"]
    _, w2 = masks(after)
    init = np.where(after >= 0, -2, -1).astype(np.int32)
    intr = {k: c["pose1"][k] for k in ("fx", "fy", "cx", "cy", "bf", "log_scale_factor")}
    # the loop map points' mean viewing directions (the scene leaves them zero, and SearchByProjection drops a point seen from behind its normal)
    d = c["pts2"]["xw"].astype(np.float64) - c["pose2"]["Ow"].astype(np.float64)
    normal2 = (d / np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-9)).astype(F32)
    pm, pn = orc.search_by_projection_sim3(c["kps1"], c["desc1"], c["scale"], (0.0, 0.0, 640.0, 480.0), Scw, intr, dict(c["pts2"], valid=w2, normal=normal2), 10, init)
    # ---- the device, one stream
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    st = torch.cuda.Stream()
    m = Matcher(max_keypoints=1024, max_mappoints=1024)
    ds = t(c["scale"])
    dk = [t(np.frombuffer(np.ascontiguousarray(c["kps" + s]).tobytes(), np.uint8).copy()) for s in "12"]
    dd = [t(c["desc1"]), t(c["desc2"])]
    kfs = Sim3KeyFrames(dk, [t(x) for x in sc["kf_mappoints"]], t(pose))
    camt = (float(c["fx"]), float(c["fy"]), float(c["cx"]), float(c["cy"]), 40.0)
    args = {k: t(sc[k]) for k in ("job_kf1", "job_kf2", "world_pos", "point_bad", "level_sigma2", "inv_level_sigma2", "rand3", "fix_scale")}
    match = t(sc["match12"])
    dh = [t(has1), t(has2)]
    views = [Matcher.frame_view(n, dk[i], dd[i], ds, (0.0, 0.0, 640.0, 480.0), None) for i in range(2)]

    def dpts(s, valid):
        return dict(world_pos=t(c["pts" + s]["xw"]), normal=None, min_dist=t(c["pts" + s]["min_dist"]), max_dist=t(c["pts" + s]["max_dist"]), desc=t(c["pts" + s]["desc"]),
                    valid=valid)

    def dmasks(mt):
        d1 = ((dh[0] != 0) & (mt < 0)).to(torch.uint8)
        d2 = dh[1].clone()
        d2[mt[mt >= 0].long()] = 0
        return d1, (d2 != 0).to(torch.uint8)

    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        pr = sim3_pairs(kfs, args["job_kf1"], args["job_kf2"], match, args["world_pos"], args["point_bad"], args["level_sigma2"], camt, pair_stride=n,
                        stream=st.cuda_stream)
        out = sim3_iterate(pr, args["rand3"], 300, args["fix_scale"], camt, min_inliers=20, max_hits=1, stream=st.cuda_stream)
        sim3_keep_inliers(match, out.hit_inlier12[:, 0].contiguous(), stream=st.cuda_stream)
        d1, d2 = dmasks(match[0])
        hs = out.hit_sim3[0, 0].cpu().numpy()                               # the host arguments of plf_match_sim3
        match2 = torch.full((n,), -7, dtype=torch.int32, device=dev)
        cnt = torch.zeros(1, dtype=torch.int32, device=dev)
        m.SearchBySim3(views[0], views[1], c["pose1"], c["pose2"], float(hs[12]), hs[:9].reshape(3, 3).copy(), hs[9:12].copy(), 7.5, dpts("1", d1), dpts("2", d2),
                       match2, cnt, stream=st.cuda_stream)
        match[0] = torch.where(match2 >= 0, match2, match[0])
        o = sim3_optimize(kfs, args["job_kf1"], args["job_kf2"], match, out.hit_sim3[:, 0].contiguous(), args["fix_scale"], args["world_pos"], args["point_bad"],
                          args["inv_level_sigma2"], camt, th2=10.0, stream=st.cuda_stream)
        dScw = o.scw[0].cpu().numpy().reshape(4, 4)                         # the host argument of plf_match_project_sim3
        _, e2 = dmasks(match[0])
        mk = torch.where(match[0] >= 0, torch.full_like(match[0], -2), torch.full_like(match[0], -1))
        nm = torch.zeros(1, dtype=torch.int32, device=dev)
        m.SearchByProjectionSim3(views[0], dScw, intr, dict(dpts("2", e2), normal=t(normal2)), 10, mk, nm, stream=st.cuda_stream)
    st.synchronize()
    assert G.same_bits(hs, sim3) and int(cnt[0]) == fn and np.array_equal(match2.cpu().numpy(), fm)
    assert int(o.n_inliers[0]) == ro["n_inliers"] and int(o.status[0]) == 0 and G.same_doubles(o.sim3[0].cpu().numpy(), np.array(ro["sim3"]))
    assert np.array_equal(match[0].cpu().numpy(), after) and G.same_bits(dScw.ravel(), ro["scw"])
    assert pn > 0 and int(nm[0]) == pn and np.array_equal(mk.cpu().numpy(), pm)
    m.close()

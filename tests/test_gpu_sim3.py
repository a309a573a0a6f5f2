"""plf_sim3_pairs / plf_sim3_iterate on the device against the definition tests/sim3ref.py, bit for bit (a NaN equals any NaN): the pair-count edges, the
chunk and workgroup edges of both kernels, the window splits with the state carried on the device, masks, overflow, degenerate triples, zero and
negative depths, NaN / Inf inputs, bad slots and indices."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sim3gen as G  # noqa: E402
import sim3ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
SIZES = (0, 2, 3, 19, 20, 21, 63, 64, 65, 255, 256, 257, 1000)


@pytest.fixture(scope="module", autouse=True)
def _leave_no_cached_device_memory():
    """this module's tensors are released when it ends, so that the modules after it start from the allocator state they would
    find without it"""
    yield
    import gc
    import torch
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _check(sc, windows=None, active=None, what=""):
    ref = G.ref_run(sc, windows, active)
    got = G.gpu_run(sc, windows, active)
    G.compare(ref, got, what)
    return ref, got


def _sizes_scene(min_inliers):
    """N pairs at every edge of the pair walk (64), of the constructor's chunks (256) and of min_inliers; n1 up to 1100 so that the chunks straddle"""
    jobs = [dict(n1=n + 5 + 7 * (i % 5) if n < 1000 else 1100, pairs=n, outliers=0.3 if n >= 19 else 0.0, null=min(2, i), bad=min(3, i), fix_scale=bool(i & 1))
            for i, n in enumerate(SIZES)]
    return G.make_scene(21 + min_inliers, jobs, min_inliers=min_inliers, max_iterations=48, pair_stride=1100, max_hits=3)


@pytest.mark.parametrize("min_inliers", [20, 3])
def test_pair_counts_at_every_edge(min_inliers):
    sc = _sizes_scene(min_inliers)
    (pr, st, _), _ = _check(sc, None, None, "sizes")
    assert pr["n_pairs"].tolist() == list(SIZES)
    ran = st["max_its"] > 0
    assert ran.tolist() == [n >= max(3, min_inliers) for n in SIZES]
    assert st["max_its"][SIZES.index(min_inliers)] == 1                      # N == min_inliers: one iteration
    assert st["max_its"][-1] == 48 if min_inliers == 20 else True


@pytest.fixture(scope="module")
def long_scene():
    """300 iterations at most: 100 pairs and 500 pairs (staged in LDS in a long window), 1000 pairs (beyond the staging limit of 853: read from global
    memory), and a job capped below the window (N near min_inliers)"""
    jobs = [dict(n1=130, pairs=100, outliers=0.4), dict(n1=520, pairs=500, outliers=0.5, fix_scale=True), dict(n1=1100, pairs=1000, outliers=0.4, scale=1.2),
            dict(n1=40, pairs=24, outliers=0.1)]
    sc = G.make_scene(31, jobs, max_iterations=300, pair_stride=1024, max_hits=4)
    sc["full"] = G.ref_run(sc)
    return sc


def test_long_scene_is_what_it_says(long_scene):
    pr, st, _ = long_scene["full"]
    assert st["max_its"].tolist()[:3] == [300, 300, 300] and 1 < st["max_its"][3] < 20
    assert pr["n_pairs"].tolist() == [100, 500, 1000, 24]
    from rgbd_pl_slam_amd import sim3
    table = sim3.its_for_n(long_scene["prob"], long_scene["min_inliers"], long_scene["max_iterations"], 1024).numpy()      # plf_sim3_its_for_n
    assert table[pr["n_pairs"]].tolist() == st["max_its"].tolist()


@pytest.mark.parametrize("iter_count", [1, 5, 255, 256, 257, 300])
def test_iter_counts_around_the_workgroup(long_scene, iter_count):
    _check(long_scene, [iter_count], None, "iter_count %d" % iter_count)


@pytest.mark.parametrize("windows", [[5] * 60, [300], [1, 7, 292]])
def test_window_splits_carry_the_state_on_the_device(long_scene, windows):
    sc = long_scene
    ref, got = _check(sc, windows, None, "windows")
    # and any split reports what the one window of 300 does
    full = sc["full"]
    for k in G.STATE_KEYS:
        assert G.same_bits(full[1][k], got[1][k]), k
    count, hits = G.merge_windows(got[2], sc["max_hits"])
    G.compare((full[0], full[1], full[2]), (got[0], got[1], [(count, hits)]), "merged")


def test_active_mask(long_scene):
    sc = long_scene
    act = np.array([1, 0, 1, 0], np.uint8)
    (pr, st, runs), got = _check(sc, [40, 30], act, "active")
    assert st["iterations_done"].tolist()[:3] == [70, 0, 70] and got[1]["best_iter"][1] == -1
    assert (got[2][0][0][1] == -1).all()                                     # the masked job's counts are untouched


def test_max_hits_of_one_with_more_hits(long_scene):
    sc = dict(long_scene, max_hits=1)
    (_, _, runs), _ = _check(sc, [300], None, "max_hits 1")
    assert runs[0][1]["n_hits"].max() > 1


@pytest.mark.parametrize("n_jobs", [1, 2, 70])
def test_jobs_of_mixed_sizes(n_jobs):
    rng = np.random.default_rng(n_jobs)
    jobs = [dict(n1=int(n) + 9, pairs=int(n), outliers=float(o), fix_scale=bool(i % 3 == 0), scale=1.0 + 0.1 * (i % 4))
            for i, (n, o) in enumerate(zip(rng.integers(15, 70, n_jobs), rng.uniform(0, 0.5, n_jobs)))]
    sc = G.make_scene(100 + n_jobs, jobs, max_iterations=24, max_hits=2)
    _check(sc, [5, 5, 14], None, "jobs %d" % n_jobs)


def test_overflow_and_statuses():
    sc = G.standard_scene()
    (pr, st, _), _ = _check(sc, None, None, "standard")
    assert pr["status"].tolist() == [0, 0, 0, 0, 0, 0, R.TOO_FEW, R.OVERFLOW, R.BAD_SLOT]


def test_small_pair_stride_stages_every_job():
    """pair_stride 128: every job's pairs fit in LDS beside the solved iterations; a window of 200 takes the one-job-per-workgroup mapping"""
    jobs = [dict(n1=128, pairs=n, outliers=0.35) for n in (128, 97, 64, 33)]
    sc = G.make_scene(41, jobs, max_iterations=200, pair_stride=128, max_hits=2)
    _check(sc, [200], None, "staged")


def _collapse(Xc1, Xc2):
    Xc1[:] = Xc1[0]
    Xc2[:] = Xc2[0]


def _collinear(Xc1, Xc2):
    t = np.linspace(-1, 1, len(Xc1))[:, None]
    Xc1[:] = Xc1[0] + t * np.array([0.5, 0.25, 1.0])
    Xc2[:] = Xc2[0] + t * np.array([0.5, 0.25, 1.0])


def _depths(Xc1, Xc2):
    Xc2[::4, 2] = 0.0
    Xc1[1::4, 2] = -Xc1[1::4, 2]
    Xc1[2::8, 2] = 0.0
    Xc2[3::8, 2] = -1.0


def test_degenerate_triples_and_depths():
    """coincident points (0 / 0 in the scale and the angle: NaN propagates as in the definition), collinear points, z = 0 and z < 0 in either projection"""
    jobs = [dict(n1=40, pairs=30, mutate=_collapse), dict(n1=40, pairs=30, mutate=_collinear), dict(n1=60, pairs=48, mutate=_depths, outliers=0.2),
            dict(n1=40, pairs=30, mutate=_collapse, fix_scale=True)]
    sc = G.make_scene(51, jobs, max_iterations=30, max_hits=2)
    (pr, st, runs), got = _check(sc, [30], None, "degenerate")
    assert np.isnan(got[1]["best_sim3"][0]).any() or got[1]["best_inliers"][0] == 0


def test_nan_and_inf_in_poses_and_positions():
    def nan_pose(Rcw, tcw):
        tcw = tcw.copy(); tcw[0] = np.nan
        return Rcw, tcw

    def inf_pose(Rcw, tcw):
        Rcw = Rcw.copy(); Rcw[1, 1] = np.inf
        return Rcw, tcw

    jobs = [dict(n1=40, pairs=30, pose_mutate=nan_pose), dict(n1=40, pairs=30, pose_mutate=inf_pose), dict(n1=50, pairs=40, outliers=0.2)]
    sc = G.make_scene(61, jobs, max_iterations=20, max_hits=2)
    ids = sc["kf_mappoints"][4][sc["kf_mappoints"][4] >= 0]
    sc["world_pos"][ids[0]] = np.nan
    sc["world_pos"][ids[1], 2] = np.inf
    sc["world_pos"][ids[2]] = -np.inf
    sc["level_sigma2"] = sc["level_sigma2"].copy()
    _check(sc, [20], None, "nan / inf")


def test_bad_indices_fault_nowhere():
    """match12 entries >= kf_n[kf2] and hugely negative, point ids out of range, kf_obs_index with -1, out of range and permuted, octaves out of range,
    slots out of range on either side"""
    jobs = [dict(n1=60, pairs=45, outliers=0.2, null=3, bad=4), dict(n1=50, pairs=40), dict(n1=30, pairs=25), dict(n1=30, pairs=25)]
    sc = G.make_scene(71, jobs, max_iterations=16, max_hits=2, obs_index=True)
    m = sc["match12"]
    before, _ = R.pairs(sc, sc["pair_stride"], G.table_of(sc))
    assert before["n_pairs"][0] == 45
    has = before["idx1"][0, :45]                                             # the key points of keyframe 1 whose pair is valid
    m[0, has[0]] = sc["kf_n"][1]
    m[0, has[1]] = 2 ** 31 - 1
    m[0, has[2]] = -2 ** 31
    sc["kf_mappoints"][0][has[3]] = len(sc["point_bad"])
    sc["kf_mappoints"][0][has[4]] = -7
    o1, o2 = sc["kf_obs_index"][0], sc["kf_obs_index"][1]
    o1[has[5]] = -1
    o1[has[6]] = sc["kf_n"][0]
    o1[has[7]], o1[has[8]] = o1[has[8]], o1[has[7]]                         # a permuted index: the octave of the other key point
    G.set_octave(sc, 0, int(has[7]), 0); G.set_octave(sc, 0, int(has[8]), 7)
    o2[m[0, has[9]]] = -1
    G.set_octave(sc, 0, int(has[10]), 99); G.set_octave(sc, 0, int(has[11]), -5)
    sc["job_kf1"][2] = -1
    sc["job_kf2"][3] = 10 ** 6
    (pr, _, _), _ = _check(sc, [16], None, "bad indices")
    assert pr["status"].tolist()[2:] == [R.BAD_SLOT, R.BAD_SLOT] and pr["n_pairs"][0] == 45 - 8


def test_python_solver_class_has_the_reference_call_shape():
    """rgbd_pl_slam_amd.Sim3Solver over one job: find() returns the first hit of the definition, iterate(5) rounds go on from where the last one returned"""
    import torch
    from rgbd_pl_slam_amd import Sim3KeyFrames, Sim3Solver
    sc = G.make_scene(81, [dict(n1=80, pairs=60, outliers=0.4, scale=1.1)], max_iterations=60, max_hits=1)
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    kfs = Sim3KeyFrames([t(np.ascontiguousarray(k).view(np.uint8).reshape(-1)) for k in sc["kf_keys"]], [t(m) for m in sc["kf_mappoints"]], t(sc["kf_pose"]))
    cam = tuple(float(x) for x in sc["cam"][[0, 1, 2, 3, 9]])

    def solver():
        s = Sim3Solver(kfs, 0, 1, t(sc["match12"][0]), t(sc["world_pos"]), t(sc["point_bad"]), t(sc["level_sigma2"]), cam, False)
        s.SetRansacParameters(0.99, 20, 60, rand3=t(sc["rand3"][0]))
        return s

    _, _, ((_, h),) = G.ref_run(sc, [60])
    assert h["n_hits"][0] > 0
    k0, sim3 = int(h["hit_iter"][0, 0]), h["hit_sim3"][0, 0]
    s = solver()
    T, inl, n = s.find()
    want = (sim3[:9] * sim3[12]).reshape(3, 3)
    assert G.same_bits(T[:3, :3].numpy(), want) and G.same_bits(T[:3, 3].numpy(), sim3[9:12]) and n == h["hit_inliers"][0, 0]
    assert np.array_equal(np.flatnonzero(inl.numpy()), np.flatnonzero(h["hit_inlier12"][0, 0]))
    assert G.same_bits(s.GetEstimatedRotation().numpy().ravel(), sim3[:9]) and s.GetEstimatedScale() == sim3[12]
    # the rounds of LoopClosing::ComputeSim3: the hit arrives in the round that holds iteration k0, and the solver then stands AT k0
    s = solver()
    for rnd in range(1, 13):
        T, no_more, _, n = s.iterate(5)
        if T is not None:
            break
    assert rnd == (k0 + 4) // 5 and int(s._pairs.iterations_done[0]) == k0 and n == h["hit_inliers"][0, 0]


def test_chain_bow_pairs_iterate_sim3_search_on_one_stream():
    """plf_match_bow_kf -> plf_sim3_pairs -> plf_sim3_iterate -> (read hit_sim3) -> plf_match_sim3 on ONE stream, no host wait before the read: the rows the
    BoW search wrote are read where they lie.  Each stage against its own reference: the oracle's SearchByBoW and SearchBySim3, tests/sim3ref.py between."""
    import torch
    import kfgen
    import orc
    from rgbd_pl_slam_amd import Matcher, Sim3KeyFrames, sim3_pairs, sim3_iterate
    n = 600
    c = kfgen.two_keyframe_scene(5, n, nodes=60, s12=1.0, tz=0.3)
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    st = torch.cuda.Stream()
    has1, has2 = c["pts1"]["valid"], c["pts2"]["valid"]
    a1, a2 = np.ascontiguousarray(c["kps1"]["angle"]), np.ascontiguousarray(c["kps2"]["angle"])
    # the scene as tests/sim3ref.py reads it: the points of keyframe 1 are rows 0 .. n - 1 of the map, those of keyframe 2 rows n .. 2 n - 1
    ar = np.arange(n, dtype=np.int32)
    keys = [np.frombuffer(np.ascontiguousarray(c["kps" + s]).tobytes(), F32).reshape(n, 7).copy() for s in "12"]
    pose = np.array([np.concatenate([c["pose" + s]["Rcw"].ravel(), c["pose" + s]["tcw"], c["pose" + s]["Ow"]]) for s in "12"], F32)
    cam = np.array([c["fx"], c["fy"], c["cx"], c["cy"], 0, 0, 0, 0, 0, 40.0], F32)
    sc = dict(cam=cam, level_sigma2=np.ascontiguousarray(c["sigma2"], F32), kf_n=np.array([n, n], np.int32), kf_pose=pose, kf_keys=keys,
              kf_octave=[np.ascontiguousarray(c["kps" + s]["octave"], np.int32) for s in "12"],
              kf_mappoints=[np.where(has1 != 0, ar, -1).astype(np.int32), np.where(has2 != 0, ar + n, -1).astype(np.int32)], kf_obs_index=None,
              world_pos=np.concatenate([c["pts1"]["xw"], c["pts2"]["xw"]]).astype(F32), point_bad=np.zeros(2 * n, np.uint8), job_kf1=np.array([0], np.int32),
              job_kf2=np.array([1], np.int32), fix_scale=np.array([0], np.uint8), prob=0.99, min_inliers=20, max_iterations=300, pair_stride=n, max_hits=1,
              rand3=G.raw_values(3, (1, 300, 3)))
    # the references, stage by stage
    em, en = orc.search_by_bow_kf(c["desc1"], c["desc2"], a1, a2, has1, has2, c["nodes1"], c["nodes2"], 0.75, 1)
    sc["match12"] = np.ascontiguousarray(em, np.int32).reshape(1, n)
    ref = G.ref_run(sc, [300])
    assert ref[0]["n_pairs"][0] > 40 and ref[2][0][1]["n_hits"][0] > 0
    sim3 = ref[2][0][1]["hit_sim3"][0, 0]
    assert np.abs(sim3[:9].reshape(3, 3) - c["R12"]).max() < 0.05 and abs(sim3[12] - 1.0) < 0.05
    c2 = dict(c, s12=float(sim3[12]), R12=sim3[:9].reshape(3, 3).copy(), t12=sim3[9:12].copy(), th=7.5)
    fm, fn = orc.search_by_sim3(c2)
    # the device, one stream
    m = Matcher(max_keypoints=1024, max_mappoints=1024)
    ds = t(c["scale"])
    dk = [t(np.frombuffer(np.ascontiguousarray(c["kps" + s]).tobytes(), np.uint8).copy()) for s in "12"]
    dd = [t(c["desc1"]), t(c["desc2"])]
    nodes = [tuple(t(x) for x in c["nodes" + s]) for s in "12"]
    hm = [t(has1), t(has2)]
    da = [t(a1), t(a2)]                                                   # (kept: the view holds addresses only)
    view = Matcher.bow_view(dd[0], dd[1], da[0], da[1], hm[0], nodes[0], nodes[1], f_has_mp=hm[1])
    kfs = Sim3KeyFrames(dk, [t(x) for x in sc["kf_mappoints"]], t(pose))
    camt = (float(c["fx"]), float(c["fy"]), float(c["cx"]), float(c["cy"]), 40.0)
    with torch.cuda.stream(st):
        match = torch.full((1, n), -7, dtype=torch.int32, device=dev)
        nm = torch.zeros(1, dtype=torch.int32, device=dev)
        args = [t(sc[k]) for k in ("job_kf1", "job_kf2", "world_pos", "point_bad", "level_sigma2", "rand3", "fix_scale")]
        from rgbd_pl_slam_amd import sim3 as S3
        table = S3.its_for_n(0.99, 20, 300, n, dev)
    st.synchronize()                                                      # (the uploads; nothing below waits before the read of hit_sim3)
    m.SearchByBoWKeyFrames([view], 0.75, 1, match, n, nm, stream=st.cuda_stream)
    pr = sim3_pairs(kfs, args[0], args[1], match, args[2], args[3], args[4], camt, pair_stride=n, table=table, stream=st.cuda_stream)
    out = sim3_iterate(pr, args[5], 300, args[6], camt, min_inliers=20, max_hits=1, stream=st.cuda_stream)
    st.synchronize()
    assert int(nm[0]) == en and np.array_equal(match[0].cpu().numpy(), em)
    got = ({k: getattr(pr, k).cpu().numpy() for k in G.PAIR_KEYS}, {k: getattr(pr, k).cpu().numpy() for k in G.STATE_KEYS},
           [(out.count.cpu().numpy(), {k: getattr(out, k).cpu().numpy() for k in G.HIT_KEYS})])
    G.compare(ref, got, "chain")
    hs = out.hit_sim3[0, 0].cpu().numpy()
    views = [Matcher.frame_view(n, dk[i], dd[i], ds, (0.0, 0.0, 640.0, 480.0), None) for i in range(2)]
    pts = [dict(world_pos=t(c["pts" + s]["xw"]), normal=None, min_dist=t(c["pts" + s]["min_dist"]), max_dist=t(c["pts" + s]["max_dist"]), desc=t(c["pts" + s]["desc"]),
                valid=t(c["pts" + s]["valid"])) for s in "12"]
    match2 = torch.full((n,), -7, dtype=torch.int32, device=dev)
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    m.SearchBySim3(views[0], views[1], c["pose1"], c["pose2"], float(hs[12]), hs[:9].reshape(3, 3).copy(), hs[9:12].copy(), 7.5, pts[0], pts[1], match2, cnt, stream=st.cuda_stream)
    st.synchronize()
    assert fn > 20 and int(cnt[0]) == fn and np.array_equal(match2.cpu().numpy(), fm)
    m.close()

"""GPU parity under contention: the four greedy-order projection matchers on the crowded and chain scenes of tests/crowdgen.py -- bit-exact, no tolerances.

k_mp_candidates / k_mp_rounds, k_lf_candidates / k_lf_rounds and the fallbacks k_match_project_points_slow, k_match_lastframe and k_project_kf_greedy replay a
strictly sequential reference loop in parallel rounds.  That is exact only because two items decided in the same round can never want each other's key point,
an argument that matters only when items compete: here they do (tests/test_match_ref.py measures how much).  Expected values come from the oracle, which
test_match_ref.py holds equal to the plain restatement tests/matchref.py and to the reference binary's fixtures; on a mismatch, matchref's `log` argument lists
the sequential decision of every item.

PLF_MATCH_CAND_AVG is read when a matcher is created: the tests that set it do so before they construct theirs."""
import numpy as np
import pytest

import crowdgen as G
import orc
from conftest import gpu_available

pytestmark = pytest.mark.gpu

STRIDE = 512        # key point slots per frame of a batched call (>= every scene's key point count, sparse frames included)
MAP_PARAMS = [(th, nn) for th in (1.0, 3.0) for nn in (0.8, 1.0)]
MAP_SCENES = {**G.map_scenes(), **G.map_chains()}
LAST_SCENES = {**G.last_scenes(), **G.last_chains()}
KF_SCENES = {**G.keyframe_scenes(), **G.keyframe_chains()}
LAST_CASES = (("forward", 0), ("backward", 0), ("neither", 0), ("forward", 1))     # the three motion classes, and mono (which switches them off)


def _need_gpu():
    if not gpu_available():
        pytest.fail("no GPU visible: the -m gpu tests need a real MI355X")


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _kp_tensor(kps):
    import torch
    return torch.from_numpy(np.frombuffer(np.ascontiguousarray(kps).tobytes(), np.uint8).copy()).cuda()


def _free3(match):
    """the protocol of include/plf.h: on input -3 reads as free, and an untouched entry comes back as -1 (the oracle leaves it as it found it)"""
    return np.where(match == -3, -1, match)


class DevFrame:
    """a scene's frame on the device, padded to STRIDE key points"""

    def __init__(self, s, with_uright=True):
        from rgbd_pl_slam_amd import Matcher
        self.n = len(s["kps"])
        kps = np.zeros(STRIDE, s["kps"].dtype); kps[:self.n] = s["kps"]
        desc = np.zeros((STRIDE, 32), np.uint8); desc[:self.n] = s["desc"]
        self.t = [_kp_tensor(kps), _dev(desc), _dev(s["scale"]), _dev(np.array([self.n], np.int32))]
        self.ur = None
        if with_uright and s.get("uright") is not None:
            ur = np.full(STRIDE, -1, np.float32); ur[:self.n] = s["uright"]
            self.ur = _dev(ur)
        self.bounds = s["bounds"]
        self._view = Matcher.frame_view

    def view(self, through_device_counter=False):
        """through_device_counter: the host count is only an upper bound (all STRIDE slots), the true one is read on the device"""
        if through_device_counter:
            return self._view(STRIDE, self.t[0], self.t[1], self.t[2], self.bounds, self.ur, n_device=self.t[3])
        return self._view(self.n, self.t[0], self.t[1], self.t[2], self.bounds, self.ur)


def _init_rows(frames):
    init = np.full((len(frames), STRIDE), -1, np.int32)
    for f, s in enumerate(frames):
        init[f, :len(s["kps"])] = s["init"]
    return init


def _map_call(m, dframes, dmp, frames, th, nn, device_counter_frame=None):
    """one plf_match_project_points call; returns (match rows, nmatches)"""
    import torch
    match = _dev(_init_rows(frames)); nm = torch.full((len(frames),), -7, dtype=torch.int32, device="cuda")
    m.SearchByProjection([d.view(f == device_counter_frame) for f, d in enumerate(dframes)], dmp, th, nn, match, STRIDE, nm)
    torch.cuda.synchronize()
    return match.cpu().numpy(), nm.cpu().numpy()


def _check_map(got, frames, mp, th, nn, what):
    match, nm = got
    for f, s in enumerate(frames):
        ref, rn = orc.search_by_projection_map(s["kps"], s["desc"], s["uright"], s["scale"], s["bounds"], mp, th, nn, s["init"])
        n = len(s["kps"])
        assert int(nm[f]) == rn, (what, f, th, nn)
        assert np.array_equal(match[f, :n], _free3(ref)), (what, f, th, nn)
        assert (match[f, n:] == -1).all(), (what, f)      # slots past the frame's key points are not touched


@pytest.mark.parametrize("cand_avg", [None, "1"], ids=["cached_candidates", "pool_of_one_per_item"])
@pytest.mark.parametrize("name", list(MAP_SCENES))
def test_map_search_single_frame(monkeypatch, name, cand_avg):
    """plf_match_project_points, one frame: k_mp_candidates / k_mp_rounds on a handle whose pool holds the scene, and with PLF_MATCH_CAND_AVG=1 on a handle
    sized to the scene, so that the frame overflows, k_match_project_points_slow (test_match_ref.py::test_pool_sizes_put_every_scene_on_the_intended_kernels)"""
    _need_gpu()
    from rgbd_pl_slam_amd import Matcher
    if cand_avg:
        monkeypatch.setenv("PLF_MATCH_CAND_AVG", cand_avg)
    s = MAP_SCENES[name]
    m = Matcher(max_keypoints=STRIDE, max_mappoints=len(s["mp"]["desc"]) if cand_avg else G.CACHED_MAX_MAPPOINTS, max_batch=1)
    d = DevFrame(s); dmp = {k: _dev(v) for k, v in s["mp"].items()}
    for th, nn in MAP_PARAMS:
        _check_map(_map_call(m, [d], dmp, [s], th, nn), [s], s["mp"], th, nn, name)
    m.close()


@pytest.mark.parametrize("cand_avg", [None, "1"], ids=["cached_candidates", "pool_of_one_per_item"])
@pytest.mark.parametrize("name", list(MAP_SCENES))
def test_map_search_batch_of_three_scenes(monkeypatch, name, cand_avg):
    """the frames of three different scenes against the map of the first; the second frame passes its key point count through the device-side counter, with a
    host count of all STRIDE slots"""
    _need_gpu()
    from rgbd_pl_slam_amd import Matcher
    if cand_avg:
        monkeypatch.setenv("PLF_MATCH_CAND_AVG", cand_avg)
    names = list(MAP_SCENES)
    at = names.index(name)
    mp = MAP_SCENES[name]["mp"]
    frames = [MAP_SCENES[name]] + [G.remap_for_map(MAP_SCENES[names[(at + k) % len(names)]], mp) for k in (1, 3)]
    m = Matcher(max_keypoints=STRIDE, max_mappoints=len(mp["desc"]) if cand_avg else G.CACHED_MAX_MAPPOINTS, max_batch=3)
    dframes = [DevFrame(s) for s in frames]; dmp = {k: _dev(v) for k, v in mp.items()}
    for th, nn in MAP_PARAMS:
        _check_map(_map_call(m, dframes, dmp, frames, th, nn, device_counter_frame=1), frames, mp, th, nn, name)
    m.close()


def test_map_search_one_frame_overflows_between_two_that_do_not(monkeypatch):
    """one call, three frames: the crowded one in the middle overflows its candidate pool and is finished by k_match_project_points_slow, its sparse neighbours
    stay with k_mp_rounds (test_match_ref.py::test_mixed_overflow_calls_split_as_intended holds the split); every frame equals its own single-frame reference"""
    _need_gpu()
    from rgbd_pl_slam_amd import Matcher
    c = G.mixed_map_call()
    monkeypatch.setenv("PLF_MATCH_CAND_AVG", str(c["cand_avg"]))
    m = Matcher(max_keypoints=STRIDE, max_mappoints=c["max_mappoints"], max_batch=3)
    dframes = [DevFrame(s) for s in c["frames"]]; dmp = {k: _dev(v) for k, v in c["mp"].items()}
    for rep in range(2):      # the second call finds the flags and the pool fill of the first
        _check_map(_map_call(m, dframes, dmp, c["frames"], c["th"], c["nnratio"], device_counter_frame=0), c["frames"], c["mp"], c["th"], c["nnratio"], "mixed")
    m.close()


# ---------------------------------------------------------------- last frame
def _dev_last(last):
    return dict(keys=_kp_tensor(last["keys"]), has_mappoint=_dev(last["has_mappoint"]), outlier=_dev(last["outlier"]), world_pos=_dev(last["world_pos"]),
                mp_desc=_dev(last["mp_desc"]), obs_positive=_dev(last["obs_positive"]))


def _last_refs(frames, last, poses, th, mono):
    """per frame the oracle's (match, n) without the rotation check and with it"""
    out = []
    for s, pose in zip(frames, poses):
        a = (s["kps"], s["desc"], s["uright"], s["scale"], s["bounds"], last, pose, th, mono)
        out.append((orc.search_by_projection_last(*a, 0, s["init"]), orc.search_by_projection_last(*a, 1, s["init"])))
    return out


def _check_last(got_by_ori, frames, refs, what):
    """check_orientation 0 and 1 equal the oracle; 2 equals 1 except that -3 stands exactly where 0 has an assignment and 1 has none"""
    for f, s in enumerate(frames):
        n = len(s["kps"])
        (r0, n0), (r1, n1) = refs[f]
        g0, g1, g2 = (got_by_ori[o][0][f, :n] for o in (0, 1, 2))
        assert int(got_by_ori[0][1][f]) == n0 and np.array_equal(g0, _free3(r0)), (what, f, "check_orientation 0")
        assert int(got_by_ori[1][1][f]) == n1 and np.array_equal(g1, _free3(r1)), (what, f, "check_orientation 1")
        assert int(got_by_ori[2][1][f]) == n1, (what, f, "check_orientation 2")
        culled = (g0 >= 0) & (g1 < 0)
        assert np.array_equal(g2 == -3, culled) and np.array_equal(np.where(culled, g1, g2), g1), (what, f, "check_orientation 2")
        for o in (0, 1, 2):
            assert (got_by_ori[o][0][f, n:] == -1).all(), (what, f)


def _last_calls(m, dframes, dlast, frames, poses, th, mono, single):
    import torch
    from rgbd_pl_slam_amd import Matcher
    got = {}
    for ori in (0, 1, 2):
        match = _dev(_init_rows(frames)); nm = torch.full((len(frames),), -7, dtype=torch.int32, device="cuda")
        if single:
            m.SearchByProjectionLastFrame(dframes[0].view(), dlast, poses[0], th, mono, ori, match, nm)
        else:
            m.SearchByProjectionLastFrameBatch([d.view(f == 1) for f, d in enumerate(dframes)], Matcher.last_view(dlast), poses, th, mono, ori, match, STRIDE, nm)
        torch.cuda.synchronize()
        got[ori] = (match.cpu().numpy(), nm.cpu().numpy())
    return got


def _last_matcher(monkeypatch, s, cand_avg):
    from rgbd_pl_slam_amd import Matcher
    if cand_avg:
        monkeypatch.setenv("PLF_MATCH_CAND_AVG", cand_avg)
    n_last = len(s["last"]["mp_desc"])
    return Matcher(max_keypoints=max(STRIDE, n_last), max_mappoints=n_last if cand_avg else G.CACHED_MAX_MAPPOINTS, max_batch=3)


@pytest.mark.parametrize("cand_avg", [None, "1"], ids=["cached_candidates", "pool_of_one_per_item"])
@pytest.mark.parametrize("name", list(LAST_SCENES))
def test_lastframe_search_single_frame(monkeypatch, name, cand_avg):
    """plf_match_project_lastframe for the three motion classes and mono: k_lf_candidates / k_lf_rounds, and with PLF_MATCH_CAND_AVG=1 (the frame overflows)
    the motion-model branch of k_match_lastframe"""
    _need_gpu()
    s = LAST_SCENES[name]
    m = _last_matcher(monkeypatch, s, cand_avg)
    dlast = _dev_last(s["last"])
    d = DevFrame(s)
    for motion, mono in LAST_CASES:
        pose = G.lf_pose(motion)
        _check_last(_last_calls(m, [d], dlast, [s], [pose], 15.0, mono, True), [s], _last_refs([s], s["last"], [pose], 15.0, mono), (name, motion, mono))
    m.close()


@pytest.mark.parametrize("cand_avg", [None, "1"], ids=["cached_candidates", "pool_of_one_per_item"])
@pytest.mark.parametrize("name", list(LAST_SCENES))
def test_lastframe_search_batch_of_three_poses(monkeypatch, name, cand_avg):
    """plf_match_project_lastframe_batch: three frames with three different poses (the scene's key points, its pre-set entries rotated per frame), the second
    counted on the device"""
    _need_gpu()
    s = LAST_SCENES[name]
    m = _last_matcher(monkeypatch, s, cand_avg)
    dlast = _dev_last(s["last"])
    d = DevFrame(s)
    frames = [dict(s, init=np.roll(s["init"], 7 * f)) for f in range(3)]
    poses = [G.lf_pose(mo) for mo in ("backward", "neither", "forward")]
    for th, mono in ((15.0, 0), (7.0, 1)):
        got = _last_calls(m, [d, d, d], dlast, frames, poses, th, mono, False)
        _check_last(got, frames, _last_refs(frames, s["last"], poses, th, mono), (name, "batch", th, mono))
    m.close()


def test_lastframe_search_one_frame_overflows_between_two_that_do_not(monkeypatch):
    """one batched call: the crowded frame in the middle is left to k_match_lastframe, the sparse ones stay with k_lf_rounds"""
    _need_gpu()
    from rgbd_pl_slam_amd import Matcher
    c = G.mixed_last_call()
    monkeypatch.setenv("PLF_MATCH_CAND_AVG", str(c["cand_avg"]))
    m = Matcher(max_keypoints=c["max_keypoints"], max_mappoints=c["max_mappoints"], max_batch=3)
    dframes = [DevFrame(s) for s in c["frames"]]; dlast = _dev_last(c["last"])
    refs = _last_refs(c["frames"], c["last"], c["poses"], c["th"], c["mono"])
    for rep in range(2):
        _check_last(_last_calls(m, dframes, dlast, c["frames"], c["poses"], c["th"], c["mono"], False), c["frames"], refs, "mixed")
    m.close()


# ---------------------------------------------------------------- keyframe (relocalisation) and Sim3 overloads
@pytest.mark.parametrize("name", list(KF_SCENES))
def test_keyframe_and_sim3_search(name):
    """plf_match_project_sim3 (k_project_kf_greedy) and plf_match_project_keyframe (the relocalisation branch of k_match_lastframe) on the clustered keyframe
    scenes, with occupied and pre-set entries, and on a chain scene each"""
    _need_gpu()
    import torch
    from rgbd_pl_slam_amd import Matcher
    s = KF_SCENES[name]
    p = s["pts"]; nk = len(s["kps"]); m_items = len(p["desc"])
    mt = Matcher(max_keypoints=max(STRIDE, m_items), max_mappoints=m_items)
    d = DevFrame(s, with_uright=False)
    dp = dict(world_pos=_dev(p["xw"]), normal=_dev(p["normal"]), min_dist=_dev(p["min_dist"]), max_dist=_dev(p["max_dist"]), desc=_dev(p["desc"]), valid=_dev(p["valid"]))
    cnt = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    for th in (3, 8):
        match = _dev(s["init"])
        mt.SearchByProjectionSim3(d.view(), s["Scw"], s["intr"], dp, th, match, cnt); torch.cuda.synchronize()
        em, en = orc.search_by_projection_sim3(s["kps"], s["desc"], s["scale"], s["bounds"], s["Scw"], s["intr"], p, th, s["init"])
        assert en > 20 and int(cnt[0]) == en and np.array_equal(match.cpu().numpy(), em), (name, th)
    kf, rl = s["kf"], s["reloc"]
    dkf = dict(keys=_kp_tensor(kf["keys"]), valid=_dev(kf["valid"]), world_pos=_dev(kf["world_pos"]), min_dist=_dev(kf["min_dist"]), max_dist=_dev(kf["max_dist"]),
               mp_desc=_dev(kf["mp_desc"]))
    for ori in (0, 1):
        match = _dev(s["init"])
        mt.SearchByProjectionKeyFrame(d.view(), dkf, rl["pose"], rl["logsf"], rl["th"], rl["orbdist"], ori, match, cnt); torch.cuda.synchronize()
        em, en = orc.search_by_projection_reloc(s["kps"], s["desc"], s["scale"], s["bounds"], kf, rl["pose"], rl["logsf"], rl["th"], rl["orbdist"], ori, s["init"])
        assert en > 10 and int(cnt[0]) == en and np.array_equal(match.cpu().numpy(), em), (name, "relocalisation", ori)
    mt.close()


# ---------------------------------------------------------------- one handle, call after call
@pytest.mark.parametrize("cand_avg", [None, "8"], ids=["cached_candidates", "crowded_call_overflows"])
def test_handle_reuse_crowded_sparse_crowded(monkeypatch, cand_avg):
    """one matcher runs a crowded call, a sparse call and the crowded call again, for the map search and for the last-frame search: the third result equals the
    first (and the oracle) -- nothing of the pool fill, the overflow flags, the `done` rows or the top-2 rows survives a call"""
    _need_gpu()
    from rgbd_pl_slam_amd import Matcher
    if cand_avg:
        monkeypatch.setenv("PLF_MATCH_CAND_AVG", cand_avg)
    c = G.mixed_map_call()
    sparse, crowded = c["frames"][0], c["frames"][1]
    m = Matcher(max_keypoints=3000, max_mappoints=3000, max_batch=2)
    ds, dc = DevFrame(sparse), DevFrame(crowded)
    dmp = {k: _dev(v) for k, v in c["mp"].items()}
    runs = []
    for fr, dfr in ((crowded, dc), (sparse, ds), (crowded, dc)):
        runs.append(_map_call(m, [dfr, dfr], dmp, [fr, fr], c["th"], c["nnratio"], device_counter_frame=1))
        _check_map(runs[-1], [fr, fr], c["mp"], c["th"], c["nnratio"], "reuse")
    assert np.array_equal(runs[0][0], runs[2][0]) and np.array_equal(runs[0][1], runs[2][1])
    c = G.mixed_last_call()
    sparse, crowded = c["frames"][0], c["frames"][1]
    ds, dc = DevFrame(sparse), DevFrame(crowded)
    dlast = _dev_last(c["last"])
    runs = []
    for fr, dfr, pose in ((crowded, dc, c["poses"][1]), (sparse, ds, c["poses"][0]), (crowded, dc, c["poses"][1])):
        runs.append(_last_calls(m, [dfr, dfr], dlast, [fr, fr], [pose, pose], c["th"], c["mono"], False))
        _check_last(runs[-1], [fr, fr], _last_refs([fr, fr], c["last"], [pose, pose], c["th"], c["mono"]), "reuse")
    for ori in (0, 1, 2):
        assert np.array_equal(runs[0][ori][0], runs[2][ori][0]) and np.array_equal(runs[0][ori][1], runs[2][ori][1])
    m.close()

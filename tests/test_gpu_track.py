"""plf_track_close_points / plf_track_need_keyframe / plf_track_motion / plf_track_clean on the device against the definition tests/trackref.py, BIT FOR
BIT: the lists, the counts, the status words and every float as its uint32 view.  No tolerance and no excluded case; a NaN compares equal to any NaN."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import posegen  # noqa: E402
import poseref  # noqa: E402
import trackgen as G  # noqa: E402
import trackref as R  # noqa: E402
import test_track_ref as T  # noqa: E402  (the scenes both suites run)

import torch  # noqa: E402
from conftest import gpu_available  # noqa: E402

pytestmark = pytest.mark.gpu

from rgbd_pl_slam_amd import _lib as L  # noqa: E402
from rgbd_pl_slam_amd import close_points, need_new_keyframe, motion_model, clean_matches, pose_optimization, pose_commit  # noqa: E402
from rgbd_pl_slam_amd.pose import camera  # noqa: E402

FIXTURES = T.FIXTURES
_refs = {}


@pytest.fixture(autouse=True)
def _need_gpu():
    if not gpu_available():
        pytest.fail("no GPU visible: the -m gpu tests need a real MI355X")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ref_of(name):
    """the definition's result for a fixture, computed once per process and left unchanged"""
    if name not in _refs:
        p, kw = FIXTURES[name]
        _refs[name] = G.ref_close(p, **kw)
    return _refs[name]


# ---- close_points
@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_close_points(name):
    """every fixture of tests/trackgen.py: the entry counts at the lane / wave / padding / size-class edges, per-frame n in one call, the depth and match
    cases, the short list and key-frame mode"""
    p, kw = FIXTURES[name]
    want = ref_of(name)
    got = G.dev_close(p, **kw)
    G.assert_close_equal(got, want, name)
    ns = got["new_kp"].shape[1]
    for f in range(len(want["n_new"])):                          # nothing is written beyond min(count, stride)
        k = min(int(want["n_new"][f]), ns)
        assert np.all(got["new_kp"][f, k:] == -1) and not got["new_pos"][f, k:].any(), name
    if name.startswith("short_list"):
        assert want["status"].all() and (want["n_new"] > ns).all()


def test_close_points_n_host():
    """n from the host for every frame, and a frame count beyond one wave of workgroups"""
    fr = [G.make_frame(300 + k, 100, stride=100) for k in range(70)]
    p = G.pack(fr)
    G.assert_close_equal(G.dev_close(p, n_host=100), G.ref_close(p), "n_host")


def test_close_points_last_frame_mode_feeds_the_matcher():
    """last-frame mode writes the temporal points into the arrays behind a plf_lastframe_view; plf_match_project_lastframe on them gives what it gives on
    arrays built on the host from the definition"""
    from rgbd_pl_slam_amd import Matcher
    rng = np.random.default_rng(77)
    n = 150
    fr = G.make_frame(78, n, match_frac=0.4)
    fr["keys"]["angle"] = rng.uniform(0, 360, n).astype(np.float32)
    fr["keys"]["octave"] = rng.integers(0, 3, n)
    fr["keys"]["x"] = rng.uniform(40, 600, n).astype(np.float32)
    fr["keys"]["y"] = rng.uniform(40, 440, n).astype(np.float32)
    p = G.pack([fr])
    last0 = G.last_arrays(p, 1)
    want = G.ref_close(p, last=last0)
    got = G.dev_close(p, last=last0)
    G.assert_close_equal(got, want, "last-frame mode")
    assert want["n_new"][0] > 20 and (want["last"][2][0] == 0).sum() == want["n_new"][0]
    created = want["new_kp"][0, :want["n_new"][0]]
    untouched = np.setdiff1d(np.arange(n), created)
    assert np.array_equal(got["last"][1][0, untouched], last0[1][0, untouched]) and np.array_equal(got["last"][0][0, untouched], last0[0][0, untouched])
    # one tiny frame pair: the current frame sees the last frame's key points from the same pose
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    cur_desc = desc.copy()
    cur_desc[:, 0] ^= rng.integers(0, 4, n, dtype=np.uint8)
    scale = (1.2 ** np.arange(8)).astype(np.float32)
    fp = fr["frustum"]
    fx, fy, cx, cy, bf = G.CAM
    pose = dict(Rcw=fp[:9], tcw=fp[9:12], Rlw=fp[:9], tlw=fp[9:12], fx=fx, fy=fy, cx=cx, cy=cy, bf=bf, b=bf / fx)
    keys = dev(np.frombuffer(p["keys"][0].tobytes(), np.uint8).copy())
    m = Matcher(max_keypoints=256)
    res = []
    for arrays in (got["last"], want["last"]):
        last = dict(keys=keys, has_mappoint=dev(arrays[0][0]), outlier=dev(np.zeros(n, np.uint8)), world_pos=dev(arrays[1][0]), mp_desc=dev(desc),
                    obs_positive=dev(arrays[2][0]))
        cur = Matcher.frame_view(n, keys, dev(cur_desc), dev(scale), (0.0, 0.0, 640.0, 480.0), dev(np.full(n, -1, np.float32)))
        match = dev(np.full(n, -1, np.int32)); nm = torch.zeros(1, dtype=torch.int32, device="cuda")
        m.SearchByProjectionLastFrame(cur, last, pose, 7.0, 0, 1, match, nm)
        torch.cuda.synchronize()
        res.append((match.cpu().numpy(), int(nm[0])))
    m.close()
    assert np.array_equal(res[0][0], res[1][0]) and res[0][1] == res[1][1]
    assert np.isin(created, res[0][0]).sum() > 10             # the temporal points are matched


# ---- need_new_keyframe
def run_need(t, n=None, n_inliers=None, item_bad=None, row_id=None):
    state = dev(t["state"].view(np.uint8).reshape(len(t["state"]), -1))
    r = need_new_keyframe(dev(t["depth"]), dev(t["match"]), dev(t["n_obs"]), dev(t["kf_row_start"]), dev(t["kf_row_item"]), state, float(t["th_depth"]),
                          n_inliers=dev(n_inliers) if n_inliers is not None else None, item_bad=dev(item_bad) if item_bad is not None else None,
                          n=dev(n) if n is not None else None, row_id=dev(row_id) if row_id is not None else None)
    torch.cuda.synchronize()
    return r.counts.cpu().numpy(), r.decision.cpu().numpy()


def test_need_keyframe_truth_table():
    rows = G.truth_table()
    want = np.array([R.decide(*r) for r in rows], np.int32)
    counts, dec = run_need(T._table_frames(rows))
    assert np.array_equal(counts, np.array([[r[2], r[3], r[4]] for r in rows]))
    assert np.array_equal(dec, want), np.nonzero(dec != want)[0][:10]


def test_need_keyframe_reference_row():
    """a reference key frame's row with null, bad and out-of-range entries, nMinObs 2 and 3, a ref_kf outside the key frames, a row_id map, per-frame n"""
    t = T.need_scene()
    counts, dec = T.ref_need(t)
    c2, d2 = run_need(t, n=t["n"], n_inliers=t["n_inliers"], item_bad=t["item_bad"], row_id=t["row_id"])
    assert np.array_equal(counts, c2) and np.array_equal(dec, d2)
    counts, dec = T.ref_need(dict(t, item_bad=None), use_inliers=False)
    c2, d2 = run_need(t, n=t["n"], row_id=t["row_id"])
    assert np.array_equal(counts, c2) and np.array_equal(dec, d2)


# ---- motion_model / clean_matches
def test_motion_model():
    """1, 64 and 65 frames, each flag combination; non-finite poses set the status bit and fault nothing"""
    for case in T.motion_cases():
        want = T.ref_motion(case)
        r = motion_model(**{k: (dev(v) if isinstance(v, np.ndarray) else v) for k, v in case.items()})
        torch.cuda.synchronize()
        assert np.array_equal(r.status.cpu().numpy(), want["status"])
        for k in want:
            if k != "status":
                assert G.same_bits(getattr(r, k).cpu().numpy(), want[k]), (sorted(case), k)


@pytest.mark.parametrize("mode", ["vo", "outliers"])
def test_clean_matches(mode):
    for Fn, rid in ((1, False), (64, True), (65, False)):
        p = G.pack([G.make_frame(500 + k, 100, stride=110, row_id=rid, match_frac=0.7) for k in range(Fn)])
        flags = (np.random.default_rng(Fn).random(p["match"].shape) < 0.4).astype(np.uint8)
        m1, f1 = p["match"].copy(), flags.copy()
        for f in range(Fn):
            R.clean_matches(mode, m1[f], f1[f], int(p["n"][f]), p["n_obs"], p["row_id"][f] if rid else None)
        dm, df = dev(p["match"]), dev(flags)
        clean_matches(mode, dm, df, n_obs=dev(p["n_obs"]) if mode == "vo" else None, row_id=dev(p["row_id"]) if rid else None, n=dev(p["n"]))
        torch.cuda.synchronize()
        assert np.array_equal(dm.cpu().numpy(), m1) and np.array_equal(df.cpu().numpy(), f1)
        assert not np.array_equal(m1, p["match"])


# ---- the whole tail of a tracked frame on one stream
def chain_scene():
    """the scene of the chain test and the definitions chained on the host (tests/poseref.py, then tests/trackref.py)"""
    Fn, nk, ne = 4, 200, 120
    rng = np.random.default_rng(900)
    frames = [posegen.make_frame(900 + k, nk, ne, "stereo", 0.15, noise_px=0.5) for k in range(Fn)]
    p = posegen.pack(frames, sentinel=False)
    P = p["pos_stride"]
    row_id = (np.arange(Fn)[:, None] * P + np.arange(P)[None, :]).astype(np.int32)
    n_obs = rng.integers(0, 4, Fn * P).astype(np.int32)
    depth = (rng.uniform(0.3, 2.5, (Fn, nk)) * float(G.TH_DEPTH)).astype(np.float32)
    depth[rng.random((Fn, nk)) < 0.1] = 0
    last_pose = np.stack([G.pose12(rng) for _ in range(Fn)])
    last_fr = np.stack([R.frustum(q) for q in last_pose])
    id_base = np.array([10000, 20000, 30000, 40000], np.int32)
    kf_row_start = np.array([0, 800], np.int32)
    kf_row_item = rng.integers(0, Fn * P, 800).astype(np.int32)
    states = [G.state(ref_kf=0, frame_id=100 + k, last_kf_id=(60, 95, 60, 95)[k], flags=(R.MAPPER_IDLE, 0)[k // 2]) for k in range(Fn)]
    srec = G.state_records(states)
    # the host chain
    want = []
    for f in range(Fn):
        ref = posegen.ref_frame(frames[f], poseref)
        assert ref["status"] == 0
        match = frames[f]["match"].copy()
        flags = np.zeros(nk, np.uint8)
        flags[match >= 0] = ref["outlier"][match >= 0]
        n_inl = sum(1 for i in range(nk) if match[i] >= 0 and not flags[i] and n_obs[row_id[f, match[i]]] > 0)
        R.clean_matches("vo", match, flags, nk, n_obs, row_id[f])
        counts, dec = R.need_new_keyframe(depth[f], match, nk, n_obs, kf_row_start, kf_row_item, None, states[f], G.TH_DEPTH, n_inl, row_id[f])
        fr = poseref.frustum_pose(ref["pose"])
        kxy = np.stack([frames[f]["keys"]["x"], frames[f]["keys"]["y"]], 1)
        kp, pos, walked = R.close_points(kxy, depth[f], match, nk, n_obs, fr, G.CAM, G.TH_DEPTH, 100, row_id[f])
        match[kp] = id_base[f] + np.arange(len(kp), dtype=np.int32)
        R.clean_matches("outliers", match, flags, nk)
        mo = R.motion_model(cur=ref["pose"], last_frustum=last_fr[f], last=ref["pose"], predict=True)
        want.append(dict(pose=ref["pose"], n_inl=n_inl, counts=counts, dec=dec, kp=kp, pos=pos, walked=walked, match=match, flags=flags, mo=mo))
    assert {w["dec"] for w in want} >= {1, 2} and all(len(w["kp"]) > 10 for w in want)
    return dict(Fn=Fn, nk=nk, p=p, row_id=row_id, n_obs=n_obs, depth=depth, last_fr=last_fr, id_base=id_base, kf_row_start=kf_row_start,
                kf_row_item=kf_row_item, srec=srec), want


def test_chain_from_pose_to_motion():
    """four frames x 200 key points: plf_pose_optimize -> plf_pose_commit -> clean -> need_keyframe -> close_points -> clean -> motion enqueued on one
    stream with no read-back until the end, against the definitions chained on the host"""
    sc, want = chain_scene()
    Fn, p, row_id, n_obs, depth, last_fr, id_base = sc["Fn"], sc["p"], sc["row_id"], sc["n_obs"], sc["depth"], sc["last_fr"], sc["id_base"]
    kf_row_start, kf_row_item, srec = sc["kf_row_start"], sc["kf_row_item"], sc["srec"]
    # the device chain: one stream, nothing read back until the end
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        keys = dev(np.frombuffer(p["keys"].tobytes(), np.uint8).reshape(Fn, -1).copy())
        match = dev(p["match"])
        d_nobs, d_rid, d_depth = dev(n_obs), dev(row_id), dev(depth)
        args = dict(stream=s.cuda_stream)
        r = pose_optimization(keys, dev(p["uright"]), match, dev(p["world_pos"]), dev(posegen.INV_SIGMA2), camera(*posegen.CAM), dev(p["pose_in"]), **args)
        n_inl = pose_commit("found", match, r.outlier, n_obs=d_nobs, row_id=d_rid, **args)
        clean_matches("vo", match, r.outlier, n_obs=d_nobs, row_id=d_rid, **args)
        nk_r = need_new_keyframe(d_depth, match, d_nobs, dev(kf_row_start), dev(kf_row_item), dev(srec.view(np.uint8).reshape(Fn, -1)), float(G.TH_DEPTH),
                                 n_inliers=n_inl, row_id=d_rid, **args)
        cp = close_points(keys, d_depth, match, d_nobs, r.frustum, G.CAM, float(G.TH_DEPTH), row_id=d_rid, id_base=dev(id_base), **args)
        clean_matches("outliers", match, r.outlier, **args)
        mo = motion_model(cur=r.pose, last_frustum=dev(last_fr), last=r.pose, predict=True, **args)
    s.synchronize()
    host = lambda t: t.cpu().numpy()
    for f, w in enumerate(want):
        assert G.same_bits(host(r.pose)[f], w["pose"]) and int(host(n_inl)[f]) == w["n_inl"], f
        assert list(host(nk_r.counts)[f]) == list(w["counts"]) and int(host(nk_r.decision)[f]) == w["dec"], f
        k = len(w["kp"])
        assert int(host(cp.n_new)[f]) == k and int(host(cp.n_walked)[f]) == w["walked"] and np.array_equal(host(cp.new_kp)[f, :k], w["kp"]), f
        assert G.same_bits(host(cp.new_pos)[f, :k], w["pos"]), f
        assert np.array_equal(host(match)[f], w["match"]) and np.array_equal(host(r.outlier)[f], w["flags"]), f
        for key in ("velocity", "pose_pred", "frustum_pred"):
            assert G.same_bits(host(getattr(mo, key))[f], w["mo"][key]), (f, key)

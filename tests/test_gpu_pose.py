"""plf_pose_optimize / plf_pose_commit on the device against the definition tests/poseref.py, BIT FOR BIT: the pose as uint32 views, the outlier flags,
the inlier counts and the status words.  No tolerance and no excluded case; the one normalisation is that a NaN compares equal to a NaN whatever its
sign and payload (IEEE leaves those to the implementation; the positions of the NaNs must coincide)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import posegen  # noqa: E402
import poseref  # noqa: E402

import torch  # noqa: E402
from conftest import gpu_available  # noqa: E402

pytestmark = pytest.mark.gpu

from rgbd_pl_slam_amd import _lib as L  # noqa: E402
from rgbd_pl_slam_amd import pose_optimization, pose_commit  # noqa: E402
from rgbd_pl_slam_amd.pose import camera  # noqa: E402

SENTINEL = 0xAB
_refs = {}


@pytest.fixture(autouse=True)
def _need_gpu():
    if not gpu_available():
        pytest.fail("no GPU visible: the -m gpu tests need a real MI355X")


def ref_of(key, frame):
    """the definition's result for one frame, computed once per process"""
    if key not in _refs:
        _refs[key] = posegen.ref_frame(frame, poseref)
    return _refs[key]


def same_bits(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


def run_gpu(p, n_mode="device", stream=None, pose_on="device", outlier=None):
    F, S = p["match"].shape
    dev = "cuda"
    keys = torch.from_numpy(np.frombuffer(np.ascontiguousarray(p["keys"]).tobytes(), np.uint8).copy()).to(dev)
    uright = torch.from_numpy(np.ascontiguousarray(p["uright"])).to(dev)
    match = torch.from_numpy(np.ascontiguousarray(p["match"])).to(dev)
    world = torch.from_numpy(p["world_pos"][0] if p["pos_stride"] == 0 else p["world_pos"]).to(dev).contiguous()
    sig = torch.from_numpy(posegen.INV_SIGMA2).to(dev)
    flags = torch.from_numpy(np.full((F, S), SENTINEL, np.uint8) if outlier is None else outlier).to(dev)
    n = torch.from_numpy(p["n"]).to(dev) if n_mode == "device" else int(p["n"][0])
    pin = torch.from_numpy(p["pose_in"]).to(dev) if pose_on == "device" else p["pose_in"]
    r = pose_optimization(keys, uright, match, world, sig, camera(*posegen.CAM), pin, n=n, outlier=flags, stream=stream)
    torch.cuda.synchronize()
    return dict(pose=r.pose.cpu().numpy(), frustum=r.frustum.cpu().numpy(), outlier=r.outlier.cpu().numpy(), n_inliers=r.n_inliers.cpu().numpy(),
                status=r.status.cpu().numpy())


def check(frames, keys, res, outlier_before=None):
    F = len(frames)
    for i, (f, k) in enumerate(zip(frames, keys)):
        ref = ref_of(k, f)
        nk = len(f["match"])
        assert same_bits(res["pose"][i], ref["pose"]), "pose of frame %d (%r)" % (i, k)
        assert int(res["n_inliers"][i]) == ref["n_inliers"] and int(res["status"][i]) == ref["status"], "count / status of frame %d (%r)" % (i, k)
        want = np.full(res["outlier"].shape[1], SENTINEL, np.uint8) if outlier_before is None else outlier_before[i].copy()
        if ref["status"] != poseref.STATUS_EARLY:
            m = np.flatnonzero(f["match"] >= 0)
            want[m] = ref["outlier"][m]
        assert np.array_equal(res["outlier"][i], want), "flags of frame %d (%r)" % (i, k)
        assert same_bits(res["frustum"][i], poseref.frustum_pose(res["pose"][i])), "frustum pose of frame %d" % i
        assert nk <= res["outlier"].shape[1]
    assert res["pose"].shape[0] == F


EDGE_COUNTS = [0, 1, 2, 3, 9, 10, 26, 27, 28, 63, 64, 65, 127, 128, 129, 191, 192, 193]     # POSE_CHUNK = 64: 63 / 64 / 65 are the chunk size -1 / 0 / +1


@pytest.mark.parametrize("mix", ["mono", "stereo", "alt"])
def test_edge_counts_and_mixes(mix):
    """every edge count around the thresholds of the routine (3, 10) and of the schedule (the 27 accumulator lanes, the 64-lane chunk), with key points
    beyond the matches, padded strides filled with sentinels that must come back untouched"""
    frames = [posegen.make_frame(100 + ne, ne + 37, ne, mix, 0.15, noise_px=0.5) for ne in EDGE_COUNTS]
    keys = [("cnt", mix, ne) for ne in EDGE_COUNTS]
    p = posegen.pack(frames, kp_stride=max(EDGE_COUNTS) + 37 + 19)
    check(frames, keys, run_gpu(p))


def test_matches_fill_whole_chunks():
    """every key point matched: N = edges = 64, 128, 65"""
    ns = [64, 128, 65, 63]
    frames = [posegen.make_frame(300 + n, n, n, "rand", 0.1, noise_px=0.5) for n in ns]
    check(frames, [("full", n) for n in ns], run_gpu(posegen.pack(frames)))


def test_more_matches_than_the_lds_list_holds():
    """POSE_LIST = 1024 matched key points are walked through their compacted list, more through all key points: 1023 / 1024 / 1025 edges, and the
    same 1025 edges among twice as many key points"""
    shapes = [(1023 + 40, 1023), (1024 + 40, 1024), (1025 + 40, 1025), (2100, 1025)]
    frames = [posegen.make_frame(400 + k, nk, ne, "alt", 0.1, noise_px=0.5) for k, (nk, ne) in enumerate(shapes)]
    check(frames, [("list", s) for s in shapes], run_gpu(posegen.pack(frames)))


def _varied(i):
    ne = (i * 7) % 30
    return posegen.make_frame(1000 + i % 97, 40, ne, ("mono", "stereo", "alt", "rand")[i % 4], (i % 5) * 0.1, noise_px=0.5, init_seed=i, rot_deg=1.0 + i % 3)


@pytest.mark.parametrize("n_frames", [1, 2, 63, 64, 65, 1000])
@pytest.mark.parametrize("n_mode", ["device", "host"])
def test_frame_counts(n_frames, n_mode):
    """a different edge count, pose and outlier share per frame; N from n_device and from n_host; world_pos per frame"""
    frames = [_varied(i) for i in range(n_frames)]
    check(frames, [("var", i) for i in range(n_frames)], run_gpu(posegen.pack(frames), n_mode=n_mode))


def test_shared_world_and_host_pose():
    """pos_stride 0: one world_pos array for every frame (frames of one scene with their own start poses and match subsets); pose_in from host memory"""
    frames = [posegen.make_frame(77, 90, 70, "alt", 0.1, noise_px=0.5, init_seed=i, drop=0.3) for i in range(65)]
    keys = [("shared", i) for i in range(65)]
    check(frames, keys, run_gpu(posegen.pack(frames, shared_pos=True), pose_on="host"))


def test_placement():
    """every frame's result equals that frame run alone in a call"""
    frames = [_varied(i) for i in range(65)]
    whole = run_gpu(posegen.pack(frames))
    S = whole["outlier"].shape[1]
    for i, f in enumerate(frames):
        alone = run_gpu(posegen.pack([f], kp_stride=S))
        for k in ("pose", "frustum"):
            assert same_bits(alone[k][0], whole[k][i]), (k, i)
        for k in ("outlier", "n_inliers", "status"):
            assert np.array_equal(alone[k][0], whole[k][i]), (k, i)


def test_control_flow_fixtures():
    fx = posegen.fixtures()
    names = sorted(fx)
    frames = [fx[k] for k in names]
    check(frames, [("fx", k) for k in names], run_gpu(posegen.pack(frames)))


def _nonfinite_frames():
    out = {}
    f = posegen.make_frame(500, 60, 40, "alt", 0.1, noise_px=0.5)
    f["world_pos"][f["match"][np.flatnonzero(f["match"] >= 0)[3]]] = np.nan
    out["nan_point"] = f
    f = posegen.make_frame(501, 60, 40, "alt", 0.1, noise_px=0.5)
    f["world_pos"][f["match"][np.flatnonzero(f["match"] >= 0)[7]], 1] = np.inf
    out["inf_point"] = f
    f = posegen.make_frame(502, 60, 40, "stereo", noise_px=0.5)
    f["tcw_init"][:] = 0.0
    out["zero_pose"] = f
    f = posegen.make_frame(503, 60, 40, "mono", noise_px=0.5)
    f["tcw_init"][5] = np.nan
    out["nan_pose"] = f
    f = posegen.make_frame(504, 60, 40, "alt", noise_px=0.5)
    f["world_pos"][:] = f["world_pos"][0]                      # every point the same: a rank-deficient system
    out["one_point"] = f
    return out


def test_non_finite_input_sets_the_status_bit_and_faults_nothing():
    fx = _nonfinite_frames()
    names = sorted(fx)
    frames = [fx[k] for k in names]
    res = run_gpu(posegen.pack(frames))
    check(frames, [("nonfinite", k) for k in names], res)
    assert res["status"][names.index("nan_pose")] & poseref.STATUS_NONFINITE
    assert not res["status"][names.index("zero_pose")] & poseref.STATUS_EARLY


def test_existing_flags_of_unmatched_key_points_stay():
    """outlier is in/out: flags of key points without a match are the caller's and stay; a frame that returns early keeps all of them"""
    frames = [_varied(i) for i in (0, 5, 9, 13)]
    rng = np.random.default_rng(5)
    before = rng.integers(0, 2, (4, 40)).astype(np.uint8)
    res = run_gpu(posegen.pack(frames), outlier=before.copy())
    check(frames, [("var", i) for i in (0, 5, 9, 13)], res, outlier_before=before)


def test_streams():
    """on a non-null stream; two back-to-back calls on one stream give identical bits"""
    frames = [_varied(i) for i in range(64)]
    p = posegen.pack(frames)
    s = torch.cuda.Stream()
    a = run_gpu(p, stream=s.cuda_stream)
    b = run_gpu(p, stream=s.cuda_stream)
    check(frames, [("var", i) for i in range(64)], a)
    for k in a:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k


# ---- plf_pose_commit
def commit_ref(mode, match, outlier, n, n_obs, n_points, row_id=None):
    """the ten-line restatement"""
    match = match.copy()
    found = np.zeros(n_points, np.int32)
    n_out = np.zeros(match.shape[0], np.int32)
    for f in range(match.shape[0]):
        for i in range(n[f]):
            row = match[f, i]
            if row < 0:
                continue
            pid = row if row_id is None else (row_id[f, row] if row < row_id.shape[1] else -1)
            known = 0 <= pid < n_points
            if mode == "discard":
                if outlier[f, i]:
                    match[f, i] = -1
                elif known and n_obs[pid] > 0:
                    n_out[f] += 1
            elif not outlier[f, i]:
                if known:
                    found[pid] += 1
                if n_obs is None or (known and n_obs[pid] > 0):
                    n_out[f] += 1
    return match, found, n_out


@pytest.mark.parametrize("mode", ["discard", "found"])
@pytest.mark.parametrize("mapped", [False, True])
def test_pose_commit(mode, mapped):
    rng = np.random.default_rng(9)
    F, S, P = 5, 300, 120
    n = np.array([300, 0, 257, 64, 299], np.int32)
    match = rng.integers(-1, P, (F, S)).astype(np.int32)
    match[match == 17] = -1
    match[0, 3] = match[2, 9] = match[4, 100] = 17            # one point matched from three frames: found raised three times
    outlier = (rng.random((F, S)) < 0.3).astype(np.uint8)
    outlier[0, 3] = outlier[2, 9] = outlier[4, 100] = 0
    n_obs = rng.integers(0, 3, P).astype(np.int32)
    match[3, 5], outlier[3, 5] = 23, 1                         # an outlier whose point has n_obs == 0
    n_obs[23] = 0
    row_id = None
    if mapped:
        row_id = np.stack([rng.permutation(P + 8)[:P] - 4 for _ in range(F)]).astype(np.int32)       # ids outside [0, P) included
    want_match, want_found, want_n = commit_ref(mode, match, outlier, n, n_obs, P, row_id)
    d = lambda a: None if a is None else torch.from_numpy(a).cuda()
    dm, found = d(match), torch.zeros(P, dtype=torch.int32, device="cuda")
    n_out = pose_commit(mode, dm, d(outlier), n_obs=d(n_obs), found=found if mode == "found" else None, row_id=d(row_id), n=d(n))
    torch.cuda.synchronize()
    assert np.array_equal(dm.cpu().numpy(), want_match)
    assert np.array_equal(n_out.cpu().numpy(), want_n)
    if mode == "found":
        assert np.array_equal(found.cpu().numpy(), want_found)
        if not mapped:
            assert want_found[17] == 3
        # mbOnlyTracking: every inlier match counts
        n_all = pose_commit("found", dm, d(outlier), n_obs=None, found=torch.zeros(P, dtype=torch.int32, device="cuda"), row_id=d(row_id), n=d(n))
        assert np.array_equal(n_all.cpu().numpy(), commit_ref("found", match, outlier, n, None, P, row_id)[2])


# ---- the IEEE operations the exactness claim rests on
def _splitmix64(x):
    x = (x + np.uint64(0x9E3779B97F4A7C15))
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def _samples(n, j):
    with np.errstate(over="ignore"):
        u = _splitmix64(np.uint64(2) * np.arange(n, dtype=np.uint64) + np.uint64(j))
    special = ((u >> np.uint64(52)) & np.uint64(0x7ff)) == np.uint64(0x7ff)
    u = np.where(special, u & ~np.uint64(1 << 62), u)
    return u.view(np.float64)


def _debug_math(op, n, width):
    lib = L.lib()
    lib.plf_debug_math.argtypes = [C.c_int32, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p]
    out = torch.zeros(n * width, dtype=torch.float64, device="cuda")
    L.check(lib.plf_debug_math(op, None, 0, n, out.data_ptr(), 0, None), "plf_debug_math")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def test_device_sqrt_and_division_are_ieee():
    """10^6 sampled operands (subnormals, huge and tiny magnitudes included) against numpy, bit for bit"""
    n = 1000000
    a, b = _samples(n, 0), _samples(n, 1)
    with np.errstate(all="ignore"):
        want_sqrt, want_div = np.sqrt(np.abs(a)), a / b
    got = _debug_math(12, n, 1)
    assert np.array_equal(got.view(np.uint64), want_sqrt.view(np.uint64))
    got = _debug_math(13, n, 1)
    nan = np.isnan(want_div)
    assert np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint64)[~nan], want_div.view(np.uint64)[~nan])


def test_device_sincos_d_equals_the_host_build():
    """plf_sincos_d on the device against the same header compiled with g++, on 2^20 angles of [1e-5, 2 pi], bit for bit"""
    n = 1 << 20
    lo, hi = 0x3EE4F8B588E368F1, 0x401921FB54442D18
    theta = (np.uint64(lo) + np.arange(n, dtype=np.uint64) * np.uint64((hi - lo) // (n - 1))).view(np.float64)
    assert theta[0] == 1e-5 and abs(theta[-1] - 2 * np.pi) < 1e-9
    s, c = np.zeros(n), np.zeros(n)
    poseref.host().pm_sincos(theta.ctypes.data, n, s.ctypes.data, c.ctypes.data)
    got = _debug_math(14, n, 2).reshape(n, 2)
    assert np.array_equal(got[:, 0].view(np.uint64), s.view(np.uint64)) and np.array_equal(got[:, 1].view(np.uint64), c.view(np.uint64))

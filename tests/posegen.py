"""Synthetic frames for the pose tests (tests/test_pose_ref.py, tests/test_gpu_pose.py, tools/bench_pose.py): points in front of a pinhole camera,
their projections as key points, a perturbed start pose.  numpy only; every array in the layout of include/plf.h's plf_pose_view."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
CAM = (520.0, 520.0, 320.0, 240.0, 40.0)          # fx, fy, cx, cy, bf
NLEVELS = 8
INV_SIGMA2 = np.array([1.0 / (1.2 ** (2 * i)) for i in range(NLEVELS)], np.float32)


def rodrigues(w):
    th = np.linalg.norm(w)
    if th < 1e-12:
        return np.eye(3)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def tcw12(R, t):
    return np.hstack([R, t.reshape(3, 1)]).astype(np.float32).reshape(12)


def make_frame(seed, n_kp, n_edges, mix="mono", outlier_share=0.0, rot_deg=2.0, trans=0.05, noise_px=0.0, outlier_px=50.0, n_points=None, init_seed=None,
               drop=0.0):
    """One frame: n_kp key points of which n_edges, at random positions, are matched.  mix: mono | stereo | alt | rand.  init_seed: the start pose
    (and, with drop, the share of matches removed again) from a generator of its own, so that frames of one scene differ.
    Returns a dict: keys (n_kp,) KP_DTYPE, uright, match (int32, -1 = none), world_pos (M, 3) float32, tcw_true / tcw_init (12,) float32,
    planted (n_kp,) bool: the displaced matches."""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy, bf = CAM
    Rt = rodrigues(rng.normal(size=3) * 0.3)
    tt = rng.normal(size=3) * 0.5
    m = n_edges if n_points is None else n_points
    z = rng.uniform(1.0, 8.0, m)
    u = rng.uniform(20.0, 620.0, m)
    v = rng.uniform(20.0, 460.0, m)
    Xc = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], 1)
    world = ((Xc - tt) @ Rt).astype(np.float32)              # Rt^T (Xc - t)
    # the key points are the projections of the FLOAT world points under the FLOAT true pose
    T = tcw12(Rt, tt).astype(np.float64)
    R32, t32 = T.reshape(3, 4)[:, :3], T.reshape(3, 4)[:, 3]
    Xc = world.astype(np.float64) @ R32.T + t32
    keys = np.zeros(n_kp, KP_DTYPE)
    keys["x"] = rng.uniform(0, 640, n_kp)
    keys["y"] = rng.uniform(0, 480, n_kp)
    keys["octave"] = rng.integers(0, NLEVELS, n_kp)
    uright = np.full(n_kp, -1.0, np.float32)
    match = np.full(n_kp, -1, np.int32)
    planted = np.zeros(n_kp, bool)
    where = np.sort(rng.choice(n_kp, n_edges, replace=False))
    rows = rng.permutation(m)[:n_edges]
    n_out = int(round(outlier_share * n_edges))
    bad = set(rng.choice(n_edges, n_out, replace=False).tolist())
    for e, (i, r) in enumerate(zip(where, rows)):
        pu = Xc[r, 0] / Xc[r, 2] * fx + cx
        pv = Xc[r, 1] / Xc[r, 2] * fy + cy
        if noise_px:
            pu += rng.normal() * noise_px
            pv += rng.normal() * noise_px
        if e in bad:
            a = rng.uniform(0, 2 * np.pi)
            pu += outlier_px * np.cos(a)
            pv += outlier_px * np.sin(a)
            planted[i] = True
        stereo = {"mono": False, "stereo": True, "alt": e % 2 == 1, "rand": rng.random() < 0.5}[mix]
        keys["x"][i], keys["y"][i] = pu, pv
        if stereo:
            uright[i] = pu - bf / Xc[r, 2]
        match[i] = r
    if init_seed is not None:
        rng = np.random.default_rng([seed, init_seed])
        gone = (rng.random(n_kp) < drop) & (match >= 0)
        match[gone] = -1
        planted[gone] = False
    Ri = rodrigues(rng.normal(size=3) / np.sqrt(3) * np.deg2rad(rot_deg)) @ Rt
    ti = tt + rng.normal(size=3) / np.sqrt(3) * trans
    return dict(keys=keys, uright=uright, match=match, world_pos=world, tcw_true=tcw12(Rt, tt), tcw_init=tcw12(Ri, ti), planted=planted)


def ref_frame(fr, poseref, outlier=None, counters=None):
    """tests/poseref.py on one frame of make_frame"""
    k = fr["keys"]
    return poseref.pose_optimization(fr["tcw_init"], np.stack([k["x"], k["y"]], 1), fr["uright"], k["octave"], fr["match"], fr["world_pos"], INV_SIGMA2, CAM,
                                     outlier=outlier, counters=counters)


# ---- the C layouts: the package's own (rgbd_pl_slam_amd/_lib.py)
import sys  # noqa: E402
sys.path.insert(0, ROOT)
from rgbd_pl_slam_amd._lib import Camera, PoseView  # noqa: E402


def camera():
    fx, fy, cx, cy, bf = CAM
    return Camera(fx, fy, cx, cy, 0, 0, 0, 0, 0, bf)


def pack(frames, kp_stride=None, shared_pos=False, sentinel=True):
    """frames of make_frame -> host arrays of one call: keys (F, S), uright, match, n (F,), world_pos (F, P, 3) or the first frame's (shared),
    pose_in (F, 12).  Entries beyond a frame's key points: match = 7 (a row that must not be read as an edge), keys NaN."""
    F = len(frames)
    S = kp_stride or max(len(f["match"]) for f in frames)
    P = max(1, max(len(f["world_pos"]) for f in frames))       # never empty: a valid address
    keys = np.zeros((F, S), KP_DTYPE)
    uright = np.full((F, S), np.nan if sentinel else -1.0, np.float32)
    match = np.full((F, S), 7 if sentinel else -1, np.int32)
    if sentinel:
        keys["x"] = np.nan
        keys["y"] = np.nan
        keys["octave"] = 1 << 20
    n = np.zeros(F, np.int32)
    world = np.zeros((1 if shared_pos else F, P, 3), np.float32)
    pose = np.zeros((F, 12), np.float32)
    for i, f in enumerate(frames):
        k = len(f["match"])
        n[i] = k
        keys[i, :k] = f["keys"]
        uright[i, :k] = f["uright"]
        match[i, :k] = f["match"]
        if not shared_pos or i == 0:
            world[i, :len(f["world_pos"])] = f["world_pos"]
        pose[i] = f["tcw_init"]
    return dict(keys=keys, uright=uright, match=match, n=n, world_pos=world, pose_in=pose, kp_stride=S, pos_stride=0 if shared_pos else P)


_cpu = None


def cpu_loop():
    """tools/pose_cpu.cpp built as a shared object (the build line of its header)"""
    global _cpu
    if _cpu is None:
        so = os.path.join(tempfile.mkdtemp(prefix="pose_cpu_"), "pose_cpu.so")
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", "-I", os.path.join(ROOT, "rgbd_pl_slam_amd", "csrc"),
                               os.path.join(ROOT, "tools", "pose_cpu.cpp"), "-o", so])
        _cpu = C.CDLL(so)
        _cpu.pose_cpu.argtypes = [C.POINTER(PoseView), C.POINTER(Camera)] + [C.c_void_p] * 6
    return _cpu


def run_cpu_loop(p, outlier=None, n_from_device=True):
    """pose_cpu over the host arrays of pack(); returns dict(pose (F, 12), frustum (F, 15), outlier (F, S) uint8, n_inliers, status)"""
    F, S = p["match"].shape
    v = PoseView()
    v.n_frames, v.kp_stride, v.pos_stride, v.nlevels = F, S, p["pos_stride"], NLEVELS
    keep = [np.ascontiguousarray(p[k]) for k in ("keys", "uright", "match", "world_pos", "n", "pose_in")] + [INV_SIGMA2.copy()]
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    v.keys_un, v.uright, v.match_of_kp, v.world_pos = (ptr(a) for a in keep[:4])
    v.n_device = ptr(keep[4]) if n_from_device else None
    v.n_host = int(p["n"][0])
    v.inv_level_sigma2 = ptr(keep[6])
    out = dict(pose=np.zeros((F, 12), np.float32), frustum=np.zeros((F, 15), np.float32),
               outlier=np.full((F, S), 0xAB, np.uint8) if outlier is None else np.array(outlier, np.uint8), n_inliers=np.zeros(F, np.int32),
               status=np.zeros(F, np.int32))
    cam = camera()
    cpu_loop().pose_cpu(C.byref(v), C.byref(cam), ptr(keep[5]), ptr(out["pose"]), ptr(out["frustum"]), ptr(out["outlier"]), ptr(out["n_inliers"]),
                        ptr(out["status"]))
    return out


def fixtures():
    """The control-flow fixtures of both suites: name -> frame.  What each forces is asserted, with the definition's counters, in tests/test_pose_ref.py."""
    fx = {}
    fx["rejected"] = make_frame(0, 40, 30, "mono", noise_px=0.5)            # rejected trials: lambda grows, inlier edges keep stale errors
    fx["ten_rejected"] = make_frame(1, 300, 200, "stereo", 0.2, noise_px=0.5)
    fx["nbad"] = make_frame(5, 128, 128, "rand", 0.3, noise_px=0.5)
    fx["nine_edges"] = make_frame(3, 20, 9, "rand", noise_px=0.5)
    fx["two_edges"] = make_frame(4, 10, 2, "mono")
    behind = make_frame(6, 50, 40, "alt", noise_px=0.5)
    i = int(np.flatnonzero(behind["match"] >= 0)[5])
    T = behind["tcw_true"].astype(np.float64).reshape(3, 4)
    behind["world_pos"][behind["match"][i]] = (T[:, :3].T @ (np.array([0.3, -0.2, -2.0]) - T[:, 3])).astype(np.float32)   # 2 m behind the camera
    fx["behind"] = behind
    stale = make_frame(501, 60, 40, "alt", 0.1, noise_px=0.5)                 # an Inf coordinate: every trial is rejected with a NaN chi2, and the inlier
    stale["world_pos"][stale["match"][np.flatnonzero(stale["match"] >= 0)[7]], 1] = np.inf   # edges keep errors that differ from those at the restored estimate
    fx["stale"] = stale
    # the final chi2 of key point 1 lies within half a float ulp ABOVE 5.991f (5.99100027595..., found by a search over the ulps of its x and y): the binary
    # narrows chi2 to float before it compares, so the edge stays an inlier; a comparison in double would flag it
    win = make_frame(705, 20, 14, "mono", noise_px=1.3)
    win["keys"]["x"][1], win["keys"]["y"][1] = np.float32(416.11297607421875), np.float32(362.4393310546875)
    fx["chi2_window"] = win
    win = make_frame(801, 20, 14, "stereo", noise_px=1.3)                      # the same for a stereo edge: key point 3 ends at 7.81500024924... above 7.815f
    win["keys"]["x"][3], win["keys"]["y"][3] = np.float32(225.7312469482422), np.float32(171.52410888671875)
    fx["chi2_window_stereo"] = win
    return fx

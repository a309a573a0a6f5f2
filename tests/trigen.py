"""Scenes for the new-map-point tests: known 3D points seen from two posed RGB-D keyframes, with pixel noise, invalid and negative depths, planted
mismatches and octave mismatches, every array in the layout of include/plf.h's plf_triangulate_view; and the three runners over a scene -- the
definition (tests/triref.py), the single-thread C++ loop (tools/tri_cpu.cpp) and the device (rgbd_pl_slam_amd.triangulate).  numpy only at import.

A scene: dict(slots=[keyframe, ...], job_kf1, job_kf2 (J,) int32, match12 (J, S) int32).  A keyframe: dict(keys (KP records), uright, depth (n,)
float32, n, pose (15 float32: Rcw, tcw, Ow), has_mp (n,) uint8, mappoints (n,) int32)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import triref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KP = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
F32 = np.float32
CAM = (517.306408, 516.469215, 318.643040, 255.313989, 40.0)      # fx, fy, cx, cy, bf of TUM1.yaml
MB = float(F32(40.0) / F32(517.306408))                             # mb = mbf / fx
SCALE_FACTOR = 1.2
NLEVELS = 8


def scales():
    sf = np.ones(NLEVELS, F32)
    for i in range(1, NLEVELS):
        sf[i] = sf[i - 1] * F32(SCALE_FACTOR)                       # as ORBextractor fills mvScaleFactor
    return sf, (sf * sf).astype(F32)


SF, SIGMA2 = scales()


def camera():
    return R.camera(CAM, MB, CAM[4], SCALE_FACTOR)


def rodrigues(w):
    th = float(np.linalg.norm(w))
    if th < 1e-12:
        return np.eye(3)
    k = np.asarray(w, float) / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def pose15(Rm, t):
    """Rcw, tcw, Ow = -Rcw^T tcw as float32"""
    Rm, t = np.asarray(Rm, float), np.asarray(t, float)
    return np.concatenate([Rm.reshape(-1), t, -(Rm.T @ t)]).astype(F32)


def keyframe(n, pose):
    return dict(keys=np.zeros(n, KP), uright=np.full(n, -1, F32), depth=np.full(n, -1, F32), n=n, pose=np.asarray(pose, F32),
                has_mp=np.zeros(n, np.uint8), mappoints=np.full(n, -1, np.int32))


def project(Xw, pose):
    p = np.asarray(pose, float)
    Xc = Xw @ p[:9].reshape(3, 3).T + p[9:12]
    with np.errstate(all="ignore"):
        return CAM[0] * Xc[:, 0] / Xc[:, 2] + CAM[2], CAM[1] * Xc[:, 1] / Xc[:, 2] + CAM[3], Xc[:, 2]


def pair_scene(seed, n1, n2, n_pairs, t2, rot2=0.02, stereo_frac=0.7, far_frac=0.25, mismatch=0.08, noisy=0.08, octave_off=0.06, bad_depth=0.04,
               pass_through=0, z_range=(0.5, 7.0), noise_px=0.3):
    """two keyframes and their match list.  n_pairs world points, in front of keyframe 1, are seen by key points of both (those of keyframe 2 permuted);
    the other key points are filler without a pair.  t2: the translation of keyframe 2 relative to keyframe 1 (its camera frame).  far_frac: the share
    of points beyond the depth sensor (8 to 60 m), monocular in both.  mismatch: the share of pairs whose second key point is another one; noisy:
    with 6 pixels of noise instead of noise_px (both times the level's scale); octave_off: with octaves five apart; bad_depth: stereo key points whose depth is invalid (-1, 0, NaN).  pass_through:
    that many extra pairs of a near stereo key point (0.3 to 0.8 m) with a key point on the same ray in keyframe 2."""
    rng = np.random.default_rng(seed)
    m = min(n_pairs, n1, n2)
    pass_through = min(pass_through, m)
    R1, t1 = rodrigues(rng.normal(size=3) * 0.05), rng.normal(size=3) * 0.3
    R2 = rodrigues(rng.normal(size=3) * rot2) @ R1
    p1, p2 = pose15(R1, t1), pose15(R2, R2 @ (R1.T @ t1) + np.asarray(t2, float))     # Xc2 = Rrel * Xc1 + t2
    kf1, kf2 = keyframe(n1, p1), keyframe(n2, p2)
    for kf in (kf1, kf2):
        kf["keys"]["x"], kf["keys"]["y"] = rng.uniform(0, 640, kf["n"]), rng.uniform(0, 480, kf["n"])
        kf["keys"]["octave"] = rng.integers(0, NLEVELS, kf["n"])
        st = rng.random(kf["n"]) < stereo_frac
        z = rng.uniform(0.5, 7.0, kf["n"])
        kf["depth"][st] = z[st]
        kf["uright"][st] = (kf["keys"]["x"][st] - CAM[4] / z[st]).astype(F32)
    match = np.full(n1, -1, np.int32)
    if m:
        i1 = np.sort(rng.choice(n1, m, replace=False))
        i2 = rng.choice(n2, m, replace=False)
        far = rng.random(m) < far_frac
        z = np.where(far, rng.uniform(8.0, 60.0, m), rng.uniform(z_range[0], z_range[1], m))
        u, v = rng.uniform(20, 620, m), rng.uniform(20, 460, m)
        if pass_through:
            z[:pass_through] = rng.uniform(0.3, 0.8, pass_through)
            far[:pass_through] = False
        Xc = np.stack([(u - CAM[2]) / CAM[0] * z, (v - CAM[3]) / CAM[1] * z, z], 1)
        Xw = (Xc - p1[9:12].astype(float)) @ p1[:9].reshape(3, 3).astype(float)
        o1 = rng.integers(0, NLEVELS, m)
        o2 = np.clip(o1 + rng.integers(-1, 2, m), 0, NLEVELS - 1)
        off = rng.random(m) < octave_off
        o2[off] = np.where(o1[off] < 4, o1[off] + 5, o1[off] - 5).clip(0, NLEVELS - 1)
        for kf, idx, octv in ((kf1, i1, o1), (kf2, i2, o2)):
            uu, vv, zz = project(Xw, kf["pose"])
            px = np.where(rng.random(m) < noisy, 6.0, noise_px) * SF[octv]
            kf["keys"]["x"][idx] = uu + rng.normal(size=m) * px
            kf["keys"]["y"][idx] = vv + rng.normal(size=m) * px
            kf["keys"]["octave"][idx] = octv
            st = (rng.random(m) < stereo_frac) & ~far & (zz > 0.1)
            zn = zz * (1 + rng.normal(size=m) * 0.01)
            kf["depth"][idx] = np.where(st, zn, -1).astype(F32)
            with np.errstate(all="ignore"):
                kf["uright"][idx] = np.where(st, kf["keys"]["x"][idx] - CAM[4] / zn, -1).astype(F32)
            bad = st & (rng.random(m) < bad_depth)
            kf["depth"][idx[bad]] = rng.choice(np.array([-1.0, 0.0, np.nan], F32), int(bad.sum()))
        if pass_through:                                             # a near stereo key point of keyframe 1, and the same ray in keyframe 2
            q = np.arange(pass_through)
            x1n = (kf1["keys"]["x"][i1[q]] - CAM[2]) / CAM[0]
            y1n = (kf1["keys"]["y"][i1[q]] - CAM[3]) / CAM[1]
            ray = np.stack([x1n, y1n, np.ones(pass_through)], 1) @ p1[:9].reshape(3, 3).astype(float) @ p2[:9].reshape(3, 3).astype(float).T
            kf2["keys"]["x"][i2[q]] = CAM[0] * ray[:, 0] / ray[:, 2] + CAM[2]
            kf2["keys"]["y"][i2[q]] = CAM[1] * ray[:, 1] / ray[:, 2] + CAM[3]
            kf2["keys"]["octave"][i2[q]] = kf1["keys"]["octave"][i1[q]]
            kf1["depth"][i1[q]] = z[q].astype(F32)
            kf1["uright"][i1[q]] = (kf1["keys"]["x"][i1[q]] - CAM[4] / z[q]).astype(F32)
            kf2["depth"][i2[q]], kf2["uright"][i2[q]] = -1, -1
        match[i1] = i2
        wrong = np.nonzero(rng.random(m) < mismatch)[0]
        wrong = wrong[wrong >= pass_through]
        match[i1[wrong]] = np.roll(i2[wrong], 1)                     # each takes another pair's key point: every i2 is still named once, as the search leaves it
    return kf1, kf2, match


def scene_of(pairs, S=None):
    """[(kf1, kf2, match12), ...] -> a scene; job j takes slots 2j and 2j + 1"""
    S = max([len(m) for _a, _b, m in pairs] + [1]) if S is None else S
    slots, m12 = [], np.full((len(pairs), S), -1, np.int32)
    for j, (a, b, m) in enumerate(pairs):
        slots += [a, b]
        m12[j, :min(len(m), S)] = m[:S]
    J = len(pairs)
    return dict(slots=slots, job_kf1=np.arange(0, 2 * J, 2, dtype=np.int32), job_kf2=np.arange(1, 2 * J, 2, dtype=np.int32), match12=m12)


def reversed_job(sc, j):
    """job j with the keyframes swapped: the same slots, match21"""
    a, b = sc["slots"][sc["job_kf1"][j]], sc["slots"][sc["job_kf2"][j]]
    m21 = np.full(sc["match12"].shape[1], -1, np.int32)
    for i1 in range(a["n"] - 1, -1, -1):
        i2 = sc["match12"][j, i1]
        if 0 <= i2 < min(b["n"], len(m21)):
            m21[i2] = i1
    return int(sc["job_kf2"][j]), int(sc["job_kf1"][j]), m21


def add_job(sc, kf1_slot, kf2_slot, match):
    sc["job_kf1"] = np.append(sc["job_kf1"], np.int32(kf1_slot))
    sc["job_kf2"] = np.append(sc["job_kf2"], np.int32(kf2_slot))
    row = np.full((1, sc["match12"].shape[1]), -1, np.int32)
    row[0, :len(match)] = match[:row.shape[1]]
    sc["match12"] = np.concatenate([sc["match12"], row])


def zero_distance_pair(seed, n=12):
    """planted: keyframe 1's Ow is (1, 1, 1) although its pose puts the camera elsewhere, every key point sits at the principal point with a depth of
    1e-30, so that UnprojectStereo returns Ow itself; both keyframes see (1, 1, 1) two metres ahead"""
    rng = np.random.default_rng(seed)
    p1 = pose15(np.eye(3), [-1.0, -1.0, 1.0]); p1[12:15] = 1.0
    p2 = pose15(np.eye(3), [-1.2, -1.0, 1.0])
    kf1, kf2 = keyframe(n, p1), keyframe(n, p2)
    kf1["keys"]["x"], kf1["keys"]["y"] = CAM[2], CAM[3]
    kf1["depth"][:] = 1e-30
    kf1["uright"][:] = CAM[2] - CAM[4] / 2.0
    kf2["keys"]["x"] = CAM[2] - 0.1 * CAM[0] + rng.normal(size=n) * 0.2
    kf2["keys"]["y"] = CAM[3] + rng.normal(size=n) * 0.2
    return kf1, kf2, rng.permutation(n).astype(np.int32)


def standard_scene(seed=1, n=300, pairs=150):
    """the scene every reason code and branch occurs in at least five times (asserted by reason_counts_ok):
      0 sideways baseline of 0.25 m            1 a baseline just above mb          2 forward motion of 1 m, with near points passed through
      3 job 2 reversed                         4 a baseline below mb: skipped      5 job 0's geometry with tcw2[0] = +Inf (x3D[3] == 0)
      6 the planted zero distances             and a few i2 beyond keyframe 2 in job 0"""
    prs = [pair_scene(seed, n, n + 17, pairs, (-0.25, 0.02, 0.03)), pair_scene(seed + 1, n - 40, n, pairs, (-0.08, 0.01, 0.02)),
           pair_scene(seed + 2, n, n, pairs, (0.01, -0.01, -1.0), pass_through=20, z_range=(1.5, 7.0)),
           pair_scene(seed + 3, n // 2, n // 2, pairs // 2, (0.005, 0.0, 0.008)), pair_scene(seed + 4, n, n, pairs, (-0.25, 0.02, 0.03)),
           zero_distance_pair(seed + 5)]
    prs[4][1]["pose"][9] = np.inf                                   # one -Inf in A's last column: that column never rotates, and sorts first
    m0 = prs[0][2]
    have = np.nonzero(m0 >= 0)[0]
    m0[have[::12]] = prs[0][1]["n"] + np.arange(len(have[::12]))     # i2 outside keyframe 2
    sc = scene_of(prs, S=n)
    k1, k2, m21 = reversed_job(sc, 2)
    add_job(sc, k1, k2, m21)
    perm = [0, 1, 2, 6, 3, 4, 5]                                     # the reversed job goes fourth
    for k in ("job_kf1", "job_kf2", "match12"):
        sc[k] = np.ascontiguousarray(sc[k][perm])
    return sc


def ref_call(sc, new_stride=None, mark_has_mp=False, id_base=None, cam=None):
    """the definition over a scene, with the call's output conventions.  Returns dict(new_i1, new_i2, new_pos, n_new, status, reason[, has_mp, mappoints])"""
    J, S = sc["match12"].shape
    ns = S if new_stride is None else new_stride
    cam = camera() if cam is None else cam
    out = dict(new_i1=np.full((J, ns), -1, np.int32), new_i2=np.full((J, ns), -1, np.int32), new_pos=np.zeros((J, ns, 3), F32), n_new=np.zeros(J, np.int32),
               status=np.zeros(J, np.int32), reason=np.zeros((J, S), np.uint8), has_mp=[s["has_mp"].copy() for s in sc["slots"]],
               mappoints=[s["mappoints"].copy() for s in sc["slots"]])
    for j in range(J):
        a, b = int(sc["job_kf1"][j]), int(sc["job_kf2"][j])
        if not (0 <= a < len(sc["slots"]) and 0 <= b < len(sc["slots"])):
            out["status"][j] = R.BAD_SLOT
            continue
        r = R.triangulate_job(sc["slots"][a], sc["slots"][b], sc["match12"][j], cam, SF, SIGMA2)
        if r["status"]:
            out["status"][j] = r["status"]
            continue
        k = min(len(r["i1"]), ns)
        out["new_i1"][j, :k], out["new_i2"][j, :k], out["new_pos"][j, :k] = r["i1"][:k], r["i2"][:k], r["pos"][:k]
        out["n_new"][j], out["status"][j] = len(r["i1"]), R.OVERFLOW if len(r["i1"]) > ns else 0
        out["reason"][j, :len(r["reason"])] = r["reason"]
        for q in range(k):
            if mark_has_mp:
                out["has_mp"][a][r["i1"][q]] = 1
                out["has_mp"][b][r["i2"][q]] = 1
            if id_base is not None:
                out["mappoints"][a][r["i1"][q]] = id_base[j] + q
                out["mappoints"][b][r["i2"][q]] = id_base[j] + q
    return out


def reason_counts(ref):
    codes = np.bincount((ref["reason"] & 15).reshape(-1), minlength=16)
    branches = np.bincount((ref["reason"] >> 4).reshape(-1), minlength=4)
    return codes, branches


def reason_counts_ok(ref, at_least=5):
    """every one of the eleven reasons and of the three branches occurs at least `at_least` times; fails loudly otherwise"""
    codes, branches = reason_counts(ref)
    assert all(codes[r] >= at_least for r in range(1, 12)), "a reason code is missing from the scene: %s" % codes[1:12].tolist()
    assert all(branches[b] >= at_least for b in range(1, 4)), "a branch is missing from the scene: %s" % branches[1:4].tolist()
    return codes, branches


_cpu = None


def cpu_loop():
    """tools/tri_cpu.cpp built as a shared object (the build line of its header)"""
    global _cpu
    if _cpu is None:
        so = os.path.join(tempfile.mkdtemp(prefix="tri_cpu_"), "tri_cpu.so")
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", os.path.join(ROOT, "tools", "tri_cpu.cpp"), "-o", so])
        from rgbd_pl_slam_amd import _lib as L
        _cpu = L.tri_prototypes(C.CDLL(so), "tri_cpu_points")
        _cpu.tri_cpu_svd_last_row.argtypes = [C.c_void_p, C.c_void_p]
        _cpu.tri_cpu_svd_last_row.restype = None
    return _cpu


def ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def cpu_call(sc, new_stride=None, mark_has_mp=False, id_base=None, mb=MB, seconds=None):
    """tools/tri_cpu.cpp over a scene; seconds: a list that receives the time of the loop itself"""
    import time
    from rgbd_pl_slam_amd import _lib as L
    lib = cpu_loop()
    J, S = sc["match12"].shape
    ns = S if new_stride is None else new_stride
    slots = sc["slots"]
    keep = dict(keys=[np.ascontiguousarray(s["keys"]) for s in slots], ur=[np.ascontiguousarray(s["uright"], F32) for s in slots],
                d=[np.ascontiguousarray(s["depth"], F32) for s in slots], has=[s["has_mp"].copy() for s in slots], mp=[s["mappoints"].copy() for s in slots])
    table = lambda arrs: np.array([a.ctypes.data for a in arrs], np.uint64)    # noqa: E731
    tk, tu, td, th, tm = (table(keep[k]) for k in ("keys", "ur", "d", "has", "mp"))
    kn = np.array([s["n"] for s in slots], np.int32)
    poses = np.ascontiguousarray(np.stack([s["pose"] for s in slots]) if slots else np.zeros((0, 15)), F32)
    v = L.TriangulateView(len(slots), tk.ctypes.data, tu.ctypes.data, td.ctypes.data, kn.ctypes.data, poses.ctypes.data, SF.ctypes.data, SIGMA2.ctypes.data,
                          NLEVELS, SCALE_FACTOR, mb, CAM[4])
    k1, k2, m12 = (np.ascontiguousarray(sc[k], np.int32) for k in ("job_kf1", "job_kf2", "match12"))
    jobs = L.TriangulateJobs(J, S, ns, k1.ctypes.data, k2.ctypes.data, m12.ctypes.data)
    idb = np.asarray(id_base, np.int32) if id_base is not None else None
    marks = L.TriangulateMarks(th.ctypes.data if mark_has_mp else None, tm.ctypes.data if idb is not None else None, idb.ctypes.data if idb is not None else None)
    cam = L.Camera(CAM[0], CAM[1], CAM[2], CAM[3], 0, 0, 0, 0, 0, CAM[4])
    out = dict(new_i1=np.full((J, ns), -1, np.int32), new_i2=np.full((J, ns), -1, np.int32), new_pos=np.zeros((J, ns, 3), F32), n_new=np.zeros(J, np.int32),
               status=np.zeros(J, np.int32), reason=np.zeros((J, S), np.uint8))
    t0 = time.perf_counter()
    lib.tri_cpu_points(C.byref(v), C.byref(cam), C.byref(jobs), C.byref(marks), ptr(out["new_i1"]), ptr(out["new_i2"]), ptr(out["new_pos"]), ptr(out["n_new"]),
                       ptr(out["status"]), ptr(out["reason"]))
    if seconds is not None:
        seconds.append(time.perf_counter() - t0)
    out["has_mp"], out["mappoints"] = keep["has"], keep["mp"]
    return out


def dev_keyframes(sc):
    """the scene's slots on the device as a KeyFrameSet"""
    import torch
    from rgbd_pl_slam_amd.triangulate import KeyFrameSet
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
    slots = sc["slots"]
    keys = [t(np.frombuffer(np.ascontiguousarray(s["keys"]).tobytes(), np.uint8).reshape(s["n"], 28).copy()) for s in slots]
    return KeyFrameSet(keys, [t(np.asarray(s["uright"], F32)) for s in slots], [t(np.asarray(s["depth"], F32)) for s in slots],
                       t(np.stack([s["pose"] for s in slots]).astype(F32)), has_mp=[t(s["has_mp"]) for s in slots], mappoints=[t(s["mappoints"]) for s in slots])


def dev_call(sc, new_stride=None, mark_has_mp=False, id_base=None, mb=MB, kfs=None):
    """the device call over a scene; returns host copies shaped as ref_call's"""
    import torch
    from rgbd_pl_slam_amd import triangulate_points
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
    kfs = dev_keyframes(sc) if kfs is None else kfs
    r = triangulate_points(kfs, t(sc["job_kf1"]), t(sc["job_kf2"]), t(sc["match12"]), CAM, mb, t(SF), t(SIGMA2), scale_factor=SCALE_FACTOR, new_stride=new_stride,
                           mark_has_mp=mark_has_mp, id_base=t(np.asarray(id_base, np.int32)) if id_base is not None else None)
    torch.cuda.synchronize()
    out = {k: getattr(r, k).cpu().numpy() for k in ("new_i1", "new_i2", "new_pos", "n_new", "status", "reason")}
    out["has_mp"] = [a.cpu().numpy() for a in kfs.keep[3]]
    out["mappoints"] = [a.cpu().numpy() for a in kfs.keep[4]]
    return out


def same_bits(a, b):
    """bit equality of two float arrays; a NaN equals any NaN"""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


def assert_equal(got, want, what=""):
    for k in ("n_new", "status", "reason", "new_i1", "new_i2"):
        assert np.array_equal(got[k], want[k]), (what, k, np.nonzero(np.asarray(got[k]) != np.asarray(want[k])))
    assert same_bits(got["new_pos"], want["new_pos"]), (what, "new_pos")
    for k in ("has_mp", "mappoints"):
        for s, (a, b) in enumerate(zip(got[k], want[k])):
            assert np.array_equal(a, b), (what, k, s)


def tiny_scene():
    prs = [pair_scene(40, 24, 20, 14, (-0.25, 0.02, 0.03)), pair_scene(41, 16, 24, 12, (0.01, -0.01, -1.0), pass_through=3, z_range=(1.5, 7.0)),
           pair_scene(42, 8, 8, 6, (0.005, 0.0, 0.008))]
    return scene_of(prs, S=24)


def tiny_fixture():
    """the content of tests/golden/tri_tiny.json: three small jobs with the definition's output bits; floats as uint32 bit patterns"""
    sc = tiny_scene()
    r = ref_call(sc, mark_has_mp=True, id_base=[100, 200, 300])
    bits = lambda a: np.ascontiguousarray(a, F32).view(np.uint32).reshape(-1).tolist()   # noqa: E731
    return {"_doc": "tests/trigen.py tiny_fixture(): inputs and the output bits of tests/triref.py; floats as uint32 bit patterns",
            "cam": bits(np.array(CAM, F32)), "mb": bits(np.array([MB], F32)), "scale_factors": bits(SF), "level_sigma2": bits(SIGMA2),
            "slots": [{"n": int(s["n"]), "x": bits(s["keys"]["x"]), "y": bits(s["keys"]["y"]), "octave": s["keys"]["octave"].tolist(), "uright": bits(s["uright"]),
                       "depth": bits(s["depth"]), "pose": bits(s["pose"])} for s in sc["slots"]],
            "job_kf1": sc["job_kf1"].tolist(), "job_kf2": sc["job_kf2"].tolist(), "match12": sc["match12"].reshape(-1).tolist(),
            "out": {"new_i1": r["new_i1"].reshape(-1).tolist(), "new_i2": r["new_i2"].reshape(-1).tolist(), "new_pos": bits(r["new_pos"]), "n_new": r["n_new"].tolist(),
                    "status": r["status"].tolist(), "reason": r["reason"].reshape(-1).tolist(), "has_mp": [a.tolist() for a in r["has_mp"]],
                    "mappoints": [a.tolist() for a in r["mappoints"]]}}


if __name__ == "__main__":
    import json
    import sys
    if sys.argv[1:] == ["--write-golden"]:
        with open(os.path.join(ROOT, "tests", "golden", "tri_tiny.json"), "w") as fh:
            json.dump(tiny_fixture(), fh, separators=(",", ":"))
            fh.write("\n")
    elif sys.argv[1:] == ["--counts"]:
        print(reason_counts(ref_call(standard_scene())))

"""Scenes for the tracking-tail tests: frames of key points with depths, matches into a small map and a camera pose, every array in the layout of
include/plf.h's plf_track_view; and the three runners over a packed batch -- the definition (tests/trackref.py), the single-thread C++ loop
(tools/track_cpu.cpp) and the device (rgbd_pl_slam_amd.track).  numpy only at import."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import trackref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KP = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
STATE = np.dtype([("frame_id", "<i8"), ("ref_kf", "<i4"), ("n_matches_inliers", "<i4"), ("last_kf_id", "<u4"), ("last_reloc_frame_id", "<u4"),
                  ("min_frames", "<i4"), ("max_frames", "<i4"), ("n_kfs", "<i4"), ("flags", "<i4")])
CAM = (517.306408, 516.469215, 318.643040, 255.313989, 40.0)      # fx, fy, cx, cy, bf of TUM1.yaml
TH_DEPTH = np.float32(40.0 * 40.0 / 517.306408)                     # mThDepth = mbf * ThDepth / fx
F32 = np.float32


def rodrigues(w):
    th = float(np.linalg.norm(w))
    if th < 1e-12:
        return np.eye(3)
    k = np.asarray(w, float) / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def pose12(rng, rot=0.3, trans=1.0):
    Rm = rodrigues(rng.normal(size=3) * rot)
    t = rng.normal(size=3) * trans
    return np.concatenate([Rm, t[:, None]], axis=1).astype(F32).reshape(-1)


def make_frame(seed, n, depth="mixed", n_points=400, match_frac=0.3, stride=None, row_id=False):
    """one frame of n key points.  depth: "mixed" (about 0.4 to 3 times th_depth, a tenth invalid), or an array of n floats.  A third of the matches name a
    point without observations, a few an id outside the map."""
    rng = np.random.default_rng(seed)
    stride = n if stride is None else stride
    keys = np.zeros(stride, KP)
    keys["x"][:n] = rng.uniform(0, 640, n).astype(F32)
    keys["y"][:n] = rng.uniform(0, 480, n).astype(F32)
    d = np.zeros(stride, F32)
    if isinstance(depth, str):
        z = rng.uniform(0.4, 3.0, n) * float(TH_DEPTH) * rng.choice([0.2, 1.0], n)
        z[rng.random(n) < 0.1] = -1.0
        d[:n] = z.astype(F32)
    else:
        d[:n] = np.asarray(depth, F32)
    match = np.full(stride, -1, np.int32)
    n_obs = rng.integers(0, 4, n_points).astype(np.int32)
    n_obs[rng.random(n_points) < 0.3] = 0
    rid = None
    rows = n_points
    if row_id:
        rows = max(n_points // 2, 1)
        rid = rng.integers(-2, n_points + 3, rows).astype(np.int32)
    if n:
        who = rng.random(n) < match_frac
        match[:n][who] = rng.integers(0, rows, int(who.sum())).astype(np.int32)
        odd = who & (rng.random(n) < 0.05)
        match[:n][odd] = rows + 7                                    # outside the map (or the row table)
    pose = pose12(rng)
    return dict(n=n, keys=keys, depth=d, match=match, n_obs=n_obs, row_id=rid, pose=pose, frustum=R.frustum(pose))


def pack(frames):
    """frames of one stride and one map -> the batch arrays"""
    S = len(frames[0]["depth"])
    p = dict(keys=np.stack([f["keys"] for f in frames]), depth=np.stack([f["depth"] for f in frames]), match=np.stack([f["match"] for f in frames]),
             n=np.array([f["n"] for f in frames], np.int32), n_obs=frames[0]["n_obs"], frustum=np.stack([f["frustum"] for f in frames]).astype(F32),
             row_id=np.stack([f["row_id"] for f in frames]) if frames[0]["row_id"] is not None else None, stride=S)
    return p


def ref_close(p, th_depth=TH_DEPTH, min_points=100, new_stride=None, id_base=None, last=None):
    """the definition over a batch, with the call's output conventions.  Returns dict(new_kp, new_pos, n_new, n_walked, status, match[, last arrays])"""
    Fn, S = p["match"].shape
    ns = S if new_stride is None else new_stride
    out = dict(new_kp=np.full((Fn, ns), -1, np.int32), new_pos=np.zeros((Fn, ns, 3), F32), n_new=np.zeros(Fn, np.int32), n_walked=np.zeros(Fn, np.int32),
               status=np.zeros(Fn, np.int32), match=p["match"].copy())
    if last is not None:
        out["last"] = tuple(a.copy() for a in last)
    for f in range(Fn):
        kxy = np.stack([p["keys"][f]["x"], p["keys"][f]["y"]], axis=1)
        kp, pos, walked = R.close_points(kxy, p["depth"][f], p["match"][f], int(p["n"][f]), p["n_obs"], p["frustum"][f], CAM, th_depth, min_points,
                                         p["row_id"][f] if p["row_id"] is not None else None)
        k = min(len(kp), ns)
        out["new_kp"][f, :k] = kp[:k]
        out["new_pos"][f, :k] = pos[:k]
        out["n_new"][f], out["n_walked"][f], out["status"][f] = len(kp), walked, 1 if len(kp) > ns else 0
        if id_base is not None:
            out["match"][f, kp[:k]] = id_base[f] + np.arange(k, dtype=np.int32)
        if last is not None:
            out["last"][0][f, kp[:k]] = 1
            out["last"][1][f, kp[:k]] = pos[:k]
            out["last"][2][f, kp[:k]] = 0
    return out


_cpu = None


def cpu_loop():
    """tools/track_cpu.cpp built as a shared object (the build line of its header)"""
    global _cpu
    if _cpu is None:
        so = os.path.join(tempfile.mkdtemp(prefix="track_cpu_"), "track_cpu.so")
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", os.path.join(ROOT, "tools", "track_cpu.cpp"), "-o", so])
        _cpu = C.CDLL(so)
        P, I, Fl = C.c_void_p, C.c_int32, C.c_float
        _cpu.track_cpu_close_points.argtypes = [I, I, P, P, P, P, I, P, I, P, I, P, P, Fl, I, I, P, P, P, P, P]
        _cpu.track_cpu_need_keyframe.argtypes = [I, I, P, P, P, I, P, I, P, I, P, P, I, P, P, P, Fl, P, P]
        _cpu.track_cpu_motion.argtypes = [I, I] + [P] * 11
        _cpu.track_cpu_clean.argtypes = [I, P, P, P, I, I, I, P, I, P, I]
        for fn in (_cpu.track_cpu_close_points, _cpu.track_cpu_need_keyframe, _cpu.track_cpu_motion, _cpu.track_cpu_clean):
            fn.restype = None
    return _cpu


def ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def cpu_close(p, th_depth=TH_DEPTH, min_points=100, new_stride=None, id_base=None, seconds=None):
    """tools/track_cpu.cpp over a packed batch; seconds: a list that receives the time of the loop itself"""
    import time
    Fn, S = p["match"].shape
    ns = S if new_stride is None else new_stride
    out = dict(new_kp=np.full((Fn, ns), -1, np.int32), new_pos=np.zeros((Fn, ns, 3), F32), n_new=np.zeros(Fn, np.int32), n_walked=np.zeros(Fn, np.int32),
               match=np.ascontiguousarray(p["match"]).copy())
    cam = np.array(CAM[:4], F32)
    rid = p["row_id"]
    keep = [np.ascontiguousarray(p[k]) for k in ("keys", "depth", "n", "n_obs", "frustum")]
    fn = cpu_loop().track_cpu_close_points
    t0 = time.perf_counter()
    fn(Fn, S, ptr(keep[0]), ptr(keep[1]), ptr(out["match"]), ptr(keep[2]), 0, ptr(rid), rid.shape[1] if rid is not None else 0, ptr(keep[3]), len(keep[3]),
       ptr(keep[4]), ptr(cam), float(th_depth), min_points, ns, ptr(np.asarray(id_base, np.int32)) if id_base is not None else None, ptr(out["new_kp"]),
       ptr(out["new_pos"]), ptr(out["n_new"]), ptr(out["n_walked"]))
    if seconds is not None:
        seconds.append(time.perf_counter() - t0)
    out["status"] = (out["n_new"] > ns).astype(np.int32)
    return out


def dev_close(p, th_depth=TH_DEPTH, min_points=100, new_stride=None, id_base=None, last=None, n_host=None):
    """the device call over a packed batch; returns host copies shaped as ref_close's"""
    import torch
    from rgbd_pl_slam_amd import close_points
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    keys = t(np.frombuffer(np.ascontiguousarray(p["keys"]).tobytes(), np.uint8).reshape(p["match"].shape[0], -1).copy())
    match = t(p["match"])
    lastd = tuple(t(a) for a in last) if last is not None else None
    r = close_points(keys, t(p["depth"]), match, t(p["n_obs"]), t(p["frustum"]), CAM, float(th_depth), min_points, n=n_host if n_host is not None else t(p["n"]),
                     row_id=t(p["row_id"]) if p["row_id"] is not None else None, new_stride=new_stride,
                     id_base=t(np.asarray(id_base, np.int32)) if id_base is not None else None, last=lastd)
    torch.cuda.synchronize()
    out = dict(new_kp=r.new_kp.cpu().numpy(), new_pos=r.new_pos.cpu().numpy(), n_new=r.n_new.cpu().numpy(), n_walked=r.n_walked.cpu().numpy(),
               status=r.status.cpu().numpy(), match=match.cpu().numpy())
    if last is not None:
        out["last"] = tuple(a.cpu().numpy() for a in lastd)
    return out


def same_bits(a, b):
    """bit equality of two float arrays; a NaN equals any NaN"""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


def assert_close_equal(got, want, what=""):
    for k in ("n_new", "n_walked", "status", "new_kp", "match"):
        if k in want and k in got:
            assert np.array_equal(got[k], want[k]), (what, k, got[k], want[k])
    assert same_bits(got["new_pos"], want["new_pos"]), (what, "new_pos")
    if "last" in want:
        assert np.array_equal(got["last"][0], want["last"][0]) and same_bits(got["last"][1], want["last"][1]) and np.array_equal(got["last"][2], want["last"][2]), (what, "last")


def state(**kw):
    """one plf_track_kf_state as a dict, the reference's defaults of a 30 fps RGB-D run"""
    s = dict(frame_id=100, ref_kf=0, n_matches_inliers=60, last_kf_id=90, last_reloc_frame_id=0, min_frames=0, max_frames=30, n_kfs=5, flags=R.MAPPER_IDLE)
    s.update(kw)
    return s


def state_records(states):
    a = np.zeros(len(states), STATE)
    for i, s in enumerate(states):
        for k, v in s.items():
            a[i][k] = v
    return a


def truth_table():
    """(state, inliers, nTotal, nMap, nRef) rows with every count and ratio at, one below and one above each threshold of NeedNewKeyFrame, nKFs at 1 / 2 / 3"""
    rows = []
    for n_kfs in (1, 2, 3):
        for flags in (R.MAPPER_IDLE, 0, R.MONO | R.MAPPER_IDLE, R.MONO, R.ONLY_TRACKING | R.MAPPER_IDLE, R.MAPPER_STOPPED | R.MAPPER_IDLE):
            # inliers around 15 and 300; nRef where nRef * 0.25 (64, 65, 68; 1200, 1201, 1204) and nRef * 0.75 / 0.4 / 0.9 (21, 22; 40, 41; 17, 18) cross them;
            # nMap / nTotal around 0.3, 0.35 and 0.20; the frame id at and either side of mnLastKeyFrameId + mMaxFrames, and inside / outside mMinFrames
            for inl in (15, 16, 17, 300, 301):
                for n_ref in (0, 17, 18, 21, 22, 40, 41, 64, 65, 68, 1200, 1201, 1204):
                    for (n_map, n_total) in ((0, 0), (29, 100), (30, 100), (31, 100), (34, 100), (35, 100), (36, 100), (19, 100), (20, 100), (21, 100), (100, 100)):
                        for fid, last_kf in ((100, 90), (100, 70), (100, 71), (100, 98)):
                            rows.append((state(frame_id=fid, last_kf_id=last_kf, n_kfs=n_kfs, flags=flags, min_frames=5), inl, n_total, n_map, n_ref))
    # the relocalisation guard, with nKFs at and above mMaxFrames, and the 32-bit wrap of the sums
    for n_kfs in (30, 31):
        for reloc in (69, 70, 71):
            rows.append((state(frame_id=100, last_kf_id=10, last_reloc_frame_id=reloc, n_kfs=n_kfs), 40, 100, 10, 100))
    rows.append((state(frame_id=5, last_kf_id=0xFFFFFFF0, max_frames=30, min_frames=20, n_kfs=4, flags=0), 40, 100, 50, 100))
    rows.append((state(frame_id=5, last_kf_id=0xFFFFFFF0, max_frames=30, min_frames=10, n_kfs=4, flags=0), 40, 100, 50, 100))
    return rows


ENTRY_COUNTS = (0, 1, 2, 63, 64, 65, 100, 101, 102, 127, 128, 129, 1000, 1023, 1024, 1025, 4000)
NON_ENTRIES = np.array([0.0, -1.0, np.nan, -0.0, -np.inf], F32)


def depths_with_entries(seed, c, extras=True):
    """c depths > 0 (a third beyond th_depth) and, with extras, the five kinds of non-entries, shuffled"""
    rng = np.random.default_rng(1000 + seed)
    z = (rng.uniform(0.3, 1.0, c) * float(TH_DEPTH) * rng.choice([1.0, 1.0, 2.5], c)).astype(F32)
    if extras:
        z = np.concatenate([z, NON_ENTRIES])
    rng.shuffle(z)
    return z


def close_fixtures():
    """name -> (packed batch, keyword arguments of ref_close / cpu_close / dev_close).  What each is for is in its name; tests/test_gpu_track.py runs every one
    on the device, tests/test_track_ref.py through the C++ loop."""
    fx = {}
    th = float(TH_DEPTH)
    for c in ENTRY_COUNTS:                                           # lane, wave, padding and size-class edges; kp_stride <= 1024 is the one-wave class
        z = depths_with_entries(c, c, extras=c not in (1023, 1024))
        fx["entries_%d" % c] = (pack([make_frame(c, len(z), z)]), {})
    z = depths_with_entries(7, 1024, extras=False)
    for name, S in (("batch_wave", 1024), ("batch_block", 1030)):    # per-frame n in one call, in both classes
        fr = [make_frame(20 + k, nn, z[:nn] if nn <= 1024 else np.concatenate([z, z[:nn - 1024]]), stride=S) for k, nn in enumerate((0, 65, 1024) + ((1030,) if S > 1024 else ()))]
        fx[name] = (pack(fr), {})
    fx["largest_stride"] = (pack([make_frame(29, 16384, depths_with_entries(29, 16379))]), {})                   # 16384 keys: the whole 128 KB of LDS
    fx["all_nonpositive"] = (pack([make_frame(30, 70, -np.abs(depths_with_entries(30, 70, False)))]), {})
    fx["all_equal"] = (pack([make_frame(31, 200, np.full(200, 0.5 * th, F32), match_frac=0.5)]), {})            # the index alone decides the order
    fx["all_equal_far"] = (pack([make_frame(32, 200, np.full(200, 2.0 * th, F32), match_frac=0.5)]), {})
    rng = np.random.default_rng(33)
    runs = (np.arange(300) // 37).astype(F32) * F32(0.25) + F32(1.0)                                              # runs of 37 equal depths: they straddle lanes 63 | 64
    rng.shuffle(runs)
    fx["equal_runs"] = (pack([make_frame(33, 300, runs, match_frac=0.5)]), {})
    for c in (99, 100, 101, 102):                                    # every entry beyond th_depth: the walk ends at entry 101
        fx["far_%d" % c] = (pack([make_frame(40 + c, c, (rng.uniform(1.5, 3.0, c) * th).astype(F32))]), {})
    z = np.concatenate([rng.uniform(0.2, 0.9, 150) * th, rng.uniform(1.1, 3.0, 150) * th]).astype(F32)
    rng.shuffle(z)
    fx["close_150_then_far"] = (pack([make_frame(50, 300, z)]), {})
    z = np.concatenate([rng.uniform(0.2, 0.9, 50) * th, rng.uniform(1.1, 3.0, 150) * th]).astype(F32)
    rng.shuffle(z)
    fx["close_50_then_far"] = (pack([make_frame(51, 200, z)]), {})
    z = depths_with_entries(52, 90)
    z[:12] = np.array([np.nan, np.inf, -0.0, 1e-45, 1e-40, 1.1754942e-38, np.inf, -np.nan, 3.4e38, 1e-45, 0.0, -1e-45], F32)
    fx["special_depths"] = (pack([make_frame(52, len(z), z)]), dict(min_points=40))
    fx["nan_threshold"] = (pack([make_frame(53, 200, depths_with_entries(53, 195))]), dict(th_depth=float("nan")))
    fx["no_cut"] = (pack([make_frame(54, 300, depths_with_entries(54, 295))]), dict(min_points=2 ** 31 - 1))
    fx["negative_min_points"] = (pack([make_frame(55, 100, depths_with_entries(55, 95))]), dict(min_points=-3))
    fx["all_matched_no_obs"] = (pack([make_frame(56, 150, depths_with_entries(56, 145), match_frac=1.0)]), {})   # matches with n_obs 0 are created again
    fx["row_id"] = (pack([make_frame(57 + k, 300, stride=320, row_id=True, match_frac=0.6) for k in range(3)]), {})
    fx["row_id_block"] = (pack([make_frame(60 + k, 1500, stride=1500, row_id=True, match_frac=0.6) for k in range(2)]), {})
    fx["short_list"] = (pack([make_frame(63 + k, 300) for k in range(2)]), dict(new_stride=10))                 # status bit, true count, nothing beyond the stride
    fx["short_list_block"] = (pack([make_frame(65, 1100)]), dict(new_stride=70))
    fx["keyframe_mode"] = (pack([make_frame(66 + k, 300, match_frac=0.5) for k in range(3)]), dict(id_base=[400, 1000, 5000]))
    fx["keyframe_mode_short"] = (pack([make_frame(69, 300, match_frac=0.5)]), dict(id_base=[400], new_stride=20))
    return fx


def last_arrays(p, seed=0):
    """the mutable arrays behind a plf_lastframe_view for a batch: has_mappoint / world_pos / obs_positive as the matches and n_obs say"""
    Fn, S = p["match"].shape
    rng = np.random.default_rng(seed)
    has = (p["match"] >= 0).astype(np.uint8)
    pos = rng.normal(size=(Fn, S, 3)).astype(F32)
    obs = np.ones((Fn, S), np.uint8)
    return has, pos, obs


def tiny_fixture():
    """the content of tests/golden/track_tiny.json: a handful of frames of <= 64 key points with the definition's output bits"""
    frames = [make_frame(90 + k, nn, stride=64, n_points=40, match_frac=0.4) for k, nn in enumerate((0, 1, 40, 64, 64))]
    p = pack(frames)
    kw = dict(min_points=10, id_base=[100, 200, 300, 400, 500])
    r = ref_close(p, **kw)
    bits = lambda a: np.ascontiguousarray(a, F32).view(np.uint32).reshape(-1).tolist()
    rng = np.random.default_rng(99)
    poses = [pose12(rng) for _ in range(6)]
    mo = [R.motion_model(cur=poses[2 * k], last_frustum=R.frustum(poses[2 * k + 1]), tlr=poses[k], tref=poses[k + 3], predict=True) for k in range(3)]
    rows = truth_table()[::2575]
    return {"_doc": "tests/trackgen.py tiny_fixture(): inputs and the output bits of tests/trackref.py; floats as uint32 bit patterns",
            "cam": bits(np.array(CAM, F32)), "th_depth": bits(np.array([TH_DEPTH])), "min_points": 10, "id_base": kw["id_base"],
            "n": p["n"].tolist(), "keys_x": bits(p["keys"]["x"]), "keys_y": bits(p["keys"]["y"]), "depth": bits(p["depth"]), "match": p["match"].reshape(-1).tolist(),
            "n_obs": p["n_obs"].tolist(), "frustum": bits(p["frustum"]),
            "out": {"new_kp": r["new_kp"].reshape(-1).tolist(), "new_pos": bits(r["new_pos"]), "n_new": r["n_new"].tolist(), "n_walked": r["n_walked"].tolist(),
                    "match": r["match"].reshape(-1).tolist()},
            "poses": bits(np.stack(poses)),
            "motion": [{k: bits(v) for k, v in m.items() if k != "status"} for m in mo],
            "decide": [[{k: int(v) for k, v in s.items()}, inl, nt, nm, nr, R.decide(s, inl, nt, nm, nr)] for (s, inl, nt, nm, nr) in rows]}


if __name__ == "__main__":
    import json
    import sys
    if sys.argv[1:] == ["--write-golden"]:
        with open(os.path.join(ROOT, "tests", "golden", "track_tiny.json"), "w") as fh:
            json.dump(tiny_fixture(), fh, separators=(",", ":"))
            fh.write("\n")

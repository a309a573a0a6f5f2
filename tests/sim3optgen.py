"""Scenes for the Sim3 optimisation (include/plf.h, "Sim3 optimisation"): pairs of keyframes over a shared cloud under a known similarity transform, with
key points at the projections (plus noise), octaves over all levels, gross outliers, NULL and bad points, absent observations, and a start transform
off the truth by a chosen angle and distance.  The scene is the dict of tests/sim3gen.py (so the Sim3 solver's definition runs on it too) plus
inv_level_sigma2, sim3_in and th2.  Also the glue that runs a scene through tests/sim3optref.py, through the host loop tools/sim3opt_cpu.cpp and through
the device, and the writer of tests/golden/sim3opt_tiny.json (python tests/sim3optgen.py --write-golden)."""
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sim3gen as G  # noqa: E402
import sim3optref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
GOLDEN = os.path.join(ROOT, "tests", "golden", "sim3opt_tiny.json")
ptr, same_bits = G.ptr, G.same_bits


def inv_level_sigma2():
    return (F32(1.0) / G.level_sigma2()).astype(F32)


def _project(cam, X):
    return np.stack([cam[0] * X[:, 0] / X[:, 2] + cam[2], cam[1] * X[:, 1] / X[:, 2] + cam[3]], 1)


def make_scene(seed, jobs, obs_index=False, th2=10.0, kp_stride=None):
    """jobs: a list of dicts: n1 (key points of keyframe 1), n2 (default n1), pairs (correspondences with two good points), outliers (share of those
    whose key point in keyframe 1 is `out_px` = 30 px off), noise (px, default 0.5), null / bad / noobs (further matches whose point in keyframe 1 is NULL /
    with a bad point / whose point has no observation in keyframe 2: needs obs_index), fix_scale, scale (the true s12), angle (of the true R12),
    off_deg / off_t (the start transform's distance from the truth; default 2 degrees, 0.05).  Each job has its own two keyframes (slots 2 j, 2 j + 1)."""
    rng = np.random.default_rng(seed)
    cam = G.CAM.copy()
    kf_n, kf_pose, kf_keys, kf_oct, kf_mp, kf_obs = [], [], [], [], [], []
    world, bad = [], []
    S = kp_stride or max(max(j["n1"] for j in jobs), 1)
    match12 = np.full((len(jobs), S), -1, np.int32)
    sim3_in = np.zeros((len(jobs), 13), F32)
    truth = []
    for jn, jb in enumerate(jobs):
        n1, n2 = jb["n1"], jb.get("n2", jb["n1"])
        m, n_null, n_bad, n_noobs = jb["pairs"], jb.get("null", 0), jb.get("bad", 0), jb.get("noobs", 0)
        tot = m + n_null + n_bad + n_noobs
        assert tot <= min(n1, n2) and (obs_index or not n_noobs)
        s12 = jb.get("scale", 1.0)
        R12, t12 = G._rot(rng, jb.get("angle", 0.2)), rng.normal(size=3) * 0.3
        Xc1 = np.stack([rng.uniform(-2, 2, tot), rng.uniform(-1.5, 1.5, tot), rng.uniform(2, 8, tot)], 1)
        Xc2 = (Xc1 - t12) @ R12 / s12                       # x1 = s R x2 + t
        Rcw1, tcw1 = G._rot(rng, rng.uniform(0, 3)), rng.normal(size=3)
        Rcw2, tcw2 = G._rot(rng, rng.uniform(0, 3)), rng.normal(size=3)
        X1w, X2w = (Xc1 - tcw1) @ Rcw1, (Xc2 - tcw2) @ Rcw2
        f1, f2 = rng.permutation(n1)[:tot], rng.permutation(n2)[:tot]
        base = len(world)
        mp1, mp2 = np.full(n1, -1, np.int32), np.full(n2, -1, np.int32)
        mp1[f1] = base + np.arange(tot)
        mp2[f2] = base + tot + np.arange(tot)
        world += list(X1w) + list(X2w)
        bad += [0] * (2 * tot)
        if f1[f1 < S].size:
            match12[jn, f1[f1 < S]] = f2[f1 < S]
        mp1[f1[m:m + n_null]] = -1
        for k in range(m + n_null, m + n_null + n_bad):
            bad[base + k + (tot if (k & 1) else 0)] = 1    # alternately the point of keyframe 1 and of keyframe 2
        noise = jb.get("noise", 0.5)
        uv1 = _project(cam, Xc1) + rng.normal(size=(tot, 2)) * noise
        uv2 = _project(cam, Xc2) + rng.normal(size=(tot, 2)) * noise
        n_out = int(round(jb.get("outliers", 0.0) * m))
        who = rng.permutation(m)[:n_out]
        ang = rng.uniform(0, 2 * np.pi, n_out)
        uv1[who] += jb.get("out_px", 30.0) * np.stack([np.cos(ang), np.sin(ang)], 1)
        obs2 = np.arange(n2, dtype=np.int32)
        obs2[f2[m + n_null + n_bad:tot]] = -1
        for n, mp, Rcw, tcw, f, uv in ((n1, mp1, Rcw1, tcw1, f1, uv1), (n2, mp2, Rcw2, tcw2, f2, uv2)):
            keys = np.zeros((n, 7), F32)
            keys[:, 0], keys[:, 1] = rng.uniform(0, 640, n), rng.uniform(0, 480, n)
            keys[f, 0:2] = uv
            octv = (rng.integers(0, G.NLEVELS, n)).astype(np.int32)
            keys[:, 5] = octv.view(F32)
            kf_n.append(n); kf_pose.append(G._pose(Rcw, tcw)); kf_keys.append(keys); kf_oct.append(octv); kf_mp.append(mp)
        kf_obs += [np.arange(n1, dtype=np.int32), obs2]
        # the start: the truth turned by off_deg about a random axis and moved by off_t
        Rs = G._rot(rng, np.deg2rad(jb.get("off_deg", 2.0))) @ R12
        d = rng.normal(size=3)
        ts = t12 + jb.get("off_t", 0.05) * d / np.linalg.norm(d)
        sim3_in[jn] = np.concatenate([Rs.ravel(), ts, [s12 * jb.get("off_s", 1.0)]]).astype(F32)
        good = np.ones(m, bool)
        good[who] = False
        truth.append(dict(R=R12, t=t12, s=s12, good_i1=np.sort(f1[:m][good]), outlier_i1=np.sort(f1[:m][~good])))
    J = len(jobs)
    sc = dict(cam=cam, level_sigma2=G.level_sigma2(), inv_level_sigma2=inv_level_sigma2(), kf_n=np.array(kf_n, np.int32),
              kf_pose=np.array(kf_pose, F32).reshape(-1, 15), kf_keys=kf_keys, kf_octave=kf_oct, kf_mappoints=kf_mp, kf_obs_index=kf_obs if obs_index else None,
              world_pos=np.array(world, F32).reshape(-1, 3), point_bad=np.array(bad, np.uint8), job_kf1=np.arange(0, 2 * J, 2, dtype=np.int32),
              job_kf2=np.arange(1, 2 * J, 2, dtype=np.int32), match12=match12, fix_scale=np.array([1 if jb.get("fix_scale") else 0 for jb in jobs], np.uint8),
              sim3_in=sim3_in, th2=th2, truth=truth)
    return sc


def standard_scene():
    """the scene of the CPU tests: small enough for the plain-Python definition to take seconds"""
    jobs = [dict(n1=40, pairs=24, outliers=0.3, null=2, bad=3),                           # 0: culls, 10 more iterations
            dict(n1=30, pairs=16, fix_scale=True),                                        # 1: clean, fixed scale: culls nothing, 5 more
            dict(n1=30, pairs=14, scale=1.3, off_s=1.05),                                 # 2: free scale off by 5 %
            dict(n1=20, pairs=9),                                                         # 3: FEW before anything is culled
            dict(n1=30, pairs=12, outliers=0.3),                                          # 4: drops below 10 after the cull
            dict(n1=12, pairs=0)]                                                         # 5: no correspondence at all
    return make_scene(7, jobs)


def tiny_scene():
    return make_scene(5, [dict(n1=16, pairs=12, outliers=0.17), dict(n1=14, pairs=11, fix_scale=True), dict(n1=12, pairs=8)])


# ---- runs
def ref_run(sc):
    return R.run(sc)


def _view(L, sc, keep):
    tk, tm = G._table(keep), G._table(sc["kf_mappoints"])
    to = G._table(sc["kf_obs_index"]) if sc["kf_obs_index"] is not None else None
    v = L.Sim3View(len(sc["kf_n"]), C.cast(tk, C.c_void_p), ptr(sc["kf_n"]), ptr(sc["kf_pose"]), C.cast(tm, C.c_void_p), C.cast(to, C.c_void_p) if to else None,
                   ptr(sc["world_pos"]), ptr(sc["point_bad"]), len(sc["point_bad"]), None, len(sc["inv_level_sigma2"]))
    return v, (tk, tm, to)


def cpu_run(lib, sc):
    """tools/sim3opt_cpu.cpp on the scene, as ref_run; counters: the iteration counts given to the two optimize() calls"""
    from rgbd_pl_slam_amd import _lib as L
    L.sim3opt_prototypes(lib, "sim3opt_cpu")
    J, S = sc["match12"].shape
    keep = [np.ascontiguousarray(k) for k in sc["kf_keys"]]
    v, hold = _view(L, sc, keep)
    sim3_in = np.ascontiguousarray(sc["sim3_in"], F32)
    jobs = L.Sim3OptJobs(J, S, ptr(sc["job_kf1"]), ptr(sc["job_kf2"]), ptr(sim3_in), ptr(sc["fix_scale"]), ptr(sc["inv_level_sigma2"]), float(sc["th2"]))
    cam = L.Camera(*[float(x) for x in sc["cam"]])
    out = dict(sim3=np.zeros((J, 8)), match12=sc["match12"].copy(), scw=np.full((J, 16), np.nan, F32), n_inliers=np.zeros(J, np.int32), status=np.zeros(J, np.int32))
    its = np.zeros((J, 2), np.int32)
    assert lib.sim3opt_cpu_optimize(C.byref(v), C.byref(cam), C.byref(jobs), ptr(out["match12"]), ptr(out["sim3"]), ptr(out["scw"]), ptr(out["n_inliers"]),
                                    ptr(out["status"]), ptr(its)) == 0
    out["its"] = its
    return out


def gpu_run(sc, stream=None):
    """the device call on the scene through rgbd_pl_slam_amd.sim3opt, read back at the end"""
    import torch
    from rgbd_pl_slam_amd import sim3 as S3, sim3opt as SO
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    keys = [t(np.ascontiguousarray(k).view(np.uint8).reshape(-1)) for k in sc["kf_keys"]]
    mps = [t(m) for m in sc["kf_mappoints"]]
    obs = [t(o) for o in sc["kf_obs_index"]] if sc["kf_obs_index"] is not None else None
    kfs = S3.Sim3KeyFrames(keys, mps, t(sc["kf_pose"]), obs)
    cam = tuple(float(x) for x in sc["cam"][[0, 1, 2, 3, 9]])
    J = sc["match12"].shape[0]
    match = t(sc["match12"])
    pre = SO.Sim3Result(sim3=torch.zeros((J, 8), dtype=torch.float64, device=dev), scw=torch.full((J, 16), float("nan"), dtype=torch.float32, device=dev),
                        n_inliers=torch.zeros(J, dtype=torch.int32, device=dev), status=torch.zeros(J, dtype=torch.int32, device=dev))
    o = SO.sim3_optimize(kfs, t(sc["job_kf1"]), t(sc["job_kf2"]), match, t(np.ascontiguousarray(sc["sim3_in"], F32)), t(sc["fix_scale"]), t(sc["world_pos"]),
                         t(sc["point_bad"]), t(sc["inv_level_sigma2"]), cam, th2=sc["th2"], out=pre, stream=stream)
    torch.cuda.synchronize()
    return dict(sim3=o.sim3.cpu().numpy(), match12=match.cpu().numpy(), scw=o.scw.cpu().numpy(), n_inliers=o.n_inliers.cpu().numpy(), status=o.status.cpu().numpy())


def same_doubles(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and a[~nan].tobytes() == b[~nan].tobytes()


def compare(ref, got, what=""):
    """two runs bit for bit (a NaN equals any NaN), the matches entry by entry"""
    assert np.array_equal(ref["status"], got["status"]), (what, "status", ref["status"], got["status"])
    assert np.array_equal(ref["n_inliers"], got["n_inliers"]), (what, "n_inliers", ref["n_inliers"], got["n_inliers"])
    for j in range(len(ref["status"])):
        assert same_doubles(ref["sim3"][j], got["sim3"][j]), (what, "sim3", j, ref["sim3"][j], got["sim3"][j])
        assert np.array_equal(ref["match12"][j], got["match12"][j]), (what, "match12", j, np.nonzero(ref["match12"][j] != got["match12"][j]))
        assert same_bits(ref["scw"][j], got["scw"][j]), (what, "scw", j, ref["scw"][j], got["scw"][j])


def golden_of(sc):
    r = ref_run(sc)
    u32 = lambda a: np.ascontiguousarray(a, F32).view(np.uint32).ravel().tolist()  # noqa: E731
    inputs = dict(sim3_in=u32(sc["sim3_in"]), world_pos=u32(sc["world_pos"]), kf_pose=u32(sc["kf_pose"]), match12=sc["match12"].ravel().tolist(),
                  keys_xy=[u32(k[:, 0:2]) for k in sc["kf_keys"]], octave=[o.tolist() for o in sc["kf_octave"]], mappoints=[m.tolist() for m in sc["kf_mappoints"]],
                  fix_scale=sc["fix_scale"].tolist(), th2=sc["th2"])
    return dict(inputs=inputs, sim3=[R.d2hex(float(x)) for x in r["sim3"].ravel()], scw=np.ascontiguousarray(r["scw"], F32).view(np.uint32).ravel().tolist(),
                match12=r["match12"].ravel().tolist(), n_inliers=r["n_inliers"].tolist(), status=r["status"].tolist(),
                optimize=[c["optimize"] for c in r["counters"]])


def dump(sc, path):
    """the flat file tools/sim3opt_cpu.cpp's stand-alone program reads"""
    J, S = sc["match12"].shape
    has_obs = sc["kf_obs_index"] is not None
    with open(path, "wb") as fh:
        fh.write(np.array([len(sc["kf_n"]), len(sc["point_bad"]), len(sc["inv_level_sigma2"]), J, S, int(has_obs)], np.int32).tobytes())
        fh.write(sc["cam"].tobytes() + np.array([sc["th2"]], F32).tobytes() + sc["kf_n"].tobytes() + sc["kf_pose"].tobytes())
        for s in range(len(sc["kf_n"])):
            fh.write(np.ascontiguousarray(sc["kf_keys"][s]).tobytes() + sc["kf_mappoints"][s].tobytes())
            if has_obs:
                fh.write(sc["kf_obs_index"][s].tobytes())
        fh.write(sc["world_pos"].tobytes() + sc["point_bad"].tobytes() + sc["inv_level_sigma2"].tobytes() + sc["job_kf1"].tobytes() + sc["job_kf2"].tobytes()
                 + np.ascontiguousarray(sc["match12"]).tobytes() + sc["fix_scale"].tobytes() + np.ascontiguousarray(sc["sim3_in"], F32).tobytes())


def all_scenes():
    """(name, scene): what the stand-alone program of tools/sim3opt_cpu.cpp is run over"""
    yield "standard", standard_scene()
    yield "tiny", tiny_scene()
    sc = make_scene(61, [dict(n1=70, pairs=40, null=4, bad=6, noobs=5, outliers=0.1), dict(n1=60, pairs=30, noobs=3, fix_scale=True, off_deg=20.0)], obs_index=True)
    live = np.nonzero(sc["match12"][0] >= 0)[0]
    sc["match12"][0, live[0]] = 10 ** 6
    sc["kf_obs_index"][1][sc["match12"][0, live[2]]] = sc["kf_n"][1] + 5
    sc["kf_mappoints"][0][live[3]] = len(sc["point_bad"])
    sc["sim3_in"][1, 4] = np.nan
    yield "indices", sc
    sc = make_scene(41, [dict(n1=1100, pairs=1030, outliers=0.05), dict(n1=40, pairs=20)])
    sc["job_kf2"][1] = 99
    yield "long", sc


if __name__ == "__main__":
    if "--dump" in sys.argv:
        d = sys.argv[sys.argv.index("--dump") + 1]
        os.makedirs(d, exist_ok=True)
        for name, sc in all_scenes():
            dump(sc, os.path.join(d, name + ".dump"))
    if "--write-golden" in sys.argv:
        os.makedirs(os.path.dirname(GOLDEN), exist_ok=True)
        with open(GOLDEN, "w") as fh:
            json.dump(golden_of(tiny_scene()), fh, separators=(",", ":"))
        print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")

"""tools/bench_pose.py -- time of the GPU PoseOptimization (plf_pose_optimize: one launch, one wave per frame, the four Levenberg rounds inside), device
in and out, on two shapes:
  frames  8192 frames x 1000 key points of which 300 are matched (every other one a stereo edge), 10 % of the matches displaced by 50 px, the start
          pose off by 2 degrees and 5 cm
  single  the first of those frames alone: what a one-frame caller pays
Warm-up, then the median of `--calls` calls timed with device events on one stream.  Beside it the single-thread loop a caller runs today
(tools/pose_cpu.cpp: the same arithmetic, g++ -O2 -ffp-contract=off, on the host this tool runs on) over the first `--cpu-frames` frames, scaled to
the frame count, and whether the two write the same bits there (pose, flags, counts, status).  States whether the device call is no slower than the
C++ loop at the 8192-frame shape.  Writes profiles/pose.json.

The per-kernel time comes from a kernel trace taken in a run of its own:
    rocprofv3 --kernel-trace --stats -d DIR --output-format csv -- python tools/bench_pose.py --calls 3 --no-json --no-cpu --shape SHAPE
    python tools/bench_pose.py --kernel-stats DIR --shape SHAPE
A measurement needs the GPU: without one this tool fails, it does not fall back."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import benchlib  # noqa: E402
OUT = os.path.join(ROOT, "profiles", "pose.json")
N_FRAMES, N_KP, N_MATCH = 8192, 1000, 300


def make_frames(F, rng):
    """F frames in the layout of tests/posegen.pack, vectorised"""
    import numpy as np
    import posegen
    fx, fy, cx, cy, bf = posegen.CAM

    def rot(w):
        th = np.linalg.norm(w, axis=1)[:, None, None]
        k = w / np.maximum(th[:, :, 0], 1e-12)
        K = np.zeros((len(w), 3, 3))
        K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -k[:, 2], k[:, 1], k[:, 2], -k[:, 0], -k[:, 1], k[:, 0]
        return np.eye(3)[None] + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)

    Rt, tt = rot(rng.normal(size=(F, 3)) * 0.3), rng.normal(size=(F, 3)) * 0.5
    z = rng.uniform(1.0, 8.0, (F, N_MATCH))
    u, v = rng.uniform(20.0, 620.0, (F, N_MATCH)), rng.uniform(20.0, 460.0, (F, N_MATCH))
    Xc = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], 2)
    world = np.einsum("fji,fnj->fni", Rt, Xc - tt[:, None, :]).astype(np.float32)
    T = np.concatenate([Rt, tt[:, :, None]], 2).astype(np.float32)
    Xc = np.einsum("fij,fnj->fni", T[:, :, :3].astype(np.float64), world.astype(np.float64)) + T[:, None, :, 3]
    pu, pv = Xc[..., 0] / Xc[..., 2] * fx + cx, Xc[..., 1] / Xc[..., 2] * fy + cy
    pu, pv = pu + rng.normal(size=pu.shape) * 0.5, pv + rng.normal(size=pv.shape) * 0.5
    gross = rng.random((F, N_MATCH)) < 0.1
    ang = rng.uniform(0, 2 * np.pi, (F, N_MATCH))
    pu, pv = pu + gross * 50.0 * np.cos(ang), pv + gross * 50.0 * np.sin(ang)
    keys = np.zeros((F, N_KP), posegen.KP_DTYPE)
    keys["x"], keys["y"] = rng.uniform(0, 640, (F, N_KP)), rng.uniform(0, 480, (F, N_KP))
    keys["octave"] = rng.integers(0, posegen.NLEVELS, (F, N_KP))
    uright = np.full((F, N_KP), -1.0, np.float32)
    match = np.full((F, N_KP), -1, np.int32)
    where = np.sort(np.argsort(rng.random((F, N_KP)), 1)[:, :N_MATCH], 1)
    rows = np.arange(F)[:, None]
    keys["x"][rows, where], keys["y"][rows, where] = pu, pv
    stereo = (np.arange(N_MATCH) % 2 == 1)[None, :]
    uright[rows, where] = np.where(stereo, pu - bf / Xc[..., 2], -1.0)
    match[rows, where] = np.arange(N_MATCH, dtype=np.int32)[None, :]
    Ri = rot(rng.normal(size=(F, 3)) / np.sqrt(3) * np.deg2rad(2.0)) @ Rt
    ti = tt + rng.normal(size=(F, 3)) / np.sqrt(3) * 0.05
    pose = np.concatenate([Ri, ti[:, :, None]], 2).astype(np.float32).reshape(F, 12)
    return dict(keys=keys, uright=uright, match=match, n=np.full(F, N_KP, np.int32), world_pos=world, pose_in=pose, kp_stride=N_KP, pos_stride=N_MATCH)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--frames", type=int, default=N_FRAMES)
    ap.add_argument("--cpu-frames", type=int, default=N_FRAMES)
    ap.add_argument("--no-json", action="store_true")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--shape", default=None, choices=("frames", "single"), help="this shape only (for a kernel trace)")
    ap.add_argument("--kernel-stats", default=None, help="directory of a rocprofv3 --kernel-trace --stats run of this tool: merge the per-kernel time")
    a = ap.parse_args()
    if a.kernel_stats:
        print(json.dumps(benchlib.merge_kernel_stats(OUT, a.kernel_stats, "k_pose_", lambda res, split: res[a.shape or "frames"].update(per_kernel_ms_traced=split))[1]))
        return
    import numpy as np
    import torch
    import posegen
    from rgbd_pl_slam_amd import pose_optimization
    from rgbd_pl_slam_amd.pose import camera, PoseResult
    assert torch.cuda.is_available(), "bench_pose.py needs the GPU"
    F = a.frames
    p = make_frames(F, np.random.default_rng(7))
    cuda = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()   # noqa: E731
    keys = cuda(np.frombuffer(p["keys"].tobytes(), np.uint8).reshape(F, -1))
    uright, match, world, pose_in, sig = cuda(p["uright"]), cuda(p["match"]), cuda(p["world_pos"]), cuda(p["pose_in"]), cuda(posegen.INV_SIGMA2)
    cam = camera(*posegen.CAM)
    st = torch.cuda.Stream()
    res = {"what": "plf_pose_optimize, device in and out, one launch per call; median of calls, device events", "calls": a.calls, "warmup": a.warmup,
           "cpu_loop": "tools/pose_cpu.cpp, one thread, g++ -O2 -ffp-contract=off, on the host of this run, over the first %d frames and scaled to the frame count"
                       % min(a.cpu_frames, F),
           "shape": {"frames": F, "key_points": N_KP, "matches": N_MATCH, "gross_outliers": 0.1, "stereo_share": 0.5}}
    for name, rows in (("frames", F), ("single", 1)):
        if a.shape and a.shape != name:
            continue
        out = PoseResult(pose=torch.empty((rows, 12), dtype=torch.float32, device="cuda"), frustum=torch.empty((rows, 15), dtype=torch.float32, device="cuda"),
                         outlier=torch.zeros((rows, N_KP), dtype=torch.uint8, device="cuda"), n_inliers=torch.empty(rows, dtype=torch.int32, device="cuda"),
                         status=torch.empty(rows, dtype=torch.int32, device="cuda"))
        run = lambda: pose_optimization(keys[:rows], uright[:rows], match[:rows], world[:rows], sig, cam, pose_in[:rows], out=out, stream=st.cuda_stream)   # noqa: E731
        ms, r = benchlib.median_ms(run, st, a.warmup, a.calls)
        torch.cuda.synchronize()
        n_in = r.n_inliers.cpu().numpy()
        row = {"rows": rows, "ms": ms, "us_per_frame": round(ms["median"] * 1000 / rows, 3), "inliers_median": float(np.median(n_in)),
               "status_nonzero": int((r.status.cpu().numpy() != 0).sum())}
        if not a.no_cpu:
            k = min(a.cpu_frames, rows)
            sub = {key: (val[:k] if hasattr(val, "shape") else val) for key, val in p.items()}
            posegen.cpu_loop()                                      # (built before the clock starts)
            t0 = time.perf_counter()
            c = posegen.run_cpu_loop(sub, outlier=np.zeros((k, N_KP), np.uint8))
            cms = (time.perf_counter() - t0) * 1000
            same = (np.array_equal(c["pose"].view(np.uint32), r.pose[:k].cpu().numpy().view(np.uint32)) and np.array_equal(c["outlier"], r.outlier[:k].cpu().numpy())
                    and np.array_equal(c["n_inliers"], n_in[:k]) and np.array_equal(c["status"], r.status[:k].cpu().numpy())
                    and np.array_equal(c["frustum"].view(np.uint32), r.frustum[:k].cpu().numpy().view(np.uint32)))
            assert same, "the C++ loop and the GPU write different bits"
            row["bits_equal_to_cpu_loop"] = True
            row["cpu_loop_frames"] = k
            row["ms_cpu_loop_single_thread"] = round(cms * rows / k, 3)
            row["cpu_over_gpu"] = round(cms * rows / k / ms["median"], 1)
            row["gpu_not_slower_than_cpu_loop"] = ms["median"] <= cms * rows / k
        res[name] = row
        print(name, json.dumps(row), flush=True)
    if not a.no_json and not a.shape:
        json.dump(res, open(OUT, "w"), indent=1)
    if "frames" in res and not res["frames"].get("gpu_not_slower_than_cpu_loop", True):
        sys.exit("the device call is slower than the C++ loop")


if __name__ == "__main__":
    main()

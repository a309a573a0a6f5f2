"""tools/bench_tri.py -- time of plf_triangulate_points (one launch, one workgroup per job), device in and out, on three shapes:
  jobs    8192 jobs x 1000 key points per keyframe with about 150 pairs each, split over the three branches and the rejects as the scenes of
          tests/trigen.py give them (a sideways baseline, one just above mb, a forward motion; 64 distinct keyframe pairs, each job its own match row)
  single  the first of those jobs alone: what a one-neighbour caller pays
  big     64 jobs x 4000 key points with about 600 pairs
Warm-up, then the median of `--calls` calls timed with device events on one stream.  Beside each the single-thread loop a caller runs today
(tools/tri_cpu.cpp, g++ -O2 -ffp-contract=off, on the host this tool runs on) over the same jobs, and whether the two write the same bits.
CONDITION, stated and checked: the device call is no slower than the C++ loop at the 8192-job shape (there is no earlier device form to compare
with).  Writes profiles/tri.json.

The per-kernel time comes from a kernel trace taken in a run of its own:
    rocprofv3 --kernel-trace --stats -d DIR --output-format csv -- python tools/bench_tri.py --calls 3 --no-json --no-cpu --shape SHAPE
    python tools/bench_tri.py --kernel-stats DIR --shape SHAPE
A measurement needs the GPU: without one this tool fails, it does not fall back."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import benchlib  # noqa: E402
OUT = os.path.join(ROOT, "profiles", "tri.json")
SHAPES = {"jobs": (8192, 1000, 150, 64), "single": (1, 1000, 150, 1), "big": (64, 4000, 600, 64)}     # jobs, key points, pairs, distinct keyframe pairs
MOTIONS = ((-0.25, 0.02, 0.03), (-0.08, 0.01, 0.02), (0.01, -0.01, -1.0))


def make_scene(J, n, pairs, distinct):
    """J jobs over `distinct` keyframe pairs of tests/trigen.pair_scene; job j reads pair j % distinct"""
    import numpy as np
    import trigen as G
    prs = [G.pair_scene(9000 + k, n, n, pairs, MOTIONS[k % 3], pass_through=20 if k % 3 == 2 else 0) for k in range(distinct)]
    sc = G.scene_of(prs, S=n)
    which = np.arange(J) % distinct
    return dict(slots=sc["slots"], job_kf1=sc["job_kf1"][which].copy(), job_kf2=sc["job_kf2"][which].copy(), match12=np.ascontiguousarray(sc["match12"][which]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-json", action="store_true")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--shape", default=None, choices=tuple(SHAPES), help="this shape only (for a kernel trace)")
    ap.add_argument("--kernel-stats", default=None, help="directory of a rocprofv3 --kernel-trace --stats run of this tool: merge the per-kernel time")
    a = ap.parse_args()
    if a.kernel_stats:
        print(json.dumps(benchlib.merge_kernel_stats(OUT, a.kernel_stats, "k_tri_", lambda res, split: res[a.shape or "jobs"].update(per_kernel_ms_traced=split))[1]))
        return
    import numpy as np
    import torch
    import trigen as G
    from rgbd_pl_slam_amd import triangulate_points
    from rgbd_pl_slam_amd.triangulate import TriangulateResult
    assert torch.cuda.is_available(), "bench_tri.py needs the GPU"
    cuda = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()   # noqa: E731
    st = torch.cuda.Stream()
    res = {"what": "plf_triangulate_points, device in and out, one launch per call; median of calls, device events", "calls": a.calls, "warmup": a.warmup,
           "cpu_loop": "tools/tri_cpu.cpp, one thread, g++ -O2 -ffp-contract=off, on the host of this run, over the same jobs",
           "condition": "the device call is no slower than the C++ loop at the 8192-job shape"}
    for name, (J, n, pairs, distinct) in SHAPES.items():
        if a.shape and a.shape != name:
            continue
        sc = make_scene(J, n, pairs, distinct)
        ns = 256 if pairs <= 256 else 1024
        kfs = G.dev_keyframes(sc)
        k1, k2, m12, sf, sg = cuda(sc["job_kf1"]), cuda(sc["job_kf2"]), cuda(sc["match12"]), cuda(G.SF), cuda(G.SIGMA2)
        out = TriangulateResult(new_i1=torch.full((J, ns), -1, dtype=torch.int32, device="cuda"), new_i2=torch.full((J, ns), -1, dtype=torch.int32, device="cuda"),
                                new_pos=torch.zeros((J, ns, 3), dtype=torch.float32, device="cuda"), n_new=torch.zeros(J, dtype=torch.int32, device="cuda"),
                                status=torch.zeros(J, dtype=torch.int32, device="cuda"), reason=torch.zeros((J, n), dtype=torch.uint8, device="cuda"))
        run = lambda: triangulate_points(kfs, k1, k2, m12, G.CAM, G.MB, sf, sg, scale_factor=G.SCALE_FACTOR, new_stride=ns, out=out, stream=st.cuda_stream)   # noqa: E731
        ms, r = benchlib.median_ms(run, st, a.warmup, a.calls)
        torch.cuda.synchronize()
        got = {k: getattr(r, k).cpu().numpy() for k in ("new_i1", "new_i2", "new_pos", "n_new", "status", "reason")}
        codes = np.bincount((got["reason"] & 15).reshape(-1), minlength=16)
        branches = np.bincount((got["reason"] >> 4).reshape(-1), minlength=4)
        npairs = int(codes[2:12].sum())
        row = {"jobs": J, "key_points": n, "pairs_per_job": round(npairs / J, 1), "ms": ms, "us_per_job": round(ms["median"] * 1000 / J, 3),
               "created_per_job": round(float(got["n_new"].mean()), 1), "share_svd": round(float(branches[1]) / max(npairs, 1), 3),
               "share_unproject": round(float(branches[2] + branches[3]) / max(npairs, 1), 3), "share_no_branch": round(float(codes[3]) / max(npairs, 1), 3)}
        if not a.no_cpu:
            G.cpu_loop()                                              # (built before the clock starts)
            sec = []
            c = G.cpu_call(sc, new_stride=ns, seconds=sec)
            same = all(np.array_equal(c[k], got[k]) for k in ("new_i1", "new_i2", "n_new", "status", "reason")) and G.same_bits(c["new_pos"], got["new_pos"])
            assert same, "the C++ loop and the GPU write different results"
            row["equal_to_cpu_loop"] = True
            row["ms_cpu_loop_single_thread"] = round(sec[0] * 1000, 3)
            row["cpu_over_gpu"] = round(sec[0] * 1000 / ms["median"], 2)
            row["gpu_not_slower_than_cpu_loop"] = ms["median"] <= sec[0] * 1000
        res[name] = row
        print(name, json.dumps(row), flush=True)
    if not a.no_json and not a.shape:
        json.dump(res, open(OUT, "w"), indent=1)
    if "jobs" in res and not res["jobs"].get("gpu_not_slower_than_cpu_loop", True):
        sys.exit("CONDITION NOT MET: the device call is slower than the C++ loop at the 8192-job shape")
    if "jobs" in res and "gpu_not_slower_than_cpu_loop" in res["jobs"]:
        print("condition met: the device call is no slower than the C++ loop at the 8192-job shape")


if __name__ == "__main__":
    main()

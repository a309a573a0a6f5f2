"""tools/bench_sim3opt.py -- time of plf_sim3_optimize (one launch), device in and out, on three shapes; every job has 100 correspondences of which
30 % are gross outliers of 30 px, and a start transform 2 degrees and 5 cm off the truth (the scenes of tests/sim3optgen.py; 64 distinct keyframe pairs,
alternately free and fixed scale):
  batch   4096 jobs
  round   64 jobs
  single  one job
Warm-up, then the median of `--calls` calls timed with device events on one stream; each timed call starts from the caller's matches (the copy that
sets match12 back is inside the timed region).  Beside each the single-thread loop a caller runs today (tools/sim3opt_cpu.cpp, g++ -O2
-ffp-contract=off, on the host this tool runs on) over the same jobs; the bits of the two are checked to be equal.
CONDITION, stated and checked: the device call takes no longer than the host loop at `batch`.  `single` is reported beside the host loop whichever way
it falls.  Writes profiles/sim3opt.json.

The per-kernel time comes from a kernel trace taken in a run of its own:
    rocprofv3 --kernel-trace --stats -d DIR --output-format csv -- python tools/bench_sim3opt.py --calls 3 --no-json --no-cpu --shape SHAPE
    python tools/bench_sim3opt.py --kernel-stats DIR --shape SHAPE
A measurement needs the GPU: without one this tool fails, it does not fall back."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import benchlib  # noqa: E402
OUT = os.path.join(ROOT, "profiles", "sim3opt.json")
SHAPES = {"batch": 4096, "round": 64, "single": 1}
DISTINCT, PAIRS, OUTLIERS, OUT_PX, OFF_DEG, OFF_T = 64, 100, 0.3, 30.0, 2.0, 0.05


def make_scene(J):
    import numpy as np
    import sim3optgen as G
    d = min(J, DISTINCT)
    sc = G.make_scene(7100, [dict(n1=120, pairs=PAIRS, outliers=OUTLIERS, out_px=OUT_PX, off_deg=OFF_DEG, off_t=OFF_T, fix_scale=bool(k & 1),
                                  scale=1.0 + 0.05 * (k % 5)) for k in range(d)])
    which = np.arange(J) % d
    sc.update(job_kf1=sc["job_kf1"][which].copy(), job_kf2=sc["job_kf2"][which].copy(), match12=np.ascontiguousarray(sc["match12"][which]),
              fix_scale=sc["fix_scale"][which].copy(), sim3_in=np.ascontiguousarray(sc["sim3_in"][which]))
    return sc


def cpu_lib():
    so = os.path.join(tempfile.mkdtemp(prefix="sim3opt_cpu_"), "sim3opt_cpu.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", "-Wno-unknown-pragmas",
                           os.path.join(ROOT, "tools", "sim3opt_cpu.cpp"), "-o", so])
    return C.CDLL(so)


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
        print(json.dumps(benchlib.merge_kernel_stats(OUT, a.kernel_stats, "k_sim3_optimize", lambda res, split: res[a.shape or "batch"].update(per_kernel_ms_traced=split))[1]))
        return
    import numpy as np
    import torch
    import sim3optgen as G
    from rgbd_pl_slam_amd import sim3 as S3, sim3opt as SO
    assert torch.cuda.is_available(), "bench_sim3opt.py needs the GPU"
    cuda = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()   # noqa: E731
    st = torch.cuda.Stream()
    res = {"what": "plf_sim3_optimize, device in and out, one launch per call; median of calls, device events; each call starts from the caller's match12",
           "calls": a.calls, "warmup": a.warmup, "correspondences_per_job": PAIRS, "outlier_share": OUTLIERS, "outlier_px": OUT_PX, "start_off_deg": OFF_DEG,
           "start_off_t": OFF_T, "cpu_loop": "tools/sim3opt_cpu.cpp, one thread, g++ -O2 -ffp-contract=off, on the host of this run, over the same jobs",
           "condition": "the device call takes no longer than the host loop at `batch`"}
    lib = None if a.no_cpu else cpu_lib()
    for name, J in SHAPES.items():
        if a.shape and a.shape != name:
            continue
        sc = make_scene(J)
        keys = [cuda(np.ascontiguousarray(k).view(np.uint8).reshape(-1)) for k in sc["kf_keys"]]
        kfs = S3.Sim3KeyFrames(keys, [cuda(m) for m in sc["kf_mappoints"]], cuda(sc["kf_pose"]))
        cam = tuple(float(x) for x in sc["cam"][[0, 1, 2, 3, 9]])
        with torch.cuda.stream(st):
            args = [cuda(sc[k]) for k in ("job_kf1", "job_kf2")]
            match0 = cuda(sc["match12"])
            match = match0.clone()
            rest = [cuda(sc[k]) for k in ("sim3_in", "fix_scale", "world_pos", "point_bad", "inv_level_sigma2")]
            out = SO.sim3_optimize(kfs, args[0], args[1], match, *rest, cam, th2=sc["th2"], stream=st.cuda_stream)
        st.synchronize()

        def run():
            with torch.cuda.stream(st):
                match.copy_(match0)
            return SO.sim3_optimize(kfs, args[0], args[1], match, *rest, cam, th2=sc["th2"], out=out, stream=st.cuda_stream)

        ms, r = benchlib.median_ms(run, st, a.warmup, a.calls)
        torch.cuda.synchronize()
        got = dict(sim3=r.sim3.cpu().numpy(), match12=match.cpu().numpy(), scw=r.scw.cpu().numpy(), n_inliers=r.n_inliers.cpu().numpy(), status=r.status.cpu().numpy())
        row = {"jobs": J, "ms": ms, "us_per_job": round(ms["median"] * 1000 / J, 3), "jobs_with_20_inliers": int((got["n_inliers"] >= 20).sum()),
               "mean_inliers": round(float(got["n_inliers"].mean()), 2)}
        if lib is not None:
            G.cpu_run(lib, sc)                                              # (warm)
            t0 = time.perf_counter()
            ref = G.cpu_run(lib, sc)
            t_cpu = time.perf_counter() - t0
            G.compare(ref, got, name)
            row.update(equal_to_cpu_loop=True, ms_cpu_loop=round(t_cpu * 1000, 3), cpu_over_gpu=round(t_cpu * 1000 / ms["median"], 3),
                       jobs_with_ten_more_iterations=int((ref["its"][:, 1] == 10).sum()))
        res[name] = row
        print(name, json.dumps(row), flush=True)
    verdict = None
    if lib is not None and "batch" in res:
        verdict = res["condition_met"] = {"batch_vs_host_loop": bool(res["batch"]["ms"]["median"] <= res["batch"]["ms_cpu_loop"])}
    if not a.no_json and not a.shape:
        json.dump(res, open(OUT, "w"), indent=1)
    if verdict is not None:
        print("condition:", json.dumps(verdict))
        if not all(verdict.values()):
            sys.exit("CONDITION NOT MET (recorded in profiles/sim3opt.json)")


if __name__ == "__main__":
    main()

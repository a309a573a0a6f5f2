"""tools/bench_sim3.py -- time of plf_sim3_iterate (two launches: count, resolve), device in and out, on three shapes, min_inliers 20, 100 pairs per
solver with 40 % gross outliers (the scenes of tests/sim3gen.py; 64 distinct keyframe pairs, each job its own raw random values):
  loop    4096 solvers (512 keyframes x 8 candidates), all 300 iterations in one call
  round   4096 solvers, one iterate(5) round of LoopClosing::ComputeSim3
  single  one solver, 300 iterations
Warm-up, then the median of `--calls` calls timed with device events on one stream; each timed call starts from the state plf_sim3_pairs leaves (three
small fills that set it back are inside the timed region).  Beside each the single-thread loop a caller runs today (tools/sim3_cpu.cpp, g++ -O2
-ffp-contract=off, on the host this tool runs on) over the same jobs in two modes: all iterations -- the same work as the device, and the bits are
checked to be equal -- and stop at each solver's first hit, which is what a caller does today (with 40 % outliers the first hit comes within a few
iterations, so this is the honest comparison for `single`).
CONDITION, stated and checked: the device call is no slower than the all-iterations loop at `loop` and no slower than the stop-at-first-hit loop at
`round`.  Writes profiles/sim3.json.

The per-kernel time comes from a kernel trace taken in a run of its own:
    rocprofv3 --kernel-trace --stats -d DIR --output-format csv -- python tools/bench_sim3.py --calls 3 --no-json --no-cpu --shape SHAPE
    python tools/bench_sim3.py --kernel-stats DIR --shape SHAPE
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
OUT = os.path.join(ROOT, "profiles", "sim3.json")
SHAPES = {"loop": (4096, 300), "round": (4096, 5), "single": (1, 300)}       # solvers, iterations per call
DISTINCT, PAIRS, OUTLIERS, MIN_INLIERS, MAX_ITS = 64, 100, 0.4, 20, 300


def make_scene(J):
    import numpy as np
    import sim3gen as G
    d = min(J, DISTINCT)
    sc = G.make_scene(7000, [dict(n1=120, pairs=PAIRS, outliers=OUTLIERS, fix_scale=bool(k & 1), scale=1.0 + 0.05 * (k % 5)) for k in range(d)],
                      min_inliers=MIN_INLIERS, max_iterations=MAX_ITS, pair_stride=128, max_hits=1)
    which = np.arange(J) % d
    sc.update(job_kf1=sc["job_kf1"][which].copy(), job_kf2=sc["job_kf2"][which].copy(), match12=np.ascontiguousarray(sc["match12"][which]),
              fix_scale=sc["fix_scale"][which].copy(), rand3=G.raw_values(77, (J, MAX_ITS, 3)))
    return sc


def cpu_lib():
    so = os.path.join(tempfile.mkdtemp(prefix="sim3_cpu_"), "sim3_cpu.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", "-Wno-unknown-pragmas", os.path.join(ROOT, "tools", "sim3_cpu.cpp"), "-o", so])
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
        print(json.dumps(benchlib.merge_kernel_stats(OUT, a.kernel_stats, "k_sim3_", lambda res, split: res[a.shape or "loop"].update(per_kernel_ms_traced=split))[1]))
        return
    import numpy as np
    import torch
    import sim3gen as G
    from rgbd_pl_slam_amd import sim3 as S3
    assert torch.cuda.is_available(), "bench_sim3.py needs the GPU"
    cuda = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()   # noqa: E731
    st = torch.cuda.Stream()
    res = {"what": "plf_sim3_iterate, device in and out, two launches per call; median of calls, device events; each call starts from the state plf_sim3_pairs leaves",
           "calls": a.calls, "warmup": a.warmup, "pairs_per_solver": PAIRS, "outlier_share": OUTLIERS, "min_inliers": MIN_INLIERS,
           "cpu_loop": "tools/sim3_cpu.cpp, one thread, g++ -O2 -ffp-contract=off, on the host of this run, over the same jobs",
           "condition": "the device call is no slower than the all-iterations C++ loop at `loop` and no slower than the stop-at-first-hit C++ loop at `round`"}
    lib = None if a.no_cpu else cpu_lib()
    for name, (J, its) in SHAPES.items():
        if a.shape and a.shape != name:
            continue
        sc = make_scene(J)
        keys = [cuda(np.ascontiguousarray(k).view(np.uint8).reshape(-1)) for k in sc["kf_keys"]]
        kfs = S3.Sim3KeyFrames(keys, [cuda(m) for m in sc["kf_mappoints"]], cuda(sc["kf_pose"]))
        cam = tuple(float(x) for x in sc["cam"][[0, 1, 2, 3, 9]])
        with torch.cuda.stream(st):
            pr = S3.sim3_pairs(kfs, cuda(sc["job_kf1"]), cuda(sc["job_kf2"]), cuda(sc["match12"]), cuda(sc["world_pos"]), cuda(sc["point_bad"]),
                               cuda(sc["level_sigma2"]), cam, pair_stride=sc["pair_stride"], min_inliers=MIN_INLIERS, max_iterations=MAX_ITS, stream=st.cuda_stream)
            rand3, fix = cuda(sc["rand3"]), cuda(sc["fix_scale"])
            out = S3.sim3_iterate(pr, rand3, 0, fix, cam, min_inliers=MIN_INLIERS, max_hits=1, stream=st.cuda_stream)

        def run():
            with torch.cuda.stream(st):
                pr.iterations_done.zero_(); pr.best_inliers.zero_(); pr.best_iter.fill_(-1)
            return S3.sim3_iterate(pr, rand3, its, fix, cam, min_inliers=MIN_INLIERS, max_hits=1, out=out, stream=st.cuda_stream)

        ms, r = benchlib.median_ms(run, st, a.warmup, a.calls)
        torch.cuda.synchronize()
        got_pairs = {k: getattr(pr, k).cpu().numpy() for k in G.PAIR_KEYS}
        got_state = {k: getattr(pr, k).cpu().numpy() for k in G.STATE_KEYS}
        got = (r.count.cpu().numpy(), {k: getattr(r, k).cpu().numpy() for k in G.HIT_KEYS})
        row = {"solvers": J, "iterations_per_call": its, "ms": ms, "us_per_solver": round(ms["median"] * 1000 / J, 3),
               "solvers_with_a_hit": int((got[1]["n_hits"] > 0).sum()), "mean_first_hit_iteration": round(float(got[1]["hit_iter"][got[1]["n_hits"] > 0].mean()), 2)}
        if lib is not None:
            t0 = time.perf_counter()
            cp, cs, (crun,) = G.cpu_run(lib, sc, [its])
            t_all = time.perf_counter() - t0
            G.compare((cp, cs, [crun]), (got_pairs, got_state, [got]), name)
            t0 = time.perf_counter()
            fp, fs, (frun,) = G.cpu_run(lib, sc, [its], first_hit=True)
            t_first = time.perf_counter() - t0
            hit = frun[1]["n_hits"] > 0
            assert np.array_equal(hit, got[1]["n_hits"] > 0) and G.same_bits(frun[1]["hit_sim3"][hit], got[1]["hit_sim3"][hit]), "first hits differ"
            # both host times include the constructor loop (sim3_cpu_pairs); it is timed alone and taken off
            t0 = time.perf_counter()
            G.cpu_run(lib, sc, [0])
            t_pairs = time.perf_counter() - t0
            row.update(equal_to_cpu_loop=True, ms_cpu_all_iterations=round((t_all - t_pairs) * 1000, 3), ms_cpu_stop_at_first_hit=round((t_first - t_pairs) * 1000, 3),
                       cpu_all_over_gpu=round((t_all - t_pairs) * 1000 / ms["median"], 2), cpu_first_hit_over_gpu=round((t_first - t_pairs) * 1000 / ms["median"], 3))
        res[name] = row
        print(name, json.dumps(row), flush=True)
    verdict = None
    if lib is not None and "loop" in res and "round" in res:
        ok_loop = res["loop"]["ms"]["median"] <= res["loop"]["ms_cpu_all_iterations"]
        ok_round = res["round"]["ms"]["median"] <= res["round"]["ms_cpu_stop_at_first_hit"]
        verdict = res["condition_met"] = {"loop_vs_all_iterations": bool(ok_loop), "round_vs_stop_at_first_hit": bool(ok_round)}
    if not a.no_json and not a.shape:
        json.dump(res, open(OUT, "w"), indent=1)
    if verdict is not None:
        print("condition:", json.dumps(verdict))
        if not all(verdict.values()):
            sys.exit("CONDITION NOT MET (recorded in profiles/sim3.json)")


if __name__ == "__main__":
    main()

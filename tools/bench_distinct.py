"""tools/bench_distinct.py -- time of the GPU ComputeDistinctiveDescriptors (plf_map_distinctive_descriptors), device in and out, on three shapes:
  local   5,000 points, observation counts long-tailed with mean about 8 (a local map after Fuse)
  global  500,000 points, the same distribution (a whole map)
  worst   1,000 points x 256 observations
and on one shape per size class, so that each schedule is judged on its own:
  small   200,000 points of 2 .. 16 observations      (k_map_small, four points per wave)
  medium  20,000 points of 17 .. 256 observations     (k_map_wave, one wave per point: the schedule the naive run uses too, so a tie is expected)
  large   300 points of 257 .. 1,500 observations     (k_map_block, one workgroup per point)
Warm-up, then the median of `--calls` calls timed with device events on one stream.  Every shape is run twice on the same box: with the three size-class
schedules, and with PLF_MAP_NAIVE=1, one wave per point whatever its count (the ballot kernel k_map_wave up to 256 observations, one wave of k_map_block
beyond) -- the A/B the small and the large schedule have to win.  Beside them, in the same file, the time of the single-thread C++ loop a caller runs
today (tools/distinct_cpu.cpp, built here with -O3 -march=native, on the host this tool runs on).  Writes profiles/distinct_descriptors.json.

The per-kernel split comes from a kernel trace taken in a run of its own, of the shipped schedule only:
    rocprofv3 --kernel-trace --stats -d DIR --output-format csv -- python tools/bench_distinct.py --only global --mode auto --calls 3 --no-json --no-cpu
    python tools/bench_distinct.py --kernel-stats DIR --only global
A measurement needs the GPU: without one this tool fails, it does not fall back."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import benchlib  # noqa: E402
OUT = os.path.join(ROOT, "profiles", "distinct_descriptors.json")
SHAPES = ("local", "global", "worst", "small", "medium", "large")


def counts_of(shape, rng):
    import numpy as np
    if shape == "worst":
        return np.full(1000, 256, np.int64)
    if shape == "small":
        return rng.integers(2, 17, 200000).astype(np.int64)
    if shape == "medium":
        return rng.integers(17, 257, 20000).astype(np.int64)
    if shape == "large":
        return rng.integers(257, 1501, 300).astype(np.int64)
    n = 5000 if shape == "local" else 500000
    c = rng.geometric(1 / 6.0, n).astype(np.int64) + 1            # 2 and up, mean 7
    tail = rng.random(n) < 0.004                                   # a few points seen from hundreds of keyframes
    c[tail] = rng.integers(100, 600, int(tail.sum()))
    return c


def cpu_loop_ms(start, desc, reps):
    with tempfile.TemporaryDirectory() as d:
        exe = benchlib.build_cpp("distinct_cpu.cpp", d, "-O3", "-march=native")
        start.tofile(os.path.join(d, "s.i32")); desc.tofile(os.path.join(d, "d.u8"))
        out = subprocess.check_output([exe, os.path.join(d, "s.i32"), os.path.join(d, "d.u8"), str(reps)], text=True).split()
    return float(out[1]), int(out[3])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=SHAPES, default=None)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--mode", choices=("both", "auto", "naive"), default="both", help="auto: the shipped schedules only (for a kernel trace)")
    ap.add_argument("--no-json", action="store_true")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--kernel-stats", default=None, help="directory of a rocprofv3 --kernel-trace --stats run of this tool with --only SHAPE: merge the per-kernel split")
    a = ap.parse_args()
    if a.kernel_stats:
        if not a.only:
            sys.exit("--kernel-stats needs --only SHAPE")
        print(json.dumps(benchlib.merge_kernel_stats(OUT, a.kernel_stats, "k_map_", lambda res, split: res["shapes"][a.only].update(per_kernel_ms_traced=split))[1]))
        return
    import numpy as np
    import torch
    import mapref
    from rgbd_pl_slam_amd import distinctive_descriptors
    assert torch.cuda.is_available(), "bench_distinct.py needs the GPU"
    res = {"what": "plf_map_distinctive_descriptors, packed form, device in and out; median of calls, device events", "calls": a.calls, "warmup": a.warmup,
           "cpu_loop": "tools/distinct_cpu.cpp, one thread, g++ -O3 -march=native, best of 3, on the host of this run", "shapes": {}}
    st = torch.cuda.Stream()
    for shape in ([a.only] if a.only else SHAPES):
        rng = np.random.default_rng(7)
        counts = counts_of(shape, rng)
        start, desc, _ = mapref.make_points(8, counts)
        ds = torch.from_numpy(start).cuda(); dd = torch.from_numpy(desc).cuda()
        md = torch.zeros((len(counts), 32), dtype=torch.uint8, device="cuda")
        row = {"points": int(len(counts)), "observations": int(counts.sum()), "mean_count": round(float(counts.mean()), 2), "max_count": int(counts.max()),
               "pair_distances": int((counts * counts).sum())}
        results = {}
        for mode in (("auto", "naive") if a.mode == "both" else (a.mode,)):
            os.environ["PLF_MAP_NAIVE"] = "1" if mode == "naive" else "0"
            row["ms_" + mode], (bo, bm) = benchlib.median_ms(lambda: distinctive_descriptors(ds, md, obs_desc=dd, stream=st.cuda_stream), st, a.warmup, a.calls)
            results[mode] = (bo.cpu().numpy(), bm.cpu().numpy())
        os.environ["PLF_MAP_NAIVE"] = "0"
        got = results.get("auto") or results["naive"]
        # a spot check that what was timed is the rule: the first 300 points against the restatement
        rbo, rbm = mapref.distinctive_all(start[:301], desc, None)
        assert np.array_equal(got[0][:300], rbo) and np.array_equal(got[1][:300], rbm)
        if a.mode == "both":
            assert np.array_equal(results["auto"][0], results["naive"][0]) and np.array_equal(results["auto"][1], results["naive"][1])
            row["naive_over_auto"] = round(row["ms_naive"]["median"] / row["ms_auto"]["median"], 2)
            row["schedules_beat_one_wave_per_point"] = row["ms_auto"]["median"] < row["ms_naive"]["median"]
        if not a.no_cpu and a.mode == "both":
            cms, chk = cpu_loop_ms(start, desc, 3)
            assert chk == int(results["auto"][0].astype(np.int64).sum() + results["auto"][1].astype(np.int64).sum()), "the C++ loop and the GPU disagree"
            row["ms_cpu_loop_single_thread"] = round(cms, 3)
            row["cpu_over_gpu"] = round(cms / row["ms_auto"]["median"], 1)
        res["shapes"][shape] = row
        print(shape, json.dumps(row), flush=True)
    if not a.no_json and not a.only and a.mode == "both":
        json.dump(res, open(OUT, "w"), indent=1)


if __name__ == "__main__":
    main()

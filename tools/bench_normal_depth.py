"""tools/bench_normal_depth.py -- time of the GPU UpdateNormalAndDepth (plf_map_update_normal_depth), packed level form, device in and out, on two shapes:
  local   5,000 points, observation counts long-tailed with mean about 8 (a local map after Fuse)
  global  500,000 points / about 4.2 M observations / 10,000 keyframes (a whole map)
Warm-up, then the median of `--calls` calls timed with device events on one stream.  Beside them, in the same file, the time of the single-thread C++
loop a caller runs today (tools/normal_depth_cpu.cpp, built here with g++ -O2 -ffp-contract=off, on the host this tool runs on); its arrays and the
device's are compared bit for bit (two NaNs at one position count as equal).  Writes profiles/normal_depth.json.  The condition it states: the
device call does not take longer than the C++ loop at the whole-map shape.

The per-kernel split comes from a kernel trace taken in a run of its own:
    rocprofv3 --kernel-trace --stats -d DIR --output-format csv -- python tools/bench_normal_depth.py --only global --calls 3 --no-json --no-cpu
    python tools/bench_normal_depth.py --kernel-stats DIR --only global
A measurement needs the GPU: without one this tool fails, it does not fall back."""
import argparse
import json
import os
import pathlib
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import benchlib  # noqa: E402
OUT = os.path.join(ROOT, "profiles", "normal_depth.json")
SHAPES = {"local": (5000, 600), "global": (500000, 10000)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=tuple(SHAPES), default=None)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-json", action="store_true")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--kernel-stats", default=None, help="directory of a rocprofv3 --kernel-trace --stats run of this tool with --only SHAPE: merge the per-kernel split")
    a = ap.parse_args()
    if a.kernel_stats:
        if not a.only:
            sys.exit("--kernel-stats needs --only SHAPE")
        print(json.dumps(benchlib.merge_kernel_stats(OUT, a.kernel_stats, "k_mapgeom_", lambda res, split: res["shapes"][a.only].update(per_kernel_ms_traced=split))[1]))
        return
    import numpy as np
    import torch
    import normref as R
    from test_normal_ref import build_cpu_loop, run_cpu_loop
    from rgbd_pl_slam_amd import update_normal_and_depth
    assert torch.cuda.is_available(), "bench_normal_depth.py needs the GPU"
    res = {"what": "plf_map_update_normal_depth, packed level form, device in and out; median of calls, device events", "calls": a.calls, "warmup": a.warmup,
           "cpu_loop": "tools/normal_depth_cpu.cpp, one thread, g++ -O2 -ffp-contract=off, best of 3, on the host of this run", "shapes": {}}
    st = torch.cuda.Stream()
    sf = R.scale_factors()
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    with tempfile.TemporaryDirectory() as tmp:
        tmp = pathlib.Path(tmp)
        exe = None if a.no_cpu else build_cpu_loop(tmp)
        for shape in ([a.only] if a.only else list(SHAPES)):
            n, n_kf = SHAPES[shape]
            counts = R.long_tailed_counts(np.random.default_rng(7), n)
            m = R.make_map(8, counts, n_kf)
            d = {k: dev(m[k]) for k in ("obs_start", "obs_kf", "kf_ow", "ref_kf", "world_pos", "level")}
            dsf = dev(sf)
            fill = torch.full((n, 5), R.SENTINEL - (1 << 32), dtype=torch.int32, device="cuda").view(torch.float32)
            nv, mn, mx = fill[:, :3].contiguous(), fill[:, 3].contiguous(), fill[:, 4].contiguous()
            call = lambda: update_normal_and_depth(d["obs_start"], d["obs_kf"], d["kf_ow"], d["ref_kf"], d["world_pos"], nv, mn, mx, ref_level=d["level"],
                                                   scale_factors=dsf, stream=st.cuda_stream)
            ms_device, used = benchlib.median_ms(call, st, a.warmup, a.calls)
            row = {"points": int(n), "observations": int(counts.sum()), "keyframes": n_kf, "mean_count": round(float(counts.mean()), 2), "max_count": int(counts.max()),
                   "ms_device": ms_device}
            if exe is not None:
                c = run_cpu_loop(exe, tmp, m, sf, reps=3)
                same = (np.array_equal(c[3], used.cpu().numpy()) and R.same_bits(c[0], nv.cpu().numpy()) and R.same_bits(c[1], mn.cpu().numpy())
                        and R.same_bits(c[2], mx.cpu().numpy()))
                assert same, "the C++ loop and the GPU disagree"
                row["ms_cpu_loop_single_thread"] = round(c[4], 3)
                row["cpu_over_gpu"] = round(c[4] / row["ms_device"]["median"], 1)
                row["equal_bits"] = bool(same)
                if shape == "global":
                    row["device_not_slower_than_cpu_loop"] = bool(row["ms_device"]["median"] <= c[4])
            res["shapes"][shape] = row
            print(shape, json.dumps(row), flush=True)
    if not a.no_json and not a.only and not a.no_cpu:
        json.dump(res, open(OUT, "w"), indent=1)


if __name__ == "__main__":
    main()

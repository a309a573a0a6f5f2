"""tools/bench_culling.py -- time of the GPU culling calls (plf_keyframe_culling, plf_map_point_culling), device in and out, on the 10,000-keyframe /
500,000-point / 4.17 M-observation map of tools/bench_covis.py:
  cull30, cull100   one sequential KeyFrameCulling of a new keyframe with 30 and 100 candidates (its neighbours along the trajectory)
  snapshot          the snapshot mode over all 10,000 keyframes
  points            MapPointCulling for 5,000 recent points
Warm-up, then the median of `--calls` calls timed with device events on one stream.  Beside them the time of the single-thread loop a caller runs
today (tools/culling_cpu.cpp, built here with -O3 -march=native, on the host this tool runs on) and whether the decisions are equal.  The condition
reported: the device call takes no longer than that loop at `snapshot` and at `cull100`.  --levels indirect reads the octaves through a kf_keys table
of per-keyframe key buffers instead of the packed arrays.  Writes profiles/culling.json.

The per-kernel split comes from a kernel trace taken in a run of its own:
    rocprofv3 --kernel-trace --stats -d DIR --output-format csv -- python tools/bench_culling.py --calls 3 --no-json --no-cpu
    python tools/bench_culling.py --kernel-stats DIR
A measurement needs the GPU: without one this tool fails, it does not fall back."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import benchlib  # noqa: E402
import bench_covis  # noqa: E402
OUT = os.path.join(ROOT, "profiles", "culling.json")
N_KF, N_POINTS, TH_DEPTH = bench_covis.N_KF, bench_covis.N_POINTS, 3.0


def make_map(rng):
    """bench_covis.make_map plus what culling reads: the feature index of every observation, octaves, depths, weights"""
    import numpy as np
    obs_start, obs_kf, row_start, row_point = bench_covis.make_map(rng)
    order = np.argsort(obs_kf, kind="stable")
    entry = np.empty(len(obs_kf), np.int64); entry[order] = np.arange(len(obs_kf))      # the row entry that is this observation
    obs_idx = (entry - row_start[obs_kf]).astype(np.int32)
    row_level = np.minimum(rng.geometric(0.45, len(row_point)) - 1, 7).astype(np.int32)   # most keys on the fine octaves, as ORB gives them
    obs_level = row_level[entry]
    row_depth = rng.uniform(0.3, 3.6, len(row_point)).astype(np.float32)                 # some beyond mThDepth
    obs_w = (1 + (row_depth[entry] < 3.3)).astype(np.uint8)                              # RGB-D: most observations weigh 2
    return dict(obs_start=obs_start, obs_kf=obs_kf, obs_idx=obs_idx, obs_level=obs_level, obs_w=obs_w, row_start=row_start, row_point=row_point,
                row_level=row_level, row_depth=row_depth, row_kf=np.arange(N_KF, dtype=np.int32), point_bad=np.zeros(N_POINTS, np.uint8))


def cpu_loop(m, cand, sequential, reps):
    import numpy as np
    ext = {"int32": "i32", "float32": "f32", "uint8": "u8"}
    with tempfile.TemporaryDirectory() as d:
        exe = benchlib.build_cpp("culling_cpu.cpp", d, "-O3", "-march=native")
        for k in ("row_start", "row_point", "row_kf", "row_level", "row_depth", "obs_start", "obs_kf", "obs_level", "obs_w", "point_bad"):
            m[k].tofile(os.path.join(d, "%s.%s" % (k, ext[str(m[k].dtype)])))
        cand.astype(np.int32).tofile(os.path.join(d, "cand_row.i32")); np.zeros(len(cand), np.uint8).tofile(os.path.join(d, "cand_flags.u8"))
        th_bits = int(np.array(TH_DEPTH, np.float32).view(np.uint32))
        out = subprocess.check_output([exe, d, str(N_KF), str(th_bits), "0", "3", "0.9", str(int(sequential)), str(reps)], text=True).split()
        o = np.fromfile(os.path.join(d, "out.i32"), np.int32)
    return float(out[1]), o[:3 * len(cand)].reshape(3, len(cand))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--levels", choices=("packed", "indirect"), default="packed")
    ap.add_argument("--no-json", action="store_true")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--cpu-repeats", type=int, default=3)
    ap.add_argument("--kernel-stats", default=None, help="directory of a rocprofv3 --kernel-trace --stats run of this tool: merge the per-kernel split")
    a = ap.parse_args()
    if a.kernel_stats:
        print(json.dumps(benchlib.merge_kernel_stats(OUT, a.kernel_stats, "k_cull_", lambda res, split: res.update(per_kernel_ms_traced_all_shapes=split))[1]))
        return
    import numpy as np
    import torch
    from rgbd_pl_slam_amd import CullMap, keyframe_culling, map_point_culling, kf_keys_table
    from rgbd_pl_slam_amd import _lib as L
    assert torch.cuda.is_available(), "bench_culling.py needs the GPU"
    rng = np.random.default_rng(7)
    m = make_map(rng)
    t = {k: torch.from_numpy(v).cuda() for k, v in m.items()}
    kw = dict(obs_w=t["obs_w"], point_bad=t["point_bad"], row_depth=t["row_depth"], th_depth=TH_DEPTH)
    if a.levels == "indirect":
        keys = np.zeros(len(m["row_point"]), L.KP_DTYPE); keys["octave"] = m["row_level"]
        pool = torch.from_numpy(np.frombuffer(keys.tobytes(), np.uint8).copy()).cuda()          # every keyframe's keys_un, back to back
        kw.update(kf_keys=kf_keys_table([pool.data_ptr() + 28 * int(s) for s in m["row_start"][:-1]]), obs_idx=t["obs_idx"])
    else:
        kw.update(row_level=t["row_level"], obs_level=t["obs_level"])
    cmap = CullMap(t["row_start"], t["row_point"], t["row_kf"], t["obs_start"], t["obs_kf"], N_KF, **kw)
    st = torch.cuda.Stream()
    cur = N_KF // 2
    near = lambda n: np.array([cur + (k // 2 + 1) * (1 if k % 2 == 0 else -1) for k in range(n)], np.int32)   # noqa: E731
    shapes = {"cull30": (near(30), True), "cull100": (near(100), True), "snapshot": (np.arange(N_KF, dtype=np.int32), False)}
    res = {"what": "plf_keyframe_culling / plf_map_point_culling, device in and out; median of calls, device events", "calls": a.calls, "warmup": a.warmup,
           "levels": a.levels, "cpu_loop": "tools/culling_cpu.cpp, one thread, g++ -O3 -march=native, best of %d, on the host of this run" % a.cpu_repeats,
           "map": {"keyframes": N_KF, "points": N_POINTS, "observations": int(m["obs_start"][-1])}, "shapes": {}}
    for name, (cand, sequential) in shapes.items():
        dc = torch.from_numpy(cand).cuda()
        box = [None]

        def run():
            with torch.cuda.stream(st):
                if box[0] is not None:
                    box[0].kf_erased.zero_(); box[0].point_went_bad.zero_()
                box[0] = keyframe_culling(cmap, dc, None, sequential, out=box[0], stream=st.cuda_stream)
            return box[0]
        ms_gpu, out = benchlib.median_ms(run, st, a.warmup, a.calls)
        status = out.status.cpu().tolist()
        row = {"candidates": len(cand), "sequential": sequential, "ms_gpu": ms_gpu, "status": status, "erased": int((out.decision == 1).sum())}
        if not a.no_cpu:
            cms, ref = cpu_loop(m, cand, sequential, a.cpu_repeats)
            d = status[0]
            got = np.stack([out.n_mps.cpu().numpy(), out.n_redundant.cpu().numpy(), out.decision.cpu().numpy()])
            assert np.array_equal(got[:, :d], ref[:, :d]), "the C++ loop and the GPU disagree"
            row.update(ms_cpu_loop_single_thread=round(cms, 3), cpu_over_gpu=round(cms / ms_gpu["median"], 1), gpu_not_slower_than_cpu_loop=ms_gpu["median"] <= cms)
        res["shapes"][name] = row
        print(name, json.dumps(row), flush=True)
    n = 5000
    found, visible = rng.integers(0, 40, n).astype(np.int32), rng.integers(1, 60, n).astype(np.int32)
    first = rng.integers(cur - 4, cur + 1, n).astype(np.int64)
    recent = rng.integers(0, N_POINTS, n)
    sums = np.add.reduceat(m["obs_w"].astype(np.int64), m["obs_start"][:-1].astype(np.int64))[recent].astype(np.int32)
    args = [torch.from_numpy(x).cuda() for x in (found, visible, first, sums)]
    dec = torch.empty(n, dtype=torch.int32, device="cuda")
    ms_gpu, out = benchlib.median_ms(lambda: map_point_culling(args[0], args[1], args[2], cur, 3, point_nobs=args[3], decision=dec, stream=st.cuda_stream), st, a.warmup, a.calls)
    res["shapes"]["points"] = {"points": n, "ms_gpu": ms_gpu, "decisions": np.bincount(out.cpu().numpy(), minlength=3).tolist()}
    print("points", json.dumps(res["shapes"]["points"]), flush=True)
    if not a.no_cpu:
        res["condition_gpu_not_slower_at_snapshot_and_cull100"] = bool(res["shapes"]["snapshot"]["gpu_not_slower_than_cpu_loop"] and
                                                                       res["shapes"]["cull100"]["gpu_not_slower_than_cpu_loop"])
    if not a.no_json:
        json.dump(res, open(OUT, "w"), indent=1)


if __name__ == "__main__":
    main()

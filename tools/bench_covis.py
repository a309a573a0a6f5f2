"""tools/bench_covis.py -- time of the GPU covisibility count (plf_covis_count), device in and out, on two shapes:
  graph   a whole-graph rebuild: UpdateConnections for all 10,000 keyframes of the map of tools/bench_distinct.py's `global` shape (500,000 points,
          about 4.2 M observations, the same long-tailed counts); every point's observers lie in a window of keyframes around a centre, as a
          trajectory leaves them, so that neighbours share dozens of points
  votes   the head of UpdateLocalKeyFrames for 8192 frames of 300 matched points each, on the same map
Warm-up, then the median of `--calls` calls timed with device events on one stream.  Beside them, in the same file, the time of the single-thread
std::map loop a caller runs today (tools/covis_cpu.cpp, built here with -O3 -march=native, on the host this tool runs on), and whether the two agree
(a checksum over counts, maxima and list fronts).  Writes profiles/covis.json.

The per-kernel split comes from a kernel trace taken in a run of its own:
    rocprofv3 --kernel-trace --stats -d DIR --output-format csv -- python tools/bench_covis.py --calls 3 --no-json --no-cpu
    python tools/bench_covis.py --kernel-stats DIR
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
OUT = os.path.join(ROOT, "profiles", "covis.json")
N_KF, N_POINTS, N_FRAMES, FRAME_POINTS = 10000, 500000, 8192, 300


def make_map(rng):
    """observation CSR by point and its transpose, the keyframes' mvpMapPoints"""
    import numpy as np
    from bench_distinct import counts_of
    counts = np.minimum(counts_of("global", rng), N_KF // 4)
    start = np.zeros(N_POINTS + 1, np.int64); start[1:] = np.cumsum(counts)
    obs_kf = np.empty(int(start[-1]), np.int32)
    centre = rng.integers(0, N_KF, N_POINTS)
    for c in np.unique(counts):                                     # all points of one count at once: c distinct offsets out of a window of 3c
        idx = np.nonzero(counts == c)[0]
        window = max(3 * int(c), 24)
        off = np.argsort(rng.random((len(idx), window)), axis=1)[:, :c] - window // 2
        kf = (centre[idx, None] + off) % N_KF
        obs_kf[(start[idx, None] + np.arange(c)[None, :]).ravel()] = kf.ravel()
    order = np.argsort(obs_kf, kind="stable")                       # transpose: the points of every keyframe
    point_of = np.repeat(np.arange(N_POINTS, dtype=np.int32), counts)
    row_point = point_of[order]
    row_start = np.zeros(N_KF + 1, np.int64); row_start[1:] = np.cumsum(np.bincount(obs_kf, minlength=N_KF))
    return start.astype(np.int32), obs_kf, row_start.astype(np.int32), row_point


def cpu_loop_ms(arrays, mode, th, reps):
    with tempfile.TemporaryDirectory() as d:
        exe = benchlib.build_cpp("covis_cpu.cpp", d, "-O3", "-march=native")
        paths = []
        for i, a in enumerate(arrays):
            paths.append(os.path.join(d, "a%d.i32" % i)); a.tofile(paths[-1])
        out = subprocess.check_output([exe, *paths, str(mode), str(th), str(reps)], text=True).split()
    return float(out[1]), int(out[3])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-json", action="store_true")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--cpu-repeats", type=int, default=1, help="the C++ loop takes about a minute per pass over the graph shape")
    ap.add_argument("--kernel-stats", default=None, help="directory of a rocprofv3 --kernel-trace --stats run of this tool: merge the per-kernel split")
    a = ap.parse_args()
    if a.kernel_stats:
        print(json.dumps(benchlib.merge_kernel_stats(OUT, a.kernel_stats, "k_covis_", lambda res, split: res.update(per_kernel_ms_traced_both_shapes=split))[1]))
        return
    import numpy as np
    import torch
    from rgbd_pl_slam_amd import update_connections, local_keyframe_votes
    assert torch.cuda.is_available(), "bench_covis.py needs the GPU"
    rng = np.random.default_rng(7)
    obs_start, obs_kf, row_start, row_point = make_map(rng)
    frame_point = rng.integers(0, N_POINTS, (N_FRAMES, FRAME_POINTS)).astype(np.int32)
    frame_point[rng.random(frame_point.shape) < 0.1] = -1           # unmatched features
    frame_start = (np.arange(N_FRAMES + 1, dtype=np.int64) * FRAME_POINTS).astype(np.int32)
    row_self = np.arange(N_KF, dtype=np.int32)
    dev = {k: torch.from_numpy(v).cuda() for k, v in (("os", obs_start), ("ok", obs_kf), ("rs", row_start), ("rp", row_point), ("self", row_self),
                                                      ("fs", frame_start), ("fp", frame_point.reshape(-1)))}
    st = torch.cuda.Stream()
    res = {"what": "plf_covis_count, device in and out; median of calls, device events", "calls": a.calls, "warmup": a.warmup,
           "cpu_loop": "tools/covis_cpu.cpp, one thread, std::map per row, g++ -O3 -march=native, best of %d, on the host of this run" % a.cpu_repeats,
           "map": {"keyframes": N_KF, "points": N_POINTS, "observations": int(obs_start[-1])}, "shapes": {}}
    sq = np.diff(obs_start).astype(np.int64)
    shapes = {
        "graph": dict(stride=256, rows=N_KF, increments=int((sq * sq).sum()),
                      run=lambda out: update_connections(dev["rs"], dev["rp"], dev["self"], dev["os"], dev["ok"], N_KF, 256, 15, out=out, stream=st.cuda_stream),
                      cpu=((row_start, row_point, row_self, obs_start, obs_kf), 0, 15)),
        "votes": dict(stride=256, rows=N_FRAMES, increments=int(sq[frame_point[frame_point >= 0]].sum()),
                      run=lambda out: local_keyframe_votes(dev["fs"], dev["fp"], dev["os"], dev["ok"], N_KF, 256, out=out, stream=st.cuda_stream),
                      cpu=((frame_start, frame_point.reshape(-1), row_self, obs_start, obs_kf), 1, 1)),
    }
    for name, s in shapes.items():
        box = [None]                                                # the output arrays of the first call serve the later ones

        def run():
            box[0] = s["run"](box[0])
            return box[0]
        ms_gpu, out = benchlib.median_ms(run, st, a.warmup, a.calls)
        n_conn, max_kf, max_w = out.n_conn.cpu().numpy().astype(np.int64), out.max_kf.cpu().numpy().astype(np.int64), out.max_w.cpu().numpy().astype(np.int64)
        live = n_conn > 0
        check = int(n_conn.sum() + (max_kf[live] + 1).sum() + max_w[live].sum())
        row = {"rows": s["rows"], "increments": s["increments"], "stride": s["stride"], "max_n_conn": int(n_conn.max()),
               "ms_gpu": ms_gpu}
        if name == "graph":
            n_ord = out.n_ord.cpu().numpy().astype(np.int64)
            check += int(n_ord.sum() + (out.ord_kf[:, 0].cpu().numpy().astype(np.int64)[live] + 1).sum())
            row["max_n_ord"] = int(n_ord.max())
        if not a.no_cpu:
            cms, chk = cpu_loop_ms(*s["cpu"], a.cpu_repeats)
            assert chk == check, ("the C++ loop and the GPU disagree", chk, check)
            row["ms_cpu_loop_single_thread"] = round(cms, 3)
            row["cpu_over_gpu"] = round(cms / row["ms_gpu"]["median"], 1)
            row["gpu_not_slower_than_cpu_loop"] = row["ms_gpu"]["median"] <= cms
        res["shapes"][name] = row
        print(name, json.dumps(row), flush=True)
    if not a.no_json:
        json.dump(res, open(OUT, "w"), indent=1)


if __name__ == "__main__":
    main()

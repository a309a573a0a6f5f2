"""tools/bench_track.py -- time of the GPU tracking tail's hot path (plf_track_close_points: one launch, one wave or one workgroup per frame), device in
and out, on three shapes:
  frames  8192 frames x 1000 key points, 300 of them matched, depths drawn so that a third of the frames have fewer than 100 entries below th_depth
  single  the first of those frames alone: what a one-frame caller pays
  big     64 frames x 4000 key points (the workgroup class)
Warm-up, then the median of `--calls` calls timed with device events on one stream.  Beside each the single-thread loop a caller runs today
(tools/track_cpu.cpp: std::sort and a walk, g++ -O2 -ffp-contract=off, on the host this tool runs on) over the same frames, and whether the two write
the same bits.  States whether the device call is no slower than the C++ loop at the 8192-frame shape.  Also the three elementwise / per-wave calls
of the tail at the frames shape.  Writes profiles/track.json.

The per-kernel time comes from a kernel trace taken in a run of its own:
    rocprofv3 --kernel-trace --stats -d DIR --output-format csv -- python tools/bench_track.py --calls 3 --no-json --no-cpu --shape SHAPE
    python tools/bench_track.py --kernel-stats DIR --shape SHAPE
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
OUT = os.path.join(ROOT, "profiles", "track.json")
SHAPES = {"frames": (8192, 1000, 300), "single": (1, 1000, 300), "big": (64, 4000, 1200)}


def make_frames(F, S, n_match, rng, n_points=4096):
    """F frames in the layout of tests/trackgen.pack, vectorised"""
    import numpy as np
    import trackgen as G
    th = float(G.TH_DEPTH)
    keys = np.zeros((F, S), G.KP)
    keys["x"], keys["y"] = rng.uniform(0, 640, (F, S)), rng.uniform(0, 480, (F, S))
    far_share = rng.choice([0.3, 0.6, 0.95], F)[:, None]            # the last kind leaves fewer than 100 close entries among 1000
    depth = np.where(rng.random((F, S)) < far_share, rng.uniform(1.05, 3.0, (F, S)), rng.uniform(0.1, 0.95, (F, S))) * th
    depth[rng.random((F, S)) < 0.1] = 0.0
    match = np.full((F, S), -1, np.int32)
    where = np.argsort(rng.random((F, S)), 1)[:, :n_match]
    match[np.arange(F)[:, None], where] = rng.integers(0, n_points, (F, n_match)).astype(np.int32)
    n_obs = rng.integers(0, 4, n_points).astype(np.int32)
    pose = np.stack([G.pose12(rng) for _ in range(min(F, 64))])
    fr = np.stack([G.R.frustum(q) for q in pose])[np.arange(F) % len(pose)]
    return dict(keys=keys, depth=depth.astype(np.float32), match=match, n=np.full(F, S, np.int32), n_obs=n_obs, frustum=fr.astype(np.float32), row_id=None, stride=S)


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
        print(json.dumps(benchlib.merge_kernel_stats(OUT, a.kernel_stats, "k_track_", lambda res, split: res[a.shape or "frames"].update(per_kernel_ms_traced=split))[1]))
        return
    import numpy as np
    import torch
    import trackgen as G
    from rgbd_pl_slam_amd import close_points, need_new_keyframe, motion_model, clean_matches
    from rgbd_pl_slam_amd.track import TrackResult
    assert torch.cuda.is_available(), "bench_track.py needs the GPU"
    cuda = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()   # noqa: E731
    st = torch.cuda.Stream()
    res = {"what": "plf_track_close_points, device in and out, one launch per call; median of calls, device events", "calls": a.calls, "warmup": a.warmup,
           "cpu_loop": "tools/track_cpu.cpp, one thread, g++ -O2 -ffp-contract=off, on the host of this run, over the same frames",
           "th_depth": float(G.TH_DEPTH), "min_points": 100}
    for name, (F, S, n_match) in SHAPES.items():
        if a.shape and a.shape != name:
            continue
        p = make_frames(F, S, n_match, np.random.default_rng(7))
        keys = cuda(np.frombuffer(p["keys"].tobytes(), np.uint8).reshape(F, -1).copy())
        depth, match, n_obs, fr = cuda(p["depth"]), cuda(p["match"]), cuda(p["n_obs"]), cuda(p["frustum"])
        out = TrackResult(new_kp=torch.full((F, S), -1, dtype=torch.int32, device="cuda"), new_pos=torch.zeros((F, S, 3), dtype=torch.float32, device="cuda"),
                          n_new=torch.empty(F, dtype=torch.int32, device="cuda"), n_walked=torch.empty(F, dtype=torch.int32, device="cuda"),
                          status=torch.empty(F, dtype=torch.int32, device="cuda"))
        run = lambda: close_points(keys, depth, match, n_obs, fr, G.CAM, float(G.TH_DEPTH), out=out, stream=st.cuda_stream)   # noqa: E731
        ms, r = benchlib.median_ms(run, st, a.warmup, a.calls)
        torch.cuda.synchronize()
        n_new, n_walked = r.n_new.cpu().numpy(), r.n_walked.cpu().numpy()
        close = ((p["depth"] > 0) & (p["depth"] <= G.TH_DEPTH)).sum(1)
        row = {"frames": F, "key_points": S, "matches": n_match, "ms": ms, "us_per_frame": round(ms["median"] * 1000 / F, 3), "created_median": float(np.median(n_new)),
               "walked_median": float(np.median(n_walked)), "frames_with_fewer_than_100_close": int((close < 100).sum()),
               "frames_with_100_or_more_close": int((close >= 100).sum())}
        if not a.no_cpu:
            G.cpu_loop()                                              # (built before the clock starts)
            sec = []
            c = G.cpu_close(p, seconds=sec)
            same = (np.array_equal(c["n_new"], n_new) and np.array_equal(c["n_walked"], n_walked) and np.array_equal(c["new_kp"], r.new_kp.cpu().numpy())
                    and G.same_bits(c["new_pos"], r.new_pos.cpu().numpy()))
            assert same, "the C++ loop and the GPU write different results"
            row["equal_to_cpu_loop"] = True
            row["ms_cpu_loop_single_thread"] = round(sec[0] * 1000, 3)
            row["cpu_over_gpu"] = round(sec[0] * 1000 / ms["median"], 2)
            row["gpu_not_slower_than_cpu_loop"] = ms["median"] <= sec[0] * 1000
        if name == "frames":                                          # the other three calls of the tail, at this shape
            flags = cuda((np.random.default_rng(8).random((F, S)) < 0.1).astype(np.uint8))
            rng = np.random.default_rng(9)
            states = cuda(G.state_records([G.state(frame_id=100 + k) for k in range(F)]).view(np.uint8).reshape(F, -1))
            start, item = cuda(np.array([0, 1000], np.int32)), cuda(rng.integers(0, 4096, 1000).astype(np.int32))
            pose = cuda(np.stack([G.pose12(rng) for _ in range(64)])[np.arange(F) % 64])
            m2 = match.clone()
            other = {"need_keyframe": lambda: need_new_keyframe(depth, match, n_obs, start, item, states, float(G.TH_DEPTH), stream=st.cuda_stream),
                     "motion_velocity_and_predict": lambda: motion_model(cur=pose, last_frustum=fr, last=pose, predict=True, stream=st.cuda_stream),
                     "clean_vo": lambda: clean_matches("vo", m2, flags, n_obs=n_obs, stream=st.cuda_stream),
                     "clean_outliers": lambda: clean_matches("outliers", m2, flags, stream=st.cuda_stream)}
            row["other_calls_ms"] = {k: benchlib.median_ms(fn, st, a.warmup, a.calls)[0] for k, fn in other.items()}
        res[name] = row
        print(name, json.dumps(row), flush=True)
    if not a.no_json and not a.shape:
        json.dump(res, open(OUT, "w"), indent=1)
    if "frames" in res and not res["frames"].get("gpu_not_slower_than_cpu_loop", True):
        sys.exit("the device call is slower than the C++ loop")


if __name__ == "__main__":
    main()

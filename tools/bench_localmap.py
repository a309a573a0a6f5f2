"""tools/bench_localmap.py -- time of the GPU local map (plf_local_keyframes + plf_local_items, then plf_local_gather + plf_local_visible), device in
and out, on the map of tools/bench_covis.py (10,000 keyframes, 500,000 points, about 4.2 M observations) and its 8192 frames of 300 matched points:
the votes of every frame (stride 256, so a longer seed is cut on both sides alike) and a whole-graph UpdateConnections are computed once and stay on
the device, the spanning tree hangs every keyframe on one of the five before it.
  chain   plf_local_keyframes + plf_local_items for all frames in one call each
  fill    plf_local_gather (positions, normals, distances, descriptors) + plf_local_visible (with the map's mnVisible) on the chain's lists
  single  the same two pairs for one frame: what a one-frame caller pays in launches
  expand  8192 frames whose 300 points are drawn from ONE keyframe's row, points seen from at most 8 keyframes only: the votes name fewer than 80
          keyframes, so the expansion loop of plf_local_keyframes runs (in `frames` every seed list is longer than 80 and nothing is expanded) and a frame
          concatenates a few dozen rows instead of 256
Warm-up, then the median of `--calls` calls timed with device events on one stream.  Beside them the time of the single-thread loop a caller runs
today (tools/localmap_cpu.cpp, built here with -O3 -march=native, on the host this tool runs on) and whether the two produce equal lists (a
position-weighted checksum over both lists, the seen flags and the true counts).  States whether the device chain is no slower than the C++ loop.
Writes profiles/localmap.json.

The per-kernel split comes from a kernel trace taken in a run of its own:
    rocprofv3 --kernel-trace --stats -d DIR --output-format csv -- python tools/bench_localmap.py --calls 3 --no-json --no-cpu --shape SHAPE
    python tools/bench_localmap.py --kernel-stats DIR --shape SHAPE
one shape per trace, so that an average is an average over calls of one size.
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
from bench_covis import make_map, N_KF, N_POINTS, N_FRAMES, FRAME_POINTS  # noqa: E402
OUT = os.path.join(ROOT, "profiles", "localmap.json")
SEED_STRIDE, KF_STRIDE, ITEM_STRIDE = 256, 264, 4096
MASK = (1 << 64) - 1


def checksum(local_kf, n_kf, local_item, n_item, seen):
    """the sum tools/localmap_cpu.cpp prints, from the device lists (64-bit wrap-around arithmetic on both sides)"""
    import torch
    def weights(stride):
        return ((torch.arange(1, stride + 1, dtype=torch.int64, device=local_kf.device) * 2654435761) & 0xFFFFFFFF)[None, :]
    def part(lst, n, extra=None):
        stride = lst.shape[1]
        live = torch.arange(stride, device=lst.device)[None, :] < n[:, None]
        v = lst.to(torch.int64) + 1
        if extra is not None:
            v = v + (extra.to(torch.int64) << 40)
        return int((v * weights(stride) * live).sum()) & MASK
    return (int(n_kf.sum()) + int(n_item.sum()) + part(local_kf, n_kf) + part(local_item, n_item, seen)) & MASK


def cpu_loop(arrays, args, reps):
    with tempfile.TemporaryDirectory() as d:
        exe = benchlib.build_cpp("localmap_cpu.cpp", d, "-O3", "-march=native")
        for name, a in arrays.items():
            a.tofile(os.path.join(d, name + ".i32"))
        out = subprocess.check_output([exe, d, *map(str, args), str(reps)], text=True).split()
    return float(out[1]), int(out[3])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--frames", type=int, default=N_FRAMES)
    ap.add_argument("--no-json", action="store_true")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--cpu-repeats", type=int, default=1)
    ap.add_argument("--shape", default=None, choices=("frames", "single", "expand"), help="this shape only (for a kernel trace)")
    ap.add_argument("--kernel-stats", default=None, help="directory of a rocprofv3 --kernel-trace --stats run of this tool: merge the per-kernel split")
    a = ap.parse_args()
    if a.kernel_stats:
        print(json.dumps(benchlib.merge_kernel_stats(OUT, a.kernel_stats, "k_local_", lambda res, split: res[a.shape or "frames"].update(per_kernel_ms_traced=split))[1]))
        return
    import numpy as np
    import torch
    from rgbd_pl_slam_amd import update_connections, local_keyframe_votes, local_keyframes, local_items, local_gather, local_visible, children_csr
    assert torch.cuda.is_available(), "bench_localmap.py needs the GPU"
    rng = np.random.default_rng(7)
    obs_start, obs_kf, row_start, row_point = make_map(rng)
    F = a.frames
    frame_point = rng.integers(0, N_POINTS, (N_FRAMES, FRAME_POINTS)).astype(np.int32)
    frame_point[rng.random(frame_point.shape) < 0.1] = -1           # unmatched features
    frame_point = frame_point[:F]
    frame_start = (np.arange(F + 1, dtype=np.int64) * FRAME_POINTS).astype(np.int32)
    counts = np.diff(obs_start)
    near = np.full((F, FRAME_POINTS), -1, np.int32)                 # the `expand` shape
    for f, c in enumerate(rng.integers(0, N_KF, F)):
        cand = row_point[row_start[c]:row_start[c + 1]]
        cand = cand[counts[cand] <= 8]
        if len(cand):
            near[f] = cand[rng.integers(0, len(cand), FRAME_POINTS)]
    parent = (np.arange(N_KF) - rng.integers(1, 6, N_KF)).astype(np.int32)
    parent[parent < 0] = -1
    cuda = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()   # noqa: E731
    d_os, d_ok, d_rs, d_rp, d_fs, d_par = map(cuda, (obs_start, obs_kf, row_start, row_point, frame_start, parent))
    st = torch.cuda.Stream()
    cov = update_connections(d_rs, d_rp, torch.arange(N_KF, dtype=torch.int32, device="cuda"), d_os, d_ok, N_KF, 256, 15)
    c_start, c_kf = children_csr(d_par)
    torch.cuda.synchronize()

    def outputs(rows):
        i32 = lambda *s: torch.full(s, -1, dtype=torch.int32, device="cuda")   # noqa: E731
        return (i32(rows, KF_STRIDE), i32(rows), i32(rows)), (i32(rows, ITEM_STRIDE), i32(rows), torch.zeros((rows, ITEM_STRIDE), dtype=torch.uint8, device="cuda"), i32(rows))

    def chain(rows, outs, votes, d_fp):
        kf = local_keyframes(votes.conn_kf[:rows], votes.n_conn[:rows], cov.ord_kf, cov.n_ord, c_start, c_kf, d_par, N_KF, out=outs[0], stream=st.cuda_stream)
        return kf, local_items(kf[0], kf[1], d_rs, d_rp, N_POINTS, frame_row_start=d_fs[:rows + 1], frame_row_item=d_fp, out=outs[1], stream=st.cuda_stream)

    mp = dict(world_pos=torch.rand((N_POINTS, 3), device="cuda"), normal=torch.rand((N_POINTS, 3), device="cuda"), min_distance=torch.rand(N_POINTS, device="cuda"),
              max_distance=torch.rand(N_POINTS, device="cuda"), desc=torch.randint(0, 256, (N_POINTS, 32), dtype=torch.uint8, device="cuda"))
    visible = torch.zeros(N_POINTS, dtype=torch.int32, device="cuda")

    def fill(rows, item, n_item, seen, dst, in_view, n_to, d_fp):
        local_gather(item, n_item, out=dst, stream=st.cuda_stream, **mp)
        return local_visible(item, n_item, seen, in_view, visible, d_fs[:rows + 1], d_fp, n_to_match=n_to, stream=st.cuda_stream)

    res = {"what": "plf_local_keyframes + plf_local_items (chain), plf_local_gather + plf_local_visible (fill), device in and out; median of calls, device events",
           "calls": a.calls, "warmup": a.warmup,
           "cpu_loop": "tools/localmap_cpu.cpp, one thread, g++ -O3 -march=native, best of %d, on the host of this run" % a.cpu_repeats,
           "map": {"keyframes": N_KF, "points": N_POINTS, "observations": int(obs_start[-1])},
           "n_frames": F, "strides": {"seed": SEED_STRIDE, "kf": KF_STRIDE, "item": ITEM_STRIDE}}
    for name, rows, points in (("frames", F, frame_point), ("single", 1, frame_point), ("expand", F, near)):
        if a.shape and a.shape != name:
            continue
        d_fp = cuda(points.reshape(-1))
        votes = local_keyframe_votes(d_fs, d_fp, d_os, d_ok, N_KF, SEED_STRIDE)
        torch.cuda.synchronize()
        n_seed = votes.n_conn.cpu().numpy()[:rows]
        outs = outputs(rows)
        ms_chain, (kf, it) = benchlib.median_ms(lambda: chain(rows, outs, votes, d_fp), st, a.warmup, a.calls)
        dst = {k: torch.zeros((rows * ITEM_STRIDE,) + tuple(v.shape[1:]), dtype=v.dtype, device="cuda") for k, v in mp.items()}
        frustum = torch.randint(0, 2, (rows * ITEM_STRIDE,), dtype=torch.uint8, device="cuda")
        in_view, n_to = frustum.clone(), torch.zeros(rows, dtype=torch.int32, device="cuda")

        def run_fill():
            in_view.copy_(frustum)                                  # (the stream's own copy: part of what a caller does between frustum and visible)
            return fill(rows, it[0], it[1], it[2], dst, in_view, n_to, d_fp)
        with torch.cuda.stream(st):
            ms_fill, _ = benchlib.median_ms(run_fill, st, a.warmup, a.calls)
        n_kf, n_item = kf[1].cpu().numpy(), it[1].cpu().numpy()
        row = {"rows": rows, "seeds_per_frame": {"median": float(np.median(n_seed)), "max": int(n_seed.max())}, "ms_chain": ms_chain, "ms_fill": ms_fill, "local_keyframes": {"median": float(np.median(n_kf)), "max": int(n_kf.max())},
               "local_points": {"median": float(np.median(n_item)), "max": int(n_item.max())}, "n_to_match_median": float(np.median(n_to.cpu().numpy()))}
        if name == "single":
            row["beside"] = "0.106 ms of a single detect_reloc query (profiles/kfdb.json)"
        elif not a.no_cpu:
            arrays = dict(seed_kf=votes.conn_kf.cpu().numpy(), n_seed=votes.n_conn.cpu().numpy(), covis_kf=cov.ord_kf.cpu().numpy(), n_covis=cov.n_ord.cpu().numpy(),
                          child_start=c_start.cpu().numpy(), child_kf=c_kf.cpu().numpy(), kf_parent=parent, kf_row_start=row_start, kf_row_item=row_point,
                          frame_row_start=frame_start, frame_row_item=points.reshape(-1))
            cms, chk = cpu_loop(arrays, (SEED_STRIDE, 256, N_POINTS, KF_STRIDE, ITEM_STRIDE), a.cpu_repeats)
            mine = checksum(kf[0], kf[1], it[0], it[1], it[2])
            assert chk == mine, ("the C++ loop and the GPU disagree", chk, mine)
            row["lists_equal_to_cpu_loop"] = True
            row["ms_cpu_loop_single_thread"] = round(cms, 3)
            row["cpu_over_gpu_chain"] = round(cms / ms_chain["median"], 1)
            row["gpu_chain_not_slower_than_cpu_loop"] = ms_chain["median"] <= cms
        res[name] = row
        print(name, json.dumps(row), flush=True)
    if not a.no_json and not a.shape:
        json.dump(res, open(OUT, "w"), indent=1)
    if any(not res[k].get("gpu_chain_not_slower_than_cpu_loop", True) for k in ("frames", "expand") if k in res):
        sys.exit("the device chain is slower than the C++ loop")


if __name__ == "__main__":
    main()

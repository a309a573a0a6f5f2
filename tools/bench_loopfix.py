"""tools/bench_loopfix.py -- time of the loop-correction calls (include/plf.h, "Loop correction"), device in and out, on the 10,000-keyframe /
500,000-point / 4.17 M-observation map of tools/bench_covis.py, three shapes:
  loop       plf_loop_sim3_pairs, plf_loop_correct_points, plf_loop_new_poses, plf_loop_normal_depth, plf_loop_commit_poses for K = 30 and K = 300
             connected keyframes (consecutive slots around the current one, their rows of the map)
  essential  plf_loop_new_poses + plf_loop_commit_poses over all keyframes and plf_loop_correct_points_by_ref over all points
  gba        plf_gba_propagate_poses + plf_gba_correct_points over the whole map, 50 keyframes unflagged, on a binary spanning tree (depth 13) and on a
             tree that is one chain of 10,000 keyframes
Warm-up, then the median of `--calls` calls timed with device events on one stream.  Every call of `loop` uses a new current-keyframe id, so that it
moves every point again.  Beside each shape the single-thread loops a caller runs today, as the reference writes them -- the walk over the K rows
alone, the by-reference loop over all points, the breadth-first queue -- (tools/loopfix_cpu.cpp, g++ -O2 -ffp-contract=off, on the host this tool
runs on) from the same state; the first call of each is checked bit-equal to the device's.  Also reported: the download and upload of
world_pos, normal, the two distances, the poses and the centres that the host loop forces on a caller whose map lives on the device.
CONDITION, stated and checked: the device chain takes no longer than the host loop at `essential` and at `loop` with K = 300.  A shape that misses it
is reported as such.  Writes profiles/loopfix.json.

The per-kernel time comes from a kernel trace taken in a run of its own:
    rocprofv3 --kernel-trace --stats -d DIR --output-format csv -- python tools/bench_loopfix.py --calls 3 --no-json --no-cpu
    python tools/bench_loopfix.py --kernel-stats DIR
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
OUT = os.path.join(ROOT, "profiles", "loopfix.json")
UNFLAGGED = 50


def make_map():
    import numpy as np
    import bench_covis
    import loopfixgen as G
    import loopfixref as R
    rng = np.random.default_rng(20240607)
    obs_start, obs_kf, row_start, row_point = bench_covis.make_map(rng)
    n_kf, n = bench_covis.N_KF, bench_covis.N_POINTS
    sc = {"n_kf": n_kf, "n_points": n, "obs_start": obs_start, "obs_kf": obs_kf, "all_row_start": row_start, "all_row_point": row_point}
    # poses: rotation about y by the slot's angle on a circle, a translation; float32.  The centres through the definition's SetPose arithmetic, vectorised.
    th = np.arange(n_kf) * (2 * np.pi / n_kf)
    T = np.zeros((n_kf, 3, 4))
    T[:, 0, 0], T[:, 0, 2], T[:, 1, 1], T[:, 2, 0], T[:, 2, 2] = np.cos(th), np.sin(th), 1.0, -np.sin(th), np.cos(th)
    T[:, :, 3] = rng.normal(size=(n_kf, 3)) * 3
    sc["kf_tcw"] = T.astype(np.float32).reshape(n_kf, 12)
    Tf = sc["kf_tcw"].astype(np.float64).reshape(n_kf, 3, 4)
    sc["kf_ow"] = ((Tf[:, 0, :3] * Tf[:, 0, 3:4] + Tf[:, 1, :3] * Tf[:, 1, 3:4] + Tf[:, 2, :3] * Tf[:, 2, 3:4]) * -1.0).astype(np.float32)
    assert (sc["kf_ow"][:8] == np.stack([R.ow_of(t) for t in sc["kf_tcw"][:8]])).all()
    sc["kf_id"] = (np.arange(n_kf, dtype=np.int64) * 3 + 5)
    sc["world_pos"] = rng.uniform(-20, 20, (n, 3)).astype(np.float32)
    sc["normal"] = np.zeros((n, 3), np.float32)
    sc["min_distance"], sc["max_distance"] = np.zeros(n, np.float32), np.zeros(n, np.float32)
    sc["point_bad"] = (rng.uniform(size=n) < 0.01).astype(np.uint8)
    sc["corrected_by"], sc["corrected_ref"] = np.full(n, -1, np.int64), np.full(n, -1, np.int64)
    sc["ref_kf"] = obs_kf[obs_start[:-1]].astype(np.int32)
    sc["ref_level"] = rng.integers(0, G.NLEVELS, n).astype(np.int32)
    sc["scale_factors"] = (np.float32(1.2) ** np.arange(G.NLEVELS)).astype(np.float32)
    sc["G"], sc["R"] = G, R
    return sc


def loop_shape(sc, K):
    import numpy as np
    G = sc["G"]
    cur = sc["n_kf"] // 2
    rank_kf = np.arange(cur - K // 2, cur - K // 2 + K, dtype=np.int32)
    rs = sc["all_row_start"]
    rows = [sc["all_row_point"][rs[k]:rs[k + 1]] for k in rank_kf]
    row_start = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    T = sc["kf_tcw"][cur].astype(np.float64).reshape(3, 4)
    Rc = G.rot(np.random.default_rng(K), 0.02)
    scw = G.quat_row(Rc @ T[:, :3], 1.02 * (Rc @ T[:, 3]) + 0.1, 1.02)
    return dict(K=K, cur=cur, rank_kf=rank_kf, row_start=row_start, row_point=np.ascontiguousarray(np.concatenate(rows), np.int32), scw=scw)


def cpu_lib():
    so = os.path.join(tempfile.mkdtemp(prefix="loopfix_cpu_"), "loopfix_cpu.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-Wno-unused-function",
                           os.path.join(ROOT, "tools", "loopfix_cpu.cpp"), "-o", so])
    from rgbd_pl_slam_amd import _lib as L
    return L.loopfix_prototypes(C.CDLL(so), "loopfix_cpu")


MAP = ("kf_tcw", "kf_ow", "world_pos", "normal", "min_distance", "max_distance", "corrected_by", "corrected_ref")


def host_state(sc):
    import numpy as np
    return {k: np.array(sc[k], copy=True) for k in MAP}


def host_loop(lib, sc, sh, m, cur_id):
    """the two loops of CorrectLoop as the reference writes them: the Sim3 pairs, then loopfix_cpu_correct_loop -- only the K rows and the points it moves"""
    import numpy as np
    from rgbd_pl_slam_amd import _lib as L
    G = sc["G"]
    p = G.ptr
    K, n, n_kf = sh["K"], sc["n_points"], sc["n_kf"]
    cor, non = np.zeros((K, 8)), np.zeros((K, 8))
    lib.loopfix_cpu_sim3_pairs(p(m["kf_tcw"]), p(m["kf_ow"]), n_kf, p(sh["rank_kf"]), K, sh["cur"], p(sh["scw"]), p(cor), p(non))
    v = L.LoopView(K, p(sh["rank_kf"]), p(sh["row_start"]), p(sh["row_point"]), n, p(sc["point_bad"]), n_kf, p(sc["kf_id"]))
    gv = G.geom_view(L, sc, m["kf_ow"])
    st = lib.loopfix_cpu_correct_loop(C.byref(v), C.byref(gv), p(cor), p(non), cur_id, p(m["kf_tcw"]), p(m["kf_ow"]), p(m["world_pos"]), p(m["corrected_by"]),
                                      p(m["corrected_ref"]), p(m["normal"]), p(m["min_distance"]), p(m["max_distance"]), None, None)
    assert st == 0


def timed_host(fn, reps):
    import numpy as np
    ms = []
    for _ in range(reps):
        t = time.perf_counter(); fn(); ms.append((time.perf_counter() - t) * 1e3)
    return round(float(np.median(ms)), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-json", action="store_true")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--cpu-repeats", type=int, default=3)
    ap.add_argument("--kernel-stats", default=None, help="directory of a rocprofv3 --kernel-trace --stats run of this tool: merge the per-kernel split")
    a = ap.parse_args()
    if a.kernel_stats:
        def put(res, split):
            res["kernels"] = split
        split = {}
        for prefix in ("k_loop", "k_gba", "k_mapgeom"):
            split.update(benchlib.kernel_split(a.kernel_stats, prefix))
        res = json.load(open(OUT)); put(res, split); json.dump(res, open(OUT, "w"), indent=1)
        print(json.dumps(split))
        return
    import numpy as np
    import torch
    from rgbd_pl_slam_amd import loopfix as LF
    if not torch.cuda.is_available():
        sys.exit("bench_loopfix needs the GPU")
    sc = make_map()
    G = sc["G"]
    lib = None if a.no_cpu else cpu_lib()
    st = torch.cuda.Stream()
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()  # noqa: E731
    const = {k: t(sc[k]) for k in ("kf_id", "point_bad", "obs_start", "obs_kf", "ref_kf", "ref_level", "scale_factors")}
    res = {"map": {"keyframes": sc["n_kf"], "points": sc["n_points"], "observations": int(sc["obs_start"][-1])}, "calls": a.calls, "shapes": {}}

    # ---- the transfer a host loop forces: the six arrays down and up again
    d = {k: t(sc[k]) for k in MAP}
    torch.cuda.synchronize()
    xfer = []
    for _ in range(3):
        t0 = time.perf_counter()
        h = {k: d[k].cpu() for k in ("world_pos", "normal", "min_distance", "max_distance", "kf_tcw", "kf_ow")}
        for k, x in h.items():
            d[k].copy_(x)
        torch.cuda.synchronize()
        xfer.append((time.perf_counter() - t0) * 1e3)
    res["transfer_ms"] = round(float(np.median(xfer)), 3)

    # ---- loop
    for K in (30, 300):
        sh = loop_shape(sc, K)
        d = {k: t(sc[k]) for k in MAP}
        ds = {k: t(sh[k]) for k in ("rank_kf", "row_start", "row_point", "scw")}
        geom = dict(G.geom_kwargs(const, d["kf_ow"]))
        call = [0]

        def run():
            call[0] += 1
            return LF.loop_correct(d["kf_tcw"], d["kf_ow"], const["kf_id"], ds["rank_kf"], sh["cur"], 10 ** 6 + call[0], ds["scw"], ds["row_start"], ds["row_point"],
                                   const["point_bad"], d["world_pos"], d["corrected_by"], d["corrected_ref"], d["normal"], d["min_distance"], d["max_distance"],
                                   geom, stream=st.cuda_stream)
        with torch.cuda.stream(st):
            first = run()
            torch.cuda.synchronize()
            entry = {"K": K, "row_entries": int(sh["row_start"][-1]), "points_moved": int((first.owner_rank >= 0).sum().item())}
            if lib is not None:
                m = host_state(sc)
                host_loop(lib, sc, sh, m, 10 ** 6 + 1)
                same = all(G.same_bits(m[k], d[k].cpu().numpy()).all() for k in MAP)
                entry["bit_equal"] = bool(same)
                ids = iter(range(10 ** 6 + 2, 10 ** 7))
                entry["host_loop_ms"] = timed_host(lambda: host_loop(lib, sc, sh, m, next(ids)), a.cpu_repeats)
                entry["host_loop_with_transfer_ms"] = round(entry["host_loop_ms"] + res["transfer_ms"], 3)
            entry["device_ms"], _ = benchlib.median_ms(run, st, a.warmup, a.calls)
        if lib is not None:
            entry["device_no_slower"] = bool(entry["device_ms"]["median"] <= entry["host_loop_ms"])
        res["shapes"]["loop_K%d" % K] = entry
        print(json.dumps({"loop_K%d" % K: entry}), flush=True)

    # ---- essential
    rng = np.random.default_rng(5)
    n_kf, n = sc["n_kf"], sc["n_points"]
    _, vscw = None, np.zeros((n_kf, 8))
    p = G.ptr
    every = np.arange(n_kf, dtype=np.int32)
    siw = np.zeros((n_kf, 8))
    R = sc["R"]
    base = [R.row8(R.from_pose(sc["kf_tcw"][k])) for k in range(0, n_kf, 100)]             # (the definition is slow: one quaternion per 100 slots, the rest a copy)
    for k in range(n_kf):
        vscw[k] = base[k // 100]
        siw[k] = vscw[k]; siw[k, 7] = 1.0 + 0.0001 * (k % 7); siw[k, 4:7] += 0.01
    swc = np.zeros((n_kf, 8))
    for k0 in range(0, n_kf, 100):
        for j in range(7):
            row = siw[k0 + j].copy()
            inv = R.row8(R.inverse(R.sim3_of(row)))
            for k in range(k0 + j, min(k0 + 100, n_kf), 7):
                swc[k] = inv
    id_to_slot = np.full(int(sc["kf_id"].max()) + 1, -1, np.int32); id_to_slot[sc["kf_id"]] = every
    marks_by = np.where(rng.uniform(size=n) < 0.3, 77, -1).astype(np.int64)
    marks_ref = sc["kf_id"][rng.integers(0, n_kf, n)]
    d = {k: t(sc[k]) for k in MAP}
    d["corrected_by"], d["corrected_ref"] = t(marks_by), t(marks_ref)
    de = {k: t(v) for k, v in dict(siw=siw, vscw=vscw, swc=swc, id_to_slot=id_to_slot, every=every).items()}

    def run_e():
        tcw_new, ow_new = LF.loop_new_poses(de["siw"], st.cuda_stream)
        LF.loop_commit_poses(de["every"], tcw_new, ow_new, d["kf_tcw"], d["kf_ow"], st.cuda_stream)
        return LF.loop_correct_points_by_ref(const["point_bad"], const["ref_kf"], d["corrected_by"], d["corrected_ref"], 77, de["id_to_slot"], de["vscw"], de["swc"],
                                             d["world_pos"], stream=st.cuda_stream)
    with torch.cuda.stream(st):
        moved = run_e()
        torch.cuda.synchronize()
        entry = {"points_moved": int(moved.sum().item())}
        if lib is not None:
            m = host_state(sc)
            tcw_new, ow_new, mv = np.zeros((n_kf, 12), np.float32), np.zeros((n_kf, 3), np.float32), np.zeros(n, np.uint8)

            def host_e():
                lib.loopfix_cpu_new_poses(p(siw), n_kf, p(tcw_new), p(ow_new))
                lib.loopfix_cpu_commit_poses(p(every), n_kf, p(tcw_new), p(ow_new), p(m["kf_tcw"]), p(m["kf_ow"]), n_kf)
                lib.loopfix_cpu_correct_points_by_ref(n, p(sc["point_bad"]), p(sc["ref_kf"]), p(marks_by), p(marks_ref), 77, p(id_to_slot), len(id_to_slot), p(vscw),
                                                      p(swc), n_kf, p(m["world_pos"]), p(mv))
            host_e()
            entry["bit_equal"] = bool(all(G.same_bits(m[k], d[k].cpu().numpy()).all() for k in ("kf_tcw", "kf_ow", "world_pos")))
            entry["host_loop_ms"] = timed_host(host_e, a.cpu_repeats)
            entry["host_loop_with_transfer_ms"] = round(entry["host_loop_ms"] + res["transfer_ms"], 3)
        entry["device_ms"], _ = benchlib.median_ms(run_e, st, a.warmup, a.calls)
    if lib is not None:
        entry["device_no_slower"] = bool(entry["device_ms"]["median"] <= entry["host_loop_ms"])
    res["shapes"]["essential"] = entry
    print(json.dumps({"essential": entry}), flush=True)

    # ---- gba: 50 unflagged keyframes in ten chains of five, in a binary spanning tree (depth 13) and in a tree that is ONE chain (depth 9,999: a
    # keyframe's parent is usually the keyframe before it, so a map's tree is close to this)
    def tree(shape):
        if shape == "binary":
            parent = ((np.arange(n_kf) - 1) // 2).astype(np.int32)
        else:
            parent = (np.arange(n_kf) - 1).astype(np.int32)
        parent[0] = -1
        flag = np.ones(n_kf, np.uint8)
        for j in range(10):
            k = n_kf - 1 - (40 * j if shape == "binary" else 900 * j)
            for _ in range(UNFLAGGED // 10):
                flag[k] = 0; k = int(parent[k])
        assert int((flag == 0).sum()) == UNFLAGGED
        return parent, flag
    origins = np.zeros(1, np.int32)
    gba = sc["kf_tcw"].copy(); gba[:, 3] += np.float32(0.01)
    point_flag = (rng.uniform(size=n) < 0.9).astype(np.uint8)
    pos_gba = (sc["world_pos"] + np.float32(0.01)).astype(np.float32)
    for shape in ("binary", "chain"):
        parent, flag = tree(shape)
        d = {k: t(sc[k]) for k in ("kf_tcw", "kf_ow", "world_pos")}
        dg = {k: t(v) for k, v in dict(parent=parent, origins=origins, gba=gba, point_flag=point_flag, pos_gba=pos_gba).items()}
        dflag, dflag0 = t(flag), t(flag)

        def run_g():
            dflag.copy_(dflag0)
            return LF.gba_correct(dg["parent"], dg["origins"], dflag, dg["gba"], d["kf_tcw"], d["kf_ow"], const["point_bad"], dg["point_flag"], dg["pos_gba"],
                                  const["ref_kf"], d["world_pos"], stream=st.cuda_stream)
        with torch.cuda.stream(st):
            run_g()
            torch.cuda.synchronize()
            entry = {"unflagged": UNFLAGGED, "tree": shape}
            if lib is not None:
                from rgbd_pl_slam_amd import _lib as L
                m = {k: np.array(sc[k], copy=True) for k in ("kf_tcw", "kf_ow", "world_pos")}
                hg, bef, hflag = gba.copy(), np.zeros((n_kf, 12), np.float32), flag.copy()
                cs, ck = np.zeros(n_kf + 1, np.int32), np.zeros(n_kf, np.int32)
                v = L.GbaView(n_kf, p(parent), p(origins), 1, p(hflag), p(hg), p(m["kf_tcw"]), p(m["kf_ow"]), p(bef))
                lib.loopfix_cpu_gba_children(C.byref(v), p(cs), p(ck))            # (GetChilds(): the caller has them)

                def host_g():
                    hflag[:] = flag
                    lib.loopfix_cpu_gba_queue(C.byref(v), p(cs), p(ck))
                    lib.loopfix_cpu_gba_correct_points(n, p(sc["point_bad"]), p(point_flag), p(pos_gba), p(sc["ref_kf"]), p(hflag), p(bef), p(m["kf_tcw"]), p(m["kf_ow"]),
                                                       n_kf, p(m["world_pos"]))
                host_g()
                entry["bit_equal"] = bool(all(G.same_bits(m[k], d[k].cpu().numpy()).all() for k in m) and G.same_bits(hg, dg["gba"].cpu().numpy()).all())
                entry["host_loop_ms"] = timed_host(host_g, a.cpu_repeats)
                entry["host_loop_with_transfer_ms"] = round(entry["host_loop_ms"] + res["transfer_ms"], 3)
            entry["device_ms"], _ = benchlib.median_ms(run_g, st, a.warmup, a.calls)
        if lib is not None:
            entry["device_no_slower"] = bool(entry["device_ms"]["median"] <= entry["host_loop_ms"])
        res["shapes"]["gba_" + shape] = entry
        print(json.dumps({"gba_" + shape: entry}), flush=True)

    if lib is not None:
        res["condition"] = "device chain no slower than the host loop at essential and at loop K = 300"
        res["condition_met"] = bool(res["shapes"]["essential"]["device_no_slower"] and res["shapes"]["loop_K300"]["device_no_slower"])
    if not a.no_json:
        json.dump(res, open(OUT, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

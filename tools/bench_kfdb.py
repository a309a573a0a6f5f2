"""tools/bench_kfdb.py -- time of the GPU KeyFrameDatabase (plf_kfdb_detect_reloc), device-resident: the full-size generated tree of tools/bench_bow.py
(k = 10, L = 6), a database of 10,000 keyframes from 1000-descriptor frames, relocalisation with Q = 1 and Q = 512 queries per call.  Warm-up, then the
median of `--calls` calls timed with device events.  The yardstick is the single-thread host loop a caller runs today, tools/kfdb_cpu.cpp (built here,
-O3 -march=native, same host), fed the very same vectors; its candidates must equal the GPU's for all 512 queries.  Writes profiles/kfdb.json.

Frames draw 70 % of their descriptors from a scene pool of 20,000 words and 30 % from the whole tree, so that words repeat across keyframes as they do
along a trajectory (uniform draws from 10^6 words would leave every inverted list nearly empty).

The per-kernel split comes from a kernel trace taken in a run of its own:
    rocprofv3 --kernel-trace --stats -d DIR --output-format csv -- python tools/bench_kfdb.py --calls 3 --no-json --no-cpu
    python tools/bench_kfdb.py --kernel-stats DIR
A measurement needs the GPU: without one this tool fails, it does not fall back."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import benchlib  # noqa: E402
OUT = os.path.join(ROOT, "profiles", "kfdb.json")
NEIGHBOUR_STAGES_MS = {"plf_bow_transform_batch, 8192 frames (README)": 2.37}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, default=10000)
    ap.add_argument("--desc", type=int, default=1000)
    ap.add_argument("--queries", type=int, default=512)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-json", action="store_true")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--kernel-stats", default=None)
    a = ap.parse_args()
    if a.kernel_stats:
        put = lambda res, split: res.update(per_kernel_avg_ms={k: v["avg_ms"] for k, v in split.items()})
        print(json.dumps(benchlib.merge_kernel_stats(OUT, a.kernel_stats, "k_kfdb_", put)[0]))
        return
    import numpy as np
    import torch
    import bowref
    from rgbd_pl_slam_amd import Vocabulary, KeyFrameDatabase
    assert torch.cuda.is_available(), "bench_kfdb.py needs the GPU"
    ref = bowref.make_vocab(2024, 10, 6, bowref.TF_IDF, bowref.L1_NORM)
    V = Vocabulary.from_arrays(ref.k, ref.L, ref.scoring, ref.weighting, ref.parent, ref.desc, ref.weight, ref.is_leaf)
    S, n, Q = a.keyframes, a.desc, a.queries
    rng = np.random.default_rng(7)
    leaves = np.flatnonzero(ref.is_leaf > 0)
    pool = rng.choice(leaves, 20000, replace=False)
    st = torch.cuda.Stream()
    db = KeyFrameDatabase(V, S, n)

    def frames(count):
        """BoW vectors of `count` generated frames, on the device"""
        outs = []
        for lo in range(0, count, 500):
            c = min(500, count - lo)
            pick = np.where(rng.uniform(0, 1, (c, n)) < 0.7, rng.choice(pool, (c, n)), rng.choice(leaves, (c, n)))
            d = ref.desc[pick].copy()
            for _ in range(12):                                      # 12 flipped bits per descriptor
                bit = rng.integers(0, 256, (c, n))
                d[np.arange(c)[:, None], np.arange(n)[None, :], bit >> 3] ^= (1 << (bit & 7)).astype(np.uint8)   # one byte per descriptor and step: no repeats
            nd = torch.full((c,), n, dtype=torch.int32, device="cuda")
            outs.append(V.transform(torch.from_numpy(d).cuda(), nd, 4, stream=st.cuda_stream))
        torch.cuda.synchronize()
        return {k: torch.cat([o[k] for o in outs]) for k in ("word_id", "word_val", "n_words")}

    kf = frames(S)
    qs = frames(Q)
    db.add(kf, np.arange(S), stream=st.cuda_stream)
    covis_slot = torch.from_numpy(rng.integers(0, S, S * 10).astype(np.int32)).cuda()
    covis_start = torch.arange(0, S * 10 + 1, 10, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    t0 = time.perf_counter(); info = db.info(); rebuild_ms = (time.perf_counter() - t0) * 1e3
    MAXC = 64
    # the first call, from the state `add` leaves: what the host loop is compared with
    cand, n_cand, stats = db.detect_relocalization_candidates(qs, (covis_start, covis_slot), MAXC, stream=st.cuda_stream)
    torch.cuda.synchronize()
    g_cand, g_n, g_stats = cand.cpu().numpy(), n_cand.cpu().numpy(), stats.cpu().numpy()
    res = {"what": "plf_kfdb_detect_reloc, device in and out", "tree": {"k": 10, "L": 6, "words": ref.n_words}, "keyframes": S, "descriptors_per_frame": n,
           "inverted_file_entries": info["n_entries"], "rebuild_and_info_ms_wall": round(rebuild_ms, 2), "calls": a.calls, "warmup": a.warmup,
           "mean_sharing_keyframes": float(g_stats[:, 0].mean()), "mean_scored_keyframes": float(g_stats[:, 2].mean()), "mean_candidates": float(g_n.mean())}
    for QQ in (1, Q):
        sub = {k: v[:QQ].contiguous() for k, v in qs.items()}
        res["gpu_ms_Q%d" % QQ] = benchlib.median_ms(lambda: db.detect_relocalization_candidates(sub, (covis_start, covis_slot), MAXC, stream=st.cuda_stream),
                                                    st, a.warmup, a.calls)[0]
    if not a.no_cpu:
        with tempfile.TemporaryDirectory() as td:
            exe = benchlib.build_cpp("kfdb_cpu.cpp", td, "-O3", "-march=native")
            open(os.path.join(td, "meta.txt"), "w").write("%d %d %d %d %d %d %d\n" % (S, n, Q, n, ref.n_words, 10, MAXC))
            for name, t in (("kf_n.i32", kf["n_words"]), ("kf_id.u32", kf["word_id"]), ("kf_val.f64", kf["word_val"]), ("q_n.i32", qs["n_words"]),
                            ("q_id.u32", qs["word_id"]), ("q_val.f64", qs["word_val"]), ("covis_start.i32", covis_start), ("covis_slot.i32", covis_slot)):
                t.cpu().numpy().tofile(os.path.join(td, name))
            cpu = json.loads(subprocess.check_output([exe, td], text=True))
            c_n = np.fromfile(os.path.join(td, "out_n.i32"), np.int32); c_cand = np.fromfile(os.path.join(td, "out_cand.i32"), np.int32).reshape(Q, MAXC)
            assert np.array_equal(c_n, g_n) and np.array_equal(c_cand, g_cand), "the host loop and the GPU disagree"
        res["cpu_single_thread_ms"] = {"first_query": cpu["first_query_ms"], "all_%d_queries" % Q: cpu["all_queries_ms"]}
        res["candidates_equal_host_loop"] = True
        res["ratio_Q1"] = round(cpu["first_query_ms"] / res["gpu_ms_Q1"]["median"], 2)
        res["ratio_Q%d" % Q] = round(cpu["all_queries_ms"] / res["gpu_ms_Q%d" % Q]["median"], 2)
    res["neighbour_stages_ms"] = NEIGHBOUR_STAGES_MS
    res["per_kernel_avg_ms"] = "not measured"
    print(json.dumps(res))
    if not a.no_json:
        json.dump(res, open(OUT, "w"), indent=1)


if __name__ == "__main__":
    main()

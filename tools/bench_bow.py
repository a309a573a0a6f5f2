"""tools/bench_bow.py -- time of the GPU DBoW2 transform (plf_bow_transform_batch), device-resident: the full-size generated tree (k = 10, L = 6, 1.1 M
nodes), 8192 frames x 1000 descriptors, levelsup 4.  Warm-up, then the median of `--calls` calls timed with device events.  Writes
profiles/bow_transform.json: ms per call, descriptors / s and the bytes the descent moves against its algorithmic bytes (n x L x k x 32 B).

The per-kernel split comes from a kernel trace taken in a run of its own (tracing slows the host; the end-to-end figure is taken without it):
    rocprofv3 --kernel-trace --stats -d DIR --output-format csv -- python tools/bench_bow.py --calls 3 --no-json
    python tools/bench_bow.py --kernel-stats DIR
A measurement needs the GPU: without one this tool fails, it does not fall back."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import benchlib  # noqa: E402
OUT = os.path.join(ROOT, "profiles", "bow_transform.json")
EXTRACT_MS_SAME_BATCH = 163.0   # BENCH_r06.json: ORB + LSD extraction step of 8192 frames


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8192)
    ap.add_argument("--desc", type=int, default=1000)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--levelsup", type=int, default=4)
    ap.add_argument("--no-json", action="store_true")
    ap.add_argument("--kernel-stats", default=None, help="directory of a rocprofv3 --kernel-trace --stats run of this tool: merge the per-kernel split")
    a = ap.parse_args()
    if a.kernel_stats:
        def put(res, split):
            res["per_kernel_ms"] = {k: v["avg_ms"] for k, v in split.items()}
            d = res["per_kernel_ms"].get("k_bow_descend16") or res["per_kernel_ms"].get("k_bow_descend32")
            if d:
                res["descent_algorithmic_GBps"] = round(res["descent_algorithmic_bytes"] / (d * 1e-3) / 1e9, 1)
                res["note"] = ("descent_algorithmic_GBps counts the L x k x 32 B of child descriptors each feature compares against; they are served from cache "
                               "(the 35 MB node table is read by every frame), so the rate may exceed the HBM peak and is not an HBM roofline fraction")
        print(json.dumps(benchlib.merge_kernel_stats(OUT, a.kernel_stats, "k_bow_", put)[0]))
        return
    import numpy as np
    import torch
    import bowref
    from rgbd_pl_slam_amd import Vocabulary
    assert torch.cuda.is_available(), "bench_bow.py needs the GPU"
    k, Lv = 10, 6
    ref = bowref.make_vocab(2024, k, Lv, bowref.TF_IDF, bowref.L1_NORM)
    V = Vocabulary.from_arrays(ref.k, ref.L, ref.scoring, ref.weighting, ref.parent, ref.desc, ref.weight, ref.is_leaf)
    F, n = a.frames, a.desc
    # descriptors near leaves, 64 distinct frames tiled over the batch (the tree walk only sees descriptors; frames repeat, the node table does not care)
    base = np.stack([bowref.make_descriptors(ref, 500 + f, n, noise_bits=30) for f in range(64)])
    desc = torch.from_numpy(base).cuda().repeat((F + 63) // 64, 1, 1)[:F].contiguous()
    nd = torch.full((F,), n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    st = torch.cuda.Stream()          # the events and the transform share this stream
    ms, out = benchlib.event_times(lambda: V.transform(desc, nd, a.levelsup, stream=st.cuda_stream), st, a.warmup, a.calls)
    # a spot check that what was timed is the transform: frame 5 against the restatement
    bow, _ = bowref.transform(ref, base[5], a.levelsup)
    nw = int(out["n_words"][5])
    assert nw == len(bow) and np.array_equal(out["word_val"][5, :nw].cpu().numpy().view(np.uint64), np.array([v for _, v in bow]).view(np.uint64))
    med = float(np.median(ms))
    total = F * n
    res = {"what": "plf_bow_transform_batch, device in and out", "tree": {"k": k, "L": Lv, "nodes": ref.n_nodes(), "words": ref.n_words},
           "frames": F, "descriptors_per_frame": n, "levelsup": a.levelsup, "calls": a.calls, "warmup": a.warmup,
           "ms_per_call_median": round(med, 3), "ms_per_call_min": round(min(ms), 3), "ms_per_call_max": round(max(ms), 3),
           "descriptors_per_s": round(total / (med * 1e-3)), "us_per_frame": round(med * 1e3 / F, 3),
           # bytes: the descent reads L x k child descriptors of 32 B per feature (algorithmic); moved from HBM at least: the descriptors in, 16 B of per-feature
           # results out and back in, the outputs (word id 4 + value 8 + node id 4 + start 4 + feature 4 per slot) -- the node table itself (35 MB) stays in cache
           "descent_algorithmic_bytes": total * Lv * k * 32,
           "hbm_bytes_lower_bound": total * (32 + 2 * 16 + 24) + ref.n_nodes() * (32 + 16 + 8),
           "share_of_extraction_step": round(med / EXTRACT_MS_SAME_BATCH, 4), "extraction_step_ms_same_batch": EXTRACT_MS_SAME_BATCH,
           "per_kernel_ms": "not measured"}
    print(json.dumps(res))
    if not a.no_json:
        json.dump(res, open(OUT, "w"), indent=1)


if __name__ == "__main__":
    main()

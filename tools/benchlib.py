"""tools/benchlib.py -- what the bench_*.py tools of the map stage share: the event-timed loop, the build of a CPU loop to compare with, and the
per-kernel split of a rocprofv3 kernel trace."""
import csv
import glob
import json
import os
import subprocess
import sys


def event_times(run, stream, warmup, calls):
    """`warmup` calls of run(), then `calls` calls timed one by one with device events on `stream` (the stream run() enqueues on): the times in ms and
    what the last call returned"""
    import torch
    out = None
    for _ in range(warmup):
        out = run()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        e0.record(stream); out = run(); e1.record(stream)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    torch.cuda.synchronize()
    return ms, out


def median_ms(run, stream, warmup, calls):
    """event_times() as the median / min / max dict the tools write, and what the last call returned"""
    import numpy as np
    ms, out = event_times(run, stream, warmup, calls)
    return {"median": round(float(np.median(ms)), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}, out


def build_cpp(src, d, *flags):
    """g++ FLAGS -std=c++17 tools/SRC -o D/<SRC without .cpp>: the program's path"""
    exe = os.path.join(d, src[:-len(".cpp")])
    subprocess.check_call(["g++", *flags, "-std=c++17", os.path.join(os.path.dirname(os.path.abspath(__file__)), src), "-o", exe])
    return exe


def kernel_split(d, prefix):
    """calls and average ms of every kernel whose name starts with `prefix`, over the *kernel_stats.csv files below d"""
    rows = {}
    for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            name = r["Name"].split("(")[0]
            if name.startswith(prefix):
                c, t = rows.get(name, (0, 0))
                rows[name] = (c + int(r["Calls"]), t + int(r["TotalDurationNs"]))
    return {k: {"calls": c, "avg_ms": round(t / c / 1e6, 4)} for k, (c, t) in rows.items() if c}


def merge_kernel_stats(out, d, prefix, put):
    """--kernel-stats: put(res, split) files the split of the trace below d in the tool's JSON at `out`, which is rewritten; returns (res, split)"""
    res = json.load(open(out))
    split = kernel_split(d, prefix)
    if not split:
        sys.exit("no %s* rows under %s" % (prefix, d))
    put(res, split)
    json.dump(res, open(out, "w"), indent=1)
    return res, split

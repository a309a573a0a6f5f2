"""The C++ adapter ORB_SLAM2_PLF::Sim3Solver (include/plf.hpp) over the mock KeyFrame / MapPoint of tests/mock/ORB_SLAM2/mock_sim3.h, driven by
tests/cpp/sim3_driver.cpp on the GPU: find() on one solver, and the round-robin of LoopClosing::ComputeSim3 over three solvers with iterate(5) per round
until one returns.  The adapter draws its raw values from rand() at SetRansacParameters, in solver order; the test draws the same values from the same
libc after the same srand() and runs tests/sim3ref.py with them: the results are equal bit for bit."""
import ctypes as C
import ctypes.util
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cppbuild  # noqa: E402
import sim3gen as G  # noqa: E402
import sim3ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
SEED, MIN_INLIERS, MAX_ITS = 4321, 20, 60


@pytest.fixture(scope="module", autouse=True)
def _leave_no_cached_device_memory():
    """this module's tensors are released when it ends, so that the modules after it start from the allocator state they would
    find without it"""
    yield
    import gc
    import torch
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _scene():
    jobs = [dict(n1=70, pairs=50, outliers=0.4, null=3, bad=4), dict(n1=40, pairs=24, outliers=0.6, fix_scale=True), dict(n1=64, pairs=48, outliers=0.5, scale=1.25)]
    return G.make_scene(91, jobs, min_inliers=MIN_INLIERS, max_iterations=MAX_ITS, max_hits=1, obs_index=True)


def _write(sc, path):
    J = len(sc["job_kf1"])
    with open(path, "w") as fh:
        fh.write("%d %d %d\n%s\n%d %s\n%d\n" % (SEED, MIN_INLIERS, MAX_ITS, cppbuild.hex32(sc["cam"][:4]), len(sc["level_sigma2"]), cppbuild.hex32(sc["level_sigma2"]), J))
        for j in range(J):
            s1, s2 = 2 * j, 2 * j + 1
            ids = np.concatenate([sc["kf_mappoints"][s1], sc["kf_mappoints"][s2]])
            base, top = ids[ids >= 0].min(), ids.max()
            fh.write("%d %d\n" % (sc["fix_scale"][j], top - base + 1))
            for p in range(base, top + 1):
                fh.write("%s %d\n" % (cppbuild.hex32(sc["world_pos"][p]), sc["point_bad"][p]))
            for s in (s1, s2):
                fh.write("%s %s %d\n" % (cppbuild.hex32(sc["kf_pose"][s][:9]), cppbuild.hex32(sc["kf_pose"][s][9:12]), sc["kf_n"][s]))
                for i in range(sc["kf_n"][s]):
                    mp = sc["kf_mappoints"][s][i]
                    fh.write("%d %d %d\n" % (sc["kf_octave"][s][i], mp - base if mp >= 0 else -1, sc["kf_obs_index"][s][i]))
            n1 = sc["kf_n"][s1]
            fh.write("%d\n" % n1)
            for i1 in range(n1):
                i2 = sc["match12"][j, i1]
                mp = sc["kf_mappoints"][s2][i2] if i2 >= 0 else -1
                fh.write("%d\n" % (mp - base if mp >= 0 else -1))


def _libc_rand(n):
    libc = C.CDLL(ctypes.util.find_library("c") or "libc.so.6")
    libc.srand(SEED)
    return np.array([libc.rand() for _ in range(n)], np.int32)


def _line(words):
    head = [int(w) for w in words[1:5]]
    if not head[2]:
        return head, None, None, None
    bar = words.index("|")
    vals = np.array([int(w) for w in words[5:bar]], np.uint32).view(F32)
    return head, vals[:16].reshape(4, 4), vals[16:29], sorted(int(w) for w in words[bar + 1:])


def _expect(h, j):
    sim3 = h["hit_sim3"][j, 0]
    T = np.eye(4, dtype=F32)
    T[:3, :3] = (sim3[:9] * sim3[12] + F32(0)).reshape(3, 3)
    T[:3, 3] = sim3[9:12]
    return T, sim3, np.flatnonzero(h["hit_inlier12"][j, 0]).tolist(), int(h["hit_inliers"][j, 0])


def test_find_and_round_robin(tmp_path):
    sc = _scene()
    _write(sc, tmp_path / "scenario.txt")
    exe = cppbuild.build_driver("sim3_driver", tmp_path, "-O1", "-Wall", "-Werror")
    subprocess.check_call([str(exe), str(tmp_path)], timeout=120)
    lines = [ln.split() for ln in open(tmp_path / "out.txt")]
    assert [ln[0] for ln in lines] in (["find", "round", "done"], ["find", "done"])
    J = len(sc["job_kf1"])
    raw = _libc_rand(J * MAX_ITS * 3).reshape(J, MAX_ITS, 3)
    # 1. find() on solver 0 alone: its values are the first 3 * MAX_ITS of the stream
    one = dict(sc, rand3=raw[:1].copy())
    for k in ("job_kf1", "job_kf2", "match12", "fix_scale"):
        one[k] = sc[k][:1]
    _, st, ((_, h),) = G.ref_run(one, [MAX_ITS])
    head, T, sim3, inl = _line(lines[0])
    assert h["n_hits"][0] > 0 and head[2] == 1
    wT, wsim3, winl, wn = _expect(h, 0)
    assert G.same_bits(T, wT) and G.same_bits(sim3, wsim3) and inl == winl and head[3] == wn
    # 2. the round-robin: every solver's values in solver order; rounds of iterate(5) until the first solver (in order) returns
    sc["rand3"] = raw
    pr, st = R.pairs(sc, sc["pair_stride"], G.table_of(sc))
    rounds, winner = 0, None
    while winner is None and rounds < 1000 and not st["no_more"].all():
        rounds += 1
        _, h = R.iterate(sc, pr, st, raw, 5, MIN_INLIERS, 1)
        hit = np.flatnonzero(h["n_hits"] > 0)
        if len(hit):
            winner = int(hit[0])
    assert winner is not None and lines[-1] == ["done", str(rounds), "1"]
    head, T, sim3, inl = _line(lines[1])
    wT, wsim3, winl, wn = _expect(h, winner)
    assert head[:2] == [winner, rounds] and head[3] == wn
    assert G.same_bits(T, wT) and G.same_bits(sim3, wsim3) and inl == winl

"""The C++ adapter ORB_SLAM2_PLF::LoopClosing::CorrectLoop (include/plf.hpp) over the mock KeyFrame / MapPoint / g2o::Sim3 of
tests/mock/ORB_SLAM2/mock_loopfix.h, driven by tests/cpp/loopfix_driver.cpp on the GPU: it walks the caller's real std::map<KeyFrame*, g2o::Sim3>, so the
rank order is the pointer order, and what it leaves in the objects -- both maps, the poses, the positions, the two marks, and the normal and depth it
returns -- equals the sequential definition tests/loopfixref.py bit for bit, with the keyframes laid out in ascending and in descending address order.
(The host loop tools/loopfix_cpu.cpp is compared with the definition in tests/test_loopfix_ref.py: it needs no GPU.)"""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cppbuild  # noqa: E402
import loopfixgen as G  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32


def _scene(reverse):
    """9 keyframes of which 6 are connected; every observation list in the order a std::map<KeyFrame*, size_t> iterates (by address: by slot, ascending or
    descending); rows of valid ids and nulls; unsigned marks (0: none)"""
    rng = np.random.default_rng(17)
    n_kf, n = 9, 120
    obs = [sorted((int(k) for k in rng.permutation(n_kf)[:rng.integers(1, 6)]), reverse=reverse) for _ in range(n)]
    ranks = sorted([7, 1, 4, 8, 2, 5], reverse=reverse)
    rows = []
    for r in range(len(ranks)):
        ids = [int(p) for p in rng.integers(0, n, [0, 1, 40, 64, 65, 30][r])]
        rows.append([-1 if i % 9 == 4 else p for i, p in enumerate(ids)])
    sc = G.make_scene(17, n_kf=n_kf, n_points=n, rank_kf=ranks, cur=4, rows=rows, obs=obs, n_bad=6, n_marked=5)
    sc["corrected_by"][sc["corrected_by"] < 0] = 0
    sc["corrected_ref"][sc["corrected_ref"] < 0] = 0
    assert sc["cur_kf_id"] > 0
    return sc


def _write(sc, reverse, path):
    with open(path, "w") as fh:
        fh.write("%d %d %d %d %s\n" % (reverse, sc["n_kf"], sc["n_points"], G.NLEVELS, cppbuild.hex32(sc["scale_factors"])))
        for k in range(sc["n_kf"]):
            fh.write("%d %s %s\n" % (sc["kf_id"][k], cppbuild.hex32(sc["kf_tcw"][k]), cppbuild.hex32(sc["kf_ow"][k])))
        for p in range(sc["n_points"]):
            s, e = sc["obs_start"][p], sc["obs_start"][p + 1]
            fh.write("%s %d %d %d %d %d %d %s\n" % (cppbuild.hex32(sc["world_pos"][p]), sc["point_bad"][p], sc["corrected_by"][p], sc["corrected_ref"][p], sc["ref_kf"][p],
                                                    sc["ref_level"][p], e - s, " ".join(str(k) for k in sc["obs_kf"][s:e])))
        fh.write("%d %d\n" % (len(sc["rank_kf"]), sc["cur_slot"]))
        for r, k in enumerate(sc["rank_kf"][::-1]):                        # (listed in the opposite order: the map, not the list, orders the walk)
            row = sc["rows"][len(sc["rank_kf"]) - 1 - r]
            fh.write("%d %d %s\n" % (k, len(row), " ".join(str(p) for p in row)))
        fh.write(cppbuild.hex64(sc["scw"]) + "\n")


@pytest.mark.parametrize("reverse", [0, 1])
def test_exact_class_adapter(tmp_path, reverse):
    sc = _scene(bool(reverse))
    ref = G.ref_run(sc)
    _write(sc, reverse, tmp_path / "scenario.txt")
    exe = cppbuild.build_driver("loopfix_driver", tmp_path, "-O1", "-Wall", "-Werror")
    subprocess.check_call([str(exe), str(tmp_path)], timeout=120)
    lines = [ln.split() for ln in open(tmp_path / "out.txt")]
    kl, pl = [ln for ln in lines if ln[0] == "K"], [ln for ln in lines if ln[0] == "P"]
    assert [int(ln[1]) for ln in kl] == list(sc["rank_kf"]) and len(pl) == sc["n_points"]
    for r, ln in enumerate(kl):
        d = np.array([int(w, 16) for w in ln[2:18]], np.uint64).view(np.float64)
        T = np.array([int(w, 16) for w in ln[18:30]], np.uint32).view(F32)
        assert G.same_bits(d[:8], ref["corrected"][r]).all() and G.same_bits(d[8:], ref["noncorrected"][r]).all(), r
        assert G.same_bits(T, ref["tcw_new"][r]).all(), r
    held = set(p for row in sc["rows"] for p in row if p >= 0)
    for p, ln in enumerate(pl):
        pos = np.array([int(w, 16) for w in ln[1:4]], np.uint32).view(F32)
        assert G.same_bits(pos, ref["world_pos"][p]).all(), p
        assert int(ln[4]) == ref["corrected_by"][p] and int(ln[5]) == ref["corrected_ref"][p], p
        if p not in held:
            assert ln[6:] == ["-1", "-1"] and ref["owner_rank"][p] == -1
            continue
        assert int(ln[6]) == ref["owner_rank"][p] and int(ln[7]) == ref["n_obs_used"][p], p
        if ref["n_obs_used"][p] > 0:
            v = np.array([int(w, 16) for w in ln[8:13]], np.uint32).view(F32)
            assert G.same_bits(v[:3], ref["normal"][p]).all() and G.same_bits(v[3:], np.array([ref["min_distance"][p], ref["max_distance"][p]], F32)).all(), p
    assert (ref["owner_rank"] >= 0).sum() > 60 and len(set(ref["owner_rank"])) >= 5

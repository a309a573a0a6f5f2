"""The C++ adapter ORB_SLAM2_PLF::Optimizer::OptimizeSim3 (include/plf.hpp), with the reference's exact signature, over the mock KeyFrame / MapPoint /
g2o::Sim3 of tests/mock/ORB_SLAM2/mock_sim3opt.h, driven by tests/cpp/sim3opt_driver.cpp on the GPU: the return value, g2oS12 and the nulled matches of
every candidate equal tests/sim3optref.py bit for bit.  The start g2oS12 is built as LoopClosing::ComputeSim3 builds it -- Quaterniond of the float
rotation --, and the definition is given the floats the adapter narrows it to."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cppbuild  # noqa: E402
import sim3optgen as G  # noqa: E402
import sim3optref as R  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32


def _scene():
    jobs = [dict(n1=70, pairs=50, outliers=0.3, null=3, bad=4, noobs=3), dict(n1=40, pairs=24, fix_scale=True), dict(n1=30, pairs=12, outliers=0.3),
            dict(n1=50, pairs=30, scale=1.25, off_s=1.04, off_deg=10.0)]
    return G.make_scene(93, jobs, obs_index=True)


def _write(sc, starts, path):
    J = len(sc["job_kf1"])
    with open(path, "w") as fh:
        fh.write("%s\n%s\n%d %s\n%d\n" % (cppbuild.hex32([sc["th2"]]), cppbuild.hex32(sc["cam"][:4]), len(sc["inv_level_sigma2"]), cppbuild.hex32(sc["inv_level_sigma2"]), J))
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
                    fh.write("%s %d %d %d\n" % (cppbuild.hex32(sc["kf_keys"][s][i, :2]), sc["kf_octave"][s][i], mp - base if mp >= 0 else -1, sc["kf_obs_index"][s][i]))
            n1 = sc["kf_n"][s1]
            fh.write("%d\n" % n1)
            for i1 in range(n1):
                i2 = sc["match12"][j, i1]
                mp = sc["kf_mappoints"][s2][i2] if i2 >= 0 else -1
                fh.write("%d\n" % (mp - base if mp >= 0 else -1))
            fh.write(cppbuild.hex64(starts[j]) + "\n")


def test_exact_signature_adapter(tmp_path):
    sc = _scene()
    J = len(sc["job_kf1"])
    # g2oS12 as ComputeSim3 makes it; the adapter narrows it to floats: rotation().toRotationMatrix(), translation(), scale()
    starts, narrowed = [], np.zeros((J, 13), F32)
    for j in range(J):
        est = R.sim3_from_rts(sc["sim3_in"][j][:9], sc["sim3_in"][j][9:12], sc["sim3_in"][j][12])
        starts.append(R.sim3_out8(est))
        Rm = R.P.quat_to_matrix(est[0])
        narrowed[j] = [R.P.f32(Rm[i][k]) for i in range(3) for k in range(3)] + [R.P.f32(v) for v in est[1]] + [R.P.f32(est[2])]
    _write(sc, starts, tmp_path / "scenario.txt")
    exe = cppbuild.build_driver("sim3opt_driver", tmp_path, "-O1", "-Wall", "-Werror")
    subprocess.check_call([str(exe), str(tmp_path)], timeout=120)
    lines = [ln.split() for ln in open(tmp_path / "out.txt")]
    assert len(lines) == J
    # in the adapter a point's observation index IS the slot the match names: the scene's kf_obs_index of keyframe 2 is the identity but for the absent ones
    ref = R.run(sc, sim3_in=narrowed)
    assert (ref["status"] == 0).sum() >= 2 and (ref["status"] == R.FEW).sum() >= 1
    for j, ln in enumerate(lines):
        bar = ln.index("|")
        got = np.array([int(w, 16) for w in ln[1:bar]], np.uint64).view(np.float64)
        want = np.array(starts[j]) if ref["status"][j] & R.FEW else ref["sim3"][j]
        assert int(ln[0]) == ref["n_inliers"][j], j
        assert G.same_doubles(got, want), (j, got, want)
        nulled = sorted(int(w) for w in ln[bar + 1:])
        assert nulled == np.flatnonzero((sc["match12"][j] >= 0) & (ref["match12"][j] < 0)).tolist(), j

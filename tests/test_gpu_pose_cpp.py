"""The C++ mirror ORB_SLAM2_PLF::Optimizer::PoseOptimization(Frame*) (include/plf.hpp) on the GPU: tests/cpp/pose_driver.cpp over the mock Frame / MapPoint of
tests/mock/ORB_SLAM2/mock_pose.h gives, on tests/golden/pose_tiny.json, the bits the definition tests/poseref.py recorded there -- return value, pose
(SetPose) and mvbOutlier, with the flags of unmatched key points left as the frame had them."""
import json
import os
import subprocess

import numpy as np
import pytest

import cppbuild
from conftest import gpu_available

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _need_gpu():
    if not gpu_available():
        pytest.fail("no GPU visible: the -m gpu tests need a real MI355X")


def test_cpp_driver_gives_the_recorded_bits(tmp_path):
    with open(os.path.join(ROOT, "tests", "golden", "pose_tiny.json")) as fh:
        doc = json.load(fh)
    exe = cppbuild.build_driver("pose_driver", tmp_path, "-O1", "-Wall")
    before = []
    lines = [cppbuild.hex32(doc["cam"]), "%d %s" % (len(doc["inv_level_sigma2"]), cppbuild.hex32(doc["inv_level_sigma2"])),
             str(len(doc["frames"]))]
    for fr in doc["frames"]:
        n = len(fr["match"])
        flags = [(7 * i + 3) % 2 for i in range(n)]                 # what the frame holds before the call
        before.append(flags)
        lines.append(str(n))
        lines.append(cppbuild.hex32(fr["tcw_init"]))
        for i in range(n):
            m = fr["match"][i]
            pt = cppbuild.hex32(fr["world_pos"][3 * m:3 * m + 3]) if m >= 0 else ""
            lines.append("%s %s %s %d %d %d %s" % (cppbuild.hex32(fr["x"][i]), cppbuild.hex32(fr["y"][i]), cppbuild.hex32(fr["uright"][i]), fr["octave"][i], flags[i], int(m >= 0), pt))
    (tmp_path / "scenario.txt").write_text("\n".join(lines) + "\n")
    run = subprocess.run([str(exe), str(tmp_path)], text=True, capture_output=True)
    assert run.returncode == 0 and "pose driver ok" in run.stdout, "driver failed (rc %d)\n%s\n%s" % (run.returncode, run.stdout, run.stderr[-2000:])
    got = (tmp_path / "out.txt").read_text().split("\n")
    for k, fr in enumerate(doc["frames"]):
        ret, pose, flags = got[3 * k].split(), got[3 * k + 1].split(), got[3 * k + 2].split()
        early = fr["status"] == 1
        assert int(ret[1]) == fr["n_inliers"], k
        want_pose = [int(np.float32(v).view(np.uint32)) for v in fr["tcw_init"]] if early else fr["pose_bits"]
        assert [int(v) for v in pose[1:]] == want_pose, k
        want = [before[k][i] if (early or fr["match"][i] < 0) else fr["outlier"][i] for i in range(len(fr["match"]))]
        assert [int(v) for v in flags[1:]] == want, k

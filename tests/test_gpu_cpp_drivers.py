"""The C++ drivers of the map-stage adapters (include/plf.hpp) on the GPU, each over its hand-worked fixture with the keyframes' addresses as keys, laid
out so that address order is the fixture's order:
  normal  tests/cpp/normal_driver.cpp: ORB_SLAM2_PLF::UpdateNormalAndDepth over the mock KeyFrame / MapPoint of tests/mock/ORB_SLAM2/mock_normal.h --
          the list call, and the one-point forwarder a MapPoint.cc would carry
  covis   tests/cpp/covis_driver.cpp: ORB_SLAM2_PLF::CovisibilityGraph over the mock KeyFrame / MapPoint / Frame of tests/mock/ORB_SLAM2/mock_covis.h --
          UpdateConnections for every keyframe in one call, GetConnectedKeyFrames, GetBestCovisibilityKeyFrames, GetCovisiblesByWeight, the parent
          candidate and the votes of UpdateLocalKeyFrames"""
import subprocess

import pytest

import normref
import test_covis_ref
import test_normal_ref
from conftest import gpu_available

pytestmark = pytest.mark.gpu

DRIVERS = {
    "normal": (test_normal_ref.build_normal_driver, lambda path: test_normal_ref.driver_scenario(normref.load_fixture(test_normal_ref.FIXTURE), path)),
    "covis": (test_covis_ref.build_covis_driver, lambda path: test_covis_ref.driver_scenario(test_covis_ref.load_fixture(), path)),
}


@pytest.fixture(autouse=True)
def _need_gpu():
    if not gpu_available():
        pytest.fail("no GPU visible: the -m gpu tests need a real MI355X")


@pytest.mark.parametrize("name", sorted(DRIVERS))
def test_cpp_driver_equals_the_hand_worked_fixture(tmp_path, name):
    build, scenario = DRIVERS[name]
    exe = build(tmp_path, flags=("-O1",))
    expect = scenario(str(tmp_path / "scenario.txt"))
    run = subprocess.run([str(exe), str(tmp_path)], text=True, capture_output=True)
    assert run.returncode == 0 and name + " driver ok" in run.stdout, "driver failed (rc %d)\n%s\n%s" % (run.returncode, run.stdout, run.stderr[-2000:])
    got = open(str(tmp_path / "out.txt")).read().split("\n")[:-1]
    assert got == expect, [(i, g, e) for i, (g, e) in enumerate(zip(got, expect)) if g != e][:5]

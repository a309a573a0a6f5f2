"""tests/cpp/normal_driver.cpp on the GPU: ORB_SLAM2_PLF::UpdateNormalAndDepth (include/plf.hpp) over the mock KeyFrame / MapPoint of
tests/mock/ORB_SLAM2/mock_normal.h runs the hand-worked fixture -- the list call, and the one-point forwarder a MapPoint.cc would carry -- with the
keyframes' addresses as keys, laid out so that address order is the fixture's observation order."""
import subprocess

import pytest

import normref
from conftest import gpu_available
from test_normal_ref import FIXTURE, build_normal_driver, driver_scenario

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _need_gpu():
    if not gpu_available():
        pytest.fail("no GPU visible: the -m gpu tests need a real MI355X")


def test_cpp_driver_equals_the_hand_worked_fixture(tmp_path):
    exe = build_normal_driver(tmp_path, flags=("-O1",))
    expect = driver_scenario(normref.load_fixture(FIXTURE), str(tmp_path / "scenario.txt"))
    run = subprocess.run([str(exe), str(tmp_path)], text=True, capture_output=True)
    assert run.returncode == 0 and "normal driver ok" in run.stdout, "driver failed (rc %d)\n%s\n%s" % (run.returncode, run.stdout, run.stderr[-2000:])
    got = open(str(tmp_path / "out.txt")).read().split("\n")[:-1]
    assert got == expect, [(i, g, e) for i, (g, e) in enumerate(zip(got, expect)) if g != e][:5]

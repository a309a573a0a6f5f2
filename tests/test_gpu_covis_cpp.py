"""tests/cpp/covis_driver.cpp on the GPU: ORB_SLAM2_PLF::CovisibilityGraph (include/plf.hpp) over the mock KeyFrame / MapPoint / Frame of
tests/mock/ORB_SLAM2/mock_covis.h runs the hand-worked fixture through the mirror's methods -- UpdateConnections for every keyframe in one call,
GetConnectedKeyFrames, GetBestCovisibilityKeyFrames, GetCovisiblesByWeight, the parent candidate and the votes of UpdateLocalKeyFrames -- with the
keyframes' addresses as keys, laid out so that address order is the fixture's key order."""
import subprocess

import pytest

from conftest import gpu_available
from test_covis_ref import build_covis_driver, driver_scenario, load_fixture

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _need_gpu():
    if not gpu_available():
        pytest.fail("no GPU visible: the -m gpu tests need a real MI355X")


def test_cpp_driver_equals_the_hand_worked_fixture(tmp_path):
    exe = build_covis_driver(tmp_path, flags=("-O1",))
    expect = driver_scenario(load_fixture(), str(tmp_path / "scenario.txt"))
    run = subprocess.run([str(exe), str(tmp_path)], text=True, capture_output=True)
    assert run.returncode == 0 and "covis driver ok" in run.stdout, "driver failed (rc %d)\n%s\n%s" % (run.returncode, run.stdout, run.stderr[-2000:])
    got = open(str(tmp_path / "out.txt")).read().split("\n")[:-1]
    assert got == expect, [(i, g, e) for i, (g, e) in enumerate(zip(got, expect)) if g != e][:5]

"""The C++ driver of the culling adapter (include/plf.hpp, ORB_SLAM2_PLF::KeyFrameCulling) on the GPU: tests/cpp/culling_driver.cpp over the mock
KeyFrame / MapPoint of tests/mock/ORB_SLAM2/mock_culling.h and the hand-worked fixture tests/golden/culling_tiny.json -- the decisions, the erase list,
and the map after the mock's own KeyFrame::SetBadFlag has run on that list (what a LocalMapping.cc forwarder does with the result)."""
import subprocess

import pytest

import cullref
import test_culling_ref as R
from conftest import gpu_available

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _need_gpu():
    if not gpu_available():
        pytest.fail("no GPU visible: the -m gpu tests need a real MI355X")


@pytest.mark.parametrize("monocular,max_culls", [(0, 0), (1, 0), (0, 1)])
def test_cpp_driver_equals_the_hand_worked_fixture(tmp_path, monocular, max_culls):
    exe = R.build_culling_driver(tmp_path, flags=("-O1",))
    fx = cullref.load_fixture()
    expect = R.driver_scenario(fx, str(tmp_path / "scenario.txt"), monocular, max_culls)
    run = subprocess.run([str(exe), str(tmp_path)], text=True, capture_output=True)
    assert run.returncode == 0 and "culling driver ok" in run.stdout, "driver failed (rc %d)\n%s\n%s" % (run.returncode, run.stdout, run.stderr[-2000:])
    got = open(str(tmp_path / "out.txt")).read().split("\n")[:-1]
    assert got == expect, [(i, g, e) for i, (g, e) in enumerate(zip(got, expect)) if g != e][:5]
    want = fx["monocular_sequential" if monocular else "sequential"]
    assert [int(line.split()[4]) for line in got if line.startswith("cand")] == want["decision"]

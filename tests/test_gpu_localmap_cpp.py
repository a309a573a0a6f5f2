"""The C++ driver of the local-map adapter (include/plf.hpp, ORB_SLAM2_PLF::UpdateLocalMap over plf::LocalMap) on the GPU: tests/cpp/localmap_driver.cpp
over the mock KeyFrame / MapPoint / Frame of tests/mock/ORB_SLAM2/mock_localmap.h and the fixture tests/golden/localmap_tiny.json -- mvpLocalKeyFrames,
mpReferenceKF, mvpLocalMapPoints, the seen flags and the frame's own row after the bad points are set to null, as the mock's restatement recorded them."""
import subprocess

import pytest

import test_localmap_ref as R
from conftest import gpu_available

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _need_gpu():
    if not gpu_available():
        pytest.fail("no GPU visible: the -m gpu tests need a real MI355X")


@pytest.mark.parametrize("stream", [False, True])
def test_cpp_driver_equals_what_the_mock_recorded(tmp_path, stream):
    """stream: the adapter's device work -- the votes, plf::LocalMap::Update with its list fills, the item pass -- on a non-blocking stream the driver makes,
    frame after frame, instead of the null stream"""
    flags = ("-O1", "-DLOCALMAP_DRIVER_STREAM", "-Wl,--no-as-needed", "-L/opt/rocm/lib", "-lamdhip64") if stream else ("-O1",)
    exe = R.build_localmap_driver(tmp_path, flags=flags)
    expect = R.driver_expect(R.load_fixture(), str(tmp_path / "scenario.txt"))
    run = subprocess.run([str(exe), str(tmp_path)] + (["stream"] if stream else []), text=True, capture_output=True)
    assert ("on a stream of its own" in run.stdout) == stream, run.stdout
    assert run.returncode == 0 and "localmap driver ok" in run.stdout, "driver failed (rc %d)\n%s\n%s" % (run.returncode, run.stdout, run.stderr[-2000:])
    got = R.parse_out(open(str(tmp_path / "out.txt")).read())
    assert got == expect, [(g, e) for g, e in zip(got, expect) if g != e][:1]
    assert [len(g["kfs"]) for g in got] == [7, 82, 82, 81]

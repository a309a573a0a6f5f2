"""The C++ mirrors ORB_SLAM2_PLF::Tracking::CreateNewKeyFrame / UpdateLastFrame / NeedNewKeyFrame (include/plf.hpp) on the GPU: tests/cpp/track_driver.cpp
over the mock classes of tests/mock/ORB_SLAM2/mock_track.h gives, on tests/golden/track_tiny.json, what the definition tests/trackref.py recorded there --
the MapPoints made in the definition's order with its positions and stored in mvpMapPoints, and the decisions with InterruptBA() and the queue test
following on the host."""
import json
import os
import subprocess

import pytest

import cppbuild
from conftest import gpu_available

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _need_gpu():
    if not gpu_available():
        pytest.fail("no GPU visible: the -m gpu tests need a real MI355X")


def scenario(doc):
    """the driver's input and what it has to print, from the golden file"""
    hx = lambda bits: " ".join("%x" % b for b in bits)
    S = 64
    lines = [hx(doc["cam"]), hx(doc["th_depth"]), str(doc["min_points"]), "%d %s" % (len(doc["n_obs"]), " ".join(str(v) for v in doc["n_obs"])), str(len(doc["n"]))]
    want = []
    at = 0
    for f, n in enumerate(doc["n"]):
        lines.append("%d %d %s" % (f % 2, n, hx(doc["frustum"][15 * f:15 * f + 15])))
        for i in range(n):
            q = f * S + i
            lines.append("%x %x %x %d" % (doc["keys_x"][q], doc["keys_y"][q], doc["depth"][q], doc["match"][q]))
        k = doc["out"]["n_new"][f]
        row = ["made", str(k), str(k)]
        for j in range(k):
            row += [str(doc["out"]["new_kp"][f * S + j]), "1"] + [str(b) for b in doc["out"]["new_pos"][(f * S + j) * 3:(f * S + j) * 3 + 3]]
        want.append(" ".join(row))
        at += n
    rows = doc["decide"]
    lines.append(str(2 * len(rows)))
    for queue in (1, 3):
        for s, inl, nt, nm, nr, dec in rows:
            lines.append("%d %d %d %d %d %d %d %d %d %d %d %d" % (s["frame_id"], inl, s["last_kf_id"], s["last_reloc_frame_id"], s["min_frames"], s["max_frames"], s["n_kfs"],
                                                                 s["flags"], queue, nt, nm, nr))
            mono = bool(s["flags"] & 8)
            need = dec == 1 or (dec == 2 and not mono and queue < 3)
            want.append("need %d %d" % (int(need), int(dec == 2)))
    return lines, want


def test_cpp_driver_gives_the_recorded_results(tmp_path):
    with open(os.path.join(ROOT, "tests", "golden", "track_tiny.json")) as fh:
        doc = json.load(fh)
    lines, want = scenario(doc)
    assert sum(w.startswith("need 1") for w in want) > 2 and sum(w.endswith(" 1") and w.startswith("need 0") for w in want) > 0
    exe = cppbuild.build_driver("track_driver", tmp_path, "-O1", "-Wall")
    (tmp_path / "scenario.txt").write_text("\n".join(lines) + "\n")
    run = subprocess.run([str(exe), str(tmp_path)], text=True, capture_output=True)
    assert run.returncode == 0 and "track driver ok" in run.stdout, "driver failed (rc %d)\n%s\n%s" % (run.returncode, run.stdout, run.stderr[-2000:])
    got = (tmp_path / "out.txt").read_text().strip().split("\n")
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, (k, g, w)

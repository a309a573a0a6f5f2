"""The reference-signature adapter ORB_SLAM2_PLF::LocalMapping::CreateNewMapPoints (include/plf.hpp) on the GPU: tests/cpp/triangulate_driver.cpp over the mock
classes of tests/mock/ORB_SLAM2/mock_triangulate.h -- GetBestCovisibilityKeyFrames, the caller's ComputeF12, the device search and the device triangulation
per neighbour, then new MapPoint / AddObservation / AddMapPoint / mlpRecentAddedMapPoints on the host -- creates the same points, in the same order and with
the same ids, as the whole-function form of the definition (tests/triref.py create_new_map_points, its search the oracle's)."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cppbuild  # noqa: E402
import kfgen  # noqa: E402
import orc  # noqa: E402
import trigen as G  # noqa: E402
import triref as R  # noqa: E402
from conftest import gpu_available  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(autouse=True)
def _need_gpu():
    if not gpu_available():
        pytest.fail("no GPU visible: the -m gpu tests need a real MI355X")


def hx(a):
    return " ".join("%x" % b for b in np.ascontiguousarray(a, F32).view(np.uint32).reshape(-1))


def case(n=400):
    """one current keyframe and two neighbours that see the same world points: (current, neighbours, their scenes)"""
    ca, cb = kfgen.two_keyframe_scene(5, n, nodes=50, tz=0.05), kfgen.two_keyframe_scene(5, n, nodes=50, tz=0.4)
    for k in ("kps1", "desc1", "uright1", "has_mp1"):
        assert np.array_equal(ca[k], cb[k])
    bf = ca["pose1"]["bf"]

    def kf_of(c, sfx):
        p = c["pose" + sfx]
        kf = G.keyframe(n, np.concatenate([p["Rcw"].reshape(-1), p["tcw"], p["Ow"]]).astype(F32))
        kf["keys"], kf["uright"] = c["kps" + sfx], c["uright" + sfx]
        with np.errstate(all="ignore"):
            kf["depth"] = np.where(kf["uright"] >= 0, F32(bf) / (kf["keys"]["x"] - kf["uright"]), -1).astype(F32)
        kf["has_mp"] = c["has_mp" + sfx].copy()
        kf["desc"], kf["c"] = c["desc" + sfx], c
        nd = np.zeros(n, np.uint32)
        ids, starts, feats = c["nodes" + sfx]
        for q, k in enumerate(ids):
            nd[feats[starts[q]:starts[q + 1]]] = k
        kf["node"] = nd
        return kf
    return kf_of(ca, "1"), [kf_of(ca, "2"), kf_of(cb, "2")], ca


def test_cpp_adapter_creates_the_definitions_points_in_its_order(tmp_path):
    cur, nbs, ca = case()
    bf = ca["pose1"]["bf"]
    mb = float(F32(bf) / F32(ca["fx"]))
    lines = [hx([ca["fx"], ca["fy"], ca["cx"], ca["cy"], bf, mb, 1.2]), str(len(ca["scale"])), hx(ca["scale"]), hx(ca["sigma2"]), "3"]
    for kf in [cur] + nbs:
        lines.append(hx(kf["pose"]))
        lines.append(hx(kf["c"]["F12"]))
        lines.append(str(kf["n"]))
        for i in range(kf["n"]):
            k = kf["keys"][i]
            lines.append("%s %d %s %d %d %s" % (hx([k["x"], k["y"], k["angle"]]), k["octave"], hx([kf["uright"][i], kf["depth"][i]]), kf["has_mp"][i], kf["node"][i],
                                                "".join("%02x" % b for b in kf["desc"][i])))

    def search(cur_kf, nb):                                        # ORBmatcher matcher(0.6, false); SearchForTriangulation(..., false)
        return orc.search_for_triangulation(dict(nb["c"], has_mp1=cur_kf["has_mp"], has_mp2=nb["has_mp"], only_stereo=0, check=0))[0]
    cam = R.camera((ca["fx"], ca["fy"], ca["cx"], ca["cy"]), mb, bf, 1.2)
    want_jobs = R.create_new_map_points(cur, nbs, search, cam, ca["scale"], ca["sigma2"], next_id=7000)
    assert len(want_jobs[0]["i1"]) > 50 and len(want_jobs[1]["i1"]) > 5
    want, next_id = [], 7000
    for r, w in enumerate(want_jobs):
        for k, (i1, i2) in enumerate(zip(w["i1"], w["i2"])):
            want.append("mp %d %d %d %d %s" % (next_id, r + 1, i1, i2, " ".join(str(b) for b in w["pos"][k].view(np.uint32))))
            next_id += 1
    total = next_id - 7000
    want.append("made %d %d %s" % (total, total, " ".join(str(int(kf["has_mp"].sum())) for kf in [cur] + nbs)))
    exe = cppbuild.build_driver("triangulate_driver", tmp_path, "-O1", "-Wall")
    (tmp_path / "scenario.txt").write_text("\n".join(lines) + "\n")
    run = subprocess.run([str(exe), str(tmp_path)], text=True, capture_output=True)
    assert run.returncode == 0 and "triangulate driver ok" in run.stdout, "driver failed (rc %d)\n%s\n%s" % (run.returncode, run.stdout, run.stderr[-2000:])
    got = (tmp_path / "out.txt").read_text().strip().split("\n")
    assert len(got) == len(want), (len(got), len(want))
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, (k, g, w)

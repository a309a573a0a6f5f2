"""plf_triangulate_points on the device against the definition tests/triref.py, BIT FOR BIT: positions (every float as its uint32 view), the lists, the
counts, the reason bytes, the status words and the in-place marks.  No tolerance and no excluded case; a NaN compares equal to any NaN."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import trigen as G  # noqa: E402
import triref as R  # noqa: E402
import test_tri_ref as T  # noqa: E402

import torch  # noqa: E402
from conftest import gpu_available  # noqa: E402

pytestmark = pytest.mark.gpu

from rgbd_pl_slam_amd import _lib as L  # noqa: E402
from rgbd_pl_slam_amd import triangulate_points, KeyFrameSet  # noqa: E402

SIDE, FORWARD = (-0.25, 0.02, 0.03), (0.01, -0.01, -1.0)


@pytest.fixture(autouse=True)
def _need_gpu():
    if not gpu_available():
        pytest.fail("no GPU visible: the -m gpu tests need a real MI355X")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def check(sc, what, **kw):
    want = G.ref_call(sc, **kw)
    got = G.dev_call(sc, **kw)
    G.assert_equal(got, want, what)
    for j in range(len(want["n_new"])):                          # nothing is written beyond min(count, stride)
        k = min(int(want["n_new"][j]), got["new_i1"].shape[1])
        assert np.all(got["new_i1"][j, k:] == -1) and np.all(got["new_i2"][j, k:] == -1) and not got["new_pos"][j, k:].any(), what
    return want


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_key_point_counts_at_the_wave_and_chunk_edges(n):
    """one job whose keyframes have n key points, half of them paired: the edges of the ballot prefix (64) and of the chunk scan (256)"""
    a, b, m = G.pair_scene(500 + n, n, n, max(1, n // 2), SIDE)
    want = check(G.scene_of([(a, b, m)]), "n=%d" % n)
    assert n < 63 or want["n_new"][0] > 0
    a, b, m = G.pair_scene(600 + n, n, max(1, n - 1), n, FORWARD, pass_through=min(20, n // 3), z_range=(1.5, 7.0))     # every key point paired, the stereo branches
    check(G.scene_of([(a, b, m)]), "n=%d forward" % n)


@pytest.mark.parametrize("jobs", [1, 2, 70])
def test_jobs_of_mixed_sizes_in_one_call(jobs):
    rng = np.random.default_rng(jobs)
    prs = []
    for j in range(jobs):
        n1, n2 = int(rng.integers(1, 140)), int(rng.integers(1, 140))
        prs.append(G.pair_scene(700 + 100 * jobs + j, n1, n2, int(rng.integers(0, n1 + 1)), (SIDE, FORWARD, (-0.08, 0.01, 0.02))[j % 3], pass_through=3 if j % 3 == 1 and min(n1, n2) > 6 else 0))
    sc = G.scene_of(prs)
    want = check(sc, "%d jobs" % jobs, mark_has_mp=True, id_base=(1000 * np.arange(jobs)).tolist())
    assert want["n_new"].sum() > 0
    if jobs == 70:
        assert len(set(want["n_new"].tolist())) > 10 and (want["n_new"] == 0).any()


def test_the_standard_scene():
    """every reason code and branch, a skipped job, an infinite pose, invalid depths, i2 beyond keyframe 2, two jobs over one pair of slots"""
    sc = G.standard_scene()
    want = check(sc, "standard")
    G.reason_counts_ok(want)


def test_all_pairs_matched_and_no_pair_matched():
    a, b, m = G.pair_scene(801, 200, 200, 200, SIDE)
    assert (m >= 0).all()
    want = check(G.scene_of([(a, b, m)]), "all matched")
    assert want["n_new"][0] > 50
    a, b, m = G.pair_scene(802, 200, 200, 0, SIDE)
    want = check(G.scene_of([(a, b, m)]), "none matched")
    assert want["n_new"][0] == 0 and np.all(want["reason"][0] == R.NO_PAIR)


def test_all_pairs_in_the_svd_branch_and_none_in_it():
    """the edges of the dense-lane compaction: 300 pairs that all take the linear triangulation (more than a chunk's 256 lanes of them in a row), and a
    job in which no pair does"""
    a, b, m = G.pair_scene(803, 300, 300, 300, (-0.5, 0.0, 0.0), stereo_frac=1.0, far_frac=0.0, mismatch=0.0, bad_depth=0.0)
    want = check(G.scene_of([(a, b, m)]), "all SVD")
    assert np.all(want["reason"][0] >> 4 == 1)
    a, b, m = G.pair_scene(804, 300, 300, 300, (0.0, 0.0, -0.09), rot2=0.0, stereo_frac=1.0, far_frac=0.0, mismatch=0.0, bad_depth=0.0, z_range=(0.5, 3.0), noise_px=0.05)
    first = G.ref_call(G.scene_of([(a, b, m)]))
    m[first["reason"][0] >> 4 == 1] = -1                               # (a few key points at the left edge have uRight < 0 and are monocular: unpaired here)
    want = check(G.scene_of([(a, b, m)]), "no SVD")
    assert not np.any(want["reason"][0] >> 4 == 1) and np.sum(want["reason"][0] >> 4 == 2) > 100


def test_short_list_overflow_and_marks_below_the_stride():
    prs = [G.pair_scene(805 + j, 300, 280, 200, SIDE) for j in range(3)]
    sc = G.scene_of(prs)
    full = G.ref_call(sc)
    assert full["n_new"].min() > 40
    want = check(sc, "short", new_stride=40, mark_has_mp=True, id_base=[10, 2000, 30000])
    assert np.all(want["status"] == R.OVERFLOW) and np.array_equal(want["n_new"], full["n_new"])
    for j in range(3):
        assert int(want["has_mp"][2 * j].sum()) == 40 and int((want["mappoints"][2 * j + 1] >= 0).sum()) == 40
    check(sc, "stride 1", new_stride=1)


def test_skipped_jobs_bad_slots_and_i2_out_of_range():
    prs = [G.pair_scene(810, 100, 100, 60, SIDE), G.pair_scene(811, 100, 100, 60, (0.01, 0.0, 0.01)), G.pair_scene(812, 100, 90, 60, SIDE)]
    m = prs[2][2]
    m[np.nonzero(m >= 0)[0][::3]] = [90, 91, 1000, 2 ** 31 - 1] * 5
    sc = G.scene_of(prs)
    for k1, k2 in ((-1, 1), (0, 6), (6, 0), (2 ** 31 - 1, -2 ** 31)):
        G.add_job(sc, k1, k2, prs[0][2])
    want = check(sc, "skips", mark_has_mp=True)
    assert want["status"].tolist() == [0, R.SKIPPED_BASELINE, 0] + [R.BAD_SLOT] * 4 and not want["n_new"][3:].any() and not want["reason"][3:].any()
    assert int(np.sum(want["reason"][2] == R.BAD_I2)) == 20
    # the same baseline is not skipped under a smaller mb, and every job is under a NaN one (mb > baseline is false)
    for mb in (0.001, float("nan")):
        cam = R.camera(G.CAM, mb, G.CAM[4], G.SCALE_FACTOR)
        want = G.ref_call(sc, cam=cam)
        got = G.dev_call(sc, mb=mb)
        G.assert_equal(got, want, "mb %r" % mb)
        assert want["status"][1] == 0


def test_nan_and_inf_in_poses_depths_and_key_points():
    prs = [G.pair_scene(820 + j, 150, 150, 100, (SIDE, FORWARD)[j % 2]) for j in range(6)]
    bad = np.array([np.nan, np.inf, -np.inf, 3.0e38, -0.0, 1e-45], np.float32)
    rng = np.random.default_rng(9)
    prs[0][0]["pose"][4] = np.nan                                  # Rcw of keyframe 1
    prs[1][1]["pose"][10] = np.nan                                 # tcw of keyframe 2: the SVD pairs come out NaN, and a NaN passes every test
    prs[2][0]["pose"][13] = np.nan                                 # Ow: the baseline is NaN, the job is not skipped
    prs[2][1]["pose"][9] = np.inf                                  # and x3D[3] == 0 in its SVD pairs
    prs[3][1]["pose"][:] = 0.0
    for a, b, _m in prs[3:]:
        for kf in (a, b):
            for arr in (kf["depth"], kf["uright"], kf["keys"]["x"], kf["keys"]["y"]):
                arr[rng.choice(kf["n"], 25, replace=False)] = rng.choice(bad, 25)
            kf["keys"]["octave"][rng.choice(kf["n"], 10, replace=False)] = [-1, 8, 100, -2 ** 31, 2 ** 31 - 1] * 2
    want = check(G.scene_of(prs), "non-finite")
    assert want["n_new"][3:].sum() > 20 and np.isnan(want["new_pos"]).any()


def test_bad_arguments_are_refused_with_a_device_present():
    for label, st in T.bad_argument_calls(L.lib()):
        assert st == L.PLF_E_BADARG, label


def test_two_neighbours_searched_and_triangulated_in_order_on_one_stream():
    """the reference's neighbour loop for one keyframe: (SearchForTriangulation, CreateNewMapPoints' body) for neighbour a, then for neighbour b, enqueued on one
    stream with the marks on, so that b's search sees the map points a's pairs created -- against the sequential loop of the definition, whose search is the
    oracle's (tests/orc.py, pinned to the reference binary)."""
    import kfgen
    import orc
    from rgbd_pl_slam_amd import Matcher
    n = 800
    ca, cb = kfgen.two_keyframe_scene(5, n, nodes=50, tz=0.05), kfgen.two_keyframe_scene(5, n, nodes=50, tz=0.4)
    for k in ("kps1", "desc1", "uright1", "has_mp1"):
        assert np.array_equal(ca[k], cb[k])                          # one current keyframe, two neighbours
    cam4 = (ca["fx"], ca["fy"], ca["cx"], ca["cy"])
    bf = ca["pose1"]["bf"]
    mb = float(np.float32(bf) / np.float32(ca["fx"]))

    def kf_of(c, sfx):
        kf = G.keyframe(n, np.concatenate([c["pose" + sfx]["Rcw"].reshape(-1), c["pose" + sfx]["tcw"], c["pose" + sfx]["Ow"]]).astype(np.float32))
        kf["keys"], kf["uright"] = c["kps" + sfx], c["uright" + sfx]
        with np.errstate(all="ignore"):
            kf["depth"] = np.where(kf["uright"] >= 0, np.float32(bf) / (kf["keys"]["x"] - kf["uright"]), -1).astype(np.float32)
        kf["has_mp"] = c["has_mp" + sfx].copy()
        return kf
    cur, nbs = kf_of(ca, "1"), [kf_of(ca, "2"), kf_of(cb, "2")]
    nbs[0]["c"], nbs[1]["c"] = ca, cb

    def search(cur_kf, nb):
        c = dict(nb["c"], has_mp1=cur_kf["has_mp"], has_mp2=nb["has_mp"], only_stereo=0, check=1)
        return orc.search_for_triangulation(c)[0]
    cam = R.camera(cam4, mb, bf, 1.2)
    ref_cur = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in cur.items()}
    ref_nbs = [{k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in nb.items()} for nb in nbs]
    want = R.create_new_map_points(ref_cur, ref_nbs, search, cam, ca["scale"], ca["sigma2"], next_id=7000)
    assert len(want[0]["i1"]) > 50 and len(want[1]["i1"]) > 10
    # the second search is not the one an unmarked keyframe would get: most of its pairs went to the first neighbour, so the marks matter
    assert int((search(cur, nbs[1]) >= 0).sum()) > 3 * int((want[1]["reason"] != R.NO_PAIR).sum())

    sc = dict(slots=[cur] + nbs)
    kfs = G.dev_keyframes(sc)
    mt = Matcher(max_keypoints=4096, max_mappoints=4096)
    ds, dsg = dev(ca["scale"]), dev(ca["sigma2"])
    st = torch.cuda.Stream()
    dkf, keep = [], []
    for slot, (c, sfx) in enumerate(((ca, "1"), (ca, "2"), (cb, "2"))):
        dd = dev(c["desc" + sfx])
        nodes = tuple(dev(x) for x in c["nodes" + sfx])
        keep += [dd, nodes]
        dkf.append(dict(keys=kfs.keep[0][slot], uright=kfs.keep[1][slot], desc=dd, has_mp=kfs.keep[3][slot], nodes=nodes, scale_factors=ds, level_sigma2=dsg))
    results = []
    id_base = dev(np.array([7000], np.int32))
    match = [torch.full((1, n), -7, dtype=torch.int32, device="cuda") for _ in range(2)]
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    one = dev(np.zeros(1, np.int32))
    for r, c in enumerate((ca, cb)):
        mt.SearchForTriangulation(dkf[0], dkf[1 + r], c["F12"], c["Ow1"], c["pose2"], 0, 1, match[r], cnt, stream=st.cuda_stream)
        # id_base of the second call is the first call's plus its count, added on the device under the same stream: nothing is read back in between
        results.append(triangulate_points(kfs, one, dev(np.array([1 + r], np.int32)), match[r], cam4 + (bf,), mb, ds, dsg, scale_factor=1.2, mark_has_mp=True,
                                          id_base=id_base, stream=st.cuda_stream))
        keep.append(id_base)                                         # (in flight on st: not to be handed back to the allocator yet)
        with torch.cuda.stream(st):
            id_base = id_base + torch.clamp(results[r].n_new, max=n)
    st.synchronize()
    torch.cuda.synchronize()
    for r in range(2):
        k = len(want[r]["i1"])
        assert int(results[r].n_new[0]) == k and int(results[r].status[0]) == 0
        assert np.array_equal(results[r].new_i1[0, :k].cpu().numpy(), want[r]["i1"]) and np.array_equal(results[r].new_i2[0, :k].cpu().numpy(), want[r]["i2"])
        assert G.same_bits(results[r].new_pos[0, :k].cpu().numpy(), want[r]["pos"])
        assert np.array_equal(results[r].reason[0].cpu().numpy(), want[r]["reason"])
    for slot, kf in enumerate([ref_cur] + ref_nbs):
        assert np.array_equal(kfs.keep[3][slot].cpu().numpy(), kf["has_mp"]) and np.array_equal(kfs.keep[4][slot].cpu().numpy(), kf["mappoints"])
    mt.close()

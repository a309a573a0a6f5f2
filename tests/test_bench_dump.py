"""bench.py --dump-outputs: what the last timed step computed, written as .npy for a fixed seeded sample of the frames.  Without a GPU the dump runs on
host tensors laid out as bench.Pipeline's buffers (sampling, padding, integer conversion, size budget); on the GPU a small real pipeline is dumped and the
sampled frames are compared with the CPU oracle, and a second pipeline built with the same arguments must dump the same arrays."""
import os
import sys

import numpy as np
import pytest
import torch

import orc

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402

NAMES = ["descriptors", "frame_index", "keypoint_count", "keypoints", "line_count", "line_descriptors", "line_equations", "lines",
         "lines_last_frame_match_count", "lines_last_frame_matches", "lines_map_match_count", "lines_map_matches",
         "points_last_frame_match_count", "points_last_frame_matches", "points_map_match_count", "points_map_matches"]


class _HostPipe:
    """the attributes of bench.Pipeline that dump_outputs reads, on host tensors; buffer set k & 1 of the last step k holds random outputs"""
    torch = torch

    def __init__(self, B, cap, nl, k, seed):
        g = torch.Generator().manual_seed(seed)
        self.B, self.cap, self.nlines, self.k = B, cap, nl, k
        ri = lambda shape, hi, dt=torch.int32: torch.randint(0, hi, shape if isinstance(shape, tuple) else (shape,), generator=g, dtype=dt)

        def bufset():
            kps = torch.rand((B, cap, 7), generator=g) * 640
            kps.view(torch.int32)[..., 5:7] = ri((B, cap, 2), 8)
            lines = torch.rand((B, nl, 17), generator=g) * 640
            lines.view(torch.int32)[..., [1, 2, 16]] = ri((B, nl, 3), 500)
            return dict(kps=kps, desc=ri((B, cap, 32), 256, torch.uint8), nk=ri(B, cap + 1), lines=lines, ldesc=ri((B, nl, 32), 256, torch.uint8),
                        leq=torch.rand((B, nl, 3), generator=g, dtype=torch.float64), nl=ri(B, nl + 1),
                        match_kp=ri((B, cap), 5000) - 1, nm_kp=ri(B, cap), match_kp_last=ri((B, cap), 1000) - 1, nm_kp_last=ri(B, cap),
                        match_ln=ri((B, nl), 500) - 1, nm_ln=ri(B, nl), match_ln_last=ri((B, nl), 100) - 1, nm_ln_last=ri(B, nl))
        self.bufs = [bufset(), bufset()]


def _load(d):
    return {n: np.load(os.path.join(d, n + ".npy")) for n in NAMES}


def test_dump_of_the_last_step_on_host_tensors(tmp_path):
    B, cap, nl = 300, 1032, 100
    pipe = _HostPipe(B, cap, nl, k=7, seed=1)
    info = bench.dump_outputs(pipe, str(tmp_path / "a"))
    assert sorted(os.listdir(tmp_path / "a")) == sorted(n + ".npy" for n in NAMES) and info["arrays"] == NAMES
    o = _load(str(tmp_path / "a"))
    assert all(a.dtype == (np.float64 if n in ("line_equations", "frame_index") else np.float32) for n, a in o.items())
    assert info["frames"] == bench.DUMP_FRAMES and info["bytes"] == sum(a.nbytes for a in o.values()) <= 64_000_000
    idx = o["frame_index"].astype(np.int64)
    assert len(np.unique(idx)) == len(idx) == bench.DUMP_FRAMES and np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < B
    bs = {k: v.numpy() for k, v in pipe.bufs[6 & 1].items()}       # the last step k = 6
    for j in (0, 17, len(idx) - 1):
        f = idx[j]
        n, m = int(bs["nk"][f]), int(bs["nl"][f])
        assert o["keypoint_count"][j] == n and o["line_count"][j] == m
        assert np.array_equal(o["keypoints"][j, :n, :5], bs["kps"][f, :n, :5]) and np.array_equal(o["keypoints"][j, :n, 5:], bs["kps"][f, :n, 5:].view(np.int32))
        assert np.array_equal(o["descriptors"][j, :n], bs["desc"][f, :n]) and not o["keypoints"][j, n:].any() and not o["descriptors"][j, n:].any()
        li = [1, 2, 16]; lf = [c for c in range(17) if c not in li]
        assert np.array_equal(o["lines"][j, :m][:, lf], bs["lines"][f, :m][:, lf]) and np.array_equal(o["lines"][j, :m][:, li], bs["lines"][f, :m][:, li].view(np.int32))
        assert np.array_equal(o["line_descriptors"][j, :m], bs["ldesc"][f, :m]) and np.array_equal(o["line_equations"][j, :m], bs["leq"][f, :m])
        assert not o["lines"][j, m:].any() and not o["line_equations"][j, m:].any()
        for name, key, cnt in (("points_map", "kp", n), ("points_last_frame", "kp_last", n), ("lines_map", "ln", m), ("lines_last_frame", "ln_last", m)):
            assert np.array_equal(o[name + "_matches"][j, :cnt], bs["match_" + key][f, :cnt]) and (o[name + "_matches"][j, cnt:] == -1).all()
            assert o[name + "_match_count"][j] == bs["nm_" + key][f]
    # the same pipeline state dumps the same arrays (the sample is fixed)
    bench.dump_outputs(pipe, str(tmp_path / "b"))
    o2 = _load(str(tmp_path / "b"))
    assert all(np.array_equal(o[n], o2[n]) for n in NAMES)


def test_dump_stays_within_64_mb_on_large_frames(tmp_path):
    # BASELINE configs[3] sizes (4000 ORB + 400 lines): 256 frames would be ~190 MB, so fewer frames are sampled
    pipe = _HostPipe(100, 4032, 400, k=2, seed=2)
    info = bench.dump_outputs(pipe, str(tmp_path))
    assert 0 < info["frames"] < 100 and info["bytes"] <= 64_000_000
    assert sum(os.path.getsize(os.path.join(tmp_path, n + ".npy")) for n in NAMES) <= 64_000_000 + 128 * len(NAMES)


@pytest.mark.gpu
def test_dump_of_a_real_pipeline_equals_the_oracle(tmp_path):
    from conftest import gpu_available
    if not gpu_available():
        pytest.fail("no GPU visible: the -m gpu tests need a real MI355X")
    W, H, NFEAT, NLINES = bench.CONFIGS[2][:4]
    dumps = []
    for run in range(2):
        pipe = bench.Pipeline(W, H, NFEAT, NLINES, 16, 0, 0, distinct=16)
        bench.timed(pipe, 2, 1)
        assert pipe.k == 3                                           # 1 warm-up + 2 timed steps
        d = str(tmp_path / ("run%d" % run))
        bench.dump_outputs(pipe, d)
        dumps.append(_load(d))
        if run == 0:
            imgs, mp = pipe.h_distinct.copy(), {k: v.cpu().numpy() for k, v in pipe.mp.items()}
            scale = pipe.scale.cpu().numpy()
        pipe.close()
    o = dumps[0]
    assert all(np.array_equal(o[n], dumps[1][n]) for n in NAMES)   # same arguments, same outputs
    assert o["frame_index"].tolist() == list(range(16))
    for f in range(16):
        ro, rl = orc.orb_extract(imgs[f], nfeatures=NFEAT), orc.line_extract(imgs[f], NLINES)
        n, m = len(ro["kps"]), len(rl["kl"])
        assert o["keypoint_count"][f] == n and o["line_count"][f] == m
        for c, fld in enumerate(("x", "y", "size", "angle", "response", "octave", "class_id")):
            assert np.array_equal(o["keypoints"][f, :n, c], ro["kps"][fld].astype(np.float32)), (f, fld)
        assert np.array_equal(o["descriptors"][f, :n], ro["desc"]) and np.array_equal(o["line_descriptors"][f, :m], rl["desc"])
        for c, fld in enumerate(rl["kl"].dtype.names):
            assert np.array_equal(o["lines"][f, :m, c], rl["kl"][fld].astype(np.float32)), (f, fld)
        assert np.allclose(o["line_equations"][f, :m], rl["eq"], rtol=0, atol=1e-9)
    # frame 0's local-map search (the map was built from frame 0's key points)
    ro = orc.orb_extract(imgs[0], nfeatures=NFEAT)
    rm, rn = orc.search_by_projection_map(ro["kps"], ro["desc"], None, scale, (0.0, 0.0, float(W), float(H)), mp, 3.0, 0.8,
                                          np.full(len(ro["kps"]), -1, np.int32))
    assert o["points_map_match_count"][0] == rn > 0 and np.array_equal(o["points_map_matches"][0, :len(rm)], rm)

"""k_orb_level (FAST tiles: pre-test, packed cornerScore, the two threshold passes, the redo in row halves, the suppression queues, the raster emission) and
k_orient_brief (moments, fastAtan2, steered BRIEF, slot -> workgroup mapping, capacity cut): byte-equal to the oracle on the small images of
tests/orbfront_cases.py, alone, in batches with flat frames between them, and at capacities below the frame's key points.  Tolerances: NONE.
What each image reaches -- exact ties, scores at either threshold, cell / tile borders, the extreme key points, exact and near-diagonal angles, lists over capacity
in pass A, in pass B and in a tile of both kinds, queues that wrap -- is asserted on the CPU in tests/test_orb_front_cases.py.

Not covered, because no input reaches it: a level with more candidates than its pool (status bit 1).  The pool holds ceil(w / 2) * ceil(h / 2) entries per cell
region, and strict 3 x 3 maxima are never adjacent, not even diagonally, so no region yields more."""
import ctypes as C

import numpy as np
import pytest

import octree_cases as oc
import orbfront_cases as fc
from conftest import gpu_available

pytestmark = pytest.mark.gpu
NL = fc.NLEVELS
SENTINEL = 0xA5


def _need_gpu():
    if not gpu_available():
        pytest.fail("no GPU visible: the -m gpu tests need a real MI355X")


def _extractor(max_batch=1):
    from rgbd_pl_slam_amd import ORBextractor
    return ORBextractor(nfeatures=fc.NF, nlevels=NL, max_width=fc.W, max_height=fc.H, max_batch=max_batch)


@pytest.fixture(scope="module")
def ext1():
    _need_gpu()
    e = _extractor()
    yield e
    e.close()


def _check_stages(ext, frame, lv, ref, what):
    for l, (k, _, _, _) in enumerate(lv):
        assert np.array_equal(ext.pyramid_level(frame, l), ref["pyr"][l]), "padded plane of %s, level %d" % (what, l)
        assert np.array_equal(ext.blurred_level(frame, l), ref["blur"][l]), "blurred plane of %s, level %d" % (what, l)
        cand = ext.candidates(frame, l)
        assert len(cand) == ref["ncand"][l], "candidates of %s, level %d: %d, oracle %d" % (what, l, len(cand), ref["ncand"][l])
        assert np.array_equal(cand, k), "candidates of %s, level %d" % (what, l)


def _check_out(kps, desc, ref, what):
    assert kps.tobytes() == ref["kps"].tobytes(), "key points of %s" % what
    assert np.array_equal(desc, ref["desc"]), "descriptors of %s" % what


@pytest.mark.parametrize("name", list(fc.CASES))
def test_every_case_equals_the_oracle(ext1, name):
    """stage by stage: padded and blurred planes, the candidates of every level as an array (the dense images: the model's claim of which path ran rests on these
    totals being the oracle's), key points and descriptors"""
    img, lv, ref = fc.ref(name)
    kps, desc = ext1(img)
    _check_stages(ext1, 0, lv, ref, "'%s'" % name)
    _check_out(kps, desc, ref, "'%s'" % name)


@pytest.mark.parametrize("B,start", fc.BATCHES)
def test_batches_with_flat_frames(B, start):
    """every frame of a batch equals the same image alone (the oracle's bytes, which test_every_case_equals_the_oracle pins the single frames to).  9, 11 and 17 frames
    leave the last group of 8 of k_orient_brief partial: one frame, a flat one; three, the last one flat.  Between them the batches hold every named image
    (test_the_batches_hold_every_named_image)."""
    _need_gpu()
    names = fc.batch_names(B, start)
    imgs = np.stack([oc.flat() if n is None else fc.ref(n)[0] for n in names])
    ext = _extractor(max_batch=B)
    res = ext.extract_batch(imgs)
    for f, n in enumerate(names):
        if n is None:
            assert len(res[f][0]) == 0 and res[f][1].shape == (0, 32), "flat frame %d" % f
            assert all(len(ext.candidates(f, l)) == 0 for l in range(NL))
        else:
            _, lv, ref = fc.ref(n)
            _check_stages(ext, f, lv, ref, "'%s' as frame %d of %d" % (n, f, B))
            _check_out(res[f][0], res[f][1], ref, "'%s' as frame %d of %d" % (n, f, B))
    ext.close()


# ---------------------------------------------------------------------------------------------------------------- capacity
CAP_FRAMES = ["satellites", "one block", "diagonal pairs"]     # 24, 2 and 15 key points
GUARD = 4                                                      # rows behind the last frame's block


def _cap_ref():
    refs = [fc.ref(n)[2] for n in CAP_FRAMES]
    assert [len(r["kps"]) for r in refs] == [24, 2, 15]
    return refs


def _check_capacity(rc, kps, desc, n, cap, refs):
    """kps / desc: uint8 arrays [(3 * cap + GUARD) rows], filled with SENTINEL before the call; n: int32 [3 + GUARD]"""
    from rgbd_pl_slam_amd import _lib as L
    most = max(len(r["kps"]) for r in refs)
    assert rc == (L.PLF_OK if cap >= most else L.PLF_E_CAPACITY), "status at capacity %d" % cap
    kps = kps.reshape(-1, 28); desc = desc.reshape(-1, 32)
    for f, r in enumerate(refs):
        m = min(len(r["kps"]), cap)
        assert n[f] == m, "n_out of frame %d at capacity %d" % (f, cap)
        # the frame's rows start at f * capacity and are the oracle's first rows
        assert kps[f * cap: f * cap + m].tobytes() == r["kps"][:m].tobytes(), "key points of frame %d at capacity %d" % (f, cap)
        assert np.array_equal(desc[f * cap: f * cap + m], r["desc"][:m]), "descriptors of frame %d at capacity %d" % (f, cap)
        # rows of the frame's block it has no key points for: untouched
        assert np.all(kps[f * cap + m: (f + 1) * cap] == SENTINEL) and np.all(desc[f * cap + m: (f + 1) * cap] == SENTINEL), "frame %d at capacity %d" % (f, cap)
    assert np.all(kps[3 * cap:] == SENTINEL) and np.all(desc[3 * cap:] == SENTINEL) and np.all(n[3:] == -1), "bytes behind the last frame at capacity %d" % cap


@pytest.mark.parametrize("cap", [24, 23, 1])
def test_capacity_host_output(cap):
    """the caller's capacity at n, n - 1 and 1 of the fullest frame: PLF_OK at n, PLF_E_CAPACITY below, n_out = min(n, capacity), the first rows, frames strided by the
    caller's capacity, nothing written behind them"""
    _need_gpu()
    from rgbd_pl_slam_amd import _lib as L
    refs = _cap_ref()
    imgs = np.stack([fc.ref(n)[0] for n in CAP_FRAMES])
    ext = _extractor(max_batch=3)
    kps = np.full((3 * cap + GUARD) * 28, SENTINEL, np.uint8); desc = np.full((3 * cap + GUARD) * 32, SENTINEL, np.uint8); n = np.full(3 + GUARD, -1, np.int32)
    rc = L.lib().plf_orb_extract_batch(ext._h, L.vp(imgs), L.MEM_HOST, 3, fc.W, fc.H, C.c_ssize_t(fc.W), C.c_ssize_t(fc.W * fc.H), L.vp(kps), L.vp(desc), L.vp(n),
                                       L.MEM_HOST, cap, None)
    _check_capacity(rc, kps, desc, n, cap, refs)
    ext.close()


@pytest.mark.parametrize("in_mem", ["host", "device"])
@pytest.mark.parametrize("cap", [24, 23, 1])
def test_capacity_device_output(cap, in_mem):
    """the same with the outputs on the device, where k_orient_brief itself gets the caller's capacity: its grid is cut to `capacity` slots, it clips n_out and sets
    status bit 2.  With the input on the host the call reads the status and returns it.  With the input on the device too the call is asynchronous and returns PLF_OK
    whatever the status word will say: the caller sees the cut in n_out == capacity only -- recorded here, not judged."""
    _need_gpu()
    import torch
    from rgbd_pl_slam_amd import _lib as L
    refs = _cap_ref()
    imgs = np.stack([fc.ref(n)[0] for n in CAP_FRAMES])
    ext = _extractor(max_batch=3)
    d_kps = torch.full(((3 * cap + GUARD) * 28,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_desc = torch.full(((3 * cap + GUARD) * 32,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_n = torch.full((3 + GUARD,), -1, dtype=torch.int32, device="cuda")
    d_img = torch.from_numpy(imgs).cuda() if in_mem == "device" else None
    torch.cuda.synchronize()
    rc = L.lib().plf_orb_extract_batch(ext._h, L.vp(d_img) if in_mem == "device" else L.vp(imgs), L.MEM_DEVICE if in_mem == "device" else L.MEM_HOST, 3, fc.W, fc.H,
                                       C.c_ssize_t(fc.W), C.c_ssize_t(fc.W * fc.H), L.vp(d_kps), L.vp(d_desc), L.vp(d_n), L.MEM_DEVICE, cap, None)
    torch.cuda.synchronize()
    if in_mem == "device":
        assert rc == L.PLF_OK
        rc = L.PLF_OK if cap >= 24 else L.PLF_E_CAPACITY      # (what the synchronous paths return for the same outputs)
    _check_capacity(rc, d_kps.cpu().numpy(), d_desc.cpu().numpy(), d_n.cpu().numpy(), cap, refs)
    ext.close()


# ---------------------------------------------------------------------------------------------------------------- parameter sets
@pytest.mark.parametrize("name", list(fc.PARAM_SETS))
def test_parameter_sets_with_clamped_last_cells(name):
    """the parameter sets of test_level_geometries_with_clamped_last_cells at the smallest sizes that keep a last cell row without a computed region behind a shortened
    one, or a last tile one column group wide, with uniform noise and the plateau pieces in that last cell and tile (test_the_shrunk_parameter_sets_keep_their_property)"""
    _need_gpu()
    from rgbd_pl_slam_amd import ORBextractor
    w, h, sf, nlev, ini, mn, nf = fc.PARAM_SETS[name]
    img = fc.param_image(name)
    lv, ref = oc.level_candidates(img, nf, nlevels=nlev, scale_factor=sf, ini_th=ini, min_th=mn)
    ext = ORBextractor(nfeatures=nf, scaleFactor=sf, nlevels=nlev, iniThFAST=ini, minThFAST=mn, max_width=w, max_height=h)
    kps, desc = ext(img)
    _check_stages(ext, 0, lv, ref, "'%s'" % name)
    _check_out(kps, desc, ref, "'%s'" % name)
    ext.close()

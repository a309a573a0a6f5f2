"""GPU parity of the split ORB front -- k_orb_pyramid (padded planes), k_orb_blur (blurred planes), k_orb_level (FAST tiles read from the planes) -- against
the CPU oracle, bit for bit: padded plane with its border, blurred plane, candidate counts, key points, descriptors.  Tolerances: NONE.

The shapes sit where the row-walking mapping can go wrong.  A wave owns 256 columns (4 per lane) -- of the padded plane (w + 38) in k_orb_pyramid, of the
level (w) in k_orb_blur -- and a band of 8 / 16 / 32 rows for <= 4 / <= 16 / more frames in flight:
  * widths 255..258 (w % 4 = 3, 0, 1, 2; one below, at, above the blur span) and 473..475 (w + 38 = 511, 512, 513: the pyramid span), 511..513, with 480 and 250
    rows where the reference accepts the aspect (a 255 x 480 image has round(width / height) = 0 octree roots); 307 x 250: level 1 is 256 wide, exactly a span;
    262 x 250: the padded plane of level 1 (218 + 38) is exactly a span;
  * heights 255, 256, 257 = one fewer, exactly, one more than a whole number of bands of 8, 16 and 32 rows, as a single frame and as batches of 5 and 17 frames.
    No accepted level is shorter than a band: every level has >= 62 rows (one 30-pixel cell inside the 16-pixel margins) and the tallest band is 32; the
    nearest case is the smallest accepted image, 221 x 221, whose deepest level (62 x 62) is one band of 32 and a cut one of 30;
  * the blur's saturation / half-to-even / tail-column image, all-255 and all-0, at 642 x 481, 333 x 250 and 221 x 221;
  * nlevels = 1, scale factors 1.1 and 1.3, 2.0 (source windows of exactly 8 bytes) and 2.5 (the wide-window resize path);
  * a device-resident batch with pitch > width and a frame stride > pitch * h; one handle alternating two sizes, and a batch after a single frame."""
import ctypes as C
import functools

import numpy as np
import pytest

import orc
from conftest import gpu_available

pytestmark = pytest.mark.gpu


def _need_gpu():
    if not gpu_available():
        pytest.fail("no GPU visible: the -m gpu tests need a real MI355X")


def _scene(seed, w, h):
    from rgbd_pl_slam_amd.synth import synth_frame
    return synth_frame(seed, w, h)


def _blur_edge(w, h):
    """the image of test_orb_blur_saturation_and_tail_columns (tests/test_gpu_orb.py), rectangles scaled to the image"""
    rng = np.random.default_rng(w)
    img = np.full((h, w), 255, np.uint8)
    img[: h // 3] = 254
    yy, xx = np.mgrid[0:h, 0:w]
    img[h // 3: h // 2] = np.where(((yy[h // 3: h // 2] // 9) + (xx[h // 3: h // 2] // 9)) % 2 == 0, 255, 253).astype(np.uint8)
    img[h // 2: 2 * h // 3] = (255 - (xx[h // 2: 2 * h // 3] % 64)).astype(np.uint8)
    img[2 * h // 3:] = rng.choice(np.array([0, 128, 254, 255], np.uint8), size=(h - 2 * h // 3, w))
    for _ in range(30):   # dark rectangles: corners on the plateaus
        x0, y0 = int(rng.integers(0, w - 40)), int(rng.integers(0, h - 40))
        img[y0:y0 + int(rng.integers(8, 40)), x0:x0 + int(rng.integers(8, 40))] = int(rng.integers(0, 256))
    return img


@functools.lru_cache(maxsize=None)
def _image(kind, w, h, seed=0):
    if kind == "scene":
        img = _scene(seed, w, h)
    elif kind == "edge":
        img = _blur_edge(w, h)
    else:
        img = np.full((h, w), int(kind), np.uint8)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def _ref(kind, w, h, seed=0, nf=1000, sf=1.2, nlev=8, ini=20, mn=7):
    """the oracle's result, computed once per case and shared"""
    return orc.orb_extract(_image(kind, w, h, seed), nfeatures=nf, scale_factor=sf, nlevels=nlev, ini_th=ini, min_th=mn, debug=True)


def _check_stages(ext, frame, ref, nlev):
    for l in range(nlev):
        assert np.array_equal(ext.pyramid_level(frame, l), ref["pyr"][l]), "padded plane of level %d, frame %d" % (l, frame)
        assert np.array_equal(ext.blurred_level(frame, l), ref["blur"][l]), "blurred plane of level %d, frame %d" % (l, frame)
        assert len(ext.candidates(frame, l)) == ref["ncand"][l], "FAST candidates of level %d, frame %d" % (l, frame)


def _check_out(kps, desc, ref):
    assert kps.tobytes() == ref["kps"].tobytes(), "key points"
    assert np.array_equal(desc, ref["desc"]), "descriptors"


def _single(kind, w, h, seed=0, nf=1000, sf=1.2, nlev=8, ini=20, mn=7, ext=None):
    from rgbd_pl_slam_amd import ORBextractor
    ref = _ref(kind, w, h, seed, nf, sf, nlev, ini, mn)
    own = ext is None
    if own:
        ext = ORBextractor(nfeatures=nf, scaleFactor=sf, nlevels=nlev, iniThFAST=ini, minThFAST=mn, max_width=w, max_height=h)
    kps, desc = ext(_image(kind, w, h, seed))
    _check_stages(ext, 0, ref, nlev)
    _check_out(kps, desc, ref)
    if own:
        ext.close()


WIDTHS = [(255, 250), (256, 250), (257, 250), (258, 250), (473, 480), (474, 480), (475, 480), (473, 250), (474, 250), (475, 250),
          (511, 480), (512, 480), (513, 480), (307, 250), (262, 250)]


@pytest.mark.parametrize("w,h", WIDTHS)
def test_widths_around_lane_group_and_span(w, h):
    _need_gpu()
    _single("scene", w, h, seed=w)


HEIGHTS = [255, 256, 257]


@pytest.mark.parametrize("h", HEIGHTS)
def test_heights_around_band_single_frame(h):
    _need_gpu()
    _single("scene", 222, h, seed=h)


def test_smallest_accepted_image():
    _need_gpu()
    _single("scene", 221, 221, seed=5)


@pytest.mark.parametrize("frames", [5, 17])
def test_heights_around_band_batches(frames):
    """5 frames in flight: bands of 16 rows; 17: bands of 32.  Three heights per batch size; every frame against its own single-frame reference."""
    _need_gpu()
    from rgbd_pl_slam_amd import ORBextractor
    for h in HEIGHTS:
        imgs = np.stack([_image("scene", 222, h, seed=h + 3 * (f % 3)) for f in range(frames)])
        ext = ORBextractor(max_width=222, max_height=h, max_batch=frames)
        res = ext.extract_batch(imgs)
        for f in range(frames):
            ref = _ref("scene", 222, h, h + 3 * (f % 3))
            if f in (0, 1, frames - 1):
                _check_stages(ext, f, ref, 8)
            _check_out(res[f][0], res[f][1], ref)
        ext.close()


@pytest.mark.parametrize("w,h", [(642, 481), (333, 250), (221, 221)])
@pytest.mark.parametrize("kind", ["edge", "255", "0"])
def test_blur_edge_images(kind, w, h):
    _need_gpu()
    _single(kind, w, h)


PARAMS = [(640, 480, 1.2, 1, 20, 7, 1000), (1280, 960, 1.1, 8, 26, 5, 2000), (723, 542, 1.3, 5, 20, 7, 800), (640, 480, 2.0, 3, 20, 7, 1000),
          (642, 481, 2.5, 3, 20, 7, 1000)]


@pytest.mark.parametrize("w,h,sf,nlev,ini,mn,nf", PARAMS)
def test_parameter_sets(w, h, sf, nlev, ini, mn, nf):
    _need_gpu()
    _single("scene", w, h, seed=31, nf=nf, sf=sf, nlev=nlev, ini=ini, mn=mn)


def test_strided_device_batch():
    """3 different device-resident frames, pitch > width, frame stride > pitch * h: every frame equals its single-frame result"""
    _need_gpu()
    import torch
    from rgbd_pl_slam_amd import ORBextractor
    from rgbd_pl_slam_amd import _lib as L
    w, h, pitch = 333, 250, 352
    fstride = pitch * h + 1000
    host = np.full(3 * fstride, 77, np.uint8)   # (the padding holds a value no frame mirrors into its border)
    for f in range(3):
        host[f * fstride: f * fstride + pitch * h].reshape(h, pitch)[:, :w] = _image("scene", w, h, seed=40 + f)
    dev = torch.from_numpy(host).cuda()
    ext = ORBextractor(max_width=w, max_height=h, max_batch=3)
    kps = np.zeros((3, ext.capacity), L.KP_DTYPE); desc = np.zeros((3, ext.capacity, 32), np.uint8); n = np.zeros(3, np.int32)
    L.check(L.lib().plf_orb_extract_batch(ext._h, L.vp(dev), L.MEM_DEVICE, 3, w, h, C.c_ssize_t(pitch), C.c_ssize_t(fstride), L.vp(kps), L.vp(desc), L.vp(n),
                                          L.MEM_HOST, ext.capacity, None), "plf_orb_extract_batch")
    for f in range(3):
        ref = _ref("scene", w, h, 40 + f)
        _check_stages(ext, f, ref, 8)
        _check_out(kps[f, :n[f]], desc[f, :n[f]], ref)
    ext.close()


def test_handle_reuse_two_sizes_and_batch_after_single():
    _need_gpu()
    from rgbd_pl_slam_amd import ORBextractor
    ext = ORBextractor(max_width=640, max_height=480, max_batch=3)
    for w, h in ((640, 480), (333, 250), (640, 480), (333, 250)):   # (the tables are uploaded again at every change of size)
        _single("scene", w, h, seed=w, ext=ext)
    imgs = np.stack([_image("scene", 333, 250, seed=40 + f) for f in range(3)])
    res = ext.extract_batch(imgs)
    for f in range(3):
        ref = _ref("scene", 333, 250, 40 + f)
        _check_stages(ext, f, ref, 8)
        _check_out(res[f][0], res[f][1], ref)
    _single("scene", 640, 480, seed=640, ext=ext)
    ext.close()

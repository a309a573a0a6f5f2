"""GPU parity of the line extractor's front: the gradient plane the LBD descriptor reads (k_blur5_sobel3 / k_sobel3, seen through plf_line_debug_gradient)
against the oracle's GaussianBlur + Sobel, pixel for pixel; the side stream the plane is computed on for large batches (plf_line_tune "front_fork"): batches,
handle reuse and both settings give the same bits; and the pre-pass of the detector (k_lsd_pre) at the widths where a row-pass item meets the image border."""
import ctypes as C

import numpy as np
import pytest

import orc
from conftest import gpu_available

pytestmark = pytest.mark.gpu
TOL = 1e-4
K5 = np.array([14, 63, 103, 63, 14], np.int64)   # cv::getGaussianKernel(5, 1) in 8-bit fixed point: the taps of GaussianBlur(5 x 5, sigma 1) on 8U


def _need_gpu():
    if not gpu_available():
        pytest.fail("no GPU visible: the -m gpu tests need a real MI355X")


def _reflect(p, n):
    p = np.abs(p)
    return np.where(p >= n, 2 * (n - 1) - p, p)


def _column_sums(img):
    """the 32-bit column sums of the 5 x 5 fixed-point blur before rounding (s / 65536 is the blurred value), REFLECT_101"""
    h, w = img.shape
    a = img.astype(np.int64)
    rows = sum(K5[t] * a[:, _reflect(np.arange(w) + t - 2, w)] for t in range(5))
    return sum(K5[t] * rows[_reflect(np.arange(h) + t - 2, h), :] for t in range(5))


def _ref_gradient(img, sobel_input):
    """(dx, dy) of the oracle: orc_sobel3_16s of orc_gaussian_blur_8u(5, 1.0) (PLF_LBD_BLURRED) or of the image itself (PLF_LBD_RAW)"""
    L = orc.lib()
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape
    src = img
    if sobel_input == orc.LBD_BLURRED:
        src = np.zeros_like(img)
        L.orc_gaussian_blur_8u(orc.p(img), C.c_ssize_t(w), orc.p(src), C.c_ssize_t(w), C.c_int(w), C.c_int(h), C.c_int(5), C.c_double(1.0))
    dx = np.zeros((h, w), np.int16); dy = np.zeros((h, w), np.int16)
    L.orc_sobel3_16s(orc.p(src), C.c_int(w), C.c_int(h), C.c_ssize_t(w), orc.p(dx), orc.p(dy))
    return dx, dy


def _half_image(w, h, seed):
    """Seeded noise in which a grid of pixels (every image border and the w % 4 tail columns included) has its 5 x 5 column sum moved onto an exact .5 boundary
    with an even integer part, where half-to-even (the vector columns) and half-up (the tail columns) give different bytes: two pixels of the window are solved for."""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (h, w), dtype=np.uint8)
    dx, dy = max(6, w // 8), max(6, h // 6)
    xs = [x for x in range(0, w, dx) if x <= w - 6] + [w - 1]
    ys = [y for y in range(0, h, dy) if y <= h - 6] + [h - 1]
    cc, nn = np.meshgrid(np.arange(256, dtype=np.int64), np.arange(256, dtype=np.int64), indexing="ij")
    for y in ys:
        for x in xs:
            x2, y3 = (x + 1 if x + 1 < w else x - 1), (y + 1 if y + 1 < h else y - 1)
            wt = np.zeros((h, w), np.int64)
            for ty in range(5):
                for tx in range(5):
                    wt[_reflect(np.int64(y + ty - 2), h), _reflect(np.int64(x + tx - 2), w)] += K5[ty] * K5[tx]
            for third in rng.integers(0, 256, 16):   # (two pixels reach the boundary for about every second window: a third one is varied until they do)
                img[y3, x] = third
                base = int((wt * img).sum()) - int(wt[y, x]) * int(img[y, x]) - int(wt[y, x2]) * int(img[y, x2])
                s = base + wt[y, x] * cc + wt[y, x2] * nn
                hit = np.argwhere(((s & 0xFFFF) == 0x8000) & (((s >> 16) & 1) == 0) & ((s >> 16) < 255))
                if len(hit):
                    img[y, x], img[y, x2] = hit[0]
                    break
    return img


def _images(w, h):
    """(name, image): noise, the two saturation images, and the .5-boundary image.  (0 / 255 checkerboards of period 1 and 2 were tried for the last two
    properties and have neither: their column sums are 255 * 33037 and 255 * (a product of tap subset sums), never 255 * 32768 = x.5, and stay below 2^24;
    the all-255 image reaches 255 * 257 * 257 >= 2^24 and _half_image the .5 boundaries.)"""
    rng = np.random.default_rng(1000 * w + h)
    return [("noise", rng.integers(0, 256, (h, w), dtype=np.uint8)), ("all255", np.full((h, w), 255, np.uint8)), ("all0", np.zeros((h, w), np.uint8)),
            ("half", _half_image(w, h, 7 * w + h))]


def _planes(img, sobel_input, ext=None):
    from rgbd_pl_slam_amd import LineSegment
    h, w = img.shape
    own = ext is None
    if own:
        ext = LineSegment(nlines=20, max_width=max(w, 16), max_height=max(h, 16), lbd_sobel_input=sobel_input)
    ext.ExtractLineSegment(img)
    dx, dy = ext.gradient(0, w, h)
    if own:
        ext.close()
    return dx, dy


SIZES = [(16, 16), (17, 33), (63, 31), (64, 32), (65, 33), (130, 70), (67, 35), (12, 40), (253, 66)]


@pytest.mark.parametrize("w,h", SIZES)
def test_gradient_plane_equals_the_oracle(w, h):
    """Every pixel of (dx, dy), both LBD inputs: smallest sizes, around 64 columns and 32 rows, w % 4 = 1, 2 and 3, an image narrower than the 16 bytes of a
    border window, and for k_blur5_sobel3's own geometry two bands of rows (more than 64 rows) and two waves of columns (more than 248, the second one holding only
    the image's last column).  The images reach the saturating column sums (>= 2^24) and the .5 boundaries on which the two rounding rules of the column filter differ."""
    from rgbd_pl_slam_amd import LineSegment
    from rgbd_pl_slam_amd.synth import synth_frame
    imgs = _images(w, h)
    if (w, h) == (130, 70):
        imgs.append(("synth", synth_frame(3, w, h)))
    # the images do what they are for (checked on the CPU, before anything needs the GPU)
    s = _column_sums(dict(imgs)["half"])
    differ = ((s & 0xFFFF) == 0x8000) & (((s >> 16) & 1) == 0)
    wvec = w & ~3
    assert differ[:, :wvec].sum() >= 4 and (w == wvec or differ[:, wvec:].sum() >= 1), "no .5 boundary in the vector / tail columns"
    assert _column_sums(dict(imgs)["all255"]).max() >= 1 << 24
    _need_gpu()
    for sobel_input in (orc.LBD_BLURRED, orc.LBD_RAW):
        ext = LineSegment(nlines=20, max_width=max(w, 16), max_height=max(h, 16), lbd_sobel_input=sobel_input)
        for name, img in imgs:
            dx, dy = _planes(img, sobel_input, ext)
            rx, ry = _ref_gradient(img, sobel_input)
            bad = (dx != rx) | (dy != ry)
            print("%s %dx%d input %d: %d of %d pixels differ" % (name, w, h, sobel_input, int(bad.sum()), bad.size))
            assert np.array_equal(dx, rx) and np.array_equal(dy, ry), (name, sobel_input, np.argwhere(bad)[:8].tolist())
        ext.close()


@pytest.mark.parametrize("w,h", [(130, 70), (253, 66)])
def test_gradient_plane_with_the_bands_of_a_large_batch(w, h):
    """k_blur5_sobel3 cuts the rows into shorter bands for a few frames in flight than for many (up to 8 / 16 / 32 / 64 rows for up to 4 / 16 / 64 / more frames):
    17 and 65 frames take the two longest, which the single-frame cases above never do"""
    _need_gpu()
    from rgbd_pl_slam_amd import LineSegment
    rng = np.random.default_rng(w)
    imgs = rng.integers(0, 256, (65, h, w), dtype=np.uint8)
    imgs[64] = _half_image(w, h, 5 * w + h)
    imgs[16] = 255
    ext = LineSegment(nlines=20, max_width=w, max_height=h, max_batch=65)
    for n in (17, 65):
        ext.extract_batch(imgs[65 - n:])
        for f in (0, n // 2, n - 1):
            dx, dy = ext.gradient(f, w, h)
            rx, ry = _ref_gradient(imgs[65 - n + f], orc.LBD_BLURRED)
            assert np.array_equal(dx, rx) and np.array_equal(dy, ry), (n, f)
    ext.close()


def _scene(w, h, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    return (((xx // (5 + seed % 3) + yy // 7) & 1) * 170 + 30 + ((xx + 2 * yy + seed) % 23) + rng.integers(0, 8, (h, w))).astype(np.uint8)


def test_batches_and_handle_reuse_with_the_fork_on():
    """One handle, max_batch 5, front_fork forced on: 130 x 70, then 65 x 33, then 130 x 70 again (twice), different images each call.  First the three calls back to back
    on one stream with device outputs and no host wait in between -- the gradient kernel of call k + 1 runs on the side stream and must not overtake the k_lbd of
    call k that still reads the plane -- then call by call with the plane read back.  Everything equals the single-frame results."""
    _need_gpu()
    import torch
    from rgbd_pl_slam_amd import LineSegment
    from rgbd_pl_slam_amd import _lib as L
    N = 20
    calls = [(130, 70, 10), (65, 33, 20), (130, 70, 30), (130, 70, 40)]   # (the fourth: a change of size waits for the device, the same size again does not)
    batches = [np.stack([_scene(w, h, s0 + f) for f in range(5)]) for w, h, s0 in calls]
    single = []   # per call, per frame: (keylines, descriptors, dx, dy) of a one-frame handle on the default single-stream schedule
    for (w, h, _), imgs in zip(calls, batches):
        one = LineSegment(nlines=N, max_width=w, max_height=h)
        res = []
        for f in range(5):
            kl, desc, _eq = one.ExtractLineSegment(imgs[f])
            res.append((kl, desc) + one.gradient(0, w, h))
        single.append(res)
        one.close()
    assert sum(len(r[0]) for res in single for r in res) > 0
    ext = LineSegment(nlines=N, max_width=130, max_height=70, max_batch=5)
    ext.tune("front_fork", 1)
    st = torch.cuda.Stream()
    outs = []
    for (w, h, _), imgs in zip(calls, batches):
        d = dict(img=torch.from_numpy(imgs).cuda(), lines=torch.zeros((5, N, 17), dtype=torch.float32, device="cuda"), desc=torch.zeros((5, N, 32), dtype=torch.uint8, device="cuda"),
                 eq=torch.zeros((5, N, 3), dtype=torch.float64, device="cuda"), n=torch.zeros(5, dtype=torch.int32, device="cuda"))
        outs.append(d)
    torch.cuda.synchronize()
    for (w, h, _), d in zip(calls, outs):
        ext.extract_batch_device(d["img"], w, h, d["lines"], d["desc"], d["eq"], d["n"], N, st.cuda_stream)
    st.synchronize()
    for ci, ((w, h, _), d) in enumerate(zip(calls, outs)):
        n = d["n"].cpu().numpy()
        for f in range(5):
            kl = np.frombuffer(d["lines"][f, :n[f]].cpu().numpy().tobytes(), L.KL_DTYPE)
            assert kl.tobytes() == single[ci][f][0].tobytes() and np.array_equal(d["desc"][f, :n[f]].cpu().numpy(), single[ci][f][1]), (ci, f)
    for f in range(5):
        dx, dy = ext.gradient(f, 130, 70)
        assert np.array_equal(dx, single[3][f][2]) and np.array_equal(dy, single[3][f][3]), f
    for ci, ((w, h, _), imgs) in enumerate(zip(calls, batches)):
        res = ext.extract_batch(imgs)
        for f in range(5):
            dx, dy = ext.gradient(f, w, h)
            assert np.array_equal(dx, single[ci][f][2]) and np.array_equal(dy, single[ci][f][3]), (ci, f)
            assert res[f][0].tobytes() == single[ci][f][0].tobytes() and np.array_equal(res[f][1], single[ci][f][1]), (ci, f)
    ext.close()


def test_front_fork_off_and_on_give_the_same_bits():
    """key lines, descriptors, equations and segments of 3 frames at 322 x 243 through extract_batch_device on a non-default stream, followed by wait_front on a
    second stream as the benchmark's step uses it; front_fork 0 against 1"""
    _need_gpu()
    import torch
    from rgbd_pl_slam_amd import LineSegment
    from rgbd_pl_slam_amd.synth import synth_frame
    w, h, N = 322, 243, 60
    imgs = np.stack([synth_frame(50 + f, w, h) for f in range(3)])
    d_img = torch.from_numpy(imgs).cuda()
    got = []
    for fork in (0, 1):
        ext = LineSegment(nlines=N, max_width=w, max_height=h, max_batch=3)
        ext.tune("front_fork", fork)
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        lines = torch.zeros((3, N, 17), dtype=torch.float32, device="cuda"); desc = torch.zeros((3, N, 32), dtype=torch.uint8, device="cuda")
        eq = torch.zeros((3, N, 3), dtype=torch.float64, device="cuda"); n = torch.zeros(3, dtype=torch.int32, device="cuda")
        marker = torch.zeros(1, device="cuda")
        torch.cuda.synchronize()
        ext.extract_batch_device(d_img, w, h, lines, desc, eq, n, N, s1.cuda_stream)
        ext.wait_front(s2.cuda_stream)
        with torch.cuda.stream(s2):
            marker += 1
        s1.synchronize(); s2.synchronize()
        assert ext.last_status(s1.cuda_stream) == 0 and float(marker[0]) == 1.0
        got.append([n.cpu().numpy(), lines.cpu().numpy(), desc.cpu().numpy(), eq.cpu().numpy()] + [ext.segments(f) for f in range(3)] +
                   [np.stack(ext.gradient(f, w, h)) for f in range(3)])
        ext.close()
    assert got[0][0].min() > 0
    for a, b in zip(got[0], got[1]):
        assert a.shape == b.shape and a.tobytes() == b.tobytes()
    ref = orc.line_extract(imgs[1], N)
    assert np.array_equal(got[1][2][1, :got[1][0][1]], ref["desc"])


def _check(img, nlines):
    """full comparison with the oracle: segments, key lines, equations, descriptors -- bit-equal floats demanded, 1e-4 only as the reported fallback"""
    from rgbd_pl_slam_amd import LineSegment
    h, w = img.shape
    ext = LineSegment(nlines=nlines, max_width=w, max_height=h)
    kl, desc, eq = ext.ExtractLineSegment(img)
    segs = ext.segments(0)
    ext.close()
    ref_seg = orc.lsd_detect(img)["lines"]
    ref = orc.line_extract(img, nlines)
    assert len(segs) == len(ref_seg), "segment count %d vs %d" % (len(segs), len(ref_seg))
    assert np.allclose(segs, ref_seg, rtol=0, atol=TOL)
    nbits = int((segs.view(np.uint32) != ref_seg.view(np.uint32)).sum())
    assert len(kl) == len(ref["kl"])
    for name in kl.dtype.names:
        a, b = kl[name], ref["kl"][name]
        if a.dtype.kind == "f":
            assert np.allclose(a, b, rtol=0, atol=TOL * max(1.0, float(np.abs(b).max()) if len(b) else 1.0)), name
        else:
            assert np.array_equal(a, b), name
    assert np.allclose(eq, ref["eq"], rtol=0, atol=1e-4)
    same_fields = all(np.array_equal(kl[n].view(np.uint32), ref["kl"][n].view(np.uint32)) for n in kl.dtype.names)
    bad_rows = int((desc != ref["desc"]).any(1).sum())
    assert bad_rows == 0, "LBD descriptors differ in %d of %d rows (keylines bit-equal: %s)" % (bad_rows, len(desc), same_fields)
    assert nbits == 0 and same_fields, "float outputs within 1e-4 but not bit-equal (segments differing words: %d)" % nbits
    return len(segs)


@pytest.mark.parametrize("h", [30, 61])
@pytest.mark.parametrize("w", [16, 17, 23, 24, 25, 31, 32, 33, 71, 88, 89])
def test_pre_pass_at_the_widths_around_a_row_item(w, h):
    """widths that put an item of consecutive row-pass outputs and its source window against the left and right image border and against the last column group of
    a tile; one scaled tile row (24 rows = 30 input rows) and a height that ends one row into the third"""
    _need_gpu()
    _check(_scene(w, h, w + h), 20)


def test_pre_pass_keeps_a_product_per_tap_when_the_taps_are_not_symmetric(monkeypatch):
    """PLF_LSD_ROW7 (read when the handle is created) makes the host's symmetry check of the 7 blur taps fail: the row pass then runs the retained form with
    items of 4 outputs and a product per tap -- same bits"""
    _need_gpu()
    monkeypatch.setenv("PLF_LSD_ROW7", "1")
    assert _check(_scene(89, 61, 3), 20) + _check(_scene(322, 243, 4), 60) > 0

"""The brute-force line matchers on the device -- k_knn2, k_knn2_batch, k_line_mad, k_lines_lastframe, k_lines_fuse_pick behind plf_match_lines_knn,
plf_line_descriptor_mad, plf_match_lines_lastframe, plf_match_lines_lastframe_batch, plf_match_lines_triangulation and plf_match_lines_fuse -- on the
directed cases of tests/linematch_cases.py, BIT FOR BIT against the sequential oracle (orc.*): no tolerance, no excluded row, sentinels behind every
output.  What each case reaches is proved on the CPU in tests/test_linematch_cases.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import linematch_cases as lc
import orc
from conftest import gpu_available

from rgbd_pl_slam_amd import _lib as L
from rgbd_pl_slam_amd import Matcher

pytestmark = pytest.mark.gpu

TAIL, SENT = 64, -77          # sentinel rows behind every output, and their value
_cache = {}


def _require_gpu():
    if not gpu_available():
        pytest.fail("no GPU visible: the -m gpu tests need a real MI355X")


@pytest.fixture(autouse=True)
def _need_gpu():
    _require_gpu()


@pytest.fixture(scope="module")
def m():
    _require_gpu()
    h = Matcher(max_keypoints=64, max_mappoints=64, max_lines=lc.SIZES_MAX_LINES, max_batch=len(lc.BATCH_FRAME_SIZES))
    yield h
    h.close()


@pytest.fixture(scope="module")
def big():
    _require_gpu()
    h = Matcher(max_keypoints=64, max_mappoints=64, max_lines=18000, max_batch=1)
    yield h
    h.close()


def once(key, fn):
    """cases and oracle results are computed once per process and shared"""
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def case(name):
    table = once("cases", lambda: {c["name"]: c for c in lc.sizes() + [lc.zero_mad(301), lc.zero_mad(300), lc.median_split(4), lc.median_split(256), lc.shared_train()] + lc.fuse_edges()})
    return table[name]


def ref_knn(c):
    return once(("knn", c["name"]), lambda: orc.knn2(c["query"], c["train"]))


def ref_last(name, q, t, has):
    return once(("last", name), lambda: orc.match_lines_knn(q, t, has))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def dev_desc(a):
    """descriptor rows on the device; an empty set still needs a pointer"""
    return dev(a) if len(a) else torch.zeros((1, 32), dtype=torch.uint8, device="cuda")


def sp(stream):
    return C.c_void_p(stream.cuda_stream) if stream is not None else None


def i32(n, value):
    return torch.full((n,), value, dtype=torch.int32, device="cuda")


def flags(seed, n, p):
    return (np.random.default_rng(seed).random(n) < p).astype(np.uint8)


def next_pow2(n):
    p = 1
    while p < n:
        p <<= 1
    return p


# ---------------------------------------------------------------- the six entry points, each with sentinels behind its outputs; (status, outputs)
def run_knn(h, q, t, mem, stream=None):
    nq = len(q)
    dq, dt = dev(q), dev_desc(t)
    if mem == L.MEM_HOST:
        out = np.zeros(2 * nq + TAIL, L.DMATCH_DTYPE); out["imgIdx"][2 * nq:] = SENT
        st = L.lib().plf_match_lines_knn(h._h, L.vp(dq), nq, L.vp(dt), len(t), L.vp(out), L.MEM_HOST, sp(stream))
    else:
        buf = torch.full(((2 * nq + TAIL) * 16,), 0xAB, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        st = L.lib().plf_match_lines_knn(h._h, L.vp(dq), nq, L.vp(dt), len(t), L.vp(buf), L.MEM_DEVICE, sp(stream))
        torch.cuda.synchronize()
        raw = buf.cpu().numpy()
        assert np.all(raw[2 * nq * 16:] == 0xAB), "plf_match_lines_knn wrote behind its 2 * nq rows"
        out = raw.view(L.DMATCH_DTYPE)
    if mem == L.MEM_HOST:
        assert np.all(out["imgIdx"][2 * nq:] == SENT), "plf_match_lines_knn wrote behind its 2 * nq rows"
    return st, out[:2 * nq].reshape(nq, 2)


def check_knn(dm, idx, dist, what):
    assert np.array_equal(dm["trainIdx"], idx), what
    assert dm["distance"].tobytes() == dist.astype(np.float32).tobytes(), what
    assert np.array_equal(dm["queryIdx"], np.repeat(np.arange(len(idx), dtype=np.int32), 2).reshape(-1, 2)), what
    assert np.all(dm["imgIdx"] == 0), what


def run_mad(h, q, t, want_knn, mem, stream=None):
    n1 = len(q)
    dq, dt = dev(q), dev(t)
    if mem == L.MEM_HOST:
        mad = np.full(2 + 2, -1.0); knn = np.zeros((n1, 2), L.DMATCH_DTYPE) if want_knn else None
        st = L.lib().plf_line_descriptor_mad(h._h, L.vp(dq), n1, L.vp(dt), len(t), L.vp(knn), L.vp(mad), L.MEM_HOST, sp(stream))
    else:
        dmad = torch.full((2 + 2,), -1.0, dtype=torch.float64, device="cuda")
        dknn = torch.zeros((n1 * 2 * 16,), dtype=torch.uint8, device="cuda") if want_knn else None
        torch.cuda.synchronize()
        st = L.lib().plf_line_descriptor_mad(h._h, L.vp(dq), n1, L.vp(dt), len(t), L.vp(dknn), L.vp(dmad), L.MEM_DEVICE, sp(stream))
        torch.cuda.synchronize()
        mad = dmad.cpu().numpy(); knn = dknn.cpu().numpy().view(L.DMATCH_DTYPE).reshape(n1, 2) if want_knn else None
    assert np.all(mad[2:] == -1.0), "plf_line_descriptor_mad wrote behind its two doubles"
    return st, mad[:2].copy(), knn


def run_lastframe(h, q, t, has, stream=None):
    ncur = len(t)
    dq, dt, dh = dev(q), dev_desc(t), dev(has)
    match = torch.cat([i32(ncur, -1), i32(TAIL, SENT)]); nm = i32(1 + TAIL, SENT)
    torch.cuda.synchronize()
    st = L.lib().plf_match_lines_lastframe(h._h, L.vp(dq), len(q), L.vp(dt), ncur, L.vp(dh), L.vp(match), L.vp(nm), sp(stream))
    torch.cuda.synchronize()
    nm = nm.cpu().numpy()
    assert np.all(nm[1:] == SENT), "plf_match_lines_lastframe wrote behind nmatches"
    return st, match.cpu().numpy(), int(nm[0])


def check_lastframe(got, ref, what):
    (st, match, n), (rmatch, rn) = got, ref
    assert st == L.PLF_OK, "%s: status %d" % (what, st)
    assert n == rn, "%s: nmatches %d, oracle %d" % (what, n, rn)
    assert np.array_equal(match, np.concatenate([rmatch, np.full(TAIL, SENT, np.int32)])), what


def run_tri(h, q, t, h1, h2, s1, s2, only, factor, stream=None):
    """stereo arrays None: NULL pointers (only_stereo must be 0); match12 is documented as overwritten: it starts as garbage"""
    n1 = len(q)
    dq, dt, d1, d2 = dev(q), dev_desc(t), dev(h1), dev(h2)
    ds1 = dev(s1) if s1 is not None else None; ds2 = dev(s2) if s2 is not None else None
    garbage = np.random.default_rng(n1).integers(-5, 1 << 20, n1).astype(np.int32)
    match = torch.cat([dev(garbage), i32(TAIL, SENT)]); nm = i32(1 + TAIL, SENT)
    torch.cuda.synchronize()
    st = L.lib().plf_match_lines_triangulation(h._h, L.vp(dq), n1, L.vp(dt), len(t), L.vp(d1), L.vp(d2), L.vp(ds1), L.vp(ds2), int(only), C.c_float(factor),
                                               L.vp(match), L.vp(nm), sp(stream))
    torch.cuda.synchronize()
    nm = nm.cpu().numpy()
    assert np.all(nm[1:] == SENT), "plf_match_lines_triangulation wrote behind nmatches"
    return st, match.cpu().numpy(), int(nm[0])


def ref_tri(q, t, h1, h2, s1, s2, only, factor):
    z1, z2 = np.zeros(len(q), np.uint8), np.zeros(max(len(t), 1), np.uint8)
    # the C entry point takes the factor as a float: the oracle gets that float's value
    return orc.lines_search_for_triangulation(q, t, h1, h2, s1 if s1 is not None else z1, s2 if s2 is not None else z2, only, float(np.float32(factor)))


def run_fuse(h, kf, ml, valid, stream=None):
    mm = len(ml)
    dkf, dml, dv = dev_desc(kf), dev(ml), dev(valid)
    garbage = np.random.default_rng(mm).integers(-5, 1 << 20, mm).astype(np.int32)
    best = torch.cat([dev(garbage), i32(TAIL, SENT)]); nf = i32(1 + TAIL, SENT)
    torch.cuda.synchronize()
    st = L.lib().plf_match_lines_fuse(h._h, L.vp(dkf), len(kf), L.vp(dml), L.vp(dv), mm, L.vp(best), L.vp(nf), sp(stream))
    torch.cuda.synchronize()
    nf = nf.cpu().numpy()
    assert np.all(nf[1:] == SENT), "plf_match_lines_fuse wrote behind nfused"
    return st, best.cpu().numpy(), int(nf[0])


def run_batch(h, last, has, frames, mode, stride, stream=None):
    """mode 'n': the count in the view alone; 'dev<=n': the view holds the stride as an upper bound, the count is on the device; 'dev>n': the device
    count is 50 too large and must clamp to the view's.  Descriptor rows and match rows behind a frame's count hold sentinels."""
    B = len(frames)
    desc = np.full((B, stride, 32), 0xCD, np.uint8); init = np.full((B, stride), SENT, np.int32)
    for f, F in enumerate(frames):
        desc[f, :len(F)] = F; init[f, :len(F)] = -1
    counts = np.asarray([len(F) for F in frames], np.int32)
    ddesc, dlast, dhas = dev(desc), dev(last), dev(has)
    dn = dev(counts + 50 if mode == "dev>n" else counts)
    views = [Matcher.lineframe_view(stride if mode == "dev<=n" else counts[f], 0, ddesc.data_ptr() + f * stride * 32, 0,
                                    None if mode == "n" else dn.data_ptr() + 4 * f) for f in range(B)]
    arr = Matcher.view_array(views, L.LineFrameView)
    match = torch.cat([dev(init).reshape(-1), i32(TAIL, SENT)]); nm = i32(B + TAIL, SENT)
    torch.cuda.synchronize()
    st = L.lib().plf_match_lines_lastframe_batch(h._h, L.vp(dlast), len(last), L.vp(dhas), arr, B, L.vp(match), stride, L.vp(nm), sp(stream))
    torch.cuda.synchronize()
    match, nm = match.cpu().numpy(), nm.cpu().numpy()
    assert np.all(match[B * stride:] == SENT) and np.all(nm[B:] == SENT), "plf_match_lines_lastframe_batch wrote behind its outputs"
    return st, match[:B * stride].reshape(B, stride), nm[:B], init


def check_batch(got, refs, what):
    """refs[f] = the oracle's (match, n) of frame f, None for a frame of fewer than two lines: its whole row stays as it was"""
    st, match, nm, init = got
    assert st == L.PLF_OK, "%s: status %d" % (what, st)
    for f, ref in enumerate(refs):
        want = init[f].copy()
        if ref is not None:
            want[:len(ref[0])] = ref[0]
        assert nm[f] == (ref[1] if ref is not None else 0), "%s frame %d: nmatches %d" % (what, f, nm[f])
        assert np.array_equal(match[f], want), "%s frame %d" % (what, f)


# ---------------------------------------------------------------- sizes: all six entry points at every boundary of the sort and of the grid
@pytest.mark.parametrize("name", ["nq%d_nt%d" % p for p in lc.SIZE_PAIRS])
def test_sizes_all_entry_points(m, name):
    c = case(name)
    q, t, has = c["query"], c["train"], c["has_mapline"]
    nq, nt = len(q), len(t)
    idx, dist = ref_knn(c)
    for mem in (L.MEM_HOST, L.MEM_DEVICE):
        st, dm = run_knn(m, q, t, mem)
        assert st == L.PLF_OK
        check_knn(dm, idx, dist, "knn mem %d" % mem)
    if nt >= 2:
        want = np.asarray(orc.line_mad(dist), np.float64).tobytes()
        for mem in (L.MEM_HOST, L.MEM_DEVICE):
            for want_knn in (True, False):
                st, mad, knn = run_mad(m, q, t, want_knn, mem)
                assert st == L.PLF_OK
                assert mad.tobytes() == want, "mad mem %d knn %d: %r, oracle %r" % (mem, want_knn, mad.tolist(), orc.line_mad(dist))
                if want_knn:
                    check_knn(knn, idx, dist, "mad's knn mem %d" % mem)
    else:
        assert L.lib().plf_line_descriptor_mad(m._h, L.vp(dev(q)), nq, L.vp(dev(t)), nt, None, L.vp(np.zeros(2)), L.MEM_HOST, None) == L.PLF_E_BADARG
    ref = ref_last(name, q, t, has)
    check_lastframe(run_lastframe(m, q, t, has), ref, "lastframe")
    check_batch(run_batch(m, q, has, [t], "n", nt + 7), [ref if nt >= 2 else None], "batch of one")
    h1, h2, s1, s2 = flags(1, nq, 0.3), flags(2, nt, 0.3), flags(3, nq, 0.8), flags(4, nt, 0.8)
    for only, a1, a2 in ((0, None, None), (1, s1, s2)):
        rmatch, rn = ref_tri(q, t, h1, h2, a1, a2, only, 0.1)
        st, match, n = run_tri(m, q, t, h1, h2, a1, a2, only, 0.1)
        assert st == L.PLF_OK and n == rn, "triangulation only_stereo %d: %d pairs, oracle %d" % (only, n, rn)
        assert np.array_equal(match, np.concatenate([rmatch, np.full(TAIL, SENT, np.int32)])), "triangulation only_stereo %d" % only
    valid = flags(5, nq, 0.8)
    rbest, rn = orc.lines_fuse(t, q, valid)
    st, best, n = run_fuse(m, t, q, valid)
    assert st == L.PLF_OK and n == rn and np.array_equal(best, np.concatenate([rbest, np.full(TAIL, SENT, np.int32)])), "fuse"


# ---------------------------------------------------------------- a zero spread, the upper median and contended train lines
@pytest.mark.parametrize("name", ["zero_mad_nq301", "zero_mad_nq300", "median_split_nq4", "median_split_nq256", "shared_train"])
def test_zero_spread_and_shared_trains(m, name):
    c = case(name)
    q, t, has = c["query"], c["train"], c["has_mapline"]
    nq, nt = len(q), len(t)
    idx, dist = ref_knn(c)
    st, mad, knn = run_mad(m, q, t, True, L.MEM_HOST)
    assert st == L.PLF_OK and mad.tobytes() == np.asarray(orc.line_mad(dist), np.float64).tobytes()
    check_knn(knn, idx, dist, "mad's knn")
    ref = ref_last(name, q, t, has)
    got = run_lastframe(m, q, t, has)
    check_lastframe(got, ref, "lastframe")
    if name == "shared_train":
        assert got[2] > 300 and [got[1][tr] for tr in lc.SHARED_TRAINS] == [c["winner"][tr] for tr in lc.SHARED_TRAINS]
    elif name.startswith("zero_mad"):
        assert mad[1] == 0.0 and got[2] == int((dist[:, 1] > dist[:, 0]).sum())
    else:
        assert mad[1] == 1.4826 * 30 and got[2] == nq // 2
    check_batch(run_batch(m, q, has, [t, t[:1], t], "n", nt + 3), [ref, None, ref], "batch")
    h1, h2, s1, s2 = flags(11, nq, 0.3), flags(12, nt, 0.3 if nt > 2 else 0.0), flags(13, nq, 0.8), flags(14, nt, 0.8 if nt > 2 else 1.0)
    for only, a1, a2 in ((0, None, None), (1, s1, s2)):
        for factor in (0.0, 0.1, 1e6):
            rmatch, rn = ref_tri(q, t, h1, h2, a1, a2, only, factor)
            st, match, n = run_tri(m, q, t, h1, h2, a1, a2, only, factor)
            what = "triangulation only_stereo %d mad_factor %g" % (only, factor)
            assert st == L.PLF_OK and n == rn, "%s: %d pairs, oracle %d" % (what, n, rn)
            assert np.array_equal(match, np.concatenate([rmatch, np.full(TAIL, SENT, np.int32)])), what
            if factor == 1e6 and not name.startswith("zero_mad"):   # (a zero spread times any factor is a zero threshold: the zero_mad sets keep their pairs)
                assert n == 0 and np.all(match[:nq] == -1), what
            elif only == 0 and nq >= 100:
                assert n > 20, what


# ---------------------------------------------------------------- the 128-descriptor tile of the batch kernel
@pytest.mark.parametrize("nlast", lc.BATCH_NLAST)
def test_batch_tile_edges_counts_and_clamp(m, nlast):
    c = once(("ties", nlast), lambda: lc.tile_ties(nlast))
    last, has, frames = c["last"], c["has_mapline"], c["frames"]
    refs = [ref_last("%s_%d" % (c["name"], f), last, F, has) if len(F) >= 2 else None for f, F in enumerate(frames)]
    assert sum(r[1] for r in refs if r is not None) > nlast
    # the 2-NN tables behind the frames, through the single-frame kernel and through the oracle
    for f, F in enumerate(frames):
        if len(F):
            st, dm = run_knn(m, last, F, L.MEM_HOST)
            assert st == L.PLF_OK
            check_knn(dm, *orc.knn2(last, F), what="knn frame %d" % f)
    for mode in ("n", "dev<=n", "dev>n"):
        check_batch(run_batch(m, last, has, frames, mode, 320), refs, "%s mode %s" % (c["name"], mode))
    # every frame alone through the single-frame call
    for f, F in enumerate(frames):
        ref = refs[f] if refs[f] is not None else (np.full(len(F), -1, np.int32), 0)
        check_lastframe(run_lastframe(m, last, F, has), ref, "frame %d alone" % f)


# ---------------------------------------------------------------- Fuse at TH_LOW
@pytest.mark.parametrize("name", ["fuse_m%d_nkf129" % mm for mm in lc.FUSE_M] + ["fuse_m65_nkf%d" % k for k in lc.FUSE_NKF if k != 129])
def test_fuse_edges(m, name):
    c = case(name)
    rbest, rn = orc.lines_fuse(c["kf"], c["ml"], c["valid"])
    st, best, n = run_fuse(m, c["kf"], c["ml"], c["valid"])
    assert st == L.PLF_OK and n == rn, "%d fused, oracle %d" % (n, rn)
    assert np.array_equal(best, np.concatenate([rbest, np.full(TAIL, SENT, np.int32)]))
    if len(c["kf"]):
        assert np.array_equal(best[:len(rbest)] >= 0, (c["flips"] <= lc.TH_LOW) & (c["valid"] != 0))
    else:
        assert n == 0 and np.all(best[:len(rbest)] == -1)


# ---------------------------------------------------------------- max_lines = 18000: the sort at 16384 / 32768 slots, 64 KB and 128 KB of dynamic LDS
@pytest.mark.parametrize("nq", lc.LARGE_NQ)
def test_large_query_sets(big, nq):
    c = once(("large", nq), lambda: lc.large(nq))
    q, t, has = c["query"], c["train"], c["has_mapline"]
    lds = "%d queries, %d KB of dynamic LDS" % (nq, next_pow2(nq) * 4 // 1024)
    h1, h2 = flags(21, nq, 0.3), flags(22, 3, 0.0)
    last = run_lastframe(big, q, t, has)
    assert last[0] == L.PLF_OK, "plf_match_lines_lastframe (k_lines_lastframe, %s) returned %d: the launch failed" % (lds, last[0])
    tri = run_tri(big, q, t, h1, h2, None, None, 0, 0.1)
    assert tri[0] == L.PLF_OK, "plf_match_lines_triangulation (k_lines_lastframe, %s) returned %d: the launch failed" % (lds, tri[0])
    mad = run_mad(big, q, t, True, L.MEM_HOST)
    assert mad[0] == L.PLF_OK, "plf_line_descriptor_mad (k_line_mad, %s) returned %d: the launch failed" % (lds, mad[0])
    idx, dist = orc.knn2(q, t)
    check_lastframe(last, orc.match_lines_knn(q, t, has), "lastframe, " + lds)
    assert last[2] > nq // 3
    rmatch, rn = ref_tri(q, t, h1, h2, None, None, 0, 0.1)
    assert tri[2] == rn and rn > nq // 2 and np.array_equal(tri[1], np.concatenate([rmatch, np.full(TAIL, SENT, np.int32)])), "triangulation, " + lds
    assert mad[1].tobytes() == np.asarray(orc.line_mad(dist), np.float64).tobytes(), "mad, %s: %r, oracle %r" % (lds, mad[1].tolist(), orc.line_mad(dist))
    check_knn(mad[2], idx, dist, "mad's knn, " + lds)


def test_large_train_set(big):
    c = once("large_train", lc.large_train)
    q, t, has = c["query"], c["train"], c["has_mapline"]
    idx, dist = orc.knn2(q, t)
    for mem in (L.MEM_HOST, L.MEM_DEVICE):
        st, dm = run_knn(big, q, t, mem)
        assert st == L.PLF_OK
        check_knn(dm, idx, dist, "knn mem %d" % mem)
    check_lastframe(run_lastframe(big, q, t, has), orc.match_lines_knn(q, t, has), "lastframe, 18000 current lines")
    st, mad, _ = run_mad(big, q, t, False, L.MEM_DEVICE)
    assert st == L.PLF_OK and mad.tobytes() == np.asarray(orc.line_mad(dist), np.float64).tobytes()
    h1, h2 = flags(31, len(q), 0.3), flags(32, len(t), 0.3)
    rmatch, rn = ref_tri(q, t, h1, h2, None, None, 0, 0.1)
    st, match, n = run_tri(big, q, t, h1, h2, None, None, 0, 0.1)
    assert st == L.PLF_OK and n == rn and np.array_equal(match[:len(q)], rmatch)
    valid = flags(33, len(q), 0.8)
    rbest, rn = orc.lines_fuse(t, q, valid)
    st, best, n = run_fuse(big, t, q, valid)
    assert st == L.PLF_OK and n == rn and 0 < rn < valid.sum() and np.array_equal(best[:len(q)], rbest)


# ---------------------------------------------------------------- a caller's stream
def test_twice_on_a_callers_stream(m):
    s = torch.cuda.Stream()
    c = case("shared_train")
    q, t, has = c["query"], c["train"], c["has_mapline"]
    f = case("fuse_m257_nkf129")
    ties = once(("ties", 129), lambda: lc.tile_ties(129))
    h1, h2 = flags(41, len(q), 0.3), flags(42, len(t), 0.3)
    runs = []
    for rep in range(2):
        knn = run_knn(m, q, t, L.MEM_DEVICE, s)
        mad = run_mad(m, q, t, True, L.MEM_DEVICE, s)
        last = run_lastframe(m, q, t, has, s)
        tri = run_tri(m, q, t, h1, h2, None, None, 0, 0.1, s)
        fuse = run_fuse(m, f["kf"], f["ml"], f["valid"], s)
        batch = run_batch(m, ties["last"], ties["has_mapline"], ties["frames"], "dev<=n", 320, s)
        assert [r[0] for r in (knn, mad, last, tri, fuse, batch)] == [L.PLF_OK] * 6
        runs.append(b"".join(np.ascontiguousarray(a).tobytes() for a in (knn[1], mad[1], mad[2], last[1], tri[1], fuse[1], batch[1], batch[2])) +
                    bytes([last[2] & 0xFF, tri[2] & 0xFF, fuse[2] & 0xFF]))
        if rep == 0:   # ... and the first run is the oracle's
            idx, dist = ref_knn(c)
            check_knn(knn[1], idx, dist, "knn on a stream")
            assert mad[1].tobytes() == np.asarray(orc.line_mad(dist), np.float64).tobytes()
            check_lastframe(last, ref_last("shared_train", q, t, has), "lastframe on a stream")
            rmatch, rn = ref_tri(q, t, h1, h2, None, None, 0, 0.1)
            assert tri[2] == rn and np.array_equal(tri[1][:len(q)], rmatch)
            rbest, rn = orc.lines_fuse(f["kf"], f["ml"], f["valid"])
            assert fuse[2] == rn and np.array_equal(fuse[1][:len(rbest)], rbest)
            refs = [ref_last("%s_%d" % (ties["name"], k), ties["last"], F, ties["has_mapline"]) if len(F) >= 2 else None for k, F in enumerate(ties["frames"])]
            check_batch(batch, refs, "batch on a stream")
    assert runs[0] == runs[1]

"""The host side of the matchers (csrc/match_host.hip): what every entry point refuses, what the calls that have nothing to do write, the host mirror of
the frame tables, two streams on one handle, and the knobs a handle reads when it is created.  Results are compared with the sequential oracle, bit-exact."""
import ctypes as C
import functools

import numpy as np
import pytest

import kfgen
import matchgen
import orc
from conftest import gpu_available

pytestmark = pytest.mark.gpu

BOUNDS = (0.0, 0.0, 640.0, 480.0)


def _need_gpu():
    if not gpu_available():
        pytest.fail("no GPU visible: the -m gpu tests need a real MI355X")


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bytes(a):
    import torch
    return torch.from_numpy(np.frombuffer(np.ascontiguousarray(a).tobytes(), np.uint8).copy()).cuda()


# ---------------------------------------------------------------- refusals
def _f(x):
    return C.c_float(x)


class _Args(dict):
    """the arguments of one call by name, in the order of the C signature; structures go by reference"""
    def call(self, fn):
        return fn(*[C.byref(v) if isinstance(v, C.Structure) else v for v in self.values()])


def null(*keys):
    return [("%s null" % k, lambda d, k=k: d.__setitem__(k, None)) for k in keys]


def val(key, *values):
    return [("%s = %r" % (key, v), lambda d, k=key, v=v: d.__setitem__(k, v)) for v in values]


def fld(key, name, *values, i=None):
    """field `name` of the structure (element i of the array) `key`"""
    def put(d, v):
        setattr(d[key] if i is None else d[key][i], name, v)
    return [("%s%s.%s = %r" % (key, "" if i is None else "[%d]" % i, name, v), lambda d, v=v: put(d, v)) for v in values]


def both(label, *muts):
    """several changes that only together reach one clause"""
    def put(d):
        for group in muts:
            for _, m in group:
                m(d)
    return [(label, put)]


BAD_BOUNDS_X = [("min_x", 640.0), ("max_x", -1.0)]   # empty, inverted
BAD_BOUNDS_Y = [("min_y", 480.0), ("max_y", -1.0)]


def bounds(key, i=None):
    return [m for name, v in BAD_BOUNDS_X + BAD_BOUNDS_Y for m in fld(key, name, v, i=i)]


def staged_kf(key, nlevels=(0, 17)):
    """the clauses of stage_keyframe on the frame view `key`"""
    return fld(key, "n", -1, 65) + bounds(key) + (fld(key, "nlevels", *nlevels) if nlevels else [])


def _refusal_table(L, h, h_mp32, h_kp32, zp):
    """[(entry point, good arguments, [(what is wrong, change)])]: every change alone makes the parent's entry point return PLF_E_BADARG.  h: 64 key points,
    64 map points, 64 lines, 2 frames; h_mp32 / h_kp32: 32 map points / 32 key points, to reach one size clause of plf_match_sim3 without the other.
    zp: a zeroed device buffer, the stand-in of every pointer that a refused call never follows."""
    from rgbd_pl_slam_amd import _lib as P
    host = np.zeros(64, np.float32)
    hp = P.vp(host)
    grid = np.zeros(64 * 48 + 1, np.int32)

    def fv(n=32):
        return P.FrameView(n, None, zp.value, zp.value, zp.value, 0.0, 0.0, 640.0, 480.0, zp.value, 8)

    def lfv(n=32):
        return P.LineFrameView(n, None, zp.value, zp.value, zp.value)

    def arr(*views):
        return (type(views[0]) * len(views))(*views)

    def mpv(m=32):
        return P.MapPointView(m, *([zp.value] * 8))

    def mlv(m=32):
        return P.MapLineView(m, *([zp.value] * 8))

    def lastv(n=32):
        return P.LastFrameView(n, *([zp.value] * 6))

    def pose_pair():
        return P.PosePair()

    def kf_pose(log_scale=0.18):
        k = P.KfPose()
        k.fx = k.fy = 500.0; k.cx = 320.0; k.cy = 240.0; k.log_scale_factor = log_scale; k.inv_level_sigma2 = hp.value
        return k

    def pts(m=32):
        return P.Points3DView(m, *([zp.value] * 6))

    def bowv():
        v = P.BowView()
        v.n_kf = 32; v.n_f = 32; v.kf_nodes = 4; v.f_nodes = 4
        for name, _ in P.BowView._fields_:
            if name not in ("n_kf", "n_f", "kf_nodes", "f_nodes"):
                setattr(v, name, zp.value)
        return v

    def triv():
        v = P.TriView()
        v.n1 = 32; v.n2 = 32; v.nodes1 = 4; v.nodes2 = 4
        for name, _ in P.TriView._fields_:
            if name not in ("n1", "n2", "nodes1", "nodes2"):
                setattr(v, name, zp.value)
        return v

    PTS_FIELDS = ("world_pos", "normal", "min_distance", "max_distance", "desc", "valid")
    T = []

    def project_points():
        return _Args(h=h, frames=arr(fv(), fv()), n_frames=2, mp=mpv(), th=_f(3.0), nnratio=_f(0.8), match_of_kp=zp, kp_stride=32, nmatches=zp, stream=None)
    T.append((L.plf_match_project_points, project_points,
              null("h", "frames", "mp", "match_of_kp", "nmatches") + val("n_frames", 0, -1, 3) + fld("mp", "m", -1, 65) +
              fld("frames", "n", -1, 65, i=1) + val("kp_stride", 31) + bounds("frames", i=1) + bounds("frames", i=0)))

    def bow():
        return _Args(h=h, pairs=arr(bowv(), bowv()), n_pairs=2, nnratio=_f(0.7), check_orientation=1, match=zp, stride=32, nmatches=zp, stream=None)
    bow_rows = (null("h", "pairs", "match", "nmatches") + val("n_pairs", 0, 3) + val("stride", 0, 65) + fld("pairs", "n_kf", -1, i=1) +
                fld("pairs", "n_f", -1, 33, i=1) + fld("pairs", "kf_nodes", -1, i=0) + fld("pairs", "f_nodes", -1, i=0))
    T.append((L.plf_match_bow, bow, bow_rows))
    T.append((L.plf_match_bow_kf, bow, bow_rows + fld("pairs", "n_kf", 33, i=1) + fld("pairs", "f_has_mp", None, i=0)))   # the keyframe overload's own rule

    def triangulation():
        return _Args(h=h, v=triv(), F12=hp, Cw1=hp, pose2=kf_pose(), only_stereo=0, check_orientation=1, match12=zp, nmatches=zp, stream=None)
    T.append((L.plf_match_triangulation, triangulation,
              null("h", "v", "F12", "Cw1", "pose2", "match12", "nmatches") + fld("v", "n1", -1, 65) + fld("v", "n2", -1, 65) + fld("v", "nodes1", -1) +
              fld("v", "nodes2", -1) + [m for name in ("has_mp1", "has_mp2", "uright1", "uright2", "keys1", "keys2", "scale_factors2", "level_sigma2_2")
                                        for m in fld("v", name, None)]))

    def lastframe():
        return _Args(h=h, cur=fv(), last=lastv(), pose=pose_pair(), th=_f(15.0), mono=0, check_orientation=1, match_of_kp=zp, nmatches=zp, stream=None)
    last_rows = fld("last", "n", -1, 65) + fld("last", "has_mappoint", None) + fld("last", "outlier", None)
    T.append((L.plf_match_project_lastframe, lastframe,
              null("h", "cur", "last", "pose", "match_of_kp", "nmatches") + last_rows + fld("cur", "n", -1, 65) + bounds("cur")))

    def lastframe_batch():
        return _Args(h=h, frames=arr(fv(), fv()), n_frames=2, last=lastv(), poses=(P.PosePair * 2)(), th=_f(15.0), mono=0, check_orientation=1, match_of_kp=zp,
                     kp_stride=32, nmatches=zp, stream=None)
    T.append((L.plf_match_project_lastframe_batch, lastframe_batch,
              null("h", "frames", "last", "poses", "match_of_kp", "nmatches") + val("n_frames", 0, 3) + last_rows + fld("frames", "n", -1, 65, i=1) +
              val("kp_stride", 31) + bounds("frames", i=1)))

    def keyframe():
        return _Args(h=h, cur=fv(), kf=lastv(), min_distance=zp, max_distance=zp, pose=pose_pair(), log_scale_factor=_f(0.18), th=_f(10.0), orb_dist=100,
                     check_orientation=1, match_of_kp=zp, nmatches=zp, stream=None)
    T.append((L.plf_match_project_keyframe, keyframe,
              null("h", "cur", "kf", "min_distance", "max_distance", "pose", "match_of_kp", "nmatches") +
              val("log_scale_factor", _f(0.0), _f(-0.18), _f(float("nan"))) + fld("cur", "nlevels", 0, 65) + fld("kf", "n", -1, 65) +
              fld("kf", "has_mappoint", None) + fld("cur", "n", -1, 65) + bounds("cur")))

    def assign_grid():
        return _Args(h=h, frame=fv(), cell_start=P.vp(grid), cell_idx=P.vp(grid), stream=None)
    T.append((L.plf_match_assign_grid, assign_grid, null("h", "frame", "cell_start", "cell_idx") + staged_kf("frame", nlevels=(17,))))

    def pts_rows(key):
        return fld(key, "m", -1, 65) + [m for name in PTS_FIELDS for m in fld(key, name, None)]

    def fuse():
        return _Args(h=h, kf=fv(), pose=kf_pose(), pts=pts(), th=_f(3.0), best_idx=zp, nfused=zp, stream=None)
    T.append((L.plf_match_fuse, fuse,
              null("h", "kf", "pose", "pts", "best_idx", "nfused") + pts_rows("pts") + fld("pose", "log_scale_factor", 0.0, -1.0) + staged_kf("kf")))

    def fuse_sim3():
        return _Args(h=h, kf=fv(), Scw=hp, intr=kf_pose(), pts=pts(), th=_f(3.0), best_idx=zp, nfused=zp, stream=None)
    sim3_rows = pts_rows("pts") + fld("intr", "log_scale_factor", 0.0, -1.0) + staged_kf("kf")
    T.append((L.plf_match_fuse_sim3, fuse_sim3, null("h", "kf", "Scw", "intr", "pts", "best_idx", "nfused") + sim3_rows))

    def project_sim3():
        return _Args(h=h, kf=fv(), Scw=hp, intr=kf_pose(), pts=pts(), th=3, match_of_kp=zp, nmatches=zp, stream=None)
    T.append((L.plf_match_project_sim3, project_sim3, null("h", "kf", "Scw", "intr", "pts", "match_of_kp", "nmatches") + sim3_rows))

    def sim3(handle=h):
        return _Args(h=handle, kf1=fv(), kf2=fv(), pose1=kf_pose(), pose2=kf_pose(), s12=_f(1.0), R12=hp, t12=hp, th=_f(7.5), pts1=pts(), pts2=pts(),
                     match12=zp, nfound=zp, stream=None)
    # (the clauses of stage_keyframe on kf1 come after the first direction's launches: not in this table)
    T.append((L.plf_match_sim3, sim3,
              null("h", "kf1", "kf2", "pose1", "pose2", "R12", "t12", "pts1", "pts2", "match12", "nfound") + fld("pts1", "m", 31) + fld("pts2", "m", 31) +
              both("kf1.n = pts1.m = -1", fld("kf1", "n", -1), fld("pts1", "m", -1)) + both("kf2.n = pts2.m = -1", fld("kf2", "n", -1), fld("pts2", "m", -1)) +
              val("s12", _f(0.0), _f(-1.0)) + fld("pose1", "log_scale_factor", 0.0) + fld("pose2", "log_scale_factor", 0.0) +
              bounds("kf2") + fld("kf2", "nlevels", 0, 17)))
    for handle, what in ((h_mp32, "max_mp"), (h_kp32, "max_kp")):
        T.append((L.plf_match_sim3, functools.partial(sim3, handle),
                  both("kf1.n = pts1.m = 40 > %s" % what, fld("kf1", "n", 40), fld("pts1", "m", 40)) +
                  both("kf2.n = pts2.m = 40 > %s" % what, fld("kf2", "n", 40), fld("pts2", "m", 40))))

    def lines_knn():
        return _Args(h=h, query=zp, nq=8, train=zp, nt=8, out=zp, mem=P.MEM_DEVICE, stream=None)
    T.append((L.plf_match_lines_knn, lines_knn, null("h", "query", "train", "out") + val("nq", 0, 65) + val("nt", 0)))

    def line_mad():
        return _Args(h=h, ldesc1=zp, n1=8, ldesc2=zp, n2=8, knn=zp, mad=zp, mem=P.MEM_DEVICE, stream=None)
    T.append((L.plf_line_descriptor_mad, line_mad, null("h", "ldesc1", "ldesc2", "mad") + val("n1", 0, 65) + val("n2", 1)))

    def lines_lastframe():
        return _Args(h=h, last_desc=zp, nlast=8, cur_desc=zp, ncur=8, last_has_mapline=zp, match_of_line=zp, nmatches=zp, stream=None)
    T.append((L.plf_match_lines_lastframe, lines_lastframe,
              null("h", "last_desc", "cur_desc", "last_has_mapline", "match_of_line", "nmatches") + val("nlast", 65) + val("ncur", 65)))

    def lines_lastframe_batch():
        return _Args(h=h, last_desc=zp, nlast=8, last_has_mapline=zp, frames=arr(lfv(), lfv()), n_frames=2, match_of_line=zp, line_stride=32, nmatches=zp,
                     stream=None)
    T.append((L.plf_match_lines_lastframe_batch, lines_lastframe_batch,
              null("h", "last_desc", "last_has_mapline", "frames", "match_of_line", "nmatches") + val("nlast", 65) + val("n_frames", 0, 3) +
              fld("frames", "n", -1, 65, i=1) + val("line_stride", 31) + fld("frames", "desc", None, i=1)))

    def lines_triangulation():
        return _Args(h=h, desc1=zp, n1=8, desc2=zp, n2=8, has_ml1=zp, has_ml2=zp, stereo1=zp, stereo2=zp, only_stereo=1, mad_factor=_f(0.1), match12=zp,
                     nmatches=zp, stream=None)
    T.append((L.plf_match_lines_triangulation, lines_triangulation,
              null("h", "desc1", "desc2", "has_ml1", "has_ml2", "stereo1", "stereo2", "match12", "nmatches") + val("n1", -1, 65) + val("n2", -1, 65) +
              val("mad_factor", _f(-0.1), _f(float("nan")))))

    def lines_fuse():
        return _Args(h=h, kf_desc=zp, n_kf=8, ml_desc=zp, valid=zp, m=8, best_idx=zp, nfused=zp, stream=None)
    T.append((L.plf_match_lines_fuse, lines_fuse,
              null("h", "kf_desc", "ml_desc", "valid", "best_idx", "nfused") + val("n_kf", -1, 65) + val("m", -1, 65)))

    def project_lines():
        return _Args(h=h, frames=arr(lfv(), lfv()), n_frames=2, ml=mlv(), th=_f(3.0), nnratio=_f(0.8), match_of_line=zp, line_stride=32, nmatches=zp, stream=None)
    T.append((L.plf_match_project_lines, project_lines,
              null("h", "frames", "ml", "match_of_line", "nmatches") + val("n_frames", 0, 3) + fld("ml", "m", -1, 65) + fld("frames", "n", -1, 65, i=1) +
              val("line_stride", 31)))

    def hamming_matrix():
        return _Args(a=zp, na=4, b=zp, nb=4, dist=zp, mem=P.MEM_DEVICE, device=0, stream=None)
    T.append((L.plf_hamming256_matrix, hamming_matrix, null("a", "b", "dist") + val("na", 0) + val("nb", 0)))
    return T


def _small_scene():
    """48 key points of a synthetic frame and 60 map points: the valid call that follows the refusals"""
    from rgbd_pl_slam_amd.synth import synth_frame
    r = orc.orb_extract(synth_frame(3), nfeatures=200)
    kps, desc = r["kps"][:48].copy(), r["desc"][:48].copy()
    scale = orc.orb_tables(200, 1.2, 8)["scale"]
    mp = matchgen.make_local_map(kps, desc, 60, 17)
    init = np.full(len(kps), -1, np.int32); init[::9] = -2
    return kps, desc, scale, mp, init, orc.search_by_projection_map(kps, desc, None, scale, BOUNDS, mp, 3.0, 0.8, init)


def test_every_entry_point_refuses_bad_arguments_and_keeps_the_handle_usable():
    """One row per clause of the entry points' `return PLF_E_BADARG`: every required pointer null, every count below its minimum and above the handle's size,
    empty and inverted frame bounds, the scale / level / factor ranges, the keyframe overload's f_has_mp rule, pts1->m != kf1->n.  No refused call launches a
    kernel.  Then the calls that have nothing to do and what they write, and one valid call on the same handle against the oracle."""
    _need_gpu()
    import torch
    from rgbd_pl_slam_amd import Matcher, _lib as P
    L = P.lib()
    # plf_matcher_create
    out = C.c_void_p(0x1234)
    assert L.plf_matcher_create(0, 64, 64, 64, 2, None) == P.PLF_E_BADARG
    for args in ((0, 0, 64, 64, 2), (0, 64, 0, 64, 2), (0, 64, 64, 0, 2), (0, 64, 64, 64, 0), (0, 18001, 64, 64, 2), (0, 64, 64, 18001, 2), (-1, 64, 64, 64, 2),
                 (4096, 64, 64, 64, 2)):
        assert L.plf_matcher_create(*args, C.byref(out)) == P.PLF_E_BADARG, args
    assert not out.value    # (the refusals after the size clauses clear *out)
    L.plf_matcher_destroy(None)
    m = Matcher(max_keypoints=64, max_mappoints=64, max_lines=64, max_batch=2)
    m_mp32 = Matcher(max_keypoints=64, max_mappoints=32, max_lines=64, max_batch=2)
    m_kp32 = Matcher(max_keypoints=32, max_mappoints=64, max_lines=64, max_batch=2)
    zeros = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    zp = C.c_void_p(zeros.data_ptr())
    torch.cuda.synchronize()
    rows = 0
    for fn, good, muts in _refusal_table(L, m._h, m_mp32._h, m_kp32._h, zp):
        for what, change in muts:
            d = good()
            change(d)
            assert d.call(fn) == P.PLF_E_BADARG, "%s: %s" % (fn.__name__, what)
            rows += 1
    assert rows > 250
    # nothing to do: PLF_OK, the counter zeroed, line triangulation's match12 all -1
    h = m._h
    nm = torch.full((2,), 77, dtype=torch.int32, device="cuda"); match = torch.full((8,), 5, dtype=torch.int32, device="cuda")
    nmp, mtp = P.vp(nm), P.vp(match)
    torch.cuda.synchronize()

    def counters():
        torch.cuda.synchronize()
        got = nm.cpu().numpy().copy()
        nm.fill_(77)
        torch.cuda.synchronize()   # (the calls run on the handle's own stream)
        return got
    assert L.plf_match_lines_lastframe(h, zp, 0, zp, 8, zp, mtp, nmp, None) == P.PLF_OK and counters().tolist() == [0, 77]
    assert L.plf_match_lines_lastframe(h, zp, 8, zp, 1, zp, mtp, nmp, None) == P.PLF_OK and counters().tolist() == [0, 77]
    lframes = (P.LineFrameView * 2)(P.LineFrameView(8, None, zp.value, zp.value, zp.value), P.LineFrameView(8, None, zp.value, zp.value, zp.value))
    assert L.plf_match_lines_lastframe_batch(h, zp, 0, zp, lframes, 2, mtp, 8, nmp, None) == P.PLF_OK and counters().tolist() == [0, 0]
    assert L.plf_match_lines_fuse(h, zp, 8, zp, zp, 0, mtp, nmp, None) == P.PLF_OK and counters().tolist() == [0, 77]
    assert L.plf_match_lines_triangulation(h, zp, 0, zp, 8, zp, zp, zp, zp, 0, _f(0.1), mtp, nmp, None) == P.PLF_OK and counters().tolist() == [0, 77]
    assert (match.cpu().numpy() == 5).all()     # n1 == 0: no entry of match12 to fill
    assert L.plf_match_lines_triangulation(h, zp, 8, zp, 1, zp, zp, zp, zp, 0, _f(0.1), mtp, nmp, None) == P.PLF_OK and counters().tolist() == [0, 77]
    assert (match.cpu().numpy() == -1).all()
    # the handle after all that: a valid call gives the oracle's result
    kps, desc, scale, mp, init, (ref_match, ref_n) = _small_scene()
    assert ref_n > 5
    dk = _bytes(kps); dd = _dev(desc); ds = _dev(scale); dmp = {k: _dev(v) for k, v in mp.items()}
    got = _dev(init); cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    m.SearchByProjection([Matcher.frame_view(len(kps), dk, dd, ds, BOUNDS)], dmp, 3.0, 0.8, got, len(kps), cnt)
    torch.cuda.synchronize()
    assert int(cnt[0]) == ref_n and np.array_equal(got.cpu().numpy(), ref_match)
    for mm in (m, m_mp32, m_kp32):
        mm.close()


# ---------------------------------------------------------------- frame-table mirror, streams
@functools.lru_cache(maxsize=None)
def _point_frame(seed):
    """a frame of about 200 key points and the match array a search starts from"""
    from rgbd_pl_slam_amd.synth import synth_frame
    r = orc.orb_extract(synth_frame(seed), nfeatures=200)
    init = np.full(len(r["kps"]), -1, np.int32); init[::13] = -2
    return r["kps"], r["desc"], init


@functools.lru_cache(maxsize=None)
def _point_map():
    """300 map points around the key points of frames 0 and 1"""
    return matchgen.make_local_map(np.concatenate([_point_frame(0)[0], _point_frame(1)[0]]), np.concatenate([_point_frame(0)[1], _point_frame(1)[1]]), 300, 40)


@functools.lru_cache(maxsize=None)
def _scale():
    return orc.orb_tables(200, 1.2, 8)["scale"]


@functools.lru_cache(maxsize=None)
def _map_ref(seed, n):
    """oracle: the first n key points of frame `seed` against the map"""
    kps, desc, init = _point_frame(seed)
    match, cnt = orc.search_by_projection_map(kps[:n], desc[:n], None, _scale(), BOUNDS, _point_map(), 3.0, 0.8, init[:n])
    assert cnt > 10
    return match, cnt


class _PointFrames:
    """device copies of frames 0 and 1 and of the map; SearchByProjection of any list of (frame, n) against the map, checked against the oracle"""
    STRIDE = 512

    def __init__(self):
        from rgbd_pl_slam_amd import Matcher
        self.Matcher = Matcher
        self.ds = _dev(_scale())
        self.dev = {s: (_bytes(_point_frame(s)[0]), _dev(_point_frame(s)[1])) for s in (0, 1)}
        self.dmp = {k: _dev(v) for k, v in _point_map().items()}

    def n(self, seed):
        return len(_point_frame(seed)[0])

    def prepare(self, spec):
        """views and outputs of one call; synchronises, so that the inputs are ready whatever stream the call uses"""
        import torch
        init = np.full((len(spec), self.STRIDE), -1, np.int32)
        for f, (s, n) in enumerate(spec):
            init[f, :n] = _point_frame(s)[2][:n]
        views = [self.Matcher.frame_view(n, self.dev[s][0], self.dev[s][1], self.ds, BOUNDS) for s, n in spec]
        job = (spec, views, _dev(init), torch.zeros(len(spec), dtype=torch.int32, device="cuda"))
        torch.cuda.synchronize()
        return job

    def launch(self, m, job, stream=None):
        _, views, match, nm = job
        m.SearchByProjection(views, self.dmp, 3.0, 0.8, match, self.STRIDE, nm, stream=stream)

    def check(self, job, what):
        spec, _, match, nm = job
        got, cnt = match.cpu().numpy(), nm.cpu().numpy()
        for f, (s, n) in enumerate(spec):
            ref_match, ref_n = _map_ref(s, n)
            assert cnt[f] == ref_n and np.array_equal(got[f, :n], ref_match), "%s, frame %d" % (what, f)

    def run(self, m, spec, what):
        import torch
        job = self.prepare(spec)
        self.launch(m, job)
        torch.cuda.synchronize()
        self.check(job, what)


@functools.lru_cache(maxsize=None)
def _line_frame(seed):
    from rgbd_pl_slam_amd.synth import synth_frame
    a = orc.line_extract(synth_frame(seed), 100)
    init = np.full(len(a["kl"]), -1, np.int32); init[::11] = -2
    return a["kl"], a["desc"], init


@functools.lru_cache(maxsize=None)
def _line_map(M):
    """M map lines around the lines of frames 0 and 1"""
    return matchgen.make_map_lines(np.concatenate([_line_frame(0)[0], _line_frame(1)[0]]), np.concatenate([_line_frame(0)[1], _line_frame(1)[1]]), M, 3)


@functools.lru_cache(maxsize=None)
def _line_ref(seed, n, M):
    kl, desc, init = _line_frame(seed)
    match, cnt = orc.search_lines_by_projection(kl[:n], desc[:n], _scale(), _line_map(M), 3.0, 0.8, init[:n])
    assert cnt > 5
    return match, cnt


class _LineFrames:
    """the same for SearchLinesByProjection: the lines of frames 0 and 1 against M map lines"""
    STRIDE = 128

    def __init__(self, M):
        self.M = M
        self.ds = _dev(_scale())
        self.dev = {s: (_bytes(_line_frame(s)[0]), _dev(_line_frame(s)[1])) for s in (0, 1)}
        self.dml = {k: _dev(v) for k, v in _line_map(M).items()}

    def n(self, seed):
        return len(_line_frame(seed)[0])

    def run(self, m, spec, what):
        import torch
        from rgbd_pl_slam_amd import Matcher
        init = np.full((len(spec), self.STRIDE), -1, np.int32)
        for f, (s, n) in enumerate(spec):
            init[f, :n] = _line_frame(s)[2][:n]
        match = _dev(init); nm = torch.zeros(len(spec), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        m.SearchLinesByProjection([Matcher.lineframe_view(n, self.dev[s][0], self.dev[s][1], self.ds) for s, n in spec], self.dml, 3.0, 0.8, match, self.STRIDE, nm)
        torch.cuda.synchronize()
        got, cnt = match.cpu().numpy(), nm.cpu().numpy()
        for f, (s, n) in enumerate(spec):
            ref_match, ref_n = _line_ref(s, n, self.M)
            assert cnt[f] == ref_n and np.array_equal(got[f, :n], ref_match), "%s, line frame %d" % (what, f)


def test_frame_table_mirror_uploads_exactly_when_the_table_changed():
    """The handle keeps a host copy of the frame table it uploaded last and skips the upload when a call brings the same bytes.  One handle: views A, A
    again (no upload), B that differs from A only in n, then one frame instead of two -- for the point table and for the line table; then Fuse, which
    stages its keyframe as a one-frame table, and A (and A's first frame alone) once more: the keyframe's table must not pass for A's."""
    _need_gpu()
    import torch
    from rgbd_pl_slam_amd import Matcher
    m = Matcher(max_keypoints=512, max_mappoints=512, max_lines=128, max_batch=2)
    P = _PointFrames()
    n0, n1 = P.n(0), P.n(1)
    A = [(0, n0), (1, n1)]
    P.run(m, A, "A")
    P.run(m, A, "A again")
    P.run(m, [(0, n0), (1, n1 - 9)], "B: n differs")
    P.run(m, [(0, n0 - 5)], "one frame")
    P.run(m, A, "A after one frame")
    # the line table
    Q = _LineFrames(300)
    l0, l1 = Q.n(0), Q.n(1)
    LA = [(0, l0), (1, l1)]
    Q.run(m, LA, "A")
    Q.run(m, LA, "A again")
    Q.run(m, [(0, l0), (1, l1 - 7)], "B: n differs")
    Q.run(m, [(1, l1)], "one frame")
    Q.run(m, LA, "A after one frame")
    # Fuse stages its keyframe as frame 0 of the point table
    c = kfgen.keyframe_scene(9, 200, 100, sim3_scale=1.0)
    p = c["pts"]
    dk = _bytes(c["kps"]); dd = _dev(c["desc"]); dsc = _dev(c["scale"]); du = _dev(c["uright"])
    kf = Matcher.frame_view(200, dk, dd, dsc, c["bounds"], du)
    dp = dict(world_pos=_dev(p["xw"]), normal=_dev(p["normal"]), min_dist=_dev(p["min_dist"]), max_dist=_dev(p["max_dist"]), desc=_dev(p["desc"]), valid=_dev(p["valid"]))
    eb, _, en = orc.fuse(c["kps"], c["desc"], c["uright"], c["scale"], c["bounds"], c["pose"], p, 3.0)
    assert en > 10
    for spec, what in ((A, "A after Fuse"), ([(0, n0)], "A's first frame after Fuse")):
        best = torch.full((100,), -7, dtype=torch.int32, device="cuda"); cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        m.Fuse(kf, c["pose"], dp, 3.0, best, cnt)
        torch.cuda.synchronize()
        assert int(cnt[0]) == en and np.array_equal(best.cpu().numpy(), eb), what
        P.run(m, spec, what)
    m.close()


def test_two_streams_on_one_handle():
    """SearchByProjection on one stream, SearchByProjectionLastFrameBatch on another with no host synchronisation in between (they share the cell lists and the
    candidate pool), SearchByProjection on the first stream again with other views: the handle orders them."""
    _need_gpu()
    import torch
    from rgbd_pl_slam_amd import Matcher
    m = Matcher(max_keypoints=512, max_mappoints=512, max_lines=64, max_batch=2)
    P = _PointFrames()
    n0, n1 = P.n(0), P.n(1)
    # the last-frame search: frames 0 and 1 (the latter cut short) against a last frame made from frame 0
    kps0, desc0, _ = _point_frame(0)
    last, pose = matchgen.make_last_frame(kps0, desc0, 5)
    poses = [pose, dict(pose, tcw=(pose["tcw"] * 1.5).astype(np.float32))]
    lspec = [(0, n0), (0, n0 - 20)]
    linit = np.full((2, P.STRIDE), -1, np.int32); lrefs = []
    for f, (s, n) in enumerate(lspec):
        init = np.full(n, -1, np.int32); init[::17] = -2
        linit[f, :n] = init
        lrefs.append(orc.search_by_projection_last(kps0[:n], desc0[:n], None, _scale(), BOUNDS, last, poses[f], 15.0, 0, 1, init))
        assert lrefs[-1][1] > 10
    dl = dict(keys=_bytes(last["keys"]), has_mappoint=_dev(last["has_mappoint"]), outlier=_dev(last["outlier"]), world_pos=_dev(last["world_pos"]),
              mp_desc=_dev(last["mp_desc"]), obs_positive=_dev(last["obs_positive"]))
    du = _dev(np.full(n0, -1, np.float32))
    lviews = [Matcher.frame_view(n, P.dev[0][0], P.dev[0][1], P.ds, BOUNDS, du) for _, n in lspec]
    lmatch = _dev(linit); lnm = torch.zeros(2, dtype=torch.int32, device="cuda")
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    first = P.prepare([(0, n0), (1, n1)]); third = P.prepare([(1, n1 - 11), (0, n0 - 3)])
    torch.cuda.synchronize()
    P.launch(m, first, stream=s1.cuda_stream)
    m.SearchByProjectionLastFrameBatch(lviews, dl, poses, 15.0, 0, 1, lmatch, P.STRIDE, lnm, stream=s2.cuda_stream)
    P.launch(m, third, stream=s1.cuda_stream)
    torch.cuda.synchronize()
    P.check(first, "stream 1, first call")
    P.check(third, "stream 1, second call")
    got = lmatch.cpu().numpy()
    for f, ((rm, rn), (_, n)) in enumerate(zip(lrefs, lspec)):
        assert int(lnm[f]) == rn and np.array_equal(got[f, :n], rm), "stream 2, frame %d" % f
    m.close()


def test_line_search_knobs_are_read_when_the_matcher_is_created(monkeypatch):
    """PLF_MATCH_LINES_STAGE_MAX / PLF_MATCH_LINES_WAVE_MAX belong to the handle: one created with both at 0 (lines read from global memory, a thread per map
    line) and called after they are unset, one created with neither set -- both give the oracle's matches on about 100 lines against 500 map lines."""
    _need_gpu()
    from rgbd_pl_slam_amd import Matcher
    monkeypatch.setenv("PLF_MATCH_LINES_STAGE_MAX", "0")
    monkeypatch.setenv("PLF_MATCH_LINES_WAVE_MAX", "0")
    forced = Matcher(max_keypoints=64, max_mappoints=512, max_lines=128, max_batch=2)
    monkeypatch.delenv("PLF_MATCH_LINES_STAGE_MAX")
    monkeypatch.delenv("PLF_MATCH_LINES_WAVE_MAX")
    default = Matcher(max_keypoints=64, max_mappoints=512, max_lines=128, max_batch=2)
    Q = _LineFrames(500)
    assert Q.n(0) >= 60 and Q.n(1) >= 60
    for m, what in ((forced, "knobs at 0 when created"), (default, "defaults")):
        Q.run(m, [(0, Q.n(0)), (1, Q.n(1) - 6)], what)
        m.close()

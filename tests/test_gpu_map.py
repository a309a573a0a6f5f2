"""MapPoint::ComputeDistinctiveDescriptors / MapLine::ComputeDistinctiveDescriptors on the GPU (plf_map_distinctive_descriptors) against the numpy
restatement tests/mapref.py.  Integer arithmetic throughout: every comparison is bit for bit, no case is excluded."""
import os
import subprocess

import numpy as np
import pytest

import mapref
import orc
from conftest import gpu_available
from cppbuild import build_driver

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
EDGE_COUNTS = [0, 1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025]
LDS_EDGE = [4095, 4096, 4097]     # either side of what the workgroup schedule keeps in LDS (MAP_BLOCK_CAP of csrc/map_common.h)


@pytest.fixture(autouse=True)
def _need_gpu():
    if not gpu_available():
        pytest.fail("no GPU visible: the -m gpu tests need a real MI355X")


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _run(start, desc, valid=None, point_id=None, rows=None, sentinel=0xA5, **kw):
    """packed form on the null stream; returns (map_desc, best_obs, best_median) on the host.  map_desc starts as `sentinel` rows."""
    import torch
    from rgbd_pl_slam_amd import distinctive_descriptors
    n = len(start) - 1
    md = torch.full((n if rows is None else rows, 32), sentinel, dtype=torch.uint8, device="cuda")
    d = _dev(desc) if len(desc) else torch.zeros((1, 32), dtype=torch.uint8, device="cuda")
    bo, bm = distinctive_descriptors(_dev(start), md, obs_desc=d, obs_valid=None if valid is None else (_dev(valid) if len(valid) else torch.zeros(1, dtype=torch.uint8, device="cuda")),
                                     point_id=None if point_id is None else _dev(point_id), **kw)
    torch.cuda.synchronize()
    return md.cpu().numpy(), bo.cpu().numpy(), bm.cpu().numpy()


def _big_case():
    """20,000 points: every edge count several times, one point each of 4095, 4096, 4097 and 5000, the rest long-tailed"""
    rng = np.random.default_rng(11)
    counts = np.minimum(rng.geometric(1 / 7.0, 20000), 200)
    counts[rng.random(20000) < 0.02] = 0
    slots = rng.choice(20000, 3 * len(EDGE_COUNTS) + 4, replace=False)
    counts[slots[:-4]] = np.repeat(EDGE_COUNTS, 3)
    counts[slots[-4:]] = LDS_EDGE + [5000]
    start, desc, valid = mapref.make_points(12, counts, invalid_share=0.1)
    return counts, start, desc, valid


_cache = {}


def _big_ref():
    if "big" not in _cache:
        counts, start, desc, valid = _big_case()
        _cache["big"] = (counts, start, desc, valid, mapref.distinctive_all(start, desc, valid), mapref.distinctive_all(start, desc, None))
    return _cache["big"]


def test_hand_worked_fixture():
    cases = mapref.load_fixture(os.path.join(GOLD, "distinct_tiny.json"))
    start = np.concatenate([[0], np.cumsum([len(c["desc"]) for c in cases])]).astype(np.int32)
    desc = np.concatenate([c["desc"] for c in cases])
    valid = np.concatenate([c["valid_arr"] if c["valid_arr"] is not None else np.ones(len(c["desc"]), np.uint8) for c in cases])
    md, bo, bm = _run(start, desc, valid)
    for i, c in enumerate(cases):
        assert (int(bo[i]), int(bm[i])) == (c["best_obs"], c["best_median"]), c["name"]
        exp = c["desc"][c["best_obs"]] if c["best_obs"] >= 0 else np.full(32, 0xA5, np.uint8)
        assert np.array_equal(md[i], exp), c["name"]


def test_20000_points_every_size_class_and_frequent_ties():
    counts, start, desc, valid, (rbo, rbm), _ = _big_ref()
    # what the case has to contain, asserted on the restatement's own output
    for c in EDGE_COUNTS + LDS_EDGE + [5000]:
        assert (counts == c).sum() >= 1, c
    assert (counts <= 16).sum() > 10000 and ((counts > 16) & (counts <= 256)).sum() > 500 and (counts > 256).sum() >= 10 and (counts > 4096).sum() == 2
    tied = 0
    for p in np.flatnonzero(counts >= 3)[:3000]:
        s, e = start[p], start[p + 1]
        pos = np.flatnonzero(valid[s:e])
        if len(pos) < 2:
            continue
        med = np.sort(mapref.hamming_matrix(desc[s:e][pos]), axis=1)[:, int(0.5 * (len(pos) - 1))]
        tied += (med == med.min()).sum() > 1
    assert tied > 1000                                           # ties on the best median are the common case here
    assert (rbo == -1).sum() >= (counts == 0).sum() > 100
    md, bo, bm = _run(start, desc, valid)
    assert np.array_equal(bo, rbo) and np.array_equal(bm, rbm)
    sentinel = np.full((len(counts), 32), 0xA5, np.uint8)
    assert np.array_equal(md, mapref.apply(sentinel, start, desc, rbo))     # rows without a valid observation stay 0xA5
    # without obs_valid
    _, _, _, _, _, (rbo2, rbm2) = _big_ref()
    md, bo, bm = _run(start, desc, None)
    assert np.array_equal(bo, rbo2) and np.array_equal(bm, rbm2) and np.array_equal(md, mapref.apply(sentinel, start, desc, rbo2))
    assert (rbo2 != rbo).sum() > 500                            # validity changed the choice often enough to matter


def test_one_wave_per_point_schedule_gives_the_same_result(monkeypatch):
    """PLF_MAP_NAIVE=1 (the A/B baseline of tools/bench_distinct.py): one wave per point whatever its count"""
    counts, start, desc, valid, (rbo, rbm), _ = _big_ref()
    monkeypatch.setenv("PLF_MAP_NAIVE", "1")
    md, bo, bm = _run(start, desc, valid)
    assert np.array_equal(bo, rbo) and np.array_equal(bm, rbm)
    assert np.array_equal(md, mapref.apply(np.full((len(counts), 32), 0xA5, np.uint8), start, desc, rbo))


def test_indirect_form_equals_packed_form():
    import torch
    from rgbd_pl_slam_amd import distinctive_descriptors, mappoints
    counts, start, desc, valid, (rbo, rbm), _ = _big_ref()
    rng = np.random.default_rng(5)
    n_kf = 37
    total = len(desc)
    kf = rng.integers(0, n_kf, total).astype(np.int32)
    idx = np.zeros(total, np.int32)
    bufs = []
    for k in range(n_kf):
        o = np.flatnonzero(kf == k)
        order = rng.permutation(len(o))
        buf = np.full((len(o) + 5, 32), 0x5A, np.uint8)            # rows in a shuffled order, spare rows at the end
        buf[order] = desc[o]; idx[o] = order
        bufs.append(_dev(buf))
    table = mappoints.kf_table(bufs)
    md = torch.full((len(counts), 32), 0xA5, dtype=torch.uint8, device="cuda")
    bo, bm = distinctive_descriptors(_dev(start), md, obs_kf=_dev(kf), obs_idx=_dev(idx), kf_desc=table, obs_valid=_dev(valid))
    torch.cuda.synchronize()
    assert np.array_equal(bo.cpu().numpy(), rbo) and np.array_equal(bm.cpu().numpy(), rbm)
    assert np.array_equal(md.cpu().numpy(), mapref.apply(np.full((len(counts), 32), 0xA5, np.uint8), start, desc, rbo))
    # a keyframe index outside the table counts as an invalid observation
    kf2 = kf.copy(); out = rng.random(total) < 0.05; kf2[out] = np.where(rng.random(out.sum()) < 0.5, -1, n_kf)
    md2 = torch.full((len(counts), 32), 0xA5, dtype=torch.uint8, device="cuda")
    bo2, bm2 = distinctive_descriptors(_dev(start), md2, obs_kf=_dev(kf2), obs_idx=_dev(idx), kf_desc=table, obs_valid=_dev(valid))
    torch.cuda.synchronize()
    ebo, ebm = mapref.distinctive_all(start, desc, valid & ~out)
    assert np.array_equal(bo2.cpu().numpy(), ebo) and np.array_equal(bm2.cpu().numpy(), ebm)


def test_point_id_rewrites_exactly_the_named_rows():
    counts, start, desc, valid, (rbo, rbm), _ = _big_ref()
    rng = np.random.default_rng(6)
    rows = 50000
    n = len(counts)
    ids = rng.choice(rows, n, replace=False).astype(np.int32)
    md, bo, bm = _run(start, desc, valid, point_id=ids, rows=rows, sentinel=0x3C)
    assert np.array_equal(bo, rbo) and np.array_equal(bm, rbm)
    exp = mapref.apply(np.full((rows, 32), 0x3C, np.uint8), start, desc, rbo, point_id=ids)
    assert np.array_equal(md, exp) and (exp != 0x3C).any(axis=1).sum() <= (rbo >= 0).sum()
    # ids outside map_desc write nothing
    ids2 = ids.copy(); ids2[::7] = rows + 3; ids2[3::7] = -1
    md, bo, bm = _run(start, desc, valid, point_id=ids2, rows=rows, sentinel=0x3C)
    keep = (ids2 >= 0) & (ids2 < rows)
    exp = np.full((rows, 32), 0x3C, np.uint8)
    for p in np.flatnonzero(keep & (rbo >= 0)):
        exp[ids2[p]] = desc[start[p] + rbo[p]]
    assert np.array_equal(md, exp) and np.array_equal(bo, rbo)


def test_filler_between_and_beyond_the_csr_ranges_is_never_read():
    """rows of the observation arrays that no valid observation names: every real point is followed by a few filler rows (0xFF descriptors), owned by an
    in-between point whose observations are all invalid, and 64 more rows follow the last range (obs_valid = 7 there: never looked at)"""
    import torch
    from rgbd_pl_slam_amd import distinctive_descriptors, mappoints
    rng = np.random.default_rng(8)
    counts = np.concatenate([rng.integers(1, 40, 300), [300, 17, 16, 1]])
    start, desc, valid = mapref.make_points(9, counts, invalid_share=0.2)
    gaps = rng.integers(0, 6, len(counts))
    total = int(counts.sum() + gaps.sum()) + 64
    fd = np.full((total, 32), 0xFF, np.uint8); fv = np.full(total, 7, np.uint8)
    s2 = np.zeros(len(counts) * 2 + 1, np.int32)
    at = 0
    for p, c in enumerate(counts):
        s2[2 * p] = at
        fd[at:at + c] = desc[start[p]:start[p + 1]]; fv[at:at + c] = valid[start[p]:start[p + 1]]
        at += c
        s2[2 * p + 1] = at
        at += gaps[p]
    s2[-1] = at
    # the in-between points: all invalid, so they come out as -1 and their 0xFF rows are never chosen
    for p in range(len(counts)):
        fv[s2[2 * p + 1]:s2[2 * p + 2]] = 0
    md = torch.full((len(s2) - 1, 32), 0xA5, dtype=torch.uint8, device="cuda")
    bo, bm = distinctive_descriptors(_dev(s2), md, obs_desc=_dev(fd), obs_valid=_dev(fv))
    torch.cuda.synchronize()
    bo = bo.cpu().numpy(); bm = bm.cpu().numpy(); mdh = md.cpu().numpy()
    rbo, rbm = mapref.distinctive_all(start, desc, valid)
    assert np.array_equal(bo[0::2], rbo) and np.array_equal(bm[0::2], rbm) and (bo[1::2] == -1).all()
    assert (mdh[1::2] == 0xA5).all()
    # indirect: the invalid filler observations carry wild keyframe indices and row indices -- an invalid observation's descriptor is never fetched
    kfi = np.where(fv == 1, 0, 2 ** 30).astype(np.int32); idx = np.where(fv == 1, np.arange(total), 2 ** 30).astype(np.int32)
    md2 = torch.full((len(s2) - 1, 32), 0xA5, dtype=torch.uint8, device="cuda")
    dfd = _dev(fd); table = mappoints.kf_table([dfd])
    bo2, bm2 = distinctive_descriptors(_dev(s2), md2, obs_kf=_dev(kfi), obs_idx=_dev(idx), kf_desc=table, obs_valid=_dev(fv))
    torch.cuda.synchronize()
    assert np.array_equal(bo2.cpu().numpy(), bo) and np.array_equal(md2.cpu().numpy(), mdh)


def test_a_call_on_a_stream_only_enqueues_and_is_ordered_with_later_work():
    import torch
    from rgbd_pl_slam_amd import distinctive_descriptors
    counts, start, desc, valid, (rbo, rbm), _ = _big_ref()
    ds, dd, dv = _dev(start), _dev(desc), _dev(valid)
    md = torch.full((len(counts), 32), 0xA5, dtype=torch.uint8, device="cuda")
    gate = torch.zeros(1 << 27, dtype=torch.float32, device="cuda")
    s = torch.cuda.Stream()
    distinctive_descriptors(ds, md.clone(), obs_desc=dd, obs_valid=dv, stream=s.cuda_stream)   # untimed: the first call of a process also sets the library up
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        for _ in range(60):
            gate.add_(1.0)                                          # tens of milliseconds of work queued ahead of the call
        done_before = torch.cuda.Event(); done_before.record(s)
        bo, bm = distinctive_descriptors(ds, md, obs_desc=dd, obs_valid=dv, stream=s.cuda_stream)
        returned_while_busy = not done_before.query()               # the call came back while the work ahead of it was still running
        snap = md.clone(); snap_bo = bo.clone()                     # later work on the same stream sees the call's results
    s.synchronize()
    assert returned_while_busy
    exp = mapref.apply(np.full((len(counts), 32), 0xA5, np.uint8), start, desc, rbo)
    assert np.array_equal(snap.cpu().numpy(), exp) and np.array_equal(snap_bo.cpu().numpy(), rbo) and np.array_equal(bm.cpu().numpy(), rbm)


def test_raw_device_addresses_and_argument_checks():
    import torch
    from rgbd_pl_slam_amd import distinctive_descriptors
    start, desc, valid = mapref.make_points(22, [5, 0, 40, 2, 300])
    rbo, rbm = mapref.distinctive_all(start, desc, valid)
    ds, dd, dv = _dev(start), _dev(desc), _dev(valid)
    md = torch.full((5, 32), 0xA5, dtype=torch.uint8, device="cuda")
    bo = torch.empty(5, dtype=torch.int32, device="cuda"); bm = torch.empty(5, dtype=torch.int32, device="cuda")
    distinctive_descriptors(ds.data_ptr(), md.data_ptr(), obs_desc=dd.data_ptr(), obs_valid=dv.data_ptr(), best_obs=bo.data_ptr(), best_median=bm.data_ptr(),
                            n_points=5, map_rows=5)
    torch.cuda.synchronize()
    assert np.array_equal(bo.cpu().numpy(), rbo) and np.array_equal(bm.cpu().numpy(), rbm)
    assert np.array_equal(md.cpu().numpy(), mapref.apply(np.full((5, 32), 0xA5, np.uint8), start, desc, rbo))
    with pytest.raises(ValueError):
        distinctive_descriptors(ds.data_ptr(), md, obs_desc=dd)                                  # an address carries no n_points
    with pytest.raises(ValueError):
        distinctive_descriptors(ds.long(), md, obs_desc=dd)                                      # int64 CSR
    with pytest.raises(ValueError):
        distinctive_descriptors(ds, md, obs_desc=torch.cat([dd, dd], 1)[:, :32])                 # not contiguous
    with pytest.raises(ValueError):
        distinctive_descriptors(ds, md, obs_desc=dd.cpu())                                       # host tensor
    with pytest.raises(ValueError):
        distinctive_descriptors(ds, md, obs_desc=dd, point_id=torch.zeros(3, dtype=torch.int32, device="cuda"))   # shorter than n_points
    with pytest.raises(TypeError):
        distinctive_descriptors(ds, md, obs_desc=dd, obs_valid=valid)                            # numpy


def test_line_side_mirror_names():
    import rgbd_pl_slam_amd as pkg
    start, desc, valid = mapref.make_points(21, [4, 0, 30, 300])
    import torch
    md = torch.full((4, 32), 0xA5, dtype=torch.uint8, device="cuda")
    bo, bm = pkg.MapLine.ComputeDistinctiveDescriptors(_dev(start), md, obs_desc=_dev(desc), obs_valid=_dev(valid))
    bo2, bm2 = pkg.MapPoint.ComputeDistinctiveDescriptors(_dev(start), md.clone(), obs_desc=_dev(desc), obs_valid=_dev(valid))
    torch.cuda.synchronize()
    rbo, rbm = mapref.distinctive_all(start, desc, valid)
    assert np.array_equal(bo.cpu().numpy(), rbo) and np.array_equal(bo2.cpu().numpy(), rbo) and np.array_equal(bm.cpu().numpy(), rbm)
    hdr = open(os.path.join(ROOT, "include", "plf.hpp")).read()
    assert "struct MapLine {" in hdr and "ComputeDistinctiveLineDescriptors" in hdr


def test_cpp_driver(tmp_path):
    exe = build_driver("mappoint_driver", tmp_path, "-O1", "-g", "-Wall")
    rng = np.random.default_rng(31)
    counts = np.concatenate([rng.integers(0, 12, 60), [16, 17, 40, 64]])
    start, desc, _ = mapref.make_points(32, counts)
    kf, idx, valid = mapref.write_driver_input(tmp_path, start, desc, n_kf=64, seed=33)
    run = subprocess.run([str(exe), str(tmp_path)], text=True, capture_output=True)
    assert run.returncode == 0 and "mappoint driver ok" in run.stdout, "driver failed (rc %d)\n%s\n%s" % (run.returncode, run.stdout, run.stderr[-2000:])
    rbo, rbm = mapref.distinctive_all(start, desc, valid)
    get = lambda name, dt: np.fromfile(str(tmp_path / name), dt)
    assert np.array_equal(get("out_best.i32", np.int32), rbo) and np.array_equal(get("out_median.i32", np.int32), rbm)
    assert np.array_equal(get("out_line_best.i32", np.int32), rbo)
    assert np.array_equal(get("out_desc.u8", np.uint8).reshape(-1, 32), mapref.apply(np.zeros((len(counts), 32), np.uint8), start, desc, rbo))
    assert np.array_equal(get("out_member.u8", np.uint8).reshape(-1, 32), mapref.apply(np.full((len(counts), 32), 0xA5, np.uint8), start, desc, rbo))
    assert (rbo == -1).sum() > 3 and (valid == 0).sum() > 10


def test_fuse_then_recompute_then_project_chain():
    """plf_match_fuse on a synthetic keyframe -> the host tail of INTEGRATION.md 1b (Replace / AddObservation) in Python -> the touched points recomputed on the
    device in place (indirect form, point_id = the dirty list) -> plf_match_project_points reads that very map_desc tensor.  Its matches must equal the
    oracle's matcher fed with the restatement's descriptors."""
    import kfgen
    import torch
    from rgbd_pl_slam_amd import Matcher, distinctive_descriptors, mappoints
    from rgbd_pl_slam_amd.matchgen import flip_bits
    nk, m, n_old = 1500, 3000, 12
    c = kfgen.keyframe_scene(41, nk, m)
    p = c["pts"]
    rng = np.random.default_rng(42)
    # the map before the call: every point is seen from 1 .. 6 of n_old older keyframes (index 1 ..); keyframe 0 is the one Fuse projects into.
    # Its observations are its base descriptor (tied to a key point of keyframe 0 by the scene) with a few flipped bits.
    kf_rows = [[] for _ in range(n_old + 1)]
    kf_rows[0] = list(c["desc"])
    obs = []                                                       # per point: {keyframe: row}, iterated in ascending keyframe index (the std::map's order)
    for i in range(m):
        ks = np.sort(rng.choice(np.arange(1, n_old + 1), int(rng.integers(1, 7)), replace=False))
        d = flip_bits(np.repeat(p["desc"][i][None], len(ks), 0), rng, 6)
        o = {}
        for k, row in zip(ks, d):
            o[int(k)] = len(kf_rows[k]); kf_rows[k].append(row)
        obs.append(o)
    kf_np = [np.array(r, np.uint8).reshape(-1, 32) for r in kf_rows]
    kf_bad = np.zeros(n_old + 1, np.uint8); kf_bad[5] = 1          # one old keyframe has gone bad since

    def csr(points):
        start = [0]; kf = []; idx = []
        for i in points:
            for k in sorted(obs[i]):
                kf.append(k); idx.append(obs[i][k])
            start.append(len(kf))
        kf = np.array(kf, np.int32); idx = np.array(idx, np.int32)
        rows = np.array([kf_np[k][j] for k, j in zip(kf, idx)], np.uint8).reshape(-1, 32)
        return np.array(start, np.int32), kf, idx, rows, (1 - kf_bad[kf]).astype(np.uint8)

    bufs = [_dev(a) for a in kf_np]                                # resident keyframe descriptor buffers; keyframe 0's is the one the matchers read
    table = mappoints.kf_table(bufs)
    st, kf, idx, rows, valid = csr(range(m))
    map_desc = torch.full((m, 32), 0xA5, dtype=torch.uint8, device="cuda")
    distinctive_descriptors(_dev(st), map_desc, obs_kf=_dev(kf), obs_idx=_dev(idx), kf_desc=table, obs_valid=_dev(valid))
    torch.cuda.synchronize()
    rbo, _ = mapref.distinctive_all(st, rows, valid)
    ref_desc = mapref.apply(np.full((m, 32), 0xA5, np.uint8), st, rows, rbo)
    assert np.array_equal(map_desc.cpu().numpy(), ref_desc)
    # ---- Fuse (search half) on the device, reading map_desc as it is
    mt = Matcher(max_keypoints=2048, max_mappoints=4096)
    dk = torch.from_numpy(np.frombuffer(np.ascontiguousarray(c["kps"]).tobytes(), np.uint8).copy()).cuda()
    ds = _dev(c["scale"]); du = _dev(c["uright"])
    kfv = Matcher.frame_view(nk, dk, bufs[0], ds, c["bounds"], du)
    alive = (rbo >= 0).astype(np.uint8) & p["valid"]
    dp = dict(world_pos=_dev(p["xw"]), normal=_dev(p["normal"]), min_dist=_dev(p["min_dist"]), max_dist=_dev(p["max_dist"]), desc=map_desc, valid=_dev(alive))
    best = torch.full((m,), -7, dtype=torch.int32, device="cuda"); cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    mt.Fuse(kfv, c["pose"], dp, 3.0, best, cnt); torch.cuda.synchronize()
    pr = dict(p); pr["desc"] = ref_desc; pr["valid"] = alive
    eb, _, en = orc.fuse(c["kps"], c["desc"], c["uright"], c["scale"], c["bounds"], c["pose"], pr, 3.0)
    best = best.cpu().numpy()
    assert int(cnt[0]) == en and en > 100 and np.array_equal(best, eb)
    # ---- the host tail of the reference loop, in list order
    bad = np.zeros(m, bool)
    kp_point = {}                                                  # pKF->GetMapPoint(idx) of keyframe 0
    dirty = set()
    for i in range(m):
        if best[i] < 0 or bad[i] or 0 in obs[i]:
            continue
        j = kp_point.get(int(best[i]))
        if j is not None:
            if not bad[j]:
                keep, drop = (j, i) if len(obs[j]) > len(obs[i]) else (i, j)   # the point with more observations survives
                for k, r in obs[drop].items():                     # MapPoint::Replace: the observations move over where the survivor is not in that keyframe
                    if k not in obs[keep]:
                        obs[keep][k] = r
                        if k == 0:
                            kp_point[r] = keep
                obs[drop] = {}; bad[drop] = True
                dirty.add(keep)
        else:
            obs[i][0] = int(best[i]); kp_point[int(best[i])] = i    # AddObservation + AddMapPoint
            dirty.add(i)
    dirty = np.array(sorted(d for d in dirty if not bad[d]), np.int32)
    assert len(dirty) > 50 and bad.sum() >= 1
    # ---- recompute the touched points on the device, in place
    st, kf, idx, rows, valid = csr(dirty)
    before = map_desc.clone()
    bo, bm = distinctive_descriptors(_dev(st), map_desc, obs_kf=_dev(kf), obs_idx=_dev(idx), kf_desc=table, obs_valid=_dev(valid), point_id=_dev(dirty))
    torch.cuda.synchronize()
    dbo, dbm = mapref.distinctive_all(st, rows, valid)
    assert np.array_equal(bo.cpu().numpy(), dbo) and np.array_equal(bm.cpu().numpy(), dbm)
    ref_desc2 = mapref.apply(ref_desc, st, rows, dbo, point_id=dirty)
    assert np.array_equal(map_desc.cpu().numpy(), ref_desc2)
    changed = (before != map_desc).any(dim=1).cpu().numpy()
    assert changed.sum() > 0 and not changed[np.setdiff1d(np.arange(m), dirty)].any()
    # ---- SearchByProjection(Frame, map points) reads the updated map_desc directly.  The frame: key points near the projections of the points, whose
    # descriptors are noisy copies of the points' NEW descriptors, so the matcher's choices depend on the recomputed rows
    nf = 2000
    sc = c["scale"]
    fk = np.zeros(nf, c["kps"].dtype)
    src = rng.integers(0, m, nf)
    fk["x"] = rng.uniform(20, 620, nf); fk["y"] = rng.uniform(20, 460, nf); fk["octave"] = rng.integers(0, 8, nf); fk["angle"] = rng.uniform(0, 360, nf)
    fk["size"] = 31; fk["response"] = 1; fk["class_id"] = -1
    fdesc = flip_bits(ref_desc2[src], rng, 30)
    mp = dict(proj_x=np.full(m, -100, np.float32), proj_y=np.full(m, -100, np.float32), proj_xr=np.full(m, -1, np.float32), level=np.zeros(m, np.int32),
              view_cos=rng.uniform(0.99, 1.0, m).astype(np.float32), in_view=(~bad & (rng.random(m) < 0.9)).astype(np.uint8),
              obs_positive=np.ones(m, np.uint8))
    mp["proj_x"][src] = (fk["x"] + rng.normal(0, 1.5, nf)).astype(np.float32); mp["proj_y"][src] = (fk["y"] + rng.normal(0, 1.5, nf)).astype(np.float32)
    mp["level"][src] = fk["octave"]
    init = np.full(nf, -1, np.int32)
    fur = np.full(nf, -1, np.float32)
    mpr = dict(mp); mpr["desc"] = ref_desc2
    em, en = orc.search_by_projection_map(fk, fdesc, fur, sc, c["bounds"], mpr, 3.0, 0.8, init)
    dmp = {k: _dev(v) for k, v in mp.items()}; dmp["desc"] = map_desc      # the tensor the recompute wrote
    fkd = torch.from_numpy(np.frombuffer(np.ascontiguousarray(fk).tobytes(), np.uint8).copy()).cuda()
    match = _dev(init); nm = torch.zeros(1, dtype=torch.int32, device="cuda")
    mt.SearchByProjection([Matcher.frame_view(nf, fkd, _dev(fdesc), ds, c["bounds"], _dev(fur))], dmp, 3.0, 0.8, match, nf, nm)
    torch.cuda.synchronize()
    assert int(nm[0]) == en and en > 100 and np.array_equal(match.cpu().numpy(), em)
    mt.close()

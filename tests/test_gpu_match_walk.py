"""GPU parity of the flat candidate walk (flat_walk in match_kernels.hip): k_mp_candidates and k_lf_candidates hand the key points of a wave's cell windows
out one per lane, 64 at a time, and compact the survivors back into per-item spans.  Bit-exact against the plain restatement tests/matchref.py.

One hand-laid scene, built with the generators of tests/crowdgen.py, holds the shapes at which that walk can go wrong (the reference's own `ub` counts, asserted
in _scene(), prove that it does):
  items 0..63     active, inactive and empty-window lanes mixed; item 3 and item 6 look at a crowd of 140 key points in a few cells (a segment that spans
                  three chunks) between lanes that own nothing; level-7 items with th = 3 (the largest radius, the most columns) at the top-left and the
                  bottom-right image corner (windows clipped at all four grid borders)
  items 64..127   a wave whose lanes all have empty windows
  items 128..191  a wave whose windows hold exactly 64 key points
  items 192..255  a wave whose windows hold exactly 65
  item  256       a third block of one lane
About a quarter of the key points are occupied before the call (-2, and indices of items with and without observations) or marked -3, so compacted slots
differ from flat positions.  The item counts 1, 63, 64, 65, 255, 256, 257 cut this list off in the middle of a wave, at its edge and one past it."""
import numpy as np
import pytest

import crowdgen as G
import matchref as R
from conftest import gpu_available
from test_gpu_match_crowded import STRIDE, DevFrame, _dev, _dev_last, _free3, _init_rows

pytestmark = pytest.mark.gpu

F = np.float32
COUNTS = [1, 63, 64, 65, 255, 256, 257]
M_ALL = 257
TH, NN = 3.0, 0.8                     # the scene's windows are laid out for this th
LF_TH = 7.0
EMPTY = (420.0, 390.0)                # no key point within 150 px
CROWD, SMALL8, LONE = (300.0, 200.0), (505.0, 105.0), (560.0, 300.0)
N_SUBSET = 170                        # the second frame of a batch: the first 170 key points (all but 10 of the crowd)


def _group(rng, n, box, first_octave, n_octaves, at):
    """n key points of one crowdgen cluster (it sits in the top-left image corner), moved so that the cluster's box starts at `at`"""
    kps, _ = G.clustered_keypoints(rng, n, n_clusters=1, first_octave=first_octave, n_octaves=n_octaves, box=box)
    kps["x"] = np.clip(kps["x"] + F(at[0]), 0, 639).astype(F); kps["y"] = np.clip(kps["y"] + F(at[1]), 0, 479).astype(F)
    return kps


_SCENE = {}


def _scene():
    """the frame, the 257 map points, and the same items as a last frame (back-projected with the `neither` pose)"""
    if _SCENE:
        return _SCENE
    rng = np.random.default_rng(4711)
    groups = [_group(rng, 60, 40.0, 0, 3, (0, 0)),                       # B  top-left corner
              _group(rng, 60, 40.0, 5, 3, (603, 445)),                   # C  bottom-right corner
              _group(rng, 31, 40.0, 2, 3, (100, 360)),                   # D
              _group(rng, 8, 4.0, 0, 2, (SMALL8[0] - 1, SMALL8[1] - 1)),   # E  eight key points inside 4 px
              _group(rng, 1, 2.0, 1, 1, LONE),                           # F  one key point
              _group(rng, 140, 12.0, 6, 2, (CROWD[0] - 6, CROWD[1] - 6))]  # A  the crowd
    kps = np.concatenate(groups)
    n = len(kps)
    first = np.cumsum([0] + [len(g) for g in groups])
    B, C, D, A = (np.arange(first[k], first[k + 1]) for k in (0, 1, 2, 5))
    base = rng.integers(0, 256, (4, 32), dtype=np.uint8)
    desc, code = G.alphabet_desc(rng, base, n)
    uright = np.where(rng.uniform(0, 1, n) < 0.5, kps["x"] - rng.uniform(2, 30, n), -1).astype(F)
    m = M_ALL
    px = np.full(m, EMPTY[0], F) + rng.uniform(-20, 20, m).astype(F); py = np.full(m, EMPTY[1], F) + rng.uniform(-20, 20, m).astype(F)
    lvl = rng.integers(0, 4, m).astype(np.int32)
    view_cos = np.where(rng.uniform(0, 1, m) < 0.5, 0.9990, 0.95).astype(F)
    in_view = np.ones(m, np.uint8)
    dcode = rng.integers(0, 4, m)

    def aim(items, pool):
        src = rng.choice(pool, len(items))
        px[items] = kps["x"][src] + rng.uniform(-6, 6, len(items)); py[items] = kps["y"][src] + rng.uniform(-6, 6, len(items))
        lvl[items] = np.clip(kps["octave"][src] + rng.integers(0, 2, len(items)), 0, 7)
        dcode[items] = np.where(rng.uniform(0, 1, len(items)) < 0.6, code[src], dcode[items])

    def put(items, at, level, vc=0.95):
        px[items] = at[0]; py[items] = at[1]; lvl[items] = level; view_cos[items] = vc

    aim(np.array([0]), B)
    aim(np.arange(7, 30), np.concatenate([B, D]))
    aim(np.arange(41, 63), np.concatenate([C, D, A]))
    put([3], CROWD, 7); put([6], CROWD, 7, 0.9990)
    put([32, 33], (5.0, 4.0), 7); put([34], (2.0, 30.0), 6)                       # clipped left and top
    put([35, 36], (636.0, 476.0), 7); put([37], (610.0, 478.0), 6, 0.9990)        # clipped right and bottom
    aim(np.array([38, 39, 40]), C)
    put([130, 131, 140, 150, 151, 152, 180, 191], SMALL8, 1)                      # 8 windows x 8 key points
    put([192, 193, 210, 211, 212, 230, 231, 255], SMALL8, 1); put([254], LONE, 2)   # 8 x 8 + 1
    put([256], (634.0, 470.0), 7)
    in_view[[1, 30, 31, 63, 100, 129, 160, 200]] = 0
    mdesc, _ = G.alphabet_desc(rng, base, m, dcode)
    obs = (rng.uniform(0, 1, m) < 0.5).astype(np.uint8)
    proj_xr = (px - rng.uniform(2, 30, m)).astype(F)
    mp = dict(proj_x=px.astype(F), proj_y=py.astype(F), proj_xr=proj_xr, level=lvl, view_cos=view_cos, in_view=in_view, desc=mdesc, obs_positive=obs)
    init = G.match_init(rng, n, np.nonzero(obs)[0], np.nonzero(obs == 0)[0])
    frame = dict(kps=kps, desc=desc, uright=uright, scale=G.scales(), bounds=G.BOUNDS, init=init)
    pose = G.lf_pose("neither")
    lk = np.zeros(m, G.KP_DTYPE); lk["octave"] = lvl; lk["angle"] = rng.uniform(0, 360, m).astype(F)
    last = dict(keys=lk, has_mappoint=in_view.copy(), outlier=(rng.uniform(0, 1, m) < 0.03).astype(np.uint8),
                world_pos=G._back_project(pose, px.astype(np.float64), py.astype(np.float64), np.full(m, 2.0)), mp_desc=mdesc, obs_positive=obs)
    # the scene is what the docstring says: the reference's own window counts
    ub = R.search_by_projection_map(kps, desc, uright, frame["scale"], G.BOUNDS, mp, TH, NN, init)[2]["ub"]
    assert ub[3] >= 130 and ub[6] >= 130 and ub[2] == 0 and ub[4] == 0 and ub[5] == 0 and ub[7] > 0
    assert ub[64:128].sum() == 0 and ub[128:192].sum() == 64 and ub[192:256].sum() == 65 and ub[256] > 0
    assert ub[[32, 33, 34, 35, 36, 37]].min() > 0
    g = R.Grid(kps, G.BOUNDS)
    wins = [g.window(px[i], py[i], F(F(4.0 * TH) * frame["scale"][7])) for i in (32, 35)]
    assert wins[0][0] == 0 and wins[0][2] == 0 and wins[1][1] == R.GRID_COLS - 1 and wins[1][3] == R.GRID_ROWS - 1
    assert max(w[1] - w[0] for w in wins) >= 5 and g.window(CROWD[0], CROWD[1], F(F(4.0 * TH) * frame["scale"][7]))[1] - g.window(CROWD[0], CROWD[1], F(F(4.0 * TH) * frame["scale"][7]))[0] >= 9
    ubl = R.search_by_projection_last(kps, desc, uright, frame["scale"], G.BOUNDS, last, pose, LF_TH, 0, 0, init)[2]["ub"]
    assert ubl[3] >= 130 and ubl[64:128].sum() == 0 and ubl[128:192].sum() == 64 and ubl[192:254].sum() + ubl[255] == 64
    _SCENE.update(frame=frame, mp=mp, last=last)
    return _SCENE


def _cut_mp(mp, m):
    return {k: np.ascontiguousarray(v[:m]) for k, v in mp.items()}


def _cut_last(last, m):
    return {k: np.ascontiguousarray(v[:m]) for k, v in last.items()}


def _fold(frame, m, n=None, uright=True):
    """the frame against the first m items: pre-set indices folded into their range; n: only the first n key points; uright False: a frame without uRight"""
    out = dict(frame)
    if n is not None:
        out.update(kps=frame["kps"][:n], desc=frame["desc"][:n], uright=frame["uright"][:n], init=frame["init"][:n])
    init = out["init"].copy(); init[init >= 0] %= m
    out["init"] = init
    if not uright:
        out["uright"] = None
    return out


def _need_gpu():
    if not gpu_available():
        pytest.fail("no GPU visible: the -m gpu tests need a real MI355X")


_REF = {}


def _ref_map(tag, s, mp, th, nn):
    key = ("map", tag, len(mp["desc"]), th, nn)
    if key not in _REF:
        _REF[key] = R.search_by_projection_map(s["kps"], s["desc"], s["uright"], s["scale"], s["bounds"], mp, th, nn, s["init"])
    return _REF[key]


def _ref_last(tag, s, last, motion, th, mono, ori):
    key = ("last", tag, len(last["mp_desc"]), motion, th, mono, ori)
    if key not in _REF:
        _REF[key] = R.search_by_projection_last(s["kps"], s["desc"], s["uright"], s["scale"], s["bounds"], last, G.lf_pose(motion), th, mono, ori, s["init"])
    return _REF[key]


def _run_map(m, dframes, frames, tags, mp, th, nn, counter_frame=None):
    import torch
    dmp = {k: _dev(v) for k, v in mp.items()}
    match = _dev(_init_rows(frames)); nm = torch.full((len(frames),), -7, dtype=torch.int32, device="cuda")
    m.SearchByProjection([d.view(f == counter_frame) for f, d in enumerate(dframes)], dmp, th, nn, match, STRIDE, nm)
    torch.cuda.synchronize()
    match, nm = match.cpu().numpy(), nm.cpu().numpy()
    for f, s in enumerate(frames):
        ref, rn, _ = _ref_map(tags[f], s, mp, th, nn)
        n = len(s["kps"])
        assert int(nm[f]) == rn, (tags[f], len(mp["desc"]), th, nn)
        assert np.array_equal(match[f, :n], _free3(ref)), (tags[f], len(mp["desc"]), th, nn)
        assert (match[f, n:] == -1).all()


def _run_last(m, dframes, frames, tags, last, motions, th, mono, ori, counter_frame=None):
    import torch
    from rgbd_pl_slam_amd import Matcher
    dlast = _dev_last(last)
    match = _dev(_init_rows(frames)); nm = torch.full((len(frames),), -7, dtype=torch.int32, device="cuda")
    m.SearchByProjectionLastFrameBatch([d.view(f == counter_frame) for f, d in enumerate(dframes)], Matcher.last_view(dlast), [G.lf_pose(mo) for mo in motions],
                                       th, mono, ori, match, STRIDE, nm)
    torch.cuda.synchronize()
    match, nm = match.cpu().numpy(), nm.cpu().numpy()
    for f, s in enumerate(frames):
        ref, rn, _ = _ref_last(tags[f], s, last, motions[f], th, mono, ori)
        n = len(s["kps"])
        assert int(nm[f]) == rn, (tags[f], len(last["mp_desc"]), motions[f], th, mono, ori)
        assert np.array_equal(match[f, :n], _free3(ref)), (tags[f], len(last["mp_desc"]), motions[f], th, mono, ori)
        assert (match[f, n:] == -1).all()


@pytest.mark.parametrize("cand_avg", [None, "1"], ids=["cached_candidates", "pool_of_one_per_item"])
@pytest.mark.parametrize("count", COUNTS)
def test_map_search_item_counts(monkeypatch, count, cand_avg):
    """one frame against the first `count` map points, with and without uRight, th 3 and 1; with a pool of one entry per item the frame overflows while some
    of its waves still fit and write their spans"""
    _need_gpu()
    from rgbd_pl_slam_amd import Matcher
    if cand_avg:
        monkeypatch.setenv("PLF_MATCH_CAND_AVG", cand_avg)
    sc = _scene()
    mp = _cut_mp(sc["mp"], count)
    m = Matcher(max_keypoints=STRIDE, max_mappoints=count if cand_avg else G.CACHED_MAX_MAPPOINTS, max_batch=1)
    for ur in (True, False):
        s = _fold(sc["frame"], count, uright=ur)
        d = DevFrame(s, with_uright=ur)
        for th, nn in ((TH, NN), (1.0, 1.0)):
            _run_map(m, [d], [s], ["full_ur%d" % ur], mp, th, nn)
    m.close()


def _batch_frames(sc, count, items_x, items_y, items_octave, items_desc):
    """three frames with different key point counts: the first N_SUBSET key points (counted on the device), the whole frame, and a sparse frame"""
    sparse = G.sparse_frame(91, 150, items_x, items_y, items_octave, items_desc, n_hit=min(30, count))
    sparse["init"] = sparse["init"].copy()
    return [_fold(sc["frame"], count, n=N_SUBSET), _fold(sc["frame"], count), sparse], ["subset", "full_ur1", "sparse"]


def _small_pool(refs_ub, count):
    """PLF_MATCH_CAND_AVG under which only the middle frame of the batch overflows: pool entries = cand_avg * count"""
    lo = max(int(refs_ub[0].sum()), int(refs_ub[2].sum())); hi = int(refs_ub[1].sum())
    avg = max(1, -(-lo // count))
    assert lo <= avg * count < hi, (lo, avg * count, hi)
    return str(avg)


@pytest.mark.parametrize("small_pool", [False, True], ids=["cached_candidates", "middle_frame_overflows"])
@pytest.mark.parametrize("count", [65, 257])
def test_map_search_batch_of_three_frames(monkeypatch, count, small_pool):
    _need_gpu()
    from rgbd_pl_slam_amd import Matcher
    sc = _scene()
    mp = _cut_mp(sc["mp"], count)
    frames, tags = _batch_frames(sc, count, mp["proj_x"], mp["proj_y"], np.maximum(mp["level"] - 1, 0), mp["desc"])
    if small_pool:
        monkeypatch.setenv("PLF_MATCH_CAND_AVG", _small_pool([_ref_map(t, s, mp, TH, NN)[2]["ub"] for t, s in zip(tags, frames)], count))
    m = Matcher(max_keypoints=STRIDE, max_mappoints=count if small_pool else G.CACHED_MAX_MAPPOINTS, max_batch=3)
    dframes = [DevFrame(s) for s in frames]
    for rep in range(2):      # the second call finds the flags and the pool fill of the first
        _run_map(m, dframes, frames, tags, mp, TH, NN, counter_frame=0)
    m.close()


@pytest.mark.parametrize("cand_avg", [None, "1"], ids=["cached_candidates", "pool_of_one_per_item"])
@pytest.mark.parametrize("count", COUNTS)
def test_lastframe_search_item_counts(monkeypatch, count, cand_avg):
    """the same items as a last frame of `count` points: three poses (the three motion classes: three level windows), with and without uRight"""
    _need_gpu()
    from rgbd_pl_slam_amd import Matcher
    if cand_avg:
        monkeypatch.setenv("PLF_MATCH_CAND_AVG", cand_avg)
    sc = _scene()
    last = _cut_last(sc["last"], count)
    m = Matcher(max_keypoints=STRIDE, max_mappoints=count if cand_avg else G.CACHED_MAX_MAPPOINTS, max_batch=3)
    motions = ["forward", "backward", "neither"]
    for ur in (True, False):
        s = _fold(sc["frame"], count, uright=ur)
        d = DevFrame(s, with_uright=ur)
        _run_last(m, [d, d, d], [s, s, s], ["full_ur%d" % ur] * 3, last, motions, LF_TH, 0, 1)
    s = _fold(sc["frame"], count)
    _run_last(m, [DevFrame(s)], [s], ["full_ur1"], last, ["neither"], 15.0, 1, 0)      # mono: no level window at all when the octave is 0
    m.close()


@pytest.mark.parametrize("small_pool", [False, True], ids=["cached_candidates", "middle_frame_overflows"])
@pytest.mark.parametrize("count", [65, 257])
def test_lastframe_search_batch_of_three_frames(monkeypatch, count, small_pool):
    _need_gpu()
    from rgbd_pl_slam_amd import Matcher
    sc = _scene()
    last = _cut_last(sc["last"], count)
    mp = _cut_mp(sc["mp"], count)
    frames, tags = _batch_frames(sc, count, mp["proj_x"], mp["proj_y"], mp["level"], mp["desc"])
    motions = ["backward", "neither", "forward"]
    if small_pool:
        ubs = [_ref_last(t, s, last, mo, LF_TH, 0, 1)[2]["ub"] for t, s, mo in zip(tags, frames, motions)]
        monkeypatch.setenv("PLF_MATCH_CAND_AVG", _small_pool(ubs, count))
    m = Matcher(max_keypoints=STRIDE, max_mappoints=count if small_pool else G.CACHED_MAX_MAPPOINTS, max_batch=3)
    dframes = [DevFrame(s) for s in frames]
    for rep in range(2):
        _run_last(m, dframes, frames, tags, last, motions, LF_TH, 0, 1, counter_frame=0)
    m.close()

"""KeyFrameCulling and MapPointCulling on the GPU (plf_keyframe_culling, plf_map_point_culling) against the restatement tests/cullref.py: every
comparison is exact equality.  Every call writes into sentinel-filled outputs with a guard behind the last entry, so each comparison also proves
what was NOT written: nothing at n_cand and beyond, kf_erased / point_went_bad only where something was erased or went bad.  Shapes are the
smallest at which a stage can go wrong: wave, workgroup and chunk edges of the row loop, the class edges 8 | 9 and 64 | 65 of the observation walk."""
import numpy as np
import pytest

import cullref
import test_culling_ref as R
from conftest import gpu_available

pytestmark = pytest.mark.gpu
SENT, GUARD, MARK = -777, 64, 7
BIG = 0x7FC00000                                                   # a float NaN's bit pattern, and a huge index
FILL = (BIG, -1, 0x7FFFFFFF, 3, -2 ** 31, BIG)
KEEPALIVE = []


@pytest.fixture(autouse=True)
def _need_gpu():
    if not gpu_available():
        pytest.fail("no GPU visible: the -m gpu tests need a real MI355X")
    yield
    del KEEPALIVE[:]


def _device_map(m, indirect=False, kf_depth=False, before=(), after=(0,)):
    """rgbd_pl_slam_amd.CullMap of the map: packed levels and depths, or the keyframes' own key and depth buffers behind pointer tables"""
    import torch
    from rgbd_pl_slam_amd import CullMap, kf_keys_table
    from rgbd_pl_slam_amd import _lib as L
    from rgbd_pl_slam_amd.mappoints import kf_table
    a = R.flat(m, before, after)
    t = {k: torch.from_numpy(v).cuda() for k, v in a.items()}
    kw = dict(obs_w=t["obs_w"] if m["obs_w"] else None, point_bad=t["point_bad"] if m["point_bad"] else None, th_depth=m["th_depth"], monocular=m["monocular"])
    if m.get("kf_gone"):
        kw["kf_gone"] = torch.tensor(m["kf_gone"], dtype=torch.uint8).cuda()
    n_kf = m["n_kf"]
    if indirect or kf_depth:
        size = [1] * n_kf
        for r, kf in enumerate(m["row_kf"]):
            if 0 <= kf < n_kf:
                size[kf] = max(size[kf], len(m["rows"][r]))
        for p, o in enumerate(m["obs"]):
            for kf, idx in zip(o, m["obs_idx"][p]):
                if 0 <= kf < n_kf:
                    size[kf] = max(size[kf], idx + 1)
    if indirect:
        keys = [np.zeros(s, L.KP_DTYPE) for s in size]
        octave = [np.full(s, -99) for s in size]                    # -99 = not set yet; left so, it would count for every candidate
        def put(kf, idx, lvl):
            assert octave[kf][idx] in (-99, lvl), "the map gives one key two octaves"
            octave[kf][idx] = lvl
        for r, kf in enumerate(m["row_kf"]):
            if 0 <= kf < n_kf:
                for i, lvl in enumerate(m["row_level"][r]):
                    if m["rows"][r][i] >= 0:
                        put(kf, i, lvl)
        for p, o in enumerate(m["obs"]):
            for kf, idx, lvl in zip(o, m["obs_idx"][p], m["obs_level"][p]):
                if 0 <= kf < n_kf:
                    put(kf, idx, lvl)
        for k, o in zip(keys, octave):
            k["octave"] = o; k["x"] = np.nan; k["class_id"] = BIG
        bufs = [torch.from_numpy(np.frombuffer(k.tobytes(), np.uint8).copy()).cuda() for k in keys]
        KEEPALIVE.append(bufs)
        kw.update(kf_keys=kf_keys_table(bufs), obs_idx=t["obs_idx"])
    else:
        kw.update(row_level=t["row_level"], obs_level=t["obs_level"])
    if not m["monocular"]:
        if kf_depth:
            depth = [np.full(s, -5.0, np.float32) for s in size]
            for r, kf in enumerate(m["row_kf"]):
                if 0 <= kf < n_kf:
                    depth[kf][:len(m["rows"][r])] = np.array(m["row_depth"][r], np.float32)
            bufs = [torch.from_numpy(d).cuda() for d in depth]
            KEEPALIVE.append(bufs)
            kw.update(kf_depth=kf_table(bufs))
        else:
            kw.update(row_depth=t["row_depth"])
    return CullMap(t["row_start"], t["row_point"], t["row_kf"], t["obs_start"], t["obs_kf"], n_kf, **kw)


def _outputs(n_cand, n_kf, n_points):
    import torch
    from rgbd_pl_slam_amd.culling import KeyFrameCullingResult
    flat = {k: torch.full((n + GUARD,), SENT, dtype=torch.int32, device="cuda") for k, n in (("n_mps", n_cand), ("n_redundant", n_cand), ("decision", n_cand),
                                                                                           ("point_nobs", n_points), ("status", 2))}
    flat.update({k: torch.full((n + GUARD,), MARK, dtype=torch.uint8, device="cuda") for k, n in (("kf_erased", n_kf), ("point_went_bad", n_points))})
    size = dict(n_mps=n_cand, n_redundant=n_cand, decision=n_cand, point_nobs=n_points, status=2, kf_erased=n_kf, point_went_bad=n_points)
    return KeyFrameCullingResult(**{k: v[:size[k]] for k, v in flat.items()}), flat, size


def _run(m, cand, flags=None, sequential=True, ratio=0.9, th_obs=3, max_culls=0, force=0, resume=False, cmap=None, cand_dev=None, **form):
    import torch
    from rgbd_pl_slam_amd import keyframe_culling
    cmap = cmap or _device_map(m, **form)
    out, flat, size = _outputs(len(cand), m["n_kf"], len(m["obs"]))
    dc = cand_dev if cand_dev is not None else torch.from_numpy(np.array(list(cand) + [0], np.int64).astype(np.int32)).cuda()[:len(cand)]
    df = None if flags is None else torch.from_numpy(np.array(list(flags) + [0], np.uint8)).cuda()
    keyframe_culling(cmap, dc, df, sequential, th_obs, ratio, max_culls, force, resume=resume, out=out)
    torch.cuda.synchronize()
    h = {k: v.cpu().numpy() for k, v in flat.items()}
    for k, v in h.items():
        assert (v[size[k]:] == (MARK if v.dtype == np.uint8 else SENT)).all(), (k, "guard overwritten")
    return {k: v[:size[k]] for k, v in h.items()}, out


def _compare(h, ref, n_cand, decided=None):
    """every element of every output against the restatement; `decided`: only that prefix of the per-candidate outputs is final"""
    d = n_cand if decided is None else decided
    for k in ("n_mps", "n_redundant", "decision"):
        assert h[k][:d].tolist() == ref[k][:d], (k, [(j, int(a), b) for j, (a, b) in enumerate(zip(h[k][:d], ref[k][:d])) if a != b][:8])
    assert h["kf_erased"].tolist() == [1 if e else MARK for e in ref["kf_erased"]], "kf_erased"
    assert h["point_went_bad"].tolist() == [1 if e else MARK for e in ref["point_went_bad"]], "point_went_bad"
    assert h["point_nobs"].tolist() == ref["point_nobs"], "point_nobs"
    assert h["status"].tolist() == [d, ref["erasures"]], ("status", h["status"].tolist(), d, ref["erasures"])


def _check(m, cand, flags=None, sequential=True, ratio=0.9, th_obs=3, **kw):
    h, _ = _run(m, cand, flags, sequential, ratio, th_obs, **kw)
    ref = cullref.keyframe_culling(m, cand, flags, th_obs, ratio, sequential)
    _compare(h, ref, len(cand))
    return h, ref


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]), k


# ---- 1. the hand-worked fixture
@pytest.mark.parametrize("indirect,kf_depth", [(False, False), (True, True), (True, False), (False, True)])
def test_the_hand_worked_fixture_in_both_modes(indirect, kf_depth):
    fx = cullref.load_fixture()
    m, cand, flags = fx["map"], fx["cand_row"], fx["cand_flags"]
    h, _ = _check(m, cand, flags, True, fx["ratio"], fx["th_obs"], indirect=indirect, kf_depth=kf_depth)
    for k in ("n_mps", "n_redundant", "decision", "point_nobs"):
        assert h[k].tolist() == fx["sequential"][k], k
    h, _ = _check(m, cand, flags, False, fx["ratio"], fx["th_obs"], indirect=indirect, kf_depth=kf_depth)
    for k in ("n_mps", "n_redundant", "decision"):
        assert h[k].tolist() == fx["snapshot"][k], k
    assert (h["kf_erased"] == MARK).all() and (h["point_went_bad"] == MARK).all()          # a snapshot erases nothing
    h, _ = _check(dict(m, monocular=1), cand, flags, True, fx["ratio"], fx["th_obs"], indirect=indirect)
    for k in ("n_mps", "n_redundant", "decision", "point_nobs"):
        assert h[k].tolist() == fx["monocular_sequential"][k], k


def _plain_map(rows, obs, row_level=None, obs_level=None, n_kf=None, row_kf=None, obs_w=None):
    n_kf = n_kf or 1 + max([k for o in obs for k in o] + [len(rows)])
    where = {}
    row_kf = row_kf or list(range(len(rows)))
    for r, row in enumerate(rows):
        for i, p in enumerate(row):
            where.setdefault((row_kf[r], p), i)
    return {"n_kf": n_kf, "row_kf": row_kf, "rows": rows, "row_level": row_level or [[0] * len(r) for r in rows], "row_depth": None, "th_depth": 0.0,
            "monocular": 1, "obs": obs, "obs_idx": [[where.get((k, p), 2000 + p) for k in o] for p, o in enumerate(obs)], "obs_w": obs_w,
            "obs_level": obs_level or [[0] * len(o) for o in obs], "point_bad": None}


# ---- 2. row lengths at the loop edges
def test_row_lengths_at_the_wave_workgroup_and_chunk_edges():
    lengths = [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2100]
    n_kf = len(lengths) + 4
    rows, obs = [], []
    for r, n in enumerate(lengths):                                 # every other point is redundant (three more observers), the others are seen by two
        rows.append(list(range(len(obs), len(obs) + n)))
        obs += [sorted([r] + [len(lengths) + k for k in range(3 if j % 2 == 0 else 1)]) for j in range(n)]
    m = _plain_map(rows, obs, n_kf=n_kf)
    h, ref = _check(m, list(range(len(lengths))), None, False, ratio=0.45)
    assert ref["n_mps"] == lengths and ref["n_redundant"] == [(n + 1) // 2 for n in lengths]
    assert ref["decision"] == [0] + [1] * (len(lengths) - 1)        # an empty row: 0 > 0.45 * 0 fails, kept
    _check(m, list(range(len(lengths))), None, True, ratio=0.45, max_culls=len(lengths))


# ---- 3. observation counts at the class edges, the third qualifying observer first, last and absent
EDGE_COUNTS = [0, 1, 2, 3, 4, 7, 8, 9, 10, 63, 64, 65, 66, 127, 128, 129, 200]


def _edge_world():
    """one candidate (slot 0, octave 2 everywhere) and, for every observation count n and placement, a point whose list has n entries: the
    candidate's own observation in the middle, qualifying observers (octave 3 = scaleLevel + 1) at the chosen places, the rest at octave 4"""
    n_kf = 260
    obs, lvl, expect, counts, quals = [], [], [], [], []
    for n in EDGE_COUNTS:
        for place in ("first", "last", "absent", "none_self"):
            kfs = list(range(1, n + 1))                             # ascending slots: std::map order
            level = [4] * n
            if n >= 1 and place != "none_self":
                kfs[n // 2] = 0                                     # the candidate itself: qualifying by octave, never counted
                kfs.sort()
                level[0] = 2
            others = [i for i, k in enumerate(kfs) if k != 0]
            q = {"first": others[:3], "last": others[:2] + others[-1:] if len(others) >= 3 else others, "absent": others[:1] + others[-1:] if len(others) >= 2 else others,
                 "none_self": others[-3:]}[place]
            for i in q:
                level[i] = 3
            obs.append(kfs); lvl.append(level)
            expect.append(len(set(q)) >= 3 and n > 3); counts.append(n); quals.append(q)
    rows = [list(range(len(obs)))]
    m = _plain_map(rows, obs, [[2] * len(obs)], lvl, n_kf=n_kf)
    return m, expect, counts, quals


def test_observation_counts_at_the_class_edges_in_every_class():
    m, expect, counts, quals = _edge_world()
    base, ref = _check(m, [0], None, False)
    assert ref["n_mps"] == [len(expect)] and ref["n_redundant"] == [sum(expect)]
    rows = [[p] for p in range(len(expect))]
    single = dict(m, rows=rows, row_kf=[0] * len(rows), row_level=[[2]] * len(rows))
    h, ref = _check(single, list(range(len(rows))), None, False)      # point by point: a row of one entry each, so that no sum can hide a swap
    assert ref["n_redundant"] == [int(e) for e in expect]
    for force in (1, 2, 3):                                           # every point by lane, by lane group, by wave: the same bits
        _same(base, _run(m, [0], None, False, force=force)[0])
        _same(h, _run(single, list(range(len(rows))), None, False, force=force)[0])
    w2 = dict(single, obs_w=[[2] * len(o) for o in m["obs"]])         # weights of 2: Observations() > 3 from two observations on
    _, ref2 = _check(w2, list(range(len(rows))), None, False, indirect=True)
    assert sum(ref2["n_redundant"]) == sum(ref["n_redundant"]) + 1     # three observers the candidate is not among: Observations() 3 -> 6
    # the walk may stop only when BOTH three observers are counted and Observations() has passed th_obs: thresholds beyond the first step of a
    # class (8 and 64 observations) and just below / at a list's length, where the three observers come first and the sum must run on
    cmap = _device_map(single)
    for th_obs in (0, 4, 8, 9, 62, 64, 65, 126, 128, 199, 200):
        ref = cullref.keyframe_culling(single, list(range(len(rows))), None, th_obs, 0.9, False)
        for force in (0, 1, 2, 3):
            got, _ = _run(single, list(range(len(rows))), None, False, th_obs=th_obs, force=force, cmap=cmap)
            _compare(got, ref, len(rows))
        want = [len(set(q)) >= 3 and n > th_obs for n, q in zip(counts, quals)]
        assert ref["n_redundant"] == [int(x) for x in want], th_obs


# ---- 4. garbage
def test_out_of_range_ids_are_skipped_and_filler_is_never_read():
    m = R.random_map(12, 60, 900, lo=3, hi=9, levels=4)
    cand = list(range(60))
    clean, _ = _check(m, cand, None, True, ratio=0.87)
    dirty = dict(m)
    dirty["rows"] = [r + [-7, len(m["obs"]), BIG, -2 ** 31] for r in m["rows"]]
    dirty["row_level"] = [r + [0, 0, 0, 0] for r in m["row_level"]]
    dirty["row_depth"] = [r + [1.0, 1.0, 1.0, 1.0] for r in m["row_depth"]]
    dirty["obs"] = [o + [60, BIG] for o in m["obs"]]                  # after the real ones: still ascending, as a std::map walk is
    dirty["obs_idx"] = [o + [0, 0] for o in m["obs_idx"]]
    dirty["obs_level"] = [o + [0, 0] for o in m["obs_level"]]
    dirty["obs_w"] = [o + [2, 2] for o in m["obs_w"]]
    for form in (dict(), dict(indirect=True, kf_depth=True)):
        got, _ = _check(dirty, cand, None, True, ratio=0.87, before=FILL, after=FILL * 40, **form)
        _same(clean, got)
    wild = cand[:20] + [-1, 60, BIG, -2 ** 31] + cand[20:]
    flags = [0] * len(wild)
    h, ref = _check(dirty, wild, flags, True, ratio=0.87, before=FILL, after=FILL * 40)
    assert [ref["decision"][j] for j in (20, 21, 22, 23)] == [3, 3, 3, 3]
    bad_row = dict(m, row_kf=[k if k % 7 else -1 - k for k in m["row_kf"]])               # rows whose keyframe is not in the table
    bad_row["row_kf"][5] = 60
    _check(bad_row, cand, None, True, ratio=0.87)


# ---- 5. random maps, sequential
@pytest.mark.parametrize("seed,kw,ratio", [(12, dict(lo=3, hi=9, levels=4), 0.8554), (13, dict(lo=2, hi=8, levels=3), 0.8597),
                                           (14, dict(lo=3, hi=10, levels=4, monocular=True), 0.8822), (12, dict(lo=3, hi=9, levels=4), 0.95)])
def test_random_maps_equal_the_one_by_one_loop(seed, kw, ratio):
    m = R.random_map(seed, 200, 5000, **kw)
    rng = np.random.default_rng(seed)
    cand = [int(x) for x in rng.permutation(200)[:40]]
    flags = [0] * 40
    flags[5] = 1
    erased = [j for j, d in enumerate(cullref.keyframe_culling(m, cand, flags, 3, ratio)["decision"]) if d == 1]
    if len(erased) >= 2:
        flags[erased[1]] = 2                                                               # mbNotErase on a keyframe the loop would erase
    cmap = _device_map(m)
    h, _ = _run(m, cand, flags, True, ratio, cmap=cmap)
    ref = cullref.keyframe_culling(m, cand, flags, 3, ratio)
    assert 0 <= ref["erasures"] <= 6 and (len(erased) < 2 or ref["decision"][erased[1]] == 2)
    _compare(h, ref, len(cand))
    for force in (1, 2, 3):                                                                # every class with erased slots and bad points present
        _same(h, _run(m, cand, flags, True, ratio, force=force, cmap=cmap)[0])
    _same(h, _run(m, cand, flags, True, ratio, indirect=True, kf_depth=True)[0])          # the keyframes' own buffers: the same bits
    stepped, out = _run(m, cand, flags, True, ratio, max_culls=1, resume=True, cmap=cmap)  # one erasure per call, resumed on the applied state
    assert out.calls == max(ref["erasures"], 1)
    _same(h, stepped)
    snap, _ = _run(m, cand, flags, False, ratio, cmap=cmap)
    if ref["erasures"] == 0:                                                               # nothing erased: the snapshot is the whole answer
        for k in ("n_mps", "n_redundant", "decision", "point_nobs"):
            assert np.array_equal(snap[k], h[k]), k
    else:
        first = ref["decision"].index(1)
        assert snap["decision"][:first + 1].tolist() == ref["decision"][:first + 1]       # ... else it is the first round
        assert snap["decision"].tolist() != ref["decision"] or seed == 14


def test_more_erasures_than_max_culls_leaves_a_final_prefix():
    m = R.random_map(13, 200, 5000, lo=2, hi=8, levels=3)
    rng = np.random.default_rng(13)
    cand = [int(x) for x in rng.permutation(200)[:40]]
    ref = cullref.keyframe_culling(m, cand, None, 3, 0.8597)
    assert ref["erasures"] == 5
    erased_at = [j for j, d in enumerate(ref["decision"]) if d == 1]
    for max_culls in (1, 3):
        h, _ = _run(m, cand, None, True, 0.8597, max_culls=max_culls)
        decided = erased_at[max_culls]                                # the keeps up to the next candidate to erase are final, it is not
        assert h["status"].tolist() == [decided, max_culls] and decided < len(cand)
        part = cullref.keyframe_culling(m, cand[:decided], None, 3, 0.8597)
        _compare(h, part, len(cand), decided)
    h, _ = _run(m, cand, None, True, 0.8597, max_culls=5)
    _compare(h, ref, len(cand))
    resumed, out = _run(m, cand, None, True, 0.8597, max_culls=2, resume=True)
    assert out.calls == 3 and resumed["status"].tolist() == [40, 5] and resumed["decision"].tolist() == ref["decision"]
    assert resumed["kf_erased"].tolist() == h["kf_erased"].tolist() and resumed["point_went_bad"].tolist() == h["point_went_bad"].tolist()


# ---- 6. the candidate list straight from the covisibility rows
def test_candidates_come_from_the_covisibility_rows_on_the_device():
    import torch
    from rgbd_pl_slam_amd import update_connections
    m = R.random_map(12, 200, 5000, lo=3, hi=9, levels=4)
    cmap = _device_map(m)
    cov = update_connections(cmap.row_start, cmap.row_point, cmap.row_kf, cmap.obs_start, cmap.obs_kf, 200, 64, 9, cmap.point_bad)
    best, n_best = cov.best_covisibility(48)                          # GetVectorCovisibleKeyFrames of every keyframe
    torch.cuda.synchronize()
    n = n_best.cpu().numpy()
    cur = int(np.nonzero((n > 5) & (n < 48))[0][0])                   # a keyframe whose list is shorter than the row: -1 filler behind it
    cand_dev = best[cur]                                              # the device row as it stands: no host round trip for the list
    cand = cand_dev.cpu().tolist()
    assert cand.count(-1) == 48 - int(n[cur]) > 0 and cur not in cand
    h, _ = _run(m, cand, None, True, 0.86, cmap=cmap, cand_dev=cand_dev)
    ref = cullref.keyframe_culling(m, cand, None, 3, 0.86)
    _compare(h, ref, len(cand))
    assert ref["decision"].count(3) == cand.count(-1)                 # the -1 filler behind the list is decided as skipped


def test_the_ratio_edge_18_and_19_of_20_in_the_double_compare():
    for n_red, want in ((18, cullref.KEEP), (19, cullref.ERASED)):
        for sequential in (False, True):
            h, ref = _check(R.ratio_edge_map(n_red), [0], None, sequential)
            assert (ref["n_mps"], ref["n_redundant"], ref["decision"]) == ([20], [n_red], [want])


# ---- 7. MapPointCulling
def test_map_point_culling_on_every_branch_of_the_table():
    import torch
    from rgbd_pl_slam_amd import map_point_culling
    cols = [list(c) for c in zip(*R.MPC_TABLE)]
    n = len(cols[0])
    dev = lambda a, dt: torch.from_numpy(np.array(a, dt)).cuda()       # noqa: E731
    out = torch.full((n + GUARD,), SENT, dtype=torch.int32, device="cuda")
    got = map_point_culling(dev(cols[0], np.int32), dev(cols[1], np.int32), dev(cols[2], np.int64), 10, 3, point_nobs=dev(cols[3], np.int32),
                            point_bad=dev(cols[4], np.uint8), decision=out[:n])
    torch.cuda.synchronize()
    assert got.cpu().tolist() == cols[5] == cullref.map_point_culling(cols[0], cols[1], cols[2], cols[3], cols[4], 10, 3)
    assert (out[n:] == SENT).all()
    # Observations() from the CSR: weights, an observer outside the table, poisoned filler; 5,000 points across several workgroups
    rng = np.random.default_rng(3)
    n, n_kf = 5000, 50
    obs = [[int(k) for k in rng.integers(-2, n_kf + 2, int(c))] for c in rng.integers(0, 7, n)]
    w = [[int(x) for x in rng.integers(1, 3, len(o))] for o in obs]
    nobs = [sum(wi for k, wi in zip(o, ws) if 0 <= k < n_kf) for o, ws in zip(obs, w)]
    found, visible = rng.integers(0, 9, n), rng.integers(0, 12, n)
    first = rng.integers(95, 102, n)
    bad = rng.integers(0, 10, n) == 0
    start = np.zeros(n + 1, np.int64); start[1:] = np.cumsum([len(o) for o in obs]); start += len(FILL)
    okf = np.array(list(FILL) + [k for o in obs for k in o] + list(FILL), np.int64).astype(np.int32)
    ow = np.array([9] * len(FILL) + [x for ws in w for x in ws] + [9] * len(FILL), np.uint8)
    for cn in (2, 3):
        got = map_point_culling(dev(found, np.int32), dev(visible, np.int32), dev(first, np.int64), 100, cn, obs_start=dev(start, np.int32),
                                obs_kf=dev(okf, np.int32), obs_w=dev(ow, np.uint8), n_kf=n_kf, point_bad=dev(bad, np.uint8))
        torch.cuda.synchronize()
        want = cullref.map_point_culling(found, visible, first, nobs, bad, 100, cn)
        assert got.cpu().tolist() == want and set(want) == {0, 1, 2}


# ---- 8. argument checks, with a device present
def test_bad_arguments_are_rejected_with_a_device_present():
    R.test_symbols_are_exported_and_reject_bad_arguments_without_a_device()

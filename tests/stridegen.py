"""Scenes for tests/test_gpu_second_rows.py: calls with more rows than a row-per-workgroup kernel's grid holds, so that a workgroup (or wave) takes a
second, third and fourth row and meets whatever the earlier one left in its LDS tables, LDS counters and per-workgroup global scratch.

Rows b, b + G, b + 2G, ... go to workgroup b, where G = min(rows, cap); every builder lays its rows out by pass (row // G), so that every workgroup
meets the prescribed sequence of row kinds, and varies the contents with b.  The caps are read from the sources by text (grid_caps()), and every
scene has rows >= 2 * cap + 7; most have 4 * cap + 7, because their sequence has four steps.  numpy and the restatements only: tests/test_second_row_scenes.py
asserts on a machine without a GPU that the scenes are what they claim to be."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rgbd_pl_slam_amd", "csrc")
BIG = 0x7FC00000


def _text(name):
    with open(os.path.join(CSRC, name)) as fh:
        return fh.read()


def _define(name, macro):
    m = re.search(r"^#define\s+%s\s+(\d+)\b" % macro, _text(name), re.M)
    assert m, (name, macro)
    return int(m.group(1))


def _find(name, pattern):
    m = re.search(pattern, _text(name))
    assert m, (name, pattern)
    return m


_caps = {}


def grid_caps():
    """every grid cap and class border the scenes depend on, parsed from the header or host file that sets it"""
    if _caps:
        return _caps
    c = _caps
    c["covis"] = _define("covis_host.hip", "COVIS_MAX_GRID")
    assert re.search(r"std::min\(v->n_rows, COVIS_MAX_GRID\)", _text("covis_host.hip"))
    m = _find("covis_host.hip", r"#define COVIS_SCRATCH_BYTES \(\(size_t\)(\d+) << (\d+)\)")
    c["covis_scratch"] = int(m.group(1)) << int(m.group(2))
    c["covis_sort_cap"] = _define("covis_common.h", "COVIS_SORT_CAP")
    c["covis_dense_default"] = _define("covis_common.h", "COVIS_DENSE_DEFAULT")
    c["cull"] = _define("culling_common.h", "CULL_MAX_GRID")
    assert re.search(r"std::min\(std::max\(n_cand, 1\), CULL_MAX_GRID\)", _text("culling_host.hip"))
    c["cull_chunk"] = _define("culling_common.h", "CULL_CHUNK")
    c["cull_lane_max"] = _define("culling_common.h", "CULL_LANE_MAX")
    c["cull_group_max"] = _define("culling_common.h", "CULL_GROUP_MAX")
    c["local"] = _define("localmap_common.h", "LOCALMAP_MAX_GRID")
    assert re.search(r"grid_lds = \(size_t\)std::min\(v->n_rows, LOCALMAP_MAX_GRID\)", _text("localmap_host.hip"))
    assert re.search(r"k_local_visible, dim3\(\(unsigned\)std::min\(n_rows, LOCALMAP_MAX_GRID\)\)", _text("localmap_host.hip"))
    m = _find("localmap_host.hip", r"k_local_keyframes, dim3\(\(unsigned\)std::min\(v->n_rows, (\d+) \* LOCALMAP_MAX_GRID\)\)")
    c["local_kf"] = int(m.group(1)) * c["local"]
    c["map_blocks"] = int(_find("map_common.h", r"map_grid\(size_t n, size_t per_block, size_t cap = (\d+)\)").group(1))
    c["map_small_max"] = _define("map_common.h", "MAP_SMALL_MAX")
    c["map_wave_max"] = _define("map_common.h", "MAP_WAVE_MAX")
    c["map_block_cap"] = _define("map_common.h", "MAP_BLOCK_CAP")
    c["mapgeom_chunk"] = _define("map_common.h", "MAPGEOM_CHUNK")
    for name, kern in (("map_host.hip", "k_map"), ("mapgeom_host.hip", "k_mapgeom")):
        t = _text(name)
        assert re.search(kern + r"_small, map_grid\(n, 16\), dim3\(256\)", t) and re.search(kern + r"_wave, map_grid\(n, 4\), dim3\(256\)", t), name
    c["map_small"], c["map_wave"] = 16 * c["map_blocks"], 4 * c["map_blocks"]
    m = _find("map_host.hip", r"k_map_block, map_grid\(n, 1, naive \? (\d+) : (\d+)\)")
    c["map_naive_block"], c["map_block"] = int(m.group(1)), int(m.group(2))
    c["mapgeom_block"] = int(_find("mapgeom_host.hip", r"k_mapgeom_block, map_grid\(n, 1, (\d+)\)").group(1))
    m = _find("track_host.hip", r"grid = \(unsigned\)std::min\(v->n_frames, (\d+) << (\d+)\)")
    c["track_close"] = int(m.group(1)) << int(m.group(2))
    m = _find("track_host.hip", r"k_track_need_keyframe, dim3\(\(unsigned\)std::min\(v->n_frames, (\d+) << (\d+)\)\)")
    c["track_kf"] = int(m.group(1)) << int(m.group(2))
    c["track_wave_keys"] = _define("track_common.h", "TRACK_WAVE_KEYS")
    m = _find("tri_host.hip", r"k_tri_points, dim3\(\(unsigned\)std::min\(jobs->n_jobs, (\d+) << (\d+)\)\)")
    c["tri"] = int(m.group(1)) << int(m.group(2))
    return c


def passes(n_rows, G):
    """(pass, workgroup) of every row"""
    r = np.arange(n_rows)
    return r // G, r % G


# ---------------------------------------------------------------------------------------------------------------- covisibility
COVIS_KF = 64              # keyframes of the small covisibility worlds
COVIS_TABLE = 16           # the forced table: it counts as full at 14 entries


def _covis_pool(n_kf):
    """three points seen by keyframe k alone (ids 3k .. 3k + 2) and one seen by k and k + 1 (id 3 n_kf + k)"""
    obs = [[k] for k in range(n_kf) for _ in range(3)] + [[k, (k + 1) % n_kf] for k in range(n_kf)]
    return obs


def _covis_row(kfs, b, n_kf, pairs=True):
    """a row that counts every keyframe of kfs (weights 1 .. 3 by keyframe and workgroup), a null entry and a point listed twice"""
    row = []
    for i, k in enumerate(kfs):
        row += [3 * k + j for j in range(1 + (k + b) % 3)]
        if pairs and i + 1 < len(kfs) and kfs[i + 1] == (k + 1) % n_kf and (k + b) % 4 == 0:
            row.append(3 * n_kf + k)
    if len(row) > 2:
        row.insert(1, -1); row.append(row[0])
    return row


def covis_table_scene():
    """the table path (dense_max_kf = 1, a table of COVIS_TABLE slots), per workgroup: a row that overflows the table (counted in the workgroup's global
    array) -> an empty row -> a row that fits the table, its keyframes disjoint from the first row's -> a row that overflows again, half of its keyframes the first
    row's -> (seven workgroups) one more overflowing row"""
    G = grid_caps()["covis"]
    n_kf, n_rows = COVIS_KF, 4 * G + 7
    obs = _covis_pool(n_kf)
    rows, selfs, kinds = [], [], []
    for r in range(n_rows):
        p, b = divmod(r, G)
        base = b * 5
        if p in (0, 4):
            kfs = [(base + i) % n_kf for i in range(24)]
        elif p == 1:
            kfs = []
        elif p == 2:
            kfs = [(base + 30 + i) % n_kf for i in range(6)]
        else:
            kfs = [(base + 12 + i) % n_kf for i in range(20)]
        row = _covis_row(kfs, b, n_kf, pairs=p != 2)
        if p == 1:
            row = [[], [-1], [-1, len(obs) + 3]][b % 3]                # no entry, a null entry, a point outside the map
        rows.append(row); kinds.append(("over", "empty", "fit", "over2", "over")[p])
        selfs.append(-1 if b % 3 else (kfs[len(kfs) // 2] if kfs else 5))   # the row's own keyframe sits in the middle of what it sees: not counted
    kf_bad = [int(k % 7 == 3) for k in range(n_kf)]
    return dict(rows=rows, selfs=selfs, obs=obs, n_kf=n_kf, stride=16, th=2, kf_bad=kf_bad, dense=1, table=COVIS_TABLE, G=G, kinds=kinds)


def covis_dense_scene():
    """the dense LDS counters, per workgroup: a row that counts every keyframe -> an empty row -> a row of one point -> the full row once more -> empty"""
    G = grid_caps()["covis"]
    n_kf, n_rows = COVIS_KF, 4 * G + 7
    obs = _covis_pool(n_kf)
    rows, selfs, kinds = [], [], []
    for r in range(n_rows):
        p, b = divmod(r, G)
        if p in (0, 3):
            row = _covis_row(list(range(n_kf)), b + p, n_kf)
        elif p == 2:
            row = [3 * n_kf + (b % n_kf)] if b % 2 else [3 * (b % n_kf)]
        else:
            row = [[], [-1]][b % 2]
        rows.append(row); selfs.append(-1); kinds.append(("full", "empty", "one", "full", "empty")[p])
    return dict(rows=rows, selfs=selfs, obs=obs, n_kf=n_kf, stride=n_kf + 3, th=2, kf_bad=[int(k % 7 == 3) for k in range(n_kf)], dense=0, table=0, G=G,
                kinds=kinds)


def covis_long_scene():
    """n_kf just above COVIS_SORT_CAP: workgroups 0 .. 2 take two consecutive rows of more than COVIS_SORT_CAP distinct keyframes, the first one longer, which
    are listed and sorted in the workgroup's global list, then a short row; every other row is short"""
    c = grid_caps()
    G, cap = c["covis"], c["covis_sort_cap"]
    n_kf, n_rows = cap + 2, 2 * G + 7
    # point 0: every keyframe; point 1: all but the last; points 2 .. 5: every third, fifth, seventh, eleventh keyframe (weights of 1 .. 6 in the long rows)
    obs = [list(range(n_kf)), list(range(n_kf - 1))] + [list(range(s, n_kf, s)) for s in (3, 5, 7, 11)]
    first = len(obs)
    obs += [[k, (k * 7 + 1) % n_kf] for k in range(0, n_kf, 13)]
    n_short = len(obs) - first
    rows, kinds = [], []
    for r in range(n_rows):
        p, b = divmod(r, G)
        if b < 3 and p < 2:
            rows.append([p, 2, 3, -1, 4, 5, 2][:7 - b]); kinds.append("long")
        else:
            rows.append([first + (r * 3 + j) % n_short for j in range(1 + r % 3)]); kinds.append("short")
    return dict(rows=rows, selfs=[-1] * n_rows, obs=obs, n_kf=n_kf, stride=n_kf + 2, th=2, kf_bad=None, dense=0, table=0, G=G, kinds=kinds)


def covis_votes_bad_scene():
    """votes, per workgroup: a row with a large maximum -> a row in which every counted keyframe is bad (a result, no local keyframe, max_kf = -1) -> a row"""
    G = grid_caps()["covis"]
    n_kf, n_rows = COVIS_KF, 2 * G + 7
    obs = _covis_pool(n_kf) + [[20 + (j % 3)] for j in range(18)]       # eighteen more points for keyframes 20 .. 22: weights of 6 to 9
    extra = 4 * n_kf
    kf_bad = [int(k < 8) for k in range(n_kf)]
    rows, kinds = [], []
    for r in range(n_rows):
        p, b = divmod(r, G)
        if p == 0:
            rows.append(_covis_row([16 + (b + i) % 40 for i in range(10)], b, n_kf, pairs=False) + list(range(extra, extra + 18))); kinds.append("large")
        elif p == 1:
            rows.append(_covis_row([(b + i) % 8 for i in range(1 + b % 5)], b, n_kf, pairs=False)); kinds.append("all_bad")
        else:
            rows.append(_covis_row([4 + i for i in range(8)], b, n_kf)); kinds.append("mixed")
    return dict(rows=rows, selfs=None, obs=obs, n_kf=n_kf, stride=16, th=1, kf_bad=kf_bad, G=G, kinds=kinds)


# ---------------------------------------------------------------------------------------------------------------- culling
def cull_scene():
    """snapshot mode over a small map, per workgroup: a candidate whose row is longer than CULL_CHUNK -> a skipped candidate (flag bit 0, a row outside the map, a
    row whose keyframe is outside the table) -> a candidate whose row is empty -> a candidate with points of all three observation classes -> (seven workgroups) a
    long row again.  The candidates name a dozen rows; `distinct` lists the (row, flag) pairs that occur and `which` the pair of every candidate, so that the
    restatement runs once per pair and its answer is tiled."""
    c = grid_caps()
    G, chunk, lane_max, group_max = c["cull"], c["cull_chunk"], c["cull_lane_max"], c["cull_group_max"]
    rng = np.random.default_rng(41)
    n_kf = 2 * group_max + 30
    obs, lvl = [], []

    def point(n, must):
        kfs = sorted(set([must] + [int(k) for k in rng.choice(n_kf - 4, n - 1, replace=False)]))    # the last four slots see nothing
        obs.append(kfs); lvl.append([int(x) for x in rng.integers(0, 4, len(kfs))])
        return len(obs) - 1

    rows, row_kf = [], []
    for L, kf in ((chunk + 6, 0), (chunk + chunk // 2, 1), (2 * chunk + 1, 2)):              # long rows: mostly few observations, a few of the larger classes
        row = []
        for i in range(L):
            n = (3, 4, 5, 2, 6)[i % 5] if i % 97 else (lane_max + 3 if i % 2 else group_max + 9)
            row.append(point(n, kf) if i % 11 else (row[-1] if row else -1))                   # a point listed twice, a null entry at the front
        rows.append(row); row_kf.append(kf)
    rows.append([]); row_kf.append(3)                                                           # row 3: empty
    for kf in (4, 5, 6):                                                                        # rows 4 .. 6: all three classes, the class borders among them
        counts = [3, lane_max, lane_max + 1, group_max, group_max + 1, 2 * group_max, 4, 7] * 3
        rng.shuffle(counts)
        rows.append([point(n, kf) for n in counts] + [-1]); row_kf.append(kf)
    rows.append([rows[4][0], rows[5][1]]); row_kf.append(n_kf)                                  # row 7: its keyframe is outside the table
    rows.append([rows[6][2]]); row_kf.append(-1)                                                # row 8: likewise
    n_rows = len(rows)
    where = {}
    for r, row in enumerate(rows):
        for i, p in enumerate(row):
            where.setdefault((row_kf[r], p), i)
    m = {"n_kf": n_kf, "row_kf": row_kf, "rows": rows, "row_level": [[int(x) for x in rng.integers(0, 4, len(r))] for r in rows], "row_depth": None,
         "th_depth": 0.0, "monocular": 1, "obs": obs, "obs_idx": [[where.get((k, p), 2000 + p) for k in o] for p, o in enumerate(obs)], "obs_w": None,
         "obs_level": lvl, "point_bad": [int(x) for x in rng.integers(0, 15, len(obs)) == 0]}
    distinct = [(0, 0), (1, 0), (2, 2),                                                         # long rows (flag bit 1 only matters to an erasure)
                (0, 1), (4, 3), (-1, 0), (n_rows, 0), (BIG, 0), (7, 0), (8, 0),                 # skipped in every way
                (3, 0), (3, 2),                                                                 # the empty row
                (4, 0), (5, 0), (6, 2)]                                                         # mixed
    by_pass = ([0, 1, 2], [3, 4, 5, 6, 7, 8, 9], [10, 11], [12, 13, 14], [2, 0, 1])
    n_cand = 4 * G + 7
    which = np.zeros(n_cand, np.int64)
    for j in range(n_cand):
        p, b = divmod(j, G)
        which[j] = by_pass[p][b % len(by_pass[p])]
    return dict(map=m, distinct=distinct, which=which, G=G, n_cand=n_cand, ratio=0.3, th_obs=3,
                kinds=[("long", "skipped", "empty", "mixed", "long")[j // G] for j in range(n_cand)])


def cull_reference(s):
    """the restatement once per distinct (row, flag) pair, tiled over the candidates; a snapshot erases nothing"""
    import cullref
    m = s["map"]
    one = cullref.keyframe_culling(m, [r for r, _ in s["distinct"]], [f for _, f in s["distinct"]], s["th_obs"], s["ratio"], False)
    ref = {k: np.array(one[k])[s["which"]].tolist() for k in ("n_mps", "n_redundant", "decision")}
    ref.update({k: one[k] for k in ("kf_erased", "point_went_bad", "point_nobs", "erasures")})
    return ref, one


# ---------------------------------------------------------------------------------------------------------------- local map
ITEMS_TABLE = 64           # the forced table of the item pass: rows of up to 32 positions stay in LDS
ITEMS_N = 300
ITEMS_STRIDE = 40


def local_items_scene():
    """both launches of the item pass in one call, per workgroup: a short row (LDS table) -> a long row (the workgroup's global table; bad ids in it, and for every
    other workgroup more items than item_stride: status 4) -> a short row -> a long row that shares half of its ids with the first long row and has ids that one
    did not touch -> (seven workgroups) a short row.  The frame's own row names ids inside and outside the row, bad ones and junk."""
    G = grid_caps()["local"]
    rng = np.random.default_rng(43)
    n_items = ITEMS_N
    item_bad = [int(x) for x in rng.integers(0, 8, n_items) == 0]
    bad_ids = [i for i in range(n_items) if item_bad[i]]
    kf_rows = []
    for i in range(16):                                                  # keyframe rows 0 .. 15: short
        kf_rows.append([int(x) for x in rng.integers(-1, n_items, 5 + i % 8)])
    long_a, long_b = [], []
    for j in range(8):
        lo = 30 * j
        if j % 2 == 0:                                                   # 16 .. 23: 60 positions, at least 45 distinct good ids: beyond item_stride
            a = list(range(lo, lo + 56)) + bad_ids[j:j + 4]
        else:                                                            # 35 distinct ids and repeats of them
            a = list(range(lo, lo + 35)) + list(range(lo, lo + 21)) + bad_ids[j:j + 4]
        rng.shuffle(a)
        long_a.append(a)
        bb = a[:28] + list(range(lo + 60, lo + 82)) + [-1, n_items]      # 24 .. 31: half of the first one's ids, and 22 it did not touch
        rng.shuffle(bb)
        long_b.append(bb)
    kf_rows += long_a + long_b
    n_rows = 4 * G + 7
    local, frame_rows, kinds = [], [], []
    for r in range(n_rows):
        p, b = divmod(r, G)
        if p in (0, 2, 4):
            lk = [(b + p) % 16, (b * 3 + 1 + p) % 16] if b % 4 else [(b + p) % 16]
            kinds.append("short")
        elif p == 1:
            lk = [16 + b % 8] + ([b % 16] if b % 3 == 0 else [])
            kinds.append("long_a")
        else:
            lk = [24 + b % 8]
            kinds.append("long_b")
        local.append(lk)
        ids = [x for k in lk for x in kf_rows[k]]
        frame_rows.append(ids[b % 3::4] + [(b * 7) % n_items, bad_ids[b % len(bad_ids)], -9, BIG])
    return dict(local=local, kf_rows=kf_rows, n_items=n_items, item_stride=ITEMS_STRIDE, item_bad=item_bad, frame_rows=frame_rows, table=ITEMS_TABLE, G=G,
                kinds=kinds)


def local_kf_scene():
    """the keyframe expansion, per wave: a row with seeds that expands -> a row with n_seed = 0 -> a row whose seeds are the keyframes the first row pushed (marks
    left over from it would suppress them, and change what they push in turn) -> (seven waves) an empty row"""
    import localmapref as R
    G = grid_caps()["local_kf"]
    n_kf = 400
    rng = np.random.default_rng(47)
    parent = [-1] + [int(rng.integers(0, k)) if rng.random() < 0.3 else -1 for k in range(1, n_kf)]
    children = [[] for _ in range(n_kf)]
    for k, p in enumerate(parent):
        if p >= 0:
            children[p].append(k)
    covis = [[int(x) for x in rng.choice(n_kf, int(rng.integers(0, 15)), replace=False) if x != k] for k in range(n_kf)]
    kf_bad = [int(x) for x in rng.integers(0, 10, n_kf) == 0]
    good = [k for k in range(n_kf) if not kf_bad[k]]
    period = 211
    first = [sorted(int(x) for x in rng.choice(good, int(rng.integers(1, 12)), replace=False)) for _ in range(period)]
    pushed = []
    for s in first:
        full = R.local_keyframes(s, covis, children, parent, kf_bad, 10, 80)
        pushed.append(full[len(s):])
    n_rows = 3 * G + 7
    seeds, kinds = [], []
    for r in range(n_rows):
        p, b = divmod(r, G)
        if p == 0:
            seeds.append(first[b % period]); kinds.append("expands")
        elif p == 2:
            seeds.append(pushed[b % period]); kinds.append("pushed")
        else:
            seeds.append([]); kinds.append("empty")
    return dict(seeds=seeds, covis=covis, children=children, parent=parent, kf_bad=kf_bad, kf_stride=16, G=G, kinds=kinds, first=first, pushed=pushed,
                period=period)


def local_visible_scene():
    """the head of SearchLocalPoints, per workgroup: full rows and rows with n_local_item = 0 in turn (the even workgroups begin with a full one); every frame's
    own row and every kept item raise the map's one `visible` array"""
    G = grid_caps()["local"]
    rng = np.random.default_rng(53)
    n_items, stride, n_rows = 200, 24, 2 * G + 7
    item_bad = (rng.integers(0, 8, n_items) == 0).astype(np.uint8)
    good = np.flatnonzero(item_bad == 0)
    period = 37
    items = np.stack([rng.choice(good, stride, replace=False) for _ in range(period)]).astype(np.int32)
    local_item = np.zeros((n_rows, stride), np.int32)
    n_local = np.zeros(n_rows, np.int32)
    frame_rows = []
    for r in range(n_rows):
        p, b = divmod(r, G)
        local_item[r] = items[(r * 5) % period]
        full = (p + b) % 2 == 0
        n_local[r] = (stride if b % 5 else stride - 3) if full else 0
        frame_rows.append([int(x) for x in local_item[r, b % 4::6]] + [int(rng.integers(0, n_items)), int(np.flatnonzero(item_bad)[b % 7]), -1, n_items])
    frustum = rng.integers(0, 2, (n_rows, stride)).astype(np.uint8)
    frustum[n_local == 0] = 1                                          # what a recycled buffer may hold behind an empty list
    seen = np.zeros((n_rows, stride), np.uint8)
    for r in range(n_rows):
        own = {x for x in frame_rows[r] if 0 <= x < n_items and not item_bad[x]}
        seen[r] = [int(x in own) for x in local_item[r]]
    start = rng.integers(0, 50, n_items).astype(np.int32)
    return dict(local_item=local_item, n_local=n_local, seen=seen, frustum=frustum, frame_rows=frame_rows, item_bad=item_bad, n_items=n_items, stride=stride,
                start=start, G=G)


def local_visible_reference(s):
    """-> (in_view (rows, stride), n_to_match, visible)"""
    import localmapref as R
    visible = s["start"].tolist()
    bad = s["item_bad"].tolist()
    n_rows, stride = s["local_item"].shape
    in_view = np.zeros((n_rows, stride), np.uint8)
    n_to = np.zeros(n_rows, np.int32)
    for r in range(n_rows):
        n = int(s["n_local"][r])
        iv, n_to[r] = R.search_local_head(s["local_item"][r, :n].tolist(), s["frustum"][r], s["n_items"], bad, s["frame_rows"][r], visible)
        in_view[r, :n] = iv
    return in_view, n_to, np.array(visible, np.int32)


# ---------------------------------------------------------------------------------------------------------------- distinctive descriptors
def _tile_csr(counts_d, idx):
    """the CSR of points idx[i] of a CSR with counts counts_d: (start, src) -- observation o of the tiled CSR is observation src[o] of the distinct one"""
    counts_d = np.asarray(counts_d, np.int64)
    start_d = np.concatenate([[0], np.cumsum(counts_d)])
    counts = counts_d[idx]
    start = np.concatenate([[0], np.cumsum(counts)])
    owner = np.repeat(np.arange(len(idx)), counts)
    src = start_d[idx][owner] + (np.arange(int(start[-1])) - start[:-1][owner])
    return start.astype(np.int32), src


def map_scene(cls):
    """one call whose points all fall into one size class, more than twice as many as its kernel's grid takes per pass, drawn from an odd period of distinct points
    (coprime to the grid, so a wave's next point is another distinct point): the restatement runs once per distinct point, `idx` tiles its answer.
      small  most points 1 .. 3 observations, a few 15 and 16; after a point of 16 comes one whose every observation is left out (none takes part)
      wave   most points 17 .. 21, a few 256; a point of 17 after one of 256
      block  most points 257 .. 259, one of MAP_BLOCK_CAP (descriptors in LDS) and one beyond it (global memory); 257 after both
    The order inside a class list is that of the binning pass's atomics, wave by wave: about the point order, not exactly."""
    import mapref
    c = grid_caps()
    small_max, wave_max, block_cap = c["map_small_max"], c["map_wave_max"], c["map_block_cap"]
    if cls == "small":
        G, P = c["map_small"], 255
        shift = G % P
        counts = np.array([1 + i % 3 for i in range(P)])
        big = [i for i in range(0, P, 8) if i < P - shift][:12]
        counts[big] = small_max
        counts[[i + 3 for i in big]] = small_max - 1
        none = [(i + shift) % P for i in big]                      # what the same lanes meet next: no valid observation
        counts[none] = 1
    elif cls == "wave":
        G, P = c["map_wave"], 255
        shift = G % P
        counts = np.array([small_max + 1 + i % 5 for i in range(P)])
        big = [i for i in range(P) if i % 64 in (0, 16)]
        assert not {(i + shift) % P for i in big} & set(big)
        counts[big] = wave_max
        none = [(big[0] + 2 * shift) % P]
    else:
        G, P = c["map_block"], 33
        shift = G % P
        counts = np.array([wave_max + 1 + i % 3 for i in range(P)])
        big = [1, 10]                                              # both followed, a pass later, by a point of 257
        counts[1], counts[10] = block_cap, block_cap + 1
        none = [(10 + 2 * shift) % P]
    n = 2 * G + 7
    start_d, desc_d, valid_d = mapref.make_points(61 + P + G % 97, counts, invalid_share=0.1)
    for i in none:
        valid_d[start_d[i]:start_d[i + 1]] = 0
    idx = np.arange(n) % P
    start, src = _tile_csr(counts, idx)
    return dict(cls=cls, G=G, P=P, shift=shift, n=n, counts_d=counts, start_d=start_d, desc_d=desc_d, valid_d=valid_d, idx=idx, start=start, desc=desc_d[src],
                valid=valid_d[src], big=big, none=none)


def map_reference(s, sentinel=0xA5):
    """(map_desc, best_obs, best_median) for the tiled points"""
    import mapref
    bo_d, bm_d = mapref.distinctive_all(s["start_d"], s["desc_d"], s["valid_d"])
    bo, bm = bo_d[s["idx"]], bm_d[s["idx"]]
    md = np.full((s["n"], 32), sentinel, np.uint8)
    have = bo >= 0
    md[have] = s["desc"][s["start"][:-1][have].astype(np.int64) + bo[have]]
    return md, bo, bm, (bo_d, bm_d)


# ---------------------------------------------------------------------------------------------------------------- normal and depth
def normal_scene():
    """one mixed call: more than twice the wave grid of wave-class points (most 17 .. 21 observations, a few 256; 17 after 256), then more than twice the
    workgroup grid of workgroup-class points (most 257 .. 259, a few longer than MAPGEOM_CHUNK and than two chunks; 257 after each), then a few points of the
    small class, without observations and with a reference keyframe outside the table"""
    import normref
    c = grid_caps()
    Gw, Gb, chunk, small_max, wave_max = c["map_wave"], c["mapgeom_block"], c["mapgeom_chunk"], c["map_small_max"], c["map_wave_max"]
    Pw, Pb = 255, 33
    cw = np.array([small_max + 1 + i % 5 for i in range(Pw)])
    big_w = [i for i in range(Pw) if i % 64 in (0, 16)]
    assert not {(i + Gw % Pw) % Pw for i in big_w} & set(big_w)
    cw[big_w] = wave_max
    cb = np.array([wave_max + 1 + i % 3 for i in range(Pb)])
    big_b = [0, 10, 20]
    cb[0], cb[10], cb[20] = chunk + 1, 2 * chunk + 1, chunk
    assert not {(i + Gb % Pb) % Pb for i in big_b} & set(big_b)
    nw, nb = 2 * Gw + 7, 2 * Gb + 7
    tail = [0, 1, small_max, 2, 0, 5]
    counts = np.concatenate([cw[np.arange(nw) % Pw], cb[np.arange(nb) % Pb], tail])
    m = normref.make_map(71, counts, 6000)
    m["ref_kf"][-1] = 6000                                          # outside the table: left alone
    return dict(m=m, counts=counts, nw=nw, nb=nb, Gw=Gw, Gb=Gb, Pw=Pw, Pb=Pb, big_w=big_w, big_b=big_b, scale=normref.scale_factors())


# ---------------------------------------------------------------------------------------------------------------- tracking tail, triangulation
TRACK_STRIDE = 6           # key points per frame: the keys are padded to 8
TRACK_PERIOD = 35          # distinct frames; odd, so coprime to the grid of 2^20


def track_close_scene():
    """more frames than k_track_close_wave's grid, from TRACK_PERIOD distinct frames of up to TRACK_STRIDE key points.  Frame f and frame f + grid differ in their
    entry count (so, mostly, in the power of two their keys are padded to); a frame without a key point follows every full one"""
    import trackgen as T
    G = grid_caps()["track_close"]
    P, S = TRACK_PERIOD, TRACK_STRIDE
    shift = G % P
    th = float(T.TH_DEPTH)
    frames, entries = [], []
    rng = np.random.default_rng(83)
    mult = next(c for c in range(1, S + 1) if (shift * c) % (S + 1) == 1)
    n_of = [(i * mult) % (S + 1) for i in range(P)]                 # a pass later the same wave meets a frame of one key point more; after the full one, none
    for i in range(P):
        n = n_of[i]
        z = (rng.uniform(0.3, 1.0, n) * th * rng.choice([1.0, 1.0, 2.5], n)).astype(np.float32)
        if n == 2 and i % 5 == 0:
            z = -np.abs(z); z[0] = 0.0                               # key points, but no entry
        elif n == S - 1:
            z[1], z[3] = np.nan, [-1.0, 0.0][i % 2]                  # two non-entries among them
        elif n > 2 and i % 2:
            z[2] = z[0]                                              # two equal depths
        frames.append(T.make_frame(900 + i, n, z, n_points=40, match_frac=0.4, stride=S))
        entries.append(int((z > 0).sum()))
    p = T.pack(frames)
    n_frames = G + 64
    idx = np.arange(n_frames) % P
    return dict(period=p, idx=idx, G=G, P=P, shift=shift, entries=np.array(entries), n_frames=n_frames, kw=dict(min_points=3, new_stride=4))


def tile_batch(p, idx):
    """the packed batch of frames idx[i] of a packed batch"""
    return dict(keys=p["keys"][idx], depth=p["depth"][idx], match=p["match"][idx], n=p["n"][idx], n_obs=p["n_obs"], frustum=p["frustum"][idx],
                row_id=p["row_id"][idx] if p["row_id"] is not None else None, stride=p["stride"])


def track_need_scene():
    """more frames than k_track_need_keyframe's grid: TRACK_PERIOD distinct frames of 8 key points over three reference rows, with per-frame n, states and
    inlier counts; a frame whose reference keyframe is outside the table (nRef 0) follows frames with long rows"""
    import trackgen as T
    import trackref as R
    G = grid_caps()["track_kf"]
    P, S = TRACK_PERIOD, 8
    rng = np.random.default_rng(89)
    fr = [T.make_frame(950 + k, k % (S + 1), stride=S, n_points=60, row_id=True, match_frac=0.7) for k in range(P)]
    p = T.pack(fr)
    n_obs = rng.integers(0, 5, 60).astype(np.int32)
    bad = (rng.random(60) < 0.2).astype(np.uint8)
    rows = [np.concatenate([rng.integers(0, 60, L), [-1, 60, 1000, -7]]) for L in (70, 3, 0, 130)]
    start = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    item = np.concatenate(rows).astype(np.int32)
    states = [T.state(ref_kf=(k % 6) - 1, n_kfs=(2, 3, 1, 7)[k % 4], n_matches_inliers=10 + 9 * k, flags=(R.MAPPER_IDLE, 0)[k % 2], frame_id=100 + k % 40) for k in range(P)]
    t = dict(depth=p["depth"], match=p["match"], n=p["n"], row_id=p["row_id"], n_obs=n_obs, item_bad=bad, kf_row_start=start, kf_row_item=item,
             state=T.state_records(states), th_depth=float(T.TH_DEPTH), n_inliers=(5 + 11 * np.arange(P)).astype(np.int32))
    n_frames = G + 64
    return dict(period=t, idx=np.arange(n_frames) % P, G=G, P=P, n_frames=n_frames)


TRI_KEYS = 12


def tri_scene():
    """more jobs than k_tri_points' grid.  Four keyframe slots: 0, 1 a pair with a sideways baseline, 2, 3 a pair whose baseline is below mb.  TRACK_PERIOD distinct
    jobs: by residue mod 7 a job names (0, 1) with a match row of its own (pairs dropped, so the counts differ), a slot outside the set (residue 3) or the short
    baseline (residue 5); the grid shifts the residue by 4, so a bad-slot job follows the full job of residue 6 and a skipped one that of residue 1.  new_stride
    is below what the full jobs create."""
    import trigen as T
    G = grid_caps()["tri"]
    P, n = TRACK_PERIOD, TRI_KEYS
    assert (G % P) % 7 == 4
    a, b, m = T.pair_scene(97, n, n, n, (-0.25, 0.02, 0.03), mismatch=0.15, noisy=0.15)
    c, d, m2 = T.pair_scene(98, n, n, n, (0.005, 0.0, 0.008))
    k1, k2 = np.zeros(P, np.int32), np.ones(P, np.int32)
    m12 = np.full((P, n), -1, np.int32)
    for i in range(P):
        row = m.copy()
        drop = (0, 2, 6, 0, 10, 0, 0)[i % 7] + (i // 7) % 2          # residues 0 and 6: (nearly) every pair
        row[(np.arange(n) * 7 + i) % n < drop] = -1
        if i % 7 == 2:
            row[i % n] = n + 3                                       # i2 beyond keyframe 2
        m12[i] = row
        if i % 7 == 3:
            k1[i], k2[i] = [(-1, 1), (0, 4), (4, 0), (2 ** 31 - 1, -2 ** 31), (1, 9)][(i // 7) % 5]
        elif i % 7 == 5:
            k1[i], k2[i], m12[i] = 2, 3, m2
    period = dict(slots=[a, b, c, d], job_kf1=k1, job_kf2=k2, match12=m12)
    n_jobs = G + 64
    idx = np.arange(n_jobs) % P
    return dict(period=period, idx=idx, G=G, P=P, n_jobs=n_jobs, new_stride=3)


def tile_jobs(sc, idx):
    return dict(slots=sc["slots"], job_kf1=np.ascontiguousarray(sc["job_kf1"][idx]), job_kf2=np.ascontiguousarray(sc["job_kf2"][idx]),
                match12=np.ascontiguousarray(sc["match12"][idx]))


def tile_result(r, idx, keys):
    return {k: (np.ascontiguousarray(v[idx]) if k in keys else v) for k, v in r.items()}

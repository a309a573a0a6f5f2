"""The covisibility graph on the GPU (plf_covis_count, plf_covis_by_weight) against the restatement tests/covisref.py, element for element.
Every call writes into sentinel-filled outputs with a guard behind the last row, so each comparison also proves what was NOT written: nothing
at `stride` and beyond, -1 in *_kf exactly from the count to `stride`, nothing at all in a row whose count is empty.  Shapes are the smallest
at which a stage can go wrong: wave and workgroup edges of the row and observation loops, the 256-entry chunks of the emit stage, the LDS list
of 4096 entries, the three counting paths."""
import numpy as np
import pytest

import covisref
from conftest import gpu_available
from test_covis_ref import load_fixture

pytestmark = pytest.mark.gpu
SENT, GUARD = -777, 64
CONN, VOTES = 0, 1


@pytest.fixture(autouse=True)
def _need_gpu():
    if not gpu_available():
        pytest.fail("no GPU visible: the -m gpu tests need a real MI355X")


def _csr(lists, before=(), after=(0,)):
    """CSR on the device with filler before the first and after the last range (never empty: a valid address)"""
    import torch
    start = np.zeros(len(lists) + 1, np.int64)
    start[1:] = np.cumsum([len(x) for x in lists])
    start += len(before)
    flat = np.array(list(before) + [x for lst in lists for x in lst] + list(after), np.int64).astype(np.int32)
    return torch.from_numpy(start.astype(np.int32)).cuda(), torch.from_numpy(flat).cuda()


def _u8(x):
    import torch
    return None if x is None else torch.from_numpy(np.array(x, np.uint8)).cuda()


class _Out:
    """sentinel-filled outputs with a guard behind the last row, shaped like rgbd_pl_slam_amd.Covisibility"""

    def __init__(self, n_rows, stride, votes):
        import torch
        from rgbd_pl_slam_amd import Covisibility
        self.c = Covisibility(n_rows, stride, torch.device("cuda", 0), votes, None)
        self.flat = {}
        for name in ("conn_kf", "conn_w", "ord_kf", "ord_w"):
            if votes and name.startswith("ord"):
                continue
            self.flat[name] = torch.full((n_rows * stride + GUARD,), SENT, dtype=torch.int32, device="cuda")
            setattr(self.c, name, self.flat[name][:n_rows * stride].view(n_rows, stride))
        for name in ("n_conn", "n_ord", "max_kf", "max_w"):
            if votes and name == "n_ord":
                continue
            self.flat[name] = torch.full((n_rows + GUARD,), SENT, dtype=torch.int32, device="cuda")
            setattr(self.c, name, self.flat[name][:n_rows])

    def host(self):
        import torch
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in self.flat.items()}


def _run(rows, selfs, obs, n_kf, stride, mode=CONN, th=15, point_bad=None, kf_bad=None, kf_key=None, dense=0, table=0, before=(), after=(0,),
         obs_before=(), obs_after=(0,)):
    import torch
    from rgbd_pl_slam_amd import update_connections, local_keyframe_votes
    rs, rp = _csr(rows, before, after)
    os_, ok = _csr(obs, obs_before, obs_after)
    key = None if kf_key is None else torch.from_numpy(np.array(kf_key, np.int64)).cuda()
    out = _Out(len(rows), stride, mode == VOTES)
    if mode == CONN:
        update_connections(rs, rp, torch.from_numpy(np.array(selfs, np.int32)).cuda(), os_, ok, n_kf, stride, th, _u8(point_bad), key, dense, table, out=out.c)
    else:
        local_keyframe_votes(rs, rp, os_, ok, n_kf, stride, _u8(point_bad), _u8(kf_bad), key, dense, table, out=out.c)
    return out


def _reference(rows, selfs, obs, n_kf, mode, th, point_bad, kf_bad, kf_key):
    if mode == CONN:
        return [covisref.update_connections(row, selfs[r], obs, n_kf, th, point_bad, kf_key) for r, row in enumerate(rows)]
    return [covisref.local_keyframe_votes(row, obs, n_kf, point_bad, kf_bad, kf_key) for row in rows]


def _compare(h, ref, stride, votes):
    """every element of every output, written or not, against the restatement's rows"""
    n_rows = len(ref)
    lists = (("conn", "conn_kf", "conn_w", "n_conn"),) if votes else (("conn", "conn_kf", "conn_w", "n_conn"), ("ord", "ord_kf", "ord_w", "n_ord"))
    for name, v in h.items():                                      # the guard behind the last row
        size = n_rows * stride if name in ("conn_kf", "conn_w", "ord_kf", "ord_w") else n_rows
        assert (v[size:] == SENT).all(), (name, "guard overwritten")
    for r, e in enumerate(ref):
        for lname, kf, w, n in lists:
            row_kf, row_w = h[kf][r * stride:(r + 1) * stride], h[w][r * stride:(r + 1) * stride]
            if e is None:
                assert h[n][r] == 0 and (row_kf == SENT).all() and (row_w == SENT).all(), (r, lname, "an empty row was written", row_kf[:8], h[n][r])
                continue
            want = e[lname]
            k = min(len(want), stride)
            assert h[n][r] == len(want), (r, lname, "count", int(h[n][r]), len(want))
            assert row_kf[:k].tolist() == [x for x, _ in want[:k]], (r, lname, row_kf[:k].tolist()[:12], want[:12])
            assert row_w[:k].tolist() == [x for _, x in want[:k]], (r, lname, row_w[:k].tolist()[:12], want[:12])
            assert (row_kf[k:] == -1).all() and (row_w[k:] == SENT).all(), (r, lname, "filler")
        if e is None:
            assert h["max_kf"][r] == -1 and h["max_w"][r] == SENT, (r, "max of an empty row")
        else:
            assert (int(h["max_kf"][r]), int(h["max_w"][r])) == tuple(e["max"]), (r, "max", h["max_kf"][r], h["max_w"][r], e["max"])


def _check(rows, selfs, obs, n_kf, stride, mode=CONN, th=15, point_bad=None, kf_bad=None, kf_key=None, dense=0, table=0, **filler):
    out = _run(rows, selfs, obs, n_kf, stride, mode, th, point_bad, kf_bad, kf_key, dense, table, **filler)
    ref = _reference(rows, selfs, obs, n_kf, mode, th, point_bad, kf_bad, kf_key)
    h = out.host()
    _compare(h, ref, stride, mode == VOTES)
    return out, h, ref


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]), k


# ---- 1. the hand-worked fixture
@pytest.mark.parametrize("keyed", [True, False])
def test_the_hand_worked_fixture_in_both_modes(keyed):
    fx = load_fixture()
    key = fx["kf_key"] if keyed else None
    rows, n_kf = fx["rows"], fx["n_kf"]
    out, h, ref = _check(rows, list(range(n_kf)), fx["obs"], n_kf, 8, CONN, fx["th"], fx["point_bad"], None, key)
    want = fx["connections_with_keys" if keyed else "connections_with_slots"]
    assert [None if e is None else {k: [list(x) for x in v] if k != "max" else list(v) for k, v in e.items()} for e in ref] == want
    assert h["n_ord"][:n_kf].tolist() == [0 if e is None else len(e["ord"]) for e in want]
    v = fx["votes"]
    _, hv, refv = _check(v["rows"], None, fx["obs"], n_kf, 8, VOTES, 1, fx["point_bad"], v["kf_bad"], key)
    assert [None if e is None else [list(x) for x in e["conn"]] for e in refv] == [None if e is None else e["conn"] for e in v["with_keys" if keyed else "with_slots"]]
    if keyed:
        import torch
        b = fx["best_covisibility"]
        best, n_best = out.c.best_covisibility(b["N"])
        torch.cuda.synchronize()
        assert best[b["row"], :int(n_best[b["row"]])].tolist() == b["with_keys"]
        for case in fx["by_weight"]["cases_with_keys"]:
            n = out.c.covisibles_by_weight(case["w"])
            torch.cuda.synchronize()
            r = fx["by_weight"]["row"]
            assert out.c.ord_kf[r, :int(n[r])].tolist() == case["result"], case["what"]
            assert int(n[5]) == 0                                   # the row without a neighbour: n_ord = 0


def _single_observer_world(lengths, n_kf):
    """row r holds lengths[r] points, point j of it seen by keyframe (r + 1 + j) % n_kf alone and by the row's keyframe r"""
    obs, rows = [], []
    for r, n in enumerate(lengths):
        rows.append(list(range(len(obs), len(obs) + n)))
        obs += [[r, (r + 1 + j) % n_kf] for j in range(n)]
    return rows, obs


# ---- 2. loop edges
def test_row_lengths_and_observation_counts_at_the_loop_edges():
    lengths = [0, 1, 63, 64, 65, 255, 256, 257, 3001]
    n_kf = 700
    rows, obs = _single_observer_world(lengths, n_kf)
    _check(rows, list(range(len(rows))), obs, n_kf, 700, CONN, 3)          # the long row wraps round the table: weights 4 and 5
    rng = np.random.default_rng(0)
    obs = [[int(k) for k in rng.choice(n_kf, n, replace=False)] for n in (1, 64, 65, 600, 7, 8, 9)]
    rows = [[0, 1, 2, 3, 4, 5, 6], [3], [], [1, 2]]
    _check(rows, [int(obs[3][0]), -1, 5, int(obs[1][63])], obs, n_kf, 640, CONN, 2)
    _check(rows, None, obs, n_kf, 640, VOTES, 1, kf_bad=[int(k % 3 == 0) for k in range(n_kf)])


# ---- 3. around stride
def test_counts_one_below_at_and_above_stride_and_untouched_memory():
    stride, n_kf = 8, 40
    obs, rows = [], []
    for n_conn, n_ord in ((7, 7), (8, 8), (9, 9), (0, 0), (12, 7), (12, 8), (12, 9), (3, 0), (0, 0)):
        row = []
        for j in range(n_conn):                                     # neighbour j + 1, seen twice if it belongs to the ordered list
            for _ in range(2 if j < n_ord else 1):
                row.append(len(obs)); obs.append([0, j + 1])
        rows.append(row)
    rows[3] = [len(obs)]; obs.append([0])                           # only the row's own observation: an empty count
    out, h, ref = _check(rows, [0] * len(rows), obs, n_kf, stride, CONN, 2)
    assert h["n_conn"][:9].tolist() == [7, 8, 9, 0, 12, 12, 12, 3, 0] and h["n_ord"][:9].tolist() == [7, 8, 9, 0, 7, 8, 9, 1, 0]
    assert ref[3] is None and ref[8] is None and len(ref[7]["ord"]) == 1
    _check(rows, None, obs, n_kf, stride, VOTES, 1, kf_bad=[1] + [0] * 39)
    # votes whose every counted keyframe is bad: a result (filler written), no local keyframe, no maximum
    _, h, ref = _check([[0, 1]], None, [[3], [3, 4]], n_kf, stride, VOTES, 1, kf_bad=[0, 0, 0, 1, 1] + [0] * 35)
    assert ref == [{"conn": [], "max": (-1, 0)}] and h["conn_kf"][:stride].tolist() == [-1] * stride


def _list_world(L, n_kf, weights, rng):
    """one row whose ordered list (th = 1) has L entries: neighbour i gets weights(i) by being seen in that many points"""
    kfs = [int(k) for k in rng.permutation(np.arange(1, n_kf))[:L]]
    w = [weights(i) for i in range(L)]
    obs = [[0] + [k for k, wk in zip(kfs, w) if wk > j] for j in range(max(w) if w else 0)]
    return list(range(len(obs))), obs


# ---- 4. sort edges
@pytest.mark.parametrize("L", [1, 2, 63, 64, 65, 1023, 1024, 1025, 4100])
def test_ordered_lists_at_the_sort_edges(L):
    rng = np.random.default_rng(L)
    n_kf = 4200 if L > 1025 else 1100
    key = [int(k) for k in rng.permutation(n_kf) * 3 - 1000]          # a random permutation, negative keys included
    cases = [("equal", lambda i: 1), ("mixed", lambda i: 1 + (i * 7919) % 5)]
    if L <= 65:
        cases.append(("distinct", lambda i: 1 + (i * 37) % L if L > 1 else 1))
    rows, obs, selfs = [], [], []
    for _, weights in cases:
        row, o = _list_world(L, n_kf, weights, rng)
        rows.append([p + len(obs) for p in row]); obs += o; selfs.append(0)
    rows.append([])
    selfs.append(0)
    for k in (key, None):
        _, h, ref = _check(rows, selfs, obs, n_kf, L + 3, CONN, 1, kf_key=k)
        assert h["n_ord"][:len(cases)].tolist() == [L] * len(cases)
        if L in (65,):
            assert sorted(w for _, w in ref[2]["ord"]) == list(range(1, L + 1))       # all weights distinct
    _check(rows, selfs, obs, n_kf, L + 3, CONN, 3, kf_key=key)                         # a threshold inside the mixed weights
    if L > 4096:                                                                       # the same long lists out of the table (gathered and sorted in global
        _, dense, _ = _check(rows, selfs, obs, n_kf, L + 3, CONN, 1, kf_key=key)           # memory) and out of the global counters of a row that fills a small table
        _, table, _ = _check(rows, selfs, obs, n_kf, L + 3, CONN, 1, kf_key=key, dense=1, table=8192)
        _, small, _ = _check(rows, selfs, obs, n_kf, L + 3, CONN, 1, kf_key=key, dense=1, table=64)
        _same(dense, table); _same(dense, small)


# ---- 5. the three counting paths
def _random_world(seed, n_kf, n_points, bad=True, cap=60):
    """long-tailed observation counts: most points seen by a few keyframes, a few by dozens (capped, so that the restatement stays quick)"""
    rng = np.random.default_rng(seed)
    cnt = np.minimum(min(n_kf, cap), 1 + (rng.pareto(1.2, n_points) * 3).astype(np.int64))
    obs = [[int(k) for k in rng.choice(n_kf, int(c), replace=False)] for c in cnt]
    rows = [[] for _ in range(n_kf)]
    for p, o in enumerate(obs):
        for k in o:
            rows[k].append(p)
    for r in rows:
        if len(r) > 3:
            r.insert(2, -1); r.append(r[0])                          # a null entry, a point listed twice
    point_bad = [int(x) for x in rng.integers(0, 12, n_points) == 0] if bad else None
    key = [int(k) for k in rng.permutation(n_kf).astype(np.int64) * 0x10001 + 0x7f0000000000]   # pointer-like
    return rows, obs, point_bad, key


@pytest.mark.parametrize("mode", [CONN, VOTES])
def test_every_counting_path_gives_identical_outputs(mode):
    n_kf = 300
    rows, obs, point_bad, key = _random_world(5, n_kf, 3000)
    rows += [[p] for p in range(len(obs)) if len(obs[p]) <= 2 and not point_bad[p]][:6] + [[]]   # short rows: they stay in the small tables
    selfs = list(range(n_kf)) + [-1] * 7 if mode == CONN else None
    kf_bad = [int(k % 7 == 0) for k in range(n_kf)] if mode == VOTES else None
    for k in (None, key):
        _, dense, ref = _check(rows, selfs, obs, n_kf, 64, mode, 15, point_bad, kf_bad, k)
        distinct = [len(covisref._count(r, s, obs, n_kf, point_bad)) for r, s in zip(rows, selfs or [None] * len(rows))]
        assert max(distinct) > 56 and 0 < sorted(distinct)[1] <= 2   # rows on both sides of the limits of the 64- and 2-entry tables
        _, table, _ = _check(rows, selfs, obs, n_kf, 64, mode, 15, point_bad, kf_bad, k, dense=1)
        _, small, _ = _check(rows, selfs, obs, n_kf, 64, mode, 15, point_bad, kf_bad, k, dense=1, table=64)
        _, tiny, _ = _check(rows, selfs, obs, n_kf, 64, mode, 15, point_bad, kf_bad, k, dense=1, table=2)
        _same(dense, table); _same(dense, small); _same(dense, tiny)


# ---- 6. garbage
def test_out_of_range_ids_are_skipped_and_filler_is_never_read():
    n_kf = 50
    rows, obs, point_bad, key = _random_world(9, n_kf, 400)
    selfs = list(range(n_kf))
    _, clean, _ = _check(rows, selfs, obs, n_kf, 50, CONN, 4, point_bad, None, key)
    big = 0x7FC00000                                                 # a float NaN's bit pattern, and a huge index
    dirty_obs = [o + [-5, n_kf, big, -2 ** 31] for o in obs]
    dirty_rows = [r + [-7, len(obs), big, -2 ** 31] for r in rows]
    fill = (big, -1, 0x7FFFFFFF, 3, -2 ** 31, big)
    _, dirty, _ = _check(dirty_rows, selfs, dirty_obs, n_kf, 50, CONN, 4, point_bad, None, key, before=fill, after=fill * 40, obs_before=fill,
                         obs_after=fill * 40)
    _same(clean, dirty)
    _, votes_clean, _ = _check(rows, None, obs, n_kf, 50, VOTES, 1, point_bad, [1, 0] * 25, key)
    _, votes_dirty, _ = _check(dirty_rows, None, dirty_obs, n_kf, 50, VOTES, 1, point_bad, [1, 0] * 25, key, before=fill, after=fill * 40,
                               obs_before=fill, obs_after=fill * 40)
    _same(votes_clean, votes_dirty)


# ---- 7. randomised
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_maps_all_rows_at_once_equal_one_row_per_call(seed):
    import torch
    from rgbd_pl_slam_amd import update_connections
    n_kf, stride = 200, 48
    rows, obs, point_bad, key = _random_world(seed, n_kf, 5000)
    selfs = list(range(n_kf))
    _, h, _ = _check(rows, selfs, obs, n_kf, stride, CONN, 15, point_bad, None, key)
    _same(h, _run(rows, selfs, obs, n_kf, stride, CONN, 15, point_bad, None, key).host())                                               # two identical calls are bit-equal
    _check(rows, None, obs, n_kf, stride, VOTES, 1, point_bad, [int(k % 5 == 1) for k in range(n_kf)], key)
    # the same rows, one per call, into the same sentinel-filled outputs
    rs, rp = _csr(rows)
    os_, ok = _csr(obs)
    dkey, dbad = torch.from_numpy(np.array(key, np.int64)).cuda(), _u8(point_bad)
    dself = torch.arange(n_kf, dtype=torch.int32, device="cuda")
    one = _Out(n_kf, stride, False)
    for r in range(n_kf):
        from rgbd_pl_slam_amd import Covisibility
        c = Covisibility(1, stride, torch.device("cuda", 0), False, None)
        for name in ("conn_kf", "conn_w", "ord_kf", "ord_w"):
            setattr(c, name, getattr(one.c, name)[r:r + 1])
        for name in ("n_conn", "n_ord", "max_kf", "max_w"):
            setattr(c, name, getattr(one.c, name)[r:r + 1])
        update_connections(rs[r:r + 2], rp, dself[r:r + 1], os_, ok, n_kf, stride, 15, dbad, dkey, out=c)
    _same(h, one.host())


# ---- 8. the chain into the keyframe database
def test_the_rows_feed_the_keyframe_database_without_a_host_round_trip():
    import torch
    import kfdbref
    import bowref
    import test_gpu_kfdb as K
    from rgbd_pl_slam_amd import update_connections
    n_kf = S = 60
    bows, _, queries = K._world(4, n_kf, S)
    db, model = K._pair(bowref.L1_NORM, S)
    db.add(K._pack(bows, K.CAP), range(n_kf)); model.add(bows, range(n_kf))
    rows, obs, point_bad, key = _random_world(21, n_kf, 900)
    rows[7] = []                                                                         # a keyframe without a neighbour, and one whose points are all bad:
    rows[8] = [p for p in range(len(obs)) if point_bad[p]][:5] + [-1]                    # their rows are not written, and must read as empty lists
    rs, rp = _csr(rows)
    os_, ok = _csr(obs)
    junk = torch.arange(n_kf * S, dtype=torch.int32, device="cuda") % S                  # what a recycled allocation may hold: plausible slots
    del junk
    cov = update_connections(rs, rp, torch.arange(n_kf, dtype=torch.int32, device="cuda"), os_, ok, n_kf, S, 6, _u8(point_bad),
                             torch.from_numpy(np.array(key, np.int64)).cuda())
    ref = [covisref.update_connections(row, s, obs, n_kf, 6, point_bad, key) for s, row in enumerate(rows)]
    covis = [[] if e is None else [k for k, _ in e["ord"]] for e in ref]
    conn = [[] if e is None else [k for k, _ in e["conn"]] for e in ref]
    assert max(len(c) for c in covis) > 10                                               # longer than the n_best = 10 the database reads
    torch.cuda.synchronize()                                                             # the database runs on its own stream
    got = K._results(db.detect_relocalization_candidates(K._pack(queries, K.CAP), cov.covis_csr(), 64), 64)
    assert got == K._expect(model.detect_reloc(queries, covis), 64) and any(g[1] for g in got)
    assert ref[7] is None and ref[8] is None
    torch.cuda.synchronize()
    assert (cov.ord_kf[7:9] == -1).all() and (cov.conn_kf[7:9] == -1).all() and cov.n_ord[7:9].tolist() == [0, 0]
    solo = [list(bows[7]), list(bows[8])]                                                # queries that score keyframes 7 and 8 themselves: their rows are read
    got = K._results(db.detect_relocalization_candidates(K._pack(solo, K.CAP), cov.covis_csr(), 64), 64)
    assert got == K._expect(model.detect_reloc(solo, covis), 64)
    qs = [3, 7, 17, 0, 8, 59, 31]                                                        # loop queries: keyframes of the graph, the two empty rows among them
    qb = [list(bows[q]) for q in qs]
    excl = cov.connected_csr(torch.tensor(qs, device="cuda"))
    ms = torch.zeros(len(qs), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    got = K._results(db.detect_loop_candidates(K._pack(qb, K.CAP), ms, cov.covis_csr(), excl, 64), 64)
    assert got == K._expect(model.detect_loop(qb, [0.0] * len(qs), covis, [conn[q] for q in qs]), 64)
    assert any(len(conn[q]) for q in qs)


# ---- 9. GetCovisiblesByWeight
def test_covisibles_by_weight_equals_the_restatement():
    import torch
    n_kf, stride = 120, 120
    rows, obs, point_bad, key = _random_world(13, n_kf, 1500)
    rows[7] = []; rows[8] = [-1]
    out, h, ref = _check(rows, list(range(n_kf)), obs, n_kf, stride, CONN, 4, point_bad, None, key)
    tops = [e["ord"][0][1] for e in ref if e]
    for w in (-3, 0, 1, 4, 5, 6, 9, max(tops), max(tops) + 1):
        n = out.c.covisibles_by_weight(w)
        torch.cuda.synchronize()
        n = n.cpu().numpy()
        for r, e in enumerate(ref):
            want = covisref.covisibles_by_weight(e["ord"] if e else [], w)
            assert h["ord_kf"][r * stride:r * stride + n[r]].tolist() == want, (w, r)
    assert ref[7] is None and ref[8] is None

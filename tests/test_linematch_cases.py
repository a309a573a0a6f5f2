"""The reach proof of tests/test_gpu_line_match.py, on the CPU: every promise of tests/linematch_cases.py is asserted on the oracle alone (spreads, accepted
counts, who wins a contended train line, which rows fuse, the tie rows), so that the GPU tests cannot pass vacuously; and orc_knn2_hamming /
orc_line_mad are restated in a few lines of numpy that must equal the C oracle bit for bit at every one of these shapes."""
import time

import numpy as np
import pytest

import linematch_cases as lc
import orc


# ---------------------------------------------------------------- the restatement
def np_knn2(q, t):
    """cv::batchDistance, K = 2: the two smallest of (distance, train index) in that order"""
    d = lc.hamming(q, t)
    nq, nt = d.shape
    idx = np.full((nq, 2), -1, np.int32); dist = np.full((nq, 2), 0x7fffffff, np.int32)
    if nt == 0:
        return idx, dist
    rows = np.arange(nq)
    idx[:, 0] = d.argmin(1); dist[:, 0] = d[rows, idx[:, 0]]
    if nt > 1:
        d = d.astype(np.int64); d[rows, idx[:, 0]] = 1 << 40
        idx[:, 1] = d.argmin(1); dist[:, 1] = d[rows, idx[:, 1]]
    return idx, dist


def np_gaps(dist):
    return dist[:, 1].astype(np.float32) - dist[:, 0].astype(np.float32)


def _np_mad(v):
    n = len(v)
    med = np.float64(np.sort(v)[n // 2])
    dev = np.abs((v.astype(np.float64) - med).astype(np.float32))
    return 1.4826 * np.float64(np.sort(dev)[n // 2])


def np_line_mad(dist):
    return _np_mad(dist[:, 0].astype(np.float32)), _np_mad(np_gaps(dist))


def knn_cases():
    """(name, query, train) of every 2-NN table the GPU tests build"""
    for c in lc.sizes() + [lc.large(n) for n in lc.LARGE_NQ] + [lc.large_train(), lc.zero_mad(301), lc.zero_mad(300), lc.median_split(4), lc.median_split(256), lc.shared_train()]:
        yield c["name"], c["query"], c["train"]
    for nlast in lc.BATCH_NLAST:
        c = lc.tile_ties(nlast)
        for F in c["frames"]:
            yield "%s_frame%d" % (c["name"], len(F)), c["last"], F
    for c in lc.fuse_edges():
        yield c["name"], c["ml"], c["kf"]


def accepted(c, factor=0.5):
    """the queries the last-frame rule accepts, from the oracle's table and spread"""
    idx, dist = orc.knn2(c["query"], c["train"])
    th = orc.line_mad(dist)[1] * factor
    return idx, dist, (np_gaps(dist).astype(np.float64) > th) & (c["has_mapline"] != 0)


# ---------------------------------------------------------------- the generator itself
def test_flip_exact_flips_exactly_and_quickly():
    rng = np.random.default_rng(0)
    base = lc.anchors(rng, 18000); counts = rng.integers(0, 257, 18000)
    t0 = time.perf_counter()
    out = lc.flip_exact(base, counts, rng)
    dt = time.perf_counter() - t0
    print("flip_exact: 18000 rows in %.3f s" % dt)
    assert np.array_equal(np.unpackbits(base ^ out, axis=1).sum(1), counts)
    assert np.array_equal(lc.flip_exact(base[:3], 256, rng), ~base[:3])
    assert dt < 1.0


def test_numpy_restatement_equals_the_c_oracle_bit_for_bit():
    n = 0
    for name, q, t in knn_cases():
        if len(q) == 0:
            continue
        idx, dist = orc.knn2(q, t)
        nidx, ndist = np_knn2(q, t)
        assert np.array_equal(idx, nidx) and np.array_equal(dist, ndist), name
        a, b = orc.line_mad(dist)
        na, nb = np_line_mad(dist)
        assert np.float64(a).tobytes() == np.float64(na).tobytes() and np.float64(b).tobytes() == np.float64(nb).tobytes(), name
        n += 1
    assert n > 60


# ---------------------------------------------------------------- sizes
def test_sizes_span_every_boundary():
    cs = lc.sizes()
    pairs = [(len(c["query"]), len(c["train"])) for c in cs]
    main = [p for p in pairs if p[0] != 5]
    assert sorted(p[0] for p in main) == [1, 2, 3, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 4097]
    for nt in (2, 3, 130):
        par = {p[0] % 2 for p in main if p[1] == nt}
        assert par == {0, 1}, nt
    assert sorted(p[1] for p in pairs if p[0] == 5) == [1, 127, 128, 129, 256, 257]
    assert max(p[0] for p in pairs) <= lc.SIZES_MAX_LINES
    differ, matched = 0, 0
    for c in cs:
        nq, nt = len(c["query"]), len(c["train"])
        idx, dist = orc.knn2(c["query"], c["train"])
        # the nearest line is the one the query was copied from, at exactly the number of flipped bits
        assert np.array_equal(dist[:, 0], c["flips"]) and np.array_equal(c["train"][idx[:, 0]], c["train"][c["which"]]), c["name"]
        if nt == 1:
            assert np.all(idx[:, 1] == -1) and np.all(dist[:, 1] == 0x7fffffff)
        v = np.sort(np_gaps(dist))
        if nq % 2 == 0 and v[nq // 2] != v[(nq - 1) // 2]:
            differ += 1
        match, n = orc.match_lines_knn(c["query"], c["train"], c["has_mapline"])
        assert n == (accepted(c)[2].sum() if nt >= 2 else 0), c["name"]
        matched += n
    assert differ >= 1 and matched > 1000
    print("sizes: %d even-n cases where v[n/2] != v[(n-1)/2], %d accepted in all" % (differ, matched))


# ---------------------------------------------------------------- large
@pytest.mark.parametrize("nq", lc.LARGE_NQ)
def test_large_accepts_about_half_and_the_winners_come_last(nq):
    c = lc.large(nq)
    idx, dist, acc = accepted(c)
    match, n = orc.match_lines_knn(c["query"], c["train"], c["has_mapline"])
    assert n == acc.sum() and 0.4 * nq < n < 0.6 * nq
    for t in range(3):
        cont = np.flatnonzero(acc & (idx[:, 0] == t))
        assert len(cont) > 2000 and match[t] == cont[-1] and match[t] >= nq - 25, (t, len(cont), match[t])
    v = np.sort(np_gaps(dist))
    print("%s: %d accepted, winners %s, v[n/2] %s v[(n-1)/2]" % (c["name"], n, match.tolist(), "!=" if v[nq // 2] != v[(nq - 1) // 2] else "=="))


def test_large_train_set():
    c = lc.large_train()
    idx, dist = orc.knn2(c["query"], c["train"])
    assert len(c["train"]) == 18000 and np.array_equal(idx[:, 0], c["which"]) and np.array_equal(dist[:, 0], c["flips"])
    assert idx[:, 0].max() > 16384 and orc.match_lines_knn(c["query"], c["train"], c["has_mapline"])[1] > 10


# ---------------------------------------------------------------- zero spread
@pytest.mark.parametrize("nq", [301, 300])
def test_zero_mad_threshold_is_zero_and_the_rule_is_strict(nq):
    c = lc.zero_mad(nq)
    idx, dist = orc.knn2(c["query"], c["train"])
    gaps = np_gaps(dist)
    assert np.array_equal(gaps == 0, c["near_dup"]) and (gaps == 0).sum() > nq / 2
    assert orc.line_mad(dist)[1] == 0.0
    want = int((dist[:, 1] > dist[:, 0]).sum())
    assert 0 < want < nq
    match, n = orc.match_lines_knn(c["query"], c["train"], c["has_mapline"])
    assert n == want
    none = np.zeros(nq, np.uint8); no_t = np.zeros(len(c["train"]), np.uint8)
    for factor in (0.0, 0.1):
        m12, n12 = orc.lines_search_for_triangulation(c["query"], c["train"], none, no_t, none, no_t, 0, factor)
        assert n12 == want and np.array_equal(m12 >= 0, gaps > 0)
    print("%s: %d of %d gaps are zero, nn12_mad 0.0, %d accepted" % (c["name"], (gaps == 0).sum(), nq, n))


# ---------------------------------------------------------------- which element is the median
@pytest.mark.parametrize("nq", [4, 256])
def test_median_split_accepted_set_depends_on_the_upper_median(nq):
    c = lc.median_split(nq)
    idx, dist = orc.knn2(c["query"], c["train"])
    gaps = np_gaps(dist)
    assert np.array_equal(gaps, c["gaps"]) and np.all(idx == [0, 1])
    v = np.sort(gaps)
    assert v[nq // 2] == 30 and v[(nq - 1) // 2] == 20
    assert orc.line_mad(dist)[1] == 1.4826 * 30
    match, n = orc.match_lines_knn(c["query"], c["train"], c["has_mapline"])
    assert n == nq // 2 == (gaps >= 30).sum()
    # the rule around the lower median: a spread of 1.4826 * 20 and the queries at gap 20 accepted as well
    low = 1.4826 * np.float64(np.sort(np.abs(gaps - v[(nq - 1) // 2]))[nq // 2])
    assert low == 1.4826 * 20 and (gaps > 0.5 * low).sum() == 3 * nq // 4


# ---------------------------------------------------------------- contended train lines
def test_shared_train_winner_is_the_last_accepted_not_the_last_near():
    c = lc.shared_train()
    idx, dist, acc = accepted(c)
    assert np.array_equal(idx[:, 0], c["near"])                      # every query's nearest is the line it was copied from ...
    r = c["runner_up"]
    assert idx[r, 0] == 0 and idx[r, 1] == c["partner"] and dist[r, 0] == dist[r, 1] and c["has_mapline"][r] and not acc[r]   # ... the tie included
    match, n = orc.match_lines_knn(c["query"], c["train"], c["has_mapline"])
    assert n == acc.sum() and n > 300 and set(np.flatnonzero(match >= 0)) == set(lc.SHARED_TRAINS)
    for t in lc.SHARED_TRAINS:
        near = np.flatnonzero(c["near"] == t)
        assert near[-1] == c["top"][t] and not c["has_mapline"][near[-1]]
        assert match[t] == c["winner"][t] == np.flatnonzero(acc & (idx[:, 0] == t))[-1] < near[-1]
        # contenders in other waves and other strides of a 256-thread block
        cont = np.flatnonzero(acc & (idx[:, 0] == t))
        assert len({q // 64 for q in cont}) > 5 and len({q // 256 for q in cont}) == 3
    assert c["winner"][0] < r < c["top"][0]
    print("shared_train: %d accepted onto %d train lines" % (n, (match >= 0).sum()))


# ---------------------------------------------------------------- the tile of the batch kernel
@pytest.mark.parametrize("nlast", lc.BATCH_NLAST)
def test_tile_ties_rows(nlast):
    c = lc.tile_ties(nlast)
    assert [len(F) for F in c["frames"]] == list(lc.BATCH_FRAME_SIZES) and len(c["last"]) == nlast
    tables = {f: orc.knn2(c["last"], F) for f, F in enumerate(c["frames"]) if len(F)}
    for f, rows in c["expect"].items():
        idx, dist = tables[f]
        for q, (i0, i1, d0, d1) in rows.items():
            assert (idx[q, 0], idx[q, 1], dist[q, 0], dist[q, 1]) == (i0, i1, d0, d1), (f, q)
    idx, dist = tables[c["identical"]]
    assert np.all(idx == [0, 1]) and np.array_equal(dist[:, 0], dist[:, 1])
    # the tie across the tile edge is the nearest pair of every query near pool[127] / pool[0]
    f129 = lc.BATCH_FRAME_SIZES.index(129); f256 = lc.BATCH_FRAME_SIZES.index(256)
    near127 = np.flatnonzero(c["which"] == 127)
    assert len(near127) >= 3 and np.all(tables[f129][0][near127] == [127, 128]) and np.all(tables[f129][1][near127, 0] == tables[f129][1][near127, 1])
    near0 = np.flatnonzero(c["which"] == 0)
    assert len(near0) >= 3 and np.all(tables[f256][0][near0] == [0, 128])
    # frames of two or more lines match something (the complement pair and the identical set have no spread: nothing), shorter ones nothing
    total = 0
    for f, F in enumerate(c["frames"]):
        n = orc.match_lines_knn(c["last"], F, c["has_mapline"])[1]
        if len(F) in (0, 1, 2, 130):
            assert n == 0
        total += n
    assert total > nlast


# ---------------------------------------------------------------- Fuse
def test_fuse_edges_fuse_up_to_th_low_and_pick_the_first_minimum():
    cs = lc.fuse_edges()
    assert sorted(len(c["ml"]) for c in cs if len(c["kf"]) == 129) == list(lc.FUSE_M)
    assert sorted({len(c["kf"]) for c in cs}) == list(lc.FUSE_NKF) and all(len(c["ml"]) > 0 for c in cs)
    invalid_at_zero = 0
    for c in cs:
        best, n = orc.lines_fuse(c["kf"], c["ml"], c["valid"])
        n_kf = len(c["kf"])
        if n_kf == 0:
            assert n == 0 and np.all(best == -1)
            continue
        want = (c["flips"] <= lc.TH_LOW) & (c["valid"] != 0)
        assert np.array_equal(best >= 0, want) and n == want.sum(), c["name"]
        first = np.where(c["which"] == n_kf - 1, 0, c["which"]) if n_kf >= 2 else c["which"]   # the last line is a copy of line 0
        assert np.array_equal(best[want], first[want]), c["name"]
        if n_kf >= 2 and len(c["ml"]) > 7:
            assert np.any(want & (c["which"] == n_kf - 1))
        invalid_at_zero += int(((c["valid"] == 0) & (c["flips"] == 0)).sum())
        if len(c["ml"]) >= 7:
            assert {50, 51} <= set(c["flips"].tolist()) and np.any(want & (c["flips"] == 50))
    assert invalid_at_zero > 10

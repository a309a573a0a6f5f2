"""Directed inputs for the brute-force line matchers (k_knn2, k_knn2_batch, k_line_mad, k_lines_lastframe, k_lines_fuse_pick).  numpy only.

Descriptors are CONSTRUCTED: a few random 32-byte anchors and copies of them with an EXACT number of flipped bits, so the Hamming distance of a copy to
its anchor is known before any matcher runs.  Every case is a dict of arrays plus the property it promises; tests/test_linematch_cases.py proves the
promises on the CPU oracle, tests/test_gpu_line_match.py runs the cases through the six C entry points."""
import numpy as np

TH_LOW = 50
BATCH_FRAME_SIZES = (0, 1, 2, 127, 128, 129, 256, 257, 130)   # the tile of k_knn2_batch holds 128 descriptors
BATCH_NLAST = (127, 128, 129, 600)


def anchors(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


def flip_exact(desc, counts, rng, within=None):
    """copies of the rows of desc with exactly counts[i] distinct bits of row i flipped (one argsort: 18000 rows take a fraction of a second); within: a
    32-byte mask, only its set bits are flipped"""
    desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    n = len(desc)
    counts = np.broadcast_to(np.asarray(counts, np.int64), (n,))
    assert counts.min(initial=0) >= 0 and counts.max(initial=0) <= 256
    if n == 0:
        return desc.copy()
    keys = rng.random((n, 256), dtype=np.float32)
    if within is not None:
        allowed = np.unpackbits(np.asarray(within, np.uint8)).astype(bool)
        assert counts.max(initial=0) <= allowed.sum()
        keys[:, ~allowed] = 2.0
    order = np.argsort(keys, axis=1)          # a random permutation of the 256 bit positions per row (the allowed ones first)
    mask = np.zeros((n, 256), np.uint8)
    np.put_along_axis(mask, order, (np.arange(256)[None, :] < counts[:, None]).astype(np.uint8), axis=1)
    return desc ^ np.packbits(mask, axis=1)


def hamming(a, b):
    """(len(a), len(b)) int32 table of Hamming distances"""
    pop = np.unpackbits(np.arange(256, dtype=np.uint8)[:, None], axis=1).sum(1).astype(np.int32)
    a = np.ascontiguousarray(a, np.uint8).reshape(-1, 32); b = np.ascontiguousarray(b, np.uint8).reshape(-1, 32)
    out = np.zeros((len(a), len(b)), np.int32)
    for k in range(32):   # one byte column at a time keeps the temporary at len(a) x len(b)
        out += pop[a[:, k, None] ^ b[None, :, k]]
    return out


def _near(rng, train, nq, max_flips, p_has):
    """nq queries, each a train row with 0 .. max_flips exact flips; which = the row, flips = the count"""
    which = rng.integers(0, len(train), nq)
    flips = rng.integers(0, max_flips + 1, nq)
    return dict(query=flip_exact(train[which], flips, rng), train=train, which=which, flips=flips,
                has_mapline=(rng.random(nq) < p_has).astype(np.uint8))


# ---------------------------------------------------------------- sizes
SIZE_PAIRS = [(1, 2), (2, 3), (3, 130), (127, 130), (128, 2), (129, 3), (255, 2), (256, 3), (257, 130), (511, 3), (512, 130), (513, 2),
              (1023, 3), (1024, 2), (1025, 130), (4097, 3)] + [(5, nt) for nt in (1, 127, 128, 129, 256, 257)]
SIZES_MAX_LINES = 4097


def sizes():
    """every power-of-two edge of the sort (and the 4-stride, 17-stride loops of a 256-thread block) against small train sets, and five queries against
    train sets at the tile edges; queries are anchors with 0 .. 59 exact flips"""
    out = []
    for k, (nq, nt) in enumerate(SIZE_PAIRS):
        rng = np.random.default_rng(1000 + k)
        c = _near(rng, anchors(rng, nt), nq, 59, 0.7)
        c["name"] = "nq%d_nt%d" % (nq, nt)
        out.append(c)
    return out


# ---------------------------------------------------------------- large
LARGE_NQ = (16384, 16385, 18000)


def large(nq):
    """nq queries against 3 train lines (thousands of contenders per train, has_mapline at 0.5): next_pow2(nq) * 4 bytes of LDS -- 64 KB at 16384,
    128 KB from 16385"""
    rng = np.random.default_rng(2000 + nq)
    c = _near(rng, anchors(rng, 3), nq, 59, 0.5)
    c["name"] = "large_nq%d" % nq
    return c


def large_train():
    """64 queries against 18000 train lines"""
    rng = np.random.default_rng(2999)
    c = _near(rng, anchors(rng, 18000), 64, 59, 0.5)
    c["name"] = "large_nt18000"
    return c


# ---------------------------------------------------------------- zero spread
def zero_mad(nq=301):
    """30 train lines: 10 anchors present twice (indices 2k, 2k + 1) and 10 unique ones.  60 % of the queries are copies of a duplicated anchor: their two
    nearest neighbours are equally far, so more than half of the gaps d2 - d1 are 0, nn12_mad is exactly 0 and so is every threshold.  Every line
    holds a MapLine on the query side (has_mapline all 1): the accepted queries are exactly those with d2 > d1."""
    rng = np.random.default_rng(3000 + nq)
    a = anchors(rng, 20)
    train = np.concatenate([np.repeat(a[:10], 2, axis=0), a[10:]])
    ndup = int(round(0.6 * nq))
    near_dup = np.zeros(nq, bool); near_dup[rng.permutation(nq)[:ndup]] = True
    which = np.where(near_dup, rng.integers(0, 20, nq), rng.integers(20, 30, nq))
    flips = rng.integers(0, 10, nq)
    return dict(name="zero_mad_nq%d" % nq, query=flip_exact(train[which], flips, rng), train=train, which=which, flips=flips, near_dup=near_dup,
                has_mapline=np.ones(nq, np.uint8))


# ---------------------------------------------------------------- which element is the median
SPLIT_GAPS = (0, 20, 30, 100)


def median_split(nq):
    """nq (even, a multiple of 4) queries between two train lines exactly 100 bits apart: a query that flips k of those 100 bits of train 0 is k bits from
    train 0 and 100 - k from train 1.  A quarter of the queries each has the gap 0, 20, 30, 100, so v[n/2] = 30 and v[(n-1)/2] = 20.  Around 30 the
    spread is 1.4826 * 30 and the last-frame threshold 22.2: the queries at 30 and 100 are accepted, half of all.  Around 20 the threshold would be
    14.8 and the queries at 20 would pass too."""
    assert nq % 4 == 0
    rng = np.random.default_rng(3500 + nq)
    a = anchors(rng, 1)
    train = np.concatenate([a, flip_exact(a, 100, rng)])
    gaps = np.asarray(SPLIT_GAPS)[rng.permutation(nq) % 4]
    query = flip_exact(np.repeat(a, nq, axis=0), (100 - gaps) // 2, rng, within=train[0] ^ train[1])
    return dict(name="median_split_nq%d" % nq, query=query, train=train, gaps=gaps, has_mapline=np.ones(nq, np.uint8))


# ---------------------------------------------------------------- contended train lines
SHARED_TRAINS = (0, 3, 9, 14, 22)


def shared_train():
    """600 queries, every one a copy (0 .. 59 flips) of one of 5 train lines among 25.  For each of the 5 the highest-indexed query near it lacks a
    MapLine; for train 0 the second-highest sits exactly half way between train 0 and another train (gap 0: it fails the strict threshold), so the
    winner there is the third-highest.  The two (three) top contenders of a train hold a MapLine otherwise; the rest are drawn at 0.7."""
    rng = np.random.default_rng(4000)
    nq = 600
    train = anchors(rng, 25)
    near = np.asarray(SHARED_TRAINS)[rng.integers(0, 5, nq)]
    query = flip_exact(train[near], rng.integers(0, 60, nq), rng)
    has = (rng.random(nq) < 0.7).astype(np.uint8)
    # a partner of train 0 at an even distance, and the bits in which the two differ
    diff = np.unpackbits(train[0][None] ^ train, axis=1)
    partner = next(j for j in range(1, 25) if j not in SHARED_TRAINS and diff[j].sum() % 2 == 0)
    top, runner_up, winner = {}, None, {}
    for t in SHARED_TRAINS:
        qs = np.flatnonzero(near == t)
        top[t] = int(qs[-1]); has[qs[-1]] = 0
        if t == 0:
            runner_up = int(qs[-2])
            bits = np.flatnonzero(diff[partner])
            mask = np.zeros(256, np.uint8); mask[rng.permutation(bits)[:len(bits) // 2]] = 1
            query[runner_up] = train[0] ^ np.packbits(mask)
            has[runner_up] = 1; has[qs[-3]] = 1; winner[t] = int(qs[-3])
        else:
            has[qs[-2]] = 1; winner[t] = int(qs[-2])
    return dict(name="shared_train", query=query, train=train, near=near, has_mapline=has, top=top, runner_up=runner_up, partner=partner, winner=winner)


# ---------------------------------------------------------------- the 128-descriptor tile of the batch kernel
def tile_ties(nlast):
    """one last frame (nlast queries) against train sets of BATCH_FRAME_SIZES lines.  The sets are prefixes of one pool of 257 anchors (a query with f
    flips of pool[c] is f bits from line c of every set that holds it unchanged) with these rows replaced:
      2 lines     both the bitwise complement of query 0 (distance 256, twice)
      129 lines   127 == 128: a tie across the tile edge, the nearest of the queries near pool[127]
      256 lines   0 == 128: the same with the earlier line in tile 0
      257 lines   5 == 140 == 256 (a third tile of one line loses a three-way tie); line 150 is 1 bit and line 126 is 6 bits from pool[126] (best in
                  tile 1, second in tile 0); line 20 is 2 bits and line 129 is 7 bits from pool[129] (the reverse)
      130 lines   all equal to pool[7]: every row of the table is (0, 1) at equal distances
    Queries 0 .. 4 are exact copies of pool[127], pool[0], pool[5], pool[126], pool[129]; expect = {frame: {query: (i0, i1, d0, d1)}}."""
    rng = np.random.default_rng(5000 + nlast)
    pool = anchors(rng, 257)
    which = rng.integers(0, 257, nlast)
    special = np.asarray([127, 0, 5, 128, 256, 126, 129, 7, 140])
    which[::3] = special[np.arange(len(which[::3])) % len(special)]
    flips = rng.integers(0, 31, nlast)
    which[:5] = [127, 0, 5, 126, 129]; flips[:5] = 0
    last = flip_exact(pool[which], flips, rng)
    one = lambda row, f: flip_exact(row[None], [f], rng)[0]
    frames = []
    for n in BATCH_FRAME_SIZES:
        F = pool[:n].copy()
        if n == 2:
            F[:] = ~last[0]
        elif n == 129:
            F[128] = F[127]
        elif n == 256:
            F[128] = F[0]
        elif n == 257:
            F[140] = F[5]; F[256] = F[5]
            F[150] = one(pool[126], 1); F[126] = one(pool[126], 6)
            F[20] = one(pool[129], 2); F[129] = one(pool[129], 7)
        elif n == 130:
            F[:] = pool[7]
        frames.append(F)
    fi = {n: k for k, n in enumerate(BATCH_FRAME_SIZES)}
    expect = {fi[2]: {0: (0, 1, 256, 256)}, fi[129]: {0: (127, 128, 0, 0)}, fi[256]: {1: (0, 128, 0, 0)},
              fi[257]: {2: (5, 140, 0, 0), 3: (150, 126, 1, 6), 4: (20, 129, 2, 7)}}
    return dict(name="tile_ties_nlast%d" % nlast, last=last, which=which, flips=flips, frames=frames, expect=expect, identical=fi[130],
                has_mapline=(rng.random(nlast) < 0.7).astype(np.uint8))


# ---------------------------------------------------------------- Fuse
FUSE_FLIPS = (0, 49, 50, 51, 52, 128, 256)
FUSE_M = (1, 63, 64, 65, 255, 256, 257)
FUSE_NKF = (0, 1, 2, 129)


def fuse_case(m, n_kf):
    """m map lines, each a keyframe line with FUSE_FLIPS[i % 7] exact flips (TH_LOW and its neighbours, the far half, the complement).  With two or more
    keyframe lines, the last one is a copy of line 0: map lines near either must pick line 0.  Every 5th row with 0 flips is invalid."""
    rng = np.random.default_rng(6000 + 1000 * n_kf + m)
    kf = anchors(rng, n_kf)
    if n_kf >= 2:
        kf[-1] = kf[0]
    flips = np.asarray(FUSE_FLIPS)[np.arange(m) % len(FUSE_FLIPS)]
    which = rng.integers(0, max(n_kf, 1), m)
    which[::2] = np.where(rng.random(len(which[::2])) < 0.5, 0, max(n_kf, 1) - 1)   # half of the rows near the duplicated pair
    ml = flip_exact(kf[which] if n_kf else anchors(rng, m), flips, rng)
    valid = np.ones(m, np.uint8)
    zero = np.flatnonzero(flips == 0)
    valid[zero[::5][1:]] = 0
    return dict(name="fuse_m%d_nkf%d" % (m, n_kf), kf=kf, ml=ml, valid=valid, which=which, flips=flips)


def fuse_edges():
    return [fuse_case(m, 129) for m in FUSE_M] + [fuse_case(65, n_kf) for n_kf in FUSE_NKF if n_kf != 129]

"""numpy restatement of MapPoint::ComputeDistinctiveDescriptors (include/MapPoint.h:75; body in lib/libORB_SLAM2.so at so@0x94460, 0x122b bytes -- the upstream
routine).  MapLine::ComputeDistinctiveDescriptors (include/MapLine.h:93) has no body in the reference and is taken as the same rule (parity unpinned).

  1. mObservations is copied: iteration order = the order of the std::map                      -> the order of the rows handed in
  2. observations whose keyframe isBad() are left out (so@0x94706)                              -> `valid`
  3. none left: return, mDescriptor untouched                                                  -> (-1, -1)
  4. all pairs ORBmatcher::DescriptorDistance (so@0x94add), the diagonal is 0
  5. std::sort per row (so@0x94dd0); median = vDists[(int)(0.5 * (N - 1))] (vmulsd by 0.5 at so@0x94ec7, truncating convert at so@0x94edd)
  6. BestMedian starts at INT_MAX (so@0x94b4e), the update is a strict <: the earliest row wins ties -> np.argmin (first minimum)
  7. mDescriptor = vDescriptors[BestIdx].clone()
"""
import numpy as np


def hamming_matrix(d):
    """(N, 32) uint8 -> (N, N) int distances.  bits as float32: every dot product is an integer <= 256, exact"""
    b = np.unpackbits(np.ascontiguousarray(d, np.uint8), axis=1).astype(np.float32)
    ones = b.sum(1)
    return (ones[:, None] + ones[None, :] - 2.0 * (b @ b.T)).astype(np.int64)


def distinctive(desc, valid=None):
    """desc: (n, 32) uint8 in iteration order, valid: (n,) or None.  Returns (position within the n rows, median), (-1, -1) without a valid row."""
    desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    pos = np.arange(len(desc)) if valid is None else np.flatnonzero(np.asarray(valid) != 0)   # step 2
    N = len(pos)
    if N == 0:
        return -1, -1                                                                        # step 3
    D = hamming_matrix(desc[pos])                                                            # step 4
    med = np.sort(D, axis=1)[:, int(0.5 * (N - 1))]                                          # step 5
    best = int(np.argmin(med))                                                               # step 6
    return int(pos[best]), int(med[best])


def distinctive_all(obs_start, obs_desc, obs_valid=None):
    """every point of a CSR: (best_obs, best_median) arrays"""
    n = len(obs_start) - 1
    bo = np.full(n, -1, np.int32); bm = np.full(n, -1, np.int32)
    for p in range(n):
        s, e = int(obs_start[p]), int(obs_start[p + 1])
        bo[p], bm[p] = distinctive(obs_desc[s:e], None if obs_valid is None else obs_valid[s:e])
    return bo, bm


def apply(map_desc, obs_start, obs_desc, best_obs, point_id=None):
    """step 7 on a copy of map_desc"""
    out = map_desc.copy()
    for p, b in enumerate(best_obs):
        if b >= 0:
            out[p if point_id is None else point_id[p]] = obs_desc[int(obs_start[p]) + int(b)]
    return out


def load_fixture(path):
    import json
    cases = json.load(open(path))["cases"]
    for c in cases:
        d = np.zeros((len(c["obs"]), 32), np.uint8)
        for i, row in enumerate(c["obs"]):
            d[i, :len(row)] = row
        c["desc"] = d
        c["valid_arr"] = None if c["valid"] is None else np.array(c["valid"], np.uint8)
    return cases


def make_points(seed, counts, dup_share=0.3, max_flips=3, invalid_share=0.0):
    """observation sets with frequent median ties: per point a base word, every observation the base with a few flipped bits, a share of exact duplicates.
    Returns obs_start (int32), obs_desc (total, 32), obs_valid (total,) uint8."""
    rng = np.random.default_rng(seed)
    counts = np.asarray(counts, np.int64)
    start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    total = int(start[-1])
    base = rng.integers(0, 256, (len(counts), 32), dtype=np.uint8)
    desc = np.repeat(base, counts, axis=0)
    nflip = rng.integers(0, max_flips + 1, total)
    for f in range(max_flips):
        rows = np.flatnonzero(nflip > f)
        bit = rng.integers(0, 256, len(rows))
        desc[rows, bit >> 3] ^= (1 << (bit & 7)).astype(np.uint8)
    dup = np.flatnonzero(rng.random(total) < dup_share)
    owner = np.searchsorted(start, dup, side="right") - 1
    src = start[owner] + (rng.random(len(dup)) * counts[owner]).astype(np.int64)
    desc[dup] = desc[src]                                   # a copy of another observation of the same point (as it stands now)
    valid = (rng.random(total) >= invalid_share).astype(np.uint8)
    return start, desc, valid


def write_driver_input(d, start, desc, n_kf, seed, bad_share=0.2):
    """the files tests/cpp/mappoint_driver.cpp reads: every observation is dealt to a keyframe (a point sees a keyframe at most once; ascending keyframe
    index = the iteration order of the driver's std::map), a share of the keyframes isBad().  Returns (obs_kf, obs_idx, obs_valid)."""
    rng = np.random.default_rng(seed)
    total = len(desc)
    kf = np.zeros(total, np.int32); idx = np.zeros(total, np.int32)
    rows = [[] for _ in range(n_kf)]
    for p in range(len(start) - 1):
        s, e = int(start[p]), int(start[p + 1])
        assert e - s <= n_kf
        ks = np.sort(rng.choice(n_kf, e - s, replace=False))
        for o, k in zip(range(s, e), ks):
            kf[o] = k; idx[o] = len(rows[k]); rows[k].append(desc[o])
    np.asarray(start, np.int32).tofile(str(d / "obs_start.i32")); kf.tofile(str(d / "obs_kf.i32")); idx.tofile(str(d / "obs_idx.i32"))
    bad = (rng.random(n_kf) < bad_share).astype(np.uint8)
    bad.tofile(str(d / "kf_bad.u8"))
    for k in range(n_kf):
        (np.array(rows[k], np.uint8).reshape(-1, 32) if rows[k] else np.zeros((0, 32), np.uint8)).tofile(str(d / ("kf%d.u8" % k)))
    return kf, idx, (1 - bad[kf]).astype(np.uint8)

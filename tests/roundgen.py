"""Scenes for the round rule of the local-map search (test data only): the drop rule, the early finish and the LDS / pool paths of k_mp_rounds.

crowdgen's descriptors are 0-6 bits from their base code or about 128 from another one, so hardly a distance falls near TH_HIGH (100) or near the drop
boundary TH_HIGH / nnratio.  Here
  near_scene    crowdgen.crowded_map with base codes 55-90 bits from a common root: the distances between unlike codes spread over about 85-130;
  hand_scene    groups of key points 80 px apart whose distances are set bit by bit: a key point carries b bits of the lower descriptor half, a map point
                a bits of the upper half, their distance is a + b.  One group per case of the issue (see each builder).
lists_of() turns a scene into what k_mp_candidates caches: per map point the (key point, distance, octave) of its candidates in the reference order.
sequential() and rounds() are the reference loop and the round rule on such lists."""
import numpy as np

import crowdgen as G
import matchref as R
from kfgen import KP_DTYPE, scales

F = np.float32
TH_HIGH = R.TH_HIGH
TH = 3.0            # the th of every call on these scenes: radius 12 px * scale factor of the level
NNRATIOS = (0.6, 0.8, 0.9, 1.0, 0.0)


def dropped(d, nn):
    """the drop rule of k_mp_candidates, in float32 as the kernel evaluates it"""
    with np.errstate(invalid="ignore"):
        return bool(d > TH_HIGH and not (F(TH_HIGH) > F(F(nn) * F(d))))


def drop_boundary(nn):
    """(largest kept distance above TH_HIGH or None, smallest dropped distance or None)"""
    above = range(TH_HIGH + 1, 257)
    kept = [d for d in above if not dropped(d, nn)]
    gone = [d for d in above if dropped(d, nn)]
    return (max(kept) if kept else None, min(gone) if gone else None)


# ---------------------------------------------------------------- lists, the reference loop and the round rule on them
def lists_of(s, th, nn=None):
    """per map point its candidates [(key point, distance, octave)] after the window, level and uRight tests, in the reference order ([] when not in view).
    Availability is left to the loops below."""
    mp = s["mp"]
    _, _, st = R.search_by_projection_map(s["kps"], s["desc"], s["uright"], s["scale"], s["bounds"], mp, th, 0.8, s["init"])
    out = []
    for m, cand in enumerate(st["cands"]):
        if cand is None or len(cand) == 0:
            out.append([])
            continue
        r = F(2.5) if float(mp["view_cos"][m]) > 0.998 else F(4.0)
        if F(th) != F(1.0):
            r = F(r * F(th))
        rad = F(r * F(s["scale"][int(mp["level"][m])]))
        d = R.hamming(mp["desc"][m], s["desc"][cand])
        ur = s["uright"]
        out.append([(int(k), int(d[c]), int(s["kps"]["octave"][k])) for c, k in enumerate(cand)
                    if not (ur is not None and ur[k] > 0 and abs(F(mp["proj_xr"][m]) - F(ur[k])) > rad)])
    return out


def _top2(entries):
    best, lvl, best2, lvl2, idx, idx2 = 256, -1, 256, -1, -1, -1
    for k, d, o in entries:
        if d < best:
            best2, lvl2, idx2, best, lvl, idx = best, lvl, idx, d, o, k
        elif d < best2:
            best2, lvl2, idx2 = d, o, k
    return best, lvl, best2, lvl2, idx, idx2


def _accept(best, lvl, best2, lvl2, nn):
    with np.errstate(invalid="ignore"):
        return best <= TH_HIGH and not (lvl == lvl2 and F(best) > F(F(nn) * F(best2)))


def sequential(lists, init, obs, nn):
    """the reference loop on cached lists"""
    match = np.array(init, np.int32).copy()
    for m, L in enumerate(lists):
        best, lvl, best2, lvl2, idx, _ = _top2([e for e in L if R._free(match[e[0]], obs)])
        if idx >= 0 and _accept(best, lvl, best2, lvl2, nn):
            match[idx] = m
    return match


def rounds(lists, init, obs, nn, drop=True, restricted=False):
    """the round rule: every unfinished map point posts on its kept free entries; one that is the lowest poster on both of its two best is decided; one whose
    best free entry lies above TH_HIGH (or that has none) is final at once.  Returns (match, rounds, entries scanned).
    drop = False keeps every entry (the rule before the drop).  restricted = True is the UNSOUND variant that posts only on entries a map point could claim
    (distance <= TH_HIGH)."""
    match = np.array(init, np.int32).copy()
    kept = [[e for e in L if not (drop and dropped(e[1], nn))] for L in lists]
    unfinished = [m for m in range(len(lists)) if kept[m]]
    n_rounds = scanned = 0
    while unfinished:
        n_rounds += 1
        free = {m: [e for e in kept[m] if R._free(match[e[0]], obs)] for m in unfinished}
        owner = {}
        for m in unfinished:
            scanned += len(kept[m])
            for k, d, _ in free[m]:
                if not (restricted and d > TH_HIGH):
                    owner[k] = min(owner.get(k, m), m)
        left, claims = [], []
        for m in unfinished:
            best, lvl, best2, lvl2, idx, idx2 = _top2(free[m])
            if idx < 0 or best > TH_HIGH:
                continue
            if owner.get(idx, m) < m or (idx2 >= 0 and owner.get(idx2, m) < m):      # an earlier unfinished map point posted on one of the two
                left.append(m)
            elif _accept(best, lvl, best2, lvl2, nn):
                claims.append((idx, m))
        for k, m in claims:
            match[k] = m
        unfinished = left
    return match, n_rounds, scanned


def kept_entries(s, th, nn):
    """the figure k_mp_candidates adds up per frame: entries of key points free before the call that the drop rule keeps"""
    obs = s["mp"].get("obs_positive")
    return sum(1 for L in lists_of(s, th) for k, d, _ in L if R._free(s["init"][k], obs) and not dropped(d, nn))


# ---------------------------------------------------------------- random crowded scenes with distances around TH_HIGH
def _flip(rng, d, nbits):
    d = d.copy()
    for b in rng.choice(256, nbits, replace=False):
        d[b >> 3] ^= np.uint8(1 << (b & 7))
    return d


def near_scene(seed, n=None, m=None):
    rng = np.random.default_rng(1000 + seed)
    n = int(rng.integers(24, 64)) if n is None else n
    m = int(rng.integers(80, 240)) if m is None else m
    a = int(rng.integers(2, 6))
    s = G.crowded_map(seed, n, m, a, (1.0, 0.5, 0.0)[seed % 3], n_clusters=2)
    root = rng.integers(0, 256, 32, dtype=np.uint8)
    base = np.stack([_flip(rng, root, int(rng.integers(55, 91))) for _ in range(a)])
    s["desc"], _ = G.alphabet_desc(rng, base, n)
    s["mp"]["desc"], _ = G.alphabet_desc(rng, base, m)
    return s


# ---------------------------------------------------------------- hand-made groups
def _bits(nbits, upper):
    d = np.zeros(32, np.uint8)
    for i in range(nbits):
        d[(16 if upper else 0) + (i >> 3)] |= np.uint8(1 << (i & 7))
    return d


class _Hand:
    """key points (x, y, octave, b bits, entry before the call) and map points (x, y, a bits, observations) at level 1: octaves 0 and 1 are admissible, the
    radius is 12 * 1.2 = 14.4 px.  Groups lie 80 px apart, so no window reaches another group."""

    def __init__(self):
        self.k, self.i, self.g = [], [], 0

    def origin(self):
        self.g += 1
        return 60.0 + 80.0 * ((self.g - 1) % 7), 50.0 + 80.0 * ((self.g - 1) // 7)

    def kp(self, x, y, octave, b, init=-1):
        self.k.append((x, y, octave, b, init))
        return len(self.k) - 1

    def item(self, x, y, a, obs=1):
        self.i.append((x, y, a, obs))
        return len(self.i) - 1

    def scene(self):
        n, m = len(self.k), len(self.i)
        kps = np.zeros(n, KP_DTYPE)
        kps["x"] = [k[0] for k in self.k]; kps["y"] = [k[1] for k in self.k]; kps["octave"] = [k[2] for k in self.k]
        kps["size"] = 31; kps["response"] = 1; kps["class_id"] = -1
        desc = np.stack([_bits(k[3], False) for k in self.k])
        init = np.array([k[4] for k in self.k], np.int32)
        mp = dict(proj_x=np.array([i[0] for i in self.i], F), proj_y=np.array([i[1] for i in self.i], F), proj_xr=np.zeros(m, F), level=np.ones(m, np.int32),
                  view_cos=np.full(m, 0.95, F), in_view=np.ones(m, np.uint8), desc=np.stack([_bits(i[2], True) for i in self.i]),
                  obs_positive=np.array([i[3] for i in self.i], np.uint8))
        return dict(kps=kps, desc=desc, uright=None, scale=scales(), bounds=G.BOUNDS, mp=mp, init=init)


def _pair(h, best, second, same_octave, rival_first):
    """map point A (84 bits of its own) sees k0 at `best` and k1 at `second`; a rival without bits sees k1 only, at second - 84 <= TH_HIGH, and takes it.
    With the rival behind A it must not take k1 before A decides where k1 can reject A; with the rival ahead, A must see k1 gone."""
    x, y = h.origin()
    a = 84
    h.kp(x - 10, y, 1, best - a)
    h.kp(x + 10, y, 1 if same_octave else 0, second - a)
    if rival_first:
        h.item(x + 20, y, 0)
    h.item(x, y, a)
    if not rival_first:
        h.item(x + 20, y, 0)


def hand_scene(nn):
    """every hand-made case of the issue in one frame, for one nnratio (the boundary distances depend on it)"""
    h = _Hand()
    kept, gone = drop_boundary(nn)
    if kept is not None:
        kept = min(kept, 184)      # (nothing is dropped for nnratio <= 0: any large second-best then; a key point holds at most 128 bits)
    # best exactly at TH_HIGH and at TH_HIGH + 1, alone and with a second-best of the other octave
    for best in (TH_HIGH, TH_HIGH + 1):
        x, y = h.origin(); h.kp(x, y, 1, best - 20); h.item(x, y, 20)
        x, y = h.origin(); h.kp(x - 3, y, 1, best - 20); h.kp(x + 3, y, 0, best - 10); h.item(x, y, 20)
    # a second-best on either side of the drop boundary, equal and different octaves, best = TH_HIGH and a lower one, the rival before and behind
    for second in (kept, gone):
        if second is None:
            continue
        for best in (TH_HIGH, 84):
            for same in (True, False):
                for rival_first in (False, True):
                    _pair(h, best, second, same, rival_first)
    # a map point whose every entry is dropped (or, where nothing is dropped, above TH_HIGH), among map points that list the same key points
    x, y = h.origin()
    for j, b in enumerate((40, 44, 44, 52)):
        h.kp(x - 6 + 4 * j, y, j & 1, b)
    h.item(x, y, 10); h.item(x, y, 128); h.item(x, y, 10); h.item(x, y, 128, obs=0); h.item(x, y, 12)
    # best rises above TH_HIGH only after an earlier map point claims: both see k0 (50, octave 1) and k1 (101, octave 0)
    x, y = h.origin(); h.kp(x - 2, y, 1, 50); h.kp(x + 2, y, 0, 101); h.item(x, y, 0); h.item(x, y, 0); h.item(x, y, 0, obs=0)
    # equal distances in one list: the first occurrence is the best, the second one the second-best (same octave: rejected for nnratio < 1; other octave: taken)
    x, y = h.origin(); h.kp(x - 2, y, 1, 30); h.kp(x + 2, y, 1, 30); h.kp(x, y + 2, 1, 70); h.item(x, y, 5); h.item(x, y, 5)
    x, y = h.origin(); h.kp(x - 2, y, 1, 30); h.kp(x + 2, y, 0, 30); h.kp(x, y + 2, 0, 30); h.item(x, y, 5); h.item(x, y, 5); h.item(x, y, 5); h.item(x, y, 5)
    # map points without observations claim, later ones overwrite
    x, y = h.origin(); h.kp(x, y, 1, 20); h.kp(x + 3, y, 0, 60); h.item(x, y, 0, obs=0); h.item(x, y, 1, obs=0); h.item(x, y, 2, obs=1); h.item(x, y, 3, obs=1)
    # entries before the call: -2, -3, and live claims of a map point with (index 0) and without observations (the obs = 0 one of the group above)
    without = max(i for i, it in enumerate(h.i) if it[3] == 0)
    with_obs = min(i for i, it in enumerate(h.i) if it[3] == 1)
    x, y = h.origin()
    for j, (b, init) in enumerate(((10, -2), (20, -3), (30, with_obs), (40, without), (50, -1))):
        h.kp(x - 8 + 4 * j, y, 1 - (j & 1), b, init)
    for a in (0, 0, 4, 4, 8):
        h.item(x, y, a)
    # a window of more than 64 key points (two 64-rank chunks of the candidate walk) with kept entries in both, and several map points on it
    x, y = h.origin()
    rng = np.random.default_rng(7)
    for j in range(100):
        h.kp(x + float(rng.uniform(-9, 9)), y + float(rng.uniform(-9, 9)), int(rng.integers(0, 3)), int(rng.integers(40, 129)) if j % 3 else int(rng.integers(60, 90)))
    for a in (0, 5, 10, 15, 20, 25, 0, 5):
        h.item(x, y, a, obs=int(a != 15))
    return h.scene()

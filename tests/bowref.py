"""numpy restatement of the DBoW2 vocabulary transform and scores -- the checker of the GPU path (tests only; the product never imports it).
Every step cites the reference, Thirdparty/DBoW2/DBoW2/<file>:<line>.  Doubles are Python floats (IEEE binary64, one rounding per operation),
added in the reference's order."""
import math

import numpy as np

TF_IDF, TF, IDF, BINARY = 0, 1, 2, 3                                               # BowVector.h:38-44
L1_NORM, L2_NORM, CHI_SQUARE, KL, BHATTACHARYYA, DOT_PRODUCT = 0, 1, 2, 3, 4, 5    # BowVector.h:47-55

_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def distance(a, b):
    """FORB::distance, FORB.cpp:82-102: 256-bit popcount of the xor"""
    return _POP[np.bitwise_xor(a, b)].sum(axis=-1)


class Vocab:
    """k, L, scoring, weighting and the node arrays (node 0 = root; NodeIds = text file line numbers)"""

    def __init__(self, k, L, scoring, weighting, parent, desc, weight, is_leaf):
        self.k, self.L, self.scoring, self.weighting = int(k), int(L), int(scoring), int(weighting)
        self.parent = np.asarray(parent, np.int32); self.desc = np.asarray(desc, np.uint8).reshape(-1, 32)
        self.weight = np.asarray(weight, np.float64); self.is_leaf = np.asarray(is_leaf, np.uint8)
        n = len(self.parent)
        # children in the order they were appended = ascending NodeId (TemplatedVocabulary.h:1416)
        ids = np.arange(1, n)
        order = ids[np.argsort(self.parent[1:], kind="stable")]
        self.child_list = order.astype(np.int64)
        cnt = np.bincount(self.parent[1:], minlength=n)
        self.child_start = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
        self.n_children = cnt
        # WordIds count the leaves in file order (:1432-1439)
        self.word_of = np.full(n, -1, np.int64)
        leaves = np.flatnonzero(self.is_leaf[1:] > 0) + 1
        self.word_of[leaves] = np.arange(len(leaves))
        self.n_words = len(leaves)
        depth = np.zeros(n, np.int32)
        while n > 1:                                          # parents precede children: settles after (tree depth) passes
            nd = depth[self.parent[1:]] + 1
            if np.array_equal(nd, depth[1:]): break
            depth[1:] = nd
        self.depth = depth
        self.min_leaf_depth = int(depth[leaves].min()) if len(leaves) else 0

    def n_nodes(self):
        return len(self.parent)


def descend(voc, desc, levelsup):
    """TemplatedVocabulary::transform(feature, word_id, weight, nid, levelsup), :1242-1283, for all rows of desc at once.
    Returns word (int64), weight (float64), nid (int64; -1 = the reference leaves it uninitialised: a leaf above level L - levelsup)."""
    desc = np.asarray(desc, np.uint8).reshape(-1, 32)
    N = len(desc)
    nid_level = voc.L - levelsup                              # :1250
    nid = np.full(N, 0 if nid_level <= 0 else -1, np.int64)   # :1251
    cur = np.zeros(N, np.int64)                               # :1253 root
    active = np.arange(N)
    level = 0
    kmax = int(voc.n_children.max())
    while len(active):
        level += 1                                            # :1258
        c = cur[active]
        start = voc.child_start[c]; cnt = voc.n_children[c]
        slot = np.arange(kmax)[None, :]
        valid = slot < cnt[:, None]
        kids = voc.child_list[np.minimum(start[:, None] + slot, len(voc.child_list) - 1)]
        d = np.empty(kids.shape, np.int32)
        for lo in range(0, len(active), 65536):               # bounded temporaries
            hi = lo + 65536
            d[lo:hi] = distance(desc[active[lo:hi], None, :], voc.desc[kids[lo:hi]])
        d[~valid] = 1 << 20
        best = np.argmin(d, axis=1)                           # first minimum = `d < best_d`, ties to the earliest child (:1262-1273)
        chosen = kids[np.arange(len(active)), best]
        cur[active] = chosen
        if level == nid_level:                                # :1275
            nid[active] = chosen
        active = active[voc.is_leaf[chosen] == 0]             # :1278
    return voc.word_of[cur], voc.weight[cur], nid             # :1281-1282


def must_normalize(scoring):
    """ScoringObject.h:76-91: 0 = none, 1 = L1, 2 = L2"""
    return {L1_NORM: 1, L2_NORM: 2, CHI_SQUARE: 1, KL: 1, BHATTACHARYYA: 1, DOT_PRODUCT: 0}[scoring]


def transform(voc, desc, levelsup):
    """TemplatedVocabulary::transform(features, BowVector&, FeatureVector&, levelsup), :1151-1218.
    Returns (bow, fv): bow = [(word, value)] ascending, fv = [(node, [features])] ascending (the std::map orders)."""
    word, weight, nid = descend(voc, desc, levelsup)
    v, fv = {}, {}
    norm = must_normalize(voc.scoring)                        # :1164-1165
    tf = voc.weighting in (TF, TF_IDF)
    for i in range(len(word)):
        w = float(weight[i])
        if w > 0:                                             # :1181 / :1209 not stopped
            wid = int(word[i])
            if tf:
                if wid in v: v[wid] += w                      # BowVector::addWeight, BowVector.cpp:34-46
                else: v[wid] = w
            elif wid not in v:
                v[wid] = w                                    # BowVector::addIfNotExist, BowVector.cpp:50-58
            assert nid[i] >= 0, "leaf above level L - levelsup: NodeId uninitialised in the reference"
            fv.setdefault(int(nid[i]), []).append(i)          # FeatureVector::addFeature, FeatureVector.cpp:31-45
    keys = sorted(v)
    if tf and v and not norm:                                 # :1188-1194
        nd = float(len(v))
        for kk in keys: v[kk] /= nd
    if norm:                                                  # BowVector::normalize, BowVector.cpp:62-84
        s = 0.0
        if norm == 1:
            for kk in keys: s += abs(v[kk])
        else:
            for kk in keys: s += v[kk] * v[kk]
            s = math.sqrt(s)
        if s > 0.0:
            for kk in keys: v[kk] /= s
    return [(kk, v[kk]) for kk in keys], [(kk, fv[kk]) for kk in sorted(fv)]


def score(scoring, v1, v2):
    """ScoringObject.cpp:23-68 (L1), :73-120 (L2), :271-311 (dot product); v1, v2 = [(word, value)] ascending.
    The reference's lower_bound jumps skip words the other vector lacks: only common words contribute, in ascending order."""
    d2 = dict(v2)
    s = 0.0
    for wid, vi in v1:
        if wid in d2:
            wi = d2[wid]
            if scoring == L1_NORM: s += abs(vi - wi) - abs(vi) - abs(wi)   # :41
            elif scoring in (L2_NORM, DOT_PRODUCT): s += vi * wi           # :91, :290
            else: raise ValueError("scoring type out of scope")
    if scoring == L1_NORM: return -s / 2.0                                 # :65
    if scoring == L2_NORM: return 1.0 if s >= 1 else 1.0 - math.sqrt(1.0 - s)   # :114-117
    return s


def flatten(bow, fv, capacity):
    """the arrays plf_bow_transform_batch writes for one frame"""
    word_id = np.zeros(capacity, np.uint32); word_val = np.zeros(capacity, np.float64)
    node_id = np.zeros(capacity, np.uint32); node_start = np.zeros(capacity + 1, np.int32); feat = np.zeros(capacity, np.int32)
    for j, (w, val) in enumerate(bow): word_id[j] = w; word_val[j] = val
    p = 0
    for j, (nd, fs) in enumerate(fv):
        node_id[j] = nd; node_start[j] = p
        feat[p:p + len(fs)] = fs; p += len(fs)
    node_start[len(fv)] = p
    return {"word_id": word_id, "word_val": word_val, "n_words": len(bow), "node_id": node_id, "node_start": node_start, "feat": feat, "n_nodes": len(fv)}


# ---- text files (loadFromTextFile, :1362-1448; blank lines skipped -- the documented deviation)
def save_text(voc, path, trailing_blank_lines=0, blank_inside=False):
    with open(path, "w") as f:
        f.write("%d %d %d %d\n" % (voc.k, voc.L, voc.scoring, voc.weighting))
        for i in range(1, voc.n_nodes()):
            if blank_inside and i == 2: f.write("\n")
            f.write("%d %d %s %r\n" % (voc.parent[i], int(voc.is_leaf[i] > 0), " ".join(str(int(b)) for b in voc.desc[i]), float(voc.weight[i])))
        f.write("\n" * trailing_blank_lines)


def parse_text(path):
    with open(path) as f:
        lines = f.read().split("\n")
    k, L, n1, n2 = (int(t) for t in lines[0].split()[:4])
    if k < 0 or k > 20 or L < 1 or L > 10 or n1 < 0 or n1 > 5 or n2 < 0 or n2 > 3:   # :1383
        raise ValueError("not a correct text file")
    parent, desc, weight, leaf = [0], [[0] * 32], [0.0], [0]
    for ln in lines[1:]:
        t = ln.split()
        if not t: continue
        parent.append(int(t[0])); leaf.append(int(int(t[1]) > 0)); desc.append([int(x) & 255 for x in t[2:34]]); weight.append(float(t[34]))
    return Vocab(k, L, n1, n2, parent, desc, weight, leaf)


# ---- seeded generator
def make_vocab(seed, k, L, weighting=TF_IDF, scoring=L1_NORM, zero_share=0.0, shallow_share=0.0, dup_share=0.0, uneven=False, full=None):
    """A level-ordered random tree: inner nodes have k children (1 .. k with `uneven`), a node above level L becomes a leaf with probability
    shallow_share, a non-first child copies its first sibling's descriptor with probability dup_share (ties), a leaf has weight 0 with
    probability zero_share; with `full` only that many randomly chosen inner nodes of a level branch k ways, the others have a
    single child (a deep tree of bounded size whose leaves all lie at level L).  TF / BINARY vocabularies carry weight 1 (TemplatedVocabulary.h:1496-1520 setNodeWeights), the others an idf-like double."""
    rng = np.random.default_rng(seed)
    parent = [np.zeros(1, np.int64)]; desc = [np.zeros((1, 32), np.uint8)]; leaf = [np.zeros(1, np.uint8)]
    inner = np.zeros(1, np.int64); n = 1
    for level in range(1, L + 1):
        cnt = rng.integers(1, k + 1, len(inner)) if uneven else np.full(len(inner), k)
        if full is not None and len(inner) > full:
            cnt[:] = 1; cnt[rng.choice(len(inner), full, replace=False)] = k
        par = np.repeat(inner, cnt)
        m = len(par)
        d = rng.integers(0, 256, (m, 32), dtype=np.uint8)
        first = np.repeat(np.cumsum(cnt) - cnt, cnt)
        dup = (rng.uniform(0, 1, m) < dup_share) & (np.arange(m) != first)
        d[dup] = d[first[dup]]
        lf = np.ones(m, np.uint8) if level == L else (rng.uniform(0, 1, m) < shallow_share).astype(np.uint8)
        ids = n + np.arange(m)
        parent.append(par); desc.append(d); leaf.append(lf)
        inner = ids[lf == 0]; n += m
        if len(inner) == 0: break
    parent = np.concatenate(parent); desc = np.concatenate(desc); leaf = np.concatenate(leaf)
    if weighting in (TF, BINARY): w = np.ones(n)
    else: w = np.log(rng.uniform(1.5, 500.0, n))
    w[rng.uniform(0, 1, n) < zero_share] = 0.0
    w[leaf == 0] = 0.0
    return Vocab(k, L, scoring, weighting, parent, desc, w, leaf)


def make_descriptors(voc, seed, n, noise_bits=20):
    """descriptors near random leaves (so the descent is not a coin toss at every level), n x 32 uint8"""
    rng = np.random.default_rng(seed)
    leaves = np.flatnonzero(voc.is_leaf > 0)
    d = voc.desc[rng.choice(leaves, n)].copy()
    bits = rng.integers(0, 256, (n, noise_bits))
    for j in range(noise_bits):
        d[np.arange(n), bits[:, j] >> 3] ^= (1 << (bits[:, j] & 7)).astype(np.uint8)
    return d

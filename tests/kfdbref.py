"""Pure-Python / numpy restatement of ORB_SLAM2::KeyFrameDatabase -- the checker of the GPU path (tests only; the product never imports it).
The class has no source in the reference; the rule is the one include/plf.h states from the binary (addresses so@... there).  Plain lists
per word, per-keyframe fields named after the reference's, float steps in np.float32, scores from bowref.score."""
import numpy as np

import bowref

F32 = np.float32


class KeyFrame:
    """the fields of ORB_SLAM2::KeyFrame the database touches.  bow = [(word, value)] ascending; best_covis = the keyframe's
    mvpOrderedConnectedKeyFrames as a list of KeyFrame objects (or None for one outside the database)."""

    def __init__(self, slot, bow):
        self.slot = slot
        self.mBowVec = list(bow)
        self.mnLoopQuery = self.mnRelocQuery = -1      # never equal to a query stamp (plf.h: the id-0 coincidence is not reproduced)
        self.mnLoopWords = self.mnRelocWords = 0
        self.mLoopScore = F32(0.0)
        self.mRelocScore = F32(0.0)                   # DEVIATION stated in plf.h: indeterminate in the reference, 0.0f here
        self.best_covis = []
        self.in_db = False


class Database:
    def __init__(self, scoring, n_words, n_best=10):
        self.scoring, self.n_best = scoring, n_best
        self.mvInvertedFile = [[] for _ in range(n_words)]
        self.stamp = 0                                # a fresh query id per call
        self.trace = None                             # the lists of the last query, for the fixture and for failing tests
        self.stale_reads = 0                          # neighbours that contributed a score an earlier query left (relocalisation)

    # void add(KeyFrame*)
    def add(self, kf):
        for w, _ in kf.mBowVec:
            self.mvInvertedFile[w].append(kf)
        kf.in_db = True
        kf.mRelocScore = F32(0.0)

    # void erase(KeyFrame*): the keyframe leaves every list, the others keep their order
    def erase(self, kf):
        for w, _ in kf.mBowVec:
            lst = self.mvInvertedFile[w]
            if kf in lst:
                lst.remove(kf)
        kf.in_db = False

    def clear(self):
        for lst in self.mvInvertedFile:
            for kf in lst:
                kf.in_db = False
            del lst[:]

    def n_entries(self):
        return sum(len(l) for l in self.mvInvertedFile)

    def _groups(self, lScoreAndMatch, counts):
        """steps 4 and 5; counts(kf) says whether a neighbour contributes and returns its score"""
        lAccScoreAndMatch, bestAccScore = [], F32(0.0)
        for si, pKFi in lScoreAndMatch:
            bestScore = accScore = si
            pBestKF = pKFi
            for pKF2 in pKFi.best_covis[:self.n_best]:
                if pKF2 is None or not pKF2.in_db:
                    continue
                s2 = counts(pKF2)
                if s2 is None:
                    continue
                accScore = F32(accScore + s2)
                if s2 > bestScore:
                    pBestKF, bestScore = pKF2, s2
            lAccScoreAndMatch.append((accScore, pBestKF))
            if accScore > bestAccScore:
                bestAccScore = accScore
        minScoreToRetain = F32(F32(0.75) * bestAccScore)
        out, spAlreadyAddedKF = [], set()
        for acc, kf in lAccScoreAndMatch:
            if acc > minScoreToRetain and id(kf) not in spAlreadyAddedKF:
                out.append(kf)
                spAlreadyAddedKF.add(id(kf))
        self.trace.update(lAccScoreAndMatch=[(float(a), k.slot) for a, k in lAccScoreAndMatch], bestAccScore=bestAccScore,
                          minScoreToRetain=float(minScoreToRetain))
        return out

    def _empty(self, n_sharing=0, max_common=0, n_scored=0):
        self.trace.update(n_sharing=n_sharing, maxCommonWords=max_common, n_scored=n_scored, bestAccScore=F32(0.0))
        return []

    # std::vector<KeyFrame*> DetectRelocalizationCandidates(Frame*)
    def DetectRelocalizationCandidates(self, bow):
        self.stamp += 1
        mnId = self.stamp
        self.trace = {}
        lKFsSharingWords = []
        for w, _ in bow:
            for pKFi in self.mvInvertedFile[w]:
                if pKFi.mnRelocQuery != mnId:
                    pKFi.mnRelocWords = 0
                    pKFi.mnRelocQuery = mnId
                    lKFsSharingWords.append(pKFi)
                pKFi.mnRelocWords += 1
        self.trace["lKFsSharingWords"] = [(k.slot, k.mnRelocWords) for k in lKFsSharingWords]
        if not lKFsSharingWords:
            return self._empty()
        maxCommonWords = max(k.mnRelocWords for k in lKFsSharingWords)
        minCommonWords = int(F32(F32(maxCommonWords) * F32(0.8)))
        lScoreAndMatch = []
        scored_now = set()
        for pKFi in lKFsSharingWords:
            if pKFi.mnRelocWords > minCommonWords:
                si = F32(bowref.score(self.scoring, bow, pKFi.mBowVec))
                pKFi.mRelocScore = si
                lScoreAndMatch.append((si, pKFi))
                scored_now.add(id(pKFi))
        self.trace.update(n_sharing=len(lKFsSharingWords), maxCommonWords=maxCommonWords, minCommonWords=minCommonWords, n_scored=len(lScoreAndMatch),
                          lScoreAndMatch=[(float(s), k.slot) for s, k in lScoreAndMatch])

        def counts(pKF2):
            if pKF2.mnRelocQuery != mnId:
                return None
            if id(pKF2) not in scored_now:
                self.stale_reads += 1
            return pKF2.mRelocScore
        return self._groups(lScoreAndMatch, counts)

    # std::vector<KeyFrame*> DetectLoopCandidates(KeyFrame*, float minScore); connected = pKF->GetConnectedKeyFrames() (+ pKF itself if it is in the database)
    def DetectLoopCandidates(self, bow, minScore, connected=()):
        self.stamp += 1
        mnId = self.stamp
        self.trace = {}
        minScore = F32(minScore)
        spConnected = set(id(k) for k in connected)
        lKFsSharingWords = []
        for w, _ in bow:
            for pKFi in self.mvInvertedFile[w]:
                if pKFi.mnLoopQuery != mnId:
                    pKFi.mnLoopWords = 0
                    if id(pKFi) not in spConnected:
                        pKFi.mnLoopQuery = mnId
                        lKFsSharingWords.append(pKFi)
                pKFi.mnLoopWords += 1
        self.trace["lKFsSharingWords"] = [(k.slot, k.mnLoopWords) for k in lKFsSharingWords]
        if not lKFsSharingWords:
            return self._empty()
        maxCommonWords = max(k.mnLoopWords for k in lKFsSharingWords)
        minCommonWords = int(F32(F32(maxCommonWords) * F32(0.8)))
        lScoreAndMatch, n_scored = [], 0
        for pKFi in lKFsSharingWords:
            if pKFi.mnLoopWords > minCommonWords:
                si = F32(bowref.score(self.scoring, bow, pKFi.mBowVec))
                pKFi.mLoopScore = si
                n_scored += 1
                if si >= minScore:
                    lScoreAndMatch.append((si, pKFi))
        self.trace.update(n_sharing=len(lKFsSharingWords), maxCommonWords=maxCommonWords, minCommonWords=minCommonWords, n_scored=n_scored,
                          lScoreAndMatch=[(float(s), k.slot) for s, k in lScoreAndMatch])
        if not lScoreAndMatch:
            return self._empty(len(lKFsSharingWords), maxCommonWords, n_scored)

        def counts(pKF2):
            if pKF2.mnLoopQuery == mnId and pKF2.mnLoopWords > minCommonWords:
                return pKF2.mLoopScore
            return None
        return self._groups(lScoreAndMatch, counts)

    def stats(self):
        """the plf_kfdb_stats of the last query"""
        t = self.trace
        return (t["n_sharing"], t["maxCommonWords"], t["n_scored"], int(np.float32(t["bestAccScore"]).view(np.uint32)))


def truncation_differs(x):
    """(int)(x * 0.8f) in float against (int)(x * 0.8) in double"""
    return int(F32(F32(x) * F32(0.8))) != int(x * 0.8)


class SlotModel:
    """the database behind the slot interface of plf_kfdb_*: bows are [(word, value)] lists, covisibility a list of rows of slots (-1 or a
    slot without a keyframe = a keyframe outside the database), results (candidate slots, stats) per query"""

    def __init__(self, scoring, n_words, max_keyframes, n_best=10):
        self.db = Database(scoring, n_words, n_best)
        self.kf = [None] * max_keyframes

    def add(self, bows, slots):
        for bow, s in zip(bows, slots):
            assert self.kf[s] is None
            self.kf[s] = KeyFrame(s, bow)
            self.db.add(self.kf[s])

    def erase(self, slots):
        for s in slots:
            if self.kf[s] is not None:
                self.db.erase(self.kf[s])
                self.kf[s] = None

    def clear(self):
        self.db.clear()
        self.kf = [None] * len(self.kf)

    def n_keyframes(self):
        return sum(k is not None for k in self.kf)

    def _covis(self, covis):
        for s, k in enumerate(self.kf):
            if k is not None:
                row = covis[s] if covis is not None and s < len(covis) else []
                k.best_covis = [self.kf[n] if 0 <= n < len(self.kf) else None for n in row]

    def detect_reloc(self, queries, covis=None):
        self._covis(covis)
        out = []
        for bow in queries:
            c = self.db.DetectRelocalizationCandidates(bow)
            out.append(([k.slot for k in c], self.db.stats()))
        return out

    def detect_loop(self, queries, min_scores, covis=None, connected=None):
        self._covis(covis)
        out = []
        for q, bow in enumerate(queries):
            conn = [self.kf[s] for s in (connected[q] if connected is not None else []) if 0 <= s < len(self.kf) and self.kf[s] is not None]
            c = self.db.DetectLoopCandidates(bow, min_scores[q], conn)
            out.append(([k.slot for k in c], self.db.stats()))
        return out


def random_bows(seed, n, n_words, lo, hi, pool=None):
    """n ascending BoW vectors of lo .. hi distinct words (drawn from `pool` when given), L1-normalised doubles"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        m = int(rng.integers(lo, hi + 1))
        src = np.arange(n_words) if pool is None else np.asarray(pool)
        w = np.sort(rng.choice(src, min(m, len(src)), replace=False))
        v = rng.uniform(0.1, 1.0, len(w))
        v = v / v.sum()
        out.append([(int(a), float(b)) for a, b in zip(w, v)])
    return out


def driver_scenario(seed, n_words, path):
    """a command file for tests/cpp/kfdb_driver.cpp (its header explains the format) and the lines of keyframe ids it has to answer with"""
    rng = np.random.default_rng(seed)
    n = 40
    bows = random_bows(seed, n, n_words, 3, 14, pool=np.arange(0, 30))
    bows[7] = list(bows[6])
    db = Database(bowref.L1_NORM, n_words)
    kfs = [KeyFrame(i, b) for i, b in enumerate(bows)]
    lines, expect = [], []
    fmt = lambda b: "%d %s" % (len(b), " ".join("%d %s" % (w, float(v).hex()) for w, v in b))
    for k in kfs:
        lines.append("kf %d %s" % (k.slot, fmt(k.mBowVec)))
    for k in kfs:
        k.best_covis = [kfs[j] for j in rng.integers(0, n, int(rng.integers(0, 14)))]
        lines.append("covis %d %d %s" % (k.slot, len(k.best_covis), " ".join(str(c.slot) for c in k.best_covis)))

    def add(i): lines.append("add %d" % i); db.add(kfs[i])
    def erase(i): lines.append("erase %d" % i); db.erase(kfs[i])

    def reloc(b):
        lines.append("reloc " + fmt(b))
        expect.append(" ".join(str(k.slot) for k in db.DetectRelocalizationCandidates(b)))

    def loop(i, ms):
        ms = float(np.float32(ms))
        lines.append("loop %d %s" % (i, ms.hex()))
        conn = [c for c in kfs[i].best_covis if c.in_db] + ([kfs[i]] if kfs[i].in_db else [])
        expect.append(" ".join(str(k.slot) for k in db.DetectLoopCandidates(kfs[i].mBowVec, ms, conn)))
    for i in rng.permutation(n)[:32]: add(int(i))
    queries = random_bows(seed + 1, 8, n_words, 3, 14, pool=np.arange(0, 30)) + [list(bows[6])]
    for q in queries: reloc(q)
    gone = [k.slot for k in kfs if k.in_db][2:6]
    for i in gone: erase(i)
    add(gone[0])
    for q in queries[:4]: reloc(q)
    for i in range(0, n, 3): loop(i, 0.0)
    for i in range(1, n, 5): loop(i, 0.05)
    lines.append("clear"); db.clear()
    reloc(queries[0])
    add(3); add(1)
    reloc(list(bows[3]))
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    assert sum(bool(e) for e in expect) > len(expect) // 3 and db.stale_reads > 0
    return expect

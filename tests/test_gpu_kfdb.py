"""KeyFrameDatabase on the GPU (plf_kfdb_*) against the restatement tests/kfdbref.py: candidates, counts and stats element for element,
bestAccScore through its bits.  Small vocabularies and at most a few hundred keyframes: every case is the smallest at which its stage
can go wrong (wave and workgroup edges of the slot loops, one long inverted list next to short ones, ties, erased slots)."""
import json
import os

import numpy as np
import pytest

import bowref
import kfdbref
from conftest import gpu_available
from kfdbref import random_bows

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NW, CAP = 120, 16          # words of the synthetic vocabularies (word NW - 1 is in no keyframe), capacity of the vectors


@pytest.fixture(autouse=True)
def _need_gpu():
    if not gpu_available():
        pytest.fail("no GPU visible: the -m gpu tests need a real MI355X")


_VOCS = {}


def _voc(scoring, n_words=NW):
    """a device vocabulary of exactly n_words words with the given scoring type: a root with its leaves in chunks of at most 32 under inner nodes"""
    from rgbd_pl_slam_amd import Vocabulary
    if (scoring, n_words) not in _VOCS:
        groups = [min(32, n_words - g) for g in range(0, n_words, 32)]
        parent = [0] + [0] * len(groups)
        leaf = [0] + [0] * len(groups)
        for g, cnt in enumerate(groups):
            parent += [1 + g] * cnt
            leaf += [1] * cnt
        n = len(parent)
        desc = np.random.default_rng(1).integers(0, 256, (n, 32), dtype=np.uint8)
        _VOCS[(scoring, n_words)] = Vocabulary.from_arrays(32, 2, scoring, bowref.TF_IDF, parent, desc, np.array(leaf, np.float64), leaf)
        assert _VOCS[(scoring, n_words)].n_words == n_words
    return _VOCS[(scoring, n_words)]


def _pack(bows, cap):
    """the dict Vocabulary.transform returns, on the device; filler beyond n_words must not be read"""
    import torch
    wid = np.full((len(bows), cap), 7, np.uint32); val = np.full((len(bows), cap), np.nan)
    for f, b in enumerate(bows):
        wid[f, :len(b)] = [w for w, _ in b]; val[f, :len(b)] = [v for _, v in b]
    n = np.array([len(b) for b in bows], np.int32)
    return {"word_id": torch.from_numpy(wid.view(np.int32)).cuda(), "word_val": torch.from_numpy(val).cuda(), "n_words": torch.from_numpy(n).cuda()}


def _csr(rows):
    import torch
    start = np.zeros(len(rows) + 1, np.int32)
    start[1:] = np.cumsum([len(r) for r in rows])
    flat = np.array([x for r in rows for x in r] + [0], np.int32)
    return torch.from_numpy(start).cuda(), torch.from_numpy(flat).cuda()


def _results(out, max_cand):
    import torch
    torch.cuda.synchronize()
    cand, n, stats = (t.cpu().numpy() for t in out)
    return [(cand[q, :min(int(n[q]), max_cand)].tolist(), int(n[q]), tuple(int(x) for x in stats[q].view(np.uint32))) for q in range(len(n))]


def _expect(ref, max_cand):
    return [(c[:max_cand], len(c), tuple(int(np.uint32(x)) for x in s)) for c, s in ref]


def _reloc(db, model, queries, covis, cap=CAP, max_cand=64):
    got = _results(db.detect_relocalization_candidates(_pack(queries, cap), _csr(covis) if covis is not None else None, max_cand), max_cand)
    exp = _expect(model.detect_reloc(queries, covis), max_cand)
    for q, (g, e) in enumerate(zip(got, exp)):
        assert g == e, ("query", q, "got (cand, n, stats)", g, "expected", e, model.db.trace if q == len(exp) - 1 else None)
    return got


def _loop(db, model, queries, min_scores, covis, conn, cap=CAP, max_cand=64):
    import torch
    ms = torch.from_numpy(np.array(min_scores, np.float32)).cuda()
    got = _results(db.detect_loop_candidates(_pack(queries, cap), ms, _csr(covis) if covis is not None else None,
                                             _csr(conn) if conn is not None else None, max_cand), max_cand)
    exp = _expect(model.detect_loop(queries, min_scores, covis, conn), max_cand)
    for q, (g, e) in enumerate(zip(got, exp)):
        assert g == e, ("query", q, "got (cand, n, stats)", g, "expected", e)
    return got


def _pair(scoring, S, n_words=NW, cap=CAP):
    from rgbd_pl_slam_amd import KeyFrameDatabase
    return KeyFrameDatabase(_voc(scoring, n_words), S, cap), kfdbref.SlotModel(scoring, n_words, S)


def _world(seed, n_kf, S):
    """keyframes: word 0 in every one (one list of n_kf entries next to short ones), keyframe 1 with a single word, keyframe 2 with CAP words,
    every fifth a copy of its predecessor; covisibility rows of 0, 3, 10 and 25 entries holding -1 and slots that hold no keyframe"""
    rng = np.random.default_rng(seed)
    bows = random_bows(seed, n_kf, NW, 2, CAP - 1, pool=np.arange(1, NW - 1))
    for i, b in enumerate(bows):
        b = [(0, 0.05)] + b[:CAP - 1]
        if i == 1: b = [(0, 1.0)]
        if i == 2: b = [(w, 1.0 / CAP) for w in range(CAP)]
        if i % 5 == 4: b = list(bows[i - 1])
        bows[i] = b
    covis = [list(rng.integers(-1, S, (0, 3, 10, 25)[s % 4])) for s in range(S)]
    queries = random_bows(seed + 7, 12, NW, 1, CAP, pool=np.arange(0, NW - 1))
    queries += [list(bows[min(4, n_kf - 1)]), list(bows[0]), [(NW - 1, 1.0)], [(0, 1.0)], list(bows[min(2, n_kf - 1)])]
    return bows, covis, queries


def test_the_hand_worked_fixture_and_an_empty_database():
    fx = json.load(open(os.path.join(GOLD, "kfdb_tiny.json")))
    db, model = _pair(fx["scoring"], 6, fx["n_words"], 8)
    queries = [[(int(w), float(v)) for w, v in q["bow"]] for q in fx["queries"]]
    empty = _results(db.detect_relocalization_candidates(_pack(queries, 8), _csr(fx["covis"]), 4), 4)
    assert empty == [([], 0, (0, 0, 0, 0))] * 3
    assert db.info()["n_keyframes"] == 0 and db.info()["n_entries"] == 0
    bows = [[(int(w), float(v)) for w, v in k["bow"]] for k in fx["keyframes"]]
    db.add(_pack(bows, 8), range(6)); model.add(bows, range(6))
    assert db.info() == {"max_keyframes": 6, "capacity": 8, "n_keyframes": 6, "n_entries": model.db.n_entries(), "n_best": 10}
    got = _reloc(db, model, queries, fx["covis"], cap=8)          # one call of three queries: the tie, the de-duplication, the stale score
    assert [g[0] for g in got] == [q["candidates"] for q in fx["queries"]]
    assert [g[2][3] for g in got] == [int(np.float32(q["bestAccScore"]).view(np.uint32)) for q in fx["queries"]]


@pytest.mark.parametrize("scoring", [bowref.L1_NORM, bowref.L2_NORM, bowref.DOT_PRODUCT])
@pytest.mark.parametrize("n_kf", [1, 63, 64, 65, 300])
def test_relocalisation_and_loop_equal_the_restatement(n_kf, scoring):
    S = n_kf + 6
    bows, covis, queries = _world(n_kf, n_kf, S)
    db, model = _pair(scoring, S)
    slots = list(np.random.default_rng(n_kf).permutation(S)[:n_kf])          # slot order is not add order
    db.add(_pack(bows, CAP), slots); model.add(bows, slots)
    assert db.info()["n_entries"] == model.db.n_entries()
    _reloc(db, model, queries, covis)
    if n_kf > 10:                                                            # erase, and re-add into the same slot: last in its lists now
        gone = slots[3:8]
        db.erase(gone); model.erase(gone)
        db.add(_pack([bows[0]], CAP), [gone[0]]); model.add([bows[0]], [gone[0]])
        assert db.info()["n_keyframes"] == model.n_keyframes() == n_kf - 4
        _reloc(db, model, queries, covis)
    # loop: connected sets of 0 .. 5 slots; minScore 0, and a score that occurs (>=)
    conn = [list(np.random.default_rng(q).integers(0, S, q % 6)) for q in range(len(queries))]
    probe = kfdbref.SlotModel(scoring, NW, S)
    probe.add([k.mBowVec for k in model.kf if k is not None], [k.slot for k in model.kf if k is not None])
    mins, hit = [], 0
    for q, bow in enumerate(queries):
        probe.detect_loop([bow], [0.0], covis, [conn[q]])
        sm = probe.db.trace.get("lScoreAndMatch", [])
        mins.append(sorted(s for s, _ in sm)[len(sm) // 2] if sm else 0.5)
        hit += bool(sm)
    assert hit
    _reloc(db, model, queries[:3], covis)
    _loop(db, model, queries, [0.0] * len(queries), covis, conn)
    got = _loop(db, model, queries, mins, covis, conn)
    assert any(g[1] for g in got)
    _loop(db, model, queries, mins, covis, [list(range(S))] * len(queries))  # every sharer excluded
    _reloc(db, model, queries, covis)                                        # the loop calls left the relocalisation state alone


def test_identical_keyframes_keep_the_earlier_and_max_cand_cuts_the_output():
    S = 70
    db, model = _pair(bowref.L1_NORM, S)
    bow = [(3, 0.25), (5, 0.25), (9, 0.5)]
    bows = [list(bow) for _ in range(66)]
    db.add(_pack(bows, CAP), range(66)); model.add(bows, range(66))
    covis = [[(s + 1) % 66, (s + 2) % 66] for s in range(66)] + [[]] * 4
    got = _reloc(db, model, [bow], covis, max_cand=64)                       # equal scores: the strict > keeps pKFi itself
    assert got[0][1] == 66 and got[0][0] == list(range(64))                  # true count beyond max_cand, only max_cand written
    got = _reloc(db, model, [bow], None, max_cand=1)
    assert got[0][:2] == ([0], 66)
    db.set_n_best(1); model.db.n_best = 1
    _reloc(db, model, [bow, bow[:2]], covis)
    db.clear(); model.clear()
    assert db.info()["n_keyframes"] == 0 and db.info()["n_entries"] == 0
    assert _reloc(db, model, [bow], covis)[0][:2] == ([], 0)
    db.add(_pack(bows[:2], CAP), [5, 1]); model.add(bows[:2], [5, 1])
    assert _reloc(db, model, [bow], None)[0][0] == [5, 1]                    # add order, not slot order


def test_one_call_of_70_queries_equals_70_calls_with_the_stale_score():
    n_kf, S = 90, 96
    bows, covis, _ = _world(11, n_kf, S)
    queries = random_bows(5, 70, NW, 3, CAP, pool=np.arange(0, 40))
    a, ma = _pair(bowref.L1_NORM, S)
    b, mb = _pair(bowref.L1_NORM, S)
    for d, m in ((a, ma), (b, mb)):
        d.add(_pack(bows, CAP), range(n_kf)); m.add(bows, range(n_kf))
    one = _reloc(a, ma, queries, covis)
    assert ma.db.stale_reads > 0                                             # a neighbour really contributed an earlier query's score
    many = [_reloc(b, mb, [q], covis)[0] for q in queries]
    assert one == many
    assert _reloc(a, ma, queries[:5], covis) == [_reloc(b, mb, [q], covis)[0] for q in queries[:5]]   # the state carries over to the next call


def test_vectors_straight_from_the_device_transform():
    import torch
    from rgbd_pl_slam_amd import KeyFrameDatabase
    ref = bowref.make_vocab(21, 6, 3, weighting=bowref.TF_IDF, scoring=bowref.L1_NORM)
    from rgbd_pl_slam_amd import Vocabulary
    V = Vocabulary.from_arrays(ref.k, ref.L, ref.scoring, ref.weighting, ref.parent, ref.desc, ref.weight, ref.is_leaf)
    cap, n_kf, n_q = 48, 40, 6
    frames = [bowref.make_descriptors(ref, 100 + f, 20 + (f * 7) % 29) for f in range(n_kf + n_q)]
    d = np.full((len(frames), cap, 32), 0xA5, np.uint8)
    for f, fr in enumerate(frames): d[f, :len(fr)] = fr
    n = torch.from_numpy(np.array([len(fr) for fr in frames], np.int32)).cuda()
    out = V.transform(torch.from_numpy(d).cuda(), n, 1)
    torch.cuda.synchronize()
    db = KeyFrameDatabase(V, n_kf, cap)
    model = kfdbref.SlotModel(ref.scoring, ref.n_words, n_kf)
    kf = {k: out[k][:n_kf] for k in ("word_id", "word_val", "n_words")}     # views of the transform's own output: no host round trip
    qs = {k: out[k][n_kf:] for k in ("word_id", "word_val", "n_words")}
    db.add(kf, range(n_kf))
    bows = [bowref.transform(ref, fr, 1)[0] for fr in frames]
    model.add(bows[:n_kf], range(n_kf))
    covis = [[(s + 1) % n_kf, (s + 3) % n_kf, -1] for s in range(n_kf)]
    got = _results(db.detect_relocalization_candidates(qs, _csr(covis), 16), 16)
    assert got == _expect(model.detect_reloc(bows[n_kf:], covis), 16)
    assert any(g[1] for g in got)


def test_chunked_queries_carry_the_stale_score_across_chunks():
    """max_keyframes = 2^20 makes the chunk 2^22 / 2^20 = 4 queries: 70 queries run as 18 chunks (q0 > 0 in every kernel, the pair counter reset per chunk),
    and the persistent score crosses chunk borders through the per-slot array"""
    S, n_kf = 1 << 20, 90
    bows, covis, _ = _world(11, n_kf, 96)
    queries = random_bows(5, 70, NW, 3, CAP, pool=np.arange(0, 40))
    slots = [int(s) for s in np.random.default_rng(2).permutation(96)[:n_kf]]
    a, ma = _pair(bowref.L1_NORM, S)
    covis_a = covis + [[]] * (S - 96)                                        # the CSR at its documented length: max_keyframes + 1 starts
    a.add(_pack(bows, CAP), slots); ma.add(bows, slots)
    b, mb = _pair(bowref.L1_NORM, 96)                                        # the same world in one chunk
    b.add(_pack(bows, CAP), slots); mb.add(bows, slots)
    before = ma.db.stale_reads
    one = _reloc(a, ma, queries, covis_a)
    assert ma.db.stale_reads > before
    assert one == _reloc(b, mb, queries, covis)
    ms = [0.0] * 70
    conn = [[slots[q % n_kf]] for q in range(70)]
    assert _loop(a, ma, queries, ms, covis_a, conn) == _loop(b, mb, queries, ms, covis, conn)
    assert _reloc(a, ma, queries[:9], covis_a) == _reloc(b, mb, queries[:9], covis)


def test_more_scored_keyframes_than_the_lds_sort_holds():
    """4100 identical keyframes are all scored by one query: 8192 sort keys, beyond the 4096 the workgroup sorts in LDS, so the sort and its padding
    run in global memory; added in a permuted slot order, so the output order is the sort's doing"""
    n_kf, S = 4100, 4200
    bow = [(3, 0.25), (5, 0.25), (9, 0.5)]
    slots = [int(s) for s in np.random.default_rng(3).permutation(S)[:n_kf]]
    db, model = _pair(bowref.L1_NORM, S)
    bows = [bow] * n_kf
    db.add(_pack(bows, CAP), slots); model.add(bows, slots)
    covis = [[] for _ in range(S)]
    for i, s in enumerate(slots[:50]): covis[s] = [slots[i + 1], -1, slots[(i + 7) % n_kf]]
    got = _reloc(db, model, [bow, bow[:1]], covis, max_cand=S)
    assert got[0][1] > 40 and got[0][2][2] == n_kf and got[1][2][2] == n_kf
    got = _reloc(db, model, [bow], None, max_cand=S)
    assert got[0][0] == slots and got[0][1] == n_kf


def test_cpp_driver_equals_the_restatement(tmp_path):
    """tests/cpp/kfdb_driver.cpp: the reference-signature adapter over mock KeyFrame / Frame objects -- add, erase, re-add, clear, relocalisation and loop
    queries (the query keyframe inside and outside the database) -- against the restatement, line for line"""
    import subprocess
    from test_kfdb_ref import build_kfdb_driver
    exe, voc = build_kfdb_driver(tmp_path, flags=("-O1",))
    expect = kfdbref.driver_scenario(9, voc.n_words, str(tmp_path / "scenario.txt"))
    run = subprocess.run([str(exe), str(tmp_path)], text=True, capture_output=True)
    assert run.returncode == 0 and "kfdb driver ok" in run.stdout, "driver failed (rc %d)\n%s\n%s" % (run.returncode, run.stdout, run.stderr[-2000:])
    got = [l.strip() for l in open(str(tmp_path / "out.txt")).read().split("\n")[:-1]]
    assert got == expect, [(i, g, e) for i, (g, e) in enumerate(zip(got, expect)) if g != e][:5]

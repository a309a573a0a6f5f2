"""KeyFrameDatabase, CPU side: the restatement (tests/kfdbref.py) against a hand-worked fixture, properties of the restatement, and the
argument checks of the plf_kfdb_* entry points, which run before any device work.  No GPU needed."""
import ctypes as C
import json
import os

import numpy as np

import bowref
import kfdbref
from cppbuild import build_driver
from kfdbref import random_bows

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _bow(rows):
    return [(int(w), float(v)) for w, v in rows]


def test_restatement_equals_the_hand_worked_fixture():
    fx = json.load(open(os.path.join(GOLD, "kfdb_tiny.json")))
    m = kfdbref.SlotModel(fx["scoring"], fx["n_words"], len(fx["keyframes"]))
    m.add([_bow(k["bow"]) for k in fx["keyframes"]], [k["slot"] for k in fx["keyframes"]])
    assert [[k.slot for k in lst] for lst in m.db.mvInvertedFile] == fx["inverted_file"]
    stale_before = 0
    for q in fx["queries"]:
        (cand, stats), = m.detect_reloc([_bow(q["bow"])], fx["covis"])
        t = m.db.trace
        assert [list(x) for x in t["lKFsSharingWords"]] == q["lKFsSharingWords"], q["name"]
        assert (t["maxCommonWords"], t["minCommonWords"]) == (q["maxCommonWords"], q["minCommonWords"]), q["name"]
        assert [list(x) for x in t["lScoreAndMatch"]] == q["lScoreAndMatch"], q["name"]
        assert [list(x) for x in t["lAccScoreAndMatch"]] == q["lAccScoreAndMatch"], q["name"]
        assert (float(t["bestAccScore"]), t["minScoreToRetain"]) == (q["bestAccScore"], q["minScoreToRetain"]), q["name"]
        assert cand == q["candidates"], q["name"]
        assert [float(k.mRelocScore) for k in m.kf] == q["mRelocScore_after"], q["name"]
        assert stats == (len(q["lKFsSharingWords"]), q["maxCommonWords"], len(q["lScoreAndMatch"]), int(np.float32(q["bestAccScore"]).view(np.uint32)))
        assert m.db.stale_reads - stale_before == q.get("stale_reads", m.db.stale_reads - stale_before)
        stale_before = m.db.stale_reads
    # the fixture's three special cases are really in it
    A, _, Cq = fx["queries"]
    assert [w for _, w in A["lKFsSharingWords"]].count(A["minCommonWords"]) == 1 and len(A["lScoreAndMatch"]) == 2          # the tie is not scored
    assert [k for _, k in A["lAccScoreAndMatch"]] == [0, 0] and A["candidates"] == [0]                                       # de-duplicated
    fresh = kfdbref.SlotModel(fx["scoring"], fx["n_words"], len(fx["keyframes"]))
    fresh.add([_bow(k["bow"]) for k in fx["keyframes"]], [k["slot"] for k in fx["keyframes"]])
    assert fresh.detect_reloc([_bow(Cq["bow"])], fx["covis"])[0][0] == Cq["candidates_without_stale_score"] != Cq["candidates"]   # the stale score decides


def test_float_truncation_never_differs_from_double_in_range():
    """A maxCommonWords at which (int)(x * 0.8f) differs from (int)(x * 0.8) was looked for and does not exist: 0.8f exceeds 0.8 by 1.5e-8
    relative, less than half an ulp of the float product, so for multiples of 5 the product rounds back to the integer, and every other x
    is 0.2 away from one.  Checked for every count a vector of PLF_BOW_MAX_CAPACITY words (and far beyond) can reach; a device test of such
    a case would prove nothing, so there is none."""
    x = np.arange(1, 100001)
    f = (x.astype(np.float32) * np.float32(0.8)).astype(np.int64)
    assert np.array_equal(f, (x.astype(np.float64) * 0.8).astype(np.int64)) and np.array_equal(f, 4 * x // 5)
    assert not any(kfdbref.truncation_differs(int(v)) for v in (5, 10, 8190, 8192))


def test_erase_then_add_moves_the_keyframe_to_the_end_of_its_lists():
    bows = [[(0, 0.5), (1, 0.5)], [(0, 0.5), (2, 0.5)], [(0, 1.0)]]
    m = kfdbref.SlotModel(bowref.L1_NORM, 4, 3)
    m.add(bows, [0, 1, 2])
    assert [k.slot for k in m.db.mvInvertedFile[0]] == [0, 1, 2]
    q = [(0, 1.0)]
    first = m.detect_reloc([q])[0]
    m.erase([0])
    assert [k.slot for k in m.db.mvInvertedFile[0]] == [1, 2] and m.db.mvInvertedFile[1] == []
    m.add([bows[0]], [0])
    assert [k.slot for k in m.db.mvInvertedFile[0]] == [1, 2, 0] and m.db.n_entries() == 5
    m.detect_reloc([q])
    assert [s for s, _ in m.db.trace["lKFsSharingWords"]] == [1, 2, 0]
    assert first[1][0] == 3


def _world(seed, scoring=bowref.L1_NORM, n_kf=40, n_words=60):
    bows = random_bows(seed, n_kf, n_words, 3, 12)
    rng = np.random.default_rng(seed + 1)
    covis = [list(rng.integers(-1, n_kf, int(rng.integers(0, 13)))) for _ in range(n_kf)]
    queries = random_bows(seed + 2, 30, n_words, 3, 12)
    return bows, covis, queries


def test_a_batch_equals_single_queries_in_order_and_the_state_matters():
    bows, covis, queries = _world(3)
    a = kfdbref.SlotModel(bowref.L1_NORM, 60, 40); a.add(bows, range(40))
    b = kfdbref.SlotModel(bowref.L1_NORM, 60, 40); b.add(bows, range(40))
    one = a.detect_reloc(queries, covis)
    many = [b.detect_reloc([q], covis)[0] for q in queries]
    assert one == many
    assert [float(k.mRelocScore) for k in a.kf] == [float(k.mRelocScore) for k in b.kf]
    assert a.db.stale_reads > 0
    rev = kfdbref.SlotModel(bowref.L1_NORM, 60, 40); rev.add(bows, range(40))
    assert rev.detect_reloc(queries[::-1], covis)[::-1] != one                       # order dependent, as the reference is


def test_loop_queries_leave_no_state():
    bows, covis, queries = _world(5)
    a = kfdbref.SlotModel(bowref.L1_NORM, 60, 40); a.add(bows, range(40))
    b = kfdbref.SlotModel(bowref.L1_NORM, 60, 40); b.add(bows, range(40))
    conn = [[q % 40, (q * 7) % 40] for q in range(len(queries))]
    ref_loop = kfdbref.SlotModel(bowref.L1_NORM, 60, 40); ref_loop.add(bows, range(40))
    loops = ref_loop.detect_loop(queries, [0.01] * len(queries), covis, conn)
    assert any(c for c, _ in loops)
    out_a, out_b = [], []
    for i, q in enumerate(queries):
        out_a.append(a.detect_reloc([q], covis)[0])
        assert b.detect_loop([queries[-1 - i]], [0.0], covis, [conn[i]]) is not None
        out_b.append(b.detect_reloc([q], covis)[0])
        assert b.detect_loop([q], [0.01], covis, [conn[i]])[0] == loops[i]          # ... and loop results do not depend on what ran before
    assert out_a == out_b


def test_symbols_are_exported_and_reject_bad_arguments_without_a_device():
    import rgbd_pl_slam_amd
    from rgbd_pl_slam_amd import _lib as L
    assert hasattr(rgbd_pl_slam_amd, "KeyFrameDatabase")
    lib = L.kfdb_prototypes(L.lib())
    for name in ("plf_kfdb_create", "plf_kfdb_destroy", "plf_kfdb_info", "plf_kfdb_set_n_best", "plf_kfdb_add_batch", "plf_kfdb_erase_batch",
                 "plf_kfdb_clear", "plf_kfdb_vectors", "plf_kfdb_detect_reloc", "plf_kfdb_detect_loop", "plf_vocab_device"):
        assert hasattr(lib, name), name
    h = C.c_void_p()
    assert lib.plf_kfdb_create(None, 10, 10, C.byref(h)) == L.PLF_E_BADARG and not h.value
    assert lib.plf_kfdb_create(None, 10, 10, None) == L.PLF_E_BADARG
    assert lib.plf_vocab_device(None) == L.PLF_E_BADARG
    info = L.KfdbInfo()
    assert lib.plf_kfdb_info(None, C.byref(info)) == L.PLF_E_BADARG
    assert lib.plf_kfdb_set_n_best(None, 10) == L.PLF_E_BADARG
    assert lib.plf_kfdb_add_batch(None, None, None, None, 0, 0, None, None) == L.PLF_E_BADARG
    assert lib.plf_kfdb_erase_batch(None, None, 0) == L.PLF_E_BADARG
    assert lib.plf_kfdb_clear(None) == L.PLF_E_BADARG
    assert lib.plf_kfdb_vectors(None, None, None, None) == L.PLF_E_BADARG
    assert lib.plf_kfdb_detect_reloc(None, None, None, None, 0, 0, None, None, 0, None, None, None, None) == L.PLF_E_BADARG
    assert lib.plf_kfdb_detect_loop(None, None, None, None, 0, 0, None, None, None, None, None, 0, None, None, None, None) == L.PLF_E_BADARG
    lib.plf_kfdb_destroy(None)


def build_kfdb_driver(tmp_path, flags=("-Werror",)):
    exe = build_driver("kfdb_driver", tmp_path, "-Wall", *flags)
    voc = bowref.make_vocab(2, 10, 2)
    bowref.save_text(voc, str(tmp_path / "voc.txt"))
    return exe, voc


def test_cpp_database_mirror_compiles_and_never_falls_back(tmp_path):
    """ORB_SLAM2_PLF::KeyFrameDatabase with the reference's signatures over tests/mock/ORB_SLAM2/mock_kfdb.h: built here with -Werror; without a GPU the
    driver must stop with plf::Error(PLF_E_HIP) at the vocabulary (tests/test_gpu_kfdb.py runs it on the GPU against the restatement)"""
    import subprocess
    from conftest import gpu_available
    exe, voc = build_kfdb_driver(tmp_path)
    expect = kfdbref.driver_scenario(4, voc.n_words, str(tmp_path / "scenario.txt"))
    run = subprocess.run([str(exe), str(tmp_path)], text=True, capture_output=True)
    if gpu_available():
        assert run.returncode == 0 and "kfdb driver ok" in run.stdout, run.stdout + run.stderr[-1000:]
        assert open(str(tmp_path / "out.txt")).read().split("\n")[:-1] == [e + " " if e else "" for e in expect]
    else:
        assert run.returncode == 1 and "plf error -4" in run.stdout, run.stdout

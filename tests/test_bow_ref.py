"""DBoW2 vocabulary, CPU side: the numpy restatement (tests/bowref.py) against a hand-worked fixture, the text-file loader of the library against
bowref's, and the host-side validation of plf_vocab_create.  No GPU needed: parsing and validation run before any device work."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import bowref
from conftest import gpu_available
from cppbuild import build_driver

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _lib():
    from rgbd_pl_slam_amd import _lib as L
    return L, L.bow_prototypes(L.lib())


def _create(L, lib, k, Lv, scoring, weighting, parent, desc, weight, leaf):
    parent = np.ascontiguousarray(parent, np.int32); desc = np.ascontiguousarray(desc, np.uint8)
    weight = np.ascontiguousarray(weight, np.float64); leaf = np.ascontiguousarray(leaf, np.uint8)
    d = L.VocabDesc(k, Lv, scoring, weighting, len(parent), parent.ctypes.data, desc.ctypes.data, weight.ctypes.data, leaf.ctypes.data)
    h = C.c_void_p()
    st = lib.plf_vocab_create(C.byref(d), 0, C.byref(h))
    if h.value:
        lib.plf_vocab_destroy(h)
    return st


def test_bowref_equals_the_hand_worked_fixture():
    fx = json.load(open(os.path.join(GOLD, "bow_tiny.json")))
    voc = bowref.parse_text(os.path.join(GOLD, "bow_tiny_voc.txt"))
    assert (voc.k, voc.L, voc.scoring, voc.weighting, voc.n_nodes(), voc.n_words, voc.min_leaf_depth) == (3, 2, 0, 0, 13, 9, 2)
    desc = np.array(fx["descriptors"], np.uint8)
    word, weight, _ = bowref.descend(voc, desc, 0)
    assert word.tolist() == fx["words"] and weight.tolist() == fx["weights"]
    # sequential adds, not count * weight: the two differ for six hits of weight 0.1
    assert fx["word0_value_before_norm"] == 0.6 != fx["count_times_weight"] == 6 * 0.1
    for lu, fv_exp in fx["fv"].items():
        bow, fv = bowref.transform(voc, desc, int(lu))
        assert [w for w, _ in bow] == [w for w, _ in fx["bow"]]
        assert np.array_equal(np.array([v for _, v in bow]).view(np.uint64), np.array([v for _, v in fx["bow"]]).view(np.uint64))
        assert [[n, f] for n, f in fv] == fv_exp
    assert bow[0][1] == 0.6 / fx["l1_norm"] != (6 * 0.1) / fx["l1_norm"]


@pytest.mark.parametrize("k,Lv,uneven", [(3, 2, False), (10, 3, False), (20, 2, True), (2, 6, True)])
def test_parser_equals_bowref_and_skips_blank_lines(tmp_path, k, Lv, uneven):
    from rgbd_pl_slam_amd import bow
    voc = bowref.make_vocab(5 + k, k, Lv, weighting=bowref.TF_IDF, scoring=bowref.L2_NORM, zero_share=0.1, shallow_share=0.2, uneven=uneven)
    for name, kw in (("plain.txt", {}), ("trailing.txt", {"trailing_blank_lines": 2}), ("inside.txt", {"blank_inside": True, "trailing_blank_lines": 1})):
        path = str(tmp_path / name)
        bowref.save_text(voc, path, **kw)
        ref = bowref.parse_text(path)
        got = bow.parse_text(path)
        assert (got["k"], got["L"], got["scoring"], got["weighting"]) == (k, Lv, bowref.L2_NORM, bowref.TF_IDF)
        assert len(got["parent"]) == voc.n_nodes() == ref.n_nodes()
        assert np.array_equal(got["parent"][1:], voc.parent[1:]) and np.array_equal(got["desc"][1:], voc.desc[1:])
        assert np.array_equal(got["is_leaf"][1:], voc.is_leaf[1:])
        assert np.array_equal(got["weight"].view(np.uint64), voc.weight.view(np.uint64)) and np.array_equal(ref.weight.view(np.uint64), voc.weight.view(np.uint64))


@pytest.mark.parametrize("header", ["21 3 0 0", "-1 3 0 0", "10 0 0 0", "10 11 0 0", "10 3 6 0", "10 3 -1 0", "10 3 0 4", "10 3 0 -1", "10 3 0", "voc"])
def test_parser_rejects_the_headers_the_reference_rejects(tmp_path, header):
    """TemplatedVocabulary.h:1383 (a header with fewer than four numbers leaves the reference's fields unset: refused here too)"""
    L, lib = _lib()
    path = tmp_path / "bad.txt"
    path.write_text(header + "\n0 1 " + " ".join(["0"] * 32) + " 1.0\n")
    d = L.VocabDesc()
    assert lib.plf_vocab_parse_text(str(path).encode(), C.byref(d)) == L.PLF_E_BADARG and not d.parent
    h = C.c_void_p()
    assert lib.plf_vocab_load_text(str(path).encode(), 0, C.byref(h)) == L.PLF_E_BADARG and not h.value


def test_parser_accepts_the_header_bounds_and_rejects_malformed_lines(tmp_path):
    L, lib = _lib()
    node = "0 1 " + " ".join(["7"] * 32) + " 0.5\n"
    for header in ("0 1 0 0", "20 10 5 3"):
        p = tmp_path / "ok.txt"; p.write_text(header + "\n" + node)
        d = L.VocabDesc()
        assert lib.plf_vocab_parse_text(str(p).encode(), C.byref(d)) == L.PLF_OK and d.n_nodes == 2
        lib.plf_vocab_desc_free(C.byref(d))
        assert not d.parent
    for bad in ("0 1 " + " ".join(["7"] * 31) + "\n", "5 1 " + " ".join(["7"] * 32) + " 0.5\n", "0 1 x\n"):   # short line, parent ahead of its child, text
        p = tmp_path / "bad.txt"; p.write_text("3 2 0 0\n" + bad)
        d = L.VocabDesc()
        assert lib.plf_vocab_parse_text(str(p).encode(), C.byref(d)) == L.PLF_E_BADARG
    d = L.VocabDesc()
    assert lib.plf_vocab_parse_text(str(tmp_path / "missing.txt").encode(), C.byref(d)) == L.PLF_E_EMPTY
    assert lib.plf_vocab_parse_text(None, C.byref(d)) == L.PLF_E_BADARG
    assert lib.plf_vocab_parse_text(str(tmp_path / "ok.txt").encode(), None) == L.PLF_E_BADARG


def test_malformed_trees_and_null_pointers_are_rejected_before_touching_the_device():
    L, lib = _lib()
    z = lambda n: np.zeros((n, 32), np.uint8)
    w = lambda n: np.ones(n)
    good = dict(parent=[0, 0, 0, 1, 1], leaf=[0, 0, 1, 1, 1])
    bad = {
        "child listed before its parent": dict(parent=[0, 2, 0, 1, 1], leaf=[0, 0, 0, 1, 1]),
        "inner node without children": dict(parent=[0, 0, 0, 1, 1], leaf=[0, 0, 0, 1, 1]),
        "leaf with children": dict(parent=[0, 0, 0, 2, 1], leaf=[0, 0, 1, 1, 1]),
        "33 children": dict(parent=[0] * 34, leaf=[0] + [1] * 33),
        "negative parent": dict(parent=[0, -1, 0, 1, 1], leaf=[0, 0, 1, 1, 1]),
        "root only": dict(parent=[0], leaf=[0]),
        "root is a leaf": dict(parent=[0, 0], leaf=[1, 1]),
    }
    for why, t in bad.items():
        n = len(t["parent"])
        assert _create(L, lib, 3, 2, 0, 0, t["parent"], z(n), w(n), t["leaf"]) == L.PLF_E_BADARG, why
    n = 5
    assert _create(L, lib, 3, 1, 0, 0, good["parent"], z(n), w(n), good["leaf"]) == L.PLF_E_BADARG       # a leaf at depth 2 > L = 1
    assert _create(L, lib, 3, 0, 0, 0, good["parent"], z(n), w(n), good["leaf"]) == L.PLF_E_BADARG
    assert _create(L, lib, 3, 2, 6, 0, good["parent"], z(n), w(n), good["leaf"]) == L.PLF_E_BADARG
    assert _create(L, lib, 3, 2, 0, 4, good["parent"], z(n), w(n), good["leaf"]) == L.PLF_E_BADARG
    h = C.c_void_p()
    assert lib.plf_vocab_create(None, 0, C.byref(h)) == L.PLF_E_BADARG
    d = L.VocabDesc(3, 2, 0, 0, 5, None, None, None, None)
    assert lib.plf_vocab_create(C.byref(d), 0, C.byref(h)) == L.PLF_E_BADARG and not h.value
    par = np.array(good["parent"], np.int32)
    d = L.VocabDesc(3, 2, 0, 0, 5, par.ctypes.data, None, None, None)
    assert lib.plf_vocab_create(C.byref(d), 0, None) == L.PLF_E_BADARG
    assert lib.plf_vocab_info(None, None) == L.PLF_E_BADARG
    assert lib.plf_bow_transform_batch(None, None, None, 1, 8, 0, 0, 0, None, None, None, None, None, None, None, None) == L.PLF_E_BADARG
    assert lib.plf_bow_score(None, None, None, 0, None, None, None, 0, None, 0, None) == L.PLF_E_BADARG
    # the valid tree passes validation: what is left is the device
    st = _create(L, lib, 3, 2, 0, 0, good["parent"], z(n), w(n), good["leaf"])
    assert st == (L.PLF_OK if gpu_available() else L.PLF_E_HIP)


def test_no_vocabulary_without_a_gpu():
    """as every other create: PLF_E_HIP, never a CPU path"""
    L, lib = _lib()
    h = C.c_void_p()
    st = lib.plf_vocab_load_text(os.path.join(GOLD, "bow_tiny_voc.txt").encode(), 0, C.byref(h))
    if gpu_available():
        assert st == L.PLF_OK and h.value
        lib.plf_vocab_destroy(h)
    else:
        assert st == L.PLF_E_HIP and not h.value
        from rgbd_pl_slam_amd import Vocabulary, PlfError
        with pytest.raises(PlfError):
            Vocabulary.from_text(os.path.join(GOLD, "bow_tiny_voc.txt"))


def test_cpp_vocabulary_mirror_compiles_and_never_falls_back(tmp_path):
    """plf::ORBVocabulary with the reference's transform signature over tests/mock/ (cv::Mat, DBoW2::BowVector / FeatureVector): built here; without a GPU
    loading a good file must throw plf::Error(PLF_E_HIP), a missing file just returns false (tests/test_gpu_bow.py runs the driver on the GPU)"""
    import subprocess
    exe = build_driver("bow_driver", tmp_path, "-Wall", "-Werror")
    voc = bowref.make_vocab(1, 3, 2)
    bowref.save_text(voc, str(tmp_path / "voc.txt"))
    bowref.make_descriptors(voc, 1, 10).tofile(str(tmp_path / "desc1.u8")); bowref.make_descriptors(voc, 2, 10).tofile(str(tmp_path / "desc2.u8"))
    run = subprocess.run([str(exe), str(tmp_path)], text=True, capture_output=True)
    if gpu_available():
        assert run.returncode == 0 and "bow driver ok" in run.stdout, run.stdout + run.stderr[-1000:]
    else:
        assert run.returncode == 1 and "plf error -4" in run.stdout and "a missing file loaded" not in run.stdout, run.stdout

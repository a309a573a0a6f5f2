"""ComputeDistinctiveDescriptors, CPU side: the numpy restatement (tests/mapref.py) against the hand-worked fixture and its own properties, the C ABI
of the new entry point, and the C++ adapter against the mocks.  No GPU needed: the argument checks run before any device work."""
import ctypes as C
import os
import subprocess

import numpy as np

import mapref
from conftest import gpu_available
from cppbuild import build_driver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def test_restatement_equals_the_hand_worked_fixture():
    cases = mapref.load_fixture(os.path.join(GOLD, "distinct_tiny.json"))
    assert len(cases) == 8
    for c in cases:
        assert mapref.distinctive(c["desc"], c["valid_arr"]) == (c["best_obs"], c["best_median"]), c["name"]
    # the distances the fixture's working is written with
    c = cases[3]
    assert mapref.hamming_matrix(c["desc"]).tolist() == [[0, 1, 2, 8], [1, 0, 1, 7], [2, 1, 0, 6], [8, 7, 6, 0]]


def test_hamming_matrix_equals_popcount():
    rng = np.random.default_rng(1)
    d = rng.integers(0, 256, (40, 32), dtype=np.uint8)
    ref = np.array([[int(np.unpackbits(a ^ b).sum()) for b in d] for a in d])
    assert np.array_equal(mapref.hamming_matrix(d), ref)


def test_invalid_entries_do_not_matter_wherever_they_sit():
    rng = np.random.default_rng(2)
    for trial in range(200):
        n = int(rng.integers(1, 30))
        _, d, _ = mapref.make_points(trial, [n])
        pos, med = mapref.distinctive(d)
        # interleave invalid rows of arbitrary content at arbitrary places: the chosen descriptor and its median stay
        k = int(rng.integers(1, 10))
        slots = np.sort(rng.integers(0, n + 1, k))
        full = np.insert(d, slots, rng.integers(0, 256, (k, 32), dtype=np.uint8), axis=0)
        valid = np.insert(np.ones(n, np.uint8), slots, 0)
        p2, m2 = mapref.distinctive(full, valid)
        assert m2 == med and np.array_equal(full[p2], d[pos]) and valid[p2] == 1
        assert p2 == np.flatnonzero(valid)[pos]                # the position counts the invalid rows, the choice does not see them
        # and the content of an invalid row is irrelevant
        full2 = full.copy(); full2[valid == 0] = 0xA5
        assert mapref.distinctive(full2, valid) == (p2, m2)


def test_permutation_changes_the_result_only_through_ties():
    rng = np.random.default_rng(3)
    moved = 0
    for trial in range(300):
        n = int(rng.integers(2, 40))
        _, d, _ = mapref.make_points(1000 + trial, [n])
        pos, med = mapref.distinctive(d)
        D = mapref.hamming_matrix(d)
        meds = np.sort(D, axis=1)[:, int(0.5 * (n - 1))]
        perm = rng.permutation(n)
        p2, m2 = mapref.distinctive(d[perm])
        assert m2 == med                                        # the best median is order-free
        assert meds[perm[p2]] == med                            # the chosen row is one of the rows that attain it ...
        first = min(i for i in range(n) if meds[perm[i]] == med)
        assert p2 == first                                      # ... namely the earliest of them in the new order
        if (meds == med).sum() == 1:
            assert perm[p2] == pos
        else:
            moved += perm[p2] != pos
    assert moved > 20                                           # ties are frequent in this generator, and the order decides them


def test_median_equals_partition_and_the_counting_rule():
    """sorted[(int)(0.5 * (N - 1))] = np.partition at that index = the smallest t with #{d <= t} > k (what the kernels compute)"""
    rng = np.random.default_rng(4)
    for trial in range(200):
        n = int(rng.integers(1, 70))
        _, d, _ = mapref.make_points(2000 + trial, [n], max_flips=int(rng.integers(1, 60)))
        D = mapref.hamming_matrix(d)
        k = int(0.5 * (n - 1))
        assert k == (n - 1) // 2
        med = np.sort(D, axis=1)[:, k]
        assert np.array_equal(med, np.partition(D, k, axis=1)[:, k])
        t = np.array([min(t for t in range(257) if (row <= t).sum() > k) for row in D])
        assert np.array_equal(med, t)


def test_abi_declares_and_exports_the_entry_point():
    """fails on a tree without the feature: plf.h has to declare plf_map_distinctive_descriptors and the cross-compiled library has to export it"""
    hdr = open(os.path.join(ROOT, "include", "plf.h")).read()
    assert "int plf_map_distinctive_descriptors(const plf_map_obs_view *obs" in hdr and "} plf_map_obs_view;" in hdr
    from rgbd_pl_slam_amd import _lib as L
    lib = L.map_prototypes(L.lib())
    assert hasattr(lib, "plf_map_distinctive_descriptors")
    import rgbd_pl_slam_amd
    assert callable(rgbd_pl_slam_amd.distinctive_descriptors) and rgbd_pl_slam_amd.MapLine.ComputeDistinctiveDescriptors is rgbd_pl_slam_amd.distinctive_descriptors


def test_misuse_is_refused_before_any_device_work():
    from rgbd_pl_slam_amd import _lib as L
    lib = L.map_prototypes(L.lib())
    a = 0x1000   # never dereferenced: every call below has to fail on the host
    call = lambda v, md=a, bo=a, bm=a, rows=4: lib.plf_map_distinctive_descriptors(C.byref(v) if v is not None else None, md, rows, bo, bm, 0, None)
    mk = lambda **kw: L.MapObsView(**{**dict(n_points=4, obs_start=a, obs_desc=a), **kw})
    assert call(None) == L.PLF_E_BADARG
    assert call(mk(), md=None) == L.PLF_E_BADARG and call(mk(), bo=None) == L.PLF_E_BADARG and call(mk(), bm=None) == L.PLF_E_BADARG
    assert call(mk(obs_start=None)) == L.PLF_E_BADARG
    assert call(mk(n_points=-1)) == L.PLF_E_BADARG
    assert call(mk(obs_desc=None)) == L.PLF_E_BADARG                                              # neither form
    assert call(mk(obs_kf=a, obs_idx=a, kf_desc=a, n_kf=1)) == L.PLF_E_BADARG                       # both forms
    assert call(mk(obs_desc=None, obs_kf=a, obs_idx=None, kf_desc=a, n_kf=1)) == L.PLF_E_BADARG     # half an indirect form
    assert call(mk(obs_desc=a + 4)) == L.PLF_E_BADARG and call(mk(), md=a + 8) == L.PLF_E_BADARG   # misaligned rows
    assert call(mk(), rows=-1) == L.PLF_E_BADARG
    assert call(mk(n_points=0)) == L.PLF_OK                                                       # nothing to do: no device needed
    if not gpu_available():
        assert call(mk()) == L.PLF_E_HIP                                                          # a well-formed call: never a CPU path


def test_cpp_adapter_compiles_against_the_mocks_and_never_falls_back(tmp_path):
    """plf::MapPoint / plf::MapLine and the ORB_SLAM2_PLF adapter over tests/mock/ORB_SLAM2/mock_map.h, driven by tests/cpp/mappoint_driver.cpp"""
    exe = build_driver("mappoint_driver", tmp_path, "-Wall", "-Werror")
    start, desc, _ = mapref.make_points(5, [3, 0, 20, 1])
    mapref.write_driver_input(tmp_path, start, desc, n_kf=32, seed=5)
    run = subprocess.run([str(exe), str(tmp_path)], text=True, capture_output=True)
    if gpu_available():
        assert run.returncode == 0 and "mappoint driver ok" in run.stdout, run.stdout + run.stderr[-1000:]
    else:
        assert run.returncode == 1 and "plf error -4" in run.stdout, run.stdout + run.stderr[-1000:]

"""Local map, CPU side: the restatement (tests/localmapref.py) against the fixture tests/golden/localmap_tiny.json -- results recorded from the
mock C++ program tests/cpp/localmap_mock.cpp, which is built and run here again --, against an independent brute-force definition with
hypothesis, and the argument checks of the four entry points, which run before any device work.  No GPU needed."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
from hypothesis import given, settings, strategies as st

import covisref
import localmapref as R
from cppbuild import build_driver

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")


def load_fixture():
    return json.load(open(os.path.join(GOLD, "localmap_tiny.json")))


def scenario_lines(fx, track=True):
    """the fixture's world as the scenario of tests/cpp/localmap_scenario.h"""
    n_kf = fx["n_kf"]
    lines = ["pool %d" % fx["pool"]] + ["kf %d %d %d" % (k, fx["kf_pos"][k], fx["kf_bad"][k]) for k in range(n_kf)]
    lines += ["parent %d %d" % (k, p) for k, p in enumerate(fx["parent"]) if p >= 0]
    lines += ["covis %d %d %s" % (k, len(c), " ".join(map(str, c))) for k, c in enumerate(fx["covis"]) if c]
    lines += ["point %d %d %d %s" % (p, fx["point_bad"][p], len(o), " ".join(map(str, o))) for p, o in enumerate(fx["obs"])]
    lines += ["row %d %d %s" % (k, len(r), " ".join(map(str, r))) for k, r in enumerate(fx["rows"]) if r]
    for f in fx["frames"]:
        lines.append("frame %d %d %s" % (f["id"], len(f["own"]), " ".join(map(str, f["own"]))))
        lines.append("infrustum %d %d %s" % (f["id"], len(f["in_frustum"]), " ".join(map(str, f["in_frustum"]))))
    if track:
        lines += ["track %d" % f["id"] for f in fx["frames"]]
    return lines


def parse_out(text):
    """out.txt of localmap_mock.cpp / localmap_driver.cpp -> one dict per tracked frame"""
    frames = []
    for line in text.split("\n"):
        w = line.split()
        if not w:
            continue
        if w[0] == "frame":
            cut = [w.index(k) for k in ("kfs", "ref", "points", "seen", "own")] + [len(w)]
            part = lambda i: [int(x) for x in w[cut[i] + 1:cut[i + 1]]]    # noqa: E731
            frames.append(dict(id=int(w[1]), kfs=part(0), ref=part(1)[0], points=part(2), seen=part(3), own=part(4)))
        elif w[0] == "head":
            frames[-1]["ntomatch"] = int(w[3])
            frames[-1]["visible"] = {x.split(":")[0]: int(x.split(":")[1]) for x in w[5:]}
    return frames


def restate(fx, f):
    """one frame of the fixture through the Python restatements"""
    n_kf, pos, kf_bad, bad, obs = fx["n_kf"], fx["kf_pos"], fx["kf_bad"], fx["point_bad"], fx["obs"]
    votes = covisref.local_keyframe_votes(f["own"], obs, n_kf, bad, kf_bad, pos)
    seed = [k for k, _ in votes["conn"]] if votes else []
    children = [sorted((k for k in range(n_kf) if fx["parent"][k] == s), key=lambda k: pos[k]) for s in range(n_kf)]
    kfs = R.local_keyframes(seed, fx["covis"], children, fx["parent"], kf_bad)
    points, seen = R.local_items(kfs, fx["rows"], len(obs), bad, f["own"])
    visible = [0] * len(obs)
    _, n = R.search_local_head(points, [p in f["in_frustum"] for p in points], len(obs), bad, f["own"], visible)
    own = [-1 if p < 0 or bad[p] else p for p in f["own"]]
    return dict(id=f["id"], kfs=kfs, ref=votes["max"][0] if votes else -1, points=points, seen=seen, own=own, ntomatch=n,
                visible={str(p): v for p, v in enumerate(visible) if v})


def test_restatement_equals_the_recorded_fixture():
    fx = load_fixture()
    assert [restate(fx, f) for f in fx["frames"]] == fx["recorded"]


def test_the_mock_program_reproduces_what_the_fixture_records(tmp_path):
    fx = load_fixture()
    exe = tmp_path / "localmap_mock"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(HERE, "mock"), os.path.join(HERE, "cpp", "localmap_mock.cpp"),
                           "-o", str(exe)])
    open(str(tmp_path / "scenario.txt"), "w").write("\n".join(scenario_lines(fx)) + "\n")
    run = subprocess.run([str(exe), str(tmp_path)], text=True, capture_output=True)
    assert run.returncode == 0 and "localmap mock ok" in run.stdout, run.stdout + run.stderr[-1000:]
    assert parse_out(open(str(tmp_path / "out.txt")).read()) == fx["recorded"]


def test_every_special_case_is_really_in_the_fixture():
    fx = load_fixture()
    sp, rec, pos, kf_bad = fx["special"], {r["id"]: r for r in fx["recorded"]}, fx["kf_pos"], fx["kf_bad"]
    r0 = rec[sp["small_frame"]]
    seeds = sorted((k for k in {k for p in fx["frames"][0]["own"] if p >= 0 and not fx["point_bad"][p] for k in fx["obs"][p]} if not kf_bad[k]), key=lambda k: pos[k])
    assert r0["kfs"][:len(seeds)] == seeds and seeds != sorted(seeds)                       # key order is not id order
    assert r0["kfs"][-1] == sp["bad_parent"] and kf_bad[sp["bad_parent"]] == 1              # a bad parent is pushed all the same ...
    ender = sp["seed_whose_parent_ends_it"]
    assert fx["parent"][ender] == sp["bad_parent"] and seeds.index(ender) < len(seeds) - 1  # ... and ends the expansion with a seed left over
    left = seeds[-1]
    assert fx["covis"][left] and all(k not in r0["kfs"] for k in fx["covis"][left])         # whose neighbour would have joined
    first = seeds[0]
    assert kf_bad[fx["covis"][first][0]] == 1 and fx["covis"][first][1] in r0["kfs"]        # a bad neighbour skipped, the next one taken ...
    assert fx["covis"][first][2] not in r0["kfs"]                                           # ... and only one per category
    kids = [k for k in range(fx["n_kf"]) if fx["parent"][k] == first]
    assert len(kids) == 2 and sum(k in r0["kfs"] for k in kids) == 1 and min(kids, key=lambda k: pos[k]) in r0["kfs"] and min(kids, key=lambda k: pos[k]) != min(kids)
    pushed = fx["covis"][first][1]
    assert fx["covis"][pushed] and fx["parent"][pushed] >= 0                                # the pushed keyframe has all three, and none of them joined
    assert fx["covis"][pushed][0] not in r0["kfs"] and fx["parent"][pushed] not in r0["kfs"]
    el = sp["seed_with_eleven_neighbours"]
    assert len(fx["covis"][el]) == 11 and fx["covis"][el][10] not in r0["kfs"] and not kf_bad[fx["covis"][el][10]]
    assert all(kf_bad[k] or k in r0["kfs"] for k in fx["covis"][el][:10])
    assert [len(rec[f]["kfs"]) for f in sp["frames_with_79_80_81_seeds"]] == [82, sp["len_from_80"], 81] and sp["len_from_80"] > 80
    tw = sp["twice_in_row"]
    assert fx["rows"][tw[0]].count(tw[1]) == 2 and r0["points"].count(tw[1]) == 1
    assert sum(tw[1] in fx["rows"][k] for k in r0["kfs"]) >= 2                              # ... and across keyframes
    own = fx["frames"][0]["own"]
    b = sp["bad_own_point"]
    assert b in own and fx["point_bad"][b] and b not in r0["points"] and any(b in fx["rows"][k] for k in r0["kfs"]) and r0["own"][own.index(b)] == -1
    a = sp["own_point_absent_from_the_local_map"]
    assert a in own and not fx["point_bad"][a] and a not in r0["points"] and r0["visible"][str(a)] == 1
    assert 0 < sum(r0["seen"]) < len(r0["seen"]) and -1 in own


ids = st.integers(-2, 12)


@settings(max_examples=300, deadline=None)
@given(rows=st.lists(st.lists(ids, max_size=9), min_size=1, max_size=6), data=st.data())
def test_marking_equals_first_occurrence_found_by_a_scan(rows, data):
    local = data.draw(st.lists(st.integers(-1, len(rows)), max_size=8))
    bad = data.draw(st.one_of(st.none(), st.lists(st.integers(0, 1), min_size=11, max_size=11)))
    own = data.draw(st.one_of(st.none(), st.lists(ids, max_size=6)))
    got = R.local_items(local, rows, 11, bad, own)
    assert got == R.local_items_by_scan(local, rows, 11, bad, own)
    items, seen = got
    assert len(set(items)) == len(items) and all(0 <= p < 11 and not (bad and bad[p]) for p in items)
    in_frustum = data.draw(st.lists(st.booleans(), min_size=len(items), max_size=len(items)))
    visible = [0] * 11
    in_view, n = R.search_local_head(items, in_frustum, 11, bad, own, visible)
    assert in_view == [int(f and not s) for f, s in zip(in_frustum, seen)] and n == sum(in_view)
    want = [sum(1 for q in (own or []) if q == p and not (bad and bad[p])) for p in range(11)]
    for p, v in zip(items, in_view):
        want[p] += v
    assert visible == want


def _pad(lists, stride, fill=-1):
    a = np.full((len(lists), stride), fill, np.int32)
    for r, lst in enumerate(lists):
        a[r, :min(len(lst), stride)] = lst[:stride]
    return a


def _flat(lists):
    start = np.zeros(len(lists) + 1, np.int32)
    start[1:] = np.cumsum([len(x) for x in lists])
    return start, np.array([x for lst in lists for x in lst] + [0], np.int32)


def test_the_single_thread_loop_equals_the_restatement(tmp_path):
    """tools/localmap_cpu.cpp -- the loop tools/bench_localmap.py times -- as a stand-alone program with -fsanitize=address,undefined and -Werror, on a
    random forest with seeds on both sides of 80 and lists on both sides of their strides: its checksum against the same sum over the restatement's lists"""
    import sys
    sys.path.insert(0, os.path.join(HERE, "..", "tools"))
    import benchlib
    rng = np.random.default_rng(5)
    n_kf, n_items, SS, CS, KS, IS = 300, 900, 64, 12, 70, 200
    parent = [-1] + [int(rng.integers(0, k)) if rng.random() < 0.3 else -1 for k in range(1, n_kf)]
    children = [[k for k in range(n_kf) if parent[k] == s] for s in range(n_kf)]
    covis = [[int(x) for x in rng.choice(n_kf, int(rng.integers(0, 15)), replace=False)] for _ in range(n_kf)]
    seeds = [sorted(int(x) for x in rng.choice(n_kf, int(n), replace=False)) + [n_kf, -3] for n in rng.integers(0, 90, 40)]
    rows = [[int(x) for x in rng.integers(-1, n_items + 2, int(rng.integers(0, 60)))] for _ in range(n_kf)]
    frames = [[int(x) for x in rng.integers(-1, n_items, 30)] for _ in seeds]
    files = dict(seed_kf=_pad(seeds, SS), n_seed=np.array([len(s) for s in seeds], np.int32), covis_kf=_pad(covis, CS),
                 n_covis=np.array([len(c) for c in covis], np.int32), kf_parent=np.array(parent, np.int32))
    files["child_start"], files["child_kf"] = _flat(children)
    files["kf_row_start"], files["kf_row_item"] = _flat(rows)
    files["frame_row_start"], files["frame_row_item"] = _flat(frames)
    for k, v in files.items():
        v.tofile(str(tmp_path / (k + ".i32")))
    weight = lambda i: ((i + 1) * 2654435761) & 0xFFFFFFFF        # noqa: E731
    want = 0
    for r, s in enumerate(seeds):
        kfs = R.local_keyframes(s[:SS], [c[:CS] for c in covis], children, parent)
        items, seen = R.local_items(kfs[:KS], rows, n_items, None, frames[r])
        want += len(kfs) + len(items) + sum((k + 1) * weight(i) for i, k in enumerate(kfs[:KS]))
        want += sum((p + 1 + (sn << 40)) * weight(i) for i, (p, sn) in enumerate(zip(items[:IS], seen[:IS])))
    exe = benchlib.build_cpp("localmap_cpu.cpp", str(tmp_path), "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined")
    run = subprocess.run([exe, str(tmp_path), str(SS), str(CS), str(n_items), str(KS), str(IS), "2"], text=True, capture_output=True)
    assert run.returncode == 0 and not run.stderr, run.stderr[-2000:]
    assert int(run.stdout.split()[3]) == want & ((1 << 64) - 1)


def test_symbols_are_exported_and_reject_bad_arguments_without_a_device():
    import rgbd_pl_slam_amd
    from rgbd_pl_slam_amd import _lib as L
    for name in ("local_keyframes", "local_items", "local_gather", "local_visible", "update_local_map", "children_csr", "LocalMap", "localmap"):
        assert hasattr(rgbd_pl_slam_amd, name), name
    lib = L.localmap_prototypes(L.lib())
    buf = np.zeros(64, np.int64)
    ptr = buf.ctypes.data                                     # a non-NULL, 16-byte aligned address: the checks must not touch it
    ptr += -ptr % 16
    from conftest import gpu_available
    hip = None if gpu_available() else L.PLF_E_HIP            # a well-formed call gets as far as the device, and no further

    def kf(p=(10, 80, 8, 0), **fields):
        v = L.LocalKfView(n_rows=1, seed_kf=ptr, n_seed=ptr, seed_stride=4, covis_kf=ptr, n_covis=ptr, covis_stride=4, child_start=ptr, child_kf=ptr,
                          kf_parent=ptr, n_kf=1)
        for k, val in fields.items():
            setattr(v, k, val)
        return lib.plf_local_keyframes(C.byref(v), C.byref(L.LocalKfParams(*p)), ptr, ptr, ptr, 0, None)

    if hip:
        assert kf() == hip
    for required in ("seed_kf", "n_seed", "covis_kf", "n_covis", "child_start", "child_kf", "kf_parent"):
        assert kf(**{required: None}) == L.PLF_E_BADARG, required
    for size, val in (("n_rows", -1), ("n_kf", -1), ("seed_stride", 0), ("covis_stride", 0)):
        assert kf(**{size: val}) == L.PLF_E_BADARG, size
    for p in ((-1, 80, 8, 0), (10, -1, 8, 0), (10, 80, 0, 0), (10, 80, 8, -1)):
        assert kf(p) == L.PLF_E_BADARG, p
    assert kf((10, 80, 8, 1), n_kf=100000, seed_stride=8000) == L.PLF_E_BADARG     # more marks than the hash set holds
    assert lib.plf_local_keyframes(None, None, ptr, ptr, ptr, 0, None) == L.PLF_E_BADARG

    def items(p=(8, 0), seen=ptr, **fields):
        v = L.LocalItemsView(n_rows=1, local_kf=ptr, n_local_kf=ptr, kf_stride=4, kf_row_start=ptr, kf_row_item=ptr, n_kf=1, n_items=1)
        for k, val in fields.items():
            setattr(v, k, val)
        return lib.plf_local_items(C.byref(v), C.byref(L.LocalItemsParams(*p)), ptr, ptr, seen, ptr, 0, None)

    if hip:
        assert items() == hip and items(seen=None) == hip
    for required in ("local_kf", "n_local_kf", "kf_row_start", "kf_row_item"):
        assert items(**{required: None}) == L.PLF_E_BADARG, required
    assert items(frame_row_start=ptr) == L.PLF_E_BADARG and items(frame_row_item=ptr) == L.PLF_E_BADARG      # both or neither
    for size, val in (("n_rows", -1), ("n_kf", -1), ("n_items", -1), ("kf_stride", 0)):
        assert items(**{size: val}) == L.PLF_E_BADARG, size
    assert items((0, 0)) == L.PLF_E_BADARG and items((8, -1)) == L.PLF_E_BADARG

    def gather(pos_floats=3, desc=ptr, n_rows=1, stride=4):
        src = L.LocalMapSrc(world_pos=ptr, desc=desc, map_rows=1, pos_floats=pos_floats)
        dst = L.LocalMapDst(world_pos=ptr, desc=ptr)
        return lib.plf_local_gather(ptr, ptr, n_rows, stride, C.byref(src), C.byref(dst), 0, None)

    if hip:
        assert gather() == hip and gather(6) == hip
    assert gather(4) == L.PLF_E_BADARG and gather(desc=ptr + 8) == L.PLF_E_BADARG and gather(n_rows=-1) == L.PLF_E_BADARG and gather(stride=0) == L.PLF_E_BADARG
    assert lib.plf_local_gather(None, ptr, 1, 4, None, None, 0, None) == L.PLF_E_BADARG

    def visible(**kw):
        a = dict(local_item=ptr, n_local_item=ptr, seen=ptr, n_rows=1, stride=4, in_view=ptr, n_to_match=ptr, visible=None, fs=None, fi=None, bad=None, n_items=1)
        a.update(kw)
        return lib.plf_local_visible(a["local_item"], a["n_local_item"], a["seen"], a["n_rows"], a["stride"], a["in_view"], a["n_to_match"], a["visible"],
                                     a["fs"], a["fi"], a["bad"], a["n_items"], 0, None)

    if hip:
        assert visible() == hip and visible(seen=None) == hip
    for required in ("local_item", "n_local_item", "in_view", "n_to_match"):
        assert visible(**{required: None}) == L.PLF_E_BADARG, required
    assert visible(fs=ptr) == L.PLF_E_BADARG and visible(n_rows=-1) == L.PLF_E_BADARG and visible(stride=0) == L.PLF_E_BADARG and visible(n_items=-1) == L.PLF_E_BADARG


def build_localmap_driver(tmp_path, flags=("-Werror",)):
    return build_driver("localmap_driver", tmp_path, "-Wall", "-I", os.path.join(HERE, "cpp"), *flags)


def driver_expect(fx, path):
    """writes the driver's scenario; returns the recorded frames without the head's share, which the adapter does not run"""
    open(path, "w").write("\n".join(scenario_lines(fx)) + "\n")
    return [{k: v for k, v in r.items() if k not in ("ntomatch", "visible")} for r in fx["recorded"]]


def test_cpp_local_map_adapter_compiles_and_never_falls_back(tmp_path):
    """ORB_SLAM2_PLF::UpdateLocalMap over tests/mock/ORB_SLAM2/mock_localmap.h: built here with -Werror; without a GPU the driver must stop with
    plf::Error(PLF_E_HIP) at its first device allocation (tests/test_gpu_localmap_cpp.py runs it on the GPU against the fixture)"""
    from conftest import gpu_available
    exe = build_localmap_driver(tmp_path)
    expect = driver_expect(load_fixture(), str(tmp_path / "scenario.txt"))
    run = subprocess.run([str(exe), str(tmp_path)], text=True, capture_output=True)
    if gpu_available():
        assert run.returncode == 0 and "localmap driver ok" in run.stdout, run.stdout + run.stderr[-1000:]
        assert parse_out(open(str(tmp_path / "out.txt")).read()) == expect
    else:
        assert run.returncode == 1 and "plf error -4" in run.stdout, run.stdout

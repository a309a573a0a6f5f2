"""Culling, CPU side: the restatement (tests/cullref.py) against the hand-worked fixture tests/golden/culling_tiny.json, against the single-thread C++
loop tools/culling_cpu.cpp on random maps (a few thousand candidates), the 0.9 edge, the MapPointCulling table, the argument checks of
plf_keyframe_culling / plf_map_point_culling (which run before any device work), and the C++ loop under the sanitizers.  No GPU needed."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

import cullref
from cppbuild import build_driver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import benchlib  # noqa: E402

NAN, INF = float("nan"), float("inf")


def random_map(seed, n_kf, n_points, lo=1, hi=9, tail=0.02, cap=40, levels=4, monocular=False):
    """a consistent map: every observation (kf, idx) has rows[kf][idx] == point.  Observation counts lo .. hi with a tail up to `cap`; every row
    gets a null entry and a point listed twice; octaves 0 .. levels - 1 per key; depths inside, above, below the gate and NaN; weights 1 and 2"""
    rng = np.random.default_rng(seed)
    cnt = rng.integers(lo, hi + 1, n_points)
    long = rng.random(n_points) < tail
    cnt[long] = rng.integers(hi, cap + 1, int(long.sum()))
    cnt = np.minimum(cnt, n_kf)
    obs = [sorted(int(k) for k in rng.choice(n_kf, int(c), replace=False)) for c in cnt]
    rows = [[] for _ in range(n_kf)]
    for p, o in enumerate(obs):
        for k in o:
            rows[k].append(p)
    for r in rows:
        if len(r) > 3:
            r.insert(2, -1); r.append(r[0])
    where = [{} for _ in range(n_kf)]
    for k, r in enumerate(rows):
        for i, p in enumerate(r):
            where[k].setdefault(p, i)                               # the observation's index: the first listing
    row_level = [[int(x) for x in rng.integers(0, levels, len(r))] for r in rows]
    th = 3.0
    pick = np.array([1.0, 2.5, th, float(np.nextafter(np.float32(th), np.float32(9))), -1.0, -0.0, NAN, 40.0], np.float32)
    row_depth = [[float(x) for x in pick[rng.choice(len(pick), len(r), p=[.35, .35, .05, .05, .05, .05, .05, .05])]] for r in rows]
    return {"n_kf": n_kf, "row_kf": list(range(n_kf)), "rows": rows, "row_level": row_level, "row_depth": row_depth, "th_depth": th,
            "monocular": int(monocular), "obs": obs, "obs_idx": [[where[k][p] for k in o] for p, o in enumerate(obs)],
            "obs_w": [[int(x) for x in rng.integers(1, 3, len(o))] for o in obs],
            "obs_level": [[row_level[k][where[k][p]] for k in o] for p, o in enumerate(obs)],
            "point_bad": [int(x) for x in rng.integers(0, 12, n_points) == 0]}


def flat(m, before=(), after=(0,)):
    """the map as the flat arrays of plf_cull_view, packed forms; `before` / `after`: filler around the CSR ranges (never empty: a valid address)"""
    def csr(lists, dtype):
        start = np.zeros(len(lists) + 1, np.int64)
        start[1:] = np.cumsum([len(x) for x in lists])
        body = [x for lst in lists for x in lst]
        if dtype is np.float32:
            fill = lambda f: [np.array(v & 0xFFFFFFFF, np.uint32).view(np.float32) for v in f]   # noqa: E731
            data = np.array(fill(before) + body + fill(after), np.float32)
        else:
            data = np.array(list(before) + body + list(after), np.int64).astype(dtype)
        return (start + len(before)).astype(np.int32), data
    a = {}
    a["row_start"], a["row_point"] = csr(m["rows"], np.int32)
    _, a["row_level"] = csr(m["row_level"], np.int32)
    if m.get("row_depth") is not None:
        _, a["row_depth"] = csr(m["row_depth"], np.float32)
    a["obs_start"], a["obs_kf"] = csr(m["obs"], np.int32)
    _, a["obs_level"] = csr(m["obs_level"], np.int32)
    _, a["obs_idx"] = csr(m["obs_idx"], np.int32)
    _, a["obs_w"] = csr(m["obs_w"] or [[1] * len(o) for o in m["obs"]], np.uint8)
    a["row_kf"] = np.array(m["row_kf"], np.int32)
    a["point_bad"] = np.array(m["point_bad"] or [0] * len(m["obs"]), np.uint8)
    return a


def build_cpu_loop(tmp_path, *flags):
    return benchlib.build_cpp("culling_cpu.cpp", str(tmp_path), *flags)


def cpu_loop(exe, d, m, cand_row, cand_flags, th_obs=3, ratio=0.9, sequential=True, repeats=1):
    """tools/culling_cpu.cpp over the map: the outputs in the shape of cullref.keyframe_culling"""
    os.makedirs(d, exist_ok=True)
    ext = {np.dtype(np.int32): "i32", np.dtype(np.float32): "f32", np.dtype(np.uint8): "u8"}
    arrays = flat(m, after=())
    arrays["cand_row"] = np.array(cand_row, np.int32)
    arrays["cand_flags"] = np.array(cand_flags if cand_flags else [0] * len(cand_row), np.uint8)
    for k, v in arrays.items():
        v.tofile(os.path.join(d, "%s.%s" % (k, ext[v.dtype])))
    th_bits = int(np.array(m["th_depth"], np.float32).view(np.uint32))
    out = subprocess.run([exe, d, str(m["n_kf"]), str(th_bits), str(int(m["monocular"])), str(th_obs), repr(float(ratio)), str(int(sequential)), str(repeats)],
                         text=True, capture_output=True)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr[-3000:])
    o = np.fromfile(os.path.join(d, "out.i32"), np.int32)
    C_, K, P = len(cand_row), m["n_kf"], len(m["obs"])
    cut = np.cumsum([C_, C_, C_, K, P, P])
    parts = np.split(o, cut[:-1])
    res = {k: [int(x) for x in v] for k, v in zip(("n_mps", "n_redundant", "decision", "kf_erased", "point_went_bad", "point_nobs"), parts)}
    res["erasures"] = int(out.stdout.split()[3])
    res["ms"] = float(out.stdout.split()[1])
    return res


def test_restatement_equals_the_hand_worked_fixture():
    fx = cullref.load_fixture()
    m = fx["map"]
    got = cullref.keyframe_culling(m, fx["cand_row"], fx["cand_flags"], fx["th_obs"], fx["ratio"])
    for k, v in fx["sequential"].items():
        assert got[k] == v, k
    got = cullref.keyframe_culling(m, fx["cand_row"], fx["cand_flags"], fx["th_obs"], fx["ratio"], sequential=False)
    for k, v in fx["snapshot"].items():
        assert got[k] == v, k
    assert sum(got["kf_erased"]) == 0 and sum(got["point_went_bad"]) == 0
    got = cullref.keyframe_culling(dict(m, monocular=1), fx["cand_row"], fx["cand_flags"], fx["th_obs"], fx["ratio"])
    for k, v in fx["monocular_sequential"].items():
        assert got[k] == v, k


def test_every_special_case_is_really_in_the_fixture():
    fx = cullref.load_fixture()
    m, seq, snap = fx["map"], fx["sequential"], fx["snapshot"]
    bits = [b for row in m["row_depth_bits"] for b in row]
    th = m["th_depth_bits"]
    assert {th, th + 1, 0x80000000, 0x7FC00000} <= set(bits) and any(b > 0x80000000 and b < 0xFF800000 for b in bits)   # at, one ulp above, -0.0f, NaN, negative
    assert m["rows"][1].count(0) == 2 and -1 in m["rows"][1]                                # a point listed twice, a null entry
    assert seq["point_nobs"][0] == 2 and fx["monocular_sequential"]["point_nobs"][0] == 3   # ... erased once per erased observer
    assert fx["cand_flags"][0] & 1 and seq["decision"][0] == 3 and fx["cand_flags"][4] & 2 and seq["decision"][4] == 2
    assert snap["decision"][2] == 1 and seq["decision"][2] == 0                             # B flips from cull to keep once A is erased
    assert snap["decision"][3] == 0 and seq["decision"][3] == 1 and snap["n_mps"][3] == seq["n_mps"][3] + 1   # p1 went bad and left C's nMPs
    assert seq["point_went_bad"][1] == 1 and m["obs_w"][1] == [1, 2]
    assert sorted(sum(w) for w in (m["obs_w"][5], m["obs_w"][6], m["obs_w"][9])) == [3, 4, 4]                  # nObs 3 and 4 by weights 1 and 2
    lvl = m["row_level"][1][2]
    assert m["obs_level"][2][1:] == [lvl + 1] * 3                                           # the boundary, counting side
    assert m["obs_level"][8][0] == m["row_level"][5][3] + 2                                 # ... and the side that does not count
    assert m["obs_level"][4][-1] > m["row_level"][3][3] + 1 and m["obs"][3][-1] == 6        # third qualifying observer first / last in the list


def ratio_edge_map(n_red):
    """one row of 20 counted points, n_red of them redundant (four more observers), the others seen by one more keyframe"""
    obs = [[0, 1, 2, 3, 4] if p < n_red else [0, 1] for p in range(20)]
    return {"n_kf": 5, "row_kf": [0], "rows": [list(range(20))], "row_level": [[0] * 20], "row_depth": None, "th_depth": 0.0, "monocular": 1,
            "obs": obs, "obs_idx": [[p] * len(o) for p, o in enumerate(obs)], "obs_w": None, "obs_level": [[0] * len(o) for o in obs], "point_bad": None}


def test_the_ratio_edge_18_and_19_of_20():
    """(double)nRedundant > 0.9 * (double)nMPs with nMPs = 20: 0.9 * 20.0 rounds to exactly 18.0, so 18 is kept and 19 is culled"""
    assert 0.9 * 20.0 == 18.0
    for n_red, want in ((18, cullref.KEEP), (19, cullref.ERASED)):
        got = cullref.keyframe_culling(ratio_edge_map(n_red), [0])
        assert (got["n_mps"], got["n_redundant"], got["decision"]) == ([20], [n_red], [want])


def test_restatement_equals_the_cpp_loop_on_random_candidates(tmp_path):
    exe = build_cpu_loop(tmp_path, "-O2")
    total = erased = 0
    for seed, kw, ratio in ((1, dict(lo=1, hi=9), 0.9), (2, dict(lo=4, hi=9, levels=2), 0.6), (3, dict(lo=3, hi=12, levels=3, monocular=True), 0.5),
                            (4, dict(lo=5, hi=10, levels=1), 0.9)):
        m = random_map(seed, 150, 2500, **kw)
        rng = np.random.default_rng(seed)
        for part in range(6):
            cand = [int(r) for r in rng.permutation(150)] + [-3, 150]
            flags = [int(f) for f in rng.choice([0, 0, 0, 0, 0, 0, 1, 2], len(cand))]
            for sequential in (True, False):
                ref = cullref.keyframe_culling(m, cand, flags, 3, ratio, sequential)
                got = cpu_loop(exe, str(tmp_path / "d"), m, cand, flags, 3, ratio, sequential)
                for k in ("n_mps", "n_redundant", "decision", "kf_erased", "point_went_bad", "point_nobs", "erasures"):
                    assert got[k] == ref[k], (seed, part, sequential, k)
                erased += ref["erasures"]
            total += len(cand)
    assert total > 3000 and erased > 20


def test_the_cpp_loop_runs_clean_under_the_sanitizers(tmp_path):
    """tools/culling_cpu.cpp as a stand-alone program with -fsanitize=address,undefined and -Werror: the fixture, and a random map with erasures"""
    exe = build_cpu_loop(tmp_path, "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    fx = cullref.load_fixture()
    got = cpu_loop(exe, str(tmp_path / "fx"), fx["map"], fx["cand_row"], fx["cand_flags"], fx["th_obs"], fx["ratio"])
    for k, v in fx["sequential"].items():
        assert got[k] == v, k
    m = random_map(2, 80, 1200, lo=4, hi=9, levels=2)
    cand = list(range(80)) + [-1, 80, 2 ** 31 - 1]
    got = cpu_loop(exe, str(tmp_path / "rnd"), m, cand, None, 3, 0.6)
    ref = cullref.keyframe_culling(m, cand, None, 3, 0.6)
    assert got["decision"] == ref["decision"] and got["point_nobs"] == ref["point_nobs"] and ref["erasures"] > 0


def build_culling_driver(tmp_path, flags=("-Werror",)):
    return build_driver("culling_driver", tmp_path, "-Wall", *flags)


def driver_scenario(fx, path, monocular=0, max_culls=0):
    """the fixture as the scenario of tests/cpp/culling_driver.cpp (keyframe s is pool[s], so mnId == slot and slot 0 is the mnId == 0 keyframe) and the
    lines it must write: the fixture's hand-worked decisions and, for the map after SetBadFlag, the restatement"""
    m = fx["map"]
    n_kf = m["n_kf"]
    size = [1] * n_kf
    for r, kf in enumerate(m["row_kf"]):
        size[kf] = max(size[kf], len(m["rows"][r]))
    for p, o in enumerate(m["obs"]):
        for kf, idx in zip(o, m["obs_idx"][p]):
            size[kf] = max(size[kf], idx + 1)
    octave = [[None] * s for s in size]
    depth = [[0x3F800000] * s for s in size]
    stereo = [[0] * s for s in size]

    def put(kf, idx, lvl):
        assert octave[kf][idx] in (None, lvl), "the fixture gives one key two octaves"
        octave[kf][idx] = lvl
    for r, kf in enumerate(m["row_kf"]):
        for i, lvl in enumerate(m["row_level"][r]):
            if m["rows"][r][i] >= 0:
                put(kf, i, lvl)
            depth[kf][i] = m["row_depth_bits"][r][i]
    for p, o in enumerate(m["obs"]):
        for kf, idx, lvl, w in zip(o, m["obs_idx"][p], m["obs_level"][p], m["obs_w"][p]):
            put(kf, idx, lvl)
            stereo[kf][idx] = int(w == 2)
    flags = dict(zip(fx["cand_row"], fx["cand_flags"]))
    assert all(bool(f & 1) == (m["row_kf"][r] == 0) for r, f in flags.items())           # bit 0 is mnId == 0: the adapter finds it itself
    lines = ["pool %d" % n_kf]
    for kf in range(n_kf):
        keys = " ".join("%d %d %d" % (o or 0, d, s) for o, d, s in zip(octave[kf], depth[kf], stereo[kf]))
        not_erase = int(any(f & 2 and m["row_kf"][r] == kf for r, f in flags.items()))
        lines.append("kf %d %d %d %d %s" % (kf, not_erase, m["th_depth_bits"], size[kf], keys))
    for p, o in enumerate(m["obs"]):
        lines.append("point %d %d %d %s" % (p, m["point_bad"][p], len(o), " ".join("%d %d" % x for x in zip(o, m["obs_idx"][p]))))
    for r, kf in enumerate(m["row_kf"]):
        lines.append("row %d %d %s" % (kf, len(m["rows"][r]), " ".join(map(str, m["rows"][r]))))
    cand = [m["row_kf"][r] for r in fx["cand_row"]]
    lines.append("cull %d %d %d %s" % (monocular, max_culls, len(cand), " ".join(map(str, cand))))
    open(path, "w").write("\n".join(lines) + "\n")
    want = fx["monocular_sequential" if monocular else "sequential"]
    ref = cullref.keyframe_culling(dict(m, monocular=monocular), fx["cand_row"], fx["cand_flags"], fx["th_obs"], fx["ratio"])
    assert ref["decision"] == want["decision"]
    expect = ["cand %d %d %d %d" % (k, a, b, d) for k, a, b, d in zip(cand, want["n_mps"], want["n_redundant"], want["decision"])]
    erased = [k for k, d in zip(cand, want["decision"]) if d == 1]
    expect.append("erase" + "".join(" %d" % k for k in erased))
    expect.append("calls %d" % (max(1, -(-len(erased) // max_culls)) if max_culls else 1))
    bad = [int(b or w) for b, w in zip(m["point_bad"], ref["point_went_bad"])]
    # a bad point has an empty observation map in the reference and nObs keeps whatever it held when the point went bad: not compared
    return expect + ["point %d %d %s" % (p, bad[p], "*" if bad[p] else str(ref["point_nobs"][p])) for p in range(len(bad))]


def test_cpp_culling_mirror_compiles_never_falls_back_and_runs_clean_under_the_sanitizers(tmp_path):
    """ORB_SLAM2_PLF::KeyFrameCulling over tests/mock/ORB_SLAM2/mock_culling.h: built through tests/cppbuild.py with -Wall -Werror and
    -fsanitize=address,undefined as a stand-alone program.  Without a GPU it gathers the whole map on the host (the adapter's host path), then must stop
    with plf::Error(PLF_E_HIP) at its first device allocation; tests/test_gpu_culling_cpp.py runs it on the GPU against the fixture."""
    from conftest import gpu_available
    exe = build_culling_driver(tmp_path, flags=("-Werror", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    driver_scenario(cullref.load_fixture(), str(tmp_path / "scenario.txt"))
    run = subprocess.run([str(exe), str(tmp_path)], text=True, capture_output=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert "AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-3000:]
    if gpu_available():
        assert run.returncode == 0 and "culling driver ok" in run.stdout, run.stdout + run.stderr[-1000:]
    else:
        assert run.returncode == 1 and "plf error -4" in run.stdout, run.stdout + run.stderr[-1000:]


MPC_TABLE = [
    # found, visible, first, nobs, bad, want, what                         (cur = 10, cnThObs = 3)
    (1, 1, 10, 9, 1, 1, "isBad: dropped"),
    (1, 5, 10, 9, 0, 2, "found ratio 0.2 < 0.25"),
    (1, 4, 10, 9, 0, 0, "found ratio exactly 0.25: not below"),
    (24, 97, 10, 9, 0, 2, "24 / 97 rounds below 0.25f"),
    (0, 0, 9, 9, 0, 0, "visible == 0, found == 0: NaN, rule 2 does not fire; age 1: keep"),
    (0, 0, 8, 3, 0, 2, "NaN ratio, age 2, three observations: rule 3"),
    (0, 0, 7, 9, 0, 1, "NaN ratio, age 3: rule 4"),
    (3, 0, 9, 9, 0, 0, "visible == 0, found > 0: +inf, keep"),
    (-3, 0, 9, 9, 0, 2, "-inf is below 0.25"),
    (9, 9, 9, 0, 0, 0, "age 1: kept whatever the observations"),
    (9, 9, 8, 3, 0, 2, "age 2, Observations() == cnThObs"),
    (9, 9, 8, 4, 0, 0, "age 2, four observations: keep"),
    (9, 9, 7, 4, 0, 1, "age 3: dropped from the list"),
    (9, 9, 7, 3, 0, 2, "age 3, three observations: rule 3 comes first"),
    (9, 9, 10 + 2 ** 32, 0, 0, 0, "mnFirstKFid is narrowed to 32 bits: age 0"),
    (9, 9, 12, 0, 0, 0, "a negative age: keep"),
]


def test_map_point_culling_table():
    cols = list(zip(*MPC_TABLE))
    got = cullref.map_point_culling(cols[0], cols[1], cols[2], cols[3], cols[4], 10, 3)
    assert got == list(cols[5]), [(g, row[5], row[6]) for g, row in zip(got, MPC_TABLE) if g != row[5]]
    mono = cullref.map_point_culling([9, 9], [9, 9], [8, 8], [3, 2], None, 10, 2)           # cnThObs = 2 when monocular
    assert mono == [0, 2]


def test_symbols_are_exported_and_reject_bad_arguments_without_a_device():
    import rgbd_pl_slam_amd
    from rgbd_pl_slam_amd import _lib as L
    for name in ("keyframe_culling", "map_point_culling", "CullMap", "culling"):
        assert hasattr(rgbd_pl_slam_amd, name), name
    lib = L.cull_prototypes(L.lib())
    buf = np.zeros(16, np.int64)
    ptr = buf.ctypes.data                                     # a non-NULL address: the checks must not touch it

    def call(mode=L.CULL_SEQUENTIAL, th_obs=3, max_culls=0, force=0, n_cand=1, outs=None, device=0, **fields):
        v = L.CullView(n_rows=1, row_start=ptr, row_point=ptr, row_kf=ptr, n_points=1, obs_start=ptr, obs_kf=ptr, n_kf=1, row_level=ptr, obs_level=ptr,
                       row_depth=ptr, th_depth=3.0, monocular=0)
        for k, val in fields.items():
            setattr(v, k, val)
        p = L.CullParams(mode, th_obs, max_culls, force, 0.9)
        o = outs or [ptr, ptr, n_cand, ptr, ptr, ptr, ptr, ptr, ptr, ptr]
        return lib.plf_keyframe_culling(C.byref(v), C.byref(p), *o, device, None)

    from conftest import gpu_available
    if not gpu_available():
        assert call() == L.PLF_E_HIP                          # a well-formed call gets as far as the device, and no further
        assert call(monocular=1, row_depth=None) == L.PLF_E_HIP
        assert call(row_level=None, obs_level=None, kf_keys=ptr, obs_idx=ptr, row_depth=None, kf_depth=ptr) == L.PLF_E_HIP
    assert lib.plf_keyframe_culling(None, None, ptr, ptr, 1, ptr, ptr, ptr, ptr, ptr, ptr, ptr, 0, None) == L.PLF_E_BADARG
    for required in ("row_start", "row_point", "row_kf", "obs_start", "obs_kf"):
        assert call(**{required: None}) == L.PLF_E_BADARG, required
    for size in ("n_rows", "n_points", "n_kf"):
        assert call(**{size: -1}) == L.PLF_E_BADARG, size
    assert call(n_cand=-1) == L.PLF_E_BADARG
    assert call(kf_keys=ptr, obs_idx=ptr) == L.PLF_E_BADARG                               # both level forms
    assert call(row_level=None, obs_level=None) == L.PLF_E_BADARG                         # neither
    assert call(obs_level=None) == L.PLF_E_BADARG and call(row_level=None) == L.PLF_E_BADARG   # half of the packed form
    assert call(row_level=None, obs_level=None, kf_keys=ptr) == L.PLF_E_BADARG            # the indirect form without obs_idx
    assert call(row_depth=None) == L.PLF_E_BADARG                                         # depths missing while monocular == 0
    assert call(kf_depth=ptr) == L.PLF_E_BADARG                                           # both depth forms
    assert call(mode=2) == L.PLF_E_BADARG and call(mode=-1) == L.PLF_E_BADARG
    assert call(th_obs=-1) == L.PLF_E_BADARG and call(max_culls=-1) == L.PLF_E_BADARG
    assert call(force=4) == L.PLF_E_BADARG and call(force=-1) == L.PLF_E_BADARG
    assert call(device=-1) == L.PLF_E_BADARG
    for missing in (0, 3, 4, 5, 6, 9):                                                    # cand_row, n_mps, n_redundant, decision, kf_erased, status
        o = [ptr, ptr, 1, ptr, ptr, ptr, ptr, ptr, ptr, ptr]
        o[missing] = None
        assert call(outs=o) == L.PLF_E_BADARG, missing

    def points(n=1, found=ptr, visible=ptr, first=ptr, nobs=ptr, obs_start=None, obs_kf=None, n_kf=0, decision=ptr, device=0):
        return lib.plf_map_point_culling(n, found, visible, first, nobs, obs_start, obs_kf, None, n_kf, None, 10, 3, decision, device, None)

    if not gpu_available():
        assert points() == L.PLF_E_HIP and points(nobs=None, obs_start=ptr, obs_kf=ptr) == L.PLF_E_HIP
    assert points(n=0) == L.PLF_OK
    assert points(n=-1) == L.PLF_E_BADARG and points(n_kf=-1) == L.PLF_E_BADARG and points(device=-1) == L.PLF_E_BADARG
    for k in ("found", "visible", "first", "decision"):
        assert points(**{k: None}) == L.PLF_E_BADARG, k
    assert points(nobs=None) == L.PLF_E_BADARG and points(nobs=None, obs_start=ptr) == L.PLF_E_BADARG

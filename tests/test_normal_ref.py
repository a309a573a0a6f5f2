"""UpdateNormalAndDepth, CPU side: the numpy restatement (tests/normref.py) against the hand-worked fixture, against the independently written
C++ loop (tools/normal_depth_cpu.cpp) and against its own properties, the C ABI of the new entry point, and the C++ adapter against the mocks.
No GPU needed: the argument checks run before any device work.  Every comparison is bit for bit (float32 viewed as uint32; two NaNs at the same
position count as equal)."""
import ctypes as C
import os
import subprocess

import numpy as np

import normref as R
from conftest import gpu_available
from cppbuild import build_driver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "normal_depth_tiny.json")
F = np.float32


def build_normal_driver(tmp_path, flags=("-Werror",)):
    return build_driver("normal_driver", tmp_path, "-Wall", *flags)


def driver_scenario(fx, path):
    """the fixture as the driver's scenario (keyframe slot s lives at pool[s]: addresses ascend with the slot, the order the fixture lists observations
    in) and the lines it must write, taken from the fixture's expected values"""
    hx = lambda a: " ".join("%08x" % int(v) for v in np.atleast_1d(np.asarray(a, F)).view(np.uint32))
    lines = ["pool %d" % len(fx["kf_ow"]), "scale %d %s" % (len(fx["scale_arr"]), hx(fx["scale_arr"]))]
    for s, (ow, octs) in enumerate(zip(fx["kf_ow_arr"], fx["kf_octaves"])):
        lines.append("kf %d %s %d %s" % (s, hx(ow), len(octs), " ".join(map(str, octs))))
    expect = []
    for c in fx["cases"]:
        assert [o[0] for o in c["obs"]] == sorted(o[0] for o in c["obs"])
        lines.append("point %s %d %d %d %s" % (hx(c["pos_arr"]), c["bad"], c["ref_kf"], len(c["obs"]), " ".join("%d %d" % tuple(o) for o in c["obs"])))
        nan = lambda h: "nan" if h == "7fc00000" else h
        expect.append("-1" if c["n"] < 0 else "%d %s %s %s" % (c["n"], " ".join(nan(h) for h in c["normal"]), nan(c["min"]), nan(c["max"])))
    lines.append("run")
    open(path, "w").write("\n".join(lines) + "\n")
    return expect


def build_cpu_loop(tmp_path):
    exe = tmp_path / "normal_depth_cpu"
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "tools", "normal_depth_cpu.cpp"), "-o", str(exe)])
    return exe


def run_cpu_loop(exe, d, m, scale, bad=None, pos_floats=3, reps=1):
    """tools/normal_depth_cpu.cpp on a map of normref.make_map's layout: (normal, min, max, n)"""
    for name, arr in (("obs_start.i32", m["obs_start"]), ("obs_kf.i32", m["obs_kf"]), ("ref_kf.i32", m["ref_kf"]), ("level.i32", m["level"])):
        np.asarray(arr, np.int32).tofile(str(d / name))
    for name, arr in (("kf_ow.f32", m["kf_ow"]), ("scale.f32", scale), ("world_pos.f32", m["world_pos"])):
        np.asarray(arr, F).tofile(str(d / name))
    if bad is not None:
        np.asarray(bad, np.uint8).tofile(str(d / "bad.u8"))
    out = subprocess.check_output([str(exe), str(d), str(reps), str(pos_floats)], text=True)
    n = len(m["obs_start"]) - 1
    return (np.fromfile(str(d / "normal.f32"), F).reshape(n, 3), np.fromfile(str(d / "min.f32"), F), np.fromfile(str(d / "max.f32"), F),
            np.fromfile(str(d / "n.i32"), np.int32), float(out.split()[1]))


def sentinel(shape):
    return np.full(shape, R.SENTINEL, np.uint32).view(F)


def test_restatement_equals_the_hand_worked_fixture():
    fx = R.load_fixture(FIXTURE)
    names = [c["name"] for c in fx["cases"]]
    assert names == ["one_observation", "two_terms_cancel_to_plus_zero", "alpha_is_rounded_before_the_multiply", "negative_zero_product_becomes_plus_zero",
                     "reference_keyframe_not_observed", "bad_point", "empty_point", "point_on_a_camera_centre"]
    a = R.fixture_arrays(fx)
    live = np.array([c["n"] >= 0 for c in fx["cases"]])
    assert np.array_equal(R.ref_levels(a["obs_start"], a["obs_kf"], a["obs_idx"], a["ref_kf"], a["kf_octaves"])[live], a["level"][live])
    n = len(names)
    nrm, mn, mx, used = R.update_all(a["obs_start"], a["obs_kf"], a["kf_ow"], a["ref_kf"], a["level"], a["scale"], a["world_pos"], sentinel((n, 3)), sentinel(n),
                                      sentinel(n), point_bad=a["point_bad"])
    for i, c in enumerate(fx["cases"]):
        assert used[i] == c["n"], c["name"]
        if c["n"] < 0:
            assert (R.bits(nrm[i]) == R.SENTINEL).all() and R.bits(mn[i]) == R.SENTINEL and R.bits(mx[i]) == R.SENTINEL, c["name"]
            continue
        assert R.same_bits(nrm[i], c["normal_arr"]) and R.same_bits(mn[i], c["min_f"]) and R.same_bits(mx[i], c["max_f"]), c["name"]
        ks = [o[0] for o in c["obs"]]
        one = R.update_one(c["pos_arr"], a["kf_ow"][ks], a["kf_ow"][c["ref_kf"]], c["level"], a["scale"])
        assert R.same_bits(one[0], c["normal_arr"]) and R.same_bits(one[1], c["min_f"]) and R.same_bits(one[2], c["max_f"]), c["name"]
        assert R.same_bits(R.natural_one(c["pos_arr"], a["kf_ow"][ks]), c["natural_normal_arr"]), c["name"]
    by = {c["name"]: c for c in fx["cases"]}
    # the values one follows on paper
    assert by["one_observation"]["normal_arr"].tolist() == [0.0, 0.0, 1.0] and by["one_observation"]["max_f"] == F(4.0) * a["scale"][2]
    assert R.bits(by["two_terms_cancel_to_plus_zero"]["normal_arr"]).tolist() == [0, 0, 0]
    assert by["reference_keyframe_not_observed"]["level"] == 5 and by["reference_keyframe_not_observed"]["max_f"] == F(5.0) * a["scale"][5]
    assert np.isnan(by["point_on_a_camera_centre"]["normal_arr"]).all() and by["point_on_a_camera_centre"]["max_f"] == 0
    # the fixture pins the rule: the natural formula gives other bits in exactly these two cases
    c = by["alpha_is_rounded_before_the_multiply"]
    assert not R.same_bits(c["normal_arr"], c["natural_normal_arr"])
    assert np.abs(R.bits(c["normal_arr"]).astype(np.int64) - R.bits(c["natural_normal_arr"]).astype(np.int64)).max() == 1       # the last bit
    c = by["negative_zero_product_becomes_plus_zero"]
    assert R.bits(c["normal_arr"])[0] == 0 and R.bits(c["natural_normal_arr"])[0] == 0x80000000


def test_vectorised_restatement_equals_the_literal_one():
    rng = np.random.default_rng(11)
    counts = R.long_tailed_counts(rng, 1500)
    counts[:4] = [0, 1, 2, 300]
    m = R.make_map(12, counts, 700, subnormal_share=0.02)
    sf = R.scale_factors()
    n = len(counts)
    nrm, mn, mx, used = R.update_all(m["obs_start"], m["obs_kf"], m["kf_ow"], m["ref_kf"], m["level"], sf, m["world_pos"], sentinel((n, 3)), sentinel(n), sentinel(n))
    for p in range(n):
        s, e = int(m["obs_start"][p]), int(m["obs_start"][p + 1])
        if s == e:
            assert used[p] == -1 and (R.bits(nrm[p]) == R.SENTINEL).all()
            continue
        one = R.update_one(m["world_pos"][p], m["kf_ow"][m["obs_kf"][s:e]], m["kf_ow"][m["ref_kf"][p]], m["level"][p], sf)
        assert used[p] == e - s and R.same_bits(one[0], nrm[p]) and R.same_bits(one[1], mn[p]) and R.same_bits(one[2], mx[p]), p


def test_two_restatements_agree_on_20000_random_points(tmp_path):
    """normref against the compiled tools/normal_depth_cpu.cpp: coordinates from 1e-3 to 1e4, subnormal differences, a few bad points, levels out of
    range, observations whose keyframe is outside the table"""
    exe = build_cpu_loop(tmp_path)
    rng = np.random.default_rng(21)
    n = 20000
    counts = R.long_tailed_counts(rng, n)
    counts[rng.random(n) < 0.01] = 0
    m = R.make_map(22, counts, 1000, spread=(1e-3, 1e4), subnormal_share=0.005)
    sub = np.flatnonzero(np.abs(m["world_pos"][:, 0]) < 1e-38)
    assert len(sub) > 20                                                            # the subnormal differences are really there
    m["level"][rng.random(n) < 0.01] = 9; m["level"][rng.random(n) < 0.01] = -2
    m["obs_kf"][rng.random(len(m["obs_kf"])) < 0.01] = 1000
    m["obs_kf"][rng.random(len(m["obs_kf"])) < 0.005] = -1
    m["ref_kf"][:3] = [-1, 1000, 5]
    bad = (rng.random(n) < 0.01).astype(np.uint8)
    sf = R.scale_factors()
    ref = R.update_all(m["obs_start"], m["obs_kf"], m["kf_ow"], m["ref_kf"], m["level"], sf, m["world_pos"], sentinel((n, 3)), sentinel(n), sentinel(n), point_bad=bad)
    got = run_cpu_loop(exe, tmp_path, m, sf, bad)
    assert np.array_equal(got[3], ref[3]) and (ref[3] == -1).sum() > 300
    assert R.same_bits(got[0], ref[0]) and R.same_bits(got[1], ref[1]) and R.same_bits(got[2], ref[2])
    # and the line rule: the same routine at the midpoint
    seg = np.concatenate([m["world_pos"], R.make_map(23, counts, 1000)["world_pos"]], axis=1)
    ml = dict(m, world_pos=seg)
    ref = R.update_all(m["obs_start"], m["obs_kf"], m["kf_ow"], m["ref_kf"], m["level"], sf, seg, sentinel((n, 3)), sentinel(n), sentinel(n), point_bad=bad)
    got = run_cpu_loop(exe, tmp_path, ml, sf, bad, pos_floats=6)
    assert np.array_equal(got[3], ref[3]) and R.same_bits(got[0], ref[0]) and R.same_bits(got[1], ref[1]) and R.same_bits(got[2], ref[2])


def test_the_sum_depends_on_the_order_of_the_observations():
    """a restatement that silently summed in double (or as a tree) would be order-free at float precision far more often than this"""
    rng = np.random.default_rng(31)
    n = 1000
    counts = rng.integers(3, 40, n)
    m = R.make_map(32, counts, 500, spread=(1e-1, 1e2))
    sf = R.scale_factors()
    z3, z1 = np.zeros((n, 3), F), np.zeros(n, F)
    a = R.update_all(m["obs_start"], m["obs_kf"], m["kf_ow"], m["ref_kf"], m["level"], sf, m["world_pos"], z3, z1, z1)
    kf2 = m["obs_kf"].copy()
    for p in range(n):
        s, e = int(m["obs_start"][p]), int(m["obs_start"][p + 1])
        kf2[s:e] = kf2[s:e][rng.permutation(e - s)]
    b = R.update_all(m["obs_start"], kf2, m["kf_ow"], m["ref_kf"], m["level"], sf, m["world_pos"], z3, z1, z1)
    changed = (R.bits(a[0]) != R.bits(b[0])).any(axis=1)
    assert changed.sum() >= 1
    assert changed.sum() > 100                                         # in fact for a large share of them
    assert R.same_bits(a[1], b[1]) and R.same_bits(a[2], b[2])          # the distances do not see the order
    assert np.abs(a[0].astype(np.float64) - b[0].astype(np.float64)).max() < 1e-5


def test_abi_declares_and_exports_the_entry_point():
    """fails on a tree without the feature: plf.h has to declare plf_map_update_normal_depth and the cross-compiled library has to export it"""
    hdr = open(os.path.join(ROOT, "include", "plf.h")).read()
    assert "int plf_map_update_normal_depth(const plf_map_geom_view *v" in hdr and "} plf_map_geom_view;" in hdr and "so@0x924e0" in hdr
    from rgbd_pl_slam_amd import _lib as L
    lib = L.mapgeom_prototypes(L.lib())
    assert hasattr(lib, "plf_map_update_normal_depth")
    import rgbd_pl_slam_amd as pkg
    assert callable(pkg.update_normal_and_depth) and pkg.MapPoint.UpdateNormalAndDepth is pkg.update_normal_and_depth
    assert pkg.MapLine.UpdateAverageDir is pkg.update_normal_and_depth and callable(pkg.kf_keys_table)


def badarg_calls(L, lib, a=0x1000, normal=None, dmin=None, dmax=None, used=None):
    """every misuse include/plf.h names, as (label, status); the arrays are never dereferenced when the call is refused on the host.  Shared with the GPU
    test, which passes real output arrays and checks that they keep their sentinels."""
    normal, dmin, dmax, used = normal or a, dmin or a, dmax or a, used or a
    call = lambda v, wp=a, nv=normal, mn=dmin, mx=dmax, rows=4, nu=used: lib.plf_map_update_normal_depth(C.byref(v) if v is not None else None, wp, nv, mn, mx, rows, nu, 0, None)
    base = dict(n_points=4, obs_start=a, obs_kf=a, kf_ow=a, n_kf=2, ref_kf=a, ref_level=a, scale_factors=a, nlevels=8, pos_floats=3)
    mk = lambda **kw: L.MapGeomView(**{**base, **kw})
    out = [("null view", call(None)), ("null world_pos", call(mk(), wp=None)), ("null normal", call(mk(), nv=None)), ("null n_obs_used", call(mk(), nu=None))]
    for f in ("obs_start", "obs_kf", "kf_ow", "ref_kf"):
        out.append(("null " + f, call(mk(**{f: None}))))
    out += [("n_points < 0", call(mk(n_points=-1))), ("n_kf < 0", call(mk(n_kf=-1))), ("map_rows < 0", call(mk(), rows=-1)),
            ("neither level form", call(mk(ref_level=None))), ("both level forms", call(mk(kf_keys=a, obs_idx=a))),
            ("indirect without obs_idx", call(mk(ref_level=None, kf_keys=a))),
            ("pos_floats 0", call(mk(pos_floats=0))), ("pos_floats 4", call(mk(pos_floats=4))),
            ("indirect with lines", call(mk(ref_level=None, kf_keys=a, obs_idx=a, pos_floats=6))),
            ("min without max", call(mk(), mx=None)), ("max without min", call(mk(), mn=None)),
            ("distances without scale factors", call(mk(scale_factors=None))), ("nlevels 0", call(mk(nlevels=0)))]
    return out, call, mk


def test_misuse_is_refused_before_any_device_work():
    from rgbd_pl_slam_amd import _lib as L
    lib = L.mapgeom_prototypes(L.lib())
    out, call, mk = badarg_calls(L, lib)
    assert len(out) == 21
    for label, st in out:
        assert st == L.PLF_E_BADARG, label
    assert call(mk(n_points=0)) == L.PLF_OK                                                       # nothing to do: no device needed
    if not gpu_available():
        assert call(mk()) == L.PLF_E_HIP                                                          # a well-formed call: never a CPU path


def test_cpp_adapter_compiles_against_the_mocks_and_never_falls_back(tmp_path):
    """plf::MapPoint::UpdateNormalAndDepth / plf::MapLine::UpdateAverageDir and the ORB_SLAM2_PLF adapter over tests/mock/ORB_SLAM2/mock_normal.h, driven by
    tests/cpp/normal_driver.cpp"""
    exe = build_normal_driver(tmp_path)
    expect = driver_scenario(R.load_fixture(FIXTURE), str(tmp_path / "scenario.txt"))
    assert len(expect) == 8
    run = subprocess.run([str(exe), str(tmp_path)], text=True, capture_output=True)
    if gpu_available():
        assert run.returncode == 0 and "normal driver ok" in run.stdout, run.stdout + run.stderr[-1000:]
    else:
        assert run.returncode == 1 and "plf error -4" in run.stdout, run.stdout + run.stderr[-1000:]

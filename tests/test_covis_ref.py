"""Covisibility graph, CPU side: the restatement (tests/covisref.py) against a hand-worked fixture, th = 1 against an independent "order
everything", and the argument checks of plf_covis_count / plf_covis_by_weight, which run before any device work.  No GPU needed."""
import ctypes as C
import json
import os

import numpy as np

import covisref
from cppbuild import build_driver

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_fixture():
    return json.load(open(os.path.join(GOLD, "covis_tiny.json")))


def _plain(res):
    return None if res is None else {k: ([list(x) for x in v] if k != "max" else list(v)) for k, v in res.items()}


def test_restatement_equals_the_hand_worked_fixture():
    fx = load_fixture()
    obs, n_kf, bad = fx["obs"], fx["n_kf"], fx["point_bad"]
    for name, key in (("connections_with_keys", fx["kf_key"]), ("connections_with_slots", None)):
        got = [_plain(covisref.update_connections(row, s, obs, n_kf, fx["th"], bad, key)) for s, row in enumerate(fx["rows"])]
        assert got == fx[name], name
    v = fx["votes"]
    for name, key in (("with_keys", fx["kf_key"]), ("with_slots", None)):
        got = [_plain(covisref.local_keyframe_votes(row, obs, n_kf, bad, v["kf_bad"], key)) for row in v["rows"]]
        assert got == v[name], name
    row0 = covisref.update_connections(fx["rows"][0], 0, obs, n_kf, fx["th"], bad, fx["kf_key"])
    b = fx["best_covisibility"]
    assert covisref.best_covisibility(row0["ord"], b["N"]) == b["with_keys"]
    for case in fx["by_weight"]["cases_with_keys"]:
        assert covisref.covisibles_by_weight(row0["ord"], case["w"]) == case["result"], case["what"]
    assert covisref.covisibles_by_weight([], 1) == []
    assert [list(x) for x in covisref.update_connections(fx["rows"][0], 0, obs, n_kf, 1, bad, fx["kf_key"])["ord"]] == fx["row0_with_keys_th1"]


def test_every_special_case_is_really_in_the_fixture():
    fx = load_fixture()
    sp, rows, obs, key = fx["special"], fx["rows"], fx["obs"], fx["kf_key"]
    keyed, slotted = fx["connections_with_keys"], fx["connections_with_slots"]
    r = sp["row_with_14_15_15_16"]
    assert sorted(w for _, w in keyed[r]["conn"]) == [14, 15, 15, 16]                      # neighbours at 14, 15 and 16
    a, b = sp["tied_at_15"]
    assert dict(map(tuple, keyed[r]["conn"]))[a] == dict(map(tuple, keyed[r]["conn"]))[b] == 15
    assert (a < b) != (key[a] < key[b])                                                     # key order is the reverse of slot order
    assert [k for k, _ in keyed[r]["ord"]] != [k for k, _ in slotted[r]["ord"]]             # ... and it decides the ordered list
    assert all(r in obs[p] for p in rows[r] if 0 <= p < len(obs))                           # the row's own observations
    assert fx["point_bad"][sp["bad_point"]] == 1 and sp["bad_point"] in rows[sp["bad_point_in_row"]]
    without = list(fx["point_bad"]); without[sp["bad_point"]] = 0                           # ... and the bad point would have counted
    assert _plain(covisref.update_connections(rows[r], r, obs, fx["n_kf"], 15, without, key)) != keyed[r]
    assert -1 in rows[sp["null_in_row"]]
    tr, tp = sp["twice_in_row"]
    assert rows[tr].count(tp) == 2
    once = list(rows[tr]); once.remove(tp)
    assert _plain(covisref.update_connections(once, tr, obs, fx["n_kf"], 15, fx["point_bad"], key)) != keyed[tr]   # the second listing counts
    assert keyed[sp["row_without_neighbour"]] is None and len(rows[sp["row_without_neighbour"]]) > 0
    lo = sp["row_below_th_with_tied_max"]
    top = max(w for _, w in keyed[lo]["conn"])
    assert top < fx["th"] and sorted(k for k, w in keyed[lo]["conn"] if w == top) == sp["tied_max"]
    assert len(keyed[lo]["ord"]) == 1 and keyed[lo]["max"] != slotted[lo]["max"]            # the first maximum in key order wins
    v = fx["votes"]
    c0 = {int(k): w for k, w in v["counter_row0"].items()}
    leader = max(c0, key=c0.get)
    assert v["kf_bad"][leader] == 1 and leader not in [k for k, _ in v["with_keys"][0]["conn"]]   # the bad keyframe holds the highest count
    assert v["with_keys"][0]["max"][1] < c0[leader]
    assert v["with_keys"][2] is None
    weights = [w for _, w in keyed[fx["by_weight"]["row"]]["ord"]]
    ws = [c["w"] for c in fx["by_weight"]["cases_with_keys"]]
    assert any(w <= min(weights) for w in ws) and any(min(weights) < w <= max(weights) for w in ws) and any(w > max(weights) for w in ws)


def _world(seed, n_kf=30, n_points=400):
    rng = np.random.default_rng(seed)
    obs = [[int(k) for k in rng.choice(n_kf, int(rng.integers(1, 9)), replace=False)] for _ in range(n_points)]
    rows = [[p for p in range(n_points) if s in obs[p]] + [-1] for s in range(n_kf)]
    bad = [int(x) for x in rng.integers(0, 10, n_points) == 0]
    key = [int(k) for k in rng.permutation(n_kf) * 7 + 3]
    return obs, rows, bad, key


def test_th_1_is_the_independent_order_everything():
    for seed in range(3):
        obs, rows, bad, key = _world(seed)
        for k in (None, key):
            for s, row in enumerate(rows):
                res = covisref.update_connections(row, s, obs, len(rows), 1, bad, k)
                every = covisref.order_everything(row, s, obs, len(rows), bad, k)
                assert (res["ord"] if res else []) == every
                if res:
                    assert sorted(res["conn"]) == sorted(every) and res["ord"][0][1] == res["max"][1]
                    high = covisref.update_connections(row, s, obs, len(rows), 15, bad, k)
                    assert high["ord"] == ([e for e in every if e[1] >= 15] or [high["max"]])


def test_symbols_are_exported_and_reject_bad_arguments_without_a_device():
    import rgbd_pl_slam_amd
    from rgbd_pl_slam_amd import _lib as L
    for name in ("update_connections", "local_keyframe_votes", "Covisibility", "covisibility"):
        assert hasattr(rgbd_pl_slam_amd, name), name
    lib = L.covis_prototypes(L.lib())
    buf = np.zeros(16, np.int64)
    ptr = buf.ctypes.data                                     # a non-NULL address: the checks must not touch it

    def call(mode=L.COVIS_CONNECTIONS, th=15, stride=4, dense=0, table=0, ord_=True, **fields):
        v = L.CovisView(n_rows=1, row_start=ptr, row_point=ptr, row_self=ptr if mode == L.COVIS_CONNECTIONS else None, n_points=1, obs_start=ptr, obs_kf=ptr,
                        n_kf=1)
        for k, val in fields.items():
            setattr(v, k, val)
        p = L.CovisParams(mode, th, stride, dense, table)
        o = ptr if ord_ else None
        return lib.plf_covis_count(C.byref(v), C.byref(p), ptr, ptr, ptr, o, o, o, ptr, ptr, 0, None)

    from conftest import gpu_available
    if not gpu_available():
        assert call() == L.PLF_E_HIP                          # a well-formed call gets as far as the device, and no further
    assert lib.plf_covis_count(None, None, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, 0, None) == L.PLF_E_BADARG
    for required in ("row_start", "row_point", "obs_start", "obs_kf"):
        assert call(**{required: None}) == L.PLF_E_BADARG, required
    for size in ("n_rows", "n_points", "n_kf"):
        assert call(**{size: -1}) == L.PLF_E_BADARG, size
    assert call(stride=0) == L.PLF_E_BADARG and call(th=0) == L.PLF_E_BADARG and call(mode=2) == L.PLF_E_BADARG
    assert call(dense=-1) == L.PLF_E_BADARG and call(table=-1) == L.PLF_E_BADARG
    assert call(mode=L.COVIS_VOTES, row_self=ptr) == L.PLF_E_BADARG          # row_self in votes mode
    assert call(ord_=False) == L.PLF_E_BADARG                                # ord_* missing in connections mode
    v = L.CovisView(n_rows=1, row_start=ptr, row_point=ptr, n_points=1, obs_start=ptr, obs_kf=ptr, n_kf=1)
    p = L.CovisParams(L.COVIS_CONNECTIONS, 15, 4, 0, 0)
    for missing in range(2, 10):                                              # every output but the three ord_* (checked above)
        args = [ptr] * 8
        args[missing - 2] = None
        assert lib.plf_covis_count(C.byref(v), C.byref(p), *args, 0, None) == L.PLF_E_BADARG, missing
    assert lib.plf_covis_count(C.byref(v), C.byref(p), *([ptr] * 8), -1, None) == L.PLF_E_BADARG
    assert lib.plf_covis_by_weight(None, ptr, 1, 4, 15, ptr, 0, None) == L.PLF_E_BADARG
    assert lib.plf_covis_by_weight(ptr, None, 1, 4, 15, ptr, 0, None) == L.PLF_E_BADARG
    assert lib.plf_covis_by_weight(ptr, ptr, 1, 4, 15, None, 0, None) == L.PLF_E_BADARG
    assert lib.plf_covis_by_weight(ptr, ptr, -1, 4, 15, ptr, 0, None) == L.PLF_E_BADARG
    assert lib.plf_covis_by_weight(ptr, ptr, 1, 0, 15, ptr, 0, None) == L.PLF_E_BADARG


def build_covis_driver(tmp_path, flags=("-Werror",)):
    return build_driver("covis_driver", tmp_path, "-Wall", *flags)


def driver_scenario(fx, path):
    """the fixture as the driver's scenario (keyframe s lives at pool[rank of its key]: its address is its key) and the lines it must write, taken from
    the fixture's hand-worked lists and, for the queries, from the restatement"""
    n_kf, obs, rows, key, v = fx["n_kf"], fx["obs"], fx["rows"], fx["kf_key"], fx["votes"]
    pos = {s: sorted(key).index(key[s]) for s in range(n_kf)}
    lines = ["pool %d" % n_kf] + ["kf %d %d %d" % (s, pos[s], v["kf_bad"][s]) for s in range(n_kf)]
    for p, o in enumerate(obs):
        o = [k for k in o if 0 <= k < n_kf]                                   # a pointer model has no observer outside the table
        lines.append("point %d %d %d %s" % (p, fx["point_bad"][p], len(o), " ".join(map(str, o))))
    null = lambda row: [p if 0 <= p < len(obs) else -1 for p in row]          # noqa: E731
    lines += ["row %d %d %s" % (s, len(r), " ".join(map(str, null(r)))) for s, r in enumerate(rows)]
    lines += ["frame %d %s" % (len(r), " ".join(map(str, null(r)))) for r in v["rows"]]
    expect = []
    lines.append("update %d" % fx["th"])
    want = fx["connections_with_keys"]
    for s, e in enumerate(want):
        pairs = lambda lst: "".join("%d:%d " % (k, w) for k, w in lst)        # noqa: E731
        expect.append("kf %d conn %sord %sparent %d" % (s, pairs(e["conn"]) if e else "", pairs(e["ord"]) if e else "", e["ord"][0][0] if e else -1))
    ids = lambda lst: "".join("%d " % k for k in lst)                         # noqa: E731
    for s, e in enumerate(want):
        ordered = [tuple(x) for x in e["ord"]] if e else []
        lines.append("connected %d" % s); expect.append(ids(k for k, _ in e["conn"]) if e else "")
        for N in (0, 1, 2, 10):
            lines.append("best %d %d" % (s, N)); expect.append(ids(covisref.best_covisibility(ordered, N)))
        for w in (10, 13, 15, 16, 17):
            lines.append("byweight %d %d" % (s, w)); expect.append(ids(covisref.covisibles_by_weight(ordered, w)))
    lines.append("weight 0 4"); expect.append("14")
    lines.append("weight 5 0"); expect.append("0")
    for f, e in enumerate(v["with_keys"]):
        lines.append("votes %d" % f)
        expect.append(("".join("%d:%d " % (k, w) for k, w in e["conn"]) if e else "") + ("max %d %d" % tuple(e["max"]) if e else "max -1 0"))
    open(path, "w").write("\n".join(lines) + "\n")
    return expect


def test_cpp_covisibility_mirror_compiles_and_never_falls_back(tmp_path):
    """ORB_SLAM2_PLF::CovisibilityGraph over tests/mock/ORB_SLAM2/mock_covis.h: built here with -Werror; without a GPU the driver must stop with
    plf::Error(PLF_E_HIP) at its first device allocation (tests/test_gpu_cpp_drivers.py runs it on the GPU against the fixture)"""
    import subprocess
    from conftest import gpu_available
    exe = build_covis_driver(tmp_path)
    expect = driver_scenario(load_fixture(), str(tmp_path / "scenario.txt"))
    run = subprocess.run([str(exe), str(tmp_path)], text=True, capture_output=True)
    if gpu_available():
        assert run.returncode == 0 and "covis driver ok" in run.stdout, run.stdout + run.stderr[-1000:]
        assert open(str(tmp_path / "out.txt")).read().split("\n")[:-1] == expect
    else:
        assert run.returncode == 1 and "plf error -4" in run.stdout, run.stdout

"""detail::MapGather and detail::ref_level of include/plf.hpp -- the one host walk under the row adapters (covisibility, culling, local map, CorrectLoop) --
checked completely without a GPU: tests/cpp/gather_host.cpp gathers a fixed map in the four registration orders under -fsanitize=address,undefined and
prints the map and every array; here the map is checked to hold every case the walk can go wrong on, and the arrays are recomputed from it by the
first-appearance rule.  A wrong index in a gathered array is an out-of-range read on the device: this is where it has to be caught."""
import subprocess

import numpy as np
import pytest

import cppbuild


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    exe = cppbuild.build_driver("gather_host", tmp_path_factory.mktemp("gather"), "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                                "-fno-sanitize-recover=all")
    run = subprocess.run([str(exe)], text=True, capture_output=True)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-3000:]          # no sanitizer complaint
    out = {}
    for ln in run.stdout.splitlines():
        out.setdefault(ln.split()[0], []).append(ln.split()[1:])
    return out


def _map(printed):
    """rows[k]: point ids, -1 = null; octave[k]; kf_id[k]; bad[p]; ref[p] (-1: none); obs[p]: {keyframe: index}"""
    m = dict(rows={}, octave={}, kf_id={}, bad={}, ref={}, obs={})
    for w in printed["map.row"]:
        m["rows"][int(w[0])] = [int(x) for x in w[1:]]
    for w in printed["map.octave"]:
        m["octave"][int(w[0])] = [int(x) for x in w[1:]]
    for w in printed["map.id"]:
        m["kf_id"][int(w[0])] = int(w[1])
    for w in printed["map.point"]:
        p = int(w[0])
        m["bad"][p], m["ref"][p] = int(w[1]), int(w[2])
        m["obs"][p] = {int(o.split(":")[0]): int(o.split(":")[1]) for o in w[3:]}
    return m


def _ints(printed, name):
    (w,) = printed[name]
    return [int(x) for x in w]


class Gather:
    """the rule: a keyframe's slot and a point's id are its rank of first appearance; a point's observations are appended once, when it gets its id, in the
    order of a std::map<KeyFrame*, size_t> (the keyframes are one array: by number); a null entry of a row is -1"""

    def __init__(self, m, with_ref=False):                          # with_ref: CorrectLoop's extra, which takes a slot for the reference keyframe
        self.m, self.with_ref, self.kfs, self.pts = m, with_ref, [], []
        self.row_start, self.row_point, self.obs_start, self.obs_kf, self.point_bad = [0], [], [0], [], []
        self.obs_idx, self.obs_level, self.n_obs, self.ref, self.level = [], [], [], [], []

    def slot(self, k):
        if k not in self.kfs:
            self.kfs.append(k)
        return self.kfs.index(k)

    def point(self, p, with_obs=True):
        if p not in self.pts:
            self.pts.append(p)
            self.point_bad.append(self.m["bad"][p])
            if with_obs:
                obs, ref = self.m["obs"][p], self.m["ref"][p]
                for k in sorted(obs):
                    self.obs_kf.append(self.slot(k))
                    self.obs_idx.append(obs[k])
                    self.obs_level.append(self.m["octave"][k][obs[k]] if obs[k] < len(self.m["octave"][k]) else 0)
                self.obs_start.append(len(self.obs_kf))
                self.n_obs.append(len(obs))
                if self.with_ref:                                   # the reference keyframe and level of UpdateNormalAndDepth
                    found, idx = ref >= 0 and len(obs) > 0, obs.get(ref, 0)
                    self.ref.append(self.slot(ref) if found else -1)
                    self.level.append(self.m["octave"][ref][idx] if found and idx < len(self.m["octave"][ref]) else 0)
        return self.pts.index(p)

    def row(self, ids, with_obs=True):
        self.row_point += [-1 if p < 0 else self.point(p, with_obs) for p in ids]
        self.row_start.append(len(self.row_point))

    def same(self, printed, mode):
        for name in ("kfs", "pts", "row_start", "row_point", "obs_start", "obs_kf", "point_bad"):
            assert _ints(printed, mode + "." + name) == getattr(self, name), (mode, name)
        self.in_range()

    def in_range(self):
        """what the device relies on"""
        assert all(-1 <= p < len(self.pts) for p in self.row_point) and all(0 <= k < len(self.kfs) for k in self.obs_kf)
        assert self.row_start[-1] == len(self.row_point) and self.obs_start[-1] == len(self.obs_kf)
        assert self.row_start == sorted(self.row_start) and self.obs_start == sorted(self.obs_start)


def test_the_map_holds_every_case(printed):
    m = _map(printed)
    rows, obs, ref = m["rows"], m["obs"], m["ref"]
    assert len(rows) == 5 and len(obs) == 8
    observers = {k for o in obs.values() for k in o}
    listed = [p for k in sorted(rows) for p in rows[k] if p >= 0]
    assert any(-1 in r and any(p >= 0 for p in r) and r[0] >= 0 and r[-1] >= 0 for r in rows.values()), "a null entry inside a row"
    assert any(r == [] for r in rows.values()), "an empty row"
    assert any(r and all(p < 0 for p in r) for r in rows.values()), "a row of nulls only"
    assert any(listed.count(p) == 2 and obs[p] for p in obs), "a point in two rows"
    assert any(not obs[p] for p in listed), "a point with no observation"
    assert any(m["bad"][p] for p in listed), "a bad point"
    first_row = next(k for k in sorted(rows) if any(p >= 0 for p in rows[k]))
    assert any(k > first_row and rows[k] for p in rows[first_row] if p >= 0 for k in obs[p]), "a keyframe first met as an observer, later a row owner"
    assert any(rows[k] and k not in observers for k in rows), "a keyframe that owns a row and observes nothing"
    assert any(ref[p] >= 0 and obs[p] and ref[p] not in obs[p] for p in listed), "a reference keyframe that does not observe its point"
    assert any(ref[p] < 0 and obs[p] for p in listed), "a point without a reference keyframe"
    assert any(ref[p] in obs[p] and obs[p][ref[p]] >= len(m["octave"][ref[p]]) for p in listed), "an observation index beyond mvKeysUn"
    assert all(0 not in o for o in m["octave"].values()), "octave 0 stands for `out of range`"


def test_covisibility_order(printed):
    m, self_slot = _map(printed), []
    g = Gather(m)
    for k in sorted(m["rows"]):
        self_slot.append(g.slot(k))
        g.row(m["rows"][k])
    g.same(printed, "covis")
    assert _ints(printed, "covis.self") == self_slot
    assert g.kfs != sorted(g.kfs), "an observer takes its slot before a later row owner"


def test_culling_order(printed):
    m = _map(printed)
    g, row_kf, cand = Gather(m), [], _ints(printed, "cull.cand")
    assert sorted(cand) == sorted(m["rows"]) and cand != sorted(cand)
    for k in cand:
        row_kf.append(g.slot(k))                                    # the candidate's own slot before its row is walked
        g.row(m["rows"][k])
    g.same(printed, "cull")
    assert _ints(printed, "cull.row_kf") == row_kf
    assert _ints(printed, "cull.obs_level") == g.obs_level and _ints(printed, "cull.obs_idx") == g.obs_idx and 0 in g.obs_level


def test_correct_loop_order(printed):
    m = _map(printed)
    g = Gather(m, with_ref=True)
    ranks = _ints(printed, "loop.rank_kf")
    K = len(ranks)
    assert ranks == list(range(K)) and 1 < K < len(m["rows"])       # slots 0 .. K-1 are the ranks in the map's order
    rank_kf = sorted(_ints(printed, "loop.kfs")[:K])
    for k in rank_kf:
        g.slot(k)
    for k in rank_kf:
        g.row(m["rows"][k])
    g.same(printed, "loop")
    assert g.kfs[:K] == rank_kf and len(g.kfs) > K
    assert _ints(printed, "loop.kf_id") == [m["kf_id"][k] for k in g.kfs]
    assert _ints(printed, "loop.n_obs") == g.n_obs and _ints(printed, "loop.ref") == g.ref and _ints(printed, "loop.level") == g.level
    assert -1 in g.ref and 0 in [lv for r, lv in zip(g.ref, g.level) if r >= 0]
    (scale,) = printed["loop.scale"]                                # the table of the first reference keyframe met, mnScaleLevels long
    assert [float.fromhex(s) for s in scale] == [float(np.float32(s)) for s in (1.0, 1.2, 1.44, 1.728, 2.0736, 2.48832)]


def test_local_map_order(printed):
    m = _map(printed)
    g = Gather(m)
    frame = _ints(printed, "local.frame_item")
    own = _ints(printed, "local.own_points")[0]
    own_pts = _ints(printed, "local.pts")[:own]
    assert -1 in frame and len(set(frame)) < len(frame)              # a null (and a nulled bad) entry, a point listed twice
    g.row([-1 if i < 0 else own_pts[i] for i in frame])
    assert g.row_point == frame and _ints(printed, "local.frame_start") == g.row_start and len(g.pts) == own
    assert not any(g.point_bad), "a bad own point is nulled by the caller before it is registered"
    g.row_start, g.row_point = [0], []
    S1 = len(g.kfs)
    for k in list(g.kfs):
        g.row(m["rows"][k], with_obs=False)
    g.same(printed, "local")
    assert len(g.kfs) == S1 and len(g.pts) > own and len(g.obs_start) == own + 1     # the observation CSR covers the frame's own points only

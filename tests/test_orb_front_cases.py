"""The reach proof of tests/test_gpu_orb_front.py, on the CPU: what the oracle and the schedule model (tests/orbfront_cases.py) do on each named image -- exact
ties, scores at the two thresholds, cell and tile borders, the four extreme key points, exact and near-diagonal angles, survivor lists over capacity in pass
A, in pass B and in one tile of both kinds, suppression queues that wrap.  pytest -s prints, per input, the candidate counts, the tiles over capacity per pass and
the angle bits."""
import os

import numpy as np

import orc
import orbfront_cases as fc

S7, S19, S20, S169 = 7, 19, 20, 169


def _l0(name):
    """level-0 candidates of an image as (x, y, response) in level coordinates, in the reference's order"""
    return [(int(x) + fc.MINB, int(y) + fc.MINB, int(r)) for x, y, r in fc.ref(name)[1][0][0]]


def _angles(name, octave=0):
    """(x, y) -> bit pattern of the angle, key points of one octave"""
    k = fc.ref(name)[2]["kps"]
    k = k[k["octave"] == octave]
    return {(int(x), int(y)): int(a) for x, y, a in zip(k["x"], k["y"], k["angle"].view(np.uint32))}


def _over(name):
    s, cap, _ = fc.sched(name)
    return {p: [(l, t["tx"], t["ty"]) for l, tiles in enumerate(s) for t in tiles if t[p + "_over"]] for p in "AB"}


def test_the_model_states_the_reference_cell_rule():
    """the level sizes and the cells of the model are the oracle's; the computed regions the tiles give their waves are the cells' sub-images minus the 3-pixel frame"""
    for name in ("ladder", "dense high"):
        r = fc.ref(name)[2]
        _, cap, geoms = fc.sched(name)
        assert fc.level_sizes(fc.W, fc.H, 1.2, fc.NLEVELS) == list(zip(r["lw"], r["lh"])) == [(192, 144), (160, 120), (133, 100)]
        assert [len(g["cells"]) for g in geoms] == r["ncells"] == [15, 8, 6]
        for g in geoms:
            seen = set()
            for t in g["tiles"]:
                for x0, x1, y0, y1, cell in t["regions"].values():
                    cx, cy, cw, ch = g["cells"][cell]
                    assert (x0, x1, y0, y1) == (cx + 3, cx + cw - 3, cy + 3, cy + ch - 3)
                    seen.add(cell)
            assert seen == set(range(len(g["cells"])))
        assert fc.accepted(geoms)
        # the widest tile region is level 2's (2 cells of 34), the tallest level 1's (44 + 38 rows): the list is sized by both
        assert cap == 68 * 41 + 4 == 2792
    g0 = fc.sched("ladder")[2][0]
    assert [t["rx0"] for t in g0["tiles"][:3]] == [19, 83, 147] and g0["tiles"][0]["xm"] == 51 and g0["rex"] == 173
    assert [g0["tiles"][0]["ry0"], g0["tiles"][0]["ym"], g0["tiles"][3]["ry0"], g0["rey"]] == [19, 57, 95, 125]


def test_the_inputs_reach_every_situation():
    for name in fc.CASES:
        img, lv, r = fc.ref(name)    # (level_candidates asserts orc_fast_cells on each level's plane == ncand)
        over = _over(name)
        print("%-16s candidates %-16s key points %-14s over capacity: pass A %s, pass B %s" % (name, r["ncand"], [int((r["kps"]["octave"] == l).sum()) for l in range(fc.NLEVELS)],
                                                                                        over["A"], over["B"]))
        if name not in fc.DENSE:
            assert over == {"A": [], "B": []}
            print("%16s level 0: %s" % ("", ["(%d, %d) %d %08X" % (x, y, s, _angles(name).get((x, y), 0xFFFFFFFF)) for x, y, s in _l0(name)]))

    # ---- the contrast ladder: 7 nothing, 8 -> 7, 20 -> 19 (both only by the retry), 21 -> 20, 230 on 60 -> 169; 255 on 0 -> 254
    at = fc.LADDER_AT
    assert _l0("ladder") == [at[8] + (S7,), at[-8] + (S7,), at[20] + (S19,), at[-20] + (S19,), at[21] + (S20,), at[-21] + (S20,), (160, 76, S169)]
    no_retry = fc.fast_cells(fc.ref("ladder")[2]["pyr"][0], fc.INI, fc.INI)
    assert [(int(x) + 16, int(y) + 16, int(s)) for x, y, s in no_retry] == [at[21] + (S20,), at[-21] + (S20,), (160, 76, S169)]
    assert set(_angles("ladder").values()) == {0}                      # a lone dot: both moments 0, angle bits 0x00000000
    assert _l0("top of the score") == [(96, 70, 254)]
    # ---- strong and weak in one cell: only the strong one; the weak one alone would be found
    assert _l0("strong and weak") == [(24, 24, S20)]
    alone = fc.ref("strong and weak")[0].copy()
    alone[24, 24] = fc.BG
    assert [tuple(int(v) for v in k) for k in fc.fast_cells(orc.orb_extract(alone, nfeatures=fc.NF, nlevels=1, debug=True)["pyr"][0], fc.INI, fc.MIN)] == [(46 - 16, 50 - 16, S7)]
    # ---- plateaus: corners at iniThFAST with equal scores, no candidate; their cells are handed to pass B and stay empty
    assert _l0("plateaus") == []
    crn = fc.fast_corners(fc.ref("plateaus")[2]["pyr"][0], fc.INI)
    assert crn[38, 35] and crn[38, 36] and crn[76, 96:99].all() and crn[76, 132:135].all() and not crn[76, 100:131].any()
    s0 = fc.sched("plateaus")[0][0]
    # (the three pixels at either end of the line see it on one side of their ring only; from the fourth on it crosses the ring twice and leaves two arcs of 7)
    assert s0[0]["need"] == [0, 1, 2, 3] and s0[1]["need"] == [0, 1, 2, 3] and s0[0]["A_queue"] == 2 and s0[1]["A_queue"] == 6
    # ---- diagonal pairs: one candidate inside a cell, two across a cell border (suppression never looks across one)
    p = fc.PAIRS_AT
    assert sorted(_l0("diagonal pairs")) == sorted([p["inside"] + (S169,)] + [c for k in p if k != "inside" for c in (p[k] + (S169,), (p[k][0] + 1, p[k][1] + 1, 139))])
    g0 = fc.sched("diagonal pairs")[2][0]
    assert g0["tiles"][0]["rx1"] == 83 == p["corner"][0] + 1 == p["tile border"][0] + 1 and g0["tiles"][0]["ym"] == 57 == p["corner"][1] + 1 == p["horizontal"][1] + 1
    assert g0["tiles"][4]["xm"] == 115 == p["vertical"][0] + 1
    # ---- extremes: (19, 19) .. (w - 20, h - 20) accepted, one pixel further out rejected
    assert _l0("extremes") == [e + (S169,) for e in fc.EXTREMES] and len(fc.ref("extremes")[2]["kps"]) == 4
    # ---- satellites: exact angles 0 / 90 / 180 / 270 and the three near-diagonals; the satellite of "135" is a candidate of response 9 through the retry
    want = {fc.SAT_AT[n]: fc.SATELLITES[n][1] for n in fc.SAT_AT}
    assert _angles("satellites") == want
    assert [want[fc.SAT_AT[n]] for n in ("none", "right", "below", "left", "above")] == [0, 0] + [int(np.float32(a).view(np.uint32)) for a in (90, 180, 270)]
    assert ["%.6f" % np.uint32(fc.SATELLITES[n][1]).view(np.float32) for n in ("45", "315", "135")] == ["44.990452", "315.009552", "135.009552"]
    assert sorted(_l0("satellites")) == sorted([xy + (S169,) for xy in fc.SAT_AT.values()] + [(142, 111, 9)])
    assert not any(int(x) + 16 == 142 for x, y, s in fc.fast_cells(fc.ref("satellites")[2]["pyr"][0], fc.INI, fc.INI))
    for n in fc.SATELLITES:
        if n != "none":
            name = "corner " + n
            assert _l0(name) == [(19, 19, S169), (fc.W - 20, fc.H - 20, S169)]
            assert _angles(name) == {(19, 19): fc.SATELLITES[n][1], (fc.W - 20, fc.H - 20): fc.SATELLITES[n][1]}
    # the pattern steered by 44.99 degrees reaches row 1 and column 1 of the blurred plane from (19, 19), and the last rows / columns from (w - 20, h - 20)
    pat = np.fromfile(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bit_pattern_31.bin"), np.int32).astype(np.float32).reshape(-1, 2)
    assert len(pat) == 512 and np.abs(pat).max() == 13
    for n in ("45", "135"):
        ang = np.uint32(fc.SATELLITES[n][1]).view(np.float32) * np.float32(0.01745329238)
        a, b = np.float32(np.cos(np.float64(ang))), np.float32(np.sin(np.float64(ang)))
        rows = np.rint(pat[:, 0] * b + pat[:, 1] * a).astype(int)
        cols = np.rint(pat[:, 0] * a - pat[:, 1] * b).astype(int)
        print("%16s pattern at %s: rows %d..%d, columns %d..%d of the key point" % ("", n, rows.min(), rows.max(), cols.min(), cols.max()))
        assert 0 <= 19 + min(rows.min(), cols.min()) <= 1 and max(rows.max(), cols.max()) >= 17
        assert fc.H - 20 + rows.max() <= fc.H - 1 and fc.W - 20 + cols.max() <= fc.W - 1
    # ---- a frame whose level 0 is empty while the higher ones are not
    assert fc.ref("one block")[2]["ncand"] == [0, 1, 1] and [int((fc.ref("one block")[2]["kps"]["octave"] == l).sum()) for l in range(3)] == [0, 1, 1]


def test_the_dense_inputs_overflow_the_list_where_they_say():
    """caps, not measurements: survivors >= 1.1 x the capacity where an overflow is wanted, each row half inside it"""
    full = [(0, 0, 0), (0, 1, 0)]      # the tiles of level 0 with 2 x 2 cells
    for name in fc.DENSE:
        s, cap, _ = fc.sched(name)
        for l, tiles in enumerate(s):
            for t in tiles:
                print("%-14s level %d tile (%d, %d): pass A %4d %-5s halves %-12s queued %3d | emitted %-12s | pass B %4d %-5s halves %-12s queued %3d"
                      % (name, l, t["tx"], t["ty"], t["A"], t["A_over"], t["A_half"], t["A_queue"], t["emitted"], t["B"], t["B_over"], t["B_half"], t["B_queue"]))
                for p in "AB":
                    assert max(t[p + "_half"]) + 4 <= cap                       # a half always fits
                    # (the claims below are about level 0; what the resized levels do is left to the comparison with the oracle)
                    assert l > 0 or not (cap - 4) * 0.9 < t[p] < (cap - 4) * 1.1,"a pass near the capacity: %d of %d" % (t[p], cap)
    t = {name: {(l, d["tx"], d["ty"]): d for l, tiles in enumerate(fc.sched(name)[0]) for d in tiles} for name in fc.DENSE}
    cap = fc.sched("dense high")[1]
    # pass A over capacity in every full tile of level 0 (and of levels 1 and 2), no pass B anywhere
    assert set(full) <= set(_over("dense high")["A"]) and _over("dense high")["B"] == [] and all(d["need"] == [] for d in t["dense high"].values())
    assert all(t["dense high"][k]["A"] >= 1.1 * cap for k in full)
    # ... and the four waves queue more than 4 x 64 corners of one half's list between them: at least one suppression queue wraps
    assert all(t["dense high"][k]["A_queue"] >= 1.1 * 256 for k in full)
    # every cell empty at iniThFAST (not even a survivor of the pre-test), pass B over capacity in the full tiles
    assert all(d["A"] == 0 and d["emitted"] == [] for d in t["dense low"].values()) and _over("dense low") == {"A": [], "B": full}
    assert all(t["dense low"][k]["B"] >= 1.1 * cap for k in full) and fc.ref("dense low")[2]["ncand"][0] > 0
    # a pass B in one piece whose queues wrap
    assert _over("two-valued") == {"A": [], "B": []} and all(d["A"] == 0 for d in t["two-valued"].values())
    assert all(t["two-valued"][k]["B"] <= 0.9 * cap and t["two-valued"][k]["B_queue"] >= 1.1 * 256 for k in full)
    # one tile of both kinds: cell (0, 0) has a maximum at iniThFAST and is emitted by pass A, the three others are empty there and overflow pass B
    for name in ("mixed", "mixed in cell"):
        d = t[name][(0, 0, 0)]
        assert d["emitted"] == [0] and d["need"] == [1, 2, 3] and not d["A_over"] and d["A"] > 0 and d["B_over"] and d["B"] >= 1.1 * cap
        assert _over(name) == {"A": [], "B": full}
    # half a tile can never overflow: why "mixed" keeps one cell of four at high contrast, not two
    g0 = fc.sched("mixed")[2][0]["tiles"][0]
    assert (g0["rx1"] - g0["rx0"]) * (g0["ry1"] - g0["ry0"]) // 2 + 4 <= cap < 3 * (g0["rx1"] - g0["rx0"]) * (g0["ry1"] - g0["ry0"]) // 4


def test_the_batches_hold_every_named_image():
    """... with a flat frame at both ends and one between full frames; the partial last groups of 8 are (flat), (full, full, flat) and (flat)"""
    lists = {B: fc.batch_names(B, s) for B, s in fc.BATCHES}
    assert {n for names in lists.values() for n in names} == set(fc.CASES) | {None}
    assert sorted(lists) == [1, 8, 9, 11, 17] and all(len(v) == B for B, v in lists.items())
    for B, names in lists.items():
        if B > 1:
            assert names[0] is None and names[-1] is None and [n is None for n in names].count(True) == 3
            mid = names.index(None, 1)
            assert names[mid - 1] is not None and names[mid + 1] is not None
    assert [n is None for n in lists[11][8:]] == [False, False, True]


def test_the_128_6_image_never_overflows():
    """the `low` image of test_orb_flat_and_noise_images fires the retry in every cell but stays far below the list's capacity: why the dense inputs above were needed"""
    r = orc.orb_extract(fc.low_128_6(), debug=True)
    s, cap, geoms = fc.schedule(r["pyr"])
    assert fc.accepted(geoms)
    most = max(max(t["A"], t["B"]) for tiles in s for t in tiles)
    print("128 +- 6, 640 x 480: capacity %d, most survivors in a pass %d, candidates %s" % (cap, most, r["ncand"]))
    assert all(t["A"] == 0 and t["emitted"] == [] and not t["B_over"] for tiles in s for t in tiles) and sum(r["ncand"]) > 0
    assert most < 0.5 * cap
    # the uniform noise of the same test: pass A over capacity in most tiles of level 0 -- the one redo the suite did reach before
    noise = np.random.default_rng(7).integers(0, 256, (480, 640), dtype=np.uint8)
    s, cap, _ = fc.schedule(orc.orb_extract(noise, debug=True)["pyr"])
    assert sum(t["A_over"] for t in s[0]) > len(s[0]) // 2 and not any(t["B_over"] for tiles in s for t in tiles)


def test_the_shrunk_parameter_sets_keep_their_property():
    """from the stated geometry: a last cell row without a computed region behind a shortened one, and a last tile one column group wide"""
    for name, (w, h, sf, nlev, ini, mn, nf) in fc.PARAM_SETS.items():
        geoms = [fc.level_geometry(a, b) for a, b in fc.level_sizes(w, h, sf, nlev)]
        assert fc.accepted(geoms)
        l, prop = fc.PARAM_LEVEL[name]
        g = geoms[l]
        last = g["tiles"][-1]
        if prop == "row":
            assert g["ncy"] % 2 == 0 and last["ym"] == last["ry1"] == g["rey"] and 0 < last["ym"] - last["ry0"] < g["hCell"]     # shortened, then empty
            assert last["regions"][2][2] == last["regions"][2][3]
        else:
            assert g["ncx"] % 2 == 1 and last["ngr"] == 1 and 1 <= last["rx1"] - last["rx0"] <= 4
        print("%-10s %4d x %3d: level %d %4d x %3d, last tile x [%d, %d) y [%d, %d), second cell row from %d, column groups %d"
              % (name, w, h, l, g["w"], g["h"], last["rx0"], last["rx1"], last["ry0"], last["ry1"], last["ym"], last["ngr"]))
        img = fc.param_image(name)
        r = orc.orb_extract(img, nfeatures=nf, scale_factor=sf, nlevels=nlev, ini_th=ini, min_th=mn, debug=True)
        assert [(a, b) for a, b in zip(r["lw"], r["lh"])] == fc.level_sizes(w, h, sf, nlev)
        s, cap, _ = fc.schedule(r["pyr"], ini, mn)
        d = s[l][-1]
        print("%10s last tile of level %d: pass A %d %s, emitted %s, pass B %d %s; candidates %s" % ("", l, d["A"], d["A_over"], d["emitted"], d["B"], d["B_over"], r["ncand"]))
        assert d["A"] > 0 and d["emitted"] and r["ncand"][l] > 0       # the dense piece reaches the last tile
        pts = fc.param_points(name)
        k0 = {(int(x) + 16, int(y) + 16): int(v) for x, y, v in fc.fast_cells(r["pyr"][0], ini, mn)}
        assert k0.get(pts["accepted"]) == S169 and pts["rejected"] not in k0 and pts["pair"] not in k0 and (pts["pair"][0] + 1, pts["pair"][1]) not in k0

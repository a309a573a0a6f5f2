"""The scenes of tests/stridegen.py are what they claim to be: every grid cap is read from the source that sets it, every scene has at least 2 * cap + 7 rows,
and every workgroup meets the prescribed sequence of row kinds -- asserted on the restatements' own counts, so that a machine without a GPU can show what
tests/test_gpu_second_rows.py runs.  No GPU needed."""
import numpy as np

import covisref
import localmapref
import stridegen as S


def _per_workgroup(kinds, G):
    """the sequence of row kinds every workgroup meets: {sequence: number of workgroups}"""
    out = {}
    for b in range(min(G, len(kinds))):
        seq = tuple(kinds[b::G])
        out[seq] = out.get(seq, 0) + 1
    return out


def test_every_cap_is_read_from_the_source_that_sets_it():
    c = S.grid_caps()
    assert c["covis"] >= 64 and c["cull"] >= 64 and c["local"] >= 64 and c["local_kf"] == 4 * c["local"]
    assert c["map_small"] == 16 * c["map_blocks"] and c["map_wave"] == 4 * c["map_blocks"] and c["map_block"] >= 64 and c["mapgeom_block"] >= 64
    assert c["track_close"] == c["track_kf"] == c["tri"] and c["tri"] >= 1 << 16
    p, b = S.passes(10, 4)
    assert p.tolist() == [0, 0, 0, 0, 1, 1, 1, 1, 2, 2] and b.tolist() == [0, 1, 2, 3, 0, 1, 2, 3, 0, 1]


def _distinct(s, r, votes=False):
    return covisref._count(s["rows"][r], None if votes or s["selfs"] is None else s["selfs"][r], s["obs"], s["n_kf"], None)


def test_covis_table_scene_overflows_empties_fits_and_overflows_again():
    s = S.covis_table_scene()
    G, n_rows = s["G"], len(s["rows"])
    assert n_rows >= 2 * G + 7 and G == S.grid_caps()["covis"]
    seqs = _per_workgroup(s["kinds"], G)
    assert seqs == {("over", "empty", "fit", "over2", "over"): 7, ("over", "empty", "fit", "over2"): G - 7}
    slots = 2
    while slots < s["table"]:
        slots <<= 1
    full = slots - slots // 8                                        # the table counts as full at 7/8
    assert s["n_kf"] > 1 and s["dense"] == 1                         # dense_max_kf = 1: not the dense counters
    for votes in (False, True):
        for b in list(range(9)) + [G - 1]:
            first, second, third, fourth = (_distinct(s, b + p * G, votes) for p in range(4))
            assert len(first) > full and len(fourth) > full, "the table overflows"
            assert len(second) == 0
            assert 0 < len(third) <= slots // 2 and not set(third) & set(first), "fits the table, disjoint keyframes"
            assert len(set(fourth) & set(first)) >= 8 and set(fourth) - set(first), "overlaps the first row's keyframes"
            assert max(first.values()) > 1 and max(fourth.values()) > 1
    assert all(len(_distinct(s, r)) > full for r in range(4 * G, n_rows))
    assert any(len(_distinct(s, r)) > s["stride"] for r in range(G))    # and lists beyond the stride


def test_covis_dense_scene_full_empty_one_point():
    s = S.covis_dense_scene()
    G = s["G"]
    assert len(s["rows"]) >= 2 * G + 7 and s["n_kf"] <= S.grid_caps()["covis_dense_default"]
    assert _per_workgroup(s["kinds"], G) == {("full", "empty", "one", "full", "empty"): 7, ("full", "empty", "one", "full"): G - 7}
    for b in (0, 1, 2, G - 1):
        assert len(_distinct(s, b)) == s["n_kf"] == len(_distinct(s, b + 3 * G)) and _distinct(s, b) != _distinct(s, b + 3 * G)
        assert len(_distinct(s, b + G)) == 0 and len(s["rows"][b + 2 * G]) == 1 and len(_distinct(s, b + 2 * G)) in (1, 2)


def test_covis_long_scene_has_two_consecutive_lists_beyond_the_sort_cap():
    s = S.covis_long_scene()
    c = S.grid_caps()
    G, cap = s["G"], c["covis_sort_cap"]
    assert len(s["rows"]) >= 2 * G + 7 and s["n_kf"] == cap + 2        # the smallest n_kf with two lengths above the cap
    p2 = 1
    while p2 < s["n_kf"]:
        p2 <<= 1
    assert c["covis_scratch"] // (p2 * 8 + (s["n_kf"] * 4 + 255) // 256 * 256) >= G      # the scratch bound leaves the grid at its cap
    for b in range(3):
        a, bb = _distinct(s, b), _distinct(s, b + G)
        assert len(a) > len(bb) > cap and len(set(a.values())) >= 4    # the first is the longer one; weights that differ
        assert s["kinds"][b + 2 * G] == "short" and 0 < len(_distinct(s, b + 2 * G)) < 10
    assert sum(k == "long" for k in s["kinds"]) == 6
    assert all(len(_distinct(s, r)) < 10 for r in range(3, G, 97))


def test_covis_votes_scene_every_counted_keyframe_bad_after_a_large_maximum():
    s = S.covis_votes_bad_scene()
    G = s["G"]
    assert len(s["rows"]) >= 2 * G + 7
    assert _per_workgroup(s["kinds"], G) == {("large", "all_bad", "mixed"): 7, ("large", "all_bad"): G - 7}
    for b in (0, 1, 2, 3, 4, 5, G - 1):
        a = covisref.local_keyframe_votes(s["rows"][b], s["obs"], s["n_kf"], None, s["kf_bad"])
        z = covisref.local_keyframe_votes(s["rows"][b + G], s["obs"], s["n_kf"], None, s["kf_bad"])
        assert a["max"][1] >= 6 and z == {"conn": [], "max": (-1, 0)}


def test_cull_scene_long_skipped_empty_mixed():
    import cullref
    s = S.cull_scene()
    c = S.grid_caps()
    G, m = s["G"], s["map"]
    assert s["n_cand"] >= 2 * G + 7 and G == c["cull"]
    assert _per_workgroup(s["kinds"], G) == {("long", "skipped", "empty", "mixed", "long"): 7, ("long", "skipped", "empty", "mixed"): G - 7}
    ref, one = S.cull_reference(s)
    by_kind = {}
    for j in list(range(40)) + list(range(G, G + 40)) + list(range(2 * G, 2 * G + 40)) + list(range(3 * G, 3 * G + 40)) + list(range(4 * G, 4 * G + 7)):
        by_kind.setdefault(s["kinds"][j], set()).add(int(s["which"][j]))
    for d in by_kind["long"]:
        r, f = s["distinct"][d]
        assert len(m["rows"][r]) > c["cull_chunk"] and not f & 1 and one["decision"][d] != cullref.SKIPPED and one["n_mps"][d] > c["cull_chunk"] // 2
    assert len(by_kind["skipped"]) == 7 and all(one["decision"][d] == cullref.SKIPPED for d in by_kind["skipped"])
    assert any(s["distinct"][d][1] & 1 for d in by_kind["skipped"]) and any(not 0 <= s["distinct"][d][0] < len(m["rows"]) for d in by_kind["skipped"])
    for d in by_kind["empty"]:
        assert m["rows"][s["distinct"][d][0]] == [] and (one["n_mps"][d], one["n_redundant"][d], one["decision"][d]) == (0, 0, cullref.KEEP)
    for d in by_kind["mixed"]:
        row = m["rows"][s["distinct"][d][0]]
        n = [len(m["obs"][p]) for p in row if p >= 0 and not m["point_bad"][p]]
        assert any(3 <= x <= c["cull_lane_max"] for x in n) and any(c["cull_lane_max"] < x <= c["cull_group_max"] for x in n) and any(x > c["cull_group_max"] for x in n)
        assert 0 < one["n_redundant"][d] < one["n_mps"][d]
    assert {cullref.KEEP, cullref.ERASED, cullref.NOT_ERASE, cullref.SKIPPED} == set(one["decision"])
    assert len(ref["decision"]) == s["n_cand"] and ref["erasures"] == 0 and not any(ref["kf_erased"])


def test_local_items_scene_short_long_short_long_with_shared_and_bad_ids():
    s = S.local_items_scene()
    G = s["G"]
    n_rows = len(s["local"])
    assert n_rows >= 2 * G + 7 and G == S.grid_caps()["local"]
    assert _per_workgroup(s["kinds"], G) == {("short", "long_a", "short", "long_b", "short"): 7, ("short", "long_a", "short", "long_b"): G - 7}
    slots = 2
    while slots < s["table"]:
        slots <<= 1
    length = lambda r: sum(len(s["kf_rows"][k]) for k in s["local"][r])   # noqa: E731
    ids = lambda r: {x for k in s["local"][r] for x in s["kf_rows"][k] if 0 <= x < s["n_items"]}   # noqa: E731
    over = 0
    for b in list(range(17)) + [G - 1]:
        assert length(b) <= slots // 2 and length(b + 2 * G) <= slots // 2 and length(b + G) > slots // 2 and length(b + 3 * G) > slots // 2
        a, bb = ids(b + G), ids(b + 3 * G)
        assert len(a & bb) >= 20 and len(bb - a) >= 20, "the second long row shares ids with the first and has ids it did not touch"
        assert any(s["item_bad"][x] for x in a), "ids marked bad in the first long row"
        want, seen = localmapref.local_items(s["local"][b + G], s["kf_rows"], s["n_items"], s["item_bad"], s["frame_rows"][b + G])
        over += len(want) > s["item_stride"]
        nxt, _ = localmapref.local_items(s["local"][b + 2 * G], s["kf_rows"], s["n_items"], s["item_bad"], s["frame_rows"][b + 2 * G])
        assert 0 < len(nxt) <= s["item_stride"], "a normal row follows"
        assert any(seen) and not all(seen), "the frame's own row clears bit 0 of some entries"
    assert 4 <= over <= 12                                            # status 4 in about half of the first long rows


def test_local_kf_scene_seeds_are_what_the_first_row_pushed():
    s = S.local_kf_scene()
    G = s["G"]
    assert len(s["seeds"]) >= 2 * G + 7 and G == S.grid_caps()["local_kf"]
    assert _per_workgroup(s["kinds"], G) == {("expands", "empty", "pushed", "empty"): 7, ("expands", "empty", "pushed"): G - 7}
    grown = 0
    for b in list(range(s["period"])):
        first = localmapref.local_keyframes(s["seeds"][b], s["covis"], s["children"], s["parent"], s["kf_bad"], 10, 80)
        assert s["seeds"][b + G] == [] and s["seeds"][b + 2 * G] == first[len(s["seeds"][b]):]
        grown += len(first) > len(s["seeds"][b])
    assert grown > s["period"] * 3 // 4 and s["period"] % 2 == 1 and np.gcd(s["period"], G) == 1


def test_local_visible_scene_alternates_empty_and_full_rows():
    s = S.local_visible_scene()
    G = s["G"]
    n = s["n_local"]
    assert len(n) >= 2 * G + 7 and G == S.grid_caps()["local"]
    for b in (0, 1, 2, 3, G - 1):
        seq = [int(n[r]) > 0 for r in range(b, len(n), G)]
        assert seq[:2] in ([True, False], [False, True]) and (len(seq) < 3 or seq[2] == seq[0])
    in_view, n_to, visible = S.local_visible_reference(s)
    assert (n_to[n == 0] == 0).all() and (n_to[n > 0] > 0).all() and not in_view[n == 0].any()
    assert (s["frustum"][n == 0] == 1).all()                          # in_view behind an empty list comes in set and must go out clear
    assert (visible >= s["start"]).all() and int((visible - s["start"]).sum()) > 5 * len(n)
    assert (in_view.sum(1) == n_to).all() and (s["seen"][n > 0].sum(1) > 0).all()


def _valid_counts(s):
    return np.array([int(s["valid_d"][s["start_d"][i]:s["start_d"][i + 1]].sum()) for i in range(s["P"])])


def test_map_scenes_fill_every_class_past_twice_its_grid():
    c = S.grid_caps()
    lo = {"small": 1, "wave": c["map_small_max"] + 1, "block": c["map_wave_max"] + 1}
    hi = {"small": c["map_small_max"], "wave": c["map_wave_max"], "block": 1 << 30}
    for cls in ("small", "wave", "block"):
        s = S.map_scene(cls)
        G, P, n = s["G"], s["P"], s["n"]
        assert G == c["map_" + cls] and n >= 2 * G + 7 and P % 2 == 1 and np.gcd(P, G) == 1 and s["shift"] == G % P
        cnt = s["counts_d"]
        assert cnt.min() >= lo[cls] and cnt.max() <= hi[cls], "every point is of this class: the class list is the whole call"
        assert (cnt == lo[cls]).sum() + (cnt == lo[cls] + 1).sum() + (cnt == lo[cls] + 2).sum() > P // 2 and (cnt >= hi[cls] if cls != "block" else cnt >= c["map_block_cap"]).sum() <= 12
        full = np.diff(s["start"].astype(np.int64))
        assert np.array_equal(full, cnt[s["idx"]]) and len(s["desc"]) == full.sum()
        nxt = cnt[(np.arange(P) + s["shift"]) % P]                    # the count of the point that the same lanes take a pass later
        valid = _valid_counts(s)
        if cls == "small":
            assert ((cnt == c["map_small_max"]) & (valid[(np.arange(P) + s["shift"]) % P] == 0)).sum() >= 8, "none taking part after 16"
        elif cls == "wave":
            assert ((cnt == c["map_wave_max"]) & (nxt == c["map_small_max"] + 1)).sum() >= 1 and ((cnt == c["map_wave_max"]) & (nxt <= c["map_small_max"] + 5)).sum() >= 7
        else:
            assert cnt[1] == c["map_block_cap"] and cnt[10] == c["map_block_cap"] + 1 and nxt[1] == c["map_wave_max"] + 1 == nxt[10]
        assert (cnt != nxt).sum() > P // 2 and (valid[s["none"]] == 0).all()
    naive_wave = 4 * c["map_blocks"]                                  # PLF_MAP_NAIVE=1: every point up to MAP_WAVE_MAX is of the wave class
    assert S.map_scene("wave")["n"] >= 2 * naive_wave + 7


def test_normal_scene_has_both_classes_past_twice_their_grids():
    s = S.normal_scene()
    c = S.grid_caps()
    counts = s["counts"]
    wave = counts[(counts > c["map_small_max"]) & (counts <= c["map_wave_max"])]
    block = counts[counts > c["map_wave_max"]]
    assert len(wave) == s["nw"] >= 2 * c["map_wave"] + 7 and len(block) == s["nb"] >= 2 * c["mapgeom_block"] + 7
    assert s["Pw"] % 2 == 1 and s["Pb"] % 2 == 1 and np.gcd(s["Pw"], s["Gw"]) == 1 and np.gcd(s["Pb"], s["Gb"]) == 1
    q = np.flatnonzero(wave[:s["Gw"]] == c["map_wave_max"])
    assert len(q) > 100 and (wave[q + s["Gw"]] <= c["map_small_max"] + 5).all() and (wave[q + s["Gw"]] == c["map_small_max"] + 1).any()
    q = np.flatnonzero(block[:s["Gb"]] > c["mapgeom_chunk"])
    assert len(q) >= 20 and (block[q + s["Gb"]] <= c["map_wave_max"] + 3).all() and (block[q + s["Gb"]] == c["map_wave_max"] + 1).any()
    assert (block > 2 * c["mapgeom_chunk"]).sum() >= 10 and (block == c["mapgeom_chunk"]).sum() >= 10
    assert (counts == 0).sum() == 2 and s["m"]["ref_kf"][-1] == len(s["m"]["kf_ow"])


def test_track_scenes_change_the_entry_count_from_one_pass_to_the_next():
    import trackgen
    s = S.track_close_scene()
    G, P = s["G"], s["P"]
    assert s["n_frames"] >= G + 64 and G == S.grid_caps()["track_close"] and P % 2 == 1 and np.gcd(P, G) == 1
    assert s["period"]["stride"] == S.TRACK_STRIDE <= S.grid_caps()["track_wave_keys"] and 4 <= S.TRACK_STRIDE <= 8
    e = s["entries"]
    nxt = e[(np.arange(P) + s["shift"]) % P]
    pad = lambda x: 1 << int(np.ceil(np.log2(max(x, 1))))            # noqa: E731
    assert (e != nxt).all() and sum(pad(a) != pad(b) for a, b in zip(e, nxt)) > P // 2
    full = np.flatnonzero(e == S.TRACK_STRIDE)
    assert len(full) >= 2 and (nxt[full] == 0).all() and ((e == 0) & (s["period"]["n"] > 0)).any()    # ... and key points none of which is an entry
    ref = trackgen.ref_close(s["period"], **s["kw"])
    assert ref["status"].any() and not ref["status"].all() and (ref["n_new"] == 0).sum() >= 5 and len(set(ref["n_walked"].tolist())) >= 4
    assert set(s["idx"][:G + 64][G:].tolist()) <= set(range(P)) and s["idx"][G] == s["shift"]
    t = S.track_need_scene()
    import test_track_ref
    counts, dec = test_track_ref.ref_need(t["period"])
    assert t["n_frames"] >= t["G"] + 64 and len(set(counts[:, 2].tolist())) >= 4 and (counts[:, 2] == 0).sum() >= 8 and len(set(dec.tolist())) >= 2


def test_tri_scene_follows_full_jobs_with_bad_slots_and_skipped_baselines():
    import trigen
    import triref
    s = S.tri_scene()
    G, P = s["G"], s["P"]
    assert s["n_jobs"] >= G + 64 and G == S.grid_caps()["tri"] and P % 2 == 1 and np.gcd(P, G) == 1
    ref = trigen.ref_call(s["period"], new_stride=s["new_stride"])
    shift = G % P
    st, nn = ref["status"], ref["n_new"]
    nxt = (np.arange(P) + shift) % P
    full = np.flatnonzero((st == triref.OVERFLOW))
    assert len(full) >= 5 and (nn[full] > s["new_stride"]).all()
    assert ((st == triref.OVERFLOW) & (st[nxt] == triref.BAD_SLOT)).sum() >= 3 and ((nn >= 2) & (st[nxt] == triref.SKIPPED_BASELINE)).sum() >= 3
    assert (st == 0).sum() >= 5 and len(set(nn.tolist())) >= 4 and (nn != nn[nxt]).sum() > P // 2
    pairs = (s["period"]["match12"] >= 0).sum(1)
    assert len(set(pairs.tolist())) >= 5 and (ref["reason"] == 0).all(axis=1).sum() == ((st == triref.BAD_SLOT) | (st == triref.SKIPPED_BASELINE)).sum()

"""The local map on the GPU (plf_local_keyframes, plf_local_items, plf_local_gather, plf_local_visible) against the restatement
tests/localmapref.py, element for element.  Every call writes into sentinel-filled outputs with a guard behind the last row, so each comparison
also proves what was NOT written: nothing at the stride and beyond, nothing between a count and the stride, nothing but the counts in a row with
an empty seed.  Shapes are the smallest at which a stage can go wrong: the 64-lane chunks of the seed, neighbour and child loops, the 256-thread
segments and the scan of the item pass, both mark classes and both table classes."""
import numpy as np
import pytest

import localmapref as R
from conftest import gpu_available

pytestmark = pytest.mark.gpu
SENT, GUARD = -777, 64
BIG = 0x7FC00000                                                  # a float NaN's bit pattern, and a huge index


@pytest.fixture(autouse=True)
def _need_gpu():
    if not gpu_available():
        pytest.fail("no GPU visible: the -m gpu tests need a real MI355X")


def _dev(a, dtype=None):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype))).cuda()


def _csr(lists, before=(), after=(0,)):
    """CSR on the device with filler before the first and after the last range (never empty: a valid address)"""
    start = np.zeros(len(lists) + 1, np.int64)
    start[1:] = np.cumsum([len(x) for x in lists])
    start += len(before)
    flat = np.array(list(before) + [x for lst in lists for x in lst] + list(after), np.int64).astype(np.int32)
    return _dev(start, np.int32), _dev(flat)


def _padded(lists, stride, fill):
    """(rows x stride) int32 with each list cut at stride and `fill` behind it, and the TRUE counts"""
    a = np.full((len(lists), stride), fill, np.int64)
    for r, lst in enumerate(lists):
        k = min(len(lst), stride)
        a[r, :k] = lst[:k]
    return _dev(a.astype(np.int32)), _dev([len(x) for x in lists], np.int32)


class _Sent:
    """sentinel-filled outputs with a guard behind the last row"""

    def __init__(self, **shapes):
        import torch
        self.flat, self.view = {}, {}
        for name, (shape, dtype) in shapes.items():
            n = int(np.prod(shape))
            self.flat[name] = torch.full((n + GUARD,), SENT if dtype != torch.uint8 else 0xA5, dtype=dtype, device="cuda")
            self.view[name] = self.flat[name][:n].view(*shape)

    def host(self):
        import torch
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in self.flat.items()}


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]), k


# ---------------------------------------------------------------------------------------------------------------- expansion
def _kf_check(seeds, covis, children, parent, kf_stride, seed_stride=None, covis_stride=None, kf_bad=None, n_best=10, max_local=80, dense=0,
              seed_fill=BIG, child_filler=((), (0,))):
    import torch
    from rgbd_pl_slam_amd import local_keyframes
    n_kf, n_rows = len(parent), len(seeds)
    seed_stride = seed_stride or max(1, max((len(s) for s in seeds), default=1))
    covis_stride = covis_stride or max(1, max((len(c) for c in covis), default=1))
    d_seed, d_nseed = _padded(seeds, seed_stride, seed_fill)
    d_cov, d_ncov = _padded(covis, covis_stride, -1)
    cs, ck = _csr(children, *child_filler)
    out = _Sent(local_kf=((n_rows, kf_stride), torch.int32), n=((n_rows,), torch.int32), status=((n_rows,), torch.int32))
    local_keyframes(d_seed, d_nseed, d_cov, d_ncov, cs, ck, _dev(parent, np.int32), n_kf, kf_bad=None if kf_bad is None else _dev(kf_bad, np.uint8),
                    n_best=n_best, max_local=max_local, dense_max_kf=dense, out=(out.view["local_kf"], out.view["n"], out.view["status"]))
    h = out.host()
    for name, size in (("local_kf", n_rows * kf_stride), ("n", n_rows), ("status", n_rows)):
        assert (h[name][size:] == SENT).all(), (name, "guard overwritten")
    refs = []
    for r, seed in enumerate(seeds):
        row = h["local_kf"][r * kf_stride:(r + 1) * kf_stride]
        if not seed:
            assert h["n"][r] == 0 and h["status"][r] == 0 and (row == SENT).all(), (r, "an empty seed wrote its row")
            refs.append([])
            continue
        want = R.local_keyframes(seed[:seed_stride], [c[:covis_stride] for c in covis], children, parent, kf_bad, n_best, max_local)
        refs.append(want)
        k = min(len(want), kf_stride)
        assert h["n"][r] == len(want), (r, "count", int(h["n"][r]), len(want))
        assert row[:k].tolist() == want[:k], (r, row[:k].tolist()[-6:], want[:k][-6:])
        assert (row[k:] == SENT).all(), (r, "written behind the count")
        assert h["status"][r] == (1 if len(seed) > seed_stride else 0) | (2 if len(want) > kf_stride else 0), (r, "status", int(h["status"][r]))
    return h, refs


def _kf_world(seed, n_kf=400, bad=True):
    """a forest (the parent of slot k, if it has one, is below k), ordered neighbour lists of 0 .. 14 entries, a tenth of the keyframes bad"""
    rng = np.random.default_rng(seed)
    parent = [-1] + [int(rng.integers(0, k)) if rng.random() < 0.3 else -1 for k in range(1, n_kf)]   # mostly roots: a pushed parent ends a row
    children = [[] for _ in range(n_kf)]
    for k, p in enumerate(parent):
        if p >= 0:
            children[p].append(k)
    covis = [[int(x) for x in rng.choice(n_kf, int(rng.integers(0, 15)), replace=False) if x != k] for k in range(n_kf)]
    kf_bad = [int(x) for x in rng.integers(0, 10, n_kf) == 0] if bad else None
    return rng, parent, children, covis, kf_bad


def _seeds(rng, n_kf, kf_bad, sizes):
    good = [k for k in range(n_kf) if not (kf_bad and kf_bad[k])]
    return [sorted(int(x) for x in rng.choice(good, n, replace=False)) for n in sizes]


@pytest.mark.parametrize("dense", [0, 1])
def test_seed_sizes_at_the_chunk_and_limit_edges(dense):
    rng, parent, children, covis, kf_bad = _kf_world(1)
    sizes = [0, 1, 63, 64, 65, 79, 80, 81, 2, 130]
    seeds = _seeds(rng, len(parent), kf_bad, sizes)
    h, refs = _kf_check(seeds, covis, children, parent, 140, kf_bad=kf_bad, dense=dense)
    grown = [len(r) - len(s) for r, s in zip(refs, seeds)]
    assert grown[sizes.index(81)] == 0 and grown[sizes.index(130)] == 0          # size() > 80 at the first test: nothing joins
    assert grown[sizes.index(80)] >= 1 and grown[sizes.index(1)] >= 1            # ... while 80 still runs an iteration


def test_both_mark_classes_write_the_same_bits_and_two_calls_too():
    rng, parent, children, covis, kf_bad = _kf_world(2)
    seeds = _seeds(rng, len(parent), kf_bad, [5, 17, 40, 70, 78, 79, 80, 0, 9])
    a, _ = _kf_check(seeds, covis, children, parent, 96, kf_bad=kf_bad)
    b, _ = _kf_check(seeds, covis, children, parent, 96, kf_bad=kf_bad, dense=1)
    c, _ = _kf_check(seeds, covis, children, parent, 96, kf_bad=kf_bad)
    _same(a, b); _same(a, c)


@pytest.mark.parametrize("dense", [0, 1])
def test_long_child_lists_whose_last_entry_alone_can_join(dense):
    lengths = [63, 64, 65, 130]
    n_kf = 700
    parent, covis, kf_bad = [-1] * n_kf, [[] for _ in range(n_kf)], [0] * n_kf
    children = [[] for _ in range(n_kf)]
    nxt = 10
    for s, L in enumerate(lengths):                               # seed s: L - 1 bad children, then the one that joins
        children[s] = list(range(nxt, nxt + L))
        for k in children[s][:-1]:
            kf_bad[k] = 1
        nxt += L
    # the same with marked instead of bad children: seed 4 + its children but the last are all seeds
    children[4] = list(range(nxt, nxt + 65))
    seeds = [[s] for s in range(4)] + [[4] + children[4][:-1]]
    _, refs = _kf_check(seeds, covis, children, parent, 80, kf_bad=kf_bad, dense=dense)
    assert refs[:4] == [[s, children[s][-1]] for s in range(4)] and refs[4][-1] == children[4][-1] and len(refs[4]) == 66


def test_the_rules_of_one_iteration():
    # slots: 0 .. 4 seeds; 10 .. 30 others
    n_kf = 40
    parent, covis, children, kf_bad = [-1] * n_kf, [[] for _ in range(n_kf)], [[] for _ in range(n_kf)], [0] * n_kf
    covis[0] = [20, 21, 22]; kf_bad[20] = 1                       # a bad neighbour is skipped, one neighbour joins
    children[0] = [23, 24]                                        # one child joins
    covis[21] = [25]; children[21] = [26]; parent[21] = 27        # a pushed keyframe is never expanded
    covis[1] = [0, 2] + [21] * 8 + [28]                           # ten marked entries, the eleventh is never considered
    parent[2] = 29; kf_bad[29] = 1                                # a bad parent joins all the same, and ends the expansion
    covis[3] = [30]                                               # ... with seeds left over
    _, refs = _kf_check([[0, 1, 2, 3], [3, 2, 1]], covis, children, parent, 16, kf_bad=kf_bad)
    assert refs == [[0, 1, 2, 3, 21, 23, 29], [3, 2, 1, 30, 29]]
    # a marked parent ends nothing; n_best below the list length
    parent[2] = 3
    _, refs = _kf_check([[0, 1, 2, 3]], covis, children, parent, 16, kf_bad=kf_bad, n_best=1)
    assert refs == [[0, 1, 2, 3, 23, 30]]
    # 79 seeds grow to 82: neighbour, child and the parent that ends it
    n_kf = 100
    parent, covis, children = [-1] * n_kf, [[] for _ in range(n_kf)], [[] for _ in range(n_kf)]
    covis[0] = [90]; children[0] = [91]; parent[0] = 92; covis[1] = [93]
    _, refs = _kf_check([list(range(79)), list(range(80)), list(range(81)), list(range(1, 80))], covis, children, parent, 96)
    assert [len(r) for r in refs] == [82, 83, 81, 80] and refs[0][79:] == [90, 91, 92] and refs[3][79:] == [93]


def test_short_neighbour_rows_truncated_seeds_and_list_overflow():
    rng, parent, children, covis, kf_bad = _kf_world(3)
    seeds = _seeds(rng, len(parent), kf_bad, [12, 3, 8, 9, 0, 30])
    _kf_check(seeds, covis, children, parent, 96, covis_stride=6, kf_bad=kf_bad)                 # n_covis (true) above a stride below 10
    _kf_check(seeds, covis, children, parent, 96, kf_bad=kf_bad, n_best=3)
    _kf_check(seeds, covis, children, parent, 96, kf_bad=kf_bad, n_best=0)
    h, _ = _kf_check(seeds, covis, children, parent, 96, seed_stride=8, kf_bad=kf_bad)           # n_seed > seed_stride: status 1
    assert h["status"][:6].tolist() == [1, 0, 0, 1, 0, 1]
    h, refs = _kf_check(seeds, covis, children, parent, 5, kf_bad=kf_bad)                        # lists beyond kf_stride: status 2, true counts
    assert h["status"][:6].tolist() == [2, 0 if len(refs[1]) <= 5 else 2, 2, 2, 0, 2]
    h, _ = _kf_check(seeds, covis, children, parent, 1, kf_bad=kf_bad, dense=1)
    assert (h["status"][[0, 2, 3, 5]] == 2).all()


@pytest.mark.parametrize("dense", [0, 1])
def test_out_of_range_slots_in_every_input_are_skipped(dense):
    rng, parent, children, covis, kf_bad = _kf_world(4, n_kf=200)
    n_kf = len(parent)
    seeds = _seeds(rng, n_kf, kf_bad, [6, 20, 64, 1])
    clean, _ = _kf_check(seeds, covis, children, parent, 96, kf_bad=kf_bad, dense=dense, n_best=14)
    junk = [-5, n_kf, BIG, -2 ** 31]
    d_seeds = [junk[:2] + s[:1] + junk[2:] + s[1:] + junk for s in seeds]
    d_covis = [junk + c for c in covis]
    d_children = [junk + c + junk for c in children]
    dirty, _ = _kf_check(d_seeds, d_covis, d_children, parent, 96, kf_bad=kf_bad, dense=dense, n_best=18, child_filler=(tuple(junk), tuple(junk) * 20))
    _same(clean, dirty)
    d_parent = [p if p >= 0 else junk[k % 4] for k, p in enumerate(parent)]
    dirty, _ = _kf_check(seeds, covis, children, d_parent, 96, kf_bad=kf_bad, dense=dense, n_best=14)
    _same(clean, dirty)


def test_colliding_and_wrapping_slots_in_the_mark_hash():
    """the hash set of marks (dense_max_kf = 1) with keyframes that all fall into one chain and chains that run over the table's end: 13 seeds of
    5000 keyframes give min(n_kf, 13 + 3 * 81) = 256 marks to hold, so 512 slots; the slot of a keyframe is (kf * 2654435761 mod 2^32) >> 23"""
    n_kf = 5000
    slot = lambda kf: ((kf * 2654435761) & 0xFFFFFFFF) >> 23      # noqa: E731
    last, prev, one = ([k for k in range(n_kf) if slot(k) == s] for s in (511, 510, 77))
    assert min(len(last), len(prev), len(one)) >= 6
    seed = sorted(last[:4] + prev[:4] + one[:5])
    parent, covis, children = [-1] * n_kf, [[] for _ in range(n_kf)], [[] for _ in range(n_kf)]
    covis[seed[0]] = last[:4] + prev[:4] + [last[4]]              # eight marked keyframes of the two wrapping chains, then one of them that is not
    children[seed[0]] = one[:5] + [one[5]]                        # likewise in the long chain
    covis[seed[1]] = [last[4], prev[4]]                           # the first was marked a moment ago
    parent[seed[2]] = last[5]                                     # joins and ends the row
    covis[seed[3]] = [prev[5]]
    other = sorted(one[:3] + last[3:6] + prev[1:3] + [5, 6, 7, 8, 9])
    covis[other[0]] = one[:3] + [one[3]]
    a, refs = _kf_check([seed, other, seed], covis, children, parent, 24, dense=1)
    assert refs[0] == seed + [last[4], one[5], prev[4], last[5]] and refs[1][13] == one[3]
    b, _ = _kf_check([seed, other, seed], covis, children, parent, 24)
    _same(a, b)


@pytest.mark.parametrize("n_rows", [1, 2, 300])
def test_many_rows_with_differing_seeds_in_one_call(n_rows):
    rng, parent, children, covis, kf_bad = _kf_world(5 + n_rows)
    seeds = _seeds(rng, len(parent), kf_bad, [int(x) for x in rng.integers(0, 90, n_rows)])
    a, _ = _kf_check(seeds, covis, children, parent, 100, kf_bad=kf_bad)
    b, _ = _kf_check(seeds, covis, children, parent, 100, kf_bad=kf_bad, dense=1)
    _same(a, b)


def test_children_csr_is_the_set_order_of_the_parent_array():
    import torch
    from rgbd_pl_slam_amd import children_csr
    rng, parent, children, _, kf_bad = _kf_world(8, n_kf=150)
    key = [int(k) for k in rng.permutation(150).astype(np.int64) * 0x10001 + 0x7f0000000000]
    for k_, b_ in ((None, None), (key, None), (key, kf_bad)):
        start, flat = children_csr(_dev(parent, np.int32), None if k_ is None else _dev(k_, np.int64), None if b_ is None else _dev(b_, np.uint8))
        torch.cuda.synchronize()
        start, flat = start.cpu().numpy(), flat.cpu().numpy()
        for p in range(150):
            want = sorted((c for c in children[p] if not (b_ and b_[c])), key=lambda c: c if k_ is None else k_[c])
            assert flat[start[p]:start[p + 1]].tolist() == want, p


# ---------------------------------------------------------------------------------------------------------------- items
def _items_check(local, rows, n_items, item_stride, item_bad=None, frame_rows=None, table=0, kf_stride=None, with_seen=True, filler=((), (0,))):
    import torch
    from rgbd_pl_slam_amd import local_items
    n_rows = len(local)
    kf_stride = kf_stride or max(1, max((len(x) for x in local), default=1))
    d_lk, d_nlk = _padded(local, kf_stride, BIG)
    rs, ri = _csr(rows, *filler)
    fs, fi = _csr(frame_rows, *filler) if frame_rows is not None else (None, None)
    out = _Sent(item=((n_rows, item_stride), torch.int32), n=((n_rows,), torch.int32), seen=((n_rows, item_stride), torch.uint8), status=((n_rows,), torch.int32))
    local_items(d_lk, d_nlk, rs, ri, n_items, item_bad=None if item_bad is None else _dev(item_bad, np.uint8), frame_row_start=fs, frame_row_item=fi,
                table_slots=table, out=(out.view["item"], out.view["n"], out.view["seen"] if with_seen else None, out.view["status"]))
    h = out.host()
    for name, size in (("item", n_rows * item_stride), ("n", n_rows), ("status", n_rows)):
        assert (h[name][size:] == SENT).all(), (name, "guard overwritten")
    assert (h["seen"][n_rows * item_stride if with_seen else 0:] == 0xA5).all(), "seen: guard overwritten"
    refs = []
    for r, lk in enumerate(local):
        want, seen = R.local_items(lk[:kf_stride], rows, n_items, item_bad, None if frame_rows is None else frame_rows[r])
        refs.append((want, seen))
        k = min(len(want), item_stride)
        row = h["item"][r * item_stride:(r + 1) * item_stride]
        assert h["n"][r] == len(want), (r, "count", int(h["n"][r]), len(want))
        assert row[:k].tolist() == want[:k], (r, row[:8].tolist(), want[:8])
        assert (row[k:] == SENT).all(), (r, "written behind the count")
        assert h["status"][r] == (4 if len(want) > item_stride else 0), (r, "status")
        if with_seen:
            srow = h["seen"][r * item_stride:(r + 1) * item_stride]
            assert srow[:k].tolist() == seen[:k] and (srow[k:] == 0xA5).all(), (r, "seen")
    return h, refs


def _split(rng, ids, parts):
    """ids cut into `parts` consecutive keyframe rows, one of them empty"""
    cuts = sorted(int(x) for x in rng.integers(0, len(ids) + 1, parts - 2)) if parts > 2 else []
    cuts = [0] + cuts + [len(ids), len(ids)]
    return [ids[a:b] for a, b in zip(cuts[:-1], cuts[1:])]


def _length_world(lengths, n_items=700, seed=0):
    rng = np.random.default_rng(seed)
    rows, local = [], []
    for L in lengths:
        ids = [int(x) for x in rng.integers(-1, n_items, L)]      # repeats, and -1 = null
        parts = _split(rng, ids, 4)
        local.append(list(range(len(rows), len(rows) + len(parts))))
        rows += parts
    item_bad = [int(x) for x in rng.integers(0, 9, n_items) == 0]
    frame_rows = [[int(x) for x in rng.integers(-1, n_items, 40)] + [BIG, -9] for _ in lengths]
    return rows, local, item_bad, frame_rows


def test_concatenated_lengths_at_the_segment_and_scan_edges_in_both_table_classes():
    lengths = [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025]
    rows, local, item_bad, frame_rows = _length_world(lengths)
    lds, refs = _items_check(local, rows, 700, 700, item_bad, frame_rows)                   # 8192 slots: every row in LDS
    glob, _ = _items_check(local, rows, 700, 700, item_bad, frame_rows, table=2)            # a limit of one position: global from length 2 on
    mixed, _ = _items_check(local, rows, 700, 700, item_bad, frame_rows, table=512)         # 256: both classes in one call
    again, _ = _items_check(local, rows, 700, 700, item_bad, frame_rows, table=512)
    _same(lds, glob); _same(lds, mixed); _same(lds, again)
    assert any(any(s) for _, s in refs) and any(not all(s) for _, s in refs if s)
    _items_check(local, rows, 700, 700, item_bad, None, table=512)                          # without the frame row: nothing is seen
    _items_check(local, rows, 700, 700, None, frame_rows, table=512, with_seen=False)


@pytest.mark.parametrize("table", [0, 64])
def test_one_id_two_thousand_times_and_repeats_inside_and_across_rows(table):
    rows = [[7] * 2000, [7, 8, 7, 9, 8], [9, 9, 10, 7]]
    _, refs = _items_check([[0, 1, 2], [2, 1, 0], [1], [0]], rows, 11, 6, None, [[8], [10, 10], [], [7]], table=table)
    assert [w for w, _ in refs] == [[7, 8, 9, 10], [9, 10, 7, 8], [7, 8, 9], [7]]
    assert [s for _, s in refs] == [[0, 1, 0, 0], [0, 1, 0, 0], [0, 0, 0], [1]]


def _ids_hashing_to(slot, slots, count, below=1 << 13):
    shift = 32 - (slots.bit_length() - 1)
    out = [i for i in range(below) if ((i * 2654435761) & 0xFFFFFFFF) >> shift == slot]
    assert len(out) >= count
    return out[:count]


def test_colliding_and_wrapping_ids_and_the_table_at_and_beyond_its_fill_limit():
    slots, n_items = 64, 1 << 13
    same = _ids_hashing_to(5, slots, 32)                          # all in one chain
    wrap = _ids_hashing_to(63, slots, 10) + _ids_hashing_to(62, slots, 10)   # chains that run over the table's end
    full = same[::-1]                                             # 32 positions: the limit of 64 slots
    rows = [same[:20] + same[:5], wrap + wrap[:10], full, full + [same[0]], wrap + same[:12]]
    frame_rows = [same[3:6], wrap[8:12], [], same[:1], [wrap[0], same[12]]]
    h, refs = _items_check([[0], [1], [2], [3], [4], [0, 1]], rows, n_items, 48, None, frame_rows + [same[:2]], table=slots)
    assert [len(w) for w, _ in refs] == [20, 20, 32, 32, 32, 40]
    g, _ = _items_check([[0], [1], [2], [3], [4], [0, 1]], rows, n_items, 48, None, frame_rows + [same[:2]], table=2)
    _same(h, g)


def test_item_stride_overflow_out_of_range_ids_and_slots():
    rows, local, item_bad, frame_rows = _length_world([300, 40, 9, 700], seed=3)
    clean, refs = _items_check(local, rows, 700, 10, item_bad, frame_rows)
    assert [len(w) > 10 for w, _ in refs] == [True, True, False, True]
    junk = [-5, 700, BIG, -2 ** 31]
    d_rows = [junk + r + junk for r in rows]
    d_local = [junk[:2] + lk + [len(rows), -1] for lk in local]
    fill = tuple(junk) * 2
    for table in (0, 16):
        dirty, _ = _items_check(d_local, d_rows, 700, 10, item_bad, frame_rows, table=table, filler=(fill, fill * 30))
        _same(clean, dirty)
    h, _ = _items_check(local, rows, 700, 10, item_bad, frame_rows, kf_stride=2)             # the keyframe list cut at its stride
    assert not np.array_equal(h["n"], clean["n"])


# ---------------------------------------------------------------------------------------------------------------- gather, visible
@pytest.mark.parametrize("pos_floats", [3, 6])
def test_gather_equals_fancy_indexing_and_skips_a_null_output(pos_floats):
    import torch
    from rgbd_pl_slam_amd import local_items, local_gather
    rng = np.random.default_rng(pos_floats)
    M, stride = 500, 130
    rows = [[int(x) for x in rng.integers(0, M, n)] for n in (120, 100, 5, 0)]
    d_lk, d_n = _padded([[0], [2], [3], [1, 0, 2]], 4, -1)
    item, n_item, _, _ = local_items(d_lk, d_n, *_csr(rows), M, stride)
    src = dict(world_pos=rng.normal(size=(M, pos_floats)).astype(np.float32), normal=rng.normal(size=(M, 3)).astype(np.float32),
               min_distance=rng.uniform(size=M).astype(np.float32), max_distance=rng.uniform(size=M).astype(np.float32),
               desc=rng.integers(0, 256, (M, 32), dtype=np.uint8))
    d_src = {k: _dev(v) for k, v in src.items()}
    fill = {k: (0xA5 if v.dtype == np.uint8 else 7.5) for k, v in src.items()}
    out = {k: torch.full((4 * stride + 3,) + v.shape[1:], fill[k], dtype=d_src[k].dtype, device="cuda") for k, v in src.items() if k != "normal"}
    got = local_gather(item, n_item, out=out, **d_src)            # normal: given, but no output for it
    torch.cuda.synchronize()
    item, n_item = item.cpu().numpy(), n_item.cpu().numpy()
    assert 0 < n_item[1] <= 5 and n_item[2] == 0 and 64 < n_item[0] <= stride and n_item[3] > stride
    for k, v in got.items():
        v = v.cpu().numpy()
        assert (v[4 * stride:] == fill[k]).all(), (k, "guard")
        for r in range(4):
            n = min(int(n_item[r]), stride)
            assert np.array_equal(v[r * stride:r * stride + n], src[k][item[r, :n]]), (k, r)
            assert (v[r * stride + n:(r + 1) * stride] == fill[k]).all(), (k, r, "written behind the count")
    full = local_gather(_dev(item), _dev(n_item), **d_src)        # the mirror's own outputs, every array
    torch.cuda.synchronize()
    assert np.array_equal(full["normal"].cpu().numpy()[:stride][:min(int(n_item[0]), stride)], src["normal"][item[0, :min(int(n_item[0]), stride)]])


def test_visible_counts_with_two_frames_sharing_points():
    import torch
    from rgbd_pl_slam_amd import local_items, local_visible
    rng = np.random.default_rng(11)
    M, stride = 300, 140
    rows = [[int(x) for x in rng.integers(0, M, n)] for n in (100, 80, 60)]
    item_bad = [int(x) for x in rng.integers(0, 8, M) == 0]
    local = [[0, 1], [1, 2]]                                      # the frames share keyframe 1
    frame_rows = [[int(x) for x in rng.integers(-1, M, 50)] + [rows[0][0], rows[0][0]], [int(x) for x in rng.integers(-1, M, 50)] + [M, BIG]]
    d_lk, d_n = _padded(local, 2, -1)
    fs, fi = _csr(frame_rows)
    d_bad = _dev(item_bad, np.uint8)
    item, n_item, seen, _ = local_items(d_lk, d_n, *_csr(rows), M, stride, d_bad, fs, fi)
    frustum = rng.integers(0, 2, (2, stride)).astype(np.uint8)
    start = rng.integers(0, 50, M).astype(np.int32)
    iv = torch.full((2 * stride + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    iv[:2 * stride] = _dev(frustum).reshape(-1)
    vis = _dev(np.concatenate([start, np.full(GUARD, SENT, np.int32)]))
    n_to = torch.full((2 + GUARD,), SENT, dtype=torch.int32, device="cuda")
    local_visible(item, n_item, seen, iv, vis[:M], fs, fi, d_bad, n_to_match=n_to[:2])
    torch.cuda.synchronize()
    want_vis = start.tolist()
    for r in range(2):
        want, _ = R.local_items(local[r], rows, M, item_bad, frame_rows[r])
        assert len(want) <= stride
        in_view, n_match = R.search_local_head(want, frustum[r], M, item_bad, frame_rows[r], want_vis)
        got = iv[r * stride:(r + 1) * stride].cpu().numpy()
        assert got[:len(want)].tolist() == in_view and (got[len(want):] == 0).all() and int(n_to[r]) == n_match, r
        assert 0 < n_match < int(frustum[r, :len(want)].sum())    # some in the frustum were seen already
    assert vis.cpu().numpy()[:M].tolist() == want_vis and (vis.cpu().numpy()[M:] == SENT).all()
    assert (iv[2 * stride:].cpu().numpy() == 0xA5).all() and (n_to[2:].cpu().numpy() == SENT).all()
    assert want_vis[rows[0][0]] >= start[rows[0][0]] + (0 if item_bad[rows[0][0]] else 2)   # listed twice in the own row: raised twice
    # without the map's counter and without seen: in_view is only cut at the counts
    iv2 = _dev(frustum).reshape(-1).clone()
    n2 = local_visible(item, n_item, None, iv2)
    torch.cuda.synchronize()
    n_host = n_item.cpu().numpy()
    assert n2.tolist() == [int(frustum[r, :n_host[r]].sum()) for r in range(2)]


# ---------------------------------------------------------------------------------------------------------------- end to end
def test_votes_to_matches_chain_equals_the_chain_with_a_host_middle():
    """local_keyframe_votes -> update_local_map -> local_gather -> plf_frustum_points -> local_visible -> plf_match_project_points on a map of 30
    keyframes, on the device end to end; the matches must equal those of the same chain with the middle (expansion, local points, gather, the
    seen rule) done by tests/localmapref.py and numpy on the host.  The geometry is tests/kfgen.py's keyframe scene (rgbd_pl_slam_amd.matchgen has
    no world positions), the descriptor noise matchgen's."""
    import torch
    import kfgen
    import covisref
    from rgbd_pl_slam_amd import Matcher, frame, local_keyframe_votes, update_connections, update_local_map, local_gather, local_visible, children_csr
    nk, m, n_kf, stride = 1200, 2500, 30, 2048
    c = kfgen.keyframe_scene(77, nk, m)
    p, pose = c["pts"], c["pose"]
    rng = np.random.default_rng(78)
    base = rng.integers(0, n_kf, m)                               # a point is seen from a window of eight consecutive keyframes
    obs = [sorted({int(base[i] + d) % n_kf for d in rng.choice(8, int(rng.integers(1, 7)), replace=False)}) for i in range(m)]
    rows = [[i for i in range(m) if k in obs[i]] for k in range(n_kf)]
    for k in range(0, n_kf, 3):
        rows[k].insert(1, -1)
    point_bad = [int(x) for x in rng.integers(0, 25, m) == 0]
    kf_bad = [int(k in (4, 17)) for k in range(n_kf)]
    parent = [-1] + [int(rng.integers(0, k)) for k in range(1, n_kf)]
    own = [int(x) for x in rng.choice(np.flatnonzero((base >= 3) & (base < 6)), 60, replace=False)] + [-1, -1]
    rs, rp = _csr(rows)
    os_, ok = _csr(obs)
    fs, fi = _csr([own])
    d_pbad, d_kbad, d_par = _dev(point_bad, np.uint8), _dev(kf_bad, np.uint8), _dev(parent, np.int32)
    cov = update_connections(rs, rp, torch.arange(n_kf, dtype=torch.int32, device="cuda"), os_, ok, n_kf, n_kf, 15, d_pbad)
    votes = local_keyframe_votes(fs, fi, os_, ok, n_kf, n_kf, d_pbad, d_kbad)
    cstart, ckf = children_csr(d_par, kf_bad=d_kbad)
    lm = update_local_map(votes, cov, cstart, ckf, d_par, rs, rp, m, stride, kf_stride=40, kf_bad=d_kbad, item_bad=d_pbad, frame_row_start=fs,
                          frame_row_item=fi, max_local=80)
    d_map = dict(world_pos=_dev(p["xw"]), normal=_dev(p["normal"]), min_distance=_dev(p["min_dist"]), max_distance=_dev(p["max_dist"]), desc=_dev(p["desc"]))
    g = local_gather(lm.local_item, lm.n_local_item, **d_map)
    cam = frame.camera(**dict(frame.TUM1, fx=pose["fx"], fy=pose["fy"], cx=pose["cx"], cy=pose["cy"], bf=pose["bf"]))
    fpose = dict(Rcw=pose["Rcw"], tcw=pose["tcw"], Ow=pose["Ow"])

    def frustum(a):
        out = dict(proj_x=torch.zeros(stride, device="cuda"), proj_y=torch.zeros(stride, device="cuda"), proj_xr=torch.zeros(stride, device="cuda"),
                   level=torch.zeros(stride, dtype=torch.int32, device="cuda"), view_cos=torch.zeros(stride, device="cuda"),
                   in_view=torch.zeros(stride, dtype=torch.uint8, device="cuda"))
        frame.frustum_points(a["world_pos"], a["normal"], a["min_distance"], a["max_distance"], fpose, cam, c["bounds"], pose["log_scale_factor"], 8, 0.5, out)
        return out

    mt = Matcher(max_keypoints=2048, max_mappoints=stride)
    keys = torch.from_numpy(np.frombuffer(np.ascontiguousarray(c["kps"]).tobytes(), np.uint8).copy()).cuda()
    d_desc, d_sc, d_ur = _dev(c["desc"]), _dev(c["scale"]), _dev(c["uright"])

    def project(fo, desc):
        mp = dict(fo); mp["desc"] = desc
        torch.cuda.synchronize()                                  # the matcher runs on its own stream
        match = torch.full((nk,), -1, dtype=torch.int32, device="cuda"); nm = torch.zeros(1, dtype=torch.int32, device="cuda")
        mt.SearchByProjection([Matcher.frame_view(nk, keys, d_desc, d_sc, c["bounds"], d_ur)], mp, 3.0, 0.8, match, nk, nm)
        torch.cuda.synchronize()
        return match.cpu().numpy(), int(nm[0])

    fo = frustum(g)
    n_to = local_visible(lm.local_item, lm.n_local_item, lm.seen, fo["in_view"])
    got = project(fo, g["desc"])
    # ---- the host middle
    ref_cov = [covisref.update_connections(row, s, obs, n_kf, 15, point_bad) for s, row in enumerate(rows)]
    covis = [[k for k, _ in e["ord"]] if e else [] for e in ref_cov]
    seed = [k for k, _ in covisref.local_keyframe_votes(own, obs, n_kf, point_bad, kf_bad)["conn"]]
    children = [[k for k in range(n_kf) if parent[k] == s and not kf_bad[k]] for s in range(n_kf)]
    lkf = R.local_keyframes(seed, covis, children, parent, kf_bad, 10, 80)
    items, seen = R.local_items(lkf, rows, m, point_bad, own)
    assert len(lkf) > len(seed) and 300 < len(items) <= stride and sum(seen) > 20
    assert lm.local_kf[0, :len(lkf)].tolist() == lkf and int(lm.n_local_kf[0]) == len(lkf) and int(lm.status[0]) == 0
    assert lm.local_item[0, :len(items)].tolist() == items and (lm.local_item[0, len(items):] == -1).all() and int(lm.ref_kf[0]) == int(votes.max_kf[0])
    idx = np.array(items)
    pad = lambda a: _dev(np.concatenate([a[idx], np.zeros((stride - len(idx),) + a.shape[1:], a.dtype)]))   # noqa: E731
    h = dict(world_pos=pad(p["xw"]), normal=pad(p["normal"]), min_distance=pad(p["min_dist"]), max_distance=pad(p["max_dist"]), desc=pad(p["desc"]))
    fr = frustum(h)
    torch.cuda.synchronize()
    iv = fr["in_view"].cpu().numpy()
    iv[:len(items)] &= 1 - np.array(seen, np.uint8)
    iv[len(items):] = 0
    fr["in_view"] = _dev(iv)
    exp = project(fr, h["desc"])
    assert int(n_to[0]) == int(iv.sum()) and 0 < int(iv.sum())
    assert np.array_equal(fo["in_view"].cpu().numpy(), iv)
    assert got[1] == exp[1] and exp[1] > 50 and np.array_equal(got[0], exp[0])

"""Inputs of tests/test_gpu_orb_front.py and their CPU side: small images that put k_orb_level (rgbd_pl_slam_amd/csrc/orb_front.hip) and k_orient_brief
(orb_kernels.hip) into each of their situations, and a numpy MODEL of the schedule k_orb_level runs on them: the cell and tile geometry, the capacity of the
survivor list, and the survivors of the pre-test per (level, tile, pass) and per row half.  The model decides nothing about results -- those come from the
oracle -- it only says which path an input takes (tests/test_orb_front_cases.py asserts it).  Test / model code only.

Geometry of every image here (octree_cases.W, H, NLEVELS = 192 x 144, 3 levels), level 0: 5 x 3 FAST cells of 32 x 38 with the computed regions
x [19, 51) [51, 83) [83, 115) [115, 147) [147, 173), y [19, 57) [57, 95) [95, 125); 3 x 2 tiles of 2 x 2 cells, so x = 83 and x = 147 are tile borders too,
and y = 95.  Key points exist for 19 <= x <= 172 = W - 20, 19 <= y <= 124 = H - 20."""
import ctypes as C
import math

import numpy as np

import orc
import octree_cases as oc

W, H, NLEVELS, EDGE, MINB = oc.W, oc.H, oc.NLEVELS, 19, 16
NF = 100      # quotas 40 / 33 / 27: every candidate of the sparse images becomes a key point
INI, MIN = 20, 7
BG = 60


# ---------------------------------------------------------------------------------------------------------------- the model
def level_sizes(w, h, scale_factor, nlevels):
    """the constructor's scale table and ComputePyramid's level sizes, in the reference's float arithmetic"""
    sf = float(np.float32(scale_factor))
    scale = [np.float32(1)]
    for _ in range(1, nlevels):
        scale.append(np.float32(float(scale[-1]) * sf))
    inv = [np.float32(1) / s for s in scale]
    rnd = lambda v: int(np.rint(v))   # cvRound: to nearest even
    return [(rnd(np.float32(w) * i), rnd(np.float32(h) * i)) for i in inv]


def level_geometry(lw, lh):
    """cell rule of ComputeKeyPointsOctTree on a level of lw x lh and the tiling k_orb_level lays over it (2 x 2 cells per workgroup).  None if the reference
    cannot tile the level.  cells: (x0, y0, w, h) of the sub-images handed to cv::FAST, which computes each minus a 3-pixel frame."""
    f32 = np.float32
    minb, maxbx, maxby = MINB, lw - MINB, lh - MINB
    width, height = f32(maxbx - minb), f32(maxby - minb)
    ncols, nrows = int(width / f32(30)), int(height / f32(30))
    if ncols < 1 or nrows < 1:
        return None
    wcell, hcell = int(math.ceil(width / f32(ncols))), int(math.ceil(height / f32(nrows)))
    xs = [j for j in range(ncols) if not minb + j * wcell >= maxbx - 6]
    ys = [i for i in range(nrows) if not minb + i * hcell >= maxby - 3]
    cells = [(minb + j * wcell, minb + i * hcell, min(minb + j * wcell + wcell + 6, maxbx) - (minb + j * wcell),
              min(minb + i * hcell + hcell + 6, maxby) - (minb + i * hcell)) for i in ys for j in xs]
    ncx, ncy = len(xs), len(ys)
    g = dict(w=lw, h=lh, wCell=wcell, hCell=hcell, ncx=ncx, ncy=ncy, cells=cells, tcx=(ncx + 1) // 2, tcy=(ncy + 1) // 2,
             rex=min(minb + (ncx - 1) * wcell + wcell + 6, maxbx) - 3, rey=min(minb + (ncy - 1) * hcell + hcell + 6, maxby) - 3)
    g["tiles"] = [_tile(g, tx, ty) for ty in range(g["tcy"]) for tx in range(g["tcx"])]
    return g


def _tile(g, tx, ty):
    """bounding box [rx0, rx1) x [ry0, ry1) of the computed regions of the tile's cells, where its second cell column / row starts (xm, ym: clamped, the last
    cell of a level may have no computed region and the one before it a shortened one), and the regions per cell in the kernel's order (wave = cell)"""
    wc, hc = g["wCell"], g["hCell"]
    cx0, cx1, cy0, cy1 = 2 * tx, min(2 * tx + 2, g["ncx"]), 2 * ty, min(2 * ty + 2, g["ncy"])
    rx0, rx1 = EDGE + cx0 * wc, g["rex"] if cx1 == g["ncx"] else EDGE + cx1 * wc
    ry0, ry1 = EDGE + cy0 * hc, g["rey"] if cy1 == g["ncy"] else EDGE + cy1 * hc
    xm = min(rx0 + wc, rx1) if cx1 - cx0 == 2 else rx1
    ym = min(ry0 + hc, ry1) if cy1 - cy0 == 2 else ry1
    regions = {}
    for wv in range(4):
        cx, cy = cx0 + (wv & 1), cy0 + (wv >> 1)
        if cx < cx1 and cy < cy1:
            regions[wv] = ((xm, rx1) if wv & 1 else (rx0, xm)) + ((ym, ry1) if wv >> 1 else (ry0, ym)) + (cy * g["ncx"] + cx,)
    # column groups of 4 the pre-test deals its threads to
    ex0 = (rx0 & ~3) - 4
    ngr = ((((rx1 - 1 - ex0) & ~3) - ((rx0 - ex0) & ~3)) >> 2) + 1
    return dict(tx=tx, ty=ty, rx0=rx0, rx1=rx1, ry0=ry0, ry1=ry1, xm=xm, ym=ym, regions=regions, ngr=ngr)


def accepted(geoms):
    """what orb_configure asks of every tile: a non-empty bounding box inside the padded plane, coordinates that pack into 8 bits, one wave per cell"""
    for g in geoms:
        if g is None or 2 * g["wCell"] > 250 or 2 * g["hCell"] > 250 or any(c[2] - 6 > 64 or c[3] - 6 > 64 for c in g["cells"]):
            return False
        for t in g["tiles"]:
            if t["rx1"] <= t["rx0"] or t["ry1"] <= t["ry0"]:
                return False
            ex0 = (t["rx0"] & ~3) - 4
            ew = ((t["rx1"] - 1) & ~3) + 8 - ex0
            if ex0 < -EDGE or ex0 + ew > g["w"] + EDGE or t["ry1"] + 3 > g["h"] + EDGE or ew > 255 or t["ry1"] - t["ry0"] > 255:
                return False
    return True


def list_cap(geoms):
    """entries of the survivor list: half the rows of the tallest tile region times the widest one -- maxima over the tiles of ALL levels -- plus one group"""
    rw = max(t["rx1"] - t["rx0"] for g in geoms for t in g["tiles"])
    rh = max(t["ry1"] - t["ry0"] for g in geoms for t in g["tiles"])
    return rw * ((rh + 1) // 2) + 4


def pretest(plane, t):
    """the pre-test of k_orb_level on a padded level plane (19 pixels of border): for every level pixel, whether two adjacent ones of the four compass points of the
    FAST ring are both brighter than the centre by more than t, or both darker"""
    p = plane.astype(np.int16)
    h, w = p.shape[0] - 2 * EDGE, p.shape[1] - 2 * EDGE
    at = lambda dx, dy: p[EDGE + dy: EDGE + dy + h, EDGE + dx: EDGE + dx + w]
    c = at(0, 0)
    dn, ds, de, dw = at(0, 3) - c, at(0, -3) - c, at(3, 0) - c, at(-3, 0) - c
    return (np.minimum(np.maximum(dn, ds), np.maximum(de, dw)) > t) | (np.maximum(np.minimum(dn, ds), np.minimum(de, dw)) < -t)


_RING = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1), (-2, 2), (-1, 3)]


def fast_corners(plane, t):
    """FAST-9/16 at threshold t, before any suppression: 9 contiguous ring pixels all brighter than centre + t or all darker than centre - t.  These are the
    survivors whose exact score reaches t, i.e. what the suppression of k_orb_level queues"""
    p = plane.astype(np.int16)
    h, w = p.shape[0] - 2 * EDGE, p.shape[1] - 2 * EDGE
    c = p[EDGE: EDGE + h, EDGE: EDGE + w]
    ring = np.stack([p[EDGE + dy: EDGE + dy + h, EDGE + dx: EDGE + dx + w] for dx, dy in _RING])
    out = np.zeros((h, w), bool)
    for flags in (ring > c + t, ring < c - t):
        for k in range(16):
            out |= np.all(flags[[(k + j) & 15 for j in range(9)]], 0)
    return out


def fast_cells(plane, ini_th, min_th):
    """the oracle's cell loop on a padded plane: candidates [n, 3] = x, y relative to the border (16, 16), response"""
    plane = np.ascontiguousarray(plane)
    lh, lw, pp = plane.shape[0] - 2 * EDGE, plane.shape[1] - 2 * EDGE, plane.shape[1]
    buf = np.zeros(lw * lh + 16, orc.KP_DTYPE)
    nc = C.c_int(0)
    n = orc.lib().orc_fast_cells(C.c_void_p(plane.ctypes.data + EDGE * pp + EDGE), C.c_int(lw), C.c_int(lh), C.c_ssize_t(pp), C.c_int(ini_th), C.c_int(min_th),
                                 orc.p(buf), C.c_int(len(buf)), C.byref(nc))
    return np.stack([buf["x"][:n], buf["y"][:n], buf["response"][:n]], 1).astype(np.float32)


def _count(mask, x0, x1, y0, y1):
    return int(mask[y0:y1, x0:x1].sum())


def schedule(planes, ini_th=INI, min_th=MIN):
    """what k_orb_level goes through on the padded planes of a frame.  Per level a list of tiles, each a dict:
      A, B            survivors of the pre-test in pass A (iniThFAST, all cells) and pass B (minThFAST, the cells without a maximum at iniThFAST; 0 without pass B)
      A_over, B_over  the pass finds more than the list holds and is redone in two row halves
      A_half, B_half  survivors of the two row halves
      A_queue, B_queue  corners at the pass threshold in the largest list the pass scores (the whole pass, or a half): what the four waves queue between them
      emitted, need   cells of the tile (wave order) with / without a strict maximum at iniThFAST
    and the capacity of the list"""
    geoms = [level_geometry(p.shape[1] - 2 * EDGE, p.shape[0] - 2 * EDGE) for p in planes]
    cap = list_cap(geoms)
    out = []
    for g, plane in zip(geoms, planes):
        at_ini = fast_cells(plane, ini_th, ini_th)
        pre = {ini_th: pretest(plane, ini_th), min_th: pretest(plane, min_th)}
        crn = {ini_th: fast_corners(plane, ini_th), min_th: fast_corners(plane, min_th)}
        tiles = []
        for t in g["tiles"]:
            has = lambda r: bool(np.any((at_ini[:, 0] + MINB >= r[0]) & (at_ini[:, 0] + MINB < r[1]) & (at_ini[:, 1] + MINB >= r[2]) & (at_ini[:, 1] + MINB < r[3])))
            emitted = [wv for wv, r in t["regions"].items() if has(r)]
            need = [wv for wv in t["regions"] if wv not in emitted]
            hr = t["ry0"] + ((t["ry1"] - t["ry0"] + 1) >> 1)
            d = dict(tx=t["tx"], ty=t["ty"], emitted=emitted, need=need)
            for name, th, on in (("A", ini_th, list(t["regions"])), ("B", min_th, need)):
                cnt = lambda m, ya, yb: sum(_count(m, t["regions"][wv][0], t["regions"][wv][1], max(t["regions"][wv][2], ya), min(t["regions"][wv][3], yb)) for wv in on)
                n = cnt(pre[th], t["ry0"], t["ry1"])
                d[name] = n
                d[name + "_over"] = n + 4 > cap
                d[name + "_half"] = (cnt(pre[th], t["ry0"], hr), cnt(pre[th], hr, t["ry1"]))
                d[name + "_queue"] = max(cnt(crn[th], t["ry0"], hr), cnt(crn[th], hr, t["ry1"])) if d[name + "_over"] else cnt(crn[th], t["ry0"], t["ry1"])
            tiles.append(d)
        out.append(tiles)
    return out, cap, geoms


# ---------------------------------------------------------------------------------------------------------------- the pieces
def canvas(bg=BG, w=W, h=H):
    return np.full((h, w), bg, np.uint8)


def dot(img, x, y, v=230):
    img[y, x] = v


# satellites of a dot of 230: name -> (pixels relative to the dot, all of 70 on the background of 60; angle of the key point as float32 bits)
SATELLITES = {
    "none": ([], 0x00000000),                                   # both moments 0
    "right": ([(10, -1), (10, 0), (10, 1)], 0x00000000),        # m01 = 0, m10 > 0: 0.0
    "below": ([(-1, 10), (0, 10), (1, 10)], 0x42B40000),        # 90.0
    "left": ([(-10, -1), (-10, 0), (-10, 1)], 0x43340000),      # 180.0
    "above": ([(-1, -10), (0, -10), (1, -10)], 0x43870000),     # 270.0
    "45": ([(8, 8)], 0x4233F639),                               # 44.990452: fastAtan2 is a polynomial, not exact on the diagonal
    "315": ([(8, -8)], 0x439D8139),                             # 315.009552
    "135": ([(-8, 8)], 0x43070272),                             # 135.009552
}


def satellite(img, x, y, name):
    dot(img, x, y)
    for dx, dy in SATELLITES[name][0]:
        img[y + dy, x + dx] = 70


# where the satellite set stands in the interior: dot positions, >= 32 pixels apart.  The dot of "135" is in cell column 4 and its satellite in column 3, alone
# there, so that the retry finds it; every other satellite shares its dot's cell.
SAT_AT = {"none": (40, 38), "below": (88, 38), "above": (128, 38), "left": (163, 38), "right": (40, 76), "45": (88, 76), "315": (128, 76), "135": (150, 103)}
LADDER_AT = {7: (35, 38), -7: (67, 38), 8: (99, 38), -8: (131, 38), 20: (35, 76), -20: (67, 76), 21: (99, 76), -21: (131, 76)}
PAIRS_AT = {"inside": (35, 38), "corner": (82, 56), "horizontal": (160, 56), "vertical": (114, 105), "tile border": (82, 110)}
EXTREMES = [(19, 19), (W - 20, 19), (19, H - 20), (W - 20, H - 20)]
OUTSIDE = [(18, 70), (W - 19, 70), (96, 18), (96, H - 19)]


def ladder():
    """one dot per cell on 60: contrasts +-7 (nothing), +-8 (response 7, retry), +-20 (response 19, retry), +-21 (response 20, the first call), and 230 (169)"""
    img = canvas()
    for c, (x, y) in LADDER_AT.items():
        dot(img, x, y, BG + c)
    dot(img, 160, 76)
    return img


def top_of_the_score():
    """255 on 0: response 254, the largest a score byte takes"""
    img = canvas(0)
    dot(img, 96, 70, 255)
    return img


def strong_and_weak():
    """a contrast-21 dot and a contrast-8 dot in ONE cell: only the strong one, the retry runs for empty cells only"""
    img = canvas()
    dot(img, 24, 24, BG + 21)
    dot(img, 46, 50, BG + 8)
    return img


def plateaus():
    """two adjacent pixels of 230, and a 1-pixel line of 230 with both ends inside cells: equal scores above iniThFAST without a strict maximum -- the cells go to the
    second pass and stay empty"""
    img = canvas()
    img[38, 35:37] = 230
    img[76, 96:135] = 230
    return img


def diagonal_pairs():
    """230 at (x, y) and 200 at (x + 1, y + 1): one candidate inside a cell, two where a cell border lies between them -- the vertical one at x = 115 inside a tile, the
    one at x = 83 between two tiles, the horizontal one at y = 57, and the corner (83, 57) where four cells and two tiles meet"""
    img = canvas()
    for x, y in PAIRS_AT.values():
        dot(img, x, y, 230)
        dot(img, x + 1, y + 1, 200)
    return img


def extremes():
    """dots on the first and last row / column that yield key points, and dots one pixel further out"""
    img = canvas()
    for x, y in EXTREMES + OUTSIDE:
        dot(img, x, y)
    return img


def satellites():
    """the satellite set in the interior: angles 0 (no moment at all), 0, 90, 180, 270 exactly and the three diagonals"""
    img = canvas()
    for name, (x, y) in SAT_AT.items():
        satellite(img, x, y, name)
    return img


def corner_satellites(name):
    """the same satellite at the dots (19, 19) and (W - 20, H - 20): the disc of the moments and the rotated pattern reach furthest into the level's border"""
    img = canvas()
    satellite(img, 19, 19, name)
    satellite(img, W - 20, H - 20, name)
    return img


def one_block():
    """a 2 x 2 block of 230: four equal scores at level 0, candidates at levels 1 and 2 only (the offset walk of k_orient_brief starts with a count of 0)"""
    img = canvas()
    img[70:72, 90:92] = 230
    return img


def dense_high():
    """uniform noise: pass A finds more survivors than the list holds in every tile of 2 x 2 cells"""
    return oc.noise(5)


def _low(seed, w=W, h=H):
    """three grey values 8 apart (a range of 16 < iniThFAST: no pixel passes at 20), mostly a checkerboard -- all four compass points of the ring differ from the
    centre -- with a quarter of the pixels redrawn at random, which makes the corners"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    v = ((xx + yy) & 1) * 2
    r = rng.random((h, w)) < 0.25
    v = np.where(r, rng.integers(0, 3, (h, w)), v)
    return (100 + 8 * v).astype(np.uint8)


def dense_low():
    """every cell empty at iniThFAST, pass B over the list in every tile of 2 x 2 cells"""
    return _low(2)


def two_valued():
    """two grey values 12 apart, a fifth of the pixels the brighter one: a pass B that fits the list (no row halves) and in which a third of the survivors are corners
    at minThFAST, so that its suppression queues wrap"""
    return (100 + 12 * (np.random.default_rng(4).random((H, W)) < 0.2)).astype(np.uint8)


def mixed(bx=51, by=57):
    """uniform noise left of bx and above by, the low image elsewhere: with (51, 57), the borders of cell (0, 0), tile (0, 0) emits that cell in pass A and redoes the
    other three in halves in pass B.  (A tile split in two equal parts cannot do that: half a tile's pixels fit the list.)"""
    img = _low(3)
    img[:by, :bx] = oc.noise(6)[:by, :bx]
    return img


def mixed_in_cell():
    """the same with the boundary inside cell (0, 0)"""
    return mixed(40, 45)


def low_128_6():
    """the `low` image of test_orb_flat_and_noise_images (tests/test_gpu_orb.py), 640 x 480: 128 +- 6"""
    rng = np.random.default_rng(7)
    rng.integers(0, 256, (480, 640), dtype=np.uint8)
    return (128 + rng.integers(-6, 7, (480, 640))).astype(np.uint8)


# name -> image; what each is for is asserted on the CPU in tests/test_orb_front_cases.py
CASES = {
    "ladder": ladder, "top of the score": top_of_the_score, "strong and weak": strong_and_weak, "plateaus": plateaus, "diagonal pairs": diagonal_pairs,
    "extremes": extremes, "satellites": satellites, "one block": one_block,
    "dense high": dense_high, "dense low": dense_low, "two-valued": two_valued, "mixed": mixed, "mixed in cell": mixed_in_cell,
}
CASES.update({"corner " + n: (lambda n=n: corner_satellites(n)) for n in SATELLITES if n != "none"})
DENSE = ("dense high", "dense low", "two-valued", "mixed", "mixed in cell")
_REF = {}


def ref(name):
    """image, per-level candidates (octree_cases.level_candidates), oracle result with stages: computed once, never modified"""
    if name not in _REF:
        img = CASES[name]()
        img.setflags(write=False)
        lv, r = oc.level_candidates(img, NF)
        _REF[name] = (img, lv, r)
    return _REF[name]


# batches of the GPU test: (frames, first named image).  9, 11 and 17 frames leave the last group of 8 frames of k_orient_brief partial.
BATCHES = [(1, 0), (8, 0), (9, 5), (11, 11), (17, 19)]


def batch_names(B, start):
    """flat frames (None) at both ends and in the middle, the named images from `start` on in between; a batch of one is a full frame"""
    names = list(CASES)
    if B == 1:
        return ["dense high"]
    return [None if f in (0, B // 2, B - 1) else names[(start + f - 1 - (f > B // 2)) % len(names)] for f in range(B)]


_SCHED = {}


def sched(name):
    if name not in _SCHED:
        _SCHED[name] = schedule(ref(name)[2]["pyr"])
    return _SCHED[name]


# ---------------------------------------------------------------------------------------------------------------- parameter sets with clamped last cells
# The parameter sets of test_level_geometries_with_clamped_last_cells (tests/test_gpu_orb.py) at the smallest sizes that keep the property, which level 0 has:
#   "row": the last cell row has no computed region and the one before it a shortened one.  ceil() makes nRows * hCell overshoot the height by < nRows, and the last
#          row loses its region at an overshoot of hCell - 6 + 2 >= 26: no level below 873 rows has it.  The width is the narrowest the reference accepts (its octree
#          wants round(width / height) >= 1 root at every level);
#   "column": the last tile is one cell column of 3 pixels, a single group of 4 columns: likewise no level below 723 columns.
# name -> (w, h, scaleFactor, nlevels, iniThFAST, minThFAST, nfeatures)
PARAM_SETS = {
    "row 1.1/8": (469, 873, 1.1, 8, 26, 5, 2000), "row 1.1/3": (456, 873, 1.1, 3, 38, 6, 3000), "row 1.3/5": (485, 873, 1.3, 5, 20, 7, 800),
    "column 1.1/8": (723, 140, 1.1, 8, 26, 5, 2000), "column 1.1/3": (723, 120, 1.1, 3, 38, 6, 3000), "column 1.3/5": (723, 176, 1.3, 5, 20, 7, 800),
}
PARAM_LEVEL = {name: (0, name.split()[0]) for name in PARAM_SETS}


def param_points(name):
    """the plateau pieces of a parameter set's image, in its last cell: an equal pair, a dot on the last computed row / column, a dot one pixel further out"""
    w, h = PARAM_SETS[name][:2]
    g = level_geometry(w, h)
    if PARAM_LEVEL[name][1] == "row":
        t = g["tiles"][-g["tcx"]]      # the last tile row's first tile; the dense piece is in its last
        return dict(pair=(t["rx0"] + 11, t["ry1"] - 10), accepted=(t["rx0"] + 41, t["ry1"] - 1), rejected=(t["rx0"] + 71, t["ry1"]))
    t = g["tiles"][g["tcx"] - 1]       # the last tile column's first tile
    return dict(pair=(t["rx0"], t["ry0"] + 10), accepted=(t["rx1"] - 1, t["ry0"] + 20), rejected=(t["rx1"], t["ry0"] + 30))


def param_image(name):
    """uniform noise over the last tile of level 0 (and a margin), the plateau pieces of param_points in the last cell row / column away from it"""
    w, h = PARAM_SETS[name][:2]
    g = level_geometry(w, h)
    last = g["tiles"][-1]
    img = canvas(BG, w, h)
    y0 = last["ry0"] - 12 if PARAM_LEVEL[name][1] == "row" else 60
    img[y0:, last["rx0"] - 12:] = oc.noise(8, 0, 256, w, h)[y0:, last["rx0"] - 12:]
    pts = param_points(name)
    img[pts["pair"][1], pts["pair"][0]: pts["pair"][0] + 2] = 230
    dot(img, *pts["accepted"])
    dot(img, *pts["rejected"])
    return img

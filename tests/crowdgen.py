"""Crowded and chain scenes for the greedy-order projection matchers (test data only).

matchgen / kfgen scatter their items over a whole VGA frame with near-random descriptors: items hardly ever want the same key point, the second-best distance is
about 128 and the ratio test never decides.  Here the key points sit in a few 40 x 40 px clusters on 2-3 adjacent octaves, descriptors come from a small alphabet
of base codes with 0-3 flipped bits (ties and near-ties everywhere), and many more items than key points aim at the clusters: the result depends on the order in
which the items are served.  Chain scenes give every item the SAME window, so the round schemes of match_kernels.hip decide one item per round while their
unfinished lists shrink across the 256-item chunk boundary.

Deterministic by seed.  Same KP_DTYPE and dict layouts as matchgen / kfgen: the orc.* wrappers, matchref and the Matcher views take the scenes unchanged."""
import numpy as np

from kfgen import KP_DTYPE, _rot, scales

F = np.float32
BOUNDS = (0.0, 0.0, 640.0, 480.0)
FX, FY, CX, CY, BF = 525.0, 525.0, 319.5, 239.5, 40.0
CROWD_SIZES = [(96, 1500, 4), (300, 3000, 6), (40, 600, 2), (500, 800, 8)]     # key points, items, base codes
CHAIN_ITEMS = [255, 256, 257, 513]
CACHED_MAX_MAPPOINTS = 4096     # a handle of this size (64 * 4096 pool entries per frame) caches every scene's candidates: none falls back


def alphabet_desc(rng, base, n, code=None):
    """n descriptors: a base code each (drawn, or given) with 0-3 flipped bits"""
    code = rng.integers(0, len(base), n) if code is None else code
    d = base[code].copy()
    for i in range(n):
        for b in rng.choice(256, int(rng.integers(0, 4)), replace=False):
            d[i, b >> 3] ^= np.uint8(1 << (b & 7))
    return d, code


def clustered_keypoints(rng, n, n_clusters=None, first_octave=None, n_octaves=None, box=40.0):
    """n key points in 2-6 clusters of box x box px on 2-3 adjacent octaves; cluster 0 lies against the left / top image border, so cell windows clamp there.
    Returns (kps, cluster of each key point)"""
    n_clusters = int(rng.integers(2, 7)) if n_clusters is None else n_clusters
    first_octave = int(rng.integers(0, 4)) if first_octave is None else first_octave
    n_octaves = int(rng.integers(2, 4)) if n_octaves is None else n_octaves
    cen = np.stack([rng.uniform(60, 580, n_clusters), rng.uniform(60, 420, n_clusters)], 1)
    cen[0] = (box / 2 - 4, box / 2 - 6)
    cl = rng.integers(0, n_clusters, n)
    kps = np.zeros(n, KP_DTYPE)
    kps["x"] = np.clip(cen[cl, 0] + rng.uniform(-box / 2, box / 2, n), 0.0, 639.0).astype(F)
    kps["y"] = np.clip(cen[cl, 1] + rng.uniform(-box / 2, box / 2, n), 0.0, 479.0).astype(F)
    kps["octave"] = first_octave + rng.integers(0, n_octaves, n)
    kps["angle"] = rng.uniform(0, 360, n).astype(F); kps["size"] = 31; kps["response"] = 1; kps["class_id"] = -1
    return kps, cl


def match_init(rng, n, with_obs, without_obs, minus3=True):
    """all kinds of entry: free, -2 (held by a point with observations), -3 (culled by an earlier check_orientation = 2 call: free), and indices set before the call
    that point at items with / without observations (with_obs / without_obs: item indices to draw from)"""
    init = np.full(n, -1, np.int32)
    u = rng.uniform(0, 1, n)
    init[u < 0.08] = -2
    if minus3:
        init[(u >= 0.08) & (u < 0.14)] = -3
    if len(with_obs):
        s = (u >= 0.14) & (u < 0.20); init[s] = rng.choice(with_obs, int(s.sum()))
    if len(without_obs):
        s = (u >= 0.20) & (u < 0.28); init[s] = rng.choice(without_obs, int(s.sum()))
    return init


def crowded_map(seed, n, m, a, obs_share, **kw):
    """frame with n clustered key points and m map points aimed at them.  Returns dict(kps, desc, uright, scale, bounds, mp, init)."""
    rng = np.random.default_rng(seed)
    sc = scales()
    kps, _ = clustered_keypoints(rng, n, **kw)
    base = rng.integers(0, 256, (a, 32), dtype=np.uint8)
    desc, code = alphabet_desc(rng, base, n)
    uright = np.where(rng.uniform(0, 1, n) < 0.5, kps["x"] - rng.uniform(2, 30, n), -1).astype(F)
    src = rng.integers(0, n, m)
    px = (kps["x"][src] + rng.uniform(-6, 6, m)).astype(F); py = (kps["y"][src] + rng.uniform(-6, 6, m)).astype(F)
    lvl = np.clip(kps["octave"][src] + rng.integers(0, 2, m), 0, 7).astype(np.int32)
    same = rng.uniform(0, 1, m) < 0.6     # the source key point's own base code, else any code of the alphabet
    mdesc, _ = alphabet_desc(rng, base, m, np.where(same, code[src], rng.integers(0, a, m)))
    view_cos = np.where(rng.uniform(0, 1, m) < 0.5, rng.uniform(0.9981, 1.0, m), rng.uniform(0.9, 0.9979, m)).astype(F)     # both RadiusByViewingCos classes
    proj_xr = np.where(uright[src] > 0, uright[src] + rng.normal(0, 1.5, m), px - rng.uniform(2, 30, m)).astype(F)
    obs = (rng.uniform(0, 1, m) < obs_share).astype(np.uint8) if 0.0 < obs_share < 1.0 else np.full(m, int(obs_share), np.uint8)
    mp = dict(proj_x=px, proj_y=py, proj_xr=proj_xr, level=lvl, view_cos=view_cos, in_view=(rng.uniform(0, 1, m) < 0.95).astype(np.uint8), desc=mdesc, obs_positive=obs)
    return dict(kps=kps, desc=desc, uright=uright, scale=sc, bounds=BOUNDS, mp=mp, init=match_init(rng, n, np.nonzero(obs)[0], np.nonzero(obs == 0)[0]))


def sparse_frame(seed, n, hit_x, hit_y, hit_octave, hit_desc, n_hit=30):
    """a frame of the matchgen kind: n key points spread over the whole image with random descriptors -- hardly any contest, small cell-window counts -- of which
    n_hit sit on items of the call (projection hit_x / hit_y, octave, descriptor), so that the frame still finds matches"""
    rng = np.random.default_rng(seed)
    kps = np.zeros(n, KP_DTYPE)
    kps["x"] = rng.uniform(0, 640, n).astype(F); kps["y"] = rng.uniform(0, 480, n).astype(F); kps["octave"] = rng.integers(0, 8, n); kps["angle"] = rng.uniform(0, 360, n).astype(F)
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    it = rng.choice(len(hit_x), n_hit, replace=False); k = rng.choice(n, n_hit, replace=False)
    kps["x"][k] = np.clip(hit_x[it] + rng.normal(0, 1, n_hit), 0, 639); kps["y"][k] = np.clip(hit_y[it] + rng.normal(0, 1, n_hit), 0, 479); kps["octave"][k] = hit_octave[it]
    desc[k] = hit_desc[it]
    uright = np.where(rng.uniform(0, 1, n) < 0.3, kps["x"] - rng.uniform(2, 30, n), -1).astype(F)
    init = np.full(n, -1, np.int32); init[rng.uniform(0, 1, n) < 0.1] = -2
    return dict(kps=kps, desc=desc, uright=uright, scale=scales(), bounds=BOUNDS, init=init)


def sparse_frame_for_map(mp, seed, n):
    return sparse_frame(seed, n, mp["proj_x"], mp["proj_y"], np.maximum(mp["level"] - 1, 0), mp["desc"])


def sparse_frame_for_last(last, pose, seed, n):
    """as sparse_frame_for_map, for the last frame's map points seen with `pose`"""
    Xc = last["world_pos"].astype(np.float64) @ pose["Rcw"].astype(np.float64).T + pose["tcw"].astype(np.float64)
    return sparse_frame(seed, n, pose["fx"] * Xc[:, 0] / Xc[:, 2] + pose["cx"], pose["fy"] * Xc[:, 1] / Xc[:, 2] + pose["cy"], last["keys"]["octave"], last["mp_desc"])


def remap_for_map(frame, mp):
    """a frame of one scene against the map points of another: same key points, its pre-set indices folded into the other map's range"""
    out = dict(frame); out["mp"] = mp
    init = frame["init"].copy(); init[init >= 0] %= len(mp["desc"])
    out["init"] = init
    return out


def chain_map(seed, m, n=48):
    """one cluster, every map point with the same projection, level and radius class (the same window and candidates), none with observations: nothing is ever
    blocked, so in the round schemes item k waits for all of 0 .. k-1 and the unfinished list shrinks by one per round"""
    rng = np.random.default_rng(seed)
    kps = np.zeros(n, KP_DTYPE)
    kps["x"] = (300 + rng.uniform(-9, 9, n)).astype(F); kps["y"] = (200 + rng.uniform(-9, 9, n)).astype(F); kps["octave"] = rng.integers(1, 3, n); kps["angle"] = rng.uniform(0, 360, n).astype(F)
    base = rng.integers(0, 256, (2, 32), dtype=np.uint8)
    desc, _ = alphabet_desc(rng, base, n)
    mdesc, _ = alphabet_desc(rng, base, m)
    mp = dict(proj_x=np.full(m, 300, F), proj_y=np.full(m, 200, F), proj_xr=np.full(m, 280, F), level=np.full(m, 2, np.int32), view_cos=np.full(m, 0.95, F),
              in_view=np.ones(m, np.uint8), desc=mdesc, obs_positive=np.zeros(m, np.uint8))
    init = np.full(n, -1, np.int32); init[::9] = -2
    return dict(kps=kps, desc=desc, uright=None, scale=scales(), bounds=BOUNDS, mp=mp, init=init)


# ---------------------------------------------------------------- last frame
MOTIONS = dict(forward=-0.15, backward=0.15, neither=0.02)      # tcw.z: tlc.z = -tcw.z (nearly) against b = bf / fx = 0.076


def lf_pose(motion, ang=0.01):
    Rcw = np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]], F)
    return dict(Rcw=Rcw, tcw=np.array([0.01, -0.005, MOTIONS[motion]], F), Rlw=np.eye(3, dtype=F), tlw=np.zeros(3, F), fx=FX, fy=FY, cx=CX, cy=CY, bf=BF, b=BF / FX)


def _back_project(pose, u, v, z):
    """world points that the pose projects to (u, v) at depth z"""
    Xc = np.stack([(u - pose["cx"]) / pose["fx"] * z, (v - pose["cy"]) / pose["fy"] * z, z], 1)
    return ((Xc - pose["tcw"].astype(np.float64)) @ pose["Rcw"].astype(np.float64)).astype(F)


def crowded_last(seed, n, m, a, obs_share=0.5, motion="forward", **kw):
    """current frame with n clustered key points; last frame of m key points whose map points were back-projected from the clusters with the scene's pose.
    Returns dict(kps, desc, uright, scale, bounds, last, pose, init); other poses for the same last frame: lf_pose()."""
    rng = np.random.default_rng(seed)
    pose = lf_pose(motion)
    kps, _ = clustered_keypoints(rng, n, **kw)
    base = rng.integers(0, 256, (a, 32), dtype=np.uint8)
    desc, code = alphabet_desc(rng, base, n)
    kz = rng.uniform(0.8, 4.0, n)
    uright = np.where(rng.uniform(0, 1, n) < 0.5, kps["x"] - BF / kz, -1).astype(F)
    src = rng.integers(0, n, m)
    u = kps["x"][src] + rng.uniform(-5, 5, m); v = kps["y"][src] + rng.uniform(-5, 5, m)
    xw = _back_project(pose, u, v, kz[src] * (1 + rng.uniform(-0.02, 0.02, m)))
    lk = np.zeros(m, KP_DTYPE)
    lk["octave"] = np.clip(kps["octave"][src] + rng.integers(-1, 2, m), 0, 7)
    # most pairs turn by 18-30 degrees (bins 2-3 of the rotation histogram); the rest by anything: their assignments are what the cull drops
    turn = np.where(rng.uniform(0, 1, m) < 0.7, rng.uniform(18, 30, m), rng.uniform(0, 360, m))
    lk["angle"] = np.mod(kps["angle"][src] + turn, 360).astype(F)
    same = rng.uniform(0, 1, m) < 0.6
    mdesc, _ = alphabet_desc(rng, base, m, np.where(same, code[src], rng.integers(0, a, m)))
    obs = (rng.uniform(0, 1, m) < obs_share).astype(np.uint8) if 0.0 < obs_share < 1.0 else np.full(m, int(obs_share), np.uint8)
    last = dict(keys=lk, has_mappoint=(rng.uniform(0, 1, m) < 0.9).astype(np.uint8), outlier=(rng.uniform(0, 1, m) < 0.05).astype(np.uint8), world_pos=xw,
                mp_desc=mdesc, obs_positive=obs)
    return dict(kps=kps, desc=desc, uright=uright, scale=scales(), bounds=BOUNDS, last=last, pose=pose,
                init=match_init(rng, n, np.nonzero(obs)[0], np.nonzero(obs == 0)[0]))


def chain_last(seed, n_last, inactive=0, n=48, motion="neither"):
    """every last-frame point is the SAME world point on the same octave (one window, one candidate set), none has observations; `inactive` of them hold no map point"""
    rng = np.random.default_rng(seed)
    pose = lf_pose(motion)
    kps = np.zeros(n, KP_DTYPE)
    kps["x"] = (300 + rng.uniform(-9, 9, n)).astype(F); kps["y"] = (200 + rng.uniform(-9, 9, n)).astype(F); kps["octave"] = rng.integers(1, 4, n); kps["angle"] = rng.uniform(0, 360, n).astype(F)
    base = rng.integers(0, 256, (2, 32), dtype=np.uint8)
    desc, _ = alphabet_desc(rng, base, n)
    mdesc, _ = alphabet_desc(rng, base, n_last)
    lk = np.zeros(n_last, KP_DTYPE); lk["octave"] = 2; lk["angle"] = rng.uniform(0, 360, n_last).astype(F)
    xw = np.repeat(_back_project(pose, np.array([300.0]), np.array([200.0]), np.array([2.0])), n_last, 0)
    has = np.ones(n_last, np.uint8); has[rng.choice(n_last, inactive, replace=False)] = 0
    last = dict(keys=lk, has_mappoint=has, outlier=np.zeros(n_last, np.uint8), world_pos=xw, mp_desc=mdesc, obs_positive=np.zeros(n_last, np.uint8))
    init = np.full(n, -1, np.int32); init[::9] = -2
    return dict(kps=kps, desc=desc, uright=None, scale=scales(), bounds=BOUNDS, last=last, pose=pose, init=init)


# ---------------------------------------------------------------- keyframe / Sim3
def crowded_keyframe(seed, nk, m, a, sim3_scale=1.04, chain=False):
    """clustered variant of kfgen.keyframe_scene: nk key points, m map points that re-observe them (chain: one cluster and ONE world point for every item).
    Returns dict(kps, uright, desc, scale, bounds, pose, pts, Scw, intr, init) for the Sim3 search, and kf / reloc for the relocalisation search, whose
    items are the features of another keyframe holding the same map points."""
    r = np.random.default_rng(seed)
    fx, fy, cx, cy, bf = F(517.3), F(516.5), F(318.6), F(255.3), F(40.0)
    sc = scales()
    if chain:
        kps = np.zeros(nk, KP_DTYPE)
        kps["x"] = (300 + r.uniform(-10, 10, nk)).astype(F); kps["y"] = (200 + r.uniform(-10, 10, nk)).astype(F); kps["octave"] = r.integers(2, 4, nk)
        kps["angle"] = r.uniform(0, 360, nk).astype(F)
    else:
        kps, _ = clustered_keypoints(r, nk)
    base = r.integers(0, 256, (a, 32), dtype=np.uint8)
    desc, code = alphabet_desc(r, base, nk)
    kz = r.uniform(0.6, 7.6, nk).astype(F)
    ur = np.where(r.random(nk) < 0.7, kps["x"] - bf / kz, F(-1)).astype(F)
    R = _rot(r.uniform(-0.08, 0.08), r.uniform(-0.05, 0.05)); t = r.uniform(-0.3, 0.3, 3).astype(F)
    Ow = (-(R.T.astype(np.float64) @ t.astype(np.float64))).astype(F)
    if chain:
        src = np.zeros(m, np.int64)
        u0 = np.full(m, 300.0); v0 = np.full(m, 200.0); z = np.full(m, 3.0); plev = np.full(m, 3)
        half = np.zeros(m); wob = np.zeros(m)
    else:
        src = r.integers(0, nk, m)
        u0 = kps["x"][src] + r.uniform(-3, 3, m) * sc[kps["octave"][src]]; v0 = kps["y"][src] + r.uniform(-3, 3, m) * sc[kps["octave"][src]]
        z = kz[src] * (1 + r.uniform(-0.01, 0.01, m)); plev = kps["octave"][src]
        half = (r.random(m) < 0.5).astype(np.float64); wob = r.uniform(-0.45, 0.45, m)
    Xc = np.stack([(u0 - cx) / fx * z, (v0 - cy) / fy * z, z], 1)
    xw = ((Xc - t) @ R.astype(np.float64)).astype(F)
    PO = xw - Ow; dist = np.linalg.norm(PO, axis=1)
    nrm = PO / dist[:, None] + (0 if chain else r.uniform(-0.3, 0.3, (m, 3)))
    nrm = (nrm / np.linalg.norm(nrm, axis=1)[:, None]).astype(F)
    dmax = (dist * 1.2 ** (plev + half - 0.5 + wob)).astype(F)
    dmin = (dmax / F(1.2 ** 7)).astype(F)
    same = r.random(m) < (1.0 if chain else 0.6)
    mdesc, _ = alphabet_desc(r, base, m, np.where(same, code[src], r.integers(0, a, m)))
    valid = np.ones(m, np.uint8) if chain else (r.random(m) > 0.08).astype(np.uint8)
    is2 = (1.0 / (sc.astype(np.float64) ** 2)).astype(F)
    lsf = float(F(np.log(F(1.2))))
    pose = dict(Rcw=R, tcw=t, Ow=Ow, fx=float(fx), fy=float(fy), cx=float(cx), cy=float(cy), bf=float(bf), log_scale_factor=lsf, inv_sigma2=is2)
    S = np.eye(4, dtype=F); S[:3, :3] = F(sim3_scale) * R; S[:3, 3] = F(sim3_scale) * t
    # occupied entries only (-2, and indices set before the call): these two overloads test the pointer alone
    init = np.full(nk, -1, np.int32); uu = r.random(nk); init[uu < 0.15] = -2; s = (uu >= 0.15) & (uu < 0.25); init[s] = r.integers(0, m, int(s.sum()))
    ik = np.zeros(m, KP_DTYPE); ik["angle"] = np.mod(kps["angle"][src] + np.where(r.random(m) < 0.7, r.uniform(18, 30, m), r.uniform(0, 360, m)), 360).astype(F)
    return dict(kps=kps, uright=ur, desc=desc, scale=sc, pose=pose, bounds=BOUNDS, Scw=S, init=init,
                intr={k: pose[k] for k in ("fx", "fy", "cx", "cy", "bf", "log_scale_factor")},
                pts=dict(xw=xw, normal=nrm, min_dist=dmin, max_dist=dmax, desc=mdesc, valid=valid),
                kf=dict(keys=ik, valid=valid, world_pos=xw, min_dist=dmin, max_dist=dmax, mp_desc=mdesc),
                reloc=dict(pose=dict(Rcw=R, tcw=t, fx=float(fx), fy=float(fy), cx=float(cx), cy=float(cy)), logsf=lsf, th=8.0 if chain else 6.0, orbdist=100))


# ---------------------------------------------------------------- the scenes of the two test files, by name
def map_scenes():
    """name -> crowded map scene; the four sizes, the three observation shares"""
    (n0, m0, a0), (n1, m1, a1), (n2, m2, a2), (n3, m3, a3) = CROWD_SIZES
    return {"n96_obs1": crowded_map(11, n0, m0, a0, 1.0), "n300_obs05": crowded_map(12, n1, m1, a1, 0.5), "n40_obs0": crowded_map(13, n2, m2, a2, 0.0),
            "n500_obs05": crowded_map(14, n3, m3, a3, 0.5)}


def map_chains():
    return {"chain%d" % m: chain_map(20 + m, m) for m in CHAIN_ITEMS}


def last_scenes():
    (n0, m0, a0), (n1, m1, a1), (n2, m2, a2), (n3, m3, a3) = CROWD_SIZES
    return {"n96_forward": crowded_last(31, n0, m0, a0, 0.5, "forward"), "n300_backward": crowded_last(32, n1, m1, a1, 0.5, "backward"),
            "n40_neither": crowded_last(33, n2, m2, a2, 0.0, "neither"), "n500_forward_obs1": crowded_last(34, n3, m3, a3, 1.0, "forward")}


def last_chains():
    """odd Lf.n (the kernels round their LDS lists to an even length) and 256 active points out of 257"""
    return {"chain255": chain_last(41, 255), "chain257": chain_last(42, 257), "chain256of257": chain_last(43, 257, inactive=1), "chain513": chain_last(44, 513)}


def keyframe_scenes():
    (n0, m0, a0), (n1, m1, a1), (n2, m2, a2), (n3, m3, a3) = CROWD_SIZES
    return {"n96": crowded_keyframe(51, n0, m0, a0), "n300": crowded_keyframe(52, n1, m1, a1, 0.97), "n40": crowded_keyframe(53, n2, m2, a2), "n500": crowded_keyframe(54, n3, m3, a3)}


def keyframe_chains():
    return {"chain257": crowded_keyframe(61, 400, 257, 1, chain=True)}


# ---------------------------------------------------------------- calls in which one frame overflows its candidate pool and the others do not
FRAME_KEYS = ("kps", "desc", "uright", "scale", "bounds", "init")


def mixed_map_call():
    """one crowded frame between two sparse ones against the crowded frame's map.  The pool of a frame holds cand_avg * max_mappoints entries
    (plf_matcher_create); a frame whose cell-window counts add up to more is handed to the fallback kernel."""
    s = crowded_map(12, *CROWD_SIZES[1], 0.5)
    frames = [sparse_frame_for_map(s["mp"], 71, 300), {k: s[k] for k in FRAME_KEYS}, sparse_frame_for_map(s["mp"], 72, 280)]
    return dict(frames=frames, mp=s["mp"], th=3.0, nnratio=0.8, cand_avg=8, max_mappoints=len(s["mp"]["desc"]), overflowing=[1])


def mixed_last_call():
    s = crowded_last(32, *CROWD_SIZES[1], 0.5, "backward")
    poses = [lf_pose("forward"), s["pose"], lf_pose("neither")]
    frames = [sparse_frame_for_last(s["last"], poses[0], 81, 300), {k: s[k] for k in FRAME_KEYS}, sparse_frame_for_last(s["last"], poses[2], 82, 280)]
    n_last = len(s["last"]["mp_desc"])
    return dict(frames=frames, last=s["last"], poses=poses, th=15.0, mono=0, cand_avg=8, max_mappoints=n_last, max_keypoints=n_last, overflowing=[1])

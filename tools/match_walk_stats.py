#!/usr/bin/env python3
"""Window key points per map point on the bench's scenes: ub (what one lane of k_mp_candidates / k_lf_candidates walks) and its per-frame sum, which is
what the kernels add up in total[f] (the fill of the candidate pool).  Recomputed on the host from the key points the bench's own step extracted, with the
kernels' formulas (k_build_grid's cell of a key point, cell_window's window); the share of a wave's lane-iterations that do work in a loop of every lane
over its own window is sum(ub) / (64 * max(ub)) per wave of 64 consecutive items.

    python tools/match_walk_stats.py [frames=256] [family=polygons]"""
import os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch
import bench
from rgbd_pl_slam_amd._lib import KP_DTYPE

B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
family = sys.argv[2] if len(sys.argv) > 2 else "polygons"
W, H, NFEAT, NLINES = bench.CONFIGS[2][:4]
COLS, ROWS = 64, 48
F = np.float32


def window_counts(kps, x, y, rad, act):
    """ub of every item: key points in the cell window of (x, y, rad), float32 as on the device"""
    inv_w, inv_h = F(COLS) / F(W), F(ROWS) / F(H)
    px = np.floor((kps["x"] * inv_w).astype(F) + F(0.5)).astype(int); py = np.floor((kps["y"] * inv_h).astype(F) + F(0.5)).astype(int)   # roundf, coordinates >= 0
    ok = (px >= 0) & (px < COLS) & (py >= 0) & (py < ROWS)
    cnt = np.zeros((COLS, ROWS), np.int64); np.add.at(cnt, (px[ok], py[ok]), 1)
    S = np.zeros((COLS + 1, ROWS + 1), np.int64); S[1:, 1:] = cnt.cumsum(0).cumsum(1)
    x0 = np.maximum(0, np.floor((x - rad) * inv_w).astype(int)); x1 = np.minimum(COLS - 1, np.ceil((x + rad) * inv_w).astype(int))
    y0 = np.maximum(0, np.floor((y - rad) * inv_h).astype(int)); y1 = np.minimum(ROWS - 1, np.ceil((y + rad) * inv_h).astype(int))
    good = act & (x0 < COLS) & (x1 >= 0) & (y0 < ROWS) & (y1 >= 0)
    x0, x1, y0, y1 = (np.clip(v, 0, m) for v, m in ((x0, COLS - 1), (x1, COLS - 1), (y0, ROWS - 1), (y1, ROWS - 1)))
    ub = S[x1 + 1, y1 + 1] - S[x0, y1 + 1] - S[x1 + 1, y0] + S[x0, y0]
    return np.where(good, ub, 0), np.where(good, x1 - x0 + 1, 0)


def report(name, ubs, cols):
    ubs = np.array(ubs); tot = ubs.sum(1)
    waves = np.pad(ubs, ((0, 0), (0, -ubs.shape[1] % 64))).reshape(ubs.shape[0], -1, 64)
    longest = waves.max(2)
    print("%s: %d frames x %d items; total[f] mean %.0f min %d max %d; ub per item mean %.2f; window columns mean %.1f max %d" %
          (name, ubs.shape[0], ubs.shape[1], tot.mean(), tot.min(), tot.max(), ubs.mean(), np.array(cols)[np.array(cols) > 0].mean(), np.max(cols)))
    for f in (0, ubs.shape[0] // 2):
        print("    frame %d: ub mean %.2f max %d, total %d" % (f, ubs[f].mean(), ubs[f].max(), tot[f]))
    print("    per wave of 64 items: sum(ub) mean %.1f, longest lane mean %.1f -> busy lane-iterations of a per-lane loop %.3f; chunks of 64 in a flat walk mean %.2f" %
          (waves.sum(2).mean(), longest.mean(), waves.sum() / (64.0 * longest.sum()), np.ceil(waves.sum(2) / 64.0).mean()))


p = bench.Pipeline(W, H, NFEAT, NLINES, B, 0, 0, distinct=B, family=family)
p.step(); p.flush(); torch.cuda.synchronize()
bs = p.bufs[0]
nk = bs["nk"].cpu().numpy(); kall = bs["kps"].cpu().numpy()
mp = {k: v.cpu().numpy() for k, v in p.mp.items()}
last = {k: v.cpu().numpy() for k, v in p.last.items()}
scale = p.scale.cpu().numpy()
rad_mp = (np.where(mp["view_cos"].astype(np.float64) > 0.998, F(2.5), F(4.0)) * F(3.0)).astype(F) * scale[mp["level"]]
lkeys = np.frombuffer(last["keys"].tobytes(), KP_DTYPE)
pose = p.poses[0][0]
Rcw = np.array(pose.Rcw[:], F).reshape(3, 3); tcw = np.array(pose.tcw[:], F)
Xc = last["world_pos"].astype(F) @ Rcw.T + tcw
u = (F(pose.fx) * Xc[:, 0] / Xc[:, 2] + F(pose.cx)).astype(F); v = (F(pose.fy) * Xc[:, 1] / Xc[:, 2] + F(pose.cy)).astype(F)
act_l = (last["has_mappoint"] != 0) & (last["outlier"] == 0) & (Xc[:, 2] > 0) & (u >= 0) & (u <= W) & (v >= 0) & (v <= H)
rad_l = F(7.0) * scale[lkeys["octave"]]
ub_mp, ub_lf, c_mp, c_lf = [], [], [], []
for f in range(B):
    k = np.frombuffer(kall[f, :nk[f]].tobytes(), KP_DTYPE)
    a, c = window_counts(k, mp["proj_x"], mp["proj_y"], rad_mp, mp["in_view"] != 0); ub_mp.append(a); c_mp.append(c)
    a, c = window_counts(k, u, v, rad_l, act_l); ub_lf.append(a); c_lf.append(c)
print("family %s, key points per frame mean %.0f" % (family, nk.mean()))
report("k_mp_candidates (th 3)", ub_mp, c_mp)
report("k_lf_candidates (th 7, pose of frame 0)", ub_lf, c_lf)
p.close()

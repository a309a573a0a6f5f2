"""Inputs of tests/test_gpu_octree.py and their CPU side: small images that put k_octree (rgbd_pl_slam_amd/csrc/orb_octree.hip) into each of its
situations, the FAST candidates of their levels from the oracle, and the trace of the octree on them (tests/models/octree_schedule.py)."""
import ctypes as C

import numpy as np

import orc
from models.octree_schedule import distribute_octree as octree_schedule

W, H, NLEVELS = 192, 144, 3      # levels 192x144, 160x120, 133x100: 5x3, 4x2 and 3x2 FAST cells
EDGE = 19


def flat():
    return np.full((H, W), 128, np.uint8)


def noise(seed, lo=0, hi=256, w=W, h=H):
    return np.random.default_rng(seed).integers(lo, hi, (h, w)).astype(np.uint8)


def two_level_noise(seed, w=W, h=H):
    """dense two-valued noise: every corner of the left half has the same response (ties in the best-key pass); the right half's contrast of 12 lies under
    iniThFAST = 20, so its cells are found by the retry with minThFAST = 7"""
    bits = np.random.default_rng(seed).integers(0, 2, (h, w)).astype(np.uint8)
    img = 100 + bits * 40
    img[:, w // 2:] = 100 + bits[:, w // 2:] * 12
    return img.astype(np.uint8)


def cluster(seed):
    """all candidates inside one 28 x 28 patch"""
    img = np.full((H, W), 128, np.uint8)
    img[60:88, 70:98] = noise(seed, 0, 256, 28, 28)
    return img


def polygons(seed, w=W, h=H):
    from rgbd_pl_slam_amd.synth import synth_frame
    return synth_frame(seed, w, h)


def level_candidates(img, nfeatures, nlevels=NLEVELS, scale_factor=1.2, ini_th=20, min_th=7):
    """per level: (candidates [n, 3] = x, y, response relative to the border, as ORBextractor.candidates gives them; W, H of the octree; quota N)"""
    ref = orc.orb_extract(img, nfeatures=nfeatures, nlevels=nlevels, scale_factor=scale_factor, ini_th=ini_th, min_th=min_th, debug=True)
    per = orc.orb_tables(nfeatures, scale_factor, nlevels)["perLevel"]
    out = []
    for l in range(nlevels):
        plane = np.ascontiguousarray(ref["pyr"][l])
        lw, lh, pp = ref["lw"][l], ref["lh"][l], plane.shape[1]
        buf = np.zeros(lw * lh + 16, orc.KP_DTYPE)
        nc = C.c_int(0)
        base = plane.ctypes.data + EDGE * pp + EDGE
        n = orc.lib().orc_fast_cells(C.c_void_p(base), C.c_int(lw), C.c_int(lh), C.c_ssize_t(pp), C.c_int(ini_th), C.c_int(min_th), orc.p(buf),
                                     C.c_int(len(buf)), C.byref(nc))
        assert n == ref["ncand"][l]
        k = np.stack([buf["x"][:n], buf["y"][:n], buf["response"][:n]], 1).astype(np.float32)
        out.append((k, lw - 32, lh - 32, int(per[l])))
    return out, ref

"""LoopClosing::CorrectLoop's Sim3 pose propagation and map-point moves, and the pose / point tails of Optimizer::OptimizeEssentialGraph and
LoopClosing::RunGlobalBundleAdjustment, on the GPU: thin mirrors of the plf_loop_* / plf_gba_* calls (include/plf.h, "Loop correction"); the compute
is HIP (csrc/loopfix_kernels.hip, csrc/mapgeom_kernels.hip).  Every array is a torch device tensor, updated in place where the C call says so; nothing
is read back by any call.  A Sim3 is 8 float64: qx qy qz qw tx ty tz s.  kf_tcw is (n_kf, 12) float32 (rows of [Rcw | tcw]), kf_ow (n_kf, 3)."""
import ctypes as C
from dataclasses import dataclass

from . import _lib as L
from .localmap import _on, _stream
from .pose import _sized
from .mappoints import _arg, update_normal_and_depth


def _lib():
    return L.loopfix_prototypes(L.lib())


def _dev(t):
    return t.device.index or 0


def loop_scw(scm, kf_tcw, matched_slot, out=None, stream=None):
    """mg2oScw = gScm * Sim3(Rmw, tmw, 1.0): scm (8,) float64, a sim3 row of sim3_optimize; matched_slot: the matched keyframe.  Returns (8,) float64."""
    import torch
    n_kf = int(kf_tcw.shape[0])
    if out is None:
        with _on(stream, kf_tcw.device):
            out = torch.zeros(8, dtype=torch.float64, device=kf_tcw.device)
    L.check(_lib().plf_loop_scw(_sized(scm, "scm", torch.float64, 8), _sized(kf_tcw, "kf_tcw", torch.float32, n_kf * 12), n_kf, int(matched_slot),
                                _sized(out, "out", torch.float64, 8), _dev(kf_tcw), _stream(stream)), "plf_loop_scw")
    return out


def loop_sim3_pairs(kf_tcw, kf_ow, rank_kf, cur_slot=0, scw=None, stream=None):
    """CorrectedSim3 / NonCorrectedSim3 for the K slots rank_kf (int32, the caller's std::map order).  scw None: only Sim3(Rcw, tcw, 1.0) per slot.
    Returns (corrected or None, noncorrected), (K, 8) float64."""
    import torch
    n_kf, K = int(kf_tcw.shape[0]), int(rank_kf.shape[0])
    with _on(stream, kf_tcw.device):
        non = torch.zeros((K, 8), dtype=torch.float64, device=kf_tcw.device)
        cor = torch.zeros((K, 8), dtype=torch.float64, device=kf_tcw.device) if scw is not None else None
    L.check(_lib().plf_loop_sim3_pairs(_sized(kf_tcw, "kf_tcw", torch.float32, n_kf * 12), _sized(kf_ow, "kf_ow", torch.float32, n_kf * 3) if kf_ow is not None else None,
                                       n_kf, _arg(rank_kf, "rank_kf", torch.int32, K), K, int(cur_slot),
                                       _sized(scw, "scw", torch.float64, 8) if scw is not None else None, _arg(cor, "corrected", torch.float64),
                                       _arg(non, "noncorrected", torch.float64), _dev(kf_tcw), _stream(stream)), "plf_loop_sim3_pairs")
    return cor, non


def loop_correct_points(rank_kf, row_start, row_point, point_bad, kf_id, corrected, noncorrected, cur_kf_id, world_pos, corrected_by, corrected_ref,
                        owner_rank=None, stream=None):
    """the point half of CorrectLoop's second loop: world_pos (n_points, 3) float32, corrected_by / corrected_ref (n_points,) int64 IN PLACE; returns
    owner_rank (n_points,) int32: the rank that moved the point, -1: left alone."""
    import torch
    K, n_points, n_kf = int(rank_kf.shape[0]), int(point_bad.shape[0]), int(kf_id.shape[0])
    v = L.LoopView(K, _arg(rank_kf, "rank_kf", torch.int32, K), _arg(row_start, "row_start", torch.int32, K + 1), _arg(row_point, "row_point", torch.int32),
                   n_points, _arg(point_bad, "point_bad", torch.uint8, n_points), n_kf, _arg(kf_id, "kf_id", torch.int64, n_kf))
    if owner_rank is None:
        with _on(stream, world_pos.device):
            owner_rank = torch.empty(n_points, dtype=torch.int32, device=world_pos.device)
    L.check(_lib().plf_loop_correct_points(C.byref(v), _sized(corrected, "corrected", torch.float64, K * 8), _sized(noncorrected, "noncorrected", torch.float64, K * 8),
                                           int(cur_kf_id), _sized(world_pos, "world_pos", torch.float32, n_points * 3),
                                           _arg(corrected_by, "corrected_by", torch.int64, n_points), _arg(corrected_ref, "corrected_ref", torch.int64, n_points),
                                           _arg(owner_rank, "owner_rank", torch.int32, n_points), _dev(world_pos), _stream(stream)), "plf_loop_correct_points")
    return owner_rank


def loop_new_poses(corrected, stream=None):
    """toCvSE3(R, t * (1. / s)) per row of corrected (K, 8) and the centre SetPose derives: returns (tcw_new (K, 12), ow_new (K, 3)) float32."""
    import torch
    K = int(corrected.shape[0])
    with _on(stream, corrected.device):
        tcw = torch.zeros((K, 12), dtype=torch.float32, device=corrected.device)
        ow = torch.zeros((K, 3), dtype=torch.float32, device=corrected.device)
    L.check(_lib().plf_loop_new_poses(_sized(corrected, "corrected", torch.float64, K * 8), K, _arg(tcw, "tcw_new", torch.float32), _arg(ow, "ow_new", torch.float32),
                                      _dev(corrected), _stream(stream)), "plf_loop_new_poses")
    return tcw, ow


def loop_commit_poses(rank_kf, tcw_new, ow_new, kf_tcw, kf_ow, stream=None):
    """kf_tcw[rank_kf[r]] = tcw_new[r], kf_ow[rank_kf[r]] = ow_new[r], in place."""
    import torch
    K, n_kf = int(rank_kf.shape[0]), int(kf_tcw.shape[0])
    L.check(_lib().plf_loop_commit_poses(_arg(rank_kf, "rank_kf", torch.int32, K), K, _sized(tcw_new, "tcw_new", torch.float32, K * 12),
                                         _sized(ow_new, "ow_new", torch.float32, K * 3), _sized(kf_tcw, "kf_tcw", torch.float32, n_kf * 12),
                                         _sized(kf_ow, "kf_ow", torch.float32, n_kf * 3), n_kf, _dev(kf_tcw), _stream(stream)), "plf_loop_commit_poses")


def kf_rank_of(rank_kf, n_kf):
    """(n_kf,) int32: the rank of each slot, -1 outside the list (slots out of range dropped); torch ops on rank_kf's device"""
    import torch
    out = torch.full((n_kf,), -1, dtype=torch.int32, device=rank_kf.device)
    ok = (rank_kf >= 0) & (rank_kf < n_kf)
    out[rank_kf[ok].long()] = torch.arange(int(rank_kf.shape[0]), dtype=torch.int32, device=rank_kf.device)[ok]
    return out


def loop_normal_depth(owner_rank, kf_rank, ow_new, world_pos, normal, min_distance, max_distance, geom, stream=None):
    """UpdateNormalAndDepth as the walk interleaves it, over the points with owner_rank >= 0: keyframe k's centre is ow_new[kf_rank[k]] when
    0 <= kf_rank[k] < owner_rank[p], kf_ow[k] otherwise.  geom: the keyword arguments of update_normal_and_depth that describe the map (obs_start,
    obs_kf, kf_ow, ref_kf, ref_level or obs_idx + kf_keys, scale_factors, point_bad, ...).  Returns n_obs_used."""
    if int(owner_rank.shape[0]) == 0:
        return owner_rank.new_empty(0)
    return update_normal_and_depth(world_pos=world_pos, normal=normal, min_distance=min_distance, max_distance=max_distance, stream=stream,
                                   device=_dev(world_pos), staged=(kf_rank, ow_new, owner_rank), **geom)


@dataclass
class LoopResult:
    corrected: object = None
    noncorrected: object = None
    owner_rank: object = None
    tcw_new: object = None
    ow_new: object = None
    n_obs_used: object = None


def loop_correct(kf_tcw, kf_ow, kf_id, rank_kf, cur_slot, cur_kf_id, scw, row_start, row_point, point_bad, world_pos, corrected_by, corrected_ref, normal,
                 min_distance, max_distance, geom, stream=None):
    """CorrectLoop's two loops, chained on one stream with nothing read back: the Sim3 pairs, the point moves, the new poses, the interleaved
    UpdateNormalAndDepth, then the poses committed.  kf_tcw, kf_ow, world_pos, the two marks, normal and the distances are updated IN PLACE.  geom as
    for loop_normal_depth (its kf_ow must be the kf_ow given here).  Returns a LoopResult; corrected[r] is the Scw plf_match_fuse_sim3 takes next."""
    n_kf = int(kf_tcw.shape[0])
    with _on(stream, kf_tcw.device):
        kf_rank = kf_rank_of(rank_kf, n_kf)
    cor, non = loop_sim3_pairs(kf_tcw, kf_ow, rank_kf, cur_slot, scw, stream)
    owner = loop_correct_points(rank_kf, row_start, row_point, point_bad, kf_id, cor, non, cur_kf_id, world_pos, corrected_by, corrected_ref, stream=stream)
    tcw_new, ow_new = loop_new_poses(cor, stream)
    used = loop_normal_depth(owner, kf_rank, ow_new, world_pos, normal, min_distance, max_distance, geom, stream)
    loop_commit_poses(rank_kf, tcw_new, ow_new, kf_tcw, kf_ow, stream)
    return LoopResult(cor, non, owner, tcw_new, ow_new, used)


def loop_correct_points_by_ref(point_bad, ref_kf, corrected_by, corrected_ref, cur_kf_id, id_to_slot, scw, swc, world_pos, moved=None, stream=None):
    """the essential-graph tail's point loop: per point that is not bad the pair (scw, swc)[slot], slot = id_to_slot[corrected_ref] where corrected_by ==
    cur_kf_id, ref_kf otherwise; world_pos IN PLACE.  scw, swc (n_kf, 8) float64: vScw, vCorrectedSwc by slot.  Returns moved (n_points,) uint8."""
    import torch
    n_points, n_kf, n_ids = int(point_bad.shape[0]), int(scw.shape[0]), int(id_to_slot.shape[0])
    if moved is None:
        with _on(stream, world_pos.device):
            moved = torch.empty(n_points, dtype=torch.uint8, device=world_pos.device)
    L.check(_lib().plf_loop_correct_points_by_ref(n_points, _arg(point_bad, "point_bad", torch.uint8, n_points), _arg(ref_kf, "ref_kf", torch.int32, n_points),
                                                  _arg(corrected_by, "corrected_by", torch.int64, n_points), _arg(corrected_ref, "corrected_ref", torch.int64, n_points),
                                                  int(cur_kf_id), _arg(id_to_slot, "id_to_slot", torch.int32) if n_ids else None, n_ids,
                                                  _sized(scw, "scw", torch.float64, n_kf * 8), _sized(swc, "swc", torch.float64, n_kf * 8), n_kf,
                                                  _sized(world_pos, "world_pos", torch.float32, n_points * 3), _arg(moved, "moved", torch.uint8, n_points),
                                                  _dev(world_pos), _stream(stream)), "plf_loop_correct_points_by_ref")
    return moved


def essential_graph_correct(corrected_siw, scw, swc, kf_tcw, kf_ow, point_bad, ref_kf, corrected_by, corrected_ref, cur_kf_id, id_to_slot, world_pos, normal,
                            min_distance, max_distance, geom, stream=None):
    """the tail of OptimizeEssentialGraph: SetPose(toCvSE3(R, t * (1. / s))) of corrected_siw (n_kf, 8) for every keyframe, the point loop with vScw = scw
    and vCorrectedSwc = swc, then UpdateNormalAndDepth with the final centres.  Everything in place; returns (moved, n_obs_used)."""
    import torch
    n_kf = int(kf_tcw.shape[0])
    with _on(stream, kf_tcw.device):
        every = torch.arange(n_kf, dtype=torch.int32, device=kf_tcw.device)
    tcw_new, ow_new = loop_new_poses(corrected_siw, stream)
    loop_commit_poses(every, tcw_new, ow_new, kf_tcw, kf_ow, stream)
    moved = loop_correct_points_by_ref(point_bad, ref_kf, corrected_by, corrected_ref, cur_kf_id, id_to_slot, scw, swc, world_pos, stream=stream)
    used = update_normal_and_depth(world_pos=world_pos, normal=normal, min_distance=min_distance, max_distance=max_distance, stream=stream,
                                   device=_dev(world_pos), **geom)
    return moved, used


def gba_propagate_poses(parent, origins, kf_flag, tcw_gba, kf_tcw, kf_ow, tcw_bef=None, stream=None):
    """the keyframe loop of RunGlobalBundleAdjustment's tail: kf_flag (uint8), tcw_gba, kf_tcw, kf_ow IN PLACE; returns tcw_bef (n_kf, 12)."""
    import torch
    n_kf, n_or = int(kf_tcw.shape[0]), int(origins.shape[0])
    if tcw_bef is None:
        with _on(stream, kf_tcw.device):
            tcw_bef = torch.zeros((n_kf, 12), dtype=torch.float32, device=kf_tcw.device)
    v = L.GbaView(n_kf, _arg(parent, "parent", torch.int32, n_kf), _arg(origins, "origins", torch.int32) if n_or else None, n_or,
                  _arg(kf_flag, "kf_flag", torch.uint8, n_kf), _sized(tcw_gba, "tcw_gba", torch.float32, n_kf * 12),
                  _sized(kf_tcw, "kf_tcw", torch.float32, n_kf * 12), _sized(kf_ow, "kf_ow", torch.float32, n_kf * 3),
                  _sized(tcw_bef, "tcw_bef", torch.float32, n_kf * 12))
    L.check(_lib().plf_gba_propagate_poses(C.byref(v), _dev(kf_tcw), _stream(stream)), "plf_gba_propagate_poses")
    return tcw_bef


def gba_correct_points(point_bad, point_flag, pos_gba, ref_kf, kf_flag, tcw_bef, kf_tcw, kf_ow, world_pos, stream=None):
    """the map-point loop of the same tail; world_pos IN PLACE."""
    import torch
    n_points, n_kf = int(point_bad.shape[0]), int(kf_tcw.shape[0])
    L.check(_lib().plf_gba_correct_points(n_points, _arg(point_bad, "point_bad", torch.uint8, n_points), _arg(point_flag, "point_flag", torch.uint8, n_points),
                                          _sized(pos_gba, "pos_gba", torch.float32, n_points * 3), _arg(ref_kf, "ref_kf", torch.int32, n_points),
                                          _arg(kf_flag, "kf_flag", torch.uint8, n_kf), _sized(tcw_bef, "tcw_bef", torch.float32, n_kf * 12),
                                          _sized(kf_tcw, "kf_tcw", torch.float32, n_kf * 12), _sized(kf_ow, "kf_ow", torch.float32, n_kf * 3), n_kf,
                                          _sized(world_pos, "world_pos", torch.float32, n_points * 3), _dev(world_pos), _stream(stream)), "plf_gba_correct_points")
    return world_pos


def gba_correct(parent, origins, kf_flag, tcw_gba, kf_tcw, kf_ow, point_bad, point_flag, pos_gba, ref_kf, world_pos, stream=None):
    """both loops of the tail on one stream; returns tcw_bef."""
    tcw_bef = gba_propagate_poses(parent, origins, kf_flag, tcw_gba, kf_tcw, kf_ow, stream=stream)
    gba_correct_points(point_bad, point_flag, pos_gba, ref_kf, kf_flag, tcw_bef, kf_tcw, kf_ow, world_pos, stream)
    return tcw_bef

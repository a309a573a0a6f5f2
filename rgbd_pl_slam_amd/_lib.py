"""ctypes loader of libplf_hip.so (the C-ABI of include/plf.h).  There is NO CPU fallback: if the
HIP library is missing or cannot be loaded this module raises."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PLF_LIB_PATH") or os.path.join(_HERE, "libplf_hip.so")   # (PLF_LIB_PATH: A/B measurements of scratch builds)

PLF_OK, PLF_E_EMPTY, PLF_E_BADARG, PLF_E_CAPACITY, PLF_E_HIP, PLF_E_NOMEM, PLF_E_RECTS = 0, -1, -2, -3, -4, -5, -6
PLF_W_TRUNCATED, PLF_W_SLOW = 1, 2
last_warning = 0   # the last positive (warning) status a call returned through check(): PLF_W_SLOW
MEM_HOST, MEM_DEVICE = 0, 1

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"),
                     ("octave", "<i4"), ("class_id", "<i4")])
KL_DTYPE = np.dtype([("angle", "<f4"), ("class_id", "<i4"), ("octave", "<i4"), ("pt_x", "<f4"), ("pt_y", "<f4"),
                     ("response", "<f4"), ("size", "<f4"), ("startPointX", "<f4"), ("startPointY", "<f4"),
                     ("endPointX", "<f4"), ("endPointY", "<f4"), ("sPointInOctaveX", "<f4"), ("sPointInOctaveY", "<f4"),
                     ("ePointInOctaveX", "<f4"), ("ePointInOctaveY", "<f4"), ("lineLength", "<f4"), ("numOfPixels", "<i4")])
DMATCH_DTYPE = np.dtype([("queryIdx", "<i4"), ("trainIdx", "<i4"), ("imgIdx", "<i4"), ("distance", "<f4")])


class OrbParams(C.Structure):
    _fields_ = [("nfeatures", C.c_int32), ("scale_factor", C.c_float), ("nlevels", C.c_int32), ("ini_th_fast", C.c_int32),
                ("min_th_fast", C.c_int32), ("device", C.c_int32), ("max_width", C.c_int32), ("max_height", C.c_int32),
                ("max_batch", C.c_int32)]


class LineParams(C.Structure):
    _fields_ = [("nlines", C.c_int32), ("seed_order", C.c_int32), ("device", C.c_int32), ("max_width", C.c_int32),
                ("max_height", C.c_int32), ("max_batch", C.c_int32), ("lbd_sobel_input", C.c_int32), ("max_ms", C.c_float)]


LBD_BLURRED, LBD_RAW = 0, 1


def line_params(nlines, seed_order, device, max_width, max_height, max_batch, lbd_sobel_input=LBD_BLURRED, max_ms=0.0):
    return LineParams(nlines, seed_order, device, max_width, max_height, max_batch, lbd_sobel_input, max_ms)


class FrameView(C.Structure):
    _fields_ = [("n", C.c_int32), ("n_device", C.c_void_p), ("keys_un", C.c_void_p), ("uright", C.c_void_p), ("desc", C.c_void_p),
                ("min_x", C.c_float), ("min_y", C.c_float), ("max_x", C.c_float), ("max_y", C.c_float),
                ("scale_factors", C.c_void_p), ("nlevels", C.c_int32)]


class MapPointView(C.Structure):
    _fields_ = [("m", C.c_int32), ("proj_x", C.c_void_p), ("proj_y", C.c_void_p), ("proj_xr", C.c_void_p),
                ("level", C.c_void_p), ("view_cos", C.c_void_p), ("in_view", C.c_void_p), ("desc", C.c_void_p),
                ("obs_positive", C.c_void_p)]


class LastFrameView(C.Structure):
    _fields_ = [("n", C.c_int32), ("has_mappoint", C.c_void_p), ("outlier", C.c_void_p), ("world_pos", C.c_void_p),
                ("keys", C.c_void_p), ("mp_desc", C.c_void_p), ("obs_positive", C.c_void_p)]


class PosePair(C.Structure):
    _fields_ = [("Rcw", C.c_float * 9), ("tcw", C.c_float * 3), ("Rlw", C.c_float * 9), ("tlw", C.c_float * 3),
                ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("bf", C.c_float), ("b", C.c_float)]


class LineFrameView(C.Structure):
    _fields_ = [("n", C.c_int32), ("n_device", C.c_void_p), ("lines_un", C.c_void_p), ("desc", C.c_void_p), ("scale_factors", C.c_void_p)]


class MapLineView(C.Structure):
    _fields_ = [("m", C.c_int32), ("x1", C.c_void_p), ("y1", C.c_void_p), ("x2", C.c_void_p), ("y2", C.c_void_p),
                ("level", C.c_void_p), ("view_cos", C.c_void_p), ("in_view", C.c_void_p), ("desc", C.c_void_p)]


class BowView(C.Structure):
    _fields_ = [("n_kf", C.c_int32), ("n_f", C.c_int32), ("kf_desc", C.c_void_p), ("f_desc", C.c_void_p), ("kf_angle", C.c_void_p),
                ("f_angle", C.c_void_p), ("kf_has_mp", C.c_void_p), ("f_has_mp", C.c_void_p), ("kf_nodes", C.c_int32), ("f_nodes", C.c_int32),
                ("kf_node_id", C.c_void_p), ("f_node_id", C.c_void_p), ("kf_node_start", C.c_void_p), ("f_node_start", C.c_void_p),
                ("kf_feat", C.c_void_p), ("f_feat", C.c_void_p)]


class Points3DView(C.Structure):
    _fields_ = [("m", C.c_int32), ("world_pos", C.c_void_p), ("normal", C.c_void_p), ("min_distance", C.c_void_p), ("max_distance", C.c_void_p),
                ("desc", C.c_void_p), ("valid", C.c_void_p)]


class KfPose(C.Structure):
    _fields_ = [("Rcw", C.c_float * 9), ("tcw", C.c_float * 3), ("Ow", C.c_float * 3), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float),
                ("cy", C.c_float), ("bf", C.c_float), ("log_scale_factor", C.c_float), ("inv_level_sigma2", C.c_void_p)]


class TriView(C.Structure):
    _fields_ = [("n1", C.c_int32), ("n2", C.c_int32), ("keys1", C.c_void_p), ("keys2", C.c_void_p), ("uright1", C.c_void_p), ("uright2", C.c_void_p),
                ("desc1", C.c_void_p), ("desc2", C.c_void_p), ("has_mp1", C.c_void_p), ("has_mp2", C.c_void_p), ("nodes1", C.c_int32), ("nodes2", C.c_int32),
                ("node_id1", C.c_void_p), ("node_id2", C.c_void_p), ("node_start1", C.c_void_p), ("node_start2", C.c_void_p), ("feat1", C.c_void_p),
                ("feat2", C.c_void_p), ("scale_factors2", C.c_void_p), ("level_sigma2_2", C.c_void_p)]


class PlfError(RuntimeError):
    def __init__(self, status, what):
        super().__init__("%s failed: %s (%d)" % (what, lib().plf_status_string(status).decode(), status))
        self.status = status


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("libplf_hip.so is not built (%s): run `python -c 'import __graft_entry__ as g; g.build()'`; "
                               "there is no CPU fallback" % LIB_PATH)
        # torch (the Python mirror's device-memory plumbing) ships its own copy of the HIP runtime: it has to be in the process BEFORE this library's
        # dependency on libamdhip64 is resolved, otherwise a later `import torch` brings a second runtime and neither sees the GPU any more
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        _lib = C.CDLL(LIB_PATH)
        _lib.plf_version.restype = C.c_char_p
        _lib.plf_status_string.restype = C.c_char_p
        _lib.plf_status_string.argtypes = [C.c_int]
    return _lib


def check(status, what):
    """errors (< 0) raise; warnings (> 0: outputs complete) are kept in `last_warning`"""
    global last_warning
    last_warning = status if status > 0 else 0
    if status < 0:
        raise PlfError(status, what)


def vp(a):
    """pointer of a numpy array, a torch tensor (device or host) or an int address"""
    if a is None:
        return None
    if isinstance(a, int):
        return C.c_void_p(a)
    if hasattr(a, "data_ptr"):
        return C.c_void_p(a.data_ptr())
    return a.ctypes.data_as(C.c_void_p)


# ---- DBoW2 vocabulary (include/plf.h, "DBoW2 vocabulary")
BOW_TF_IDF, BOW_TF, BOW_IDF, BOW_BINARY = 0, 1, 2, 3
BOW_L1_NORM, BOW_L2_NORM, BOW_CHI_SQUARE, BOW_KL, BOW_BHATTACHARYYA, BOW_DOT_PRODUCT = 0, 1, 2, 3, 4, 5
BOW_MAX_CAPACITY = 8192


class VocabDesc(C.Structure):
    _fields_ = [("k", C.c_int32), ("L", C.c_int32), ("scoring", C.c_int32), ("weighting", C.c_int32), ("n_nodes", C.c_int32),
                ("parent", C.c_void_p), ("desc", C.c_void_p), ("weight", C.c_void_p), ("is_leaf", C.c_void_p)]


class VocabInfo(C.Structure):
    _fields_ = [("k", C.c_int32), ("L", C.c_int32), ("scoring", C.c_int32), ("weighting", C.c_int32), ("n_nodes", C.c_int32),
                ("n_words", C.c_int32), ("min_leaf_depth", C.c_int32)]


def bow_prototypes(l):
    """argument types of the vocabulary entry points (pointers are 64-bit: ctypes' default int would cut them)"""
    P, I = C.c_void_p, C.c_int32
    l.plf_vocab_parse_text.argtypes = [C.c_char_p, C.POINTER(VocabDesc)]
    l.plf_vocab_desc_free.argtypes = [C.POINTER(VocabDesc)]
    l.plf_vocab_desc_free.restype = None
    l.plf_vocab_create.argtypes = [C.POINTER(VocabDesc), I, C.POINTER(P)]
    l.plf_vocab_load_text.argtypes = [C.c_char_p, I, C.POINTER(P)]
    l.plf_vocab_destroy.argtypes = [P]
    l.plf_vocab_destroy.restype = None
    l.plf_vocab_info.argtypes = [P, C.POINTER(VocabInfo)]
    l.plf_bow_transform_batch.argtypes = [P, P, P, I, I, I, I, I, P, P, P, P, P, P, P, P]
    l.plf_bow_transform.argtypes = [P, P, I, I, I, I, P, P, P, P, P, P, P, P]
    l.plf_bow_score.argtypes = [P, P, P, I, P, P, P, I, P, I, P]
    return l


# ---- keyframe database (include/plf.h, "Keyframe database")
class KfdbInfo(C.Structure):
    _fields_ = [("max_keyframes", C.c_int32), ("capacity", C.c_int32), ("n_keyframes", C.c_int32), ("n_entries", C.c_int32), ("n_best", C.c_int32)]


KFDB_STATS_DTYPE = np.dtype([("n_sharing", "<i4"), ("max_common_words", "<i4"), ("n_scored", "<i4"), ("best_acc_score", "<f4")])


def kfdb_prototypes(l):
    P, I = C.c_void_p, C.c_int32
    l.plf_vocab_device.argtypes = [P]
    l.plf_kfdb_create.argtypes = [P, I, I, C.POINTER(P)]
    l.plf_kfdb_destroy.argtypes = [P]
    l.plf_kfdb_destroy.restype = None
    l.plf_kfdb_info.argtypes = [P, C.POINTER(KfdbInfo)]
    l.plf_kfdb_set_n_best.argtypes = [P, I]
    l.plf_kfdb_add_batch.argtypes = [P, P, P, P, I, I, P, P]
    l.plf_kfdb_erase_batch.argtypes = [P, P, I]
    l.plf_kfdb_clear.argtypes = [P]
    l.plf_kfdb_vectors.argtypes = [P, C.POINTER(P), C.POINTER(P), C.POINTER(P)]
    l.plf_kfdb_detect_reloc.argtypes = [P, P, P, P, I, I, P, P, I, P, P, P, P]
    l.plf_kfdb_detect_loop.argtypes = [P, P, P, P, I, I, P, P, P, P, P, I, P, P, P, P]
    return l


# ---- map (include/plf.h, "Map")
class MapObsView(C.Structure):
    _fields_ = [("n_points", C.c_int32), ("obs_start", C.c_void_p), ("obs_desc", C.c_void_p), ("obs_kf", C.c_void_p), ("obs_idx", C.c_void_p),
                ("kf_desc", C.c_void_p), ("n_kf", C.c_int32), ("obs_valid", C.c_void_p), ("point_id", C.c_void_p)]


def map_prototypes(l):
    P, I = C.c_void_p, C.c_int32
    l.plf_map_distinctive_descriptors.argtypes = [C.POINTER(MapObsView), P, I, P, P, I, P]
    return l


# ---- map geometry (include/plf.h, "Map geometry")
class MapGeomView(C.Structure):
    _fields_ = [("n_points", C.c_int32), ("obs_start", C.c_void_p), ("obs_kf", C.c_void_p), ("obs_idx", C.c_void_p), ("kf_ow", C.c_void_p),
                ("n_kf", C.c_int32), ("ref_kf", C.c_void_p), ("ref_level", C.c_void_p), ("kf_keys", C.c_void_p), ("scale_factors", C.c_void_p),
                ("nlevels", C.c_int32), ("point_bad", C.c_void_p), ("point_id", C.c_void_p), ("pos_floats", C.c_int32)]


def mapgeom_prototypes(l):
    P, I = C.c_void_p, C.c_int32
    l.plf_map_update_normal_depth.argtypes = [C.POINTER(MapGeomView), P, P, P, P, I, P, I, P]
    return l


# ---- covisibility graph (include/plf.h, "Covisibility graph")
COVIS_CONNECTIONS, COVIS_VOTES = 0, 1


class CovisView(C.Structure):
    _fields_ = [("n_rows", C.c_int32), ("row_start", C.c_void_p), ("row_point", C.c_void_p), ("row_self", C.c_void_p), ("n_points", C.c_int32),
                ("obs_start", C.c_void_p), ("obs_kf", C.c_void_p), ("point_bad", C.c_void_p), ("n_kf", C.c_int32), ("kf_bad", C.c_void_p),
                ("kf_key", C.c_void_p)]


class CovisParams(C.Structure):
    _fields_ = [("mode", C.c_int32), ("th", C.c_int32), ("stride", C.c_int32), ("dense_max_kf", C.c_int32), ("table_slots", C.c_int32)]


def covis_prototypes(l):
    P, I = C.c_void_p, C.c_int32
    l.plf_covis_count.argtypes = [C.POINTER(CovisView), C.POINTER(CovisParams), P, P, P, P, P, P, P, P, I, P]
    l.plf_covis_by_weight.argtypes = [P, P, I, I, I, P, I, P]
    return l


# ---- culling (include/plf.h, "Culling")
CULL_SNAPSHOT, CULL_SEQUENTIAL = 0, 1


class CullView(C.Structure):
    _fields_ = [("n_rows", C.c_int32), ("row_start", C.c_void_p), ("row_point", C.c_void_p), ("row_kf", C.c_void_p), ("n_points", C.c_int32),
                ("obs_start", C.c_void_p), ("obs_kf", C.c_void_p), ("obs_idx", C.c_void_p), ("obs_w", C.c_void_p), ("point_bad", C.c_void_p),
                ("n_kf", C.c_int32), ("kf_gone", C.c_void_p), ("row_level", C.c_void_p), ("obs_level", C.c_void_p), ("kf_keys", C.c_void_p),
                ("row_depth", C.c_void_p), ("kf_depth", C.c_void_p), ("th_depth", C.c_float), ("monocular", C.c_int32)]


class CullParams(C.Structure):
    _fields_ = [("mode", C.c_int32), ("th_obs", C.c_int32), ("max_culls", C.c_int32), ("force_class", C.c_int32), ("ratio", C.c_double)]


def cull_prototypes(l):
    P, I = C.c_void_p, C.c_int32
    l.plf_keyframe_culling.argtypes = [C.POINTER(CullView), C.POINTER(CullParams), P, P, I, P, P, P, P, P, P, P, I, P]
    l.plf_map_point_culling.argtypes = [I, P, P, P, P, P, P, P, I, P, C.c_int64, I, P, I, P]
    return l


# ---- local map (include/plf.h, "Local map")
class LocalKfView(C.Structure):
    _fields_ = [("n_rows", C.c_int32), ("seed_kf", C.c_void_p), ("n_seed", C.c_void_p), ("seed_stride", C.c_int32), ("covis_kf", C.c_void_p),
                ("n_covis", C.c_void_p), ("covis_stride", C.c_int32), ("child_start", C.c_void_p), ("child_kf", C.c_void_p), ("kf_parent", C.c_void_p),
                ("kf_bad", C.c_void_p), ("n_kf", C.c_int32)]


class LocalKfParams(C.Structure):
    _fields_ = [("n_best", C.c_int32), ("max_local", C.c_int32), ("kf_stride", C.c_int32), ("dense_max_kf", C.c_int32)]


class LocalItemsView(C.Structure):
    _fields_ = [("n_rows", C.c_int32), ("local_kf", C.c_void_p), ("n_local_kf", C.c_void_p), ("kf_stride", C.c_int32), ("kf_row_start", C.c_void_p),
                ("kf_row_item", C.c_void_p), ("n_kf", C.c_int32), ("item_bad", C.c_void_p), ("n_items", C.c_int32), ("frame_row_start", C.c_void_p),
                ("frame_row_item", C.c_void_p)]


class LocalItemsParams(C.Structure):
    _fields_ = [("item_stride", C.c_int32), ("table_slots", C.c_int32)]


class LocalMapSrc(C.Structure):
    _fields_ = [("world_pos", C.c_void_p), ("normal", C.c_void_p), ("min_distance", C.c_void_p), ("max_distance", C.c_void_p), ("desc", C.c_void_p),
                ("map_rows", C.c_int32), ("pos_floats", C.c_int32)]


class LocalMapDst(C.Structure):
    _fields_ = [("world_pos", C.c_void_p), ("normal", C.c_void_p), ("min_distance", C.c_void_p), ("max_distance", C.c_void_p), ("desc", C.c_void_p)]


def localmap_prototypes(l):
    P, I = C.c_void_p, C.c_int32
    l.plf_local_keyframes.argtypes = [C.POINTER(LocalKfView), C.POINTER(LocalKfParams), P, P, P, I, P]
    l.plf_local_items.argtypes = [C.POINTER(LocalItemsView), C.POINTER(LocalItemsParams), P, P, P, P, I, P]
    l.plf_local_gather.argtypes = [P, P, I, I, C.POINTER(LocalMapSrc), C.POINTER(LocalMapDst), I, P]
    l.plf_local_visible.argtypes = [P, P, P, I, I, P, P, P, P, P, P, I, I, P]
    return l


# ---- pose optimisation (include/plf.h, "Pose optimisation")
POSE_EARLY, POSE_NONFINITE = 1, 2
POSE_COMMIT_DISCARD, POSE_COMMIT_FOUND = 0, 1


class Camera(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3", "bf")]


class PoseView(C.Structure):
    _fields_ = [("n_frames", C.c_int32), ("kp_stride", C.c_int32), ("pos_stride", C.c_int32), ("keys_un", C.c_void_p), ("uright", C.c_void_p),
                ("n_device", C.c_void_p), ("n_host", C.c_int32), ("match_of_kp", C.c_void_p), ("world_pos", C.c_void_p),
                ("inv_level_sigma2", C.c_void_p), ("nlevels", C.c_int32)]


def pose_prototypes(l):
    P, I = C.c_void_p, C.c_int32
    l.plf_pose_optimize.argtypes = [C.POINTER(PoseView), C.POINTER(Camera), P, I, P, P, P, P, P, I, P]
    l.plf_pose_commit.argtypes = [I, P, P, P, I, I, I, P, I, P, I, P, P, I, P]
    return l


# ---- tracking tail (include/plf.h, "Tracking tail")
TRACK_OVERFLOW, TRACK_NONFINITE = 1, 1
TRACK_CLOSE_LIST, TRACK_CLOSE_KEYFRAME, TRACK_CLOSE_LASTFRAME = 0, 1, 2
TRACK_ONLY_TRACKING, TRACK_MAPPER_STOPPED, TRACK_MAPPER_IDLE, TRACK_MONO = 1, 2, 4, 8
TRACK_MOTION_VELOCITY, TRACK_MOTION_PREDICT, TRACK_MOTION_LASTPOSE = 1, 2, 4
TRACK_CLEAN_VO, TRACK_CLEAN_OUTLIERS = 0, 1
TRACK_KF_STATE_DTYPE = np.dtype([("frame_id", "<i8"), ("ref_kf", "<i4"), ("n_matches_inliers", "<i4"), ("last_kf_id", "<u4"),
                                 ("last_reloc_frame_id", "<u4"), ("min_frames", "<i4"), ("max_frames", "<i4"), ("n_kfs", "<i4"), ("flags", "<i4")])


class TrackView(C.Structure):
    _fields_ = [("n_frames", C.c_int32), ("kp_stride", C.c_int32), ("keys_un", C.c_void_p), ("depth", C.c_void_p), ("match_of_kp", C.c_void_p),
                ("n_device", C.c_void_p), ("n_host", C.c_int32), ("row_id", C.c_void_p), ("id_stride", C.c_int32), ("n_obs", C.c_void_p),
                ("n_points", C.c_int32), ("pose", C.c_void_p)]


class TrackCloseParams(C.Structure):
    _fields_ = [("th_depth", C.c_float), ("min_points", C.c_int32), ("mode", C.c_int32), ("new_stride", C.c_int32)]


class TrackLastFrameOut(C.Structure):
    _fields_ = [("has_mappoint", C.c_void_p), ("world_pos", C.c_void_p), ("obs_positive", C.c_void_p)]


class TrackKfView(C.Structure):
    _fields_ = [("kf_row_start", C.c_void_p), ("kf_row_item", C.c_void_p), ("n_kf", C.c_int32), ("item_bad", C.c_void_p)]


def track_prototypes(l):
    P, I = C.c_void_p, C.c_int32
    l.plf_track_close_points.argtypes = [C.POINTER(TrackView), C.POINTER(Camera), C.POINTER(TrackCloseParams), P, C.POINTER(TrackLastFrameOut),
                                         P, P, P, P, P, I, P]
    l.plf_track_need_keyframe.argtypes = [C.POINTER(TrackView), C.POINTER(TrackKfView), P, P, C.c_float, P, P, I, P]
    l.plf_track_motion.argtypes = [I, I, P, P, P, P, P, P, P, P, P, P, P, I, P]
    l.plf_track_clean.argtypes = [I, P, P, P, I, I, I, P, I, P, I, I, P]
    return l


# ---- new map points (include/plf.h, "New map points")
TRI_OVERFLOW, TRI_SKIPPED_BASELINE, TRI_BAD_SLOT = 1, 2, 4
(TRI_NO_PAIR, TRI_CREATED, TRI_NO_BRANCH, TRI_W_ZERO, TRI_Z1, TRI_Z2, TRI_REPROJ1, TRI_REPROJ2, TRI_ZERO_DIST, TRI_SCALE, TRI_BAD_I2) = range(1, 12)
TRI_BRANCH_SVD, TRI_BRANCH_KF1, TRI_BRANCH_KF2, TRI_BRANCH_MASK = 0x10, 0x20, 0x30, 0x30


class TriangulateView(C.Structure):
    _fields_ = [("n_kf", C.c_int32), ("kf_keys", C.c_void_p), ("kf_uright", C.c_void_p), ("kf_depth", C.c_void_p), ("kf_n", C.c_void_p),
                ("kf_pose", C.c_void_p), ("scale_factors", C.c_void_p), ("level_sigma2", C.c_void_p), ("nlevels", C.c_int32),
                ("scale_factor", C.c_float), ("mb", C.c_float), ("mbf", C.c_float)]


class TriangulateJobs(C.Structure):
    _fields_ = [("n_jobs", C.c_int32), ("kp_stride", C.c_int32), ("new_stride", C.c_int32), ("job_kf1", C.c_void_p), ("job_kf2", C.c_void_p),
                ("match12", C.c_void_p)]


class TriangulateMarks(C.Structure):
    _fields_ = [("kf_has_mp", C.c_void_p), ("kf_mappoints", C.c_void_p), ("id_base", C.c_void_p)]


def tri_prototypes(l, name="plf_triangulate_points"):
    """the device call; name="tri_cpu_points": the host loop tools/tri_cpu.cpp, the same signature without device and stream"""
    P, I = C.c_void_p, C.c_int32
    tail = [I, P] if name == "plf_triangulate_points" else []
    getattr(l, name).argtypes = [C.POINTER(TriangulateView), C.POINTER(Camera), C.POINTER(TriangulateJobs), C.POINTER(TriangulateMarks), P, P, P, P, P, P] + tail
    return l


class Sim3View(C.Structure):
    _fields_ = [("n_kf", C.c_int32), ("kf_keys", C.c_void_p), ("kf_n", C.c_void_p), ("kf_pose", C.c_void_p), ("kf_mappoints", C.c_void_p),
                ("kf_obs_index", C.c_void_p), ("world_pos", C.c_void_p), ("point_bad", C.c_void_p), ("n_points", C.c_int32),
                ("level_sigma2", C.c_void_p), ("nlevels", C.c_int32)]


class Sim3Jobs(C.Structure):
    _fields_ = [("n_jobs", C.c_int32), ("kp_stride", C.c_int32), ("pair_stride", C.c_int32), ("job_kf1", C.c_void_p), ("job_kf2", C.c_void_p),
                ("match12", C.c_void_p), ("fix_scale", C.c_void_p)]


class Sim3PairSet(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("idx1", "x3dc1", "x3dc2", "max_err1", "max_err2", "p1im1", "p2im2", "n_pairs", "status")]


class Sim3State(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("iterations_done", "best_inliers", "best_iter", "max_its", "best_sim3", "no_more")]


class Sim3Hits(C.Structure):
    _fields_ = [("max_hits", C.c_int32)] + [(n, C.c_void_p) for n in ("n_hits", "hit_iter", "hit_inliers", "hit_sim3", "hit_inlier12")]


def sim3_prototypes(l, prefix="plf_sim3"):
    """the device calls; prefix="sim3_cpu": the host loops of tools/sim3_cpu.cpp, the same signatures without device and stream"""
    P, I = C.c_void_p, C.c_int32
    tail = [I, P] if prefix == "plf_sim3" else []
    getattr(l, prefix + "_its_for_n").argtypes = [C.c_double, I, I, I, P]
    getattr(l, prefix + "_pairs").argtypes = [C.POINTER(Sim3View), C.POINTER(Camera), C.POINTER(Sim3Jobs), P, C.POINTER(Sim3PairSet), C.POINTER(Sim3State)] + tail
    getattr(l, prefix + "_iterate").argtypes = [C.POINTER(Sim3Jobs), C.POINTER(Camera), C.POINTER(Sim3PairSet), P, I, I, I, P, C.POINTER(Sim3State), P,
                                                C.POINTER(Sim3Hits)] + tail
    return l


class Sim3OptJobs(C.Structure):
    _fields_ = [("n_jobs", C.c_int32), ("kp_stride", C.c_int32), ("job_kf1", C.c_void_p), ("job_kf2", C.c_void_p), ("sim3_in", C.c_void_p),
                ("fix_scale", C.c_void_p), ("inv_level_sigma2", C.c_void_p), ("th2", C.c_float)]


def sim3opt_prototypes(l, prefix="plf_sim3"):
    """the device calls; prefix="sim3opt_cpu": the host loops of tools/sim3opt_cpu.cpp, the same signatures without device and stream (the optimise
    loop takes one more pointer: the iteration counts)"""
    P, I = C.c_void_p, C.c_int32
    tail = [I, P] if prefix == "plf_sim3" else []
    getattr(l, prefix + "_optimize").argtypes = [C.POINTER(Sim3View), C.POINTER(Camera), C.POINTER(Sim3OptJobs), P, P, P, P, P] + (tail or [P])
    getattr(l, prefix + "_keep_inliers").argtypes = [P, P, P, I, I] + tail
    return l


# ---- loop correction (include/plf.h, "Loop correction")
class LoopView(C.Structure):
    _fields_ = [("K", C.c_int32), ("rank_kf", C.c_void_p), ("row_start", C.c_void_p), ("row_point", C.c_void_p), ("n_points", C.c_int32),
                ("point_bad", C.c_void_p), ("n_kf", C.c_int32), ("kf_id", C.c_void_p)]


class GbaView(C.Structure):
    _fields_ = [("n_kf", C.c_int32), ("parent", C.c_void_p), ("origins", C.c_void_p), ("n_origins", C.c_int32), ("kf_flag", C.c_void_p),
                ("tcw_gba", C.c_void_p), ("kf_tcw", C.c_void_p), ("kf_ow", C.c_void_p), ("tcw_bef", C.c_void_p)]


def loopfix_prototypes(l, prefix="plf"):
    """the device calls; prefix="loopfix_cpu": the host loops of tools/loopfix_cpu.cpp, the same signatures without device and stream"""
    P, I, Q = C.c_void_p, C.c_int32, C.c_int64
    dev = prefix == "plf"
    tail = [I, P] if dev else []
    lp, gb = (prefix + "_loop_", prefix + "_gba_") if dev else (prefix + "_", prefix + "_gba_")
    getattr(l, lp + "scw").argtypes = [P, P, I, I, P] + tail
    getattr(l, lp + "sim3_pairs").argtypes = [P, P, I, P, I, I, P, P, P] + tail
    getattr(l, lp + "correct_points").argtypes = [C.POINTER(LoopView), P, P, Q, P, P, P, P] + tail
    getattr(l, lp + "new_poses").argtypes = [P, I, P, P] + tail
    getattr(l, lp + "commit_poses").argtypes = [P, I, P, P, P, P, I] + tail
    getattr(l, lp + "normal_depth").argtypes = [C.POINTER(MapGeomView), P, P, I, P, P, P, P, P, I, P] + tail
    getattr(l, lp + "correct_points_by_ref").argtypes = [I, P, P, P, P, Q, P, Q, P, P, I, P, P] + tail
    getattr(l, gb + "propagate_poses").argtypes = [C.POINTER(GbaView)] + tail
    getattr(l, gb + "correct_points").argtypes = [I, P, P, P, P, P, P, P, P, I, P] + tail
    if not dev:   # the loops as the reference writes them (tools/loopfix_cpu.cpp)
        l.loopfix_cpu_correct_loop.argtypes = [C.POINTER(LoopView), C.POINTER(MapGeomView), P, P, Q, P, P, P, P, P, P, P, P, P, P]
        l.loopfix_cpu_gba_children.argtypes = [C.POINTER(GbaView), P, P]
        l.loopfix_cpu_gba_queue.argtypes = [C.POINTER(GbaView), P, P]
    return l

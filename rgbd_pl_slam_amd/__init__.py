"""rgbd_pl_slam_amd -- MI355X-native point+line feature front-end (ORB + LSD/LBD + Hamming matchers)
behind the call shapes of maxee1900/RGBD-PL-SLAM.  The compute path is libplf_hip.so (HIP, gfx950);
this package is the thin host-side mirror used by tests and bench.  No CPU fallback exists."""
from ._lib import PlfError, LIB_PATH  # noqa: F401
from .orb import ORBextractor  # noqa: F401
from .lines import LineSegment  # noqa: F401
from .matcher import Matcher, DescriptorDistance  # noqa: F401
from . import frame  # noqa: F401
from .bow import Vocabulary  # noqa: F401
from .kfdb import KeyFrameDatabase  # noqa: F401
from . import mappoints  # noqa: F401
from .mappoints import distinctive_descriptors, update_normal_and_depth, kf_keys_table, MapPoint, MapLine  # noqa: F401
from . import covisibility  # noqa: F401
from .covisibility import update_connections, local_keyframe_votes, Covisibility  # noqa: F401
from . import culling  # noqa: F401
from .culling import keyframe_culling, map_point_culling, CullMap  # noqa: F401
from . import localmap  # noqa: F401
from .localmap import local_keyframes, local_items, local_gather, local_visible, update_local_map, children_csr, LocalMap  # noqa: F401
from . import pose  # noqa: F401
from .pose import pose_optimization, pose_commit, PoseResult  # noqa: F401
from . import track  # noqa: F401
from .track import close_points, need_new_keyframe, motion_model, clean_matches, kf_state  # noqa: F401
from . import triangulate  # noqa: F401
from .triangulate import triangulate_points, KeyFrameSet  # noqa: F401
from . import sim3  # noqa: F401
from .sim3 import sim3_pairs, sim3_iterate, Sim3Solver, Sim3KeyFrames  # noqa: F401
from . import sim3opt  # noqa: F401
from .sim3opt import sim3_optimize, sim3_keep_inliers  # noqa: F401
from . import loopfix  # noqa: F401
from .loopfix import loop_scw, loop_sim3_pairs, loop_correct, essential_graph_correct, gba_correct  # noqa: F401

// loopfix_kernels.hip -- LoopClosing::CorrectLoop's pose propagation and map-point moves, and the point / pose tails of
// Optimizer::OptimizeEssentialGraph and LoopClosing::RunGlobalBundleAdjustment, on the device (include/plf.h, "Loop correction").  The arithmetic is
// loopfix_common.h's, the one header the host loop tools/loopfix_cpu.cpp compiles too; this file is only the schedule.
//
// Schedule.  The reference corrects a point once, by the first keyframe of an ordered walk that holds it.  In parallel that is an ownership rule: the
// owner of a point is the lowest rank whose row holds it.
//   k_loop_claim   one workgroup per rank (grid = K, no cap): its 256 lanes stride the rank's row of row_point, so a wave reads 256 contiguous bytes
//                  per step; an entry that the walk would not skip does atomicMin(owner_rank[p], rank).  Integer minimum: the result does not depend
//                  on arrival order.  owner_rank was set to LOOPFIX_NONE by a memset on the stream.
//   k_loop_move    one point per lane (grid = ceil(n_points / 256), no cap, so there is no second pass of a workgroup): reads the owner, loads the
//                  owner's two Sim3 (16 doubles, L2-resident: K rows), inverts the corrected one in registers (one division pair and a rotation: less
//                  than the latency of the loads it sits between), moves the point, writes the two marks.  12 B read + 12 B written per moved point
//                  plus 4 + 16 B of marks: memory-bound; double arithmetic in registers, no local arrays indexed at run time, no scratch.
//   k_loop_by_ref  the same move with the Sim3 pair chosen per point by keyframe slot; one point per lane.
//   k_gba_points   float only; one point per lane.
//   the per-rank and per-keyframe kernels (pairs, new poses, commit) are one item per lane over K or n_kf items: tens to thousands of lanes,
//   latency-bound, nothing to schedule.
//   the GBA pose tail: k_gba_mark / k_gba_init, then ceil(log2(n_kf)) launches of k_gba_jump (anc = anc[anc], double-buffered) decide which keyframes
//   hang below an origin without any lane walking the depth of the tree; k_gba_chain then walks only the unflagged keyframes above its own (the chain
//   is sequential by nature), k_gba_commit sets the poses in a launch of its own because the chain reads the old ones.
// No kernel of THIS file caps its grid: a lane's index is its item.  The staged UpdateNormalAndDepth runs in mapgeom_kernels.hip, whose kernels do
// cap their grids and walk grid-stride loops (tests/test_gpu_loopfix.py runs them past every cap with the staged fields set).
#include "plf_common.h"
#include "loopfix_common.h"

__device__ __forceinline__ int64_t lf_item() { return (int64_t)blockIdx.x * LOOPFIX_THREADS + threadIdx.x; }

__global__ void __launch_bounds__(64) k_loop_scw(LfScwArgs a)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) lf_scw(a);
}

__global__ void __launch_bounds__(LOOPFIX_THREADS) k_loop_pairs(LfPairsArgs a)
{
    const int64_t r = lf_item();
    if (r < a.K) lf_pairs_one(a, (int)r);
}

__global__ void __launch_bounds__(LOOPFIX_THREADS) k_loop_claim(LfPointsArgs a)
{
    const int r = blockIdx.x;
    const int64_t s = a.v.row_start[r], e = a.v.row_start[r + 1];
    if (s < 0) return;
    for (int64_t i = s + threadIdx.x; i < e; i += LOOPFIX_THREADS) {
        const int32_t p = lf_claimed_point(a, r, i);
        if (p >= 0) atomicMin(&a.owner_rank[p], r);
    }
}

__global__ void __launch_bounds__(LOOPFIX_THREADS) k_loop_move(LfPointsArgs a)
{
    const int64_t p = lf_item();
    if (p < a.v.n_points) lf_move_point(a, p);
}

__global__ void __launch_bounds__(LOOPFIX_THREADS) k_loop_new_poses(LfPoseArgs a)
{
    const int64_t r = lf_item();
    if (r < a.K) lf_new_pose(a, (int)r);
}

__global__ void __launch_bounds__(LOOPFIX_THREADS) k_loop_commit_poses(LfPoseArgs a)
{
    const int64_t r = lf_item();
    if (r < a.K) lf_commit_pose(a, (int)r);
}

__global__ void __launch_bounds__(LOOPFIX_THREADS) k_loop_by_ref(LfByRefArgs a)
{
    const int64_t p = lf_item();
    if (p < a.n_points) lf_by_ref_point(a, p);
}

__global__ void __launch_bounds__(LOOPFIX_THREADS) k_gba_mark(LfGbaArgs a)
{
    const int64_t i = lf_item();
    if (i < a.v.n_origins) lf_gba_mark_origin(a, (int32_t)i);
}

__global__ void __launch_bounds__(LOOPFIX_THREADS) k_gba_init(LfGbaArgs a)
{
    const int64_t k = lf_item();
    if (k < a.v.n_kf) lf_gba_init(a, (int32_t)k);
}

__global__ void __launch_bounds__(LOOPFIX_THREADS) k_gba_jump(LfGbaArgs a)
{
    const int64_t k = lf_item();
    if (k < a.v.n_kf) lf_gba_jump(a, (int32_t)k);
}

__global__ void __launch_bounds__(LOOPFIX_THREADS) k_gba_chain(LfGbaArgs a)
{
    const int64_t k = lf_item();
    if (k < a.v.n_kf) lf_gba_chain(a, (int32_t)k);
}

__global__ void __launch_bounds__(LOOPFIX_THREADS) k_gba_commit(LfGbaArgs a)
{
    const int64_t k = lf_item();
    if (k < a.v.n_kf) lf_gba_commit(a, (int32_t)k);
}

__global__ void __launch_bounds__(LOOPFIX_THREADS) k_gba_points(LfGbaPointsArgs a)
{
    const int64_t p = lf_item();
    if (p < a.n_points) lf_gba_point(a, p);
}

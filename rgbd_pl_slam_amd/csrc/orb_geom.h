// orb_geom.h -- per-handle geometry of the ORB pipeline shared by host code and kernels.
#pragma once
#include <stdint.h>

#define PLF_MAX_LEVELS 12
#define PLF_EDGE 19        // EDGE_THRESHOLD of the reference (so@0x7609c: 19 - 3 = 16)
#define PLF_MINB 16        // minBorderX/Y
#define PLF_HALF_PATCH 15
#define PLF_PATCH 31
#ifndef PLF_ORB_LEVEL_THREADS
#define PLF_ORB_LEVEL_THREADS 256   // workgroup size of k_orb_level (one tile of 2 x 2 cells): 4 waves x 72 VGPRs still fit a CU next to 16 region-growing waves
#endif

struct OrbLevel {
    int w, h;            // level image (interior) size
    int ppitch;          // padded plane pitch = w + 38
    uint32_t plane_off;  // byte offset of the padded plane inside one frame's pyramid block
    int bpitch;          // pitch of the blurred / score planes (multiple of 64)
    uint32_t blur_off;   // byte offset inside one frame's blur block (score block uses the same offsets)
    int ncells;          // FAST cells of this level
    int cell_base;       // index of the first cell in the cell table
    int wCell, hCell;
    int quota;           // mnFeaturesPerLevel[l]
    float scale;         // mvScaleFactor[l]
    int size_i;          // int(31 * scale), so@0x76996
    uint32_t pool_off;   // candidate pool: first entry inside one frame's pool block
    uint32_t pool_cap;   // entries
    uint32_t sel_off;    // selected keypoints: first entry inside one frame's sel block
    uint32_t sel_cap;    // quota + 8
    uint32_t tabx_off, taby_off;  // resize coefficient tables (levels >= 1)
    // k_orb_level: the effective cell grid (cells skipped by the reference's loop are at the row / column ends), tiles of 2 x 2 cells, and the
    // end of the last cell's computed region (cell sub-image minus its 3-pixel frame; the regions of neighbouring cells abut)
    int ncx, ncy, tcx, tcy, rex, rey;
    int tile_base;       // k_orb_level covers all levels in one launch: first workgroup of this level (OrbGeom::tiles_total in all)
};

struct OrbGeom {
    int nlevels;
    int iniTh, minTh;
    int in_w, in_h;
    int cells_total;
    int maxsel;            // max over levels of sel_cap
    uint32_t pyr_stride;   // bytes per frame
    uint32_t blur_stride;  // bytes per frame
    uint32_t pool_stride;  // entries per frame
    uint32_t sel_stride;   // entries per frame
    int tiles_total;       // workgroups of k_orb_level (tiles of all levels of one frame)
    // LDS layout of k_orb_level (bytes; maxima over the levels): pixel tile pitch, score tile pitch, byte offsets of the survivor list, the score tile and the
    // per-wave corner queues of the non-maximum suppression
    int lds_pw, lds_sp, lds_off_list, lds_off_s, lds_off_q, lds_total;
    int lds_list_cap;    // entries of the FAST survivor list: half the pixels of the largest computed region of a tile (k_orb_level redoes denser passes in two row halves)
    OrbLevel lv[PLF_MAX_LEVELS];
};

// Row-walking kernels of the ORB front (k_orb_pyramid, k_orb_blur): a wave owns PLF_ORB_SPAN columns (4 per lane) and a band of rows.  The band height follows the
// frames in flight: a few frames need many short waves to fill the chip, a large batch long ones that amortise a band's lead-in.
#define PLF_ORB_SPAN 256
#ifdef __HIPCC__
__host__ __device__
#endif
static inline int orb_band_shift(int frames) { return frames <= 4 ? 3 : frames <= 16 ? 4 : 5; }   // bands of 8 / 16 / 32 rows
// workgroups (one wave each) of a level: k_orb_pyramid covers the padded plane's columns and the level's rows, k_orb_blur the level's columns and rows
#ifdef __HIPCC__
__host__ __device__
#endif
static inline int orb_pyr_spans(const OrbLevel &L) { return (L.ppitch + PLF_ORB_SPAN - 1) / PLF_ORB_SPAN; }
#ifdef __HIPCC__
__host__ __device__
#endif
static inline int orb_blur_spans(const OrbLevel &L) { return (L.w + PLF_ORB_SPAN - 1) / PLF_ORB_SPAN; }
#ifdef __HIPCC__
__host__ __device__
#endif
static inline int orb_bands(const OrbLevel &L, int band_shift) { return (L.h + (1 << band_shift) - 1) >> band_shift; }

// LDS of k_octree (byte offsets into the dynamic block, by descending alignment): node state, cap_nodes entries of 56 bytes, the sort / best-key words and the
// scanned cell counts of the gather (`off`, one int per cell of the level with the most cells).  The host sizes the launch with .total, the kernel carves the
// block with the offsets.
struct OctLds {
    uint32_t ccnt, skey, rectA, rectB, nA, nB, slot_of, mid, off, newpos, work, candA, candB, misc, total;
};
#define PLF_OCT_MISC_INTS 48   // wave totals of the block scans (2 x 3 x 4), broadcast word, root counts (8)
#ifdef __HIPCC__
__host__ __device__
#endif
static inline OctLds orb_octree_lds(int cap_nodes, int cap_sort, int cap_cells)
{
    OctLds o;
    const uint32_t C = (uint32_t)cap_nodes, NC = (uint32_t)cap_cells;
    uint32_t p = 0;
    o.ccnt = p; p += 16 * C;
    p = (p + 7) & ~7u;
    o.skey = p; p += 8 * (uint32_t)cap_sort;
    o.rectA = p; p += 8 * C;
    o.rectB = p; p += 8 * C;
    o.nA = p; p += 4 * C;
    o.nB = p; p += 4 * C;
    o.slot_of = p; p += 4 * C;
    o.mid = p; p += 4 * C;
    o.off = p; p += 4 * NC;
    o.newpos = p; p += 2 * C;
    o.work = p; p += 2 * C;
    o.candA = p; p += 2 * C;
    o.candB = p; p += 2 * C;
    p = (p + 3) & ~3u;
    o.misc = p; p += 4 * PLF_OCT_MISC_INTS;
    o.total = p;
    return o;
}

#ifdef __HIPCC__
#include "plf_common.h"
// the __constant__ tables of orb_kernels.hip, uploaded when a handle is created
void plf_orb_upload_constants(const int *umax16);
// batch driver (batch_host.hip): the status word of the batch just enqueued on `s`, copied to pinned host memory in stream order (orb_host.hip)
int plf_orb_status_async(plf_orb *h, int32_t *host_dst, hipStream_t s);

// Register budget of the ORB front kernels: 8 waves per SIMD = at most 64 VGPRs.  Not for their own occupancy but for co-residency: four region-growing waves
// hold 416 of a SIMD's 512 VGPRs for 80 ms, and in the 96 that are left a 56-register ORB wave fits TOGETHER with a matcher wave (40-48), an 80-register one
// alone: +2.5 % for the pipeline.
#ifndef PLF_ORB_LEVEL_WPE
#define PLF_ORB_LEVEL_WPE 8
#endif
#define OF_OCC __attribute__((amdgpu_waves_per_eu(PLF_ORB_LEVEL_WPE, PLF_ORB_LEVEL_WPE)))
// issue priority above the other throughput kernels (matchers, k_lsd_pre, NFA stages: 0), below the region chain (3)
#ifndef PLF_ORB_PRIO
#define PLF_ORB_PRIO 2
#endif
typedef uint32_t __attribute__((aligned(1))) plf_u32u;
typedef short plf_s2v __attribute__((ext_vector_type(2)));

// ---- kernels launched by orb_host.hip (orb_pyramid.hip, orb_front.hip, orb_octree.hip, orb_kernels.hip)
__global__ void k_orb_pyramid(const uint8_t *in, ptrdiff_t in_pitch, ptrdiff_t in_fstride, uint8_t *pyr, int l, int band_shift, const int *xofs, const short2 *xa, const int *yofs, const short2 *yb,
                              OrbGeom g);
__global__ void k_orb_blur(const uint8_t *pyr, uint8_t *blur, int band_shift, OrbGeom g, int4 taps);
__global__ void k_orb_level(const uint8_t *pyr, const int4 *cells, int2 *cellinfo, uint2 *pool, int *poolcnt, int *status, OrbGeom g);
__global__ void k_octree(const int2 *cellinfo, const uint2 *pool, uint2 *keys_all, int *nodeof_all, uint8_t *quad_all, uint2 *sel, int *selcnt, int *ncand_dbg, int *status, OrbGeom g,
                         int cap_nodes, int cap_sort, int cap_cells);
__global__ void k_orient_brief(const uint8_t *pyr, const uint8_t *blur, const uint2 *sel, const int *selcnt, plf_keypoint *kps, uint8_t *desc, int *n_out, int capacity, int *status, OrbGeom g,
                               int nframes);
#endif

// Internal kernel interface of liborbx (not part of the C ABI).
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/orbx.h"
#include "orbx_geom.hpp"

namespace orbx {

// Where the levels of frame f live.  Level 0 is the caller's image (no copy);
// levels >= 1 are in the handle's pyramid block.
struct FramePtrs {
    const uint8_t* in;
    size_t in_fstride;
    int in_pitch;
    uint8_t* pyr;
    size_t pyr_fstride;
};

// The device tables of one image size: written once, then only read
struct GeomTabs {
    const Geometry* geom;       // device copy
    const Cell* cells;          // device cell table
    const int2* xtab;           // resize tables (levels >= 1)
    const int2* ytab;
    const int4* pyr_bands;      // K1 small-batch band tables (Geometry::pg)
};

struct ExtractBufs : GeomTabs {
    uint32_t* slots;            // [B][slots_per_frame] FAST candidates
    int* cell_counts;           // [B][ncells]
    uint32_t* spill;            // [B][spill_per_frame] quadtree overflow (packed kp)
    uint32_t* spill_node;       // [B][spill_per_frame]
    uint8_t* qt_nodes;          // [B][qtg_per_frame] K3 node arrays of the levels whose list outgrows LDS
    uint32_t* qt_out;           // [B][out_per_frame] retained keypoints (level coords)
    int* qt_cnt;                // [B][nlevels]
    int* status;                // device error word (bit flags)
    int resize_mode;            // ORBX_RESIZE_* (orbx_set_cv_modes): K1's vertical pass
    int blur_mode;              // ORBX_BLUR_*: K4's GaussianBlur column pass and kernel
};

// XCD-aware workgroup order.  The dispatcher hands flat workgroup id b to XCD b % 8;
// each XCD has its own 4 MiB L2.  xcd_block maps b to a logical id so that every
// XCD owns one contiguous range of logical ids (whole frames, in order), so the
// overlapping reads of neighbouring cells / keypoint patches hit that XCD's L2.
constexpr int kXcds = 8;
__device__ __forceinline__ int xcd_block(int b, int nblocks)
{
    const int q = nblocks / kXcds, r = nblocks - q * kXcds;
    const int x = b % kXcds, k = b / kXcds;
    return x * q + min(x, r) + k;
}

enum : int {
    kStatusListOverflow = 1,
    kStatusOutOverflow = 2,
    kStatusCapOverflow = 4,
};

// K3 launch plan: runs of consecutive levels sharing a kernel configuration.  glob: the node arrays
// live in global memory (ExtractBufs::qt_nodes) because lcap nodes need more LDS than a workgroup has.
struct QtGroup {
    int l0, nl, nt, kpt, glob, lcap, cellcap;
};
constexpr int kQtMaxGroups = kMaxLevels + 1;
int qt_plan(const Geometry& g, int batch, QtGroup* out);   // returns the group count
// per level: the launched template (nt, kpt, glob, wide), its capacities, the gather's owner-map room in bytes
// and the index of its launch (eight ints, the rows of orbx_debug_qt_plan)
struct QtLevelPlan {
    int nt, kpt, glob, wide, lcap, cellcap, gather_room, launch;
};
void qt_report(const Geometry& g, int batch, QtLevelPlan* out);   // out[g.nlevels]
// host: decides qt_glob per level and lays out the per-frame global node block (qtg_*); false if a
// level cannot be run at all
bool qt_prepare(Geometry& g);
constexpr int kQtMergedMaxBatch = 8;   // batches up to this size run all levels in one launch
constexpr int kLatencyMaxBatch = 8;    // batches up to this size: FAST one cell per wave, describe one keypoint per wave
// cell_counts flag: the cell's candidates start at its own slot base (it did not fit its wave's output buffer).
// Otherwise they follow the wave's earlier cells' in one run from the slot base of the wave's first cell
// (kCellsPerWave consecutive cells of the level above kLatencyMaxBatch frames, one cell below), so a cell's
// first slot is that base plus the counts of the wave's cells before it (orbx_quadtree.hip cell_slot_word).
constexpr uint32_t kCellDirect = 0x80000000u;
__host__ __device__ inline int fast_cells_per_wave(int batch) { return batch <= kLatencyMaxBatch ? 1 : kCellsPerWave; }
// Workgroup size and keypoints per thread of level l's quadtree: level 0 holds most candidates
// (KITTI ~6,800), level 1 ~2,700, levels >= 2 a few hundred.  Measured per launch (KITTI, 192 frames):
// fewer waves per workgroup on the small levels does not shorten them (one wave for levels 3-7:
// 70 us against 84 us for 256 threads on levels 2-7 together, plus a separate level-2 launch), since
// a split round is a chain of dependent LDS steps whatever the workgroup size.
// Levels whose node list runs from global memory (LevelGeom::qt_glob) take one configuration.
constexpr int kQtGlobNT = 512, kQtGlobKPT = 8;
__host__ __device__ inline int qt_nt(const Geometry& g, int l)
{
    return g.lv[l].qt_glob ? kQtGlobNT : (l >= 2 ? 256 : 512);
}
__host__ __device__ inline int qt_kpt(const Geometry& g, int l)
{
    return g.lv[l].qt_glob ? kQtGlobKPT : (l == 0 ? g.qt_kpt0 : (l == 1 ? 8 : 4));
}
__host__ __device__ inline int qt_regcap(const Geometry& g, int l) { return qt_nt(g, l) * qt_kpt(g, l); }

// host: K1 small-batch launch groups and their band tables (Geometry::pg) from the resize row tables
bool pyr_plan(Geometry& g, const Tap* yt, std::vector<int4>& bands);
// K1's launches for a batch: the fused kernel's, one per level group (small batches, where pyr_plan made groups),
// or one per level from the level before it; their count and the levels they read, as a bit mask
struct PyrLaunches { bool fused; int n, srcmask; };
PyrLaunches pyr_launches(const Geometry& g, int batch);
void launch_pyramid(const Geometry& g, const ExtractBufs& b, const FramePtrs& p, int batch, hipStream_t s);
size_t pyr_level_lds(const Geometry& g, int l);   // k_pyramid_level's dynamic LDS for level l (>= 1)
void fast_groups(Geometry& g);   // host: FAST launch groups (cell ranges, LDS sizes)
// K2's launches for a batch: cells [cb, ce) with per-wave LDS sized for an rw x rh ROI
struct FastRun { int cb, ce, rw, rh; };
constexpr int kFastMaxRuns = 2;   // Geometry::fast_groups at most
int fast_plan(const Geometry& g, int batch, FastRun* out);   // returns the launch count
void launch_fast(const Geometry& g, const ExtractBufs& b, const FramePtrs& p, int batch, hipStream_t s);
void launch_quadtree(const Geometry& g, const ExtractBufs& b, int* frame_counts, int batch, hipStream_t s);
void launch_describe(const Geometry& g, const ExtractBufs& b, const FramePtrs& p, orbx_keypoint* kps,
                     uint8_t* desc, int cap, int batch, hipStream_t s);

void launch_stereo(const Geometry& g, const Geometry* d_geom, const FramePtrs& PL, const FramePtrs& PR,
                   const orbx_keypoint* kps, const uint8_t* desc, const int* counts, int cap, const int* fl,
                   const int* fr, int npairs, float bf, float maxD, int rband, float* uright, float* depth, int* sad,
                   int* ngood, hipStream_t s);

}  // namespace orbx

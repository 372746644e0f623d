// gfx950 kernels of the ORB extractor (ORB_SLAM2::ORBextractor::operator(),
// src/ORBextractor.cc:1248-1334).  Integer/bitwise path: no MFMA.
//
//   K3 k_quadtree       DistributeOctTree, :644-907 (one workgroup per frame x level)
#include <hip/hip_runtime.h>

#include <algorithm>

#include "orbx_device.hpp"
#include "orbx_kernels.hpp"

namespace orbx {

// ---------------------------------------------------------------------------
// K3: DistributeOctTree (src/ORBextractor.cc:644-907), one workgroup per
// (frame, level).  Keypoints stay in registers (KPT per thread, overflow in a
// global spill array) and carry the list position of their node; nodes live in
// LDS arrays indexed by list position and are renumbered every round, so the
// std::list push_front/erase order is reproduced with prefix sums:
//   after a round the list is [children of the last split node (n4..n1), ...,
//   children of the first split node, surviving nodes in their old order].
// The phase-2 size sort breaks ties by creation order (canonical; the
// reference uses heap addresses).
// ---------------------------------------------------------------------------
constexpr int QT_NT = 512;
constexpr int QT_NW = QT_NT / 64;
#ifdef ORBX_QT_PROF
// per-level phase cycle sums (thread 0 of each workgroup): gather, init, phase-1 rounds, phase-2
// rounds, phase-2 sorts, retain, #phase-1 rounds, #phase-2 rounds, #workgroups
__device__ unsigned long long g_qt_prof[16][16];
// stamps accumulate in registers and are flushed once at the end: a global atomic per stamp would hold
// every later barrier (__syncthreads waits for the wave's outstanding memory operations)
#define QT_STAMP(slot, t0)                                                            \
    do {                                                                              \
        const long long t1_ = clock64();                                              \
        qt_acc[slot] += (unsigned long long)(t1_ - (t0));                             \
        t0 = t1_;                                                                     \
    } while (0)
#else
#define QT_STAMP(slot, t0) ((void)0)
#endif

// Inclusive wave64 prefix sum with DPP: row shifts within each 16-lane row, then row broadcasts
// (lane 15 into row 1 and 3, lane 31 into rows 2 and 3).  Six dependent VALU steps of a few cycles
// each, where a __shfl_up ladder is six ds_bpermute round trips through the LDS crossbar.
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v)
{
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xF, 0xF, true);   // row_shr:1
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xF, 0xF, true);   // row_shr:2
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xF, 0xF, true);   // row_shr:4
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xF, 0xF, true);   // row_shr:8
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xA, 0xF, false);  // row_bcast:15
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xC, 0xF, false);  // row_bcast:31
    return v;
}

// Exclusive scan of a[0..n) in LDS by the whole block; returns the total.  Each thread scans a
// contiguous run of per = ceil(n / NT) entries; wave totals meet in wsum, which every thread then
// reads whole (QT_NW broadcast reads) instead of waiting on one thread's serial pass.
template <int QT_NT>
__device__ uint32_t block_scan_excl(uint32_t* a, int n, uint32_t* wsum)
{
    constexpr int QT_NW = QT_NT / 64;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int per = (n + QT_NT - 1) / QT_NT;
    const int b = tid * per, e = min(n, b + per);
    uint32_t local = 0;
    for (int i = b; i < e; ++i) local += a[i];
    const uint32_t inc = wave_incl_scan(local);
    if (lane == 63) wsum[wid] = inc;
    __syncthreads();
    uint32_t before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < QT_NW; ++w) {
        const uint32_t t = wsum[w];
        before += w < wid ? t : 0u;
        total += t;
    }
    uint32_t run = before + inc - local;
    for (int i = b; i < e; ++i) {
        const uint32_t t = a[i];
        a[i] = run;
        run += t;
    }
    __syncthreads();
    return total;
}

// Exclusive scan of v(0..n) into a[]; returns the total.  v is evaluated (twice) by the thread whose run
// holds the element, so a scan whose terms come from LDS already in place needs no barrier before it.
template <int QT_NT, class F>
__device__ uint32_t block_scan_fn(uint32_t* a, int n, uint32_t* wsum, F&& v)
{
    constexpr int QT_NW = QT_NT / 64;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int per = (n + QT_NT - 1) / QT_NT;
    const int b = tid * per, e = min(n, b + per);
    uint32_t local = 0;
    for (int i = b; i < e; ++i) local += v(i);
    const uint32_t inc = wave_incl_scan(local);
    if (lane == 63) wsum[wid] = inc;
    __syncthreads();
    uint32_t before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < QT_NW; ++w) {
        const uint32_t t = wsum[w];
        before += w < wid ? t : 0u;
        total += t;
    }
    uint32_t run = before + inc - local;
    for (int i = b; i < e; ++i) {
        const uint32_t t = v(i);
        a[i] = run;
        run += t;
    }
    __syncthreads();
    return total;
}

__device__ __forceinline__ int next_pow2(int v)
{
    int p = 1;
    while (p < v) p <<= 1;
    return p;
}

// The slot of cell c's first candidate, in two steps around the level's exclusive count scan: before it, the
// word cell_slot_word (the cell's own slot base | kCellDirect for a directly written cell, else its wave's first
// cell's slot base), after it cell_slot_fix (the run offset: the counts of the wave's cells before c).  cpw:
// FAST's cells per wave for this batch (fast_cells_per_wave); level cell lists start at multiples of it.
static_assert(offsetof(Cell, slot_base) == 16 && alignof(Cell) >= 4 && sizeof(Cell) % 4 == 0,
              "cell_slot_base reads Cell::slot_base as dword 4");
__device__ __forceinline__ uint32_t cell_slot_base(const Cell* cells, int c)
{
    return ((const uint32_t*)(cells + c))[4];   // Cell::slot_base (a whole-dword scalar-friendly load)
}
__device__ __forceinline__ uint32_t cell_slot_word(const Cell* cells, int cb, int c, uint32_t raw, int cpw)
{
    return (raw & kCellDirect) ? (cell_slot_base(cells, cb + c) | kCellDirect) : cell_slot_base(cells, cb + c - c % cpw);
}
__device__ __forceinline__ uint32_t cell_slot_fix(uint32_t w, const uint32_t* scan, int c, int cpw)
{
    return (w & kCellDirect) ? (w & ~kCellDirect) : w + scan[c] - scan[c - c % cpw];
}

struct QtLayout {
    size_t scan, rect, cnt, srank, npos, snode, sinfo, ccnt, cpos, vprev, vnew, skey, best, wsum, sh, kpa, escan, total;
};

// Keypoints held in LDS instead of registers (kpa, one dword per register slot) by the wide LDS-node
// templates (16+ keypoints per thread): their 32 register arrays under the 128-VGPR budget spilled to
// scratch.  Slot r of thread t is kpa[t + r * NT], so a wave's accesses are conflict-free.
__host__ __device__ constexpr int qt_kpn(int nt, int kpt, int glob) { return (!glob && kpt >= 16) ? nt * kpt : 0; }

// ixb: bytes per node index (2 with the node arrays in LDS, 4 in global memory); kpn: LDS keypoint slots
__host__ __device__ inline QtLayout qt_layout(int lcap, int cellcap, int ixb = 2, int kpn = 0)
{
    QtLayout L;
    size_t o = 0;
    auto take = [&](size_t bytes) {
        const size_t r = o;
        o += (bytes + 15) & ~(size_t)15;
        return r;
    };
    // scans: the cells' counts (cellcap), a round's split ranks (<= lcap) and phase 2's non-split flags from
    // lcap + 1 (scan2), so 2 lcap + 2 entries cover the rounds
    const int scan_n = (2 * lcap + 2 > cellcap ? 2 * lcap + 2 : cellcap) + 1;
    L.scan = take(sizeof(uint32_t) * scan_n);
    L.rect = take(sizeof(int16_t) * 4 * 2 * lcap);   // [2 buffers][4 coords][lcap]
    L.cnt = take(sizeof(uint32_t) * 2 * lcap);
    L.srank = take((size_t)ixb * lcap);
    L.npos = take((size_t)ixb * lcap);
    L.snode = take((size_t)ixb * lcap);
    L.sinfo = take(sizeof(uint32_t) * lcap);
    L.ccnt = take(sizeof(uint32_t) * 4 * lcap);
    L.cpos = take((size_t)ixb * 4 * lcap);
    L.vprev = take((size_t)ixb * lcap);
    L.vnew = take((size_t)ixb * lcap);
    L.skey = take(sizeof(uint32_t) * (lcap + 4));   // + padding to whole 16-byte groups (rank sort)
    // the retain step's per-node best keys reuse the node rectangles (dead once the rounds end: 16 bytes per
    // node against 8), which takes 8 bytes per node off the workgroup's LDS
    L.best = L.rect;
    L.wsum = take(sizeof(uint32_t) * (QT_NW + 1));
    L.sh = take(sizeof(int) * 16);
    L.kpa = take(sizeof(uint32_t) * kpn);
    // the global-node form's prefixes of expandable children (step C), which the LDS forms pack into the high
    // halves of scan: no bytes with 16-bit indices
    L.escan = take(ixb == 4 ? sizeof(uint32_t) * (lcap + 1) : 0);
    L.total = o;
    return L;
}

// LDS of a global-node workgroup: the wave totals and the shared scalars only
constexpr size_t kQtGlobWsum = 0, kQtGlobSh = 64, kQtGlobSmem = 128;
// Largest LDS node layout a workgroup takes (the CU's 160 KiB); larger lists run from global memory.
// The LDS form packs a keypoint's child slot (4 * lcap) beside its node index in one 32-bit word.
constexpr size_t kQtLdsMax = 160 * 1024;
constexpr int kQtLdsMaxList = 16383;
// Step C of a round scans (children, expandable children) per split node in the 16-bit halves of one word: a
// list of lcap nodes splits into at most 4 * lcap children.  The global-node form scans the two apart.
static_assert(4 * kQtLdsMaxList < 0x10000, "the LDS forms' packed child / expandable-child prefixes would wrap");

// shared scalar slots
// SH_BIG: some phase-2 node holds more than 0xFFFF keys, so the packed (size, creation) sort key overflows
enum { SH_N = 0, SH_L, SH_PHASE, SH_M, SH_DONE, SH_KK, SH_ERR, SH_S, SH_C, SH_NEWL, SH_BIG };

// ctr[key] += 1 for every lane with key >= 0, one LDS atomic per run of equal keys in consecutive
// lanes.  Lanes hold consecutive candidates (cell order), which are spatial neighbours and mostly fall
// into the same node and quadrant: in the first split rounds thousands of keypoints meet at a handful
// of counters, and one atomic per lane serialises on them.  Called by whole waves (uniform control).
__device__ __forceinline__ void wave_run_add(uint32_t* ctr, int key)
{
    const int lane = threadIdx.x & 63;
    const int prev = __builtin_amdgcn_update_dpp(-2, key, 0x138, 0xF, 0xF, false);   // wave_shr:1, lane 0 <- -2
    const unsigned long long heads = __ballot(key != prev);
    if (key >= 0 && key != prev) {
        const unsigned long long later = lane == 63 ? 0ull : heads >> (lane + 1);
        const int len = later ? (int)__builtin_ctzll(later) + 1 : 64 - lane;
        atomicAdd(&ctr[key], (uint32_t)len);
    }
}

#ifndef ORBX_QT0_WPE
#define ORBX_QT0_WPE 4
#endif
#ifndef ORBX_QT1_WPE
#define ORBX_QT1_WPE 4
#endif
#ifndef ORBX_QT2_WPE
#define ORBX_QT2_WPE 6
#endif
// Minimum waves per SIMD (HIP's second __launch_bounds__ argument), i.e. a VGPR budget per template:
//   <512,16> (level 0) 4: 128 VGPRs (7 dwords spilled) instead of the compiler's 172, so two workgroups
//            share a CU and a 384-frame launch runs every frame at once: 106 -> 68 us;
//   <512,8>  (level 1) 5: 96 VGPRs (5 spilled) instead of 128: 43.8 -> 42.5 us;
//   <256,4>  (levels 2-7) 6: 80 VGPRs (3 spilled) instead of 100: 88 -> 70 us.
// Smaller workgroups also find room beside describe's sooner under the pipeline (+1.5% frames/s together).
// Round 3: levels 1 and 2-7 at 128 / 96 VGPRs (4 / 5 waves per SIMD, no spill): their occupancy is set by
// LDS and workgroup waves anyway (2 and 5 workgroups per CU), quadtree 0.165 -> 0.164 ms.
// FAST at 5 (94 VGPRs, no spill) measured slower (485 -> 495 us) and keeps the compiler's choice.
// Round 5: <256,4> at 6 (80 VGPRs, 5 dwords spilled) once its LDS fits six workgroups per CU (the retain
// step's keys over the node rectangles, the scan array at 2 lcap + 3 entries instead of 4 lcap + 1, the rank
// sort's keys at lcap + 4 instead of the next power of two: 28.7 -> 23.0 KB at KITTI): 135 -> 120 us per
// 1,024 frames; at 7 (72 VGPRs, 12 dwords spilled) 123 us.  With the dynamic LDS at a constant base (dyn_lds)
// none of the three spills at these budgets; <256,4> at 7 then spills 5 dwords (112 against 117 us, the
// pipelined rate unchanged).
#define ORBX_QT_WPE(NT, KPT, G) ((G) ? 1                                          \
                                 : ((NT) == 512 && (KPT) == 16) ? ORBX_QT0_WPE  \
                                 : ((NT) == 512 && (KPT) == 8) ? ORBX_QT1_WPE   \
                                 : ((NT) == 256) ? ORBX_QT2_WPE : 1)
//
// The node-list form of DistributeOctTree, one workgroup per (frame, level).
// kG: the node arrays live in the level's global region (LevelGeom::qtg_off) instead of LDS, with 32-bit
// node indices, for budgets whose node list outgrows a workgroup's LDS (e.g. Tracking's
// 2 * nFeatures initialisation extractor, src/Tracking.cc:133, at 4000 features).  The algorithm and its
// order of operations are the same; only the wave totals and the shared scalars stay in LDS.
// kWide: images wider or taller than 4096 px, whose packed keypoints split x / y at Geometry::kp_xbits; the
// standard form keeps the 12-bit split as a constant (a runtime split costs <256,4> a spilled register)
template <int QT_NT, int QT_KPT, bool kG, bool kWide>
__device__ __forceinline__ void qt_nodes(const int l, const int f, const Geometry* __restrict__ G,
                                         const Cell* __restrict__ cells, const uint32_t* __restrict__ slots,
                                         const int* __restrict__ cell_counts,
                                         uint32_t* __restrict__ spill,
                                         uint32_t* __restrict__ spill_node, uint8_t* __restrict__ gnodes,
                                         uint32_t* __restrict__ qt_out, int* __restrict__ qt_cnt,
                                         int* __restrict__ frame_counts, int* __restrict__ status, int lcap,
                                         int cellcap)
{
    // node index type; kNoneI marks "no node" (and compares above every valid rank)
    using Ix = typename std::conditional<kG, uint32_t, uint16_t>::type;
    constexpr Ix kNoneI = (Ix)~(Ix)0;
    constexpr uint32_t kPosMask = kG ? 0xFFFFFFFFu : 0xFFFFu;   // node position bits of a keypoint's node word
    uint8_t* const smem = dyn_lds();   // the dynamic LDS (no static LDS in this kernel)
    const int tid = threadIdx.x;
#ifdef ORBX_QT_PROF
    const long long qt_t0 = clock64();
    unsigned long long qt_acc[16] = {};
#endif
    const LevelGeom& LG = G->lv[l];
    const uint32_t xb = kWide ? (uint32_t)__builtin_amdgcn_readfirstlane(G->kp_xbits) : 12u;   // packed keypoint x width
    // lcap / cellcap: node-list and cell capacity of this launch's levels (qt_launch)
    constexpr bool kKpL = qt_kpn(QT_NT, QT_KPT, kG) > 0;
    const QtLayout Ly = qt_layout(lcap, cellcap, (int)sizeof(Ix), qt_kpn(QT_NT, QT_KPT, kG));
    uint32_t* kpa = (uint32_t*)(smem + Ly.kpa);
    uint8_t* nb = smem;
    if constexpr (kG) nb = gnodes + (size_t)f * G->qtg_per_frame + LG.qtg_off;
    uint32_t* scan = (uint32_t*)(nb + Ly.scan);
    int16_t* rect = (int16_t*)(nb + Ly.rect);
    uint32_t* cntb = (uint32_t*)(nb + Ly.cnt);
    Ix* srank = (Ix*)(nb + Ly.srank);
    Ix* npos = (Ix*)(nb + Ly.npos);
    Ix* snode = (Ix*)(nb + Ly.snode);
    uint32_t* sinfo = (uint32_t*)(nb + Ly.sinfo);   // per list position: split candidate flag | midlines
    uint32_t* ccnt = (uint32_t*)(nb + Ly.ccnt);
    Ix* cpos = (Ix*)(nb + Ly.cpos);
    Ix* vprev = (Ix*)(nb + Ly.vprev);
    Ix* vnew = (Ix*)(nb + Ly.vnew);
    uint32_t* skey = (uint32_t*)(nb + Ly.skey);
    uint32_t* escan = (uint32_t*)(nb + Ly.escan);   // kG only
    unsigned long long* best = (unsigned long long*)(nb + Ly.best);
    uint32_t* wsum = (uint32_t*)(smem + (kG ? kQtGlobWsum : Ly.wsum));
    int* sh = (int*)(smem + (kG ? kQtGlobSh : Ly.sh));
    // rect buffers: [buf][coord][lcap], coord 0..3 = x0, x1, y0, y1
    auto R = [&](int buf, int coord) { return rect + (size_t)(buf * 4 + coord) * lcap; };

    // ---- 1. gather this level's FAST candidates in reference order ----------
    const int ncl = LG.ncells, cb = LG.cell_begin;
    const uint32_t* fslots = slots + (size_t)f * G->slots_per_frame;
    // LDS node arrays (rect .. wsum) are free until the candidates are in registers: the cells' slot bases
    // load there beside the counts (both in flight together), and after the scan a per-candidate owner
    // map (u16 cell index) lets every candidate's slot load go out at once, with no per-candidate binary
    // search and no dependent cell-table load.
    uint32_t* gbase = (uint32_t*)(nb + Ly.rect);
    uint16_t* owner = (uint16_t*)(gbase + ncl);
    const size_t gregion = kG ? 0 : Ly.wsum - Ly.rect;
    const bool gb_ok = !kG && ncl <= 65536 && (size_t)4 * ncl <= gregion;   // block-uniform
    const int cpw = fast_cells_per_wave(gridDim.y);   // gridDim.y = the batch FAST ran on
    for (int c = tid; c < ncl; c += QT_NT) {
        const uint32_t raw = (uint32_t)cell_counts[(size_t)f * G->ncells + cb + c];
        scan[c] = raw & ~kCellDirect;
        if (gb_ok) gbase[c] = cell_slot_word(cells, cb, c, raw, cpw);
    }
    __syncthreads();
    const int n = (int)block_scan_excl<QT_NT>(scan, ncl, wsum);
    // the slot of cell c's first candidate without the per-cell table (the search and staged forms)
    auto caddr = [&](int c) -> uint32_t {
        const uint32_t raw = (uint32_t)cell_counts[(size_t)f * G->ncells + cb + c];
        return cell_slot_fix(cell_slot_word(cells, cb, c, raw, cpw), scan, c, cpw);
    };
#ifdef ORBX_QT_PROF
    long long qt_g = qt_t0;
    QT_STAMP(4, qt_g);
#endif
    const bool omap = gb_ok && (size_t)4 * ncl + 2 * (size_t)n <= gregion;
    if (omap) {
        for (int c = tid; c < ncl; c += QT_NT) {
            const int base = (int)scan[c], cnt = (c + 1 < ncl ? (int)scan[c + 1] : n) - base;
            gbase[c] = cell_slot_fix(gbase[c], scan, c, cpw);
            for (int j = 0; j < cnt; ++j) owner[base + j] = (uint16_t)c;
        }
        __syncthreads();
    }
#ifdef ORBX_QT_PROF
    QT_STAMP(14, qt_g);
#endif
    uint32_t* fspill = spill + (size_t)f * G->spill_per_frame + (LG.slot_begin > 0 ? 0 : 0);
    uint32_t* fspill_node = spill_node + (size_t)f * G->spill_per_frame;
    // spill region of this level: levels share the frame's spill array in level order
    {
        int off = 0;
        for (int q = 0; q < l; ++q) {
            const int extra = G->lv[q].slot_cap - qt_regcap(*G, q);
            off += extra > 0 ? extra : 0;
        }
        fspill += off;
        fspill_node += off;
    }
    auto fetch = [&](int i) -> uint32_t {
        if (omap) {
            const int c = owner[i];
            return fslots[gbase[c] + (uint32_t)(i - (int)scan[c])];
        }
        int lo = 0, hi = ncl - 1;   // last cell with scan[c] <= i
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if ((int)scan[mid] <= i) lo = mid; else hi = mid - 1;
        }
        return fslots[caddr(lo) + (i - (int)scan[lo])];
    };
    uint32_t kp[kKpL ? 1 : QT_KPT], nd[QT_KPT];
    // register slot r's keypoint (candidate tid + r * QT_NT)
    auto kpr = [&](int r) -> uint32_t {
        if constexpr (kKpL) return kpa[tid + r * QT_NT];
        else return kp[r];
    };
    // kG: the level's global region is sized to stage every candidate slot (qt_prepare); every thread
    // copies whole cells into it (a cell's candidates are contiguous in its slots) and then reads its own
    // indices
    uint32_t* stage = (uint32_t*)(nb + Ly.rect);
    const bool staged = kG && (long long)n * 4 <= LG.qtg_bytes - (long long)Ly.rect;   // block-uniform
    if (staged) {
        for (int c = tid; c < ncl; c += QT_NT) {
            const int base = (int)scan[c], cnt = (c + 1 < ncl ? (int)scan[c + 1] : n) - base;
            const uint32_t* src = fslots + caddr(c);
            // 8 loads in flight per batch instead of one dependent HBM round trip per candidate
            for (int j0 = 0; j0 < cnt; j0 += 8) {
                uint32_t v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = j0 + u < cnt ? src[j0 + u] : 0u;
#pragma unroll
                for (int u = 0; u < 8; ++u)
                    if (j0 + u < cnt) stage[base + j0 + u] = v[u];
            }
        }
        __syncthreads();
    }
    // register slot r of thread t is candidate t + r * QT_NT (a wave's lanes hold consecutive candidates:
    // coalesced loads, conflict-free LDS slots, runs of equal nodes for wave_run_add).  The owner-map and
    // staged forms are branch-free (indices clamped, the loads of every slot in flight together); the
    // search form branches.
    if (n > 0 && (omap || staged)) {   // block-uniform
        // every slot's load in flight before the first LDS store: an LDS store waiting for its global load
        // holds the LDS reads queued behind it (the next slot's owner lookups), which serialised the slots'
        // HBM round trips (level 0: 17.9k of the workgroup's 130k cycles)
        uint32_t v[QT_KPT];
#pragma unroll
        for (int r = 0; r < QT_KPT; ++r) {
            const int ii = min(tid + r * QT_NT, n - 1);
            if (omap) {
                const int c = owner[ii];
                v[r] = fslots[gbase[c] + (uint32_t)(ii - (int)scan[c])];
            } else {
                v[r] = stage[ii];
            }
        }
#pragma unroll
        for (int r = 0; r < QT_KPT; ++r) {
            const int i = tid + r * QT_NT;
            if constexpr (kKpL) kpa[i] = i < n ? v[r] : 0u;
            else kp[r] = i < n ? v[r] : 0u;
            nd[r] = 0;
        }
    } else {
#pragma unroll
        for (int r = 0; r < QT_KPT; ++r) {
            const int i = tid + r * QT_NT;
            if constexpr (kKpL) kpa[i] = i < n ? fetch(i) : 0u;
            else kp[r] = i < n ? fetch(i) : 0u;
            nd[r] = 0;
        }
    }
    for (int i = QT_NT * QT_KPT + tid; i < n; i += QT_NT) fspill[i - QT_NT * QT_KPT] = staged ? stage[i] : fetch(i);
#ifdef ORBX_QT_PROF
    QT_STAMP(15, qt_g);
#endif
    __syncthreads();   // the staging area becomes the node arrays
#ifdef ORBX_QT_PROF
    QT_STAMP(13, qt_g);
#endif

    // visit every keypoint (register part unrolled, spill part in a loop)
    auto visit = [&](auto&& fn) {
#pragma unroll
        for (int r = 0; r < QT_KPT; ++r) {
            const int i = tid + r * QT_NT;
            if (i < n) {
                uint32_t k = kpr(r);
                fn(k, nd[r], i);
            }
        }
        for (int i = QT_NT * QT_KPT + tid; i < n; i += QT_NT) {
            uint32_t k = fspill[i - QT_NT * QT_KPT];
            uint32_t d = fspill_node[i - QT_NT * QT_KPT];
            fn(k, d, i);
            fspill_node[i - QT_NT * QT_KPT] = d;
        }
    };

#ifdef ORBX_QT_PROF
    __syncthreads();
    long long qt_t = qt_t0;
    QT_STAMP(0, qt_t);
#endif
    // ---- 2. initial nodes, src/ORBextractor.cc:650-699 ------------------------
    const int nIni = LG.nIni;
    const float hX = LG.hX;
    const int N = LG.nfeat;
    for (int i = tid; i < nIni; i += QT_NT) ccnt[i] = 0;
    __syncthreads();
    auto root_of = [&](uint32_t k) {
        int r = (int)((float)(int)kp_x(k, xb) / hX);
        return r >= nIni ? nIni - 1 : r;
    };
    const int wave_i0 = tid - (tid & 63);   // this wave's first candidate index in register slot 0
#pragma unroll
    for (int r = 0; r < QT_KPT; ++r) {
        if (wave_i0 + r * QT_NT >= n) break;   // wave-uniform
        const int i = tid + r * QT_NT;
        int key = -1;
        if (i < n) {
            key = root_of(kpr(r));
            nd[r] = (uint32_t)key;
        }
        wave_run_add(ccnt, key);
    }
    for (int i = QT_NT * QT_KPT + tid; i < n; i += QT_NT) {   // spilled candidates
        const int key = root_of(fspill[i - QT_NT * QT_KPT]);
        fspill_node[i - QT_NT * QT_KPT] = (uint32_t)key;
        atomicAdd(&ccnt[key], 1u);
    }
    __syncthreads();
    if (tid == 0) {
        int L = 0;
        for (int i = 0; i < nIni; ++i) {
            npos[i] = kNoneI;
            if (ccnt[i] > 0) {
                if (L < lcap) {
                    R(0, 0)[L] = (int16_t)(int)(hX * (float)i);
                    R(0, 1)[L] = (int16_t)(int)(hX * (float)(i + 1));
                    R(0, 2)[L] = 0;
                    R(0, 3)[L] = (int16_t)LG.qh;
                    cntb[L] = ccnt[i];
                }
                npos[i] = (Ix)L;
                ++L;
            }
        }
        sh[SH_N] = n;
        sh[SH_L] = L;
        sh[SH_PHASE] = 1;
        sh[SH_DONE] = 0;
        sh[SH_BIG] = 0;
        sh[SH_ERR] = L > lcap ? kStatusListOverflow : 0;
        if (L > lcap) sh[SH_DONE] = 1;
    }
    __syncthreads();
    visit([&](uint32_t&, uint32_t& d, int) { d = npos[d]; });

    int cur = 0;
#ifdef ORBX_QT_PROF
    __syncthreads();
    QT_STAMP(1, qt_t);
    const long long qt_r0 = qt_t;
#endif
    // A round is five barrier-separated steps (phase 1: 8 barriers, was 15):
    //   A  split set: phase 1 every node with more than one key, ranked in list order (a scan);
    //      phase 2 vPrev ranked by (size, creation) descending.  The ranking thread also writes the
    //      node's midlines (ExtractorNode::DivideNode, :572-573) and clears its four child counters.
    //   B  count pass: every keypoint's child slot (4 * split rank + quadrant) and the child counts.
    //   C  one scan of (children, expandable children) per split node, packed in 16-bit halves;
    //      phase 2 then finds how many candidates are split (kk) and the non-split ranks.
    //   D  the new list: children of split rank s at Ctot - prefix(s) - children(s) (later splits in
    //      front, n4..n1), the rest after them in order; expandable children in creation order.
    //   E  relabel every keypoint with its new list position.
    // The scans evaluate their terms from LDS already in place (block_scan_fn), so no barrier precedes them.
    uint32_t* scan2 = scan + lcap + 1;   // phase 2's non-split flags (scan[0..S] holds step C's prefixes)
    while (true) {
        __syncthreads();
        if (sh[SH_DONE]) break;
#ifdef ORBX_QT_PROF
        if (sh[SH_PHASE] == 1) qt_acc[6] += 1;
        else qt_acc[7] += 1;
#endif
        const int L = sh[SH_L];
        const int phase = sh[SH_PHASE];
        uint32_t* cntc = cntb + (size_t)cur * lcap;
        uint32_t* cntn = cntb + (size_t)(cur ^ 1) * lcap;
        int16_t *cx0 = R(cur, 0), *cx1 = R(cur, 1), *cy0 = R(cur, 2), *cy1 = R(cur, 3);
        int16_t *nx0 = R(cur ^ 1, 0), *nx1 = R(cur ^ 1, 1), *ny0 = R(cur ^ 1, 2), *ny1 = R(cur ^ 1, 3);
        const Ix* vin = cur ? vnew : vprev;   // this round's vPrev (the previous round's expandable children)
        Ix* vout = cur ? vprev : vnew;
        auto set_split = [&](int s, int p) {
            srank[p] = (Ix)s;
            snode[s] = (Ix)p;
            const int hx = (int)ceilf((float)(cx1[p] - cx0[p]) / 2);
            const int hy = (int)ceilf((float)(cy1[p] - cy0[p]) / 2);
            sinfo[p] = 0x80000000u | (uint32_t)(cx0[p] + hx) | ((uint32_t)(cy0[p] + hy) << xb);
            ccnt[4 * p] = ccnt[4 * p + 1] = ccnt[4 * p + 2] = ccnt[4 * p + 3] = 0;
        };

        // ---- A ----
        int S;   // number of candidate (split) nodes this round
        if (phase == 1) {
            S = (int)block_scan_fn<QT_NT>(scan, L, wsum, [&](int p) { return cntc[p] > 1 ? 1u : 0u; });
            for (int p = tid; p < L; p += QT_NT) {
                const int sp = (int)scan[p];
                if (cntc[p] > 1) {
                    set_split(sp, p);
                } else {
                    srank[p] = kNoneI;
                    sinfo[p] = 0u;
                }
                npos[p] = (Ix)(p - sp);   // rank among non-split nodes
            }
        } else {
            // phase 2: sort vPrev by (size, creation) descending and split from the front.  The keys
            // are unique (creation index in the low bits), so an element's place is the number of
            // larger keys: every thread ranks its elements against the whole key array by broadcast
            // 16-byte reads, with one barrier in place of a bitonic network's log2(m)^2 / 2 stages.
            const int m = sh[SH_M];
            const int m4 = (m + 3) >> 2;
            for (int k = tid; k < 4 * m4; k += QT_NT) {
                uint32_t key = 0u;   // 0: below every key
                if (k < m) {
                    const uint32_t c = cntc[vin[k]];
                    key = (c << 16) | (uint32_t)k;
                    if (c > 0xFFFFu) sh[SH_BIG] = 1;   // the packed key would wrap (reset at the round's end)
                }
                skey[k] = key;
            }
            for (int p = tid; p < L; p += QT_NT) {
                srank[p] = kNoneI;
                sinfo[p] = 0u;
            }
            __syncthreads();
            if (sh[SH_BIG] == 0 && m <= 0x10000) {   // block-uniform
                const uint4* k4 = (const uint4*)skey;
                for (int k = tid; k < m; k += QT_NT) {
                    const uint32_t key = skey[k];
                    int j = 0;
                    for (int i4 = 0; i4 < m4; ++i4) {
                        const uint4 v = k4[i4];
                        j += (int)(v.x > key) + (int)(v.y > key) + (int)(v.z > key) + (int)(v.w > key);
                    }
                    set_split(j, (int)vin[k]);
                }
            } else {
                // a node of more than 0xFFFF keys (huge levels with small budgets) or more than 2^16
                // candidates: the same order, compared as (size, creation) pairs
                for (int k = tid; k < m; k += QT_NT) {
                    const uint32_t c = cntc[vin[k]];
                    int j = 0;
                    for (int k2 = 0; k2 < m; ++k2) {
                        const uint32_t c2 = cntc[vin[k2]];
                        j += (int)(c2 > c || (c2 == c && k2 > k));
                    }
                    set_split(j, (int)vin[k]);
                }
            }
            S = m;
        }
        __syncthreads();
        QT_STAMP(3, qt_t);

        // ---- B: a keypoint's child slot is 4 * (its node's list position) + quadrant; the candidate flag
        // and quadrant are kept in its node word beside the position for the relabel (bit 18, bits 16-17).
        // kG: node words hold the full position, and the relabel recomputes the child slot (sinfo is
        // unchanged until then).
        auto child_key = [&](uint32_t k, uint32_t d) {
            const uint32_t p = d & kPosMask;
            const uint32_t w = sinfo[p];
            if (!(w & 0x80000000u)) return -1;
            return (int)(4 * p + (kp_x(k, xb) >= kp_x(w, xb) ? 1u : 0u) + (kp_y(k, xb) >= kp_y(w, xb) ? 2u : 0u));
        };
        if constexpr (!kG) {
            // keys first, branch-free (every slot's node and keypoint LDS reads in flight together; a slot
            // past n has node 0, a valid index, and is masked), then the counts: interleaved, each slot's
            // loads would wait behind the previous slot's atomics
            uint32_t wv[QT_KPT], kv[QT_KPT];
#pragma unroll
            for (int r = 0; r < QT_KPT; ++r) wv[r] = sinfo[nd[r] & 0xFFFFu];
#pragma unroll
            for (int r = 0; r < QT_KPT; ++r) kv[r] = kpr(r);
#pragma unroll
            for (int r = 0; r < QT_KPT; ++r) {
                const int i = tid + r * QT_NT;
                const uint32_t w = wv[r], k = kv[r];
                const bool cand = i < n && (w & 0x80000000u);
                const uint32_t qd = (kp_x(k, xb) >= kp_x(w, xb) ? 1u : 0u) + (kp_y(k, xb) >= kp_y(w, xb) ? 2u : 0u);
                nd[r] = (nd[r] & 0xFFFFu) | (cand ? 0x40000u | (qd << 16) : 0u);
            }
#pragma unroll
            for (int r = 0; r < QT_KPT; ++r) {
                if (wave_i0 + r * QT_NT >= n) break;   // wave-uniform
                wave_run_add(ccnt, (nd[r] & 0x40000u) ? (int)(4 * (nd[r] & 0xFFFFu) + ((nd[r] >> 16) & 3u)) : -1);
            }
        } else {
#pragma unroll
            for (int r = 0; r < QT_KPT; ++r) {
                if (wave_i0 + r * QT_NT >= n) break;   // wave-uniform
                const int i = tid + r * QT_NT;
                wave_run_add(ccnt, i < n ? child_key(kpr(r), nd[r]) : -1);
            }
        }
        for (int i = QT_NT * QT_KPT + tid; i < n; i += QT_NT) {
            uint32_t& d = fspill_node[i - QT_NT * QT_KPT];
            const int key = child_key(fspill[i - QT_NT * QT_KPT], d);
            if constexpr (!kG) d = (d & 0xFFFFu) | (key >= 0 ? 0x40000u | ((uint32_t)(key & 3) << 16) : 0u);
            if (key >= 0) atomicAdd(&ccnt[key], 1u);
        }
        if (tid == 0) sh[SH_KK] = S;   // phase 2: lowered in step C by the split that reaches N
        __syncthreads();
        QT_STAMP(9, qt_t);

        // ---- C: children (low half) and expandable children (high half) per split rank; kG scans the halves
        // apart (scan, escan): its lists are not bounded by kQtLdsMaxList, and a packed prefix would wrap ----
        auto kids = [&](int s) -> uint32_t {
            const int p = snode[s];
            uint32_t v = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint32_t c = ccnt[4 * p + q];
                v += (c > 0 ? 1u : 0u) + (c > 1 ? 0x10000u : 0u);
            }
            return v;
        };
        uint32_t preC, preE;   // prefixes at kk: children, expandable children
        if constexpr (kG) {
            preC = block_scan_fn<QT_NT>(scan, S, wsum, [&](int s) { return kids(s) & 0xFFFFu; });
            preE = block_scan_fn<QT_NT>(escan, S, wsum, [&](int s) { return kids(s) >> 16; });
        } else {
            const uint32_t T = block_scan_fn<QT_NT>(scan, S, wsum, kids);
            preC = T & 0xFFFFu;
            preE = T >> 16;
        }
        auto pre_c = [&](int s) -> uint32_t { return kG ? scan[s] : scan[s] & 0xFFFFu; };
        auto pre_e = [&](int s) -> uint32_t { return kG ? escan[s] : scan[s] >> 16; };
        int kk = S;
        if (phase == 2) {
            // how many candidates are actually split: the size after splitting j grows with j (a split
            // node leaves >= 1 child), so the one j that crosses N writes
            for (int j = tid; j < S; j += QT_NT) {
                const int cs = (int)(kids(j) & 0xFFFFu), sj = (int)pre_c(j);
                if (L + sj + cs - (j + 1) >= N && L + sj - j < N) sh[SH_KK] = j + 1;
            }
            __syncthreads();
            kk = sh[SH_KK];
            if (kk < S) {
                preC = pre_c(kk);
                preE = pre_e(kk);
            }
            block_scan_fn<QT_NT>(scan2, L, wsum, [&](int p) {
                return (srank[p] != kNoneI && (int)srank[p] < kk) ? 1u : 0u;
            });
        }
        QT_STAMP(10, qt_t);
        const int Ctot = (int)preC, nexp = (int)preE;
        const int newL = Ctot + (L - kk);
        if (newL > lcap) {
            if (tid == 0) {
                sh[SH_ERR] |= kStatusListOverflow;
                sh[SH_DONE] = 1;
            }
            continue;
        }

        // ---- D ----
        for (int s = tid; s < kk; s += QT_NT) {
            const int p = snode[s];
            uint32_t c4[4];
            int cs = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                c4[q] = ccnt[4 * p + q];
                cs += c4[q] > 0;
            }
            const int pos0 = Ctot - (int)pre_c(s) - cs;   // later splits are pushed in front
            int e = (int)pre_e(s);
            const uint32_t w = sinfo[p];
            const int mx = (int)kp_x(w, xb), my = (int)kp_y(w, xb);
            const int x0 = cx0[p], x1 = cx1[p], y0 = cy0[p], y1 = cy1[p];
            int np = pos0 + cs;   // n1 lands last (it was pushed first)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint32_t c = c4[q];
                if (c == 0) continue;   // (no keypoint looks its slot up)
                --np;
                cpos[4 * p + q] = (Ix)np;
                nx0[np] = (int16_t)((q & 1) ? mx : x0);
                nx1[np] = (int16_t)((q & 1) ? x1 : mx);
                ny0[np] = (int16_t)((q & 2) ? my : y0);
                ny1[np] = (int16_t)((q & 2) ? y1 : my);
                cntn[np] = c;
                if (c > 1) vout[e++] = (Ix)np;   // creation order: split rank, then n1..n4
            }
        }
        for (int p = tid; p < L; p += QT_NT) {
            const bool split = srank[p] != kNoneI && (int)srank[p] < kk;
            if (!split) {
                const int np = Ctot + (phase == 1 ? (int)npos[p] : p - (int)scan2[p]);
                npos[p] = (Ix)np;
                nx0[np] = cx0[p];
                nx1[np] = cx1[p];
                ny0[np] = cy0[p];
                ny1[np] = cy1[p];
                cntn[np] = cntc[p];
                // a phase-2 candidate past kk keeps its keypoints: its child slots all lead to its new place
                if (srank[p] != kNoneI) cpos[4 * p] = cpos[4 * p + 1] = cpos[4 * p + 2] = cpos[4 * p + 3] = (Ix)np;
            }
        }
        if (tid == 0) {
            // src/ORBextractor.cc:793-803 and :871-872 (read at the next round's start)
            sh[SH_L] = newL;
            if (newL >= N || newL == L) {
                sh[SH_DONE] = 1;
            } else if (phase == 1) {
                if (newL + 3 * nexp > N) sh[SH_PHASE] = 2;
            }
            sh[SH_M] = nexp;
            sh[SH_BIG] = 0;
        }
        __syncthreads();
        QT_STAMP(11, qt_t);

        // ---- E: relabel keypoints with their new list position ----
        if constexpr (!kG) {
            // register slots branch-free: one LDS read per slot from the child or the node table, every
            // slot's read in flight together; slots past n keep node 0
            uint32_t v[QT_KPT];
#pragma unroll
            for (int r = 0; r < QT_KPT; ++r) {
                const uint32_t d = nd[r];
                const Ix* src = (d & 0x40000u) ? cpos + (4 * (d & 0xFFFFu) + ((d >> 16) & 3u)) : npos + (d & 0xFFFFu);
                v[r] = (uint32_t)*src;
            }
#pragma unroll
            for (int r = 0; r < QT_KPT; ++r) nd[r] = tid + r * QT_NT < n ? v[r] : 0u;
            for (int i = QT_NT * QT_KPT + tid; i < n; i += QT_NT) {   // spilled keypoints
                uint32_t& d = fspill_node[i - QT_NT * QT_KPT];
                const int ck = (d & 0x40000u) ? (int)(4 * (d & 0xFFFFu) + ((d >> 16) & 3u)) : -1;
                d = ck >= 0 ? (uint32_t)cpos[ck] : (uint32_t)npos[d & kPosMask];
            }
        } else {
            visit([&](uint32_t& k, uint32_t& d, int) {
                // child slot from the count pass, -1 if the node was not a candidate
                const int ck = child_key(k, d);
                d = ck >= 0 ? (uint32_t)cpos[ck] : (uint32_t)npos[d & kPosMask];
            });
        }
        QT_STAMP(12, qt_t);
        cur ^= 1;
    }

#ifdef ORBX_QT_PROF
    // (the round loop's time: stamped at each round's end below would need the phase; charge the
    // whole loop to slot 2 and let the caller split it with the sort and round counts)
    qt_acc[2] += (unsigned long long)(clock64() - qt_r0);
    qt_t = clock64();
#endif
    // ---- 4. retain the best keypoint per node (first max wins), :882-906 -----
    const int L = sh[SH_L];
    const bool ok = sh[SH_ERR] == 0;
    for (int p = tid; p < L && ok; p += QT_NT) best[p] = 0ull;
    __syncthreads();
    if (ok) {
        visit([&](uint32_t& k, uint32_t& d, int i) {
            const unsigned long long key = ((unsigned long long)(k >> 24) << 56) |
                                           ((unsigned long long)(0xFFFFFFu - (uint32_t)i) << 32) |
                                           (unsigned long long)(k & 0xFFFFFFu);
            atomicMax(&best[d], key);
        });
    }
    __syncthreads();
    const int outn = ok ? (L < LG.cap ? L : LG.cap) : 0;
    uint32_t* out = qt_out + (size_t)f * G->out_per_frame + LG.out_off;
    for (int p = tid; p < outn; p += QT_NT) {
        const unsigned long long key = best[p];
        const uint32_t x = kp_x((uint32_t)key, xb) + kMinBorder;
        const uint32_t y = kp_y((uint32_t)key, xb) + kMinBorder;
        out[p] = pack_kp(x, y, (uint32_t)(key >> 56), xb);
    }
    if (tid == 0) {
        qt_cnt[(size_t)f * G->nlevels + l] = outn;
#ifdef ORBX_QT_PROF
        QT_STAMP(5, qt_t);
        qt_acc[8] = 1;
        for (int k = 0; k < 16; ++k) atomicAdd(&g_qt_prof[l][k], qt_acc[k]);
#endif
        atomicAdd(&frame_counts[f], outn);
        int err = sh[SH_ERR];
        if (ok && L > LG.cap) err |= kStatusOutOverflow;
        if (err) atomicOr(status, err);
    }
}

template <int QT_NT, int QT_KPT, bool kG, bool kWide>
__global__ __launch_bounds__(QT_NT, ORBX_QT_WPE(QT_NT, QT_KPT, kG)) void k_quadtree(
    int level0, const Geometry* __restrict__ G, const Cell* __restrict__ cells, const uint32_t* __restrict__ slots,
    const int* __restrict__ cell_counts, uint32_t* __restrict__ spill,
    uint32_t* __restrict__ spill_node, uint8_t* __restrict__ gnodes, uint32_t* __restrict__ qt_out,
    int* __restrict__ qt_cnt, int* __restrict__ frame_counts, int* __restrict__ status, int lcap, int cellcap)
{
    qt_nodes<QT_NT, QT_KPT, kG, kWide>(level0 + blockIdx.x, blockIdx.y, G, cells, slots, cell_counts, spill,
                                spill_node, gnodes, qt_out, qt_cnt, frame_counts, status, lcap, cellcap);
}

template <int NT, int KPT, bool kG>
static void qt_launch(const Geometry& g, const ExtractBufs& b, int* frame_counts, const QtGroup& q, int batch,
                      hipStream_t s)
{
    const size_t smem = kG ? kQtGlobSmem : qt_layout(q.lcap, q.cellcap, 2, qt_kpn(NT, KPT, 0)).total;
    auto launch = [&](auto kern) {
        hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
        hipLaunchKernelGGL(kern, dim3(q.nl, batch), dim3(NT), smem, s, q.l0, b.geom, b.cells, b.slots, b.cell_counts,
                           b.spill, b.spill_node, b.qt_nodes, b.qt_out, b.qt_cnt, frame_counts, b.status, q.lcap,
                           q.cellcap);
    };
    if (g.kp_xbits == 12) launch(k_quadtree<NT, KPT, kG, false>);
    else launch(k_quadtree<NT, KPT, kG, true>);
}

// Launch groups.  A group's node capacity is the largest cap + 4 of its levels: a level's list never holds
// more than cap + 3 nodes (phase 1 stops before L + 3 * expandable exceeds N, phase 2 once L >= N;
// cap >= max(N + 2, 4 * nIni)), so the coarse levels' workgroups take less LDS than level 0's and more of
// them fit on a CU.
int qt_plan(const Geometry& g, int batch, QtGroup* out)
{
    auto caps = [&](QtGroup& q) {
        q.lcap = 8;
        q.cellcap = 1;
        for (int l = q.l0; l < q.l0 + q.nl; ++l) {
            q.lcap = std::max(q.lcap, g.lv[l].cap + 4);
            q.cellcap = std::max(q.cellcap, g.lv[l].ncells);
        }
    };
    bool anyg = false;
    for (int l = 0; l < g.nlevels; ++l) anyg |= g.lv[l].qt_glob != 0;
    // Small batches (the per-frame host path): one launch of the level-0 kernel over every level, so
    // the levels run concurrently instead of as dependent launches (latency, not throughput).
    // A level run with more register capacity than qt_regcap(g, l) spills less than its region holds.
    if (batch <= kQtMergedMaxBatch && !anyg) {
        QtGroup q{0, g.nlevels, 512, g.qt_kpt0, 0, 0, 0};
        caps(q);
        if (qt_layout(q.lcap, q.cellcap, 2, qt_kpn(q.nt, q.kpt, 0)).total <= kQtLdsMax) {
            out[0] = q;
            return 1;
        }
    }
    // one launch per run of consecutive levels with the same configuration; the launched template is
    // exactly qt_nt / qt_kpt, which size the spill regions
    int n = 0;
    for (int l0 = 0; l0 < g.nlevels;) {
        const int nt = qt_nt(g, l0), kpt = qt_kpt(g, l0), gl = g.lv[l0].qt_glob;
        int l1 = l0 + 1;
        while (l1 < g.nlevels && qt_nt(g, l1) == nt && qt_kpt(g, l1) == kpt && g.lv[l1].qt_glob == gl) ++l1;
        QtGroup q{l0, l1 - l0, nt, kpt, gl, 0, 0};
        caps(q);
        out[n++] = q;
        l0 = l1;
    }
    return n;
}

// What launch_quadtree runs for each level of a batch, read from the plan and the layout (orbx_debug_qt_plan).
// gather_room: the bytes the gather compares 4 * ncells + 2 * n against when it picks the owner map (gregion).
void qt_report(const Geometry& g, int batch, QtLevelPlan* out)
{
    QtGroup grp[kQtMaxGroups];
    const int ng = qt_plan(g, batch, grp);
    for (int i = 0; i < ng; ++i) {
        const QtGroup& q = grp[i];
        const int nt = q.glob ? kQtGlobNT : q.nt, kpt = q.glob ? kQtGlobKPT : q.kpt;
        const QtLayout Ly = qt_layout(q.lcap, q.cellcap, q.glob ? 4 : 2, qt_kpn(nt, kpt, q.glob));
        for (int l = q.l0; l < q.l0 + q.nl; ++l)
            out[l] = QtLevelPlan{nt, kpt, q.glob, g.kp_xbits != 12, q.lcap, q.cellcap,
                                 q.glob ? 0 : (int)(Ly.wsum - Ly.rect), i};
    }
}

bool qt_prepare(Geometry& g)
{
    // a level's own node list decides; a group whose shared capacity outgrows LDS moves to global too
    for (int l = 0; l < g.nlevels; ++l) {
        const int lc = g.lv[l].cap + 4;
        const int kpn = qt_kpn(l == 0 ? 512 : 256, l == 0 ? g.qt_kpt0 : 4, 0);
        g.lv[l].qt_glob = lc > kQtLdsMaxList || qt_layout(lc, g.lv[l].ncells, 2, kpn).total > kQtLdsMax;
        g.lv[l].qtg_off = g.lv[l].qtg_bytes = 0;
    }
    QtGroup grp[kQtMaxGroups];
    for (;;) {
        const int ng = qt_plan(g, 1 << 30, grp);
        bool moved = false;
        for (int i = 0; i < ng; ++i) {
            if (grp[i].glob || qt_layout(grp[i].lcap, grp[i].cellcap, 2, qt_kpn(grp[i].nt, grp[i].kpt, 0)).total <= kQtLdsMax)
                continue;
            for (int l = grp[i].l0; l < grp[i].l0 + grp[i].nl; ++l) g.lv[l].qt_glob = 1;
            moved = true;
        }
        if (moved) continue;
        // global regions: the group's node layout with 32-bit indices, or room to stage every candidate
        // slot of the level (the gather reads them in index order from there), whichever is larger
        long long off = 0;
        for (int i = 0; i < ng; ++i) {
            if (!grp[i].glob) continue;
            const QtLayout Ly = qt_layout(grp[i].lcap, grp[i].cellcap, 4);
            for (int l = grp[i].l0; l < grp[i].l0 + grp[i].nl; ++l) {
                long long bytes = std::max((long long)Ly.total, (long long)Ly.rect + 4LL * g.lv[l].slot_cap);
                bytes = (bytes + 255) & ~255LL;
                g.lv[l].qtg_off = off;
                g.lv[l].qtg_bytes = bytes;
                off += bytes;
            }
        }
        g.qtg_per_frame = off;
        return true;
    }
}

#ifdef ORBX_QT_PROF
}  // namespace orbx
extern "C" int orbx_debug_qt_prof(unsigned long long* out, int reset)
{
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(orbx::g_qt_prof), sizeof(orbx::g_qt_prof)) != hipSuccess) return -1;
    if (reset) {
        static unsigned long long zero[16][16];
        if (hipMemcpyToSymbol(HIP_SYMBOL(orbx::g_qt_prof), zero, sizeof(zero)) != hipSuccess) return -1;
    }
    return 0;
}
namespace orbx {
#endif

void launch_quadtree(const Geometry& g, const ExtractBufs& b, int* frame_counts, int batch, hipStream_t s)
{
    QtGroup grp[kQtMaxGroups];
    const int ng = qt_plan(g, batch, grp);
    for (int i = 0; i < ng; ++i) {
        const QtGroup& q = grp[i];
        if (q.glob) qt_launch<kQtGlobNT, kQtGlobKPT, true>(g, b, frame_counts, q, batch, s);
        else if (q.nt == 512 && q.kpt == 24) qt_launch<512, 24, false>(g, b, frame_counts, q, batch, s);
        else if (q.nt == 512 && q.kpt == 16) qt_launch<512, 16, false>(g, b, frame_counts, q, batch, s);
        else if (q.nt == 512) qt_launch<512, 8, false>(g, b, frame_counts, q, batch, s);
        else qt_launch<256, 4, false>(g, b, frame_counts, q, batch, s);
    }
}

}  // namespace orbx

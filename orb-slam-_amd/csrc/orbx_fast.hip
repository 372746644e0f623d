// gfx950 kernels of the ORB extractor (ORB_SLAM2::ORBextractor::operator(),
// src/ORBextractor.cc:1248-1334).  Integer/bitwise path: no MFMA.
//
//   K2 k_fast_cells     per-cell FAST-9 + NMS + threshold retry, :952-1000
#include <hip/hip_runtime.h>

#include <algorithm>

#include "orbx_device.hpp"
#include "orbx_kernels.hpp"

namespace orbx {

// ---------------------------------------------------------------------------
// K2: FAST-9/16 on one cell ROI per wave (cv::FAST(roi, kps, th, true)).
// s = max(A, -B) with A = max over 9-arcs of min(v - ring), B = min of max:
// a pixel is a corner at t iff s > t, and cornerScore = s - 1.
// NMS is evaluated inside the cell with scores masked by the cell threshold;
// the cell falls back to minThFAST iff NMS at iniThFAST keeps nothing
// (src/ORBextractor.cc:982-987).  Survivors are emitted row-major, i.e. in
// OpenCV's emission order.
// ---------------------------------------------------------------------------
// The ROI tile holds the pixel bytes x, one byte per pixel.  A byte read into the low half of a VGPR
// (ds_read_u8_d16) is the f16 bit pattern of the denormal x * 2^-24: denormals are exact fixed-point
// values (the kernels run with f16 denormals preserved, .amdhsa_float_denorm_mode_16_64 3), so f16
// max/min/sub/compare on them are exact integer operations, and a non-negative result's bit pattern is
// its integer value.  Each ring value enters the arithmetic as the packed pair (h, -h): the compiler
// folds that into the first packed instruction's source modifiers (op_sel_hi = 0, neg_hi), so it costs
// nothing, and packed f16 max/min/sub work on both polarities at once.  (Round 2 stored 0x6400 | x, the
// normal f16 1024 + x, 2 bytes per pixel: the byte tile halves the tile's LDS and its commit is one
// alignbyte and one 4-byte store per pass.)  gfx950's v_pk_maximum3_f16 / v_pk_minimum3_f16 take three
// operands: a 9-arc max of the pairs is the "brighter" arc value and, in the other half, minus the 9-arc
// min ("darker").
typedef _Float16 fh2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ fh2 as_fh2(uint32_t u) { return __builtin_bit_cast(fh2, u); }
__device__ __forceinline__ fh2 pmax2(fh2 a, fh2 b) { return __builtin_elementwise_maximum(a, b); }
__device__ __forceinline__ fh2 pmin2(fh2 a, fh2 b) { return __builtin_elementwise_minimum(a, b); }
__device__ __forceinline__ fh2 pmax3(fh2 a, fh2 b, fh2 c) { return pmax2(pmax2(a, b), c); }
__device__ __forceinline__ fh2 pmin3(fh2 a, fh2 b, fh2 c) { return pmin2(pmin2(a, b), c); }
// pixel byte as the f16 denormal x * 2^-24; an integer threshold likewise
__device__ __forceinline__ _Float16 px16(const uint8_t* p) { return __builtin_bit_cast(_Float16, (uint16_t)*p); }
__device__ __forceinline__ _Float16 int16_as_f16(int t) { return __builtin_bit_cast(_Float16, (uint16_t)t); }
__device__ __forceinline__ fh2 dup_neg(_Float16 h)
{
    fh2 r;
    r.x = h;
    r.y = -h;
    return r;
}

// Tile row pitch in dwords (pixels): a compile-time constant per kernel instantiation, so every ring
// and neighbour access is one base register plus an immediate LDS offset (no per-access address
// arithmetic).  40 covers the ROIs of every BASELINE configuration (37-38 px); 68 the 66-px cap.
__host__ __device__ constexpr int fast_tile_pitch(int max_roi_w) { return max_roi_w <= 40 ? 40 : 68; }
// per-wave LDS: ROI tile [rh][TP] bytes, zero-bordered strength map [rh - 4][TP] bytes (the
// detection window plus a one-pixel frame, at the tile's pitch so a map index is a tile index minus a
// constant), and the candidate list (u16 tile indices) of the largest window, filled from both ends
__host__ __device__ inline size_t fast_map_bytes(int rw, int rh)
{
    return ((size_t)(rh - 4) * fast_tile_pitch(rw) + 3) & ~(size_t)3;
}
__host__ __device__ inline int fast_list_cap(int rw, int rh) { return (rh - 6) * (rw - 6); }
// Output buffer (packed candidates) of the wave's cells, written to HBM once after its last cell: a global
// store inside the cell loop would make the next cell's wait for its prefetched ROI (vmcnt counts loads
// and stores, completed in issue order) wait for the store's round trip as well.
#ifndef ORBX_FAST_OBCAP
#define ORBX_FAST_OBCAP 128
#endif
constexpr int kFastObCap = ORBX_FAST_OBCAP;
constexpr int kFastScratch = 128;   // a u16 per lane after obuf (the masked-off lanes' list and map writes)
__host__ __device__ inline size_t fast_list_bytes(int rw, int rh) { return (2 * (size_t)fast_list_cap(rw, rh) + 3) & ~(size_t)3; }
__host__ __device__ inline size_t fast_wave_bytes(int rw, int rh)
{
    const size_t tile = (size_t)rh * fast_tile_pitch(rw);
    return (tile + fast_map_bytes(rw, rh) + fast_list_bytes(rw, rh) + 4 * kFastObCap + kFastScratch + 15) & ~(size_t)15;
}

// max(v - minMax, maxMin - v) over the 16 cyclic 9-arcs of the Bresenham ring of the
// pixel at tile byte c[0]
template <int TP>
__device__ __forceinline__ int fast_strength(const uint8_t* c)
{
    fh2 x[16];
    x[0] = dup_neg(px16(c + 3 * TP));
    x[1] = dup_neg(px16(c + 3 * TP + 1));
    x[2] = dup_neg(px16(c + 2 * TP + 2));
    x[3] = dup_neg(px16(c + TP + 3));
    x[4] = dup_neg(px16(c + 3));
    x[5] = dup_neg(px16(c - TP + 3));
    x[6] = dup_neg(px16(c - 2 * TP + 2));
    x[7] = dup_neg(px16(c - 3 * TP + 1));
    x[8] = dup_neg(px16(c - 3 * TP));
    x[9] = dup_neg(px16(c - 3 * TP - 1));
    x[10] = dup_neg(px16(c - 2 * TP - 2));
    x[11] = dup_neg(px16(c - TP - 3));
    x[12] = dup_neg(px16(c - 3));
    x[13] = dup_neg(px16(c + TP - 3));
    x[14] = dup_neg(px16(c + 2 * TP - 2));
    x[15] = dup_neg(px16(c + 3 * TP - 1));
    fh2 m3[16], a[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) m3[k] = pmax3(x[k], x[(k + 1) & 15], x[(k + 2) & 15]);
#pragma unroll
    for (int k = 0; k < 16; ++k) a[k] = pmax3(m3[k], m3[(k + 3) & 15], m3[(k + 6) & 15]);
    const fh2 b0 = pmin3(a[0], a[1], a[2]), b1 = pmin3(a[3], a[4], a[5]), b2 = pmin3(a[6], a[7], a[8]);
    const fh2 b3 = pmin3(a[9], a[10], a[11]), b4 = pmin3(a[12], a[13], a[14]);
    const fh2 mm = pmin3(pmin3(b0, b1, b2), pmin2(b3, b4), a[15]);   // (minMax, -maxMin)
    const fh2 d = dup_neg(px16(c)) - mm;   // (v - minMax, maxMin - v)
    // the integer value of a non-negative result; a negative one reads as a negative int16 (not a corner)
    return (int)__builtin_bit_cast(int16_t, __builtin_fmaxf16(d.x, d.y));
}

// Compass value q of the pixel at c[0]: a 9-arc holds two consecutive compass points (ring positions
// 0, 4, 8, 12), so s > t needs some consecutive pair brighter than v + t or darker than v - t, i.e.
// q = max(max pair-min - v, v - min pair-max) > t.  An integer-valued f16.  Over the 4-cycle
// (N, E, S, W) the largest pair minimum is min(max(N, S), max(E, W)): each consecutive pair holds one of
// {N, S} and one of {E, W}, and the larger of N, S forms a pair with each of E, W.  Three packed ops.
template <int TP>
__device__ __forceinline__ _Float16 fast_compass_q(const uint8_t* c)
{
    const fh2 a = dup_neg(px16(c + 3 * TP)), b = dup_neg(px16(c + 3)), d = dup_neg(px16(c - 3 * TP)),
              e = dup_neg(px16(c - 3));
    const fh2 m = pmin2(pmax2(a, d), pmax2(b, e));   // (br, -dk)
    const fh2 q = m - dup_neg(px16(c));              // (br - v, v - dk)
    return __builtin_fmaxf16(q.x, q.y);   // one v_max_f16 (SDWA high-half operand)
}

// strict 3x3 non-maximum suppression on the strength map at threshold t (m[0]: the pixel).  cv::FAST keeps
// a corner whose score s - 1 beats every neighbour's score, a neighbour that is no corner at t scoring 0:
//   s > t and, for each neighbour n, (n > t ? s > n : s > 1),
// and since s > t already beats every n <= t, that is s > max(t, 1, n_0 .. n_7): four max3, one compare.
// (t1 = max(t, 1), wave-uniform)
__device__ __forceinline__ uint32_t umax3(uint32_t a, uint32_t b, uint32_t c) { return __builtin_elementwise_max(__builtin_elementwise_max(a, b), c); }
template <int TP>
__device__ __forceinline__ bool nms_keep(const uint8_t* m, uint32_t t1)
{
    const uint32_t a = umax3(m[-TP - 1], m[-TP], m[-TP + 1]);
    const uint32_t b = umax3(m[-1], m[1], m[TP - 1]);
    const uint32_t c = umax3(m[TP], m[TP + 1], t1);
    return (uint32_t)m[0] > umax3(a, b, c);
}

// ROI bytes of one cell staged in registers, in passes of rpp whole rows: lane = rl * nd + kl loads
// dword kl of row u * rpp + rl (nd = dwords per ROI row) at its exact byte, so a pass costs one register.
// LD passes are prefetched (the launch's largest ROI: 8 for
// 38 x 39, 10 for 38 x 46 ROIs); bigger ROIs load their remainder synchronously.
// kCellsPerWave (orbx_geom.hpp) cells per wave: the next cell's ROI loads fly under this one's passes

template <int LD>
struct FastPrefetch {
    uint32_t w[LD];
};

struct FastCellSrc {
    const uint8_t* src;   // ROI origin
    int pitch, nd, rh;    // dwords per row ceil(roi_w / 4), rows
};

// The lane map of the tile pitch's widest row (TP / 4 dwords + the extra one): rows per pass and the
// lane's (row in pass, dword) are compile-time / per-kernel constants, so every pass's offsets are
// immediates; a narrower cell leaves its lanes past its own dwords idle.
// Each lane loads its dword at the exact (unaligned) ROI byte, which gfx950 serves exactly
// (tools/probes/glb_unaligned.hip), so the commit is a plain store: TP / 4 lanes per row.
__host__ __device__ constexpr int fast_lanes_per_row(int tp) { return tp / 4; }
template <int TP>
struct FastLaneMap {
    static constexpr int kND1 = fast_lanes_per_row(TP), kRPP = 64 / kND1;
    int rl, kl;
    __device__ explicit FastLaneMap(int lane) : rl(lane / kND1), kl(lane - (lane / kND1) * kND1) {}
};

template <int TP, int LD>
__device__ __forceinline__ void fast_issue(const FastCellSrc& S, const FastLaneMap<TP>& M, int u0, FastPrefetch<LD>& F)
{
    // branch-free: every lane loads, its row clamped to the ROI's last and its dword to the row's last (the
    // lanes past a row's dwords and past a pass's rows repeat a neighbour's load, which the commit stores to
    // the same place): no exec save / branch / restore per pass
    // (an empty cell -- the level padding's -- loads nothing: its clamps would go negative)
    if (S.rh <= 0 || S.nd <= 0) return;   // wave-uniform
    const __attribute__((address_space(1))) uint8_t* base = (const __attribute__((address_space(1))) uint8_t*)S.src;
    const uint32_t kb = 4u * (uint32_t)min(M.kl, S.nd - 1);
#pragma unroll
    for (int u = 0; u < LD; ++u) {
        const uint32_t row = (uint32_t)min((u0 + u) * FastLaneMap<TP>::kRPP + M.rl, S.rh - 1);
        F.w[u] = *(const __attribute__((address_space(1))) uint32_t*)(base + (__umul24(row, (uint32_t)S.pitch) + kb));
    }
}

// The first LD passes of a cell (u0 = 0) without per-pass address arithmetic or tests: every pass loads, from
// a scalar row offset plus the lane's fixed one, through a buffer descriptor whose size ends at the ROI's last
// byte, so the rows past the ROI read zeros (gfx950's range check covers soffset too,
// tools/probes/buffer_oob.hip) instead of each pass taking a scalar compare and branch.  The commit stores the
// passes holding ROI rows at immediate LDS offsets (a partial pass's rows past the ROI land in the map,
// cleared after the commit).  No VALU per pass; the general form below clamps every lane's row (3 VALU per pass).
template <int TP, int LD>
__device__ __forceinline__ void fast_issue0(const FastCellSrc& S, const FastLaneMap<TP>& M, FastPrefetch<LD>& F)
{
    constexpr int kRPP = FastLaneMap<TP>::kRPP;
    if (S.rh <= 0 || S.nd <= 0) return;   // wave-uniform
    const uint32_t lo = __umul24((uint32_t)M.rl, (uint32_t)S.pitch) + 4u * (uint32_t)min(M.kl, S.nd - 1);
    // the pass's row offset goes in the scalar offset (buffer_load ... offen with soffset), the lane's in the
    // vector one
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)S.src, (short)0,
                                                                         (S.rh - 1) * S.pitch + 4 * S.nd, 0x00020000);
#pragma unroll
    for (int u = 0; u < LD; ++u) F.w[u] = __builtin_amdgcn_raw_buffer_load_b32(rs, lo, u * kRPP * S.pitch, 0);
}
template <int TP, int LD>
__device__ __forceinline__ void fast_commit0(const FastPrefetch<LD>& F, const FastCellSrc& S, const FastLaneMap<TP>& M,
                                             uint8_t* tile)
{
    constexpr int kRPP = FastLaneMap<TP>::kRPP;
    if (S.rh > 0 && S.nd > 0) {   // wave-uniform (empty cells store nothing)
        const uint32_t a = __umul24((uint32_t)M.rl, (uint32_t)TP) + 4u * (uint32_t)min(M.kl, S.nd - 1) +
                           (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint8_t*)tile;
#pragma unroll
        for (int u = 0; u < LD; ++u)
            if (u * kRPP < S.rh)   // wave-uniform; an immediate offset
                *(__attribute__((address_space(3))) uint32_t*)(uintptr_t)(a + (uint32_t)(u * kRPP * TP)) = F.w[u];
    }
}

// 4 pixels of ROI row r from column 4 kl: the lane's dword and its neighbour's realigned by the row's
// byte shift (v_alignbyte uses the shift's low two bits, so the shift of pass u is the lane's first one
// plus a uniform step), one 4-byte LDS store at an immediate offset per pass
template <int TP, int LD>
__device__ __forceinline__ void fast_commit(const FastPrefetch<LD>& F, const FastCellSrc& S,
                                            const FastLaneMap<TP>& M, int u0, uint8_t* tile)
{
    constexpr int kRPP = FastLaneMap<TP>::kRPP;
    if (S.rh > 0 && S.nd > 0) {   // wave-uniform (empty cells store nothing)
        // 32-bit LDS byte addresses (a pointer offset compiles to a 64-bit multiply-add)
        const uint32_t dst = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint8_t*)tile +
                             4u * (uint32_t)min(M.kl, S.nd - 1);
#pragma unroll
        for (int u = 0; u < LD; ++u) {
            const uint32_t row = (uint32_t)min(u0 * kRPP + u * kRPP + M.rl, S.rh - 1);
            *(__attribute__((address_space(3))) uint32_t*)(uintptr_t)(__umul24(row, (uint32_t)TP) + dst) = F.w[u];
        }
    }
}

#ifdef ORBX_FAST_PROF
// per-phase cycle sums of all FAST waves: staging commit, map clear, pass 1, pass 2, NMS, output, cells
__device__ unsigned long long g_fast_prof[8];
#define FP_STAMP(k)                          \
    do {                                     \
        const long long t1_ = clock64();     \
        fp_acc[k] += t1_ - fp_t;             \
        fp_t = t1_;                          \
    } while (0)
#else
#define FP_STAMP(k) ((void)0)
#endif

__device__ __forceinline__ unsigned long long ballot64(bool p) { return __builtin_amdgcn_ballot_w64(p); }
// (a + b) << 1 in one v_add_lshl_u32
__device__ __forceinline__ uint32_t add_lshl1(uint32_t a, uint32_t b)
{
    uint32_t r;
    asm("v_add_lshl_u32 %0, %1, %2, 1" : "=v"(r) : "v"(a), "s"(b));
    return r;
}
__device__ __forceinline__ uint16_t* lds_u16(uint32_t a) { return (uint16_t*)(__attribute__((address_space(3))) uint16_t*)(uintptr_t)a; }
// per lane: a if the lane's bit of the scalar mask m is set, else b -- one v_cndmask on the mask, with every
// lane active (the compiler's form of the select is an exec-masked region)
__device__ __forceinline__ uint16_t* lds_select(unsigned long long m, uint16_t* a, uint16_t* b)
{
    const uint32_t ua = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint16_t*)a;
    const uint32_t ub = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint16_t*)b;
    uint32_t r;
    asm volatile("v_cndmask_b32 %0, %1, %2, %3" : "=v"(r) : "v"(ub), "v"(ua), "s"(m));
    return (uint16_t*)(__attribute__((address_space(3))) uint16_t*)(uintptr_t)r;
}

// K2: one wave per workgroup (LDS is granted per wave), cpw consecutive cells per wave.  Per cell
// (src/ORBextractor.cc:952-1000, cv::FAST on the cell ROI with nonmax suppression, retried at
// minThFAST when iniThFAST keeps nothing):
//   pass 1   compass value q of every window pixel; q > iniThFAST lists the pixel at the list's front,
//            minThFAST < q <= iniThFAST at its back (q <= t implies strength <= t)
//   pass 2a  exact strength of the front entries into the map (kept if above the lower threshold)
//   NMS      at iniThFAST over the front entries
//   pass 2b  only when it kept nothing: strengths of the back entries, then NMS at minThFAST over both
//   output   kept pixels marked in a per-row bitmask, emitted in row-major order (cv::FAST's order)
// On the synthetic KITTI sequence about 45% of cells fall back, and the front holds about 2% of the
// pixels against 26% for both ends, so the fallback-free cells skip most strength evaluations.
#ifndef ORBX_FAST_WPE
#define ORBX_FAST_WPE 1
#endif
#ifndef ORBX_FAST_WPE10
#define ORBX_FAST_WPE10 1   // 6 (80 VGPRs, 6 dwords spilled) measured 200.9 against 183.3 us
#endif
// A wave's candidates go to HBM as one run from its first cell's slot region, which starts on a 128-byte line
// (the slot regions of a wave's cells are consecutive, so the run fits).  (Measured and removed in round 4:
// the run taken from a per-(frame, level) fill counter by one atomic after the wave's last cell, which makes
// each level's candidates dense -- quadtree fetch 1.05x algorithmic -- but makes every wave wait on the
// atomic's round trip: FAST +13-19 us per 384 frames, -0.8% frames/s)
// Row-validity masks of pass 1: 0 = a ballot of one compare per row step; 1 = scalar arithmetic per trip
// (697.6 against 641.5 us: FAST is sensitive to its scalar instruction count), 2 = the last trip's masks
// hoisted out of the loop, a select per trip (657.7 us)
template <int TP, int LD>
__global__ __launch_bounds__(64, LD >= 10 ? ORBX_FAST_WPE10 : ORBX_FAST_WPE) void k_fast_cells(const Geometry* __restrict__ G, FramePtrs P,
                                                   const Cell* __restrict__ cells, uint32_t* __restrict__ slots,
                                                   int* __restrict__ cell_counts, int cb, int ce, int rw, int rh,
                                                   int cpw)
{
    // cells [cb, ce); LDS sized from the group's largest cell ROI (rw x rh)
    const int lane = threadIdx.x;
    const int lb = xcd_block(blockIdx.x + blockIdx.y * gridDim.x, gridDim.x * gridDim.y);
    const int f = lb / gridDim.x;
    const int c0 = cb + (lb - f * gridDim.x) * cpw;
    const int c1 = min(c0 + cpw, ce);
    if (c0 >= c1) return;   // wave-uniform; no block barriers below
    uint8_t* tile = dyn_lds();
    uint8_t* map = tile + (size_t)rh * TP;
    uint16_t* list = (uint16_t*)(map + fast_map_bytes(rw, rh));
    uint32_t* obuf = (uint32_t*)((uint8_t*)list + fast_list_bytes(rw, rh));
    const int lcap = fast_list_cap(rw, rh);
    uint16_t* const bscratch = (uint16_t*)(obuf + kFastObCap) + lane;
    uint32_t* fslots = slots + (size_t)f * G->slots_per_frame;
    // lane i: the wave's cell c0 + i -- its candidate count, obuf offset (buffered cells) and the slot its
    // candidates start at.  The wave's cells (one level: the cell lists are padded to whole waves) are
    // buffered in obuf and go to HBM together after its last cell, as one run from a 128-byte line, so the
    // quadtree's gather reads few partial lines.  A cell that does not fit obuf, and the wave's cells after
    // it, write to their own slot regions (flagged kCellDirect in cell_counts).
    int cnt_all = 0, c_off = -1;   // c_off >= 0: the lane's cell is buffered
    int obn = 0;
    bool direct = false;   // wave-uniform
    // kept-pixel bitmask, one u64 per window row: aliases the tile, which is dead once every strength
    // of the cell is known
    unsigned long long* kept = (unsigned long long*)tile;
    const int t_ini = G->ini_th, t_min = G->min_th;
    const int t_lo = min(t_ini, t_min);
    const _Float16 f_hi = int16_as_f16(t_ini), f_lo = int16_as_f16(t_lo);   // thresholds as denormals
#ifdef ORBX_FAST_PROF
    long long fp_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    long long fp_t = clock64();
#endif

    // ROI -> LDS: aligned dword loads (alignbyte realigns rows of any pitch; the ROI ends >= 16
    // px before the level's right edge, so the 8-byte read stays in the row), 4 packed pixels
    // per 16-byte LDS store.  The next cell's loads are issued before this cell's passes.
    auto cell_src = [&](const Cell& C) {
        FastCellSrc S;
        int pitch;
        const uint8_t* img = level_base(P, G, f, C.level, pitch);
        S.src = img + (size_t)C.roi_y0 * pitch + C.roi_x0;
        S.pitch = pitch;
        S.nd = (C.roi_w + 3) >> 2;
        S.rh = C.roi_h;
        return S;
    };
    // the cell descriptor as whole dwords: scalar loads (a 16-bit field read is a vector load, whose
    // vmcnt wait would also drain every store still in flight)
    auto load_cell = [&](int ci) {
        const uint32_t* w = (const uint32_t*)(cells + ci);
        const uint32_t w0 = w[0], w1 = w[1];
        Cell r;
        r.level = (int16_t)(w0 & 0xFFFF);
        r.roi_w = (int16_t)(w0 >> 16);
        r.roi_h = (int16_t)(w1 & 0xFFFF);
        r.pad = 0;
        r.roi_x0 = (int32_t)w[2];
        r.roi_y0 = (int32_t)w[3];
        r.slot_base = (int32_t)w[4];
        r.slot_cap = (int32_t)w[5];
        return r;
    };
    Cell C = load_cell(c0);
    FastCellSrc S = cell_src(C);
    const FastLaneMap<TP> M(lane);
    FastPrefetch<LD> F;
    fast_issue0(S, M, F);

#pragma unroll 1
    for (int c = c0; c < c1; ++c) {
        const int dw = C.roi_w - 6, dh = C.roi_h - 6;
        const Cell Cc = C;
        FP_STAMP(7);
        fast_commit0(F, S, M, tile);
        for (int u0 = LD; u0 * FastLaneMap<TP>::kRPP < S.rh; u0 += LD) {   // ROIs beyond LD passes
            FastPrefetch<LD> R;
            fast_issue(S, M, u0, R);
            fast_commit(R, S, M, u0, tile);
        }
        const int mapn = (dh + 2) * TP;
        FP_STAMP(0);
        if constexpr (TP % 8 == 0) {   // the map (at rh * TP) and mapn are whole 8-byte words: half the stores
            for (int i = lane; i < mapn >> 3; i += 64) ((uint2*)map)[i] = make_uint2(0u, 0u);
        } else {
            for (int i = lane; i < (mapn + 3) >> 2; i += 64) ((uint32_t*)map)[i] = 0u;
        }
        wave_lds_sync();
        FP_STAMP(1);
        if (c + 1 < c1) {   // prefetch the next cell (registers only; lands under the passes below)
            C = load_cell(c + 1);
            S = cell_src(C);
            fast_issue0(S, M, F);
        }
        if (dw <= 0 || dh <= 0) {
            wave_lds_sync();
            continue;
        }

        // ---- pass 1: a pass covers 64 / cw rows of cw = 32 or 64 columns (row-major lanes); two row
        // steps per trip.  Lanes outside the window read in-bounds LDS (the tile's slack rows, the map)
        // and are masked out.  Pixels are named by their window index m = i * TP + j: the pixel's tile
        // value is tile[m + 3 * TP + 3] and its map byte map[m + TP + 1], so every ring, compass and
        // neighbour access is (tile or map) + m plus a non-negative immediate offset.
        int nf = 0, nb = 0;   // front / back entries
        // Exec for the list writes comes straight from the scalar masks (inverse ballot: no per-lane flag
        // in a VGPR, no VALU compare to rebuild it).  The order of entries inside a list does not matter
        // (survivors are emitted through the row bitmask), so a trip's back entries take
        // [lcap - nb - count, lcap - nb) in lane order.  The loop is compiled once per column width
        // (cw = 32 or 64), so the second row step's offset is an immediate.
        auto pass1 = [&](auto cw_tag) {
            constexpr int kCwShift = decltype(cw_tag)::value;
            const int cw_shift = kCwShift > 0 ? kCwShift : (dw <= 32 ? 5 : 6);
            const int col = lane & ((1 << cw_shift) - 1);
            const int rstep = 64 >> cw_shift;
            const int rlane = lane >> cw_shift;
            int t = rlane * TP + col;   // the lane's window index m in the trip's first row step
            // LDS address of list[lcap - nb] in u16 entries: a back write's byte address is one v_add_lshl from
            // it, and its update one scalar subtract of the count
            const uint32_t bend = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint16_t*)(list + lcap);
            uint32_t bptr = bend >> 1;
            const int rlane_b = rlane + rstep;
            // Thresholds per lane: +inf in the lanes past the window's columns, so a full trip's compares need no
            // column mask (two scalar ANDs per row step fewer).  The last, partial trip also takes its row masks
            // (the loop body is a lambda of the two masks, inlined twice).
            const _Float16 inf16 = __builtin_bit_cast(_Float16, (uint16_t)0x7C00);
            const _Float16 th_hi = col < dw ? f_hi : inf16, th_lo = col < dw ? f_lo : inf16;
            int rem = dh;
            auto trip = [&](auto full_tag, const unsigned long long va, const unsigned long long vb) {
                constexpr bool kFull = decltype(full_tag)::value;
                const _Float16 qa = fast_compass_q<TP>(tile + t + (3 * TP + 3));
                const _Float16 qb = fast_compass_q<TP>(tile + t + (rstep * TP + 3 * TP + 3));
                const unsigned long long hqa = ballot64(qa > th_hi), hqb = ballot64(qb > th_hi);
                const unsigned long long lqa = ballot64(qa > th_lo) & ~hqa, lqb = ballot64(qb > th_lo) & ~hqb;
                const unsigned long long mfa = kFull ? hqa : hqa & va, mba = kFull ? lqa : lqa & va;
                const unsigned long long mfb = kFull ? hqb : hqb & vb, mbb = kFull ? lqb : lqb & vb;
                // front entries are rare (about 2% of the pixels): one scalar test per trip skips both writes'
                // exec save / restore and the count updates (s_or sets SCC)
                if (mfa | mfb) {
                    if (__builtin_amdgcn_inverse_ballot_w64(mfa)) list[nf + lanes_below(mfa)] = (uint16_t)t;
                    nf += __popcll(mfa);
                    if (__builtin_amdgcn_inverse_ballot_w64(mfb)) list[nf + lanes_below(mfb)] = (uint16_t)(t + rstep * TP);
                    nf += __popcll(mfb);
                }
                // back entries (a quarter of the pixels: the mask is rarely empty) written by every lane, the
                // lanes outside the mask into their own scratch dword: an address select instead of the exec
                // save / branch / restore (FAST's time follows its scalar instruction count)
                bptr -= (uint32_t)__popcll(mba);
                *lds_select(mba, lds_u16(add_lshl1((uint32_t)lanes_below(mba), bptr)), bscratch) = (uint16_t)t;
                bptr -= (uint32_t)__popcll(mbb);
                *lds_select(mbb, lds_u16(add_lshl1((uint32_t)lanes_below(mbb), bptr)), bscratch) = (uint16_t)(t + rstep * TP);
                t += 2 * rstep * TP;
            };
            // a bottom-tested count of full trips: one scalar decrement, compare and branch per trip
            const int nfull = rem / (2 * rstep);
            if (nfull > 0) {
                int k = nfull;
                do trip(std::true_type{}, 0ull, 0ull);
                while (--k > 0);
            }
            rem -= nfull * 2 * rstep;
            if (rem > 0) trip(std::false_type{}, ballot64(rlane < rem), ballot64(rlane_b < rem));
            nb = (int)((bend >> 1) - bptr);
        };
        if constexpr (LD < 10) {   // (the 10-register prefetch kernels: 76 VGPRs, 6 waves per SIMD)
            if (dw <= 32) pass1(std::integral_constant<int, 5>{});
            else pass1(std::integral_constant<int, 6>{});
        } else {
            pass1(std::integral_constant<int, 0>{});
        }
        wave_lds_sync();
        FP_STAMP(2);

        // ---- pass 2: exact strengths of list entries [j0, j1) (front: ascending positions, back:
        // descending from lcap - 1) into the map; the entries above the lower threshold are compacted in
        // place (a trip writes at or before what it has read).  Returns the compacted count.
        auto strengths = [&](int n, bool back) {
            int n2 = 0;
            // one entry per lane per trip: the strength's 16 ring values and their arc maxima are the
            // kernel's register peak, and only ~15% of the window gets here
            // full trips (64 entries) without the tail clamp and its mask; the last, partial trip peeled (the
            // 8-register prefetch only: 67 VGPRs; the 10-register ones would drop to 6 waves per SIMD)
            if constexpr (LD < 10) {
            auto trip = [&](const int j0, auto full_tag) {
                constexpr bool kFull = decltype(full_tag)::value;
                const int ja = j0 + lane;
                const int jc = kFull ? ja : min(ja, n - 1);   // lanes past the list re-test its last entry
                const int ka = list[back ? lcap - 1 - jc : jc];
                const int sa = fast_strength<TP>(tile + ka + (3 * TP + 3));
                const unsigned long long ma = kFull ? ballot64(sa > t_lo) : ballot64(ja < n) & ballot64(sa > t_lo);
                *(uint8_t*)lds_select(ma, (uint16_t*)(map + ka + (TP + 1)), bscratch) = (uint8_t)sa;
                wave_lds_sync();   // the entries are read before the compaction overwrites the list
                *lds_select(ma, &list[back ? lcap - 1 - (n2 + lanes_below(ma)) : n2 + lanes_below(ma)], bscratch) = (uint16_t)ka;
                n2 += __popcll(ma);
            };
            int j0 = 0;
            for (; j0 + 64 <= n; j0 += 64) trip(j0, std::true_type{});
            if (j0 < n) trip(j0, std::false_type{});
            } else
            for (int j0 = 0; j0 < n; j0 += 64) {
                const int ja = j0 + lane;
                // lanes past the list re-test its last entry, masked out below
                const int pa = back ? lcap - 1 - min(ja, n - 1) : min(ja, n - 1);
                const int ka = list[pa];
                const int sa = fast_strength<TP>(tile + ka + (3 * TP + 3));
                // mask before any branch (an i1 live across a divergent branch is materialised in a VGPR)
                const unsigned long long ma = ballot64(ja < n) & ballot64(sa > t_lo);
                // both stores by every lane through address selects (the masked-off lanes into scratch)
                *(uint8_t*)lds_select(ma, (uint16_t*)(map + ka + (TP + 1)), bscratch) = (uint8_t)sa;
                wave_lds_sync();   // the entries are read before the compaction overwrites the list
                *lds_select(ma, &list[back ? lcap - 1 - (n2 + lanes_below(ma)) : n2 + lanes_below(ma)], bscratch) = (uint16_t)ka;
                n2 += __popcll(ma);
            }
            wave_lds_sync();
            return n2;
        };
        const int nf2 = strengths(nf, false);
        FP_STAMP(3);

        // ---- NMS: rounds of 64 entries over the front [0, nf2) then the back; survivors remembered
        // per round (at most 2 * 57 rounds for the 66 x 66 cap: two masks)
        auto nms = [&](int nfr, int nbk, int th, unsigned long long (&keepm)[2]) {
            const int rounds = (nfr + nbk + 63) >> 6;
            int kept_n = 0;
            keepm[0] = keepm[1] = 0;
            auto round = [&](int r, unsigned long long& km) {
                const int j = lane + (r << 6);
                // branch-free: lanes past the entries re-test the last one, masked out of the ballot
                const int jc = min(j, nfr + nbk - 1);
                const int k = list[jc < nfr ? jc : lcap - 1 - (jc - nfr)];
                const bool keep = (j < nfr + nbk) & nms_keep<TP>(map + k + (TP + 1), (uint32_t)max(th, 1));
                km |= (unsigned long long)keep << (r & 63);
                kept_n += __popcll(ballot64(keep));
            };
            // one loop per mask word, so that the word is not selected by the round at run time
            const int r1 = min(rounds, 64);
            for (int r = 0; r < r1; ++r) round(r, keepm[0]);
            for (int r = 64; r < rounds; ++r) round(r, keepm[1]);
            return kept_n;
        };
        unsigned long long keepm[2];
        int nbk = 0;
        int kept_n = nms(nf2, 0, t_ini, keepm);
        if (kept_n == 0) {   // src/ORBextractor.cc:982-987: retry the cell at minThFAST
            if (t_min < t_ini) nbk = strengths(nb, true);
            kept_n = nms(nf2, nbk, t_min, keepm);
        }
        FP_STAMP(4);

        // ---- output, row-major (cv::FAST's order) into the wave's output buffer, or straight to HBM for a
        // cell with more than the buffer holds.  Survivors of the front list alone (no fallback: about 55% of
        // KITTI cells) are already in row-major order -- pass 1 appends a trip's front entries in lane order,
        // trips in row order, and the strength pass compacts in place -- so they go out by one ballot per NMS
        // round.  A fallback cell merges front and back survivors through a per-row bitmask (the tile is dead
        // now): one bit per kept pixel, then lane i emits window row i.
        if (kept_n > 0) {
            const int xr0 = Cc.roi_x0 + 3 - kMinBorder, yr0 = Cc.roi_y0 + 3 - kMinBorder;
            const uint32_t kxb = (uint32_t)G->kp_xbits;   // packed keypoint x width (pack_kp)
            const int ci = c - c0;
            const bool buffered = !direct && obn + kept_n <= kFastObCap;   // wave-uniform
            const int rounds = (nf2 + nbk + 63) >> 6;
            // (one copy of the emission per destination, so that each store's address space is known: a pointer
            // that may be either compiles to flat stores, which wait on both counters)
            auto emit = [&](uint32_t* dst) {
                if (nbk == 0) {
                    int idx = 0;
                    auto round = [&](int r, unsigned long long kw) {
                        const bool keep = (kw >> (r & 63)) & 1ull;
                        const unsigned long long km = ballot64(keep);
                        if (km == 0ull) return;   // wave-uniform
                        if (keep) {
                            const int m = list[lane + (r << 6)];   // window (i, j) at m = i * TP + j
                            const int wi = m / TP, wj = m - wi * TP;
                            const int sc = map[m + TP + 1];
                            dst[idx + lanes_below(km)] = pack_kp((uint32_t)(xr0 + wj), (uint32_t)(yr0 + wi), (uint32_t)(sc - 1), kxb);
                        }
                        idx += __popcll(km);
                    };
                    for (int r = 0; r < min(rounds, 64); ++r) round(r, keepm[0]);
                    for (int r = 64; r < rounds; ++r) round(r, keepm[1]);
                } else {
                    for (int i = lane; i < dh; i += 64) kept[i] = 0ull;
                    wave_lds_sync();
                    auto mark = [&](int r, unsigned long long kw) {
                        if (!((kw >> (r & 63)) & 1ull)) return;
                        const int j = lane + (r << 6);
                        const int m = list[j < nf2 ? j : lcap - 1 - (j - nf2)];
                        const int wi = m / TP;
                        atomicOr(&kept[wi], 1ull << (m - wi * TP));
                    };
                    for (int r = 0; r < min(rounds, 64); ++r) mark(r, keepm[0]);
                    for (int r = 64; r < rounds; ++r) mark(r, keepm[1]);
                    wave_lds_sync();
                    // lane i emits window row i (rows <= 60): prefix sum of the row counts gives its first slot
                    const unsigned long long rowbits = lane < dh ? kept[lane] : 0ull;
                    const int cnt = __popcll(rowbits);
                    int base = 0;
                    {
                        int v = cnt;
                        // inclusive wave scan of the counts
#pragma unroll
                        for (int o = 1; o < 64; o <<= 1) {
                            const int u = __shfl_up(v, o);
                            if (lane >= o) v += u;
                        }
                        base = v - cnt;
                    }
                    unsigned long long bits = rowbits;
                    int idx = base;
                    while (bits) {
                        const int jj = __builtin_ctzll(bits);
                        bits &= bits - 1;
                        const int sc = map[(lane + 1) * TP + jj + 1];
                        dst[idx++] = pack_kp((uint32_t)(xr0 + jj), (uint32_t)(yr0 + lane), (uint32_t)(sc - 1), kxb);
                    }
                }
            };
            if (buffered) {
                if (lane == ci) c_off = obn;
                emit(obuf + obn);
                obn += kept_n;
            } else {   // rare: more than obuf holds
                direct = true;
                emit(fslots + Cc.slot_base);
            }
        }
        if (lane == c - c0) cnt_all = kept_n;
        wave_lds_sync();   // tile, map and list are rewritten by the next cell
        FP_STAMP(5);
#ifdef ORBX_FAST_PROF
        fp_acc[6] += 1;
#endif
    }
    if (obn > 0) {   // the buffered cells: one run from the wave's first cell's slot base (128-byte aligned)
        uint32_t* out = fslots + cells[c0].slot_base;
        if (lane < obn) out[lane] = obuf[lane];
        if (kFastObCap > 64 && lane + 64 < obn) out[lane + 64] = obuf[lane + 64];
        static_assert(kFastObCap <= 128, "two stores per lane");
    }
    // a cell written straight to its own slots is flagged; the buffered ones' slots follow from the counts
    if (lane < c1 - c0)
        cell_counts[(size_t)f * G->ncells + c0 + lane] = (int)((uint32_t)cnt_all | (c_off < 0 && cnt_all > 0 ? kCellDirect : 0u));
#ifdef ORBX_FAST_PROF
    if (lane == 0)
        for (int k = 0; k < 8; ++k) atomicAdd(&g_fast_prof[k], (unsigned long long)fp_acc[k]);
#endif
}
#ifdef ORBX_FAST_PROF
}  // namespace orbx
extern "C" int orbx_debug_fast_prof(unsigned long long* out, int reset)
{
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(orbx::g_fast_prof), sizeof(orbx::g_fast_prof)) != hipSuccess) return -1;
    if (reset) {
        static unsigned long long zero[8];
        if (hipMemcpyToSymbol(HIP_SYMBOL(orbx::g_fast_prof), zero, sizeof(zero)) != hipSuccess) return -1;
    }
    return 0;
}
namespace orbx {
#endif

// LDS per CU on gfx950: the occupancy a FAST launch's per-wave tiles allow, up to what the kernel's
// registers allow (<40, 8>: 71 VGPRs, 7 waves per SIMD, 28 one-wave workgroups per CU; round 3's
// realigning staging: 80 VGPRs, 24)
#ifndef ORBX_FAST_OCC
#define ORBX_FAST_OCC 28
#endif
constexpr size_t kLdsPerCu = 160 * 1024;
constexpr int kFastVgprWavesPerCu = ORBX_FAST_OCC;
static int fast_blocks_per_cu(int w, int h)
{
    return std::min((int)(kLdsPerCu / fast_wave_bytes(w, h)), kFastVgprWavesPerCu);
}

void fast_groups(Geometry& g)
{
    // The longest prefix of levels whose largest ROI keeps level 0's occupancy is launch 0; the
    // remaining levels are launch 1.  Cells are stored level by level, so each launch is a contiguous
    // range.  With the byte tile every KITTI level's ROI (up to 38x46) fits the register-limited 6 waves
    // per SIMD, so KITTI runs one launch.
    int w = g.lv[0].roi_mw, h = g.lv[0].roi_mh, split = g.nlevels;
    const int occ0 = fast_blocks_per_cu(std::max(w, 8), std::max(h, 8));
    for (int l = 1; l < g.nlevels; ++l) {
        const int nw = std::max(w, g.lv[l].roi_mw), nh = std::max(h, g.lv[l].roi_mh);
        if (fast_blocks_per_cu(nw, nh) < occ0) {
            split = l;
            break;
        }
        w = nw;
        h = nh;
    }
    g.fast_cb[0] = 0;
    g.fast_rw[0] = std::max(w, 8);
    g.fast_rh[0] = std::max(h, 8);
    if (split == g.nlevels) {
        g.fast_groups = 1;
        g.fast_cb[1] = g.ncells;
        return;
    }
    int w1 = 8, h1 = 8;
    for (int l = split; l < g.nlevels; ++l) {
        w1 = std::max(w1, g.lv[l].roi_mw);
        h1 = std::max(h1, g.lv[l].roi_mh);
    }
    g.fast_groups = 2;
    g.fast_cb[1] = g.lv[split].cell_begin;
    g.fast_cb[2] = g.ncells;
    g.fast_rw[1] = w1;
    g.fast_rh[1] = h1;
}

template <int TP, int LD>
static void fast_launch(const ExtractBufs& b, const FramePtrs& p, int cb, int ce, int rw, int rh, int cpw,
                        int batch, hipStream_t s)
{
    dim3 grid((ce - cb + cpw - 1) / cpw, batch);
    const size_t smem = fast_wave_bytes(rw, rh);
    hipFuncSetAttribute((const void*)k_fast_cells<TP, LD>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    hipLaunchKernelGGL((k_fast_cells<TP, LD>), grid, dim3(64), smem, s, b.geom, p, b.cells, b.slots, b.cell_counts,
                       cb, ce, rw, rh, cpw);
}

int fast_plan(const Geometry& g, int batch, FastRun* out)
{
    // small batches: every cell in one launch sized for the largest ROI (one launch latency fewer; the
    // occupancy split only pays when the chip is full)
    if (batch <= kLatencyMaxBatch && g.fast_groups > 1) {
        out[0] = {0, g.ncells, std::max(g.fast_rw[0], g.fast_rw[1]), std::max(g.fast_rh[0], g.fast_rh[1])};
        return 1;
    }
    int n = 0;
    for (int i = 0; i < g.fast_groups; ++i)
        if (g.fast_cb[i + 1] > g.fast_cb[i]) out[n++] = {g.fast_cb[i], g.fast_cb[i + 1], g.fast_rw[i], g.fast_rh[i]};
    return n;
}

void launch_fast(const Geometry& g, const ExtractBufs& b, const FramePtrs& p, int batch, hipStream_t s)
{
    // small batches (the per-frame host path) are latency-bound: one cell per wave, 3x the waves
    const int cpw = fast_cells_per_wave(batch);
    FastRun run[kFastMaxRuns];
    const int n = fast_plan(g, batch, run);
    for (int i = 0; i < n; ++i) {
        const FastRun& r = run[i];
        // register prefetch passes: the run's largest ROI in passes of whole rows (FastLaneMap)
        const int rpp = 64 / fast_lanes_per_row(fast_tile_pitch(r.rw)), ld = (r.rh + rpp - 1) / rpp;
        if (fast_tile_pitch(r.rw) == 40) {
            if (ld <= 8) fast_launch<40, 8>(b, p, r.cb, r.ce, r.rw, r.rh, cpw, batch, s);
            else fast_launch<40, 10>(b, p, r.cb, r.ce, r.rw, r.rh, cpw, batch, s);
        } else {
            fast_launch<68, 10>(b, p, r.cb, r.ce, r.rw, r.rh, cpw, batch, s);
        }
    }
}

}  // namespace orbx

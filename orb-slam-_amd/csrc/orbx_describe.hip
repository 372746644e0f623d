// gfx950 kernels of the ORB extractor (ORB_SLAM2::ORBextractor::operator(),
// src/ORBextractor.cc:1248-1334).  Integer/bitwise path: no MFMA.
//
//   K4 k_describe       IC_Angle + GaussianBlur + rBRIEF + scale/pack,
//                       :84-128, :1300-1332, :141-192
#include <hip/hip_runtime.h>

#include <algorithm>

#include "orbx_device.hpp"
#include "orbx_kernels.hpp"
#include "orbx_math.hpp"

namespace orbx {

// ---------------------------------------------------------------------------
// K4: a wave describes kDescPerWave consecutive retained keypoints.
//   raw   the 43-row neighbourhood of the keypoint in LDS, 48 B per row.
//         Interior keypoints arrive by LDS-DMA (global_load_lds_dwordx4: three
//         instructions of 16-byte pieces, three per row, so row r starts at
//         byte sh_r = (src + r*pitch) & 3 of its LDS row);
//         border keypoints are filled with reflect-101 bytes at shift 0.  The next keypoint's DMA is issued as soon as the
//         current one's raw reads are done, so it lands under the BRIEF work.
//   angle IC_Angle: u*I and v*I over the 749-pixel disc as per-lane column
//         sums (lane = disc column, half-wave = upper/lower rows), wave
//         reduction, then cv::fastAtan2 (src/ORBextractor.cc:84-128).
//   blur  GaussianBlur 7x7 integer kernel [18 34 49 55 49 34 18], >>16
//         (SURVEY.md A.3): the horizontal pass is v_dot4_u32_u8 on 4 output
//         columns x 2 rows per lane, stored transposed as u16 row pairs; the
//         vertical pass is evaluated only at the 512 BRIEF sample points with
//         four v_dot2_u32_u16 each.
//   BRIEF fmaf sample coordinates, 256 tests -> four __ballot
//         words = the descriptor's little-endian u64 words (:141-192).
// ---------------------------------------------------------------------------
constexpr int kRawP = 48;                             // LDS row pitch (bytes): the 43 columns + shift slack
constexpr int kRawRows = 44;                          // 43 rows used (row 43 repeats row 42)
constexpr int kRawSlots = kRawRows * kRawP / 4;
// row-blurred, transposed: [col][row pairs], 23 dwords per column (22 hold the 44 rows; the odd pitch spreads
// the horizontal pass's column stores over the banks: 48 LDS-array cycles per keypoint against 68 at 22, and
// 98 against 108 for the blur reads of tools/gen/brief_slots.py's slots)
constexpr int kTCols = 40, kTP = 23;
#ifndef ORBX_DESC_KPW
#define ORBX_DESC_KPW 4
#endif
constexpr int kDescPerWave = ORBX_DESC_KPW;           // keypoints per wave (lane state set up once per wave)
#ifndef ORBX_DESC_WAVES
#define ORBX_DESC_WAVES 1
#endif
// waves per describe workgroup: one, so a workgroup's LDS (6.3 KB) frees as soon as its own keypoints are done
// and no wave waits on slower siblings (4 waves: 863 us per 384 frames, 2: 815, 1: 768; pipelined 169.1k ->
// 176.4k frames/s)
constexpr int kDescWaves = ORBX_DESC_WAVES;

// Horizontal-pass items (row pair rp << 8 | column group cg) that BRIEF can read: a sample
// (18 + xx, 18 + yy) has |(x, y)| <= 18.39 before rounding (the pattern's largest radius), so a
// column group needs only the row pairs its disc chord reaches, plus the 7-tap reach of
// blur_acc.  189 of the 22 x 10 items: three per lane, row-pair major so that the lanes of a
// load read neighbouring raw dwords (distinct LDS banks).
__constant__ uint16_t c_blur_items[192] = {2,3,4,5,6,257,258,259,260,261,262,263,513,514,515,516,517,518,519,768,769,770,771,772,773,774,775,776,1024,1025,1026,1027,1028,1029,1030,1031,1032,1280,1281,1282,1283,1284,1285,1286,1287,1288,1536,1537,1538,1539,1540,1541,1542,1543,1544,1545,1792,1793,1794,1795,1796,1797,1798,1799,1800,1801,2048,2049,2050,2051,2052,2053,2054,2055,2056,2057,2304,2305,2306,2307,2308,2309,2310,2311,2312,2313,2560,2561,2562,2563,2564,2565,2566,2567,2568,2569,2816,2817,2818,2819,2820,2821,2822,2823,2824,2825,3072,3073,3074,3075,3076,3077,3078,3079,3080,3081,3328,3329,3330,3331,3332,3333,3334,3335,3336,3337,3584,3585,3586,3587,3588,3589,3590,3591,3592,3593,3840,3841,3842,3843,3844,3845,3846,3847,3848,3849,4096,4097,4098,4099,4100,4101,4102,4103,4104,4352,4353,4354,4355,4356,4357,4358,4359,4360,4609,4610,4611,4612,4613,4614,4615,4616,4865,4866,4867,4868,4869,4870,4871,5122,5123,5124,5125,5126,5127,5379,5380,5381,5382,65535,65535,65535};
constexpr int kUmax[16] = {15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3};
// GaussianBlur(7x7, sigma 2)'s integer taps per ORBX_BLUR_* mode: OpenCV <= 3.4.1 (scalar and
// SSE2 column passes) converts getGaussianKernel's floats at x256, [18 34 49 55 49 34 18] (sum 257); 3.4.6+ / 4.x's
// bit-exact GaussianBlur carries the rounding error inwards and closes the sum at 256, [18 34 48 56 48 34 18]
__host__ __device__ constexpr uint32_t blur_tap(int bm, int t)
{
    return t == 2 || t == 4 ? (bm == ORBX_BLUR_BITEXACT ? 48u : 49u)
                            : t == 3 ? (bm == ORBX_BLUR_BITEXACT ? 56u : 55u) : (t == 1 || t == 5 ? 34u : 18u);
}
// GaussianBlur's 7 taps starting at byte `off` of four consecutive raw dwords: the weight bytes of dword d
__host__ __device__ constexpr uint32_t blur_wshift(int off, int d, int bm = ORBX_BLUR_SCALAR)
{
    uint32_t w = 0;
    for (int b = 0; b < 4; ++b) {
        const int t = 4 * d + b - off;
        if (t >= 0 && t < 7) w |= blur_tap(bm, t) << (8 * b);
    }
    return w;
}
constexpr int kPattern[1024] = {
#include "orb_pattern.inc"
};
#include "orb_slots.inc"

// Keypoint-independent lane state of k_describe, a function of the lane alone, built at compile time
// (the kernel loads it instead of computing ~235 VALU instructions per wave).
//   IC_Angle: lane 2i + h owns disc row v = i - 15 (i < 31), half h: u = -15..0 or 1..15, as 4
//   realigned dwords of the raw row dotted (v_dot4_u32_u8) with per-lane weights that are zero
//   outside |u| <= umax[|v|]: w1 = (u + 16) for m10 (minus 16 * sum I), w0 = 1 for sum I.
//   rBRIEF: the pattern's 512 points hold 375 distinct ones.  Each is blurred once, in slot 64 q + lane (lane,
//   round q < 6) of a u16 table; test m = 64 wd + lane (wd = q >> 1) reads its two samples (e = q & 1) from
//   slot byte offsets rd[q].  Which point sits in which slot (orb_slots.inc, tools/gen/brief_slots.py) keeps
//   each half-round's 32 points a compact cluster of the pattern, so their blur reads share LDS addresses
//   and spread over the banks at any keypoint angle (98 LDS-array cycles per keypoint against 156 for the
//   points in order of first use, 212 for the 512 points of round 4), and orders lanes inside each
//   half-round for the table reads' banks.
constexpr int kDescSlots = 6;   // distinct sample points per lane (384 slots >= 375)
struct DescLane {
    uint32_t w1[4], w0[4];
    float upx[kDescSlots], upy[kDescSlots];
    uint32_t rd[8];
};
struct DescLaneTable {
    DescLane l[64];
};
constexpr DescLaneTable make_desc_lanes()
{
    DescLaneTable t{};
    for (int lane = 0; lane < 64; ++lane) {
        const int icv = lane >> 1, ich = lane & 1, vrow = icv - 15;
        const int rmax = icv < 31 ? kUmax[vrow < 0 ? -vrow : vrow] : -1;
        for (int k = 0; k < 4; ++k)
            for (int b = 0; b < 4; ++b) {
                const int uu = (ich ? 1 : -15) + 4 * k + b;
                if (uu <= (ich ? 15 : 0) && (uu < 0 ? -uu : uu) <= rmax) {
                    t.l[lane].w1[k] |= (uint32_t)(uu + 16) << (8 * b);
                    t.l[lane].w0[k] |= 1u << (8 * b);
                }
            }
    }
    for (int lane = 0; lane < 64; ++lane) {
        for (int q = 0; q < kDescSlots; ++q) {
            const int i = kSlotPt[64 * q + lane];
            t.l[lane].upx[q] = (float)kPattern[2 * i];
            t.l[lane].upy[q] = (float)kPattern[2 * i + 1];
        }
        for (int q = 0; q < 8; ++q) {
            const int m = (q >> 1) * 64 + lane, e = q & 1;
            t.l[lane].rd[q] = 2u * (uint32_t)kPtSlot[2 * m + e];
        }
    }
    return t;
}
// every pattern point's slot holds that point
constexpr bool desc_slots_ok()
{
    for (int i = 0; i < 512; ++i) {
        const int s = kPtSlot[i];
        if (s < 0 || s >= 64 * kDescSlots) return false;
        const int j = kSlotPt[s];
        if (kPattern[2 * j] != kPattern[2 * i] || kPattern[2 * j + 1] != kPattern[2 * i + 1]) return false;
    }
    return true;
}
static_assert(desc_slots_ok(), "orb_slots.inc does not match orb_pattern.inc");
__constant__ DescLaneTable c_desc_lanes = make_desc_lanes();

// Sample coordinates as float bits: fl + 1.5 * 2^23 rounds fl to the nearest integer, ties to even
// (one f32 addition into [2^23, 2^24), whose ulp is 1; the magic number is even, so the tie parity
// is fl's), exactly __float2int_rn for |fl| < 2^22, and leaves that integer in the low mantissa
// bits: bits = 0x4B400000 + round(fl).  The blur lookup indexes with these bits directly.
constexpr float kRoundMagic = 12582912.0f;
constexpr uint32_t kRoundBits = 0x4B400000u;

// blurred value at patch row 18 + yy, column 18 + xx (|xx|, |yy| <= 19, given as kRoundMagic
// bits by, bx): sum_t k[t] * rowblur[y+t][x], + 2^15 (the >> 16 rounding) folded into the sum.
// The dword index is (18 + xx) * kTP + ((18 + yy) >> 1), in wrapping u32 arithmetic on the bits of
// bx (its low 24 bits are 0x400000 + xx) and by (bits 1..23: 0x200000 + ((18 + yy) >> 1) - 9).
// The LDS byte address in three VALU: bfe of by's bits 1..23 (0x200000 + (yy >> 1)), shifted and added to
// mad24(bx, 4 kTP, C) with C = rowT + 4 (9 - 0x200000 + (18 - 0x400000) kTP) (mod 2^32); the compiler's
// form of (by >> 1) + bx * kTP + rowT took five.
constexpr uint32_t kBlurByte0 = 4u * (9u - 0x200000u + (18u - 0x400000u) * (uint32_t)kTP);
template <int kBM>
__device__ __forceinline__ uint32_t blur_acc(uint32_t C, uint32_t by, uint32_t bx)
{
    const uint32_t t = __umul24(bx, 4u * (uint32_t)kTP) + C, f = __builtin_amdgcn_ubfe(by, 1, 23);
    uint32_t a;
    // one v_lshl_add_u32 (the compiler rewrites (f << 2) + t as (by << 1) & mask plus an add)
    asm("v_lshl_add_u32 %0, %1, 2, %2" : "=v"(a) : "v"(f), "v"(t));
    const __attribute__((address_space(3))) uint32_t* col = (const __attribute__((address_space(3))) uint32_t*)(uintptr_t)a;
    const uint32_t d0 = col[0], d1 = col[1], d2 = col[2], d3 = col[3];
    // rows y..y+6 are (d0.lo d0.hi d1.lo d1.hi d2.lo d2.hi d3.lo) for even y and (d0.hi .. d3.hi) for odd y:
    // shifting the dword chain right by 16 bits for odd y (v_alignbit uses its shift's low five bits, so
    // by << 4 is that shift) leaves the same weights for both parities -- in SGPRs, where the per-lane
    // selection of round 4 (four v_cndmask, a test) held both weight sets in VGPRs
    const uint32_t sh = by << 4;
    const uint32_t e0 = __builtin_amdgcn_alignbit(d1, d0, sh), e1 = __builtin_amdgcn_alignbit(d2, d1, sh);
    const uint32_t e2 = __builtin_amdgcn_alignbit(d3, d2, sh), e3 = d3 >> (sh & 31u);
    constexpr unsigned short k1 = (unsigned short)blur_tap(kBM, 2), k3 = (unsigned short)blur_tap(kBM, 3);
    uint32_t acc = __builtin_amdgcn_udot2(as_us2(e0), ushort2_t{18, 34}, 1u << 15, false);
    acc = __builtin_amdgcn_udot2(as_us2(e1), ushort2_t{k1, k3}, acc, false);
    acc = __builtin_amdgcn_udot2(as_us2(e2), ushort2_t{k1, 34}, acc, false);
    return __builtin_amdgcn_udot2(as_us2(e3), ushort2_t{18, 0}, acc, false);
}
// How k_describe stages the 43 x 43 patch of a keypoint at (cx, cy) of level l (w x h pixels, `pitch` bytes per
// row); the one statement of the choice, for the staging and for the border fix-up (tests/test_describe_borders.py
// restates it as classify() and asserts that its images put keypoints in every class).
//   kPatchDma      interior keypoints, and right-border ones whose 43 columns are all inside the level
//                  (cx + 21 < w): those read up to 9 bytes past the row end, which land in the row padding or in the
//                  next row of the same level (cy + 22 < h) and only feed blurred columns BRIEF never samples
//                  (|x| <= 18 + the 3-tap reach).  About 2/3 of the 6.5% of KITTI keypoints the byte path took before.
//   kPatchBufDma   border keypoints of levels >= 1 whose rows have >= 16 bytes of padding: the same DMA through a
//                  buffer descriptor over the level's rows; bytes outside the level read as zeros and are repaired
//                  in LDS.  A 16-byte piece can straddle the descriptor's end only within the level's last 16 bytes,
//                  which the padding bound makes row padding (a level with less, e.g. 444 px in a 448-byte pitch,
//                  takes the byte path).  Not for cx < 21 with cy <= 21: there the piece that holds level row 0's
//                  first pixels starts at offset -4 (0xFFFFFFFC) and the range check does not deliver its in-level
//                  bytes, which no fix-up repairs (measured: keypoints at (20, 19) got wrong descriptors).
//   kPatchBytes    the rest (level 0 is the caller's image, with no room around it to read past): reflect-101 bytes.
enum { kPatchDma = 0, kPatchBufDma = 1, kPatchBytes = 2 };
__device__ __forceinline__ int desc_patch_path(int l, int cx, int cy, int w, int h, int pitch)
{
    if (cx >= 21 && cy >= 21 && cy + 21 < h && (cx + 31 <= w || (cx + 21 < w && cy + 22 < h))) return kPatchDma;
    if (l > 0 && pitch - w >= 16 && !(cx < 21 && cy <= 21)) return kPatchBufDma;
    return kPatchBytes;
}
#ifndef ORBX_DESC_WPE
#define ORBX_DESC_WPE 1
#endif
// kBM: ORBX_BLUR_* (the kernel taps; ORBX_BLUR_SSE2 also rounds the column pass half to even on the level's
// columns below w & ~3, as SymmColumnVec_32s8u does)
template <int kBM>
__global__ __launch_bounds__(64 * kDescWaves, ORBX_DESC_WPE) void k_describe(const Geometry* __restrict__ G, FramePtrs P,
                                               const uint32_t* __restrict__ qt_out,
                                               const int* __restrict__ qt_cnt,
                                               orbx_keypoint* __restrict__ kps, uint8_t* __restrict__ desc,
                                               int cap, int* __restrict__ status, int kpw)
{
    __shared__ __attribute__((aligned(16))) uint32_t s_raw[kDescWaves][kRawSlots];
    __shared__ __attribute__((aligned(16))) uint32_t s_rowT[kDescWaves][kTCols * kTP];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;   // wave: uniform (SGPR)
    const int lb = xcd_block(blockIdx.x + blockIdx.y * gridDim.x, gridDim.x * gridDim.y);
    const int f = lb / gridDim.x, bx = lb - f * gridDim.x;
    const int L = G->nlevels;
    const uint32_t kxb = (uint32_t)__builtin_amdgcn_readfirstlane(G->kp_xbits);   // packed keypoint x width
    const int* cnts = qt_cnt + (size_t)f * L;
    uint32_t* raw32 = s_raw[wave];
    uint8_t* raw = (uint8_t*)raw32;
    uint32_t* rowT = s_rowT[wave];
    const int g0 = (bx * kDescWaves + wave) * kpw;

    // ---- keypoint-independent lane state (c_desc_lanes), loaded once for the wave's keypoints ----
    const int icv = lane >> 1, ich = lane & 1;
    const int vrow = icv - 15;
    const DescLane& DL = c_desc_lanes.l[lane];
    uint32_t W1[4], W0[4];
    float ppx[kDescSlots], ppy[kDescSlots];
    uint32_t rdo[8];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        W1[k] = DL.w1[k];
        W0[k] = DL.w0[k];
    }
#pragma unroll
    for (int q = 0; q < kDescSlots; ++q) {
        ppx[q] = DL.upx[q];
        ppy[q] = DL.upy[q];
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) rdo[q] = DL.rd[q];
    const int ic_row = 21 + vrow, ic_col = ich ? 22 : 6;   // raw row, patch column of the first pixel
    int bitem[3];
#pragma unroll
    for (int it = 0; it < 3; ++it) bitem[it] = c_blur_items[lane + 64 * it];

    // output index g (level-major, as the reference concatenates levels) -> level, keypoint: lane j < kpw
    // looks up the wave's keypoint j once, up front, so no keypoint waits for its packed entry's global load
    // before its patch DMA can go out.  The wave's indices are consecutive, so past the frame's total (or
    // the output capacity) the rest are too, and the valid lanes are a prefix.
    int my_l = 0;
    uint32_t my_pk = 0;
    bool my_ok = false;
    if (lane < kpw) {
        const int g = g0 + lane;
        int base = 0, l = 0;
        for (; l < L; ++l) {
            if (g < base + cnts[l]) break;
            base += cnts[l];
        }
        if (l < L) {
            if (g >= cap) {
                atomicOr(status, (int)kStatusCapOverflow);
            } else {
                my_ok = true;
                my_l = l;
                my_pk = qt_out[(size_t)f * G->out_per_frame + G->lv[l].out_off + (g - base)];
            }
        }
    }
    const int nkp = __builtin_popcountll(__ballot(my_ok));
    auto lookup = [&](int jj, int& l, uint32_t& pk) -> bool {
        if (jj >= nkp) return false;
        l = __builtin_amdgcn_readlane(my_l, jj);
        pk = (uint32_t)__builtin_amdgcn_readlane((int)my_pk, jj);
        return true;
    };
    // raw patch rows cy-21..cy+21 from column cx-21 (48 bytes used per row); sets the
    // wave-uniform row-shift state: row r starts at byte (sb + r*sp) & 3 of its LDS row
    // the DMA's address registers kept live until the loop-top wait for it, so no later write to them makes
    // the compiler wait for the DMA (a write-after-read on a VMEM source register) before BRIEF
    uint32_t dma_va[3] = {0u, 0u, 0u};
    auto fill = [&](int l, uint32_t pk, int& sb, int& sp) {
        const int cx = (int)kp_x(pk, kxb), cy = (int)kp_y(pk, kxb);
        const int w = G->lv[l].w, h = G->lv[l].h;
        int pitch;
        const uint8_t* img = level_base(P, G, f, l, pitch);
        const int path = desc_patch_path(l, cx, cy, w, h, pitch);
        if (path == kPatchDma) {
            // 16-byte piece c = 64 t + lane of DMA instruction t (global_load_lds_dwordx4: lane L's 16 bytes
            // land at byte 16 L of the instruction's 1 KiB) is piece c % 3 of row c / 3, so three instructions
            // fill rows 0..43 (the third with lanes 0..3 only; row 43 repeats row 42).  Each row's aligned
            // bytes start at or after the 4-byte aligned allocation; a row reads 48 bytes from its aligned
            // start, at most cx + 26 (inside the level row, or in the next row of the same level for the
            // right-border case).  (Round 2: eleven 4-row global_load_lds_dword instructions into 64-byte
            // rows, 2816 B; the 48-byte rows take the wave to 5.6 KB of LDS, 7 waves per SIMD.)
            const uintptr_t s0 = (uintptr_t)(img + (size_t)(cy - 21) * pitch + (cx - 21));
            const uint8_t* ub = (const uint8_t*)(s0 & ~(uintptr_t)3);   // wave-uniform, aligned
            sb = (int)(s0 & 3);
            sp = pitch & 3;
#pragma unroll
            for (int t = 0; t < 3; ++t) {
                const int c = 64 * t + lane, row = c / 3, k = c - 3 * row;
                if (t < 2 || lane < 4) {
                    const uint32_t o = (uint32_t)((sb + min(row, 42) * pitch) & ~3) + 16u * (uint32_t)k;
                    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(ub + o),
                                                     (__attribute__((address_space(3))) void*)(raw32 + 256 * t), 16, 0, 0);
                    dma_va[t] = o;
                }
            }
        } else if (path == kPatchBufDma) {
            // Border keypoints of levels >= 1 (about 5% of KITTI's keypoints, 12% at level 7): the same DMA,
            // through a buffer descriptor over the level's rows (pitch x h bytes of the handle's pyramid block),
            // so that the patch bytes outside the level read as zeros instead of touching memory; the reflect-101
            // bytes are copied in from inside the patch at the loop top.  Offsets of rows above the level wrap to
            // large unsigned values, also out of range.  Every 16-byte piece that holds a pixel the patch uses lies
            // whole inside the descriptor: desc_patch_path keeps away the keypoints for which one would start before
            // it or straddle its end.  What pins this is tests/test_describe_borders.py: the oracle's descriptors at
            // every side and corner this path takes (the last level's bottom-right corner included, whose last pieces
            // reach the descriptor's end), with the row padding and the bytes past the level set to 0x00, 0xFF and
            // 0x5A (orbx_debug_fill_workspace); no probe of the range check itself is relied on.
            const long long s0 = (long long)(cy - 21) * pitch + (cx - 21);
            const uint32_t a0 = (uint32_t)(s0 & ~3ll);
            sb = (int)(s0 & 3);
            sp = pitch & 3;   // 0: pitch = align64(w)
            const __amdgpu_buffer_rsrc_t rs =
                __builtin_amdgcn_make_buffer_rsrc((void*)img, (short)0, pitch * h, 0x00020000);
#pragma unroll
            for (int t = 0; t < 3; ++t) {
                const int c = 64 * t + lane, row = c / 3, k = c - 3 * row;
                if (t < 2 || lane < 4) {
                    const uint32_t o = a0 + (uint32_t)((sb + min(row, 42) * pitch) & ~3) + 16u * (uint32_t)k;
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)(raw32 + 256 * t), 16,
                                                         o, 0, 0, 0);
                    dma_va[t] = o;
                }
            }
        } else {
            sb = 0;
            sp = 0;
            // level-0 border keypoints (the caller's image: no room around it to read past), those of levels
            // with under 16 bytes of row padding and the top-left ones of desc_patch_path: reflect-101 bytes,
            // lane = column (43 of the 48 per row), the column reflection once per lane,
            // the row's per row (wave-uniform), and 11 rows' loads in flight before their LDS stores
            static_assert(kRawRows >= 44, "rows 0..43 filled");
            const uint8_t* col = img + reflect101(cx - 21 + min(lane, 42), w);
            for (int s0 = 0; s0 < 44; s0 += 11) {
                uint8_t v[11];
#pragma unroll
                for (int u = 0; u < 11; ++u) v[u] = col[(size_t)reflect101(cy - 21 + min(s0 + u, 42), h) * pitch];   // row 43 repeats row 42
                if (lane < kRawP) {
#pragma unroll
                    for (int u = 0; u < 11; ++u) raw[(s0 + u) * kRawP + lane] = v[u];
                }
            }
            // (no-op at run time: every byte load above is consumed; it tells the compiler's wait-count pass so,
            // which otherwise waits for the DMA path's loads before BRIEF reuses these registers)
            __builtin_amdgcn_s_waitcnt(0x0F70);
        }
    };

    int nl = 0, sb = 0, sp = 0;
    uint32_t npk = 0;
    bool nvalid = lookup(0, nl, npk);
    if (nvalid) fill(nl, npk, sb, sp);
    // IC_Angle (src/ORBextractor.cc:84-128) of the wave's keypoints up front, from the level images in
    // global memory: a keypoint lies >= 19 px inside its level (FAST's cell windows), so its radius-15 disc
    // never leaves it (lanes 62-63 read row 16 with zero weights).  cv::fastAtan2 and sincosf then run
    // once per wave with lane j on keypoint j, instead of once per keypoint on every lane (the angle was
    // 17% of the launch).  Loads of every keypoint first, then the sums.
    float kp_ang = 0.f, kp_cos = 1.f, kp_sin = 0.f;
    int ic_m10 = 0, ic_m01 = 0;   // lane j: keypoint j's moments
    // (keypoints in groups of 4: one group's 20 row dwords in registers at a time)
    constexpr int kIcGroup = kDescPerWave < 4 ? kDescPerWave : 4;
#pragma unroll 1
    for (int j0 = 0; j0 < kDescPerWave && j0 < nkp; j0 += kIcGroup) {
        uint32_t q[kIcGroup][5], qs[kIcGroup];
#pragma unroll
        for (int ji = 0; ji < kIcGroup; ++ji) {
            const int jj = j0 + ji;
            const int jc = jj < nkp ? jj : nkp - 1;   // wave-uniform
            const int l = __builtin_amdgcn_readlane(my_l, jc);
            const uint32_t pk = (uint32_t)__builtin_amdgcn_readlane((int)my_pk, jc);
            const int cx = (int)kp_x(pk, kxb), cy = (int)kp_y(pk, kxb);
            int pitch;
            const uint8_t* img = level_base(P, G, f, l, pitch);
            const uintptr_t a = (uintptr_t)(img + (size_t)(cy + vrow) * pitch + (cx - 15 + 16 * ich));
            // (as a global pointer: an integer cast loses the address space, and flat loads count against both
            // wait counters)
            const __attribute__((address_space(1))) uint32_t* src =
                (const __attribute__((address_space(1))) uint32_t*)(a & ~(uintptr_t)3);
            qs[ji] = (uint32_t)(a & 3);
#pragma unroll
            for (int k = 0; k < 5; ++k) q[ji][k] = src[k];
        }
        int pv[kIcGroup][2];   // the lane's partial moments of the group's keypoints: (m10, m01)
#pragma unroll
        for (int ji = 0; ji < kIcGroup; ++ji) {
            uint32_t s1 = 0u, s0 = 0u;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t w = __builtin_amdgcn_alignbyte(q[ji][k + 1], q[ji][k], qs[ji]);
                s1 = __builtin_amdgcn_udot4(w, W1[k], s1, false);
                s0 = __builtin_amdgcn_udot4(w, W0[k], s0, false);
            }
            pv[ji][0] = (int)s1 - 16 * (int)s0;
            pv[ji][1] = vrow * (int)s0;
        }
        if constexpr (kIcGroup == 4) {
            // the eight wave sums as one reduce-scatter: v_permlane32_swap and v_permlane16_swap exchange half /
            // quarter waves, so each swap-and-add halves the lanes of two sums at once and packs them into one
            // register; the last 16-lane step is the DPP butterfly of wave_sum.  28 VALU for the group instead of
            // eight wave_sum (64).  Quarters of Q0: (m10 k0, m10 k1, m01 k0, m01 k1); of Q1 the same for k2, k3.
            auto swap_add = [](int a, int b, bool sixteen) {
                const auto r = sixteen ? __builtin_amdgcn_permlane16_swap(a, b, false, false)
                                       : __builtin_amdgcn_permlane32_swap(a, b, false, false);
                return (int)r[0] + (int)r[1];
            };
            auto row_sum = [](int v) {
                v += __builtin_amdgcn_mov_dpp(v, 0xB1, 0xF, 0xF, true);    // quad_perm [1,0,3,2]
                v += __builtin_amdgcn_mov_dpp(v, 0x4E, 0xF, 0xF, true);    // quad_perm [2,3,0,1]
                v += __builtin_amdgcn_mov_dpp(v, 0x141, 0xF, 0xF, true);   // row_half_mirror
                return v + __builtin_amdgcn_mov_dpp(v, 0x140, 0xF, 0xF, true);   // row_mirror
            };
            const int r0 = swap_add(pv[0][0], pv[0][1], false), r1 = swap_add(pv[1][0], pv[1][1], false);
            const int r2 = swap_add(pv[2][0], pv[2][1], false), r3 = swap_add(pv[3][0], pv[3][1], false);
            const int q0 = row_sum(swap_add(r0, r1, true)), q1 = row_sum(swap_add(r2, r3, true));
            const int m10[4] = {__builtin_amdgcn_readlane(q0, 0), __builtin_amdgcn_readlane(q0, 16),
                                __builtin_amdgcn_readlane(q1, 0), __builtin_amdgcn_readlane(q1, 16)};
            const int m01[4] = {__builtin_amdgcn_readlane(q0, 32), __builtin_amdgcn_readlane(q0, 48),
                                __builtin_amdgcn_readlane(q1, 32), __builtin_amdgcn_readlane(q1, 48)};
#pragma unroll
            for (int ji = 0; ji < 4; ++ji)
                if (lane == j0 + ji) {
                    ic_m10 = m10[ji];
                    ic_m01 = m01[ji];
                }
        } else {
#pragma unroll
            for (int ji = 0; ji < kIcGroup; ++ji) {
                const int x10 = wave_sum(pv[ji][0]), x01 = wave_sum(pv[ji][1]);
                if (lane == j0 + ji) {
                    ic_m10 = x10;
                    ic_m01 = x01;
                }
            }
        }
    }
    if (nkp > 0) {
        kp_ang = fast_atan2_deg((float)ic_m01, (float)ic_m10);
        glibc_sincosf_pair(kp_ang * kFactorPI, &kp_sin, &kp_cos);   // (src/ORBextractor.cc:148)
    }
#pragma unroll 1
    for (int jj = 0; jj < kpw && nvalid; ++jj) {
        const int oidx = g0 + jj, l = nl;
        const uint32_t pk = npk;
        const int csb = sb, csp = sp;
        const LevelGeom& LG = G->lv[l];
        const int cx = (int)kp_x(pk, kxb), cy = (int)kp_y(pk, kxb), score = (int)(pk >> 24);
        // this keypoint's DMA has landed.  vmcnt counts loads and stores and retires them in issue order, and
        // the previous keypoint's three output stores (desc dwordx2, cv::KeyPoint dwordx4 + dwordx3) were issued
        // after this DMA: waiting down to 3 leaves their round trip in flight
        // (the builtin, not inline asm: the compiler's wait-count pass sees it, and does not wait again for
        // loads it already covers -- an inline-asm wait is opaque to it; gfx9 simm16: vmcnt[3:0], expcnt[6:4]
        // = 7, lgkmcnt[11:8] = 15, vmcnt[5:4] at [15:14])
        // (also right for jj = 0: the IC_Angle loads issued after the first keypoint's DMA were waited for)
        __builtin_amdgcn_s_waitcnt(0x0F73);   // vmcnt(3)
        asm volatile("" ::"v"(dma_va[0]), "v"(dma_va[1]), "v"(dma_va[2]));
        wave_lds_sync();
        // a level >= 1 border keypoint's patch: reflect-101 (copyMakeBorder's BORDER_REFLECT_101, which
        // GaussianBlur applies at the level's edges) from the bytes inside it, columns first (lane = row), then
        // whole rows (lane = column), so the corners reflect in both directions.  The patch spans level columns
        // cx - 21 .. cx + 21 and rows cy - 21 .. cy + 21 (patch row 43 repeats row 42), and a keypoint lies >= 19 px
        // inside its level, so one reflection reaches every byte.
        // (kPatchBufDma needs l > 0, where LG.pitch is the pitch fill() staged with)
        if (desc_patch_path(l, cx, cy, LG.w, LG.h, LG.pitch) == kPatchBufDma) {
            const int w = LG.w, h = LG.h, x0 = cx - 21, y0 = cy - 21;
            auto at = [&](int r, int c) { return raw + r * kRawP + ((csb + r * csp) & 3) + c; };
            if (x0 < 0 || x0 + 42 >= w) {   // wave-uniform
                if (lane < kRawRows) {
#pragma unroll
                    for (int c = 0; c < 2; ++c)
                        if (x0 + c < 0) *at(lane, c) = *at(lane, -(x0 + c) - x0);
#pragma unroll
                    for (int c = 40; c <= 42; ++c)
                        if (x0 + c >= w) *at(lane, c) = *at(lane, 2 * w - 2 - (x0 + c) - x0);
                }
                wave_lds_sync();
            }
            if (y0 < 0 || y0 + 42 >= h) {   // wave-uniform
                // (cy in [19, h - 20]: only patch rows 0, 1 (above) and 41, 42, 43 (below) can leave the level)
                constexpr int kEdgeRows[5] = {0, 1, 41, 42, 43};
#pragma unroll
                for (int i = 0; i < 5; ++i) {
                    const int r = kEdgeRows[i], Y = y0 + min(r, 42);
                    if (Y >= 0 && Y < h) continue;   // wave-uniform
                    const int rr = (Y < 0 ? -Y : 2 * h - 2 - Y) - y0;
                    if (lane <= 42) *at(r, lane) = *at(rr, lane);
                }
                wave_lds_sync();
            }
        }

        // horizontal 7-tap pass: lane item = (row pair rp, column group cg) -> 2 rows x 4 columns.
        // Output column j of the realigned bytes R0 | R1 | R2 is sum_t w[t] * byte[j + t]: a dot4 of each
        // dword with the kernel shifted by j (zero outside the 7 taps), 10 dot4 per row instead of 8
        // byte-realignments and 8 dot4.
        // (kW[j][d] = blur_wshift(j, d): for the default kernel {18 | 34 << 8 | 49 << 16 | 55 << 24, 49 | 34 << 8 |
        // 18 << 16, 0} for j = 0, and so on)
        constexpr uint32_t kW[4][3] = {
            {blur_wshift(0, 0, kBM), blur_wshift(0, 1, kBM), blur_wshift(0, 2, kBM)},
            {blur_wshift(1, 0, kBM), blur_wshift(1, 1, kBM), blur_wshift(1, 2, kBM)},
            {blur_wshift(2, 0, kBM), blur_wshift(2, 1, kBM), blur_wshift(2, 2, kBM)},
            {blur_wshift(3, 0, kBM), blur_wshift(3, 1, kBM), blur_wshift(3, 2, kBM)}};
        static_assert(kBM != ORBX_BLUR_SCALAR || (kW[0][0] == (18u | 34u << 8 | 49u << 16 | 55u << 24) &&
                                                  kW[3][2] == (34u | 18u << 8)), "row-pass weights");
        // Rows that all start at the same byte shift S (csp == 0: the level pitch is a multiple of 4, or the
        // reflect-101 byte path) skip the realignment: output column j is a dot4 of each raw dword with the
        // kernel shifted by S + j bytes, still 10 dot4 per row (2 or 3 per column) and no alignbyte.
        auto hpass = [&](auto s_tag) {
            constexpr int S = decltype(s_tag)::value;   // -1: per-row shifts
#pragma unroll
            for (int it = 0; it < 3; ++it) {
                if (bitem[it] == 0xFFFF) break;
                const int rp = bitem[it] >> 8, cg = bitem[it] & 0xFF;
                uint32_t o[2][4];
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    const int r = 2 * rp + e;
                    const uint32_t* rr = raw32 + r * (kRawP / 4) + cg;
                    const uint32_t W[4] = {rr[0], rr[1], rr[2], rr[3]};
                    if constexpr (S < 0) {
                        const uint32_t sh = ((uint32_t)csb + __umul24((uint32_t)r, (uint32_t)csp)) & 3u;
                        const uint32_t R[3] = {__builtin_amdgcn_alignbyte(W[1], W[0], sh),
                                               __builtin_amdgcn_alignbyte(W[2], W[1], sh),
                                               __builtin_amdgcn_alignbyte(W[3], W[2], sh)};
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            uint32_t acc = __builtin_amdgcn_udot4(R[0], kW[j][0], 0u, false);
                            acc = __builtin_amdgcn_udot4(R[1], kW[j][1], acc, false);
                            if (j >= 2) acc = __builtin_amdgcn_udot4(R[2], kW[j][2], acc, false);
                            o[e][j] = acc;
                        }
                    } else {
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            uint32_t acc = 0u;
#pragma unroll
                            for (int d = 0; d < 4; ++d) {
                                const uint32_t w = blur_wshift(S + j, d, kBM);   // folds to a constant
                                if (w) acc = __builtin_amdgcn_udot4(W[d], w, acc, false);
                            }
                            o[e][j] = acc;
                        }
                    }
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    rowT[(4 * cg + j) * kTP + rp] = o[0][j] | (o[1][j] << 16);
                }
            }
        };
        if (csp != 0) hpass(std::integral_constant<int, -1>{});
        else if (csb == 0) hpass(std::integral_constant<int, 0>{});
        else if (csb == 1) hpass(std::integral_constant<int, 1>{});
        else if (csb == 2) hpass(std::integral_constant<int, 2>{});
        else hpass(std::integral_constant<int, 3>{});
        wave_lds_sync();   // raw is free: start the next keypoint's patch, it lands under BRIEF
        nvalid = lookup(jj + 1, nl, npk);
        if (nvalid) fill(nl, npk, sb, sp);

        // rBRIEF with the reference's contracted FMAs; blur evaluated at each sample point
        const float angle = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, kp_ang), jj));
        const float a = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, kp_cos), jj));
        const float b = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, kp_sin), jj));
        // GaussianBlur's u8 saturation: min(t0, 255) < min(t1, 255) iff t0 < min(t1, 255)
        const uint32_t cblur = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint32_t*)rowT + kBlurByte0;
        // the lane's distinct sample points blurred, two per packed coordinate evaluation, then written to
        // the u16 sample table over rowT's first 768 bytes (one wave: its LDS reads and writes complete in
        // issue order, so every sample's rowT reads precede the table writes)
        typedef float f2v __attribute__((ext_vector_type(2)));
        // (the magic pair through an opaque scalar move: as a literal the compiler splits BX's packed add into two
        // v_add_f32, VOP3P having no literal operand)
        float mgs = kRoundMagic;
        asm("" : "+s"(mgs));
        const f2v va = {a, a}, vb = {b, b}, mg = {mgs, mgs};
        uint32_t tv[kDescSlots];
#pragma unroll
        for (int q = 0; q < kDescSlots; q += 2) {
            // (v_pk_mul / v_pk_fma / v_pk_add: the same roundings as the scalar statements, two samples per
            // instruction)
            const f2v PX = {ppx[q], ppx[q + 1]}, PY = {ppy[q], ppy[q + 1]};
            const f2v BY = __builtin_elementwise_fma(PX, vb, PY * va) + mg;
            const f2v BX = __builtin_elementwise_fma(PX, va, -(PY * vb)) + mg;
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                uint32_t t = blur_acc<kBM>(cblur, __float_as_uint(BY[e]), __float_as_uint(BX[e]));
                if constexpr (kBM == ORBX_BLUR_SSE2) {
                    // SymmColumnVec_32s8u: _mm_cvtps_epi32 of the exact sum T / 2^16 rounds half to even, so a
                    // tie (T % 2^16 == 2^15, here t = T + 2^15 with t % 2^16 == 0) above an even T >> 16 (t's bit
                    // 16 set) rounds down, on every level column below w & ~3
                    const int xl = cx + (int)(__float_as_uint(BX[e]) - kRoundBits);
                    if ((t & 0x1FFFFu) == 0x10000u && xl < (LG.w & ~3)) t -= 0x10000u;
                }
                tv[q + e] = t;
            }
        }
        uint16_t* const stab = (uint16_t*)rowT;
#pragma unroll
        for (int q = 0; q < kDescSlots; ++q) stab[64 * q + lane] = (uint16_t)(tv[q] >> 16);
        wave_lds_sync();
        unsigned long long words[4];
#pragma unroll
        for (int wd = 0; wd < 4; ++wd) {
            const uint32_t t0 = *(const uint16_t*)((const uint8_t*)stab + rdo[2 * wd]);
            const uint32_t t1 = *(const uint16_t*)((const uint8_t*)stab + rdo[2 * wd + 1]);
            words[wd] = __ballot(t0 < (t1 < 255u ? t1 : 255u));
        }
        {   // A/B knob: per-keypoint stores (round 2)
            const size_t o = (size_t)f * cap + oidx;
            if (lane < 4) reinterpret_cast<unsigned long long*>(desc + o * 32)[lane] = words[lane];
            if (lane == 0) {
                float x = (float)cx, y = (float)cy;
                if (l != 0) {
                    x *= LG.scale;
                    y *= LG.scale;
                }
                orbx_keypoint k;
                k.x = x;
                k.y = y;
                k.size = LG.patch_size;
                k.angle = angle;
                k.response = (float)score;
                k.octave = l;
                k.class_id = -1;
                kps[o] = k;
            }
        }
        wave_lds_sync();   // rowT is rewritten by the next keypoint
    }
}

void launch_describe(const Geometry& g, const ExtractBufs& b, const FramePtrs& p, orbx_keypoint* kps,
                     uint8_t* desc, int cap, int batch, hipStream_t s)
{
    // small batches (the per-frame host path) are latency-bound: one keypoint per wave
    const int kpw = batch <= kLatencyMaxBatch ? 1 : kDescPerWave;
    dim3 grid((g.out_per_frame + kDescWaves * kpw - 1) / (kDescWaves * kpw), batch);
    if (b.blur_mode == ORBX_BLUR_SSE2)
        hipLaunchKernelGGL(k_describe<ORBX_BLUR_SSE2>, grid, dim3(64 * kDescWaves), 0, s, b.geom, p, b.qt_out, b.qt_cnt,
                           kps, desc, cap, b.status, kpw);
    else if (b.blur_mode == ORBX_BLUR_BITEXACT)
        hipLaunchKernelGGL(k_describe<ORBX_BLUR_BITEXACT>, grid, dim3(64 * kDescWaves), 0, s, b.geom, p, b.qt_out,
                           b.qt_cnt, kps, desc, cap, b.status, kpw);
    else
        hipLaunchKernelGGL(k_describe<ORBX_BLUR_SCALAR>, grid, dim3(64 * kDescWaves), 0, s, b.geom, p, b.qt_out,
                           b.qt_cnt, kps, desc, cap, b.status, kpw);
}

}  // namespace orbx

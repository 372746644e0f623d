// Device helpers shared by the kernels of liborbx, one copy each: wave-level LDS ordering and reductions,
// pyramid level addressing, 256-bit Hamming distance and the matchers' rotation-consistency check.
#pragma once
#include <hip/hip_runtime.h>

#include "orbx_kernels.hpp"

namespace orbx {

// orders this wave's LDS accesses (a wave-level barrier for data exchanged through LDS)
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The dynamic LDS of a kernel without static LDS, as the constant address 0.  An extern __shared__ array's
// address is a symbol the compiler adds to every LDS address it forms from a runtime offset (one v_add of 0
// each, and registers to hold the sums: k_quadtree<256,4> and <512,16> spilled 16 and 8 bytes per lane to
// scratch with it).  The backend lowers __builtin_amdgcn_groupstaticsize (the static LDS size) to a
// constant, so base plus offset folds into the instructions; the check below costs one scalar compare of
// two constants per wave.
__device__ __forceinline__ uint8_t* dyn_lds()
{
    const uint32_t base = __builtin_amdgcn_groupstaticsize();
    if (base != 0u) __builtin_trap();   // a kernel with static LDS would need the rounded offset and a larger launch size
    return (uint8_t*)(__attribute__((address_space(3))) uint8_t*)(uintptr_t)base;
}

// the number of set bits of mask below this lane
__device__ __forceinline__ int lanes_below(unsigned long long mask)
{
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32),
                                          __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// level l of frame f: level 0 is the caller's image, levels >= 1 live in the pyramid block
__device__ __forceinline__ const uint8_t* level_base(const FramePtrs& P, const Geometry* G, int f, int l,
                                                     int& pitch)
{
    if (l == 0) {
        pitch = P.in_pitch;
        return P.in + (size_t)f * P.in_fstride;
    }
    pitch = G->lv[l].pitch;
    return P.pyr + (size_t)f * P.pyr_fstride + G->lv[l].pyr_off;
}

typedef unsigned short ushort2_t __attribute__((ext_vector_type(2)));

__device__ __forceinline__ ushort2_t as_us2(uint32_t v)
{
    ushort2_t r;
    r.x = (unsigned short)(v & 0xFFFF);
    r.y = (unsigned short)(v >> 16);
    return r;
}

// BORDER_REFLECT_101 index inside the 19-px pad of a level (ComputePyramid :1350-1373)
__device__ __forceinline__ int reflect101(int p, int len)
{
    if (len == 1) return 0;
    while (p < 0 || p >= len) p = p < 0 ? -p : 2 * len - 2 - p;
    return p;
}

// 256-bit Hamming distance of descriptors held as two 16-byte halves: popcount(a ^ b), identical to the
// reference's 8 x u32 SWAR DescriptorDistance (src/ORBmatcher.cc:1728-1744)
__device__ __forceinline__ int ham256(const uint4& a0, const uint4& a1, const uint4& b0, const uint4& b1)
{
    return __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) +
           __popc(a1.x ^ b1.x) + __popc(a1.y ^ b1.y) + __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
}

__device__ __forceinline__ int ham256(const ulonglong2& a0, const ulonglong2& a1, const ulonglong2& b0,
                                      const ulonglong2& b1)
{
    return __popcll(a0.x ^ b0.x) + __popcll(a0.y ^ b0.y) + __popcll(a1.x ^ b1.x) + __popcll(a1.y ^ b1.y);
}

// ---- wave reductions; every one needs all 64 lanes active.  wave_sum and wave_min_full: row (16-lane)
// reductions with DPP permutations, then the four rows by readlane (no LDS round trips) ----
__device__ __forceinline__ int wave_sum(int v)
{
    v += __builtin_amdgcn_mov_dpp(v, 0xB1, 0xF, 0xF, true);    // quad_perm [1,0,3,2]
    v += __builtin_amdgcn_mov_dpp(v, 0x4E, 0xF, 0xF, true);    // quad_perm [2,3,0,1]
    v += __builtin_amdgcn_mov_dpp(v, 0x141, 0xF, 0xF, true);   // row_half_mirror
    v += __builtin_amdgcn_mov_dpp(v, 0x140, 0xF, 0xF, true);   // row_mirror
    return __builtin_amdgcn_readlane(v, 0) + __builtin_amdgcn_readlane(v, 16) +
           __builtin_amdgcn_readlane(v, 32) + __builtin_amdgcn_readlane(v, 48);
}

__device__ __forceinline__ uint32_t wave_min_full(uint32_t v)
{
    v = min(v, (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xF, 0xF, true));    // quad_perm [1,0,3,2]
    v = min(v, (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x4E, 0xF, 0xF, true));    // quad_perm [2,3,0,1]
    v = min(v, (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x141, 0xF, 0xF, true));   // row_half_mirror
    v = min(v, (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x140, 0xF, 0xF, true));   // row_mirror
    const uint32_t a = (uint32_t)__builtin_amdgcn_readlane((int)v, 0);
    const uint32_t b = (uint32_t)__builtin_amdgcn_readlane((int)v, 16);
    const uint32_t c = (uint32_t)__builtin_amdgcn_readlane((int)v, 32);
    const uint32_t d = (uint32_t)__builtin_amdgcn_readlane((int)v, 48);
    return min(min(a, b), min(c, d));
}

// u64 min by butterfly shuffles
__device__ __forceinline__ unsigned long long wave_min_shfl(unsigned long long v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long y = __shfl_xor(v, o);
        v = y < v ? y : v;
    }
    return v;
}

// ---- the matchers' rotation-consistency check (rotHist, HISTO_LENGTH = 30) ----
constexpr int kHisto = 30;

// bin of the angle difference a1 - a2 (degrees): round(rot / HISTO_LENGTH), as the reference's
// factor = 1 / HISTO_LENGTH (bins 0..12 used)
__device__ __forceinline__ int rot_bin(float a1, float a2)
{
    const float factor = 1.0f / kHisto;
    float rot = a1 - a2;
    if (rot < 0.0f) rot += 360.0f;
    int bin = (int)roundf(rot * factor);
    if (bin == kHisto) bin = 0;
    return bin;
}

// ComputeThreeMaxima (src/ORBmatcher.cc:1679-1723): the three fullest bins of hist[kHisto], -1 where a bin
// is empty or (ind2, ind3) holds less than 0.1 of the fullest
__device__ __forceinline__ void three_maxima(const int* hist, int& ind1, int& ind2, int& ind3)
{
    int i1 = -1, i2 = -1, i3 = -1, max1 = 0, max2 = 0, max3 = 0;   // locals: updated through the references they stay in scratch
    for (int i = 0; i < kHisto; ++i) {
        const int s = hist[i];
        if (s > max1) { max3 = max2; max2 = max1; max1 = s; i3 = i2; i2 = i1; i1 = i; }
        else if (s > max2) { max3 = max2; max2 = s; i3 = i2; i2 = i; }
        else if (s > max3) { max3 = s; i3 = i; }
    }
    if ((float)max2 < 0.1f * (float)max1) { i2 = -1; i3 = -1; }
    else if ((float)max3 < 0.1f * (float)max1) { i3 = -1; }
    ind1 = i1;
    ind2 = i2;
    ind3 = i3;
}

// FRAME_GRID_COLS / FRAME_GRID_ROWS (include/Frame.h:37-38): the feature grid of the window searches
constexpr int kFrameGridCols = 64, kFrameGridRows = 48;

// ---- camera pose arithmetic of the pose-projection searches (orbx_proj.hip) and Frame::isInFrustum
// (orbx_frame.hip): oracle/orbref.c proj_* operation for operation ----
__device__ __forceinline__ int ps_x86_int(double v)   // cvttsd2si: NaN / out of range -> INT_MIN
{
    return (v >= -2147483648.0 && v < 2147483648.0) ? (int)v : (-2147483647 - 1);
}

__device__ __forceinline__ float ps_row(const float* r, int stride, float x, float y, float z)
{
    return (r[0] * x + r[stride] * y) + r[2 * stride] * z;   // OpenCV 3.x gemm small-matrix order
}

struct PsCam {
    float R[9], t[3], Ow[3];
    int fwd, bwd;
};

__device__ __forceinline__ PsCam ps_camera(int mode, const float* __restrict__ pose, const orbm_pose_params& P)
{
    PsCam c;
    if (mode == ORBM_PROJ_SIM3 || mode == ORBM_FUSE_SIM3) {   // Decompose Scw (:298-303)
        double d = 0.0;
        for (int k = 0; k < 3; ++k) d += (double)pose[k] * (double)pose[k];
        const float scw = (float)__builtin_sqrt(d);
        const float s = (float)(1.0 / (double)scw);
        for (int r = 0; r < 3; ++r) {
            for (int k = 0; k < 3; ++k) c.R[3 * r + k] = pose[4 * r + k] * s + 0.0f;
            c.t[r] = pose[4 * r + 3] * s + 0.0f;
        }
    } else {
        for (int r = 0; r < 3; ++r) {
            for (int k = 0; k < 3; ++k) c.R[3 * r + k] = pose[4 * r + k];
            c.t[r] = pose[4 * r + 3];
        }
    }
    for (int r = 0; r < 3; ++r) c.Ow[r] = -ps_row(c.R + r, 3, c.t[0], c.t[1], c.t[2]);   // -Rcw.t()*tcw
    c.fwd = c.bwd = 0;
    if (mode == ORBM_PROJ_LAST_FRAME) {   // tlc = Rlw*twc+tlw (:1409-1417)
        const float tlc2 = ps_row(pose + 20, 1, c.Ow[0], c.Ow[1], c.Ow[2]) + pose[23];
        c.fwd = tlc2 > P.b && !P.mono;
        c.bwd = -tlc2 > P.b && !P.mono;
    }
    return c;
}

// MapPoint::PredictScale (src/MapPoint.cc:385-417)
__device__ __forceinline__ int ps_predict_scale(float max_dist, float dist, const orbm_pose_params& P)
{
    const float ratio = max_dist / dist;
    int n = ps_x86_int(__builtin_ceil(log((double)ratio) / (double)P.log_scale));
    if (n < 0) n = 0;
    else if (n >= P.nlevels) n = P.nlevels - 1;
    return n;
}

}  // namespace orbx

// gfx950 kernels of the ORB extractor (ORB_SLAM2::ORBextractor::operator(),
// src/ORBextractor.cc:1248-1334).  Integer/bitwise path: no MFMA.
//
//   K1 k_pyramid_level  ComputePyramid, src/ORBextractor.cc:1342-1377
//      k_pyramid_fused  the same for small batches, several levels per launch
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>

#include "orbx_device.hpp"
#include "orbx_kernels.hpp"

namespace orbx {

// ---------------------------------------------------------------------------
// K1: level l from level l-1, cv::resize INTER_LINEAR u8 fixed point
// (11-bit coefficients, 22-bit vertical rounding) — SURVEY.md A.2.
// Coefficient tables are built on the host exactly like OpenCV builds them.
// ---------------------------------------------------------------------------
#ifndef ORBX_PYR_ROWS
#define ORBX_PYR_ROWS 12   // output rows per block (round 4, 768-frame steps: 12 -> 267.8k / 267.9k against 8 ->
                           // 265.6k / 266.1k frames/s on one box, launches within 2 us of each other; 16 -> 267.0k)
#endif
#ifndef ORBX_PYR_NT
#define ORBX_PYR_NT 256
#endif
constexpr int kPyrRows = ORBX_PYR_ROWS;
constexpr int kPyrNT = ORBX_PYR_NT;   // threads per pyramid workgroup

// SURVEY.md A.2's SSE2 vertical pass (ORBX_RESIZE_SSE2): VResizeLinearVec_32s8u's
// ((mulhi16(h0 >> 4, b0) + mulhi16(h1 >> 4, b1) + 2) >> 2) of the horizontal sums h0, h1 (h >> 4 <= 32640 and
// b <= 2048 are non-negative: mulhi16 is the plain (x * b) >> 16, every product a 24 x 24-bit multiply)
__device__ __forceinline__ uint32_t rz_sse2(uint32_t h0, uint32_t h1, uint32_t b0, uint32_t b1)
{
    const uint32_t v = ((__umul24(h0 >> 4, b0) >> 16) + (__umul24(h1 >> 4, b1) >> 16) + 2u) >> 2;
    return min(v, 255u);
}

// kA: every staged source row starts 4-byte aligned in LDS (source pitch and base multiples of 4, always
// so for levels >= 1), so a lane's realignment shift is the same on every row.  kRM: ORBX_RESIZE_* (columns
// [0, rz_simd_end) of an ORBX_RESIZE_SSE2 level take rz_sse2; rz_simd_end is a multiple of 4, so a 4-column
// group takes one form)
template <bool kWin, bool kA, int kRM>
__global__ __launch_bounds__(kPyrNT) void k_pyramid_level(const Geometry* __restrict__ G, FramePtrs P, int l,
                                                       const int2* __restrict__ xtab,
                                                       const int2* __restrict__ ytab, int lp)
{
    // A block makes kPyrRows output rows of one frame.  The source rows they need arrive in LDS by
    // LDS-DMA (global_load_lds_dwordx4): row r is the 16-byte aligned run of lp bytes that holds it,
    // at LDS byte r * lp, so its pixel x sits at r * lp + sh_r + x with sh_r = its start address & 15
    // (0 on every row of levels >= 1, whose pitch is a multiple of 64).  A chunk is fetched only if it
    // holds a byte of its row: it then lies in the row's own 16-byte aligned span, which cannot cross a
    // page boundary, so no read leaves the caller's allocation.  (Round 2: aligned dword loads realigned
    // by alignbyte and stored to LDS, about 14 VALU per staged dword.)
    extern __shared__ __attribute__((aligned(16))) uint32_t s_src[];
    const int lb = xcd_block(blockIdx.y + blockIdx.z * gridDim.y, gridDim.y * gridDim.z);
    const int f = lb / gridDim.y, dy0 = (lb - f * gridDim.y) * kPyrRows;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const LevelGeom& D = G->lv[l];
    const int sw = G->lv[l - 1].w;
    const int dyn = min(kPyrRows, D.h - dy0);
    int spitch;
    const uint8_t* src = level_base(P, G, f, l - 1, spitch);
    const int sy0 = ytab[D.ytab_off + dy0].x & 0xFFFF;
    const int sy1 = (int)((uint32_t)ytab[D.ytab_off + dy0 + dyn - 1].x >> 16);
    const int nrows = sy1 - sy0 + 1;
    const int nc = lp >> 4;   // 16-byte chunks per staged row
    const uintptr_t ra = (uintptr_t)src + (size_t)sy0 * spitch;
    const uint8_t* gb = (const uint8_t*)(ra & ~(uintptr_t)15);
    const uint32_t sh0 = (uint32_t)(ra & 15);
    // row r's offset from gb: sh0 + r * spitch; the chunk split uses the float reciprocal of nc
    // ((i + 0.5) / nc sits 0.5 / nc from any integer: exact for i < 2^22)
    const int total = nrows * nc;
    const float inv_nc = 1.0f / (float)nc;
    const int nt = blockDim.x;
    for (int i0 = wave * 64; i0 < total; i0 += nt) {
        const int i = i0 + lane;
        const int r = (int)(((float)i + 0.5f) * inv_nc), c = i - __mul24(r, nc);
        const uint32_t ro = sh0 + __umul24((uint32_t)r, (uint32_t)spitch);
        const uint32_t co = (ro & ~15u) + 16u * (uint32_t)c;
        if (i < total && co < ro + (uint32_t)sw)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(gb + co),
                                             (__attribute__((address_space(3))) void*)(s_src + 4 * i0), 16, 0, 0);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const uint8_t* S = (const uint8_t*)s_src;
    // LDS byte of staged row r's pixel 0 (block-uniform)
    auto rowb = [&](int r) -> uint32_t { return (uint32_t)(r * lp) + ((sh0 + (uint32_t)r * (uint32_t)spitch) & 15u); };
    // a thread owns a group of 4 output columns: their coefficients are loaded once and
    // reused for the block's rows
    const int q = (D.w + 3) >> 2;
    uint8_t* drow0 = P.pyr + (size_t)f * P.pyr_fstride + D.pyr_off + (size_t)dy0 * D.pitch;
    for (int g = threadIdx.x; g < q; g += nt) {
        const int dx0 = g * 4;
        // every product fits a 24 x 24 -> 32-bit multiply (v_mul_u32_u24, full rate; the compiler
        // otherwise emits the quarter-rate v_mul_lo_u32 for h * b).  The two taps keep separate
        // addresses: byte reads at x0 and x0 + 1 merge into an unaligned ds_read_u16, which
        // measured 3.5x slower for the whole kernel.
        int x0[4], x1[4];
        uint32_t a0[4], a1[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int2 xt = xtab[D.xtab_off + min(dx0 + k, D.w - 1)];
            x0[k] = xt.x & 0xFFFF;
            x1[k] = (int)((uint32_t)xt.x >> 16);
            a0[k] = (uint32_t)xt.y & 0xFFFFu;
            a1[k] = (uint32_t)xt.y >> 16;
        }
        if constexpr (kWin) {
            // The group's 8 taps lie in the 8 bytes from x0[0] (LevelGeom::pyr_win, checked on the host):
            // per source row three dword reads, realigned to x0[0] by two alignbytes; each column's tap
            // pair is one v_perm into a u16 pair and one v_dot2_u32_u16 with (a0, a1)
            uint32_t sel[4], ak[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                sel[k] = (uint32_t)(x0[k] - x0[0]) | 0x0C00u | ((uint32_t)(x1[k] - x0[0]) << 16) | 0x0C000000u;
                ak[k] = a0[k] | (a1[k] << 16);
            }
            const uint32_t xo = (uint32_t)x0[0] & ~3u, xw = (uint32_t)x0[0] & 3u;
            auto hrow = [&](int r, uint32_t h[4]) {
                uint32_t A, wo;
                if constexpr (kA) {   // one add per row: the row offset is block-uniform, the shift per lane
                    A = rowb(r) + xo;
                    wo = xw;
                } else {
                    A = rowb(r) + (uint32_t)x0[0];
                    wo = A & 3u;
                    A &= ~3u;
                }
                const uint32_t* qd = (const uint32_t*)(S + A);
                const uint32_t d0 = qd[0], d1 = qd[1], d2 = qd[2];
                const uint32_t e0 = __builtin_amdgcn_alignbyte(d1, d0, wo), e1 = __builtin_amdgcn_alignbyte(d2, d1, wo);
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    h[k] = __builtin_amdgcn_udot2(as_us2(__builtin_amdgcn_perm(e1, e0, sel[k])), as_us2(ak[k]), 0u,
                                                  false);
            };
            // Output rows in order; consecutive rows share a source row (lo(y + 1) == hi(y)) at scale
            // factors up to 2, and that row's horizontal sums are kept instead of recomputed.  The
            // vertical sum is taken x4, (4 (h0 b0 + h1 b1) + 2^23) >> 24 = (h0 b0 + h1 b1 + 2^21) >> 22,
            // so each result is byte 3 of its sum and two v_perm pack four of them; the host checks that
            // the coefficient sums keep 4 * 255 * sum(a) * sum(b) + 2^23 below 2^32, which also makes
            // every result <= 255 (no saturation).
            int cr = -1;
            uint32_t hc[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int rr = 0; rr < kPyrRows; ++rr) {
                if (rr >= dyn) break;
                const int2 yt = ytab[D.ytab_off + dy0 + rr];
                const int lo = (yt.x & 0xFFFF) - sy0, hi = (int)((uint32_t)yt.x >> 16) - sy0;
                const uint32_t b0 = ((uint32_t)yt.y & 0xFFFFu) << 2, b1 = ((uint32_t)yt.y >> 16) << 2;
                uint32_t h0[4], h1[4];
                if (lo == cr) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) h0[k] = hc[k];
                } else {
                    hrow(lo, h0);
                }
                if (hi == lo) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) h1[k] = h0[k];
                } else {
                    hrow(hi, h1);
                }
                uint32_t acc[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    // two v_mad_u32_u24 (the compiler's form is two multiplies and an add3)
                    uint32_t t;
                    asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(t) : "v"(h0[k]), "s"(b0), "v"(1u << 23));
                    asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(acc[k]) : "v"(h1[k]), "s"(b1), "v"(t));
                }
                uint32_t packed = __builtin_amdgcn_perm(acc[1], acc[0], 0x0C0C0703u) |
                                  __builtin_amdgcn_perm(acc[3], acc[2], 0x07030C0Cu);
                if constexpr (kRM == 1) {
                    if (dx0 < D.rz_simd_end) {
                        packed = 0u;
#pragma unroll
                        for (int k = 0; k < 4; ++k) packed |= rz_sse2(h0[k], h1[k], b0 >> 2, b1 >> 2) << (8 * k);
                    }
                }
                *reinterpret_cast<uint32_t*>(drow0 + (size_t)rr * D.pitch + dx0) = packed;
                cr = hi;
#pragma unroll
                for (int k = 0; k < 4; ++k) hc[k] = h1[k];
            }
            continue;
        }
        for (int rr = 0; rr < dyn; ++rr) {
            const int2 yt = ytab[D.ytab_off + dy0 + rr];
            const uint8_t* r0 = S + rowb((yt.x & 0xFFFF) - sy0);
            const uint8_t* r1 = S + rowb((int)((uint32_t)yt.x >> 16) - sy0);
            const uint32_t b0 = (uint32_t)yt.y & 0xFFFFu, b1 = (uint32_t)yt.y >> 16;
            uint32_t packed = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t h0 = __umul24(r0[x0[k]], a0[k]) + __umul24(r0[x1[k]], a1[k]);
                const uint32_t h1 = __umul24(r1[x0[k]], a0[k]) + __umul24(r1[x1[k]], a1[k]);
                const uint32_t v = (kRM == 1 && dx0 < D.rz_simd_end) ? rz_sse2(h0, h1, b0, b1)
                                                                    : (__umul24(h0, b0) + __umul24(h1, b1) + (1u << 21)) >> 22;
                packed |= min(v, 255u) << (8 * k);
            }
            // columns past the level width land in the row's pitch padding (pitch = align64(w))
            *reinterpret_cast<uint32_t*>(drow0 + (size_t)rr * D.pitch + dx0) = packed;
        }
    }
}

// ---------------------------------------------------------------------------
// K1 for small batches (the per-frame host path, batch <= kLatencyMaxBatch): levels s+1..s+n from level s
// in one launch, so a single frame's pyramid is one or two launches instead of a chain of seven (each
// ~4.6 us of launch latency for a 640x480 frame).  Large batches keep one launch per level: there the
// kernel is VALU-bound and the bands' halo rows would add work.
// ---------------------------------------------------------------------------
constexpr int kPyrMaxNT = 512;

constexpr int kPyrChunk = 8;   // output rows per work item (unrolled; their row-table entries loaded up front)

// Rows [e.x, e.y] of level D from the source rows held in LDS (row r of the source level at LDS byte
// (r - sfirst) * slp + ((ssh0 + (r - sfirst) * ssp) & 15)), into LDS (dst, pitch dlp, from row e.x; unless
// `last`) and, for the rows this block owns ([e.z, e.w]), into the level's global image.
__device__ __forceinline__ void pyr_rows(const LevelGeom& Dg, const int2* __restrict__ xtab,
                                         const int2* __restrict__ ytab, const uint8_t* S, int slp, int sfirst,
                                         uint32_t ssh0, uint32_t ssp, uint8_t* dst, int dlp, int4 e, bool last,
                                         uint8_t* gimg, int nt, int split, int wave, int lane, int rm)
{
    // the level's fields in registers: the stores below could alias the geometry as far as the compiler
    // knows, which would reload them after every store
    const int w = Dg.w, pitch = Dg.pitch, xoff = Dg.xtab_off, yoff = Dg.ytab_off, win = Dg.pyr_win;
    const int xs = rm == 1 ? Dg.rz_simd_end : 0;   // ORBX_RESIZE_SSE2 columns (a multiple of 4)
    auto rowb = [&](int r) -> uint32_t {
        const int k = r - sfirst;
        return (uint32_t)(k * slp) + ((ssh0 + (uint32_t)k * ssp) & 15u);
    };
    // work items: (chunk of up to kPyrChunk rows, 4-column group), a wave's 64 groups in one chunk, so
    // every wave walks its rows in lock-step (row tables by scalar loads); on narrow levels the threads
    // beyond the first chunk take further chunks instead of idling
    const int q = (w + 3) >> 2, qp = (q + 63) & ~63;
    const int nrows = e.y - e.x + 1;
    const int nch = max((nrows + kPyrChunk - 1) / kPyrChunk, split ? min(nrows, nt / qp) : 1);
    const int rpc = (nrows + nch - 1) / nch;   // <= kPyrChunk
    const int items = qp * nch;
    for (int w0 = wave * 64; w0 < items; w0 += nt) {
        const int c = w0 / qp;
        const int g = w0 - c * qp + lane;
        const int r0 = e.x + c * rpc, nr = min(e.y - r0 + 1, rpc);
        if (g >= q || nr <= 0) continue;
        const int dx0 = g * 4;
        int2 yt[kPyrChunk];
#pragma unroll
        for (int k = 0; k < kPyrChunk; ++k) yt[k] = ytab[yoff + r0 + min(k, nr - 1)];
        // every product fits a 24 x 24 -> 32-bit multiply (v_mul_u32_u24, full rate; the compiler
        // otherwise emits the quarter-rate v_mul_lo_u32 for h * b).  The two taps keep separate
        // addresses: byte reads at x0 and x0 + 1 merge into an unaligned ds_read_u16, which
        // measured 3.5x slower for the whole kernel.
        int x0[4], x1[4];
        uint32_t a0[4], a1[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int2 xt = xtab[xoff + min(dx0 + k, w - 1)];
            x0[k] = xt.x & 0xFFFF;
            x1[k] = (int)((uint32_t)xt.x >> 16);
            a0[k] = (uint32_t)xt.y & 0xFFFFu;
            a1[k] = (uint32_t)xt.y >> 16;
        }
        auto put = [&](int rr, uint32_t packed) {
            if (!last) *reinterpret_cast<uint32_t*>(dst + (rr - e.x) * dlp + dx0) = packed;
            // columns past the level width land in the row's pitch padding (pitch = align64(w))
            if (rr >= e.z && rr <= e.w) *reinterpret_cast<uint32_t*>(gimg + (size_t)rr * pitch + dx0) = packed;
        };
        if (win) {   // block-uniform
            // The group's 8 taps lie in the 8 bytes from x0[0] (LevelGeom::pyr_win, checked on the host):
            // per source row three dword reads, realigned to x0[0] by two alignbytes; each column's tap
            // pair is one v_perm into a u16 pair and one v_dot2_u32_u16 with (a0, a1)
            uint32_t sel[4], ak[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                sel[k] = (uint32_t)(x0[k] - x0[0]) | 0x0C00u | ((uint32_t)(x1[k] - x0[0]) << 16) | 0x0C000000u;
                ak[k] = a0[k] | (a1[k] << 16);
            }
            auto hrow = [&](int r, uint32_t h[4]) {
                const uint32_t A = rowb(r) + (uint32_t)x0[0];
                const uint32_t* qd = (const uint32_t*)(S + (A & ~3u));
                const uint32_t d0 = qd[0], d1 = qd[1], d2 = qd[2], wo = A & 3u;
                const uint32_t e0 = __builtin_amdgcn_alignbyte(d1, d0, wo), e1 = __builtin_amdgcn_alignbyte(d2, d1, wo);
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    h[k] = __builtin_amdgcn_udot2(as_us2(__builtin_amdgcn_perm(e1, e0, sel[k])), as_us2(ak[k]), 0u,
                                                  false);
            };
            // Output rows in order; consecutive rows share a source row (lo(y + 1) == hi(y)) at scale
            // factors up to 2, and that row's horizontal sums are kept instead of recomputed.  The
            // vertical sum is taken x4, (4 (h0 b0 + h1 b1) + 2^23) >> 24 = (h0 b0 + h1 b1 + 2^21) >> 22,
            // so each result is byte 3 of its sum and two v_perm pack four of them; the host checks that
            // the coefficient sums keep 4 * 255 * sum(a) * sum(b) + 2^23 below 2^32, which also makes
            // every result <= 255 (no saturation).
            int cr = -1;
            uint32_t hc[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int k = 0; k < kPyrChunk; ++k) {
                if (k >= nr) break;
                const int lo = yt[k].x & 0xFFFF, hi = (int)((uint32_t)yt[k].x >> 16);
                const uint32_t b0 = ((uint32_t)yt[k].y & 0xFFFFu) << 2, b1 = ((uint32_t)yt[k].y >> 16) << 2;
                uint32_t h0[4], h1[4];
                if (lo == cr) {
#pragma unroll
                    for (int t = 0; t < 4; ++t) h0[t] = hc[t];
                } else {
                    hrow(lo, h0);
                }
                if (hi == lo) {
#pragma unroll
                    for (int t = 0; t < 4; ++t) h1[t] = h0[t];
                } else {
                    hrow(hi, h1);
                }
                uint32_t acc[4];
#pragma unroll
                for (int t = 0; t < 4; ++t) acc[t] = __umul24(h1[t], b1) + (__umul24(h0[t], b0) + (1u << 23));
                uint32_t packed = __builtin_amdgcn_perm(acc[1], acc[0], 0x0C0C0703u) |
                                  __builtin_amdgcn_perm(acc[3], acc[2], 0x07030C0Cu);
                if (dx0 < xs) {
                    packed = 0u;
#pragma unroll
                    for (int t = 0; t < 4; ++t) packed |= rz_sse2(h0[t], h1[t], b0 >> 2, b1 >> 2) << (8 * t);
                }
                put(r0 + k, packed);
                cr = hi;
#pragma unroll
                for (int t = 0; t < 4; ++t) hc[t] = h1[t];
            }
        } else {
#pragma unroll
            for (int k = 0; k < kPyrChunk; ++k) {
                if (k >= nr) break;
                const uint8_t* p0 = S + rowb(yt[k].x & 0xFFFF);
                const uint8_t* p1 = S + rowb((int)((uint32_t)yt[k].x >> 16));
                const uint32_t b0 = (uint32_t)yt[k].y & 0xFFFFu, b1 = (uint32_t)yt[k].y >> 16;
                uint32_t packed = 0;
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const uint32_t h0 = __umul24(p0[x0[t]], a0[t]) + __umul24(p0[x1[t]], a1[t]);
                    const uint32_t h1 = __umul24(p1[x0[t]], a0[t]) + __umul24(p1[x1[t]], a1[t]);
                    const uint32_t v = dx0 < xs ? rz_sse2(h0, h1, b0, b1) : (__umul24(h0, b0) + __umul24(h1, b1) + (1u << 21)) >> 22;
                    packed |= min(v, 255u) << (8 * t);
                }
                put(r0 + k, packed);
            }
        }
    }
}

// One block per (frame, band): a band is `rows` rows of the group's last level; its band-table entries
// (Geometry::pg, pyr_plan) name the rows of every level of the group it computes and the rows it owns.
// Level s's rows arrive in LDS by LDS-DMA (global_load_lds_dwordx4 of the 16-byte chunks that hold each
// row, so row r sits at LDS byte r * lp + sh_r with sh_r = its start address & 15; 0 for levels >= 1,
// whose pitch is a multiple of 64).  A chunk is fetched only if it holds a byte of its row: it then lies
// in the row's own 16-byte aligned span, which cannot cross a page boundary, so no read leaves the
// caller's allocation.  Levels s+1 .. s+n-1 stay in LDS (two row buffers) for the next level, and each
// block writes the rows it owns to the pyramid.  Blocks recompute the few rows their neighbours share
// (about one per level at each band edge) instead of synchronising.
__global__ __launch_bounds__(kPyrMaxNT) void k_pyramid_fused(const Geometry* __restrict__ G, FramePtrs P, int gi,
                                                    const int2* __restrict__ xtab, const int2* __restrict__ ytab,
                                                    const int4* __restrict__ bands, int rm)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t s_src[];
    const PyrGroup& PG = G->pg[gi];
    const int nt = blockDim.x;
    const int lb = xcd_block(blockIdx.y + blockIdx.z * gridDim.y, gridDim.y * gridDim.z);
    const int f = lb / gridDim.y, band = lb - f * gridDim.y;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int s = PG.s, n = PG.n;
    const int4* B = bands + PG.bt_off + (size_t)band * (n + 1);
    const int4 e0 = B[0];
    const int sw = G->lv[s].w;
    int spitch;
    const uint8_t* src = level_base(P, G, f, s, spitch);
    const int lp0 = ((sw + 30) >> 4) << 4;   // the 16-byte chunks spanning a row at any start alignment
    const int nc = lp0 >> 4;
    const uintptr_t ra = (uintptr_t)src + (size_t)e0.x * spitch;
    const uint8_t* gb = (const uint8_t*)(ra & ~(uintptr_t)15);
    const uint32_t sh0 = (uint32_t)(ra & 15);
    // row r's offset from gb: sh0 + r * spitch; the chunk split uses the float reciprocal of nc
    // ((i + 0.5) / nc sits 0.5 / nc from any integer: exact for i < 2^22)
    const int total = (e0.y - e0.x + 1) * nc;
    const float inv_nc = 1.0f / (float)nc;
    for (int i0 = wave * 64; i0 < total; i0 += nt) {
        const int i = i0 + lane;
        const int r = (int)(((float)i + 0.5f) * inv_nc), c = i - __mul24(r, nc);
        const uint32_t ro = sh0 + __umul24((uint32_t)r, (uint32_t)spitch);
        const uint32_t co = (ro & ~15u) + 16u * (uint32_t)c;
        if (i < total && co < ro + (uint32_t)sw)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(gb + co),
                                             (__attribute__((address_space(3))) void*)(s_src + 4 * i0), 16, 0, 0);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    uint8_t* X = (uint8_t*)s_src;
    uint8_t* Y = X + PG.lds_x;
    const uint8_t* S = X;
    int slp = lp0, sfirst = e0.x;
    uint32_t ssh0 = sh0, ssp = (uint32_t)spitch;
    for (int i = 1; i <= n; ++i) {
        const LevelGeom& D = G->lv[s + i];
        const int4 e = B[i];
        const bool last = i == n;
        uint8_t* dst = (i & 1) ? Y : X;
        const int dlp = ((D.w + 15) >> 4) << 4;
        uint8_t* gimg = P.pyr + (size_t)f * P.pyr_fstride + D.pyr_off;
        pyr_rows(D, xtab, ytab, S, slp, sfirst, ssh0, ssp, dst, dlp, e, last, gimg, nt, PG.split, wave, lane, rm);
        if (last) break;
        __syncthreads();   // level s+i is whole in LDS; the buffer it was made from is free
        S = dst;
        slp = dlp;
        sfirst = e.x;
        ssh0 = 0;
        ssp = 0;
    }
}

bool pyr_plan(Geometry& g, const Tap* yt, std::vector<int4>& bands)
{
    bands.clear();
    g.pyr_ngroups = 0;
    if (g.nlevels < 2) return true;
    // ORBX_PYR_FUSED=0: per-level launches for every batch (tested against the oracle,
    // tests/test_gpu_parity.py test_pyramid_per_level_launches_small_batch)
    if (const char* v = getenv("ORBX_PYR_FUSED"))
        if (atoi(v) == 0) return true;
    // group starts (first computed level of each launch): levels 1-3 from level 0, 4-7 from level 3 (640x480
    // host path: 0.147 against 0.150-0.156 ms for 1 or 3 launches); bands of 4 rows of a group's last level
    std::vector<int> st = {1};
    if (4 < g.nlevels) st.push_back(4);
    const int R = 4;
    auto lo = [&](int j, int y) { return yt[g.lv[j].ytab_off + y].x & 0xFFFF; };
    auto hi = [&](int j, int y) { return (int)((uint32_t)yt[g.lv[j].ytab_off + y].x >> 16); };
    auto lds_pitch = [&](int j, bool staged) { return staged ? ((g.lv[j].w + 30) >> 4) << 4 : ((g.lv[j].w + 15) >> 4) << 4; };
    for (size_t gi = 0; gi < st.size(); ++gi) {
        const int s = st[gi] - 1, b = gi + 1 < st.size() ? st[gi + 1] - 1 : g.nlevels - 1, n = b - s;
        const int K = (g.lv[b].h + R - 1) / R;
        // start[j - s][k]: first row of level j owned by band k (k = K: the level height)
        std::vector<std::vector<int>> start(n + 1, std::vector<int>(K + 1));
        for (int k = 0; k <= K; ++k) start[n][k] = std::min(k * R, g.lv[b].h);
        for (int j = b - 1; j > s; --j) {
            start[j - s][0] = 0;
            start[j - s][K] = g.lv[j].h;
            for (int k = 1; k < K; ++k) start[j - s][k] = std::max(start[j - s][k - 1], lo(j + 1, start[j + 1 - s][k]));
        }
        PyrGroup& P = g.pg[g.pyr_ngroups];
        P.s = s;
        P.n = n;
        P.rows = R;
        P.nbands = K;
        P.bt_off = (int)bands.size();
        P.lds_x = P.lds_y = 0;
        int qmax = 0;
        for (int j = s + 1; j <= b; ++j) qmax = std::max(qmax, (g.lv[j].w + 3) >> 2);
        P.nt = qmax > 256 ? std::min(kPyrMaxNT, (qmax + 63) & ~63) : 256;
        P.split = 1;
        std::vector<int4> e(n + 1);
        for (int k = 0; k < K; ++k) {
            e[n] = make_int4(start[n][k], start[n][k + 1] - 1, start[n][k], start[n][k + 1] - 1);
            for (int j = b - 1; j > s; --j) {
                const int of = start[j - s][k], ol = start[j - s][k + 1] - 1;
                int f0 = lo(j + 1, e[j + 1 - s].x), l0 = hi(j + 1, e[j + 1 - s].y);
                if (of <= ol) {
                    f0 = std::min(f0, of);
                    l0 = std::max(l0, ol);
                }
                e[j - s] = make_int4(f0, l0, of, ol);
            }
            e[0] = make_int4(lo(s + 1, e[1].x), hi(s + 1, e[1].y), 0, -1);
            for (int i = 0; i <= n; ++i) {
                if (e[i].y < e[i].x) {   // (cannot happen for a shrinking pyramid) per-level launches
                    g.pyr_ngroups = 0;
                    bands.clear();
                    return true;
                }
                const int bytes = (e[i].y - e[i].x + 1) * lds_pitch(s + i, i == 0);
                if (i % 2 == 0) P.lds_x = std::max(P.lds_x, bytes);
                else if (i < n) P.lds_y = std::max(P.lds_y, bytes);
            }
            bands.insert(bands.end(), e.begin(), e.end());
        }
        // + 16 bytes: the window path's third dword of a group at the end of the last row; a group whose rows
        // outgrow a workgroup's LDS (very wide images) leaves the small-batch path on the per-level launches
        if (P.lds_x + P.lds_y + 16 > 160 * 1024) {
            g.pyr_ngroups = 0;
            bands.clear();
            return true;
        }
        ++g.pyr_ngroups;
    }
    return true;
}

// k_pyramid_level's LDS row pitch for level l: the 16-byte chunks spanning a source row at any start alignment
static int pyr_lds_pitch(const Geometry& g, int l) { return ((g.lv[l - 1].w + 15 + 15) >> 4) << 4; }

size_t pyr_level_lds(const Geometry& g, int l)
{
    // source rows per block: kPyrRows * (src/dst scale) + 2, bounded by the level ratio; + 16 bytes: the
    // window path's third dword of a group at the end of the last row
    const int srows = (kPyrRows * g.lv[l - 1].h + g.lv[l].h - 1) / g.lv[l].h + 2;
    return (size_t)srows * pyr_lds_pitch(g, l) + 16;
}

PyrLaunches pyr_launches(const Geometry& g, int batch)
{
    PyrLaunches r = {batch <= kLatencyMaxBatch && g.pyr_ngroups > 0, 0, 0};
    r.n = r.fused ? g.pyr_ngroups : g.nlevels - 1;
    for (int i = 0; i < r.n; ++i) r.srcmask |= 1 << (r.fused ? g.pg[i].s : i);
    return r;
}

void launch_pyramid(const Geometry& g, const ExtractBufs& b, const FramePtrs& p, int batch, hipStream_t s)
{
    const PyrLaunches pl = pyr_launches(g, batch);
    if (pl.fused) {
        for (int i = 0; i < pl.n; ++i) {
            const PyrGroup& P = g.pg[i];
            const size_t smem = (size_t)P.lds_x + P.lds_y + 16;
            if (smem > 64 * 1024)
                hipFuncSetAttribute((const void*)k_pyramid_fused, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
            hipLaunchKernelGGL(k_pyramid_fused, dim3(1, P.nbands, batch), dim3(P.nt), smem, s, b.geom, p, i, b.xtab,
                               b.ytab, b.pyr_bands, b.resize_mode);
        }
        return;
    }
    for (int l = 1; l <= pl.n; ++l) {
        const int h = g.lv[l].h;
        const int lp = pyr_lds_pitch(g, l);
        const size_t smem = pyr_level_lds(g, l);
        dim3 grid(1, (h + kPyrRows - 1) / kPyrRows, batch);
        // a thread per 4-column group: narrow levels take fewer waves per block
        const int q = (g.lv[l].w + 3) >> 2;
        const int nt = std::min(kPyrNT, (q + 63) & ~63);
        const bool al = l >= 2 || (((uintptr_t)p.in | (uintptr_t)p.in_pitch | (uintptr_t)p.in_fstride) & 3) == 0;
        // (levels of images wider than about 4,000 px stage more than the default 64 KiB; ensure_geometry
        // rejects any above the workgroup's 160 KiB, pyr_level_lds)
        auto launch = [&](auto kern) {
            if (smem > 64 * 1024)
                hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
            hipLaunchKernelGGL(kern, grid, dim3(nt), smem, s, b.geom, p, l, b.xtab, b.ytab, lp);
        };
        auto go = [&](auto rm_tag) {
            constexpr int RM = decltype(rm_tag)::value;
            if (g.lv[l].pyr_win && al) launch(k_pyramid_level<true, true, RM>);
            else if (g.lv[l].pyr_win) launch(k_pyramid_level<true, false, RM>);
            else launch(k_pyramid_level<false, false, RM>);
        };
        if (b.resize_mode == ORBX_RESIZE_SSE2) go(std::integral_constant<int, 1>{});
        else go(std::integral_constant<int, 0>{});
    }
}

}  // namespace orbx

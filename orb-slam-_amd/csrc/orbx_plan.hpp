// The extractor's size planner: everything a (params, rows, cols) decides before a kernel planner or the
// device is asked.  Host arithmetic only (no HIP), so a plain C++ program can run it under sanitizers
// (tests/test_geometry_plan.py); restates ORB-SLAM2's level sizes, FAST cell grid and quadtree roots
// (orbx_geom.hpp names the lines).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/orbx.h"
#include "orbx_geom.hpp"

namespace orbx {

inline int cv_round(float v) { return (int)std::lrint(v); }
inline int cv_floor(float v) { int i = (int)v; return i - (i > v); }
inline int cv_ceil(float v) { int i = (int)v; return i + (i < v); }

struct Tables {
    int nlevels = 0;
    float scale[kMaxLevels], inv_scale[kMaxLevels], sigma2[kMaxLevels], inv_sigma2[kMaxLevels];
    int nfeat[kMaxLevels];
    int umax[16];
};

// ORBextractor::ORBextractor, src/ORBextractor.cc:466-540
inline bool make_tables(const orbx_params& p, Tables& t)
{
    if (p.nlevels < 1 || p.nlevels > kMaxLevels || p.nfeatures < 0 || !(p.scale_factor > 1.0f)) return false;
    t.nlevels = p.nlevels;
    const double sf = (double)p.scale_factor;
    t.scale[0] = 1.0f;
    t.sigma2[0] = 1.0f;
    for (int i = 1; i < p.nlevels; i++) {
        t.scale[i] = (float)((double)t.scale[i - 1] * sf);
        t.sigma2[i] = t.scale[i] * t.scale[i];
    }
    for (int i = 0; i < p.nlevels; i++) {
        t.inv_scale[i] = 1.0f / t.scale[i];
        t.inv_sigma2[i] = 1.0f / t.sigma2[i];
    }
    const float factor = (float)(1.0f / sf);
    float desired = (float)p.nfeatures * (1 - factor) / (1 - (float)std::pow((double)factor, (double)p.nlevels));
    int sum = 0;
    for (int l = 0; l < p.nlevels - 1; l++) {
        t.nfeat[l] = cv_round(desired);
        sum += t.nfeat[l];
        desired *= factor;
    }
    t.nfeat[p.nlevels - 1] = std::max(p.nfeatures - sum, 0);
    const int vmax = cv_floor(15 * std::sqrt(2.f) / 2 + 1);
    const int vmin = cv_ceil(15 * std::sqrt(2.f) / 2);
    const double hp2 = 15 * 15;
    for (int v = 0; v <= vmax; ++v) t.umax[v] = (int)std::lrint(std::sqrt(hp2 - v * v));
    for (int v = 15, v0 = 0; v >= vmin; --v) {
        while (t.umax[v0] == t.umax[v0 + 1]) ++v0;
        t.umax[v] = v0;
        ++v0;
    }
    return true;
}

inline short sat_s16(float v)
{
    const int i = cv_round(v);
    return (short)std::min(std::max(i, -32768), 32767);
}

// cv::resize INTER_LINEAR coefficient tables: x: {x0 | x1<<16, a0 | a1<<16},
// y: {y0 | y1<<16, b0 | b1<<16}
inline void resize_tables(int sw, int sh, int dw, int dh, std::vector<Tap>& xt, std::vector<Tap>& yt)
{
    const double inv_scale_x = (double)dw / sw, inv_scale_y = (double)dh / sh;
    const double scale_x = 1. / inv_scale_x, scale_y = 1. / inv_scale_y;
    for (int dx = 0; dx < dw; dx++) {
        float fx = (float)((dx + 0.5) * scale_x - 0.5);
        int sx = cv_floor(fx);
        fx -= sx;
        if (sx < 0) { fx = 0; sx = 0; }
        if (sx >= sw - 1) { fx = 0; sx = sw - 1; }
        const int x1 = sx + 1 < sw ? sx + 1 : sw - 1;
        const int a0 = sat_s16((1.f - fx) * 2048), a1 = sat_s16(fx * 2048);
        xt.push_back(Tap{sx | (x1 << 16), (a0 & 0xFFFF) | (a1 << 16)});
    }
    for (int dy = 0; dy < dh; dy++) {
        float fy = (float)((dy + 0.5) * scale_y - 0.5);
        int sy = cv_floor(fy);
        fy -= sy;
        const int b0 = sat_s16((1.f - fy) * 2048), b1 = sat_s16(fy * 2048);
        const int y0 = std::min(std::max(sy, 0), sh - 1), y1 = std::min(std::max(sy + 1, 0), sh - 1);
        yt.push_back(Tap{y0 | (y1 << 16), (b0 & 0xFFFF) | (b1 << 16)});
    }
}

// What one image size plans on the host: the geometry up to the kernel planners' fields (pyr_plan, fast_groups,
// qt_prepare and the spill sum fill those in, orbx_api.hip ensure_geometry), the cell table and the resize tables
struct FramePlan {
    Geometry geom;
    std::vector<Cell> cells;
    std::vector<Tap> xtab, ytab;
};

inline orbx_status plan_frame(const Tables& t, int ini_th, int min_th, int rows, int cols, FramePlan& plan)
{
    // packed keypoint coordinates (pack_kp): x and y share 24 bits, 12 / 12 up to 4096 x 4096
    auto bits = [](int v) { int b = 0; while ((1 << b) < v) ++b; return b; };
    if (rows <= 0 || cols <= 0 || bits(cols) + bits(rows) > kKpCoordBits) return ORBX_EINVAL;
    plan = FramePlan{};
    Geometry& g = plan.geom;
    std::vector<Cell>& cells = plan.cells;
    std::vector<Tap>& xt = plan.xtab;
    std::vector<Tap>& yt = plan.ytab;
    g.rows = rows;
    g.cols = cols;
    g.nlevels = t.nlevels;
    g.kp_xbits = std::max(bits(cols), std::min(12, kKpCoordBits - bits(rows)));
    g.ini_th = std::min(std::max(ini_th, 0), 255);
    g.min_th = std::min(std::max(min_th, 0), 255);
    std::memcpy(g.umax, t.umax, sizeof(g.umax));
    long long pyr = 0;
    int slot = 0, out = 0, maxcells = 1, lcap = 8;
    int prev_w = cols, prev_h = rows;
    for (int l = 0; l < t.nlevels; ++l) {
        LevelGeom& L = g.lv[l];
        // src/ORBextractor.cc:1347-1348
        L.w = cv_round((float)cols * t.inv_scale[l]);
        L.h = cv_round((float)rows * t.inv_scale[l]);
        L.pitch = (L.w + 63) & ~63;
        if (l > 0) {
            L.pyr_off = pyr;
            pyr += (long long)L.pitch * L.h;
            L.xtab_off = (int)xt.size();
            L.ytab_off = (int)yt.size();
            resize_tables(prev_w, prev_h, L.w, L.h, xt, yt);
            L.rz_simd_end = rz_simd_end(L.w);
            L.pyr_win = 1;
            for (int g0 = 0; g0 < L.w; g0 += 4) {   // k_pyramid_level's byte window per 4-column group
                const int first = xt[L.xtab_off + g0].x & 0xFFFF;
                for (int k = 0; k < 4; ++k) {
                    const int x = xt[L.xtab_off + std::min(g0 + k, L.w - 1)].x;
                    if ((x & 0xFFFF) < first || (x >> 16) - first > 7) L.pyr_win = 0;
                }
            }
            // the window path's x4 vertical sums: 4 * 255 * sum(a) * sum(b) + 2^23 < 2^32 (then every
            // result is <= 255 as well); OpenCV's coefficient pairs sum to 2048, give or take a rounding
            long long sa = 0, sb = 0;
            for (int i = L.xtab_off; i < (int)xt.size(); ++i)
                sa = std::max(sa, (long long)(xt[i].y & 0xFFFF) + ((unsigned)xt[i].y >> 16));
            for (int i = L.ytab_off; i < (int)yt.size(); ++i)
                sb = std::max(sb, (long long)(yt[i].y & 0xFFFF) + ((unsigned)yt[i].y >> 16));
            if (4LL * 255 * sa * sb + (1LL << 23) >= (1LL << 32)) L.pyr_win = 0;
        }
        prev_w = L.w;
        prev_h = L.h;
        // FAST cell grid, src/ORBextractor.cc:932-972
        const int minB = kMinBorder;
        const int maxBX = L.w - kEdge + 3, maxBY = L.h - kEdge + 3;
        const float width = (float)(maxBX - minB), height = (float)(maxBY - minB);
        const int nCols = (int)(width / 30.f), nRows = (int)(height / 30.f);
        if (nCols <= 0 || nRows <= 0) return ORBX_EINVAL;
        const int wCell = (int)std::ceil(width / nCols), hCell = (int)std::ceil(height / nRows);
        L.cell_begin = (int)cells.size();
        L.slot_begin = slot;
        for (int i = 0; i < nRows; i++) {
            const float iniY = (float)(minB + i * hCell);
            float maxY = iniY + hCell + 6;
            if (iniY >= maxBY - 3) continue;
            if (maxY > maxBY) maxY = (float)maxBY;
            for (int j = 0; j < nCols; j++) {
                const float iniX = (float)(minB + j * wCell);
                float maxX = iniX + wCell + 6;
                if (iniX >= maxBX - 6) continue;
                if (maxX > maxBX) maxX = (float)maxBX;
                Cell c{};
                c.level = (int16_t)l;
                c.roi_x0 = (int)iniX;
                c.roi_y0 = (int)iniY;
                c.roi_w = (int16_t)((int)maxX - (int)iniX);
                c.roi_h = (int16_t)((int)maxY - (int)iniY);
                if (c.roi_w > 66 || c.roi_h > 66) return ORBX_EINVAL;
                g.max_roi_w = std::max(g.max_roi_w, (int)c.roi_w);
                g.max_roi_h = std::max(g.max_roi_h, (int)c.roi_h);
                L.roi_mw = std::max(L.roi_mw, (int)c.roi_w);
                L.roi_mh = std::max(L.roi_mh, (int)c.roi_h);
                const int dw = c.roi_w - 6, dh = c.roi_h - 6;
                // a FAST wave's cells (kCellsPerWave consecutive cells of the level) write one run from the
                // first one's slot base: it starts on a 128-byte line, so the quadtree's gather reads whole lines
                if (((int)cells.size() - L.cell_begin) % kCellsPerWave == 0) slot = (slot + 31) & ~31;
                c.slot_base = slot;
                c.slot_cap = (dw > 0 && dh > 0) ? ((dw + 1) / 2) * ((dh + 1) / 2) : 0;
                slot += c.slot_cap;
                cells.push_back(c);
            }
        }
        // empty cells up to a whole number of FAST waves (kCellsPerWave): no wave spans two levels
        while (((int)cells.size() - L.cell_begin) % kCellsPerWave) {
            Cell c{};
            c.level = (int16_t)l;
            c.slot_base = slot;
            cells.push_back(c);
        }
        L.ncells = (int)cells.size() - L.cell_begin;
        L.slot_cap = slot - L.slot_begin;
        maxcells = std::max(maxcells, L.ncells);
        // DistributeOctTree roots, src/ORBextractor.cc:650-653
        L.qw = L.w - 2 * kMinBorder;
        L.qh = L.h - 2 * kMinBorder;
        L.nIni = (int)std::round((float)L.qw / L.qh);
        if (L.nIni <= 0) return ORBX_EINVAL;
        L.hX = (float)L.qw / L.nIni;
        L.nfeat = t.nfeat[l];
        L.cap = std::max(L.nfeat + 2, 4 * L.nIni);
        L.out_off = out;
        out += L.cap;
        lcap = std::max(lcap, L.cap + 4);
        L.scale = t.scale[l];
        L.inv_scale = t.inv_scale[l];
        L.patch_size = (float)(int)(31 * t.scale[l]);   // :1013
    }
    g.ncells = (int)cells.size();
    g.slots_per_frame = (slot + 31) & ~31;   // frames' slot blocks start on 128-byte lines
    g.out_per_frame = out;
    g.max_cells_level = maxcells;
    g.lcap = lcap;
    g.pyr_bytes = (pyr + 255) & ~255LL;
    g.qt_kpt0 = (long long)rows * cols > kQtBigArea ? 24 : 16;
    return ORBX_OK;
}

}  // namespace orbx

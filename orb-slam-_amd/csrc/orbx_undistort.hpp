// cv::undistortPoints(src, dst, K, D, noArray(), K) as Frame::UndistortKeyPoints and
// Frame::ComputeImageBounds call it (src/Frame.cc:562-566, :603): OpenCV 3.x cvUndistortPoints with R = I,
// P = K.  One function for the host entry points and the device kernel (orbx_frame.hip), so both run the same
// source text: all arithmetic in double, no contraction (the library builds with -ffp-contract=off), the
// reciprocal focal lengths multiplied (not divided by), exactly 5 fixed-point iterations.
// Unpinned against a real OpenCV.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/orbx.h"

namespace orbx {

struct UdCam {
    double fx, fy, cx, cy, ifx, ify, k1, k2, p1, p2, k3;
};

// mK and mDistCoef are CV_32F; cvUndistortPoints converts them to double first
__host__ __device__ inline UdCam ud_camera(const orbx_camera& c)
{
    UdCam u;
    u.fx = (double)c.fx;
    u.fy = (double)c.fy;
    u.cx = (double)c.cx;
    u.cy = (double)c.cy;
    u.ifx = 1. / u.fx;
    u.ify = 1. / u.fy;
    u.k1 = (double)c.k1;
    u.k2 = (double)c.k2;
    u.p1 = (double)c.p1;
    u.p2 = (double)c.p2;
    u.k3 = (double)c.k3;
    return u;
}

__host__ __device__ inline void ud_point(const UdCam& c, float xf, float yf, float* xo, float* yo)
{
    double x = ((double)xf - c.cx) * c.ifx;
    double y = ((double)yf - c.cy) * c.ify;
    const double x0 = x, y0 = y;
    for (int j = 0; j < 5; ++j) {
        const double r2 = x * x + y * y;
        const double icdist = 1. / (1 + ((c.k3 * r2 + c.k2) * r2 + c.k1) * r2);
        const double dX = 2 * c.p1 * x * y + c.p2 * (r2 + 2 * x * x);
        const double dY = c.p1 * (r2 + 2 * y * y) + 2 * c.p2 * x * y;
        x = (x0 - dX) * icdist;
        y = (y0 - dY) * icdist;
    }
    // xx = P(0,:) . (x, y, 1), yy = P(1,:) . (x, y, 1), ww = 1 for P = K
    *xo = (float)((c.fx * x + 0. * y) + c.cx);
    *yo = (float)((0. * x + c.fy * y) + c.cy);
}

}  // namespace orbx

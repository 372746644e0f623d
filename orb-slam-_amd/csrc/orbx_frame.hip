// The Frame tail: what the Frame constructors do between the extractor and the matchers
// (src/Frame.cc:145-197, :212-284), and Frame::isInFrustum of Tracking::SearchLocalPoints.  Kernels and their
// C entry points (include/orbx.h).
//
// T1 k_undistort    Frame::UndistortKeyPoints (:539-579): one lane per keypoint, ud_point (orbx_undistort.hpp,
//                   the host entry points' own function) on pt, the other five fields copied
// T2 k_rgbd_stereo  Frame::ComputeStereoFromRGBD (:875-896): one lane per keypoint, one depth pixel each
// T3 k_frustum      Frame::isInFrustum (:342-398): one lane per MapPoint, the camera and PredictScale of the
//                   pose searches (orbx_device.hpp); nToMatch by one ballot and one atomicAdd per wave
// Each is one launch over the whole batch: workgroup b serves frame b / bpf, entries (b % bpf) * 256 ...
// The work is a few dozen bytes and, for T1 / T3, a few hundred double / float operations per lane:
// launch- and latency-bound.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "orbx_device.hpp"
#include "orbx_host.hpp"
#include "orbx_kernels.hpp"
#include "orbx_undistort.hpp"

namespace orbx {

constexpr int kFtBlock = 256;

// d_kps_un may alias d_kps (in place): no __restrict__, each lane reads its keypoint before it writes it
__global__ __launch_bounds__(kFtBlock) void k_undistort(const orbx_keypoint* kps, const int* __restrict__ counts,
                                                        int cap, int bpf, orbx_camera cam, orbx_keypoint* kps_un)
{
    const int f = blockIdx.x / bpf, i = (blockIdx.x - f * bpf) * kFtBlock + threadIdx.x;
    if (i >= min(counts[f], cap)) return;
    const size_t o = (size_t)f * cap + i;
    orbx_keypoint kp = kps[o];
    if (cam.k1 != 0.0f) {   // mDistCoef.at<float>(0)==0.0: mvKeysUn=mvKeys (:543-547)
        const UdCam c = ud_camera(cam);
        ud_point(c, kp.x, kp.y, &kp.x, &kp.y);
    }
    kps_un[o] = kp;
}

__global__ __launch_bounds__(kFtBlock) void k_rgbd_stereo(const orbx_keypoint* __restrict__ kps,
                                                          const orbx_keypoint* __restrict__ kps_un,
                                                          const int* __restrict__ counts, int cap, int bpf,
                                                          const float* __restrict__ depth, int rows, int cols,
                                                          size_t dstep, size_t dfs, float bf,
                                                          float* __restrict__ uright, float* __restrict__ depth_out)
{
    const int f = blockIdx.x / bpf, i = (blockIdx.x - f * bpf) * kFtBlock + threadIdx.x;
    if (i >= min(counts[f], cap)) return;
    const size_t o = (size_t)f * cap + i;
    // imDepth.at<float>(v,u): Mat::at(int, int) through float -> int conversions (cvttss2si)
    const int y = ps_x86_int((double)kps[o].y), x = ps_x86_int((double)kps[o].x);
    float ur = -1.0f, dp = -1.0f;
    if ((unsigned)y < (unsigned)rows && (unsigned)x < (unsigned)cols) {
        const float d = reinterpret_cast<const float*>(reinterpret_cast<const uint8_t*>(depth) + (size_t)f * dfs +
                                                       (size_t)y * dstep)[x];
        if (d > 0) {
            dp = d;
            ur = kps_un[o].x - bf / d;
        }
    }
    uright[o] = ur;
    depth_out[o] = dp;
}

__global__ __launch_bounds__(kFtBlock) void k_frustum(const orbm_map_point* __restrict__ pts,
                                                      const int* __restrict__ npts, int pcap, int bpf,
                                                      const float* __restrict__ pose, orbm_pose_params P, float limit,
                                                      orbm_proj_point* __restrict__ out, int* __restrict__ ninview)
{
    const int f = blockIdx.x / bpf, m = (blockIdx.x - f * bpf) * kFtBlock + threadIdx.x;
    const bool live = m < min(npts[f], pcap);
    bool inview = false;
    if (live) {
        const size_t mo = (size_t)f * pcap + m;
        const orbm_map_point M = pts[mo];
        orbm_proj_point o;
        o.proj_x = o.proj_y = o.proj_xr = o.view_cos = 0.0f;
        o.level = 0;
        o.flags = M.flags & 2;
        if (M.flags & 1) {
            const PsCam c = ps_camera(ORBM_PROJ_KEYFRAME, pose + (size_t)f * 12, P);   // mRcw, mtcw, mOw (:336-339)
            const float X = M.x, Y = M.y, Z = M.z;
            const float PcX = ps_row(c.R, 1, X, Y, Z) + c.t[0];   // mRcw*P+mtcw
            const float PcY = ps_row(c.R + 3, 1, X, Y, Z) + c.t[1];
            const float PcZ = ps_row(c.R + 6, 1, X, Y, Z) + c.t[2];
            do {
                if (PcZ < 0.0f) break;
                const float invz = 1.0f / PcZ;
                const float u = __builtin_fmaf(P.fx * PcX, invz, P.cx);   // fx*PcX*invz+cx
                const float v = __builtin_fmaf(P.fy * PcY, invz, P.cy);
                if (u < P.min_x || u > P.max_x) break;
                if (v < P.min_y || v > P.max_y) break;
                const float maxD = 1.2f * M.max_dist, minD = 0.8f * M.min_dist;
                const float PO0 = X - c.Ow[0], PO1 = Y - c.Ow[1], PO2 = Z - c.Ow[2];
                double s = 0.0;
                s += (double)PO0 * (double)PO0;
                s += (double)PO1 * (double)PO1;
                s += (double)PO2 * (double)PO2;
                const float dist = (float)__builtin_sqrt(s);   // cv::norm(PO)
                if (dist < minD || dist > maxD) break;
                double dot = 0.0;   // PO.dot(Pn)
                dot += (double)PO0 * (double)M.nx;
                dot += (double)PO1 * (double)M.ny;
                dot += (double)PO2 * (double)M.nz;
                const float viewCos = (float)(dot / (double)dist);
                if (viewCos < limit) break;
                o.proj_x = u;
                o.proj_y = v;
                o.proj_xr = __builtin_fmaf(-P.bf, invz, u);   // u - mbf*invz
                o.view_cos = viewCos;
                o.level = ps_predict_scale(M.max_dist, dist, P);
                o.flags |= 1;
                inview = true;
            } while (false);
        }
        out[mo] = o;
    }
    const int n = __popcll(__ballot(inview));
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(&ninview[f], n);
}

namespace {

// workgroups per frame and in all; false when the grid does not fit
bool ft_grid(int nframes, int cap, int* bpf, unsigned* nblocks)
{
    *bpf = (cap + kFtBlock - 1) / kFtBlock;
    const unsigned long long n = (unsigned long long)*bpf * (unsigned long long)nframes;
    *nblocks = (unsigned)n;
    return n <= 0x7FFFFFFFull;
}

}  // namespace

}  // namespace orbx

using namespace orbx;

extern "C" {

orbx_status orbx_undistort_points(const orbx_camera* cam, const float* xy, int n, float* xy_out)
{
    if (!cam || n < 0 || (n > 0 && (!xy || !xy_out))) return ORBX_EINVAL;
    const UdCam c = ud_camera(*cam);
    for (int i = 0; i < n; ++i) ud_point(c, xy[2 * i], xy[2 * i + 1], &xy_out[2 * i], &xy_out[2 * i + 1]);
    return ORBX_OK;
}

orbx_status orbx_image_bounds(const orbx_camera* cam, int rows, int cols, float* bounds)
{
    if (!cam || rows <= 0 || cols <= 0 || !bounds) return ORBX_EINVAL;
    if (cam->k1 != 0.0f) {
        const float w = (float)cols, h = (float)rows;
        float m[8] = {0.0f, 0.0f, w, 0.0f, 0.0f, h, w, h};
        orbx_undistort_points(cam, m, 4, m);
        bounds[0] = std::min(m[0], m[4]);   // :607-610
        bounds[1] = std::max(m[2], m[6]);
        bounds[2] = std::min(m[1], m[3]);
        bounds[3] = std::max(m[5], m[7]);
    } else {
        bounds[0] = 0.0f;
        bounds[1] = (float)cols;
        bounds[2] = 0.0f;
        bounds[3] = (float)rows;
    }
    return ORBX_OK;
}

orbx_status orbx_undistort_batch_device(const orbx_keypoint* d_kps, const int* d_counts, int nframes, int cap,
                                        const orbx_camera* cam, orbx_keypoint* d_kps_un, void* stream)
{
    int bpf;
    unsigned nb;
    if (!d_kps || !d_counts || nframes < 0 || cap <= 0 || !cam || !d_kps_un || !ft_grid(nframes, cap, &bpf, &nb))
        return ORBX_EINVAL;
    if (nframes == 0 || (cam->k1 == 0.0f && d_kps_un == d_kps)) return ORBX_OK;
    hipLaunchKernelGGL(k_undistort, dim3(nb), dim3(kFtBlock), 0, (hipStream_t)stream, d_kps, d_counts, cap, bpf, *cam,
                       d_kps_un);
    return hipGetLastError() == hipSuccess ? ORBX_OK : ORBX_EDEVICE;
}

orbx_status orbx_rgbd_stereo_batch_device(const orbx_keypoint* d_kps, const orbx_keypoint* d_kps_un,
                                          const int* d_counts, int nframes, int cap, const float* d_depth, int rows,
                                          int cols, size_t depth_step, size_t depth_frame_stride, float bf,
                                          float* d_uright, float* d_depth_out, void* stream)
{
    int bpf;
    unsigned nb;
    if (!d_kps || !d_kps_un || !d_counts || nframes < 0 || cap <= 0 || !d_depth || rows <= 0 || cols <= 0 ||
        depth_step < 4 * (size_t)cols || depth_step % 4 || !d_uright || !d_depth_out ||
        (nframes > 1 && (depth_frame_stride < depth_step * rows || depth_frame_stride % 4)) ||
        !ft_grid(nframes, cap, &bpf, &nb))
        return ORBX_EINVAL;
    if (nframes == 0) return ORBX_OK;
    hipLaunchKernelGGL(k_rgbd_stereo, dim3(nb), dim3(kFtBlock), 0, (hipStream_t)stream, d_kps, d_kps_un, d_counts, cap,
                       bpf, d_depth, rows, cols, depth_step, nframes > 1 ? depth_frame_stride : 0, bf, d_uright,
                       d_depth_out);
    return hipGetLastError() == hipSuccess ? ORBX_OK : ORBX_EDEVICE;
}

orbx_status orbx_rgbd_stereo(int device, const orbx_keypoint* kps, const orbx_keypoint* kps_un, int n,
                             const float* depth, int rows, int cols, size_t depth_step, float bf, float* uright,
                             float* depth_out)
{
    if (n < 0 || rows <= 0 || cols <= 0 || !depth || depth_step < 4 * (size_t)cols || depth_step % 4)
        return ORBX_EINVAL;
    if (n == 0) return ORBX_OK;
    if (!kps || !kps_un || !uright || !depth_out) return ORBX_EINVAL;
    for (int i = 0; i < n; ++i)   // negated: a NaN coordinate fails too
        if (!(kps[i].x >= 0.0f && kps[i].x < (float)cols && kps[i].y >= 0.0f && kps[i].y < (float)rows))
            return ORBX_EINVAL;
    HostCall c(device);
    const size_t N = (size_t)n;
    const auto ocn = c.in(&n, 1);
    const auto ok = c.in(kps, N);
    const auto oku = c.in(kps_un, N);
    const auto od = c.in(depth, depth_step / 4 * (size_t)rows);   // depth_step is a multiple of 4
    const auto oo = c.out<float>(2 * N);                          // uright, depth_out
    orbx_status rc = c.begin();
    if (rc != ORBX_OK) return rc;
    rc = orbx_rgbd_stereo_batch_device(c.dev(ok), c.dev(oku), c.dev(ocn), 1, n, c.dev(od), rows, cols, depth_step, 0,
                                       bf, c.dev(oo), c.dev(oo, N), c.stream());
    if (rc != ORBX_OK) return rc;
    c.fetch(oo, uright, N);
    c.fetch(oo, depth_out, N, N);
    return c.finish();
}

orbx_status orbm_frustum_batch_device(const orbm_map_point* d_pts, const int* d_npts, int nframes, int pcap,
                                      const float* d_pose, const orbm_pose_params* params, float viewing_cos_limit,
                                      orbm_proj_point* d_out, int* d_ninview, void* stream)
{
    int bpf;
    unsigned nb;
    if (!d_pts || !d_npts || nframes < 0 || pcap <= 0 || !d_pose || !params || params->nlevels < 1 ||
        params->nlevels > 16 || !d_out || !d_ninview || !ft_grid(nframes, pcap, &bpf, &nb))
        return ORBX_EINVAL;
    if (nframes == 0) return ORBX_OK;
    hipStream_t s = (hipStream_t)stream;
    hipMemsetAsync(d_ninview, 0, sizeof(int) * (size_t)nframes, s);
    hipLaunchKernelGGL(k_frustum, dim3(nb), dim3(kFtBlock), 0, s, d_pts, d_npts, pcap, bpf, d_pose, *params,
                       viewing_cos_limit, d_out, d_ninview);
    return hipGetLastError() == hipSuccess ? ORBX_OK : ORBX_EDEVICE;
}

orbx_status orbm_frustum(int device, const orbm_map_point* pts, int np, const float* pose,
                         const orbm_pose_params* params, float viewing_cos_limit, orbm_proj_point* out, int* ninview)
{
    if (np < 0 || !pose || !params || params->nlevels < 1 || params->nlevels > 16 || !ninview) return ORBX_EINVAL;
    *ninview = 0;
    if (np == 0) return ORBX_OK;
    if (!pts || !out) return ORBX_EINVAL;
    HostCall c(device);
    const auto ocn = c.in(&np, 1);
    const auto opo = c.in(pose, 12);
    const auto op = c.in(pts, (size_t)np);
    const auto on = c.out<int>(1);
    const auto oo = c.out<orbm_proj_point>((size_t)np);
    orbx_status rc = c.begin();
    if (rc != ORBX_OK) return rc;
    rc = orbm_frustum_batch_device(c.dev(op), c.dev(ocn), 1, np, c.dev(opo), params, viewing_cos_limit, c.dev(oo),
                                   c.dev(on), c.stream());
    if (rc != ORBX_OK) return rc;
    c.fetch(on, ninview, 1);
    c.fetch(oo, out, (size_t)np);
    return c.finish();
}

}  // extern "C"

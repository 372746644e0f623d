// The match loop of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:284-450) over the vMatchedPairs that
// SearchForTriangulation (orbm_bow_search_device, ORBM_TRIANGULATION) left on the device, emitting the new MapPoints
// in the layout orbm_refresh_map_points_device reads.  Kernels and C entry points (include/orbx.h).
//
// T1 k_triangulate     one lane per (pair, idx1).  Range checks first (KeyFrame slots, idx2, octaves, stereo depth),
//                      then the reference's loop body statement by statement: parallax of the two rays, the 4x4
//                      cv::SVD (OpenCV 3.x JacobiSVDImpl_<float> on A transposed) or KeyFrame::UnprojectStereo, depth
//                      signs, chi-square reprojection error, scale consistency.  Writes d_status always and d_x3d for
//                      a created point.  At, Vt (32 floats) and W (4 doubles) stay in registers: the six (i, j) pairs
//                      of a sweep and the final selection sort are unrolled, so no array is indexed by a runtime
//                      value; the sort moves rows with selects.  The sweep loop is data dependent (a lane leaves it
//                      when no pair rotated), so a wave runs as long as its slowest lane.
// T2 k_triang_compact  one workgroup per pair: a running scan over d_status in chunks of 256 entries (ballot + lane
//                      rank inside a wave, the four wave totals through LDS), so pair p's created points land at
//                      p * match_stride + k in ascending idx1, the order of vMatchedIndices.  Writes the MapPoint,
//                      its two observations (ordered by the caller's KeyFrame rank), its ref, idx1, the has_mp marks
//                      and d_nnew[p].
// Arithmetic: DESIGN.md §3 "Triangulation arithmetic"; -ffp-contract=off, the reference's FMAs written out.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "orbx_device.hpp"
#include "orbx_host.hpp"
#include "orbx_kernels.hpp"
#include "orbx_math.hpp"

namespace orbx {

constexpr int kTriThreads = 256;   // T1 block; T2 block and scan chunk
constexpr int kTriSweeps = 30;     // max_iter = std::max(m, 30)

// One Jacobi rotation of rows i and j of At (and of Vt), or none when the rows are orthogonal already.
__device__ __forceinline__ bool tri_rotate(float (&Ai)[4], float (&Aj)[4], float (&Vi)[4], float (&Vj)[4], double& Wi,
                                           double& Wj)
{
    const double eps = (double)(1.1920928955078125e-07f * 2.0f);   // FLT_EPSILON*2, a float in the reference
    double a = Wi, b = Wj, p = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) p += (double)Ai[k] * (double)Aj[k];
    if (__builtin_fabs(p) <= eps * __builtin_sqrt(a * b)) return false;
    p *= 2.0;
    const double beta = a - b, gamma = __builtin_sqrt(p * p + beta * beta);   // hypot(p, beta)
    float c, s;
    if (beta < 0.0) {
        const double delta = (gamma - beta) * 0.5;
        s = (float)__builtin_sqrt(delta / gamma);
        c = (float)(p / (gamma * (double)s * 2.0));
    } else {
        c = (float)__builtin_sqrt((gamma + beta) / (gamma * 2.0));
        s = (float)(p / (gamma * (double)c * 2.0));
    }
    a = b = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float t0 = c * Ai[k] + s * Aj[k];
        const float t1 = -s * Ai[k] + c * Aj[k];
        Ai[k] = t0;
        Aj[k] = t1;
        a += (double)t0 * (double)t0;
        b += (double)t1 * (double)t1;
    }
    Wi = a;
    Wj = b;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float t0 = c * Vi[k] + s * Vj[k];
        const float t1 = -s * Vi[k] + c * Vj[k];
        Vi[k] = t0;
        Vj[k] = t1;
    }
    return true;
}

// cv::SVD::compute(A, w, u, vt, MODIFY_A | FULL_UV) as far as vt.row(3): At = A transposed on entry.
__device__ __forceinline__ void tri_svd_last_row(float (&At)[4][4], float (&x)[4])
{
    float Vt[4][4];
    double W[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        double sd = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            sd += (double)At[i][k] * (double)At[i][k];
            Vt[i][k] = i == k ? 1.0f : 0.0f;
        }
        W[i] = sd;
    }
    for (int iter = 0; iter < kTriSweeps; ++iter) {
        bool changed = false;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = i + 1; j < 4; ++j) changed |= tri_rotate(At[i], At[j], Vt[i], Vt[j], W[i], W[j]);
        if (!changed) break;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        double sd = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) sd += (double)At[i][k] * (double)At[i][k];
        W[i] = __builtin_sqrt(sd);
    }
    // selection sort to descending W (strict <); the rows of At are not needed any more
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        int j = i;
        double wj = W[i];
#pragma unroll
        for (int k = i + 1; k < 4; ++k) {
            const bool up = wj < W[k];
            j = up ? k : j;
            wj = up ? W[k] : wj;
        }
#pragma unroll
        for (int k = i + 1; k < 4; ++k) {
            const bool sw = j == k;
            const double wi = W[i];
            W[i] = sw ? W[k] : wi;
            W[k] = sw ? wi : W[k];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float vi = Vt[i][q];
                Vt[i][q] = sw ? Vt[k][q] : vi;
                Vt[k][q] = sw ? vi : Vt[k][q];
            }
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) x[q] = Vt[3][q];
}

// row.dot(x3Dt) + t: the dot product and the sum in double, rounded once
__device__ __forceinline__ float tri_dot_add(const float* r, const float (&X)[3], float t)
{
    double d = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) d += (double)r[k] * (double)X[k];
    return (float)(d + (double)t);
}

// cv::norm(x3D - Ow), rounded to float
__device__ __forceinline__ float tri_dist(const float (&X)[3], const float* Ow)
{
    double d = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float n = X[k] - Ow[k];
        d += (double)n * (double)n;
    }
    return (float)__builtin_sqrt(d);
}

// the reprojection test of one KeyFrame (:362-413): true = continue
__device__ __forceinline__ bool tri_reproj_fails(const PsCam& c, const float (&X)[3], float z, float kx, float ky,
                                                 float ur, bool stereo, float sigma2, const orbm_pose_params& P)
{
    const float x = tri_dot_add(c.R, X, c.t[0]);
    const float y = tri_dot_add(c.R + 3, X, c.t[1]);
    const float invz = (float)(1.0 / (double)z);
    const float u = __builtin_fmaf(P.fx * x, invz, P.cx);
    const float v = __builtin_fmaf(P.fy * y, invz, P.cy);
    const float ex = u - kx, ey = v - ky;
    float e2 = __builtin_fmaf(ex, ex, ey * ey);
    if (!stereo) return (double)e2 > 5.991 * (double)sigma2;
    const float u_r = __builtin_fmaf(-P.bf, invz, u);
    const float er = u_r - ur;
    e2 = __builtin_fmaf(er, er, e2);
    return (double)e2 > 7.8 * (double)sigma2;
}

// KeyFrame::UnprojectStereo (src/KeyFrame.cc:615-631), z > 0 checked by the caller
__device__ __forceinline__ void tri_unproject(const PsCam& c, float u, float v, float z, float invfx, float invfy,
                                              const orbm_pose_params& P, float (&X)[3])
{
    const float x = (u - P.cx) * z * invfx;
    const float y = (v - P.cy) * z * invfy;
#pragma unroll
    for (int r = 0; r < 3; ++r) X[r] = ps_row(c.R + r, 3, x, y, z) + c.Ow[r];   // Twc's rotation is Rcw.t()
}

__global__ __launch_bounds__(kTriThreads) void k_triangulate(
    const orbx_keypoint* __restrict__ kps, const orbx_keypoint* __restrict__ kps_raw,
    const float* __restrict__ uright, const float* __restrict__ depth, const int* __restrict__ counts, int nkf, int cap,
    const float* __restrict__ pose, const int* __restrict__ pair_a, const int* __restrict__ pair_b, int npairs,
    const int* __restrict__ match, int match_stride, orbm_pose_params P, float* __restrict__ x3d,
    int* __restrict__ status)
{
    const int i1 = blockIdx.x * kTriThreads + (int)threadIdx.x;
    if (i1 >= cap) return;
    const orbx_keypoint* __restrict__ const raw = kps_raw ? kps_raw : kps;
    for (int p = blockIdx.y; p < npairs; p += gridDim.y) {
        const size_t e = (size_t)p * (size_t)match_stride + (size_t)i1;
        const int a = pair_a[p], b = pair_b[p];
        if (a < 0 || a >= nkf || b < 0 || b >= nkf) {
            status[e] = ORBM_TRI_INVALID;
            continue;
        }
        if (i1 >= min(counts[a], cap)) {
            status[e] = ORBM_TRI_NO_MATCH;
            continue;
        }
        const int i2 = match[e];
        if (i2 < 0) {
            status[e] = ORBM_TRI_NO_MATCH;
            continue;
        }
        if (i2 >= min(counts[b], cap)) {
            status[e] = ORBM_TRI_INVALID;
            continue;
        }
        const size_t f1 = (size_t)a * cap + i1, f2 = (size_t)b * cap + i2;
        const float k1x = kps[f1].x, k1y = kps[f1].y, k2x = kps[f2].x, k2y = kps[f2].y;
        const int o1 = kps[f1].octave, o2 = kps[f2].octave;
        const float ur1 = uright ? uright[f1] : -1.0f, ur2 = uright ? uright[f2] : -1.0f;
        const bool st1 = ur1 >= 0.0f, st2 = ur2 >= 0.0f;
        const float d1 = st1 ? depth[f1] : -1.0f, d2 = st2 ? depth[f2] : -1.0f;
        if (o1 < 0 || o1 >= P.nlevels || o2 < 0 || o2 >= P.nlevels || (st1 && !(d1 > 0.0f)) || (st2 && !(d2 > 0.0f))) {
            status[e] = ORBM_TRI_INVALID;
            continue;
        }
        const PsCam c1 = ps_camera(ORBM_PROJ_KEYFRAME, pose + (size_t)a * 12, P);
        const PsCam c2 = ps_camera(ORBM_PROJ_KEYFRAME, pose + (size_t)b * 12, P);
        const float invfx = 1.0f / P.fx, invfy = 1.0f / P.fy;
        const float xn1[2] = {(k1x - P.cx) * invfx, (k1y - P.cy) * invfy};
        const float xn2[2] = {(k2x - P.cx) * invfx, (k2y - P.cy) * invfy};
        // ray = Rwc*xn, cosParallaxRays (:303-305)
        double dot = 0.0, n1 = 0.0, n2 = 0.0;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const float r1 = ps_row(c1.R + r, 3, xn1[0], xn1[1], 1.0f);
            const float r2 = ps_row(c2.R + r, 3, xn2[0], xn2[1], 1.0f);
            dot += (double)r1 * (double)r2;
            n1 += (double)r1 * (double)r1;
            n2 += (double)r2 * (double)r2;
        }
        const float cpr = (float)(dot / (__builtin_sqrt(n1) * __builtin_sqrt(n2)));
        float cs1 = cpr + 1.0f, cs2 = cs1;
        if (st1) cs1 = glibc_sincosf(2.0f * atan2f(P.b / 2.0f, d1), 1);   // cos(2*atan2(mb/2, mvDepth[idx1]))
        else if (st2) cs2 = glibc_sincosf(2.0f * atan2f(P.b / 2.0f, d2), 1);
        const float cs = cs2 < cs1 ? cs2 : cs1;   // std::min(cs1, cs2)

        float X[3];
        int code;
        if (cpr < cs && cpr > 0.0f && (st1 || st2 || (double)cpr < 0.9998)) {
            // A.row = xn*Tcw.row(2) - Tcw.row(k) (:322-326), held transposed
            float At[4][4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float a2 = k < 3 ? c1.R[6 + k] : c1.t[2], b2 = k < 3 ? c2.R[6 + k] : c2.t[2];
                At[k][0] = xn1[0] * a2 - (k < 3 ? c1.R[k] : c1.t[0]);
                At[k][1] = xn1[1] * a2 - (k < 3 ? c1.R[3 + k] : c1.t[1]);
                At[k][2] = xn2[0] * b2 - (k < 3 ? c2.R[k] : c2.t[0]);
                At[k][3] = xn2[1] * b2 - (k < 3 ? c2.R[3 + k] : c2.t[1]);
            }
            float h[4];
            tri_svd_last_row(At, h);
            if (h[3] == 0.0f) {
                status[e] = ORBM_TRI_W_ZERO;
                continue;
            }
            const float iw = (float)(1.0 / (double)h[3]);   // x3D.rowRange(0,3)/x3D.at<float>(3)
#pragma unroll
            for (int k = 0; k < 3; ++k) X[k] = h[k] * iw + 0.0f;
            code = ORBM_TRI_CREATED_SVD;
        } else if (st1 && cs1 < cs2) {
            tri_unproject(c1, raw[f1].x, raw[f1].y, d1, invfx, invfy, P, X);   // mvKeys, not mvKeysUn
            code = ORBM_TRI_CREATED_STEREO1;
        } else if (st2 && cs2 < cs1) {
            tri_unproject(c2, raw[f2].x, raw[f2].y, d2, invfx, invfy, P, X);
            code = ORBM_TRI_CREATED_STEREO2;
        } else {
            status[e] = ORBM_TRI_LOW_PARALLAX;
            continue;
        }

        const float z1 = tri_dot_add(c1.R + 6, X, c1.t[2]);
        if (z1 <= 0.0f) {
            status[e] = ORBM_TRI_Z1;
            continue;
        }
        const float z2 = tri_dot_add(c2.R + 6, X, c2.t[2]);
        if (z2 <= 0.0f) {
            status[e] = ORBM_TRI_Z2;
            continue;
        }
        const float s1 = P.scale[o1], s2 = P.scale[o2];
        if (tri_reproj_fails(c1, X, z1, k1x, k1y, ur1, st1, s1 * s1, P)) {
            status[e] = ORBM_TRI_REPROJ1;
            continue;
        }
        if (tri_reproj_fails(c2, X, z2, k2x, k2y, ur2, st2, s2 * s2, P)) {
            status[e] = ORBM_TRI_REPROJ2;
            continue;
        }
        const float dist1 = tri_dist(X, c1.Ow), dist2 = tri_dist(X, c2.Ow);
        if (dist1 == 0.0f || dist2 == 0.0f) {
            status[e] = ORBM_TRI_ZERO_DIST;
            continue;
        }
        const float ratio_dist = dist2 / dist1, ratio_octave = s1 / s2, ratio_factor = 1.5f * P.scale[1];
        if (ratio_dist * ratio_factor < ratio_octave || ratio_dist > ratio_octave * ratio_factor) {
            status[e] = ORBM_TRI_SCALE;
            continue;
        }
        x3d[3 * e] = X[0];
        x3d[3 * e + 1] = X[1];
        x3d[3 * e + 2] = X[2];
        status[e] = code;
    }
}

__global__ __launch_bounds__(kTriThreads) void k_triang_compact(
    const int* __restrict__ counts, int nkf, int cap, const int* __restrict__ kf_rank,
    const int* __restrict__ pair_a, const int* __restrict__ pair_b, const int* __restrict__ match, int match_stride,
    const float* __restrict__ x3d, const int* __restrict__ status, orbm_map_point* __restrict__ new_pts,
    orbm_observation* __restrict__ new_obs, orbm_observation* __restrict__ new_ref, int* __restrict__ new_idx1,
    int* __restrict__ nnew, uint8_t* __restrict__ mark)
{
    __shared__ int wave_total[kTriThreads / 64];
    const int p = blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int a = pair_a[p], b = pair_b[p];
    int n = 0;
    if (a >= 0 && a < nkf && b >= 0 && b < nkf) n = min(counts[a], cap);
    // (kf1, idx1) first unless the caller's std::map iterates KeyFrame 2 first; equal ranks keep the insertion order
    const bool swap = n > 0 && (kf_rank ? kf_rank[b] < kf_rank[a] : b < a);
    const size_t base = (size_t)p * (size_t)match_stride;
    int run = 0;   // created points of the chunks before this one
    for (int c0 = 0; c0 < n; c0 += kTriThreads) {
        const int i1 = c0 + tid;
        const int st = i1 < n ? status[base + i1] : ORBM_TRI_NO_MATCH;
        const bool made = st == ORBM_TRI_CREATED_SVD || st == ORBM_TRI_CREATED_STEREO1 || st == ORBM_TRI_CREATED_STEREO2;
        const unsigned long long m = __ballot(made);
        if (lane == 0) wave_total[w] = __popcll(m);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int q = 0; q < kTriThreads / 64; ++q) {
            const int t = wave_total[q];
            before += q < w ? t : 0;
            total += t;
        }
        if (made) {
            const size_t k = base + (size_t)(run + before + lanes_below(m));
            const size_t e = base + i1;
            const int i2 = match[e];   // in range: k_triangulate checked it before it set a created status
            orbm_map_point mp;
            mp.x = x3d[3 * e];
            mp.y = x3d[3 * e + 1];
            mp.z = x3d[3 * e + 2];
            mp.nx = mp.ny = mp.nz = mp.max_dist = mp.min_dist = mp.angle = 0.0f;
            mp.octave = 0;
            mp.flags = 3;
            mp.pad = 0;
            new_pts[k] = mp;
            orbm_observation oa, ob;
            oa.kf = a;
            oa.idx = i1;
            ob.kf = b;
            ob.idx = i2;
            new_obs[2 * k] = swap ? ob : oa;
            new_obs[2 * k + 1] = swap ? oa : ob;
            new_ref[k] = oa;
            new_idx1[k] = i1;
            if (mark) {
                mark[(size_t)a * cap + i1] = 1;
                mark[(size_t)b * cap + i2] = 1;
            }
        }
        run += total;
        __syncthreads();   // wave_total is rewritten by the next chunk
    }
    if (tid == 0) nnew[p] = run;
}

namespace {

bool tri_args_ok(int nkf, int cap, int npairs, int match_stride, const orbm_pose_params* params, const void* uright,
                 const void* depth)
{
    return nkf >= 0 && npairs >= 0 && cap > 0 && cap <= ORBM_MAX_FEATURES && match_stride >= cap && params &&
           params->nlevels >= 1 && params->nlevels <= 16 && (uright != nullptr) == (depth != nullptr);
}

}  // namespace

}  // namespace orbx

using namespace orbx;

extern "C" {

orbx_status orbm_triangulate_device(const orbx_keypoint* d_kps, const orbx_keypoint* d_kps_raw, const float* d_uright,
                                    const float* d_depth, const int* d_counts, int nkf, int cap, const float* d_pose,
                                    const int* d_kf_rank, const int* d_pair_a, const int* d_pair_b, int npairs,
                                    const int* d_match, int match_stride, const orbm_pose_params* params, float* d_x3d,
                                    int* d_status, orbm_map_point* d_new_pts, orbm_observation* d_new_obs,
                                    orbm_observation* d_new_ref, int* d_new_idx1, int* d_nnew, uint8_t* d_mark,
                                    void* stream)
{
    if (!tri_args_ok(nkf, cap, npairs, match_stride, params, d_uright, d_depth) || !d_kps || !d_counts || !d_pose ||
        !d_pair_a || !d_pair_b || !d_match || !d_x3d || !d_status || !d_new_pts || !d_new_obs || !d_new_ref ||
        !d_new_idx1 || !d_nnew)
        return ORBX_EINVAL;
    if (npairs == 0) return ORBX_OK;
    const dim3 grid((unsigned)((cap + kTriThreads - 1) / kTriThreads), (unsigned)std::min(npairs, 65535));
    hipLaunchKernelGGL(k_triangulate, grid, dim3(kTriThreads), 0, (hipStream_t)stream, d_kps, d_kps_raw, d_uright,
                       d_depth, d_counts, nkf, cap, d_pose, d_pair_a, d_pair_b, npairs, d_match, match_stride, *params,
                       d_x3d, d_status);
    hipLaunchKernelGGL(k_triang_compact, dim3((unsigned)npairs), dim3(kTriThreads), 0, (hipStream_t)stream, d_counts,
                       nkf, cap, d_kf_rank, d_pair_a, d_pair_b, d_match, match_stride, d_x3d, d_status, d_new_pts,
                       d_new_obs, d_new_ref, d_new_idx1, d_nnew, d_mark);
    return hipGetLastError() == hipSuccess ? ORBX_OK : ORBX_EDEVICE;
}

orbx_status orbm_triangulate(int device, const orbx_keypoint* kps1, const orbx_keypoint* kps1_raw, const float* uright1,
                             const float* depth1, int n1, const float* T1w, const orbx_keypoint* kps2,
                             const orbx_keypoint* kps2_raw, const float* uright2, const float* depth2, int n2,
                             const float* T2w, const int* match, const orbm_pose_params* params, float* x3d,
                             int* status, orbm_map_point* new_pts, orbm_observation* new_obs,
                             orbm_observation* new_ref, int* new_idx1, int* nnew, uint8_t* mark1, uint8_t* mark2)
{
    const bool stereo = uright1 || depth1 || uright2 || depth2;
    if (n1 < 0 || n1 > ORBM_MAX_FEATURES || n2 < 0 || n2 > ORBM_MAX_FEATURES || !params || params->nlevels < 1 ||
        params->nlevels > 16 || !T1w || !T2w || !nnew || (mark1 != nullptr) != (mark2 != nullptr) ||
        (stereo && (!uright1 || !depth1 || !uright2 || !depth2)) || (kps1_raw != nullptr) != (kps2_raw != nullptr))
        return ORBX_EINVAL;
    if (n1 > 0 && (!kps1 || !match || !x3d || !status || !new_pts || !new_obs || !new_ref || !new_idx1))
        return ORBX_EINVAL;
    if (n2 > 0 && !kps2) return ORBX_EINVAL;
    *nnew = 0;
    if (n1 == 0) return ORBX_OK;
    // the two KeyFrames as a table of two at stride cap; KeyFrame 1 is slot 0, so the slot order is (kf1, kf2)
    const int cap = std::max(n1, n2);
    const size_t c = (size_t)cap;
    const int head[4] = {n1, n2, 0, 1};   // d_counts[2], d_pair_a[1], d_pair_b[1]
    float poses[24];
    std::memcpy(poses, T1w, sizeof(float) * 12);
    std::memcpy(poses + 12, T2w, sizeof(float) * 12);
    HostCall hc(device);
    const size_t m1 = (size_t)n1, m2 = (size_t)n2;
    const auto oh = hc.in(head, 4);
    const auto og = hc.in(poses, 24);
    const auto ok = hc.stage<orbx_keypoint>(2 * c);
    const auto okr = hc.stage<orbx_keypoint>(2 * c);
    const auto ou = hc.stage<float>(2 * c);
    const auto odp = hc.stage<float>(2 * c);
    const auto om = hc.in(match, m1);
    const auto omk = hc.stage<uint8_t>(2 * c);
    const auto ox = hc.inout(x3d, 3 * m1);                  // entries of no created point keep their bits
    const auto os = hc.out<int>(c + 1);                     // status[cap], nnew
    const auto op = hc.out<orbm_map_point>(c);
    const auto oo = hc.out<orbm_observation>(3 * c);        // new_obs[2 * cap], new_ref[cap]
    const auto oi = hc.out<int>(c);
    orbx_status rc = hc.prepare();
    if (rc != ORBX_OK) return rc;
    pack_pair(hc.host(ok), c, kps1, m1, kps2, m2);
    pack_pair(hc.host(okr), c, kps1_raw, m1, kps2_raw, m2);
    pack_pair(hc.host(ou), c, uright1, m1, uright2, m2);
    pack_pair(hc.host(odp), c, depth1, m1, depth2, m2);
    pack_pair(hc.host(omk), c, mark1, m1, mark2, m2);
    if ((rc = hc.upload()) != ORBX_OK) return rc;
    rc = orbm_triangulate_device(hc.dev(ok), kps1_raw ? hc.dev(okr) : nullptr, stereo ? hc.dev(ou) : nullptr,
                                 stereo ? hc.dev(odp) : nullptr, hc.dev(oh), 2, cap, hc.dev(og), nullptr,
                                 hc.dev(oh, 2), hc.dev(oh, 3), 1, hc.dev(om), cap, params, hc.dev(ox), hc.dev(os),
                                 hc.dev(op), hc.dev(oo), hc.dev(oo, 2 * c), hc.dev(oi), hc.dev(os, c),
                                 mark1 ? hc.dev(omk) : nullptr, hc.stream());
    if (rc != ORBX_OK) return rc;
    // the compacted arrays are fetched whole: entries at and past *nnew hold whatever the device block held
    hc.fetch(os, status, m1);
    hc.fetch(os, nnew, 1, c);
    hc.fetch(omk, mark1, m1);
    hc.fetch(omk, mark2, m2, c);
    // staged: only the first *nnew compacted entries are the call's
    std::vector<orbm_map_point> hp(c);
    std::vector<orbm_observation> ho(3 * c);
    std::vector<int> hi(c);
    hc.fetch(op, hp.data(), c);
    hc.fetch(oo, ho.data(), 3 * c);
    hc.fetch(oi, hi.data(), c);
    if ((rc = hc.finish()) != ORBX_OK) return rc;
    const size_t k = (size_t)std::max(0, std::min(*nnew, n1));
    std::memcpy(new_pts, hp.data(), sizeof(orbm_map_point) * k);
    std::memcpy(new_obs, ho.data(), sizeof(orbm_observation) * 2 * k);
    std::memcpy(new_ref, ho.data() + 2 * c, sizeof(orbm_observation) * k);
    std::memcpy(new_idx1, hi.data(), sizeof(int) * k);
    return ORBX_OK;
}

}  // extern "C"

// MapPoint refresh: MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:242-307) and
// MapPoint::UpdateNormalAndDepth (:330-371) over a KeyFrame table, in place on the orbm_map_point / descriptor
// arrays the projection matchers read.  Kernel and C entry points (include/orbx.h).
//
// M1 k_mp_refresh   one wave per MapPoint, up to four MapPoints per workgroup.  The wave walks the point's
//                   observation list in chunks of 64, in list order:
//                     - every lane checks its observation (KeyFrame slot and feature index in range) before it
//                       reads anything through it; one bad observation and the point is left alone (best = -2);
//                     - normal: each lane's (Pos - Ow_i) / |Pos - Ow_i| goes to LDS and lanes 0..2 add one component
//                       each, in list order (the float sum's order is the caller's std::map order);
//                     - descriptor: the descriptors of the good KeyFrames are compacted into LDS (ballot + lane
//                       rank, so the rows keep list order) with their position in the full list.
//                   Median: distances are integers in 0..256, so a row's k-th smallest is the least v with
//                   count(d <= v) >= k + 1: nine bisection steps, no sort.  Up to 32 good rows (nearly every
//                   MapPoint) the wave's 64 lanes hold the whole matrix in registers, rows x column slices
//                   (mp_median_sliced), and a step is a few compares and shuffles.  Beyond, lane i owns rows i,
//                   i + 64, ... and a step is one pass over the LDS rows (all lanes read the same row: a broadcast, no
//                   bank conflict) with __popcll.  The winner is the wave minimum of (median << 16) | row, which is
//                   the reference's first strictly smaller median.
// LDS per wave: 36 B per observation of max_obs (rounded up to 4) + 768 B; nothing static (dyn_lds).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "orbx_device.hpp"
#include "orbx_host.hpp"
#include "orbx_kernels.hpp"

namespace orbx {

constexpr int kMpWaves = 4;          // MapPoints per workgroup at most
constexpr int kMpLdsObs = 1024;      // observations' worth of LDS per workgroup at most (ORBM_MAX_OBSERVATIONS)

// one wave's LDS: mo4 descriptors (32 B), mo4 list positions (int), one chunk's 64 x 3 unit-vector components
__host__ __device__ constexpr size_t mp_wave_bytes(int mo4) { return (size_t)mo4 * 36 + 64 * 3 * sizeof(float); }

// (median << 16) | row of this lane's row when the point has at most G <= 32 good rows: the wave holds the whole
// matrix in registers, as G rows (a power of two >= ng) by S = 64 / G column slices.  Lane s * G + r computes row r's
// distances to columns s, s + S, ... once (G / S of them); a bisection step is then that many compares and
// log2(S) shuffles, with no LDS pass.  All 64 lanes take part; lanes of rows at and past ng return ~0.
template <int G>
__device__ __forceinline__ uint32_t mp_median_sliced(const ulonglong2* sdesc, int ng, int need, int lane)
{
    constexpr int S = 64 / G, C = G / S;
    const int r = lane & (G - 1), s = lane / G;
    const bool row = r < ng;
    const ulonglong2 a0 = sdesc[2 * (row ? r : 0)], a1 = sdesc[2 * (row ? r : 0) + 1];
    int d[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int j = s + c * S;
        const int jj = j < ng ? j : 0;   // a column past ng is never read (G may exceed the LDS rows) and never counts
        const int h = ham256(a0, a1, sdesc[2 * jj], sdesc[2 * jj + 1]);
        d[c] = j < ng ? h : 0x7FFF;
    }
    int lo = 0, hi = 256;   // count(d <= hi) >= need holds throughout
    for (int it = 0; it < 9; ++it) {
        const int mid = (lo + hi) >> 1;
        int cnt = 0;
#pragma unroll
        for (int c = 0; c < C; ++c) cnt += d[c] <= mid;
#pragma unroll
        for (int o = G; o < 64; o <<= 1) cnt += __shfl_xor(cnt, o);
        if (cnt >= need) hi = mid;
        else lo = mid + 1;
    }
    return row ? ((uint32_t)hi << 16) | (uint32_t)r : 0xFFFFFFFFu;
}

// pts is read (x, y, z, flags) and written (the fields `what` selects) by the same wave: no __restrict__
__global__ __launch_bounds__(kMpWaves * 64) void k_mp_refresh(
    int what, const orbx_keypoint* __restrict__ kps, const ulonglong2* __restrict__ desc,
    const int* __restrict__ counts, int nkf, int cap, const float* __restrict__ pose,
    const uint8_t* __restrict__ kf_bad, const int* __restrict__ obs_ptr, const orbm_observation* __restrict__ obs,
    const orbm_observation* __restrict__ ref, int np, int max_obs, int mo4, orbm_pose_params P, orbm_map_point* pts,
    ulonglong2* __restrict__ pdesc, int* __restrict__ best)
{
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int m = blockIdx.x * (int)(blockDim.x >> 6) + w;
    if (m >= np) return;   // every exit below is taken by the whole wave
    uint8_t* const lds = dyn_lds() + (size_t)w * mp_wave_bytes(mo4);
    ulonglong2* const sdesc = (ulonglong2*)lds;
    int* const spos = (int*)(lds + (size_t)mo4 * 32);
    float* const sunit = (float*)(lds + (size_t)mo4 * 36);

    const int p0 = obs_ptr[m], n = obs_ptr[m + 1] - p0;
    if (!(pts[m].flags & 1) || n == 0) {   // mbBad (:251, :338), observations.empty() (:256, :345)
        if (lane == 0) best[m] = -1;
        return;
    }
    // what the reference would read out of bounds: the ref first, the observations chunk by chunk
    const orbm_observation rf = ref[m];
    bool invalid = p0 < 0 || n < 0 || n > max_obs || rf.kf < 0 || rf.kf >= nkf;
    int level = 0;
    if (!invalid) {
        invalid = rf.idx < 0 || rf.idx >= min(counts[rf.kf], cap);
        if (!invalid) {
            level = kps[(size_t)rf.kf * cap + rf.idx].octave;   // pRefKF->mvKeysUn[observations[pRefKF]].octave (:361)
            invalid = level < 0 || level >= P.nlevels;
        }
    }
    const float X = pts[m].x, Y = pts[m].y, Z = pts[m].z;
    float acc = 0.0f;   // lanes 0..2: one component of normal (cv::Mat::zeros(3,1,CV_32F), :348)
    int ng = 0;         // vDescriptors.size() so far
    for (int c0 = 0; c0 < n && !invalid; c0 += 64) {
        const int j = c0 + lane;
        orbm_observation o;
        o.kf = o.idx = -1;
        bool ok = false;
        if (j < n) {
            o = obs[(size_t)p0 + j];
            ok = o.kf >= 0 && o.kf < nkf && o.idx >= 0 && o.idx < min(counts[o.kf], cap);
        }
        if (__ballot(j < n && !ok)) {
            invalid = true;
            break;
        }
        if (ok && (what & ORBM_REFRESH_NORMAL_DEPTH)) {   // normali = mWorldPos - Owi; normali/cv::norm(normali) (:353-355)
            const PsCam c = ps_camera(ORBM_PROJ_KEYFRAME, pose + (size_t)o.kf * 12, P);
            const float n0 = X - c.Ow[0], n1 = Y - c.Ow[1], n2 = Z - c.Ow[2];
            double d = 0.0;
            d += (double)n0 * (double)n0;
            d += (double)n1 * (double)n1;
            d += (double)n2 * (double)n2;
            const float s = (float)(1.0 / __builtin_sqrt(d));
            sunit[3 * lane] = n0 * s;
            sunit[3 * lane + 1] = n1 * s;
            sunit[3 * lane + 2] = n2 * s;
        }
        const bool good = ok && (what & ORBM_REFRESH_DESCRIPTOR) && !kf_bad[o.kf];   // !pKF->isBad() (:265)
        const unsigned long long gm = __ballot(good);
        if (good) {
            const int r = ng + lanes_below(gm);
            const ulonglong2* d = desc + 2 * ((size_t)o.kf * cap + o.idx);
            sdesc[2 * r] = d[0];
            sdesc[2 * r + 1] = d[1];
            spos[r] = j;
        }
        ng += __popcll(gm);
        wave_lds_sync();
        if ((what & ORBM_REFRESH_NORMAL_DEPTH) && lane < 3) {
            const int cnt = min(64, n - c0);
            for (int i = 0; i < cnt; ++i) acc = acc + sunit[3 * i + lane];   // normal = normal + ... (:355)
        }
        wave_lds_sync();
    }
    if (invalid) {
        if (lane == 0) best[m] = -2;
        return;
    }

    if (what & ORBM_REFRESH_NORMAL_DEPTH) {
        float* const f = (float*)(pts + m);   // x y z nx ny nz max_dist min_dist
        const float inv_n = (float)(1.0 / (double)n);
        if (lane < 3) f[3 + lane] = acc * inv_n + 0.0f;   // mNormalVector = normal/n (:369)
        if (lane == 0) {
            const PsCam c = ps_camera(ORBM_PROJ_KEYFRAME, pose + (size_t)rf.kf * 12, P);
            const float q0 = X - c.Ow[0], q1 = Y - c.Ow[1], q2 = Z - c.Ow[2];   // PC = Pos - pRefKF->GetCameraCenter()
            double d = 0.0;
            d += (double)q0 * (double)q0;
            d += (double)q1 * (double)q1;
            d += (double)q2 * (double)q2;
            const float dist = (float)__builtin_sqrt(d);
            const float maxd = dist * P.scale[level];   // mfMaxDistance = dist*levelScaleFactor (:367)
            f[6] = maxd;
            f[7] = maxd / P.scale[P.nlevels - 1];       // mfMinDistance (:368)
        }
    }

    int bst = -1;
    if ((what & ORBM_REFRESH_DESCRIPTOR) && ng > 0) {   // vDescriptors.empty() (:269)
        const int need = ((ng - 1) >> 1) + 1;           // vDists[0.5*(N-1)] is the need-th smallest (:294)
        uint32_t key = 0xFFFFFFFFu;
        if (ng <= 8) {   // ng is the same in every lane
            key = mp_median_sliced<8>(sdesc, ng, need, lane);
        } else if (ng <= 16) {
            key = mp_median_sliced<16>(sdesc, ng, need, lane);
        } else if (ng <= 32) {
            key = mp_median_sliced<32>(sdesc, ng, need, lane);
        } else {
            for (int r = lane; r < ng; r += 64) {   // lane i owns rows i, i + 64, ...; one LDS pass per bisection step
                const ulonglong2 a0 = sdesc[2 * r], a1 = sdesc[2 * r + 1];
                int lo = 0, hi = 256;   // count(d <= hi) >= need holds throughout
                for (int it = 0; it < 9; ++it) {
                    const int mid = (lo + hi) >> 1;
                    int cnt = 0;
                    for (int i = 0; i < ng; ++i) cnt += ham256(a0, a1, sdesc[2 * i], sdesc[2 * i + 1]) <= mid;
                    if (cnt >= need) hi = mid;
                    else lo = mid + 1;
                }
                key = min(key, ((uint32_t)hi << 16) | (uint32_t)r);   // rows ascend: the first least median stays
            }
        }
        const int win = (int)(wave_min_full(key) & 0xFFFFu);   // median<BestMedian (:296)
        if (lane < 2) pdesc[2 * (size_t)m + lane] = sdesc[2 * win + lane];   // mDescriptor = vDescriptors[BestIdx].clone()
        bst = spos[win];
    }
    if (lane == 0) best[m] = bst;
}

namespace {

bool mp_args_ok(int what, int nkf, int cap, int np, const orbm_pose_params* params)
{
    return what >= 1 && what <= (ORBM_REFRESH_DESCRIPTOR | ORBM_REFRESH_NORMAL_DEPTH) && nkf >= 0 && np >= 0 &&
           cap > 0 && cap <= ORBM_MAX_FEATURES && params && params->nlevels >= 1 && params->nlevels <= 16;
}

}  // namespace

}  // namespace orbx

using namespace orbx;

extern "C" {

orbx_status orbm_refresh_map_points_device(int what, const orbx_keypoint* d_kps, const uint8_t* d_desc,
                                           const int* d_counts, int nkf, int cap, const float* d_pose,
                                           const uint8_t* d_kf_bad, const int* d_obs_ptr,
                                           const orbm_observation* d_obs, const orbm_observation* d_ref, int np,
                                           int max_obs, const orbm_pose_params* params, orbm_map_point* d_pts,
                                           uint8_t* d_pdesc, int* d_best, void* stream)
{
    if (!mp_args_ok(what, nkf, cap, np, params) || max_obs < 1 || max_obs > ORBM_MAX_OBSERVATIONS || !d_kps ||
        !d_desc || !d_counts || !d_pose || !d_kf_bad || !d_obs_ptr || !d_obs || !d_ref || !d_pts || !d_pdesc || !d_best)
        return ORBX_EINVAL;
    if (np == 0) return ORBX_OK;
    const int mo4 = (max_obs + 3) & ~3;   // keeps every wave's LDS block 16-byte aligned
    const int waves = std::max(1, std::min(kMpWaves, kMpLdsObs / mo4));
    const unsigned nb = (unsigned)(((long long)np + waves - 1) / waves);
    hipLaunchKernelGGL(k_mp_refresh, dim3(nb), dim3(64 * waves), waves * mp_wave_bytes(mo4), (hipStream_t)stream, what,
                       d_kps, (const ulonglong2*)d_desc, d_counts, nkf, cap, d_pose, d_kf_bad, d_obs_ptr, d_obs, d_ref,
                       np, max_obs, mo4, *params, d_pts, (ulonglong2*)d_pdesc, d_best);
    return hipGetLastError() == hipSuccess ? ORBX_OK : ORBX_EDEVICE;
}

orbx_status orbm_refresh_map_points(int device, int what, const orbx_keypoint* kps, const uint8_t* desc,
                                    const int* counts, int nkf, int cap, const float* pose, const uint8_t* kf_bad,
                                    const int* obs_ptr, const orbm_observation* obs, const orbm_observation* ref,
                                    int np, const orbm_pose_params* params, orbm_map_point* pts, uint8_t* pdesc,
                                    int* best)
{
    if (!mp_args_ok(what, nkf, cap, np, params)) return ORBX_EINVAL;
    if (np == 0) return ORBX_OK;
    if (!obs_ptr || !ref || !pts || !pdesc || !best || (nkf > 0 && (!kps || !desc || !counts || !pose || !kf_bad)))
        return ORBX_EINVAL;
    int max_obs = 1;
    if (obs_ptr[0] < 0) return ORBX_EINVAL;
    for (int m = 0; m < np; ++m) {
        if (obs_ptr[m + 1] < obs_ptr[m]) return ORBX_EINVAL;
        max_obs = std::max(max_obs, obs_ptr[m + 1] - obs_ptr[m]);
    }
    if (max_obs > ORBM_MAX_OBSERVATIONS || (obs_ptr[np] > 0 && !obs)) return ORBX_EINVAL;
    const size_t nk = (size_t)nkf * (size_t)cap, no = (size_t)obs_ptr[np];
    HostCall c(device);
    const size_t K = (size_t)nkf, P = (size_t)np;
    const auto ok = c.in(kps, nk);
    const auto od = c.in(desc, 32 * nk);
    const auto oc = c.in(counts, K);
    const auto opo = c.in(pose, 12 * K);
    const auto ob = c.in(kf_bad, K);
    const auto oop = c.in(obs_ptr, P + 1);
    const auto oo = c.in(obs, no);
    const auto orf = c.in(ref, P);
    const auto op = c.inout(pts, P);
    const auto opd = c.inout(pdesc, 32 * P);
    const auto obt = c.out<int>(P);
    orbx_status rc = c.begin();
    if (rc != ORBX_OK) return rc;
    rc = orbm_refresh_map_points_device(what, c.dev(ok), c.dev(od), c.dev(oc), nkf, cap, c.dev(opo), c.dev(ob),
                                        c.dev(oop), c.dev(oo), c.dev(orf), np, max_obs, params, c.dev(op), c.dev(opd),
                                        c.dev(obt), c.stream());
    if (rc != ORBX_OK) return rc;
    c.fetch(obt, best, P);
    return c.finish();
}

}  // extern "C"

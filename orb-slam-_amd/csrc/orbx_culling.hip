// LocalMapping's culls on the device: MapPointCulling (src/LocalMapping.cc:170-205) and KeyFrameCulling (:632-696)
// with the observation-side edits they cause -- MapPoint::SetBadFlag (src/MapPoint.cc:151-168),
// MapPoint::EraseObservation (:111-137), KeyFrame::EraseMapPointMatch (src/KeyFrame.cc:222-227) and the observation
// loop of KeyFrame::SetBadFlag (:469-471) -- and the stable compaction of the observation CSR that follows them.
// Kernels and C entry points (include/orbx.h).
//
// Everything is integers but GetFoundRatio's float division and the depth compares; nothing is summed in an order
// that could change, so every output is deterministic.  The culls never move an observation: they set the entry's
// byte in the erased mask, and an entry whose byte is set does not exist for any kernel here.
//
// M1 k_mc_verdict   one lane per recent MapPoint.  The verdict in the reference's order; a culled point has its list
//                   checked entry by entry, then SetBadFlag: flags bit 0 clears, every live observation nulls its
//                   KeyFrame's entry and sets its mask byte.  Points are independent: the only shared writes are -1s.
// M2 k_mc_keep      one 1,024-lane workgroup: the KEPT points in list order (ballot + lane rank, wave totals in LDS).
// K1 k_kc_cull      one 1,024-lane workgroup walks the candidates in order; a candidate's edits reach the next one
//                   through a barrier and an agent-scope fence.  Four lanes share a feature and stride its MapPoint's
//                   list; the three counters of a candidate live in LDS.  Per candidate: count (reads only), verdict,
//                   then for a culled one check (every list the edit walks, before the first write) and apply.  The
//                   group that first raises claim[mp] to the candidate's number owns the MapPoint, so an observation
//                   is erased once however many features name the point.
// O1 k_co_count / O2 k_co_scan / O3 k_co_scatter   live entries per point, their exclusive scan (in the output
//                   pointer array itself), and the scatter in list order.
// Table pointers are kernel arguments of their own.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstring>

#include "orbx_device.hpp"
#include "orbx_host.hpp"
#include "orbx_kernels.hpp"

namespace orbx {

constexpr int kCuThreads = 1024;
constexpr int kCuSub = 4;                        // lanes per feature
constexpr int kCuGroups = kCuThreads / kCuSub;   // features in flight

// a MapPoint's list, checked before it is walked (the difference in 64 bits: the pointers may hold anything)
__device__ __forceinline__ bool cu_list(const int* __restrict__ obs_ptr, int mp, int& p0, int& len)
{
    p0 = obs_ptr[mp];
    const long long l = (long long)obs_ptr[mp + 1] - (long long)p0;
    len = (int)l;
    return p0 >= 0 && l >= 0 && l <= ORBM_MAX_OBSERVATIONS;
}

// (kf, idx) names a feature of the table: mvpMapPoints[idx], mvuRight[idx], mvKeysUn[idx] of KeyFrame kf exist
__device__ __forceinline__ bool cu_obs_ok(const orbm_observation o, const int* __restrict__ counts, int nkf, int cap)
{
    if (o.kf < 0 || o.kf >= nkf) return false;
    const int n = min(counts[o.kf], cap);
    return o.idx >= 0 && o.idx < n;
}

// the minimum over the lanes of a feature's group
__device__ __forceinline__ int cu_group_min(int v)
{
#pragma unroll
    for (int o = 1; o < kCuSub; o <<= 1) v = min(v, __shfl_xor(v, o));
    return v;
}

__device__ __forceinline__ int cu_group_sum(int v)
{
#pragma unroll
    for (int o = 1; o < kCuSub; o <<= 1) v += __shfl_xor(v, o);
    return v;
}

__global__ void k_mc_verdict(const int* __restrict__ recent, int nrecent, int cur_kfid, int th_obs,
                             const int* __restrict__ counts, int* __restrict__ kf_mp, int nkf, int cap,
                             orbm_map_point* __restrict__ pts, const int* __restrict__ obs_ptr,
                             const orbm_observation* __restrict__ obs, uint8_t* __restrict__ erased, int nmp,
                             const int* __restrict__ nobs, const int* __restrict__ found,
                             const int* __restrict__ visible, const int* __restrict__ first_kfid,
                             int* __restrict__ verdict)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nrecent) return;
    const int mp = recent[k];
    if (mp < 0 || mp >= nmp) {
        verdict[k] = ORBM_CULL_INVALID;
        return;
    }
    const int flags = pts[mp].flags;
    int v;
    if (!(flags & 1)) {
        v = ORBM_CULL_ERASED_BAD;   // isBad() (:186)
    } else {
        const float ratio = __fdiv_rn((float)found[mp], (float)visible[mp]);   // GetFoundRatio (MapPoint.cc:236-240)
        const int age = (int)((unsigned)cur_kfid - (unsigned)first_kfid[mp]);
        if (ratio < 0.25f) v = ORBM_CULL_RATIO;                                // :190
        else if (age >= 2 && nobs[mp] <= th_obs) v = ORBM_CULL_OBS;            // :195
        else if (age >= 3) v = ORBM_CULL_DROPPED_OLD;                          // :200
        else v = ORBM_CULL_KEPT;
    }
    if (v == ORBM_CULL_RATIO || v == ORBM_CULL_OBS) {
        // SetBadFlag (MapPoint.cc:151-168): the whole list is checked before the first write
        int p0, len;
        bool ok = cu_list(obs_ptr, mp, p0, len);
        if (ok)
            for (int q = 0; q < len; ++q)
                if (!erased[(size_t)p0 + q]) ok &= cu_obs_ok(obs[(size_t)p0 + q], counts, nkf, cap);
        if (!ok) {
            v = ORBM_CULL_INVALID;
        } else {
            pts[mp].flags = flags & ~1;
            for (int q = 0; q < len; ++q) {
                if (erased[(size_t)p0 + q]) continue;
                const orbm_observation o = obs[(size_t)p0 + q];
                kf_mp[(size_t)o.kf * cap + o.idx] = -1;   // EraseMapPointMatch (KeyFrame.cc:222-227)
                erased[(size_t)p0 + q] = 1;               // mObservations.clear()
            }
        }
    }
    verdict[k] = v;
}

__global__ __launch_bounds__(kCuThreads) void k_mc_keep(const int* __restrict__ recent, int nrecent,
                                                        const int* __restrict__ verdict,
                                                        int* __restrict__ recent_out, int* __restrict__ nout)
{
    constexpr int T = kCuThreads, W = T / 64;
    __shared__ int s_w[W];
    const int tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6;
    int run = 0;
    for (int c0 = 0; c0 < nrecent; c0 += T) {
        const int k = c0 + tid;
        const bool in = k < nrecent && verdict[k] == ORBM_CULL_KEPT;
        const unsigned long long m = __ballot(in);
        if (lane == 0) s_w[w] = __popcll(m);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int q = 0; q < W; ++q) {
            const int a = s_w[q];
            before += q < w ? a : 0;
            total += a;
        }
        if (in) recent_out[run + before + lanes_below(m)] = recent[k];
        run += total;
        __syncthreads();   // s_w is rewritten by the next chunk
    }
    if (tid == 0) *nout = run;
}

__global__ __launch_bounds__(kCuThreads) void k_kc_cull(
    const int* __restrict__ ord_row, const int* __restrict__ nord_t, int ccap, int root, int nkf,
    const int* __restrict__ counts, int* __restrict__ kf_mp, int cap, const orbx_keypoint* __restrict__ kps,
    const float* __restrict__ uright, const float* __restrict__ depth, float th_depth, int stereo, int nlevels,
    const uint8_t* __restrict__ noterase, orbm_map_point* __restrict__ pts, const int* __restrict__ obs_ptr,
    const orbm_observation* __restrict__ obs, uint8_t* __restrict__ erased, orbm_observation* __restrict__ ref,
    int* __restrict__ nobs, int nmp, int* __restrict__ claim, int* __restrict__ verdict, int* __restrict__ nmps,
    int* __restrict__ nred, int* __restrict__ culled, int* __restrict__ nculled, int* __restrict__ ncand)
{
    constexpr int T = kCuThreads;
    __shared__ int s_cnt[3];   // nMPs, nRedundantObservations, invalid input
    const int tid = (int)threadIdx.x, sub = tid & (kCuSub - 1), grp = tid / kCuSub;

    const int n = *nord_t;
    if (n < 0 || n > ccap) {   // no candidate list to walk
        for (int j = tid; j < ccap; j += T) culled[j] = -1;
        if (tid == 0) {
            *nculled = 0;
            *ncand = -1;
        }
        return;
    }
    int ncul = 0;
    for (int j = 0; j < n; ++j) {
        const int c = ord_row[j];
        if (tid < 3) s_cnt[tid] = 0;
        __syncthreads();
        int v = ORBM_KFCULL_KEPT;
        const int nc = (c >= 0 && c < nkf) ? counts[c] : -1;
        if (c < 0 || c >= nkf || nc < 0 || nc > cap) v = ORBM_KFCULL_INVALID;
        if (c >= 0 && c == root) v = ORBM_KFCULL_SKIP_ROOT;   // pKF->mnId==0 (:643)
        int NM = 0, NR = 0;
        if (v == ORBM_KFCULL_KEPT) {
            // the count (:651-691): nothing is written
            const size_t row = (size_t)c * cap;
            int my_mps = 0, my_red = 0;
            bool bad = false;
            for (int i = grp; i < nc; i += kCuGroups) {
                const int mp = kf_mp[row + i];
                if (mp < -1 || mp >= nmp) {
                    bad = true;
                    continue;
                }
                if (mp < 0) continue;                           // !pMP (:654)
                // what the tests below read goes out in one round of loads, not one per branch: the candidate is a
                // chain of dependent loads, and its length is the kernel's time
                const int fl = pts[mp].flags, no = nobs[mp], lvl = kps[row + i].octave;
                const float d = stereo ? depth[row + i] : 0.0f;
                int p0, len;
                const bool lok = cu_list(obs_ptr, mp, p0, len);
                if (!(fl & 1)) continue;                        // isBad() (:656)
                if (stereo && (d > th_depth || d < 0.0f)) continue;   // :660
                my_mps += sub == 0;
                if (no <= 3) continue;                          // pMP->Observations()>thObs (:665)
                if (lvl < 0 || lvl >= nlevels || !lok) {
                    bad = true;
                    continue;
                }
                int cnt = 0;
                // no branch in the body, and indices made safe instead: the loop unrolls and the loads of two entries
                // go out together.  idx < cap lies inside the table whatever the KeyFrame's count
#pragma unroll 2
                for (int q = sub; q < len; q += kCuSub) {
                    const bool live = !erased[(size_t)p0 + q];
                    const orbm_observation o = obs[(size_t)p0 + q];
                    const bool in = o.kf >= 0 && o.kf < nkf && o.idx >= 0 && o.idx < cap;
                    const int kf = in ? o.kf : c, idx = in ? o.idx : 0;
                    const int n = counts[kf], li = kps[(size_t)kf * cap + idx].octave;
                    const bool other = in && idx < n && kf != c;           // pKFi==pKF is skipped (:673)
                    bad |= live && (!in || idx >= n || (other && (li < 0 || li >= nlevels)));
                    cnt += live && other && li >= 0 && li < nlevels && li <= lvl + 1;   // :677
                }
                cnt = cu_group_sum(cnt);
                my_red += sub == 0 && cnt >= 3;                 // nObs>=thObs (:684)
            }
            if (my_mps) atomicAdd(s_cnt, my_mps);
            if (my_red) atomicAdd(s_cnt + 1, my_red);
            if (bad) s_cnt[2] = 1;
            __syncthreads();
            NM = s_cnt[0];
            NR = s_cnt[1];
            const bool invalid = s_cnt[2] != 0;
            __syncthreads();   // s_cnt[2] is written again by the check below
            if (invalid) v = ORBM_KFCULL_INVALID;
            else if ((double)NR > 0.9 * (double)NM)             // :693
                v = noterase[c] ? ORBM_KFCULL_TO_BE_ERASED : ORBM_KFCULL_CULLED;   // mbNotErase (KeyFrame.cc:459-463)
        }
        if (v == ORBM_KFCULL_CULLED) {
            // every list the edit walks, before the first write (KeyFrame.cc:469-471 asks no isBad())
            const size_t row = (size_t)c * cap;
            bool bad = false;
            for (int i = grp; i < nc; i += kCuGroups) {
                const int mp = kf_mp[row + i];
                if (mp < 0) continue;
                int p0, len;
                if (!cu_list(obs_ptr, mp, p0, len)) {
                    bad = true;
                    continue;
                }
                for (int q = sub; q < len; q += kCuSub)
                    if (!erased[(size_t)p0 + q] && !cu_obs_ok(obs[(size_t)p0 + q], counts, nkf, cap)) bad = true;
            }
            if (bad) s_cnt[2] = 1;
            __syncthreads();
            if (s_cnt[2]) v = ORBM_KFCULL_INVALID;
        }
        if (v == ORBM_KFCULL_CULLED) {
            const size_t row = (size_t)c * cap;
            for (int i = grp; i < nc; i += kCuGroups) {
                const int mp = kf_mp[row + i];
                if (mp < 0) continue;
                // EraseObservation(pKF) (MapPoint.cc:111-137), once per MapPoint: mObservations.count(pKF) is 0 after
                int own = 0;
                if (sub == 0) own = atomicMax(claim + mp, j + 1) < j + 1;
                own = __shfl(own, (tid & 63) & ~(kCuSub - 1));
                if (!own) continue;
                int p0, len;
                cu_list(obs_ptr, mp, p0, len);
                int first = INT_MAX, rem = INT_MAX;   // the entry of pKF, and mObservations.begin() without it
                for (int q = sub; q < len; q += kCuSub) {
                    if (erased[(size_t)p0 + q]) continue;
                    if (first == INT_MAX && obs[(size_t)p0 + q].kf == c) first = q;
                }
                first = cu_group_min(first);
                if (first == INT_MAX) continue;       // the list lacks the candidate
                for (int q = sub; q < len; q += kCuSub)
                    if (q != first && rem == INT_MAX && !erased[(size_t)p0 + q]) rem = q;
                rem = cu_group_min(rem);
                const int eidx = obs[(size_t)p0 + first].idx;
                const int dec = (uright && uright[row + eidx] >= 0.0f) ? 2 : 1;   // :118-122
                const int left = nobs[mp] - dec;
                if (sub == 0) {
                    erased[(size_t)p0 + first] = 1;                               // mObservations.erase(pKF)
                    nobs[mp] = left;
                    if (rem != INT_MAX && ref[mp].kf == c) ref[mp] = obs[(size_t)p0 + rem];   // :126-127
                    int f = pts[mp].flags;
                    f = left > 0 ? (f | 2) : (f & ~2);
                    if (left <= 2) f &= ~1;                                       // bBad (:130), mbBad=true (:157)
                    pts[mp].flags = f;
                }
                if (left <= 2)
                    for (int q = sub; q < len; q += kCuSub) {                     // SetBadFlag (:151-168)
                        if (q == first || erased[(size_t)p0 + q]) continue;
                        const orbm_observation o = obs[(size_t)p0 + q];
                        kf_mp[(size_t)o.kf * cap + o.idx] = -1;
                        erased[(size_t)p0 + q] = 1;
                    }
            }
        }
        if (tid == 0) {
            verdict[j] = v;
            if (v == ORBM_KFCULL_KEPT || v == ORBM_KFCULL_CULLED || v == ORBM_KFCULL_TO_BE_ERASED) {
                nmps[j] = NM;
                nred[j] = NR;
            }
            culled[j] = v == ORBM_KFCULL_CULLED ? c : -1;
        }
        ncul += v == ORBM_KFCULL_CULLED;
        // the next candidate reads what this one wrote
        __threadfence();
        __syncthreads();
    }
    for (int j = n + tid; j < ccap; j += T) culled[j] = -1;
    if (tid == 0) {
        *nculled = ncul;
        *ncand = n;
    }
}

// ---- the compaction ----

__global__ void k_co_count(const int* __restrict__ obs_ptr, const uint8_t* __restrict__ erased, int nmp,
                           int* __restrict__ out_ptr, int* __restrict__ status)
{
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= nmp) return;
    int p0, len, live = 0;
    if (!cu_list(obs_ptr, m, p0, len)) *status = ORBM_CONN_INVALID;   // compacted as an empty list
    else
        for (int q = 0; q < len; ++q) live += !erased[(size_t)p0 + q];
    out_ptr[m + 1] = live;
}

// the counts at out_ptr[1 .. nmp] become the exclusive scan at out_ptr[0 .. nmp]
__global__ __launch_bounds__(kCuThreads) void k_co_scan(int nmp, int* __restrict__ out_ptr)
{
    constexpr int T = kCuThreads, W = T / 64;
    __shared__ int s_w[W];
    const int tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6;
    int run = 0;
    if (tid == 0) out_ptr[0] = 0;
    for (int c0 = 0; c0 < nmp; c0 += T) {
        const int m = c0 + tid;
        const int v = m < nmp ? out_ptr[m + 1] : 0;
        int x = v;   // inclusive scan inside the wave
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int y = __shfl_up(x, o);
            if (lane >= o) x += y;
        }
        if (lane == 63) s_w[w] = x;
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int q = 0; q < W; ++q) {
            const int a = s_w[q];
            before += q < w ? a : 0;
            total += a;
        }
        if (m < nmp) out_ptr[m + 1] = run + before + x;
        run += total;
        __syncthreads();   // s_w is rewritten by the next chunk
    }
}

__global__ void k_co_scatter(const int* __restrict__ obs_ptr, const orbm_observation* __restrict__ obs,
                             const uint8_t* __restrict__ erased, int nmp, const int* __restrict__ out_ptr,
                             orbm_observation* __restrict__ out)
{
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= nmp) return;
    int p0, len;
    if (!cu_list(obs_ptr, m, p0, len)) return;
    size_t dst = (size_t)out_ptr[m];
    for (int q = 0; q < len; ++q)
        if (!erased[(size_t)p0 + q]) out[dst++] = obs[(size_t)p0 + q];
}

namespace {

bool cu_table_ok(int nkf, int cap, int nmp)
{
    return nkf >= 0 && nkf <= ORBV_DB_MAX_KEYFRAMES && cap > 0 && cap <= ORBM_MAX_FEATURES && nmp >= 0;
}

// obs_ptr ascends from >= 0 (the host forms: the lengths size the uploads)
bool cu_ptr_ok(const int* obs_ptr, int nmp)
{
    if (!obs_ptr || obs_ptr[0] < 0) return false;
    for (int m = 0; m < nmp; ++m)
        if (obs_ptr[m + 1] < obs_ptr[m]) return false;
    return true;
}

}  // namespace

}  // namespace orbx

using namespace orbx;

extern "C" {

orbx_status orbm_map_point_culling_device(const int* d_recent, int nrecent, int cur_kfid, int th_obs,
                                          const int* d_counts, int* d_kf_mp, int nkf, int cap, orbm_map_point* d_pts,
                                          const int* d_obs_ptr, const orbm_observation* d_obs, uint8_t* d_obs_erased,
                                          int nmp, const int* d_nobs, const int* d_found, const int* d_visible,
                                          const int* d_first_kfid, int* d_verdict, int* d_recent_out,
                                          int* d_nrecent_out, void* stream)
{
    if (!cu_table_ok(nkf, cap, nmp) || nrecent < 0 || (nrecent > 0 && (!d_recent || !d_verdict || !d_recent_out)) ||
        !d_counts || !d_kf_mp || !d_pts || !d_obs_ptr || !d_obs || !d_obs_erased || !d_nobs || !d_found ||
        !d_visible || !d_first_kfid || !d_nrecent_out)
        return ORBX_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    if (nrecent > 0)
        hipLaunchKernelGGL(k_mc_verdict, dim3((unsigned)((nrecent + 255) / 256)), dim3(256), 0, s, d_recent, nrecent,
                           cur_kfid, th_obs, d_counts, d_kf_mp, nkf, cap, d_pts, d_obs_ptr, d_obs, d_obs_erased, nmp,
                           d_nobs, d_found, d_visible, d_first_kfid, d_verdict);
    hipLaunchKernelGGL(k_mc_keep, dim3(1), dim3(kCuThreads), 0, s, d_recent, nrecent, d_verdict, d_recent_out,
                       d_nrecent_out);
    return hipGetLastError() == hipSuccess ? ORBX_OK : ORBX_EDEVICE;
}

size_t orbm_culling_work_bytes(int nmp)
{
    if (nmp < 0) return 0;
    return ((size_t)nmp + 1) * sizeof(int);
}

orbx_status orbm_keyframe_culling_device(const orbm_covis_graph* graph, int nkf, int ccap, int t, int root,
                                         const int* d_counts, int* d_kf_mp, int cap, const orbx_keypoint* d_kps,
                                         const float* d_uright, const float* d_depth, float th_depth, int stereo,
                                         int nlevels, const uint8_t* d_kf_noterase, orbm_map_point* d_pts,
                                         const int* d_obs_ptr, const orbm_observation* d_obs, uint8_t* d_obs_erased,
                                         orbm_observation* d_ref, int* d_nobs, int nmp, int* d_verdict, int* d_nmps,
                                         int* d_nred, int* d_culled, int* d_nculled, int* d_ncand, void* d_work,
                                         size_t work_bytes, void* stream)
{
    if (!graph || !graph->ord_kf || !graph->nord || !cu_table_ok(nkf, cap, nmp) || ccap < 1 ||
        ccap > ORBM_MAX_CONNECTIONS || t < 0 || t >= nkf || root < -1 || root >= nkf || nlevels < 1 || nlevels > 16 ||
        !d_counts || !d_kf_mp || !d_kps || (stereo && !d_depth) || !d_kf_noterase || !d_pts || !d_obs_ptr || !d_obs ||
        !d_obs_erased || !d_ref || !d_nobs || !d_verdict || !d_nmps || !d_nred || !d_culled || !d_nculled ||
        !d_ncand || !d_work || ((uintptr_t)d_work & 3) || work_bytes < orbm_culling_work_bytes(nmp))
        return ORBX_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_kc_cull, dim3(1), dim3(kCuThreads), 0, s, graph->ord_kf + (size_t)t * ccap, graph->nord + t,
                       ccap, root, nkf, d_counts, d_kf_mp, cap, d_kps, d_uright, d_depth, th_depth, stereo, nlevels,
                       d_kf_noterase, d_pts, d_obs_ptr, d_obs, d_obs_erased, d_ref, d_nobs, nmp, (int*)d_work,
                       d_verdict, d_nmps, d_nred, d_culled, d_nculled, d_ncand);
    if (hipGetLastError() != hipSuccess) return ORBX_EDEVICE;
    // the claims go back to zero
    if (hipMemsetAsync(d_work, 0, orbm_culling_work_bytes(nmp), s) != hipSuccess) return ORBX_EDEVICE;
    return ORBX_OK;
}

orbx_status orbm_compact_observations_device(const int* d_obs_ptr, const orbm_observation* d_obs,
                                             const uint8_t* d_obs_erased, int nmp, int* d_obs_ptr_out,
                                             orbm_observation* d_obs_out, int* d_status, void* stream)
{
    if (nmp < 0 || !d_obs_ptr || !d_obs || !d_obs_erased || !d_obs_ptr_out || !d_obs_out || !d_status)
        return ORBX_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(d_status, 0, sizeof(int), s) != hipSuccess) return ORBX_EDEVICE;
    const dim3 g((unsigned)std::max(1, (nmp + 255) / 256)), b(256);
    hipLaunchKernelGGL(k_co_count, g, b, 0, s, d_obs_ptr, d_obs_erased, nmp, d_obs_ptr_out, d_status);
    hipLaunchKernelGGL(k_co_scan, dim3(1), dim3(kCuThreads), 0, s, nmp, d_obs_ptr_out);
    hipLaunchKernelGGL(k_co_scatter, g, b, 0, s, d_obs_ptr, d_obs, d_obs_erased, nmp, d_obs_ptr_out, d_obs_out);
    return hipGetLastError() == hipSuccess ? ORBX_OK : ORBX_EDEVICE;
}

orbx_status orbm_map_point_culling(int device, const int* recent, int nrecent, int cur_kfid, int th_obs,
                                   const int* counts, int* kf_mp, int nkf, int cap, orbm_map_point* pts,
                                   const int* obs_ptr, const orbm_observation* obs, uint8_t* obs_erased, int nmp,
                                   const int* nobs, const int* found, const int* visible, const int* first_kfid,
                                   int* verdict, int* recent_out, int* nrecent_out)
{
    if (!cu_table_ok(nkf, cap, nmp) || nkf < 1 || nrecent < 0 || (nrecent > 0 && (!recent || !verdict || !recent_out)) ||
        !counts || !kf_mp || !nrecent_out || !cu_ptr_ok(obs_ptr, nmp) ||
        (nmp > 0 && (!pts || !nobs || !found || !visible || !first_kfid)) ||
        (obs_ptr[nmp] > 0 && (!obs || !obs_erased)))
        return ORBX_EINVAL;
    const size_t K = (size_t)nkf, M = (size_t)nmp, R = (size_t)nrecent, E = (size_t)obs_ptr[nmp];
    HostCall c(device);
    const auto orc = c.in(recent, R);
    const auto ocn = c.in(counts, K);
    const auto okm = c.inout(kf_mp, K * (size_t)cap);
    const auto opt = c.inout(pts, M);
    const auto oop = c.in(obs_ptr, M + 1);
    const auto oob = c.in(obs, E);
    const auto oer = c.inout(obs_erased, E);
    const auto ono = c.in(nobs, M);
    const auto ofo = c.in(found, M);
    const auto ovi = c.in(visible, M);
    const auto ofk = c.in(first_kfid, M);
    // the outputs go up as well: what the call does not write keeps its bits
    const auto ove = c.inout(verdict, R);
    const auto oro = c.inout(recent_out, R);
    const auto onr = c.inout(nrecent_out, 1);
    orbx_status rc = c.begin();
    if (rc != ORBX_OK) return rc;
    rc = orbm_map_point_culling_device(c.dev(orc), nrecent, cur_kfid, th_obs, c.dev(ocn), c.dev(okm), nkf, cap,
                                       c.dev(opt), c.dev(oop), c.dev(oob), c.dev(oer), nmp, c.dev(ono), c.dev(ofo),
                                       c.dev(ovi), c.dev(ofk), c.dev(ove), c.dev(oro), c.dev(onr), c.stream());
    if (rc != ORBX_OK) return rc;
    return c.finish();
}

orbx_status orbm_keyframe_culling(int device, const orbm_covis_graph* graph, int nkf, int ccap, int t, int root,
                                  const int* counts, int* kf_mp, int cap, const orbx_keypoint* kps,
                                  const float* uright, const float* depth, float th_depth, int stereo, int nlevels,
                                  const uint8_t* kf_noterase, orbm_map_point* pts, const int* obs_ptr,
                                  const orbm_observation* obs, uint8_t* obs_erased, orbm_observation* ref, int* nobs,
                                  int nmp, int* verdict, int* nmps, int* nred, int* culled, int* nculled, int* ncand)
{
    if (!graph || !graph->ord_kf || !graph->nord || !cu_table_ok(nkf, cap, nmp) || nkf < 1 || ccap < 1 ||
        ccap > ORBM_MAX_CONNECTIONS || t < 0 || t >= nkf || root < -1 || root >= nkf || nlevels < 1 || nlevels > 16 ||
        !counts || !kf_mp || !kps || (stereo && !depth) || !kf_noterase || !cu_ptr_ok(obs_ptr, nmp) ||
        (nmp > 0 && (!pts || !ref || !nobs)) || (obs_ptr[nmp] > 0 && (!obs || !obs_erased)) || !verdict || !nmps ||
        !nred || !culled || !nculled || !ncand)
        return ORBX_EINVAL;
    const size_t K = (size_t)nkf, M = (size_t)nmp, E = (size_t)obs_ptr[nmp], F = K * (size_t)cap, CC = (size_t)ccap;
    const size_t wbytes = orbm_culling_work_bytes(nmp);
    HostCall c(device);
    const auto ook = c.in(graph->ord_kf, K * CC);
    const auto ono = c.in(graph->nord, K);
    const auto ocn = c.in(counts, K);
    const auto okm = c.inout(kf_mp, F);
    const auto okp = c.in(kps, F);
    const auto our = c.in(uright, uright ? F : 0);
    const auto ode = c.in(depth, depth ? F : 0);
    const auto one = c.in(kf_noterase, K);
    const auto opt = c.inout(pts, M);
    const auto oop = c.in(obs_ptr, M + 1);
    const auto oob = c.in(obs, E);
    const auto orf = c.inout(ref, M);
    const auto onb = c.inout(nobs, M);
    const auto oer = c.inout(obs_erased, E);
    const auto ove = c.inout(verdict, CC);
    const auto onm = c.inout(nmps, CC);
    const auto onr = c.inout(nred, CC);
    const auto ocu = c.inout(culled, CC);
    const auto onc = c.inout(nculled, 1);
    const auto ocd = c.inout(ncand, 1);
    const auto owk = c.out<uint8_t>(wbytes);
    orbx_status rc = c.begin();
    if (rc != ORBX_OK) return rc;
    if (hipMemsetAsync(c.dev(owk), 0, wbytes, c.stream()) != hipSuccess) return ORBX_EDEVICE;
    orbm_covis_graph g;
    std::memset(&g, 0, sizeof g);
    g.ord_kf = c.dev(ook);
    g.nord = c.dev(ono);
    rc = orbm_keyframe_culling_device(&g, nkf, ccap, t, root, c.dev(ocn), c.dev(okm), cap, c.dev(okp),
                                      uright ? c.dev(our) : nullptr, c.dev(ode), th_depth, stereo, nlevels, c.dev(one),
                                      c.dev(opt), c.dev(oop), c.dev(oob), c.dev(oer), c.dev(orf), c.dev(onb), nmp,
                                      c.dev(ove), c.dev(onm), c.dev(onr), c.dev(ocu), c.dev(onc), c.dev(ocd),
                                      c.dev(owk), wbytes, c.stream());
    if (rc != ORBX_OK) return rc;
    return c.finish();
}

orbx_status orbm_compact_observations(int device, const int* obs_ptr, const orbm_observation* obs,
                                      const uint8_t* obs_erased, int nmp, int* obs_ptr_out,
                                      orbm_observation* obs_out, int* status)
{
    if (nmp < 0 || !cu_ptr_ok(obs_ptr, nmp) || !obs_ptr_out || !status ||
        (obs_ptr[nmp] > 0 && (!obs || !obs_erased || !obs_out)))
        return ORBX_EINVAL;
    for (int m = 0; m < nmp; ++m)
        if (obs_ptr[m + 1] - obs_ptr[m] > ORBM_MAX_OBSERVATIONS) return ORBX_EINVAL;
    const size_t M = (size_t)nmp, E = (size_t)obs_ptr[nmp];
    HostCall c(device);
    const auto oop = c.in(obs_ptr, M + 1);
    const auto oob = c.in(obs, E);
    const auto oer = c.in(obs_erased, E);
    const auto opo = c.inout(obs_ptr_out, M + 1);
    const auto ooo = c.inout(obs_out, E);
    const auto ost = c.inout(status, 1);
    orbx_status rc = c.begin();
    if (rc != ORBX_OK) return rc;
    rc = orbm_compact_observations_device(c.dev(oop), c.dev(oob), c.dev(oer), nmp, c.dev(opo), c.dev(ooo), c.dev(ost),
                                          c.stream());
    if (rc != ORBX_OK) return rc;
    return c.finish();
}

}  // extern "C"

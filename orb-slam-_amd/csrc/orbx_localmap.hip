// Tracking::UpdateLocalMap on the device: UpdateLocalKeyFrames (src/Tracking.cc:1283-1391), UpdateLocalPoints
// (:1257-1280) and the first loop of SearchLocalPoints (:1198-1214, with the test at :1222), over the KeyFrame and
// MapPoint tables the refresh and the triangulation keep current.  Its outputs are the inputs of
// orbm_frustum_batch_device and orbm_search_by_projection_device.  Kernels and C entry points (include/orbx.h).
//
// Everything is integers; counters are integer atomics, which commute, so every output is deterministic.
//
// L0 k_lm_invert   (only with d_kf_rank) slot at rank position r, into a table filled with -1 first: a hole left
//                  over means the ranks are no permutation, and every frame is invalid.
// L1/L2 k_lm_select<LDSV>  one workgroup per frame.
//                  votes: one lane per frame feature walks its MapPoint's observation list and adds one to each
//                  KeyFrame (atomics in LDS up to ORBM_LOCAL_MAP_LDS_KEYFRAMES, in the frame's scratch beyond); the frame's
//                  own and outlier MapPoints set their bit in the frame's bitmap (mnLastFrameSeen, :1210).
//                  select: ordered compaction over rank positions (ballot + lane rank, wave totals through LDS) and
//                  the maximum of (votes, lowest rank); then wave 0 runs the expansion, sequential over at most 81
//                  KeyFrames: the 10 covisibles, then 64 children at a time, are tested by the lanes at once and the
//                  first eligible one is taken with a ballot.  The list goes to the frame's scratch, not to the
//                  caller's array: a frame found invalid later must leave no trace.
// L3 k_lm_first    one workgroup per (local KeyFrame k, frame), one lane per feature i: atomic max of
//                  INT_MAX - (k * cap + i) into key[MapPoint].  Zero means untouched, the greatest key is the first
//                  occurrence in list order.
// L4 k_lm_count    per (k, frame) the lanes whose key won, for a MapPoint that is not bad: list entries per KeyFrame.
//    k_lm_gather   per (k, frame): the entries of the KeyFrames before k, an ordered scan of its own in chunks, and the
//                  copy of the orbm_map_point (flags rewritten) and the descriptor (two 16-byte loads and stores).
//    k_lm_finish   puts the touched key and bitmap entries back to zero (cost follows the local map, not the whole
//                  map) and writes what belongs to the frame: the cleaned d_frame_mp, d_claimed, the KeyFrame list,
//                  the reference KeyFrame, the counts and the status.
// Table pointers are kernel arguments of their own: a pointer read from a struct in memory has no address space the
// compiler can see, and becomes flat loads.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstring>

#include "orbx_device.hpp"
#include "orbx_host.hpp"
#include "orbx_kernels.hpp"

namespace orbx {

constexpr int kLmSelThreads = 1024;
constexpr int kLmRowThreads = 256;
constexpr int kLmKfLimit = 80;               // mvpLocalKeyFrames.size()>80 (:1337)
constexpr int kLmHead = kLmKfLimit + 4;      // an expanding list grows to 83 entries at most
constexpr int kLmMaxGridX = 128;
// per-frame header in the scratch
enum { kLmNList = 0, kLmStatus = 1, kLmRef = 2, kLmKeep = 3, kLmTotal = 4, kLmHdr = 8 };

static_assert(ORBM_LOCAL_MAP_LDS_KEYFRAMES * sizeof(int) <= 32768, "the LDS vote counters");

// The caller's scratch of orbm_local_map_device (orbx_localmap.hip), offsets and strides in ints: the rank table
// [nkf], then per frame a header (8), the KeyFrame list [kfcap] and the entries per KeyFrame [kfcap] -- small, and
// cleared by one memset per call (small_bytes) -- then per frame the vote counters [nkf], the first-occurrence keys
// [nmp] and the frame's MapPoint bitmap [(nmp + 31) / 32], which the kernels put back to zero entry by entry.
struct LmLayout {
    size_t inv, hdr, hstride, big, bstride, small_bytes, bytes;
};
static LmLayout lm_layout(int nkf, int nmp, int nframes, int kfcap)
{
    LmLayout L;
    L.inv = 0;
    L.hdr = (size_t)nkf;
    L.hstride = (size_t)kLmHdr + 2 * (size_t)kfcap;
    L.big = L.hdr + L.hstride * (size_t)nframes;
    L.bstride = (size_t)nkf + (size_t)nmp + ((size_t)nmp + 31) / 32;
    L.small_bytes = L.big * sizeof(int);
    L.bytes = (L.big + L.bstride * (size_t)nframes) * sizeof(int);
    return L;
}

__global__ void k_lm_invert(const int* __restrict__ rank, int nkf, int* __restrict__ inv)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nkf) return;
    const int r = rank[f];
    if (r >= 0 && r < nkf) inv[r] = f;
}

template <bool LDSV>
__global__ __launch_bounds__(kLmSelThreads) void k_lm_select(
    const int* __restrict__ fcounts, const int* __restrict__ frame_mp, const int* __restrict__ outlier, int fcap,
    const orbm_map_point* __restrict__ pts, const int* __restrict__ obs_ptr, const orbm_observation* __restrict__ obs,
    int nmp, const uint8_t* __restrict__ kf_bad, const int* __restrict__ inv, const int* __restrict__ covis,
    const int* __restrict__ child_ptr, const int* __restrict__ child, const int* __restrict__ parent, int nkf,
    const int* __restrict__ local_kf, const int* __restrict__ nlocal_kf, int kfcap, int* __restrict__ hdr,
    size_t hstride, int* __restrict__ big, size_t bstride)
{
    constexpr int T = kLmSelThreads, W = T / 64;
    __shared__ int svotes[LDSV ? ORBM_LOCAL_MAP_LDS_KEYFRAMES : 1];
    __shared__ int s_flag[2];   // invalid input, any vote
    __shared__ int s_wtot[W];
    __shared__ unsigned long long s_wmax[W];
    __shared__ int s_head[kLmHead];
    const int fr = blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6;
    int* const hdr_f = hdr + (size_t)fr * hstride;
    int* const list = hdr_f + kLmHdr;
    int* const gvotes = big + (size_t)fr * bstride;
    unsigned* const bitmap = (unsigned*)(gvotes + (size_t)nkf + (size_t)nmp);
    const int* const fmp = frame_mp + (size_t)fr * fcap;
    const int* const fol = outlier ? outlier + (size_t)fr * fcap : nullptr;

    if (tid < 2) s_flag[tid] = 0;
    if (LDSV)
        for (int i = tid; i < nkf; i += T) svotes[i] = 0;
    __syncthreads();

    auto votes_of = [&](int slot) -> int {
        if constexpr (LDSV) return svotes[slot];
        else return __hip_atomic_load(gvotes + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    };

    const int n = fcounts[fr];
    const bool n_ok = n >= 0 && n <= fcap;
    bool bad_in = !n_ok, voted = false;
    if (inv)
        for (int r = tid; r < nkf; r += T) bad_in |= inv[r] < 0;   // the ranks are no permutation
    // every range check comes before the read it guards; a lane that meets a bad index skips what hangs on it
    if (n_ok)
        for (int i = tid; i < n; i += T) {
            const int mp = fmp[i], ol = fol ? fol[i] : -1;
            if (mp < -1 || mp >= nmp || ol < -1 || ol >= nmp) {
                bad_in = true;
                continue;
            }
            if (ol >= 0) atomicOr(bitmap + (ol >> 5), 1u << (ol & 31));   // mnLastFrameSeen (:842, :965)
            if (mp < 0 || !(pts[mp].flags & 1)) continue;                   // NULL, or isBad(): nulled (:1300)
            atomicOr(bitmap + (mp >> 5), 1u << (mp & 31));                  // mnLastFrameSeen (:1210)
            const int p0 = obs_ptr[mp], len = obs_ptr[mp + 1] - p0;
            if (p0 < 0 || len < 0 || len > ORBM_MAX_OBSERVATIONS) {
                bad_in = true;
                continue;
            }
            for (int j = 0; j < len; ++j) {
                const int kf = obs[(size_t)p0 + j].kf;
                if (kf < 0 || kf >= nkf) {
                    bad_in = true;
                    continue;
                }
                if constexpr (LDSV) atomicAdd(svotes + kf, 1);   // keyframeCounter[it->first]++ (:1296)
                else atomicAdd(gvotes + kf, 1);
                voted = true;
            }
        }
    if (bad_in) s_flag[0] = 1;
    if (voted) s_flag[1] = 1;
    if (!LDSV) __threadfence();
    __syncthreads();
    bool invalid = s_flag[0] != 0;
    const bool any = s_flag[1] != 0;
    int nlist = 0, ref = -1, keep = 0, status = 0;

    if (!invalid && !any) {
        // keyframeCounter.empty(): mvpLocalKeyFrames and mpReferenceKF stand (:1305)
        keep = 1;
        const int np = nlocal_kf[fr];
        bool b = np < 0 || np > kfcap;
        if (!b)
            for (int k = tid; k < np; k += T) {
                const int kf = local_kf[(size_t)fr * kfcap + k];
                if (kf < 0 || kf >= nkf) b = true;
                else list[k] = kf;
            }
        if (b) s_flag[0] = 1;
        __syncthreads();
        invalid = s_flag[0] != 0;
        nlist = np;
    } else if (!invalid) {
        // first stage, in rank order (:1315-1330)
        int run = 0;
        unsigned long long best = 0;
        for (int c0 = 0; c0 < nkf; c0 += T) {
            const int r = c0 + tid;
            bool in = false;
            int slot = -1, v = 0;
            if (r < nkf) {
                slot = inv ? inv[r] : r;
                v = votes_of(slot);
                in = v > 0 && !kf_bad[slot];   // pKF->isBad(): continue (:1319)
            }
            const unsigned long long m = __ballot(in);
            if (lane == 0) s_wtot[w] = __popcll(m);
            __syncthreads();
            int before = 0, total = 0;
#pragma unroll
            for (int q = 0; q < W; ++q) {
                const int t = s_wtot[q];
                before += q < w ? t : 0;
                total += t;
            }
            if (in) {
                const int pos = run + before + lanes_below(m);
                if (pos < kLmHead) s_head[pos] = slot;
                if (pos < kfcap) list[pos] = slot;
                // it->second>max (:1322): the most votes, the lowest rank among equals
                const unsigned long long key = ((unsigned long long)(unsigned)v << 32) | (0xFFFFFFFFu - (unsigned)r);
                best = key > best ? key : best;
            }
            run += total;
            __syncthreads();   // s_wtot is rewritten by the next chunk
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long y = __shfl_xor(best, o);
            best = y > best ? y : best;
        }
        if (lane == 0) s_wmax[w] = best;
        __syncthreads();
#pragma unroll
        for (int q = 0; q < W; ++q) best = s_wmax[q] > best ? s_wmax[q] : best;
        if (best) {
            const int r = (int)(0xFFFFFFFFu - (unsigned)best);
            ref = inv ? inv[r] : r;   // pKFmax (:1325)
        }
        const int nfirst = run;
        // expansion (:1334-1384): over the first-stage entries only, by one wave
        if (w == 0) {
            int nn = nfirst;
            bool xbad = false;
            auto listed = [&](int c) -> bool {   // mnTrackReferenceForFrame==mCurrentFrame.mnId
                const int v = votes_of(c);
                if (v > 0 && !kf_bad[c]) return true;
                for (int q = nfirst; q < nn; ++q)
                    if (s_head[q] == c) return true;
                return false;
            };
            auto push = [&](int c) {
                if (lane == 0) {
                    s_head[nn] = c;
                    if (nn < kfcap) list[nn] = c;
                }
                ++nn;
                wave_lds_sync();
            };
            for (int it = 0; it < nfirst && nn <= kLmKfLimit; ++it) {   // size()>80: break (:1337)
                const int kf = s_head[it];
                {   // GetBestCovisibilityKeyFrames(10) (:1342-1356)
                    const int c = lane < 10 ? covis[(size_t)kf * 10 + lane] : -1;
                    const bool cb = c < -1 || c >= nkf;
                    const bool el = c >= 0 && !cb && !kf_bad[c] && !listed(c);
                    if (__ballot(cb)) {
                        xbad = true;
                        break;
                    }
                    const unsigned long long m = __ballot(el);
                    if (m) push(__shfl(c, __ffsll((long long)m) - 1));
                }
                {   // GetChilds() (:1358-1371): every child is range-checked, the first eligible one is taken
                    const int c0 = child_ptr[kf], c1 = child_ptr[kf + 1];
                    if (c0 < 0 || c1 < c0) {
                        xbad = true;
                        break;
                    }
                    int found = -1;
                    for (int b = c0; b < c1; b += 64) {
                        const int j = b + lane;
                        const int c = j < c1 ? child[j] : 0;
                        const bool cb = j < c1 && (c < 0 || c >= nkf);
                        const bool el = j < c1 && !cb && !kf_bad[c] && !listed(c);
                        if (__ballot(cb)) xbad = true;
                        const unsigned long long m = __ballot(el);
                        if (found < 0 && m) found = __shfl(c, __ffsll((long long)m) - 1);
                    }
                    if (xbad) break;
                    if (found >= 0) push(found);
                }
                const int p = parent[kf];   // GetParent() (:1373-1382): isBad() is not asked
                if (p < -1 || p >= nkf) {
                    xbad = true;
                    break;
                }
                if (p >= 0 && !listed(p)) {
                    push(p);
                    break;   // leaves the outer loop (:1380)
                }
            }
            if (lane == 0) {
                s_wtot[0] = nn;
                if (xbad) s_flag[0] = 1;
            }
        }
        __syncthreads();
        invalid = s_flag[0] != 0;
        const int nn = s_wtot[0];
        nlist = min(nn, kfcap);
        if (nn > kfcap) status |= ORBM_LOCAL_MAP_KF_TRUNCATED;
    }

    if (!LDSV && n_ok) {   // the counters go back to zero: the same walk, the same checks
        __syncthreads();
        for (int i = tid; i < n; i += T) {
            const int mp = fmp[i];
            if (mp < 0 || mp >= nmp || !(pts[mp].flags & 1)) continue;
            const int p0 = obs_ptr[mp], len = obs_ptr[mp + 1] - p0;
            if (p0 < 0 || len < 0 || len > ORBM_MAX_OBSERVATIONS) continue;
            for (int j = 0; j < len; ++j) {
                const int kf = obs[(size_t)p0 + j].kf;
                if (kf >= 0 && kf < nkf) gvotes[kf] = 0;
            }
        }
    }
    if (tid == 0) {
        hdr_f[kLmNList] = invalid ? 0 : nlist;
        hdr_f[kLmStatus] = invalid ? ORBM_LOCAL_MAP_INVALID : status;
        hdr_f[kLmRef] = ref;
        hdr_f[kLmKeep] = keep;
        hdr_f[kLmTotal] = 0;
    }
}

// the walk L3, L4 and the cleanup share: local KeyFrame k of frame fr, its count checked
struct LmRow {
    int kf, cnt;
};

__device__ __forceinline__ LmRow lm_row(const int* __restrict__ list, int k, const int* __restrict__ counts, int cap)
{
    LmRow r;
    r.kf = list[k];   // in [0, nkf): k_lm_select checked it
    r.cnt = counts[r.kf];
    if (r.cnt < 0 || r.cnt > cap) r.cnt = -1;
    return r;
}

__global__ __launch_bounds__(kLmRowThreads) void k_lm_first(
    const int* __restrict__ counts, const int* __restrict__ kf_mp, int cap, int nmp, int nframes, int kfcap,
    int* __restrict__ hdr, size_t hstride, int* __restrict__ big, size_t bstride, int nkf)
{
    const int tid = (int)threadIdx.x;
    for (int fr = blockIdx.y; fr < nframes; fr += gridDim.y) {
        int* const hdr_f = hdr + (size_t)fr * hstride;
        const int* const list = hdr_f + kLmHdr;
        int* const key = big + (size_t)fr * bstride + (size_t)nkf;
        const int nlist = hdr_f[kLmNList];
        for (int k = blockIdx.x; k < nlist; k += gridDim.x) {
            const LmRow R = lm_row(list, k, counts, cap);
            bool bad = R.cnt < 0;
            for (int i = tid; i < R.cnt; i += kLmRowThreads) {
                const int mp = kf_mp[(size_t)R.kf * cap + i];
                if (mp < -1 || mp >= nmp) bad = true;
                else if (mp >= 0) atomicMax(key + mp, INT_MAX - (k * cap + i));
            }
            if (bad) atomicOr(hdr_f + kLmStatus, (int)ORBM_LOCAL_MAP_INVALID);
        }
    }
}

// does (k, i) put its MapPoint on the list: the first occurrence (:1271) of a MapPoint that is not bad (:1273)
__device__ __forceinline__ bool lm_entry(int mp, int nmp, const int* __restrict__ key, int mykey,
                                         const orbm_map_point* __restrict__ pts)
{
    return mp >= 0 && mp < nmp && key[mp] == mykey && (pts[mp].flags & 1);
}

__global__ __launch_bounds__(kLmRowThreads) void k_lm_count(
    const int* __restrict__ counts, const int* __restrict__ kf_mp, int cap, const orbm_map_point* __restrict__ pts,
    int nmp, int nframes, int kfcap, int* __restrict__ hdr, size_t hstride, const int* __restrict__ big,
    size_t bstride, int nkf)
{
    __shared__ int s_w[kLmRowThreads / 64];
    const int tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6;
    for (int fr = blockIdx.y; fr < nframes; fr += gridDim.y) {
        int* const hdr_f = hdr + (size_t)fr * hstride;
        const int* const list = hdr_f + kLmHdr;
        int* const cnt = hdr_f + kLmHdr + kfcap;
        const int* const key = big + (size_t)fr * bstride + (size_t)nkf;
        if (hdr_f[kLmStatus] & ORBM_LOCAL_MAP_INVALID) continue;
        const int nlist = hdr_f[kLmNList];
        for (int k = blockIdx.x; k < nlist; k += gridDim.x) {
            const LmRow R = lm_row(list, k, counts, cap);
            int c = 0;
            for (int i = tid; i < R.cnt; i += kLmRowThreads)
                c += lm_entry(kf_mp[(size_t)R.kf * cap + i], nmp, key, INT_MAX - (k * cap + i), pts);
            c = wave_sum(c);
            if (lane == 0) s_w[w] = c;
            __syncthreads();
            if (tid == 0) cnt[k] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(kLmRowThreads) void k_lm_gather(
    const int* __restrict__ counts, const int* __restrict__ kf_mp, int cap, const orbm_map_point* __restrict__ pts,
    const ulonglong2* __restrict__ pdesc, int nmp, int nframes, int kfcap, int* __restrict__ hdr, size_t hstride,
    const int* __restrict__ big, size_t bstride, int nkf, int* __restrict__ local_mp,
    orbm_map_point* __restrict__ out_pts, ulonglong2* __restrict__ out_pdesc, int pcap)
{
    constexpr int W = kLmRowThreads / 64;
    __shared__ int s_w[W];
    const int tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6;
    for (int fr = blockIdx.y; fr < nframes; fr += gridDim.y) {
        int* const hdr_f = hdr + (size_t)fr * hstride;
        const int* const list = hdr_f + kLmHdr;
        const int* const cnt = hdr_f + kLmHdr + kfcap;
        const int* const key = big + (size_t)fr * bstride + (size_t)nkf;
        const unsigned* const bitmap = (const unsigned*)(key + (size_t)nmp);
        if (hdr_f[kLmStatus] & ORBM_LOCAL_MAP_INVALID) continue;
        const int nlist = hdr_f[kLmNList];
        for (int k = blockIdx.x; k < nlist; k += gridDim.x) {
            // the entries of the KeyFrames before k: at most kfcap * cap, which fits an int
            int part = 0;
            for (int j = tid; j < k; j += kLmRowThreads) part += cnt[j];
            part = wave_sum(part);
            if (lane == 0) s_w[w] = part;
            __syncthreads();
            int run = 0;
#pragma unroll
            for (int q = 0; q < W; ++q) run += s_w[q];
            __syncthreads();
            const LmRow R = lm_row(list, k, counts, cap);
            for (int c0 = 0; c0 < R.cnt && run < pcap; c0 += kLmRowThreads) {
                const int i = c0 + tid;
                const bool live = i < R.cnt;   // a lane past the count forms no position: k * cap + i may not fit
                const int mp = live ? kf_mp[(size_t)R.kf * cap + i] : -1;
                const bool e = lm_entry(mp, nmp, key, INT_MAX - (k * cap + (live ? i : 0)), pts);
                const unsigned long long m = __ballot(e);
                if (lane == 0) s_w[w] = __popcll(m);
                __syncthreads();
                int before = 0, total = 0;
#pragma unroll
                for (int q = 0; q < W; ++q) {
                    const int t = s_w[q];
                    before += q < w ? t : 0;
                    total += t;
                }
                const int pos = run + before + lanes_below(m);
                if (e && pos < pcap) {
                    const size_t o = (size_t)fr * pcap + pos;
                    orbm_map_point p = pts[mp];
                    // mnLastFrameSeen == mCurrentFrame.mnId: continue (:1222)
                    const int seen = (bitmap[mp >> 5] >> (mp & 31)) & 1u;
                    p.flags = (seen ? 0 : 1) | (p.flags & 2);
                    out_pts[o] = p;
                    out_pdesc[2 * o] = pdesc[2 * (size_t)mp];
                    out_pdesc[2 * o + 1] = pdesc[2 * (size_t)mp + 1];
                    local_mp[o] = mp;
                }
                run += total;
                __syncthreads();   // s_w is rewritten by the next chunk
            }
        }
        if (blockIdx.x == 0 && tid == 0) {   // mvpLocalMapPoints.size(), uncut (no other block reads it here)
            int total = 0;
            for (int j = 0; j < nlist; ++j) total += cnt[j];
            hdr_f[kLmTotal] = total;
        }
    }
}

__global__ __launch_bounds__(kLmRowThreads) void k_lm_finish(
    const int* __restrict__ counts, const int* __restrict__ kf_mp, int cap, const orbm_map_point* __restrict__ pts,
    int nmp, int nframes, int kfcap, const int* __restrict__ hdr, size_t hstride, int* __restrict__ big,
    size_t bstride, int nkf, const int* __restrict__ fcounts, int* __restrict__ frame_mp,
    const int* __restrict__ outlier, int fcap, int* __restrict__ local_kf, int* __restrict__ nlocal_kf,
    int* __restrict__ ref_kf, int* __restrict__ nlocal, int pcap, uint8_t* __restrict__ claimed,
    int* __restrict__ status)
{
    const int tid = (int)threadIdx.x;
    for (int fr = blockIdx.y; fr < nframes; fr += gridDim.y) {
        const int* const hdr_f = hdr + (size_t)fr * hstride;
        const int* const list = hdr_f + kLmHdr;
        int* const key = big + (size_t)fr * bstride + (size_t)nkf;
        unsigned* const bitmap = (unsigned*)(key + (size_t)nmp);
        const int nlist = hdr_f[kLmNList];
        for (int k = blockIdx.x; k < nlist; k += gridDim.x) {   // the keys k_lm_first touched
            const LmRow R = lm_row(list, k, counts, cap);
            for (int i = tid; i < R.cnt; i += kLmRowThreads) {
                const int mp = kf_mp[(size_t)R.kf * cap + i];
                if (mp >= 0 && mp < nmp) key[mp] = 0;
            }
        }
        if (blockIdx.x != 0) continue;
        const int st = hdr_f[kLmStatus];
        const bool valid = !(st & ORBM_LOCAL_MAP_INVALID);
        const int n = fcounts[fr];
        if (n >= 0 && n <= fcap) {
            int* const fmp = frame_mp + (size_t)fr * fcap;
            const int* const fol = outlier ? outlier + (size_t)fr * fcap : nullptr;
            for (int i = tid; i < n; i += kLmRowThreads) {
                const int mp = fmp[i], ol = fol ? fol[i] : -1;
                if (ol >= 0 && ol < nmp) bitmap[ol >> 5] = 0;
                const bool in = mp >= 0 && mp < nmp;
                if (in) bitmap[mp >> 5] = 0;
                if (!valid) continue;   // every index of a valid frame is in range
                const int fl = in ? pts[mp].flags : 0;
                if (in && !(fl & 1)) fmp[i] = -1;   // mCurrentFrame.mvpMapPoints[i]=NULL (:1300, :1205)
                claimed[(size_t)fr * fcap + i] = (fl & 3) == 3;
            }
        }
        const int total = hdr_f[kLmTotal];
        if (valid) {
            if (!hdr_f[kLmKeep]) {
                for (int k = tid; k < nlist; k += kLmRowThreads) local_kf[(size_t)fr * kfcap + k] = list[k];
                if (tid == 0) nlocal_kf[fr] = nlist;
            }
            if (tid == 0) {
                if (hdr_f[kLmRef] >= 0) ref_kf[fr] = hdr_f[kLmRef];   // if(pKFmax) (:1386)
                nlocal[fr] = min(total, pcap);
            }
        }
        if (tid == 0)
            status[fr] = valid ? (st | (total > pcap ? (int)ORBM_LOCAL_MAP_POINTS_TRUNCATED : 0))
                               : (int)ORBM_LOCAL_MAP_INVALID;
    }
}

namespace {

bool lm_dims_ok(int nkf, int cap, int nmp, int nframes, int fcap, int kfcap, int pcap)
{
    return nkf >= 0 && nkf <= ORBV_DB_MAX_KEYFRAMES && nmp >= 0 && nframes >= 0 && cap > 0 &&
           cap <= ORBM_MAX_FEATURES && fcap > 0 && fcap <= ORBM_MAX_FEATURES && kfcap > 0 && pcap > 0 &&
           (long long)kfcap * (long long)cap <= (long long)INT_MAX;
}

}  // namespace

}  // namespace orbx

using namespace orbx;

extern "C" {

size_t orbm_local_map_work_bytes(int nkf, int nmp, int nframes, int kfcap)
{
    if (nkf < 0 || nkf > ORBV_DB_MAX_KEYFRAMES || nmp < 0 || nframes < 0 || kfcap <= 0) return 0;
    return std::max<size_t>(lm_layout(nkf, nmp, nframes, kfcap).bytes, 64);
}

orbx_status orbm_local_map_device(const int* d_counts, const int* d_kf_mp, const uint8_t* d_kf_bad,
                                  const int* d_kf_rank, const int* d_covis, const int* d_child_ptr,
                                  const int* d_child, const int* d_parent, int nkf, int cap,
                                  const orbm_map_point* d_pts, const uint8_t* d_pdesc, const int* d_obs_ptr,
                                  const orbm_observation* d_obs, int nmp, const int* d_fcounts, int* d_frame_mp,
                                  const int* d_frame_outlier, int nframes, int fcap, int* d_local_kf,
                                  int* d_nlocal_kf, int kfcap, int* d_ref_kf, int* d_local_mp, int* d_nlocal,
                                  orbm_map_point* d_out_pts, uint8_t* d_out_pdesc, int pcap, uint8_t* d_claimed,
                                  int* d_status, void* d_work, size_t work_bytes, void* stream)
{
    if (!lm_dims_ok(nkf, cap, nmp, nframes, fcap, kfcap, pcap) || !d_counts || !d_kf_mp || !d_kf_bad || !d_covis ||
        !d_child_ptr || !d_child || !d_parent || !d_pts || !d_pdesc || !d_obs_ptr || !d_obs || !d_fcounts ||
        !d_frame_mp || !d_local_kf || !d_nlocal_kf || !d_ref_kf || !d_local_mp || !d_nlocal || !d_out_pts ||
        !d_out_pdesc || !d_claimed || !d_status || !d_work || ((uintptr_t)d_work & 3) ||
        work_bytes < orbm_local_map_work_bytes(nkf, nmp, nframes, kfcap))
        return ORBX_EINVAL;
    if (nframes == 0) return ORBX_OK;
    hipStream_t s = (hipStream_t)stream;
    const LmLayout L = lm_layout(nkf, nmp, nframes, kfcap);
    int* const wk = (int*)d_work;
    int* const hdr = wk + L.hdr;
    int* const big = wk + L.big;
    const int* inv = nullptr;
    if (d_kf_rank && nkf > 0) {
        if (hipMemsetAsync(wk + L.inv, 0xFF, sizeof(int) * (size_t)nkf, s) != hipSuccess) return ORBX_EDEVICE;
        hipLaunchKernelGGL(k_lm_invert, dim3((unsigned)((nkf + 255) / 256)), dim3(256), 0, s, d_kf_rank, nkf,
                           wk + L.inv);
        inv = wk + L.inv;
    }
    const dim3 gsel((unsigned)nframes);
    if (nkf <= ORBM_LOCAL_MAP_LDS_KEYFRAMES)
        hipLaunchKernelGGL(k_lm_select<true>, gsel, dim3(kLmSelThreads), 0, s, d_fcounts, d_frame_mp, d_frame_outlier,
                           fcap, d_pts, d_obs_ptr, d_obs, nmp, d_kf_bad, inv, d_covis, d_child_ptr, d_child, d_parent,
                           nkf, d_local_kf, d_nlocal_kf, kfcap, hdr, L.hstride, big, L.bstride);
    else
        hipLaunchKernelGGL(k_lm_select<false>, gsel, dim3(kLmSelThreads), 0, s, d_fcounts, d_frame_mp,
                           d_frame_outlier, fcap, d_pts, d_obs_ptr, d_obs, nmp, d_kf_bad, inv, d_covis, d_child_ptr,
                           d_child, d_parent, nkf, d_local_kf, d_nlocal_kf, kfcap, hdr, L.hstride, big, L.bstride);
    const dim3 grow((unsigned)std::min(kfcap, kLmMaxGridX), (unsigned)std::min(nframes, 65535));
    hipLaunchKernelGGL(k_lm_first, grow, dim3(kLmRowThreads), 0, s, d_counts, d_kf_mp, cap, nmp, nframes, kfcap, hdr,
                       L.hstride, big, L.bstride, nkf);
    hipLaunchKernelGGL(k_lm_count, grow, dim3(kLmRowThreads), 0, s, d_counts, d_kf_mp, cap, d_pts, nmp, nframes, kfcap,
                       hdr, L.hstride, big, L.bstride, nkf);
    hipLaunchKernelGGL(k_lm_gather, grow, dim3(kLmRowThreads), 0, s, d_counts, d_kf_mp, cap, d_pts,
                       (const ulonglong2*)d_pdesc, nmp, nframes, kfcap, hdr, L.hstride, big, L.bstride, nkf,
                       d_local_mp, d_out_pts, (ulonglong2*)d_out_pdesc, pcap);
    hipLaunchKernelGGL(k_lm_finish, grow, dim3(kLmRowThreads), 0, s, d_counts, d_kf_mp, cap, d_pts, nmp, nframes,
                       kfcap, hdr, L.hstride, big, L.bstride, nkf, d_fcounts, d_frame_mp, d_frame_outlier, fcap,
                       d_local_kf, d_nlocal_kf, d_ref_kf, d_nlocal, pcap, d_claimed, d_status);
    if (hipGetLastError() != hipSuccess) return ORBX_EDEVICE;
    // the rank table, the headers and the lists: small, and zero again like the rest
    if (hipMemsetAsync(wk, 0, L.small_bytes, s) != hipSuccess) return ORBX_EDEVICE;
    return ORBX_OK;
}

orbx_status orbm_local_map(int device, const int* counts, const int* kf_mp, const uint8_t* kf_bad, const int* kf_rank,
                           const int* covis, const int* child_ptr, const int* child, const int* parent, int nkf,
                           int cap, const orbm_map_point* pts, const uint8_t* pdesc, const int* obs_ptr,
                           const orbm_observation* obs, int nmp, int n, int* frame_mp, const int* frame_outlier,
                           int* local_kf, int* nlocal_kf, int kfcap, int* ref_kf, int* local_mp, int* nlocal,
                           orbm_map_point* out_pts, uint8_t* out_pdesc, int pcap, uint8_t* claimed, int* status)
{
    const int fcap = std::max(n, 1);
    if (n < 0 || !lm_dims_ok(nkf, cap, nmp, 1, fcap, kfcap, pcap) || !child_ptr || !obs_ptr || !local_kf ||
        !nlocal_kf || !ref_kf || !local_mp || !nlocal || !out_pts || !out_pdesc || !status ||
        (n > 0 && (!frame_mp || !claimed)) || (nkf > 0 && (!counts || !kf_mp || !kf_bad || !covis || !parent)) ||
        (nmp > 0 && (!pts || !pdesc)))
        return ORBX_EINVAL;
    if (child_ptr[0] < 0 || obs_ptr[0] < 0) return ORBX_EINVAL;
    for (int f = 0; f < nkf; ++f)
        if (child_ptr[f + 1] < child_ptr[f]) return ORBX_EINVAL;
    for (int m = 0; m < nmp; ++m)
        if (obs_ptr[m + 1] < obs_ptr[m]) return ORBX_EINVAL;
    if ((child_ptr[nkf] > 0 && !child) || (obs_ptr[nmp] > 0 && !obs)) return ORBX_EINVAL;
    const size_t wbytes = orbm_local_map_work_bytes(nkf, nmp, 1, kfcap);
    const size_t K = (size_t)nkf, M = (size_t)nmp, N = (size_t)n;
    HostCall c(device);
    const auto ofc = c.in(&n, 1);   // d_fcounts
    const auto ocn = c.in(counts, K);
    const auto okm = c.in(kf_mp, K * (size_t)cap);
    const auto okb = c.in(kf_bad, K);
    const auto okr = c.in(kf_rank, kf_rank ? K : 0);
    const auto ocv = c.in(covis, 10 * K);
    const auto ocp = c.in(child_ptr, K + 1);
    const auto och = c.in(child, (size_t)child_ptr[nkf]);
    const auto opa = c.in(parent, K);
    const auto opt = c.in(pts, M);
    const auto opd = c.in(pdesc, 32 * M);
    const auto oop = c.in(obs_ptr, M + 1);
    const auto oob = c.in(obs, (size_t)obs_ptr[nmp]);
    const auto ofo = c.in(frame_outlier, frame_outlier ? N : 0);
    // outputs go up as well: what the call does not write keeps its bits
    const auto ofm = c.inout(frame_mp, N);
    const auto ocl = c.inout(claimed, N);
    const auto olk = c.inout(local_kf, (size_t)kfcap);
    const auto onk = c.inout(nlocal_kf, 1);
    const auto ork = c.inout(ref_kf, 1);
    const auto olm = c.inout(local_mp, (size_t)pcap);
    const auto oop2 = c.inout(out_pts, (size_t)pcap);
    const auto ood = c.inout(out_pdesc, 32 * (size_t)pcap);
    const auto onl = c.inout(nlocal, 1);
    const auto ost = c.inout(status, 1);
    const auto owk = c.out<uint8_t>(wbytes);
    orbx_status rc = c.begin();
    if (rc != ORBX_OK) return rc;
    if (hipMemsetAsync(c.dev(owk), 0, wbytes, c.stream()) != hipSuccess) return ORBX_EDEVICE;
    rc = orbm_local_map_device(c.dev(ocn), c.dev(okm), c.dev(okb), kf_rank && nkf > 0 ? c.dev(okr) : nullptr,
                               c.dev(ocv), c.dev(ocp), c.dev(och), c.dev(opa), nkf, cap, c.dev(opt), c.dev(opd),
                               c.dev(oop), c.dev(oob), nmp, c.dev(ofc), c.dev(ofm),
                               frame_outlier && n > 0 ? c.dev(ofo) : nullptr, 1, fcap, c.dev(olk), c.dev(onk), kfcap,
                               c.dev(ork), c.dev(olm), c.dev(onl), c.dev(oop2), c.dev(ood), pcap, c.dev(ocl),
                               c.dev(ost), c.dev(owk), wbytes, c.stream());
    if (rc != ORBX_OK) return rc;
    return c.finish();
}

}  // extern "C"

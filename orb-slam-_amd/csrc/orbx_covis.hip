// The covisibility graph on the device: KeyFrame::UpdateConnections (src/KeyFrame.cc:289-379) with AddConnection
// (:123-136) and UpdateBestCovisibles (:138-157), the connection part of SetBadFlag (:466-467, :476-477) with
// EraseConnection (:553-567), and the getters the other tables are fed from: GetBestCovisibilityKeyFrames (:174-182),
// GetConnectedKeyFrames (:159-166), GetCovisiblesByWeight (:184-199) and GetChilds.  Kernels and C entry points
// (include/orbx.h).
//
// Everything is integers; counters are integer atomics, which commute, so every output is deterministic.
//
// The targets run one after another on the stream, each as two launches, so that a target reads the rows the one
// before it wrote:
// C0 k_cv_rankcheck      (only with d_kf_rank, once per call) one counter per rank position: a rank out of range or
//                        met twice means the ranks are no permutation, and every target is invalid.
// C1 k_cv_vote<LDSV>     one 1,024-lane workgroup.  votes: one lane per feature walks its MapPoint's observation
//                        list and adds one to each KeyFrame but the target (atomics in LDS up to
//                        ORBM_LOCAL_MAP_LDS_KEYFRAMES, in the scratch beyond).  select: two ordered compactions over
//                        the slots (ballot + lane rank, wave totals through LDS): every voted KeyFrame with its count,
//                        which is the target's map row, and those at or above th, which are vPairs; the maximum of
//                        (votes, lowest rank) is pKFmax.  check: one wave per vPairs neighbour reads its map row,
//                        every entry range-checked, and learns whether the target is in it and whether an insert
//                        fits.  The status is decided here, before the first write to the graph.
// C2 k_cv_apply          one workgroup per vPairs neighbour, and one for the target's own rows.  A neighbour's map row
//                        goes to LDS as 64-bit keys (weight << 32 | rank << 16 | slot) in slot order with the
//                        target's entry inserted or overwritten; the shifted tail is written back, the keys are
//                        sorted descending by a bitonic network, and the ordered rows are written from them.  Equal
//                        weight: nothing is touched.  The position of the target in a row is the count of smaller
//                        slots, taken while the row is loaded: the whole row is read for the sort anyway.
// E1 k_cv_erase_check / E2 k_cv_erase_apply   the same split for EraseConnection.
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

constexpr int kCvVoteThreads = 1024;
constexpr int kCvRowThreads = 256;
constexpr int kCvMaxGrid = 256;
// header of the scratch
enum { kCvNV = 1, kCvNP = 2, kCvT = 3, kCvRankBad = 4, kCvGo = 5, kCvHdr = 16 };

static_assert(ORBM_MAX_CONNECTIONS * sizeof(long long) <= 32768, "the LDS sort keys");
static_assert(ORBV_DB_MAX_KEYFRAMES <= 65536, "rank and slot share the low word of a sort key");

struct CvLayout {
    size_t dup, votes, m_kf, m_w, p_kf, p_w, small_bytes, bytes;
};

static CvLayout cv_layout(int nkf, int ccap)
{
    CvLayout L;
    L.dup = kCvHdr;
    L.m_kf = L.dup + (size_t)nkf;
    L.m_w = L.m_kf + (size_t)ccap;
    L.p_kf = L.m_w + (size_t)ccap;
    L.p_w = L.p_kf + (size_t)ccap;
    L.votes = L.p_w + (size_t)ccap;   // last: the vote kernel puts its own counters back
    L.small_bytes = L.votes * sizeof(int);
    L.bytes = (L.votes + (size_t)nkf) * sizeof(int);
    return L;
}

__device__ __forceinline__ long long cv_key(int w, int rank, int slot)
{
    return (long long)(((unsigned long long)(unsigned)w << 32) | ((unsigned long long)(unsigned)rank << 16) |
                       (unsigned long long)(unsigned)slot);
}
__device__ __forceinline__ int cv_key_slot(long long k) { return (int)((unsigned long long)k & 0xFFFFull); }
__device__ __forceinline__ int cv_key_w(long long k) { return (int)(k >> 32); }

__global__ void k_cv_rankcheck(const int* __restrict__ rank, int nkf, int* __restrict__ dup, int* __restrict__ hdr)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nkf) return;
    const int r = rank[f];
    if (r < 0 || r >= nkf || atomicAdd(dup + r, 1) != 0) hdr[kCvRankBad] = 1;
}

template <bool LDSV>
__global__ __launch_bounds__(kCvVoteThreads) void k_cv_vote(
    const int* __restrict__ targets, int ti, const int* __restrict__ counts, const int* __restrict__ kf_mp, int cap,
    const int* __restrict__ rank, const orbm_map_point* __restrict__ pts, const int* __restrict__ obs_ptr,
    const orbm_observation* __restrict__ obs, int nmp, int nkf, int ccap, int th, const int* __restrict__ conn_kf,
    const int* __restrict__ nconn, int* __restrict__ hdr, int* __restrict__ gvotes, int* __restrict__ m_kf,
    int* __restrict__ m_w, int* __restrict__ p_kf, int* __restrict__ p_w, int* __restrict__ status)
{
    constexpr int T = kCvVoteThreads, W = T / 64;
    __shared__ int svotes[LDSV ? ORBM_LOCAL_MAP_LDS_KEYFRAMES : 1];
    __shared__ int s_flag[3];   // invalid input, any vote, no room
    __shared__ int s_wtot[2][W];
    __shared__ unsigned long long s_wmax[W];
    const int tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6;

    if (tid < 3) s_flag[tid] = 0;
    if (LDSV)
        for (int i = tid; i < nkf; i += T) svotes[i] = 0;
    __syncthreads();

    auto votes_of = [&](int slot) -> int {
        if constexpr (LDSV) return svotes[slot];
        else return __hip_atomic_load(gvotes + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    };

    const int t = targets[ti];
    const bool t_ok = t >= 0 && t < nkf;
    const int n = t_ok ? counts[t] : -1;
    const bool n_ok = n >= 0 && n <= cap;
    const int* const fmp = kf_mp + (size_t)(t_ok ? t : 0) * cap;
    bool bad_in = false, voted = false;
    // every range check comes before the read it guards; a lane that meets a bad index skips what hangs on it
    if (n_ok)
        for (int i = tid; i < n; i += T) {
            const int mp = fmp[i];
            if (mp < -1 || mp >= nmp) {
                bad_in = true;
                continue;
            }
            if (mp < 0 || !(pts[mp].flags & 1)) continue;   // !pMP, or isBad() (:306-310)
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
                if (kf == t) continue;   // mit->first->mnId==mnId (:316)
                if constexpr (LDSV) atomicAdd(svotes + kf, 1);   // KFcounter[mit->first]++ (:318)
                else atomicAdd(gvotes + kf, 1);
                voted = true;
            }
        }
    if (bad_in) s_flag[0] = 1;
    if (voted) s_flag[1] = 1;
    if (!LDSV) __threadfence();
    __syncthreads();
    bool invalid = s_flag[0] != 0 || !n_ok || hdr[kCvRankBad] != 0;
    const bool any = s_flag[1] != 0;
    int nv = 0, np = 0;

    if (!invalid && any) {
        // the map row in slot order, vPairs beside it, and pKFmax (:328-352)
        int run = 0, run2 = 0;
        unsigned long long best = 0;
        for (int c0 = 0; c0 < nkf; c0 += T) {
            const int slot = c0 + tid;
            const int v = slot < nkf ? votes_of(slot) : 0;
            const bool in = v > 0, in2 = v >= th;
            const unsigned long long m = __ballot(in), m2 = __ballot(in2);
            if (lane == 0) {
                s_wtot[0][w] = __popcll(m);
                s_wtot[1][w] = __popcll(m2);
            }
            __syncthreads();
            int before = 0, total = 0, before2 = 0, total2 = 0;
#pragma unroll
            for (int q = 0; q < W; ++q) {
                const int a = s_wtot[0][q], b = s_wtot[1][q];
                before += q < w ? a : 0;
                total += a;
                before2 += q < w ? b : 0;
                total2 += b;
            }
            if (in) {
                const int pos = run + before + lanes_below(m);
                if (pos < ccap) {
                    m_kf[pos] = slot;
                    m_w[pos] = v;
                }
                // mit->second>nmax (:336): the most votes, the lowest rank among equals
                const unsigned r = (unsigned)(rank ? rank[slot] : slot);
                const unsigned long long key =
                    ((unsigned long long)(unsigned)v << 32) | ((unsigned long long)(0xFFFFu - r) << 16) | (unsigned)slot;
                best = key > best ? key : best;
            }
            if (in2) {
                const int pos = run2 + before2 + lanes_below(m2);
                if (pos < ccap) {
                    p_kf[pos] = slot;
                    p_w[pos] = v;
                }
            }
            run += total;
            run2 += total2;
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
        nv = run;
        np = run2;
        if (np == 0) {   // vPairs.empty(): pKFmax alone (:348-352)
            np = 1;
            if (tid == 0) {
                p_kf[0] = (int)(best & 0xFFFFull);
                p_w[0] = (int)(best >> 32);
            }
        }
        __syncthreads();
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

    const bool full = nv > ccap;
    if (!invalid && any && !full) {
        // the map row of every neighbour that receives AddConnection: its count, every entry, the target's presence
        for (int q = w; q < np; q += W) {
            const int nb = p_kf[q];
            const int nc = nconn[nb];
            if (nc < 0 || nc > ccap) {
                if (lane == 0) s_flag[0] = 1;
                continue;
            }
            bool rb = false, present = false;
            for (int j = lane; j < nc; j += 64) {
                const int e = conn_kf[(size_t)nb * ccap + j];
                rb |= e < 0 || e >= nkf;
                present |= e == t;
            }
            const bool anyb = __ballot(rb) != 0, anyp = __ballot(present) != 0;
            if (lane == 0) {
                if (anyb) s_flag[0] = 1;
                else if (!anyp && nc == ccap) s_flag[2] = 1;
            }
        }
        __syncthreads();
        invalid = s_flag[0] != 0;
    }
    if (tid == 0) {
        int st = 0;
        if (invalid) st = ORBM_CONN_INVALID;
        else if (!any) st = ORBM_CONN_EMPTY;
        else if (full || s_flag[2]) st = ORBM_CONN_NOSPC;
        hdr[kCvNV] = nv;
        hdr[kCvNP] = np;
        hdr[kCvT] = t;
        hdr[kCvGo] = st == 0;
        if (st != 0) status[ti] = st;
    }
}

// descending bitonic sort of P (a power of two) keys in LDS, by the whole workgroup
__device__ __forceinline__ void cv_sort_desc(long long* keys, int P, int tid, int T)
{
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < P; i += T) {
                const int l = i ^ j;
                if (l > i) {
                    const long long a = keys[i], b = keys[l];
                    const bool desc = (i & k) == 0;
                    if (desc ? a < b : a > b) {
                        keys[i] = b;
                        keys[l] = a;
                    }
                }
            }
            __syncthreads();
        }
}

// keys[0, cnt) -> padded, sorted, written as the ordered rows of KeyFrame f (UpdateBestCovisibles, :138-157)
__device__ __forceinline__ void cv_write_ordered(long long* keys, int cnt, int f, int ccap, int* __restrict__ ord_kf,
                                                 int* __restrict__ ord_w, int tid, int T)
{
    int P = 1;
    while (P < cnt) P <<= 1;
    for (int j = cnt + tid; j < P; j += T) keys[j] = LLONG_MIN;
    __syncthreads();
    cv_sort_desc(keys, P, tid, T);
    for (int j = tid; j < cnt; j += T) {
        const long long k = keys[j];
        ord_kf[(size_t)f * ccap + j] = cv_key_slot(k);
        ord_w[(size_t)f * ccap + j] = cv_key_w(k);
    }
}

// where t stands in the map row of nb: the entries below it, and its index or -1
__device__ __forceinline__ void cv_locate(const int* __restrict__ conn_kf, int nb, int nc, int ccap, int t, int tid,
                                          int T, int* s_loc, int& lt, int& fidx)
{
    if (tid == 0) {
        s_loc[0] = 0;
        s_loc[1] = -1;
    }
    __syncthreads();
    int below = 0, at = -1;
    for (int j = tid; j < nc; j += T) {
        const int e = conn_kf[(size_t)nb * ccap + j];
        below += e < t;
        if (e == t) at = j;
    }
    if (below) atomicAdd(s_loc, below);
    if (at >= 0) atomicMax(s_loc + 1, at);
    __syncthreads();
    lt = s_loc[0];
    fidx = s_loc[1];
    __syncthreads();   // s_loc is rewritten by the next row
}

__global__ __launch_bounds__(kCvRowThreads) void k_cv_apply(
    int ti, const int* __restrict__ rank, int nkf, int ccap, int root, int* __restrict__ conn_kf,
    int* __restrict__ conn_w, int* __restrict__ nconn, int* __restrict__ ord_kf, int* __restrict__ ord_w,
    int* __restrict__ nord, int* __restrict__ parent, uint8_t* __restrict__ first, const int* __restrict__ hdr,
    const int* __restrict__ m_kf, const int* __restrict__ m_w, const int* __restrict__ p_kf,
    const int* __restrict__ p_w, int* __restrict__ status)
{
    constexpr int T = kCvRowThreads;
    __shared__ long long keys[ORBM_MAX_CONNECTIONS];
    __shared__ int s_loc[2];
    const int tid = (int)threadIdx.x;
    if (!hdr[kCvGo]) return;
    const int t = hdr[kCvT], nv = hdr[kCvNV], np = hdr[kCvNP];
    const int rt = rank ? rank[t] : t;
    for (int q = blockIdx.x; q <= np; q += gridDim.x) {
        if (q == np) {
            // the target's own rows (:354-376): the map is KFcounter, the ordered list vPairs alone
            const size_t row = (size_t)t * ccap;
            for (int j = tid; j < nv; j += T) {
                conn_kf[row + j] = m_kf[j];
                conn_w[row + j] = m_w[j];
            }
            for (int j = tid; j < np; j += T) {
                const int s = p_kf[j];
                keys[j] = cv_key(p_w[j], rank ? rank[s] : s, s);
            }
            __syncthreads();
            cv_write_ordered(keys, np, t, ccap, ord_kf, ord_w, tid, T);
            if (tid == 0) {
                nconn[t] = nv;
                nord[t] = np;
                if (first[t] && t != root) {   // mbFirstConnection && mnId!=0 (:371)
                    parent[t] = cv_key_slot(keys[0]);
                    first[t] = 0;
                }
                status[ti] = 0;
            }
            __syncthreads();
            continue;
        }
        // AddConnection(nb <- t, w) (:123-136); k_cv_vote checked the row and that an insert fits
        const int nb = p_kf[q], w = p_w[q];
        const int nc = nconn[nb];
        const size_t row = (size_t)nb * ccap;
        int lt, fidx;
        cv_locate(conn_kf, nb, nc, ccap, t, tid, T, s_loc, lt, fidx);
        if (fidx >= 0 && conn_w[row + fidx] == w) continue;   // the same weight: return, no re-sort (:131)
        const int newc = fidx >= 0 ? nc : nc + 1;
        for (int j = tid; j < nc; j += T) {
            const int e = conn_kf[row + j];
            const int ww = j == fidx ? w : conn_w[row + j];
            keys[fidx >= 0 || j < lt ? j : j + 1] = cv_key(ww, rank ? rank[e] : e, e);
        }
        if (fidx < 0 && tid == 0) keys[lt] = cv_key(w, rt, t);
        __syncthreads();
        if (fidx >= 0) {
            if (tid == 0) conn_w[row + fidx] = w;
        } else {
            for (int j = lt + tid; j < newc; j += T) {   // the shifted tail, with the new entry at its head
                const long long k = keys[j];
                conn_kf[row + j] = cv_key_slot(k);
                conn_w[row + j] = cv_key_w(k);
            }
        }
        __syncthreads();
        cv_write_ordered(keys, newc, nb, ccap, ord_kf, ord_w, tid, T);
        if (tid == 0) {
            nconn[nb] = newc;
            nord[nb] = newc;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(kCvVoteThreads) void k_cv_erase_check(
    const int* __restrict__ targets, int ti, int nkf, int ccap, const int* __restrict__ conn_kf,
    const int* __restrict__ nconn, int* __restrict__ hdr, int* __restrict__ status)
{
    constexpr int T = kCvVoteThreads, W = T / 64;
    __shared__ int s_bad;
    const int tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (tid == 0) s_bad = 0;
    __syncthreads();
    const int t = targets[ti];
    const bool t_ok = t >= 0 && t < nkf;
    const int nc = t_ok ? nconn[t] : -1;
    const bool ok = nc >= 0 && nc <= ccap && hdr[kCvRankBad] == 0;
    if (ok)
        for (int q = w; q < nc; q += W) {
            const int nb = conn_kf[(size_t)t * ccap + q];
            if (nb < 0 || nb >= nkf) {
                if (lane == 0) s_bad = 1;
                continue;
            }
            const int nn = nconn[nb];
            if (nn < 0 || nn > ccap) {
                if (lane == 0) s_bad = 1;
                continue;
            }
            bool rb = false;
            for (int j = lane; j < nn; j += 64) {
                const int e = conn_kf[(size_t)nb * ccap + j];
                rb |= e < 0 || e >= nkf;
            }
            if (rb) s_bad = 1;
        }
    __syncthreads();
    if (tid == 0) {
        const bool good = ok && !s_bad;
        hdr[kCvT] = t;
        hdr[kCvNV] = good ? nc : 0;
        hdr[kCvGo] = good;
        status[ti] = good ? 0 : (int)ORBM_CONN_INVALID;
    }
}

__global__ __launch_bounds__(kCvRowThreads) void k_cv_erase_apply(
    const int* __restrict__ rank, int ccap, int* __restrict__ conn_kf, int* __restrict__ conn_w,
    int* __restrict__ nconn, int* __restrict__ ord_kf, int* __restrict__ ord_w, int* __restrict__ nord,
    const int* __restrict__ hdr)
{
    constexpr int T = kCvRowThreads;
    __shared__ long long keys[ORBM_MAX_CONNECTIONS];
    __shared__ int s_loc[2];
    const int tid = (int)threadIdx.x;
    if (!hdr[kCvGo]) return;
    const int t = hdr[kCvT], nt = hdr[kCvNV];
    for (int q = blockIdx.x; q <= nt; q += gridDim.x) {
        if (q == nt) {   // mConnectedKeyFrameWeights.clear(), mvpOrderedConnectedKeyFrames.clear() (:476-477)
            if (tid == 0) {
                nconn[t] = 0;
                nord[t] = 0;
            }
            continue;
        }
        // EraseConnection(nb, t) (:553-567); the target's row entries stand, only its counts are cleared above
        const int nb = conn_kf[(size_t)t * ccap + q];
        if (nb == t) continue;
        const int nc = nconn[nb];
        const size_t row = (size_t)nb * ccap;
        int lt, fidx;
        cv_locate(conn_kf, nb, nc, ccap, t, tid, T, s_loc, lt, fidx);
        if (fidx < 0) continue;
        const int newc = nc - 1;
        for (int j = tid; j < nc; j += T) {
            if (j == fidx) continue;
            const int e = conn_kf[row + j];
            keys[j < fidx ? j : j - 1] = cv_key(conn_w[row + j], rank ? rank[e] : e, e);
        }
        __syncthreads();
        for (int j = fidx + tid; j < newc; j += T) {
            const long long k = keys[j];
            conn_kf[row + j] = cv_key_slot(k);
            conn_w[row + j] = cv_key_w(k);
        }
        __syncthreads();
        cv_write_ordered(keys, newc, nb, ccap, ord_kf, ord_w, tid, T);
        if (tid == 0) {
            nconn[nb] = newc;
            nord[nb] = newc;
        }
        __syncthreads();
    }
}

// ---- getters ----

__global__ void k_cv_best(const int* __restrict__ ord_kf, const int* __restrict__ nord, int nkf, int ccap, int N,
                          int* __restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)nkf * (size_t)N) return;
    const int f = (int)(i / (size_t)N), j = (int)(i % (size_t)N);
    const int no = min(max(nord[f], 0), ccap);
    out[i] = j < no ? ord_kf[(size_t)f * ccap + j] : -1;
}

__global__ void k_cv_mask(const int* __restrict__ conn_kf, const int* __restrict__ nconn, int nkf, int ccap, int t,
                          uint8_t* __restrict__ mask)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    const int nc = min(max(nconn[t], 0), ccap);
    if (j >= nc) return;
    const int e = conn_kf[(size_t)t * ccap + j];
    if (e >= 0 && e < nkf) mask[e] = 1;
}

__global__ void k_cv_by_weight(const int* __restrict__ ord_w, const int* __restrict__ nord, int nkf, int ccap, int w,
                               int* __restrict__ out)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nkf) return;
    const int no = min(max(nord[f], 0), ccap);
    // upper_bound(mvOrderedWeights, w, weightComp) (:191): the first weight below w in the descending list
    int lo = 0, hi = no;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (ord_w[(size_t)f * ccap + mid] < w) hi = mid;
        else lo = mid + 1;
    }
    out[f] = lo == no ? 0 : lo;   // it==end(): an empty vector (:192)
}

// ---- GetChilds() as a CSR ----
enum { kChBad = 0, kChGo = 1 };

__global__ void k_ch_count(const int* __restrict__ parent, const uint8_t* __restrict__ bad, int nkf,
                           int* __restrict__ hdr, int* __restrict__ cnt)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= nkf) return;
    const int p = parent[c];
    if (p < -1 || p >= nkf) hdr[kChBad] = 1;
    else if (p >= 0 && !bad[c]) atomicAdd(cnt + p, 1);
}

// the exclusive scan of the counts into child_ptr; the counts become the fill cursors
__global__ __launch_bounds__(kCvVoteThreads) void k_ch_scan(int nkf, int* __restrict__ hdr, int* __restrict__ cnt,
                                                            int* __restrict__ child_ptr, int* __restrict__ status)
{
    constexpr int T = kCvVoteThreads, W = T / 64;
    __shared__ int s_w[W];
    const int tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (hdr[kChBad] || hdr[kCvRankBad]) {
        if (tid == 0) {
            hdr[kChGo] = 0;
            *status = ORBM_CONN_INVALID;
        }
        return;
    }
    int run = 0;
    for (int c0 = 0; c0 < nkf; c0 += T) {
        const int f = c0 + tid;
        const int v = f < nkf ? cnt[f] : 0;
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
        if (f < nkf) {
            const int start = run + before + x - v;
            child_ptr[f] = start;
            cnt[f] = start;
        }
        run += total;
        __syncthreads();   // s_w is rewritten by the next chunk
    }
    if (tid == 0) {
        child_ptr[nkf] = run;
        hdr[kChGo] = 1;
        *status = 0;
    }
}

__global__ void k_ch_fill(const int* __restrict__ parent, const uint8_t* __restrict__ bad, int nkf,
                          const int* __restrict__ hdr, int* __restrict__ cursor, int* __restrict__ tmp)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= nkf || !hdr[kChGo]) return;
    const int p = parent[c];
    if (p >= 0 && !bad[c]) tmp[atomicAdd(cursor + p, 1)] = c;
}

// a child's place among its siblings is the number of them with a lower rank (std::set<KeyFrame*> order)
__global__ void k_ch_order(const int* __restrict__ parent, const uint8_t* __restrict__ bad,
                           const int* __restrict__ rank, int nkf, const int* __restrict__ hdr,
                           const int* __restrict__ child_ptr, const int* __restrict__ tmp, int* __restrict__ child)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= nkf || !hdr[kChGo]) return;
    const int p = parent[c];
    if (p < 0 || bad[c]) return;
    const int a = child_ptr[p], b = child_ptr[p + 1];
    const int rc = rank ? rank[c] : c;
    int k = 0;
    for (int j = a; j < b; ++j) {
        const int s = tmp[j];
        k += (rank ? rank[s] : s) < rc;
    }
    child[a + k] = c;
}

namespace {

bool cv_graph_ok(const orbm_covis_graph* g)
{
    return g && g->conn_kf && g->conn_w && g->nconn && g->ord_kf && g->ord_w && g->nord && g->parent && g->first;
}

bool cv_dims_ok(int nkf, int ccap)
{
    return nkf >= 0 && nkf <= ORBV_DB_MAX_KEYFRAMES && ccap >= 1 && ccap <= ORBM_MAX_CONNECTIONS;
}

// the rank table's permutation check, once per call
void cv_rankcheck(const int* d_kf_rank, int nkf, int* wk, const CvLayout& L, hipStream_t s)
{
    if (d_kf_rank && nkf > 0)
        hipLaunchKernelGGL(k_cv_rankcheck, dim3((unsigned)((nkf + 255) / 256)), dim3(256), 0, s, d_kf_rank, nkf,
                           wk + L.dup, wk);
}

}  // namespace

}  // namespace orbx

using namespace orbx;

extern "C" {

size_t orbm_connections_work_bytes(int nkf, int ccap)
{
    if (!cv_dims_ok(nkf, ccap)) return 0;
    return cv_layout(nkf, ccap).bytes;
}

orbx_status orbm_update_connections_device(const orbm_covis_graph* graph, int nkf, int ccap, const int* d_counts,
                                           const int* d_kf_mp, int cap, const int* d_kf_rank,
                                           const orbm_map_point* d_pts, const int* d_obs_ptr,
                                           const orbm_observation* d_obs, int nmp, const int* d_targets, int ntargets,
                                           int th, int root, int* d_status, void* d_work, size_t work_bytes,
                                           void* stream)
{
    if (!cv_graph_ok(graph) || !cv_dims_ok(nkf, ccap) || cap <= 0 || cap > ORBM_MAX_FEATURES || nmp < 0 ||
        ntargets < 0 || th < 1 || root < -1 || root >= nkf || !d_counts || !d_kf_mp || !d_pts || !d_obs_ptr ||
        !d_obs || !d_targets || !d_status || !d_work || ((uintptr_t)d_work & 3) ||
        work_bytes < orbm_connections_work_bytes(nkf, ccap))
        return ORBX_EINVAL;
    if (ntargets == 0) return ORBX_OK;
    hipStream_t s = (hipStream_t)stream;
    const CvLayout L = cv_layout(nkf, ccap);
    const orbm_covis_graph g = *graph;
    int* const wk = (int*)d_work;
    cv_rankcheck(d_kf_rank, nkf, wk, L, s);
    const unsigned grid = (unsigned)std::max(1, std::min(std::min(nkf, ccap + 1), kCvMaxGrid));
    for (int i = 0; i < ntargets; ++i) {
        if (nkf <= ORBM_LOCAL_MAP_LDS_KEYFRAMES)
            hipLaunchKernelGGL(k_cv_vote<true>, dim3(1), dim3(kCvVoteThreads), 0, s, d_targets, i, d_counts, d_kf_mp,
                               cap, d_kf_rank, d_pts, d_obs_ptr, d_obs, nmp, nkf, ccap, th, g.conn_kf, g.nconn, wk,
                               wk + L.votes, wk + L.m_kf, wk + L.m_w, wk + L.p_kf, wk + L.p_w, d_status);
        else
            hipLaunchKernelGGL(k_cv_vote<false>, dim3(1), dim3(kCvVoteThreads), 0, s, d_targets, i, d_counts, d_kf_mp,
                               cap, d_kf_rank, d_pts, d_obs_ptr, d_obs, nmp, nkf, ccap, th, g.conn_kf, g.nconn, wk,
                               wk + L.votes, wk + L.m_kf, wk + L.m_w, wk + L.p_kf, wk + L.p_w, d_status);
        hipLaunchKernelGGL(k_cv_apply, dim3(grid), dim3(kCvRowThreads), 0, s, i, d_kf_rank, nkf, ccap, root,
                           g.conn_kf, g.conn_w, g.nconn, g.ord_kf, g.ord_w, g.nord, g.parent, g.first, wk,
                           wk + L.m_kf, wk + L.m_w, wk + L.p_kf, wk + L.p_w, d_status);
    }
    if (hipGetLastError() != hipSuccess) return ORBX_EDEVICE;
    // the header, the rank counters and the staged rows: zero again like the vote counters
    if (hipMemsetAsync(wk, 0, L.small_bytes, s) != hipSuccess) return ORBX_EDEVICE;
    return ORBX_OK;
}

orbx_status orbm_erase_connections_device(const orbm_covis_graph* graph, int nkf, int ccap, const int* d_kf_rank,
                                          const int* d_targets, int ntargets, int* d_status, void* d_work,
                                          size_t work_bytes, void* stream)
{
    if (!cv_graph_ok(graph) || !cv_dims_ok(nkf, ccap) || ntargets < 0 || !d_targets || !d_status || !d_work ||
        ((uintptr_t)d_work & 3) || work_bytes < orbm_connections_work_bytes(nkf, ccap))
        return ORBX_EINVAL;
    if (ntargets == 0) return ORBX_OK;
    hipStream_t s = (hipStream_t)stream;
    const CvLayout L = cv_layout(nkf, ccap);
    const orbm_covis_graph g = *graph;
    int* const wk = (int*)d_work;
    cv_rankcheck(d_kf_rank, nkf, wk, L, s);
    const unsigned grid = (unsigned)std::max(1, std::min(std::min(nkf, ccap + 1), kCvMaxGrid));
    for (int i = 0; i < ntargets; ++i) {
        hipLaunchKernelGGL(k_cv_erase_check, dim3(1), dim3(kCvVoteThreads), 0, s, d_targets, i, nkf, ccap, g.conn_kf,
                           g.nconn, wk, d_status);
        hipLaunchKernelGGL(k_cv_erase_apply, dim3(grid), dim3(kCvRowThreads), 0, s, d_kf_rank, ccap, g.conn_kf,
                           g.conn_w, g.nconn, g.ord_kf, g.ord_w, g.nord, wk);
    }
    if (hipGetLastError() != hipSuccess) return ORBX_EDEVICE;
    if (hipMemsetAsync(wk, 0, L.small_bytes, s) != hipSuccess) return ORBX_EDEVICE;
    return ORBX_OK;
}

orbx_status orbm_best_covisibles_device(const orbm_covis_graph* graph, int nkf, int ccap, int N, int* d_out,
                                        void* stream)
{
    if (!cv_graph_ok(graph) || !cv_dims_ok(nkf, ccap) || N < 1 || N > ORBM_MAX_CONNECTIONS || !d_out)
        return ORBX_EINVAL;
    if (nkf == 0) return ORBX_OK;
    const size_t total = (size_t)nkf * (size_t)N;
    hipLaunchKernelGGL(k_cv_best, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       graph->ord_kf, graph->nord, nkf, ccap, N, d_out);
    return hipGetLastError() == hipSuccess ? ORBX_OK : ORBX_EDEVICE;
}

orbx_status orbm_connected_mask_device(const orbm_covis_graph* graph, int nkf, int ccap, int t, uint8_t* d_mask,
                                       void* stream)
{
    if (!cv_graph_ok(graph) || !cv_dims_ok(nkf, ccap) || t < 0 || t >= nkf || !d_mask) return ORBX_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(d_mask, 0, (size_t)nkf, s) != hipSuccess) return ORBX_EDEVICE;
    hipLaunchKernelGGL(k_cv_mask, dim3((unsigned)((ccap + 255) / 256)), dim3(256), 0, s, graph->conn_kf, graph->nconn,
                       nkf, ccap, t, d_mask);
    return hipGetLastError() == hipSuccess ? ORBX_OK : ORBX_EDEVICE;
}

orbx_status orbm_covisibles_by_weight_device(const orbm_covis_graph* graph, int nkf, int ccap, int w, int* d_n,
                                             void* stream)
{
    if (!cv_graph_ok(graph) || !cv_dims_ok(nkf, ccap) || !d_n) return ORBX_EINVAL;
    if (nkf == 0) return ORBX_OK;
    hipLaunchKernelGGL(k_cv_by_weight, dim3((unsigned)((nkf + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       graph->ord_w, graph->nord, nkf, ccap, w, d_n);
    return hipGetLastError() == hipSuccess ? ORBX_OK : ORBX_EDEVICE;
}

size_t orbm_children_work_bytes(int nkf)
{
    if (nkf < 0 || nkf > ORBV_DB_MAX_KEYFRAMES) return 0;
    return ((size_t)kCvHdr + 3 * (size_t)nkf) * sizeof(int);
}

orbx_status orbm_children_device(const int* d_parent, const uint8_t* d_kf_bad, const int* d_kf_rank, int nkf,
                                 int* d_child_ptr, int* d_child, int* d_status, void* d_work, size_t work_bytes,
                                 void* stream)
{
    if (nkf < 0 || nkf > ORBV_DB_MAX_KEYFRAMES || !d_parent || !d_kf_bad || !d_child_ptr || !d_child || !d_status ||
        !d_work || ((uintptr_t)d_work & 3) || work_bytes < orbm_children_work_bytes(nkf))
        return ORBX_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    int* const wk = (int*)d_work;
    int* const dup = wk + kCvHdr;
    int* const cnt = dup + nkf;
    int* const tmp = cnt + nkf;
    const dim3 g((unsigned)std::max(1, (nkf + 255) / 256)), b(256);
    if (d_kf_rank && nkf > 0) hipLaunchKernelGGL(k_cv_rankcheck, g, b, 0, s, d_kf_rank, nkf, dup, wk);
    hipLaunchKernelGGL(k_ch_count, g, b, 0, s, d_parent, d_kf_bad, nkf, wk, cnt);
    hipLaunchKernelGGL(k_ch_scan, dim3(1), dim3(kCvVoteThreads), 0, s, nkf, wk, cnt, d_child_ptr, d_status);
    hipLaunchKernelGGL(k_ch_fill, g, b, 0, s, d_parent, d_kf_bad, nkf, wk, cnt, tmp);
    hipLaunchKernelGGL(k_ch_order, g, b, 0, s, d_parent, d_kf_bad, d_kf_rank, nkf, wk, d_child_ptr, tmp, d_child);
    if (hipGetLastError() != hipSuccess) return ORBX_EDEVICE;
    if (hipMemsetAsync(wk, 0, orbm_children_work_bytes(nkf), s) != hipSuccess) return ORBX_EDEVICE;
    return ORBX_OK;
}

orbx_status orbm_update_connections(int device, const orbm_covis_graph* graph, int nkf, int ccap, const int* counts,
                                    const int* kf_mp, int cap, const int* kf_rank, const orbm_map_point* pts,
                                    const int* obs_ptr, const orbm_observation* obs, int nmp, const int* targets,
                                    int ntargets, int th, int root, int* status)
{
    if (!cv_graph_ok(graph) || !cv_dims_ok(nkf, ccap) || nkf < 1 || cap <= 0 || cap > ORBM_MAX_FEATURES || nmp < 0 ||
        ntargets < 0 || th < 1 || root < -1 || root >= nkf || !counts || !kf_mp || !obs_ptr ||
        (nmp > 0 && !pts) || (ntargets > 0 && (!targets || !status)))
        return ORBX_EINVAL;
    if (obs_ptr[0] < 0) return ORBX_EINVAL;
    for (int m = 0; m < nmp; ++m)
        if (obs_ptr[m + 1] < obs_ptr[m]) return ORBX_EINVAL;
    if (obs_ptr[nmp] > 0 && !obs) return ORBX_EINVAL;
    if (ntargets == 0) return ORBX_OK;
    const size_t wbytes = orbm_connections_work_bytes(nkf, ccap);
    const size_t K = (size_t)nkf, M = (size_t)nmp, R = K * (size_t)ccap;
    HostCall c(device);
    const auto ocn = c.in(counts, K);
    const auto okm = c.in(kf_mp, K * (size_t)cap);
    const auto okr = c.in(kf_rank, kf_rank ? K : 0);
    const auto opt = c.in(pts, M);
    const auto oop = c.in(obs_ptr, M + 1);
    const auto oob = c.in(obs, (size_t)obs_ptr[nmp]);
    const auto otg = c.in(targets, (size_t)ntargets);
    // the graph and the status go up as well: what the call does not write keeps its bits
    const auto ock = c.inout(graph->conn_kf, R);
    const auto ocw = c.inout(graph->conn_w, R);
    const auto onc = c.inout(graph->nconn, K);
    const auto ook = c.inout(graph->ord_kf, R);
    const auto oow = c.inout(graph->ord_w, R);
    const auto ono = c.inout(graph->nord, K);
    const auto opa = c.inout(graph->parent, K);
    const auto ofi = c.inout(graph->first, K);
    const auto ost = c.inout(status, (size_t)ntargets);
    const auto owk = c.out<uint8_t>(wbytes);
    orbx_status rc = c.begin();
    if (rc != ORBX_OK) return rc;
    if (hipMemsetAsync(c.dev(owk), 0, wbytes, c.stream()) != hipSuccess) return ORBX_EDEVICE;
    const orbm_covis_graph g = {c.dev(ock), c.dev(ocw), c.dev(onc), c.dev(ook),
                                c.dev(oow), c.dev(ono), c.dev(opa), c.dev(ofi)};
    rc = orbm_update_connections_device(&g, nkf, ccap, c.dev(ocn), c.dev(okm), cap, kf_rank ? c.dev(okr) : nullptr,
                                        c.dev(opt), c.dev(oop), c.dev(oob), nmp, c.dev(otg), ntargets, th, root,
                                        c.dev(ost), c.dev(owk), wbytes, c.stream());
    if (rc != ORBX_OK) return rc;
    return c.finish();
}

}  // extern "C"

// KeyFrameDatabase on the device:
//   KeyFrameDatabase::add / erase / clear / DetectLoopCandidates / DetectRelocalizationCandidates
//                                                     src/KeyFrameDatabase.cc:40-309
//   TemplatedVocabulary::score -> L1Scoring::score    Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68
//
// Storage is a forward index: ptr[slot], n[slot], live[slot] and every keyframe's BowVector appended to
// word[] / weight[].  No inverted file: every inverted-file list is in add order, so lKFsSharingWords
// (first encounter while walking the query's words upwards) is the sort by (smallest shared word, slot).
//
// One query:
//   D1 k_kfdb_share       one wave per slot: each lane binary-searches a strided share of the keyframe's
//                         words in the query (staged in LDS while it fits) -> common words, smallest one
//   D2 k_kfdb_threshold   maxCommonWords over the slots, minCommonWords = maxCommonWords * 0.8f
//   D3 k_kfdb_score       one wave per slot with words > minCommonWords: L1 terms in parallel, summed in
//                         ascending word order by one dependent chain of double adds
//   D4 k_kfdb_candidates  one workgroup: sort the scored slots by (smallest shared word, slot), accumulate
//                         the covisible neighbours' scores, threshold at 0.75 * best, deduplicate, compact
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <mutex>
#include <new>
#include <vector>

#include "../../include/orbx.h"
#include "orbx_device.hpp"
#include "orbx_host.hpp"

namespace orbx {

int voc_device(const orbx_vocabulary* v);   // orbx_voc.hip

constexpr int kKfdbLdsQuery = 8192;   // query words the share pass stages in LDS (32 KiB); larger queries stay in global memory
constexpr int kKfdbLdsSort = 2048;    // slots whose candidate pass sorts in LDS (16 bytes each); more sort in global scratch
constexpr int kKfdbShareNT = 512;     // 8 waves = 8 slots per workgroup
constexpr int kKfdbScoreNT = 256;
constexpr int kKfdbCandNT = 512;
constexpr int kKfdbCovis = 10;        // GetBestCovisibilityKeyFrames(10)

__device__ __forceinline__ int kfdb_qn(const int* __restrict__ qn_p, int qcap) { return max(0, min(*qn_p, qcap)); }

// index of w in q[0, qn) (ascending), or -1
template <class Q>
__device__ __forceinline__ int kfdb_find(Q q, int qn, int w)
{
    int lo = 0, hi = qn;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (q[mid] < w) lo = mid + 1;
        else hi = mid;
    }
    return (lo < qn && q[lo] == w) ? lo : -1;
}

// KeyFrameDatabase::add for nframes BowVectors at f * cap: slot0 + f gets the words appended behind `base`
__global__ __launch_bounds__(256) void k_kfdb_append(const int* __restrict__ src_word,
                                                     const double* __restrict__ src_weight,
                                                     const int* __restrict__ counts, int nframes, int cap, int slot0,
                                                     long long base, long long* __restrict__ ptr, int* __restrict__ n,
                                                     int* __restrict__ live, float* __restrict__ lscore,
                                                     float* __restrict__ rscore, int* __restrict__ word,
                                                     double* __restrict__ weight)
{
    __shared__ long long s_part[256];
    const int f = blockIdx.x, tid = threadIdx.x;
    long long before = 0;
    for (int g = tid; g < f; g += 256) before += max(0, min(counts[g], cap));
    s_part[tid] = before;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) s_part[tid] += s_part[tid + o];
        __syncthreads();
    }
    const long long off = base + s_part[0];
    const int m = max(0, min(counts[f], cap));
    if (tid == 0) {
        ptr[slot0 + f] = off;
        n[slot0 + f] = m;
        live[slot0 + f] = 1;
        lscore[slot0 + f] = 0.0f;   // mLoopScore / mRelocScore before any query: defined as 0
        rscore[slot0 + f] = 0.0f;
    }
    const size_t s = (size_t)f * cap;
    for (int i = tid; i < m; i += 256) {
        word[off + i] = src_word[s + i];
        weight[off + i] = src_weight[s + i];
    }
}

// D1: words[slot] = query words the keyframe holds (0 for an erased or connected slot), minw[slot] = the
// smallest of them; also resets the candidate pass's dedupe table
template <bool kLds>
__global__ __launch_bounds__(kKfdbShareNT) void k_kfdb_share(const long long* __restrict__ ptr,
                                                             const int* __restrict__ n, const int* __restrict__ live,
                                                             const int* __restrict__ word, int nslots,
                                                             const int* __restrict__ qword,
                                                             const int* __restrict__ qn_p, int qcap,
                                                             const uint8_t* __restrict__ connected,
                                                             int* __restrict__ words, int* __restrict__ minw,
                                                             int* __restrict__ first)
{
    extern __shared__ int s_q[];
    const int tid = threadIdx.x;
    const int qn = kfdb_qn(qn_p, qcap);
    if (kLds) {
        for (int i = tid; i < qn; i += kKfdbShareNT) s_q[i] = qword[i];
        __syncthreads();
    }
    const int lane = tid & 63, slot = blockIdx.x * (kKfdbShareNT / 64) + (tid >> 6);
    if (slot >= nslots) return;
    int c = 0, mw = INT_MAX;
    if (live[slot] && !(connected && connected[slot])) {
        const long long p = ptr[slot];
        const int m = n[slot];
        for (int i0 = 0; i0 < m; i0 += 64) {
            const int i = i0 + lane;
            bool hit = false;
            int w = 0;
            if (i < m) {
                w = word[p + i];
                if (kLds) hit = kfdb_find(s_q, qn, w) >= 0;
                else hit = kfdb_find(qword, qn, w) >= 0;
            }
            const unsigned long long b = __ballot(hit);
            c += __popcll(b);
            // words ascend: the first hit of the first chunk that has one is the smallest shared word
            const int w0 = __shfl(w, b ? __ffsll((long long)b) - 1 : 0);
            if (b && mw == INT_MAX) mw = w0;
        }
    }
    if (lane == 0) {
        words[slot] = c;
        minw[slot] = mw;
        first[slot] = INT_MAX;
    }
}

// D2: meta[0] = maxCommonWords, meta[1] = minCommonWords = maxCommonWords * 0.8f (int -> float, a float
// multiply, truncation: src/KeyFrameDatabase.cc:120, :235)
__global__ __launch_bounds__(1024) void k_kfdb_threshold(const int* __restrict__ words, int nslots,
                                                         int* __restrict__ meta)
{
    __shared__ int s_max[1024];
    const int tid = threadIdx.x;
    int m = 0;
    for (int i = tid; i < nslots; i += 1024) m = max(m, words[i]);
    s_max[tid] = m;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if (tid < o) s_max[tid] = max(s_max[tid], s_max[tid + o]);
        __syncthreads();
    }
    if (tid == 0) {
        meta[0] = s_max[0];
        meta[1] = (int)((float)s_max[0] * 0.8f);
    }
}

// D3: L1Scoring::score(query, keyframe).  list == NULL: every slot with words > minCommonWords, its float
// score kept in fscore[slot]; else the nlist listed slots, as doubles in dscore (an erased slot gives 0).
__global__ __launch_bounds__(kKfdbScoreNT) void k_kfdb_score(const long long* __restrict__ ptr,
                                                             const int* __restrict__ n, const int* __restrict__ live,
                                                             const int* __restrict__ word,
                                                             const double* __restrict__ weight, int nslots,
                                                             const int* __restrict__ qword,
                                                             const double* __restrict__ qweight,
                                                             const int* __restrict__ qn_p, int qcap,
                                                             const int* __restrict__ words,
                                                             const int* __restrict__ meta,
                                                             const int* __restrict__ list, int nlist,
                                                             float* __restrict__ fscore, double* __restrict__ dscore)
{
    const int tid = threadIdx.x, lane = tid & 63;
    const int idx = blockIdx.x * (kKfdbScoreNT / 64) + (tid >> 6);
    int slot;
    if (list) {
        if (idx >= nlist) return;
        slot = list[idx];
        if (slot < 0 || slot >= nslots || !live[slot]) {
            if (lane == 0) dscore[idx] = 0.0;
            return;
        }
    } else {
        slot = idx;
        if (slot >= nslots || !(words[slot] > meta[1])) return;
    }
    const int qn = kfdb_qn(qn_p, qcap);
    const long long p = ptr[slot];
    const int m = n[slot];
    double score = 0;
    for (int i0 = 0; i0 < m; i0 += 64) {
        const int i = i0 + lane;
        double term = 0.0;
        bool hit = false;
        if (i < m) {
            const int j = kfdb_find(qword, qn, word[p + i]);
            if (j >= 0) {
                const double vi = qweight[j], wi = weight[p + i];
                term = fabs(vi - wi) - fabs(vi) - fabs(wi);
                hit = true;
            }
        }
        // the terms in ascending word order, one dependent add after another (every lane keeps the same sum)
        unsigned long long b = __ballot(hit);
        while (b) {
            const int l = __ffsll((long long)b) - 1;
            score += __shfl(term, l);
            b &= b - 1;
        }
    }
    score = -score / 2.0;
    if (lane == 0) {
        if (dscore) dscore[idx] = score;
        if (fscore) fscore[slot] = (float)score;
    }
}

__device__ __forceinline__ void kfdb_bitonic(unsigned long long* k, int p2)
{
    for (int size = 2; size <= p2; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = threadIdx.x; i < (p2 >> 1); i += kKfdbCandNT) {
                const int lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
                const bool up = (lo & size) == 0;
                const unsigned long long a = k[lo], b = k[hi];
                if ((a > b) == up) {
                    k[lo] = b;
                    k[hi] = a;
                }
            }
            __syncthreads();
        }
    }
}

// D4: lScoreAndMatch -> lAccScoreAndMatch -> the candidate list (src/KeyFrameDatabase.cc:141-196, :255-308).
// kG: more than kKfdbLdsSort slots keep keys, sums and best keyframes in global scratch (the same network).
template <bool kG>
__global__ __launch_bounds__(kKfdbCandNT) void k_kfdb_candidates(int nslots, const int* __restrict__ words,
                                                                 const int* __restrict__ minw,
                                                                 const int* __restrict__ meta,
                                                                 const float* __restrict__ fscore,
                                                                 const int* __restrict__ covis, int loop,
                                                                 float min_score, unsigned long long* __restrict__ gkey,
                                                                 float* __restrict__ gacc, int* __restrict__ gbest,
                                                                 int p2max, int* __restrict__ first,
                                                                 int* __restrict__ cand, int* __restrict__ ncand)
{
    extern __shared__ __attribute__((aligned(16))) unsigned long long s_dyn[];
    __shared__ int s_tmp[kKfdbCandNT];
    __shared__ float s_red[kKfdbCandNT];
    __shared__ int s_m, s_run;
    const int tid = threadIdx.x;
    unsigned long long* key = kG ? gkey : s_dyn;
    float* acc = kG ? gacc : reinterpret_cast<float*>(s_dyn + p2max);
    int* best = kG ? gbest : reinterpret_cast<int*>(s_dyn + p2max) + p2max;
    const int minc = meta[1];
    if (tid == 0) s_m = 0;
    __syncthreads();
    for (int s = tid; s < nslots; s += kKfdbCandNT) {
        bool in = words[s] > minc;
        if (in && loop) in = fscore[s] >= min_score;   // si >= minScore (:136)
        if (in) key[atomicAdd(&s_m, 1)] = ((unsigned long long)(uint32_t)minw[s] << 16) | (uint32_t)s;
    }
    __syncthreads();
    const int m = s_m;
    int p2 = 1;
    while (p2 < m) p2 <<= 1;
    for (int i = m + tid; i < p2; i += kKfdbCandNT) key[i] = ~0ull;
    __syncthreads();
    kfdb_bitonic(key, p2);

    // accumulate by covisibility, in neighbour order, in float
    float top = loop ? min_score : 0.0f;   // bestAccScore
    for (int i = tid; i < m; i += kKfdbCandNT) {
        const int s = (int)(key[i] & 0xFFFF);
        const float si = fscore[s];
        float a = si, bs = si;
        int bk = s;
        if (covis)
            for (int j = 0; j < kKfdbCovis; ++j) {
                const int nb = covis[(size_t)s * kKfdbCovis + j];
                if (nb < 0 || nb >= nslots) continue;
                // loop: mnLoopQuery == id && mnLoopWords > minCommonWords (:159); reloc: mnRelocQuery == id (:273)
                if (!(loop ? words[nb] > minc : words[nb] > 0)) continue;
                const float s2 = fscore[nb];
                a += s2;
                if (s2 > bs) {
                    bk = nb;
                    bs = s2;
                }
            }
        acc[i] = a;
        best[i] = bk;
        if (a > top) top = a;
    }
    s_red[tid] = top;
    __syncthreads();
    for (int o = kKfdbCandNT / 2; o > 0; o >>= 1) {
        if (tid < o && s_red[tid + o] > s_red[tid]) s_red[tid] = s_red[tid + o];
        __syncthreads();
    }
    const float keep = 0.75f * s_red[0];   // minScoreToRetain
    // spAlreadyAddedKF: the first retained entry of each pBestKF
    for (int i = tid; i < m; i += kKfdbCandNT)
        if (acc[i] > keep) atomicMin(&first[best[i]], i);
    if (tid == 0) s_run = 0;
    __syncthreads();
    for (int c0 = 0; c0 < m; c0 += kKfdbCandNT) {
        const int i = c0 + tid;
        bool out = false;
        int bk = 0;
        if (i < m && acc[i] > keep) {
            bk = best[i];
            out = __hip_atomic_load(&first[bk], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == i;
        }
        // block-wide exclusive scan of the flags
        s_tmp[tid] = out ? 1 : 0;
        __syncthreads();
        for (int o = 1; o < kKfdbCandNT; o <<= 1) {
            const int t = tid >= o ? s_tmp[tid - o] : 0;
            __syncthreads();
            s_tmp[tid] += t;
            __syncthreads();
        }
        const int pos = s_run + s_tmp[tid] - (out ? 1 : 0);
        if (out) cand[pos] = bk;
        __syncthreads();
        if (tid == kKfdbCandNT - 1) s_run += s_tmp[tid];
        __syncthreads();
    }
    if (tid == 0) *ncand = s_run;
}

}  // namespace orbx

struct orbv_database {
    int device = 0;
    int nwords = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev = nullptr;      // end of the last asynchronous query
    bool ev_set = false;
    std::mutex mu;
    int nslots = 0, cap_slots = 0;
    long long used = 0, cap_words = 0;
    std::vector<uint8_t> h_live;   // host mirror (info, orbv_db_scores' slot check)
    // forward index
    long long* d_ptr = nullptr;
    int* d_n = nullptr;
    int* d_live = nullptr;
    float* d_lscore = nullptr;    // mLoopScore per slot
    float* d_rscore = nullptr;    // mRelocScore per slot
    int* d_word = nullptr;
    double* d_weight = nullptr;
    // per-query scratch, cap_slots entries each
    int* d_words = nullptr;
    int* d_minw = nullptr;
    int* d_first = nullptr;
    unsigned long long* d_key = nullptr;   // p2(cap_slots)
    float* d_acc = nullptr;
    int* d_best = nullptr;
    int* d_meta = nullptr;        // [2]
    int p2cap = 0;
};

namespace {

using orbx::DeviceGuard;
using orbx::HostCall;

template <class T>
bool dalloc(T*& p, size_t n, hipStream_t s)
{
    return hipMallocAsync((void**)&p, sizeof(T) * (n ? n : 1), s) == hipSuccess;
}

template <class T>
void dfree(T*& p, hipStream_t s)
{
    if (p) hipFreeAsync(p, s);
    p = nullptr;
}

// work on stream s follows the last asynchronous query
void follow(orbv_database* db, hipStream_t s)
{
    if (db->ev_set) hipStreamWaitEvent(s, db->ev, 0);
}

void mark(orbv_database* db, hipStream_t s)
{
    db->ev_set = hipEventRecord(db->ev, s) == hipSuccess;
}

template <class T>
bool regrow(T*& p, size_t keep, size_t n, hipStream_t s)
{
    T* q = nullptr;
    if (!dalloc(q, n, s)) return false;
    if (p && keep && hipMemcpyAsync(q, p, sizeof(T) * keep, hipMemcpyDeviceToDevice, s) != hipSuccess) {
        hipFreeAsync(q, s);
        return false;
    }
    dfree(p, s);
    p = q;
    return true;
}

// room for need_slots slots and need_words words: doubling, device-to-device copies in stream order on the
// database's stream, complete on return
orbx_status ensure(orbv_database* db, long long need_slots, long long need_words)
{
    if (need_slots > ORBV_DB_MAX_KEYFRAMES) return ORBX_ENOSPC;
    hipStream_t s = db->stream;
    bool ok = true, any = false;
    if (need_slots > db->cap_slots) {
        long long c = db->cap_slots > 0 ? db->cap_slots : 1;
        while (c < need_slots) c *= 2;
        if (c > ORBV_DB_MAX_KEYFRAMES) c = ORBV_DB_MAX_KEYFRAMES;
        int p2 = 1;
        while (p2 < c) p2 <<= 1;
        follow(db, s);
        const size_t k = (size_t)db->nslots;
        ok = regrow(db->d_ptr, k, c, s) && regrow(db->d_n, k, c, s) && regrow(db->d_live, k, c, s) &&
             regrow(db->d_lscore, k, c, s) && regrow(db->d_rscore, k, c, s) && regrow(db->d_words, 0, c, s) &&
             regrow(db->d_minw, 0, c, s) && regrow(db->d_first, 0, c, s) && regrow(db->d_key, 0, p2, s) &&
             regrow(db->d_acc, 0, p2, s) && regrow(db->d_best, 0, p2, s);
        if (ok) {
            db->cap_slots = (int)c;
            db->p2cap = p2;
        }
        any = true;
    }
    if (ok && need_words > db->cap_words) {
        long long c = db->cap_words > 0 ? db->cap_words : 1;
        while (c < need_words) c *= 2;
        follow(db, s);
        ok = regrow(db->d_word, (size_t)db->used, (size_t)c, s) && regrow(db->d_weight, (size_t)db->used, (size_t)c, s);
        if (ok) db->cap_words = c;
        any = true;
    }
    if (any && hipStreamSynchronize(s) != hipSuccess) return ORBX_EDEVICE;
    if (any) db->ev_set = false;
    return ok ? ORBX_OK : ORBX_ENOMEM;
}

bool ascending_in(const int32_t* w, int n, int nwords)
{
    for (int i = 0; i < n; ++i)
        if (w[i] < 0 || w[i] >= nwords || (i > 0 && w[i] <= w[i - 1])) return false;
    return true;
}

// appends nframes BowVectors (device arrays, f * cap layout) whose clamped counts sum to `total`
orbx_status append(orbv_database* db, const int32_t* d_word, const double* d_weight, const int* d_counts, int nframes,
                   int cap, long long total, hipStream_t s)
{
    orbx_status st = ensure(db, (long long)db->nslots + nframes, db->used + total);
    if (st != ORBX_OK) return st;
    follow(db, s);
    hipLaunchKernelGGL(orbx::k_kfdb_append, dim3(nframes), dim3(256), 0, s, d_word, d_weight, d_counts, nframes, cap,
                       db->nslots, db->used, db->d_ptr, db->d_n, db->d_live, db->d_lscore, db->d_rscore, db->d_word,
                       db->d_weight);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(s) != hipSuccess) return ORBX_EDEVICE;
    db->ev_set = false;
    db->nslots += nframes;
    db->used += total;
    db->h_live.resize((size_t)db->nslots, 1);
    return ORBX_OK;
}

// the four query stages on stream s; every pointer a device pointer
orbx_status query(orbv_database* db, bool loop, const int32_t* d_qw, const double* d_qwt, const int* d_qn, int qcap,
                  const uint8_t* d_conn, const int32_t* d_covis, float min_score, int* d_cand, int* d_ncand,
                  int* d_words, float* d_scores, hipStream_t s)
{
    const int ns = db->nslots;
    follow(db, s);
    if (ns == 0) {
        if (hipMemsetAsync(d_ncand, 0, sizeof(int), s) != hipSuccess) return ORBX_EDEVICE;
        mark(db, s);
        return ORBX_OK;
    }
    float* fscore = loop ? db->d_lscore : db->d_rscore;
    const int nshare = (ns + orbx::kKfdbShareNT / 64 - 1) / (orbx::kKfdbShareNT / 64);
    if (qcap <= orbx::kKfdbLdsQuery)
        hipLaunchKernelGGL(orbx::k_kfdb_share<true>, dim3(nshare), dim3(orbx::kKfdbShareNT),
                           (size_t)qcap * sizeof(int), s, db->d_ptr, db->d_n, db->d_live, db->d_word, ns, d_qw, d_qn,
                           qcap, loop ? d_conn : nullptr, db->d_words, db->d_minw, db->d_first);
    else
        hipLaunchKernelGGL(orbx::k_kfdb_share<false>, dim3(nshare), dim3(orbx::kKfdbShareNT), 0, s, db->d_ptr,
                           db->d_n, db->d_live, db->d_word, ns, d_qw, d_qn, qcap, loop ? d_conn : nullptr,
                           db->d_words, db->d_minw, db->d_first);
    hipLaunchKernelGGL(orbx::k_kfdb_threshold, dim3(1), dim3(1024), 0, s, db->d_words, ns, db->d_meta);
    const int nscore = (ns + orbx::kKfdbScoreNT / 64 - 1) / (orbx::kKfdbScoreNT / 64);
    hipLaunchKernelGGL(orbx::k_kfdb_score, dim3(nscore), dim3(orbx::kKfdbScoreNT), 0, s, db->d_ptr, db->d_n,
                       db->d_live, db->d_word, db->d_weight, ns, d_qw, d_qwt, d_qn, qcap, db->d_words, db->d_meta,
                       (const int*)nullptr, 0, fscore, (double*)nullptr);
    if (ns <= orbx::kKfdbLdsSort) {
        int p2 = 1;
        while (p2 < ns) p2 <<= 1;
        hipLaunchKernelGGL(orbx::k_kfdb_candidates<false>, dim3(1), dim3(orbx::kKfdbCandNT), (size_t)p2 * 16, s, ns,
                           db->d_words, db->d_minw, db->d_meta, fscore, d_covis, loop ? 1 : 0, min_score, db->d_key,
                           db->d_acc, db->d_best, p2, db->d_first, d_cand, d_ncand);
    } else {
        hipLaunchKernelGGL(orbx::k_kfdb_candidates<true>, dim3(1), dim3(orbx::kKfdbCandNT), 0, s, ns, db->d_words,
                           db->d_minw, db->d_meta, fscore, d_covis, loop ? 1 : 0, min_score, db->d_key, db->d_acc,
                           db->d_best, db->p2cap, db->d_first, d_cand, d_ncand);
    }
    bool ok = hipGetLastError() == hipSuccess;
    if (ok && d_words)
        ok = hipMemcpyAsync(d_words, db->d_words, sizeof(int) * ns, hipMemcpyDeviceToDevice, s) == hipSuccess;
    if (ok && d_scores)
        ok = hipMemcpyAsync(d_scores, fscore, sizeof(float) * ns, hipMemcpyDeviceToDevice, s) == hipSuccess;
    mark(db, s);
    return ok ? ORBX_OK : ORBX_EDEVICE;
}

orbx_status detect_host(orbv_database* db, bool loop, const int32_t* q_word, const double* q_weight, int qn,
                        const uint8_t* connected, const int32_t* covis, float min_score, int* cand, int cap,
                        int* ncand, int* words, float* scores)
{
    if (!db || qn < 0 || qn > ORBV_MAX_FEATURES || (qn > 0 && (!q_word || !q_weight)) || !ncand || cap < 0 ||
        (cap > 0 && !cand))
        return ORBX_EINVAL;
    *ncand = 0;
    if (!ascending_in(q_word, qn, db->nwords)) return ORBX_EINVAL;
    std::lock_guard<std::mutex> lk(db->mu);
    const size_t ns = (size_t)db->nslots;
    HostCall c(db->device);
    if (c.status() != ORBX_OK) return c.status();
    const auto oqn = c.in(&qn, 1);
    const auto oqw = c.in(q_word, (size_t)qn);
    const auto oqv = c.in(q_weight, (size_t)qn);
    const auto oconn = c.in(connected, loop && connected ? ns : 0);
    const auto ocov = c.in(covis, covis ? ns * orbx::kKfdbCovis : 0);
    const auto onc = c.out<int>(1);
    const auto ocand = c.out<int>(ns);
    const auto owords = c.out<int>(ns);
    const auto oscores = c.out<float>(ns);
    orbx_status st = c.begin();
    if (st != ORBX_OK) return st;
    st = query(db, loop, c.dev(oqw), c.dev(oqv), c.dev(oqn), qn, loop && connected ? c.dev(oconn) : nullptr,
               covis ? c.dev(ocov) : nullptr, min_score, c.dev(ocand), c.dev(onc), words ? c.dev(owords) : nullptr,
               scores ? c.dev(oscores) : nullptr, c.stream());
    if (st != ORBX_OK) return st;
    int nc = 0;
    std::vector<int> all(ns);
    c.fetch(onc, &nc, 1);
    c.fetch(ocand, all.data(), ns);
    c.fetch(owords, words, ns);
    c.fetch(oscores, scores, ns);
    if ((st = c.finish()) != ORBX_OK) return st;
    db->ev_set = false;   // the call's stream has drained
    if (nc < 0 || (size_t)nc > ns) return ORBX_EDEVICE;
    *ncand = nc;
    for (int i = 0; i < nc && i < cap; ++i) cand[i] = all[(size_t)i];
    return nc > cap ? ORBX_ENOSPC : ORBX_OK;
}

orbx_status detect_device(orbv_database* db, bool loop, const int32_t* d_q_word, const double* d_q_weight,
                          const int* d_qn, int q_cap, const uint8_t* d_connected, const int32_t* d_covis,
                          float min_score, int nslots, int* d_cand, int* d_ncand, int* d_words, float* d_scores,
                          void* stream)
{
    if (!db || !d_q_word || !d_q_weight || !d_qn || q_cap <= 0 || q_cap > ORBV_MAX_FEATURES || !d_cand || !d_ncand)
        return ORBX_EINVAL;
    std::lock_guard<std::mutex> lk(db->mu);
    if (nslots != db->nslots) return ORBX_EINVAL;
    DeviceGuard guard(db->device);
    return query(db, loop, d_q_word, d_q_weight, d_qn, q_cap, d_connected, d_covis, min_score, d_cand, d_ncand,
                 d_words, d_scores, (hipStream_t)stream);
}

}  // namespace

extern "C" {

orbx_status orbv_score(int scoring, const int32_t* word1, const double* weight1, int n1, const int32_t* word2,
                       const double* weight2, int n2, double* score)
{
    if (scoring != 0 || n1 < 0 || n2 < 0 || n1 > ORBV_MAX_FEATURES || n2 > ORBV_MAX_FEATURES || !score ||
        (n1 > 0 && (!word1 || !weight1)) || (n2 > 0 && (!word2 || !weight2)))
        return ORBX_EINVAL;
    if (!ascending_in(word1, n1, INT_MAX) || !ascending_in(word2, n2, INT_MAX)) return ORBX_EINVAL;
    int i = 0, j = 0;
    double s = 0;
    while (i < n1 && j < n2) {
        const double vi = weight1[i], wi = weight2[j];
        if (word1[i] == word2[j]) {
            s += fabs(vi - wi) - fabs(vi) - fabs(wi);
            ++i;
            ++j;
        } else if (word1[i] < word2[j]) {
            i = (int)(std::lower_bound(word1 + i, word1 + n1, word2[j]) - word1);   // v1.lower_bound(v2_it->first)
        } else {
            j = (int)(std::lower_bound(word2 + j, word2 + n2, word1[i]) - word2);
        }
    }
    *score = -s / 2.0;
    return ORBX_OK;
}

orbx_status orbv_db_create(const orbx_vocabulary* v, int reserve_keyframes, int reserve_words, orbv_database** out)
{
    if (!v || !out || reserve_keyframes < 0 || reserve_words < 0) return ORBX_EINVAL;
    *out = nullptr;
    int scoring = -1, nwords = 0;
    if (orbv_info(v, nullptr, nullptr, &scoring, nullptr, nullptr, &nwords) != ORBX_OK || scoring != 0)
        return ORBX_EINVAL;   // L1_NORM only
    const int device = orbx::voc_device(v);
    if (!orbx::device_ok(device)) return ORBX_EDEVICE;
    DeviceGuard guard(device);
    orbv_database* db = new (std::nothrow) orbv_database();
    if (!db) return ORBX_ENOMEM;
    db->device = device;
    db->nwords = nwords;
    if (hipStreamCreateWithFlags(&db->stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&db->ev, hipEventDisableTiming) != hipSuccess) {
        orbv_db_destroy(db);
        return ORBX_EDEVICE;
    }
    if (!dalloc(db->d_meta, 2, db->stream)) {
        orbv_db_destroy(db);
        return ORBX_ENOMEM;
    }
    int rk = reserve_keyframes > 0 ? reserve_keyframes : 1024;
    if (rk > ORBV_DB_MAX_KEYFRAMES) rk = ORBV_DB_MAX_KEYFRAMES;
    const long long rw = reserve_words > 0 ? reserve_words : (long long)1 << 20;
    const orbx_status st = ensure(db, rk, rw);
    if (st != ORBX_OK) {
        orbv_db_destroy(db);
        return st;
    }
    *out = db;
    return ORBX_OK;
}

void orbv_db_destroy(orbv_database* db)
{
    if (!db) return;
    DeviceGuard guard(db->device);
    if (db->stream) {
        hipStream_t s = db->stream;
        follow(db, s);
        dfree(db->d_ptr, s);
        dfree(db->d_n, s);
        dfree(db->d_live, s);
        dfree(db->d_lscore, s);
        dfree(db->d_rscore, s);
        dfree(db->d_word, s);
        dfree(db->d_weight, s);
        dfree(db->d_words, s);
        dfree(db->d_minw, s);
        dfree(db->d_first, s);
        dfree(db->d_key, s);
        dfree(db->d_acc, s);
        dfree(db->d_best, s);
        dfree(db->d_meta, s);
        hipStreamSynchronize(s);
        hipStreamDestroy(s);
    }
    if (db->ev) hipEventDestroy(db->ev);
    delete db;
}

orbx_status orbv_db_add(orbv_database* db, const int32_t* bow_word, const double* bow_weight, int n, int* slot)
{
    if (!db || n < 0 || n > ORBV_MAX_FEATURES || (n > 0 && (!bow_word || !bow_weight))) return ORBX_EINVAL;
    if (!ascending_in(bow_word, n, db->nwords)) return ORBX_EINVAL;
    std::lock_guard<std::mutex> lk(db->mu);
    if (db->nslots >= ORBV_DB_MAX_KEYFRAMES) return ORBX_ENOSPC;
    HostCall c(db->device);
    if (c.status() != ORBX_OK) return c.status();
    const auto on = c.in(&n, 1);
    const auto ow = c.in(bow_word, (size_t)n);
    const auto ov = c.in(bow_weight, (size_t)n);
    orbx_status st = c.begin();
    if (st != ORBX_OK) return st;
    const int cap = n > 0 ? n : 1;
    st = append(db, c.dev(ow), c.dev(ov), c.dev(on), 1, cap, n, c.stream());
    if (st != ORBX_OK) return st;
    if ((st = c.finish()) != ORBX_OK) return st;
    if (slot) *slot = db->nslots - 1;
    return ORBX_OK;
}

orbx_status orbv_db_add_batch_device(orbv_database* db, const int32_t* d_bow_word, const double* d_bow_weight,
                                     const int* d_bow_n, int nframes, int cap, int* slots, void* stream)
{
    if (!db || nframes < 0 || cap <= 0 || cap > ORBV_MAX_FEATURES || !d_bow_word || !d_bow_weight || !d_bow_n)
        return ORBX_EINVAL;
    if (nframes == 0) return ORBX_OK;
    std::lock_guard<std::mutex> lk(db->mu);
    if ((long long)db->nslots + nframes > ORBV_DB_MAX_KEYFRAMES) return ORBX_ENOSPC;
    DeviceGuard guard(db->device);
    hipStream_t s = (hipStream_t)stream;
    std::vector<int> cnt((size_t)nframes);
    if (hipMemcpyAsync(cnt.data(), d_bow_n, sizeof(int) * nframes, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
        return ORBX_EDEVICE;
    long long total = 0;
    for (int f = 0; f < nframes; ++f) total += std::max(0, std::min(cnt[(size_t)f], cap));
    const int slot0 = db->nslots;
    const orbx_status st = append(db, d_bow_word, d_bow_weight, d_bow_n, nframes, cap, total, s);
    if (st != ORBX_OK) return st;
    if (slots)
        for (int f = 0; f < nframes; ++f) slots[f] = slot0 + f;
    return ORBX_OK;
}

orbx_status orbv_db_erase(orbv_database* db, int slot)
{
    if (!db) return ORBX_EINVAL;
    std::lock_guard<std::mutex> lk(db->mu);
    if (slot < 0 || slot >= db->nslots) return ORBX_EINVAL;
    if (!db->h_live[(size_t)slot]) return ORBX_OK;
    DeviceGuard guard(db->device);
    follow(db, db->stream);
    if (hipMemsetAsync(db->d_live + slot, 0, sizeof(int), db->stream) != hipSuccess ||
        hipStreamSynchronize(db->stream) != hipSuccess)
        return ORBX_EDEVICE;
    db->ev_set = false;
    db->h_live[(size_t)slot] = 0;
    return ORBX_OK;
}

orbx_status orbv_db_clear(orbv_database* db)
{
    if (!db) return ORBX_EINVAL;
    std::lock_guard<std::mutex> lk(db->mu);
    DeviceGuard guard(db->device);
    // queries still in flight read the storage: wait for them before the slots are reused
    follow(db, db->stream);
    if (hipStreamSynchronize(db->stream) != hipSuccess) return ORBX_EDEVICE;
    db->ev_set = false;
    db->nslots = 0;
    db->used = 0;
    db->h_live.clear();
    return ORBX_OK;
}

orbx_status orbv_db_info(const orbv_database* db, int* nslots, int* nlive, size_t* words_stored)
{
    if (!db) return ORBX_EINVAL;
    orbv_database* d = const_cast<orbv_database*>(db);
    std::lock_guard<std::mutex> lk(d->mu);
    if (nslots) *nslots = d->nslots;
    if (nlive) {
        int c = 0;
        for (uint8_t l : d->h_live) c += l ? 1 : 0;
        *nlive = c;
    }
    if (words_stored) *words_stored = (size_t)d->used;
    return ORBX_OK;
}

orbx_status orbv_db_scores(orbv_database* db, const int32_t* q_word, const double* q_weight, int qn, const int* slots,
                           int ns, double* scores)
{
    if (!db || qn < 0 || qn > ORBV_MAX_FEATURES || (qn > 0 && (!q_word || !q_weight)) || ns < 0 ||
        (ns > 0 && (!slots || !scores)))
        return ORBX_EINVAL;
    if (!ascending_in(q_word, qn, db->nwords)) return ORBX_EINVAL;
    if (ns == 0) return ORBX_OK;
    std::lock_guard<std::mutex> lk(db->mu);
    for (int i = 0; i < ns; ++i)
        if (slots[i] < 0 || slots[i] >= db->nslots) return ORBX_EINVAL;
    HostCall c(db->device);
    if (c.status() != ORBX_OK) return c.status();
    const auto oqn = c.in(&qn, 1);
    const auto oqw = c.in(q_word, (size_t)qn);
    const auto oqv = c.in(q_weight, (size_t)qn);
    const auto osl = c.in(slots, (size_t)ns);
    const auto osc = c.out<double>((size_t)ns);
    orbx_status st = c.begin();
    if (st != ORBX_OK) return st;
    follow(db, c.stream());
    const int nb = (ns + orbx::kKfdbScoreNT / 64 - 1) / (orbx::kKfdbScoreNT / 64);
    hipLaunchKernelGGL(orbx::k_kfdb_score, dim3(nb), dim3(orbx::kKfdbScoreNT), 0, c.stream(), db->d_ptr, db->d_n,
                       db->d_live, db->d_word, db->d_weight, db->nslots, c.dev(oqw), c.dev(oqv), c.dev(oqn), qn,
                       (const int*)nullptr, (const int*)nullptr, c.dev(osl), ns, (float*)nullptr, c.dev(osc));
    if (hipGetLastError() != hipSuccess) return ORBX_EDEVICE;
    c.fetch(osc, scores, (size_t)ns);
    if ((st = c.finish()) != ORBX_OK) return st;
    db->ev_set = false;
    return ORBX_OK;
}

orbx_status orbv_db_detect_loop(orbv_database* db, const int32_t* q_word, const double* q_weight, int qn,
                                const uint8_t* connected, const int32_t* covis, float min_score, int* cand, int cap,
                                int* ncand, int* words, float* scores)
{
    return detect_host(db, true, q_word, q_weight, qn, connected, covis, min_score, cand, cap, ncand, words, scores);
}

orbx_status orbv_db_detect_reloc(orbv_database* db, const int32_t* q_word, const double* q_weight, int qn,
                                 const int32_t* covis, int* cand, int cap, int* ncand, int* words, float* scores)
{
    return detect_host(db, false, q_word, q_weight, qn, nullptr, covis, 0.0f, cand, cap, ncand, words, scores);
}

orbx_status orbv_db_detect_loop_device(orbv_database* db, const int32_t* d_q_word, const double* d_q_weight,
                                       const int* d_qn, int q_cap, const uint8_t* d_connected,
                                       const int32_t* d_covis, float min_score, int nslots, int* d_cand,
                                       int* d_ncand, int* d_words, float* d_scores, void* stream)
{
    return detect_device(db, true, d_q_word, d_q_weight, d_qn, q_cap, d_connected, d_covis, min_score, nslots,
                         d_cand, d_ncand, d_words, d_scores, stream);
}

orbx_status orbv_db_detect_reloc_device(orbv_database* db, const int32_t* d_q_word, const double* d_q_weight,
                                        const int* d_qn, int q_cap, const int32_t* d_covis, int nslots, int* d_cand,
                                        int* d_ncand, int* d_words, float* d_scores, void* stream)
{
    return detect_device(db, false, d_q_word, d_q_weight, d_qn, q_cap, nullptr, d_covis, 0.0f, nslots, d_cand,
                         d_ncand, d_words, d_scores, stream);
}

}  // extern "C"

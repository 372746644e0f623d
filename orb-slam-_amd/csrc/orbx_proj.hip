// gfx950 kernels of the matchers that project MapPoints into a frame and search a window of its
// 64x48 grid in GetFeaturesInArea order (src/Frame.cc:410-495, src/KeyFrame.cc:569-608).  SURVEY.md §8f row 3.
//   LocalMapSearch   SearchByProjection(Frame&, vector<MapPoint*>, th) (src/ORBmatcher.cc:45-129), the
//                    local-map search of Tracking::SearchLocalPoints
//   PoseSearch<MODE> SearchByProjection(CurrentFrame, LastFrame) (:1396-1538), SearchByProjection(CurrentFrame,
//                    pKF, sAlreadyFound) (:1540-1667), SearchByProjection(pKF, Scw, ...) (:290-403),
//                    Fuse(pKF, ...) (:893-1043), Fuse(pKF, Scw, ...) (:1045-1168)
//   Sim3Search       SearchBySim3 (:1170-1394), with kernels of its own at the end of the file
// A search is a policy struct: its point and parameter types, the projection of a point to a window, the
// extra candidate test, the fields of a list entry, the accept test and which matches claim a feature.
// Every search runs the same three stages:
//
// J1 k_pj_grid     one workgroup per frame: (cell, feature) keys of AssignFeaturesToGrid
//                  sorted in LDS, so a window's columns are one key range and the keys
//                  run in GetFeaturesInArea's visiting order (ix, then iy, then insertion)
// J2 k_points<S>   kSub lanes per MapPoint: project it (S::project), then the reference's sequential scan
//                  over its window against the frame's claims on entry, kept as the first kTop candidates
//                  in (distance, visiting position) order -- best and second are the first two.  The Fuse
//                  overloads claim nothing during the search: they keep the first minimum and finish here.
// J3 k_resolve<S>  one wave per frame replays the MapPoints in order, 64 at a time
//                  (replay_chunks): each takes the first unclaimed entries of its list; the
//                  lanes before the first collision with an earlier lane's claim commit
//                  together; a MapPoint whose list ran out searches its window again.
//                  Assignments and claims live in LDS.  Then, for the searches that check rotation,
//                  ComputeThreeMaxima over per-feature bin masks.
// Float arithmetic is oracle/orbref.c proj_* operation for operation (no contraction in this
// file; the reference's GCC -march=native FMAs are explicit).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "orbx_device.hpp"
#include "orbx_host.hpp"
#include "orbx_kernels.hpp"

namespace orbx {

// J1 as a stable counting sort over the 3072 cells: per-cell counts by LDS atomics (the
// arrival slot is unordered), an exclusive scan, a scatter, then each feature's stable rank
// = the number of lower indices in its own cell segment (a few entries).  Keys are
// cell << 16 | index in ascending order, i.e. (cell, insertion) order.
constexpr int kPjCells = kFrameGridCols * kFrameGridRows;

// per frame: cap keys, then the kPjCells + 1 cell offsets (cell c = keys [off[c], off[c + 1]))
__host__ __device__ inline size_t pj_grid_stride(int cap) { return (size_t)cap + kPjCells + 4; }

__host__ __device__ inline size_t pj_grid_smem(int cap) { return (size_t)4 * (kPjCells + 4) + (size_t)6 * cap + 16; }

__global__ __launch_bounds__(256) void k_pj_grid(const orbx_keypoint* __restrict__ kps, const int* __restrict__ counts,
                                                 int cap, float min_x, float min_y, float grid_w_inv,
                                                 float grid_h_inv, uint32_t* __restrict__ gkeys)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t s_grid[];
    __shared__ uint32_t s_wsum[4];
    uint32_t* start = s_grid;                                   // [kPjCells + 1] counts, then offsets
    uint16_t* code = (uint16_t*)(s_grid + kPjCells + 4);        // [cap] cell, 0xFFFF = outside the grid
    uint16_t* pos = code + cap;                                 // [cap] arrival slot within the cell
    uint16_t* tmp = pos + cap;                                  // [cap] features grouped by cell
    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = min(counts[f], cap);
    for (int c = tid; c <= kPjCells; c += 256) start[c] = 0u;
    __syncthreads();
    const orbx_keypoint* k = kps + (size_t)f * cap;
    for (int i = tid; i < n; i += 256) {   // PosInGrid, src/Frame.cc:504-518
        const int px = (int)roundf((k[i].x - min_x) * grid_w_inv);
        const int py = (int)roundf((k[i].y - min_y) * grid_h_inv);
        uint16_t cc = 0xFFFF;
        if (px >= 0 && px < kFrameGridCols && py >= 0 && py < kFrameGridRows) {
            cc = (uint16_t)(px * kFrameGridRows + py);
            pos[i] = (uint16_t)atomicAdd(&start[cc], 1u);
        }
        code[i] = cc;
    }
    __syncthreads();
    constexpr int kPer = kPjCells / 256;   // 12 consecutive cells per thread
    uint32_t loc[kPer], sum = 0;
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
        loc[j] = start[tid * kPer + j];
        sum += loc[j];
    }
    uint32_t incl = sum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(incl, o);
        if (lane >= o) incl += y;
    }
    if (lane == 63) s_wsum[wave] = incl;
    __syncthreads();
    uint32_t base = incl - sum;
    for (int w = 0; w < wave; ++w) base += s_wsum[w];
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
        start[tid * kPer + j] = base;
        base += loc[j];
    }
    if (tid == 255) start[kPjCells] = base;
    __syncthreads();
    for (int i = tid; i < n; i += 256)
        if (code[i] != 0xFFFF) tmp[start[code[i]] + pos[i]] = (uint16_t)i;
    __syncthreads();
    uint32_t* out = gkeys + (size_t)f * pj_grid_stride(cap);
    for (int c = tid; c <= kPjCells; c += 256) out[cap + c] = start[c];   // cell -> first key position
    for (int i = tid; i < n; i += 256) {
        const int cc = code[i];
        if (cc == 0xFFFF) continue;
        const int s0 = (int)start[cc], s1 = (int)start[cc + 1];
        int r = 0;
        for (int j = s0; j < s1; ++j) r += tmp[j] < i;
        out[s0 + r] = (uint32_t)cc << 16 | (uint32_t)i;
    }
}

// The stream-ordered scratch of one call: the sorted grids of its frames, then (16-byte aligned) what the
// search keeps between its kernels -- the J2 lists, or SearchBySim3's vnMatch1 | vnMatch2.
struct GridScratch {
    uint32_t* gkeys;
    void* tail;
    size_t bytes;
    GridScratch(void* base, int nframes, int cap, size_t tail_bytes)
    {
        const size_t keys = ((size_t)nframes * pj_grid_stride(cap) * 4 + 15) & ~(size_t)15;
        gkeys = (uint32_t*)base;
        tail = (uint8_t*)base + keys;
        bytes = keys + tail_bytes;
    }
};

template <class Params>
static void launch_pj_grid(const orbx_keypoint* kps, const int* counts, int nframes, int cap, const Params& P,
                           uint32_t* gkeys, hipStream_t s)
{
    const size_t sm = pj_grid_smem(cap);
    hipFuncSetAttribute((const void*)k_pj_grid, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sm);
    hipLaunchKernelGGL(k_pj_grid, dim3(nframes), dim3(256), sm, s, kps, counts, cap, P.min_x, P.min_y, P.grid_w_inv,
                       P.grid_h_inv, gkeys);
}

// One frame of the batch as a search reads it: sorted grid, keypoints, right coordinates and claims on entry
// (both null in SearchBySim3, which reads neither), descriptors
struct FrameView {
    const uint32_t* keys;
    const orbx_keypoint* K;
    const float* U;
    const uint8_t* C;
    const uint8_t* D;
    int cap;
};

__device__ __forceinline__ FrameView frame_view(const orbx_keypoint* kps, const uint8_t* desc, const float* uright,
                                                const uint8_t* claimed, const uint32_t* gkeys, int f, int cap)
{
    const size_t o = (size_t)f * cap;
    return FrameView{gkeys + (size_t)f * pj_grid_stride(cap), kps + o, uright + o, claimed + o, desc + o * 32, cap};
}

// GetFeaturesInArea(u, v, r, minLevel, maxLevel) of one MapPoint: S::project fills the first line,
// proj_window the cell box and the key range [lo, hi) of its columns
struct ProjWindow {
    float u, v, r, ur;   // ur: the MapPoint's right coordinate, for the stereo tests
    int minLevel, maxLevel, cx0, cx1, cy0, cy1, lo, hi;
};

// The float -> int conversion of the cell bounds.  The two differ on NaN and out-of-range values, and each
// search keeps the one of its reference code: oracle/orbref.c:1546-1551 (local map), :1786-1795 (pose, Sim3).
struct CastInt {
    static __device__ __forceinline__ int of(float v) { return (int)v; }
};
struct X86Int {
    static __device__ __forceinline__ int of(float v) { return ps_x86_int(v); }
};

// false where GetFeaturesInArea returns no feature
template <class ToInt, class Params>
__device__ __forceinline__ bool proj_window(ProjWindow& w, const Params& P, const uint32_t* keys, int cap)
{
    w.lo = w.hi = 0;
    const int cx0 = max(0, ToInt::of(floorf((w.u - P.min_x - w.r) * P.grid_w_inv)));
    if (cx0 >= kFrameGridCols) return false;
    const int cx1 = min(kFrameGridCols - 1, ToInt::of(ceilf((w.u - P.min_x + w.r) * P.grid_w_inv)));
    if (cx1 < 0) return false;
    w.cy0 = max(0, ToInt::of(floorf((w.v - P.min_y - w.r) * P.grid_h_inv)));
    if (w.cy0 >= kFrameGridRows) return false;
    w.cy1 = min(kFrameGridRows - 1, ToInt::of(ceilf((w.v - P.min_y + w.r) * P.grid_h_inv)));
    if (w.cy1 < 0) return false;
    w.cx0 = cx0;
    w.cx1 = cx1;
    w.lo = (int)keys[cap + cx0 * kFrameGridRows];
    w.hi = (int)keys[cap + (cx1 + 1) * kFrameGridRows];
    return true;
}

// what a search tests after the shared row, level and box filter
enum { kNoExtra, kStereoExtra, kChi2Extra };

// candidate at key position p: the feature index if it is in the window and passes the search's extra
// test, else -1
template <class S>
__device__ __forceinline__ int window_candidate(const ProjWindow& w, const FrameView& F, int p,
                                                const typename S::Params& P)
{
    const uint32_t key = F.keys[p];
    const int iy = (int)(key >> 16) % kFrameGridRows;
    if (iy < w.cy0 || iy > w.cy1) return -1;
    const int idx = (int)(key & 0xFFFF);
    const orbx_keypoint kp = F.K[idx];
    if (kp.octave < w.minLevel) return -1;
    if (w.maxLevel >= 0 && kp.octave > w.maxLevel) return -1;
    const float distx = kp.x - w.u, disty = kp.y - w.v;
    if (!(fabsf(distx) < w.r && fabsf(disty) < w.r)) return -1;
    if constexpr (S::kExtra == kStereoExtra) {   // :86-91, :1475-1481
        const float ur = F.U[idx];
        if (ur > 0 && fabsf(w.ur - ur) > w.r) return -1;
    }
    if constexpr (S::kExtra == kChi2Extra) {   // :982-1006
        const float ur = F.U[idx];
        const float ex = w.u - kp.x, ey = w.v - kp.y;
        const float is2 = P.inv_sigma2[kp.octave & 15];
        if (ur >= 0) {
            const float er = w.ur - ur;
            const float e2 = __builtin_fmaf(er, er, __builtin_fmaf(ex, ex, ey * ey));
            if ((double)(e2 * is2) > 7.8) return -1;
        } else {
            const float e2 = __builtin_fmaf(ex, ex, ey * ey);
            if ((double)(e2 * is2) > 5.99) return -1;
        }
    }
    return idx;
}

// The first kTop candidates of a window in (distance, visiting position) order -- the order in which
// the reference's sequential strict-< scan ranks them -- packed as dist:9 | bin:5 | octave:4 | idx:14
// (frames of up to ORBM_MAX_FEATURES = 16384 features; a distance is at most 256, 9 bits).
// A claim made later in the call only removes candidates, so the replay takes the first unclaimed
// entries of this list and scans the window again only when more than kTop were taken.
constexpr int kTop = 8;
struct TopK {
    uint32_t e[kTop];
    int n;   // candidates seen (saturating at 255)
};

__device__ __forceinline__ uint32_t top_entry(int dist, int bin, int oct, int idx)
{
    return (uint32_t)dist << 23 | (uint32_t)bin << 18 | (uint32_t)(oct & 15) << 14 | (uint32_t)idx;
}
static_assert(ORBM_MAX_FEATURES <= (1 << 14), "top_entry packs a feature index in 14 bits");
__device__ __forceinline__ int top_idx(uint32_t e) { return (int)(e & 0x3FFF); }
__device__ __forceinline__ int top_oct(uint32_t e) { return (int)((e >> 14) & 15); }
__device__ __forceinline__ int top_bin(uint32_t e) { return (int)((e >> 18) & 31); }
__device__ __forceinline__ int top_dist(uint32_t e) { return (int)(e >> 23); }

__device__ __forceinline__ void top_insert(TopK& t, uint32_t entry)
{
    const uint32_t dnew = entry >> 23;
    uint32_t carry = entry;
    bool shifting = false;   // stable: after the entries of equal distance, then everything moves down
#pragma unroll
    for (int k = 0; k < kTop; ++k) {
        const bool take = shifting || k >= t.n || (t.e[k] >> 23) > dnew;
        if (take) {
            const uint32_t x = t.e[k];
            t.e[k] = carry;
            carry = x;
            shifting = true;
        }
    }
    t.n = min(t.n + 1, 255);
}

// J2 / P1 give a MapPoint kSub adjacent lanes: sub-lane s scans window positions lo + s, lo + s +
// kSub, ...  Each keeps its own first kTop as 64-bit keys dist:9 | position:16 | entry low 23 bits
// (bin, octave, index), i.e. in (distance, visiting position) order, and the group merges its
// lists by kTop rounds of a min over the group's heads.  Same list as one sequential scan.
constexpr int kSub = 4;
struct TopK64 {
    unsigned long long e[kTop];
    int n;   // candidates this sub-lane saw (saturating)
};

__device__ __forceinline__ unsigned long long top_key(uint32_t entry, int p)
{
    return (unsigned long long)(entry >> 23) << 39 | (unsigned long long)p << 23 | (entry & 0x7FFFFFu);
}

__device__ __forceinline__ void top64_insert(TopK64& t, unsigned long long key)
{
    unsigned long long carry = key;
    bool shifting = false;   // positions only grow within a sub-lane: equal distances stay in visiting order
#pragma unroll
    for (int k = 0; k < kTop; ++k) {
        const bool take = shifting || k >= t.n || t.e[k] > key;
        if (take) {
            const unsigned long long x = t.e[k];
            t.e[k] = carry;
            carry = x;
            shifting = true;
        }
    }
    t.n = min(t.n + 1, 255);
}

__device__ __forceinline__ unsigned long long sub_min_u64(unsigned long long v)
{
#pragma unroll
    for (int o = 1; o < kSub; o <<= 1) {
        const unsigned long long y = __shfl_xor(v, o);
        v = y < v ? y : v;
    }
    return v;
}

// every lane of the group returns the merged list (entries as top_entry packs them)
__device__ __forceinline__ TopK top_merge(TopK64& t)
{
    int total = t.n;
#pragma unroll
    for (int o = 1; o < kSub; o <<= 1) total += __shfl_xor(total, o);
    TopK out;
    out.n = min(total, 255);
    int have = min(t.n, kTop);
#pragma unroll
    for (int r = 0; r < kTop; ++r) {
        const unsigned long long h = have > 0 ? t.e[0] : ~0ull;
        const unsigned long long m = sub_min_u64(h);
        if (have > 0 && h == m) {   // keys are unique (positions): only the owner pops
#pragma unroll
            for (int k = 0; k + 1 < kTop; ++k) t.e[k] = t.e[k + 1];
            --have;
        }
        out.e[r] = m == ~0ull ? 0u : (uint32_t)((m >> 39) << 23 | (m & 0x7FFFFFu));
    }
    return out;
}

// J2 result per MapPoint: the top-kTop list and the accept decision of its first entries
struct TopResult {
    uint32_t e[kTop];
    int n;        // candidates in the window (not claimed on entry), saturating
    int accept;   // the reference's accept test on the J2 best (and second)
};

// a candidate as (distance, visiting position, index): the minimum is the first minimum of the sequential scan
__device__ __forceinline__ unsigned long long first_key(int dist, int p, int idx)
{
    return (unsigned long long)dist << 32 | (unsigned long long)p << 16 | (unsigned)idx;
}

// Sub-lane `sub` of a MapPoint's kSub lanes walks the window's columns in GetFeaturesInArea order (rows
// cy0..cy1 only): visit(position, index, distance) for every candidate that passes the search's tests and,
// in a claiming search, is not claimed on entry.  q0 | q1 is the MapPoint's descriptor.
template <class S, class Visit>
__device__ __forceinline__ void walk_window(const ProjWindow& w, const FrameView& F, int sub, const uint4& q0,
                                            const uint4& q1, const typename S::Params& P, Visit visit)
{
    for (int cx = w.cx0; cx <= w.cx1; ++cx) {
        const int a = (int)F.keys[F.cap + cx * kFrameGridRows + w.cy0], b = (int)F.keys[F.cap + cx * kFrameGridRows + w.cy1 + 1];
        for (int p = a + sub; p < b; p += kSub) {
            const int idx = window_candidate<S>(w, F, p, P);
            if (idx < 0 || (S::kClaims && F.C[idx])) continue;
            const uint4* d = reinterpret_cast<const uint4*>(F.D + (size_t)idx * 32);
            visit(p, idx, ham256(q0, q1, d[0], d[1]));
        }
    }
}

// One wave searches the window again against the claims on entry and those made in this call: b1 = the
// first minimum as first_key packs it and, where the accept test needs it (S::kSecond), b2 = the first
// minimum of the rest -- the sequential scan's best and second.  ~0 = none.
template <class S>
__device__ __forceinline__ void rescan_window(const ProjWindow& w, const FrameView& F, const uint8_t* taken,
                                              const uint4& q0, const uint4& q1, const typename S::Params& P,
                                              unsigned long long& b1, unsigned long long& b2)
{
    const int lane = threadIdx.x;
    b1 = b2 = ~0ull;
    for (int p0 = w.lo; p0 < w.hi; p0 += 64) {
        const int p = p0 + lane;
        unsigned long long key = ~0ull;
        if (p < w.hi) {
            const int idx = window_candidate<S>(w, F, p, P);
            if (idx >= 0 && !F.C[idx] && !taken[idx]) {
                const uint4* d = reinterpret_cast<const uint4*>(F.D + (size_t)idx * 32);
                key = first_key(ham256(q0, q1, d[0], d[1]), p, idx);
            }
        }
        const unsigned long long c1 = wave_min_shfl(key);
        if constexpr (S::kSecond) {   // merge: the multiset top two by (dist, position)
            const unsigned long long c2 = wave_min_shfl(key == c1 ? ~0ull : key);
            if (c1 < b1) {
                b2 = min(b1, c2);
                b1 = c1;
            } else {
                b2 = min(b2, c1);
            }
        } else {
            b1 = c1 < b1 ? c1 : b1;
        }
    }
}

// ---- chunk-parallel, in-order replay of the reference's greedy loop (both searches) ----
// A claim made earlier in the call only removes candidates, so each MapPoint's result is a function
// of its J2 list and of the claims of the MapPoints before it.  A chunk of 64 MapPoints settles in
// rounds: every pending lane takes the first unclaimed entries of its list; the first lane whose
// choice collides with a claim of an earlier pending lane, or whose list ran out, stops the round;
// the lanes before it are final and commit together (last writer = the largest MapPoint index,
// claims, rotation bins); the next round starts at that lane, which now sees every claim before it.
// A lane whose list ran out searches its window again, wave-parallel, against the claims.
struct ReplayLds {
    int* mo;          // [cap] MapPoint assigned to the feature (last writer), -1
    uint32_t* bins;   // [cap] rotation bins of the matches that assigned the feature
    int* first;       // [cap] smallest pending lane claiming the feature in this round (64 = none)
    uint8_t* taken;   // [cap] claimed earlier in this call
    int* hist;        // [32] rotHist sizes
};

// kBig (frames of more than kReplayLdsCap features): `mo` is the frame's output row in global memory (the
// last-writer atomics go to it directly, and the final copy is in place), the rest stays in LDS: 9 bytes per
// feature instead of 13, so up to kProjMaxFeatures features fit a workgroup's 160 KiB.
constexpr int kReplayLdsCap = 8192;
template <bool kBig>
__device__ __forceinline__ ReplayLds replay_lds(int cap, int* mo_global)
{
    extern __shared__ int s_replay[];
    ReplayLds S;
    if constexpr (kBig) {
        S.mo = mo_global;
        S.bins = reinterpret_cast<uint32_t*>(s_replay);
        S.first = s_replay + cap;
        S.hist = s_replay + 2 * cap;
        S.taken = reinterpret_cast<uint8_t*>(s_replay + 2 * cap + 32);
    } else {
        S.mo = s_replay;
        S.bins = reinterpret_cast<uint32_t*>(s_replay + cap);
        S.first = s_replay + 2 * cap;
        S.hist = s_replay + 3 * cap;
        S.taken = reinterpret_cast<uint8_t*>(s_replay + 3 * cap + 32);
    }
    return S;
}

inline size_t replay_lds_bytes(int cap) { return cap > kReplayLdsCap ? (size_t)9 * cap + 128 : (size_t)13 * cap + 128; }

struct ReplayPick {
    int g, accept, bin;
};

template <bool kSecond, bool kRot, class ObsFn, class AcceptFn, class RescanFn>
__device__ __forceinline__ int replay_chunks(int n, int np, const TopResult* __restrict__ R, const ReplayLds& S,
                                             ObsFn obs_of, AcceptFn accept_of, RescanFn rescan)
{
    const int lane = threadIdx.x;
    for (int i = lane; i < n; i += 64) {
        S.mo[i] = -1;
        S.bins[i] = 0u;
        S.first[i] = 64;
        S.taken[i] = 0;
    }
    if (lane < 32) S.hist[lane] = 0;
    __syncthreads();
    int count = 0;
    for (int base = 0; base < np; base += 64) {
        const int m = base + lane;
        TopResult r{{0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u}, 0, 0};
        int obs = 0;
        if (m < np) {
            r = R[m];
            obs = obs_of(m);
        }
        // no candidate, or (single-best searches) a J2 best over the threshold: final, no match
        bool pending = r.n > 0 && (kSecond || r.accept);
        unsigned long long pend = __ballot(pending);
        while (pend) {
            int k1 = -1, k2 = -1;
            uint32_t c1 = 0u, c2 = 0u;
            bool out_of_list = false;
            if (pending) {
                const int lim = min(r.n, kTop);
#pragma unroll
                for (int k = 0; k < kTop; ++k) {
                    if (k < lim && (kSecond ? k2 < 0 : k1 < 0) && !S.taken[top_idx(r.e[k])]) {
                        if (k1 < 0) {
                            k1 = k;
                            c1 = r.e[k];
                        } else {
                            k2 = k;
                            c2 = r.e[k];
                        }
                    }
                }
                out_of_list = (kSecond ? k2 < 0 : k1 < 0) && r.n > kTop;
            }
            const bool acc = pending && !out_of_list && k1 >= 0 && accept_of(c1, k2 >= 0, c2);
            const bool claim = acc && obs;
            if (claim) atomicMin(&S.first[top_idx(c1)], lane);
            __syncthreads();
            bool stop = pending && out_of_list;
            if (pending && !out_of_list && k1 >= 0)
                stop = S.first[top_idx(c1)] < lane || (kSecond && k2 >= 0 && S.first[top_idx(c2)] < lane);
            __syncthreads();
            if (claim) S.first[top_idx(c1)] = 64;
            const unsigned long long stops = __ballot(stop);
            const int j0 = stops ? __builtin_ctzll(stops) : 64;
            const bool commit = pending && lane < j0;
            if (commit && acc) {
                const int g = top_idx(c1);
                atomicMax(&S.mo[g], m);   // F.mvpMapPoints[bestIdx] = pMP, in MapPoint order
                if (kRot) {
                    atomicOr(&S.bins[g], 1u << top_bin(c1));
                    atomicAdd(&S.hist[top_bin(c1)], 1);
                }
                if (obs) S.taken[g] = 1;
            }
            count += __popcll(__ballot(commit && acc));
            if (commit) pending = false;
            __syncthreads();
            if (j0 < 64 && __builtin_amdgcn_readlane((int)out_of_list, j0)) {   // wave-uniform
                const ReplayPick pk = rescan(base + j0, S.taken);
                if (pk.accept) {
                    if (lane == 0) {
                        atomicMax(&S.mo[pk.g], base + j0);
                        if (kRot) {
                            atomicOr(&S.bins[pk.g], 1u << pk.bin);
                            atomicAdd(&S.hist[pk.bin], 1);
                        }
                        if (__builtin_amdgcn_readlane(obs, j0)) S.taken[pk.g] = 1;
                    }
                    ++count;
                }
                if (lane == j0) pending = false;
                __syncthreads();
            }
            pend = __ballot(pending);
        }
    }
    __syncthreads();
    return count;
}

// ---- the searches ----
// SearchByProjection(F, vpMapPoints, th): Frame::isInFrustum has projected the MapPoint already
struct LocalMapSearch {
    using Point = orbm_proj_point;
    using Params = orbm_proj_params;
    using ToInt = CastInt;
    struct Ctx {};
    static constexpr int kExtra = kStereoExtra;
    static constexpr bool kClaims = true, kSecond = true;

    static __device__ __forceinline__ Ctx context(const float*, int, const Params&) { return Ctx{}; }
    static __device__ __forceinline__ bool project(const Ctx&, const Point& M, const Params& P, ProjWindow& w)
    {
        const int level = M.level;
        if (level < 0 || level >= 16) return false;   // outside mvScaleFactors: UB in the reference
        float r = M.view_cos > 0.998 ? 2.5f : 4.0f;   // RadiusByViewingCos, src/ORBmatcher.cc:130-136
        if (P.th != 1.0f) r *= P.th;
        w.r = r * P.scale[level];
        w.u = M.proj_x;
        w.v = M.proj_y;
        w.ur = M.proj_xr;
        w.minLevel = level - 1;   // bCheckLevels is true for level >= 0
        w.maxLevel = level;
        return true;
    }
    static __device__ __forceinline__ bool rot(const Params&) { return false; }
    static __device__ __forceinline__ int bin(const Point&, const orbx_keypoint&) { return 0; }
    static __device__ __forceinline__ int oct(const orbx_keypoint& kp) { return kp.octave; }
    // best (d1, level l1) against the second (d2, l2; 256, -1 = none).  A candidate at distance 256 is never
    // the reference's second (dist < bestDist2 = 256 fails, :100-104): bestLevel2 stays -1, from a list entry
    // and from a rescan's b2 alike
    static __device__ __forceinline__ bool accept(const Params& P, int d1, int l1, int d2, int l2)
    {
        if (!(d1 <= 100)) return false;   // TH_HIGH
        if (d2 >= 256) l2 = -1;
        if (l1 == l2 && (float)d1 > P.nnratio * (float)d2) return false;
        return true;
    }
    static __device__ __forceinline__ int obs(const Point& M) { return (M.flags & 2) ? 1 : 0; }
};

// the per-MapPoint part before GetFeaturesInArea; false where the reference `continue`s
template <int MODE>
__device__ __forceinline__ bool ps_project(const PsCam& c, const orbm_map_point& M, const orbm_pose_params& P,
                                           ProjWindow& w)
{
    const float X = M.x, Y = M.y, Z = M.z;
    const float xc = ps_row(c.R, 1, X, Y, Z) + c.t[0];
    const float yc = ps_row(c.R + 3, 1, X, Y, Z) + c.t[1];
    const float zc = ps_row(c.R + 6, 1, X, Y, Z) + c.t[2];
    w.ur = 0.0f;
    if (MODE == ORBM_PROJ_LAST_FRAME || MODE == ORBM_PROJ_KEYFRAME) {
        const float invzc = (float)(1.0 / (double)zc);
        if (MODE == ORBM_PROJ_LAST_FRAME && invzc < 0) return false;
        const float u = __builtin_fmaf(P.fx * xc, invzc, P.cx);   // fx*xc*invzc+cx
        const float v = __builtin_fmaf(P.fy * yc, invzc, P.cy);
        if (u < P.min_x || u > P.max_x) return false;
        if (v < P.min_y || v > P.max_y) return false;
        w.u = u;
        w.v = v;
        if (MODE == ORBM_PROJ_LAST_FRAME) {   // :1446-1458
            const int L = M.octave & 15;
            w.r = P.th * P.scale[L];
            if (c.fwd) { w.minLevel = L; w.maxLevel = -1; }
            else if (c.bwd) { w.minLevel = 0; w.maxLevel = L; }
            else { w.minLevel = L - 1; w.maxLevel = L + 1; }
            w.ur = __builtin_fmaf(-P.bf, invzc, u);   // u - mbf*invzc
            return true;
        }
    } else {
        if (zc < 0.0f) return false;
        const float invz = MODE == ORBM_FUSE_SIM3 ? (float)(1.0 / (double)zc) : 1.0f / zc;
        const float x = xc * invz, y = yc * invz;
        const float u = __builtin_fmaf(P.fx, x, P.cx);
        const float v = __builtin_fmaf(P.fy, y, P.cy);
        if (!(u >= P.min_x && u < P.max_x && v >= P.min_y && v < P.max_y)) return false;   // IsInImage
        w.u = u;
        w.v = v;
        if (MODE == ORBM_FUSE) w.ur = __builtin_fmaf(-P.bf, invz, u);
    }
    const float maxD = 1.2f * M.max_dist, minD = 0.8f * M.min_dist;
    const float PO0 = X - c.Ow[0], PO1 = Y - c.Ow[1], PO2 = Z - c.Ow[2];
    double s = 0.0;
    s += (double)PO0 * (double)PO0;
    s += (double)PO1 * (double)PO1;
    s += (double)PO2 * (double)PO2;
    const float dist = (float)__builtin_sqrt(s);   // cv::norm(PO)
    if (dist < minD || dist > maxD) return false;
    if (MODE != ORBM_PROJ_KEYFRAME) {   // PO.dot(Pn) < 0.5*dist
        double dot = 0.0;
        dot += (double)PO0 * (double)M.nx;
        dot += (double)PO1 * (double)M.ny;
        dot += (double)PO2 * (double)M.nz;
        if (dot < 0.5 * (double)dist) return false;
    }
    const int L = ps_predict_scale(M.max_dist, dist, P);
    w.r = P.th * P.scale[L & 15];
    w.minLevel = L - 1;
    w.maxLevel = MODE == ORBM_PROJ_KEYFRAME ? L + 1 : L;
    return true;
}

// ps_x86_int, ps_row, PsCam / ps_camera and ps_predict_scale (MapPoint::PredictScale) are shared with
// Frame::isInFrustum (orbx_frame.hip): orbx_device.hpp
template <int MODE>
struct PoseSearch {
    using Point = orbm_map_point;
    using Params = orbm_pose_params;
    using ToInt = X86Int;
    using Ctx = PsCam;
    static constexpr int kExtra = MODE == ORBM_PROJ_LAST_FRAME ? kStereoExtra : (MODE == ORBM_FUSE ? kChi2Extra : kNoExtra);
    static constexpr bool kClaims = MODE <= ORBM_PROJ_SIM3, kSecond = false;

    static __device__ __forceinline__ Ctx context(const float* pose, int f, const Params& P)
    {
        return ps_camera(MODE, pose + (size_t)f * 24, P);
    }
    static __device__ __forceinline__ bool project(const Ctx& c, const Point& M, const Params& P, ProjWindow& w)
    {
        return ps_project<MODE>(c, M, P, w);
    }
    static __device__ __forceinline__ bool rot(const Params& P)
    {
        return (MODE == ORBM_PROJ_LAST_FRAME || MODE == ORBM_PROJ_KEYFRAME) && P.check_ori;
    }
    static __device__ __forceinline__ int bin(const Point& M, const orbx_keypoint& kp) { return rot_bin(M.angle, kp.angle); }
    static __device__ __forceinline__ int oct(const orbx_keypoint&) { return 0; }
    static __device__ __forceinline__ bool accept(const Params& P, int d1, int, int, int)
    {
        return d1 <= (MODE == ORBM_PROJ_LAST_FRAME ? 100 : (MODE == ORBM_PROJ_KEYFRAME ? P.orb_dist : 50));   // TH_HIGH / TH_LOW
    }
    // LAST_FRAME claims a feature only for a MapPoint with Observations() > 0 (:1471-1473); the
    // other searches skip every feature already assigned (:1609-1610, :375-376)
    static __device__ __forceinline__ int obs(const Point& M) { return MODE != ORBM_PROJ_LAST_FRAME || (M.flags & 2) ? 1 : 0; }
};

template <class S>
__global__ __launch_bounds__(256) void k_points(const orbx_keypoint* __restrict__ kps, const uint8_t* __restrict__ desc,
                                                const float* __restrict__ uright, const uint8_t* __restrict__ claimed,
                                                int cap, const float* __restrict__ pose,
                                                const typename S::Point* __restrict__ pts,
                                                const uint8_t* __restrict__ pdesc, const int* __restrict__ npts, int pcap,
                                                typename S::Params P, const uint32_t* __restrict__ gkeys,
                                                TopResult* __restrict__ res, int* __restrict__ match,
                                                int* __restrict__ nmatches)
{
    const int f = blockIdx.y, m = blockIdx.x * (256 / kSub) + threadIdx.x / kSub, sub = threadIdx.x % kSub;
    if (m >= min(npts[f], pcap)) return;   // uniform over the kSub lanes of a MapPoint
    const size_t mo = (size_t)f * pcap + m;
    TopK64 T64;
    T64.n = 0;
#pragma unroll
    for (int k = 0; k < kTop; ++k) T64.e[k] = 0ull;
    unsigned long long best = ~0ull;   // a search without claims: the first minimum
    const typename S::Point M = pts[mo];
    bool scanned = false;
    if (M.flags & 1) {
        const typename S::Ctx c = S::context(pose, f, P);
        const FrameView F = frame_view(kps, desc, uright, claimed, gkeys, f, cap);
        ProjWindow w;
        if (S::project(c, M, P, w) && proj_window<typename S::ToInt>(w, P, F.keys, cap)) {
            scanned = true;
            const uint4* qd = reinterpret_cast<const uint4*>(pdesc + mo * 32);
            const uint4 q0 = qd[0], q1 = qd[1];
            const bool rot = S::rot(P);
            if constexpr (S::kClaims)
                walk_window<S>(w, F, sub, q0, q1, P, [&](int p, int idx, int dist) {
                    top64_insert(T64, top_key(top_entry(dist, rot ? S::bin(M, F.K[idx]) : 0, S::oct(F.K[idx]), idx), p));
                });
            else
                walk_window<S>(w, F, sub, q0, q1, P, [&](int p, int idx, int dist) {
                    const unsigned long long key = first_key(dist, p, idx);
                    best = key < best ? key : best;
                });
        }
    }
    if constexpr (S::kClaims) {
        const TopK T = top_merge(T64);   // whole group: `scanned` is uniform over it
        if (sub != 0) return;
        TopResult R;
#pragma unroll
        for (int k = 0; k < kTop; ++k) R.e[k] = T.e[k];
        R.n = T.n;
        // the scan's best / second are the first two entries (multiset top two, first wins ties)
        R.accept = scanned && T.n > 0 &&
                   S::accept(P, top_dist(T.e[0]), top_oct(T.e[0]), T.n > 1 ? top_dist(T.e[1]) : 256,
                             T.n > 1 ? top_oct(T.e[1]) : -1);
        res[mo] = R;
    } else {
        best = sub_min_u64(best);
        if (sub != 0) return;
        const bool accept = best != ~0ull && S::accept(P, (int)(best >> 32), 0, 256, -1);
        match[mo] = accept ? (int)(best & 0xFFFF) : -1;
        if (accept) atomicAdd(&nmatches[f], 1);
    }
}

template <class S, bool kBig>
__global__ __launch_bounds__(64) void k_resolve(const orbx_keypoint* __restrict__ kps, const uint8_t* __restrict__ desc,
                                                const float* __restrict__ uright, const uint8_t* __restrict__ claimed,
                                                const int* __restrict__ counts, int cap, const float* __restrict__ pose,
                                                const typename S::Point* __restrict__ pts,
                                                const uint8_t* __restrict__ pdesc, const int* __restrict__ npts, int pcap,
                                                typename S::Params P, const uint32_t* __restrict__ gkeys,
                                                const TopResult* __restrict__ res, int* __restrict__ match,
                                                int* __restrict__ nmatches)
{
    const int f = blockIdx.x, lane = threadIdx.x;
    const int n = min(counts[f], cap), np = min(npts[f], pcap);
    int* Mo = match + (size_t)f * cap;
    const ReplayLds L = replay_lds<kBig>(cap, Mo);
    const FrameView F = frame_view(kps, desc, uright, claimed, gkeys, f, cap);
    const typename S::Point* Pf = pts + (size_t)f * pcap;
    const typename S::Ctx c = S::context(pose, f, P);
    const bool rot = S::rot(P);
    auto obs_of = [&](int m) { return S::obs(Pf[m]); };
    auto accept_of = [&](uint32_t c1, bool has2, uint32_t c2) {
        return S::accept(P, top_dist(c1), top_oct(c1), has2 ? top_dist(c2) : 256, has2 ? top_oct(c2) : -1);
    };
    auto rescan = [&](int m, const uint8_t* taken) {
        const typename S::Point Mp = Pf[m];
        ProjWindow w;
        S::project(c, Mp, P, w);   // true and non-empty: J2 found candidates in it
        proj_window<typename S::ToInt>(w, P, F.keys, cap);
        const uint4* qd = reinterpret_cast<const uint4*>(pdesc + ((size_t)f * pcap + m) * 32);
        const uint4 q0 = qd[0], q1 = qd[1];
        unsigned long long b1, b2;
        rescan_window<S>(w, F, taken, q0, q1, P, b1, b2);
        ReplayPick pk{-1, 0, 0};
        if (b1 != ~0ull) {
            pk.g = (int)(b1 & 0xFFFF);
            const bool has2 = b2 != ~0ull;
            pk.accept = S::accept(P, (int)(b1 >> 32), S::oct(F.K[pk.g]), has2 ? (int)(b2 >> 32) : 256,
                                  has2 ? S::oct(F.K[(int)(b2 & 0xFFFF)]) : -1);
            if (rot) pk.bin = S::bin(Mp, F.K[pk.g]);
        }
        return pk;
    };
    int count = rot ? replay_chunks<S::kSecond, true>(n, np, res + (size_t)f * pcap, L, obs_of, accept_of, rescan)
                    : replay_chunks<S::kSecond, false>(n, np, res + (size_t)f * pcap, L, obs_of, accept_of, rescan);
    uint32_t drop = 0u;   // the bins outside the three maxima
    if (rot) {            // ComputeThreeMaxima (:1679-1723); every match in another bin is undone
        int ind1, ind2, ind3;
        three_maxima(L.hist, ind1, ind2, ind3);
        drop = 0x3FFFFFFFu;
        if (ind1 >= 0) drop &= ~(1u << ind1);
        if (ind2 >= 0) drop &= ~(1u << ind2);
        if (ind3 >= 0) drop &= ~(1u << ind3);
        for (int i = 0; i < kHisto; ++i)
            if ((drop >> i) & 1u) count -= L.hist[i];
    }
    if (rot || !kBig)   // kBig: the assignments are in the output row already; the filter NULLs in place
        for (int i = lane; i < n; i += 64) Mo[i] = (L.bins[i] & drop) ? -2 : L.mo[i];
    if (lane == 0) nmatches[f] = count;
}

static size_t proj_scratch_bytes(int nframes, int cap, int pcap)
{
    return GridScratch(nullptr, nframes, cap, (size_t)nframes * pcap * sizeof(TopResult)).bytes;
}

// J1, J2 and, for a search with claims, J3 of one call
template <class S>
static void launch_search(const orbx_keypoint* kps, const uint8_t* desc, const float* uright, const uint8_t* claimed,
                          const int* counts, int nframes, int cap, const float* pose, const typename S::Point* pts,
                          const uint8_t* pdesc, const int* npts, int pcap, const typename S::Params& P, void* scratch,
                          int* match, int* nmatches, hipStream_t s)
{
    const GridScratch sc(scratch, nframes, cap, 0);
    TopResult* res = (TopResult*)sc.tail;
    launch_pj_grid(kps, counts, nframes, cap, P, sc.gkeys, s);
    if (!S::kClaims) hipMemsetAsync(nmatches, 0, sizeof(int) * (size_t)nframes, s);
    hipLaunchKernelGGL(k_points<S>, dim3((pcap + 256 / kSub - 1) / (256 / kSub), nframes), dim3(256), 0, s, kps, desc,
                       uright, claimed, cap, pose, pts, pdesc, npts, pcap, P, sc.gkeys, res, match, nmatches);
    if constexpr (S::kClaims) {
        auto resolve = [&](auto kern) {
            hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)replay_lds_bytes(cap));
            hipLaunchKernelGGL(kern, dim3(nframes), dim3(64), replay_lds_bytes(cap), s, kps, desc, uright, claimed,
                               counts, cap, pose, pts, pdesc, npts, pcap, P, sc.gkeys, res, match, nmatches);
        };
        if (cap > kReplayLdsCap) resolve(k_resolve<S, true>);
        else resolve(k_resolve<S, false>);
    }
}

static void launch_proj(const orbx_keypoint* kps, const uint8_t* desc, const float* uright, const uint8_t* claimed,
                        const int* counts, int nframes, int cap, const orbm_proj_point* pts, const uint8_t* pdesc,
                        const int* npts, int pcap, const orbm_proj_params& P, void* scratch, int* match, int* nmatches,
                        hipStream_t s)
{
    launch_search<LocalMapSearch>(kps, desc, uright, claimed, counts, nframes, cap, nullptr, pts, pdesc, npts, pcap, P,
                                  scratch, match, nmatches, s);
}

// fn(PoseSearch<mode>{})
template <class Fn>
static void with_pose_search(int mode, Fn fn)
{
    switch (mode) {
    case ORBM_PROJ_LAST_FRAME: return fn(PoseSearch<ORBM_PROJ_LAST_FRAME>{});
    case ORBM_PROJ_KEYFRAME: return fn(PoseSearch<ORBM_PROJ_KEYFRAME>{});
    case ORBM_PROJ_SIM3: return fn(PoseSearch<ORBM_PROJ_SIM3>{});
    case ORBM_FUSE: return fn(PoseSearch<ORBM_FUSE>{});
    default: return fn(PoseSearch<ORBM_FUSE_SIM3>{});
    }
}

static void launch_pose_search(int mode, const orbx_keypoint* kps, const uint8_t* desc, const float* uright,
                               const uint8_t* claimed, const int* counts, int nframes, int cap, const float* pose,
                               const orbm_map_point* pts, const uint8_t* pdesc, const int* npts, int pcap,
                               const orbm_pose_params& P, void* scratch, int* match, int* nmatches, hipStream_t s)
{
    with_pose_search(mode, [&](auto search) {
        launch_search<decltype(search)>(kps, desc, uright, claimed, counts, nframes, cap, pose, pts, pdesc, npts, pcap,
                                        P, scratch, match, nmatches, s);
    });
}

// =====================================================================================
// ORBmatcher::SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th) (:1170-1394), the mutual
// search of LoopClosing::ComputeSim3 (src/LoopClosing.cc:323).
//
// J1 k_pj_grid     as above, once per KeyFrame of the batch (not per pair)
// J2 k_s3_points   grid (features, pairs, 2 directions), kSub lanes per feature of the searching
//                  KeyFrame: its MapPoint goes to its own camera, through the relative Sim3 to the
//                  other camera, and scans that KeyFrame's window like the Fuse modes (first
//                  minimum, no claims): vnMatch1 / vnMatch2
// J3 k_s3_agree    one lane per i1: vnMatch2[vnMatch1[i1]] == i1 (:1375-1391)
// =====================================================================================

// the second camera of one direction: p3Dc_other = M * p3Dc_own + t (:1186-1189)
struct S3Rel {
    float M[9], t[3];
};

// sim3 = s12, R12 (row-major), t12.  dir 0 (KF1 searches KF2): sR21 = (1.0/s12)*R12.t(), t21 = -sR21*t12;
// dir 1: sR12 = s12*R12, t12.  MatExpr scales are convertTo with a float alpha (as ps_camera's Scw split).
__device__ __forceinline__ S3Rel s3_relative(int dir, const float* __restrict__ sim3)
{
    S3Rel c;
    const float s12 = sim3[0];
    const float* R12 = sim3 + 1;
    const float* t12 = sim3 + 10;
    if (dir) {
        for (int r = 0; r < 3; ++r) {
            for (int k = 0; k < 3; ++k) c.M[3 * r + k] = R12[3 * r + k] * s12 + 0.0f;
            c.t[r] = t12[r];
        }
    } else {
        const float s = (float)(1.0 / (double)s12);
        for (int r = 0; r < 3; ++r) {
            for (int k = 0; k < 3; ++k) c.M[3 * r + k] = R12[3 * k + r] * s + 0.0f;
            c.t[r] = -ps_row(c.M + 3 * r, 1, t12[0], t12[1], t12[2]);
        }
    }
    return c;
}

// :1226-1257 / :1306-1337; false where the reference `continue`s.  Unlike ps_project the distance
// test is on cv::norm of the camera-frame point, and there is no viewing-angle test.
__device__ __forceinline__ bool s3_project(const float* __restrict__ Tsw, const S3Rel& c, const orbm_map_point& M,
                                           const orbm_pose_params& P, ProjWindow& w)
{
    const float a0 = ps_row(Tsw, 1, M.x, M.y, M.z) + Tsw[3];
    const float a1 = ps_row(Tsw + 4, 1, M.x, M.y, M.z) + Tsw[7];
    const float a2 = ps_row(Tsw + 8, 1, M.x, M.y, M.z) + Tsw[11];
    const float xc = ps_row(c.M, 1, a0, a1, a2) + c.t[0];
    const float yc = ps_row(c.M + 3, 1, a0, a1, a2) + c.t[1];
    const float zc = ps_row(c.M + 6, 1, a0, a1, a2) + c.t[2];
    if (zc < 0.0f) return false;
    const float invz = (float)(1.0 / (double)zc);
    const float x = xc * invz, y = yc * invz;
    const float u = __builtin_fmaf(P.fx, x, P.cx);
    const float v = __builtin_fmaf(P.fy, y, P.cy);
    if (!(u >= P.min_x && u < P.max_x && v >= P.min_y && v < P.max_y)) return false;   // IsInImage
    const float maxD = 1.2f * M.max_dist, minD = 0.8f * M.min_dist;
    double s = 0.0;
    s += (double)xc * (double)xc;
    s += (double)yc * (double)yc;
    s += (double)zc * (double)zc;
    const float dist = (float)__builtin_sqrt(s);   // cv::norm(p3Dc2)
    if (dist < minD || dist > maxD) return false;
    const int L = ps_predict_scale(M.max_dist, dist, P);
    w.u = u;
    w.v = v;
    w.ur = 0.0f;
    w.r = P.th * P.scale[L & 15];
    w.minLevel = L - 1;
    w.maxLevel = L;
    return true;
}

// the window search of one direction, as the Fuse overloads: no claims, no extra test, the first minimum
struct Sim3Search {
    using Params = orbm_pose_params;
    using ToInt = X86Int;
    static constexpr int kExtra = kNoExtra;
    static constexpr bool kClaims = false;
};

__global__ __launch_bounds__(256) void k_s3_points(const orbx_keypoint* __restrict__ kps,
                                                   const uint8_t* __restrict__ desc,
                                                   const orbm_map_point* __restrict__ mps,
                                                   const uint8_t* __restrict__ mpdesc, const int* __restrict__ counts,
                                                   int nkf, int cap, const float* __restrict__ pose,
                                                   const int* __restrict__ pair_a, const int* __restrict__ pair_b,
                                                   const float* __restrict__ sim3,
                                                   const uint8_t* __restrict__ already1,
                                                   const uint8_t* __restrict__ already2, orbm_pose_params P,
                                                   const uint32_t* __restrict__ gkeys, int* __restrict__ match1,
                                                   int* __restrict__ match2)
{
    const int p = blockIdx.y, dir = blockIdx.z;
    const int m = blockIdx.x * (256 / kSub) + threadIdx.x / kSub, sub = threadIdx.x % kSub;
    if (m >= cap) return;   // uniform over the kSub lanes of a feature, like every branch up to the reduction
    const size_t po = (size_t)p * cap + m;
    const int fa = pair_a[p], fb = pair_b[p];
    const int fs = dir ? fb : fa, ft = dir ? fa : fb;   // the searching KeyFrame and the one searched
    unsigned long long best = ~0ull;                    // first minimum as (dist, position, index)
    const bool pair_ok = (unsigned)fa < (unsigned)nkf && (unsigned)fb < (unsigned)nkf && sim3[(size_t)p * 13] > 0.0f;
    if (pair_ok && m < min(counts[fs], cap) && !(dir ? already2[po] : already1[po])) {
        const size_t so = (size_t)fs * cap + m;
        const orbm_map_point M = mps[so];
        if (M.flags & 1) {
            const S3Rel c = s3_relative(dir, sim3 + (size_t)p * 13);
            const size_t to = (size_t)ft * cap;
            const FrameView F{gkeys + (size_t)ft * pj_grid_stride(cap), kps + to, nullptr, nullptr, desc + to * 32, cap};
            ProjWindow w;
            if (s3_project(pose + (size_t)fs * 12, c, M, P, w) && proj_window<Sim3Search::ToInt>(w, P, F.keys, cap)) {
                const uint4* qd = reinterpret_cast<const uint4*>(mpdesc + so * 32);
                const uint4 q0 = qd[0], q1 = qd[1];
                walk_window<Sim3Search>(w, F, sub, q0, q1, P, [&](int q, int idx, int dist) {
                    const unsigned long long key = first_key(dist, q, idx);
                    best = key < best ? key : best;
                });
            }
        }
    }
    best = sub_min_u64(best);
    if (sub != 0) return;
    const int r = (best != ~0ull && (int)(best >> 32) <= 100) ? (int)(best & 0xFFFF) : -1;   // TH_HIGH
    if (dir) match2[po] = r;
    else match1[po] = r;
}

__global__ __launch_bounds__(256) void k_s3_agree(const int* __restrict__ match1, const int* __restrict__ match2,
                                                  int cap, int* __restrict__ match12, int* __restrict__ nfound)
{
    const int p = blockIdx.y, i1 = blockIdx.x * 256 + threadIdx.x;
    int r = -1;
    if (i1 < cap) {
        const int idx2 = match1[(size_t)p * cap + i1];   // a key's index: < cap
        if (idx2 >= 0 && match2[(size_t)p * cap + idx2] == i1) r = idx2;
        match12[(size_t)p * cap + i1] = r;
    }
    const int n = __popcll(__ballot(r >= 0));
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(&nfound[p], n);
}

static size_t sim3_scratch_bytes(int nkf, int npairs, int cap)
{
    return GridScratch(nullptr, nkf, cap, (size_t)2 * npairs * cap * 4).bytes;
}

static void launch_search_by_sim3(const orbx_keypoint* kps, const uint8_t* desc, const orbm_map_point* mps,
                                  const uint8_t* mpdesc, const int* counts, int nkf, int cap, const float* pose,
                                  const int* pair_a, const int* pair_b, const float* sim3, const uint8_t* already1,
                                  const uint8_t* already2, int npairs, const orbm_pose_params& P, void* scratch,
                                  int* match12, int* nfound, int* match1, int* match2, hipStream_t s)
{
    const GridScratch sc(scratch, nkf, cap, 0);
    int* tmp = (int*)sc.tail;
    if (!match1) match1 = tmp;
    if (!match2) match2 = tmp + (size_t)npairs * cap;
    launch_pj_grid(kps, counts, nkf, cap, P, sc.gkeys, s);
    hipMemsetAsync(nfound, 0, sizeof(int) * (size_t)npairs, s);
    hipLaunchKernelGGL(k_s3_points, dim3((cap + 256 / kSub - 1) / (256 / kSub), npairs, 2), dim3(256), 0, s, kps, desc,
                       mps, mpdesc, counts, nkf, cap, pose, pair_a, pair_b, sim3, already1, already2, P, sc.gkeys,
                       match1, match2);
    hipLaunchKernelGGL(k_s3_agree, dim3((cap + 255) / 256, npairs), dim3(256), 0, s, match1, match2, cap, match12,
                       nfound);
}

}  // namespace orbx

using namespace orbx;

extern "C" {

orbx_status orbm_search_by_projection_device(const orbx_keypoint* d_kps, const uint8_t* d_desc, const float* d_uright,
                                             const uint8_t* d_claimed, const int* d_counts, int nframes, int cap,
                                             const orbm_proj_point* d_pts, const uint8_t* d_pdesc, const int* d_npts,
                                             int pcap, const orbm_proj_params* params, int* d_match,
                                             int* d_nmatches, void* stream)
{
    if (!d_kps || !d_desc || !d_uright || !d_claimed || !d_counts || nframes < 0 || cap <= 0 || cap > ORBM_MAX_FEATURES ||
        !d_pts || !d_pdesc || !d_npts || pcap <= 0 || !params || !d_match || !d_nmatches)
        return ORBX_EINVAL;
    if (nframes == 0) return ORBX_OK;
    hipStream_t s = (hipStream_t)stream;
    return with_scratch(proj_scratch_bytes(nframes, cap, pcap), s, [&](void* scratch) {
        launch_proj(d_kps, d_desc, d_uright, d_claimed, d_counts, nframes, cap, d_pts, d_pdesc, d_npts, pcap, *params,
                    scratch, d_match, d_nmatches, s);
    });
}

orbx_status orbm_search_by_projection(int device, const orbx_keypoint* kps, const uint8_t* desc, const float* uright,
                                      const uint8_t* claimed, int n, const orbm_proj_point* pts, const uint8_t* pdesc,
                                      int np, const orbm_proj_params* params, int* match, int* nmatches)
{
    if (n < 0 || n > ORBM_MAX_FEATURES || np < 0 || !params || !nmatches) return ORBX_EINVAL;
    *nmatches = 0;
    if (n == 0) return ORBX_OK;
    if (!kps || !desc || !uright || !claimed || !match || (np > 0 && (!pts || !pdesc))) return ORBX_EINVAL;
    for (int i = 0; i < np; ++i)
        if ((pts[i].flags & 1) && (pts[i].level < 0 || pts[i].level >= 16)) return ORBX_EINVAL;
    for (int i = 0; i < n; ++i) match[i] = -1;
    if (np == 0) return ORBX_OK;
    HostCall c(device);
    const int cn[2] = {n, np};
    const auto ocn = c.in(cn, 2);
    const auto ok = c.in(kps, (size_t)n);
    const auto od = c.in(desc, (size_t)32 * n);
    const auto ou = c.in(uright, (size_t)n);
    const auto oc = c.in(claimed, (size_t)n);
    const auto op = c.in(pts, (size_t)np);
    const auto opd = c.in(pdesc, (size_t)32 * np);
    const auto om = c.out<int>((size_t)n + 1);   // nmatches, match
    orbx_status rc = c.begin();
    if (rc != ORBX_OK) return rc;
    rc = orbm_search_by_projection_device(c.dev(ok), c.dev(od), c.dev(ou), c.dev(oc), c.dev(ocn), 1, n, c.dev(op),
                                          c.dev(opd), c.dev(ocn, 1), np, params, c.dev(om, 1), c.dev(om), c.stream());
    if (rc != ORBX_OK) return rc;
    c.fetch(om, match, (size_t)n, 1);
    c.fetch(om, nmatches, 1);
    return c.finish();
}

orbx_status orbm_project_search_device(int mode, const orbx_keypoint* d_kps, const uint8_t* d_desc,
                                       const float* d_uright, const uint8_t* d_claimed, const int* d_counts,
                                       int nframes, int cap, const float* d_pose, const orbm_map_point* d_pts,
                                       const uint8_t* d_pdesc, const int* d_npts, int pcap,
                                       const orbm_pose_params* params, int* d_match, int* d_nmatches, void* stream)
{
    if (mode < ORBM_PROJ_LAST_FRAME || mode > ORBM_FUSE_SIM3 || !d_kps || !d_desc || !d_uright || !d_claimed ||
        !d_counts || nframes < 0 || cap <= 0 || cap > ORBM_MAX_FEATURES || !d_pose || !d_pts || !d_pdesc || !d_npts ||
        pcap <= 0 || !params || !d_match || !d_nmatches || params->nlevels < 1 || params->nlevels > 16)
        return ORBX_EINVAL;
    if (nframes == 0) return ORBX_OK;
    hipStream_t s = (hipStream_t)stream;
    return with_scratch(proj_scratch_bytes(nframes, cap, pcap), s, [&](void* scratch) {
        launch_pose_search(mode, d_kps, d_desc, d_uright, d_claimed, d_counts, nframes, cap, d_pose, d_pts, d_pdesc,
                           d_npts, pcap, *params, scratch, d_match, d_nmatches, s);
    });
}

orbx_status orbm_project_search(int device, int mode, const orbx_keypoint* kps, const uint8_t* desc,
                                const float* uright, const uint8_t* claimed, int n, const float* pose,
                                const orbm_map_point* pts, const uint8_t* pdesc, int np,
                                const orbm_pose_params* params, int* match, int* nmatches)
{
    if (mode < ORBM_PROJ_LAST_FRAME || mode > ORBM_FUSE_SIM3 || n < 0 || n > ORBM_MAX_FEATURES || np < 0 || !params ||
        !nmatches || !pose || params->nlevels < 1 || params->nlevels > 16)
        return ORBX_EINVAL;
    const bool search = mode <= ORBM_PROJ_SIM3;
    const int nout = search ? n : np;
    *nmatches = 0;
    if (nout > 0 && !match) return ORBX_EINVAL;
    if ((n > 0 && (!kps || !desc || !uright || (search && !claimed))) || (np > 0 && (!pts || !pdesc)))
        return ORBX_EINVAL;
    for (int i = 0; i < n; ++i)
        if (kps[i].octave < 0 || kps[i].octave >= 16) return ORBX_EINVAL;
    if (mode == ORBM_PROJ_LAST_FRAME)
        for (int i = 0; i < np; ++i)
            if ((pts[i].flags & 1) && (pts[i].octave < 0 || pts[i].octave >= 16)) return ORBX_EINVAL;
    for (int i = 0; i < nout; ++i) match[i] = -1;
    if (n == 0 || np == 0) return ORBX_OK;
    HostCall c(device);
    const int cn[2] = {n, np};
    const auto ocn = c.in(cn, 2);
    const auto opo = c.in(pose, 24);
    const auto ok = c.in(kps, (size_t)n);
    const auto od = c.in(desc, (size_t)32 * n);
    const auto ou = c.in(uright, (size_t)n);
    const auto oc = c.in(search ? claimed : nullptr, (size_t)n);
    const auto op = c.in(pts, (size_t)np);
    const auto opd = c.in(pdesc, (size_t)32 * np);
    const auto om = c.out<int>((size_t)nout + 1);   // nmatches, match
    orbx_status rc = c.begin();
    if (rc != ORBX_OK) return rc;
    rc = orbm_project_search_device(mode, c.dev(ok), c.dev(od), c.dev(ou), c.dev(oc), c.dev(ocn), 1, n, c.dev(opo),
                                    c.dev(op), c.dev(opd), c.dev(ocn, 1), np, params, c.dev(om, 1), c.dev(om),
                                    c.stream());
    if (rc != ORBX_OK) return rc;
    c.fetch(om, match, (size_t)nout, 1);
    c.fetch(om, nmatches, 1);
    return c.finish();
}

orbx_status orbm_search_by_sim3_device(const orbx_keypoint* d_kps, const uint8_t* d_desc, const orbm_map_point* d_mps,
                                       const uint8_t* d_mpdesc, const int* d_counts, int nkf, int cap,
                                       const float* d_pose, const int* d_pair_a, const int* d_pair_b,
                                       const float* d_sim3, const uint8_t* d_already1, const uint8_t* d_already2,
                                       int npairs, const orbm_pose_params* params, int* d_match12, int* d_nfound,
                                       int* d_match1, int* d_match2, void* stream)
{
    if (nkf < 0 || npairs < 0 || npairs > 65535 || cap <= 0 || cap > ORBM_MAX_FEATURES || !params ||
        params->nlevels < 1 || params->nlevels > 16)
        return ORBX_EINVAL;
    if (npairs == 0) return ORBX_OK;
    if (nkf == 0 || !d_kps || !d_desc || !d_mps || !d_mpdesc || !d_counts || !d_pose || !d_pair_a || !d_pair_b ||
        !d_sim3 || !d_already1 || !d_already2 || !d_match12 || !d_nfound)
        return ORBX_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    return with_scratch(sim3_scratch_bytes(nkf, npairs, cap), s, [&](void* scratch) {
        launch_search_by_sim3(d_kps, d_desc, d_mps, d_mpdesc, d_counts, nkf, cap, d_pose, d_pair_a, d_pair_b, d_sim3,
                              d_already1, d_already2, npairs, *params, scratch, d_match12, d_nfound, d_match1,
                              d_match2, s);
    });
}

orbx_status orbm_search_by_sim3(int device, const orbx_keypoint* kps1, const uint8_t* desc1,
                                const orbm_map_point* mps1, const uint8_t* mpdesc1, const uint8_t* already1, int n1,
                                const float* T1w, const orbx_keypoint* kps2, const uint8_t* desc2,
                                const orbm_map_point* mps2, const uint8_t* mpdesc2, const uint8_t* already2, int n2,
                                const float* T2w, float s12, const float* R12, const float* t12,
                                const orbm_pose_params* params, int* match12, int* nfound, int* match1, int* match2)
{
    if (n1 < 0 || n1 > ORBM_MAX_FEATURES || n2 < 0 || n2 > ORBM_MAX_FEATURES || !params || !nfound || !T1w || !T2w ||
        !R12 || !t12 || !(s12 > 0.0f) || params->nlevels < 1 || params->nlevels > 16)
        return ORBX_EINVAL;
    *nfound = 0;
    if ((n1 > 0 && (!kps1 || !desc1 || !mps1 || !mpdesc1 || !already1 || !match12)) ||
        (n2 > 0 && (!kps2 || !desc2 || !mps2 || !mpdesc2 || !already2)))
        return ORBX_EINVAL;
    for (int i = 0; i < n1; ++i)
        if (kps1[i].octave < 0 || kps1[i].octave >= 16) return ORBX_EINVAL;
    for (int i = 0; i < n2; ++i)
        if (kps2[i].octave < 0 || kps2[i].octave >= 16) return ORBX_EINVAL;
    for (int i = 0; i < n1; ++i) match12[i] = -1;
    if (match1)
        for (int i = 0; i < n1; ++i) match1[i] = -1;
    if (match2)
        for (int i = 0; i < n2; ++i) match2[i] = -1;
    if (n1 == 0 || n2 == 0) return ORBX_OK;
    // the two KeyFrames as a batch of two at stride cap
    const int cap = std::max(n1, n2);
    const size_t c = (size_t)cap;
    const int head[4] = {n1, n2, 0, 1};   // d_counts[2], d_pair_a[1], d_pair_b[1]
    float geo[24 + 13];                    // d_pose[2 * 12], d_sim3[13]
    std::memcpy(geo, T1w, sizeof(float) * 12);
    std::memcpy(geo + 12, T2w, sizeof(float) * 12);
    geo[24] = s12;
    std::memcpy(geo + 25, R12, sizeof(float) * 9);
    std::memcpy(geo + 34, t12, sizeof(float) * 3);
    HostCall hc(device);
    const auto oh = hc.in(head, 4);
    const auto og = hc.in(geo, 24 + 13);
    const auto ok = hc.stage<orbx_keypoint>(2 * c);
    const auto od = hc.stage<uint8_t>(32 * 2 * c);
    const auto om = hc.stage<orbm_map_point>(2 * c);
    const auto omd = hc.stage<uint8_t>(32 * 2 * c);
    const auto oa = hc.stage<uint8_t>(2 * c);    // already1[cap], already2[cap]
    const auto oo = hc.out<int>(3 * c + 1);      // nfound, match12, match1, match2
    orbx_status rc = hc.prepare();
    if (rc != ORBX_OK) return rc;
    const size_t m1 = (size_t)n1, m2 = (size_t)n2;
    pack_pair(hc.host(ok), c, kps1, m1, kps2, m2);
    pack_pair(hc.host(od), 32 * c, desc1, 32 * m1, desc2, 32 * m2);
    pack_pair(hc.host(om), c, mps1, m1, mps2, m2);
    pack_pair(hc.host(omd), 32 * c, mpdesc1, 32 * m1, mpdesc2, 32 * m2);
    pack_pair(hc.host(oa), c, already1, m1, already2, m2);
    if ((rc = hc.upload()) != ORBX_OK) return rc;
    rc = orbm_search_by_sim3_device(hc.dev(ok), hc.dev(od), hc.dev(om), hc.dev(omd), hc.dev(oh), 2, cap, hc.dev(og),
                                    hc.dev(oh, 2), hc.dev(oh, 3), hc.dev(og, 24), hc.dev(oa), hc.dev(oa, c), 1, params,
                                    hc.dev(oo, 1), hc.dev(oo), hc.dev(oo, 1 + c), hc.dev(oo, 1 + 2 * c), hc.stream());
    if (rc != ORBX_OK) return rc;
    hc.fetch(oo, nfound, 1);
    hc.fetch(oo, match12, m1, 1);
    hc.fetch(oo, match1, m1, 1 + c);
    hc.fetch(oo, match2, m2, 1 + 2 * c);
    return hc.finish();
}

}  // extern "C"

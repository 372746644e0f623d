// Initializer (src/Initializer.cc, include/Initializer.h): Initialize (:45-159) and everything it calls, as
// Tracking::MonocularInitialization drives it right after SearchForInitialization, batched over frame pairs.
// Kernels and C entry points (include/orbx.h).  The arithmetic order of everything below is DESIGN.md §3
// "Initializer arithmetic": cv::SVDecomp on CV_32F as OpenCV 3.x's JacobiSVDImpl_<float> with its basis-completion
// loop, Mat::inv / cv::determinant of a 3x3 in double, CV_32F products as the small-matrix gemm, the scalar float
// statements with the FMAs a contracting compiler forms written out, acos from orbx_math.hpp.  Parity with a real
// OpenCV is unpinned; the Python restatement of tests/test_initializer.py, this code compiled for the CPU
// (orbm_initialize_host) and the gfx950 code agree bit for bit.
//
// k_init_setup:  one workgroup of 256 lanes per pair.  Validates (every index in front of the read it guards),
//   compacts vMatches12 into mvMatches12 in ascending i (ballot prefix), Normalize of both key sets (the four float
//   sums per frame are sequential by definition: one lane each), T2.inv(), T2.t(), and the 8-point sets of every
//   iteration (RandomInt and the swap-with-back removal as at most 8 overrides).
// k_init_hyp:    one lane per (iteration, H or F, pair), 64 iterations of one model to a wave.  The lane runs the
//   8-point solve (the Jacobi SVD works on private arrays: runtime-indexed, so in scratch, 1 KB a lane) and then
//   CheckHomography / CheckFundamental over the N matches, where the score is the reference's own in-order float
//   sum and the inlier mask is built a 64-bit word at a time.  The lanes of a wave read the same match at the same
//   time.  (One wave per hypothesis with lane 0 solving was measured first: 353 ms per 4,096 pairs, all of it in the
//   one-lane solve; DESIGN.md §5 Initializer.)
// k_init_select: one workgroup per pair.  Lane 0 walks the H and then the F scores in iteration order (strict >
//   from 0), computes RH and picks the model; the lanes expand the two masks.
// k_init_cand:   one wave64 per (candidate, pair): 4 of DecomposeE or 8 of Faugeras' decomposition, then CheckRT
//   with the lanes striding over the matches; the parallax entry by rank selection.
// k_init_finish: one workgroup per pair.  Lane 0 applies ReconstructF's / ReconstructH's decision, the lanes copy the
//   winner out and prune the matches.
// The device call allocates nothing; everything between the kernels lives in the caller's workspace.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstring>
#include <vector>

#include "orbx_host.hpp"
#include "orbx_math.hpp"

namespace orbx {

constexpr int kInLanes = 256;
constexpr int kInMaxIters = 4096;   // the planner's limit on max_iterations
constexpr int kInMaxPairs = 65535;  // a grid dimension
constexpr int kInHdrInts = 16;
constexpr int kInFloats = 64;
constexpr int kInHypFloats = 16;    // the model's 9 floats, the score, 6 unused
constexpr int kInCandFloats = 16;   // R[9], t[3], nGood (int), parallax, singular (int), 1 unused

enum { kInN = 0, kInValid = 1, kInN1 = 2, kInN2 = 3, kInPickH = 4, kInPickF = 5, kInModel = 6, kInStatus = 7 };
enum { kInT1 = 0, kInT2inv = 9, kInT2t = 18, kInH = 27, kInF = 36, kInMean = 45 };   // kInMean: mx1 my1 sx1 sy1 mx2 ..

struct InLayout {
    size_t pair_bytes, m_off, sets_off, hyp_off, hyp_bytes, cand_off, cand_bytes, total;
    int words;
};

__host__ __device__ inline InLayout in_layout(int npairs, int cap, int iters)
{
    InLayout L;
    L.words = (cap + 63) / 64;
    L.m_off = (size_t)4 * (kInHdrInts + kInFloats);
    L.sets_off = L.m_off + (size_t)8 * cap;
    L.hyp_off = L.sets_off + (size_t)32 * iters;
    L.hyp_bytes = (size_t)4 * kInHypFloats + (size_t)8 * L.words;
    L.cand_off = L.hyp_off + L.hyp_bytes * 2 * (size_t)iters;
    L.cand_bytes = (size_t)4 * kInCandFloats + (size_t)16 * cap + (((size_t)cap + 3) & ~(size_t)3);
    L.pair_bytes = (L.cand_off + 8 * L.cand_bytes + 15) & ~(size_t)15;
    L.total = L.pair_bytes * (size_t)npairs;
    return L;
}

struct InPair {
    int* hdr;
    float* fl;
    int *m1, *m2, *sets;
    uint8_t* hyps;
    uint8_t* cands;
};

ORBX_HD InPair in_pair(void* work, const InLayout& L, int p, int cap)
{
    uint8_t* b = (uint8_t*)work + L.pair_bytes * (size_t)p;
    InPair W;
    W.hdr = (int*)b;
    W.fl = (float*)(W.hdr + kInHdrInts);
    W.m1 = (int*)(b + L.m_off);
    W.m2 = W.m1 + cap;
    W.sets = (int*)(b + L.sets_off);
    W.hyps = b + L.hyp_off;
    W.cands = b + L.cand_off;
    return W;
}

struct InHyp {
    float* M;
    float* score;
    unsigned long long* words;
};

ORBX_HD InHyp in_hyp(const InPair& W, const InLayout& L, int which, int it, int iters)
{
    uint8_t* b = W.hyps + L.hyp_bytes * ((size_t)which * iters + it);
    InHyp H;
    H.M = (float*)b;
    H.score = H.M + 9;
    H.words = (unsigned long long*)(H.M + kInHypFloats);
    return H;
}

struct InCand {
    float *R, *t;
    int* ngood;
    float* parallax;
    int* singular;
    float *p3d, *cosp;
    uint8_t* flags;   // per match: bit 0 = vP3D written and its cosine pushed, bit 1 = vbGood
};

ORBX_HD InCand in_cand(const InPair& W, const InLayout& L, int c, int cap)
{
    uint8_t* b = W.cands + L.cand_bytes * (size_t)c;
    InCand C;
    C.R = (float*)b;
    C.t = C.R + 9;
    C.ngood = (int*)(C.R + 12);
    C.parallax = C.R + 13;
    C.singular = (int*)(C.R + 14);
    C.p3d = C.R + kInCandFloats;
    C.cosp = C.p3d + (size_t)3 * cap;
    C.flags = (uint8_t*)(C.cosp + cap);
    return C;
}

// ---- lanes ----
ORBX_HD int in_tid()
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (int)threadIdx.x;
#else
    return 0;
#endif
}

ORBX_HD void in_sync()
{
#if defined(__HIP_DEVICE_COMPILE__)
    __syncthreads();
#endif
}

// lane 0's value in every lane of the wave
ORBX_HD float in_bcast(float v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __shfl(v, 0);
#else
    return v;
#endif
}

template <int NT>
struct InShared {
    int wave_n[NT / 64 + 1];
    int bad, win, ok;
    float sum[8];
};

// rank of this lane among the chunk's lanes with `flag` set, in lane order, and their number
template <int NT>
ORBX_HD int in_rank(InShared<NT>& S, bool flag, int* total)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const unsigned long long b = __ballot(flag);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) S.wave_n[wave] = __popcll(b);
    __syncthreads();
    int base = 0, tot = 0;
    for (int w = 0; w < NT / 64; ++w) {
        const int c = S.wave_n[w];
        if (w < wave) base += c;
        tot += c;
    }
    *total = tot;
    return base + __popcll(b & ((1ull << lane) - 1ull));
#else
    *total = flag ? 1 : 0;
    return 0;
#endif
}

// ---- small cv::Mat arithmetic ----
// C = A * B for 3x3 CV_32F: the small-matrix gemm, (a0 b0 + a1 b1) + a2 b2 in float
ORBX_HD void in_mul33(const float* A, const float* B, float* C)
{
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            C[3 * i + j] = (A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j]) + A[3 * i + 2] * B[6 + j];
}

ORBX_HD void in_t33(const float* A, float* At)
{
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) At[3 * i + j] = A[3 * j + i];
}

// cv::determinant of a 3x3 CV_32F: the cofactor expansion in double
ORBX_HD double in_det33(const float* m)
{
    const double m00 = m[0], m01 = m[1], m02 = m[2], m10 = m[3], m11 = m[4], m12 = m[5], m20 = m[6], m21 = m[7],
                 m22 = m[8];
    return (m00 * (m11 * m22 - m12 * m21) - m01 * (m10 * m22 - m12 * m20)) + m02 * (m10 * m21 - m11 * m20);
}

// cv::Mat::inv() of a 3x3 CV_32F: the cofactors times 1 / det in double, each rounded once; det == 0 gives zeros
ORBX_HD void in_inv33(const float* m, float* o)
{
    double d = in_det33(m);
    if (d == 0.0) {
        for (int i = 0; i < 9; ++i) o[i] = 0.0f;
        return;
    }
    d = 1.0 / d;
    const double s00 = m[0], s01 = m[1], s02 = m[2], s10 = m[3], s11 = m[4], s12 = m[5], s20 = m[6], s21 = m[7],
                 s22 = m[8];
    o[0] = (float)((s11 * s22 - s12 * s21) * d);
    o[1] = (float)((s02 * s21 - s01 * s22) * d);
    o[2] = (float)((s01 * s12 - s02 * s11) * d);
    o[3] = (float)((s12 * s20 - s10 * s22) * d);
    o[4] = (float)((s00 * s22 - s02 * s20) * d);
    o[5] = (float)((s02 * s10 - s00 * s12) * d);
    o[6] = (float)((s10 * s21 - s11 * s20) * d);
    o[7] = (float)((s01 * s20 - s00 * s21) * d);
    o[8] = (float)((s00 * s11 - s01 * s10) * d);
}

// ---- cv::SVDecomp on CV_32F: JacobiSVDImpl_<float> ----
// At: n1 rows of m floats (row stride m), the first n of them the Jacobi rows, the others zero on entry; Vt: n x n;
// W: n doubles.  On return the rows are sorted to descending W; with `complete` the rows of At are normalised and the
// rows of zero singular value (and the rows n .. n1-1) are filled from RNG(0x12345678) and orthogonalised.
ORBX_HD void in_svd(float* At, int m, int n, int n1, float* Vt, double* W, bool complete)
{
    const float epsf = 1.1920928955078125e-07f * 2.0f;   // FLT_EPSILON*2
    const double eps = (double)epsf;
    for (int i = 0; i < n; ++i) {
        double sd = 0.0;
        for (int k = 0; k < m; ++k) sd += (double)At[i * m + k] * (double)At[i * m + k];
        W[i] = sd;
        for (int k = 0; k < n; ++k) Vt[i * n + k] = i == k ? 1.0f : 0.0f;
    }
    const int max_iter = m > 30 ? m : 30;
    for (int iter = 0; iter < max_iter; ++iter) {
        bool changed = false;
        for (int i = 0; i < n - 1; ++i)
            for (int j = i + 1; j < n; ++j) {
                float* Ai = At + i * m;
                float* Aj = At + j * m;
                double a = W[i], b = W[j], p = 0.0;
                for (int k = 0; k < m; ++k) p += (double)Ai[k] * (double)Aj[k];
                if (__builtin_fabs(p) <= eps * __builtin_sqrt(a * b)) continue;
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
                for (int k = 0; k < m; ++k) {
                    const float t0 = c * Ai[k] + s * Aj[k];
                    const float t1 = -s * Ai[k] + c * Aj[k];
                    Ai[k] = t0;
                    Aj[k] = t1;
                    a += (double)t0 * (double)t0;
                    b += (double)t1 * (double)t1;
                }
                W[i] = a;
                W[j] = b;
                changed = true;
                float* Vi = Vt + i * n;
                float* Vj = Vt + j * n;
                for (int k = 0; k < n; ++k) {
                    const float t0 = c * Vi[k] + s * Vj[k];
                    const float t1 = -s * Vi[k] + c * Vj[k];
                    Vi[k] = t0;
                    Vj[k] = t1;
                }
            }
        if (!changed) break;
    }
    for (int i = 0; i < n; ++i) {
        double sd = 0.0;
        for (int k = 0; k < m; ++k) sd += (double)At[i * m + k] * (double)At[i * m + k];
        W[i] = __builtin_sqrt(sd);
    }
    for (int i = 0; i < n - 1; ++i) {
        int j = i;
        for (int k = i + 1; k < n; ++k)
            if (W[j] < W[k]) j = k;
        if (i != j) {
            const double w = W[i];
            W[i] = W[j];
            W[j] = w;
            for (int k = 0; k < m; ++k) {
                const float t = At[i * m + k];
                At[i * m + k] = At[j * m + k];
                At[j * m + k] = t;
            }
            for (int k = 0; k < n; ++k) {
                const float t = Vt[i * n + k];
                Vt[i * n + k] = Vt[j * n + k];
                Vt[j * n + k] = t;
            }
        }
    }
    if (!complete) return;
    unsigned long long rng = 0x12345678ull;
    const double minval = (double)FLT_MIN;
    for (int i = 0; i < n1; ++i) {
        float* Ai = At + i * m;
        double sd = i < n ? W[i] : 0.0;
        for (int ii = 0; ii < 100 && sd <= minval; ++ii) {
            const float val0 = (float)(1.0 / (double)m);
            for (int k = 0; k < m; ++k) {
                rng = (unsigned long long)(unsigned)rng * 4164903690ull + (rng >> 32);
                Ai[k] = ((unsigned)rng & 256u) != 0u ? val0 : -val0;
            }
            for (int iter = 0; iter < 2; ++iter)
                for (int j = 0; j < i; ++j) {
                    const float* Aj = At + j * m;
                    sd = 0.0;
                    for (int k = 0; k < m; ++k) sd += (double)(Ai[k] * Aj[k]);
                    float asum = 0.0f;
                    for (int k = 0; k < m; ++k) {
                        const float t = (float)((double)Ai[k] - sd * (double)Aj[k]);
                        Ai[k] = t;
                        asum += __builtin_fabsf(t);
                    }
                    asum = asum > epsf * 100.0f ? 1.0f / asum : 0.0f;
                    for (int k = 0; k < m; ++k) Ai[k] *= asum;
                }
            sd = 0.0;
            for (int k = 0; k < m; ++k) sd += (double)Ai[k] * (double)Ai[k];
            sd = __builtin_sqrt(sd);
        }
        const float s = (float)(sd > minval ? 1.0 / sd : 0.0);
        for (int k = 0; k < m; ++k) Ai[k] *= s;
    }
}

// cv::SVD::compute of a 3x3 CV_32F: w (floats, descending), u and vt row-major
ORBX_HD void in_svd33(const float* A, float* w, float* u, float* vt)
{
    float At[9];
    double W[3];
    in_t33(A, At);
    in_svd(At, 3, 3, 3, vt, W, true);
    in_t33(At, u);
    for (int i = 0; i < 3; ++i) w[i] = (float)W[i];
}

// ---- Normalize (:1047-1103) of one frame's keys: {meanX, meanY, sX, sY}; the sums by one lane each ----
template <int NT>
ORBX_HD void in_normalize(InShared<NT>& S, const orbx_keypoint* k1, int n1, const orbx_keypoint* k2, int n2,
                          float* out8)
{
    const int tid = in_tid();
    // lanes 0..3 take one sum each; a single lane takes all four
    const int q0 = NT >= 4 ? tid : 0, q1 = NT >= 4 ? (tid < 4 ? tid + 1 : 0) : 4;
    for (int q = q0; q < q1; ++q) {
        const orbx_keypoint* k = (q & 2) ? k2 : k1;
        const int n = (q & 2) ? n2 : n1;
        float s = 0.0f;
        if (q & 1)
            for (int i = 0; i < n; ++i) s += k[i].y;
        else
            for (int i = 0; i < n; ++i) s += k[i].x;
        S.sum[q] = s / (float)n;
    }
    in_sync();
    for (int q = q0; q < q1; ++q) {
        {
            const orbx_keypoint* k = (q & 2) ? k2 : k1;
            const int n = (q & 2) ? n2 : n1;
            const float mean = S.sum[q];
            float s = 0.0f;
            if (q & 1)
                for (int i = 0; i < n; ++i) s += __builtin_fabsf(k[i].y - mean);
            else
                for (int i = 0; i < n; ++i) s += __builtin_fabsf(k[i].x - mean);
            s = s / (float)n;
            S.sum[4 + q] = (float)(1.0 / (double)s);
        }
    }
    in_sync();
    if (tid == 0) {
        out8[0] = S.sum[0];
        out8[1] = S.sum[1];
        out8[2] = S.sum[4];
        out8[3] = S.sum[5];
        out8[4] = S.sum[2];
        out8[5] = S.sum[3];
        out8[6] = S.sum[6];
        out8[7] = S.sum[7];
    }
}

// the 8 indices of one iteration (:96-120): RandomInt(0, size - 1) and the swap-with-back removal on
// vAvailableIndices = 0 .. n-1 without the list: the removals are at most 8 (position, value) overrides, the newest
// first
ORBX_HD void in_set(int n, const int* r, int* out)
{
    int pos[8], val[8];
    for (int j = 0; j < 8; ++j) {
        const int size = n - j;
        const int randi = (int)(((double)(r[j] & 0x7fffffff) / 2147483648.0) * (double)size);
        int idx = randi, back = size - 1;
        bool fi = false, fb = false;
        for (int q = j - 1; q >= 0; --q) {
            if (!fi && pos[q] == randi) {
                idx = val[q];
                fi = true;
            }
            if (!fb && pos[q] == size - 1) {
                back = val[q];
                fb = true;
            }
        }
        out[j] = idx;
        pos[j] = randi;
        val[j] = back;
    }
}

struct InTables {
    const orbx_keypoint* kps;
    const int* counts;
    int nframes, cap;
    float fx, fy, cx, cy;
};

// ---- setup ----
template <int NT>
ORBX_HD void in_setup(InShared<NT>& S, const InTables& T, int a, int b, const int* match12, const int* draws,
                      int iters, bool iters_ok, const InPair& W, int* status)
{
    const int tid = in_tid();
    bool ok = iters_ok && (unsigned)a < (unsigned)T.nframes && (unsigned)b < (unsigned)T.nframes;
    int n1 = 0, n2 = 0;
    if (ok) {
        n1 = T.counts[a];
        n2 = T.counts[b];
        ok = n1 >= 0 && n1 <= T.cap && n2 >= 0 && n2 <= T.cap;
    }
    if (tid == 0) S.bad = 0;
    in_sync();
    if (ok) {
        int bad = 0;
        for (int i = tid; i < n1; i += NT) {
            const int m = match12[i];
            if (m < -1 || m >= n2) bad = 1;
        }
        if (bad) S.bad = 1;   // every writer stores the same value
    }
    in_sync();
    ok = ok && !S.bad;
    int n = 0;
    if (ok) {
        for (int c = 0; c < n1; c += NT) {
            const int i = c + tid;
            const int m = i < n1 ? match12[i] : -1;
            int total;
            const int k = n + in_rank(S, m >= 0, &total);
            if (m >= 0) {
                W.m1[k] = i;
                W.m2[k] = m;
            }
            n += total;
            in_sync();   // wave_n is rewritten by the next chunk
        }
        ok = n >= 8;   // RandomInt(0, size - 1) of :106 is undefined below
    }
    if (!ok) {   // of an invalid pair only the status is written (and the workspace's own mark)
        if (tid == 0) {
            W.hdr[kInValid] = 0;
            W.hdr[kInStatus] = ORBM_INIT_INVALID;
            *status = ORBM_INIT_INVALID;
        }
        return;
    }
    const orbx_keypoint* k1 = T.kps + (size_t)a * T.cap;
    const orbx_keypoint* k2 = T.kps + (size_t)b * T.cap;
    in_normalize(S, k1, n1, k2, n2, W.fl + kInMean);
    if (tid == 0) {
        const float* mn = W.fl + kInMean;
        float T1[9] = {mn[2], 0.0f, -mn[0] * mn[2], 0.0f, mn[3], -mn[1] * mn[3], 0.0f, 0.0f, 1.0f};
        float T2[9] = {mn[6], 0.0f, -mn[4] * mn[6], 0.0f, mn[7], -mn[5] * mn[7], 0.0f, 0.0f, 1.0f};
        float T2inv[9], T2t[9];
        in_inv33(T2, T2inv);
        in_t33(T2, T2t);
        for (int i = 0; i < 9; ++i) {
            W.fl[kInT1 + i] = T1[i];
            W.fl[kInT2inv + i] = T2inv[i];
            W.fl[kInT2t + i] = T2t[i];
        }
        W.hdr[kInN] = n;
        W.hdr[kInValid] = 1;
        W.hdr[kInN1] = n1;
        W.hdr[kInN2] = n2;
        W.hdr[kInStatus] = 0;
    }
    for (int it = tid; it < iters; it += NT) {
        int set[8];
        in_set(n, draws + 8 * it, set);
        for (int j = 0; j < 8; ++j) W.sets[8 * it + j] = set[j];
    }
}

// ---- the 8-point solves ----
// vPn[i] of Normalize for one key
ORBX_HD void in_norm_pt(const orbx_keypoint& k, const float* mn, float* x, float* y)
{
    *x = (k.x - mn[0]) * mn[2];
    *y = (k.y - mn[1]) * mn[3];
}

// ComputeH21 (:333-383) and H21i = T2inv*Hn*T1, H12i = H21i.inv()
ORBX_HD void in_compute_h(const float* p1, const float* p2, const float* T1, const float* T2inv, float* H21,
                          float* H12)
{
    float At[9 * 16], Vt[81];
    double Wd[9];
    for (int i = 0; i < 8; ++i) {
        const float u1 = p1[2 * i], v1 = p1[2 * i + 1], u2 = p2[2 * i], v2 = p2[2 * i + 1];
        const float r0[9] = {0.0f, 0.0f, 0.0f, -u1, -v1, -1.0f, v2 * u1, v2 * v1, v2};
        const float r1[9] = {u1, v1, 1.0f, 0.0f, 0.0f, 0.0f, -u2 * u1, -u2 * v1, -u2};
        for (int c = 0; c < 9; ++c) {
            At[c * 16 + 2 * i] = r0[c];
            At[c * 16 + 2 * i + 1] = r1[c];
        }
    }
    in_svd(At, 16, 9, 9, Vt, Wd, false);
    float tmp[9];
    in_mul33(T2inv, Vt + 72, tmp);
    in_mul33(tmp, T1, H21);
    in_inv33(H21, H12);
}

// ComputeF21 (:393-437) and F21i = T2t*Fn*T1
ORBX_HD void in_compute_f(const float* p1, const float* p2, const float* T1, const float* T2t, float* F21)
{
    float At[81], Vt[64];
    double Wd[8];
    for (int i = 0; i < 8; ++i) {
        const float u1 = p1[2 * i], v1 = p1[2 * i + 1], u2 = p2[2 * i], v2 = p2[2 * i + 1];
        float* r = At + 9 * i;
        r[0] = u2 * u1;
        r[1] = u2 * v1;
        r[2] = u2;
        r[3] = v2 * u1;
        r[4] = v2 * v1;
        r[5] = v2;
        r[6] = u1;
        r[7] = v1;
        r[8] = 1.0f;
    }
    for (int k = 0; k < 9; ++k) At[72 + k] = 0.0f;
    in_svd(At, 9, 8, 9, Vt, Wd, true);   // m < n: the roles swap, vt is temp_u and its row 8 the completion row
    float w[3], u[9], vt[9], uw[9], Fn[9], tmp[9];
    in_svd33(At + 72, w, u, vt);
    w[2] = 0.0f;
    const float D[9] = {w[0], 0.0f, 0.0f, 0.0f, w[1], 0.0f, 0.0f, 0.0f, w[2]};
    in_mul33(u, D, uw);
    in_mul33(uw, vt, Fn);
    in_mul33(T2t, Fn, tmp);
    in_mul33(tmp, T1, F21);
}

// the two chi-square values of match i under H (:497-549)
ORBX_HD void in_terms_h(const float* h, const float* hi, float u1, float v1, float u2, float v2, float inv_s2,
                        float* c1, float* c2)
{
    const float w2 = (float)(1.0 / (double)(__builtin_fmaf(hi[6], u2, hi[7] * v2) + hi[8]));
    const float u2in1 = (__builtin_fmaf(hi[0], u2, hi[1] * v2) + hi[2]) * w2;
    const float v2in1 = (__builtin_fmaf(hi[3], u2, hi[4] * v2) + hi[5]) * w2;
    const float ax = u1 - u2in1, ay = v1 - v2in1;
    *c1 = __builtin_fmaf(ax, ax, ay * ay) * inv_s2;
    const float w1 = (float)(1.0 / (double)(__builtin_fmaf(h[6], u1, h[7] * v1) + h[8]));
    const float u1in2 = (__builtin_fmaf(h[0], u1, h[1] * v1) + h[2]) * w1;
    const float v1in2 = (__builtin_fmaf(h[3], u1, h[4] * v1) + h[5]) * w1;
    const float bx = u2 - u1in2, by = v2 - v1in2;
    *c2 = __builtin_fmaf(bx, bx, by * by) * inv_s2;
}

// the two chi-square values of match i under F (:623-672)
ORBX_HD void in_terms_f(const float* f, float u1, float v1, float u2, float v2, float inv_s2, float* c1, float* c2)
{
    const float a2 = __builtin_fmaf(f[0], u1, f[1] * v1) + f[2];
    const float b2 = __builtin_fmaf(f[3], u1, f[4] * v1) + f[5];
    const float c2_ = __builtin_fmaf(f[6], u1, f[7] * v1) + f[8];
    const float num2 = __builtin_fmaf(a2, u2, b2 * v2) + c2_;
    *c1 = ((num2 * num2) / __builtin_fmaf(a2, a2, b2 * b2)) * inv_s2;
    const float a1 = __builtin_fmaf(f[0], u2, f[3] * v2) + f[6];
    const float b1 = __builtin_fmaf(f[1], u2, f[4] * v2) + f[7];
    const float c1_ = __builtin_fmaf(f[2], u2, f[5] * v2) + f[8];
    const float num1 = __builtin_fmaf(a1, u1, b1 * v1) + c1_;
    *c2 = ((num1 * num1) / __builtin_fmaf(a1, a1, b1 * b1)) * inv_s2;
}

// iteration `it` of FindHomography (which = 0) or FindFundamental (1) as an independent hypothesis, by one lane: the
// 8-point solve, then CheckHomography / CheckFundamental over the N matches with the score summed as it goes
ORBX_HD void in_hypothesis(const InTables& T, int a, int b, const InPair& W, const InHyp& H, int which, int it,
                           float sigma)
{
    if (W.hdr[kInValid] != 1) return;
    const int N = W.hdr[kInN];
    const orbx_keypoint* k1 = T.kps + (size_t)a * T.cap;
    const orbx_keypoint* k2 = T.kps + (size_t)b * T.cap;
    float M[9], Mi[9], p1[16], p2[16];
    for (int j = 0; j < 8; ++j) {
        const int idx = W.sets[8 * it + j];
        in_norm_pt(k1[W.m1[idx]], W.fl + kInMean, p1 + 2 * j, p1 + 2 * j + 1);
        in_norm_pt(k2[W.m2[idx]], W.fl + kInMean + 4, p2 + 2 * j, p2 + 2 * j + 1);
    }
    if (which == 0) {
        in_compute_h(p1, p2, W.fl + kInT1, W.fl + kInT2inv, M, Mi);
    } else {
        in_compute_f(p1, p2, W.fl + kInT1, W.fl + kInT2t, M);
        for (int i = 0; i < 9; ++i) Mi[i] = 0.0f;
    }
    const float th = which == 0 ? (float)5.991 : (float)3.841, th_score = (float)5.991;
    const float inv_s2 = (float)(1.0 / (double)(sigma * sigma));
    float score = 0.0f;
    for (int base = 0; base < N; base += 64) {
        unsigned long long wb = 0;
        for (int j = 0; j < 64 && base + j < N; ++j) {
            const int i = base + j;
            const orbx_keypoint& q1 = k1[W.m1[i]];
            const orbx_keypoint& q2 = k2[W.m2[i]];
            float c1, c2;
            if (which == 0) in_terms_h(M, Mi, q1.x, q1.y, q2.x, q2.y, inv_s2, &c1, &c2);
            else in_terms_f(M, q1.x, q1.y, q2.x, q2.y, inv_s2, &c1, &c2);
            bool in = true;
            if (c1 > th) in = false;
            else score += th_score - c1;
            if (c2 > th) in = false;
            else score += th_score - c2;
            if (in) wb |= 1ull << j;
        }
        H.words[base >> 6] = wb;
    }
    for (int i = 0; i < 9; ++i) H.M[i] = M[i];
    *H.score = score;
}

// ---- select ----
struct InOut {
    int *status, *model, *reason;
    float *scores, *H21, *F21;
    uint8_t *inliersH, *inliersF;
    float *R21, *t21, *p3d;
    uint8_t* triangulated;
    int* ngood;
    float* parallax;
    int* nmatches_left;
    int* matches_out;
};

ORBX_HD InOut in_out_of(const orbm_init_out& o, int p, int cap, int match_stride)
{
    InOut O;
    const size_t s = (size_t)p;
    O.status = o.status + s;
    O.model = o.model + s;
    O.reason = o.reason + s;
    O.scores = o.scores + 2 * s;
    O.H21 = o.H21 + 9 * s;
    O.F21 = o.F21 + 9 * s;
    O.inliersH = o.inliersH + s * cap;
    O.inliersF = o.inliersF + s * cap;
    O.R21 = o.R21 + 9 * s;
    O.t21 = o.t21 + 3 * s;
    O.p3d = o.p3d + 3 * s * cap;
    O.triangulated = o.triangulated + s * cap;
    O.ngood = o.ngood + 8 * s;
    O.parallax = o.parallax + 8 * s;
    O.nmatches_left = o.nmatches_left + s;
    O.matches_out = o.matches_out ? o.matches_out + s * match_stride : nullptr;
    return O;
}

template <int NT>
ORBX_HD void in_select(InShared<NT>& S, const InPair& W, const InLayout& L, int cap, int iters, const InOut& O)
{
    if (W.hdr[kInValid] != 1) return;
    const int tid = in_tid();
    const int N = W.hdr[kInN];
    if (tid == 0) {
        int pick[2];
        float best[2];
        for (int which = 0; which < 2; ++which) {
            pick[which] = -1;
            best[which] = 0.0f;
            for (int it = 0; it < iters; ++it) {
                const float sc = *in_hyp(W, L, which, it, iters).score;
                if (sc > best[which]) {
                    best[which] = sc;
                    pick[which] = it;
                }
            }
        }
        const float RH = best[0] / (best[0] + best[1]);
        const int model = (double)RH > 0.40 ? 1 : 2;
        const bool none = pick[model - 1] < 0;   // both scores 0: the reference reads an empty cv::Mat
        W.hdr[kInPickH] = pick[0];
        W.hdr[kInPickF] = pick[1];
        W.hdr[kInModel] = none ? 0 : model;
        W.hdr[kInStatus] = none ? ORBM_INIT_NO_MODEL : 0;
        O.scores[0] = best[0];
        O.scores[1] = best[1];
        for (int which = 0; which < 2; ++which) {
            float* dst = which ? O.F21 : O.H21;
            const float* src = pick[which] >= 0 ? in_hyp(W, L, which, pick[which], iters).M : nullptr;
            for (int i = 0; i < 9; ++i) {
                dst[i] = src ? src[i] : 0.0f;
                W.fl[(which ? kInF : kInH) + i] = dst[i];
            }
        }
        S.win = pick[0];
        S.ok = pick[1];
    }
    for (int i = tid; i < cap; i += NT) {
        O.inliersH[i] = 0;
        O.inliersF[i] = 0;
    }
    in_sync();
    for (int which = 0; which < 2; ++which) {
        const int pick = which ? S.ok : S.win;
        if (pick < 0) continue;
        const unsigned long long* words = in_hyp(W, L, which, pick, iters).words;
        uint8_t* dst = which ? O.inliersF : O.inliersH;
        for (int j = tid; j < N; j += NT)
            if ((words[j >> 6] >> (j & 63)) & 1ull) dst[W.m1[j]] = 1;   // m1 < n1 <= cap in a pair that setup wrote
    }
}

// ---- the motion candidates ----
// DecomposeE (:1280-1300) of E21 = K.t()*F21*K: candidate c of ReconstructF's four (R1 t, R2 t, R1 -t, R2 -t)
ORBX_HD void in_cand_f(const float* F21, const float* K, int c, float* R, float* t)
{
    float Kt[9], tmp[9], E[9], w[3], u[9], vt[9];
    in_t33(K, Kt);
    in_mul33(Kt, F21, tmp);
    in_mul33(tmp, K, E);
    in_svd33(E, w, u, vt);
    double nn = 0.0;
    for (int r = 0; r < 3; ++r) nn += (double)u[3 * r + 2] * (double)u[3 * r + 2];
    const float inv = (float)(1.0 / __builtin_sqrt(nn));
    for (int r = 0; r < 3; ++r) {
        const float tr = u[3 * r + 2] * inv + 0.0f;
        t[r] = (c & 2) ? tr * -1.0f + 0.0f : tr;
    }
    const float Wm[9] = {0.0f, -1.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f};
    float Wt[9], uw[9];
    in_t33(Wm, Wt);
    in_mul33(u, (c & 1) ? Wt : Wm, uw);
    in_mul33(uw, vt, R);
    if (in_det33(R) < 0.0)
        for (int i = 0; i < 9; ++i) R[i] = R[i] * -1.0f + 0.0f;
}

// candidate c of ReconstructH's eight (:832-934); false where d1/d2 < 1.00001 || d2/d3 < 1.00001 returns
ORBX_HD bool in_cand_h(const float* H21, const float* K, int c, float* R, float* t)
{
    float invK[9], tmp[9], A[9], w[3], U[9], Vt[9];
    in_inv33(K, invK);
    in_mul33(invK, H21, tmp);
    in_mul33(tmp, K, A);
    in_svd33(A, w, U, Vt);
    const float s = (float)(in_det33(U) * in_det33(Vt));
    const float d1 = w[0], d2 = w[1], d3 = w[2];
    if ((double)(d1 / d2) < 1.00001 || (double)(d2 / d3) < 1.00001) return false;
    const float d12 = __builtin_fmaf(d1, d1, -(d2 * d2)), d13 = __builtin_fmaf(d1, d1, -(d3 * d3)),
                d23 = __builtin_fmaf(d2, d2, -(d3 * d3));
    const float aux1 = (float)__builtin_sqrt((double)(d12 / d13));
    const float aux3 = (float)__builtin_sqrt((double)(d23 / d13));
    const int i = c & 3;
    const float x1 = (i & 2) ? -aux1 : aux1, x3 = (i & 1) ? -aux3 : aux3;
    const bool neg = i == 1 || i == 2;
    float Rp[9] = {1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f};
    float tp[3];
    if (c < 4) {
        const float aux_s = (float)(__builtin_sqrt((double)(d12 * d23)) / (double)((d1 + d3) * d2));
        const float ct = __builtin_fmaf(d2, d2, d1 * d3) / ((d1 + d3) * d2);
        const float st = neg ? -aux_s : aux_s;
        Rp[0] = ct;
        Rp[2] = -st;
        Rp[6] = st;
        Rp[8] = ct;
        const float k = d1 - d3;
        tp[0] = x1 * k + 0.0f;
        tp[1] = 0.0f * k + 0.0f;
        tp[2] = -x3 * k + 0.0f;
    } else {
        const float aux_s = (float)(__builtin_sqrt((double)(d12 * d23)) / (double)((d1 - d3) * d2));
        const float cp = __builtin_fmaf(d1, d3, -(d2 * d2)) / ((d1 - d3) * d2);
        const float sp = neg ? -aux_s : aux_s;
        Rp[0] = cp;
        Rp[2] = sp;
        Rp[4] = -1.0f;
        Rp[6] = sp;
        Rp[8] = -cp;
        const float k = d1 + d3;
        tp[0] = x1 * k + 0.0f;
        tp[1] = 0.0f * k + 0.0f;
        tp[2] = x3 * k + 0.0f;
    }
    float sURp[9];   // (s*U)*Rp: the gemm with alpha = s in double
    for (int r = 0; r < 3; ++r)
        for (int q = 0; q < 3; ++q)
            sURp[3 * r + q] =
                (float)((double)((U[3 * r] * Rp[q] + U[3 * r + 1] * Rp[3 + q]) + U[3 * r + 2] * Rp[6 + q]) * (double)s);
    in_mul33(sURp, Vt, R);
    float tt[3];
    double nn = 0.0;
    for (int r = 0; r < 3; ++r) {
        tt[r] = (U[3 * r] * tp[0] + U[3 * r + 1] * tp[1]) + U[3 * r + 2] * tp[2];
        nn += (double)tt[r] * (double)tt[r];
    }
    const float inv = (float)(1.0 / __builtin_sqrt(nn));
    for (int r = 0; r < 3; ++r) t[r] = tt[r] * inv + 0.0f;
    return true;
}

struct InView {
    float P1[12], P2[12], O2[3], R[9], t[3];
    float fx, fy, cx, cy, th2;
};

// the body of CheckRT's loop (:1175-1258) for one inlier match: 0 = skipped, bit 0 = counted (vP3D written), bit 1 =
// vbGood
ORBX_HD int in_check_point(const InView& V, float x1, float y1, float x2, float y2, float* X, float* cosp)
{
    float At[16], Vt[16];
    double Wd[4];
    for (int k = 0; k < 4; ++k) {   // A.row = pt * P.row(2) - P.row(.), held transposed
        At[4 * k] = x1 * V.P1[8 + k] - V.P1[k];
        At[4 * k + 1] = y1 * V.P1[8 + k] - V.P1[4 + k];
        At[4 * k + 2] = x2 * V.P2[8 + k] - V.P2[k];
        At[4 * k + 3] = y2 * V.P2[8 + k] - V.P2[4 + k];
    }
    in_svd(At, 4, 4, 4, Vt, Wd, false);
    const float iw = (float)(1.0 / (double)Vt[15]);
    for (int k = 0; k < 3; ++k) X[k] = Vt[12 + k] * iw + 0.0f;
    const float big = __builtin_inff();
    for (int k = 0; k < 3; ++k)
        if (!(__builtin_fabsf(X[k]) < big)) return 0;   // !isfinite
    double n1 = 0.0, n2 = 0.0, dot = 0.0;
    for (int k = 0; k < 3; ++k) {
        const float a = X[k] - 0.0f, b = X[k] - V.O2[k];
        n1 += (double)a * (double)a;
        n2 += (double)b * (double)b;
        dot += (double)a * (double)b;
    }
    const float dist1 = (float)__builtin_sqrt(n1), dist2 = (float)__builtin_sqrt(n2);
    const float cp = (float)(dot / (double)(dist1 * dist2));
    const bool low = (double)cp < 0.99998;
    if (X[2] <= 0.0f && low) return 0;
    float X2[3];
    for (int r = 0; r < 3; ++r) X2[r] = ((V.R[3 * r] * X[0] + V.R[3 * r + 1] * X[1]) + V.R[3 * r + 2] * X[2]) + V.t[r];
    if (X2[2] <= 0.0f && low) return 0;
    const float iz1 = (float)(1.0 / (double)X[2]);
    const float e1x = __builtin_fmaf(V.fx * X[0], iz1, V.cx) - x1, e1y = __builtin_fmaf(V.fy * X[1], iz1, V.cy) - y1;
    if (__builtin_fmaf(e1x, e1x, e1y * e1y) > V.th2) return 0;
    const float iz2 = (float)(1.0 / (double)X2[2]);
    const float e2x = __builtin_fmaf(V.fx * X2[0], iz2, V.cx) - x2, e2y = __builtin_fmaf(V.fy * X2[1], iz2, V.cy) - y2;
    if (__builtin_fmaf(e2x, e2x, e2y * e2y) > V.th2) return 0;
    *cosp = cp;
    return low ? 3 : 1;
}

// one candidate: its (R, t), then CheckRT (:1123-1278) over the chosen model's inliers
ORBX_HD void in_candidate(const InTables& T, int a, int b, const InPair& W, const InLayout& L, int iters, int c,
                          float sigma)
{
    if (W.hdr[kInValid] != 1 || W.hdr[kInStatus] != 0) return;
    const int model = W.hdr[kInModel];
    if (model == 2 && c >= 4) return;
    const int N = W.hdr[kInN];
    const InCand C = in_cand(W, L, c, T.cap);
    const float K[9] = {T.fx, 0.0f, T.cx, 0.0f, T.fy, T.cy, 0.0f, 0.0f, 1.0f};
    InView V;
    float okf = 0.0f;
    for (int i = 0; i < 9; ++i) V.R[i] = 0.0f;
    for (int i = 0; i < 3; ++i) V.t[i] = 0.0f;
    const int lane = in_tid();
    if (lane == 0) {
        bool ok = true;
        if (model == 2) in_cand_f(W.fl + kInF, K, c, V.R, V.t);
        else ok = in_cand_h(W.fl + kInH, K, c, V.R, V.t);
        okf = ok ? 1.0f : 0.0f;
    }
    okf = in_bcast(okf);
    if (okf == 0.0f) {
        if (lane == 0) {
            *C.singular = 1;
            *C.ngood = 0;
            *C.parallax = 0.0f;
        }
        return;
    }
    for (int i = 0; i < 9; ++i) V.R[i] = in_bcast(V.R[i]);
    for (int i = 0; i < 3; ++i) V.t[i] = in_bcast(V.t[i]);
    for (int r = 0; r < 3; ++r) {
        for (int q = 0; q < 4; ++q) {
            V.P1[4 * r + q] = q < 3 ? K[3 * r + q] : 0.0f;
            const float m0 = q < 3 ? V.R[q] : V.t[0], m1 = q < 3 ? V.R[3 + q] : V.t[1],
                        m2 = q < 3 ? V.R[6 + q] : V.t[2];
            V.P2[4 * r + q] = (K[3 * r] * m0 + K[3 * r + 1] * m1) + K[3 * r + 2] * m2;
        }
        // O2 = -R.t()*t: the gemm with alpha = -1
        V.O2[r] = (float)((double)((V.R[r] * V.t[0] + V.R[3 + r] * V.t[1]) + V.R[6 + r] * V.t[2]) * -1.0);
    }
    V.fx = T.fx;
    V.fy = T.fy;
    V.cx = T.cx;
    V.cy = T.cy;
    V.th2 = (float)(4.0 * (double)(sigma * sigma));
    const orbx_keypoint* k1 = T.kps + (size_t)a * T.cap;
    const orbx_keypoint* k2 = T.kps + (size_t)b * T.cap;
    const unsigned long long* words =
        in_hyp(W, L, model - 1, W.hdr[model == 1 ? kInPickH : kInPickF], iters).words;
#if defined(__HIP_DEVICE_COMPILE__)
    const int NL = 64;
#else
    const int NL = 1;
#endif
    int ngood = 0;
    for (int base = 0; base < N; base += NL) {
        const int i = base + lane;
        int f = 0;
        if (i < N) {
            float X[3] = {0.0f, 0.0f, 0.0f}, cp = 0.0f;
            if ((words[i >> 6] >> (i & 63)) & 1ull) {
                const orbx_keypoint& q1 = k1[W.m1[i]];
                const orbx_keypoint& q2 = k2[W.m2[i]];
                f = in_check_point(V, q1.x, q1.y, q2.x, q2.y, X, &cp);
            }
            C.flags[i] = (uint8_t)f;
            C.cosp[i] = cp;
            for (int k = 0; k < 3; ++k) C.p3d[3 * (size_t)i + k] = f ? X[k] : 0.0f;
        }
#if defined(__HIP_DEVICE_COMPILE__)
        ngood += __popcll(__ballot(f != 0));
#else
        ngood += f != 0;
#endif
    }
    if (lane == 0) {
        for (int i = 0; i < 9; ++i) C.R[i] = V.R[i];
        for (int i = 0; i < 3; ++i) C.t[i] = V.t[i];
        *C.singular = 0;
        *C.ngood = ngood;
        *C.parallax = 0.0f;
    }
    in_sync();   // the wave's own stores to cosp / flags, read below by other lanes
    if (ngood == 0) return;
    // sort(vCosParallax) then entry min(50, size - 1): the entry of that rank.  A cosine that is NaN (a point at the
    // first camera's centre passes every test of the loop) sorts behind every number; equal keys rank by position.
    const int want = ngood - 1 < 50 ? ngood - 1 : 50;
    for (int i = lane; i < N; i += NL) {
        if (!C.flags[i]) continue;
        const float v = C.cosp[i];
        const bool vnan = v != v;
        int rank = 0;
        for (int j = 0; j < N; ++j)
            if (C.flags[j]) {
                const float u = C.cosp[j];
                const bool unan = u != u;
                const bool tie = u == v || (unan && vnan);
                rank += (u < v || (vnan && !unan) || (tie && j < i)) ? 1 : 0;
            }
        if (rank == want)
            *C.parallax = (float)(((double)fixed_acosf(v) * 180.0) / 3.1415926535897932384626433832795);
    }
}

// ---- the decision of ReconstructF (:721-791) / ReconstructH (:938-1004) and the outputs ----
template <int NT>
ORBX_HD void in_finish(InShared<NT>& S, const InPair& W, const InLayout& L, int cap, int iters, const int* match12,
                       int match_stride, int flags, const InOut& O)
{
    if (W.hdr[kInValid] != 1) return;
    const int tid = in_tid();
    const int N = W.hdr[kInN], n1 = W.hdr[kInN1];
    const int model = W.hdr[kInModel];
    if (tid == 0) {
        int status = W.hdr[kInStatus], reason = ORBM_INIT_REASON_NONE, win = -1;
        const float min_parallax = 1.0f;
        const int min_tri = 50;
        int good[8];
        float par[8];
        for (int c = 0; c < 8; ++c) {
            good[c] = 0;
            par[c] = 0.0f;
        }
        if (status == 0) {
            const int pick = W.hdr[model == 1 ? kInPickH : kInPickF];
            const unsigned long long* words = in_hyp(W, L, model - 1, pick, iters).words;
            int ninl = 0;
            for (int j = 0; j < N; j += 64) {
                unsigned long long wb = words[j >> 6];
#if defined(__HIP_DEVICE_COMPILE__)
                ninl += __popcll(wb);
#else
                ninl += __builtin_popcountll(wb);
#endif
            }
            const int nc = model == 2 ? 4 : 8;
            bool singular = false;
            for (int c = 0; c < nc; ++c) {
                const InCand C = in_cand(W, L, c, cap);
                if (*C.singular) singular = true;
                good[c] = *C.ngood;
                par[c] = *C.parallax;
            }
            if (model == 2) {
                int mx = good[0];
                for (int c = 1; c < 4; ++c) mx = good[c] > mx ? good[c] : mx;
                const int a = (int)(0.9 * (double)ninl);
                const int nmin = a > min_tri ? a : min_tri;
                int nsim = 0;
                for (int c = 0; c < 4; ++c)
                    if ((double)good[c] > 0.7 * (double)mx) ++nsim;
                if (mx < nmin || nsim > 1) {
                    reason = ORBM_INIT_F_AMBIGUOUS;
                } else {
                    int c = 0;
                    while (good[c] != mx) ++c;   // the else-if chain takes the first candidate with maxGood
                    if (par[c] > min_parallax) win = c;
                    else reason = ORBM_INIT_F_PARALLAX;
                }
            } else if (singular) {
                reason = ORBM_INIT_H_SINGULAR;
                for (int c = 0; c < 8; ++c) {
                    good[c] = 0;
                    par[c] = 0.0f;
                }
            } else {
                int best = 0, second = 0, idx = -1;
                float bpar = -1.0f;
                for (int c = 0; c < 8; ++c) {
                    if (good[c] > best) {
                        second = best;
                        best = good[c];
                        idx = c;
                        bpar = par[c];
                    } else if (good[c] > second) {
                        second = good[c];
                    }
                }
                if ((double)second < 0.75 * (double)best && bpar >= min_parallax && best > min_tri &&
                    (double)best > 0.9 * (double)ninl)
                    win = idx;
                else reason = ORBM_INIT_H_TEST;
            }
            if (win < 0) status = ORBM_INIT_FAILED;
        }
        *O.status = status;
        *O.model = model;
        *O.reason = reason;
        for (int c = 0; c < 8; ++c) {
            O.ngood[c] = good[c];
            O.parallax[c] = par[c];
        }
        const float* R = win >= 0 ? in_cand(W, L, win, cap).R : nullptr;
        for (int i = 0; i < 9; ++i) O.R21[i] = R ? R[i] : 0.0f;
        for (int i = 0; i < 3; ++i) O.t21[i] = R ? R[9 + i] : 0.0f;
        int left = N;
        if (win >= 0) {
            const uint8_t* fl = in_cand(W, L, win, cap).flags;
            left = 0;
            for (int j = 0; j < N; ++j) left += (fl[j] >> 1) & 1;
        }
        *O.nmatches_left = left;
        S.win = win;
    }
    for (int i = tid; i < cap; i += NT) {
        O.triangulated[i] = 0;
        for (int k = 0; k < 3; ++k) O.p3d[3 * (size_t)i + k] = 0.0f;
    }
    in_sync();
    const int win = S.win;
    if (win >= 0) {
        const InCand C = in_cand(W, L, win, cap);
        for (int j = tid; j < N; j += NT) {
            const int f = C.flags[j];
            if (!f) continue;
            const int i1 = W.m1[j];
            for (int k = 0; k < 3; ++k) O.p3d[3 * (size_t)i1 + k] = C.p3d[3 * (size_t)j + k];
            O.triangulated[i1] = (uint8_t)((f >> 1) & 1);
        }
    }
    if ((flags & ORBM_INIT_PRUNE_MATCHES) && O.matches_out) {
        in_sync();   // triangulated is complete
        // Tracking.cc: if(mvIniMatches[i]>=0 && !vbTriangulated[i]) mvIniMatches[i]=-1, after a successful Initialize
        for (int i = tid; i < match_stride; i += NT) {
            const int m = match12[i];
            O.matches_out[i] = (win >= 0 && i < n1 && m >= 0 && !O.triangulated[i]) ? -1 : m;
        }
    }
}

// ---- kernels ----
__global__ __launch_bounds__(kInLanes) void k_init_setup(InTables T, const int* __restrict__ pair_a,
                                                         const int* __restrict__ pair_b,
                                                         const int* __restrict__ match12, int match_stride,
                                                         const int* __restrict__ draws, int draws_stride, int iters,
                                                         int iters_ok, void* work, InLayout L, int* status)
{
    __shared__ InShared<kInLanes> S;
    const int p = blockIdx.x;
    in_setup<kInLanes>(S, T, pair_a[p], pair_b[p], match12 + (size_t)p * match_stride,
                       draws + (size_t)p * draws_stride, iters, iters_ok != 0, in_pair(work, L, p, T.cap), status + p);
}

__global__ __launch_bounds__(64) void k_init_hyp(InTables T, const int* __restrict__ pair_a,
                                                 const int* __restrict__ pair_b, void* work, InLayout L, int iters,
                                                 float sigma)
{
    // a wave is 64 iterations of one model: its lanes take the same branches but for the Jacobi's own tests
    const int it = (int)(blockIdx.x >> 1) * 64 + (int)threadIdx.x, which = blockIdx.x & 1, p = blockIdx.y;
    const InPair W = in_pair(work, L, p, T.cap);
    if (it >= iters || W.hdr[kInValid] != 1) return;   // an invalid pair's indices were never checked
    in_hypothesis(T, pair_a[p], pair_b[p], W, in_hyp(W, L, which, it, iters), which, it, sigma);
}

__global__ __launch_bounds__(kInLanes) void k_init_select(void* work, InLayout L, int cap, int iters,
                                                          orbm_init_out out, int match_stride)
{
    __shared__ InShared<kInLanes> S;
    const int p = blockIdx.x;
    in_select<kInLanes>(S, in_pair(work, L, p, cap), L, cap, iters, in_out_of(out, p, cap, match_stride));
}

__global__ __launch_bounds__(64) void k_init_cand(InTables T, const int* __restrict__ pair_a,
                                                  const int* __restrict__ pair_b, void* work, InLayout L, int iters,
                                                  float sigma)
{
    const int c = blockIdx.x, p = blockIdx.y;
    const InPair W = in_pair(work, L, p, T.cap);
    if (W.hdr[kInValid] != 1) return;
    in_candidate(T, pair_a[p], pair_b[p], W, L, iters, c, sigma);
}

__global__ __launch_bounds__(kInLanes) void k_init_finish(void* work, InLayout L, int cap, int iters,
                                                          const int* __restrict__ match12, int match_stride,
                                                          int flags, orbm_init_out out)
{
    __shared__ InShared<kInLanes> S;
    const int p = blockIdx.x;
    in_finish<kInLanes>(S, in_pair(work, L, p, cap), L, cap, iters, match12 + (size_t)p * match_stride, match_stride,
                        flags, in_out_of(out, p, cap, match_stride));
}

static bool in_out_ok(const orbm_init_out* o, int flags)
{
    if (!o) return false;
    const uintptr_t a4 = (uintptr_t)o->status | (uintptr_t)o->model | (uintptr_t)o->reason | (uintptr_t)o->scores |
                         (uintptr_t)o->H21 | (uintptr_t)o->F21 | (uintptr_t)o->R21 | (uintptr_t)o->t21 |
                         (uintptr_t)o->p3d | (uintptr_t)o->ngood | (uintptr_t)o->parallax |
                         (uintptr_t)o->nmatches_left | (uintptr_t)o->matches_out;
    return o->status && o->model && o->reason && o->scores && o->H21 && o->F21 && o->inliersH && o->inliersF &&
           o->R21 && o->t21 && o->p3d && o->triangulated && o->ngood && o->parallax && o->nmatches_left &&
           (!(flags & ORBM_INIT_PRUNE_MATCHES) || o->matches_out) && !(a4 & 3);
}

static bool in_params_ok(const orbm_pose_params* P, float sigma, int flags)
{
    return P && sigma > 0.0f && !(flags & ~ORBM_INIT_PRUNE_MATCHES);
}

}  // namespace orbx

using namespace orbx;

extern "C" {

float orbx_fixed_acosf(float x) { return fixed_acosf(x); }

void orbx_init_sets(int n, const int* draws, int iterations, int* sets)
{
    if (n < 8 || !draws || !sets) return;
    for (int it = 0; it < iterations; ++it) in_set(n, draws + 8 * it, sets + 8 * it);
}

size_t orbm_init_workspace_bytes(int npairs, int cap, int max_iterations)
{
    if (npairs < 0 || npairs > kInMaxPairs || cap < 1 || cap > ORBM_MAX_FEATURES || max_iterations < 1 ||
        max_iterations > kInMaxIters)
        return 0;
    return in_layout(npairs, cap, max_iterations).total;
}

orbx_status orbm_initialize_device(const orbx_keypoint* d_kps, const int* d_counts, int nframes, int cap,
                                   const int* d_pair_a, const int* d_pair_b, int npairs, const int* d_matches12,
                                   int match_stride, const int* d_draws, int draws_stride,
                                   const orbm_pose_params* params, float sigma, int max_iterations, int flags,
                                   void* d_work, size_t work_bytes, const orbm_init_out* out, void* stream)
{
    const bool iters_ok = max_iterations >= 1 && max_iterations <= kInMaxIters;
    const int iters = iters_ok ? max_iterations : 1;
    const uintptr_t a4 = (uintptr_t)d_kps | (uintptr_t)d_counts | (uintptr_t)d_pair_a | (uintptr_t)d_pair_b |
                         (uintptr_t)d_matches12 | (uintptr_t)d_draws;
    if (!d_kps || !d_counts || nframes < 0 || cap < 1 || cap > ORBM_MAX_FEATURES || !d_pair_a || !d_pair_b ||
        npairs < 0 || npairs > kInMaxPairs || !d_matches12 || match_stride < cap || !d_draws ||
        (iters_ok && draws_stride < 8 * max_iterations) || !in_params_ok(params, sigma, flags) || !d_work ||
        !in_out_ok(out, flags) || (a4 & 3) || ((uintptr_t)d_work & 15) ||
        work_bytes < in_layout(npairs, cap, iters).total)
        return ORBX_EINVAL;
    if (npairs == 0) return ORBX_OK;
    const InTables T = {d_kps, d_counts, nframes, cap, params->fx, params->fy, params->cx, params->cy};
    const InLayout L = in_layout(npairs, cap, iters);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_init_setup, dim3((unsigned)npairs), dim3(kInLanes), 0, s, T, d_pair_a, d_pair_b, d_matches12,
                       match_stride, d_draws, draws_stride, iters, iters_ok ? 1 : 0, d_work, L, out->status);
    if (iters_ok) {
        hipLaunchKernelGGL(k_init_hyp, dim3((unsigned)(2 * ((iters + 63) / 64)), (unsigned)npairs), dim3(64), 0, s, T,
                           d_pair_a, d_pair_b, d_work, L, iters, sigma);
        hipLaunchKernelGGL(k_init_select, dim3((unsigned)npairs), dim3(kInLanes), 0, s, d_work, L, cap, iters, *out,
                           match_stride);
        hipLaunchKernelGGL(k_init_cand, dim3(8u, (unsigned)npairs), dim3(64), 0, s, T, d_pair_a, d_pair_b, d_work, L,
                           iters, sigma);
        hipLaunchKernelGGL(k_init_finish, dim3((unsigned)npairs), dim3(kInLanes), 0, s, d_work, L, cap, iters,
                           d_matches12, match_stride, flags, *out);
    }
    return hipGetLastError() == hipSuccess ? ORBX_OK : ORBX_EDEVICE;
}

// the one-pair forms: a table of two frames (slots 0 and 1) at stride cap
static bool in_one_args_ok(const orbx_keypoint* kps1, int n1, const orbx_keypoint* kps2, int n2, const int* matches12,
                           const int* draws, const orbm_pose_params* params, float sigma, int flags,
                           const orbm_init_out* out)
{
    const uintptr_t a4 = (uintptr_t)kps1 | (uintptr_t)kps2 | (uintptr_t)matches12 | (uintptr_t)draws;
    return n1 >= 0 && n1 <= ORBM_MAX_FEATURES && n2 >= 0 && n2 <= ORBM_MAX_FEATURES &&
           (n1 == 0 || (kps1 && matches12)) && (n2 == 0 || kps2) && draws && in_params_ok(params, sigma, flags) &&
           in_out_ok(out, flags) && !(a4 & 3);
}

orbx_status orbm_initialize_host(const orbx_keypoint* kps1, int n1, const orbx_keypoint* kps2, int n2,
                                 const int* matches12, const int* draws, const orbm_pose_params* params, float sigma,
                                 int max_iterations, int flags, const orbm_init_out* out)
{
    if (!in_one_args_ok(kps1, n1, kps2, n2, matches12, draws, params, sigma, flags, out)) return ORBX_EINVAL;
    if (max_iterations < 1 || max_iterations > kInMaxIters) {   // no draw is read
        *out->status = ORBM_INIT_INVALID;
        return ORBX_OK;
    }
    const int iters = max_iterations;
    int cap = n1 > n2 ? n1 : n2;
    if (cap < 1) cap = 1;
    std::vector<orbx_keypoint> kps((size_t)2 * cap);
    pack_pair(kps.data(), (size_t)cap, kps1, (size_t)n1, kps2, (size_t)n2);
    std::vector<int> m12((size_t)cap, -1);
    if (n1) std::memcpy(m12.data(), matches12, sizeof(int) * (size_t)n1);
    const int counts[2] = {n1, n2};
    const InLayout L = in_layout(1, cap, iters);
    std::vector<unsigned long long> work(L.total / 8 + 2);
    void* w = work.data();   // operator new aligns to 16
    const InTables T = {kps.data(), counts, 2, cap, params->fx, params->fy, params->cx, params->cy};
    const InPair W = in_pair(w, L, 0, cap);
    InShared<1> S;
    int st = 0;
    in_setup<1>(S, T, 0, 1, m12.data(), draws, iters, true, W, &st);
    if (st) {
        *out->status = st;
        return ORBX_OK;
    }
    // outputs of the table's width, copied out at the caller's n1
    const size_t C = (size_t)cap;
    std::vector<uint8_t> inH(C), inF(C), tri(C);
    std::vector<float> p3d(3 * C);
    std::vector<int> mout(C);
    orbm_init_out o = *out;
    o.inliersH = inH.data();
    o.inliersF = inF.data();
    o.triangulated = tri.data();
    o.p3d = p3d.data();
    o.matches_out = (flags & ORBM_INIT_PRUNE_MATCHES) ? mout.data() : nullptr;
    const InOut O = in_out_of(o, 0, cap, cap);
    for (int which = 0; which < 2; ++which)
        for (int it = 0; it < iters; ++it) in_hypothesis(T, 0, 1, W, in_hyp(W, L, which, it, iters), which, it, sigma);
    in_select<1>(S, W, L, cap, iters, O);
    for (int c = 0; c < 8; ++c) in_candidate(T, 0, 1, W, L, iters, c, sigma);
    in_finish<1>(S, W, L, cap, iters, m12.data(), cap, flags, O);
    if (n1) {
        std::memcpy(out->inliersH, inH.data(), (size_t)n1);
        std::memcpy(out->inliersF, inF.data(), (size_t)n1);
        std::memcpy(out->triangulated, tri.data(), (size_t)n1);
        std::memcpy(out->p3d, p3d.data(), sizeof(float) * 3 * (size_t)n1);
        if (flags & ORBM_INIT_PRUNE_MATCHES) std::memcpy(out->matches_out, mout.data(), sizeof(int) * (size_t)n1);
    }
    return ORBX_OK;
}

orbx_status orbm_initialize(int device, const orbx_keypoint* kps1, int n1, const orbx_keypoint* kps2, int n2,
                            const int* matches12, const int* draws, const orbm_pose_params* params, float sigma,
                            int max_iterations, int flags, const orbm_init_out* out)
{
    if (!in_one_args_ok(kps1, n1, kps2, n2, matches12, draws, params, sigma, flags, out)) return ORBX_EINVAL;
    if (max_iterations < 1 || max_iterations > kInMaxIters) {   // no draw is read and nothing is launched
        *out->status = ORBM_INIT_INVALID;
        return ORBX_OK;
    }
    const int iters = max_iterations;
    int cap = n1 > n2 ? n1 : n2;
    if (cap < 1) cap = 1;
    const size_t C = (size_t)cap, m1 = (size_t)n1;
    const InLayout L = in_layout(1, cap, iters);
    const int head[4] = {n1, n2, 0, 1};   // counts, pair
    struct Res {
        int status, model, reason, left;
        float scores[2], H21[9], F21[9], R21[9], t21[3], parallax[8];
        int ngood[8];
    } r;
    HostCall c(device);
    const auto okp = c.stage<orbx_keypoint>(2 * C);
    const auto om12 = c.stage<int>(C);
    const auto ohd = c.in(head, 4);
    const auto odr = c.in(draws, (size_t)8 * iters);
    const auto ores = c.out<Res>(1);
    const auto oiH = c.out<uint8_t>(C);
    const auto oiF = c.out<uint8_t>(C);
    const auto otr = c.out<uint8_t>(C);
    const auto op3 = c.out<float>(3 * C);
    const auto omo = c.out<int>(C);
    const auto owk = c.out<uint8_t>(L.total + 16);
    orbx_status rc = c.prepare();
    if (rc != ORBX_OK) return rc;
    pack_pair(c.host(okp), C, kps1, m1, kps2, (size_t)n2);
    std::fill_n(std::copy_n(matches12, m1, c.host(om12)), C - m1, -1);
    rc = c.upload();
    if (rc != ORBX_OK) return rc;
    Res* const d = c.dev(ores);
    orbm_init_out o;
    o.status = &d->status;
    o.model = &d->model;
    o.reason = &d->reason;
    o.scores = d->scores;
    o.H21 = d->H21;
    o.F21 = d->F21;
    o.inliersH = c.dev(oiH);
    o.inliersF = c.dev(oiF);
    o.R21 = d->R21;
    o.t21 = d->t21;
    o.p3d = c.dev(op3);
    o.triangulated = c.dev(otr);
    o.ngood = d->ngood;
    o.parallax = d->parallax;
    o.nmatches_left = &d->left;
    o.matches_out = c.dev(omo);
    uint8_t* wk = (uint8_t*)(((uintptr_t)c.dev(owk) + 15) & ~(uintptr_t)15);
    rc = orbm_initialize_device(c.dev(okp), c.dev(ohd), 2, cap, c.dev(ohd, 2), c.dev(ohd, 3), 1, c.dev(om12), cap,
                                c.dev(odr), 8 * iters, params, sigma, max_iterations, flags, wk, L.total,
                                &o, c.stream());
    if (rc != ORBX_OK) return rc;
    std::vector<uint8_t> inH(C), inF(C), tri(C);
    std::vector<float> p3d(3 * C);
    std::vector<int> mout(C);
    c.fetch(ores, &r, 1);
    c.fetch(oiH, inH.data(), C);
    c.fetch(oiF, inF.data(), C);
    c.fetch(otr, tri.data(), C);
    c.fetch(op3, p3d.data(), 3 * C);
    c.fetch(omo, mout.data(), C);
    rc = c.finish();
    if (rc != ORBX_OK) return rc;
    *out->status = r.status;
    if (r.status & ORBM_INIT_INVALID) return ORBX_OK;   // of an invalid pair only the status is written
    *out->model = r.model;
    *out->reason = r.reason;
    *out->nmatches_left = r.left;
    std::memcpy(out->scores, r.scores, sizeof(r.scores));
    std::memcpy(out->H21, r.H21, sizeof(r.H21));
    std::memcpy(out->F21, r.F21, sizeof(r.F21));
    std::memcpy(out->R21, r.R21, sizeof(r.R21));
    std::memcpy(out->t21, r.t21, sizeof(r.t21));
    std::memcpy(out->parallax, r.parallax, sizeof(r.parallax));
    std::memcpy(out->ngood, r.ngood, sizeof(r.ngood));
    if (n1) {
        std::memcpy(out->inliersH, inH.data(), m1);
        std::memcpy(out->inliersF, inF.data(), m1);
        std::memcpy(out->triangulated, tri.data(), m1);
        std::memcpy(out->p3d, p3d.data(), sizeof(float) * 3 * m1);
        if (flags & ORBM_INIT_PRUNE_MATCHES) std::memcpy(out->matches_out, mout.data(), sizeof(int) * m1);
    }
    return ORBX_OK;
}

}  // extern "C"

// Sim3Solver (src/Sim3Solver.cc, include/Sim3Solver.h): the RANSAC of LoopClosing::ComputeSim3
// (src/LoopClosing.cc:274-323) between SearchByBoW(KF, KF) and SearchBySim3.  Kernels and C entry points
// (include/orbx.h).  The arithmetic order of everything below is DESIGN.md §3 "Sim3 solver arithmetic": cv::Mat
// CV_32F products as OpenCV 3.x's small-matrix gemm, MatExpr scales as convertTo with a float alpha, cv::eigen as
// JacobiImpl_<float>, cv::Rodrigues in double, sin / cos / atan2 from orbx_math.hpp and not from a math library.
// Parity with a real OpenCV is unpinned; the Python restatement of tests/test_sim3_solver.py, this code compiled for
// the CPU (orbm_sim3_solve_host) and the gfx950 code agree bit for bit.
//
// k_sim3_setup: one workgroup of 256 lanes per solver, the constructor (:37-112): every lane takes one i1 of a
//   256-feature chunk, decides whether the pair survives (both MapPoints, not bad, GetIndexInKeyFrame on both
//   sides) and computes its camera-frame points, projections and error bounds; survivors are stored at their rank
//   in i1 order (ballot prefix, as po_rank), so the compacted arrays are the reference's vectors.
// k_sim3_hyp: one wave64 per (iteration, solver).  RandomInt and the removal pick the triplet, every lane computes
//   the same 3-point solve (ComputeSim3, wave-uniform), then the lanes stride over the N pairs (CheckInliers) and
//   the inliers are one ballot word per 64 pairs, counted by popcount.
// k_sim3_select: one workgroup per solver.  Lane 0 walks the hypotheses in iteration order with the reference's
//   rule (:183-200, :203), the lanes expand the chosen mask into vbInliers and vbAlreadyMatched2.
// The device calls allocate nothing; the solvers live in the caller's workspace between the calls.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

#include "orbx_host.hpp"
#include "orbx_math.hpp"

namespace orbx {

constexpr int kS3Lanes = 256;
constexpr int kS3HdrInts = 8;      // N, valid, mRansacMaxIts
constexpr int kS3MaxGrid = 65535;  // solvers and iterations per call: a grid dimension each
constexpr int kS3HypFloats = 16;   // s12, R12[9], t12[3], the inlier count (int), 2 unused

// ---- workspace: per solver the compacted pairs, then per (solver, iteration of a call) one hypothesis ----
struct S3Layout {
    size_t solver_bytes, hyp_off, hyp_bytes, total;
    int words;
};

__host__ __device__ inline S3Layout s3_layout(int nsolvers, int cap, int iters)
{
    S3Layout L;
    L.words = (cap + 63) / 64;
    L.solver_bytes = ((size_t)kS3HdrInts * 4 + (size_t)cap * 4 * 14 + 15) & ~(size_t)15;
    L.hyp_off = L.solver_bytes * (size_t)nsolvers;
    L.hyp_bytes = (size_t)kS3HypFloats * 4 + (size_t)L.words * 8;
    L.total = L.hyp_off + L.hyp_bytes * (size_t)nsolvers * (size_t)iters;
    return L;
}

struct S3Solver {
    int* hdr;
    int *idx1, *idx2;   // mvnIndices1; indexKF2 of the pair's second MapPoint
    float *X1, *X2;     // mvX3Dc1, mvX3Dc2
    float *P1, *P2;     // mvP1im1, mvP2im2
    float *E1, *E2;     // mvnMaxError1, mvnMaxError2 as floats
};

ORBX_HD S3Solver s3_solver(void* work, const S3Layout& L, int s, int cap)
{
    uint8_t* b = (uint8_t*)work + L.solver_bytes * (size_t)s;
    S3Solver W;
    W.hdr = (int*)b;
    W.idx1 = W.hdr + kS3HdrInts;
    W.idx2 = W.idx1 + cap;
    W.X1 = (float*)(W.idx2 + cap);
    W.X2 = W.X1 + (size_t)3 * cap;
    W.P1 = W.X2 + (size_t)3 * cap;
    W.P2 = W.P1 + (size_t)2 * cap;
    W.E1 = W.P2 + (size_t)2 * cap;
    W.E2 = W.E1 + cap;
    return W;
}

struct S3Hyp {
    float* sim3;
    int* inl;
    unsigned long long* words;
};

ORBX_HD S3Hyp s3_hyp(void* work, const S3Layout& L, size_t h)
{
    uint8_t* b = (uint8_t*)work + L.hyp_off + L.hyp_bytes * h;
    S3Hyp H;
    H.sim3 = (float*)b;
    H.inl = (int*)(H.sim3 + 13);
    H.words = (unsigned long long*)(H.sim3 + kS3HypFloats);
    return H;
}

// ---- lanes ----
ORBX_HD int s3_tid()
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (int)threadIdx.x;
#else
    return 0;
#endif
}

ORBX_HD void s3_sync()
{
#if defined(__HIP_DEVICE_COMPILE__)
    __syncthreads();
#endif
}

template <int NT>
struct S3Shared {
    int wave_n[NT / 64 + 1];
    int bad, pick;
};

// rank of this lane among the chunk's lanes with `flag` set, in lane order, and their number
template <int NT>
ORBX_HD int s3_rank(S3Shared<NT>& S, bool flag, int* total)
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

// one row of a cv::Mat 3x3 * 3x1 product (gemm's small-matrix path): float, left to right
ORBX_HD float s3_row(const float* r, float x, float y, float z) { return (r[0] * x + r[1] * y) + r[2] * z; }

// FromCameraToImage / the tail of Project: invz = 1/z, x*invz, fx*x+cx
ORBX_HD void s3_to_image(const orbm_pose_params& P, float x, float y, float z, float* u, float* v)
{
    const float invz = (float)(1.0 / (double)z);
    const float xn = x * invz, yn = y * invz;
    *u = __builtin_fmaf(P.fx, xn, P.cx);
    *v = __builtin_fmaf(P.fy, yn, P.cy);
}

// ---- setup: the constructor ----
struct S3Tables {
    const orbx_keypoint* kps;
    const int* counts;
    int nkf, cap;
    const float* pose;
    const int* kf_mp;
    const orbm_map_point* pts;
    int nmp;
    const int* obs_ptr;
    const orbm_observation* obs;
    const uint8_t* erased;
    orbm_pose_params P;
};

enum { kS3Skip = 0, kS3Keep = 1, kS3Bad = 2 };

// MapPoint::GetIndexInKeyFrame: the idx of the live observation in KeyFrame kf (n features), -1 none, -2 where the
// list descends or the idx is outside the KeyFrame
ORBX_HD int s3_index_in_kf(const S3Tables& T, int mp, int kf, int n)
{
    const int b = T.obs_ptr[mp], e = T.obs_ptr[mp + 1];
    if (b < 0 || e < b) return -2;
    for (int k = b; k < e; ++k) {
        if (T.erased && T.erased[k]) continue;
        const orbm_observation o = T.obs[k];
        if (o.kf == kf) return (o.idx < 0 || o.idx >= n) ? -2 : o.idx;
    }
    return -1;
}

struct S3Pair {
    int idx2;
    float X1[3], X2[3], P1[2], P2[2], E1, E2;
};

// :64-101 for one i1 < na; every range check in front of the read it guards
ORBX_HD int s3_pair(const S3Tables& T, const int* match12, int a, int b, int na, int nb, int i1, S3Pair* o)
{
    const int idx2 = match12[i1];
    if (idx2 < -1 || idx2 >= nb) return kS3Bad;
    const int mp1 = T.kf_mp[(size_t)a * T.cap + i1];
    if (mp1 < -1 || mp1 >= T.nmp) return kS3Bad;
    if (idx2 < 0) return kS3Skip;                                  // !vpMatched12[i1]
    const int mp2 = T.kf_mp[(size_t)b * T.cap + idx2];
    if (mp2 < -1 || mp2 >= T.nmp) return kS3Bad;
    if (mp2 < 0 || mp1 < 0) return kS3Skip;                        // !pMP1
    const orbm_map_point M1 = T.pts[mp1], M2 = T.pts[mp2];
    if (!(M1.flags & 1) || !(M2.flags & 1)) return kS3Skip;        // isBad()
    const int k1 = s3_index_in_kf(T, mp1, a, na), k2 = s3_index_in_kf(T, mp2, b, nb);
    if (k1 == -2 || k2 == -2) return kS3Bad;
    if (k1 < 0 || k2 < 0) return kS3Skip;
    const int o1 = T.kps[(size_t)a * T.cap + k1].octave, o2 = T.kps[(size_t)b * T.cap + k2].octave;
    if ((unsigned)o1 >= (unsigned)T.P.nlevels || (unsigned)o2 >= (unsigned)T.P.nlevels) return kS3Bad;
    const float s1 = T.P.scale[o1] * T.P.scale[o1], s2 = T.P.scale[o2] * T.P.scale[o2];   // mvLevelSigma2
    o->E1 = (float)(unsigned long long)(9.210 * (double)s1);       // vector<size_t>::push_back(9.210*sigmaSquare1)
    o->E2 = (float)(unsigned long long)(9.210 * (double)s2);
    const float* Ta = T.pose + (size_t)a * 12;
    const float* Tb = T.pose + (size_t)b * 12;
    for (int r = 0; r < 3; ++r) {
        o->X1[r] = s3_row(Ta + 4 * r, M1.x, M1.y, M1.z) + Ta[4 * r + 3];
        o->X2[r] = s3_row(Tb + 4 * r, M2.x, M2.y, M2.z) + Tb[4 * r + 3];
    }
    s3_to_image(T.P, o->X1[0], o->X1[1], o->X1[2], &o->P1[0], &o->P1[1]);
    s3_to_image(T.P, o->X2[0], o->X2[1], o->X2[2], &o->P2[0], &o->P2[1]);
    o->idx2 = k2;
    return kS3Keep;
}

template <int NT>
ORBX_HD void s3_setup(S3Shared<NT>& S, const S3Tables& T, int a, int b, const int* match12, const int* maxits,
                      const S3Solver& W, int* n_out, int* iterations, int* best, int* status)
{
    const int tid = s3_tid();
    bool ok = (unsigned)a < (unsigned)T.nkf && (unsigned)b < (unsigned)T.nkf;
    int na = 0, nb = 0;
    if (ok) {
        na = T.counts[a];
        nb = T.counts[b];
        ok = na >= 0 && na <= T.cap && nb >= 0 && nb <= T.cap;
    }
    if (tid == 0) S.bad = 0;
    s3_sync();
    if (ok) {
        int bad = 0;
        S3Pair p;
        for (int i1 = tid; i1 < na; i1 += NT)
            if (s3_pair(T, match12, a, b, na, nb, i1, &p) == kS3Bad) bad = 1;
        if (bad) S.bad = 1;   // every writer stores the same value
    }
    s3_sync();
    if (!ok || S.bad) {   // of an invalid solver only the status is written (and the workspace's own mark)
        if (tid == 0) {
            W.hdr[0] = 0;
            W.hdr[1] = 0;
            W.hdr[2] = 0;
            *status = ORBM_SIM3_INVALID;
        }
        return;
    }
    int n = 0;
    for (int c = 0; c < na; c += NT) {
        const int i1 = c + tid;
        S3Pair p;
        const bool keep = i1 < na && s3_pair(T, match12, a, b, na, nb, i1, &p) == kS3Keep;
        int total;
        const int k = n + s3_rank(S, keep, &total);
        if (keep) {
            W.idx1[k] = i1;
            W.idx2[k] = p.idx2;
            for (int r = 0; r < 3; ++r) {
                W.X1[3 * k + r] = p.X1[r];
                W.X2[3 * k + r] = p.X2[r];
            }
            W.P1[2 * k] = p.P1[0];
            W.P1[2 * k + 1] = p.P1[1];
            W.P2[2 * k] = p.P2[0];
            W.P2[2 * k + 1] = p.P2[1];
            W.E1[k] = p.E1;
            W.E2[k] = p.E2;
        }
        n += total;
        s3_sync();   // wave_n is rewritten by the next chunk
    }
    if (tid == 0) {
        W.hdr[0] = n;
        W.hdr[1] = 1;
        W.hdr[2] = maxits[n];   // SetRansacParameters: mRansacMaxIts for N = n
        *n_out = n;
        *iterations = 0;
        *best = 0;
        *status = 0;
    }
}

// ---- one hypothesis ----

// DUtils::Random::RandomInt(0, size - 1) three times with the swap-with-back removal of :163-177 on mvAllIndices =
// 0 .. n-1, n >= 3, without the list: after the first removal position pos0 holds n-1, after the second position
// pos1 holds what position n-2 held
ORBX_HD void s3_triplet(int n, const int* r, int* out)
{
    int pos[3];
    for (int i = 0; i < 3; ++i)
        pos[i] = (int)(((double)(r[i] & 0x7fffffff) / 2147483648.0) * (double)(n - i));
    out[0] = pos[0];
    out[1] = pos[1] == pos[0] ? n - 1 : pos[1];
    const int q = pos[2] == pos[1] ? n - 2 : pos[2];
    out[2] = q == pos[0] ? n - 1 : q;
}

// OpenCV's own hypot of lapack.cpp
ORBX_HD float s3_hypot(float a, float b)
{
    a = __builtin_fabsf(a);
    b = __builtin_fabsf(b);
    if (a > b) {
        b = b / a;
        return a * __builtin_sqrtf(1.0f + b * b);
    }
    if (b > 0.0f) {
        a = a / b;
        return b * __builtin_sqrtf(1.0f + a * a);
    }
    return 0.0f;
}

// cv::eigen of a symmetric 4x4 CV_32F: JacobiImpl_<float> -- W eigenvalues descending, V their vectors as rows
ORBX_HD void s3_jacobi4(float* A, float* W, float* V)
{
    const int n = 4;
    const float eps = FLT_EPSILON;
    int indR[4], indC[4];
    for (int i = 0; i < 16; ++i) V[i] = (i % 5 == 0) ? 1.0f : 0.0f;
    for (int k = 0; k < n; ++k) {
        W[k] = A[5 * k];
        if (k < n - 1) {
            int m = k + 1;
            float mv = __builtin_fabsf(A[n * k + m]);
            for (int i = k + 2; i < n; ++i) {
                const float val = __builtin_fabsf(A[n * k + i]);
                if (mv < val) { mv = val; m = i; }
            }
            indR[k] = m;
        }
        if (k > 0) {
            int m = 0;
            float mv = __builtin_fabsf(A[k]);
            for (int i = 1; i < k; ++i) {
                const float val = __builtin_fabsf(A[n * i + k]);
                if (mv < val) { mv = val; m = i; }
            }
            indC[k] = m;
        }
    }
    for (int iters = 0; iters < 30 * n * n; ++iters) {
        int k = 0;
        float mv = __builtin_fabsf(A[indR[0]]);
        for (int i = 1; i < n - 1; ++i) {
            const float val = __builtin_fabsf(A[n * i + indR[i]]);
            if (mv < val) { mv = val; k = i; }
        }
        int l = indR[k];
        for (int i = 1; i < n; ++i) {
            const float val = __builtin_fabsf(A[n * indC[i] + i]);
            if (mv < val) { mv = val; k = indC[i]; l = i; }
        }
        const float p = A[n * k + l];
        if (__builtin_fabsf(p) <= eps) break;
        const float y = (float)((double)(W[l] - W[k]) * 0.5);
        float t = __builtin_fabsf(y) + s3_hypot(p, y);
        float s = s3_hypot(p, t);
        const float c = t / s;
        s = p / s;
        t = (p / t) * p;
        if (y < 0.0f) {
            s = -s;
            t = -t;
        }
        A[n * k + l] = 0.0f;
        W[k] = W[k] - t;
        W[l] = W[l] + t;
#define S3_ROTATE(v0, v1)            \
    do {                             \
        const float a0 = v0, b0 = v1; \
        v0 = a0 * c - b0 * s;        \
        v1 = a0 * s + b0 * c;        \
    } while (0)
        for (int i = 0; i < k; ++i) S3_ROTATE(A[n * i + k], A[n * i + l]);
        for (int i = k + 1; i < l; ++i) S3_ROTATE(A[n * k + i], A[n * i + l]);
        for (int i = l + 1; i < n; ++i) S3_ROTATE(A[n * k + i], A[n * l + i]);
        for (int i = 0; i < n; ++i) S3_ROTATE(V[n * k + i], V[n * l + i]);
#undef S3_ROTATE
        for (int j = 0; j < 2; ++j) {
            const int idx = j == 0 ? k : l;
            if (idx < n - 1) {
                int m = idx + 1;
                float mx = __builtin_fabsf(A[n * idx + m]);
                for (int i = idx + 2; i < n; ++i) {
                    const float val = __builtin_fabsf(A[n * idx + i]);
                    if (mx < val) { mx = val; m = i; }
                }
                indR[idx] = m;
            }
            if (idx > 0) {
                int m = 0;
                float mx = __builtin_fabsf(A[idx]);
                for (int i = 1; i < idx; ++i) {
                    const float val = __builtin_fabsf(A[n * i + idx]);
                    if (mx < val) { mx = val; m = i; }
                }
                indC[idx] = m;
            }
        }
    }
    for (int k = 0; k < n - 1; ++k) {
        int m = k;
        for (int i = k + 1; i < n; ++i)
            if (W[m] < W[i]) m = i;
        if (k != m) {
            const float w = W[m];
            W[m] = W[k];
            W[k] = w;
            for (int i = 0; i < n; ++i) {
                const float v = V[n * m + i];
                V[n * m + i] = V[n * k + i];
                V[n * k + i] = v;
            }
        }
    }
}

struct S3Model {
    float s, R[9], t[3];   // ms12i, mR12i, mt12i
    float M12[9];          // sR of mT12i (its translation is t)
    float M21[9], t21[3];  // mT21i
};

// ComputeSim3(P1, P2): p1 / p2 hold the three points, point j at [3 * j]
ORBX_HD void s3_compute(const float* p1, const float* p2, bool fix_scale, S3Model* m)
{
    const float third = (float)(1.0 / 3.0);
    float O1[3], O2[3], Pr1[9], Pr2[9];   // row-major 3x3, column j = point j
    for (int r = 0; r < 3; ++r) {
        O1[r] = ((p1[r] + p1[3 + r]) + p1[6 + r]) * third + 0.0f;
        O2[r] = ((p2[r] + p2[3 + r]) + p2[6 + r]) * third + 0.0f;
    }
    for (int r = 0; r < 3; ++r)
        for (int j = 0; j < 3; ++j) {
            Pr1[3 * r + j] = p1[3 * j + r] - O1[r];
            Pr2[3 * r + j] = p2[3 * j + r] - O2[r];
        }
    float M[9];   // Pr2 * Pr1.t()
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            M[3 * i + j] = (Pr2[3 * i] * Pr1[3 * j] + Pr2[3 * i + 1] * Pr1[3 * j + 1]) + Pr2[3 * i + 2] * Pr1[3 * j + 2];
    const float N11 = (M[0] + M[4]) + M[8], N12 = M[5] - M[7], N13 = M[6] - M[2], N14 = M[1] - M[3];
    const float N22 = (M[0] - M[4]) - M[8], N23 = M[1] + M[3], N24 = M[6] + M[2];
    const float N33 = (-M[0] + M[4]) - M[8], N34 = M[5] + M[7], N44 = (-M[0] - M[4]) + M[8];
    float A[16] = {N11, N12, N13, N14, N12, N22, N23, N24, N13, N23, N33, N34, N14, N24, N34, N44};
    float W[4], V[16];
    s3_jacobi4(A, W, V);
    // evec.row(0): the quaternion; ang = atan2(norm(vec), q0); vec = 2*ang*vec/norm(vec)
    double nn = 0.0;
    nn += (double)V[1] * (double)V[1];
    nn += (double)V[2] * (double)V[2];
    nn += (double)V[3] * (double)V[3];
    const double nrm = __builtin_sqrt(nn);
    const double ang = fixed_atan2(nrm, (double)V[0]);
    const float alpha = (float)((2.0 * ang) / nrm);
    const float rv[3] = {V[1] * alpha + 0.0f, V[2] * alpha + 0.0f, V[3] * alpha + 0.0f};
    // cv::Rodrigues
    double rx = (double)rv[0], ry = (double)rv[1], rz = (double)rv[2];
    const double theta = __builtin_sqrt((rx * rx + ry * ry) + rz * rz);
    if (theta < DBL_EPSILON) {
        for (int i = 0; i < 9; ++i) m->R[i] = (i % 4 == 0) ? 1.0f : 0.0f;
    } else {
        double sn, cs, th3;
        po_sincos_theta3(theta, &sn, &cs, &th3);
        const double c1 = 1.0 - cs, itheta = 1.0 / theta;
        rx = rx * itheta;
        ry = ry * itheta;
        rz = rz * itheta;
        const double rrt[9] = {rx * rx, rx * ry, rx * rz, rx * ry, ry * ry, ry * rz, rx * rz, ry * rz, rz * rz};
        const double rc[9] = {0.0, -rz, ry, rz, 0.0, -rx, -ry, rx, 0.0};
        for (int i = 0; i < 9; ++i) {
            const double id = (i % 4 == 0) ? 1.0 : 0.0;
            m->R[i] = (float)((cs * id + c1 * rrt[i]) + sn * rc[i]);
        }
    }
    const float* R = m->R;
    float P3[9];   // mR12i * Pr2
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            P3[3 * i + j] = (R[3 * i] * Pr2[j] + R[3 * i + 1] * Pr2[3 + j]) + R[3 * i + 2] * Pr2[6 + j];
    if (!fix_scale) {
        // Pr1.dot(P3): dotProd_'s groups of four, then the tail
        double nom = 0.0;
        for (int i = 0; i < 8; i += 4)
            nom += (((double)Pr1[i] * (double)P3[i] + (double)Pr1[i + 1] * (double)P3[i + 1]) +
                    (double)Pr1[i + 2] * (double)P3[i + 2]) + (double)Pr1[i + 3] * (double)P3[i + 3];
        nom += (double)Pr1[8] * (double)P3[8];
        double den = 0.0;
        for (int i = 0; i < 9; ++i) den += (double)(P3[i] * P3[i]);   // cv::pow(P3, 2, aux_P3) is a float product
        m->s = (float)(nom / den);
    } else {
        m->s = 1.0f;
    }
    const float s = m->s;
    for (int r = 0; r < 3; ++r)   // O1 - ms12i*mR12i*O2: gemm with alpha = -s, beta = 1 in double
        m->t[r] = (float)((double)s3_row(R + 3 * r, O2[0], O2[1], O2[2]) * (-(double)s) + (double)O1[r]);
    const float sinv = (float)(1.0 / (double)s);
    for (int r = 0; r < 3; ++r) {
        for (int k = 0; k < 3; ++k) {
            m->M12[3 * r + k] = R[3 * r + k] * s + 0.0f;
            m->M21[3 * r + k] = R[3 * k + r] * sinv + 0.0f;
        }
        m->t21[r] = -s3_row(m->M21 + 3 * r, m->t[0], m->t[1], m->t[2]);
    }
}

// CheckInliers for pair i
ORBX_HD bool s3_inlier(const S3Solver& W, const S3Model& m, const orbm_pose_params& P, int i)
{
    const float* X1 = W.X1 + 3 * (size_t)i;
    const float* X2 = W.X2 + 3 * (size_t)i;
    float c[3], u, v;
    for (int r = 0; r < 3; ++r) c[r] = s3_row(m.M12 + 3 * r, X2[0], X2[1], X2[2]) + m.t[r];   // Project(mvX3Dc2, mT12i)
    s3_to_image(P, c[0], c[1], c[2], &u, &v);
    const float d1x = W.P1[2 * (size_t)i] - u, d1y = W.P1[2 * (size_t)i + 1] - v;
    for (int r = 0; r < 3; ++r) c[r] = s3_row(m.M21 + 3 * r, X1[0], X1[1], X1[2]) + m.t21[r];   // Project(mvX3Dc1, mT21i)
    s3_to_image(P, c[0], c[1], c[2], &u, &v);
    const float d2x = u - W.P2[2 * (size_t)i], d2y = v - W.P2[2 * (size_t)i + 1];
    double e1 = 0.0, e2 = 0.0;
    e1 += (double)d1x * (double)d1x;
    e1 += (double)d1y * (double)d1y;
    e2 += (double)d2x * (double)d2x;
    e2 += (double)d2y * (double)d2y;
    const float err1 = (float)e1, err2 = (float)e2;
    return err1 < W.E1[i] && err2 < W.E2[i];
}

// iteration k of one iterate() call, as an independent hypothesis (one wave64, or one lane on the CPU)
ORBX_HD void s3_hypothesis(const S3Solver& W, const S3Hyp& H, const orbm_pose_params& P, int cap, bool fix_scale,
                           int min_inliers, int k, const int* draws, int iterations)
{
    const int N = W.hdr[0];
    if (W.hdr[1] != 1 || N < min_inliers || N > cap) return;   // N > cap: a workspace that was never set up
    if (iterations < 0 || iterations + k >= W.hdr[2]) return;   // past mRansacMaxIts: never looked at
    int tri[3];
    s3_triplet(N, draws, tri);
    float p1[9], p2[9];
    for (int j = 0; j < 3; ++j)
        for (int r = 0; r < 3; ++r) {
            p1[3 * j + r] = W.X1[3 * (size_t)tri[j] + r];
            p2[3 * j + r] = W.X2[3 * (size_t)tri[j] + r];
        }
    S3Model m;
    s3_compute(p1, p2, fix_scale, &m);
    int cnt = 0;
#if defined(__HIP_DEVICE_COMPILE__)
    const int lane = threadIdx.x;
    for (int base = 0; base < N; base += 64) {
        const int i = base + lane;
        const bool in = i < N && s3_inlier(W, m, P, i);
        const unsigned long long b = __ballot(in);
        if (lane == 0) H.words[base >> 6] = b;
        cnt += __popcll(b);
    }
    if (lane != 0) return;
#else
    for (int base = 0; base < N; base += 64) {
        unsigned long long b = 0;
        for (int j = 0; j < 64 && base + j < N; ++j)
            if (s3_inlier(W, m, P, base + j)) b |= 1ull << j;
        H.words[base >> 6] = b;
        cnt += __builtin_popcountll(b);
    }
#endif
    H.sim3[0] = m.s;
    for (int i = 0; i < 9; ++i) H.sim3[1 + i] = m.R[i];
    for (int i = 0; i < 3; ++i) H.sim3[10 + i] = m.t[i];
    *H.inl = cnt;
}

// ---- the sequential rule of iterate() over the call's hypotheses, and the masks ----
struct S3Out {
    int *iterations, *best;
    float* sim3;
    uint8_t *inliers12, *already2;
    int *ninliers, *nomore, *used;
};

template <int NT>
ORBX_HD void s3_select(S3Shared<NT>& S, const S3Solver& W, void* work, const S3Layout& L, size_t hyp0, int cap,
                       int min_inliers, int nit, const S3Out& O)
{
    const int tid = s3_tid();
    const int N = W.hdr[0];
    if (tid == 0) {
        int pick = -1, nomore = 0, used = 0, ninl = 0;
        if (W.hdr[1] != 1 || N < min_inliers || N > cap || *O.iterations < 0) {
            // bNoMore and nothing else; an invalid solver has no result either, nor has one whose state is
            // negative: k_sim3_hyp computed nothing for it
            nomore = 1;
        } else {
            const int maxits = W.hdr[2];
            int it = *O.iterations, best = *O.best;
            while (it < maxits && used < nit) {
                const int inl = *s3_hyp(work, L, hyp0 + (size_t)used).inl;
                ++used;
                ++it;
                if (inl >= best) {
                    best = inl;
                    if (inl > min_inliers) {
                        pick = used - 1;
                        ninl = inl;
                        break;
                    }
                }
            }
            if (pick < 0 && it >= maxits) nomore = 1;
            *O.iterations = it;
            *O.best = best;
        }
        S.pick = pick;
        const float* src = pick >= 0 ? s3_hyp(work, L, hyp0 + (size_t)pick).sim3 : nullptr;
        for (int i = 0; i < 13; ++i) O.sim3[i] = src ? src[i] : 0.0f;
        *O.ninliers = ninl;
        *O.nomore = nomore;
        *O.used = used;
    }
    for (int i = tid; i < cap; i += NT) {
        O.inliers12[i] = 0;
        O.already2[i] = 0;
    }
    s3_sync();
    const int pick = S.pick;
    if (pick < 0) return;
    const unsigned long long* words = s3_hyp(work, L, hyp0 + (size_t)pick).words;
    for (int j = tid; j < N; j += NT)
        if ((words[j >> 6] >> (j & 63)) & 1ull) {
            const int i1 = W.idx1[j], i2 = W.idx2[j];   // below cap in a workspace that setup wrote
            if ((unsigned)i1 < (unsigned)cap) O.inliers12[i1] = 1;   // vbInliers[mvnIndices1[i]]
            if ((unsigned)i2 < (unsigned)cap) O.already2[i2] = 1;    // SearchBySim3 :1206-1208 on the inlier's MapPoint
        }
}

// ---- kernels ----
__global__ __launch_bounds__(kS3Lanes) void k_sim3_setup(S3Tables T, const int* __restrict__ pair_a,
                                                         const int* __restrict__ pair_b,
                                                         const int* __restrict__ match12, int match_stride,
                                                         const int* __restrict__ maxits, void* work, S3Layout L,
                                                         int* n_out, int* iterations, int* best, int* status)
{
    __shared__ S3Shared<kS3Lanes> S;
    const int s = blockIdx.x;
    s3_setup<kS3Lanes>(S, T, pair_a[s], pair_b[s], match12 + (size_t)s * match_stride, maxits,
                       s3_solver(work, L, s, T.cap), n_out + s, iterations + s, best + s, status + s);
}

__global__ __launch_bounds__(64) void k_sim3_hyp(void* work, S3Layout L, int cap, orbm_pose_params P, int fix_scale,
                                                 int min_inliers, int nit, const int* __restrict__ rand,
                                                 const int* __restrict__ rand_off,
                                                 const int* __restrict__ iterations)
{
    const int k = blockIdx.x, s = blockIdx.y;
    s3_hypothesis(s3_solver(work, L, s, cap), s3_hyp(work, L, (size_t)s * nit + k), P, cap, fix_scale != 0,
                  min_inliers, k, rand + rand_off[s] + 3 * k, iterations[s]);
}

__global__ __launch_bounds__(kS3Lanes) void k_sim3_select(void* work, S3Layout L, int cap, int min_inliers, int nit,
                                                          int* iterations, int* best, float* sim3, uint8_t* inliers12,
                                                          uint8_t* already2, int* ninliers, int* nomore, int* used)
{
    __shared__ S3Shared<kS3Lanes> S;
    const int s = blockIdx.x;
    const S3Out O = {iterations + s, best + s, sim3 + (size_t)s * 13, inliers12 + (size_t)s * cap,
                     already2 + (size_t)s * cap, ninliers + s, nomore + s, used + s};
    s3_select<kS3Lanes>(S, s3_solver(work, L, s, cap), work, L, (size_t)s * nit, cap, min_inliers, nit, O);
}

}  // namespace orbx

using namespace orbx;

extern "C" {

double orbx_fixed_atan2(double y, double x) { return fixed_atan2(y, x); }

void orbx_sim3_triplet(int n, const int* r, int* out3)
{
    if (n >= 3 && r && out3) s3_triplet(n, r, out3);
}

size_t orbm_sim3_workspace_bytes(int nsolvers, int cap, int max_iters_per_call)
{
    if (nsolvers < 0 || nsolvers > kS3MaxGrid || cap < 1 || cap > ORBM_MAX_FEATURES || max_iters_per_call < 1 ||
        max_iters_per_call > kS3MaxGrid)
        return 0;
    return s3_layout(nsolvers, cap, max_iters_per_call).total;
}

int orbm_sim3_ransac_iterations(int n, double probability, int min_inliers, int max_iterations)
{
    const float epsilon = (float)min_inliers / n;
    int nIterations;
    if (min_inliers == n) {
        nIterations = 1;
    } else {
        const double v = ceil(log(1 - probability) / log(1 - pow(epsilon, 3)));
        nIterations = (v >= -2147483648.0 && v < 2147483648.0) ? (int)v : INT_MIN;
    }
    const int lo = nIterations < max_iterations ? nIterations : max_iterations;
    return lo > 1 ? lo : 1;
}

static bool s3_params_ok(const orbm_pose_params* P) { return P && P->nlevels >= 1 && P->nlevels <= 16; }

orbx_status orbm_sim3_setup_device(const orbx_keypoint* d_kps, const int* d_counts, int nkf, int cap,
                                   const float* d_pose, const int* d_kf_mp, const orbm_map_point* d_pts, int nmp,
                                   const int* d_obs_ptr, const orbm_observation* d_obs, const uint8_t* d_obs_erased,
                                   const int* d_pair_a, const int* d_pair_b, int nsolvers, const int* d_match12,
                                   int match_stride, const orbm_pose_params* params, const int* d_maxits,
                                   void* d_work, size_t work_bytes, int* d_n, int* d_iterations, int* d_best_inliers,
                                   int* d_status, void* stream)
{
    const uintptr_t a4 = (uintptr_t)d_kps | (uintptr_t)d_counts | (uintptr_t)d_pose | (uintptr_t)d_kf_mp |
                         (uintptr_t)d_pts | (uintptr_t)d_obs_ptr | (uintptr_t)d_obs | (uintptr_t)d_pair_a |
                         (uintptr_t)d_pair_b | (uintptr_t)d_match12 | (uintptr_t)d_maxits | (uintptr_t)d_n |
                         (uintptr_t)d_iterations | (uintptr_t)d_best_inliers | (uintptr_t)d_status;
    if (!d_kps || !d_counts || nkf < 0 || cap < 1 || cap > ORBM_MAX_FEATURES || !d_pose || !d_kf_mp || nmp < 0 ||
        (nmp > 0 && (!d_pts || !d_obs_ptr)) || !d_pair_a || !d_pair_b || nsolvers < 0 || nsolvers > kS3MaxGrid ||
        !d_match12 ||
        match_stride < cap || !s3_params_ok(params) || !d_maxits || !d_work || !d_n || !d_iterations ||
        !d_best_inliers || !d_status || (a4 & 3) || ((uintptr_t)d_work & 15) ||
        work_bytes < s3_layout(nsolvers, cap, 1).total)
        return ORBX_EINVAL;
    if (nsolvers == 0) return ORBX_OK;
    const S3Tables T = {d_kps, d_counts, nkf, cap, d_pose, d_kf_mp, d_pts, nmp, d_obs_ptr, d_obs, d_obs_erased, *params};
    // the solver part of the layout does not depend on the iterations per call
    hipLaunchKernelGGL(k_sim3_setup, dim3((unsigned)nsolvers), dim3(kS3Lanes), 0, (hipStream_t)stream, T, d_pair_a,
                       d_pair_b, d_match12, match_stride, d_maxits, d_work, s3_layout(nsolvers, cap, 1), d_n,
                       d_iterations, d_best_inliers, d_status);
    return hipGetLastError() == hipSuccess ? ORBX_OK : ORBX_EDEVICE;
}

orbx_status orbm_sim3_iterate_device(void* d_work, size_t work_bytes, int nsolvers, int cap,
                                     const orbm_pose_params* params, int fix_scale, int min_inliers, int nit,
                                     const int* d_rand, const int* d_rand_off, int* d_iterations, int* d_best_inliers,
                                     float* d_sim3, uint8_t* d_inliers12, uint8_t* d_already2, int* d_ninliers,
                                     int* d_nomore, int* d_used, void* stream)
{
    const uintptr_t a4 = (uintptr_t)d_rand | (uintptr_t)d_rand_off | (uintptr_t)d_iterations |
                         (uintptr_t)d_best_inliers | (uintptr_t)d_sim3 | (uintptr_t)d_ninliers | (uintptr_t)d_nomore |
                         (uintptr_t)d_used;
    if (!d_work || nsolvers < 0 || nsolvers > kS3MaxGrid || cap < 1 || cap > ORBM_MAX_FEATURES || !s3_params_ok(params) || min_inliers < 3 ||
        nit < 1 || nit > kS3MaxGrid || !d_rand || !d_rand_off || !d_iterations || !d_best_inliers || !d_sim3 ||
        !d_inliers12 || !d_already2 || !d_ninliers || !d_nomore || !d_used || (a4 & 3) || ((uintptr_t)d_work & 15) ||
        work_bytes < s3_layout(nsolvers, cap, nit).total)
        return ORBX_EINVAL;
    if (nsolvers == 0) return ORBX_OK;
    const S3Layout L = s3_layout(nsolvers, cap, nit);
    hipLaunchKernelGGL(k_sim3_hyp, dim3((unsigned)nit, (unsigned)nsolvers), dim3(64), 0, (hipStream_t)stream, d_work, L,
                       cap, *params, fix_scale, min_inliers, nit, d_rand, d_rand_off, d_iterations);
    hipLaunchKernelGGL(k_sim3_select, dim3((unsigned)nsolvers), dim3(kS3Lanes), 0, (hipStream_t)stream, d_work, L, cap,
                       min_inliers, nit, d_iterations, d_best_inliers, d_sim3, d_inliers12, d_already2, d_ninliers,
                       d_nomore, d_used);
    return hipGetLastError() == hipSuccess ? ORBX_OK : ORBX_EDEVICE;
}

// the one-pair forms: a table of two KeyFrames (slots 0 and 1) at stride cap
struct S3One {
    int cap = 0, nobs = 0;
    std::vector<int> maxits;
};

static bool s3_one_args_ok(const orbx_keypoint* kps1, const int* kf_mp1, int n1, const float* T1w,
                           const orbx_keypoint* kps2, const int* kf_mp2, int n2, const float* T2w,
                           const orbm_map_point* pts, int nmp, const int* obs_ptr, const orbm_observation* obs,
                           const int* match12, const orbm_pose_params* params, int min_inliers, int max_iterations,
                           int nit, const int* rand, const int* iterations, const int* best_inliers, const int* n,
                           const float* sim3, const uint8_t* inliers12, const uint8_t* already2, const int* ninliers,
                           const int* nomore, const int* used, const int* status, S3One* one)
{
    const uintptr_t a4 = (uintptr_t)kps1 | (uintptr_t)kf_mp1 | (uintptr_t)T1w | (uintptr_t)kps2 | (uintptr_t)kf_mp2 |
                         (uintptr_t)T2w | (uintptr_t)pts | (uintptr_t)obs_ptr | (uintptr_t)obs | (uintptr_t)match12 |
                         (uintptr_t)rand | (uintptr_t)iterations | (uintptr_t)best_inliers | (uintptr_t)n |
                         (uintptr_t)sim3 | (uintptr_t)ninliers | (uintptr_t)nomore | (uintptr_t)used |
                         (uintptr_t)status;
    if (n1 < 0 || n1 > ORBM_MAX_FEATURES || n2 < 0 || n2 > ORBM_MAX_FEATURES || (n1 > 0 && (!kps1 || !kf_mp1)) ||
        (n2 > 0 && (!kps2 || !kf_mp2)) || (n1 > 0 && (!match12 || !inliers12)) || (n2 > 0 && !already2) || !T1w ||
        !T2w || nmp < 0 || (nmp > 0 && (!pts || !obs_ptr)) || !s3_params_ok(params) || min_inliers < 3 ||
        max_iterations < 1 || nit < 1 || nit > kS3MaxGrid || !rand || !iterations || !best_inliers || !n || !sim3 ||
        !ninliers || !nomore || !used || !status || (a4 & 3))
        return false;
    one->nobs = 0;
    if (nmp > 0) {
        if (obs_ptr[0] < 0) return false;
        for (int m = 0; m < nmp; ++m)
            if (obs_ptr[m + 1] < obs_ptr[m]) return false;
        one->nobs = obs_ptr[nmp];
        if (one->nobs > 0 && !obs) return false;
    }
    one->cap = n1 > n2 ? n1 : n2;
    if (one->cap < 1) one->cap = 1;
    return true;
}

static void s3_fill_maxits(S3One* one, double probability, int min_inliers, int max_iterations)
{
    one->maxits.resize((size_t)one->cap + 1);
    for (int k = 0; k <= one->cap; ++k)
        one->maxits[(size_t)k] = orbm_sim3_ransac_iterations(k, probability, min_inliers, max_iterations);
}

orbx_status orbm_sim3_solve_host(const orbx_keypoint* kps1, const int* kf_mp1, int n1, const float* T1w,
                                 const orbx_keypoint* kps2, const int* kf_mp2, int n2, const float* T2w,
                                 const orbm_map_point* pts, int nmp, const int* obs_ptr, const orbm_observation* obs,
                                 const uint8_t* obs_erased, const int* match12, const orbm_pose_params* params,
                                 int fix_scale, double probability, int min_inliers, int max_iterations, int nit,
                                 const int* rand, int* iterations, int* best_inliers, int* n, float* sim3,
                                 uint8_t* inliers12, uint8_t* already2, int* ninliers, int* nomore, int* used,
                                 int* status)
{
    S3One one;
    if (!s3_one_args_ok(kps1, kf_mp1, n1, T1w, kps2, kf_mp2, n2, T2w, pts, nmp, obs_ptr, obs, match12, params,
                        min_inliers, max_iterations, nit, rand, iterations, best_inliers, n, sim3, inliers12, already2,
                        ninliers, nomore, used, status, &one))
        return ORBX_EINVAL;
    s3_fill_maxits(&one, probability, min_inliers, max_iterations);
    const int cap = one.cap;
    std::vector<orbx_keypoint> kps((size_t)2 * cap);
    std::vector<int> kf_mp((size_t)2 * cap, -1), m12((size_t)cap, -1);
    float pose[24];
    const int counts[2] = {n1, n2};
    if (n1) {
        std::memcpy(kps.data(), kps1, sizeof(orbx_keypoint) * (size_t)n1);
        std::memcpy(kf_mp.data(), kf_mp1, sizeof(int) * (size_t)n1);
        std::memcpy(m12.data(), match12, sizeof(int) * (size_t)n1);
    }
    if (n2) {
        std::memcpy(kps.data() + cap, kps2, sizeof(orbx_keypoint) * (size_t)n2);
        std::memcpy(kf_mp.data() + cap, kf_mp2, sizeof(int) * (size_t)n2);
    }
    std::memcpy(pose, T1w, sizeof(float) * 12);
    std::memcpy(pose + 12, T2w, sizeof(float) * 12);
    const S3Layout L = s3_layout(1, cap, nit);
    std::vector<unsigned long long> work(L.total / 8 + 2);
    void* w = work.data();   // operator new aligns to 16
    const S3Tables T = {kps.data(), counts, 2, cap, pose, kf_mp.data(), pts, nmp, obs_ptr, obs, obs_erased, *params};
    const S3Solver W = s3_solver(w, L, 0, cap);
    S3Shared<1> S;
    int st = 0, nn = 0, it0 = 0, best0 = 0;
    s3_setup<1>(S, T, 0, 1, m12.data(), one.maxits.data(), W, &nn, &it0, &best0, &st);
    *status = st;
    if (st) return ORBX_OK;
    for (int k = 0; k < nit; ++k)
        s3_hypothesis(W, s3_hyp(w, L, (size_t)k), *params, cap, fix_scale != 0, min_inliers, k, rand + 3 * k,
                      *iterations);
    std::vector<uint8_t> in12((size_t)cap), al2((size_t)cap);
    const S3Out O = {iterations, best_inliers, sim3, in12.data(), al2.data(), ninliers, nomore, used};
    s3_select<1>(S, W, w, L, 0, cap, min_inliers, nit, O);
    *n = nn;
    if (n1) std::memcpy(inliers12, in12.data(), (size_t)n1);
    if (n2) std::memcpy(already2, al2.data(), (size_t)n2);
    return ORBX_OK;
}

orbx_status orbm_sim3_solve(int device, const orbx_keypoint* kps1, const int* kf_mp1, int n1, const float* T1w,
                            const orbx_keypoint* kps2, const int* kf_mp2, int n2, const float* T2w,
                            const orbm_map_point* pts, int nmp, const int* obs_ptr, const orbm_observation* obs,
                            const uint8_t* obs_erased, const int* match12, const orbm_pose_params* params,
                            int fix_scale, double probability, int min_inliers, int max_iterations, int nit,
                            const int* rand, int* iterations, int* best_inliers, int* n, float* sim3,
                            uint8_t* inliers12, uint8_t* already2, int* ninliers, int* nomore, int* used, int* status)
{
    S3One one;
    if (!s3_one_args_ok(kps1, kf_mp1, n1, T1w, kps2, kf_mp2, n2, T2w, pts, nmp, obs_ptr, obs, match12, params,
                        min_inliers, max_iterations, nit, rand, iterations, best_inliers, n, sim3, inliers12, already2,
                        ninliers, nomore, used, status, &one))
        return ORBX_EINVAL;
    s3_fill_maxits(&one, probability, min_inliers, max_iterations);
    const int cap = one.cap, nobs = one.nobs;
    const S3Layout L = s3_layout(1, cap, nit);
    const size_t C = (size_t)cap, m1 = (size_t)n1, m2 = (size_t)n2;
    const int head[8] = {n1, n2, 0, 1, 0, *iterations, *best_inliers, 0};   // counts, pair, rand_off, state, pad
    struct Res {
        int n, status, ninliers, nomore, used, s0, s1, pad;   // s0, s1: scratch
        float sim3[16];
    } r;
    HostCall c(device);
    const auto okp = c.stage<orbx_keypoint>(2 * C);
    const auto omp = c.stage<int>(2 * C);
    const auto om12 = c.stage<int>(C);
    const auto ohd = c.in(head, 8);
    const auto opo = c.stage<float>(24);
    const auto omx = c.in(one.maxits.data(), C + 1);
    const auto ord = c.in(rand, (size_t)3 * nit);
    const auto opt = c.in(pts, (size_t)nmp);
    const auto oop = c.in(nmp ? obs_ptr : nullptr, (size_t)nmp + 1);
    const auto oob = c.in(obs, (size_t)nobs);
    const auto oer = c.in(obs_erased, (size_t)nobs);
    const auto ores = c.out<Res>(1);
    const auto oin = c.out<uint8_t>(C);
    const auto oal = c.out<uint8_t>(C);
    const auto owk = c.out<uint8_t>(L.total);
    orbx_status rc = c.prepare();
    if (rc != ORBX_OK) return rc;
    pack_pair(c.host(okp), C, kps1, m1, kps2, m2);
    pack_pair(c.host(omp), C, kf_mp1, m1, kf_mp2, m2, 0xFF);
    std::fill_n(std::copy_n(match12, m1, c.host(om12)), C - m1, -1);
    pack_pair(c.host(opo), 12, T1w, 12, T2w, 12);
    rc = c.upload();
    if (rc != ORBX_OK) return rc;
    Res* const d = c.dev(ores);
    // the constructor's own zero state goes to the two scratch words; iterate starts from the caller's state
    rc = orbm_sim3_setup_device(c.dev(okp), c.dev(ohd), 2, cap, c.dev(opo), c.dev(omp), nmp ? c.dev(opt) : nullptr,
                                nmp, nmp ? c.dev(oop) : nullptr, c.dev(oob),
                                nobs && obs_erased ? c.dev(oer) : nullptr, c.dev(ohd, 2), c.dev(ohd, 3), 1,
                                c.dev(om12), cap, params, c.dev(omx), c.dev(owk), L.total, &d->n, &d->s0, &d->s1,
                                &d->status, c.stream());
    if (rc != ORBX_OK) return rc;
    rc = orbm_sim3_iterate_device(c.dev(owk), L.total, 1, cap, params, fix_scale, min_inliers, nit, c.dev(ord),
                                  c.dev(ohd, 4), c.dev(ohd, 5), c.dev(ohd, 6), d->sim3, c.dev(oin), c.dev(oal),
                                  &d->ninliers, &d->nomore, &d->used, c.stream());
    if (rc != ORBX_OK) return rc;
    int state[2];
    std::vector<uint8_t> in12(C), al2(C);
    c.fetch(ores, &r, 1);
    c.fetch(ohd, state, 2, 5);
    c.fetch(oin, in12.data(), C);
    c.fetch(oal, al2.data(), C);
    rc = c.finish();
    if (rc != ORBX_OK) return rc;
    *status = r.status;
    if (r.status) return ORBX_OK;   // of an invalid solver only the status is written
    *n = r.n;
    *iterations = state[0];
    *best_inliers = state[1];
    std::memcpy(sim3, r.sim3, sizeof(float) * 13);
    *ninliers = r.ninliers;
    *nomore = r.nomore;
    *used = r.used;
    if (n1) std::memcpy(inliers12, in12.data(), (size_t)n1);
    if (n2) std::memcpy(already2, al2.data(), (size_t)n2);
    return ORBX_OK;
}

}  // extern "C"

// PnPsolver (src/PnPsolver.cc, include/PnPsolver.h): the EPnP RANSAC of Tracking::Relocalization
// (src/Tracking.cc:1393-1554) between SearchByBoW(KF, F) and Optimizer::PoseOptimization.  Kernels and C entry points
// (include/orbx.h).  The arithmetic order of everything below is DESIGN.md §3 "PnP solver arithmetic": EPnP in double
// in the reference's operation order, cvMulTransposed as OpenCV 3.x's non-gemm path with completeSymm, cvSVD /
// cvInvert(CV_SVD) / cvSolve(CV_SVD) as JacobiSVDImpl_<double> (DBL_EPSILON * 10, DBL_MIN, its sort and its basis
// completion) and SVBkSb.  Parity with a real OpenCV is unpinned; the Python restatement of tests/test_pnp_solver.py,
// this code compiled for the CPU (orbm_pnp_solve_host) and the gfx950 code agree bit for bit.
//
// k_pnp_setup: one workgroup of 256 lanes per solver, the constructor (:67-110) and SetRansacParameters (:121-157):
//   every lane takes one frame feature of a 256-feature chunk, decides whether its match survives (a MapPoint, not
//   bad) and survivors are stored at their rank in feature order (ballot prefix), so the compacted arrays are the
//   reference's vectors.
// k_pnp_hyp: one lane per (iteration, solver).  RandomInt and the removal pick the four points, compute_pose runs on
//   private arrays (the 12x12 double Jacobi rows are runtime-indexed, so in scratch, 1.2 KB a lane), then the lane
//   walks the N points (CheckInliers) and leaves Tcw, the inlier count and the inlier words.
// k_pnp_select: one wave per solver.  Lane 0 walks the hypotheses in iteration order with the reference's rule
//   (:209-237, :241-257); Refine() is a function of the best set alone, so it runs only where the best changes and
//   its outcome stays in the solver between the calls.  The lanes then expand the returned mask into vbInliers and
//   the frame's MapPoint row.
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

constexpr int kPnLanes = 256;
constexpr int kPnHypLanes = 64;
// header: 0 N, 1 valid, 2 mRansacMaxIts, 3 mRansacMinInliers; carried: 8 Refine() of the best, 9 mnRefinedInliers
constexpr int kPnHdrInts = 16;
constexpr int kPnMaxGrid = 65535;  // solvers and iterations per call
constexpr int kPnHypFloats = 16;   // Tcw[12], the inlier count (int), 3 unused
constexpr int kPnCarryOff = 32;    // the part of a solver that iterate() carries from call to call starts here

// ---- workspace: per solver the header, the carried state, the compacted points and Refine's arrays, then per
// (solver, iteration of a call) one hypothesis ----
struct PnLayout {
    size_t solver_bytes, hyp_off, hyp_bytes, total;
    int words;
};

__host__ __device__ inline size_t pn_carry_bytes(int words)
{
    return (size_t)(kPnHdrInts * 4 - kPnCarryOff) + 24 * 4 + (size_t)words * 16;
}

__host__ __device__ inline PnLayout pn_layout(int nsolvers, int cap, int slots)
{
    PnLayout L;
    L.words = (cap + 63) / 64;
    L.solver_bytes = ((size_t)kPnCarryOff + pn_carry_bytes(L.words) + (size_t)cap * 8 * 7 + (size_t)cap * 4 * 9 + 15) &
                     ~(size_t)15;
    L.hyp_off = L.solver_bytes * (size_t)nsolvers;
    L.hyp_bytes = (size_t)kPnHypFloats * 4 + (size_t)L.words * 8;
    L.total = L.hyp_off + L.hyp_bytes * (size_t)nsolvers * (size_t)slots;
    return L;
}

struct PnSolver {
    int* hdr;
    float *best_tcw, *ref_tcw;              // mBestTcw, mRefinedTcw (3x4)
    unsigned long long *best_w, *ref_w;     // mvbBestInliers, mvbRefinedInliers
    double *al, *pc;                        // Refine's alphas and pcs
    float *P3, *P2, *E;                     // mvP3Dw, mvP2D, mvMaxError
    int *kp, *mp, *sel;                     // mvKeyPointIndices, the MapPoint's index, Refine's vIndices
};

ORBX_HD PnSolver pn_solver(void* work, const PnLayout& L, int s, int cap)
{
    uint8_t* b = (uint8_t*)work + L.solver_bytes * (size_t)s;
    PnSolver W;
    W.hdr = (int*)b;
    W.best_tcw = (float*)(W.hdr + kPnHdrInts);
    W.ref_tcw = W.best_tcw + 12;
    W.best_w = (unsigned long long*)(W.ref_tcw + 12);
    W.ref_w = W.best_w + L.words;
    W.al = (double*)(W.ref_w + L.words);
    W.pc = W.al + (size_t)4 * cap;
    W.P3 = (float*)(W.pc + (size_t)3 * cap);
    W.P2 = W.P3 + (size_t)3 * cap;
    W.E = W.P2 + (size_t)2 * cap;
    W.kp = (int*)(W.E + cap);
    W.mp = W.kp + cap;
    W.sel = W.mp + cap;
    return W;
}

struct PnHyp {
    float* tcw;
    int* inl;
    unsigned long long* words;
};

ORBX_HD PnHyp pn_hyp(void* work, const PnLayout& L, size_t h)
{
    uint8_t* b = (uint8_t*)work + L.hyp_off + L.hyp_bytes * h;
    PnHyp H;
    H.tcw = (float*)b;
    H.inl = (int*)(H.tcw + 12);
    H.words = (unsigned long long*)(H.tcw + kPnHypFloats);
    return H;
}

// ---- lanes ----
ORBX_HD int pn_tid()
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (int)threadIdx.x;
#else
    return 0;
#endif
}

ORBX_HD void pn_sync()
{
#if defined(__HIP_DEVICE_COMPILE__)
    __syncthreads();
#endif
}

template <int NT>
struct PnShared {
    int wave_n[NT / 64 + 1];
    int bad, pick;
};

// rank of this lane among the chunk's lanes with `flag` set, in lane order, and their number
template <int NT>
ORBX_HD int pn_rank(PnShared<NT>& S, bool flag, int* total)
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

// ---- setup: the constructor and SetRansacParameters ----
struct PnTables {
    const orbx_keypoint* kps;
    const int* counts;
    int nframes, cap;
    const int* kf_mp;
    int nkf;
    const orbm_map_point* pts;
    int nmp;
    orbm_pose_params P;
    float th2;
    int max_iterations;
};

enum { kPnSkip = 0, kPnKeep = 1, kPnBad = 2 };

// :81-99 for one frame feature i < nf; every range check in front of the read it guards
ORBX_HD int pn_entry(const PnTables& T, const int* match, int f, int kf, int i, int* mp_out, int* octave)
{
    const int m = match[i];
    if (m < -1 || m >= T.cap) return kPnBad;
    if (m < 0) return kPnSkip;
    const int mp = T.kf_mp[(size_t)kf * T.cap + m];
    if (mp < -1 || mp >= T.nmp) return kPnBad;
    if (mp < 0) return kPnSkip;                      // !pMP
    if (!(T.pts[mp].flags & 1)) return kPnSkip;      // isBad()
    const int o = T.kps[(size_t)f * T.cap + i].octave;
    if ((unsigned)o >= (unsigned)T.P.nlevels) return kPnBad;
    *mp_out = mp;
    *octave = o;
    return kPnKeep;
}

template <int NT>
ORBX_HD void pn_setup(PnShared<NT>& S, const PnTables& T, int f, int kf, const int* match, const int* mininl,
                      const int* maxits, const PnSolver& W, int words, int* n_out, int* iterations, int* best,
                      int* status)
{
    const int tid = pn_tid();
    bool ok = (unsigned)f < (unsigned)T.nframes && (unsigned)kf < (unsigned)T.nkf;
    int nf = 0;
    if (ok) {
        nf = T.counts[f];
        ok = nf >= 0 && nf <= T.cap;
    }
    if (tid == 0) S.bad = 0;
    pn_sync();
    if (ok) {
        int bad = 0, mp, o;
        for (int i = tid; i < nf; i += NT)
            if (pn_entry(T, match, f, kf, i, &mp, &o) == kPnBad) bad = 1;
        if (bad) S.bad = 1;   // every writer stores the same value
    }
    pn_sync();
    int n = 0;
    if (ok && !S.bad) {
        for (int c = 0; c < nf; c += NT) {
            const int i = c + tid;
            int mp = -1, o = 0;
            const bool keep = i < nf && pn_entry(T, match, f, kf, i, &mp, &o) == kPnKeep;
            int total;
            const int k = n + pn_rank(S, keep, &total);
            if (keep) {
                const orbx_keypoint kpt = T.kps[(size_t)f * T.cap + i];
                const orbm_map_point M = T.pts[mp];
                const float sigma2 = T.P.scale[o] * T.P.scale[o];   // mvLevelSigma2
                W.P2[2 * k] = kpt.x;
                W.P2[2 * k + 1] = kpt.y;
                W.P3[3 * k] = M.x;
                W.P3[3 * k + 1] = M.y;
                W.P3[3 * k + 2] = M.z;
                W.E[k] = sigma2 * T.th2;   // mvMaxError
                W.kp[k] = i;
                W.mp[k] = mp;
            }
            n += total;
            pn_sync();   // wave_n is rewritten by the next chunk
        }
        // the per-n tables are the caller's: entries the calls cannot run with make the solver invalid
        const int mi = mininl[n], mx = maxits[n];
        if (mi < 4 || mx < 1 || mx > T.max_iterations) ok = false;
    }
    if (!ok || S.bad) {   // of an invalid solver only the status is written (and the workspace's own mark)
        if (tid == 0) {
            W.hdr[0] = 0;
            W.hdr[1] = 0;
            W.hdr[2] = 0;
            W.hdr[3] = 0;
            *status = ORBM_PNP_INVALID;
        }
        return;
    }
    for (int i = tid; i < 24; i += NT) W.best_tcw[i] = 0.0f;   // best_tcw and ref_tcw are adjacent
    for (int i = tid; i < 2 * words; i += NT) W.best_w[i] = 0ull;
    if (tid == 0) {
        W.hdr[0] = n;
        W.hdr[1] = 1;
        W.hdr[2] = maxits[n];
        W.hdr[3] = mininl[n];
        for (int i = 4; i < kPnHdrInts; ++i) W.hdr[i] = 0;
        *n_out = n;
        *iterations = 0;
        *best = 0;
        *status = 0;
    }
}

// ---- the draw ----
// DUtils::Random::RandomInt(0, size - 1) four times with the swap-with-back removal of :188-201 on mvAllIndices =
// 0 .. n-1, n >= 4, without the list: a removal at position p leaves there what the back held
ORBX_HD void pn_quad(int n, const int* r, int* out)
{
    int mpos[4], mval[4];
    for (int i = 0; i < 4; ++i) {
        const int pos = (int)(((double)(r[i] & 0x7fffffff) / 2147483648.0) * (double)(n - i));
        const int back = n - 1 - i;
        int v = pos, b = back;
        for (int j = 0; j < i; ++j) {   // later removals overwrite earlier ones
            if (mpos[j] == pos) v = mval[j];
            if (mpos[j] == back) b = mval[j];
        }
        out[i] = v;
        mpos[i] = pos;
        mval[i] = b;
    }
}

// ---- OpenCV pieces in double ----
// lapack.cpp's own hypot
ORBX_HD double pn_hypot(double a, double b)
{
    a = __builtin_fabs(a);
    b = __builtin_fabs(b);
    if (a > b) {
        b = b / a;
        return a * __builtin_sqrt(1.0 + b * b);
    }
    if (b > 0.0) {
        a = a / b;
        return b * __builtin_sqrt(1.0 + a * a);
    }
    return 0.0;
}

// JacobiSVDImpl_<double>, the shape of in_svd (orbx_init.hip): At n rows of m doubles, Vt n x n or NULL (the rows of
// At and W do not depend on it), W n doubles.  On return the rows are sorted to descending W and normalised; rows of
// singular value <= DBL_MIN are filled from RNG(0x12345678) and orthogonalised (n1 = n).
ORBX_HD void pn_svd(double* At, int m, int n, double* Vt, double* W)
{
    const double eps = DBL_EPSILON * 10.0;
    for (int i = 0; i < n; ++i) {
        double sd = 0.0;
        for (int k = 0; k < m; ++k) sd += At[i * m + k] * At[i * m + k];
        W[i] = sd;
        if (Vt)
            for (int k = 0; k < n; ++k) Vt[i * n + k] = i == k ? 1.0 : 0.0;
    }
    const int max_iter = m > 30 ? m : 30;
    for (int iter = 0; iter < max_iter; ++iter) {
        bool changed = false;
        for (int i = 0; i < n - 1; ++i)
            for (int j = i + 1; j < n; ++j) {
                double* Ai = At + i * m;
                double* Aj = At + j * m;
                double a = W[i], b = W[j], p = 0.0;
                for (int k = 0; k < m; ++k) p += Ai[k] * Aj[k];
                if (__builtin_fabs(p) <= eps * __builtin_sqrt(a * b)) continue;
                p *= 2.0;
                const double beta = a - b, gamma = pn_hypot(p, beta);
                double c, s;
                if (beta < 0.0) {
                    const double delta = (gamma - beta) * 0.5;
                    s = __builtin_sqrt(delta / gamma);
                    c = p / (gamma * s * 2.0);
                } else {
                    c = __builtin_sqrt((gamma + beta) / (gamma * 2.0));
                    s = p / (gamma * c * 2.0);
                }
                a = b = 0.0;
                for (int k = 0; k < m; ++k) {
                    const double t0 = c * Ai[k] + s * Aj[k];
                    const double t1 = -s * Ai[k] + c * Aj[k];
                    Ai[k] = t0;
                    Aj[k] = t1;
                    a += t0 * t0;
                    b += t1 * t1;
                }
                W[i] = a;
                W[j] = b;
                changed = true;
                if (Vt) {
                    double* Vi = Vt + i * n;
                    double* Vj = Vt + j * n;
                    for (int k = 0; k < n; ++k) {
                        const double t0 = c * Vi[k] + s * Vj[k];
                        const double t1 = -s * Vi[k] + c * Vj[k];
                        Vi[k] = t0;
                        Vj[k] = t1;
                    }
                }
            }
        if (!changed) break;
    }
    for (int i = 0; i < n; ++i) {
        double sd = 0.0;
        for (int k = 0; k < m; ++k) sd += At[i * m + k] * At[i * m + k];
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
                const double t = At[i * m + k];
                At[i * m + k] = At[j * m + k];
                At[j * m + k] = t;
            }
            if (Vt)
                for (int k = 0; k < n; ++k) {
                    const double t = Vt[i * n + k];
                    Vt[i * n + k] = Vt[j * n + k];
                    Vt[j * n + k] = t;
                }
        }
    }
    unsigned long long rng = 0x12345678ull;
    const double minval = DBL_MIN;
    for (int i = 0; i < n; ++i) {
        double* Ai = At + i * m;
        double sd = W[i];
        for (int ii = 0; ii < 100 && sd <= minval; ++ii) {
            const double val0 = 1.0 / (double)m;
            for (int k = 0; k < m; ++k) {
                rng = (unsigned long long)(unsigned)rng * 4164903690ull + (rng >> 32);
                Ai[k] = ((unsigned)rng & 256u) != 0u ? val0 : -val0;
            }
            for (int iter = 0; iter < 2; ++iter)
                for (int j = 0; j < i; ++j) {
                    const double* Aj = At + j * m;
                    sd = 0.0;
                    for (int k = 0; k < m; ++k) sd += Ai[k] * Aj[k];
                    double asum = 0.0;
                    for (int k = 0; k < m; ++k) {
                        const double t = Ai[k] - sd * Aj[k];
                        Ai[k] = t;
                        asum += __builtin_fabs(t);
                    }
                    asum = asum > eps * 100.0 ? 1.0 / asum : 0.0;
                    for (int k = 0; k < m; ++k) Ai[k] *= asum;
                }
            sd = 0.0;
            for (int k = 0; k < m; ++k) sd += Ai[k] * Ai[k];
            sd = __builtin_sqrt(sd);
        }
        const double s = sd > minval ? 1.0 / sd : 0.0;
        for (int k = 0; k < m; ++k) Ai[k] *= s;
    }
}

// SVBkSb's threshold: the sum of the singular values in order, times DBL_EPSILON * 2
ORBX_HD double pn_threshold(const double* W, int n)
{
    double t = 0.0;
    for (int i = 0; i < n; ++i) t += W[i];
    return t * (DBL_EPSILON * 2.0);
}

// cvInvert(A, Ainv, CV_SVD) of a 3x3: SVD::compute, then SVD::backSubst without a right-hand side
ORBX_HD void pn_invert33(const double* A, double* X)
{
    double At[9], Vt[9], W[3];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) At[3 * r + c] = A[3 * c + r];
    pn_svd(At, 3, 3, Vt, W);
    for (int i = 0; i < 9; ++i) X[i] = 0.0;
    const double thr = pn_threshold(W, 3);
    for (int i = 0; i < 3; ++i) {
        double wi = W[i];
        if (__builtin_fabs(wi) <= thr) continue;
        wi = 1.0 / wi;
        double buf[3];
        for (int j = 0; j < 3; ++j) buf[j] = At[3 * i + j] * wi;
        for (int r = 0; r < 3; ++r) {
            const double s = Vt[3 * i + r];
            for (int j = 0; j < 3; ++j) X[3 * r + j] = X[3 * r + j] + s * buf[j];
        }
    }
}

// cvSolve(L, rho, x, CV_SVD) of the 6 x n system whose columns are cols[] of l_6x10, n <= 5
ORBX_HD void pn_solve6(const double* l_6x10, const int* cols, int n, const double* rho, double* x)
{
    double At[30], Vt[25], W[5];
    for (int c = 0; c < n; ++c)
        for (int r = 0; r < 6; ++r) At[6 * c + r] = l_6x10[10 * r + cols[c]];
    pn_svd(At, 6, n, Vt, W);
    for (int j = 0; j < n; ++j) x[j] = 0.0;
    const double thr = pn_threshold(W, n);
    for (int i = 0; i < n; ++i) {
        double wi = W[i];
        if (__builtin_fabs(wi) <= thr) continue;
        wi = 1.0 / wi;
        double s = 0.0;
        for (int j = 0; j < 6; ++j) s += At[6 * i + j] * rho[j];
        s *= wi;
        for (int j = 0; j < n; ++j) x[j] = x[j] + s * Vt[n * i + j];
    }
}

// qr_solve (:860-950) of the 6x4 system; A and b are overwritten.  Returns where the reference returns: on eta == 0
// x keeps its content (x is zero at the start of each gauss_newton)
ORBX_HD bool pn_qr_solve(double* A, double* b, double* x)
{
    const int nr = 6, nc = 4;
    double A1[4], A2[4];
    for (int k = 0; k < nc; ++k) {
        // the scan as written: it starts at row k again and so never looks at the last row
        double eta = __builtin_fabs(A[nc * k + k]);
        for (int i = k + 1; i < nr; ++i) {
            const double elt = __builtin_fabs(A[nc * (i - 1) + k]);
            if (eta < elt) eta = elt;
        }
        if (eta == 0.0) return false;
        const double inv_eta = 1.0 / eta;
        double sum = 0.0;
        for (int i = k; i < nr; ++i) {
            A[nc * i + k] *= inv_eta;
            sum += A[nc * i + k] * A[nc * i + k];
        }
        double sigma = __builtin_sqrt(sum);
        if (A[nc * k + k] < 0.0) sigma = -sigma;
        A[nc * k + k] += sigma;
        A1[k] = sigma * A[nc * k + k];
        A2[k] = -eta * sigma;
        for (int j = k + 1; j < nc; ++j) {
            double s2 = 0.0;
            for (int i = k; i < nr; ++i) s2 += A[nc * i + k] * A[nc * i + j];
            const double tau = s2 / A1[k];
            for (int i = k; i < nr; ++i) A[nc * i + j] -= tau * A[nc * i + k];
        }
    }
    for (int j = 0; j < nc; ++j) {   // b <- Qt b
        double tau = 0.0;
        for (int i = j; i < nr; ++i) tau += A[nc * i + j] * b[i];
        tau /= A1[j];
        for (int i = j; i < nr; ++i) b[i] -= tau * A[nc * i + j];
    }
    x[nc - 1] = b[nc - 1] / A2[nc - 1];   // X = R-1 b
    for (int i = nc - 2; i >= 0; --i) {
        double sum = 0.0;
        for (int j = i + 1; j < nc; ++j) sum += A[nc * i + j] * x[j];
        x[i] = (b[i] - sum) / A2[i];
    }
    return true;
}

// ---- EPnP ----
// The correspondences of one compute_pose: add_correspondence of the solver's points sel[0 .. n), with the alphas and
// pcs arrays of that many points (private for the four of a hypothesis, in the workspace for Refine)
struct PnSet {
    const float *P3, *P2;
    const int* sel;
    int n;
    double *al, *pc;
    double fu, fv, uc, vc;
};

ORBX_HD double pn_pw(const PnSet& S, int i, int j) { return (double)S.P3[3 * (size_t)S.sel[i] + j]; }
ORBX_HD double pn_us(const PnSet& S, int i, int j) { return (double)S.P2[2 * (size_t)S.sel[i] + j]; }
ORBX_HD double pn_dot3(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
ORBX_HD double pn_dist2(const double* a, const double* b)
{
    return (a[0] - b[0]) * (a[0] - b[0]) + (a[1] - b[1]) * (a[1] - b[1]) + (a[2] - b[2]) * (a[2] - b[2]);
}

// what the restatement's log records of one compute_pose (test hooks read it; the device drops it)
struct PnTrace {
    int N;            // the approximation chosen
    int b_neg;        // bit a: b[0] < 0 in find_betas_approx_a
    int b1_neg;       // bit a: b[1] < 0 in approx 2 / 3
    int sign_flip;    // bit a: solve_for_sign flipped
    int det_flip;     // bit a: det < 0
    int qr_singular;  // qr_solve returned early
};

// compute_R_and_t (:651-662): compute_ccs, compute_pcs, solve_for_sign, estimate_R_and_t, reprojection_error
ORBX_HD double pn_R_and_t(const PnSet& S, const double* ut, const double* betas, double* R, double* t, int bit,
                          PnTrace* tr)
{
    const int n = S.n;
    double ccs[12];
    for (int i = 0; i < 12; ++i) ccs[i] = 0.0;
    for (int i = 0; i < 4; ++i) {
        const double* v = ut + 12 * (11 - i);
        for (int j = 0; j < 12; ++j) ccs[j] += betas[i] * v[j];
    }
    for (int i = 0; i < n; ++i) {
        const double* a = S.al + 4 * (size_t)i;
        for (int j = 0; j < 3; ++j)
            S.pc[3 * (size_t)i + j] = a[0] * ccs[j] + a[1] * ccs[3 + j] + a[2] * ccs[6 + j] + a[3] * ccs[9 + j];
    }
    if (S.pc[2] < 0.0) {   // solve_for_sign; ccs is not read again
        tr->sign_flip |= bit;
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < 3; ++j) S.pc[3 * (size_t)i + j] = -S.pc[3 * (size_t)i + j];
    }
    double pc0[3] = {0.0, 0.0, 0.0}, pw0[3] = {0.0, 0.0, 0.0};
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < 3; ++j) {
            pc0[j] += S.pc[3 * (size_t)i + j];
            pw0[j] += pn_pw(S, i, j);
        }
    for (int j = 0; j < 3; ++j) {
        pc0[j] /= (double)n;
        pw0[j] /= (double)n;
    }
    double abt[9];
    for (int i = 0; i < 9; ++i) abt[i] = 0.0;
    for (int i = 0; i < n; ++i) {
        const double w0 = pn_pw(S, i, 0) - pw0[0], w1 = pn_pw(S, i, 1) - pw0[1], w2 = pn_pw(S, i, 2) - pw0[2];
        for (int j = 0; j < 3; ++j) {
            const double c = S.pc[3 * (size_t)i + j] - pc0[j];
            abt[3 * j] += c * w0;
            abt[3 * j + 1] += c * w1;
            abt[3 * j + 2] += c * w2;
        }
    }
    // cvSVD(ABt, D, U, V, CV_SVD_MODIFY_A): U's column i is row i of At, V's column i row i of Vt
    double At[9], Vt[9], W[3];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) At[3 * r + c] = abt[3 * c + r];
    pn_svd(At, 3, 3, Vt, W);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            R[3 * i + j] = At[i] * Vt[j] + At[3 + i] * Vt[3 + j] + At[6 + i] * Vt[6 + j];
    const double det = R[0] * R[4] * R[8] + R[1] * R[5] * R[6] + R[2] * R[3] * R[7] - R[2] * R[4] * R[6] -
                       R[1] * R[3] * R[8] - R[0] * R[5] * R[7];
    if (det < 0.0) {
        tr->det_flip |= bit;
        R[6] = -R[6];
        R[7] = -R[7];
        R[8] = -R[8];
    }
    for (int r = 0; r < 3; ++r) t[r] = pc0[r] - pn_dot3(R + 3 * r, pw0);
    double sum2 = 0.0;   // reprojection_error
    for (int i = 0; i < n; ++i) {
        const double pw[3] = {pn_pw(S, i, 0), pn_pw(S, i, 1), pn_pw(S, i, 2)};
        const double Xc = pn_dot3(R, pw) + t[0];
        const double Yc = pn_dot3(R + 3, pw) + t[1];
        const double inv_Zc = 1.0 / (pn_dot3(R + 6, pw) + t[2]);
        const double ue = S.uc + S.fu * Xc * inv_Zc;
        const double ve = S.vc + S.fv * Yc * inv_Zc;
        const double u = pn_us(S, i, 0), v = pn_us(S, i, 1);
        sum2 += __builtin_sqrt((u - ue) * (u - ue) + (v - ve) * (v - ve));
    }
    return sum2 / (double)n;
}

// compute_pose (:477-525): R row-major 3x3, t
ORBX_HD void pn_compute_pose(const PnSet& S, double* R, double* t, PnTrace* tr)
{
    const int n = S.n;
    tr->N = 0;
    tr->b_neg = tr->b1_neg = tr->sign_flip = tr->det_flip = tr->qr_singular = 0;
    // choose_control_points
    double cws[12];
    cws[0] = cws[1] = cws[2] = 0.0;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < 3; ++j) cws[j] += pn_pw(S, i, j);
    for (int j = 0; j < 3; ++j) cws[j] /= (double)n;
    {
        double A[9], W[3];   // PW0tPW0: the upper triangle summed row after row, then completeSymm
        for (int i = 0; i < 9; ++i) A[i] = 0.0;
        for (int k = 0; k < n; ++k) {
            const double d[3] = {pn_pw(S, k, 0) - cws[0], pn_pw(S, k, 1) - cws[1], pn_pw(S, k, 2) - cws[2]};
            for (int a = 0; a < 3; ++a)
                for (int b = a; b < 3; ++b) A[3 * a + b] += d[a] * d[b];
        }
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < a; ++b) A[3 * a + b] = A[3 * b + a];
        pn_svd(A, 3, 3, nullptr, W);   // symmetric: its transpose is itself; A becomes UCt
        for (int i = 1; i < 4; ++i) {
            const double k = __builtin_sqrt(W[i - 1] / (double)n);
            for (int j = 0; j < 3; ++j) cws[3 * i + j] = cws[j] + k * A[3 * (i - 1) + j];
        }
    }
    // compute_barycentric_coordinates
    {
        double cc[9], ci[9];
        for (int i = 0; i < 3; ++i)
            for (int j = 1; j < 4; ++j) cc[3 * i + j - 1] = cws[3 * j + i] - cws[i];
        pn_invert33(cc, ci);
        for (int i = 0; i < n; ++i) {
            double* a = S.al + 4 * (size_t)i;
            const double p0 = pn_pw(S, i, 0), p1 = pn_pw(S, i, 1), p2 = pn_pw(S, i, 2);
            for (int j = 0; j < 3; ++j)
                a[1 + j] = ci[3 * j] * (p0 - cws[0]) + ci[3 * j + 1] * (p1 - cws[1]) + ci[3 * j + 2] * (p2 - cws[2]);
            a[0] = 1.0 - a[1] - a[2] - a[3];
        }
    }
    // fill_M and cvMulTransposed(M, MtM, 1): the upper triangle summed over the 2n rows in order, zeros included
    double ut[144], d12[12];
    for (int i = 0; i < 144; ++i) ut[i] = 0.0;
    for (int i = 0; i < n; ++i) {
        const double* as = S.al + 4 * (size_t)i;
        const double u = pn_us(S, i, 0), v = pn_us(S, i, 1);
        double M1[12], M2[12];
        for (int c = 0; c < 4; ++c) {
            M1[3 * c] = as[c] * S.fu;
            M1[3 * c + 1] = 0.0;
            M1[3 * c + 2] = as[c] * (S.uc - u);
            M2[3 * c] = 0.0;
            M2[3 * c + 1] = as[c] * S.fv;
            M2[3 * c + 2] = as[c] * (S.vc - v);
        }
        for (int a = 0; a < 12; ++a)
            for (int b = a; b < 12; ++b) ut[12 * a + b] += M1[a] * M1[b];
        for (int a = 0; a < 12; ++a)
            for (int b = a; b < 12; ++b) ut[12 * a + b] += M2[a] * M2[b];
    }
    for (int a = 0; a < 12; ++a)
        for (int b = 0; b < a; ++b) ut[12 * a + b] = ut[12 * b + a];
    pn_svd(ut, 12, 12, nullptr, d12);   // cvSVD(MtM, D, Ut, 0, MODIFY_A | U_T): the rows of At are Ut
    // compute_L_6x10, compute_rho
    double l_6x10[60], rho[6];
    {
        double dv[4][6][3];
        for (int i = 0; i < 4; ++i) {
            const double* v = ut + 12 * (11 - i);
            int a = 0, b = 1;
            for (int j = 0; j < 6; ++j) {
                dv[i][j][0] = v[3 * a] - v[3 * b];
                dv[i][j][1] = v[3 * a + 1] - v[3 * b + 1];
                dv[i][j][2] = v[3 * a + 2] - v[3 * b + 2];
                b++;
                if (b > 3) {
                    a++;
                    b = a + 1;
                }
            }
        }
        for (int i = 0; i < 6; ++i) {
            double* row = l_6x10 + 10 * i;
            row[0] = pn_dot3(dv[0][i], dv[0][i]);
            row[1] = 2.0 * pn_dot3(dv[0][i], dv[1][i]);
            row[2] = pn_dot3(dv[1][i], dv[1][i]);
            row[3] = 2.0 * pn_dot3(dv[0][i], dv[2][i]);
            row[4] = 2.0 * pn_dot3(dv[1][i], dv[2][i]);
            row[5] = pn_dot3(dv[2][i], dv[2][i]);
            row[6] = 2.0 * pn_dot3(dv[0][i], dv[3][i]);
            row[7] = 2.0 * pn_dot3(dv[1][i], dv[3][i]);
            row[8] = 2.0 * pn_dot3(dv[2][i], dv[3][i]);
            row[9] = pn_dot3(dv[3][i], dv[3][i]);
        }
        rho[0] = pn_dist2(cws, cws + 3);
        rho[1] = pn_dist2(cws, cws + 6);
        rho[2] = pn_dist2(cws, cws + 9);
        rho[3] = pn_dist2(cws + 3, cws + 6);
        rho[4] = pn_dist2(cws + 3, cws + 9);
        rho[5] = pn_dist2(cws + 6, cws + 9);
    }
    double best_err = 0.0;
    for (int ap = 1; ap <= 3; ++ap) {
        const int bit = 1 << ap;
        double betas[4], bs[5];
        // find_betas_approx_1 / 2 / 3
        const int c1[4] = {0, 1, 3, 6}, c23[5] = {0, 1, 2, 3, 4};
        if (ap == 1) {
            pn_solve6(l_6x10, c1, 4, rho, bs);
            if (bs[0] < 0.0) {
                tr->b_neg |= bit;
                betas[0] = __builtin_sqrt(-bs[0]);
                betas[1] = -bs[1] / betas[0];
                betas[2] = -bs[2] / betas[0];
                betas[3] = -bs[3] / betas[0];
            } else {
                betas[0] = __builtin_sqrt(bs[0]);
                betas[1] = bs[1] / betas[0];
                betas[2] = bs[2] / betas[0];
                betas[3] = bs[3] / betas[0];
            }
        } else {
            pn_solve6(l_6x10, c23, ap == 2 ? 3 : 5, rho, bs);
            if (bs[0] < 0.0) {
                tr->b_neg |= bit;
                betas[0] = __builtin_sqrt(-bs[0]);
                betas[1] = (bs[2] < 0.0) ? __builtin_sqrt(-bs[2]) : 0.0;
            } else {
                betas[0] = __builtin_sqrt(bs[0]);
                betas[1] = (bs[2] > 0.0) ? __builtin_sqrt(bs[2]) : 0.0;
            }
            if (bs[1] < 0.0) {
                tr->b1_neg |= bit;
                betas[0] = -betas[0];
            }
            betas[2] = ap == 2 ? 0.0 : bs[3] / betas[0];
            betas[3] = 0.0;
        }
        // gauss_newton
        double x[4] = {0.0, 0.0, 0.0, 0.0};
        for (int k = 0; k < 5; ++k) {
            double A[24], b[6];
            for (int i = 0; i < 6; ++i) {
                const double* rowL = l_6x10 + i * 10;
                double* rowA = A + i * 4;
                rowA[0] = 2.0 * rowL[0] * betas[0] + rowL[1] * betas[1] + rowL[3] * betas[2] + rowL[6] * betas[3];
                rowA[1] = rowL[1] * betas[0] + 2.0 * rowL[2] * betas[1] + rowL[4] * betas[2] + rowL[7] * betas[3];
                rowA[2] = rowL[3] * betas[0] + rowL[4] * betas[1] + 2.0 * rowL[5] * betas[2] + rowL[8] * betas[3];
                rowA[3] = rowL[6] * betas[0] + rowL[7] * betas[1] + rowL[8] * betas[2] + 2.0 * rowL[9] * betas[3];
                b[i] = rho[i] - (rowL[0] * betas[0] * betas[0] + rowL[1] * betas[0] * betas[1] +
                                 rowL[2] * betas[1] * betas[1] + rowL[3] * betas[0] * betas[2] +
                                 rowL[4] * betas[1] * betas[2] + rowL[5] * betas[2] * betas[2] +
                                 rowL[6] * betas[0] * betas[3] + rowL[7] * betas[1] * betas[3] +
                                 rowL[8] * betas[2] * betas[3] + rowL[9] * betas[3] * betas[3]);
            }
            if (!pn_qr_solve(A, b, x)) tr->qr_singular |= bit;
            for (int i = 0; i < 4; ++i) betas[i] += x[i];
        }
        double Ra[9], ta[3];
        const double err = pn_R_and_t(S, ut, betas, Ra, ta, bit, tr);
        // N = 1; if (rep_errors[2] < rep_errors[1]) N = 2; if (rep_errors[3] < rep_errors[N]) N = 3
        if (ap == 1 || err < best_err) {
            best_err = err;
            tr->N = ap;
            for (int i = 0; i < 9; ++i) R[i] = Ra[i];
            for (int i = 0; i < 3; ++i) t[i] = ta[i];
        }
    }
}

// CheckInliers (:308-339) for point i
ORBX_HD bool pn_inlier(const PnSolver& W, const double* R, const double* t, const PnSet& C, int i)
{
    const float* X = W.P3 + 3 * (size_t)i;
    const double x = (double)X[0], y = (double)X[1], z = (double)X[2];
    const float Xc = (float)(R[0] * x + R[1] * y + R[2] * z + t[0]);
    const float Yc = (float)(R[3] * x + R[4] * y + R[5] * z + t[1]);
    const float invZc = (float)(1.0 / (R[6] * x + R[7] * y + R[8] * z + t[2]));
    const double ue = C.uc + C.fu * (double)Xc * (double)invZc;
    const double ve = C.vc + C.fv * (double)Yc * (double)invZc;
    const float distX = (float)((double)W.P2[2 * (size_t)i] - ue);
    const float distY = (float)((double)W.P2[2 * (size_t)i + 1] - ve);
    const float error2 = distX * distX + distY * distY;
    return error2 < W.E[i];
}

ORBX_HD int pn_check_inliers(const PnSolver& W, const double* R, const double* t, const PnSet& C, int N,
                             unsigned long long* words)
{
    int cnt = 0;
    for (int base = 0; base < N; base += 64) {
        unsigned long long b = 0;
        for (int j = 0; j < 64 && base + j < N; ++j)
            if (pn_inlier(W, R, t, C, base + j)) b |= 1ull << j;
        words[base >> 6] = b;
        cnt += __builtin_popcountll(b);
    }
    return cnt;
}

ORBX_HD PnSet pn_camera(const PnSolver& W, const orbm_pose_params& P)
{
    PnSet S;
    S.P3 = W.P3;
    S.P2 = W.P2;
    S.sel = nullptr;
    S.n = 0;
    S.al = S.pc = nullptr;
    S.fu = (double)P.fx;
    S.fv = (double)P.fy;
    S.uc = (double)P.cx;
    S.vc = (double)P.cy;
    return S;
}

// the Rcw, tcw convertTo(CV_32F) of :217-223 / :294-300
ORBX_HD void pn_tcw(const double* R, const double* t, float* tcw)
{
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) tcw[4 * r + c] = (float)R[3 * r + c];
        tcw[4 * r + 3] = (float)t[r];
    }
}

// the iterations a call runs unless it returns: while(mnIterations<mRansacMaxIts || nCurrentIterations<nIterations)
ORBX_HD int pn_call_iterations(int iterations, int maxits, int nit)
{
    const int left = iterations < maxits ? maxits - iterations : 0;
    return left > nit ? left : nit;
}

// iteration k of one iterate() call, as an independent hypothesis (one lane)
ORBX_HD void pn_hypothesis(const PnSolver& W, const PnHyp& H, const orbm_pose_params& P, int cap, int slots, int k,
                           int nit, const int* rand, int rand_off, int nrand, int iterations, PnTrace* tr)
{
    const int N = W.hdr[0];
    if (W.hdr[1] != 1 || N < W.hdr[3] || N > cap || iterations < 0) return;
    const int cnt = pn_call_iterations(iterations, W.hdr[2], nit);
    if (k >= cnt || k >= slots) return;
    const long long d0 = (long long)rand_off + 4ll * k;
    if (rand_off < 0 || d0 + 4 > (long long)nrand) {   // draws the caller did not supply: an iteration without inliers
        *H.inl = -1;
        return;
    }
    int sel[4];
    pn_quad(N, rand + d0, sel);
    double al[16], pc[12], R[9], t[3];
    PnSet S = pn_camera(W, P);
    S.sel = sel;
    S.n = 4;
    S.al = al;
    S.pc = pc;
    pn_compute_pose(S, R, t, tr);
    *H.inl = pn_check_inliers(W, R, t, S, N, H.words);
    pn_tcw(R, t, H.tcw);
}

// Refine() (:260-305) on mvbBestInliers; leaves its outcome in the solver
ORBX_HD void pn_refine(const PnSolver& W, const orbm_pose_params& P, int N, PnTrace* tr)
{
    int n = 0;
    for (int i = 0; i < N; ++i)
        if ((W.best_w[i >> 6] >> (i & 63)) & 1ull) W.sel[n++] = i;
    PnSet S = pn_camera(W, P);
    S.sel = W.sel;
    S.n = n;
    S.al = W.al;
    S.pc = W.pc;
    double R[9], t[3];
    pn_compute_pose(S, R, t, tr);
    const int inl = pn_check_inliers(W, R, t, S, N, W.ref_w);
    W.hdr[9] = inl;
    W.hdr[8] = inl > W.hdr[3] ? 1 : 0;
    if (W.hdr[8]) pn_tcw(R, t, W.ref_tcw);
}

// ---- the sequential rule of iterate() over the call's hypotheses, and the masks ----
struct PnOut {
    int *iterations, *best;
    float* tcw;
    int* has_pose;
    uint8_t* inliers;
    int *ninliers, *nomore, *used, *frame_mp;
};

template <int NT>
ORBX_HD void pn_select(PnShared<NT>& S, const PnSolver& W, void* work, const PnLayout& L, size_t hyp0, int cap,
                       int slots, const orbm_pose_params& P, int nit, const PnOut& O, PnTrace* refine_tr,
                       int* nrefines)
{
    const int tid = pn_tid();
    const int N = W.hdr[0];
    if (tid == 0) {
        int pick = 0, nomore = 0, used = 0, ninl = 0;   // pick: 0 none, 1 mRefinedTcw, 2 mBestTcw
        if (W.hdr[1] != 1 || N < W.hdr[3] || N > cap || *O.iterations < 0) {
            // bNoMore and nothing else; an invalid solver has no result either, nor has one whose state is negative
            nomore = 1;
        } else {
            const int maxits = W.hdr[2], min_inl = W.hdr[3], words = (N + 63) / 64;
            int it = *O.iterations, best = *O.best;
            int cnt = pn_call_iterations(it, maxits, nit);
            if (cnt > slots) cnt = slots;
            while (used < cnt) {
                const PnHyp H = pn_hyp(work, L, hyp0 + (size_t)used);
                const int inl = *H.inl;
                ++used;
                ++it;
                if (inl >= min_inl) {
                    if (inl > best) {
                        best = inl;
                        for (int i = 0; i < words; ++i) W.best_w[i] = H.words[i];
                        for (int i = 0; i < 12; ++i) W.best_tcw[i] = H.tcw[i];
                        PnTrace tr;
                        pn_refine(W, P, N, &tr);
                        if (refine_tr) refine_tr[*nrefines] = tr;
                        if (nrefines) ++*nrefines;
                    }
                    if (W.hdr[8]) {
                        pick = 1;
                        ninl = W.hdr[9];
                        break;
                    }
                }
            }
            if (!pick) {   // the loop ended, so mnIterations >= mRansacMaxIts
                nomore = 1;
                if (best >= min_inl) {
                    pick = 2;
                    ninl = best;
                }
            }
            *O.iterations = it;
            *O.best = best;
        }
        S.pick = pick;
        const float* src = pick == 1 ? W.ref_tcw : pick == 2 ? W.best_tcw : nullptr;
        for (int i = 0; i < 12; ++i) O.tcw[i] = src ? src[i] : 0.0f;
        *O.has_pose = pick ? 1 : 0;
        *O.ninliers = ninl;
        *O.nomore = nomore;
        *O.used = used;
    }
    for (int i = tid; i < cap; i += NT) {
        O.inliers[i] = 0;
        O.frame_mp[i] = -1;
    }
    pn_sync();
    const int pick = S.pick;
    if (!pick) return;
    const unsigned long long* words = pick == 1 ? W.ref_w : W.best_w;
    for (int j = tid; j < N; j += NT)
        if ((words[j >> 6] >> (j & 63)) & 1ull) {
            const int i = W.kp[j];   // below cap in a workspace that setup wrote
            if ((unsigned)i < (unsigned)cap) {
                O.inliers[i] = 1;          // vbInliers[mvKeyPointIndices[i]]
                O.frame_mp[i] = W.mp[j];   // src/Tracking.cc:1481-1490
            }
        }
}

// ---- kernels ----
__global__ __launch_bounds__(kPnLanes) void k_pnp_setup(PnTables T, const int* __restrict__ frame_of,
                                                        const int* __restrict__ kf_of,
                                                        const int* __restrict__ match, int match_stride,
                                                        const int* __restrict__ mininl,
                                                        const int* __restrict__ maxits, void* work, PnLayout L,
                                                        int* n_out, int* iterations, int* best, int* status)
{
    __shared__ PnShared<kPnLanes> S;
    const int s = blockIdx.x;
    pn_setup<kPnLanes>(S, T, frame_of[s], kf_of[s], match + (size_t)s * match_stride, mininl, maxits,
                       pn_solver(work, L, s, T.cap), L.words, n_out + s, iterations + s, best + s, status + s);
}

__global__ __launch_bounds__(kPnHypLanes) void k_pnp_hyp(void* work, PnLayout L, int cap, int slots,
                                                         orbm_pose_params P, int nit, const int* __restrict__ rand,
                                                         const int* __restrict__ rand_off, int nrand,
                                                         const int* __restrict__ iterations)
{
    const int k = blockIdx.x * kPnHypLanes + threadIdx.x, s = blockIdx.y;
    if (k >= slots) return;
    PnTrace tr;
    pn_hypothesis(pn_solver(work, L, s, cap), pn_hyp(work, L, (size_t)s * slots + k), P, cap, slots, k, nit, rand,
                  rand_off[s], nrand, iterations[s], &tr);
}

__global__ __launch_bounds__(64) void k_pnp_select(void* work, PnLayout L, int cap, int slots, orbm_pose_params P,
                                                   int nit, int* iterations, int* best, float* tcw, int* has_pose,
                                                   uint8_t* inliers, int* ninliers, int* nomore, int* used,
                                                   int* frame_mp)
{
    __shared__ PnShared<64> S;
    const int s = blockIdx.x;
    const PnOut O = {iterations + s, best + s, tcw + (size_t)s * 12, has_pose + s, inliers + (size_t)s * cap,
                     ninliers + s, nomore + s, used + s, frame_mp + (size_t)s * cap};
    pn_select<64>(S, pn_solver(work, L, s, cap), work, L, (size_t)s * slots, cap, slots, P, nit, O, nullptr, nullptr);
}

}  // namespace orbx

using namespace orbx;

extern "C" {

void orbx_pnp_quad(int n, const int* r, int* out4)
{
    if (n >= 4 && r && out4) pn_quad(n, r, out4);
}

int orbx_pnp_qr_solve(double* A24, double* b6, double* x4)
{
    if (!A24 || !b6 || !x4) return -1;
    return pn_qr_solve(A24, b6, x4) ? 1 : 0;
}

void orbx_pnp_svd12(const double* A144, double* ut144, double* w12)
{
    if (!A144 || !ut144 || !w12) return;
    for (int r = 0; r < 12; ++r)
        for (int c = 0; c < 12; ++c) ut144[12 * r + c] = A144[12 * c + r];
    pn_svd(ut144, 12, 12, nullptr, w12);
}

size_t orbm_pnp_workspace_bytes(int nsolvers, int cap, int max_iters_per_call)
{
    if (nsolvers < 0 || nsolvers > kPnMaxGrid || cap < 1 || cap > ORBM_MAX_FEATURES || max_iters_per_call < 1 ||
        max_iters_per_call > kPnMaxGrid)
        return 0;
    return pn_layout(nsolvers, cap, max_iters_per_call).total;
}

size_t orbm_pnp_state_bytes(int cap)
{
    if (cap < 1 || cap > ORBM_MAX_FEATURES) return 0;
    return pn_carry_bytes((cap + 63) / 64);
}

void orbm_pnp_ransac_parameters(int n, double probability, int min_inliers, int max_iterations, int min_set,
                                float epsilon, int* out_min_inliers, int* out_max_iterations)
{
    const float fn = (float)n * epsilon;   // int nMinInliers = N*mRansacEpsilon
    int nMinInliers = (fn >= -2147483648.0f && fn < 2147483648.0f) ? (int)fn : INT_MIN;
    if (nMinInliers < min_inliers) nMinInliers = min_inliers;
    if (nMinInliers < min_set) nMinInliers = min_set;
    if (epsilon < (float)nMinInliers / n) epsilon = (float)nMinInliers / n;
    int nIterations;
    if (nMinInliers == n) {
        nIterations = 1;
    } else {
        const double v = ceil(log(1 - probability) / log(1 - pow(epsilon, 3)));
        nIterations = (v >= -2147483648.0 && v < 2147483648.0) ? (int)v : INT_MIN;
    }
    const int lo = nIterations < max_iterations ? nIterations : max_iterations;
    if (out_min_inliers) *out_min_inliers = nMinInliers;
    if (out_max_iterations) *out_max_iterations = lo > 1 ? lo : 1;
}

static bool pn_params_ok(const orbm_pose_params* P) { return P && P->nlevels >= 1 && P->nlevels <= 16; }

static int pn_slots(int nit, int max_iterations) { return nit > max_iterations ? nit : max_iterations; }

orbx_status orbm_pnp_setup_device(const orbx_keypoint* d_kps, const int* d_counts, int nframes, int cap,
                                  const int* d_kf_mp, int nkf, const orbm_map_point* d_pts, int nmp,
                                  const int* d_frame_of, const int* d_kf_of, int nsolvers, const int* d_match,
                                  int match_stride, const orbm_pose_params* params, float th2,
                                  const int* d_min_inliers, const int* d_maxits, int max_iterations, void* d_work,
                                  size_t work_bytes, int* d_n, int* d_iterations, int* d_best_inliers, int* d_status,
                                  void* stream)
{
    const uintptr_t a4 = (uintptr_t)d_kps | (uintptr_t)d_counts | (uintptr_t)d_kf_mp | (uintptr_t)d_pts |
                         (uintptr_t)d_frame_of | (uintptr_t)d_kf_of | (uintptr_t)d_match | (uintptr_t)d_min_inliers |
                         (uintptr_t)d_maxits | (uintptr_t)d_n | (uintptr_t)d_iterations | (uintptr_t)d_best_inliers |
                         (uintptr_t)d_status;
    if (!d_kps || !d_counts || nframes < 0 || cap < 1 || cap > ORBM_MAX_FEATURES || !d_kf_mp || nkf < 0 || nmp < 0 ||
        (nmp > 0 && !d_pts) || !d_frame_of || !d_kf_of || nsolvers < 0 || nsolvers > kPnMaxGrid || !d_match ||
        match_stride < cap || !pn_params_ok(params) || !d_min_inliers || !d_maxits || max_iterations < 1 ||
        max_iterations > kPnMaxGrid || !d_work || !d_n || !d_iterations || !d_best_inliers || !d_status || (a4 & 3) ||
        ((uintptr_t)d_work & 15) || work_bytes < pn_layout(nsolvers, cap, 1).total)
        return ORBX_EINVAL;
    if (nsolvers == 0) return ORBX_OK;
    const PnTables T = {d_kps, d_counts, nframes, cap, d_kf_mp, nkf, d_pts, nmp, *params, th2, max_iterations};
    // the solver part of the layout does not depend on the iterations per call
    hipLaunchKernelGGL(k_pnp_setup, dim3((unsigned)nsolvers), dim3(kPnLanes), 0, (hipStream_t)stream, T, d_frame_of,
                       d_kf_of, d_match, match_stride, d_min_inliers, d_maxits, d_work, pn_layout(nsolvers, cap, 1),
                       d_n, d_iterations, d_best_inliers, d_status);
    return hipGetLastError() == hipSuccess ? ORBX_OK : ORBX_EDEVICE;
}

orbx_status orbm_pnp_iterate_device(void* d_work, size_t work_bytes, int nsolvers, int cap,
                                    const orbm_pose_params* params, int min_set, int max_iterations, int nit,
                                    const int* d_rand, int nrand, const int* d_rand_off, int* d_iterations,
                                    int* d_best_inliers, float* d_tcw, int* d_has_pose, uint8_t* d_inliers,
                                    int* d_ninliers, int* d_nomore, int* d_used, int* d_frame_mp_out, void* stream)
{
    const uintptr_t a4 = (uintptr_t)d_rand | (uintptr_t)d_rand_off | (uintptr_t)d_iterations |
                         (uintptr_t)d_best_inliers | (uintptr_t)d_tcw | (uintptr_t)d_has_pose |
                         (uintptr_t)d_ninliers | (uintptr_t)d_nomore | (uintptr_t)d_used | (uintptr_t)d_frame_mp_out;
    if (!d_work || nsolvers < 0 || nsolvers > kPnMaxGrid || cap < 1 || cap > ORBM_MAX_FEATURES ||
        !pn_params_ok(params) || min_set != 4 || max_iterations < 1 || max_iterations > kPnMaxGrid || nit < 1 ||
        nit > kPnMaxGrid || !d_rand || nrand < 0 || !d_rand_off || !d_iterations || !d_best_inliers || !d_tcw ||
        !d_has_pose || !d_inliers || !d_ninliers || !d_nomore || !d_used || !d_frame_mp_out || (a4 & 3) ||
        ((uintptr_t)d_work & 15) || work_bytes < pn_layout(nsolvers, cap, pn_slots(nit, max_iterations)).total)
        return ORBX_EINVAL;
    if (nsolvers == 0) return ORBX_OK;
    const int slots = pn_slots(nit, max_iterations);
    const PnLayout L = pn_layout(nsolvers, cap, slots);
    hipLaunchKernelGGL(k_pnp_hyp, dim3((unsigned)((slots + kPnHypLanes - 1) / kPnHypLanes), (unsigned)nsolvers),
                       dim3(kPnHypLanes), 0, (hipStream_t)stream, d_work, L, cap, slots, *params, nit, d_rand,
                       d_rand_off, nrand, d_iterations);
    hipLaunchKernelGGL(k_pnp_select, dim3((unsigned)nsolvers), dim3(64), 0, (hipStream_t)stream, d_work, L, cap, slots,
                       *params, nit, d_iterations, d_best_inliers, d_tcw, d_has_pose, d_inliers, d_ninliers, d_nomore,
                       d_used, d_frame_mp_out);
    return hipGetLastError() == hipSuccess ? ORBX_OK : ORBX_EDEVICE;
}

// the one-solver forms: a table of one frame and one KeyFrame at stride cap
struct PnOne {
    int cap = 0, slots = 0;
    std::vector<int> mininl, maxits;
};

static bool pn_one_args_ok(const orbx_keypoint* kps, int n, const int* kf_mp, int nk, const orbm_map_point* pts,
                           int nmp, const int* match, const orbm_pose_params* params, double probability,
                           int min_inliers, int max_iterations, int min_set, float epsilon, int nit, const int* rand,
                           const int* iterations, const int* best_inliers, const void* state, const int* n_out,
                           const float* tcw, const int* has_pose, const uint8_t* inliers, const int* ninliers,
                           const int* nomore, const int* used, const int* frame_mp_out, const int* status, PnOne* one)
{
    const uintptr_t a4 = (uintptr_t)kps | (uintptr_t)kf_mp | (uintptr_t)pts | (uintptr_t)match | (uintptr_t)rand |
                         (uintptr_t)iterations | (uintptr_t)best_inliers | (uintptr_t)n_out | (uintptr_t)tcw |
                         (uintptr_t)has_pose | (uintptr_t)ninliers | (uintptr_t)nomore | (uintptr_t)used |
                         (uintptr_t)frame_mp_out | (uintptr_t)status;
    if (n < 0 || n > ORBM_MAX_FEATURES || nk < 0 || nk > ORBM_MAX_FEATURES ||
        (n > 0 && (!kps || !match || !inliers || !frame_mp_out)) || (nk > 0 && !kf_mp) || nmp < 0 ||
        (nmp > 0 && !pts) || !pn_params_ok(params) || min_set != 4 || max_iterations < 1 ||
        max_iterations > kPnMaxGrid || nit < 1 || nit > kPnMaxGrid || !rand || !iterations || !best_inliers ||
        !state || !n_out || !tcw || !has_pose || !ninliers || !nomore || !used || !status || (a4 & 3) ||
        ((uintptr_t)state & 7))
        return false;
    one->cap = n > nk ? n : nk;
    if (one->cap < 1) one->cap = 1;
    one->slots = pn_slots(nit, max_iterations);
    one->mininl.resize((size_t)one->cap + 1);
    one->maxits.resize((size_t)one->cap + 1);
    for (int k = 0; k <= one->cap; ++k)
        orbm_pnp_ransac_parameters(k, probability, min_inliers, max_iterations, min_set, epsilon,
                                   &one->mininl[(size_t)k], &one->maxits[(size_t)k]);
    return true;
}

orbx_status orbm_pnp_solve_host(const orbx_keypoint* kps, int n, const int* kf_mp, int nk, const orbm_map_point* pts,
                                int nmp, const int* match, const orbm_pose_params* params, float th2,
                                double probability, int min_inliers, int max_iterations, int min_set, float epsilon,
                                int nit, const int* rand, int* iterations, int* best_inliers, void* state,
                                int* n_out, float* tcw, int* has_pose, uint8_t* inliers, int* ninliers, int* nomore,
                                int* used, int* frame_mp_out, int* status, orbm_pnp_trace* trace, int trace_cap,
                                int* ntrace)
{
    PnOne one;
    if (!pn_one_args_ok(kps, n, kf_mp, nk, pts, nmp, match, params, probability, min_inliers, max_iterations, min_set,
                        epsilon, nit, rand, iterations, best_inliers, state, n_out, tcw, has_pose, inliers, ninliers,
                        nomore, used, frame_mp_out, status, &one) ||
        trace_cap < 0 || (trace_cap > 0 && (!trace || !ntrace)))
        return ORBX_EINVAL;
    const int cap = one.cap, slots = one.slots;
    std::vector<orbx_keypoint> kp((size_t)cap);
    std::vector<int> kmp((size_t)cap, -1), mt((size_t)cap, -1);
    if (n) {
        std::memcpy(kp.data(), kps, sizeof(orbx_keypoint) * (size_t)n);
        std::memcpy(mt.data(), match, sizeof(int) * (size_t)n);
    }
    if (nk) std::memcpy(kmp.data(), kf_mp, sizeof(int) * (size_t)nk);
    const PnLayout L = pn_layout(1, cap, slots);
    std::vector<unsigned long long> work(L.total / 8 + 2);
    void* w = work.data();   // operator new aligns to 16
    const PnTables T = {kp.data(), &n, 1, cap, kmp.data(), 1, pts, nmp, *params, th2, max_iterations};
    const PnSolver W = pn_solver(w, L, 0, cap);
    PnShared<1> S;
    int st = 0, nn = 0, it0 = 0, best0 = 0;
    pn_setup<1>(S, T, 0, 0, mt.data(), one.mininl.data(), one.maxits.data(), W, L.words, &nn, &it0, &best0, &st);
    *status = st;
    if (st) return ORBX_OK;
    const size_t carry = pn_carry_bytes(L.words);
    if (*iterations != 0) std::memcpy((uint8_t*)w + kPnCarryOff, state, carry);   // a solver that goes on
    std::vector<PnTrace> tr((size_t)slots + 1), rtr((size_t)slots + 1);
    for (int k = 0; k < slots; ++k) {
        tr[(size_t)k].N = 0;
        pn_hypothesis(W, pn_hyp(w, L, (size_t)k), *params, cap, slots, k, nit, rand, 0, 4 * slots, *iterations,
                      &tr[(size_t)k]);
    }
    std::vector<uint8_t> in((size_t)cap);
    std::vector<int> fmp((size_t)cap);
    int nref = 0;
    const PnOut O = {iterations, best_inliers, tcw, has_pose, in.data(), ninliers, nomore, used, fmp.data()};
    pn_select<1>(S, W, w, L, 0, cap, slots, *params, nit, O, rtr.data(), &nref);
    std::memcpy(state, (uint8_t*)w + kPnCarryOff, carry);
    *n_out = nn;
    if (n) {
        std::memcpy(inliers, in.data(), (size_t)n);
        std::memcpy(frame_mp_out, fmp.data(), sizeof(int) * (size_t)n);
    }
    if (ntrace) {   // the iterations consumed, then the Refine() calls: what each compute_pose met
        int m = 0;
        for (int k = 0; k < *used + nref && m < trace_cap; ++k, ++m) {
            const PnTrace& t = k < *used ? tr[(size_t)k] : rtr[(size_t)(k - *used)];
            trace[m].refine = k < *used ? 0 : 1;
            trace[m].N = t.N;
            trace[m].b_neg = t.b_neg;
            trace[m].b1_neg = t.b1_neg;
            trace[m].sign_flip = t.sign_flip;
            trace[m].det_flip = t.det_flip;
            trace[m].qr_singular = t.qr_singular;
            trace[m].inliers = k < *used ? *pn_hyp(w, L, (size_t)k).inl : 0;
        }
        *ntrace = m;
    }
    return ORBX_OK;
}

orbx_status orbm_pnp_solve(int device, const orbx_keypoint* kps, int n, const int* kf_mp, int nk,
                           const orbm_map_point* pts, int nmp, const int* match, const orbm_pose_params* params,
                           float th2, double probability, int min_inliers, int max_iterations, int min_set,
                           float epsilon, int nit, const int* rand, int* iterations, int* best_inliers, void* state,
                           int* n_out, float* tcw, int* has_pose, uint8_t* inliers, int* ninliers, int* nomore,
                           int* used, int* frame_mp_out, int* status)
{
    PnOne one;
    if (!pn_one_args_ok(kps, n, kf_mp, nk, pts, nmp, match, params, probability, min_inliers, max_iterations, min_set,
                        epsilon, nit, rand, iterations, best_inliers, state, n_out, tcw, has_pose, inliers, ninliers,
                        nomore, used, frame_mp_out, status, &one))
        return ORBX_EINVAL;
    const int cap = one.cap, slots = one.slots;
    const PnLayout L = pn_layout(1, cap, slots);
    const size_t C = (size_t)cap, carry = pn_carry_bytes(L.words);
    const int head[8] = {n, 0, 0, 0, *iterations, *best_inliers, 0, 0};   // count, frame, kf, rand_off, state, pad
    struct Res {
        int n, status, has_pose, ninliers, nomore, used, s0, s1;   // s0, s1: scratch
        float tcw[16];
    } r;
    HostCall c(device);
    const auto okp = c.stage<orbx_keypoint>(C);
    const auto omp = c.stage<int>(C);
    const auto omt = c.stage<int>(C);
    const auto ohd = c.in(head, 8);
    const auto omi = c.in(one.mininl.data(), C + 1);
    const auto omx = c.in(one.maxits.data(), C + 1);
    const auto ord = c.in(rand, (size_t)4 * slots);
    const auto opt = c.in(pts, (size_t)nmp);
    const auto ost = c.in((const uint8_t*)state, carry);
    const auto ores = c.out<Res>(1);
    const auto oin = c.out<uint8_t>(C);
    const auto ofm = c.out<int>(C);
    const auto owk = c.out<uint8_t>(L.total);
    orbx_status rc = c.prepare();
    if (rc != ORBX_OK) return rc;
    std::fill_n(std::copy_n(kps, (size_t)n, c.host(okp)), C - (size_t)n, orbx_keypoint{});
    std::fill_n(std::copy_n(kf_mp, (size_t)nk, c.host(omp)), C - (size_t)nk, -1);
    std::fill_n(std::copy_n(match, (size_t)n, c.host(omt)), C - (size_t)n, -1);
    rc = c.upload();
    if (rc != ORBX_OK) return rc;
    Res* const d = c.dev(ores);
    // the constructor's own zero state goes to the two scratch words; iterate starts from the caller's state
    rc = orbm_pnp_setup_device(c.dev(okp), c.dev(ohd), 1, cap, c.dev(omp), 1, nmp ? c.dev(opt) : nullptr, nmp,
                               c.dev(ohd, 1), c.dev(ohd, 2), 1, c.dev(omt), cap, params, th2, c.dev(omi), c.dev(omx),
                               max_iterations, c.dev(owk), L.total, &d->n, &d->s0, &d->s1, &d->status, c.stream());
    if (rc != ORBX_OK) return rc;
    if (*iterations != 0 &&
        hipMemcpyAsync(c.dev(owk) + kPnCarryOff, c.dev(ost), carry, hipMemcpyDeviceToDevice, c.stream()) != hipSuccess)
        return ORBX_EDEVICE;
    rc = orbm_pnp_iterate_device(c.dev(owk), L.total, 1, cap, params, min_set, max_iterations, nit, c.dev(ord),
                                 4 * slots, c.dev(ohd, 3), c.dev(ohd, 4), c.dev(ohd, 5), d->tcw, &d->has_pose,
                                 c.dev(oin), &d->ninliers, &d->nomore, &d->used, c.dev(ofm), c.stream());
    if (rc != ORBX_OK) return rc;
    int st2[2];
    std::vector<uint8_t> in(C), carried(carry);
    std::vector<int> fmp(C);
    c.fetch(ores, &r, 1);
    c.fetch(ohd, st2, 2, 4);
    c.fetch(oin, in.data(), C);
    c.fetch(ofm, fmp.data(), C);
    c.fetch(owk, carried.data(), carry, kPnCarryOff);
    rc = c.finish();
    if (rc != ORBX_OK) return rc;
    *status = r.status;
    if (r.status) return ORBX_OK;   // of an invalid solver only the status is written
    *n_out = r.n;
    *iterations = st2[0];
    *best_inliers = st2[1];
    std::memcpy(tcw, r.tcw, sizeof(float) * 12);
    *has_pose = r.has_pose;
    *ninliers = r.ninliers;
    *nomore = r.nomore;
    *used = r.used;
    std::memcpy(state, carried.data(), carry);
    if (n) {
        std::memcpy(inliers, in.data(), (size_t)n);
        std::memcpy(frame_mp_out, fmp.data(), sizeof(int) * (size_t)n);
    }
    return ORBX_OK;
}

}  // extern "C"

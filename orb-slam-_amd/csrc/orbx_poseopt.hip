// Optimizer::PoseOptimization (src/Optimizer.cc:239-451): motion-only bundle adjustment of one Frame -- one 6-DoF
// vertex, one unary edge per feature with a MapPoint, Levenberg-Marquardt on a 6x6 system, four rounds with an
// inlier / outlier classification after each -- and the discard loop Tracking runs on its result
// (src/Tracking.cc:830-848, :953-972).  Kernel and C entry points (include/orbx.h).
//
// k_pose_opt: one workgroup of 256 lanes per frame.  The g2o control flow (sparse_optimizer.cpp optimize,
// optimization_algorithm_levenberg.cpp solve, block_solver.hpp, base_unary_edge.hpp, robust_kernel_impl.cpp,
// linear_solver_dense.h, types_six_dof_expmap, se3quat.h) is restated in po_frame below; its arithmetic order is
// DESIGN.md §3 "Pose optimisation arithmetic".  All of it is IEEE double without contraction.
//
// One pass (po_pass) evaluates the level-0 edges at one estimate: every lane takes one feature of a 256-feature
// chunk and computes the edge's 28 terms -- the 21 upper-triangle products of A^T (w Omega) A, the 6 of
// -A^T (w Omega) e and rho[0] -- into LDS at the edge's rank among the chunk's level-0 edges (ballot prefix), then
// lanes 0..27, one per component, add the chunk's terms to their accumulator in rank order.  H, b and the robust
// chi2 are therefore summed in edge order, the only order that equals a sequential reference bit for bit.  Lane 0
// runs the serial part between passes: lambda, the LDLT solve, the SE3 update, the step test.
// A trial's pass also builds the system at the trial estimate; when the trial is accepted that is the next
// iteration's computeActiveErrors + buildSystem, so an iteration costs one pass per trial.
// The level of an edge is its outlier flag (d_outlier), which the classification writes; no other per-edge state
// is kept, and nothing is allocated.
//
// po_frame is a template over the lanes per workgroup: the kernel instantiates 256, and orbm_pose_optimization_host
// -- the same code on the CPU, one lane -- is what the tests without a GPU compare with their restatement.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstring>

#include "orbx_host.hpp"
#include "orbx_math.hpp"

namespace orbx {

constexpr int kPoLanes = 256;
constexpr int kPoTerms = 28;   // 21 H (upper, row-major), 6 b, rho[0]
constexpr int kPoChi = 27;

struct PoSE3 {
    double qx, qy, qz, qw;   // Eigen::Quaterniond coeffs order
    double t[3];
};

// ---- Eigen / se3quat.h pieces, restated ----

ORBX_HD void po_cross(const double* a, const double* b, double* o)
{
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}

// Quaternion * vector: uv = 2 q.vec x v; v + w uv + q.vec x uv
ORBX_HD void po_rotate(const PoSE3& E, const double* v, double* o)
{
    const double q[3] = {E.qx, E.qy, E.qz};
    double uv[3], c[3];
    po_cross(q, v, uv);
    uv[0] = uv[0] + uv[0];
    uv[1] = uv[1] + uv[1];
    uv[2] = uv[2] + uv[2];
    po_cross(q, uv, c);
    for (int i = 0; i < 3; ++i) o[i] = (v[i] + E.qw * uv[i]) + c[i];
}

// SE3Quat::normalizeRotation
ORBX_HD void po_normalize_rotation(PoSE3* E)
{
    if (E->qw < 0.0) {
        E->qx = -E->qx;
        E->qy = -E->qy;
        E->qz = -E->qz;
        E->qw = -E->qw;
    }
    double s = E->qx * E->qx;
    s += E->qy * E->qy;
    s += E->qz * E->qz;
    s += E->qw * E->qw;
    const double n = __builtin_sqrt(s);
    E->qx = E->qx / n;
    E->qy = E->qy / n;
    E->qz = E->qz / n;
    E->qw = E->qw / n;
}

// Quaterniond(Matrix3d), m row-major
ORBX_HD void po_quat_from_matrix(const double* m, PoSE3* E)
{
    double t = (m[0] + m[4]) + m[8];
    if (t > 0.0) {
        t = __builtin_sqrt(t + 1.0);
        E->qw = 0.5 * t;
        t = 0.5 / t;
        E->qx = (m[7] - m[5]) * t;
        E->qy = (m[2] - m[6]) * t;
        E->qz = (m[3] - m[1]) * t;
    } else {
        int i = 0;
        if (m[4] > m[0]) i = 1;
        if (m[8] > m[i * 4]) i = 2;
        // j = (i + 1) % 3, k = (j + 1) % 3; the three cases spelled out so that m is never indexed at run time
        double mii, mjj, mkk, mkj, mjk, mji, mij, mki, mik;
        if (i == 0) {
            mii = m[0]; mjj = m[4]; mkk = m[8]; mkj = m[7]; mjk = m[5]; mji = m[3]; mij = m[1]; mki = m[6]; mik = m[2];
        } else if (i == 1) {
            mii = m[4]; mjj = m[8]; mkk = m[0]; mkj = m[2]; mjk = m[6]; mji = m[7]; mij = m[5]; mki = m[1]; mik = m[3];
        } else {
            mii = m[8]; mjj = m[0]; mkk = m[4]; mkj = m[3]; mjk = m[1]; mji = m[2]; mij = m[6]; mki = m[5]; mik = m[7];
        }
        t = __builtin_sqrt(((mii - mjj) - mkk) + 1.0);
        const double qi = 0.5 * t;
        t = 0.5 / t;
        E->qw = (mkj - mjk) * t;
        const double qj = (mji + mij) * t;
        const double qk = (mki + mik) * t;
        E->qx = i == 0 ? qi : (i == 2 ? qj : qk);
        E->qy = i == 1 ? qi : (i == 0 ? qj : qk);
        E->qz = i == 2 ? qi : (i == 1 ? qj : qk);
    }
}

// Quaterniond::toRotationMatrix, row-major
ORBX_HD void po_to_matrix(const PoSE3& E, double* r)
{
    const double tx = 2.0 * E.qx, ty = 2.0 * E.qy, tz = 2.0 * E.qz;
    const double twx = tx * E.qw, twy = ty * E.qw, twz = tz * E.qw;
    const double txx = tx * E.qx, txy = ty * E.qx, txz = tz * E.qx;
    const double tyy = ty * E.qy, tyz = tz * E.qy, tzz = tz * E.qz;
    r[0] = 1.0 - (tyy + tzz);
    r[1] = txy - twz;
    r[2] = txz + twy;
    r[3] = txy + twz;
    r[4] = 1.0 - (txx + tzz);
    r[5] = tyz - twx;
    r[6] = txz - twy;
    r[7] = tyz + twx;
    r[8] = 1.0 - (txx + tyy);
}

// Converter::toSE3Quat of a row-major 3x4 float mTcw
ORBX_HD void po_from_pose(const float* T, PoSE3* E)
{
    double m[9];
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) m[r * 3 + c] = (double)T[r * 4 + c];
        E->t[r] = (double)T[r * 4 + 3];
    }
    po_quat_from_matrix(m, E);
    po_normalize_rotation(E);
}

// SE3Quat::exp(dx) * E
ORBX_HD void po_exp_times(const double* dx, const PoSE3& E, PoSE3* out)
{
    const double o0 = dx[0], o1 = dx[1], o2 = dx[2];
    double s = o0 * o0;
    s += o1 * o1;
    s += o2 * o2;
    const double theta = __builtin_sqrt(s);
    const double Om[9] = {0.0, -o2, o1, o2, 0.0, -o0, -o1, o0, 0.0};   // skew(omega)
    double Om2[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double a = Om[i * 3] * Om[j];
            a += Om[i * 3 + 1] * Om[3 + j];
            a += Om[i * 3 + 2] * Om[6 + j];
            Om2[i * 3 + j] = a;
        }
    double R[9], V[9];
    if (theta < 0.00001) {
        for (int i = 0; i < 9; ++i) {
            const double id = (i % 4 == 0) ? 1.0 : 0.0;
            R[i] = (id + Om[i]) + Om2[i];
            V[i] = R[i];
        }
    } else {
        double sn, cs, th3;
        po_sincos_theta3(theta, &sn, &cs, &th3);
        const double a = sn / theta, b = (1.0 - cs) / (theta * theta), c = (theta - sn) / th3;
        for (int i = 0; i < 9; ++i) {
            const double id = (i % 4 == 0) ? 1.0 : 0.0;
            R[i] = (id + a * Om[i]) + b * Om2[i];
            V[i] = (id + b * Om[i]) + c * Om2[i];
        }
    }
    PoSE3 X;
    po_quat_from_matrix(R, &X);
    po_normalize_rotation(&X);
    for (int i = 0; i < 3; ++i) {
        double a = V[i * 3] * dx[3];
        a += V[i * 3 + 1] * dx[4];
        a += V[i * 3 + 2] * dx[5];
        X.t[i] = a;
    }
    double rt[3];
    po_rotate(X, E.t, rt);
    for (int i = 0; i < 3; ++i) out->t[i] = X.t[i] + rt[i];
    // Quaternion product X.r * E.r
    out->qw = ((X.qw * E.qw - X.qx * E.qx) - X.qy * E.qy) - X.qz * E.qz;
    out->qx = ((X.qw * E.qx + X.qx * E.qw) + X.qy * E.qz) - X.qz * E.qy;
    out->qy = ((X.qw * E.qy + X.qy * E.qw) + X.qz * E.qx) - X.qx * E.qz;
    out->qz = ((X.qw * E.qz + X.qz * E.qw) + X.qx * E.qy) - X.qy * E.qx;
    po_normalize_rotation(out);
}

// Eigen::LDLT of the symmetric 6x6 H + lambda I (H packed upper, row-major) and its solve of b.  False (x
// untouched) where isPositive() is false.
struct PoLdltWork {
    double m[36], y[6], temp[6];
    int tr[6];
};

ORBX_HD bool po_ldlt_solve(const double* Hp, double lambda, const double* b, double* x, PoLdltWork* W)
{
    double* m = W->m;
    double* y = W->y;
    double* temp = W->temp;
    int* tr = W->tr;
    int p = 0;
    for (int j = 0; j < 6; ++j)
        for (int k = j; k < 6; ++k, ++p) m[j * 6 + k] = m[k * 6 + j] = Hp[p];
    for (int j = 0; j < 6; ++j) m[j * 7] = m[j * 7] + lambda;
    int sign = 0;   // 0 ZeroSign, 1 PositiveSemiDef, -1 NegativeSemiDef, 2 Indefinite
    for (int k = 0; k < 6; ++k) {
        int idx = k;
        double big = __builtin_fabs(m[k * 7]);
        for (int j = k + 1; j < 6; ++j) {
            const double a = __builtin_fabs(m[j * 7]);
            if (a > big) {
                big = a;
                idx = j;
            }
        }
        tr[k] = idx;
        if (idx != k) {
            double tmp;
            for (int j = 0; j < k; ++j) { tmp = m[k * 6 + j]; m[k * 6 + j] = m[idx * 6 + j]; m[idx * 6 + j] = tmp; }
            for (int i = idx + 1; i < 6; ++i) { tmp = m[i * 6 + k]; m[i * 6 + k] = m[i * 6 + idx]; m[i * 6 + idx] = tmp; }
            tmp = m[k * 7]; m[k * 7] = m[idx * 7]; m[idx * 7] = tmp;
            for (int i = k + 1; i < idx; ++i) { tmp = m[i * 6 + k]; m[i * 6 + k] = m[idx * 6 + i]; m[idx * 6 + i] = tmp; }
        }
        if (k > 0) {
            for (int j = 0; j < k; ++j) temp[j] = m[j * 7] * m[k * 6 + j];
            double s = 0.0;
            for (int j = 0; j < k; ++j) s += m[k * 6 + j] * temp[j];
            m[k * 7] = m[k * 7] - s;
            for (int i = k + 1; i < 6; ++i) {
                s = 0.0;
                for (int j = 0; j < k; ++j) s += m[i * 6 + j] * temp[j];
                m[i * 6 + k] = m[i * 6 + k] - s;
            }
        }
        const double akk = m[k * 7];
        const bool valid = __builtin_fabs(akk) > 0.0;
        if (k == 0 && !valid) {
            for (int j = 0; j < 6; ++j) tr[j] = j;
            break;
        }
        if (valid)
            for (int i = k + 1; i < 6; ++i) m[i * 6 + k] = m[i * 6 + k] / akk;
        if (sign == 1) {
            if (akk < 0.0) sign = 2;
        } else if (sign == -1) {
            if (akk > 0.0) sign = 2;
        } else if (sign == 0) {
            if (akk > 0.0) sign = 1;
            else if (akk < 0.0) sign = -1;
        }
    }
    if (!(sign == 1 || sign == 0)) return false;
    for (int i = 0; i < 6; ++i) y[i] = b[i];
    for (int k = 0; k < 6; ++k) { const double tmp = y[k]; y[k] = y[tr[k]]; y[tr[k]] = tmp; }
    for (int i = 1; i < 6; ++i)
        for (int j = 0; j < i; ++j) y[i] = y[i] - m[i * 6 + j] * y[j];
    const double tol = 1.0 / DBL_MAX;
    for (int i = 0; i < 6; ++i) y[i] = __builtin_fabs(m[i * 7]) > tol ? y[i] / m[i * 7] : 0.0;
    for (int i = 4; i >= 0; --i)
        for (int j = 5; j > i; --j) y[i] = y[i] - m[j * 6 + i] * y[j];
    for (int k = 5; k >= 0; --k) { const double tmp = y[k]; y[k] = y[tr[k]]; y[tr[k]] = tmp; }
    for (int i = 0; i < 6; ++i) x[i] = y[i];
    return true;
}

// ---- one edge ----

struct PoCam {
    double fx, fy, cx, cy, bf;
};

struct PoObs {
    double u, v, ur, inv_sigma2, X[3];
    bool stereo;
};

// computeError() at E: the error vector (2 or 3 rows) and chi2(); pc = the point in the camera
ORBX_HD double po_error(const PoSE3& E, const PoCam& C, const PoObs& o, double* e, double* pc)
{
    double r[3];
    po_rotate(E, o.X, r);
    for (int i = 0; i < 3; ++i) pc[i] = r[i] + E.t[i];   // SE3Quat::map
    e[2] = 0.0;
    if (o.stereo) {
        const double invz = (double)(float)(1.0 / pc[2]);   // const float invz = 1.0f/trans_xyz[2]
        const double pu = (pc[0] * invz) * C.fx + C.cx;
        e[0] = o.u - pu;
        e[1] = o.v - ((pc[1] * invz) * C.fy + C.cy);
        e[2] = o.ur - (pu - C.bf * invz);
    } else {
        e[0] = o.u - ((pc[0] / pc[2]) * C.fx + C.cx);   // project2d
        e[1] = o.v - ((pc[1] / pc[2]) * C.fy + C.cy);
    }
    double chi2 = e[0] * (o.inv_sigma2 * e[0]);
    chi2 += e[1] * (o.inv_sigma2 * e[1]);
    if (o.stereo) chi2 += e[2] * (o.inv_sigma2 * e[2]);
    return chi2;
}

// computeError, robustify, linearizeOplus and constructQuadraticForm of one edge: its 28 terms
ORBX_HD void po_edge_terms(const PoSE3& E, const PoCam& C, const PoObs& o, bool huber, double* term)
{
    double e[3], pc[3];
    const double chi2 = po_error(E, C, o, e, pc);
    double rho0 = chi2, rho1 = 1.0;
    if (huber) {
        // delta = the float sqrt(5.991) / sqrt(7.815), dsqr = delta * delta
        const double delta = o.stereo ? (double)(float)__builtin_sqrt(7.815) : (double)(float)__builtin_sqrt(5.991);
        const double dsqr = delta * delta;
        if (!(chi2 <= dsqr)) {
            const double sq = __builtin_sqrt(chi2);
            rho0 = (2.0 * sq) * delta - dsqr;
            rho1 = delta / sq;
        }
    }
    const double w = rho1 * o.inv_sigma2;
    const double x = pc[0], y = pc[1], invz = 1.0 / pc[2], invz2 = invz * invz;
    double A[18];
    A[0] = ((x * y) * invz2) * C.fx;
    A[1] = -(1.0 + (x * x) * invz2) * C.fx;
    A[2] = (y * invz) * C.fx;
    A[3] = -invz * C.fx;
    A[4] = 0.0;
    A[5] = (x * invz2) * C.fx;
    A[6] = (1.0 + (y * y) * invz2) * C.fy;
    A[7] = ((-x * y) * invz2) * C.fy;
    A[8] = (-x * invz) * C.fy;
    A[9] = 0.0;
    A[10] = -invz * C.fy;
    A[11] = (y * invz2) * C.fy;
    A[12] = A[0] - (C.bf * y) * invz2;
    A[13] = A[1] + (C.bf * x) * invz2;
    A[14] = A[2];
    A[15] = A[3];
    A[16] = 0.0;
    A[17] = A[5] - C.bf * invz2;
    const int rows = o.stereo ? 3 : 2;
    int p = 0;
#pragma unroll
    for (int j = 0; j < 6; ++j)
#pragma unroll
        for (int k = j; k < 6; ++k, ++p) {
            double s = A[j] * (w * A[k]);
            s += A[6 + j] * (w * A[6 + k]);
            if (rows == 3) s += A[12 + j] * (w * A[12 + k]);
            term[p] = s;
        }
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double s = A[j] * (w * e[0]);
        s += A[6 + j] * (w * e[1]);
        if (rows == 3) s += A[12 + j] * (w * e[2]);
        term[21 + j] = -s;   // b -= ...
    }
    term[kPoChi] = rho0;
}

// ---- one frame ----

struct PoFrame {
    const orbx_keypoint* kps;
    const float* uright;
    int n;
    int* mp;
    const orbm_map_point* pts;
    int nmp;
    const float* pose_in;
    const orbm_pose_params* P;
    int flags;
    float* pose_out;
    uint8_t* outlier;
    int* frame_outlier;
    int* ninliers;
    int* nmatches_map;
    orbm_pose_opt_trace* trace;
    int* status;
    int fcap;
};

// Diagnostic build only (-DORBX_PO_DIAG_TICKS, tools/diag/pose_opt_time.py --ticks): lane 0 counts the shader clock
// it spends in the ordered sweep and in the whole frame, and the trace's nbad[2] / nbad[3] carry the two counts
// instead of their own values.  The product build has none of it.
#if defined(ORBX_PO_DIAG_TICKS) && defined(__HIP_DEVICE_COMPILE__)
#define PO_TICKS_BEGIN() const long long po_t0_ = clock64()
#define PO_TICKS_END(acc) \
    do {                  \
        if (threadIdx.x == 0) (acc) += clock64() - po_t0_; \
    } while (0)
#else
#define PO_TICKS_BEGIN() (void)0
#define PO_TICKS_END(acc) (void)0
#endif

template <int NT>
struct PoShared {
    double T[kPoTerms * (NT + 1)];   // a chunk's terms, component-major, one double of padding per component
    double acc[kPoTerms];            // the pass in progress
    double cur[kPoTerms];            // H, b, chi2 at E
    double x[6];
    PoLdltWork ldlt;                 // the solve's workspace: indexed at run time, so not in registers
    PoSE3 E, Et, Elast;
    orbm_pose_opt_trace tr;
    long long t_sweep, t_frame;      // ORBX_PO_DIAG_TICKS
    double lambda, ni, cur_chi, ini_chi, rho;
    int wave_n[NT / 64 + 1];
    int count, count2, bad, again, stop, qmax, lm_bad, iters, rejected, ok2;
};

template <int NT>
ORBX_HD int po_tid()
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (int)threadIdx.x;
#else
    return 0;
#endif
}

ORBX_HD void po_sync()
{
#if defined(__HIP_DEVICE_COMPILE__)
    __syncthreads();
#endif
}

ORBX_HD void po_count(int* p, int v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    if (v) atomicAdd(p, v);
#else
    *p += v;
#endif
}

// rank of this lane among the chunk's lanes with `flag` set, in lane order, and their number
template <int NT>
ORBX_HD int po_rank(PoShared<NT>& S, bool flag, int* total)
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

ORBX_HD void po_load_obs(const PoFrame& F, int i, int mp, PoObs* o)
{
    const orbx_keypoint kp = F.kps[i];
    const float ur = F.uright[i];
    const orbm_map_point M = F.pts[mp];
    o->u = (double)kp.x;
    o->v = (double)kp.y;
    o->ur = (double)ur;
    o->stereo = !(ur < 0.0f);   // mvuRight[i]<0: monocular
    o->inv_sigma2 = (double)F.P->inv_sigma2[kp.octave];
    o->X[0] = (double)M.x;
    o->X[1] = (double)M.y;
    o->X[2] = (double)M.z;
}

// computeActiveErrors + activeRobustChi2 + buildSystem at E over the level-0 edges, summed in edge order into S.acc
template <int NT>
ORBX_HD void po_pass(PoShared<NT>& S, const PoFrame& F, const PoCam& C, const PoSE3& E, bool huber)
{
    const int tid = po_tid<NT>();
    for (int c = tid; c < kPoTerms; c += NT) S.acc[c] = 0.0;
    for (int base = 0; base < F.n; base += NT) {
        const int i = base + tid;
        int mp = -1;
        if (i < F.n) mp = F.mp[i];
        const bool act = mp >= 0 && !F.outlier[i];
        double term[kPoTerms];
        if (act) {
            PoObs o;
            po_load_obs(F, i, mp, &o);
            po_edge_terms(E, C, o, huber, term);
        }
        int total;
        const int rank = po_rank(S, act, &total);
        if (act)
            for (int c = 0; c < kPoTerms; ++c) S.T[c * (NT + 1) + rank] = term[c];
        po_sync();
        PO_TICKS_BEGIN();
        for (int c = tid; c < kPoTerms; c += NT) {
            double a = S.acc[c];
            const double* t = S.T + c * (NT + 1);
            for (int k = 0; k < total; ++k) a += t[k];
            S.acc[c] = a;
        }
        PO_TICKS_END(S.t_sweep);
        po_sync();
    }
    po_sync();
}

template <int NT>
ORBX_HD void po_frame(PoShared<NT>& S, const PoFrame& F)
{
    const int tid = po_tid<NT>();
    const orbm_pose_params& P = *F.P;
    if (tid == 0) S.t_sweep = S.t_frame = 0;
    PO_TICKS_BEGIN();
    // ---- validation: each check in front of the read it guards; of an invalid frame only the status is written
    // S.bad: the count is out of range (lane 0's word, only read by the others); S.count2: a bad feature
    if (tid == 0) {
        S.bad = (F.n < 0 || F.n > F.fcap) ? 1 : 0;
        S.count2 = 0;
    }
    po_sync();
    if (!S.bad) {
        int bad = 0;
        for (int i = tid; i < F.n; i += NT) {
            const int mp = F.mp[i];
            if (mp < -1 || mp >= F.nmp) bad = 1;
            else if (mp >= 0 && (unsigned)F.kps[i].octave >= (unsigned)P.nlevels) bad = 1;
        }
        po_count(&S.count2, bad);
    }
    po_sync();
    if (S.bad || S.count2) {
        if (tid == 0) *F.status = ORBM_POSE_OPT_INVALID;
        return;
    }
    // ---- the edges: nInitialCorrespondences, mvbOutlier[i] = false (:280-360)
    if (tid == 0) S.count = 0;
    po_sync();
    {
        int n = 0;
        for (int i = tid; i < F.n; i += NT)
            if (F.mp[i] >= 0) {
                F.outlier[i] = 0;
                ++n;
            }
        po_count(&S.count, n);
    }
    po_sync();
    const int ncorr = S.count;
    const PoCam C = {(double)P.fx, (double)P.fy, (double)P.cx, (double)P.cy, (double)P.bf};
    if (tid == 0) {
        orbm_pose_opt_trace& tr = S.tr;
        for (int r = 0; r < 4; ++r) tr.iters[r] = tr.rejected[r] = tr.nbad[r] = 0;
        tr.rounds = 0;
        tr.ncorr = ncorr;
    }
    int nbad = 0;
    if (ncorr >= 3) {
        if (tid == 0)
            for (int j = 0; j < 6; ++j) S.x[j] = 0.0;
        for (int it = 0; it < 4; ++it) {
            const bool huber = it < 3;   // setRobustKernel(0) after round index 2
            const int nact = ncorr - nbad;
            if (tid == 0) {
                po_from_pose(F.pose_in, &S.E);   // vSE3->setEstimate(Converter::toSE3Quat(pFrame->mTcw))
                S.Elast = S.E;
                S.iters = S.rejected = 0;
                S.stop = 0;
            }
            po_sync();
            if (nact > 0) {   // else initializeOptimization leaves no vertex and optimize returns -1
                {
                    const PoSE3 E = S.E;
                    po_pass(S, F, C, E, huber);
                }
                if (tid == 0)
                    for (int c = 0; c < kPoTerms; ++c) S.cur[c] = S.acc[c];
                po_sync();
                for (int iter = 0; iter < 10; ++iter) {
                    if (tid == 0) {
                        S.cur_chi = S.ini_chi = S.cur[kPoChi];
                        if (iter == 0) {   // computeLambdaInit
                            double md = 0.0;
                            int p = 0;
                            for (int j = 0; j < 6; p += 6 - j, ++j) {
                                const double a = __builtin_fabs(S.cur[p]);
                                md = a < md ? md : a;   // std::max(fabs(H(j,j)), maxDiagonal)
                            }
                            S.lambda = 1e-5 * md;
                            S.ni = 2.0;
                            S.lm_bad = 0;
                        }
                        S.qmax = 0;
                    }
                    do {
                        if (tid == 0) {
                            S.ok2 = po_ldlt_solve(S.cur, S.lambda, S.cur + 21, S.x, &S.ldlt) ? 1 : 0;
                            po_exp_times(S.x, S.E, &S.Et);   // update() runs with the previous x after a failed solve
                        }
                        po_sync();
                        {
                            const PoSE3 Et = S.Et;
                            po_pass(S, F, C, Et, huber);
                        }
                        if (tid == 0) {
                            const double temp_chi = S.ok2 ? S.acc[kPoChi] : DBL_MAX;
                            double rho = S.cur_chi - temp_chi;
                            double scale = 0.0;
                            for (int j = 0; j < 6; ++j) scale += S.x[j] * (S.lambda * S.x[j] + S.cur[21 + j]);
                            scale += 1e-3;
                            rho /= scale;
                            S.Elast = S.Et;
                            if (rho > 0.0 && __builtin_isfinite(temp_chi)) {
                                const double u = 2.0 * rho - 1.0;
                                double alpha = 1.0 - (u * u) * u;
                                alpha = alpha < 2.0 / 3.0 ? alpha : 2.0 / 3.0;        // std::min(alpha, upper)
                                const double sf = 1.0 / 3.0 < alpha ? alpha : 1.0 / 3.0;   // std::max(lower, alpha)
                                S.lambda *= sf;
                                S.ni = 2.0;
                                S.cur_chi = temp_chi;
                                S.E = S.Et;   // discardTop
                                for (int c = 0; c < kPoTerms; ++c) S.cur[c] = S.acc[c];
                            } else {
                                S.lambda *= S.ni;
                                S.ni *= 2.0;
                                ++S.rejected;   // pop
                            }
                            ++S.qmax;
                            S.rho = rho;
                            S.again = (rho < 0.0 && S.qmax < 10) ? 1 : 0;
                        }
                        po_sync();
                    } while (S.again);
                    if (tid == 0) {
                        ++S.iters;
                        if (S.qmax == 10 || S.rho == 0.0) S.stop = 1;
                        else {
                            if ((S.ini_chi - S.cur_chi) * 1e3 < S.ini_chi) ++S.lm_bad;
                            else S.lm_bad = 0;
                            if (S.lm_bad >= 3) S.stop = 1;
                        }
                    }
                    po_sync();
                    if (S.stop) break;
                }
            }
            // ---- classification (:381-438): an outlier's error at the final estimate, any other edge's as the
            // last computeActiveErrors left it
            if (tid == 0) S.count2 = 0;
            po_sync();
            {
                const PoSE3 E = S.E, El = S.Elast;
                int nb = 0;
                for (int i = tid; i < F.n; i += NT) {
                    const int mp = F.mp[i];
                    if (mp < 0) continue;
                    PoObs o;
                    po_load_obs(F, i, mp, &o);
                    double e[3], pc[3];
                    const float chi2 = (float)po_error(F.outlier[i] ? E : El, C, o, e, pc);
                    const bool out = chi2 > (o.stereo ? 7.815f : 5.991f);
                    F.outlier[i] = out ? 1 : 0;
                    nb += out ? 1 : 0;
                }
                po_count(&S.count2, nb);
            }
            po_sync();
            nbad = S.count2;
            if (tid == 0) {
                S.tr.iters[it] = S.iters;
                S.tr.rejected[it] = S.rejected;
                S.tr.nbad[it] = nbad;
                S.tr.rounds = it + 1;
            }
            po_sync();
            if (ncorr < 10) break;   // optimizer.edges().size()<10
        }
        if (tid == 0) {   // Converter::toCvMat(SE3Quat)
            double R[9];
            po_to_matrix(S.E, R);
            for (int r = 0; r < 3; ++r) {
                for (int c = 0; c < 3; ++c) F.pose_out[r * 4 + c] = (float)R[r * 3 + c];
                F.pose_out[r * 4 + 3] = (float)S.E.t[r];
            }
        }
    } else {
        for (int j = tid; j < 12; j += NT) F.pose_out[j] = F.pose_in[j];
    }
    // ---- the loop after the optimiser (src/Tracking.cc:830-848): discard or count
    po_sync();   // every lane has read ncorr from S.count before it is reused
    if (tid == 0) S.count = 0;
    po_sync();
    {
        int nm = 0;
        const bool discard = (F.flags & ORBM_POSE_OPT_DISCARD) != 0;
        for (int i = tid; i < F.n; i += NT) {
            const int mp = F.mp[i];
            int ol = -1;
            if (mp >= 0) {
                if (F.outlier[i]) {
                    if (discard) {
                        ol = mp;
                        F.mp[i] = -1;
                        F.outlier[i] = 0;
                    }
                } else if (F.pts[mp].flags & 2) {
                    ++nm;
                }
            }
            if (discard) F.frame_outlier[i] = ol;
        }
        po_count(&S.count, nm);
    }
    po_sync();
    if (tid == 0) {
        *F.ninliers = ncorr >= 3 ? ncorr - nbad : 0;
        *F.nmatches_map = S.count;
        PO_TICKS_END(S.t_frame);
#if defined(ORBX_PO_DIAG_TICKS)
        S.tr.nbad[2] = (int)S.t_sweep;
        S.tr.nbad[3] = (int)S.t_frame;
#endif
        if (F.trace) *F.trace = S.tr;
        *F.status = 0;
    }
}

__global__ __launch_bounds__(kPoLanes) void k_pose_opt(const orbx_keypoint* kps, const float* uright,
                                                       const int* fcounts, int fcap, int* frame_mp,
                                                       const orbm_map_point* pts, int nmp, const float* pose_in,
                                                       int pose_stride, orbm_pose_params P, int flags,
                                                       float* pose_out, uint8_t* outlier, int* frame_outlier,
                                                       int* ninliers, int* nmatches_map, orbm_pose_opt_trace* trace,
                                                       int* status)
{
    __shared__ PoShared<kPoLanes> S;
    const int f = blockIdx.x;
    const size_t o = (size_t)f * fcap;
    PoFrame F;
    F.kps = kps + o;
    F.uright = uright + o;
    F.n = fcounts[f];
    F.mp = frame_mp + o;
    F.pts = pts;
    F.nmp = nmp;
    F.pose_in = pose_in + (size_t)f * pose_stride;
    F.P = &P;
    F.flags = flags;
    F.pose_out = pose_out + (size_t)f * 12;
    F.outlier = outlier + o;
    F.frame_outlier = frame_outlier ? frame_outlier + o : nullptr;
    F.ninliers = ninliers + f;
    F.nmatches_map = nmatches_map + f;
    F.trace = trace ? trace + f : nullptr;
    F.status = status + f;
    F.fcap = fcap;
    po_frame<kPoLanes>(S, F);
}

}  // namespace orbx

using namespace orbx;

extern "C" {

void orbx_po_sincos_theta3(double theta, double* out3)
{
    po_sincos_theta3(theta, out3, out3 + 1, out3 + 2);
}

static bool po_args_ok(const void* kps, const void* uright, const void* counts, int nframes, int fcap,
                       const void* frame_mp, const void* pts, int nmp, const void* pose_in, int pose_stride,
                       const orbm_pose_params* params, int flags, const void* pose_out, const void* outlier,
                       const void* frame_outlier, const void* ninliers, const void* nmatches_map, const void* trace,
                       const void* status)
{
    const uintptr_t a4 = (uintptr_t)kps | (uintptr_t)uright | (uintptr_t)counts | (uintptr_t)frame_mp |
                         (uintptr_t)pts | (uintptr_t)pose_in | (uintptr_t)pose_out | (uintptr_t)frame_outlier |
                         (uintptr_t)ninliers | (uintptr_t)nmatches_map | (uintptr_t)trace | (uintptr_t)status;
    return kps && uright && counts && nframes >= 0 && fcap > 0 && fcap <= ORBM_MAX_FEATURES && frame_mp && nmp >= 0 &&
           (pts || nmp == 0) && pose_in && (pose_stride == 12 || pose_stride == 24) && params &&
           params->nlevels >= 1 && params->nlevels <= 16 && !(flags & ~ORBM_POSE_OPT_DISCARD) && pose_out &&
           outlier && (frame_outlier || !(flags & ORBM_POSE_OPT_DISCARD)) && ninliers && nmatches_map && status &&
           !(a4 & 3);
}

orbx_status orbm_pose_optimization_device(const orbx_keypoint* d_kps, const float* d_uright, const int* d_fcounts,
                                          int nframes, int fcap, int* d_frame_mp, const orbm_map_point* d_pts,
                                          int nmp, const float* d_pose_in, int pose_stride,
                                          const orbm_pose_params* params, int flags, float* d_pose_out,
                                          uint8_t* d_outlier, int* d_frame_outlier, int* d_ninliers,
                                          int* d_nmatches_map, orbm_pose_opt_trace* d_trace, int* d_status,
                                          void* stream)
{
    if (!po_args_ok(d_kps, d_uright, d_fcounts, nframes, fcap, d_frame_mp, d_pts, nmp, d_pose_in, pose_stride, params,
                    flags, d_pose_out, d_outlier, d_frame_outlier, d_ninliers, d_nmatches_map, d_trace, d_status))
        return ORBX_EINVAL;
    if (nframes == 0) return ORBX_OK;
    hipLaunchKernelGGL(k_pose_opt, dim3((unsigned)nframes), dim3(kPoLanes), 0, (hipStream_t)stream, d_kps, d_uright,
                       d_fcounts, fcap, d_frame_mp, d_pts, nmp, d_pose_in, pose_stride, *params, flags, d_pose_out,
                       d_outlier, d_frame_outlier, d_ninliers, d_nmatches_map, d_trace, d_status);
    return hipGetLastError() == hipSuccess ? ORBX_OK : ORBX_EDEVICE;
}

orbx_status orbm_pose_optimization_host(const orbx_keypoint* kps, const float* uright, int n, int* frame_mp,
                                        const orbm_map_point* pts, int nmp, const float* pose_in,
                                        const orbm_pose_params* params, int flags, float* pose_out, uint8_t* outlier,
                                        int* frame_outlier, int* ninliers, int* nmatches_map,
                                        orbm_pose_opt_trace* trace, int* status)
{
    if (n < 0 || n > ORBM_MAX_FEATURES ||
        !po_args_ok(kps, uright, &n, 1, n > 0 ? n : 1, frame_mp, pts, nmp, pose_in, 12, params, flags, pose_out,
                    outlier, frame_outlier, ninliers, nmatches_map, trace, status))
        return ORBX_EINVAL;
    PoShared<1> S;
    PoFrame F = {kps,      uright,  n,             frame_mp, pts,          nmp,   pose_in, params, flags,
                 pose_out, outlier, frame_outlier, ninliers, nmatches_map, trace, status,  n};
    po_frame<1>(S, F);
    return ORBX_OK;
}

orbx_status orbm_pose_optimization(int device, const orbx_keypoint* kps, const float* uright, int n, int* frame_mp,
                                   const orbm_map_point* pts, int nmp, const float* pose_in,
                                   const orbm_pose_params* params, int flags, float* pose_out, uint8_t* outlier,
                                   int* frame_outlier, int* ninliers, int* nmatches_map, orbm_pose_opt_trace* trace,
                                   int* status)
{
    if (n < 0 || n > ORBM_MAX_FEATURES ||
        !po_args_ok(kps, uright, &n, 1, n > 0 ? n : 1, frame_mp, pts, nmp, pose_in, 12, params, flags, pose_out,
                    outlier, frame_outlier, ninliers, nmatches_map, trace, status))
        return ORBX_EINVAL;
    // The per-feature blocks are sized by cap, not by in()'s own empty-block rule: the device call takes cap as
    // its frame stride (which must be > 0) and the results are fetched cap elements at a time, so an empty frame
    // is one element with no source, never read.
    const size_t cap = n > 0 ? (size_t)n : 1;
    struct Res {
        int status, ninliers, nmatches_map;
        float pose[12];
        orbm_pose_opt_trace tr;
    } res;
    HostCall c(device);
    const auto ocn = c.in(&n, 1);
    const auto opo = c.in(pose_in, 12);
    const auto ok = c.in(n ? kps : nullptr, cap);
    const auto our = c.in(n ? uright : nullptr, cap);
    const auto omp = c.in(n ? frame_mp : nullptr, cap);
    const auto oout = c.in(n ? outlier : nullptr, cap);
    const auto op = c.in(pts, (size_t)nmp);
    const auto ores = c.out<Res>(1);
    const auto ofo = c.out<int>(cap);
    orbx_status rc = c.begin();
    if (rc != ORBX_OK) return rc;
    Res* const d = c.dev(ores);
    rc = orbm_pose_optimization_device(c.dev(ok), c.dev(our), c.dev(ocn), 1, (int)cap, c.dev(omp), c.dev(op), nmp,
                                       c.dev(opo), 12, params, flags, d->pose, c.dev(oout), c.dev(ofo), &d->ninliers,
                                       &d->nmatches_map, &d->tr, &d->status, c.stream());
    if (rc != ORBX_OK) return rc;
    c.fetch(ores, &res, 1);
    std::vector<int> mp_new(cap), fo_new(cap);
    std::vector<uint8_t> out_new(cap);
    c.fetch(omp, mp_new.data(), cap);
    c.fetch(oout, out_new.data(), cap);
    c.fetch(ofo, fo_new.data(), cap);
    rc = c.finish();
    if (rc != ORBX_OK) return rc;
    *status = res.status;
    if (res.status) return ORBX_OK;   // of an invalid frame only the status is written
    *ninliers = res.ninliers;
    *nmatches_map = res.nmatches_map;
    std::memcpy(pose_out, res.pose, sizeof(res.pose));
    if (trace) *trace = res.tr;
    if (n > 0) {
        std::memcpy(outlier, out_new.data(), (size_t)n);
        if (flags & ORBM_POSE_OPT_DISCARD) {
            std::memcpy(frame_mp, mp_new.data(), sizeof(int) * (size_t)n);
            std::memcpy(frame_outlier, fo_new.data(), sizeof(int) * (size_t)n);
        }
    }
    return ORBX_OK;
}

}  // extern "C"

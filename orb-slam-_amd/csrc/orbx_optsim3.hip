// Optimizer::OptimizeSim3 (src/Optimizer.cc:1046-1241): the 7-DoF refinement LoopClosing::ComputeSim3 runs between
// SearchBySim3 and SearchByProjection(pKF, Scw, ...) (src/LoopClosing.cc:325-335) -- one free Sim3 vertex, two
// projection edges per correspondence with fixed points, Levenberg-Marquardt on a 7x7 system, two rounds with an
// inlier check after each -- and the small gather that builds its vpMatches1 on the device (:313-318 plus what
// SearchBySim3 added).  Kernels and C entry points (include/orbx.h).
//
// k_optimize_sim3: one workgroup of 256 lanes per (KF1, KF2) pair.  The g2o control flow (sparse_optimizer.cpp
// optimize, optimization_algorithm_levenberg.cpp solve, block_solver.hpp, linear_solver_dense.h, base_binary_edge.hpp
// constructQuadraticForm and the numeric linearizeOplus, robust_kernel_impl.cpp, types_seven_dof_expmap.h, sim3.h) is
// restated in os_pair below, in the manner of orbx_poseopt.hip; its arithmetic order is DESIGN.md §3 "Sim3
// optimisation arithmetic".  All of it is IEEE double without contraction.
//
// One pass (os_pass) evaluates the remaining edges at one estimate.  The 14 perturbed estimates of the numeric
// Jacobian, Sim3(+-1e-9 e_d) * E, do not depend on the edge: lanes 0..14 compute them (and E itself) with their
// inverses into LDS once per pass.  Then every lane takes one edge of a 256-edge chunk -- lane 2k the e12 and lane
// 2k + 1 the e21 of the chunk's k-th feature of KF1 -- and computes the edge's 36 terms: the 28 upper-triangle
// products of B^T (rho1 Omega) B, the 7 of -B^T (rho1 Omega) e and rho[0], into LDS at the edge's rank among the
// chunk's edges (ballot prefix); lanes 0..35, one per component, add the chunk's terms to their accumulator in rank
// order.  H, b and the robust chi2 are therefore summed in edge order e12(i), e21(i), e12(i'), ..., the only order
// that equals a sequential reference bit for bit.  Lane 0 runs the serial part between passes: lambda, the LDLT
// solve, the Sim3 update, the step test.  A trial's pass also builds the system at the trial estimate; when the trial
// is accepted that is the next iteration's computeActiveErrors + buildSystem.
// A correspondence removed by the first check is one whose d_matches1 entry is -1: no other per-correspondence
// state is kept, and nothing is allocated.
//
// os_pair is a template over the lanes per workgroup: the kernel instantiates 256, and orbm_optimize_sim3_host -- the
// same code on the CPU, one lane -- is what the tests without a GPU compare with their restatement.
// The quaternion pieces and the LDLT repeat those of orbx_poseopt.hip (at size 7), whose text stays as it is.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstring>
#include <vector>

#include "orbx_host.hpp"
#include "orbx_math.hpp"

namespace orbx {

constexpr int kOsLanes = 256;
constexpr int kOsTerms = 36;   // 28 H (upper, row-major), 7 b, rho[0]
constexpr int kOsB = 28;
constexpr int kOsChi = 35;
constexpr int kOsEst = 15;     // E, then Sim3(+1e-9 e_d) * E and Sim3(-1e-9 e_d) * E for d = 0..6
constexpr int kOsMaxGrid = 65535;

struct OsSim3 {
    double qx, qy, qz, qw;   // Eigen::Quaterniond coeffs order, not normalised (g2o::Sim3 does not)
    double t[3];
    double s;
};

// ---- Eigen / sim3.h pieces, restated ----

ORBX_HD void os_cross(const double* a, const double* b, double* o)
{
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}

// Quaternion * vector: uv = 2 q.vec x v; v + w uv + q.vec x uv
ORBX_HD void os_rotate(double qx, double qy, double qz, double qw, const double* v, double* o)
{
    const double q[3] = {qx, qy, qz};
    double uv[3], c[3];
    os_cross(q, v, uv);
    uv[0] = uv[0] + uv[0];
    uv[1] = uv[1] + uv[1];
    uv[2] = uv[2] + uv[2];
    os_cross(q, uv, c);
    for (int i = 0; i < 3; ++i) o[i] = (v[i] + qw * uv[i]) + c[i];
}

// Quaterniond(Matrix3d), m row-major
ORBX_HD void os_quat_from_matrix(const double* m, OsSim3* E)
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
ORBX_HD void os_to_matrix(const OsSim3& E, double* r)
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

// Sim3::map: s * (r * xyz) + t
ORBX_HD void os_map(const OsSim3& S, const double* v, double* o)
{
    double r[3];
    os_rotate(S.qx, S.qy, S.qz, S.qw, v, r);
    for (int i = 0; i < 3; ++i) o[i] = S.s * r[i] + S.t[i];
}

// Sim3::inverse: Sim3(r.conjugate(), r.conjugate() * ((-1. / s) * t), 1. / s)
ORBX_HD void os_inverse(const OsSim3& S, OsSim3* o)
{
    const double c = -1.0 / S.s;
    const double v[3] = {c * S.t[0], c * S.t[1], c * S.t[2]};
    o->qx = -S.qx;
    o->qy = -S.qy;
    o->qz = -S.qz;
    o->qw = S.qw;
    os_rotate(o->qx, o->qy, o->qz, o->qw, v, o->t);
    o->s = 1.0 / S.s;
}

// Sim3::operator*: r = a.r * b.r (Eigen's product, not renormalised), t = a.s * (a.r * b.t) + a.t, s = a.s * b.s
ORBX_HD void os_mul(const OsSim3& a, const OsSim3& b, OsSim3* o)
{
    double rt[3];
    os_rotate(a.qx, a.qy, a.qz, a.qw, b.t, rt);
    const double w = ((a.qw * b.qw - a.qx * b.qx) - a.qy * b.qy) - a.qz * b.qz;
    const double x = ((a.qw * b.qx + a.qx * b.qw) + a.qy * b.qz) - a.qz * b.qy;
    const double y = ((a.qw * b.qy + a.qy * b.qw) + a.qz * b.qx) - a.qx * b.qz;
    const double z = ((a.qw * b.qz + a.qz * b.qw) + a.qx * b.qy) - a.qy * b.qx;
    for (int i = 0; i < 3; ++i) o->t[i] = a.s * rt[i] + a.t[i];
    o->qx = x;
    o->qy = y;
    o->qz = z;
    o->qw = w;
    o->s = a.s * b.s;
}

// Sim3(const Vector7d& update), sim3.h:70-142: omega, upsilon, sigma
ORBX_HD void os_from_update(const double* u, OsSim3* X)
{
    const double o0 = u[0], o1 = u[1], o2 = u[2], sigma = u[6];
    double n2 = o0 * o0;
    n2 += o1 * o1;
    n2 += o2 * o2;
    const double theta = __builtin_sqrt(n2);
    const double Om[9] = {0.0, -o2, o1, o2, 0.0, -o0, -o1, o0, 0.0};   // skew(omega)
    double Om2[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double a = Om[i * 3] * Om[j];
            a += Om[i * 3 + 1] * Om[3 + j];
            a += Om[i * 3 + 2] * Om[6 + j];
            Om2[i * 3 + j] = a;
        }
    const double s = fixed_exp(sigma);
    const double eps = 0.00001;
    double A, B, C, R[9];
    const bool small_theta = theta < eps;
    double sn = 0.0, cs = 1.0, th3 = 0.0;
    if (small_theta) {
        for (int i = 0; i < 9; ++i) {
            const double id = (i % 4 == 0) ? 1.0 : 0.0;
            R[i] = (id + Om[i]) + Om2[i];
        }
    } else {
        po_sincos_theta3(theta, &sn, &cs, &th3);
        const double a = sn / theta, b = (1.0 - cs) / (theta * theta);
        for (int i = 0; i < 9; ++i) {
            const double id = (i % 4 == 0) ? 1.0 : 0.0;
            R[i] = (id + a * Om[i]) + b * Om2[i];
        }
    }
    if (__builtin_fabs(sigma) < eps) {
        C = 1.0;
        if (small_theta) {
            A = 1.0 / 2.0;
            B = 1.0 / 6.0;
        } else {
            const double theta2 = theta * theta;
            A = (1.0 - cs) / theta2;
            B = (theta - sn) / (theta2 * theta);
        }
    } else {
        C = (s - 1.0) / sigma;
        if (small_theta) {
            const double sigma2 = sigma * sigma;
            A = ((sigma - 1.0) * s + 1.0) / sigma2;
            B = (((0.5 * sigma2 - sigma) + 1.0) * s) / (sigma2 * sigma);
        } else {
            const double a = s * sn, b = s * cs;
            const double theta2 = theta * theta, sigma2 = sigma * sigma;
            const double c = theta2 + sigma2;
            A = (a * sigma + (1.0 - b) * theta) / (theta * c);
            B = (C - ((b - 1.0) * sigma + a * theta) / c) / theta2;   // "* 1. / theta2": the product by 1 is exact
        }
    }
    os_quat_from_matrix(R, X);
    for (int i = 0; i < 3; ++i) {   // t = W * upsilon, W = A * Omega + B * Omega2 + C * I
        double acc = 0.0;
        for (int j = 0; j < 3; ++j) {
            const double id = (i == j) ? 1.0 : 0.0;
            const double w = (A * Om[i * 3 + j] + B * Om2[i * 3 + j]) + C * id;
            const double p = w * u[3 + j];
            acc = j == 0 ? p : acc + p;
        }
        X->t[i] = acc;
    }
    X->s = s;
}

// Eigen::LDLT of the symmetric 7x7 H + lambda I (H packed upper, row-major) and its solve of b.  False (x untouched)
// where isPositive() is false.  orbx_poseopt.hip's po_ldlt_solve at size 7.
constexpr int kOsN = 7;
struct OsLdltWork {
    double m[kOsN * kOsN], y[kOsN], temp[kOsN];
    int tr[kOsN];
};

ORBX_HD bool os_ldlt_solve(const double* Hp, double lambda, const double* b, double* x, OsLdltWork* W)
{
    constexpr int N = kOsN, D = kOsN + 1;
    double* m = W->m;
    double* y = W->y;
    double* temp = W->temp;
    int* tr = W->tr;
    int p = 0;
    for (int j = 0; j < N; ++j)
        for (int k = j; k < N; ++k, ++p) m[j * N + k] = m[k * N + j] = Hp[p];
    for (int j = 0; j < N; ++j) m[j * D] = m[j * D] + lambda;
    int sign = 0;   // 0 ZeroSign, 1 PositiveSemiDef, -1 NegativeSemiDef, 2 Indefinite
    for (int k = 0; k < N; ++k) {
        int idx = k;
        double big = __builtin_fabs(m[k * D]);
        for (int j = k + 1; j < N; ++j) {
            const double a = __builtin_fabs(m[j * D]);
            if (a > big) {
                big = a;
                idx = j;
            }
        }
        tr[k] = idx;
        if (idx != k) {
            double tmp;
            for (int j = 0; j < k; ++j) { tmp = m[k * N + j]; m[k * N + j] = m[idx * N + j]; m[idx * N + j] = tmp; }
            for (int i = idx + 1; i < N; ++i) { tmp = m[i * N + k]; m[i * N + k] = m[i * N + idx]; m[i * N + idx] = tmp; }
            tmp = m[k * D]; m[k * D] = m[idx * D]; m[idx * D] = tmp;
            for (int i = k + 1; i < idx; ++i) { tmp = m[i * N + k]; m[i * N + k] = m[idx * N + i]; m[idx * N + i] = tmp; }
        }
        if (k > 0) {
            for (int j = 0; j < k; ++j) temp[j] = m[j * D] * m[k * N + j];
            double s = 0.0;
            for (int j = 0; j < k; ++j) s += m[k * N + j] * temp[j];
            m[k * D] = m[k * D] - s;
            for (int i = k + 1; i < N; ++i) {
                s = 0.0;
                for (int j = 0; j < k; ++j) s += m[i * N + j] * temp[j];
                m[i * N + k] = m[i * N + k] - s;
            }
        }
        const double akk = m[k * D];
        const bool valid = __builtin_fabs(akk) > 0.0;
        if (k == 0 && !valid) {
            for (int j = 0; j < N; ++j) tr[j] = j;
            break;
        }
        if (valid)
            for (int i = k + 1; i < N; ++i) m[i * N + k] = m[i * N + k] / akk;
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
    for (int i = 0; i < N; ++i) y[i] = b[i];
    for (int k = 0; k < N; ++k) { const double tmp = y[k]; y[k] = y[tr[k]]; y[tr[k]] = tmp; }
    for (int i = 1; i < N; ++i)
        for (int j = 0; j < i; ++j) y[i] = y[i] - m[i * N + j] * y[j];
    const double tol = 1.0 / DBL_MAX;
    for (int i = 0; i < N; ++i) y[i] = __builtin_fabs(m[i * D]) > tol ? y[i] / m[i * D] : 0.0;
    for (int i = N - 2; i >= 0; --i)
        for (int j = N - 1; j > i; --j) y[i] = y[i] - m[j * N + i] * y[j];
    for (int k = N - 1; k >= 0; --k) { const double tmp = y[k]; y[k] = y[tr[k]]; y[tr[k]] = tmp; }
    for (int i = 0; i < N; ++i) x[i] = y[i];
    return true;
}

// ---- the tables and one correspondence ----

struct OsTables {
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

enum { kOsSkip = 0, kOsKeep = 1, kOsBad = 2 };

// MapPoint::GetIndexInKeyFrame: the idx of the live observation in KeyFrame kf (n features), -1 none, -2 where the
// list descends or the idx is outside the KeyFrame (orbx_sim3.hip's s3_index_in_kf)
ORBX_HD int os_index_in_kf(const OsTables& T, int mp, int kf, int n)
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

// one row of a cv::Mat 3x3 * 3x1 product (gemm's small-matrix path): float, left to right
ORBX_HD float os_row(const float* r, float x, float y, float z) { return (r[0] * x + r[1] * y) + r[2] * z; }

struct OsCorr {
    int i2, mp1, mp2;
};

// :1099-1136 for one i < na: whether feature i of KF1 makes a correspondence; every range check in front of the read
// it guards
ORBX_HD int os_corr(const OsTables& T, const int* matches1, int a, int b, int nb, int i, OsCorr* c)
{
    const int mp2 = matches1[i];
    if (mp2 < -1 || mp2 >= T.nmp) return kOsBad;
    const int mp1 = T.kf_mp[(size_t)a * T.cap + i];
    if (mp1 < -1 || mp1 >= T.nmp) return kOsBad;
    if (mp2 < 0) return kOsSkip;   // !vpMatches1[i]
    if (mp1 < 0) return kOsSkip;   // !pMP1
    if (!(T.pts[mp1].flags & 1) || !(T.pts[mp2].flags & 1)) return kOsSkip;   // isBad()
    const int i2 = os_index_in_kf(T, mp2, b, nb);
    if (i2 == -2) return kOsBad;
    if (i2 < 0) return kOsSkip;
    const int o1 = T.kps[(size_t)a * T.cap + i].octave, o2 = T.kps[(size_t)b * T.cap + i2].octave;
    if ((unsigned)o1 >= (unsigned)T.P.nlevels || (unsigned)o2 >= (unsigned)T.P.nlevels) return kOsBad;
    c->i2 = i2;
    c->mp1 = mp1;
    c->mp2 = mp2;
    return kOsKeep;
}

struct OsCam {
    double fx, fy, cx, cy;
};

struct OsEdge {
    double X[3], u, v, inv_sigma2;
};

// the e12 (kind 0: the point of KF2 in camera 2, the keypoint i of KF1) or the e21 (kind 1) of a correspondence
ORBX_HD void os_load_edge(const OsTables& T, int a, int b, int i, const OsCorr& c, int kind, OsEdge* e)
{
    const int kf = kind ? a : b;   // the camera the fixed point lives in
    const orbm_map_point M = T.pts[kind ? c.mp1 : c.mp2];
    const float* Tk = T.pose + (size_t)kf * 12;
    for (int r = 0; r < 3; ++r) e->X[r] = (double)(os_row(Tk + 4 * r, M.x, M.y, M.z) + Tk[4 * r + 3]);
    const orbx_keypoint kp = kind ? T.kps[(size_t)b * T.cap + c.i2] : T.kps[(size_t)a * T.cap + i];
    e->u = (double)kp.x;
    e->v = (double)kp.y;
    e->inv_sigma2 = (double)T.P.inv_sigma2[kp.octave];
}

// computeError() with the estimate S (e12) or its inverse (e21) already chosen: obs - cam_map(project(S.map(X)))
ORBX_HD void os_error(const OsSim3& S, const OsCam& C, const OsEdge& o, double* e)
{
    double p[3];
    os_map(S, o.X, p);
    e[0] = o.u - ((p[0] / p[2]) * C.fx + C.cx);
    e[1] = o.v - ((p[1] / p[2]) * C.fy + C.cy);
}

ORBX_HD double os_chi2(const OsEdge& o, const double* e)
{
    double chi2 = e[0] * (o.inv_sigma2 * e[0]);
    chi2 += e[1] * (o.inv_sigma2 * e[1]);
    return chi2;
}

struct OsEst {
    OsSim3 S, Sinv;
};

// computeError, robustify, the numeric linearizeOplus and constructQuadraticForm of one edge: its 36 terms
ORBX_HD void os_edge_terms(const OsEst* est, const OsCam& C, const OsEdge& o, int kind, double delta, double* term)
{
    double e[2];
    os_error(kind ? est[0].Sinv : est[0].S, C, o, e);
    const double chi2 = os_chi2(o, e);
    double rho0 = chi2, rho1 = 1.0;
    const double dsqr = delta * delta;
    if (!(chi2 <= dsqr)) {
        const double sq = __builtin_sqrt(chi2);
        rho0 = (2.0 * sq) * delta - dsqr;
        rho1 = delta / sq;
    }
    const double w = rho1 * o.inv_sigma2;
    const double scalar = 1.0 / (2 * 1e-9);
    double J0[kOsN], J1[kOsN];
#pragma unroll
    for (int d = 0; d < kOsN; ++d) {
        double ep[2], em[2];
        os_error(kind ? est[1 + 2 * d].Sinv : est[1 + 2 * d].S, C, o, ep);
        os_error(kind ? est[2 + 2 * d].Sinv : est[2 + 2 * d].S, C, o, em);
        J0[d] = scalar * (ep[0] - em[0]);
        J1[d] = scalar * (ep[1] - em[1]);
    }
    int p = 0;
#pragma unroll
    for (int j = 0; j < kOsN; ++j)
#pragma unroll
        for (int k = j; k < kOsN; ++k, ++p) {
            double s = J0[j] * (w * J0[k]);
            s += J1[j] * (w * J1[k]);
            term[p] = s;
        }
#pragma unroll
    for (int j = 0; j < kOsN; ++j) {
        double s = J0[j] * (w * e[0]);
        s += J1[j] * (w * e[1]);
        term[kOsB + j] = -s;   // b -= ...
    }
    term[kOsChi] = rho0;
}

// ---- one pair ----

struct OsPair {
    const OsTables* T;   // the kernel's own parameter: a copy would put its pointers behind private memory
    int a, b;
    const float* sim3_in;
    int* matches1;
    float th2;
    int fix_scale;
    double* sim3_out;
    float* sim3f_out;
    float* scw;
    int* nin;
    orbm_opt_sim3_trace* trace;
    int* status;
};

template <int NT>
struct OsShared {
    double T[kOsTerms * (NT + 1)];   // a chunk's terms, component-major, one double of padding per component
    double acc[kOsTerms];            // the pass in progress
    double cur[kOsTerms];            // H, b, chi2 at E
    double x[kOsN];
    OsLdltWork ldlt;                 // the solve's workspace: indexed at run time, so not in registers
    OsEst est[kOsEst];               // the pass's estimates and their inverses
    OsSim3 E, Et, Elast;
    orbm_opt_sim3_trace tr;
    double lambda, ni, cur_chi, ini_chi, rho;
    int wave_n[NT / 64 + 1];
    int count, bad, again, stop, qmax, lm_bad, iters, rejected, ok2;
};

ORBX_HD int os_tid()
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (int)threadIdx.x;
#else
    return 0;
#endif
}

ORBX_HD void os_sync()
{
#if defined(__HIP_DEVICE_COMPILE__)
    __syncthreads();
#endif
}

ORBX_HD void os_count(int* p, int v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    if (v) atomicAdd(p, v);
#else
    *p += v;
#endif
}

// rank of this lane among the chunk's lanes with `flag` set, in lane order, and their number
template <int NT>
ORBX_HD int os_rank(OsShared<NT>& S, bool flag, int* total)
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

// VertexSim3Expmap::oplusImpl: Sim3(update) * E, update[6] zeroed with _fix_scale
ORBX_HD void os_oplus(const double* u, int fix_scale, const OsSim3& E, OsSim3* out)
{
    double v[kOsN];
    for (int j = 0; j < kOsN; ++j) v[j] = u[j];
    if (fix_scale) v[6] = 0.0;
    OsSim3 X;
    os_from_update(v, &X);
    os_mul(X, E, out);
}

// computeActiveErrors + activeRobustChi2 + buildSystem at E over the remaining edges, summed in edge order into S.acc
template <int NT>
ORBX_HD void os_pass(OsShared<NT>& S, const OsPair& F, const OsCam& C, int na, int nb, double delta, const OsSim3& E)
{
    const int tid = os_tid();
    for (int c = tid; c < kOsTerms; c += NT) S.acc[c] = 0.0;
    for (int k = tid; k < kOsEst; k += NT) {
        OsSim3 X = E;
        if (k > 0) {
            double u[kOsN];
            for (int j = 0; j < kOsN; ++j) u[j] = 0.0;
            u[(k - 1) >> 1] = (k & 1) ? 1e-9 : -1e-9;
            os_oplus(u, F.fix_scale, E, &X);
        }
        S.est[k].S = X;
        os_inverse(X, &S.est[k].Sinv);
    }
    os_sync();
    for (int base = 0; base < 2 * na; base += NT) {
        const int edge = base + tid;
        const int i = edge >> 1, kind = edge & 1;
        OsCorr c;
        const bool act = i < na && os_corr(*F.T, F.matches1, F.a, F.b, nb, i, &c) == kOsKeep;
        double term[kOsTerms];
        if (act) {
            OsEdge o;
            os_load_edge(*F.T, F.a, F.b, i, c, kind, &o);
            os_edge_terms(S.est, C, o, kind, delta, term);
        }
        int total;
        const int rank = os_rank(S, act, &total);
        if (act)
            for (int t = 0; t < kOsTerms; ++t) S.T[t * (NT + 1) + rank] = term[t];
        os_sync();
        for (int t = tid; t < kOsTerms; t += NT) {
            double a = S.acc[t];
            const double* src = S.T + t * (NT + 1);
            for (int k = 0; k < total; ++k) a += src[k];
            S.acc[t] = a;
        }
        os_sync();
    }
    os_sync();
}

// SparseOptimizer::optimize(max_iters) with OptimizationAlgorithmLevenberg from S.E; leaves S.E, S.Elast, S.iters,
// S.rejected
template <int NT>
ORBX_HD void os_optimize(OsShared<NT>& S, const OsPair& F, const OsCam& C, int na, int nb, double delta, int max_iters)
{
    const int tid = os_tid();
    if (tid == 0) {
        S.iters = S.rejected = 0;
        S.stop = 0;
    }
    os_sync();
    {
        const OsSim3 E = S.E;
        os_pass(S, F, C, na, nb, delta, E);
    }
    if (tid == 0)
        for (int c = 0; c < kOsTerms; ++c) S.cur[c] = S.acc[c];
    os_sync();
    for (int iter = 0; iter < max_iters; ++iter) {
        if (tid == 0) {
            S.cur_chi = S.ini_chi = S.cur[kOsChi];
            if (iter == 0) {   // computeLambdaInit
                double md = 0.0;
                int p = 0;
                for (int j = 0; j < kOsN; p += kOsN - j, ++j) {
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
                S.ok2 = os_ldlt_solve(S.cur, S.lambda, S.cur + kOsB, S.x, &S.ldlt) ? 1 : 0;
                if (F.fix_scale) S.x[6] = 0.0;   // oplusImpl zeroes the solver's own update[6]
                os_oplus(S.x, F.fix_scale, S.E, &S.Et);   // update() runs with the previous x after a failed solve
            }
            os_sync();
            {
                const OsSim3 Et = S.Et;
                os_pass(S, F, C, na, nb, delta, Et);
            }
            if (tid == 0) {
                const double temp_chi = S.ok2 ? S.acc[kOsChi] : DBL_MAX;
                double rho = S.cur_chi - temp_chi;
                double scale = 0.0;
                for (int j = 0; j < kOsN; ++j) scale += S.x[j] * (S.lambda * S.x[j] + S.cur[kOsB + j]);
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
                    for (int c = 0; c < kOsTerms; ++c) S.cur[c] = S.acc[c];
                } else {
                    S.lambda *= S.ni;
                    S.ni *= 2.0;
                    ++S.rejected;   // pop
                }
                ++S.qmax;
                S.rho = rho;
                S.again = (rho < 0.0 && S.qmax < 10) ? 1 : 0;
            }
            os_sync();
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
        os_sync();
        if (S.stop) break;
    }
}

// the checks of :1186-1203 and :1220-1234: a correspondence either of whose chi2 (as the last computeActiveErrors
// left it, at S.Elast) exceeds th2 gets its match set to -1; returns their number
template <int NT>
ORBX_HD int os_check(OsShared<NT>& S, const OsPair& F, const OsCam& C, int na, int nb)
{
    const int tid = os_tid();
    if (tid == 0) S.count = 0;
    os_sync();
    {
        const OsSim3 El = S.Elast;
        OsSim3 Eli;
        os_inverse(El, &Eli);
        const double th2 = (double)F.th2;
        int n = 0;
        for (int i = tid; i < na; i += NT) {
            OsCorr c;
            if (os_corr(*F.T, F.matches1, F.a, F.b, nb, i, &c) != kOsKeep) continue;
            OsEdge o;
            double e[2];
            os_load_edge(*F.T, F.a, F.b, i, c, 0, &o);
            os_error(El, C, o, e);
            const double chi12 = os_chi2(o, e);
            os_load_edge(*F.T, F.a, F.b, i, c, 1, &o);
            os_error(Eli, C, o, e);
            const double chi21 = os_chi2(o, e);
            if (chi12 > th2 || chi21 > th2) {
                F.matches1[i] = -1;
                ++n;
            }
        }
        os_count(&S.count, n);
    }
    os_sync();
    const int n = S.count;
    os_sync();   // every lane has read the count before it is reused
    return n;
}

template <int NT>
ORBX_HD void os_pair(OsShared<NT>& S, const OsPair& F)
{
    const int tid = os_tid();
    const OsTables& T = *F.T;
    // ---- validation: each check in front of the read it guards; of an invalid pair only the status is written
    bool ok = (unsigned)F.a < (unsigned)T.nkf && (unsigned)F.b < (unsigned)T.nkf;
    int na = 0, nb = 0;
    if (ok) {
        na = T.counts[F.a];
        nb = T.counts[F.b];
        ok = na >= 0 && na <= T.cap && nb >= 0 && nb <= T.cap && F.sim3_in[0] > 0.0f;
    }
    if (tid == 0) {
        S.bad = 0;
        S.count = 0;
    }
    os_sync();
    if (ok) {
        int bad = 0, n = 0;
        OsCorr c;
        for (int i = tid; i < na; i += NT) {
            const int r = os_corr(T, F.matches1, F.a, F.b, nb, i, &c);
            if (r == kOsBad) bad = 1;
            n += r == kOsKeep ? 1 : 0;
        }
        if (bad) S.bad = 1;   // every writer stores the same value
        os_count(&S.count, n);   // nCorrespondences
    }
    os_sync();
    if (!ok || S.bad) {
        if (tid == 0) *F.status = ORBM_OPT_SIM3_INVALID;
        return;
    }
    const int ncorr = S.count;
    os_sync();   // every lane has read ncorr before S.count is reused
    const OsCam C = {(double)T.P.fx, (double)T.P.fy, (double)T.P.cx, (double)T.P.cy};
    const double delta = (double)__builtin_sqrtf(F.th2);   // const float deltaHuber = sqrt(th2)
    if (tid == 0) {
        // g2o::Sim3(Converter::toMatrix3d(R), Converter::toVector3d(t), s)
        double R[9];
        for (int i = 0; i < 9; ++i) R[i] = (double)F.sim3_in[1 + i];
        os_quat_from_matrix(R, &S.E);
        for (int i = 0; i < 3; ++i) S.E.t[i] = (double)F.sim3_in[10 + i];
        S.E.s = (double)F.sim3_in[0];
        S.Elast = S.E;
        for (int j = 0; j < kOsN; ++j) S.x[j] = 0.0;
        orbm_opt_sim3_trace& tr = S.tr;
        tr.iters[0] = tr.iters[1] = tr.rejected[0] = tr.rejected[1] = 0;
        tr.nbad = 0;
        tr.ncorr = ncorr;
        tr.rounds = 0;
    }
    os_sync();
    int result = 0;
    if (ncorr >= 1) {   // with no edge initializeOptimization leaves no vertex and optimize does nothing
        os_optimize(S, F, C, na, nb, delta, 5);
        const int nbad = os_check(S, F, C, na, nb);
        if (tid == 0) {
            S.tr.iters[0] = S.iters;
            S.tr.rejected[0] = S.rejected;
            S.tr.nbad = nbad;
            S.tr.rounds = 1;
        }
        os_sync();
        if (ncorr - nbad >= 10) {
            os_optimize(S, F, C, na, nb, delta, nbad > 0 ? 10 : 5);
            const int nbad2 = os_check(S, F, C, na, nb);
            result = (ncorr - nbad) - nbad2;   // nIn
            if (tid == 0) {
                S.tr.iters[1] = S.iters;
                S.tr.rejected[1] = S.rejected;
                S.tr.rounds = 2;
                // g2oS12 = vSim3_recov->estimate()
                const OsSim3 E = S.E;
                F.sim3_out[0] = E.qx;
                F.sim3_out[1] = E.qy;
                F.sim3_out[2] = E.qz;
                F.sim3_out[3] = E.qw;
                for (int i = 0; i < 3; ++i) F.sim3_out[4 + i] = E.t[i];
                F.sim3_out[7] = E.s;
                if (F.sim3f_out) {
                    double R[9];
                    os_to_matrix(E, R);
                    F.sim3f_out[0] = (float)E.s;
                    for (int i = 0; i < 9; ++i) F.sim3f_out[1 + i] = (float)R[i];
                    for (int i = 0; i < 3; ++i) F.sim3f_out[10 + i] = (float)E.t[i];
                }
                if (F.scw) {
                    // gSmw = Sim3(toMatrix3d(R2w), toVector3d(t2w), 1.0); Converter::toCvMat(gScm * gSmw)
                    const float* Tb = T.pose + (size_t)F.b * 12;
                    OsSim3 M, W;
                    double R[9];
                    for (int r = 0; r < 3; ++r) {
                        for (int c = 0; c < 3; ++c) R[r * 3 + c] = (double)Tb[r * 4 + c];
                        M.t[r] = (double)Tb[r * 4 + 3];
                    }
                    os_quat_from_matrix(R, &M);
                    M.s = 1.0;
                    os_mul(E, M, &W);
                    os_to_matrix(W, R);
                    for (int r = 0; r < 3; ++r) {
                        for (int c = 0; c < 3; ++c) F.scw[r * 4 + c] = (float)(W.s * R[r * 3 + c]);
                        F.scw[r * 4 + 3] = (float)W.t[r];
                    }
                }
            }
        }
    }
    if (tid == 0) {
        *F.nin = result;
        if (F.trace) *F.trace = S.tr;
        *F.status = 0;
    }
}

__global__ __launch_bounds__(kOsLanes) void k_optimize_sim3(OsTables T, const int* __restrict__ pair_a,
                                                            const int* __restrict__ pair_b, const float* sim3_in,
                                                            int* matches1, int match_stride, float th2, int fix_scale,
                                                            double* sim3_out, float* sim3f_out, float* scw, int* nin,
                                                            orbm_opt_sim3_trace* trace, int* status)
{
    __shared__ OsShared<kOsLanes> S;
    const int p = blockIdx.x;
    OsPair F;
    F.T = &T;
    F.a = pair_a[p];
    F.b = pair_b[p];
    F.sim3_in = sim3_in + (size_t)p * 13;
    F.matches1 = matches1 + (size_t)p * match_stride;
    F.th2 = th2;
    F.fix_scale = fix_scale;
    F.sim3_out = sim3_out + (size_t)p * 8;
    F.sim3f_out = sim3f_out ? sim3f_out + (size_t)p * 13 : nullptr;
    F.scw = scw ? scw + (size_t)p * 12 : nullptr;
    F.nin = nin + p;
    F.trace = trace ? trace + p : nullptr;
    F.status = status + p;
    os_pair<kOsLanes>(S, F);
}

// vpMapPointMatches of src/LoopClosing.cc:313-318 after SearchBySim3 (:323): the BoW match of an inlier, else the
// match SearchBySim3 added, as MapPoint indices
__global__ __launch_bounds__(256) void k_sim3_gather_matches(const int* __restrict__ kf_mp,
                                                             const int* __restrict__ counts, int nkf, int cap,
                                                             const int* __restrict__ pair_a,
                                                             const int* __restrict__ pair_b,
                                                             const uint8_t* __restrict__ inliers12,
                                                             const int* __restrict__ bow_match12, int bow_stride,
                                                             const int* __restrict__ sbs_match12, int* matches1,
                                                             int match_stride)
{
    const int p = blockIdx.y;
    const int i1 = blockIdx.x * 256 + threadIdx.x;
    if (i1 >= cap) return;
    const int a = pair_a[p], b = pair_b[p];
    int out = -1;
    if ((unsigned)a < (unsigned)nkf && (unsigned)b < (unsigned)nkf) {
        const int na = counts[a], nb = counts[b];
        if (i1 < na) {
            int j = -1;
            if (inliers12[(size_t)p * cap + i1]) j = bow_match12[(size_t)p * bow_stride + i1];
            else j = sbs_match12[(size_t)p * cap + i1];
            if (j >= 0 && j < nb && j < cap) out = kf_mp[(size_t)b * cap + j];
        }
    }
    matches1[(size_t)p * match_stride + i1] = out;
}

}  // namespace orbx

using namespace orbx;

extern "C" {

double orbx_fixed_exp(double x) { return fixed_exp(x); }

static bool os_params_ok(const orbm_pose_params* P) { return P && P->nlevels >= 1 && P->nlevels <= 16; }

static bool os_args_ok(const void* kps, const void* counts, int nkf, int cap, const void* pose, const void* kf_mp,
                       const void* pts, int nmp, const void* obs_ptr, const void* obs, const void* pair_a,
                       const void* pair_b, int npairs, const void* sim3_in, const void* matches1, int match_stride,
                       const orbm_pose_params* params, const void* sim3_out, const void* sim3f_out, const void* scw,
                       const void* nin, const void* trace, const void* status)
{
    const uintptr_t a4 = (uintptr_t)kps | (uintptr_t)counts | (uintptr_t)pose | (uintptr_t)kf_mp | (uintptr_t)pts |
                         (uintptr_t)obs_ptr | (uintptr_t)obs | (uintptr_t)pair_a | (uintptr_t)pair_b |
                         (uintptr_t)sim3_in | (uintptr_t)matches1 | (uintptr_t)sim3f_out | (uintptr_t)scw |
                         (uintptr_t)nin | (uintptr_t)trace | (uintptr_t)status;
    return kps && counts && nkf >= 0 && cap >= 1 && cap <= ORBM_MAX_FEATURES && pose && kf_mp && nmp >= 0 &&
           (nmp == 0 || (pts && obs_ptr)) && pair_a && pair_b && npairs >= 0 && npairs <= kOsMaxGrid && sim3_in &&
           matches1 && match_stride >= cap && os_params_ok(params) && sim3_out && nin && status && !(a4 & 3) &&
           !((uintptr_t)sim3_out & 7);
}

orbx_status orbm_optimize_sim3_device(const orbx_keypoint* d_kps, const int* d_counts, int nkf, int cap,
                                      const float* d_pose, const int* d_kf_mp, const orbm_map_point* d_pts, int nmp,
                                      const int* d_obs_ptr, const orbm_observation* d_obs,
                                      const uint8_t* d_obs_erased, const int* d_pair_a, const int* d_pair_b,
                                      int npairs, const float* d_sim3_in, int* d_matches1, int match_stride, float th2,
                                      int fix_scale, const orbm_pose_params* params, double* d_sim3_out,
                                      float* d_sim3f_out, float* d_scw, int* d_nin, orbm_opt_sim3_trace* d_trace,
                                      int* d_status, void* stream)
{
    if (!os_args_ok(d_kps, d_counts, nkf, cap, d_pose, d_kf_mp, d_pts, nmp, d_obs_ptr, d_obs, d_pair_a, d_pair_b,
                    npairs, d_sim3_in, d_matches1, match_stride, params, d_sim3_out, d_sim3f_out, d_scw, d_nin,
                    d_trace, d_status))
        return ORBX_EINVAL;
    if (npairs == 0) return ORBX_OK;
    const OsTables T = {d_kps, d_counts, nkf, cap, d_pose, d_kf_mp, d_pts, nmp, d_obs_ptr, d_obs, d_obs_erased, *params};
    hipLaunchKernelGGL(k_optimize_sim3, dim3((unsigned)npairs), dim3(kOsLanes), 0, (hipStream_t)stream, T, d_pair_a,
                       d_pair_b, d_sim3_in, d_matches1, match_stride, th2, fix_scale != 0 ? 1 : 0, d_sim3_out,
                       d_sim3f_out, d_scw, d_nin, d_trace, d_status);
    return hipGetLastError() == hipSuccess ? ORBX_OK : ORBX_EDEVICE;
}

orbx_status orbm_sim3_gather_matches_device(const int* d_kf_mp, const int* d_counts, int nkf, int cap,
                                            const int* d_pair_a, const int* d_pair_b, int npairs,
                                            const uint8_t* d_inliers12, const int* d_bow_match12, int bow_stride,
                                            const int* d_sbs_match12, int* d_matches1, int match_stride, void* stream)
{
    const uintptr_t a4 = (uintptr_t)d_kf_mp | (uintptr_t)d_counts | (uintptr_t)d_pair_a | (uintptr_t)d_pair_b |
                         (uintptr_t)d_bow_match12 | (uintptr_t)d_sbs_match12 | (uintptr_t)d_matches1;
    if (!d_kf_mp || !d_counts || nkf < 0 || cap < 1 || cap > ORBM_MAX_FEATURES || !d_pair_a || !d_pair_b ||
        npairs < 0 || npairs > kOsMaxGrid || !d_inliers12 || !d_bow_match12 || bow_stride < cap || !d_sbs_match12 ||
        !d_matches1 || match_stride < cap || (a4 & 3))
        return ORBX_EINVAL;
    if (npairs == 0) return ORBX_OK;
    hipLaunchKernelGGL(k_sim3_gather_matches, dim3((unsigned)((cap + 255) / 256), (unsigned)npairs), dim3(256), 0,
                       (hipStream_t)stream, d_kf_mp, d_counts, nkf, cap, d_pair_a, d_pair_b, d_inliers12,
                       d_bow_match12, bow_stride, d_sbs_match12, d_matches1, match_stride);
    return hipGetLastError() == hipSuccess ? ORBX_OK : ORBX_EDEVICE;
}

// the one-pair forms: a table of two KeyFrames (slots 0 and 1) at stride cap
struct OsOne {
    int cap = 1, nobs = 0;
    std::vector<orbx_keypoint> kps;
    std::vector<int> kf_mp, m1;
    float pose[24];
    int counts[2];
};

static bool os_one_ok(const orbx_keypoint* kps1, const int* kf_mp1, int n1, const float* T1w,
                      const orbx_keypoint* kps2, int n2, const float* T2w, const orbm_map_point* pts, int nmp,
                      const int* obs_ptr, const orbm_observation* obs, const float* sim3_in, const int* matches1,
                      const orbm_pose_params* params, const double* sim3_out, const float* sim3f_out, const float* scw,
                      const int* nin, const orbm_opt_sim3_trace* trace, const int* status, OsOne* one)
{
    const uintptr_t a4 = (uintptr_t)kps1 | (uintptr_t)kf_mp1 | (uintptr_t)T1w | (uintptr_t)kps2 | (uintptr_t)T2w |
                         (uintptr_t)pts | (uintptr_t)obs_ptr | (uintptr_t)obs | (uintptr_t)sim3_in |
                         (uintptr_t)matches1 | (uintptr_t)sim3f_out | (uintptr_t)scw | (uintptr_t)nin |
                         (uintptr_t)trace | (uintptr_t)status;
    if (n1 < 0 || n1 > ORBM_MAX_FEATURES || n2 < 0 || n2 > ORBM_MAX_FEATURES ||
        (n1 > 0 && (!kps1 || !kf_mp1 || !matches1)) || (n2 > 0 && !kps2) || !T1w || !T2w || nmp < 0 ||
        (nmp > 0 && (!pts || !obs_ptr)) || !sim3_in || !os_params_ok(params) || !sim3_out || !nin || !status ||
        (a4 & 3) || ((uintptr_t)sim3_out & 7))
        return false;
    one->nobs = 0;
    if (nmp > 0) {
        if (obs_ptr[0] < 0) return false;
        for (int m = 0; m < nmp; ++m)
            if (obs_ptr[m + 1] < obs_ptr[m]) return false;
        one->nobs = obs_ptr[nmp];
        if (one->nobs > 0 && !obs) return false;
    }
    const int cap = n1 > n2 ? (n1 > 0 ? n1 : 1) : (n2 > 0 ? n2 : 1);
    one->cap = cap;
    one->kps.assign((size_t)2 * cap, orbx_keypoint{});
    one->kf_mp.assign((size_t)2 * cap, -1);
    one->m1.assign((size_t)cap, -1);
    if (n1) {
        std::memcpy(one->kps.data(), kps1, sizeof(orbx_keypoint) * (size_t)n1);
        std::memcpy(one->kf_mp.data(), kf_mp1, sizeof(int) * (size_t)n1);
        std::memcpy(one->m1.data(), matches1, sizeof(int) * (size_t)n1);
    }
    if (n2) std::memcpy(one->kps.data() + cap, kps2, sizeof(orbx_keypoint) * (size_t)n2);
    std::memcpy(one->pose, T1w, sizeof(float) * 12);
    std::memcpy(one->pose + 12, T2w, sizeof(float) * 12);
    one->counts[0] = n1;
    one->counts[1] = n2;
    return true;
}

struct OsRes {
    double sim3[8];
    float sim3f[13], scw[12];
    int nin, status;
    orbm_opt_sim3_trace tr;
};

// of an invalid pair only the status is written; the Sim3 outputs only where the reference reaches :1237
static void os_copy_out(const OsRes& r, const int* m1, int n1, int* matches1, double* sim3_out, float* sim3f_out,
                        float* scw, int* nin, orbm_opt_sim3_trace* trace, int* status)
{
    *status = r.status;
    if (r.status) return;
    *nin = r.nin;
    if (trace) *trace = r.tr;
    if (n1) std::memcpy(matches1, m1, sizeof(int) * (size_t)n1);
    if (r.tr.rounds == 2) {
        std::memcpy(sim3_out, r.sim3, sizeof(r.sim3));
        if (sim3f_out) std::memcpy(sim3f_out, r.sim3f, sizeof(r.sim3f));
        if (scw) std::memcpy(scw, r.scw, sizeof(r.scw));
    }
}

orbx_status orbm_optimize_sim3_host(const orbx_keypoint* kps1, const int* kf_mp1, int n1, const float* T1w,
                                    const orbx_keypoint* kps2, int n2, const float* T2w, const orbm_map_point* pts,
                                    int nmp, const int* obs_ptr, const orbm_observation* obs,
                                    const uint8_t* obs_erased, const float* sim3_in, int* matches1, float th2,
                                    int fix_scale, const orbm_pose_params* params, double* sim3_out, float* sim3f_out,
                                    float* scw, int* nin, orbm_opt_sim3_trace* trace, int* status)
{
    OsOne one;
    if (!os_one_ok(kps1, kf_mp1, n1, T1w, kps2, n2, T2w, pts, nmp, obs_ptr, obs, sim3_in, matches1, params, sim3_out,
                   sim3f_out, scw, nin, trace, status, &one))
        return ORBX_EINVAL;
    OsRes r;
    std::memset(&r, 0, sizeof(r));
    OsPair F;
    const OsTables T = {one.kps.data(), one.counts, 2,   one.cap, one.pose,   one.kf_mp.data(),
                        pts,            nmp,        obs_ptr, obs,   obs_erased, *params};
    F.T = &T;
    F.a = 0;
    F.b = 1;
    F.sim3_in = sim3_in;
    F.matches1 = one.m1.data();
    F.th2 = th2;
    F.fix_scale = fix_scale != 0 ? 1 : 0;
    F.sim3_out = r.sim3;
    F.sim3f_out = r.sim3f;
    F.scw = r.scw;
    F.nin = &r.nin;
    F.trace = &r.tr;
    F.status = &r.status;
    OsShared<1> S;
    os_pair<1>(S, F);
    os_copy_out(r, one.m1.data(), n1, matches1, sim3_out, sim3f_out, scw, nin, trace, status);
    return ORBX_OK;
}

orbx_status orbm_optimize_sim3(int device, const orbx_keypoint* kps1, const int* kf_mp1, int n1, const float* T1w,
                               const orbx_keypoint* kps2, int n2, const float* T2w, const orbm_map_point* pts, int nmp,
                               const int* obs_ptr, const orbm_observation* obs, const uint8_t* obs_erased,
                               const float* sim3_in, int* matches1, float th2, int fix_scale,
                               const orbm_pose_params* params, double* sim3_out, float* sim3f_out, float* scw,
                               int* nin, orbm_opt_sim3_trace* trace, int* status)
{
    OsOne one;
    if (!os_one_ok(kps1, kf_mp1, n1, T1w, kps2, n2, T2w, pts, nmp, obs_ptr, obs, sim3_in, matches1, params, sim3_out,
                   sim3f_out, scw, nin, trace, status, &one))
        return ORBX_EINVAL;
    const size_t C = (size_t)one.cap;
    const int nobs = one.nobs;
    const int head[4] = {one.counts[0], one.counts[1], 0, 1};   // counts, pair
    OsRes r;
    HostCall c(device);
    const auto okp = c.in(one.kps.data(), 2 * C);
    const auto omp = c.in(one.kf_mp.data(), 2 * C);
    const auto om1 = c.in(one.m1.data(), C);
    const auto ohd = c.in(head, 4);
    const auto opo = c.in(one.pose, 24);
    const auto osi = c.in(sim3_in, 13);
    const auto opt = c.in(pts, (size_t)nmp);
    const auto oop = c.in(nmp ? obs_ptr : nullptr, (size_t)nmp + 1);
    const auto oob = c.in(obs, (size_t)nobs);
    const auto oer = c.in(obs_erased, (size_t)nobs);
    const auto ores = c.out<OsRes>(1);
    orbx_status rc = c.begin();
    if (rc != ORBX_OK) return rc;
    OsRes* const d = c.dev(ores);
    rc = orbm_optimize_sim3_device(c.dev(okp), c.dev(ohd), 2, one.cap, c.dev(opo), c.dev(omp),
                                   nmp ? c.dev(opt) : nullptr, nmp, nmp ? c.dev(oop) : nullptr, c.dev(oob),
                                   nobs && obs_erased ? c.dev(oer) : nullptr, c.dev(ohd, 2), c.dev(ohd, 3), 1,
                                   c.dev(osi), c.dev(om1), one.cap, th2, fix_scale, params, d->sim3, d->sim3f, d->scw,
                                   &d->nin, &d->tr, &d->status, c.stream());
    if (rc != ORBX_OK) return rc;
    std::vector<int> m1(C);
    c.fetch(ores, &r, 1);
    c.fetch(om1, m1.data(), C);
    rc = c.finish();
    if (rc != ORBX_OK) return rc;
    os_copy_out(r, m1.data(), n1, matches1, sim3_out, sim3f_out, scw, nin, trace, status);
    return ORBX_OK;
}

}  // extern "C"

// Arithmetic helpers shared by the gfx950 kernels and the host.
//
// Everything here must round exactly like the reference's CPU code:
//   * cv::fastAtan2        (OpenCV 3.x atan_f32, float, no FMA)   SURVEY.md A.4
//   * glibc 2.35 cosf/sinf (sysdeps/ieee754/flt-32 sincosf.h; double
//     evaluation, table of the x86-64 libm — constants read back from the
//     host libm, algorithm verified equal to libm on every float in
//     [0, 2*pi] by tests/test_host_math.py)                          SURVEY.md A.5 / F7
// The library is compiled with -ffp-contract=off; the FMAs below are the ones
// glibc's x86-64 FMA variant forms and are written out explicitly.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define ORBX_HD __host__ __device__ __forceinline__
#else
#define ORBX_HD inline
#endif

namespace orbx {

// __sincosf_table[0] (glibc sincosf_data.c, x86-64 build without TOINT intrinsics).
// __sincosf_table[1] is the same table with the cosine coefficients c0..c4 negated, so a
// cosine polynomial evaluated through it is exactly the negation of the one below
// (negating every fma operand negates the correctly rounded result).
constexpr double kSC_hpi_inv = 0x1.45f306dc9c883p+23, kSC_hpi = 0x1.921fb54442d18p+0;
constexpr double kSC_c0 = 0x1p0, kSC_c1 = -0x1.ffffffd0c621cp-2, kSC_c2 = 0x1.55553e1068f19p-5,
                 kSC_c3 = -0x1.6c087e89a359dp-10, kSC_c4 = 0x1.99343027bf8c3p-16;
constexpr double kSC_s1 = -0x1.555545995a603p-3, kSC_s2 = 0x1.1107605230bc4p-7, kSC_s3 = -0x1.994eb3774cf24p-13;

ORBX_HD uint32_t f32_bits(float f) { union { float f; uint32_t u; } c; c.f = f; return c.u; }
ORBX_HD uint32_t abstop12(float x) { return (f32_bits(x) >> 20) & 0x7ff; }

ORBX_HD double fma_d(double a, double b, double c) { return __builtin_fma(a, b, c); }

// sinf_poly (table 0): sine polynomial
ORBX_HD float sin_poly(double x, double x2)
{
    const double x3 = x * x2;
    const double s1 = fma_d(x2, kSC_s3, kSC_s2);
    const double x7 = x3 * x2;
    const double s = fma_d(x3, kSC_s1, x);
    return (float)fma_d(x7, s1, s);
}

// sinf_poly (table 0): cosine polynomial
ORBX_HD float cos_poly(double x2)
{
    const double x4 = x2 * x2;
    const double c2 = fma_d(x2, kSC_c4, kSC_c3);
    const double c1 = fma_d(x2, kSC_c1, kSC_c0);
    const double x6 = x4 * x2;
    const double c = fma_d(x4, kSC_c2, c1);
    return (float)fma_d(x6, c2, c);
}

// glibc sinf and cosf of one argument, |y| < 120 (every BRIEF angle is in [0, 2*pi)).
// glibc's sinf(y) = sinf_poly(x*s, x*x, p, n) and cosf(y) = sinf_poly(x*s, x*x, p, n^1)
// with p = table (n & 2); the reduction is shared.
ORBX_HD void glibc_sincosf_pair(float y, float* sinv, float* cosv)
{
    const float pio4f = 0x1.921FB6p-1f;
    double x = y;
    if (abstop12(y) < abstop12(pio4f)) {
        const double x2 = x * x;
        if (abstop12(y) < abstop12(0x1p-12f)) {
            *sinv = y;
            *cosv = 1.0f;
            return;
        }
        *sinv = sin_poly(x, x2);
        *cosv = cos_poly(x2);
        return;
    }
    const double r = x * kSC_hpi_inv;
    const int n = ((int32_t)r + 0x800000) >> 24;
    x = fma_d(-(double)n, kSC_hpi, x);
    const double xs = ((n + 1) & 2) ? -x : x;   // sign[n & 3] = {1, -1, -1, 1}
    const double x2 = x * x;
    const float sp = sin_poly(xs, x2);
    const float cp = (n & 2) ? -cos_poly(x2) : cos_poly(x2);
    // n even: sinf = sine poly, cosf = cosine poly; n odd: swapped
    *sinv = (n & 1) ? cp : sp;
    *cosv = (n & 1) ? sp : cp;
}

// which = 0 -> sinf(y), 1 -> cosf(y)
ORBX_HD float glibc_sincosf(float y, int which)
{
    float s, c;
    glibc_sincosf_pair(y, &s, &c);
    return which ? c : s;
}

// cv::fastAtan2 (OpenCV 3.x), degrees in [0, 360)
ORBX_HD float fast_atan2_deg(float y, float x)
{
    const float k180pi = (float)(180 / 3.1415926535897932384626433832795);
    const float p1 = 0.9997878412794807f * k180pi;
    const float p3 = -0.3258083974640975f * k180pi;
    const float p5 = 0.1555786518463281f * k180pi;
    const float p7 = -0.04432655554792128f * k180pi;
    const float ax = x < 0 ? -x : x, ay = y < 0 ? -y : y;
    const float eps = (float)2.2204460492503131e-16;   // (float)DBL_EPSILON
    float a, c, c2;
    if (ax >= ay) {
        c = ay / (ax + eps);
        c2 = c * c;
        a = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
    } else {
        c = ax / (ay + eps);
        c2 = c * c;
        a = 90.f - (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
    }
    if (x < 0) a = 180.f - a;
    if (y < 0) a = 360.f - a;
    return a;
}

// sin(th), cos(th) and th^3 for the pose optimiser's SE3 exponential (th = |omega| >= 0; DESIGN.md §3 "Pose
// optimisation arithmetic").  A fixed sequence of double + - * that the host and the gfx950 code evaluate alike -- the
// device math library and glibc differ by an ulp, and that ulp reaches the pose.  Reduction by quadrant with a
// three-part pi/2 (k * kPO_p1 and k * kPO_p2 are exact for k < 2^20), then the published fdlibm minimax polynomials
// on [-pi/4, pi/4] without their tail corrections.  Not correctly rounded: within 1 ulp of glibc on [1e-5, 4].
constexpr double kPO_invpio2 = 6.36619772367581382433e-01;
constexpr double kPO_p1 = 1.57079632673412561417e+00, kPO_p2 = 6.07710050630396597660e-11,
                 kPO_p3 = 2.02226624871116645580e-21;
constexpr double kPO_S1 = -1.66666666666666324348e-01, kPO_S2 = 8.33333333332248946124e-03,
                 kPO_S3 = -1.98412698298579493134e-04, kPO_S4 = 2.75573137070700676789e-06,
                 kPO_S5 = -2.50507602534068634195e-08, kPO_S6 = 1.58969099521155010221e-10;
constexpr double kPO_C1 = 4.16666666666666019037e-02, kPO_C2 = -1.38888888888741095749e-03,
                 kPO_C3 = 2.48015872894767294178e-05, kPO_C4 = -2.75573143513906633035e-07,
                 kPO_C5 = 2.08757232129817482790e-09, kPO_C6 = -1.13596475577881948265e-11;

ORBX_HD void po_sincos_theta3(double th, double* sinv, double* cosv, double* th3)
{
    *th3 = th * th * th;
    const double kf = th * kPO_invpio2 + 0.5;
    const long long k = kf < 9.0e15 ? (long long)kf : 0;   // a NaN fails the comparison: 0
    const double kd = (double)k;
    const double r = ((th - kd * kPO_p1) - kd * kPO_p2) - kd * kPO_p3;
    const double z = r * r;
    const double sp =
        r + (z * r) * (kPO_S1 + z * (kPO_S2 + z * (kPO_S3 + z * (kPO_S4 + z * (kPO_S5 + z * kPO_S6)))));
    const double cr = z * (kPO_C1 + z * (kPO_C2 + z * (kPO_C3 + z * (kPO_C4 + z * (kPO_C5 + z * kPO_C6)))));
    const double cp = 1.0 - (0.5 * z - z * cr);
    switch ((int)(k & 3)) {
    case 0: *sinv = sp; *cosv = cp; break;
    case 1: *sinv = cp; *cosv = -sp; break;
    case 2: *sinv = -sp; *cosv = -cp; break;
    default: *sinv = -cp; *cosv = sp; break;
    }
}

// atan2(y, x) in double for the Sim3 solver's quaternion angle (DESIGN.md §3 "Sim3 solver arithmetic"): a fixed
// sequence of double + - * / and comparisons that the host and the gfx950 code evaluate alike, for the same reason as
// po_sincos_theta3.  The published fdlibm scheme: atan by reduction to one of five intervals (breakpoints 7/16,
// 11/16, 19/16, 39/16) with a two-part atan(0.5), atan(1), atan(1.5), atan(inf) and the degree-11 minimax
// polynomial in z = x*x split into odd and even halves; atan2 by quadrant with a two-part pi.  The exponent tests of
// fdlibm are comparisons of values here (|x| < 2^-29, |x| >= 2^66, |y/x| beyond 2^+-60 decided on the quotient), so
// inputs whose quotient over- or underflows take the limit branch.  Within 1 ulp of glibc (tests/test_sim3_solver.py).
constexpr double kAT_hi0 = 4.63647609000806093515e-01, kAT_hi1 = 7.85398163397448278999e-01,
                 kAT_hi2 = 9.82793723247329054082e-01, kAT_hi3 = 1.57079632679489655800e+00;
constexpr double kAT_lo0 = 2.26987774529616870924e-17, kAT_lo1 = 3.06161699786838301793e-17,
                 kAT_lo2 = 1.39033110312309984516e-17, kAT_lo3 = 6.12323399573676603587e-17;
constexpr double kAT_0 = 3.33333333333329318027e-01, kAT_1 = -1.99999999998764832476e-01,
                 kAT_2 = 1.42857142725034663711e-01, kAT_3 = -1.11111104054623557880e-01,
                 kAT_4 = 9.09088713343650656196e-02, kAT_5 = -7.69187620504482999495e-02,
                 kAT_6 = 6.66107313738753120669e-02, kAT_7 = -5.83357013379057348645e-02,
                 kAT_8 = 4.97687799461593236017e-02, kAT_9 = -3.65315727442169155270e-02,
                 kAT_10 = 1.62858201153657823623e-02;
constexpr double kAT_pi = 3.1415926535897931160e+00, kAT_pi_lo = 1.2246467991473531772e-16;

// atan(x), x >= 0 and not NaN
ORBX_HD double fixed_atan_pos(double x)
{
    if (x >= 73786976294838206464.0) return kAT_hi3 + kAT_lo3;   // 2^66
    if (x < 0.4375) {
        if (x < 1.862645149230957e-09) return x;                 // 2^-29
        const double z = x * x, w = z * z;
        const double s1 = z * (kAT_0 + w * (kAT_2 + w * (kAT_4 + w * (kAT_6 + w * (kAT_8 + w * kAT_10)))));
        const double s2 = w * (kAT_1 + w * (kAT_3 + w * (kAT_5 + w * (kAT_7 + w * kAT_9))));
        return x - x * (s1 + s2);
    }
    double hi, lo;
    if (x < 1.1875) {
        if (x < 0.6875) {
            hi = kAT_hi0; lo = kAT_lo0;
            x = (2.0 * x - 1.0) / (2.0 + x);
        } else {
            hi = kAT_hi1; lo = kAT_lo1;
            x = (x - 1.0) / (x + 1.0);
        }
    } else if (x < 2.4375) {
        hi = kAT_hi2; lo = kAT_lo2;
        x = (x - 1.5) / (1.0 + 1.5 * x);
    } else {
        hi = kAT_hi3; lo = kAT_lo3;
        x = -1.0 / x;
    }
    const double z = x * x, w = z * z;
    const double s1 = z * (kAT_0 + w * (kAT_2 + w * (kAT_4 + w * (kAT_6 + w * (kAT_8 + w * kAT_10)))));
    const double s2 = w * (kAT_1 + w * (kAT_3 + w * (kAT_5 + w * (kAT_7 + w * kAT_9))));
    return hi - ((x * (s1 + s2) - lo) - x);
}

ORBX_HD double fixed_atan2(double y, double x)
{
    if (x != x || y != y) return x + y;
    const bool xneg = x < 0.0 || (x == 0.0 && 1.0 / x < 0.0);
    const bool yneg = y < 0.0 || (y == 0.0 && 1.0 / y < 0.0);
    const double pio2 = kAT_hi3 + 0.5 * kAT_pi_lo;
    if (y == 0.0) {
        if (!xneg) return y;                          // atan2(+-0, +anything) = +-0
        return yneg ? -kAT_pi : kAT_pi;
    }
    if (x == 0.0) return yneg ? -pio2 : pio2;
    const double ax = xneg ? -x : x, ay = yneg ? -y : y;
    const double inf = __builtin_inf();
    double z;
    if (ax == inf) {
        z = ay == inf ? (xneg ? 3.0 * kAT_hi1 : kAT_hi1) : (xneg ? kAT_pi : 0.0);
        return yneg ? -z : z;
    }
    if (ay == inf) return yneg ? -pio2 : pio2;
    const double q = ay / ax;
    if (q > 1152921504606846976.0) z = pio2;                       // 2^60
    else if (xneg && q < 8.673617379884035e-19) z = 0.0;           // 2^-60
    else z = fixed_atan_pos(q);
    if (!xneg) return yneg ? -z : z;
    return yneg ? (z - kAT_pi_lo) - kAT_pi : kAT_pi - (z - kAT_pi_lo);
}

// acosf(x) for the Initializer's parallax angle (DESIGN.md §3 "Initializer arithmetic"): a fixed sequence of double
// * + and one sqrt that the host and the gfx950 code evaluate alike, rounded to float once.  Abramowitz & Stegun,
// Handbook of Mathematical Functions, 4.4.46 (from Hastings, Approximations for Digital Computers): for 0 <= x <= 1,
// arccos x = sqrt(1 - x) * (a0 + a1 x + ... + a7 x^7) + e(x), |e(x)| <= 2 x 10^-8 (stated to one digit: a0 itself is
// 2.18e-8 below pi / 2); arccos(-x) = pi - arccos x.  |x| > 1 and NaN give NaN (the square root of a negative number).
constexpr double kAC_0 = 1.5707963050, kAC_1 = -0.2145988016, kAC_2 = 0.0889789874, kAC_3 = -0.0501743046,
                 kAC_4 = 0.0308918810, kAC_5 = -0.0170881256, kAC_6 = 0.0066700901, kAC_7 = -0.0012624911;

ORBX_HD float fixed_acosf(float xf)
{
    const double x = (double)xf;
    const double a = x < 0.0 ? -x : x;
    const double p =
        kAC_0 + a * (kAC_1 + a * (kAC_2 + a * (kAC_3 + a * (kAC_4 + a * (kAC_5 + a * (kAC_6 + a * kAC_7))))));
    const double r = __builtin_sqrt(1.0 - a) * p;
    return (float)(x < 0.0 ? kAT_pi - r : r);
}

// exp(x) in double for the Sim3 optimiser's scale update (DESIGN.md §3 "Sim3 optimisation arithmetic"): a fixed
// sequence of double + - * / that the host and the gfx950 code evaluate alike, for the same reason as
// po_sincos_theta3.  The published fdlibm scheme: k = the integer nearest x / ln2 (0 for |x| <= ln2 / 2), r = (x -
// k * ln2_hi) - k * ln2_lo with a two-part ln2 (k * ln2_hi is exact for |k| < 2^11), the degree-5 minimax polynomial
// in r * r, and the result scaled by 2^k built from its exponent bits.  |x| < 2^-28 gives 1 + x, so fixed_exp(0) is
// exactly 1.  Domain [-708, 709]: above it +inf, below it 0 (no subnormal results), NaN gives NaN.  Within 1 ulp of
// glibc on [-5, 5] (tests/test_optimize_sim3.py).
constexpr double kEX_ln2hi = 6.93147180369123816490e-01, kEX_ln2lo = 1.90821492927058770002e-10,
                 kEX_invln2 = 1.44269504088896338700e+00;
constexpr double kEX_P1 = 1.66666666666666019037e-01, kEX_P2 = -2.77777777770155933842e-03,
                 kEX_P3 = 6.61375632143793436117e-05, kEX_P4 = -1.65339022054652515390e-06,
                 kEX_P5 = 4.13813679705723846039e-08;

ORBX_HD double fixed_exp(double x)
{
    if (x != x) return x;
    if (x > 709.0) return __builtin_inf();
    if (x < -708.0) return 0.0;
    const double ax = x < 0.0 ? -x : x;
    double hi = x, lo = 0.0;
    long long k = 0;
    if (ax > 0.5 * (kEX_ln2hi + kEX_ln2lo)) {
        k = (long long)(kEX_invln2 * x + (x < 0.0 ? -0.5 : 0.5));
        const double t = (double)k;
        hi = x - t * kEX_ln2hi;
        lo = t * kEX_ln2lo;
    } else if (ax < 3.7252902984619140625e-09) {   // 2^-28
        return 1.0 + x;
    }
    const double r = hi - lo;
    const double t = r * r;
    const double c = r - t * (kEX_P1 + t * (kEX_P2 + t * (kEX_P3 + t * (kEX_P4 + t * kEX_P5))));
    if (k == 0) return 1.0 - ((r * c) / (c - 2.0) - r);
    const double y = 1.0 - ((lo - (r * c) / (2.0 - c)) - hi);
    union { uint64_t u; double d; } two_k;
    two_k.u = (uint64_t)(1023 + k) << 52;   // k in [-1022, 1023] on the domain
    return y * two_k.d;
}

// (float)(CV_PI/180.f), src/ORBextractor.cc:131
constexpr float kFactorPI = (float)(3.1415926535897932384626433832795 / 180.f);

}  // namespace orbx

// tanh and atanh exactly as glibc's libm (2.35, dbl-64) computes them: the
// fdlibm algorithms (expm1, log1p) with glibc's evaluation order of the two
// polynomials, in plain IEEE double operations (no fma: the build sets
// -ffp-contract=off; fp64 division is correctly rounded).  The oracle's BP
// (oracle/refcpu.c) calls libm's tanh / atanh, and on non-converging frames a
// single last-bit difference in one message can decide bits many iterations
// later, so the generic kernel (ldpc_decode_kernel), which has to decode any
// code like the oracle, uses these; the kernels of the BASELINE codes keep the
// lean <= 4 ulp forms of ldpc.hip.  Compared with libm on 20 M arguments
// (|x| over 1e-17 .. 30 for tanh, |x| <= 0.999999 for atanh): every result
// bit-identical.
#pragma once
#include "common.hpp"

namespace pl {

PL_DEV uint32_t f64_hi(double x) { return (uint32_t)((uint64_t)__double_as_longlong(x) >> 32); }
PL_DEV double f64_with_hi(double x, uint32_t h) {
    return __longlong_as_double((long long)(((uint64_t)__double_as_longlong(x) & 0xffffffffull) | ((uint64_t)h << 32)));
}

// expm1(x), x finite and |x| < 56 ln2 (s_expm1.c)
PL_DEV double libm_expm1(double x) {
    constexpr double ln2_hi = 6.93147180369123816490e-01, ln2_lo = 1.90821492927058770002e-10,
                     invln2 = 1.44269504088896338700e+00;
    constexpr double Q1 = -3.33333333333331316428e-02, Q2 = 1.58730158725481460165e-03,
                     Q3 = -7.93650757867487942473e-05, Q4 = 4.00821782732936239552e-06,
                     Q5 = -2.01099218183624371326e-07;
    double y, hi, lo, c = 0.0, t, e;
    int32_t k;
    uint32_t hx = f64_hi(x);
    const bool neg = (hx >> 31) != 0;
    hx &= 0x7fffffffu;
    if (hx >= 0x4043687Au && neg) return 1e-300 - 1.0;  // x <= -56 ln2
    if (hx > 0x3fd62e42u) {                             // |x| > 0.5 ln2
        if (hx < 0x3FF0A2B2u) {                         // and < 1.5 ln2
            hi = neg ? x + ln2_hi : x - ln2_hi;
            lo = neg ? -ln2_lo : ln2_lo;
            k = neg ? -1 : 1;
        } else {
            k = (int32_t)(invln2 * x + (neg ? -0.5 : 0.5));
            t = k;
            hi = x - t * ln2_hi;
            lo = t * ln2_lo;
        }
        x = hi - lo;
        c = (hi - x) - lo;
    } else if (hx < 0x3c900000u) {
        return x;
    } else {
        k = 0;
    }
    const double hfx = 0.5 * x, hxs = x * hfx;
    const double R1 = 1.0 + hxs * Q1, h2 = hxs * hxs, R2 = Q2 + hxs * Q3, h4 = h2 * h2, R3 = Q4 + hxs * Q5;
    const double r1 = R1 + h2 * R2 + h4 * R3;
    t = 3.0 - r1 * hfx;
    e = hxs * ((r1 - t) / (6.0 - x * t));
    if (k == 0) return x - (x * e - hxs);
    e = (x * (e - c) - c);
    e -= hxs;
    if (k == -1) return 0.5 * (x - e) - 0.5;
    if (k == 1) return x < -0.25 ? -2.0 * (e - (x + 0.5)) : 1.0 + 2.0 * (x - e);
    if (k <= -2 || k > 56) {
        y = 1.0 - (e - x);
        y = f64_with_hi(y, f64_hi(y) + ((uint32_t)k << 20));
        return y - 1.0;
    }
    if (k < 20) {
        t = f64_with_hi(1.0, 0x3ff00000u - (0x200000u >> k));  // 1 - 2^-k
        y = t - (e - x);
    } else {
        t = f64_with_hi(1.0, (uint32_t)(0x3ff - k) << 20);  // 2^-k
        y = x - (e + t);
        y += 1.0;
    }
    return f64_with_hi(y, f64_hi(y) + ((uint32_t)k << 20));
}

// tanh(x), any x (s_tanh.c)
PL_DEV double libm_tanh(double x) {
    const uint32_t jx = f64_hi(x), ix = jx & 0x7fffffffu;
    const bool neg = (jx >> 31) != 0;
    if (ix >= 0x7ff00000u) return neg ? 1.0 / x - 1.0 : 1.0 / x + 1.0;  // +-1 for +-inf, NaN for NaN
    double z = 1.0;                                                     // |x| >= 22
    if (ix < 0x40360000u) {
        if (x == 0.0) return x;
        if (ix < 0x3c800000u) return x * (1.0 + x);  // |x| < 2^-55
        const double ax = fabs(x);
        if (ix >= 0x3ff00000u) {
            const double t = libm_expm1(2.0 * ax);
            z = 1.0 - 2.0 / (t + 2.0);
        } else {
            const double t = libm_expm1(-2.0 * ax);
            z = -t / (t + 2.0);
        }
    }
    return neg ? -z : z;
}

// log1p(x), 0 <= x < 2^53 (s_log1p.c)
PL_DEV double libm_log1p_pos(double x) {
    constexpr double ln2_hi = 6.93147180369123816490e-01, ln2_lo = 1.90821492927058770002e-10;
    constexpr double Lp1 = 6.666666666666735130e-01, Lp2 = 3.999999999940941908e-01, Lp3 = 2.857142874366239149e-01,
                     Lp4 = 2.222219843214978396e-01, Lp5 = 1.818357216161805012e-01, Lp6 = 1.531383769920937332e-01,
                     Lp7 = 1.479819860511658591e-01;
    double f, c = 0.0;
    int32_t k = 0, hu = 1;
    const int32_t hx = (int32_t)f64_hi(x);
    if (hx < 0x3FDA827A) {  // x < 0.41422
        if (hx < 0x3e200000) return hx < 0x3c900000 ? x : x - x * x * 0.5;  // x < 2^-29
        f = x;
    } else {
        double u = 1.0 + x;
        hu = (int32_t)f64_hi(u);
        k = (hu >> 20) - 1023;
        c = (k > 0) ? 1.0 - (u - x) : x - (u - 1.0);
        c /= u;
        hu &= 0x000fffff;
        if (hu < 0x6a09e) {
            u = f64_with_hi(u, (uint32_t)hu | 0x3ff00000u);
        } else {
            k += 1;
            u = f64_with_hi(u, (uint32_t)hu | 0x3fe00000u);
            hu = (0x00100000 - hu) >> 2;
        }
        f = u - 1.0;
    }
    const double hfsq = 0.5 * f * f;
    if (hu == 0) {  // |f| < 2^-20
        if (f == 0.0) {
            if (k == 0) return 0.0;
            c += k * ln2_lo;
            return k * ln2_hi + c;
        }
        const double R = hfsq * (1.0 - 0.66666666666666666 * f);
        return k == 0 ? f - R : k * ln2_hi - ((R - (k * ln2_lo + c)) - f);
    }
    const double s = f / (2.0 + f), z = s * s;
    const double R1 = z * Lp1, z2 = z * z, R2 = Lp2 + z * Lp3, z4 = z2 * z2, R3 = Lp4 + z * Lp5, z6 = z4 * z2,
                 R4 = Lp6 + z * Lp7;
    const double R = R1 + z2 * R2 + z4 * R3 + z6 * R4;
    if (k == 0) return f - (hfsq - s * (hfsq + R));
    return k * ln2_hi - ((hfsq - (s * (hfsq + R) + (k * ln2_lo + c))) - f);
}

// atanh(x), |x| < 1 or NaN (e_atanh.c)
PL_DEV double libm_atanh(double x) {
    const double xa = fabs(x);
    double t;
    if (xa < 0.5) {
        if (xa < 0x1.0p-28) return x;
        t = xa + xa;
        t = 0.5 * libm_log1p_pos(t + t * xa / (1.0 - xa));
    } else if (xa < 1.0) {
        t = 0.5 * libm_log1p_pos((xa + xa) / (1.0 - xa));
    } else {
        return (x - x) / (x - x);  // NaN
    }
    return __builtin_copysign(t, x);
}

}  // namespace pl

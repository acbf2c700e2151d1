"""expm1 and log1p as glibc 2.35's dbl-64 libm computes them, vectorised in plain NumPy operations.

np.expm1 / np.log1p are whatever the NumPy build dispatches to (SIMD paths whose last bits differ from
glibc's), and math.expm1 / math.log1p are the C library of the machine that runs them.  The exact log-MAP
demapper (include/polarldpc.h at pl_qam_demap_logmap) is defined on glibc's results, so the host definition
carries the two algorithms itself: s_expm1.c and s_log1p.c (fdlibm, with glibc's evaluation order of the
polynomials), every step one IEEE double operation in the order of csrc/libm_exact.hpp, every branch computed
for every element and selected.

Domains, those of the demapper: expm1 for x <= 0, -inf (-> -1.0) and NaN (-> NaN); log1p for 0 <= x < 2^53 and
NaN (-> NaN).  Outside them an AssertionError.
"""
from __future__ import annotations

import numpy as np

LN2_HI = 6.93147180369123816490e-01
LN2_LO = 1.90821492927058770002e-10
INVLN2 = 1.44269504088896338700e+00
Q1, Q2, Q3, Q4, Q5 = (-3.33333333333331316428e-02, 1.58730158725481460165e-03, -7.93650757867487942473e-05,
                      4.00821782732936239552e-06, -2.01099218183624371326e-07)
LP1, LP2, LP3, LP4, LP5, LP6, LP7 = (6.666666666666735130e-01, 3.999999999940941908e-01, 2.857142874366239149e-01,
                                     2.222219843214978396e-01, 1.818357216161805012e-01, 1.531383769920937332e-01,
                                     1.479819860511658591e-01)


def _hi(x: np.ndarray) -> np.ndarray:
    """the high 32 bits of each double, as int64"""
    return (x.view(np.uint64) >> np.uint64(32)).astype(np.int64)


def _with_hi(x: np.ndarray, h: np.ndarray) -> np.ndarray:
    """x with its high 32 bits replaced by h (int64, 0 .. 2^32 - 1)"""
    return ((x.view(np.uint64) & np.uint64(0xFFFFFFFF)) | (h.astype(np.uint64) << np.uint64(32))).view(np.float64)


def expm1(x) -> np.ndarray:
    """glibc's expm1 on x <= 0, -inf and NaN; float64 in, float64 out, any shape"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    nan = np.isnan(x)
    assert not np.any(x[~nan] > 0.0), "expm1 here takes x <= 0, -inf or NaN"
    hx = _hi(x) & 0x7FFFFFFF
    const = (hx >= 0x4043687A) & ~nan  # x <= -56 ln 2: tiny - 1.0
    tiny = (hx < 0x3C900000)  # |x| < 2^-54: x itself
    v = np.where(const | nan | tiny, -1.0, x)  # the lanes the arithmetic below decides; the others are overwritten
    hv = _hi(v) & 0x7FFFFFFF
    red = hv > 0x3FD62E42  # |x| > 0.5 ln 2
    near = red & (hv < 0x3FF0A2B2)  # and < 1.5 ln 2: k = -1
    with np.errstate(all="ignore"):
        kf = np.trunc(INVLN2 * v + -0.5)  # (int)(...): toward zero
        k = np.where(near, -1, np.where(red, kf, 0.0)).astype(np.int64)
        t = k.astype(np.float64)
        hi = np.where(near, v + LN2_HI, v - t * LN2_HI)
        lo = np.where(near, -LN2_LO, t * LN2_LO)
        xr = np.where(red, hi - lo, v)
        c = np.where(red, (hi - xr) - lo, 0.0)
        hfx = 0.5 * xr
        hxs = xr * hfx
        R1 = 1.0 + hxs * Q1
        h2 = hxs * hxs
        R2 = Q2 + hxs * Q3
        h4 = h2 * h2
        R3 = Q4 + hxs * Q5
        r1 = (R1 + h2 * R2) + h4 * R3
        t = 3.0 - r1 * hfx
        e = hxs * ((r1 - t) / (6.0 - xr * t))
        k0 = xr - (xr * e - hxs)
        e = xr * (e - c) - c
        e = e - hxs
        km1 = 0.5 * (xr - e) - 0.5
        y = 1.0 - (e - xr)  # k <= -2: exp(x) - 1 from y 2^k, the k added into the exponent field
        y = (y.view(np.int64) + (np.where(k <= -2, k, 0) << 52)).view(np.float64)
        far = y - 1.0
        out = np.where(k == 0, k0, np.where(k == -1, km1, far))
        out = np.where(tiny, x, out)
        out = np.where(const, -1.0, out)
        out = np.where(nan, x + x, out)
    return out


def log1p(x) -> np.ndarray:
    """glibc's log1p on 0 <= x < 2^53 and NaN; float64 in, float64 out, any shape"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    nan = np.isnan(x)
    assert not np.any(x[~nan] < 0.0) and not np.any(x[~nan] >= 2.0 ** 53), "log1p here takes 0 <= x < 2^53 or NaN"
    v = np.where(nan, 1.0, x)
    hx = _hi(v)
    small = hx < 0x3FDA827A  # x < sqrt(2) - 1
    tiny = hx < 0x3E200000  # x < 2^-29
    with np.errstate(all="ignore"):
        tiny_out = np.where(hx < 0x3C900000, v, v - (v * v) * 0.5)
        u = 1.0 + v
        hu = _hi(u)
        k = (hu >> 20) - 1023
        c = np.where(k > 0, 1.0 - (u - v), v - (u - 1.0))
        c = c / u
        hu = hu & 0x000FFFFF
        low = hu < 0x6A09E
        u = np.where(low, _with_hi(u, hu | 0x3FF00000), _with_hi(u, hu | 0x3FE00000))
        k = np.where(low, k, k + 1)
        hu = np.where(low, hu, (0x00100000 - hu) >> 2)
        f = np.where(small, v, u - 1.0)
        k = np.where(small, 0, k)
        hu = np.where(small, 1, hu)
        c = np.where(small, 0.0, c)
        kd = k.astype(np.float64)
        hfsq = (0.5 * f) * f
        # hu == 0: |f| < 2^-20
        z_f0 = np.where(k == 0, 0.0, kd * LN2_HI + (c + kd * LN2_LO))
        R = hfsq * (1.0 - 0.66666666666666666 * f)
        z_f = np.where(k == 0, f - R, kd * LN2_HI - ((R - (kd * LN2_LO + c)) - f))
        z_out = np.where(f == 0.0, z_f0, z_f)
        s = f / (2.0 + f)
        z = s * s
        R1 = z * LP1
        z2 = z * z
        R2 = LP2 + z * LP3
        z4 = z2 * z2
        R3 = LP4 + z * LP5
        z6 = z4 * z2
        R4 = LP6 + z * LP7
        R = ((R1 + z2 * R2) + z4 * R3) + z6 * R4
        gen = np.where(k == 0, f - (hfsq - s * (hfsq + R)),
                       kd * LN2_HI - ((hfsq - (s * (hfsq + R) + (kd * LN2_LO + c))) - f))
        out = np.where(hu == 0, z_out, gen)
        out = np.where(tiny, tiny_out, out)
        out = np.where(nan, x + x, out)
    return out

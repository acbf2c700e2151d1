"""The exact log-MAP demapper (include/polarldpc.h at pl_qam_demap_logmap) restated as plain loops.

Independent of the package and of the library, as qam_ref is: Python floats (IEEE doubles), one operation a
step, loops over frames, bits and levels, with math.expm1 / math.log1p -- the C library's, which is glibc 2.35's
on the machines the fixture tests/golden/libm_expm1_log1p.json was made on.  libm_is_the_fixtures() says whether
this machine's math.* reproduces that fixture; the tests that use these loops skip where it does not.
"""
import functools
import json
import math
import os

import numpy as np

import qam_ref as Q

FIXTURE = os.path.join(os.path.dirname(__file__), "golden", "libm_expm1_log1p.json")
SKIP_REASON = "this machine's math.expm1 / math.log1p are not glibc 2.35's: they disagree with " \
              "tests/golden/libm_expm1_log1p.json on the fixture's own arguments"


@functools.lru_cache(maxsize=None)
def fixture():
    """{"expm1": (args, results), "log1p": (args, results)} as float64 arrays"""
    with open(FIXTURE) as f:
        raw = json.load(f)
    return {k: (np.array([float.fromhex(a) for a, _ in raw[k]]), np.array([float.fromhex(r) for _, r in raw[k]]))
            for k in ("expm1", "log1p")}


@functools.lru_cache(maxsize=None)
def libm_is_the_fixtures():
    for name, fn in (("expm1", math.expm1), ("log1p", math.log1p)):
        args, want = fixture()[name]
        got = np.array([fn(float(a)) for a in args])
        if not np.array_equal(got.view(np.uint64), want.view(np.uint64)):
            return False
    return True


def expm1(x):
    """math.expm1 with the definition's extensions: -inf -> -1.0, NaN -> NaN"""
    if x != x:
        return x
    if x == -math.inf:
        return -1.0
    return math.expm1(x)


def log1p(x):
    return x if x != x else math.log1p(x)


def axis_llr(r, table, p, W):
    """the LLR of axis bit p of the axis value r at weight W; table: [(x_a, bits)] in ascending level index"""
    d = []
    for xa, ab in table:
        t = r - xa
        d.append((t * t, ab[p]))
    D, c = [], []
    for v in (0, 1):
        Dv = Q._min(x for x, bit in d if bit == v)
        T = 0.0
        for x, bit in d:
            if bit == v:
                q = (Dv - x) * W
                e = expm1(q) + 1.0
                T = T + e
        D.append(Dv)
        c.append(log1p(T - 1.0))
    return ((D[1] - D[0]) * W) + (c[0] - c[1])


def level_table(m):
    """[(x_a, bits)] by level index: index 0 the largest level"""
    hb, sc = m // 2, Q.scale_of(m)
    return [(float(a) * sc, b) for a, b in sorted(Q.axis_table(hb), key=lambda ab: -ab[0])]


def demap(y, E, m, sigma, dtype=np.float64):
    """y [B][>= 2 S] -> LLRs [B, E] of dtype, by the definition's operations on Python floats"""
    table = level_table(m)
    s2 = sigma * sigma
    w = 1.0 / (2.0 * s2)
    y = np.asarray(y, dtype=np.float64)
    B = y.shape[0]
    out = np.zeros((B, E), dtype=np.float64)
    for b in range(B):
        for t in range(E):
            s, i = divmod(t, m)
            out[b, t] = axis_llr(float(y[b, 2 * s + (i & 1)]), table, i // 2, w)
    with np.errstate(over="ignore"):
        return out.astype(dtype)


def demap_csi(y, h, E, m, sigma, Lc, dtype=np.float64):
    """y [B][>= 2 S], h [B][>= 2 Q] -> LLRs [B, E] of dtype, by the definition's operations on Python floats"""
    table = level_table(m)
    s2 = sigma * sigma
    w = 1.0 / (2.0 * s2)
    y, h = np.asarray(y, dtype=np.float64), np.asarray(h, dtype=np.float64)
    B = y.shape[0]
    out = np.zeros((B, E), dtype=np.float64)
    for b in range(B):
        for t in range(E):
            s, i = divmod(t, m)
            q = s // Lc
            hr, hi = float(h[b, 2 * q]), float(h[b, 2 * q + 1])
            yi, yq = float(y[b, 2 * s]), float(y[b, 2 * s + 1])
            g = hr * hr + hi * hi
            if g == 0.0:
                out[b, t] = 0.0  # the erased symbol: +0.0
                continue
            if i & 1:
                u = hr * yq - hi * yi
            else:
                u = hr * yi + hi * yq
            out[b, t] = axis_llr(u / g, table, i // 2, w * g)
    with np.errstate(over="ignore"):
        return out.astype(dtype)


# ---- the a-posteriori LLR in mpmath, and the bound on the definition's distance from it ----
def exact_mp(r, table, p, W):
    """log sum_{bit 0} e^(-W d_a) - log sum_{bit 1} e^(-W d_a) at 100 digits, from the doubles r, x_a and W"""
    import mpmath
    with mpmath.workdps(100):
        rr, WW = mpmath.mpf(r), mpmath.mpf(W)
        s = [mpmath.mpf(0), mpmath.mpf(0)]
        dmin = min((rr - mpmath.mpf(xa)) ** 2 for xa, _ in table)  # a common shift: no underflow to zero
        for xa, ab in table:
            s[ab[p]] += mpmath.exp(-WW * ((rr - mpmath.mpf(xa)) ** 2 - dmin))
        return mpmath.log(s[0]) - mpmath.log(s[1])


def logmap_bound_mp(r, table, p, W):
    """A bound on |llr - exact_mp| for finite inputs without overflow, in mpmath, from the operation count.

    With u = 2^-53 (half an ulp, relative, of every correctly rounded operation) and 1 ulp = 2 u for the two
    functions (glibc documents both below 1 ulp):
      d_a = t * t, t = r - x_a:  t carries u |t|, so d_a carries (2 u + u) d_a = 3 u d_a  (second order dropped
                     here and below, and paid for by the factor at the end)
      D_v - d_a      the operands' errors 3 u (D_v + d_a) and u of the result; with the product by W, one more u:
                     |delta q| <= u W (3 (D_v + d_a) + 2 (d_a - D_v)) =: dq_a
      e_a = expm1(q) + 1.0:  relative to e_a = e^q <= 1: dq_a from the argument, 2 u of expm1's own (its
                     absolute error 2 u |expm1 q| <= 2 u), u of the addition: |delta e_a| <= e_a dq_a + 3 u
      T_v            n = 2^(h-1) terms, each sum rounds once, T <= n: |delta T| <= sum_a |delta e_a| + (n - 1) u T
      T_v - 1.0      exact or u (T - 1): + u (T - 1)
      c_v = log1p(T - 1):  d/dx log1p(x) = 1 / T: |delta T| / T, and 2 u c_v of the function
      (D_1 - D_0) W  3 u (D_1 + D_0) W from the operands, 2 u |D_1 - D_0| W from the two operations
      c_0 - c_1 and the final sum: u |c_0 - c_1| + u |llr|
    The dropped second-order terms are products of two of these relative errors, each at most u W d_a < 2^-20 on
    the demapper's range, so the bound is that sum times (1 + 2^-20)."""
    import mpmath
    with mpmath.workdps(100):
        u = mpmath.mpf(2) ** -53
        rr, WW = mpmath.mpf(r), mpmath.mpf(W)
        d = [((rr - mpmath.mpf(xa)) ** 2, ab[p]) for xa, ab in table]
        total = mpmath.mpf(0)
        D, c = [], []
        for v in (0, 1):
            dv = [x for x, bit in d if bit == v]
            Dv = min(dv)
            T = mpmath.mpf(0)
            dT = mpmath.mpf(0)
            for x in dv:
                e = mpmath.exp(-WW * (x - Dv))
                dq = u * WW * (3 * (Dv + x) + 2 * (x - Dv))
                T += e
                dT += e * dq + 3 * u
            dT += (len(dv) - 1) * u * T + u * (T - 1)
            cv = mpmath.log(T)
            total += dT / T + 2 * u * cv
            D.append(Dv)
            c.append(cv)
        ml = (D[1] - D[0]) * WW
        total += 3 * u * (D[1] + D[0]) * WW + 2 * u * abs(ml)
        total += u * abs(c[0] - c[1]) + u * abs(ml + c[0] - c[1])
        return total * (1 + mpmath.mpf(2) ** -20)

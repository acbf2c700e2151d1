"""The Gray-mapped QAM definition (include/polarldpc.h at pl_qam_check) restated as plain loops.

Independent of the package and of the library: Python floats (IEEE doubles), one operation
a step, loops over symbols, bits and levels.  The noise is the stream contract's, through
channel_ref's Philox, uniforms and mpmath normals (imported, not copied), at the QAM
source's counter (s, f_lo, f_hi, 0x9A3A9A3A) with the AWGN key.
"""
import math

import numpy as np

import channel_ref as R

SALT_QAM = 0x9A3A9A3A
MS = (2, 4, 6, 8)


def scale_of(m):
    h = m // 2
    D = 2 * (4 ** h - 1) // 3
    assert 3 * D == 2 * (4 ** h - 1)
    return 1.0 / math.sqrt(float(D))


def axis_level(b):
    """integer level of the axis bits b_0, b_1, ...: c_0 = b_0, c_p = c_(p-1) ^ b_p, idx = sum c_p 2^(h-1-p)"""
    h = len(b)
    c, idx = 0, 0
    for p in range(h):
        c = c ^ (int(b[p]) & 1)
        idx += c << (h - 1 - p)
    return (2 ** h - 1) - 2 * idx


def axis_table(h):
    """[(level, bits)] of every pattern of h axis bits"""
    out = []
    for v in range(2 ** h):
        b = [(v >> (h - 1 - p)) & 1 for p in range(h)]
        out.append((axis_level(b), b))
    return out


def modulate(bits, m):
    """bits [B][E] -> float64 [B, 2 S]"""
    h, sc = m // 2, scale_of(m)
    bits = np.asarray(bits)
    B, E = bits.shape
    S = -(-E // m)
    x = np.zeros((B, 2 * S), dtype=np.float64)
    for b in range(B):
        for s in range(S):
            for axis in range(2):
                ab = []
                for p in range(h):
                    t = s * m + 2 * p + axis
                    ab.append(int(bits[b, t]) & 1 if t < E else 0)
                x[b, 2 * s + axis] = float(axis_level(ab)) * sc
    return x


def _min(vals):
    it = iter(vals)
    best = next(it)
    for v in it:
        if v < best:
            best = v
    return best  # every value is NaN or none is


def demap(y, E, m, sigma, dtype=np.float64):
    """y [B][>= 2 S] -> LLRs [B, E] of dtype, by the definition's operations on Python floats"""
    h, sc = m // 2, scale_of(m)
    table = [(float(a) * sc, b) for a, b in axis_table(h)]
    s2 = sigma * sigma
    w = 1.0 / (2.0 * s2)
    y = np.asarray(y, dtype=np.float64)
    B = y.shape[0]
    out = np.zeros((B, E), dtype=np.float64)
    for b in range(B):
        for t in range(E):
            s, i = divmod(t, m)
            r = float(y[b, 2 * s + (i & 1)])
            p = i // 2
            d = []
            for xa, ab in table:
                tt = r - xa
                d.append((tt * tt, ab[p]))
            d0 = _min(v for v, bit in d if bit == 0)
            d1 = _min(v for v, bit in d if bit == 1)
            out[b, t] = (d1 - d0) * w
    return out.astype(dtype)


# ---- noise ----
def qam_ints(seed, frame_offset, batch, S):
    """(ia, ic) uint64 [batch, S] of the symbols' Box-Muller pairs"""
    return R.uniform_ints(np.arange(S)[None, :], R._frames(frame_offset, batch), SALT_QAM, R.noise_key(seed))


def qam_normals_mp(seed, frame_offset, batch, S):
    """z [batch, 2 S] object array of mpf: z0 -> I, z1 -> Q of each symbol"""
    z0, z1 = R.normals_mp(*qam_ints(seed, frame_offset, batch, S))
    return R.interleave(z0, z1, 2 * S)


def qam_normals_np(seed, frame_offset, batch, S):
    z0, z1 = R.normals_np(*qam_ints(seed, frame_offset, batch, S))
    return R.interleave(z0, z1, 2 * S)


def qam_awgn_mp(x, z, sigma):
    """y = x + sigma z on object arrays; x float64 (exact), sigma a double"""
    return R.to_mp(x) + z * R.MP.mpf(sigma)


def qam_awgn_bound_mp(x, z, sigma):
    """|y_dev - y_exact| <= 2^-52 (8 sigma |z| + |x| + sigma |z|).

    The first-order propagation of channel_ref.awgn_bound_mp: sigma z carries 8 eps of
    sigma |z| (log 3, sqrt 2, cospi / sinpi 4, the two products 1/2 each: 7, and one for
    the second-order terms); x = a scale is the definition's own double, exact here; the
    one addition rounds once, half an eps of |y| <= |x| + sigma |z|, stated as one."""
    az = abs(z) * R.MP.mpf(sigma)
    return (az * 8 + abs(R.to_mp(x)) + az) * R.MP.mpf(R.EPS)


# ---- exact hard-decision error probability of each axis bit ----
def pam_bit_error_prob(h, sigma):
    """[P(bit p decided wrong)] for p = 0 .. h-1 on one axis of the 2^h-level Gray PAM at noise sigma.

    The max-log LLR's sign is the bit of the nearest level, so the decision thresholds lie at the
    midpoints between neighbouring levels.  Each transmitted level contributes the Gaussian mass of
    the intervals whose level carries the other bit, as differences of 0.5 erfc; the levels are
    equally likely."""
    sc = scale_of(2 * h)
    tab = sorted((float(a) * sc, b) for a, b in axis_table(h))  # ascending amplitude
    L = len(tab)
    edges = [-math.inf] + [(tab[i][0] + tab[i + 1][0]) / 2 for i in range(L - 1)] + [math.inf]

    def q(v):  # P(N(0, sigma) > v)
        return 0.5 * math.erfc(v / (sigma * math.sqrt(2.0)))
    out = []
    for p in range(h):
        tot = 0.0
        for xa, ba in tab:
            for j, (_, bj) in enumerate(tab):
                if bj[p] != ba[p]:
                    tot += q(edges[j] - xa) - q(edges[j + 1] - xa)
        out.append(tot / L)
    return out


def snr_for_error_rate(h, lo=1e-2, hi=1e-1):
    """The first Es/N0 on the 0.5 dB grid, coming down from 40 dB, at which pam_bit_error_prob averages
    inside (lo, hi); the average of that point is at least 2 lo."""
    snr = 40.0
    while snr > -20.0:
        avg = sum(pam_bit_error_prob(h, R.sigma_of(snr))) / h
        if 2 * lo <= avg < hi:
            return snr
        snr -= 0.5
    raise AssertionError("no Es/N0 with an average error rate in range")

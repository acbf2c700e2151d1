"""The block Rayleigh fading definition (include/polarldpc.h at pl_qam_fading_check) restated as plain loops.

Independent of the package and of the library, as qam_ref is: Python floats (IEEE doubles), one
operation a step, loops over frames, symbols and bits.  The coefficients are the stream contract's,
through channel_ref's Philox, uniforms and mpmath normals (imported, not copied), at the counter
(q, f_lo, f_hi, 0xFADE9A3A) with the AWGN key; the constellation table and the minima are qam_ref's.
"""
import math

import numpy as np

import channel_ref as R
import qam_ref as Q

SALT_FADE = 0xFADE9A3A
C = float.fromhex("0x1.6a09e667f3bcdp-1")  # the double nearest 1 / sqrt(2)
LC_FRAME = 2 ** 30


def blocks(S, Lc):
    return -(-S // Lc)


def fade(x, h, noise, Lc):
    """y [B, 2 S] = h x + noise: x, noise [B][2 S] (noise is sigma z), h [B][>= 2 Q] with Re, Im interleaved;
    symbol s takes block s // Lc.  Each step one operation, in the definition's order."""
    x, h, noise = (np.asarray(a, dtype=np.float64) for a in (x, h, noise))
    B, S = x.shape[0], x.shape[1] // 2
    y = np.zeros((B, 2 * S), dtype=np.float64)
    for b in range(B):
        for s in range(S):
            q = s // Lc
            hr, hi = float(h[b, 2 * q]), float(h[b, 2 * q + 1])
            xi, xq = float(x[b, 2 * s]), float(x[b, 2 * s + 1])
            a = hr * xi
            c = hi * xq
            y[b, 2 * s] = (a - c) + float(noise[b, 2 * s])
            a = hr * xq
            c = hi * xi
            y[b, 2 * s + 1] = (a + c) + float(noise[b, 2 * s + 1])
    return y


def demap_csi(y, h, E, m, sigma, Lc, dtype=np.float64):
    """y [B][>= 2 S], h [B][>= 2 Q] -> LLRs [B, E] of dtype, by the definition's operations on Python floats"""
    hb, sc = m // 2, Q.scale_of(m)
    table = [(float(a) * sc, b) for a, b in Q.axis_table(hb)]
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
            r = u / g  # g != 0.0: Python's float division is the IEEE one (inf and NaN included)
            wg = w * g
            p = i // 2
            d = []
            for xa, ab in table:
                tt = r - xa
                d.append((tt * tt, ab[p]))
            d0 = Q._min(v for v, bit in d if bit == 0)
            d1 = Q._min(v for v, bit in d if bit == 1)
            out[b, t] = (d1 - d0) * wg
    with np.errstate(over="ignore"):
        return out.astype(dtype)


# ---- the coefficients ----
def fade_ints(seed, frame_offset, batch, nblocks):
    """(ia, ic) uint64 [batch, nblocks] of the blocks' Box-Muller pairs"""
    return R.uniform_ints(np.arange(nblocks)[None, :], R._frames(frame_offset, batch), SALT_FADE, R.noise_key(seed))


def fade_normals_mp(seed, frame_offset, batch, nblocks):
    """g [batch, 2 Q] object array of mpf: g0 -> Re, g1 -> Im of each block (before the factor C)"""
    g0, g1 = R.normals_mp(*fade_ints(seed, frame_offset, batch, nblocks))
    return R.interleave(g0, g1, 2 * nblocks)


def fade_normals_np(seed, frame_offset, batch, nblocks):
    g0, g1 = R.normals_np(*fade_ints(seed, frame_offset, batch, nblocks))
    return R.interleave(g0, g1, 2 * nblocks)


def expand(h, S, Lc):
    """h [B, >= 2 Q] -> [B, 2 S]: every symbol its block's coefficient"""
    q = np.arange(S) // Lc
    out = np.empty((h.shape[0], 2 * S), dtype=h.dtype)
    out[:, 0::2], out[:, 1::2] = h[:, 2 * q], h[:, 2 * q + 1]
    return out


def rayleigh_mp(x, g, z, sigma, Lc):
    """(h [B, 2 Q], y [B, 2 S]) object arrays of mpf: h = g C, y = h x + sigma z in exact arithmetic; x float64
    (exact), g and z the mpmath normals, sigma and C doubles"""
    S = x.shape[1] // 2
    h = g * R.MP.mpf(C)
    he, xm = expand(h, S, Lc), R.to_mp(x)
    y = np.empty(x.shape, dtype=object)
    y[:, 0::2] = he[:, 0::2] * xm[:, 0::2] - he[:, 1::2] * xm[:, 1::2]
    y[:, 1::2] = he[:, 0::2] * xm[:, 1::2] + he[:, 1::2] * xm[:, 0::2]
    return h, y + z * R.MP.mpf(sigma)


def rayleigh_bound_mp(x, g, z, sigma, Lc):
    """(bound on |h_dev - h|, bound on |y_dev - y|) in the units of qam_ref.qam_awgn_bound_mp.

    |h_dev - h| <= 2^-52 8 |h| per component:
      a normal carries 13/2 eps relative (channel_ref.awgn_bound_mp: log 3, sqrt 2, cospi / sinpi 4, their
      product 1/2); the product with the double C rounds once (1/2): 7, and one eps for the second-order terms,
      the 8 that qam_awgn_bound_mp states for sigma z.
    |y_dev - y| <= 2^-52 (11 (|hr xI| + |hi xQ|) + 9 sigma |z|) for the I axis, Q likewise:
      hr * xI        8 eps from hr (x is exact), one for the product:           9 |hr xI|
      hi * xQ        likewise:                                                  9 |hi xQ|
      their sum      the two errors add, one eps of the operands' magnitude:    10 (|hr xI| + |hi xQ|)
      sigma * z      8 sigma |z| (qam_awgn_bound_mp)
      the last sum   one eps of the operands' magnitude:                        + |hr xI| + |hi xQ| + sigma |z|
    Each rounding is half an eps of its result, which the operands' magnitudes bound; it is stated as one."""
    S = x.shape[1] // 2
    ah = abs(g * R.MP.mpf(C))
    he, ax = expand(ah, S, Lc), abs(R.to_mp(x))
    prod = np.empty(x.shape, dtype=object)
    prod[:, 0::2] = he[:, 0::2] * ax[:, 0::2] + he[:, 1::2] * ax[:, 1::2]
    prod[:, 1::2] = he[:, 0::2] * ax[:, 1::2] + he[:, 1::2] * ax[:, 0::2]
    az = abs(z) * R.MP.mpf(sigma)
    eps = R.MP.mpf(R.EPS)
    return ah * (8 * eps), (prod * 11 + az * 9) * eps


# ---- exact hard-decision error probability of each axis bit under fast Rayleigh fading ----
def qbar(v, sigma):
    """P(N(0, sigma^2 / g) > v) averaged over g = |h|^2 ~ Exp(1): 0.5 (1 - c / sqrt(c c + 2)), c = v / sigma.

    E_g[Q(c sqrt(g))] = 0.5 (1 - sqrt(c^2 / (2 + c^2))) for c >= 0 (the classical Rayleigh average of the
    Gaussian tail) and one minus it for -c.  For c >= 0 it is written 1 / (s (s + c)), s = sqrt(c c + 2), which is
    the same number without the cancellation: 1 - c / s = (s - c) / s = 2 / (s (s + c))."""
    if v == math.inf:
        return 0.0
    if v == -math.inf:
        return 1.0
    c = abs(v) / sigma
    s = math.sqrt(c * c + 2.0)
    t = 1.0 / (s * (s + c))
    return t if v >= 0 else 1.0 - t


def rayleigh_pam_bit_error_prob(h, sigma):
    """[P(bit p decided wrong)] for p = 0 .. h-1 on one axis of the 2^h-level Gray PAM behind fast Rayleigh fading
    with channel state: qam_ref.pam_bit_error_prob with the Gaussian tail replaced by its average qbar.

    Equalisation (r = u / g) leaves the decision thresholds at the midpoints between neighbouring levels and
    scales the axis noise to sigma / |h|; the weight w g is positive, so the LLR's sign is still the bit of the
    nearest level.  Given |h|^2 = g the figure is pam_bit_error_prob(h, sigma / sqrt(g)), and it is linear in
    the tails, so the average over g goes through to each tail."""
    sc = Q.scale_of(2 * h)
    tab = sorted((float(a) * sc, b) for a, b in Q.axis_table(h))  # ascending amplitude
    L = len(tab)
    edges = [-math.inf] + [(tab[i][0] + tab[i + 1][0]) / 2 for i in range(L - 1)] + [math.inf]
    out = []
    for p in range(h):
        tot = 0.0
        for xa, ba in tab:
            for j, (_, bj) in enumerate(tab):
                if bj[p] != ba[p]:
                    tot += qbar(edges[j] - xa, sigma) - qbar(edges[j + 1] - xa, sigma)
        out.append(tot / L)
    return out


def snr_for_error_rate(h, lo=1e-2, hi=1e-1):
    """The first Es/N0 on the 0.5 dB grid, coming down from 60 dB, at which rayleigh_pam_bit_error_prob averages
    inside (lo, hi); the average of that point is at least 2 lo."""
    snr = 60.0
    while snr > -20.0:
        avg = sum(rayleigh_pam_bit_error_prob(h, R.sigma_of(snr))) / h
        if 2 * lo <= avg < hi:
            return snr
        snr -= 0.5
    raise AssertionError("no Es/N0 with an average error rate in range")

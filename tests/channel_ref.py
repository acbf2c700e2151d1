"""Host restatement of the device frame source's stream contract.

NumPy and mpmath only: no HIP, no ctypes, nothing of the package's native side.
Everything here is written from the contract, so that a device kernel and this
file agree only if both follow it:

  Philox4x32-10 (Salmon et al., SC'11): multipliers 0xD2511F53 / 0xCD9E8D57, key
  bumps 0x9E3779B9 / 0xBB67AE85, 10 rounds.

  f = frame_offset + b, the global frame index, unsigned 64 bit.

  source        counter                      key                          use
  message bits  (w, f_lo, f_hi, 0xB175B175)  (seed_lo, seed_hi)           bit j = bit j % 32 of word x at w = j // 32
  AWGN          (q, f_lo, f_hi, 0xA3A3A3A3)  (seed_lo ^ 0x5bd1e995, hi)   pair q -> normals of bits 2q, 2q + 1
  Rayleigh      (j, f_lo, f_hi, salt)        as AWGN                      salt 0xFADE0001 -> (h_r, h_i), 0xFADE0002 -> (z, -)
  BSC           (j, f_lo, f_hi, 0xB5CB5C00)  as AWGN                      flip iff u < p

  a = y << 32 | x, c = w << 32 | z; u1 = ((a >> 11) + 1) 2^-53 in (0, 1],
  u2 = (c >> 11) 2^-53 in [0, 1); z0 = sqrt(-2 ln u1) cos(2 pi u2),
  z1 = sqrt(-2 ln u1) sin(2 pi u2); the BSC's u is the u2 form applied to a.

  sigma = sqrt(1 / (2 10^(snr/10))) in double.
  AWGN      llr = 2 (s + sigma z) / sigma^2, s = 1 - 2 (byte & 1), s = 1 without a codeword.
  Rayleigh  h = sqrt((h_r^2 + h_i^2) / 2), llr = 2 (h s + sigma z) h / sigma^2.

The uniforms are kept as their 53-bit integers (ia = a >> 11, ic = c >> 11), which
are exact; normals and LLRs come from them in mpmath at PREC bits (object arrays
of mpf), or in NumPy floating point for the statistical checks.
"""
import math

import mpmath
import numpy as np

M32 = 0xFFFFFFFF
M64 = 0xFFFFFFFFFFFFFFFF
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
SALT_BITS, SALT_AWGN, SALT_BSC = 0xB175B175, 0xA3A3A3A3, 0xB5CB5C00
SALT_FADE_H, SALT_FADE_Z = 0xFADE0001, 0xFADE0002
NOISE_KEY_XOR = 0x5bd1e995

PREC = 128
MP = mpmath.mp.clone()
MP.prec = PREC
EPS = 2.0 ** -52


# ---- Philox4x32-10 ------------------------------------------------------------

def philox4x32_10(counter, key):
    """Scalar Philox4x32-10 on Python integers: (c0, c1, c2, c3), (k0, k1) -> 4 words."""
    c0, c1, c2, c3 = (int(v) & M32 for v in counter)
    k0, k1 = (int(v) & M32 for v in key)
    for _ in range(10):
        p0, p1 = PHILOX_M0 * c0, PHILOX_M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + PHILOX_W0) & M32, (k1 + PHILOX_W1) & M32
    return c0, c1, c2, c3


def philox4x32_10_np(counter, key):
    """Vectorised Philox4x32-10: counter and key are sequences of 4 and 2 uint64
    arrays (or scalars) holding 32-bit values, broadcast against each other; the
    32 x 32 -> 64 bit products are single uint64 multiplications."""
    u = np.uint64
    c0, c1, c2, c3 = np.broadcast_arrays(*[np.asarray(v, dtype=u) & u(M32) for v in counter])
    k0, k1 = (np.asarray(v, dtype=u) & u(M32) for v in key)
    for _ in range(10):
        p0, p1 = u(PHILOX_M0) * c0, u(PHILOX_M1) * c2
        c0, c1, c2, c3 = (p1 >> u(32)) ^ c1 ^ k0, p1 & u(M32), (p0 >> u(32)) ^ c3 ^ k1, p0 & u(M32)
        k0, k1 = (k0 + u(PHILOX_W0)) & u(M32), (k1 + u(PHILOX_W1)) & u(M32)
    return c0, c1, c2, c3


# ---- stream layout ------------------------------------------------------------

def _frames(frame_offset, batch):
    """Global frame indices [batch, 1] as uint64 (Python integers: no wrap at 2^32 or 2^63)."""
    return np.array([(int(frame_offset) + b) & M64 for b in range(int(batch))], dtype=np.uint64)[:, None]


def _ctr(index, frames, salt):
    f = np.asarray(frames, dtype=np.uint64)
    return (np.asarray(index, dtype=np.uint64), f & np.uint64(M32), f >> np.uint64(32), np.uint64(salt))


def message_key(seed):
    seed = int(seed) & M64
    return seed & M32, seed >> 32


def noise_key(seed):
    seed = int(seed) & M64
    return (seed & M32) ^ NOISE_KEY_XOR, seed >> 32


def uniform_ints(index, frames, salt, key):
    """The two 53-bit integers of one Philox call per (frame, index): ia = a >> 11
    (u1 = (ia + 1) 2^-53, or u = ia 2^-53 for the BSC) and ic = c >> 11 (u2 = ic 2^-53)."""
    x, y, z, w = philox4x32_10_np(_ctr(index, frames, salt), key)
    s = np.uint64
    return ((y << s(32)) | x) >> s(11), ((w << s(32)) | z) >> s(11)


def message_bits(seed, frame_offset, batch, k):
    """uint8 [batch, k] message bits."""
    nw = (k + 31) // 32
    x = philox4x32_10_np(_ctr(np.arange(nw)[None, :], _frames(frame_offset, batch), SALT_BITS), message_key(seed))[0]
    bits = (x[:, :, None] >> np.arange(32, dtype=np.uint64)[None, None, :]) & np.uint64(1)
    return bits.reshape(batch, nw * 32)[:, :k].astype(np.uint8)


def awgn_ints(seed, frame_offset, batch, n):
    """(ia, ic) uint64 [batch, ceil(n / 2)] of the AWGN pairs."""
    return uniform_ints(np.arange((n + 1) // 2)[None, :], _frames(frame_offset, batch), SALT_AWGN, noise_key(seed))


def rayleigh_ints(seed, frame_offset, batch, n):
    """((ia, ic) of the fading pair, (ia, ic) of the noise pair), each uint64 [batch, n]."""
    f, j, key = _frames(frame_offset, batch), np.arange(n)[None, :], noise_key(seed)
    return uniform_ints(j, f, SALT_FADE_H, key), uniform_ints(j, f, SALT_FADE_Z, key)


def bsc_flips(seed, frame_offset, batch, n, p):
    """uint8 [batch, n]: 1 where the BSC flips (u < p; both sides exact doubles)."""
    ia, _ = uniform_ints(np.arange(n)[None, :], _frames(frame_offset, batch), SALT_BSC, noise_key(seed))
    return (ia.astype(np.float64) * 2.0 ** -53 < float(p)).astype(np.uint8)


def sigma_of(snr_db):
    return math.sqrt(1.0 / (2.0 * 10.0 ** (snr_db / 10.0)))


# ---- Box-Muller ---------------------------------------------------------------

WIDE = np.longdouble if np.finfo(np.longdouble).nmant >= 63 else np.float64


def normals_np(ia, ic, dtype=np.float64):
    """(z0, z1) in NumPy floating point.  2 u2 is reduced exactly on the integer:
    the octant comes from ic's top three bits and the remaining angle, in
    [0, pi / 4], from the low 50 (or their complement), so no product with pi
    is ever rounded near a zero of cos or sin."""
    ia, ic = np.asarray(ia, dtype=np.uint64), np.asarray(ic, dtype=np.uint64)
    rad = np.sqrt(dtype(-2.0) * np.log((ia.astype(dtype) + dtype(1.0)) * dtype(2.0 ** -53)))
    octant = (ic >> np.uint64(50)).astype(np.int64)            # 2 pi u2 = (octant + frac) pi / 4
    low = ic & np.uint64((1 << 50) - 1)
    odd = (octant & 1) == 1
    frac = np.where(odd, np.uint64(1 << 50) - low, low).astype(dtype) * dtype(2.0 ** -50)   # in [0, 1], exact
    phi = frac * _pi(dtype) / dtype(4.0)
    # the angle is k pi/4 + t with k even: k = octant, t = phi in an even octant,
    # k = octant + 1, t = -phi (frac = the complement) in an odd one
    k = np.where(odd, octant + 1, octant) % 8
    st, ct = np.where(odd, -1.0, 1.0).astype(dtype) * np.sin(phi), np.cos(phi)
    cos_t = np.select([k == 0, k == 2, k == 4, k == 6], [ct, -st, -ct, st])
    sin_t = np.select([k == 0, k == 2, k == 4, k == 6], [st, ct, -st, -ct])
    return rad * cos_t, rad * sin_t


def _pi(dtype):
    """pi rounded to dtype (np.pi carries only 53 bits)."""
    if dtype is np.float64:
        return np.float64(np.pi)
    hi = np.longdouble(np.pi)
    return hi + np.longdouble(float(MP.pi - MP.mpf(np.pi)))


def _obj(values, shape):
    out = np.empty(len(values), dtype=object)
    out[:] = values
    return out.reshape(shape)


def normals_mp(ia, ic):
    """(z0, z1) as object arrays of mpf at PREC bits.  t = 2 u2 in [0, 2) is an
    exact dyadic: its quadrant and the remainder r in [0, 1/2) are taken exactly
    before pi r meets cos and sin."""
    ia, ic = np.asarray(ia, dtype=np.uint64), np.asarray(ic, dtype=np.uint64)
    z0, z1 = [], []
    two53, half = MP.mpf(2) ** 53, MP.mpf(1) / 2
    for va, vc in zip(ia.ravel().tolist(), ic.ravel().tolist()):
        rad = MP.sqrt(-2 * MP.log(MP.mpf(va + 1) / two53))
        quad, rem = divmod(vc, 1 << 51)                        # 2 u2 = quad / 2 + rem 2^-52
        r = MP.mpf(rem) / (MP.mpf(2) ** 52)
        assert 0 <= r < half
        c, s = MP.cos(MP.pi * r), MP.sin(MP.pi * r)
        c, s = ((c, s), (-s, c), (-c, -s), (s, -c))[quad]
        z0.append(rad * c)
        z1.append(rad * s)
    return _obj(z0, ia.shape), _obj(z1, ia.shape)


def interleave(z0, z1, n):
    """[B, P] pairs -> [B, n] (bit 2q from z0, 2q + 1 from z1)."""
    out = np.empty((z0.shape[0], 2 * z0.shape[1]), dtype=z0.dtype)
    out[:, 0::2], out[:, 1::2] = z0, z1
    return out[:, :n]


def to_mp(a):
    """float64 array -> object array of the same values as mpf (exact)."""
    a = np.asarray(a, dtype=np.float64)
    return _obj([MP.mpf(v) for v in a.ravel().tolist()], a.shape)


def signs(codeword, shape):
    """BPSK symbols 1 - 2 (byte & 1) as Python-int object array; all +1 without a codeword."""
    if codeword is None:
        return np.ones(shape, dtype=np.int64).astype(object)
    return (1 - 2 * (np.asarray(codeword).astype(np.int64) & 1)).astype(object)


def awgn_llr_mp(z, s, sigma):
    """llr = 2 (s + sigma z) / sigma^2 on object arrays; sigma a double, squared exactly."""
    sg = MP.mpf(sigma)
    return (z * sg + s) * (2 / (sg * sg))


def awgn_bound_mp(z, sigma, libm_ulps=0):
    """|llr_device - llr_exact| <= 2^-52 (2 / sigma^2) (8 sigma |z| + 2 (1 + sigma |z|)).

    First-order propagation, in units of eps = 2^-52 relative (an error of k ulp
    is at most k eps relative; a correctly rounded operation is half of one,
    with or without FMA contraction, which only drops roundings).  The uniforms
    and 2 u2 are exact.  With the OpenCL / ocml double-precision bounds:
      log(u1)               3       (-2 x is exact)
      sqrt                  3/2 + 1/2 = 2   (a square root halves, then rounds)
      cospi / sinpi         4
      rad * cs              2 + 4 + 1/2 = 13/2
      sigma * z             7
    so sigma z carries at most 7 eps sigma |z|: 8 with one eps for the second-order
    terms.  y = s + sigma z rounds once (1/2 of |y| <= 1 + sigma |z|), 2 y is
    exact, the division rounds once (1/2) and divides by the rounded product
    sigma * sigma (1/2): 3/2, stated as 2, of 1 + sigma |z|.
    libm_ulps widens the sigma |z| term for a reference that is itself computed
    in double."""
    sg = MP.mpf(sigma)
    az = abs(z) * sg
    return (az * (8 + libm_ulps) + (az + 1) * 2) * (MP.mpf(EPS) * 2 / (sg * sg))


RAYLEIGH_C = 18


def rayleigh_h_mp(hr, hi):
    h2 = (hr * hr + hi * hi) / 2
    return _obj([MP.sqrt(v) for v in h2.ravel().tolist()], h2.shape)


def rayleigh_llr_mp(h, z, s, sigma):
    """llr = 2 (h s + sigma z) h / sigma^2 on object arrays."""
    sg = MP.mpf(sigma)
    return (h * s + z * sg) * h * (2 / (sg * sg))


def rayleigh_bound_mp(h, z, sigma):
    """|llr_device - llr_exact| <= 2^-52 (2 / sigma^2) 18 h (h + sigma |z|).

    Same units and function bounds as awgn_bound_mp.  Each normal (h_r, h_i, z)
    carries 13/2 eps relative.  Then
      h_r^2, h_i^2          2 * 13/2 + 1/2 = 27/2
      their sum             27/2 + 1/2 = 14  (both positive; halving is exact)
      h = sqrt              7 + 1/2 = 15/2
      sigma * z             7 (of sigma |z|);  h * s is exact
      y = h s + sigma z     15/2 h + 7 sigma |z| + 1/2 |y|  <=  8 h + 15/2 sigma |z|
      (2 y) * h             h (8 h + 15/2 sigma |z|) + (15/2 + 1/2) |y| h  <=  h (16 h + 31/2 sigma |z|)
      / (sigma * sigma)     + (1/2 + 1/2) |y| h                            <=  h (17 h + 33/2 sigma |z|)
    with |y| <= h + sigma |z| throughout: 17 h (h + sigma |z|), and one more eps
    for the second-order terms as in the AWGN bound."""
    sg = MP.mpf(sigma)
    return h * (h + abs(z) * sg) * (MP.mpf(EPS) * 2 * RAYLEIGH_C / (sg * sg))


def max_ratio(dev, ref, bound):
    """Largest |dev - ref| / bound over float64 dev and object arrays ref, bound."""
    err = abs(to_mp(dev) - ref) / bound
    return float(max(err.ravel().tolist()))


# ---- encoders and CRC -----------------------------------------------------------

def kronecker_power(n):
    """F^{(x) n} for F = [[1, 0], [1, 1]], int64 [2^n, 2^n]."""
    F = np.array([[1, 0], [1, 1]], dtype=np.int64)
    G = np.ones((1, 1), dtype=np.int64)
    for _ in range(n):
        G = np.kron(G, F)
    return G


def polar_u(msg, frozen_mask):
    """u [B, N]: bit 0 of the message bytes at the unfrozen positions in rising order, 0 elsewhere."""
    msg = np.asarray(msg).astype(np.int64) & 1
    u = np.zeros((msg.shape[0], len(frozen_mask)), dtype=np.int64)
    u[:, np.flatnonzero(np.asarray(frozen_mask) == 0)] = msg
    return u


def polar_encode_kron(u):
    """x = u F^{(x) n} over GF(2), natural index, from the Kronecker definition."""
    u = np.asarray(u, dtype=np.int64)
    n = int(round(math.log2(u.shape[-1])))
    return (u @ kronecker_power(n)) % 2


def polar_encode_butterfly(u):
    """The same product for long codes, as n stages over NumPy arrays: stage d
    adds (mod 2) the entry whose index has bit d set to the one that has it
    clear (test_channel_ref_host.py holds it to the Kronecker product)."""
    x = np.array(u, dtype=np.int64) & 1
    N = x.shape[-1]
    idx = np.arange(N)
    d = 1
    while d < N:
        lo = idx[(idx & d) == 0]
        x[..., lo] ^= x[..., lo | d]
        d <<= 1
    return x


def crc_bits(data, crc_len, poly):
    """The crc_len CRC bits (MSB first) of a bit sequence: bit-serial, MSB-first,
    zero initial register, polynomial without its leading term."""
    reg, top, mask = 0, 1 << (crc_len - 1), (1 << crc_len) - 1
    for bit in data:
        reg ^= (int(bit) & 1) << (crc_len - 1)
        reg = ((reg << 1) ^ poly) if reg & top else (reg << 1)
        reg &= mask
    return [(reg >> (crc_len - 1 - t)) & 1 for t in range(crc_len)]


def gf2_encode(msg, G):
    return (((np.asarray(msg).astype(np.int64) & 1) @ (np.asarray(G).astype(np.int64) & 1)) % 2).astype(np.uint8)

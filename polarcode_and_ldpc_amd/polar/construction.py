"""Polar code construction (host side, one-off).

The reference's construction API (src/polar/construction.py): the
Bhattacharyya bounds (:11-48), its "gaussian approximation" recursion
(:51-97), construct_polar_code with its three methods, returning both index
sets sorted (:100-140), and calculate_channel_capacities (:143-174).  Every
function gives the reference's values (tests/test_host_api.py, fixtures made
by tests/golden/make_golden.py:job_host_api).

Those indices are in Arikan order; the SC/SCL decoders of the reference (and of
this package) number bits in natural order, so `construct_frozen_set(...,
bit_reversed=True)` applies the bit reversal that makes the set usable with
them."""
from __future__ import annotations

import math
from typing import Tuple

import numpy as np

from .utils import bit_reverse_indices


def _polarize(x0: float, n: int, bad, good) -> np.ndarray:
    """n levels of the channel-splitting recursion: child 2i = bad(x[i]),
    child 2i+1 = good(x[i]), element-wise (the reference's per-index loops)."""
    x = np.array([x0], dtype=np.float64)
    for _ in range(n):
        nx = np.empty(2 * len(x))
        nx[0::2] = bad(x)
        nx[1::2] = good(x)
        x = nx
    return x


def _sq(z: np.ndarray) -> np.ndarray:
    """z ** 2 as the reference's scalar `Z[i] ** 2` rounds it: libm pow(z, 2),
    which is 1 ulp off z * z for ~0.1 % of inputs (np.square is z * z)."""
    return np.array([math.pow(float(v), 2.0) for v in z])


def bhattacharyya_bounds(N: int, snr_db: float) -> np.ndarray:
    """Z of each bit channel, Z0 = exp(-SNR); degraded 2Z - Z^2, upgraded Z^2
    (construction.py:11-48).  Smaller is more reliable."""
    return _polarize(np.exp(-(10 ** (snr_db / 10.0))), int(np.log2(N)), lambda z: 2 * z - _sq(z), _sq)


def gaussian_approximation(N: int, snr_db: float) -> np.ndarray:
    """The reference's simplified "GA" mean recursion (construction.py:51-97):
    mu0 = 2 SNR; degraded child 0.9 mu below 10 (else mu), upgraded child 2 mu
    saturated at 100.  Larger is more reliable."""
    return _polarize(2.0 * 10 ** (snr_db / 10.0), int(np.log2(N)),
                     lambda m: np.where(m < 10, m * 0.9, m), lambda m: np.minimum(2 * m, 100.0))


def construct_polar_code(N: int, K: int, method: str = "bhattacharyya", snr_db: float = 0.0
                         ) -> Tuple[np.ndarray, np.ndarray]:
    """(frozen, info), both ascending (construction.py:100-140).

    "bhattacharyya": the K smallest Z; "gaussian_approximation": the first K of
    argsort(mu) reversed; any other method: the bit-reversal heuristic of
    generate_frozen_bits (the K largest bit-reversed indices).  Ties are broken
    by np.argsort exactly as the reference does (same call, same input)."""
    if method == "bhattacharyya":
        order = np.argsort(bhattacharyya_bounds(N, snr_db))
    elif method == "gaussian_approximation":
        order = np.argsort(gaussian_approximation(N, snr_db))[::-1]
    else:  # the K largest bit-reversed indices, sliced as the reference ([-K:], [:-K])
        order = np.argsort(bit_reverse_indices(int(np.log2(N))))
        return np.sort(order[:-K]), np.sort(order[-K:])
    return np.sort(order[K:]), np.sort(order[:K])


def calculate_channel_capacities(N: int, snr_db: float) -> np.ndarray:
    """1 - H2((1 - Z) / 2) per bit channel from the Bhattacharyya Z, 1 below
    Z = 1e-10 and 0 above 1 - 1e-10 (construction.py:143-174)."""
    Z = bhattacharyya_bounds(N, snr_db)
    cap = np.zeros(N)
    for i, z in enumerate(Z):  # scalar ufunc calls: the reference's rounding
        if z < 1e-10:
            cap[i] = 1.0
        elif z <= 1 - 1e-10:
            p = (1 - z) / 2
            if 0 < p < 1:
                cap[i] = 1 - (-p * np.log2(p) - (1 - p) * np.log2(1 - p))
    return cap


def construct_frozen_set(N: int, K: int, snr_db: float = 2.0, bit_reversed: bool = True) -> np.ndarray:
    """Sorted frozen index set for the SC/SCL decoders (bit-reversed
    Bhattacharyya construction at design SNR snr_db)."""
    frozen, _ = construct_polar_code(N, K, "bhattacharyya", snr_db)
    if bit_reversed:
        frozen = bit_reverse_indices(int(np.log2(N)))[frozen]
    return np.sort(np.asarray(frozen, dtype=np.int64))


def bit_channel_bhattacharyya(z_leaf) -> np.ndarray:
    """Bhattacharyya parameter of each u_l given one per codeword position (the leaves may differ), in the
    decoders' order: the first f/g level pairs the adjacent inputs (x[2k], x[2k+1]) and the even-indexed
    u are decoded from the f outputs (oracle/refnumpy.py:_llr_pass, stage 0 has half = 1).  So on
    a = z[0::2], b = z[1::2]: out[0::2] = rec(a + b - a b), out[1::2] = rec(a b).  With equal leaves this
    is bhattacharyya_bounds(N, snr)[bit_reverse_indices(n)] up to rounding."""
    z = np.asarray(z_leaf, dtype=np.float64)
    assert z.ndim == 1 and len(z) >= 1 and len(z) & (len(z) - 1) == 0, "one value per position, a power of 2 of them"
    if len(z) == 1:
        return z.copy()
    a, b = z[0::2], z[1::2]
    out = np.empty(len(z))
    out[0::2] = bit_channel_bhattacharyya(a + b - a * b)
    out[1::2] = bit_channel_bhattacharyya(a * b)
    return out


def construct_rate_matched(K: int, matcher, snr_db: float = 2.0) -> np.ndarray:
    """Sorted frozen index set of a K-bit code on the rate-matched mother code of `matcher` (a
    polar.PolarRateMatcher), for the SC/SCL decoders.

    Leaf Z per codeword position, with Z0 = exp(-10^(snr_db / 10)) per transmitted symbol: a position
    sent c times math.pow(Z0, c); punctured 1.0 (nothing is known); shortened 0.0 (known).  The bit
    channels' Z come from bit_channel_bhattacharyya.  The information set is the first K of
    np.argsort(Z, kind="stable") restricted to the indices outside matcher.forced_frozen(): ties go to
    the lower index.

    Example, exact in floating point: N = 8, E = 6, puncture, sub_blocks None, snr_db = 30, so that
    Z0 = exp(-1000) = 0.0.  Positions 0 and 1 are punctured: the leaves are (1, 1, 0, 0, 0, 0, 0, 0).
    The first level pairs (1, 1), (0, 0), (0, 0), (0, 0): the f side is (1 + 1 - 1, 0, 0, 0) = (1, 0, 0, 0)
    and feeds the even u, the g side is (1 * 1, 0, 0, 0) = (1, 0, 0, 0) and feeds the odd u.  On either,
    the next level pairs (1, 0) and (0, 0): f side (1, 0), g side (0, 0); and the last level turns (1, 0)
    into (1, 0) and (0, 0) into (0, 0).  Interleaving back, Z = (1, 1, 0, 0, 0, 0, 0, 0) by index: u_0 and
    u_1 carry nothing, and six indices tie at 0.0.  The stable order is 2, 3, 4, 5, 6, 7, 0, 1, so K = 3
    gives the information set {2, 3, 4} and the frozen set {0, 1, 5, 6, 7}: ties go to the lower index.
    K = 7 would take index 0 with Z = 1.0 and raises.

    ValueError when fewer than K indices lie outside the forced set, or when a chosen index has
    Z >= 1.0: too many information bits for what is sent at this design SNR, or rounding has hidden a
    zero-capacity channel."""
    N = matcher.N
    z0 = math.exp(-(10 ** (snr_db / 10.0)))
    count = np.bincount(matcher.positions_host(), minlength=N)
    leaf = np.array([math.pow(z0, int(c)) if c else (0.0 if matcher.mode == "shorten" else 1.0) for c in count])
    Z = bit_channel_bhattacharyya(leaf)
    forced = np.zeros(N, dtype=bool)
    forced[matcher.forced_frozen()] = True
    order = [int(i) for i in np.argsort(Z, kind="stable") if not forced[i]]
    if K < 1 or len(order) < K:
        raise ValueError("K = %d outside 1 .. %d, the indices that shortening leaves free" % (K, len(order)))
    info = order[:K]
    worst = max(Z[i] for i in info)
    if worst >= 1.0:
        raise ValueError("K = %d puts information on a bit channel with Z >= 1: too many information bits for "
                         "E = %d at the design SNR %g dB" % (K, matcher.E, snr_db))
    frozen = np.ones(N, dtype=bool)
    frozen[info] = False
    return np.flatnonzero(frozen).astype(np.int64)

"""Block Rayleigh fading for the QAM symbols, everything that needs no GPU: channel.QAMModem's host methods
against the definition written as loops (tests/qam_fading_ref.py), the erased symbol, the h = 1 case against the
AWGN demapper, pl_qam_fading_check through the library, the closed-form error rate against a quadrature, and the
salt.

The definition: include/polarldpc.h at pl_qam_fading_check.  fading_inputs() is the input set the GPU tests share
(tests/test_gpu_qam_fading.py)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import channel_ref as R
import qam_fading_ref as F
import qam_ref as Q
from test_qam_host import bits_view, host_inputs, modem, same_bits
from polarcode_and_ldpc_amd import _native
from polarcode_and_ldpc_amd.channel.qam import sigma_of

MS = Q.MS
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# coefficients on the demapper's edges: zero, a signed zero, g underflowing to 0, g overflowing, NaN, inf, unity
H_SPECIALS = [(0.0, 0.0), (-0.0, 0.0), (1e-200, 0.0), (1e200, 0.0), (math.nan, 0.0), (math.inf, 0.0), (1.0, 0.0)]


def coherences(S):
    """Lc of the grid: fast, short blocks, one symbol short of the frame, the frame, beyond it, the largest"""
    return sorted({1, 2, 3, S, S + 5, 2 ** 30} | ({S - 1} if S - 1 >= 1 else set()))


def fading_inputs(m, E, B, Lc, seed=0):
    """(y float64 [B, 2 S] from host_inputs, its specials included; h float64 [B, 2 Q] random with H_SPECIALS
    written over its first entries, row by row)"""
    _, y = host_inputs(m, E, B, seed)
    S = -(-E // m)
    nq = F.blocks(S, Lc)
    rng = np.random.default_rng(77 * m + 13 * E + B + 1000 * min(Lc, 999) + seed)
    h = rng.standard_normal((B, 2 * nq)) * F.C
    flat = h.reshape(-1)
    sp = np.array(H_SPECIALS, dtype=np.float64).reshape(-1)
    n = min(len(sp), flat.size) & ~1  # whole coefficients
    flat[:n] = sp[:n]
    return y, h


# ---- the host methods against the loops ----
@pytest.mark.parametrize("m", MS)
def test_demap_csi_host_equals_the_loops(m):
    snr = 7.5
    for E in sorted({1, m, m + 1, 2 * m - 1, 2 * m, 2 * m + 1, 3 * m - 1, 64, 65}):
        S = -(-E // m)
        for B in (1, 5):
            for Lc in coherences(S):
                y, h = fading_inputs(m, E, B, Lc)
                for dt in (np.float64, np.float32):
                    got = modem(m).demap_csi_host(y, h, E, snr, coherence=Lc, dtype=dt)
                    want = F.demap_csi(y, h, E, m, sigma_of(snr), Lc, dtype=dt)
                    assert same_bits(got, want), (E, B, Lc, dt)
                assert same_bits(modem(m).demap_csi_host(y[0], h[0], E, snr, coherence=Lc), want64(y, h, E, m, snr, Lc)[0])


def want64(y, h, E, m, snr, Lc):
    return F.demap_csi(y[:1], h[:1], E, m, sigma_of(snr), Lc)


@pytest.mark.parametrize("m", MS)
def test_zero_gain_erases_the_symbol(m):
    """g == 0.0 (a zero, a signed zero, an underflowing square): +0.0, sign bit clear, for all m LLRs of the
    symbol, whatever y holds there (NaN and inf included)"""
    E = 8 * m
    _, y = host_inputs(m, E, 2)
    h = np.full((2, 2 * 8), 0.7)
    zeros = [(0.0, 0.0), (-0.0, 0.0), (-0.0, -0.0), (1e-200, 0.0), (1e-170, -1e-170), (0.0, 5e-324)]
    for s, c in enumerate(zeros):
        h[:, 2 * s:2 * s + 2] = c
    y[1, :4] = [np.nan, np.inf, -np.inf, 1e300]
    for dt in (np.float64, np.float32):
        llr = modem(m).demap_csi_host(y, h, E, 3.0, coherence=1, dtype=dt)
        erased = llr[:, :len(zeros) * m]
        assert np.all(bits_view(erased) == 0), dt
        rest = llr[0, len(zeros) * m:]
        assert np.all(rest != 0)  # the other symbols are demapped


@pytest.mark.parametrize("m", MS)
def test_unit_gain_equals_the_awgn_demapper(m):
    """h = (1.0, 0.0) everywhere with finite y: bit for bit demap_host's result"""
    for E in (1, m + 1, 64, 131):
        _, y = host_inputs(m, E, 3)
        y = np.where(np.isfinite(y), y, 0.25)
        S = -(-E // m)
        for Lc in (1, 3, 2 ** 30):
            h = np.zeros((3, 2 * F.blocks(S, Lc)))
            h[:, 0::2] = 1.0
            for dt in (np.float64, np.float32):
                got = modem(m).demap_csi_host(y, h, E, 7.5, coherence=Lc, dtype=dt)
                assert same_bits(got, modem(m).demap_host(y, E, 7.5, dtype=dt)), (E, Lc, dt)


@pytest.mark.parametrize("m", MS)
def test_fade_host_equals_the_loops(m):
    for E in (1, m + 1, 65):
        S = -(-E // m)
        for B in (1, 5):
            bits, _ = host_inputs(m, E, B)
            x = modem(m).modulate_host(bits)
            for Lc in coherences(S):
                _, h = fading_inputs(m, E, B, Lc)
                noise = 0.1 * np.random.default_rng(E + Lc % 1000).standard_normal((B, 2 * S))
                got = modem(m).fade_host(x, h, noise, Lc)
                assert same_bits(got, F.fade(x, h, noise, Lc)), (E, B, Lc)
                assert same_bits(modem(m).fade_host(x[0], h[0], noise[0], Lc), got[0])
    assert modem(m).blocks(65, 3) == F.blocks(-(-65 // m), 3)


def test_round_trip_without_noise():
    """fade then demap_csi returns the sent bits for any non-zero coefficient: the conjugate in u and the sign of
    the weight"""
    for m in MS:
        E = 40 * m
        bits = np.random.default_rng(m).integers(0, 2, (3, E), dtype=np.uint8)
        x = modem(m).modulate_host(bits)
        for Lc in (1, 7, 2 ** 30):
            h = np.random.default_rng(Lc % 1000).standard_normal((3, 2 * F.blocks(40, Lc))) * F.C
            y = modem(m).fade_host(x, h, np.zeros_like(x), Lc)
            llr = modem(m).demap_csi_host(y, h, E, 10.0, coherence=Lc)
            assert np.array_equal((llr <= 0).astype(np.uint8), bits), (m, Lc)


# ---- pl_qam_fading_check ----
def _refusal(m, E, Lc):
    S, nq = ctypes.c_int64(-7), ctypes.c_int64(-7)
    rc = _native.lib.pl_qam_fading_check(m, E, Lc, ctypes.byref(S), ctypes.byref(nq))
    assert rc == _native.PL_EINVAL and S.value == -7 and nq.value == -7
    with pytest.raises(AssertionError) as e:
        _native.qam_fading_check(m, E, Lc)
    return str(e.value)


def test_fading_check_refusals_in_order():
    for m in (0, 3, 10, -2):
        assert "m = %d must be 2, 4, 6 or 8" % m in _refusal(m, 8, 1)
    assert "m = 3" in _refusal(3, 0, 0)  # m comes first
    for E in (0, -1, 2 ** 30 + 1):
        assert "E = %d outside 1 .. 2^30" % E in _refusal(4, E, 1)
    assert "E = 0" in _refusal(4, 0, 0)  # E comes before the coherence length
    for Lc in (0, -1, 2 ** 30 + 1, 2 ** 40):
        assert "coherence = %d outside 1 .. 2^30" % Lc in _refusal(4, 8, Lc)
    with pytest.raises(AssertionError, match="coherence = 0"):
        modem(4).blocks(8, 0)


def test_fading_check_values():
    for m in MS:
        for E in (1, m, m + 1, 1000, 2 ** 30):
            S = -(-E // m)
            for Lc, want in ((1, S), (S, 1), (2 ** 30, 1)) + (((S - 1, 2),) if S > 1 else ()):
                assert _native.qam_fading_check(m, E, Lc) == (S, want), (m, E, Lc)
                assert modem(m).blocks(E, Lc) == want
            assert _native.qam_fading_check(m, E, 3) == (S, -(-S // 3))
    assert _native.lib.pl_qam_fading_check(4, 10, 2, None, None) == 0  # NULL out-pointers
    nq = ctypes.c_int64()
    assert _native.lib.pl_qam_fading_check(4, 10, 2, None, ctypes.byref(nq)) == 0 and nq.value == 2
    assert _native.lib.pl_qam_fading_check(4, 10, 0, None, None) == _native.PL_EINVAL


# ---- the closed-form error rate ----
def _quadrature(h, sigma):
    """E over g ~ Exp(1) of qam_ref.pam_bit_error_prob(h, sigma / sqrt(g)): g = -ln(1 - v), v uniform, by
    Gauss-Legendre on pieces of (0, 1) that shrink towards both ends, where the integrand is steep"""
    cuts = [0.0] + [10.0 ** -k for k in range(12, 0, -1)] + [1 - 10.0 ** -k for k in range(1, 13)] + [1.0]
    nodes, weights = np.polynomial.legendre.leggauss(64)
    tot = np.zeros(h)
    for a, b in zip(cuts[:-1], cuts[1:]):
        for t, wt in zip(nodes, weights):
            v = 0.5 * (b - a) * t + 0.5 * (a + b)
            g = -math.log1p(-v)
            tot += 0.5 * (b - a) * wt * np.array(Q.pam_bit_error_prob(h, sigma / math.sqrt(g)))
    return tot


@pytest.mark.parametrize("h", [1, 2, 3, 4])
def test_rayleigh_error_prob_equals_the_quadrature(h):
    for snr in (F.snr_for_error_rate(h), F.snr_for_error_rate(h) + 12.0):
        sigma = R.sigma_of(snr)
        got = np.array(F.rayleigh_pam_bit_error_prob(h, sigma))
        want = _quadrature(h, sigma)
        assert np.all(np.abs(got - want) <= 1e-6 * want), (h, snr, got, want)
    assert all(0 <= v < 1e-15 for v in F.rayleigh_pam_bit_error_prob(h, R.sigma_of(200.0)))


def test_rayleigh_error_prob_shape():
    # the search's points, on the 0.5 dB grid coming down from 60 dB
    assert [F.snr_for_error_rate(h) for h in (1, 2, 3, 4)] == [13.5, 19.5, 24.5, 29.5]
    for h in (1, 2, 3, 4):
        s = R.sigma_of(F.snr_for_error_rate(h))
        pr = F.rayleigh_pam_bit_error_prob(h, s)
        assert 2e-2 <= sum(pr) / h < 1e-1 and pr == sorted(pr)
        assert all(f > a for f, a in zip(pr, Q.pam_bit_error_prob(h, s)))  # fading costs, at equal Es/N0
    # QPSK: one threshold at 0, the classical 0.5 (1 - sqrt(snr / (1 + snr))) with snr = scale^2 / (2 sigma^2)
    s = 0.2
    snr = Q.scale_of(2) ** 2 / (2 * s * s)
    assert abs(F.rayleigh_pam_bit_error_prob(1, s)[0] - 0.5 * (1 - math.sqrt(snr / (1 + snr)))) < 1e-15
    assert F.qbar(math.inf, s) == 0.0 and F.qbar(-math.inf, s) == 1.0 and abs(F.qbar(0.0, s) - 0.5) < 1e-15
    for v in (0.01, 0.3, 2.0):
        c = v / s
        assert abs(F.qbar(v, s) - 0.5 * (1 - c / math.sqrt(c * c + 2))) < 1e-15
        assert abs(F.qbar(v, s) + F.qbar(-v, s) - 1.0) < 1e-15


# ---- the salt ----
def test_salt_is_the_headers_and_is_new():
    text = open(os.path.join(ROOT, "polarcode_and_ldpc_amd", "csrc", "qam_check.hpp")).read()
    (lit,) = re.findall(r"constexpr\s+uint32_t\s+SALT_FADE\s*=\s*(0x[0-9A-Fa-f]+)u?\s*;", text)
    assert int(lit, 16) == F.SALT_FADE == 0xFADE9A3A
    api = open(os.path.join(ROOT, "include", "polarldpc.h")).read()
    assert "0xFADE9A3A" in api
    others = {Q.SALT_QAM, 0xFADE0001, 0xFADE0002, R.SALT_FADE_H, R.SALT_FADE_Z, R.SALT_BITS, R.SALT_AWGN, R.SALT_BSC}
    assert F.SALT_FADE not in others
    assert F.C == math.sqrt(2.0) / 2.0 == math.sqrt(0.5)  # halving is exact: the double nearest 1 / sqrt(2)

"""Gray-mapped QAM, everything that needs no GPU: the constellation's properties, channel.QAMModem's
host methods against the definition written as loops (tests/qam_ref.py), noise-free round trips,
pl_qam_check through the library, and the harness's refusal of the all-zero-codeword shortcut.

The definition: include/polarldpc.h at pl_qam_check.  host_inputs() is the input set the GPU tests share
(tests/test_gpu_qam.py)."""
import functools

import numpy as np
import pytest

import qam_ref as Q
from polarcode_and_ldpc_amd import _native
from polarcode_and_ldpc_amd.channel import QAMModem
from polarcode_and_ldpc_amd.channel.qam import sigma_of

MS = Q.MS


@functools.lru_cache(maxsize=None)
def modem(m):
    return QAMModem(m)


def bits_view(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def same_bits(got, want):
    """bit for bit outside NaN; NaN exactly where the other has NaN (payload unspecified)"""
    assert got.dtype == want.dtype and got.shape == want.shape
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), "NaN positions differ"
    return np.array_equal(bits_view(got)[~gn], bits_view(want)[~wn])


def specials(m):
    """axis values that sit on the demapper's edges: every level, every midpoint between neighbours
    (ties), +-0, +-1e200 (every distance overflows), +-inf, NaN"""
    h, sc = m // 2, Q.scale_of(m)
    lev = [float(a) * sc for a in range(-(2 ** h - 1), 2 ** h, 2)]
    mid = [(lev[i] + lev[i + 1]) / 2 for i in range(len(lev) - 1)]
    return np.array(lev + mid + [0.0, -0.0, 1e200, -1e200, np.inf, -np.inf, np.nan], dtype=np.float64)


def host_inputs(m, E, B, seed=0):
    """(bits uint8 [B, E] with any byte value, y float64 [B, 2 S]): y = the clean symbols plus noise, with
    the specials written over its first entries (row by row, wrapping over the rows)"""
    rng = np.random.default_rng(1000 * m + 7 * E + B + seed)
    bits = rng.integers(0, 256, size=(B, E), dtype=np.uint8)
    S = -(-E // m)
    y = Q_modulate_fast(bits, m) + 0.3 * rng.standard_normal((B, 2 * S))
    sp = specials(m)
    flat = y.reshape(-1)
    n = min(len(sp), flat.size)
    flat[:n] = sp[:n]
    if flat.size > len(sp):  # and once more from the end, so that the last (cut) symbol meets them too
        flat[-n:] = sp[:n][::-1]
    return bits, y


def Q_modulate_fast(bits, m):
    return modem(m).modulate_host(bits)


# ---- the constellation ----
@pytest.mark.parametrize("m", MS)
def test_constellation_properties(m):
    h = m // 2
    tab = Q.axis_table(h)
    levels = sorted(a for a, _ in tab)
    assert levels == list(range(-(2 ** h - 1), 2 ** h, 2))
    by_level = {a: b for a, b in tab}
    for a in levels[:-1]:  # Gray: neighbours differ in exactly one bit
        assert sum(x != y for x, y in zip(by_level[a], by_level[a + 2])) == 1
    assert by_level[2 ** h - 1] == [0] * h
    sc = Q.scale_of(m)
    pts = np.array([float(a) * sc for a in levels])
    energy = np.mean(pts[:, None] ** 2 + pts[None, :] ** 2)
    assert abs(energy - 1.0) <= 2 * np.spacing(1.0)
    x = modem(m).modulate_host(np.zeros((1, m), dtype=np.uint8))
    assert np.array_equal(x, np.full((1, 2), float(2 ** h - 1) * sc))
    assert modem(m).scale == sc and _native.qam_check(m, 1)[1] == sc


# ---- the host methods against the loops ----
@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("E,B", [(1, 3), (5, 2), (64, 2), (131, 3)])
def test_host_methods_equal_the_loops(m, E, B):
    bits, y = host_inputs(m, E, B)
    x = modem(m).modulate_host(bits)
    assert x.dtype == np.float64 and np.array_equal(bits_view(x), bits_view(Q.modulate(bits, m)))
    assert np.array_equal(bits_view(modem(m).modulate_host(bits[0])), bits_view(x[0]))
    snr = 7.5
    for dt in (np.float64, np.float32):
        got = modem(m).demap_host(y, E, snr, dtype=dt)
        want = Q.demap(y, E, m, sigma_of(snr), dtype=dt)
        assert same_bits(got, want)
        assert same_bits(modem(m).demap_host(y[0], E, snr, dtype=dt), want[0])


@pytest.mark.parametrize("m", MS)
def test_specials_give_nan_only_where_the_definition_does(m):
    sp = specials(m)
    E = m * ((len(sp) + 1) // 2)
    y = np.zeros((1, 2 * modem(m).S(E)))
    y[0, :len(sp)] = sp
    llr = modem(m).demap_host(y, E, 3.0)
    nan_axis = np.isnan(sp) | (np.abs(sp) >= 1e200)
    per_axis = llr.reshape(-1, m // 2, 2).transpose(0, 2, 1).reshape(-1, m // 2)[:len(sp)]  # [axis value, p]
    assert np.array_equal(np.isnan(per_axis), np.repeat(nan_axis[:, None], m // 2, axis=1))


@pytest.mark.parametrize("m", MS)
def test_noise_free_round_trip(m):
    for E in (1, m - 1, m, m + 1, 1000):
        bits = np.random.default_rng(m * 17 + E).integers(0, 2, size=(2, E), dtype=np.uint8)
        for dt in (np.float64, np.float32):
            llr = modem(m).demap_host(modem(m).modulate_host(bits), E, 10.0, dtype=dt)
            assert llr.shape == (2, E) and not np.any(llr == 0)
            assert np.array_equal((llr <= 0).astype(np.uint8), bits)


# ---- pl_qam_check ----
def test_qam_check_values():
    for m in MS:
        for E in (1, m - 1, m, m + 1, 1000, 2 ** 30 - 1, 2 ** 30):
            S, scale = _native.qam_check(m, E)
            assert S == -(-E // m)
            D = 2 * (4 ** (m // 2) - 1) // 3
            want = np.float64(1.0) / np.sqrt(np.float64(D))
            assert np.float64(scale).view(np.uint64) == want.view(np.uint64)
    assert [2 * (4 ** h - 1) // 3 for h in (1, 2, 3, 4)] == [2, 10, 42, 170]


def _refusal(m, E):
    S, scale = np.zeros(1, np.int64), np.zeros(1, np.float64)
    import ctypes
    rc = _native.lib.pl_qam_check(m, E, S.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                  scale.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
    assert rc == _native.PL_EINVAL
    with pytest.raises(AssertionError) as e:
        _native.qam_check(m, E)
    return str(e.value)


def test_qam_check_refusals_in_order():
    for m in (0, 1, 3, 5, 7, 9, 10, -2, 16):
        assert "m = %d must be 2, 4, 6 or 8" % m in _refusal(m, 8)
    assert "m = 3" in _refusal(3, 0)  # m comes first
    for E in (0, -1, 2 ** 30 + 1, 2 ** 40):
        assert "E = %d outside 1 .. 2^30" % E in _refusal(4, E)
    with pytest.raises(AssertionError):
        QAMModem(1)
    with pytest.raises(AssertionError):
        modem(4).S(0)


# ---- the harness ----
def test_all_zero_codeword_shortcut_is_refused():
    from polarcode_and_ldpc_amd.harness.montecarlo import ldpc_round_fn

    class DecoderStub:
        n, m, plan = 24, 12, None

    with pytest.raises(AssertionError, match="all-zero"):
        ldpc_round_fn(DecoderStub(), modulation=QAMModem(4))
    with pytest.raises(AssertionError, match="all-zero"):
        ldpc_round_fn(DecoderStub(), modulation=QAMModem(4), rate_matcher=object())


def test_pam_bit_error_prob_is_a_probability_and_bpsk_like_at_h1():
    import math
    s = 0.4
    (p,) = Q.pam_bit_error_prob(1, s)
    assert abs(p - 0.5 * math.erfc(Q.scale_of(2) / (s * math.sqrt(2)))) < 1e-15
    for h in (2, 3, 4):
        pr = Q.pam_bit_error_prob(h, 0.05)
        assert all(0 < v < 0.5 for v in pr) and pr == sorted(pr)  # the first bit is the best protected
        assert 1e-2 <= sum(Q.pam_bit_error_prob(h, sigma_of(Q.snr_for_error_rate(h)))) / h < 1e-1

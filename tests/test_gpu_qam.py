"""Gray-mapped QAM on the device (csrc/qam.hip) against channel.QAMModem's host methods, which
tests/test_qam_host.py holds to the definition's loops (tests/qam_ref.py); the noise against the stream
contract in mpmath; the uncoded error rate against the exact PAM figure; the harness chains; the C-ABI's
refusals.  The definition: include/polarldpc.h at pl_qam_check."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import channel_ref as R
import qam_ref as Q
from test_qam_host import bits_view, host_inputs, same_bits

pytestmark = pytest.mark.gpu

MS = Q.MS
TT = {np.float64: torch.float64, np.float32: torch.float32}
SENTINEL = -12345.5


def lengths(m):
    """E of the grid: one bit, one symbol and one past, a cut third symbol, around the float demapper's
    two-symbol group (2 m) -- whole groups and the cut one take different store paths --, around 64, long"""
    return sorted({1, m, m + 1, 3 * m - 1, 2 * m - 1, 2 * m, 2 * m + 1, 64, 65, 1000, 1027})


@functools.lru_cache(maxsize=None)
def modem(m):
    from polarcode_and_ldpc_amd.channel import QAMModem
    return QAMModem(m)


def _native():
    from polarcode_and_ldpc_amd import _native as n
    return n


def view(B, width, ld, off, dtype):
    """a [B, width] view of row pitch ld that starts off elements into a sentinel-filled flat tensor"""
    flat = torch.full((off + B * ld + 8,), 0 if dtype == torch.uint8 else SENTINEL, dtype=dtype, device="cuda")
    return flat, flat[off:off + B * ld].view(B, ld)[:, :width]


def only_view_written(flat, B, width, ld, off):
    h = flat.cpu().numpy().copy()
    rows = h[off:off + B * ld].reshape(B, ld)
    rows[:, :width] = SENTINEL
    return bool(np.all(h == SENTINEL))


# ---- modulate ----
@pytest.mark.parametrize("m", MS)
def test_modulate_equals_host(gpu, m):
    for B in (1, 67):
        for E in lengths(m):
            bits, _ = host_inputs(m, E, B)  # bytes 0 .. 255: bit 0 counts
            want = modem(m).modulate_host(bits)
            got = modem(m).modulate(torch.from_numpy(bits).cuda())
            assert got.dtype == torch.float64 and np.array_equal(bits_view(got.cpu().numpy()), bits_view(want)), (B, E)
            assert np.array_equal(bits_view(modem(m).modulate(bits)), bits_view(want))  # NumPy in, NumPy out
            # pitched bits and symbols, the symbols one element past a 16-byte boundary
            S2 = 2 * modem(m).S(E)
            _, e = view(B, E, E + 3, 1, torch.uint8)
            e.copy_(torch.from_numpy(bits))
            flat, x = view(B, S2, S2 + 1, 1, torch.float64)
            assert modem(m).modulate(e, out=x) is x
            assert np.array_equal(bits_view(x.cpu().numpy()), bits_view(want)), (B, E)
            assert only_view_written(flat, B, S2, S2 + 1, 1)


# ---- demap ----
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("m", MS)
def test_demap_equals_host(gpu, m, dtype):
    snr = 7.5
    for B in (1, 67):
        for E in lengths(m):
            _, y = host_inputs(m, E, B)
            want = modem(m).demap_host(y, E, snr, dtype=dtype)
            yd = torch.from_numpy(y).cuda()
            got = modem(m).demap(yd, E, snr, dtype=dtype)
            assert got.dtype == TT[dtype] and same_bits(got.cpu().numpy(), want), (B, E)
            assert same_bits(modem(m).demap(y, E, snr, dtype=dtype), want)  # NumPy in, NumPy out
            # pitched rows on both sides; the output starts 1, 2, 3 elements past a 16-byte boundary
            S2 = y.shape[1]
            _, yv = view(B, S2, S2 + 1, 1, torch.float64)
            yv.copy_(yd)
            for off in range(1, 16 // np.dtype(dtype).itemsize):
                flat, out = view(B, E, E + 3, off, TT[dtype])
                assert modem(m).demap(yv, E, snr, out=out) is out
                assert same_bits(out.cpu().numpy(), want), (B, E, off)
                assert only_view_written(flat, B, E, E + 3, off), (B, E, off)


# ---- awgn ----
@pytest.mark.parametrize("m", MS)
def test_awgn_against_mpmath(gpu, m):
    """every y within qam_awgn_bound_mp of the mpmath value; the largest error / bound is printed"""
    E, B, seed, off = 50, 3, 0x1234567890ABCDEF, (1 << 40) + 5
    S = modem(m).S(E)
    z = Q.qam_normals_mp(seed, off, B, S)
    bits, _ = host_inputs(m, E, B)
    worst = 0.0
    for snr in (0.0, 20.0):
        sigma = R.sigma_of(snr)
        for given in (bits, None):
            x = modem(m).modulate_host(bits if given is not None else np.zeros((B, E), np.uint8))
            y = modem(m).awgn(None if given is None else torch.from_numpy(given).cuda(), E, B, snr, seed, off)
            ratio = R.max_ratio(y.cpu().numpy(), Q.qam_awgn_mp(x, z, sigma), Q.qam_awgn_bound_mp(x, z, sigma))
            worst = max(worst, ratio)
    print("qam awgn m=%d: largest error / bound = %.3f" % (m, worst))
    assert worst <= 1.0


@pytest.mark.parametrize("m", MS)
def test_awgn_maps_every_length(gpu, m):
    """y - x is the frame's noise whatever the bits and the length: the mapping inside the fused kernel"""
    snr, seed = 3.0, 99
    sigma = R.sigma_of(snr)
    for B in (1, 67):
        for E in lengths(m):
            bits, _ = host_inputs(m, E, B)
            S = modem(m).S(E)
            noise = sigma * Q.qam_normals_np(seed, 11, B, S)
            y = modem(m).awgn(bits, E, B, snr, seed, 11)
            assert isinstance(y, np.ndarray) and np.allclose(y - modem(m).modulate_host(bits), noise, rtol=0, atol=1e-12)
            y0 = modem(m).awgn(None, E, B, snr, seed, 11)
            zero = modem(m).awgn(torch.zeros((B, E), dtype=torch.uint8, device="cuda"), E, B, snr, seed, 11)
            assert torch.equal(y0, zero)
            flat, out = view(B, 2 * S, 2 * S + 1, 1, torch.float64)  # pitched, misaligned rows
            modem(m).awgn(torch.from_numpy(bits).cuda(), E, B, snr, seed, 11, out=out)
            assert np.array_equal(bits_view(out.cpu().numpy()), bits_view(y)) and only_view_written(flat, B, 2 * S, 2 * S + 1, 1)


def test_awgn_frames_do_not_depend_on_the_batch(gpu):
    m, E, B, snr, seed = 6, 100, 9, 2.0, 7
    bits = torch.from_numpy(host_inputs(m, E, B)[0]).cuda()
    whole = modem(m).awgn(bits, E, B, snr, seed, 0)
    side = torch.cuda.Stream()
    for f in range(B):
        one = modem(m).awgn(bits[f:f + 1], E, 1, snr, seed, f)
        assert torch.equal(one[0], whole[f])
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        again = modem(m).awgn(bits, E, B, snr, seed, 0, stream=side)
    side.synchronize()
    assert torch.equal(again, whole)
    assert not torch.equal(modem(m).awgn(bits, E, B, snr, seed + 1, 0), whole)


def test_awgn_noise_moments(gpu):
    m, E, B, snr = 4, 1024, 2048, 5.0
    bits = torch.from_numpy(np.random.default_rng(1).integers(0, 2, (B, E), dtype=np.uint8)).cuda()
    y = modem(m).awgn(bits, E, B, snr, 2024, 0)
    z = ((y - modem(m).modulate(bits)) / R.sigma_of(snr)).cpu().numpy().ravel()
    n = z.size
    assert n == 1 << 20
    assert abs(z.mean()) <= 5 / math.sqrt(n)
    assert abs(z.var() - 1.0) <= 5 * math.sqrt(2.0 / n)


# ---- the uncoded error rate ----
@pytest.mark.parametrize("m", MS)
def test_uncoded_error_rate(gpu, m):
    """llr <= 0 against the sent bits, per bit index of the symbol: each count within 5 binomial standard
    errors of pam_bit_error_prob at an Es/N0 chosen from that function (bits 2 p and 2 p + 1 share the
    figure of axis bit p).  Pins sigma's Es/N0 convention and the bit-to-axis order end to end."""
    h = m // 2
    snr = Q.snr_for_error_rate(h)
    prob = Q.pam_bit_error_prob(h, R.sigma_of(snr))
    assert 1e-2 <= sum(prob) / h < 1e-1
    S, B = -(-1024 // m), 1024
    E = S * m
    bits = np.random.default_rng(m).integers(0, 2, (B, E), dtype=np.uint8)
    bd = torch.from_numpy(bits).cuda()
    llr = modem(m).demap(modem(m).awgn(bd, E, B, snr, 31337, 0), E, snr)
    wrong = ((llr <= 0).to(torch.uint8) != bd).cpu().numpy().reshape(B, S, m)
    n = B * S
    assert n * m >= 1 << 20
    for i in range(m):
        p = prob[i // 2]
        got = int(wrong[:, :, i].sum())
        print("m=%d bit %d: %d errors, expected %.1f +- %.1f" % (m, i, got, n * p, math.sqrt(n * p * (1 - p))))
        assert abs(got - n * p) <= 5 * math.sqrt(n * p * (1 - p)), (m, i, snr)


# ---- the chains ----
def test_polar_chain(gpu):
    import polarcode_and_ldpc_amd.polar as P
    from polarcode_and_ldpc_amd.harness.montecarlo import polar_round_fn
    N, K, E = 256, 100, 200
    rm = P.PolarRateMatcher(N, E, "puncture")
    dec = P.SCLDecoder(N, K, list_size=4, frozen_bits=P.construct_rate_matched(K, rm))
    assert polar_round_fn(dec, seed=5, rate_matcher=rm, modulation=modem(4))(0, 30.0, 0, 256).tolist() == [0, 0, 256]
    low = polar_round_fn(dec, seed=5, rate_matcher=rm, modulation=modem(4))(1, 2.0, 0, 256)
    assert low[2] == 256 and low[1] > 0  # 16-QAM at 2 dB does fail: the counters are not trivially 0
    plain = P.SCLDecoder(N, 128, list_size=4, frozen_bits=P.construct_frozen_set(N, 128))
    assert polar_round_fn(plain, seed=5, modulation=modem(8))(0, 40.0, 0, 256).tolist() == [0, 0, 256]
    # the default path: the counts of a call written without the new argument
    for kw in ({}, {"rate_matcher": rm}):
        d = dec if kw else plain
        assert polar_round_fn(d, seed=5, modulation=None, **kw)(1, 1.0, 3, 256).tolist() == \
            polar_round_fn(d, seed=5, **kw)(1, 1.0, 3, 256).tolist()


def test_ldpc_chain(gpu):
    import polarcode_and_ldpc_amd.ldpc as L
    from polarcode_and_ldpc_amd.harness.montecarlo import ldpc_round_fn
    Z = 27
    base = L.qc_encodable_base(8, 12, Z, 3, 2, core=4, chained=False)
    enc = L.QCLDPCEncoder(base, Z)
    rm = L.QCRateMatcher(base, Z, 260, punctured=2, fillers=5, start=0)
    decs = [L.QCLayeredMSDecoder(rm.decoder_base(), Z, max_iter=20, normalization=0.75, early_stop=True, dtype=dt)
            for dt in (np.float64, np.float32)]
    decs.append(L.QCFixedMSDecoder(rm.decoder_base(), Z, max_iter=20, normalization=0.75))
    for dec in decs:
        f = ldpc_round_fn(dec, seed=3, encoder=enc, rate_matcher=rm, modulation=modem(6))
        assert f(0, 30.0, 0, 256).tolist() == [0, 0, 256], dec
        assert f(1, 30.0, 256, 100).tolist() == [0, 0, 100], dec  # a smaller round on the same buffers
    low = ldpc_round_fn(decs[0], seed=3, encoder=enc, rate_matcher=rm, modulation=modem(6))(1, 4.0, 0, 256)
    assert low[2] == 256 and low[1] > 0
    # the whole codeword, no matcher
    for dt in (np.float64, np.float32):
        dec = L.QCLayeredMSDecoder(base, Z, max_iter=20, normalization=0.75, early_stop=True, dtype=dt)
        assert ldpc_round_fn(dec, seed=3, encoder=enc, modulation=modem(6))(0, 30.0, 0, 256).tolist() == [0, 0, 256]
    fx = L.QCFixedMSDecoder(base, Z, max_iter=20, normalization=0.75)
    assert ldpc_round_fn(fx, seed=3, encoder=enc, modulation=modem(2))(0, 30.0, 0, 256).tolist() == [0, 0, 256]
    # the default path: the counts of a call written without the new argument
    for e in (None, enc):
        for kw in ({}, {"rate_matcher": rm}):
            d = decs[1] if kw else dec
            assert ldpc_round_fn(d, seed=3, encoder=e, modulation=None, **kw)(1, -1.0, 7, 256).tolist() == \
                ldpc_round_fn(d, seed=3, encoder=e, **kw)(1, -1.0, 7, 256).tolist()
    with pytest.raises(AssertionError, match="all-zero"):
        ldpc_round_fn(dec, modulation=modem(4))


def test_simulate_and_cli(gpu, capsys):
    import json
    import polarcode_and_ldpc_amd.ldpc as L
    from polarcode_and_ldpc_amd.harness import ber
    cfg = {"encoding": {"N": 256, "K": 100}}
    b, f, pts = ber.simulate_polar([30.0], 256, 100, cfg, list_size=4, batch=256, rate_match=dict(E=200, mode="puncture"),
                                   modulation=modem(4))
    assert pts[0].frames == 256 and pts[0].frame_errors == 0
    base = L.qc_encodable_base(8, 12, 27, 3, 2, core=4, chained=False)
    b, f, pts = ber.simulate_qc_ldpc([30.0], 256, 100, base, 27, batch=256, random_codewords=True,
                                     rate_match=(260, 2, 5), modulation=modem(6), dtype=np.float32)
    assert pts[0].frames == 256 and pts[0].frame_errors == 0
    with pytest.raises(AssertionError, match="all-zero"):
        ber.simulate_qc_ldpc([30.0], 256, 100, base, 27, batch=256, modulation=modem(6))
    ber.main(["--code", "polar", "--N", "256", "--K", "100", "--list-size", "4", "--polar-rm", "200,puncture",
              "--modulation", "16qam", "--snr=30:30:1", "--frames", "256", "--batch", "256"])
    res = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert res["points"][0]["frames"] == 256 and res["points"][0]["frame_errors"] == 0


# ---- the C-ABI ----
def test_capi_refusals(gpu):
    n = _native()
    lib, EINVAL = n.lib, n.PL_EINVAL
    m, E, B = 4, 10, 2
    S2 = 6
    e = torch.zeros((B, E), dtype=torch.uint8, device="cuda")
    x = torch.full((B, S2 + 2), SENTINEL, dtype=torch.float64, device="cuda")
    l64 = torch.full((B, E + 2), SENTINEL, dtype=torch.float64, device="cuda")
    l32 = torch.full((B, E + 2), SENTINEL, dtype=torch.float32, device="cuda")
    ep, xp, lp, fp = e.data_ptr(), x.data_ptr(), l64.data_ptr(), l32.data_ptr()
    st = n._stream()
    u64 = ctypes.c_uint64

    def mod(m=m, E=E, B=B, e=ep, lde=E, x=xp, ldx=S2 + 2):
        return lib.pl_qam_modulate(m, E, B, e, lde, x, ldx, st)

    def awgn(m=m, E=E, B=B, e=ep, lde=E, snr=3.0, y=xp, ldy=S2 + 2):
        return lib.pl_qam_awgn(m, E, B, e, lde, snr, u64(1), 0, y, ldy, st)

    def demap(m=m, E=E, B=B, y=xp, ldy=S2 + 2, snr=3.0, llr=lp, ldl=E + 2, flags=0):
        return lib.pl_qam_demap(m, E, B, y, ldy, snr, llr, ldl, flags, st)

    def refused(rc, word):
        msg = (lib.pl_last_error() or b"").decode()
        assert rc == EINVAL and word in msg, (rc, msg, word)

    for fn in (mod, awgn, demap):
        refused(fn(m=3), "m = 3")
        refused(fn(m=0), "m = 0")
        refused(fn(E=0), "E = 0")
        refused(fn(E=(1 << 30) + 1), "E = ")
        refused(fn(B=-1), "batch")
    refused(mod(e=None), "NULL")
    refused(mod(x=None), "NULL")
    refused(awgn(y=None), "NULL")
    refused(demap(y=None), "NULL")
    refused(demap(llr=None), "NULL")
    refused(mod(lde=E - 1), "ld_e")
    refused(awgn(lde=E - 1), "ld_e")
    refused(mod(ldx=S2 - 1), "ld_x")
    refused(awgn(ldy=S2 - 1), "ld_y")
    refused(demap(ldy=S2 - 1), "ld_y")
    refused(demap(ldl=E - 1), "ld_llr")
    refused(demap(flags=2), "flag")
    refused(demap(flags=-1), "flag")
    for bad in (math.nan, math.inf, -math.inf):
        refused(awgn(snr=bad), "snr_db")
        refused(demap(snr=bad), "snr_db")
    refused(mod(x=xp + 4), "aligned")
    refused(awgn(y=xp + 4), "aligned")
    refused(demap(y=xp + 4), "aligned")
    refused(demap(llr=lp + 4), "aligned")
    refused(demap(llr=fp + 2, flags=n.PL_QAM_LLR_F32), "aligned")
    assert awgn(e=None, lde=0) == 0  # NULL bits: the all-zero frame, ld_e unused
    assert demap(llr=fp + 4, flags=n.PL_QAM_LLR_F32) == 0  # a float pointer needs 4-byte alignment only
    torch.cuda.synchronize()
    # batch == 0 launches nothing, whatever the pointers
    x.fill_(SENTINEL)
    l64.fill_(SENTINEL)
    assert mod(B=0, e=None, x=None) == 0 and awgn(B=0, y=None) == 0 and demap(B=0, y=None, llr=None) == 0
    assert mod(B=0) == 0 and awgn(B=0) == 0 and demap(B=0) == 0
    torch.cuda.synchronize()
    assert bool((x == SENTINEL).all()) and bool((l64 == SENTINEL).all())
    # nothing was launched by a refused call either
    assert bool((e == 0).all())

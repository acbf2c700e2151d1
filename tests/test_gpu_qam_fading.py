"""Block Rayleigh fading for the QAM symbols on the device (csrc/qam.hip: qam_rayleigh_kernel,
qam_demap_csi_kernel) against channel.QAMModem's host methods, which tests/test_qam_fading_host.py holds to the
definition's loops (tests/qam_fading_ref.py); the coefficients and the received symbols against the stream contract
in mpmath; the uncoded error rate under fast fading against the closed form; the harness chains; the C-ABI's
refusals.  The definition: include/polarldpc.h at pl_qam_fading_check."""
import ctypes
import json
import math

import numpy as np
import pytest
import torch

import channel_ref as R
import qam_fading_ref as F
import qam_ref as Q
from test_gpu_qam import SENTINEL, TT, lengths, modem, only_view_written, view
from test_qam_fading_host import fading_inputs
from test_qam_host import bits_view, host_inputs, same_bits

pytestmark = pytest.mark.gpu

MS = Q.MS
FRAME = 2 ** 30


def grid(m):
    """(B, E, S, Lc) of the grid: test_gpu_qam's lengths, one frame and several blocks of threads, fast fading,
    short blocks, exactly the frame, quasi-static"""
    for B in (1, 67):
        for E in lengths(m):
            S = -(-E // m)
            for Lc in sorted({1, 3, S, FRAME}):
                yield B, E, S, Lc


def _native():
    from polarcode_and_ldpc_amd import _native as n
    return n


# ---- demap_csi ----
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("m", MS)
def test_demap_csi_equals_host(gpu, m, dtype):
    snr = 7.5
    for B, E, S, Lc in grid(m):
        y, h = fading_inputs(m, E, B, Lc)  # the specials of both included
        nq = F.blocks(S, Lc)
        want = modem(m).demap_csi_host(y, h, E, snr, coherence=Lc, dtype=dtype)
        yd, hd = torch.from_numpy(y).cuda(), torch.from_numpy(h).cuda()
        got = modem(m).demap_csi(yd, hd, E, snr, coherence=Lc, dtype=dtype)
        assert got.dtype == TT[dtype] and same_bits(got.cpu().numpy(), want), (B, E, Lc)
        if Lc == 3:  # NumPy in, NumPy out
            assert same_bits(modem(m).demap_csi(y, h, E, snr, coherence=Lc, dtype=dtype), want)
        # pitched rows on all three sides: y and h one element past a 16-byte boundary, the output 1, 2, 3 past
        _, yv = view(B, 2 * S, 2 * S + 1, 1, torch.float64)
        yv.copy_(yd)
        _, hv = view(B, 2 * nq, 2 * nq + 1, 1, torch.float64)
        hv.copy_(hd)
        for off in range(1, 16 // np.dtype(dtype).itemsize):
            flat, out = view(B, E, E + 3, off, TT[dtype])
            assert modem(m).demap_csi(yv, hv, E, snr, coherence=Lc, out=out) is out
            assert same_bits(out.cpu().numpy(), want), (B, E, Lc, off)
            assert only_view_written(flat, B, E, E + 3, off), (B, E, Lc, off)


@pytest.mark.parametrize("m", MS)
def test_unit_gain_equals_the_awgn_demapper(gpu, m):
    """the two kernels on the same finite y, h = (1.0, 0.0): bit for bit"""
    E, B = 1027, 5
    y = host_inputs(m, E, B)[1]
    y = torch.from_numpy(np.where(np.isfinite(y), y, 0.25)).cuda()
    h = torch.zeros((B, 2 * modem(m).S(E)), dtype=torch.float64, device="cuda")
    h[:, 0::2] = 1.0
    for dt in (np.float64, np.float32):
        got = modem(m).demap_csi(y, h, E, 7.5, coherence=1, dtype=dt)
        assert same_bits(got.cpu().numpy(), modem(m).demap(y, E, 7.5, dtype=dt).cpu().numpy())  # NaN at +-1e200


# ---- rayleigh ----
@pytest.mark.parametrize("m", MS)
def test_rayleigh_against_the_definition(gpu, m):
    """y against fade() on the device's own coefficients and the stream's noise (pins the block index and the
    operation order up to the normals' last bits), h against the stream's normals times C"""
    snr, seed, off = 3.0, 99, 11
    sigma = R.sigma_of(snr)
    for B, E, S, Lc in grid(m):
        nq = F.blocks(S, Lc)
        bits, _ = host_inputs(m, E, B)
        y, h = modem(m).rayleigh(bits, E, B, snr, seed, coherence=Lc, frame_offset=off)
        assert isinstance(y, np.ndarray) and isinstance(h, np.ndarray) and y.shape == (B, 2 * S) and h.shape == (B, 2 * nq)
        x = modem(m).modulate_host(bits)
        noise = sigma * Q.qam_normals_np(seed, off, B, S)
        assert np.allclose(y, modem(m).fade_host(x, h, noise, Lc), rtol=0, atol=1e-12), (B, E, Lc)
        if B == 1:  # and the loops themselves, where they are cheap
            assert np.allclose(y, F.fade(x, h, noise, Lc), rtol=0, atol=1e-12), (E, Lc)
        assert np.allclose(h, F.fade_normals_np(seed, off, B, nq) * F.C, rtol=0, atol=1e-12), (B, E, Lc)
        # a coefficient depends on (seed, f, q) only: the fast-fading call's first Q are these, bit for bit
        bd = torch.from_numpy(bits).cuda()
        _, h1 = modem(m).rayleigh(bd, E, B, snr, seed, coherence=1, frame_offset=off)
        assert np.array_equal(bits_view(h1[:, :2 * nq].cpu().numpy()), bits_view(h)), (B, E, Lc)
        # no bits: the all-zero bits
        y0, h0 = modem(m).rayleigh(None, E, B, snr, seed, coherence=Lc, frame_offset=off)
        yz, hz = modem(m).rayleigh(torch.zeros_like(bd), E, B, snr, seed, coherence=Lc, frame_offset=off)
        assert torch.equal(y0, yz) and torch.equal(h0, hz) and np.array_equal(bits_view(h0.cpu().numpy()), bits_view(h))
        # pitched, misaligned rows on both outputs
        fy, oy = view(B, 2 * S, 2 * S + 1, 1, torch.float64)
        fh, oh = view(B, 2 * nq, 2 * nq + 1, 1, torch.float64)
        ry, rh = modem(m).rayleigh(bd, E, B, snr, seed, coherence=Lc, frame_offset=off, out=oy, h_out=oh)
        assert ry is oy and rh is oh
        assert np.array_equal(bits_view(oy.cpu().numpy()), bits_view(y)) and np.array_equal(bits_view(oh.cpu().numpy()), bits_view(h))
        assert only_view_written(fy, B, 2 * S, 2 * S + 1, 1) and only_view_written(fh, B, 2 * nq, 2 * nq + 1, 1)


@pytest.mark.parametrize("m", MS)
def test_rayleigh_against_mpmath(gpu, m):
    """every h and y within qam_fading_ref.rayleigh_bound_mp (its docstring derives it) of the mpmath value; the
    largest error / bound is printed"""
    E, B, Lc, seed, off = 50, 3, 3, 0x1234567890ABCDEF, (1 << 40) + 5
    S = modem(m).S(E)
    nq = F.blocks(S, Lc)
    z = Q.qam_normals_mp(seed, off, B, S)
    g = F.fade_normals_mp(seed, off, B, nq)
    bits, _ = host_inputs(m, E, B)
    x = modem(m).modulate_host(bits)
    worst_h = worst_y = 0.0
    for snr in (0.0, 20.0):
        sigma = R.sigma_of(snr)
        y, h = modem(m).rayleigh(torch.from_numpy(bits).cuda(), E, B, snr, seed, coherence=Lc, frame_offset=off)
        h_mp, y_mp = F.rayleigh_mp(x, g, z, sigma, Lc)
        bh, by = F.rayleigh_bound_mp(x, g, z, sigma, Lc)
        worst_h = max(worst_h, R.max_ratio(h.cpu().numpy(), h_mp, bh))
        worst_y = max(worst_y, R.max_ratio(y.cpu().numpy(), y_mp, by))
    print("qam rayleigh m=%d: largest error / bound = %.3f (h), %.3f (y)" % (m, worst_h, worst_y))
    assert worst_h <= 1.0 and worst_y <= 1.0


@pytest.mark.parametrize("m", MS)
def test_noise_is_the_awgn_calls(gpu, m):
    """with equal seeds, rayleigh's y - h x and awgn's y - x are the same noise"""
    E, B, snr, seed, off = 203, 7, 4.0, 4242, 3
    bits = host_inputs(m, E, B)[0]
    x = modem(m).modulate_host(bits)
    for Lc in (1, 5, FRAME):
        y, h = modem(m).rayleigh(bits, E, B, snr, seed, coherence=Lc, frame_offset=off)
        hx = modem(m).fade_host(x, h, np.zeros_like(x), Lc)
        ya = modem(m).awgn(bits, E, B, snr, seed, off)
        assert np.allclose(y - hx, ya - x, rtol=0, atol=1e-12), Lc
        assert np.abs(ya - x).max() > 1e-3


def test_frames_do_not_depend_on_the_batch(gpu):
    m, E, B, Lc, snr, seed = 6, 100, 9, 4, 2.0, 7
    bits = torch.from_numpy(host_inputs(m, E, B)[0]).cuda()
    wy, wh = modem(m).rayleigh(bits, E, B, snr, seed, coherence=Lc)
    for f in range(B):
        y1, h1 = modem(m).rayleigh(bits[f:f + 1], E, 1, snr, seed, coherence=Lc, frame_offset=f)
        assert torch.equal(y1[0], wy[f]) and torch.equal(h1[0], wh[f])
    ya, ha = modem(m).rayleigh(bits[:4], E, 4, snr, seed, coherence=Lc, frame_offset=0)  # the offset split
    yb, hb = modem(m).rayleigh(bits[4:], E, B - 4, snr, seed, coherence=Lc, frame_offset=4)
    assert torch.equal(torch.cat([ya, yb]), wy) and torch.equal(torch.cat([ha, hb]), wh)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        sy, sh = modem(m).rayleigh(bits, E, B, snr, seed, coherence=Lc, stream=side)
        sl = modem(m).demap_csi(sy, sh, E, snr, coherence=Lc, stream=side)
    side.synchronize()
    assert torch.equal(sy, wy) and torch.equal(sh, wh)
    assert torch.equal(sl, modem(m).demap_csi(wy, wh, E, snr, coherence=Lc))
    oy, oh = modem(m).rayleigh(bits, E, B, snr, seed + 1, coherence=Lc)
    assert not torch.equal(oh, wh) and not torch.equal(oy, wy)


def test_coefficient_moments(gpu):
    """2^20 coefficients: each component N(0, 1/2), |h|^2 ~ Exp(1) (mean 1, variance 1), at 5 standard errors"""
    m, S, B = 4, 1024, 1024
    _, h = modem(m).rayleigh(None, S * m, B, 10.0, 2025, coherence=1)
    h = h.cpu().numpy()
    n = B * S
    assert h.shape == (B, 2 * S) and n == 1 << 20
    for part in (h[:, 0::2].ravel(), h[:, 1::2].ravel()):
        assert abs(part.mean()) <= 5 / math.sqrt(n)
        assert abs(part.var() - 0.5) <= 5 * math.sqrt(2.0 / n) / 2
    g = h[:, 0::2] ** 2 + h[:, 1::2] ** 2
    assert abs(g.mean() - 1.0) <= 5 / math.sqrt(n)
    # independence of the two parts, and of neighbouring blocks
    assert abs(np.mean(h[:, 0::2] * h[:, 1::2])) <= 5 * 0.5 / math.sqrt(n)
    assert abs(np.mean(h[:, 0:-2:2] * h[:, 2::2])) <= 5 * 0.5 / math.sqrt(n - B)


# ---- the uncoded error rate under fast fading ----
@pytest.mark.parametrize("m", MS)
def test_uncoded_error_rate(gpu, m):
    """llr <= 0 against the sent bits, per bit index of the symbol, Lc = 1 (independent symbols): each count within
    5 binomial standard errors of rayleigh_pam_bit_error_prob at the Es/N0 its search gives.  Pins the sign of the
    weight w g, the conjugate in u and sigma's convention end to end."""
    hb = m // 2
    snr = F.snr_for_error_rate(hb)
    prob = F.rayleigh_pam_bit_error_prob(hb, R.sigma_of(snr))
    assert 1e-2 <= sum(prob) / hb < 1e-1
    S, B = -(-1024 // m), 1024
    E = S * m
    bits = np.random.default_rng(m).integers(0, 2, (B, E), dtype=np.uint8)
    bd = torch.from_numpy(bits).cuda()
    y, h = modem(m).rayleigh(bd, E, B, snr, 31337, coherence=1)
    llr = modem(m).demap_csi(y, h, E, snr, coherence=1)
    wrong = ((llr <= 0).to(torch.uint8) != bd).cpu().numpy().reshape(B, S, m)
    n = B * S
    assert n * m >= 1 << 20
    for i in range(m):
        p = prob[i // 2]
        got = int(wrong[:, :, i].sum())
        print("m=%d at %.1f dB bit %d: %d errors, expected %.1f +- %.1f" % (m, snr, i, got, n * p, math.sqrt(n * p * (1 - p))))
        assert abs(got - n * p) <= 5 * math.sqrt(n * p * (1 - p)), (m, i, snr)


# ---- the chains ----
def fadings(E):
    """(fading, interleaver): fast, blocks of 16 symbols behind a triangular interleaver, quasi-static"""
    from polarcode_and_ldpc_amd.channel import BitInterleaver
    return [(1, None), (16, BitInterleaver("tri", E)), (FRAME, None)]


def test_polar_chain(gpu):
    import polarcode_and_ldpc_amd.polar as P
    from polarcode_and_ldpc_amd.harness.montecarlo import polar_round_fn
    N, K, E = 256, 100, 200
    rm = P.PolarRateMatcher(N, E, "puncture")
    dec = P.SCLDecoder(N, K, list_size=4, frozen_bits=P.construct_rate_matched(K, rm))
    for fading, ilv in fadings(E):
        f = polar_round_fn(dec, seed=5, rate_matcher=rm, modulation=modem(4), interleaver=ilv, fading=fading)
        assert f(0, 60.0, 0, 256).tolist() == [0, 0, 256], fading
    low = polar_round_fn(dec, seed=5, rate_matcher=rm, modulation=modem(4), fading=1)(1, 2.0, 0, 256)
    assert low[2] == 256 and low[1] > 0  # it does fail at 2 dB: the counters are not trivially 0
    plain = P.SCLDecoder(N, 128, list_size=4, frozen_bits=P.construct_frozen_set(N, 128))
    assert polar_round_fn(plain, seed=5, modulation=modem(4), fading=1)(0, 60.0, 0, 256).tolist() == [0, 0, 256]
    # the default path: the counts of a call written without the new argument
    for kw in ({}, {"rate_matcher": rm}):
        d = dec if kw else plain
        for mod in (None, modem(4)):
            assert polar_round_fn(d, seed=5, modulation=mod, fading=None, **kw)(1, 1.0, 3, 256).tolist() == \
                polar_round_fn(d, seed=5, modulation=mod, **kw)(1, 1.0, 3, 256).tolist()
    for kw in ({}, {"rate_matcher": rm}):
        with pytest.raises(AssertionError, match="fading needs a modulation"):
            polar_round_fn(dec if kw else plain, fading=4, **kw)


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
        for fading, ilv in fadings(rm.E):
            f = ldpc_round_fn(dec, seed=3, encoder=enc, rate_matcher=rm, modulation=modem(6), interleaver=ilv,
                              fading=fading)
            assert f(0, 60.0, 0, 256).tolist() == [0, 0, 256], (dec, fading)
    low = ldpc_round_fn(decs[0], seed=3, encoder=enc, rate_matcher=rm, modulation=modem(6), fading=1)(1, 2.0, 0, 256)
    assert low[2] == 256 and low[1] > 0
    # the whole codeword, no matcher
    whole = L.QCLayeredMSDecoder(base, Z, max_iter=20, normalization=0.75, early_stop=True, dtype=np.float32)
    assert ldpc_round_fn(whole, seed=3, encoder=enc, modulation=modem(6), fading=1)(0, 60.0, 0, 256).tolist() == [0, 0, 256]
    # the default path: the counts of a call written without the new argument
    for kw in ({}, {"rate_matcher": rm}):
        d = decs[1] if kw else whole
        for mod in (None, modem(6)):
            assert ldpc_round_fn(d, seed=3, encoder=enc, modulation=mod, fading=None, **kw)(1, -1.0, 7, 256).tolist() == \
                ldpc_round_fn(d, seed=3, encoder=enc, modulation=mod, **kw)(1, -1.0, 7, 256).tolist()
    for kw in ({}, {"rate_matcher": rm}):
        with pytest.raises(AssertionError, match="fading needs a modulation"):
            ldpc_round_fn(decs[1] if kw else whole, encoder=enc, fading=4, **kw)


def test_simulate_and_cli(gpu, capsys, tmp_path):
    import polarcode_and_ldpc_amd.ldpc as L
    from polarcode_and_ldpc_amd.harness import ber
    cfg = {"encoding": {"N": 256, "K": 100}}
    log = tmp_path / "polar.jsonl"
    b, f, pts = ber.simulate_polar([60.0], 256, 100, cfg, list_size=4, batch=256, rate_match=dict(E=200, mode="puncture"),
                                   modulation=modem(4), fading=4, log_path=str(log))
    assert pts[0].frames == 256 and pts[0].frame_errors == 0
    assert '"fading": 4' in log.read_text()
    base = L.qc_encodable_base(8, 12, 27, 3, 2, core=4, chained=False)
    log2 = tmp_path / "qc.jsonl"
    b, f, pts = ber.simulate_qc_ldpc([60.0], 256, 100, base, 27, batch=256, random_codewords=True,
                                     rate_match=(260, 2, 5), modulation=modem(6), dtype=np.float32, fading=4,
                                     log_path=str(log2))
    assert pts[0].frames == 256 and pts[0].frame_errors == 0
    assert '"fading": 4' in log2.read_text()
    log3 = tmp_path / "plain.jsonl"
    ber.simulate_polar([30.0], 256, 100, cfg, list_size=4, batch=256, modulation=modem(4), log_path=str(log3))
    assert "fading" not in log3.read_text()
    with pytest.raises(AssertionError, match="fading needs a modulation"):
        ber.simulate_polar([60.0], 256, 100, cfg, list_size=4, batch=256, fading=4)
    common = ["--code", "polar", "--N", "256", "--K", "100", "--list-size", "4", "--polar-rm", "200,puncture",
              "--modulation", "16qam", "--snr=60:60:1", "--frames", "256", "--batch", "256"]
    for i, (extra, key) in enumerate(((["--fading", "4"], 4), (["--fading", "frame"], FRAME), ([], None))):
        path = tmp_path / ("cli%d.jsonl" % i)
        ber.main(common + extra + ["--log", str(path)])
        res = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
        assert res["points"][0]["frames"] == 256
        if key == 4:
            assert res["points"][0]["frame_errors"] == 0
        run = json.loads(path.read_text().splitlines()[0])["key"]
        assert run.get("fading") == key and ("fading" in run) == (key is not None)
    with pytest.raises(SystemExit):
        ber.main(common + ["--fading", "soon"])
    capsys.readouterr()


# ---- the C-ABI ----
def test_capi_refusals(gpu):
    n = _native()
    lib, EINVAL = n.lib, n.PL_EINVAL
    m, E, B, Lc = 4, 10, 2, 2
    S2, Q2 = 6, 4
    e = torch.zeros((B, E), dtype=torch.uint8, device="cuda")
    x = torch.full((B, S2 + 2), SENTINEL, dtype=torch.float64, device="cuda")
    hh = torch.full((B, Q2 + 2), SENTINEL, dtype=torch.float64, device="cuda")
    l64 = torch.full((B, E + 2), SENTINEL, dtype=torch.float64, device="cuda")
    l32 = torch.full((B, E + 2), SENTINEL, dtype=torch.float32, device="cuda")
    ep, xp, hp, lp, fp = e.data_ptr(), x.data_ptr(), hh.data_ptr(), l64.data_ptr(), l32.data_ptr()
    st = n._stream()
    u64 = ctypes.c_uint64

    def ray(m=m, E=E, Lc=Lc, B=B, e=ep, lde=E, snr=3.0, y=xp, ldy=S2 + 2, h=hp, ldh=Q2 + 2):
        return lib.pl_qam_rayleigh(m, E, Lc, B, e, lde, snr, u64(1), 0, y, ldy, h, ldh, st)

    def demap(m=m, E=E, Lc=Lc, B=B, y=xp, ldy=S2 + 2, h=hp, ldh=Q2 + 2, snr=3.0, llr=lp, ldl=E + 2, flags=0):
        return lib.pl_qam_demap_csi(m, E, Lc, B, y, ldy, h, ldh, snr, llr, ldl, flags, st)

    def refused(rc, word):
        msg = (lib.pl_last_error() or b"").decode()
        assert rc == EINVAL and word in msg, (rc, msg, word)

    for fn in (ray, demap):
        refused(fn(m=3), "m = 3")
        refused(fn(m=0), "m = 0")
        refused(fn(E=0), "E = 0")
        refused(fn(E=(1 << 30) + 1), "E = ")
        refused(fn(Lc=0), "coherence = 0")
        refused(fn(Lc=(1 << 30) + 1), "coherence = %d" % ((1 << 30) + 1))
        refused(fn(m=3, Lc=0), "m = 3")  # the conditions' order
        refused(fn(B=-1), "batch")
        refused(fn(y=None), "NULL")
        refused(fn(h=None), "h_dev")
        refused(fn(y=xp + 4), "aligned")
        refused(fn(h=hp + 4), "aligned")
        refused(fn(ldy=S2 - 1), "ld_y")
        refused(fn(ldh=Q2 - 1), "ld_h")
        for bad in (math.nan, math.inf, -math.inf):
            refused(fn(snr=bad), "snr_db")
    refused(ray(lde=E - 1), "ld_e")
    refused(demap(llr=None), "NULL")
    refused(demap(ldl=E - 1), "ld_llr")
    refused(demap(flags=2), "flag")
    refused(demap(flags=-1), "flag")
    refused(demap(llr=lp + 4), "aligned")
    refused(demap(llr=fp + 2, flags=n.PL_QAM_LLR_F32), "aligned")
    torch.cuda.synchronize()
    # nothing was launched by a refused call
    assert bool((x == SENTINEL).all()) and bool((hh == SENTINEL).all()) and bool((l64 == SENTINEL).all())
    # batch == 0 launches nothing, whatever the pointers (NULL, or poisoned ones that no kernel may touch)
    poison = 0xDEAD0000
    assert ray(B=0, e=None, y=None, h=None) == 0 and demap(B=0, y=None, h=None, llr=None) == 0
    assert ray(B=0, e=poison, y=poison, h=poison) == 0 and demap(B=0, y=poison, h=poison, llr=poison) == 0
    assert ray(B=0) == 0 and demap(B=0) == 0
    torch.cuda.synchronize()
    assert bool((x == SENTINEL).all()) and bool((hh == SENTINEL).all()) and bool((l64 == SENTINEL).all())
    # and the accepted forms: NULL bits are the all-zero frame (ld_e unused); a float pointer needs 4-byte alignment
    assert ray(e=None, lde=0) == 0
    assert demap(llr=fp + 4, flags=n.PL_QAM_LLR_F32) == 0
    assert ray(B=1, ldh=Q2) == 0 and demap(B=1, ldh=Q2) == 0  # ld_h = 2 Q exactly
    torch.cuda.synchronize()
    assert bool((e == 0).all()) and bool((x[:, S2:] == SENTINEL).all()) and bool((hh[:, Q2:] == SENTINEL).all())

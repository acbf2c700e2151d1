"""The exact log-MAP demapper on the device (csrc/qam.hip: qam_demap_logmap_kernel) against channel.QAMModem's
host methods, which tests/test_qam_logmap_host.py holds to the definition's loops (tests/qam_logmap_ref.py); through
the device channels; the calibration of the LLRs as probabilities on device noise; the harness chains against the
same chains run stage by stage through the host definition; the CLI; the C-ABI's refusals.  The definition:
include/polarldpc.h at pl_qam_demap_logmap."""
import json
import math

import numpy as np
import pytest
import torch

import qam_fading_ref as F
import qam_ref as Q
from test_gpu_qam import SENTINEL, TT, lengths, only_view_written, view
from test_qam_fading_host import fading_inputs
from test_qam_host import same_bits
from test_qam_logmap_host import AWGN_POINTS, RAYLEIGH_POINTS, SNRS, logmap_inputs, modem, same_up_to_zero_sign

pytestmark = pytest.mark.gpu

MS = Q.MS
FRAME = 2 ** 30


def _native():
    from polarcode_and_ldpc_amd import _native as n
    return n


# ---- equality with the host ----
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("m", MS)
def test_demap_equals_host(gpu, m, dtype):
    for B in (1, 5):
        for E in lengths(m):
            _, y = logmap_inputs(m, E, B)  # levels, ties, zeros, overflowing values, inf and NaN included
            yd = torch.from_numpy(y).cuda()
            for snr in SNRS:
                want = modem(m).demap_host(y, E, snr, dtype=dtype, method="logmap")
                got = modem(m).demap(yd, E, snr, dtype=dtype, method="logmap")
                assert got.dtype == TT[dtype] and same_bits(got.cpu().numpy(), want), (B, E, snr)
            snr = 3.0
            want = modem(m).demap_host(y, E, snr, dtype=dtype, method="logmap")
            assert same_bits(modem(m, "logmap").demap(y, E, snr, dtype=dtype), want)  # NumPy in and out, the modem's own
            # pitched rows on both sides; the output starts 1, 2, 3 elements past a 16-byte boundary
            S2 = y.shape[1]
            _, yv = view(B, S2, S2 + 1, 1, torch.float64)
            yv.copy_(yd)
            for off in range(1, 16 // np.dtype(dtype).itemsize):
                flat, out = view(B, E, E + 3, off, TT[dtype])
                assert modem(m).demap(yv, E, snr, out=out, method="logmap") is out
                assert same_bits(out.cpu().numpy(), want), (B, E, off)
                assert only_view_written(flat, B, E, E + 3, off), (B, E, off)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("m", MS)
def test_demap_csi_equals_host(gpu, m, dtype):
    """the grid of lengths, batches and coherence lengths, the Es/N0 set cycling over it"""
    case = 0
    for B in (1, 5):
        for E in lengths(m):
            S = -(-E // m)
            y = logmap_inputs(m, E, B)[1]
            yd = torch.from_numpy(y).cuda()
            for Lc in sorted({1, 3, S, FRAME}):
                snr = SNRS[case % len(SNRS)]
                case += 1
                _, h = fading_inputs(m, E, B, Lc)  # the coefficient specials on its first entries
                nq = F.blocks(S, Lc)
                want = modem(m).demap_csi_host(y, h, E, snr, coherence=Lc, dtype=dtype, method="logmap")
                hd = torch.from_numpy(h).cuda()
                got = modem(m).demap_csi(yd, hd, E, snr, coherence=Lc, dtype=dtype, method="logmap")
                assert got.dtype == TT[dtype] and same_bits(got.cpu().numpy(), want), (B, E, Lc, snr)
                if Lc == 3:  # NumPy in, NumPy out, the modem's own demapper
                    assert same_bits(modem(m, "logmap").demap_csi(y, h, E, snr, coherence=Lc, dtype=dtype), want)
                # pitched rows on all three sides: y and h one element past a 16-byte boundary, the output 1, 2, 3 past
                _, yv = view(B, 2 * S, 2 * S + 1, 1, torch.float64)
                yv.copy_(yd)
                _, hv = view(B, 2 * nq, 2 * nq + 1, 1, torch.float64)
                hv.copy_(hd)
                for off in range(1, 16 // np.dtype(dtype).itemsize):
                    flat, out = view(B, E, E + 3, off, TT[dtype])
                    assert modem(m).demap_csi(yv, hv, E, snr, coherence=Lc, out=out, method="logmap") is out
                    assert same_bits(out.cpu().numpy(), want), (B, E, Lc, off)
                    assert only_view_written(flat, B, E, E + 3, off), (B, E, Lc, off)
    assert case >= 4 * len(SNRS)


@pytest.mark.parametrize("m", MS)
def test_properties_on_the_device(gpu, m):
    """h = (1.0, 0.0) with finite y: the channel-state kernel equals the AWGN one; the defaults are max-log; QPSK
    equals max-log up to the sign of a zero"""
    E, B = 1027, 5
    y = logmap_inputs(m, E, B)[1]
    yd = torch.from_numpy(np.where(np.isfinite(y), y, 0.25)).cuda()
    h = torch.zeros((B, 2 * modem(m).S(E)), dtype=torch.float64, device="cuda")
    h[:, 0::2] = 1.0
    for dt in (np.float64, np.float32):
        for snr in SNRS:
            lm = modem(m).demap(yd, E, snr, dtype=dt, method="logmap").cpu().numpy()
            assert same_bits(modem(m).demap_csi(yd, h, E, snr, coherence=1, dtype=dt, method="logmap").cpu().numpy(), lm)
            ml = modem(m).demap(yd, E, snr, dtype=dt).cpu().numpy()
            assert same_bits(modem(m).demap(yd, E, snr, dtype=dt, method="maxlog").cpu().numpy(), ml)
            assert same_bits(modem(m, "logmap").demap(yd, E, snr, dtype=dt, method="maxlog").cpu().numpy(), ml)
            assert same_bits(ml, modem(m).demap_host(yd.cpu().numpy(), E, snr, dtype=dt))
            if m == 2:
                assert same_up_to_zero_sign(lm, ml)
            elif snr < 60:
                assert not same_bits(lm, ml)


# ---- through the device channel ----
@pytest.mark.parametrize("m", MS)
def test_through_the_device_channels(gpu, m):
    E, B, seed = 1027, 5, 77
    bits = torch.from_numpy(np.random.default_rng(m).integers(0, 2, (B, E), dtype=np.uint8)).cuda()
    for snr in SNRS:
        y = modem(m).awgn(bits, E, B, snr, seed, 3)
        for dt in (np.float64, np.float32):
            got = modem(m, "logmap").demap(y, E, snr, dtype=dt)
            assert same_bits(got.cpu().numpy(), modem(m).demap_host(y.cpu().numpy(), E, snr, dtype=dt, method="logmap"))
        for Lc in (1, 16, FRAME):
            y, h = modem(m).rayleigh(bits, E, B, snr, seed, coherence=Lc, frame_offset=3)
            for dt in (np.float64, np.float32):
                got = modem(m, "logmap").demap_csi(y, h, E, snr, coherence=Lc, dtype=dt)
                want = modem(m).demap_csi_host(y.cpu().numpy(), h.cpu().numpy(), E, snr, coherence=Lc, dtype=dt,
                                               method="logmap")
                assert same_bits(got.cpu().numpy(), want), (snr, Lc, dt)


# ---- calibration on the device ----
def calibration_device(llr, bits, m):
    """test_qam_logmap_host.calibration on device tensors [B, E]: z of each of the m bit positions of the symbol"""
    E = llr.shape[1]
    pos = torch.arange(E, device=llr.device) % m
    a = llr.abs()
    p = 1.0 / (1.0 + torch.exp(a))
    wrong = ((llr < 0) != (bits != 0)).to(torch.float64)
    z = []
    for i in range(m):
        sel = pos == i
        z.append(float((wrong[:, sel].sum() - p[:, sel].sum()) / torch.sqrt((p[:, sel] * (1.0 - p[:, sel])).sum())))
    return np.array(z)


@pytest.mark.parametrize("m,snr,fading", [(m, s, False) for m, s in AWGN_POINTS] + [(m, s, True) for m, s in RAYLEIGH_POINTS])
def test_calibration(gpu, m, snr, fading):
    """B x E = 2048 x 1024 random device bits through pl_qam_awgn / pl_qam_rayleigh (Lc = 1): the log-MAP LLR
    predicts its own error rate within 5 standard errors at every bit position of the symbol"""
    B, E = 2048, 1024
    gen = torch.Generator(device="cuda").manual_seed(1000 * m + int(snr))
    bits = torch.randint(0, 2, (B, E), dtype=torch.uint8, device="cuda", generator=gen)
    if fading:
        y, h = modem(m).rayleigh(bits, E, B, snr, 31337 + m, coherence=1)
        lm = modem(m).demap_csi(y, h, E, snr, coherence=1, method="logmap")
        ml = modem(m).demap_csi(y, h, E, snr, coherence=1)
    else:
        y = modem(m).awgn(bits, E, B, snr, 31337 + m, 0)
        lm = modem(m).demap(y, E, snr, method="logmap")
        ml = modem(m).demap(y, E, snr)
    z, zm = calibration_device(lm, bits, m), calibration_device(ml, bits, m)
    print("m=%d %s %.0f dB: z logmap %s, maxlog %s" % (m, "Rayleigh" if fading else "AWGN", snr, np.round(z, 2), np.round(zm, 1)))
    assert np.all(np.abs(z) <= 5), z


# ---- the chains ----
def test_polar_chain(gpu):
    import polarcode_and_ldpc_amd.polar as P
    from polarcode_and_ldpc_amd.channel import BitInterleaver
    from polarcode_and_ldpc_amd.harness import montecarlo as MC
    n = _native()
    N, K, E, B, seed = 256, 100, 200, 256, 5
    rm = P.PolarRateMatcher(N, E, "puncture")
    dec = P.SCLDecoder(N, K, list_size=4, frozen_bits=P.construct_rate_matched(K, rm))
    ilv = BitInterleaver("rect", E, rows=6)
    md = modem(6, "logmap")
    f = MC.polar_round_fn(dec, seed=seed, rate_matcher=rm, modulation=md, interleaver=ilv)
    assert f(0, 60.0, 0, B).tolist() == [0, 0, B]
    fr = MC.polar_round_fn(dec, seed=seed, rate_matcher=rm, modulation=md, interleaver=ilv, fading=1)
    assert fr(0, 60.0, 0, B).tolist() == [0, 0, B]
    low = f(1, 2.0, 0, B)
    assert low[2] == B and low[1] > 0
    # the same round stage by stage, the demapper through the host definition on the downloaded symbols
    s = MC._stream_seed(seed, 1)
    msg = torch.empty((B, K), dtype=torch.uint8, device="cuda")
    cw = torch.empty((B, N), dtype=torch.uint8, device="cuda")
    MC._polar_messages(msg, s, 0, K, None)
    n.polar_encode(dec.plan, msg, cw)
    tx = ilv.interleave(rm.select(cw))
    sym = md.awgn(tx, E, B, 2.0, s ^ 0xA5A5A5A5, frame_offset=0)
    rx = torch.from_numpy(md.demap_host(sym.cpu().numpy(), E, 2.0)).cuda()
    llr = torch.empty((B, N), dtype=torch.float64, device="cuda")
    rm.recover(ilv.deinterleave(rx), out=llr)
    out = torch.empty((B, K), dtype=torch.uint8, device="cuda")
    dec.plan.decode(llr, out)
    counts = torch.zeros(3, dtype=torch.int64, device="cuda")
    n.count_errors(msg, out, K, counts)
    assert counts.cpu().numpy().tolist() == low.tolist()
    # and the max-log chain is another chain: the modem's demapper reaches the kernel
    assert MC.polar_round_fn(dec, seed=seed, rate_matcher=rm, modulation=modem(6), interleaver=ilv)(1, 2.0, 0, B).tolist() \
        != low.tolist()


def test_ldpc_chain(gpu):
    import polarcode_and_ldpc_amd.ldpc as L
    from polarcode_and_ldpc_amd.channel import BitInterleaver
    from polarcode_and_ldpc_amd.harness import montecarlo as MC
    n = _native()
    Z, B, seed = 27, 256, 3
    base = L.qc_encodable_base(8, 12, Z, 3, 2, core=4, chained=False)
    enc = L.QCLDPCEncoder(base, Z)
    rm = L.QCRateMatcher(base, Z, 260, punctured=2, fillers=5, start=0)
    E, kf = rm.E, rm.k - rm.fillers
    ilv = BitInterleaver("rect", E, rows=6)
    md = modem(6, "logmap")
    decs = [L.QCLayeredMSDecoder(rm.decoder_base(), Z, max_iter=20, normalization=0.75, early_stop=True, dtype=dt)
            for dt in (np.float64, np.float32)]
    decs.append(L.QCFixedMSDecoder(rm.decoder_base(), Z, max_iter=20, normalization=0.75))
    for dec in decs:
        for fading in (None, 1):
            f = MC.ldpc_round_fn(dec, seed=seed, encoder=enc, rate_matcher=rm, modulation=md, interleaver=ilv, fading=fading)
            assert f(0, 60.0, 0, B).tolist() == [0, 0, B], (dec, fading)
    for dec, dt in ((decs[0], np.float64), (decs[1], np.float32)):
        low = MC.ldpc_round_fn(dec, seed=seed, encoder=enc, rate_matcher=rm, modulation=md, interleaver=ilv)(1, 4.0, 0, B)
        assert low[2] == B and low[1] > 0
        s = MC._stream_seed(seed, 1)
        msg = torch.empty((B, rm.k), dtype=torch.uint8, device="cuda")
        n.random_bits(s, 0, msg)
        msg[:, kf:] = 0
        cw = torch.empty((B, rm.n), dtype=torch.uint8, device="cuda")
        enc.encode_batch_device(msg, out=cw)
        tx = ilv.interleave(rm.select(cw))
        sym = md.awgn(tx, E, B, 4.0, s ^ 0xA5A5A5A5, frame_offset=0)
        rx = torch.from_numpy(md.demap_host(sym.cpu().numpy(), E, 4.0, dtype=dt)).cuda()
        llr = torch.empty((B, rm.n_dec), dtype=TT[dt], device="cuda")
        rm.recover(ilv.deinterleave(rx), out=llr)
        out = torch.empty((B, rm.n_dec), dtype=torch.uint8, device="cuda")
        its = torch.empty((B,), dtype=torch.int32, device="cuda")
        dec.plan.decode(llr, out, its)
        counts = torch.zeros(3, dtype=torch.int64, device="cuda")
        n.count_errors(msg, out, kf, counts)
        assert counts.cpu().numpy().tolist() == low.tolist(), dt


# ---- simulate_* and the CLI ----
def test_simulate_and_cli(gpu, capsys, tmp_path):
    import polarcode_and_ldpc_amd.ldpc as L
    from polarcode_and_ldpc_amd.harness import ber
    cfg = {"encoding": {"N": 256, "K": 100}}
    log = tmp_path / "polar.jsonl"
    b, f, pts = ber.simulate_polar([60.0], 256, 100, cfg, list_size=4, batch=256, rate_match=dict(E=200, mode="puncture"),
                                   modulation=modem(6, "logmap"), log_path=str(log))
    assert pts[0].frames == 256 and pts[0].frame_errors == 0
    assert json.loads(log.read_text().splitlines()[0])["key"]["demapper"] == "logmap"
    base = L.qc_encodable_base(8, 12, 27, 3, 2, core=4, chained=False)
    log2 = tmp_path / "qc.jsonl"
    b, f, pts = ber.simulate_qc_ldpc([60.0], 256, 100, base, 27, batch=256, random_codewords=True,
                                     rate_match=(260, 2, 5), modulation=modem(6, "logmap"), dtype=np.float32, fading=4,
                                     log_path=str(log2))
    assert pts[0].frames == 256 and pts[0].frame_errors == 0
    assert json.loads(log2.read_text().splitlines()[0])["key"]["demapper"] == "logmap"
    log3 = tmp_path / "plain.jsonl"
    ber.simulate_polar([30.0], 256, 100, cfg, list_size=4, batch=256, modulation=modem(6), log_path=str(log3))
    assert "demapper" not in log3.read_text()
    # the command line, the same command three ways at a point where frames fail
    common = ["--code", "polar", "--N", "256", "--K", "100", "--list-size", "4", "--polar-rm", "200,puncture",
              "--modulation", "64qam", "--snr=8:8:1", "--frames", "256", "--batch", "256"]
    runs = {}
    for name, extra in (("logmap", ["--demapper", "logmap"]), ("maxlog", ["--demapper", "maxlog"]), ("none", [])):
        path = tmp_path / ("cli_%s.jsonl" % name)
        ber.main(common + extra + ["--log", str(path)])
        res = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
        assert res["points"][0]["frames"] == 256
        runs[name] = (json.loads(path.read_text().splitlines()[0])["key"], res["points"])
    assert runs["logmap"][0].get("demapper") == "logmap"
    assert "demapper" not in runs["none"][0] and runs["maxlog"] == runs["none"]
    key = dict(runs["logmap"][0])
    del key["demapper"]
    assert key == runs["none"][0] and runs["logmap"][1] != runs["none"][1]
    with pytest.raises(SystemExit):
        ber.main(common[:10] + common[12:] + ["--demapper", "logmap"])  # without --modulation
    capsys.readouterr()


# ---- the C-ABI ----
def test_capi_refusals(gpu):
    n = _native()
    lib, EINVAL = n.lib, n.PL_EINVAL
    m, E, B, Lc = 4, 10, 2, 2
    S2, Q2 = 6, 4
    x = torch.full((B, S2 + 2), SENTINEL, dtype=torch.float64, device="cuda")
    hh = torch.full((B, Q2 + 2), SENTINEL, dtype=torch.float64, device="cuda")
    l64 = torch.full((B, E + 2), SENTINEL, dtype=torch.float64, device="cuda")
    l32 = torch.full((B, E + 2), SENTINEL, dtype=torch.float32, device="cuda")
    xp, hp, lp, fp = x.data_ptr(), hh.data_ptr(), l64.data_ptr(), l32.data_ptr()
    st = n._stream()

    def demap(m=m, E=E, Lc=None, B=B, y=xp, ldy=S2 + 2, h=None, ldh=None, snr=3.0, llr=lp, ldl=E + 2, flags=0):
        return lib.pl_qam_demap_logmap(m, E, B, y, ldy, snr, llr, ldl, flags, st)

    def csi(m=m, E=E, Lc=Lc, B=B, y=xp, ldy=S2 + 2, h=hp, ldh=Q2 + 2, snr=3.0, llr=lp, ldl=E + 2, flags=0):
        return lib.pl_qam_demap_csi_logmap(m, E, Lc, B, y, ldy, h, ldh, snr, llr, ldl, flags, st)

    def refused(rc, word):
        msg = (lib.pl_last_error() or b"").decode()
        assert rc == EINVAL and word in msg, (rc, msg, word)

    for fn in (demap, csi):
        refused(fn(m=3), "m = 3")
        refused(fn(m=0), "m = 0")
        refused(fn(E=0), "E = 0")
        refused(fn(E=(1 << 30) + 1), "E = ")
        refused(fn(B=-1), "batch")
        refused(fn(y=None), "NULL")
        refused(fn(llr=None), "NULL")
        refused(fn(y=xp + 4), "aligned")
        refused(fn(llr=lp + 4), "aligned")
        refused(fn(llr=fp + 2, flags=n.PL_QAM_LLR_F32), "aligned")
        refused(fn(ldy=S2 - 1), "ld_y")
        refused(fn(ldl=E - 1), "ld_llr")
        refused(fn(flags=2), "flag")
        refused(fn(flags=-1), "flag")
        for bad in (math.nan, math.inf, -math.inf):
            refused(fn(snr=bad), "snr_db")
    refused(csi(Lc=0), "coherence = 0")
    refused(csi(Lc=(1 << 30) + 1), "coherence = %d" % ((1 << 30) + 1))
    refused(csi(m=3, Lc=0), "m = 3")  # the conditions' order
    refused(csi(h=None), "h_dev")
    refused(csi(h=hp + 4), "aligned")
    refused(csi(ldh=Q2 - 1), "ld_h")
    torch.cuda.synchronize()
    assert bool((l64 == SENTINEL).all()) and bool((l32 == SENTINEL).all())  # nothing was launched by a refused call
    # batch == 0 launches nothing, whatever the pointers (NULL, or poisoned ones that no kernel may touch)
    poison = 0xDEAD0000
    assert demap(B=0, y=None, llr=None) == 0 and csi(B=0, y=None, h=None, llr=None) == 0
    assert demap(B=0, y=poison, llr=poison) == 0 and csi(B=0, y=poison, h=poison, llr=poison) == 0
    assert demap(B=0) == 0 and csi(B=0) == 0
    torch.cuda.synchronize()
    assert bool((l64 == SENTINEL).all())
    # and the accepted forms: a float pointer needs 4-byte alignment only; ld_h = 2 Q exactly
    x.zero_()
    hh.fill_(1.0)
    assert demap(llr=fp + 4, flags=n.PL_QAM_LLR_F32) == 0 and csi(llr=fp + 4, flags=n.PL_QAM_LLR_F32) == 0
    assert demap() == 0 and csi(B=1, ldh=Q2) == 0
    torch.cuda.synchronize()
    assert bool((l64[:, E:] == SENTINEL).all()) and bool((l64[:, :E] != SENTINEL).all())

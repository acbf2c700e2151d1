"""PolarRateMatcher on the device (polar_ratematch.hip) against its host reference,
the selection written out in NumPy (tests/test_polar_ratematch_host.py pins that
one).  Bars: select array_equal; recover bit-equal, compared as integers.

The shared case set at batches 1 and 67 with fp64 and fp32 LLRs; then both store
paths on row-pitched views, two streams, the empty batch, special values,
accumulation over two matchers, the identity matcher, shortening end to end,
noise-free round trips through SC and SCL, the decoders on recovered LLRs against
the C oracle, the harness, and the C-ABI's refusals."""
import ctypes
import functools
import json

import numpy as np
import pytest
import torch

from test_polar_ratematch_host import CASES, IDS, MODES, SHUFFLE32, lengths, matcher

pytestmark = pytest.mark.gpu

B = 67
TT = {np.float64: torch.float64, np.float32: torch.float32}


def _P():
    import polarcode_and_ldpc_amd.polar as P
    return P


def _N():
    from polarcode_and_ldpc_amd import _native
    return _native


def bits_equal(got, want):
    """bit-equal float64 arrays (the integer views are compared: NaN payloads and zero signs count)"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype == np.float64 and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    return np.array_equal(got.view(np.uint64), want.view(np.uint64))


@functools.lru_cache(maxsize=None)
def frames(N, E):
    """(codeword bytes [B, N], any byte value; LLRs float64 [B, E])"""
    rs = np.random.RandomState(7 * N + E)
    cw = rs.randint(0, 256, (B, N)).astype(np.uint8)
    llr = rs.standard_normal((B, E)) * 4.0
    cw.setflags(write=False)
    llr.setflags(write=False)
    return cw, llr


@pytest.mark.parametrize("N,nsub,name", CASES, ids=IDS)
def test_select_equals_host(gpu, N, nsub, name):
    for mode in MODES:
        for E in lengths(N):
            rm = matcher(N, nsub, name, mode, E)
            cw, _ = frames(N, E)
            want = rm.select_host(cw)
            dev = torch.from_numpy(cw.copy()).cuda()
            for b in (1, B):
                got = rm.select(dev[:b])
                assert got.is_cuda and got.dtype == torch.uint8 and got.shape == (b, E)
                assert np.array_equal(got.cpu().numpy(), want[:b]), (mode, E, b)
            assert np.array_equal(rm.select(cw[:5]), want[:5])  # NumPy in, NumPy out


@pytest.mark.parametrize("N,nsub,name", CASES, ids=IDS)
def test_recover_equals_host(gpu, N, nsub, name):
    for mode in MODES:
        for E in lengths(N):
            rm = matcher(N, nsub, name, mode, E)
            _, llr64 = frames(N, E)
            for tin in (np.float64, np.float32):
                llr = llr64.astype(tin)
                want = rm.recover_host(llr)
                dev = torch.from_numpy(llr).cuda()
                for b in (1, B):
                    got = rm.recover(dev[:b])
                    assert got.is_cuda and got.dtype == torch.float64 and got.shape == (b, N)
                    assert bits_equal(got.cpu().numpy(), want[:b]), (mode, E, tin, b)
            got = rm.recover(llr64[:5].astype(np.float32))  # NumPy in, NumPy out
            assert isinstance(got, np.ndarray) and bits_equal(got, rm.recover_host(llr64[:5].astype(np.float32)))
            mine = np.full((5, N), -3.0)
            assert rm.recover(llr64[:5], out=mine) is mine and bits_equal(mine, rm.recover_host(llr64[:5]))


def _pitched(rows, off, ld, fill, dtype):
    """(buffer, view [rows, ld] of it `off` elements behind a 16-byte boundary)"""
    buf = torch.full((off + rows * ld + 32,), fill, dtype=dtype, device="cuda")
    assert buf.data_ptr() % 16 == 0
    return buf, buf[off:off + rows * ld].view(rows, ld)


@pytest.mark.parametrize("N,nsub,name", [(64, 32, "shuf"), (1024, 32, "shuf"), (64, 1, "id")])
@pytest.mark.parametrize("off", [0, 1, 3, 8, 15])
def test_pitched_views_on_both_store_paths(gpu, N, nsub, name, off):
    """Outputs `off` bytes (select) or elements (recover) behind a 16-byte boundary.  off = 0 with a pitch
    that keeps rows on boundaries: 16-byte stores and a cut last piece only; otherwise an odd pitch, so the
    head piece differs from row to row and element stores run at both row ends.  The inputs always sit at
    an odd offset and pitch.  Beyond E and N nothing changes."""
    for mode in MODES:
        for E in (N // 2 + 1, 2 * N + 5):
            rm = matcher(N, nsub, name, mode, E)
            cw, llr64 = frames(N, E)
            # select
            _, cv = _pitched(B, 3, N + 5, 0x5B, torch.uint8)
            cv[:, :N] = torch.from_numpy(cw.copy()).cuda()
            ld = (E + 15) // 16 * 16 + 16 if off == 0 else E + 3 + E % 2
            ebuf, ev = _pitched(B, off, ld, 0xAA, torch.uint8)
            out = ev[:, :E]
            assert out.data_ptr() % 16 == off and cv.data_ptr() % 2 == 1
            assert rm.select(cv[:, :N], out=out) is out
            assert np.array_equal(out.cpu().numpy(), rm.select_host(cw)), (mode, E)
            flat = ebuf.cpu().numpy()
            assert (flat[:off] == 0xAA).all() and (flat[off + B * ld:] == 0xAA).all()
            assert (flat[off:off + B * ld].reshape(B, ld)[:, E:] == 0xAA).all()
            # recover, both input types, fresh and accumulating
            for tin in (np.float64, np.float32):
                llr = llr64.astype(tin)
                _, lv = _pitched(B, 1, E + 3 + E % 2, 7.0, TT[tin])
                lv[:, :E] = torch.from_numpy(llr).cuda()
                ld = N + 2 if off == 0 else N + 3
                obuf, ov = _pitched(B, off, ld, -5.0, torch.float64)
                out = ov[:, :N]
                assert out.data_ptr() % 16 == (8 * off) % 16
                want = rm.recover_host(llr)
                assert rm.recover(lv[:, :E], out=out) is out
                assert bits_equal(out.cpu().numpy(), want), (mode, E, tin)
                rm.recover(lv[:, :E], out=out, accumulate=True)
                assert bits_equal(out.cpu().numpy(), rm.recover_host(llr, out=want, accumulate=True)), (mode, E, tin)
                flat = obuf.cpu().numpy()
                assert (flat[:off] == -5.0).all() and (flat[off + B * ld:] == -5.0).all()
                assert (flat[off:off + B * ld].reshape(B, ld)[:, N:] == -5.0).all()
                assert (lv.cpu().numpy()[:, E:] == 7.0).all()


def test_two_streams_and_empty_batch(gpu):
    rm = matcher(1024, 32, "shuf", "shorten", 2 * 1024 + 5)
    N, E = rm.N, rm.E
    cw, llr = frames(N, E)
    c, l = torch.from_numpy(cw.copy()).cuda(), torch.from_numpy(llr.copy()).cuda()
    e0, r0 = rm.select(c), rm.recover(l)
    torch.cuda.synchronize()
    outs = []
    for s in (torch.cuda.Stream(), torch.cuda.Stream()):
        with torch.cuda.stream(s):
            outs.append((rm.select(c), rm.recover(l)))
    torch.cuda.synchronize()
    for e, r in outs:
        assert torch.equal(e, e0) and bits_equal(r.cpu().numpy(), r0.cpu().numpy())
    assert np.array_equal(e0.cpu().numpy(), rm.select_host(cw)) and bits_equal(r0.cpu().numpy(), rm.recover_host(llr))
    # B = 0: shapes and types, nothing launched
    e = rm.select(c[:0])
    assert e.shape == (0, E) and e.dtype == torch.uint8 and e.is_cuda
    r = rm.recover(l[:0].to(torch.float32))
    assert r.shape == (0, N) and r.dtype == torch.float64 and r.is_cuda
    assert rm.select(np.zeros((0, N), np.uint8)).shape == (0, E)
    lib = _N().lib
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    keep_r, keep_e = r0.clone(), e0.clone()
    assert lib.pl_polar_rate_recover(ctypes.byref(rm.rm), l.data_ptr(), E, 0, r0.data_ptr(), N, 1024.0, 0, st) == 0
    assert lib.pl_polar_rate_match(ctypes.byref(rm.rm), c.data_ptr(), N, 0, e0.data_ptr(), E, st) == 0
    torch.cuda.synchronize()
    assert torch.equal(r0, keep_r) and torch.equal(e0, keep_e)


def test_special_values(gpu):
    """+-inf and -0.0 anywhere, the infinities of one position of one sign (no inf - inf); NaNs with payloads
    in fp64 where a position has a single term, so that no addition and no conversion touches them: they
    are copied bit for bit."""
    nan_seen = False
    for mode, E in (("puncture", 45), ("shorten", 45), ("puncture", 64), ("shorten", 64 + 64 + 5)):
        rm = matcher(64, 32, "shuf", mode, E)
        pos = rm.positions_host()
        rs = np.random.RandomState(E + len(mode))
        llr = rs.standard_normal((B, E)) * 4
        kind = rs.randint(0, 6, (B, E))
        llr[kind == 0] = -0.0
        llr[kind == 1] = 0.0
        llr = np.where(kind == 2, np.where(pos % 2 == 0, np.inf, -np.inf)[None, :], llr)
        single = (np.bincount(pos, minlength=64)[pos] == 1)[None, :] & (kind == 3)
        for tin in (np.float64, np.float32):
            x = llr.astype(tin)
            if tin == np.float64 and single.any():
                u = x.view(np.uint64)
                pay = rs.randint(1, 1 << 20, x.shape).astype(np.uint64)
                sign = rs.randint(0, 2, x.shape).astype(np.uint64) << np.uint64(63)
                u[single] = (np.uint64(0x7FF8000000000000) | pay | sign)[single]
                assert np.isnan(x[single]).all()
                nan_seen = True
            want = rm.recover_host(x)
            got = rm.recover(torch.from_numpy(x).cuda()).cpu().numpy()
            assert bits_equal(got, want), (mode, E, tin)
            assert np.isinf(want).any() and (np.signbit(want) & (want == 0)).any()
            assert np.isnan(want).any() == bool(tin == np.float64 and single.any())
    assert nan_seen


@pytest.mark.parametrize("tin", [np.float64, np.float32])
def test_accumulate_over_two_matchers(gpu, tin):
    """Chase combining: a punctured first transmission, then a repeated one through another permutation;
    what the first did not send starts from +0.0."""
    N = 64
    m1 = matcher(N, 32, "shuf", "puncture", N - 19)
    m2 = matcher(N, 32, "rev", "puncture", 2 * N + 5)
    rs = np.random.RandomState(11)
    l1 = (rs.standard_normal((B, m1.E)) * 4).astype(tin)
    l2 = (rs.standard_normal((B, m2.E)) * 4).astype(tin)
    h1 = m1.recover_host(l1)
    h2 = m2.recover_host(l2, out=h1, accumulate=True)
    assert (h1[:, m1.untransmitted] == 0).all() and not bits_equal(h1, h2)
    for b in (1, B):
        out = m1.recover(torch.from_numpy(l1[:b]).cuda())
        assert bits_equal(out.cpu().numpy(), h1[:b])
        got = m2.recover(torch.from_numpy(l2[:b]).cuda(), out=out, accumulate=True)
        assert got is out and bits_equal(out.cpu().numpy(), h2[:b]), b
    # a shortened second transmission leaves what it does not send as it is
    m3 = matcher(N, 32, "shuf", "shorten", N - 19)
    l3 = (rs.standard_normal((B, m3.E)) * 4).astype(tin)
    h3 = m3.recover_host(l3, out=h2, accumulate=True)
    assert np.array_equal(h3[:, m3.untransmitted], h2[:, m3.untransmitted])
    out = torch.from_numpy(h2.copy()).cuda()
    m3.recover(torch.from_numpy(l3).cuda(), out=out, accumulate=True)
    assert bits_equal(out.cpu().numpy(), h3)
    with pytest.raises(AssertionError):
        m2.recover(torch.from_numpy(l2).cuda(), accumulate=True)  # nothing to accumulate into


@pytest.mark.parametrize("N", [2, 64, 1024])
def test_identity_matcher_copies(gpu, N):
    """E = N, nsub = 1: select is a byte copy, recover a bit copy (fp32 widened)."""
    for mode in MODES:
        rm = matcher(N, 1, "id", mode, N)
        cw, llr = frames(N, N)
        c = torch.from_numpy(cw.copy()).cuda()
        assert torch.equal(rm.select(c), c)
        assert bits_equal(rm.recover(torch.from_numpy(llr.copy()).cuda()).cpu().numpy(), llr)
        f = llr.astype(np.float32)
        assert bits_equal(rm.recover(torch.from_numpy(f).cuda()).cpu().numpy(), f.astype(np.float64))


def _encode(dec, msg):
    cw = torch.empty((msg.shape[0], dec.N), dtype=torch.uint8, device="cuda")
    _N().polar_encode(dec.plan, msg, cw)
    return cw


@pytest.mark.parametrize("N,nsub,name", [(64, 32, "shuf"), (64, 1, "id"), (1024, 32, "shuf")])
def test_shortened_codewords_are_zero_where_not_sent(gpu, N, nsub, name):
    P = _P()
    for E in (N - 19, N - 1):
        rm = matcher(N, nsub, name, "shorten", E)
        K = E // 2
        frozen = P.construct_rate_matched(K, rm)
        rm.check_frozen(frozen)
        dec = P.SCDecoder(N, K, frozen_bits=frozen)
        msg = torch.from_numpy(np.random.RandomState(E).randint(0, 2, (B, K)).astype(np.uint8)).cuda()
        cw = _encode(dec, msg).cpu().numpy()
        assert cw.any() and not cw[:, rm.untransmitted].any()
        # the same K on the mother code's own frozen set does leave ones there
        plain = P.SCDecoder(N, K, frozen_bits=P.construct_frozen_set(N, K))
        assert _encode(plain, msg).cpu().numpy()[:, rm.untransmitted].any()
        with pytest.raises(AssertionError, match="shortening forces"):
            rm.check_frozen(plain.frozen_bits)


@pytest.mark.parametrize("N", [64, 256])
@pytest.mark.parametrize("mode", MODES)
def test_noise_free_round_trip(gpu, N, mode):
    P = _P()
    for E in (N - 19, N + 7):
        rm = P.PolarRateMatcher(N, E, mode, SHUFFLE32)
        K = E // 2
        frozen = P.construct_rate_matched(K, rm)
        msg = np.random.RandomState(N + E).randint(0, 2, (B, K)).astype(np.uint8)
        for dec in (P.SCDecoder(N, K, frozen_bits=frozen), P.SCLDecoder(N, K, list_size=4, frozen_bits=frozen)):
            tx = rm.select(_encode(dec, torch.from_numpy(msg).cuda()))
            llr = rm.recover(8.0 * (1.0 - 2.0 * tx.to(torch.float64)))
            got = dec.decode_batch(llr).cpu().numpy()
            assert np.array_equal(got, msg), (E, dec)


@pytest.mark.parametrize("mode", MODES)
def test_decoders_on_recovered_llrs_equal_the_oracle(gpu, oracle, mode):
    """N = 256, E = 192, K = 96 at 1 dB, 64 frames: a quarter of the decoder inputs are exactly 0.0
    (puncture) or 1024.0 (shorten).  SC and SCL L = 8 must give the C oracle's bits on these LLRs."""
    from polarcode_and_ldpc_amd.channel.awgn import AWGNChannel
    P = _P()
    N, E, K, F = 256, 192, 96, 64
    rm = P.PolarRateMatcher(N, E, mode, SHUFFLE32)
    frozen = P.construct_rate_matched(K, rm)
    sc = P.SCDecoder(N, K, frozen_bits=frozen)
    scl = P.SCLDecoder(N, K, list_size=8, frozen_bits=frozen)
    msg = torch.from_numpy(np.random.RandomState(1).randint(0, 2, (F, K)).astype(np.uint8)).cuda()
    tx = rm.select(_encode(sc, msg))
    rx = AWGNChannel(1.0).llr_batch_device(tx, E, F, seed=9, frame_offset=0)
    llr = rm.recover(rx)
    host = llr.cpu().numpy()
    fill = 0.0 if mode == "puncture" else 1024.0
    assert (host[:, rm.untransmitted] == fill).all() and len(rm.untransmitted) == N - E
    assert bits_equal(host, rm.recover_host(rx.cpu().numpy()))
    got_sc = sc.decode_batch(llr).cpu().numpy()
    assert np.array_equal(got_sc, oracle.sc_decode(N, frozen, host, threads=4))
    got_scl = scl.decode_batch(llr).cpu().numpy()
    assert np.array_equal(got_scl, oracle.scl_decode(N, 8, frozen, host, threads=4))


def test_harness_round_fn(gpu):
    from polarcode_and_ldpc_amd.harness.montecarlo import polar_round_fn
    P = _P()
    N, K = 128, 64
    dec = P.SCDecoder(N, K, frozen_bits=P.construct_frozen_set(N, K))
    ident = P.PolarRateMatcher(N, N)
    a = polar_round_fn(dec, seed=5)(1, 1.0, 0, 256)
    b = polar_round_fn(dec, seed=5, rate_matcher=ident)(1, 1.0, 0, 256)
    assert a.tolist() == b.tolist() and a[2] == 256
    a, b = polar_round_fn(dec, seed=5)(1, -2.0, 0, 256), polar_round_fn(dec, seed=5, rate_matcher=ident)(1, -2.0, 0, 256)
    assert a.tolist() == b.tolist() and a[1] > 0  # frames do fail there: the counters are not trivially 0
    crc = P.CASCLDecoder(N, K, 4, frozen_bits=P.construct_frozen_set(N, K), crc_polynomial="CRC-8")
    assert polar_round_fn(crc, seed=5, crc_polynomial="CRC-8")(0, 1.0, 0, 256).tolist() == \
        polar_round_fn(crc, seed=5, crc_polynomial="CRC-8", rate_matcher=ident)(0, 1.0, 0, 256).tolist()
    # counts belong to the frames, not to the calls
    rm = P.PolarRateMatcher(N, 100, "puncture", SHUFFLE32)
    pdec = P.SCDecoder(N, 50, frozen_bits=P.construct_rate_matched(50, rm))
    f = polar_round_fn(pdec, seed=3, rate_matcher=rm)
    whole = f(1, 1.0, 0, 256)
    assert whole[2] == 256 and whole[0] >= whole[1]
    assert (f(1, 1.0, 0, 128) + f(1, 1.0, 128, 128)).tolist() == whole.tolist()
    low = f(1, -2.0, 0, 256)
    assert low[1] > 0 and (f(1, -2.0, 0, 128) + f(1, -2.0, 128, 128)).tolist() == low.tolist()  # frames do fail there
    assert f(0, 12.0, 0, 256).tolist() == [0, 0, 256]
    # the wrong mother code, and a frozen set that does not shorten
    with pytest.raises(AssertionError, match="mother code"):
        polar_round_fn(dec, rate_matcher=P.PolarRateMatcher(64, 50))
    with pytest.raises(AssertionError, match="shortening forces"):
        polar_round_fn(dec, rate_matcher=P.PolarRateMatcher(N, 100, "shorten"))


def test_simulate_polar_rate_matched_and_cli(gpu, tmp_path, capsys):
    from polarcode_and_ldpc_amd.harness import ber
    snr, nfr = [-2.0, 3.0], 512
    cfg = {"encoding": {"N": 128, "K": 50}}
    rmargs = dict(E=100, mode="shorten", sub_blocks=SHUFFLE32)
    log = tmp_path / "points.jsonl"
    kw = dict(list_size=4, batch=256, seed=0)
    _, _, pts = ber.simulate_polar(snr, nfr, 10 ** 9, cfg, log_path=str(log), rate_match=rmargs, **kw)
    assert [p.frames for p in pts] == [nfr] * 2 and [p.info_bits for p in pts] == [50] * 2
    assert pts[0].frame_errors > pts[1].frame_errors >= 0
    rows = [json.loads(l) for l in log.read_text().splitlines() if l.strip()]
    assert len(rows) == 2
    assert all(r["key"]["E"] == 100 and r["key"]["mode"] == "shorten" and r["key"]["perm"] == SHUFFLE32 for r in rows)
    size = log.stat().st_size
    _, _, again = ber.simulate_polar(snr, nfr, 10 ** 9, cfg, log_path=str(log), rate_match=rmargs, **kw)
    assert [(p.frame_errors, p.bit_errors) for p in again] == [(p.frame_errors, p.bit_errors) for p in pts]
    assert log.stat().st_size == size  # resumed: both points came from the log
    # another mode is another run key; a given frozen set is used as it is
    import polarcode_and_ldpc_amd.polar as P
    fr = P.construct_rate_matched(50, P.PolarRateMatcher(128, 100, "puncture", SHUFFLE32))
    _, _, other = ber.simulate_polar(snr, nfr, 10 ** 9, dict(cfg, frozen_bits=fr), log_path=str(log),
                                     rate_match=dict(rmargs, mode="puncture"), **kw)
    assert log.stat().st_size > size and [p.frames for p in other] == [nfr] * 2
    # without rate matching the key is what it was: no E, mode or perm
    plain = tmp_path / "plain.jsonl"
    ber.simulate_polar([3.0], 256, 10 ** 9, cfg, log_path=str(plain), **kw)
    key = json.loads(plain.read_text().splitlines()[0])["key"]
    assert not {"E", "mode", "perm", "known_llr"} & set(key)
    # the command line, with a log and a resume from it
    clog = tmp_path / "cli.jsonl"
    argv = ["--code", "polar", "--N", "128", "--K", "50", "--list-size", "4", "--polar-rm",
            "100,shorten," + ",".join(str(p) for p in SHUFFLE32), "--snr=-2:3:5", "--frames", str(nfr),
            "--max-errors", str(10 ** 9), "--batch", "256", "--log", str(clog)]
    for turn in range(2):
        capsys.readouterr()
        ber.main(argv)
        out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
        assert out["code"] == "polar" and out["snr_db"] == snr
        assert [(p["frame_errors"], p["bit_errors"]) for p in out["points"]] == \
            [(p.frame_errors, p.bit_errors) for p in pts]
        csize = clog.stat().st_size if turn == 0 else csize
        assert clog.stat().st_size == csize
    with pytest.raises(SystemExit):
        ber.main(["--code", "polar", "--polar-rm", "100,repeat"])


def test_capi_refusals(gpu):
    """Every refusal comes before the first device call: nothing is written."""
    N_ = _N()
    rm = matcher(64, 32, "shuf", "shorten", 45)
    N, E, b = rm.N, rm.E, 5
    cw, llr = frames(N, E)
    c = torch.from_numpy(cw[:b].copy()).cuda()
    l = torch.from_numpy(llr[:b].copy()).cuda()
    e = torch.full((b, E), 0xAA, dtype=torch.uint8, device="cuda")
    o = torch.full((b, N + 1), -5.0, dtype=torch.float64, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    R = ctypes.byref(rm.rm)
    bad = N_.PolarRateMatch(64, 45, 1, 4, (ctypes.c_uint8 * 32)(0, 1, 1, 2))  # no permutation
    sel, rec = N_.lib.pl_polar_rate_match, N_.lib.pl_polar_rate_recover
    P_ = lambda t: t.data_ptr()  # noqa: E731
    ld = N + 1
    calls = {
        "rm NULL": lambda: sel(None, P_(c), N, b, P_(e), E, st),
        "rm refused": lambda: sel(ctypes.byref(bad), P_(c), N, b, P_(e), E, st),
        "cw NULL": lambda: sel(R, None, N, b, P_(e), E, st),
        "e NULL": lambda: sel(R, P_(c), N, b, None, E, st),
        "batch < 0": lambda: sel(R, P_(c), N, -1, P_(e), E, st),
        "ld_cw < N": lambda: sel(R, P_(c), N - 1, b, P_(e), E, st),
        "ld_e < E": lambda: sel(R, P_(c), N, b, P_(e), E - 1, st),
        "recover rm NULL": lambda: rec(None, P_(l), E, b, P_(o), ld, 1024.0, 0, st),
        "recover rm refused": lambda: rec(ctypes.byref(bad), P_(l), E, b, P_(o), ld, 1024.0, 0, st),
        "llr NULL": lambda: rec(R, None, E, b, P_(o), ld, 1024.0, 0, st),
        "out NULL": lambda: rec(R, P_(l), E, b, None, ld, 1024.0, 0, st),
        "recover batch < 0": lambda: rec(R, P_(l), E, -1, P_(o), ld, 1024.0, 0, st),
        "ld_llr < E": lambda: rec(R, P_(l), E - 1, b, P_(o), ld, 1024.0, 0, st),
        "ld_out < N": lambda: rec(R, P_(l), E, b, P_(o), N - 1, 1024.0, 0, st),
        "flags 2": lambda: rec(R, P_(l), E, b, P_(o), ld, 1024.0, 2, st),
        "flags 8": lambda: rec(R, P_(l), E, b, P_(o), ld, 1024.0, 8, st),
        "out misaligned": lambda: rec(R, P_(l), E, b, P_(o) + 4, ld, 1024.0, 0, st),
        "llr misaligned": lambda: rec(R, P_(l) + 4, E, b, P_(o), ld, 1024.0, 0, st),
        "llr f32 misaligned": lambda: rec(R, P_(l) + 2, E, b, P_(o), ld, 1024.0, N_.PL_PRM_LLR_F32, st),
        "known 0": lambda: rec(R, P_(l), E, b, P_(o), ld, 0.0, 0, st),
        "known < 0": lambda: rec(R, P_(l), E, b, P_(o), ld, -1024.0, 0, st),
        "known inf": lambda: rec(R, P_(l), E, b, P_(o), ld, float("inf"), 0, st),
        "known nan": lambda: rec(R, P_(l), E, b, P_(o), ld, float("nan"), 0, st),
    }
    for name, call in calls.items():
        assert call() == N_.PL_EINVAL and N_.lib.pl_last_error(), name
    assert b"known_llr" in (calls["known nan"](), N_.lib.pl_last_error())[1]
    assert b"no permutation" in (calls["rm refused"](), N_.lib.pl_last_error())[1]
    torch.cuda.synchronize()
    assert (e == 0xAA).all() and (o == -5.0).all()  # nothing was launched
    # the derived fields a caller leaves in the struct are not trusted
    junk = N_.PolarRateMatch(64, 45, 1, 32, (ctypes.c_uint8 * 32)(*SHUFFLE32), 7, 7, 7, 7, (ctypes.c_uint8 * 32)(*[3] * 32))
    assert sel(ctypes.byref(junk), P_(c), N, b, P_(e), E, st) == 0
    assert rec(ctypes.byref(junk), P_(l), E, b, P_(o), ld, 1024.0, 0, st) == 0
    torch.cuda.synchronize()
    assert np.array_equal(e.cpu().numpy(), rm.select_host(cw[:b]))
    got = o.cpu().numpy()
    assert bits_equal(got[:, :N], rm.recover_host(llr[:b])) and (got[:, N:] == -5.0).all()
    with pytest.raises(AssertionError):
        rm.select(c[:, :-1])
    with pytest.raises(AssertionError):
        rm.recover(l[:, :-1])

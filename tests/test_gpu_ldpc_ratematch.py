"""QCRateMatcher on the device (ldpc_qc_ratematch.hip) against its host reference,
the selection loop written out in NumPy (tests/test_ldpc_ratematch_host.py pins
that one).  Bars: select array_equal; recover bit-equal, compared as integers.

The configurations are the host test's, at batches 1 and 67, with all four
LLR / output type pairs; then accumulation over two matchers, row-pitched views
on both store paths, two streams, the empty batch, special values, the identity
matcher, a noise-free round trip through encoder and decoder, the harness and
the C-ABI's refusals."""
import ctypes
import functools
import json

import numpy as np
import pytest
import torch

from test_ldpc_ratematch_host import CASES, IDS, MB, NB, base_of, configs, matcher

pytestmark = pytest.mark.gpu

B = 67
PAIRS = [(np.float64, np.float64), (np.float64, np.float32), (np.float32, np.float64), (np.float32, np.float32)]
TT = {np.float64: torch.float64, np.float32: torch.float32}
UI = {np.float64: np.uint64, np.float32: np.uint32}


def _L():
    import polarcode_and_ldpc_amd.ldpc as L
    return L


def _N():
    from polarcode_and_ldpc_amd import _native
    return _native


def bits_equal(got, want):
    """bit-equal float arrays of one type (the integer views are compared: NaN payloads and zero signs count)"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    u = UI[got.dtype.type]
    return np.array_equal(got.view(u), want.view(u))


@functools.lru_cache(maxsize=None)
def frames(Z, name):
    """(codeword bytes [B, n], any byte value; LLRs float64 [B, E]) of a configuration"""
    rm = matcher(Z, name)
    rs = np.random.RandomState(1000 * Z + len(name))
    cw = rs.randint(0, 256, (B, rm.n)).astype(np.uint8)
    llr = rs.standard_normal((B, rm.E)) * 4.0
    cw.setflags(write=False)
    llr.setflags(write=False)
    return cw, llr


@pytest.mark.parametrize("Z,name", CASES, ids=IDS)
def test_select_equals_host(gpu, Z, name):
    rm = matcher(Z, name)
    cw, _ = frames(Z, name)
    want = rm.select_host(cw)
    dev = torch.from_numpy(cw.copy()).cuda()
    for b in (1, B):
        got = rm.select(dev[:b])
        assert got.is_cuda and got.dtype == torch.uint8 and got.shape == (b, rm.E)
        assert np.array_equal(got.cpu().numpy(), want[:b]), b
    assert np.array_equal(rm.select(cw[:5]), want[:5])  # NumPy in, NumPy out


@pytest.mark.parametrize("Z,name", CASES, ids=IDS)
def test_recover_equals_host(gpu, Z, name):
    rm = matcher(Z, name)
    _, llr64 = frames(Z, name)
    for tin, tout in PAIRS:
        llr = llr64.astype(tin)
        dev = torch.from_numpy(llr).cuda()
        for n_out in (rm.n_dec, rm.n) if (tin, tout) == PAIRS[0] else (rm.n_dec,):
            want = rm.recover_host(llr, n_out=n_out, dtype=tout)
            for b in (1, B):
                got = rm.recover(dev[:b], n_out=n_out, dtype=tout)
                assert got.is_cuda and got.dtype == TT[tout] and got.shape == (b, n_out)
                assert bits_equal(got.cpu().numpy(), want[:b]), (tin, tout, n_out, b)
    got = rm.recover(llr64[:5].astype(np.float32), dtype="float32")  # NumPy in, NumPy out
    assert bits_equal(got, rm.recover_host(llr64[:5].astype(np.float32), dtype=np.float32))
    mine = np.full((5, rm.n_dec), -3.0)
    assert rm.recover(llr64[:5], out=mine) is mine and bits_equal(mine, rm.recover_host(llr64[:5]))


@pytest.mark.parametrize("Z", [7, 96])
@pytest.mark.parametrize("name", ["p2_f5_short", "p0_f5_mid_rep"])
@pytest.mark.parametrize("tin,tout", PAIRS)
def test_accumulate_over_two_matchers(gpu, Z, name, tin, tout):
    """Soft combining: a second transmission of the same frames from another start is added to the
    first one's recovery; what neither sent keeps the first recovery's value (fillers, zeros)."""
    L = _L()
    m1 = matcher(Z, name)
    c = dict(configs(Z)[name])
    c["start"] = (m1.rv_start(1) + 3) % m1.ncb
    m2 = L.QCRateMatcher(base_of(Z), Z, **c)
    assert m2.c0 != m1.c0
    rs = np.random.RandomState(Z)
    l1, l2 = ((rs.standard_normal((B, m1.E)) * 4).astype(tin) for _ in range(2))
    n = m1.n
    h1 = m1.recover_host(l1, n_out=n, dtype=tout)
    h2 = m2.recover_host(l2, out=h1, accumulate=True)
    assert not bits_equal(h1, h2)
    for b in (1, B):
        out = m1.recover(torch.from_numpy(l1[:b]).cuda(), n_out=n, dtype=tout)
        assert bits_equal(out.cpu().numpy(), h1[:b])
        got = m2.recover(torch.from_numpy(l2[:b]).cuda(), out=out, accumulate=True)
        assert got is out and bits_equal(out.cpu().numpy(), h2[:b]), b
    with pytest.raises(AssertionError):
        m2.recover(torch.from_numpy(l2).cuda(), accumulate=True)  # nothing to accumulate into


def _pitched(rows, off, ld, fill, dtype):
    """(buffer, view [rows, ld] of it `off` elements in)"""
    buf = torch.full((off + rows * ld + 32,), fill, dtype=dtype, device="cuda")
    return buf, buf[off:off + rows * ld].view(rows, ld)


@pytest.mark.parametrize("Z,name", [(7, "p2_f5_rep"), (27, "p0_f0_wrap"), (96, "p2_f5_infiller"), (96, "p0_f5_mid_rep")])
@pytest.mark.parametrize("vec", [True, False])
def test_pitched_views_on_both_store_paths(gpu, Z, name, vec):
    """Rows on 16-byte boundaries (16-byte stores and a cut last piece) or at an odd element offset with an
    odd pitch (a head piece that differs from row to row, element stores at both ends); the inputs always
    at an odd offset and pitch.  Beyond E and n_out nothing changes."""
    rm = matcher(Z, name)
    cw, llr64 = frames(Z, name)
    n, E, n_out = rm.n, rm.E, rm.n_dec
    # select
    _, cv = _pitched(B, 3, n + 5 + n % 2, 0x5B, torch.uint8)
    cv[:, :n] = torch.from_numpy(cw.copy()).cuda()
    ld, off = ((E + 15) // 16 * 16 + 16, 32) if vec else (E + 3 + E % 2, 1)
    ebuf, ev = _pitched(B, off, ld, 0xAA, torch.uint8)
    out = ev[:, :E]
    assert (out.data_ptr() % 16 == 0 and ld % 16 == 0) == vec and cv.data_ptr() % 2 == 1
    assert rm.select(cv[:, :n], out=out) is out
    assert np.array_equal(out.cpu().numpy(), rm.select_host(cw))
    flat = ebuf.cpu().numpy()
    assert (flat[:off] == 0xAA).all() and (flat[off + B * ld:] == 0xAA).all()
    assert (flat[off:off + B * ld].reshape(B, ld)[:, E:] == 0xAA).all()
    one = rm.select(cv[5:6, :n], out=ev[7:8, :E])  # one row: the pitch plays no part
    assert np.array_equal(one.cpu().numpy(), rm.select_host(cw[5:6]))
    # recover, both output types, fresh and accumulating
    for tin, tout in PAIRS:
        llr = llr64.astype(tin)
        _, lv = _pitched(B, 1, E + 3 + E % 2, 7.0, TT[tin])
        lv[:, :E] = torch.from_numpy(llr).cuda()
        ept = 16 // np.dtype(tout).itemsize
        ld, off = ((n_out + ept - 1) // ept * ept + ept, 2 * ept) if vec else (n_out + 3 + n_out % 2, 1)
        obuf, ov = _pitched(B, off, ld, -5.0, TT[tout])
        out = ov[:, :n_out]
        assert (out.data_ptr() % 16 == 0 and (ld * np.dtype(tout).itemsize) % 16 == 0) == vec
        want = rm.recover_host(llr, n_out=n_out, dtype=tout)
        assert rm.recover(lv[:, :E], out=out) is out
        assert bits_equal(out.cpu().numpy(), want), (tin, tout)
        rm.recover(lv[:, :E], out=out, accumulate=True)
        assert bits_equal(out.cpu().numpy(), rm.recover_host(llr, out=want, accumulate=True)), (tin, tout)
        flat = obuf.cpu().numpy()
        assert (flat[:off] == -5.0).all() and (flat[off + B * ld:] == -5.0).all()
        assert (flat[off:off + B * ld].reshape(B, ld)[:, n_out:] == -5.0).all()
        assert (lv.cpu().numpy()[:, E:] == 7.0).all()


def test_two_streams_and_empty_batch(gpu):
    rm = matcher(27, "p2_f5_rep")
    cw, llr = frames(27, "p2_f5_rep")
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
    assert e.shape == (0, rm.E) and e.dtype == torch.uint8 and e.is_cuda
    r = rm.recover(l[:0], dtype=np.float32)
    assert r.shape == (0, rm.n_dec) and r.dtype == torch.float32 and r.is_cuda
    assert rm.select(np.zeros((0, rm.n), np.uint8)).shape == (0, rm.E)
    N = _N()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    keep = r0.clone()
    assert N.lib.pl_ldpc_rate_recover(ctypes.byref(rm.rm), l.data_ptr(), rm.E, 0, r0.data_ptr(), rm.n_dec, rm.n_dec,
                                      1024.0, 0, st) == 0
    assert N.lib.pl_ldpc_rate_match(ctypes.byref(rm.rm), c.data_ptr(), rm.n, 0, e0.data_ptr(), rm.E, st) == 0
    torch.cuda.synchronize()
    assert torch.equal(r0, keep)


@pytest.mark.parametrize("Z", [7, 96])
def test_special_values(gpu, Z):
    """+-inf and -0.0 anywhere, the infinities of one position of one sign (no inf - inf); NaNs with
    payloads where a position has a single term and the types agree, so that no addition and no
    conversion touches them: they are copied bit for bit."""
    for name in ("p0_f0_rep", "p2_f5_rep", "p0_f5_mid_short"):
        rm = matcher(Z, name)
        pos = rm.positions_host()
        rs = np.random.RandomState(Z + len(name))
        llr = rs.standard_normal((B, rm.E)) * 4
        kind = rs.randint(0, 6, (B, rm.E))
        llr[kind == 0] = -0.0
        llr[kind == 1] = 0.0
        llr = np.where(kind == 2, np.where(pos % 2 == 0, np.inf, -np.inf)[None, :], llr)
        single = (np.bincount(pos, minlength=rm.n)[pos] == 1)[None, :] & (kind == 3)
        for tin, tout in PAIRS:
            x = llr.astype(tin)
            if tin == tout and single.any():
                u = x.view(UI[tin])
                pay = rs.randint(1, 1 << 20, x.shape).astype(UI[tin])
                quiet = UI[tin](0x7FF8000000000000 if tin == np.float64 else 0x7FC00000)
                sign = (rs.randint(0, 2, x.shape).astype(UI[tin]) << UI[tin](63 if tin == np.float64 else 31))
                u[single] = (quiet | pay | sign)[single]
                assert np.isnan(x[single]).all()
            want = rm.recover_host(x, dtype=tout)
            got = rm.recover(torch.from_numpy(x).cuda(), dtype=tout).cpu().numpy()
            assert bits_equal(got, want), (name, tin, tout)
            assert np.isinf(want).any() and (np.signbit(want) & (want == 0)).any()
            assert np.isnan(want).any() == bool(tin == tout and single.any())
    assert single.any()  # the last configuration has single terms: NaNs were tested


def test_identity_matcher(gpu):
    """punctured = 0, F = 0, start = 0, E = n: recovery returns the LLRs, and the harness counts what it
    counts without a matcher (the noise is keyed per frame and bit)."""
    from polarcode_and_ldpc_amd.channel.awgn import AWGNChannel
    from polarcode_and_ldpc_amd.harness.montecarlo import ldpc_round_fn
    L = _L()
    Z = 27
    base = base_of(Z)
    rm = L.QCRateMatcher(base, Z, NB * Z)
    assert rm.decoder_rows() == MB and rm.n_dec == rm.n and rm.M == rm.n and rm.c0 == 0
    cw = torch.from_numpy(frames(Z, "p0_f0_short")[0] & 1).cuda()
    assert torch.equal(rm.select(cw), cw)
    llr = torch.empty((B, rm.n), dtype=torch.float64, device="cuda")
    AWGNChannel(1.0).llr_batch_device(cw, rm.n, B, seed=11, frame_offset=0, out=llr)
    assert np.array_equal(rm.recover(llr).cpu().numpy(), llr.cpu().numpy())
    for dtype in (np.float64, np.float32):
        dec = L.QCLayeredMSDecoder(base, Z, max_iter=20, normalization=0.75, early_stop=True, dtype=dtype)
        for enc in (None, L.QCLDPCEncoder(base, Z)):
            plain = ldpc_round_fn(dec, seed=3, encoder=enc)
            rated = ldpc_round_fn(dec, seed=3, encoder=enc, rate_matcher=rm)
            for snr in (-3.0, 1.5):
                a, b = plain(1, snr, 100, 1003), rated(1, snr, 100, 1003)
                assert a.tolist() == b.tolist() and a[2] == 1003, (dtype, enc, snr)
            assert 0 < plain(1, -3.0, 100, 1003)[1] < 1003  # frames do fail there: the counters are not trivially 0
    with pytest.raises(AssertionError, match="decoder_base"):
        ldpc_round_fn(dec, rate_matcher=matcher(Z, "p2_f5_short"))


@pytest.mark.parametrize("Z,seed,E", [(27, 67, 167), (96, 4, 677)])
def test_noise_free_round_trip_with_punctured_columns(gpu, Z, seed, E):
    """Encode, select with two punctured block columns and E < M, noise-free LLRs, recover, decode on
    decoder_base(): the message comes back within max_iter.  The seeds were chosen on the CPU so that
    the host restatement (tests/qc_layered_ref.py) succeeds -- a random base can leave both punctured
    columns in every row they touch -- and that is asserted first; then the device equals it."""
    from qc_layered_ref import qc_layered_ms_ref
    L = _L()
    base = L.qc_encodable_base(MB, NB, Z, 3, seed, core=4, chained=False)
    rm = L.QCRateMatcher(base, Z, E, punctured=2)
    assert E < rm.M and rm.decoder_rows() < MB
    msg = np.random.RandomState(5).randint(0, 2, (B, rm.k)).astype(np.uint8)
    enc = L.QCLDPCEncoder(base, Z)
    cw = enc.encode_batch_device(torch.from_numpy(msg).cuda())
    assert np.array_equal(cw.cpu().numpy(), enc.encode_batch(msg))
    tx = rm.select(cw)
    assert np.array_equal(tx.cpu().numpy(), rm.select_host(cw.cpu().numpy()))
    for dtype in (np.float64, np.float32):
        rx = (8.0 * (1.0 - 2.0 * tx.to(torch.float64))).to(TT[dtype])
        llr = rm.recover(rx, dtype=dtype)
        assert bits_equal(llr.cpu().numpy(), rm.recover_host(rx.cpu().numpy(), dtype=dtype))
        rb, ri, _ = qc_layered_ms_ref(rm.decoder_base(), Z, llr.cpu().numpy(), 20, 0.75, True, dtype=dtype)
        assert np.array_equal(rb[:, :rm.k], msg) and ri.max() < 20, "the host restatement does not decode this seed"
        dec = L.QCLayeredMSDecoder(rm.decoder_base(), Z, max_iter=20, normalization=0.75, early_stop=True, dtype=dtype)
        bits, its = dec.decode_batch(llr, return_iterations=True)
        assert np.array_equal(bits.cpu().numpy(), rb) and np.array_equal(its.cpu().numpy(), ri)
        assert np.array_equal(bits.cpu().numpy()[:, :rm.n_dec], cw.cpu().numpy()[:, :rm.n_dec])


def test_harness_round_fn_rate_matched(gpu):
    """Shortened and punctured frames through ldpc_round_fn: counts belong to the frames, not to the calls;
    a lower rate at the same Es/N0 fails less often."""
    from polarcode_and_ldpc_amd.harness.montecarlo import ldpc_round_fn
    L = _L()
    Z = 27
    base = base_of(Z)
    enc = L.QCLDPCEncoder(base, Z)
    fer = {}
    for E in (170, 260):
        rm = L.QCRateMatcher(base, Z, E, punctured=2, fillers=5, start=0)
        dec = L.QCLayeredMSDecoder(rm.decoder_base(), Z, max_iter=20, normalization=0.75, early_stop=True,
                                   dtype=np.float32)
        f = ldpc_round_fn(dec, seed=3, encoder=enc, rate_matcher=rm)
        a = f(0, 12.0, 0, 1003)
        assert a.tolist() == [0, 0, 1003]
        lo = f(1, 0.0, 0, 1003)
        assert lo[2] == 1003 and lo[0] >= lo[1]
        assert (f(1, 0.0, 0, 500) + f(1, 0.0, 500, 503)).tolist() == lo.tolist()
        assert ldpc_round_fn(dec, seed=3, encoder=enc, rate_matcher=rm)(1, 0.0, 0, 1003).tolist() == lo.tolist()
        zero = ldpc_round_fn(dec, seed=3, rate_matcher=rm)(1, 0.0, 0, 1003)  # the all-zero codeword
        assert zero[2] == 1003 and zero[0] >= zero[1]
        fer[E] = lo[1]
    assert fer[260] < fer[170] and fer[170] > 0


def test_simulate_qc_ldpc_rate_matched_and_cli(gpu, tmp_path, capsys):
    from polarcode_and_ldpc_amd.harness import ber
    L = _L()
    base = L.qc_encodable_base(8, 12, 27, 3, 2, core=4, chained=False)
    snr, frames_ = [-1.0, 2.0], 3000
    rmargs = (200, 2, 5, 9 * 27, 31)
    n_dec = L.QCRateMatcher(base, 27, *rmargs).n_dec
    log = tmp_path / "points.jsonl"
    kw = dict(max_iter=20, normalization=0.75, dtype=np.float32, batch=1024, seed=5, random_codewords=True)
    _, f, pts = ber.simulate_qc_ldpc(snr, frames_, 10 ** 9, base, 27, log_path=str(log), rate_match=rmargs, **kw)
    assert [p.frames for p in pts] == [frames_] * 2 and [p.info_bits for p in pts] == [4 * 27 - 5] * 2
    assert frames_ > pts[0].frame_errors > pts[1].frame_errors >= 0
    rows = [json.loads(l) for l in log.read_text().splitlines() if l.strip()]
    assert len(rows) == 2 and all(r["key"]["rm"] == list(rmargs) and r["key"]["n_dec"] == n_dec for r in rows)
    size = log.stat().st_size
    _, _, again = ber.simulate_qc_ldpc(snr, frames_, 10 ** 9, base, 27, log_path=str(log), rate_match=rmargs, **kw)
    assert [(p.frame_errors, p.bit_errors) for p in again] == [(p.frame_errors, p.bit_errors) for p in pts]
    assert log.stat().st_size == size  # resumed: both points came from the log
    # the dict form is the same run; another E is another run key
    _, _, d = ber.simulate_qc_ldpc(snr, frames_, 10 ** 9, base, 27, log_path=str(log), **kw,
                                   rate_match=dict(E=200, punctured=2, fillers=5, ncb=243, start=31))
    assert log.stat().st_size == size and [p.frame_errors for p in d] == [p.frame_errors for p in pts]
    _, _, other = ber.simulate_qc_ldpc(snr, frames_, 10 ** 9, base, 27, log_path=str(tmp_path / "other.jsonl"),
                                       rate_match=(230, 2, 5, 243, 31), **kw)
    assert other[0].frame_errors < pts[0].frame_errors
    # the command line, with a log and a resume from it
    clog = tmp_path / "cli.jsonl"
    argv = ["--code", "qcldpc", "--qc", "8,12,27,3,2,4", "--rm", "200,2,5,243,31", "--ldpc-codewords", "random",
            "--dtype", "float32", "--norm", "0.75", "--snr=-1:2:3", "--frames", str(frames_), "--max-errors",
            str(10 ** 9), "--batch", "1024", "--seed", "5", "--max-iter", "20", "--log", str(clog)]
    # qc_encodable_base's default is chained=True: the command line's code is that one
    cbase = L.qc_encodable_base(8, 12, 27, 3, 2, core=4)
    _, _, cpts = ber.simulate_qc_ldpc(snr, frames_, 10 ** 9, cbase, 27, rate_match=rmargs, **kw)
    for _ in range(2):
        capsys.readouterr()
        ber.main(argv)
        out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
        assert out["code"] == "qcldpc" and out["snr_db"] == snr
        assert [(p["frame_errors"], p["bit_errors"]) for p in out["points"]] == \
            [(p.frame_errors, p.bit_errors) for p in cpts]
        csize = clog.stat().st_size if _ == 0 else csize
        assert clog.stat().st_size == csize
    capsys.readouterr()
    ber.main(["--code", "qcldpc", "--qc", "8,12,27,3,2,4", "--rm", "200,2,5", "--snr=1:1:1", "--frames", "1024",
              "--batch", "1024"])  # the all-zero codeword, default ncb and start
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert out["points"][0]["frames"] == 1024 and out["points"][0]["info_bits"] == 103
    with pytest.raises(SystemExit):
        ber.main(["--code", "qcldpc", "--rm", "200,2"])


def test_capi_refusals(gpu):
    """Every refusal comes before the first device call: nothing is written."""
    N = _N()
    rm = matcher(27, "p2_f5_short")
    cw, llr = frames(27, "p2_f5_short")
    n, E, hi, b = rm.n, rm.E, rm.hi, 5
    c = torch.from_numpy(cw[:b].copy()).cuda()
    l = torch.from_numpy(llr[:b].copy()).cuda()
    e = torch.full((b, E), 0xAA, dtype=torch.uint8, device="cuda")
    o = torch.full((b, n), -5.0, dtype=torch.float64, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    R = ctypes.byref(rm.rm)
    bad = N.RateMatch(MB, NB, 27, 2, 5, -1, 0, 0)  # E = 0
    sel, rec = N.lib.pl_ldpc_rate_match, N.lib.pl_ldpc_rate_recover
    P_ = lambda t: t.data_ptr()  # noqa: E731
    for name, call in {
        "rm NULL": lambda: sel(None, P_(c), n, b, P_(e), E, st),
        "rm refused": lambda: sel(ctypes.byref(bad), P_(c), n, b, P_(e), E, st),
        "cw NULL": lambda: sel(R, None, n, b, P_(e), E, st),
        "e NULL": lambda: sel(R, P_(c), n, b, None, E, st),
        "batch < 0": lambda: sel(R, P_(c), n, -1, P_(e), E, st),
        "ld_cw < n": lambda: sel(R, P_(c), n - 1, b, P_(e), E, st),
        "ld_e < E": lambda: sel(R, P_(c), n, b, P_(e), E - 1, st),
        "recover rm NULL": lambda: rec(None, P_(l), E, b, P_(o), n, n, 1024.0, 0, st),
        "recover rm refused": lambda: rec(ctypes.byref(bad), P_(l), E, b, P_(o), n, n, 1024.0, 0, st),
        "llr NULL": lambda: rec(R, None, E, b, P_(o), n, n, 1024.0, 0, st),
        "out NULL": lambda: rec(R, P_(l), E, b, None, n, n, 1024.0, 0, st),
        "recover batch < 0": lambda: rec(R, P_(l), E, -1, P_(o), n, n, 1024.0, 0, st),
        "n_out <= hi": lambda: rec(R, P_(l), E, b, P_(o), n, hi, 1024.0, 0, st),
        "n_out > n": lambda: rec(R, P_(l), E, b, P_(o), n + 1, n + 1, 1024.0, 0, st),
        "ld_llr < E": lambda: rec(R, P_(l), E - 1, b, P_(o), n, n, 1024.0, 0, st),
        "ld_out < n_out": lambda: rec(R, P_(l), E, b, P_(o), n - 1, n, 1024.0, 0, st),
        "flags": lambda: rec(R, P_(l), E, b, P_(o), n, n, 1024.0, 8, st),
        "out misaligned": lambda: rec(R, P_(l), E, b, P_(o) + 4, n, n - 1, 1024.0, 0, st),
        "llr misaligned": lambda: rec(R, P_(l) + 2, E, b, P_(o), n, n, 1024.0, N.PL_RM_LLR_F32, st),
    }.items():
        assert call() == N.PL_EINVAL and N.lib.pl_last_error(), name
    assert b"highest transmitted position" in (rec(R, P_(l), E, b, P_(o), n, hi, 1024.0, 0, st), N.lib.pl_last_error())[1]
    torch.cuda.synchronize()
    assert (e == 0xAA).all() and (o == -5.0).all()  # nothing was launched
    # the derived fields a caller leaves in the struct are not trusted
    junk = N.RateMatch(*[getattr(rm.rm, f) for f, _ in N.RateMatch._fields_][:8], 1, 2, 3, 4, 5, 6, 7)
    assert sel(ctypes.byref(junk), P_(c), n, b, P_(e), E, st) == 0
    assert rec(ctypes.byref(junk), P_(l), E, b, P_(o), n, hi + 1, 1024.0, 0, st) == 0
    torch.cuda.synchronize()
    assert np.array_equal(e.cpu().numpy(), rm.select_host(cw[:b]))
    got = o.cpu().numpy()
    assert bits_equal(got[:, :hi + 1], rm.recover_host(llr[:b], n_out=hi + 1)) and (got[:, hi + 1:] == -5.0).all()
    with pytest.raises(AssertionError):
        rm.recover(l, n_out=hi)
    with pytest.raises(AssertionError):
        rm.select(c[:, :-1])

"""QCLDPCEncoder.encode_batch_device (ldpc_qc_encode.hip) against the host encoder
(tests/test_ldpc_qc_encode_host.py checks that one against the expanded H) and
against the dense generator path, LDPCEncoder(H=qc_expand).encode_batch_device.
Bar: array_equal.

The bases are the host test's: Z = 1, 7, 27, 64 (64, 9, 2, 1 frames per
wavefront, with 1, 10 and 0 idle lanes), 65 and 96 (two wavefronts, 63 and 32
idle lanes, workgroup barriers), 1024 (the largest workgroup); g = mb, 4, 3 and
0; extensions with and without a row that reads an extension parity.  Batches:
1, 67, and one below / at / above the frames of a workgroup."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from test_ldpc_qc_encode_host import CASES, DENSE, base_of, probe

pytestmark = pytest.mark.gpu


def _L():
    import polarcode_and_ldpc_amd.ldpc as L
    return L


def _N():
    from polarcode_and_ldpc_amd import _native
    return _native


@functools.lru_cache(maxsize=None)
def fpg_of(case):
    rc, p, msg = probe(*base_of(case))
    assert rc == 0, msg
    return p.fpw * p.fpb


@functools.lru_cache(maxsize=None)
def pool(case):
    """(messages, codewords of the host encoder): enough rows for every batch of the case."""
    base, Z = base_of(case)
    enc = _L().QCLDPCEncoder(base, Z)
    msg = np.random.RandomState(77 + len(case)).randint(0, 2, (max(67, fpg_of(case) + 1), enc.k)).astype(np.uint8)
    cw = enc.encode_batch(msg).astype(np.uint8)
    msg.setflags(write=False)
    cw.setflags(write=False)
    return msg, cw


@functools.lru_cache(maxsize=None)
def encoder(case):
    return _L().QCLDPCEncoder(*base_of(case))


@pytest.mark.parametrize("case", sorted(CASES))
def test_device_encode_equals_host(gpu, case):
    msg, want = pool(case)
    enc = encoder(case)
    fpg = fpg_of(case)
    dev = torch.from_numpy(msg.copy()).cuda()
    for B in sorted({1, 67, fpg - 1, fpg, fpg + 1} - {0}):
        got = enc.encode_batch_device(dev[:B])
        assert got.dtype == torch.uint8 and got.shape == (B, enc.n) and got.is_cuda
        assert np.array_equal(got.cpu().numpy(), want[:B]), (case, B)


@pytest.mark.parametrize("case", DENSE)
def test_device_encode_equals_dense_path(gpu, case):
    L = _L()
    base, Z = base_of(case)
    msg, want = pool(case)
    enc = encoder(case)
    dense = L.LDPCEncoder(enc.n, enc.k, H=L.qc_expand(base, Z))
    assert np.array_equal(dense.info_positions, np.arange(enc.k))
    dev = torch.from_numpy(msg[:67].copy()).cuda()
    a = enc.encode_batch_device(dev)
    b = dense.encode_batch_device(dev)
    assert torch.equal(a, b) and np.array_equal(a.cpu().numpy(), want[:67])


def _pitched(rows, off, ld, fill):
    """(buffer, view [B, ld] of it `off` bytes in)"""
    buf = torch.full((off + rows * ld + 64,), fill, dtype=torch.uint8, device="cuda")
    return buf, buf[off:off + rows * ld].view(rows, ld)


@pytest.mark.parametrize("case", ["z27", "z7_core4_chained", "z65_core4_chained", "z96_triangular"])
@pytest.mark.parametrize("vin,vout", [(True, True), (True, False), (False, True), (False, False)])
def test_pitched_views_and_dirty_messages(gpu, case, vin, vout):
    """Row-pitched message and out views: 16-byte aligned with a pitch that is a multiple of 16 (the
    16-byte path) or at an odd offset with an odd pitch (the byte path); message bytes 2 and 255."""
    msg, want = pool(case)
    enc = encoder(case)
    B, k, n = 67, enc.k, enc.n
    ldm, offm = ((k + 15) // 16 * 16 + 16, 32) if vin else (k + 3 + (k % 2), 1)
    ldc, offc = ((n + 15) // 16 * 16 + 32, 16) if vout else (n + 5 + (n % 2), 3)
    assert ldm > k and ldc > n and (ldm % 16 == 0) == vin and (ldc % 16 == 0) == vout
    dirty = np.where(msg[:B] == 1, 255, 2).astype(np.uint8)
    dirty[::3] = msg[:B][::3]
    _, mv = _pitched(B, offm, ldm, 0x5B)
    mv[:, :k] = torch.from_numpy(dirty).cuda()
    obuf, ov = _pitched(B, offc, ldc, 0xAA)
    m_in, out = mv[:, :k], ov[:, :n]
    assert (m_in.data_ptr() % 16 == 0) == vin and (out.data_ptr() % 16 == 0) == vout
    got = enc.encode_batch_device(m_in, out=out)
    assert got.data_ptr() == out.data_ptr()
    assert np.array_equal(out.cpu().numpy(), want[:B])
    flat = obuf.cpu().numpy()
    assert (flat[:offc] == 0xAA).all() and (flat[offc + B * ldc:] == 0xAA).all()
    assert (flat[offc:offc + B * ldc].reshape(B, ldc)[:, n:] == 0xAA).all()  # the bytes beyond n stay untouched
    assert (mv.cpu().numpy()[:, k:] == 0x5B).all()
    # one row: the pitch plays no part
    got1 = enc.encode_batch_device(m_in[5:6], out=out[7:8])
    assert np.array_equal(got1.cpu().numpy(), want[5:6])


def test_numpy_input_and_empty_batch(gpu):
    msg, want = pool("z27")
    enc = encoder("z27")
    got = enc.encode_batch_device(msg[:11])
    assert got.is_cuda and np.array_equal(got.cpu().numpy(), want[:11])
    got = enc.encode_batch_device(msg[:11].astype(np.int64) + 4)  # other integer types; & 1 on the device
    assert np.array_equal(got.cpu().numpy(), want[:11])
    e = enc.encode_batch_device(np.zeros((0, enc.k), np.uint8))
    assert e.shape == (0, enc.n) and e.dtype == torch.uint8 and e.is_cuda
    out = torch.empty((0, enc.n), dtype=torch.uint8, device="cuda")
    assert enc.encode_batch_device(torch.empty((0, enc.k), dtype=torch.uint8, device="cuda"), out=out) is out
    with pytest.raises(AssertionError):
        enc.encode_batch_device(msg[:3, :-1])


@pytest.mark.parametrize("case", ["z7", "z65_core4_chained"])
def test_two_streams_and_second_call(gpu, case):
    msg, want = pool(case)
    enc = encoder(case)
    dev = torch.from_numpy(msg[:67].copy()).cuda()
    first = enc.encode_batch_device(dev)
    torch.cuda.synchronize()
    outs = []
    for s in (torch.cuda.Stream(), torch.cuda.Stream()):
        with torch.cuda.stream(s):
            outs.append(enc.encode_batch_device(dev))
    torch.cuda.synchronize()
    again = enc.encode_batch_device(dev)
    for o in outs + [again]:
        assert torch.equal(o, first)
    assert np.array_equal(first.cpu().numpy(), want[:67])


@pytest.mark.parametrize("case", ["z7", "z27", "z96", "z65_core4_chained", "z65_core4_nr"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_decoder_round_trip(gpu, case, dtype):
    """Noise-free LLRs of the device codewords: the decoder returns them after one iteration.  A word
    that is no codeword would leave a non-zero syndrome and run all 20."""
    L = _L()
    base, Z = base_of(case)
    msg, want = pool(case)
    cw = encoder(case).encode_batch_device(torch.from_numpy(msg[:67].copy()).cuda())
    llr = (8.0 * (1.0 - 2.0 * cw.to(torch.float64))).to(torch.float64 if dtype == np.float64 else torch.float32)
    dec = L.QCLayeredMSDecoder(base, Z, max_iter=20, normalization=0.75, early_stop=True, dtype=dtype)
    bits, its = dec.decode_batch(llr, return_iterations=True)
    assert torch.equal(bits, cw) and np.array_equal(cw.cpu().numpy(), want[:67])
    assert (its.cpu().numpy() == 1).all()


def test_harness_round_fn(gpu):
    from polarcode_and_ldpc_amd.harness.montecarlo import ldpc_round_fn
    L = _L()
    base, Z = base_of("z27")
    dec = L.QCLayeredMSDecoder(base, Z, max_iter=20, normalization=0.75, early_stop=True)

    def fn():
        return ldpc_round_fn(dec, encoder=L.QCLDPCEncoder(base, Z), seed=3)

    f = fn()
    a = f(0, 12.0, 0, 1003)
    assert a.tolist() == [0, 0, 1003]
    assert f(0, 12.0, 0, 1003).tolist() == a.tolist() and fn()(0, 12.0, 0, 1003).tolist() == a.tolist()
    assert (f(0, 12.0, 0, 500) + f(0, 12.0, 500, 503)).tolist() == a.tolist()
    # the same where frames fail: the counts belong to the frames, not to the calls
    lo = f(1, -2.0, 0, 1003)
    assert lo[2] == 1003 and 0 < lo[1] < 1003 and lo[0] >= lo[1]
    assert (f(1, -2.0, 0, 500) + f(1, -2.0, 500, 503)).tolist() == lo.tolist() == fn()(1, -2.0, 0, 1003).tolist()


def _create(lib, base, Z):
    sh = np.ascontiguousarray(base, np.int32)
    h = ctypes.c_void_p()
    rc = lib.pl_ldpc_qc_encoder_create(sh.shape[0], sh.shape[1], Z, sh.ctypes.data_as(ctypes.c_void_p), ctypes.byref(h))
    return rc, h


def test_capi_arguments(gpu):
    N = _N()
    base, Z = base_of("z27")
    msg, want = pool("z27")
    k, n, B = msg.shape[1], want.shape[1], 5
    rc, h = _create(N.lib, base, Z)
    assert rc == 0, N.lib.pl_last_error()
    m = torch.from_numpy(msg[:B].copy()).cuda()
    c = torch.zeros((B, n), dtype=torch.uint8, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    P_ = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    enc = N.lib.pl_ldpc_qc_encode
    for name, call in {
        "encoder NULL": lambda: enc(None, P_(m), k, B, P_(c), n, st),
        "msg NULL": lambda: enc(h, None, k, B, P_(c), n, st),
        "cw NULL": lambda: enc(h, P_(m), k, B, None, n, st),
        "ld_msg < k": lambda: enc(h, P_(m), k - 1, B, P_(c), n, st),
        "ld_cw < n": lambda: enc(h, P_(m), k, B, P_(c), n - 1, st),
        "batch < 0": lambda: enc(h, P_(m), k, -1, P_(c), n, st),
    }.items():
        assert call() == N.PL_EINVAL and N.lib.pl_last_error(), name
    torch.cuda.synchronize()
    assert not c.any()  # nothing was launched
    assert enc(h, P_(m), k, 0, P_(c), n, st) == 0 and enc(h, P_(m), k, B, P_(c), n, st) == 0
    torch.cuda.synchronize()
    assert np.array_equal(c.cpu().numpy(), want[:B])
    assert N.lib.pl_debug_set_qc_encoder_device(h, 0) == N.PL_EUNSUPPORTED  # the product library has no such hook
    assert N.lib.pl_ldpc_qc_encoder_destroy(h) == 0 and N.lib.pl_ldpc_qc_encoder_destroy(None) == 0
    out = ctypes.c_void_p(1)
    sh = np.ascontiguousarray(_L().qc_random_base(4, 8, 7, 3, seed=115), np.int32)
    assert N.lib.pl_ldpc_qc_encoder_create(4, 8, 7, sh.ctypes.data_as(ctypes.c_void_p), ctypes.byref(out)) \
        == N.PL_EUNSUPPORTED and out.value is None
    assert N.lib.pl_ldpc_qc_encoder_create(4, 8, 7, sh.ctypes.data_as(ctypes.c_void_p), None) == N.PL_EINVAL


def test_wrong_device_is_refused(gpu):
    """Encoding from another device than the encoder's is refused as plans refuse it (the diagnostic
    build's pl_debug_set_qc_encoder_device stands in for a second GPU); destroy works after use."""
    N = _N()
    D = N.load_diag()
    assert D is not None, "diagnostic library not built (make -C polarcode_and_ldpc_amd/csrc diag)"
    base, Z = base_of("z65_core4_chained")
    msg, want = pool("z65_core4_chained")
    k, n, B = msg.shape[1], want.shape[1], 9
    rc, h = _create(D, base, Z)
    assert rc == 0, D.pl_last_error()
    m = torch.from_numpy(msg[:B].copy()).cuda()
    c = torch.zeros((B, n), dtype=torch.uint8, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    P_ = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    cur = torch.cuda.current_device()
    assert D.pl_debug_set_qc_encoder_device(h, cur + 7) == 0
    assert D.pl_ldpc_qc_encode(h, P_(m), k, B, P_(c), n, st) == N.PL_EINVAL
    assert b"not the encoder's device" in D.pl_last_error()
    torch.cuda.synchronize()
    assert not c.any()
    assert D.pl_debug_set_qc_encoder_device(h, cur) == 0
    assert D.pl_ldpc_qc_encode(h, P_(m), k, B, P_(c), n, st) == 0
    torch.cuda.synchronize()
    assert np.array_equal(c.cpu().numpy(), want[:B])
    assert D.pl_ldpc_qc_encoder_destroy(h) == 0


def test_simulate_qc_ldpc_and_cli(gpu, tmp_path, capsys):
    """harness.ber.simulate_qc_ldpc and `--code qcldpc`: all-zero and random codewords, the point log and
    a resume from it, the --qc parsing with and without a core."""
    import json
    from polarcode_and_ldpc_amd.harness import ber
    L = _L()
    base = L.qc_encodable_base(6, 10, 27, 3, 2, core=4)
    snr, frames = [-1.0, 1.0], 3000
    res = {}
    for rnd in (False, True):
        log = str(tmp_path / ("points_%d.jsonl" % rnd))
        b, f, pts = ber.simulate_qc_ldpc(snr, frames, 10 ** 9, base, 27, max_iter=20, normalization=0.75,
                                         dtype=np.float32, batch=1024, seed=5, random_codewords=rnd, log_path=log)
        assert [p.frames for p in pts] == [frames, frames] and [p.info_bits for p in pts] == [108, 108]
        assert pts[0].frame_errors > pts[1].frame_errors >= 0 and pts[0].frame_errors < frames
        assert np.allclose(f, [p.frame_errors / frames for p in pts]) and len(b) == 2
        with open(log) as fh:
            assert len([l for l in fh if l.strip()]) >= 2
        # a resume takes both points from the log: same counts, no new row
        size = (tmp_path / ("points_%d.jsonl" % rnd)).stat().st_size
        _, _, again = ber.simulate_qc_ldpc(snr, frames, 10 ** 9, base, 27, max_iter=20, normalization=0.75,
                                           dtype=np.float32, batch=1024, seed=5, random_codewords=rnd, log_path=log)
        assert [(p.frame_errors, p.bit_errors) for p in again] == [(p.frame_errors, p.bit_errors) for p in pts]
        assert (tmp_path / ("points_%d.jsonl" % rnd)).stat().st_size == size
        res[rnd] = [(p.frame_errors, p.bit_errors) for p in pts]
    # float64 on the same frames: another decoder, the same frame source
    _, _, p64 = ber.simulate_qc_ldpc(snr, frames, 10 ** 9, base, 27, batch=1024, seed=5, random_codewords=True)
    assert [p.frames for p in p64] == [frames, frames]
    # the command line: the same code, seed and frames give the same counts
    argv = ["--code", "qcldpc", "--qc", "6,10,27,3,2,4", "--ldpc-codewords", "random", "--dtype", "float32", "--norm",
            "0.75", "--snr=-1:1:2", "--frames", str(frames), "--max-errors", str(10 ** 9), "--batch", "1024",
            "--seed", "5", "--max-iter", "20"]
    capsys.readouterr()
    ber.main(argv)
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert out["code"] == "qcldpc" and out["snr_db"] == snr
    assert [(p["frame_errors"], p["bit_errors"]) for p in out["points"]] == res[True]
    capsys.readouterr()
    ber.main(["--code", "qcldpc", "--qc", "4,8,27,3,1", "--snr=1:1:1", "--frames", "1024", "--batch", "1024"])
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert out["points"][0]["frames"] == 1024 and out["points"][0]["info_bits"] == 108
    with pytest.raises(SystemExit):
        ber.main(["--code", "qcldpc", "--qc", "4,8,27,3"])

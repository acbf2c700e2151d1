"""The bit interleaver on the device (csrc/interleave.hip) against channel.BitInterleaver's host methods, which
tests/test_interleave_host.py holds to the definition's loops (tests/interleave_ref.py): bit for bit, at
every store path, pitch and alignment, on both sides of the LDS threshold; a non-default stream; the
C-ABI's refusals; the harness chains against chains composed by hand from the public device methods.
The definition: include/polarldpc.h at pl_interleave_check."""
import functools
import json

import numpy as np
import pytest
import torch

from test_interleave_host import llr_payload, raw

pytestmark = pytest.mark.gpu

SMALL = (1, 2, 3, 5, 6, 7, 9, 10, 11, 64, 65, 1000, 1027, 4095, 4096)
LONG = (500499, 500500, 500501)  # around T (T + 1) / 2 at T = 1000: the direct kernels
KINDS = [("tri", None)] + [("rect", r) for r in (1, 2, 3, 4, 6, 8, 64)]
DTYPES = {"u8": np.uint8, "f64": np.float64, "f32": np.float32}
TT = {np.uint8: torch.uint8, np.float64: torch.float64, np.float32: torch.float32}
INT = {1: torch.uint8, 4: torch.int32, 8: torch.int64}
FILL = {np.uint8: 0xA5, np.float64: -12345.5, np.float32: -12345.5}


def _native():
    from polarcode_and_ldpc_amd import _native as n
    return n


@functools.lru_cache(maxsize=None)
def ilv(kind, rows, E):
    from polarcode_and_ldpc_amd.channel import BitInterleaver
    return BitInterleaver(kind, E, rows=rows)


def threshold(dtype):
    return _native().ILV_LDS_MAX_E[np.dtype(dtype).itemsize]


def lengths(dtype):
    """(E, batches): the grid, the long frames, and the largest E of the LDS regime and that plus 1"""
    t = threshold(dtype)
    return [(E, (1, 67)) for E in SMALL] + [(E, (1,)) for E in LONG] + [(t, (1, 3)), (t + 1, (1, 3))]


def payload(B, E, dtype, seed):
    if dtype == np.uint8:
        return np.random.default_rng(seed).integers(0, 256, size=(B, E), dtype=np.uint8)  # bytes copied whole
    return llr_payload((B, E), dtype, seed=seed)


def view(B, E, ld, off, dtype):
    """a [B, E] view of row pitch ld that starts off elements past a 16-byte boundary of a sentinel-filled
    flat tensor (the allocator's blocks are aligned far beyond 16 bytes)"""
    flat = torch.full((off + B * ld + 8,), FILL[dtype], dtype=TT[dtype], device="cuda")
    assert flat.data_ptr() % 16 == 0
    return flat, flat[off:off + B * ld].view(B, ld)[:, :E]


def put(dst, a):
    """a's bits into the device view dst (through integers: no float ever touches them)"""
    dst.view(INT[a.dtype.itemsize]).copy_(torch.from_numpy(raw(a).view("i%d" % a.dtype.itemsize)
                                                           if a.dtype.itemsize > 1 else a))


def bits_of(t):
    return raw(t.contiguous().view(INT[t.element_size()]).cpu().numpy())


def only_view_written(flat, B, E, ld, off, dtype):
    h = bits_of(flat).copy()
    fill = raw(np.array([FILL[dtype]], dtype=dtype))[0]
    h[off:off + B * ld].reshape(B, ld)[:, :E] = fill
    return bool(np.all(h == fill))


def run(il, x, out=None, stream=None):
    """bits (uint8, a tensor or NumPy) are interleaved, LLRs deinterleaved"""
    fn = il.interleave if str(x.dtype).split(".")[-1] == "uint8" else il.deinterleave
    return fn(x, out=out, stream=stream)


def host(il, a):
    return il.interleave_host(a) if a.dtype == np.uint8 else il.deinterleave_host(a)


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("kind,rows", KINDS, ids=lambda v: str(v))
def test_equals_host(gpu, kind, rows, dt):
    """contiguous tensors in, a fresh tensor out; NumPy in, NumPy out"""
    dtype = DTYPES[dt]
    for E, batches in lengths(dtype):
        il = ilv(kind, rows, E)
        for B in batches:
            a = payload(B, E, dtype, seed=E + B)
            want = raw(host(il, a))
            x = torch.empty((B, E), dtype=TT[dtype], device="cuda")
            put(x, a)
            got = run(il, x)
            assert got.dtype == TT[dtype] and got.shape == (B, E) and np.array_equal(bits_of(got), want), (E, B)
        if E <= 1027:
            back = run(il, a)
            assert isinstance(back, np.ndarray) and back.dtype == dtype and np.array_equal(raw(back), want), E


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("kind,rows", KINDS, ids=lambda v: str(v))
def test_pitch_alignment_and_sentinels(gpu, kind, rows, dt):
    """pitched rows on both sides, the input 3 and the output 1, 2 and 3 elements past a 16-byte boundary;
    nothing beyond E or between the rows is written"""
    dtype = DTYPES[dt]
    for E, batches in lengths(dtype):
        il = ilv(kind, rows, E)
        B = batches[-1]
        a = payload(B, E, dtype, seed=3 * E + B)
        want = raw(host(il, a))
        _, x = view(B, E, E + 5, 3, dtype)
        put(x, a)
        for off in (1, 2, 3):
            flat, out = view(B, E, E + 3, off, dtype)
            assert run(il, x, out=out) is out
            assert np.array_equal(bits_of(out), want), (E, B, off)
            assert only_view_written(flat, B, E, E + 3, off, dtype), (E, B, off)


def test_round_trip_and_stream(gpu):
    """deinterleave(interleave) is the identity on the device; a non-default stream gives the same bits"""
    side = torch.cuda.Stream()
    for kind, rows in (("tri", None), ("rect", 6)):
        for E in (1027, threshold(np.float64) + 1):
            il = ilv(kind, rows, E)
            a = payload(5, E, np.float64, seed=E)
            x = torch.empty((5, E), dtype=torch.float64, device="cuda")
            put(x, a)
            want = bits_of(il.deinterleave(x))
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                again = il.deinterleave(x, stream=side)
            side.synchronize()
            assert np.array_equal(bits_of(again), want)
            b = torch.from_numpy(payload(5, E, np.uint8, seed=E)).cuda()
            f = il.interleave(b)
            with torch.cuda.stream(side):
                side.wait_stream(torch.cuda.current_stream())
                f2 = il.interleave(b, stream=side)
            side.synchronize()
            assert torch.equal(f, f2)
            # the LLRs of the interleaved bits, deinterleaved, are the LLRs of the bits
            assert torch.equal(il.deinterleave(f.to(torch.float32)), b.to(torch.float32))


def test_out_rules(gpu):
    il = ilv("rect", 4, 10)
    b = torch.zeros((2, 10), dtype=torch.uint8, device="cuda")
    l = torch.zeros((2, 10), dtype=torch.float64, device="cuda")
    for bad in (torch.zeros((2, 10), dtype=torch.float64, device="cuda"), torch.zeros((2, 11), dtype=torch.uint8, device="cuda"),
                torch.zeros((3, 10), dtype=torch.uint8, device="cuda"), torch.zeros((2, 10), dtype=torch.uint8),
                torch.zeros((2, 20), dtype=torch.uint8, device="cuda")[:, ::2]):
        with pytest.raises(AssertionError, match="out must be"):
            il.interleave(b, out=bad)
    with pytest.raises(AssertionError, match="out must be"):
        il.deinterleave(l, out=torch.zeros((2, 10), dtype=torch.float32, device="cuda"))
    with pytest.raises(AssertionError, match="bits must be"):
        il.interleave(l)
    with pytest.raises(AssertionError, match="llr must be"):
        il.deinterleave(b)
    with pytest.raises(AssertionError, match="overlap"):
        il.interleave(b, out=b)
    assert il.interleave(torch.zeros((0, 10), dtype=torch.uint8, device="cuda")).shape == (0, 10)
    # a strided input is made contiguous first
    wide = torch.from_numpy(payload(2, 20, np.uint8, seed=1)).cuda()
    assert torch.equal(il.interleave(wide[:, ::2]), il.interleave(wide[:, ::2].contiguous()))


# ---- the C-ABI ----
def test_capi_refusals(gpu):
    n = _native()
    lib, EINVAL = n.lib, n.PL_EINVAL
    RECT, TRI = n.PL_ILV_RECT, n.PL_ILV_TRI
    E, B, ld = 10, 2, 12
    e = torch.full((B, ld), 7, dtype=torch.uint8, device="cuda")
    f = torch.full((B, ld), 9, dtype=torch.uint8, device="cuda")
    l64 = torch.full((2, B, ld), -12345.5, dtype=torch.float64, device="cuda")
    l32 = torch.full((2, B, ld), -12345.5, dtype=torch.float32, device="cuda")
    ep, fp = e.data_ptr(), f.data_ptr()
    st = n._stream()

    def il(kind=RECT, rows=4, E=E, B=B, e=ep, lde=ld, f=fp, ldf=ld):
        return lib.pl_bit_interleave(kind, rows, E, B, e, lde, f, ldf, st)

    def de(kind=RECT, rows=4, E=E, B=B, f=l64[0].data_ptr(), ldf=ld, e=l64[1].data_ptr(), lde=ld, flags=0):
        return lib.pl_llr_deinterleave(kind, rows, E, B, f, ldf, e, lde, flags, st)

    def refused(rc, word):
        msg = (lib.pl_last_error() or b"").decode()
        assert rc == EINVAL and word in msg, (rc, msg, word)

    for fn in (il, de):
        refused(fn(kind=2), "kind = 2")
        refused(fn(kind=-1, E=0, rows=99), "kind = -1")
        refused(fn(E=0), "E = 0")
        refused(fn(E=0, rows=0), "E = 0")
        refused(fn(E=(1 << 30) + 1), "E = ")
        refused(fn(rows=0), "rows = 0")
        refused(fn(rows=65), "rows = 65")
        refused(fn(kind=TRI, rows=4), "rows = 4")
        refused(fn(B=-1), "batch")
        refused(fn(e=None), "NULL")
        refused(fn(f=None), "NULL")
        refused(fn(lde=E - 1), "ld_e")
        refused(fn(ldf=E - 1), "ld_f")
    refused(de(flags=2), "flag")
    refused(de(flags=-1), "flag")
    refused(de(f=l64[0].data_ptr() + 4), "aligned")
    refused(de(e=l64[1].data_ptr() + 4), "aligned")
    refused(de(f=l32[0].data_ptr() + 2, e=l32[1].data_ptr(), flags=n.PL_ILV_LLR_F32), "aligned")
    # overlap: the same buffer, a shifted one, rows of one side in the gaps of the other, the last byte
    refused(il(f=ep), "overlap")
    refused(il(f=ep + E), "overlap")  # row 0 of f ends inside row 1 of e
    refused(il(f=ep + ld + E - 1), "overlap")
    refused(il(e=fp + 1), "overlap")
    refused(de(e=l64[0].data_ptr()), "overlap")
    refused(de(e=l64[0].data_ptr() + 8 * (ld + E - 1)), "overlap")
    refused(de(f=l32[0].data_ptr(), e=l32[0].data_ptr() + 4 * (ld + E - 1), flags=n.PL_ILV_LLR_F32), "overlap")
    torch.cuda.synchronize()
    assert bool((e == 7).all()) and bool((f == 9).all()) and bool((l64 == -12345.5).all())  # nothing was launched
    # just clear of each other is accepted, and a float pointer needs 4-byte alignment only
    assert il(B=1, f=ep + E) == 0  # one row: [e, e + E) then [f, f + E)
    assert de(B=1, f=l32[0].data_ptr() + 4, e=l32[1].data_ptr() + 4, flags=n.PL_ILV_LLR_F32) == 0
    assert il(kind=TRI, rows=0) == 0
    torch.cuda.synchronize()
    # batch == 0 launches nothing, whatever the pointers
    f.fill_(9)
    assert il(B=0, e=None, f=None) == 0 and de(B=0, e=None, f=None) == 0 and il(B=0) == 0 and de(B=0) == 0
    torch.cuda.synchronize()
    assert bool((f == 9).all())


# ---- the chains ----
def modem(m):
    from polarcode_and_ldpc_amd.channel import QAMModem
    return None if m is None else QAMModem(m)


def make_ilv(kind, E, mod):
    from polarcode_and_ldpc_amd.channel import BitInterleaver
    if kind == "tri":
        return BitInterleaver("tri", E)
    return BitInterleaver.for_modem(mod, E) if mod is not None else BitInterleaver("rect", E, rows=4)


def channel_by_hand(il, mod, tx, snr, seed, offset, dtype=np.float64):
    """interleave, the channel (BPSK or QAM), deinterleave: the public device methods"""
    from polarcode_and_ldpc_amd.channel import AWGNChannel
    B, E = tx.shape
    f = il.interleave(tx)
    if mod is None:
        rx = AWGNChannel(snr).llr_batch_device(f, E, B, seed=seed, frame_offset=offset)
    else:
        rx = mod.demap(mod.awgn(f, E, B, snr, seed, frame_offset=offset), E, snr, dtype=dtype)
    return il.deinterleave(rx)


def polar_by_hand(dec, rm, il, mod, seed, snr_index, snr, offset, B):
    from polarcode_and_ldpc_amd.harness.montecarlo import _stream_seed
    n = _native()
    s = _stream_seed(seed, snr_index)
    msg = torch.empty((B, dec._n_info), dtype=torch.uint8, device="cuda")
    n.random_bits(s, offset, msg)
    cw = torch.empty((B, dec.N), dtype=torch.uint8, device="cuda")
    n.polar_encode(dec.plan, msg, cw)
    tx = rm.select(cw) if rm is not None else cw
    rx = channel_by_hand(il, mod, tx, snr, s ^ 0xA5A5A5A5, offset)
    llr = rm.recover(rx) if rm is not None else rx
    out = torch.empty((B, dec._n_info), dtype=torch.uint8, device="cuda")
    dec.plan.decode(llr, out)
    counts = torch.zeros(3, dtype=torch.int64, device="cuda")
    n.count_errors(msg, out, dec._n_info, counts)
    return counts.cpu().tolist()


MODS = [None, 4, 6]
SNR = {None: 0.0, 4: 6.0, 6: 10.0}  # where these short codes fail now and then: the counts are not trivial


@pytest.mark.parametrize("kind", ["rect", "tri"])
@pytest.mark.parametrize("m", MODS, ids=["bpsk", "16qam", "64qam"])
def test_polar_chain(gpu, m, kind):
    import polarcode_and_ldpc_amd.polar as P
    from polarcode_and_ldpc_amd.harness.montecarlo import polar_round_fn
    N, K, E, B = 256, 100, 200, 256
    rm = P.PolarRateMatcher(N, E, "puncture")
    dec = P.SCLDecoder(N, K, list_size=4, frozen_bits=P.construct_rate_matched(K, rm))
    mod = modem(m)
    il = make_ilv(kind, E, mod)
    fn = polar_round_fn(dec, seed=5, rate_matcher=rm, modulation=mod, interleaver=il)
    got = fn(1, SNR[m], 3, B).tolist()
    print("polar chain %s %s: [bit errors, frame errors, frames] = %s" % (m, kind, got))
    assert got == polar_by_hand(dec, rm, il, mod, 5, 1, SNR[m], 3, B) and got[2] == B
    assert fn(0, SNR[m], 0, 100).tolist() == polar_by_hand(dec, rm, il, mod, 5, 0, SNR[m], 0, 100)  # a smaller round
    assert fn(0, 40.0, 0, B).tolist() == [0, 0, B]
    with pytest.raises(AssertionError, match="transmitted length"):
        polar_round_fn(dec, seed=5, rate_matcher=rm, modulation=mod, interleaver=make_ilv(kind, E + 1, mod))


def test_polar_chain_without_a_matcher_and_default(gpu):
    import polarcode_and_ldpc_amd.polar as P
    from polarcode_and_ldpc_amd.harness.montecarlo import polar_round_fn
    N, K, B = 256, 128, 256
    dec = P.SCLDecoder(N, K, list_size=4, frozen_bits=P.construct_frozen_set(N, K))
    mod = modem(4)
    il = make_ilv("rect", N, mod)
    got = polar_round_fn(dec, seed=5, modulation=mod, interleaver=il)(1, 7.0, 3, B).tolist()
    assert got == polar_by_hand(dec, None, il, mod, 5, 1, 7.0, 3, B)
    # interleaver=None: the counts of a call written without the argument
    rm = P.PolarRateMatcher(N, 200, "puncture")
    drm = P.SCLDecoder(N, 100, list_size=4, frozen_bits=P.construct_rate_matched(100, rm))
    for d, kw in ((dec, {}), (drm, {"rate_matcher": rm}), (drm, {"rate_matcher": rm, "modulation": mod})):
        assert polar_round_fn(d, seed=5, interleaver=None, **kw)(1, 5.0, 3, B).tolist() == \
            polar_round_fn(d, seed=5, **kw)(1, 5.0, 3, B).tolist()


def ldpc_by_hand(dec, enc, rm, il, mod, seed, snr_index, snr, offset, B):
    from polarcode_and_ldpc_amd.harness.montecarlo import _stream_seed
    n = _native()
    s = _stream_seed(seed, snr_index)
    msg = torch.empty((B, enc.k), dtype=torch.uint8, device="cuda")
    n.random_bits(s, offset, msg)
    kf = enc.k if rm is None else rm.k - rm.fillers
    msg[:, kf:] = 0
    cw = enc.encode_batch_device(msg)
    tx = rm.select(cw) if rm is not None else cw
    rx = channel_by_hand(il, mod, tx, snr, s ^ 0xA5A5A5A5, offset, dtype=dec.dtype)
    llr = rm.recover(rx, dtype=dec.dtype) if rm is not None else rx
    out = torch.empty((B, dec.n), dtype=torch.uint8, device="cuda")
    its = torch.empty((B,), dtype=torch.int32, device="cuda")
    dec.plan.decode(llr, out, its)
    counts = torch.zeros(3, dtype=torch.int64, device="cuda")
    info = torch.from_numpy(np.asarray(enc.info_positions, dtype=np.int64)).cuda()
    n.count_errors(msg, out if rm is not None else out.index_select(1, info).contiguous(), kf, counts)
    return counts.cpu().tolist()


@functools.lru_cache(maxsize=None)
def qc_code():
    import polarcode_and_ldpc_amd.ldpc as L
    Z = 27
    base = L.qc_encodable_base(8, 12, Z, 3, 2, core=4, chained=False)
    return base, Z, L.QCLDPCEncoder(base, Z), L.QCRateMatcher(base, Z, 260, punctured=2, fillers=5, start=0)


@pytest.mark.parametrize("kind", ["rect", "tri"])
@pytest.mark.parametrize("m", MODS, ids=["bpsk", "16qam", "64qam"])
def test_ldpc_chain(gpu, m, kind):
    import polarcode_and_ldpc_amd.ldpc as L
    from polarcode_and_ldpc_amd.harness.montecarlo import ldpc_round_fn
    base, Z, enc, rm = qc_code()
    mod = modem(m)
    il = make_ilv(kind, rm.E, mod)
    B = 256
    for dt in (np.float64, np.float32):
        dec = L.QCLayeredMSDecoder(rm.decoder_base(), Z, max_iter=20, normalization=0.75, early_stop=True, dtype=dt)
        fn = ldpc_round_fn(dec, seed=3, encoder=enc, rate_matcher=rm, modulation=mod, interleaver=il)
        got = fn(1, SNR[m] + 2.0, 7, B).tolist()
        print("ldpc chain %s %s %s: [bit errors, frame errors, frames] = %s" % (m, kind, np.dtype(dt).name, got))
        assert got == ldpc_by_hand(dec, enc, rm, il, mod, 3, 1, SNR[m] + 2.0, 7, B) and got[2] == B, dt
        assert fn(0, 40.0, 0, 100).tolist() == [0, 0, 100]


def test_ldpc_chain_without_a_matcher_and_default(gpu):
    import polarcode_and_ldpc_amd.ldpc as L
    from polarcode_and_ldpc_amd.harness.montecarlo import ldpc_round_fn
    base, Z, enc, rm = qc_code()
    mod = modem(6)
    dec = L.QCLayeredMSDecoder(base, Z, max_iter=20, normalization=0.75, early_stop=True, dtype=np.float32)
    il = make_ilv("rect", dec.n, mod)
    got = ldpc_round_fn(dec, seed=3, encoder=enc, modulation=mod, interleaver=il)(1, 9.0, 7, 256).tolist()
    assert got == ldpc_by_hand(dec, enc, None, il, mod, 3, 1, 9.0, 7, 256)
    drm = L.QCLayeredMSDecoder(rm.decoder_base(), Z, max_iter=20, normalization=0.75, early_stop=True)
    for e in (None, enc):
        for d, kw in ((dec, {}), (drm, {"rate_matcher": rm})):
            assert ldpc_round_fn(d, seed=3, encoder=e, interleaver=None, **kw)(1, -1.0, 7, 256).tolist() == \
                ldpc_round_fn(d, seed=3, encoder=e, **kw)(1, -1.0, 7, 256).tolist()
    with pytest.raises(AssertionError, match="interleaver needs an encoder"):
        ldpc_round_fn(dec, interleaver=il, encoder=None)
    with pytest.raises(AssertionError, match="interleaver needs an encoder"):
        ldpc_round_fn(drm, interleaver=make_ilv("tri", rm.E, None), encoder=None, rate_matcher=rm)


def test_simulate_and_cli(gpu, capsys, tmp_path):
    from polarcode_and_ldpc_amd.channel import BitInterleaver
    from polarcode_and_ldpc_amd.harness import ber
    cfg = {"encoding": {"N": 256, "K": 100}}
    log = tmp_path / "polar.jsonl"
    b, f, pts = ber.simulate_polar([30.0], 256, 100, cfg, list_size=4, batch=256, rate_match=dict(E=200, mode="puncture"),
                                   modulation=modem(4), interleaver=BitInterleaver("tri", 200), log_path=str(log))
    assert pts[0].frames == 256 and pts[0].frame_errors == 0
    assert '"interleave": ["tri", 0]' in log.read_text()
    with pytest.raises(AssertionError, match="transmitted length"):
        ber.simulate_polar([30.0], 256, 100, cfg, list_size=4, batch=256, rate_match=dict(E=200, mode="puncture"),
                           interleaver=BitInterleaver("tri", 256))
    base, Z, enc, rm = qc_code()
    log2 = tmp_path / "qc.jsonl"
    b, f, pts = ber.simulate_qc_ldpc([30.0], 256, 100, base, Z, batch=256, random_codewords=True, rate_match=(260, 2, 5),
                                     modulation=modem(6), dtype=np.float32, interleaver=("rect", None),
                                     log_path=str(log2))
    assert pts[0].frames == 256 and pts[0].frame_errors == 0
    assert '"interleave": ["rect", 6]' in log2.read_text()
    with pytest.raises(AssertionError, match="interleaver needs an encoder"):
        ber.simulate_qc_ldpc([30.0], 256, 100, base, Z, batch=256, rate_match=(260, 2, 5), interleaver=("tri", None))
    # the run key has no entry without the argument
    log3 = tmp_path / "plain.jsonl"
    ber.simulate_polar([30.0], 256, 100, cfg, list_size=4, batch=256, rate_match=dict(E=200, mode="puncture"),
                       log_path=str(log3))
    assert "interleave" not in log3.read_text()
    # the command line
    common = ["--code", "polar", "--N", "256", "--K", "100", "--list-size", "4", "--polar-rm", "200,puncture",
              "--snr=30:30:1", "--frames", "256", "--batch", "256"]
    for i, (extra, key) in enumerate(((["--modulation", "16qam", "--interleave", "rect"], ["rect", 4]),
                                      (["--interleave", "rect", "--interleave-rows", "8"], ["rect", 8]),
                                      (["--modulation", "64qam", "--interleave", "tri"], ["tri", 0]), ([], None))):
        path = tmp_path / ("cli%d.jsonl" % i)
        ber.main(common + extra + ["--log", str(path)])
        res = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
        assert res["points"][0]["frames"] == 256 and res["points"][0]["frame_errors"] == 0
        text = path.read_text()
        assert ('"interleave": %s' % json.dumps(key) in text) if key else ("interleave" not in text)
    with pytest.raises(SystemExit):
        ber.main(common + ["--interleave", "rect"])  # neither rows nor a modem to take them from
    capsys.readouterr()

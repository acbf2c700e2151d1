"""QCLayeredBPDecoder (ldpc_qc_bp.hip) against the NumPy restatement of its
definition (tests/qc_bp_ref.py).  Bar: hard decisions, iteration counts and fp64
posteriors array_equal, the posteriors by bit pattern (-0.0 is not +0.0),
everywhere.  Every condition on the inputs (frames that stop at different
iterations and frames that never stop, clamps that act) is asserted on the
restatement before the device is asked."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from qc_bp_ref import qc_bp_ref
from test_qc_bp_ref_host import awgn, random_base, same_bits

pytestmark = pytest.mark.gpu

B = 67


def _L():
    import polarcode_and_ldpc_amd.ldpc as L
    return L


def _N():
    from polarcode_and_ldpc_amd import _native
    return _native


def _rows_base(degrees, nb, Z, seed):
    """A base matrix whose block row i has degrees[i] non-zero blocks (random columns and shifts)."""
    rng = np.random.RandomState(seed)
    base = np.full((len(degrees), nb), -1, dtype=np.int64)
    for i, d in enumerate(degrees):
        base[i, np.sort(rng.choice(nb, d, replace=False))] = rng.randint(0, Z, d)
    return base


def _dec(base, Z, max_iter=20, early_stop=True, layer_order=None, clip=64.0):
    return _L().QCLayeredBPDecoder(np.array(base), Z, max_iter=max_iter, early_stop=early_stop, layer_order=layer_order,
                                   clip=clip)


def _ref(base, Z, L, max_iter=20, early_stop=True, layer_order=None, clip=64.0):
    cnt = {}
    r = qc_bp_ref(base, Z, L, max_iter, clip, early_stop, layer_order, clamps=cnt)
    for x in r:
        x.setflags(write=False)
    return r + (cnt,)


def _same(got, want):
    bits, its, post = (x.cpu().numpy() if isinstance(x, torch.Tensor) else x for x in got)
    assert np.array_equal(bits, want[0])
    assert np.array_equal(its, want[1])
    assert post.dtype == np.float64 and same_bits(post, want[2])


def _soft(dec, llr):
    return dec.decode_batch(llr, return_iterations=True, return_llr=True)


def _frozen(a):
    a.setflags(write=False)
    return a


def _cuda(a):
    return torch.from_numpy(np.array(a)).cuda()


# ---- lifting sizes ----------------------------------------------------------------------
ZS = {1: (64, 4), 7: (9, 4), 27: (2, 4), 64: (1, 4), 96: (1, 1)}  # Z: (frames per wavefront, wavefronts per workgroup)


@functools.lru_cache(maxsize=None)
def _z_base(Z):
    return _frozen(random_base(4, 8, Z, 3, seed=500 + Z))


@functools.lru_cache(maxsize=None)
def _z_llr(Z):
    """B frames of AWGN LLRs at -1 dB: at every Z some frames stop at once, some later, some never"""
    return _frozen(awgn(8 * Z, B, -1.0, seed=600 + Z))


@functools.lru_cache(maxsize=None)
def _z_want(Z, early_stop):
    return _ref(_z_base(Z), Z, _z_llr(Z), early_stop=early_stop)


@pytest.mark.parametrize("early_stop", [True, False])
@pytest.mark.parametrize("Z", sorted(ZS))
def test_lifting_sizes(gpu, Z, early_stop):
    """Z = 1, 7, 27, 64: 64, 9, 2 and 1 frames per wavefront (SUBWAVE, each frame stops on its own); 96:
    one workgroup per frame, its second wavefront half filled.  67 frames: more than one workgroup
    everywhere but at Z = 1, where they are one full wavefront and three frames of a second."""
    want = _z_want(Z, early_stop)
    if early_stop:
        print(Z, "restatement iterations:", np.bincount(want[1], minlength=21))
        assert len(np.unique(want[1][want[1] < 20])) >= 3, "the frames do not stop at different iterations"
        assert (want[1] == 20).any(), "every frame stops"
    else:
        assert (want[1] == 20).all() and not same_bits(want[2], _z_want(Z, True)[2])
    dec = _dec(_z_base(Z), Z, early_stop=early_stop)
    info = dec.plan.info
    assert info.reserved == 17 and info.frames_per_block == ZS[Z][0] * ZS[Z][1]
    _same(_soft(dec, _cuda(_z_llr(Z))), want)


# ---- row degrees x lifting size x state home: every compiled instance ----------------------
DEGREES = [(8, 3, 5), (12, 15, 9), (24, 32, 17), (40, 33, 2)]


@functools.lru_cache(maxsize=None)
def _deg_case(degrees, Z):
    base = _frozen(_rows_base(degrees, 48, Z, seed=700 + degrees[0] + Z))
    L = _frozen(awgn(48 * Z, 19, 4.0, seed=800 + degrees[0] + Z))  # dense rows: a high SNR keeps the messages moving
    return base, L, _ref(base, Z, L, max_iter=6)


@pytest.mark.parametrize("home", ["lds", "workspace"])
@pytest.mark.parametrize("Z", [7, 96])
@pytest.mark.parametrize("degrees", DEGREES, ids=lambda d: "deg%d" % max(d))
def test_row_degrees_and_state_homes(gpu, monkeypatch, degrees, Z, home):
    """Row degrees up to 8, 16, 32 and 40 on mixed rows, one of them of degree 2 (its inputs swap): the
    rule keeps no input in registers, so the four instances -- SUBWAVE (Z = 7) and block (Z = 96) mapping,
    state in LDS and (PL_LMS_GLOBAL=1) in the workspace -- serve them all.  19 frames, 6 iterations."""
    base, L, want = _deg_case(degrees, Z)
    assert want[1].max() == 6 and np.abs(want[2]).max() > np.abs(L).max()  # frames that run on, posteriors that grow
    if home == "workspace":
        monkeypatch.setenv("PL_LMS_GLOBAL", "1")
    dec = _dec(base, Z, max_iter=6)
    info = dec.plan.info
    assert info.reserved == (17 if home == "lds" else 18) and info.fused_top == 0
    state = ((8 * 48 * Z + 15) // 16 * 16 + 8 * Z * sum(degrees) + 15) // 16 * 16
    assert dec.plan.workspace_bytes(19) == (19 * state if home == "workspace" else 0)
    _same(_soft(dec, _cuda(L)), want)
    if home == "workspace":
        assert dec.plan.workspace_stats()[0] == 1
        dec.plan.release()
        assert dec.plan.workspace_stats() == (0, 0)


# ---- layer order, an empty block row ---------------------------------------------------------
@pytest.mark.parametrize("option", ["layer_order", "empty_row", "empty_row_and_order"])
def test_layer_order_and_an_empty_block_row(gpu, option):
    """The slots of R follow the stream: a permuted layer order moves them, a block row without blocks
    takes none and is skipped."""
    Z = 27
    base, L = np.array(_z_base(Z)), _z_llr(Z)
    kw = {}
    if option != "layer_order":
        base[1] = -1
    if option != "empty_row":
        kw["layer_order"] = [2, 0, 3, 1]
    want = _ref(base, Z, L, **kw)
    assert not same_bits(want[2], _z_want(Z, True)[2])  # the option shows in the posteriors
    assert want[1].min() < 20 and len(np.unique(want[1])) > 2
    _same(_soft(_dec(base, Z, **kw), _cuda(L)), want)


# ---- special inputs ---------------------------------------------------------------------------
@pytest.mark.parametrize("Z", [27, 96])
@pytest.mark.parametrize("early_stop", [True, False])
def test_special_inputs(gpu, Z, early_stop):
    """A NaN (an erasure), a +inf and a -inf (+-clip), an all-inf, an all -inf, an all-zero and an all-NaN
    frame among ordinary ones: every posterior finite and under 2 clip + ln 2, and equal to the
    restatement's."""
    base = _z_base(Z)
    L = np.array(_z_llr(Z)[:12])
    L[0, 3], L[1, 5], L[2, 7], L[3, :], L[4, :], L[5, :], L[6, :] = np.nan, np.inf, -np.inf, np.inf, 0.0, -np.inf, np.nan
    L[7, 2] = -0.0
    want = _ref(base, Z, L, early_stop=early_stop)
    assert np.isfinite(want[2]).all() and np.abs(want[2]).max() <= 128.0 + np.log(2.0)
    assert want[0][4].all() and not want[2][4].any() and want[0][6].all() and want[3]["llr"] >= 3 * 8 * Z + 3
    if early_stop:
        assert want[1][3] == 1 and not want[0][3].any()
    _same(_soft(_dec(base, Z, early_stop=early_stop), _cuda(L)), want)


def test_small_clip_where_the_clamp_acts(gpu):
    """clip = 4.0 at -1 dB: the load and the messages are clamped (counted in the restatement), the
    posteriors stay under 8 + ln 2."""
    Z = 27
    base, L = _z_base(Z), _z_llr(Z)
    want = _ref(base, Z, L, clip=4.0)
    print("clamps:", want[3], "iterations:", np.bincount(want[1], minlength=21))
    assert want[3]["llr"] > 0 and want[3]["q"] > 0 and 4.0 < np.abs(want[2]).max() <= 8.0 + np.log(2.0)
    assert not same_bits(want[2], _z_want(Z, True)[2])
    _same(_soft(_dec(base, Z, clip=4.0), _cuda(L)), want)


# ---- API edges ------------------------------------------------------------------------------
def test_max_iter_0_and_batch_0(gpu):
    Z = 27
    base, L = _z_base(Z), np.array(_z_llr(Z)[:9])
    L[0, :3] = [np.nan, np.inf, -200.0]
    want = _ref(base, Z, L, max_iter=0)
    assert want[1].max() == 0 and want[2][0, :3].tolist() == [0.0, 64.0, -64.0]  # the load clamps, nothing else
    assert np.array_equal(want[2][1:], L[1:])
    dec = _dec(base, Z, max_iter=0)
    _same(_soft(dec, _cuda(L)), want)
    # a degree-1 row is no obstacle when no check is evaluated
    one = np.array(base)
    one[0] = -1
    one[0, 3] = 5
    _same(_soft(_dec(one, Z, max_iter=0), _cuda(L)), want)
    with pytest.raises(ValueError, match="degree-1"):
        _dec(one, Z).decode_batch(_cuda(L))
    # batch 0, device and host
    dec = _dec(base, Z)
    bits, its, post = _soft(dec, torch.empty((0, 8 * Z), dtype=torch.float64, device="cuda"))
    assert bits.shape == (0, 8 * Z) and its.shape == (0,) and post.shape == (0, 8 * Z) and bits.is_cuda
    bits, its, post = _soft(dec, np.zeros((0, 8 * Z)))
    assert bits.shape == (0, 8 * Z) and its.shape == (0,) and post.shape == (0, 8 * Z)
    N = _N()
    assert N.lib.pl_decode(dec.plan.handle, None, 0, 8 * Z, None, None, None) == N.PL_OK


def test_strided_llr_and_pitched_out(gpu):
    """A strided llr view is decoded as it is (any row pitch, unit inner stride); `out=` receives the bits;
    a column-strided view goes through one contiguous copy."""
    Z = 7
    base, L = _z_base(Z), _z_llr(Z)
    want = _z_want(Z, True)
    dec = _dec(base, Z)
    n = 8 * Z
    for pitch, off in ((n + 3, 1), (64, 0)):
        buf = torch.full((B * pitch + off,), 99.0, dtype=torch.float64, device="cuda")
        view = buf[off:off + B * pitch].view(B, pitch)[:, :n]
        view.copy_(_cuda(L))
        assert view.stride(0) == pitch and not view.is_contiguous()
        out = torch.full((B, n), 7, dtype=torch.uint8, device="cuda")
        bits, its, post = dec.decode_batch(view, out=out, return_iterations=True, return_llr=True)
        assert bits is out
        _same((bits, its, post), want)
        assert bool((buf.view(-1)[off:off + B * pitch].view(B, pitch)[:, n:] == 99.0).all())
    wide = torch.zeros((B, 2 * n), dtype=torch.float64, device="cuda")
    wide[:, ::2] = _cuda(L)
    _same(_soft(dec, wide[:, ::2]), want)
    # the C-ABI with a pitch on the posteriors: pl_ldpc_decode_soft, ld_post > n
    N = _N()
    P = ctypes.c_void_p
    llr = _cuda(L)
    bits = torch.empty((B, n), dtype=torch.uint8, device="cuda")
    its = torch.empty((B,), dtype=torch.int32, device="cuda")
    post = torch.full((B, n + 5), 99.0, dtype=torch.float64, device="cuda")
    assert N.lib.pl_ldpc_decode_soft(dec.plan.handle, P(llr.data_ptr()), B, n, P(bits.data_ptr()), P(its.data_ptr()),
                                     P(post.data_ptr()), n + 5, None) == N.PL_OK
    torch.cuda.synchronize()
    _same((bits, its, post[:, :n].contiguous()), want)
    assert bool((post[:, n:] == 99.0).all())
    # fp32 and int8 LLRs are not this plan's
    f32 = torch.zeros((3, n), dtype=torch.float32, device="cuda")
    assert N.lib.pl_ldpc_decode_f32(dec.plan.handle, P(f32.data_ptr()), 3, n, P(bits.data_ptr()), None, None, 0, None,
                                    0, None) == N.PL_EUNSUPPORTED
    assert N.lib.pl_ldpc_decode_i8(dec.plan.handle, P(f32.data_ptr()), 3, n, P(bits.data_ptr()), None, None, 0, None,
                                   0, None) == N.PL_EUNSUPPORTED


def test_numpy_and_cuda_and_the_return_forms(gpu):
    """NumPy in gives NumPy out (int64 bits and iterations, float64 posteriors), CUDA tensors in give CUDA
    tensors out; return_llr with and without return_iterations; decode() of one frame."""
    Z = 27
    base, L = _z_base(Z), _z_llr(Z)
    want = _z_want(Z, True)
    dec = _dec(base, Z)
    got = _soft(dec, np.array(L))
    assert all(isinstance(x, np.ndarray) for x in got) and got[0].dtype == np.int64 and got[1].dtype == np.int64
    _same(got, want)
    got = _soft(dec, _cuda(L))
    assert all(isinstance(x, torch.Tensor) and x.is_cuda for x in got)
    assert got[0].dtype == torch.uint8 and got[1].dtype == torch.int32 and got[2].dtype == torch.float64
    _same(got, want)
    bits, post = dec.decode_batch(_cuda(L), return_llr=True)
    assert torch.equal(bits, got[0]) and torch.equal(post, got[2])
    bits, its = dec.decode_batch(_cuda(L), return_iterations=True)
    assert torch.equal(bits, got[0]) and torch.equal(its, got[1])
    assert torch.equal(dec.decode_batch(_cuda(L)), got[0])
    out = np.zeros((B, 8 * Z), dtype=np.int64)
    assert dec.decode_batch(np.array(L), out=out) is out and np.array_equal(out, want[0])
    # fp32 LLRs widen exactly: the restatement sees the same values
    L32 = np.array(L).astype(np.float32)
    _same(_soft(dec, torch.from_numpy(L32).cuda()), _ref(base, Z, L32.astype(np.float64)))
    b1, i1 = dec.decode(np.array(L[0]), return_iterations=True)
    assert np.array_equal(b1, want[0][0]) and i1 == want[1][0]
    assert np.array_equal(dec.decode(np.array(L[0])), want[0][0])
    assert dec.plan.info.reserved == 17 and dec.plan.info.n_in == 8 * Z


# ---- a larger code ----------------------------------------------------------------------------
def test_the_harness_code_12_24_81(gpu):
    """ber.py's default quasi-cyclic code (--qc 12,24,81,3,1) at 64 frames: n = 1944, one workgroup of
    128 threads a frame, P and R (8 n + 8 Z blocks bytes) in LDS."""
    from test_ldpc_qc_bp_host import probe
    Lib = _L()
    Z = 81
    base = Lib.qc_encodable_base(12, 24, Z, 3, 1)
    blocks = int((base >= 0).sum())
    rc, p, msg = probe(base, Z)
    assert rc == 0, msg
    state = (8 * 24 * Z + 8 * Z * blocks + 15) // 16 * 16  # 8 n = 15 552 is a multiple of 16
    assert p.state_bytes == state and state + 128 <= 160 * 1024 and p.use_global == 0 and p.kernel == 17
    assert (p.fpw, p.fpb, p.threads, p.lds_bytes) == (1, 1, 128, state + 128)
    L = awgn(24 * Z, 64, 0.5, seed=81)
    want = _ref(base, Z, L)
    print("restatement iterations:", np.bincount(want[1], minlength=21))
    assert len(np.unique(want[1])) >= 3
    dec = _dec(base, Z)
    assert dec.plan.info.reserved == 17 and dec.plan.info.lds_bytes == p.lds_bytes
    _same(_soft(dec, _cuda(L)), want)


# ---- the harness ------------------------------------------------------------------------------
def test_simulate_qc_ldpc_bp_equals_the_chain_built_by_hand(gpu, tmp_path):
    """simulate_qc_ldpc(algo="bp") with an encoder, a rate matcher and a log-MAP 64-QAM modem: its counts
    are those of the same chain assembled from the public classes on the same seed; the run key carries
    algo and clip, and without algo= nothing is added to it."""
    import json
    from polarcode_and_ldpc_amd.channel.qam import QAMModem
    from polarcode_and_ldpc_amd.harness import ber
    from polarcode_and_ldpc_amd.harness.montecarlo import MonteCarlo, ldpc_round_fn
    Lib = _L()
    Z = 27
    base = Lib.qc_encodable_base(8, 12, Z, 3, 2, core=4, chained=False)
    snr, nfr = [6.0, 9.0, 12.0], 512  # Es/N0 per 64-QAM symbol at rate 0.39: from most frames lost to few
    kw = dict(max_iter=20, batch=256, seed=5, random_codewords=True, rate_match=(264, 2, 5))
    log = tmp_path / "points.jsonl"
    _, _, got = ber.simulate_qc_ldpc(snr, nfr, 10 ** 9, base, Z, algo="bp", clip=32.0,
                                     modulation=QAMModem(6, demapper="logmap"), log_path=str(log), **kw)
    rm = Lib.QCRateMatcher(base, Z, 264, 2, 5)
    dec = Lib.QCLayeredBPDecoder(rm.decoder_base(), Z, max_iter=20, early_stop=True, clip=32.0)
    mc = MonteCarlo(ldpc_round_fn(dec, seed=5, encoder=Lib.QCLDPCEncoder(base, Z), rate_matcher=rm,
                                  modulation=QAMModem(6, demapper="logmap")),
                    info_bits=rm.k - rm.fillers, batch=256, device=torch.device("cuda", 0))
    hand = mc.run(snr, nfr, 10 ** 9)
    counts = [(p.frame_errors, p.bit_errors, p.frames) for p in got]
    print("bp:", counts)
    assert counts == [(p.frame_errors, p.bit_errors, p.frames) for p in hand]
    assert [c[2] for c in counts] == [nfr] * 3 and counts[0][0] > counts[2][0] >= 0  # the counters are not trivial
    rows = [json.loads(l) for l in log.read_text().splitlines() if l.strip()]
    assert len(rows) == 3 and all(r["key"]["algo"] == "bp" and r["key"]["clip"] == 32.0 for r in rows)
    assert rows[0]["key"]["dtype"] == "float64"
    # the default is min-sum: the same call without algo= is the call it was
    _, _, ms = ber.simulate_qc_ldpc(snr, nfr, 10 ** 9, base, Z, normalization=0.75,
                                    modulation=QAMModem(6, demapper="logmap"), log_path=str(log), **kw)
    _, _, ms2 = ber.simulate_qc_ldpc(snr, nfr, 10 ** 9, base, Z, normalization=0.75, algo="minsum", clip=3.0,
                                     modulation=QAMModem(6, demapper="logmap"), **kw)
    rows = [json.loads(l) for l in log.read_text().splitlines() if l.strip()]
    assert len(rows) == 6 and all("algo" not in r["key"] and "clip" not in r["key"] for r in rows[3:])
    assert [(p.frame_errors, p.bit_errors) for p in ms] == [(p.frame_errors, p.bit_errors) for p in ms2]
    assert [(p.frame_errors, p.bit_errors) for p in ms] != [c[:2] for c in counts]
    with pytest.raises(ValueError):
        ber.simulate_qc_ldpc(snr, nfr, 10 ** 9, base, Z, algo="bp", fixed=(4.0, 31, 31), **kw)
    with pytest.raises(ValueError):
        ber.simulate_qc_ldpc(snr, nfr, 10 ** 9, base, Z, algo="spa", **kw)


# ---- the error rate ---------------------------------------------------------------------------
def test_fewer_frame_errors_than_unnormalised_min_sum_at_rate_one_sixth(gpu):
    """The rate-1/6 chain of DESIGN.md 4.4e (--qc 12,24,81,3,1 --rm 5832,0,0, 64-QAM with the log-MAP
    demapper, rect interleaver, random codewords, 20 iterations, seed 0) at Es/N0 = 2 dB, where on 131 072
    frames sum-product lost 726 frames, min-sum at normalisation 1.0 lost 2 403 and at 0.75 lost 5 831
    (DESIGN.md 4.3g).  On the first 8 192 of those frames sum-product must lose strictly fewer than
    un-normalised min-sum: about 45 against 150 expected."""
    from polarcode_and_ldpc_amd.channel.qam import QAMModem
    from polarcode_and_ldpc_amd.harness import ber
    base = _L().qc_encodable_base(12, 24, 81, 3, 1)
    kw = dict(max_iter=20, batch=8192, seed=0, random_codewords=True, rate_match=(5832, 0, 0),
              interleaver=("rect", None))
    _, _, bp = ber.simulate_qc_ldpc([2.0], 8192, 10 ** 9, base, 81, algo="bp",
                                    modulation=QAMModem(6, demapper="logmap"), **kw)
    _, _, ms = ber.simulate_qc_ldpc([2.0], 8192, 10 ** 9, base, 81, normalization=1.0,
                                    modulation=QAMModem(6, demapper="logmap"), **kw)
    print("frame errors of 8192: bp", bp[0].frame_errors, "min-sum 1.0", ms[0].frame_errors)
    assert bp[0].frames == ms[0].frames == 8192
    assert bp[0].frame_errors < ms[0].frame_errors

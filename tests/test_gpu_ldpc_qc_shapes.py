"""QCLayeredMSDecoder (ldpc_qc_layered.hip), both precisions, against the base-matrix
restatement (tests/qc_layered_ref.py) at the lifting sizes, planner edges and
meta-word packing edges at which the kernel takes another path.  Bar: hard
decisions and iteration counts array_equal, posteriors array_equal with
equal_nan.  Every condition on the inputs is asserted on the restatement before
the device is asked."""
import ctypes
import functools

import numpy as np
import pytest

from qc_layered_ref import block_row_vars, qc_layered_ms_ref

pytestmark = pytest.mark.gpu

DTYPES = [np.float64, np.float32]
LDS_MAX = 160 * 1024


def _L():
    import polarcode_and_ldpc_amd.ldpc as L
    return L


def _N():
    from polarcode_and_ldpc_amd import _native
    return _native


def _awgn(n, frames, snr_db, seed):
    """All-zero codeword over BPSK + AWGN, LLR = 2 y / sigma^2."""
    rng = np.random.RandomState(seed)
    sigma = np.sqrt(1.0 / (2.0 * 10.0 ** (snr_db / 10.0)))
    return 2.0 * (1.0 + sigma * rng.randn(frames, n)) / sigma ** 2


def _rows_base(degrees, nb, Z, seed):
    """A base matrix whose block row i has degrees[i] non-zero blocks (random columns and shifts)."""
    rng = np.random.RandomState(seed)
    base = np.full((len(degrees), nb), -1, dtype=np.int64)
    for i, d in enumerate(degrees):
        base[i, np.sort(rng.choice(nb, d, replace=False))] = rng.randint(0, Z, d)
    return base


def _probe(base, Z, dtype, max_iter=20):
    N = _N()
    sh = np.ascontiguousarray(base, np.int32)
    out = N.LdpcQcPlanProbe()
    args = (sh.shape[0], sh.shape[1], Z, sh.ctypes.data_as(ctypes.c_void_p), None, max_iter, 1, 0.75, 0)
    if dtype == np.float32:
        rc = N.lib.pl_debug_ldpc_qc_plan_probe_flags(*args, N.PL_LDPC_QC_F32, ctypes.byref(out))
    else:
        rc = N.lib.pl_debug_ldpc_qc_plan_probe(*args, ctypes.byref(out))
    assert rc == 0, N.lib.pl_last_error()
    return out


def _dec(base, Z, dtype, **kw):
    return _L().QCLayeredMSDecoder(np.array(base), Z, dtype=dtype, **kw)


def _same(got, want, dtype):
    bits, its, post = got
    assert np.array_equal(bits, want[0])
    assert np.array_equal(its, want[1])
    assert post.dtype == dtype and want[2].dtype == dtype
    assert np.array_equal(post, want[2], equal_nan=True)


def _soft(dec, llr):
    return dec.decode_batch(np.array(llr), return_iterations=True, return_llr=True)


# ---- a. lifting sizes ----------------------------------------------------------------
# Z: frames per workgroup (fpw x fpb) of the (4, 8) plan, the same in both precisions
FPG = {2: 128, 3: 84, 32: 8, 33: 4, 63: 4, 65: 1, 128: 1, 384: 1, 1000: 1, 1024: 1}
SNR_HI, SNR_LO = -1.0, -5.0  # even frames converge within 20 iterations, odd frames (almost) never do


@functools.lru_cache(maxsize=None)
def _z_base(Z):
    b = _L().qc_random_base(4, 8, Z, 3, seed=100 + Z + 8)
    b.setflags(write=False)
    return b


@functools.lru_cache(maxsize=None)
def _z_pool(Z):
    """fpg + 1 frames (one workgroup and one frame more); 16, or 9 at Z >= 384, for one frame per
    workgroup.  Even frames at -1 dB, odd frames at -5 dB."""
    fpg = FPG[Z]
    frames = fpg + 1 if fpg > 1 else (9 if Z >= 384 else 16)
    llr = np.empty((frames, 8 * Z))
    llr[0::2] = _awgn(8 * Z, (frames + 1) // 2, SNR_HI, seed=1000 + Z)
    llr[1::2] = _awgn(8 * Z, frames // 2, SNR_LO, seed=2000 + Z)
    if Z > 64:
        llr[-1] = _stuck_frame(_z_base(Z), Z)[0]
    llr.setflags(write=False)
    return llr


def _stuck_frame(base, Z):
    """(frame, r): every LLR +8 but one of -1e9, at the variable whose three checks have the largest
    smallest index r within their block rows.  What its checks return to it in 20 iterations stays far
    below 1e9, so the frame never stops, and after the first iteration its only unsatisfied checks
    are those three, at index r or above -- an early-stop vote that misses the word of a later
    wavefront stops it there."""
    best = (-1, None)
    for j in range(base.shape[1]):
        rows = np.nonzero(base[:, j] >= 0)[0]
        for c in range(Z):
            r = min((c - base[i, j]) % Z for i in rows)  # check r of block row i reads j Z + (r + s) % Z
            best = max(best, (int(r), j * Z + c))
    frame = np.full(base.shape[1] * Z, 8.0)
    frame[best[1]] = -1e9
    return frame, best[0]


@functools.lru_cache(maxsize=None)
def _z_want(Z, dtype, early_stop):
    r = qc_layered_ms_ref(_z_base(Z), Z, _z_pool(Z), 20, 0.75, early_stop, dtype=dtype)
    for x in r:
        x.setflags(write=False)
    return r


@pytest.mark.parametrize("early_stop", [True, False])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Z", sorted(FPG))
def test_lifting_sizes(gpu, Z, dtype, early_stop):
    """Z = 2, 3: 32 and 21 frames per wavefront, the stop mask shifted by up to 62 bits; 32: the second
    frame's mask in bits 32..63; 33, 63: fpw == 1 with idle lanes of lane / z == 1; 65: a second
    wavefront with one working lane; 128: two full wavefronts; 384: six; 1000, 1024: all 16 vote words."""
    fpg = FPG[Z]
    llr, want = _z_pool(Z), _z_want(Z, dtype, early_stop)
    if early_stop:
        its = want[1]
        print(Z, dtype.__name__, "restatement iterations:", np.bincount(its, minlength=21))
        if fpg > 1:
            assert len(set(its[:fpg + 1].tolist())) > 1
            if Z <= 32:  # several frames per wavefront: they differ within the first wavefront too
                assert len(set(its[:64 // Z].tolist())) > 1
        for B in sorted({max(fpg - 1, 2), fpg + 1, len(llr)}):
            assert its[:B].min() < 20 and its[:B].max() == 20
        if Z > 64:  # the last frame never stops; at Z >= 384 its unsatisfied checks lie past the fourth wavefront
            assert its[-1] == 20
        if Z >= 384:
            assert _stuck_frame(_z_base(Z), Z)[1] >= 256
            first = qc_layered_ms_ref(_z_base(Z), Z, llr[-1:], 1, 0.75, False, dtype=dtype)
            assert first[0].sum() == 1  # after iteration 1 that variable alone is wrong: its three checks only
    else:
        assert (want[1] == 20).all()
    dec = _dec(_z_base(Z), Z, dtype, max_iter=20, normalization=0.75, early_stop=early_stop)
    info = dec.plan.info
    p = _probe(_z_base(Z), Z, dtype)
    assert info.reserved == (13 if dtype == np.float32 else 11) and p.use_global == 0
    assert info.frames_per_block == fpg == p.fpw * p.fpb and p.fpw == (64 // Z if Z <= 64 else 1)
    assert p.threads == (64 * p.fpb if Z <= 64 else (Z + 63) // 64 * 64) and p.lds_bytes <= LDS_MAX
    if Z == 1024 and dtype == np.float64:
        assert p.state_bytes == 147456  # the largest LDS-resident (4, 8) plan
    for B in sorted({1, max(fpg - 1, 1), fpg + 1, len(llr)}):
        _same(_soft(dec, llr[:B]), [w[:B] for w in want], dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_z1024_dcap32(gpu, dtype):
    """Row degrees [12, 24, 3, 32] at Z = 1024: the 32-register q[] instance at 1024 threads.  The
    state (8 n + 24 m, or 4 n + 16 m, bytes) exceeds the LDS, so it lives in the workspace."""
    Z = 1024
    base = _rows_base([12, 24, 3, 32], 32, Z, seed=24)
    p = _probe(base, Z, dtype, max_iter=5)
    assert (p.dcap, p.mw, p.threads, p.use_global, p.fpw, p.fpb) == (32, 2, 1024, 1, 1, 1)
    assert p.state_bytes == (196608 if dtype == np.float32 else 360448) and p.lds_bytes == 128
    llr = np.concatenate([_awgn(32 * Z, 1, 10.0, seed=40), _awgn(32 * Z, 1, 3.0, seed=41), _awgn(32 * Z, 1, -5.0, seed=42)])
    want = qc_layered_ms_ref(base, Z, llr, 5, 0.75, True, dtype=dtype)
    print("restatement iterations:", want[1])
    assert want[1].min() < 5 and want[1].max() == 5
    dec = _dec(base, Z, dtype, max_iter=5, normalization=0.75)
    assert dec.plan.info.reserved == (14 if dtype == np.float32 else 12)
    _same(_soft(dec, llr), want, dtype)


# ---- b. LDS / workspace edge ---------------------------------------------------------
# (mb, nb, Z) of the largest plan that keeps the state in LDS and its neighbour, the smallest that moves
# it to the workspace: one step in Z (block mapping: state + 128 vote bytes <= 160 KB) or in nb (sub-wave
# mapping: state x fpw <= 160 KB).  (dtype, LDS side, workspace side, LDS bytes of the LDS side, blocks per
# block column of the random base: few enough that no row has more than 16)
EDGES = {
    "f64_block": (np.float64, (5, 10, 909), (5, 10, 910), 163760, 3),
    "f32_block": (np.float32, (8, 16, 1023), (8, 16, 1024), 163808, 3),
    "f64_subwave": (np.float64, (64, 160, 32), (64, 161, 32), 163840, 3),
    "f32_subwave": (np.float32, (64, 448, 32), (64, 449, 32), 163840, 1),
}


@pytest.mark.parametrize("side", ["lds", "workspace"])
@pytest.mark.parametrize("edge", sorted(EDGES))
def test_lds_workspace_edge(gpu, edge, side):
    dtype, lds_shape, ws_shape, lds_bytes, dv = EDGES[edge]
    mb, nb, Z = lds_shape if side == "lds" else ws_shape
    base = _L().qc_random_base(mb, nb, Z, dv, seed=7)
    assert (base >= 0).sum(axis=1).max() <= 16  # one meta word: 8 n + 20 m, or 4 n + 12 m, bytes of state
    p = _probe(base, Z, dtype, max_iter=3)
    elem = 4 if dtype == np.float32 else 8
    a16 = lambda b: (b + 15) // 16 * 16  # noqa: E731
    assert p.state_bytes == a16(a16(elem * nb * Z) + (2 * elem + 4) * mb * Z) and p.mw == 1
    if side == "lds":
        assert p.use_global == 0 and p.lds_bytes == lds_bytes <= LDS_MAX
    else:
        assert p.use_global == 1 and p.lds_bytes == (0 if Z <= 64 else 128)
        assert p.state_bytes * p.fpw + (0 if Z <= 64 else 128) > LDS_MAX
    llr = np.concatenate([_awgn(nb * Z, 2, 2.0, seed=51), _awgn(nb * Z, 1, -5.0, seed=52)])
    want = qc_layered_ms_ref(base, Z, llr, 3, 0.75, True, dtype=dtype)
    dec = _dec(base, Z, dtype, max_iter=3, normalization=0.75)
    assert dec.plan.info.reserved == {(np.float64, "lds"): 11, (np.float64, "workspace"): 12,
                                      (np.float32, "lds"): 13, (np.float32, "workspace"): 14}[(dtype, side)]
    _same(_soft(dec, llr), want, dtype)


# ---- c. packing edges ----------------------------------------------------------------
# name: (row degrees, widest first so that iteration 1 sees the crafted inputs untouched; nb; Z; max_iter;
#        noisy frames; dcap; mw)
PACK = {
    "deg8": ([8, 5, 3], 12, 7, 8, 4, 8, 1),       # the ceiling of the 8-register instance
    "deg16": ([16, 9, 4], 20, 7, 8, 4, 16, 1),    # one-word packing full: idx1 / nidx 15, flags in bits 16..31
    "deg65": ([65, 64, 33], 70, 7, 8, 4, 0, 4),   # the sign words' boundaries in the two-pass form
    "deg2047": ([2047, 40], 2047, 2, 3, 2, 0, 65),  # the largest degree accepted: idx1 / nidx use all 11 bits
}


@functools.lru_cache(maxsize=None)
def _pack_case(name):
    degrees, nb, Z, max_iter, noisy, dcap, mw = PACK[name]
    base = _rows_base(degrees, nb, Z, seed=len(name) + degrees[0])
    n = nb * Z
    V = block_row_vars(base, Z, 0)
    d = V.shape[1]
    assert d == max(degrees) == degrees[0]
    last, last2 = V[:, d - 1], V[:, d - 2]  # the last (two) inputs of every check of the widest row
    llr = _awgn(n, noisy + 4, 2.0, seed=61)
    c = llr[noisy:]
    rng = np.random.RandomState(62)
    # (i) the smallest |LLR| of every check of the widest row at its last input, either sign
    c[0, last] = 0.25 * np.abs(c[0]).min() * rng.choice([-1.0, 1.0], Z) * (1.0 + np.arange(Z)) / Z
    assert (np.abs(c[0][V]).argmin(axis=1) == d - 1).all()
    c[1, last] = np.nan      # (ii) a single NaN, at the last input
    c[2, last] = 0.0         # (iii) a single exact zero, at the last input
    c[3, last] = 0.0         # (iv) two zeros, at the last two inputs
    c[3, last2] = -0.0
    assert (np.isnan(c[1][V]).sum(axis=1) == 1).all() and np.isnan(c[1][V][:, d - 1]).all()
    assert ((c[2][V] == 0).sum(axis=1) == 1).all() and ((c[3][V] == 0).sum(axis=1) == 2).all()
    base.setflags(write=False)
    llr.setflags(write=False)
    return base, Z, max_iter, llr, dcap, mw


@functools.lru_cache(maxsize=None)
def _pack_want(name, dtype, early_stop):
    base, Z, max_iter, llr, _, _ = _pack_case(name)
    return qc_layered_ms_ref(base, Z, llr, max_iter, 0.75, early_stop, dtype=dtype)


@pytest.mark.parametrize("early_stop", [True, False])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", sorted(PACK))
def test_packing_edges(gpu, name, dtype, early_stop):
    base, Z, max_iter, llr, dcap, mw = _pack_case(name)
    p = _probe(base, Z, dtype, max_iter=max_iter)
    assert (p.dcap, p.mw, p.maxdc) == (dcap, mw, PACK[name][0][0])
    want = _pack_want(name, dtype, early_stop)
    if not early_stop:
        assert np.isnan(want[2][-3]).any()
    dec = _dec(base, Z, dtype, max_iter=max_iter, normalization=0.75, early_stop=early_stop)
    _same(_soft(dec, llr), want, dtype)


# ---- d. rate-matched frames ----------------------------------------------------------
# name: frames; the bases are the NR-like ones of tests/test_ldpc_qc_encode_host.py and one more
# of the same builder at the largest 5G lifting size
RATE = {"z7_core4_nr": 32, "z65_core4_nr": 16, "z384_core4_nr": 8}


@functools.lru_cache(maxsize=None)
def _rate_case(name):
    """Codewords of QCLDPCEncoder over BPSK + AWGN, even frames at 3 dB and odd frames at -3 dB; then the
    first two block columns punctured (exact 0.0) and the last Z // 2 + 3 information positions, zero
    filler bits in the message, known (+inf).  Found on the restatement, in both precisions: the even
    frames stop within 1..6 iterations on the codeword sent, most odd frames run to max_iter (a few
    stop late, or on another codeword); every frame has +inf posteriors
    at the filler positions and none ever has a NaN posterior (the infinities are all +inf and no check
    has all but one input infinite, so inf - inf does not occur), with or without early stop."""
    if name == "z384_core4_nr":
        base, Z = _L().qc_encodable_base(6, 10, 384, 3, 3, core=4, chained=False), 384
    else:
        from test_ldpc_qc_encode_host import base_of
        base, Z = base_of(name)
    frames = RATE[name]
    mb, nb = base.shape
    kb, fill = nb - mb, Z // 2 + 3
    rng = np.random.RandomState(70 + Z)
    msg = rng.randint(0, 2, (frames, kb * Z)).astype(np.uint8)
    msg[:, kb * Z - fill:] = 0
    cw = np.asarray(_L().QCLDPCEncoder(np.array(base), Z).encode_batch(msg)).astype(np.float64)
    assert (cw[:, :kb * Z] == msg).all()  # systematic: the filler positions are codeword positions
    sigma = np.sqrt(1.0 / (2.0 * 10.0 ** (np.where(np.arange(frames) % 2 == 0, 3.0, -3.0) / 10.0)))[:, None]
    llr = 2.0 * ((1.0 - 2.0 * cw) + sigma * rng.randn(frames, nb * Z)) / sigma ** 2
    llr[:, :2 * Z] = 0.0
    llr[:, kb * Z - fill:kb * Z] = np.inf
    llr.setflags(write=False)
    return np.array(base), Z, llr, cw.astype(np.int64)


@pytest.mark.parametrize("early_stop", [True, False])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", sorted(RATE))
def test_rate_matched_frames(gpu, name, dtype, early_stop):
    base, Z, llr, cw = _rate_case(name)
    # every check of iteration 1 that reads both punctured block columns has two zero inputs
    both = [i for i in range(base.shape[0]) if base[i, 0] >= 0 and base[i, 1] >= 0]
    assert both
    want = qc_layered_ms_ref(base, Z, llr, 20, 0.75, early_stop, dtype=dtype)
    print(name, dtype.__name__, "restatement iterations:", np.bincount(want[1], minlength=21))
    if early_stop:
        assert want[1].min() < 20 and want[1].max() == 20
        assert (want[1][0::2] < 20).all() and (want[0][0::2] == cw[0::2]).all()  # 3 dB: the codewords sent
    assert np.isposinf(want[2]).any(axis=1).all() and not np.isnan(want[2]).any()
    dec = _dec(base, Z, dtype, max_iter=20, normalization=0.75, early_stop=early_stop)
    _same(_soft(dec, llr), want, dtype)

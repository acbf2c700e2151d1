"""QCLayeredMSDecoder(dtype=np.float32) -- the single-precision instances of
qc_frame_kernel, PL_LDPC_QC_F32 -- against the NumPy float32 restatement of the
layered definition (tests/layered_ref32.py) on the expanded H with the block
rows as layers.  Bar everywhere: hard decisions and iteration counts
array_equal, posteriors array_equal with equal_nan and dtype float32.

The shapes are tests/test_gpu_ldpc_qc.py's, each the smallest at which its
mapping can go wrong: Z = 1 (64 frames per wavefront), 7 (9 frames and one idle
lane), 27 (2 frames, 10 idle lanes), 64 (exactly one wavefront), 96 (two
wavefronts, 32 idle lanes, workgroup barrier)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from layered_ref import awgn_llrs, layered_ms_ref
from layered_ref32 import layered_ms_literal32, layered_ms_ref32, to_f32

pytestmark = pytest.mark.gpu

FRAMES = 67
SNR = -1.0
F32 = np.float32
FLT_MIN = np.finfo(np.float32).tiny


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


@functools.lru_cache(maxsize=None)
def _base(name):
    L = _L()
    if isinstance(name, int):  # the (4, 8) code of that Z
        b = L.qc_random_base(4, 8, name, 3, seed=100 + name + 8)
    elif name == "deg40":  # every block row of degree 40: the two-pass instance, three meta words
        b = L.qc_random_base(3, 40, 7, 3, seed=147)
        assert ((b >= 0).sum(axis=1) == 40).all()
    elif name == "deg12":  # largest degree in 9..16: the 16-input instance, one meta word
        b = _rows_base([12, 5, 9], 20, 7, seed=12)
    elif name == "deg24":  # rows of degree 9..16 and 17..32: the 32-input instance, two meta words
        b = _rows_base([12, 24, 3, 32], 32, 7, seed=24)
    else:
        raise KeyError(name)
    b.setflags(write=False)
    return b


def _Z(name):
    return name if isinstance(name, int) else 7


@functools.lru_cache(maxsize=None)
def _H(name):
    H = _L().qc_expand(_base(name), _Z(name))
    H.setflags(write=False)
    return H


def _layers(name):
    return _L().qc_block_layers(_base(name).shape[0], _Z(name))


@functools.lru_cache(maxsize=None)
def _llr(name, frames=FRAMES, snr=SNR, seed=1234):
    a = awgn_llrs(_base(name).shape[1] * _Z(name), frames, snr, seed=seed)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _want(name, norm, early_stop, max_iter, frames=FRAMES, snr=SNR, seed=1234):
    """The float32 restatement's (bits, iterations, posterior) with the block rows as layers; shared, read-only."""
    r = layered_ms_ref32(_H(name), _llr(name, frames, snr, seed), _layers(name), max_iter, norm, early_stop)
    for x in r:
        x.setflags(write=False)
    return r


def _dec(name, **kw):
    return _L().QCLayeredMSDecoder(np.array(_base(name)), _Z(name), dtype=np.float32, **kw)


def _same(got, want):
    bits, its, post = got
    assert np.array_equal(bits, want[0])
    assert np.array_equal(its, want[1])
    assert post.dtype == np.float32 and want[2].dtype == np.float32
    assert np.array_equal(post, want[2], equal_nan=True)


def _soft(dec, llr):
    return dec.decode_batch(np.array(llr), return_iterations=True, return_llr=True)


def _host(t):
    return [x.cpu().numpy() for x in t]


def _probe(name, flags, lms_global=0, max_iter=8):
    N = _N()
    sh = np.ascontiguousarray(_base(name), np.int32)
    out = N.LdpcQcPlanProbe()
    assert N.lib.pl_debug_ldpc_qc_plan_probe_flags(sh.shape[0], sh.shape[1], _Z(name),
                                                   sh.ctypes.data_as(ctypes.c_void_p), None, max_iter, 1, 0.75,
                                                   lms_global, flags, ctypes.byref(out)) == 0, N.lib.pl_last_error()
    return out


def _state_bytes(name):
    """4 n + 8 m + 4 mw m, each part on a 16-byte boundary (include/polarldpc.h)."""
    base, Z = _base(name), _Z(name)
    m, n = base.shape[0] * Z, base.shape[1] * Z
    maxdc = int((base >= 0).sum(axis=1).max())
    mw = 1 if maxdc <= 16 else 1 + (maxdc + 31) // 32
    a16 = lambda b: (b + 15) // 16 * 16  # noqa: E731
    return a16(a16(4 * n) + 8 * m + 4 * m * mw)


# ---- 1. against the restatement ------------------------------------------------
@pytest.mark.parametrize("max_iter", [20, 1])
@pytest.mark.parametrize("early_stop", [True, False])
@pytest.mark.parametrize("norm", [1.0, 0.75])
@pytest.mark.parametrize("Z", [7, 27, 64, 96])
def test_against_restatement(gpu, Z, norm, early_stop, max_iter):
    want = _want(Z, norm, early_stop, max_iter)
    if early_stop and max_iter == 20 and norm == 0.75:
        print(Z, norm, "float32 restatement iterations:", np.bincount(want[1], minlength=21))
        assert want[1].min() <= 3 and (want[1] == 20).any()
    # a decoder that runs in fp64 and rounds its posteriors at the end does not pass: the two differ
    w64 = layered_ms_ref(_H(Z), _llr(Z), _layers(Z), max_iter, norm, early_stop)[2].astype(F32)
    differ = int((~((w64 == want[2]) | (np.isnan(w64) & np.isnan(want[2])))).any(axis=1).sum())
    print(Z, norm, early_stop, max_iter, "frames whose float32 posterior differs from the rounded float64 one:",
          differ, "of", FRAMES)
    assert differ >= 1
    dec = _dec(Z, max_iter=max_iter, normalization=norm, early_stop=early_stop)
    info = dec.plan.info
    assert info.reserved == 13 and info.kind == 1 and info.n_in == info.n_out == 8 * Z
    _same(_soft(dec, _llr(Z)), want)


# ---- 2. Z = 1 --------------------------------------------------------------------
def test_z1_is_the_serial_schedule(gpu):
    """Z = 1: 64 frames per wavefront, and the block rows are the single rows in order."""
    frames = 4 * 64 + 1
    llr = _llr(1, frames, 2.0)
    H = _H(1)
    want = _want(1, 0.75, True, 20, frames, 2.0)
    print("Z = 1 float32 restatement iterations:", np.bincount(want[1], minlength=21))
    assert len(set(want[1].tolist())) > 1  # frames of one wavefront stop at different iterations
    dec = _dec(1, max_iter=20, normalization=0.75)
    p = _probe(1, _N().PL_LDPC_QC_F32, max_iter=20)
    assert dec.plan.info.reserved == 13 and dec.plan.info.frames_per_block == p.fpw * p.fpb
    got = _soft(dec, llr)
    _same(got, want)
    for f in range(0, frames, 16):
        b, i, post = layered_ms_literal32(H, llr[f], 20, 0.75, True)
        assert np.array_equal(got[0][f], b) and got[1][f] == i and np.array_equal(got[2][f], post, equal_nan=True)


# ---- 3. ragged wavefronts and workgroups ---------------------------------------
@pytest.mark.parametrize("Z", [1, 7, 27, 64, 96])
def test_ragged_batches(gpu, Z):
    """Batches 1, one short of a workgroup's frames and one more, with the frames per workgroup the
    single-precision plan chose: masked frames in the last wavefront, a ragged last workgroup."""
    dec = _dec(Z, max_iter=20, normalization=0.75)
    fpg = dec.plan.info.frames_per_block
    p = _probe(Z, _N().PL_LDPC_QC_F32, max_iter=20)
    assert fpg == p.fpw * p.fpb and p.fpw == (64 // Z if Z <= 64 else 1)
    frames, snr = (fpg + 1, 2.0) if Z == 1 else (FRAMES, SNR)
    assert fpg + 1 <= frames
    want = _want(Z, 0.75, True, 20, frames, snr)
    llr = _llr(Z, frames, snr)
    for B in sorted({1, max(fpg - 1, 1), fpg + 1}):
        _same(_soft(dec, llr[:B]), [w[:B] for w in want])


# ---- 4. degrees above each register cap ----------------------------------------
@pytest.mark.parametrize("name,dcap,mw", [("deg40", 0, 3), ("deg12", 16, 1), ("deg24", 32, 2)])
@pytest.mark.parametrize("early_stop", [True, False])
def test_degrees_above_each_cap(gpu, name, dcap, mw, early_stop):
    p = _probe(name, _N().PL_LDPC_QC_F32)
    assert (p.dcap, p.mw) == (dcap, mw) and p.kernel == 13 and p.state_bytes == _state_bytes(name)
    llr = np.array(_llr(name, 16, 3.0))
    llr[3, 10] = np.nan
    llr[5, 7] = 0.0
    want = layered_ms_ref32(_H(name), llr, _layers(name), 8, 0.75, early_stop)
    _same(_soft(_dec(name, max_iter=8, normalization=0.75, early_stop=early_stop), llr), want)


# ---- 5. special values -----------------------------------------------------------
SPECIAL = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e300, -1e300, 5e-324, 1e-45, -1e-40, 3.4028235e38,
                    -3.4028235e38, 1e-38, 3.5e38])


@pytest.mark.parametrize("Z", [27, 96])
@pytest.mark.parametrize("early_stop", [True, False])
def test_special_values(gpu, Z, early_stop):
    """Given as float64: +-1e300 and 3.5e38 round to +-inf, 5e-324 to 0, 1e-45 and -1e-40 to subnormals,
    +-3.4028235e38 to +-FLT_MAX, in the kernel's load as in the restatement's astype."""
    n = 8 * Z
    rng = np.random.RandomState(99)
    llr = awgn_llrs(n, 32, 2.0, seed=98)
    for f in range(32):
        llr[f, rng.choice(n, 6, replace=False)] = SPECIAL[rng.randint(0, len(SPECIAL), 6)]
    assert llr.dtype == np.float64
    want = layered_ms_ref32(_H(Z), llr, _layers(Z), 20, 0.75, early_stop)
    nan_frames = int(np.isnan(want[2]).any(axis=1).sum())
    print("frames with a NaN posterior:", nan_frames, "of 32")
    assert nan_frames > 0
    dec = _dec(Z, max_iter=20, normalization=0.75, early_stop=early_stop)
    _same(_soft(dec, llr), want)  # NumPy in: astype(float32) on the host
    got = dec.decode_batch(torch.from_numpy(llr).cuda(), return_iterations=True, return_llr=True)
    _same(_host(got), want)       # CUDA float64 in: rounded by the kernel's load


# ---- 6. subnormals survive -------------------------------------------------------
@pytest.mark.parametrize("Z", [27, 96])
def test_subnormals_are_kept(gpu, Z):
    llr = awgn_llrs(8 * Z, 8, 1.0, seed=77) * 1e-41
    want = layered_ms_ref32(_H(Z), llr, _layers(Z), 5, 0.75, False)
    assert (want[2] != 0).all() and (np.abs(want[2]) < FLT_MIN).all()  # a flushing kernel returns zeros
    dec = _dec(Z, max_iter=5, normalization=0.75, early_stop=False)
    _same(_soft(dec, llr), want)
    for t in (torch.from_numpy(llr).cuda(), torch.from_numpy(to_f32(llr)).cuda()):
        _same(_host(dec.decode_batch(t, return_iterations=True, return_llr=True)), want)


# ---- 7. input routes -------------------------------------------------------------
def test_input_routes_agree(gpu):
    Z, n = 27, 8 * 27
    dec = _dec(Z, max_iter=20, normalization=0.75)
    want = _want(Z, 0.75, True, 20)
    llr = np.array(_llr(Z))
    _same(_soft(dec, llr), want)  # NumPy float64
    # CUDA float64 and float32 views with row pitch n + 40, padding NaN; device tensors out, `out` honoured
    for dt in (torch.float64, torch.float32):
        wide = torch.full((FRAMES, n + 40), float("nan"), dtype=dt, device="cuda")
        wide[:, :n] = torch.from_numpy(llr).cuda().to(dt)
        view = wide[:, :n]
        assert view.stride(0) == n + 40
        out = torch.empty((FRAMES, n), dtype=torch.uint8, device="cuda")
        bits, its, post = dec.decode_batch(view, out=out, return_iterations=True, return_llr=True)
        assert bits.data_ptr() == out.data_ptr() and post.is_cuda and its.is_cuda and post.dtype == torch.float32
        _same(_host((bits, its, post)), want)
        bits2 = dec.decode_batch(view)
        assert bits2.is_cuda and np.array_equal(bits2.cpu().numpy(), want[0])
    # CUDA float16: converted with .to(torch.float32); a different input, so a different result
    h16 = llr.astype(np.float16)
    w16 = layered_ms_ref32(_H(Z), h16, _layers(Z), 20, 0.75, True)
    changed = int((~((w16[2] == want[2]) | (np.isnan(w16[2]) & np.isnan(want[2])))).any(axis=1).sum())
    print("frames whose posterior the float16 rounding of the input changes:", changed, "of", FRAMES)
    assert changed >= 1
    got = dec.decode_batch(torch.from_numpy(h16).cuda(), return_iterations=True, return_llr=True)
    assert got[2].dtype == torch.float32
    _same(_host(got), w16)
    # host `out`, one frame, the empty batch
    hb = np.full((FRAMES, n), -1, dtype=np.int64)
    r = dec.decode_batch(llr, out=hb, return_llr=True)
    assert r[0] is hb and np.array_equal(hb, want[0]) and r[1].dtype == np.float32
    assert np.array_equal(r[1], want[2], equal_nan=True)
    b, i = dec.decode(llr[4], return_iterations=True)
    assert np.array_equal(b, want[0][4]) and i == want[1][4]
    got0 = dec.decode_batch(llr[:0], return_iterations=True, return_llr=True)
    assert got0[0].shape == (0, n) and got0[1].shape == (0,) and got0[2].shape == (0, n)
    assert got0[0].dtype == np.int64 and got0[1].dtype == np.int64 and got0[2].dtype == np.float32
    for dt in (torch.float32, torch.float64):
        e = dec.decode_batch(torch.empty((0, n), dtype=dt, device="cuda"), return_iterations=True, return_llr=True)
        assert [tuple(x.shape) for x in e] == [(0, n), (0,), (0, n)]
        assert [x.dtype for x in e] == [torch.uint8, torch.int32, torch.float32]


# ---- 8. the state in the workspace ---------------------------------------------
def test_workspace_home(gpu, monkeypatch):
    monkeypatch.setenv("PL_LMS_GLOBAL", "1")
    want = _want(27, 0.75, True, 20)
    dec = _dec(27, max_iter=20, normalization=0.75)
    plan = dec.plan
    assert plan.info.reserved == 14
    unit = plan.workspace_bytes(1)
    assert unit == _state_bytes(27) == 2160 and plan.workspace_bytes(FRAMES) == FRAMES * unit
    l64 = torch.from_numpy(np.array(_llr(27))).cuda()
    l32 = l64.to(torch.float32)
    for llr in (l32, l64):
        _same(_host(dec.decode_batch(llr, return_iterations=True, return_llr=True)), want)
    plan.release()
    for nbytes in (FRAMES * unit, 3 * unit, unit):  # caller-owned workspaces: chunks of 67, 3 and 1 frames
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        for llr in (l32, l64):  # pl_ldpc_decode_f32 with a workspace, pl_decode_ws
            bits = torch.zeros((FRAMES, 8 * 27), dtype=torch.uint8, device="cuda")
            its = torch.zeros(FRAMES, dtype=torch.int32, device="cuda")
            plan.decode(llr, bits, its, ws=ws)
            assert np.array_equal(bits.cpu().numpy(), want[0]) and np.array_equal(its.cpu().numpy(), want[1])
    assert plan.workspace_stats() == (0, 0)  # a caller's workspace leaves the plan's own alone
    # reserve / release / stats, in the single-precision unit
    plan.reserve(FRAMES)
    assert plan.workspace_stats() == (1, FRAMES * unit)
    bits = torch.zeros((FRAMES, 8 * 27), dtype=torch.uint8, device="cuda")
    its = torch.zeros(FRAMES, dtype=torch.int32, device="cuda")
    plan.decode(l32, bits, its)
    assert plan.workspace_stats() == (1, FRAMES * unit)  # no regrowth
    assert np.array_equal(bits.cpu().numpy(), want[0]) and np.array_equal(its.cpu().numpy(), want[1])
    plan.release()
    assert plan.workspace_stats() == (0, 0)
    # one workgroup per frame on the workspace too
    d96 = _dec(96, max_iter=20, normalization=0.75)
    assert d96.plan.info.reserved == 14 and d96.plan.workspace_bytes(1) == _state_bytes(96)
    _same(_soft(d96, _llr(96)), _want(96, 0.75, True, 20))


# ---- 9. many frames ------------------------------------------------------------------
@pytest.mark.parametrize("Z", [27, 96])
def test_1000_and_1003_frames(gpu, Z):
    # 1000 is a multiple of the Z = 27 mapping's frames per workgroup, 1003 is not
    want = _want(Z, 0.75, True, 20, 1003, SNR, 5)
    print("Z", Z, "float32 restatement iterations:", np.bincount(want[1], minlength=21))
    assert want[1].min() < 20 and want[1].max() == 20
    pool = torch.from_numpy(to_f32(_llr(Z, 1003, SNR, 5))).cuda()
    dec = _dec(Z, max_iter=20, normalization=0.75)
    assert 1003 % dec.plan.info.frames_per_block != 0 or Z == 96
    for B in (1000, 1003):
        got = dec.decode_batch(pool[:B], return_iterations=True, return_llr=True)
        _same(_host(got), [w[:B] for w in want])


# ---- 10. boundaries of the feature ---------------------------------------------
def test_boundaries(gpu):
    N, L = _N(), _L()
    Z, n = 27, 8 * 27
    llr = np.array(_llr(Z))
    l64 = torch.from_numpy(llr).cuda()
    l32 = l64.to(torch.float32)
    bits = torch.zeros((FRAMES, n), dtype=torch.uint8, device="cuda")
    its = torch.zeros(FRAMES, dtype=torch.int32, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    P_ = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    # a plan without the flag: the entry point refuses, Plan.decode raises
    d64 = L.QCLayeredMSDecoder(np.array(_base(Z)), Z, max_iter=20, normalization=0.75)
    assert d64.dtype == np.float64 and d64.plan.info.reserved == 11 and not d64.plan.f32
    rc = N.lib.pl_ldpc_decode_f32(d64.plan.handle, P_(l32), FRAMES, n, P_(bits), P_(its), None, 0, None, 0, st)
    assert rc == N.PL_EUNSUPPORTED and b"PL_LDPC_QC_F32" in N.lib.pl_last_error()
    with pytest.raises(AssertionError):
        d64.plan.decode(l32, bits, its)
    with pytest.raises(AssertionError):
        d64.plan.decode_soft(l32, bits, its, torch.empty((FRAMES, n), dtype=torch.float32, device="cuda"))
    # ... and the default decoder given float32 LLRs is still the float64 decoder on their values
    w64 = layered_ms_ref(_H(Z), to_f32(llr).astype(np.float64), _layers(Z), 20, 0.75, True)
    got = d64.decode_batch(l32, return_iterations=True, return_llr=True)
    assert got[2].dtype == torch.float64
    g = _host(got)
    assert np.array_equal(g[0], w64[0]) and np.array_equal(g[1], w64[1])
    assert np.array_equal(g[2], w64[2], equal_nan=True)
    # dtype
    for dt in (np.float32, torch.float32, "float32"):
        assert L.QCLayeredMSDecoder(np.array(_base(Z)), Z, dtype=dt).dtype == np.float32
    for dt in (np.float16, torch.float16, "int32", torch.bfloat16):
        with pytest.raises(ValueError):
            L.QCLayeredMSDecoder(np.array(_base(Z)), Z, dtype=dt)
    # a single-precision plan: pl_decode with fp64 LLRs (the Monte-Carlo harness's route) is the float32 decoder
    want = _want(Z, 0.75, True, 20)
    d32 = _dec(Z, max_iter=20, normalization=0.75)
    assert d32.plan.f32
    d32.plan.decode(l64, bits, its)
    assert np.array_equal(bits.cpu().numpy(), want[0]) and np.array_equal(its.cpu().numpy(), want[1])
    # llr and post must both be fp32, or both fp64
    with pytest.raises(AssertionError):
        d32.plan.decode_soft(l32, bits, its, torch.empty((FRAMES, n), dtype=torch.float64, device="cuda"))
    with pytest.raises(AssertionError):
        d32.plan.decode_soft(l64, bits, its, torch.empty((FRAMES, n), dtype=torch.float32, device="cuda"))
    # the other flag bits are ignored
    p2 = N.qc_ldpc_plan(np.array(_base(Z)), Z, None, 20, True, 0.75, flags=2)
    assert p2.info.reserved == 11
    p3 = N.qc_ldpc_plan(np.array(_base(Z)), Z, None, 20, True, 0.75, flags=3)
    assert p3.info.reserved == 13

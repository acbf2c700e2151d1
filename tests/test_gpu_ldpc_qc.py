"""QCLayeredMSDecoder (ldpc_qc_layered.hip) against the NumPy restatement of the
layered definition (tests/layered_ref.py) on the expanded H with the block rows
as layers, and against LayeredMSDecoder on the same H and layers.  Bar: hard
decisions and iteration counts array_equal, posteriors array_equal with
equal_nan.

Z is the smallest shape at which each mapping can go wrong: 1 (64 frames per
wavefront), 7 (9 frames and one idle lane), 27 (2 frames, 10 idle lanes), 64
(exactly one wavefront), 96 (two wavefronts, 32 idle lanes, workgroup barrier)."""
import functools
import threading

import numpy as np
import pytest
import torch

from layered_ref import awgn_llrs, layered_ms_literal, layered_ms_ref

pytestmark = pytest.mark.gpu

FRAMES = 67
SNR = -1.0


def _L():
    import polarcode_and_ldpc_amd.ldpc as L
    return L


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
    elif name == "empty_row":  # the Z = 27 code with an empty block row put in
        b = np.insert(np.array(_base(27)), 2, -1, axis=0)
    elif name == "big":  # 8 n + 20 m = 184 320 bytes of state: the workspace
        b = L.qc_random_base(32, 64, 160, 3, seed=160)
    else:
        raise KeyError(name)
    b.setflags(write=False)
    return b


def _Z(name):
    return name if isinstance(name, int) else {"deg40": 7, "deg12": 7, "deg24": 7, "empty_row": 27, "big": 160}[name]


@functools.lru_cache(maxsize=None)
def _H(name):
    H = _L().qc_expand(_base(name), _Z(name))
    H.setflags(write=False)
    return H


@functools.lru_cache(maxsize=None)
def _llr(name, frames=FRAMES, snr=SNR, seed=1234):
    a = awgn_llrs(_base(name).shape[1] * _Z(name), frames, snr, seed=seed)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _want(name, norm, early_stop, max_iter, frames=FRAMES):
    """The restatement's (bits, iterations, posterior) with the block rows as layers; shared, read-only."""
    L = _L()
    r = layered_ms_ref(_H(name), _llr(name, frames), L.qc_block_layers(_base(name).shape[0], _Z(name)), max_iter, norm,
                       early_stop)
    for x in r:
        x.setflags(write=False)
    return r


def _dec(name, **kw):
    return _L().QCLayeredMSDecoder(np.array(_base(name)), _Z(name), **kw)


def _same(got, want):
    bits, its, post = got
    assert np.array_equal(bits, want[0])
    assert np.array_equal(its, want[1])
    assert np.array_equal(post, want[2], equal_nan=True)


def _soft(dec, llr):
    return dec.decode_batch(np.array(llr), return_iterations=True, return_llr=True)


# ---- 1. against the restatement ------------------------------------------------
@pytest.mark.parametrize("max_iter", [20, 1])
@pytest.mark.parametrize("early_stop", [True, False])
@pytest.mark.parametrize("norm", [1.0, 0.75])
@pytest.mark.parametrize("Z", [7, 27, 64, 96])
def test_against_restatement(gpu, Z, norm, early_stop, max_iter):
    want = _want(Z, norm, early_stop, max_iter)
    if early_stop and max_iter == 20:
        print(Z, norm, "restatement iterations:", np.bincount(want[1], minlength=21))
        assert want[1].min() <= 3 and (want[1] == 20).any()
    dec = _dec(Z, max_iter=max_iter, normalization=norm, early_stop=early_stop)
    info = dec.plan.info
    assert info.reserved == 11 and info.kind == 1 and info.n_in == info.n_out == 8 * Z
    assert info.frames_per_block == (4 * (64 // Z) if Z <= 64 else 1)
    _same(_soft(dec, _llr(Z)), want)


def test_z1_is_the_serial_schedule(gpu):
    """Z = 1: 64 frames per wavefront, and the block rows are the single rows in order."""
    frames = 4 * 64 + 1
    llr = _llr(1, frames, 2.0)
    H = _H(1)
    want = layered_ms_ref(H, llr, _L().qc_block_layers(4, 1), 20, 0.75, True)
    print("Z = 1 restatement iterations:", np.bincount(want[1], minlength=21))
    assert len(set(want[1].tolist())) > 1  # frames of one wavefront stop at different iterations
    dec = _dec(1, max_iter=20, normalization=0.75)
    assert dec.plan.info.reserved == 11 and dec.plan.info.frames_per_block == 256
    got = _soft(dec, llr)
    _same(got, want)
    for f in range(0, frames, 16):
        b, i, p = layered_ms_literal(H, llr[f], 20, 0.75, True)
        assert np.array_equal(got[0][f], b) and got[1][f] == i and np.array_equal(got[2][f], p, equal_nan=True)


def test_max_iter_zero(gpu):
    for Z in (7, 96):
        llr = np.array(_llr(Z)[:5])
        _same(_soft(_dec(Z, max_iter=0), llr), (llr <= 0, np.zeros(5, np.int64), llr))


# ---- 2. ragged wavefronts and workgroups ---------------------------------------
@pytest.mark.parametrize("Z", [1, 7, 27, 64, 96])
def test_ragged_batches(gpu, Z):
    """Batches 1, one short of a workgroup's frames and one more: masked frames in the last
    wavefront, a ragged last workgroup, frames of one wavefront stopping at different iterations."""
    dec = _dec(Z, max_iter=20, normalization=0.75)
    fpg = dec.plan.info.frames_per_block
    assert fpg == {1: 256, 7: 36, 27: 8, 64: 4, 96: 1}[Z]
    frames = fpg + 1 if Z == 1 else FRAMES
    want = layered_ms_ref(_H(1), _llr(1, frames, 2.0), _L().qc_block_layers(4, 1), 20, 0.75, True) if Z == 1 \
        else _want(Z, 0.75, True, 20)
    llr = _llr(1, frames, 2.0) if Z == 1 else _llr(Z)
    if fpg > 1:
        assert len(set(want[1][:fpg + 1].tolist())) > 1
    for B in sorted({1, max(fpg - 1, 1), fpg + 1}):
        _same(_soft(dec, llr[:B]), [w[:B] for w in want])


# ---- 3. degrees above each register cap ----------------------------------------
@pytest.mark.parametrize("name,dcap,mw", [("deg40", 0, 3), ("deg12", 16, 1), ("deg24", 32, 2)])
@pytest.mark.parametrize("early_stop", [True, False])
def test_degrees_above_each_cap(gpu, name, dcap, mw, early_stop):
    import ctypes
    from polarcode_and_ldpc_amd import _native
    base, Z = _base(name), _Z(name)
    sh = np.ascontiguousarray(base, np.int32)
    out = _native.LdpcQcPlanProbe()
    assert _native.lib.pl_debug_ldpc_qc_plan_probe(sh.shape[0], sh.shape[1], Z, sh.ctypes.data_as(ctypes.c_void_p), None,
                                                   8, 1, 0.75, 0, ctypes.byref(out)) == 0
    assert (out.dcap, out.mw) == (dcap, mw)
    llr = np.array(_llr(name, 16, 3.0))
    llr[3, 10] = np.nan
    llr[5, 7] = 0.0
    want = layered_ms_ref(_H(name), llr, _L().qc_block_layers(base.shape[0], Z), 8, 0.75, early_stop)
    _same(_soft(_dec(name, max_iter=8, normalization=0.75, early_stop=early_stop), llr), want)


# ---- 4. special values and normalizations --------------------------------------
@pytest.mark.parametrize("Z", [27, 96])
@pytest.mark.parametrize("early_stop", [True, False])
def test_special_values(gpu, Z, early_stop):
    n = 8 * Z
    rng = np.random.RandomState(99)
    llr = awgn_llrs(n, 32, 2.0, seed=98)
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e300, -1e300, 5e-324])
    for f in range(32):
        llr[f, rng.choice(n, 6, replace=False)] = special[rng.randint(0, len(special), 6)]
    want = layered_ms_ref(_H(Z), llr, _L().qc_block_layers(4, Z), 20, 0.75, early_stop)
    nan_frames = int(np.isnan(want[2]).any(axis=1).sum())
    print("frames with a NaN posterior:", nan_frames, "of 32")
    assert nan_frames > 0
    _same(_soft(_dec(Z, max_iter=20, normalization=0.75, early_stop=early_stop), llr), want)


@pytest.mark.parametrize("norm", [-0.5, 1.25])
def test_other_normalizations(gpu, norm):
    for Z in (7, 96):
        llr = _llr(Z)[:16]
        want = layered_ms_ref(_H(Z), llr, _L().qc_block_layers(4, Z), 8, norm, True)
        _same(_soft(_dec(Z, max_iter=8, normalization=norm), llr), want)


# ---- 5. layer order, empty block row -------------------------------------------
def test_layer_order_and_empty_block_row(gpu):
    L = _L()
    base, Z = _base("empty_row"), 27
    assert ((base >= 0).sum(axis=1) == 0).tolist() == [False, False, True, False, False]
    order = [3, 0, 4, 2, 1]
    llr = _llr("empty_row")[:10]
    w_nat = layered_ms_ref(_H("empty_row"), llr, L.qc_block_layers(5, Z), 3, 0.75, False)
    w_ord = layered_ms_ref(_H("empty_row"), llr, L.qc_block_layers(5, Z, order), 3, 0.75, False)
    assert all(not np.array_equal(w_nat[2][f], w_ord[2][f]) for f in range(10))
    _same(_soft(L.QCLayeredMSDecoder(base, Z, max_iter=3, normalization=0.75, early_stop=False), llr), w_nat)
    dec = L.QCLayeredMSDecoder(base, Z, max_iter=3, normalization=0.75, early_stop=False, layer_order=order)
    assert [l[0] // Z for l in dec.layers] == order
    _same(_soft(dec, llr), w_ord)
    # with early stop: the empty block row takes no part in the syndrome either
    w_es = layered_ms_ref(_H("empty_row"), llr, L.qc_block_layers(5, Z, order), 20, 0.75, True)
    _same(_soft(L.QCLayeredMSDecoder(base, Z, max_iter=20, normalization=0.75, layer_order=order), llr), w_es)
    with pytest.raises(AssertionError):
        L.QCLayeredMSDecoder(base, Z, layer_order=[0, 1, 2, 3, 3]).plan


# ---- 6. both state homes -------------------------------------------------------
def test_workspace_path(gpu, monkeypatch):
    monkeypatch.setenv("PL_LMS_GLOBAL", "1")
    want = _want(27, 0.75, True, 20)
    dec = _dec(27, max_iter=20, normalization=0.75)
    plan = dec.plan
    assert plan.info.reserved == 12
    llr = torch.from_numpy(np.array(_llr(27))).cuda()
    _same([x.cpu().numpy() for x in dec.decode_batch(llr, return_iterations=True, return_llr=True)], want)
    need = plan.workspace_bytes(FRAMES)
    unit = plan.workspace_bytes(1)
    assert unit > 0 and need == FRAMES * unit
    for nbytes in (need, 3 * unit, unit):  # pl_decode_ws: chunks of 67, 3 frames (a ragged wavefront each) and 1
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        bits = torch.empty((FRAMES, 8 * 27), dtype=torch.uint8, device="cuda")
        its = torch.empty(FRAMES, dtype=torch.int32, device="cuda")
        plan.decode(llr, bits, its, ws=ws)
        assert np.array_equal(bits.cpu().numpy(), want[0]) and np.array_equal(its.cpu().numpy(), want[1])
    # one workgroup per frame on the workspace too
    d96 = _dec(96, max_iter=20, normalization=0.75)
    assert d96.plan.info.reserved == 12
    _same(_soft(d96, _llr(96)), _want(96, 0.75, True, 20))


def test_state_too_large_for_lds(gpu):
    L = _L()
    base, Z = _base("big"), 160
    dec = L.QCLayeredMSDecoder(np.array(base), Z, max_iter=3, normalization=0.75)
    assert dec.plan.info.reserved == 12 and dec.plan.workspace_bytes(1) == 8 * 10240 + 20 * 5120
    llr = awgn_llrs(64 * Z, 3, 1.0, seed=77)
    want = layered_ms_ref(_H("big"), llr, L.qc_block_layers(32, Z), 3, 0.75, True)
    _same(_soft(dec, llr), want)


# ---- 7. device against device --------------------------------------------------
@pytest.mark.parametrize("Z", [27, 96])
def test_equals_generic_layered_decoder(gpu, Z):
    L = _L()
    # 1000 frames, and 1003: 1000 is a multiple of the Z = 27 mapping's 8 frames per workgroup
    pool = torch.from_numpy(awgn_llrs(8 * Z, 1003, SNR, seed=5)).cuda()
    qc = _dec(Z, max_iter=20, normalization=0.75)
    assert 1003 % qc.plan.info.frames_per_block != 0 or Z == 96
    gen = L.LayeredMSDecoder(np.array(_H(Z)), max_iter=20, normalization=0.75, layers=L.qc_block_layers(4, Z))
    for B in (1000, 1003):
        llr = pool[:B]
        a = qc.decode_batch(llr, return_iterations=True, return_llr=True)
        b = gen.decode_batch(llr, return_iterations=True, return_llr=True)
        its = a[1].cpu().numpy()
        print("Z", Z, "frames", B, "iterations:", np.bincount(its, minlength=21))
        assert its.min() < 20 and its.max() == 20
        _same([x.cpu().numpy() for x in a], [x.cpu().numpy() for x in b])


# ---- 8. plumbing ---------------------------------------------------------------
def test_plumbing(gpu):
    L = _L()
    Z, n = 27, 8 * 27
    dec = _dec(Z, max_iter=20, normalization=0.75)
    assert dec.m == 4 * Z and dec.n == n and dec._H is None  # no dense H behind the constructor
    want = _want(Z, 0.75, True, 20)
    llr = np.array(_llr(Z))
    got0 = dec.decode_batch(llr[:0], return_iterations=True, return_llr=True)
    assert got0[0].shape == (0, n) and got0[1].shape == (0,) and got0[2].shape == (0, n)
    # a CUDA view with row pitch > n; device tensors out, no host copy
    wide = torch.full((FRAMES, n + 40), float("nan"), dtype=torch.float64, device="cuda")
    wide[:, :n] = torch.from_numpy(llr).cuda()
    out = torch.empty((FRAMES, n), dtype=torch.uint8, device="cuda")
    bits, its, post = dec.decode_batch(wide[:, :n], out=out, return_iterations=True, return_llr=True)
    assert bits.data_ptr() == out.data_ptr() and post.is_cuda and its.is_cuda
    _same((bits.cpu().numpy(), its.cpu().numpy(), post.cpu().numpy()), want)
    bits2 = dec.decode_batch(wide[:, :n])
    assert bits2.is_cuda and np.array_equal(bits2.cpu().numpy(), want[0])
    hb = np.full((FRAMES, n), -1, dtype=np.int64)
    r = dec.decode_batch(llr, out=hb, return_llr=True)
    assert r[0] is hb and np.array_equal(hb, want[0]) and np.array_equal(r[1], want[2])
    # one frame
    b, i = dec.decode(llr[4], return_iterations=True)
    assert np.array_equal(b, want[0][4]) and i == want[1][4]
    assert np.array_equal(dec.decode(llr[5]), want[0][5])
    assert np.array_equal(dec.H, _H(Z))
    # a block row with a single block: ValueError as LayeredMSDecoder, from Python and from the C-ABI
    b1 = np.array(_base(Z))
    b1[0] = -1
    b1[0, 3] = 5
    with pytest.raises(ValueError, match="zero-size array to reduction operation minimum"):
        L.QCLayeredMSDecoder(b1, Z, max_iter=5).decode_batch(np.ones((2, n)))
    from polarcode_and_ldpc_amd import _native
    with pytest.raises(ValueError, match="degree-1"):
        _native.qc_ldpc_plan(b1, Z, None, 5, True, 1.0)
    _same(_soft(L.QCLayeredMSDecoder(b1, Z, max_iter=0), llr[:3]), (llr[:3] <= 0, np.zeros(3, np.int64), llr[:3]))


def test_two_streams_one_plan(gpu, monkeypatch):
    monkeypatch.setenv("PL_LMS_GLOBAL", "1")
    want = _want(27, 0.75, True, 20)
    plan = _dec(27, max_iter=20, normalization=0.75).plan
    assert plan.info.reserved == 12
    llr = torch.from_numpy(np.array(_llr(27))).cuda()
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream() for _ in range(2)]
    outs = [(torch.empty((FRAMES, 216), dtype=torch.uint8, device="cuda"),
             torch.empty(FRAMES, dtype=torch.int32, device="cuda"),
             torch.empty((FRAMES, 216), dtype=torch.float64, device="cuda")) for _ in range(2)]
    errs = []

    def work(k):
        try:
            torch.cuda.set_device(0)
            for _ in range(4):
                plan.decode_soft(llr, outs[k][0], outs[k][1], outs[k][2], stream=streams[k])
            streams[k].synchronize()
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    th = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    assert plan.workspace_stats()[0] == 2
    for o in outs:
        _same([x.cpu().numpy() for x in o], want)


def test_reserve_release_and_wrong_device(gpu, monkeypatch):
    """pl_plan_reserve / pl_plan_release on a workspace-resident plan, and the refusal of every
    decode entry point from another device (the diagnostic build's pl_debug_set_plan_device
    stands in for a second GPU)."""
    import ctypes
    from polarcode_and_ldpc_amd import _native
    monkeypatch.setenv("PL_LMS_GLOBAL", "1")
    want = _want(27, 0.75, True, 20)
    plan = _dec(27, max_iter=20, normalization=0.75).plan
    unit = plan.workspace_bytes(1)
    plan.reserve(FRAMES)
    assert plan.workspace_stats() == (1, FRAMES * unit)
    llr = torch.from_numpy(np.array(_llr(27))).cuda()
    bits = torch.empty((FRAMES, 216), dtype=torch.uint8, device="cuda")
    its = torch.empty(FRAMES, dtype=torch.int32, device="cuda")
    plan.decode(llr, bits, its)
    assert plan.workspace_stats() == (1, FRAMES * unit)  # no regrowth
    assert np.array_equal(bits.cpu().numpy(), want[0]) and np.array_equal(its.cpu().numpy(), want[1])
    plan.release()
    assert plan.workspace_stats() == (0, 0)

    D = _native.load_diag()
    assert D is not None, "diagnostic library not built (make -C polarcode_and_ldpc_amd/csrc diag)"
    sh = np.ascontiguousarray(_base(27), np.int32)
    h = ctypes.c_void_p()
    assert D.pl_ldpc_qc_plan_create(4, 8, 27, sh.ctypes.data_as(ctypes.c_void_p), None, 20, 1, 0.75, 0,
                                    ctypes.byref(h)) == 0, D.pl_last_error()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    P_ = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    ws = torch.empty(FRAMES * unit, dtype=torch.uint8, device="cuda")
    post = torch.empty((FRAMES, 216), dtype=torch.float64, device="cuda")
    cur = torch.cuda.current_device()
    assert D.pl_debug_set_plan_device(h, cur + 7) == 0
    calls = {
        "pl_decode": lambda: D.pl_decode(h, P_(llr), FRAMES, 216, P_(bits), P_(its), st),
        "pl_decode_ws": lambda: D.pl_decode_ws(h, P_(llr), FRAMES, 216, P_(bits), P_(its), P_(ws), ws.numel(), st),
        "pl_ldpc_decode_soft": lambda: D.pl_ldpc_decode_soft(h, P_(llr), FRAMES, 216, P_(bits), P_(its), P_(post),
                                                             216, st),
        "pl_plan_reserve": lambda: D.pl_plan_reserve(h, FRAMES, st),
        "pl_plan_release": lambda: D.pl_plan_release(h, st),
    }
    for name, call in calls.items():
        assert call() == _native.PL_EINVAL, name
        assert b"not the plan's device" in D.pl_last_error(), name
    assert D.pl_debug_set_plan_device(h, cur) == 0
    bits.zero_()
    assert D.pl_ldpc_decode_soft(h, P_(llr), FRAMES, 216, P_(bits), P_(its), P_(post), 216, st) == 0
    torch.cuda.synchronize()
    _same((bits.cpu().numpy(), its.cpu().numpy(), post.cpu().numpy()), want)
    assert D.pl_plan_destroy(h) == 0

"""QCFixedMSDecoder (ldpc_qc_fixed.hip) and the LLR quantiser against the NumPy
integer restatement (tests/qc_fixed_ref.py).  Bar: hard decisions, iteration
counts and int8 posteriors array_equal, everywhere.  Every condition on the
inputs (frames that stop early and frames that do not, clamps that act) is
asserted on the restatement before the device is asked."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from qc_fixed_ref import qc_fixed_ms_ref, quantize_ref
from test_qc_fixed_ref_host import SHAPES, integer_case

pytestmark = pytest.mark.gpu

B = 67
STD = dict(norm16=12, llr_scale=4.0, llr_max=31, msg_max=31)   # the decoder's default setting
WIDE = dict(norm16=12, llr_scale=8.0, llr_max=127, msg_max=63)  # the one that saturates


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


def _dec(base, Z, p, max_iter=20, early_stop=True, layer_order=None):
    return _L().QCFixedMSDecoder(np.array(base), Z, max_iter=max_iter, normalization=p["norm16"] / 16.0,
                                 early_stop=early_stop, layer_order=layer_order, llr_scale=p["llr_scale"],
                                 llr_max=p["llr_max"], msg_max=p["msg_max"])


def _ref(base, Z, L, p, max_iter=20, early_stop=True, layer_order=None):
    r = qc_fixed_ms_ref(base, Z, L, max_iter, p["norm16"], p["llr_max"], p["msg_max"], early_stop, layer_order)
    for x in r[:3]:
        x.setflags(write=False)
    return r


def _same(got, want):
    bits, its, post = (x.cpu().numpy() if isinstance(x, torch.Tensor) else x for x in got)
    assert np.array_equal(bits, want[0])
    assert np.array_equal(its, want[1])
    assert post.dtype == np.int8 and np.array_equal(post, want[2])


def _soft(dec, llr):
    return dec.decode_batch(llr, return_iterations=True, return_llr=True)


def _frozen(a):
    a.setflags(write=False)
    return a


# ---- lifting sizes ----------------------------------------------------------------------
ZS = {1: (64, 4), 7: (9, 4), 27: (2, 4), 64: (1, 4), 96: (1, 1)}  # Z: (frames per wavefront, wavefronts per workgroup)


@functools.lru_cache(maxsize=None)
def _z_base(Z):
    return _frozen(_L().qc_random_base(4, 8, Z, 3, seed=500 + Z))


@functools.lru_cache(maxsize=None)
def _z_llr(Z, p="STD"):
    """B frames of AWGN LLRs at 1 dB, quantised by the restatement's quantiser"""
    p = {"STD": STD, "WIDE": WIDE}[p]
    return _frozen(quantize_ref(_awgn(8 * Z, B, 1.0, seed=600 + Z), p["llr_scale"], p["llr_max"]))


@functools.lru_cache(maxsize=None)
def _z_want(Z, early_stop):
    return _ref(_z_base(Z), Z, _z_llr(Z), STD, early_stop=early_stop)


@pytest.mark.parametrize("early_stop", [True, False])
@pytest.mark.parametrize("Z", sorted(ZS))
def test_lifting_sizes(gpu, Z, early_stop):
    """Z = 1, 7, 27, 64: 64, 9, 2 and 1 frames per wavefront (SUBWAVE, the stop mask of frame f shifted by
    f Z bits); 96: one workgroup per frame, its second wavefront half filled.  67 frames: more than one
    workgroup everywhere but at Z = 1, where they are one full wavefront and three frames of a second."""
    want = _z_want(Z, early_stop)
    if early_stop and Z > 1:
        print(Z, "restatement iterations:", np.bincount(want[1], minlength=21))
        assert want[1].min() < 20, "no frame stops early"
        assert len(np.unique(want[1])) > 1, "every frame stops at the same iteration"
    dec = _dec(_z_base(Z), Z, STD, early_stop=early_stop)
    info = dec.plan.info
    assert info.reserved == 15 and info.fused_top == 8
    assert info.frames_per_block == ZS[Z][0] * ZS[Z][1]
    _same(_soft(dec, torch.from_numpy(np.array(_z_llr(Z))).cuda()), want)


# ---- row degrees x lifting size x state home: every compiled instance ----------------------
# the block rows' degrees -> (DCAP, words a check): one word up to degree 14
DEGREES = {(8, 3, 5): (8, 1), (12, 9, 14): (16, 1), (12, 15, 9): (16, 2), (24, 32, 17): (32, 2), (40, 33, 2): (0, 3)}


@functools.lru_cache(maxsize=None)
def _deg_case(degrees, Z):
    base = _frozen(_rows_base(degrees, 48, Z, seed=700 + degrees[0] + Z))
    # dense rows return small messages: high-SNR LLRs at the wide setting keep the magnitudes moving
    L = _frozen(quantize_ref(_awgn(48 * Z, 19, 4.0, seed=800 + degrees[0] + Z), WIDE["llr_scale"], WIDE["llr_max"]))
    return base, L, _ref(base, Z, L, WIDE, max_iter=6)


@pytest.mark.parametrize("home", ["lds", "workspace"])
@pytest.mark.parametrize("Z", [7, 96])
@pytest.mark.parametrize("degrees", sorted(DEGREES), ids=lambda d: "deg%d" % max(d))
def test_row_degrees_and_state_homes(gpu, monkeypatch, degrees, Z, home):
    """Row degrees <= 8, 14 (one word a check), 15 (two), a 24 + 32 mix and 40: the instances that keep 8,
    16 and 32 inputs in registers and the two-pass form (with two flag words a check), each in the
    SUBWAVE (Z = 7) and the block (Z = 96) mapping, with the state in LDS and (PL_LMS_GLOBAL=1) in the
    workspace.  19 frames."""
    dcap, mw = DEGREES[degrees]
    base, L, want = _deg_case(degrees, Z)
    assert np.abs(want[2].astype(np.int64)).max() > 31 and want[3]["sat"] > 0  # the magnitudes do move
    if home == "workspace":
        monkeypatch.setenv("PL_LMS_GLOBAL", "1")
    dec = _dec(base, Z, WIDE, max_iter=6)
    info = dec.plan.info
    assert info.fused_top == dcap and info.reserved == (15 if home == "lds" else 16)
    state = (4 * mw * len(degrees) * Z + 48 * Z + 15) // 16 * 16
    assert dec.plan.workspace_bytes(19) == (19 * state if home == "workspace" else 0)
    _same(_soft(dec, torch.from_numpy(np.array(L)).cuda()), want)
    if home == "workspace":
        assert dec.plan.workspace_stats()[0] == 1
        dec.plan.release()
        assert dec.plan.workspace_stats() == (0, 0)


def test_state_beyond_lds_goes_to_the_workspace(gpu):
    """(16, 64, 1024), rows of up to 15 blocks: 64 Ki + 8 x 16 Ki = 192 KiB of state, above the 160 KB of
    LDS: the planner's own choice of the workspace.  3 frames, 4 iterations."""
    Z = 1024
    base = _L().qc_random_base(16, 64, Z, 3, seed=91)
    L = quantize_ref(_awgn(64 * Z, 3, 1.0, seed=92), 4.0, 31)
    want = _ref(base, Z, L, STD, max_iter=4)
    dec = _dec(base, Z, STD, max_iter=4)
    assert dec.plan.info.reserved == 16 and dec.plan.workspace_bytes(3) == 3 * (64 * Z + 8 * 16 * Z)
    _same(_soft(dec, torch.from_numpy(L).cuda()), want)


# ---- batches, options, inputs at Z = 7 ------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _b_llr():
    return _frozen(quantize_ref(_awgn(56, 1003, 1.0, seed=77), 4.0, 31))


@functools.lru_cache(maxsize=None)
def _b_want():
    return _ref(_z_base(7), 7, _b_llr(), STD)


@pytest.mark.parametrize("batch", [1, 67, 1003])
def test_batches(gpu, batch):
    """1003 frames at Z = 7 (36 per workgroup): 27 full workgroups and a ragged 28th whose last wavefront
    has 4 of its 9 frames; 67 and 1 are the same frames' prefixes."""
    want = tuple(x[:batch] for x in _b_want()[:3])
    dec = _dec(_z_base(7), 7, STD)
    _same(_soft(dec, torch.from_numpy(np.array(_b_llr()[:batch])).cuda()), want)
    if batch == 1:
        bits, its = dec.decode(np.array(_b_llr()[0]), return_iterations=True)
        assert np.array_equal(bits, want[0][0]) and its == want[1][0]


@pytest.mark.parametrize("option", ["layer_order", "no_early_stop", "max_iter_0"])
def test_options(gpu, option):
    Z = 27
    base, L = _z_base(Z), _z_llr(Z)
    kw = {"layer_order": dict(layer_order=[2, 0, 3, 1]), "no_early_stop": dict(early_stop=False),
          "max_iter_0": dict(max_iter=0)}[option]
    want = _ref(base, Z, L, STD, **kw)
    if option == "layer_order":
        assert not np.array_equal(want[2], _z_want(Z, True)[2])  # the order shows in the posteriors
    if option == "max_iter_0":
        assert want[1].max() == 0 and np.array_equal(want[2], L)
    _same(_soft(_dec(base, Z, STD, **kw), torch.from_numpy(np.array(L)).cuda()), want)


def test_all_three_clamps_act(gpu):
    """AWGN LLRs at 1 dB, scale 8, llr_max = 127, msg_max = 63: the posteriors saturate."""
    Z = 27
    base, L = _z_base(Z), _z_llr(Z, "WIDE")
    want = _ref(base, Z, L, WIDE)
    print("clamps:", want[3], "iterations:", np.bincount(want[1], minlength=21))
    assert want[3]["llr"] == 0  # the restatement's quantiser clamped already: count what it clamped
    raw = np.rint(_awgn(8 * Z, B, 1.0, seed=600 + Z) * 8.0)
    assert np.count_nonzero(np.abs(raw) > 127) > 0 and want[3]["msg"] > 0 and want[3]["sat"] > 0
    assert np.abs(want[2].astype(np.int64)).max() == 127
    _same(_soft(_dec(base, Z, WIDE), torch.from_numpy(np.array(L)).cuda()), want)
    # the decoder's own input clamp: the same frames at llr_max = 63 without requantising
    p = dict(WIDE, llr_max=63)
    want = _ref(base, Z, L, p)
    assert min(want[3].values()) > 0, want[3]
    _same(_soft(_dec(base, Z, p), torch.from_numpy(np.array(L)).cuda()), want)


def test_hand_worked_saturation_on_the_device(gpu):
    """tests/test_qc_fixed_ref_host.py's example, each clamp once: Z = 1, 64 frames a wavefront."""
    base = np.array([[0, 0, -1, -1], [-1, -1, 0, 0]])
    L = np.array([[-128, -5, 3, -2]], dtype=np.int8)
    dec = _L().QCFixedMSDecoder(base, 1, max_iter=1, normalization=1.0, llr_max=127, msg_max=100)
    bits, its, post = dec.decode_batch(L, return_iterations=True, return_llr=True)
    assert post.tolist() == [[-127, -105, 1, 1]] and bits.tolist() == [[1, 1, 0, 0]] and its.tolist() == [1]


def test_special_rows(gpu):
    """A row of -128 (clamped to -llr_max, never -128 in the state), an all-zero row (every minimum 0,
    decisions all 1), rows of +-127, among ordinary frames."""
    Z = 27
    base = _z_base(Z)
    L = np.array(_z_llr(Z)[:9])
    L[1], L[3], L[5], L[6] = -128, 0, 127, -127
    for p in (STD, dict(WIDE, norm16=16, msg_max=127)):
        want = _ref(base, Z, L, p)
        assert want[0][3].all() and not want[2][3].any() and want[2][1].min() >= -127
        _same(_soft(_dec(base, Z, p), torch.from_numpy(L).cuda()), want)


def test_pitched_int8_views(gpu):
    """int8 device views with a row pitch (and an odd first byte) are decoded as they are; `out` and the
    posteriors come back dense."""
    Z = 7
    L, want = _b_llr()[:B], tuple(x[:B] for x in _b_want()[:3])
    dec = _dec(_z_base(7), Z, STD)
    for pitch, off in ((56 + 3, 1), (64, 0), (56 + 16, 5)):
        buf = torch.full((B * pitch + off,), 99, dtype=torch.int8, device="cuda")
        view = buf[off:off + B * pitch].view(B, pitch)[:, :56]
        view.copy_(torch.from_numpy(np.array(L)))
        assert view.stride(0) == pitch and not view.is_contiguous()
        out = torch.full((B, 56), 7, dtype=torch.uint8, device="cuda")
        bits, its, post = dec.decode_batch(view, out=out, return_iterations=True, return_llr=True)
        assert bits is out
        _same((bits, its, post), want)


@pytest.mark.parametrize("kind", ["cuda64", "cuda32", "cuda16", "numpy64", "numpy32", "cuda64_pitched"])
def test_floating_input_goes_through_the_quantiser(gpu, kind):
    """fp64 / fp32 / fp16 device tensors through pl_llr_quantize, NumPy arrays through quantize_host: the
    decoder sees what the restatement's quantiser makes of the same values."""
    Z = 27
    base = _z_base(Z)
    x = _awgn(8 * Z, B, 1.0, seed=600 + Z)
    x[0, :6] = [np.nan, np.inf, -np.inf, 0.125, 0.375, -0.625]  # NaN -> 0, +-inf -> +-31, the ties to even
    np_t = {"64": np.float64, "32": np.float32, "16": np.float16}[kind[-2:] if kind[-2:].isdigit() else "64"]
    x = x.astype(np_t)
    # a narrower type widens exactly: the restatement quantises the values the type holds
    Lq = quantize_ref(x.astype(np.float32 if np_t == np.float16 else np_t), 4.0, 31)
    assert Lq[0, :6].tolist() == [0, 31, -31, 0, 2, -2]
    want = _ref(base, Z, Lq, STD)
    dec = _dec(base, Z, STD)
    if kind.startswith("numpy"):
        got = _soft(dec, x)
        assert got[0].dtype == np.int64 and got[1].dtype == np.int64
    elif kind == "cuda64_pitched":
        buf = torch.zeros((B, 8 * Z + 5), dtype=torch.float64, device="cuda")
        buf[:, :8 * Z] = torch.from_numpy(x).cuda()
        got = _soft(dec, buf[:, :8 * Z])
    else:
        got = _soft(dec, torch.from_numpy(x).cuda())
    _same(got, want)
    with pytest.raises(TypeError):
        dec.decode_batch(torch.zeros((1, 8 * Z), dtype=torch.int32, device="cuda"))


@pytest.mark.parametrize("n,rows,pitch,off", [(56, 67, 56, 0), (56, 67, 61, 3), (216, 5, 216, 8), (1, 40, 1, 0),
                                               (15, 9, 15, 1), (16, 9, 32, 0), (2593, 3, 2600, 7), (40, 0, 40, 0)])
@pytest.mark.parametrize("tin", [np.float64, np.float32])
def test_quantiser_kernel(gpu, tin, n, rows, pitch, off):
    """pl_llr_quantize against the restatement: any pitch in and out, output rows that start on and off a
    16-byte boundary, rows shorter than a piece, an empty batch; the bytes around the rows stay."""
    N = _N()
    rs = np.random.RandomState(n + rows)
    x = (rs.standard_normal((rows, n)) * 5.0).astype(tin)
    x.ravel()[::7] = np.round(x.ravel()[::7] * 4.0) / 4.0 + 0.125  # ties
    if x.size >= 3:
        x.ravel()[:3] = [np.nan, np.inf, -np.inf]
    src = torch.zeros((rows, n + 3), dtype=torch.from_numpy(x).dtype, device="cuda")
    src[:, :n] = torch.from_numpy(x).cuda()
    buf = torch.full((rows * pitch + off + 16,), 99, dtype=torch.int8, device="cuda")
    out = buf[off:off + rows * pitch].view(rows, pitch)[:, :n]
    N.llr_quantize(src[:, :n], 4.0, 31, out)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    want = np.full(rows * pitch + off + 16, 99, dtype=np.int8)
    if rows:
        w = want[off:off + rows * pitch].reshape(rows, pitch)
        w[:, :n] = quantize_ref(x, 4.0, 31)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("mb,nb,Z", SHAPES)
def test_equals_the_fp64_kernel_where_no_clamp_acts(gpu, mb, nb, Z):
    """norm16 = 16, msg_max = 127 and integer LLRs on which the restatement reports no clamp: the
    fixed-point kernel equals the shipped fp64 kernel at normalisation 1.0, value for value."""
    base, L, want, _ = integer_case(mb, nb, Z)
    assert not any(want[3].values())
    Lib = _L()
    fx = Lib.QCFixedMSDecoder(base, Z, max_iter=20, normalization=1.0, llr_max=127, msg_max=127)
    got = _soft(fx, torch.from_numpy(np.array(L)).cuda())
    _same(got, want)
    fl = Lib.QCLayeredMSDecoder(base, Z, max_iter=20, normalization=1.0, early_stop=True)
    fb, fi, fp = fl.decode_batch(torch.from_numpy(L.astype(np.float64)).cuda(), return_iterations=True,
                                 return_llr=True)
    assert torch.equal(got[0], fb) and torch.equal(got[1], fi)
    assert torch.equal(got[2].to(torch.float64), fp)


# ---- the C-ABI ------------------------------------------------------------------------------
def _capture(fn):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g


@pytest.mark.parametrize("home", ["lds", "workspace"])
def test_decode_i8_on_a_caller_workspace_replayed_from_a_graph(gpu, monkeypatch, home):
    """pl_ldpc_decode_i8 with workspace_dev set allocates nothing: captured once (one stream, one kernel
    node), replayed on two inputs; the replays equal the eager decodes and the restatement."""
    if home == "workspace":
        monkeypatch.setenv("PL_LMS_GLOBAL", "1")
    Z, h = 27, 19  # two workgroups of 8 frames and a ragged third
    base, L_all = _z_base(Z), _z_llr(Z)[:2 * h]
    want = _ref(base, Z, L_all, STD)
    assert not np.array_equal(want[1][:h], want[1][h:])
    dec = _dec(base, Z, STD)
    plan = dec.plan
    assert plan.info.reserved == (15 if home == "lds" else 16)
    need = plan.workspace_bytes(h)
    assert (need > 0) == (home == "workspace")
    llr = torch.from_numpy(np.array(L_all[:h])).cuda()
    out = torch.empty((h, 8 * Z), dtype=torch.uint8, device="cuda")
    its = torch.empty((h,), dtype=torch.int32, device="cuda")
    post = torch.empty((h, 8 * Z), dtype=torch.int8, device="cuda")
    ws = torch.empty(max(16, need), dtype=torch.uint8, device="cuda")
    g = _capture(lambda: plan._decode(llr, out, its, post, ws, None))
    assert plan.workspace_stats() == (0, 0)  # the caller's workspace only
    for part in (slice(0, h), slice(h, 2 * h)):
        llr.copy_(torch.from_numpy(np.array(L_all[part])))
        eager = _soft(dec, llr)
        for t, v in ((out, 7), (its, -1), (post, 99)):
            t.fill_(v)
        g.replay()
        torch.cuda.synchronize()
        _same((out, its, post), tuple(x[part] for x in want[:3]))
        assert torch.equal(out, eager[0]) and torch.equal(its, eager[1]) and torch.equal(post, eager[2])


def test_wrong_plan_refusals(gpu):
    """A fixed-point plan decodes through pl_ldpc_decode_i8 only, and pl_ldpc_decode_i8 decodes nothing
    else; every refusal comes before the first launch: nothing is written."""
    N = _N()
    Z = 7
    base = _z_base(Z)
    fx = _dec(base, Z, STD).plan
    fl = _L().QCLayeredMSDecoder(base, Z, max_iter=5, dtype=np.float32).plan
    n = 8 * Z
    f64 = torch.zeros((3, n), dtype=torch.float64, device="cuda")
    f32 = torch.zeros((3, n), dtype=torch.float32, device="cuda")
    i8 = torch.zeros((3, n), dtype=torch.int8, device="cuda")
    bits = torch.full((3, n), 7, dtype=torch.uint8, device="cuda")
    ws = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    P = ctypes.c_void_p

    def last():
        return N.lib.pl_last_error().decode()

    calls = {
        "pl_decode": lambda: N.lib.pl_decode(fx.handle, P(f64.data_ptr()), 3, n, P(bits.data_ptr()), None, None),
        "pl_decode_ws": lambda: N.lib.pl_decode_ws(fx.handle, P(f64.data_ptr()), 3, n, P(bits.data_ptr()), None,
                                                   P(ws.data_ptr()), 4096, None),
        "pl_ldpc_decode_soft": lambda: N.lib.pl_ldpc_decode_soft(fx.handle, P(f64.data_ptr()), 3, n,
                                                                 P(bits.data_ptr()), None, P(f64.data_ptr()), n, None),
        "pl_ldpc_decode_f32": lambda: N.lib.pl_ldpc_decode_f32(fx.handle, P(f32.data_ptr()), 3, n, P(bits.data_ptr()),
                                                               None, None, 0, None, 0, None),
    }
    for name, call in calls.items():
        assert call() == N.PL_EUNSUPPORTED, name
        assert "pl_ldpc_decode_i8" in last(), (name, last())
    assert N.lib.pl_ldpc_decode_i8(fl.handle, P(i8.data_ptr()), 3, n, P(bits.data_ptr()), None, None, 0, None, 0,
                                   None) == N.PL_EUNSUPPORTED
    assert "fixed-point" in last()
    # the argument checks of pl_ldpc_decode_i8 itself
    assert N.lib.pl_ldpc_decode_i8(fx.handle, P(i8.data_ptr()), 3, n - 1, P(bits.data_ptr()), None, None, 0, None, 0,
                                   None) == N.PL_EINVAL and "ld < n" in last()
    assert N.lib.pl_ldpc_decode_i8(fx.handle, P(i8.data_ptr()), 3, n, P(bits.data_ptr()), None, P(i8.data_ptr()),
                                   n - 1, None, 0, None) == N.PL_EINVAL and "ld_post < n" in last()
    assert N.lib.pl_ldpc_decode_i8(fx.handle, None, 3, n, P(bits.data_ptr()), None, None, 0, None, 0,
                                   None) == N.PL_EINVAL
    assert N.lib.pl_ldpc_decode_i8(fx.handle, None, 0, n, None, None, None, 0, None, 0, None) == N.PL_OK  # empty
    torch.cuda.synchronize()
    assert bool((bits == 7).all())
    # the Python layer: dtypes and plans go together
    with pytest.raises(AssertionError):
        fx.decode(f64, bits)
    with pytest.raises(AssertionError):
        fl.decode(i8, bits)
    # the quantiser's refusals
    q = N.lib.pl_llr_quantize
    o = P(i8.data_ptr())
    for args, word in (((P(f64.data_ptr()), 2, n, 3, n, 4.0, 31, o, n, None), "flag"),
                       ((P(f64.data_ptr()), 0, n, -1, n, 4.0, 31, o, n, None), "batch"),
                       ((P(f64.data_ptr()), 0, n, 3, 0, 4.0, 31, o, n, None), "n must"),
                       ((P(f64.data_ptr()), 0, n, 3, n, 0.0, 31, o, n, None), "scale"),
                       ((P(f64.data_ptr()), 0, n, 3, n, float("inf"), 31, o, n, None), "scale"),
                       ((P(f64.data_ptr()), 0, n, 3, n, float("nan"), 31, o, n, None), "scale"),
                       ((P(f64.data_ptr()), 0, n, 3, n, 4.0, 128, o, n, None), "llr_max"),
                       ((P(f64.data_ptr()), 0, n - 1, 3, n, 4.0, 31, o, n, None), "ld < n"),
                       ((P(f64.data_ptr()), 0, n, 3, n, 4.0, 31, o, n - 1, None), "ld_out"),
                       ((None, 0, n, 3, n, 4.0, 31, o, n, None), "NULL"),
                       ((P(f64.data_ptr() + 4), 0, n, 2, n, 4.0, 31, o, n, None), "aligned")):
        assert q(*args) == N.PL_EINVAL and word in last(), (word, last())
    torch.cuda.synchronize()
    assert not bool(i8.any())


# ---- the harness ----------------------------------------------------------------------------
def test_harness_round_equals_the_host_chain(gpu):
    """One ldpc_round_fn round of 256 frames with encoder and rate matcher: the three counters equal the
    same chain recomputed on the host from the round's own LLRs -- quantised and decoded by the
    restatement, counted over the k - fillers message positions."""
    from polarcode_and_ldpc_amd import _native
    from polarcode_and_ldpc_amd.channel.awgn import AWGNChannel
    from polarcode_and_ldpc_amd.harness.montecarlo import _stream_seed, ldpc_round_fn
    Lib = _L()
    Z, frames, offset = 27, 256, 100
    base = Lib.qc_encodable_base(8, 12, Z, 3, 2, core=4, chained=False)
    rm = Lib.QCRateMatcher(base, Z, 260, punctured=2, fillers=5, start=0)
    enc = Lib.QCLDPCEncoder(base, Z)
    dec = _dec(rm.decoder_base(), Z, STD)
    got = ldpc_round_fn(dec, seed=3, encoder=enc, rate_matcher=rm)(1, 0.0, offset, frames)
    # the round's own frames, from the device frame source the other tests pin: messages with a zero
    # filler tail, codewords, the E selected bits, AWGN, recovery into the decoder's fp64 input
    s = _stream_seed(3, 1)
    msg = torch.empty((frames, rm.k), dtype=torch.uint8, device="cuda")
    _native.random_bits(s, offset, msg)
    msg[:, rm.k - rm.fillers:] = 0
    tx = rm.select(enc.encode_batch_device(msg))
    rx = torch.empty((frames, rm.E), dtype=torch.float64, device="cuda")
    AWGNChannel(0.0).llr_batch_device(tx, rm.E, frames, seed=s ^ 0xA5A5A5A5, frame_offset=offset, out=rx)
    seen = {"llr": rm.recover(rx).cpu().numpy(), "msg": msg.cpu().numpy()}
    assert seen["llr"].dtype == np.float64 and seen["llr"].shape == (frames, rm.n_dec)
    kf = rm.k - rm.fillers
    Lq = quantize_ref(seen["llr"], 4.0, 31)
    bits = qc_fixed_ms_ref(rm.decoder_base(), Z, Lq, 20, 12, 31, 31, True)[0]
    err = bits[:, :kf] != seen["msg"][:, :kf]
    want = [int(err.sum()), int(err.any(axis=1).sum()), frames]
    print("harness round:", got.tolist(), "host chain:", want)
    assert 0 < want[1] < frames  # some frames fail and some do not: the counters are not trivial
    assert got.tolist() == want
    # the plain chain (no rate matcher) takes the decoder too: all-zero codeword, high SNR, no error
    plain = ldpc_round_fn(_dec(base, Z, STD), seed=3)
    assert plain(0, 12.0, 0, frames).tolist() == [0, 0, frames]


def test_simulate_qc_ldpc_fixed_and_unchanged_without(gpu, tmp_path, capsys):
    """simulate_qc_ldpc(fixed=...) runs the fixed-point decoder and keys its log rows with the three
    parameters; without fixed= counts, run key and log rows are what they were."""
    import json
    from polarcode_and_ldpc_amd.harness import ber
    from polarcode_and_ldpc_amd.harness.montecarlo import MonteCarlo, ldpc_round_fn
    Lib = _L()
    Z = 27
    base = Lib.qc_encodable_base(8, 12, Z, 3, 2, core=4, chained=False)
    snr, nfr = [-1.0, 2.0], 2048
    kw = dict(max_iter=20, normalization=0.75, batch=1024, seed=5, random_codewords=True)
    log = tmp_path / "points.jsonl"
    _, _, flt = ber.simulate_qc_ldpc(snr, nfr, 10 ** 9, base, Z, dtype=np.float32, log_path=str(log), **kw)
    # what it returns today: the same MonteCarlo over the float decoder, built by hand
    dec = Lib.QCLayeredMSDecoder(base, Z, max_iter=20, normalization=0.75, early_stop=True, dtype=np.float32)
    mc = MonteCarlo(ldpc_round_fn(dec, seed=5, info_bits=dec.n - dec.m, encoder=Lib.QCLDPCEncoder(base, Z)),
                    info_bits=dec.n - dec.m, batch=1024, device=torch.device("cuda", 0))
    hand = mc.run(snr, nfr, 10 ** 9)
    assert [(p.frame_errors, p.bit_errors, p.frames) for p in flt] == \
        [(p.frame_errors, p.bit_errors, p.frames) for p in hand]
    rows = [json.loads(l) for l in log.read_text().splitlines() if l.strip()]
    assert len(rows) == 2 and all("fixed" not in r["key"] for r in rows)
    assert sorted(rows[0]["key"]) == sorted(["code", "n", "k", "Z", "max_iter", "norm", "dtype", "random", "frames",
                                             "max_errors", "seed", "base", "round_frames", "lib"])
    _, _, fix = ber.simulate_qc_ldpc(snr, nfr, 10 ** 9, base, Z, fixed=(4.0, 31, 31), log_path=str(log), **kw)
    rows = [json.loads(l) for l in log.read_text().splitlines() if l.strip()]
    assert len(rows) == 4 and all(r["key"]["fixed"] == [4.0, 31, 31] for r in rows[2:])
    assert [p.frames for p in fix] == [nfr] * 2 and nfr > fix[0].frame_errors > fix[1].frame_errors >= 0
    fdec = _dec(base, Z, STD)
    mc = MonteCarlo(ldpc_round_fn(fdec, seed=5, info_bits=fdec.n - fdec.m, encoder=Lib.QCLDPCEncoder(base, Z)),
                    info_bits=fdec.n - fdec.m, batch=1024, device=torch.device("cuda", 0))
    assert [(p.frame_errors, p.bit_errors) for p in mc.run(snr, nfr, 10 ** 9)] == \
        [(p.frame_errors, p.bit_errors) for p in fix]
    # the command line
    capsys.readouterr()
    ber.main(["--code", "qcldpc", "--qc", "8,12,27,3,2,4", "--fixed", "4,31,31", "--ldpc-codewords", "random",
              "--norm", "0.75", "--snr=-1:2:3", "--frames", str(nfr), "--max-errors", str(10 ** 9), "--batch", "1024",
              "--seed", "5", "--max-iter", "20"])
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    cbase = Lib.qc_encodable_base(8, 12, Z, 3, 2, core=4)  # the command line's code: chained
    _, _, cfix = ber.simulate_qc_ldpc(snr, nfr, 10 ** 9, cbase, Z, fixed=(4.0, 31, 31), **kw)
    assert [(p["frame_errors"], p["bit_errors"]) for p in out["points"]] == \
        [(p.frame_errors, p.bit_errors) for p in cfix]
    with pytest.raises(SystemExit):
        ber.main(["--code", "qcldpc", "--fixed", "4,31"])

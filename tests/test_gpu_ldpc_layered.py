"""LayeredMSDecoder (ldpc_layered.hip) against the NumPy restatement of its
definition (tests/layered_ref.py).  Bar: hard decisions and iteration counts
array_equal, posteriors array_equal with equal_nan (no transcendental is
involved, so the arithmetic is reproducible bit for bit)."""
import functools
import threading

import numpy as np
import pytest
import torch

from layered_ref import awgn_llrs, layered_ms_ref

pytestmark = pytest.mark.gpu


def _L():
    import polarcode_and_ldpc_amd.ldpc as L
    return L


@functools.lru_cache(maxsize=None)
def _code(name):
    L = _L()
    if name == "r96":
        H = L.regular_construction(96, 3, 6, seed=96)
    elif name == "r504":
        H = L.regular_construction(504, 3, 6, seed=3)
    elif name == "r480":
        H = L.regular_construction(480, 4, 8, seed=484)
    elif name == "r2048":
        H = L.regular_construction(2048, 3, 6, seed=2048)
    elif name == "r8192":
        H = L.regular_construction(8192, 3, 6, seed=1)
    elif name == "irr504":
        # one zero-degree row, one row of degree >= 13 (two rows ORed into a third), no degree-1 row
        H = L.regular_construction(504, 3, 6, seed=3).copy()
        H[11] = 0
        H[40] = H[40] | H[41] | H[42]
        deg = H.sum(axis=1)
        assert deg.min() == 0 and deg.max() >= 13 and not (deg == 1).any()
    elif name == "irr504w":
        # a row of degree > 32: its negative flags take more than one state word
        H = np.array(_code("irr504"))
        H[40] = H[40] | H[43] | H[44] | H[45] | H[46]
        assert H.sum(axis=1).max() > 32
    else:
        raise KeyError(name)
    H.setflags(write=False)
    return H


# SNR (dB, all-zero codeword) per code at which the restatement's iteration counts
# hold, for both normalisations, a frame that stops within 3 iterations and one
# that uses all 20 (asserted below on the restatement)
SNR = {"r96": -0.5, "r504": -1.25, "r480": -1.0, "irr504": -1.25}
FRAMES = 67


@functools.lru_cache(maxsize=None)
def _llr(name):
    a = awgn_llrs(_code(name).shape[1], FRAMES, SNR[name], seed=1234)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _want(name, norm, early_stop, max_iter):
    """The restatement's (bits, iterations, posterior) with the default layers; shared, read-only."""
    H = _code(name)
    r = layered_ms_ref(H, _llr(name), _L().layer_schedule(H), max_iter, norm, early_stop)
    for x in r:
        x.setflags(write=False)
    return r


def _same(got, want):
    bits, its, post = got
    assert np.array_equal(bits, want[0])
    assert np.array_equal(its, want[1])
    assert np.array_equal(post, want[2], equal_nan=True)


# ---- 1. against the restatement ------------------------------------------------
@pytest.mark.parametrize("max_iter", [20, 1])
@pytest.mark.parametrize("early_stop", [True, False])
@pytest.mark.parametrize("norm", [1.0, 0.75])
@pytest.mark.parametrize("name", ["r96", "r504", "r480", "irr504"])
def test_against_restatement(gpu, name, norm, early_stop, max_iter):
    want = _want(name, norm, early_stop, max_iter)
    if early_stop and max_iter == 20:
        print(name, norm, "restatement iterations:", np.bincount(want[1], minlength=21))
        assert want[1].min() <= 3 and (want[1] == 20).any()
    dec = _L().LayeredMSDecoder(_code(name), max_iter=max_iter, normalization=norm, early_stop=early_stop)
    assert dec.plan.info.reserved == 9 and dec.plan.info.kind == 1
    _same(dec.decode_batch(np.array(_llr(name)), return_iterations=True, return_llr=True), want)


@pytest.mark.parametrize("early_stop", [True, False])
def test_row_degree_above_32(gpu, early_stop):
    L = _L()
    H = _code("irr504w")
    llr = np.array(_llr("irr504")[:16])
    llr[3, 100] = np.nan
    llr[5, 7] = 0.0
    want = layered_ms_ref(H, llr, L.layer_schedule(H), 8, 0.75, early_stop)
    dec = L.LayeredMSDecoder(H, max_iter=8, normalization=0.75, early_stop=early_stop)
    _same(dec.decode_batch(llr, return_iterations=True, return_llr=True), want)


# ---- 2. layers wider than a wavefront, and the LDS limit -----------------------
@pytest.mark.parametrize("name,frames,max_iter", [("r2048", 9, 20), ("r8192", 3, 5)])
def test_wide_layers(gpu, name, frames, max_iter):
    L = _L()
    H = _code(name)
    layers = L.layer_schedule(H)
    assert max(len(l) for l in layers) > 64
    if name == "r8192":
        assert len(layers) == 9 and max(len(l) for l in layers) == 723
    llr = awgn_llrs(H.shape[1], frames, 1.0, seed=77)
    dec = L.LayeredMSDecoder(H, max_iter=max_iter, normalization=0.75)
    assert dec.plan.info.reserved == 9 and dec.plan.info.frames_per_block == 1
    _same(dec.decode_batch(llr, return_iterations=True, return_llr=True),
          layered_ms_ref(H, llr, layers, max_iter, 0.75, True))


# ---- 3. workspace path ----------------------------------------------------------
def test_workspace_path(gpu, monkeypatch):
    monkeypatch.setenv("PL_LMS_GLOBAL", "1")
    want = _want("r504", 0.75, True, 20)
    dec = _L().LayeredMSDecoder(_code("r504"), max_iter=20, normalization=0.75)
    plan = dec.plan
    assert plan.info.reserved == 10
    llr = torch.from_numpy(np.array(_llr("r504"))).cuda()
    _same([x.cpu().numpy() for x in dec.decode_batch(llr, return_iterations=True, return_llr=True)], want)
    need = plan.workspace_bytes(FRAMES)
    unit = plan.workspace_bytes(1)
    assert unit > 0 and need == FRAMES * unit
    for nbytes in (need, unit):
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        bits = torch.empty((FRAMES, 504), dtype=torch.uint8, device="cuda")
        its = torch.empty(FRAMES, dtype=torch.int32, device="cuda")
        plan.decode(llr, bits, its, ws=ws)
        assert np.array_equal(bits.cpu().numpy(), want[0]) and np.array_equal(its.cpu().numpy(), want[1])
    # a wide-layer code (one workgroup per frame) on the workspace too
    H = _code("r2048")
    l2 = awgn_llrs(2048, 3, 1.0, seed=78)
    d2 = _L().LayeredMSDecoder(H, max_iter=4, normalization=0.75)
    assert d2.plan.info.reserved == 10
    _same(d2.decode_batch(l2, return_iterations=True, return_llr=True),
          layered_ms_ref(H, l2, d2.layers, 4, 0.75, True))


# ---- 4. layer order is honoured -------------------------------------------------
def test_layer_order(gpu):
    L = _L()
    H = _code("r96")
    llr = np.array(_llr("r96")[:10])
    greedy = L.layer_schedule(H)
    serial = [[c] for c in range(H.shape[0])]
    rev = greedy[::-1]
    w_serial = layered_ms_ref(H, llr, serial, 3, 0.75, False)
    w_rev = layered_ms_ref(H, llr, rev, 3, 0.75, False)
    assert all(not np.array_equal(w_serial[2][f], w_rev[2][f]) for f in range(10))
    for layers, want in ((serial, w_serial), (rev, w_rev)):
        dec = L.LayeredMSDecoder(H, max_iter=3, normalization=0.75, early_stop=False, layers=layers)
        assert [list(l) for l in dec.layers] == [list(l) for l in layers]
        _same(dec.decode_batch(llr, return_iterations=True, return_llr=True), want)


# ---- 5. special values ----------------------------------------------------------
@pytest.mark.parametrize("early_stop", [True, False])
def test_special_values(gpu, early_stop):
    L = _L()
    H = _code("r96")
    rng = np.random.RandomState(99)
    llr = awgn_llrs(96, 32, 2.0, seed=98)
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e300, -1e300, 5e-324])
    for f in range(32):
        llr[f, rng.choice(96, 6, replace=False)] = special[rng.randint(0, len(special), 6)]
    want = layered_ms_ref(H, llr, L.layer_schedule(H), 20, 0.75, early_stop)
    nan_frames = int(np.isnan(want[2]).any(axis=1).sum())
    print("frames with a NaN posterior:", nan_frames, "of 32")
    assert nan_frames > 0
    dec = L.LayeredMSDecoder(H, max_iter=20, normalization=0.75, early_stop=early_stop)
    _same(dec.decode_batch(llr, return_iterations=True, return_llr=True), want)


# ---- 6. plumbing ------------------------------------------------------------------
def test_plumbing(gpu):
    L = _L()
    H = _code("r96")
    dec = L.LayeredMSDecoder(H, max_iter=20, normalization=0.75)
    assert [len(l) for l in dec.layers] == [9, 8, 8, 8, 5, 6, 3, 1]
    llr65 = awgn_llrs(96, 65, 1.0, seed=3)
    want = layered_ms_ref(H, llr65, dec.layers, 20, 0.75, True)
    for B in (0, 1, 65):  # 65: a ragged last workgroup
        got = dec.decode_batch(llr65[:B], return_iterations=True, return_llr=True)
        assert got[0].shape == (B, 96) and got[1].shape == (B,) and got[2].shape == (B, 96)
        _same(got, [w[:B] for w in want])
    # a CUDA view with row pitch > n; device tensors out
    wide = torch.full((65, 128), float("nan"), dtype=torch.float64, device="cuda")
    wide[:, :96] = torch.from_numpy(llr65).cuda()
    out = torch.empty((65, 96), dtype=torch.uint8, device="cuda")
    bits, its, post = dec.decode_batch(wide[:, :96], out=out, return_iterations=True, return_llr=True)
    assert bits.data_ptr() == out.data_ptr() and post.is_cuda and its.is_cuda
    _same((bits.cpu().numpy(), its.cpu().numpy(), post.cpu().numpy()), want)
    # out= is reused; return_llr without return_iterations
    out.zero_()
    bits2, post2 = dec.decode_batch(wide[:, :96], out=out, return_llr=True)
    assert bits2.data_ptr() == out.data_ptr() and np.array_equal(out.cpu().numpy(), want[0])
    assert np.array_equal(post2.cpu().numpy(), want[2])
    hb = np.full((65, 96), -1, dtype=np.int64)
    r = dec.decode_batch(llr65, out=hb, return_llr=True)
    assert r[0] is hb and np.array_equal(hb, want[0]) and np.array_equal(r[1], want[2])
    assert np.array_equal(dec.decode_batch(llr65), want[0])
    # one frame
    b, i = dec.decode(llr65[4], return_iterations=True)
    assert np.array_equal(b, want[0][4]) and i == want[1][4]
    assert np.array_equal(dec.decode(llr65[5]), want[0][5])
    # max_iter = 0: the decisions of the channel LLRs
    d0 = L.LayeredMSDecoder(H, max_iter=0)
    _same(d0.decode_batch(llr65[:5], return_iterations=True, return_llr=True),
          (llr65[:5] <= 0, np.zeros(5, np.int64), llr65[:5]))


def test_soft_output_other_plans_and_degree_one(gpu):
    from polarcode_and_ldpc_amd import _native
    L = _L()
    H = _code("r96")
    ms = L.MSDecoder(H, max_iter=5)
    llr = torch.from_numpy(awgn_llrs(96, 4, 1.0, seed=3)).cuda()
    bits = torch.empty((4, 96), dtype=torch.uint8, device="cuda")
    post = torch.empty((4, 96), dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError):
        ms.plan.decode_soft(llr, bits, None, post)
    from polarcode_and_ldpc_amd.polar import SCDecoder
    sc = SCDecoder(64, 32)
    rc = _native.lib.pl_ldpc_decode_soft(sc.plan.handle, None, 0, 64, None, None, None, 64, None)
    assert rc == _native.PL_EUNSUPPORTED
    H1 = H.copy()
    H1[0] = 0
    H1[0, 3] = 1
    with pytest.raises(ValueError, match="zero-size array to reduction operation minimum"):
        L.LayeredMSDecoder(H1, max_iter=5).decode_batch(np.ones((2, 96)))
    # as MSDecoder, no iteration means no empty minimum: the channel decisions
    l0 = awgn_llrs(96, 3, 1.0, seed=4)
    _same(L.LayeredMSDecoder(H1, max_iter=0).decode_batch(l0, return_iterations=True, return_llr=True),
          (l0 <= 0, np.zeros(3, np.int64), l0))
    with pytest.raises(ValueError):  # the C-ABI's own check
        _native.layered_ldpc_plan(*L.dense_to_csr(H1), 96, L.layer_schedule(H1), 5, True, 1.0)
    with pytest.raises(AssertionError):  # rows 0.. of a layer sharing a column
        L.LayeredMSDecoder(H, layers=[list(range(H.shape[0]))]).plan


def test_two_streams_one_plan(gpu, monkeypatch):
    monkeypatch.setenv("PL_LMS_GLOBAL", "1")
    want = _want("r504", 0.75, True, 20)
    dec = _L().LayeredMSDecoder(_code("r504"), max_iter=20, normalization=0.75)
    plan = dec.plan
    assert plan.info.reserved == 10
    llr = torch.from_numpy(np.array(_llr("r504"))).cuda()
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream() for _ in range(2)]
    outs = [(torch.empty((FRAMES, 504), dtype=torch.uint8, device="cuda"),
             torch.empty(FRAMES, dtype=torch.int32, device="cuda"),
             torch.empty((FRAMES, 504), dtype=torch.float64, device="cuda")) for _ in range(2)]
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


# ---- 7. convergence sanity (a property, not parity) -----------------------------
def test_converges_faster_than_flooding(gpu):
    from polarcode_and_ldpc_amd.harness.montecarlo import ldpc_round_fn
    L = _L()
    H = _code("r504")
    counts = {}
    for name, dec in (("layered", L.LayeredMSDecoder(H, max_iter=5, normalization=0.75)),
                      ("flooding", L.MSDecoder(H, max_iter=5, normalization=0.75))):
        counts[name] = ldpc_round_fn(dec, seed=7)(0, 0.0, 0, 4096)
    print("frame errors of 4096 at 0 dB, 5 iterations:", {k: int(v[1]) for k, v in counts.items()})
    assert counts["layered"][2] == counts["flooding"][2] == 4096
    assert counts["layered"][1] < counts["flooding"][1]

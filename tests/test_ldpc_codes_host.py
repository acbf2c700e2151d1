"""The code table of tests/ldpc_codes.py on the host (no GPU): every code has
the degrees it is there for and gets the kernel it is there for from the
planner's device-free probe, so the GPU cases of test_gpu_ldpc_kernels.py mean
what their ids say; and the C oracle's hand-written pairwise sum agrees with
np.sum (oracle/refnumpy.py) where variable degrees reach 128."""
import ctypes

import numpy as np
import pytest

import ldpc_codes as C


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


@pytest.mark.parametrize("cid", sorted(C.SHAPES))
def test_code_degrees(cid):
    H, rp, ci = C.code(cid)
    n, m, rows, cols = C.SHAPES[cid]
    assert H.shape == (m, n)
    assert set(H.sum(axis=0).tolist()) == cols
    rowdeg = H.sum(axis=1)
    if cid == "widecols":
        assert (rowdeg.min(), rowdeg.max()) == C.WIDECOLS_ROWDEG and H.sum() == 2256
    else:
        assert set(rowdeg.tolist()) == rows
    assert np.array_equal(np.diff(rp), rowdeg) and len(ci) == H.sum()


def test_builders():
    L = C._L()
    H = L.regular_construction(96, 3, 6, seed=99)
    M = C.moved(H)
    assert np.array_equal(M.sum(axis=0), H.sum(axis=0))           # column weights stay
    d = M.sum(axis=1) - H.sum(axis=1)
    assert d[0] == 10 and sorted(d[1:].tolist()) == [-1] * 10 + [0] * 37  # ten donors, each used once
    assert np.array_equal(np.flatnonzero(M[0] & ~H[0]), np.flatnonzero(H[0] == 0)[:10])
    I = C.irregular(H)
    assert H.sum() - I.sum() == 5 and all(I[r, np.flatnonzero(H[r])[0]] == 0 for r in (0, 5, 11, 17, 23))
    D = C.blockdiag(H, M[:5])
    assert D.shape == (53, 192) and np.array_equal(D[:48, :96], H) and np.array_equal(D[48:, 96:], M[:5])
    assert D[:48, 96:].sum() == 0 and D[48:, :96].sum() == 0
    W = C.colweights(160, C.WIDECOLS_WS, 5)
    assert np.array_equal(W.sum(axis=0), C.WIDECOLS_WS)
    rs = np.random.RandomState(5)
    assert np.array_equal(np.flatnonzero(W[:, 0]), np.sort(rs.choice(160, 2, replace=False)))


@pytest.mark.parametrize("case", sorted(C.PLANS), ids=lambda k: "%s-%s-%s" % (k[0], "ms" if k[1] else "bp",
                                                                             C.OVERRIDE_ENV[k[2]] or "default"))
def test_plan_table(case):
    from polarcode_and_ldpc_amd import _native
    cid, algo, override = case
    want = dict(C.PLANS[case])
    H, rp, ci = C.code(cid)
    out = _native.LdpcPlanProbe()
    rc = _native.lib.pl_debug_ldpc_plan_probe(len(rp) - 1, H.shape[1], _ptr(rp), _ptr(ci), algo, C.MAX_ITER, 1, 0.75,
                                              override, 0, 0, ctypes.byref(out))
    assert rc == 0, _native.lib.pl_last_error()
    lds = want.pop("lds", None)
    got = {k: getattr(out, k) for k in want}
    assert got == want
    if lds is not None:
        assert out.lds_bytes == lds
    if want["use_global"]:
        assert out.work_bytes_per_frame == 16 * len(ci)


def test_compact_instances():
    """Which ldpc_ms_compact_kernel instance each compact case launches:
    pick_kernel's predicate (n <= 8192, regular, (3,6), |norm| <= 1) restated."""
    compact = {k[0] for k, v in C.PLANS.items() if v["kernel"] == 5}
    assert {cid for cid, _ in C.COMPACT_INSTANCE} == compact
    for (cid, norm), want in C.COMPACT_INSTANCE.items():
        assert C.compact_instance(cid, norm) == want, (cid, norm)
    assert set(C.COMPACT_INSTANCE.values()) == {"8,0,0", "0,0,0", "8,3,6", "8,3,6,PRE"}


@pytest.mark.parametrize("algo,norm", [("bp", 1.0), ("ms", 0.75), ("ms", 1.0)])
def test_oracle_pairwise_sum_equals_numpy(oracle, algo, norm):
    """widecols has variables of degree 2..128 (every branch of NumPy's pairwise
    add.reduce up to its 128-term block): the C oracle against np.sum itself,
    2 frames, 20 iterations, no early stop."""
    from oracle import refnumpy
    H, rp, ci = C.code("widecols")
    llr = C.awgn_llrs("widecols")[:2]
    want, _ = refnumpy.ldpc_batch(H, llr, algo, 20, False, norm)
    got, its = oracle.ldpc_decode(rp, ci, H.shape[1], llr, algo, 20, False, norm)
    assert np.array_equal(got, want) and np.array_equal(its, [20, 20])

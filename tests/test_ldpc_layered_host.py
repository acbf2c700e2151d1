"""Host side of the layered min-sum decoder (no GPU): the default layer
schedule, the plan creator's argument checks (made before any device work) and
the NumPy restatement the GPU tests compare against."""
import ctypes

import numpy as np
import pytest

from layered_ref import awgn_llrs, check_rows, layered_ms_literal, layered_ms_ref


def _L():
    import polarcode_and_ldpc_amd.ldpc as L
    return L


@pytest.mark.parametrize("n,dv,dc,seed,sizes", [
    (96, 3, 6, 96, [9, 8, 8, 8, 5, 6, 3, 1]),
    (504, 3, 6, 3, [43, 43, 39, 43, 36, 26, 13, 9]),
    (480, 4, 8, 484, None),
])
def test_layer_schedule_first_fit(n, dv, dc, seed, sizes):
    L = _L()
    H = L.regular_construction(n, dv, dc, seed=seed)
    H[5] = 0  # a zero-degree row lands in layer 0
    layers = L.layer_schedule(H)
    if sizes is not None:
        assert [len(l) for l in L.layer_schedule(L.regular_construction(n, dv, dc, seed=seed))] == sizes
    else:
        full = L.layer_schedule(L.regular_construction(n, dv, dc, seed=seed))
        assert len(full) == 12 and max(len(l) for l in full) == 29
    m = H.shape[0]
    assert np.array_equal(np.sort(np.concatenate(layers)), np.arange(m))  # a partition of the rows
    assert 5 in layers[0]
    where = np.empty(m, dtype=int)
    for i, l in enumerate(layers):
        where[l] = i
        assert (H[l].sum(axis=0) <= 1).all()  # variable-disjoint
    # first fit: every earlier layer holds an earlier row that shares a column with c
    for c in range(m):
        for i in range(where[c]):
            earlier = layers[i][layers[i] < c]
            assert (H[earlier] @ H[c]).any(), (c, i)


def _create(rp, ci, n, layers, max_iter=5):
    from polarcode_and_ldpc_amd import _native
    rp = np.ascontiguousarray(rp, np.int32)
    ci = np.ascontiguousarray(ci, np.int32)
    lp = np.zeros(len(layers) + 1, np.int32)
    lp[1:] = np.cumsum([len(l) for l in layers])
    lr = np.ascontiguousarray(np.concatenate([np.asarray(l, np.int32) for l in layers]), np.int32)
    h = ctypes.c_void_p()
    P = ctypes.c_void_p
    rc = _native.lib.pl_ldpc_layered_plan_create(len(rp) - 1, n, rp.ctypes.data_as(P), ci.ctypes.data_as(P), len(layers),
                                                 lp.ctypes.data_as(P), lr.ctypes.data_as(P), max_iter, 1, 0.75, 0,
                                                 ctypes.byref(h))
    if rc == 0:
        _native.lib.pl_plan_destroy(h)
    return rc, _native.lib.pl_last_error()


def test_layered_plan_argument_errors():
    """Layer validation returns before any device work."""
    from polarcode_and_ldpc_amd import _native
    assert _native.PL_LDPC_LMS == 2
    # H: rows 0 and 1 share column 1; rows 0 and 2 are disjoint
    rows = [[0, 1], [1, 2], [2, 3], [4, 5]]
    rp = np.cumsum([0] + [len(r) for r in rows])
    ci = np.concatenate(rows)
    assert _create(rp, ci, 6, [[0, 3], [1], [2]])[0] != _native.PL_EINVAL  # valid layers pass the checks
    rc, msg = _create(rp, ci, 6, [[0, 3], [1], [1]])  # row 1 twice (in place of row 2)
    assert rc == _native.PL_EINVAL and b"row 1 repeats" in msg
    rc, msg = _create(rp, ci, 6, [[0, 3], [1], [2], [0]])  # row 0 twice (one entry too many)
    assert rc == _native.PL_EINVAL and b"exactly once" in msg
    rc, msg = _create(rp, ci, 6, [[0, 3], [1]])  # row 2 missing
    assert rc == _native.PL_EINVAL and b"exactly once" in msg
    rc, msg = _create(rp, ci, 6, [[0, 1], [2, 3]])  # rows 0 and 1 share column 1
    assert rc == _native.PL_EINVAL and b"share column 1" in msg
    bad_rp = np.array(rp)
    bad_rp[2] = rp[-1] + 1000  # a middle entry past the end: refused before col_idx is read there
    rc, msg = _create(bad_rp, ci, 6, [[0, 3], [1], [2]])
    assert rc == _native.PL_EINVAL and b"monotone" in msg
    rows1 = [[0, 1], [3], [2, 3], [4, 5]]  # a degree-1 row
    rc, msg = _create(np.cumsum([0] + [len(r) for r in rows1]), np.concatenate(rows1), 6, [[0, 1, 3], [2]])
    assert rc == _native.PL_EUNSUPPORTED and b"degree-1" in msg


def test_restatement_serial_schedule_equals_literal_loop():
    L = _L()
    H = L.regular_construction(96, 3, 6, seed=96)
    H[7] = 0
    llr = awgn_llrs(96, 6, 1.0, seed=5)
    llr[1, 3] = np.nan
    llr[2, 10] = 0.0
    llr[3, 20] = np.inf
    serial = [[c] for c in range(H.shape[0])]
    for norm, es, mi in ((0.75, True, 20), (1.0, False, 3), (0.75, True, 0)):
        bits, its, post = layered_ms_ref(H, llr, serial, mi, norm, es)
        for f in range(len(llr)):
            b, i, p = layered_ms_literal(H, llr[f], mi, norm, es)
            assert np.array_equal(bits[f], b) and its[f] == i
            assert np.array_equal(post[f], p, equal_nan=True)
    assert np.isnan(post[1]).any()


def test_restatement_noiseless_stops_at_one():
    L = _L()
    H = L.regular_construction(96, 3, 6, seed=96)
    assert [len(r) for r in check_rows(H)] == [6] * 48
    llr = np.full((3, 96), 4.0)
    bits, its, post = layered_ms_ref(H, llr, L.layer_schedule(H), 20, 0.75, True)
    assert not bits.any() and (its == 1).all() and (post > 4.0).all()
    # a degree-1 check is an empty minimum, as in MSDecoder
    H1 = H.copy()
    H1[0] = 0
    H1[0, 3] = 1
    with pytest.raises(ValueError, match="zero-size array"):
        layered_ms_ref(H1, llr, L.layer_schedule(H1), 2)

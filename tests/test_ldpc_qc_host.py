"""Quasi-cyclic LDPC on the host (no GPU): the base-matrix functions of
ldpc/matrix.py and the planner's qc_plan_build through its device-free window,
pl_debug_ldpc_qc_plan_probe.  The geometry and the FNV-1a digest of the layer
stream are pinned by tests/golden/ldpc_qc_plan_digests.json, recorded from the
build that introduced the plan."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

INT32 = 2 ** 31


def _L():
    import polarcode_and_ldpc_amd.ldpc as L
    return L


def _N():
    from polarcode_and_ldpc_amd import _native
    return _native


@functools.lru_cache(maxsize=None)
def _base(name):
    L = _L()
    if isinstance(name, int):  # the (4, 8) code of that Z, as tests/test_gpu_ldpc_qc.py
        return L.qc_random_base(4, 8, name, 3, seed=100 + name + 8)
    if name == "deg40":
        return L.qc_random_base(3, 40, 7, 3, seed=147)
    if name == "deg17_32":
        return L.qc_random_base(4, 24, 7, 3, seed=24)
    if name == "big":
        return L.qc_random_base(32, 64, 160, 3, seed=160)
    raise KeyError(name)


# id: (base, Z, lms_global, what the case is there for)
CASES = {
    "z1": (1, 1, 0, {"kernel": 11, "fpw": 64, "dcap": 8}),
    "z7": (7, 7, 0, {"kernel": 11, "fpw": 9, "dcap": 8}),
    "z27": (27, 27, 0, {"kernel": 11, "fpw": 2, "dcap": 8}),
    "z64": (64, 64, 0, {"kernel": 11, "fpw": 1, "dcap": 8}),
    "z96": (96, 96, 0, {"kernel": 11, "fpw": 1, "fpb": 1, "threads": 128, "dcap": 8}),
    "deg40_two_pass": ("deg40", 7, 0, {"kernel": 11, "maxdc": 40, "dcap": 0, "mw": 3}),
    "deg17_32_mw2": ("deg17_32", 7, 0, {"kernel": 11, "dcap": 32, "mw": 2}),
    "z27_forced_global": (27, 27, 1, {"kernel": 12, "use_global": 1, "lds_bytes": 0}),
    "z96_forced_global": (96, 96, 1, {"kernel": 12, "use_global": 1, "lds_bytes": 128}),
    "big_state_global": ("big", 160, 0, {"kernel": 12, "use_global": 1, "state_bytes": 184320, "threads": 192}),
}
FIELDS = ("kernel", "z", "mb", "nb", "maxdc", "dcap", "mw", "fpw", "fpb", "threads", "lds_bytes", "use_global",
          "state_bytes", "table_len")


def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def probe(base, Z, order=None, max_iter=20, lms_global=0):
    N = _N()
    sh = np.ascontiguousarray(base, dtype=np.int32)
    lo = None if order is None else np.ascontiguousarray(order, dtype=np.int32)
    out = N.LdpcQcPlanProbe()
    rc = N.lib.pl_debug_ldpc_qc_plan_probe(sh.shape[0], sh.shape[1], Z, _ptr(sh), _ptr(lo), max_iter, 1, 0.75,
                                           lms_global, ctypes.byref(out))
    return rc, out, (N.lib.pl_last_error() or b"").decode()


def probe_dict(case):
    name, Z, force, _ = CASES[case]
    rc, out, msg = probe(_base(name), Z, lms_global=force)
    assert rc == 0, msg
    got = {f: getattr(out, f) for f in FIELDS}
    got["digest"] = "%016x" % out.digest
    return got


# ---- the base-matrix functions ---------------------------------------------------
@pytest.mark.parametrize("name,Z", [(1, 1), (7, 7), (27, 27), ("deg40", 7)])
def test_qc_expand_is_the_definition(name, Z):
    L = _L()
    base = _base(name)
    mb, nb = base.shape
    H = np.zeros((mb * Z, nb * Z), dtype=int)
    for i in range(mb):
        for j in range(nb):
            for r in range(Z):
                if base[i, j] >= 0:
                    H[i * Z + r, j * Z + (r + base[i, j]) % Z] = 1
    got = L.qc_expand(base, Z)
    assert got.shape == H.shape and np.array_equal(got, H)
    assert np.array_equal(got.sum(axis=1), np.repeat((base >= 0).sum(axis=1), Z))


@pytest.mark.parametrize("name,Z", [(1, 1), (7, 7), (27, 27), (96, 96), ("deg40", 7), ("deg17_32", 7)])
def test_qc_to_csr_equals_dense_to_csr(name, Z):
    L = _L()
    base = np.array(_base(name))
    if name == 27:
        base[2] = -1  # an empty block row
    rp, ci = L.qc_to_csr(base, Z)
    rp2, ci2 = L.dense_to_csr(L.qc_expand(base, Z))
    assert rp.dtype == rp2.dtype == np.int32 and ci.dtype == ci2.dtype == np.int32
    assert np.array_equal(rp, rp2) and np.array_equal(ci, ci2)


def test_block_layers_are_variable_disjoint_and_accepted_by_the_layered_planner():
    L, N = _L(), _N()
    base, Z = _base(27), 27
    H = L.qc_expand(base, Z)
    assert [l.tolist() for l in L.qc_block_layers(4, Z)] == [list(range(i * Z, (i + 1) * Z)) for i in range(4)]
    order = [2, 0, 3, 1]
    layers = L.qc_block_layers(4, Z, order)
    assert [int(l[0]) // Z for l in layers] == order and all(len(l) == Z for l in layers)
    for l in layers:
        assert H[l].sum(axis=0).max() <= 1
    rp, ci = L.qc_to_csr(base, Z)
    lp = np.arange(5, dtype=np.int32) * Z
    lr = np.ascontiguousarray(np.concatenate(layers), np.int32)
    out = N.LdpcLayeredPlanProbe()
    rc = N.lib.pl_debug_ldpc_layered_plan_probe(4 * Z, 8 * Z, _ptr(rp), _ptr(ci), 4, _ptr(lp), _ptr(lr), 20, 1, 0.75,
                                                0, 0, 0, ctypes.byref(out))
    assert rc == 0, N.lib.pl_last_error()
    assert out.max_layer == Z and out.n_layers == 4
    # the two plans lay the state out alike
    rc, q, msg = probe(base, Z, order)
    assert rc == 0, msg
    assert (q.state_bytes, q.mw, q.maxdc) == (out.state_bytes, out.mw, out.maxdc)


def test_qc_random_base_is_reproducible():
    L = _L()
    for mb, nb, Z, dv, seed in ((4, 8, 7, 3, 115), (4, 8, 96, 3, 204), (3, 40, 7, 3, 147), (12, 24, 27, 3, 1)):
        a = L.qc_random_base(mb, nb, Z, dv, seed)
        assert np.array_equal(a, L.qc_random_base(mb, nb, Z, dv, seed))
        assert a.shape == (mb, nb) and a.min() >= -1 and a.max() < Z
        assert ((a >= 0).sum(axis=0) == dv).all() and ((a >= 0).sum(axis=1) >= 2).all()
    assert not np.array_equal(L.qc_random_base(4, 8, 7, 3, 115), L.qc_random_base(4, 8, 7, 3, 116))
    # the definition, spelled out
    rng = np.random.RandomState(115)
    while True:
        want = np.full((4, 8), -1)
        for j in range(8):
            rows = rng.choice(4, 3, replace=False)
            want[rows, j] = rng.randint(0, 7, 3)
        if ((want >= 0).sum(axis=1) >= 2).all():
            break
    assert np.array_equal(L.qc_random_base(4, 8, 7, 3, 115), want)
    assert ((_base("deg40") >= 0).sum(axis=1) == 40).all()


# ---- the planner -------------------------------------------------------------------
@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(GOLDEN, "ldpc_qc_plan_digests.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("case", sorted(CASES))
def test_qc_plan_equals_recorded(case, recorded):
    got = probe_dict(case)
    for k, v in CASES[case][3].items():
        assert got[k] == v, (k, got)
    assert set(recorded[case]) == set(FIELDS) | {"digest"}
    assert got == recorded[case]


def test_geometry():
    g = {c: probe_dict(c) for c in CASES}
    assert [g[c]["fpw"] for c in ("z1", "z7", "z27", "z64")] == [64, 9, 2, 1]
    for c in ("z1", "z7", "z27", "z64"):  # four wavefronts of fpw frames, state in LDS, no vote words
        assert g[c]["threads"] == 256 and g[c]["fpb"] == 4
        assert g[c]["lds_bytes"] == 4 * g[c]["fpw"] * g[c]["state_bytes"]
    assert g["z96"]["lds_bytes"] == g["z96"]["state_bytes"] + 128
    assert 17 <= g["deg17_32_mw2"]["maxdc"] <= 32
    assert g["big_state_global"]["state_bytes"] == 8 * 10240 + 20 * 5120 > 160 * 1024 - 128
    # per layer: block row, degree, (block column, shift) pairs
    for c in CASES:
        base = _base(CASES[c][0])
        assert g[c]["table_len"] == 2 * base.shape[0] + 2 * int((base >= 0).sum())
    # the state's home does not change the tables
    assert g["z27"]["digest"] == g["z27_forced_global"]["digest"]


def test_layer_order_reorders_the_stream():
    base = _base(27)
    d = {}
    for order in (None, [0, 1, 2, 3], [3, 1, 0, 2]):
        rc, out, msg = probe(base, 27, order)
        assert rc == 0, msg
        d[str(order)] = out.digest
    assert d["None"] == d["[0, 1, 2, 3]"] != d["[3, 1, 0, 2]"]
    # the digest is FNV-1a over the stream the header documents
    t = []
    for i in [3, 1, 0, 2]:
        cols = np.nonzero(base[i] >= 0)[0]
        t += [i, len(cols)] + [int(x) for j in cols for x in (j, base[i, j])]
    h = 14695981039346656037
    for byte in np.asarray(t, np.int32).tobytes():
        h = ((h ^ byte) * 1099511628211) % 2 ** 64
    assert h == d["[3, 1, 0, 2]"]


def test_refusals():
    N = _N()
    EINVAL, EUNSUPPORTED = N.PL_EINVAL, N.PL_EUNSUPPORTED
    base = np.array(_base(7))

    def refused(code, *a, **kw):
        rc, _, msg = probe(*a, **kw)
        assert rc == code and msg, (rc, msg)
        return msg

    out = N.LdpcQcPlanProbe()
    sh = np.ascontiguousarray(base, np.int32)
    for mb, nb, Z in ((0, 8, 7), (4, 0, 7), (4, 8, 0), (-1, 8, 7)):
        assert N.lib.pl_debug_ldpc_qc_plan_probe(mb, nb, Z, _ptr(sh), None, 20, 1, 1.0, 0, ctypes.byref(out)) == EINVAL
        assert N.lib.pl_last_error()
    two = np.zeros((1, 2), np.int32)
    refused(EINVAL, two, INT32 // 2)                      # nb Z = 2^31
    refused(EINVAL, np.zeros((2, 1), np.int32), INT32 // 2)  # mb Z = 2^31
    for bad in (-2, 7, 100):
        b = base.copy()
        b[1, 2] = bad
        assert "shift" in refused(EINVAL, b, 7)
    for order in ([0, 1, 2, 2], [0, 1, 2, 4], [-1, 0, 1, 2]):
        assert "permutation" in refused(EINVAL, base, 7, order)
    refused(EINVAL, base, 7, max_iter=-1)
    # a block row with one block: the layered plan's refusal, word for word; fine without an iteration
    b1 = base.copy()
    b1[0] = -1
    b1[0, 3] = 5
    msg = refused(EUNSUPPORTED, b1, 7)
    L = _L()
    rp, ci = L.qc_to_csr(b1, 7)
    lp = np.arange(5, dtype=np.int32) * 7
    lr = np.arange(28, dtype=np.int32)
    lout = N.LdpcLayeredPlanProbe()
    assert N.lib.pl_debug_ldpc_layered_plan_probe(28, 56, _ptr(rp), _ptr(ci), 4, _ptr(lp), _ptr(lr), 20, 1, 1.0, 0, 0,
                                                  0, ctypes.byref(lout)) == EUNSUPPORTED
    assert msg == N.lib.pl_last_error().decode() and "degree-1" in msg
    assert probe(b1, 7, max_iter=0)[0] == 0
    # a block row without blocks is allowed
    b0 = base.copy()
    b0[2] = -1
    rc, o, m = probe(b0, 7)
    assert rc == 0 and o.table_len == 2 * 4 + 2 * int((b0 >= 0).sum()), m
    assert "2048" in refused(EUNSUPPORTED, np.zeros((1, 2048), np.int32), 1)
    assert probe(np.zeros((1, 2047), np.int32), 1)[0] == 0
    assert "1024" in refused(EUNSUPPORTED, two, 1025)
    assert probe(two, 1024)[0] == 0
    # EINVAL comes first
    refused(EINVAL, two, 1025, max_iter=-1)

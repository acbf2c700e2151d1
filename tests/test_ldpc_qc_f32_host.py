"""The quasi-cyclic planner with PL_LDPC_QC_F32, on the host (no GPU), through
pl_debug_ldpc_qc_plan_probe_flags: flags = 0 is pl_debug_ldpc_qc_plan_probe; with
the flag the single-precision state layout (4 n + 8 m + 4 mw m bytes), the same
LDS rules on the new sizes, kernel codes 13 / 14, and the same layer stream."""
import ctypes
import functools

import numpy as np
import pytest

KB160 = 160 * 1024
INT32 = 2 ** 31
FIELDS = ("kernel", "z", "mb", "nb", "maxdc", "dcap", "mw", "fpw", "fpb", "threads", "lds_bytes", "use_global",
          "state_bytes", "table_len")
# id: (base, Z, lms_global, unused) -- the codes of tests/test_ldpc_qc_host.py, built the same way
CASES = {
    "z1": (1, 1, 0, None),
    "z7": (7, 7, 0, None),
    "z27": (27, 27, 0, None),
    "z64": (64, 64, 0, None),
    "z96": (96, 96, 0, None),
    "deg40_two_pass": ("deg40", 7, 0, None),
    "deg17_32_mw2": ("deg17_32", 7, 0, None),
    "z27_forced_global": (27, 27, 1, None),
    "z96_forced_global": (96, 96, 1, None),
    "big_state_global": ("big", 160, 0, None),
}


def _L():
    import polarcode_and_ldpc_amd.ldpc as L
    return L


def _N():
    from polarcode_and_ldpc_amd import _native
    return _native


@functools.lru_cache(maxsize=None)
def _base(name):
    L = _L()
    if isinstance(name, int):  # the (4, 8) code of that Z
        return L.qc_random_base(4, 8, name, 3, seed=100 + name + 8)
    return {"deg40": lambda: L.qc_random_base(3, 40, 7, 3, seed=147),
            "deg17_32": lambda: L.qc_random_base(4, 24, 7, 3, seed=24),
            "big": lambda: L.qc_random_base(32, 64, 160, 3, seed=160)}[name]()


def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def probe0(base, Z, order=None, max_iter=20, lms_global=0):
    """pl_debug_ldpc_qc_plan_probe, the call without flags."""
    N = _N()
    sh = np.ascontiguousarray(base, dtype=np.int32)
    lo = None if order is None else np.ascontiguousarray(order, dtype=np.int32)
    out = N.LdpcQcPlanProbe()
    rc = N.lib.pl_debug_ldpc_qc_plan_probe(sh.shape[0], sh.shape[1], Z, _ptr(sh), _ptr(lo), max_iter, 1, 0.75,
                                           lms_global, ctypes.byref(out))
    return rc, out, (N.lib.pl_last_error() or b"").decode()


def probe(base, Z, order=None, max_iter=20, lms_global=0, flags=1):
    N = _N()
    sh = np.ascontiguousarray(base, dtype=np.int32)
    lo = None if order is None else np.ascontiguousarray(order, dtype=np.int32)
    out = N.LdpcQcPlanProbe()
    rc = N.lib.pl_debug_ldpc_qc_plan_probe_flags(sh.shape[0], sh.shape[1], Z, _ptr(sh), _ptr(lo), max_iter, 1, 0.75,
                                                 lms_global, flags, ctypes.byref(out))
    return rc, out, (N.lib.pl_last_error() or b"").decode()


def as_dict(out):
    d = {f: getattr(out, f) for f in FIELDS}
    d["digest"] = out.digest
    return d


def state_bytes(m, n, mw):
    a16 = lambda b: (b + 15) // 16 * 16  # noqa: E731
    return a16(a16(4 * n) + 8 * m + 4 * m * mw)


def test_flag_value():
    assert _N().PL_LDPC_QC_F32 == 1


@pytest.mark.parametrize("case", sorted(CASES))
def test_flags_zero_is_the_plain_probe(case):
    name, Z, force, _ = CASES[case]
    rc0, a, msg0 = probe0(_base(name), Z, lms_global=force)
    for flags in (0, 2, 0x7ffffffe):  # the other bits are ignored
        rc1, b, msg1 = probe(_base(name), Z, lms_global=force, flags=flags)
        assert rc0 == rc1 == 0, (msg0, msg1)
        assert as_dict(a) == as_dict(b)


@pytest.mark.parametrize("case", sorted(CASES))
def test_f32_plan_of_each_case(case):
    name, Z, force, _ = CASES[case]
    base = _base(name)
    rc, a, msg = probe0(base, Z, lms_global=force)
    assert rc == 0, msg
    rc, b, msg = probe(base, Z, lms_global=force)
    assert rc == 0, msg
    # the layer stream does not depend on the precision, nor does the mapping of checks to threads
    assert (b.table_len, b.digest) == (a.table_len, a.digest)
    for f in ("z", "mb", "nb", "maxdc", "dcap", "mw", "fpw"):
        assert getattr(a, f) == getattr(b, f), f
    m, n = base.shape[0] * Z, base.shape[1] * Z
    sb = state_bytes(m, n, b.mw)
    assert b.state_bytes == sb < a.state_bytes
    if Z <= 64:
        wave = sb * b.fpw
        want_global = bool(force) or wave > KB160
        assert b.use_global == want_global and b.kernel == (14 if want_global else 13)
        assert b.fpb == (4 if want_global else max(1, min(4, 65536 // wave)))  # the 64 KB rule
        assert b.threads == 64 * b.fpb and b.lds_bytes == (0 if want_global else wave * b.fpb)
    else:
        want_global = bool(force) or sb + 128 > KB160
        assert b.use_global == want_global and b.kernel == (14 if want_global else 13)
        assert (b.fpw, b.fpb, b.threads) == (1, 1, (Z + 63) // 64 * 64)
        assert b.lds_bytes == (0 if want_global else sb) + 128


def test_f32_sizes_and_homes():
    L = _L()
    rc, o, msg = probe(_base(27), 27)
    assert rc == 0 and (o.kernel, o.state_bytes, o.fpw, o.fpb, o.lds_bytes) == (13, 2160, 2, 4, 8 * 2160), msg
    # forced to the workspace: no LDS but the block mapping's vote words
    rc, o, _ = probe(_base(27), 27, lms_global=1)
    assert rc == 0 and (o.kernel, o.use_global, o.lds_bytes) == (14, 1, 0)
    rc, o, _ = probe(_base(96), 96, lms_global=1)
    assert rc == 0 and (o.kernel, o.use_global, o.lds_bytes) == (14, 1, 128)
    # the 64 KB rule picks fewer wavefronts once fpw states no longer fit four times
    b = L.qc_random_base(16, 32, 64, 3, seed=1)  # n = 2048, m = 1024: 20 480 B in fp32, 36 864 B in fp64
    rc, o, _ = probe(b, 64)
    assert rc == 0 and (o.state_bytes, o.fpb, o.threads, o.lds_bytes) == (20480, 3, 192, 61440)
    rc, o, _ = probe(b, 64, flags=0)
    assert rc == 0 and (o.state_bytes, o.fpb, o.threads) == (36864, 1, 64)
    # (32, 64, 128), n = 8192: 147 456 B -> 81 920 B, both in LDS, one frame per workgroup
    b = L.qc_random_base(32, 64, 128, 3, seed=1)
    rc, o, _ = probe(b, 128, flags=0)
    assert rc == 0 and (o.kernel, o.state_bytes, o.lds_bytes) == (11, 147456, 147456 + 128)
    rc, o, _ = probe(b, 128)
    assert rc == 0 and (o.kernel, o.state_bytes, o.lds_bytes, o.threads) == (13, 81920, 81920 + 128, 128)
    assert 2 * o.lds_bytes == 164096 > KB160  # known: two workgroups per CU miss the LDS by the vote words
    # (32, 64, 160): the workspace in fp64, LDS in fp32
    rc, o, _ = probe(_base("big"), 160, flags=0)
    assert rc == 0 and (o.kernel, o.state_bytes) == (12, 184320)
    rc, o, _ = probe(_base("big"), 160)
    assert rc == 0 and (o.kernel, o.use_global, o.state_bytes, o.lds_bytes) == (13, 0, 102400, 102400 + 128)
    # (32, 64, 320): 204 800 B, the workspace in fp32 as well (planner only)
    b = L.qc_random_base(32, 64, 320, 3, seed=320)
    rc, o, _ = probe(b, 320)
    assert rc == 0 and (o.kernel, o.use_global, o.state_bytes, o.lds_bytes, o.threads) == (14, 1, 204800, 128, 320)


def test_refusals_are_the_same_with_the_flag():
    N = _N()
    base = np.array(_base(7))
    two = np.zeros((1, 2), np.int32)
    b_shift = base.copy()
    b_shift[1, 2] = 7
    b1 = base.copy()
    b1[0] = -1
    b1[0, 3] = 5
    cases = [
        (two, INT32 // 2, {}),
        (np.zeros((2, 1), np.int32), INT32 // 2, {}),
        (b_shift, 7, {}),
        (base, 7, {"order": [0, 1, 2, 2]}),
        (base, 7, {"max_iter": -1}),
        (b1, 7, {}),
        (np.zeros((1, 2048), np.int32), 1, {}),
        (two, 1025, {}),
        (two, 1025, {"max_iter": -1}),
    ]
    codes = []
    for b, Z, kw in cases:
        rc0, _, msg0 = probe0(b, Z, **kw)
        rc1, _, msg1 = probe(b, Z, **kw)
        assert rc0 == rc1 and rc0 in (N.PL_EINVAL, N.PL_EUNSUPPORTED) and msg0 == msg1 and msg0, (rc0, rc1, msg0, msg1)
        codes.append(rc0)
    assert codes == [N.PL_EINVAL] * 5 + [N.PL_EUNSUPPORTED] * 3 + [N.PL_EINVAL]
    out = N.LdpcQcPlanProbe()
    sh = np.ascontiguousarray(base, np.int32)
    for mb, nb, Z in ((0, 8, 7), (4, 0, 7), (4, 8, 0), (-1, 8, 7)):
        assert N.lib.pl_debug_ldpc_qc_plan_probe_flags(mb, nb, Z, _ptr(sh), None, 20, 1, 1.0, 0, 1,
                                                       ctypes.byref(out)) == N.PL_EINVAL
    assert N.lib.pl_debug_ldpc_qc_plan_probe_flags(4, 8, 7, _ptr(sh), None, 20, 1, 1.0, 0, 1, None) == N.PL_EINVAL
    # what is allowed stays allowed
    assert probe(b1, 7, max_iter=0)[0] == 0
    assert probe(np.zeros((1, 2047), np.int32), 1)[0] == 0
    assert probe(two, 1024)[0] == 0

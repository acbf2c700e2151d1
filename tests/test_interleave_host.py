"""The bit interleaver, everything that needs no GPU: the definition's loops (tests/interleave_ref.py) are a
bijection; channel.BitInterleaver's permutation() and host methods and pl_interleave_index (the code the
kernels run) equal them bit for bit; large sizes through pl_interleave_index against an independent count;
pl_interleave_check's refusals in the stated order.

The definition: include/polarldpc.h at pl_interleave_check.  llr_payload() is the input set the GPU tests
share (tests/test_gpu_interleave.py)."""
import ctypes
import functools

import numpy as np
import pytest

import interleave_ref as R
from polarcode_and_ldpc_amd import _native
from polarcode_and_ldpc_amd.channel import BitInterleaver, QAMModem

KIND = {"rect": _native.PL_ILV_RECT, "tri": _native.PL_ILV_TRI}
TRI_ES = range(1, 601)
RECT_ES = range(1, 301)


@functools.lru_cache(maxsize=None)
def ref_positions(kind, rows, E):
    return np.array(R.positions(kind, rows, E), dtype=np.int64)


def cases():
    for E in TRI_ES:
        yield "tri", 0, E
    for E in RECT_ES:
        for rows in R.RECT_ROWS:
            yield "rect", rows, E


def make(kind, rows, E):
    return BitInterleaver(kind, E, rows=rows if kind == "rect" else None)


def llr_payload(shape, dtype, seed=0):
    """floats of `dtype` with every kind of value a copy must not change: NaNs of several payloads and both
    signs, +-inf, +-0.0, denormals, the largest and smallest normals, and random bit patterns"""
    dtype = np.dtype(dtype)
    u = np.dtype("u%d" % dtype.itemsize)
    rng = np.random.default_rng(seed + dtype.itemsize)
    bits = rng.integers(0, np.iinfo(u).max, size=shape, dtype=u, endpoint=True)
    fi = np.finfo(dtype)
    sp = np.array([np.nan, -np.nan, np.inf, -np.inf, 0.0, -0.0, fi.tiny, -fi.tiny, fi.max, fi.min,
                   fi.smallest_subnormal, -fi.smallest_subnormal, fi.tiny / 2, 1.0, -1.5], dtype=dtype).view(u)
    quiet = np.array([1], dtype=u) << (fi.nmant - 1)
    nan_payloads = (np.array([np.inf], dtype=dtype).view(u) | quiet | np.array([1, 2, 0x155], dtype=u))
    sp = np.concatenate([sp, nan_payloads, nan_payloads ^ (np.array([1], dtype=u) << (8 * dtype.itemsize - 1)),
                         np.array([np.inf], dtype=dtype).view(u) | np.array([1], dtype=u)])  # a signalling NaN
    flat = bits.reshape(-1)
    n = min(len(sp), flat.size)
    flat[:n] = sp[:n]
    flat[flat.size - n:] = sp[:n][::-1]
    return bits.view(dtype)


def raw(a):
    a = np.ascontiguousarray(a)
    return a.view("u%d" % a.dtype.itemsize)


def test_reference_is_a_bijection():
    for kind, rows, E in cases():
        order = R.output_order(kind, rows, E)
        assert sorted(order) == list(range(E)), (kind, rows, E)


def test_reference_shapes():
    """the definition's own statements: RECT with rows = 1 and E <= rows is the identity; TRI's first
    column is the row starts; with E = T (T + 1) / 2 the last column is one cell"""
    assert R.output_order("rect", 1, 17) == list(range(17))
    assert R.output_order("rect", 64, 9) == list(range(9))
    assert R.output_order("rect", 3, 7) == [0, 3, 6, 1, 4, 2, 5]  # C = 3: rows 012 345 6
    assert R.output_order("tri", 0, 6) == [0, 3, 5, 1, 4, 2]  # T = 3: rows 012 34 5
    assert R.output_order("tri", 0, 5) == [0, 3, 1, 4, 2]
    assert R.output_order("tri", 0, 4) == [0, 3, 1, 2]  # the last row is empty


def test_permutation_and_index_equal_the_loops():
    for kind, rows, E in cases():
        want = ref_positions(kind, rows, E)
        il = make(kind, rows, E)
        assert il.dim == (R.tri_T(E) if kind == "tri" else -(-E // rows)), (kind, rows, E)
        got = il.permutation()
        assert got.dtype == np.int64 and np.array_equal(got, want), (kind, rows, E)
        pos = ctypes.c_int64()
        for k in range(E):  # the C entry point, the code the kernels run, at every k
            assert _native.lib.pl_interleave_index(KIND[kind], rows, E, k, ctypes.byref(pos)) == 0
            assert pos.value == want[k], (kind, rows, E, k)


def test_host_methods_equal_the_loops():
    rng = np.random.default_rng(5)
    for kind, rows, E in cases():
        il = make(kind, rows, E)
        order, want = R.output_order(kind, rows, E), ref_positions(kind, rows, E).tolist()
        e = rng.integers(0, 256, size=(2, E), dtype=np.uint8)
        f = il.interleave_host(e)
        assert f.dtype == np.uint8
        for b in range(2):
            assert f[b].tolist() == [e[b, k] for k in order], (kind, rows, E)
        assert np.array_equal(il.interleave_host(e[0]), f[0])
        for dt in (np.float64, np.float32):
            llr = llr_payload((2, E), dt, seed=E)
            g = il.deinterleave_host(llr)
            assert g.dtype == dt
            for b in range(2):
                bits = raw(llr[b]).tolist()
                assert raw(g[b]).tolist() == [bits[p] for p in want], (kind, rows, E, dt)
            # deinterleaving after interleaving is the identity, on raw bits
            assert np.array_equal(raw(il.deinterleave_host(il.interleave_host(raw(llr)).view(dt))), raw(llr))
        assert np.array_equal(il.deinterleave_host(f), e)


def test_rect_puts_bit_r_of_symbol_s_at_row_r():
    for m in (2, 4, 6, 8):
        for S in (1, 2, 5, 33):
            E = m * S
            il = BitInterleaver.for_modem(QAMModem(m), E)
            assert (il.kind, il.rows, il.dim) == ("rect", m, S)
            e = np.arange(E, dtype=np.int64)
            f = il.interleave_host(e).reshape(S, m)
            for s in range(S):
                for r in range(m):
                    assert f[s, r] == e[r * S + s]


def tri_E(T):
    return T * (T + 1) // 2


LARGE = [("tri", 0, E) for E in (1 << 30, (1 << 30) - 1, tri_E(1000) - 1, tri_E(1000), tri_E(1000) + 1,
                                 tri_E(46340) - 1, tri_E(46340), tri_E(46340) + 1)] + \
        [("rect", rows, E) for rows in (3, 8) for E in (1 << 30, (1 << 30) - 1)]


@pytest.mark.parametrize("kind,rows,E", LARGE, ids=lambda v: str(v))
def test_large_sizes_against_the_column_count(kind, rows, E):
    assert E <= 1 << 30
    ref = R.ByColumns(kind, rows, E)
    dim = _native.interleave_check(KIND[kind], rows, E)
    assert dim == (ref.T if kind == "tri" else ref.C)
    rng = np.random.default_rng(E % 1000003 + rows)
    ks = sorted(set(range(64)) | set(range(E - 64, E)) | set(int(k) for k in rng.integers(0, E, 4096)))
    for k in ks:
        assert _native.interleave_index(KIND[kind], rows, E, k) == ref.pos(k), (kind, rows, E, k)
    # pos is strictly increasing along each column: down the first and the last columns of the first rows,
    # and down the columns of the random k
    for k in ks[:64] + ks[-64:] + ks[64:96]:
        i, c = ref.cell(k)
        col = [st + c for st in ref.starts if st + c < E]
        if kind == "tri":
            col = col[:ref.T - c]
        near = col[max(0, i - 3):i + 4]
        got = [_native.interleave_index(KIND[kind], rows, E, x) for x in near]
        assert all(b == a + 1 for a, b in zip(got, got[1:])), (kind, rows, E, k)


def test_small_ByColumns_equals_the_loops():
    """the independent count itself, where the loops can check it"""
    for kind, rows, E in cases():
        if E % 3 == 0 or E < 20:
            ref = R.ByColumns(kind, rows, E)
            assert [ref.pos(k) for k in range(E)] == ref_positions(kind, rows, E).tolist(), (kind, rows, E)


def test_check_refusals_in_order():
    lib = _native.lib

    def refused(kind, rows, E, word):
        rc = lib.pl_interleave_check(kind, rows, E, None)
        msg = (lib.pl_last_error() or b"").decode()
        assert rc == _native.PL_EINVAL and msg.startswith(word), (kind, rows, E, msg)

    RECT, TRI = _native.PL_ILV_RECT, _native.PL_ILV_TRI
    for kind in (-1, 2, 7):
        refused(kind, 99, 0, "kind = ")  # everything wrong: the kind is named
    for kind, rows in ((RECT, 0), (RECT, 65), (TRI, 1)):
        for E in (0, -1, (1 << 30) + 1):
            refused(kind, rows, E, "E = ")  # E before rows
    for rows in (0, -1, 65):
        refused(RECT, rows, 10, "rows = ")
    for rows in (1, -1, 64):
        refused(TRI, rows, 10, "rows = ")
    assert lib.pl_interleave_check(RECT, 64, 1, None) == 0 and lib.pl_interleave_check(TRI, 0, 1 << 30, None) == 0
    assert _native.interleave_check(RECT, 1, 1 << 30) == 1 << 30
    # pl_interleave_index: k outside 0 .. E-1
    pos = ctypes.c_int64(-7)
    for k in (-1, 10, 1 << 40):
        assert lib.pl_interleave_index(RECT, 4, 10, k, ctypes.byref(pos)) == _native.PL_EINVAL and pos.value == -7
        assert (lib.pl_last_error() or b"").decode().startswith("k = ")
    assert lib.pl_interleave_index(RECT, 4, 10, 0, None) == _native.PL_EINVAL
    # the Python class: AssertionError naming the condition, and no device call to make one
    for args, word in ((("rect", 10, 0), "rows"), (("rect", 10, 65), "rows"), (("tri", 10, 3), "rows"),
                       (("rect", 0, 4), "E = "), (("tri", (1 << 30) + 1), "E = "), (("diag", 10), "kind"),
                       (("rect", 10), "rows")):
        with pytest.raises(AssertionError, match=word):
            BitInterleaver(*args)
    assert _native.ILV_LDS_MAX_E[1] >= _native.ILV_LDS_MAX_E[4] >= _native.ILV_LDS_MAX_E[8] >= 1

"""The NumPy restatement of the int8 fixed-point quasi-cyclic decoder
(tests/qc_fixed_ref.py) pinned on the CPU: where no clamp acts it is the fp64
restatement at normalisation 1.0 value for value; a hand-worked example makes
each of the three clamps act once; the quantiser's edges, for the restatement and
for the package's quantize_host."""
import functools

import numpy as np
import pytest

from qc_fixed_ref import qc_fixed_ms_ref, quantize_ref
from qc_layered_ref import qc_layered_ms_ref

B = 67
SHAPES = [(4, 8, 7), (4, 8, 27), (6, 12, 96)]


def _L():
    import polarcode_and_ldpc_amd.ldpc as L
    return L


@functools.lru_cache(maxsize=None)
def integer_case(mb, nb, Z):
    """(base, L int8 [B, n], the fixed restatement's result at (16, 127, 127), 20 iterations, early stop):
    uniform integer LLRs of the largest amplitude <= 8 at which no clamp acts.  Shared with the device
    test's cross-check against the fp64 kernel."""
    base = _L().qc_random_base(mb, nb, Z, 3, seed=300 + Z)
    for amp in range(8, 0, -1):
        L = np.random.RandomState(400 + Z).randint(-amp, amp + 1, (B, nb * Z)).astype(np.int8)
        got = qc_fixed_ms_ref(base, Z, L, 20, 16, 127, 127, True)
        if not any(got[3].values()):
            break
    for a in (base, L) + got[:3]:
        a.setflags(write=False)
    return base, L, got, amp


@pytest.mark.parametrize("mb,nb,Z", SHAPES)
def test_equals_fp64_restatement_where_no_clamp_acts(mb, nb, Z):
    base, L, (bits, its, post, clamps), amp = integer_case(mb, nb, Z)
    print((mb, nb, Z), "amplitude", amp, "clamps", clamps, "max |P|", int(np.abs(post.astype(np.int64)).max()),
          "iterations", np.bincount(its, minlength=21))
    assert clamps == {"llr": 0, "msg": 0, "sat": 0} and amp >= 1
    assert np.abs(post.astype(np.int64)).max() < 127
    wb, wi, wp = qc_layered_ms_ref(base, Z, L.astype(np.float64), 20, 1.0, True)
    assert np.array_equal(bits, wb) and np.array_equal(its, wi)
    assert np.array_equal(post.astype(np.float64), wp)


def test_hand_worked_saturation():
    """Z = 1, two block rows, one iteration, norm16 = 16, llr_max = 127, msg_max = 100:
         L = [-128, -5, 3, -2]        P = [-127, -5, 3, -2]                       the llr clamp, once
         row 0 (v0, v1): q = [-127, -5]
             j = 0: min 5, one negative other    -> R = -5,   P0 = clamp(-132) = -127     the 127 clamp, once
             j = 1: min 127 -> 100, one negative -> R = -100, P1 = -105                   the msg clamp, once
         row 1 (v2, v3): q = [3, -2]
             j = 0: min 2, one negative other    -> R = -2,   P2 = 1
             j = 1: min 3, no negative other     -> R = +3,   P3 = 1
       decisions [1, 1, 0, 0]: both parities even."""
    base = np.array([[0, 0, -1, -1], [-1, -1, 0, 0]])
    L = np.array([[-128, -5, 3, -2]], dtype=np.int8)
    for early_stop in (False, True):
        bits, its, post, clamps = qc_fixed_ms_ref(base, 1, L, 1, 16, 127, 100, early_stop)
        assert post.dtype == np.int8 and post.tolist() == [[-127, -105, 1, 1]]
        assert bits.tolist() == [[1, 1, 0, 0]] and its.tolist() == [1]
        assert clamps == {"llr": 1, "msg": 1, "sat": 1}
    # the second iteration: row 0 q = [-127 + 5, -105 + 100] = [-122, -5] -> R = [-5, -100], P = [-127, -105];
    # row 1 q = [1 + 2, 1 - 3] = [3, -2] as before.  A fixed point, with early stop off: two more clamps
    bits, its, post, clamps = qc_fixed_ms_ref(base, 1, L, 2, 16, 127, 100, False)
    assert post.tolist() == [[-127, -105, 1, 1]] and its.tolist() == [2]
    assert clamps == {"llr": 1, "msg": 2, "sat": 1}
    # max_iter = 0: the clamped input, no iteration
    bits, its, post, clamps = qc_fixed_ms_ref(base, 1, L, 0, 16, 127, 100, True)
    assert post.tolist() == [[-127, -5, 3, -2]] and bits.tolist() == [[1, 1, 0, 1]] and its.tolist() == [0]


QUANT = [  # (llr, scale, llr_max, expected)
    (0.125, 4.0, 31, 0), (-0.125, 4.0, 31, 0),      # +-0.5 / scale: the tie goes to the even 0
    (0.375, 4.0, 31, 2), (-0.375, 4.0, 31, -2),     # 1.5 -> 2
    (0.625, 4.0, 31, 2), (-0.625, 4.0, 31, -2),     # 2.5 -> 2
    (0.875, 4.0, 31, 4), (0.126, 4.0, 31, 1), (0.124, 4.0, 31, 0),
    (float("nan"), 4.0, 31, 0), (float("inf"), 4.0, 31, 31), (-float("inf"), 4.0, 31, -31),
    (7.75, 4.0, 31, 31), (7.8, 4.0, 31, 31), (-7.9, 4.0, 31, -31), (1e300, 4.0, 127, 127), (-1e300, 1e300, 127, -127),
    (100.0, 8.0, 127, 127), (-16.0, 8.0, 127, -127), (15.9, 8.0, 127, 127), (15.8, 8.0, 127, 126),
    (0.0, 4.0, 31, 0), (-0.0, 4.0, 31, 0), (5e-324, 4.0, 31, 0),
]


@pytest.mark.parametrize("which", ["restatement", "package"])
def test_quantiser_edges(which):
    q = quantize_ref if which == "restatement" else _L().quantize_host
    for v, scale, lim, want in QUANT:
        got = q(np.array([[v]], dtype=np.float64), scale, lim)
        assert got.dtype == np.int8 and got.shape == (1, 1) and int(got[0, 0]) == want, (v, scale, lim, int(got[0, 0]))
        if abs(v) < 1e30 or v != v:  # what float32 holds exactly (every value above but the huge ones and 5e-324)
            f = np.array([[v]], dtype=np.float32)
            if float(f[0, 0]) == v or v != v:
                assert int(q(f, scale, lim)[0, 0]) == want, ("float32", v)
    # float32 input is widened, the product is a double's: float32(5) * 0.1 is 0.5 -> 0 in double,
    # 0.50000000745 -> 1 with the scale rounded to float32
    assert int(q(np.array([[5.0]], dtype=np.float32), 0.1, 31)[0, 0]) == 0
    assert int(q(np.array([[15.0]], dtype=np.float32), 0.1, 31)[0, 0]) == 2  # 1.5 -> 2
    # float32 specials and a whole array at once
    f = np.array([[np.nan, np.inf, -np.inf, 3.4e38, -3.4e38, 1e-45]], dtype=np.float32)
    assert q(f, 4.0, 31).tolist() == [[0, 31, -31, 31, -31, 0]]
    rs = np.random.RandomState(9)
    x = rs.standard_normal((5, 33)) * 6.0
    assert np.array_equal(quantize_ref(x, 4.0, 31), _L().quantize_host(x, 4.0, 31))
    assert np.array_equal(quantize_ref(x.astype(np.float32), 8.0, 127), _L().quantize_host(x.astype(np.float32), 8.0, 127))

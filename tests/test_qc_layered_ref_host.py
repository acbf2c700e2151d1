"""tests/qc_layered_ref.py (the block-row-vectorised restatement from the base
matrix) held to tests/layered_ref.py and tests/layered_ref32.py on the expanded
H with the block rows as layers (no GPU): hard decisions and iteration counts
array_equal, posteriors array_equal with equal_nan, in both precisions.  The two
share no code: this one never sees H, those never see the base matrix."""
import functools

import numpy as np
import pytest

from layered_ref import awgn_llrs, layered_ms_ref
from layered_ref32 import layered_ms_ref32
from qc_layered_ref import qc_layered_ms_ref

FRAMES = 12


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


# name -> (base, Z, layer_order); the bases are those of tests/test_gpu_ldpc_qc.py
@functools.lru_cache(maxsize=None)
def _case(name):
    L = _L()
    order = None
    if isinstance(name, int):
        base, Z = L.qc_random_base(4, 8, name, 3, seed=100 + name + 8), name
    elif name == "z7_permuted":
        base, Z, order = L.qc_random_base(4, 8, 7, 3, seed=115), 7, (2, 0, 3, 1)
    elif name == "deg40":
        base, Z = L.qc_random_base(3, 40, 7, 3, seed=147), 7
    elif name == "deg12":
        base, Z = _rows_base([12, 5, 9], 20, 7, seed=12), 7
    elif name == "deg24":
        base, Z = _rows_base([12, 24, 3, 32], 32, 7, seed=24), 7
    elif name in ("empty_row", "empty_row_permuted"):
        base, Z = np.insert(L.qc_random_base(4, 8, 27, 3, seed=135), 2, -1, axis=0), 27
        assert ((base >= 0).sum(axis=1) == 0).tolist() == [False, False, True, False, False]
        order = (3, 0, 4, 2, 1) if name == "empty_row_permuted" else None
    else:
        raise KeyError(name)
    base.setflags(write=False)
    return base, Z, order


@functools.lru_cache(maxsize=None)
def _frames(name):
    """Noisy frames at two SNRs, then: a punctured block column, an inf run, a NaN, +-0, 5e-324,
    and one frame with all of them."""
    base, Z, _ = _case(name)
    n = base.shape[1] * Z
    llr = np.concatenate([awgn_llrs(n, FRAMES // 2, -4.0, seed=31), awgn_llrs(n, FRAMES - FRAMES // 2, 3.0, seed=32)])
    run = slice(n - Z // 2 - 3, n)
    llr[6, Z:2 * Z] = 0.0
    llr[7, run] = np.inf
    llr[8, (3 * Z + 1) % n] = np.nan
    llr[9, [0, n // 2]] = [-0.0, 0.0]
    llr[10, [1 % n, n - 1]] = [5e-324, -5e-324]
    llr[11, :Z] = 0.0
    llr[11, run] = np.inf
    llr[11, n // 2] = np.nan
    llr[11, n // 2 - 1] = -0.0
    llr[11, n // 2 + 1] = 5e-324
    llr.setflags(write=False)
    return llr


CASES = [1, 2, 7, 33, "z7_permuted", "deg12", "deg24", "deg40", "empty_row", "empty_row_permuted"]


@pytest.mark.parametrize("max_iter", [0, 1, 20])
@pytest.mark.parametrize("early_stop", [True, False])
@pytest.mark.parametrize("name", CASES)
def test_equals_the_expanded_restatements(name, early_stop, max_iter):
    L = _L()
    base, Z, order = _case(name)
    llr = _frames(name)
    H = L.qc_expand(base, Z)
    layers = L.qc_block_layers(base.shape[0], Z, order)
    for dtype, ref in ((np.float64, layered_ms_ref), (np.float32, layered_ms_ref32)):
        want = ref(H, llr, layers, max_iter, 0.75, early_stop)
        got = qc_layered_ms_ref(base, Z, llr, max_iter, 0.75, early_stop, layer_order=order, dtype=dtype)
        assert got[0].dtype == np.int64 and got[1].dtype == np.int64 and got[2].dtype == dtype == want[2].dtype
        assert np.array_equal(got[0], want[0])
        assert np.array_equal(got[1], want[1])
        assert np.array_equal(got[2], want[2], equal_nan=True)
        if max_iter == 20 and early_stop and isinstance(name, int) and name > 2:
            assert got[1].min() < 20 and got[1].max() == 20  # both ends of the early stop are exercised
        if max_iter == 20 and not early_stop:
            assert np.isnan(got[2][8]).any() and np.isnan(got[2][11]).any()


def test_layer_order_changes_the_result():
    """The permuted cases above would pass with layer_order ignored by both sides only if it made no difference."""
    base, Z, order = _case("empty_row_permuted")
    llr = _frames("empty_row_permuted")[:6]
    a = qc_layered_ms_ref(base, Z, llr, 3, 0.75, False)
    b = qc_layered_ms_ref(base, Z, llr, 3, 0.75, False, layer_order=order)
    assert all(not np.array_equal(a[2][f], b[2][f]) for f in range(6))


def test_float32_is_not_float64_rounded():
    base, Z, _ = _case(33)
    llr = _frames(33)[:6]
    a = qc_layered_ms_ref(base, Z, llr, 20, 0.75, False)[2].astype(np.float32)
    b = qc_layered_ms_ref(base, Z, llr, 20, 0.75, False, dtype=np.float32)[2]
    assert b.dtype == np.float32 and not np.array_equal(a, b, equal_nan=True)

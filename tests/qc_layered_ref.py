"""A second NumPy restatement of the layered normalised min-sum decoder, for
quasi-cyclic codes, written from the base matrix alone (tests/layered_ref.py is
the first; this one shares no code with it or with the package and never
expands H).  H[i Z + r, j Z + (r + s) % Z] = 1 for every block base[i, j] = s
>= 0; the layers are the block rows, visited in layer_order:

    P[v] = llr[v];  R[i][r, j] = 0
    for it in range(max_iter):
        for i in layer_order (block rows with at least one block):
            V[r, j] = col_j Z + (r + s_j) % Z            # col_j ascending: the CSR position
            q = P[V] - R[i]                              # [Z, d], all Z checks of the block row at once
            R[i][r, j] = np.prod(np.sign(q[r, others])) * np.min(np.abs(q[r, others])) * normalization
            P[V] = q + R[i]
        decoded = P <= 0
        if early_stop and every block row's Z parities are even: iterations = it + 1; break

The Z checks of a block row share no variable (every block is a permutation),
so updating them together is the serial order.  A block row without blocks
takes part in neither the updates nor the syndrome.  dtype=np.float32: P, R,
q and the normalisation are float32 and every step is one binary32 operation
(the sign product is exact: its factors are +-1, 0 and NaN); asserted below, so
a silent promotion cannot pass.  LLRs reach float32 by astype: round to nearest
even, beyond FLT_MAX +-inf, 5e-324 to 0.
"""
import numpy as np


def block_row_vars(base, Z, i):
    """V [Z, d]: the variable of check r of block row i at CSR position j."""
    cols = np.nonzero(base[i] >= 0)[0]
    r = np.arange(Z, dtype=np.int64)[:, None]
    return cols[None, :] * Z + (r + base[i, cols][None, :]) % Z


def qc_layered_ms_ref(base, Z, llr, max_iter, normalization, early_stop, layer_order=None, dtype=np.float64):
    """llr [B, nb Z] -> (bits int64 [B, n], iterations int64 [B], posterior dtype [B, n])."""
    base = np.asarray(base, dtype=np.int64)
    mb, nb = base.shape
    dtype = np.dtype(dtype).type
    assert dtype in (np.float64, np.float32)
    with np.errstate(all="ignore"):
        P = np.array(llr).astype(dtype)
    assert P.ndim == 2 and P.shape[1] == nb * Z
    norm = dtype(normalization)
    order = list(range(mb)) if layer_order is None else [int(i) for i in layer_order]
    assert sorted(order) == list(range(mb))
    V = {i: block_row_vars(base, Z, i) for i in order}
    order = [i for i in order if V[i].shape[1] > 0]
    B = P.shape[0]
    R = {i: np.zeros((B, Z, V[i].shape[1]), dtype=dtype) for i in order}
    decoded = P <= 0
    iterations = np.full(B, max_iter, dtype=np.int64)
    active = np.ones(B, dtype=bool)
    with np.errstate(all="ignore"):
        for it in range(max_iter):
            idx = np.nonzero(active)[0]
            if len(idx) == 0:
                break
            Pa = P[idx]
            for i in order:
                v = V[i]
                d = v.shape[1]
                q = Pa[:, v] - R[i][idx]
                Rn = np.empty_like(q)
                for j in range(d):
                    others = np.delete(q, j, axis=2)
                    Rn[:, :, j] = np.prod(np.sign(others), axis=2) * np.min(np.abs(others), axis=2) * norm
                assert q.dtype == dtype and Rn.dtype == dtype
                R[i][idx] = Rn
                Pa[:, v] = q + Rn
            P[idx] = Pa
            decoded[idx] = Pa <= 0
            if early_stop:
                ok = np.ones(len(idx), dtype=bool)
                for i in order:
                    ok &= (np.bitwise_xor.reduce(decoded[idx][:, V[i]], axis=2) == 0).all(axis=1)
                iterations[idx[ok]] = it + 1
                active[idx[ok]] = False
    assert P.dtype == dtype
    return decoded.astype(np.int64), iterations, P

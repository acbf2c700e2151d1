"""NumPy float32 restatement of the layered normalised min-sum decoder: the
definition a QCLayeredMSDecoder(dtype=np.float32) is tested against
(include/polarldpc.h, PL_LDPC_QC_F32).  It is tests/layered_ref.py's
layered_ms_ref with P, R and the normalisation in float32:

    P[v] = float32(llr[v]);  R[c][j] = float32(0);  norm32 = float32(normalization)
    for it in range(max_iter):
        for layer in layers: for c in layer (deg > 0):
            q = P[rows[c]] - R[c]                                    # float32
            R[c][j] = np.prod(np.sign(q[others])) * np.min(np.abs(q[others])) * norm32
            P[rows[c]] = q + R[c]
        decoded = P <= 0
        if early_stop and H @ decoded % 2 == 0: iterations = it + 1; break

Every operation is one IEEE binary32 operation (NumPy keeps float32 operands in
float32 and flushes no subnormal); the functions assert the dtypes of q, the
new R and the final P, so a silent promotion to float64 cannot pass.
"""
import numpy as np

from layered_ref import check_rows

F32 = np.float32


def to_f32(llr):
    """float32(llr): round to nearest even, beyond FLT_MAX +-inf, 5e-324 to 0; a float32 array as it is."""
    with np.errstate(all="ignore"):
        return np.array(llr).astype(F32)


def layered_ms_ref32(H, llr, layers, max_iter, normalization=1.0, early_stop=True):
    """llr [B, n] -> (bits int64 [B, n], iterations int64 [B], posterior float32 [B, n])."""
    H = np.asarray(H)
    rows = check_rows(H)
    P = to_f32(llr)
    norm32 = F32(normalization)
    B = P.shape[0]
    R = [np.zeros((B, len(r)), dtype=F32) for r in rows]
    decoded = P <= 0
    iterations = np.full(B, max_iter, dtype=np.int64)
    if max_iter == 0:
        iterations[:] = 0
    active = np.ones(B, dtype=bool)
    Hs = (H == 1).astype(np.int64)
    with np.errstate(all="ignore"):
        for it in range(max_iter):
            idx = np.nonzero(active)[0]
            if len(idx) == 0:
                break
            for layer in layers:
                for c in layer:
                    v = rows[c]
                    d = len(v)
                    if d == 0:
                        continue
                    q = P[np.ix_(idx, v)] - R[c][idx]
                    assert q.dtype == F32
                    Rn = np.empty_like(q)
                    for j in range(d):
                        others = np.delete(q, j, axis=1)
                        r = np.prod(np.sign(others), axis=1) * np.min(np.abs(others), axis=1) * norm32
                        assert r.dtype == F32
                        Rn[:, j] = r
                    assert Rn.dtype == F32
                    R[c][idx] = Rn
                    P[np.ix_(idx, v)] = q + Rn
            decoded[idx] = P[idx] <= 0
            if early_stop:
                ok = ((decoded[idx].astype(np.int64) @ Hs.T) % 2 == 0).all(axis=1)
                iterations[idx[ok]] = it + 1
                active[idx[ok]] = False
    assert P.dtype == F32
    return decoded.astype(np.int64), iterations, P


def layered_ms_literal32(H, llr, max_iter, normalization=1.0, early_stop=True):
    """One frame, the serial schedule [[0], [1], ...], as a literal row-by-row loop over float32 scalars."""
    H = np.asarray(H)
    rows = check_rows(H)
    P = to_f32(llr)
    norm32 = F32(normalization)
    R = [np.zeros(len(r), dtype=F32) for r in rows]
    decoded = P <= 0
    iterations = max_iter
    Hs = (H == 1).astype(np.int64)
    with np.errstate(all="ignore"):
        for it in range(max_iter):
            for c, v in enumerate(rows):
                if len(v) == 0:
                    continue
                q = P[v] - R[c]
                assert q.dtype == F32
                for j in range(len(v)):
                    others = np.array([q[i] for i in range(len(v)) if i != j], dtype=F32)
                    r = np.prod(np.sign(others)) * np.min(np.abs(others)) * norm32
                    assert r.dtype == F32
                    R[c][j] = r
                P[v] = q + R[c]
            decoded = P <= 0
            if early_stop and np.all(Hs @ decoded.astype(np.int64) % 2 == 0):
                iterations = it + 1
                break
    assert P.dtype == F32 and all(r.dtype == F32 for r in R)
    return decoded.astype(np.int64), iterations, P

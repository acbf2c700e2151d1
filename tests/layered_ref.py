"""NumPy restatement of the layered normalised min-sum decoder (the definition
LayeredMSDecoder is tested against; include/polarldpc.h, pl_ldpc_layered_plan_create).

    P[v] = llr[v];  R[c][j] = 0.0
    for it in range(max_iter):
        for layer in layers: for c in layer (deg > 0):
            q = P[rows[c]] - R[c]
            R[c][j] = np.prod(np.sign(q[others])) * np.min(np.abs(q[others])) * normalization
            P[rows[c]] = q + R[c]
        decoded = P <= 0
        if early_stop and H @ decoded % 2 == 0: iterations = it + 1; break

Written from the definition with np.sign / np.prod / np.min, vectorised over the
frames only (a sign product of +-1 / 0 / NaN factors and a NaN-propagating
minimum do not depend on the order of evaluation).
"""
import numpy as np


def check_rows(H):
    """rows[c]: the columns where H[c] == 1, ascending (dense_to_csr's reading of H)."""
    H = np.asarray(H)
    return [np.nonzero(H[c] == 1)[0] for c in range(H.shape[0])]


def layered_ms_ref(H, llr, layers, max_iter, normalization=1.0, early_stop=True):
    """llr [B, n] -> (bits int64 [B, n], iterations int64 [B], posterior float64 [B, n])."""
    H = np.asarray(H)
    rows = check_rows(H)
    P = np.array(llr, dtype=np.float64)
    B = P.shape[0]
    R = [np.zeros((B, len(r))) for r in rows]
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
                    Rn = np.empty_like(q)
                    for j in range(d):
                        others = np.delete(q, j, axis=1)
                        Rn[:, j] = np.prod(np.sign(others), axis=1) * np.min(np.abs(others), axis=1) * normalization
                    R[c][idx] = Rn
                    P[np.ix_(idx, v)] = q + Rn
            decoded[idx] = P[idx] <= 0
            if early_stop:
                ok = ((decoded[idx].astype(np.int64) @ Hs.T) % 2 == 0).all(axis=1)
                iterations[idx[ok]] = it + 1
                active[idx[ok]] = False
    return decoded.astype(np.int64), iterations, P


def layered_ms_literal(H, llr, max_iter, normalization=1.0, early_stop=True):
    """One frame, the serial schedule [[0], [1], ...], as a literal row-by-row loop."""
    H = np.asarray(H)
    rows = check_rows(H)
    P = np.array(llr, dtype=np.float64)
    R = [np.zeros(len(r)) for r in rows]
    decoded = P <= 0
    iterations = max_iter
    Hs = (H == 1).astype(np.int64)
    with np.errstate(all="ignore"):
        for it in range(max_iter):
            for c, v in enumerate(rows):
                if len(v) == 0:
                    continue
                q = P[v] - R[c]
                for j in range(len(v)):
                    others = np.array([q[i] for i in range(len(v)) if i != j])
                    R[c][j] = np.prod(np.sign(others)) * np.min(np.abs(others)) * normalization
                P[v] = q + R[c]
            decoded = P <= 0
            if early_stop and np.all(Hs @ decoded.astype(np.int64) % 2 == 0):
                iterations = it + 1
                break
    return decoded.astype(np.int64), iterations, P


def awgn_llrs(n, frames, snr_db, seed):
    """All-zero codeword over BPSK + AWGN, LLR = 2 y / sigma^2 (the channel module's convention)."""
    rng = np.random.RandomState(seed)
    sigma = np.sqrt(1.0 / (2.0 * 10.0 ** (snr_db / 10.0)))
    return 2.0 * (1.0 + sigma * rng.randn(frames, n)) / sigma ** 2

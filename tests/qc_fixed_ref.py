"""NumPy restatement of the int8 fixed-point quasi-cyclic layered min-sum decoder
and of its LLR quantiser (include/polarldpc.h, pl_ldpc_qc_fixed_plan_create and
pl_llr_quantize), in int64, written from the base matrix alone.  It shares no
code with the package or with the other restatements.

    P[v] = clamp(L[v], -llr_max, llr_max);  R[i][r, j] = 0
    for it in range(max_iter):
        for i in layer_order (block rows with at least one block):
            V[r, j] = col_j Z + (r + s_j) % Z            # col_j ascending: the CSR position
            q = clamp(P[V] - R[i], -127, 127)            # [Z, d], all Z checks of the block row at once
            mag[r, j] = min(msg_max, (min_{k != j} |q[r, k]| * norm16) >> 4)
            R[i][r, j] = -mag if an odd number of k != j has q[r, k] < 0 else mag
            P[V] = clamp(q + R[i], -127, 127)
        decoded = P <= 0
        if early_stop and every block row's Z parities are even: iterations = it + 1; break

The Z checks of a block row share no variable, so updating them together is the
serial order.  The restatement also counts how often each of the three clamps
changed a value: "llr" (the input clamp at llr_max), "msg" (the message clamp at
msg_max) and "sat" (the clamps of q and of P at 127, together).
"""
import numpy as np


def quantize_ref(llr, scale, llr_max):
    """clamp(rint(double(llr) * scale), -llr_max, llr_max) as int8; NaN -> 0, +-inf -> +-llr_max."""
    a = np.asarray(llr)
    assert a.dtype in (np.float64, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        x = np.rint(a.astype(np.float64) * np.float64(scale))  # float32 widens exactly; half to even
    x = np.where(np.isnan(x), 0.0, x)
    return np.clip(x, -llr_max, llr_max).astype(np.int8)


def _clamp(x, lim, counter, key):
    y = np.clip(x, -lim, lim)
    counter[key] += int(np.count_nonzero(y != x))
    return y


def qc_fixed_ms_ref(base, Z, L, max_iter, norm16, llr_max, msg_max, early_stop, layer_order=None):
    """L int8 [B, nb Z] -> (bits int64 [B, n], iterations int64 [B], posterior int8 [B, n], clamps dict)."""
    base = np.asarray(base, dtype=np.int64)
    mb, nb = base.shape
    L = np.asarray(L)
    assert L.dtype == np.int8 and L.ndim == 2 and L.shape[1] == nb * Z
    assert 1 <= norm16 <= 16 and 1 <= llr_max <= 127 and 1 <= msg_max <= 127
    clamps = {"llr": 0, "msg": 0, "sat": 0}
    P = _clamp(L.astype(np.int64), llr_max, clamps, "llr")
    order = list(range(mb)) if layer_order is None else [int(i) for i in layer_order]
    assert sorted(order) == list(range(mb))
    rr = np.arange(Z, dtype=np.int64)[:, None]
    V = {}
    for i in order:
        cols = np.nonzero(base[i] >= 0)[0]
        V[i] = cols[None, :] * Z + (rr + base[i, cols][None, :]) % Z
    order = [i for i in order if V[i].shape[1] > 0]
    B = P.shape[0]
    R = {i: np.zeros((B, Z, V[i].shape[1]), dtype=np.int64) for i in order}
    decoded = P <= 0
    iterations = np.full(B, max_iter, dtype=np.int64)
    active = np.ones(B, dtype=bool)
    for it in range(max_iter):
        idx = np.nonzero(active)[0]
        if len(idx) == 0:
            break
        Pa = P[idx]
        for i in order:
            v = V[i]
            d = v.shape[1]
            assert d >= 2, "a block row with one block has no minimum over the others"
            q = _clamp(Pa[:, v] - R[i][idx], 127, clamps, "sat")
            a, neg = np.abs(q), q < 0
            Rn = np.empty_like(q)
            for j in range(d):
                mn = np.delete(a, j, axis=2).min(axis=2)
                raw = (mn * norm16) >> 4
                mag = np.minimum(raw, msg_max)
                clamps["msg"] += int(np.count_nonzero(mag != raw))
                odd = np.delete(neg, j, axis=2).sum(axis=2) % 2 == 1
                Rn[:, :, j] = np.where(odd, -mag, mag)
            R[i][idx] = Rn
            Pa[:, v] = _clamp(q + Rn, 127, clamps, "sat")
        assert np.abs(Pa).max(initial=0) <= 127
        P[idx] = Pa
        decoded[idx] = Pa <= 0
        if early_stop:
            ok = np.ones(len(idx), dtype=bool)
            for i in order:
                ok &= (np.bitwise_xor.reduce(decoded[idx][:, V[i]], axis=2) == 0).all(axis=1)
            iterations[idx[ok]] = it + 1
            active[idx[ok]] = False
    return decoded.astype(np.int64), iterations, P.astype(np.int8), clamps

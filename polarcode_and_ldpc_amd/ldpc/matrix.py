"""Parity-check matrices (host side) and their CSR form.

mackay_construction reproduces the reference's H for a given seed
(src/ldpc/matrix.py:12-50: global np.random.seed, then one
np.random.choice(m, dv, replace=False) per column), so
LDPCEncoder(504, 252, dv=3, dc=6, seed=42)'s matrix is available offline.
regular_construction builds a (dv, dc)-regular H (every check has degree dc), the
kind Min-Sum needs (the reference's MSDecoder fails on degree-1 checks)."""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np


def dense_to_csr(H: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """CSR over rows of the entries equal to 1, ascending columns."""
    H = np.asarray(H)
    rows, cols = np.nonzero(H == 1)
    row_ptr = np.zeros(H.shape[0] + 1, dtype=np.int32)
    np.add.at(row_ptr, rows + 1, 1)
    return np.cumsum(row_ptr, dtype=np.int32), cols.astype(np.int32)


def csr_to_dense(row_ptr, col_idx, n: int) -> np.ndarray:
    m = len(row_ptr) - 1
    H = np.zeros((m, n), dtype=int)
    for c in range(m):
        H[c, col_idx[row_ptr[c]:row_ptr[c + 1]]] = 1
    return H


def layer_schedule(H: np.ndarray) -> list:
    """Layers for LayeredMSDecoder: a first-fit colouring of the rows in row
    order.  Row c joins the lowest-numbered layer that holds no row sharing a
    column with c (layers numbered in order of creation), so the rows of a layer
    are variable-disjoint and zero-degree rows land in layer 0.  Returns a list
    of int arrays (ascending row indices)."""
    row_ptr, col_idx = dense_to_csr(H)
    used = []    # per layer: bool [n], columns taken by its rows
    layers = []
    for c in range(len(row_ptr) - 1):
        cols = col_idx[row_ptr[c]:row_ptr[c + 1]]
        for l, u in enumerate(used):
            if not u[cols].any():
                break
        else:
            l = len(used)
            used.append(np.zeros(np.asarray(H).shape[1], dtype=bool))
            layers.append([])
        used[l][cols] = True
        layers[l].append(c)
    return [np.asarray(l, dtype=np.int64) for l in layers]


def _qc_base(base, Z: int) -> np.ndarray:
    base = np.asarray(base)
    assert base.ndim == 2 and base.size > 0 and int(Z) >= 1, "base must be [mb, nb] and Z >= 1"
    assert np.all((base >= -1) & (base < int(Z))), "base entries must lie in -1 .. Z-1"
    return base.astype(np.int64)


def qc_expand(base, Z: int) -> np.ndarray:
    """Dense H of the quasi-cyclic code (base, Z): base is int [mb, nb], entry -1
    a zero Z x Z block, entry s in 0 .. Z-1 the identity shifted cyclically by s,
    H[i Z + r, j Z + (r + s) % Z] = 1.  For tests and small codes; the decoder
    (QCLayeredMSDecoder) never expands H."""
    base = _qc_base(base, Z)
    mb, nb = base.shape
    H = np.zeros((mb * Z, nb * Z), dtype=int)
    r = np.arange(Z)
    for i, j in zip(*np.nonzero(base >= 0)):
        H[i * Z + r, j * Z + (r + base[i, j]) % Z] = 1
    return H


def qc_to_csr(base, Z: int) -> Tuple[np.ndarray, np.ndarray]:
    """dense_to_csr(qc_expand(base, Z)) without the dense matrix."""
    base = _qc_base(base, Z)
    mb, nb = base.shape
    deg = (base >= 0).sum(axis=1)
    row_ptr = np.zeros(mb * Z + 1, dtype=np.int32)
    row_ptr[1:] = np.cumsum(np.repeat(deg, Z), dtype=np.int64)
    r = np.arange(Z)[:, None]
    cols = []
    for i in range(mb):
        j = np.nonzero(base[i] >= 0)[0]  # ascending block columns: ascending columns within a row
        cols.append((j[None, :] * Z + (r + base[i, j][None, :]) % Z).ravel())
    return row_ptr, np.concatenate(cols).astype(np.int32)


def qc_block_layers(mb: int, Z: int, order=None) -> list:
    """The block rows as layers: int arrays [i Z, (i+1) Z) for i in `order`
    (default 0 .. mb-1).  The Z checks of a block row share no variable."""
    order = range(mb) if order is None else order
    return [np.arange(int(i) * Z, (int(i) + 1) * Z, dtype=np.int64) for i in order]


def qc_random_base(mb: int, nb: int, Z: int, dv: int, seed: int) -> np.ndarray:
    """A seeded random base matrix: every block column gets dv non-zero blocks in
    distinct block rows with uniform shifts; the whole matrix is redrawn (the
    generator continuing) until every block row has at least 2 non-zero blocks."""
    rng = np.random.RandomState(seed)
    while True:
        base = np.full((mb, nb), -1, dtype=np.int64)
        for j in range(nb):
            rows = rng.choice(mb, dv, replace=False)
            base[rows, j] = rng.randint(0, Z, dv)
        if np.all((base >= 0).sum(axis=1) >= 2):
            return base


def qc_encoding_structure(base) -> Tuple[int, Optional[int]]:
    """(g, x) of a base matrix that QCLDPCEncoder can encode from: the parity part
    base[:, kb:], kb = nb - mb >= 1, is a core of g block rows (g == 0 or g >= 3)
    followed by a lower-triangular extension (include/polarldpc.h,
    pl_ldpc_qc_encoder_create).  x is the middle row of parity column kb, None when
    g == 0.  ValueError naming the first rule violated for anything else."""
    base = np.asarray(base)
    if base.ndim != 2 or base.size == 0:
        raise ValueError("base must be [mb, nb]")
    mb, nb = base.shape
    kb = nb - mb
    if kb < 1:
        raise ValueError("kb = nb - mb must be >= 1 (no message block column)")
    P = base[:, kb:] >= 0

    def ext_ok(i):
        return bool(P[i, i]) and not P[i, i + 1:].any()

    f = mb - 1
    while f >= 0 and ext_ok(f):
        f -= 1
    if f < 0:
        return 0, None
    g = f + 2  # the last row that is no extension row is core row g - 2
    if g > mb:
        raise ValueError("block row %d is no extension row (a diagonal block and none to its right) and cannot be "
                         "the last but one row of a core" % f)
    if g == 2:
        raise ValueError("a core of g = 2 block rows: g must be 0 or >= 3")
    if P[:g, g:].any():
        i, t = np.argwhere(P[:g, g:])[0]
        raise ValueError("core block row %d has a block in parity column kb+%d" % (i, g + t))
    rows = np.nonzero(P[:g, 0])[0]
    if len(rows) != 3 or rows[0] != 0 or rows[2] != g - 1:
        raise ValueError("parity column kb+0 must have exactly three blocks in the core, in rows 0, x and g-1 = %d "
                         "(it has them in rows %s)" % (g - 1, rows.tolist()))
    x = int(rows[1])
    if base[0, kb] != base[g - 1, kb]:
        raise ValueError("the first and the last block of parity column kb+0 must have equal shifts (%d, %d)"
                         % (base[0, kb], base[g - 1, kb]))
    for t in range(1, g):
        rows = np.nonzero(P[:g, t])[0]
        if rows.tolist() != [t - 1, t]:
            raise ValueError("parity column kb+%d must have exactly two blocks in the core, in rows %d and %d"
                             % (t, t - 1, t))
        if base[t - 1, kb + t] != 0 or base[t, kb + t] != 0:
            raise ValueError("the dual-diagonal blocks of parity column kb+%d must have shift 0" % t)
    return g, x


def qc_encodable_base(mb: int, nb: int, Z: int, dv: int, seed: int, core: Optional[int] = None,
                      chained: bool = True) -> np.ndarray:
    """A seeded random base matrix of the structure qc_encoding_structure accepts,
    with g = mb (core None) or g = core (0 or 3 .. mb) core rows.  Message columns
    as qc_random_base; then x in 1 .. g-2 and the shifts (a, b) of parity column
    kb; then per extension row its diagonal shift and, where an earlier parity
    column is allowed (any below the diagonal when `chained`, else a core one),
    one more block there.  chained=False: no extension row reads an extension
    parity.  The whole matrix is redrawn (the generator continuing) until every
    block row has at least 2 non-zero blocks."""
    g = mb if core is None else int(core)
    kb = nb - mb
    if kb < 1 or not (g == 0 or 3 <= g <= mb):
        raise ValueError("needs nb - mb >= 1 and core == 0 or 3 <= core <= mb")
    rng = np.random.RandomState(seed)
    while True:
        base = np.full((mb, nb), -1, dtype=np.int64)
        for j in range(kb):
            rows = rng.choice(mb, dv, replace=False)
            base[rows, j] = rng.randint(0, Z, dv)
        if g > 0:
            x = rng.randint(1, g - 1)
            a, b = rng.randint(0, Z, 2)
            base[0, kb] = base[g - 1, kb] = a
            base[x, kb] = b
            for t in range(1, g):
                base[t - 1, kb + t] = base[t, kb + t] = 0
        for i in range(g, mb):
            base[i, kb + i] = rng.randint(0, Z)
            lim = i if chained else g
            if lim > 0:
                col = kb + rng.randint(0, lim)
                base[i, col] = rng.randint(0, Z)
        if np.all((base >= 0).sum(axis=1) >= 2):
            return base


def mackay_construction(n: int, k: int, dv: int, dc: int, seed: Optional[int] = None) -> np.ndarray:
    m = n - k
    if dv * n != dc * m:
        raise ValueError(f"Degree constraint not satisfied: dv*n={dv*n} != dc*m={dc*m}")
    if seed is not None:
        np.random.seed(seed)
    H = np.zeros((m, n), dtype=int)
    for col in range(n):
        H[np.random.choice(m, dv, replace=False), col] = 1
    return H


def generate_ldpc_matrix(n: int, k: int, method: str = "mackay", dv: int = 3, dc: int = 6,
                         seed: Optional[int] = None) -> np.ndarray:
    """src/ldpc/matrix.py:53-91 (mackay / random)."""
    m = n - k
    if method == "mackay":
        if dv * n != dc * m:
            dc = (dv * n) // m
        return mackay_construction(n, k, dv, dc, seed)
    if method == "random":
        if seed is not None:
            np.random.seed(seed)
        return np.random.randint(0, 2, (m, n))
    raise ValueError(f"Unknown method: {method}")


def regular_construction(n: int, dv: int = 3, dc: int = 6, seed: int = 0) -> np.ndarray:
    """(dv, dc)-regular H by a seeded socket permutation without repeated edges."""
    assert (n * dv) % dc == 0
    m = n * dv // dc
    rng = np.random.RandomState(seed)
    while True:
        sockets = np.repeat(np.arange(m), dc)
        rng.shuffle(sockets)
        cols = sockets.reshape(n, dv)
        s = np.sort(cols, axis=1)
        if np.all(s[:, 1:] != s[:, :-1]):
            H = np.zeros((m, n), dtype=int)
            H[cols.ravel(), np.repeat(np.arange(n), dv)] = 1
            return H


def peg_construction(n: int, k: int, dv: int) -> np.ndarray:
    """The reference's simplified progressive edge growth (matrix.py:94-132):
    column by column, dv times pick the least-loaded check not yet used by this
    column (first such check on ties)."""
    m = n - k
    H = np.zeros((m, n), dtype=int)
    load = np.zeros(m, dtype=np.int64)
    for col in range(n):
        used = np.zeros(m, dtype=bool)
        for _ in range(min(dv, m)):
            cand = np.where(used, np.iinfo(np.int64).max, load)
            r = int(np.argmin(cand))
            used[r] = True
            H[r, col] = 1
            load[r] += 1
    return H


def create_systematic_generator(H: np.ndarray):
    """(G [k, n], P) or (None, None) when the last m columns of H are singular
    over GF(2) (matrix.py:135-187)."""
    from .encoder import _systematic_generator
    return _systematic_generator(H)


def check_matrix_rank(H: np.ndarray) -> int:
    """np.linalg.matrix_rank, as the reference (real rank, not GF(2); matrix.py:190-200)."""
    return int(np.linalg.matrix_rank(H))


def calculate_girth(H: np.ndarray) -> int:
    """The reference returns a density-based estimate (matrix.py:203-225): 6 for
    density < 0.1, else 4."""
    m, n = H.shape
    return 6 if np.sum(H) / (m * n) < 0.1 else 4


def gf2_systematic_pair(H: np.ndarray):
    """A valid systematic code for any H over GF(2): (Hp, G) with Hp = H with its
    columns permuted so the message occupies positions 0..k-1 and G [n, k]
    (pyldpc's orientation: codeword = G @ message mod 2), k = n - rank_GF2(H).
    Used by the lib_wrappers substitute for the unavailable pyldpc."""
    A = (np.asarray(H) % 2).astype(np.uint8)
    m, n = A.shape
    pivots, r = [], 0
    for c in range(n - 1, -1, -1):  # parity checks on the right when possible
        if r == m:
            break
        nz = np.nonzero(A[r:, c])[0]
        if len(nz) == 0:
            continue
        p = r + nz[0]
        if p != r:
            A[[r, p]] = A[[p, r]]
        rows = np.nonzero(A[:, c])[0]
        A[rows[rows != r]] ^= A[r]
        pivots.append(c)
        r += 1
    piv_row = {c: i for i, c in enumerate(pivots)}
    info = [c for c in range(n) if c not in piv_row]
    parity = sorted(pivots)
    perm = np.array(info + parity)
    k = len(info)
    G = np.zeros((n, k), dtype=int)
    G[:k] = np.eye(k, dtype=int)
    for t, c in enumerate(parity):
        G[k + t] = A[piv_row[c], info]
    return np.asarray(H)[:, perm], G


"""The quasi-cyclic encoder on the host (no GPU): qc_encoding_structure,
qc_encodable_base and QCLDPCEncoder's NumPy encode against the expanded H and
against the dense generator path (valid_generator), and the planner's
qc_encoder_plan_build through its device-free window,
pl_debug_ldpc_qc_encoder_probe.  The stream's digest is checked against the stream
rebuilt here from the layout include/polarldpc.h documents: no recorded golden."""
import ctypes
import functools

import numpy as np
import pytest

# id: (mb, nb, Z, dv, seed, core, chained) -> the g the base is meant to have
CASES = {
    "z1": ((4, 8, 1, 3, 1, None, True), 4),
    "z7": ((4, 8, 7, 3, 1, None, True), 4),
    "z27": ((4, 8, 27, 3, 1, None, True), 4),
    "z64": ((4, 8, 64, 3, 1, None, True), 4),
    "z96": ((4, 8, 96, 3, 1, None, True), 4),
    "z7_core4_chained": ((6, 10, 7, 3, 2, 4, True), 4),
    "z7_core4_nr": ((6, 10, 7, 3, 2, 4, False), 4),
    "z65_core4_chained": ((8, 12, 65, 3, 7, 4, True), 4),
    "z65_core4_nr": ((8, 12, 65, 3, 7, 4, False), 4),
    "z96_triangular": ((4, 8, 96, 3, 5, 0, True), 0),
    "z27_triangular_flat": ((4, 8, 27, 3, 5, 0, False), 0),
    "z2_core3": ((3, 5, 2, 2, 8, None, True), 3),
    "z33_core3_ext": ((7, 12, 33, 3, 11, 3, True), 3),
    "z1024": ((3, 5, 1024, 2, 9, None, True), 3),
}
DENSE = sorted(c for c in CASES if c != "z1024")  # the dense elimination of the Z = 1024 code is skipped
NMSG = 67


def _L():
    import polarcode_and_ldpc_amd.ldpc as L
    return L


def _N():
    from polarcode_and_ldpc_amd import _native
    return _native


@functools.lru_cache(maxsize=None)
def base_of(case):
    mb, nb, Z, dv, seed, core, chained = CASES[case][0]
    b = _L().qc_encodable_base(mb, nb, Z, dv, seed, core=core, chained=chained)
    b.setflags(write=False)
    return b, Z


@functools.lru_cache(maxsize=None)
def messages(case):
    b, Z = base_of(case)
    m = np.random.RandomState(1000 + len(case)).randint(0, 2, (NMSG, (b.shape[1] - b.shape[0]) * Z)).astype(np.uint8)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def codewords(case):
    b, Z = base_of(case)
    c = _L().QCLDPCEncoder(b, Z).encode_batch(messages(case))
    c.setflags(write=False)
    return c


def ext_reads_ext(base, g):
    """extension rows that read the parity of another extension row"""
    mb, nb = base.shape
    kb = nb - mb
    return [i for i in range(g, mb) if (base[i, kb + g:kb + i] >= 0).any()]


def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def probe(base, Z, shape=None):
    N = _N()
    sh = np.ascontiguousarray(base, dtype=np.int32)
    mb, nb = sh.shape if shape is None else shape
    out = N.QcEncoderProbe()
    rc = N.lib.pl_debug_ldpc_qc_encoder_probe(mb, nb, Z, _ptr(sh), ctypes.byref(out))
    return rc, out, (N.lib.pl_last_error() or b"").decode()


def stream_of(base, Z):
    """(stream, synchronisation points) from the documented layout."""
    base = np.asarray(base)
    mb, nb = base.shape
    kb = nb - mb
    g, x = _L().qc_encoding_structure(base)
    t = [g, x or 0, int(base[0, kb]) if g else 0, int(base[x, kb]) if g else 0]
    for i in range(g):
        cols = np.nonzero(base[i, :kb] >= 0)[0]
        t += [len(cols)] + [int(v) for j in cols for v in (j, base[i, j])]
    dirty = set(range(kb + 1, kb + g))  # p_1 .. p_{g-1} are written behind p_0's synchronisation
    nsync = 1 if g else 0
    for i in range(g, mb):
        cols = np.nonzero(base[i, :kb + i] >= 0)[0]
        sync = int(any(int(j) in dirty for j in cols))
        t += [int(base[i, kb + i]), sync, len(cols)] + [int(v) for j in cols for v in (j, base[i, j])]
        if sync:
            dirty.clear()
            nsync += 1
        dirty.add(kb + i)
    return np.asarray(t, np.int32), nsync


def fnv1a(a):
    h = 14695981039346656037
    for byte in a.tobytes():
        h = ((h ^ byte) * 1099511628211) % 2 ** 64
    return h


# ---- the structure ---------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(CASES))
def test_structure_is_the_intended_one(case):
    L = _L()
    base, Z = base_of(case)
    mb, nb, _, dv, seed, core, chained = CASES[case][0]
    g, x = L.qc_encoding_structure(base)
    assert g == CASES[case][1] == (mb if core is None else core)
    assert (x is None) == (g == 0) and (g == 0 or 0 < x < g - 1)
    assert base.shape == (mb, nb) and base.min() >= -1 and base.max() < Z
    assert ((base >= 0).sum(axis=1) >= 2).all() and ((base[:, :nb - mb] >= 0).sum(axis=0) == dv).all()
    assert np.array_equal(base, L.qc_encodable_base(mb, nb, Z, dv, seed, core=core, chained=chained))
    enc = L.QCLDPCEncoder(base, Z)
    assert (enc.n, enc.k, enc.m, enc.mb, enc.nb, enc.Z) == (nb * Z, (nb - mb) * Z, mb * Z, mb, nb, Z)
    assert np.array_equal(enc.info_positions, np.arange(enc.k)) and np.array_equal(enc.base, base)
    assert enc.get_code_rate() == enc.k / enc.n and "QCLDPCEncoder" in repr(enc)


def test_draw_order_is_the_documented_one():
    L = _L()
    mb, nb, Z, dv, seed, g = 6, 10, 7, 3, 2, 4
    kb = nb - mb
    for chained in (True, False):
        rng = np.random.RandomState(seed)
        while True:
            want = np.full((mb, nb), -1)
            for j in range(kb):
                rows = rng.choice(mb, dv, replace=False)
                want[rows, j] = rng.randint(0, Z, dv)
            x = rng.randint(1, g - 1)
            a, b = rng.randint(0, Z, 2)
            want[0, kb] = want[g - 1, kb] = a
            want[x, kb] = b
            for t in range(1, g):
                want[t - 1, kb + t] = want[t, kb + t] = 0
            for i in range(g, mb):
                want[i, kb + i] = rng.randint(0, Z)
                lim = i if chained else g
                col = kb + rng.randint(0, lim)
                want[i, col] = rng.randint(0, Z)
            if ((want >= 0).sum(axis=1) >= 2).all():
                break
        assert np.array_equal(L.qc_encodable_base(mb, nb, Z, dv, seed, core=g, chained=chained), want)


def test_chained_and_nr_like_premises():
    """The (8, 12, 65) chained base has an extension row that reads an extension parity;
    its chained=False twin and the (6, 10, 7) one have none."""
    assert ext_reads_ext(base_of("z65_core4_chained")[0], 4)
    assert not ext_reads_ext(base_of("z65_core4_nr")[0], 4)
    assert not ext_reads_ext(base_of("z7_core4_nr")[0], 4)
    assert ext_reads_ext(base_of("z96_triangular")[0], 0)
    assert not ext_reads_ext(base_of("z27_triangular_flat")[0], 0)
    assert base_of("z33_core3_ext")[0].shape[0] > 3  # g = 3 with extension rows


# ---- the host encoder ------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(CASES))
def test_encode_batch_gives_codewords_of_the_expanded_H(case):
    L = _L()
    base, Z = base_of(case)
    msg, cw = messages(case), codewords(case)
    k = msg.shape[1]
    assert cw.shape == (NMSG, base.shape[1] * Z) and set(np.unique(cw)) <= {0, 1}
    assert np.array_equal(cw[:, :k], msg)
    rp, ci = L.qc_to_csr(base, Z)  # H c = 0, row by row of the expanded H (CSR: the Z = 1024 H stays sparse)
    syn = np.bitwise_xor.reduceat(cw[:, ci], rp[:-1], axis=1)
    assert not syn.any()
    enc = L.QCLDPCEncoder(base, Z)
    assert enc.verify_codeword(cw[3]) and not enc.verify_codeword(cw[3] ^ (np.arange(cw.shape[1]) == k))
    if case != "z1024":
        H = L.qc_expand(base, Z)
        assert np.array_equal(enc.H, H) and not ((cw @ H.T) % 2).any()


@pytest.mark.parametrize("case", DENSE)
def test_encode_batch_equals_the_dense_generator(case):
    L = _L()
    base, Z = base_of(case)
    msg = messages(case)
    G, info = L.valid_generator(L.qc_expand(base, Z))
    assert np.array_equal(info, np.arange(msg.shape[1]))  # Hp is invertible: rank m Z
    assert np.array_equal(codewords(case), (msg.astype(np.int64) @ G) % 2)


@pytest.mark.parametrize("case", ["z7", "z65_core4_chained", "z27_triangular_flat"])
def test_message_values_are_taken_and_1_and_encode_is_one_row(case):
    L = _L()
    base, Z = base_of(case)
    enc = L.QCLDPCEncoder(base, Z)
    msg = messages(case)
    dirty = msg.astype(np.int64) + 2 * np.random.RandomState(5).randint(0, 100, msg.shape)
    dirty[0, :] = msg[0] | 254
    assert np.array_equal(enc.encode_batch(dirty), codewords(case))
    assert np.array_equal(enc.encode(msg[5]), codewords(case)[5])
    assert enc.encode(msg[5]).shape == (enc.n,)


# ---- refusals --------------------------------------------------------------------------
def _bad_bases():
    L = _L()
    good = np.array(base_of("z7_core4_chained")[0])  # (6, 10), g = 4, kb = 4
    kb = 4
    g, x = L.qc_encoding_structure(good)
    assert g == 4
    out = {"qc_random_base": (L.qc_random_base(4, 8, 7, 3, seed=115), 7)}
    b = good.copy(); b[3, kb] = (b[0, kb] + 1) % 7
    out["unequal_first_last"] = (b, 7)
    b = good.copy(); b[1, kb + 2] = 3
    out["dual_diagonal_shift"] = (b, 7)
    b = good.copy(); b[3 - x, kb] = 2  # the free middle row of parity column kb
    out["fourth_block"] = (b, 7)
    # g = 2: row 0 is the only row that is no extension row
    b = np.full((3, 5), -1); b[:, 0] = 1; b[:, 1] = 2
    b[0, 2] = 0; b[0, 3] = 0; b[1, 3] = 0; b[1, 2] = 0; b[2, 4] = 0
    out["g2"] = (b, 7)
    b = good.copy(); b[4, kb + 5] = 1
    out["right_of_extension_diagonal"] = (b, 7)
    return out


@pytest.mark.parametrize("name", ["qc_random_base", "unequal_first_last", "dual_diagonal_shift", "fourth_block", "g2",
                                  "right_of_extension_diagonal"])
def test_structure_violations_are_refused(name):
    L, N = _L(), _N()
    base, Z = _bad_bases()[name]
    with pytest.raises(ValueError) as e1:
        L.qc_encoding_structure(base)
    assert str(e1.value)
    with pytest.raises(ValueError):
        L.QCLDPCEncoder(base, Z)
    rc, _, msg = probe(base, Z)
    assert rc == N.PL_EUNSUPPORTED and msg, (rc, msg)
    if name == "g2":
        assert "g = 2" in msg and "g = 2" in str(e1.value)


def test_argument_refusals():
    L, N = _L(), _N()
    good = np.array(base_of("z7")[0])
    with pytest.raises(ValueError):  # kb = 0
        L.qc_encoding_structure(good[:, 4:])
    with pytest.raises(ValueError):
        L.QCLDPCEncoder(good[:, 4:], 7)
    rc, _, msg = probe(good[:, 4:], 7)
    assert rc == N.PL_EINVAL and "kb" in msg
    with pytest.raises(ValueError):
        L.QCLDPCEncoder(good, 1025)
    rc, _, msg = probe(good, 1025)
    assert rc == N.PL_EUNSUPPORTED and "1024" in msg
    assert probe(base_of("z1024")[0], 1024)[0] == 0
    for bad in (7, 100, -2):  # a shift >= z
        b = good.copy()
        b[1, 2] = bad
        with pytest.raises(ValueError):
            L.QCLDPCEncoder(b, 7)
        rc, _, msg = probe(b, 7)
        assert rc == N.PL_EINVAL and "shift" in msg
    for Z in (0, -3):
        with pytest.raises(ValueError):
            L.QCLDPCEncoder(good, Z)
        rc, _, msg = probe(good, Z)
        assert rc == N.PL_EINVAL and msg
    out = N.QcEncoderProbe()
    assert N.lib.pl_debug_ldpc_qc_encoder_probe(4, 8, 7, None, ctypes.byref(out)) == N.PL_EINVAL
    assert N.lib.pl_debug_ldpc_qc_encoder_probe(4, 8, 7, _ptr(np.ascontiguousarray(good, np.int32)), None) == N.PL_EINVAL
    # (nb + g) Z above 160 KB: a triangular code with 161 block columns of 1024 bits
    mb, nb = 2, 161
    big = np.full((mb, nb), -1)
    big[:, 0] = 0
    big[0, nb - 2] = big[1, nb - 1] = 0
    assert L.qc_encoding_structure(big) == (0, None)
    with pytest.raises(ValueError):
        L.QCLDPCEncoder(big, 1024)
    rc, _, msg = probe(big, 1024)
    assert rc == N.PL_EUNSUPPORTED and "160 KB" in msg
    assert probe(big[:, 1:], 1024)[0] == 0 and L.QCLDPCEncoder(big[:, 1:], 1024).n == 160 * 1024


# ---- the planner -----------------------------------------------------------------------
def test_probe_geometry():
    fpw = {}
    for case in sorted(CASES):
        base, Z = base_of(case)
        rc, p, msg = probe(base, Z)
        assert rc == 0, msg
        g, x = _L().qc_encoding_structure(base)
        kb = base.shape[1] - base.shape[0]
        assert (p.g, p.x) == (g, x or 0)
        assert (p.a, p.b) == ((int(base[0, kb]), int(base[x, kb])) if g else (0, 0))
        frame = ((base.shape[1] + g) * Z + 15) // 16 * 16
        assert p.subwave == (Z <= 64) and p.fpw == (64 // Z if Z <= 64 else 1)
        assert p.threads == (64 * p.fpb if Z <= 64 else (Z + 63) // 64 * 64) and 1 <= p.fpb <= 4
        assert p.lds_bytes == frame * p.fpw * p.fpb <= 160 * 1024
        fpw[case] = p.fpw
    assert [fpw[c] for c in ("z1", "z7", "z27", "z64")] == [64, 9, 2, 1]
    for case in ("z65_core4_chained", "z65_core4_nr", "z96", "z96_triangular"):
        assert probe(*base_of(case))[1].threads == 128
    assert probe(*base_of("z1024"))[1].threads == 1024


@pytest.mark.parametrize("case", sorted(CASES))
def test_stream_is_the_documented_layout(case):
    base, Z = base_of(case)
    rc, p, msg = probe(base, Z)
    assert rc == 0, msg
    t, nsync = stream_of(base, Z)
    mb = base.shape[0]
    assert p.table_len == len(t) == 4 + p.g + 3 * (mb - p.g) + 2 * int((base >= 0).sum()) - 2 * (mb - p.g) \
        - 2 * ((3 + 2 * (p.g - 1)) if p.g else 0)
    assert p.digest == fnv1a(t)
    assert p.n_sync == nsync


# The sync flags of the extension rows, worked out by hand from the rule (a row is flagged iff it reads a
# parity block column written since the last synchronisation point; behind p_0's, p_1 .. p_{g-1} count as
# written) and the parity parts of the seeded bases:
#   (6, 10, 7) core 4: row 4 reads p_2 (flag), row 5 reads p_1 (chained) or p_3 (not), both from before row 4's
#     synchronisation -- this chained draw has no row that reads an extension parity, so the twins tie;
#   (8, 12, 65) core 4 chained: rows 4 .. 7 read p_2 (flag), p_4 (flag), p_1, p_4 (visible since row 5's);
#     chained=False: p_2 (flag), p_1, p_0, p_1;
#   (4, 8, 96) triangular: row 0 reads no parity, rows 1 .. 3 read p_0 (flag), p_0, p_1 (flag);
#   (7, 12, 33) core 3: rows 3 .. 6 read p_1 (flag), p_0, p_1, p_2.
SYNC_FLAGS = {
    "z7_core4_chained": [1, 0],
    "z7_core4_nr": [1, 0],
    "z65_core4_chained": [1, 1, 0, 0],
    "z65_core4_nr": [1, 0, 0, 0],
    "z96_triangular": [0, 1, 0, 1],
    "z27_triangular_flat": [0, 0, 0, 0],
    "z33_core3_ext": [1, 0, 0, 0],
}


def flags_of(stream, mb):
    g = int(stream[0])
    at = 4
    for _ in range(g):
        at += 1 + 2 * int(stream[at])
    out = []
    for _ in range(g, mb):
        out.append(int(stream[at + 1]))
        at += 3 + 2 * int(stream[at + 2])
    assert at == len(stream)
    return out


@pytest.mark.parametrize("case", sorted(SYNC_FLAGS))
def test_sync_flags_are_the_hand_derived_ones(case):
    """Pins the rule itself: stream_of repeats the planner's bookkeeping, these literals do not.  The digest
    test ties the planner's stream to stream_of's, so the planner's flags are these."""
    base, Z = base_of(case)
    t, nsync = stream_of(base, Z)
    g = CASES[case][1]
    assert flags_of(t, base.shape[0]) == SYNC_FLAGS[case]
    rc, p, msg = probe(base, Z)
    assert rc == 0, msg
    assert p.n_sync == nsync == (1 if g else 0) + sum(SYNC_FLAGS[case]) and p.digest == fnv1a(t)


def test_synchronisation_points():
    n = {c: probe(*base_of(c))[1].n_sync for c in CASES}
    # an NR-like extension: one synchronisation behind p_0's for all its rows
    assert n["z7_core4_nr"] == 2 and n["z65_core4_nr"] == 2
    # fewer than for the chained twin, whose row 5 reads row 4's parity
    assert n["z65_core4_chained"] == 3 > n["z65_core4_nr"]
    # the seed-2 (6, 10, 7) chained draw has no row that reads an extension parity (SYNC_FLAGS): a tie
    assert not ext_reads_ext(base_of("z7_core4_chained")[0], 4) and n["z7_core4_chained"] == n["z7_core4_nr"]
    # a core alone: p_0's; a triangular part whose rows read no parity: none
    assert n["z7"] == n["z2_core3"] == 1 and n["z27_triangular_flat"] == 0
    assert n["z96_triangular"] == 2

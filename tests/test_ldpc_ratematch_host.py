"""Rate matching on the host (no GPU): the planner's derived fields and refusals
through its device-free window pl_debug_rate_match_probe, the closed form of
include/polarldpc.h (pl_rate_match) against the selection loop, QCRateMatcher's
select_host / recover_host, decoder_rows / decoder_base.

The loop is written out once more here (nr_positions), so that select_host is
itself pinned and not only compared with what it feeds.

Bases: qc_encodable_base(8, 12, Z, 3, seed, core=4, chained=False), kb = 4, for
Z = 1, 7, 27, 96, and one core=None base (g = mb).  The configurations of a
base (configs) cover punctured 0 and 2; F = 0, 5 and k - P (at Z = 1 no code has
five message bits left to shorten: F = 5 is a refusal there, tested as one, and
k - P - 1 stands in); E < M without a wrap, start > 0 with a wrap, E = M,
E = 2 M + 5 (positions with 2 and with 3 terms), start inside the filler run,
ncb = k - P with start a filler, ncb < n - P, start no multiple of Z."""
import ctypes
import functools

import numpy as np
import pytest

ZS = (1, 7, 27, 96)
MB, NB, KB = 8, 12, 4


def _L():
    import polarcode_and_ldpc_amd.ldpc as L
    return L


def _N():
    from polarcode_and_ldpc_amd import _native
    return _native


@functools.lru_cache(maxsize=None)
def base_of(Z, core=4):
    b = _L().qc_encodable_base(MB, NB, Z, 3, 40 + Z, core=core, chained=False)
    b.setflags(write=False)
    return b


def configs(Z):
    """name -> QCRateMatcher keyword arguments for the (8, 12, Z) code."""
    n, k = NB * Z, KB * Z
    out = {}

    def add(name, punctured, F, ncb, start, E):
        P = punctured * Z
        F = {"5": 5 if k - P >= 5 else k - P - 1, "all": k - P, "0": 0}[F]
        ncb = {"n": n - P, "k": k - P, "mid": k - P + 3 * Z + (1 if Z > 1 else 0)}[ncb]
        M = ncb - F
        lo = k - P - F  # the first filler's buffer position
        start = {"0": 0, "odd": (Z + 1) % ncb, "late": ncb - 1 - Z // 2, "filler": lo + F // 2,
                 "filler0": lo}[start] % ncb
        E = {"short": max(1, (3 * M) // 5), "M": M, "rep": 2 * M + 5}[E]
        out[name] = dict(E=E, punctured=punctured, fillers=F, ncb=ncb, start=start)

    add("p0_f0_short", 0, "0", "n", "0", "short")         # E < M, no wrap
    add("p0_f0_wrap", 0, "0", "n", "late", "short")       # start > 0, wraps
    add("p0_f0_full", 0, "0", "n", "odd", "M")            # E = M, start no multiple of Z
    add("p0_f0_rep", 0, "0", "n", "odd", "rep")           # 2 and 3 terms
    add("p2_f5_short", 2, "5", "n", "0", "short")
    add("p2_f5_infiller", 2, "5", "n", "filler", "M")     # start inside the filler run
    add("p2_f5_rep", 2, "5", "n", "late", "rep")
    add("p0_f5_ncbk", 0, "5", "k", "filler0", "short")    # no parity in the buffer, start a filler
    add("p2_f5_ncbk_rep", 2, "5", "k", "filler", "rep")
    add("p2_fall_short", 2, "all", "n", "filler", "short")  # only parity is sent
    add("p0_fall_rep", 0, "all", "n", "filler0", "rep")
    add("p2_f0_mid_full", 2, "0", "mid", "odd", "M")      # ncb < n - P
    add("p0_f5_mid_rep", 0, "5", "mid", "filler", "rep")
    add("p0_f5_mid_short", 0, "5", "mid", "late", "short")
    add("p2_f0_ncbk_full", 2, "0", "k", "odd", "M")
    return out


CASES = [(Z, name) for Z in ZS for name in configs(1)]
IDS = ["z%d-%s" % c for c in CASES]


def nr_positions(n, k, P, F, ncb, start, E):
    """The selection loop of include/polarldpc.h: the codeword position of each t."""
    pos, t, j = [], 0, 0
    while t < E:
        b = (start + j) % ncb
        if not (k - P - F <= b < k - P):
            pos.append(P + b)
            t += 1
        j += 1
    return np.array(pos, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def matcher(Z, name, core=4):
    return _L().QCRateMatcher(base_of(Z, core), Z, **configs(Z)[name])


def test_configs_cover_what_they_claim():
    for Z in ZS:
        n, k = NB * Z, KB * Z
        seen = set()
        for name, c in configs(Z).items():
            P, F, ncb, start, E = c["punctured"] * Z, c["fillers"], c["ncb"], c["start"], c["E"]
            M, lo = ncb - F, k - P - F
            assert 0 <= F <= k - P and k - P <= ncb <= n - P and 0 <= start < ncb and E >= 1 and M >= 1, (Z, name)
            pos = nr_positions(n, k, P, F, ncb, start, E)
            wraps = bool((np.diff(pos) < 0).any())
            seen |= {"P%d" % c["punctured"], "F0" if F == 0 else "Fall" if F == k - P else "Fsome"}
            seen |= {"short_nowrap"} if E < M and not wraps else set()
            seen |= {"start_wrap"} if start > 0 and wraps and E < M else set()
            seen |= {"E=M"} if E == M else set()
            seen |= {"rep23"} if E == 2 * M + 5 and set(np.bincount(pos)[np.bincount(pos) > 0]) == {2, 3} else set()
            seen |= {"start_filler"} if F and lo <= start < lo + F else set()
            seen |= {"ncbk_start_filler"} if ncb == k - P and F and lo <= start < lo + F else set()
            seen |= {"ncb_small"} if k - P < ncb < n - P else set()
            seen |= {"start_unaligned"} if start % Z else set()
        want = {"P0", "P2", "F0", "Fall", "Fsome", "short_nowrap", "start_wrap", "E=M", "rep23", "start_filler",
                "ncbk_start_filler", "ncb_small"} | ({"start_unaligned"} if Z > 1 else set())
        assert want <= seen, (Z, want - seen)
        assert any(c["fillers"] == 5 for c in configs(Z).values()) == (Z > 1)


@pytest.mark.parametrize("Z,name", CASES, ids=IDS)
def test_probe_and_closed_form_match_the_loop(Z, name):
    rm = matcher(Z, name)
    c = configs(Z)[name]
    n, k, P, F, ncb, start, E = NB * Z, KB * Z, c["punctured"] * Z, c["fillers"], c["ncb"], c["start"], c["E"]
    pos = nr_positions(n, k, P, F, ncb, start, E)
    assert np.array_equal(rm.positions_host(), pos)
    assert np.array_equal(rm.select_host(np.arange(n)), pos)
    assert np.array_equal(rm.select_host(np.arange(2 * n).reshape(2, n) % 251), (np.arange(2 * n).reshape(2, n) % 251)[:, pos])
    # the derived fields, from the loop alone
    nonfiller = [b for b in range(ncb) if not (k - P - F <= b < k - P)]  # compact index -> buffer position
    M = len(nonfiller)
    c0 = nonfiller.index(pos[0] - P)
    counts = np.bincount(pos, minlength=n)
    assert (rm.rm.n, rm.rm.k, rm.rm.P, rm.rm.ncb) == (n, k, P, ncb)
    assert (rm.M, rm.c0, rm.hi, rm.max_reps) == (M, c0, int(pos.max()), int(counts.max()))
    assert (rm.rm.M, rm.rm.c0, rm.rm.hi, rm.rm.max_reps) == (M, c0, int(pos.max()), int(counts.max()))
    # the closed form: bit t is compact index (c0 + t) mod M ...
    lo = k - P - F
    cc = (c0 + np.arange(E)) % M
    assert np.array_equal(P + np.where(cc < lo, cc, cc + F), pos)
    # ... and compact index c receives t = r, r + M, ... < E, r = (c - c0) mod M
    for ci in {0, c0, M - 1, (c0 + E - 1) % M, (c0 + E) % M, M // 2}:
        p = P + nonfiller[ci]
        r = (ci - c0) % M
        assert np.array_equal(np.nonzero(pos == p)[0], np.arange(r, E, M)), (ci, p)
    # no filler and no punctured position is ever sent
    assert pos.min() >= P and not ((pos >= k - F) & (pos < k)).any() and pos.max() < P + ncb


def test_default_ncb_and_rv_start():
    L = _L()
    Z = 27
    rm = L.QCRateMatcher(base_of(Z), Z, 100, punctured=2)
    assert rm.ncb == NB * Z - 2 * Z and rm.M == rm.ncb and rm.fillers == 0 and rm.start == 0 and rm.filler_llr == 1024.0
    assert [rm.rv_start(v) for v in range(4)] == [(v * rm.ncb) // (4 * Z) * Z for v in range(4)]
    assert rm.rv_start(0) == 0 and all(rm.rv_start(v) % Z == 0 and rm.rv_start(v) < rm.ncb for v in range(4))
    assert "E=100" in repr(rm)


def _probe(*a):
    N = _N()
    out = N.RateMatch()
    rc = N.lib.pl_debug_rate_match_probe(*a, ctypes.byref(out))
    return rc, (N.lib.pl_last_error() or b"").decode(), out


def test_refusals_name_the_first_violated_condition():
    N = _N()
    Z = 7
    n, k = NB * Z, KB * Z  # 84, 28
    ok = (MB, NB, Z, 2, 5, -1, 3, 40)
    rc, _, out = _probe(*ok)
    assert rc == 0 and out.ncb == n - 2 * Z and out.E == 40
    bad = {
        "mb, nb and Z must be >= 1": [(0, NB, Z, 0, 0, -1, 0, 1), (MB, 0, Z, 0, 0, -1, 0, 1), (MB, NB, 0, 0, 0, -1, 0, 1)],
        "kb = nb - mb must be >= 1": [(8, 8, Z, 0, 0, -1, 0, 1), (9, 8, Z, 0, 0, -1, 0, 1)],
        "nb Z must fit 32 bits": [(1, 1 << 16, 1 << 15, 0, 0, -1, 0, 1)],
        "punctured = 4 outside 0 .. kb-1 = 3": [(MB, NB, Z, 4, 0, -1, 0, 1)],
        "punctured = -1 outside 0 .. kb-1 = 3": [(MB, NB, Z, -1, 0, -1, 0, 1)],
        "fillers = 15 outside 0 .. k - P = 14": [(MB, NB, Z, 2, 15, -1, 0, 1)],
        "fillers = -1 outside": [(MB, NB, Z, 0, -1, -1, 0, 1)],
        "ncb = 13 outside k - P = 14 .. n - P = 70": [(MB, NB, Z, 2, 0, 13, 0, 1)],
        "ncb = 71 outside k - P = 14 .. n - P = 70": [(MB, NB, Z, 2, 0, 71, 0, 1)],
        "start = 70 outside 0 .. ncb-1 = 69": [(MB, NB, Z, 2, 0, -1, 70, 1)],
        "start = -1 outside 0 .. ncb-1 = 27": [(MB, NB, Z, 0, 0, 28, -1, 1)],
        "E = 0 must be >= 1": [(MB, NB, Z, 0, 0, -1, 0, 0), ],
        "E = -5 must be >= 1": [(MB, NB, Z, 0, 0, -1, 0, -5)],
        "M = ncb - fillers = 0 must be >= 1": [(MB, NB, Z, 0, k, k, 0, 1), (MB, NB, Z, 2, 14, 14, 0, 1)],
    }
    for msg, calls in bad.items():
        for a in calls:
            rc, err, _ = _probe(*a)
            assert rc == N.PL_EINVAL and msg in err, (a, err)
    # the order: the first violated condition is the one named
    rc, err, _ = _probe(MB, NB, Z, 9, 99, 1, -1, 0)
    assert rc == N.PL_EINVAL and err.startswith("punctured")
    rc, err, _ = _probe(MB, NB, Z, 0, 99, 1, -1, 0)
    assert rc == N.PL_EINVAL and err.startswith("fillers")
    rc, err, _ = _probe(MB, NB, Z, 0, 0, 1, -1, 0)
    assert rc == N.PL_EINVAL and err.startswith("ncb")
    rc, err, _ = _probe(MB, NB, Z, 0, 0, -1, -1, 0)
    assert rc == N.PL_EINVAL and err.startswith("start")
    assert N.lib.pl_debug_rate_match_probe(*ok, None) == N.PL_EINVAL
    assert N.lib.pl_ldpc_rate_match_check(None) == N.PL_EINVAL
    # F = 5 where the code has fewer message bits left (Z = 1, k = 4)
    rc, err, _ = _probe(MB, NB, 1, 0, 5, -1, 0, 1)
    assert rc == N.PL_EINVAL and "fillers = 5 outside 0 .. k - P = 4" in err
    # the check entry point: derived fields written over whatever the caller left there
    rm = N.RateMatch(MB, NB, Z, 2, 5, -1, 3, 40, 1, 2, 3, 4, 5, 6, 7)
    assert N.lib.pl_ldpc_rate_match_check(ctypes.byref(rm)) == 0
    assert [getattr(rm, f) for f, _ in N.RateMatch._fields_] == [getattr(out, f) for f, _ in N.RateMatch._fields_]
    # the Python class raises what the library refuses, and its own for a base outside the structure
    L = _L()
    with pytest.raises(AssertionError, match="punctured = 4"):
        L.QCRateMatcher(base_of(Z), Z, 10, punctured=4)
    with pytest.raises(AssertionError, match="M = ncb - fillers = 0"):
        L.QCRateMatcher(base_of(Z), Z, 10, fillers=k, ncb=k)
    with pytest.raises(ValueError):
        L.QCRateMatcher(L.qc_random_base(4, 8, 7, 3, seed=115), 7, 10)
    with pytest.raises(AssertionError, match="n_out"):
        matcher(7, "p0_f0_rep").recover_host(np.zeros((1, matcher(7, "p0_f0_rep").E)), n_out=NB * 7 - 1)


@pytest.mark.parametrize("Z,name", CASES, ids=IDS)
def test_decoder_rows_and_base_against_a_scan(Z, name):
    L = _L()
    rm = matcher(Z, name)
    base = base_of(Z)
    pos = rm.positions_host()
    g = L.qc_encoding_structure(base)[0]
    assert g == 4
    want = next(r for r in range(max(g, 1), MB + 1) if (pos < (KB + r) * Z).all())
    assert rm.decoder_rows() == want and rm.n_dec == (KB + want) * Z
    db = rm.decoder_base()
    assert np.array_equal(db, base[:want, :KB + want])
    assert not (base[:want, KB + want:] >= 0).any()  # the rows kept involve no bit beyond n_dec
    assert L.qc_encoding_structure(db)[0] == g
    # a codeword of the whole code, cut to n_dec, is a codeword of the decoder's code
    msg = np.random.RandomState(Z).randint(0, 2, (3, KB * Z))
    cw = L.QCLDPCEncoder(base, Z).encode_batch(msg)
    small = L.QCLDPCEncoder(db, Z)
    assert all(small.verify_codeword(c[:rm.n_dec]) for c in cw)
    assert np.array_equal(small.encode_batch(msg), cw[:, :rm.n_dec])


def test_decoder_rows_of_a_base_without_extension():
    L = _L()
    Z = 27
    base = base_of(Z, core=None)
    assert L.qc_encoding_structure(base)[0] == MB
    for name in ("p0_f0_short", "p2_f5_ncbk_rep", "p0_f0_rep"):
        rm = matcher(Z, name, core=None)
        assert rm.decoder_rows() == MB and rm.n_dec == NB * Z and np.array_equal(rm.decoder_base(), base)
        assert np.array_equal(rm.positions_host(), matcher(Z, name).positions_host())  # the base plays no part


@pytest.mark.parametrize("Z,name", CASES, ids=IDS)
def test_recover_host_puts_each_llr_where_select_took_the_bit(Z, name):
    L = _L()
    rm = matcher(Z, name)
    n, k, E = rm.n, rm.k, rm.E
    pos = rm.positions_host()
    rs = np.random.RandomState(7 * Z + len(name))
    msg = rs.randint(0, 2, (3, k))
    msg[:, k - rm.fillers:] = 0
    cw = L.QCLDPCEncoder(base_of(Z), Z).encode_batch(msg)
    tx = rm.select_host(cw)
    assert tx.shape == (3, E) and np.array_equal(tx, cw[:, pos])
    # BPSK without noise: every transmitted position decides its codeword bit, fillers decide 0
    for n_out in (rm.n_dec, n):
        got = rm.recover_host(1.0 - 2.0 * tx, n_out=n_out)
        assert got.shape == (3, n_out) and got.dtype == np.float64
        sent = np.zeros(n_out, bool)
        sent[pos] = True
        assert np.array_equal(got[:, sent], (1.0 - 2.0 * cw[:, :n_out][:, sent]) * np.bincount(pos, minlength=n_out)[sent])
        fil = np.zeros(n_out, bool)
        fil[k - rm.fillers:k] = True
        assert (got[:, fil] == 1024.0).all() and not (sent & fil).any()
        assert (got[:, ~sent & ~fil] == 0).all() and not np.signbit(got[:, ~sent & ~fil]).any()
    # distinct LLRs: position p holds the sum of its t's, added in ascending t, in the output type
    llr = (rs.standard_normal((2, E)) * 3).astype(np.float32)
    for T in (np.float64, np.float32):
        got = rm.recover_host(llr, dtype=T)
        assert got.dtype == T
        for p in {int(pos[0]), int(pos[-1]), int(pos.max()), int(pos.min())}:
            want = None
            for t in np.nonzero(pos == p)[0]:
                want = llr[:, t].astype(T) if want is None else want + llr[:, t].astype(T)
            assert np.array_equal(got[:, p], want)
    # a single term is a copy: -0.0 stays -0.0; accumulate adds to the earlier recovery and keeps the rest
    z = np.full((1, E), -0.0)
    got = rm.recover_host(z)
    single = np.bincount(pos, minlength=rm.n_dec) == 1
    assert np.signbit(got[0, single]).all()
    first = rm.recover_host(llr.astype(np.float64))
    keep = first.copy()
    both = rm.recover_host(llr.astype(np.float64), out=first, accumulate=True)
    assert np.array_equal(first, keep)  # out is not modified
    sent = np.bincount(pos, minlength=rm.n_dec) > 0
    assert np.array_equal(both[:, sent], first[:, sent] + first[:, sent]) and np.array_equal(both[:, ~sent], first[:, ~sent])

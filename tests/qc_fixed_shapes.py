"""Case tables and builders of tests/test_ldpc_qc_fixed_shapes_host.py and
tests/test_gpu_ldpc_qc_fixed_shapes.py: QCFixedMSDecoder (ldpc_qc_fixed.hip on
ldpc_qc_frame.hpp, plan kernels 15 and 16) at every lifting size, planner edge,
check-word packing edge and rate-matched frame at which the kernel takes another
path.  No tests and no device use here.

The geometry columns of the tables are computed from the text of
qc_fixed_plan_build and qc_map (ldpc_plan.cpp), not read from the library; the host
file holds them against pl_debug_ldpc_qc_fixed_plan_probe:
    mw = 1 if maxdc <= 14 else 1 + ceil(maxdc / 32);  dcap = 8, 16, 32 up to those degrees, else 0
    state = align16(4 m mw + n)                       the check words, then the byte-wide P
    Z <= 64:  fpw = 64 // Z frames a wavefront; in LDS iff state fpw <= 160 KB;
              fpb = max(1, min(4, 65536 // (state fpw))), 4 on the workspace; threads = 64 fpb;
              lds = state fpw fpb, 0 on the workspace
    Z > 64:   fpw = fpb = 1; in LDS iff state + 128 vote bytes <= 160 KB; threads = roundup64(Z);
              lds = state + 128, or 128 on the workspace
Every builder asserts on the restatement (tests/qc_fixed_ref.py, the only reference)
the conditions its frames are there for, so a test that took its expectation from a
builder has them checked before the device is asked."""
import ctypes
import functools

import numpy as np

from qc_fixed_ref import qc_fixed_ms_ref, quantize_ref
from qc_layered_ref import block_row_vars
from test_gpu_ldpc_qc_shapes import _rows_base as rows_base, _stuck_frame

STD = dict(norm16=12, llr_scale=4.0, llr_max=31, msg_max=31)      # the decoder's default setting
FULL = dict(norm16=16, llr_scale=4.0, llr_max=127, msg_max=127)   # every field of a check word can fill
STUCK = dict(STD, llr_max=127)                                    # STD with the input clamp out of the way
LDS_MAX = 160 * 1024


def L():
    import polarcode_and_ldpc_amd.ldpc as L
    return L


def N():
    from polarcode_and_ldpc_amd import _native
    return _native


def awgn(n, frames, snr_db, seed):
    """All-zero codeword over BPSK + AWGN, LLR = 2 y / sigma^2."""
    rng = np.random.RandomState(seed)
    sigma = np.sqrt(1.0 / (2.0 * 10.0 ** (snr_db / 10.0)))
    return 2.0 * (1.0 + sigma * rng.randn(frames, n)) / sigma ** 2


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays[0] if len(arrays) == 1 else arrays


def probe(base, Z, max_iter, p):
    """pl_debug_ldpc_qc_fixed_plan_probe of (base, Z) at the setting p: the planner's geometry, no device call."""
    sh = np.ascontiguousarray(base, np.int32)
    out = N().LdpcQcFixedPlanProbe()
    rc = N().lib.pl_debug_ldpc_qc_fixed_plan_probe(sh.shape[0], sh.shape[1], Z, sh.ctypes.data_as(ctypes.c_void_p), None,
                                                   max_iter, 1, p["norm16"], p["llr_max"], p["msg_max"], 0,
                                                   ctypes.byref(out))
    assert rc == 0, N().lib.pl_last_error()
    return out


def geometry(p):
    """A probe as the tables spell a plan."""
    return dict(kernel=p.kernel, dcap=p.dcap, mw=p.mw, fpw=p.fpw, fpb=p.fpb, threads=p.threads, lds=p.lds_bytes,
                use_global=p.use_global, state=p.state_bytes)


def _g(kernel, dcap, mw, fpw, fpb, threads, lds, state):
    return dict(kernel=kernel, dcap=dcap, mw=mw, fpw=fpw, fpb=fpb, threads=threads, lds=lds,
                use_global=int(kernel == 16), state=state)


def ref(base, Z, llr, p, max_iter, early_stop=True, layer_order=None):
    """(bits, iterations, posteriors) of the restatement, read-only."""
    return frozen(*qc_fixed_ms_ref(base, Z, llr, max_iter, p["norm16"], p["llr_max"], p["msg_max"], early_stop,
                                   layer_order)[:3])


def unsatisfied(base, Z, bits):
    """(block row, index within it) of the checks one frame's decisions leave unsatisfied."""
    out = []
    for i in range(np.asarray(base).shape[0]):
        V = block_row_vars(np.asarray(base), Z, i)
        out += [(i, int(r)) for r in np.nonzero(np.bitwise_xor.reduce(bits[V], axis=1))[0]]
    return out


def mixed(its, max_iter):
    """Some frame stops before max_iter and some frame runs all of it."""
    return bool(its.min() < max_iter and its.max() == max_iter)


# ---- a. lifting sizes ------------------------------------------------------------------
# qc_random_base(4, 8, Z, 3, seed): rows of at most 8 blocks, one word a check, n = 8 Z, m = 4 Z,
# state = align16(24 Z).  Z = 2, 3: 32 and 21 frames a wavefront, the stop mask shifted by up to 62 bits;
# 32: the second frame's mask in bits 32..63; 33, 63: fpw == 1 with idle lanes of lane / Z == 1; 65: a second
# wavefront with one working lane; 128: two full wavefronts; 384: six; 1000, 1024: all 16 vote words.
Z_ITER = 20
Z_SNR = (-1.0, -5.0)  # even, odd frames
LIFT = {
    2: _g(15, 8, 1, 32, 4, 256, 6144, 48),
    3: _g(15, 8, 1, 21, 4, 256, 6720, 80),
    32: _g(15, 8, 1, 2, 4, 256, 6144, 768),
    33: _g(15, 8, 1, 1, 4, 256, 3200, 800),
    63: _g(15, 8, 1, 1, 4, 256, 6080, 1520),
    65: _g(15, 8, 1, 1, 1, 128, 1696, 1568),
    128: _g(15, 8, 1, 1, 1, 128, 3200, 3072),
    384: _g(15, 8, 1, 1, 1, 384, 9344, 9216),
    1000: _g(15, 8, 1, 1, 1, 1024, 24128, 24000),
    1024: _g(15, 8, 1, 1, 1, 1024, 24704, 24576),
}
# Z: the smallest index r, within their block rows, of the checks of the stuck frame's one negative variable
STUCK_R = {65: 51, 128: 124, 384: 329, 1000: 700, 1024: 790}
# Z: the seed of the base.  At Z = 128 the base of seed 108 + Z has a second variable in two of the stuck
# variable's checks; it turns negative in iteration 1 and leaves checks below r unsatisfied
Z_SEED = {128: 237}


def fpg(Z):
    return LIFT[Z]["fpw"] * LIFT[Z]["fpb"]


@functools.lru_cache(maxsize=None)
def z_base(Z):
    return frozen(L().qc_random_base(4, 8, Z, 3, seed=Z_SEED.get(Z, 108 + Z)))


@functools.lru_cache(maxsize=None)
def z_pool(Z):
    """fpg + 1 frames (one workgroup and one frame more); 16, or 9 at Z >= 384, for one frame per workgroup.
    Even frames at -1 dB, odd frames at -5 dB, quantised at STD.  For Z > 64 the last frame is the stuck
    one: every LLR +8 and one of -127."""
    frames = fpg(Z) + 1 if fpg(Z) > 1 else (9 if Z >= 384 else 16)
    llr = np.empty((frames, 8 * Z))
    llr[0::2] = awgn(8 * Z, (frames + 1) // 2, Z_SNR[0], seed=1000 + Z)
    llr[1::2] = awgn(8 * Z, frames // 2, Z_SNR[1], seed=2000 + Z)
    q = quantize_ref(llr, STD["llr_scale"], STD["llr_max"])
    if Z > 64:
        q[-1] = stuck_frame(Z)[0]
    return frozen(q)


@functools.lru_cache(maxsize=None)
def stuck_frame(Z):
    """(frame int8, r): _stuck_frame's construction in int8: +8 everywhere and -127 at the variable whose
    checks have the largest smallest index r within their block rows."""
    f, r = _stuck_frame(z_base(Z), Z)
    frame = np.full(8 * Z, 8, dtype=np.int8)
    frame[int(np.argmin(f))] = -127
    assert (frame == -127).sum() == 1 and (frame == 8).sum() == 8 * Z - 1
    return frozen(frame), r


def z_batches(Z):
    return sorted({1, max(fpg(Z) - 1, 1), fpg(Z) + 1, len(z_pool(Z))})


@functools.lru_cache(maxsize=None)
def z_want(Z, early_stop):
    base, llr = z_base(Z), z_pool(Z)
    assert (base >= 0).sum(axis=1).max() <= 8
    want = ref(base, Z, llr, STD, Z_ITER, early_stop)
    its = want[1]
    if early_stop:
        assert mixed(its, Z_ITER), its
        for B in z_batches(Z):
            if B >= 2:
                assert mixed(its[:B], Z_ITER), (B, its)  # every batch above one frame holds both kinds
        if Z <= 32:  # several frames per wavefront: they differ within the first wavefront too
            assert len(set(its[:64 // Z].tolist())) > 1
    else:
        assert (its == Z_ITER).all()
    return want


@functools.lru_cache(maxsize=None)
def stuck_want(Z, early_stop):
    """The pool at llr_max = 127, where the stuck frame's -127 stands.  It never stops, and after iteration 1
    every unsatisfied check sits at index >= r of its block row -- at Z >= 384 past the fourth wavefront, so
    an early-stop vote that misses the word of a later wavefront stops it there."""
    base, llr = z_base(Z), z_pool(Z)
    frame, r = stuck_frame(Z)
    assert Z > 64 and np.array_equal(llr[-1], frame) and r == STUCK_R[Z] and (Z < 384 or r >= 256)
    want = ref(base, Z, llr, STUCK, Z_ITER, early_stop)
    at = int(np.argmin(frame))  # the stuck variable
    first = ref(base, Z, llr[-1:], STUCK, 1, False)
    assert want[1][-1] == Z_ITER and first[2][0][at] <= -34 and want[2][-1][at] <= -34
    bad = unsatisfied(base, Z, (first[2][0] <= 0).astype(np.int64))  # the syndrome of the one-iteration posteriors
    assert bad and min(i_r[1] for i_r in bad) >= r
    if early_stop:
        assert mixed(want[1], Z_ITER)
    return want


# Row degrees [12, 24, 3, 32] at Z = 1024: the 32-register instance at 1024 threads; two words a check:
# 8 m + n = 65 536 bytes, in LDS (the fp64 state of the same code is not)
D32 = dict(degrees=[12, 24, 3, 32], nb=32, Z=1024, max_iter=5, snr=(10.0, 3.0, -5.0))
D32_GEOM = _g(15, 32, 2, 1, 1, 1024, 65664, 65536)


@functools.lru_cache(maxsize=None)
def d32_case():
    Z, nb = D32["Z"], D32["nb"]
    base = rows_base(D32["degrees"], nb, Z, seed=24)
    llr = np.concatenate([awgn(nb * Z, 1, s, seed=40 + k) for k, s in enumerate(D32["snr"])])
    return frozen(base, quantize_ref(llr, STD["llr_scale"], STD["llr_max"]))


@functools.lru_cache(maxsize=None)
def d32_want():
    base, llr = d32_case()
    want = ref(base, D32["Z"], llr, STD, D32["max_iter"])
    assert mixed(want[1], D32["max_iter"]), want[1]
    return want


# ---- b. planner edges ------------------------------------------------------------------
# name: (row degrees' common value, mb, nb, Z, frames, geometry).  Pairs: the largest plan that keeps the state
# in LDS (kernel 15) and its neighbour, the smallest on the workspace (kernel 16): one step in Z (block
# mapping) or in nb (sub-wave mapping).  Then the fpb ladder: Z = 32, mb = 32, state = 4096 + 32 nb,
# fpb = min(4, 65536 // (2 state)).
EDGE_ITER = 6
EDGE_SNR = (10.0, 8.0, -5.0)  # frame k at EDGE_SNR[k % 3]
EDGES = {
    "block_1w_lds": (6, 20, 80, 1023, 3, _g(15, 8, 1, 1, 1, 1024, 163808, 163680)),
    "block_1w_ws": (6, 20, 80, 1024, 3, _g(16, 8, 1, 1, 1, 1024, 128, 163840)),
    "block_2w_lds": (20, 10, 80, 1023, 3, _g(15, 32, 2, 1, 1, 1024, 163808, 163680)),
    "block_2w_ws": (20, 10, 80, 1024, 3, _g(16, 32, 2, 1, 1, 1024, 128, 163840)),
    "subwave_lds": (6, 256, 1536, 32, 3, _g(15, 8, 1, 2, 1, 64, 163840, 81920)),
    "subwave_ws": (6, 256, 1537, 32, 3, _g(16, 8, 1, 2, 4, 256, 0, 81952)),
    "z1_lds": (6, 256, 1536, 1, 65, _g(15, 8, 1, 64, 1, 64, 163840, 2560)),
    "z1_ws": (6, 256, 1537, 1, 65, _g(16, 8, 1, 64, 4, 256, 0, 2576)),
    "fpb_128": (6, 32, 128, 32, 9, _g(15, 8, 1, 2, 4, 256, 65536, 8192)),
    "fpb_129": (6, 32, 129, 32, 7, _g(15, 8, 1, 2, 3, 192, 49344, 8224)),
    "fpb_213": (6, 32, 213, 32, 7, _g(15, 8, 1, 2, 3, 192, 65472, 10912)),
    "fpb_214": (6, 32, 214, 32, 5, _g(15, 8, 1, 2, 2, 128, 43776, 10944)),
    "fpb_384": (6, 32, 384, 32, 5, _g(15, 8, 1, 2, 2, 128, 65536, 16384)),
    "fpb_385": (6, 32, 385, 32, 3, _g(15, 8, 1, 2, 1, 64, 32832, 16416)),
}


@functools.lru_cache(maxsize=None)
def edge_case(name):
    deg, mb, nb, Z, frames, _ = EDGES[name]
    base = rows_base([deg] * mb, nb, Z, seed=7 + nb + Z)
    llr = np.empty((frames, nb * Z))
    for k in range(3):
        llr[k::3] = awgn(nb * Z, len(range(k, frames, 3)), EDGE_SNR[k], seed=50 + k)
    return frozen(base, quantize_ref(llr, STD["llr_scale"], STD["llr_max"]))


@functools.lru_cache(maxsize=None)
def edge_want(name):
    base, llr = edge_case(name)
    deg, mb, nb, Z, frames, g = EDGES[name]
    assert ((base >= 0).sum(axis=1) == deg).all() and len(llr) == frames
    want = ref(base, Z, llr, STD, EDGE_ITER)
    assert mixed(want[1], EDGE_ITER), want[1]
    if name.startswith("fpb"):
        # fpg + 1 frames: the workgroup's later wavefronts hold live frames, of both kinds
        assert frames == g["fpw"] * g["fpb"] + 1
        if g["fpb"] > 1:
            assert mixed(want[1][g["fpw"]:frames - 1], EDGE_ITER)
    if name.startswith("z1"):
        assert frames == g["fpw"] + 1  # a second wavefront (a second workgroup on the LDS side) runs
    return want


# ---- c. check-word packing edges ---------------------------------------------------------
# name: (row degrees, widest first so that iteration 1 sees the crafted inputs untouched; nb; Z; max_iter;
# noisy frames; geometry).  One word a check (7 + 7 + 4 + 14 bits) up to degree 14; above, 8 + 8 + 11 bits
# and the parity in word 0 and 32 flags a word behind it.
PACK = {
    "deg8": ([8, 5, 3], 12, 7, 8, 3, _g(15, 8, 1, 9, 4, 256, 6336, 176)),            # the 8-register instance full
    "deg14": ([14, 9, 4], 20, 7, 8, 3, _g(15, 16, 1, 9, 4, 256, 8064, 224)),         # one word full: idx1 13, flag bit 31
    "deg16": ([16, 9, 4], 20, 7, 8, 3, _g(15, 16, 2, 9, 4, 256, 11520, 320)),        # the 16-register instance, two words
    "deg32": ([32, 20, 5], 40, 7, 8, 3, _g(15, 32, 2, 9, 4, 256, 16128, 448)),       # a flag word full, bit 31
    "deg33": ([33, 20, 5], 40, 7, 8, 3, _g(15, 0, 3, 9, 4, 256, 19584, 544)),        # the two-pass form, one flag in word 2
    "deg64": ([64, 33, 5], 70, 7, 8, 3, _g(15, 0, 3, 9, 4, 256, 27072, 752)),        # two flag words full
    "deg65": ([65, 64, 33], 70, 7, 8, 3, _g(15, 0, 4, 9, 4, 256, 29952, 832)),       # one flag in word 3
    "deg2047": ([2047, 40], 2047, 2, 3, 0, _g(16, 0, 65, 32, 4, 256, 0, 5136)),      # all 11 bits of idx1 beside the parity
}
CRAFTED = ("min_last", "all_negative", "last_negative", "zero_last", "zeros_last_two", "all_127")


@functools.lru_cache(maxsize=None)
def pack_case(name):
    """(base, llr): the noisy frames (2 dB), then the six crafted frames, CRAFTED in order: on the inputs V of
    every check of the widest row
      min_last        the strictly smallest |L| at the last input, either sign: idx1 = d - 1
      all_negative    every flag set, parity d mod 2
      last_negative   the magnitudes of all_negative, only the last input negative: the top flag of the last word
      zero_last       a single 0, at the last input
      zeros_last_two  zeros at the last two inputs
      all_127         every |L| = 127, either sign: both stored minima 127"""
    degrees, nb, Z, _, noisy, _ = PACK[name]
    base = rows_base(degrees, nb, Z, seed=len(name) + degrees[0])
    V = block_row_vars(base, Z, 0)
    d = V.shape[1]
    assert d == max(degrees) == degrees[0] == int(name[3:])
    last, last2 = V[:, d - 1], V[:, d - 2]
    llr = quantize_ref(awgn(nb * Z, noisy + len(CRAFTED), 2.0, seed=61), FULL["llr_scale"], FULL["llr_max"])
    c = llr[noisy:]
    rng = np.random.RandomState(62)
    away = lambda x, k: np.where(x < 0, np.minimum(x, -k), np.maximum(x, k)).astype(np.int8)  # noqa: E731  |x| >= k
    c[0, V] = away(c[0, V], 3)
    c[0, last] = rng.choice([-2, -1, 1, 2], Z)
    c[1, V] = -np.abs(away(c[1, V], 1))
    c[2, V] = np.abs(c[1, V])
    c[2, last] = c[1, last]
    for k in (3, 4):
        c[k, V] = away(c[k, V], 1)
    c[3, last] = 0
    c[4, last] = 0
    c[4, last2] = 0
    c[5, V] = rng.choice([-127, 127], V.shape)
    return frozen(base, llr)


@functools.lru_cache(maxsize=None)
def pack_want(name, early_stop):
    """The crafted properties on L[V], then the restatement."""
    base, llr = pack_case(name)
    degrees, nb, Z, max_iter, noisy, _ = PACK[name]
    V = block_row_vars(np.asarray(base), Z, 0)
    d = V.shape[1]
    assert len(llr) == noisy + 6 and (np.abs(llr.astype(np.int64)) <= 127).all()
    c = {k: llr[noisy + i].astype(np.int64)[V] for i, k in enumerate(CRAFTED)}  # [Z, d] each
    a = np.sort(np.abs(c["min_last"]), axis=1)
    assert (np.abs(c["min_last"]).argmin(axis=1) == d - 1).all() and (a[:, 0] < a[:, 1]).all() and (a[:, 0] > 0).all()
    assert len(set(np.sign(c["min_last"][:, d - 1]).tolist())) == 2 or Z < 3  # either sign
    assert (c["all_negative"] < 0).all()
    assert (c["last_negative"][:, :d - 1] > 0).all() and (c["last_negative"][:, d - 1] < 0).all()
    assert np.array_equal(np.abs(c["last_negative"]), np.abs(c["all_negative"]))
    assert ((c["zero_last"] == 0).sum(axis=1) == 1).all() and (c["zero_last"][:, d - 1] == 0).all()
    assert ((c["zeros_last_two"] == 0).sum(axis=1) == 2).all() and (c["zeros_last_two"][:, d - 2:] == 0).all()
    assert (np.abs(c["all_127"]) == 127).all() and (c["all_127"] < 0).any() and (c["all_127"] > 0).any()
    want = ref(base, Z, llr, FULL, max_iter, early_stop)
    # the flags matter: the same magnitudes with other signs give other posteriors
    assert not np.array_equal(want[2][noisy + 1], want[2][noisy + 2])
    return want


# ---- d. rate-matched frames ------------------------------------------------------------
# name: (frames, SNR of the even frames, of the odd frames, in dB, geometry); the NR-like bases of
# tests/test_gpu_ldpc_qc_shapes.py: (6, 10, 7) with rows of up to 7 blocks, (8, 12, 65) up to 5, (6, 10, 384) up to 6
RATE_ITER = 20
RATE = {
    "z7_core4_nr": (32, 3.0, -3.0, _g(15, 8, 1, 9, 4, 256, 8640, 240)),
    "z65_core4_nr": (16, 3.0, -3.0, _g(15, 8, 1, 1, 1, 128, 2992, 2864)),
    "z384_core4_nr": (8, 3.0, -3.0, _g(15, 8, 1, 1, 1, 384, 13184, 13056)),
}


@functools.lru_cache(maxsize=None)
def rate_base(name):
    if name == "z384_core4_nr":
        return frozen(L().qc_encodable_base(6, 10, 384, 3, 3, core=4, chained=False)), 384
    from test_ldpc_qc_encode_host import base_of
    return base_of(name)


@functools.lru_cache(maxsize=None)
def rate_case(name):
    """(base, Z, llr int8, codewords, filler positions): codewords of QCLDPCEncoder (host) over BPSK + AWGN,
    quantised at STD; then the first two block columns punctured (0) and the last Z // 2 + 3 information
    positions, zero filler bits in the message, known (+llr_max)."""
    base, Z = rate_base(name)
    frames, hi, lo, _ = RATE[name]
    mb, nb = base.shape
    kb, fill = nb - mb, Z // 2 + 3
    rng = np.random.RandomState(70 + Z)
    msg = rng.randint(0, 2, (frames, kb * Z)).astype(np.uint8)
    msg[:, kb * Z - fill:] = 0
    cw = np.asarray(L().QCLDPCEncoder(np.array(base), Z).encode_batch(msg)).astype(np.int64)
    assert (cw[:, :kb * Z] == msg).all()  # systematic: the filler positions are codeword positions
    sigma = np.sqrt(1.0 / (2.0 * 10.0 ** (np.where(np.arange(frames) % 2 == 0, hi, lo) / 10.0)))[:, None]
    llr = quantize_ref(2.0 * ((1.0 - 2.0 * cw) + sigma * rng.randn(frames, nb * Z)) / sigma ** 2,
                       STD["llr_scale"], STD["llr_max"])
    fillers = np.arange(kb * Z - fill, kb * Z)
    llr[:, :2 * Z] = 0
    llr[:, fillers] = STD["llr_max"]
    return np.array(base), Z, frozen(llr), frozen(cw), fillers


def rate_layer_order(base):
    """(order, both): the block rows that read both punctured block columns first, then the others.  In the
    natural order a row that reads one of the two columns writes it before a row that reads both comes
    (at Z = 65, rows 0 and 1 before row 5, the only one), and that row's minimum is no longer 0."""
    both = [i for i in range(base.shape[0]) if base[i, 0] >= 0 and base[i, 1] >= 0]
    return both + [i for i in range(base.shape[0]) if i not in both], both


@functools.lru_cache(maxsize=None)
def rate_want(name, early_stop, reordered=True):
    """reordered: the layer order of rate_layer_order; otherwise the natural order, on the same frames."""
    base, Z, llr, cw, fillers = rate_case(name)
    order, both = rate_layer_order(base)
    assert both and (llr[:, :2 * Z] == 0).all() and (llr[:, fillers] == STD["llr_max"]).all()
    # every check that reads both punctured columns has two zero inputs in iteration 1: every minimum over the
    # others is 0 and every message 0, so one iteration over those rows alone, the first of the order, moves no
    # posterior
    first = ref(base[both], Z, llr, STD, 1, False)
    assert np.array_equal(first[2], llr)
    want = ref(base, Z, llr, STD, RATE_ITER, early_stop, order if reordered else None)
    assert (want[2][:, fillers] > 0).all()
    assert (want[0][0::2] == cw[0::2]).all()  # 3 dB: the codewords sent, with or without early stop
    if early_stop:
        assert (want[1][0::2] < RATE_ITER).all() and want[1].max() == RATE_ITER, want[1]
    else:
        assert (want[1] == RATE_ITER).all()
    return want


# ---- e. what the tables reach ----------------------------------------------------------
def all_geometries():
    """name -> (base, Z, max_iter, setting, geometry row) of every case of a. to d."""
    g = {}
    for Z, row in LIFT.items():
        g["lift_%d" % Z] = (z_base(Z), Z, Z_ITER, STD, row)
        if Z > 64:
            g["stuck_%d" % Z] = (z_base(Z), Z, Z_ITER, STUCK, row)
    g["d32"] = (d32_case()[0], D32["Z"], D32["max_iter"], STD, D32_GEOM)
    for name, row in EDGES.items():
        g["edge_" + name] = (edge_case(name)[0], row[3], EDGE_ITER, STD, row[5])
    for name, row in PACK.items():
        g["pack_" + name] = (pack_case(name)[0], row[2], row[3], FULL, row[5])
    for name, row in RATE.items():
        g["rate_" + name] = (rate_base(name)[0], rate_base(name)[1], RATE_ITER, STD, row[3])
    return g

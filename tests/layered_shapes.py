"""Case tables and builders of tests/test_ldpc_layered_shapes_host.py and
tests/test_gpu_ldpc_layered_shapes.py: LayeredMSDecoder (ldpc_layered.hip,
ldpc_layered_kernel<WAVE, GLOBAL>) at every layer width, planner edge, packing
edge and layer shape at which lms_geom or lms_check_update takes another path,
and lms_decode_impl's chunks for all four layered decoders.

The geometry columns of the tables are computed from the text of lms_geom
(ldpc_plan.cpp), not read from the library; the host file holds them against
pl_debug_ldpc_layered_plan_probe:
    mw = 1 if maxdc <= 16 else 1 + ceil(maxdc / 32)
    state = align16(align16(8 n) + 16 m + 4 m mw)
    WAVE (largest layer <= 64): in LDS iff state <= 160 KB; fpb = max(1, min(4, 65536 // state)),
        4 on the workspace; threads = 64 fpb; lds = state fpb
    block: in LDS iff state + 128 <= 160 KB; fpb = 1; threads = min(1024, roundup64(largest layer));
        lds = state + 128, or 128 on the workspace
Every builder asserts on the restatement the conditions its frames are there
for (frames that stop early and frames that run to max_iter, the position of a
minimum, a NaN posterior), so a test that took its expectation from a builder
has them checked before the device is asked."""
import ctypes
import functools

import numpy as np

from layered_ref import layered_ms_ref
from qc_layered_ref import block_row_vars, qc_layered_ms_ref
from test_gpu_ldpc_qc_shapes import PACK as QC_PACK, _pack_case, _rows_base, _stuck_frame

NORM = 0.75


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


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def probe(row_ptr, col_idx, n, layers, max_iter, force_global=0):
    """pl_debug_ldpc_layered_plan_probe of (CSR, layers): the planner's geometry, no device call."""
    rp = np.ascontiguousarray(row_ptr, np.int32)
    ci = np.ascontiguousarray(col_idx, np.int32)
    lp = np.zeros(len(layers) + 1, np.int32)
    lp[1:] = np.cumsum([len(l) for l in layers])
    lr = np.ascontiguousarray(np.concatenate([np.asarray(l, np.int32).ravel() for l in layers]), np.int32)
    out = N().LdpcLayeredPlanProbe()
    rc = N().lib.pl_debug_ldpc_layered_plan_probe(len(rp) - 1, n, _ptr(rp), _ptr(ci), len(layers), _ptr(lp), _ptr(lr),
                                                  max_iter, 1, NORM, 0, 0, force_global, ctypes.byref(out))
    assert rc == 0, N().lib.pl_last_error()
    return out


def qc_probe(base, Z, max_iter, force_global=0):
    """probe() of the expanded H with the block rows as layers, without the dense matrix."""
    base = np.asarray(base)
    rp, ci = L().qc_to_csr(base, Z)
    return probe(rp, ci, base.shape[1] * Z, L().qc_block_layers(base.shape[0], Z), max_iter, force_global)


def geometry(p):
    """A probe as the tables spell a plan; trips: those of the kernel's layer loop at the widest layer."""
    return dict(wave=p.wave, use_global=p.use_global, fpb=p.fpb, threads=p.threads, mw=p.mw,
                state=p.state_bytes, lds=p.lds_bytes,
                trips=1 if p.wave else -(-p.max_layer // p.threads))


def _g(wave, use_global, fpb, threads, mw, state, lds, trips=1):
    return dict(wave=wave, use_global=use_global, fpb=fpb, threads=threads, mw=mw, state=state, lds=lds, trips=trips)


# ---- a. layer widths -------------------------------------------------------------------
# qc_random_base(2, 4, Z, 2, seed): both block rows have degree 4, n = 4 Z, m = 2 Z, state = align16(72 Z)
WIDTH_ITER = 10
WIDTH_FRAMES = 5
WIDTH_SNR_HI = 2.0
# Z: the odd frames' SNR in dB.  At Z >= 1024 frames at 0 dB (almost) never stop within 10 iterations; the
# short codes stop by iteration 4 there and need a noisier channel for a frame that does not
WIDTH_SNR_LO = {64: -4.0, 65: -4.0, 1024: 0.0, 1025: 0.0, 2049: 0.0}
WIDTHS = {
    64: _g(1, 0, 4, 256, 1, 4608, 18432),              # the widest layer a wavefront takes
    65: _g(0, 0, 1, 128, 1, 4688, 4816),               # second wavefront with one working lane
    1024: _g(0, 0, 1, 1024, 1, 73728, 73856),          # 16 wavefronts, all 16 vote words, one check per thread
    1025: _g(0, 0, 1, 1024, 1, 73808, 73936, 2),       # second trip of the layer loop, taken by thread 0 alone
    2049: _g(0, 0, 1, 1024, 1, 147536, 147664, 3),     # third trip, one check; state still in LDS
}
WIDTH_GLOBAL = {1025: _g(0, 1, 1, 1024, 1, 73808, 128, 2)}  # PL_LMS_GLOBAL=1: the strided loop on workspace state


@functools.lru_cache(maxsize=None)
def width_base(Z):
    return frozen(L().qc_random_base(2, 4, Z, 2, seed=300 + Z))


@functools.lru_cache(maxsize=None)
def width_llr(Z):
    """Five frames, even ones at 2 dB and odd ones at WIDTH_SNR_LO[Z]; at Z = 1024 a sixth, _stuck_frame."""
    n = 4 * Z
    llr = np.empty((WIDTH_FRAMES + (Z == 1024), n))
    llr[0:WIDTH_FRAMES:2] = awgn(n, 3, WIDTH_SNR_HI, seed=3000 + Z)
    llr[1:WIDTH_FRAMES:2] = awgn(n, 2, WIDTH_SNR_LO[Z], seed=4000 + Z)
    if Z == 1024:
        llr[-1] = _stuck_frame(width_base(Z), Z)[0]
    return frozen(llr)


def width_batches(Z):
    """1 and all frames; at Z = 64 also 5: one workgroup of four and a ragged one."""
    return sorted({1, WIDTH_FRAMES, len(width_llr(Z))})


def unsatisfied(base, Z, bits):
    """(block row, index within it) of the checks one frame's decisions leave unsatisfied."""
    out = []
    for i in range(np.asarray(base).shape[0]):
        V = block_row_vars(np.asarray(base), Z, i)
        out += [(i, int(r)) for r in np.nonzero(np.bitwise_xor.reduce(bits[V], axis=1))[0]]
    return out


@functools.lru_cache(maxsize=None)
def width_want(Z, early_stop):
    base, llr = width_base(Z), width_llr(Z)
    assert ((base >= 0).sum(axis=1) == 4).all()
    want = qc_layered_ms_ref(base, Z, llr, WIDTH_ITER, NORM, early_stop, dtype=np.float64)
    its = want[1]
    if early_stop:
        print("Z", Z, "restatement iterations:", its)
        assert its[:WIDTH_FRAMES].min() < WIDTH_ITER and its[:WIDTH_FRAMES].max() == WIDTH_ITER
        assert its[0] < WIDTH_ITER  # the batch of one stops early
        if Z == 1024:
            # the stuck frame never stops, and what keeps it going after iteration 1 lies past the eighth
            # wavefront (check i Z + r votes in wavefront r // 64): a vote that drops the words of late
            # wavefronts stops it there
            assert its[-1] == WIDTH_ITER and _stuck_frame(base, Z)[1] >= 512
            first = qc_layered_ms_ref(base, Z, llr[-1:], 1, NORM, False, dtype=np.float64)
            assert first[0].sum() == 1  # after iteration 1 that variable alone is wrong
            bad = unsatisfied(base, Z, first[0][0])
            assert len(bad) == 2 and min(r for _, r in bad) >= 512
    else:
        assert (its == WIDTH_ITER).all()
    return frozen(*want)


# ---- b. planner edges ------------------------------------------------------------------
# The WAVE ladder: qc_random_base(4, 8, 64, 3, seed) in the first 8 block columns of a (4, nb) base, the
# other block columns empty.  Row degrees <= 8: mw = 1, state = 64 (8 nb + 80).
LADDER_Z, LADDER_ITER, LADDER_FRAMES = 64, 20, 9
LADDER_SNR = (-1.0, -5.0)  # even, odd frames
LADDER = {
    22: _g(1, 0, 4, 256, 1, 16384, 65536),
    23: _g(1, 0, 3, 192, 1, 16896, 50688),
    32: _g(1, 0, 3, 192, 1, 21504, 64512),
    33: _g(1, 0, 2, 128, 1, 22016, 44032),
    54: _g(1, 0, 2, 128, 1, 32768, 65536),
    55: _g(1, 0, 1, 64, 1, 33280, 33280),
    310: _g(1, 0, 1, 64, 1, 163840, 163840),   # the last one in LDS
    311: _g(1, 1, 4, 256, 1, 164352, 0),       # the workspace, the planner's own choice
}


@functools.lru_cache(maxsize=None)
def ladder_base(nb):
    core = L().qc_random_base(4, 8, LADDER_Z, 3, seed=164)
    assert (core >= 0).sum(axis=1).max() <= 8
    base = np.full((4, nb), -1, dtype=np.int64)
    base[:, :8] = core
    return frozen(base)


@functools.lru_cache(maxsize=None)
def ladder_llr(nb):
    """Nine frames; the 512 variables the checks read are the same draw at every nb."""
    llr = awgn(nb * LADDER_Z, LADDER_FRAMES, 0.0, seed=5000 + nb)  # the variables of no check: any value
    llr[0::2, :512] = awgn(512, 5, LADDER_SNR[0], seed=5001)
    llr[1::2, :512] = awgn(512, 4, LADDER_SNR[1], seed=5002)
    return frozen(llr)


def ladder_batches(nb):
    fpb = LADDER[nb]["fpb"]
    return sorted({1, fpb, fpb + 1, LADDER_FRAMES})  # a workgroup full, ragged, and followed by a second


@functools.lru_cache(maxsize=None)
def ladder_want(nb, early_stop):
    base, llr = ladder_base(nb), ladder_llr(nb)
    want = qc_layered_ms_ref(base, LADDER_Z, llr, LADDER_ITER, NORM, early_stop, dtype=np.float64)
    its = want[1]
    if early_stop:
        print("nb", nb, "restatement iterations:", its)
        assert its.min() < LADDER_ITER and its.max() == LADDER_ITER
        assert its[0] < LADDER_ITER and its[1] == LADDER_ITER  # every batch above one frame holds both kinds
    else:
        assert (its == LADDER_ITER).all()
    # a variable of no check keeps its LLR
    assert np.array_equal(want[2][:, 512:], llr[:, 512:]) and not np.array_equal(want[2][:, :512], llr[:, :512])
    return frozen(*want)


# The block mapping's LDS edge: state + 128 vote bytes <= 160 KB.  The QC suite's pair, through the generic decoder
EDGE_ITER = 3
BLOCK_EDGE = {
    909: _g(0, 0, 1, 960, 1, 163632, 163760),
    910: _g(0, 1, 1, 960, 1, 163808, 128),
}


@functools.lru_cache(maxsize=None)
def edge_case(Z):
    base = L().qc_random_base(5, 10, Z, 3, seed=7)
    assert (base >= 0).sum(axis=1).max() <= 16
    llr = np.concatenate([awgn(10 * Z, 2, 2.0, seed=51), awgn(10 * Z, 1, -5.0, seed=52)])
    return frozen(base, llr)


@functools.lru_cache(maxsize=None)
def edge_want(Z, early_stop):
    base, llr = edge_case(Z)
    want = qc_layered_ms_ref(base, Z, llr, EDGE_ITER, NORM, early_stop, dtype=np.float64)
    if early_stop:
        print("Z", Z, "restatement iterations:", want[1])
        assert want[1].min() < EDGE_ITER and want[1].max() == EDGE_ITER
    return frozen(*want)


# ---- c. packing edges ------------------------------------------------------------------
# name: (row degrees, widest first so that iteration 1 sees the crafted inputs untouched; nb; Z; max_iter; noisy
# frames): the two the QC suite's table lacks, the first degrees of the two-word and three-word forms
PACK_MORE = {
    "deg17": ([17, 9, 4], 20, 7, 8, 4),
    "deg33": ([33, 20, 5], 40, 7, 8, 4),
}
PACKS = {
    "deg16": _g(1, 0, 4, 256, 1, 1552, 6208),       # one word full: idx1 / nidx 15
    "deg17": _g(1, 0, 4, 256, 2, 1632, 6528),       # the first degree of the two-word form
    "deg33": _g(1, 0, 4, 256, 3, 2832, 11328),      # ... of the three-word form
    "deg65": _g(1, 0, 4, 256, 4, 4592, 18368),      # the flag words' boundaries
    "deg2047": _g(1, 0, 1, 64, 65, 33856, 33856),   # all 11 position bits
}


@functools.lru_cache(maxsize=None)
def pack_case(name):
    """(base, Z, max_iter, llr): noisy frames, then (i) the smallest |LLR| of every check of the widest row at
    its last input, (ii) a single NaN there, (iii) a single zero there, (iv) two zeros at the last two inputs."""
    if name in QC_PACK:
        return _pack_case(name)[:4]
    degrees, nb, Z, max_iter, noisy = PACK_MORE[name]
    base = _rows_base(degrees, nb, Z, seed=len(name) + degrees[0])
    V = block_row_vars(base, Z, 0)
    d = V.shape[1]
    assert d == max(degrees) == degrees[0]
    last, last2 = V[:, d - 1], V[:, d - 2]
    llr = awgn(nb * Z, noisy + 4, 2.0, seed=61)
    c = llr[noisy:]
    rng = np.random.RandomState(62)
    c[0, last] = 0.25 * np.abs(c[0]).min() * rng.choice([-1.0, 1.0], Z) * (1.0 + np.arange(Z)) / Z
    c[1, last] = np.nan
    c[2, last] = 0.0
    c[3, last] = 0.0
    c[3, last2] = -0.0
    return frozen(base, llr)[0], Z, max_iter, llr


@functools.lru_cache(maxsize=None)
def pack_want(name, early_stop):
    base, Z, max_iter, llr = pack_case(name)
    V = block_row_vars(np.asarray(base), Z, 0)
    d = V.shape[1]
    assert d == (base >= 0).sum(axis=1).max() == int(name[3:])
    c = llr[-4:]
    assert (np.abs(c[0][V]).argmin(axis=1) == d - 1).all()  # the minimum at the last position
    assert (np.isnan(c[1][V]).sum(axis=1) == 1).all() and np.isnan(c[1][V][:, d - 1]).all()
    assert ((c[2][V] == 0).sum(axis=1) == 1).all() and (c[2][V][:, d - 1] == 0).all()
    assert ((c[3][V] == 0).sum(axis=1) == 2).all() and (c[3][V][:, d - 2:] == 0).all()
    want = qc_layered_ms_ref(base, Z, llr, max_iter, NORM, early_stop, dtype=np.float64)
    if not early_stop:
        assert np.isnan(want[2][-3]).any()  # the NaN frame has NaN posteriors
    return frozen(*want)


# ---- d. irregular layers ---------------------------------------------------------------
IRR_N, IRR_ITER = 640, 8
_IRR_HEAD = [[65, 2, 33, 17, 16, 32, 64, 0, 3, 40] + [6] * 30, [], [], [255, 5, 9]]
_IRR_TAIL = [[12], [31, 34, 63, 66, 96, 97, 2, 2]]
IRR_LAYERS = {
    "block": _IRR_HEAD + [[7] * 70] + _IRR_TAIL,   # largest layer 70: two wavefronts, a barrier per layer
    "wave": _IRR_HEAD + [[7] * 60] + _IRR_TAIL,    # largest layer 60: one wavefront, the mixed degrees side by side
}
IRREGULAR = {
    "block": _g(0, 0, 1, 128, 9, 11472, 11600),    # m = 122: 5120 + 1952 + 4392 = 11464
    "wave": _g(1, 0, 4, 256, 9, 10944, 43776),     # m = 112: 5120 + 1792 + 4032
}


def irregular(n, layer_degrees, seed):
    """(H, layers): each layer is a fresh random permutation of the n columns, cut into rows of the listed
    degrees, so a layer's rows are disjoint by construction.  Rows are numbered in the order listed."""
    rng = np.random.RandomState(seed)
    m = sum(len(d) for d in layer_degrees)
    H = np.zeros((m, n), dtype=int)
    layers, c = [], 0
    for degs in layer_degrees:
        assert sum(degs) <= n
        perm, at = rng.permutation(n), 0
        layers.append(np.arange(c, c + len(degs), dtype=np.int64))
        for d in degs:
            H[c, perm[at:at + d]] = 1
            at, c = at + d, c + 1
    return H, layers


@functools.lru_cache(maxsize=None)
def irregular_case(name):
    """(H, layers, llr): five frames at 6 dB, four at 1 dB, and two more with +-0, +-inf, NaN and the
    extremes of the format put in at random places (test_gpu_ldpc_layered.py's test_special_values)."""
    H, layers = irregular(IRR_N, IRR_LAYERS[name], seed=640)
    deg = H.sum(axis=1)
    assert [len(l) for l in layers].count(0) == 2 and 1 in [len(l) for l in layers]
    assert deg.min() == 0 and deg.max() == 255 and not (deg == 1).any()
    first = deg[layers[0]]  # neighbouring lanes on both sides of 16, 32 and 64
    assert {16, 17, 32, 33, 64, 65} <= set(first.tolist())
    llr = np.concatenate([awgn(IRR_N, 5, 6.0, seed=641), awgn(IRR_N, 4, 1.0, seed=642), awgn(IRR_N, 2, 6.0, seed=643)])
    rng = np.random.RandomState(644)
    llr[9, rng.choice(IRR_N, 6, replace=False)] = [0.0, -0.0, np.inf, -np.inf, np.nan, 5e-324]
    llr[10, rng.choice(IRR_N, 6, replace=False)] = [np.nan, 1e300, -1e300, np.inf, 0.0, -0.0]
    return frozen(H, llr)[0], layers, llr


@functools.lru_cache(maxsize=None)
def irregular_want(name, early_stop):
    H, layers, llr = irregular_case(name)
    want = layered_ms_ref(H, llr, layers, IRR_ITER, NORM, early_stop)
    if early_stop:
        print(name, "restatement iterations:", want[1])
        assert (want[1][:5] <= 2).all() and (want[1][5:9] == IRR_ITER).all()
    assert np.isnan(want[2][9:]).any()
    return frozen(*want)


# ---- e. posteriors across chunks -------------------------------------------------------
# lms_decode_impl (capi.cpp) serves all four layered decoders.  13 frames with PL_LDPC_CHUNK=5: chunks of 5, 5
# and 3.  name: (decoder, environment besides the chunk); the first five are on the workspace by PL_LMS_GLOBAL
CHUNK, CHUNK_FRAMES = 5, 13
CHUNKED = {
    "lms_r504": dict(wave=1, use_global=1, reserved=10),   # LayeredMSDecoder, one wavefront per frame
    "lms_z1025": dict(wave=0, use_global=1, reserved=10),  # LayeredMSDecoder, one workgroup per frame (a. at Z = 1025)
    "qc_f64": dict(reserved=12),               # QCLayeredMSDecoder at Z = 27
    "qc_f32": dict(reserved=14),               # ... dtype=np.float32
    "qc_i8": dict(reserved=16),                # QCFixedMSDecoder at Z = 27
}
CHUNK_LADDER = (311, 2, 5)  # b.'s 311-column plan on the workspace by the planner's choice: chunks of 2, 2 and 1


def _chunk_llr(n, snr_hi, snr_lo, seed):
    """The first chunk at snr_hi (every frame stops early, on the codeword sent), the others at snr_lo (none
    stops): frame k of a later chunk differs from frame k of the first in bits, count and posterior."""
    return np.concatenate([awgn(n, CHUNK, snr_hi, seed=seed), awgn(n, CHUNK_FRAMES - CHUNK, snr_lo, seed=seed + 1)])


def chunks_differ(want, max_iter, chunk=CHUNK):
    bits, its, post = want
    assert (its[:chunk] < max_iter).all() and not bits[:chunk].any()
    assert (its[chunk:] == max_iter).all() and bits[chunk:].any(axis=1).all()
    for k in range(chunk, len(its)):
        assert not np.array_equal(post[k], post[k % chunk], equal_nan=True)


@functools.lru_cache(maxsize=None)
def chunk_case(name):
    """(make: () -> decoder, llr as the decoder's device input, want)."""
    Lib = L()
    if name == "lms_r504":
        H = Lib.regular_construction(504, 3, 6, seed=3)
        layers = Lib.layer_schedule(H)
        assert max(len(l) for l in layers) <= 64
        llr = _chunk_llr(504, 2.0, -3.0, seed=700)
        want = layered_ms_ref(H, llr, layers, 10, NORM, True)
        make = lambda: Lib.LayeredMSDecoder(H, max_iter=10, normalization=NORM, layers=layers)  # noqa: E731
        it = 10
    elif name == "lms_z1025":
        Z, base = 1025, width_base(1025)
        llr = _chunk_llr(4 * Z, 3.0, -3.0, seed=710)
        want = qc_layered_ms_ref(base, Z, llr, 6, NORM, True, dtype=np.float64)
        make = lambda: Lib.LayeredMSDecoder(Lib.qc_expand(base, Z), max_iter=6, normalization=NORM,  # noqa: E731
                                            layers=Lib.qc_block_layers(2, Z))
        it = 6
    else:
        Z, it = 27, 10
        base = frozen(Lib.qc_random_base(4, 8, Z, 3, seed=727))
        llr = _chunk_llr(8 * Z, 2.0, -5.0, seed=720)
        if name == "qc_i8":
            from qc_fixed_ref import qc_fixed_ms_ref, quantize_ref
            llr = quantize_ref(llr, 4.0, 31)
            want = qc_fixed_ms_ref(base, Z, llr, it, 12, 31, 31, True)[:3]
            make = lambda: Lib.QCFixedMSDecoder(np.array(base), Z, max_iter=it, normalization=NORM)  # noqa: E731
        else:
            dtype = {"qc_f64": np.float64, "qc_f32": np.float32}[name]
            llr = llr.astype(dtype)
            want = qc_layered_ms_ref(base, Z, llr, it, NORM, True, dtype=dtype)
            make = lambda: Lib.QCLayeredMSDecoder(np.array(base), Z, max_iter=it, normalization=NORM,  # noqa: E731
                                                  dtype=dtype)
    print(name, "restatement iterations:", want[1])
    chunks_differ(want, it)
    return make, frozen(llr), frozen(*want)


@functools.lru_cache(maxsize=None)
def chunk_ladder_case():
    """Frames 0, 2 (they stop early) | 1, 3 | 5 (they do not) of b.'s frames at nb = 311."""
    nb, chunk, frames = CHUNK_LADDER
    order = [0, 2, 1, 3, 5]
    assert len(order) == frames
    llr = np.array(ladder_llr(nb)[order])
    want = tuple(np.array(w[order]) for w in ladder_want(nb, True))
    assert (want[1][:chunk] < LADDER_ITER).all() and (want[1][chunk:] == LADDER_ITER).all()
    for k in range(chunk, frames):
        assert not np.array_equal(want[0][k], want[0][k % chunk]) and not np.array_equal(want[2][k], want[2][k % chunk])
    return frozen(llr), frozen(*want)


# ---- f. what the tables reach ----------------------------------------------------------
def all_geometries():
    """name -> geometry row of every case of a. to d. (e. adds the decoders, not geometries)."""
    g = {}
    g.update({"width_%d" % z: v for z, v in WIDTHS.items()})
    g.update({"width_%d_global" % z: v for z, v in WIDTH_GLOBAL.items()})
    g.update({"ladder_%d" % nb: v for nb, v in LADDER.items()})
    g.update({"edge_%d" % z: v for z, v in BLOCK_EDGE.items()})
    g.update({"pack_" + k: v for k, v in PACKS.items()})
    g.update({"irregular_" + k: v for k, v in IRREGULAR.items()})
    return g

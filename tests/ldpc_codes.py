"""The LDPC codes, the plan each must get and the channel inputs shared by
tests/test_ldpc_codes_host.py (planner, no GPU) and tests/test_gpu_ldpc_kernels.py
(the kernels against the oracle).  A plain module: no fixtures, every builder
deterministic and cached."""
import functools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

BP, MS = 0, 1
DEFAULT, GENERIC, REG, COMPACT = 0, 1, 2, 3  # PL_LDPC_KERNEL_* of include/polarldpc.h
OVERRIDE_ENV = {DEFAULT: None, GENERIC: "generic", REG: "reg", COMPACT: "compact"}  # PL_LDPC_KERNEL


def _L():
    import polarcode_and_ldpc_amd.ldpc as L
    return L


# ---- builders ----

def irregular(H):
    """Clear a fixed handful of entries (the first one of a few rows): variable
    degrees differ, every row keeps degree >= 2."""
    H = H.copy()
    for r in (0, 5, 11, 17, 23):
        H[r, np.flatnonzero(H[r])[0]] = 0
    assert H.sum(axis=1).min() >= 2
    return H


def moved(H, r0=0, k=10):
    """For the first k columns that row r0 lacks, move one entry of the column
    from a donor row into r0, each donor row used once: column weights stay,
    row r0 gains degree k, the donors lose one."""
    H = H.copy()
    used = {r0}
    cols = np.flatnonzero(H[r0] == 0)[:k]
    assert len(cols) == k
    for c in cols:
        donor = next(r for r in np.flatnonzero(H[:, c]) if r not in used)
        used.add(donor)
        H[donor, c] = 0
        H[r0, c] = 1
    return H


def blockdiag(A, B):
    H = np.zeros((A.shape[0] + B.shape[0], A.shape[1] + B.shape[1]), dtype=A.dtype)
    H[:A.shape[0], :A.shape[1]] = A
    H[A.shape[0]:, A.shape[1]:] = B
    return H


def colweights(m, ws, seed):
    """m x len(ws): column c has ws[c] ones in rows drawn without replacement,
    column by column from one RandomState(seed)."""
    rs = np.random.RandomState(seed)
    H = np.zeros((m, len(ws)), dtype=int)
    for c, w in enumerate(ws):
        H[rs.choice(m, w, replace=False), c] = 1
    return H


@functools.lru_cache(maxsize=None)
def R(n, dv, dc, seed):
    """regular_construction(n, dv, dc, seed).  The (3,15) code of diag_deg15 is
    read from tests/golden instead: regular_construction redraws until no edge
    repeats, about a million draws (a minute) at n = 1280, dc = 15.  The
    fixture holds that matrix, per column its rows."""
    if (n, dv, dc, seed) == (1280, 3, 15, 1283):
        rows = np.load(os.path.join(GOLDEN, "ldpc_regular_1280_3_15_seed1283.npz"))["rows"].astype(int)
        H = np.zeros((n * dv // dc, n), dtype=int)
        H[rows.ravel(), np.repeat(np.arange(n), dv)] = 1
    else:
        H = _L().regular_construction(n, dv, dc, seed=seed)
    H.setflags(write=False)
    return H


WIDECOLS_WS = [2, 3, 7, 8, 9, 15, 16, 17, 23, 24, 25, 31, 32, 33, 64, 127, 128] * 4

_BUILD = {
    "irr96": lambda: irregular(R(96, 3, 6, 99)),
    "widecols": lambda: colweights(160, WIDECOLS_WS, 5),
    "irr2048": lambda: irregular(R(2048, 3, 6, 2051)),
    "moved504": lambda: moved(R(504, 3, 6, 507)),
    "moved2048": lambda: moved(R(2048, 3, 6, 2051)),
    "r1000_36": lambda: R(1000, 3, 6, 1003),
    "r480_48": lambda: R(480, 4, 8, 8),
    "r720_48": lambda: R(720, 4, 8, 724),
    "r504_36": lambda: R(504, 3, 6, 507),
    "r1000_48": lambda: R(1000, 4, 8, 21),
    "r1500_36": lambda: R(1500, 3, 6, 1503),
    "diag_deg15": lambda: blockdiag(R(1024, 3, 6, 1027), R(1280, 3, 15, 1283)),
    "r8194_36": lambda: R(8194, 3, 6, 8197),
    "r2048_36": lambda: R(2048, 3, 6, 2051),  # the (3,6)-regular min-sum kernel's code of the pitch test
}


@functools.lru_cache(maxsize=None)
def code(cid):
    """(H, row_ptr, col_idx) of a code id; the arrays are shared: read only."""
    H = np.array(_BUILD[cid]())
    rp, ci = _L().dense_to_csr(H)
    for a in (H, rp, ci):
        a.setflags(write=False)
    return H, rp, ci


# id: (n, m, row-degree set, column-degree set)
SHAPES = {
    "irr96": (96, 48, {5, 6}, {2, 3}),
    "widecols": (68, 160, None, set(WIDECOLS_WS)),  # row degrees: 6..22, see WIDECOLS_ROWDEG
    "irr2048": (2048, 1024, {5, 6}, {2, 3}),
    "moved504": (504, 252, {5, 6, 16}, {3}),
    "moved2048": (2048, 1024, {5, 6, 16}, {3}),
    "r1000_36": (1000, 500, {6}, {3}),
    "r480_48": (480, 240, {8}, {4}),
    "r720_48": (720, 360, {8}, {4}),
    "r504_36": (504, 252, {6}, {3}),
    "r1000_48": (1000, 500, {8}, {4}),
    "r1500_36": (1500, 750, {6}, {3}),
    "diag_deg15": (2304, 768, {6, 15}, {3}),
    "r8194_36": (8194, 4097, {6}, {3}),
    "r2048_36": (2048, 1024, {6}, {3}),
}
WIDECOLS_ROWDEG = (6, 22)  # smallest and largest row degree of widecols


def _p(kernel, **kw):
    d = {"kernel": kernel, "use_global": 0, "threads": 256, "reg_variant": 0, "compact": 0, "ms36": 0}
    d.update(kw)
    return d


_GEN_LDS = _p(1)
_GEN_GLOBAL = _p(1, use_global=1, threads=1024)
_COMPACT = _p(5, threads=1024, compact=1)


def _reg(v):
    return _p(2, reg_variant=v)


def _grp(v):
    return _p(7, reg_variant=v)


# (code id, algo, PL_LDPC_KERNEL override): what the planner must decide.  kernel: pl_plan_info.reserved
# (1 generic, 2 register-cached, 5 compact min-sum, 7 degree-grouped BP, 8 (3,6)-regular min-sum);
# threads: the generic kernel runs 256 threads up to E = 4096 edges, 1024 above; the register-cached and
# grouped kernels 256; the compact one 1024.  "lds": the dynamic LDS size where the case pins it.
PLANS = {
    ("irr96", BP, DEFAULT): _GEN_LDS,
    ("irr96", MS, DEFAULT): _GEN_LDS,
    ("widecols", BP, DEFAULT): _GEN_LDS,
    ("widecols", MS, DEFAULT): _GEN_LDS,
    ("irr2048", BP, DEFAULT): _GEN_GLOBAL,
    ("irr2048", MS, DEFAULT): _COMPACT,
    ("irr2048", MS, GENERIC): _GEN_GLOBAL,
    ("moved504", BP, DEFAULT): _reg(1),  # a check of degree 16: no grouped kernel
    ("moved504", MS, DEFAULT): _reg(1),
    ("moved2048", BP, DEFAULT): _GEN_GLOBAL,
    ("moved2048", MS, DEFAULT): _GEN_GLOBAL,  # a check of degree 16: no compact kernel
    ("r1000_36", BP, DEFAULT): _grp(2),
    ("r1000_36", MS, DEFAULT): _reg(2),
    ("r1000_36", BP, REG): _reg(2),
    ("r480_48", BP, DEFAULT): _grp(3),
    ("r480_48", MS, DEFAULT): _reg(3),
    ("r480_48", BP, REG): _reg(3),
    ("r720_48", BP, DEFAULT): _grp(4),
    ("r720_48", MS, DEFAULT): _reg(4),
    ("r720_48", BP, REG): _reg(4),
    ("r504_36", BP, DEFAULT): _grp(1),
    ("r504_36", MS, DEFAULT): _reg(1),
    ("r504_36", BP, REG): _reg(1),
    ("r1000_48", BP, DEFAULT): _p(1, use_global=1, threads=256),  # E = 4000
    ("r1000_48", MS, DEFAULT): _COMPACT,
    ("r1500_36", BP, DEFAULT): _GEN_GLOBAL,
    ("r1500_36", MS, DEFAULT): _COMPACT,
    ("diag_deg15", BP, DEFAULT): _GEN_GLOBAL,
    ("diag_deg15", MS, DEFAULT): _COMPACT,
    ("r8194_36", MS, DEFAULT): dict(_COMPACT, lds=147632),
    ("r2048_36", MS, DEFAULT): _p(8, threads=1024, compact=1, ms36=2),
}

# (code id, normalization) -> ldpc_ms_compact_kernel<VPT, DV, DC[, PRE]> instance the compact plan launches
COMPACT_INSTANCE = {
    ("irr2048", 1.0): "8,0,0", ("irr2048", 0.75): "8,0,0", ("irr2048", 1.25): "8,0,0", ("irr2048", 0.0): "8,0,0",
    ("irr2048", -0.5): "8,0,0",
    ("r1000_48", 1.0): "8,0,0", ("r1000_48", 0.75): "8,0,0",
    ("r1500_36", 1.0): "8,3,6,PRE", ("r1500_36", 0.75): "8,3,6,PRE", ("r1500_36", 0.0): "8,3,6,PRE",
    ("r1500_36", -0.5): "8,3,6,PRE", ("r1500_36", 1.25): "8,3,6",
    ("diag_deg15", 1.0): "8,0,0", ("diag_deg15", 0.75): "8,0,0", ("diag_deg15", 1.25): "8,0,0",
    ("r8194_36", 1.0): "0,0,0", ("r8194_36", 0.75): "0,0,0", ("r8194_36", 1.25): "0,0,0",
}


def compact_instance(cid, norm):
    """pick_kernel's choice among the compact min-sum instances (ldpc.hip), restated."""
    H = code(cid)[0]
    n = H.shape[1]
    dvs, dcs = set(H.sum(axis=0).tolist()), set(H.sum(axis=1).tolist())
    regular = len(dvs) == 1 and len(dcs) == 1
    if n <= 8192 and regular and (max(dvs), max(dcs)) == (3, 6):
        return "8,3,6,PRE" if abs(norm) <= 1 else "8,3,6"
    return "8,0,0" if n <= 8192 else "0,0,0"


# ---- channel inputs ----

MAX_ITER = 50

# Es/N0 range (dB) of the all-zero-codeword AWGN frames, below each code's waterfall: the oracle runs at
# least half the frames of every case to MAX_ITER (asserted by the GPU test on the oracle's output)
SNR_DB = {
    "irr96": (-6.0, 0.0),
    "widecols": (-6.0, 0.0),
    "irr2048": (-4.0, -1.5),
    "moved504": (-5.0, -1.0),
    "moved2048": (-4.0, -1.5),
    "r1000_36": (-4.5, -1.5),
    "r480_48": (-5.0, -1.0),
    "r720_48": (-5.0, -1.0),
    "r504_36": (-5.0, -1.0),
    "r1000_48": (-4.5, -1.5),
    "r1500_36": (-3.0, -0.5),
    "diag_deg15": (-1.0, 2.5),
    "r8194_36": (-3.0, -1.0),
    "r2048_36": (-4.0, -1.5),
}


def batch_size(n):
    return 256 if n <= 1000 else (24 if n <= 4096 else 8)


@functools.lru_cache(maxsize=None)
def awgn_llrs(cid):
    """Noisy all-zero-codeword LLRs [batch_size(n), n], one Es/N0 per frame
    uniform in SNR_DB[cid], from RandomState(1)."""
    n = SHAPES[cid][0]
    B = batch_size(n)
    rng = np.random.RandomState(1)
    snr = rng.uniform(*SNR_DB[cid], size=(B, 1))
    sigma = np.sqrt(1.0 / (2.0 * 10 ** (snr / 10.0)))
    llr = 2.0 * (1.0 + sigma * rng.randn(B, n)) / sigma ** 2
    llr.setflags(write=False)
    return llr


def special_llrs(rng, B, n):
    """Noisy all-zero-codeword LLRs with the special values of min-sum's check
    statistics: exact zeros (one or many per check), -0, +-inf, NaN (one, a few)."""
    snr = rng.uniform(0.5, 2.5, size=(B, 1))
    sigma = np.sqrt(1.0 / (2.0 * 10 ** (snr / 10.0)))
    llr = 2.0 * (1.0 + sigma * rng.randn(B, n)) / sigma ** 2
    llr[1, ::5] = 0.0
    llr[2, ::97] = -0.0
    llr[3, 7] = np.nan
    llr[4, 11], llr[4, 12] = np.inf, -np.inf
    llr[5, :3] = np.nan
    llr[6, rng.rand(n) < 0.3] = 0.0          # erasures: checks with 1, 2 or more zeros
    llr[7, rng.rand(n) < 0.02] = np.nan      # scattered NaN
    llr[8, rng.rand(n) < 0.1] = np.inf
    llr[8, rng.rand(n) < 0.1] = -np.inf
    llr[9, :] = np.where(rng.rand(n) < 0.5, 0.0, -0.0)
    return llr


@functools.lru_cache(maxsize=None)
def special_inputs(cid):
    n = SHAPES[cid][0]
    llr = special_llrs(np.random.RandomState(n), 12, n)
    llr.setflags(write=False)
    return llr

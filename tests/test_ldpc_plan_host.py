"""The host-side LDPC planner (csrc/ldpc_plan.cpp) through its device-free
window, pl_debug_ldpc_plan_probe / pl_debug_ldpc_layered_plan_probe (no GPU):
for one code per kernel-selection branch, the chosen kernel, its geometry and
the FNV-1a digest of the table buffer equal the values recorded from the
library as it was before the planner was split out of the C-ABI
(tests/golden/ldpc_plan_digests.json).  Each case names the kernel code of the
branch it is there for, so a case that drifts to another branch fails too."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN
from ldpc_codes import irregular as _irregular

BP, MS = 0, 1
DEFAULT, GENERIC, REG, COMPACT = 0, 1, 2, 3  # PL_LDPC_KERNEL_* of include/polarldpc.h


def _L():
    import polarcode_and_ldpc_amd.ldpc as L
    return L


# regular_construction draws until no edge repeats, which takes thousands of draws at (4,8):
# seeds whose draw ends within a second or two
SEEDS = {(480, 4, 8): 8, (1000, 4, 8): 21}


@functools.lru_cache(maxsize=None)
def _code(kind, n, dv, dc):
    L = _L()
    if kind == "mackay":  # tests/test_gpu_ldpc.py test_bp_grouped_variants_vs_oracle: check degrees up to 15
        return L.mackay_construction(n, n // 2, dv, dc, seed=n + dv)
    H = L.regular_construction(n, dv, dc, seed=SEEDS.get((n, dv, dc), n + dv))
    if kind == "irregular":
        return _irregular(H)
    if kind == "wide_row":  # row 0 widened to degree >= 18
        H = H.copy()
        H[0, :18] = 1
    return H


# id: (kernel code, code kind, n, dv, dc, algo, PL_LDPC_KERNEL override, PL_BP_FPG (0: unset))
FLOODING = {
    # 1: generic kernel, state in LDS
    "generic_lds_bp": (1, "irregular", 96, 3, 6, BP, DEFAULT, 0),
    "generic_lds_ms": (1, "irregular", 96, 3, 6, MS, DEFAULT, 0),
    "generic_lds_regular_override": (1, "regular", 96, 3, 6, BP, GENERIC, 0),
    # 1: generic kernel, T / C in the global workspace (2 E 8 > 64 KB)
    "generic_global_bp": (1, "irregular", 2048, 3, 6, BP, DEFAULT, 0),
    "generic_global_ms_override": (1, "irregular", 2048, 3, 6, MS, GENERIC, 0),
    # 2: register-cached kernel
    "reg_ms_504": (2, "regular", 504, 3, 6, MS, DEFAULT, 0),
    "reg_bp_504_override": (2, "regular", 504, 3, 6, BP, REG, 0),
    "reg_ms_480_v3": (2, "regular", 480, 4, 8, MS, DEFAULT, 0),
    # 7: degree-grouped BP, variants 1..4
    "grp_504_fpg_default": (7, "regular", 504, 3, 6, BP, DEFAULT, 0),
    "grp_504_fpg1": (7, "regular", 504, 3, 6, BP, DEFAULT, 1),
    "grp_1000_v2": (7, "regular", 1000, 3, 6, BP, DEFAULT, 0),
    "grp_480_v3": (7, "regular", 480, 4, 8, BP, DEFAULT, 0),
    # variant 4 at n = 720: a (4,8) code of n = 1000 has 2 E 8 > 64 KB and leaves the LDS-resident kernels
    "grp_720_v4": (7, "regular", 720, 4, 8, BP, DEFAULT, 0),
    "grp_mackay_600_deg15": (7, "mackay", 600, 3, 6, BP, DEFAULT, 0),
    # 5: compact min-sum
    "compact_irregular_2048": (5, "irregular", 2048, 3, 6, MS, DEFAULT, 0),
    "compact_2048_override": (5, "regular", 2048, 3, 6, MS, COMPACT, 0),
    # (4,8) at n = 1000, the smallest round n whose T / C exceed LDS: drawing an n = 4096 (4,8) code
    # with regular_construction takes minutes on a CPU
    "compact_1000_48": (5, "regular", 1000, 4, 8, MS, DEFAULT, 0),
    # the VPT = 0 instance: n > 8192 whose 8 n + 20 m + 128 bytes still fit 160 KB.  A (3,6) code of
    # n = 10240 needs 184 448 and does not (it gets the generic kernel); n = 9000 fits
    "compact_9000_vpt0": (5, "regular", 9000, 3, 6, MS, DEFAULT, 0),
    # 8: (3,6)-regular min-sum
    "ms36_2048": (8, "regular", 2048, 3, 6, MS, DEFAULT, 0),
    "ms36_4096": (8, "regular", 4096, 3, 6, MS, DEFAULT, 0),
    "ms36_8192": (8, "regular", 8192, 3, 6, MS, DEFAULT, 0),
}
FLOODING_FIELDS = ("kernel", "threads", "lds_bytes", "use_global", "reg_variant", "grp", "fpg", "tl", "npad", "compact",
                   "ms36", "work_bytes", "table_len", "grp_at", "vw_at")

# id: (code kind, n, dv, dc, what the case is there for); layers: layer_schedule's first fit
LAYERED = {
    "wave_96": ("regular", 96, 3, 6, {"wave": 1, "mw": 1}),      # every layer <= 64 checks
    "block_1000": ("regular", 1000, 3, 6, {"wave": 0, "mw": 1}),  # a layer of more than 64 checks
    "deg18_96": ("wide_row", 96, 3, 6, {"mw": 2}),               # a row of degree >= 18: a second meta word
}
LAYERED_FIELDS = ("kernel", "maxdc", "n_layers", "max_layer", "mw", "wave", "use_global", "fpb", "threads", "lds_bytes",
                  "state_bytes", "off_mm", "off_meta", "table_len")


def flooding_args(case):
    _, kind, n, dv, dc, algo, override, fpg = FLOODING[case]
    rp, ci = _L().dense_to_csr(_code(kind, n, dv, dc))
    return rp, ci, n, algo, override, fpg


def layered_args(case):
    kind, n, dv, dc, _ = LAYERED[case]
    L = _L()
    H = _code(kind, n, dv, dc)
    rp, ci = L.dense_to_csr(H)
    layers = L.layer_schedule(H)
    lp = np.zeros(len(layers) + 1, np.int32)
    lp[1:] = np.cumsum([len(l) for l in layers])
    return rp, ci, n, lp, np.ascontiguousarray(np.concatenate(layers), np.int32)


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(GOLDEN, "ldpc_plan_digests.json")) as f:
        return json.load(f)


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


@pytest.mark.parametrize("case", sorted(FLOODING))
def test_flooding_plan_equals_recorded(case, recorded):
    from polarcode_and_ldpc_amd import _native
    rp, ci, n, algo, override, fpg = flooding_args(case)
    out = _native.LdpcPlanProbe()
    rc = _native.lib.pl_debug_ldpc_plan_probe(len(rp) - 1, n, _ptr(rp), _ptr(ci), algo, 20, 1, 0.75, override, fpg, 0,
                                              ctypes.byref(out))
    assert rc == 0, _native.lib.pl_last_error()
    got = {"kernel": out.kernel, "threads": out.threads, "lds_bytes": out.lds_bytes, "use_global": out.use_global,
           "reg_variant": out.reg_variant, "grp": out.grp, "fpg": out.fpg, "tl": out.tl, "npad": out.npad,
           "compact": out.compact, "ms36": out.ms36, "work_bytes": out.work_bytes_per_frame,
           "table_len": out.table_len, "grp_at": out.grp_at, "vw_at": out.ms_vw_at, "digest": "%016x" % out.digest}
    assert got["kernel"] == FLOODING[case][0], got
    want = recorded["flooding"][case]
    assert set(want) == set(FLOODING_FIELDS) | {"digest"}
    assert got == want


def test_flooding_cases_reach_every_reg_variant_and_vpt0(recorded):
    r = recorded["flooding"]
    assert [r[c]["reg_variant"] for c in ("reg_ms_504", "reg_ms_480_v3")] == [1, 3]
    assert [r[c]["reg_variant"] for c in ("grp_504_fpg_default", "grp_1000_v2", "grp_480_v3", "grp_720_v4")] == [1, 2, 3, 4]
    assert r["grp_mackay_600_deg15"]["npad"] > 0  # mixed check degrees: padded T' positions
    assert (r["grp_504_fpg_default"]["fpg"], r["grp_504_fpg1"]["fpg"], r["grp_1000_v2"]["fpg"]) == (2, 1, 1)
    assert r["generic_global_bp"]["use_global"] == 1 and r["generic_global_bp"]["work_bytes"] > 0
    assert r["generic_lds_bp"]["use_global"] == 0
    assert [r[c]["ms36"] for c in ("ms36_2048", "ms36_4096", "ms36_8192")] == [2, 4, 8]


@pytest.mark.parametrize("force_global", [0, 1])
@pytest.mark.parametrize("case", sorted(LAYERED))
def test_layered_plan_equals_recorded(case, force_global, recorded):
    from polarcode_and_ldpc_amd import _native
    rp, ci, n, lp, lr = layered_args(case)
    out = _native.LdpcLayeredPlanProbe()
    rc = _native.lib.pl_debug_ldpc_layered_plan_probe(len(rp) - 1, n, _ptr(rp), _ptr(ci), len(lp) - 1, _ptr(lp),
                                                      _ptr(lr), 20, 1, 0.75, 0, 0, force_global, ctypes.byref(out))
    assert rc == 0, _native.lib.pl_last_error()
    got = {f: getattr(out, f) for f in LAYERED_FIELDS}
    got["digest"] = "%016x" % out.digest
    assert got["kernel"] == (10 if force_global else 9)
    for k, v in LAYERED[case][4].items():
        assert got[k] == v, (k, got)
    assert got == recorded["layered"]["%s_global%d" % (case, force_global)]


def test_probe_refuses_what_the_creators_refuse():
    """Same checks, codes and messages as the plan creators; row_ptr is proven
    monotone and within [0, E] before col_idx is read."""
    from polarcode_and_ldpc_amd import _native
    lib = _native.lib
    ci = np.arange(6, dtype=np.int32)
    out = _native.LdpcPlanProbe()
    lout = _native.LdpcLayeredPlanProbe()
    lp, lr = np.array([0, 1, 2], np.int32), np.array([0, 1], np.int32)
    for bad in ([0, 7, 6], [0, 1000, 6]):
        rp = np.array(bad, np.int32)
        rc = lib.pl_debug_ldpc_plan_probe(2, 8, _ptr(rp), _ptr(ci), BP, 20, 1, 1.0, 0, 0, 0, ctypes.byref(out))
        assert rc == _native.PL_EINVAL and b"monotone" in lib.pl_last_error()
        rc = lib.pl_debug_ldpc_layered_plan_probe(2, 8, _ptr(rp), _ptr(ci), 2, _ptr(lp), _ptr(lr), 20, 1, 1.0, 0, 0, 0,
                                                  ctypes.byref(lout))
        assert rc == _native.PL_EINVAL and b"monotone" in lib.pl_last_error()
    rp = np.array([0, 1, 6], np.int32)  # a degree-1 check: min-sum only
    assert lib.pl_debug_ldpc_plan_probe(2, 8, _ptr(rp), _ptr(ci), MS, 20, 1, 1.0, 0, 0, 0,
                                        ctypes.byref(out)) == _native.PL_EUNSUPPORTED
    assert b"degree-1" in lib.pl_last_error()
    assert lib.pl_debug_ldpc_plan_probe(2, 8, _ptr(rp), _ptr(ci), BP, 20, 1, 1.0, 0, 0, 0, ctypes.byref(out)) == 0
    assert lib.pl_debug_ldpc_plan_probe(2, 8, _ptr(rp), _ptr(ci), BP, 0, 1, 1.0, 0, 0, 0,
                                        ctypes.byref(out)) == _native.PL_EINVAL
    assert lib.pl_debug_ldpc_plan_probe(2, 8, _ptr(rp), _ptr(ci), 7, 20, 1, 1.0, 0, 0, 0,
                                        ctypes.byref(out)) == _native.PL_EINVAL

"""The fixed-point quasi-cyclic planner on the CPU: the state layout and the
mapping through pl_debug_ldpc_qc_fixed_plan_probe against the layout the header
documents, the LDS / workspace boundary, PL_LMS_GLOBAL, every refusal and their
order; then the same builder as a stand-alone program under AddressSanitizer +
UBSan (tests/asan/qc_fixed_plan_check.cpp with csrc/ldpc_plan.cpp alone: no HIP,
no library, no preload).  QCFixedMSDecoder's constructor checks need no device."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "asan")
CLANGXX = os.environ.get("CLANGXX", "/opt/rocm/lib/llvm/bin/clang++")
LDS_MAX = 160 * 1024
VOTE = 128


def _N():
    from polarcode_and_ldpc_amd import _native
    return _native


def _L():
    import polarcode_and_ldpc_amd.ldpc as L
    return L


def probe(base, Z, max_iter=20, norm16=12, llr_max=31, msg_max=31, lms_global=0, layer_order=None):
    """(rc, probe, message)"""
    N = _N()
    sh = np.ascontiguousarray(base, np.int32)
    lo = None if layer_order is None else np.ascontiguousarray(layer_order, np.int32)
    out = N.LdpcQcFixedPlanProbe()
    rc = N.lib.pl_debug_ldpc_qc_fixed_plan_probe(sh.shape[0], sh.shape[1], Z, sh.ctypes.data_as(ctypes.c_void_p),
                                                 None if lo is None else lo.ctypes.data_as(ctypes.c_void_p), max_iter,
                                                 1, norm16, llr_max, msg_max, lms_global, ctypes.byref(out))
    return rc, out, N.lib.pl_last_error().decode()


def float_probe(base, Z, flags=0):
    N = _N()
    sh = np.ascontiguousarray(base, np.int32)
    out = N.LdpcQcPlanProbe()
    assert N.lib.pl_debug_ldpc_qc_plan_probe_flags(sh.shape[0], sh.shape[1], Z, sh.ctypes.data_as(ctypes.c_void_p),
                                                   None, 20, 1, 0.75, 0, flags, ctypes.byref(out)) == 0
    return out


def rows_base(degrees, nb, Z, seed=0):
    rng = np.random.RandomState(seed)
    base = np.full((len(degrees), nb), -1, dtype=np.int64)
    for i, d in enumerate(degrees):
        base[i, np.sort(rng.choice(nb, d, replace=False))] = rng.randint(0, Z, d)
    return base


def align16(b):
    return (b + 15) & ~15


@pytest.mark.parametrize("degrees,nb,Z", [([6, 6, 6, 6], 8, 1), ([6, 6, 6, 6], 8, 7), ([6, 5, 8, 2], 8, 27),
                                          ([6, 6, 6, 6], 8, 64), ([6, 6, 6, 6], 8, 96), ([12, 16, 9], 16, 7), ([12, 14, 9], 16, 7), ([15, 2], 16, 96),
                                          ([17, 32, 24], 48, 7), ([33, 2], 48, 96), ([40, 64, 65], 70, 7),
                                          ([6] * 46, 68, 384), ([3] * 16, 24, 1024)])
def test_layout_and_mapping(degrees, nb, Z):
    """Per frame [m][mw] u32 check words with mw = 1 for degrees <= 14 and 1 + ceil(maxdc / 32) above, then
    P[n] int8, rounded up to 16: n + 4 m, and n + 8 m up to degree 32; the mapping, the register cap and
    the stream are the floating plan's."""
    base = rows_base(degrees, nb, Z)
    rc, p, msg = probe(base, Z)
    assert rc == 0, msg
    mb, maxdc = len(degrees), max(degrees)
    m, n = mb * Z, nb * Z
    mw = 1 if maxdc <= 14 else 1 + (maxdc + 31) // 32
    assert (p.z, p.mb, p.nb, p.maxdc, p.mw) == (Z, mb, nb, maxdc, mw)
    assert (p.norm16, p.llr_max, p.msg_max) == (12, 31, 31)
    assert p.off_p == 4 * m * mw and p.state_bytes == align16(p.off_p + n)
    if maxdc <= 32:
        assert p.state_bytes == align16(n + (4 if maxdc <= 14 else 8) * m)
    assert p.dcap == (8 if maxdc <= 8 else 16 if maxdc <= 16 else 32 if maxdc <= 32 else 0)
    fpw = 64 // Z if Z <= 64 else 1
    assert p.fpw == fpw
    if Z <= 64:
        wave = p.state_bytes * fpw
        home = wave > LDS_MAX
        assert p.fpb == (4 if home else max(1, min(4, 65536 // wave))) and p.threads == 64 * p.fpb
        assert p.lds_bytes == (0 if home else wave * p.fpb)
    else:
        home = p.state_bytes + VOTE > LDS_MAX
        assert p.fpb == 1 and p.threads == (Z + 63) // 64 * 64
        assert p.lds_bytes == (0 if home else p.state_bytes) + VOTE
    assert p.use_global == int(home) and p.kernel == (16 if home else 15)
    fl, f32 = float_probe(base, Z), float_probe(base, Z, _N().PL_LDPC_QC_F32)
    assert (p.table_len, p.digest, p.dcap, p.fpw) == (fl.table_len, fl.digest, fl.dcap, fl.fpw)
    assert p.state_bytes < f32.state_bytes < fl.state_bytes
    # PL_LMS_GLOBAL=1: the workspace, whatever the size
    rc, g, msg = probe(base, Z, lms_global=1)
    assert rc == 0 and g.use_global == 1 and g.kernel == 16 and g.state_bytes == p.state_bytes
    assert g.lds_bytes == (0 if Z <= 64 else VOTE) and g.fpb == (4 if Z <= 64 else 1)


def test_the_46_68_384_code_is_lds_resident():
    """The fp32 decoder left (46, 68, 384) in the workspace (4 n + 12 m = 316 416 bytes).  Its rows have at
    most 9 blocks (one word a check up to 14), so in int8 it is n + 4 m = 96 768 bytes and in LDS (with two words a check, n + 8 m =
    167 424, it would have missed the 160 KB by 3 584 bytes); n = 8 192 is 24 576 bytes against fp32's 81 920."""
    base = _L().qc_random_base(46, 68, 384, 3, seed=1)
    assert (base >= 0).sum(axis=1).max() == 9
    rc, p, msg = probe(base, 384)
    assert rc == 0, msg
    assert p.state_bytes == 68 * 384 + 4 * 46 * 384 == 96768 and p.use_global == 0 and p.kernel == 15
    assert float_probe(base, 384, _N().PL_LDPC_QC_F32).use_global == 1
    rc, p, msg = probe(_L().qc_random_base(32, 64, 128, 3, seed=1), 128)
    assert rc == 0 and p.state_bytes == 8192 + 4 * 4096 and p.lds_bytes == 24576 + VOTE and p.use_global == 0


@pytest.mark.parametrize("Z", [64, 96])
def test_lds_boundary(Z):
    """The largest state that stays in LDS and the next one, for one frame per wavefront (Z = 64:
    64 fpw = 1 state bytes against 160 KB) and one per workgroup (Z = 96: the vote words count)."""
    # degree-2 rows: mw = 1, state = align16(nb Z + 4 mb Z); nb = mb + 1 block columns keep it simple
    def state(mb):
        return align16((mb + 1) * Z + 4 * mb * Z)
    limit = LDS_MAX - (0 if Z <= 64 else VOTE)
    mb = max(k for k in range(2, 800) if state(k) <= limit)
    for k, home in ((mb, 0), (mb + 1, 1)):
        base = np.full((k, k + 1), -1, dtype=np.int64)
        base[np.arange(k), np.arange(k)] = 0
        base[np.arange(k), np.arange(k) + 1] = 1
        rc, p, msg = probe(base, Z)
        assert rc == 0, msg
        assert p.state_bytes == state(k) and p.use_global == home and p.kernel == 15 + home, (k, p.state_bytes)
        assert (p.state_bytes <= limit) == (home == 0)


def test_refusals_and_their_order():
    N = _N()
    base = rows_base([6, 6, 6, 6], 8, 7)

    def refused(code, word, b=base, Z=7, **kw):
        rc, _, msg = probe(b, Z, **kw)
        assert rc == code and word in msg, (rc, msg)

    for bad in (0, 17, -1, 2 ** 31 - 1):
        refused(N.PL_EINVAL, "norm16", norm16=bad)
    for bad in (0, 128, -1, -128):
        refused(N.PL_EINVAL, "llr_max", llr_max=bad)
        refused(N.PL_EINVAL, "msg_max", msg_max=bad)
    for lo, hi in ((1, 1), (16, 127)):
        assert probe(base, 7, norm16=lo, llr_max=hi, msg_max=hi)[0] == 0
    # the first one violated is named
    refused(N.PL_EINVAL, "norm16", norm16=0, llr_max=0, msg_max=0)
    refused(N.PL_EINVAL, "llr_max", llr_max=0, msg_max=0)
    # pl_ldpc_qc_plan_create's checks come first, in its order ...
    refused(N.PL_EINVAL, "max_iter", max_iter=-1, norm16=0)
    shifted = base.copy()
    shifted[0, np.nonzero(base[0] >= 0)[0][0]] = 7
    refused(N.PL_EINVAL, "shift", b=shifted, norm16=0)
    refused(N.PL_EINVAL, "layer_order", layer_order=[0, 1, 2, 2], norm16=0)
    refused(N.PL_EINVAL, "max_iter", max_iter=-1, b=shifted)
    # ... and its PL_EUNSUPPORTED ones behind the three parameters
    one = base.copy()
    one[0] = -1
    one[0, 3] = 5
    refused(N.PL_EUNSUPPORTED, "degree-1", b=one)
    refused(N.PL_EINVAL, "msg_max", b=one, msg_max=128)
    assert probe(one, 7, max_iter=0)[0] == 0  # no check is evaluated
    refused(N.PL_EUNSUPPORTED, "2048", b=np.zeros((1, 2048), dtype=np.int64), Z=1)
    refused(N.PL_EUNSUPPORTED, "1024", b=np.zeros((1, 2), dtype=np.int64), Z=1025)
    refused(N.PL_EINVAL, "norm16", b=np.zeros((1, 2), dtype=np.int64), Z=1025, norm16=17)
    assert N.lib.pl_debug_ldpc_qc_fixed_plan_probe(1, 2, 1, None, None, 20, 1, 12, 31, 31, 0, None) == N.PL_EINVAL
    # the floating-point entry points still ignore every flag bit but bit 0: no new bit was added
    assert float_probe(base, 7, 2 | 4 | 8).kernel == 11 and float_probe(base, 7, 1 | 2 | 4 | 8).kernel == 13


def test_decoder_constructor():
    L = _L()
    base = rows_base([6, 6, 6, 6], 8, 7)
    d = L.QCFixedMSDecoder(base, 7)
    assert (d.max_iter, d.normalization, d.norm16, d.early_stop, d.llr_scale, d.llr_max, d.msg_max) == \
        (50, 0.75, 12, True, 4.0, 31, 31)
    assert (d.n, d.m, d.Z, d.mb, d.nb) == (56, 28, 7, 4, 8) and d.layer_order is None
    assert d.H.shape == (28, 56) and len(d.layers) == 4 and "QCFixedMSDecoder" in repr(d)
    assert not isinstance(d, L.QCLayeredMSDecoder)
    for norm, n16 in ((1.0, 16), (0.0625, 1), (0.5, 8)):
        assert L.QCFixedMSDecoder(base, 7, normalization=norm).norm16 == n16
    for bad in (0.7, 0.0, 1.0625, -0.5, 0.76):
        with pytest.raises(ValueError, match="normalization"):
            L.QCFixedMSDecoder(base, 7, normalization=bad)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="llr_scale"):
            L.QCFixedMSDecoder(base, 7, llr_scale=bad)
    # the floating decoder keeps refusing every dtype but the two floats
    with pytest.raises(ValueError):
        L.QCLayeredMSDecoder(base, 7, dtype=np.int8)
    # an empty host batch needs no device
    bits, its, post = d.decode_batch(np.zeros((0, 56), dtype=np.int8), return_iterations=True, return_llr=True)
    assert bits.shape == (0, 56) and its.shape == (0,) and post.shape == (0, 56) and post.dtype == np.int8
    q = d.quantize_host(np.array([[0.125, 0.375, 100.0, np.nan]]))
    assert q.dtype == np.int8 and q.tolist() == [[0, 2, 31, 0]]


@pytest.mark.skipif(not os.path.exists(CLANGXX) and shutil.which("clang++") is None, reason="needs clang++")
def test_qc_fixed_planner_under_asan():
    cxx = CLANGXX if os.path.exists(CLANGXX) else shutil.which("clang++")
    build = os.path.join(HERE, "_build")
    os.makedirs(build, exist_ok=True)
    exe = os.path.join(build, "qc_fixed_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                    "-fno-sanitize-recover=all", os.path.join(HERE, "qc_fixed_plan_check.cpp"),
                    os.path.join(ROOT, "polarcode_and_ldpc_amd", "csrc", "ldpc_plan.cpp"), "-o", exe],
                   check=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "all checks passed" in p.stdout
    assert "ERROR: AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr

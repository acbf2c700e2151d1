"""The quasi-cyclic sum-product planner on the CPU, through
pl_debug_ldpc_qc_bp_plan_probe: the state layout against the formula the header
documents, the LDS / workspace boundary in both mappings, frames per wavefront
and wavefronts per workgroup by lifting size, the layer stream's digest against
the min-sum plan's, every refusal and their order.  QCLayeredBPDecoder's
constructor checks need no device."""
import ctypes

import numpy as np
import pytest

LDS_MAX = 160 * 1024
WAVE_MAX = 64 * 1024
VOTE = 128


def _N():
    from polarcode_and_ldpc_amd import _native
    return _native


def _L():
    import polarcode_and_ldpc_amd.ldpc as L
    return L


def probe(base, Z, max_iter=20, clip=64.0, lms_global=0, layer_order=None):
    """(rc, probe, message)"""
    N = _N()
    sh = np.ascontiguousarray(base, np.int32)
    lo = None if layer_order is None else np.ascontiguousarray(layer_order, np.int32)
    out = N.LdpcQcBpPlanProbe()
    rc = N.lib.pl_debug_ldpc_qc_bp_plan_probe(sh.shape[0], sh.shape[1], Z, sh.ctypes.data_as(ctypes.c_void_p),
                                              None if lo is None else lo.ctypes.data_as(ctypes.c_void_p), max_iter,
                                              1, clip, lms_global, ctypes.byref(out))
    return rc, out, N.lib.pl_last_error().decode()


def minsum_probe(base, Z, layer_order=None):
    N = _N()
    sh = np.ascontiguousarray(base, np.int32)
    lo = None if layer_order is None else np.ascontiguousarray(layer_order, np.int32)
    out = N.LdpcQcPlanProbe()
    assert N.lib.pl_debug_ldpc_qc_plan_probe(sh.shape[0], sh.shape[1], Z, sh.ctypes.data_as(ctypes.c_void_p),
                                             None if lo is None else lo.ctypes.data_as(ctypes.c_void_p), 20, 1, 0.75,
                                             0, ctypes.byref(out)) == 0
    return out


def rows_base(degrees, nb, Z, seed=0):
    rng = np.random.RandomState(seed)
    base = np.full((len(degrees), nb), -1, dtype=np.int64)
    for i, d in enumerate(degrees):
        base[i, np.sort(rng.choice(nb, d, replace=False))] = rng.randint(0, Z, d)
    return base


def align16(b):
    return (b + 15) & ~15


def state_bytes(nb, Z, blocks):
    return align16(align16(8 * nb * Z) + 8 * Z * blocks)


# Z: (frames per wavefront, wavefronts per workgroup) of the (4, 8) code with 6 blocks a row
FPW_FPB = {1: (64, 4), 7: (9, 4), 27: (2, 4), 64: (1, 4), 65: (1, 1), 96: (1, 1), 1024: (1, 1)}


@pytest.mark.parametrize("Z", sorted(FPW_FPB))
def test_frames_per_wavefront_and_per_workgroup(Z):
    base = rows_base([6, 6, 6, 6], 8, Z)
    rc, p, msg = probe(base, Z)
    assert rc == 0, msg
    assert (p.fpw, p.fpb) == FPW_FPB[Z]
    assert p.threads == (64 * p.fpb if Z <= 64 else (Z + 63) // 64 * 64)
    assert p.state_bytes == state_bytes(8, Z, 24)
    if Z <= 64:  # the wavefront's frames fit 64 KB / 4 here, so four wavefronts share a workgroup
        assert p.state_bytes * p.fpw * 4 <= WAVE_MAX and p.lds_bytes == p.state_bytes * p.fpw * p.fpb
    if Z == 1024:  # 8 x 1024 x 8 + 24 x 1024 x 8 = 256 KiB: the workspace
        assert p.use_global == 1 and p.kernel == 18 and p.lds_bytes == VOTE


@pytest.mark.parametrize("degrees,nb,Z", [([6, 6, 6, 6], 8, 1), ([6, 5, 8, 2], 8, 27), ([6, 0, 6, 6], 8, 7),
                                          ([12, 15, 9], 16, 7), ([15, 2], 16, 96), ([17, 32, 24], 48, 7),
                                          ([33, 2], 48, 96), ([40, 64, 65], 70, 7), ([6] * 46, 68, 384),
                                          ([3] * 16, 24, 1024)])
def test_layout_and_mapping(degrees, nb, Z):
    """P[n] f64, then at off_r = align16(8 n) R as [blocks][Z] f64; state_bytes = align16(off_r + 8 Z blocks);
    no check words, no register-resident instance; the mapping and the stream are the min-sum plan's."""
    base = rows_base(degrees, nb, Z)
    rc, p, msg = probe(base, Z, clip=12.5)
    assert rc == 0, msg
    mb, blocks = len(degrees), sum(degrees)
    n = nb * Z
    assert (p.z, p.mb, p.nb, p.maxdc, p.mw, p.dcap, p.clip) == (Z, mb, nb, max(degrees), 0, 0, 12.5)
    assert p.off_r == align16(8 * n) and p.state_bytes == align16(p.off_r + 8 * Z * blocks)
    fpw = 64 // Z if Z <= 64 else 1
    assert p.fpw == fpw
    if Z <= 64:
        wave = p.state_bytes * fpw
        home = wave > LDS_MAX
        assert p.fpb == (4 if home else max(1, min(4, WAVE_MAX // wave))) and p.threads == 64 * p.fpb
        assert p.lds_bytes == (0 if home else wave * p.fpb)
    else:
        home = p.state_bytes + VOTE > LDS_MAX
        assert p.fpb == 1 and p.threads == (Z + 63) // 64 * 64
        assert p.lds_bytes == (0 if home else p.state_bytes) + VOTE
    assert p.use_global == int(home) and p.kernel == (18 if home else 17)
    ms = minsum_probe(base, Z)
    assert (p.table_len, p.digest, p.fpw) == (ms.table_len, ms.digest, ms.fpw)
    assert p.table_len == 2 * mb + 2 * blocks
    # PL_LMS_GLOBAL=1: the workspace, whatever the size
    rc, g, msg = probe(base, Z, clip=12.5, lms_global=1)
    assert rc == 0 and g.use_global == 1 and g.kernel == 18 and g.state_bytes == p.state_bytes
    assert g.lds_bytes == (0 if Z <= 64 else VOTE) and g.fpb == (4 if Z <= 64 else 1)


def test_layer_order_gives_the_min_sum_plans_stream():
    base = rows_base([6, 5, 8, 2], 8, 27)
    order = [2, 0, 3, 1]
    rc, p, msg = probe(base, 27, layer_order=order)
    assert rc == 0, msg
    assert p.digest == minsum_probe(base, 27, order).digest != minsum_probe(base, 27).digest
    assert p.state_bytes == probe(base, 27)[1].state_bytes


def _chain(k):
    """k degree-2 block rows over k + 1 block columns: 2 k blocks."""
    base = np.full((k, k + 1), -1, dtype=np.int64)
    base[np.arange(k), np.arange(k)] = 0
    base[np.arange(k), np.arange(k) + 1] = 1
    return base


@pytest.mark.parametrize("Z,bound", [(64, "lds"), (96, "lds"), (16, "lds"), (64, "wave"), (16, "wave")])
def test_lds_and_wavefront_bounds(Z, bound):
    """The largest state on one side of each bound and the next one: the 160 KB of a workgroup's LDS in
    the SUBWAVE mapping (Z = 64: one frame a wavefront; Z = 16: four) and in the block mapping (Z = 96:
    the vote words count), where the state moves to the workspace; and the 64 KB a wavefront's frames
    may take before fewer than four wavefronts share a workgroup."""
    fpw = 64 // Z if Z <= 64 else 1

    def state(k):
        return state_bytes(k + 1, Z, 2 * k)

    if bound == "lds":
        limit = LDS_MAX - (0 if Z <= 64 else VOTE)
        k0 = max(k for k in range(2, 2000) if state(k) * fpw <= limit)
        for k, home in ((k0, 0), (k0 + 1, 1)):
            rc, p, msg = probe(_chain(k), Z)
            assert rc == 0, msg
            assert p.state_bytes == state(k) and p.use_global == home and p.kernel == 17 + home, (k, p.state_bytes)
            assert (p.state_bytes * fpw <= limit) == (home == 0)
            if Z <= 64:
                assert p.fpb == (4 if home else 1)
    else:
        k0 = max(k for k in range(2, 2000) if state(k) * fpw * 4 <= WAVE_MAX)
        for k, fpb in ((k0, 4), (k0 + 1, 3)):
            rc, p, msg = probe(_chain(k), Z)
            assert rc == 0, msg
            assert p.use_global == 0 and p.fpb == fpb == WAVE_MAX // (p.state_bytes * fpw)
            assert p.lds_bytes == p.state_bytes * fpw * fpb and p.threads == 64 * fpb


def test_refusals_and_their_order():
    N = _N()
    base = rows_base([6, 6, 6, 6], 8, 7)

    def refused(code, word, b=base, Z=7, **kw):
        rc, _, msg = probe(b, Z, **kw)
        assert rc == code and word in msg, (rc, msg)

    for bad in (0.0, -0.0, -1.0, 2.0 ** 20 + 1.0, float("inf"), -float("inf"), float("nan"), 1e300):
        refused(N.PL_EINVAL, "clip", clip=bad)
    for good in (2.0 ** 20, 5e-324, 1e-3, 64.0):
        assert probe(base, 7, clip=good)[0] == 0
    # pl_ldpc_qc_plan_create's checks come first, in its order ...
    refused(N.PL_EINVAL, "must be >= 1", b=np.zeros((1, 2), dtype=np.int64), Z=0, clip=0.0)
    refused(N.PL_EINVAL, "32 bits", b=np.zeros((1, 2), dtype=np.int64), Z=2 ** 30, clip=0.0)
    refused(N.PL_EINVAL, "max_iter", max_iter=-1, clip=0.0)
    shifted = base.copy()
    shifted[0, np.nonzero(base[0] >= 0)[0][0]] = 7
    refused(N.PL_EINVAL, "shift", b=shifted, clip=0.0)
    refused(N.PL_EINVAL, "max_iter", max_iter=-1, b=shifted)
    refused(N.PL_EINVAL, "layer_order", layer_order=[0, 1, 2, 2], clip=0.0)
    # ... and its PL_EUNSUPPORTED ones behind clip; the degree-1 refusal has a message of its own
    one = base.copy()
    one[0] = -1
    one[0, 3] = 5
    refused(N.PL_EUNSUPPORTED, "sum-product on a degree-1 check", b=one)
    rc, _, msg = probe(one, 7)
    assert "min-sum" not in msg
    refused(N.PL_EINVAL, "clip", b=one, clip=0.0)
    assert probe(one, 7, max_iter=0)[0] == 0  # no check is evaluated
    refused(N.PL_EUNSUPPORTED, "2048", b=np.zeros((1, 2048), dtype=np.int64), Z=1)
    assert probe(np.zeros((1, 2047), dtype=np.int64), 1)[0] == 0
    refused(N.PL_EUNSUPPORTED, "1024", b=np.zeros((1, 2), dtype=np.int64), Z=1025)
    refused(N.PL_EINVAL, "clip", b=np.zeros((1, 2), dtype=np.int64), Z=1025, clip=float("nan"))
    # degree-1 comes before the degree and Z bounds, as in the min-sum plan
    big = np.zeros((2, 2048), dtype=np.int64)
    big[1, 1:] = -1
    refused(N.PL_EUNSUPPORTED, "degree-1", b=big, Z=1)
    assert N.lib.pl_debug_ldpc_qc_bp_plan_probe(1, 2, 1, None, None, 20, 1, 64.0, 0, None) == N.PL_EINVAL
    # the min-sum plan's own degree-1 message is what it was
    sh = np.ascontiguousarray(one, np.int32)
    out = N.LdpcQcPlanProbe()
    assert N.lib.pl_debug_ldpc_qc_plan_probe(4, 8, 7, sh.ctypes.data_as(ctypes.c_void_p), None, 20, 1, 0.75, 0,
                                             ctypes.byref(out)) == N.PL_EUNSUPPORTED
    assert "min-sum on a degree-1 check" in N.lib.pl_last_error().decode()


def test_decoder_constructor():
    L = _L()
    base = rows_base([6, 6, 6, 6], 8, 7)
    d = L.QCLayeredBPDecoder(base, 7)
    assert (d.max_iter, d.early_stop, d.clip, d.layer_order) == (50, True, 64.0, None)
    assert (d.n, d.m, d.Z, d.mb, d.nb) == (56, 28, 7, 4, 8)
    assert d.H.shape == (28, 56) and np.array_equal(d.H, L.qc_expand(base, 7)) and len(d.layers) == 4
    assert "QCLayeredBPDecoder" in repr(d) and "clip=64.0" in repr(d)
    assert not isinstance(d, L.QCLayeredMSDecoder) and isinstance(d, L.LayeredMSDecoder)
    assert L.QCLayeredBPDecoder(base, 7, 10, False, [3, 2, 1, 0], 4.0).layer_order == [3, 2, 1, 0]
    with pytest.raises(TypeError):
        L.QCLayeredBPDecoder(base, 7, dtype=np.float32)
    for bad in (0.0, -1.0, float("inf"), float("nan"), 2.0 ** 20 + 1):
        with pytest.raises(ValueError, match="clip"):
            L.QCLayeredBPDecoder(base, 7, clip=bad)
    # an empty host batch needs no device
    bits, its, post = d.decode_batch(np.zeros((0, 56)), return_iterations=True, return_llr=True)
    assert bits.shape == (0, 56) and its.shape == (0,) and post.shape == (0, 56) and post.dtype == np.float64
    one = base.copy()
    one[0] = -1
    one[0, 3] = 5
    with pytest.raises(ValueError, match="degree-1"):
        L.QCLayeredBPDecoder(one, 7).decode_batch(np.zeros((0, 56)))
    assert L.QCLayeredBPDecoder(one, 7, max_iter=0).decode_batch(np.zeros((0, 56))).shape == (0, 56)

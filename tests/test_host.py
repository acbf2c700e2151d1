"""Host-side logic that needs no GPU: the C-ABI library loads and exports every
symbol include/polarldpc.h declares; frozen-set construction, CRC, encoders and
H construction reproduce the reference's values (golden vectors)."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT, golden


def _header_symbols():
    txt = open(os.path.join(ROOT, "include", "polarldpc.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(pl_[a-z0-9_]+)\s*\(", txt)))


def test_library_exports_every_header_symbol():
    from polarcode_and_ldpc_amd import _native
    syms = _header_symbols()
    assert len(syms) >= 11
    for s in syms:
        assert hasattr(_native.lib, s), s
    assert set(syms) == set(_native.EXPORTS)
    # the error channel works without a device
    assert isinstance(_native.lib.pl_last_error(), bytes)


def test_plan_create_argument_errors():
    """Argument validation happens before any device work (no GPU needed)."""
    from polarcode_and_ldpc_amd import _native
    h = ctypes.c_void_p()
    mask = np.zeros(100, np.uint8)
    rc = _native.lib.pl_polar_plan_create(100, 50, mask.ctypes.data_as(ctypes.c_void_p), 8, 0, ctypes.byref(h))
    assert rc == _native.PL_EINVAL and b"power of 2" in _native.lib.pl_last_error()
    mask = np.zeros(64, np.uint8)
    rc = _native.lib.pl_polar_plan_create(64, 32, mask.ctypes.data_as(ctypes.c_void_p), 65537, 0, ctypes.byref(h))
    assert rc == _native.PL_EUNSUPPORTED  # lists above 65536
    rp = np.array([0, 1], np.int32)
    ci = np.array([3], np.int32)
    rc = _native.lib.pl_ldpc_plan_create(1, 4, rp.ctypes.data_as(ctypes.c_void_p), ci.ctypes.data_as(ctypes.c_void_p),
                                         1, 20, 1, 1.0, 0, ctypes.byref(h))
    assert rc == _native.PL_EUNSUPPORTED  # MS on a degree-1 check


def test_no_cpu_fallback_without_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("device present")
    from polarcode_and_ldpc_amd.polar import SCDecoder
    with pytest.raises(RuntimeError):
        SCDecoder(64, 32).decode(np.ones(64))


def test_frozen_sets_match_reference():
    from polarcode_and_ldpc_amd.polar import construct_frozen_set, generate_frozen_bits
    assert np.array_equal(generate_frozen_bits(1024, 512)[0],
                          golden("polar_sc_1024_default.npz")["default_frozen"])
    assert np.array_equal(construct_frozen_set(1024, 512, 2.0), golden("polar_sc_1024_bhatta.npz")["bhatta_frozen"])
    d = golden("polar_scl_4096_l8.npz")
    assert np.array_equal(construct_frozen_set(4096, 2048, 2.0), d["frozen"])
    d = golden("polar_p1.npz")
    assert np.array_equal(generate_frozen_bits(256, 128)[0], d["frozen"])
    f, i = generate_frozen_bits(1024, 512)
    assert np.array_equal(i, np.arange(1, 1024, 2))


def test_bit_reverse():
    from polarcode_and_ldpc_amd.polar.utils import bit_reverse, bit_reverse_indices
    for n in (1, 3, 10):
        r = bit_reverse_indices(n)
        assert all(r[i] == bit_reverse(i, n) for i in range(1 << n))
        assert np.array_equal(r[r], np.arange(1 << n))


def test_crc_matches_reference():
    from polarcode_and_ldpc_amd.polar import crc_check, crc_encode
    d = golden("crc.npz")
    for poly in ("CRC-8", "CRC-16", "CRC-24"):
        tag = poly.replace("-", "")
        for data, enc in zip(d[tag + "_data"], d[tag + "_enc"]):
            assert np.array_equal(crc_encode(data, poly), enc)
            assert crc_check(enc, poly)
            bad = enc.copy()
            bad[0] ^= 1
            assert not crc_check(bad, poly)


def test_polar_encoder_kat():
    from polarcode_and_ldpc_amd.polar import PolarEncoder
    d = golden("polar_kat16.npz")
    enc = PolarEncoder(16, 8, frozen_bits=d["frozen"])
    assert np.array_equal(enc.encode(d["msg"]), d["codeword"])
    # encoding is an involution on u
    from polarcode_and_ldpc_amd.polar import polar_transform
    u = np.random.RandomState(0).randint(0, 2, (5, 256))
    assert np.array_equal(polar_transform(polar_transform(u)), u)


def test_ldpc_matrix_and_encoder_match_reference():
    from polarcode_and_ldpc_amd.ldpc import LDPCEncoder, csr_to_dense, dense_to_csr, mackay_construction
    d = golden("ldpc_bp_504.npz")
    H = mackay_construction(504, 252, 3, 6, seed=42)
    rp, ci = dense_to_csr(H)
    assert np.array_equal(rp, d["row_ptr"]) and np.array_equal(ci, d["col_idx"])
    assert np.array_equal(csr_to_dense(rp, ci, 504), H)
    deg = np.diff(rp)
    assert deg.min() == 0 and (deg == 1).sum() == 2 and deg.max() == 13 and rp[-1] == 1512
    enc = LDPCEncoder(504, 252, dv=3, dc=6, seed=42)
    assert enc.use_direct_solving
    assert np.array_equal(enc.encode_batch(d["harness_msg"]), d["harness_cw"])
    assert np.array_equal(enc.encode_batch(d["enc_msg"]), d["enc_cw"])
    assert not enc.verify_codeword(d["harness_cw"][0])  # invalid codewords (quirk 2)


def test_regular_construction():
    from polarcode_and_ldpc_amd.ldpc import regular_construction
    H = regular_construction(8192, 3, 6, seed=1)
    assert (H.sum(axis=0) == 3).all() and (H.sum(axis=1) == 6).all()


def test_host_channel_and_encoder_regenerate_p1():
    """the BER-parity tests' "reference side" uses the build's
    host PolarEncoder and AWGNChannel.transmit.  Replaying the reference's own
    generation of polar_p1.npz (benchmarks/throughput_test.py:196-228: 10
    warm-up frames, then 100 messages, AWGNChannel(3.0, seed=42), the global
    legacy NumPy stream of src/channel/awgn.py:34-35,88) with them reproduces the
    fixture's messages and LLRs bit for bit."""
    from polarcode_and_ldpc_amd.channel import AWGNChannel
    from polarcode_and_ldpc_amd.polar import PolarEncoder
    g = golden("polar_p1.npz")
    state = np.random.get_state()
    try:
        enc = PolarEncoder(256, 128)
        assert np.array_equal(np.asarray(enc.get_frozen_bits_positions()), g["frozen"])
        ch = AWGNChannel(snr_db=3.0, seed=42)
        for _ in range(10):  # warm-up frames (their decodes draw nothing from the stream)
            ch.transmit(enc.encode(np.random.randint(0, 2, 128)), return_llr=True)
        msgs = np.array([np.random.randint(0, 2, 128) for _ in range(100)])
        llrs = np.array([ch.transmit(enc.encode(m), return_llr=True) for m in msgs])
    finally:
        np.random.set_state(state)
    assert np.array_equal(msgs, g["msg"])
    assert llrs.dtype == np.float64 and np.array_equal(llrs, g["llr"])

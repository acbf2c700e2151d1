"""ctypes binding of libpolarldpc.so (include/polarldpc.h).

The HIP library is the only compute path: if it is missing or cannot be
loaded this module raises at import time -- there is no CPU fallback.
PyTorch (ROCm) is used only to own device buffers and streams: it is imported
first so that the library binds to the same HIP runtime instance as torch.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np
import torch  # noqa: F401  (loads torch's libamdhip64 first; our .so reuses it)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PL_LIB_PATH", os.path.join(_HERE, "_lib", "libpolarldpc.so"))

PL_OK, PL_EINVAL, PL_ENOMEM, PL_EHIP, PL_EUNSUPPORTED = 0, -1, -2, -3, -4
PL_LDPC_BP, PL_LDPC_MS, PL_LDPC_LMS = 0, 1, 2
PL_LDPC_QC_F32 = 1  # pl_ldpc_qc_plan_create flag: state and arithmetic in single precision

EXPORTS = (
    "pl_polar_plan_create", "pl_ldpc_plan_create", "pl_decode", "pl_plan_reserve", "pl_plan_get_info",
    "pl_plan_destroy", "pl_last_error", "pl_random_bits", "pl_polar_encode", "pl_awgn_llr",
    "pl_count_errors", "pl_debug_polar_stamps", "pl_debug_ldpc_stamps", "pl_debug_polar_deadstore", "pl_polar_plan_set_crc", "pl_crc_append",
    "pl_rayleigh_llr", "pl_bsc", "pl_gf2_encode", "pl_decode_ws", "pl_plan_workspace_bytes",
    "pl_plan_release", "pl_plan_workspace_stats", "pl_debug_set_plan_device", "pl_debug_polar_fpw",
    "pl_debug_polar_flagged", "pl_polar_plan_small_batch", "pl_ldpc_layered_plan_create", "pl_ldpc_decode_soft",
    "pl_debug_ldpc_plan_probe", "pl_debug_ldpc_layered_plan_probe", "pl_ldpc_qc_plan_create",
    "pl_debug_ldpc_qc_plan_probe", "pl_ldpc_decode_f32", "pl_debug_ldpc_qc_plan_probe_flags",
    "pl_ldpc_qc_encoder_create", "pl_ldpc_qc_encode", "pl_ldpc_qc_encoder_destroy", "pl_debug_ldpc_qc_encoder_probe",
    "pl_debug_set_qc_encoder_device", "pl_ldpc_rate_match_check", "pl_debug_rate_match_probe", "pl_ldpc_rate_match",
    "pl_ldpc_rate_recover", "pl_ldpc_qc_fixed_plan_create", "pl_ldpc_decode_i8", "pl_llr_quantize",
    "pl_debug_ldpc_qc_fixed_plan_probe", "pl_polar_rate_match_check", "pl_debug_polar_rate_match_probe",
    "pl_polar_rate_match_forced", "pl_polar_rate_match", "pl_polar_rate_recover",
    "pl_qam_check", "pl_qam_modulate", "pl_qam_awgn", "pl_qam_demap",
    "pl_qam_fading_check", "pl_qam_rayleigh", "pl_qam_demap_csi", "pl_qam_demap_logmap", "pl_qam_demap_csi_logmap",
    "pl_interleave_check", "pl_interleave_index", "pl_interleave_lds_max_e", "pl_bit_interleave", "pl_llr_deinterleave",
    "pl_ldpc_qc_bp_plan_create", "pl_debug_ldpc_qc_bp_plan_probe",
)
PL_QUANT_LLR_F32 = 1  # pl_llr_quantize flag: llr_dev is float (else double)
PL_RM_LLR_F32, PL_RM_OUT_F32, PL_RM_ACCUMULATE = 1, 2, 4  # pl_ldpc_rate_recover flags
PL_PRM_PUNCTURE, PL_PRM_SHORTEN = 0, 1  # pl_polar_rm.mode
PL_PRM_LLR_F32, PL_PRM_ACCUMULATE = 1, 4  # pl_polar_rate_recover flags
PL_QAM_LLR_F32 = 1  # pl_qam_demap flag: llr_dev is float (else double)
PL_ILV_RECT, PL_ILV_TRI = 0, 1  # the interleaver's kind
PL_ILV_LLR_F32 = 1  # pl_llr_deinterleave flag: f_dev and e_dev are float (else double)


class PlanInfo(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int32), ("n_in", ctypes.c_int32), ("n_out", ctypes.c_int32),
                ("list_size", ctypes.c_int32), ("lds_bytes", ctypes.c_int32), ("fused_top", ctypes.c_int32),
                ("frames_per_block", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class LdpcPlanProbe(ctypes.Structure):
    """pl_ldpc_plan_probe: what the host-side planner decides for a flooding plan (no device call)."""
    _fields_ = [(f, ctypes.c_int32) for f in ("kernel", "threads", "lds_bytes", "use_global", "reg_variant", "grp",
                                              "fpg", "tl", "npad", "compact", "ms36")] + \
               [(f, ctypes.c_int64) for f in ("work_bytes_per_frame", "table_len", "grp_at", "ms_vw_at")] + \
               [("digest", ctypes.c_uint64)]


class LdpcLayeredPlanProbe(ctypes.Structure):
    """pl_ldpc_layered_plan_probe: the layered kernel's geometry."""
    _fields_ = [(f, ctypes.c_int32) for f in ("kernel", "maxdc", "n_layers", "max_layer", "mw", "wave", "use_global",
                                              "fpb", "threads", "lds_bytes")] + \
               [(f, ctypes.c_int64) for f in ("state_bytes", "off_mm", "off_meta", "table_len")] + \
               [("digest", ctypes.c_uint64)]


class LdpcQcPlanProbe(ctypes.Structure):
    """pl_ldpc_qc_plan_probe: the quasi-cyclic layered kernel's geometry."""
    _fields_ = [(f, ctypes.c_int32) for f in ("kernel", "z", "mb", "nb", "maxdc", "dcap", "mw", "fpw", "fpb", "threads",
                                              "lds_bytes", "use_global")] + \
               [(f, ctypes.c_int64) for f in ("state_bytes", "table_len")] + \
               [("digest", ctypes.c_uint64)]


class LdpcQcFixedPlanProbe(ctypes.Structure):
    """pl_ldpc_qc_fixed_plan_probe: the fixed-point quasi-cyclic kernel's geometry."""
    _fields_ = [(f, ctypes.c_int32) for f in ("kernel", "z", "mb", "nb", "maxdc", "dcap", "mw", "fpw", "fpb", "threads",
                                              "lds_bytes", "use_global", "norm16", "llr_max", "msg_max", "pad")] + \
               [(f, ctypes.c_int64) for f in ("state_bytes", "off_p", "table_len")] + \
               [("digest", ctypes.c_uint64)]


class LdpcQcBpPlanProbe(ctypes.Structure):
    """pl_ldpc_qc_bp_plan_probe: the quasi-cyclic sum-product kernel's geometry."""
    _fields_ = [(f, ctypes.c_int32) for f in ("kernel", "z", "mb", "nb", "maxdc", "dcap", "mw", "fpw", "fpb", "threads",
                                              "lds_bytes", "use_global")] + \
               [("clip", ctypes.c_double)] + \
               [(f, ctypes.c_int64) for f in ("state_bytes", "off_r", "table_len")] + \
               [("digest", ctypes.c_uint64)]


class QcEncoderProbe(ctypes.Structure):
    """pl_qc_encoder_probe: the quasi-cyclic encoder's structure, geometry and stream."""
    _fields_ = [(f, ctypes.c_int32) for f in ("g", "x", "a", "b", "subwave", "fpw", "fpb", "threads", "lds_bytes",
                                              "n_sync")] + \
               [("table_len", ctypes.c_int64), ("digest", ctypes.c_uint64)]


class RateMatch(ctypes.Structure):
    """pl_rate_match: the parameters of a rate matching and the fields pl_ldpc_rate_match_check derives."""
    _fields_ = [(f, ctypes.c_int32) for f in ("mb", "nb", "z", "punctured", "fillers", "ncb", "start", "E",
                                              "n", "k", "P", "M", "c0", "hi", "max_reps")]


class PolarRateMatch(ctypes.Structure):
    """pl_polar_rm: the parameters of a polar rate matching and the fields pl_polar_rate_match_check derives."""
    _fields_ = [(f, ctypes.c_int32) for f in ("N", "E", "mode", "nsub")] + [("perm", ctypes.c_uint8 * 32)] + \
               [(f, ctypes.c_int32) for f in ("S", "U", "max_reps", "pad")] + [("inv", ctypes.c_uint8 * 32)]


def _load(path=LIB_PATH):
    if not os.path.exists(path):
        raise ImportError(
            "polarcode_and_ldpc_amd: native library %s not found -- build it with "
            "`python -c 'import __graft_entry__ as g; g.build()'` (make -C polarcode_and_ldpc_amd/csrc). "
            "There is no CPU fallback." % path)
    L = ctypes.CDLL(path)
    P, I32, I64, D = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_double
    PP = ctypes.POINTER(ctypes.c_void_p)
    L.pl_polar_plan_create.argtypes = [I32, I32, P, I32, I32, PP]
    L.pl_ldpc_plan_create.argtypes = [I32, I32, P, P, I32, I32, I32, D, I32, PP]
    L.pl_ldpc_layered_plan_create.argtypes = [I32, I32, P, P, I32, P, P, I32, I32, D, I32, PP]
    L.pl_debug_ldpc_plan_probe.argtypes = [I32, I32, P, P, I32, I32, I32, D, I32, I32, I32, ctypes.POINTER(LdpcPlanProbe)]
    L.pl_debug_ldpc_layered_plan_probe.argtypes = [I32, I32, P, P, I32, P, P, I32, I32, D, I32, I32, I32,
                                                   ctypes.POINTER(LdpcLayeredPlanProbe)]
    L.pl_ldpc_qc_plan_create.argtypes = [I32, I32, I32, P, P, I32, I32, D, I32, PP]
    L.pl_debug_ldpc_qc_plan_probe.argtypes = [I32, I32, I32, P, P, I32, I32, D, I32, ctypes.POINTER(LdpcQcPlanProbe)]
    L.pl_debug_ldpc_qc_plan_probe_flags.argtypes = [I32, I32, I32, P, P, I32, I32, D, I32, I32,
                                                    ctypes.POINTER(LdpcQcPlanProbe)]
    L.pl_ldpc_qc_fixed_plan_create.argtypes = [I32, I32, I32, P, P, I32, I32, I32, I32, I32, PP]
    L.pl_debug_ldpc_qc_fixed_plan_probe.argtypes = [I32, I32, I32, P, P, I32, I32, I32, I32, I32, I32,
                                                    ctypes.POINTER(LdpcQcFixedPlanProbe)]
    L.pl_ldpc_qc_bp_plan_create.argtypes = [I32, I32, I32, P, P, I32, I32, D, PP]
    L.pl_debug_ldpc_qc_bp_plan_probe.argtypes = [I32, I32, I32, P, P, I32, I32, D, I32,
                                                 ctypes.POINTER(LdpcQcBpPlanProbe)]
    L.pl_ldpc_decode_i8.argtypes = [P, P, I64, I64, P, P, P, I64, P, I64, P]
    L.pl_llr_quantize.argtypes = [P, I32, I64, I64, I32, D, I32, P, I64, P]
    L.pl_ldpc_qc_encoder_create.argtypes = [I32, I32, I32, P, PP]
    L.pl_ldpc_qc_encode.argtypes = [P, P, I64, I64, P, I64, P]
    L.pl_ldpc_qc_encoder_destroy.argtypes = [P]
    L.pl_debug_ldpc_qc_encoder_probe.argtypes = [I32, I32, I32, P, ctypes.POINTER(QcEncoderProbe)]
    L.pl_debug_set_qc_encoder_device.argtypes = [P, I32]
    L.pl_ldpc_rate_match_check.argtypes = [ctypes.POINTER(RateMatch)]
    L.pl_debug_rate_match_probe.argtypes = [I32] * 8 + [ctypes.POINTER(RateMatch)]
    L.pl_ldpc_rate_match.argtypes = [ctypes.POINTER(RateMatch), P, I64, I64, P, I64, P]
    L.pl_ldpc_rate_recover.argtypes = [ctypes.POINTER(RateMatch), P, I64, I64, P, I64, I32, D, I32, P]
    L.pl_polar_rate_match_check.argtypes = [ctypes.POINTER(PolarRateMatch)]
    L.pl_debug_polar_rate_match_probe.argtypes = [I32] * 4 + [P, ctypes.POINTER(PolarRateMatch)]
    L.pl_polar_rate_match_forced.argtypes = [ctypes.POINTER(PolarRateMatch), P]
    L.pl_polar_rate_match.argtypes = [ctypes.POINTER(PolarRateMatch), P, I64, I64, P, I64, P]
    L.pl_polar_rate_recover.argtypes = [ctypes.POINTER(PolarRateMatch), P, I64, I64, P, I64, D, I32, P]
    L.pl_qam_check.argtypes = [I32, I64, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_double)]
    L.pl_qam_modulate.argtypes = [I32, I64, I64, P, I64, P, I64, P]
    L.pl_qam_awgn.argtypes = [I32, I64, I64, P, I64, D, ctypes.c_uint64, I64, P, I64, P]
    L.pl_qam_demap.argtypes = [I32, I64, I64, P, I64, D, P, I64, I32, P]
    L.pl_qam_fading_check.argtypes = [I32, I64, I64, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)]
    L.pl_qam_rayleigh.argtypes = [I32, I64, I64, I64, P, I64, D, ctypes.c_uint64, I64, P, I64, P, I64, P]
    L.pl_qam_demap_csi.argtypes = [I32, I64, I64, I64, P, I64, P, I64, D, P, I64, I32, P]
    L.pl_qam_demap_logmap.argtypes = L.pl_qam_demap.argtypes
    L.pl_qam_demap_csi_logmap.argtypes = L.pl_qam_demap_csi.argtypes
    L.pl_interleave_check.argtypes = [I32, I32, I64, ctypes.POINTER(ctypes.c_int64)]
    L.pl_interleave_index.argtypes = [I32, I32, I64, I64, ctypes.POINTER(ctypes.c_int64)]
    L.pl_interleave_lds_max_e.argtypes = [I32]
    L.pl_bit_interleave.argtypes = [I32, I32, I64, I64, P, I64, P, I64, P]
    L.pl_llr_deinterleave.argtypes = [I32, I32, I64, I64, P, I64, P, I64, I32, P]
    L.pl_ldpc_decode_soft.argtypes = [P, P, I64, I64, P, P, P, I64, P]
    L.pl_ldpc_decode_f32.argtypes = [P, P, I64, I64, P, P, P, I64, P, I64, P]
    L.pl_decode.argtypes = [P, P, I64, I64, P, P, P]
    L.pl_plan_reserve.argtypes = [P, I64, P]
    L.pl_decode_ws.argtypes = [P, P, I64, I64, P, P, P, I64, P]
    L.pl_plan_workspace_bytes.argtypes = [P, I64, ctypes.POINTER(ctypes.c_int64)]
    L.pl_plan_release.argtypes = [P, P]
    L.pl_plan_workspace_stats.argtypes = [P, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)]
    L.pl_debug_set_plan_device.argtypes = [P, I32]
    L.pl_plan_get_info.argtypes = [P, ctypes.POINTER(PlanInfo)]
    L.pl_polar_plan_small_batch.argtypes = [P, ctypes.POINTER(ctypes.c_int64)]
    L.pl_plan_destroy.argtypes = [P]
    L.pl_last_error.restype = ctypes.c_char_p
    L.pl_random_bits.argtypes = [ctypes.c_uint64, I64, I64, I32, P, P]
    L.pl_polar_encode.argtypes = [P, P, I64, P, P]
    L.pl_awgn_llr.argtypes = [P, I32, I64, D, ctypes.c_uint64, I64, P, I64, P]
    L.pl_count_errors.argtypes = [P, I64, P, I64, I32, I64, P, P]
    L.pl_debug_polar_stamps.argtypes = [P, P, I64, I64, P, P, P]
    L.pl_debug_polar_fpw.argtypes = [P, P, I64, I64, P, P, I32, P]
    L.pl_debug_ldpc_stamps.argtypes = [P, P, I64, I64, P, P, P, P]
    L.pl_debug_polar_deadstore.argtypes = [P, P, I64, I64, P, P, I32, P]
    L.pl_debug_polar_flagged.argtypes = [P, P, I64, I64, P, P, P]
    L.pl_polar_plan_set_crc.argtypes = [P, I32, ctypes.c_uint32]
    L.pl_crc_append.argtypes = [P, I64, I64, I32, I32, ctypes.c_uint32, P]
    L.pl_rayleigh_llr.argtypes = [P, I32, I64, D, ctypes.c_uint64, I64, P, I64, P]
    L.pl_bsc.argtypes = [P, I32, I64, D, ctypes.c_uint64, I64, P, I64, P]
    L.pl_gf2_encode.argtypes = [P, I32, I32, P, I64, I64, P, I64, P]
    for name in EXPORTS:
        getattr(L, name).restype = ctypes.c_int if name != "pl_last_error" else ctypes.c_char_p
    L.pl_interleave_lds_max_e.restype = ctypes.c_int64
    return L


lib = _load()
_BUILD_ID = None
DIAG_LIB_PATH = os.path.join(_HERE, "_lib", "diag", "libpolarldpc_diag.so")


def load_diag():
    """The diagnostic build (make diag: stamped kernels, test hooks), bound like
    the product library, or None if it was not built.  Tests and tools only."""
    return _load(DIAG_LIB_PATH) if os.path.exists(DIAG_LIB_PATH) else None


def build_id() -> str:
    """Digest of the loaded libpolarldpc.so (keys resumable result logs to the
    decoder build that produced them)."""
    global _BUILD_ID
    if _BUILD_ID is None:
        import hashlib
        with open(LIB_PATH, "rb") as f:
            _BUILD_ID = hashlib.sha1(f.read()).hexdigest()[:16]
    return _BUILD_ID


class NativeError(RuntimeError):
    pass


def check(rc: int, what: str):
    if rc == PL_OK:
        return
    msg = (lib.pl_last_error() or b"").decode(errors="replace")
    if rc == PL_EINVAL:
        raise AssertionError("%s: %s" % (what, msg))
    if rc == PL_EUNSUPPORTED:
        raise ValueError("%s: %s" % (what, msg))
    raise NativeError("%s failed (%d): %s" % (what, rc, msg))


def _stream(stream=None) -> int:
    if stream is None:
        stream = torch.cuda.current_stream()
    return int(stream.cuda_stream) if hasattr(stream, "cuda_stream") else int(stream)


def _ld(t: "torch.Tensor") -> int:
    """Row pitch in elements; a single row may carry any stride (e.g. 0 from a
    NumPy newaxis view), so it is normalised to the row length."""
    return int(t.stride(0)) if t.shape[0] > 1 else int(t.shape[1])


def _dptr(t: "torch.Tensor"):
    assert t.is_cuda and (t.dim() < 2 or t.stride(-1) == 1), "device tensor must have unit inner stride"
    return ctypes.c_void_p(t.data_ptr())


def require_gpu():
    if not torch.cuda.is_available():
        raise RuntimeError("polarcode_and_ldpc_amd: no HIP device visible (the decoders run on MI355X only)")


class Plan:
    """Owner of a pl_plan*.  The plan holds device constants; decode workspace is
    per stream (grown lazily by the library) or caller-supplied (decode(ws=...))."""

    def __init__(self, handle: ctypes.c_void_p):
        self._h = handle
        info = PlanInfo()
        check(lib.pl_plan_get_info(self._h, ctypes.byref(info)), "pl_plan_get_info")
        self.info = info
        # a quasi-cyclic plan created with PL_LDPC_QC_F32 (it also takes fp32 llr / post); fixed at creation
        self.f32 = info.reserved in (13, 14)
        # an int8 fixed-point plan (pl_ldpc_qc_fixed_plan_create): int8 llr / post through pl_ldpc_decode_i8 only
        self.fixed = info.reserved in (15, 16)

    @property
    def handle(self):
        return self._h

    def reserve(self, max_batch: int, stream=None):
        """Pre-size `stream`'s workspace (default: torch's current stream)."""
        check(lib.pl_plan_reserve(self._h, int(max_batch), ctypes.c_void_p(_stream(stream))), "pl_plan_reserve")

    def release(self, stream=None):
        """Free `stream`'s workspace (default: torch's current stream)."""
        check(lib.pl_plan_release(self._h, ctypes.c_void_p(_stream(stream))), "pl_plan_release")

    def workspace_stats(self):
        """(streams with a workspace, their total bytes)."""
        n, b = ctypes.c_int64(), ctypes.c_int64()
        check(lib.pl_plan_workspace_stats(self._h, ctypes.byref(n), ctypes.byref(b)), "pl_plan_workspace_stats")
        return int(n.value), int(b.value)

    def small_batch_frames(self) -> int:
        """Largest batch decoded on the small-batch tree instance (0: none)."""
        b = ctypes.c_int64()
        check(lib.pl_polar_plan_small_batch(self._h, ctypes.byref(b)), "pl_polar_plan_small_batch")
        return int(b.value)

    def workspace_bytes(self, batch: int) -> int:
        b = ctypes.c_int64()
        check(lib.pl_plan_workspace_bytes(self._h, int(batch), ctypes.byref(b)), "pl_plan_workspace_bytes")
        return int(b.value)

    def _check(self, llr, bits, iters):
        # the kernels write bits at row pitch n_out and iters densely; llr rows
        # may carry any pitch >= n_in but unit inner stride
        assert isinstance(llr, torch.Tensor) and llr.is_cuda, "llr must be a device tensor"
        if self.fixed or llr.dtype == torch.int8:
            assert self.fixed and llr.dtype == torch.int8, "int8 llr and fixed-point plans go together only"
        elif llr.dtype == torch.float32:
            assert self.f32, "fp32 llr: quasi-cyclic plans created with PL_LDPC_QC_F32 only"
        else:
            assert llr.dtype == torch.float64
        assert llr.dim() == 2 and llr.stride(1) == 1 and llr.shape[1] >= self.info.n_in
        assert bits.is_cuda and bits.dtype == torch.uint8 and bits.shape == (llr.shape[0], self.info.n_out)
        assert bits.is_contiguous(), "bits must be contiguous [B, n_out] (row pitch n_out)"
        if iters is not None:
            assert iters.is_cuda and iters.dtype == torch.int32 and iters.shape == (llr.shape[0],) \
                and iters.is_contiguous(), "iters must be a contiguous int32 [B] device tensor"

    def decode(self, llr: "torch.Tensor", bits: "torch.Tensor", iters: "torch.Tensor | None" = None, stream=None,
               ws: "torch.Tensor | None" = None):
        """llr fp64 [B, >=n_in] device, bits uint8 [B, n_out] contiguous, iters int32 [B]
        or None; ws: optional caller-owned uint8 device workspace (pl_decode_ws).
        A PL_LDPC_QC_F32 plan also takes fp32 llr (pl_ldpc_decode_f32); a fixed-point
        plan takes int8 llr only (pl_ldpc_decode_i8)."""
        self._check(llr, bits, iters)
        assert ws is None or (ws.is_cuda and ws.is_contiguous())
        self._decode(llr, bits, iters, None, ws, stream)

    def _decode(self, llr, bits, iters, post, ws, stream):
        """The one call of each decode entry point, arguments already checked: fp32
        llr -> pl_ldpc_decode_f32 (post and ws optional), fp64 with post ->
        pl_ldpc_decode_soft, fp64 with ws -> pl_decode_ws, else pl_decode."""
        # addresses go as plain ints: the argtypes table makes them pointers (0 and None: NULL)
        head = (self._h, llr.data_ptr(), llr.shape[0], _ld(llr), bits.data_ptr(),
                iters.data_ptr() if iters is not None else None)
        soft = (None, 0) if post is None else (post.data_ptr(), _ld(post))
        work = (None, 0) if ws is None else (ws.data_ptr(), ws.numel() * ws.element_size())
        st = _stream(stream)
        if llr.dtype == torch.int8:
            check(lib.pl_ldpc_decode_i8(*head, *soft, *work, st), "pl_ldpc_decode_i8")
        elif llr.dtype == torch.float32:
            check(lib.pl_ldpc_decode_f32(*head, *soft, *work, st), "pl_ldpc_decode_f32")
        elif post is not None:
            check(lib.pl_ldpc_decode_soft(*head, *soft, st), "pl_ldpc_decode_soft")
        elif ws is not None:
            check(lib.pl_decode_ws(*head, *work, st), "pl_decode_ws")
        else:
            check(lib.pl_decode(*head, st), "pl_decode")

    def decode_soft(self, llr: "torch.Tensor", bits: "torch.Tensor", iters: "torch.Tensor | None",
                    post: "torch.Tensor", stream=None):
        """decode() of a layered min-sum plan that also writes the posterior LLRs:
        post fp64 [B, >=n] device with unit inner stride (pl_ldpc_decode_soft).
        Any other plan kind raises ValueError.  A PL_LDPC_QC_F32 plan also takes
        llr and post both fp32 (pl_ldpc_decode_f32)."""
        self._check(llr, bits, iters)
        assert post.is_cuda and post.dtype == llr.dtype and post.dim() == 2 and post.stride(1) == 1 \
            and post.shape[0] == llr.shape[0] and post.shape[1] >= self.info.n_in, \
            "post must be a [B, >=n] device tensor of llr's dtype (float64; float32 on a PL_LDPC_QC_F32 plan; " \
            "int8 on a fixed-point plan) with unit inner stride"
        self._decode(llr, bits, iters, post, None, stream)

    def decode_stamped(self, llr: "torch.Tensor", bits: "torch.Tensor", stamps: "torch.Tensor", stream=None):
        """Diagnostic decode accumulating per-phase cycle totals into stamps (int64 [5])."""
        check(lib.pl_debug_polar_stamps(self._h, ctypes.c_void_p(llr.data_ptr()), llr.shape[0], _ld(llr),
                                        _dptr(bits), _dptr(stamps), ctypes.c_void_p(_stream(stream))),
              "pl_debug_polar_stamps")

    def decode_fpw(self, llr: "torch.Tensor", bits: "torch.Tensor", stamps=None, grid: int = 0, stream=None):
        """Diagnostic: the frame-per-wavefront prototype (pl_debug_polar_fpw, N=1024 L=8)."""
        check(lib.pl_debug_polar_fpw(self._h, ctypes.c_void_p(llr.data_ptr()), llr.shape[0], _ld(llr),
                                     _dptr(bits), _dptr(stamps) if stamps is not None else None, int(grid),
                                     ctypes.c_void_p(_stream(stream))), "pl_debug_polar_fpw")

    def set_crc(self, crc_len: int, poly: int):
        """CRC-aided list selection (pl_polar_plan_set_crc); crc_len 0 = off."""
        check(lib.pl_polar_plan_set_crc(self._h, int(crc_len), ctypes.c_uint32(int(poly) & 0xFFFFFFFF)),
              "pl_polar_plan_set_crc")

    def close(self):
        if getattr(self, "_h", None):
            lib.pl_plan_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def polar_plan(N: int, K: int, frozen_mask: np.ndarray, list_size: int, flags: int = 0) -> Plan:
    require_gpu()
    mask = np.ascontiguousarray(frozen_mask, dtype=np.uint8)
    h = ctypes.c_void_p()
    check(lib.pl_polar_plan_create(int(N), int(K), mask.ctypes.data_as(ctypes.c_void_p), int(list_size),
                                   int(flags), ctypes.byref(h)), "pl_polar_plan_create")
    return Plan(h)


def ldpc_plan(row_ptr: np.ndarray, col_idx: np.ndarray, n: int, algo: int, max_iter: int, early_stop: bool,
              normalization: float = 1.0) -> Plan:
    require_gpu()
    rp = np.ascontiguousarray(row_ptr, dtype=np.int32)
    ci = np.ascontiguousarray(col_idx, dtype=np.int32)
    h = ctypes.c_void_p()
    check(lib.pl_ldpc_plan_create(len(rp) - 1, int(n), rp.ctypes.data_as(ctypes.c_void_p),
                                  ci.ctypes.data_as(ctypes.c_void_p), int(algo), int(max_iter),
                                  int(bool(early_stop)), float(normalization), 0, ctypes.byref(h)),
          "pl_ldpc_plan_create")
    return Plan(h)


def layered_ldpc_plan(row_ptr: np.ndarray, col_idx: np.ndarray, n: int, layers, max_iter: int, early_stop: bool,
                      normalization: float = 1.0) -> Plan:
    """Layered min-sum plan (pl_ldpc_layered_plan_create); layers: a sequence of
    row-index sequences, visited in that order."""
    rp = np.ascontiguousarray(row_ptr, dtype=np.int32)
    ci = np.ascontiguousarray(col_idx, dtype=np.int32)
    lp = np.zeros(len(layers) + 1, dtype=np.int32)
    lp[1:] = np.cumsum([len(l) for l in layers])
    lr = np.ascontiguousarray(np.concatenate([np.asarray(l, dtype=np.int32).ravel() for l in layers])
                              if len(layers) else np.zeros(0, np.int32), dtype=np.int32)
    require_gpu()
    h = ctypes.c_void_p()
    check(lib.pl_ldpc_layered_plan_create(len(rp) - 1, int(n), rp.ctypes.data_as(ctypes.c_void_p),
                                          ci.ctypes.data_as(ctypes.c_void_p), len(layers),
                                          lp.ctypes.data_as(ctypes.c_void_p), lr.ctypes.data_as(ctypes.c_void_p),
                                          int(max_iter), int(bool(early_stop)), float(normalization), 0,
                                          ctypes.byref(h)), "pl_ldpc_layered_plan_create")
    return Plan(h)


def qc_ldpc_plan(base: np.ndarray, Z: int, layer_order, max_iter: int, early_stop: bool,
                 normalization: float = 1.0, flags: int = 0) -> Plan:
    """Quasi-cyclic layered min-sum plan (pl_ldpc_qc_plan_create); base: int [mb, nb]
    shifts (-1: zero block); layer_order: a permutation of the block rows or None;
    flags: 0 or PL_LDPC_QC_F32."""
    sh = np.ascontiguousarray(base, dtype=np.int32)
    assert sh.ndim == 2, "base must be [mb, nb]"
    lo = None if layer_order is None else np.ascontiguousarray(layer_order, dtype=np.int32).ravel()
    assert lo is None or len(lo) == sh.shape[0], "layer_order must list the mb block rows"
    require_gpu()
    h = ctypes.c_void_p()
    check(lib.pl_ldpc_qc_plan_create(sh.shape[0], sh.shape[1], int(Z), sh.ctypes.data_as(ctypes.c_void_p),
                                     None if lo is None else lo.ctypes.data_as(ctypes.c_void_p), int(max_iter),
                                     int(bool(early_stop)), float(normalization), int(flags), ctypes.byref(h)),
          "pl_ldpc_qc_plan_create")
    return Plan(h)


def qc_fixed_ldpc_plan(base: np.ndarray, Z: int, layer_order, max_iter: int, early_stop: bool, norm16: int,
                       llr_max: int, msg_max: int) -> Plan:
    """int8 fixed-point quasi-cyclic layered min-sum plan (pl_ldpc_qc_fixed_plan_create); base and
    layer_order as qc_ldpc_plan's."""
    sh = np.ascontiguousarray(base, dtype=np.int32)
    assert sh.ndim == 2, "base must be [mb, nb]"
    lo = None if layer_order is None else np.ascontiguousarray(layer_order, dtype=np.int32).ravel()
    assert lo is None or len(lo) == sh.shape[0], "layer_order must list the mb block rows"
    require_gpu()
    h = ctypes.c_void_p()
    check(lib.pl_ldpc_qc_fixed_plan_create(sh.shape[0], sh.shape[1], int(Z), sh.ctypes.data_as(ctypes.c_void_p),
                                           None if lo is None else lo.ctypes.data_as(ctypes.c_void_p), int(max_iter),
                                           int(bool(early_stop)), int(norm16), int(llr_max), int(msg_max),
                                           ctypes.byref(h)), "pl_ldpc_qc_fixed_plan_create")
    return Plan(h)


def qc_bp_ldpc_plan(base: np.ndarray, Z: int, layer_order, max_iter: int, early_stop: bool, clip: float) -> Plan:
    """fp64 quasi-cyclic layered sum-product plan (pl_ldpc_qc_bp_plan_create); base and layer_order as
    qc_ldpc_plan's."""
    sh = np.ascontiguousarray(base, dtype=np.int32)
    assert sh.ndim == 2, "base must be [mb, nb]"
    lo = None if layer_order is None else np.ascontiguousarray(layer_order, dtype=np.int32).ravel()
    assert lo is None or len(lo) == sh.shape[0], "layer_order must list the mb block rows"
    require_gpu()
    h = ctypes.c_void_p()
    check(lib.pl_ldpc_qc_bp_plan_create(sh.shape[0], sh.shape[1], int(Z), sh.ctypes.data_as(ctypes.c_void_p),
                                        None if lo is None else lo.ctypes.data_as(ctypes.c_void_p), int(max_iter),
                                        int(bool(early_stop)), float(clip), ctypes.byref(h)),
          "pl_ldpc_qc_bp_plan_create")
    return Plan(h)


def llr_quantize(llr: "torch.Tensor", scale: float, llr_max: int, out: "torch.Tensor", stream=None):
    """pl_llr_quantize: llr float64 or float32 [B, >= n], out int8 [B, >= n] with n = out.shape[1]: device
    tensors (or views) with unit inner stride, any row pitch."""
    assert llr.dtype in (torch.float64, torch.float32) and out.dtype == torch.int8
    assert llr.dim() == 2 and out.dim() == 2 and llr.shape[0] == out.shape[0] and llr.shape[1] >= out.shape[1]
    if out.shape[0] == 0:
        return
    check(lib.pl_llr_quantize(_dptr(llr), PL_QUANT_LLR_F32 if llr.dtype == torch.float32 else 0, _ld(llr),
                              llr.shape[0], out.shape[1], float(scale), int(llr_max), _dptr(out), _ld(out),
                              _stream(stream)), "pl_llr_quantize")


class QcEncoder:
    """Owner of a pl_qc_encoder* (pl_ldpc_qc_encoder_create): the device stream of a
    base matrix of the encodable structure, bound to the device current at creation."""

    def __init__(self, handle: ctypes.c_void_p, k: int, n: int):
        self._h, self.k, self.n = handle, k, n

    @property
    def handle(self):
        return self._h

    def encode(self, msg: "torch.Tensor", cw: "torch.Tensor", stream=None):
        """msg uint8 [B, k], cw uint8 [B, n]: device tensors with unit inner stride, any row pitch."""
        assert msg.dtype == torch.uint8 and cw.dtype == torch.uint8 and msg.dim() == 2 and cw.dim() == 2
        assert msg.shape == (cw.shape[0], self.k) and cw.shape[1] == self.n
        if msg.shape[0] == 0:
            return
        check(lib.pl_ldpc_qc_encode(self._h, _dptr(msg), _ld(msg), msg.shape[0], _dptr(cw), _ld(cw),
                                    ctypes.c_void_p(_stream(stream))), "pl_ldpc_qc_encode")

    def close(self):
        if getattr(self, "_h", None):
            lib.pl_ldpc_qc_encoder_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def qc_encoder(base: np.ndarray, Z: int) -> QcEncoder:
    """pl_ldpc_qc_encoder_create; base: int [mb, nb] shifts (-1: zero block) of the encodable structure."""
    sh = np.ascontiguousarray(base, dtype=np.int32)
    assert sh.ndim == 2, "base must be [mb, nb]"
    require_gpu()
    h = ctypes.c_void_p()
    check(lib.pl_ldpc_qc_encoder_create(sh.shape[0], sh.shape[1], int(Z), sh.ctypes.data_as(ctypes.c_void_p),
                                        ctypes.byref(h)), "pl_ldpc_qc_encoder_create")
    return QcEncoder(h, (sh.shape[1] - sh.shape[0]) * int(Z), sh.shape[1] * int(Z))


def rate_match_probe(mb: int, nb: int, Z: int, punctured: int, fillers: int, ncb: int, start: int, E: int) -> RateMatch:
    """pl_debug_rate_match_probe: the checked parameters with the derived fields (no device call); ncb < 0:
    the default n - P.  AssertionError with the first violated condition."""
    rm = RateMatch()
    check(lib.pl_debug_rate_match_probe(int(mb), int(nb), int(Z), int(punctured), int(fillers), int(ncb), int(start),
                                        int(E), ctypes.byref(rm)), "pl_debug_rate_match_probe")
    return rm


def rate_match(rm: RateMatch, cw: "torch.Tensor", e: "torch.Tensor", stream=None):
    """pl_ldpc_rate_match: cw uint8 [B, >= n], e uint8 [B, >= E]: device tensors, unit inner stride, any row pitch."""
    check(lib.pl_ldpc_rate_match(ctypes.byref(rm), cw.data_ptr(), _ld(cw), cw.shape[0], e.data_ptr(), _ld(e),
                                 _stream(stream)), "pl_ldpc_rate_match")


def rate_recover(rm: RateMatch, llr: "torch.Tensor", out: "torch.Tensor", n_out: int, filler_llr: float,
                 accumulate: bool = False, stream=None):
    """pl_ldpc_rate_recover: llr [B, >= E], out [B, >= n_out], each float64 or float32 on the device."""
    flags = (PL_RM_LLR_F32 if llr.dtype == torch.float32 else 0) | (PL_RM_OUT_F32 if out.dtype == torch.float32 else 0) \
        | (PL_RM_ACCUMULATE if accumulate else 0)
    check(lib.pl_ldpc_rate_recover(ctypes.byref(rm), llr.data_ptr(), _ld(llr), llr.shape[0], out.data_ptr(), _ld(out),
                                   int(n_out), float(filler_llr), flags, _stream(stream)), "pl_ldpc_rate_recover")


def polar_rate_match_probe(N: int, E: int, mode: int, perm) -> PolarRateMatch:
    """pl_debug_polar_rate_match_probe: the checked parameters with the derived fields (no device call); perm:
    the sub-block permutation, nsub = len(perm) entries.  AssertionError with the first violated condition."""
    p = np.ascontiguousarray(perm, dtype=np.uint8).ravel()
    rm = PolarRateMatch()
    check(lib.pl_debug_polar_rate_match_probe(int(N), int(E), int(mode), len(p), p.ctypes.data_as(ctypes.c_void_p),
                                              ctypes.byref(rm)), "pl_debug_polar_rate_match_probe")
    return rm


def polar_rate_match_forced(rm: PolarRateMatch) -> np.ndarray:
    """pl_polar_rate_match_forced: uint8 [N], 1 where u_j must be frozen (no device call)."""
    mask = np.zeros(rm.N, dtype=np.uint8)
    check(lib.pl_polar_rate_match_forced(ctypes.byref(rm), mask.ctypes.data_as(ctypes.c_void_p)),
          "pl_polar_rate_match_forced")
    return mask


def polar_rate_match(rm: PolarRateMatch, cw: "torch.Tensor", e: "torch.Tensor", stream=None):
    """pl_polar_rate_match: cw uint8 [B, >= N], e uint8 [B, >= E]: device tensors, unit inner stride, any row pitch."""
    check(lib.pl_polar_rate_match(ctypes.byref(rm), cw.data_ptr(), _ld(cw), cw.shape[0], e.data_ptr(), _ld(e),
                                  _stream(stream)), "pl_polar_rate_match")


def polar_rate_recover(rm: PolarRateMatch, llr: "torch.Tensor", out: "torch.Tensor", known_llr: float,
                       accumulate: bool = False, stream=None):
    """pl_polar_rate_recover: llr float64 or float32 [B, >= E], out float64 [B, >= N] on the device."""
    flags = (PL_PRM_LLR_F32 if llr.dtype == torch.float32 else 0) | (PL_PRM_ACCUMULATE if accumulate else 0)
    check(lib.pl_polar_rate_recover(ctypes.byref(rm), llr.data_ptr(), _ld(llr), llr.shape[0], out.data_ptr(), _ld(out),
                                    float(known_llr), flags, _stream(stream)), "pl_polar_rate_recover")


def qam_check(m: int, E: int):
    """pl_qam_check: (S, scale) of m bits per symbol and E transmitted bits (no device call).
    AssertionError with the first violated condition."""
    S, scale = ctypes.c_int64(), ctypes.c_double()
    check(lib.pl_qam_check(int(m), int(E), ctypes.byref(S), ctypes.byref(scale)), "pl_qam_check")
    return int(S.value), float(scale.value)


def qam_modulate(m: int, E: int, e: "torch.Tensor", x: "torch.Tensor", stream=None):
    """pl_qam_modulate: e uint8 [B, >= E], x float64 [B, >= 2 S]: device tensors, unit inner stride, any row pitch."""
    check(lib.pl_qam_modulate(int(m), int(E), e.shape[0], e.data_ptr(), _ld(e), x.data_ptr(), _ld(x), _stream(stream)),
          "pl_qam_modulate")


def qam_awgn(m: int, E: int, e: "torch.Tensor | None", snr_db: float, seed: int, frame_offset: int, y: "torch.Tensor",
             stream=None):
    """pl_qam_awgn: e uint8 [B, >= E] or None (all-zero bits), y float64 [B, >= 2 S] on the device."""
    check(lib.pl_qam_awgn(int(m), int(E), y.shape[0], None if e is None else e.data_ptr(), 0 if e is None else _ld(e),
                          float(snr_db), ctypes.c_uint64(seed & (2**64 - 1)), int(frame_offset), y.data_ptr(), _ld(y),
                          _stream(stream)), "pl_qam_awgn")


def qam_demap(m: int, E: int, y: "torch.Tensor", snr_db: float, llr: "torch.Tensor", stream=None, logmap: bool = False):
    """pl_qam_demap, or with logmap pl_qam_demap_logmap: y float64 [B, >= 2 S], llr float64 or float32 [B, >= E] on
    the device."""
    name = "pl_qam_demap_logmap" if logmap else "pl_qam_demap"
    check(getattr(lib, name)(int(m), int(E), y.shape[0], y.data_ptr(), _ld(y), float(snr_db), llr.data_ptr(), _ld(llr),
                             PL_QAM_LLR_F32 if llr.dtype == torch.float32 else 0, _stream(stream)), name)


def qam_fading_check(m: int, E: int, coherence: int):
    """pl_qam_fading_check: (S, Q) of m bits per symbol, E transmitted bits and a coherence length in symbols
    (no device call).  AssertionError with the first violated condition."""
    S, Q = ctypes.c_int64(), ctypes.c_int64()
    check(lib.pl_qam_fading_check(int(m), int(E), int(coherence), ctypes.byref(S), ctypes.byref(Q)),
          "pl_qam_fading_check")
    return int(S.value), int(Q.value)


def qam_rayleigh(m: int, E: int, coherence: int, e: "torch.Tensor | None", snr_db: float, seed: int, frame_offset: int,
                 y: "torch.Tensor", h: "torch.Tensor", stream=None):
    """pl_qam_rayleigh: e uint8 [B, >= E] or None (all-zero bits), y float64 [B, >= 2 S], h float64 [B, >= 2 Q]
    on the device."""
    check(lib.pl_qam_rayleigh(int(m), int(E), int(coherence), y.shape[0], None if e is None else e.data_ptr(),
                              0 if e is None else _ld(e), float(snr_db), ctypes.c_uint64(seed & (2**64 - 1)),
                              int(frame_offset), y.data_ptr(), _ld(y), h.data_ptr(), _ld(h), _stream(stream)),
          "pl_qam_rayleigh")


def qam_demap_csi(m: int, E: int, coherence: int, y: "torch.Tensor", h: "torch.Tensor", snr_db: float,
                  llr: "torch.Tensor", stream=None, logmap: bool = False):
    """pl_qam_demap_csi, or with logmap pl_qam_demap_csi_logmap: y float64 [B, >= 2 S], h float64 [B, >= 2 Q], llr
    float64 or float32 [B, >= E] on the device."""
    name = "pl_qam_demap_csi_logmap" if logmap else "pl_qam_demap_csi"
    check(getattr(lib, name)(int(m), int(E), int(coherence), y.shape[0], y.data_ptr(), _ld(y), h.data_ptr(), _ld(h),
                             float(snr_db), llr.data_ptr(), _ld(llr),
                             PL_QAM_LLR_F32 if llr.dtype == torch.float32 else 0, _stream(stream)), name)


# the largest E the interleaver kernels permute in LDS, by element size in bytes; longer frames go the direct way
ILV_LDS_MAX_E = {size: int(lib.pl_interleave_lds_max_e(size)) for size in (1, 4, 8)}


def interleave_check(kind: int, rows: int, E: int) -> int:
    """pl_interleave_check: C (PL_ILV_RECT) or T (PL_ILV_TRI) of the interleaver (no device call).
    AssertionError with the first violated condition."""
    dim = ctypes.c_int64()
    check(lib.pl_interleave_check(int(kind), int(rows), int(E), ctypes.byref(dim)), "pl_interleave_check")
    return int(dim.value)


def interleave_index(kind: int, rows: int, E: int, k: int) -> int:
    """pl_interleave_index: pos(k) by the code the kernels run (no device call)."""
    pos = ctypes.c_int64()
    check(lib.pl_interleave_index(int(kind), int(rows), int(E), int(k), ctypes.byref(pos)), "pl_interleave_index")
    return int(pos.value)


def bit_interleave(kind: int, rows: int, E: int, e: "torch.Tensor", f: "torch.Tensor", stream=None):
    """pl_bit_interleave: e, f uint8 [B, >= E]: device tensors, unit inner stride, any row pitch."""
    check(lib.pl_bit_interleave(int(kind), int(rows), int(E), e.shape[0], e.data_ptr(), _ld(e), f.data_ptr(), _ld(f),
                                _stream(stream)), "pl_bit_interleave")


def llr_deinterleave(kind: int, rows: int, E: int, f: "torch.Tensor", e: "torch.Tensor", stream=None):
    """pl_llr_deinterleave: f, e [B, >= E] on the device, both float64 or both float32."""
    check(lib.pl_llr_deinterleave(int(kind), int(rows), int(E), f.shape[0], f.data_ptr(), _ld(f), e.data_ptr(), _ld(e),
                                  PL_ILV_LLR_F32 if f.dtype == torch.float32 else 0, _stream(stream)),
          "pl_llr_deinterleave")


def random_bits(seed: int, frame_offset: int, bits: "torch.Tensor", stream=None):
    B, k = bits.shape
    check(lib.pl_random_bits(ctypes.c_uint64(seed & (2**64 - 1)), int(frame_offset), B, k, _dptr(bits),
                             ctypes.c_void_p(_stream(stream))), "pl_random_bits")


def polar_encode(plan: Plan, msg: "torch.Tensor", codeword: "torch.Tensor", stream=None):
    check(lib.pl_polar_encode(plan.handle, _dptr(msg), msg.shape[0], _dptr(codeword),
                              ctypes.c_void_p(_stream(stream))), "pl_polar_encode")


def awgn_llr(codeword: "torch.Tensor | None", n: int, batch: int, snr_db: float, seed: int, frame_offset: int,
             llr: "torch.Tensor", stream=None):
    cw = _dptr(codeword) if codeword is not None else None
    check(lib.pl_awgn_llr(cw, int(n), int(batch), float(snr_db), ctypes.c_uint64(seed & (2**64 - 1)),
                          int(frame_offset), _dptr(llr), _ld(llr), ctypes.c_void_p(_stream(stream))),
          "pl_awgn_llr")


def count_errors(ref: "torch.Tensor", dec: "torch.Tensor", width: int, counts: "torch.Tensor", stream=None):
    check(lib.pl_count_errors(_dptr(ref), _ld(ref), _dptr(dec), _ld(dec), int(width), ref.shape[0],
                              _dptr(counts), ctypes.c_void_p(_stream(stream))), "pl_count_errors")


def crc_append(msg: "torch.Tensor", k_data: int, crc_len: int, poly: int, stream=None):
    """msg uint8 [B, >= k_data+crc_len]: write the CRC bits of msg[:, :k_data] after them."""
    check(lib.pl_crc_append(_dptr(msg), _ld(msg), msg.shape[0], int(k_data), int(crc_len),
                            ctypes.c_uint32(int(poly) & 0xFFFFFFFF), ctypes.c_void_p(_stream(stream))),
          "pl_crc_append")


def rayleigh_llr(codeword, n: int, batch: int, snr_db: float, seed: int, frame_offset: int, llr, stream=None):
    cw = _dptr(codeword) if codeword is not None else None
    check(lib.pl_rayleigh_llr(cw, int(n), int(batch), float(snr_db), ctypes.c_uint64(seed & (2**64 - 1)),
                              int(frame_offset), _dptr(llr), _ld(llr), ctypes.c_void_p(_stream(stream))),
          "pl_rayleigh_llr")


def bsc(codeword, n: int, batch: int, crossover_prob: float, seed: int, frame_offset: int, out, stream=None):
    cw = _dptr(codeword) if codeword is not None else None
    check(lib.pl_bsc(cw, int(n), int(batch), float(crossover_prob), ctypes.c_uint64(seed & (2**64 - 1)),
                     int(frame_offset), _dptr(out), _ld(out), ctypes.c_void_p(_stream(stream))), "pl_bsc")


def gf2_encode(g_packed: "torch.Tensor", k: int, n: int, msg: "torch.Tensor", cw: "torch.Tensor", stream=None):
    """cw = msg . G (GF(2)); g_packed int32 [ceil(k/32), n] device (pack_gf2_columns)."""
    assert g_packed.dtype == torch.int32 and g_packed.is_contiguous() and g_packed.shape == ((k + 31) // 32, n)
    check(lib.pl_gf2_encode(_dptr(g_packed), int(k), int(n), _dptr(msg), _ld(msg), msg.shape[0], _dptr(cw), _ld(cw),
                            ctypes.c_void_p(_stream(stream))), "pl_gf2_encode")


def pack_gf2_columns(G: np.ndarray) -> np.ndarray:
    """k x n 0/1 matrix -> int32 [ceil(k/32), n]: bit i of [w, j] = G[32 w + i, j]."""
    G = (np.asarray(G) & 1).astype(np.uint64)
    k, n = G.shape
    kw = (k + 31) // 32
    Gp = np.zeros((kw * 32, n), np.uint64)
    Gp[:k] = G
    w = (Gp.reshape(kw, 32, n) << np.arange(32, dtype=np.uint64)[None, :, None]).sum(axis=1)
    return w.astype(np.uint32).view(np.int32)

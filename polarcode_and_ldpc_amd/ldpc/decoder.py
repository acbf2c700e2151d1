"""Drop-in BPDecoder / MSDecoder backed by the gfx950 HIP kernel (ldpc.hip).

Same constructors, attributes and `.decode(llr)` contract as the reference's
src/ldpc/decoder.py (BPDecoder :11-205, MSDecoder :208-355), plus
`decode_batch` for host or device batches.  No CPU path.
LayeredMSDecoder (ldpc_layered.hip) is a build-defined extension: the serial
schedule with posterior LLR output; QCLayeredMSDecoder (ldpc_qc_layered.hip) is
the same decoder for a quasi-cyclic code given by its base matrix, and
QCFixedMSDecoder (ldpc_qc_fixed.hip) its int8 fixed-point counterpart;
QCLayeredBPDecoder (ldpc_qc_bp.hip) is the sum-product decoder on the same schedule.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from .. import _native
from .matrix import dense_to_csr, layer_schedule, qc_block_layers, qc_expand

_TORCH = {np.float64: torch.float64, np.float32: torch.float32, np.int8: torch.int8}


class _LdpcBase:
    _algo = _native.PL_LDPC_BP
    normalization = 1.0

    def _setup(self, H, max_iter, early_stop):
        self.H = H
        self.m, self.n = H.shape
        self.max_iter = max_iter
        self.early_stop = early_stop
        self._row_ptr, self._col_idx = dense_to_csr(H)  # entries == 1, ascending (decoder.py:43-47)
        deg = np.diff(self._row_ptr)
        self.check_degrees = deg
        self.var_neighbors = None  # the reference's Python adjacency lists are not materialised
        self._plan = None

    @property
    def plan(self):
        if self._plan is None:
            self._plan = _native.ldpc_plan(self._row_ptr, self._col_idx, self.n, self._algo, self.max_iter,
                                           self.early_stop, self.normalization)
        return self._plan

    # What a subclass may change about decode_batch, which has this one body:
    _elem = np.float64  # element type of the decoder's state, host LLRs and posteriors
    _soft_output = False  # decode_batch(return_llr=True) exists: the layered classes
    # The layered classes write the bits into a host `out` and check runnability on an empty host
    # batch; the flooding ones (BP, MS) do neither.  Nobody chose the difference; it is kept.
    _host_out = False

    def _check_runnable(self):
        pass

    def _device_llr(self, llr):
        """A CUDA [B, n] tensor as the kernels read it: fp64, unit inner stride, any row pitch."""
        if llr.dtype != torch.float64 or llr.stride(1) != 1:
            llr = llr.to(torch.float64).contiguous()
        return llr

    def _host_llr(self, llr):
        return np.asarray(llr, dtype=np.float64)

    def _run(self, llr, out=None, soft=False):
        """Device batch, no host copy and no synchronise: llr [B, >=n] as _device_llr
        leaves it -> (bits uint8 [B, n], iters int32 [B], posterior [B, n] or None)."""
        self._check_runnable()  # deliberate: an empty device batch is checked too
        B, dev = llr.shape[0], llr.device
        if out is None:
            out = torch.empty((B, self.n), dtype=torch.uint8, device=dev)
        # deliberate: allocated, and handed to the kernel, whether the caller asked for iterations or not
        iters = torch.empty((B,), dtype=torch.int32, device=dev)
        post = torch.empty((B, self.n), dtype=_TORCH[self._elem], device=dev) if soft else None
        if B == 0:
            pass  # deliberate: no library call, not even the plan's creation
        elif post is None:
            self.plan.decode(llr, out, iters)
        else:
            # a float32 decoder given fp64 LLRs: the fp64-I/O instance writes the float32 posteriors
            # widened to an fp64 buffer, which rounds back exactly (the class docstring)
            wide = post if post.dtype == llr.dtype else torch.empty((B, self.n), dtype=llr.dtype, device=dev)
            self.plan.decode_soft(llr, out, iters, wide)
            if wide is not post:
                post.copy_(wide)
        return out, iters, post

    def decode_batch(self, llr, out: Optional[torch.Tensor] = None, return_iterations: bool = False,
                     return_llr: bool = False):
        """Bits [B, n]; with return_iterations / return_llr (the layered classes
        only) also the iteration counts and the posterior LLRs, in the order bits,
        iterations, posterior.  A CUDA tensor in gives CUDA tensors out (no host
        copy; `out`: a uint8 [B, n] device tensor for the bits); NumPy in gives
        int64 / float NumPy out (`out`, layered classes only: an int64 [B, n]
        array for the bits)."""
        if return_llr and not self._soft_output:
            raise TypeError("decode_batch() got an unexpected keyword argument 'return_llr'")

        def pick(bits, its, post):  # deliberate: a bare array, not a 1-tuple, when only the bits are asked for
            r = (bits,) + ((its,) if return_iterations else ()) + ((post,) if return_llr else ())
            return r if len(r) > 1 else bits

        if isinstance(llr, torch.Tensor) and llr.is_cuda:
            assert llr.dim() == 2 and llr.shape[1] == self.n, "LLR length must be %d" % self.n
            return pick(*self._run(self._device_llr(llr), out, return_llr))
        a = self._host_llr(llr.cpu().numpy() if isinstance(llr, torch.Tensor) else llr)
        assert a.ndim == 2 and a.shape[1] == self.n, "LLR length must be %d" % self.n
        if not self._host_out:
            out = None  # deliberate (BP, MS): a host `out` is ignored, a fresh int64 array comes back
        if a.shape[0] == 0:
            if self._host_out:
                self._check_runnable()  # deliberate: BP / MS return the empty result unchecked
            bits = np.zeros((0, self.n), dtype=np.int64) if out is None else out  # deliberate: `out` itself
            return pick(bits, np.zeros(0, dtype=np.int64), np.zeros((0, self.n), dtype=self._elem))
        _native.require_gpu()
        bits, its, post = self._run(torch.from_numpy(np.ascontiguousarray(a)).cuda(), None, return_llr)
        if post is not None:
            post = post.cpu().numpy()
        b = bits.cpu().numpy().astype(np.int64)
        if out is not None:
            out[...] = b
            b = out
        return pick(b, its.cpu().numpy().astype(np.int64), post)


class BPDecoder(_LdpcBase):
    """Flooding sum-product decoder (src/ldpc/decoder.py:11-205)."""

    def __init__(self, H: np.ndarray, max_iter: int = 50, early_stop: bool = True):
        self._algo = _native.PL_LDPC_BP
        self._setup(H, max_iter, early_stop)

    def decode(self, llr: np.ndarray, return_iterations: bool = False):
        assert len(llr) == self.n, f"LLR length must be {self.n}"
        bits, its = self.decode_batch(np.asarray(llr, dtype=np.float64)[None, :], return_iterations=True)
        if return_iterations:
            return bits[0], int(its[0])
        return bits[0]

    def __repr__(self) -> str:
        return f"BPDecoder(n={self.n}, m={self.m}, max_iter={self.max_iter})"


class MSDecoder(_LdpcBase):
    """(Normalised) min-sum decoder (src/ldpc/decoder.py:208-355)."""

    def __init__(self, H: np.ndarray, max_iter: int = 50, normalization: float = 1.0, early_stop: bool = True):
        self._algo = _native.PL_LDPC_MS
        self.normalization = normalization
        self._setup(H, max_iter, early_stop)

    def _check_runnable(self):
        # the reference evaluates np.min over the other inputs of every check;
        # a degree-1 check makes that an empty reduction (decoder.py:282)
        if self.max_iter > 0 and np.any(self.check_degrees == 1):
            raise ValueError("zero-size array to reduction operation minimum which has no identity")

    def decode(self, llr: np.ndarray) -> np.ndarray:
        assert len(llr) == self.n, f"LLR length must be {self.n}"
        return self.decode_batch(np.asarray(llr, dtype=np.float64)[None, :])[0]

    def __repr__(self) -> str:
        return f"MSDecoder(n={self.n}, m={self.m}, max_iter={self.max_iter}, norm={self.normalization})"


class LayeredMSDecoder(_LdpcBase):
    """Layered (row-serial) normalised min-sum decoder with posterior LLR output
    (ldpc_layered.hip).  Build-defined: the reference has flooding decoders only.

    The rows of H are visited layer by layer, each check updating the posteriors
    of its variables at once (MSDecoder's check rule on q = P - R), which
    converges in about half the iterations of the flooding schedule.  `layers`:
    a sequence of row-index sequences that lists every row once and whose rows
    share no column within a layer (default: layer_schedule(H));
    `[[c] for c in range(m)]` is the classic serial schedule."""

    _soft_output = True
    _host_out = True

    def __init__(self, H: np.ndarray, max_iter: int = 50, normalization: float = 1.0, early_stop: bool = True,
                 layers=None):
        self._algo = _native.PL_LDPC_LMS
        self.normalization = normalization
        self._setup(H, max_iter, early_stop)
        self.layers = [np.asarray(l, dtype=np.int64).ravel() for l in (layer_schedule(H) if layers is None else layers)]

    @property
    def plan(self):
        if self._plan is None:
            self._plan = _native.layered_ldpc_plan(self._row_ptr, self._col_idx, self.n, self.layers, self.max_iter,
                                                   self.early_stop, self.normalization)
        return self._plan

    def _check_runnable(self):
        # as MSDecoder: np.min over the other inputs of a degree-1 check is an empty reduction
        if self.max_iter > 0 and np.any(self.check_degrees == 1):
            raise ValueError("zero-size array to reduction operation minimum which has no identity")

    def decode(self, llr: np.ndarray, return_iterations: bool = False):
        assert len(llr) == self.n, f"LLR length must be {self.n}"
        bits, its = self.decode_batch(np.asarray(llr, dtype=np.float64)[None, :], return_iterations=True)
        if return_iterations:
            return bits[0], int(its[0])
        return bits[0]

    def __repr__(self) -> str:
        return (f"LayeredMSDecoder(n={self.n}, m={self.m}, max_iter={self.max_iter}, norm={self.normalization}, "
                f"layers={len(self.layers)})")


def _qc_state_dtype(dtype):
    """np.float64 or np.float32 from a NumPy / torch dtype or its name; anything else: ValueError."""
    if isinstance(dtype, torch.dtype):
        dtype = {torch.float64: np.float64, torch.float32: np.float32}.get(dtype, dtype)
    try:
        name = None if dtype is None else np.dtype(dtype).name
    except TypeError:
        name = None
    if name not in ("float64", "float32"):
        raise ValueError("QCLayeredMSDecoder: dtype must be float64 or float32, not %r" % (dtype,))
    return np.float64 if name == "float64" else np.float32


class QCLayeredMSDecoder(LayeredMSDecoder):
    """LayeredMSDecoder for a quasi-cyclic code given by its base matrix
    (ldpc_qc_layered.hip).  `base`: int [mb, nb], -1 a zero Z x Z block, s in
    0 .. Z-1 the identity shifted cyclically by s (qc_expand).  The layers are
    the block rows, visited in `layer_order` (default 0 .. mb-1).  By definition
    equal, bit for bit, to LayeredMSDecoder(qc_expand(base, Z),
    layers=qc_block_layers(mb, Z, layer_order)); H is never expanded unless `.H`
    is read.

    `dtype`: np.float64 (default) or np.float32 (also torch.float32, "float32").
    A float32 decoder is the same definition with every value and operation in
    IEEE binary32 (include/polarldpc.h, PL_LDPC_QC_F32): half the state, and
    fp32 or fp64 device LLRs are read as they are, with no conversion pass on
    the input.  Its results equal a NumPy float32 restatement bit for bit; they
    are not the float64 decoder's rounded.  Posteriors come back as float32;
    for fp64 device LLRs with return_llr the kernel writes them widened to an
    fp64 [B, n] buffer that is then narrowed (exact), one extra pass and three
    times the posterior bytes -- pass fp32 LLRs where the posteriors matter."""

    def __init__(self, base: np.ndarray, Z: int, max_iter: int = 50, normalization: float = 1.0,
                 early_stop: bool = True, layer_order=None, dtype=np.float64):
        self._algo = _native.PL_LDPC_LMS
        self.dtype = _qc_state_dtype(dtype)
        self.base = np.array(base, dtype=np.int64)
        assert self.base.ndim == 2, "base must be [mb, nb]"
        self.Z = int(Z)
        self.mb, self.nb = self.base.shape
        self.m, self.n = self.mb * self.Z, self.nb * self.Z
        self.max_iter = max_iter
        self.early_stop = early_stop
        self.normalization = normalization
        self.layer_order = None if layer_order is None else [int(i) for i in layer_order]
        self.check_degrees = np.repeat((self.base >= 0).sum(axis=1), self.Z)
        self.var_neighbors = None
        self._plan = None
        self._H = None

    @property
    def H(self):
        if self._H is None:
            self._H = qc_expand(self.base, self.Z)
        return self._H

    @property
    def layers(self):
        return qc_block_layers(self.mb, self.Z, self.layer_order)

    @property
    def plan(self):
        if self._plan is None:
            self._plan = _native.qc_ldpc_plan(self.base, self.Z, self.layer_order, self.max_iter, self.early_stop,
                                              self.normalization,
                                              _native.PL_LDPC_QC_F32 if self.dtype == np.float32 else 0)
        return self._plan

    # The dtype policy: what a float32 decoder changes about decode_batch.
    @property
    def _elem(self):
        return self.dtype

    def _device_llr(self, llr):
        """float32 decoder: fp32 and fp64 tensors are read as they are (unit inner
        stride, any row pitch); any other dtype is converted with .to(torch.float32)."""
        if self.dtype != np.float32:
            return super()._device_llr(llr)
        if llr.dtype not in (torch.float32, torch.float64):
            llr = llr.to(torch.float32)
        return llr if llr.stride(1) == 1 else llr.contiguous()

    def _host_llr(self, llr):
        if self.dtype != np.float32:
            return super()._host_llr(llr)
        with np.errstate(all="ignore"):  # beyond FLT_MAX: +-inf, by definition
            return np.asarray(llr).astype(np.float32)

    def __repr__(self) -> str:
        return (f"QCLayeredMSDecoder(n={self.n}, m={self.m}, Z={self.Z}, max_iter={self.max_iter}, "
                f"norm={self.normalization}" + (", dtype=float32)" if self.dtype == np.float32 else ")"))


def quantize_host(llr, scale: float, llr_max: int) -> np.ndarray:
    """The LLR quantiser of the fixed-point decoder on the host (include/polarldpc.h, pl_llr_quantize):
    clamp(rint(double(llr) * scale), -llr_max, llr_max) as int8, rint half to even, NaN -> 0, +-inf ->
    +-llr_max.  float64 and float32 (widened exactly) as they are; any other dtype through float64."""
    a = np.asarray(llr)
    if a.dtype not in (np.float64, np.float32):
        a = a.astype(np.float64)
    assert np.isfinite(scale) and scale > 0 and 1 <= llr_max <= 127
    with np.errstate(invalid="ignore", over="ignore"):
        x = np.rint(a.astype(np.float64) * np.float64(scale))
    return np.clip(np.where(np.isnan(x), 0.0, x), -float(llr_max), float(llr_max)).astype(np.int8)


class QCFixedMSDecoder(LayeredMSDecoder):
    """int8 fixed-point layered normalised min-sum for a quasi-cyclic code given by
    its base matrix (ldpc_qc_fixed.hip).  `base`, `Z` and `layer_order` as
    QCLayeredMSDecoder's.  The definition -- integer arithmetic with three
    saturation bounds, exactly reproducible -- is printed in include/polarldpc.h at
    pl_ldpc_qc_fixed_plan_create: posteriors saturate at 127, channel LLRs at
    `llr_max`, check-to-variable messages at `msg_max`, and the normalisation is
    `normalization` = norm16 / 16 with norm16 an integer in 1 .. 16 (ValueError
    otherwise).

    decode / decode_batch take int8 LLRs (NumPy arrays, or CUDA tensors with any row
    pitch) as they are, and floating LLRs through the quantiser
    L = clamp(rint(llr * llr_scale), -llr_max, llr_max): CUDA tensors through the
    device kernel (fp64 and fp32 as they are, other floating types through fp32),
    NumPy arrays through quantize_host and one upload.  return_llr gives the final
    int8 posteriors."""

    _elem = np.int8

    def __init__(self, base: np.ndarray, Z: int, max_iter: int = 50, normalization: float = 0.75,
                 early_stop: bool = True, layer_order=None, llr_scale: float = 4.0, llr_max: int = 31,
                 msg_max: int = 31):
        n16 = float(normalization) * 16.0
        if n16 != int(n16) or not 1 <= int(n16) <= 16:
            raise ValueError("QCFixedMSDecoder: normalization * 16 must be an integer in 1 .. 16, not %r" % (n16,))
        if not (np.isfinite(llr_scale) and llr_scale > 0):
            raise ValueError("QCFixedMSDecoder: llr_scale must be finite and > 0, not %r" % (llr_scale,))
        self._algo = _native.PL_LDPC_LMS
        self.base = np.array(base, dtype=np.int64)
        assert self.base.ndim == 2, "base must be [mb, nb]"
        self.Z = int(Z)
        self.mb, self.nb = self.base.shape
        self.m, self.n = self.mb * self.Z, self.nb * self.Z
        self.max_iter = max_iter
        self.early_stop = early_stop
        self.normalization = normalization
        self.norm16 = int(n16)
        self.llr_scale, self.llr_max, self.msg_max = float(llr_scale), int(llr_max), int(msg_max)
        self.layer_order = None if layer_order is None else [int(i) for i in layer_order]
        self.check_degrees = np.repeat((self.base >= 0).sum(axis=1), self.Z)
        self.var_neighbors = None
        self._plan = None
        self._H = None

    H = QCLayeredMSDecoder.H
    layers = QCLayeredMSDecoder.layers

    @property
    def plan(self):
        if self._plan is None:
            self._plan = _native.qc_fixed_ldpc_plan(self.base, self.Z, self.layer_order, self.max_iter,
                                                    self.early_stop, self.norm16, self.llr_max, self.msg_max)
        return self._plan

    def quantize_host(self, llr) -> np.ndarray:
        return quantize_host(llr, self.llr_scale, self.llr_max)

    def quantize(self, llr: "torch.Tensor", out: Optional[torch.Tensor] = None) -> "torch.Tensor":
        """A floating CUDA tensor [B, >= n] (unit inner stride, any row pitch) -> int8 [B, n] on the device
        (pl_llr_quantize); `out`: an int8 [B, n] device tensor or view to write into."""
        if not llr.dtype.is_floating_point:
            raise TypeError("QCFixedMSDecoder: LLRs must be int8 or floating, not %s" % (llr.dtype,))
        if llr.dtype not in (torch.float64, torch.float32):
            llr = llr.to(torch.float32)  # exact for the narrower floating types
        if llr.stride(1) != 1:
            llr = llr.contiguous()
        if out is None:
            out = torch.empty((llr.shape[0], self.n), dtype=torch.int8, device=llr.device)
        _native.llr_quantize(llr, self.llr_scale, self.llr_max, out)
        return out

    def _device_llr(self, llr):
        if llr.dtype != torch.int8:
            return self.quantize(llr)
        return llr if llr.stride(1) == 1 else llr.contiguous()

    def _host_llr(self, llr):
        a = np.asarray(llr)
        if a.dtype == np.int8:
            return a
        if not np.issubdtype(a.dtype, np.floating):
            raise TypeError("QCFixedMSDecoder: LLRs must be int8 or floating, not %s" % (a.dtype,))
        return self.quantize_host(a)

    def decode(self, llr: np.ndarray, return_iterations: bool = False):
        assert len(llr) == self.n, f"LLR length must be {self.n}"
        bits, its = self.decode_batch(np.asarray(llr)[None, :], return_iterations=True)
        if return_iterations:
            return bits[0], int(its[0])
        return bits[0]

    def __repr__(self) -> str:
        return (f"QCFixedMSDecoder(n={self.n}, m={self.m}, Z={self.Z}, max_iter={self.max_iter}, "
                f"norm={self.norm16}/16, llr_scale={self.llr_scale}, llr_max={self.llr_max}, msg_max={self.msg_max})")


class QCLayeredBPDecoder(LayeredMSDecoder):
    """Layered sum-product (belief propagation) decoder for a quasi-cyclic code given
    by its base matrix (ldpc_qc_bp.hip), fp64.  `base`, `Z` and `layer_order`, the
    schedule, the stop rule and the hard decision as QCLayeredMSDecoder's; the check
    rule is the exact box-plus, evaluated as a forward / backward recursion with
    glibc's expm1 and log1p, and every variable-to-check message is clamped to
    +-`clip` (finite, 0 < clip <= 2**20; ValueError otherwise).  The definition is
    printed in include/polarldpc.h at pl_ldpc_qc_bp_plan_create; bits, iteration
    counts and posteriors equal a NumPy restatement of it bit for bit.  NaN LLRs are
    erasures and +-inf are +-clip, so every posterior is finite
    (|P| <= 2 clip + ln 2)."""

    def __init__(self, base: np.ndarray, Z: int, max_iter: int = 50, early_stop: bool = True, layer_order=None,
                 clip: float = 64.0):
        clip = float(clip)
        if not 0.0 < clip <= 2.0 ** 20:  # a NaN fails the comparison
            raise ValueError("QCLayeredBPDecoder: clip must be finite with 0 < clip <= 2**20, not %r" % (clip,))
        self._algo = _native.PL_LDPC_LMS
        self.base = np.array(base, dtype=np.int64)
        assert self.base.ndim == 2, "base must be [mb, nb]"
        self.Z = int(Z)
        self.mb, self.nb = self.base.shape
        self.m, self.n = self.mb * self.Z, self.nb * self.Z
        self.max_iter = max_iter
        self.early_stop = early_stop
        self.clip = clip
        self.layer_order = None if layer_order is None else [int(i) for i in layer_order]
        self.check_degrees = np.repeat((self.base >= 0).sum(axis=1), self.Z)
        self.var_neighbors = None
        self._plan = None
        self._H = None

    H = QCLayeredMSDecoder.H
    layers = QCLayeredMSDecoder.layers

    @property
    def plan(self):
        if self._plan is None:
            self._plan = _native.qc_bp_ldpc_plan(self.base, self.Z, self.layer_order, self.max_iter, self.early_stop,
                                                 self.clip)
        return self._plan

    def _check_runnable(self):
        if self.max_iter > 0 and np.any(self.check_degrees == 1):
            raise ValueError("sum-product on a degree-1 check: the box-plus of no input")

    def __repr__(self) -> str:
        return (f"QCLayeredBPDecoder(n={self.n}, m={self.m}, Z={self.Z}, max_iter={self.max_iter}, "
                f"clip={self.clip})")

"""Bit interleaver between rate matching and the QAM modem.

BitInterleaver(kind, E, rows) spreads a rate matcher's E transmitted bits over the
unequally reliable bit positions of the QAM symbols and brings the E received LLRs
back into the rate matcher's order: "rect", a row-column interleaver (rows = the
modem's bits per symbol puts bit r of symbol s at e[r C + s]), or "tri", an
isosceles-triangular one.  The definition is stated once, in include/polarldpc.h
at pl_interleave_check.  permutation() is its closed form in vectorised NumPy;
interleave_host / deinterleave_host apply it, bit for bit what the device kernels
(csrc/interleave.hip) do; the device methods take NumPy in and give NumPy back, or
CUDA tensors in and out with no host copy.
"""
from __future__ import annotations

import numpy as np

from .. import _native
from .qam import QAMModem

KINDS = {"rect": _native.PL_ILV_RECT, "tri": _native.PL_ILV_TRI}


def _isqrt(x: np.ndarray) -> np.ndarray:
    """floor(sqrt(x)) of int64 x < 2^52: the float root, mended by one step either way"""
    r = np.sqrt(x.astype(np.float64)).astype(np.int64)
    r -= r * r > x
    r += (r + 1) * (r + 1) <= x
    return r


class BitInterleaver:
    """kind "rect" (1 <= rows <= 64) or "tri" (rows None); 1 <= E <= 2^30.  AssertionError names the
    condition violated (include/polarldpc.h, pl_interleave_check).  Construction makes no device call."""

    def __init__(self, kind: str, E: int, rows=None):
        assert kind in KINDS, "kind = %r must be 'rect' or 'tri'" % (kind,)
        assert kind == "tri" or rows is not None, "rows is required for kind 'rect'"
        self.kind, self.E = kind, int(E)
        self.rows = 0 if rows is None else int(rows)
        self.dim = _native.interleave_check(KINDS[kind], self.rows, self.E)  # C or T
        self._perm = None

    @classmethod
    def for_modem(cls, modem, E: int) -> "BitInterleaver":
        """the row-column interleaver with one row per bit of the modem's symbol"""
        return cls("rect", E, rows=modem.m)

    @property
    def key(self):
        """[kind, rows], what identifies the interleaver beside E in a run key"""
        return [self.kind, self.rows]

    # ---- the definition's closed form, vectorised ----
    def permutation(self) -> np.ndarray:
        """pos as int64 [E]: f[pos[k]] = e[k]"""
        if self._perm is None:
            E, k = self.E, np.arange(self.E, dtype=np.int64)
            if self.kind == "rect":
                C = self.dim
                r, c = k // C, k % C
                Rf, q = E // C, E % C
                pos = c * Rf + np.minimum(c, q) + r
            else:
                T = self.dim
                b = 2 * T + 1

                def row(x):  # the largest i <= T with st(i) <= x
                    v = b * b - 8 * x
                    s = _isqrt(v)
                    return (b - (s + (s * s < v))) // 2

                def st(i):
                    return i * T - i * (i - 1) // 2

                i = row(k)
                j = k - st(i)
                Rf = int(row(np.array([E], dtype=np.int64))[0])
                q, a = E - st(Rf), T - Rf
                d = np.maximum(j - a, 0)
                pos = np.minimum(j, q) + Rf * np.minimum(j, a) + d * Rf - d * (d - 1) // 2 + i
            pos.setflags(write=False)
            self._perm = pos
        return self._perm

    def interleave_host(self, bits) -> np.ndarray:
        """bits [B, E] (or [E]) of any dtype -> the same shape and dtype: f[..., pos[k]] = e[..., k]"""
        e = np.asarray(bits)
        assert e.shape[-1] == self.E, "the last axis must have E = %d entries" % self.E
        f = np.empty_like(e)
        f[..., self.permutation()] = e
        return f

    def deinterleave_host(self, llr) -> np.ndarray:
        """llr [B, E] (or [E]) of any dtype -> the same shape and dtype, bit for bit: e[..., k] = f[..., pos[k]]"""
        f = np.asarray(llr)
        assert f.shape[-1] == self.E, "the last axis must have E = %d entries" % self.E
        bits = f.view("u%d" % f.dtype.itemsize) if f.dtype.kind == "f" else f  # NaN payloads survive fancy indexing
        return np.ascontiguousarray(bits[..., self.permutation()]).view(f.dtype)

    # ---- device ----
    def _device(self, x, out, dtypes, what, stream, launch):
        import torch
        host = not isinstance(x, torch.Tensor)
        if host:
            _native.require_gpu()
            x = torch.from_numpy(np.ascontiguousarray(x)).cuda()
        assert x.is_cuda and x.dtype in dtypes and x.dim() == 2 and x.shape[1] == self.E, \
            "%s must be %s [B, E = %d]" % (what, " or ".join(str(d) for d in dtypes), self.E)
        if x.stride(1) != 1 or (x.shape[0] > 1 and x.stride(0) < self.E):
            x = x.contiguous()
        y = out if out is not None else torch.empty((x.shape[0], self.E), dtype=x.dtype, device="cuda")
        QAMModem._check_out(y, x.shape[0], self.E, x.dtype, "out", "E")
        if x.shape[0]:
            launch(KINDS[self.kind], self.rows, self.E, x, y, stream=stream)
        return y.cpu().numpy() if host and out is None else y

    def interleave(self, bits, out=None, stream=None):
        """f[b][pos(k)] = e[b][k] on the device (pl_bit_interleave): bits uint8 [B, E] CUDA tensor (unit inner
        stride, any row pitch) -> uint8 [B, E] CUDA tensor, `out` if given (any row pitch >= E; bytes beyond E
        stay untouched; it must not overlap bits).  A NumPy array goes to the device and comes back as NumPy."""
        import torch
        return self._device(bits if isinstance(bits, torch.Tensor) else np.asarray(bits, dtype=np.uint8), out,
                            (torch.uint8,), "bits", stream, _native.bit_interleave)

    def deinterleave(self, llr, out=None, stream=None):
        """e[b][k] = f[b][pos(k)] on the device (pl_llr_deinterleave): llr float64 or float32 [B, E] CUDA tensor
        -> the same dtype [B, E], `out` if given, as interleave; values bit for bit.  A NumPy array (float32
        stays float32, anything else becomes float64) goes to the device and comes back as NumPy."""
        import torch
        if not isinstance(llr, torch.Tensor):
            llr = np.asarray(llr)
            llr = llr if llr.dtype == np.float32 else llr.astype(np.float64, copy=False)
        return self._device(llr, out, (torch.float64, torch.float32), "llr", stream, _native.llr_deinterleave)

    def __repr__(self) -> str:
        return "BitInterleaver(%r, E=%d%s)" % (self.kind, self.E, ", rows=%d" % self.rows if self.kind == "rect" else "")

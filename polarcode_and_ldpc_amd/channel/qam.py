"""Gray-mapped square QAM: modulator, complex AWGN, max-log soft demapper.

QAMModem(bits_per_symbol) stands between a rate matcher's E transmitted bits and
the E LLRs it takes back: QPSK, 16-, 64- and 256-QAM (BPSK stays with
AWGNChannel / pl_awgn_llr).  The definition -- bit to axis, the Gray axis
mapping, the scale, the symbol layout, the noise stream and the demapper's
operation order -- is stated once, in include/polarldpc.h at pl_qam_check.
modulate_host / demap_host are that definition in vectorised NumPy, bit for bit
what the device kernels (csrc/qam.hip) compute; the device methods take NumPy in
and give NumPy back, or CUDA tensors in and out with no host copy.
"""
from __future__ import annotations

import math

import numpy as np

from .. import _native

NAMES = {"qpsk": 2, "16qam": 4, "64qam": 6, "256qam": 8}


def sigma_of(snr_db: float) -> float:
    """sqrt(1 / (2 10^(snr_db / 10))) in the expression order of pl_awgn_llr; snr_db is Es/N0 per symbol."""
    return math.sqrt(1.0 / (2.0 * 10.0 ** (float(snr_db) / 10.0)))


class QAMModem:
    """m = bits_per_symbol in {2, 4, 6, 8}; h = m / 2 bits per axis.  AssertionError names the condition
    violated (include/polarldpc.h, pl_qam_check).  Construction makes no device call."""

    def __init__(self, bits_per_symbol: int):
        _, self.scale = _native.qam_check(bits_per_symbol, 1)
        self.m = int(bits_per_symbol)
        self.h = self.m // 2
        L = 1 << self.h
        # the axis mapping, enumerated: pattern b_0 .. b_(h-1) -> integer level; then each level's bits
        pat = (np.arange(L)[:, None] >> np.arange(self.h - 1, -1, -1)[None, :]) & 1  # [L, h], b_0 first
        lev = self._levels(pat)
        self.levels = np.arange(L - 1, -L, -2, dtype=np.int64)  # by index: idx 0 the largest
        self.level_bits = np.empty((L, self.h), dtype=np.int64)  # bits of the level at each index
        self.level_bits[(L - 1 - lev) // 2] = pat
        self.level_values = self.levels.astype(np.float64) * np.float64(self.scale)

    def _levels(self, b: np.ndarray) -> np.ndarray:
        """integer levels of axis bits b [..., h] (b_0 first): c_p = c_(p-1) ^ b_p, idx = sum c_p 2^(h-1-p)"""
        c = np.bitwise_xor.accumulate(b.astype(np.int64) & 1, axis=-1)
        idx = (c << np.arange(self.h - 1, -1, -1)).sum(axis=-1)
        return ((1 << self.h) - 1) - 2 * idx

    def S(self, E: int) -> int:
        """symbols per frame of E transmitted bits"""
        return _native.qam_check(self.m, E)[0]

    # ---- the definition, vectorised ----
    def modulate_host(self, bits) -> np.ndarray:
        """bits [B, E] (or [E]; bit 0 of each entry) -> float64 [B, 2 S] (or [2 S]): I, Q interleaved."""
        bits = np.asarray(bits)
        b2 = np.atleast_2d(bits)
        E = b2.shape[1]
        S = self.S(E)
        pad = np.zeros((b2.shape[0], S * self.m), dtype=np.int64)
        pad[:, :E] = b2.astype(np.int64) & 1
        a = self._levels(pad.reshape(-1, S, self.h, 2).transpose(0, 1, 3, 2))  # [B, S, axis]
        x = (a.astype(np.float64) * np.float64(self.scale)).reshape(-1, 2 * S)
        return x[0] if bits.ndim == 1 else x

    def demap_host(self, y, E: int, snr_db: float, dtype=np.float64) -> np.ndarray:
        """y float64 [B, >= 2 S] (or [2 S]) -> LLRs [B, E] (or [E]) of `dtype` (float64 or float32)."""
        y = np.asarray(y, dtype=np.float64)
        y2 = np.atleast_2d(y)
        S = self.S(E)
        assert y2.shape[1] >= 2 * S, "y must hold 2 S = %d values a frame" % (2 * S)
        sigma = sigma_of(snr_db)
        s2 = sigma * sigma
        w = np.float64(1.0 / (2.0 * s2))
        r = y2[:, :2 * S].reshape(-1, S, 2)
        with np.errstate(over="ignore", invalid="ignore"):
            t = r[..., None] - self.level_values
            d = t * t  # [B, S, axis, level]
            out = np.empty((r.shape[0], S, self.h, 2), dtype=np.float64)
            for p in range(self.h):
                one = self.level_bits[:, p] == 1
                out[:, :, p, :] = (d[..., one].min(axis=-1) - d[..., ~one].min(axis=-1)) * w
            llr = out.reshape(-1, S * self.m)[:, :E].astype(np.dtype(dtype))
        return llr[0] if y.ndim == 1 else llr

    # ---- device ----
    def modulate(self, bits, out=None):
        """Clean symbols on the device (pl_qam_modulate): bits uint8 [B, E] CUDA tensor (unit inner stride, any
        row pitch) -> float64 [B, 2 S] CUDA tensor, `out` if given (any row pitch >= 2 S; elements beyond stay
        untouched).  A NumPy array goes to the device and comes back as NumPy."""
        import torch
        host = not isinstance(bits, torch.Tensor)
        e = torch.from_numpy(np.array(bits, dtype=np.uint8)).cuda() if host else bits
        assert e.is_cuda and e.dtype == torch.uint8 and e.dim() == 2 and e.shape[1] >= 1, "bits must be uint8 [B, E]"
        E = int(e.shape[1])
        S = self.S(E)
        if e.stride(1) != 1 or (e.shape[0] > 1 and e.stride(0) < E):
            e = e.contiguous()
        x = out if out is not None else torch.empty((e.shape[0], 2 * S), dtype=torch.float64, device="cuda")
        self._check_out(x, e.shape[0], 2 * S, torch.float64, "out", "2 S")
        if e.shape[0]:
            _native.qam_modulate(self.m, E, e, x)
        return x.cpu().numpy() if host and out is None else x

    def awgn(self, bits, E: int, batch: int, snr_db: float, seed: int, frame_offset: int = 0, out=None, stream=None):
        """Received symbols y = x + sigma z on the device (pl_qam_awgn), mapped and disturbed in one pass: bits
        uint8 [batch, E] (CUDA tensor or NumPy) or None, the all-zero bits -> float64 [batch, 2 S], `out` if
        given.  Frame b draws the stream (seed, frame_offset + b); snr_db is Es/N0 per symbol.  NumPy bits
        come back as NumPy; with None the result is a CUDA tensor."""
        import torch
        _native.require_gpu()
        host = bits is not None and not isinstance(bits, torch.Tensor)
        e = torch.from_numpy(np.array(bits, dtype=np.uint8)).cuda() if host else bits
        E, batch = int(E), int(batch)
        S = self.S(E)
        if e is not None:
            assert e.is_cuda and e.dtype == torch.uint8 and e.shape == (batch, E), "bits must be uint8 [batch, E]"
            if e.stride(1) != 1 or (batch > 1 and e.stride(0) < E):
                e = e.contiguous()
        y = out if out is not None else torch.empty((batch, 2 * S), dtype=torch.float64, device="cuda")
        self._check_out(y, batch, 2 * S, torch.float64, "out", "2 S")
        if batch:
            _native.qam_awgn(self.m, E, e, snr_db, seed, frame_offset, y, stream=stream)
        return y.cpu().numpy() if host and out is None else y

    def demap(self, y, E: int, snr_db: float, dtype=np.float64, out=None, stream=None):
        """Max-log LLRs on the device (pl_qam_demap): y float64 [B, >= 2 S] CUDA tensor (unit inner stride, any row
        pitch) -> [B, E] CUDA tensor of `dtype` (float64 or float32), `out` if given (its dtype counts; any row
        pitch >= E; elements beyond E stay untouched).  A NumPy array goes to the device and comes back as
        NumPy."""
        import torch
        host = not isinstance(y, torch.Tensor)
        r = torch.from_numpy(np.array(y, dtype=np.float64)).cuda() if host else y
        E = int(E)
        S = self.S(E)
        assert r.is_cuda and r.dtype == torch.float64 and r.dim() == 2 and r.shape[1] >= 2 * S, \
            "y must be float64 [B, >= 2 S = %d]" % (2 * S)
        if r.stride(1) != 1 or (r.shape[0] > 1 and r.stride(0) < 2 * S):
            r = r.contiguous()
        tdt = torch.float32 if np.dtype(dtype) == np.float32 else torch.float64
        assert tdt == torch.float32 or np.dtype(dtype) == np.float64, "dtype must be float64 or float32"
        llr = out if out is not None else torch.empty((r.shape[0], E), dtype=tdt, device="cuda")
        self._check_out(llr, r.shape[0], E, llr.dtype if out is not None else tdt, "out", "E")
        assert llr.dtype in (torch.float32, torch.float64), "out must be float64 or float32"
        if r.shape[0]:
            _native.qam_demap(self.m, E, r, snr_db, llr, stream=stream)
        return llr.cpu().numpy() if host and out is None else llr

    @staticmethod
    def _check_out(t, B, width, dtype, name, what):
        assert t.is_cuda and t.dtype == dtype and t.dim() == 2 and t.shape == (B, width) and t.stride(1) == 1 \
            and (B <= 1 or t.stride(0) >= width), \
            "%s must be a [B, %s = %d] device tensor of %s, rows apart" % (name, what, width, dtype)

    def __repr__(self) -> str:
        return "QAMModem(bits_per_symbol=%d)" % self.m

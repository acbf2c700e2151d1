"""Gray-mapped square QAM: modulator, complex AWGN, max-log and exact log-MAP soft demappers.

QAMModem(bits_per_symbol) stands between a rate matcher's E transmitted bits and
the E LLRs it takes back: QPSK, 16-, 64- and 256-QAM (BPSK stays with
AWGNChannel / pl_awgn_llr).  The definition -- bit to axis, the Gray axis
mapping, the scale, the symbol layout, the noise stream and the demapper's
operation order -- is stated once, in include/polarldpc.h at pl_qam_check.
modulate_host / demap_host are that definition in vectorised NumPy, bit for bit
what the device kernels (csrc/qam.hip) compute; the device methods take NumPy in
and give NumPy back, or CUDA tensors in and out with no host copy.

Block Rayleigh fading of the symbols with channel state at the demapper (the
definition: include/polarldpc.h at pl_qam_fading_check) rides on it: rayleigh /
demap_csi on the device, fade_host / demap_csi_host as the definition in NumPy.

The demapper is max-log by default; QAMModem(m, demapper="logmap"), or method="logmap" at a call, gives the
exact log-MAP LLR (the definition: include/polarldpc.h at pl_qam_demap_logmap), on the device and in the host
methods alike; its expm1 and log1p are glibc's algorithms restated in libm_np.
"""
from __future__ import annotations

import math

import numpy as np

from .. import _native
from . import libm_np

NAMES = {"qpsk": 2, "16qam": 4, "64qam": 6, "256qam": 8}
DEMAPPERS = ("maxlog", "logmap")


def sigma_of(snr_db: float) -> float:
    """sqrt(1 / (2 10^(snr_db / 10))) in the expression order of pl_awgn_llr; snr_db is Es/N0 per symbol."""
    return math.sqrt(1.0 / (2.0 * 10.0 ** (float(snr_db) / 10.0)))


class QAMModem:
    """m = bits_per_symbol in {2, 4, 6, 8}; h = m / 2 bits per axis.  AssertionError names the condition
    violated (include/polarldpc.h, pl_qam_check).  demapper: "maxlog" or "logmap", what demap, demap_csi and their
    host forms compute when their `method` is None.  Construction makes no device call."""

    def __init__(self, bits_per_symbol: int, demapper: str = "maxlog"):
        _, self.scale = _native.qam_check(bits_per_symbol, 1)
        assert demapper in DEMAPPERS, "demapper %r must be one of %s" % (demapper, ", ".join(DEMAPPERS))
        self.demapper = demapper
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

    def _method(self, method) -> str:
        """a call's method: None is the modem's own demapper"""
        if method is None:
            return self.demapper
        assert method in DEMAPPERS, "demapper %r must be one of %s" % (method, ", ".join(DEMAPPERS))
        return method

    def _axis_llrs(self, d, W, logmap: bool) -> np.ndarray:
        """d [B, S, axis, level], W a scalar or [B, S, 1] -> [B, S, h, axis]: max-log, or the exact log-MAP of
        pl_qam_demap_logmap, the levels of each set in ascending index"""
        out = np.empty(d.shape[:2] + (self.h, 2), dtype=np.float64)
        for p in range(self.h):
            one = self.level_bits[:, p] == 1
            D1, D0 = d[..., one].min(axis=-1), d[..., ~one].min(axis=-1)
            out[:, :, p, :] = (D1 - D0) * W
            if logmap:
                c = []
                for D, idx in ((D0, np.flatnonzero(~one)), (D1, np.flatnonzero(one))):
                    T = np.zeros_like(D)
                    for a in idx:
                        T = T + (libm_np.expm1((D - d[..., a]) * W) + 1.0)
                    c.append(libm_np.log1p(T - 1.0))
                out[:, :, p, :] = out[:, :, p, :] + (c[0] - c[1])
        return out

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

    def demap_host(self, y, E: int, snr_db: float, dtype=np.float64, method=None) -> np.ndarray:
        """y float64 [B, >= 2 S] (or [2 S]) -> LLRs [B, E] (or [E]) of `dtype` (float64 or float32); method: None
        (the modem's demapper), "maxlog" or "logmap"."""
        logmap = self._method(method) == "logmap"
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
            out = self._axis_llrs(d, w, logmap)
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

    def demap(self, y, E: int, snr_db: float, dtype=np.float64, out=None, stream=None, method=None):
        """LLRs on the device, max-log (pl_qam_demap) or exact log-MAP (pl_qam_demap_logmap) by `method` (None: the
        modem's demapper): y float64 [B, >= 2 S] CUDA tensor (unit inner stride, any row
        pitch) -> [B, E] CUDA tensor of `dtype` (float64 or float32), `out` if given (its dtype counts; any row
        pitch >= E; elements beyond E stay untouched).  A NumPy array goes to the device and comes back as
        NumPy."""
        import torch
        logmap = self._method(method) == "logmap"
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
            _native.qam_demap(self.m, E, r, snr_db, llr, stream=stream, logmap=logmap)
        return llr.cpu().numpy() if host and out is None else llr

    # ---- block Rayleigh fading; the definition: include/polarldpc.h at pl_qam_fading_check ----
    def blocks(self, E: int, coherence: int) -> int:
        """Q, fading blocks per frame of E transmitted bits at a coherence length of `coherence` symbols"""
        return _native.qam_fading_check(self.m, E, coherence)[1]

    @staticmethod
    def _per_symbol(h2, S, coherence):
        """(hr, hi) [B, S] of the coefficients h2 [B, >= 2 Q]: symbol s takes block s // coherence"""
        q = np.arange(S) // int(coherence)
        assert h2.shape[1] >= 2 * (int(q[-1]) + 1), "h must hold 2 Q = %d values a frame" % (2 * (int(q[-1]) + 1))
        return h2[:, 2 * q], h2[:, 2 * q + 1]

    def fade_host(self, x, h, noise, coherence: int) -> np.ndarray:
        """y = h x + noise by the definition's operations: x, noise float64 [B, 2 S] (or [2 S]; noise is sigma z),
        h float64 [B, >= 2 Q] (or [>= 2 Q]), Re and Im interleaved -> float64 [B, 2 S] (or [2 S])."""
        x = np.asarray(x, dtype=np.float64)
        x2, n2 = np.atleast_2d(x), np.atleast_2d(np.asarray(noise, dtype=np.float64))
        hr, hi = self._per_symbol(np.atleast_2d(np.asarray(h, dtype=np.float64)), x2.shape[1] // 2, coherence)
        xi, xq = x2[:, 0::2], x2[:, 1::2]
        y = np.empty_like(x2)
        with np.errstate(over="ignore", invalid="ignore"):
            y[:, 0::2] = (hr * xi - hi * xq) + n2[:, 0::2]
            y[:, 1::2] = (hr * xq + hi * xi) + n2[:, 1::2]
        return y[0] if x.ndim == 1 else y

    def demap_csi_host(self, y, h, E: int, snr_db: float, coherence: int = 1, dtype=np.float64,
                       method=None) -> np.ndarray:
        """y float64 [B, >= 2 S], h float64 [B, >= 2 Q] (or one frame of each) -> LLRs [B, E] (or [E]) of `dtype`
        (float64 or float32); a symbol whose |h|^2 is 0.0 gives +0.0; method as demap_host's."""
        logmap = self._method(method) == "logmap"
        y = np.asarray(y, dtype=np.float64)
        y2 = np.atleast_2d(y)
        S = _native.qam_fading_check(self.m, E, coherence)[0]
        assert y2.shape[1] >= 2 * S, "y must hold 2 S = %d values a frame" % (2 * S)
        hr, hi = self._per_symbol(np.atleast_2d(np.asarray(h, dtype=np.float64)), S, coherence)
        sigma = sigma_of(snr_db)
        s2 = sigma * sigma
        w = np.float64(1.0 / (2.0 * s2))
        yi, yq = y2[:, 0:2 * S:2], y2[:, 1:2 * S:2]
        with np.errstate(over="ignore", under="ignore", invalid="ignore", divide="ignore"):
            g = hr * hr + hi * hi
            ui = hr * yi + hi * yq
            uq = hr * yq - hi * yi
            r = np.stack([ui / g, uq / g], axis=-1)  # [B, S, axis]
            wg = (w * g)[..., None]
            t = r[..., None] - self.level_values
            d = t * t  # [B, S, axis, level]
            out = self._axis_llrs(d, wg, logmap)
            out[g == 0.0] = 0.0
            llr = out.reshape(-1, S * self.m)[:, :E].astype(np.dtype(dtype))
        return llr[0] if y.ndim == 1 else llr

    def rayleigh(self, bits, E: int, batch: int, snr_db: float, seed: int, coherence: int = 1, frame_offset: int = 0,
                 out=None, h_out=None, stream=None):
        """Received symbols y = h x + sigma z and the coefficients h on the device (pl_qam_rayleigh), mapped, faded
        and disturbed in one pass: bits as awgn's (uint8 [batch, E], CUDA tensor or NumPy, or None) -> (y float64
        [batch, 2 S], h float64 [batch, 2 Q]), `out` and `h_out` if given (any row pitch; elements beyond stay
        untouched).  Block q of frame b draws the stream (seed, frame_offset + b, q) whatever the coherence
        length; the noise is awgn's for the same seed.  NumPy bits come back as NumPy."""
        import torch
        _native.require_gpu()
        host = bits is not None and not isinstance(bits, torch.Tensor)
        e = torch.from_numpy(np.array(bits, dtype=np.uint8)).cuda() if host else bits
        E, batch = int(E), int(batch)
        S, Q = _native.qam_fading_check(self.m, E, coherence)
        if e is not None:
            assert e.is_cuda and e.dtype == torch.uint8 and e.shape == (batch, E), "bits must be uint8 [batch, E]"
            if e.stride(1) != 1 or (batch > 1 and e.stride(0) < E):
                e = e.contiguous()
        y = out if out is not None else torch.empty((batch, 2 * S), dtype=torch.float64, device="cuda")
        h = h_out if h_out is not None else torch.empty((batch, 2 * Q), dtype=torch.float64, device="cuda")
        self._check_out(y, batch, 2 * S, torch.float64, "out", "2 S")
        self._check_out(h, batch, 2 * Q, torch.float64, "h_out", "2 Q")
        if batch:
            _native.qam_rayleigh(self.m, E, coherence, e, snr_db, seed, frame_offset, y, h, stream=stream)
        if host:
            return (y.cpu().numpy() if out is None else y), (h.cpu().numpy() if h_out is None else h)
        return y, h

    def demap_csi(self, y, h, E: int, snr_db: float, coherence: int = 1, dtype=np.float64, out=None, stream=None,
                  method=None):
        """LLRs with channel state on the device, max-log (pl_qam_demap_csi) or exact log-MAP
        (pl_qam_demap_csi_logmap) by `method` (None: the modem's demapper): y float64 [B, >= 2 S] and h float64
        [B, >= 2 Q], CUDA tensors (unit inner stride, any row pitch) -> [B, E] CUDA tensor of `dtype` (float64 or
        float32), `out` if given (its dtype counts; any row pitch >= E; elements beyond E stay untouched).  NumPy
        arrays go to the device and the result comes back as NumPy."""
        import torch
        logmap = self._method(method) == "logmap"
        host = not isinstance(y, torch.Tensor)
        r = torch.from_numpy(np.array(y, dtype=np.float64)).cuda() if host else y
        c = torch.from_numpy(np.array(h, dtype=np.float64)).cuda() if not isinstance(h, torch.Tensor) else h
        E = int(E)
        S, Q = _native.qam_fading_check(self.m, E, coherence)
        assert r.is_cuda and r.dtype == torch.float64 and r.dim() == 2 and r.shape[1] >= 2 * S, \
            "y must be float64 [B, >= 2 S = %d]" % (2 * S)
        assert c.is_cuda and c.dtype == torch.float64 and c.dim() == 2 and c.shape[0] == r.shape[0] \
            and c.shape[1] >= 2 * Q, "h must be float64 [B, >= 2 Q = %d]" % (2 * Q)
        if r.stride(1) != 1 or (r.shape[0] > 1 and r.stride(0) < 2 * S):
            r = r.contiguous()
        if c.stride(1) != 1 or (c.shape[0] > 1 and c.stride(0) < 2 * Q):
            c = c.contiguous()
        tdt = torch.float32 if np.dtype(dtype) == np.float32 else torch.float64
        assert tdt == torch.float32 or np.dtype(dtype) == np.float64, "dtype must be float64 or float32"
        llr = out if out is not None else torch.empty((r.shape[0], E), dtype=tdt, device="cuda")
        self._check_out(llr, r.shape[0], E, llr.dtype if out is not None else tdt, "out", "E")
        assert llr.dtype in (torch.float32, torch.float64), "out must be float64 or float32"
        if r.shape[0]:
            _native.qam_demap_csi(self.m, E, coherence, r, c, snr_db, llr, stream=stream, logmap=logmap)
        return llr.cpu().numpy() if host and out is None else llr

    @staticmethod
    def _check_out(t, B, width, dtype, name, what):
        assert t.is_cuda and t.dtype == dtype and t.dim() == 2 and t.shape == (B, width) and t.stride(1) == 1 \
            and (B <= 1 or t.stride(0) >= width), \
            "%s must be a [B, %s = %d] device tensor of %s, rows apart" % (name, what, width, dtype)

    def __repr__(self) -> str:
        if self.demapper != "maxlog":
            return "QAMModem(bits_per_symbol=%d, demapper=%r)" % (self.m, self.demapper)
        return "QAMModem(bits_per_symbol=%d)" % self.m

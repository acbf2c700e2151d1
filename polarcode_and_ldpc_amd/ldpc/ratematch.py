"""Rate matching for quasi-cyclic LDPC codes: puncture, shorten, repeat.

QCRateMatcher selects the E transmitted bits of a codeword of the code (base, Z)
and brings received LLRs back to codeword positions, on the device
(pl_ldpc_rate_match / pl_ldpc_rate_recover, csrc/ldpc_qc_ratematch.hip).  The
definition -- the parameters, the selection loop, the recovery's sum order,
fillers, accumulation -- is stated once, in include/polarldpc.h at pl_rate_match.
select_host / recover_host are that loop written out in NumPy, with no closed
form: the reference the device results are tested against.
"""
from __future__ import annotations

import numpy as np

from .. import _native
from .matrix import qc_encoding_structure


def _float_dtype(dtype) -> np.dtype:
    name = str(dtype).replace("torch.", "")
    d = np.dtype(name if name in ("float32", "float64") else dtype)
    assert d in (np.dtype(np.float32), np.dtype(np.float64)), "dtype must be float64 or float32"
    return d


class QCRateMatcher:
    """Rate matching of the code (base, Z), base int [mb, nb] of the structure
    QCLDPCEncoder encodes from (qc_encoding_structure).

    punctured: leading block columns never sent; fillers: the last `fillers`
    message bits are known zeros and never sent; ncb: length of the circular
    buffer behind the punctured columns (default n - P); start: where reading
    begins in it; E: transmitted bits per frame, with wrap-around repetition when
    E exceeds the buffer.  filler_llr: what recover writes at a filler, the sign
    that decodes to bit 0.  AssertionError names the first condition violated
    (include/polarldpc.h, pl_rate_match).  Construction makes no device call."""

    def __init__(self, base, Z: int, E: int, punctured: int = 0, fillers: int = 0, ncb=None, start: int = 0,
                 filler_llr: float = 1024.0):
        self.base = np.array(base, dtype=np.int64)
        if self.base.ndim != 2 or self.base.size == 0:
            raise ValueError("base must be [mb, nb]")
        self.Z = int(Z)
        self.mb, self.nb = self.base.shape
        self.g, _ = qc_encoding_structure(self.base)
        self.rm = _native.rate_match_probe(self.mb, self.nb, self.Z, punctured, fillers, -1 if ncb is None else ncb,
                                           start, E)
        self.kb = self.nb - self.mb
        self.n, self.k, self.P = self.rm.n, self.rm.k, self.rm.P
        self.E, self.punctured, self.fillers, self.ncb, self.start = int(E), int(punctured), int(fillers), \
            self.rm.ncb, int(start)
        self.M, self.c0, self.hi, self.max_reps = self.rm.M, self.rm.c0, self.rm.hi, self.rm.max_reps
        self.filler_llr = float(filler_llr)
        self._pos = None

    # ---- the definition, literally ----
    def positions_host(self) -> np.ndarray:
        """int64 [E]: the codeword position of transmitted bit t, by the selection loop."""
        if self._pos is None:
            lo, hi = self.k - self.P - self.fillers, self.k - self.P  # buffer positions lo .. hi-1 are the fillers
            pos, j = [], 0
            while len(pos) < self.E:
                b = (self.start + j) % self.ncb
                if not lo <= b < hi:
                    pos.append(self.P + b)
                j += 1
            self._pos = np.array(pos, dtype=np.int64)
            self._pos.setflags(write=False)
        return self._pos

    def select_host(self, cw) -> np.ndarray:
        """e[:, t] = cw[:, position of t]: cw [B, n] (or [n]) -> [B, E] (or [E]), cw's dtype."""
        cw = np.asarray(cw)
        assert cw.shape[-1] == self.n, "codewords must have n = %d entries" % self.n
        e = np.empty(cw.shape[:-1] + (self.E,), dtype=cw.dtype)
        for t, p in enumerate(self.positions_host()):
            e[..., t] = cw[..., p]
        return e

    def recover_host(self, llr, n_out=None, dtype=np.float64, out=None, accumulate: bool = False) -> np.ndarray:
        """The recovery of the definition: llr float [B, E] -> `dtype` [B, n_out].  accumulate: added to
        `out` (an earlier recovery, not modified) at the transmitted positions, the rest of it kept."""
        llr = np.asarray(llr)
        assert llr.ndim == 2 and llr.shape[1] == self.E, "llr must be [B, E]"
        T = _float_dtype(dtype if out is None else out.dtype)
        n_out = self._n_out(n_out, out)
        s = np.zeros((llr.shape[0], n_out), dtype=T)  # +0.0
        seen = np.zeros(n_out, dtype=bool)
        for t, p in enumerate(self.positions_host()):
            term = llr[:, t].astype(T)
            s[:, p] = s[:, p] + term if seen[p] else term
            seen[p] = True
        if accumulate:
            assert out is not None and out.shape == s.shape, "accumulate needs out [B, n_out]"
            res = np.array(out, dtype=T)
            res[:, seen] = res[:, seen] + s[:, seen]
            return res
        s[:, self.k - self.fillers:self.k] = T.type(self.filler_llr)
        return s

    # ---- the decoder's code ----
    def decoder_rows(self) -> int:
        """The smallest mb' with max(g, 1) <= mb' <= mb whose code (kb + mb') Z covers the highest
        transmitted position: later extension rows only involve parity bits that were never sent."""
        for r in range(max(self.g, 1), self.mb + 1):
            if self.hi < (self.kb + r) * self.Z:
                return r
        raise AssertionError("unreachable: hi < n")

    def decoder_base(self) -> np.ndarray:
        """base[:mb', :kb + mb']: a valid code, since extension row i has nothing right of column kb + i."""
        r = self.decoder_rows()
        return self.base[:r, :self.kb + r].copy()

    @property
    def n_dec(self) -> int:
        """Length of the decoder_base() code, recover's default n_out."""
        return (self.kb + self.decoder_rows()) * self.Z

    def rv_start(self, rv: int) -> int:
        """floor(rv ncb / (4 Z)) Z: four evenly spread start offsets on block boundaries.  Build-defined,
        a convenience; it reproduces no standard's table."""
        return (int(rv) * self.ncb) // (4 * self.Z) * self.Z

    def _n_out(self, n_out, out) -> int:
        n_out = int(n_out) if n_out is not None else (out.shape[1] if out is not None else self.n_dec)
        assert self.hi < n_out <= self.n, "n_out must lie in hi + 1 = %d .. n = %d" % (self.hi + 1, self.n)
        return n_out

    # ---- device ----
    def select(self, cw, out=None):
        """Transmitted bytes of codewords on the device (pl_ldpc_rate_match): cw uint8 [B, n] CUDA tensor
        (unit inner stride, any row pitch) -> uint8 [B, E] CUDA tensor, `out` if given (any row pitch
        >= E; bytes beyond E stay untouched).  A NumPy array goes to the device and comes back as NumPy."""
        import torch
        host = not isinstance(cw, torch.Tensor)
        c = torch.from_numpy(np.array(cw, dtype=np.uint8)).cuda() if host else cw
        assert c.is_cuda and c.dtype == torch.uint8 and c.dim() == 2 and c.shape[1] == self.n, \
            "cw must be uint8 [B, n = %d]" % self.n
        if c.stride(1) != 1 or (c.shape[0] > 1 and c.stride(0) < self.n):
            c = c.contiguous()
        e = out if out is not None else torch.empty((c.shape[0], self.E), dtype=torch.uint8, device="cuda")
        assert e.is_cuda and e.dtype == torch.uint8 and e.shape == (c.shape[0], self.E) and e.stride(1) == 1 \
            and (e.shape[0] <= 1 or e.stride(0) >= self.E), "out must be a uint8 [B, E] device tensor, rows apart"
        if c.shape[0]:
            _native.rate_match(self.rm, c, e)
        return e.cpu().numpy() if host and out is None else e

    def recover(self, llr, n_out=None, dtype=np.float64, out=None, accumulate: bool = False):
        """LLRs of E received values back at codeword positions on the device (pl_ldpc_rate_recover): llr
        float64 or float32 [B, E] CUDA tensor (unit inner stride, any row pitch) -> `dtype` [B, n_out]
        CUDA tensor, `out` if given (its dtype and width count; elements beyond n_out stay untouched).
        n_out defaults to n_dec, the length of the decoder_base() code.  accumulate: soft-combine into
        `out`, which holds an earlier recovery of the same frames (of this or another matcher of the
        code).  A NumPy array goes to the device and comes back as NumPy (a NumPy `out` is written)."""
        import torch
        host = not isinstance(llr, torch.Tensor)
        out_np = out if host and isinstance(out, np.ndarray) else None
        l = torch.from_numpy(np.array(llr)).cuda() if host else llr
        assert l.is_cuda and l.dtype in (torch.float32, torch.float64) and l.dim() == 2 and l.shape[1] == self.E, \
            "llr must be float64 or float32 [B, E = %d]" % self.E
        if l.stride(1) != 1 or (l.shape[0] > 1 and l.stride(0) < self.E):
            l = l.contiguous()
        if host and out is not None and not isinstance(out, torch.Tensor):
            out = torch.from_numpy(np.array(out)).cuda()
        n_out = self._n_out(n_out, out)
        assert out is not None or not accumulate, "accumulate needs out, the earlier recovery"
        if out is None:
            T = torch.float32 if _float_dtype(dtype) == np.float32 else torch.float64
            out = torch.empty((l.shape[0], n_out), dtype=T, device="cuda")
        assert out.is_cuda and out.dtype in (torch.float32, torch.float64) and out.shape == (l.shape[0], n_out) \
            and out.stride(1) == 1 and (out.shape[0] <= 1 or out.stride(0) >= n_out), \
            "out must be a float [B, n_out] device tensor, rows apart"
        if l.shape[0]:
            _native.rate_recover(self.rm, l, out, n_out, self.filler_llr, accumulate)
        if out_np is not None:
            out_np[...] = out.cpu().numpy()
            return out_np
        return out.cpu().numpy() if host else out

    def __repr__(self) -> str:
        return ("QCRateMatcher(n=%d, k=%d, Z=%d, E=%d, punctured=%d, fillers=%d, ncb=%d, start=%d)"
                % (self.n, self.k, self.Z, self.E, self.punctured, self.fillers, self.ncb, self.start))

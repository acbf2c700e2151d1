"""Rate matching for polar codes: puncture, shorten, repeat.

PolarRateMatcher selects the E transmitted bits of a codeword of the mother code
of length N through a sub-block interleaver, and brings received LLRs back to
the N decoder inputs, on the device (pl_polar_rate_match /
pl_polar_rate_recover, csrc/polar_ratematch.hip).  The definition -- the
parameters, the interleaved sequence, the selection, the recovery's sum order,
known_llr, accumulation, and the frozen set a shortened code needs -- is stated
once, in include/polarldpc.h at pl_polar_rm.  select_host / recover_host are
that selection written out in NumPy as a loop, with no closed form: the
reference the device results are tested against.
"""
from __future__ import annotations

import numpy as np

from .. import _native

MODES = {"puncture": _native.PL_PRM_PUNCTURE, "shorten": _native.PL_PRM_SHORTEN}


class PolarRateMatcher:
    """Rate matching of the polar mother code of length N to E transmitted bits.

    mode: "puncture" or "shorten", what happens when E < N (E >= N repeats);
    sub_blocks: the permutation of the nsub = len(sub_blocks) sub-blocks of N / nsub
    positions (None: nsub = 1, plain block puncturing / shortening); known_llr:
    what recover writes at a shortened position, the sign that decodes to bit 0,
    finite.  Shortening forces forced_frozen() to be frozen; that set is small only
    when sub_blocks keeps the highest sub-blocks last (see the header).
    AssertionError names the first condition violated (include/polarldpc.h,
    pl_polar_rm).  Construction makes no device call."""

    def __init__(self, N: int, E: int, mode: str = "puncture", sub_blocks=None, known_llr: float = 1024.0):
        if mode not in MODES:
            raise ValueError("mode must be 'puncture' or 'shorten'")
        perm = [0] if sub_blocks is None else [int(p) for p in sub_blocks]
        assert 1 <= len(perm) <= 32 and all(0 <= p < 256 for p in perm), \
            "sub_blocks must hold 1 .. 32 sub-block numbers"
        self.rm = _native.polar_rate_match_probe(N, E, MODES[mode], perm)
        self.N, self.E, self.mode, self.nsub = int(N), int(E), mode, len(perm)
        self.perm = np.array(perm, dtype=np.int64)
        self.S, self.U, self.max_reps = self.rm.S, self.rm.U, self.rm.max_reps
        self.known_llr = float(known_llr)
        assert np.isfinite(self.known_llr) and self.known_llr > 0, "known_llr must be finite and > 0"
        self._pos = None

    # ---- the definition, literally ----
    def positions_host(self) -> np.ndarray:
        """int64 [E]: the codeword position of transmitted bit t, by the selection written out."""
        if self._pos is None:
            y = []  # the interleaved sequence: sub-block perm[q] is the q-th one
            for q in range(self.nsub):
                for r in range(self.S):
                    y.append(int(self.perm[q]) * self.S + r)
            pos = []
            if self.E >= self.N:
                m = 0
                while len(pos) < self.E:
                    pos.append(y[m])
                    m = m + 1 if m + 1 < self.N else 0
            elif self.mode == "puncture":
                pos = y[self.N - self.E:]
            else:
                pos = y[:self.E]
            self._pos = np.array(pos, dtype=np.int64)
            self._pos.setflags(write=False)
        return self._pos

    @property
    def untransmitted(self) -> np.ndarray:
        """Sorted codeword positions that are never sent (empty when E >= N)."""
        sent = np.zeros(self.N, dtype=bool)
        sent[self.positions_host()] = True
        return np.flatnonzero(~sent)

    def select_host(self, cw) -> np.ndarray:
        """e[:, t] = cw[:, position of t]: cw [B, N] (or [N]) -> [B, E] (or [E]), cw's dtype."""
        cw = np.asarray(cw)
        assert cw.shape[-1] == self.N, "codewords must have N = %d entries" % self.N
        e = np.empty(cw.shape[:-1] + (self.E,), dtype=cw.dtype)
        for t, p in enumerate(self.positions_host()):
            e[..., t] = cw[..., p]
        return e

    def recover_host(self, llr, out=None, accumulate: bool = False) -> np.ndarray:
        """The recovery of the definition: llr float64 or float32 [B, E] -> float64 [B, N].  accumulate: added
        to `out` (an earlier recovery, not modified) at the transmitted positions, the rest of it kept."""
        llr = np.asarray(llr)
        assert llr.ndim == 2 and llr.shape[1] == self.E, "llr must be [B, E]"
        s = np.zeros((llr.shape[0], self.N), dtype=np.float64)  # +0.0
        seen = np.zeros(self.N, dtype=bool)
        for t, p in enumerate(self.positions_host()):
            term = llr[:, t].astype(np.float64)
            s[:, p] = s[:, p] + term if seen[p] else term
            seen[p] = True
        if accumulate:
            assert out is not None and out.shape == s.shape, "accumulate needs out [B, N]"
            res = np.array(out, dtype=np.float64)
            res[:, seen] = res[:, seen] + s[:, seen]
            return res
        if self.mode == "shorten":
            s[:, ~seen] = self.known_llr
        return s

    # ---- the frozen set a shortened code needs ----
    def forced_frozen(self) -> np.ndarray:
        """Sorted u indices that must be frozen (pl_polar_rate_match_forced): for shorten with E < N every
        superset of an untransmitted position, else none."""
        return np.flatnonzero(_native.polar_rate_match_forced(self.rm)).astype(np.int64)

    def check_frozen(self, frozen_bits) -> None:
        """AssertionError when a forced index is not in frozen_bits."""
        missing = np.setdiff1d(self.forced_frozen(), np.asarray(frozen_bits, dtype=np.int64))
        assert missing.size == 0, ("the frozen set lacks %d indices that shortening forces (first: %d): the "
                                   "untransmitted bits would not be zero" % (missing.size, missing[0] if missing.size else -1))

    # ---- device ----
    def select(self, cw, out=None):
        """Transmitted bytes of codewords on the device (pl_polar_rate_match): cw uint8 [B, N] CUDA tensor
        (unit inner stride, any row pitch) -> uint8 [B, E] CUDA tensor, `out` if given (any row pitch
        >= E; bytes beyond E stay untouched).  A NumPy array goes to the device and comes back as NumPy."""
        import torch
        host = not isinstance(cw, torch.Tensor)
        c = torch.from_numpy(np.array(cw, dtype=np.uint8)).cuda() if host else cw
        assert c.is_cuda and c.dtype == torch.uint8 and c.dim() == 2 and c.shape[1] == self.N, \
            "cw must be uint8 [B, N = %d]" % self.N
        if c.stride(1) != 1 or (c.shape[0] > 1 and c.stride(0) < self.N):
            c = c.contiguous()
        e = out if out is not None else torch.empty((c.shape[0], self.E), dtype=torch.uint8, device="cuda")
        assert e.is_cuda and e.dtype == torch.uint8 and e.shape == (c.shape[0], self.E) and e.stride(1) == 1 \
            and (e.shape[0] <= 1 or e.stride(0) >= self.E), "out must be a uint8 [B, E] device tensor, rows apart"
        if c.shape[0]:
            _native.polar_rate_match(self.rm, c, e)
        return e.cpu().numpy() if host and out is None else e

    def recover(self, llr, out=None, accumulate: bool = False):
        """LLRs of E received values back at the N decoder inputs on the device (pl_polar_rate_recover): llr
        float64 or float32 [B, E] CUDA tensor (unit inner stride, any row pitch) -> float64 [B, N] CUDA
        tensor, `out` if given (any row pitch >= N; elements beyond N stay untouched).  accumulate:
        soft-combine into `out`, which holds an earlier recovery of the same frames (of this or another
        matcher of the same N).  A NumPy array goes to the device and comes back as NumPy (a NumPy `out`
        is written)."""
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
        assert out is not None or not accumulate, "accumulate needs out, the earlier recovery"
        if out is None:
            out = torch.empty((l.shape[0], self.N), dtype=torch.float64, device="cuda")
        assert out.is_cuda and out.dtype == torch.float64 and out.shape == (l.shape[0], self.N) \
            and out.stride(1) == 1 and (out.shape[0] <= 1 or out.stride(0) >= self.N), \
            "out must be a float64 [B, N] device tensor, rows apart"
        if l.shape[0]:
            _native.polar_rate_recover(self.rm, l, out, self.known_llr, accumulate)
        if out_np is not None:
            out_np[...] = out.cpu().numpy()
            return out_np
        return out.cpu().numpy() if host else out

    def __repr__(self) -> str:
        return "PolarRateMatcher(N=%d, E=%d, mode=%s, sub_blocks=%s)" % (self.N, self.E, self.mode, self.perm.tolist())

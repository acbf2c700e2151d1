"""Monte-Carlo BER/FER engine: frames sharded over GPUs, one all-reduce per round.

Semantics follow benchmarks/ber_simulation.py:132-293 of the reference:
per SNR point, frames of random messages are encoded, sent through BPSK/AWGN
and decoded; BER = bit errors / (frames * K), FER = frame errors / frames, and a
point stops once `max_errors` frame errors are seen (:191-192) or `num_frames`
frames are done (:167).  Differences, by design:
  * frames run in rounds of `batch` frames per rank; the stop test is applied
    after each round (the reference stops at the exact frame), so a point may
    overshoot max_errors by less than one round -- BER/FER stay unbiased;
  * frame f of SNR point s uses the noise/message stream (seed, s, f) (Philox on
    the device), so results are identical for any number of GPUs;
  * the only collective is one all-reduce (SUM) of int64[3] = {bit errors,
    frame errors, frames} per round (RCCL over xGMI on GPUs, gloo on CPU).
"""
from __future__ import annotations

import math
from dataclasses import asdict, dataclass, field
from typing import Callable, List, Optional, Sequence

import numpy as np


def wilson_interval(errors: int, total: int, confidence: float = 0.95):
    """(rate, lower, upper): the Wilson score interval of
    src/utils/metrics.py:138-167 (calculate_ber_with_confidence)."""
    if total == 0:
        return 0.0, 0.0, 0.0
    from statistics import NormalDist
    z = NormalDist().inv_cdf(1 - (1 - confidence) / 2)
    p = errors / total
    den = 1 + z ** 2 / total
    center = (p + z ** 2 / (2 * total)) / den
    margin = z * math.sqrt(p * (1 - p) / total + z ** 2 / (4 * total ** 2)) / den
    return p, max(0.0, center - margin), min(1.0, center + margin)


def shard(total: int, rank: int, world: int):
    """Contiguous shard [start, start+count) of `total` frames for `rank`."""
    base, extra = divmod(total, world)
    start = rank * base + min(rank, extra)
    return start, base + (1 if rank < extra else 0)


@dataclass
class PointResult:
    snr_db: float
    frames: int
    frame_errors: int
    bit_errors: int
    info_bits: int
    ber: float = 0.0
    fer: float = 0.0
    ber_ci: tuple = field(default_factory=tuple)
    fer_ci: tuple = field(default_factory=tuple)
    rounds: int = 0

    def finalize(self):
        tb = self.frames * self.info_bits
        self.ber, lo, hi = wilson_interval(self.bit_errors, tb)
        self.ber_ci = (lo, hi)
        self.fer, lo, hi = wilson_interval(self.frame_errors, self.frames)
        self.fer_ci = (lo, hi)
        return self

    def as_dict(self):
        return asdict(self)


RoundFn = Callable[[int, float, int, int], np.ndarray]
"""round_fn(snr_index, snr_db, global_frame_offset, nframes) -> int64[3] local
counts {bit errors, frame errors, frames} for frames [offset, offset+nframes)."""


class MonteCarlo:
    def __init__(self, round_fn: RoundFn, info_bits: int, batch: int, group=None, device=None):
        self.round_fn = round_fn
        self.info_bits = info_bits
        self.batch = int(batch)
        self.group = group
        self.device = device
        import torch.distributed as dist
        self._dist = dist if (dist.is_available() and dist.is_initialized()) else None
        self.rank = self._dist.get_rank(group) if self._dist else 0
        self.world = self._dist.get_world_size(group) if self._dist else 1

    def _allreduce(self, counts: np.ndarray) -> np.ndarray:
        if self.world == 1:
            return counts
        import torch
        # RCCL reduces device tensors; gloo (CPU tests, one-GPU rehearsals) host ones
        dev = "cpu" if self._dist.get_backend(self.group) == "gloo" else self.device
        t = torch.as_tensor(counts, dtype=torch.int64, device=dev)
        self._dist.all_reduce(t, group=self.group)
        return t.cpu().numpy()

    def _finished(self, log: "Optional[PointLog]") -> dict:
        """Finished points of `log`, read on rank 0 and broadcast, so that every
        rank skips the same SNR points even when the ranks do not share a file
        system (or the file changes between their reads): a disagreement would
        pair different points' all-reduces."""
        done = log.load() if (log is not None and self.rank == 0) else {}
        if self.world > 1:
            box = [sorted((k, v.as_dict()) for k, v in done.items())]
            self._dist.broadcast_object_list(box, src=self._dist.get_global_rank(self.group, 0)
                                             if self.group is not None else 0, group=self.group)
            done = {}
            for k, d in box[0]:
                done[k] = PointResult(snr_db=d["snr_db"], frames=d["frames"], frame_errors=d["frame_errors"],
                                      bit_errors=d["bit_errors"], info_bits=d["info_bits"],
                                      rounds=d.get("rounds", 0)).finalize()
        return done

    def run_point(self, snr_index: int, snr_db: float, num_frames: int, max_errors: int) -> PointResult:
        res = PointResult(snr_db=float(snr_db), frames=0, frame_errors=0, bit_errors=0, info_bits=self.info_bits)
        done = 0
        while done < num_frames and res.frame_errors < max_errors:
            round_total = min(self.batch * self.world, num_frames - done)
            start, count = shard(round_total, self.rank, self.world)
            local = np.zeros(3, dtype=np.int64)
            if count > 0:
                local = np.asarray(self.round_fn(snr_index, snr_db, done + start, count), dtype=np.int64)
            tot = self._allreduce(local)
            res.bit_errors += int(tot[0])
            res.frame_errors += int(tot[1])
            res.frames += int(tot[2])
            res.rounds += 1
            done += round_total
        return res.finalize()

    def run(self, snr_db_range: Sequence[float], num_frames: int, max_errors: int,
            log: "Optional[PointLog]" = None) -> List[PointResult]:
        """One PointResult per SNR point.  With a PointLog, points already in the
        log (same run key) are taken from it, and each new point is appended as
        soon as it finishes (rank 0), so an interrupted sweep resumes where it
        stopped.  Point i always draws the stream (seed, i, frame): a resumed
        sweep gives the same counts as an uninterrupted one."""
        done = self._finished(log)
        out = []
        for i, s in enumerate(snr_db_range):
            key = round(float(s), 9)
            if key in done:
                out.append(done[key])
                continue
            p = self.run_point(i, s, num_frames, max_errors)
            if log is not None and self.rank == 0:
                log.append(p)
            out.append(p)
        return out


class PointLog:
    """Append-only JSON-lines record of finished SNR points (SURVEY §5
    checkpoint / resume; the reference writes its results once at the end,
    src/utils/visualization.py:84-112).  Each row carries the run key (code,
    decoder, code construction digest, frames, max_errors, frames per round,
    seed, decoder library build id): rows of another configuration -- or of
    another build of the decoder library -- in the same file are ignored."""

    def __init__(self, path, key: dict):
        import json
        import os
        self.path = str(path)
        self.key = json.loads(json.dumps(key, sort_keys=True))
        d = os.path.dirname(self.path)
        if d:
            os.makedirs(d, exist_ok=True)

    def load(self):
        import json
        import os
        done = {}
        if not os.path.exists(self.path):
            return done
        with open(self.path) as f:
            for line in f:
                line = line.strip()
                if not line:
                    continue
                try:
                    row = json.loads(line)
                except ValueError:
                    continue  # a row cut short by an interruption
                if row.get("key") != self.key:
                    continue
                p = row["point"]
                r = PointResult(snr_db=p["snr_db"], frames=p["frames"], frame_errors=p["frame_errors"],
                                bit_errors=p["bit_errors"], info_bits=p["info_bits"], rounds=p.get("rounds", 0))
                done[round(float(r.snr_db), 9)] = r.finalize()
        return done

    def append(self, p: PointResult):
        import json
        import os
        with open(self.path, "ab+") as f:
            f.seek(0, os.SEEK_END)
            if f.tell() > 0:  # a torn last row (interrupted write) keeps its own line
                f.seek(-1, os.SEEK_END)
                if f.read(1) != b"\n":
                    f.write(b"\n")
            f.write((json.dumps({"key": self.key, "point": p.as_dict()}) + "\n").encode())
            f.flush()
            os.fsync(f.fileno())


# ---------------------------------------------------------------------------
# GPU round functions (device-resident frame source + decode + count)

def _stream_seed(seed: int, snr_index: int) -> int:
    return (int(seed) * 0x9E3779B97F4A7C15 + (snr_index + 1) * 0xBF58476D1CE4E5B9) & (2 ** 64 - 1)


def _polar_messages(msg, s, offset, K, crc_polynomial):
    """polar_round_fn's messages (its plain path stays as it was): random K bits; with crc_polynomial, data
    bits + their CRC on the device (pl_crc_append)."""
    from .. import _native
    _native.random_bits(s, offset, msg)
    if crc_polynomial is not None:
        from ..polar.utils import CRC_POLYNOMIALS
        name = crc_polynomial if crc_polynomial in CRC_POLYNOMIALS else "CRC-8"
        L = int(name.split("-")[1])
        _native.crc_append(msg, K - L, L, CRC_POLYNOMIALS[name])


def _qam_channel(modem, bits, E, nframes, snr_db, seed, offset, bufs, rx, fading=None):
    """The chains' channel with a channel.QAMModem: the E transmitted bits of each frame through modem.awgn
    (seed and frame offset as the BPSK call's) and modem.demap into rx [nframes, E], whose dtype the next
    stage reads.  The symbols live in bufs["sym"].  With fading, a coherence length in symbols, modem.rayleigh
    and modem.demap_csi instead, same seed and offset; the coefficients live in bufs["csi"].  The demapper is the
    modem's own (QAMModem's demapper: max-log, or the exact log-MAP)."""
    import torch
    S2 = 2 * modem.S(E)
    if "sym" not in bufs or bufs["sym"].shape[0] < nframes:
        bufs["sym"] = torch.empty((nframes, S2), dtype=torch.float64, device="cuda")
    sym = bufs["sym"][:nframes]
    if fading is None:
        modem.awgn(bits, E, nframes, snr_db, seed, frame_offset=offset, out=sym)
        modem.demap(sym, E, snr_db, out=rx)
        return
    if "csi" not in bufs or bufs["csi"].shape[0] < nframes:
        bufs["csi"] = torch.empty((nframes, 2 * modem.blocks(E, fading)), dtype=torch.float64, device="cuda")
    csi = bufs["csi"][:nframes]
    modem.rayleigh(bits, E, nframes, snr_db, seed, coherence=fading, frame_offset=offset, out=sym, h_out=csi)
    modem.demap_csi(sym, csi, E, snr_db, coherence=fading, out=rx)


def _channel(modem, ilv, bits, E, nframes, snr_db, seed, offset, bufs, rx, fading=None):
    """The chains' channel for the E transmitted bits of each frame, into rx [nframes, E]: BPSK
    (AWGNChannel.llr_batch_device) or, with a channel.QAMModem, _qam_channel (fading: its block Rayleigh
    fading, which _check_fading ties to a modem).  With a channel.BitInterleaver
    the bits are interleaved in front of it and the LLRs deinterleaved behind it, in rx's dtype; the
    interleaved bits and LLRs live in bufs["ilv_tx"] and bufs["ilv_rx"]."""
    if ilv is not None:
        import torch
        if "ilv_tx" not in bufs or bufs["ilv_tx"].shape[0] < nframes:
            bufs["ilv_tx"] = torch.empty((nframes, E), dtype=torch.uint8, device="cuda")
            bufs["ilv_rx"] = torch.empty((nframes, E), dtype=rx.dtype, device="cuda")
        out, rx = rx, bufs["ilv_rx"][:nframes]
        bits = ilv.interleave(bits, out=bufs["ilv_tx"][:nframes])
    if modem is None:
        from ..channel.awgn import AWGNChannel
        AWGNChannel(snr_db).llr_batch_device(bits, E, nframes, seed=seed, frame_offset=offset, out=rx)
    else:
        _qam_channel(modem, bits, E, nframes, snr_db, seed, offset, bufs, rx, fading)
    if ilv is not None:
        ilv.deinterleave(rx, out=out)


def _check_interleaver(ilv, E):
    assert ilv is None or ilv.E == E, "the interleaver's E = %d must be the transmitted length %d" % (ilv.E, E)


def _check_fading(fading, modem):
    assert fading is None or modem is not None, \
        "fading needs a modulation: the block-fading channel carries QAM symbols (QPSK is the 1-bit-per-axis case)"


def _polar_rate_matched_round_fn(decoder, seed, crc_polynomial, rm, modem=None, ilv=None, fading=None):
    """polar_round_fn's rate-matched chain; see there."""
    import torch
    from .. import _native
    N, K, E = decoder.N, decoder._n_info, rm.E
    assert decoder.N == rm.N, "the decoder and the rate matcher must share the mother code: N = %d" % rm.N
    rm.check_frozen(decoder.frozen_bits)
    _check_interleaver(ilv, E)
    bufs = {}

    def fn(snr_index, snr_db, offset, nframes):
        if bufs.get("B", 0) < nframes:
            bufs.update(B=nframes, msg=torch.empty((nframes, K), dtype=torch.uint8, device="cuda"),
                        cw=torch.empty((nframes, N), dtype=torch.uint8, device="cuda"),
                        tx=torch.empty((nframes, E), dtype=torch.uint8, device="cuda"),
                        rx=torch.empty((nframes, E), dtype=torch.float64, device="cuda"),
                        llr=torch.empty((nframes, N), dtype=torch.float64, device="cuda"),
                        out=torch.empty((nframes, K), dtype=torch.uint8, device="cuda"))
        msg, cw, tx, rx, llr, out = (bufs[k][:nframes] for k in ("msg", "cw", "tx", "rx", "llr", "out"))
        s = _stream_seed(seed, snr_index)
        _polar_messages(msg, s, offset, K, crc_polynomial)
        _native.polar_encode(decoder.plan, msg, cw)
        rm.select(cw, out=tx)
        _channel(modem, ilv, tx, E, nframes, snr_db, s ^ 0xA5A5A5A5, offset, bufs, rx, fading)
        rm.recover(rx, out=llr)
        decoder.plan.decode(llr, out)
        counts = torch.zeros(3, dtype=torch.int64, device="cuda")
        _native.count_errors(msg, out, K, counts)
        return counts.cpu().numpy()

    return fn


def polar_round_fn(decoder, seed: int = 0, crc_polynomial: Optional[str] = None, rate_matcher=None, modulation=None,
                   interleaver=None, fading=None):
    """Round function for a drop-in SC/SCL decoder (polar.SCDecoder/SCLDecoder).
    Random K-bit messages (CRC appended when crc_polynomial is given, as
    src/polar/encoder.py:74-78 does), device polar encoder, device AWGN,
    decode, device error count over the K decoded bits.

    rate_matcher = a polar.PolarRateMatcher of the decoder's N: only E bits of
    each frame cross the channel.  Messages (+ CRC), pl_polar_encode, select,
    AWGN over the E symbols (same seed derivation as without a matcher), recover
    to N fp64 LLRs, decode, count.  snr_db is per transmitted symbol (Es/N0), as
    in the LDPC chain: a repeated bit collects the energy of each copy.  The
    decoder's frozen set must contain rate_matcher.forced_frozen()
    (check_frozen; polar.construct_rate_matched builds one).

    modulation = a channel.QAMModem: the transmitted bits (the matcher's E, or the
    whole codeword) cross the channel as Gray-mapped QAM symbols, modem.awgn then
    modem.demap (max-log, fp64), with the seed derivation of the BPSK call; snr_db
    is then Es/N0 per QAM symbol.  None: BPSK, every call as before.

    interleaver = a channel.BitInterleaver whose E is the transmitted length (the
    matcher's E, or N): the chain becomes select, interleave, channel (BPSK or
    QAM), deinterleave, recover (include/polarldpc.h at pl_interleave_check).
    None: every call, seed and buffer as before.

    fading = a coherence length in symbols (1 .. 2^30; 2^30 is quasi-static): the
    QAM symbols cross block Rayleigh fading, modem.rayleigh then modem.demap_csi
    with the coefficients known at the receiver (include/polarldpc.h at
    pl_qam_fading_check), seed and offset as the AWGN call's.  It needs a
    modulation.  None: every count as before."""
    _check_fading(fading, modulation)
    if rate_matcher is not None:
        return _polar_rate_matched_round_fn(decoder, seed, crc_polynomial, rate_matcher, modulation, interleaver,
                                            fading)
    import torch
    from .. import _native
    N, K = decoder.N, decoder._n_info
    _check_interleaver(interleaver, N)
    bufs = {}

    def fn(snr_index, snr_db, offset, nframes):
        if bufs.get("B", 0) < nframes:
            bufs.update(B=nframes, msg=torch.empty((nframes, K), dtype=torch.uint8, device="cuda"),
                        cw=torch.empty((nframes, N), dtype=torch.uint8, device="cuda"),
                        llr=torch.empty((nframes, N), dtype=torch.float64, device="cuda"),
                        out=torch.empty((nframes, K), dtype=torch.uint8, device="cuda"))
        msg, cw, llr, out = (bufs[k][:nframes] for k in ("msg", "cw", "llr", "out"))
        s = _stream_seed(seed, snr_index)
        if crc_polynomial is None:
            _native.random_bits(s, offset, msg)
        else:  # data bits + their CRC, on the device (pl_crc_append)
            from ..polar.utils import CRC_POLYNOMIALS
            name = crc_polynomial if crc_polynomial in CRC_POLYNOMIALS else "CRC-8"
            L = int(name.split("-")[1])
            _native.random_bits(s, offset, msg)
            _native.crc_append(msg, K - L, L, CRC_POLYNOMIALS[name])
        _native.polar_encode(decoder.plan, msg, cw)
        _channel(modulation, interleaver, cw, N, nframes, snr_db, s ^ 0xA5A5A5A5, offset, bufs, llr, fading)
        decoder.plan.decode(llr, out)
        counts = torch.zeros(3, dtype=torch.int64, device="cuda")
        _native.count_errors(msg, out, K, counts)
        return counts.cpu().numpy()

    return fn


def _plan_decode(decoder, llr, out, its):
    """decoder.plan.decode(llr, out, its); a fixed-point decoder (ldpc.QCFixedMSDecoder) quantises the
    floating LLRs on the device first: the channel and the recovery stay floating."""
    if getattr(decoder.plan, "fixed", False):
        llr = decoder.quantize(llr)
    decoder.plan.decode(llr, out, its)


def _rate_matched_round_fn(decoder, seed, encoder, rm, modem=None, ilv=None, fading=None):
    """ldpc_round_fn's rate-matched chain; see there."""
    import torch
    from .. import _native
    from ..channel.awgn import AWGNChannel
    n_dec, E, kf = rm.n_dec, rm.E, rm.k - rm.fillers
    assert decoder.n == n_dec, "the decoder must be built on rate_matcher.decoder_base(): n = %d" % n_dec
    assert kf >= 1, "every message bit is a filler: no error to count"
    assert encoder is None or (encoder.n == rm.n and encoder.k == rm.k
                               and np.array_equal(encoder.info_positions, np.arange(rm.k))), \
        "the encoder must be the systematic encoder of the rate matcher's code"
    _check_interleaver(ilv, E)
    ftype = torch.float32 if np.dtype(getattr(decoder, "dtype", np.float64)) == np.float32 else torch.float64
    bufs = {}

    def fn(snr_index, snr_db, offset, nframes):
        if bufs.get("B", 0) < nframes:
            bufs.update(B=nframes, rx=torch.empty((nframes, E), dtype=torch.float64 if modem is None else ftype,
                                                  device="cuda"),
                        llr=torch.empty((nframes, n_dec), dtype=ftype, device="cuda"),
                        out=torch.empty((nframes, n_dec), dtype=torch.uint8, device="cuda"),
                        its=torch.empty((nframes,), dtype=torch.int32, device="cuda"),
                        zero=torch.zeros((nframes, kf), dtype=torch.uint8, device="cuda"),
                        msg=torch.empty((nframes, rm.k), dtype=torch.uint8, device="cuda"),
                        cw=torch.empty((nframes, rm.n), dtype=torch.uint8, device="cuda"),
                        tx=torch.empty((nframes, E), dtype=torch.uint8, device="cuda"))
        rx, llr, out, its, zero, msg, cw, tx = (bufs[x][:nframes] for x in ("rx", "llr", "out", "its", "zero", "msg",
                                                                            "cw", "tx"))
        s = _stream_seed(seed, snr_index)
        counts = torch.zeros(3, dtype=torch.int64, device="cuda")
        if encoder is None:
            AWGNChannel(snr_db).llr_batch_device(None, E, nframes, seed=s, frame_offset=offset, out=rx)
            ref = zero
        else:
            _native.random_bits(s, offset, msg)
            msg[:, kf:] = 0  # the fillers are known zeros
            encoder.encode_batch_device(msg, out=cw)
            rm.select(cw, out=tx)
            _channel(modem, ilv, tx, E, nframes, snr_db, s ^ 0xA5A5A5A5, offset, bufs, rx, fading)
            ref = msg
        rm.recover(rx, out=llr)
        _plan_decode(decoder, llr, out, its)
        _native.count_errors(ref, out, kf, counts)
        return counts.cpu().numpy()

    return fn


def ldpc_round_fn(decoder, seed: int = 0, info_bits: Optional[int] = None, encoder=None, rate_matcher=None,
                  modulation=None, interleaver=None, fading=None):
    """Round function for BPDecoder / MSDecoder / LayeredMSDecoder (any decoder
    with `.plan`, `.n` and `.m`).  A QCFixedMSDecoder takes the same chain: the
    channel LLRs (and the recovery) stay fp64 and the decoder quantises them.  A
    QCLayeredBPDecoder (sum-product, fp64) takes it as the fp64 min-sum decoders do.

    encoder None: the all-zero codeword (BP and min-sum are codeword-symmetric);
    errors over the first `info_bits` positions, like ber_simulation.py:265-269
    (decoded[:k]).  encoder = an LDPCEncoder: random k-bit messages (device
    Philox), valid codewords on the device (LDPCEncoder.encode_batch_device,
    pl_gf2_encode), errors over the encoder's info positions -- the whole Monte
    Carlo chain device-resident.

    rate_matcher = a ldpc.QCRateMatcher: only E bits of each frame cross the
    channel.  `decoder` is built on rate_matcher.decoder_base(), `encoder` (a
    QCLDPCEncoder of the whole code, or None) encodes random messages whose
    filler tail is zero; then select, AWGN over E, recover into the decoder's
    dtype, decode, errors over the first k - fillers positions (`info_bits` is
    not used).  With the all-zero codeword encode and select are skipped.

    modulation = a channel.QAMModem: the transmitted bits cross the channel as
    Gray-mapped QAM symbols (modem.awgn, modem.demap; polar_round_fn has the
    details); the demapper writes fp32 for a float32 decoder, else fp64.  A QAM
    bit channel is not symmetric -- a bit's error probability depends on the
    other bits of its symbol -- so the all-zero codeword stands for nothing:
    `encoder` is required.  None: BPSK, every call as before.

    interleaver = a channel.BitInterleaver whose E is the transmitted length (the
    matcher's E, or n): select, interleave, channel, deinterleave (in the dtype
    the channel wrote), recover.  The all-zero codeword shortcut transmits no
    bits to interleave, so `encoder` is required here too.  None: every call as
    before.

    fading = a coherence length in symbols: block Rayleigh fading of the QAM
    symbols with channel state at the demapper (polar_round_fn has the details);
    it needs a modulation.  None: every count as before."""
    _check_fading(fading, modulation)
    assert modulation is None or encoder is not None, \
        "modulation needs an encoder: the bit channels of a QAM symbol are not symmetric, so the all-zero " \
        "codeword shortcut is invalid"
    assert interleaver is None or encoder is not None, \
        "interleaver needs an encoder: the all-zero codeword shortcut transmits no bits to interleave"
    if rate_matcher is not None:
        return _rate_matched_round_fn(decoder, seed, encoder, rate_matcher, modulation, interleaver, fading)
    import torch
    from .. import _native
    from ..channel.awgn import AWGNChannel
    n = decoder.n
    _check_interleaver(interleaver, n)
    if encoder is not None:
        k = encoder.k
        info = torch.from_numpy(np.asarray(encoder.info_positions, dtype=np.int64)).cuda()
    else:
        k = info_bits if info_bits is not None else n - decoder.m
    f32 = modulation is not None and np.dtype(getattr(decoder, "dtype", np.float64)) == np.float32
    bufs = {}

    def fn(snr_index, snr_db, offset, nframes):
        if bufs.get("B", 0) < nframes:
            bufs.update(B=nframes, llr=torch.empty((nframes, n), dtype=torch.float32 if f32 else torch.float64,
                                                   device="cuda"),
                        out=torch.empty((nframes, n), dtype=torch.uint8, device="cuda"),
                        its=torch.empty((nframes,), dtype=torch.int32, device="cuda"),
                        zero=torch.zeros((nframes, n), dtype=torch.uint8, device="cuda"),
                        msg=torch.empty((nframes, k), dtype=torch.uint8, device="cuda"),
                        cw=torch.empty((nframes, n), dtype=torch.uint8, device="cuda"))
        llr, out, its, zero, msg, cw = (bufs[x][:nframes] for x in ("llr", "out", "its", "zero", "msg", "cw"))
        s = _stream_seed(seed, snr_index)
        counts = torch.zeros(3, dtype=torch.int64, device="cuda")
        if encoder is None:
            AWGNChannel(snr_db).llr_batch_device(None, n, nframes, seed=s, frame_offset=offset, out=llr)
            _plan_decode(decoder, llr, out, its)
            _native.count_errors(zero, out, k, counts)
        else:
            _native.random_bits(s, offset, msg)
            encoder.encode_batch_device(msg, out=cw)
            _channel(modulation, interleaver, cw, n, nframes, snr_db, s ^ 0xA5A5A5A5, offset, bufs, llr, fading)
            _plan_decode(decoder, llr, out, its)
            _native.count_errors(msg, out.index_select(1, info).contiguous(), k, counts)
        return counts.cpu().numpy()

    return fn


def stub_round_fn(seed: int = 0, info_bits: int = 16):
    """Deterministic CPU round function (tests and plumbing rehearsals only): the
    counts of frame f at SNR point i depend only on (seed, i, f), like the
    device round functions' Philox streams, so any sharding gives the same
    points.  Frame error iff hash(seed, i, f) % 1000 < 400 >> i; bit errors
    1 + f % 5 per erroneous frame."""
    def fn(snr_index, snr_db, offset, nframes):
        f = np.arange(offset, offset + nframes, dtype=np.uint64)
        h = (f * np.uint64(2654435761) + np.uint64((seed * 1000003 + snr_index * 97) & 0xFFFFFFFF)) % np.uint64(1000)
        err = h < np.uint64(400 >> min(snr_index, 16))
        bits = np.where(err, 1 + (f % np.uint64(5)), 0).astype(np.int64)
        return np.array([int(bits.sum()), int(err.sum()), int(nframes)], dtype=np.int64)
    return fn

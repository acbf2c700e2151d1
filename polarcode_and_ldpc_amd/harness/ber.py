"""Batched, multi-GPU counterpart of benchmarks/ber_simulation.py (:24-293).

`run_ber_simulation` keeps the reference's arguments and result layout
({'snr_db', 'polar': {'self': {'ber', 'fer'}}, 'ldpc': {'self': ...}} saved to
output_dir/data/ber_simulation_results.json) and adds per-point frame / error
counts with Wilson intervals.  Frames are generated, decoded and counted on the
device in rounds (harness/montecarlo.py): the max_errors stop is applied per
round, frames are sharded over the ranks of an initialised torch.distributed
group with one all-reduce of the counters per round.

Code choices follow the reference's simulate_* (:132-293): polar frozen set from
PolarLibWrapper(N, K, 2.0) (offline substitute: bit-reversed Bhattacharyya),
LDPC H from LDPCLibWrapper(n, k, dv, dc, seed=42) (offline substitute), BP with
max_iterations, errors over the k message positions.  LDPC frames use the
all-zero codeword (BP is codeword-symmetric) or, on request, random messages
through a device encoder; polar frames use random messages through the device
encoder.  simulate_qc_ldpc is the same for a quasi-cyclic code given by its base
matrix (layered min-sum, fp64, fp32 or int8 fixed point, or layered sum-product;
codewords from QCLDPCEncoder).
"""
from __future__ import annotations

from pathlib import Path
from typing import Dict, Optional, Sequence

import numpy as np

from ..utils.visualization import save_results
from .montecarlo import MonteCarlo, PointLog, ldpc_round_fn, polar_round_fn


def _digest(*arrays) -> str:
    import hashlib
    h = hashlib.sha1()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str(a.shape).encode())
        h.update(a.astype(np.int64).tobytes())
    return h.hexdigest()[:16]


def _log(log_path, mc, **key):
    """PointLog whose run key names everything a point's counts depend on: the
    code construction (digest of the frozen set / H), the decoder, the frame
    budget, the frames per round and the decoder library build."""
    if not log_path:
        return None
    from .. import _native
    return PointLog(log_path, dict(key, round_frames=mc.batch * mc.world, lib=_native.build_id()))


def _interleaver(interleaver, E, modulation):
    """simulate_*'s interleaver argument as a channel.BitInterleaver of the transmitted length E: one is
    checked against E; a (kind, rows) pair is built at E, rows None standing for the modem's bits per symbol
    (kind "rect") or for no rows (kind "tri")."""
    from ..channel.interleave import BitInterleaver
    if not isinstance(interleaver, BitInterleaver):
        kind, rows = interleaver
        if kind == "rect" and rows is None:
            assert modulation is not None, "a 'rect' interleaver needs its rows, or a modulation to take them from"
            rows = modulation.m
        interleaver = BitInterleaver(kind, E, rows=rows)
    assert interleaver.E == E, "the interleaver's E = %d must be the transmitted length %d" % (interleaver.E, E)
    return interleaver


def _demapper_key(modulation):
    """the run key's "demapper": present only for a modem whose demapper is not the default max-log"""
    return {"demapper": modulation.demapper} if modulation.demapper != "maxlog" else {}


def simulate_polar(snr_db_range: Sequence[float], num_frames: int, max_errors: int, config: Dict,
                   list_size: int = 0, crc_polynomial: Optional[str] = None, batch: int = 65536, seed: int = 0,
                   group=None, log_path=None, rate_match=None, modulation=None, interleaver=None, fading=None):
    """ber_simulation.py:132-198 -> (ber, fer, points).  list_size 0 = SC (the
    reference), >= 1 = SCL, with crc_polynomial = CA-SCL (CRC inside the K bits).
    log_path: JSON-lines file of finished points; a rerun resumes from it.

    rate_match: None, or a dict of PolarRateMatcher's arguments behind N (E, mode,
    sub_blocks, known_llr): E bits of each frame are transmitted
    (polar_round_fn's rate_matcher) and snr_db is per transmitted symbol.  The
    frozen set is config["frozen_bits"] when present, else
    construct_rate_matched(K, matcher) at its default design SNR.  E, mode, the
    permutation and known_llr enter the log's run key only when rate matching is
    used.

    modulation: None (BPSK), or a channel.QAMModem: the transmitted bits cross the
    channel as Gray-mapped QAM symbols (polar_round_fn's modulation) and snr_db is
    Es/N0 per QAM symbol; its bits per symbol enter the run key only when given.  A modem
    built with demapper="logmap" demaps with the exact log-MAP LLR, and "demapper" enters
    the run key only then.

    interleaver: None, a channel.BitInterleaver of the transmitted length (E, or N
    without rate matching) or a (kind, rows) pair to build one there (rows None:
    the modem's bits per symbol): polar_round_fn's interleaver.  [kind, rows]
    enters the run key, as "interleave", only when given.

    fading: None, or a coherence length in symbols: block Rayleigh fading of the QAM
    symbols with channel state at the demapper (polar_round_fn's fading; it needs a
    modulation).  It enters the run key, as "fading", only when given."""
    import torch
    from ..lib_wrappers import PolarLibWrapper
    from ..polar.decoder import CASCLDecoder, SCDecoder, SCLDecoder
    N, K = config["encoding"]["N"], config["encoding"]["K"]
    rm, more = None, {}
    if rate_match is not None:
        from ..polar.construction import construct_rate_matched
        from ..polar.ratematch import PolarRateMatcher
        rm = PolarRateMatcher(N, **rate_match)
        fr = config["frozen_bits"] if "frozen_bits" in config else construct_rate_matched(K, rm)
        more = dict(E=rm.E, mode=rm.mode, perm=rm.perm.tolist(), known_llr=rm.known_llr)
    else:
        fr = PolarLibWrapper(N, K, 2.0).get_frozen_bits_positions()
    kw = {}
    if modulation is not None:
        more = dict(more, modulation=modulation.m, **_demapper_key(modulation))
        kw["modulation"] = modulation
    if interleaver is not None:
        kw["interleaver"] = _interleaver(interleaver, rm.E if rm is not None else N, modulation)
        more = dict(more, interleave=kw["interleaver"].key)
    if fading is not None:
        kw["fading"] = int(fading)
        more = dict(more, fading=int(fading))
    if list_size <= 0:
        dec = SCDecoder(N, K, frozen_bits=fr)
    elif crc_polynomial:
        dec = CASCLDecoder(N, K, list_size, frozen_bits=fr, crc_polynomial=crc_polynomial)
    else:
        dec = SCLDecoder(N, K, list_size, frozen_bits=fr)
    mc = MonteCarlo(polar_round_fn(dec, seed=seed, crc_polynomial=crc_polynomial, rate_matcher=rm, **kw), info_bits=K,
                    batch=batch, group=group, device=torch.device("cuda", torch.cuda.current_device()))
    log = _log(log_path, mc, code="polar", N=N, K=K, list_size=list_size, crc=crc_polynomial, frames=num_frames,
               max_errors=max_errors, seed=seed, frozen=_digest(np.sort(np.asarray(fr))), **more)
    pts = mc.run(snr_db_range, num_frames, max_errors, log=log)
    return np.array([p.ber for p in pts]), np.array([p.fer for p in pts]), pts


def simulate_ldpc(snr_db_range: Sequence[float], num_frames: int, max_errors: int, config: Dict,
                  batch: int = 65536, seed: int = 0, group=None, random_codewords: bool = False, log_path=None):
    """ber_simulation.py:201-293 -> (ber, fer, points).  random_codewords: random
    messages encoded into valid codewords on the device (LDPCEncoder.
    encode_batch_device) instead of the all-zero codeword."""
    import torch
    from ..ldpc.decoder import BPDecoder
    from ..ldpc.encoder import LDPCEncoder
    from ..lib_wrappers import LDPCLibWrapper
    n, k = config["encoding"]["n"], config["encoding"]["k"]
    cons = config.get("construction", config["encoding"])
    lib = LDPCLibWrapper(n, k, dv=cons.get("dv", 3), dc=cons.get("dc", 6), seed=42)
    H = lib.get_parity_check_matrix()
    dec = BPDecoder(H, max_iter=config["decoding"].get("max_iterations", 50))
    enc = LDPCEncoder(n, lib.k, H=H) if random_codewords else None
    mc = MonteCarlo(ldpc_round_fn(dec, seed=seed, info_bits=lib.k, encoder=enc), info_bits=lib.k, batch=batch,
                    group=group, device=torch.device("cuda", torch.cuda.current_device()))
    log = _log(log_path, mc, code="ldpc", n=n, k=lib.k, max_iter=dec.max_iter, random=random_codewords,
               frames=num_frames, max_errors=max_errors, seed=seed, dv=cons.get("dv", 3), dc=cons.get("dc", 6),
               H=_digest(np.asarray(H) & 1))
    pts = mc.run(snr_db_range, num_frames, max_errors, log=log)
    return np.array([p.ber for p in pts]), np.array([p.fer for p in pts]), pts


def simulate_qc_ldpc(snr_db_range: Sequence[float], num_frames: int, max_errors: int, base, Z: int,
                     max_iter: int = 20, normalization: float = 0.75, dtype=np.float64, batch: int = 65536,
                     seed: int = 0, group=None, random_codewords: bool = False, log_path=None, rate_match=None,
                     fixed=None, modulation=None, interleaver=None, fading=None, algo: str = "minsum",
                     clip: float = 64.0):
    """simulate_ldpc for the quasi-cyclic code (base, Z): QCLayeredMSDecoder (layered
    normalised min-sum, early stop, state in `dtype`) on frames of the all-zero
    codeword or, random_codewords, of random messages encoded on the device from
    the base matrix (QCLDPCEncoder: base must have its structure, e.g. from
    qc_encodable_base).  H is never expanded.  -> (ber, fer, points), errors over
    the k = (nb - mb) Z message positions.

    rate_match: None, or QCRateMatcher's arguments behind (base, Z) -- a dict, or
    the sequence (E, punctured, fillers[, ncb[, start]]): E bits of each frame are
    transmitted (ldpc_round_fn's rate_matcher), the decoder works on the
    matcher's decoder_base(), errors over the k - fillers message positions.

    fixed: None, or (llr_scale, llr_max, msg_max): the int8 fixed-point decoder
    QCFixedMSDecoder with these parameters instead (`dtype` is not used; the
    channel LLRs stay fp64 and the decoder quantises them).  The three values
    enter the log's run key, as "fixed", only when given.

    modulation: None (BPSK), or a channel.QAMModem (ldpc_round_fn's modulation; it needs
    random_codewords); snr_db is then Es/N0 per QAM symbol, and its bits per symbol enter the
    run key.

    interleaver: as simulate_polar's (the transmitted length is the matcher's E, or n);
    ldpc_round_fn's interleaver, which needs random_codewords.

    fading: as simulate_polar's (ldpc_round_fn's fading).

    algo: "minsum" (the default: the decoders above), or "bp": the layered sum-product
    decoder QCLayeredBPDecoder with the clamp `clip` instead (fp64; `normalization`,
    `dtype` are not used and `fixed` must be None).  "algo" and "clip" enter the log's
    run key only with "bp"."""
    import torch
    from ..ldpc.decoder import QCFixedMSDecoder, QCLayeredBPDecoder, QCLayeredMSDecoder
    from ..ldpc.encoder import QCLDPCEncoder
    base = np.asarray(base, dtype=np.int64)
    more = {}
    if fixed is not None:
        fixed = (float(fixed[0]), int(fixed[1]), int(fixed[2]))
        more["fixed"] = list(fixed)
    if algo not in ("minsum", "bp"):
        raise ValueError("simulate_qc_ldpc: algo must be 'minsum' or 'bp', not %r" % (algo,))
    if algo == "bp":
        if fixed is not None:
            raise ValueError("simulate_qc_ldpc: algo='bp' is fp64; it does not go with fixed=")
        more["algo"], more["clip"] = "bp", float(clip)
    kw = {}
    if modulation is not None:
        more["modulation"] = modulation.m
        more.update(_demapper_key(modulation))
        kw["modulation"] = modulation
    if fading is not None:
        more["fading"] = kw["fading"] = int(fading)

    def with_interleaver(E):
        if interleaver is not None:
            kw["interleaver"] = _interleaver(interleaver, E, modulation)
            more["interleave"] = kw["interleaver"].key

    def make_decoder(b):
        if algo == "bp":
            return QCLayeredBPDecoder(b, Z, max_iter=max_iter, early_stop=True, clip=clip)
        if fixed is None:
            return QCLayeredMSDecoder(b, Z, max_iter=max_iter, normalization=normalization, early_stop=True, dtype=dtype)
        return QCFixedMSDecoder(b, Z, max_iter=max_iter, normalization=normalization, early_stop=True,
                                llr_scale=fixed[0], llr_max=fixed[1], msg_max=fixed[2])

    def dtype_name(dec):
        return "int8" if fixed is not None else np.dtype(getattr(dec, "dtype", np.float64)).name
    if rate_match is not None:
        from ..ldpc.ratematch import QCRateMatcher
        rm = QCRateMatcher(base, Z, **rate_match) if isinstance(rate_match, dict) else QCRateMatcher(base, Z, *rate_match)
        dec = make_decoder(rm.decoder_base())
        k = rm.k - rm.fillers
        with_interleaver(rm.E)
        enc = QCLDPCEncoder(base, Z) if random_codewords else None
        mc = MonteCarlo(ldpc_round_fn(dec, seed=seed, encoder=enc, rate_matcher=rm, **kw), info_bits=k, batch=batch,
                        group=group, device=torch.device("cuda", torch.cuda.current_device()))
        log = _log(log_path, mc, code="qcldpc", n=rm.n, k=k, Z=int(Z), max_iter=max_iter, norm=float(normalization),
                   dtype=dtype_name(dec), random=random_codewords, frames=num_frames, max_errors=max_errors,
                   seed=seed, base=_digest(base + 1), rm=[rm.E, rm.punctured, rm.fillers, rm.ncb, rm.start],
                   filler_llr=rm.filler_llr, n_dec=rm.n_dec, **more)
        pts = mc.run(snr_db_range, num_frames, max_errors, log=log)
        return np.array([p.ber for p in pts]), np.array([p.fer for p in pts]), pts
    dec = make_decoder(base)
    k = dec.n - dec.m
    with_interleaver(dec.n)
    enc = QCLDPCEncoder(base, Z) if random_codewords else None
    mc = MonteCarlo(ldpc_round_fn(dec, seed=seed, info_bits=k, encoder=enc, **kw), info_bits=k, batch=batch, group=group,
                    device=torch.device("cuda", torch.cuda.current_device()))
    log = _log(log_path, mc, code="qcldpc", n=dec.n, k=k, Z=int(Z), max_iter=max_iter, norm=float(normalization),
               dtype=dtype_name(dec), random=random_codewords, frames=num_frames, max_errors=max_errors,
               seed=seed, base=_digest(base + 1), **more)
    pts = mc.run(snr_db_range, num_frames, max_errors, log=log)
    return np.array([p.ber for p in pts]), np.array([p.fer for p in pts]), pts


def run_ber_simulation(snr_db_range: np.ndarray, num_frames: int, max_errors: int, polar_config: Dict,
                       ldpc_config: Dict, output_dir: Path, use_third_party: bool = False, batch: int = 65536,
                       list_size: int = 0, crc_polynomial: Optional[str] = None, resume: bool = False) -> Dict:
    """ber_simulation.py:296-... -> results dict (also saved as JSON).  resume:
    keep per-point rows in output_dir/data/ber_points.jsonl and take finished
    points from it (opt-in: a fresh call always simulates)."""
    snr = np.asarray(snr_db_range, dtype=float)
    results = {"snr_db": snr.tolist(), "polar": {}, "ldpc": {}}
    points = Path(output_dir) / "data" / "ber_points.jsonl" if resume else None
    pb, pf, pp = simulate_polar(snr, num_frames, max_errors, polar_config, list_size, crc_polynomial, batch,
                                log_path=points)
    results["polar"]["self"] = {"ber": pb.tolist(), "fer": pf.tolist(), "points": [p.as_dict() for p in pp]}
    lb, lf, lp = simulate_ldpc(snr, num_frames, max_errors, ldpc_config, batch, log_path=points)
    results["ldpc"]["self"] = {"ber": lb.tolist(), "fer": lf.tolist(), "points": [p.as_dict() for p in lp]}
    if use_third_party:
        print("Warning: third-party libraries (polarcodes, pyldpc) are not available offline")
    save_results(results, Path(output_dir) / "data" / "ber_simulation_results.json")
    return results


def _parse_range(s: str):
    a, b, c = (float(x) for x in s.split(":"))
    return np.arange(a, b + c / 2, c)


def main(argv=None):
    """CLI (one process per GPU under torchrun; RCCL all-reduce of the counters):
    python -m polarcode_and_ldpc_amd.harness.ber --code polar --N 1024 --K 512 \\
        --list-size 32 --crc CRC-8 --snr=-2:5:1 --frames 1000000 --max-errors 100
    python -m polarcode_and_ldpc_amd.harness.ber --code qcldpc --qc 12,24,81,3,1 --ldpc-codewords random \\
        --dtype float32 --norm 0.75 --snr=-1.25:-0.75:0.25 --frames 524288 --max-errors 1000000"""
    import argparse
    import json
    import os
    import torch
    import torch.distributed as dist
    ap = argparse.ArgumentParser()
    ap.add_argument("--code", choices=["polar", "ldpc", "qcldpc"], default="polar")
    ap.add_argument("--N", type=int, default=1024)
    ap.add_argument("--K", type=int, default=512)
    ap.add_argument("--list-size", type=int, default=0)
    ap.add_argument("--crc", default=None)
    ap.add_argument("--n", type=int, default=504)
    ap.add_argument("--k", type=int, default=252)
    ap.add_argument("--max-iter", type=int, default=20)
    ap.add_argument("--snr", default="-2:5:1")
    ap.add_argument("--frames", type=int, default=1 << 20)
    ap.add_argument("--max-errors", type=int, default=100)
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--out", default=None)
    ap.add_argument("--log", "--resume-log", dest="log", default=None,
                    help="JSON-lines file of finished SNR points; a rerun resumes from it (under torchrun spell it "
                         "--resume-log: torchrun's own parser takes --log for an abbreviation of --log-dir)")
    ap.add_argument("--ldpc-codewords", choices=["zero", "random"], default="zero",
                    help="LDPC frames: all-zero codeword, or random messages encoded on the device")
    ap.add_argument("--qc", default="12,24,81,3,1",
                    help="--code qcldpc: mb,nb,Z,dv,seed[,core], the code qc_encodable_base(mb, nb, Z, dv, seed, core)")
    ap.add_argument("--rm", default=None,
                    help="--code qcldpc: E,punctured,fillers[,ncb[,start]], rate matching (ldpc.QCRateMatcher): E bits "
                         "of each frame are transmitted")
    ap.add_argument("--polar-rm", default=None,
                    help="--code polar: E,mode[,p0,p1,...], rate matching (polar.PolarRateMatcher): E bits of each "
                         "frame are transmitted; mode puncture or shorten; p0,p1,... the sub-block permutation")
    ap.add_argument("--dtype", choices=["float64", "float32"], default="float64",
                    help="--code qcldpc: the decoder's state and arithmetic")
    ap.add_argument("--fixed", default=None,
                    help="--code qcldpc: scale,llr_max,msg_max, the int8 fixed-point decoder (ldpc.QCFixedMSDecoder) "
                         "instead of the floating one; --dtype is then not used")
    ap.add_argument("--qc-algo", choices=["minsum", "bp"], default="minsum",
                    help="--code qcldpc: the check rule, normalised min-sum (the default) or sum-product "
                         "(ldpc.QCLayeredBPDecoder, fp64; --norm, --dtype are then not used)")
    ap.add_argument("--clip", type=float, default=64.0, help="--qc-algo bp: the clamp of the messages")
    ap.add_argument("--modulation", choices=["qpsk", "16qam", "64qam", "256qam"], default=None,
                    help="--code polar, qcldpc: Gray-mapped QAM (channel.QAMModem) instead of BPSK; --snr is then Es/N0 "
                         "per QAM symbol; qcldpc needs --ldpc-codewords random")
    ap.add_argument("--demapper", choices=["maxlog", "logmap"], default=None,
                    help="with --modulation: the soft demapper, max-log (the default) or the exact log-MAP LLR")
    ap.add_argument("--interleave", choices=["rect", "tri"], default=None,
                    help="--code polar, qcldpc: a bit interleaver (channel.BitInterleaver) between rate matching and "
                         "the channel: row-column or triangular; qcldpc needs --ldpc-codewords random")
    ap.add_argument("--interleave-rows", type=int, default=None,
                    help="--interleave rect: its rows; default: the bits per symbol of --modulation")
    ap.add_argument("--fading", default=None, metavar="LC",
                    help="with --modulation: block Rayleigh fading with channel state at the demapper; LC is the "
                         "coherence length in symbols (1: fast fading), or 'frame' for one coefficient a frame")
    ap.add_argument("--norm", type=float, default=0.75, help="--code qcldpc: min-sum normalisation")
    ap.add_argument("--seed", type=int, default=0, help="--code qcldpc: seed of the frame source")
    ap.add_argument("--cpu-stub", action="store_true",
                    help="plumbing check on CPU: gloo ranks and a deterministic stub round function "
                         "(montecarlo.stub_round_fn) instead of the device decoders; not a simulation")
    a = ap.parse_args(argv)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if not a.cpu_stub:
        torch.cuda.set_device(local)
    if world > 1:
        if a.cpu_stub:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    snr = _parse_range(a.snr)
    mod = {}
    if a.demapper is not None and a.modulation is None:
        ap.error("--demapper needs --modulation")
    if a.modulation is not None and not a.cpu_stub:
        if a.code == "ldpc":
            ap.error("--modulation goes with --code polar or qcldpc")
        from ..channel.qam import NAMES, QAMModem
        mod["modulation"] = QAMModem(NAMES[a.modulation], demapper=a.demapper or "maxlog")
    if a.fading is not None:
        if a.fading != "frame" and not a.fading.isdigit():
            ap.error("--fading takes a coherence length in symbols, or 'frame'")
        if a.modulation is None:
            ap.error("--fading needs --modulation")
        if not a.cpu_stub:
            mod["fading"] = 1 << 30 if a.fading == "frame" else int(a.fading)
    if a.interleave is not None and not a.cpu_stub:
        if a.code == "ldpc":
            ap.error("--interleave goes with --code polar or qcldpc")
        if a.interleave == "rect" and a.interleave_rows is None and a.modulation is None:
            ap.error("--interleave rect needs --interleave-rows or --modulation")
        if a.interleave == "tri" and a.interleave_rows is not None:
            ap.error("--interleave-rows goes with --interleave rect")
        mod["interleaver"] = (a.interleave, a.interleave_rows)
    if a.cpu_stub:
        from .montecarlo import stub_round_fn
        mc = MonteCarlo(stub_round_fn(seed=7, info_bits=a.K), info_bits=a.K, batch=a.batch)
        log = _log(a.log, mc, code="stub", K=a.K, frames=a.frames, max_errors=a.max_errors,
                   **({"demapper": a.demapper} if a.demapper == "logmap" else {}))
        pts = mc.run(snr, a.frames, a.max_errors, log=log)
        ber, fer = np.array([p.ber for p in pts]), np.array([p.fer for p in pts])
    elif a.code == "polar":
        more = {}
        if a.polar_rm is not None:
            f = a.polar_rm.split(",")
            if len(f) < 2 or f[1] not in ("puncture", "shorten"):
                ap.error("--polar-rm takes E,mode[,p0,p1,...] with mode puncture or shorten")
            more["rate_match"] = dict(E=int(f[0]), mode=f[1], sub_blocks=[int(x) for x in f[2:]] or None)
        ber, fer, pts = simulate_polar(snr, a.frames, a.max_errors, {"encoding": {"N": a.N, "K": a.K}},
                                       a.list_size, a.crc, a.batch, log_path=a.log, **more, **mod)
    elif a.code == "qcldpc":
        from ..ldpc.matrix import qc_encodable_base
        q = [int(x) for x in a.qc.split(",")]
        if len(q) not in (5, 6):
            ap.error("--qc takes mb,nb,Z,dv,seed[,core]")
        base = qc_encodable_base(*q[:5], core=q[5] if len(q) == 6 else None)
        rm = None
        if a.rm is not None:
            rm = [int(x) for x in a.rm.split(",")]
            if len(rm) not in (3, 4, 5):
                ap.error("--rm takes E,punctured,fillers[,ncb[,start]]")
        more = {} if rm is None else {"rate_match": rm}
        if a.fixed is not None:
            fx = a.fixed.split(",")
            if len(fx) != 3:
                ap.error("--fixed takes scale,llr_max,msg_max")
            more["fixed"] = (float(fx[0]), int(fx[1]), int(fx[2]))
        if a.qc_algo == "bp":
            if a.fixed is not None:
                ap.error("--qc-algo bp does not go with --fixed")
            more.update(algo="bp", clip=a.clip)
        ber, fer, pts = simulate_qc_ldpc(snr, a.frames, a.max_errors, base, q[2], max_iter=a.max_iter,
                                         normalization=a.norm, dtype=np.dtype(a.dtype).type, batch=a.batch,
                                         seed=a.seed, random_codewords=a.ldpc_codewords == "random", log_path=a.log,
                                         **more, **mod)
    else:
        ber, fer, pts = simulate_ldpc(snr, a.frames, a.max_errors,
                                      {"encoding": {"n": a.n, "k": a.k}, "decoding": {"max_iterations": a.max_iter}},
                                      a.batch, random_codewords=a.ldpc_codewords == "random", log_path=a.log)
    if int(os.environ.get("RANK", "0")) == 0:
        res = {"code": a.code, "snr_db": snr.tolist(), "ber": ber.tolist(), "fer": fer.tolist(), "gpus": world,
               "points": [p.as_dict() for p in pts]}
        print(json.dumps(res))
        if a.out:
            save_results(res, a.out)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()

"""Exact log-MAP demapper timing (diagnostic): HIP events around repeated launches.

usage: python tools/qam_logmap_bench.py [--E 1024] [--batch 65536] [--m 4,6,8] [--reps 5] [--rounds 20] [--snr-per-bit 1.5]

At `batch` frames of E transmitted bits, for each m bits per symbol and for fp32 and fp64 LLRs, in the same rounds,
alternated: the max-log and the log-MAP demapper on the same received symbols -- `demap` (qam_demap_kernel and
qam_demap_logmap_kernel without channel state) on AWGN symbols, `demap_csi` (qam_demap_csi_kernel and
qam_demap_logmap_kernel with it) on block-faded symbols at coherence lengths 1 and 16.  The Es/N0 is m times
--snr-per-bit dB (6, 9, 12 dB by default): a waterfall-like point, where the neighbouring levels' terms are
computed and not skipped.  One warm-up call each, then `rounds` rounds of `reps` launches; one JSON line per
group gives each kernel's median per-launch time with its spread and the ratio to max-log's.  The LLRs of every
run are compared with the sent bits, so a run that times garbage fails."""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from polarcode_and_ldpc_amd import _native
from polarcode_and_ldpc_amd.channel import QAMModem

ap = argparse.ArgumentParser()
ap.add_argument("--E", type=int, default=1024)
ap.add_argument("--batch", type=int, default=65536)
ap.add_argument("--m", default="4,6,8")
ap.add_argument("--reps", type=int, default=5, help="launches per timed round")
ap.add_argument("--rounds", type=int, default=20)
ap.add_argument("--snr-per-bit", type=float, default=1.5, help="Es/N0 in dB = m times this")
a = ap.parse_args()
E, B, LCS = a.E, a.batch, (1, 16)


def timed(fn, reps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / reps


def race(fns):
    """name -> per-launch times: one warm-up each, then rounds of reps launches, alternated"""
    for f in fns.values():
        f()
    torch.cuda.synchronize()
    t = {name: [] for name in fns}
    for _ in range(a.rounds):
        for name, f in fns.items():
            t[name].append(timed(f, a.reps))
    return t


bits = torch.empty((B, E), dtype=torch.uint8, device="cuda")
_native.random_bits(4243, 0, bits)
for m in (int(x) for x in a.m.split(",")):
    modem, snr = QAMModem(m), m * a.snr_per_bit
    S = modem.S(E)
    sym = {None: modem.awgn(bits, E, B, snr, 7, 0)}
    csi = {}
    for Lc in LCS:
        sym[Lc], csi[Lc] = modem.rayleigh(bits, E, B, snr, 7, coherence=Lc)
    for dt in (torch.float32, torch.float64):
        for Lc in (None,) + LCS:
            llr = {k: torch.empty((B, E), dtype=dt, device="cuda") for k in ("maxlog", "logmap")}
            if Lc is None:
                fns = {k: (lambda k=k: modem.demap(sym[None], E, snr, out=llr[k], method=k)) for k in llr}
            else:
                fns = {k: (lambda k=k: modem.demap_csi(sym[Lc], csi[Lc], E, snr, coherence=Lc, out=llr[k], method=k))
                       for k in llr}
            t = race(fns)
            first = float(np.median(t["maxlog"]))
            rows = {k: dict(ms=float(np.median(v)), ms_min=min(v), ms_max=max(v), over_maxlog=float(np.median(v)) / first)
                    for k, v in t.items()}
            print(json.dumps(dict(group="awgn" if Lc is None else "csi_lc%d" % Lc, m=m, E=E, batch=B, snr_db=snr,
                                  llr=str(dt).split(".")[-1], rounds=a.rounds, reps=a.reps, kernels=rows)), flush=True)
            agree = {k: float(((v <= 0).to(torch.uint8) == (bits & 1)).float().mean()) for k, v in llr.items()}
            assert min(agree.values()) > 0.7, "the LLRs disagree with the sent bits: %s" % agree
            assert abs(agree["maxlog"] - agree["logmap"]) < 0.01, agree
            del llr

"""Block-fading QAM timing (diagnostic): HIP events around repeated launches.

usage: python tools/qam_fading_bench.py [--E 1024] [--batch 65536] [--m 6] [--reps 5] [--rounds 20] [--snr 20.0]

At `batch` frames of E transmitted bits and m bits per symbol, in the same rounds, alternated:
the two demappers on the same received symbols -- `demap` (qam_demap_kernel) and `demap_csi`
(qam_demap_csi_kernel) at coherence lengths 1 and 16 -- with fp32 and with fp64 LLRs, and the two
transmit kernels, `awgn` (qam_tx_kernel with noise) and `rayleigh` (qam_rayleigh_kernel) at the same
coherence lengths.  One warm-up call each, then `rounds` rounds of `reps` launches; one JSON line per
group gives each kernel's median per-launch time with its spread and the ratio to the group's first.
The LLRs of the two demappers' runs are compared with the sent bits, so a run that times garbage
fails."""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from polarcode_and_ldpc_amd import _native
from polarcode_and_ldpc_amd.channel import QAMModem

ap = argparse.ArgumentParser()
ap.add_argument("--E", type=int, default=1024)
ap.add_argument("--batch", type=int, default=65536)
ap.add_argument("--m", type=int, default=6)
ap.add_argument("--reps", type=int, default=5, help="launches per timed round")
ap.add_argument("--rounds", type=int, default=20)
ap.add_argument("--snr", type=float, default=20.0, help="Es/N0 in dB")
a = ap.parse_args()
E, B, LCS = a.E, a.batch, (1, 16)
modem = QAMModem(a.m)
S = modem.S(E)


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


def report(group, t, **more):
    first = float(np.median(next(iter(t.values()))))
    rows = {name: dict(ms=float(np.median(v)), ms_min=min(v), ms_max=max(v), over_first=float(np.median(v)) / first)
            for name, v in t.items()}
    print(json.dumps(dict(group=group, m=a.m, E=E, batch=B, rounds=a.rounds, reps=a.reps, **more, kernels=rows)), flush=True)


bits = torch.empty((B, E), dtype=torch.uint8, device="cuda")
_native.random_bits(4243, 0, bits)
sym = torch.empty((B, 2 * S), dtype=torch.float64, device="cuda")
csi = {Lc: torch.empty((B, 2 * modem.blocks(E, Lc)), dtype=torch.float64, device="cuda") for Lc in LCS}
faded = {Lc: torch.empty_like(sym) for Lc in LCS}

tx = {"awgn": lambda: modem.awgn(bits, E, B, a.snr, 7, 0, out=sym)}
for Lc in LCS:
    tx["rayleigh_lc%d" % Lc] = lambda Lc=Lc: modem.rayleigh(bits, E, B, a.snr, 7, coherence=Lc, out=faded[Lc], h_out=csi[Lc])
report("transmit", race(tx))

for dt in (torch.float32, torch.float64):
    llr = {name: torch.empty((B, E), dtype=dt, device="cuda") for name in ["demap"] + ["demap_csi_lc%d" % Lc for Lc in LCS]}
    rx = {"demap": lambda: modem.demap(sym, E, a.snr, out=llr["demap"])}
    for Lc in LCS:
        rx["demap_csi_lc%d" % Lc] = lambda Lc=Lc: modem.demap_csi(faded[Lc], csi[Lc], E, a.snr, coherence=Lc,
                                                                  out=llr["demap_csi_lc%d" % Lc])
    report("demap", race(rx), llr=str(dt).split(".")[-1],
           bytes_read_plus_written=dict(demap=B * (2 * S * 8 + E * llr["demap"].element_size()),
                                        **{"demap_csi_lc%d" % Lc: B * (2 * S * 8 + csi[Lc].shape[1] * 8
                                                                       + E * llr["demap"].element_size()) for Lc in LCS}))
    for name, v in llr.items():
        agree = float(((v <= 0).to(torch.uint8) == (bits & 1)).float().mean())
        assert agree > 0.9, "%s disagrees with the sent bits: %.3f" % (name, agree)
    del llr

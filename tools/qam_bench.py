"""Gray-mapped QAM timing (diagnostic): HIP events around repeated launches.

usage: python tools/qam_bench.py [--E 1024] [--batch 65536] [--reps 5] [--rounds 20] [--snr 10.0]

Timed at `batch` frames of E transmitted bits, for m = 4 and m = 8 bits per symbol:
`modulate` (qam_tx_kernel without noise), `awgn` (qam_tx_kernel with noise) and `demap`
(qam_demap_kernel) with fp64 and with fp32 LLRs.  Each runs against two yardsticks in the
same rounds, alternated: `bpsk`, pl_awgn_llr over the same E bits (one LLR a bit: the chain
without a modem), and `copy`, one device-to-device copy (torch's copy_ of a contiguous
uint8 tensor) that moves the kernel's bytes read plus written, that is a copy of half of
them.  One warm-up call each, then `rounds` rounds of `reps` launches; one JSON line per
measurement gives the median and the spread of the per-launch time, the bytes moved over
it, and the ratios of the medians."""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from polarcode_and_ldpc_amd import _native
from polarcode_and_ldpc_amd.channel import AWGNChannel, QAMModem

ap = argparse.ArgumentParser()
ap.add_argument("--E", type=int, default=1024)
ap.add_argument("--batch", type=int, default=65536)
ap.add_argument("--reps", type=int, default=5, help="launches per timed round")
ap.add_argument("--rounds", type=int, default=20)
ap.add_argument("--snr", type=float, default=10.0, help="Es/N0 in dB")
a = ap.parse_args()
E, B = a.E, a.batch


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


def copy_of(moved):
    src = torch.empty(moved // 2, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    return lambda: dst.copy_(src)


bits = torch.empty((B, E), dtype=torch.uint8, device="cuda")
_native.random_bits(4243, 0, bits)
bpsk_llr = torch.empty((B, E), dtype=torch.float64, device="cuda")


def bpsk():
    AWGNChannel(a.snr).llr_batch_device(bits, E, B, seed=7, frame_offset=0, out=bpsk_llr)


def report(op, m, t, moved, **more):
    k, c, p = (float(np.median(t[x])) for x in ("kernel", "copy", "bpsk"))
    print(json.dumps(dict(op=op, m=m, E=E, batch=B, bytes_read_plus_written=moved, kernel_ms=k,
                          kernel_ms_min=min(t["kernel"]), kernel_ms_max=max(t["kernel"]), kernel_gbps=moved / k / 1e6,
                          copy_ms=c, copy_gbps=moved / c / 1e6, kernel_over_copy=k / c, bpsk_awgn_llr_ms=p,
                          kernel_ns_per_bit=k * 1e6 / (B * E), bpsk_ns_per_bit=p * 1e6 / (B * E), rounds=a.rounds,
                          reps=a.reps, **more)), flush=True)


for m in (4, 8):
    modem = QAMModem(m)
    S2 = 2 * modem.S(E)
    sym = torch.empty((B, S2), dtype=torch.float64, device="cuda")
    moved = B * (E + S2 * 8)
    report("modulate", m, race({"kernel": lambda: modem.modulate(bits, out=sym), "copy": copy_of(moved), "bpsk": bpsk}),
           moved)
    report("awgn", m, race({"kernel": lambda: modem.awgn(bits, E, B, a.snr, 7, 0, out=sym), "copy": copy_of(moved),
                            "bpsk": bpsk}), moved)
    for dt in (torch.float64, torch.float32):
        llr = torch.empty((B, E), dtype=dt, device="cuda")
        moved = B * (S2 * 8 + E * llr.element_size())
        report("demap", m, race({"kernel": lambda: modem.demap(sym, E, a.snr, out=llr), "copy": copy_of(moved),
                                 "bpsk": bpsk}), moved, llr=str(dt).split(".")[-1])
        ok = bool(((llr <= 0).to(torch.uint8) == (bits & 1)).float().mean() > 0.5)
        assert ok, "demap disagrees with the sent bits"
        del llr
    del sym

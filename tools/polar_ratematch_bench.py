"""Polar rate matching timing (diagnostic): HIP events around repeated launches.

usage: python tools/polar_ratematch_bench.py [--N 1024] [--batch 65536] [--reps 5] [--rounds 20] [--step]
                                             [--list-size 8] [--snr 1.0]

Timed at N and `batch` frames, sub-block permutation of 32 (a fixed shuffle):
`recover` (polar_rate_recover_kernel, fp64 LLRs) at E = 3N/4, puncture, and at
E = 3N/2, and `select` (polar_rate_match_kernel) at E = 3N/4.  Each runs against
the yardstick: one device-to-device copy (torch's copy_ of a contiguous uint8
tensor, a hipMemcpyAsync) that moves the same number of bytes read plus written,
that is a copy of (read + written) / 2 bytes.  One warm-up call each, then
`rounds` rounds of `reps` launches, kernel and copy alternated; one JSON line per
measurement gives the median and the spread of the per-launch time and the ratio
of the medians.
--step: one Monte Carlo step of harness.polar_round_fn's rate-matched chain at
E = 3N/4, K = E/2 -- random bits, encode, select, AWGN LLRs over E, recover, SCL
decode, error count -- with events between the stages; the median of `rounds`
steps and the share of select and recover."""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from polarcode_and_ldpc_amd import _native
from polarcode_and_ldpc_amd.channel import AWGNChannel
from polarcode_and_ldpc_amd.polar import PolarRateMatcher, SCLDecoder, construct_rate_matched

ap = argparse.ArgumentParser()
ap.add_argument("--N", type=int, default=1024)
ap.add_argument("--batch", type=int, default=65536)
ap.add_argument("--reps", type=int, default=5, help="launches per timed round")
ap.add_argument("--rounds", type=int, default=20)
ap.add_argument("--step", action="store_true", help="also time one Monte Carlo step")
ap.add_argument("--list-size", type=int, default=8)
ap.add_argument("--snr", type=float, default=1.0, help="--step: Es/N0 in dB")
a = ap.parse_args()
N, B = a.N, a.batch
PERM = [13, 2, 8, 0, 19, 5, 16, 11, 3, 21, 9, 18, 6, 14, 1, 17, 10, 4, 15, 7, 20, 12, 27, 31, 22, 30, 24, 29, 26, 23, 28, 25]


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


def report(op, rm, t, moved):
    k, c = float(np.median(t["kernel"])), float(np.median(t["copy"]))
    print(json.dumps({"op": op, "N": N, "E": rm.E, "mode": rm.mode, "batch": B, "bytes_read_plus_written": moved,
                      "kernel_ms": k, "kernel_ms_min": min(t["kernel"]), "kernel_ms_max": max(t["kernel"]),
                      "copy_ms": c, "copy_ms_min": min(t["copy"]), "copy_ms_max": max(t["copy"]),
                      "kernel_over_copy": k / c, "kernel_gbps": moved / k / 1e6, "copy_gbps": moved / c / 1e6,
                      "rounds": a.rounds, "reps": a.reps}), flush=True)


def copy_of(moved):
    src = torch.empty(moved // 2, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    return lambda: dst.copy_(src)


cw = torch.empty((B, N), dtype=torch.uint8, device="cuda")
_native.random_bits(4243, 0, cw)
for E, mode in ((3 * N // 4, "puncture"), (3 * N // 2, "puncture")):
    rm = PolarRateMatcher(N, E, mode, PERM)
    llr = torch.randn((B, E), dtype=torch.float64, device="cuda")
    out = torch.empty((B, N), dtype=torch.float64, device="cuda")
    moved = B * (E + N) * 8
    report("recover", rm, race({"kernel": lambda: rm.recover(llr, out=out), "copy": copy_of(moved)}), moved)
    if rm.max_reps == 1:
        idx = torch.from_numpy(rm.positions_host().copy()).cuda()
        assert torch.equal(out.index_select(1, idx), llr), "recover differs from the gather of its input"
    del llr, out
rm = PolarRateMatcher(N, 3 * N // 4, "puncture", PERM)
E = rm.E
tx = torch.empty((B, E), dtype=torch.uint8, device="cuda")
moved = B * 2 * E
report("select", rm, race({"kernel": lambda: rm.select(cw, out=tx), "copy": copy_of(moved)}), moved)
assert torch.equal(tx, cw.index_select(1, torch.from_numpy(rm.positions_host().copy()).cuda())), "select differs"

if a.step:
    K = E // 2
    dec = SCLDecoder(N, K, list_size=a.list_size, frozen_bits=construct_rate_matched(K, rm))
    msg = torch.empty((B, K), dtype=torch.uint8, device="cuda")
    rx = torch.empty((B, E), dtype=torch.float64, device="cuda")
    llr = torch.empty((B, N), dtype=torch.float64, device="cuda")
    bits = torch.empty((B, K), dtype=torch.uint8, device="cuda")
    counts = torch.zeros(3, dtype=torch.int64, device="cuda")
    stages = [
        ("random_bits", lambda: _native.random_bits(7, 0, msg)),
        ("encode", lambda: _native.polar_encode(dec.plan, msg, cw)),
        ("select", lambda: rm.select(cw, out=tx)),
        ("awgn", lambda: AWGNChannel(a.snr).llr_batch_device(tx, E, B, seed=7 ^ 0xA5A5A5A5, frame_offset=0, out=rx)),
        ("recover", lambda: rm.recover(rx, out=llr)),
        ("decode", lambda: dec.plan.decode(llr, bits)),
        ("count", lambda: _native.count_errors(msg, bits, K, counts)),
    ]
    rows = []
    for r in range(a.rounds + 1):  # the first step warms up
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(stages) + 1)]
        ev[0].record()
        for i, (_, f) in enumerate(stages):
            f()
            ev[i + 1].record()
        torch.cuda.synchronize()
        if r:
            rows.append([ev[i].elapsed_time(ev[i + 1]) for i in range(len(stages))])
    rows = np.asarray(rows)
    step = rows.sum(axis=1)
    med = {s[0]: float(np.median(rows[:, i])) for i, s in enumerate(stages)}
    print(json.dumps({"step": "scl", "N": N, "E": E, "K": K, "list_size": a.list_size, "batch": B, "snr_db": a.snr,
                      "step_ms": float(np.median(step)), "step_ms_min": float(step.min()),
                      "step_ms_max": float(step.max()), "stage_ms": med,
                      "recover_share": med["recover"] / float(np.median(step)),
                      "select_share": med["select"] / float(np.median(step)),
                      "frame_errors_per_step": int(counts[1].item()) // (a.rounds + 1)}), flush=True)

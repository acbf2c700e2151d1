"""Bit interleaver timing (diagnostic): HIP events around repeated launches.

usage: python tools/interleave_bench.py [--E 1024,8192] [--batch 65536] [--reps 5] [--rounds 20] [--rows 6]
                                        [--step]

Timed at `batch` frames of E elements, for both kinds ("rect" with `rows` rows, "tri"):
`interleave` (uint8) and `deinterleave` (fp32, fp64).  Each runs against its yardstick in the
same rounds, alternated: `copy`, one device-to-device copy (torch's copy_ of a contiguous
uint8 tensor) of the same bytes -- the kernel reads batch x E elements and writes as many.
One warm-up call each, then `rounds` rounds of `reps` launches; one JSON line per
measurement gives the median and the spread of the per-launch time, the bytes moved over
it, and the ratio of the medians.

--step: the interleaver's share of one rate-matched 64-QAM Monte-Carlo step instead: a
polar N = 1024 K = 512 SCL L = 8 chain at E = 768, timed with the interleaver and without.
"""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from polarcode_and_ldpc_amd import _native
from polarcode_and_ldpc_amd.channel import BitInterleaver, QAMModem

ap = argparse.ArgumentParser()
ap.add_argument("--E", default="1024,8192")
ap.add_argument("--batch", type=int, default=65536)
ap.add_argument("--reps", type=int, default=5, help="launches per timed round")
ap.add_argument("--rounds", type=int, default=20)
ap.add_argument("--rows", type=int, default=6, help="rows of the rect interleaver")
ap.add_argument("--step", action="store_true")
a = ap.parse_args()
B = a.batch


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


def step():
    import polarcode_and_ldpc_amd.polar as P
    from polarcode_and_ldpc_amd.harness.montecarlo import polar_round_fn
    N, K, E = 1024, 512, 768
    rm = P.PolarRateMatcher(N, E, "puncture")
    dec = P.SCLDecoder(N, K, list_size=8, frozen_bits=P.construct_rate_matched(K, rm))
    modem = QAMModem(6)
    fns = {"none": polar_round_fn(dec, seed=1, rate_matcher=rm, modulation=modem)}
    for kind in ("rect", "tri"):
        il = BitInterleaver(kind, E, rows=6 if kind == "rect" else None)
        fns[kind] = polar_round_fn(dec, seed=1, rate_matcher=rm, modulation=modem, interleaver=il)
    t = race({k: (lambda f=f: f(0, 12.0, 0, B)) for k, f in fns.items()})
    med = {k: float(np.median(v)) for k, v in t.items()}
    print(json.dumps(dict(op="step", chain="polar N=1024 K=512 E=768 SCL L=8 64-QAM", batch=B, step_ms=med,
                          share={k: (med[k] - med["none"]) / med[k] for k in ("rect", "tri")}, rounds=a.rounds,
                          reps=a.reps)), flush=True)


if a.step:
    step()
    sys.exit(0)

for E in (int(x) for x in a.E.split(",")):
    for kind in ("rect", "tri"):
        il = BitInterleaver(kind, E, rows=a.rows if kind == "rect" else None)
        for dt in (torch.uint8, torch.float32, torch.float64):
            if dt == torch.uint8:
                src = torch.empty((B, E), dtype=dt, device="cuda")
                _native.random_bits(4243, 0, src)
                fn = il.interleave
            else:
                src = torch.randn((B, E), dtype=dt, device="cuda")
                fn = il.deinterleave
            dst = torch.empty_like(src)
            flat_s = src.view(torch.uint8).view(-1)
            flat_d = torch.empty_like(flat_s)  # the copy's own destination: dst keeps the kernel's output
            moved = 2 * flat_s.numel()
            t = race({"kernel": lambda: fn(src, out=dst), "copy": lambda: flat_d.copy_(flat_s)})
            k, c = float(np.median(t["kernel"])), float(np.median(t["copy"]))
            lds = E <= _native.ILV_LDS_MAX_E[src.element_size()]
            print(json.dumps(dict(op="interleave" if dt == torch.uint8 else "deinterleave", kind=kind, rows=il.rows,
                                  dtype=str(dt).split(".")[-1], E=E, batch=B, path="lds" if lds else "direct",
                                  bytes_read_plus_written=moved, kernel_ms=k, kernel_ms_min=min(t["kernel"]),
                                  kernel_ms_max=max(t["kernel"]), kernel_gbps=moved / k / 1e6, copy_ms=c,
                                  copy_gbps=moved / c / 1e6, kernel_over_copy=k / c, rounds=a.rounds, reps=a.reps)),
                  flush=True)
            # the timed launch did its work: against the permutation on a few frames
            pos = torch.from_numpy(il.permutation().copy()).cuda()
            if dt == torch.uint8:
                want = torch.empty_like(src[:4])
                want[:, pos] = src[:4]
            else:
                want = src[:4][:, pos]
            assert torch.equal(dst[:4], want), "the kernel disagrees with the permutation"
            del src, dst, flat_s, flat_d

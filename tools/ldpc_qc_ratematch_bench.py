"""Rate matching timing (diagnostic): HIP events around repeated launches.

usage: python tools/ldpc_qc_ratematch_bench.py --qc mb,nb,Z,dv,seed [--core G] [--batch 65536] [--punctured 2]
                                               [--fillers 0] [--efrac 0.6,1.0,2.5] [--step] [--snr 1.0]
                                               [--max-iter 20] [--norm 0.75] [--reps 3] [--rounds 5]

The code is qc_encodable_base(mb, nb, Z, dv, seed, core, chained=False); per entry f
of --efrac a QCRateMatcher with E = round(f M) and start = rv_start(1).  Timed:
`select` (rate_match_kernel) and `recover` (rate_recover_kernel) for fp64 -> fp64 and
fp32 -> fp32, each against what one would write in torch with a precomputed index --
index_select for the selection; zero_ + index_copy_ (index_add_ once positions
repeat: atomics, order undefined) + the filler columns for the recovery -- and
asserted equal to it where no position repeats.  One warm-up call each, then
`rounds` rounds of `reps` launches, kernel and baseline alternated; one JSON line per
measurement gives the median and the spread of the per-launch time.  `hbm_floor_ms`
is the bytes a perfect kernel moves, batch 2 E for the selection and batch (E + n_out)
sizeof for the recovery, at the rate a device-to-device copy of 1 GiB reaches in this
process (read + write bytes per second).
--step: one Monte Carlo step of harness.ldpc_round_fn's rate-matched chain -- random
bits, encode, select, AWGN LLRs over E, recover, QCLayeredMSDecoder on decoder_base()
(early stop), error count -- for a float64 and a float32 decoder, events between the
stages; the median of `rounds` steps and the share of select + recover."""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from polarcode_and_ldpc_amd import _native
from polarcode_and_ldpc_amd.channel import AWGNChannel
from polarcode_and_ldpc_amd.ldpc import QCLDPCEncoder, QCLayeredMSDecoder, QCRateMatcher, qc_encodable_base

ap = argparse.ArgumentParser()
ap.add_argument("--qc", required=True, help="mb,nb,Z,dv,seed")
ap.add_argument("--core", type=int, default=4)
ap.add_argument("--batch", type=int, default=65536)
ap.add_argument("--punctured", type=int, default=2)
ap.add_argument("--fillers", type=int, default=0)
ap.add_argument("--efrac", default="0.6,1.0,2.5", help="E as multiples of M")
ap.add_argument("--step", action="store_true", help="also time one Monte Carlo step, fp64 and fp32 decoder")
ap.add_argument("--snr", type=float, default=1.0, help="--step: Es/N0 in dB")
ap.add_argument("--max-iter", type=int, default=20)
ap.add_argument("--norm", type=float, default=0.75)
ap.add_argument("--reps", type=int, default=3, help="launches per timed round")
ap.add_argument("--rounds", type=int, default=5)
a = ap.parse_args()
mb, nb, Z, dv, seed = (int(x) for x in a.qc.split(","))
base = qc_encodable_base(mb, nb, Z, dv, seed, core=a.core, chained=False)
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


# the device's copy rate: 1 GiB device to device, read + write bytes per second
src = torch.empty(1 << 30, dtype=torch.uint8, device="cuda")
dst = torch.empty_like(src)
dst.copy_(src)
torch.cuda.synchronize()
copy_ms = float(np.median([timed(lambda: dst.copy_(src), 3) for _ in range(5)]))
rate = 2.0 * (1 << 30) / (copy_ms * 1e-3)
del src, dst

probe = QCRateMatcher(base, Z, 1, punctured=a.punctured, fillers=a.fillers)
n, k, F = probe.n, probe.k, a.fillers
cw = torch.empty((B, n), dtype=torch.uint8, device="cuda")
_native.random_bits(4243, 0, cw)
for frac in (float(x) for x in a.efrac.split(",")):
    E = max(1, int(round(frac * probe.M)))
    rm = QCRateMatcher(base, Z, E, punctured=a.punctured, fillers=F, start=probe.rv_start(1))
    idx = torch.from_numpy(rm.positions_host().copy()).cuda()
    common = {"mb": mb, "nb": nb, "Z": Z, "n": n, "k": k, "batch": B, "punctured": a.punctured, "fillers": F,
              "E": E, "M": rm.M, "E_over_M": E / rm.M, "start": rm.start, "max_reps": rm.max_reps,
              "copy_gbps": rate / 1e9}
    tx, tx2 = (torch.empty((B, E), dtype=torch.uint8, device="cuda") for _ in range(2))
    t = race({"kernel": lambda: rm.select(cw, out=tx), "torch": lambda: torch.index_select(cw, 1, idx, out=tx2)})
    assert torch.equal(tx, tx2), "select differs from index_select"
    for name, v in t.items():
        print(json.dumps(dict(common, op="select", impl=name, ms=float(np.median(v)), ms_min=min(v), ms_max=max(v),
                              hbm_floor_ms=B * 2 * E / rate * 1e3)), flush=True)
    del tx2
    n_out = rm.n_dec
    for T in (torch.float64, torch.float32):
        llr = torch.randn((B, E), dtype=T, device="cuda")
        out, out2 = (torch.empty((B, n_out), dtype=T, device="cuda") for _ in range(2))

        def baseline():
            out2.zero_()
            if rm.max_reps == 1:
                out2.index_copy_(1, idx, llr)
            else:
                out2.index_add_(1, idx, llr)
            if F:
                out2[:, k - F:k] = rm.filler_llr

        t = race({"kernel": lambda: rm.recover(llr, out=out), "torch": baseline})
        if rm.max_reps == 1:
            assert torch.equal(out, out2), "recover differs from index_copy_"
        else:
            assert torch.allclose(out, out2, rtol=1e-4, atol=1e-4), "recover is far from index_add_"
        for name, v in t.items():
            print(json.dumps(dict(common, op="recover", dtype=str(T).replace("torch.", ""), n_out=n_out, impl=name,
                                  ms=float(np.median(v)), ms_min=min(v), ms_max=max(v),
                                  hbm_floor_ms=B * (E + n_out) * llr.element_size() / rate * 1e3)), flush=True)
        del llr, out, out2

    if a.step:
        enc = QCLDPCEncoder(base, Z)
        msg = torch.empty((B, k), dtype=torch.uint8, device="cuda")
        rx = torch.empty((B, E), dtype=torch.float64, device="cuda")
        bits = torch.empty((B, n_out), dtype=torch.uint8, device="cuda")
        its = torch.empty((B,), dtype=torch.int32, device="cuda")
        for dtype in (np.float64, np.float32):
            dec = QCLayeredMSDecoder(rm.decoder_base(), Z, max_iter=a.max_iter, normalization=a.norm, early_stop=True,
                                     dtype=dtype)
            llr = torch.empty((B, n_out), dtype=torch.float32 if dtype == np.float32 else torch.float64, device="cuda")
            counts = torch.zeros(3, dtype=torch.int64, device="cuda")

            def draw():
                _native.random_bits(7, 0, msg)
                msg[:, k - F:] = 0

            stages = [
                ("random_bits", draw),
                ("encode", lambda: enc.encode_batch_device(msg, out=cw)),
                ("select", lambda: rm.select(cw, out=tx)),
                ("awgn", lambda: AWGNChannel(a.snr).llr_batch_device(tx, E, B, seed=7 ^ 0xA5A5A5A5, frame_offset=0, out=rx)),
                ("recover", lambda: rm.recover(rx, out=llr)),
                ("decode", lambda: dec.plan.decode(llr, bits, its)),
                ("count", lambda: _native.count_errors(msg, bits, k - F, counts)),
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
            print(json.dumps(dict(common, step=np.dtype(dtype).name, snr_db=a.snr, n_dec=n_out,
                                  step_ms=float(np.median(step)), step_ms_min=float(step.min()),
                                  step_ms_max=float(step.max()), stage_ms=med,
                                  ratematch_share=(med["select"] + med["recover"]) / float(np.median(step)),
                                  mean_iter=float(its.double().mean()),
                                  frame_errors_per_step=int(counts[1].item()) // (a.rounds + 1))), flush=True)
            del llr
    del tx

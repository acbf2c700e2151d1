"""Quasi-cyclic encoder timing (diagnostic): HIP events around repeated launches.

usage: python tools/ldpc_qc_encode_bench.py --qc mb,nb,Z,dv,seed [--core G] [--unchained] [--batch 65536]
                                            [--dense] [--step] [--snr -1.0] [--max-iter 20] [--norm 0.75]
                                            [--reps 3] [--rounds 5]

The code is qc_encodable_base(mb, nb, Z, dv, seed, core, chained).  `qcenc` is
QCLDPCEncoder.encode_batch_device (ldpc_qc_encode.hip, from the base matrix);
--dense adds `dense`, LDPCEncoder(n, k, H=qc_expand(base, Z)).encode_batch_device
(gf2_encode_kernel on the bit-packed k x n generator), asserts equal codewords, and
times the two alternately on the same device messages: one warm-up call each, then
`rounds` rounds of `reps` launches; one JSON line per encoder gives the median and
the spread of the per-launch time.  `hbm_floor_ms` is batch (k + n) bytes at the
rate a device-to-device copy of 1 GiB reaches here (read + write bytes per
second, measured the same way).
--step: one Monte Carlo step of harness.ldpc_round_fn's chain -- random bits,
encode, AWGN LLRs, QCLayeredMSDecoder (early stop), error count -- for a float64
and a float32 decoder, events between the stages; the median of `rounds` steps
and the encoder's share."""
import argparse, ctypes, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from polarcode_and_ldpc_amd import _native
from polarcode_and_ldpc_amd.channel import AWGNChannel
from polarcode_and_ldpc_amd.ldpc import (LDPCEncoder, QCLDPCEncoder, QCLayeredMSDecoder, qc_encodable_base,
                                         qc_expand)

ap = argparse.ArgumentParser()
ap.add_argument("--qc", required=True, help="mb,nb,Z,dv,seed")
ap.add_argument("--core", type=int, default=None, help="core block rows (default mb)")
ap.add_argument("--unchained", action="store_true", help="chained=False: no extension row reads an extension parity")
ap.add_argument("--batch", type=int, default=65536)
ap.add_argument("--dense", action="store_true", help="also time the dense generator path")
ap.add_argument("--step", action="store_true", help="also time one Monte Carlo step, fp64 and fp32 decoder")
ap.add_argument("--snr", type=float, default=-1.0, help="--step: Es/N0 in dB")
ap.add_argument("--max-iter", type=int, default=20)
ap.add_argument("--norm", type=float, default=0.75)
ap.add_argument("--reps", type=int, default=3, help="launches per timed round")
ap.add_argument("--rounds", type=int, default=5)
a = ap.parse_args()
mb, nb, Z, dv, seed = (int(x) for x in a.qc.split(","))
base = qc_encodable_base(mb, nb, Z, dv, seed, core=a.core, chained=not a.unchained)
B = a.batch
enc = QCLDPCEncoder(base, Z)
n, k = enc.n, enc.k
msg = torch.empty((B, k), dtype=torch.uint8, device="cuda")
_native.random_bits(4243, 0, msg)
cw = torch.empty((B, n), dtype=torch.uint8, device="cuda")


def timed(fn, reps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / reps


# the device's copy rate: 1 GiB device to device, read + write bytes per second
src = torch.empty(1 << 30, dtype=torch.uint8, device="cuda")
dst = torch.empty_like(src)
dst.copy_(src)
torch.cuda.synchronize()
copy_ms = float(np.median([timed(lambda: dst.copy_(src), 3) for _ in range(5)]))
rate = 2.0 * (1 << 30) / (copy_ms * 1e-3)
del src, dst
floor_ms = B * (k + n) / rate * 1e3

encs = {"qcenc": lambda: enc.encode_batch_device(msg, out=cw)}
if a.dense:
    dense = LDPCEncoder(n, k, H=qc_expand(base, Z))
    cw2 = torch.empty_like(cw)
    encs["dense"] = lambda: dense.encode_batch_device(msg, out=cw2)
for f in encs.values():  # warm-up: encoder creation, first launch
    f()
torch.cuda.synchronize()
if a.dense:
    assert torch.equal(cw, cw2), "the two encoders differ"
times = {name: [] for name in encs}
for _ in range(a.rounds):
    for name, f in encs.items():  # alternated, so drift hits both alike
        times[name].append(timed(f, a.reps))
p = _native.QcEncoderProbe()
sh = np.ascontiguousarray(base, np.int32)
_native.check(_native.lib.pl_debug_ldpc_qc_encoder_probe(mb, nb, Z, sh.ctypes.data, ctypes.byref(p)), "probe")
for name, t in times.items():
    ms = float(np.median(t))
    print(json.dumps({"encoder": name, "mb": mb, "nb": nb, "Z": Z, "n": n, "k": k, "core": enc.g,
                      "chained": not a.unchained, "batch": B, "ms": ms, "ms_min": min(t), "ms_max": max(t),
                      "hbm_floor_ms": floor_ms, "copy_gbps": rate / 1e9, "n_sync": int(p.n_sync),
                      "lds_bytes": int(p.lds_bytes), "threads": int(p.threads)}))

if a.step:
    llr = torch.empty((B, n), dtype=torch.float64, device="cuda")
    out = torch.empty((B, n), dtype=torch.uint8, device="cuda")
    its = torch.empty((B,), dtype=torch.int32, device="cuda")
    info = torch.arange(k, device="cuda")
    for dtype in (np.float64, np.float32):
        dec = QCLayeredMSDecoder(base, Z, max_iter=a.max_iter, normalization=a.norm, early_stop=True, dtype=dtype)
        counts = torch.zeros(3, dtype=torch.int64, device="cuda")
        stages = [
            ("random_bits", lambda: _native.random_bits(7, 0, msg)),
            ("encode", lambda: enc.encode_batch_device(msg, out=cw)),
            ("awgn", lambda: AWGNChannel(a.snr).llr_batch_device(cw, n, B, seed=7 ^ 0xA5A5A5A5, frame_offset=0, out=llr)),
            ("decode", lambda: dec.plan.decode(llr, out, its)),
            ("count", lambda: _native.count_errors(msg, out.index_select(1, info).contiguous(), k, counts)),
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
        print(json.dumps({"step": np.dtype(dtype).name, "n": n, "batch": B, "snr_db": a.snr,
                          "step_ms": float(np.median(step)), "step_ms_min": float(step.min()),
                          "step_ms_max": float(step.max()), "stage_ms": med,
                          "encode_share": med["encode"] / float(np.median(step)),
                          "mean_iter": float(its.double().mean()),
                          "frame_errors_per_step": int(counts[1].item()) // (a.rounds + 1)}))

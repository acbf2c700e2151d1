"""LDPC decode kernel timing (diagnostic): HIP events around repeated launches.

usage: python tools/ldpc_bench.py [--batch 65536] [--algo bp,ms,lms,qclms,qclms32,qclms8,qcbp] [--n 504] [--seed 3]
                                  [--fixed 4,31,31] [--clip 64]
                                  [--qc mb,nb,Z,dv,seed] [--qc-encodable]
                                  [--random-codewords] [--max-iter 20] [--no-early-stop]
                                  [--snr 3.0] [--valid] [--norm 0.75] [--reps 5] [--rounds 3]

Default (no --n): the bench's (504,252) MacKay code (seed 42, degree-1 rows: BP
only) with the bench's invalid codewords, or --valid for the all-zero codeword.
--n N: regular_construction(N, 3, 6, seed) with the all-zero codeword, which all
three algorithms decode (ms and lms need --n: the default code has degree-1 rows).
--qc mb,nb,Z,dv,seed: the quasi-cyclic code qc_random_base(mb, nb, Z, dv, seed) with
the all-zero codeword; `qclms` is QCLayeredMSDecoder on the base matrix and `lms`
the generic layered decoder on the same H (from qc_to_csr, never dense) with the
same block-row layers.  With both, their bits and iteration counts on the timed
frames must be equal (asserted).  `qclms32` is QCLayeredMSDecoder(dtype=float32)
on the same device frames, cast once to fp32 outside the timed region; it is
another decoder (every operation in binary32), so its results are reported, not
compared: `frames_differ_from_qclms` counts the frames whose bits differ.
`qclms8` is QCFixedMSDecoder (int8 fixed point, --fixed scale,llr_max,msg_max) on the
same device frames, quantised once by the decoder's own kernel outside the timed
region; reported like qclms32, with `frames_differ_from_qclms32` when both run.
`qcbp` is QCLayeredBPDecoder (layered sum-product, fp64, --clip) on the same fp64 frames;
another decoder again, reported with `frames_differ_from_qclms` when both run.
--qc-encodable: the code qc_encodable_base(mb, nb, Z, dv, seed) instead, whose parity
part QCLDPCEncoder can encode from; without it --qc means what it always meant.
--random-codewords (needs --qc-encodable): the frames carry random messages encoded on
the device by QCLDPCEncoder instead of the all-zero codeword; frame errors are
counted against those codewords.
--algo takes a comma-separated list; the decoders are timed alternately on the
same frames, `rounds` times each, and one JSON line per entry gives the median
and the spread of the per-launch time.  Each entry may carry its own iteration
limit as `name:max_iter` (default --max-iter), e.g. `--algo ms:20,lms:10` times
layered-10 against flooding-20."""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from polarcode_and_ldpc_amd.channel import AWGNChannel
from polarcode_and_ldpc_amd import _native
from polarcode_and_ldpc_amd.ldpc import (BPDecoder, MSDecoder, LayeredMSDecoder, LDPCEncoder, QCLDPCEncoder,
                                         QCFixedMSDecoder, QCLayeredBPDecoder, QCLayeredMSDecoder, qc_block_layers, qc_encodable_base, qc_random_base,
                                         qc_to_csr, regular_construction)

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=65536)
ap.add_argument("--snr", type=float, default=3.0)
ap.add_argument("--valid", action="store_true", help="all-zero codewords (early stop active)")
ap.add_argument("--algo", default="bp", help="comma-separated: bp, ms, lms, each optionally :max_iter")
ap.add_argument("--max-iter", type=int, default=20)
ap.add_argument("--no-early-stop", action="store_true")
ap.add_argument("--norm", type=float, default=0.75, help="min-sum normalisation (ms, lms)")
ap.add_argument("--n", type=int, default=0, help="regular (3,6) code of this length instead of the bench's code")
ap.add_argument("--seed", type=int, default=3, help="regular_construction seed (--n)")
ap.add_argument("--qc", default="", help="mb,nb,Z,dv,seed: a qc_random_base code instead (algos lms, qclms)")
ap.add_argument("--qc-encodable", action="store_true", help="--qc builds qc_encodable_base(mb, nb, Z, dv, seed)")
ap.add_argument("--random-codewords", action="store_true",
                help="--qc-encodable: random codewords from QCLDPCEncoder instead of the all-zero one")
ap.add_argument("--fixed", default="4,31,31", help="qclms8: llr_scale,llr_max,msg_max")
ap.add_argument("--clip", type=float, default=64.0, help="qcbp: the clamp of the messages")
ap.add_argument("--reps", type=int, default=5, help="launches per timed round")
ap.add_argument("--rounds", type=int, default=3)
a = ap.parse_args()
B = a.batch
if (a.qc_encodable and not a.qc) or (a.random_codewords and not a.qc_encodable):
    raise SystemExit("--qc-encodable needs --qc mb,nb,Z,dv,seed, and --random-codewords needs --qc-encodable")
qc = None
if a.qc:
    mb, nb, Z, dv, qseed = (int(x) for x in a.qc.split(","))
    if a.qc_encodable:
        qc = qc_encodable_base(mb, nb, Z, dv, qseed)
    else:
        qc = qc_random_base(mb, nb, Z, dv, qseed)
    n, k = nb * Z, (nb - mb) * Z
    H = None
    cw = None
    if a.random_codewords:
        msg = torch.empty((B, k), dtype=torch.uint8, device="cuda")
        _native.random_bits(4243, 0, msg)
        cw = QCLDPCEncoder(qc, Z).encode_batch_device(msg)
elif a.n:
    n, k = a.n, a.n // 2
    H = regular_construction(n, 3, 6, seed=a.seed)
    cw = None
else:
    n, k = 504, 252
    enc = LDPCEncoder(n, k, dv=3, dc=6, seed=42)
    H = enc.H
    if a.valid:
        cw = None
    else:
        rs = np.random.RandomState(42)
        base = enc.encode_batch(rs.randint(0, 2, (4096, k)))
        cw = torch.from_numpy(np.tile(base, (B // 4096 + 1, 1))[:B].astype(np.uint8)).cuda()
es = not a.no_early_stop


class GenericOnQc:
    """The generic layered decoder on the expanded quasi-cyclic H with the block rows as layers."""

    def __init__(self, max_iter):
        rp, ci = qc_to_csr(qc, Z)
        self.plan = _native.layered_ldpc_plan(rp, ci, n, qc_block_layers(mb, Z), max_iter, es, a.norm)

    def _check_runnable(self):
        pass


def make(spec):
    name, _, mi = spec.partition(":")
    mi = int(mi) if mi else a.max_iter
    if qc is not None:
        if name == "qclms":
            return QCLayeredMSDecoder(qc, Z, max_iter=mi, normalization=a.norm, early_stop=es)
        if name == "qclms32":
            return QCLayeredMSDecoder(qc, Z, max_iter=mi, normalization=a.norm, early_stop=es, dtype=np.float32)
        if name == "qclms8":
            fs, fl, fm = a.fixed.split(",")
            return QCFixedMSDecoder(qc, Z, max_iter=mi, normalization=a.norm, early_stop=es, llr_scale=float(fs),
                                    llr_max=int(fl), msg_max=int(fm))
        if name == "qcbp":
            return QCLayeredBPDecoder(qc, Z, max_iter=mi, early_stop=es, clip=a.clip)
        if name == "lms":
            return GenericOnQc(mi)
        raise SystemExit("--qc takes --algo lms, qclms, qclms32, qclms8 and qcbp only, not %r" % spec)
    if name in ("qclms", "qclms32", "qclms8", "qcbp"):
        raise SystemExit("--algo %s needs --qc mb,nb,Z,dv,seed" % name)
    if name == "bp":
        return BPDecoder(H, max_iter=mi, early_stop=es)
    if name == "ms":
        return MSDecoder(H, max_iter=mi, normalization=a.norm, early_stop=es)
    if name == "lms":
        return LayeredMSDecoder(H, max_iter=mi, normalization=a.norm, early_stop=es)
    raise SystemExit("unknown --algo %r" % spec)


specs = a.algo.split(",")
if not a.n and qc is None and any(s.partition(":")[0] in ("ms", "lms") for s in specs):
    raise SystemExit("the default (504,252) code has degree-1 rows, which min-sum cannot decode: "
                     "give --n N (a regular (3,6) code) with --algo ms / lms")
decs = [make(s) for s in specs]
llr = AWGNChannel(a.snr).llr_batch_device(cw, n, B, seed=4242)
llr32 = llr.to(torch.float32) if any(s.partition(":")[0] == "qclms32" for s in specs) else None


llr8 = {s: d.quantize(llr) for s, d in zip(specs, decs) if s.partition(":")[0] == "qclms8"}


def frames_of(spec):
    """The timed frames in the type the decoder reads: fp32 for qclms32 (cast above, once), int8 for
    qclms8 (quantised above, once), else fp64."""
    return llr8[spec] if spec in llr8 else llr32 if spec.partition(":")[0] == "qclms32" else llr


out = torch.empty((B, n), dtype=torch.uint8, device="cuda")
its = torch.empty((B,), dtype=torch.int32, device="cuda")
stats = []
results = {}
for s, d in zip(specs, decs):  # warm-up: plan creation, workspace, first launch
    d._check_runnable()
    d.plan.decode(frames_of(s), out, its)
    torch.cuda.synchronize()
    wrong = (out != 0).any(dim=1) if cw is None else (out != cw).any(dim=1) if a.random_codewords else None
    stats.append({"mean_iter": float(its.double().mean()),
                  "frame_errors": int(wrong.sum()) if wrong is not None else None})
    if qc is not None:
        results[s] = (out.clone(), its.clone())
if qc is not None:  # the two decoders are one definition: equal on the timed frames
    names = {s.partition(":")[0]: s for s in specs if s.partition(":")[2] in ("", str(a.max_iter))}
    if "lms" in names and "qclms" in names:
        (b0, i0), (b1, i1) = results[names["lms"]], results[names["qclms"]]
        assert torch.equal(b0, b1) and torch.equal(i0, i1), "qclms and lms differ on the timed frames"
    if "qclms" in names and "qclms32" in names:
        (b0, _), (b1, _) = results[names["qclms"]], results[names["qclms32"]]
        stats[specs.index(names["qclms32"])]["frames_differ_from_qclms"] = int((b0 != b1).any(dim=1).sum())
    if "qclms" in names and "qcbp" in names:
        (b0, _), (b1, _) = results[names["qclms"]], results[names["qcbp"]]
        stats[specs.index(names["qcbp"])]["frames_differ_from_qclms"] = int((b0 != b1).any(dim=1).sum())
    if "qclms32" in names and "qclms8" in names:
        (b0, _), (b1, _) = results[names["qclms32"]], results[names["qclms8"]]
        stats[specs.index(names["qclms8"])]["frames_differ_from_qclms32"] = int((b0 != b1).any(dim=1).sum())
times = [[] for _ in decs]
for _ in range(a.rounds):
    for i, d in enumerate(decs):  # alternated, so drift hits every decoder alike
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        x = frames_of(specs[i])
        for _ in range(a.reps):
            d.plan.decode(x, out, its)
        ev[1].record()
        torch.cuda.synchronize()
        times[i].append(ev[0].elapsed_time(ev[1]) / a.reps)
for s, d, t, st in zip(specs, decs, times, stats):
    ms = float(np.median(t))
    print(json.dumps({"algo": s, "n": n, "batch": B, "early_stop": es, "snr_db": a.snr, "kernel_ms": ms,
                      "kernel_ms_min": min(t), "kernel_ms_max": max(t), "info_mbps": B * k / ms / 1e3,
                      "mean_iter": st["mean_iter"], "frame_errors": st["frame_errors"],
                      **({"codewords": "random"} if a.random_codewords else {}),
                      "plan_kernel": int(d.plan.info.reserved), "lds_bytes": int(d.plan.info.lds_bytes),
                      **{k: st[k] for k in ("frames_differ_from_qclms", "frames_differ_from_qclms32") if k in st},
                      "frames_per_block": int(d.plan.info.frames_per_block),
                      "kernel": os.environ.get("PL_LDPC_KERNEL", "default")}))

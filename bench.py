#!/usr/bin/env python3
"""Benchmark: decoded info-Mbps of the MI355X decoders (BASELINE.json metric).

Headline (`value`): Polar N=1024 K=512 SCL L=8, 65 536 AWGN frames per GPU
(BASELINE.json configs[1]); a step = one batched decode of the resident LLR
matrix + on-device error count (+ one all-reduce of the counters when N > 1).
Secondary keys, each with its own roofline:
  `ldpc`       LDPC (504,252) BP max_iter=20 (configs[2]) on the reference
               harness's frames (benchmarks/throughput_test.py:285-315: its
               encoder's invalid codewords, so every frame runs 20 iterations);
               `ldpc.valid_codewords`: all-zero codewords with early stop;
  `end_to_end` the polar Monte-Carlo step with fresh device messages, encoding
               and AWGN inside the timed region (SURVEY §8 d);
  `cascl_l32`  CA-SCL N=1024 K=512 L=32 + CRC-8 (configs[3]) decode throughput
               and a -2..5 dB BER/FER sweep through harness.ber (max_errors stop,
               frames sharded over the ranks);
  `long_block` configs[4] per GPU (1 M frames / 8): polar N=4096 K=2048 SCL L=8
               and LDPC n=8192 (3,6)-regular min-sum, 131 072 frames each.
`cpu_baseline`: the reference's NumPy decode loops restated (oracle/refnumpy.py,
bit-exact with the reference fixtures) over a spawn pool of host processes on the
first frames of the same LLR batch; the C port (oracle/refcpu.c, OpenMP) beside it.

info-Mbps = frames * K_info / t / 1e6 (throughput_test.py:217, :304).
Usage: python bench.py [--gpus N --steps K --warmup W] [--dump-outputs DIR] [--full].
A plain run sets up the headline's frames, warms up, times exactly K steps and
prints the result line (no CPU pool, no secondary key, no detail file).  `--full`
adds every secondary key above and the CPU baselines, as one run measured them
before the option existed; `--sections` / `--skip-*` select among them.
`--dump-outputs DIR` writes what the headline's last timed step left for its
caller (see dump_outputs) as DIR/<name>.npy.  With N > 1 and no
WORLD_SIZE in the environment, bench.py re-launches itself under
torch.distributed.run with N ranks (before any GPU call).  `--cpu-stub` runs the
same rank/timing/all-reduce path on CPU (gloo) with a stub decode: a plumbing
check, never a measurement.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

METRIC = "decoded info-Mbps: polar N=1024 SCL L=8 & LDPC(504,252) BP, 1/2/4/8 GPUs"
HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec (MI355X_MICROARCH.md)
HBM_ACHIEVABLE_GBS = 6290.0  # measured float4 copy (MI355X_MICROARCH.md, chip-level parameters)
CLOCK_GHZ = 2.4


SECTIONS = ("polar", "e2e", "polar_default", "sc_default", "config0", "ldpc", "ldpc_valid", "cascl", "sweep",
            "long_polar", "long_ms", "long_ms_noes")


def log(*a):
    print(*a, file=sys.stderr, flush=True)


# ---------------------------------------------------------------- ranks
class Runtime:
    """One process per GPU (RCCL) or, with --cpu-stub, per CPU rank (gloo)."""

    def __init__(self, stub: bool, backend: str = "nccl"):
        self.world = int(os.environ.get("WORLD_SIZE", "1"))
        self.rank = int(os.environ.get("RANK", "0"))
        self.local = int(os.environ.get("LOCAL_RANK", "0"))
        self.stub = stub
        self.host_reduce = stub or backend == "gloo"
        if stub:
            self.device = torch.device("cpu")
            if self.world > 1:
                dist.init_process_group("gloo")
        else:
            # --dist-backend gloo: ranks may share a GPU (a rehearsal of the
            # multi-rank path on a one-GPU box; RCCL refuses duplicate GPUs)
            dev = self.local if backend == "nccl" else self.local % torch.cuda.device_count()
            torch.cuda.set_device(dev)
            self.device = torch.device("cuda", dev)
            if self.world > 1:
                if backend == "nccl":
                    dist.init_process_group("nccl", device_id=self.device)
                else:
                    dist.init_process_group("gloo")

    def sync(self):
        if not self.stub:
            torch.cuda.synchronize()

    def barrier(self):
        if self.world > 1:
            dist.barrier()

    def all_reduce(self, t, op=None):
        if self.world > 1:
            if self.host_reduce and t.is_cuda:
                h = t.cpu()
                dist.all_reduce(h, op=op or dist.ReduceOp.SUM)
                t.copy_(h)
            else:
                dist.all_reduce(t, op=op or dist.ReduceOp.SUM)
        return t

    def gather(self, x: float):
        """x from every rank, rank order."""
        if self.world == 1:
            return [x]
        t = torch.tensor([x], dtype=torch.float64, device="cpu" if self.host_reduce else self.device)
        out = [torch.zeros_like(t) for _ in range(self.world)]
        dist.all_gather(out, t)
        return [float(o.item()) for o in out]

    def close(self):
        if self.world > 1:
            dist.destroy_process_group()


def timed_steps(step, steps, warmup, rt, on_timed=None):
    """W untimed warmup steps, then EXACTLY `steps` steps bracketed by barrier +
    device synchronisation on both sides.  Returns (max over ranks, per-rank)."""
    for _ in range(warmup):
        step()
    rt.sync()
    rt.barrier()
    rt.sync()
    if on_timed is not None:
        on_timed()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    rt.sync()
    rt.barrier()
    rt.sync()
    dt = time.perf_counter() - t0
    per_rank = rt.gather(dt)
    return max(per_rank), per_rank


class KernelTimer:
    """HIP events around each decode launch, on the stream it is launched on
    (the decoders launch on torch's current stream); reset when the timed
    region starts, so the mean covers exactly the timed launches."""

    def __init__(self):
        self.pairs = []

    def __call__(self, fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        self.pairs.append((s, e))

    def reset(self):
        self.pairs = []

    def mean_ms(self):
        torch.cuda.synchronize()
        return float(np.mean([s.elapsed_time(e) for s, e in self.pairs])) if self.pairs else float("nan")


# ---------------------------------------------------------------- roofline
def _pmc(name):
    p = os.path.join(ROOT, "profiles", "pmc_traffic.json")
    try:
        return json.load(open(p)).get(name)
    except Exception:
        return None


def roofline(name, kernel, frames, bytes_per_frame, kms):
    """Algorithmic bytes per launch / live kernel time against HBM peak, plus the
    PMC figures for the same kernel from profiles/pmc_traffic.json: HBM-side
    traffic per launch (2*FETCH_SIZE + WRITE_SIZE, MI355X_MICROARCH.md gfx950
    correction) and the VALU issue rate against the SIMD-32 ceiling (a wave64
    fp64 VALU instruction occupies a SIMD 4 cycles, any other VALU 2 cycles:
    MI355X_MICROARCH.md:53-54 and the 78.6 / 157.3 TF fp64 / fp32 vector peaks)."""
    achieved = frames * bytes_per_frame / (kms / 1e3) / 1e9
    r = dict(bound="hbm", achieved=achieved, peak=HBM_PEAK_GBS, unit="GB/s", frac=achieved / HBM_PEAK_GBS,
             traffic=None, algorithmic_bytes_per_frame=bytes_per_frame, frames_per_launch=frames, kernel=kernel,
             kernel_ms=kms)
    p = _pmc(name)
    if not p:
        return r
    r["traffic"] = float(p["bytes_per_launch"]) * frames / float(p.get("frames", frames))
    r["traffic_unit"] = "HBM-side bytes per launch (2*FETCH_SIZE+WRITE_SIZE, rocprofv3 PMC)"
    r["traffic_source"] = p.get("source")
    r["traffic_GBps"] = r["traffic"] / (kms / 1e3) / 1e9
    r["traffic_frac"] = r["traffic_GBps"] / HBM_PEAK_GBS
    r["traffic_frac_of_achievable"] = r["traffic_GBps"] / HBM_ACHIEVABLE_GBS
    r["traffic_frames_profiled"] = p.get("frames")
    # the PMC pass's library build against the one measured now (pmc_summary.py records it)
    from polarcode_and_ldpc_amd import _native
    r["traffic_build"] = p.get("build")
    r["traffic_same_build"] = p.get("build") == _native.build_id()
    if "wave_time_shares" in p:
        r["wave_time_shares"] = p["wave_time_shares"]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if "valu_fp64_per_launch" in p and "valu_per_launch" in p:
        scale = frames / float(p.get("frames", frames))
        f64 = float(p["valu_fp64_per_launch"]) * scale
        other = max(0.0, float(p["valu_per_launch"]) * scale - f64)
        # SIMD-cycles needed at full issue / SIMD-cycles available in the launch
        need = 4.0 * f64 + 2.0 * other
        avail = cus * 4 * CLOCK_GHZ * 1e9 * kms / 1e3
        r["valu"] = dict(fp64_instr=f64, other_instr=other, simd_cycles_needed=need, simd_cycles_available=avail,
                         frac=need / avail, ceiling="4 cyc/wave64 fp64 VALU, 2 cyc other VALU, per SIMD-32; "
                                                   "%d CUs x 4 SIMDs x %.1f GHz" % (cus, CLOCK_GHZ),
                         source=p.get("source"))
    return r


# ---------------------------------------------------------------- CPU baseline
def cpu_share():
    """(processes the CPU legs use, what the host offers).  The GPU box gives one
    GPU a 16-CPU share of a larger host (os.sched_getaffinity lists every CPU of
    the machine); the legs use min(affinity, cgroup quota, PL_BENCH_CPU_CAP=16)
    processes and report the host's figures beside it."""
    aff = len(os.sched_getaffinity(0))
    quota = None
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            quota = max(1, -(-int(q) // int(per)))
    except Exception:
        pass
    cap = int(os.environ.get("PL_BENCH_CPU_CAP", "16"))
    used = max(1, min(aff, quota or aff, cap))
    model = "unknown"
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                model = line.split(":", 1)[1].strip()
                break
    except OSError:
        pass
    # cpu_model: the restatement runs within 7 % of the reference on one core of
    # the same machine (tools/cpu_calibration.py, profiles/r05/cpu_calibration*.json)
    return used, dict(host_cpus_affinity=aff, cgroup_cpu_quota=quota, cap=cap, os_cpu_count=os.cpu_count(),
                      cpu_model=model)


def cpu_processes():
    return cpu_share()[0]


def _mism(bits, gpu_bits):
    return int((np.asarray(bits) != np.asarray(gpu_bits)).any(axis=1).sum())


def numpy_baseline(pool, procs, what, fn, frames, info_bits, gpu_bits, single=None):
    """Time the NumPy restatement of the reference loops on `frames` frames over
    the pool; `single` = (fn, frames) times it in this process (one core)."""
    t0 = time.perf_counter()
    bits = fn()
    ct = time.perf_counter() - t0
    res = dict(value=frames * info_bits / ct / 1e6, unit="info-Mbps", cores=procs, kind="port",
               sample="first %d frames of the same LLR batch: %s (oracle/refnumpy.py, the reference's NumPy "
                      "per-frame loops restated, bit-exact with its fixtures), %d spawn processes, %.1f s"
                      % (frames, what, procs, ct),
               mismatching_frames_vs_gpu=_mism(bits, gpu_bits), host=cpu_share()[1])
    if single is not None:
        sfn, sframes = single
        t0 = time.perf_counter()
        sb = sfn()
        st = time.perf_counter() - t0
        res["single_core"] = dict(value=sframes * info_bits / st / 1e6, unit="info-Mbps", cores=1, kind="port",
                                  sample="first %d frames, one process, %.1f s" % (sframes, st),
                                  mismatching_frames_vs_gpu=_mism(sb, gpu_bits[:sframes]))
    return res


def c_port(res, what, fn, frames, info_bits, gpu_bits, procs):
    """The C restatement (oracle/refcpu.c, OpenMP) beside the NumPy figure."""
    t0 = time.perf_counter()
    bits = fn()
    ct = time.perf_counter() - t0
    res["c_port"] = dict(value=frames * info_bits / ct / 1e6, unit="info-Mbps", cores=procs, kind="port",
                         sample="first %d frames, oracle/refcpu.c %s (loop-faithful C restatement), OpenMP %d "
                                "threads, %.1f s" % (frames, what, procs, ct),
                         mismatching_frames_vs_gpu=_mism(bits, gpu_bits))
    return res


# ---------------------------------------------------------------- polar
def polar_fixture(rt, N, K, L, B, snr, seed, frozen_snr=2.0):
    from polarcode_and_ldpc_amd import _native
    from polarcode_and_ldpc_amd.channel import AWGNChannel
    from polarcode_and_ldpc_amd.polar import SCLDecoder, construct_frozen_set
    # frozen_snr None: the reference's default set (generate_frozen_bits, the
    # decoders' frozen_bits=None case that throughput_test.py runs)
    frozen = None if frozen_snr is None else construct_frozen_set(N, K, frozen_snr)
    dec = SCLDecoder(N, K, list_size=L, frozen_bits=frozen)
    frozen = dec.frozen_bits
    off = rt.rank * B  # global frame indices: identical frames for any GPU count
    msg = torch.empty((B, K), dtype=torch.uint8, device="cuda")
    _native.random_bits(seed, off, msg)
    cw = torch.empty((B, N), dtype=torch.uint8, device="cuda")
    _native.polar_encode(dec.plan, msg, cw)
    llr = AWGNChannel(snr).llr_batch_device(cw, N, B, seed=seed, frame_offset=off)
    del cw
    return dec, frozen, msg, llr


def rank_fields(dt_per_rank, steps, counts):
    """Per-rank step times (the value is taken at the max) and the counters
    all-reduced over the ranks (frames counted = world x frames per GPU x steps)."""
    return dict(rank_ms_per_step=[t / steps * 1e3 for t in dt_per_rank], frames_counted=int(counts[2]),
                frame_errors=int(counts[1]), bit_errors=int(counts[0]))


def polar_kernel_name(plan, n):
    i = plan.info
    if i.reserved == 4:
        return "polar_tree_kernel<n=%d,LCAP=%d,%s,F=%d>" % (n, 64 // max(1, i.frames_per_block),
                                                          "SC" if i.list_size == 0 else "SCL", i.fused_top)
    return "polar_lane_kernel (generation %d)" % i.reserved


def decode_loop(rt, plan, llr, out, msg, width, steps, warmup, iters=None):
    """Timed decode + device error count (+ counter all-reduce) steps."""
    from polarcode_and_ldpc_amd import _native
    kt = KernelTimer()
    counts = torch.zeros(3, dtype=torch.int64, device="cuda")
    sc = torch.zeros(3, dtype=torch.int64, device="cuda")

    def step():
        kt(lambda: plan.decode(llr, out, iters))
        if rt.world == 1:  # pl_count_errors accumulates: no per-step reduction needed
            _native.count_errors(msg, out, width, counts)
            return
        sc.zero_()
        _native.count_errors(msg, out, width, sc)
        rt.all_reduce(sc)
        counts.add_(sc)

    def start():
        kt.reset()
        counts.zero_()

    dt, per_rank = timed_steps(step, steps, warmup, rt, on_timed=start)
    return dt, per_rank, kt.mean_ms(), counts.cpu().numpy()


DUMP_MAX_BYTES = 32 << 20  # decoded_bits.npy; the whole dump stays far below 64 MB


def dump_outputs(path, out, counts):
    """--dump-outputs: the arrays the headline's timed path hands its caller after
    the last timed step.  decoded_bits.npy: the decoded info bits (float32, one row
    per frame) of a fixed, seeded sample of this rank's frames when the whole
    (B, K) matrix would exceed DUMP_MAX_BYTES; decoded_bits_frames.npy: the sampled
    rows' frame indices within the rank's batch (float64, ascending);
    error_counts.npy: the device counters {bit errors, frame errors, frames} over
    the timed steps (float64).  The frames are a function of the arguments alone
    (seeded Philox on global frame indices), so two builds run with the same
    arguments can be compared array for array."""
    os.makedirs(path, exist_ok=True)
    B, K = out.shape
    rows = min(B, max(1, DUMP_MAX_BYTES // (4 * K)))
    idx = np.arange(B) if rows == B else np.sort(np.random.RandomState(20240).permutation(B)[:rows])
    bits = out[torch.from_numpy(idx).to(out.device)].cpu().numpy().astype(np.float32)
    np.save(os.path.join(path, "decoded_bits.npy"), bits)
    np.save(os.path.join(path, "decoded_bits_frames.npy"), idx.astype(np.float64))
    np.save(os.path.join(path, "error_counts.npy"), np.asarray(counts, dtype=np.float64))
    log("bench.py: outputs of the last timed step (%d of %d frames) in %s" % (rows, B, path))


def _bench_headline(args, rt, pool, N, K, L, B):
    """BASELINE configs[1] decode (+ the end-to-end Monte-Carlo step)."""
    from polarcode_and_ldpc_amd import _native
    from polarcode_and_ldpc_amd.channel import AWGNChannel
    dec, frozen, msg, llr = polar_fixture(rt, N, K, L, B, args.snr, 42)
    plan = dec.plan
    out = torch.empty((B, K), dtype=torch.uint8, device="cuda")
    dt, per_rank, kms, c = decode_loop(rt, plan, llr, out, msg, K, args.steps, args.warmup)
    if args.dump_outputs and rt.rank == 0:
        dump_outputs(args.dump_outputs, out, c)
    res = dict(value=B * rt.world * args.steps * K / dt / 1e6, ms_per_step=dt / args.steps * 1e3,
               rank_ms_per_step=[t / args.steps * 1e3 for t in per_rank], kernel_ms=kms, B=B,
               roofline=roofline("polar_scl_1024_l8", polar_kernel_name(plan, 10), B, 8 * N + K, kms),
               plan=dict(lds_bytes=plan.info.lds_bytes, fused_top=plan.info.fused_top),
               ber=float(c[0]) / max(1, c[2] * K), fer=float(c[1]) / max(1, c[2]), frames_counted=int(c[2]))
    if pool is not None:
        from oracle import oracle as O
        from oracle import refnumpy as R
        S, S1, S2 = min(args.cpu_frames_numpy, B), min(8, B), min(args.cpu_frames, B)
        llr_h = llr[:max(S, S2)].cpu().numpy()
        got = out[:llr_h.shape[0]].cpu().numpy().astype(np.int64)
        procs = cpu_processes()
        res["cpu_baseline"] = numpy_baseline(
            pool, procs, "SCL N=1024 L=%d" % L, lambda: R.polar_batch(N, L, frozen, llr_h[:S], pool=pool), S, K,
            got[:S], single=(lambda: R.polar_batch(N, L, frozen, llr_h[:S1]), S1))
        c_port(res["cpu_baseline"], "SCL L=%d" % L, lambda: O.scl_decode(N, L, frozen, llr_h[:S2], threads=procs),
               S2, K, got[:S2], procs)
        del llr_h

    if "e2e" in args.sec:
        # End-to-end Monte Carlo (SURVEY §8 d): fresh messages, encoding, AWGN,
        # decode and error count per step, all on the device.
        ch = AWGNChannel(args.snr)
        ec = torch.zeros(3, dtype=torch.int64, device="cuda")
        sc = torch.zeros(3, dtype=torch.int64, device="cuda")
        stepno = [0]
        ekt = KernelTimer()
        msg2, out2 = torch.empty_like(msg), torch.empty_like(out)
        cw2 = torch.empty((B, N), dtype=torch.uint8, device="cuda")
        llr2 = torch.empty_like(llr)

        def e2e_step():
            o = rt.rank * B + stepno[0] * B * rt.world  # fresh global frame indices every step
            stepno[0] += 1
            _native.random_bits(43, o, msg2)
            _native.polar_encode(plan, msg2, cw2)
            ch.llr_batch_device(cw2, N, B, seed=43, frame_offset=o, out=llr2)
            ekt(lambda: plan.decode(llr2, out2))
            sc.zero_()
            _native.count_errors(msg2, out2, K, sc)
            rt.all_reduce(sc)
            ec.add_(sc)

        def e2e_start():
            ec.zero_()
            ekt.reset()

        edt, _ = timed_steps(e2e_step, args.steps, args.warmup, rt, on_timed=e2e_start)
        e = ec.cpu().numpy()
        ekms = ekt.mean_ms()
        res["end_to_end"] = dict(value=B * rt.world * args.steps * K / edt / 1e6, unit="info-Mbps",
                                 ms_per_step=edt / args.steps * 1e3, kernel_ms=ekms,
                                 roofline=roofline("polar_scl_1024_l8", polar_kernel_name(plan, 10), B, 8 * N + K,
                                                   ekms),
                                 what="per step: device random messages + polar encode + AWGN LLRs (Philox) + "
                                      "SCL decode + error count (+ all-reduce)",
                                 ber=float(e[0]) / max(1, e[2] * K), fer=float(e[1]) / max(1, e[2]))
        del msg2, out2, cw2, llr2
        if pool is not None:
            res["end_to_end"]["cpu_baseline"] = e2e_cpu_baseline(args, pool, dec, frozen, N, K, L)
    return res


def bench_polar(args, rt, pool):
    from polarcode_and_ldpc_amd import _native
    from polarcode_and_ldpc_amd.channel import AWGNChannel
    N, K, L, B = 1024, 512, args.list_size, args.batch
    res = {}
    if "polar" in args.sec:
        res.update(_bench_headline(args, rt, pool, N, K, L, B))
    if "polar_default" in args.sec:
        # like-for-like with throughput_test.py (SURVEY §8 d): the default frozen
        # set, info = indices whose bit reversal is >= N - K
        dd, dfr, dmsg, dllr = polar_fixture(rt, N, K, L, B, args.snr, 47, frozen_snr=None)
        dout = torch.empty((B, K), dtype=torch.uint8, device="cuda")
        ddt, dpr, dkms, dc = decode_loop(rt, dd.plan, dllr, dout, dmsg, K, args.steps, args.warmup)
        res["default_frozen_set"] = dict(
            metric="decoded info-Mbps, polar N=1024 K=512 SCL L=%d, reference default frozen set "
                   "(generate_frozen_bits) @ %.1f dB" % (L, args.snr),
            value=B * rt.world * args.steps * K / ddt / 1e6, unit="info-Mbps", ms_per_step=ddt / args.steps * 1e3,
            kernel_ms=dkms, fer=float(dc[1]) / max(1, dc[2]), **rank_fields(dpr, args.steps, dc),
            roofline=roofline("polar_scl_1024_l8_default", polar_kernel_name(dd.plan, 10), B, 8 * N + K, dkms))
        if pool is not None:
            from oracle import refnumpy as R
            S = min(args.cpu_frames_numpy, B)
            lh = dllr[:S].cpu().numpy()
            res["default_frozen_set"]["cpu_baseline"] = numpy_baseline(
                pool, cpu_processes(), "SCL N=1024 L=%d, default frozen set" % L,
                lambda: R.polar_batch(N, L, dfr, lh, pool=pool), S, K, dout[:S].cpu().numpy().astype(np.int64))
        del dd, dmsg, dllr, dout
        torch.cuda.empty_cache()
    return res


def e2e_cpu_baseline(args, pool, dec, frozen, N, K, L):
    """The reference's own frame loop (benchmarks/ber_simulation.py:167-189:
    np.random.randint messages, host encoder, AWGNChannel.transmit, decode)
    with the NumPy decode restatement, on S frames; the GPU decodes the same
    host LLRs for the mismatch count."""
    from oracle import refnumpy as R
    from polarcode_and_ldpc_amd.channel import AWGNChannel
    from polarcode_and_ldpc_amd.polar import PolarEncoder
    S = max(16, args.cpu_frames_numpy // 4)
    state = np.random.get_state()
    enc = PolarEncoder(N, K, frozen_bits=frozen)
    ch = AWGNChannel(args.snr, seed=43)
    t0 = time.perf_counter()
    msgs = np.random.randint(0, 2, (S, K))
    llr_h = ch.transmit(enc.encode_batch(msgs), return_llr=True)
    bits = R.polar_batch(N, L, frozen, llr_h, pool=pool)
    ct = time.perf_counter() - t0
    np.random.set_state(state)
    got = dec.decode_batch(torch.from_numpy(llr_h).cuda()).cpu().numpy().astype(np.int64)
    procs = cpu_processes()
    return dict(value=S * K / ct / 1e6, unit="info-Mbps", cores=procs, kind="port",
                sample="%d frames of the reference's frame loop (messages, host encoder, AWGNChannel.transmit, "
                       "NumPy SCL L=%d restatement), %d spawn processes, %.1f s" % (S, L, procs, ct),
                mismatching_frames_vs_gpu=_mism(bits, got), host=cpu_share()[1])


def bench_sc_default(args, rt, pool):
    """The reference's published polar number (benchmarks/results/data/
    throughput_results.json:4-14, produced by throughput_test.py:197-235): SC
    N=1024 K=512, default frozen set (generate_frozen_bits), 3 dB."""
    from polarcode_and_ldpc_amd import _native
    from polarcode_and_ldpc_amd.channel import AWGNChannel
    from polarcode_and_ldpc_amd.polar import SCDecoder
    N, K, B = 1024, 512, args.batch
    dec = SCDecoder(N, K)  # frozen_bits=None: the reference's default set
    off = rt.rank * B
    msg = torch.empty((B, K), dtype=torch.uint8, device="cuda")
    _native.random_bits(48, off, msg)
    cw = torch.empty((B, N), dtype=torch.uint8, device="cuda")
    _native.polar_encode(dec.plan, msg, cw)
    llr = AWGNChannel(args.snr).llr_batch_device(cw, N, B, seed=48, frame_offset=off)
    del cw
    out = torch.empty((B, K), dtype=torch.uint8, device="cuda")
    dt, pr, kms, c = decode_loop(rt, dec.plan, llr, out, msg, K, args.steps, args.warmup)
    res = dict(metric="decoded info-Mbps, polar N=1024 K=512 SC, reference default frozen set @ %.1f dB "
                      "(the reference's published polar throughput configuration)" % args.snr,
               value=B * rt.world * args.steps * K / dt / 1e6, unit="info-Mbps", ms_per_step=dt / args.steps * 1e3,
               kernel_ms=kms, frames_per_gpu=B, fer=float(c[1]) / max(1, c[2]), **rank_fields(pr, args.steps, c),
               published_reference=dict(value=0.003983, unit="Mbps",
                                        source="benchmarks/results/data/throughput_results.json:4-14 "
                                               "(reference hardware, NumPy, one frame at a time)"),
               roofline=roofline("polar_sc_1024_default", polar_kernel_name(dec.plan, 10), B, 8 * N + K, kms))
    if pool is not None:
        from oracle import oracle as O
        from oracle import refnumpy as R
        S, S1, S2 = min(1024, B), min(64, B), min(16384, B)
        lh = llr[:S2].cpu().numpy()
        got = out[:S2].cpu().numpy().astype(np.int64)
        fr = dec.frozen_bits
        procs = cpu_processes()
        res["cpu_baseline"] = numpy_baseline(pool, procs, "SC N=1024, default frozen set",
                                             lambda: R.polar_batch(N, 0, fr, lh[:S], pool=pool), S, K, got[:S],
                                             single=(lambda: R.polar_batch(N, 0, fr, lh[:S1]), S1))
        c_port(res["cpu_baseline"], "SC", lambda: O.sc_decode(N, fr, lh, threads=procs), S2, K, got, procs)
    del llr, out, msg
    return res


def bench_config0(args, rt, pool):
    """BASELINE configs[0]: polar N=256 K=128 SC, 100 frames @ 3 dB, made as
    benchmarks/throughput_test.py:196-228 makes them (PolarEncoder default
    frozen set, AWGNChannel(3.0, seed=42), 10 warm-up frames, then 100 random
    messages; tests/test_host.py pins this replay to the reference's own
    frames).  The reference decodes them one at a time in NumPy on one core;
    here the 100 frames are one GPU batch (launch-latency bound: a plumbing
    figure, not a throughput claim)."""
    from polarcode_and_ldpc_amd.channel import AWGNChannel
    from polarcode_and_ldpc_amd.polar import PolarEncoder, SCDecoder
    N, K, F = 256, 128, 100
    state = np.random.get_state()
    enc = PolarEncoder(N, K)
    ch = AWGNChannel(snr_db=3.0, seed=42)
    for _ in range(10):
        ch.transmit(enc.encode(np.random.randint(0, 2, K)), return_llr=True)
    msgs = np.array([np.random.randint(0, 2, K) for _ in range(F)])
    llr_h = np.array([ch.transmit(enc.encode(m), return_llr=True) for m in msgs])
    np.random.set_state(state)
    dec = SCDecoder(N, K, frozen_bits=enc.get_frozen_bits_positions())
    llr = torch.from_numpy(llr_h).cuda()
    out = torch.empty((F, K), dtype=torch.uint8, device="cuda")
    kt = KernelTimer()
    dt, pr = timed_steps(lambda: kt(lambda: dec.plan.decode(llr, out)), args.steps, args.warmup, rt,
                         on_timed=kt.reset)
    got = out.cpu().numpy().astype(np.int64)
    res = dict(metric="decoded info-Mbps, polar N=256 K=128 SC, the 100 throughput_test.py frames @ 3 dB "
                      "(BASELINE configs[0])", value=F * rt.world * args.steps * K / dt / 1e6, unit="info-Mbps",
               ms_per_step=dt / args.steps * 1e3, kernel_ms=kt.mean_ms(), frames=F,
               rank_ms_per_step=[t / args.steps * 1e3 for t in pr],
               frame_errors=int((got != msgs).any(axis=1).sum()),
               roofline=roofline("polar_sc_256", polar_kernel_name(dec.plan, 8), F, 8 * N + K, kt.mean_ms()))
    if pool is not None:
        from oracle import refnumpy as R
        fr = dec.frozen_bits
        res["cpu_baseline"] = numpy_baseline(pool, cpu_processes(), "SC N=256, the 100 configs[0] frames",
                                             lambda: R.polar_batch(N, 0, fr, llr_h, pool=pool), F, K, got,
                                             single=(lambda: R.polar_batch(N, 0, fr, llr_h), F))
        res["cpu_baseline"]["note"] = "single_core is the reference configuration itself (one process, NumPy)"
    return res


# ---------------------------------------------------------------- LDPC
LDPC_KERNELS = {1: "ldpc_decode_kernel<BP>", 2: "ldpc_reg_kernel<BP,DV=3>", 3: "ldpc_check_kernel<BP>",
                5: "ldpc_ms_compact_kernel<8,3,6,true>", 7: "ldpc_bp_grp_kernel<3,6,2,false>",
                8: "ldpc_ms36_kernel<8>"}


def ldpc_kernel_name(plan):
    """The kernel pl_plan_get_info's `reserved` names (capi.cpp pl_plan_get_info)."""
    r = int(plan.info.reserved)
    if r == 7:  # the degree-grouped BP kernel: frames per workgroup (FPG) as its last template argument
        return "ldpc_bp_grp_kernel<3,6,2,false,%d>" % max(1, int(plan.info.frames_per_block))
    return LDPC_KERNELS.get(r, "ldpc kernel id %d" % r)


def bench_ldpc_valid(args, rt, pool, enc, plan, kname):
    """Second frame source (SURVEY §8 d): valid codewords (all-zero; BP is
    codeword-symmetric) at the same SNR, early stop on."""
    from polarcode_and_ldpc_amd.channel import AWGNChannel
    n, k, B = enc.n, enc.k, args.batch
    llr0 = AWGNChannel(args.snr).llr_batch_device(None, n, B, seed=4243, frame_offset=rt.rank * B)
    out0 = torch.empty((B, n), dtype=torch.uint8, device="cuda")
    its0 = torch.empty((B,), dtype=torch.int32, device="cuda")
    vkt = KernelTimer()
    dt0, pr0 = timed_steps(lambda: vkt(lambda: plan.decode(llr0, out0, its0)), args.steps, args.warmup, rt,
                           on_timed=vkt.reset)
    vkms = vkt.mean_ms()
    res = dict(value=B * rt.world * args.steps * k / dt0 / 1e6, unit="info-Mbps",
               ms_per_step=dt0 / args.steps * 1e3, kernel_ms=vkms,
               roofline=roofline("ldpc_bp_504_valid", kname, B, 9 * n, vkms),
               rank_ms_per_step=[t / args.steps * 1e3 for t in pr0],
               mean_iterations=float(its0.double().mean().item()),
               bit_errors=int(out0.sum().item()),
               what="all-zero codeword frames (device AWGN), BP max_iter=20, early stop")
    if pool is not None:
        from oracle import refnumpy as R
        S = min(args.cpu_frames_numpy, B)
        lh = llr0[:S].cpu().numpy()
        res["cpu_baseline"] = numpy_baseline(
            pool, cpu_processes(), "BP-20 (504,252), all-zero codewords, early stop",
            lambda: R.ldpc_batch(enc.H, lh, "bp", 20, True, pool=pool)[0], S, k,
            out0[:S].cpu().numpy().astype(np.int64))
    return res


def bench_ldpc(args, rt, pool):
    from polarcode_and_ldpc_amd.channel import AWGNChannel
    from polarcode_and_ldpc_amd.ldpc import BPDecoder, LDPCEncoder

    n, k, B = 504, 252, args.batch
    enc = LDPCEncoder(n, k, dv=3, dc=6, seed=42)  # throughput_test.py:285 (rank-251 H, direct solving)
    dec = BPDecoder(enc.H, max_iter=20)
    plan = dec.plan
    kname = ldpc_kernel_name(plan)
    if "ldpc" not in args.sec:  # a profiling pass of the valid-codeword key alone
        return dict(valid_codewords=bench_ldpc_valid(args, rt, pool, enc, plan, kname))
    rs = np.random.RandomState(42 + rt.rank)
    U = 4096  # distinct messages, tiled; every frame gets its own noise
    base = enc.encode_batch(rs.randint(0, 2, (U, k)))
    cw = torch.from_numpy(np.tile(base, (B // U + 1, 1))[:B].astype(np.uint8)).cuda()
    llr = AWGNChannel(args.snr).llr_batch_device(cw, n, B, seed=4242, frame_offset=rt.rank * B)
    out = torch.empty((B, n), dtype=torch.uint8, device="cuda")
    its = torch.empty((B,), dtype=torch.int32, device="cuda")
    dt, per_rank, kms, c = decode_loop(rt, plan, llr, out, cw, k, args.steps, args.warmup, its)
    counted = rank_fields(per_rank, args.steps, c)
    res = dict(metric="decoded info-Mbps, LDPC (504,252) BP max_iter=20, reference-harness frames @ %.1f dB"
                      % args.snr,
               value=B * rt.world * args.steps * k / dt / 1e6, unit="info-Mbps", ms_per_step=dt / args.steps * 1e3,
               rank_ms_per_step=[t / args.steps * 1e3 for t in per_rank], kernel_ms=kms,
               frames_counted=counted["frames_counted"], mean_iterations=float(its.double().mean().item()),
               roofline=roofline("ldpc_bp_504", kname, B, 9 * n, kms))
    res["roofline"]["limit"] = "VALU issue (fp64 transcendentals): see roofline.valu"
    if "ldpc_valid" in args.sec:
        res["valid_codewords"] = bench_ldpc_valid(args, rt, pool, enc, plan, kname)
    if pool is not None:
        from oracle import oracle as O
        from oracle import refnumpy as R
        from polarcode_and_ldpc_amd.ldpc import dense_to_csr
        S, S1, S2 = min(args.cpu_frames_numpy, B), min(8, B), min(args.cpu_frames_ldpc, B)
        llr_h = llr[:max(S, S2)].cpu().numpy()
        got = out[:llr_h.shape[0]].cpu().numpy().astype(np.int64)
        procs = cpu_processes()
        res["cpu_baseline"] = numpy_baseline(
            pool, procs, "BP-20 (504,252)", lambda: R.ldpc_batch(enc.H, llr_h[:S], "bp", 20, True, pool=pool)[0],
            S, k, got[:S], single=(lambda: R.ldpc_batch(enc.H, llr_h[:S1], "bp", 20, True)[0], S1))
        rp, ci = dense_to_csr(enc.H)
        c_port(res["cpu_baseline"], "BP-20",
               lambda: O.ldpc_decode(rp, ci, n, llr_h[:S2], "bp", 20, True, 1.0, threads=procs)[0], S2, k,
               got[:S2], procs)
    return res


# ---------------------------------------------------------------- configs[3], configs[4]
def bench_cascl(args, rt, pool=None):
    """BASELINE configs[3]: CA-SCL N=1024 K=512 L=32 + CRC-8 (the CRC is inside
    the K info bits, src/polar/encoder.py:74-78)."""
    from polarcode_and_ldpc_amd import _native
    from polarcode_and_ldpc_amd.channel import AWGNChannel
    from polarcode_and_ldpc_amd.harness.ber import simulate_polar
    from polarcode_and_ldpc_amd.polar import CASCLDecoder, construct_frozen_set
    from polarcode_and_ldpc_amd.polar.utils import CRC_POLYNOMIALS
    N, K, L, B = 1024, 512, 32, args.batch
    fr = construct_frozen_set(N, K, 2.0)
    dec = CASCLDecoder(N, K, list_size=L, frozen_bits=fr, crc_polynomial="CRC-8")
    off = rt.rank * B
    msg = torch.empty((B, K), dtype=torch.uint8, device="cuda")
    _native.random_bits(44, off, msg)
    _native.crc_append(msg, K - 8, 8, CRC_POLYNOMIALS["CRC-8"])
    cw = torch.empty((B, N), dtype=torch.uint8, device="cuda")
    _native.polar_encode(dec.plan, msg, cw)
    llr = AWGNChannel(1.0).llr_batch_device(cw, N, B, seed=44, frame_offset=off)
    del cw
    out = torch.empty((B, K), dtype=torch.uint8, device="cuda")
    steps = min(args.steps, args.extra_steps)
    dt, pr, kms, c = decode_loop(rt, dec.plan, llr, out, msg, K, steps, 1)
    res = dict(metric="decoded info-Mbps, CA-SCL N=1024 K=512 L=32 + CRC-8 (BASELINE configs[3]) @ 1.0 dB",
               value=B * rt.world * steps * K / dt / 1e6, unit="info-Mbps", steps=steps,
               ms_per_step=dt / steps * 1e3, kernel_ms=kms, frames_per_gpu=B, **rank_fields(pr, steps, c),
               ber=float(c[0]) / max(1, c[2] * K), fer=float(c[1]) / max(1, c[2]),
               roofline=roofline("polar_cascl_1024_l32", polar_kernel_name(dec.plan, 10), B, 8 * N + K, kms))
    if pool is not None:
        # the C restatement of CA-SCL (oracle/refcpu.c) on 64 frames of the same
        # batch, against the GPU's CA-SCL bits; the reference's own NumPy path
        # for these frames is its plain SCLDecoder (use_crc is inert, decoder.py:
        # 202-203, 259), timed on 32 frames against a GPU plain-SCL decode of them
        from oracle import oracle as O
        from oracle import refnumpy as R
        from polarcode_and_ldpc_amd.polar import SCLDecoder
        S, S2 = min(args.cpu_frames_l32, B), min(64, B)
        lh = llr[:max(S, S2)].cpu().numpy()
        procs = cpu_processes()
        plain = SCLDecoder(N, K, L, frozen_bits=fr).decode_batch(torch.from_numpy(lh[:S]).cuda())
        res["cpu_baseline"] = numpy_baseline(pool, procs, "plain SCL N=1024 L=32 (the reference's SCLDecoder; "
                                             "use_crc inert)", lambda: R.polar_batch(N, L, fr, lh[:S], pool=pool), S,
                                             K, plain.cpu().numpy().astype(np.int64))
        c_port(res["cpu_baseline"], "CA-SCL L=32 CRC-8",
               lambda: O.cascl_decode(N, L, fr, lh[:S2], "CRC-8", threads=procs), S2, K,
               out[:S2].cpu().numpy().astype(np.int64), procs)
    del llr, out, msg
    if "sweep" in args.sec:
        t0 = time.perf_counter()
        snrs = np.arange(-2.0, 5.5, 1.0)
        _, _, pts = simulate_polar(snrs, args.sweep_frames, args.sweep_max_errors, {"encoding": {"N": N, "K": K}},
                                   list_size=L, crc_polynomial="CRC-8", batch=min(B, 32768), seed=3)
        res["sweep"] = dict(what="harness.ber.simulate_polar: CA-SCL L=32 CRC-8, -2..5 dB Es/N0, max_errors=%d, "
                                 "<= %d frames per point, frames sharded over %d rank(s), one all-reduce per round"
                                 % (args.sweep_max_errors, args.sweep_frames, rt.world),
                            seconds=time.perf_counter() - t0,
                            points=[dict(snr_db=p.snr_db, frames=p.frames, frame_errors=p.frame_errors,
                                         bit_errors=p.bit_errors, ber=p.ber, fer=p.fer, fer_ci=list(p.fer_ci))
                                    for p in pts])
    return res


def bench_long(args, rt, pool=None):
    """BASELINE configs[4] per GPU: 1 M frames over 8 GPUs = 131 072 frames each."""
    B = args.long_batch
    steps = min(args.steps, args.extra_steps)
    res = {}
    if "long_polar" in args.sec:
        res.update(_long_polar(rt, B, steps, pool))
    for es in (True, False):
        if ("long_ms" if es else "long_ms_noes") in args.sec:
            res.update(_long_ms(rt, B, steps, es, pool))
    return res


def _long_polar(rt, B, steps, pool=None):
    N, K = 4096, 2048
    dec, _, msg, llr = polar_fixture(rt, N, K, 8, B, 1.0, 45)
    out = torch.empty((B, K), dtype=torch.uint8, device="cuda")
    dt, pr, kms, c = decode_loop(rt, dec.plan, llr, out, msg, K, steps, 1)
    res = {"polar_4096_l8": dict(
        metric="decoded info-Mbps, polar N=4096 K=2048 SCL L=8 @ 1.0 dB", value=B * rt.world * steps * K / dt / 1e6,
        unit="info-Mbps", steps=steps, ms_per_step=dt / steps * 1e3, kernel_ms=kms, frames_per_gpu=B,
        llr_bytes_per_gpu=B * N * 8, fer=float(c[1]) / max(1, c[2]), **rank_fields(pr, steps, c),
        roofline=roofline("polar_scl_4096_l8", polar_kernel_name(dec.plan, 12), B, 8 * N + K, kms))}
    if pool is not None:
        from oracle import oracle as O
        from oracle import refnumpy as R
        S, S2 = min(16, B), min(128, B)
        lh = llr[:S2].cpu().numpy()
        got = out[:S2].cpu().numpy().astype(np.int64)
        procs = cpu_processes()
        fr = dec.frozen_bits
        r = res["polar_4096_l8"]["cpu_baseline"] = numpy_baseline(
            pool, procs, "SCL N=4096 L=8", lambda: R.polar_batch(N, 8, fr, lh[:S], pool=pool), S, K, got[:S])
        c_port(r, "SCL N=4096 L=8", lambda: O.scl_decode(N, 8, fr, lh, threads=procs), S2, K, got, procs)
    del dec, msg, llr, out
    torch.cuda.empty_cache()
    return res


def _long_ms(rt, B, steps, es, pool=None):
    from polarcode_and_ldpc_amd.channel import AWGNChannel
    from polarcode_and_ldpc_amd.ldpc import MSDecoder
    from polarcode_and_ldpc_amd.ldpc.matrix import regular_construction
    n = 8192
    H = regular_construction(n, 3, 6, seed=11)  # every check degree 6 (min-sum needs >= 2)
    k = n - H.shape[0]
    dec = MSDecoder(H, max_iter=20, normalization=1.0, early_stop=es)
    llr = AWGNChannel(1.5).llr_batch_device(None, n, B, seed=46, frame_offset=rt.rank * B)
    out = torch.empty((B, n), dtype=torch.uint8, device="cuda")
    its = torch.empty((B,), dtype=torch.int32, device="cuda")
    zero = torch.zeros((B, k), dtype=torch.uint8, device="cuda")
    dt, pr, kms, c = decode_loop(rt, dec.plan, llr, out, zero, k, steps, 1, its)
    res = {"ldpc_8192_ms20" + ("" if es else "_no_early_stop"): dict(
        metric="decoded info-Mbps, LDPC n=8192 (3,6)-regular min-sum max_iter=20, all-zero codeword @ 1.5 dB, "
               "early stop %s" % ("on" if es else "off"),
        value=B * rt.world * steps * k / dt / 1e6, unit="info-Mbps", steps=steps, ms_per_step=dt / steps * 1e3,
        kernel_ms=kms, frames_per_gpu=B, mean_iterations=float(its.double().mean().item()),
        llr_bytes_per_gpu=B * n * 8, fer=float(c[1]) / max(1, c[2]), **rank_fields(pr, steps, c),
        roofline=roofline("ldpc_ms_8192" + ("" if es else "_noes"), ldpc_kernel_name(dec.plan), B, 9 * n, kms))}
    if pool is not None:
        from oracle import oracle as O
        from oracle import refnumpy as R
        from polarcode_and_ldpc_amd.ldpc import dense_to_csr
        S, S2 = min(16, B), min(512, B)
        lh = llr[:S2].cpu().numpy()
        got = out[:S2].cpu().numpy().astype(np.int64)
        procs = cpu_processes()
        key = next(iter(res))
        r = res[key]["cpu_baseline"] = numpy_baseline(
            pool, procs, "MS-20 n=8192 early stop %s" % ("on" if es else "off"),
            lambda: R.ldpc_batch(H, lh[:S], "ms", 20, es, 1.0, pool=pool)[0], S, k, got[:S])
        rp, ci = dense_to_csr(H)
        c_port(r, "MS-20 n=8192", lambda: O.ldpc_decode(rp, ci, n, lh, "ms", 20, es, 1.0, threads=procs)[0], S2, k,
               got, procs)
    del llr, out, its, zero, dec
    torch.cuda.empty_cache()
    return res


# ---------------------------------------------------------------- CPU stub
def bench_stub(args, rt):
    """--cpu-stub: the rank / barrier / timing / counter all-reduce path of
    bench_polar on CPU tensors with a stub decode (hard decision of synthetic
    LLRs, one bit flipped in every 7th global frame).  A plumbing check: the
    counters must equal the closed form for the global frame range."""
    N, K, B = 256, 128, args.batch
    g = torch.Generator().manual_seed(42 + rt.rank)
    msg = torch.randint(0, 2, (B, K), generator=g, dtype=torch.uint8)
    frames = torch.arange(rt.rank * B, (rt.rank + 1) * B)
    llr = torch.zeros((B, N), dtype=torch.float64)
    llr[:, :K] = 1.0 - 2.0 * msg.double()
    flip = frames % 7 == 0
    llr[flip, (frames[flip] % K)] *= -1.0
    out = torch.empty_like(msg)
    counts = torch.zeros(3, dtype=torch.int64)
    sc = torch.zeros(3, dtype=torch.int64)

    def step():
        out.copy_((llr[:, :K] < 0).to(torch.uint8))
        e = (out != msg).sum(dim=1)
        sc.copy_(torch.stack([e.sum(), (e > 0).sum(), torch.tensor(B)]).to(torch.int64))
        rt.all_reduce(sc)
        counts.add_(sc)

    dt, per_rank = timed_steps(step, args.steps, args.warmup, rt, on_timed=counts.zero_)
    return dict(value=B * rt.world * args.steps * K / dt / 1e6, ms_per_step=dt / args.steps * 1e3,
                rank_ms_per_step=[t / args.steps * 1e3 for t in per_rank],
                counts=[int(x) for x in counts.tolist()], B=B)


# ---------------------------------------------------------------- output
MAX_LINE = 6000  # the driver keeps ~8 KB of stdout: the one JSON line must fit well inside it
PMC_NOTE = ("roofline.traffic: HBM-side bytes per launch (2*FETCH_SIZE+WRITE_SIZE, gfx950 correction) from a "
            "separate rocprofv3 --pmc pass of the same build at the same batch (profiles/pmc_traffic.json); "
            "achieved/frac from algorithmic bytes over HIP-event kernel time in this run")


def _r(x, sig=4):
    """Round floats to `sig` significant digits (None / ints / strings pass)."""
    if isinstance(x, float):
        if x != x or x in (float("inf"), float("-inf")):
            return None
        return float("%.*g" % (sig, x))
    if isinstance(x, dict):
        return {k: _r(v, sig) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_r(v, sig) for v in x]
    return x


def _roof_short(r):
    if not r:
        return None
    return _r(dict(bound=r.get("bound"), achieved=r.get("achieved"), peak=r.get("peak"), unit=r.get("unit"),
                   frac=r.get("frac"), traffic=r.get("traffic"), kernel=r.get("kernel"),
                   kernel_ms=r.get("kernel_ms"), frames=r.get("frames_per_launch"),
                   traffic_same_build=r.get("traffic_same_build")))


def _cpu_short(c, with_sample=False):
    if not c:
        return None
    out = dict(value=c.get("value"), unit=c.get("unit"), cores=c.get("cores"), kind=c.get("kind"),
               mismatches=c.get("mismatching_frames_vs_gpu"))
    if with_sample:
        out["sample"] = c.get("sample")
    if c.get("single_core"):
        out["single_core"] = c["single_core"].get("value")
    if c.get("c_port"):
        out["c_port"] = c["c_port"].get("value")
        out["c_port_mismatches"] = c["c_port"].get("mismatching_frames_vs_gpu")
    return _r(out)


def _key_short(k):
    """value, ms_per_step, kernel_ms, roofline frac / traffic, CPU figures of one secondary key."""
    r = k.get("roofline") or {}
    c = k.get("cpu_baseline") or {}
    out = dict(value=k.get("value"), ms_per_step=k.get("ms_per_step"), kernel_ms=k.get("kernel_ms"),
               frac=r.get("frac"), traffic=r.get("traffic"))
    for f in ("mean_iterations", "fer"):
        if k.get(f) is not None:
            out[f] = k[f]
    if c:
        out["cpu"] = c.get("value")
        out["cpu_cores"] = c.get("cores")
        out["cpu_mismatches"] = c.get("mismatching_frames_vs_gpu")
        if c.get("c_port"):
            out["cpu_c_port"] = c["c_port"].get("value")
    return _r(out)


def compact_line(full, detail_path=None):
    """The one stdout line: the contract fields, the headline roofline and
    cpu_baseline, and a compact summary of every secondary key.  Wave shares,
    VALU splits, per-rank detail of the secondary keys and the sweep's
    intervals go to the detail file (`--detail-out`)."""
    line = {k: full.get(k) for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step",
                                     "rank_ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
                                     "data", "config")}
    line = _r(line, 6)
    line["roofline"] = _roof_short(full.get("roofline"))
    if line["roofline"] is not None:
        line["roofline"]["traffic_source"] = "separate PMC pass (see pmc_note)"
    line["cpu_baseline"] = _cpu_short(full.get("cpu_baseline"), with_sample=True)
    if full.get("cpu_baseline_note"):
        line["cpu_baseline_note"] = full["cpu_baseline_note"]
    line["ber"], line["fer"] = _r(full.get("ber")), _r(full.get("fer"))
    keys = {}
    for name in ("end_to_end", "default_frozen_set", "polar_sc_default", "config0_sc_256", "ldpc", "cascl_l32"):
        if full.get(name):
            keys[name] = _key_short(full[name])
    if full.get("ldpc", {}).get("valid_codewords"):
        keys["ldpc.valid_codewords"] = _key_short(full["ldpc"]["valid_codewords"])
    sw = (full.get("cascl_l32") or {}).get("sweep")
    if sw:
        keys["cascl_l32.sweep"] = dict(seconds=_r(sw.get("seconds")),
                                       points=[[p["snr_db"], p["frames"], p["frame_errors"], _r(p["ber"], 3),
                                                _r(p["fer"], 3)] for p in sw.get("points", [])],
                                       cols="snr_db,frames,frame_errors,ber,fer")
    for name, v in (full.get("long_block") or {}).items():
        keys["long_block." + name] = _key_short(v)
    line["keys"] = keys
    line["pmc_note"] = PMC_NOTE
    if detail_path:
        line["detail"] = detail_path
    s = json.dumps(line)
    if len(s) > MAX_LINE:  # never exceed the driver's tail: drop the secondary keys' CPU figures, then samples
        for v in keys.values():
            for f in ("cpu_cores", "cpu_mismatches", "cpu_c_port", "ms_per_step"):
                v.pop(f, None)
        if line["cpu_baseline"]:
            line["cpu_baseline"].pop("sample", None)
        line["pmc_note"] = "traffic from a separate PMC pass (profiles/pmc_traffic.json)"
    return line


def write_detail(full, path):
    """The full result (wave shares, VALU splits, per-rank times, samples, sweep
    intervals) as JSON; returns the path written (relative to the repo) or None."""
    if not path:
        return None
    p = path if os.path.isabs(path) else os.path.join(ROOT, path)
    try:
        os.makedirs(os.path.dirname(p), exist_ok=True)
        with open(p, "w") as f:
            json.dump(full, f, indent=1)
    except OSError as e:
        log("bench.py: could not write the detail file %s: %s" % (p, e))
        return None
    log("bench.py: full result in %s" % p)
    return os.path.relpath(p, ROOT)


# ---------------------------------------------------------------- main
def self_launch(args):
    """--gpus N > 1 without a torch.distributed environment: start N ranks under
    torch.distributed.run as a child process (nothing here has touched the GPU)
    and exit with its status."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    log("bench.py: launching %d ranks: %s" % (args.gpus, " ".join(cmd)))
    return subprocess.call(cmd, env=env)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--list-size", type=int, default=8)
    ap.add_argument("--snr", type=float, default=3.0)
    ap.add_argument("--cpu-frames", type=int, default=4096, help="frames for the C-port baseline (polar)")
    ap.add_argument("--cpu-frames-ldpc", type=int, default=32768, help="frames for the C-port baseline (LDPC)")
    ap.add_argument("--cpu-frames-numpy", type=int, default=256, help="frames for the NumPy baseline")
    ap.add_argument("--cpu-frames-l32", type=int, default=32, help="frames for the NumPy SCL L=32 baseline")
    ap.add_argument("--long-batch", type=int, default=131072, help="configs[4] frames per GPU (1 M / 8)")
    ap.add_argument("--extra-steps", type=int, default=5, help="cap on timed steps of the configs[3]/[4] keys")
    ap.add_argument("--sweep-frames", type=int, default=131072)
    ap.add_argument("--sweep-max-errors", type=int, default=200)
    ap.add_argument("--skip-cpu", action="store_true")
    ap.add_argument("--skip-ldpc", action="store_true")
    ap.add_argument("--skip-configs", action="store_true", help="no configs[3]/[4] keys")
    ap.add_argument("--skip-sweep", action="store_true", help="no CA-SCL BER sweep")
    ap.add_argument("--skip-extra", action="store_true",
                    help="only the headline decodes (no end-to-end / valid-codeword / configs[3,4] runs)")
    ap.add_argument("--sections", default=None,
                    help="comma list of " + ",".join(SECTIONS) + " (profiling passes: one kernel per section)")
    ap.add_argument("--full", action="store_true",
                    help="also run every secondary key (end-to-end, other frozen sets / decoders / sizes, LDPC, "
                         "CA-SCL + BER sweep, long blocks) and the CPU baselines; without it only the headline "
                         "decode is set up, timed and reported")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the headline's decoded bits (a fixed sample of the frames) "
                         "and error counters of the last timed step as DIR/<name>.npy")
    ap.add_argument("--detail-out", default=None,
                    help="file for the full result (stdout carries one compact line); '' = none; "
                         "default: bench_out/bench_detail.json with --full, none without")
    ap.add_argument("--cpu-stub", action="store_true", help="CPU/gloo plumbing check with a stub decode")
    ap.add_argument("--dist-backend", default="nccl", choices=["nccl", "gloo"],
                    help="gloo: host-side counter reduction, ranks may share one GPU (rehearsal only)")
    args = ap.parse_args()
    sec = set(SECTIONS) if args.sections is None else set(args.sections.split(","))
    assert sec <= set(SECTIONS), "unknown section in --sections"
    if args.detail_out is None:
        args.detail_out = "bench_out/bench_detail.json" if args.full else ""
    if not args.full:
        # a plain run: the headline decode alone (its roofline comes from the timed
        # launches' own HIP events), no CPU pool
        if args.sections is not None:
            ap.error("--sections selects among the keys of a --full run: add --full")
        sec = {"polar"}
        args.skip_cpu = True
    if args.dump_outputs and (args.cpu_stub or "polar" not in sec):
        ap.error("--dump-outputs writes the headline decode's outputs: it needs the polar section and no --cpu-stub")
    if args.skip_extra:
        sec &= {"polar", "ldpc"}
    if args.skip_ldpc:
        sec -= {"ldpc", "ldpc_valid"}
    if args.skip_configs:
        sec -= {"cascl", "sweep", "long_polar", "long_ms", "long_ms_noes"}
    if args.skip_sweep:
        sec.discard("sweep")
    args.sec = sec

    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        sys.exit(self_launch(args))

    rt = Runtime(args.cpu_stub, args.dist_backend)
    if args.cpu_stub:
        r = bench_stub(args, rt)
        if rt.rank == 0:
            print(json.dumps({"metric": METRIC + " [cpu-stub plumbing check, not a measurement]", "value": r["value"],
                              "unit": "info-Mbps", "n_gpus": rt.world, "steps": args.steps, "warmup": args.warmup,
                              "ms_per_step": r["ms_per_step"], "rank_ms_per_step": r["rank_ms_per_step"],
                              "higher_is_better": True, "scaling": "weak", "stub": True, "counts": r["counts"],
                              "frames_per_rank": r["B"]}), flush=True)
        rt.close()
        return

    # the CPU-baseline pool is spawned before the first GPU call (rank 0, N = 1)
    pool = None
    if rt.rank == 0 and rt.world == 1 and not args.skip_cpu:
        from oracle import refnumpy as R
        pool = R.make_pool(cpu_processes())
        # every worker started before the first timed region: spawned workers
        # re-import this module (torch included), and 16 of them doing so beside
        # the headline steps delayed its launches (r03_g: 7.14 ms per step
        # around a 6.11 ms kernel; the later keys, timed after, were unaffected)
        pool.map(time.sleep, [0.5] * cpu_processes(), chunksize=1)
    pol = bench_polar(args, rt, pool)
    extra = {}
    if "sc_default" in args.sec:
        extra["polar_sc_default"] = bench_sc_default(args, rt, pool)
    if "config0" in args.sec:
        extra["config0_sc_256"] = bench_config0(args, rt, pool)
    ldp = bench_ldpc(args, rt, pool) if args.sec & {"ldpc", "ldpc_valid"} else None
    if "cascl" in args.sec:
        extra["cascl_l32"] = bench_cascl(args, rt, pool)
    if args.sec & {"long_polar", "long_ms", "long_ms_noes"}:
        extra["long_block"] = bench_long(args, rt, pool)
    if pool is not None:
        pool.close()
    if rt.rank == 0:
        full = {
            "metric": METRIC, "value": pol.get("value"), "unit": "info-Mbps", "n_gpus": rt.world,
            "steps": args.steps, "warmup": args.warmup, "ms_per_step": pol.get("ms_per_step"),
            "rank_ms_per_step": pol.get("rank_ms_per_step"),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f64",
            "data": "synthetic: random messages, device polar encoder, device AWGN (Philox) at %.1f dB Es/N0" % args.snr,
            "config": {"workload": "polar N=1024 K=512 SCL L=%d decode (BASELINE configs[1]), bit-reversed "
                                   "Bhattacharyya(2 dB) frozen set" % args.list_size,
                       "global_batch": args.batch * rt.world, "frames_per_gpu": args.batch,
                       "parallelism": "frame-sharded x%d (one RCCL all-reduce of error counters per step)" % rt.world},
            "roofline": pol.get("roofline"),
            "cpu_baseline": pol.get("cpu_baseline"),
            "ber": pol.get("ber"), "fer": pol.get("fer"), "plan": pol.get("plan"),
            "end_to_end": pol.get("end_to_end"),
            "default_frozen_set": pol.get("default_frozen_set"),
        }
        if ldp is not None:
            full["ldpc"] = ldp
        full.update(extra)
        if full["cpu_baseline"] is None:
            # the contract times the CPU path on rank 0 at N = 1 only: the N = 1
            # line of the same build carries it (the host cores are shared by the
            # N ranks here, so a figure taken now would measure contention)
            full["cpu_baseline_note"] = ("not measured: %s" % (
                "a plain run times the headline alone (--full adds it)" if not args.full else
                "--skip-cpu" if args.skip_cpu else "timed on rank 0 at N = 1 only (see the N = 1 line of this build)"))
        path = write_detail(full, args.detail_out)
        print(json.dumps(compact_line(full, path)), flush=True)
    rt.close()


if __name__ == "__main__":
    main()

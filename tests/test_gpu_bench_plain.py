"""A plain `bench.py --gpus 1 --steps K --warmup W` run measures the headline
alone: one JSON line with the contract fields, exactly K timed steps, no
secondary key, no CPU baseline, no detail file.  `--dump-outputs DIR` leaves the
last timed step's decoded bits and the device error counters as float .npy
files, and the bits equal a decode of the same frames through the Python API."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_headline_only_and_dump(gpu, tmp_path):
    B, steps = 2048, 3
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    dump = str(tmp_path / "dump")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", "1", "--batch", str(B), "--snr", "-1.0", "--dump-outputs", dump],
                       capture_output=True, text=True, timeout=120, env=env, cwd=str(tmp_path))
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    r = json.loads(lines[0])
    assert r["n_gpus"] == 1 and r["steps"] == steps and r["warmup"] == 1
    assert r["unit"] == "info-Mbps" and r["higher_is_better"] is True and r["dtype"] == "f64"
    assert r["ms_per_step"] > 0
    assert r["value"] == pytest.approx(B * 512 / (r["ms_per_step"] * 1e-3) / 1e6, rel=1e-4)
    assert r["keys"] == {} and r["cpu_baseline"] is None and "detail" not in r
    assert sorted(os.listdir(str(tmp_path))) == ["dump"]  # nothing but the dump is written

    a = {n: np.load(os.path.join(dump, n)) for n in sorted(os.listdir(dump))}
    assert sorted(a) == ["decoded_bits.npy", "decoded_bits_frames.npy", "error_counts.npy"]
    assert sum(os.path.getsize(os.path.join(dump, n)) for n in a) <= 64 * 1000 * 1000
    bits, idx, counts = a["decoded_bits.npy"], a["decoded_bits_frames.npy"], a["error_counts.npy"]
    assert bits.dtype == np.float32 and bits.shape == (B, 512) and np.isin(bits, (0.0, 1.0)).all()
    assert np.array_equal(idx, np.arange(B))
    assert counts.dtype == np.float64 and counts[2] == B * steps  # counted over exactly the timed steps
    assert 0 < counts[1] < B * steps and counts[1] % steps == 0  # at -1 dB some frames fail, the same ones every step
    assert r["fer"] == pytest.approx(counts[1] / counts[2], rel=1e-3)

    # the same frames (seed 42, global frame indices from 0) decoded through the Python API
    import torch
    from polarcode_and_ldpc_amd import _native
    from polarcode_and_ldpc_amd.channel import AWGNChannel
    from polarcode_and_ldpc_amd.polar import SCLDecoder, construct_frozen_set
    dec = SCLDecoder(1024, 512, list_size=8, frozen_bits=construct_frozen_set(1024, 512, 2.0))
    msg = torch.empty((B, 512), dtype=torch.uint8, device="cuda")
    _native.random_bits(42, 0, msg)
    cw = torch.empty((B, 1024), dtype=torch.uint8, device="cuda")
    _native.polar_encode(dec.plan, msg, cw)
    llr = AWGNChannel(-1.0).llr_batch_device(cw, 1024, B, seed=42, frame_offset=0)
    got = dec.decode_batch(llr).cpu().numpy()
    assert np.array_equal(got.astype(np.float32), bits)
    wrong = (got != msg.cpu().numpy()).any(axis=1).sum()
    assert counts[1] == wrong * steps

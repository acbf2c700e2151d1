"""The driver keeps only the last ~8 KB of bench.py's stdout (VERDICT r03:
BENCH_r03 parsed null because the full line was 24 KB).  The stdout line is
built by bench.compact_line; this checks it on the round-3 payload."""
import json
import os

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _payload():
    with open(os.path.join(ROOT, "profiles", "r03_j", "bench.json")) as f:
        return json.load(f)


def test_compact_line_fits_driver_tail():
    full = _payload()
    line = bench.compact_line(full, "gpurun_out/bench_detail.json")
    s = json.dumps(line)
    assert len(s) <= bench.MAX_LINE, len(s)
    assert "\n" not in s
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "dtype", "config",
              "roofline", "cpu_baseline", "higher_is_better", "scaling", "vs_baseline", "data"):
        assert k in line, k
    r = line["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "kernel", "kernel_ms"):
        assert k in r and r[k] is not None, k
    c = line["cpu_baseline"]
    for k in ("value", "cores", "kind", "mismatches"):
        assert k in c and c[k] is not None, k
    assert abs(line["value"] - full["value"]) / full["value"] < 1e-5
    # every secondary key keeps a compact summary with its roofline fraction
    for name in ("ldpc", "cascl_l32", "end_to_end", "default_frozen_set", "polar_sc_default", "config0_sc_256",
                 "long_block.polar_4096_l8", "long_block.ldpc_8192_ms20",
                 "long_block.ldpc_8192_ms20_no_early_stop", "ldpc.valid_codewords"):
        assert name in line["keys"], name
        assert line["keys"][name]["value"] is not None
    for name in ("ldpc", "cascl_l32", "long_block.polar_4096_l8"):
        assert line["keys"][name]["frac"] is not None
    assert json.loads(s) == line


def test_dump_outputs_sample_is_fixed_and_bounded(tmp_path, monkeypatch):
    """--dump-outputs: float32/float64 .npy files; an output above the byte budget is
    cut to the same seeded, ascending sample of rows on every call."""
    import numpy as np
    import torch
    B, K = 1000, 16
    out = torch.from_numpy(np.random.RandomState(1).randint(0, 2, (B, K)).astype(np.uint8))
    counts = np.array([5, 3, 2000], dtype=np.int64)
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 100 * 4 * K)
    dirs = [str(tmp_path / "a"), str(tmp_path / "b")]
    for d in dirs:
        bench.dump_outputs(d, out, counts)
    a, b = ({n: np.load(os.path.join(d, n)) for n in sorted(os.listdir(d))} for d in dirs)
    assert sorted(a) == ["decoded_bits.npy", "decoded_bits_frames.npy", "error_counts.npy"]
    for n in a:
        assert a[n].dtype in (np.float32, np.float64) and np.array_equal(a[n], b[n]), n
    idx = a["decoded_bits_frames.npy"].astype(np.int64)
    assert idx.shape == (100,) and (np.diff(idx) > 0).all() and 0 <= idx[0] and idx[-1] < B
    assert a["decoded_bits.npy"].shape == (100, K) and a["decoded_bits.npy"].nbytes <= 100 * 4 * K
    assert np.array_equal(a["decoded_bits.npy"], out.numpy()[idx].astype(np.float32))
    assert np.array_equal(a["error_counts.npy"], [5.0, 3.0, 2000.0])
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", B * 4 * K)  # the whole output fits: no sampling
    bench.dump_outputs(dirs[0], out, counts)
    assert np.array_equal(np.load(os.path.join(dirs[0], "decoded_bits.npy")), out.numpy().astype(np.float32))
    assert np.array_equal(np.load(os.path.join(dirs[0], "decoded_bits_frames.npy")), np.arange(B))


def test_sections_need_full():
    """Secondary keys are measured only behind --full: asking for one without it is an error."""
    import subprocess
    import sys
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--sections", "ldpc"], capture_output=True,
                       text=True, timeout=120, cwd=ROOT)
    assert p.returncode == 2 and "--full" in p.stderr and p.stdout == ""


def test_compact_line_survives_extra_ranks():
    """An 8-rank line (per-rank times) stays under the limit too."""
    full = _payload()
    full["rank_ms_per_step"] = [6.123456789] * 8
    for v in full.values():
        if isinstance(v, dict) and "rank_ms_per_step" in v:
            v["rank_ms_per_step"] = [6.123456789] * 8
    assert len(json.dumps(bench.compact_line(full, "x"))) <= bench.MAX_LINE

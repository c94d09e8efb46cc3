"""bench.py --dump-outputs / --full: a plain run prints the headline line and nothing it does
not need; --full keeps the roofline, the self-check and the cpu_baseline; the dumped y is the
SpMV of the last timed step, on inputs that are the same from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def _bench_module():
    sys.path.insert(0, ROOT)
    import bench
    return bench


def test_dump_outputs_writes_float_npy(tmp_path):
    import torch
    bench = _bench_module()
    y64 = torch.arange(10, dtype=torch.float64)
    y32 = torch.arange(5, dtype=torch.float32)
    bench.dump_outputs(str(tmp_path / "d"), {"y": y64, "z": y32})
    a, b = np.load(tmp_path / "d" / "y.npy"), np.load(tmp_path / "d" / "z.npy")
    assert a.dtype == np.float64 and np.array_equal(a, y64.numpy())
    assert b.dtype == np.float32 and np.array_equal(b, y32.numpy())


def test_dump_outputs_samples_the_same_entries_over_the_limit(tmp_path):
    import torch
    bench = _bench_module()
    y = torch.arange(100000, dtype=torch.float64)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"y": y}, limit=80000)
    a, b = np.load(tmp_path / "a" / "y.npy"), np.load(tmp_path / "b" / "y.npy")
    assert a.nbytes <= 80000 and a.size > 0
    assert np.array_equal(a, b)                      # fixed, seeded sample
    assert np.all(np.diff(a) > 0) and np.all(np.isin(a, y.numpy()))


@pytest.mark.parametrize("argv", [["--steps", "0"], ["--steps", "-3"]])
def test_steps_must_be_positive(argv, monkeypatch):
    bench = _bench_module()
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    with pytest.raises(SystemExit):
        bench.parse()


def _run(args, tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args,
                       capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def _y_ref(matrix, scale):
    sys.path.insert(0, ROOT)
    from cfs_spmv_amd import synth
    from oracle import oracle
    n, rp, ci, va, _ = synth.generate(matrix, scale)
    x = synth.make_x(n, 42)
    y_ld, absrow = oracle.csr_spmv_ld(n, rp, ci, va, x)
    return y_ld, np.maximum(np.abs(y_ld), absrow)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["sss", "csr"])
def test_plain_run_prints_the_headline_and_dumps_y(fmt, tmp_path):
    out = tmp_path / "out"
    d = _run(["--gpus", "1", "--steps", "7", "--warmup", "2", "--matrix", "pwtk", "--scale", "0.05",
              "--format", fmt, "--dump-outputs", str(out)], tmp_path)
    for k in HEADLINE:
        assert k in d, k
    assert d["steps"] == 7 and d["warmup"] == 2 and d["dtype"] == "f64" and d["ms_per_step"] > 0
    assert "roofline" not in d and "cpu_baseline" not in d
    assert sorted(os.listdir(out)) == ["y.npy"]
    y = np.load(out / "y.npy")
    y_ref, den = _y_ref("pwtk", 0.05)
    assert y.dtype == np.float64 and y.shape == y_ref.shape
    assert float(np.max(np.abs(y - y_ref) / den)) <= 1e-12


@pytest.mark.gpu
def test_full_run_keeps_roofline_and_cpu_baseline(tmp_path):
    d = _run(["--gpus", "1", "--steps", "10", "--warmup", "2", "--matrix", "pwtk", "--scale", "0.05",
              "--full", "--cpu-loops", "4"], tmp_path)
    for k in HEADLINE:
        assert k in d, k
    r = d["roofline"]
    assert r["kernel"] == "cfs_sym_tile_kernel" and r["kernel_samples"] >= 1 and r["kernel_ms"] > 0
    assert d["cpu_baseline"]["value"] > 0

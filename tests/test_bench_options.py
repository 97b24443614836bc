"""CPU: bench.py's options that need no GPU -- --full / --dump-outputs are accepted, --steps is checked before anything touches the GPU,
and the writer behind --dump-outputs (bench.dump_outputs: float32 / float64 arrays, a bounded, seeded, repeatable sample)."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def test_bench_help_lists_full_and_dump_outputs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "--full" in out.stdout and "--dump-outputs" in out.stdout


def test_bench_rejects_zero_steps():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 2 and "--steps must be >= 1" in out.stderr, out.stderr[-2000:]


def test_dump_outputs_writes_bounded_repeatable_float_arrays(tmp_path):
    import bench
    rng = np.random.RandomState(0)
    big, small = np.arange(120000, dtype=np.float32).reshape(3, 40000), rng.rand(7).astype(np.float32)   # distinct values
    variables = [("big", big, 2 * big), ("small", small, -small)]
    pred = rng.rand(2, 5, 5).astype(np.float32)
    a = bench.dump_outputs(str(tmp_path / "a"), 0.25, pred, variables)
    b = bench.dump_outputs(str(tmp_path / "b"), 0.25, pred, variables)
    for name in ("loss", "predictions", "weights_sample", "momentum_sample"):
        on_disk = np.load(str(tmp_path / "a" / (name + ".npy")))
        assert on_disk.dtype in (np.float32, np.float64)
        np.testing.assert_array_equal(on_disk, a[name])
        np.testing.assert_array_equal(a[name], b[name])
    assert a["loss"].dtype == np.float64 and a["loss"][0] == 0.25
    np.testing.assert_array_equal(a["predictions"], pred)
    k = bench.DUMP_PER_VARIABLE
    w, m = a["weights_sample"], a["momentum_sample"]
    assert w.shape == (k + small.size,)
    assert np.isin(w[:k], big).all() and len(np.unique(w[:k])) == k   # distinct positions of the big variable
    np.testing.assert_array_equal(m[:k], 2 * w[:k])                    # the Momentum slots at the same positions
    np.testing.assert_array_equal(w[k:], small)                        # a small variable whole
    np.testing.assert_array_equal(m[k:], -small)

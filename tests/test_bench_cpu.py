"""bench.py contract smoke on CPU (the real numbers come from the GPU run;
this checks the JSON contract the driver depends on)."""
import json
import subprocess
import sys


def test_bench_json_contract_cpu():
    out = subprocess.run(
        [sys.executable, "bench.py", "--steps", "3", "--warmup", "1",
         "--device", "cpu", "--batch-size", "16"],
        capture_output=True, text=True, timeout=300, check=True)
    line = [l for l in out.stdout.strip().splitlines()
            if l.startswith("{")][-1]
    r = json.loads(line)
    for key in ["metric", "value", "unit", "n_gpus", "steps", "warmup",
                "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                "dtype", "data", "config"]:
        assert key in r, key
    assert r["scaling"] == "weak"
    assert r["data"] == "synthetic"
    assert r["n_gpus"] == 1
    assert r["value"] > 0
    assert r["config"]["parallelism"] == "dp1"
    assert r["config"]["timed_blocks"] == 1  # plain run: one K-step block


def test_bench_dump_outputs_and_full_cpu(tmp_path):
    """--dump-outputs writes the state after exactly warmup + steps steps
    (identical from run to run, with or without --full's extra blocks)."""
    import numpy as np
    dumps = []
    for name, extra in [("a", []), ("b", ["--full"])]:
        d = tmp_path / name
        out = subprocess.run(
            [sys.executable, "bench.py", "--steps", "2", "--warmup", "1",
             "--device", "cpu", "--batch-size", "16", "--dump-outputs",
             str(d)] + extra,
            capture_output=True, text=True, timeout=300, check=True)
        r = json.loads([l for l in out.stdout.strip().splitlines()
                        if l.startswith("{")][-1])
        assert r["steps"] == 2 and r["ms_per_step"] > 0
        if not extra:
            assert r["config"]["timed_blocks"] == 1
        dumps.append({f.stem: np.load(f) for f in sorted(d.glob("*.npy"))})
    a, b = dumps
    assert set(a) == {"params", "y", "loss_accum"}
    assert a["params"].shape == (2343,) and a["y"].shape == (16, 10)
    for k in a:
        assert a[k].dtype == np.float32
        assert np.isfinite(a[k]).all()
        assert np.array_equal(a[k], b[k]), k

"""bench.py's own contract, with the device set-up and the workload swapped for CPU stubs: a plain run times exactly --steps
steps and does nothing else after them; --full adds the decode, the child runs and the CPU baseline; --dump-outputs writes what
the last timed step returned."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

EXTRAS = ("at_tolerance", "other_configs", "training_step_record", "cpu_baseline")


def _bench(monkeypatch, capsys, *argv):
    import bench
    calls = {"run": [], "decode": 0}

    class Model:
        def decode_first_stage(self, z):
            calls["decode"] += 1
            return z * 2

    def make_workload(args, device, rank, dist):
        last = {}

        def run(n, x, start_index):
            calls["run"].append(n)
            for _ in range(n):
                time.sleep(0.02)
                x = x * 0.5 + 1
            if n:
                last.update(x_prev=x, pred_x0=x * 3)
            return x
        return {"run": run, "x0": torch.arange(24.0).reshape(2, 3, 4), "S": 50, "model": Model(), "inp": None, "hip": None,
                "outputs": lambda: dict(last)}

    monkeypatch.setattr(bench, "setup", lambda args, local: (torch.device("cpu"), "gloo"))
    monkeypatch.setattr(bench, "make_workload", make_workload)
    for name in EXTRAS:
        monkeypatch.setattr(bench, name, lambda *a, _n=name, **k: calls.setdefault(_n, {"value": 1.0}))
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MUDG_ATTN_FP8"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--operand", "bf16", *argv])
    bench.main()
    lines = [l for l in capsys.readouterr().out.splitlines() if l.strip()]
    assert len(lines) == 1
    return json.loads(lines[0]), calls


def test_plain_run_times_the_steps_and_nothing_else(monkeypatch, capsys):
    rec, calls = _bench(monkeypatch, capsys, "--gpus", "1", "--steps", "5", "--warmup", "2")
    assert calls["run"] == [2, 5] and calls["decode"] == 0
    assert not any(name in calls for name in EXTRAS)
    assert rec["steps"] == 5 and rec["warmup"] == 2 and rec["ms_per_step"] > 0
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in rec, key
    assert rec["unit"] == "steps/s" and rec["higher_is_better"] is True and rec["dtype"] == "bf16"
    assert abs(rec["value"] - 1000.0 / rec["ms_per_step"]) < 0.01 * rec["value"]


def test_full_run_keeps_the_extras(monkeypatch, capsys):
    rec, calls = _bench(monkeypatch, capsys, "--gpus", "1", "--steps", "3", "--warmup", "1", "--full")
    assert calls["run"] == [1, 3] and calls["decode"] == 2
    assert all(name in calls for name in EXTRAS)
    for key in ("at_tolerance", "other_configs", "training_step", "cpu_baseline", "clips_per_min", "vae_decode_ms_per_clip"):
        assert key in rec, key


def test_dump_outputs_writes_the_last_timed_step(monkeypatch, capsys, tmp_path):
    _bench(monkeypatch, capsys, "--gpus", "1", "--steps", "4", "--warmup", "1", "--dump-outputs", str(tmp_path))
    x = torch.arange(24.0).reshape(2, 3, 4)
    for _ in range(5):
        x = x * 0.5 + 1
    got = {name: np.load(tmp_path / (name + ".npy")) for name in ("x_prev", "pred_x0")}
    assert all(a.dtype == np.float32 and a.shape == (2, 3, 4) for a in got.values())
    np.testing.assert_array_equal(got["x_prev"], x.numpy())
    np.testing.assert_array_equal(got["pred_x0"], (x * 3).numpy())


def test_dump_outputs_samples_large_outputs_the_same_way_every_time(monkeypatch, tmp_path):
    import bench
    monkeypatch.setattr(bench, "DUMP_BYTES", 4000)
    arrays = {"a": torch.randn(3000), "b": torch.randn(10, 100)}
    bench.dump_outputs(str(tmp_path / "1"), arrays)
    bench.dump_outputs(str(tmp_path / "2"), arrays)
    sizes = 0
    for name in arrays:
        one, two = np.load(tmp_path / "1" / (name + ".npy")), np.load(tmp_path / "2" / (name + ".npy"))
        np.testing.assert_array_equal(one, two)
        assert np.isin(one, arrays[name].numpy()).all()
        sizes += one.nbytes
    assert 0 < sizes <= 4000

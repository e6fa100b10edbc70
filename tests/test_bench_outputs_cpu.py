"""CPU: what a plain `bench.py` run does beyond the headline (nothing without --full) and how --dump-outputs writes what the timed
path computed -- host logic only."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_plain_run_has_no_secondary_legs():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 3, False, None)
    assert not any(bench.leg(a, s) for s in (a.no_roofline, a.no_cpu_baseline, a.no_train_leg, a.no_bf16_leg, a.no_f32_mfma_leg))
    f = bench.parse(["--full", "--no-cpu-baseline"])
    assert bench.leg(f, f.no_roofline) and bench.leg(f, f.no_train_leg) and not bench.leg(f, f.no_cpu_baseline)


def test_parse_rejects_what_a_plain_run_cannot_do():
    with pytest.raises(SystemExit):
        bench.parse(["--dump-event-raw", "x.json"])            # the instrumented pass runs with --full only
    assert bench.parse(["--full", "--dump-event-raw", "x.json"]).dump_event_raw == "x.json"
    with pytest.raises(SystemExit):
        bench.parse(["--steps", "0"])


def test_dump_outputs_writes_every_array_in_float32_or_float64(tmp_path):
    arrays = {"theta": torch.arange(8, dtype=torch.float32).reshape(1, 8), "mask": np.ones((2, 3), dtype=np.int32),
              "loss_total": np.float64(0.125)}
    bench.dump_outputs(str(tmp_path), arrays)
    assert sorted(os.listdir(tmp_path)) == ["loss_total.npy", "mask.npy", "theta.npy"]
    theta, mask, loss = (np.load(tmp_path / n) for n in ("theta.npy", "mask.npy", "loss_total.npy"))
    assert theta.dtype == np.float32 and np.array_equal(theta, arrays["theta"].numpy())
    assert mask.dtype == np.float32 and np.array_equal(mask, np.ones((2, 3)))
    assert loss.dtype == np.float64 and loss == 0.125


def test_dump_outputs_samples_within_the_budget_the_same_way_every_time(tmp_path):
    rng = np.random.default_rng(3)
    arrays = {"small": rng.standard_normal(100).astype(np.float32), "big": rng.standard_normal(10000).astype(np.float32),
              "bigger": rng.standard_normal(20000)}
    budget = 4 * 100 + 4 * 3000 + 8 * 3000 + 3 * bench.NPY_HEADER_BYTES
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrays, budget=budget)
    got = {n: np.load(tmp_path / "a" / (n + ".npy")) for n in arrays}
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= budget      # files, headers included
    assert np.array_equal(got["small"], arrays["small"])                     # within its share: written whole
    assert 0 < got["big"].size < 10000 and np.isin(got["big"], arrays["big"]).all()
    assert got["bigger"].dtype == np.float64 and 0 < got["bigger"].size < 20000
    for n in arrays:                                                         # a fixed sample: identical from run to run
        assert np.array_equal(got[n], np.load(tmp_path / "b" / (n + ".npy")))

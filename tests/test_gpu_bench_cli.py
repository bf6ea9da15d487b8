"""bench.py as a command: a plain run times exactly --steps rounds and prints the headline line alone, and
--dump-outputs writes what the last timed round computed (one small FedAvg run, checked against the oracle over
the same synthetic inputs regenerated on the host)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle.cpu_reference import fedavg_flat

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_line_and_dumped_outputs(gpu_device, tmp_path):
    from fedscale_amd import synth

    K, P, seed = 7, 100_003, 11  # P odd and no multiple of 64; several blocks
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--clients", str(K), "--params", str(P), "--seed", str(seed), "--dump-outputs", str(out)],
                       cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert (line["steps"], line["warmup"], line["n_gpus"], line["dtype"]) == (3, 1, 1, "f32")
    assert line["unit"] == "client-updates/s" and line["higher_is_better"] is True and "FedAvg" in line["metric"]
    assert line["ms_per_step"] > 0 and line["value"] == pytest.approx(K / (line["ms_per_step"] * 1e-3))
    assert line["full"] is False
    for moved in ("sustained", "other_configs", "drop_in_one_gpu", "card_state", "pcie_inclusive", "schema"):
        assert moved not in line, moved
    assert line["cpu_baseline"] is None
    assert line["dumped_outputs"]["files"] == {"model.npy": [P, P]}
    assert sorted(os.listdir(out)) == ["model.npy"]
    got = np.load(out / "model.npy")
    assert got.dtype == np.float32 and got.shape == (P,)
    x = synth.host_columns(seed, range(K), np.arange(P))  # the inputs bench.Workload fills on the device
    np.testing.assert_array_equal(got, fedavg_flat(x))

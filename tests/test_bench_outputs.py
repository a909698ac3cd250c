"""bench.py's `--dump-outputs DIR`: what the last timed step hands its caller, written so that two builds run with the same
arguments can be compared file for file.  On the CPU the dump itself (seeded sample, master copies, dtypes); on the GPU a
small plain run end to end."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_takes_master_copies_and_a_seeded_sample(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "torch", torch)
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 64)
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(32, 16), torch.nn.BatchNorm1d(16))
    masters = {id(p): p.detach() * 2 for p in model[0].parameters()}      # the BatchNorm affine has no master copy

    class Optimizer:
        @staticmethod
        def master_of(p):
            return masters.get(id(p))

    class Trainer:
        optimizer = Optimizer()

    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), Trainer(), model, torch.tensor(1.5))
    for f in ("loss", "parameters", "buffers"):
        assert (tmp_path / "a" / f"{f}.npy").read_bytes() == (tmp_path / "b" / f"{f}.npy").read_bytes(), f
    loss = np.load(tmp_path / "a" / "loss.npy")
    assert loss.dtype == np.float64 and loss.tolist() == [1.5]
    par = np.load(tmp_path / "a" / "parameters.npy")
    assert par.dtype == np.float32 and par.shape == (64 + 16 + 16 + 16,)
    w = (model[0].weight.detach() * 2).numpy().reshape(-1)
    assert np.isin(par[:64], w).all() and len(np.unique(par[:64])) == 64        # 64 distinct positions of the master
    np.testing.assert_array_equal(par[64:80], (model[0].bias.detach() * 2).numpy())
    np.testing.assert_array_equal(par[80:96], model[1].weight.detach().numpy())
    buf = np.load(tmp_path / "a" / "buffers.npy")                              # running mean / var, not the step count
    assert buf.dtype == np.float32 and buf.shape == (32,)


@pytest.mark.gpu
def test_plain_run_dumps_the_last_timed_step(tmp_path):
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--global-batch", "32", "--bert-layers", "2", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    rec = json.loads(lines[0])
    assert rec["steps"] == 2 and rec["warmup"] == 1 and rec["ms_per_step"] > 0
    assert "cpu_baseline" not in rec and rec["config"]["kernel_launches_per_step"] is None     # --full only
    files = {f: np.load(out / f"{f}.npy") for f in ("loss", "parameters", "buffers")}
    assert files["loss"].dtype == np.float64 and files["loss"].tolist() == [rec["config"]["final_loss"]]
    assert files["parameters"].dtype == np.float32 and files["buffers"].dtype == np.float32
    assert all(np.isfinite(a).all() for a in files.values())
    assert sum(os.path.getsize(out / f"{f}.npy") for f in files) <= 64 << 20

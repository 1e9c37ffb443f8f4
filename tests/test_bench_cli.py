"""bench.py's command line on the CPU: a plain run does only what the headline figure needs; the CPU baselines (which
run before the GPU is touched) come only with --full.  The run stops at "needs a GPU" either way, so no device is used."""
import sys

import pytest
import torch

import bench


def _run(monkeypatch, *extra):
    called = []
    for name in ("cpu_baseline", "config3_cpu_sample", "config4_cpu_sample", "config5_cpu_sample"):
        monkeypatch.setattr(bench, name, lambda *a, _n=name, **k: called.append(_n))
    for var in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
        monkeypatch.delenv(var, raising=False)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "1", "--warmup", "0"] + list(extra))
    with pytest.raises(SystemExit, match="needs a GPU"):
        bench.main()
    return called


def test_plain_run_takes_no_cpu_samples(monkeypatch):
    assert _run(monkeypatch) == []


def test_full_run_takes_every_cpu_sample(monkeypatch):
    assert _run(monkeypatch, "--full") == ["cpu_baseline", "config3_cpu_sample", "config4_cpu_sample", "config5_cpu_sample"]
    assert _run(monkeypatch, "--full", "--no-config4") == ["cpu_baseline", "config3_cpu_sample", "config5_cpu_sample"]

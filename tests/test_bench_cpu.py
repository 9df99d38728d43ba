"""CPU tests of bench.py's host-side pieces: the --dump-outputs writer and the option checks that run before any GPU work."""
import os
import subprocess
import sys

import numpy as np
import torch
import torch.nn as nn

import bench


def _stepped_net():
    torch.manual_seed(3)
    net = nn.Sequential(nn.Linear(40, 50), nn.BatchNorm1d(50), nn.Linear(50, 3), nn.Linear(3, 3))
    loss = net[:3](torch.randn(8, 40)).square().mean()      # the last Linear gets no gradient
    loss.backward()
    return net, loss


def test_dump_outputs_writes_float32_samples(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 1000)
    net, loss = _stepped_net()
    for d in ("a", "b"):
        bench.dump_outputs(net, loss, str(tmp_path / d))
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["buffers_sample.npy", "grads_sample.npy", "loss.npy", "params_sample.npy"]
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype == np.float32 and np.array_equal(a, b), n          # same sample positions on every call
    assert np.load(tmp_path / "a" / "loss.npy")[0] == np.float32(loss.item())
    flat = torch.cat([p.detach().reshape(-1) for p in net.parameters()])
    grads = torch.cat([torch.zeros_like(p).reshape(-1) if p.grad is None else p.grad.reshape(-1) for p in net.parameters()])
    assert flat.numel() > 1000
    idx = torch.randint(flat.numel(), (1000,), generator=torch.Generator().manual_seed(0)).unique()
    assert np.array_equal(np.load(tmp_path / "a" / "params_sample.npy"), flat[idx].numpy())
    assert np.array_equal(np.load(tmp_path / "a" / "grads_sample.npy"), grads[idx].numpy())
    bufs = torch.cat([net[1].running_mean, net[1].running_var])           # shorter than the sample: kept whole
    assert np.array_equal(np.load(tmp_path / "a" / "buffers_sample.npy"), bufs.numpy())


def test_dump_outputs_stays_below_64_mb():
    assert 3 * bench.DUMP_SAMPLE * 4 + 4 < 64 * 10**6


def test_gemm_log_needs_full():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gemm-log", "launches.csv"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "--full" in r.stderr

"""bench.py's --dump-outputs writer on CPU: float arrays only, a fixed sample of the parameters whatever the run, and
the same files for the same state."""
import numpy as np
import torch

import bench


def _net_after_one_step(seed=0):
    torch.manual_seed(seed)
    net = torch.nn.Sequential(torch.nn.Linear(8, 16), torch.nn.BatchNorm1d(16), torch.nn.Linear(16, 2)).train()
    out = net(torch.randn(4, 8))
    out.sum().backward()
    return net, [out[:, :1], out[:, 1:]]


def test_dump_outputs_writes_float_arrays_reproducibly(tmp_path):
    last = {"loss": 1.5, "f0": 2.0, "sil": 0.25}
    files = {}
    for run in ("a", "b"):
        net, preds = _net_after_one_step()
        nbytes = bench.dump_outputs(tmp_path / run, net, preds, last)
        files[run] = {p.name: np.load(p) for p in sorted((tmp_path / run).glob("*.npy"))}
        assert nbytes == sum(a.nbytes for a in files[run].values()) <= 64 << 20
    a, b = files["a"], files["b"]
    assert set(a) == {"loss.npy", "f0_pred.npy", "sil_pred.npy", "params_sample.npy", "grads_sample.npy",
                      "bn_buffers.npy"}
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert a["loss.npy"].dtype == np.float64 and a["loss.npy"].tolist() == [1.5, 2.0, 0.25]
    assert all(np.array_equal(a[k], b[k]) for k in a)
    n_params = sum(p.numel() for p in net.parameters())
    assert a["params_sample.npy"].shape == (min(n_params, bench.DUMP_SAMPLE),)
    flat = torch.cat([p.detach().reshape(-1) for p in net.parameters()]).numpy()
    assert np.array_equal(np.sort(a["params_sample.npy"]), np.sort(flat))     # small net: the sample is all of it
    assert np.abs(a["grads_sample.npy"]).sum() > 0
    assert a["bn_buffers.npy"].shape == (32,)                                  # running mean + var of 16 channels


def test_dump_outputs_sample_is_bounded_and_fixed(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 10)
    net, preds = _net_after_one_step()
    last = {"loss": 0.0, "f0": 0.0, "sil": 0.0}
    bench.dump_outputs(tmp_path / "a", net, preds, last)
    bench.dump_outputs(tmp_path / "b", net, preds, last)
    a, b = (np.load(tmp_path / d / "params_sample.npy") for d in ("a", "b"))
    assert a.shape == (10,) and np.array_equal(a, b)

"""The ragged multi-rate resampler: one launch over rows at many source rates equals ``Resampler`` on each row alone,
bit for bit, and stays within the float64 oracle's tolerance."""
import math

import numpy as np
import pytest
import torch

from oracle import resample_ref as rr
from pitchextractor_amd.resample import RaggedResampler, Resampler

pytestmark = pytest.mark.gpu

RATES = (8000, 11025, 16000, 22050, 24000, 32000, 44100, 48000, 96000)


def _width(rate, target):
    if rate == target:
        return 1
    g = math.gcd(rate, target)
    orig, new = rate // g, target // g
    return math.ceil(6 * orig / (min(orig, new) * 0.99))


def _rows(target, rng):
    rates, lengths = [], []
    for r in RATES:
        g = math.gcd(r, target)
        w = _width(r, target)
        for n in (1, max(1, w - 1), w, r // g, 9001, int(rng.integers(1, 4 * r))):
            rates.append(r)
            lengths.append(n)
    perm = rng.permutation(len(rates))
    return [rates[k] for k in perm], [lengths[k] for k in perm]


def _check_rows(y, out_len, rates, lengths, xs, target, dev, oracle=True):
    assert y.shape[1] >= max(out_len)
    for r, (rate, n) in enumerate(zip(rates, lengths)):
        m = int(out_len[r])
        assert m == (n if rate == target else Resampler(rate, target).out_len(n))
        alone = Resampler(rate, target)(torch.from_numpy(xs[r]).to(dev))
        assert torch.equal(y[r, :m], alone), (r, rate, n)
        assert (y[r, m:] == 0).all(), (r, rate, n)
        if rate == target:
            assert np.array_equal(y[r, :m].cpu().numpy(), xs[r])
        if oracle:
            ref = rr.resample(xs[r], rate, target)
            got = y[r, :m].cpu().numpy().astype(np.float64)
            assert got.shape == ref.shape
            assert np.abs(got - ref).max() <= 2e-6 * max(1.0, np.abs(ref).max()), (r, rate, n)


@pytest.mark.parametrize("target", [24000, 16000])
def test_one_launch_equals_each_row_alone(hip_device, target):
    rng = np.random.default_rng(target)
    rates, lengths = _rows(target, rng)
    xs = [(0.3 * rng.standard_normal(n)).astype(np.float32) for n in lengths]
    rs = RaggedResampler(target)
    # packed rows
    packed = torch.from_numpy(np.concatenate(xs)).to(hip_device)
    y, out_len = rs(packed, rates, lengths)
    out_len = out_len.cpu().numpy()
    assert out_len.dtype == np.int32
    _check_rows(y, out_len, rates, lengths, xs, target, hip_device)
    # padded rows into a wider (uninitialised) output buffer: the tail up to y_width is written as zeros
    padded = np.zeros((len(xs), max(lengths) + 3), np.float32)
    for r, x in enumerate(xs):
        padded[r, :len(x)] = x
    y2, out_len2 = rs(torch.from_numpy(padded).to(hip_device), rates, lengths, y_width=y.shape[1] + 300)
    assert y2.shape == (len(xs), y.shape[1] + 300)
    assert torch.equal(y2[:, :y.shape[1]], y) and (y2[:, y.shape[1]:] == 0).all()
    assert np.array_equal(out_len2.cpu().numpy(), out_len)


def test_full_size_mixed_batch(hip_device):
    """256 rows of 4 s over {16k, 24k, 44.1k, 48k}: tiled replicas agree bit for bit, the launch is linear in the
    input, and three rows match the float64 oracle."""
    rng = np.random.default_rng(7)
    mix = (16000, 24000, 44100, 48000)
    base_rates = [mix[k % 4] for k in range(64)]
    n_max = 4 * 48000
    base = np.zeros((64, n_max), np.float32)
    lengths = []
    for r, rate in enumerate(base_rates):
        n = 4 * rate - int(rng.integers(0, 2000))
        base[r, :n] = 0.3 * rng.standard_normal(n)
        lengths.append(n)
    x = torch.from_numpy(np.tile(base, (4, 1))).to(hip_device)
    rates, lens = base_rates * 4, lengths * 4
    rs = RaggedResampler(24000)
    y, out_len = rs(x, rates, lens)
    assert y.shape[0] == 256
    for k in range(1, 4):
        assert torch.equal(y[64 * k:64 * (k + 1)], y[:64])
    y2, _ = rs(2 * x, rates, lens)
    assert torch.equal(y2, 2 * y)
    out_len = out_len.cpu().numpy()
    for r in (0, 2, 3):                                   # 16 kHz, 44.1 kHz and 48 kHz rows
        ref = rr.resample(base[r, :lengths[r]], base_rates[r], 24000)
        got = y[r, :out_len[r]].cpu().numpy().astype(np.float64)
        assert np.abs(got - ref).max() <= 2e-6 * max(1.0, np.abs(ref).max()), r


def test_host_checks_refuse_before_launch(hip_device):
    rs = RaggedResampler(24000)
    x = torch.zeros(2, 100, device=hip_device)
    with pytest.raises(RuntimeError, match="invalid argument"):
        rs(x, [44100, 16000], [100, 100], y_width=100)     # 16 kHz row: 150 outputs do not fit
    with pytest.raises(ValueError):
        rs(x, [44100, 16000], [101, 100])


def test_rows_without_samples_need_no_launch(hip_device):
    """An empty input goes through whatever its stride is (``torch.from_numpy`` of an empty array has stride 0), as it
    does for the trackers and the stress conditions: no row has an output, nothing is launched."""
    rs = RaggedResampler(24000)
    for x, lengths in ((torch.from_numpy(np.zeros(0, np.float32)).to(hip_device), [0, 0]),
                       (torch.zeros((2, 0), device=hip_device), None)):
        y, out_lengths = rs(x, [16000, 24000], lengths)
        assert tuple(y.shape) == (2, 0) and out_lengths.cpu().tolist() == [0, 0]

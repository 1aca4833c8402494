"""The synthetic-kind seam on the GPU: a fourth, test-only kind registered from outside goes through ``Collater``,
``H2DPrefetcher`` and ``DeviceMelLoader._finish`` like the built-in ones.  No kernel of its own: its stage fills each
of its rows' windows with a constant."""
from typing import NamedTuple

import numpy as np
import pytest
import torch

from pitchextractor_amd import meldataset as md
from pitchextractor_amd import synthetic_items

pytestmark = pytest.mark.gpu

SR, HOP = 24000, 300


class FillRequest(NamedTuple):
    value: float
    out_len: int


class FillBatch(NamedTuple):
    rows: torch.Tensor
    out_len: torch.Tensor
    values: torch.Tensor


class Fill:
    name, Request, Batch = "fill", FillRequest, FillBatch

    def collate(self, batch, rows, row_rates, mixed):
        reqs = [batch[i][-1] for i in rows]
        return FillBatch(torch.tensor(rows, dtype=torch.int64), torch.tensor([r.out_len for r in reqs]),
                         torch.tensor([r.value for r in reqs], dtype=torch.float32))

    def run(self, loader, waves, lengths, dev_batch, host_batch, src_sr):
        assert dev_batch.rows.is_cuda and not host_batch.rows.is_cuda and waves.is_contiguous()
        assert waves.shape[1] >= int(host_batch.out_len.max()) and src_sr == SR
        for row, n, value in zip(host_batch.rows.tolist(), host_batch.out_len.tolist(), host_batch.values.tolist()):
            waves[row, :n] = value
        return waves, lengths


def _plain(index, n):
    wave = torch.from_numpy(np.random.default_rng(index).uniform(-0.5, 0.5, n).astype(np.float32))
    frames = 1 + n // HOP
    return wave, torch.full((frames,), 100.0 + index), torch.zeros(frames), 0, SR


def _filled(value, n):
    frames = 1 + n // HOP
    return torch.zeros(0), torch.full((frames,), 200.0), torch.zeros(frames), 0, SR, FillRequest(value, n)


def _through_the_loader(loader, host):
    mels, f0s, sils = loader._finish(loader._submit(host))
    torch.cuda.synchronize()
    assert not loader._host
    return mels, f0s, sils


@pytest.mark.parametrize("out_lens,width", [((6000, 9000), None), ((6000, 15000), 12000)],
                         ids=["inside-the-plain-rows", "wider-than-waves"])
def test_a_kind_registered_from_outside_runs_as_a_loader_stage(monkeypatch, hip_device, out_lens, width):
    """4 rows at 24 kHz: two plain 0.5 s rows and two rows of the test's kind.  ``width``: the collated ``waves`` cut to
    that many columns (every plain row still whole), as a whole-batch resample to a lower rate leaves them, so that the
    stage has to widen them for its longest window."""
    monkeypatch.setattr(synthetic_items, "KINDS", synthetic_items.KINDS + [Fill()])

    class _Host:
        dataset = None

    loader = md.DeviceMelLoader(_Host(), md.MelSpectrogram(**md.DEFAULT_MEL_PARAMS), hip_device)
    plain = [_plain(0, 12000), _plain(1, 12000)]
    values = (0.25, -0.5)
    batch = [plain[0], _filled(values[0], out_lens[0]), plain[1], _filled(values[1], out_lens[1])]
    host = md.Collater()(batch)
    assert len(host) == 7 and type(host[6]) is FillBatch and host[6].rows.tolist() == [1, 3]
    assert host[1].tolist() == [12000, out_lens[0], 12000, out_lens[1]] and (host[0][[1, 3]] == 0).all()
    if width is not None:
        assert host[0].shape[1] == max(out_lens) > width
        host = (host[0][:, :width].contiguous(),) + host[1:]
    mels, f0s, sils = _through_the_loader(loader, host)
    assert tuple(mels.shape) == (4, 1, 80, 192) and torch.isfinite(mels).all()

    # the kind's rows: the log-mel of the same constant windows
    windows = torch.zeros((2, max(out_lens)), device=hip_device)
    for k, (value, n) in enumerate(zip(values, out_lens)):
        windows[k, :n] = value
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=hip_device)  # noqa: E731
    want = loader.mel.log_mel_ragged(windows, i32(list(out_lens)), i32([0, 0]), max_frames=192)
    assert torch.equal(mels[[1, 3]], want)
    assert not torch.equal(mels[1], mels[3])
    # the plain rows: as in the batch without the kind's rows
    alone = _through_the_loader(loader, md.Collater()(plain))
    assert torch.equal(mels[[0, 2]], alone[0])
    assert torch.equal(f0s[[0, 2]], alone[1]) and torch.equal(sils[[0, 2]], alone[2])
    assert (f0s[1, :1 + out_lens[0] // HOP] == 200.0).all() and (f0s[1, 1 + out_lens[0] // HOP:] == 0).all()

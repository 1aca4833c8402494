"""The synthetic-kind registry without a GPU: the collated layout over every registered kind, and the ``Request`` /
``Batch`` types across pickle (worker processes) and field-by-field reconstruction (``pin_memory``)."""
import pickle
import random

import numpy as np
import pytest
import torch

from pitchextractor_amd import meldataset as md
from pitchextractor_amd import synthetic_items
from tests.test_cheaptrick_cpu import PS_CFG, RS_CFG, WORLD_CFG, _ds, _files


def _same(a, b):
    assert type(a) is type(b)
    if isinstance(a, tuple):
        assert len(a) == len(b)
        for u, v in zip(a, b):
            _same(u, v)
    elif torch.is_tensor(a) or isinstance(a, np.ndarray):
        assert a.dtype == b.dtype
        np.testing.assert_array_equal(np.asarray(a), np.asarray(b))
    else:
        assert a == b


@pytest.fixture(scope="module")
def mixed_batch(tmp_path_factory):
    """[plain item, cached-mel item, the first drawn item of every registered kind in draw order] + the dataset."""
    lines = _files(tmp_path_factory.mktemp("kinds"), [2.0, 1.0])
    ds = _ds(lines, {"enabled": True, "absolute_count": 16, "pitch_shift": {**PS_CFG, "noise_db": -50.0},
                     "world_vocoder": WORLD_CFG, "world_resynthesis": RS_CFG})
    assert ds._synthetic_generators == [kind.name for kind in synthetic_items.KINDS]
    random.seed(11); np.random.seed(11)
    first = {}
    for i in range(16):
        item = ds[2 + i]
        first.setdefault(type(item[-1]), item)
    assert set(first) == {kind.Request for kind in synthetic_items.KINDS}
    plain = ds[0]
    assert len(plain) == 5
    mel = torch.from_numpy(np.random.default_rng(0).standard_normal((80, 150)).astype(np.float32))
    return [plain, ds[1] + (mel,)] + list(first.values()), ds


def test_registry_names_and_types():
    assert [kind.name for kind in synthetic_items.KINDS] == ["pitch_shift", "world_vocoder", "world_resynthesis"]
    assert md._SYNTHETIC_BATCHES == (md.PitchShiftBatch, md.WorldBatch, md.ResynthesisBatch)
    assert [kind.Request for kind in synthetic_items.KINDS] == [md.PitchShiftRequest, md.WorldRequest,
                                                                md.ResynthesisRequest]
    assert [kind.Batch for kind in synthetic_items.KINDS] == list(md._SYNTHETIC_BATCHES)
    assert md.synthetic_window is synthetic_items.synthetic_window


def test_collated_layout_over_every_kind(mixed_batch):
    batch, ds = mixed_batch
    out = md.Collater()(batch)
    kinds = synthetic_items.KINDS
    assert len(out) == 6 + 2 + len(kinds)
    waves, lengths, crops, f0s, sils, source_sr = out[:6]
    assert waves.shape[0] == lengths.shape[0] == crops.shape[0] == len(batch) and source_sr == 24000
    assert f0s.shape == sils.shape == (len(batch), 192)
    cached_rows, cached_mels = out[6:8]
    assert cached_rows.tolist() == [1] and cached_mels.shape == (1, 80, 192)
    assert torch.equal(cached_mels[0, :, :150], batch[1][5]) and (cached_mels[0, :, 150:] == 0).all()
    n_max = 0
    for kind, pack in zip(kinds, out[8:]):                       # one batch per kind, in registry order
        assert type(pack) is kind.Batch
        rows = [i for i, item in enumerate(batch) if isinstance(item[-1], kind.Request)]
        assert rows and pack.rows.tolist() == rows and pack.rows.dtype == torch.int64
        assert pack.out_len.tolist() == [batch[i][-1].out_len for i in rows]
        for i in rows:
            assert int(lengths[i]) == batch[i][-1].out_len and int(crops[i]) == batch[i][-1].frame_start
            assert (waves[i] == 0).all()
            n_max = max(n_max, batch[i][-1].out_len)
    for i in (0, 1):
        n = batch[i][0].shape[0]
        assert int(lengths[i]) == n and torch.equal(waves[i, :n], batch[i][0])
        n_max = max(n_max, n)
    assert waves.shape[1] == n_max
    # a kind without rows leaves no batch behind, the others keep their order
    no_vocoder = [item for item in batch if not isinstance(item[-1], md.WorldRequest)]
    assert [type(t) for t in md.Collater()(no_vocoder)[8:]] == [md.PitchShiftBatch, md.ResynthesisBatch]
    # the field types that differ between the kinds
    ps, wd, rs = out[8:]
    assert torch.is_tensor(ps.out_start) and ps.src_sr is None
    assert isinstance(wd.out_start, np.ndarray) and isinstance(rs.out_start, np.ndarray)
    assert rs.src_sr.dtype == torch.int32 and rs.src_sr.tolist() == [24000]


def test_plain_items_collate_to_the_bare_six_tuple(mixed_batch):
    batch, ds = mixed_batch
    out = md.Collater()([batch[0], ds[1]])
    assert len(out) == 6 and all(torch.is_tensor(t) for t in out[:5]) and out[5] == 24000


def test_requests_and_batches_survive_pickle_and_pin_memory_reconstruction(mixed_batch):
    batch, _ = mixed_batch
    out = md.Collater()(batch)
    for kind in synthetic_items.KINDS:
        req = next(item[-1] for item in batch if isinstance(item[-1], kind.Request))
        pack = next(t for t in out[6:] if isinstance(t, kind.Batch))
        for t in (req, pack):
            assert hasattr(t, "_fields") and type(t).__module__ == synthetic_items.__name__
            assert getattr(md, type(t).__name__) is type(t)              # importable as meldataset.<name>
            _same(pickle.loads(pickle.dumps(t)), t)
            _same(type(t)(*t), t)                                        # what pin_memory does to a namedtuple
    _same(pickle.loads(pickle.dumps(tuple(batch[2:]))), tuple(batch[2:]))    # whole items, as a worker sends them

"""``ragged.row_layout`` / ``packed_offsets``: packed 1-D or padded 2-D rows as lengths and offsets (no GPU; the helper
reads shapes and strides only, so CPU tensors serve)."""
import numpy as np
import pytest
import torch

from pitchextractor_amd.ragged import packed_offsets, row_layout


def _rows(x, lengths, offsets):
    flat = x.as_strided((x.untyped_storage().nbytes() // x.element_size(),), (1,), 0)
    return [flat[x.storage_offset() + o:x.storage_offset() + o + n] for n, o in zip(lengths, offsets)]


def test_packed_rows_with_and_without_slack():
    x = torch.arange(12, dtype=torch.float32)
    assert row_layout(x, [5, 4, 3]) == ([5, 4, 3], [0, 5, 9])                 # fills the tensor exactly
    lengths, offsets = row_layout(x, (5, 4))                                  # three samples of trailing slack
    assert (lengths, offsets) == ([5, 4], [0, 5])
    assert all(type(v) is int for v in lengths + offsets)
    assert [r.tolist() for r in _rows(x, lengths, offsets)] == [[0, 1, 2, 3, 4], [5, 6, 7, 8]]
    assert row_layout(x, np.array([12], np.int32)) == ([12], [0])


def test_packed_rows_missing_lengths():
    x = torch.zeros(7)
    with pytest.raises(ValueError, match="need their lengths"):
        row_layout(x)
    assert row_layout(x, whole_by_default=True) == ([7], [0])                 # one row of the whole tensor
    assert row_layout(x, [3, 2], whole_by_default=True) == ([3, 2], [0, 3])   # the flag changes nothing else


def test_padded_rows_follow_the_row_stride():
    base = torch.arange(4 * 10, dtype=torch.float32).reshape(4, 10)
    x = base[:, :6]                                                           # width 6, row stride 10
    assert x.stride() == (10, 1) and not x.is_contiguous()
    assert row_layout(x) == ([6, 6, 6, 6], [0, 10, 20, 30])                   # lengths default to the width
    lengths, offsets = row_layout(x, [6, 0, 2, 5])
    assert (lengths, offsets) == ([6, 0, 2, 5], [0, 10, 20, 30])
    assert [r.tolist() for r in _rows(x, lengths, offsets)] == [x[r, :n].tolist() for r, n in enumerate(lengths)]
    y = base[1::2, 2:7]                                                       # every other row, offset view
    lengths, offsets = row_layout(y, [5, 1])
    assert offsets == [0, 20]
    assert [r.tolist() for r in _rows(y, lengths, offsets)] == [y[0].tolist(), y[1, :1].tolist()]


def test_empty_batch():
    assert row_layout(torch.zeros(0), []) == ([], [])
    assert row_layout(torch.zeros(9), []) == ([], [])
    assert row_layout(torch.zeros((0, 16))) == ([], [])
    assert row_layout(torch.zeros((0, 16)), []) == ([], [])
    assert row_layout(torch.zeros(0), whole_by_default=True) == ([0], [0])
    off = packed_offsets([])
    assert off.dtype == np.int64 and off.shape == (0,)


def test_zero_length_row_in_the_middle():
    x = torch.zeros(10)
    assert row_layout(x, [4, 0, 6]) == ([4, 0, 6], [0, 4, 4])
    assert row_layout(x, [0, 0, 3, 0]) == ([0, 0, 3, 0], [0, 0, 0, 3])
    off = packed_offsets(np.array([4, 0, 6], np.int32))
    assert off.dtype == np.int64 and off.tolist() == [0, 4, 4]
    big = packed_offsets([2 ** 31, 2 ** 31, 1])                               # no int32 arithmetic on the way
    assert big.tolist() == [0, 2 ** 31, 2 ** 32]


def test_refusals():
    padded = torch.zeros((3, 8))
    with pytest.raises(ValueError, match="padded width"):
        row_layout(padded, [8, 9, 1])
    with pytest.raises(ValueError, match="negative"):
        row_layout(padded, [8, -1, 1])
    with pytest.raises(ValueError, match="3 padded rows"):
        row_layout(padded, [8, 8])
    packed = torch.zeros(10)
    with pytest.raises(ValueError, match="exceed the input"):
        row_layout(packed, [6, 5])
    with pytest.raises(ValueError, match="negative"):
        row_layout(packed, [6, -1])
    with pytest.raises(ValueError, match="negative"):
        row_layout(packed, [12, -2])                                          # the sum fits, one row does not
    with pytest.raises(ValueError, match="need their lengths"):
        row_layout(packed, None)
    with pytest.raises(ValueError, match="1-D packed or a 2-D padded"):
        row_layout(torch.zeros((2, 3, 4)), [1, 1])
    assert row_layout(packed, [10]) == ([10], [0])                            # the bounds themselves are allowed
    assert row_layout(padded, [8, 8, 8])[0] == [8, 8, 8]


def test_host_audio_is_refused_in_the_callers_name():
    from pitchextractor_amd.ragged import check_waves
    from pitchextractor_amd.resample import RaggedResampler
    for bad in (torch.zeros(8), np.zeros(8, np.float32), None):
        with pytest.raises(RuntimeError, match=r"^RaggedResampler \(HIP\) needs contiguous-row float32 device audio; no CPU"):
            RaggedResampler(24000)(bad, [16000], [8])
        with pytest.raises(RuntimeError, match=r"^somebody \(HIP\) needs .* no CPU fallback exists$"):
            check_waves(bad, "somebody")


def test_the_helpers_noise_stimuli_and_rir_share(monkeypatch):
    """What moved here from noise.py, stimuli.py and rir.py refuses what it refused there, with the same types."""
    from pitchextractor_amd import noise, ragged, rir, stimuli
    assert noise.STAT_KEYS is stimuli.STAT_KEYS and noise.to_device is ragged.to_device is stimuli.to_device
    for module in (noise, stimuli, rir):
        for name in ("_device", "_check_device", "_extent", "_output"):
            assert not hasattr(module, name), (module.__name__, name)
    # not a GPU device; a CPU tensor, a wrong dtype, no tensor at all
    assert ragged.gpu_device("cuda:1", "noise") == torch.device("cuda:1")
    with pytest.raises(RuntimeError, match=r"^rir \(HIP\) needs a GPU device, got cpu; no CPU fallback exists$"):
        ragged.gpu_device("cpu", "rir")
    for bad in (torch.zeros(8), torch.zeros(8, dtype=torch.float64), np.zeros(8, np.float32), None):
        with pytest.raises(RuntimeError, match=r"^noise.white \(HIP\) needs a contiguous float32 device tensor; no CPU"):
            ragged.check_device_tensor(bad, "noise.white")
    with pytest.raises(RuntimeError, match="contiguous float64 device tensor"):
        ragged.check_device_tensor(torch.zeros(8), "stimuli.synth", torch.float64)
    pl = dict(rows=2, offsets=np.array([3, 0]), lengths=np.array([5, 2]))
    assert ragged.plan_extent(pl) == 8 and ragged.plan_extent(dict(rows=0, offsets=np.zeros(0), lengths=np.zeros(0))) == 0
    with pytest.raises(RuntimeError, match=r"^noise.bed \(HIP\) needs a contiguous float32 device tensor"):
        ragged.plan_output(pl, torch.zeros(8), "cuda", "noise.bed")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        noise.white([4], out=torch.zeros(4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rir.synthesize([], 24000, out=torch.zeros(4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        stimuli.finish(dict(rows=0), torch.zeros(4))
    with pytest.raises(RuntimeError, match=r"^stimuli.tone \(HIP\) needs a contiguous float32 device tensor"):
        stimuli.tone(dict(rows=0), None)
    # a short output: the device check is stood in for, the length check is the one under test
    monkeypatch.setattr(ragged, "check_device_tensor", lambda t, who, dtype=torch.float32: None)
    with pytest.raises(ValueError, match=r"^noise.bed: the output is shorter than the plan's rows$"):
        ragged.plan_output(pl, torch.zeros(7), None, "noise.bed")
    with pytest.raises(ValueError, match=r"^rir.synthesize: the output is shorter than the rooms' responses$"):
        ragged.plan_output(pl, torch.zeros(7), None, "rir.synthesize", "the output is shorter than the rooms' responses")
    out = torch.zeros(8)
    assert ragged.plan_output(pl, out, None, "noise.bed") is out
    # one value per row
    assert ragged.per_row(3, 4, "x").tolist() == [3, 3, 3, 3] and ragged.per_row(3, 4, "x").dtype == np.int64
    assert ragged.per_row([1.5, 2.5], 2, "x", np.float64).tolist() == [1.5, 2.5]
    assert ragged.per_row(7, 0, "x").size == 0 and ragged.per_row([], 0, "x").size == 0
    for bad in ([1, 2, 3], [], [[1, 2], [3, 4]]):
        with pytest.raises(ValueError, match="^one per row$"):
            ragged.per_row(bad, 2, "one per row")
    with pytest.raises(ValueError, match="one warm-up and one white offset per row"):
        noise.plan_rows([4, 4], warmup=[1, 2, 3])
    with pytest.raises(ValueError, match="one warm-up and one white offset per row"):
        noise.plan_rows([4, 4], white_offsets=[0])
    # recordings as one packed batch, behind both public classes
    from pitchextractor_amd import stress
    beds, rirs = noise.NoiseSet([[1.0, 2.0], [3.0]], "cuda"), stress.RirSet([[1.0, 2.0], [3.0]])
    assert isinstance(beds, ragged.PackedRecordings) and isinstance(rirs, ragged.PackedRecordings)
    assert beds.key == rirs.key and beds.lengths == rirs.lengths == [2, 1] and beds.offsets == rirs.offsets == [0, 2]
    assert beds.packed.dtype == np.float32 and beds.packed.tolist() == [1.0, 2.0, 3.0] and len(beds) == len(rirs) == 2
    assert beds.recordings[1].tolist() == rirs.rirs[1].tolist() == [3.0] and rirs.plan["rows"] == 2
    with pytest.raises(ValueError, match="^NoiseSet: at least one recording, each of at least one sample$"):
        noise.NoiseSet([[1.0], []])
    with pytest.raises(ValueError, match="^RirSet: at least one impulse response, each of at least one sample$"):
        stress.RirSet([])
    packed, offsets, lengths = ragged.pack_tracks([np.array([1.0, 2.0]), torch.tensor([[3.0]]), []], "cpu")
    assert packed.tolist() == [1.0, 2.0, 3.0, 0.0] and offsets == [0, 2, 3] and lengths == [2, 1, 0]
    assert ragged.pack_tracks([], "cpu")[0].tolist() == [0.0]

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

"""``ops.Scaled``, a tensor with its "h2" scale word, on host tensors: what travels with a view, what a slice is, how
an operand without a word is read, and who keeps the word alive.  (The words' values are GPU tests:
tests/test_split_products_gpu.py::test_h2_amax_words_in_a_training_step.)"""
import gc
import struct
import weakref

import pytest
import torch

from pitchextractor_amd import ops


def _word(bits=0x40400000):
    return torch.tensor([bits], dtype=torch.int32)


@pytest.fixture
def passes(monkeypatch):
    """Stand-alone absmax passes asked for, with a host stand-in for the kernel."""
    calls = []

    def absmax(t, out=None):
        calls.append(t)
        return t.abs().max().view(1).view(torch.int32)

    monkeypatch.setattr(ops, "absmax", absmax)
    monkeypatch.setattr(ops, "MATMUL_BF16", False)
    return calls


def test_a_view_keeps_the_word():
    t, w = torch.arange(24, dtype=torch.float32).view(2, 3, 4), _word()
    s = ops.Scaled(t, w)
    flat = s.view(-1, s.shape[-1])
    assert isinstance(flat, ops.Scaled) and flat.amax is w
    assert flat.shape == (6, 4) and flat.t.data_ptr() == t.data_ptr()
    assert s.view(6, 4).view(2, 12).amax is w


def test_a_slice_is_a_plain_tensor():
    t = torch.arange(24, dtype=torch.float32).view(2, 3, 4)
    s = ops.Scaled(t, _word())
    for part, want in ((s[0], t[0]), (s[:, :, 1:3], t[:, :, 1:3]), (s[1, 2], t[1, 2])):
        assert type(part) is torch.Tensor and torch.equal(part, want)
        assert ops._tw(part) == (part, None)


def test_no_word_and_a_plain_tensor_are_alike(passes, monkeypatch):
    t, w = torch.tensor([0.5, -3.0, 2.0]), _word()
    assert ops._tw(t) == (t, None) and ops._tw(ops.Scaled(t)) == (t, None) and ops._tw(ops.Scaled(t, w)) == (t, w)
    monkeypatch.setattr(ops, "FP32_MATMUL", "h2")
    for operand in (t, ops.Scaled(t)):                       # each is measured, once
        passes.clear()
        m = ops.Scaled.measured(operand)
        assert len(passes) == 1 and passes[0] is t and m.t is t
        assert m.amax.item() == struct.unpack("<i", struct.pack("<f", 3.0))[0]
    passes.clear()
    kept = ops.Scaled.measured(ops.Scaled(t, w))             # a word handed over is the word used
    assert kept.amax is w and kept.t is t and not passes
    for mode in ("x3", "native"):                            # outside h2 nobody reads a word: none is made
        monkeypatch.setattr(ops, "FP32_MATMUL", mode)
        assert ops.Scaled.measured(t).amax is None and ops.Scaled.bounded(t, 1.25).amax is None and not passes
        assert ops.amax_word() is None


def test_a_bound_is_a_constant_word(passes, monkeypatch):
    monkeypatch.setattr(ops, "FP32_MATMUL", "h2")
    t = torch.tensor([0.5, -1.0])
    b = ops.Scaled.bounded(t, 1.25)
    assert b.t is t and b.amax.dtype == torch.int32 and b.amax.numel() == 1 and not passes
    assert b.amax.item() == struct.unpack("<i", struct.pack("<f", 1.25))[0]
    assert ops.Scaled.bounded(torch.zeros(3), 1.25).amax is b.amax


def test_the_pairing_keeps_the_word_alive():
    t, w = torch.ones(4), _word()
    alive = weakref.ref(w)
    s = ops.Scaled(t, w)
    v = s.view(2, 2)
    del w
    gc.collect()
    assert alive() is not None and s.amax is alive()
    del s
    gc.collect()
    assert alive() is not None and v.amax is alive()         # a view holds it as well
    del v
    gc.collect()
    assert alive() is None


def test_a_packed_weight_keeps_its_weights_word():
    t, w = torch.ones(8, 16), _word()
    pw = ops.PackedWeight(ops.Scaled(t, w))
    assert pw.fp32 is t and pw.amax is w and pw.shape == t.shape
    plain = ops.PackedWeight(t)
    assert plain.fp32 is t and plain.amax is None and plain.frag is None

"""Mixed source rates in one batch, host side (no GPU): the Collater's per-row rates and the argument checks of the
ragged multi-rate resampler's C entry points."""
import ctypes

import numpy as np
import pytest
import torch

from pitchextractor_amd import _lib, build
from pitchextractor_amd import meldataset as md
from tests.test_data_layer import write_wav

RATES = (16000, 24000, 44100, 48000)


def _items(tmp_path, rates=RATES, seconds=(1.3, 4.0, 0.7, 2.9)):
    lines = []
    for i, (sr, dur) in enumerate(zip(rates, seconds)):
        n = int(dur * sr)
        wave = (0.3 * np.sin(2 * np.pi * (150 + 20 * i) * np.arange(n) / sr)).astype(np.float32)
        p = tmp_path / f"m{i}.wav"
        write_wav(p, wave, sr, "float32")
        np.save(str(p) + "_f0.npy", np.full(1 + int(dur * 24000) // 300, 150.0 + 20 * i, np.float32))
        lines.append(f"{p}|0\n")
    ds = md.MelDataset(lines, verbose=False)
    np.random.seed(3)
    return [ds[i] for i in range(len(lines))]


def test_collater_accepts_mixed_rates(tmp_path):
    items = _items(tmp_path)
    assert [it[4] for it in items] == list(RATES)
    waves, lengths, crops, f0s, sils, rates = md.Collater()(items)
    assert torch.is_tensor(rates) and rates.dtype == torch.int32 and rates.tolist() == list(RATES)
    for i, item in enumerate(items):
        w1, l1, c1, f1, s1, r1 = md.Collater()([item])
        assert r1 == RATES[i]
        assert lengths[i] == l1[0] and crops[i] == c1[0]
        assert torch.equal(f0s[i], f1[0]) and torch.equal(sils[i], s1[0])
        assert torch.equal(waves[i, :l1[0]], w1[0]) and (waves[i, l1[0]:] == 0).all()


def test_single_rate_batch_keeps_an_int(tmp_path):
    items = _items(tmp_path, rates=(44100,) * 3, seconds=(1.0, 2.0, 0.5))
    out = md.Collater()(items)
    assert type(out[5]) is int and out[5] == 44100


def test_pitch_shift_batch_carries_base_rates():
    def item(sr, n, out_len):
        req = md.PitchShiftRequest("x.wav", 2.0, 1.0, n, 0, 0, out_len, 0, None)
        return torch.ones(n), torch.zeros(10), torch.zeros(10), 0, sr, req
    batch = [item(16000, 1000, 1500), (torch.ones(800), torch.zeros(5), torch.zeros(5), 0, 24000),
             item(44100, 2000, 1089)]
    out = md.Collater()(batch)
    assert out[5].tolist() == [16000, 24000, 44100]
    pack = out[-1]
    assert isinstance(pack, md.PitchShiftBatch)
    assert pack.rows.tolist() == [0, 2] and pack.src_sr.tolist() == [16000, 44100]
    assert pack.src_len.tolist() == [1000, 2000] and pack.src.numel() == 3000
    single = md.Collater()([item(16000, 1000, 1500), item(16000, 700, 1050)])
    assert single[5] == 16000 and single[-1].src_sr is None


# --------------------------------------------------------------------------- C ABI, host side only
@pytest.fixture(scope="module")
def lib():
    build.build_library(verbose=False)
    return _lib.load()


def test_ragged_plan_and_forward_argument_checks(lib):
    """A plan whose rates all equal the target is a plan of copies and allocates nothing on the device, so every
    host-side check of pe_resample_ragged_forward can run here; nothing is launched."""
    bad = -1
    plan = ctypes.c_void_p()
    rates = (ctypes.c_int * 2)(24000, 24000)
    assert lib.pe_resample_ragged_plan_create(ctypes.byref(plan), rates, 0, 24000, 6, 0.99) == bad
    assert lib.pe_resample_ragged_plan_create(ctypes.byref(plan), rates, 17, 24000, 6, 0.99) == bad
    assert lib.pe_resample_ragged_plan_create(ctypes.byref(plan), (ctypes.c_int * 1)(-1), 1, 24000, 6, 0.99) == bad
    assert lib.pe_resample_ragged_plan_create(ctypes.byref(plan), None, 1, 24000, 6, 0.99) == bad
    assert lib.pe_resample_ragged_plan_create(ctypes.byref(plan), rates, 2, 24000, 6, 0.99) == 0
    try:
        assert lib.pe_resample_ragged_out_len(plan, 1, 1234) == 1234
        assert lib.pe_resample_ragged_out_len(plan, 2, 1234) == bad
        assert lib.pe_resample_ragged_out_len(None, 0, 1234) == bad
        buf = (ctypes.c_float * 64)()
        x = y = ctypes.cast(buf, ctypes.c_void_p)
        off = ctypes.cast((ctypes.c_long * 2)(0, 16), ctypes.c_void_p)
        n_in = (ctypes.c_int * 2)(16, 10)
        idx = (ctypes.c_int * 2)(0, 1)
        p_n, p_i = ctypes.cast(n_in, ctypes.c_void_p), ctypes.cast(idx, ctypes.c_void_p)

        def fwd(**kw):
            a = dict(plan=plan, x=x, off=off, n=p_n, i=p_i, hn=p_n, hi=p_i, batch=2, y=y, stride=32, width=16)
            a.update(kw)
            return lib.pe_resample_ragged_forward(a["plan"], a["x"], a["off"], a["n"], a["i"], a["hn"], a["hi"],
                                                  a["batch"], a["y"], a["stride"], a["width"], None)
        for name in ("plan", "x", "off", "n", "i", "hn", "hi", "y"):
            assert fwd(**{name: None}) == bad, name
        assert fwd(stride=15) == bad                                   # y_stride < y_width
        assert fwd(width=15) == bad                                    # row 0's 16 outputs do not fit
        assert fwd(batch=-1) == bad
        idx[1] = 2
        assert fwd() == bad                                            # rate index out of range
        idx[1] = -1
        assert fwd() == bad
        idx[1] = 1
        assert fwd(batch=0) == 0                                       # nothing to do, nothing launched
    finally:
        assert lib.pe_resample_ragged_plan_destroy(plan) == 0

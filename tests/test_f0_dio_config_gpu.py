"""The HIP DIO + StoneMask tracker (csrc/f0_dio.hip) off its default configuration (``dio_ref.CONFIG_CASES``).

The six checks of tests/test_f0_dio_gpu.py -- band signals, events, candidates, ``pe_f0_dio_fix`` equal to the float32
restatement exactly, StoneMask, end to end with row-alone bit-identity -- under their rules, each on the restatement's
float64 result of the stage before it and against 4x the configuration's own float32-vs-float64 yardstick.  A batch is
the three short rows around an up- and a down-glide that are margin inputs under that configuration
(tests/test_f0_dio_cpu.py asserts it, and that each configuration reaches what it is there for).
"""
import numpy as np
import pytest
import torch

from tests import dio_ref as D
from tests import test_f0_dio_gpu as G

pytestmark = pytest.mark.gpu

CASES = pytest.mark.parametrize("case", D.CONFIG_CASES, ids=D.CASE_IDS)


def _batch(case):
    _, sr, hop, config, inputs = case
    return G._batch(sr, hop, config, inputs)


@CASES
def test_band_signals(case):
    G.check_band_signals(_batch(case))


@CASES
def test_events(case):
    G.check_events(_batch(case))


@CASES
def test_candidates(case):
    G.check_candidates(_batch(case))


@CASES
def test_contour_fix_equals_the_float32_restatement(case):
    G.check_contour_fix(_batch(case))


@CASES
def test_stonemask(case):
    G.check_stonemask(_batch(case))


@CASES
def test_end_to_end_ragged_and_deterministic(case):
    G.check_end_to_end(_batch(case), True)


def test_stonemask_leaves_frames_above_a_twelfth_of_the_rate_unvoiced():
    """8 kHz: fs / 12 is 667 Hz, under the default f0_ceil.  The frames whose DIO value lies above it come back as 0."""
    B = _batch(D.CONFIG_CASES[0])
    tr, pl = B["tr"], B["pl"]
    assert B["sr"] == 8000 and tr.n_fft == 1024
    f0 = np.zeros(pl["n_frames"], np.float32)
    for _, _, ref, _, _, fo, T in G._rows(B):
        f0[fo:fo + T] = ref["dio"]
    out = tr.stage_stonemask(B["flat"], torch.from_numpy(f0).cuda(), pl).cpu().numpy()
    above = f0 > B["sr"] / 12.0
    total = 0
    for _, _, ref, _, _, fo, T in G._rows(B):
        here = above[fo:fo + T]
        total += int(here.sum())
        assert not np.any(ref["f0"][here] > 0) and not np.any(out[fo:fo + T][here] > 0)
    print(f"[f0_dio] sr 8000: {total} frames with a DIO value above fs / 12, all 0 after StoneMask on both sides")
    assert total >= 10


def test_track_f0_passes_f0_ceil_to_the_kernel():
    """The keyword reaches the kernels and the tracker cache keeps configurations apart."""
    from pitchextractor_amd import inference
    from pitchextractor_amd.f0_tracker import WorldDioTracker
    sr, hop = 24000, 300
    y = D.margin_inputs(sr)[0]                                        # 75 -> 780 Hz
    default = inference.track_f0(y, sr=sr, hop_length=hop, backend="dio")
    low = inference.track_f0(y, sr=sr, hop_length=hop, backend="dio", f0_ceil=400.0)
    direct = WorldDioTracker(sr, hop, f0_ceil=400.0).track(torch.from_numpy(y).cuda())[0]
    print(f"[f0_dio] track_f0: voiced frames {int((default > 0).sum())} by default, {int((low > 0).sum())} under f0_ceil "
          f"400, highest {default.max():.1f} / {low.max():.1f} Hz")
    assert np.array_equal(low, direct)
    assert default.max() > 700.0 and 0 < low.max() <= 400.0 * 1.2 and (low > 0).sum() < (default > 0).sum()
    assert np.array_equal(inference.track_f0(y, sr=sr, hop_length=hop, backend="dio"), default)

"""The mix at an SNR is one implementation (csrc/snr_mix.h) behind two entry points, ``pe_noise_mix`` and
``pe_stim_finish``.  Two things hold it there:

* the bits both entry points left BEFORE they shared it, recorded on an MI355X with the parent build by
  tests/golden/make_snr_mix_parent_golden.py as digests (tests/golden/snr_mix_parent_bits.json), on the cases of
  tests/snr_mix_cases.py: every piece-boundary length alone, packed at odd offsets and padded, both sides of the peak
  rule, silent rows, rows without noise, a warm-up in the noise plan, and a row of 258 pieces (more than one 256-wide walk);
* the two entry points against each other: without a fade, ``stimuli.finish`` IS ``noise.mix_at_snr``.
"""
import json
from pathlib import Path

import numpy as np
import pytest
import torch

from pitchextractor_amd import noise as N, stimuli as S
from tests import snr_mix_cases as cases

pytestmark = pytest.mark.gpu

GOLDEN = json.loads((Path(__file__).resolve().parent / "golden" / "snr_mix_parent_bits.json").read_text())


@pytest.fixture(scope="module")
def got(hip_device):
    """Every case once: {case: (y, stats)}."""
    return cases.run_cases(hip_device)


def test_the_cases_are_the_recorded_ones_and_reach_both_sides_of_the_peak_rule(got):
    assert sorted(got) == sorted(GOLDEN)
    for entry in ("mix/", "stim"):
        peaks = np.concatenate([st[:, 0].cpu().numpy() for name, (_, st) in got.items() if name.startswith(entry)])
        scales = np.concatenate([st[:, 3].cpu().numpy() for name, (_, st) in got.items() if name.startswith(entry)])
        assert np.any(peaks > 0.99) and np.any((peaks > 0.0) & (peaks <= 0.99)) and np.any(peaks == 0.0), entry
        assert np.any(scales == 0.0) and np.any(scales > 0.0), entry


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_the_bits_are_the_parent_builds(got, name):
    y, stats = got[name]
    print(name, "peak", stats[:, 0].cpu().tolist(), "scale", stats[:, 3].cpu().tolist())
    assert {"y": cases.digest(y), "stats": cases.digest(stats)} == GOLDEN[name]


def test_finish_without_a_fade_is_mix_at_snr(hip_device):
    """At a sample rate below 50 Hz the fade is 0 samples, and ``finish`` of caller-supplied rows with noise is the
    mix alone: ``y`` and ``stats`` equal ``mix_at_snr``'s of the same signal, noise and SNRs."""
    sr = 40
    assert S.fade_samples(sr) == 0
    table = [(1, 0.25, 20.0, ""), (7, 0.25, 10.0, ""), (2047, 0.25, 0.0, ""), (2048, 0.9, 0.0, ""),
             (2049, 0.25, -5.0, ""), (6149, 0.9, -5.0, ""), (2049, 0.25, 20.0, "signal"), (2049, 0.25, 60.0, "noise"),
             (3 * 2048, 0.25, 3.5, "")]
    rows = [cases.row_inputs(200 + r, n, amp, what) for r, (n, amp, _, what) in enumerate(table)]
    lengths, snr = [n for n, _, _, _ in table], [s for _, _, s, _ in table]
    x = torch.from_numpy(np.concatenate([r[0] for r in rows])).to(hip_device)
    z = torch.from_numpy(np.concatenate([r[1] for r in rows])).to(hip_device)
    want_y, want_stats = N.mix_at_snr(x, z, snr, lengths, return_stats=True)
    pl = S.plan_rows([cases.stim_spec(n, sr, s) for n, s in zip(lengths, snr)], sr)
    assert pl["fade"] == 0 and pl["n_noise"] == sum(lengths)
    y, stats = S.finish(pl, x.clone(), z, return_stats=True)
    assert torch.equal(y, want_y) and torch.equal(stats, want_stats)
    peaks = stats[:, 0].cpu().numpy()
    assert np.any(peaks > 0.99) and np.any(peaks <= 0.99) and not torch.equal(y, x)

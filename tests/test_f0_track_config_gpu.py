"""The HIP F0 tracker (csrc/f0_track.hip) off its default configuration, against the float64 restatement.

The rules are those of tests/test_f0_track_gpu.py: the kernel gets 4x the case's own float32-vs-float64 yardstick
(``f0_track_ref.config_yardstick`` on the case's own rows) for cents, strength and contour; on margin rows the candidate
sets and the voicing agree in every frame, on natural rows at most 1 % of the frames may differ in either; two runs
agree, and a row alone is bit-identical to the row in the packed batch.  That the rows are margin inputs under their
configuration, and that each configuration reaches what it is there for (``f0_track_ref.CONFIG_CASES``), is asserted on
the CPU in tests/test_f0_track_config_cpu.py.

On a natural row a frame differs in its set when its count differs or when a matched pair is further apart than two
neighbouring maxima of r can be (``f0_track_ref.set_deviation``): with more than 14 maxima the count alone is always 15.
On the white-noise rows the 14 selected of 50 to 340 maxima are the quantity under test, so there the matched frames are
also held to 4x the rows' own float32-vs-float64 deviation in cents and strength.  Every figure is printed before it is
asserted; tools/bench_f0_track.py records them in profiles/bench_f0_track.json.
"""
import numpy as np
import pytest
import torch

from tests import f0_track_ref as R
from tests.test_f0_track_gpu import _compare, _pack, _row

pytestmark = pytest.mark.gpu


def run_case(case):
    """One configuration case on the device: the deviations of every row (the assertions run on the way)."""
    from pitchextractor_amd.f0_tracker import PraatACTracker
    name, sr, hop, min_pitch, config, inputs = case
    tr = PraatACTracker(sr, hop, min_pitch=min_pitch, **dict(config))
    margin, natural, pairs, nat_pairs, yard = R.case_fixtures(case)
    waves, kinds = margin + natural, ["margin"] * len(margin) + ["natural"] * len(natural)
    refs = [a for a, _ in pairs] + [a for a, _ in nat_pairs]
    print(f"[f0_track config] {name} sr {sr} hop {hop} min_pitch {min_pitch} {dict(config)} fft {tr.n_fft}: yardstick "
          f"cents {yard['cents']:.3e} strength {yard['strength']:.3e} natural contour {yard['natural_cents']:.3e} natural "
          f"sets {yard['natural_set_cents']:.3e} cents {yard['natural_set_strength']:.3e}")
    assert all(R.is_margin_input(a, yard["strength"], yard["cents"]) for a, _ in pairs)
    flat, lengths = _pack(waves)
    out = tr.track(flat, lengths, return_candidates=True)
    again = tr.track(flat, lengths, return_candidates=True)
    for k in ("cand_f", "cand_s", "cand_n"):
        assert np.array_equal(out[k], again[k]), "two runs differ"
    assert all(np.array_equal(a, b) for a, b in zip(out["f0"], again["f0"]))
    devs = []
    for r, (kind, ref) in enumerate(zip(kinds, refs)):
        got = _row(out, r)
        tag = f"{name} row {r} ({kind}, {len(waves[r]) / sr:.2f} s)"
        # the strength tolerance is only printed for a natural row; on the noise rows it is the one asserted below
        dev = _compare(tag, got, ref, 4 * (yard["cents"] if kind == "margin" else yard["natural_cents"]),
                       4 * (yard["natural_set_strength"] if inputs == "noise" else yard["strength"]), kind == "margin")
        sets = R.set_deviation(ref, got)
        print(f"[f0_track config] {tag}: frames with another set {sets['mismatches']} of {sets['frames']}, the others "
              f"within {sets['cents']:.3e} cents {sets['strength']:.3e} strength; maxima per frame up to "
              f"{int(ref['n_maxima'].max())}")
        assert sets["mismatches"] <= (0 if kind == "margin" else 0.01 * sets["frames"]), (tag, sets)
        if inputs == "noise":
            assert sets["cents"] <= 4 * yard["natural_set_cents"], (tag, sets)
            assert sets["strength"] <= 4 * yard["natural_set_strength"], (tag, sets)
        devs.append(dict(dev, kind=kind, set_other=sets["mismatches"], set_cents=sets["cents"],
                         set_strength=sets["strength"]))
    for r, w in enumerate(waves):
        alone = tr.track(torch.from_numpy(w).cuda(), return_candidates=True)
        assert np.array_equal(alone["f0"][0], out["f0"][r]), f"row {r} differs alone"
        packed = _row(out, r)
        for k in ("cand_f", "cand_s", "cand_n"):
            assert np.array_equal(alone[k], packed[k]), f"row {r} {k} differs alone"
    return yard, devs


@pytest.mark.parametrize("case", R.CONFIG_CASES, ids=R.CASE_IDS)
def test_configuration_against_the_restatement(case):
    run_case(case)


def test_track_f0_passes_max_pitch_to_the_kernel():
    """The keyword reaches the kernel and the tracker cache keeps configurations apart."""
    from pitchextractor_amd import inference
    from pitchextractor_amd.f0_tracker import PraatACTracker
    sr, hop = 16000, 160
    y = R.CASE_INPUTS["ceiling"](sr)[0][0]                            # tones at 150, 420, 220 and 500 Hz
    default = inference.track_f0(y, sr=sr, hop_length=hop, backend="praat", min_pitch=75.0)
    low = inference.track_f0(y, sr=sr, hop_length=hop, backend="praat", min_pitch=75.0, max_pitch=300.0)
    direct = PraatACTracker(sr, hop, min_pitch=75.0, max_pitch=300.0).track(torch.from_numpy(y).cuda())[0]
    print(f"[f0_track config] track_f0: voiced frames {int((default > 0).sum())} by default, {int((low > 0).sum())} "
          f"under max_pitch 300, highest {default.max():.1f} / {low.max():.1f} Hz")
    assert np.array_equal(low, direct)
    assert default.max() > 400.0 and 0 < low.max() < 300.0 and (low > 0).sum() < (default > 0).sum()
    assert np.array_equal(inference.track_f0(y, sr=sr, hop_length=hop, backend="praat", min_pitch=75.0), default)

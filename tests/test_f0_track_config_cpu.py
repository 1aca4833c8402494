"""The inputs of the F0 tracker's configuration cases (tests/f0_track_ref.py ``CONFIG_CASES``), without a device.

tests/test_f0_track_config_gpu.py holds the kernels to 4x each case's own float32-vs-float64 yardstick and demands equal
candidate sets and voicing on the margin rows.  That is only fair if the rows are margin inputs under that
configuration, and only worth running if the configuration reaches the code it is there for.  Both are asserted here, on
the float64 run of the restatement: conditions (a)-(c) and the ceiling gap (d) against the case's own yardstick, the
float32 restatement keeping every margin path and staying inside 1 % on the natural rows, and per case the branch
counts.  Every figure is printed before it is asserted.
"""
import numpy as np
import pytest

from tests import f0_track_ref as R

CASES = {c[0]: c for c in R.CONFIG_CASES}


@pytest.mark.parametrize("case", R.CONFIG_CASES, ids=R.CASE_IDS)
def test_rows_are_margin_inputs_and_float32_keeps_them(case):
    name, sr, hop, min_pitch, config, _ = case
    margin, natural, pairs, nat_pairs, yard = R.case_fixtures(case)
    print(f"[f0_track config] {name} ({sr}, {hop}, min_pitch {min_pitch}, {dict(config)}): yardstick cents "
          f"{yard['cents']:.3e} strength {yard['strength']:.3e} natural contour {yard['natural_cents']:.3e} natural sets "
          f"{yard['natural_set_cents']:.3e} cents {yard['natural_set_strength']:.3e}")
    assert 3 <= len(margin) + len(natural) <= 4 or not margin
    assert all(len(y) <= 2 * sr for y in margin + natural)
    bound = 1000.0 * yard["strength"]
    ceil_bound = 1000.0 * (2.0 ** (yard["cents"] / 1200.0) - 1.0)
    if margin:
        assert 0 < yard["strength"] < 1e-5 and 0 < yard["cents"] < 0.5
    for r, (a, b) in enumerate(pairs):
        d = R.deviation(a, b)
        print(f"[f0_track config]   margin row {r}: frames {d['frames']} voiced {int((a['f0'] > 0).sum())} path margin "
              f"{a['margin']:.3e} threshold gap {a['thr_gap']:.3e} 15th gap {a['gap15']:.3e} (bound {bound:.3e}) ceiling "
              f"gap {a['ceil_gap']:.3e} (bound {ceil_bound:.3e}); float32: flips {d['voicing_flips']} set mismatches "
              f"{d['set_mismatches']}")
        assert a["margin"] >= bound and a["thr_gap"] > bound and a["gap15"] > bound and a["ceil_gap"] >= ceil_bound
        assert R.is_margin_input(a, yard["strength"], yard["cents"])
        assert d["voicing_flips"] == 0 and d["set_mismatches"] == 0 and R.set_deviation(a, b)["mismatches"] == 0
        assert np.array_equal(a["f0"] > 0, b["f0"] > 0)
    for r, (a, b) in enumerate(nat_pairs):
        d, sets = R.deviation(a, b), R.set_deviation(a, b)
        print(f"[f0_track config]   natural row {r}: frames {d['frames']} maxima per frame {int(a['n_maxima'].min())} .. "
              f"{int(a['n_maxima'].max())}; float32: flips {d['voicing_flips']} frames with another set "
              f"{sets['mismatches']}")
        assert d["voicing_flips"] <= 0.01 * d["frames"] and sets["mismatches"] <= 0.01 * d["frames"]


def _above(res):
    live = np.arange(R.N_CAND)[None, :] < res["cand_n"][:, None]
    return (live & (res["cand_f"] >= res["consts"].ceiling)).any(axis=1)


def test_ceiling_300_takes_the_ceiling_branch():
    _, _, pairs, _, _ = R.case_fixtures(CASES["ceiling_300"])
    above = sum(int(_above(a).sum()) for a, _ in pairs)
    alone = sum(int(R.unvoiced_by_ceiling(a).sum()) for a, _ in pairs)
    voiced = sum(int((a["f0"] > 0).sum()) for a, _ in pairs)
    print(f"[f0_track config] ceiling_300: frames with a candidate at or above 300 Hz {above}, frames unvoiced because "
          f"the path's candidate is one {alone}, voiced frames {voiced}")
    assert above >= 20 and alone >= 20 and voiced >= 20
    assert pairs[0][0]["consts"].ceiling == 300.0
    for a, _ in pairs:                                              # such a frame is unvoiced in the contour
        assert not np.any(a["f0"][R.unvoiced_by_ceiling(a)] > 0)


def _local_and_voiced_without_ceiling(cand_f, cand_s, cand_n, c):
    """``f0_track_ref._local_and_voiced`` of a path that takes a candidate at or above the ceiling for voiced."""
    f, s = cand_f.astype(np.float64), cand_s.astype(np.float64)
    valid = np.arange(R.N_CAND)[None, :] < np.asarray(cand_n)[:, None]
    voiced = valid & (f > 0)
    local = np.where(voiced, s - c.octave_cost * np.log2(c.ceiling / np.where(voiced, f, 1.0)), s)
    return np.where(valid, local, -np.inf), voiced, np.where(voiced, np.log2(np.where(voiced, f, 1.0)), 0.0)


def test_ceiling_300_separates_a_path_that_forgets_the_ceiling(monkeypatch):
    """On the bursts row the contour changes when the path takes candidates at or above the ceiling for voiced, although
    the contour itself is still gated by the ceiling: the ceiling in the local score and the transitions is reached."""
    _, sr, hop, min_pitch, config, inputs = CASES["ceiling_300"]
    y = R.CASE_INPUTS[inputs](sr)[0][2]
    c = R.Consts(sr, hop, min_pitch=min_pitch, **dict(config))
    cand = R.candidates(y, c)
    _, kept = R.viterbi(*cand, c)
    monkeypatch.setattr(R, "_local_and_voiced", _local_and_voiced_without_ceiling)
    _, forgot = R.viterbi(*cand, c)                                  # its contour is still gated by the ceiling
    flips = int(np.count_nonzero((kept > 0) != (forgot > 0)))
    print(f"[f0_track config] ceiling_300 bursts row: {int((kept > 0).sum())} voiced frames, {flips} more when the path "
          "forgets the ceiling")
    assert flips >= 10


def test_ceiling_nyquist_is_the_clamp():
    _, sr, hop, min_pitch, config, _ = CASES["ceiling_nyquist"]
    c = R.Consts(sr, hop, min_pitch=min_pitch, **dict(config))
    assert c.ceiling == 0.5 * sr < dict(config)["max_pitch"]
    # the local score of every voiced candidate moves with log2(ceiling / f): not the default's
    _, _, pairs, _, _ = R.case_fixtures(CASES["ceiling_nyquist"])
    default = R.track(R.CASE_INPUTS["glides"](sr)[0][0], sr, hop, min_pitch=min_pitch)
    assert np.array_equal(default["cand_f"], pairs[0][0]["cand_f"]) and default["margin"] != pairs[0][0]["margin"]


def test_costs_a_separates_the_two_transition_costs():
    """The weak burst is voiced when a voicing change costs 0.14 and unvoiced when it costs what an octave jump does."""
    _, sr, hop, min_pitch, config, inputs = CASES["costs_a"]
    cfg = dict(config, min_pitch=min_pitch)
    y = R.CASE_INPUTS[inputs](sr)[0][2]
    a = R.track(y, sr, hop, **cfg)
    swapped = R.track(y, sr, hop, **dict(cfg, voiced_unvoiced_cost=cfg["octave_jump_cost"]))
    flips = int(np.count_nonzero((a["f0"] > 0) != (swapped["f0"] > 0)))
    print(f"[f0_track config] costs_a burst row: {int((a['f0'] > 0).sum())} voiced frames, {flips} of them unvoiced "
          "when the voicing change is charged the jump cost")
    assert flips >= 5


def test_costs_zero_has_free_transitions():
    _, sr, hop, min_pitch, config, _ = CASES["costs_zero"]
    c = R.Consts(sr, hop, min_pitch=min_pitch, **dict(config))
    assert c.octave_cost == 0.0 and c.octave_jump_cost == 0.0 and c.vuv_cost == 0.0
    # with nothing to pay the path is the strongest candidate of every frame
    for a, _ in R.case_fixtures(CASES["costs_zero"])[2]:
        live = np.arange(R.N_CAND)[None, :] < a["cand_n"][:, None]
        assert np.array_equal(a["path"], np.argmax(np.where(live, a["cand_s"], -np.inf), axis=1))


@pytest.mark.parametrize("name", ["thresholds_low", "thresholds_high"])
def test_thresholds_reach_both_sides_of_the_unvoiced_strength(name):
    _, _, pairs, _, _ = R.case_fixtures(CASES[name])
    positive = zero = 0
    for a, _ in pairs:
        term = a["cand_s"][:, 0].astype(np.float64) - a["consts"].voicing
        positive += int(np.count_nonzero((term > 0) & ~a["silent"]))
        zero += int(np.count_nonzero((term == 0) & ~a["silent"]))
    print(f"[f0_track config] {name}: frames (not digitally silent) whose unvoiced strength has a positive intensity "
          f"term {positive}, a zero one {zero}")
    assert positive >= 10 and zero >= 10


def test_maxima_rows_fill_the_rank_and_drop():
    _, _, _, nat48, _ = R.case_fixtures(CASES["maxima_48k"])
    _, _, _, nat16, _ = R.case_fixtures(CASES["maxima_16k"])
    a48, a16 = nat48[0][0], nat16[0][0]
    print(f"[f0_track config] maxima per frame: 48 kHz {int(a48['n_maxima'].min())} .. {int(a48['n_maxima'].max())} "
          f"over {a48['n_maxima'].size} frames, 16 kHz {int(a16['n_maxima'].min())} .. {int(a16['n_maxima'].max())}")
    assert a48["n_maxima"].size == 53 and a48["n_maxima"].max() > 256
    assert a16["n_maxima"].min() > R.N_CAND - 1 and a16["n_maxima"].max() <= 256
    assert np.all(a48["cand_n"] == R.N_CAND)                         # every frame drops all but the 14 best

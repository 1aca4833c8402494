"""The HIP F0 tracker (csrc/f0_track.hip) against the float64 restatement (tests/f0_track_ref.py).

Tolerances are not fitted to the kernel: the yardstick of a configuration is the deviation of the restatement run in
float32 from its float64 run on that configuration's own inputs (``f0_track_ref.config_yardstick``: cents of a
candidate's frequency and absolute strength over its margin inputs, cents of the contour over its natural inputs); the
kernel gets 4x that (its FFT factorisation, reduction order and sinf / log2f differ from numpy's).  Candidates are
compared as sets matched by frequency and the path as a contour, never by candidate index.  On margin inputs
(conditions (a)-(c), asserted in tests/test_f0_track_cpu.py) voicing must agree in every frame; on the natural inputs at
most 1 % of the frames may differ in voicing or in their candidate set, every other frame meets the frequency tolerance.
Every figure is printed before it is asserted; tools/bench_f0_track.py records them per configuration in
profiles/bench_f0_track.json.
"""
import numpy as np
import pytest
import torch

from tests import f0_track_ref as R

pytestmark = pytest.mark.gpu


def _tracker(sr, hop, min_pitch):
    from pitchextractor_amd.f0_tracker import PraatACTracker
    return PraatACTracker(sr, hop, min_pitch=min_pitch)


def _pack(waves):
    flat = torch.from_numpy(np.concatenate(waves).astype(np.float32)).cuda()
    return flat, [len(w) for w in waves]


def _row(out, r):
    o, n = int(out["frame_offsets"][r]), int(out["frames"][r])
    return dict(f0=out["f0"][r], cand_f=out["cand_f"][o:o + n], cand_s=out["cand_s"][o:o + n],
                cand_n=out["cand_n"][o:o + n])


def _compare(tag, got, ref, tol_cents, tol_strength, margin):
    T = ref["cand_n"].shape[0]
    assert got["cand_n"].shape[0] == T and got["f0"].shape[0] == T, (tag, "frame count")
    dev = R.deviation(ref, got)
    print(f"[f0_track] {tag}: frames {T} cand cents {dev['cents']:.3e} (tol {tol_cents:.3e}) strength "
          f"{dev['strength']:.3e} (tol {tol_strength:.3e}) set mismatches {dev['set_mismatches']} voicing flips "
          f"{dev['voicing_flips']} contour cents {dev['contour_cents']:.3e}")
    if margin:
        assert dev["set_mismatches"] == 0 and dev["voicing_flips"] == 0, (tag, dev)
        assert dev["cents"] <= tol_cents and dev["strength"] <= tol_strength, (tag, dev)
    else:
        assert dev["set_mismatches"] <= 0.01 * T and dev["voicing_flips"] <= 0.01 * T, (tag, dev)
    assert dev["contour_cents"] <= tol_cents, (tag, dev)
    # frames below the digital-silence rule hold the unvoiced candidate only, on both sides
    assert np.array_equal(got["cand_n"][ref["silent"]], np.ones(int(ref["silent"].sum()), np.int32))
    return dev


@pytest.mark.parametrize("sr,hop,min_pitch,long_seconds", R.GPU_CONFIGS)
def test_ragged_batch_against_the_restatement(sr, hop, min_pitch, long_seconds):
    tr = _tracker(sr, hop, min_pitch)
    margin = R.margin_inputs(sr, long_seconds)
    natural = R.natural_inputs(sr)
    short = [np.zeros(tr.nsamp_window // 2, np.float32), 0.1 * np.ones(int(3.0 * sr / min_pitch) + 5, np.float32)]
    waves = [short[0]] + margin[:2] + [natural[0], short[1]] + margin[2:] + [natural[1]]
    kinds = ["short"] + ["margin"] * 2 + ["natural", "short"] + ["margin"] * 2 + ["natural"]
    pairs = R.reference_pairs(sr, hop, min_pitch, long_seconds)
    yard = R.config_yardstick(sr, hop, min_pitch, long_seconds)
    yard_cents, yard_strength = yard["cents"], yard["strength"]
    print(f"[f0_track] sr {sr} hop {hop} min_pitch {min_pitch} fft {tr.n_fft}: yardstick cents {yard_cents:.3e} "
          f"strength {yard_strength:.3e} natural contour cents {yard['natural_cents']:.3e}")
    assert all(R.is_margin_input(a, yard_strength) for a, _ in pairs)
    flat, lengths = _pack(waves)
    out = tr.track(flat, lengths, return_candidates=True)
    again = tr.track(flat, lengths, return_candidates=True)
    for k in ("cand_f", "cand_s", "cand_n"):
        assert np.array_equal(out[k], again[k]), "two runs differ"
    assert all(np.array_equal(a, b) for a, b in zip(out["f0"], again["f0"]))
    assert out["f0"][0].size == 0                                     # shorter than one window: no frames
    refs = {"margin": iter(a for a, _ in pairs), "natural": iter(a for a, _ in R.natural_pairs(sr, hop, min_pitch))}
    for r, kind in enumerate(kinds):
        got = _row(out, r)
        if kind == "short":
            ref = R.track(waves[r], sr, hop, min_pitch=min_pitch)
            assert got["f0"].shape[0] == ref["f0"].shape[0] and not np.any(got["f0"] > 0)
            continue
        _compare(f"row {r} ({kind}, {len(waves[r]) / sr:.2f} s)", got, next(refs[kind]),
                 4 * (yard_cents if kind == "margin" else yard["natural_cents"]), 4 * yard_strength, kind == "margin")
    # every row alone, and in a padded 2-D batch, is bit-identical to the row inside the packed batch
    width = max(lengths)
    padded = torch.zeros((len(waves), width), dtype=torch.float32, device="cuda")
    for r, w in enumerate(waves):
        padded[r, :len(w)] = torch.from_numpy(w)
    in_padded = tr.track(padded, lengths)
    for r, w in enumerate(waves):
        alone = tr.track(torch.from_numpy(w).cuda())[0]
        assert np.array_equal(alone, out["f0"][r]), f"row {r} differs alone"
        assert np.array_equal(in_padded[r], out["f0"][r]), f"row {r} differs in the padded batch"


def test_back_pointer_spill_equals_the_restatement():
    sr, hop, min_pitch, seconds = R.SPILL_CONFIG
    tr = _tracker(sr, hop, min_pitch)
    margin = R.config_margin_inputs(sr, hop, min_pitch, seconds)
    pairs = R.reference_pairs(sr, hop, min_pitch, seconds)
    yard = R.config_yardstick(sr, hop, min_pitch, seconds)
    yard_cents, yard_strength = yard["cents"], yard["strength"]
    print(f"[f0_track] spill sr {sr} hop {hop} min_pitch {min_pitch}: yardstick cents {yard_cents:.3e} strength "
          f"{yard_strength:.3e}")
    assert all(R.is_margin_input(a, yard_strength) for a, _ in pairs)
    assert tr.frame_count(len(margin[-1])) > tr.lds_frames
    assert tr.plan([len(w) for w in margin])["workspace_bytes"] == 16 * tr.frame_count(len(margin[-1]))
    flat, lengths = _pack(margin)
    out = tr.track(flat, lengths, return_candidates=True)
    for r in range(len(margin)):
        _compare(f"spill row {r}", _row(out, r), pairs[r][0], 4 * yard_cents, 4 * yard_strength, True)
    alone = tr.track(torch.from_numpy(margin[-1]).cuda())[0]
    assert np.array_equal(alone, out["f0"][-1])


def test_host_tensors_are_refused():
    tr = _tracker(24000, 300, 40.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tr.track(torch.zeros(24000))


def test_track_f0_feeds_pitch_metrics():
    from pitchextractor_amd import inference
    from pitchextractor_amd.meldataset import align_length
    sr, hop = 24000, 300
    y, curve = R.glide_signal(2.0, 120.0, 300.0, sr, seed=3)
    f0 = inference.track_f0(y, sr=sr, hop_length=hop)
    ref = R.track(y, sr, hop)
    assert f0.dtype == np.float32 and f0.shape == ref["f0"].shape
    L = 1 + len(y) // hop
    m = inference.pitch_metrics(align_length(f0, L), align_length(ref["f0"], L))
    assert m["vuv_error"] == 0.0 and m["rpa"] == 1.0 and m["rms_cents"] < 0.1


def _stats_in_kernel_order(x):
    """{mean, max |x - mean|} of one row as ``pe_row_stats`` documents it: 64 pieces of ceil(n / 64) samples; in a piece
    thread t of 256 adds samples t, t + 256, .. in float64, the threads are summed as a binary tree (t += t + h,
    h = 128 .. 1), the pieces in order; mean = float32(sum / n); the peak is a float32 maximum."""
    n = x.size
    if n == 0:
        return np.float32(0.0), np.float32(0.0)
    per = -(-n // 64)
    total = np.float64(0.0)
    for c in range(64):
        piece = x[c * per:min(c * per + per, n)].astype(np.float64)
        lanes = np.zeros(256, np.float64)
        for k in range(0, piece.size, 256):
            part = piece[k:k + 256]
            lanes[:part.size] += part
        h = 128
        while h:
            lanes[:h] += lanes[h:2 * h]
            h >>= 1
        total = total + lanes[0]
    mean = np.float32(total / np.float64(n))
    return mean, np.max(np.abs(x - mean)).astype(np.float32)


def test_row_stats_do_not_depend_on_the_plan_stride():
    from pitchextractor_amd import _lib
    from pitchextractor_amd.f0_tracker import PraatACTracker, WorldDioTracker
    lengths = [0, 1, 255, 70001]                                      # the last: all 64 pieces, a ragged tail
    rng = np.random.default_rng(5)
    rows = [(rng.standard_normal(n) * 0.2 + 0.25).astype(np.float32) for n in lengths]
    flat, _ = _pack(rows)
    trackers = [PraatACTracker(24000, 300), WorldDioTracker(24000, 300)]
    plans = [tr.plan(lengths) for tr in trackers]
    assert plans[0]["meta"].shape[1] != plans[1]["meta"].shape[1]
    got = []
    for tr, pl in zip(trackers, plans):
        meta_d = torch.from_numpy(pl["meta"]).cuda()
        stats = torch.full((len(lengths), 2), float("nan"), dtype=torch.float32, device="cuda")
        tr._row_stats(flat, meta_d, len(lengths), stats, _lib.stream_ptr(), 0)
        got.append(stats.cpu().numpy())
    assert np.array_equal(got[0].view(np.uint32), got[1].view(np.uint32))
    for r, x in enumerate(rows):
        mean, peak = _stats_in_kernel_order(x)
        print(f"[row_stats] row {r}: n {x.size} mean {got[0][r, 0]!r} (numpy {mean!r}) peak {got[0][r, 1]!r} "
              f"(numpy {peak!r})")
        assert got[0][r, 0] == mean and got[0][r, 1] == peak

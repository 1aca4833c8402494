"""The HIP DIO + StoneMask tracker (csrc/f0_dio.hip) against the float64 restatement (tests/dio_ref.py).

Every stage runs through its own entry point on the restatement's float64 result of the stage before it, cast to
float32, so an error shows at the stage that makes it.  Tolerances are not fitted to the kernels: the yardstick of a
configuration is the deviation of the restatement's float32 run from its float64 run on that configuration's own
inputs (``dio_ref.config_yardstick``), and the kernels get 4x that (FFT factorisation, reduction order and device
transcendentals differ from numpy's).  ``pe_f0_dio_fix`` only compares and copies: it must equal the float32
restatement exactly.  On margin inputs (asserted in tests/test_f0_dio_cpu.py) event counts, best bands and voicing
are equal; on the natural inputs at most 1 % of the frames may differ in voicing.  Every figure is printed before it is
asserted; tools/bench_f0_dio.py records them in profiles/bench_f0_dio.json.

Each check is a function of a batch (``_batch``) that returns the worst figures of its margin rows, so that
tests/test_f0_dio_config_gpu.py runs the same checks on the configurations of ``dio_ref.CONFIG_CASES``.
"""
import functools
import json
import os

import numpy as np
import pytest
import torch

from tests import dio_ref as D

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _batch(sr, hop, config=(), inputs=None):
    """The ragged batch of one configuration: the short rows around its margin and natural rows, the float64 run of
    every row, the plan and the yardstick.  ``config`` / ``inputs``: as ``dio_ref.reference_pairs`` takes them."""
    from pitchextractor_amd.f0_tracker import WorldDioTracker
    cfg = dict(config)
    tr = WorldDioTracker(sr, hop, **cfg)
    short = D.short_inputs(sr)
    margin, natural = D.config_margin_inputs(sr, inputs), (D.natural_inputs(sr) if inputs is None else [])
    waves = short[:2] + margin[:1] + [short[2]] + natural + margin[1:]
    kinds = ["short"] * 2 + ["margin"] + ["short"] + ["natural"] * len(natural) + ["margin"] * (len(margin) - 1)
    m_refs = iter(a for a, _ in D.reference_pairs(sr, hop, True, config, inputs))
    n_refs = iter(a for a, _ in D.natural_pairs(sr, hop, True, config, inputs))
    refs = [next(m_refs) if k == "margin" else next(n_refs) if k == "natural" else D.track(w, sr, hop, **cfg)
            for w, k in zip(waves, kinds)]
    flat = torch.from_numpy(np.concatenate(waves).astype(np.float32)).cuda()
    lengths = [len(w) for w in waves]
    pl = tr._device_plan(flat, lengths)
    tag = f"sr {sr}" + "".join(f" {k} {v:g}" for k, v in config) + ("" if inputs is None else f" hop {hop}")
    return dict(tr=tr, sr=sr, hop=hop, cfg=cfg, tag=tag, waves=waves, kinds=kinds, refs=refs, flat=flat,
                lengths=lengths, pl=pl, yard=D.config_yardstick(sr, hop, config, inputs))


def _rows(B):
    pl = B["pl"]
    for r, (kind, ref) in enumerate(zip(B["kinds"], B["refs"])):
        yield r, kind, ref, int(pl["sample_offsets"][r]), int(pl["lengths"][r]), int(pl["frame_offsets"][r]), \
            int(pl["frames"][r])


def _pack_events(B):
    tr, pl = B["tr"], B["pl"]
    slots = pl["n_event_slots"] * tr.bands * 4
    e_idx, e_frac = np.zeros(slots, np.int32), np.zeros(slots, np.float32)
    e_count = np.zeros((pl["n_rows"], tr.bands, 4), np.int32)
    for r, _, ref, _, n, _, _ in _rows(B):
        cap, base = n // 2 + 1, int(pl["event_offsets"][r]) * tr.bands * 4
        for b in range(tr.bands):
            for k in range(4):
                idx, frac = ref["events"][b][k]
                at = base + (b * 4 + k) * cap
                assert idx.size <= cap
                e_idx[at:at + idx.size], e_frac[at:at + idx.size] = idx, frac
                e_count[r, b, k] = idx.size
    return torch.from_numpy(e_idx).cuda(), torch.from_numpy(e_frac).cuda(), torch.from_numpy(e_count).cuda()


@pytest.mark.parametrize("sr,hop", D.GPU_CONFIGS)
def test_band_signals(sr, hop):
    check_band_signals(_batch(sr, hop))


def check_band_signals(B):
    tag = B["tag"]
    sig = B["tr"].stage_bands(B["flat"], B["pl"]).cpu().numpy()
    tol, worst_rel = 4 * B["yard"]["band"], 0.0
    for r, kind, ref, so, n, _, _ in _rows(B):
        if n == 0:
            continue
        got = sig[:, so:so + n]
        peak = float(np.max(np.abs(ref["bands"])))
        err = float(np.max(np.abs(got - ref["bands"])))
        print(f"[f0_dio] {tag} bands row {r} ({kind}, {n} samples, {-(-n // B['tr'].block_step)} blocks): peak "
              f"{peak:.3e} error / peak {err / max(peak, 1e-30):.3e} (tol {tol:.3e})")
        assert np.all(np.isfinite(got))
        assert err <= tol * peak if peak > 0 else err == 0.0
        worst_rel = max(worst_rel, err / peak if peak > 0 else 0.0)
    return dict(band=worst_rel)


@pytest.mark.parametrize("sr,hop", D.GPU_CONFIGS)
def test_events(sr, hop):
    check_events(_batch(sr, hop))


def check_events(B):
    tag = B["tag"]
    tr, pl = B["tr"], B["pl"]
    sig = np.zeros((tr.bands, pl["n_samples"]), np.float32)
    for _, _, ref, so, n, _, _ in _rows(B):
        sig[:, so:so + n] = ref["bands"]
    e_idx, e_frac, e_count = (t.cpu().numpy() for t in tr.stage_events(torch.from_numpy(sig).cuda(), pl))
    tol, worst_edge = 4 * B["yard"]["edge"], 0.0
    for r, kind, ref, _, n, _, _ in _rows(B):
        same = np.array_equal(e_count[r], ref["counts"])
        worst = 0.0
        if same:
            for kg, kr in zip(tr.row_events(e_idx, e_frac, e_count, pl, r), ref["events"]):
                for (ig, fg), (ir, fr) in zip(kg, kr):
                    if ir.size:
                        worst = max(worst, float(np.max(np.abs((ig - ir) + (fg.astype(np.float64) - fr)))))
        print(f"[f0_dio] {tag} events row {r} ({kind}): edges {int(ref['counts'].sum())} counts equal {same} fine "
              f"edge error {worst:.3e} samples (tol {tol:.3e})")
        if kind != "natural":
            assert same
        if same:
            assert worst <= tol
        if kind == "margin":
            worst_edge = max(worst_edge, worst)
    return dict(edge=worst_edge)


@pytest.mark.parametrize("sr,hop", D.GPU_CONFIGS)
def test_candidates(sr, hop):
    check_candidates(_batch(sr, hop))


def check_candidates(B):
    tag = B["tag"]
    tr, pl = B["tr"], B["pl"]
    cand, score, best, band = (t.cpu().numpy() for t in tr.stage_candidates(*_pack_events(B), pl))
    yard = B["yard"]
    fig = dict(cand_cents=0.0, score=0.0, best_band_differs=0)
    for r, kind, ref, _, _, fo, T in _rows(B):
        got = dict(cand=cand[:, fo:fo + T], score=score[:, fo:fo + T], best=best[fo:fo + T],
                   best_band=band[fo:fo + T], bands=ref["bands"], counts=ref["counts"], events=ref["events"],
                   f0=ref["f0"])
        dev = D.stage_deviation(ref, got)
        print(f"[f0_dio] {tag} candidates row {r} ({kind}, {T} frames): cents {dev['cand_cents']:.3e} (tol "
              f"{4 * yard['cand_cents']:.3e}) score {dev['score']:.3e} (tol {4 * yard['score']:.3e}) accepted differ "
              f"{dev['cand_flips']} best band differs {dev['best_band_differs']} (gap {dev['best_band_gap']:.3e} cents)")
        assert got["cand"].shape == ref["cand"].shape
        if kind == "natural":
            assert dev["cand_flips"] <= 0.01 * ref["cand"].size
            continue
        assert dev["cand_flips"] == 0
        assert dev["cand_cents"] <= 4 * yard["cand_cents"] and dev["score"] <= 4 * yard["score"]
        assert dev["best_band_differs"] == 0 or dev["best_band_gap"] <= 4 * yard["cand_cents"]
        same = got["best_band"] == ref["best_band"]
        assert np.array_equal(got["best"][same] > 0, ref["best"][same] > 0)
        if kind == "margin":
            fig = dict(cand_cents=max(fig["cand_cents"], dev["cand_cents"]), score=max(fig["score"], dev["score"]),
                       best_band_differs=fig["best_band_differs"] + dev["best_band_differs"])
    return fig


@pytest.mark.parametrize("sr,hop", D.GPU_CONFIGS)
def test_contour_fix_equals_the_float32_restatement(sr, hop):
    check_contour_fix(_batch(sr, hop))


def check_contour_fix(B):
    tag = B["tag"]
    tr, pl = B["tr"], B["pl"]
    G = pl["n_frames"]
    best, cand = np.zeros(G, np.float32), np.zeros((tr.bands, G), np.float32)
    for _, _, ref, _, _, fo, T in _rows(B):
        best[fo:fo + T], cand[:, fo:fo + T] = ref["best"], ref["cand"]
    steps = tr.stage_fix(torch.from_numpy(best).cuda(), torch.from_numpy(cand).cuda(), pl).cpu().numpy()
    for r, kind, ref, _, _, fo, T in _rows(B):
        want = D.fix_contour(best[fo:fo + T], cand[:, fo:fo + T], ref["consts"], np.float32)
        changed = [int(np.count_nonzero(want[s] != (want[s - 1] if s else best[fo:fo + T]))) for s in range(4)]
        print(f"[f0_dio] {tag} fix row {r} ({kind}, {T} frames): frames changed by step 1 .. 4 {changed}")
        for s in range(4):
            assert np.array_equal(steps[s, fo:fo + T], want[s]), (r, s)
    return dict(fix_equals_float32_restatement=True)


@pytest.mark.parametrize("sr,hop", D.GPU_CONFIGS)
def test_stonemask(sr, hop):
    check_stonemask(_batch(sr, hop))


def check_stonemask(B):
    tag = B["tag"]
    tr, pl = B["tr"], B["pl"]
    f0 = np.zeros(pl["n_frames"], np.float32)
    for _, _, ref, _, _, fo, T in _rows(B):
        f0[fo:fo + T] = ref["dio"]
    out = tr.stage_stonemask(B["flat"], torch.from_numpy(f0).cuda(), pl).cpu().numpy()
    tol, fig = 4 * B["yard"]["stonemask_cents"], dict(stonemask_cents=0.0, stonemask_flips=0)
    for r, kind, ref, _, _, fo, T in _rows(B):
        worst, flips = D.contour_deviation(ref["f0"], out[fo:fo + T])
        moved = float(np.max(D.cents(ref["f0"][ref["f0"] > 0], ref["dio"][ref["f0"] > 0]))) if np.any(ref["f0"] > 0) else 0
        print(f"[f0_dio] {tag} stonemask row {r} ({kind}, {T} frames): {worst:.3e} cents (tol {tol:.3e}) voicing "
              f"flips {flips}; the refinement itself moves up to {moved:.2f} cents")
        assert worst <= tol
        assert flips == 0 if kind != "natural" else flips <= 0.01 * T
        if kind == "margin":
            fig = dict(stonemask_cents=max(fig["stonemask_cents"], worst), stonemask_flips=fig["stonemask_flips"] + flips)
    return fig


@pytest.mark.parametrize("stonemask", [True, False])
@pytest.mark.parametrize("sr,hop", D.GPU_CONFIGS)
def test_end_to_end_ragged_and_deterministic(sr, hop, stonemask):
    check_end_to_end(_batch(sr, hop), stonemask)


def check_end_to_end(B, stonemask):
    from pitchextractor_amd.f0_tracker import WorldDioTracker
    tag = B["tag"]
    tr = B["tr"] if stonemask else WorldDioTracker(B["sr"], B["hop"], stonemask=False, **B["cfg"])
    yard, key = B["yard"], "f0" if stonemask else "dio"
    tol = {"margin": 4 * yard["cents" if stonemask else "dio_cents"],
           "natural": 4 * yard["natural_cents" if stonemask else "natural_dio_cents"]}
    out = tr.track(B["flat"], B["lengths"])
    again = tr.track(B["flat"], B["lengths"])
    assert all(np.array_equal(a, b) for a, b in zip(out, again)), "two runs differ"
    fig = dict(contour_cents=0.0, voicing_flips=0, frames=0)
    for r, kind, ref, _, _, _, T in _rows(B):
        got = out[r]
        assert got.dtype == np.float32 and got.shape == (T,)
        if kind == "short":
            assert not np.any(got > 0) and not np.any(ref[key] > 0)
            continue
        worst, flips = D.contour_deviation(ref[key], got)
        print(f"[f0_dio] {tag} stonemask {stonemask} row {r} ({kind}, {T} frames, {int((got > 0).sum())} voiced): "
              f"contour {worst:.3e} cents (tol {tol[kind]:.3e}) voicing flips {flips}")
        assert worst <= tol[kind]
        assert flips == 0 if kind == "margin" else flips <= 0.01 * T
        if kind == "margin":
            fig = dict(contour_cents=max(fig["contour_cents"], worst), voicing_flips=fig["voicing_flips"] + flips,
                       frames=fig["frames"] + T)
    # every row alone, and in a padded 2-D batch, is bit-identical to the row inside the packed batch
    width = max(max(B["lengths"]), 1)
    padded = torch.zeros((len(B["waves"]), width), dtype=torch.float32, device="cuda")
    for r, w in enumerate(B["waves"]):
        padded[r, :len(w)] = torch.from_numpy(w)
    in_padded = tr.track(padded, B["lengths"])
    for r, w in enumerate(B["waves"]):
        alone = tr.track(torch.from_numpy(w).cuda())[0]
        assert np.array_equal(alone, out[r]), f"row {r} differs alone"
    for r in range(len(B["waves"])):
        assert np.array_equal(in_padded[r], out[r]), f"row {r} differs in the padded batch"
    return fig


def test_track_f0_feeds_pitch_metrics():
    from pitchextractor_amd import inference
    from pitchextractor_amd.meldataset import align_length
    sr, hop = 24000, 300
    y = D.margin_inputs(sr)[0]
    ref = D.reference_pairs(sr, hop)[0][0]
    f0 = inference.track_f0(y, sr=sr, hop_length=hop, backend="dio")
    assert f0.dtype == np.float32 and f0.shape == ref["f0"].shape
    L = 1 + len(y) // hop
    m = inference.pitch_metrics(align_length(f0, L), align_length(ref["f0"], L))
    print(f"[f0_dio] track_f0(backend='dio') against the restatement: {m}")
    assert m["vuv_error"] == 0.0 and m["rpa"] == 1.0
    with pytest.raises(ValueError):
        inference.track_f0(y, sr=sr, hop_length=hop, backend="harvest")


def test_wav_folder_is_labelled_by_the_chain(tmp_path, hip_device):
    from pitchextractor_amd.meldataset import build_dataloader
    from tests.test_data_layer import write_wav
    sr, hop = 24000, 300
    f0_params = {"bad_f0_threshold": 5, "zero_fill_value": 0.0, "backend_order": ["pyworld_dio", "praat"],
                 "backends": {"pyworld_dio": {"type": "pyworld", "enabled": True,
                                              "config": {"algorithm": "dio", "fallback": None, "stonemask": True}},
                              "praat": {"type": "praat", "enabled": True, "config": {"method": "ac"}}}}
    suffix = "_f0-pyworld_dio_praat"
    files = []
    for k, (a, b) in enumerate([(90.0, 300.0), (80.0, 380.0), (300.0, 120.0), (200.0, 600.0)]):
        y = D.S.glide_signal(1.0, a, b, sr, seed=30 + k)[0]
        p = str(tmp_path / f"utt{k}.wav")
        write_wav(p, y, sr, "float32")
        files.append((p, y))
    short = str(tmp_path / "short.wav")
    write_wav(short, 0.1 * np.ones(1000, np.float32), sr, "float32")
    lines = [f"{p}|0\n" for p, _ in files] + [f"{short}|0\n"]
    build_dataloader(lines, validation=True, batch_size=4, num_workers=0, device=hip_device,
                     dataset_config={"mel_params": {"sample_rate": sr, "win_len": 1024, "n_fft": 1024, "n_mels": 80,
                                                    "hop_length": hop}, "f0_params": f0_params})
    pairs = [(D.track(y, sr, hop), D.track(y, sr, hop, dtype=np.float32)) for _, y in files]
    yard = max(D.contour_deviation(a["f0"], b["f0"])[0] for a, b in pairs)
    for (p, y), (ref, ref32) in zip(files, pairs):
        got = np.load(p + suffix + ".npy")
        with open(p + suffix + ".json") as fh:
            meta = json.load(fh)
        assert meta == {"cache_identifier": "-pyworld_dio_praat", "backend": "pyworld_dio", "sample_rate": sr,
                        "hop_length": hop}
        worst, flips = D.contour_deviation(ref["f0"], got)
        flips32 = D.contour_deviation(ref["f0"], ref32["f0"])[1]
        print(f"[f0_dio prepass] {os.path.basename(p)}: {int((got > 0).sum())} voiced of {got.size}, contour "
              f"{worst:.3e} cents (yardstick {yard:.3e}, tolerance 4x), voicing flips {flips} (float32 restatement "
              f"{flips32})")
        assert got.dtype == np.float32 and got.shape == ref["f0"].shape and (got > 0).sum() > 30
        assert worst <= 4 * yard and flips <= max(flips32, 0.01 * got.size)
    # too short to be voiced for DIO and shorter than one window for praat: every backend failed, as in the reference
    assert np.load(short + suffix + ".npy").shape == (0,)
    with open(short + suffix + ".json") as fh:
        assert json.load(fh)["backend"] == ""

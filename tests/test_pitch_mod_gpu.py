"""Pitch modulation on the GPU (csrc/pitch_mod.hip) against the float64 restatement of tests/pitch_mod_ref.py: the
wave kernel's accuracy on its boundaries, its bit-identity across layouts, the label kernel, audio and label taken
together through the F0 tracker, and the loader stage."""
import functools
import random
from typing import NamedTuple

import numpy as np
import pytest
import torch

from pitchextractor_amd import pitch_mod as PM
from tests import pitch_mod_ref as R

pytestmark = pytest.mark.gpu

SR, HOP = 24000, 32
MODS = {
    "none": PM.Modulation(),
    "ramp": PM.Modulation((), 0.5),                                          # s from 0.5 to 1.5: the widest staging
    "four": PM.Modulation(((0.03, 6.0, 0.7), (0.005, 13.0, 2.0), (0.02, 0.9, 4.0), (0.04, 40.0, 1.0)), 0.0),
    "mixed": PM.Modulation(((0.05, 5.5, 0.3), (0.01, 11.0, 1.0)), -0.2),
}
SPANS = ("start", "mid", "end")


def bits(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def rows():
    """The rows of every wave test: lengths around the kernel's tile and one that is whole hops (so that a span can end
    at n), noise plus a tone, float32."""
    tile = PM.kernel_consts()["tile"]
    lengths = [0, 1, tile - 1, tile, tile + 1, 2 * tile + 3, 96 * HOP]
    rng = np.random.default_rng(17)
    waves = [(0.3 * rng.standard_normal(n) + 0.4 * np.sin(2 * np.pi * 440.0 * np.arange(n) / SR)).astype(np.float32)
             for n in lengths]
    return lengths, waves


def spans_of(kind, lengths):
    """(spans, counts): from the row's first frame; from an odd frame to before the row's end; from frame 3 to the last
    frame (t1 = n for the row of whole hops)."""
    crop = {"start": 0, "mid": 5, "end": 3}[kind]
    spans, counts = PM.frame_spans(lengths, [crop] * len(lengths), HOP)
    if kind == "mid":
        counts = np.maximum(counts - 6, 0)
        spans[:, 1] = (crop + np.maximum(counts, 1) - 1) * HOP
    return spans, counts


def mods_of(name, counts):
    return [MODS[name] if c >= 2 else None for c in counts]


@functools.lru_cache(maxsize=None)
def reference(kind, name, quality):
    """Per row (float64 restatement, float32 restatement), computed once."""
    lengths, waves = rows()
    spans, counts = spans_of(kind, lengths)
    return [(R.warp(x, int(a), int(b), m, SR, quality), R.warp_f32(x, int(a), int(b), m, SR, quality))
            for x, (a, b), m in zip(waves, spans, mods_of(name, counts))]


def padded(waves, dev, order=None, extra=0):
    order = list(range(len(waves))) if order is None else order
    x = torch.zeros((len(order), max(len(w) for w in waves) + extra), device=dev)
    for k, r in enumerate(order):
        x[k, :len(waves[r])] = torch.from_numpy(waves[r]).to(dev)
    return x


def run_padded(kind, name, quality, dev, order=None, **kw):
    lengths, waves = rows()
    order = list(range(len(waves))) if order is None else order
    spans, counts = spans_of(kind, lengths)
    mods = mods_of(name, counts)
    return PM.modulate(padded(waves, dev, order), [lengths[r] for r in order], spans[order], [mods[r] for r in order],
                       sr=SR, hop=HOP, quality=quality, **kw)


# ------------------------------------------------------------------------------------------------------------ accuracy
@pytest.mark.parametrize("quality", ["kaiser_fast", "kaiser_best"])
@pytest.mark.parametrize("name", sorted(MODS))
@pytest.mark.parametrize("kind", SPANS)
def test_wave_accuracy_on_the_kernels_boundaries(hip_device, kind, name, quality):
    """The kernel's deviation from the float64 restatement, relative to the row's maximum, is held to 4x the deviation
    of the float32 restatement (the kernel's arithmetic in numpy) from the same."""
    lengths, waves = rows()
    spans, counts = spans_of(kind, lengths)
    assert spans[-1, 1] == lengths[-1] or kind != "end"
    got = run_padded(kind, name, quality, hip_device).cpu().numpy()
    worst_kernel = worst_f32 = 0.0
    for r, (n, (y64, y32)) in enumerate(zip(lengths, reference(kind, name, quality))):
        assert not got[r, n:].any()
        if n == 0:
            continue
        top = float(np.max(np.abs(y64)))
        worst_kernel = max(worst_kernel, float(np.max(np.abs(got[r, :n].astype(np.float64) - y64))) / top)
        worst_f32 = max(worst_f32, float(np.max(np.abs(y32.astype(np.float64) - y64))) / top)
        t0, t1 = (int(v) for v in spans[r])
        outside = np.r_[0:min(t0 + 1, n), min(t1, n):n]
        assert np.array_equal(bits(got[r, :n])[outside], bits(waves[r])[outside])
        if counts[r] < 2 or name == "none":
            assert np.array_equal(bits(got[r, :n]), bits(waves[r]))
        else:
            assert not np.array_equal(got[r, t0 + 1:t1], waves[r][t0 + 1:t1])
    print(f"{kind} {name} {quality}: kernel {worst_kernel:.3e}, float32 restatement {worst_f32:.3e}")
    assert worst_kernel <= 4.0 * worst_f32


# --------------------------------------------------------------------------------------------------------- bit-identity
@pytest.mark.parametrize("kind,name,quality", [("mid", "mixed", "kaiser_fast"), ("end", "ramp", "kaiser_best"),
                                               ("start", "four", "kaiser_fast")])
def test_wave_is_bit_identical_across_layouts(hip_device, kind, name, quality):
    lengths, waves = rows()
    spans, counts = spans_of(kind, lengths)
    mods = mods_of(name, counts)
    call = functools.partial(PM.modulate, sr=SR, hop=HOP, quality=quality)
    base = run_padded(kind, name, quality, hip_device)
    want = [bits(base[r, :n]) for r, n in enumerate(lengths)]
    # alone
    for r, n in enumerate(lengths):
        if n:
            alone = call(torch.from_numpy(waves[r]).to(hip_device), None, spans[r:r + 1], [mods[r]])
            assert np.array_equal(bits(alone), want[r]), r
    # packed back to back: the third row starts at the odd offset 1
    flat = torch.from_numpy(np.concatenate(waves + [np.zeros(5, np.float32)])).to(hip_device)
    packed = call(flat, lengths, spans, mods)
    off = np.cumsum([0] + lengths)
    assert off[2] % 2 == 1
    assert all(np.array_equal(bits(packed[off[r]:off[r] + n]), want[r]) for r, n in enumerate(lengths))
    assert not packed[off[-1]:].any()
    # reversed batch order
    order = list(range(len(lengths)))[::-1]
    back = run_padded(kind, name, quality, hip_device, order)
    assert all(np.array_equal(bits(back[k, :lengths[r]]), want[r]) for k, r in enumerate(order))
    # into a wider stride, from a packed input
    wide = torch.full((len(lengths), max(lengths) + 37), 9.0, device=hip_device)
    assert call(flat, lengths, spans, mods, out=wide) is wide
    assert all(np.array_equal(bits(wide[r, :n]), want[r]) and (wide[r, n:] == 9.0).all() for r, n in enumerate(lengths))
    # the table from L2 or from its copy in LDS
    if quality == "kaiser_fast":
        for in_lds in (False, True):
            assert np.array_equal(bits(run_padded(kind, name, quality, hip_device, table_in_lds=in_lds)), bits(base))
    # not selected, and the identity: the input's bits
    x = padded(waves, hip_device)
    for none in ([None] * len(lengths), [PM.Modulation()] * len(lengths)):
        assert np.array_equal(bits(call(x, lengths, spans, none)), bits(x))
    # in place is refused
    with pytest.raises(ValueError):
        call(x, lengths, spans, mods, out=x)


# ------------------------------------------------------------------------------------------------------------ labels
def label_case():
    rng = np.random.default_rng(23)
    W = 192
    counts = [1, 2, 61, 192, 100, 37]
    mods = [None, MODS["ramp"], MODS["four"], MODS["mixed"], None, PM.Modulation()]
    f0 = (120.0 + 200.0 * rng.random((len(counts), W))).astype(np.float32)
    sil = np.zeros_like(f0)
    for r in range(len(counts)):
        f0[r, counts[r]:] = 7.0                                  # past the kept frames: copied whatever it holds
        for a, b in ((0, 2), (20, 31), (40, 41), (90, 120), (185, 192)):
            if r % 2 == 0:
                f0[r, a:min(b, counts[r])] = 0.0                 # unvoiced as 0 Hz
            else:
                f0[r, a:min(b, counts[r])], sil[r, a:min(b, counts[r])] = 61.5, 1.0      # a fill under the flag
    f0[3, 130:140] = 0.0                                         # 0 Hz without the flag
    sil[3, 150:155] = 1.0                                        # the flag over a voiced-looking value
    spans = np.array([[5 * HOP, (5 + max(c, 1) - 1) * HOP] for c in counts], np.int64)
    return counts, spans, mods, f0, sil


def test_labels_follow_the_restatement(hip_device):
    """Voiced results within 1 float32 ulp of the restatement's float64 value, flags equal, copies bit-exact."""
    counts, spans, mods, f0, sil = label_case()
    got_f, got_q = PM.modulate_labels(torch.from_numpy(f0).to(hip_device), torch.from_numpy(sil).to(hip_device),
                                      counts, spans, HOP, mods, sr=SR)
    got_f, got_q = got_f.cpu().numpy(), got_q.cpu().numpy()
    worst = 0.0
    for r, (c, mod) in enumerate(zip(counts, mods)):
        want_f, want_q = R.labels(f0[r], sil[r], c, mod, HOP, SR)
        assert np.array_equal(got_q[r], want_q), r
        assert np.array_equal(bits(got_f[r, c:]), bits(f0[r, c:])) and np.array_equal(bits(got_q[r, c:]), bits(sil[r, c:]))
        if mod is None or mod.identity:
            assert np.array_equal(bits(got_f[r]), bits(f0[r])) and np.array_equal(bits(got_q[r]), bits(sil[r]))
            continue
        w32 = want_f.astype(np.float32)
        ulps = np.abs(got_f[r].astype(np.float64) - w32.astype(np.float64)) / np.spacing(np.abs(w32)).astype(np.float64)
        worst = max(worst, float(ulps.max()))
        unvoiced = (want_q == 1) | (want_f == 0)
        assert np.array_equal(bits(got_f[r])[unvoiced], bits(w32)[unvoiced])            # copied, not scaled
        if c >= 61:                                              # the two-frame row is its fill throughout
            assert unvoiced[:c].any() and (~unvoiced[:c]).any()
            assert not np.array_equal(got_f[r, :c], f0[r, :c])
    print(f"labels: worst deviation {worst:.2f} float32 ulp")
    assert worst <= 1.0
    with pytest.raises(ValueError):
        PM.modulate_labels(torch.from_numpy(f0).to(hip_device), torch.from_numpy(sil).to(hip_device),
                           [c + 1 for c in counts], spans, HOP, mods, sr=SR)


# ------------------------------------------------------------------------------------------------------ audio and label
def test_audio_and_label_agree(hip_device):
    """A 220 Hz, 10-partial complex of 1 s with a constant label under vibrato plus a ramp, tracked by
    ``PraatACTracker`` (min_pitch 100): the RMS distance in cents between the tracked contour and the new labels is at
    most a quarter of the distance between the old and the new labels.  The same condition holds on the CPU for the
    restatement's output under the float64 tracker of tests/f0_track_ref.py (0.55 against 65.8 cents;
    tests/test_pitch_mod_cpu.py::test_audio_and_label_agree_on_the_restatement)."""
    from pitchextractor_amd.f0_tracker import PraatACTracker
    c = R.CONSISTENCY
    n, hop, sr = c["n"], c["hop"], c["sr"]
    L = 1 + n // hop
    x = torch.from_numpy(R.complex_tone(c["f0"], sr, n)).to(hip_device)
    y = PM.modulate(x, None, [[0, n]], [c["mod"]], sr=sr, hop=hop)
    f0 = torch.zeros((1, 192), device=hip_device)
    f0[0, :L] = c["f0"]
    new_f0, new_sil = PM.modulate_labels(f0, torch.zeros_like(f0), [L], [[0, n]], hop, [c["mod"]], sr=sr)
    assert not new_sil.any() and not new_f0[0, L:].any()
    tracker = PraatACTracker(sr, hop, min_pitch=c["min_pitch"])
    tracked = tracker.track(y)[0]
    to_new, old_to_new = R.consistency_scores(tracked, tracker.frame_times(n), new_f0[0, :L].cpu().numpy())
    print(f"rms cents: tracked vs new labels {to_new:.3f}, old vs new labels {old_to_new:.3f}")
    assert to_new <= 0.25 * old_to_new
    before = tracker.track(x)[0]
    assert R.rms_cents(before, np.full(before.size, c["f0"])) < 1.0


# -------------------------------------------------------------------------------------------------------- the modulator
def test_apply_moves_the_selected_rows_only(hip_device):
    lengths, waves = rows()
    x = padded(waves, hip_device)
    crops = [0, 0, 5, 0, 3, 7, 3]
    f0 = torch.full((len(lengths), 192), 180.0, device=hip_device)
    sil = torch.zeros_like(f0)
    pm = PM.PitchModulator({"vibrato": {"p": 1}, "glide": {"p": 1}, "p": 1}, SR, HOP, seed=2)
    plan = pm.draw(len(lengths))
    assert plan.on.all()
    nothing = pm.apply(x, lengths, crops, f0, sil, plan.without(range(len(lengths))))
    assert nothing[0] is x and nothing[1] is f0 and nothing[2] is sil
    y, f0n, siln = pm.apply(x, lengths, crops, f0, sil, plan.without([3, 5]))
    spans, counts = PM.frame_spans(lengths, crops, HOP)
    for r, n in enumerate(lengths):
        moved = r not in (3, 5) and counts[r] >= 2
        assert np.array_equal(bits(y[r]), bits(x[r])) != moved, r
        assert np.array_equal(bits(f0n[r]), bits(f0[r])) != moved, r
        if moved:
            want = R.warp_f32(waves[r], int(spans[r, 0]), int(spans[r, 1]), plan.mods[r], SR)
            assert np.max(np.abs(y[r, :n].cpu().numpy() - want)) <= 1e-5
            lab, _ = R.labels(f0[r].cpu().numpy(), sil[r].cpu().numpy(), counts[r], plan.mods[r], HOP, SR)
            assert np.allclose(f0n[r].cpu().numpy(), lab, rtol=2.0 ** -23)
    assert not siln.any()


# ----------------------------------------------------------------------------------------------------------- the loader
MEL = {"sample_rate": 24000, "win_len": 1024, "n_fft": 1024, "n_mels": 80, "hop_length": 300}
FULL = {"seed": 3, "p": 1.0, "vibrato": {"p": 1.0}, "flutter": {"p": 0.5}, "drift": {"p": 0.5}, "glide": {"p": 0.7}}
GAIN = {"seed": 1, "gain": {"p": 1.0}, "polarity": {"p": 0.5}}


@pytest.fixture(scope="module")
def file_list(tmp_path_factory):
    from pitchextractor_amd import synthetic
    from tests.test_data_layer import write_wav
    root = tmp_path_factory.mktemp("pitch_mod_files")
    lines = []
    for i, dur in enumerate((2.0, 1.3, 0.9, 2.2)):
        wave, f0, _ = synthetic.utterance(i, duration=dur)
        p = root / f"u{i}.wav"
        write_wav(p, wave, 24000, "float32")
        np.save(str(p) + "_f0.npy", f0)
        lines.append(f"{p}|0\n")
    return lines


def make_loader(lines, modulation, augmentation=None, validation=False):
    from pitchextractor_amd import meldataset as md
    cfg = {"mel_params": dict(MEL), "dataloader": {"start_method": None}, "verbose": False}
    if modulation is not None:
        cfg["pitch_modulation"] = modulation
    if augmentation is not None:
        cfg["augmentation"] = augmentation
    return md.build_dataloader(lines, validation=validation, batch_size=2, num_workers=0, device="cuda:0",
                               dataset_config=cfg)


def seed_all():
    np.random.seed(5)
    random.seed(5)
    torch.manual_seed(5)


def batches(lines, modulation, augmentation=None, validation=False, plans=None):
    loader = make_loader(lines, modulation, augmentation, validation)
    if plans is not None and loader.augmenter is not None:
        draw = loader.augmenter.draw
        loader.augmenter.draw = lambda n: plans.append(draw(n)) or plans[-1]
    seed_all()
    got = [tuple(t.cpu().numpy() for t in b) for b in loader]
    assert len(got) == 2
    return got


def same(a, b, parts=(0, 1, 2)):
    return all(np.array_equal(bits(x[k]), bits(y[k])) for x, y in zip(a, b) for k in parts)


def test_loader_stage(file_list, hip_device):
    from pitchextractor_amd import meldataset as md
    plain = batches(file_list, None)
    for off in ({**FULL, "enabled": False}, {**FULL, "p": 0.0}, {"seed": 3}):
        assert same(plain, batches(file_list, off))
    on = batches(file_list, FULL)
    assert all(not np.array_equal(a[k], b[k]) for a, b in zip(on, plain) for k in (0, 1))
    assert all(np.isfinite(a[0]).all() and np.isfinite(a[1]).all() for a in on)
    assert same(on, batches(file_list, FULL)) and not same(on, batches(file_list, {**FULL, "seed": 4}), parts=(0,))
    assert same(batches(file_list, FULL, validation=True), batches(file_list, None, validation=True))
    assert not same(batches(file_list, {**FULL, "apply_to_validation": True}, validation=True),
                    batches(file_list, None, validation=True), parts=(0, 1))
    with pytest.raises(ValueError):
        make_loader(file_list, {**FULL, "vibrato": {"p": 1.0, "depth_cents": [0, 500]}})
    # p: 1 is PitchModulator.apply with the same plans on the collated batches, then the mel launch
    loader = make_loader(file_list, None)
    manual = PM.PitchModulator(FULL, 24000, 300, seed=3)
    seed_all()
    for host, want in zip(loader.loader, on):
        waves, lengths, crops, f0s, sils = (t.to(hip_device) for t in host[:5])
        plan = manual.draw(len(lengths))
        waves, f0s, sils = manual.apply(waves, host[1].tolist(), host[2].tolist(), f0s, sils, plan)
        mels = loader.mel.log_mel_ragged(waves, lengths, crops, max_frames=md.MAX_MEL_LENGTH)
        assert same([want], [(mels, f0s, sils)])
    # the Augmenter draws what it drew without the stage, and works on the modulated rows
    alone, both = [], []
    gained = batches(file_list, None, GAIN, plans=alone)
    mixed = batches(file_list, FULL, GAIN, plans=both)
    assert len(alone) == len(both) == 2
    assert all(np.array_equal(p.gain_db, q.gain_db) and np.array_equal(p.polarity_on, q.polarity_on) and
               np.array_equal(p.noise_seed, q.noise_seed) for p, q in zip(alone, both))
    assert same(mixed, on, parts=(1, 2)) and same(gained, plain, parts=(1, 2)) and not same(mixed, gained, parts=(0,))


class FillRequest(NamedTuple):
    value: float
    out_len: int


class FillBatch(NamedTuple):
    rows: torch.Tensor
    out_len: torch.Tensor
    values: torch.Tensor


class Fill:
    """A test-only synthetic kind: its stage writes a ramp of the row's value over the row's window."""
    name, Request, Batch = "fill", FillRequest, FillBatch

    def collate(self, batch, rows, row_rates, mixed):
        reqs = [batch[i][-1] for i in rows]
        return FillBatch(torch.tensor(rows, dtype=torch.int64), torch.tensor([r.out_len for r in reqs]),
                         torch.tensor([r.value for r in reqs], dtype=torch.float32))

    def run(self, loader, waves, lengths, dev_batch, host_batch, src_sr):
        for row, n, value in zip(host_batch.rows.tolist(), host_batch.out_len.tolist(), host_batch.values.tolist()):
            waves[row, :n] = value * torch.sin(torch.arange(n, device=waves.device) * 0.05)
        return waves, lengths


def test_cached_and_synthetic_rows_are_left_alone(monkeypatch, hip_device):
    """Four rows through ``DeviceMelLoader``: a plain one, one with a cached spectrogram, one of a synthetic kind, a
    plain one.  The stage moves the plain rows only, unless ``apply_to_synthetic`` is set."""
    from pitchextractor_amd import meldataset as md
    from pitchextractor_amd import synthetic_items
    monkeypatch.setattr(synthetic_items, "KINDS", synthetic_items.KINDS + [Fill()])
    n, hop = 12000, 300
    frames = 1 + n // hop

    def plain(index, cached=False):
        rng = np.random.default_rng(index)
        item = (torch.from_numpy(rng.uniform(-0.5, 0.5, n).astype(np.float32)), torch.full((frames,), 100.0 + index),
                torch.zeros(frames), 0, 24000)
        return item + (torch.from_numpy(rng.standard_normal((80, frames)).astype(np.float32)),) if cached else item

    filled = (torch.zeros(0), torch.full((frames,), 200.0), torch.zeros(frames), 0, 24000, FillRequest(0.4, n))
    host = md.Collater()([plain(0), plain(1, cached=True), filled, plain(2)])
    assert host[6].tolist() == [1] and type(host[8]) is FillBatch

    class _Host:
        dataset = None

    def through(modulation):
        mod = None if modulation is None else PM.PitchModulator(modulation, 24000, hop, seed=1)
        loader = md.DeviceMelLoader(_Host(), md.MelSpectrogram(**md.DEFAULT_MEL_PARAMS), hip_device, None, mod)
        out = loader._finish(loader._submit(host))
        torch.cuda.synchronize()
        assert not loader._host
        return out

    config = {"p": 1.0, "vibrato": {"p": 1.0}, "glide": {"p": 1.0}}
    base, on, asked = through(None), through(config), through({**config, "apply_to_synthetic": True})
    for r, moved_on, moved_asked in ((0, True, True), (1, False, False), (2, False, True), (3, True, True)):
        for k in range(3 if r != 1 else 2):                      # a cached row's mel is the cached one either way
            assert torch.equal(on[k][r], base[k][r]) != (moved_on and k < 2), (r, k)
            assert torch.equal(asked[k][r], base[k][r]) != (moved_asked and k < 2), (r, k)
    assert torch.equal(on[0][1], base[0][1]) and torch.equal(on[1][1], base[1][1])

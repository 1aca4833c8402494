"""WORLD CheapTrick on the GPU against the float64 restatement (tests/cheaptrick_ref.py) in the log domain, with the
float32 restatement as the yardstick (the project's rule for float32 kernels: 4 x its own deviation from float64); bit
identity of ragged batching and of frame sub-ranges; the hand-off of the envelope to the synthesizer in place; the
analysis / resynthesis chain with the Praat-style tracker as an independent witness; and the data loader with
``world_resynthesis`` items on.  pyworld is not available: parity with its binary is unpinned.

Measured on the MI355X, worst ratio over a configuration's rows of max |ln gpu - ln float64| to the float32
restatement's own: fs 8000 / 5 ms 1.76, 8000 / 12.5 ms 1.44, 24000 / 5 ms 1.15, 24000 / 12.5 ms 0.88, 48000 / 5 ms
1.18, 48000 / 12.5 ms 1.56, 24000 / 12.5 ms with q1 = 0 0.88 (the deviations: 1.8e-6 on the all-zero row to 6.8e-4 on
the 48 kHz floor row).  The tracker's worst frame on the resynthesized tone is 3.10 cents (3 semitones up) and 6.51
cents (glide) off the label."""
import random

import numpy as np
import pytest
import torch

from pitchextractor_amd import inference, stimuli
from pitchextractor_amd import meldataset as md
from pitchextractor_amd import world
from pitchextractor_amd.f0_tracker import PraatACTracker
from tests import cheaptrick_ref as ct
from tests.test_data_layer import write_wav

pytestmark = pytest.mark.gpu


def _voice(fs, seconds, f0, seed, level=0.5):
    """A harmonic complex (1 / h partials up to 0.45 fs) over a little noise."""
    n = int(seconds * fs)
    t = np.arange(n) / fs
    rng = np.random.default_rng(seed)
    x = sum(np.sin(2 * np.pi * h * f0 * t + h) / h for h in range(1, max(2, int(0.45 * fs / f0))))
    x = level * x / np.abs(x).max() + 1e-3 * rng.standard_normal(n)
    return x.astype(np.float32)


def _rows(fs, fp):
    """name -> (wave float32, f0 float32): 0.1 to 0.4 s each."""
    N = ct.default_fft_size(fs)
    floor = ct.f0_floor_of(fs, N)
    frames = lambda x: 1 + int(len(x) / (fs * fp / 1000.0))  # noqa: E731
    rows = {}
    x = _voice(fs, 0.3, 132.7, 1)
    L = frames(x)                                               # the last frames sit at and past the row's end: clamped
    f0 = np.full(L, 132.7, np.float32)
    f0[L // 3:L // 3 + 3] = 0.0                                 # unvoiced frames
    rows["voiced_gap"] = (x, f0)
    x = _voice(fs, 0.4, floor * 1.01, 2)
    f0 = np.full(frames(x), floor + 0.05, np.float32)
    f0[1::2] = floor - 0.05                                     # just above and just below the floor
    rows["floor"] = (x, f0)
    x = _voice(fs, 0.2, 311.3, 3)
    rows["glide"] = (x, np.linspace(250.0, 380.0, frames(x)).astype(np.float32))
    rows["one_frame"] = (_voice(fs, 0.1, 200.0, 4), np.array([200.0], np.float32))
    rows["no_frames"] = (_voice(fs, 0.1, 200.0, 5), np.zeros(0, np.float32))
    rows["zeros"] = (np.zeros(int(0.1 * fs), np.float32), np.full(5, 150.0, np.float32))
    x = _voice(fs, 0.3, 180.0, 6, level=0.9)
    x[len(x) // 2:] *= np.float32(1e-4 / 0.9)                   # a 1e-4 passage next to a full-scale one
    rows["quiet_after_loud"] = (x, np.full(frames(x), 180.0, np.float32))
    if fs == 8000:
        x = _voice(fs, 0.1, 1000.0, 7)
        rows["f0_1000"] = (x, np.full(frames(x), 1000.0, np.float32))       # a 25-sample window
    return rows


CONFIGS = [(8000, 5.0, -0.15), (8000, 12.5, -0.15), (24000, 5.0, -0.15), (24000, 12.5, -0.15), (48000, 5.0, -0.15),
           (48000, 12.5, -0.15), (24000, 12.5, 0.0)]
_CASES = {}


def _cases(cfg):
    """The configuration's rows with their float64 and float32 restatements, computed once, never modified."""
    if cfg not in _CASES:
        fs, fp, q1 = cfg
        out = {}
        for name, (x, f0) in _rows(fs, fp).items():
            r64 = ct.cheaptrick(x.astype(np.float64), f0, fs, fp, q1=q1)
            r32 = ct.cheaptrick(x.astype(np.float64), f0, fs, fp, q1=q1, fp32=True)
            for a in (x, f0, r64, r32):
                a.setflags(write=False)
            out[name] = dict(x=x, f0=f0, r64=r64, r32=r32)
        _CASES[cfg] = out
    return _CASES[cfg]


def _run(cases, names, dev, fs, fp, q1=-0.15, padded=False, lead=0, **kw):
    """The named rows as one batch -> one (frames, bins) array per row.  ``lead``: a row of that many samples and no
    frames goes first, so the named rows start at that offset."""
    xs = [np.zeros(lead, np.float32)] * bool(lead) + [cases[n]["x"] for n in names]
    f0s = [np.zeros(0, np.float32)] * bool(lead) + [cases[n]["f0"] for n in names]
    lengths = [len(x) for x in xs]
    if padded:
        x = torch.zeros((len(xs), max(lengths) + 3), dtype=torch.float32)
        for r, a in enumerate(xs):
            x[r, :len(a)] = torch.from_numpy(a.copy())
        x = x.to(dev)
    else:
        x = torch.from_numpy(np.concatenate(xs + [np.zeros(1, np.float32)])).to(dev)
    env = world.cheaptrick_ragged(x, lengths, f0s, fs, fp, q1=q1, **kw)
    return [env.row(r).cpu().numpy() for r in range(len(f0s))][bool(lead):]


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: f"fs{c[0]}-fp{c[1]}-q{c[2]}")
def test_accuracy_against_the_restatement(hip_device, cfg):
    """max |ln sp - ln float64| per row <= 4 x the float32 restatement's own, one ragged launch per configuration."""
    fs, fp, q1 = cfg
    cases = _cases(cfg)
    names = list(cases)
    N = ct.default_fft_size(fs)
    assert N == {8000: 512, 24000: 1024, 48000: 2048}[fs]
    got = _run(cases, names, hip_device, fs, fp, q1)
    worst = 0.0
    for name, sp in zip(names, got):
        c = cases[name]
        assert sp.shape == c["r64"].shape == (c["f0"].size, N // 2 + 1) and sp.dtype == np.float32
        if not sp.size:
            continue
        assert np.isfinite(sp).all() and (sp > 0).all()
        e_gpu = np.abs(np.log(sp.astype(np.float64)) - np.log(c["r64"])).max()
        e_32 = np.abs(np.log(c["r32"].astype(np.float64)) - np.log(c["r64"])).max()
        print(f"[cheaptrick] fs {fs} fp {fp} q1 {q1} {name}: frames {sp.shape[0]} e_gpu {e_gpu:.3e} e_32 {e_32:.3e} "
              f"ratio {e_gpu / e_32:.2f}")
        worst = max(worst, e_gpu / e_32)
        assert e_gpu <= 4 * e_32, (name, e_gpu, e_32)
    print(f"[cheaptrick] fs {fs} fp {fp} q1 {q1}: worst ratio {worst:.2f}")
    # the single-row form is the same launch
    one = world.cheaptrick(torch.from_numpy(cases["glide"]["x"].copy()).to(hip_device), cases["glide"]["f0"], fs, fp,
                           q1=q1)
    np.testing.assert_array_equal(one.cpu().numpy(), got[names.index("glide")])


def test_bit_identity(hip_device):
    fs, fp = 24000, 5.0
    cases = _cases((fs, fp, -0.15))
    names = ["voiced_gap", "no_frames", "quiet_after_loud", "glide", "one_frame"]
    batch = _run(cases, names, hip_device, fs, fp)
    for k, name in enumerate(names):
        alone = _run(cases, [name], hip_device, fs, fp)[0]
        np.testing.assert_array_equal(alone, batch[k])
        odd = _run(cases, [name], hip_device, fs, fp, lead=1001)[0]          # packed at an odd sample offset
        np.testing.assert_array_equal(odd, alone)
    padded = _run(cases, names, hip_device, fs, fp, padded=True)
    rev = _run(cases, names[::-1], hip_device, fs, fp)[::-1]                 # first becomes last
    for k in range(len(names)):
        np.testing.assert_array_equal(padded[k], batch[k])
        np.testing.assert_array_equal(rev[k], batch[k])
    # a frame sub-range is the slice of the full analysis
    sub = [(5, 9), (0, 0), (0, len(cases["quiet_after_loud"]["f0"])), (11, 1), (0, 1)]
    part = _run(cases, names, hip_device, fs, fp, frames=sub)
    for k, (first, count) in enumerate(sub):
        assert part[k].shape[0] == count
        np.testing.assert_array_equal(part[k], batch[k][first:first + count])
    with pytest.raises(Exception, match="invalid argument"):
        _run(cases, ["glide"], hip_device, fs, fp, frames=[(30, len(cases["glide"]["f0"]))])


def test_argument_refusals(hip_device):
    x = torch.zeros(2400, device=hip_device)
    f0 = np.full(8, 120.0, np.float32)
    with pytest.raises(ValueError, match="fft_size"):
        world.cheaptrick(x, f0, 24000, 5.0, fft_size=4096)
    with pytest.raises(Exception, match="unsupported"):                        # 3 fs / (512 - 3) > 71 Hz
        world.cheaptrick(x, f0, 24000, 5.0, fft_size=512)
    assert world.cheaptrick(x, f0, 24000, 5.0, fft_size=512, f0_floor=150.0).shape == (8, 257)
    assert world.cheaptrick(x, f0, 24000, 5.0, fft_size=2048).shape == (8, 1025)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        world.cheaptrick(x.double(), f0, 24000, 5.0)
    with pytest.raises(ValueError, match="one F0 curve per row"):
        world.cheaptrick_ragged(x, [1200, 1200], [f0], 24000, 5.0)
    with pytest.raises(ValueError, match="smaller"):
        world.cheaptrick_ragged(x, [2400], [f0], 24000, 5.0, out=torch.zeros(100, device=hip_device))


def test_hand_off_to_the_synthesizer(hip_device):
    """resynthesize_ragged = cheaptrick_ragged, then world_synthesize_ragged reading the envelope where it lies."""
    fs, fp, N = 24000, 12.5, 1024
    bins = N // 2 + 1
    cases = _cases((fs, fp, -0.15))
    names = ["voiced_gap", "quiet_after_loud", "glide"]
    xs = [cases[n]["x"] for n in names]
    f0s = [cases[n]["f0"] for n in names]
    new = [f * np.float32(2 ** (3 / 12)) for f in f0s]
    new[0] = new[0].copy()
    new[0][:2] = 20.0                                                        # below lowest_f0: labelled 0, unvoiced
    x = torch.from_numpy(np.concatenate(xs)).to(hip_device)
    lengths = [len(a) for a in xs]
    ap = torch.full((bins,), 0.3, device=hip_device)
    gains = torch.tensor([0.5, 1.0, 2.0])
    seeds = [3, 2 ** 63 + 5, 7]
    y_len = [world.output_length(len(f), fs, fp) for f in f0s]
    for windows in (None, ([0, 1500, 700], [y_len[0], 2000, 1111])):
        kw = {} if windows is None else dict(out_start=windows[0], out_len=windows[1])
        out, labels = world.resynthesize_ragged(x, lengths, f0s, new, fs, fp, ap=ap, seeds=seeds, gains=gains, **kw)
        for lab, f in zip(labels, new):
            np.testing.assert_array_equal(lab, np.where(f.astype(np.float64) > world.lowest_f0(fs, N), f, 0.0))
        assert (labels[0][:2] == 0).all() and (labels[0][2:5] > 0).all()
        # by hand, the envelope at odd offsets with a stride wider than a frame
        stride = bins + 7
        offs = np.cumsum([11] + [len(f) * stride for f in f0s])[:-1]
        buf = torch.full((int(offs[-1] + len(f0s[-1]) * stride),), float("nan"), device=hip_device)
        env = world.cheaptrick_ragged(x, lengths, f0s, fs, fp, fft_size=N, out=buf, out_offsets=offs,
                                      out_strides=[stride] * 3)
        assert env.sp.data_ptr() == buf.data_ptr()
        want = torch.zeros_like(out)
        world.world_synthesize_ragged(labels, buf, env.frame0_offsets(), env.strides, gains, want, fs=fs,
                                      frame_period=fp, fft_size=N, ap=ap, ap_offsets=[0] * 3, ap_strides=[0] * 3,
                                      seeds=seeds, **kw)
        assert torch.equal(out, want) and out.abs().max() > 0.05 and torch.isfinite(out).all()
    one, label = world.resynthesize(x[:lengths[0]], f0s[0], new[0], fs, fp, ap=ap, seed=3)
    full, _ = world.resynthesize_ragged(x, lengths, f0s, new, fs, fp, ap=ap, seeds=seeds)
    assert torch.equal(one, full[0, :y_len[0]]) and one.numel() == y_len[0]
    np.testing.assert_array_equal(label, labels[0])


def test_resynthesized_tone_is_tracked_on_its_label(hip_device):
    """A "Bright Belt" 220 Hz tone complex (``stimuli.timbre_tones``, 0.4 s at 24 kHz), analysed with its analytic F0
    and resynthesized 3 semitones up and on a 200 -> 277 Hz glide, then tracked by ``inference.track_f0`` (praat).
    Compared: frames voiced in the label and at least 3 frames inside the voiced run.  Conditions: the tracker is
    voiced on >= 90 % of them and within 50 cents of the label (``test_f0_track_gpu``'s criterion for synthetic
    signals).  The float64 chain cheaptrick_ref -> world_ref.synthesize -> f0_track_ref on this input: 26 frames
    compared, all voiced, worst frame 3.1 cents (3 semitones up) and 6.5 cents (glide)."""
    fs, hop, fp = 24000, 300, 12.5
    tone = stimuli.timbre_tones([220.0], {"Bright Belt": stimuli.TIMBRE_PROFILES["Bright Belt"]}, duration=0.4, sr=fs,
                                device=hip_device)
    x = tone.rows()[0]
    L = 1 + x.numel() // hop
    f0 = np.full(L, 220.0)
    for tag, new in (("3 semitones up", f0 * 2 ** (3 / 12)), ("glide", np.linspace(200.0, 277.0, L))):
        wave, label = world.resynthesize(x, f0, new, fs, fp)
        np.testing.assert_array_equal(label, new)
        got = inference.track_f0(wave, sr=fs, hop_length=hop).astype(np.float64)
        times = PraatACTracker(fs, hop).frame_times(wave.numel())
        want = np.interp(times, np.arange(L) * (fp / 1000.0), label)
        frame = times / (fp / 1000.0)
        keep = (frame >= 3) & (frame <= L - 1 - 3)
        voiced = got[keep] > 0
        cents = 1200.0 * np.abs(np.log2(np.maximum(got[keep], 1e-5) / want[keep]))
        print(f"[cheaptrick] {tag}: {int(keep.sum())} frames, voiced {voiced.mean():.2f}, worst "
              f"{cents[voiced].max():.2f} cents")
        assert keep.sum() >= 20 and voiced.mean() >= 0.9
        assert cents[voiced].max() <= 50.0


def _loader(tmp_path, resyn):
    lines = []
    for i, dur in enumerate((2.0, 3.0, 0.9, 2.6)):
        sr = 16000 if i == 2 else 24000                       # one base file at another rate: resampled first
        n, f = int(dur * sr), 110.0 + 37.0 * i
        t = np.arange(n) / sr
        wave = sum(0.3 / h * np.sin(2 * np.pi * h * f * t + h) for h in (1, 2, 3)).astype(np.float32)
        p = tmp_path / f"u{i}.wav"
        if not p.exists():
            write_wav(p, wave, sr, "float32")
            np.save(str(p) + "_f0.npy", np.full(1 + int(dur * 24000) // 300, f, np.float32))
        lines.append(f"{p}|0\n")
    syn = {"enabled": True, "absolute_count": 8, "apply_to_validation": True,
           "pitch_shift": {"enabled": True, "semitones": [-2, 1, 4], "gain_db_range": [-6.0, 3.0]},
           "world_vocoder": {"enabled": True, "backend": "hip", "duration": {"min": 0.6, "max": 1.2}}}
    if resyn is not None:
        syn["world_resynthesis"] = resyn
    cfg = {"mel_params": {"sample_rate": 24000, "win_len": 1024, "n_fft": 1024, "n_mels": 80, "hop_length": 300},
           "dataloader": {"start_method": None}, "verbose": False, "synthetic_data": syn}
    return md.build_dataloader(lines, validation=True, batch_size=6, num_workers=0, device="cuda:0",
                               dataset_config=cfg)


def test_dataloader_with_resynthesis_items(tmp_path, hip_device):
    """Rows of resynthesized items equal the log-mel of ``resynthesize_ragged`` on the item's own request, bit for bit;
    labels and silences are the request's.  With the block absent or disabled the batches are the same bits."""
    resyn = {"enabled": True, "backend": "hip", "semitones": [-3, 2, 5], "noise_db": -55.0, "aperiodicity": 0.1,
             "modulation": {"vibrato_probability": 0.5}}
    loader = _loader(tmp_path, resyn)
    ds = loader.dataset
    assert ds._synthetic_generators == ["pitch_shift", "world_vocoder", "world_resynthesis"]
    assert len(ds) == 12 and len(loader) == 2
    np.random.seed(13); random.seed(13)
    got = [(m, f.cpu().numpy(), s.cpu().numpy()) for m, f, s in loader]
    np.random.seed(13); random.seed(13)
    cfg = ds.synthetic_resynthesis_config
    ap = torch.full((513,), cfg["aperiodicity"], device=hip_device)
    n_resyn = n_crop = n_rate = 0
    for bi in range(2):
        m, f, s = got[bi]
        assert tuple(m.shape) == (6, 1, 80, 192) and torch.isfinite(m).all()
        for k, i in enumerate(range(6 * bi, 6 * bi + 6)):
            if i < 4:
                ds.path_to_wave_and_label(ds.data_list[i])         # consume the item's draws
                continue
            item = ds[i]
            req = item[-1]
            if not isinstance(req, md.ResynthesisRequest):
                continue
            n_resyn += 1
            n_crop += req.crop > 0
            n_rate += item[4] != 24000
            src = item[0].to(hip_device)
            if item[4] != 24000:
                src = loader._ragged(src, [item[4]], [src.numel()])[0][0, :req.n].contiguous()
            waves = torch.zeros((1, req.out_len), device=hip_device)
            _, labels = world.resynthesize_ragged(
                src, [req.n], [req.base_curve], [req.curve], 24000, cfg["frame_period"], ap=ap, seeds=[req.seed],
                gains=torch.tensor([req.gain], dtype=torch.float32), out=waves, out_start=[req.out_start],
                out_len=[req.out_len], out_noise=torch.from_numpy(req.noise).to(hip_device), q1=cfg["q1"],
                fft_size=cfg["fft_size"])
            np.testing.assert_array_equal(labels[0], req.curve)
            i32 = lambda v: torch.tensor([v], dtype=torch.int32, device=hip_device)  # noqa: E731
            want = ds.to_melspec.log_mel_ragged(waves, i32(req.out_len), i32(req.frame_start), max_frames=192)
            assert torch.equal(m[k], want[0]), (bi, k)
            label = md.align_length(req.curve.astype(np.float32), 1 + req.n // 300)[req.crop:req.crop + 192]
            np.testing.assert_array_equal(f[k, :label.size], label)
            np.testing.assert_array_equal(s[k, :label.size], (label == 0).astype(np.float32))
            assert (f[k, label.size:] == 0).all()
    assert n_resyn >= 2 and n_crop >= 1 and n_rate >= 1
    # absent or disabled: the same bits
    batches = []
    for block in (None, {**resyn, "enabled": False}):
        off = _loader(tmp_path, block)
        assert off.dataset._synthetic_generators == ["pitch_shift", "world_vocoder"]
        np.random.seed(13); random.seed(13)
        batches.append([tuple(t.cpu() for t in b) for b in off])
    for a, b in zip(*batches):
        for u, v in zip(a, b):
            assert torch.equal(u, v)

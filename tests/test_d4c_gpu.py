"""WORLD D4C on the GPU against the float64 restatement (tests/d4c_ref.py), with the float32 restatement as the
yardstick (the project's rule for float32 kernels: 4 x its own deviation from float64, per configuration): a0
absolutely, the bands' coarse aperiodicity in dB, the expanded aperiodicity in the 20 log10 domain; equal verdicts on
every frame outside the stated margins; bit identity of ragged batching and frame sub-ranges; the refusals; resynthesis
with ``ap="d4c"`` as the explicit chain and with the Praat-style tracker as a witness; and the data loader with
``aperiodicity: d4c``.  pyworld is not available: parity with its binary is unpinned.

Measured on the MI355X, ratio of the kernel's largest deviation from float64 to the float32 restatement's own over a
configuration's rows (a0, coarse dB, 20 log10 ap): 16 kHz / 5 ms 0.10, 0.61, 0.61; 24 kHz / 5 ms 0.11, 0.55, 0.55; 24
kHz / 12.5 ms at threshold 0 0.09, 0.50, 0.50; 48 kHz / 5 ms 0.14, 1.88, 1.90; 25 kHz / 10 ms 0.16, 0.45, 0.45 (the
deviations: 2e-7 in a0, 0.7e-4 to 4.3e-4 dB).  Frames outside the verdict comparison: 0 of 317 (162 at 25 kHz) at
threshold 0.85, 6 of 131 at threshold 0.  The tracker's worst frame on the resynthesized tone is 2.66 cents off."""
import random

import numpy as np
import pytest
import torch

from pitchextractor_amd import inference, stimuli
from pitchextractor_amd import meldataset as md
from pitchextractor_amd import world
from pitchextractor_amd.f0_tracker import PraatACTracker
from tests import cheaptrick_ref as ct
from tests import d4c_cases as dc
from tests import d4c_ref as d4
from tests.test_data_layer import write_wav

pytestmark = pytest.mark.gpu


def _run(cases, names, dev, cfg, padded=False, lead=0, **kw):
    """The named rows as one batch -> per row (ap (frames, bins), bands (frames, 1 + bands)).  ``lead``: a row of that
    many samples and no frames goes first, so the named rows start at that offset."""
    fs, fp, thr = cfg
    xs = [np.zeros(lead, np.float32)] * bool(lead) + [cases[n]["x"] for n in names]
    f0s = [np.zeros(0, np.float32)] * bool(lead) + [cases[n]["f0"].copy() for n in names]
    lengths = [len(x) for x in xs]
    if padded:
        x = torch.zeros((len(xs), max(lengths) + 3), dtype=torch.float32)
        for r, a in enumerate(xs):
            x[r, :len(a)] = torch.from_numpy(a.copy())
        x = x.to(dev)
    else:
        x = torch.from_numpy(np.concatenate(xs + [np.zeros(1, np.float32)])).to(dev)
    env, bands = world.d4c_ragged(x, lengths, f0s, fs, fp, threshold=thr, return_bands=True, **kw)
    bands = bands.cpu().numpy()
    ends = np.cumsum(env.counts)
    return [(env.row(r).cpu().numpy(), bands[ends[r] - env.counts[r]:ends[r]]) for r in range(len(f0s))][bool(lead):]


@pytest.mark.parametrize("cfg", dc.CONFIGS, ids=lambda c: f"fs{c[0]}-fp{c[1]}-thr{c[2]}")
def test_accuracy_against_the_restatement(hip_device, cfg):
    """Per configuration, one ragged launch: verdicts equal on every frame outside the margins (at most 10 % of the
    F0-voiced frames lie inside); |a0 - float64|, |coarse - float64| in dB and |20 log10 ap - 20 log10 float64| at most
    4 x the float32 restatement's own largest deviation on the configuration's rows."""
    fs, fp, thr = cfg
    cases = dc.cases(cfg)
    names = list(cases)
    const = d4.constants(fs)
    bins = ct.default_fft_size(fs) // 2 + 1
    got = _run(cases, names, hip_device, cfg)
    db = lambda a: 20.0 * np.log10(np.asarray(a, dtype=np.float64))  # noqa: E731
    yard = {"a0": 0.0, "coarse": 0.0, "ap": 0.0}
    err = dict(yard)
    n_voiced = n_out = 0
    for name, (ap, band) in zip(names, got):
        c = cases[name]
        assert ap.shape == c["ap64"].shape == (c["f0"].size, bins) and ap.dtype == np.float32
        assert band.shape == c["b64"].shape == (c["f0"].size, 1 + const["bands"])
        assert np.isfinite(ap).all() and (ap > 0).all() and (ap <= 1).all()
        ex = dc.excluded_frames(cases, c, cfg)
        n_voiced += int((c["f0"] > 0).sum())
        n_out += int(ex.sum())
        u64, u32, ugpu = (np.isnan(b[:, 1]) for b in (c["b64"], c["b32"], band))
        assert (ugpu == u64)[~ex].all(), (name, np.flatnonzero((ugpu != u64) & ~ex))
        assert (band[~(c["f0"] > 0), 0] == 0).all() and (ap[ugpu] == 1.0).all()
        yard["a0"] = max(yard["a0"], np.abs(c["b32"][:, 0] - c["b64"][:, 0]).max(initial=0.0))
        err["a0"] = max(err["a0"], np.abs(band[:, 0] - c["b64"][:, 0])[~ex].max(initial=0.0))
        ok32, okg = ~u64 & ~u32, ~u64 & ~ugpu & ~ex
        yard["coarse"] = max(yard["coarse"], np.abs(c["b32"][ok32, 1:] - c["b64"][ok32, 1:]).max(initial=0.0))
        err["coarse"] = max(err["coarse"], np.abs(band[okg, 1:] - c["b64"][okg, 1:]).max(initial=0.0))
        yard["ap"] = max(yard["ap"], np.abs(db(c["ap32"][ok32]) - db(c["ap64"][ok32])).max(initial=0.0))
        err["ap"] = max(err["ap"], np.abs(db(ap[okg]) - db(c["ap64"][okg])).max(initial=0.0))
    for k in yard:
        print(f"[d4c] fs {fs} fp {fp} thr {thr} {k}: gpu {err[k]:.3e} float32 restatement {yard[k]:.3e} ratio "
              f"{err[k] / yard[k]:.2f}")
    print(f"[d4c] fs {fs} fp {fp} thr {thr}: {n_voiced} F0-voiced frames, {n_out} outside the verdict comparison")
    assert n_out <= 0.1 * n_voiced
    for k in yard:
        assert err[k] <= 4 * yard[k], (k, err[k], yard[k])
    # the single-row form is the same launches
    k = names.index("glide_47_40")
    one = world.d4c(torch.from_numpy(cases[names[k]]["x"].copy()).to(hip_device), cases[names[k]]["f0"], fs, fp,
                    threshold=thr)
    np.testing.assert_array_equal(one.cpu().numpy(), got[k][0])


def _same(a, b):
    for u, v in zip(a, b):
        np.testing.assert_array_equal(u, v)


def test_bit_identity(hip_device):
    cfg = dc.CONFIGS[1]
    fs, fp, _ = cfg
    cases = dc.cases(cfg)
    bins = ct.default_fft_size(fs) // 2 + 1
    names = ["vowel_noise", "zeros", "quiet_after_loud", "glide_47_40", "one_frame", "unvoiced_stretches"]
    batch = _run(cases, names, hip_device, cfg)
    again = _run(cases, names, hip_device, cfg)                              # run twice
    for k, name in enumerate(names):
        _same(again[k], batch[k])
        _same(_run(cases, [name], hip_device, cfg)[0], batch[k])             # alone
        _same(_run(cases, [name], hip_device, cfg, lead=1001)[0], batch[k])  # packed at an odd sample offset
    padded = _run(cases, names, hip_device, cfg, padded=True)
    rev = _run(cases, names[::-1], hip_device, cfg)[::-1]                    # first becomes last
    for k in range(len(names)):
        _same(padded[k], batch[k])
        _same(rev[k], batch[k])
    # a frame sub-range is the slice of the full analysis
    sub = [(5, 9), (0, 0), (0, len(cases["quiet_after_loud"]["f0"])), (11, 1), (0, 1), (17, 30)]
    part = _run(cases, names, hip_device, cfg, frames=sub)
    for k, (first, count) in enumerate(sub):
        assert part[k][0].shape[0] == part[k][1].shape[0] == count
        _same(part[k], (batch[k][0][first:first + count], batch[k][1][first:first + count]))
    # out= at a larger stride and odd offsets: the same bits, nothing else written
    stride = bins + 5
    counts = [len(cases[n]["f0"]) for n in names]
    offs = np.cumsum([3] + [c * stride for c in counts])[:-1]
    buf = torch.full((int(offs[-1] + counts[-1] * stride),), -7.0, device=hip_device)
    wide = _run(cases, names, hip_device, cfg, out=buf, out_offsets=offs, out_strides=[stride] * len(names))
    for k in range(len(names)):
        _same(wide[k], batch[k])
    host = buf.cpu().numpy()
    assert (host[:3] == -7.0).all()
    for off, cnt in zip(offs, counts):
        gaps = host[off:off + cnt * stride].reshape(cnt, stride)[:, bins:]
        assert (gaps == -7.0).all()


def test_refusals(hip_device):
    x = torch.zeros(2400, device=hip_device)
    f0 = np.full(8, 120.0, np.float32)
    with pytest.raises(Exception, match="unsupported"):
        world.d4c(torch.zeros(800, device=hip_device), f0, 8000, 5.0)
    with pytest.raises(Exception, match="unsupported"):
        world.d4c(x, f0, 50000, 5.0, fft_size=2048)
    with pytest.raises(ValueError, match="fft_size"):
        world.d4c(x, f0, 24000, 5.0, fft_size=4096)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        world.d4c(x.double(), f0, 24000, 5.0)
    with pytest.raises(ValueError, match="one F0 curve per row"):
        world.d4c_ragged(x, [1200, 1200], [f0], 24000, 5.0)
    with pytest.raises(ValueError, match="smaller"):
        world.d4c_ragged(x, [2400], [f0], 24000, 5.0, out=torch.zeros(100, device=hip_device))
    with pytest.raises(Exception, match="invalid argument"):                  # frames beyond the curve
        world.d4c_ragged(x, [2400], [f0], 24000, 5.0, frames=[(4, 8)])
    with pytest.raises(ValueError, match="threshold"):
        world.d4c(x, f0, 24000, 5.0, threshold=float("nan"))
    # a host plan that is not the plan's: the entry points refuse before any launch
    from pitchextractor_amd import _lib
    lib = _lib.load()
    meta = np.array([[0, 2400, 0, 0, 8, 3, 0, 513]], np.int64)                 # a frame prefix that is not 0
    meta_d = torch.from_numpy(meta).to(hip_device)
    f0_d = torch.from_numpy(f0).to(hip_device)
    band = torch.zeros((8, 4), device=hip_device)
    out = torch.zeros(8 * 513, device=hip_device)
    table = world._d4c_table(2048, 2048, hip_device)
    with pytest.raises(Exception, match="invalid argument"):
        _lib.check(lib.pe_d4c_bands(x.data_ptr(), f0_d.data_ptr(), meta_d.data_ptr(), meta.ctypes.data,
                                    table.data_ptr(), 1, 24000.0, 5.0, 0.85, 1024, band.data_ptr(), None), "pe_d4c_bands")
    with pytest.raises(Exception, match="invalid argument"):
        _lib.check(lib.pe_d4c_expand(band.data_ptr(), meta_d.data_ptr(), meta.ctypes.data, 1, 24000.0, 1024,
                                     out.data_ptr(), None), "pe_d4c_expand")
    with pytest.raises(ValueError, match="not a mode"):
        world.resynthesize(x, f0, f0, 24000, 5.0, ap="harvest")


def test_resynthesis_with_d4c_is_the_explicit_chain(hip_device):
    """``resynthesize(..., ap="d4c")`` = ``world_synthesize`` fed with ``cheaptrick`` and ``d4c`` of the same frames;
    ``ap=None`` and a tensor ``ap`` are the chains they were; windows analyse only the frames they read."""
    cfg = dc.CONFIGS[2]
    fs, fp, _ = cfg
    cases = dc.cases(cfg)
    c = cases["vowel_noise"]
    x = torch.from_numpy(c["x"].copy()).to(hip_device)
    f0 = c["f0"]
    new = f0 * np.float32(2 ** (3 / 12))
    sp = world.cheaptrick(x, f0, fs, fp)
    label = world.label_curve(new, fs, 1024)
    for thr in (0.0, 0.85):
        ap = world.d4c(x, f0, fs, fp, threshold=thr)
        assert ap.shape == sp.shape
        want = world.world_synthesize(label, sp, ap, fs, fp, seed=11)
        got, lab = world.resynthesize(x, f0, new, fs, fp, ap="d4c", seed=11, d4c_threshold=thr)
        np.testing.assert_array_equal(lab, label)
        assert torch.equal(got, want) and torch.isfinite(got).all() and got.abs().max() > 0.05
    assert not torch.equal(got, world.resynthesize(x, f0, new, fs, fp, seed=11)[0])
    # None and a template: the chains they were
    tmpl = torch.full((513,), 0.3, device=hip_device)
    for a in (None, tmpl):
        got, _ = world.resynthesize(x, f0, new, fs, fp, ap=a, seed=11)
        assert torch.equal(got, world.world_synthesize(label, sp, a, fs, fp, seed=11))
    # ragged, with windows: the rows' windows of the whole-row result
    names = ["vowel_noise", "quiet_after_loud", "unvoiced_stretches"]
    xs = [cases[n]["x"] for n in names]
    f0s = [cases[n]["f0"] for n in names]
    news = [np.where(np.isnan(f), 0, f) * np.float32(2 ** (-2 / 12)) for f in f0s]
    xx = torch.from_numpy(np.concatenate(xs)).to(hip_device)
    lengths = [len(a) for a in xs]
    seeds = [3, 2 ** 63 + 5, 7]
    full, _ = world.resynthesize_ragged(xx, lengths, f0s, news, fs, fp, ap="d4c", seeds=seeds, d4c_threshold=0.0)
    starts, lens = [0, 1500, 700], [3000, 2000, 1111]
    part, _ = world.resynthesize_ragged(xx, lengths, f0s, news, fs, fp, ap="d4c", seeds=seeds, d4c_threshold=0.0,
                                        out_start=starts, out_len=lens)
    for r in range(3):
        assert torch.equal(part[r, :lens[r]], full[r, starts[r]:starts[r] + lens[r]])


def test_resynthesized_tone_with_d4c_is_tracked_on_its_label(hip_device):
    """tests/test_cheaptrick_gpu.py's witness with the estimated aperiodicity: a "Bright Belt" 220 Hz tone complex
    resynthesized 3 semitones up with ``ap="d4c"``, ``d4c_threshold=0.0``, tracked by the Praat-style tracker: voiced on
    every compared frame and within that test's 50 cents of the label."""
    fs, hop, fp = 24000, 300, 12.5
    tone = stimuli.timbre_tones([220.0], {"Bright Belt": stimuli.TIMBRE_PROFILES["Bright Belt"]}, duration=0.4, sr=fs,
                                device=hip_device)
    x = tone.rows()[0]
    L = 1 + x.numel() // hop
    f0 = np.full(L, 220.0)
    new = f0 * 2 ** (3 / 12)
    wave, label = world.resynthesize(x, f0, new, fs, fp, ap="d4c", d4c_threshold=0.0)
    np.testing.assert_array_equal(label, new)
    got = inference.track_f0(wave, sr=fs, hop_length=hop).astype(np.float64)
    times = PraatACTracker(fs, hop).frame_times(wave.numel())
    want = np.interp(times, np.arange(L) * (fp / 1000.0), label)
    frame = times / (fp / 1000.0)
    keep = (frame >= 3) & (frame <= L - 1 - 3)
    voiced = got[keep] > 0
    cents = 1200.0 * np.abs(np.log2(np.maximum(got[keep], 1e-5) / want[keep]))
    print(f"[d4c] tone 3 semitones up: {int(keep.sum())} frames, voiced {voiced.mean():.2f}, worst "
          f"{cents[voiced].max():.2f} cents")
    assert keep.sum() >= 20 and voiced.all()
    assert cents.max() <= 50.0


def _loader(tmp_path, mode):
    """Six listed files (one at another rate) and two ``world_resynthesis`` items: one batch of 8."""
    lines = []
    for i, dur in enumerate((1.0, 1.5, 0.9, 2.6, 0.7, 1.2)):
        sr = 16000 if i == 2 else 24000                       # one base file at another rate: resampled first
        n, f = int(dur * sr), 110.0 + 37.0 * i
        t = np.arange(n) / sr
        rng = np.random.default_rng(i)
        wave = (sum(0.3 / h * np.sin(2 * np.pi * h * f * t + h) for h in (1, 2, 3, 4, 5)) +
                0.01 * rng.standard_normal(n)).astype(np.float32)
        p = tmp_path / f"u{i}.wav"
        if not p.exists():
            write_wav(p, wave, sr, "float32")
            np.save(str(p) + "_f0.npy", np.full(1 + int(dur * 24000) // 300, f, np.float32))
        lines.append(f"{p}|0\n")
    syn = {"enabled": True, "absolute_count": 2, "apply_to_validation": True, "pitch_shift": {"enabled": False},
           "world_resynthesis": {"enabled": True, "backend": "hip", "semitones": [-3, 2, 5], "noise_db": -55.0,
                                 "aperiodicity": mode, "modulation": {"vibrato_probability": 0.5}}}
    cfg = {"mel_params": {"sample_rate": 24000, "win_len": 1024, "n_fft": 1024, "n_mels": 80, "hop_length": 300},
           "dataloader": {"start_method": None}, "verbose": False, "synthetic_data": syn}
    return md.build_dataloader(lines, validation=True, batch_size=8, num_workers=0, device="cuda:0",
                               dataset_config=cfg)


def test_dataloader_with_d4c_aperiodicity(tmp_path, hip_device):
    """A B = 8 batch with two resynthesis rows and ``aperiodicity: d4c`` equals the stage run by hand on the items' own
    requests, bit for bit; the same dataset with ``aperiodicity: 0.1`` is the constant-template chain it was, and the
    two modes' items are the same draws."""
    rows = {}
    for mode in ("d4c", 0.1):
        loader = _loader(tmp_path, mode)
        ds = loader.dataset
        assert ds._synthetic_generators == ["world_resynthesis"] and len(ds) == 8 and len(loader) == 1
        np.random.seed(13); random.seed(13)
        (m, f, s), = [(m, f.cpu().numpy(), s.cpu().numpy()) for m, f, s in loader]
        np.random.seed(13); random.seed(13)
        cfg = ds.synthetic_resynthesis_config
        assert cfg["aperiodicity"] == mode and cfg["d4c_threshold"] == 0.0
        ap = "d4c" if mode == "d4c" else torch.full((513,), mode, device=hip_device)
        rows[mode] = (m[6:].clone(), f[6:], s[6:])
        n_resyn = 0
        for i in range(8):
            if i < 6:
                ds.path_to_wave_and_label(ds.data_list[i])             # consume the item's draws
                continue
            item = ds[i]
            req = item[-1]
            assert isinstance(req, md.ResynthesisRequest)
            n_resyn += 1
            src = item[0].to(hip_device)
            if item[4] != 24000:
                src = loader._ragged(src, [item[4]], [src.numel()])[0][0, :req.n].contiguous()
            waves = torch.zeros((1, req.out_len), device=hip_device)
            world.resynthesize_ragged(
                src, [req.n], [req.base_curve], [req.curve], 24000, cfg["frame_period"], ap=ap, seeds=[req.seed],
                gains=torch.tensor([req.gain], dtype=torch.float32), out=waves, out_start=[req.out_start],
                out_len=[req.out_len], out_noise=torch.from_numpy(req.noise).to(hip_device), q1=cfg["q1"],
                fft_size=cfg["fft_size"], d4c_threshold=0.0)
            i32 = lambda v: torch.tensor([v], dtype=torch.int32, device=hip_device)  # noqa: E731
            want = ds.to_melspec.log_mel_ragged(waves, i32(req.out_len), i32(req.frame_start), max_frames=192)
            assert torch.equal(m[i], want[0]), (mode, i)
        assert n_resyn == 2
    # the mode changes the audio and nothing else: labels and silences are the same draws
    assert not torch.equal(rows["d4c"][0], rows[0.1][0])
    np.testing.assert_array_equal(rows["d4c"][1], rows[0.1][1])
    np.testing.assert_array_equal(rows["d4c"][2], rows[0.1][2])

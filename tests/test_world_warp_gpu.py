"""Voice transforms of WORLD frames on the GPU (csrc/world_warp.hip, ``world.warp_envelopes``, ``resynthesize(...,
transform=)``) against the float64 restatement (tests/world_warp_ref.py) with the float32 restatement as the yardstick
(the project's rule for float32 kernels: 4 x its own deviation from float64, ln sp and ap measured apart); identity as a
bit copy; bit identity of ragged batching; the resynthesis chain with the Praat-style tracker as an independent witness;
and the data loader with the ``world_resynthesis.transform`` block on.

Which test catches which mistake (tests/test_world_warp_cpu.py shows, on the rows of the accuracy test, that the first
two put ln sp hundreds of times past the bound asserted here): warping with alpha in place of 1 / alpha and
interpolating sp linearly fail ``test_accuracy_against_the_restatement``; positions that run past the last source frame
(a dropped clamp) are refused by the plan, which fails ``test_accuracy_against_the_restatement`` (its rows end on clamped
frames), ``test_resynthesized_vowel_is_tracked_on_its_label`` (rate 0.8) and ``test_positions_past_the_last_frame``.

Measured on the MI355X, max deviation of the kernel over that of the float32 restatement (ln sp, ap): 8 kHz / 257 bins
0.85, no ap; 24 kHz / 12.5 ms / 513 bins 0.74, 0.77; 48 kHz / 1025 bins 0.75, 0.73; 24 kHz / 5 ms with the time mix
alone 2.42, 0.94 (deviations 4e-6 to 5e-5 in ln sp, 8e-8 to 5e-7 in ap).  The tracker's worst frame off the label, in
cents, from one run: identity 2.59, formant 0.85 2.89, formant 1.2 2.33, rate 0.8 1.91, rate 1.25 3.51, all at once with
``ap="d4c"`` 2.05."""
import random

import numpy as np
import pytest
import torch

from pitchextractor_amd import inference
from pitchextractor_amd import meldataset as md
from pitchextractor_amd import world
from pitchextractor_amd.f0_tracker import PraatACTracker
from tests import world_warp_cases as wc
from tests.test_data_layer import write_wav

pytestmark = pytest.mark.gpu
VT = world.VoiceTransform


def _run(rows, positions, transforms, dev, fs, fft_size, lead=0, in_pad=0, out_pad=0, use_ap=True):
    """The rows (dicts with sp, ap) as one launch -> [(sp_out, ap_out or None)] per row.  ``lead``: floats before the
    first row (an odd offset); ``in_pad`` / ``out_pad``: floats between frames (strides wider than the bins); the
    output buffers are pre-filled with NaN, and what lies between the frames must still be NaN afterwards."""
    bins = fft_size // 2 + 1
    counts = np.array([len(c["sp"]) for c in rows], np.int64)
    stride = bins + in_pad
    offsets = lead + np.cumsum(counts * stride) - counts * stride

    def pack(key, shift):
        buf = np.full(int(shift + lead + (counts * stride).sum()) + 1, 0.5, np.float32)
        for c, o, n in zip(rows, offsets + shift, counts):
            view = buf[o:o + n * stride].reshape(n, stride)
            view[:, :bins] = c[key]
        return torch.from_numpy(buf).to(dev)
    first = np.zeros(len(rows), np.int64)
    env = world.Envelopes(pack("sp", 0), offsets, np.full(len(rows), stride), first, counts, fft_size)
    with_ap = use_ap and all(c["ap"] is not None for c in rows)
    ap = world.Envelopes(pack("ap", 5), offsets + 5, np.full(len(rows), stride), first, counts, fft_size) \
        if with_ap else None
    n_out = np.array([len(p) for p in positions], np.int64)
    o_stride = bins + out_pad
    o_off = 3 * bool(out_pad) + np.cumsum(n_out * o_stride) - n_out * o_stride
    out = torch.full((int(o_off[-1] + n_out[-1] * o_stride) + 1,), float("nan"), device=dev)
    got, ap_out = world.warp_envelopes(env, ap, positions, transforms, fs, out=out, out_offsets=o_off,
                                       out_strides=np.full(len(rows), o_stride))
    assert got.sp.data_ptr() == out.data_ptr() and (ap_out is None) == (ap is None)
    res = []
    written = torch.zeros_like(out, dtype=torch.bool)
    for r in range(len(rows)):
        sp_r = got.row(r)
        ap_r = None if ap_out is None else ap_out.as_strided(sp_r.shape, sp_r.stride(), int(got.offsets[r]))
        written.as_strided(sp_r.shape, sp_r.stride(), int(got.offsets[r])).fill_(True)
        res.append((sp_r.cpu().numpy(), None if ap_r is None else ap_r.cpu().numpy()))
    assert torch.isnan(out[~written]).all() and not torch.isnan(out[written]).any()
    return res


@pytest.mark.parametrize("cfg", wc.CONFIGS[:3], ids=wc.config_id)
def test_identity_is_a_copy(hip_device, cfg):
    """alpha 1, no tilt, whole positions: sp bit for bit (and ap without breath), at 257 / 513 / 1025 bins, into a
    wider stride; with breath alone sp is still the copy and ap is not."""
    fs, _, N = cfg[:3]
    rows = wc.cases(cfg)
    whole = [np.arange(len(c["sp"]), dtype=np.float64) for c in rows]
    same = VT(f_hi=wc.f_hi_of(cfg))
    for kw in (dict(), dict(lead=1001, in_pad=3, out_pad=7)):
        got = _run(rows, whole, [same] * len(rows), hip_device, fs, N, **kw)
        for c, (sp, ap) in zip(rows, got):
            np.testing.assert_array_equal(sp, c["sp"])
            if c["ap"] is not None:
                np.testing.assert_array_equal(ap, c["ap"])
    got = _run(rows, whole, [same, same._replace(breath=3.0), same._replace(f_hi=2000.0), same,
                             same._replace(breath=-3.0)], hip_device, fs, N)
    for r, (c, (sp, ap)) in enumerate(zip(rows, got)):
        np.testing.assert_array_equal(sp, c["sp"])
        if c["ap"] is not None and len(c["ap"]):
            assert np.array_equal(ap, c["ap"]) == (r in (0, 2, 3))
    # the last frame read twice, and frames read out of order, are copies too
    back = [np.arange(len(c["sp"]), dtype=np.float64)[::-1].copy() for c in rows]
    got = _run(rows, back, [same] * len(rows), hip_device, fs, N)
    for c, (sp, _) in zip(rows, got):
        np.testing.assert_array_equal(sp, c["sp"][::-1])


@pytest.mark.parametrize("cfg", wc.CONFIGS, ids=wc.config_id)
def test_accuracy_against_the_restatement(hip_device, cfg):
    """Per configuration, over its rows with no element left out: max |ln sp - ln float64| and max |ap - float64| of
    the kernel <= 4 x the float32 restatement's own, one ragged launch."""
    fs, fp, N, thr, rate, alpha, tilt, breath = cfg
    rows = wc.cases(cfg)
    t = VT(alpha, rate, tilt, breath, wc.f_hi_of(cfg))
    got = _run(rows, [c["pos"] for c in rows], [t] * len(rows), hip_device, fs, N, lead=7, out_pad=5)
    for c, (sp, ap) in zip(rows, got):
        assert sp.shape == c["sp64"].shape and sp.dtype == np.float32 and np.isfinite(sp).all() and (sp > 0).all()
        if ap is not None:
            assert ap.shape == c["ap64"].shape and (ap >= 0).all() and (ap <= 1).all()
    e_sp, e_ap = wc.deviations(rows, [g[0] for g in got], [g[1] for g in got])
    y_sp, y_ap = wc.yardsticks(cfg)
    print(f"[world_warp] {wc.config_id(cfg)} ln sp: gpu {e_sp:.3e} float32 restatement {y_sp:.3e} ratio "
          f"{e_sp / y_sp:.2f}")
    if thr is not None:
        print(f"[world_warp] {wc.config_id(cfg)} ap: gpu {e_ap:.3e} float32 restatement {y_ap:.3e} ratio "
              f"{e_ap / y_ap:.2f}")
    assert e_sp <= 4 * y_sp
    assert e_ap <= 4 * y_ap


def test_positions_past_the_last_frame(hip_device):
    cfg = wc.CONFIGS[1]
    rows = wc.cases(cfg)[:1]
    with pytest.raises(Exception, match="invalid argument"):
        _run(rows, [np.arange(8) * 1.25], [VT(rate=1.25)], hip_device, cfg[0], cfg[2])       # 7.5 and 8.75 > 6
    with pytest.raises(Exception, match="invalid argument"):
        _run(rows, [np.array([0.0, 1.0])], [VT(formant=2.5)], hip_device, cfg[0], cfg[2])


def test_row_independence(hip_device):
    """A row is bit-identical alone, at an odd offset, padded (wider strides in and out) and batched in two orders."""
    cfg = wc.CONFIGS[1]
    fs, N = cfg[0], cfg[2]
    rows = wc.cases(cfg)
    ts = [VT(0.8, 1.25, -3.0, 6.0), VT(1.25, 1.0, 0.0, 0.0), VT(1.0, 1.0, 0.0, 2.0), VT(), VT(1.1, 0.8, 1.5, -4.0)]
    pos = [wc.positions_for(len(c["sp"]), t.rate) for c, t in zip(rows, ts)]
    batch = _run(rows, pos, ts, hip_device, fs, N)
    rev = _run(rows[::-1], pos[::-1], ts[::-1], hip_device, fs, N)[::-1]
    padded = _run(rows, pos, ts, hip_device, fs, N, in_pad=11, out_pad=1)
    for k in range(len(rows)):
        alone = _run(rows[k:k + 1], pos[k:k + 1], ts[k:k + 1], hip_device, fs, N)[0]
        odd = _run(rows[k:k + 1], pos[k:k + 1], ts[k:k + 1], hip_device, fs, N, lead=1001)[0]
        for other in (alone, odd, rev[k], padded[k]):
            np.testing.assert_array_equal(other[0], batch[k][0])
            np.testing.assert_array_equal(other[1], batch[k][1])
        no_ap = _run(rows[k:k + 1], pos[k:k + 1], ts[k:k + 1], hip_device, fs, N, use_ap=False)[0]
        np.testing.assert_array_equal(no_ap[0], batch[k][0])
        assert no_ap[1] is None
    assert batch[3][0].shape == (0, N // 2 + 1)
    # one template for every row and frame: the read of a flat row
    tmpl = torch.linspace(0.05, 0.6, N // 2 + 1, device=hip_device)
    bins = N // 2 + 1
    env = world.Envelopes(torch.from_numpy(np.concatenate([rows[0]["sp"].reshape(-1), [0.0]]).astype(np.float32))
                          .to(hip_device), np.zeros(1, np.int64), np.full(1, bins), np.zeros(1, np.int64),
                          np.array([7]), N)
    _, ap = world.warp_envelopes(env, tmpl, [pos[0]], [VT(breath=6.0, rate=1.25)], fs)
    want = torch.clamp(tmpl.double() * 10.0 ** (6.0 / 20.0), 0, 1)
    assert torch.allclose(ap.reshape(len(pos[0]), bins).double(), want.expand(len(pos[0]), bins), rtol=1e-6)


# --------------------------------------------------------------------------- resynthesis
FS, HOP, FP, N = 24000, 300, 12.5, 1024


def _vowel(seconds=0.6, f0=140.0):
    """A harmonic complex with the formants of "ah" (amplitudes from the vowel generator's template) over a little
    noise, with its analytic curve."""
    n = int(seconds * FS)
    t = np.arange(n) / FS
    env = world.formant_templates(world.DEFAULT_VOWELS[:1], FS, N)[0]
    freq = np.arange(N // 2 + 1) * FS / N
    x = sum(np.sqrt(np.interp(h * f0, freq, env)) * np.sin(2 * np.pi * h * f0 * t + h) for h in range(1, int(0.45 * FS / f0)))
    x = 0.5 * x / np.abs(x).max() + 1e-3 * np.random.default_rng(0).standard_normal(n)
    return x.astype(np.float32), np.full(1 + n // HOP, f0)


def test_identity_transform_is_the_untransformed_resynthesis(hip_device):
    """``transform=VoiceTransform()`` goes through the kernel's copy and equals ``transform=None`` bit for bit: without
    ap, with a template, with the recording's own; and for cropped windows of a ragged batch."""
    x, f0 = _vowel()
    xd = torch.from_numpy(x).to(hip_device)
    new = f0 * 2 ** (2 / 12)
    new[:3] = 0.0
    tmpl = torch.full((N // 2 + 1,), 0.2, device=hip_device)
    for ap in (None, tmpl, "d4c"):
        a, la = world.resynthesize(xd, f0, new, FS, FP, ap=ap, seed=5)
        b, lb = world.resynthesize(xd, f0, new, FS, FP, ap=ap, seed=5, transform=VT())
        assert torch.equal(a, b) and a.abs().max() > 0.05
        np.testing.assert_array_equal(la, lb)
    xs = torch.cat([xd, xd[:9000]])
    kw = dict(ap="d4c", seeds=[1, 2], out_start=[2000, 0], out_len=[3000, 4000], d4c_threshold=0.0)
    f0s, news = [f0, f0[:31]], [new, new[:31]]
    a, _ = world.resynthesize_ragged(xs, [len(x), 9000], f0s, news, FS, FP, **kw)
    b, _ = world.resynthesize_ragged(xs, [len(x), 9000], f0s, news, FS, FP, transforms=[None, VT()], **kw)
    assert torch.equal(a, b) and a.abs().max() > 0.05


def test_resynthesized_vowel_is_tracked_on_its_label(hip_device):
    """The vowel resynthesized on a 150 -> 200 Hz glide with its formants at 0.85 and 1.2, at rate 0.8 and 1.25, and
    all of it at once with its own aperiodicity, tracked by ``inference.track_f0`` (praat).  Compared: frames at least 3
    frames inside the label (the tracker's window from the voicing boundary).  Conditions: voiced on >= 90 % of them
    and within 50 cents of the label."""
    x, f0 = _vowel()
    xd = torch.from_numpy(x).to(hip_device)
    worst = {}
    for tag, t, ap in (("identity", VT(), None), ("formant 0.85", VT(formant=0.85), None),
                       ("formant 1.2", VT(formant=1.2), None), ("rate 0.8", VT(rate=0.8), None),
                       ("rate 1.25", VT(rate=1.25), None), ("d4c", VT(1.2, 0.8, -2.0, 3.0), "d4c")):
        G = world.warped_frames(len(x), HOP, t.rate)
        assert G == {1.0: 49, 0.8: 61, 1.25: 39}[t.rate]
        new = np.linspace(150.0, 200.0, G)
        wave, label = world.resynthesize(xd, f0, new, FS, FP, ap=ap, transform=t, d4c_threshold=0.0)
        np.testing.assert_array_equal(label, new)
        assert wave.numel() == int(G * FP * FS / 1000) and torch.isfinite(wave).all()
        got = inference.track_f0(wave, sr=FS, hop_length=HOP).astype(np.float64)
        times = PraatACTracker(FS, HOP).frame_times(wave.numel())
        want = np.interp(times, np.arange(G) * (FP / 1000.0), label)
        frame = times / (FP / 1000.0)
        keep = (frame >= 3) & (frame <= G - 1 - 3)
        voiced = got[keep] > 0
        cents = 1200.0 * np.abs(np.log2(np.maximum(got[keep], 1e-5) / want[keep]))
        worst[tag] = float(cents[voiced].max())
        print(f"[world_warp] {tag}: {int(keep.sum())} frames, voiced {voiced.mean():.2f}, worst {worst[tag]:.2f} cents "
              f"(identity: {worst['identity']:.2f})")
        assert keep.sum() >= 25 and voiced.mean() >= 0.9
        assert worst[tag] <= 50.0
    # the formants did move: the envelope's centroid below 4 kHz goes more than half of the way alpha asks for
    sp = world.cheaptrick(xd, f0, FS, FP)
    env = world.Envelopes(sp.reshape(-1), np.zeros(1, np.int64), np.full(1, 513), np.zeros(1, np.int64),
                          np.array([len(f0)]), N)
    k = torch.arange(171, device=hip_device, dtype=torch.float32)            # bins below 4 kHz
    centroid = lambda e: float((e[10:40, :171] * k).sum() / e[10:40, :171].sum())  # noqa: E731
    c1 = centroid(sp)
    for alpha in (0.85, 1.2):
        w, _ = world.warp_envelopes(env, None, [np.arange(len(f0), dtype=np.float64)], [VT(formant=alpha)], FS)
        assert (centroid(w.row(0)) / c1 - 1.0) / (alpha - 1.0) > 0.5


# --------------------------------------------------------------------------- the loader
def _loader(tmp_path, transform):
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
    resyn = {"enabled": True, "backend": "hip", "semitones": [-3, 2, 5], "noise_db": -55.0, "aperiodicity": "d4c",
             "modulation": {"vibrato_probability": 0.5}}
    if transform is not None:
        resyn["transform"] = transform
    cfg = {"mel_params": {"sample_rate": 24000, "win_len": 1024, "n_fft": 1024, "n_mels": 80, "hop_length": 300},
           "dataloader": {"start_method": None}, "verbose": False,
           "synthetic_data": {"enabled": True, "absolute_count": 4, "apply_to_validation": True,
                              "pitch_shift": {"enabled": False}, "world_resynthesis": resyn}}
    return md.build_dataloader(lines, validation=True, batch_size=8, num_workers=0, device="cuda:0",
                               dataset_config=cfg)


def test_dataloader_with_transformed_items(tmp_path, hip_device):
    """A B = 8 batch with 4 resynthesis rows and the block on: every such row is the log-mel of ``resynthesize_ragged``
    on the item's own request with its transform, bit for bit; its labels are the request's curve, which is
    ``label_curve`` of itself; the waves are finite; and the batch differs from the one without the block."""
    block = {"probability": 1.0, "formant_ratio_range": [0.85, 1.2], "rate_range": [0.8, 1.25],
             "tilt_db_per_octave_range": [-3.0, 3.0], "breath_db_range": [-3.0, 6.0]}
    loader = _loader(tmp_path, block)
    ds = loader.dataset
    assert ds._synthetic_generators == ["world_resynthesis"] and len(ds) == 8 and len(loader) == 1
    np.random.seed(13); random.seed(13)
    (m, f, s), = [(m, f.cpu().numpy(), s.cpu().numpy()) for m, f, s in loader]
    assert tuple(m.shape) == (8, 1, 80, 192) and torch.isfinite(m).all()
    np.random.seed(13); random.seed(13)
    cfg = ds.synthetic_resynthesis_config
    rates = set()
    for i in range(8):
        if i < 4:
            ds.path_to_wave_and_label(ds.data_list[i])             # consume the item's draws
            continue
        item = ds[i]
        req = item[-1]
        assert isinstance(req, md.ResynthesisRequest) and req.transform is not None
        t = VT(*req.transform)
        rates.add(t.rate > 1)
        n_out = world.warped_length(req.n, t.rate)
        np.testing.assert_array_equal(req.curve, world.label_curve(req.curve, 24000, cfg["fft_size"]))
        assert req.curve.size == 1 + n_out // 300 == req.positions.size
        src = item[0].to(hip_device)
        if item[4] != 24000:
            src = loader._ragged(src, [item[4]], [src.numel()])[0][0, :req.n].contiguous()
        waves = torch.zeros((1, req.out_len), device=hip_device)
        _, labels = world.resynthesize_ragged(
            src, [req.n], [req.base_curve], [req.curve], 24000, cfg["frame_period"], ap="d4c", seeds=[req.seed],
            gains=torch.tensor([req.gain], dtype=torch.float32), out=waves, out_start=[req.out_start],
            out_len=[req.out_len], out_noise=torch.from_numpy(req.noise).to(hip_device), q1=cfg["q1"],
            fft_size=cfg["fft_size"], d4c_threshold=0.0, transforms=[t], positions=[req.positions])
        np.testing.assert_array_equal(labels[0], req.curve)
        assert torch.isfinite(waves).all() and waves.abs().max() > 0.01
        i32 = lambda v: torch.tensor([v], dtype=torch.int32, device=hip_device)  # noqa: E731
        want = ds.to_melspec.log_mel_ragged(waves, i32(req.out_len), i32(req.frame_start), max_frames=192)
        assert torch.equal(m[i], want[0]), i
        label = md.align_length(req.curve.astype(np.float32), 1 + n_out // 300)[req.crop:req.crop + 192]
        np.testing.assert_array_equal(f[i, :label.size], label)
        np.testing.assert_array_equal(s[i, :label.size], (label == 0).astype(np.float32))
    assert len(rates) == 2                                        # a slower and a faster item
    plain = _loader(tmp_path, None)
    np.random.seed(13); random.seed(13)
    (m0, f0, _), = list(plain)
    assert torch.equal(m0[:4], m[:4]) and not torch.equal(m0[4:], m[4:])
    assert not np.array_equal(f0.cpu().numpy()[4:], f[4:])
    off = _loader(tmp_path, {**block, "probability": 0})
    np.random.seed(13); random.seed(13)
    (m1, f1, s1), = list(off)
    assert torch.equal(m1, m0) and torch.equal(f1, f0)

"""WORLD-vocoder synthesis on the GPU against the float64 restatement (tests/world_ref.py): the responses stage, end
to end with the float32 restatement as the yardstick, bit identity of ragged batching, the window form, the default
noise, the tracker as an independent witness, and the data loader with WORLD items on.  24 kHz, hop 300, N = 1024;
every row gets its pulse table from the product's ``time_base`` and an explicit noise.

Measured end to end on the MI355X, max |gpu - float64| per row with the float32 restatement's in brackets (peaks 0.2
to 0.6): two 2.2e-07 (9.9e-08), glide_vib 3.2e-07 (2.5e-07), hi 1.2e-07 (1.1e-07), morph 3.1e-07 (3.1e-07), gap
2.9e-07 (3.0e-07); a single response is at worst 2.7e-07 off (morph).  N = 512: 2.9e-07 (2.9e-07), N = 2048: 3.3e-07
(2.1e-07).  The tracker's worst frame on the glide is 6.1 cents off the drawn curve."""
import random

import numpy as np
import pytest
import torch

from oracle import mel_ref, train_ref
from pitchextractor_amd import inference
from pitchextractor_amd import meldataset as md
from pitchextractor_amd import world
from pitchextractor_amd.f0_tracker import PraatACTracker
from tests import world_ref as ref
from tests.test_data_layer import write_wav

pytestmark = pytest.mark.gpu
FS, HOP, N, FP = ref.FS, ref.HOP, ref.FFT, ref.FRAME_PERIOD
BINS = N // 2 + 1
NAMES = ["two", "glide_vib", "hi", "morph", "gap"]


@pytest.fixture(scope="module")
def cases():
    """name -> dict(f0, sp, ap, table, noise, f64, f32, resp64): computed once, never modified."""
    out = {}
    rng = np.random.default_rng(11)
    for name, (f0, sp, ap) in ref.rows().items():
        table = world.time_base(f0, FS, FP, N)
        n = world.output_length(f0.size, FS, FP)
        noise = rng.standard_normal(n).astype(np.float32)
        sp32 = sp.astype(np.float32)
        ap32 = None if ap is None else ap.astype(np.float32)
        args = (f0.size, sp32.astype(np.float64), None if ap32 is None else ap32.astype(np.float64), FS, FP, *table,
                noise.astype(np.float64))
        resp64 = ref.responses(*args)
        resp32 = ref.responses(*args, fp32=True)
        out[name] = dict(f0=f0, sp=sp32, ap=ap32, table=table, noise=noise, n=n, resp64=resp64,
                         f64=ref.overlap_add(resp64, table.index, n), f32=ref.overlap_add(resp32, table.index, n))
        for v in out[name].values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return out


def _batch(cases, names, dev, tile=(), zero_ap=(), out_start=None, out_len=None, out_rows=None, out=None, gains=None,
           out_noise=None, keep=False):
    """Run rows as one ragged batch.  ``tile``: rows whose one-template sp is tiled to (L, 513); ``zero_ap``: rows
    that get an explicit all-zero ap.  Returns (plan, kept buffers, out as numpy)."""
    sps, aps, noises = [], [], []
    sp_off, sp_str, ap_off, ap_str, n_off = [], [], [], [], []
    so = ao = no = 0
    for nm in names:
        c = cases[nm]
        L = c["f0"].size
        sp = np.tile(c["sp"], (L, 1)) if (nm in tile and c["sp"].ndim == 1) else c["sp"]
        ap = np.zeros((L, BINS), np.float32) if nm in zero_ap else c["ap"]
        sps.append(sp.reshape(-1)); sp_off.append(so); sp_str.append(BINS if sp.ndim == 2 else 0); so += sp.size
        if ap is None:
            ap_off.append(-1); ap_str.append(0)
        else:
            aps.append(ap.reshape(-1)); ap_off.append(ao); ap_str.append(BINS if ap.ndim == 2 else 0); ao += ap.size
        noises.append(c["noise"]); n_off.append(no); no += c["noise"].size
    dv = lambda parts: torch.from_numpy(np.concatenate(parts)).to(dev) if parts else None  # noqa: E731
    R = len(names)
    plan = world.Plan([cases[nm]["f0"].size for nm in names], [cases[nm]["table"] for nm in names], sp_off, sp_str,
                      ap_off, ap_str, n_off, None, out_start, out_len, out_rows,
                      None if out is None else out.stride(0), fs=FS, frame_period_ms=FP, fft_size=N,
                      f0s=[cases[nm]["f0"] for nm in names])
    if out is None:
        out = torch.zeros((R, plan.out_stride), dtype=torch.float32, device=dev)
    g = torch.ones(R, dtype=torch.float32, device=dev) if gains is None else gains
    kept = world.WorldSynth().run(plan, dv(sps), dv(aps), g, out, dv(noises), out_noise, keep=keep)
    torch.cuda.synchronize()
    return plan, kept, out.cpu().numpy()


def test_responses_stage(hip_device, cases):
    plan, kept, _ = _batch(cases, NAMES, hip_device, keep=True)
    resp = kept["responses"].cpu().numpy()
    assert plan.n_pulses == sum(cases[nm]["table"].index.size for nm in NAMES)
    lo = 0
    for nm in NAMES:
        want = cases[nm]["resp64"]
        got = resp[lo:lo + want.shape[0]]
        lo += want.shape[0]
        err = np.abs(got - want).max(axis=1)
        print(f"[world] responses {nm}: pulses {want.shape[0]} worst {err.max():.3e} of peak {np.abs(want).max():.3e}")
        assert np.isfinite(got).all()
        assert (err <= 1e-5 * np.abs(want).max()).all(), (nm, err.max(), np.abs(want).max())
    c = cases["two"]
    assert c["table"].noise_size[-1] == 0 and c["table"].index.size == 2
    assert c["table"].index[0] < N // 2 - 1 and c["table"].index[-1] + N // 2 > c["n"]      # both clipped at an end


def test_end_to_end_within_twice_float32(hip_device, cases):
    _, _, out = _batch(cases, NAMES, hip_device)
    for r, nm in enumerate(NAMES):
        c = cases[nm]
        got = out[r, :c["n"]]
        e_gpu, e_32 = np.abs(got - c["f64"]).max(), np.abs(c["f32"] - c["f64"]).max()
        print(f"[world] end to end {nm}: e_gpu {e_gpu:.3e} e_32 {e_32:.3e} peak {np.abs(c['f64']).max():.3f}")
        assert e_gpu <= 2 * e_32 + 1e-5, (nm, e_gpu, e_32)
        if c["n"] > 1024:
            m64, m32, mg = (mel_ref.log_mel(np.asarray(x, np.float64)) for x in (c["f64"], c["f32"], got))
            assert np.abs(mg - m64).max() <= 2 * np.abs(m32 - m64).max() + 1e-3, nm


def test_bit_identity(hip_device, cases):
    _, _, batch = _batch(cases, NAMES, hip_device)
    for nm in ("two", "hi", "morph"):
        c = cases[nm]
        _, _, alone = _batch(cases, [nm], hip_device)
        np.testing.assert_array_equal(alone[0, :c["n"]], batch[NAMES.index(nm), :c["n"]])
        dev = lambda a: None if a is None else torch.tensor(a, device=hip_device)  # noqa: E731
        got = world.world_synthesize(c["f0"], dev(c["sp"]), dev(c["ap"]), FS, FP, noise=dev(c["noise"])).cpu().numpy()
        np.testing.assert_array_equal(got, alone[0, :c["n"]])
    for nm in ("hi", "gap"):                                   # one (513,) template == its (L, 513) tiling
        _, _, a = _batch(cases, [nm], hip_device)
        _, _, b = _batch(cases, [nm], hip_device, tile=(nm,))
        np.testing.assert_array_equal(a, b)
        _, _, z = _batch(cases, [nm], hip_device, zero_ap=(nm,))    # ap=None == explicit zeros
        np.testing.assert_array_equal(a, z)


def test_rows_split_over_launches(hip_device, cases, monkeypatch):
    """A batch whose responses pass the workspace limit runs in several launches and gives the same bits."""
    names = ["glide_vib", "two", "hi", "gap"]
    dv = lambda a: torch.from_numpy(np.concatenate(a)).to(hip_device)  # noqa: E731
    sp_off = np.arange(4) * BINS
    n_off = np.concatenate([[0], np.cumsum([cases[nm]["n"] for nm in names])[:-1]])
    outs = []
    for limit in (world.WORKSPACE_BYTES, 300 * N * 4):          # 109 + 2 | 409 | 107 pulses under the small limit
        monkeypatch.setattr(world, "WORKSPACE_BYTES", limit)
        out = torch.zeros((4, 12000), dtype=torch.float32, device=hip_device)
        world.world_synthesize_ragged([cases[nm]["f0"] for nm in names], dv([cases[nm]["sp"] for nm in names]), sp_off,
                                      [0] * 4, torch.tensor([1.0, 0.5, 2.0, 0.25]), out, fs=FS, frame_period=FP,
                                      fft_size=N, tables=[cases[nm]["table"] for nm in names],
                                      noise=dv([cases[nm]["noise"] for nm in names]), noise_offsets=n_off,
                                      out_noise=torch.arange(sum(cases[nm]["n"] for nm in names), dtype=torch.float32,
                                                             device=hip_device) * 1e-7)
        outs.append(out.cpu().numpy())
    np.testing.assert_array_equal(outs[0], outs[1])
    assert np.abs(outs[0][1, :600] - (0.5 * cases["two"]["f64"] + np.arange(12000, 12600) * 1e-7)).max() < 1e-6


def test_window_write_matches_full_row(hip_device):
    """The loader's form: output windows of a 3 s row, two gains and additive noise, written into given batch rows."""
    L = 240
    t = np.arange(L) * (FP / 1000.0)
    f0 = np.linspace(140.0, 260.0, L) * 2.0 ** (np.sin(2 * np.pi * 4.5 * t) * (0.3 / 12.0))
    table = world.time_base(f0, FS, FP, N)
    n = world.output_length(L, FS, FP)
    assert n == 72000
    sp = torch.from_numpy(ref.envelope("uh", FS, N).astype(np.float32)).to(hip_device)
    noise = torch.randn(n, device=hip_device)
    full = world.world_synthesize(f0, sp, None, FS, FP, noise=noise).cpu().numpy()
    W = 58412
    out = torch.zeros((3, 60000), dtype=torch.float32, device=hip_device)
    out_noise = torch.randn(2 * W, device=hip_device) * 1e-3
    both = torch.cat([noise, noise])
    world.world_synthesize_ragged([f0, f0], sp, [0, 0], [0, 0], torch.tensor([0.5, 2.0]), out, out_rows=[2, 0],
                                  out_start=[n - W, 0], out_len=[W, W], fs=FS, frame_period=FP, fft_size=N,
                                  tables=[table, table], noise=both, noise_offsets=[0, n], out_noise=out_noise)
    torch.cuda.synchronize()
    o, on = out.cpu().numpy(), out_noise.cpu().numpy()
    np.testing.assert_allclose(o[2, :W], np.float32(0.5) * full[n - W:] + on[:W], rtol=0, atol=1e-6)
    np.testing.assert_allclose(o[0, :W], np.float32(2.0) * full[:W] + on[W:], rtol=0, atol=1e-6)
    assert (o[1] == 0).all() and (o[0, W:] == 0).all() and (o[2, W:] == 0).all()
    plan = world.Plan([L], [table], [0], [0], out_start=[n - W], out_len=[W], fs=FS, frame_period_ms=FP, fft_size=N)
    assert 0 < plan.n_pulses < table.index.size


def test_default_noise(hip_device, cases):
    c = cases["morph"]
    dev = lambda a: torch.tensor(a, device=hip_device)  # noqa: E731
    sp, ap = dev(c["sp"]), dev(c["ap"])
    a = world.world_synthesize(c["f0"], sp, ap, FS, FP, seed=7)
    b = world.world_synthesize(c["f0"], sp, ap, FS, FP, seed=7)
    other = world.world_synthesize(c["f0"], sp, ap, FS, FP, seed=8)
    assert torch.equal(a, b) and not torch.equal(a, other)
    silent = world.world_synthesize(c["f0"], sp, ap, FS, FP, noise=torch.zeros(c["n"], device=hip_device))
    torch.manual_seed(3)
    given = world.world_synthesize(c["f0"], sp, ap, FS, FP, noise=torch.randn(c["n"], device=hip_device))
    rms = lambda x: float(torch.sqrt(torch.mean(x.double() ** 2)))  # noqa: E731
    drawn, explicit = rms(a - silent), rms(given - silent)
    print(f"[world] aperiodic rms: drawn {drawn:.3e} explicit {explicit:.3e}")
    assert explicit > 0 and 0.5 <= drawn / explicit <= 2.0


def test_tracker_follows_the_drawn_curve(hip_device):
    """Independent of the restatement: the Praat-style tracker on a synthesized 120-frame glide."""
    f0 = np.linspace(110.0, 320.0, 120)
    sp = torch.from_numpy(ref.envelope("ah", FS, N).astype(np.float32)).to(hip_device)
    wave = world.world_synthesize(f0, sp, None, FS, FP, seed=1)
    got = inference.track_f0(wave, sr=FS, hop_length=HOP)
    times = PraatACTracker(FS, HOP).frame_times(wave.numel())
    assert got.size == times.size > 100
    want = np.interp(times, np.arange(f0.size) * (FP / 1000.0), f0)
    frame = times / (FP / 1000.0)
    inner = (frame >= 3) & (frame <= f0.size - 1 - 3)
    assert inner.sum() > 90 and (got[inner] > 0).all()
    cents = 1200.0 * np.abs(np.log2(got[inner] / want[inner]))
    print(f"[world] tracker: worst {cents.max():.2f} cents over {int(inner.sum())} frames")
    assert cents.max() <= 50.0


@pytest.mark.parametrize("fft_size", [512, 2048])
def test_other_transform_lengths(hip_device, fft_size):
    """The 512 and 2048 instances on one short voiced row with a loud aperiodic part."""
    f0 = np.full(6, 187.7)
    sp = ref.envelope("ih", FS, fft_size).astype(np.float32)
    ap = np.full(fft_size // 2 + 1, 0.4, np.float32)
    n = world.output_length(6, FS, FP)
    noise = np.random.default_rng(5).standard_normal(n).astype(np.float32)
    f64 = ref.synthesize(f0, sp.astype(np.float64), ap.astype(np.float64), FS, FP, noise.astype(np.float64))
    f32 = ref.synthesize(f0, sp.astype(np.float64), ap.astype(np.float64), FS, FP, noise.astype(np.float64), fp32=True)
    dev = lambda a: torch.tensor(a, device=hip_device)  # noqa: E731
    got = world.world_synthesize(f0, dev(sp), dev(ap), FS, FP, noise=dev(noise)).cpu().numpy()
    e_gpu, e_32 = np.abs(got - f64).max(), np.abs(f32 - f64).max()
    print(f"[world] fft {fft_size}: e_gpu {e_gpu:.3e} e_32 {e_32:.3e}")
    assert e_gpu <= 2 * e_32 + 1e-5


def test_dataloader_with_world_items(tmp_path, hip_device):
    """build_dataloader with both generators on: WORLD rows equal the log-mel of the GPU's own single-row synthesis
    (gain, additive noise and crop window applied), labels and silences equal the host's."""
    lines = []
    for i, dur in enumerate((2.0, 3.0, 0.9, 2.6, 2.0, 4.0, 1.4, 2.2)):
        sr = 16000 if i == 6 else FS                 # the second batch mixes source rates: its rows are resampled first
        n, f = int(dur * sr), 110.0 + 37.0 * i
        t = np.arange(n) / sr
        wave = sum(0.3 / h * np.sin(2 * np.pi * h * f * t + h) for h in (1, 2, 3)).astype(np.float32)
        p = tmp_path / f"u{i}.wav"
        write_wav(p, wave, sr, "float32")
        np.save(str(p) + "_f0.npy", np.full(1 + int(dur * FS) // HOP, f, np.float32))
        lines.append(f"{p}|0\n")
    syn = {"enabled": True, "ratio": 0.5, "apply_to_validation": True,
           "pitch_shift": {"enabled": True, "semitones": [-2, 1, 4], "gain_db_range": [-6.0, 3.0]},
           "world_vocoder": {"enabled": True, "backend": "hip", "duration": {"min": 0.6, "max": 3.2},
                             "noise_db": -60.0}}
    cfg = {"mel_params": {"sample_rate": FS, "win_len": 1024, "n_fft": 1024, "n_mels": 80, "hop_length": HOP},
           "dataloader": {"start_method": None}, "verbose": False, "synthetic_data": syn}
    loader = md.build_dataloader(lines, validation=True, batch_size=6, num_workers=0, device="cuda:0",
                                 dataset_config=cfg)
    ds = loader.dataset
    assert ds._synthetic_generators == ["pitch_shift", "world_vocoder"]
    assert len(ds) == 12 and len(loader) == 2
    np.random.seed(6); random.seed(6)
    got = [(m.cpu().numpy(), f.cpu().numpy(), s.cpu().numpy()) for m, f, s in loader]
    np.random.seed(6); random.seed(6)
    gen = ds._world_generator
    templates = gen.device_templates(hip_device)
    n_world = n_crop = 0
    for bi in range(2):
        m, f, s = got[bi]
        assert m.shape == (6, 1, 80, 192) and np.isfinite(m).all()
        for k, i in enumerate(range(6 * bi, 6 * bi + 6)):
            if i < 8:
                ds.path_to_wave_and_label(ds.data_list[i])         # consume the item's draws
                continue
            item = ds[i]
            req = item[-1]
            if not isinstance(req, md.WorldRequest):
                continue
            n_world += 1
            n_crop += req.crop > 0
            full = world.world_synthesize(req.curve, templates[req.template], None, FS, gen.frame_period,
                                          seed=req.seed).cpu().numpy()
            wave = np.zeros(req.n, np.float32)
            wave[req.out_start:req.out_start + req.out_len] = (
                np.float32(req.gain) * full[req.out_start:req.out_start + req.out_len] + req.noise)
            mel = mel_ref.log_mel(wave)[:, req.crop:req.crop + 192].astype(np.float32)
            rm, rf, rs = train_ref.collate([(mel, item[1].numpy(), item[2].numpy())])
            assert np.abs(m[k] - rm[0]).max() <= 1e-3, (bi, k)
            np.testing.assert_array_equal(f[k], rf[0])
            np.testing.assert_array_equal(s[k], rs[0])
    assert n_world == 2 and n_crop == 1                         # one WORLD row is longer than 192 frames

"""HIP mel front end away from DEFAULT_MEL_PARAMS: filterbank tables, hop, work split, alignment, ragged entry.

Parameter sets and what each reaches in the plan's chunk tables: tests/mel_plan_ref.py (pinned on the CPU by
tests/test_oracle_mel.py::test_chunk_table_is_pinned).  Reference: the float64 oracle, oracle/mel_ref.py.

Tolerances
* shape, padding, an empty filter's row: exact;
* mel power on white noise: 1e-4 relative on every bin with ref >= 2.5e-7 * ref.max() (the >= 1e-2 floor of
  tests/test_mel_gpu.py at its ~4e4 frame peak, made relative), and those bins are >= 99 % of all bins;
* normalised log-mel: 1e-3 absolute everywhere;
* against exact arithmetic the kernel is at most twice as far off as the CPU float32 ``torch.stft`` path
  (floors 1e-4 log, 1e-5 power), per parameter set;
* work split, batch size, max_frames, pad value, fast (float2) vs slow (per-sample) loads, ragged entry vs
  per-row calls: bit for bit (``torch.equal``) -- the arithmetic of a frame does not depend on any of them.

Measured worst error against float64 per set (MI355X; CPU = float32 torch.stft + float32 filterbank product):

    set              power, noise (relative)      log-mel, noise and sweep (absolute)
                     HIP        CPU float32       HIP        CPU float32
    sr16k            6.6e-07    8.8e-07           9.3e-05    2.6e-04
    mels128          5.1e-06    2.3e-06           1.4e-04    1.9e-04
    sr44k1_hop441    8.0e-07    1.5e-06           1.0e-04    2.8e-04
    sr22k05_hop275   4.5e-07    6.4e-07           1.9e-04    1.9e-04
    band50_7600      1.1e-06    1.7e-06           1.5e-04    1.5e-04
    band0_4000       1.9e-06    2.7e-06           2.1e-04    2.3e-04
    mels200          7.6e-06    5.1e-06           2.4e-04    2.1e-04
    hop75            2.5e-06    1.9e-06           1.9e-04    2.3e-04
    hop1200          3.5e-07    9.2e-07           4.0e-07    2.3e-07

The log-mel figures are set by the sweep's bins near the 1e-5 log floor (hop1200: the 0.25 s utterance is all
silence at that hop, so only noise counts).  Power on mels128 is 2.2x the CPU path's error, inside the 1e-5 floor
of that comparison: both figures are FFT rounding noise (~1e-8 of the frame peak) seen through the narrowest
filters, one or two taps wide, where nothing averages it; the CPU figure itself moves by 20 % between hosts.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import mel_ref
from pitchextractor_amd import synthetic
from pitchextractor_amd.mel import MelSpectrogram
from tests import mel_plan_ref

pytestmark = pytest.mark.gpu

N_NOISE = 6000
STRONG = 2.5e-7          # relative floor of the bins held to 1e-4
DEFAULT = mel_ref.DEFAULT_MEL_PARAMS


# ---- 2. parameter sweep -------------------------------------------------------------------------------------------

def _sweep_index(sr, hop):
    """First utterance whose silenced gap (10-30 frames) leaves at least 30 % of a 0.25 s sweep sounding; at a hop
    where none does (hop 1200: 6 frames) utterance 0, silent, which still checks the log floor."""
    for i in range(32):
        if np.count_nonzero(synthetic.utterance(i, duration=0.25, sr=sr, hop=hop)[0]) >= 0.3 * int(0.25 * sr):
            return i
    return 0


@functools.lru_cache(maxsize=None)
def _reference(name):
    """Inputs and CPU references of one parameter set, computed once and shared read-only."""
    params = dict(next(p for n, p, _ in mel_plan_ref.PARAM_SETS if n == name))
    kw = mel_plan_ref.mel_kwargs(params)
    sr, hop = params["sample_rate"], params["hop_length"]
    rng = np.random.default_rng(len(name) + sr + hop)
    waves = {"noise": (0.3 * rng.standard_normal(N_NOISE)).astype(np.float32),
             "sweep": synthetic.utterance(_sweep_index(sr, hop), duration=0.25, sr=sr, hop=hop)[0]}
    ref64 = {k: mel_ref.mel_spectrogram(w, **kw) for k, w in waves.items()}
    cpu32 = {k: np.asarray(mel_ref.mel_spectrogram_torch_stft(w, **kw), dtype=np.float64) for k, w in waves.items()}
    for v in list(waves.values()) + list(ref64.values()) + list(cpu32.values()):
        v.setflags(write=False)
    return kw, waves, ref64, cpu32


def _rel_err(got, ref, strong):
    return (np.abs(got - ref)[strong] / ref[strong]).max()


@pytest.mark.parametrize("name", mel_plan_ref.PARAM_IDS)
def test_parameter_set_matches_float64_oracle(hip_device, name):
    kw, waves, ref64, cpu32 = _reference(name)
    n_mels, hop = kw["n_mels"], kw["hop_length"]
    tf = MelSpectrogram(**kw)
    empty = mel_plan_ref.empty_filters(**kw)
    hip_log = cpu_log = 0.0
    for kind, wave in waves.items():
        ref = ref64[kind]
        L = 1 + wave.shape[0] // hop
        dev = torch.tensor(wave, device=hip_device)
        power = tf(dev).cpu().numpy()
        logm = tf.log_mel_batch(dev[None], max_frames=L + 3).cpu().numpy()
        assert power.shape == ref.shape == (n_mels, L)
        assert logm.shape == (1, 1, n_mels, L + 3)
        assert (logm[0, 0, :, L:] == 0).all()
        assert np.isfinite(power).all() and (power >= 0).all()
        for m in empty:
            assert (power[m] == 0.0).all() and (ref[m] == 0.0).all()

        lref = mel_ref.log_normalise(ref)
        err_log = np.abs(logm[0, 0, :, :L].astype(np.float64) - lref).max()
        err_log_pow = np.abs(mel_ref.log_normalise(power.astype(np.float64)) - lref).max()
        hip_log = max(hip_log, err_log, err_log_pow)
        cpu_log = max(cpu_log, np.abs(mel_ref.log_normalise(cpu32[kind]) - lref).max())
        print(f"{name} {kind}: log-mel max |err| HIP {err_log:.2e}")
        assert err_log <= 1e-3 and err_log_pow <= 1e-3

        if kind == "noise":
            strong = ref >= STRONG * ref.max()
            share = strong.mean()
            hip_pow = _rel_err(power.astype(np.float64), ref, strong)
            cpu_pow = _rel_err(cpu32[kind], ref, strong)
            print(f"{name} noise: strong share {share:.4f}; power rel err HIP {hip_pow:.2e}, CPU fp32 {cpu_pow:.2e}")
            assert share >= 0.99
            assert hip_pow <= 1e-4
    print(f"{name}: log-mel max |err| vs float64: HIP {hip_log:.2e}, CPU fp32 {cpu_log:.2e}")
    assert hip_log <= max(2.0 * cpu_log, 1e-4)
    assert hip_pow <= max(2.0 * cpu_pow, 1e-5)


@pytest.mark.parametrize("bad", [dict(n_mels=40),                 # a filter of 9 chunks > kMaxParts
                                 dict(n_mels=256),                # 280 pairs > 256
                                 dict(f_min=4000.0, f_max=4000.0),
                                 dict(f_min=8000.0, f_max=4000.0),
                                 dict(f_min=-1.0)],
                         ids=["mels40", "mels256", "fmax_eq_fmin", "fmax_lt_fmin", "fmin_negative"])
def test_unsupported_parameters_are_refused_cleanly(hip_device, bad):
    wave = torch.tensor(_reference("band0_4000")[1]["noise"], device=hip_device)
    tf = MelSpectrogram(**{**DEFAULT, **bad})
    with pytest.raises(RuntimeError):
        tf(wave)
    with pytest.raises(RuntimeError):                    # and again: the failed plan left nothing half built
        tf.log_mel_batch(wave[None], max_frames=8)
    kw, _, ref64, _ = _reference("band0_4000")           # the process is still usable
    got = MelSpectrogram(**kw)(wave).cpu().numpy().astype(np.float64)
    strong = ref64["noise"] >= STRONG * ref64["noise"].max()
    assert _rel_err(got, ref64["noise"], strong) <= 1e-4


# ---- 3. work split and batch independence, bit for bit ------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _rows(n):
    rng = np.random.default_rng(n)
    rows = (0.3 * rng.standard_normal((4, n))).astype(np.float32)
    rows.setflags(write=False)
    return rows


@functools.lru_cache(maxsize=None)
def _batch4(n, max_frames):
    """Power and log-mel of the 4 rows run as a batch of 4, on the device; checked once against the oracle."""
    dev = torch.device("cuda:0")
    tf = MelSpectrogram(**DEFAULT)
    rows = torch.tensor(_rows(n)).to(dev)
    power, logm = tf(rows), tf.log_mel_batch(rows, max_frames=max_frames)
    L = 1 + n // 300
    ref = mel_ref.log_mel(_rows(n)[1])
    assert np.abs(logm[1, 0, :, :L].cpu().numpy() - ref).max() <= 1e-3
    assert np.abs(mel_ref.log_normalise(power[1].cpu().numpy().astype(np.float64)) - ref).max() <= 1e-3
    return power, logm


def _check_tiled(hip_device, n, batch, max_frames):
    power4, log4 = _batch4(n, max_frames)
    tf = MelSpectrogram(**DEFAULT)
    rows = torch.tensor(_rows(n)).to(hip_device)
    big = rows.repeat((batch + 3) // 4, 1)[:batch].contiguous()
    sel = torch.arange(batch, device=hip_device) % 4
    power = tf(big)
    assert power.shape == (batch, 80, 1 + n // 300)
    assert torch.equal(power, power4[sel])
    logm = tf.log_mel_batch(big, max_frames=max_frames)
    assert logm.shape == (batch, 1, 80, max_frames)
    assert torch.equal(logm, log4[sel])
    assert (logm[..., 1 + n // 300:] == 0).all()


@pytest.mark.parametrize("batch", [1, 4, 48, 256, 512, 1100])
def test_short_rows_do_not_depend_on_batch_size(hip_device, batch):
    """17 valid frames of 24: spans 4 to 20, a last range ending inside a 16-frame chunk, and at 1100 rows one
    range per row with more rows than resident workgroups."""
    _check_tiled(hip_device, 4800, batch, 24)


@pytest.mark.parametrize("batch", [48, 64, 100, 128])
def test_two_second_rows_do_not_depend_on_batch_size(hip_device, batch):
    _check_tiled(hip_device, 48000, batch, 192)


@pytest.mark.parametrize("max_frames", [1, 3, 4, 5, 17, 40])
def test_max_frames_and_pad_value(hip_device, max_frames):
    power4, log4 = _batch4(4800, 24)
    tf = MelSpectrogram(**DEFAULT)
    row = torch.tensor(_rows(4800)[:1], device=hip_device)
    k = min(max_frames, 17)
    out = tf.log_mel_batch(row, max_frames=max_frames)
    assert out.shape == (1, 1, 80, max_frames)
    assert torch.equal(out[..., :k], log4[:1, :, :, :k])
    assert (out[..., k:] == 0).all()
    for log_mode, want in ((1, log4[0, 0]), (0, power4[0])):
        buf = torch.full((1, 1, 80, max_frames), 99.0, device=hip_device)
        tf._run(row, buf, (buf.stride(0), buf.stride(2), buf.stride(3)), max_frames, log_mode, -7.5)
        assert torch.equal(buf[0, 0, :, :k], want[:, :k])
        assert (buf[..., k:] == -7.5).all()


# ---- 4. float2 fast path vs per-sample path -----------------------------------------------------------------------

def _both(tf, waves, max_frames):
    return tf(waves), tf.log_mel_batch(waves, max_frames=max_frames)


def test_odd_row_stride_equals_contiguous(hip_device):
    buf = torch.zeros((4, 4801), device=hip_device)
    buf[:, :4800] = torch.tensor(_rows(4800), device=hip_device)
    view = buf[:, :4800]
    assert view.stride() == (4801, 1)                   # rows 1 and 3 start 4 bytes off an 8-byte boundary
    tf = MelSpectrogram(**DEFAULT)
    power4, log4 = _batch4(4800, 24)
    power, logm = _both(tf, view, 24)
    assert torch.equal(power, power4) and torch.equal(logm, log4)


def test_view_at_odd_storage_offset_equals_aligned_copy(hip_device):
    """``buf[1:]``: even length, even (unit) strides, but the first sample sits 4 bytes off an 8-byte boundary;
    the kernel must look at the address, not at the stride, before it loads sample pairs."""
    buf = torch.zeros(4801, device=hip_device)
    buf[1:] = torch.tensor(_rows(4800)[2], device=hip_device)
    view = buf[1:]
    assert view.data_ptr() % 8 == 4 and view.shape == (4800,)
    tf = MelSpectrogram(**DEFAULT)
    power4, log4 = _batch4(4800, 24)
    assert torch.equal(tf(view), power4[2])
    assert torch.equal(tf.log_mel_batch(view[None], max_frames=24), log4[2:3])
    # the same in a batch: a (2, 4800) view of a buffer that starts one sample late
    buf2 = torch.zeros(2 * 4800 + 1, device=hip_device)
    buf2[1:] = torch.tensor(_rows(4800)[:2], device=hip_device).reshape(-1)
    view2 = buf2[1:].view(2, 4800)
    assert view2.data_ptr() % 8 == 4 and view2.stride() == (4800, 1)
    power, logm = _both(tf, view2, 24)
    assert torch.equal(power, power4[:2]) and torch.equal(logm, log4[:2])


def test_odd_hop_equals_odd_stride_rows(hip_device):
    """Hop 275: every second interior frame starts at an odd sample; in an odd-stride buffer the rows swap which."""
    kw = _reference("sr22k05_hop275")[0]
    tf = MelSpectrogram(**kw)
    rows = torch.tensor(_rows(6000), device=hip_device)
    buf = torch.zeros((4, 6001), device=hip_device)
    buf[:, :6000] = rows
    L = 1 + 6000 // 275
    a_pow, a_log = _both(tf, rows, L + 2)
    b_pow, b_log = _both(tf, buf[:, :6000], L + 2)
    assert torch.equal(a_pow, b_pow) and torch.equal(a_log, b_log)
    ref = mel_ref.log_mel(_rows(6000)[3], **kw)
    assert np.abs(a_log[3, 0, :, :L].cpu().numpy() - ref).max() <= 1e-3
    assert (a_log[..., L:] == 0).all()


# ---- 5. ragged entry ----------------------------------------------------------------------------------------------

RAGGED_FRAMES = 24


def _ragged_rows(hop):
    """(length, frame_start) per row; n_full = frames of a 6000-sample row."""
    n_full = 1 + 6000 // hop
    rows = [(513, 0), (512, 0),                         # neighbours: shortest legal row / too short for reflect padding
            (6000, n_full - 1),                         # one valid frame
            (6000, n_full), (6000, n_full + 5),         # padding only
            (6000, -3),                                 # clamped to 0
            (5999, 2), (4321, 1)]
    if n_full >= RAGGED_FRAMES:                         # the crop ends exactly at the last frame
        rows.append((6000, n_full - RAGGED_FRAMES))
    return rows


@pytest.mark.parametrize("name", ["default", "sr16k"])
def test_ragged_rows(hip_device, name):
    """Hop 300 gives a 6000-sample row 21 frames, fewer than max_frames = 24, so the row whose crop ends exactly at
    its last frame exists at hop 160 (38 frames) only."""
    kw = dict(DEFAULT) if name == "default" else _reference(name)[0]
    hop = kw["hop_length"]
    spec = _ragged_rows(hop)
    assert name != "sr16k" or spec[-1] == (6000, 14)
    B = len(spec)
    rng = np.random.default_rng(hop)
    waves = np.zeros((B, 6000), np.float32)
    for i, (n, _) in enumerate(spec):
        waves[i, :n] = 0.2 * rng.standard_normal(n)
    tf = MelSpectrogram(**kw)
    dev = torch.from_numpy(waves).to(hip_device)
    lens = torch.tensor([n for n, _ in spec], dtype=torch.int32, device=hip_device)
    starts = torch.tensor([s for _, s in spec], dtype=torch.int32, device=hip_device)
    out = tf.log_mel_ragged(dev, lens, starts, max_frames=RAGGED_FRAMES)
    assert out.shape == (B, 1, kw["n_mels"], RAGGED_FRAMES)

    buf = torch.zeros((B, 6001), device=hip_device)
    buf[:, :6000] = dev
    assert buf[:, :6000].stride() == (6001, 1)
    assert torch.equal(tf.log_mel_ragged(buf[:, :6000], lens, starts, max_frames=RAGGED_FRAMES), out)

    got = out.cpu().numpy()
    seen_valid = set()
    for i, (n, start) in enumerate(spec):
        if n <= 512:
            assert (got[i] == 0).all()
            continue
        s = max(start, 0)
        ref = mel_ref.log_mel(waves[i, :n], **kw)[:, s:s + RAGGED_FRAMES]
        k = ref.shape[1]
        seen_valid.add(k)
        assert k == max(0, min(RAGGED_FRAMES, 1 + n // hop - s))
        assert np.abs(got[i, 0, :, :k] - ref).max() <= 1e-3 if k else True, i
        assert (got[i, 0, :, k:] == 0).all(), i
        per_row = tf.log_mel_batch(dev[i:i + 1, :n], max_frames=1 + n // hop)
        assert torch.equal(out[i, 0, :, :k], per_row[0, 0, :, s:s + k]), i
    assert {0, 1, 1 + 513 // hop} <= seen_valid and (RAGGED_FRAMES in seen_valid) == (name == "sr16k")
    # a negative start is start 0: rows 5 and a fresh start-0 run of the same samples agree
    zero = tf.log_mel_ragged(dev[5:6], lens[5:6], torch.zeros(1, dtype=torch.int32, device=hip_device),
                             max_frames=RAGGED_FRAMES)
    assert torch.equal(zero[0], out[5])

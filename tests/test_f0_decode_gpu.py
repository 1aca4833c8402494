"""F0 bin decoding on the device (``ops.decode_f0_bins``, ``inference.predict_f0(decoder=...)``,
``inference.pitch_metrics``) against the float64 restatement in ``tests/f0_decode_ref.py``.

Tolerances come from the restatement, not from the kernels:

* ``weighted`` / ``weighted_viterbi`` Hz and ``confidence``: the restatement run in float32 against its float64 run
  on the test's own inputs, times 4 (the device's libm and summation order differ from numpy's), capped at 1e-5
  relative in Hz (0.017 cent).  On this file's inputs (seed 1, 4 096 rows of N(0,1) logits / 4 096 peaked rows)
  float32 numpy is off by 1.27e-6 / 8.1e-7 relative in Hz and by 1.59e-7 / 1.87e-7 in confidence, so the allowances
  are 5.1e-6 / 3.2e-6 in Hz and 6.3e-7 / 7.5e-7 in confidence (``test_weighted_and_confidence_within_float32_rounding``
  prints the figures; an MI355X measured 7.7e-7 / 3.6e-7 in Hz and 1.5e-7 / 2.1e-7 in confidence against float64).
* Viterbi on *margin* inputs (a noisy ridge along a glide, plus planted octave spikes that ``argmax`` follows): the
  path must equal the float64 path on EVERY frame; the inputs qualify only if the float32 restatement already does.
* Viterbi on *adversarial* inputs (i.i.d. N(0,1) logits, where an fp32 DP may legitimately pick another path): the
  float64 score of the returned path must be within ``4 L 2^-24 max|delta|`` of the float64 optimum.
"""
import numpy as np
import pytest
import torch

from oracle import model_ref
from pitchextractor_amd import inference, ops, synthetic
from tests import f0_decode_ref as ref
from tests.test_f0_decode_cpu import GOLDEN, metrics_f32_tolerance

pytestmark = pytest.mark.gpu

HZ_CAP = 1e-5


def margin_logits(rng, N, T=192, C=360):
    """float32 (N, T, C): ``max(-0.5 ((cents(c) - cents_true[t]) / 25)^2, -30)`` along a linear glide in Hz
    (U(60, 250) -> U(120, 500) Hz, the distribution of ``synthetic.utterance``), on 8 random frames per sequence the
    bin one octave (60 bins) above the truth raised to +6 (above the ridge's 0, so ``argmax`` goes there; the
    transition band forbids the 60-bin jump), then N(0, 0.5) noise on every bin.  Returns (logits, true cents)."""
    cents_c = ref.bin_cents(np.arange(C))
    out = np.zeros((N, T, C), dtype=np.float32)
    truth = np.zeros((N, T))
    for n in range(N):
        hz = np.linspace(rng.uniform(60.0, 250.0), rng.uniform(120.0, 500.0), T)
        ct = 1200.0 * np.log2(hz / 10.0)
        raw = np.maximum(-0.5 * ((cents_c[None, :] - ct[:, None]) / 25.0) ** 2, -30.0)
        frames = rng.choice(T, 8, replace=False)
        octave = np.rint((ct[frames] - ref.CENTS0) / 20.0).astype(int) + 60
        raw[frames, octave] = 6.0
        out[n] = (raw + rng.normal(0.0, 0.5, size=(T, C))).astype(np.float32)
        truth[n] = ct
    return out, truth


def decode_gpu(x, dev, lengths=None, method="argmax"):
    xd = x if isinstance(x, torch.Tensor) else torch.from_numpy(x).to(dev)
    ld = None if lengths is None else torch.tensor(lengths, dtype=torch.int32, device=dev)
    f0, conf, bins = ops.decode_f0_bins(xd, ld, method)
    torch.cuda.synchronize()
    return f0.cpu().numpy(), conf.cpu().numpy(), bins.cpu().numpy()


def rel_err(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.abs(b))) if a.size else 0.0


def float32_allowance(x2d, bins):
    """(Hz allowance for the weighted average, Hz allowance for f(bin), confidence allowance) on rows ``x2d`` decoded
    at ``bins``: 4 x (float32 restatement vs float64 restatement), Hz capped at 1e-5.  Also returns the raw figures."""
    hz64 = ref.cents_to_hz(ref.weighted_cents(x2d, bins))
    hz32 = ref.cents_to_hz(ref.weighted_cents(x2d, bins, np.float32), np.float32)
    b64, b32 = ref.bin_hz(bins), ref.bin_hz(bins, np.float32)
    c64, c32 = ref.confidence(x2d, bins), ref.confidence(x2d, bins, np.float32)
    raw = (rel_err(hz32, hz64), rel_err(b32, b64), rel_err(c32, c64))
    return min(4 * raw[0], HZ_CAP), min(4 * raw[1], HZ_CAP), 4 * raw[2], raw


def test_argmax_bins_exact_with_ties(hip_device):
    rng = np.random.default_rng(2)
    N, T, C = 3, 128, 360
    x = rng.normal(size=(N, T, C)).astype(np.float32)
    top = np.float32(9.0)
    x[0, 0, [17, 200]] = top                       # two equal maxima
    x[0, 1, [5, 6, 300]] = top                     # three
    x[0, 2, [0, 359]] = top                        # at the row ends
    x[0, 3, [359]] = top
    x[0, 4, [0]] = top
    x[0, 5, :] = np.float32(0.25)                  # a constant row
    x[0, 6, [63, 64]] = top                        # across the lanes' second round
    x[0, 7, [320, 64, 128]] = top
    rows = x.reshape(-1, C)
    rbins = ref.argmax_bins(rows)
    assert rbins[:8].tolist() == [17, 5, 0, 359, 0, 0, 63, 64]
    _, hz_tol, conf_tol, _ = float32_allowance(rows, rbins)
    # rows inside a wider buffer (ld_t > C)
    wide = torch.zeros((N, T, C + 8), dtype=torch.float32, device=hip_device)
    wide[:, :, :C] = torch.from_numpy(x).to(hip_device)
    for xd in (torch.from_numpy(x).to(hip_device), wide[:, :, :C]):
        f0, conf, bins = decode_gpu(xd, hip_device)
        assert bins.dtype == np.int32 and f0.dtype == np.float32 and bins.shape == (N, T)
        assert np.array_equal(bins.reshape(-1), rbins)
        assert rel_err(f0.reshape(-1), ref.bin_hz(rbins)) <= hz_tol
        assert rel_err(conf.reshape(-1), ref.confidence(rows, rbins)) <= conf_tol
    # (T, C) is N = 1; two bins only
    small = rng.normal(size=(512, 2)).astype(np.float32)
    f0, conf, bins = decode_gpu(small, hip_device, method="weighted")
    sbins = ref.argmax_bins(small)
    hz_tol, _, conf_tol, _ = float32_allowance(small, sbins)
    assert bins.shape == (512,) and np.array_equal(bins, sbins)
    assert rel_err(f0, ref.cents_to_hz(ref.weighted_cents(small, sbins))) <= hz_tol
    assert rel_err(conf, ref.confidence(small, sbins)) <= conf_tol


def test_weighted_and_confidence_within_float32_rounding(hip_device):
    rng = np.random.default_rng(1)
    flat = rng.normal(size=(32, 128, 360)).astype(np.float32)
    peaked, _ = margin_logits(rng, 32, T=128)
    for name, x in (("N(0,1)", flat), ("peaked", peaked)):
        f0, conf, bins = decode_gpu(x, hip_device, method="weighted")
        rows = x.reshape(-1, x.shape[-1])
        rbins = ref.argmax_bins(rows)
        assert np.array_equal(bins.reshape(-1), rbins)
        hz64 = ref.cents_to_hz(ref.weighted_cents(rows, rbins))
        c64 = ref.confidence(rows, rbins)
        hz_tol, _, conf_tol, raw = float32_allowance(rows, rbins)
        got_hz, got_conf = rel_err(f0.reshape(-1), hz64), rel_err(conf.reshape(-1), c64)
        print(f"{name}: float32 numpy vs float64: Hz {raw[0]:.2e} conf {raw[2]:.2e}; allowance Hz {hz_tol:.2e} "
              f"conf {conf_tol:.2e}; device Hz {got_hz:.2e} conf {got_conf:.2e}")
        assert got_hz <= hz_tol
        assert got_conf <= conf_tol
        assert np.all((conf > 0) & (conf <= 1))


def test_viterbi_equals_float64_path_on_margin_inputs(hip_device):
    rng = np.random.default_rng(0)
    x, _ = margin_logits(rng, 6)
    p64 = ref.viterbi_paths(x)
    p32 = ref.viterbi_paths(x, dtype=np.float32)
    assert np.array_equal(p32, p64), "inputs do not qualify: float32 and float64 restatements disagree"
    am = ref.argmax_bins(x)
    differ = (am != p64).sum(axis=1)
    print("frames where argmax leaves the Viterbi path:", differ.tolist())
    assert differ.min() >= 8                        # a decoder that ignores the transitions cannot pass
    assert np.abs(np.diff(p64, axis=1)).max() <= 11
    f0, conf, bins = decode_gpu(x, hip_device, method="viterbi")
    assert np.array_equal(bins, p64)                # every frame; nothing left out
    f0w, confw, binsw = decode_gpu(x, hip_device, method="weighted_viterbi")
    assert np.array_equal(binsw, p64) and np.array_equal(confw, conf)
    rows, path = x.reshape(-1, 360), p64.reshape(-1)
    hz_tol, bin_tol, conf_tol, _ = float32_allowance(rows, path)
    assert rel_err(f0.reshape(-1), ref.bin_hz(path)) <= bin_tol
    assert rel_err(f0w.reshape(-1), ref.cents_to_hz(ref.weighted_cents(rows, path))) <= hz_tol
    assert rel_err(conf.reshape(-1), ref.confidence(rows, path)) <= conf_tol


ADVERSARIAL = [
    pytest.param(192, 360, [1, 2, 191, 192, 57, 100, 192], id="ragged"),
    pytest.param(700, 360, [700, 333, 1, 699, 700, 64, 512], id="spilled-T700"),
    pytest.param(192, 722, [192, 191, 2, 192, 77, 1, 130], id="C722"),
]


def check_adversarial(x, lengths, bins):
    for n, L in enumerate(lengths):
        path = bins[n, :L]
        assert np.all(bins[n, L:] == 0)
        assert path.min() >= 0 and path.max() < x.shape[2]
        if L > 1:
            assert np.abs(np.diff(path)).max() <= 11
        best, peak = ref.viterbi_path(x[n, :L], return_delta=True)
        opt = ref.path_score(x[n, :L], best)
        tol = 4 * L * 2.0 ** -24 * peak             # two fp32 roundings per frame on numbers <= the score, doubled
        got = ref.path_score(x[n, :L], path)
        assert opt - got <= tol, (n, L, opt, got, tol)


@pytest.mark.parametrize("T,C,lengths", ADVERSARIAL)
def test_viterbi_score_on_adversarial_inputs(hip_device, T, C, lengths):
    rng = np.random.default_rng(7)
    x = rng.normal(size=(7, T, C)).astype(np.float32)
    f0, conf, bins = decode_gpu(x, hip_device, lengths, "viterbi")
    check_adversarial(x, lengths, bins)
    for n, L in enumerate(lengths):
        assert np.all(f0[n, L:] == 0) and np.all(conf[n, L:] == 0)
    rows = np.concatenate([x[n, :L] for n, L in enumerate(lengths)])
    path = np.concatenate([bins[n, :L] for n, L in enumerate(lengths)])
    _, bin_tol, conf_tol, _ = float32_allowance(rows, path)
    assert rel_err(np.concatenate([f0[n, :L] for n, L in enumerate(lengths)]), ref.bin_hz(path)) <= bin_tol
    assert rel_err(np.concatenate([conf[n, :L] for n, L in enumerate(lengths)]), ref.confidence(rows, path)) <= conf_tol


def test_a_sequence_alone_equals_the_same_sequence_in_a_ragged_batch(hip_device):
    rng = np.random.default_rng(9)
    lengths = [1, 2, 191, 192, 57]
    x = rng.normal(size=(5, 192, 360)).astype(np.float32)
    xd = torch.from_numpy(x).to(hip_device)
    for method in ops.F0_DECODERS:
        batch = decode_gpu(xd, hip_device, lengths, method)
        for n, L in enumerate(lengths):
            alone = decode_gpu(xd[n:n + 1], hip_device, [L], method)
            for a, b in zip(alone, batch):
                assert np.array_equal(a[0].view(np.int32), b[n].view(np.int32)), (method, n)
        flat = decode_gpu(xd[3], hip_device, None, method)           # (T, C), no lengths
        for a, b in zip(flat, batch):
            assert np.array_equal(a.view(np.int32), b[3].view(np.int32))


def test_full_size_all_methods(hip_device):
    """N = 256, T = 192, C = 360 (the inference batch): 70.8 MB of logits, decoded by all four methods."""
    rng = np.random.default_rng(3)
    x, _ = margin_logits(rng, 256)
    p64 = ref.viterbi_paths(x)
    assert np.array_equal(ref.viterbi_paths(x, dtype=np.float32), p64), "inputs do not qualify"
    am = ref.argmax_bins(x)
    xd = torch.from_numpy(x).to(hip_device)
    rows = x.reshape(-1, 360)
    for method in ops.F0_DECODERS:
        f0, conf, bins = decode_gpu(xd, hip_device, None, method)
        want = (p64 if "viterbi" in method else am).reshape(-1)
        assert np.array_equal(bins.reshape(-1), want), method
        hz_tol, bin_tol, conf_tol, _ = float32_allowance(rows[::16], want[::16])
        if method.startswith("weighted"):
            assert rel_err(f0.reshape(-1), ref.cents_to_hz(ref.weighted_cents(rows, want))) <= hz_tol
        else:
            assert rel_err(f0.reshape(-1), ref.bin_hz(want)) <= bin_tol
        assert rel_err(conf.reshape(-1), ref.confidence(rows, want)) <= conf_tol


def test_predict_f0_decodes_a_classifier_end_to_end(tmp_path, hip_device):
    state = model_ref.seeded_state(31, num_class=360, hidden_size=64)
    torch.save({"model": state}, tmp_path / "c.pth")
    net = inference.load_model(tmp_path / "c.pth", device=hip_device)
    assert net.num_class == 360
    wave, _, _ = synthetic.utterance(2, duration=4.2)               # 337 frames -> chunks at 0, 144, 288
    logits = inference.predict_f0(net, wave)
    assert isinstance(logits, np.ndarray) and logits.shape == (433, 360) and logits.dtype == np.float32
    spans = [(0, 192), (192, 384), (384, 433)]                      # the chunks inside the concatenation
    # decoded Hz sit exactly on the bin grid, so a Viterbi path is read back from them with the loss's own mapping
    vpath = model_ref.f0_to_bins(inference.predict_f0(net, wave, decoder="viterbi"))
    for method in ops.F0_DECODERS:
        got, conf = inference.predict_f0(net, wave, decoder=method, return_confidence=True)
        assert got.shape == conf.shape == (433,) and got.dtype == np.float32
        assert np.array_equal(got, inference.predict_f0(net, wave, decoder=method))
        assert np.all((conf > 0) & (conf <= 1))
        if "viterbi" in method:
            # an untrained network's logits are nearly flat: judge each chunk's path by its float64 score
            path = vpath
            for a, b in spans:
                best, peak = ref.viterbi_path(logits[a:b], return_delta=True)
                tol = 4 * (b - a) * 2.0 ** -24 * peak
                assert ref.path_score(logits[a:b], best) - ref.path_score(logits[a:b], path[a:b]) <= tol
                assert np.abs(np.diff(path[a:b])).max() <= 11
        else:
            path = ref.argmax_bins(logits)
        hz_tol, bin_tol, conf_tol, _ = float32_allowance(logits, path)
        if method.startswith("weighted"):
            assert rel_err(got, ref.cents_to_hz(ref.weighted_cents(logits, path))) <= hz_tol
        else:
            assert rel_err(got, ref.bin_hz(path)) <= bin_tol
            assert np.array_equal(model_ref.f0_to_bins(got), path)
        assert rel_err(conf, ref.confidence(logits, path)) <= conf_tol

    # the detector head: recompute its logits for the same chunks and cut between two of them
    mel = inference.waveform_to_mel(wave, None, hip_device)
    batch = torch.zeros((3, 1, 80, 192), dtype=torch.float32, device=hip_device)
    for i, s in enumerate((0, 144, 288)):
        e = min(s + 192, mel.shape[-1])
        batch[i, 0, :, :e - s] = mel[:, s:e]
    with torch.no_grad():
        _, sil = net(batch.transpose(-1, -2))
    z = np.concatenate([sil[i].cpu().numpy()[:b - a] for i, (a, b) in enumerate(spans)]).astype(np.float64)
    prob = np.sort(1.0 / (1.0 + np.exp(-z)))
    k = int(np.argmax(np.diff(prob[100:333]))) + 100                # the widest gap near the middle
    p = 0.5 * (prob[k] + prob[k + 1])
    plain = inference.predict_f0(net, wave, decoder="weighted_viterbi")
    gated = inference.predict_f0(net, wave, decoder="weighted_viterbi", silence_threshold=p)
    silent = 1.0 / (1.0 + np.exp(-z)) > p
    assert 0 < silent.sum() < 433
    assert np.all(gated[silent] == 0) and np.array_equal(gated[~silent], plain[~silent]) and np.all(plain > 0)
    assert np.all(inference.predict_f0(net, wave, decoder="argmax", silence_threshold=0.0) == 0)
    assert np.array_equal(inference.predict_f0(net, wave, decoder="argmax", silence_threshold=1.0),
                          inference.predict_f0(net, wave, decoder="argmax"))

    reg = model_ref.seeded_state(31, hidden_size=64, num_layers=2)
    torch.save({"model": reg}, tmp_path / "r.pth")
    rnet = inference.load_model(tmp_path / "r.pth", device=hip_device)
    with pytest.raises(ValueError):
        inference.predict_f0(rnet, wave, decoder="argmax")
    with pytest.raises(ValueError):
        inference.predict_f0(net, wave, decoder="median")


def test_pitch_metrics_on_the_device(hip_device):
    g = np.load(GOLDEN)
    for k in range(len(g["seeds"])):
        pred, r = g[f"pred_{k}"], g[f"ref_{k}"]
        want = ref.pitch_metrics(pred, r)
        for args in ((pred, r), (torch.from_numpy(pred).to(hip_device), torch.from_numpy(r).to(hip_device))):
            got = inference.pitch_metrics(*args)
            assert got["n_voiced"] == want["n_voiced"] and got["n_frames"] == want["n_frames"]
            assert isinstance(got["n_voiced"], int)
            for key in ("rms_cents", "rpa", "rca", "vuv_error"):
                if np.isnan(want[key]):
                    assert np.isnan(got[key]), key
                else:
                    assert abs(got[key] - want[key]) <= 1e-6 * abs(want[key]), (k, key, got[key], want[key])
            golden = float(g[f"rms_{k}"])
            if np.isnan(golden):
                assert np.isnan(got["rms_cents"]) and got["n_voiced"] == 0
            else:
                assert abs(got["rms_cents"] - golden) <= metrics_f32_tolerance(pred, r)[1]
    # another threshold, and a longer track than one pass of the workgroup
    rng = np.random.default_rng(4)
    r = rng.uniform(60.0, 500.0, 5000).astype(np.float32)
    r[rng.random(5000) < 0.2] = 0
    pred = (r * 2.0 ** (rng.normal(0, 40.0, 5000) / 1200.0)).astype(np.float32)
    pred[rng.random(5000) < 0.1] = 0
    for thr in (50.0, 25.0):
        got = inference.pitch_metrics(pred, r, threshold_cents=thr)
        want = ref.pitch_metrics(pred, r, threshold_cents=thr)
        for key in ("rms_cents", "rpa", "rca", "vuv_error"):
            assert abs(got[key] - want[key]) <= 1e-6 * abs(want[key]), (thr, key)
        assert (got["n_voiced"], got["n_frames"]) == (want["n_voiced"], want["n_frames"])

"""The augmentation on the device (``pitchextractor_amd.augment``, ``csrc/augment.hip``, ``pe_stress_clip_rows``) against
the float64 restatement tests/augment_ref.py: the cascade's accuracy on the kernel's own boundaries, its bit-identity
across layouts, the per-row clip, the Augmenter's chain and the loader stage.

The accuracy bound per sample is ``|y - y_ref| <= 2^-24 |y_ref| + 2^-26 max_row |y_ref|``.  The first term is the one
rounding to float32.  The second is derived, not measured: the scan reassociates the recurrence, each reassociated
operation errs by 2^-53 relative in double, a state error is amplified by at most ``(1 - r)^-2 <= 2^24`` at the pole
radius limit ``r = 1 - 2^-12``, and a handful (8) of such operations meet in one sample: 2^-53 2^24 2^3 = 2^-26.
The accuracy test prints each row's worst error over its bound before it asserts; measured on an MI355X: 0.70 of the
bound at worst (4096 samples, 8 stages), the worst error 2^-24.6 of the row's maximum, which is the rounding."""
import math
import random

import numpy as np
import pytest
import torch

from pitchextractor_amd import augment as A, stress
from tests import augment_ref as R

pytestmark = pytest.mark.gpu
f32 = np.float32
SR = 48000


def bits(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def edge_highpass():
    """The high-pass nearest the pole-radius limit that the designer allows at 48 kHz, Q = 1 / sqrt(2): the smallest f
    by bisection."""
    lo, hi = 2.0, 3.0
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        try:
            A.highpass(SR, mid)
            hi = mid
        except ValueError:
            lo = mid
    stage = A.highpass(SR, hi)
    assert A.MAX_POLE_RADIUS - 1e-9 < A.pole_radius(stage) <= A.MAX_POLE_RADIUS
    return stage


@pytest.fixture(scope="module")
def case():
    """One batch on the kernel's boundaries, its cascades and the float64 reference of every row, made once."""
    k = A.kernel_consts()
    P, Bk = k["piece"], k["block"]
    lengths = [0, 1, 2, P - 1, P, P + 1, Bk - 1, Bk, Bk + 1, 2 * Bk + 3, 2 * Bk + 3]
    pool = np.stack([edge_highpass(), A.peaking(SR, 3500.0, 5.0, 1.2), A.lowshelf(SR, 200.0, -6.0),
                     A.lowpass(SR, 9000.0, 0.9), A.highshelf(SR, 6000.0, 4.0), A.peaking(SR, 180.0, -6.0, 3.0),
                     A.highpass(SR, 60.0, 0.6), A.peaking(SR, 40.0, 9.0, 3.0)])
    counts = np.array([(0, 1, 3, 8)[r % 4] for r in range(len(lengths))], np.int32)
    counts[-1] = 8
    rng = np.random.default_rng(0)
    rows = [(0.1 * rng.standard_normal(n)).astype(f32) for n in lengths]
    rows[-1] = np.zeros(lengths[-1], f32)
    rows[-1][0] = 1.0                                           # a unit impulse through all eight stages
    sos = np.tile(np.asarray(A.IDENTITY), (len(lengths), 8, 1))
    for r, c in enumerate(counts):
        sos[r, :c] = pool[:c]
    refs = [R.cascade(x, sos[r, :counts[r]]) for r, x in enumerate(rows)]
    return dict(lengths=lengths, rows=rows, sos=sos, counts=counts, refs=refs, P=P, Bk=Bk)


def run_batch(case, dev, order=None, lead=0):
    """The rows packed back to back in ``order`` behind ``lead`` samples of another row; the results per row."""
    order = list(range(len(case["rows"]))) if order is None else order
    head = [np.full(lead, 0.5, f32)] if lead else []
    x = torch.from_numpy(np.concatenate(head + [case["rows"][r] for r in order] + [np.zeros(1, f32)])).to(dev)
    lengths = ([lead] if lead else []) + [case["lengths"][r] for r in order]
    sos = np.concatenate(([case["sos"][:1]] if lead else []) + [case["sos"][order]])
    counts = np.concatenate(([[2]] if lead else []) + [case["counts"][order]]).astype(np.int32)
    y = A.biquad_cascade(x, sos, counts, lengths).cpu().numpy()
    out, o = {}, lead
    for r in order:
        out[r] = y[o:o + case["lengths"][r]]
        o += case["lengths"][r]
    assert not y[o:].any()
    return out


@pytest.fixture(scope="module")
def batch(case, hip_device):
    return run_batch(case, hip_device)


def test_cascade_accuracy_on_the_kernels_boundaries(case, batch):
    worst_share, worst_abs = 0.0, 0.0
    for r, ref in enumerate(case["refs"]):
        got = batch[r].astype(np.float64)
        assert got.shape == ref.shape
        if ref.size == 0:
            continue
        top = np.max(np.abs(ref))
        err, bound = np.abs(got - ref), 2.0 ** -24 * np.abs(ref) + 2.0 ** -26 * top
        share = float(np.max(err / np.maximum(bound, 1e-300)))
        print(f"row {r}: n = {ref.size}, stages = {case['counts'][r]}, worst error / bound = {share:.3f}, "
              f"worst error / row max = 2^{math.log2(max(float(np.max(err)) / top, 1e-300)):.2f}")
        ulps = np.abs(bits(batch[r]).astype(np.int64) - bits(ref.astype(f32)).astype(np.int64))
        print(f"        {int((ulps > 0).sum())} of {ref.size} samples are not the rounded reference, by {int(ulps.max())} "
              "ulp at the most")
        worst_share, worst_abs = max(worst_share, share), max(worst_abs, float(np.max(err)) / top)
        assert np.all(err <= bound), (r, share)
        if case["counts"][r] == 0:
            assert np.array_equal(bits(batch[r]), bits(case["rows"][r]))
    print(f"worst error / bound = {worst_share:.3f}, worst error / row max = 2^{math.log2(worst_abs):.2f}")
    # the impulse row is the cascade's impulse response: it is not the input
    assert np.max(np.abs(case["refs"][-1][1:])) > 0


def test_cascade_is_bit_identical_across_layouts(case, batch, hip_device):
    n_rows = len(case["rows"])
    rev = run_batch(case, hip_device, order=list(range(n_rows))[::-1])
    odd = run_batch(case, hip_device, lead=3)
    width = max(case["lengths"])
    pad = np.full((n_rows, width), 0.25, f32)
    for r, x in enumerate(case["rows"]):
        pad[r, :x.size] = x
    padded = A.biquad_cascade(torch.from_numpy(pad).to(hip_device), case["sos"], case["counts"], case["lengths"])
    x_in = torch.from_numpy(pad).to(hip_device)
    assert A.biquad_cascade(x_in, case["sos"], case["counts"], case["lengths"], out=x_in) is x_in
    for r in range(n_rows):
        n, want = case["lengths"][r], bits(batch[r])
        assert np.array_equal(bits(rev[r]), want), r
        assert np.array_equal(bits(odd[r]), want), r
        assert np.array_equal(bits(padded[r, :n]), want) and not padded[r, n:].any(), r
        assert np.array_equal(bits(x_in[r, :n]), want), r                            # in place
        assert np.array_equal(bits(x_in[r, n:]), bits(pad[r, n:])), r                # and nothing past the row
        x = torch.from_numpy(np.concatenate([case["rows"][r], np.zeros(1, f32)])).to(hip_device)[:n]
        alone = A.biquad_cascade(x, case["sos"][r, :max(case["counts"][r], 1)], case["counts"][r])
        assert np.array_equal(bits(alone), want), r


def test_clip_rows_is_three_single_clips(hip_device):
    rng = np.random.default_rng(3)
    lengths = [5000, 4097, 777]
    rows = [(0.3 * rng.standard_normal(n)).astype(f32) for n in lengths]
    x = torch.from_numpy(np.concatenate(rows)).to(hip_device)
    percents = [0.0, 5.0, 20.0]
    y, thr = stress.apply_sample_clipping_rows(x, percents, lengths, return_threshold=True)
    o = 0
    for r, (n, pc) in enumerate(zip(lengths, percents)):
        one, t = stress.apply_sample_clipping(torch.from_numpy(rows[r]).to(hip_device), pc, return_threshold=True)
        assert np.array_equal(bits(y[o:o + n]), bits(one)), r
        assert np.array_equal(bits(thr[r:r + 1]), bits(t)), r
        o += n
    assert np.array_equal(bits(y[:5000]), bits(rows[0])) and math.isnan(float(thr[0]))
    assert float(thr[1]) > float(thr[2]) > 0 and float(y[5000:9097].abs().max()) == float(thr[1])


# ------------------------------------------------------------------------------------------------------------ the chain
def responses():
    rng = np.random.default_rng(5)
    return [(rng.standard_normal(n) * np.exp(-np.arange(n) / (n / 6.0))).astype(f32) for n in (900, 2500, 5000)]


def chain_config(p):
    return {"reverb": {"p": p, "responses": responses()}, "noise": {"p": p, "snr_db": [5.0, 20.0], "warmup": 512},
            "filter": {"p": p, "highpass": {"p": 1.0}}, "clipping": {"p": p, "percent": [1.0, 10.0]},
            "gain": {"p": p}, "polarity": {"p": p}}


@pytest.fixture(scope="module")
def waves(hip_device):
    rng = np.random.default_rng(9)
    lengths = [3001 + 397 * r for r in range(16)]
    pad = np.zeros((16, max(lengths)), f32)
    for r, n in enumerate(lengths):
        pad[r, :n] = 0.2 * rng.standard_normal(n)
    return torch.from_numpy(pad).to(hip_device), lengths


def test_apply_with_nothing_selected_is_the_input(waves):
    x, lengths = waves
    aug = A.Augmenter(chain_config(0.0), 24000, seed=1)
    y = aug.apply(x, lengths, aug.draw(16))
    assert y is not x and np.array_equal(bits(y), bits(x))


def test_apply_gain_alone_is_one_float32_multiply(waves):
    x, lengths = waves
    aug = A.Augmenter({"gain": {"p": 1.0, "gain_db": [6.0206, 6.0206]}}, 24000)
    y = aug.apply(x, lengths, aug.draw(16))
    g = f32(10.0 ** (6.0206 / 20.0))
    assert np.array_equal(bits(y), bits((x.cpu().numpy() * g).astype(f32)))
    flip = A.Augmenter({"polarity": {"p": 1.0}}, 24000)
    flipped, want = bits(flip.apply(x, lengths, flip.draw(16))), bits(-x.cpu().numpy())
    assert all(np.array_equal(flipped[r, :n], want[r, :n]) for r, n in enumerate(lengths))


def test_apply_touches_the_selected_rows_only(waves):
    x, lengths = waves
    cfg = chain_config(0.5)
    for seed in range(64):
        plan = A.Augmenter(cfg, 24000, seed=seed).draw(16)
        picks = [getattr(plan, f"{t}_on") for t in A.TRANSFORMS]
        if all(p.any() and not p.all() for p in picks) and not (plan.gain_on | plan.polarity_on).all():
            break
    else:
        pytest.fail("no seed below 64 selects some rows and not others for every transform")
    for p in picks:                                              # checked on the host plan
        assert 0 < int(p.sum()) < 16
    assert np.all(plan.n_stages[plan.filter_on] >= 1)
    aug = A.Augmenter(cfg, 24000, seed=seed)
    y, stages = aug.apply(x, lengths, aug.draw(16), return_stages=True)
    assert np.array_equal(bits(stages["gain"]), bits(y)) and np.array_equal(bits(stages["input"]), bits(x))
    chain = ["input", "reverb", "noise", "filter", "clipping", "gain"]
    selected = {"reverb": plan.reverb_on, "noise": plan.noise_on, "filter": plan.filter_on,
                "clipping": plan.clipping_on, "gain": plan.gain_on | plan.polarity_on}
    for before, name in zip(chain[:-1], chain[1:]):
        a, b = bits(stages[before]), bits(stages[name])
        for r, n in enumerate(lengths):
            same = np.array_equal(a[r, :n], b[r, :n])
            assert same != bool(selected[name][r]), (name, r)


def test_a_filter_only_plan_is_the_cascade(waves):
    x, lengths = waves
    aug = A.Augmenter({"filter": {"p": 1.0}}, 24000, seed=4)
    plan = aug.draw(16)
    assert plan.filter_on.all() and len(set(plan.n_stages.tolist())) > 1
    want = A.biquad_cascade(x, plan.sos, plan.n_stages, lengths)
    got = aug.apply(x, lengths, plan)
    assert np.array_equal(bits(got), bits(want)) and not np.array_equal(bits(got), bits(x))
    ref = R.cascade_f32(x[3, :lengths[3]].cpu().numpy(), plan.sos[3, :plan.n_stages[3]])
    top = float(np.max(np.abs(ref)))
    assert np.max(np.abs(got[3, :lengths[3]].cpu().numpy().astype(np.float64) - ref)) <= 2.0 ** -23 * top


# ------------------------------------------------------------------------------------------------------------ the loader
@pytest.fixture(scope="module")
def file_list(tmp_path_factory):
    from pitchextractor_amd import synthetic
    from tests.test_data_layer import write_wav
    root = tmp_path_factory.mktemp("augment_files")
    lines = []
    for i, dur in enumerate((2.0, 1.3, 0.9, 2.2)):
        wave, f0, _ = synthetic.utterance(i, duration=dur)
        p = root / f"u{i}.wav"
        write_wav(p, wave, 24000, "float32")
        np.save(str(p) + "_f0.npy", f0)
        lines.append(f"{p}|0\n")
    return lines


def batches(lines, augmentation, validation=False):
    from pitchextractor_amd import meldataset as md
    cfg = {"mel_params": {"sample_rate": 24000, "win_len": 1024, "n_fft": 1024, "n_mels": 80, "hop_length": 300},
           "dataloader": {"start_method": None}, "verbose": False}
    if augmentation is not None:
        cfg["augmentation"] = augmentation
    loader = md.build_dataloader(lines, validation=validation, batch_size=2, num_workers=0, device="cuda:0",
                                 dataset_config=cfg)
    np.random.seed(5)
    random.seed(5)
    torch.manual_seed(5)
    got = [tuple(t.cpu().numpy() for t in b) for b in loader]
    assert len(got) == 2
    return got


def same(a, b, parts=(0, 1, 2)):
    return all(np.array_equal(bits(x[k]), bits(y[k])) for x, y in zip(a, b) for k in parts)


def test_loader_stage(file_list, hip_device):
    full = {**chain_config(1.0), "seed": 1}
    plain = batches(file_list, None)
    assert same(plain, batches(file_list, {**full, "enabled": False}))
    on = batches(file_list, full)
    assert same(on, plain, parts=(1, 2))                        # f0s and is_silences
    assert all(not np.array_equal(a[0], b[0]) for a, b in zip(on, plain))
    assert all(np.isfinite(a[0]).all() for a in on)
    assert same(on, batches(file_list, full))
    other = batches(file_list, {**full, "seed": 2})
    assert same(other, plain, parts=(1, 2)) and not same(other, on, parts=(0,))
    assert same(batches(file_list, full, validation=True), batches(file_list, None, validation=True))
    asked = batches(file_list, {**full, "apply_to_validation": True}, validation=True)
    assert not same(asked, batches(file_list, None, validation=True), parts=(0,))

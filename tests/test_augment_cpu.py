"""The augmentation's host side without a device: the float64 restatement (tests/augment_ref.py) against scipy, the
coefficient designers, ``Augmenter.draw``, config validation, the C entry points' argument checks and the loader's
handling of the ``augmentation`` key."""
import ctypes
import math
import random

import numpy as np
import pytest
import scipy.signal

from pitchextractor_amd import _lib, augment as A, build
from tests import augment_ref as R

ARG = -1
SR = 24000


def random_stable_cascade(rng, stages):
    """Stages with poles at a random radius below the kernel's limit and a random angle, and random zeros."""
    sos = np.zeros((stages, 5))
    for s in range(stages):
        r, th = rng.uniform(0.2, R.MAX_POLE_RADIUS), rng.uniform(0.01, math.pi - 0.01)
        sos[s] = [*rng.uniform(-1.0, 1.0, 3), -2.0 * r * math.cos(th), r * r]
    return sos


@pytest.mark.parametrize("stages", [1, 3, 8])
def test_restatement_is_scipy_sosfilt(stages):
    rng = np.random.default_rng(stages)
    sos = random_stable_cascade(rng, stages)
    x = (0.1 * rng.standard_normal(700)).astype(np.float32)
    scipy_sos = np.concatenate([sos[:, :3], np.ones((stages, 1)), sos[:, 3:]], axis=1)
    want = scipy.signal.sosfilt(scipy_sos, x.astype(np.float64))
    got = R.cascade(x, sos)
    assert np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want))


def test_designers_hit_their_marks():
    half = 10.0 * math.log10(0.5)
    for sr in (16000, 24000, 48000):
        for f in (300.0, 1000.0, 5000.0):
            for gain in (-9.0, 4.5):
                assert abs(R.magnitude_db(A.peaking(sr, f, gain, 1.3), sr, f) - gain) <= 1e-9
                assert abs(R.magnitude_db(A.lowshelf(sr, f, gain), sr, 0.0) - gain) <= 1e-9
                assert abs(R.magnitude_db(A.lowshelf(sr, f, gain), sr, sr / 2.0)) <= 1e-9
                assert abs(R.magnitude_db(A.highshelf(sr, f, gain), sr, sr / 2.0) - gain) <= 1e-9
                assert abs(R.magnitude_db(A.highshelf(sr, f, gain), sr, 0.0)) <= 1e-9
            assert abs(R.magnitude_db(A.lowpass(sr, f, 1.0 / math.sqrt(2.0)), sr, f) - half) <= 1e-9
            assert abs(R.magnitude_db(A.highpass(sr, f, 1.0 / math.sqrt(2.0)), sr, f) - half) <= 1e-9


def test_designers_are_the_restated_cookbook():
    for name, args in (("lowpass", (SR, 3000.0, 0.8)), ("highpass", (SR, 120.0, 0.6)),
                       ("peaking", (SR, 900.0, -5.0, 2.0)), ("lowshelf", (SR, 250.0, 6.0, 0.7)),
                       ("highshelf", (SR, 4000.0, -7.0, 0.9))):
        got, want = getattr(A, name)(*args), getattr(R, name)(*args)
        assert got.dtype == np.float64 and got.shape == (5,)
        np.testing.assert_allclose(got, want, rtol=1e-14, atol=0)
        assert abs(A.pole_radius(got) - R.pole_radius(got)) <= 1e-12
        assert A.pole_radius(got) <= A.MAX_POLE_RADIUS


def test_pole_radius_refusal_names_the_stage():
    assert A.MAX_POLE_RADIUS == R.MAX_POLE_RADIUS
    with pytest.raises(ValueError, match=r"highpass\(sr=48000, f=2.0, Q=0.707\).*pole radius"):
        A.highpass(48000, 2.0, 0.707)
    A.highpass(48000, 3.0, 0.707)
    with pytest.raises(ValueError, match="row 1 stage 0"):
        A.cascade_table(np.array([[A.IDENTITY], [[1.0, 0.0, 0.0, -1.9999, 0.99995]]]), None, 2)


def test_default_ranges_fit_the_limit_at_16_to_48_khz():
    """Every corner of every default filter range is a stage the kernel takes."""
    for sr in (16000, 22050, 24000, 44100, 48000):
        cfg = A.check_config({"filter": {"p": 1.0}}, sr)["filter"]
        for kind in ("highpass", "lowpass", "peaking", "shelf"):
            sub = cfg[kind]
            for f in sub["f"]:
                for q in sub["Q"]:
                    for g in sub.get("gain_db", (0.0,)):
                        for low in (True, False):
                            assert A._try_stage(kind, sr, f, g, q, low) is not None, (sr, kind, f, q, g)


FULL = {"reverb": {"p": 0.5, "responses": [[1.0, 0.5], [1.0], [0.2, 0.1, 0.3]]}, "noise": {"p": 0.5},
        "filter": {"p": 0.5}, "clipping": {"p": 0.5}, "gain": {"p": 0.5}, "polarity": {"p": 0.5}}


def plans_equal(a, b):
    return all(np.array_equal(getattr(a, k), getattr(b, k)) for k in a.__dataclass_fields__)


def test_draw_is_seeded_and_leaves_the_global_generators_alone():
    random.seed(1)
    np.random.seed(1)
    before = random.getstate(), np.random.get_state()
    p0 = A.Augmenter(FULL, SR, seed=7, rank=0).draw(16)
    p1 = A.Augmenter(FULL, SR, seed=7, rank=0).draw(16)
    assert plans_equal(p0, p1)
    assert not plans_equal(p0, A.Augmenter(FULL, SR, seed=8, rank=0).draw(16))
    assert not plans_equal(p0, A.Augmenter(FULL, SR, seed=7, rank=1).draw(16))
    after = random.getstate(), np.random.get_state()
    assert before[0] == after[0]
    assert all(np.array_equal(x, y) for x, y in zip(before[1], after[1]))
    # a second batch continues the stream
    a = A.Augmenter(FULL, SR, seed=7)
    assert plans_equal(a.draw(16), p0) and not plans_equal(a.draw(16), p0)
    assert p0.n_stages.max() <= A.MAX_STAGES and p0.sos.shape == (16, 8, 5)
    assert np.all((p0.rir_index >= 0) & (p0.rir_index < 3))


@pytest.mark.parametrize("off", A.TRANSFORMS)
def test_disabling_one_transform_leaves_the_others_draws(off):
    full = A.Augmenter(FULL, SR, seed=11).draw(32)
    cfg = {k: v for k, v in FULL.items() if k != off}
    part = A.Augmenter(cfg, SR, seed=11).draw(32)
    assert not getattr(part, f"{off}_on").any() and getattr(full, f"{off}_on").any()
    values = {"reverb": (), "noise": ("noise_colour", "snr_db", "noise_seed"), "filter": ("n_stages", "sos"),
              "clipping": ("clip_percent",), "gain": ("gain_db",), "polarity": ()}
    # reverb's index needs the responses, which leave with the transform
    skip = {f"{off}_on", *values[off]} | ({"rir_index"} if off == "reverb" else set())
    for k in full.__dataclass_fields__:
        if k not in skip:
            assert np.array_equal(getattr(full, k), getattr(part, k)), k
    # switched off as a whole: the same values, nothing selected
    none = A.Augmenter({**FULL, "enabled": False}, SR, seed=11).draw(32)
    assert not any(getattr(none, f"{t}_on").any() for t in A.TRANSFORMS)
    assert np.array_equal(none.snr_db, full.snr_db) and np.array_equal(none.gain_db, full.gain_db)


def test_plan_factors_and_without():
    plan = A.Augmenter({"gain": {"p": 0.5, "gain_db": [6.0206, 6.0206]}, "polarity": {"p": 0.5}}, SR, seed=2).draw(32)
    g = plan.factors()
    assert g.dtype == np.float32
    want = np.float32(10.0 ** (6.0206 / 20.0))
    for r in range(32):
        assert g[r] == (want if plan.gain_on[r] else np.float32(1.0)) * (-1 if plan.polarity_on[r] else 1)
    cut = plan.without([0, 5])
    assert not cut.gain_on[[0, 5]].any() and not cut.polarity_on[[0, 5]].any()
    assert np.array_equal(cut.gain_on[6:], plan.gain_on[6:])


@pytest.mark.parametrize("bad", [
    {"reverbb": {"p": 0.1}}, {"noise": {"p": 1.5}}, {"noise": {"p": 0.5, "snr_db": [30.0, 10.0]}},
    {"noise": {"colours": ["white", "violet"]}}, {"noise": {"colours": []}}, {"noise": {"snr": [1, 2]}},
    {"clipping": {"percent": [0.0, 120.0]}}, {"gain": {"gain_db": [0.0, float("inf")]}}, {"gain": {"gain_db": "loud"}},
    {"filter": {"p": 1.0, "peaking": {"count": [0, 9]}}}, {"filter": {"p": 1.0, "lowpass": {"f": [2000.0, 12000.0]}}},
    {"filter": {"p": 1.0, "highpass": {"f": [0.2, 0.5]}}}, {"filter": {"p": 1.0, "shelf": {"Q": [0.0, 1.0]}}},
    {"filter": {"bandpass": {}}}, {"reverb": {"p": 0.5}}, {"reverb": {"p": 0.5, "library": "cathedral"}},
    {"reverb": {"p": 0.5, "files": []}}, {"polarity": 0.5}, ["noise"],
])
def test_config_validation(bad):
    with pytest.raises(ValueError, match="augmentation"):
        A.Augmenter(bad, SR)


def test_config_defaults():
    a = A.Augmenter({}, SR)
    assert not a.active and not a.draw(3).noise_on.any()
    assert A.Augmenter({"gain": {"p": 0.2}}, SR).active
    assert not A.Augmenter({"enabled": False, "gain": {"p": 0.2}}, SR).active
    cfg = A.check_config(None, SR)
    assert cfg["apply_to_validation"] is False and cfg["apply_to_synthetic"] is True and cfg["seed"] == 0


def test_wrappers_refuse_host_tensors():
    import torch
    x = torch.zeros(64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.biquad_cascade(x, [A.IDENTITY])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.apply_gain(x, 1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.Augmenter({}, SR).apply(x, None, A.Augmenter({}, SR).draw(1))


@pytest.fixture(scope="module")
def lib():
    build.build_library(verbose=False)
    return _lib.load()


def test_entry_points_check_their_arguments_before_any_device_call(lib):
    """Device pointers are host buffers or null throughout and no GPU is present: every answer is the host's."""
    consts = np.zeros(3, np.int64)
    assert lib.pe_augment_biquad_consts(consts.ctypes.data) == 0
    P, Bk, S = (int(v) for v in consts)
    assert (P, S) == (A.kernel_consts()["piece"], A.MAX_STAGES) and Bk % P == 0 and Bk // P == 256
    assert lib.pe_augment_biquad_consts(None) == ARG
    buf = ctypes.cast((ctypes.c_float * 64)(), ctypes.c_void_p)
    meta = np.array([[0, 8], [8, 5]], np.int64)
    sos = np.tile(np.asarray(A.IDENTITY), (2, 8, 1))
    count = np.array([1, 8], np.int32)
    p = lambda a: a.ctypes.data  # noqa: E731

    def call(x=buf, m=buf, hm=meta, K=2, R=2, s=buf, hs=sos, c=buf, hc=count, y=buf):
        return lib.pe_augment_biquad(x, m, None if hm is None else p(hm), K, R, s, None if hs is None else p(hs), c,
                                     None if hc is None else p(hc), y, None)

    for null in ("x", "m", "s", "c", "y", "hm", "hs", "hc"):
        assert call(**{null: None}) == ARG, null
    assert call(K=1) == ARG and call(R=-1) == ARG and call(R=65536) == ARG
    for bad_count in (-1, 9):
        assert call(hc=np.array([1, bad_count], np.int32)) == ARG
    neg = meta.copy()
    neg[1, 1] = -1
    assert call(hm=neg) == ARG
    off = meta.copy()
    off[0, 0] = -4
    assert call(hm=off) == ARG
    for stage in ([1.0, 0.0, math.nan, 0.0, 0.0], [math.inf, 0.0, 0.0, 0.0, 0.0], [1.0, 0.0, 0.0, -2.0, 1.0],
                  [1.0, 0.0, 0.0, 0.0, 1.0], [1.0, 0.0, 0.0, 2.1, 1.05], [1.0, 0.0, 0.0, -1.9999, 0.99995],
                  [1.0, 0.0, 0.0, -0.9999, 0.0], [1.0, 0.0, 0.0, 0.0, 0.9999]):
        bad = sos.copy()
        bad[1, 7] = stage
        assert call(hs=bad) == ARG, stage
        bad = sos.copy()
        bad[0, 1] = stage                                   # past the row's one stage: not read
        assert call(hs=bad, x=None) == ARG and call(hs=bad, hm=np.zeros((2, 2), np.int64), x=None) == 0
    # just inside the limit, and nothing to do
    edge = sos.copy()
    r = A.MAX_POLE_RADIUS
    edge[1, 0] = [1.0, 0.0, 0.0, 0.0, r * r * (1 - 1e-15)]
    assert call(hs=edge, hm=np.zeros((2, 2), np.int64), x=None, y=None) == 0
    assert lib.pe_augment_biquad(None, None, None, 2, 0, None, None, None, None, None, None) == 0

    gains = np.array([1.0, -2.0], np.float32)
    g = lambda **kw: lib.pe_augment_gain(kw.get("x", buf), buf, p(kw.get("hm", meta)), kw.get("K", 2), 2,  # noqa: E731
                                         kw.get("g", buf), kw.get("hg", p(gains)), kw.get("y", buf), None)
    assert g(x=None) == ARG and g(y=None) == ARG and g(g=None) == ARG and g(hg=None) == ARG and g(K=0) == ARG
    assert g(hg=p(np.array([1.0, math.nan], np.float32))) == ARG and g(hm=neg) == ARG

    stress_meta = np.zeros((2, lib.pe_stress_plan_fields()), np.int64)
    n, o = np.array([8, 5], np.int64), np.array([0, 8], np.int64)
    assert lib.pe_stress_plan(2, p(n), p(o), p(o), p(np.zeros(4, np.int64)), p(stress_meta),
                              p(np.zeros(2, np.int64))) == 0
    q, copy = np.array([0.9, 0.5]), np.array([0, 1], np.int32)

    def clip(x=buf, hm=stress_meta, q_d=buf, hq=q, c_d=buf, hc=copy, y=buf):
        return lib.pe_stress_clip_rows(x, buf, p(hm), 2, q_d, None if hq is None else p(hq), c_d,
                                       None if hc is None else p(hc), y, None, None)

    for null in ("x", "q_d", "hq", "c_d", "hc", "y"):
        assert clip(**{null: None}) == ARG, null
    assert clip(hq=np.array([1.5, 0.5])) == ARG and clip(hq=np.array([math.nan, 0.5])) == ARG
    assert clip(hq=np.array([0.9, 7.0]), x=None) == ARG           # a copy's q is not read; the null x answers
    assert clip(hm=meta) == ARG                                    # not a stress plan


def test_build_dataloader_pops_the_augmentation_key(monkeypatch):
    """The dataset is built without the key, and the loader gets the Augmenter: seeded with (seed, rank), none for a
    disabled block or a validation loader that did not ask."""
    from pitchextractor_amd import meldataset as md
    seen = {}

    class Dataset(md.MelDataset):
        def __init__(self, path_list, **kw):
            seen["kwargs"] = dict(kw)
            super().__init__(path_list, **kw)

    monkeypatch.setattr(md, "MelDataset", Dataset)
    monkeypatch.setattr(md, "DataLoader", lambda dataset, **kw: type("L", (), {"dataset": dataset})())
    monkeypatch.setattr(A.Augmenter, "prepare", lambda self, device: self)
    aug = {"seed": 9, "gain": {"p": 1.0}}
    cfg = {"verbose": False, "augmentation": aug}

    def loader(config, validation=False, shard=None):
        return md.build_dataloader([], validation=validation, batch_size=2, num_workers=0, device="cuda:0",
                                   dataset_config=config, shard=shard)

    got = loader(cfg, shard=(3, 4, 0))
    assert "augmentation" not in seen["kwargs"] and "augmentation" in cfg
    assert isinstance(got.augmenter, A.Augmenter)
    assert plans_equal(got.augmenter.draw(4), A.Augmenter(aug, 24000, seed=9, rank=3).draw(4))
    assert loader({"verbose": False}).augmenter is None
    assert loader({"verbose": False, "augmentation": {**aug, "enabled": False}}).augmenter is None
    assert loader(cfg, validation=True).augmenter is None
    assert loader({"verbose": False, "augmentation": {**aug, "apply_to_validation": True}},
                  validation=True).augmenter is not None
    with pytest.raises(ValueError, match="augmentation"):
        loader({"verbose": False, "augmentation": {"pitch": {}}})
    with pytest.raises(TypeError):
        md.MelDataset([], verbose=False, augmentation=aug)

"""The additive-noise path without a GPU: the restatement in tests/noise_ref.py against published and independent
answers (Philox known answer, normal statistics, ``scipy.signal.lfilter``, the pink response), the summary table, and
every refusal of the C entry points and of the Python layer, none of which reaches the device."""
import ctypes
import math

import numpy as np
import pytest

from tests import noise_ref as R

f32 = np.float32


def test_philox_known_answer():
    """Philox4x32-10 with a zero key and a zero counter: the published known answer of the Random123 test vectors."""
    assert [f"{w:08x}" for w in R.philox4x32(0, [0])[0]] == ["6627e8d5", "e169c58d", "bc57ac4c", "9b00dbd8"]
    # counter and key halves land where common.h puts them: {lo, hi, 0, 0} and {seed lo, seed hi}
    both = R.philox4x32((7 << 32) | 5, [(3 << 32) | 9, 1])
    assert both.shape == (2, 4) and len({tuple(r) for r in both}) == 2
    assert not np.array_equal(R.philox4x32(5, [9]), R.philox4x32((7 << 32) | 5, [9]))
    assert not np.array_equal(R.philox4x32(5, [9]), R.philox4x32(5, [(3 << 32) | 9]))
    assert np.array_equal(R.philox4x32(-1, [4]), R.philox4x32(2 ** 64 - 1, [4]))


@pytest.mark.parametrize("seed", [0, 7, 1234])
def test_normal_statistics(seed):
    N = 1 << 16
    z = R.white(N, seed)
    mean, var = float(np.mean(z)), float(np.var(z))
    print(f"seed {seed}: |mean| {abs(mean):.3e} (bound {5 / math.sqrt(N):.3e}), |var - 1| {abs(var - 1):.3e} "
          f"(bound {5 * math.sqrt(2 / N):.3e})")
    assert abs(mean) <= 5 / math.sqrt(N)
    assert abs(var - 1.0) <= 5 * math.sqrt(2.0 / N)
    u1, u2 = R.uniforms(seed, np.arange(N))
    assert u1.min() > 0.0 and u1.max() < 1.0 and u2.min() >= 0.0 and u2.max() < 1.0
    assert np.array_equal(u2.astype(f32).astype(np.float64), u2)
    dev = float(np.max(np.abs(R.randn32_numpy(seed, np.arange(N)).astype(np.float64) - z)))
    print(f"seed {seed}: max |numpy float32 - float64| over {N} draws {dev:.3e}")
    assert dev < 1e-3                                      # at worst u1 rounds to 1: sqrt(2^-24) = 2.4e-4
    assert np.array_equal(R.white(100, seed, warmup=50), z[50:150])                # sample i is generated sample warmup + i


def test_recurrence_against_scipy():
    from scipy.signal import lfilter
    from pitchextractor_amd import noise as N
    rng = np.random.default_rng(3)
    w = rng.standard_normal(6149)
    custom = {"d0": 0.3, "d1": -0.2, "sections": [(0.999, 0.01), (0.9, 0.2), (-0.8, 0.1), (0.5, 0.3), (0.25, -0.4),
                                                  (0.99, 0.02), (0.7, 0.05), (-0.3, 0.6)]}
    for colour in ("white", "pink", "brown", custom):
        d0, d1, sections = N.colour_sections(colour, 24000)
        want = sum(lfilter(b, a, w) for b, a in R.lfilter_form(d0, d1, sections))
        state, before, got = [0.0] * len(sections), 0.0, np.zeros(w.size)
        for j, v in enumerate(w.tolist()):                                          # colour() before its float32 rounding
            acc = d0 * v + d1 * before
            for k, (a, b) in enumerate(sections):
                state[k] = a * state[k] + b * v
                acc += state[k]
            got[j], before = acc, v
        err = float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
        print(f"{colour if isinstance(colour, str) else 'custom'}: max |recurrence - lfilter| / max |lfilter| {err:.3e}")
        assert err <= 1e-12
        assert np.array_equal(R.colour(w, d0, d1, sections, warmup=100), got[100:].astype(f32))


@pytest.mark.parametrize("sr", [16000, 24000, 48000])
def test_pink_response(sr):
    from pitchextractor_amd import noise as N
    d0, d1, sections = N.colour_sections("pink", sr)
    assert (d0, d1, tuple(sections)) == R.PINK
    f = np.geomspace(sr / 2000.0, sr / 2.2, 4096)
    flat = R.response_db(d0, d1, sections, f, sr) + 10.0 * np.log10(f)              # -3 dB / octave taken out
    ripple = float(flat.max() - flat.min())
    print(f"{sr} Hz: pink response within {ripple:.4f} dB peak to peak of -3 dB / octave")
    assert ripple <= 0.1


def test_colours():
    from pitchextractor_amd import noise as N
    assert N.NOISE_COLOURS == ("white", "pink", "brown")
    assert N.colour_sections("white", 24000) == (1.0, 0.0, [])
    assert N.colour_sections("brown", 24000) == (0.0, 0.0, [(math.exp(-2.0 * math.pi * 20.0 / 24000), 1.0)])
    assert N.colour_sections({"d0": 2.0, "sections": [(0.5, 1.0)]}, 8000) == (2.0, 0.0, [(0.5, 1.0)])
    for bad in ("violet", 3, {"sections": [(1.0, 1.0)]}, {"sections": [(-1.0, 1.0)]}, {"sections": [(0.5, math.nan)]},
                {"d0": math.inf}, {"sections": [(0.5, 1.0)] * 9}):
        with pytest.raises(ValueError):
            N.colour_sections(bad, 24000)
    with pytest.raises(ValueError):
        N.colour_sections("pink", 0)
    assert N.row_seeds(5, 3).tolist() == [5, 6, 7] and N.row_seeds([9, 2], 2).tolist() == [9, 2]
    assert N.row_seeds(2 ** 63, 1).tolist() == [-2 ** 63]                          # the same 64 bits
    with pytest.raises(ValueError):
        N.row_seeds([1, 2], 3)


def test_bed_and_mix_restatement():
    rec = np.arange(5, dtype=f32)
    assert R.bed(rec, 12, 3).tolist() == [3, 4, 0, 1, 2, 3, 4, 0, 1, 2, 3, 4]
    assert R.bed(rec[:1], 4, 0).tolist() == [0, 0, 0, 0] and R.bed(rec, 0, 4).size == 0
    rng = np.random.default_rng(11)
    x = (0.1 * np.sin(np.arange(4000) * 0.05)).astype(f32)
    z = rng.standard_normal(4000).astype(f32)
    for snr in (-5.0, 0.0, 20.0, 60.0):
        y, st = R.mix(x, z, snr, peak_normalize=False)
        got = 20.0 * math.log10(st[1] / (st[3] * st[2]))
        assert abs(got - snr) <= 1e-5                                               # float32 scale alone: 5e-7 dB
        assert np.array_equal(y, x + z * f32(st[3])) and st[0] == float(np.max(np.abs(y)))
    y, st = R.mix(x * f32(9.0), z, 0.0)
    assert st[0] > 0.99 and np.array_equal(y, (x * f32(9.0) + z * f32(st[3])) / f32(st[0] + 1e-6))
    for a, b in ((np.zeros(100, f32), z[:100]), (x[:100], np.zeros(100, f32))):
        y, st = R.mix(a, b, 10.0)
        assert np.array_equal(y, a) and st[3] == 0.0
    y, st = R.mix(np.zeros(0, f32), np.zeros(0, f32), 10.0)
    assert y.size == 0 and st.tolist() == [0.0, 0.0, 0.0, 0.0]


def _records():
    nan = math.nan
    rows = [("white", 20.0, 0, 0.9, 0.95, 0.99, 0.01), ("white", 20.0, 1, 0.7, nan, 0.97, 0.05),
            ("white", 20.0, 2, nan, nan, 0.96, nan), ("white", 0.0, 0, 0.4, 0.6, 0.8, 0.2),
            ("white", 0.0, 1, 0.2, 0.5, 0.7, 0.3), ("white", 0.0, 2, 0.3, nan, 0.75, 0.1),
            ("pink", 20.0, 0, 0.85, 0.9, 0.98, 0.02),                               # a group of one item
            ("brown", 0.0, 0, nan, nan, 0.5, nan), ("brown", 0.0, 1, nan, nan, 0.6, nan)]   # metrics that are all NaN
    keys = ("source", "snr_db", "item", "RPA", "RCA", "VUV", "OctaveError")
    records = [dict(zip(keys, row)) for row in rows]
    baseline = [dict(item=0, RPA=0.95, RCA=0.97, VUV=1.0, OctaveError=0.0),
                dict(item=1, RPA=0.9, RCA=nan, VUV=0.98, OctaveError=0.02),
                dict(item=2, RPA=nan, RCA=nan, VUV=0.99, OctaveError=nan)]
    return records, baseline


def test_summary_table():
    """``inference.summarize_with_drop`` against the plain-loop restatement and, group by group, against what a pandas
    ``groupby(...).agg(["mean", "std"])`` with the baseline's column means gives (the notebooks' own tools) where pandas is
    installed."""
    from pitchextractor_amd import inference
    records, baseline = _records()
    keys, metrics = ("source", "snr_db"), ("RPA", "RCA", "VUV", "OctaveError")
    got = inference.summarize_with_drop(records, baseline, keys)
    want = R.summarize_with_drop(records, baseline, keys)
    assert [(g["source"], g["snr_db"]) for g in got] == [("white", 20.0), ("white", 0.0), ("pink", 20.0), ("brown", 0.0)]
    assert len(got) == len(want)
    same = lambda a, b: (math.isnan(a) and math.isnan(b)) or abs(a - b) <= 1e-15 * max(1.0, abs(b))  # noqa: E731
    for g, w in zip(got, want):
        assert list(g) == list(w)
        assert all(same(g[k], w[k]) if isinstance(w[k], float) and k not in keys else g[k] == w[k] for k in w)
    pink = got[2]
    assert math.isnan(pink["RPA_std"]) and pink["RPA_mean"] == 0.85 and math.isnan(got[3]["RPA_mean"])
    assert math.isnan(got[0]["RCA_std"]) and got[0]["RCA_mean"] == 0.95             # one value left after the NaN
    assert inference.summarize_with_drop(records, baseline, "source")[0]["source"] == "white"
    try:
        import pandas as pd
    except ImportError:                                                             # the notebooks' tool is optional here
        return
    frame, base = pd.DataFrame(records), pd.DataFrame(baseline)[list(metrics)].mean()
    table = frame.groupby(list(keys))[list(metrics)].agg(["mean", "std"])
    for g in got:
        line = table.loc[(g["source"], g["snr_db"])]
        for m in metrics:
            assert same(g[m + "_mean"], float(line[(m, "mean")])) and same(g[m + "_std"], float(line[(m, "std")]))
            drop = float(line[(m, "mean")]) - base[m] if m == "OctaveError" else base[m] - float(line[(m, "mean")])
            assert same(g[m + "_drop"], float(drop))


def test_condition_validation():
    from pitchextractor_amd import noise as N, stress
    assert "additive_noise" in stress.CONDITION_KINDS and "noise" not in stress.CONDITION_KINDS
    with pytest.raises(ValueError, match="snr_db"):
        stress.Condition("additive_noise", "x")
    for bad in (math.nan, math.inf, [10.0, math.nan]):
        with pytest.raises(ValueError, match="finite"):
            stress.Condition("additive_noise", "x", snr_db=bad)
    for bad in ("violet", 7, {"sections": [(1.5, 1.0)]}):
        with pytest.raises(ValueError):
            stress.Condition("additive_noise", "x", snr_db=10.0, source=bad)
    with pytest.raises(ValueError):
        stress.Condition("noise", "x", snr_db=10.0)
    bed = N.NoiseSet([np.ones(5, f32)], device="cuda")                              # host data only until it is used
    for ok in (dict(snr_db=10), dict(snr_db=[10.0, 0.0]), dict(snr_db=-5.0, source="pink", seed=3),
               dict(snr_db=0.0, source={"d0": 1.0, "sections": [(0.5, 1.0)]}), dict(snr_db=0.0, source=bed)):
        assert stress.Condition("additive_noise", "x", **ok).kind == "additive_noise"
    with pytest.raises(ValueError):
        N.NoiseSet([])
    with pytest.raises(ValueError):
        N.NoiseSet([np.zeros(0, f32)])


def test_argument_checks_run_before_any_device_call():
    from pitchextractor_amd import _lib, noise as N
    lib = _lib.load()
    p = lambda a: ctypes.cast(a, ctypes.c_void_p)  # noqa: E731
    buf = p((ctypes.c_double * 128)())
    ARG, WS = -1, -3
    assert lib.pe_noise_plan_fields() == 8 and lib.pe_noise_param_fields() == 100
    pl = N.plan_rows([0, 1, 7, 2049, 3 * 2048 + 5], warmup=5, seeds=3, colour="pink", sr=24000)
    assert pl["piece"] == R.PIECE and pl["stat_fields"] == 4 and pl["bed_fields"] == 3
    assert pl["meta"][:, 4].tolist() == [0, 1, 1, 2, 4] and pl["meta"][:, 5].tolist() == [0, 0, 1, 2, 4]
    assert pl["meta"][:, 6].tolist() == [3, 4, 5, 6, 7] and pl["n_samples"] == 8206 and pl["n_pieces"] == 8
    # the colour table: a^(8 2^m) and a^2048 of every section, to rounding
    prm = pl["params"]
    assert prm[:3].tolist() == [R.PINK[0], R.PINK[1], 6.0]
    for k, (a, b) in enumerate(R.PINK[2]):
        q = prm[4 + 12 * k:16 + 12 * k]
        assert q[0] == a and q[1] == b and q[11] == 0.0
        assert np.allclose(q[2:11], [a ** (8 * 2 ** m) for m in range(9)], rtol=1e-12, atol=0.0)
    meta, params, R_ = pl["meta"].ctypes.data, prm.ctypes.data, pl["rows"]
    ws_bytes = lib.pe_noise_workspace_bytes(pl["n_pieces"])
    assert ws_bytes == pl["n_pieces"] * 64 and lib.pe_noise_workspace_bytes(0) == 0

    # the C plan refuses what the Python layer refuses
    L = ctypes.c_long
    one = lambda v: p((L * 1)(v))  # noqa: E731
    co = lambda *v: p((ctypes.c_double * 20)(*v))  # noqa: E731
    plan = lambda n=10, off=0, warm=0, woff=-1, c=co(1.0, 0.0, 0.5, 1.0), ns=1: lib.pe_noise_plan(  # noqa: E731
        1, one(n), one(off), one(warm), one(0), one(woff), c, ns, buf, buf, buf, buf)
    assert plan() == 0 and plan(n=0) == 0 and plan(ns=0) == 0 and plan(c=co(1.0, 0.0, -0.999, 1.0)) == 0
    assert plan(n=-1) == ARG and plan(off=-1) == ARG and plan(warm=-1) == ARG and plan(woff=-2) == ARG
    assert plan(n=1 << 31) == ARG and plan(n=1 << 30, warm=1 << 30) == ARG
    assert plan(c=co(1.0, 0.0, 1.0, 1.0)) == ARG and plan(c=co(1.0, 0.0, -1.0, 1.0)) == ARG        # |a| >= 1
    assert plan(c=co(1.0, 0.0, 1.5, 1.0)) == ARG and plan(c=co(1.0, 0.0, math.nan, 1.0)) == ARG
    assert plan(c=co(1.0, 0.0, 0.5, math.inf)) == ARG and plan(c=co(math.nan, 0.0, 0.5, 1.0)) == ARG
    assert plan(c=co(1.0, -math.inf, 0.5, 1.0)) == ARG
    assert plan(c=co(1.0, 0.0, *([0.5, 1.0] * 9)), ns=9) == ARG and plan(ns=-1) == ARG and plan(c=None) == ARG
    assert plan(c=co(1.0, 0.0, *([0.5, 1.0] * 8)), ns=8) == 0
    assert lib.pe_noise_plan(1, None, None, None, None, None, co(1.0, 0.0), 0, buf, buf, buf, buf) == ARG
    for colour in ({"sections": [(1.0, 1.0)]}, {"sections": [(0.5, 1.0)] * 9}, {"d1": math.nan}):
        with pytest.raises(ValueError):
            N.plan_rows([10], colour=colour)
    for kw in (dict(lengths=[-1]), dict(lengths=[5], warmup=-1), dict(lengths=[5], offsets=[0, 1]),
               dict(lengths=[5, 5], warmup=[1]), dict(lengths=[5, 5], seeds=[1])):
        with pytest.raises(ValueError):
            N.plan_rows(**kw)

    def broken(field, value, row=3):
        bad = pl["meta"].copy()
        bad[row, field] = value
        return bad

    beds = (L * 15)(*([0, 5, 4] * 5))
    snr = (ctypes.c_double * 5)(10.0, 0.0, -5.0, 20.0, 60.0)

    def white(m=meta, md=buf, rows=R_, y=buf):
        return lib.pe_noise_white(md, m, rows, y, None)

    def colour(m=meta, md=buf, pd=buf, hp=params, w=None, nw=0, rows=R_, y=buf, ws=buf, wb=ws_bytes):
        return lib.pe_noise_colour(md, m, pd, hp, w, nw, rows, y, ws, wb, None)

    def bed(m=meta, md=buf, audio=buf, nb=5, bd=buf, hb=p(beds), rows=R_, y=buf):
        return lib.pe_noise_bed(md, m, audio, nb, bd, hb, rows, y, None)

    def mix(m=meta, x=buf, z=buf, md=buf, sd=buf, hs=p(snr), rows=R_, y=buf, st=buf, ws=buf, wb=ws_bytes):
        return lib.pe_noise_mix(x, z, md, m, sd, hs, 1, rows, y, st, ws, wb, None)

    # a plan that is not pe_noise_plan's
    for bad in (broken(1, -1), broken(0, -1), broken(2, -1), broken(3, 2000), broken(4, 9), broken(5, 1),
                broken(7, -2), broken(4, 1, row=0), broken(1, 1 << 31)):
        b = bad.ctypes.data
        assert white(m=b) == ARG and colour(m=b) == ARG and bed(m=b) == ARG and mix(m=b) == ARG
    for fn in (white, colour, bed, mix):
        assert fn(m=None) == ARG and fn(md=None) == ARG and fn(y=None) == ARG
        assert fn(rows=-1) == ARG and fn(rows=65536) == ARG
    # the colour table: a copy that pe_noise_plan did not make, a pole on the unit circle, too many sections
    for at, value in ((2, 9.0), (2, 2.5), (2, -1.0), (4, 1.0), (4, -1.0), (4, 1.25), (5, math.nan), (0, math.inf),
                      (6, 0.5), (14, 0.5), (3, 1.0)):
        bad = prm.copy()
        bad[at] = value
        assert colour(hp=bad.ctypes.data) == ARG
    assert colour(hp=None) == ARG and colour(pd=None) == ARG
    assert colour(ws=None, wb=0) == WS and colour(wb=ws_bytes - 1) == WS
    # a given white input that is missing or too short for warm-up + n
    given = N.plan_rows([7, 100], warmup=5, white_offsets=[0, 12], colour="brown", sr=24000)
    gm, gp, gw = given["meta"].ctypes.data, given["params"].ctypes.data, lib.pe_noise_workspace_bytes(given["n_pieces"])
    assert lib.pe_noise_colour(buf, gm, buf, gp, None, 117, 2, buf, buf, gw, None) == ARG
    assert lib.pe_noise_colour(buf, gm, buf, gp, buf, 116, 2, buf, buf, gw, None) == ARG
    # beds: L >= 1, 0 <= start < L, inside the bed audio, a table
    for at, value in ((1, 0), (2, 5), (2, -1), (0, -1), (0, 1), (1, 6), (4, 7)):
        bad = (L * 15)(*([0, 5, 4] * 5))
        bad[at] = value
        assert bed(hb=p(bad)) == ARG
    assert bed(hb=None) == ARG and bed(bd=None) == ARG and bed(audio=None) == ARG and bed(nb=4) == ARG
    # the mix: a finite snr_db per row, every pointer, the workspace
    for bad in (math.nan, math.inf, -math.inf):
        assert mix(hs=p((ctypes.c_double * 5)(10.0, 0.0, bad, 20.0, 60.0))) == ARG
    assert mix(hs=None) == ARG and mix(sd=None) == ARG and mix(x=None) == ARG and mix(z=None) == ARG
    assert mix(st=None) == ARG and mix(ws=None, wb=0) == WS and mix(wb=8) == WS
    # nothing to do is not an error, and needs no pointer
    empty = N.plan_rows([0, 0], warmup=7)
    em = empty["meta"].ctypes.data
    assert empty["n_pieces"] == 0
    assert lib.pe_noise_white(None, em, 2, None, None) == 0 and lib.pe_noise_white(None, None, 0, None, None) == 0
    assert lib.pe_noise_colour(None, em, None, params, None, 0, 2, None, None, 0, None) == 0
    assert lib.pe_noise_colour(None, None, None, params, None, 0, 0, None, None, 0, None) == 0
    assert lib.pe_noise_bed(None, em, None, 0, None, None, 2, None, None) == 0
    assert lib.pe_noise_mix(None, None, None, em, None, None, 1, 2, None, None, None, 0, None) == 0


def test_host_tensors_are_refused():
    import torch
    from pitchextractor_amd import noise as N, stress
    x = torch.zeros(4800)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        N.mix_at_snr(x, x, 10.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        N.mix_at_snr(np.zeros(4800, f32), np.zeros(4800, f32), 10.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        stress.apply_additive_noise(x, 24000, 10.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        stress.apply_condition(stress.Condition("additive_noise", "x", snr_db=10.0), x, 24000)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        N.white([100], 0, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        N.coloured([100], "pink", 24000, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        N.coloured([100], "pink", 24000, white=torch.zeros(4196))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        N.bed(N.NoiseSet([np.ones(5, f32)], device="cpu"), [100])
    with pytest.raises(ValueError):
        N.coloured([100], "pink", 24000, seeds=1, white=torch.zeros(4196))
    bed = N.NoiseSet([np.ones(5, f32), np.ones(3, f32)])
    for kw in (dict(index=2), dict(index=-1), dict(index=1, start=3), dict(start=-1), dict(index=[0, 1])):
        with pytest.raises(ValueError):
            N.bed(bed, [100], **kw)

"""F0 bin decoding without a GPU: the float64 restatement against brute force and the loss's bin grid, the metrics
restatement against the reference's recorded results, and the host-side argument checks of the new entry points."""
import ctypes
import inspect
from pathlib import Path

import numpy as np
import pytest

from oracle import model_ref
from pitchextractor_amd import _lib, build
from tests import f0_decode_ref as ref

GOLDEN = Path(__file__).resolve().parent / "golden" / "pitch_metrics_golden.npz"


def metrics_f32_tolerance(pred, ref_hz):
    """What the reference's float32 ``hz_to_cents`` may lose against float64 on these tracks, in cents.

    A cents value is ``1200 * log2(f / 55)`` in float32: the division rounds (2^-24 relative, i.e. 1.4427 * 2^-24
    absolute in the logarithm), the logarithm is allowed one ulp (2^-23 of its value), the product and the
    assignment into the float32 array round once more (2^-24 of the value): at most
    ``1200 * 1.4427 * 2^-24 + 3 * 2^-24 * |cents|`` per value.  A difference of two adds both plus its own rounding,
    and the root mean square of the differences cannot be off by more than the largest of them; the float32 mean
    of the squares adds a relative 2^-24 per level of numpy's pairwise sum (4e-6 is generous for < 2^16 frames)."""
    n = min(len(pred), len(ref_hz))
    p, r = np.asarray(pred[:n], dtype=np.float64), np.asarray(ref_hz[:n], dtype=np.float64)
    m = r > 0
    if not m.any():
        return 0.0, 0.0
    cp = ref.hz_to_cents55(np.maximum(p[m], 1e-5))
    cr = ref.hz_to_cents55(r[m])
    u = 2.0 ** -24
    per_frame = 2 * 1200 * 1.4427 * u + 3 * u * (np.abs(cp) + np.abs(cr)) + u * np.abs(cp - cr)
    frame_tol = float(per_frame.max())
    rms = float(np.sqrt(np.mean((cp - cr) ** 2)))
    return frame_tol, frame_tol + 4e-6 * rms


def test_viterbi_restatement_matches_brute_force():
    """C = 6, T = 5, band narrowed to 3 (transitions reach |i - j| <= 2): all 6^5 paths enumerated.  The DP returns
    the maximum score exactly (it adds in the same order) and, among equal scores, the path of the tie rule."""
    rng = np.random.default_rng(5)
    for case in range(6):
        x = rng.normal(size=(5, 6))
        if case >= 3:                       # few distinct values: many exact ties between paths
            x = np.round(x)
        if case == 5:
            x[:] = 0.0
        path = ref.viterbi_path(x, band=3)
        best, arg = ref.brute_force_best(x, band=3)
        assert ref.path_score(x, path, band=3) == best
        assert np.array_equal(path, arg), (case, path, arg)
        assert np.abs(np.diff(path)).max() <= 2


def test_viterbi_restatement_band_and_normalisers():
    """A(i, j) rows sum to one with their own normaliser at the ends; nothing beyond 11 bins."""
    A = np.exp(ref.log_transition(40))
    assert np.allclose(A.sum(axis=1), 1.0, atol=1e-14)
    assert A[0, 0] == 12 / 78 and A[20, 20] == 12 / 144 and A[20, 31] == 1 / 144 and A[20, 32] == 0 and A[0, 12] == 0


def test_bins_are_those_of_the_loss():
    b = np.arange(360)
    assert np.array_equal(model_ref.f0_to_bins(ref.bin_hz(b)), b)
    assert np.array_equal(model_ref.f0_to_bins(ref.bin_hz(b, np.float32).astype(np.float32)), b)
    assert np.array_equal(model_ref.f0_to_bins(ref.bin_hz(np.arange(722)), 722), np.arange(722))


def test_argmax_restatement_takes_the_lowest_index():
    x = np.zeros((4, 10), dtype=np.float32)
    x[1, [3, 7]] = 2.0
    x[2, [0, 9]] = 1.0
    x[3, [9]] = 1.0
    assert ref.argmax_bins(x).tolist() == [0, 3, 0, 9]
    f0, conf, bins = ref.decode(x, "weighted", length=3)
    assert bins.tolist() == [0, 3, 0, 0] and f0[3] == 0 and conf[3] == 0
    assert abs(conf[0] - 0.1) < 1e-15


def test_weighted_restatement_is_a_local_mean():
    """Symmetric weights around the peak give back the bin's own frequency; a one-sided shoulder pulls towards it."""
    x = np.full((2, 360), -20.0)
    x[0, 100], x[0, 99], x[0, 101] = 5.0, 3.0, 3.0
    x[1, 100], x[1, 101] = 5.0, 5.0 + np.log(0.5)
    f0, _, bins = ref.decode(x, "weighted")
    assert bins.tolist() == [100, 100]
    assert abs(1200 * np.log2(f0[0] / ref.bin_hz(100))) < 1e-6
    assert abs(1200 * np.log2(f0[1] / ref.bin_hz(100)) - 20.0 / 3.0) < 1e-6


def test_metrics_restatement_matches_reference_results():
    g = np.load(GOLDEN)
    for k in range(len(g["seeds"])):
        pred, r = g[f"pred_{k}"], g[f"ref_{k}"]
        got = ref.pitch_metrics(pred, r)
        want = float(g[f"rms_{k}"])
        frame_tol, rms_tol = metrics_f32_tolerance(pred, r)
        assert got["n_frames"] == min(len(pred), len(r))
        if np.isnan(want):
            assert got["n_voiced"] == 0 and np.isnan(got["rms_cents"]) and np.isnan(got["rpa"]) and np.isnan(got["rca"])
            continue
        f32 = ref.pitch_metrics(pred, r, dtype=np.float32)["rms_cents"]
        print(f"case {k}: rms {got['rms_cents']:.6f} reference {want:.6f} float32 restatement {f32:.6f} "
              f"tolerance {rms_tol:.2e}")
        assert abs(got["rms_cents"] - want) <= rms_tol
        # the reference's circular distance, frame by frame (compared on the circle: the wrap at +-600 is a jump)
        n = got["n_frames"]
        m = r[:n] > 0
        d = ref.hz_to_cents55(np.maximum(pred[:n][m], np.float32(1e-5))) - ref.hz_to_cents55(r[:n][m])
        circ = np.mod(d + 600.0, 1200.0) - 600.0
        gap = np.mod(circ - g[f"circ_{k}"].astype(np.float64) + 600.0, 1200.0) - 600.0
        assert np.abs(gap).max() <= frame_tol
        assert got["n_voiced"] == int(m.sum())
        # rca forgives what rpa does not: octave errors were planted in every voiced case
        assert got["rca"] > got["rpa"]


def test_metrics_restatement_counts():
    r = np.array([100.0, 100.0, 100.0, 0.0, 0.0, 100.0], dtype=np.float32)
    p = np.array([100.0, 200.0, 0.0, 0.0, 50.0, 103.0], dtype=np.float32)      # 103 Hz = +51.2 cents
    m = ref.pitch_metrics(p, r)
    assert (m["n_voiced"], m["n_frames"]) == (4, 6)
    assert m["rpa"] == 0.25 and m["rca"] == 0.5 and m["vuv_error"] == 2 / 6
    assert ref.pitch_metrics(p, r, threshold_cents=52.0)["rpa"] == 0.5
    assert ref.pitch_metrics(p[:0], r)["n_frames"] == 0


@pytest.fixture(scope="module")
def lib():
    build.build_library(verbose=False)
    return _lib.load()


def test_decode_argument_checks_run_before_any_device_call(lib):
    """No GPU here: every refusal below comes from the host-side checks, with the documented codes."""
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def frames(logits=p, ld_t=360, ld_n=192 * 360, C=360, bins_in=None, N=2, T=192, method=_lib.PE_F0_ARGMAX,
               bins_out=p, f0=p, conf=p):
        return lib.pe_f0_decode_frames(logits, ld_t, ld_n, C, None, bins_in, N, T, method, bins_out, f0, conf, None)

    def viterbi(logits=p, ld_t=360, ld_n=192 * 360, C=360, N=2, T=192, bins_out=p, ws=None, ws_bytes=0):
        return lib.pe_f0_viterbi(logits, ld_t, ld_n, C, None, N, T, bins_out, ws, ws_bytes, None)

    bad_arg, unsupported, workspace = -1, -2, -3
    assert frames(C=1, ld_t=1) == bad_arg
    assert frames(logits=None) == bad_arg and frames(f0=None) == bad_arg and frames(conf=None) == bad_arg
    assert frames(bins_out=None) == bad_arg                       # no bins in, nowhere to put the arg max
    assert frames(method=2) == bad_arg and frames(method=-1) == bad_arg
    assert frames(ld_t=359) == bad_arg and frames(ld_n=191 * 360) == bad_arg and frames(N=0) == bad_arg
    assert frames(C=1025, ld_t=1025, ld_n=192 * 1025) == unsupported
    assert viterbi(C=1, ld_t=1) == bad_arg and viterbi(logits=None) == bad_arg and viterbi(bins_out=None) == bad_arg
    assert viterbi(T=0) == bad_arg and viterbi(C=1025, ld_t=1025, ld_n=192 * 1025) == unsupported
    # back-pointers in LDS: no workspace asked for; T = 700 spills them
    assert lib.pe_f0_viterbi_workspace_bytes(256, 192, 360) == 0
    need = lib.pe_f0_viterbi_workspace_bytes(7, 700, 360)
    assert need == 7 * 700 * 360
    assert viterbi(N=7, T=700, ld_n=700 * 360) == workspace
    assert viterbi(N=7, T=700, ld_n=700 * 360, ws=p, ws_bytes=need - 1) == workspace
    assert lib.pe_pitch_metrics(None, p, 10, 50.0, p, None) == bad_arg
    assert lib.pe_pitch_metrics(p, p, 0, 50.0, p, None) == bad_arg
    assert lib.pe_pitch_metrics(p, p, 10, -1.0, p, None) == bad_arg
    assert lib.pe_pitch_metrics(p, p, 10, 50.0, None, None) == bad_arg


def test_python_layers_refuse_before_a_launch():
    """Unknown method names and the new keyword arguments are checked first: ValueError without a device."""
    import torch
    from pitchextractor_amd import inference, ops
    with pytest.raises(ValueError):
        ops.decode_f0_bins(torch.zeros(4, 8), method="median")
    with pytest.raises(ValueError):
        ops.decode_f0_bins(torch.zeros(4, 8), method="argmax")      # a host tensor: no CPU fallback
    sig = inspect.signature(inference.predict_f0)
    for name in ("decoder", "silence_threshold", "return_confidence"):
        assert sig.parameters[name].kind is inspect.Parameter.KEYWORD_ONLY
    assert sig.parameters["decoder"].default is None and sig.parameters["silence_threshold"].default is None

    class Regression:
        num_class = 1

    class Classifier:
        num_class = 360

    with pytest.raises(ValueError):
        inference.predict_f0(Regression(), np.zeros(2400, dtype=np.float32), decoder="argmax")
    with pytest.raises(ValueError):
        inference.predict_f0(Classifier(), np.zeros(2400, dtype=np.float32), decoder="median")
    # pitch_metrics of nothing is defined without a device
    m = inference.pitch_metrics(np.zeros(0, dtype=np.float32), np.zeros(5, dtype=np.float32))
    assert m["n_frames"] == 0 and np.isnan(m["rms_cents"])

"""Host side of batched ragged inference (no GPU): ``inference.chunk_plan`` against the frame-by-frame restatement in
``tests/predict_batch_ref.py``, and the refusals of ``pe_mel_forward_chunks`` / ``pe_stitch_chunks`` /
``inference.predict_f0_batch`` that are answered before any device call."""
import ctypes

import numpy as np
import pytest
import torch

from pitchextractor_amd import _lib, build, inference, ops
from tests import predict_batch_ref as ref

# (chunk_size, overlap) per mode; n_frames runs over 1 .. 3 * chunk_size, which reaches a single chunk, a last chunk
# of one frame and a tail chunk lying wholly inside its predecessor
SETTINGS = [(mode, cs, ov) for mode in inference.STITCH_MODES
            for cs, ov in ((192, 48), (64, 16), (8, 4) if mode == "crossfade" else (8, 3))]


@pytest.mark.parametrize("mode,cs,ov", SETTINGS)
def test_chunk_plan_equals_the_restatement(mode, cs, ov):
    seen = set()
    for n in range(1, 3 * cs + 1):
        plan = inference.chunk_plan(n, cs, ov, mode)
        row = plan["rows"][0]
        spans = ref.chunk_spans(n, cs, ov)
        assert row["starts"] == [s for s, _ in spans] and row["valid"] == [e - s for s, e in spans]
        want, want_w = ref.frame_map(n, cs, ov, mode)
        got, got_w = ref.plan_frame_map(plan, 0)        # also: the runs tile the output, every frame exactly once
        assert np.array_equal(got, want), (mode, cs, ov, n)
        assert np.array_equal(got_w.view(np.int32), want_w.view(np.int32)), (mode, cs, ov, n)
        assert row["out_len"] == plan["n_out"] == (sum(e - s for s, e in spans) if mode == "concat" else n)
        # the chunk table lists exactly the chunks that are read, in order, by their first frame
        used = sorted(set(want[:, 0].tolist()) | set(want[want[:, 2] >= 0, 2].tolist()))
        assert row["kept"] == used and plan["meta"][:, 2].tolist() == [spans[k][0] for k in used]
        assert plan["chunk_valid"].tolist() == [spans[k][1] - spans[k][0] for k in used]
        if mode != "center":
            assert used == list(range(len(spans)))
        seen |= {"one chunk"} if len(spans) == 1 else set()
        seen |= {"last chunk of one frame"} if spans[-1][1] - spans[-1][0] == 1 and len(spans) > 1 else set()
        seen |= {"tail inside its predecessor"} if len(spans) > 1 and spans[-2][1] == n else set()
        seen |= {"chunk left out"} if len(used) < len(spans) else set()
    assert {"one chunk", "last chunk of one frame", "tail inside its predecessor"} <= seen
    assert ("chunk left out" in seen) == (mode == "center")


def test_concat_reproduces_the_notebook_spans():
    plan = inference.chunk_plan(337)                    # 4.2 s at 24 kHz, hop 300: chunks at 0, 144, 288
    runs = plan["runs"]
    assert [(int(r[2]), int(r[2] + r[3])) for r in runs] == [(0, 192), (192, 384), (384, 433)]
    assert plan["n_out"] == 433 and np.all(runs[:, 4] == 0) and runs[:, 0].tolist() == [0, 1, 2]
    assert plan["rows"][0]["starts"] == [0, 144, 288] and plan["rows"][0]["valid"] == [192, 192, 49]


@pytest.mark.parametrize("mode", inference.STITCH_MODES)
def test_rows_of_a_batch_are_the_rows_alone_shifted(mode):
    frames, offs, counts = [337, 300, 1, 645, 0, 192], [7, 0, 500, 9, 3, 1], [11, 12, 13, 14, 15, 16]
    plan = inference.chunk_plan(frames, 192, 48, mode, sample_offsets=offs, sample_counts=counts)
    assert plan["meta"].dtype == plan["runs"].dtype == np.int64
    assert plan["meta"].shape[1] == 3 and plan["runs"].shape[1] == 8
    chunk_at = out_at = run_at = 0
    for r, n in enumerate(frames):
        alone = inference.chunk_plan(n, 192, 48, mode)
        row = plan["rows"][r]
        K, n_runs = alone["meta"].shape[0], alone["runs"].shape[0]
        assert row["chunks"] == (chunk_at, chunk_at + K) and row["runs"] == (run_at, run_at + n_runs)
        assert row["out_offset"] == out_at and row["out_len"] == alone["n_out"]
        meta = plan["meta"][chunk_at:chunk_at + K]
        assert np.all(meta[:, 0] == offs[r]) and np.all(meta[:, 1] == counts[r])
        assert np.array_equal(meta[:, 2], alone["meta"][:, 2])
        moved = alone["runs"].copy()
        moved[:, 0] += chunk_at
        moved[moved[:, 4] > 0, 6] += chunk_at
        moved[:, 2] += out_at
        assert np.array_equal(plan["runs"][run_at:run_at + n_runs], moved)
        chunk_at, out_at, run_at = chunk_at + K, out_at + alone["n_out"], run_at + n_runs
    assert (chunk_at, out_at, run_at) == (plan["meta"].shape[0], plan["n_out"], plan["runs"].shape[0])
    assert inference.chunk_plan([], 192, 48, mode)["runs"].shape == (0, 8)


def test_plan_refusals():
    for overlap in (192, 200):
        with pytest.raises(ValueError):
            inference.chunk_plan(100, 192, overlap)
    with pytest.raises(ValueError):
        inference.chunk_plan(100, 192, 97, "crossfade")             # three chunks would cover a frame
    inference.chunk_plan(100, 192, 96, "crossfade")
    inference.chunk_plan(100, 192, 191, "center")
    with pytest.raises(ValueError):
        inference.chunk_plan(100, 192, 48, "median")
    with pytest.raises(ValueError):
        inference.chunk_plan(100, 192, -1)
    with pytest.raises(ValueError):
        inference.chunk_plan([100, 50], sample_offsets=[0])


def test_length_groups_keep_a_long_row_from_padding_the_short_ones():
    frames = [100, 24001, 90, 110, 95]
    groups = inference._length_groups(frames, 4 * 360, 1 << 20)     # 728 frames of 360 bins per MiB
    assert sorted(r for g in groups for r in g) == list(range(5))
    assert [frames[r] for g in groups for r in g] == sorted(frames)
    for g in groups:
        assert len(g) == 1 or len(g) * max(frames[r] for r in g) * 4 * 360 <= 1 << 20
    assert [1] in groups and len(groups) == 2
    assert inference._length_groups(frames, 4 * 360, 1 << 40) == [[2, 4, 0, 3, 1]]


@pytest.fixture(scope="module")
def lib():
    build.build_library(verbose=False)
    return _lib.load()


def _table(rows):
    t = np.ascontiguousarray(np.array(rows, np.int64).reshape(len(rows), -1 if rows else 8))
    return t, t.ctypes.data


def test_mel_chunk_arguments_are_checked_on_the_host(lib):
    assert lib.pe_mel_chunk_fields() == 3
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)               # stands for the plan and every device pointer: never read
    elems = 100000

    def call(rows, n=None, plan=p, wave=p, dev=p, out=p, cs=192, host=True):
        t, addr = _table(rows)
        return lib.pe_mel_forward_chunks(plan, wave, elems, dev, addr if host else None, len(rows) if n is None else n,
                                         cs, out, 192 * 80, 1, 80, 1, 1e-5, -4.0, 4.0, 0.0, None)
    ok = [0, 24000, 0]
    assert call([ok], plan=None) == call([ok], wave=None) == call([ok], dev=None) == call([ok], out=None) == -1
    assert call([ok], host=False) == -1 and call([ok], n=-1) == -1 and call([ok], cs=-1) == -1
    assert call([[0, 512, 0]]) == -1                    # n_fft / 2 samples cannot be reflect-padded
    assert call([[-1, 24000, 0]]) == -1 and call([[0, 24000, -1]]) == -1
    assert call([ok, [elems - 23999, 24000, 0]]) == -1   # the row ends past the wave
    assert call([[0, 1 << 31, 0]]) == -1                # ... as does this one
    assert call([ok] * 65536) == -2


def test_stitch_arguments_are_checked_on_the_host(lib):
    assert lib.pe_stitch_run_fields() == 8
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(rows, C=5, n_chunks=3, cs=192, n_dst=500, x=p, dev=p, out=p, det=None, det_out=None, host=True, ld=None):
        t, addr = _table(rows)
        ld = C if ld is None else ld
        return lib.pe_stitch_chunks(x, ld, det, dev, addr if host else None, len(rows), n_chunks, cs, C, out, ld,
                                    det_out, n_dst, None)
    copy, seam = [0, 0, 0, 144, 0, 0, 0, 0], [0, 144, 144, 48, 48, 0, 1, 0]
    assert call([copy, seam], C=0) == call([copy, seam], C=1025) == -2
    assert call([copy], x=None) == call([copy], dev=None) == call([copy], out=None) == call([copy], host=False) == -1
    assert call([copy], det=p) == call([copy], det_out=p) == -1             # the detector pair goes together
    assert call([copy], ld=4) == -1 and call([copy], n_dst=-1) == -1
    assert call([seam, copy]) == -1                                         # out of order
    assert call([copy, [1, 0, 143, 10, 0, 0, 0, 0]]) == -1                  # overlapping
    assert call([[0, 100, 0, 93, 0, 0, 0, 0]]) == -1                        # leaves its chunk
    assert call([[3, 0, 0, 10, 0, 0, 0, 0]]) == call([[-1, 0, 0, 10, 0, 0, 0, 0]]) == -1     # no such chunk
    assert call([[0, 0, 495, 10, 0, 0, 0, 0]]) == -1                        # leaves the destination
    assert call([[0, 0, 0, 0, 0, 0, 0, 0]]) == -1                           # an empty run
    assert call([[0, 144, 144, 48, 48, 0, 3, 0]]) == -1                     # a seam with no second chunk
    assert call([[0, 144, 144, 48, 48, 1, 1, 0]]) == -1                     # more frames than the seam has
    assert call([[0, 144, 144, 48, 48, 0, 1, 150]]) == -1                   # the second chunk's frames run out
    assert call([], n_dst=0, x=None, dev=None, out=None) == 0               # nothing to do


def test_python_layer_refusals():
    net = inference.JDCNet(num_class=1, sequence_model_config={"hidden_size": 8, "num_layers": 1})
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        inference.predict_f0_batch(net, torch.zeros(24000))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        inference.predict_f0_batch(net, torch.zeros(2, 24000), [24000, 12000])
    assert inference.predict_f0_batch(net, []) == []
    with pytest.raises(ValueError):
        inference.predict_f0_batch(net, torch.zeros(24000), decoder="argmax")        # a regression model
    with pytest.raises(ValueError):
        inference.predict_f0_batch(net, torch.zeros(24000), return_confidence=True)
    runs = inference.chunk_plan(100)["runs"]
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.stitch_chunks(torch.zeros(1, 192, 5), runs, torch.from_numpy(runs), torch.zeros(100, 5))

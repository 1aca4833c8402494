"""The device time base (``world.time_base_device``, ``csrc/world_time_base.hip``) against the integer restatement
(``tests/world_time_base_ref.py``), bit for bit: these are IEEE ``+ - * /``, conversions, ``floor`` and compares in
double with contraction off and exact integer sums, so equality is the requirement, not a tolerance."""
import random

import numpy as np
import pytest
import torch

from pitchextractor_amd import meldataset as md
from pitchextractor_amd import world
from tests import world_time_base_ref as tb
from tests.test_data_layer import write_wav

pytestmark = pytest.mark.gpu

PIECE = tb.PIECE
A = (8000, 512, 10.0)
B = (24000, 1024, 12.5)
C = (48000, 2048, 10.0)


def period_for(n: int, L: int, fs) -> float:
    """A frame period (ms) at which ``L`` frames are exactly ``n`` samples."""
    fp = 1000.0 * (n + 0.5) / (L * fs)
    assert world.output_length(L, fs, fp) == n
    return fp


def vuv_row(L, seed=0):
    return tb.margin_curves(L, seed)["vuv"]


def steep_row(L=40):
    return np.append(np.linspace(173.0, 200.0, L - 1), 60.0)


def boundary_rows():
    """Constant-F0 rows of config A (110 frames, 8800 samples, three pieces) found with the restatement: one with a
    pulse on a piece's last sample, one with a pulse on a piece's first."""
    last = first = None
    for f in np.arange(100.0, 400.0, 0.37):
        idx = tb.time_base_vec(np.full(110, f), A[0], A[2], A[1]).table.index
        if last is None and (idx % PIECE == PIECE - 1).any():
            last = f
        elif first is None and ((idx % PIECE == 0) & (idx > 0)).any():        # another row than `last`
            first = f
        if last is not None and first is not None:
            break
    assert last is not None and first is not None
    return np.full(110, last), np.full(110, first)


def _run(rows, cfg, device, **kw):
    fs, fft, fp = cfg
    tables, hook = world.time_base_device(rows, fs, fp, fft, device, hooks=True, **kw)
    return tables, hook


def _check_rows(rows, cfg, device):
    """Every row of one launch against the restatement: counts, tables and the per-sample hooks."""
    fs, fft, fp = cfg
    tables, hook = _run(rows, cfg, device)
    got = tables.host()
    counts = tables.counts.cpu().numpy()
    plan = hook["plan"]
    f0i, lo, hi = (hook[k].cpu().numpy() for k in ("f0i", "lo", "hi"))
    for r, f0 in enumerate(rows):
        want = tb.time_base_vec(f0, fs, fp, fft)
        assert counts[r] == want.count == got[r].index.size, r
        assert plan.capacity[r] >= want.count
        np.testing.assert_array_equal(got[r].index, want.table.index)
        np.testing.assert_array_equal(got[r].vuv, want.table.vuv)
        np.testing.assert_array_equal(got[r].shift.view(np.uint64), want.table.shift.view(np.uint64))
        np.testing.assert_array_equal(got[r].noise_size, want.table.noise_size)
        assert got[r].index.dtype == np.int64 and got[r].shift.dtype == np.float64 and got[r].vuv.dtype == bool
        a, n = int(plan.sample_offsets[r]), int(plan.samples[r])
        assert n == want.f0i.size
        np.testing.assert_array_equal(f0i[a:a + n].view(np.uint64), want.f0i.view(np.uint64))
        np.testing.assert_array_equal(lo[a:a + n].view(np.uint64), want.lo)
        np.testing.assert_array_equal(hi[a:a + n], want.hi)
    return got


def test_rows_of_the_three_configurations(hip_device):
    last, first = boundary_rows()
    rows_a = [np.array([140.0, 150.0]), vuv_row(120, 1), last, first, np.zeros(60), steep_row(70)]
    got = _check_rows(rows_a, A, hip_device)
    assert (got[2].index % PIECE == PIECE - 1).any() and (got[3].index % PIECE == 0).any()
    rows_b = [np.full(120, 200.0), np.zeros(120), vuv_row(150, 2), steep_row(40), np.array([0.0, 300.0])]
    got = _check_rows(rows_b, B, hip_device)
    assert (np.diff(got[0].index) == 120).all() and (np.diff(got[1].index) == 48).all()       # the zero-margin rows
    assert got[2].vuv.any() and not got[2].vuv.all()
    _check_rows([tb.margin_curves(30, 3)["glide"]], C, hip_device)


@pytest.mark.parametrize("n", [PIECE - 1, PIECE, PIECE + 1, 3 * PIECE + 17])
def test_row_lengths_around_a_piece(hip_device, n):
    L = 51 if n < 2 * PIECE else 153
    cfg = (8000, 512, period_for(n, L, 8000))
    rows = [tb.margin_curves(L, 4)["glide"], vuv_row(L, 5), np.zeros(L)]
    _, hook = _run(rows, cfg, hip_device)
    assert hook["plan"].samples.tolist() == [n] * 3 and hook["plan"].n_pieces == 3 * ((n + PIECE - 1) // PIECE)
    _check_rows(rows, cfg, hip_device)


def test_batch_layouts(hip_device):
    """A row's slots and count are the same bits alone, in the batch in any row order, packed behind a row of odd
    length, and with the unused slots preset to a sentinel, which survives."""
    cfg = (8000, 512, period_for(PIECE - 1, 51, 8000))
    last, first = boundary_rows()
    rows = [tb.margin_curves(51, 6)["glide"], vuv_row(120, 7), last, np.zeros(77), steep_row(64), first]
    n = [world.output_length(len(f), cfg[0], cfg[2]) for f in rows]
    assert n[0] % 2 == 1 and len(set(n)) >= 4
    alone = [_run([f], cfg, hip_device)[0].host()[0] for f in rows]

    def same(a, b):
        for x, y in zip(a, b):
            assert x.dtype == y.dtype
            np.testing.assert_array_equal(x.view(np.uint64) if x.dtype == np.float64 else x,
                                          y.view(np.uint64) if y.dtype == np.float64 else y)

    for order in ([0, 1, 2, 3, 4, 5], [5, 3, 1, 0, 4, 2], [2, 0, 5, 4, 3, 1]):
        got = _run([rows[i] for i in order], cfg, hip_device)[0].host()
        for k, i in enumerate(order):
            same(got[k], alone[i])
    # unused slots keep what the caller put there
    plan = world.TimeBasePlan(rows, cfg[0], cfg[2], cfg[1])
    S, R = plan.n_slots, plan.n_rows
    buf = torch.full((16 * S + 8 * R + 8 + S,), 0xAB, dtype=torch.uint8, device=hip_device)
    buf[16 * S:16 * S + 8 * R + 8] = 0                               # counts and the status word
    tables, _ = _run(rows, cfg, hip_device, buffer=buf)
    got = tables.host()
    index, shift, vuv = tables.index.cpu().numpy(), tables.shift.cpu().numpy(), tables.vuv.cpu().numpy()
    sentinel = np.frombuffer(b"\xab" * 8, dtype=np.int64)[0]
    unused = 0
    for r in range(R):
        same(got[r], alone[r])
        a, b = int(tables.slot_offsets[r]) + got[r].index.size, int(tables.slot_offsets[r + 1])
        unused += b - a
        assert (index[a:b] == sentinel).all() and (shift[a:b].view(np.int64) == sentinel).all()
        assert (vuv[a:b] == 0xAB).all()
    assert unused >= R and int(tables.status[0]) == 0


def _refuse(*a, **k):
    raise AssertionError("a host time base was computed in device mode")


def test_through_world_synthesize(hip_device, monkeypatch):
    fs, fft, fp = B
    bins = fft // 2 + 1
    f0 = vuv_row(60, 8)
    g = torch.Generator().manual_seed(3)
    sp = (torch.rand((60, bins), generator=g) + 0.1).to(hip_device)
    ap = (0.3 * torch.rand((bins,), generator=g)).to(hip_device)
    n = world.output_length(60, fs, fp)
    want = torch.zeros((1, n), dtype=torch.float32, device=hip_device)
    world.world_synthesize_ragged([f0], sp.reshape(-1), [0], [bins], torch.ones(1), want, fs=fs, frame_period=fp,
                                  fft_size=fft, ap=ap, ap_offsets=[0], ap_strides=[0], seeds=[5],
                                  tables=[tb.table_of(f0, fs, fp, fft)])
    monkeypatch.setattr(world, "time_base", _refuse)
    got = world.world_synthesize(f0, sp, ap, fs, fp, seed=5, time_base="device")
    assert got.shape == (n,) and float(got.abs().max()) > 0
    assert torch.equal(got, want[0])
    ragged = torch.zeros((1, n), dtype=torch.float32, device=hip_device)
    world.world_synthesize_ragged([f0], sp.reshape(-1), [0], [bins], torch.ones(1), ragged, fs=fs, frame_period=fp,
                                  fft_size=fft, ap=ap, ap_offsets=[0], ap_strides=[0], seeds=[5], tables="device")
    assert torch.equal(ragged, want)


def _loader(tmp_path, mode):
    lines = []
    for i, dur in enumerate((2.0, 1.3)):
        n, f = int(dur * 24000), 120.0 + 41.0 * i
        t = np.arange(n) / 24000
        wave = sum(0.3 / h * np.sin(2 * np.pi * h * f * t + h) for h in (1, 2, 3)).astype(np.float32)
        p = tmp_path / f"u{i}.wav"
        if not p.exists():
            write_wav(p, wave, 24000, "float32")
            np.save(str(p) + "_f0.npy", np.full(1 + n // 300, f, np.float32))
        lines.append(f"{p}|0\n")
    syn = {"enabled": True, "absolute_count": 6, "apply_to_validation": True, "pitch_shift": {"enabled": False},
           "world_vocoder": {"enabled": True, "backend": "hip", "duration": {"min": 0.6, "max": 1.2},
                             "time_base": mode},
           "world_resynthesis": {"enabled": True, "backend": "hip", "semitones": [-3, 2, 5], "noise_db": -55.0,
                                 "aperiodicity": 0.1, "modulation": {"vibrato_probability": 0.5}, "time_base": mode}}
    cfg = {"mel_params": {"sample_rate": 24000, "win_len": 1024, "n_fft": 1024, "n_mels": 80, "hop_length": 300},
           "dataloader": {"start_method": None}, "verbose": False, "synthetic_data": syn}
    return md.build_dataloader(lines, validation=True, batch_size=8, num_workers=0, device="cuda:0",
                               dataset_config=cfg)


LOADER_SEED = 2


def test_through_the_loader(tmp_path, hip_device, monkeypatch):
    """A batch with world_vocoder and world_resynthesis rows in device mode equals the same batch in host mode with
    ``world.time_base`` replaced by the restatement, bit for bit; in device mode no host table is computed."""
    host = _loader(tmp_path, "host")
    monkeypatch.setattr(world, "time_base", tb.table_of)
    np.random.seed(LOADER_SEED); random.seed(LOADER_SEED)
    want = [tuple(t.cpu() for t in b) for b in host]
    np.random.seed(LOADER_SEED); random.seed(LOADER_SEED)
    ds = host.dataset
    kinds = [type(ds[i][-1]).__name__ for i in range(len(ds))]
    assert kinds.count("WorldRequest") >= 2 and kinds.count("ResynthesisRequest") >= 2, kinds
    monkeypatch.setattr(world, "time_base", _refuse)
    device = _loader(tmp_path, "device")
    assert device.dataset._world_generator.time_base == "device"
    np.random.seed(LOADER_SEED); random.seed(LOADER_SEED)
    got = [tuple(t.cpu() for t in b) for b in device]
    assert len(got) == len(want) == 1 and tuple(got[0][0].shape) == (8, 1, 80, 192)
    for a, b in zip(got, want):
        for u, v in zip(a, b):
            assert torch.equal(u, v)

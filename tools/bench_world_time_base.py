"""Cost of WORLD's time base on the host and on the device, and what the device mode changes downstream.

64 rows of 4 s at 24 kHz, 12.5 ms frames (hop 300), N = 1024 -- bench_cheaptrick.py's workload and rows.  Reports, all
from one session: (1) the host ``world.time_base`` loop over the 64 label curves (wall clock); (2) the three launches of
``pe_world_time_base`` one by one, by device events around back-to-back launches on buffers that are already on the
device; (3) ``time_base_device(...).host()`` with its plan, uploads and copy-back (wall clock around a synchronize);
(4) ``resynthesize_ragged`` of the whole rows with ``tables=None`` (host) and ``tables="device"``; (5) the loader stage
of a B = 256 batch with 64 resynthesis rows in both modes -- in host mode the stage is handed the tables a worker
computed, so the worker's share is (1) / 64 per item --; next to the fp32 training step of the flagship batch
(bench.py as a child process).  Also the differences between the two modes on these rows: pulse counts, the largest
``|d shift * fs|`` and the largest sample difference of a synthesized row.  Writes profiles/bench_world_time_base.json
and prints the JSON line.  Needs a GPU.  Not a gate: the numbers to beat are the host path's of the same session.
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
import bench_cheaptrick as bc  # noqa: E402
from pitchextractor_amd import _lib  # noqa: E402
from pitchextractor_amd import meldataset as md  # noqa: E402
from pitchextractor_amd import world  # noqa: E402

SR, HOP, N, ROWS, BATCH, FP = bc.SR, bc.HOP, bc.N, bc.ROWS, bc.BATCH, bc.FP


def host_ms(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(np.min(ts))


def stage_events_us(curves, dev, launches=20, reps=5):
    """Median device time of each launch alone, in microseconds per launch."""
    plan = world.TimeBasePlan(curves, SR, FP, N)
    up = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    meta_d, cf_d, cv_d = up(plan.meta), up(plan.cf), up(plan.cv)
    buf = world.time_base_buffer(plan.n_slots, plan.n_rows, dev)
    S, R = plan.n_slots, plan.n_rows
    lib = _lib.load()
    ws = torch.empty(lib.pe_world_time_base_workspace_bytes(plan.n_pieces), dtype=torch.uint8, device=dev)
    base = buf.data_ptr()

    def launch(stages):
        _lib.check(lib.pe_world_time_base(
            cf_d.data_ptr(), cv_d.data_ptr(), meta_d.data_ptr(), plan.meta.ctypes.data, R, plan.fs,
            plan.frame_period_ms, stages, base, base + 8 * S, base + 16 * S + 8 * R + 8, base + 16 * S,
            base + 16 * S + 8 * R, None, None, None, ws.data_ptr(), ws.numel(), _lib.stream_ptr()), "pe_world_time_base")

    out = {}
    for name, stages in (("sums", 1), ("pulses", 4), ("scan", 2), ("all_three", 7)):
        launch(7)                                                    # the workspace as a full run leaves it
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(launches):                                # (the scan rescans its own output: the same work)
                launch(stages)
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b) * 1e3 / launches)
        out[name + "_us"] = float(np.median(ts))
    out.update(pieces=plan.n_pieces, slots=plan.n_slots, samples=plan.n_samples)
    return out


def loader_stage(dev, waves, f0s, new, reps, mode):
    class _Dataset:
        synthetic_resynthesis_config = {"fft_size": N, "frame_period": FP, "aperiodicity": 0.0,
                                        "q1": world.CHEAPTRICK_Q1, "time_base": mode}

    class _Host:
        dataset = _Dataset()

    loader = md.DeviceMelLoader(_Host(), md.MelSpectrogram(**md.DEFAULT_MEL_PARAMS), dev)
    rng = np.random.default_rng(1)
    items = []
    for r in range(ROWS):
        n = len(waves[r])
        curve = world.label_curve(new[r], SR, N)
        crop = int(rng.integers(0, 1 + n // HOP - 192))
        start, count, first = md.synthetic_window(n, crop, HOP, 1024)
        table = world.no_table() if mode == "device" else world.time_base(curve, SR, FP, N)
        req = md.ResynthesisRequest("", 1.0, n, crop, start, count, first, f0s[r].astype(np.float64), curve,
                                    table.index, table.shift, table.vuv, world.noise_seed(curve), None)
        label = torch.from_numpy(curve[crop:crop + 192].astype(np.float32))
        items.append((torch.from_numpy(waves[r]), label, (label == 0).float(), first, SR, req))
    plain = (torch.zeros(192 * HOP), torch.zeros(192), torch.zeros(192), 0, SR)
    batch = [items[i // 4] if i % 4 == 0 else plain for i in range(BATCH)]
    host = md.Collater()(batch)
    pack_host = host[-1]
    dev_items = md.H2DPrefetcher(dev).submit(host)[0]
    torch.cuda.synchronize()
    waves_d, lengths_d, pack = dev_items[0], dev_items[1], dev_items[-1]
    return bc.wall_ms(lambda: loader._run_stage(md.WORLD_RESYNTHESIS, waves_d, lengths_d, pack, pack_host, SR), reps)


def differences(curves, x, lengths, f0s, new, dev):
    host = [world.time_base(c, SR, FP, N) for c in curves]
    devt = world.time_base_device(curves, SR, FP, N, dev).host()
    same = [h.index.size == d.index.size and np.array_equal(h.index, d.index) and np.array_equal(h.vuv, d.vuv)
            for h, d in zip(host, devt)]
    worst = max(float(np.abs(h.shift - d.shift).max()) * SR for h, d, s in zip(host, devt, same) if s)
    outs = [world.resynthesize_ragged(x, lengths, f0s, new, SR, FP, fft_size=N, seeds=list(range(ROWS)),
                                      tables=t)[0] for t in (None, "device")]
    res = {"rows_with_identical_pulses": int(sum(same)), "rows": len(same),
           "max_abs_shift_difference_samples": worst,
           "max_abs_sample_difference_of_a_synthesized_row": float((outs[0] - outs[1]).abs().max()),
           "max_abs_sample": float(outs[0].abs().max())}
    zero = {"const_200_hz_1p5_s_24k": (np.full(120, 200.0), 24000), "unvoiced_1p5_s_24k": (np.zeros(120), 24000),
            "unvoiced_1p5_s_16k": (np.zeros(120), 16000)}
    res["zero_margin_pulse_counts_host_vs_device"] = {
        k: [int(world.time_base(f, fs, 12.5, N).index.size),
            int(world.time_base_device([f], fs, 12.5, N, dev).host()[0].index.size)] for k, (f, fs) in zero.items()}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-train-step", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "bench_world_time_base.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_world_time_base: no GPU visible; this benchmark does not run without one")
    dev = torch.device("cuda:0")
    waves, f0s, new = bc.make_rows()
    lengths = [len(w) for w in waves]
    x = torch.from_numpy(np.concatenate(waves)).to(dev)
    curves = [world.label_curve(c, SR, N) for c in new]
    host_loop = host_ms(lambda: [world.time_base(c, SR, FP, N) for c in curves], a.reps)
    kernels = stage_events_us(curves, dev)
    device_tb = bc.wall_ms(lambda: world.time_base_device(curves, SR, FP, N, dev).host(), a.reps)
    resyn = {m: bc.wall_ms(lambda t=t: world.resynthesize_ragged(x, lengths, f0s, new, SR, FP, fft_size=N,
                                                                 seeds=list(range(ROWS)), tables=t), a.reps)
             for m, t in (("host", None), ("device", "device"))}
    stage = {m: loader_stage(dev, waves, f0s, new, a.reps, m) for m in ("host", "device")}
    res = {"rows": ROWS, "seconds_per_row": bc.SECONDS, "fft_size": N, "frame_period_ms": FP,
           "pulses": int(sum(world.time_base(c, SR, FP, N).index.size for c in curves)),
           "host_time_base_loop_ms_median": host_loop[0], "host_time_base_loop_ms_min": host_loop[1],
           "host_time_base_ms_per_row": host_loop[0] / ROWS, "kernels": kernels,
           "time_base_device_host_ms_median": device_tb[0], "time_base_device_host_ms_min": device_tb[1],
           "resynthesize_ragged_ms_median": {m: v[0] for m, v in resyn.items()},
           "resynthesize_ragged_ms_min": {m: v[1] for m, v in resyn.items()},
           "loader_stage_ms_median": {m: v[0] for m, v in stage.items()},
           "loader_stage_ms_min": {m: v[1] for m, v in stage.items()}, "loader_batch": BATCH,
           "loader_resynthesis_rows": ROWS,
           "worker_cpu_ms_per_batch_host_mode": host_loop[0], "worker_cpu_ms_per_batch_device_mode": 0.0,
           "differences": differences(curves, x, lengths, f0s, new, dev)}
    if not a.no_train_step:
        res["training_step_ms_fp32_batch256"] = bc.training_step_ms()
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

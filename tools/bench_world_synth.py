"""Device cost of the WORLD-vocoder synthetic rows (synthetic_data.world_vocoder, backend hip) per training batch.

64 rows of 1.5 s at 24 kHz, hop 300, N = 1024 -- the share a ``ratio: 0.25`` batch of 256 carries with both generators
on -- drawn by ``WorldGenerator`` from fixed seeds with the reference's shipped settings (110-320 Hz, vibrato).  Times
``world_synthesize_ragged`` between device events (host plan, three small host-to-device copies and the two launches
included), then the two kernels alone from a run of its own under ``rocprofv3 --kernel-trace --stats`` (no counters),
started here as a child process, and the training step of the flagship batch (256 utterances x 192 frames, fp32) in
the same session by running bench.py as a child process.  Writes profiles/bench_world_synth.json and
profiles/bench_world_synth_kernel_stats.csv and prints the JSON line.  Needs a GPU.

    python tools/bench_world_synth.py               # time, trace, training step
    python tools/bench_world_synth.py --trace-run   # what the traced child runs

Not a gate.  The responses kernel does four 1024-point complex transforms in LDS per pulse plus about 513 x (2 log, 2
exp, 3 sincos): its flop and its bytes are reported with the share of the fp32 vector peak and of the 6.29 TB/s copy
rate they imply; the overlap-add reads every response once (fft_size floats per pulse) and is reported against the copy
rate.
"""
import argparse
import csv
import json
import random
import shutil
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from pitchextractor_amd import world  # noqa: E402

SR, HOP, N, ROWS, SECONDS = 24000, 300, 1024, 64, 1.5
HBM_COPY_TBS = 6.29                       # measured copy rate of the MI355X microarchitecture guide
VALU_FP32_TFLOPS = 157.3                  # vector fp32 peak (spec) of the same guide
KERNELS = ("world_responses_kernel", "world_ola_kernel")
CONFIG = {"duration": {"min": SECONDS, "max": SECONDS}, "pitch_range": [110.0, 320.0], "gain_db_range": [-18.0, -6.0],
          "noise_db": -60.0,
          "modulation": {"vibrato_probability": 0.5, "vibrato_semitones": 0.4, "vibrato_rate_range": [4.0, 6.0]}}


def make_batch(dev):
    random.seed(0)
    np.random.seed(0)
    gen = world.WorldGenerator(SR, HOP, N, CONFIG)
    draws = [gen.draw() for _ in range(ROWS)]
    n = [world.output_length(d.curve.size, SR, gen.frame_period) for d in draws]
    out = torch.zeros((256, max(n)), dtype=torch.float32, device=dev)
    args = dict(f0s=[d.curve for d in draws], sp=gen.device_templates(dev).reshape(-1),
                sp_offsets=[d.template * (N // 2 + 1) for d in draws], sp_strides=[0] * ROWS,
                gains=torch.tensor([d.gain for d in draws], dtype=torch.float32, device=dev), out=out,
                out_rows=np.arange(0, 256, 256 // ROWS)[:ROWS], fs=SR, frame_period=gen.frame_period, fft_size=N,
                tables=[d.table for d in draws], seeds=[world.noise_seed(d.curve) for d in draws],
                out_noise=torch.from_numpy(np.concatenate([d.noise for d in draws]).astype(np.float32)).to(dev))
    return args, sum(d.table.index.size for d in draws), sum(n)


def trace_run(dev):
    args, _, _ = make_batch(dev)
    for _ in range(10):
        world.world_synthesize_ragged(**args)
    torch.cuda.synchronize()


def kernel_rows(out_csv: Path):
    prof = shutil.which("rocprofv3")
    if prof is None:
        raise SystemExit("bench_world_synth: rocprofv3 not found; kernel times are not optional")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "world", "--",
               sys.executable, str(Path(__file__).resolve()), "--trace-run"]
        subprocess.run(cmd, check=True, timeout=600, stdout=subprocess.DEVNULL)
        stats = sorted(Path(tmp).rglob("*kernel_stats.csv"))
        trace = sorted(Path(tmp).rglob("*kernel_trace.csv"))
        if not stats or not trace:
            raise SystemExit("bench_world_synth: the profiler wrote no kernel_stats.csv / kernel_trace.csv")
        rows = list(csv.DictReader(open(stats[0])))
        events = list(csv.DictReader(open(trace[0])))
    keep = [r for r in rows if any(k in r.get("Name", "") for k in KERNELS)]
    if not keep:
        raise SystemExit("bench_world_synth: none of the WORLD kernels appear in the trace")
    with open(out_csv, "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=list(keep[0].keys()))
        w.writeheader()
        w.writerows(keep)
    per = {}
    for k in KERNELS:
        d = [int(e["End_Timestamp"]) - int(e["Start_Timestamp"]) for e in events if k in e.get("Kernel_Name", "")]
        d = d[2:] if len(d) > 4 else d                                  # the first calls carry the code load
        if d:
            per[k] = {"calls": len(d), "avg_us": sum(d) / len(d) / 1e3, "min_us": min(d) / 1e3, "max_us": max(d) / 1e3}
    return per


def training_step_ms():
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "10", "--warmup", "3", "--no-cpu-baseline",
           "--no-native-ref"]
    res = subprocess.run(cmd, check=True, timeout=900, capture_output=True, text=True, cwd=str(ROOT))
    line = [ln for ln in res.stdout.splitlines() if ln.startswith("{")][-1]
    return float(json.loads(line)["ms_per_step"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--no-train-step", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "bench_world_synth.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_world_synth: no GPU visible; this benchmark does not run without one")
    dev = torch.device("cuda:0")
    if a.trace_run:
        trace_run(dev)
        return
    args, pulses, samples = make_batch(dev)
    for _ in range(5):
        world.world_synthesize_ragged(**args)
    torch.cuda.synchronize()
    ts = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        world.world_synthesize_ragged(**args)
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    kern = kernel_rows(out.with_name(out.stem + "_kernel_stats.csv"))
    res = {"rows": ROWS, "seconds_per_row": SECONDS, "fft_size": N, "pulses": pulses, "output_samples": samples,
           "workspace_bytes": pulses * N * 4, "ms_per_batch_median": float(np.median(ts)),
           "ms_per_batch_min": float(np.min(ts)), "kernels": kern}
    bins = N // 2 + 1
    if "world_responses_kernel" in kern:
        k = kern["world_responses_kernel"]
        flop = pulses * (4 * 5 * N * np.log2(N) + bins * 7 * 20)         # transforms + ~20 flop per transcendental
        moved = pulses * (N * 4 + 2 * bins * 4)                          # responses written; templates stay in L2
        k.update(flop=float(flop), bytes=moved, us_per_pulse_per_cu=k["avg_us"] * 256 / pulses,
                 share_of_valu_peak=flop / (k["avg_us"] * 1e-6) / 1e12 / VALU_FP32_TFLOPS,
                 share_of_copy_rate=moved / (k["avg_us"] * 1e-6) / 1e12 / HBM_COPY_TBS,
                 bound="LDS passes and barriers of four transforms per pulse, then transcendentals")
    if "world_ola_kernel" in kern:
        k = kern["world_ola_kernel"]
        moved = pulses * N * 4 + samples * 8
        k.update(bytes=moved, share_of_copy_rate=moved / (k["avg_us"] * 1e-6) / 1e12 / HBM_COPY_TBS,
                 bound="memory: every response read once")
    res["device_ms_per_batch"] = sum(k["avg_us"] for k in kern.values()) / 1e3
    res["pitch_shift_ms_same_rows"] = json.loads((ROOT / "profiles" / "bench_pitch_shift.json").read_text())[
        "pitch_shift_ms_median"]
    if not a.no_train_step:
        step = training_step_ms()
        res["training_step_ms_fp32_batch256"] = step
        res["stage_to_training_step_ratio"] = res["ms_per_batch_median"] / step
    out.write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

"""Device cost of WORLD D4C and of the resynthesis rows that use it (``world_resynthesis`` with ``aperiodicity: d4c``).

The rows of tools/bench_cheaptrick.py: 64 rows of 4 s at 24 kHz, 12.5 ms frames (hop 300) -- the share a ``ratio: 0.25``
batch of 256 carries.  Reports, from one session: (1) the band-analysis launch and the expansion launch alone, from a
run of its own under ``rocprofv3 --kernel-trace --stats`` (no counters) started here as a child process, at pyworld's
threshold and at the data layer's 0; (2) ``d4c_ragged`` with its host work (wall clock around a synchronize); (3) the
loader stage (``DeviceMelLoader._run_stage`` of the ``world_resynthesis`` kind) for a B = 256 batch with 64 resynthesis
rows cropped to the 192-frame window, in ``d4c`` mode and in the numeric mode; (4) the fp32 training step of the
flagship batch (bench.py as a child process) before and after the rest, so that the shares are of this session's step.
With ``--ratios FILE`` the measured accuracy ratios (the ``[d4c]`` records tests/test_d4c_gpu.py prints) are copied in.
Writes profiles/bench_d4c.json and profiles/bench_d4c_kernel_stats.csv and prints the JSON line.  Needs a GPU.

    python tools/bench_d4c.py               # time, trace, training step
    python tools/bench_d4c.py --trace-run   # what the traced child runs

Not a gate.  No counter run is made here: what bounds the band-analysis kernel is not known.
"""
import argparse
import csv
import json
import re
import shutil
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
import bench_cheaptrick as bc  # noqa: E402
from pitchextractor_amd import meldataset as md  # noqa: E402
from pitchextractor_amd import world  # noqa: E402

SR, HOP, N, ROWS, BATCH, FP = bc.SR, bc.HOP, bc.N, bc.ROWS, bc.BATCH, bc.FP
KERNELS = ("d4c_bands_kernel", "d4c_expand_kernel")
THRESHOLDS = (world.D4C_THRESHOLD, 0.0)
TRACE_REPS = 6


def trace_run(dev):
    waves, f0s, _ = bc.make_rows()
    x = torch.from_numpy(np.concatenate(waves)).to(dev)
    for thr in THRESHOLDS:                                       # TRACE_REPS calls at each threshold, in this order
        for _ in range(TRACE_REPS):
            world.d4c_ragged(x, [len(w) for w in waves], f0s, SR, FP, threshold=thr, fft_size=N)
    torch.cuda.synchronize()


def kernel_rows(out_csv: Path):
    prof = shutil.which("rocprofv3")
    if prof is None:
        raise SystemExit("bench_d4c: rocprofv3 not found; kernel times are not optional")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "d4c", "--",
               sys.executable, str(Path(__file__).resolve()), "--trace-run"]
        subprocess.run(cmd, check=True, timeout=600, stdout=subprocess.DEVNULL)
        stats = sorted(Path(tmp).rglob("*kernel_stats.csv"))
        trace = sorted(Path(tmp).rglob("*kernel_trace.csv"))
        if not stats or not trace:
            raise SystemExit("bench_d4c: the profiler wrote no kernel_stats.csv / kernel_trace.csv")
        rows = list(csv.DictReader(open(stats[0])))
        events = list(csv.DictReader(open(trace[0])))
    keep = [r for r in rows if any(k in r.get("Name", "") for k in KERNELS)]
    if len(keep) < 2:
        raise SystemExit("bench_d4c: the D4C kernels do not appear in the trace")
    with open(out_csv, "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=list(keep[0].keys()))
        w.writeheader()
        w.writerows(keep)
    out = {}
    for k in KERNELS:
        d = [int(e["End_Timestamp"]) - int(e["Start_Timestamp"]) for e in events if k in e.get("Kernel_Name", "")]
        if len(d) != TRACE_REPS * len(THRESHOLDS):
            raise SystemExit(f"bench_d4c: {len(d)} launches of {k} in the trace")
        for i, thr in enumerate(THRESHOLDS):
            part = d[i * TRACE_REPS + 2:(i + 1) * TRACE_REPS]    # the first calls carry the code load
            out[f"{k}_threshold_{thr}"] = {"calls": len(part), "avg_us": sum(part) / len(part) / 1e3,
                                           "min_us": min(part) / 1e3, "max_us": max(part) / 1e3}
    return out


def loader_stage(dev, waves, f0s, new, reps, aperiodicity):
    """tools/bench_cheaptrick.py's stage with the block's ``aperiodicity`` set: a collated B = 256 batch whose 64
    resynthesis rows are cropped windows."""
    class _Dataset:
        synthetic_resynthesis_config = {"fft_size": N, "frame_period": FP, "aperiodicity": aperiodicity,
                                        "d4c_threshold": 0.0, "q1": world.CHEAPTRICK_Q1}

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
        table = world.time_base(curve, SR, FP, N)
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


def accuracy_ratios(path):
    """{configuration: {quantity: ratio}} from the ``[d4c] fs .. ratio r`` records of the GPU test's output."""
    out = {}
    pat = re.compile(r"\[d4c\] fs (\d+) fp ([\d.]+) thr ([\d.]+) (a0|coarse|ap): gpu (\S+) float32 restatement (\S+) "
                     r"ratio (\S+)")
    for m in pat.finditer(Path(path).read_text()):
        out.setdefault(f"fs{m[1]}-fp{m[2]}-thr{m[3]}", {})[m[4]] = {"gpu": float(m[5]), "float32": float(m[6]),
                                                                  "ratio": float(m[7])}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--no-train-step", action="store_true")
    ap.add_argument("--ratios", default=None, help="output of tests/test_d4c_gpu.py run with -s")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "bench_d4c.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_d4c: no GPU visible; this benchmark does not run without one")
    dev = torch.device("cuda:0")
    if a.trace_run:
        trace_run(dev)
        return
    step_before = None if a.no_train_step else bc.training_step_ms()
    waves, f0s, new = bc.make_rows()
    lengths = [len(w) for w in waves]
    x = torch.from_numpy(np.concatenate(waves)).to(dev)
    frames = sum(len(f) for f in f0s)
    res = {"rows": ROWS, "seconds_per_row": bc.SECONDS, "sample_rate": SR, "fft_size": N, "frame_period_ms": FP,
           "frames": frames, "n_d": 2048, "bands": 3, "loader_batch": BATCH, "loader_resynthesis_rows": ROWS,
           "bound": "not known: no counter run was made"}
    for thr in THRESHOLDS:
        ms = bc.wall_ms(lambda: world.d4c_ragged(x, lengths, f0s, SR, FP, threshold=thr, fft_size=N), a.reps)
        res[f"d4c_ragged_ms_median_threshold_{thr}"], res[f"d4c_ragged_ms_min_threshold_{thr}"] = ms
    _, band = world.d4c_ragged(x, lengths, f0s, SR, FP, fft_size=N, return_bands=True)
    res["frames_with_band_analysis_at_0.85"] = int((~torch.isnan(band[:, 1])).sum())
    for tag, mode in (("d4c", "d4c"), ("numeric_0.1", 0.1), ("numeric_0", 0.0)):
        ms = loader_stage(dev, waves, f0s, new, a.reps, mode)
        res[f"loader_stage_ms_median_{tag}"], res[f"loader_stage_ms_min_{tag}"] = ms
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    res["kernels"] = kernel_rows(out.with_name(out.stem + "_kernel_stats.csv"))
    if a.ratios:
        res["accuracy_ratios_gpu_over_float32_restatement"] = accuracy_ratios(a.ratios)
    if not a.no_train_step:
        step_after = bc.training_step_ms()
        res["training_step_ms_fp32_batch256_before"], res["training_step_ms_fp32_batch256_after"] = step_before, step_after
        step = 0.5 * (step_before + step_after)
        res["bands_kernel_to_training_step_ratio"] = res["kernels"]["d4c_bands_kernel_threshold_0.0"]["avg_us"] / 1e3 / step
        res["d4c_ragged_to_training_step_ratio"] = res["d4c_ragged_ms_median_threshold_0.0"] / step
        res["stage_d4c_to_training_step_ratio"] = res["loader_stage_ms_median_d4c"] / step
        res["stage_numeric_to_training_step_ratio"] = res["loader_stage_ms_median_numeric_0.1"] / step
    out.write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

"""Device cost of labelling a batch with the on-device DIO + StoneMask tracker (f0_tracker.WorldDioTracker) next to
training on it.

One resident batch at 24 kHz, hop 300, pyworld's defaults: 256 rows of 4 s (321 frames each).  The batch is tracked in
a loop between two device events and the total is divided by the number of calls (``track`` includes its host work:
plan, the launches of the five stages and the row statistics, one device-to-host copy of the contours).  Kernel times
come from a run of their own under ``rocprofv3 --kernel-trace --stats`` (no counters), started here as a child process
once the timing is done.  The training step of the flagship batch (256 utterances x 192 frames, fp32) is measured in
the same session by running bench.py as a child process.  The figures tests/test_f0_dio_gpu.py asserts are recorded
per configuration.  Writes profiles/bench_f0_dio.json and profiles/bench_f0_dio_kernel_stats.csv and prints the JSON
line.  Needs a GPU.

    python tools/bench_f0_dio.py               # time, trace, training step
    python tools/bench_f0_dio.py --trace-run   # what the traced child runs: a few calls on the batch
    python tools/bench_f0_dio.py --configurations-only   # only re-measure the configuration cases, in place

Not a gate: labelling happens once per file, not once per step.
"""
import argparse
import csv
import json
import shutil
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from pitchextractor_amd import synthetic  # noqa: E402
from pitchextractor_amd.f0_tracker import WorldDioTracker  # noqa: E402

SR, HOP = 24000, 300
KERNELS = ("f0_sum_kernel", "f0_peak_kernel", "f0_peak_final_kernel", "dio_bands_kernel", "dio_events_kernel",
           "dio_prefix_kernel", "dio_candidates_kernel", "dio_best_kernel", "dio_fix_kernel", "stonemask_kernel")


def make_batch(dev):
    waves = [synthetic.utterance(i, duration=4.0, sr=SR, hop=HOP)[0] for i in range(256)]
    return torch.from_numpy(np.concatenate(waves)).to(dev), [len(w) for w in waves]


def trace_run(dev):
    tr = WorldDioTracker(SR, HOP)
    flat, lengths = make_batch(dev)
    for _ in range(5):
        tr.track(flat, lengths)
    torch.cuda.synchronize()


def timed_loop(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def kernel_rows(out_csv: Path):
    """Run the traced child; per-kernel (calls, avg / min / max us), rows kept in ``out_csv``."""
    prof = shutil.which("rocprofv3")
    if prof is None:
        raise SystemExit("bench_f0_dio: rocprofv3 not found; kernel times are not optional")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "f0_dio", "--",
               sys.executable, str(Path(__file__).resolve()), "--trace-run"]
        subprocess.run(cmd, check=True, timeout=600, stdout=subprocess.DEVNULL)
        stats = sorted(Path(tmp).rglob("*kernel_stats.csv"))
        if not stats:
            raise SystemExit("bench_f0_dio: the profiler wrote no kernel_stats.csv")
        rows = list(csv.DictReader(open(stats[0])))
    keep = [r for r in rows if any(k in r.get("Name", "") for k in KERNELS)]
    if not keep:
        raise SystemExit("bench_f0_dio: none of the tracker kernels appear in the trace")
    with open(out_csv, "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=list(keep[0].keys()))
        w.writeheader()
        w.writerows(keep)
    per = {}
    for r in keep:
        name = next(k for k in KERNELS if k in r["Name"])
        if "dio_events_kernel" in name:
            name += "<scatter>" if "true" in r["Name"] or "<1" in r["Name"] else "<count>"
        calls = int(r["Calls"])
        per[name] = {"calls": calls, "avg_us": float(r["TotalDurationNs"]) / calls / 1e3,
                     "min_us": float(r["MinNs"]) / 1e3, "max_us": float(r["MaxNs"]) / 1e3}
    return per


def training_step_ms():
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "10", "--warmup", "3", "--no-cpu-baseline",
           "--no-native-ref"]
    res = subprocess.run(cmd, check=True, timeout=900, capture_output=True, text=True, cwd=str(ROOT))
    line = [ln for ln in res.stdout.splitlines() if ln.startswith("{")][-1]
    return float(json.loads(line)["ms_per_step"])


def deviation_records(dev):
    """The end-to-end figures of tests/test_f0_dio_gpu.py: per configuration the yardstick (float32 against float64
    restatement on that configuration's inputs) and the tracker's deviation from the float64 restatement."""
    from tests import dio_ref as D
    out = []
    for sr, hop in D.GPU_CONFIGS:
        tr = WorldDioTracker(sr, hop)
        yard = {k: v for k, v in D.config_yardstick(sr, hop).items() if isinstance(v, float)}
        rec = {"sr": sr, "hop": hop, "block_fft": tr.n_fft, "yardstick": yard}
        for kind, waves, refs in (("margin", D.margin_inputs(sr), [a for a, _ in D.reference_pairs(sr, hop)]),
                                  ("natural", D.natural_inputs(sr), [a for a, _ in D.natural_pairs(sr, hop)])):
            got = tr.track(torch.from_numpy(np.concatenate(waves)).to(dev), [len(w) for w in waves])
            devs = [D.contour_deviation(ref["f0"], g) for ref, g in zip(refs, got)]
            rec[kind] = {"frames": int(sum(len(g) for g in got)), "voicing_flips": int(sum(d[1] for d in devs)),
                         "contour_cents": max(d[0] for d in devs)}
        rec["ratio_to_yardstick"] = {"margin": rec["margin"]["contour_cents"] / yard["cents"],
                                     "natural": rec["natural"]["contour_cents"] / yard["natural_cents"]}
        out.append(rec)
    return out


def configuration_records(dev):
    """What tests/test_f0_dio_config_gpu.py asserts, as figures: per case of ``dio_ref.CONFIG_CASES`` the yardstick of
    its own rows and, stage by stage and end to end, the kernels' deviation from the float64 restatement on the margin
    rows (the tests' assertions run on the way)."""
    from tests import dio_ref as D
    from tests import test_f0_dio_gpu as G
    out = []
    for name, sr, hop, config, inputs in D.CONFIG_CASES:
        B = G._batch(sr, hop, config, inputs)
        tr = B["tr"]
        device = {}
        for check in (G.check_band_signals, G.check_events, G.check_candidates, G.check_contour_fix,
                      G.check_stonemask):
            device.update(check(B))
        device.update(G.check_end_to_end(B, True))
        out.append({"case": name, "sr": sr, "hop": hop, "config": dict(config), "inputs": [list(i) for i in inputs],
                    "block_fft": tr.n_fft, "bands": tr.bands, "voice_range_minimum": tr.voice_range_minimum,
                    "yardstick": {k: v for k, v in B["yard"].items() if isinstance(v, float)}, "device": device})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=2.0, help="seconds of timed work")
    ap.add_argument("--configurations-only", action="store_true",
                    help="measure only tracker_vs_float64_restatement_configurations and put it into the existing --out")
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--no-train-step", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "bench_f0_dio.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_f0_dio: no GPU visible; this benchmark does not run without one")
    dev = torch.device("cuda:0")
    if args.trace_run:
        trace_run(dev)
        return
    if args.configurations_only:
        res = json.loads(Path(args.out).read_text())
        res["tracker_vs_float64_restatement_configurations"] = configuration_records(dev)
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
        print(json.dumps(res["tracker_vs_float64_restatement_configurations"]))
        return
    tr = WorldDioTracker(SR, HOP)
    flat, lengths = make_batch(dev)
    fn = lambda: tr.track(flat, lengths)  # noqa: E731
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    per_call_ms = timed_loop(fn, 3) / 3
    calls = max(3, int(args.window * 1e3 / max(per_call_ms, 1e-3)))
    t0 = time.time()
    ms = timed_loop(fn, calls) / calls
    plan = tr.plan(lengths)
    voiced = int(sum(int(np.count_nonzero(c)) for c in tr.track(flat, lengths)))
    res = {"sr": SR, "hop": HOP, "block_fft": tr.n_fft, "bands": tr.bands, "taps": tr.taps, "rows": len(lengths),
           "samples": int(sum(lengths)), "frames": plan["n_frames"], "voiced_frames": voiced,
           "blocks": plan["n_blocks"], "ms_per_track_call": ms, "calls": calls, "wall_s": round(time.time() - t0, 2)}
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    res["kernels"] = kernel_rows(out.with_name(out.stem + "_kernel_stats.csv"))
    res["tracker_vs_float64_restatement"] = deviation_records(dev)
    res["tracker_vs_float64_restatement_configurations"] = configuration_records(dev)
    if not args.no_train_step:
        step = training_step_ms()
        res["training_step_ms_fp32_batch256"] = step
        res["label_to_training_step_ratio"] = ms / step
    out.write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

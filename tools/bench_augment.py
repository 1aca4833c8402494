"""Device cost of the training-time augmentation (``pitchextractor_amd.augment``).

Reports, from one session: (a) ``pe_augment_biquad`` (the parallel scan in double) against ``pe_stress_biquad`` (the
systolic wave, one dependent recurrence per sample) on the rows of tools/bench_stress.py, 64 rows of 4 s at 24 kHz, with
the same 8 stages for every row -- mild peaking stages on a quiet input, so that the old kernel's clamp never acts and
the two compute the same filter (their largest difference is reported); (b) the full chain at ``p = 1`` (reverb, noise,
filter, clipping, gain, polarity) on a B = 256 batch of 2-s rows with the host work of ``Augmenter.apply`` (wall clock
around a synchronize) and the host cost of ``draw``, beside the fp32 training step of the flagship batch (bench.py as a
child process, before and after the rest), as the other loader stages are reported.  Kernel times come from a run of
its own under ``rocprofv3 --kernel-trace --stats`` (no counters) started here as a child process.  Writes
profiles/bench_augment.json and profiles/bench_augment_kernel_stats.csv and prints the JSON line.  Needs a GPU.

    python tools/bench_augment.py               # time, trace, training step
    python tools/bench_augment.py --trace-run   # what the traced child runs

Not a gate.  The reverb's responses are three decaying-noise responses of 0.5 s, not the shoebox library.
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
from pitchextractor_amd import augment, stress  # noqa: E402

SR, ROWS, SECONDS, BATCH, BATCH_SECONDS = 24000, 64, 4.0, 256, 2.0
CURVE = [{"freq": 90.0 * 2.0 ** k, "gain_db": (3.0, -3.0)[k % 2], "Q": 1.0} for k in range(8)]     # 90 Hz .. 11.5 kHz
TRACE_REPS = 6
KERNELS = ("augment_", "stress_", "noise_", "mix_")


def filter_rows(dev):
    rng = np.random.default_rng(0)
    n = int(SR * SECONDS)
    return torch.from_numpy((0.01 * rng.standard_normal((ROWS, n))).astype(np.float32)).to(dev)


def curve_sos():
    return np.stack([augment.peaking(SR, s["freq"], s["gain_db"], s["Q"]) for s in CURVE])


def chain(dev):
    rng = np.random.default_rng(1)
    n = int(SR * BATCH_SECONDS)
    x = torch.from_numpy((0.1 * rng.standard_normal((BATCH, n))).astype(np.float32)).to(dev)
    m = SR // 2
    responses = [(rng.standard_normal(m) * np.exp(-np.arange(m) / (m / 7.0))).astype(np.float32) for _ in range(3)]
    config = {t: {"p": 1.0} for t in augment.TRANSFORMS}
    config["reverb"]["responses"] = responses
    aug = augment.Augmenter(config, SR, seed=0).prepare(dev)
    return aug, x, [n] * BATCH


def trace_run(dev):
    x, sos = filter_rows(dev), curve_sos()
    for _ in range(TRACE_REPS):
        augment.biquad_cascade(x, sos)
    for _ in range(TRACE_REPS):
        stress.apply_microphone_eq(x, SR, CURVE)
    aug, xb, lengths = chain(dev)
    plan = aug.draw(BATCH)
    for _ in range(TRACE_REPS):
        aug.apply(xb, lengths, plan)
    torch.cuda.synchronize()


def kernel_rows(out_csv: Path):
    prof = shutil.which("rocprofv3")
    if prof is None:
        raise SystemExit("bench_augment: rocprofv3 not found; kernel times are not optional")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "augment", "--",
               sys.executable, str(Path(__file__).resolve()), "--trace-run"]
        subprocess.run(cmd, check=True, timeout=600, stdout=subprocess.DEVNULL)
        stats = sorted(Path(tmp).rglob("*kernel_stats.csv"))
        trace = sorted(Path(tmp).rglob("*kernel_trace.csv"))
        if not stats or not trace:
            raise SystemExit("bench_augment: the profiler wrote no kernel_stats.csv / kernel_trace.csv")
        rows = list(csv.DictReader(open(stats[0])))
        events = list(csv.DictReader(open(trace[0])))
    keep = [r for r in rows if any(k in r.get("Name", "") for k in KERNELS)]
    if not keep:
        raise SystemExit("bench_augment: the augmentation kernels do not appear in the trace")
    with open(out_csv, "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=list(keep[0].keys()))
        w.writeheader()
        w.writerows(keep)
    events.sort(key=lambda e: int(e["Start_Timestamp"]))
    names = [e.get("Kernel_Name", "") for e in events]
    first_chain = [i for i, nm in enumerate(names) if "stress_biquad_kernel" in nm][-1] + 1     # the chain follows (a)
    out = {"filter_rows": {}, "chain_per_apply": {}}
    for part, lo, hi in (("filter_rows", 0, first_chain), ("chain_per_apply", first_chain, len(events))):
        by_name = {}
        for e in events[lo:hi]:
            nm = e.get("Kernel_Name", "")
            if any(k in nm for k in KERNELS):
                short = re.search(r"(\w+_kernel)", nm)[1]
                by_name.setdefault(short, []).append(int(e["End_Timestamp"]) - int(e["Start_Timestamp"]))
        for short, d in by_name.items():
            per_rep = len(d) // TRACE_REPS if part == "chain_per_apply" else 1
            steady = d[2 * per_rep:] if len(d) > 2 * per_rep else d       # the first calls carry the code load
            out[part][short] = {"launches_per_call": per_rep, "avg_us": sum(steady) / len(steady) / 1e3,
                                "min_us": min(steady) / 1e3, "max_us": max(steady) / 1e3,
                                "us_per_call": per_rep * sum(steady) / len(steady) / 1e3}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--no-train-step", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "bench_augment.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_augment: no GPU visible; this benchmark does not run without one")
    dev = torch.device("cuda:0")
    if a.trace_run:
        trace_run(dev)
        return
    step_before = None if a.no_train_step else bc.training_step_ms()
    k = augment.kernel_consts()
    res = {"sr": SR, "rows": ROWS, "seconds_per_row": SECONDS, "stages": len(CURVE), "piece": k["piece"],
           "block": k["block"], "chain_batch": BATCH, "chain_seconds_per_row": BATCH_SECONDS,
           "chain_reverb_responses": "3 x 0.5 s decaying noise"}
    # (a) the two cascades on the same rows and stages
    x, sos = filter_rows(dev), curve_sos()
    new, old = augment.biquad_cascade(x, sos), stress.apply_microphone_eq(x, SR, CURVE)
    res["old_kernel_peak_output"] = float(old.abs().max())
    if not res["old_kernel_peak_output"] < 1.0:
        raise SystemExit("bench_augment: the old kernel's clamp acted; the two cascades are not the same filter")
    res["max_abs_difference_new_old"] = float((new - old).abs().max())
    for tag, fn in (("scan", lambda: augment.biquad_cascade(x, sos)),
                    ("systolic", lambda: stress.apply_microphone_eq(x, SR, CURVE))):
        res[f"filter_call_ms_median_{tag}"], res[f"filter_call_ms_min_{tag}"] = bc.wall_ms(fn, a.reps)
    # (b) the chain
    aug, xb, lengths = chain(dev)
    plan = aug.draw(BATCH)
    res["chain_apply_ms_median"], res["chain_apply_ms_min"] = bc.wall_ms(lambda: aug.apply(xb, lengths, plan), a.reps)
    res["chain_draw_ms_median"], res["chain_draw_ms_min"] = bc.wall_ms(lambda: aug.draw(BATCH), a.reps)
    res["chain_mean_stages"] = float(plan.n_stages.mean())
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    res["kernels"] = kernel_rows(out.with_name(out.stem + "_kernel_stats.csv"))
    ka = res["kernels"]["filter_rows"]
    res["scan_kernel_us"], res["systolic_kernel_us"] = ka["augment_biquad_kernel"]["avg_us"], \
        ka["stress_biquad_kernel"]["avg_us"]
    res["systolic_over_scan_kernel_ratio"] = res["systolic_kernel_us"] / res["scan_kernel_us"]
    res["chain_kernels_us_per_apply"] = sum(v["us_per_call"] for v in res["kernels"]["chain_per_apply"].values())
    if not a.no_train_step:
        step_after = bc.training_step_ms()
        res["training_step_ms_fp32_batch256_before"], res["training_step_ms_fp32_batch256_after"] = step_before, step_after
        step = 0.5 * (step_before + step_after)
        res["chain_apply_to_training_step_ratio"] = res["chain_apply_ms_median"] / step
        res["chain_kernels_to_training_step_ratio"] = res["chain_kernels_us_per_apply"] / 1e3 / step
    out.write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

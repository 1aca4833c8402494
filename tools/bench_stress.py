"""Device cost of the stress conditions (pitchextractor_amd.stress) next to the inference they feed.

One resident batch: 64 rows of 4 s at 24 kHz.  Conditions: a 1.5-s impulse response (18 partitions), the three
microphone profiles, clipping at 10 %, AGC pumping at 10 dB.  Each condition is called in a loop between two device
events and the total is divided by the number of calls (a call includes its host work: the row plan, its copy to the
device, the output allocation).  Kernel times come from a run of their own under ``rocprofv3 --kernel-trace --stats``
(no counters), started here as a child process once the timing is done.  ``predict_f0`` of the same 64 rows (a randomly
initialised default JDCNet, one call per row as the sweep makes them) is timed in the same session.  Writes
profiles/bench_stress.json and profiles/bench_stress_kernel_stats.csv and prints the JSON line.  Needs a GPU.

    python tools/bench_stress.py               # time, trace, predict_f0
    python tools/bench_stress.py --trace-run   # what the traced child runs: a few calls of every condition

Not a gate: a sweep degrades the set once per condition and then runs the model on every row.
"""
import argparse
import csv
import json
import shutil
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from pitchextractor_amd import inference, stress, synthetic  # noqa: E402
from pitchextractor_amd.model import JDCNet  # noqa: E402

SR, ROWS, SECONDS, RIR_SECONDS = 24000, 64, 4.0, 1.5
KERNELS = ("stress_spectra_kernel", "stress_rir_convolve_kernel", "stress_rir_normalize_kernel", "stress_biquad_kernel",
           "stress_clip_kernel", "stress_agc_walk_kernel", "stress_agc_apply_kernel")


def make_batch(dev):
    waves = [synthetic.utterance(i, duration=SECONDS, sr=SR, hop=300)[0] for i in range(ROWS)]
    return torch.from_numpy(np.concatenate(waves)).to(dev), [len(w) for w in waves]


def make_rir():
    rng = np.random.default_rng(0)
    n = int(RIR_SECONDS * SR)
    return stress.RirSet([stress.prepare_rir(rng.standard_normal(n) * np.exp(-np.arange(n) / (n / 6.9)))])


def conditions(flat, lengths, rirs):
    calls = {"rir_1.5s": lambda: stress.apply_rir(flat, rirs, 0, lengths),
             "clipping_10pct": lambda: stress.apply_sample_clipping(flat, 10.0, lengths),
             "agc_10db": lambda: stress.apply_agc_pumping(flat, 10.0, SR, 0.15, lengths)}
    for name in stress.MICROPHONE_PROFILES:
        calls["microphone_" + name] = (lambda n=name: stress.apply_microphone_eq(flat, SR, n, lengths))
    return calls


def timed_loop(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def trace_run(dev):
    flat, lengths = make_batch(dev)
    for fn in conditions(flat, lengths, make_rir()).values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()


def kernel_rows(out_csv: Path):
    """Run the traced child; per-kernel (calls, avg / min / max us), rows kept in ``out_csv``."""
    prof = shutil.which("rocprofv3")
    if prof is None:
        raise SystemExit("bench_stress: rocprofv3 not found; kernel times are not optional")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "stress", "--",
               sys.executable, str(Path(__file__).resolve()), "--trace-run"]
        subprocess.run(cmd, check=True, timeout=600, stdout=subprocess.DEVNULL)
        stats = sorted(Path(tmp).rglob("*kernel_stats.csv"))
        if not stats:
            raise SystemExit("bench_stress: the profiler wrote no kernel_stats.csv")
        rows = list(csv.DictReader(open(stats[0])))
    keep = [r for r in rows if any(k in r.get("Name", "") for k in KERNELS)]
    if not keep:
        raise SystemExit("bench_stress: none of the stress kernels appear in the trace")
    with open(out_csv, "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=list(keep[0].keys()))
        w.writeheader()
        w.writerows(keep)
    per = {}
    for r in keep:
        name = next(k for k in KERNELS if k in r["Name"])
        calls = int(r["Calls"])
        per[name] = {"calls": calls, "avg_us": float(r["TotalDurationNs"]) / calls / 1e3,
                     "min_us": float(r["MinNs"]) / 1e3, "max_us": float(r["MaxNs"]) / 1e3}
    return per


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "bench_stress.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_stress: no GPU visible; this benchmark does not run without one")
    dev = torch.device("cuda:0")
    if args.trace_run:
        trace_run(dev)
        return
    flat, lengths = make_batch(dev)
    rirs = make_rir()
    res = {"sr": SR, "rows": ROWS, "samples": int(sum(lengths)), "rir_samples": rirs.lengths[0],
           "rir_partitions": rirs.plan["n_blocks"], "blocks": stress.plan_rows(lengths, [0] * ROWS, [0] * ROWS)["n_blocks"],
           "agc_smoothing": stress.agc_parameters(10.0, SR, 0.15)["smoothing"], "ms_per_call": {}}
    for name, fn in conditions(flat, lengths, rirs).items():
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        first = timed_loop(fn, 2)
        res["ms_per_call"][name] = timed_loop(fn, max(3, min(200, int(500.0 / max(first, 1e-3)))))
    torch.manual_seed(0)
    net = JDCNet(num_class=1).to(dev).eval()
    rows = [w.cpu().numpy() for w in torch.split(flat, lengths)]
    predict = lambda: [inference.predict_f0(net, w) for w in rows]  # noqa: E731
    predict()
    torch.cuda.synchronize()
    res["predict_f0_ms_all_rows"] = timed_loop(predict, 3)
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    res["kernels"] = kernel_rows(out.with_name(out.stem + "_kernel_stats.csv"))
    out.write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

"""Cost of reading pitch out of a model for a whole set: the per-row ``inference.predict_f0`` loop against
``inference.predict_f0_batch``.

Two resident sets at 24 kHz: the 64 rows of 4 s of tools/bench_stress.py, and one 5-minute row beside 63 rows of 2 s.
A randomly initialised default JDCNet (regression) serves both paths; they are timed alternately in one process after
a warm-up of each, with a host clock around a device synchronise (the per-row loop ends on the host anyway), and the
median of the repetitions is kept.  Kernel times of ``pe_mel_forward_chunks`` and ``pe_stitch_chunks`` come from a run
of their own under ``rocprofv3 --kernel-trace --stats`` (no counters), started here as a child process once the timing
is done: the child calls ``predict_f0_batch`` three times per (set, model) for the regression model and for a
722-class model without a decoder ("center": the stitch moves the logits once), and every dispatch is matched to its
call by its order.  Achieved bytes/s (stitch: one read and one write of the stitched logits; mel: the samples read once,
the chunks written) stand next to the rate of a device-to-device copy of 256 MiB measured in the same session.  Writes
profiles/bench_predict_batch.json and profiles/bench_predict_batch_kernel_stats.csv and prints the JSON line.  Needs a
GPU.  Not a gate.

    python tools/bench_predict_batch.py               # time, trace
    python tools/bench_predict_batch.py --trace-run   # what the traced child runs
"""
import argparse
import csv
import json
import shutil
import statistics
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from pitchextractor_amd import inference, synthetic  # noqa: E402
from pitchextractor_amd.model import JDCNet  # noqa: E402

SR, HOP, REPS, TRACE_CALLS = 24000, 300, 5, 3
KERNELS = {"mel": "mel_fwd_kernel", "stitch": "stitch_chunks_kernel"}
TRACE_CLASSES = (1, 722)


def make_sets():
    """name -> list of float32 waves."""
    four = [synthetic.utterance(i, duration=4.0, sr=SR, hop=HOP)[0] for i in range(64)]
    long_row = np.concatenate([synthetic.utterance(100 + i, duration=30.0, sr=SR, hop=HOP)[0] for i in range(10)])
    mixed = [long_row] + [synthetic.utterance(i, duration=2.0, sr=SR, hop=HOP)[0] for i in range(63)]
    return {"64_rows_of_4s": four, "5min_row_and_63_of_2s": mixed}


def upload(waves, dev):
    return torch.from_numpy(np.concatenate(waves)).to(dev), [len(w) for w in waves]


def clocked(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def copy_rate(dev):
    """bytes/s (read + write) of a device-to-device copy of 256 MiB."""
    src = torch.empty((64 << 20,), dtype=torch.float32, device=dev)
    dst = torch.empty_like(src)
    dst.copy_(src)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(10):
        dst.copy_(src)
    b.record()
    b.synchronize()
    return 2.0 * src.numel() * 4 * 10 / (a.elapsed_time(b) * 1e-3)


def trace_models(dev):
    torch.manual_seed(0)
    return [JDCNet(num_class=c).to(dev).eval() for c in TRACE_CLASSES]


def trace_run(dev):
    nets = trace_models(dev)
    for waves in make_sets().values():
        flat, lengths = upload(waves, dev)
        for net in nets:
            for _ in range(TRACE_CALLS):
                inference.predict_f0_batch(net, flat, lengths)
    torch.cuda.synchronize()


def traced_bytes():
    """Per traced (set, model), in the child's order: (label, mel bytes, stitch bytes)."""
    out = []
    for name, waves in make_sets().items():
        lengths = [len(w) for w in waves]
        plan = inference.chunk_plan([1 + n // HOP for n in lengths], 192, 48, "center")
        mel = 4 * sum(lengths) + 4 * plan["meta"].shape[0] * 192 * 80
        out += [(f"{name}/num_class_{c}", mel, 2 * 4 * plan["n_out"] * c) for c in TRACE_CLASSES]
    return out


def kernel_rows(out_csv: Path):
    prof = shutil.which("rocprofv3")
    if prof is None:
        raise SystemExit("bench_predict_batch: rocprofv3 not found; kernel times are not optional")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "predict", "--",
               sys.executable, str(Path(__file__).resolve()), "--trace-run"]
        subprocess.run(cmd, check=True, timeout=900, stdout=subprocess.DEVNULL)
        stats = sorted(Path(tmp).rglob("*kernel_stats.csv"))
        trace = sorted(Path(tmp).rglob("*kernel_trace.csv"))
        if not stats or not trace:
            raise SystemExit("bench_predict_batch: the profiler wrote no kernel_stats.csv / kernel_trace.csv")
        keep = [r for r in csv.DictReader(open(stats[0])) if any(k in r.get("Name", "") for k in KERNELS.values())]
        dispatches = list(csv.DictReader(open(trace[0])))
    if not keep:
        raise SystemExit("bench_predict_batch: neither kernel appears in the trace")
    with open(out_csv, "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=list(keep[0].keys()))
        w.writeheader()
        w.writerows(keep)
    dispatches.sort(key=lambda r: int(r["Start_Timestamp"]))
    cases = traced_bytes()
    per = {}
    for key, kernel in KERNELS.items():
        ns = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in dispatches if kernel in r["Kernel_Name"]]
        # the mel kernel also serves waveform_to_mel; the child makes no such call
        if len(ns) != TRACE_CALLS * len(cases):
            raise SystemExit(f"bench_predict_batch: {len(ns)} dispatches of {kernel}, expected {TRACE_CALLS * len(cases)}")
        for i, (label, mel_bytes, stitch_bytes) in enumerate(cases):
            us = [t / 1e3 for t in ns[i * TRACE_CALLS + 1:(i + 1) * TRACE_CALLS]]          # the first call warms up
            nbytes = mel_bytes if key == "mel" else stitch_bytes
            avg = sum(us) / len(us)
            per.setdefault(label, {})[key] = {"avg_us": avg, "min_us": min(us), "max_us": max(us), "bytes": nbytes,
                                              "bytes_per_s": nbytes / (avg * 1e-6)}
    return per


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "bench_predict_batch.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_predict_batch: no GPU visible; this benchmark does not run without one")
    dev = torch.device("cuda:0")
    if args.trace_run:
        trace_run(dev)
        return
    torch.manual_seed(0)
    net = JDCNet(num_class=1).to(dev).eval()
    res = {"sr": SR, "reps": REPS, "sets": {}}
    for name, waves in make_sets().items():
        flat, lengths = upload(waves, dev)
        per_row = lambda: [inference.predict_f0(net, w) for w in waves]  # noqa: E731
        paths = {"per_row_ms": per_row}
        for mode in inference.STITCH_MODES:
            paths[f"batch_{mode}_ms"] = (lambda m=mode: inference.predict_f0_batch(net, flat, lengths, stitch=m))
        for fn in paths.values():
            fn()
        times = {k: [] for k in paths}
        for _ in range(REPS):                           # alternating: drift of the clocks falls on every path alike
            for k, fn in paths.items():
                times[k].append(clocked(fn))
        plan = inference.chunk_plan([1 + n // HOP for n in lengths], 192, 48, "concat")
        entry = {"rows": len(waves), "samples": int(sum(lengths)), "chunks": int(plan["meta"].shape[0])}
        for k, v in times.items():
            entry[k] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
        res["sets"][name] = entry
    res["copy_bytes_per_s"] = copy_rate(dev)
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    res["kernels"] = kernel_rows(out.with_name(out.stem + "_kernel_stats.csv"))
    out.write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

"""Device cost of decoding F0 classifier logits (ops.decode_f0_bins) next to the forward that produces them.

Resident logits of the inference batch, 256 chunks x 192 frames x 360 bins (70.8 MB); each of the four decoders and,
in the same process, the eval forward of the same 256-chunk batch through JDCNet(num_class=360).  The kernels are
short, so each item is looped between two device events for its share of a window of about a second per item, the
items taking turns (alternating rounds), and the total is divided by the number of calls.  Kernel times come from a
run of their own under ``rocprofv3 --kernel-trace --stats`` (no counters), started here as a child process once the
timing is done.  Writes profiles/bench_f0_decode.json and profiles/bench_f0_decode_kernel_stats.csv and prints the
JSON line.  Needs a GPU: without one it fails, it does not fall back.

    python tools/bench_f0_decode.py               # time, then trace
    python tools/bench_f0_decode.py --trace-run   # what the traced child runs: a few calls of each decoder

Gate: every decoder must take less time than the eval forward of the same batch (decoding must never be what an
inference call waits for); exit status 1 otherwise.  The frame-wise pass is bound by HBM (one read of the logits):
its share of the 6.29 TB/s copy rate is reported.  The Viterbi kernel is bound by latency (one barrier and 23 LDS
reads per frame): its time is reported, not a share of a peak.
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

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from pitchextractor_amd import ops  # noqa: E402
from pitchextractor_amd.model import JDCNet  # noqa: E402

N, T, C = 256, 192, 360
HBM_COPY_TBS = 6.29                       # measured copy rate of the MI355X microarchitecture guide
KERNELS = ("f0_decode_frames_kernel", "f0_viterbi_kernel", "pitch_metrics_kernel")


def make_logits(dev):
    """A ridge along a glide plus N(0, 1) noise: the kind of rows a trained classifier gives."""
    g = torch.Generator(device="cpu").manual_seed(0)
    centre = torch.linspace(60.0, 240.0, T)[None, :, None] + 40.0 * torch.rand((N, 1, 1), generator=g)
    bins = torch.arange(C, dtype=torch.float32)[None, None, :]
    x = torch.clamp(-0.5 * ((bins - centre) / 1.25) ** 2, min=-30.0) + torch.randn((N, T, C), generator=g)
    return x.to(dev)


def trace_run(dev):
    x = make_logits(dev)
    for _ in range(20):
        for m in ops.F0_DECODERS:
            f0, _, _ = ops.decode_f0_bins(x, None, m)
        ops.pitch_metrics(f0.reshape(-1), f0.reshape(-1))
    torch.cuda.synchronize()


def timed_loop(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def kernel_stats(out_csv: Path) -> dict:
    """Run the traced child, keep the rows of this file's kernels in ``out_csv``; {kernel: average microseconds}."""
    prof = shutil.which("rocprofv3")
    if prof is None:
        raise SystemExit("bench_f0_decode: rocprofv3 not found; kernel times are not optional")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "f0_decode", "--",
               sys.executable, str(Path(__file__).resolve()), "--trace-run"]
        subprocess.run(cmd, check=True, timeout=300, stdout=subprocess.DEVNULL)
        found = sorted(Path(tmp).rglob("*kernel_stats.csv"))
        if not found:
            raise SystemExit("bench_f0_decode: the profiler wrote no kernel_stats.csv")
        rows = list(csv.DictReader(open(found[0])))
    keep = [r for r in rows if any(k in r.get("Name", "") for k in KERNELS)]
    if not keep:
        raise SystemExit("bench_f0_decode: none of the decode kernels appear in the trace")
    with open(out_csv, "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=list(keep[0].keys()))
        w.writeheader()
        w.writerows(keep)
    out = {}
    for r in keep:
        name = next(k for k in KERNELS if k in r["Name"])
        out[name] = {"calls": int(r["Calls"]), "avg_us": float(r["AverageNs"]) / 1e3,
                     "min_us": float(r["MinNs"]) / 1e3, "max_us": float(r["MaxNs"]) / 1e3}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=1.0, help="seconds of timed work per item")
    ap.add_argument("--rounds", type=int, default=4, help="alternating rounds the window is split into")
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "bench_f0_decode.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_f0_decode: no GPU visible; this benchmark does not run without one")
    dev = torch.device("cuda:0")
    if args.trace_run:
        trace_run(dev)
        return

    x = make_logits(dev)
    net = JDCNet(num_class=C).to(dev).eval()
    mel = torch.randn((N, 1, 80, T), generator=torch.Generator().manual_seed(1)).to(dev)

    def forward():
        with torch.no_grad():
            net(mel.transpose(-1, -2))

    items = {m: (lambda m=m: ops.decode_f0_bins(x, None, m)) for m in ops.F0_DECODERS}
    items["eval_forward"] = forward
    calls = {}
    for name, fn in items.items():                # warm up every shape, then size each loop to its share of time
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        per_call_ms = timed_loop(fn, 5) / 5
        calls[name] = max(5, int(args.window * 1e3 / args.rounds / max(per_call_ms, 1e-3)))
    total = {k: 0.0 for k in items}
    t0 = time.time()
    for _ in range(args.rounds):
        for name, fn in items.items():
            total[name] += timed_loop(fn, calls[name])
    res = {"N": N, "T": T, "C": C, "logits_mb": N * T * C * 4 / 1e6, "rounds": args.rounds,
           "wall_s": round(time.time() - t0, 2)}
    fwd = total["eval_forward"] / (args.rounds * calls["eval_forward"])
    res["eval_forward_ms"] = fwd
    res["methods"] = {}
    for m in ops.F0_DECODERS:
        ms = total[m] / (args.rounds * calls[m])
        res["methods"][m] = {"ms_per_call": ms, "calls": args.rounds * calls[m], "ratio_to_eval_forward": ms / fwd}
    res["gate"] = "every decoder faster than the eval forward of the same batch"
    res["gate_passed"] = all(v["ratio_to_eval_forward"] < 1.0 for v in res["methods"].values())

    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    res["kernels"] = kernel_stats(out.with_name(out.stem + "_kernel_stats.csv"))
    fr = res["kernels"].get("f0_decode_frames_kernel")
    if fr:
        moved = N * T * C * 4 + N * T * 12                           # one read of the logits, three (N, T) outputs
        tbs = moved / (fr["avg_us"] * 1e-6) / 1e12
        res["frames_pass"] = {"bytes": moved, "achieved_tb_s": tbs, "share_of_copy_rate": tbs / HBM_COPY_TBS,
                              "copy_rate_tb_s": HBM_COPY_TBS, "bound": "HBM"}
    res["viterbi_note"] = "latency-bound (one barrier and 23 LDS reads per frame per sequence): time, not a share"
    out.write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))
    if not res["gate_passed"]:
        raise SystemExit(1)


if __name__ == "__main__":
    main()

"""Device cost of the codec stress conditions (``pitchextractor_amd.codec``).

Reports, from one session, on 64 rows of 4 s at 24 kHz (the rows of tools/bench_predict_batch.py): the fused transform
codec call (``TransformCodec.__call__``, 64 kbps, frames of 1024 and of 256), its three stage calls, ``apply_mulaw`` and
``apply_g711u``, each per call with its host work (the row plan, its copy to the device, the output allocation; wall
clock around a synchronize), beside ``predict_f0_batch`` over the same rows and a device-to-device copy of 256 MiB
measured in the same session.  Kernel times come from a run of its own under ``rocprofv3 --kernel-trace --stats`` (no
counters) started here as a child process; each kernel's bytes (what the algorithm has to move, computed from the
shapes) over its time is given as a share of the measured copy rate.  Writes profiles/bench_codec.json and
profiles/bench_codec_kernel_stats.csv and prints the JSON line.  Needs a GPU.

    python tools/bench_codec.py               # time and trace
    python tools/bench_codec.py --trace-run   # what the traced child runs

Not a gate.  What bounds a kernel is not said here: that takes a counter run.
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

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
import bench_cheaptrick as bc  # noqa: E402
import bench_predict_batch as bp  # noqa: E402
from pitchextractor_amd import codec, inference, synthetic  # noqa: E402
from pitchextractor_amd.model import JDCNet  # noqa: E402

SR, HOP, ROWS, SECONDS, KBPS = 24000, 300, 64, 4.0, 64
FRAMES = (1024, 256)
TRACE_REPS = 6


def make_rows(dev):
    waves = [synthetic.utterance(i, duration=SECONDS, sr=SR, hop=HOP)[0] for i in range(ROWS)]
    return bp.upload(waves, dev)


def calls(x, lengths):
    """name -> thunk, in the order the traced child runs them."""
    out = {}
    for M in FRAMES:
        c = codec.TransformCodec(SR, KBPS, M)
        X, _ = c.mdct(x, lengths)
        deq = c.quantize(X)[3]
        out[f"apply_{M}"] = lambda c=c: c(x, lengths)
        out[f"mdct_{M}"] = lambda c=c: c.mdct(x, lengths)
        out[f"quantize_{M}"] = lambda c=c, X=X: c.quantize(X)
        out[f"imdct_{M}"] = lambda c=c, deq=deq: c.imdct(deq, x, lengths)
    out["mulaw"] = lambda: codec.apply_mulaw(x, lengths)
    out["g711u"] = lambda: codec.apply_g711u(x, SR, lengths)
    return out


def trace_run(dev):
    x, lengths = make_rows(dev)
    for name, fn in calls(x, lengths).items():
        for _ in range(TRACE_REPS if name != "g711u" else 0):        # its mu-law has another size: wall clock only
            fn()
    torch.cuda.synchronize()


def kernel_bytes(n_samples, n_frames):
    """kernel name fragment -> bytes the algorithm moves per launch, by frame size."""
    out = {}
    for M in FRAMES:
        F = n_frames[M]
        out[M] = {"codec_frames_kernel<1>": 4 * (2 * n_samples + F * M), "codec_quantize_kernel": 4 * 3 * F * M,
                  "codec_frames_kernel<2>": 4 * (F * M + 2 * F * M),
                  "codec_frames_kernel<3>": 4 * (2 * n_samples + 2 * F * M),
                  "codec_overlap_kernel": 4 * (2 * F * M + n_samples)}
    return out


def kernel_rows(out_csv: Path):
    prof = shutil.which("rocprofv3")
    if prof is None:
        raise SystemExit("bench_codec: rocprofv3 not found; kernel times are not optional")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "codec", "--",
               sys.executable, str(Path(__file__).resolve()), "--trace-run"]
        subprocess.run(cmd, check=True, timeout=600, stdout=subprocess.DEVNULL)
        stats = sorted(Path(tmp).rglob("*kernel_stats.csv"))
        trace = sorted(Path(tmp).rglob("*kernel_trace.csv"))
        if not stats or not trace:
            raise SystemExit("bench_codec: the profiler wrote no kernel_stats.csv / kernel_trace.csv")
        rows = list(csv.DictReader(open(stats[0])))
        events = list(csv.DictReader(open(trace[0])))
    keep = [r for r in rows if "codec_" in r.get("Name", "")]
    if not keep:
        raise SystemExit("bench_codec: the codec kernels do not appear in the trace")
    with open(out_csv, "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=list(keep[0].keys()))
        w.writeheader()
        w.writerows(keep)
    by_name = {}
    for e in events:
        nm = e.get("Kernel_Name", "")
        m = re.search(r"(codec_\w+_kernel)(?:<(\d+)(?:, *(\d+))?>)?", nm)
        if m:
            short = m[1] + (f"<{m[3]}>" if m[3] else "") + (f" M={m[2]}" if m[2] else "")
            by_name.setdefault(short, []).append(int(e["End_Timestamp"]) - int(e["Start_Timestamp"]))
    out = {}
    for short, d in by_name.items():
        steady = d[2:] if len(d) > 4 else d                     # the first calls carry the code load
        out[short] = {"launches": len(d), "avg_us": sum(steady) / len(steady) / 1e3, "min_us": min(steady) / 1e3,
                      "max_us": max(steady) / 1e3}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "bench_codec.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_codec: no GPU visible; this benchmark does not run without one")
    dev = torch.device("cuda:0")
    if a.trace_run:
        trace_run(dev)
        return
    x, lengths = make_rows(dev)
    n_samples = int(sum(lengths))
    res = {"sr": SR, "rows": ROWS, "seconds_per_row": SECONDS, "bitrate_kbps": KBPS, "samples": n_samples,
           "copy_rate_TBps": bp.copy_rate(dev) / 1e12, "call_ms": {}}
    n_frames = {}
    for M in FRAMES:
        c = codec.TransformCodec(SR, KBPS, M)
        n_frames[M] = int(c.plan(lengths)["n_frames"])
        res[f"frames_{M}"], res[f"budget_bits_{M}"], res[f"cutoff_bin_{M}"] = n_frames[M], c.budget, c.cutoff_bin
    for name, fn in calls(x, lengths).items():
        med, lo = bc.wall_ms(fn, a.reps)
        res["call_ms"][name] = {"median": med, "min": lo}
    torch.manual_seed(0)
    net = JDCNet(num_class=1).to(dev).eval()
    med, lo = bc.wall_ms(lambda: inference.predict_f0_batch(net, x, lengths), max(a.reps // 3, 5))
    res["predict_f0_batch_ms"] = {"median": med, "min": lo}
    res["apply_1024_to_predict_ratio"] = res["call_ms"]["apply_1024"]["median"] / med
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    res["kernels"] = kernel_rows(out.with_name(out.stem + "_kernel_stats.csv"))
    nbytes = kernel_bytes(n_samples, n_frames)
    for short, k in res["kernels"].items():
        m = re.match(r"(codec_\w+_kernel(?:<\d>)?)(?: M=(\d+))?", short)
        if short.startswith("codec_mulaw"):
            k["bytes"] = 8 * n_samples
        elif m and m[2] and m[1] in nbytes[int(m[2])]:
            k["bytes"] = nbytes[int(m[2])][m[1]]
        if "bytes" in k:
            k["share_of_copy_rate"] = k["bytes"] / (k["avg_us"] * 1e-6) / 1e12 / res["copy_rate_TBps"]
    out.write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

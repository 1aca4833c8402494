"""Cost of the room-response library (pitchextractor_amd.rir): the nine (room, T60) entries of the reference's
Utils/room_and_microphone_stress.ipynb at 24 kHz.

Timed with their host work (room table, plan, tile table, uploads, the output allocation and, for the measurement,
the copy of the result to the host), wall clock around a device synchronisation: the calibrated ``room_library`` call
(one ``synthesize`` and one ``measure_t60`` per bisection step), the synthesis alone (the nine calibrated rooms as one
ragged batch, one launch) and the measurement alone (the nine responses, one launch).  The per-kernel split comes from
a run of its own under ``rocprofv3 --kernel-trace --stats`` (no counters), started here as a child process once the
timing is done: the child builds the library once and then makes and measures the batch three times.  The same rows for
the float64 restatement in tests/rir_ref.py on the CPU, for the entries whose estimated image count stays below
``--ref-images`` (the others are listed with their estimate).  Writes profiles/bench_rir_synth.json and
profiles/bench_rir_synth_kernel_stats.csv and prints the JSON line.  Needs a GPU; there is no fallback.

    python tools/bench_rir_synth.py               # time, trace, CPU restatement
    python tools/bench_rir_synth.py --trace-run   # what the traced child runs

Not a gate: the library is made once per sweep, not once per training step.
"""
import argparse
import csv
import json
import math
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
from pitchextractor_amd import rir  # noqa: E402

FS = 24000
KERNELS = ("rir_synth_kernel", "rir_decay_kernel")


def wall_ms(fn, calls=1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls, out


def library_rooms(lib):
    return [dict(rir.ROOMS[e["room"]], beta=e["beta"], n_samples=n) for e, n in zip(lib.entries, lib.lengths)]


def estimated_images(room, fs, c=343.0):
    radius = (room["n_samples"] + 41) * c / fs
    return 4.0 / 3.0 * math.pi * radius ** 3 / float(np.prod(room["dims"]))


def trace_run(dev):
    lib = rir.room_library(FS, device=dev)
    rooms = library_rooms(lib)
    for _ in range(3):
        h, lengths = rir.synthesize(rooms, FS, device=dev)
        rir.measure_t60(h, lengths, FS)
    torch.cuda.synchronize()


def kernel_rows(out_csv: Path):
    """Run the traced child; per-kernel (calls, avg / min / max us, total ms), rows kept in ``out_csv``."""
    prof = shutil.which("rocprofv3")
    if prof is None:
        raise SystemExit("bench_rir_synth: rocprofv3 not found; kernel times are not optional")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "rir", "--",
               sys.executable, str(Path(__file__).resolve()), "--trace-run"]
        subprocess.run(cmd, check=True, timeout=600, stdout=subprocess.DEVNULL)
        stats = sorted(Path(tmp).rglob("*kernel_stats.csv"))
        if not stats:
            raise SystemExit("bench_rir_synth: the profiler wrote no kernel_stats.csv")
        rows = list(csv.DictReader(open(stats[0])))
    keep = [r for r in rows if any(k in r.get("Name", "") for k in KERNELS)]
    if not keep:
        raise SystemExit("bench_rir_synth: none of the rir kernels appear in the trace")
    with open(out_csv, "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=list(keep[0].keys()))
        w.writeheader()
        w.writerows(keep)
    per = {}
    for r in keep:
        name = next(k for k in KERNELS if k in r["Name"])
        calls = int(r["Calls"])
        per[name] = {"calls": calls, "avg_us": float(r["TotalDurationNs"]) / calls / 1e3,
                     "min_us": float(r["MinNs"]) / 1e3, "max_us": float(r["MaxNs"]) / 1e3,
                     "total_ms": float(r["TotalDurationNs"]) / 1e6}
    return per


def cpu_rows(lib, limit):
    """The restatement on the CPU, entry by entry: seconds of the synthesis and of the measurement."""
    from tests import rir_ref
    rows = []
    for e, room in zip(lib.entries, library_rooms(lib)):
        row = {"room": e["room"], "target_t60": e["target_t60"], "n_samples": room["n_samples"],
               "estimated_images": estimated_images(room, FS)}
        if row["estimated_images"] <= limit:
            t0 = time.perf_counter()
            h, K, _ = rir_ref.image_source(room, float(FS))
            t1 = time.perf_counter()
            m = rir_ref.schroeder(h, float(FS))
            t2 = time.perf_counter()
            got = lib.responses()[e["index"]]
            err = np.abs(got.astype(np.float64) - h.astype(np.float64))
            bound = 2.0 ** -24 * np.abs(h.astype(np.float64)) + K * 2.0 ** -44       # tests/test_rir_gpu.py's
            row.update(synthesis_s=t1 - t0, measurement_s=t2 - t1, t60=m["t60"], contributions=int(K.sum()),
                       samples_differing=int(np.count_nonzero(got != h)), max_abs_difference=float(err.max()),
                       within_bound=bool(np.all(err <= bound)))
        else:
            row["skipped"] = "above --ref-images"
        print(f"[bench_rir_synth] cpu {json.dumps(row)}", flush=True)
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--ref-images", type=float, default=1.5e6)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "bench_rir_synth.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rir_synth: no GPU visible; this benchmark does not run without one")
    dev = torch.device("cuda:0")
    if args.trace_run:
        trace_run(dev)
        return
    rir.synthesize([dict(rir.ROOMS["small_room"], beta=0.5, n_samples=2000)], FS, device=dev)     # loads the library
    first_ms, lib = wall_ms(lambda: rir.room_library(FS, device=dev))
    again_ms, lib = wall_ms(lambda: rir.room_library(FS, device=dev))
    rooms = library_rooms(lib)
    res = {"fs": FS, "entries": [dict(e, n_samples=n, estimated_images=estimated_images(r, FS))
                                 for e, n, r in zip(lib.entries, lib.lengths, rooms)],
           "tile": rir.plan_rooms([], FS)["tile"], "tiles": rir.plan_rooms(rooms, FS)["n_tiles"],
           "samples": int(sum(lib.lengths)), "ms": {"room_library_first_call": first_ms, "room_library": again_ms}}
    print(f"[bench_rir_synth] library {json.dumps(res['ms'])}", flush=True)
    synth_ms, (h, lengths) = wall_ms(lambda: rir.synthesize(rooms, FS, device=dev), 3)
    res["ms"]["synthesize_nine"] = synth_ms
    res["ms"]["measure_t60_nine"] = wall_ms(lambda: rir.measure_t60(h, lengths, FS), 10)[0]
    res["batch_equals_library"] = bool(torch.equal(h, lib.h))
    print(f"[bench_rir_synth] {json.dumps(res['ms'])}", flush=True)
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    res["kernels"] = kernel_rows(out.with_name(out.stem + "_kernel_stats.csv"))
    print(f"[bench_rir_synth] kernels {json.dumps(res['kernels'])}", flush=True)
    res["cpu_restatement"] = cpu_rows(lib, args.ref_images)
    out.write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

"""Device cost of labelling a batch with the on-device F0 tracker (f0_tracker.PraatACTracker) next to training on it.

Two resident batches at 24 kHz, hop 300, reference defaults (min_pitch 40: 1798-sample window, 4096-point FFT):
``uniform`` = 256 rows of 4 s (314 frames each) and ``ragged`` = one 5-minute row beside 255 rows of 2 s.  Each batch
is tracked in a loop between two device events for its share of a window, the batches taking turns, and the total is
divided by the number of calls (``track`` includes its host work: plan, five launches, one device-to-host copy of the
contours).  Kernel times come from a run of their own under ``rocprofv3 --kernel-trace --stats`` (no counters), started
here as a child process once the timing is done.  The training step of the flagship batch (256 utterances x 192
frames, fp32) is measured in the same session by running bench.py as a child process.  Writes
profiles/bench_f0_track.json and profiles/bench_f0_track_kernel_stats.csv and prints the JSON line.  Needs a GPU.

    python tools/bench_f0_track.py               # time, trace, training step
    python tools/bench_f0_track.py --trace-run   # what the traced child runs: a few calls on each batch
    python tools/bench_f0_track.py --configurations-only   # only re-measure the configuration cases, in place

Not a gate: labelling happens once per file, not once per step.  The frame kernel is bound by VALU and LDS (two
4096-point real transforms and about 15 x 13 sinc evaluations of 140 taps per frame), the path kernel by latency (one
dependent step per frame per row); bytes moved and FFT flop per launch are reported with the share of the 6.29 TB/s
copy rate and of the fp32 vector peak they imply.
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
from pitchextractor_amd.f0_tracker import N_CAND, PraatACTracker  # noqa: E402

SR, HOP = 24000, 300
HBM_COPY_TBS = 6.29                       # measured copy rate of the MI355X microarchitecture guide
VALU_FP32_TFLOPS = 157.3                  # vector fp32 peak (spec) of the same guide
KERNELS = ("f0_sum_kernel", "f0_peak_kernel", "f0_peak_final_kernel", "f0_frames_kernel", "f0_path_kernel")


def make_batches(dev):
    def rows(count, seconds):
        return [synthetic.utterance(i, duration=seconds, sr=SR, hop=HOP)[0] for i in range(count)]
    uniform = rows(256, 4.0)
    long_row = np.concatenate([synthetic.utterance(1000 + i, duration=10.0, sr=SR, hop=HOP)[0] for i in range(30)])
    ragged = [long_row] + rows(255, 2.0)
    out = {}
    for name, waves in (("uniform", uniform), ("ragged", ragged)):
        out[name] = (torch.from_numpy(np.concatenate(waves)).to(dev), [len(w) for w in waves])
    return out


def trace_run(dev):
    tr = PraatACTracker(SR, HOP)
    for name, (flat, lengths) in make_batches(dev).items():
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
    """Run the traced child; per-kernel (calls, total / min / max ns) over both batches, rows kept in ``out_csv``."""
    prof = shutil.which("rocprofv3")
    if prof is None:
        raise SystemExit("bench_f0_track: rocprofv3 not found; kernel times are not optional")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "f0_track", "--",
               sys.executable, str(Path(__file__).resolve()), "--trace-run"]
        subprocess.run(cmd, check=True, timeout=600, stdout=subprocess.DEVNULL)
        stats = sorted(Path(tmp).rglob("*kernel_stats.csv"))
        trace = sorted(Path(tmp).rglob("*kernel_trace.csv"))
        if not stats or not trace:
            raise SystemExit("bench_f0_track: the profiler wrote no kernel_stats.csv / kernel_trace.csv")
        rows = list(csv.DictReader(open(stats[0])))
        events = list(csv.DictReader(open(trace[0])))
    keep = [r for r in rows if any(k in r.get("Name", "") for k in KERNELS)]
    if not keep:
        raise SystemExit("bench_f0_track: none of the tracker kernels appear in the trace")
    with open(out_csv, "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=list(keep[0].keys()))
        w.writeheader()
        w.writerows(keep)
    # the two batches alternate in blocks of five calls: split each kernel's launches into the two halves in time order
    per = {}
    for k in KERNELS:
        ev = sorted((int(e["Start_Timestamp"]), int(e["End_Timestamp"]) - int(e["Start_Timestamp"]))
                    for e in events if k in e.get("Kernel_Name", ""))
        half = len(ev) // 2
        for name, part in (("uniform", ev[:half]), ("ragged", ev[half:])):
            d = [x[1] for x in part]
            if d:
                per.setdefault(name, {})[k] = {"calls": len(d), "avg_us": sum(d) / len(d) / 1e3, "min_us": min(d) / 1e3,
                                               "max_us": max(d) / 1e3}
    return per


def training_step_ms():
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "10", "--warmup", "3", "--no-cpu-baseline",
           "--no-native-ref"]
    res = subprocess.run(cmd, check=True, timeout=900, capture_output=True, text=True, cwd=str(ROOT))
    line = [ln for ln in res.stdout.splitlines() if ln.startswith("{")][-1]
    return float(json.loads(line)["ms_per_step"])


def deviation_records(dev):
    """What tests/test_f0_track_gpu.py asserts, as figures: per test configuration the yardstick (float32 against
    float64 restatement on that configuration's inputs) and the kernel's worst deviation from the float64 restatement
    on the same inputs; the tests allow a ratio of 4."""
    from tests import f0_track_ref as R
    out = []
    for cfg in R.GPU_CONFIGS + [R.SPILL_CONFIG]:
        sr, hop, mp, seconds = cfg
        tr = PraatACTracker(sr, hop, min_pitch=mp)
        yard = R.config_yardstick(*cfg)
        rec = {"sr": sr, "hop": hop, "min_pitch": mp, "n_fft": tr.n_fft, "yardstick": yard}
        for kind, waves, refs in (("margin", R.config_margin_inputs(*cfg), [a for a, _ in R.reference_pairs(*cfg)]),
                                  ("natural", R.natural_inputs(sr), [a for a, _ in R.natural_pairs(sr, hop, mp)])):
            got = tr.track(torch.from_numpy(np.concatenate(waves)).to(dev), [len(w) for w in waves],
                           return_candidates=True)
            devs = []
            for r, ref in enumerate(refs):
                o, n = int(got["frame_offsets"][r]), int(got["frames"][r])
                devs.append(R.deviation(ref, dict(f0=got["f0"][r], cand_f=got["cand_f"][o:o + n],
                                                  cand_s=got["cand_s"][o:o + n], cand_n=got["cand_n"][o:o + n])))
            rec[kind] = {"frames": sum(d["frames"] for d in devs), "voicing_flips": sum(d["voicing_flips"] for d in devs),
                         "set_mismatches": sum(d["set_mismatches"] for d in devs),
                         "contour_cents": max(d["contour_cents"] for d in devs)}
            if kind == "margin":
                rec[kind].update(candidate_cents=max(d["cents"] for d in devs),
                                 strength=max(d["strength"] for d in devs))
        rec["ratio_to_yardstick"] = {"margin_cents": rec["margin"]["candidate_cents"] / yard["cents"],
                                     "margin_strength": rec["margin"]["strength"] / yard["strength"],
                                     "natural_contour_cents": rec["natural"]["contour_cents"] / yard["natural_cents"]}
        out.append(rec)
    return out


def configuration_records(dev):
    """What tests/test_f0_track_config_gpu.py asserts, as figures: per case of ``f0_track_ref.CONFIG_CASES`` the
    yardsticks of its own rows and the kernel's deviation from the float64 restatement, per row kind (the test's
    assertions run on the way)."""
    from tests import f0_track_ref as R
    from tests.test_f0_track_config_gpu import run_case
    out = []
    for case in R.CONFIG_CASES:
        name, sr, hop, mp, config, inputs = case
        yard, devs = run_case(case)
        rec = {"case": name, "sr": sr, "hop": hop, "min_pitch": mp, "config": dict(config), "inputs": inputs,
               "yardstick": yard}
        for kind in ("margin", "natural"):
            rows = [d for d in devs if d["kind"] == kind]
            if rows:
                rec[kind] = {"rows": len(rows), "frames": sum(d["frames"] for d in rows),
                             "voicing_flips": sum(d["voicing_flips"] for d in rows),
                             "set_mismatches": sum(d["set_mismatches"] for d in rows),
                             "frames_with_another_set": sum(d["set_other"] for d in rows),
                             "candidate_cents": max(d["cents" if kind == "margin" else "set_cents"] for d in rows),
                             "strength": max(d["strength" if kind == "margin" else "set_strength"] for d in rows),
                             "contour_cents": max(d["contour_cents"] for d in rows)}
        out.append(rec)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=2.0, help="seconds of timed work per batch")
    ap.add_argument("--configurations-only", action="store_true",
                    help="measure only kernel_vs_float64_restatement_configurations and put it into the existing --out")
    ap.add_argument("--rounds", type=int, default=4, help="alternating rounds the window is split into")
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--no-train-step", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "bench_f0_track.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_f0_track: no GPU visible; this benchmark does not run without one")
    dev = torch.device("cuda:0")
    if args.trace_run:
        trace_run(dev)
        return
    if args.configurations_only:
        res = json.loads(Path(args.out).read_text())
        res["kernel_vs_float64_restatement_configurations"] = configuration_records(dev)
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
        print(json.dumps(res["kernel_vs_float64_restatement_configurations"]))
        return
    tr = PraatACTracker(SR, HOP)
    batches = make_batches(dev)
    items = {name: (lambda fl=flat, ln=lengths: tr.track(fl, ln)) for name, (flat, lengths) in batches.items()}
    calls = {}
    for name, fn in items.items():
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        per_call_ms = timed_loop(fn, 3) / 3
        calls[name] = max(3, int(args.window * 1e3 / args.rounds / max(per_call_ms, 1e-3)))
    total = {k: 0.0 for k in items}
    t0 = time.time()
    for _ in range(args.rounds):
        for name, fn in items.items():
            total[name] += timed_loop(fn, calls[name])
    res = {"sr": SR, "hop": HOP, "n_fft": tr.n_fft, "window_samples": tr.nsamp_window, "rounds": args.rounds,
           "wall_s": round(time.time() - t0, 2), "batches": {}}
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    kern = kernel_rows(out.with_name(out.stem + "_kernel_stats.csv"))
    fft_flop = 2 * 2.5 * tr.n_fft * np.log2(tr.n_fft)
    for name, (flat, lengths) in batches.items():
        plan = tr.plan(lengths)
        G = plan["n_frames"]
        ms = total[name] / (args.rounds * calls[name])
        b = {"rows": len(lengths), "samples": int(sum(lengths)), "frames": G, "longest_row_frames": int(max(plan["frames"])),
             "ms_per_track_call": ms, "calls": args.rounds * calls[name], "kernels": kern.get(name, {})}
        k = b["kernels"]
        for sk in ("f0_sum_kernel", "f0_peak_kernel"):
            if sk in k:
                moved = 4 * sum(lengths)                                 # one pass over the audio each
                tbs = moved / (k[sk]["avg_us"] * 1e-6) / 1e12
                k[sk].update(bytes=moved, achieved_tb_s=tbs, share_of_copy_rate=tbs / HBM_COPY_TBS)
        if "f0_frames_kernel" in k:
            moved = 4 * sum(lengths) + G * (2 * N_CAND * 4 + 4)          # audio once from HBM, candidates written
            us = k["f0_frames_kernel"]["avg_us"]
            k["f0_frames_kernel"].update(bytes_hbm=moved, window_bytes_l2=G * tr.nsamp_window * 4,
                                         share_of_copy_rate=moved / (us * 1e-6) / 1e12 / HBM_COPY_TBS,
                                         fft_flop=G * fft_flop,
                                         fft_share_of_valu_peak=G * fft_flop / (us * 1e-6) / 1e12 / VALU_FP32_TFLOPS,
                                         us_per_frame_per_cu=us * 256 / max(G, 1), bound="VALU / LDS")
        if "f0_path_kernel" in k:
            k["f0_path_kernel"].update(bytes=G * (2 * N_CAND * 4 + 8),
                                       ns_per_step_longest_row=k["f0_path_kernel"]["avg_us"] * 1e3 /
                                       max(b["longest_row_frames"], 1), bound="latency (one dependent step per frame)")
        res["batches"][name] = b
    res["kernel_vs_float64_restatement"] = deviation_records(dev)
    res["kernel_vs_float64_restatement_configurations"] = configuration_records(dev)
    if not args.no_train_step:
        step = training_step_ms()
        res["training_step_ms_fp32_batch256"] = step
        res["label_to_training_step_ratio"] = {n: b["ms_per_track_call"] / step for n, b in res["batches"].items()}
    out.write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

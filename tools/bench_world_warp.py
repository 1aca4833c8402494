"""Device cost of the voice transforms of WORLD frames (csrc/world_warp.hip) and of the resynthesis rows that use them
(``world_resynthesis`` with a ``transform`` block).

The rows of tools/bench_cheaptrick.py: 64 rows of 4 s at 24 kHz, 12.5 ms frames (hop 300, 20 544 source frames) -- the
share a ``ratio: 0.25`` batch of 256 carries.  Reports, from one session: (1) the warp launch alone, from a run of its
own under ``rocprofv3 --kernel-trace --stats`` (no counters) started here as a child process, in three variants: the
identity (the copy branch), formant + tilt + breath at rate 1 (one source frame per output frame) and the same at rate
0.8 (two source frames per output frame, 25 664 output frames), each with an aperiodicity of the envelope's layout; next
to each its bytes moved over that time as a share of the 6.29 TB/s copy rate, and ``pe_d4c_expand``'s share from
profiles/bench_d4c.json; (2) ``warp_envelopes`` with its host work (wall clock around a synchronize); (3) the loader
stage (``DeviceMelLoader._run_stage`` of the ``world_resynthesis`` kind) for a B = 256 batch with 64 resynthesis rows
cropped to the 192-frame window, with and without transforms, in ``d4c`` mode and with a constant template; (4) the fp32
training step of the flagship batch (bench.py as a child process) before and after the rest, so that the shares are of
this session's step.  With ``--ratios FILE`` the accuracy ratios and tracker figures (the ``[world_warp]`` records
tests/test_world_warp_gpu.py prints) are copied in.  Writes profiles/bench_world_warp.json and
profiles/bench_world_warp_kernel_stats.csv and prints the JSON line.  Needs a GPU.

    python tools/bench_world_warp.py               # time, trace, training step
    python tools/bench_world_warp.py --trace-run   # what the traced child runs

Not a gate.  No counter run is made here.
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
BINS = N // 2 + 1
KERNEL = "world_warp_kernel"
VT = world.VoiceTransform
# name -> (transform, source rows read per output frame and buffer)
VARIANTS = {"identity": (VT(), 1), "formant_tilt_breath_rate_1": (VT(1.1, 1.0, -2.0, 3.0), 1),
            "formant_tilt_breath_rate_0.8": (VT(1.1, 0.8, -2.0, 3.0), 2)}
TRACE_REPS = 6


def analysed(dev):
    """The rows' envelopes and aperiodicities as the resynthesis hands them to the warp, and the frames per row."""
    waves, f0s, _ = bc.make_rows()
    x = torch.from_numpy(np.concatenate(waves)).to(dev)
    lengths = [len(w) for w in waves]
    env = world.cheaptrick_ragged(x, lengths, f0s, SR, FP, fft_size=N)
    ap = world.d4c_ragged(x, lengths, f0s, SR, FP, threshold=0.0, fft_size=N)
    return env, ap, [len(f) for f in f0s]


def positions_of(t, frames, n):
    return [world.source_positions(world.warped_frames(n, HOP, t.rate), t.rate, f) for f in frames]


def trace_run(dev):
    env, ap, frames = analysed(dev)
    n = int(bc.SECONDS * SR)
    for t, _ in VARIANTS.values():                               # TRACE_REPS calls of each variant, in this order
        pos = positions_of(t, frames, n)
        for _ in range(TRACE_REPS):
            world.warp_envelopes(env, ap, pos, [t] * ROWS, SR)
    torch.cuda.synchronize()


def kernel_rows(out_csv: Path):
    prof = shutil.which("rocprofv3")
    if prof is None:
        raise SystemExit("bench_world_warp: rocprofv3 not found; kernel times are not optional")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "warp", "--",
               sys.executable, str(Path(__file__).resolve()), "--trace-run"]
        subprocess.run(cmd, check=True, timeout=600, stdout=subprocess.DEVNULL)
        stats = sorted(Path(tmp).rglob("*kernel_stats.csv"))
        trace = sorted(Path(tmp).rglob("*kernel_trace.csv"))
        if not stats or not trace:
            raise SystemExit("bench_world_warp: the profiler wrote no kernel_stats.csv / kernel_trace.csv")
        rows = list(csv.DictReader(open(stats[0])))
        events = list(csv.DictReader(open(trace[0])))
    keep = [r for r in rows if KERNEL in r.get("Name", "")]
    if not keep:
        raise SystemExit("bench_world_warp: the warp kernel does not appear in the trace")
    with open(out_csv, "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=list(keep[0].keys()))
        w.writeheader()
        w.writerows(keep)
    d = [int(e["End_Timestamp"]) - int(e["Start_Timestamp"]) for e in events if KERNEL in e.get("Kernel_Name", "")]
    if len(d) != TRACE_REPS * len(VARIANTS):
        raise SystemExit(f"bench_world_warp: {len(d)} launches of {KERNEL} in the trace")
    out = {}
    for i, name in enumerate(VARIANTS):
        part = d[i * TRACE_REPS + 2:(i + 1) * TRACE_REPS]        # the first calls carry the code load
        out[name] = {"calls": len(part), "avg_us": sum(part) / len(part) / 1e3, "min_us": min(part) / 1e3,
                     "max_us": max(part) / 1e3}
    return out


def loader_stage(dev, waves, f0s, new, reps, aperiodicity, transformed):
    """tools/bench_cheaptrick.py's stage with the block's ``aperiodicity`` set and, when ``transformed``, one drawn
    transform per resynthesis row: a collated B = 256 batch whose 64 resynthesis rows are cropped windows."""
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
        base = f0s[r].astype(np.float64)
        t, pos, n_out = None, None, n
        curve = np.asarray(new[r], np.float64)
        if transformed:
            t = VT(rng.uniform(0.85, 1.2), rng.uniform(0.8, 1.25), rng.uniform(-3.0, 3.0), rng.uniform(-3.0, 6.0))
            n_out = world.warped_length(n, t.rate)
            pos = world.source_positions(world.warped_frames(n, HOP, t.rate), t.rate, base.size)
            curve = world.time_warp_curve(curve, pos)
        curve = world.label_curve(curve, SR, N)
        crop = int(rng.integers(0, 1 + n_out // HOP - 192))
        start, count, first = md.synthetic_window(n_out, crop, HOP, 1024)
        table = world.time_base(curve, SR, FP, N)
        req = md.ResynthesisRequest("", 1.0, n, crop, start, count, first, base, curve, table.index, table.shift,
                                    table.vuv, world.noise_seed(curve), None, None if t is None else tuple(t), pos)
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


def test_records(path):
    """The ``[world_warp]`` records of the GPU test's output: accuracy ratios per configuration, tracker figures."""
    text = Path(path).read_text()
    ratios, tracked = {}, {}
    for m in re.finditer(r"\[world_warp\] (\S+) (ln sp|ap): gpu (\S+) float32 restatement (\S+) ratio (\S+)", text):
        ratios.setdefault(m[1], {})[m[2]] = {"gpu": float(m[3]), "float32": float(m[4]), "ratio": float(m[5])}
    for m in re.finditer(r"\[world_warp\] ([^:\n]+): (\d+) frames, voiced (\S+), worst (\S+) cents", text):
        tracked[m[1]] = {"frames": int(m[2]), "voiced": float(m[3]), "worst_cents": float(m[4])}
    return {"accuracy_ratios_gpu_over_float32_restatement": ratios, "tracker_worst_frame": tracked}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--no-train-step", action="store_true")
    ap.add_argument("--ratios", default=None, help="output of tests/test_world_warp_gpu.py run with -s")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "bench_world_warp.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_world_warp: no GPU visible; this benchmark does not run without one")
    dev = torch.device("cuda:0")
    if a.trace_run:
        trace_run(dev)
        return
    step_before = None if a.no_train_step else bc.training_step_ms()
    waves, f0s, new = bc.make_rows()
    n = int(bc.SECONDS * SR)
    env, d4c, frames = analysed(dev)
    res = {"rows": ROWS, "seconds_per_row": bc.SECONDS, "sample_rate": SR, "fft_size": N, "frame_period_ms": FP,
           "source_frames": sum(frames), "loader_batch": BATCH, "loader_resynthesis_rows": ROWS, "variants": {}}
    for name, (t, reads) in VARIANTS.items():
        pos = positions_of(t, frames, n)
        ms = bc.wall_ms(lambda: world.warp_envelopes(env, d4c, pos, [t] * ROWS, SR), a.reps)
        out_frames = sum(len(p) for p in pos)
        res["variants"][name] = {"transform": list(t), "output_frames": out_frames,
                                 "bytes": float(out_frames * BINS * 4 * 2 * (reads + 1)),   # sp and ap, read and written
                                 "warp_envelopes_ms_median": ms[0], "warp_envelopes_ms_min": ms[1]}
    for tag, mode in (("d4c", "d4c"), ("template_0.1", 0.1)):
        for transformed in (False, True):
            ms = loader_stage(dev, waves, f0s, new, a.reps, mode, transformed)
            key = f"loader_stage_ms_{tag}_{'transformed' if transformed else 'plain'}"
            res[key + "_median"], res[key + "_min"] = ms
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    for name, k in kernel_rows(out.with_name(out.stem + "_kernel_stats.csv")).items():
        v = res["variants"][name]
        v["kernel"] = k
        v["share_of_copy_rate"] = v["bytes"] / (k["avg_us"] * 1e-6) / 1e12 / bc.HBM_COPY_TBS
    sib = json.loads((ROOT / "profiles" / "bench_d4c.json").read_text())
    sib_us = sib["kernels"]["d4c_expand_kernel_threshold_0.0"]["avg_us"]
    res["d4c_expand_share_of_copy_rate"] = sib["frames"] * BINS * 4 / (sib_us * 1e-6) / 1e12 / bc.HBM_COPY_TBS
    if a.ratios:
        res.update(test_records(a.ratios))
    if not a.no_train_step:
        step_after = bc.training_step_ms()
        res["training_step_ms_fp32_batch256_before"], res["training_step_ms_fp32_batch256_after"] = step_before, step_after
        step = 0.5 * (step_before + step_after)
        for k in [k for k in res if k.startswith("loader_stage_ms_") and k.endswith("_median")]:
            res[k.replace("loader_stage_ms_", "stage_").replace("_median", "_to_training_step_ratio")] = res[k] / step
        res["kernel_rate_0.8_to_training_step_ratio"] = \
            res["variants"]["formant_tilt_breath_rate_0.8"]["kernel"]["avg_us"] / 1e3 / step
    out.write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

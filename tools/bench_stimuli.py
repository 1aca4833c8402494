"""Device cost of the synthesized evaluation stimuli (pitchextractor_amd.stimuli) next to the inference they feed.

Three sets at 24 kHz: the timbre notebook's grid (4 ranges x 15 frequencies x 4 profiles = 240 rows of 2.5 s), the
dynamic-pitch sets (12 vibrato rows of 3 s and the 4 glides), and a 2 000-row timbre grid.  Every stage (phase, synth,
tone, finish, reference) and the metrics kernel is called in a loop between two device events and the total is divided
by the number of calls; a call includes its host work (the output allocation, for ``reference`` the frame times and
their upload).  ``plan`` is the host-only row plan with its copy to the device.  Next to them, in the same session:
``predict_f0_batch`` on the same rows (a randomly initialised default JDCNet) and, for the two notebook sets, the host
path: the NumPy restatement (tests/stimuli_ref.py) of every row plus one upload.  Also the metrics kernel on one
24 000-frame row (its lag search is O(L^2)).  Writes profiles/bench_stimuli.json and prints the JSON line.  Needs a GPU.

Not a gate: the statement to support is what share of a sweep the stimuli cost next to the model's forward.
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from pitchextractor_amd import inference, stimuli as S  # noqa: E402
from pitchextractor_amd.model import JDCNet  # noqa: E402
from tests import stimuli_ref as R  # noqa: E402

SR = 24000


def timed_loop(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def timed(fn):
    fn()
    torch.cuda.synchronize()
    first = timed_loop(fn, 1)
    return timed_loop(fn, max(2, min(50, int(300.0 / max(first, 1e-3)))))


def timbre_rows(n_freqs_per_range):
    rows = []
    for rng in S.VOCAL_RANGES:
        for f in S.frequency_grid(rng["min_hz"], rng["max_hz"], n_freqs_per_range):
            rows += [S.timbre_row(float(f), p, 2.5, SR, timbre=name) for name, p in S.TIMBRE_PROFILES.items()]
    return rows


def dynamic_rows():
    v, g = S.VIBRATO_GRID, S.GLIDE_GRID
    rows = [S.vibrato_row(r, d, v["base_frequency_hz"], v["duration_seconds"], SR) for r in v["rates_hz"]
            for d in v["depth_cents"]]
    return rows + [S.glide_row(d, g["start_hz"], g["end_hz"], SR) for d in g["durations_seconds"]]


def host_path(rows, dev):
    """The NumPy restatement of every row, then one upload: seconds."""
    t0 = time.perf_counter()
    rng = np.random.default_rng(S.TIMBRE_STIMULUS["random_seed"])
    out = []
    for row in rows:
        if row["kind"] == S.K_TONE:
            noise = rng.standard_normal(row["n"]).astype(np.float32) if row["snr_db"] is not None else None
            pre = R.tone_prefade(row["a"], SR, row["duration"], [(h, a) for h, a in row["partials"]])
            out.append(R.finish(pre, SR, noise, row["snr_db"])[0])
        elif row["kind"] == S.K_GLIDE:
            out.append(R.synthesize_from_f0_curve(R.glide_curve(row["duration"], row["a"], row["b"], SR)[1], SR))
        else:
            out.append(R.synthesize_from_f0_curve(
                R.vibrato_curve(row["c"], row["b"], row["a"], row["duration"], SR)[1], SR))
    torch.from_numpy(np.concatenate(out)).to(dev)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def bench_set(name, rows, net, dev, host):
    pl = S.to_device(S.plan_rows(rows, SR), dev)
    res = {"rows": pl["rows"], "samples": pl["n_samples"], "pieces": pl["n_pieces"], "ms": {}}
    t0 = time.perf_counter()
    for _ in range(3):
        S.to_device(S.plan_rows(rows, SR), dev)
    torch.cuda.synchronize()
    res["ms"]["plan_host"] = (time.perf_counter() - t0) / 3 * 1e3
    noise = torch.randn((max(pl["n_noise"], 1),), dtype=torch.float32, device=dev)
    y = torch.zeros((pl["n_samples"],), dtype=torch.float32, device=dev)
    if pl["has_phases"]:
        ph = S.phase(pl, None, dev)
        res["ms"]["phase"] = timed(lambda: S.phase(pl, None, dev))
        res["ms"]["synth"] = timed(lambda: S.synth(pl, ph, y))
        del ph
    if pl["has_tones"]:
        res["ms"]["tone"] = timed(lambda: S.tone(pl, y))
    res["ms"]["finish"] = timed(lambda: S.finish(pl, y, noise))
    frames = [1 + int(n) // 300 for n in pl["lengths"]]
    res["ms"]["reference"] = timed(lambda: S.reference(pl, frames, None, dev))
    res["ms"]["stimuli_total"] = sum(v for k, v in res["ms"].items())
    del y
    st = S.build(rows, SR, noise=noise if pl["n_noise"] else None, device=dev)
    predict = lambda: inference.predict_f0_batch(net, st.audio, st.lengths, stitch="concat")  # noqa: E731
    preds = predict()
    torch.cuda.synchronize()
    res["ms"]["predict_f0_batch"] = timed_loop(predict, 2)
    refs = st.reference_f0([int(p.numel()) for p in preds])
    res["ms"]["dynamic_metrics"] = timed(lambda: S.dynamic_metrics_rows(preds, refs, dev))
    res["frames_longest_row"] = max(int(p.numel()) for p in preds)
    res["stimuli_share_of_sweep"] = res["ms"]["stimuli_total"] / (res["ms"]["stimuli_total"]
                                                                  + res["ms"]["predict_f0_batch"])
    if host:
        res["ms"]["host_numpy_plus_upload"] = host_path(rows, dev) * 1e3
    print(f"[bench_stimuli] {name}: {json.dumps(res)}", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "bench_stimuli.json"))
    ap.add_argument("--big-rows", type=int, default=2000)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_stimuli: no GPU visible; this benchmark does not run without one")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    net = JDCNet(num_class=1).to(dev).eval()
    res = {"sr": SR, "sets": {}}
    res["sets"]["timbre_grid_240"] = bench_set("timbre grid", timbre_rows(15), net, dev, host=True)
    res["sets"]["dynamic_12_vibrato_4_glide"] = bench_set("dynamic sets", dynamic_rows(), net, dev, host=True)
    res["sets"][f"timbre_grid_{args.big_rows}"] = bench_set("big grid", timbre_rows(args.big_rows // 16), net, dev,
                                                            host=False)
    # the lag search on one long row: 24 000 frames (five minutes at 12.5 ms)
    L = 24000
    ref = torch.from_numpy(R.shifted_vibrato_track(0, frames=L)).to(dev)
    pred = torch.from_numpy(R.shifted_vibrato_track(3, frames=L)).to(dev)
    S.dynamic_metrics_rows([pred], [ref], dev)
    torch.cuda.synchronize()
    res["dynamic_metrics_24000_frames_ms"] = timed_loop(lambda: S.dynamic_metrics_rows([pred], [ref], dev), 2)
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
